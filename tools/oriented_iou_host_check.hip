// Runs the arithmetic of snvc_amd/csrc/oriented_iou.hip (pair_eval<float> and pair_eval<Dual>, which are __host__ __device__) on
// the HOST, without a device: 200000 seeded pairs of both forms, kinds and enclosing types, among them all-zero input, identical
// shapes, a NaN or an infinity in one scalar, and coordinates rounded to integers (many exact ties, self-intersecting subjects).
// Each lane's vertex lists get a heap block of exactly the size the kernels give them in LDS and the last lane's column of it,
// so an index one past the end is a heap overflow that a host sanitizer reports.  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fsanitize=address,undefined \
//         -Iinclude -Isnvc_amd/csrc -o /tmp/oriented_iou_host_check tools/oriented_iou_host_check.hip snvc_amd/csrc/common.hip
//   /tmp/oriented_iou_host_check
//
// It prints the number of pairs and how many gave eight finite outputs; a sanitizer report, if any, ends the run.  Host code
// only: this is never run under a sanitizer on a GPU.
#include "../snvc_amd/csrc/oriented_iou.hip"

#include <cstdio>
#include <random>
#include <vector>

int main() {
    using namespace snvc;
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> U(-3.f, 3.f);
    long pairs = 0, finite = 0;
    for (int it = 0; it < 200000; ++it) {
        const int form = it & 1, kind = (it >> 1) & 1, enc = (it >> 2) & 1, mode = (it >> 3) % 6;
        float in[20];
        for (int i = 0; i < 20; ++i) in[i] = U(rng);
        if (mode == 1)
            for (int i = 0; i < 20; ++i) in[i] = 0.f;                                  // every point coincides
        if (mode == 2)
            for (int i = 0; i < (form == SNVC_OIOU_BOXES ? 5 : 8); ++i) in[(form == SNVC_OIOU_BOXES ? 5 : 8) + i] = in[i];   // identical
        if (mode == 3) in[it % 20] = NAN;
        if (mode == 4) in[it % 20] = INFINITY;
        if (mode == 5)
            for (int i = 0; i < 20; ++i) in[i] = std::round(in[i]);                    // exact ties, self-intersecting quadrilaterals
        std::vector<float> lf(lists_floats<float>()), ld(lists_floats<Dual>());
        float out[8];
        pair_eval<float>(Lists<float>{lf.data() + kBlock - 1}, in, form, kind, enc, out);
        Dual din[20], dout[8];
        for (int i = 0; i < 20; ++i) din[i] = {in[i], i == it % 20 ? 1.f : 0.f};
        pair_eval<Dual>(Lists<Dual>{ld.data() + kBlock - 1}, din, form, kind, enc, dout);
        bool ok = true;
        for (int k = 0; k < 8; ++k) ok = ok && std::isfinite(out[k]) && out[k] == dout[k].v;
        finite += ok;
        ++pairs;
    }
    std::printf("%ld pairs run on the host, %ld with eight finite outputs equal in both instantiations\n", pairs, finite);
    return 0;
}
