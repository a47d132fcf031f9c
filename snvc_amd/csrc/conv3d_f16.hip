// fp16-storage 3D convolution family for gfx950 (BASELINE.json configs[4]: "High-res local model ... 64ch,
// fp16 with MFMA").  The layers are the local trunk's
// (snvc/models/vernier.py:249-264: 1x1x1, 7x7x7, 5x5x5, dilated 5x5x5, 3x3x3) and the 16x hourglass's
// (snvc/models/submodule.py:223-268: 3x3x3 stride 1 / stride 2, ConvTranspose3d(k3,s2,p1,op1)).
// The reference has no fp16 path (its kernels dispatch float/double only and the model never calls .half()),
// so this mode is an extension whose parity target is this library's own fp32 path (tests/test_gpu_f16.py).
//
// Storage: activations and weights are IEEE half in HBM, products accumulate in fp32 on
// v_mfma_f32_32x32x16_f16, the per-channel affine / residual / ReLU run in fp32 on the accumulators and the
// result is rounded to half once, on the way out.
//
// Layout "C8": [N][C/8][D][H][W][8] -- eight consecutive channels of one voxel are one 16-byte piece.  That
// is the MFMA's own operand shape (a lane feeds 8 k-values = 8 channels of ONE voxel), so:
//   * staging is a plain copy: the LDS image of a chunk is [channel group][IN_D][IN_H][IN_W] pieces, filled by
//     LDS-DMA (global_load_lds_dwordx4, one piece per lane, padding pieces read a zero constant), with
//     per-VOXEL granularity -- no alignment classes along W as in the fp32 NCDHW kernels;
//   * a B fragment is ONE ds_read_b128 (32 consecutive voxels x 2 k-groups), conflict-free;
//   * the epilogue stores 16-byte pieces, 512 contiguous bytes per half-wave: the rows of the weight matrix
//     are permuted when packed so that accumulator register r of a lane is channel 16*(lane>>5) + r, i.e. a
//     lane ends up with two whole 8-channel pieces of its voxel.
// K = 16 per MFMA is either two channel groups of one tap (MODE 0: small kernels, two groups resident) or
// two TAPS of one channel group (MODE 1: 5^3 / 7^3 / stride-2 layers, whose LDS image of a single group is
// already 37-92 KB): lanes 32-63 then read the same image one tap further on, which is only a different
// (precomputed) lane base address.
// A fragments (weights) are NOT staged in LDS: a chunk of a 7^3 layer needs 343 KB of them.  Each wave streams
// them from L2 in consumption order through a small register ring (they are packed exactly in that order), so
// the chunk loop has no barrier besides the image hand-over and the LDS holds images only.
#include <type_traits>

#include "common.hpp"
#include "elementwise_internal.hpp"
#include "prep_bodies.hpp"
#include "snvc_fused.h"
#include "snvc_prep.h"
#include "snvc_dedup.h"
#include "snvc_alias.h"
#include "snvc_hgdedup.h"

namespace snvc {
namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ const unsigned g_zero16h[4] __attribute__((aligned(16))) = {0u, 0u, 0u, 0u};

struct F16Args {
    const _Float16 *x;
    const _Float16 *wp;
    const float *scale, *bias;
    const _Float16 *res;
    _Float16 *y;
    float *y_f32;        // EPI 1: [N][1][Dout][Hout][Wout] fp32 plane of output channel 0; EPI 2: [N][Cout][Dout][Hout][Wout] fp32
    // split mode (PL = 2, "f16x3"): every tensor is a pair of C8 half planes, value = hi + lo; x / res / y are the hi planes
    const _Float16 *x_lo, *res_lo;
    _Float16 *y_lo;
    const float *head;   // split EPI 0, Cout == 32: y_head[n][voxel] = sum_c head[c] * (the value written for channel c, unscaled: * head_mul)
    float *y_head;       //   fp32 plane [N][Dout][Hout][Wout] (the classifier's projection of the layer's own result, r3 side head)
    float head_mul;      //   2^-out_exp (EPI 2: applied to the fp32 result, which the epilogue forms in the residual's units)
    float res_mul;       // split residual: its stored units relative to the result's, 2^(e_y - e_res) (exact)
    int *overflow;       // split output: set to 1 if a value had to be clamped to half's range (the caller's exponent was too large)
    // EPI 4 (r5, "tail projection"): the layer's result is not stored; its contraction with a one-channel transposed layer's
    // weights W'[c][27 taps] is -- t_out[n][tap][class][pd][ph][pw] fp32 (see snvc_f16x3_deconv3d_tail_forward)
    const _Float16 *tail_w;   // [block m][8-channel group j][hi | lo][lane][8]: A fragments (32 tap rows x 16 channels), values * 2^w_exp
    float *t_out;
    float tail_mul;           // 2^-(e_y + w_exp): exact
    int64_t t_bs;             // floats between samples of t_out
    const float *res_f32;     // EPI 2 (r6): a float32 NCDHW tensor of the result's shape added to the stored result (ADD_POST; the training
                              //   step's data gradients take a skip connection's gradient this way), batch stride yf_bs; or NULL
    double *stats;            // EPI 2 (r6): per-(sample, slot, 32-channel group) fp64 (sum, sum of squares) of the stored float32 result, the layout
                              //   conv_stats_fold_kernel folds: [((n * T + slot) * groups + cg)][32][2], slot = (z-class * gridDim.x + blockIdx.x) * 4 + wave
    const float *x_mul;       // conv2d_x3q_kernel: device scalar the input pair was multiplied by (a power of two from its own maximum), or NULL
    int CGin;            // input channel groups (Cin / 8, rounded up)
    int Cout;
    int Din, Hin, Win;
    int Dout, Hout, Wout;      // dims of the OUTPUT TENSOR
    int nd, nh, nw;            // output positions this launch computes per dim (== Dout.. except for parity classes)
    int osd, osh, osw, offd, offh, offw;   // output coordinate = position * os + off
    int pad_d, pad_h, pad_w;   // image coordinate = position * STRIDE + tap * DIL - pad
    int isd, ish, iod, ioh;    // input coordinate (D, H) = image coordinate * is + io  (sub-grid classes; W is never scaled)
    int tiles_d, tiles_h, tiles_w;
    int nchunks, flags;
    int N, cls_mode;           // blockIdx.z = class * N + n.  cls_mode 0: one class; 1: the 8 parity classes of a transposed
                               // layer (own weights each); 2: the 4 (depth, height) sub-grids of a dilation-2 layer
    int64_t cls_wstride;       // halves between the packed weights of consecutive classes (cls_mode 1)
    int64_t x_bs, y_bs, r_bs, yf_bs;   // batch strides in elements
};

// The channel-interleaved float32 layout (include/snvc_fused.h): [classes][C/8][H][pitch][8] per sample, column x at lp + x.
// Float index of output channel oc (mode 0: oc = cls * C + co; mode 1: oc = co * 3 + cls) at (h, x); one definition for the
// epilogue that writes the layout, the kernel that reads it and the host test (I: int on the device, where one sample stays below
// 2^31 floats -- the launchers check that -- and 64-bit divisions would cost more than the stores).
template <class I>
__host__ __device__ __forceinline__ I il_index(int mode, I oc, I C, I H, I pitch, I lp, I cls0, I h, I x) {
    const I cls = mode ? oc % 3 : oc / C, co = mode ? oc / 3 : oc % C, groups = (C + 7) / 8;
    return ((((cls0 + cls) * groups + (co >> 3)) * H + h) * pitch + lp + x) * 8 + (co & 7);
}

// il_mode 2: the layer's rows are class-major (row r = cls * C + co, written interleaved as mode 0) while its plain result stays
// class-minor: row r goes to plane co * 3 + cls.  One definition for the epilogue and the host query (snvc_prep_plain_plane).
template <class I>
__host__ __device__ __forceinline__ I il_plain_plane(I r, I C) { return (r % C) * 3 + r / C; }

// conv2d_x3q_kernel<Cfg, 1>: the fp32 result is written a second time, channel-interleaved
struct F16IlArgs : F16Args {
    float *y_il;
    int64_t il_bs;             // floats between samples of y_il
    int il_mode, il_C, il_pitch, il_lp, il_cls0;
};

// conv3d_x3q_kernel<EPI, 1>: the image is the sheared first layer's result, formed from its 2D operands (x / x_lo are not read)
struct F16SrcArgs : F16Args {
    const float *gi;           // [N][6][CGin][Hin][pitch][8]: G (classes 0..2) and G' (3..5), zero outside the rows
    const float *p_il;         // [N][3][CGin][Hin][Win][8]: the left half's depth-class planes
    const float *v_scale, *v_bias;      // the first layer's folded affine, [8 * CGin]
    int64_t gi_bs;             // floats between samples of gi
    int v_pitch, v_lp, v_q, v_m0, v_off, v_off2, v_flags;      // v_flags: SNVC_EPI_RELU | SRC_DEDUP
};
constexpr int SRC_DEDUP = 1 << 30;      // F16SrcArgs::v_flags, internal (the C entry points refuse it): duplicate wedge tiles are not computed

// The wedge (include/snvc_dedup.h).  Left of the image's first column the sheared half of v1 reads the zero pad of gi -- a G index below
// 0 -- and on the interior planes (class 1) nothing else of v1 = f(G + P) depends on d.  Tile (d0, w0) of the 4 x 4 x 32 tiling is PURE
// when its whole input image, planes d0 - 1 .. d0 + 4 and columns w0 - 1 .. w0 + 32, lies there: all interior planes, not the last
// column (which reads G'), and the largest G index of the image -- column w0 + 32 on plane d0 - 1 -- below 0.  Pure tiles of one
// (n, th, tw) receive the same image, run the same MFMAs in the same order and store the same bits on each of their depth rows.  The
// pure d0 of a column are consecutive; the first is the representative, the others are duplicates.  One definition for the kernel
// that skips the duplicates, the kernel that copies them back, the launcher and the host query.
__host__ __device__ __forceinline__ bool wedge_tile_pure(int D, int W, int q, int m0, int off, int d0, int w0) {
    return d0 >= 2 && d0 + 3 <= D - 3 && w0 + 32 < W - 1 && q * (w0 + 32) - (d0 - 1) - m0 + off < 0;
}
__host__ __device__ __forceinline__ bool wedge_tile_duplicate(int D, int W, int q, int m0, int off, int d0, int w0) {
    return wedge_tile_pure(D, W, q, m0, off, d0, w0) && wedge_tile_pure(D, W, q, m0, off, d0 - 4, w0);
}

// Aliased duplicates (include/snvc_alias.h).  A duplicate tile's depth rows hold, bit for bit, what the representative's rows with the
// same d & 3 hold, so a reader that looks THERE needs no copy behind the producer: the duplicates' rows of the tensor are never written
// and never read.  WedgeDesc = snvc_wedge_desc: the producer's (D, W, q, m0, off); all zero aliases nothing (D - 3 < 0).
// wedge_first_pure: the representative's d0 of tile column w0 where the column has pure tiles at all -- the rule of wedge_tile_pure
// solved for d0: d0 >= 2 on the 4-grid is d0 >= 4, and q (w0 + 32) - (d0 - 1) - m0 + off < 0 is d0 >= q (w0 + 32) - m0 + off + 2.
// wedge_alias_depth(d, w) -> the plane whose row holds voxel (d, ., w)'s bits: the identity outside duplicate tiles.  No loop, one
// definition for the three readers and the host query (snvc_alias_depth) that the host test walks against wedge_tile_duplicate.
using WedgeDesc = snvc_wedge_desc;
__host__ __device__ __forceinline__ int wedge_first_pure(const WedgeDesc &g, int w0) {
    const int lo = g.q * (w0 + 32) - g.m0 + g.off + 2;
    return ((lo > 4 ? lo : 4) + 3) & ~3;
}
__host__ __device__ __forceinline__ int wedge_alias_depth(const WedgeDesc &g, int d, int w) {
    const int w0 = w & ~31, d0 = d & ~3, first = wedge_first_pure(g, w0);
    return (w0 + 32 < g.W - 1 && d0 > first && d0 + 3 <= g.D - 3) ? first + (d & 3) : d;
}
// conv3d_x3s2q_kernel<1>: the input pair's duplicate rows are read at their representative's
struct F16AliasArgs : F16Args {
    WedgeDesc in_alias;
};
// The hourglass's duplicates (include/snvc_hgdedup.h).  v2, conv2's result, at voxel (d, w) reads v1 on planes d - 1 .. d + 1 and columns
// w - 1 .. w + 1, so it is d-invariant -- v2(d) == v2(d - 4) bit for bit: same image, same MFMAs, same lane of a 4-plane tile -- where
// those all lie on the wedge: d - 1 >= 1, d + 1 <= D - 2, w + 1 < W - 1 and the largest G index, column w + 1 on plane d - 1, below 0.
// The first stride-2 layer's output tile (od0, ow0) of the 2 x 4 x 32 tiling is PURE when its whole 5 x 9 x 65 image, planes 2 od0 - 1 ..
// 2 od0 + 3 and columns 2 ow0 - 1 .. 2 ow0 + 63, lies there; it then stores what tile (od0 - 2, ow0) stores.  The pure od0 of a column are
// consecutive even numbers; the first is the representative, the others are duplicates.  g is still the PRODUCER's (D, W, q, m0, off).
// hg_first_pure: the rule solved for od0: 2 od0 - 2 > X = q (2 ow0 + 64) - m0 + off is od0 >= (X + 4) >> 1, od0 >= 2, on the 2-grid.
// hg_alias_depth(od, ow) -> the output plane whose row holds voxel (od, ., ow)'s bits: the identity outside duplicate tiles.  One
// definition for the walk that skips the duplicates (conv3d_x3s2q_kernel<2>), the reader (conv3d_x3q_kernel<0, 2>) and the host query.
__host__ __device__ __forceinline__ bool hg_tile_pure(const WedgeDesc &g, int od0, int ow0) {
    return od0 >= 2 && 2 * od0 + 4 <= g.D - 2 && 2 * ow0 + 64 < g.W - 1 && g.q * (2 * ow0 + 64) - (2 * od0 - 2) - g.m0 + g.off < 0;
}
__host__ __device__ __forceinline__ int hg_first_pure(const WedgeDesc &g, int ow0) {
    const int lo = (g.q * (2 * ow0 + 64) - g.m0 + g.off + 4) >> 1;
    return ((lo > 2 ? lo : 2) + 1) & ~1;
}
__host__ __device__ __forceinline__ int hg_alias_depth(const WedgeDesc &g, int od, int ow) {
    const int ow0 = ow & ~31, od0 = od & ~1, first = hg_first_pure(g, ow0);
    return (2 * ow0 + 64 < g.W - 1 && od0 > first && 2 * od0 + 4 <= g.D - 2) ? first + (od & 1) : od;
}
// conv3d_x3s2q_kernel<2>'s walk over the LIVE tiles of a sample.  First representatives do not fall from one tile column to the next, and
// every column's last pure tile is the same, so the duplicate columns of depth tile td are the leading k(td) ones and k steps up, one
// column at a time, then back to 0: at most HG_COLS + 2 runs of depth tiles with a constant k.  Run s holds the depth tiles from td0[s]
// on, tiles_w - k_s live tiles per row (k_s = s, and 0 for the last run), and ends at live tile cum[s] of the sample; an empty run
// repeats its predecessor's cum.  Built by hg_live_walk from hg_first_pure; shapes with more duplicate columns are not given this form.
constexpr int HG_COLS = 4;
struct HgLive { int cum[HG_COLS + 2], td0[HG_COLS + 2], live_tiles; };
// live tile u < live_tiles of a sample -> (td, th, tw): the run (a select chain over the descriptor's words -- in the kernel they are
// kernel arguments and u is wave-uniform, so all of it sits in scalar registers and nothing is fetched from memory), then the tile in it.
// One definition for the kernel and the host query (snvc_hgdedup_live_tile) that the host test walks against the predicate.
__host__ __device__ __forceinline__ void hg_live_tile(const HgLive &lv, int tiles_h, int tiles_w, int u, int &td, int &th, int &tw) {
    int base = 0, t0 = 0, k = 0;
#pragma unroll
    for (int s = 1; s < HG_COLS + 2; ++s) {
        const bool in = u >= lv.cum[s - 1];
        base = in ? lv.cum[s - 1] : base;
        t0 = in ? lv.td0[s] : t0;
        k = in ? (s == HG_COLS + 1 ? 0 : s) : k;
    }
    const int v = u - base, wl = tiles_w - k, slab = tiles_h * wl, rem = v % slab;
    td = t0 + v / slab; th = rem / wl; tw = k + rem % wl;
}
// conv3d_x3s2q_kernel<2>: <1>'s aliased read, and the duplicate tiles of the OUTPUT are no jobs of the walk (their rows stay unwritten)
struct F16LiveArgs : F16AliasArgs {
    HgLive live;
};
constexpr int SRC_NO_COPY = 1 << 29;    // F16SrcArgs::v_flags, internal, with SRC_DEDUP: no wedge_copy_kernel behind the launch (the readers alias)

// A-fragment register ring depth (k-steps ahead).  Measured on cfg5 (k7 / k5 / k3 ms): 2: 9.70 / 1.92 / 0.91;
// 4: 9.38 / 2.00 / 0.91; 6: 8.99 / 1.82 / 0.85 (242-246 VGPRs, no spills); 8: 8.89 / 1.83 / 0.86 with spills.

template <int KD_, int KH_, int KW_, int STRIDE_, int DIL_, int MI_, int TD_, int TH_, int KCG_, int MODE_, bool DB_, int OCC_,
          int DILW_ = DIL_, int PL_ = 1, bool DYN_ = false>
struct F16Cfg {
    // DYN (split transposed layers): the 2x2x2 box of a parity class is walked over its REAL taps only -- (1+pd)(1+ph)(1+pw) of
    // them, 27 over the eight classes instead of 64 -- in pairs (two taps per MFMA), their offsets held in scalar registers.
    static constexpr bool DYN = DYN_;
    // PL = 2: split mode.  Activations and weights are (hi, lo) pairs of halves, value = hi + lo (22 significant bits), and a
    // product is evaluated as hi*hi + lo_w*hi_x + hi_w*lo_x on three v_mfma_f32_32x32x16_f16 with fp32 accumulation: the fp32
    // layers' contraction at fp32 accuracy (the dropped lo*lo term is 2^-22 of the product) on the 16x faster half pipe.
    // PL = 3: split mode with the two planes of the image taken one after the other (a pass over the hi plane: lo_w*hi_x +
    // hi_w*hi_x; a pass over the lo plane: hi_w*lo_x) -- half the LDS for the layers whose image is large (stride 2).
    static constexpr int PL = PL_;
    static constexpr bool SPLIT = PL_ >= 2, SERIAL = PL_ == 3;
    static constexpr int RES_PL = PL_ == 2 ? 2 : 1;         // planes resident in LDS
    static constexpr int PASSES = SERIAL ? 2 : 1;           // image passes per channel chunk
    static constexpr int PF = DYN_ ? 2 : (SPLIT ? 3 : 6);   // A-fragment ring depth (k-steps ahead)
    // DIL applies to D and H, DILW to W (they differ only for the sub-grid form of a dilated layer, see F16K5D2)
    static constexpr int KD = KD_, KH = KH_, KW = KW_, STRIDE = STRIDE_, DIL = DIL_, DILW = DILW_, MI = MI_, TD = TD_, TH = TH_;
    static constexpr int KCG = KCG_, MODE = MODE_, OCC = OCC_;
    static constexpr bool DB = DB_;
    static constexpr int IN_D = (TD - 1) * STRIDE + (KD - 1) * DIL + 1;
    static constexpr int IN_H = (TH - 1) * STRIDE + (KH - 1) * DIL + 1;
    static constexpr int IN_W = 31 * STRIDE + (KW - 1) * DILW + 1;
    static constexpr int VOX = IN_D * IN_H * IN_W;          // pieces per channel-group image
    static constexpr int GB = VOX * 16;                     // bytes per channel-group image
    static constexpr int ITEMS = RES_PL * KCG * VOX;        // image = [plane][channel group][voxel] pieces
    static constexpr int PLANE_BYTES = KCG * GB;
    static constexpr int NIT = (ITEMS + 255) / 256;
    static constexpr int IMG_BYTES = NIT * 256 * 16;        // whole DMA rounds
    static constexpr int LDS_BYTES = IMG_BYTES * (DB ? 2 : 1);
    static constexpr int NB = TD * TH / 4;
    static constexpr bool UNROLL_D = KD <= 3;
    static constexpr int SEGS = UNROLL_D ? 1 : KD;          // runtime-looped kernel depth slices
    static constexpr int TSEG = UNROLL_D ? KD * KH * KW : KH * KW;
    static constexpr int NPS = (TSEG + 1) / 2;              // MODE 1: tap pairs per segment
    static constexpr int NS = MODE == 0 ? TSEG * (KCG / 2) : NPS * KCG;   // k-steps per segment
    static constexpr int STEPS = SEGS * NS;                 // k-steps per chunk
    static constexpr int SEG_BYTES = DIL * IN_H * IN_W * 16;
    static_assert(TD * TH % 4 == 0, "rows split over 4 waves");
    static_assert(MODE == 1 || KCG % 2 == 0, "MODE 0 pairs channel groups");
    static_assert(NIT <= 32, "validity mask is one register");
    static_assert((TD * TH / 4) * 4 == TD * TH, "whole rows per wave");
    // voxel offset of tap t of a segment (kd = 0 for looped segments)
    static constexpr int tapoff(int t) {
        const int kd = UNROLL_D ? t / (KH * KW) : 0, kh = (t / KW) % KH, kw = t % KW;
        return ((kd * DIL) * IN_H + kh * DIL) * IN_W + kw * DILW;
    }
};

// MFMA row i of a 32-channel block holds output channel 16*((i>>2)&1) + 4*(i>>3) + (i&3): accumulator register r of
// lane l (row (r&3) + 8*(r>>2) + 4*(l>>5)) is then channel 16*(l>>5) + r.
__host__ __device__ constexpr int f16_row_channel(int i) { return 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3); }

__device__ __forceinline__ int xcd_remap16(int b, int n) {
    const int q = n >> 3, r = n & 7, xcd = b & 7, k = b >> 3;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}

// The 16x16x32 form's statistics fold of 8 per-lane fp64 sums over the W lanes of an aligned lane group: a transposing butterfly.
// At xor distance o = W/2, W/4, W/8 a lane keeps one half of its values (the upper half where its bit o is set) and adds its partner's
// sums of that half; below that the one value left is added across.  v[0] of a lane with (lane & (W/8 - 1)) == 0 is then the group's
// sum of value `which` = 4 * bit(W/2) + 2 * bit(W/4) + bit(W/8) of that lane: 8 shuffles (W = 16) for 8 values instead of 32, each a
// pair of 4-byte lane exchanges.  (In conv3d_f16_kernel its selects spill: that kernel keeps the plain xor trees.)
template <int W>
__device__ __forceinline__ int stats_fold8(double (&v)[8], int lane) {
    int which = 0;
#pragma unroll
    for (int n = 4, o = W / 2; n >= 1; n >>= 1, o >>= 1) {
        const bool up = (lane & o) != 0;
        which += up ? n : 0;
#pragma unroll
        for (int k = 0; k < n; ++k) {
            const double keep = up ? v[k + n] : v[k], send = up ? v[k] : v[k + n];
            v[k] = keep + __shfl_xor(send, o, 64);
        }
    }
#pragma unroll
    for (int o = W / 16; o >= 1; o >>= 1) v[0] += __shfl_xor(v[0], o, 64);
    return which;
}

// EPI 0: C8 half output (+affine, residual, ReLU); 1: fp32 plane of channel 0 (+Sigmoid); 2: fp32 NCDHW output (split mode);
// 3: EPI 0 + the side head (split mode, one 32-channel block); 4: tail projection (split transposed layer whose ONLY consumer is a
// transposed layer to one channel: the per-voxel contraction with that layer's 27 taps is done here, on the matrix pipe)
template <class Cfg, int EPI>
__global__ void __launch_bounds__(256, Cfg::OCC)
conv3d_f16_kernel(const F16Args a_) {
    F16Args a = a_;
    // cls_mode 1 (transposed layer): blockIdx.z = (pd, ph) * N + n and the WIDTH parity is the low bit of the tile index -- the two
    // classes that write the even and the odd voxels of the same output lines (and read the same residual lines) are neighbours
    // in launch order on one XCD, so their half-line stores meet in that L2 and leave it as whole lines (r4; with all eight
    // classes on blockIdx.z the fp32-output layer of the cfg2 hourglass wrote and read every line twice: 0.223 ms)
    int cls = blockIdx.z / a.N;
    int tile_raw = blockIdx.x, tiles_launch = a.tiles_d * a.tiles_h * a.tiles_w;
    if (a.cls_mode == 1) {
        tiles_launch *= 2;
        tile_raw = xcd_remap16(blockIdx.x, tiles_launch);
        cls = (cls << 1) | (tile_raw & 1);
        tile_raw >>= 1;
        a.offd = (cls >> 2) & 1; a.offh = (cls >> 1) & 1; a.offw = cls & 1;
        a.wp += cls * a.cls_wstride;
    } else if (a.cls_mode == 2) {
        const int pd = (cls >> 1) & 1, ph = cls & 1;
        a.offd = a.iod = pd; a.offh = a.ioh = ph;
        a.nd = (a.Dout - pd + 1) / 2; a.nh = (a.Hout - ph + 1) / 2;
    }
    constexpr int S = Cfg::STRIDE, MI = Cfg::MI, TD = Cfg::TD, TH = Cfg::TH, NB = Cfg::NB, KCG = Cfg::KCG;
    constexpr int IN_H = Cfg::IN_H, IN_W = Cfg::IN_W, VOX = Cfg::VOX, GB = Cfg::GB, NIT = Cfg::NIT, ITEMS = Cfg::ITEMS;
    constexpr int PF = Cfg::PF, PL = Cfg::PL;
    constexpr bool SPLIT = Cfg::SPLIT, SERIAL = Cfg::SERIAL;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int ntiles = a.tiles_d * a.tiles_h * a.tiles_w;
    const int t = a.cls_mode == 1 ? tile_raw : xcd_remap16(blockIdx.x, ntiles);
    const int tw = t % a.tiles_w, th = (t / a.tiles_w) % a.tiles_h, td = t / (a.tiles_w * a.tiles_h);
    const int cb = blockIdx.y;              // block of 32*MI output channels
    const int64_t n = blockIdx.z % a.N;
    const int od0 = td * TD, oh0 = th * TH, ow0 = tw * 32;
    if (od0 >= a.nd || oh0 >= a.nh) return;      // a smaller class of an odd extent: whole tile outside (block-uniform)
    const int id0 = od0 * S - a.pad_d, ih0 = oh0 * S - a.pad_h, iw0 = ow0 * S - a.pad_w;

    f32x16 acc[NB][MI];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int m = 0; m < MI; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][m][r] = 0.0f;

    // ---- staging geometry: piece i of the image = (group, dd, hh, ww); its source offset (in pieces, relative to
    // the chunk's first channel group) and validity do not depend on the chunk
    const int in_hw = a.Hin * a.Win, in_dhw = in_hw * a.Din;
    unsigned off[NIT];
    unsigned vmask = 0, gmask = 0, pmask = 0;           // per piece: valid, its channel group (KCG <= 2), its plane
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = it * 256 + tid;
        const int pg = i / VOX, r = i - pg * VOX;
        const int plane = pg / KCG, g = pg - plane * KCG;
        gmask |= (unsigned)(g & 1) << it;
        pmask |= (unsigned)(plane & 1) << it;
        const int dd = r / (IN_H * IN_W), r2 = r - dd * (IN_H * IN_W);
        const int hh = r2 / IN_W, ww = r2 - hh * IN_W;
        const int gd = (id0 + dd) * a.isd + a.iod, gh = (ih0 + hh) * a.ish + a.ioh, gw = iw0 + ww;
        const bool ok = i < ITEMS && (unsigned)gd < (unsigned)a.Din && (unsigned)gh < (unsigned)a.Hin &&
                        (unsigned)gw < (unsigned)a.Win;
        off[it] = ok ? (unsigned)(g * in_dhw + gd * in_hw + gh * a.Win + gw) : 0u;
        vmask |= (ok ? 1u : 0u) << it;
    }
    static_assert(KCG <= 2, "gmask holds one bit per piece");
    const _Float16 *xn = a.x + n * a.x_bs, *xn_lo = SPLIT ? a.x_lo + n * a.x_bs : nullptr;
    const int wbase = tid & ~63;
    auto issue = [&](int pass, int buf) {           // pass = chunk (* 2 + plane when the planes are taken serially)
        const int chunk = SERIAL ? pass >> 1 : pass;
        const bool lo_pass = SERIAL && (pass & 1);
        const int64_t coff = (int64_t)chunk * KCG * in_dhw * 8;
        const int cg_left = a.CGin - chunk * KCG;
        char *const ibuf = lds + buf * Cfg::IMG_BYTES;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = it * 256 + tid;
            const bool ok = ((vmask >> it) & 1u) && (KCG == 1 || (int)((gmask >> it) & 1u) < cg_left);
            const _Float16 *xc = (((PL == 2 && ((pmask >> it) & 1u)) || lo_pass) ? xn_lo : xn) + coff;
            const void *src = ok ? static_cast<const void *>(xc + (size_t)off[it] * 8) : static_cast<const void *>(g_zero16h);
            if (ITEMS % 256 == 0 || i < ITEMS)
                __builtin_amdgcn_global_load_lds(static_cast<const float *>(src),
                                                 reinterpret_cast<float *>(ibuf + (it * 256 + wbase) * 16), 16, 0, 0);
        }
    };

    // ---- B-fragment addressing (bytes inside an image).  Lane (l & 31) = output column; lanes 32..63 feed the
    // second k-group: the next channel group (MODE 0) or the next tap (MODE 1) -- a constant added to the lane base.
    const int lanebase = (lane & 31) * S * 16;
    int rowoff[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = wave * NB + nb;
        rowoff[nb] = ((row / TH) * S * IN_H + (row % TH) * S) * IN_W * 16;
    }
    constexpr int D_SAME = Cfg::DILW;
    constexpr int D_ROW = Cfg::DIL * IN_W - (Cfg::KW - 1) * Cfg::DILW;
    constexpr int D_SLICE = Cfg::DIL * IN_H * IN_W - (Cfg::KH - 1) * Cfg::DIL * IN_W - (Cfg::KW - 1) * Cfg::DILW;
    const int b_grp = lanebase + half * GB;
    const int b_same = lanebase + half * D_SAME * 16;
    const int b_row = lanebase + half * D_ROW * 16;
    const int b_slice = lanebase + half * D_SLICE * 16;
    const int b_none = lanebase;

    // ---- A fragments: [cout block][chunk][segment][k-step][m][lane] pieces, consumed in exactly that order
    // (split mode: [..][k-step][m][hi | lo][lane])
    constexpr int MA = MI * (SPLIT ? 2 : 1);
    // DYN: this class's real taps, in (kd, kh, kw) order with kw fastest; pair p = taps (2p, 2p + 1)
    int dyn_np = 0, dyn_toff[4] = {0, 0, 0, 0}, dyn_base[4] = {0, 0, 0, 0};
    if constexpr (Cfg::DYN) {
        const int nw = 1 + (cls & 1), nh = 1 + ((cls >> 1) & 1), ndp = 1 + ((cls >> 2) & 1);
        const int T = nw * nh * ndp;
        dyn_np = T > 1 ? T / 2 : 1;
        auto vox = [&](int t) { return (((t / (nw * nh)) * IN_H) + (t / nw) % nh) * IN_W + t % nw; };
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int ta = 2 * p, tb = 2 * p + 1;
            dyn_toff[p] = vox(ta) * 16;
            dyn_base[p] = lanebase + half * ((tb < T ? vox(tb) - vox(ta) : 0) * 16);
        }
    }
    const int64_t steps_total = Cfg::DYN ? (int64_t)a.nchunks * 2 * dyn_np : (int64_t)a.nchunks * Cfg::PASSES * Cfg::STEPS;
    const h8 *wq = reinterpret_cast<const h8 *>(a.wp) + ((int64_t)cb * steps_total * MA) * 64 + lane;
    h8 q[PF][MA];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
#pragma unroll
        for (int m = 0; m < MA; ++m) q[i][m] = wq[m * 64];
        wq += MA * 64;     // the packed buffer carries PF steps of zero padding behind the last block
    }

    auto compute = [&](const char *img, bool lo_pass) {
        if constexpr (Cfg::DYN) {
            static_assert(!Cfg::DYN || (PL == 2 && KCG == 2 && Cfg::MODE == 1 && PF == 2), "DYN: resident split planes, two groups, tap pairs");
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (p >= dyn_np) break;                  // block-uniform
#pragma unroll
                for (int g = 0; g < 2; ++g) {            // k-step (p, g): ring slot g, refilled with the step two ahead
                    h8 af[MA];
#pragma unroll
                    for (int m = 0; m < MA; ++m) { af[m] = q[g][m]; q[g][m] = wq[m * 64]; }
                    wq += MA * 64;
                    h8 bf[NB], bl[NB];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        const char *src = img + g * GB + dyn_toff[p] + dyn_base[p] + rowoff[nb];
                        bf[nb] = *reinterpret_cast<const h8 *>(src);
                        bl[nb] = *reinterpret_cast<const h8 *>(src + Cfg::PLANE_BYTES);
                    }
#pragma unroll
                    for (int m = 0; m < MI; ++m) {
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m + 1], bf[nb], acc[nb][m], 0, 0, 0);
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m], bl[nb], acc[nb][m], 0, 0, 0);
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m], bf[nb], acc[nb][m], 0, 0, 0);
                    }
                }
            }
            return;
        }
        // B fragments are double-buffered in registers: the LDS reads of k-step s + 1 are issued BEFORE the MFMAs of step s (r4;
        // the compiler's own schedule sank every ds_read to just in front of its MFMA -- an exposed LDS round trip per fragment,
        // hidden only by the other waves of the SIMD: 0.76 of the pipe on the bare loop at 3 waves per SIMD, 0.64 at 2)
        constexpr int NBF = NB * (PL == 2 ? 2 : 1);
        auto step_addr = [&](int s, int &base, int &toff) {      // s is a constant after unrolling
            if constexpr (Cfg::MODE == 0) {
                const int tp = s / (KCG / 2), j = s % (KCG / 2);
                base = b_grp;
                toff = 2 * j * GB + Cfg::tapoff(tp) * 16;
            } else {
                const int g = s / Cfg::NPS, p = s % Cfg::NPS;
                const int ta = 2 * p, tb = 2 * p + 1;
                toff = g * GB + Cfg::tapoff(ta) * 16;
                if (tb >= Cfg::TSEG) base = b_none;              // odd tap count: the pair's second half has zero weights
                else {
                    const int delta = Cfg::tapoff(tb) - Cfg::tapoff(ta);
                    base = delta == D_SAME ? b_same : (delta == D_ROW ? b_row : b_slice);
                }
            }
        };
        h8 bfr[2][NBF];
        auto load_b = [&](int buf, const char *simg, int s) {
            int base, toff;
            step_addr(s, base, toff);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                bfr[buf][nb] = *reinterpret_cast<const h8 *>(simg + base + toff + rowoff[nb]);
                if constexpr (PL == 2)
                    bfr[buf][NB + nb] = *reinterpret_cast<const h8 *>(simg + Cfg::PLANE_BYTES + base + toff + rowoff[nb]);
            }
        };
        load_b(0, img, 0);
#pragma unroll 1
        for (int seg = 0; seg < Cfg::SEGS; ++seg) {
            const char *simg = img + seg * Cfg::SEG_BYTES;
#pragma unroll
            for (int s = 0; s < Cfg::NS; ++s) {
                const int cur = s & 1, nxt = cur ^ 1;
                h8 af[MA];
#pragma unroll
                for (int m = 0; m < MA; ++m) af[m] = q[0][m];
#pragma unroll
                for (int i = 0; i + 1 < PF; ++i)
#pragma unroll
                    for (int m = 0; m < MA; ++m) q[i][m] = q[i + 1][m];
                // (r5, measured and dropped: not fetching w_lo for the steps of a lo pass -- they multiply w_hi alone.  The branch
                // around two of the four loads costs the counted vmcnt waits of the ring: hg conv1 0.345 -> 0.79 ms.)
#pragma unroll
                for (int m = 0; m < MA; ++m) q[PF - 1][m] = wq[m * 64];
                wq += MA * 64;
                // the next step's fragments (behind a depth slice's last step: the first step of the next slice)
                if (s + 1 < Cfg::NS) load_b(nxt, simg, s + 1);
                else if (Cfg::SEGS > 1 && seg + 1 < Cfg::SEGS) load_b(nxt, simg + Cfg::SEG_BYTES, 0);
                __builtin_amdgcn_sched_barrier(0);          // the loads stay up here: nothing of them sinks into the MFMA block
                if constexpr (PL == 2) {
                    // the three product terms row by row: consecutive MFMAs write different accumulators (no back-to-back
                    // dependence), the two correction terms before the leading one
#pragma unroll
                    for (int m = 0; m < MI; ++m) {
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m + 1], bfr[cur][nb], acc[nb][m], 0, 0, 0);
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m], bfr[cur][NB + nb], acc[nb][m], 0, 0, 0);
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m], bfr[cur][nb], acc[nb][m], 0, 0, 0);
                    }
                } else if constexpr (SERIAL) {
#pragma unroll
                    for (int m = 0; m < MI; ++m) {
                        if (!lo_pass) {
#pragma unroll
                            for (int nb = 0; nb < NB; ++nb)
                                acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m + 1], bfr[cur][nb], acc[nb][m], 0, 0, 0);
                        }
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[2 * m], bfr[cur][nb], acc[nb][m], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < MI; ++m)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[nb][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[m], bfr[cur][nb], acc[nb][m], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (Cfg::SEGS > 1 && Cfg::NS % 2 == 1) {      // an odd number of steps: the prefetched slice start sits in buffer 1
#pragma unroll
                for (int i = 0; i < NBF; ++i) bfr[0][i] = bfr[1][i];
            }
        }
    };

    const int npass = a.nchunks * Cfg::PASSES;
    if constexpr (Cfg::DB) {
        issue(0, 0);
        __syncthreads();
        for (int ps = 0; ps < npass; ++ps) {
            if (ps + 1 < npass) issue(ps + 1, (ps + 1) & 1);
            compute(lds + (ps & 1) * Cfg::IMG_BYTES, SERIAL && (ps & 1));
            __syncthreads();     // drains the DMA of the next pass and retires every read of this pass's buffer
        }
    } else {
        for (int ps = 0; ps < npass; ++ps) {
            issue(ps, 0);
            __syncthreads();
            compute(lds, SERIAL && (ps & 1));
            __syncthreads();
        }
    }

    // ---- epilogue: lane = voxel (lane & 31) of row nb; registers r = channels 16*half + r of block m
    const int out_hw = a.Hout * a.Wout;
    const int64_t out_dhw = (int64_t)out_hw * a.Dout;
    const int pw_ = ow0 + (lane & 31);
    const bool relu = (a.flags & SNVC_EPI_RELU) != 0, add_pre = (a.flags & SNVC_EPI_ADD_PRE) != 0,
               add_post = (a.flags & SNVC_EPI_ADD_POST) != 0;
    int64_t sp[NB];
    bool okv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = wave * NB + nb;
        const int pd = od0 + row / TH, ph = oh0 + row % TH;
        okv[nb] = pd < a.nd && ph < a.nh && pw_ < a.nw;
        sp[nb] = okv[nb] ? ((int64_t)(pd * a.osd + a.offd) * out_hw + (ph * a.osh + a.offh) * a.Wout + (pw_ * a.osw + a.offw)) : 0;
    }
    if constexpr (EPI == 1) {
        // one output channel (row 0 of block 0 = register 0 of the lanes with half == 0), Sigmoid, fp32 plane
        const float sc = a.scale ? a.scale[0] : 1.0f, bi = a.scale ? a.bias[0] : 0.0f;
        float *yp = a.y_f32 + n * a.yf_bs;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float v = acc[nb][0][0] * sc + bi;
            if (relu) v = v > 0.0f ? v : 0.0f;
            if (a.flags & SNVC_EPI_SIGMOID) v = 1.0f / (1.0f + expf(-v));
            if (okv[nb] && half == 0) yp[sp[nb]] = v;
        }
    } else if constexpr (EPI == 4) {
        // The layer's result v = act(affine(acc) + residual) (64 channels per voxel, never stored) feeds ONLY a transposed layer to one
        // channel (the global stack's folded tail: classifier(bn(deconv(v)) + ...) -- reference submodule.py:127-146,166 with
        // vernier.py:366-371's composition).  That layer is out[o] = sum over (voxel i, tap k) with o = 2 i - 1 + k of T[k][i],
        // T[k][i] = sum_c W'[c][k] v[c][i]: a 27 x C contraction PER VOXEL, independent of every other voxel -- done here as three
        // half-precision MFMAs per 8-channel group on the (hi, lo) pair of v (the same split arithmetic as the layer itself; the B operand of
        // v_mfma_f32_32x32x16_f16 is exactly what a lane holds: 8 channels of one voxel).  Written: 27 fp32 planes per class instead of
        // C channels of fp32 (0.42 of the bytes at C = 64), contiguous along W inside a class (the NCDHW form stored 4 bytes at an 8-byte stride).
        static_assert(EPI != 4 || SPLIT, "tail projection: split mode");
        const _Float16 *rn = a.res ? a.res + n * a.r_bs : nullptr, *rn_lo = a.res ? a.res_lo + n * a.r_bs : nullptr;
        h8 tw[MI][2][2];
        {
            const h8 *twp = reinterpret_cast<const h8 *>(a.tail_w) + lane;
#pragma unroll
            for (int m = 0; m < MI; ++m)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) tw[m][j][s2] = twp[((m * 2 + j) * 2 + s2) * 64];
        }
        constexpr float kHalfMax = 65504.0f;
        float vmax = 0.0f;
        const int64_t cls_vox = (int64_t)a.nd * a.nh * a.nw;
        float *tn = a.t_out + n * a.t_bs + (int64_t)cls * cls_vox;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int row = wave * NB + nb;
            const int pd = od0 + row / TH, ph = oh0 + row % TH;
            f32x16 tacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) tacc[r] = 0.0f;
#pragma unroll
            for (int m = 0; m < MI; ++m) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int cj = m * 32 + 16 * half + 8 * j;
                    f32x4 sc[2], bi[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        sc[k] = a.scale ? *reinterpret_cast<const f32x4 *>(a.scale + cj + 4 * k) : f32x4(1.0f);
                        bi[k] = a.scale ? *reinterpret_cast<const f32x4 *>(a.bias + cj + 4 * k) : f32x4(0.0f);
                    }
                    h8 rv = h8((_Float16)0.0f), rl = h8((_Float16)0.0f);
                    if (rn) {
                        const int64_t gj = (int64_t)(cj >> 3) * out_dhw;
                        rv = *reinterpret_cast<const h8 *>(rn + (gj + sp[nb]) * 8);
                        rl = *reinterpret_cast<const h8 *>(rn_lo + (gj + sp[nb]) * 8);
                    }
                    h8 o, ol;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float v = __builtin_fmaf(acc[nb][m][8 * j + e], sc[e >> 2][e & 3], bi[e >> 2][e & 3]);
                        const float rr = ((float)rv[e] + (float)rl[e]) * a.res_mul;
                        if (add_pre) v += rr;
                        if (relu) v = __builtin_fmaxf(v, 0.0f);
                        if (add_post) v += rr;
                        v = __builtin_amdgcn_fmed3f(v, -kHalfMax, kHalfMax);
                        vmax = __builtin_fmaxf(vmax, okv[nb] ? __builtin_fabsf(v) : 0.0f);
                        o[e] = (_Float16)v;
                        ol[e] = (_Float16)(v - (float)o[e]);
                    }
                    tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(tw[m][j][1], o, tacc, 0, 0, 0);
                    tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(tw[m][j][0], ol, tacc, 0, 0, 0);
                    tacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(tw[m][j][0], o, tacc, 0, 0, 0);
                }
            }
            if (okv[nb]) {
                const int64_t spc = ((int64_t)pd * a.nh + ph) * a.nw + pw_;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tap = (r & 3) + 8 * (r >> 2) + 4 * half;       // accumulator row of this register
                    if (tap < 27) tn[(int64_t)tap * 8 * cls_vox + spc] = tacc[r] * a.tail_mul;
                }
            }
        }
        if (vmax >= kHalfMax && a.overflow) atomicOr(a.overflow, 1);
    } else {
        // EPI 0: C8 half output (split mode: a (hi, lo) pair); EPI 2: fp32 NCDHW output (a split-mode layer handing its result
        // to the fp32 kernels).  Residual: C8 (split mode: a pair).
        const _Float16 *rn = a.res ? a.res + n * a.r_bs : nullptr;
        const _Float16 *rn_lo = (SPLIT && a.res) ? a.res_lo + n * a.r_bs : nullptr;
        constexpr bool C8OUT = EPI == 0 || EPI == 3, side = EPI == 3 && SPLIT && MI == 1;
        _Float16 *yn = C8OUT ? a.y + n * a.y_bs : nullptr;
        _Float16 *yn_lo = (C8OUT && SPLIT) ? a.y_lo + n * a.y_bs : nullptr;
        float *yf = EPI == 2 ? a.y_f32 + n * a.yf_bs : nullptr;
        const float *__restrict__ rf = (EPI == 2 && a.res_f32) ? a.res_f32 + n * a.yf_bs : nullptr;
        constexpr float kHalfMax = 65504.0f;
        // Epilogue arithmetic is counted in VALU instructions (every one costs matrix-pipe time of the co-resident waves): the
        // affine is one FMA, ReLU and the clamp to half's range are ONE v_med3 (lower bound 0 or -65504), the overflow flag is a
        // running max of |v| compared once at the end, and the residual's conversions exist only in the with-residual instance.
        const float lo_bound = relu ? 0.0f : -kHalfMax;
        float vmax = 0.0f;
        const bool want_stats = EPI == 2 && a.stats != nullptr;
        // EPI 2 (r6): the input pair held x * x_mul[0] (a device-side power of two): taken out of the channel scale here, exactly
        const float x_inv = (EPI == 2 && a.x_mul) ? 1.0f / a.x_mul[0] : 1.0f;
        auto run = [&](auto has_res_tag) {
            constexpr bool HAS_RES = decltype(has_res_tag)::value;
#pragma unroll
            for (int m = 0; m < MI; ++m) {
                if ((cb * MI + m) * 32 >= a.Cout) break;                // Cout = 32 * odd: the last block is half empty
                const int c0 = (cb * MI + m) * 32 + 16 * half;          // first of this lane's 16 channels
                float hsum[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) hsum[nb] = 0.0f;
                // one 8-channel group (a C8 piece) at a time: its affine / head weights are live only while its pieces are formed
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int cj = c0 + 8 * j;
                    f32x4 sc[2], bi[2], hw4[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        sc[k] = (a.scale ? *reinterpret_cast<const f32x4 *>(a.scale + cj + 4 * k) : f32x4(1.0f)) * x_inv;
                        bi[k] = a.scale ? *reinterpret_cast<const f32x4 *>(a.bias + cj + 4 * k) : f32x4(0.0f);
                        if constexpr (side) hw4[k] = *reinterpret_cast<const f32x4 *>(a.head + cj + 4 * k);
                    }
                    const int64_t gj = (int64_t)(cj >> 3) * out_dhw;        // this group's plane of pieces
                    // EPI 2 with a.stats: this lane's sums over its voxels of the group's 8 channels, in fp64 from the first value on
                    // (fp32 sums lose the variance of data whose mean is large against its spread); folded per group: 32 registers
                    double st_s[8], st_q[8];
                    if constexpr (EPI == 2) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) st_s[e] = st_q[e] = 0.0;
                    }
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        h8 rv = h8((_Float16)0.0f), rl = h8((_Float16)0.0f);
                        if constexpr (HAS_RES) {
                            rv = *reinterpret_cast<const h8 *>(rn + (gj + sp[nb]) * 8);
                            if (rn_lo) rl = *reinterpret_cast<const h8 *>(rn_lo + (gj + sp[nb]) * 8);
                        }
                        h8 o, ol;
                        float rfv[8];
                        if constexpr (EPI == 2) {
                            // the float32 residual's eight values in flight together, ahead of the stores (which the compiler must
                            // otherwise keep in order with them: one exposed HBM latency per channel, measured 2x on the whole kernel)
                            if (rf && okv[nb]) {
#pragma unroll
                                for (int e = 0; e < 8; ++e) rfv[e] = rf[(int64_t)(cj + e) * out_dhw + sp[nb]];
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float v = __builtin_fmaf(acc[nb][m][8 * j + e], sc[e >> 2][e & 3], bi[e >> 2][e & 3]);
                            if constexpr (HAS_RES) {
                                const float rr = ((float)rv[e] + (float)rl[e]) * a.res_mul;
                                if (add_pre) v += rr;
                                if (relu) v = __builtin_fmaxf(v, 0.0f);
                                if (add_post) v += rr;
                            }
                            if constexpr (EPI == 2) {
                                if constexpr (!HAS_RES) { if (relu) v = __builtin_fmaxf(v, 0.0f); }
                                if (okv[nb]) {
                                    const int64_t at = (int64_t)(cj + e) * out_dhw + sp[nb];
                                    yf[at] = rf ? __builtin_fmaf(v, a.head_mul, rfv[e]) : v * a.head_mul;     // 2^-e_y: exact
                                    if (want_stats) {
                                        const double sv = (double)(v * a.head_mul);
                                        st_s[e] += sv;
                                        st_q[e] = __builtin_fma(sv, sv, st_q[e]);
                                    }
                                }
                            } else {
                                if constexpr (SPLIT) {
                                    // ReLU (when no residual follows it) and the clamp that keeps the pair finite, in one v_med3;
                                    // the flag looks at what is STORED (after the activation) and only at voxels of the tensor
                                    v = __builtin_amdgcn_fmed3f(v, HAS_RES ? -kHalfMax : lo_bound, kHalfMax);
                                    vmax = __builtin_fmaxf(vmax, okv[nb] ? __builtin_fabsf(v) : 0.0f);
                                } else if constexpr (!HAS_RES) {
                                    if (relu) v = __builtin_fmaxf(v, 0.0f);
                                }
                                if constexpr (side) hsum[nb] += hw4[e >> 2][e & 3] * v;
                                o[e] = (_Float16)v;
                                if constexpr (SPLIT) ol[e] = (_Float16)(v - (float)o[e]);
                            }
                        }
                        if constexpr (C8OUT) {
                            if (okv[nb]) {
                                *reinterpret_cast<h8 *>(yn + (gj + sp[nb]) * 8) = o;
                                if constexpr (SPLIT) *reinterpret_cast<h8 *>(yn_lo + (gj + sp[nb]) * 8) = ol;
                            }
                        }
                    }
                    if constexpr (EPI == 2) {
                        if (want_stats) {
                            // the 32 lanes of a half-wave hold the same 16 channels at 32 columns: fold them, lane 0 of the half writes its slot
                            const int zc = blockIdx.z / a.N, groups = (a.Cout + 31) >> 5;
                            const int64_t slots = (int64_t)(gridDim.z / a.N) * gridDim.x * 4;
                            const int64_t slot = ((int64_t)zc * gridDim.x + blockIdx.x) * 4 + wave;
                            double *dst = a.stats + ((((int64_t)n * slots + slot) * groups + (cb * MI + m)) * 32 + 16 * half + 8 * j) * 2;
#pragma unroll
                            for (int e = 0; e < 8; ++e) {       // plain xor trees: this form has no registers to spare for stats_fold8's selects
                                double s0 = st_s[e], s1 = st_q[e];
#pragma unroll
                                for (int o = 16; o >= 1; o >>= 1) {
                                    s0 += __shfl_xor(s0, o, 64);
                                    s1 += __shfl_xor(s1, o, 64);
                                }
                                if ((lane & 31) == 0) {
                                    dst[e * 2] = s0;
                                    dst[e * 2 + 1] = s1;
                                }
                            }
                        }
                    }
                }
                if constexpr (side) {     // the two half-waves hold channels 0..15 / 16..31 of the same 32 voxels
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        const float tot = hsum[nb] + __shfl_xor(hsum[nb], 32, 64);
                        if (okv[nb] && half == 0) a.y_head[n * out_dhw + sp[nb]] = tot * a.head_mul;
                    }
                }
            }
        };
        if (rn) run(std::true_type{});
        else run(std::false_type{});
        const bool clamped = vmax >= kHalfMax;      // a NaN never raises the flag (fmaxf drops it)
        if constexpr (C8OUT && SPLIT) {
            if (clamped && a.overflow) atomicOr(a.overflow, 1);
        }
    }
}

// ------------------------------------------------------------------------------------ 16x16x32 form of the 3x3x3 layer (r4)
// Split-mode 3x3x3 / stride-1 layer on v_mfma_f32_16x16x32_f16 instead of 32x32x16: under the chip's power limit the 16x16x32
// shape sustains 18-26 % more flops on dense random operands (a quarter of the accumulator updates per flop; tools/micro/
// mfma_power.hip).  Same tile as conv3d_f16_kernel's F16K3X (4 x 4 x 32 voxels x 32 output channels per workgroup).
//   K = 32 per MFMA = 4 k-blocks of one C8 piece: k-block kb = lane >> 4 is ONE OF FOUR TAPS of one channel group (tap 4 q + kb of the
//   27 in (kd, kh, kw) raster order: 7 quads = 28 slots, the 28th with zero weights), so a chunk is one channel group and its image
//   -- both planes, [plane][voxel] pieces, 39 KB -- is DOUBLE-BUFFERED at two workgroups per CU (2 x 78 KB);
//   B fragment (rows = k, 16 voxels): lane (voxel lane & 15, kb) reads ONE piece -- 16 voxels of the row's left or right half;
//   A fragment (16 output channels x 32 k): row i of co-half h is channel 8 * (i >> 2) + 4 * h + (i & 3) of the block, so that
//   lane (kb, voxel) ends up with accumulator rows 4 kb .. 4 kb + 3 of both halves = the 8 channels of C8 group kb: one piece.
//   Per k-step (a tap quad): 4 A fragments (2 halves x hi | lo), 16 B fragments (4 rows x 2 halves of the row x hi | lo, fetched
//   in two half-steps of 8), 48 MFMAs (16 cycles each).
// (First form, measured and replaced: two taps x two channel groups per MFMA -- an 80 KB image, single-buffered, whose refills cost
// 10 % of conv2: 0.838 ms against 0.818 for this one; profiles/r4/kernel_experiments_r4.txt items 16-18.)
// How the refill overlaps the MFMAs -- three facts about the toolchain and the hardware decide the shape of the loop:
//   * the backend drains every LDS-DMA in flight (s_waitcnt vmcnt(0)) in front of the first ds_read that follows one: it cannot tell
//     the two buffers apart (the DMA intrinsic carries no alias scope; __restrict__ does not reach it).  So the B-fragment reads are
//     inline-asm ds_read_b128 with hand-counted lgkmcnt waits: the 8 reads of half-step hs + 1 are issued in front of the MFMAs of
//     half-step hs, whose own 8 reads are then exactly what `lgkmcnt(8)` waits for; the wait names the registers as in/out operands
//     so that no MFMA moves in front of it;
//   * with an LDS-DMA in flight, every compiler-placed vmcnt wait is vmcnt(0) (the DMA is a FLAT-class access to two address spaces:
//     "pending flat");
//   * vmcnt retires in order anyway: waiting for a weight fragment issued after a DMA waits for that DMA.
//   So the DMA of the next chunk is issued LATE -- in front of k-step FILL_STEP of 7, after a forced wait for the weight fragments
//   still in flight -- and no register load issued after it is consumed before the barrier that ends the chunk (FILL_STEP = 7 - PF):
//   the refill has the last PF k-steps of MFMAs to land in.
typedef float f32x4q __attribute__((ext_vector_type(4)));
typedef _Float16 h4q __attribute__((ext_vector_type(4)));

struct X3QCfg {
    static constexpr int TD = 4, TH = 4, NB = 4, IN_D = 6, IN_H = 6, IN_W = 34, VOX = IN_D * IN_H * IN_W, GB = VOX * 16;
    static constexpr int ITEMS = 2 * VOX, PLANE_BYTES = GB, NIT = (ITEMS + 255) / 256;
    static constexpr int IMG_BYTES = NIT * 256 * 16, LDS_BYTES = 2 * IMG_BYTES;
    static constexpr int NQ = 7, PF = 2, FILL_STEP = NQ - PF;      // a fragment fetched at k-step s is consumed at s + PF
};

template <int IMM>
__device__ __forceinline__ void lds_read_b128_to(h8 &v, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(IMM) : "memory");
}

template <int N>
__device__ __forceinline__ void wait_lgkm_for(h8 (&b)[8]) {
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7])
                 : "n"(N)
                 : "memory");
}

// SRC 1 (the fused sheared first layer): nothing is fetched by DMA -- the workgroup FORMS the next chunk's image, the first layer's
// result v1 = med3(fma(G + P, scale, bias)) as a split pair, and writes it into the other buffer with ds_write_b128, piece by piece
// where the DMA would have put it.  Thread t < 204 owns image column (hh, ww) = (t / 34, t % 34) and walks its 6 depth positions in
// twelve HALF pieces (4 channels of one plane): half piece j is formed among the first MFMAs of half-step j + 1 from the 16 bytes of
// G (whose index drops by one per plane) and 16 of P (both channel-interleaved) fetched behind half piece j - 1's arithmetic in
// half-step j, into the same registers; the second half completes the pair and writes it.  The scale sits in scalar registers.
// Threads 204..255 repeat columns 0..51 (the same values to the same addresses: no divergence).  Nothing depends on the lane's
// voxel being inside the tensor: coordinates are clamped into it (every address is that of a voxel of the tensor; gi is zero around
// its rows, so an out-of-range G index reads the 0 the expand pass substitutes), and a voxel outside gets med3's bounds (0, 0): a
// zero piece.  The arithmetic is sheared_expand_split_kernel's `emit`, operation for operation.
template <int SRC, class A>
__device__ __forceinline__ const F16SrcArgs &src_args_of(const A &a) {
    if constexpr (SRC == 1) return a;
    else return *reinterpret_cast<const F16SrcArgs *>(&a);
}

// SRC 2 (include/snvc_hgdedup.h): the input pair is the hourglass's first stride-2 layer's, written without its duplicate tiles
// (a.in_alias, the descriptor of THAT layer's input): a piece of such a row is fetched from the representative's plane -- whole 128-byte
// lines of another plane, decided once per workgroup in the fill geometry and nowhere else.
template <int EPI, int SRC = 0>      // EPI 0: split C8 output; 3: + the side head (Cout == 32); 2 (r6): float32 NCDHW output (+ float32 residual, + statistics)
__global__ void __launch_bounds__(256, 2)
conv3d_x3q_kernel(const std::conditional_t<SRC == 1, F16SrcArgs, std::conditional_t<SRC == 2, F16AliasArgs, F16Args>> a) {
    using Cfg = X3QCfg;
    constexpr int NB = Cfg::NB, TH = Cfg::TH, IN_H = Cfg::IN_H, IN_W = Cfg::IN_W, VOX = Cfg::VOX, NIT = Cfg::NIT, NQ = Cfg::NQ;
    constexpr int ITEMS = Cfg::ITEMS, PF = Cfg::PF;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kb = lane >> 4, col = lane & 15;
    // the output-channel blocks of a tile are consecutive jobs of the same XCD: the second reads the tile's input from that XCD's L2
    // (as separate grid rows -- blockIdx.y -- the 64 -> 64 hourglass layer fetched its input twice: 299 MB against 159)
    const int ntiles = a.tiles_d * a.tiles_h * a.tiles_w, cblocks = a.Cout >> 5;
    const int job = xcd_remap16(blockIdx.x, ntiles * cblocks);
    const int t = job / cblocks, cb = job - t * cblocks;
    const int tw = t % a.tiles_w, th = (t / a.tiles_w) % a.tiles_h, td = t / (a.tiles_w * a.tiles_h);
    const int64_t n = blockIdx.z;
    const int od0 = td * Cfg::TD, oh0 = th * TH, ow0 = tw * 32;
    const int id0 = od0 - a.pad_d, ih0 = oh0 - a.pad_h, iw0 = ow0 - a.pad_w;
    if constexpr (SRC == 1) {      // block-uniform, in front of every LDS access and barrier: wedge_copy_kernel stores this tile behind the launch
        if ((a.v_flags & SRC_DEDUP) && wedge_tile_duplicate(a.Din, a.Win, a.v_q, a.v_m0, a.v_off, od0, ow0)) return;
    }

    f32x4q acc[NB][2][2];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[nb][ph][h] = f32x4q{0.0f, 0.0f, 0.0f, 0.0f};

    const int in_hw = a.Hin * a.Win, in_dhw = in_hw * a.Din;
    unsigned off[NIT];
    unsigned vmask = 0, pmask = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = it * 256 + tid;
        const int plane = i / VOX, r = i - plane * VOX;
        pmask |= (unsigned)(plane & 1) << it;
        const int dd = r / (IN_H * IN_W), r2 = r - dd * (IN_H * IN_W);
        const int hh = r2 / IN_W, ww = r2 - hh * IN_W;
        const int gd = id0 + dd, gh = ih0 + hh, gw = iw0 + ww;
        const bool ok = i < ITEMS && (unsigned)gd < (unsigned)a.Din && (unsigned)gh < (unsigned)a.Hin && (unsigned)gw < (unsigned)a.Win;
        int sd = gd;      // the plane that holds the piece
        if constexpr (SRC == 2) sd = hg_alias_depth(a.in_alias, gd, gw);
        off[it] = ok ? (unsigned)(sd * in_hw + gh * a.Win + gw) : 0u;
        vmask |= (ok ? 1u : 0u) << it;
    }
    const _Float16 *xn = a.x + n * a.x_bs, *xn_lo = a.x_lo + n * a.x_bs;
    const int wbase = tid & ~63;
    auto issue = [&](int chunk, int buf) {     // every wave issues all NIT instructions (pieces past the image land in the buffer's padding)
        const int64_t coff = (int64_t)chunk * in_dhw * 8;
        char *const ibuf = lds + buf * Cfg::IMG_BYTES;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const _Float16 *xc = (((pmask >> it) & 1u) ? xn_lo : xn) + coff;
            const void *src = ((vmask >> it) & 1u) ? static_cast<const void *>(xc + (size_t)off[it] * 8) : static_cast<const void *>(g_zero16h);
            __builtin_amdgcn_global_load_lds(static_cast<const float *>(src), reinterpret_cast<float *>(ibuf + (it * 256 + wbase) * 16), 16, 0, 0);
        }
    };
    int qoff[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        int tp = 4 * q + kb;
        tp = tp < 27 ? tp : 26;                     // the 28th slot: zero weights, tap 26's piece
        qoff[q] = (((tp / 9) * IN_H + (tp / 3) % 3) * IN_W + tp % 3 + col) * 16;
    }
    int rowoff[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = wave * NB + nb;
        rowoff[nb] = ((row / TH) * IN_H + (row % TH)) * IN_W * 16;
    }
    const int64_t steps_total = (int64_t)a.nchunks * NQ;
    const h8 *wq = reinterpret_cast<const h8 *>(a.wp) + ((int64_t)cb * steps_total * 4) * 64 + lane;
    const int c0 = cb * 32 + 8 * kb;               // first of this lane's 8 output channels
    const bool has_aff = a.scale != nullptr;       // decided once: the epilogue's constants are fetched inside the last chunk
    h8 q_[PF][4];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
#pragma unroll
        for (int m = 0; m < 4; ++m) q_[i][m] = wq[m * 64];
        wq += 4 * 64;
    }

    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)lds;
    // SRC 1: the state of this thread's image column (see the head comment); untouched, and removed, with SRC 0
    constexpr int COLS = IN_H * IN_W;
    const F16SrcArgs &aa = src_args_of<SRC>(a);      // SRC 0: never read
    struct {
        unsigned g_off, p_off, w_off, g_slab, p_slab;      // bytes
        float hi, lo, vmax;
        const char *gb, *pb;
        f32x4q g, p, bi[2];      // the operands of one half piece (4 channels); the channel group's bias
        float sc[8];             // the channel group's scale: uniform, held in scalar registers
        h4q chi, clo;            // the first half piece, until the second completes the pair
    } pr{};
    auto prod_setup = [&]() {
        const int cid = tid < COLS ? tid : tid - COLS;
        const int hh = cid / IN_W, ww = cid - hh * IN_W;
        const int gh = ih0 + hh, gw = iw0 + ww;
        const bool col_ok = (unsigned)gh < (unsigned)aa.Hin && (unsigned)gw < (unsigned)aa.Win;
        const int ghc = gh < 0 ? 0 : (gh < aa.Hin ? gh : aa.Hin - 1), gwc = gw < 0 ? 0 : (gw < aa.Win ? gw : aa.Win - 1);
        const bool last = gwc == aa.Win - 1;
        const int i0 = last ? aa.v_q * (aa.Win - 1) - aa.v_m0 + aa.v_off2 : aa.v_q * gwc - aa.v_m0 + aa.v_off;      // the G | G' index at d = 0
        pr.g_off = (unsigned)((((last ? 3 * aa.CGin : 0) * aa.Hin + ghc) * aa.v_pitch + aa.v_lp + i0) * 32);
        pr.p_off = (unsigned)((ghc * aa.Win + gwc) * 32);
        pr.g_slab = (unsigned)(aa.Hin * aa.v_pitch * 32);
        pr.p_slab = (unsigned)(aa.Hin * aa.Win * 32);
        pr.w_off = (unsigned)(cid * 16);
        pr.hi = col_ok ? 65504.0f : 0.0f;
        pr.lo = (col_ok && !(aa.v_flags & SNVC_EPI_RELU)) ? -65504.0f : 0.0f;
        pr.gb = reinterpret_cast<const char *>(aa.gi + n * aa.gi_bs);
        pr.pb = reinterpret_cast<const char *>(aa.p_il + n * 3 * (int64_t)aa.CGin * aa.Hin * aa.Win * 8);
    };
    auto prod_affine = [&](int group) {      // per-lane loads of a uniform address: no scalar load enters the hand-counted loop
        int z = 0;
        asm volatile("" : "+v"(z));
        const f32x4q *s = reinterpret_cast<const f32x4q *>(aa.v_scale + group * 8 + z), *b = reinterpret_cast<const f32x4q *>(aa.v_bias + group * 8 + z);
        const f32x4q s0 = s[0], s1 = s[1];
        pr.bi[0] = b[0]; pr.bi[1] = b[1];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            pr.sc[e] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, e < 4 ? s0[e & 3] : s1[e & 3])));
    };
    // half piece j = 2 dd + half: channels 4 half .. 4 half + 3 of plane dd of the column
    auto prod_load = [&](int group, int j) {
        const int gd = id0 + (j >> 1);
        const int gdc = gd < 0 ? 0 : (gd < aa.Din ? gd : aa.Din - 1);
        const int cls = gdc == aa.Din - 1 ? 2 : (gdc == 0 ? 0 : 1);
        const unsigned slab = (unsigned)(cls * aa.CGin + group);
        pr.g = *reinterpret_cast<const f32x4q *>(pr.gb + (pr.g_off + (slab * pr.g_slab - (unsigned)gdc * 32u + 16u * (j & 1))));
        pr.p = *reinterpret_cast<const f32x4q *>(pr.pb + (pr.p_off + (slab * pr.p_slab + 16u * (j & 1))));
    };
    auto prod_form = [&](int buf, int j) {
        const int dd = j >> 1, half = j & 1;
        const bool d_ok = (unsigned)(id0 + dd) < (unsigned)aa.Din;
        const float hb = d_ok ? pr.hi : 0.0f, lb = d_ok ? pr.lo : 0.0f;
        h4q o, ol;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = __builtin_fmaf(pr.g[e] + pr.p[e], pr.sc[4 * half + e], pr.bi[half][e]);
            const float tc = __builtin_amdgcn_fmed3f(t, lb, hb);
            pr.vmax = __builtin_fmaxf(pr.vmax, __builtin_fabsf(tc));
            o[e] = (_Float16)tc;
            ol[e] = (_Float16)(tc - (float)o[e]);
        }
        if (half == 0) {
            pr.chi = o;
            pr.clo = ol;
        } else {
            char *const dst = lds + pr.w_off + buf * Cfg::IMG_BYTES + dd * (COLS * 16);
            *reinterpret_cast<h8 *>(dst) = __builtin_shufflevector(pr.chi, o, 0, 1, 2, 3, 4, 5, 6, 7);
            *reinterpret_cast<h8 *>(dst + Cfg::PLANE_BYTES) = __builtin_shufflevector(pr.clo, ol, 0, 1, 2, 3, 4, 5, 6, 7);
        }
    };
    constexpr int NHP = 2 * Cfg::IN_D;      // half pieces per column and chunk
    if constexpr (SRC == 1) {
        prod_setup();
        prod_affine(0);
#pragma unroll
        for (int j = 0; j < NHP; ++j) {
            prod_load(0, j);
            prod_form(0, j);
        }
    } else {
        issue(0, 0);
    }
    __syncthreads();
    // The LAST chunk is a copy of the loop body of its own (LAST is a constant in it): it has no next chunk to fetch fragments for, so
    // from k-step FILL_STEP on it requests nothing of the weights (they were 8 KB of the next block's fragments or padding per wave,
    // loaded for nothing) and, at FILL_STEP, the epilogue's per-channel constants instead -- 16-byte loads into the registers the ring
    // has just given up, which land under the last two k-steps.  Fetched behind the last barrier, one dword at a time, they cost every
    // tile an exposed L2 round trip.  (As a branch inside ONE loop body the ring's hand-over across the branch became register copies
    // of loads in flight, i.e. a vmcnt(0) in front of k-step FILL_STEP + 1 that waited for the refill.)
    h8 epc[6];         // scale[0..3], scale[4..7], bias[0..3], bias[4..7], head[0..3], head[4..7] of this lane's 8 channels
    auto run_chunk = [&](const int chunk, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        const unsigned img = lds_base + (unsigned)((chunk & 1) * Cfg::IMG_BYTES);
        h8 bfr[2][8];      // [buffer][(row of the half-step) * 4 + (row half) * 2 + plane]
        auto load_b = [&](int buf, int hs) {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const unsigned addr = img + (unsigned)(qoff[hs >> 1] + rowoff[2 * (hs & 1) + rr]);
                lds_read_b128_to<0>(bfr[buf][rr * 4 + 0], addr);
                lds_read_b128_to<Cfg::PLANE_BYTES>(bfr[buf][rr * 4 + 1], addr);
                lds_read_b128_to<256>(bfr[buf][rr * 4 + 2], addr);
                lds_read_b128_to<Cfg::PLANE_BYTES + 256>(bfr[buf][rr * 4 + 3], addr);
            }
        };
        load_b(0, 0);
        h8 af[4];
#pragma unroll
        for (int hs = 0; hs < 2 * NQ; ++hs) {
            const int cur = hs & 1, nx = cur ^ 1;
            if ((hs & 1) == 0) {
                if (hs == 2 * Cfg::FILL_STEP) {
                    // every weight fragment in flight lands first: none is waited for between here and the barrier
#pragma unroll
                    for (int i = 0; i < PF; ++i) asm volatile("" ::"v"(q_[i][0]), "v"(q_[i][1]), "v"(q_[i][2]), "v"(q_[i][3]));
                    if constexpr (!LAST && SRC != 1) issue(chunk + 1, (chunk + 1) & 1);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) af[m] = q_[0][m];
#pragma unroll
                for (int i = 0; i + 1 < PF; ++i)
#pragma unroll
                    for (int m = 0; m < 4; ++m) q_[i][m] = q_[i + 1][m];
                if constexpr (!LAST && SRC == 1) {      // once per chunk: the next channel group's affine
                    if (hs == 0) prod_affine(chunk + 1);
                }
                if constexpr (!LAST) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) q_[PF - 1][m] = wq[m * 64];      // from k-step FILL_STEP on: fragments of the NEXT chunk
                    wq += 4 * 64;
                } else if (hs < 2 * Cfg::FILL_STEP) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) q_[PF - 1][m] = wq[m * 64];
                    wq += 4 * 64;
                } else if (hs == 2 * Cfg::FILL_STEP) {
                    if (has_aff) {       // block-uniform, decided once
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            epc[k] = *reinterpret_cast<const h8 *>(a.scale + c0 + 4 * k);
                            epc[2 + k] = *reinterpret_cast<const h8 *>(a.bias + c0 + 4 * k);
                        }
                    }
                    if constexpr (EPI == 3) {
#pragma unroll
                        for (int k = 0; k < 2; ++k) epc[4 + k] = *reinterpret_cast<const h8 *>(a.head + c0 + 4 * k);
                    }
                }
            }
            if (hs + 1 < 2 * NQ) {
                load_b(nx, hs + 1);
                wait_lgkm_for<8>(bfr[cur]);
            } else {
                wait_lgkm_for<0>(bfr[cur]);
            }
            __builtin_amdgcn_sched_barrier(0);
            // SRC 1: half piece hs - 1 of the next image is formed among this half-step's MFMAs from the operands fetched in the last one, then
            // half piece hs's operands are fetched into the same registers; a completed pair is written behind the wait above, in front of
            // the next half-step's reads: `lgkmcnt(8)` there still names exactly the 8 reads issued last
            constexpr bool FORM = !LAST && SRC == 1;
            if constexpr (FORM) {
                if (hs >= 1 && hs <= NHP) prod_form((chunk + 1) & 1, hs - 1);
                if (hs < NHP) prod_load(chunk + 1, hs);
            }
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const h8 aw = term == 0 ? af[2 * h + 1] : af[2 * h];
                            const h8 bx = bfr[cur][rr * 4 + ph * 2 + (term == 1 ? 1 : 0)];
                            acc[2 * (hs & 1) + rr][ph][h] =
                                __builtin_amdgcn_mfma_f32_16x16x32_f16(aw, bx, acc[2 * (hs & 1) + rr][ph][h], 0, 0, 0);
                        }
            if constexpr (FORM) {
                if (hs >= 1 && hs <= NHP) {
#pragma unroll
                    for (int k = 0; k < 12; ++k) {      // the VALU work between the first MFMAs, the fetches behind it, the rest of the MFMAs under them
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();     // drains the DMA of the next chunk and retires every read (SRC 1: every write) of the buffers
    };
    for (int chunk = 0; chunk + 1 < a.nchunks; ++chunk) run_chunk(chunk, std::false_type{});
    run_chunk(a.nchunks - 1, std::true_type{});
    if constexpr (SRC == 1) {      // the expand pass's flag: a stored |v1| at half's limit (halo voxels are other tiles' own: same OR)
        if (pr.vmax >= 65504.0f && a.overflow) atomicOr(a.overflow, 1);
    }
    // the constants are waited for HERE, in front of the first store: a value first read behind a store (the compiler sinks the side
    // head's sum there) is waited for with vmcnt(0), i.e. until the wave's own stores are acknowledged
    if (has_aff) asm volatile("" ::"v"(epc[0]), "v"(epc[1]), "v"(epc[2]), "v"(epc[3]));
    if constexpr (EPI == 3) asm volatile("" ::"v"(epc[4]), "v"(epc[5]));

    const int out_hw = a.Hout * a.Wout;
    const int64_t out_dhw = (int64_t)out_hw * a.Dout;
    const bool relu = (a.flags & SNVC_EPI_RELU) != 0;
    float sc[8], bi[8], hw8[8];
    const float x_inv = (EPI == 2 && a.x_mul) ? 1.0f / a.x_mul[0] : 1.0f;      // see conv3d_f16_kernel's EPI 2
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = (has_aff ? __builtin_bit_cast(f32x4q, epc[e >> 2])[e & 3] : 1.0f) * x_inv;
        bi[e] = has_aff ? __builtin_bit_cast(f32x4q, epc[2 + (e >> 2)])[e & 3] : 0.0f;
        hw8[e] = (EPI == 3) ? __builtin_bit_cast(f32x4q, epc[4 + (e >> 2)])[e & 3] : 0.0f;
    }
    if constexpr (EPI == 2) {
        // the training step's layers (r6): lane (kb, col) stores its 8 channels of 16 consecutive voxels as float32 NCDHW (64-byte runs per
        // channel), adds the float32 residual (a skip connection's gradient), and leaves the statistics of what it stored -- per wave and
        // 32-channel group, the layout conv_stats_fold_kernel folds (slot = tile * 4 + wave)
        float *yf = a.y_f32 + n * a.yf_bs + (int64_t)c0 * out_dhw;
        const float *__restrict__ rf = a.res_f32 ? a.res_f32 + n * a.yf_bs + (int64_t)c0 * out_dhw : nullptr;
        const bool want_stats = a.stats != nullptr;
        double st_s[8], st_q[8];           // in fp64 from the first value on, as conv3d_f16_kernel's EPI 2
#pragma unroll
        for (int e = 0; e < 8; ++e) st_s[e] = st_q[e] = 0.0;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int row = wave * NB + nb;
            const int pd = od0 + row / TH, phh = oh0 + row % TH;
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                const int pw = ow0 + 16 * ph + col;
                const bool ok = pd < a.nd && phh < a.nh && pw < a.nw;
                const int64_t sp = ok ? ((int64_t)pd * out_hw + phh * a.Wout + pw) : 0;
                float rfv[8];
                if (rf && ok) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) rfv[e] = rf[(int64_t)e * out_dhw + sp];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = __builtin_fmaf(acc[nb][ph][e >> 2][e & 3], sc[e], bi[e]);
                    if (relu) v = __builtin_fmaxf(v, 0.0f);
                    const float sv = v * a.head_mul;
                    if (ok) {
                        yf[(int64_t)e * out_dhw + sp] = rf ? sv + rfv[e] : sv;
                        if (want_stats) {
                            st_s[e] += (double)sv;
                            st_q[e] = __builtin_fma((double)sv, (double)sv, st_q[e]);
                        }
                    }
                }
            }
        }
        if (want_stats) {
            const int groups = a.Cout >> 5;
            double *dst = a.stats + ((((int64_t)n * ntiles * 4 + (int64_t)t * 4 + wave) * groups + cb) * 32 + 8 * kb) * 2;
            const int e = stats_fold8<16>(st_s, lane);            // over the 16 columns of this k-block's lanes
            stats_fold8<16>(st_q, lane);
            if ((col & 1) == 0) {
                dst[e * 2] = st_s[0];
                dst[e * 2 + 1] = st_q[0];
            }
        }
        return;
    }
    _Float16 *yn = a.y + n * a.y_bs + (int64_t)(cb * 4 + kb) * out_dhw * 8;
    _Float16 *yn_lo = a.y_lo + n * a.y_bs + (int64_t)(cb * 4 + kb) * out_dhw * 8;
    constexpr float kHalfMax = 65504.0f;
    const float lo_bound = relu ? 0.0f : -kHalfMax;
    float vmax = 0.0f;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = wave * NB + nb;
        const int pd = od0 + row / TH, phh = oh0 + row % TH;
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
            const int pw = ow0 + 16 * ph + col;
            const bool ok = pd < a.nd && phh < a.nh && pw < a.nw;
            const int64_t sp = ok ? ((int64_t)pd * out_hw + phh * a.Wout + pw) : 0;
            h8 o, ol;
            float hsum = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = __builtin_fmaf(acc[nb][ph][e >> 2][e & 3], sc[e], bi[e]);
                v = __builtin_amdgcn_fmed3f(v, lo_bound, kHalfMax);
                vmax = __builtin_fmaxf(vmax, ok ? __builtin_fabsf(v) : 0.0f);      // what is stored (after the ReLU), inside the tensor
                if constexpr (EPI == 3) hsum += hw8[e] * v;
                o[e] = (_Float16)v;
                ol[e] = (_Float16)(v - (float)o[e]);
            }
            if (ok) {
                *reinterpret_cast<h8 *>(yn + sp * 8) = o;
                *reinterpret_cast<h8 *>(yn_lo + sp * 8) = ol;
            }
            if constexpr (EPI == 3) {
                float tot = hsum + __shfl_xor(hsum, 16, 64);
                tot += __shfl_xor(tot, 32, 64);
                if (ok && kb == 0) a.y_head[n * out_dhw + sp] = tot * a.head_mul;
            }
        }
    }
    if (vmax >= kHalfMax && a.overflow) atomicOr(a.overflow, 1);
}

// The COPY route of the wedge (snvc_dedup_fused_first_conv3d_forward: the caller sees a fully populated tensor).  GlobalStack's step no
// longer takes it where both readers of conv2's results can alias (SRC_NO_COPY, include/snvc_alias.h: conv3d_x3s2q_kernel<1> and
// deconv_tail_gather_alias_kernel read the representative's rows, this launch and its 33 MB of stores are gone); it remains for every
// other reader -- another stride-2 form, the unfused tail, a caller of the C entry point.
// Behind conv3d_x3q_kernel<EPI, 1> with SRC_DEDUP, on its stream: the duplicate wedge tiles it returned from.  Workgroup = one
// duplicate tile (tw, td) of one (n, th): ONE depth row of the column's representative tile -- both planes, every channel group, the
// tile's rows inside the tensor, 32 columns, and the side head's row -- is read (16.5 KB at 32 channels) and stored to the tile's four
// depth rows (one row per workgroup -- four times the loads -- measured slower: profiles/wedge_dedup/copy_kernel_variants.txt).  16-byte loads and stores only: a C8 piece is 16 bytes; the side head's rows are
// 16-byte aligned because the launcher asks W % 4 == 0 of a deduplicated launch.  The grid spans the duplicate range of tile column 0,
// the widest (wedge_tile_pure is monotone in w0): workgroups of narrower columns' non-duplicates return.
struct WedgeCopyArgs {
    _Float16 *y, *y_lo;
    float *y_head;             // or NULL
    int64_t y_bs;              // halves between samples of y / y_lo
    int CG, D, H, W, q, m0, off;
    int td0, ntw;              // first duplicate depth tile of column 0; tile columns with duplicates
};

__global__ void __launch_bounds__(256)
wedge_copy_kernel(const WedgeCopyArgs a) {
    const int tw = blockIdx.x % a.ntw, td = a.td0 + blockIdx.x / a.ntw;
    const int d0 = td * X3QCfg::TD, w0 = tw * 32, h0 = blockIdx.y * X3QCfg::TH;
    if (!wedge_tile_duplicate(a.D, a.W, a.q, a.m0, a.off, d0, w0)) return;      // block-uniform
    int rep = d0 - X3QCfg::TD;
    while (wedge_tile_pure(a.D, a.W, a.q, a.m0, a.off, rep - X3QCfg::TD, w0)) rep -= X3QCfg::TD;
    const int64_t n = blockIdx.z, hw = (int64_t)a.H * a.W, dhw = hw * a.D;
    const int tid = threadIdx.x;
    // item = ((plane * CG + group) * 4 + row) * 32 + column: 256 items are two channel groups' rows, CG / 2 rounds per plane
    const int col = tid & 31, h = h0 + ((tid >> 5) & 3);
    const int rounds = 2 * a.CG * 128 / 256;
    if (h < a.H) {
        for (int r0 = 0; r0 < rounds; r0 += 4) {
            uint4 *p[4];
            uint4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int g = 2 * (r0 + k) + (tid >> 7);      // plane * CG + group
                const bool on = r0 + k < rounds;
                const int plane = on ? g / a.CG : 0, cg = on ? g - plane * a.CG : 0;
                p[k] = reinterpret_cast<uint4 *>((plane ? a.y_lo : a.y) + n * a.y_bs) + (cg * dhw + (int64_t)h * a.W + w0 + col);
                if (on) v[k] = p[k][rep * hw];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (r0 + k < rounds) {
#pragma unroll
                    for (int r = 0; r < X3QCfg::TD; ++r) p[k][(d0 + r) * hw] = v[k];
                }
            }
        }
    }
    if (a.y_head && tid < 32) {
        const int hh = h0 + (tid >> 3);
        if (hh < a.H) {
            uint4 *p = reinterpret_cast<uint4 *>(a.y_head + n * dhw + (int64_t)hh * a.W + w0) + (tid & 7);
            const uint4 v = p[rep * hw / 4];
#pragma unroll
            for (int r = 0; r < X3QCfg::TD; ++r) p[(d0 + r) * hw / 4] = v;
        }
    }
}

// ------------------------------------------------------------------------- depth-1 (2D) layers in split mode (r5)
// The sheared first layer's prep -- G = a depth-1 3x7 convolution of the upsampled right feature, 32 -> 96 channels, and its small
// relatives (G', the left half's 3x3 depth-class planes) -- ran on the fp32 matrix pipe: 7.8 GFLOP at 93 TFLOP/s = 84 us of a
// 2.1 ms step whose other layers had all moved to the 16x faster half pipe.  Same scheme as conv3d_x3q_kernel (three
// v_mfma_f32_16x16x32_f16 per fp32 product on (hi, lo) pairs, K = 32 = four taps of one C8 piece, image double-buffered and refilled
// late under hand-counted waits), on a 2D tile: 16 rows x 32 columns x 32 output channels per workgroup, taps in (kh, kw) raster order
// (3x7: 21 taps in 6 quads; 3x3: 9 in 3).  The result leaves as plain fp32 [N][Cout][H][W] times `head_mul` (the expand pass that
// consumes G applies the layer's affine itself); the input's scale is read from the device (`x_mul`: the feature's own maximum).
template <int KH_, int KW_>
struct X2QCfg {
    static constexpr int KH = KH_, KW = KW_, TH = 16, NB = 4, IN_H = TH + KH - 1, IN_W = 32 + KW - 1, VOX = IN_H * IN_W, GB = VOX * 16;
    static constexpr int ITEMS = 2 * VOX, PLANE_BYTES = GB, NIT = (ITEMS + 255) / 256;
    static constexpr int IMG_BYTES = NIT * 256 * 16, LDS_BYTES = 2 * IMG_BYTES;
    static constexpr int TAPS = KH * KW, NQ = (TAPS + 3) / 4, PF = 2, FILL_STEP = NQ - PF;
    static_assert(NQ > PF, "the refill is issued PF k-steps before the chunk ends");
};

// IL 1: the result is written a second time in the channel-interleaved layout (il_index) the fused first layer reads.
// The body of conv2d_x3q_kernel<Cfg, IL> for workgroup `bx` of the layer's (tile, channel block) jobs: the layer's own launch passes its
// blockIdx.x, the pooled launch (conv2d_x3q_pool_kernel) the index inside the layer's block range.
template <class Cfg, int IL>
__device__ __forceinline__ void conv2d_x3q_body(const std::conditional_t<IL == 1, F16IlArgs, F16Args> a, const int bx) {
    constexpr int NB = Cfg::NB, IN_W = Cfg::IN_W, VOX = Cfg::VOX, NIT = Cfg::NIT, NQ = Cfg::NQ;
    constexpr int ITEMS = Cfg::ITEMS, PF = Cfg::PF;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kb = lane >> 4, col = lane & 15;
    const int ntiles = a.tiles_h * a.tiles_w, cblocks = a.Cout >> 5;
    const int job = xcd_remap16(bx, ntiles * cblocks);
    const int t = job / cblocks, cb = job - t * cblocks;
    const int tw = t % a.tiles_w, th = t / a.tiles_w;
    const int64_t n = blockIdx.z;
    const int oh0 = th * Cfg::TH, ow0 = tw * 32;
    const int ih0 = oh0 - a.pad_h, iw0 = ow0 - a.pad_w;

    f32x4q acc[NB][2][2];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[nb][ph][h] = f32x4q{0.0f, 0.0f, 0.0f, 0.0f};

    const int in_hw = a.Hin * a.Win;
    unsigned off[NIT];
    unsigned vmask = 0, pmask = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = it * 256 + tid;
        const int plane = i / VOX, r = i - plane * VOX;
        pmask |= (unsigned)(plane & 1) << it;
        const int hh = r / IN_W, ww = r - hh * IN_W;
        const int gh = ih0 + hh, gw = iw0 + ww;
        const bool ok = i < ITEMS && (unsigned)gh < (unsigned)a.Hin && (unsigned)gw < (unsigned)a.Win;
        off[it] = ok ? (unsigned)(gh * a.Win + gw) : 0u;
        vmask |= (ok ? 1u : 0u) << it;
    }
    const _Float16 *xn = a.x + n * a.x_bs, *xn_lo = a.x_lo + n * a.x_bs;
    const int wbase = tid & ~63;
    auto issue = [&](int chunk, int buf) {
        const int64_t coff = (int64_t)chunk * in_hw * 8;
        char *const ibuf = lds + buf * Cfg::IMG_BYTES;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const _Float16 *xc = (((pmask >> it) & 1u) ? xn_lo : xn) + coff;
            const void *src = ((vmask >> it) & 1u) ? static_cast<const void *>(xc + (size_t)off[it] * 8) : static_cast<const void *>(g_zero16h);
            __builtin_amdgcn_global_load_lds(static_cast<const float *>(src), reinterpret_cast<float *>(ibuf + (it * 256 + wbase) * 16), 16, 0, 0);
        }
    };
    int qoff[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        int tp = 4 * q + kb;
        tp = tp < Cfg::TAPS ? tp : Cfg::TAPS - 1;       // a slot beyond the last tap: zero weights, the last tap's piece
        qoff[q] = ((tp / Cfg::KW) * IN_W + tp % Cfg::KW + col) * 16;
    }
    int rowoff[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) rowoff[nb] = (wave * NB + nb) * IN_W * 16;
    const int64_t steps_total = (int64_t)a.nchunks * NQ;
    const h8 *wq = reinterpret_cast<const h8 *>(a.wp) + ((int64_t)cb * steps_total * 4) * 64 + lane;
    h8 q_[PF][4];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
#pragma unroll
        for (int m = 0; m < 4; ++m) q_[i][m] = wq[m * 64];
        wq += 4 * 64;
    }

    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)lds;
    issue(0, 0);
    __syncthreads();
    for (int chunk = 0; chunk < a.nchunks; ++chunk) {
        const unsigned img = lds_base + (unsigned)((chunk & 1) * Cfg::IMG_BYTES);
        const bool more = chunk + 1 < a.nchunks;
        h8 bfr[2][8];      // [buffer][(row of the half-step) * 4 + (row half) * 2 + plane]
        auto load_b = [&](int buf, int hs) {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const unsigned addr = img + (unsigned)(qoff[hs >> 1] + rowoff[2 * (hs & 1) + rr]);
                lds_read_b128_to<0>(bfr[buf][rr * 4 + 0], addr);
                lds_read_b128_to<Cfg::PLANE_BYTES>(bfr[buf][rr * 4 + 1], addr);
                lds_read_b128_to<256>(bfr[buf][rr * 4 + 2], addr);
                lds_read_b128_to<Cfg::PLANE_BYTES + 256>(bfr[buf][rr * 4 + 3], addr);
            }
        };
        load_b(0, 0);
        h8 af[4];
#pragma unroll
        for (int hs = 0; hs < 2 * NQ; ++hs) {
            const int cur = hs & 1, nx = cur ^ 1;
            if ((hs & 1) == 0) {
                if (hs == 2 * Cfg::FILL_STEP) {
                    // every weight fragment in flight lands first: none is waited for between here and the barrier
#pragma unroll
                    for (int i = 0; i < PF; ++i) asm volatile("" ::"v"(q_[i][0]), "v"(q_[i][1]), "v"(q_[i][2]), "v"(q_[i][3]));
                    if (more) issue(chunk + 1, (chunk + 1) & 1);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) af[m] = q_[0][m];
#pragma unroll
                for (int i = 0; i + 1 < PF; ++i)
#pragma unroll
                    for (int m = 0; m < 4; ++m) q_[i][m] = q_[i + 1][m];
#pragma unroll
                for (int m = 0; m < 4; ++m) q_[PF - 1][m] = wq[m * 64];      // from k-step FILL_STEP on: fragments of the NEXT chunk
                wq += 4 * 64;
            }
            if (hs + 1 < 2 * NQ) {
                load_b(nx, hs + 1);
                wait_lgkm_for<8>(bfr[cur]);
            } else {
                wait_lgkm_for<0>(bfr[cur]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int term = 0; term < 3; ++term)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const h8 aw = term == 0 ? af[2 * h + 1] : af[2 * h];
                            const h8 bx = bfr[cur][rr * 4 + ph * 2 + (term == 1 ? 1 : 0)];
                            acc[2 * (hs & 1) + rr][ph][h] =
                                __builtin_amdgcn_mfma_f32_16x16x32_f16(aw, bx, acc[2 * (hs & 1) + rr][ph][h], 0, 0, 0);
                        }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();     // drains the DMA of the next chunk and retires every read of this chunk's buffer
    }

    // epilogue: lane (kb, col) holds channels cb * 32 + 8 kb + e of columns col / col + 16 of its four rows; fp32 [N][Cout][H][W]
    const int64_t out_hw = (int64_t)a.Hout * a.Wout;
    const bool relu = (a.flags & SNVC_EPI_RELU) != 0;
    const int c0 = cb * 32 + 8 * kb;
    const float xm = a.x_mul ? a.head_mul / a.x_mul[0] : a.head_mul;
    float sc[8], bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = (a.scale ? a.scale[c0 + e] : 1.0f) * xm;
        bi[e] = a.scale ? a.bias[c0 + e] : 0.0f;
    }
    // il_mode 2 (class-major rows of a layer whose plain result is class-minor): row c0 + e is channel co * 3 + cls of the plain result
    int64_t yc0 = c0, ystep = out_hw;
    if constexpr (IL == 1) {
        if (a.il_mode == 2) {
            yc0 = il_plain_plane(c0, a.il_C);
            ystep = 3 * out_hw;
        }
    }
    float *yn = a.y_f32 + n * a.yf_bs + yc0 * out_hw;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int phh = oh0 + wave * NB + nb;
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
            const int pw = ow0 + 16 * ph + col;
            if (phh < a.nh && pw < a.nw) {
                float *yp = yn + (int64_t)phh * a.Wout + pw;
                float v8[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = __builtin_fmaf(acc[nb][ph][e >> 2][e & 3], sc[e], bi[e]);
                    if (relu) v = __builtin_fmaxf(v, 0.0f);
                    yp[e * ystep] = v;
                    v8[e] = v;
                }
                if constexpr (IL == 1) {
                    float *il = a.y_il + n * a.il_bs;
                    if (a.il_mode != 1) {      // class-major rows (0, 2), C % 8 == 0: the lane's 8 channels are one channel group
                        float *dst = il + il_index<int>(0, c0, a.il_C, a.Hout, a.il_pitch, a.il_lp, a.il_cls0, phh, pw);
                        *reinterpret_cast<f32x4q *>(dst) = f32x4q{v8[0], v8[1], v8[2], v8[3]};
                        *reinterpret_cast<f32x4q *>(dst + 4) = f32x4q{v8[4], v8[5], v8[6], v8[7]};
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) il[il_index<int>(1, c0 + e, a.il_C, a.Hout, a.il_pitch, a.il_lp, a.il_cls0, phh, pw)] = v8[e];
                    }
                }
            }
        }
    }
}

template <class Cfg, int IL = 0>
__global__ void __launch_bounds__(256, 2)
conv2d_x3q_kernel(const std::conditional_t<IL == 1, F16IlArgs, F16Args> a) {
    conv2d_x3q_body<Cfg, IL>(a, blockIdx.x);
}

// The first layer's three depth-1 layers of a step in ONE launch (include/snvc_prep.h): blockIdx.x runs over G's jobs, then G''s, then the
// left planes' (long jobs first); a block finds its layer from the two cumulative job counts -- wave-uniform, no table in memory -- and
// runs that layer's own kernel body on that layer's own argument record with its LOCAL job index (xcd_remap16 sees the local index
// and the layer's own job count, as in the layer's own launch).  Each of the three launches alone holds less than one resident
// round of workgroups (512 slots on 256 CUs); together they fill it.  The records travel by value and are chosen by uniform
// branches -- the 3x3 body on its own, the 3x7 body once for G and G' with the record picked between the two arguments (one inlined
// body per range took 235 VGPRs, this takes the 3x7 kernel's 232) -- never by an index into an array of records, which may be moved
// to scratch.
struct X2QPoolArgs {
    F16IlArgs g, gcol, left;
    int end_g, end_gcol;       // jobs of G; of G and G': the first block of the next range
};
static_assert(sizeof(X2QPoolArgs) <= 4096, "the kernel argument segment");

__host__ __device__ __forceinline__ int pool_range3(int b, int end0, int end1, int &local) {
    if (b < end0) { local = b; return 0; }
    if (b < end1) { local = b - end0; return 1; }
    local = b - end1;
    return 2;
}

__global__ void __launch_bounds__(256, 2)
conv2d_x3q_pool_kernel(const X2QPoolArgs p) {
    int local;
    const int sub = pool_range3((int)blockIdx.x, p.end_g, p.end_gcol, local);
    if (sub == 2) conv2d_x3q_body<X2QCfg<3, 3>, 1>(p.left, local);
    else conv2d_x3q_body<X2QCfg<3, 7>, 1>(sub == 0 ? p.g : p.gcol, local);      // one of two records, not an index: both stay kernel arguments
}

// ------------------------------------------------------------------------- 16x16x32 form of the stride-2 3x3x3 split layer (r5)
// The hourglass's stride-2 layers (snvc/models/submodule.py:88-94,170-181) were the layers furthest from any roof: the 2x4x32 output tile
// of conv3d_f16_kernel<F16K3S2X> needs a 5 x 9 x 65-piece image PER PLANE (46.8 KB), so the planes were taken one after the other,
// single-buffered at two workgroups per CU: every pass a fill with nothing under it but the other workgroup, the weights of a
// chunk streamed twice (hi pass, lo pass), 14 k-steps of 32x32x16 MFMAs per fill.  hg conv1 at cfg2: 1.16 GB moved at 3.4 TB/s.
// This form: ONE PERSISTENT workgroup of 8 waves per CU with THREE image slots (144 KB of the CU's 160 KB LDS),
// v_mfma_f32_16x16x32_f16 (K = 32 = four taps of one C8 piece, as conv3d_x3q_kernel), 64 output channels per workgroup: wave =
// (row pair of the 2x4 output rows) x (32-channel half), so a wave holds only ITS half's weights -- a step's w_hi and w_lo, 2 x 56
// VGPRs: MFMA operands cannot sit in AGPRs, and vmcnt retires in order: a weight fetched behind an LDS-DMA would wait for it, so a
// step's weights are all in registers before its refills are requested.  A step (one channel group of one tile, both planes):
//   the NEXT step's hi plane is requested into the spare slot;
//   phase L: acc += w_hi * x_lo   from the lo slot, 7 tap quads x 8 MFMAs per wave;
//   barrier (LDS reads only); the next step's lo plane is requested into the lo slot just released;
//   phase H: acc += w_lo * x_hi + w_hi * x_hi   from the hi slot, 7 quads x 16 MFMAs; as each quad retires its weight registers the
//            next step's fragments are requested into them (first read behind the barrier below);
//   barrier (drains everything); the hi slot becomes the spare one.
// Steps run on across tile boundaries (the next tile's first planes are requested under this tile's last step, the epilogue's
// stores drain under the next tile's MFMAs): with one workgroup per CU nothing else would hide a workgroup's first fill, last
// wait and stores -- one workgroup per tile measured 397 us on hg conv1, of which 257 remained with MFMAs AND refills off.
// Measured (tools/time_hg.py, back to back): hg conv1 395-407 -> 326 us, hg conv3 93 -> 85 us.  What still bounds it is the
// refill itself: 1.08 GB through 94 KB-per-CU bursts reach 3.3 TB/s (a deeper queue needs a fourth slot the LDS does not have).
// The image rows are stored POLYPHASE in blocks of 32 columns -- 16 even columns, then the 16 odd ones -- so that the 16 output columns of
// a fragment read consecutive pieces for every tap (column 2c + kw: kw = 0 / 2 -> even piece c / c + 1, kw = 1 -> odd piece c):
// conflict-free ds_read_b128 where the natural order reads at a 32-byte stride, while 32 consecutive LDS positions are still 32
// consecutive columns, i.e. a DMA round fetches whole 128-byte lines.  Same values as the 32x32x16 form up to fp32 summation order.
struct X3S2Cfg {
    static constexpr int TD = 2, TH = 4, NB = 2, IN_D = 5, IN_H = 9, IN_W = 65, VOX = IN_D * IN_H * IN_W;
    static constexpr int THREADS = 512, NIT = (VOX + THREADS - 1) / THREADS, SLOT_BYTES = NIT * THREADS * 16, LDS_BYTES = 3 * SLOT_BYTES;
    static constexpr int NQ = 7;
};

template <int N>
__device__ __forceinline__ void wait_lgkm_for4(h8 (&b)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : "n"(N) : "memory");
}

// ALIAS: the input pair's duplicate wedge tiles were not written (a.in_alias, include/snvc_alias.h): a piece of such a row is fetched
// from the representative's plane -- the same 128-byte lines of another plane, decided in geometry() and nowhere else.
// ALIAS 2 (include/snvc_hgdedup.h): <1>'s read, and the walk runs over the LIVE jobs only -- total_jobs is their count and decode() maps
// a live index to its tile (a.live); the step pipeline never sees a duplicate, whose rows of the output pair stay unwritten.
template <int ALIAS = 0>
__global__ void __launch_bounds__(512, 1)
conv3d_x3s2q_kernel(const std::conditional_t<ALIAS == 2, F16LiveArgs, std::conditional_t<ALIAS == 1, F16AliasArgs, F16Args>> a, const int total_jobs) {
    using Cfg = X3S2Cfg;
    constexpr int NB = Cfg::NB, TH = Cfg::TH, IN_H = Cfg::IN_H, IN_W = Cfg::IN_W, VOX = Cfg::VOX, NIT = Cfg::NIT, NQ = Cfg::NQ;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    // 8 waves: wave = (row pair 0..3) + 4 * (32-channel half of the 64 output channels).  Two waves per SIMD: each holds the weights of ITS
    // 32 channels only (2 x 56 VGPRs for a step's w_hi and w_lo -- MFMA operands cannot sit in AGPRs, and all 64 channels' 224 do not
    // fit beside the B fragments), every B fragment is read by the two waves that share its rows
    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, chalf = tid >> 8, kb = lane >> 4, col = lane & 15;
    // PERSISTENT: one workgroup per CU walks the jobs b, b + G, b + 2 G, ... (job = (sample, tile, 64-channel block); G a multiple of 8,
    // so a workgroup stays inside its XCD's contiguous range of tiles).  With one workgroup per CU nothing else hides a workgroup's
    // start-up (first fill: a whole HBM round trip), its last wait and its stores -- measured with the MFMAs AND the refills
    // switched off, one workgroup per tile still took 257 of 397 us on hg conv1.  Here the chunk pipeline simply runs on across
    // tile boundaries: the next tile's first planes are requested under the last phase H of this one, the epilogue's stores drain
    // under the next tile's MFMAs.
    const int ntiles = a.tiles_d * a.tiles_h * a.tiles_w, cblocks = a.Cout >> 6;
    const int in_hw = a.Hin * a.Win, in_dhw = in_hw * a.Din;
    const int wbase = tid & ~63;

    struct Job { int od0, oh0, ow0, cb; int64_t n; };
    auto decode = [&](int b) {
        const int j = xcd_remap16(b, total_jobs);
        Job jb;
        if constexpr (ALIAS == 2) {
            const int cb = j % cblocks, r = j / cblocks, u = r % a.live.live_tiles;      // wave-uniform: scalar registers throughout
            jb.n = r / a.live.live_tiles; jb.cb = cb;
            int td, th, tw;
            hg_live_tile(a.live, a.tiles_h, a.tiles_w, u, td, th, tw);
            jb.od0 = td * Cfg::TD; jb.oh0 = th * TH; jb.ow0 = tw * 32;
            return jb;
        }
        const int cb = j % cblocks, r = j / cblocks, t = r % ntiles;
        jb.n = r / ntiles; jb.cb = cb;
        const int tw = t % a.tiles_w, th = (t / a.tiles_w) % a.tiles_h, td = t / (a.tiles_w * a.tiles_h);
        jb.od0 = td * Cfg::TD; jb.oh0 = th * TH; jb.ow0 = tw * 32;
        return jb;
    };
    // staging geometry of a tile: piece i of a slot = (dd, hh, position in the polyphase row)
    unsigned off[NIT];
    unsigned vmask = 0;
    auto geometry = [&](const Job &jb) {
        const int id0 = 2 * jb.od0 - a.pad_d, ih0 = 2 * jb.oh0 - a.pad_h, iw0 = 2 * jb.ow0 - a.pad_w;
        vmask = 0;
        // the pieces' (dd, hh, pp) are derived from the thread index anew at every tile hand-over: kept across the step loop they are
        // 18 more live values than the register file has (they were spilled, and reloaded one wait at a time in front of the refill)
        int tid_ = tid;
        asm volatile("" : "+v"(tid_));
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = it * 512 + tid_;
            const int dd = i / (IN_H * IN_W), r2 = i - dd * (IN_H * IN_W);
            const int hh = r2 / IN_W, pp = r2 - hh * IN_W;
            // row layout: [16 even columns][16 odd columns] twice, then column 64 -- 32 consecutive positions are 32 consecutive
            // columns (permuted): a DMA round still fetches whole 128-byte lines
            const int blk = pp >> 5, rr_ = pp & 31;
            const int ww = pp == 64 ? 64 : (rr_ < 16 ? 2 * (16 * blk + rr_) : 2 * (16 * blk + rr_ - 16) + 1);
            const int gd = id0 + dd, gh = ih0 + hh, gw = iw0 + ww;
            const bool ok = i < VOX && (unsigned)gd < (unsigned)a.Din && (unsigned)gh < (unsigned)a.Hin && (unsigned)gw < (unsigned)a.Win;
            int sd = gd;      // the plane that holds the piece
            if constexpr (ALIAS) sd = wedge_alias_depth(a.in_alias, gd, gw);
            off[it] = ok ? (unsigned)(sd * in_hw + gh * a.Win + gw) : 0u;
            vmask |= (ok ? 1u : 0u) << it;
        }
    };
    auto issue = [&](int64_t n, int chunk, bool lo_plane, int slot) {      // every wave issues all NIT rounds (pieces past the image land in the slot's padding)
        const _Float16 *xc = (lo_plane ? a.x_lo : a.x) + n * a.x_bs + (int64_t)chunk * in_dhw * 8;
        char *const ibuf = lds + slot * Cfg::SLOT_BYTES;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const void *src = ((vmask >> it) & 1u) ? static_cast<const void *>(xc + (size_t)off[it] * 8) : static_cast<const void *>(g_zero16h);
            __builtin_amdgcn_global_load_lds(static_cast<const float *>(src), reinterpret_cast<float *>(ibuf + (it * 512 + wbase) * 16), 16, 0, 0);
        }
    };
    // this lane's byte offset of tap 4 q + kb inside a slot (output column `col` of the tile's left half; + 256 B: the right half)
    int qoff[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        int tp = 4 * q + kb;
        tp = tp < 27 ? tp : 26;                     // the 28th slot: zero weights, tap 26's piece
        const int kd = tp / 9, kh = (tp / 3) % 3, kw = tp % 3;
        // column 2 c + kw of output column c = col (+ 16 for the right half: + 32 positions): kw = 0 -> even piece c, kw = 1 -> odd piece c,
        // kw = 2 -> even piece c + 1 (for c = 15 the first piece of the next block: position 32)
        const int pos = kw == 0 ? col : (kw == 1 ? 16 + col : (col == 15 ? 32 : col + 1));
        qoff[q] = ((kd * IN_H + kh) * IN_W + pos) * 16;
    }
    int rowoff[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = wave * NB + nb;
        rowoff[nb] = ((2 * (row / TH)) * IN_H + 2 * (row % TH)) * IN_W * 16;
    }
    // weights: [cb][chunk][quad][co half (4)][hi | lo][lane] pieces (pack_q16s_weights_kernel with NH = 4)
    // (the pointer stays wave-uniform and the lane is added in the index: the loads take the scalar-base form, one VGPR of offset
    // for all 56 fragments of a step instead of a 64-bit address pair each)
    const h8 *const wall = reinterpret_cast<const h8 *>(a.wp);
    const int64_t wchunk = (int64_t)NQ * 8 * 64;     // pieces per (cb, chunk)

    int b = blockIdx.x;
    Job cur = decode(b);
    geometry(cur);
    h8 WH[NQ][2], WL[NQ][2];
    {
        const h8 *wc = wall + (int64_t)cur.cb * a.nchunks * wchunk;
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                WH[q][h] = wc[(q * 8 + (2 * chalf + h) * 2) * 64 + lane];
                WL[q][h] = wc[(q * 8 + (2 * chalf + h) * 2 + 1) * 64 + lane];
            }
    }
    f32x4q acc[NB][2][2];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[nb][ph][h] = f32x4q{0.0f, 0.0f, 0.0f, 0.0f};

    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)lds;
    int s_hi = 0, s_sp = 2;                          // slots: hi plane, (1 = lo plane, fixed), spare
    issue(cur.n, 0, false, 0);
    issue(cur.n, 0, true, 1);
    __syncthreads();
    const int gstride = gridDim.x;
    constexpr float kHalfMax = 65504.0f;
    const bool has_aff = a.scale != nullptr;         // decided once, not per channel
    float vmax = 0.0f;
    int chunk = 0;
    while (true) {
        const bool last_chunk = chunk + 1 == a.nchunks;
        const bool next_job = last_chunk && b + gstride < total_jobs;
        const bool more = !last_chunk || next_job;
        // the next step's hi plane is requested FIRST (the spare slot is free): with the lo plane following behind phase L, a request
        // is outstanding for all but the few hundred cycles around the two barriers (requested only behind phase L, every CU asked
        // for its 94 KB at the same moment and then waited: hg conv1 moved 3.2 TB/s)
        Job nxt = cur;
        if (next_job) {                              // block-uniform: the tile behind this one (all of this tile's planes are requested already)
            nxt = decode(b + gstride);
            geometry(nxt);
        }
        const int nchunk = last_chunk ? 0 : chunk + 1;
        if (more) issue(nxt.n, nchunk, false, s_sp);
        h8 bfr[2][4];      // [buffer][row * 2 + row half]
        auto load_b = [&](int buf, unsigned img, int q) {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const unsigned addr = img + (unsigned)(qoff[q] + rowoff[rr]);
                lds_read_b128_to<0>(bfr[buf][rr * 2 + 0], addr);
                lds_read_b128_to<512>(bfr[buf][rr * 2 + 1], addr);
            }
        };
        // ---- phase L: w_hi * x_lo
        {
            const unsigned img = lds_base + (unsigned)Cfg::SLOT_BYTES;
            load_b(0, img, 0);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int cb_ = q & 1, nx = cb_ ^ 1;
                if (q + 1 < NQ) {
                    load_b(nx, img, q + 1);
                    wait_lgkm_for4<4>(bfr[cb_]);
                } else {
                    wait_lgkm_for4<0>(bfr[cb_]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                        for (int h = 0; h < 2; ++h)
                            acc[rr][ph][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(WH[q][h], bfr[cb_][rr * 2 + ph], acc[rr][ph][h], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the lo slot is released by every wave (a bare s_barrier: no vector-memory wait -- the hi plane's refill stays in flight; this
        // chunk's weights landed before the barrier that ended the previous step)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (more) issue(nxt.n, nchunk, true, 1);
        // ---- phase H: (w_lo + w_hi) * x_hi
        {
            const h8 *wn = wall + ((int64_t)nxt.cb * a.nchunks + nchunk) * wchunk;
            const unsigned img = lds_base + (unsigned)(s_hi * Cfg::SLOT_BYTES);
            load_b(0, img, 0);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int cb_ = q & 1, nx = cb_ ^ 1;
                if (q + 1 < NQ) {
                    load_b(nx, img, q + 1);
                    wait_lgkm_for4<4>(bfr[cb_]);
                } else {
                    wait_lgkm_for4<0>(bfr[cb_]);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int term = 0; term < 2; ++term)
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                            for (int h = 0; h < 2; ++h)
                                acc[rr][ph][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(term == 0 ? WL[q][h] : WH[q][h], bfr[cb_][rr * 2 + ph],
                                                                                        acc[rr][ph][h], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                // the next step's weights of this quad, into the registers the quad has just retired (first read behind the barrier below)
                if (more) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        WH[q][h] = wn[(q * 8 + (2 * chalf + h) * 2) * 64 + lane];
                        WL[q][h] = wn[(q * 8 + (2 * chalf + h) * 2 + 1) * 64 + lane];
                    }
                }
            }
        }
        __syncthreads();                             // drains the refill and retires every read of the hi slot
        { const int o = s_hi; s_hi = s_sp; s_sp = o; }
        if (!last_chunk) { ++chunk; continue; }

        // ---- epilogue of the finished tile: lane (kb, col) holds, per 32-channel block bb, the 8 channels of C8 group 4 bb + kb for
        // voxel col (+16) of its rows.  Its stores drain under the next tile's first phase.
        {
            const int out_hw = a.Hout * a.Wout;
            const int64_t out_dhw = (int64_t)out_hw * a.Dout;
            const bool relu = (a.flags & SNVC_EPI_RELU) != 0;
            const float lo_bound = relu ? 0.0f : -kHalfMax;
            {
                const int bb = chalf;
                const int c0 = cur.cb * 64 + bb * 32 + 8 * kb;
                // four 16-byte loads behind ONE block-uniform test (they were sixteen dwords, each behind its own).  Requested ahead of
                // the step's last barrier instead -- into the B fragments' registers -- they cost the kernel its 256-register budget:
                // 68-84 bytes of scratch, reloaded in front of every refill (profiles/epilogue_round_trips/)
                f32x4q scv[2] = {f32x4q{1.0f, 1.0f, 1.0f, 1.0f}, f32x4q{1.0f, 1.0f, 1.0f, 1.0f}};
                f32x4q biv[2] = {f32x4q{0.0f, 0.0f, 0.0f, 0.0f}, f32x4q{0.0f, 0.0f, 0.0f, 0.0f}};
                if (has_aff) {
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        scv[k] = *reinterpret_cast<const f32x4q *>(a.scale + c0 + 4 * k);
                        biv[k] = *reinterpret_cast<const f32x4q *>(a.bias + c0 + 4 * k);
                    }
                }
                float sc[8], bi[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    sc[e] = scv[e >> 2][e & 3];
                    bi[e] = biv[e >> 2][e & 3];
                }
                const int64_t gplane = (int64_t)(cur.cb * 8 + bb * 4 + kb) * out_dhw * 8;
                _Float16 *yn = a.y + cur.n * a.y_bs + gplane, *yn_lo = a.y_lo + cur.n * a.y_bs + gplane;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int row = wave * NB + nb;
                    const int pd = cur.od0 + row / TH, phh = cur.oh0 + row % TH;
#pragma unroll
                    for (int ph = 0; ph < 2; ++ph) {
                        const int pw = cur.ow0 + 16 * ph + col;
                        const bool ok = pd < a.nd && phh < a.nh && pw < a.nw;
                        const int64_t sp = ok ? ((int64_t)pd * out_hw + phh * a.Wout + pw) : 0;
                        h8 o, ol;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float v = __builtin_fmaf(acc[nb][ph][e >> 2][e & 3], sc[e], bi[e]);
                            v = __builtin_amdgcn_fmed3f(v, lo_bound, kHalfMax);
                            vmax = __builtin_fmaxf(vmax, ok ? __builtin_fabsf(v) : 0.0f);
                            o[e] = (_Float16)v;
                            ol[e] = (_Float16)(v - (float)o[e]);
                            acc[nb][ph][e >> 2][e & 3] = 0.0f;
                        }
                        if (ok) {
                            *reinterpret_cast<h8 *>(yn + sp * 8) = o;
                            *reinterpret_cast<h8 *>(yn_lo + sp * 8) = ol;
                        }
                    }
                }
            }
        }
        if (!next_job) break;                        // block-uniform: every wave of the workgroup leaves here
        b += gstride;
        cur = nxt;
        chunk = 0;
    }
    if (vmax >= kHalfMax && a.overflow) atomicOr(a.overflow, 1);
}

// 16x16x32 form of the 5^3 / dilated 5^3 / 7^3 layers (split mode with the planes serial, one channel group per chunk, as F16K5X /
// F16K5D2X / F16K7X; and the fp16-storage family): K = 32 = FOUR TAPS of one C8 piece -- k-block kb = lane >> 4 is tap 4 q + kb of
// the list of ALL K^3 taps in (kd, kh, kw) raster order, cut into equal runtime-looped segments (a segment is what gets unrolled):
// 5^3: one segment of 32 quads for 125 taps (2 % padding; slice by slice -- 5 x 7 quads for 5 x 25 taps, the first form -- the
// plain 5^3 layer gained nothing over the 13 tap pairs of the 32x32x16 form), 7^3: two segments of 43 quads for 343 taps (0.3 %
// instead of 6 %).  A slot beyond the last tap has zero weights and re-reads the last tap's piece.  A lane's byte offset per quad
// comes from a table in LDS behind the image, fetched one quad ahead (a register table of 32 or 43 does not fit; computed per quad
// -- two divisions -- it ate the gain in the forms with 16 MFMAs per half-step).  Measured against the slice-by-slice form: 7^3
// -2..3 %, dilated 5^3 -6..10 %, 5^3 -18..22 % against its 32x32x16 form.  Same tile, image, staging, sub-grid classes and epilogue
// contract as the 32x32x16 forms; residual (before / after the activation) supported; C8 output only.
// flat segments of the 16x16x32 forms (Q16SCfg::FSEG): 5^3 and dilated 5^3 one (125 taps = 32 quads), 7^3 two (343 taps = 2 x 43 quads)
constexpr int q16s_flat_segments(int ks) { return ks == 7 ? 2 : 1; }
constexpr int q16s_steps(int ks) {      // k-steps per pass
    const int f = q16s_flat_segments(ks), k3 = ks * ks * ks;
    return f * (((k3 + f - 1) / f + 3) / 4);
}

template <int KS_, int DILW_, int PLQ_ = 3, int NHB_ = 1>
struct Q16SCfg {
    // PLQ = 3: split mode, planes serial (a hi pass: lo_w * hi_x + hi_w * hi_x; a lo pass: hi_w * lo_x); PLQ = 1: the fp16-STORAGE family
    // (one plane, one MFMA per product, C8 half output).  NHB: 32-channel blocks per workgroup (2: every B fragment feeds two
    // blocks -- the fp16-storage form needs that: with one block its LDS reads alone saturate the LDS at the MFMA rate)
    static constexpr int KS = KS_, DILW = DILW_, PLQ = PLQ_, NHB = NHB_, TD = 4, TH = 4, NB = 4;
    static constexpr bool SPLIT = PLQ_ == 3;
    static constexpr int NH = 2 * NHB, MA = NH * (SPLIT ? 2 : 1), PASSES = SPLIT ? 2 : 1;
    static constexpr int IN_D = TD + KS - 1, IN_H = TH + KS - 1, IN_W = 32 + (KS - 1) * DILW, VOX = IN_D * IN_H * IN_W;
    static constexpr int ITEMS = VOX, NIT = (ITEMS + 255) / 256, IMG_BYTES = NIT * 256 * 16;
    static constexpr int K3 = KS * KS * KS, KSEG = q16s_flat_segments(KS);      // segments of the flat tap list
    static constexpr int NQ = ((K3 + KSEG - 1) / KSEG + 3) / 4, NT = 4 * NQ, PF = 2;      // quads / tap slots per segment
    static constexpr int STEPS = KSEG * NQ;                 // k-steps per pass
    static_assert(STEPS == q16s_steps(KS) && KSEG * NT >= K3 && (KSEG - 1) * NT < K3, "the segments cover the taps");
    static constexpr int TAB_BYTES = KSEG * NT * 4;         // byte offset of every tap slot's piece inside the image
    static constexpr int LDS_BYTES = IMG_BYTES + TAB_BYTES;
    static_assert(NIT <= 32, "validity mask is one register");
    static_assert(PLQ_ == 3 || PLQ_ == 1, "planes serial (split) or one plane (fp16 storage)");
};

template <class Cfg>
__global__ void __launch_bounds__(256, 2)
conv3d_q16s_kernel(const F16Args a_) {
    F16Args a = a_;
    const int cls = blockIdx.z / a.N;
    if (a.cls_mode == 2) {
        const int pd = (cls >> 1) & 1, ph = cls & 1;
        a.offd = a.iod = pd; a.offh = a.ioh = ph;
        a.nd = (a.Dout - pd + 1) / 2; a.nh = (a.Hout - ph + 1) / 2;
    }
    constexpr int NB = Cfg::NB, TH = Cfg::TH, IN_H = Cfg::IN_H, IN_W = Cfg::IN_W, NIT = Cfg::NIT, NQ = Cfg::NQ;
    constexpr int ITEMS = Cfg::ITEMS, PF = Cfg::PF, KS = Cfg::KS, NH = Cfg::NH, MA = Cfg::MA;
    constexpr bool SPLIT = Cfg::SPLIT;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kb = lane >> 4, col = lane & 15;
    const int ntiles = a.tiles_d * a.tiles_h * a.tiles_w;
    const int t = xcd_remap16(blockIdx.x, ntiles);
    const int tw = t % a.tiles_w, th = (t / a.tiles_w) % a.tiles_h, td = t / (a.tiles_w * a.tiles_h);
    const int cb = blockIdx.y;
    const int64_t n = blockIdx.z - cls * a.N;
    const int od0 = td * Cfg::TD, oh0 = th * TH, ow0 = tw * 32;
    if (od0 >= a.nd || oh0 >= a.nh) return;      // a smaller class of an odd extent: whole tile outside (block-uniform)
    const int id0 = od0 - a.pad_d, ih0 = oh0 - a.pad_h, iw0 = ow0 - a.pad_w;

    f32x4q acc[NB][2][NH];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph)
#pragma unroll
            for (int h = 0; h < NH; ++h) acc[nb][ph][h] = f32x4q{0.0f, 0.0f, 0.0f, 0.0f};

    const int in_hw = a.Hin * a.Win, in_dhw = in_hw * a.Din;
    unsigned off[NIT];
    unsigned vmask = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = it * 256 + tid;
        const int dd = i / (IN_H * IN_W), r2 = i - dd * (IN_H * IN_W);
        const int hh = r2 / IN_W, ww = r2 - hh * IN_W;
        const int gd = (id0 + dd) * a.isd + a.iod, gh = (ih0 + hh) * a.ish + a.ioh, gw = iw0 + ww;
        const bool ok = i < ITEMS && (unsigned)gd < (unsigned)a.Din && (unsigned)gh < (unsigned)a.Hin && (unsigned)gw < (unsigned)a.Win;
        off[it] = ok ? (unsigned)(gd * in_hw + gh * a.Win + gw) : 0u;
        vmask |= (ok ? 1u : 0u) << it;
    }
    const _Float16 *xn = a.x + n * a.x_bs, *xn_lo = SPLIT ? a.x_lo + n * a.x_bs : nullptr;
    const int wbase = tid & ~63;
    auto issue = [&](int pass) {                    // split: pass = chunk * 2 + plane; fp16 storage: pass = chunk
        const int chunk = SPLIT ? pass >> 1 : pass;
        const _Float16 *xc = ((SPLIT && (pass & 1)) ? xn_lo : xn) + (int64_t)chunk * in_dhw * 8;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = it * 256 + tid;
            const void *src = ((vmask >> it) & 1u) ? static_cast<const void *>(xc + (size_t)off[it] * 8) : static_cast<const void *>(g_zero16h);
            if (ITEMS % 256 == 0 || i < ITEMS)
                __builtin_amdgcn_global_load_lds(static_cast<const float *>(src), reinterpret_cast<float *>(lds + (it * 256 + wbase) * 16), 16, 0, 0);
        }
    };
    // this lane's byte offset inside the image for every quad of taps: the LDS table (written here, visible behind the first pass's
    // barrier), two quads of it in registers at a time
    int qo2[2] = {0, 0};
    const int *const qlane = reinterpret_cast<const int *>(lds + Cfg::IMG_BYTES) + kb;
    {
        int *const qtab = reinterpret_cast<int *>(lds + Cfg::IMG_BYTES);
        for (int i = tid; i < Cfg::KSEG * Cfg::NT; i += 256) {
            const int tp = i < Cfg::K3 ? i : Cfg::K3 - 1;          // a slot beyond the last tap: zero weights, the last tap's piece
            const int kd = tp / (KS * KS), r = tp - kd * (KS * KS), kh = r / KS, kw = r - kh * KS;
            qtab[i] = ((kd * IN_H + kh) * IN_W + kw * Cfg::DILW) * 16;
        }
    }
    const int col16 = col * 16;
    int rowoff[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = wave * NB + nb;
        rowoff[nb] = ((row / TH) * IN_H + (row % TH)) * IN_W * 16;
    }
    // A fragments: [cout block][chunk][pass][segment][quad][co half][hi | lo (split)][lane] pieces, in consumption order
    const int npass = a.nchunks * Cfg::PASSES;
    const int64_t steps_total = (int64_t)npass * Cfg::STEPS;
    const h8 *wq = reinterpret_cast<const h8 *>(a.wp) + ((int64_t)cb * steps_total * MA) * 64 + lane;
    h8 q_[PF][MA];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
#pragma unroll
        for (int m = 0; m < MA; ++m) q_[i][m] = wq[m * 64];
        wq += MA * 64;
    }

    for (int ps = 0; ps < npass; ++ps) {
        issue(ps);
        __syncthreads();
        const bool lo_pass = SPLIT && (ps & 1);
        // half-step hs = 2 s + j: rows 2 j, 2 j + 1 of k-step s = (segment, quad); its 4 B fragments are fetched one half-step ahead
        h8 bfr[2][4];
        auto load_b = [&](int buf, int qo, int j) {
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int ph = 0; ph < 2; ++ph)
                    bfr[buf][rr * 2 + ph] = *reinterpret_cast<const h8 *>(lds + qo + rowoff[2 * j + rr] + ph * 256);
        };
        qo2[0] = qlane[0] + col16;
        load_b(0, qo2[0], 0);
        h8 af[MA];
#pragma unroll 1
        for (int seg = 0; seg < Cfg::KSEG; ++seg) {
            const int *const qseg = qlane + seg * Cfg::NT;
#pragma unroll
            for (int hs = 0; hs < 2 * NQ; ++hs) {
                const int cur = hs & 1, nxt = cur ^ 1, j = hs & 1;
                if (j == 0) {
#pragma unroll
                    for (int m = 0; m < MA; ++m) af[m] = q_[0][m];
#pragma unroll
                    for (int i = 0; i + 1 < PF; ++i)
#pragma unroll
                        for (int m = 0; m < MA; ++m) q_[i][m] = q_[i + 1][m];
#pragma unroll
                    for (int m = 0; m < MA; ++m) q_[PF - 1][m] = wq[m * 64];
                    wq += MA * 64;
                    // the next quad's offset (behind the segment's last quad: the next segment's first)
                    const int qn = (hs >> 1) + 1;      // a constant after unrolling
                    if (qn < NQ) qo2[qn & 1] = qseg[4 * qn] + col16;
                    else if (seg + 1 < Cfg::KSEG) qo2[qn & 1] = qseg[Cfg::NT] + col16;
                }
                if (hs + 1 < 2 * NQ) load_b(nxt, qo2[((hs + 1) >> 1) & 1], (hs + 1) & 1);
                else if (seg + 1 < Cfg::KSEG) load_b(nxt, qo2[NQ & 1], 0);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (SPLIT) {
                    if (!lo_pass) {
#pragma unroll
                        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                            for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                                for (int h = 0; h < NH; ++h)
                                    acc[2 * j + rr][ph][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[2 * h + 1], bfr[cur][rr * 2 + ph], acc[2 * j + rr][ph][h], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                    for (int ph = 0; ph < 2; ++ph)
#pragma unroll
                        for (int h = 0; h < NH; ++h)
                            acc[2 * j + rr][ph][h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[SPLIT ? 2 * h : h], bfr[cur][rr * 2 + ph], acc[2 * j + rr][ph][h], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            // 2 NQ half-steps per segment: an even count, so the buffer roles repeat from segment to segment
            if constexpr (NQ % 2 == 1) qo2[0] = qo2[1];      // the next segment's first quad looks in slot 0
        }
        __syncthreads();
    }

    // ---- epilogue: lane (kb, col) holds, per 32-channel block, the 8 channels of C8 group 4 * block + kb for voxel col (+16) of its rows
    const int out_hw = a.Hout * a.Wout;
    const int64_t out_dhw = (int64_t)out_hw * a.Dout;
    const bool relu = (a.flags & SNVC_EPI_RELU) != 0, add_pre = (a.flags & SNVC_EPI_ADD_PRE) != 0, add_post = (a.flags & SNVC_EPI_ADD_POST) != 0;
    constexpr float kHalfMax = 65504.0f;
    float vmax = 0.0f;
#pragma unroll
    for (int blk = 0; blk < Cfg::NHB; ++blk) {
        const int cblk = cb * Cfg::NHB + blk;
        if (cblk * 32 >= a.Cout) break;
        const int c0 = cblk * 32 + 8 * kb;
        float sc[8], bi[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sc[e] = a.scale ? a.scale[c0 + e] : 1.0f;
            bi[e] = a.scale ? a.bias[c0 + e] : 0.0f;
        }
        const int64_t gplane = (int64_t)(cblk * 4 + kb) * out_dhw * 8;
        _Float16 *yn = a.y + n * a.y_bs + gplane, *yn_lo = SPLIT ? a.y_lo + n * a.y_bs + gplane : nullptr;
        const _Float16 *rn = a.res ? a.res + n * a.r_bs + gplane : nullptr, *rn_lo = (SPLIT && a.res) ? a.res_lo + n * a.r_bs + gplane : nullptr;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int row = wave * NB + nb;
            const int pd = od0 + row / TH, phh = oh0 + row % TH;
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                const int pw = ow0 + 16 * ph + col;
                const bool ok = pd < a.nd && phh < a.nh && pw < a.nw;
                const int64_t sp = ok ? ((int64_t)(pd * a.osd + a.offd) * out_hw + (phh * a.osh + a.offh) * a.Wout + (pw * a.osw + a.offw)) : 0;
                h8 rv = h8((_Float16)0.0f), rl = h8((_Float16)0.0f);
                if (rn) {
                    rv = *reinterpret_cast<const h8 *>(rn + sp * 8);
                    if constexpr (SPLIT) rl = *reinterpret_cast<const h8 *>(rn_lo + sp * 8);
                }
                h8 o, ol;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = __builtin_fmaf(acc[nb][ph][2 * blk + (e >> 2)][e & 3], sc[e], bi[e]);
                    const float rr = SPLIT ? ((float)rv[e] + (float)rl[e]) * a.res_mul : (float)rv[e];
                    if (rn && add_pre) v += rr;
                    if (relu) v = v > 0.0f ? v : 0.0f;
                    if (rn && add_post) v += rr;
                    if constexpr (SPLIT) {
                        v = __builtin_amdgcn_fmed3f(v, -kHalfMax, kHalfMax);
                        vmax = __builtin_fmaxf(vmax, ok ? __builtin_fabsf(v) : 0.0f);
                    }
                    o[e] = (_Float16)v;
                    if constexpr (SPLIT) ol[e] = (_Float16)(v - (float)o[e]);
                }
                if (ok) {
                    *reinterpret_cast<h8 *>(yn + sp * 8) = o;
                    if constexpr (SPLIT) *reinterpret_cast<h8 *>(yn_lo + sp * 8) = ol;
                }
            }
        }
    }
    if constexpr (SPLIT) {
        if (vmax >= kHalfMax && a.overflow) atomicOr(a.overflow, 1);
    }
}

// packed weights of conv3d_q16s_kernel: [cb][chunk][pass][slice kd][quad][co half (NH)][hi | lo (NPL)][lane][8]
__global__ void pack_q16s_weights_kernel(const float *__restrict__ w, _Float16 *__restrict__ out, int Cout, int Cin, int K3, int NSEG, int NT,
                                         int NQ, int nchunks, int NH, int NPL, int PASSES, float wmul, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int64_t r = i;
    const int e = (int)(r % 8); r /= 8;
    const int lane = (int)(r % 64); r /= 64;
    const int pl = (int)(r % NPL); r /= NPL;
    const int h = (int)(r % NH); r /= NH;
    const int q = (int)(r % NQ); r /= NQ;
    const int kd = (int)(r % NSEG); r /= NSEG;                 // segment: a depth slice of NT = K * K taps, or all K^3 taps (3^3)
    r /= PASSES;                                               // both passes of a chunk see the same weights
    const int chunk = (int)(r % nchunks); r /= nchunks;
    const int cb = (int)r;
    const int row = lane & 15, kb = lane >> 4;
    const int co = (cb * (NH / 2) + (h >> 1)) * 32 + 8 * (row >> 2) + 4 * (h & 1) + (row & 3);
    const int ci = chunk * 8 + e;
    const int tp = 4 * q + kb;
    float v = 0.0f;
    // segment kd holds taps kd * NT .. of the (kd, kh, kw) raster: a depth slice (NT = K * K) or a run of the flat list (NT = 4 NQ slots)
    if (tp < NT && kd * NT + tp < K3 && co < Cout && ci < Cin) v = w[((int64_t)co * Cin + ci) * K3 + kd * NT + tp] * wmul;
    const _Float16 hi = (_Float16)v;
    out[i] = pl == 0 ? hi : (_Float16)(v - (float)hi);
}

// ------------------------------------------------------------------------------------ weight packing
struct PackArgs {
    const float *w;
    _Float16 *out;
    int Cout, Cin, K;          // K = original cubic kernel size
    int transposed, pd, ph, pw;  // transposed: parity class of this packing ([Cin][Cout][3][3][3] source)
    int KD, KH, KW, KCG, MODE, MI, SEGS, TSEG, NPS, NS, unroll_d;
    int nchunks, cblocks;
    int PL;                    // >= 2: split mode, [..][m][hi | lo][lane][8]; values are w * wmul (a power of two) split as hi + lo
    int PASSES;                // 2: planes taken serially, the k-steps of a chunk are stored once per pass
    int dyn;                   // 1: transposed class packed over its real taps only (F16Cfg::DYN): NS = 2 * pairs of this class
    float wmul;
    int64_t total;             // elements (halves)
};

__global__ void pack_f16_weights_kernel(const PackArgs p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.total) return;
    int64_t r = i;
    const int e = (int)(r % 8); r /= 8;
    const int lane = (int)(r % 64); r /= 64;
    const int npl = p.PL >= 2 ? 2 : 1;
    const int pl = (int)(r % npl); r /= npl;
    const int m = (int)(r % p.MI); r /= p.MI;
    const int s = (int)(r % p.NS); r /= p.NS;
    const int seg = (int)(r % p.SEGS); r /= p.SEGS;
    r /= p.PASSES;                                             // both passes of a chunk see the same weights
    const int chunk = (int)(r % p.nchunks); r /= p.nchunks;
    const int cb = (int)r;
    const int half = lane >> 5;
    const int co = (cb * p.MI + m) * 32 + f16_row_channel(lane & 31);
    int tap, g;
    if (p.dyn) { g = s % p.KCG; tap = 2 * (s / p.KCG) + half; }
    else if (p.MODE == 0) { tap = s / (p.KCG / 2); g = 2 * (s % (p.KCG / 2)) + half; }
    else { g = s / p.NPS; tap = 2 * (s % p.NPS) + half; }
    const int ci = (chunk * p.KCG + g) * 8 + e;
    float v = 0.0f;
    if (p.dyn) {
        const int nw = 1 + p.pw, nh = 1 + p.ph, ndp = 1 + p.pd;
        if (tap < nw * nh * ndp && co < p.Cout && ci < p.Cin) {
            const int b[3] = {tap / (nw * nh), (tap / nw) % nh, tap % nw}, par[3] = {p.pd, p.ph, p.pw};
            int k3[3];
            for (int d = 0; d < 3; ++d) k3[d] = par[d] == 0 ? 1 : (b[d] == 0 ? 2 : 0);      // parity 1: box tap 0 = kernel index 2, tap 1 = index 0
            v = p.w[((((int64_t)ci * p.Cout + co) * 3 + k3[0]) * 3 + k3[1]) * 3 + k3[2]];
        }
    } else if (tap < p.TSEG && co < p.Cout && ci < p.Cin) {
        const int kd = p.unroll_d ? tap / (p.KH * p.KW) : seg, kh = (tap / p.KW) % p.KH, kw = tap % p.KW;
        if (!p.transposed) {
            v = p.w[((((int64_t)co * p.Cin + ci) * p.K + kd) * p.K + kh) * p.K + kw];
        } else {
            // parity class: per dim, parity 0 -> only box tap 0 exists (kernel index 1); parity 1 -> box tap 0 is
            // kernel index 2 (input offset 0), box tap 1 is kernel index 0 (input offset +1)
            const int par[3] = {p.pd, p.ph, p.pw}, b[3] = {kd, kh, kw};
            int k3[3];
            bool ok = true;
            for (int d = 0; d < 3; ++d) {
                if (par[d] == 0) { ok = ok && b[d] == 0; k3[d] = 1; }
                else k3[d] = b[d] == 0 ? 2 : 0;
            }
            if (ok) v = p.w[((((int64_t)ci * p.Cout + co) * 3 + k3[0]) * 3 + k3[1]) * 3 + k3[2]];
        }
    }
    if (p.PL >= 2) {
        v *= p.wmul;
        const _Float16 hi = (_Float16)v;
        p.out[i] = pl ? (_Float16)(v - (float)hi) : hi;
    } else {
        p.out[i] = (_Float16)v;
    }
}

// ------------------------------------------------------------------------------------ configurations
//                        KD KH KW S  D  MI TD TH KCG MODE DB   OCC
using F16K1   = F16Cfg<1, 1, 1, 1, 1, 2, 4, 4, 2, 0, true, 2>;
using F16K3   = F16Cfg<3, 3, 3, 1, 1, 2, 4, 4, 2, 0, true, 2>;
using F16K3H  = F16Cfg<3, 3, 3, 1, 1, 1, 4, 4, 2, 0, true, 2>;     // one 32-channel block: the 1-channel head
using F16K3S2 = F16Cfg<3, 3, 3, 2, 1, 2, 2, 4, 1, 1, false, 2>;
using F16K5   = F16Cfg<5, 5, 5, 1, 1, 2, 4, 4, 1, 1, true, 2>;
// dilation 2 = four independent (depth, height)-parity sub-grids, each a convolution with dilation (1,1,2): the image
// of a tile is 8x8x40 pieces (41 KB) instead of 12x12x40 (92 KB: one workgroup per CU with its staging exposed)
using F16K5D2 = F16Cfg<5, 5, 5, 1, 1, 2, 4, 4, 1, 1, false, 2, 2>;
// (a double-buffered image at one workgroup per CU: 14.3 ms against 9.0 on cfg5's conv1 -- two co-resident workgroups matter)
using F16K7   = F16Cfg<7, 7, 7, 1, 1, 2, 4, 4, 1, 1, false, 2>;
using F16DC   = F16Cfg<2, 2, 2, 1, 1, 2, 4, 4, 2, 0, true, 2>;      // one parity class of ConvTranspose3d(k3,s2,p1,op1)
// r3: MI = 1 forms for layers with exactly 32 output channels (the released F = 32 model, vernier.py:249-264: every
// trunk layer but the hourglass's inner ones).  The 64-channel forms above would multiply a second, all-zero weight
// block (half of the MFMAs wasted: released-shape conv1 ran at 0.27 of the fp16 peak).  Same tiles and images; a wave
// carries 4 accumulators instead of 8.
using F16K1N   = F16Cfg<1, 1, 1, 1, 1, 1, 4, 4, 2, 0, true, 2>;
using F16K3S2N = F16Cfg<3, 3, 3, 2, 1, 1, 2, 4, 1, 1, false, 2>;
using F16K5N   = F16Cfg<5, 5, 5, 1, 1, 1, 4, 4, 1, 1, true, 2>;
using F16K5D2N = F16Cfg<5, 5, 5, 1, 1, 1, 4, 4, 1, 1, false, 2, 2>;
using F16K7N   = F16Cfg<7, 7, 7, 1, 1, 1, 4, 4, 1, 1, false, 2>;
using F16DCN   = F16Cfg<2, 2, 2, 1, 1, 1, 4, 4, 2, 0, true, 2>;

// r4 split mode ("f16x3": fp32-accurate layers on the half pipe, see F16Cfg::PL): one channel group per chunk, two taps per MFMA
// (MODE 1), hi and lo planes of the image side by side in LDS (2 x 19.6 KB), single-buffered at two workgroups per CU (three
// before the k-loop's B fragments were double-buffered in registers: 194-238 VGPRs now).  conv2 at cfg2 takes 0.88-0.90 ms in
// every form tried since (2 or 3 WG/CU, image single- or double-buffered, loads sunk or hoisted): the SAME launch on all-zero
// operands takes 0.76 ms -- the layer is bound by the chip's power limit (the clock under this kernel is 1.62 GHz of 2.4), not
// by a stall a schedule could remove; profiles/r4/kernel_experiments_r4.txt item 10.
//                         KD KH KW S  D  MI TD TH KCG MODE DB    OCC DILW PL
using F16K3X  = F16Cfg<3, 3, 3, 1, 1, 1, 4, 4, 1, 1, false, 2, 1, 2>;
using F16K3X2 = F16Cfg<3, 3, 3, 1, 1, 2, 4, 4, 1, 1, false, 2, 1, 2>;
// experiment (desc.algo & SNVC_ALGO_X3_SERIAL): planes taken serially, the 19.6 KB image double-buffered
using F16K3XS  = F16Cfg<3, 3, 3, 1, 1, 1, 4, 4, 1, 1, true, 3, 1, 3>;
// (measured and not kept, conv2 at cfg2: resident planes double-buffered at 2 WG/CU 1.03 ms, a 4x8x32 tile 0.94 ms, the serial
// form above 0.91-1.07 ms, against 0.89-0.92 ms for the single-buffered 4x4x32 tile at 3 WG/CU)
// small layers (SNVC_ALGO_X3_SMALL, chosen by the caller when a launch would not fill the chip): 2x4x32 tiles, one 32-channel
// block per workgroup -- four times the workgroups of F16K3X2 (the hourglass's 48x24x78 level: 216 -> 864)
using F16K3XT  = F16Cfg<3, 3, 3, 1, 1, 1, 2, 4, 1, 1, false, 4, 1, 2>;
using F16K3X2S = F16Cfg<3, 3, 3, 1, 1, 2, 4, 4, 1, 1, true, 2, 1, 3>;
// stride 2: the image of a 2x4x32 tile is 5 x 9 x 65 pieces (46.8 KB per plane): the planes are taken serially (PL = 3)
using F16K3S2X = F16Cfg<3, 3, 3, 2, 1, 2, 2, 4, 1, 1, false, 2, 1, 3>;
// one parity class of ConvTranspose3d(k3,s2,p1,op1): 2x2x2 box taps, both planes resident, double-buffered
// (first forms, all 8 box taps with zero weights where a class has none: KCG = 1 double-buffered 0.255 ms, KCG = 2 0.284 ms on hg conv5)
using F16DCX  = F16Cfg<2, 2, 2, 1, 1, 2, 4, 4, 2, 1, false, 2, 1, 2, true>;
// r5, SNVC_ALGO_X3_SMALL on the stride-2 and transposed split layers: the hourglass's quarter-resolution level (cfg2: 48x24x78) gives
// a 2x4x32 / 4x4x32 tiling 432 / 216 tiles -- fewer workgroups than the chip has slots, each one a serial chain of 16 / 4 single-
// buffered fills whose latency nothing hides.  Half-height tiles: twice the workgroups, 64 accumulator registers instead of 128
// (three workgroups per CU), images of 28 KB (stride 2, per plane) / 32 KB (transposed, both planes).
using F16K3S2XT = F16Cfg<3, 3, 3, 2, 1, 2, 1, 4, 1, 1, false, 3, 1, 3>;
using F16DCXT   = F16Cfg<2, 2, 2, 1, 1, 2, 2, 4, 2, 1, false, 3, 1, 2, true>;

// split forms of the local trunk's other layer kinds (snvc/models/vernier.py:249-278): 1x1x1 (two channel groups per MFMA, both
// planes resident), 5^3 / dilated 5^3 (sub-grid classes) / 7^3 (planes serial: their single-plane images are 37 / 41 / 61 KB),
// the 32-output-channel transposed layer (hourglass_downsample_16's conv12), and the one-channel occupancy head (EPI 1 on F16K3X)
//                         KD KH KW S  D  MI TD TH KCG MODE DB    OCC DILW PL
using F16K1X   = F16Cfg<1, 1, 1, 1, 1, 1, 4, 4, 2, 0, true, 3, 1, 2>;
using F16K5X   = F16Cfg<5, 5, 5, 1, 1, 1, 4, 4, 1, 1, false, 3, 1, 3>;
using F16K5D2X = F16Cfg<5, 5, 5, 1, 1, 1, 4, 4, 1, 1, false, 2, 2, 3>;
using F16K7X   = F16Cfg<7, 7, 7, 1, 1, 1, 4, 4, 1, 1, false, 2, 1, 3>;
using F16DCXN  = F16Cfg<2, 2, 2, 1, 1, 1, 4, 4, 2, 1, false, 3, 1, 2, true>;

// A fragments of the tail projection (conv3d_f16_kernel EPI 4): [m][j][hi | lo][lane][8]; row (lane & 31) = tap, k = 8 * (lane >> 5) + e
// is channel 32 m + 16 (lane >> 5) + 8 j + e -- the channel that accumulator register 8 j + e of lane (voxel, lane >> 5) holds
__global__ void pack_tail_weights_kernel(const float *__restrict__ w, _Float16 *__restrict__ out, int Cin, float wmul, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int r = i;
    const int e = r % 8; r /= 8;
    const int lane = r % 64; r /= 64;
    const int pl = r % 2; r /= 2;
    const int j = r % 2; r /= 2;
    const int m = r;
    const int tap = lane & 31, c = 32 * m + 16 * (lane >> 5) + 8 * j + e;
    const float v = (tap < 27 && c < Cin) ? w[c * 27 + tap] * wmul : 0.0f;
    const _Float16 hi = (_Float16)v;
    out[i] = pl == 0 ? hi : (_Float16)(v - (float)hi);
}

// out[o] = bias + res[o] + sum over (i, k) with o = 2 i - 1 + k (per dimension) of T[k][i]: the scatter half of a transposed layer
// (k3, s2, p1, op1) to one channel whose per-voxel contraction T was formed by the producing layer (EPI 4).  T is class-major:
// [27][8 = (i_d & 1, i_h & 1, i_w & 1)][nd][nh][nw], i = 2 p + r.  A thread owns 4 consecutive outputs of one output row
// (ow = 4 j .. 4 j + 3): every T element is read exactly once, 4-byte loads consecutive across the lanes, one 16-byte store.
// ALIAS: the residual's duplicate wedge tiles were not written (include/snvc_alias.h).  The thread's four outputs lie in one 32-column
// tile (4 j is 4-aligned) of one plane: one remap of od per thread, for the residual's load only.
template <int ALIAS>
__device__ __forceinline__ void deconv_tail_gather_body(const float *__restrict__ t, const float *__restrict__ bias, const float *__restrict__ res,
                                                        float *__restrict__ y, int nd, int nh, int nw, int64_t t_bs, int64_t y_bs, int64_t r_bs,
                                                        const WedgeDesc &ra) {
    const int OD = 4 * nd, OH = 4 * nh;
    const int64_t total = (int64_t)OD * OH * nw;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % nw);
    const int64_t r0 = i / nw;
    const int oh = (int)(r0 % OH), od = (int)(r0 / OH);
    const int64_t n = blockIdx.y;
    const int64_t cls_vox = (int64_t)nd * nh * nw, tap_stride = 8 * cls_vox;
    const float *tn = t + n * t_bs;
    const float b = bias ? bias[0] : 0.0f;
    float o0 = b, o1 = b, o2 = b, o3 = b;
    // per dimension: even output 2 a: (k = 1, i = a); odd output 2 a + 1: (k = 2, i = a) and (k = 0, i = a + 1)
    const int ad = od >> 1, ah = oh >> 1;
    const int ndd = (od & 1) ? 2 : 1, nhh = (oh & 1) ? 2 : 1;
    const bool last_w = j + 1 >= nw;
    for (int a_ = 0; a_ < ndd; ++a_) {
        const int kd = (od & 1) ? (a_ ? 0 : 2) : 1, id = ad + a_;
        if (id >= 2 * nd) continue;
        for (int b_ = 0; b_ < nhh; ++b_) {
            const int kh = (oh & 1) ? (b_ ? 0 : 2) : 1, ih = ah + b_;
            if (ih >= 2 * nh) continue;
            const int cdh = ((id & 1) << 2) | ((ih & 1) << 1);
            const int64_t base = ((int64_t)(id >> 1) * nh + (ih >> 1)) * nw + j;
            const float *t0 = tn + (int64_t)((kd * 3 + kh) * 3) * tap_stride + base;      // kw = 0
            const float *c0 = t0 + (int64_t)cdh * cls_vox, *c1 = t0 + (int64_t)(cdh | 1) * cls_vox;      // i_w even / odd at p_w = j
            // ow = 4j: (kw 1, i_w = 2j); 4j+1: (kw 2, 2j) + (kw 0, 2j+1); 4j+2: (kw 1, 2j+1); 4j+3: (kw 2, 2j+1) + (kw 0, 2j+2)
            o0 += c0[tap_stride];
            o1 += c0[2 * tap_stride] + c1[0];
            o2 += c1[tap_stride];
            o3 += c1[2 * tap_stride] + (last_w ? 0.0f : c0[1]);
        }
    }
    const int64_t sp = ((int64_t)od * OH + oh) * (4 * nw) + 4 * j;
    if (res) {
        int64_t rsp = sp;
        if constexpr (ALIAS) rsp = ((int64_t)wedge_alias_depth(ra, od, 4 * j) * OH + oh) * (4 * nw) + 4 * j;
        const f32x4 rv = *reinterpret_cast<const f32x4 *>(res + n * r_bs + rsp);
        o0 += rv[0]; o1 += rv[1]; o2 += rv[2]; o3 += rv[3];
    }
    *reinterpret_cast<f32x4 *>(y + n * y_bs + sp) = f32x4{o0, o1, o2, o3};
}

__global__ void __launch_bounds__(256)
deconv_tail_gather_kernel(const float *__restrict__ t, const float *__restrict__ bias, const float *__restrict__ res, float *__restrict__ y,
                          int nd, int nh, int nw, int64_t t_bs, int64_t y_bs, int64_t r_bs) {
    deconv_tail_gather_body<0>(t, bias, res, y, nd, nh, nw, t_bs, y_bs, r_bs, WedgeDesc{});
}
__global__ void __launch_bounds__(256)
deconv_tail_gather_alias_kernel(const float *__restrict__ t, const float *__restrict__ bias, const float *__restrict__ res, float *__restrict__ y,
                                int nd, int nh, int nw, int64_t t_bs, int64_t y_bs, int64_t r_bs, const WedgeDesc ra) {
    deconv_tail_gather_body<1>(t, bias, res, y, nd, nh, nw, t_bs, y_bs, r_bs, ra);
}

// The power of two that puts max|x| into [2^13, 2^14) (1 for an all-zero or non-finite tensor) -- the scale of a split pair whose range is
// only known from the data -- in ONE launch (r5; the torch expression it replaces was ten small launches): every workgroup folds its
// share into scratch[0] (float bits of a non-negative maximum order like unsigned integers), the last one to arrive (scratch[1]) turns
// the maximum into the scale and leaves both words zero for the next call.  NaNs do not take part (fmaxf drops them), +-inf gives 1.
// (the body: workgroup `bx` of `nblocks` that fold x into scratch[0 .. 1]; split_scale_pair_kernel runs it for two tensors in one grid)
__device__ __forceinline__ void split_scale_body(const float *x, int64_t n, unsigned *scratch, float *out,
                                                 const unsigned bx, const unsigned nblocks) {
    float m = 0.0f;
    const int64_t stride = (int64_t)nblocks * 256 * 4;
    const int64_t n4 = n & ~(int64_t)3;
    auto amax4 = [](const f32x4 v) {
        return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])), __builtin_fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3])));
    };
    // few workgroups, four independent 16-byte loads in flight per thread: the launch's time is the chain of same-address atomics
    // at its end (r5: 234 workgroups 9.1 us for 3.8 MB; <= 48 workgroups: see profiles/r5)
    int64_t i = ((int64_t)bx * 256 + threadIdx.x) * 4;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 v0 = *reinterpret_cast<const f32x4 *>(x + i), v1 = *reinterpret_cast<const f32x4 *>(x + i + stride);
        const f32x4 v2 = *reinterpret_cast<const f32x4 *>(x + i + 2 * stride), v3 = *reinterpret_cast<const f32x4 *>(x + i + 3 * stride);
        m = __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fmaxf(amax4(v0), amax4(v1)), __builtin_fmaxf(amax4(v2), amax4(v3))));
    }
    for (; i < n4; i += stride) m = __builtin_fmaxf(m, amax4(*reinterpret_cast<const f32x4 *>(x + i)));
    if (bx == 0 && threadIdx.x < (int)(n - n4)) m = __builtin_fmaxf(m, __builtin_fabsf(x[n4 + threadIdx.x]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = __builtin_fmaxf(__builtin_fmaxf(part[0], part[1]), __builtin_fmaxf(part[2], part[3]));
        atomicMax(scratch, __builtin_bit_cast(unsigned, m));
        __threadfence();
        if (atomicAdd(scratch + 1, 1u) == nblocks - 1) {
            const float amax = __builtin_bit_cast(float, atomicExch(scratch, 0u));
            atomicExch(scratch + 1, 0u);
            float e = floorf(log2f(16384.0f / amax));          // amax = 0 -> +inf, amax = inf -> -inf: "not finite" below
            e = (e == e && __builtin_fabsf(e) < 3.0e38f) ? __builtin_fminf(__builtin_fmaxf(e, -24.0f), 40.0f) : 0.0f;
            out[0] = exp2f(e);
        }
    }
}

__global__ void __launch_bounds__(256)
split_scale_kernel(const float *__restrict__ x, int64_t n, unsigned *__restrict__ scratch, float *__restrict__ out) {
    split_scale_body(x, n, scratch, out, blockIdx.x, gridDim.x);
}

// Stage A of the pooled first-layer prep (include/snvc_prep.h): two tensors' scales in one grid.  Workgroups [0, nb0) fold x0 into
// scratch words (0, 1) and leave out0, workgroups [nb0, gridDim.x) fold x1 into words (2, 3) and leave out1 -- each half is
// split_scale_kernel with its own workgroup count, last-arrival rule and zeroing; the halves share nothing.
__global__ void __launch_bounds__(256)
split_scale_pair_kernel(const float *__restrict__ x0, int64_t n0, float *__restrict__ out0, const float *__restrict__ x1, int64_t n1,
                        float *__restrict__ out1, unsigned *__restrict__ scratch4, const unsigned nb0) {
    int local;
    const bool second = pool_range3((int)blockIdx.x, (int)nb0, (int)gridDim.x, local) != 0;       // workgroup-uniform
    split_scale_body(second ? x1 : x0, second ? n1 : n0, scratch4 + (second ? 2 : 0), second ? out1 : out0, (unsigned)local,
                     second ? gridDim.x - nb0 : nb0);
}

// Stage B: the three split pairs the pooled layers read, in one 1D grid of three block ranges: Rq (sheared_upsample_split_kernel's
// body with (WU, off)), Rq' (the same with (WU2, off2)) and the left feature's pair (ncdhw_f32_to_c8_split_kernel's body, its
// (blocks per row, channel groups, samples) grid flattened, x fastest).
struct SplitProducersArgs {
    const float *right, *left, *mul_right, *mul_left;
    _Float16 *rq_hi, *rq_lo, *rq2_hi, *rq2_lo, *l_hi, *l_lo;
    int C, H, W, q, WU, off, WU2, off2;
    int64_t total, total2, S;      // items of Rq, of Rq'; positions of one (sample, channel group) of the left feature
    int end_rq, end_rq2;           // blocks of Rq; of Rq and Rq'
    int row_blocks, groups;        // the left pair's grid: ceil(S / 256) blocks per (sample, channel group), C / 8 groups
};

__global__ void __launch_bounds__(256)
split_producers_kernel(const SplitProducersArgs p) {
    int local;
    const int sub = pool_range3((int)blockIdx.x, p.end_rq, p.end_rq2, local);
    if (sub == 0) {
        prep::sheared_upsample_split_body(p.right, p.rq_hi, p.rq_lo, p.mul_right, p.C, p.H, p.W, p.q, p.WU, p.off, p.total, (unsigned)local);
    } else if (sub == 1) {
        prep::sheared_upsample_split_body(p.right, p.rq2_hi, p.rq2_lo, p.mul_right, p.C, p.H, p.W, p.q, p.WU2, p.off2, p.total2, (unsigned)local);
    } else {
        const int bx = local % p.row_blocks, r = local / p.row_blocks, g = r % p.groups, n = r / p.groups;
        prep::ncdhw_f32_to_c8_split_body(p.left, p.l_hi, p.l_lo, p.C, p.S, (int64_t)p.C * p.S, 2 * (int64_t)p.C * p.S, 1.0f, p.mul_left,
                                         (int64_t)bx * 256 + threadIdx.x, g, n);
    }
}

// ------------------------------------------------------------------------------------ kernel forms
// One record per kernel form: the weight layout its packer writes, how its launch is laid out, which calls it takes and the launcher
// of each.  make_f16_plan picks the record of a layer; the packers, f16_geometry and the two forward calls read it and never ask
// which form it is.  A new form is one new record, and the line of plain_form / split_form that chooses it.
struct F16Geom {
    int classes;               // parity classes of the launch (the 8 transposed ones: 4 on gridDim.z, 2 on gridDim.x)
    int64_t ntiles;            // tiles of the largest class
    int64_t jobs;              // GRID_JOBS: (tile, channel block) jobs per sample; GRID_PERSISTENT: over all samples
    int64_t stats_slots;       // statistics epilogue: slots per sample, one per wave of every workgroup that a sample has on x and z
    dim3 grid;
};
using F16Launch = void (*)(const F16Args &, const F16Geom &, hipStream_t);

// what a call asks of a form, in the order a record's launchers stand; TO_C8: a C8 tensor -- the split pair, or fp16 storage's one half
enum F16Call { TO_SRC_HEAD, TO_SRC, TO_TAIL, TO_F32, TO_HEAD, TO_C8, TO_PLANE, F16_CALLS };
enum F16Classes { CLS_ONE = 0, CLS_TRANSPOSED = 1, CLS_SUBGRID = 2 };      // F16Args::cls_mode: one class, 8 transposed, 4 shared (d, h) parity
// (tiles, channel blocks, N x classes) | (tile, channel block) jobs on x, samples on z | persistent, one workgroup per CU
enum F16Grid { GRID_TILES, GRID_JOBS, GRID_PERSISTENT };

// pack_q16s_weights_kernel's layout [cb][chunk][pass][segment][quad][co half (NH)][hi | lo (NPL)][lane][8]; NQ = 0: pack_f16_weights_kernel's
struct Q16Layout { int K3, NSEG, NQ, NH, NPL, PASSES; };

struct F16Form {
    PackArgs pack;             // pack_f16_weights_kernel's layout: the Cfg's constants (the per-call fields are zero)
    Q16Layout q16;
    int MI, KCG;               // 32-channel blocks per workgroup, channel groups per chunk
    int chunk_frags;           // 64 x 8 fragments of one (channel block, chunk)
    int pad_frags;             // fragments of read-ahead padding behind a class
    int cls_mode, TD, TH, grid;
    bool split_res, stats;     // takes a split residual; has the statistics epilogue (on TO_F32)
    const char *unsupported;   // what a call without a launcher (or a residual without split_res) is told
    F16Launch launch[F16_CALLS];

    constexpr F16Form on(F16Call c, F16Launch l) const { F16Form f = *this; f.launch[c] = l; return f; }
};

template <class Cfg, int EPI>
void launch_f16(const F16Args &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_f16_kernel<Cfg, EPI>>(g.grid, 256, Cfg::LDS_BYTES, st, a);
}
template <class Cfg>
void launch_q16s(const F16Args &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_q16s_kernel<Cfg>>(g.grid, 256, Cfg::LDS_BYTES, st, a);
}
template <int EPI>
void launch_x3q(const F16Args &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_x3q_kernel<EPI>>(g.grid, 256, X3QCfg::LDS_BYTES, st, a);
}
template <int EPI>      // the fused sheared first layer: the image is formed in the launch; a is the F16SrcArgs the caller built
void launch_x3q_src(const F16Args &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_x3q_kernel<EPI, 1>>(g.grid, 256, X3QCfg::LDS_BYTES, st, static_cast<const F16SrcArgs &>(a));
}
// The duplicate wedge tiles of a [D][.][W] layer on the 4 x 4 x 32 tiling, by a walk of wedge_tile_pure: per tile column tw < max_tw
// the representative and the last duplicate depth tile (-1 / -1 without duplicates).  Returns the duplicates of one (n, th).
struct WedgeRange { int64_t dups; int td0, td1, ntw; };      // column 0's first and last duplicate; columns with duplicates (the leading ones)
WedgeRange wedge_ranges(int D, int W, int q, int m0, int off, int64_t *first_td, int64_t *last_td, int max_tw) {
    WedgeRange r{0, -1, -1, 0};
    const int tiles_d = (D + X3QCfg::TD - 1) / X3QCfg::TD, tiles_w = (W + 31) / 32;
    for (int tw = 0; tw < tiles_w; ++tw) {
        int first = -1, last = -1;
        for (int td = 0; td < tiles_d; ++td) {
            if (!wedge_tile_pure(D, W, q, m0, off, td * X3QCfg::TD, tw * 32)) continue;
            if (first < 0) first = td;
            last = td;
        }
        if (last == first) first = last = -1;      // a lone pure tile has no duplicate
        if (tw < max_tw && first_td && last_td) { first_td[tw] = first; last_td[tw] = last; }
        if (first < 0) continue;
        r.dups += last - first;
        r.ntw = tw + 1;
        if (tw == 0) { r.td0 = first + 1; r.td1 = last; }
    }
    return r;
}
// behind launch_x3q_src with SRC_DEDUP: wedge_copy_kernel over the duplicates' bounding range; nothing without duplicates
void launch_wedge_copy(const F16SrcArgs &a, hipStream_t st) {
    const WedgeRange r = wedge_ranges(a.Din, a.Win, a.v_q, a.v_m0, a.v_off, nullptr, nullptr, 0);
    if (r.dups == 0) return;
    WedgeCopyArgs w{a.y, a.y_lo, a.y_head, a.y_bs, a.Cout / 8, a.Dout, a.Hout, a.Wout, a.v_q, a.v_m0, a.v_off, r.td0, r.ntw};
    wedge_copy_kernel<<<dim3((unsigned)((r.td1 - r.td0 + 1) * r.ntw), (unsigned)a.tiles_h, (unsigned)a.N), 256, 0, st>>>(w);
}

// persistent: one workgroup per CU (144 KB of LDS each), a multiple of 8 so that a workgroup's jobs b, b + G, ... stay on its XCD
int x3s2q_workgroups(const F16Geom &g) {
    int wg = device_cu_count();
    if (wg <= 0) wg = 256;
    if (g.jobs < wg) wg = g.jobs >= 8 ? (int)(g.jobs & ~(int64_t)7) : (int)g.jobs;
    return wg;
}
void launch_x3s2q(const F16Args &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_x3s2q_kernel<0>>(dim3((unsigned)x3s2q_workgroups(g)), X3S2Cfg::THREADS, X3S2Cfg::LDS_BYTES, st, a, (int)g.jobs);
}
// the same launch on an input pair whose duplicate wedge tiles were not written (snvc_alias_f16x3_conv3d_forward)
void launch_x3s2q_alias(const F16AliasArgs &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_x3s2q_kernel<1>>(dim3((unsigned)x3s2q_workgroups(g)), X3S2Cfg::THREADS, X3S2Cfg::LDS_BYTES, st, a, (int)g.jobs);
}

// The hourglass's duplicates (include/snvc_hgdedup.h) of the stride-2 layer behind a [D][.][W] tensor written under g, on the 2 x 4 x 32
// tiling of its output, by the closed forms: per tile column tw < max_tw the representative's and the last duplicate's depth tile
// (-1 / -1 without duplicates).  dups: the duplicates of one (n, th); ncols: the columns with duplicates (the leading ones).
struct HgRange { int64_t dups; int ncols, last_td; };
HgRange hg_ranges(const WedgeDesc &g, int64_t *first_td, int64_t *last_td, int max_tw) {
    HgRange r{0, 0, -1};
    for (int tw = 0; tw < max_tw; ++tw) first_td[tw] = last_td[tw] = -1;
    if (g.D < 10) return r;                              // od0 >= 2 and 2 od0 + 4 <= D - 2
    const int last = ((g.D - 6) >> 1) & ~1;              // the last pure od0 of every column that has one
    r.last_td = last / X3S2Cfg::TD;
    for (int tw = 0; 2 * (32 * tw) + 64 < g.W - 1; ++tw) {
        const int first = hg_first_pure(g, 32 * tw);
        if (first >= last) break;                        // none, or a lone pure tile: no duplicate here nor in any later column
        if (tw < max_tw) { first_td[tw] = first / X3S2Cfg::TD; last_td[tw] = r.last_td; }
        r.dups += (last - first) / X3S2Cfg::TD;
        r.ncols = tw + 1;
    }
    return r;
}
// HgLive of a launch with tiles_d x tiles_h x tiles_w tiles per sample; false: no duplicates, or more duplicate columns than the walk has runs
bool hg_live_walk(const WedgeDesc &g, int tiles_d, int tiles_h, int tiles_w, HgLive &lv) {
    int64_t first[HG_COLS], last[HG_COLS];
    const HgRange r = hg_ranges(g, first, last, HG_COLS);
    if (r.dups == 0 || r.ncols > HG_COLS) return false;
    int end[HG_COLS + 2];                                // the last depth tile of every run
    for (int c = 0; c < HG_COLS; ++c) end[c] = c < r.ncols ? (int)first[c] : r.last_td;
    end[HG_COLS] = r.last_td;
    end[HG_COLS + 1] = tiles_d - 1;
    int cum = 0, td0 = 0;
    for (int s = 0; s < HG_COLS + 2; ++s) {
        const int k = s == HG_COLS + 1 ? 0 : s;
        lv.td0[s] = td0;
        cum += (end[s] + 1 - td0) * tiles_h * (tiles_w - k);
        lv.cum[s] = cum;
        td0 = end[s] + 1;
    }
    lv.live_tiles = cum;
    return cum == (int64_t)tiles_d * tiles_h * tiles_w - r.dups * tiles_h;
}
// launch_x3s2q_alias whose walk leaves the output's duplicate tiles out (snvc_hgdedup_f16x3_conv3d_forward): g.jobs counts the live jobs
void launch_x3s2q_live(const F16LiveArgs &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_x3s2q_kernel<2>>(dim3((unsigned)x3s2q_workgroups(g)), X3S2Cfg::THREADS, X3S2Cfg::LDS_BYTES, st, a, (int)g.jobs);
}
// launch_x3q<0> on an input pair written that way (snvc_hgdedup_reader_f16x3_conv3d_forward)
void launch_x3q_hg_alias(const F16AliasArgs &a, const F16Geom &g, hipStream_t st) {
    launch_lds<conv3d_x3q_kernel<0, 2>>(g.grid, 256, X3QCfg::LDS_BYTES, st, a);
}

// a 32x32x16 form: everything but its class mode and its statistics bit follows from the Cfg; EPI 0 C8, 1 plane, 2 float32, 3 side head, 4 tail
template <class Cfg, int... EPI>
constexpr F16Form f16_form(int cls_mode, bool stats = false) {
    constexpr F16Call call_of[5] = {TO_C8, TO_PLANE, TO_F32, TO_HEAD, TO_TAIL};
    constexpr int npl = Cfg::PL >= 2 ? 2 : 1;
    F16Form f{};
    f.pack.KD = Cfg::KD; f.pack.KH = Cfg::KH; f.pack.KW = Cfg::KW; f.pack.KCG = Cfg::KCG; f.pack.MODE = Cfg::MODE; f.pack.MI = Cfg::MI;
    f.pack.SEGS = Cfg::SEGS; f.pack.TSEG = Cfg::TSEG; f.pack.NPS = Cfg::NPS; f.pack.NS = Cfg::NS; f.pack.unroll_d = Cfg::UNROLL_D ? 1 : 0;
    f.pack.PL = Cfg::PL; f.pack.PASSES = Cfg::PASSES; f.pack.dyn = Cfg::DYN ? 1 : 0;
    f.MI = Cfg::MI; f.KCG = Cfg::KCG; f.TD = Cfg::TD; f.TH = Cfg::TH;
    f.chunk_frags = Cfg::PASSES * Cfg::STEPS * Cfg::MI * npl;
    f.pad_frags = Cfg::PF * Cfg::MI * npl;
    f.cls_mode = cls_mode; f.grid = GRID_TILES; f.split_res = true; f.stats = stats;
    f.unsupported = Cfg::PL >= 2 ? "snvc_f16x3_conv3d_forward: no kernel" : "snvc_f16_conv3d_forward: no kernel";
    ((f.launch[call_of[EPI]] = launch_f16<Cfg, EPI>), ...);
    return f;
}

// a 16x16x32 form: pad_steps k-steps of read-ahead behind a class; its launchers are added with on()
constexpr F16Form q16_form(Q16Layout q, int TD, int TH, int pad_steps, int cls_mode, int grid, bool split_res, bool stats, const char *unsupported) {
    F16Form f{};
    f.q16 = q; f.MI = q.NH / 2; f.KCG = 1; f.TD = TD; f.TH = TH;
    f.chunk_frags = q.PASSES * q.NSEG * q.NQ * q.NH * q.NPL;
    f.pad_frags = pad_steps * q.NH * q.NPL;
    f.cls_mode = cls_mode; f.grid = grid; f.split_res = split_res; f.stats = stats; f.unsupported = unsupported;
    return f;
}
template <class C>      // flat tap segments: 5^3 one of all 125 taps, 7^3 two of 172 slots
constexpr F16Form q16s_form(F16Call c, const char *unsupported) {
    return q16_form({C::K3, C::KSEG, C::NQ, C::NH, C::SPLIT ? 2 : 1, C::PASSES}, C::TD, C::TH, C::PF, C::DILW == 2 ? CLS_SUBGRID : CLS_ONE, GRID_TILES, true,
                    false, unsupported).on(c, launch_q16s<C>);
}

// The records stand in the order in which the dispatch switches used to name their kernels, and an EPI list names its launchers last to
// first: the compiler emits kernels in the order (and a pack's in the reverse of the order) of first use, and this order keeps the code
// object byte for byte what it was (profiles/f16_host_plan/device_code_identity.txt).
// fp16 storage (snvc_f16_conv3d_*)
constexpr const char *kQ16C8 = "snvc_f16_conv3d_forward: the 16x16x32 form writes C8 tensors";
constexpr F16Form FORM_K7QN   = q16s_form<Q16SCfg<7, 1, 1, 1>>(TO_C8, kQ16C8);
constexpr F16Form FORM_K5QN   = q16s_form<Q16SCfg<5, 1, 1, 1>>(TO_C8, kQ16C8);
constexpr F16Form FORM_K5D2QN = q16s_form<Q16SCfg<5, 2, 1, 1>>(TO_C8, kQ16C8);
constexpr F16Form FORM_K7Q    = q16s_form<Q16SCfg<7, 1, 1, 2>>(TO_C8, kQ16C8);
constexpr F16Form FORM_K5Q    = q16s_form<Q16SCfg<5, 1, 1, 2>>(TO_C8, kQ16C8);
constexpr F16Form FORM_K5D2Q  = q16s_form<Q16SCfg<5, 2, 1, 2>>(TO_C8, kQ16C8);
constexpr F16Form FORM_K1     = f16_form<F16K1, 0>(CLS_ONE);
constexpr F16Form FORM_K3     = f16_form<F16K3, 0>(CLS_ONE);
constexpr F16Form FORM_K3H    = f16_form<F16K3H, 1>(CLS_ONE);              // the one-channel fp32 plane
constexpr F16Form FORM_K3S2   = f16_form<F16K3S2, 0>(CLS_ONE);
constexpr F16Form FORM_K5     = f16_form<F16K5, 0>(CLS_ONE);
constexpr F16Form FORM_K5D2   = f16_form<F16K5D2, 0>(CLS_SUBGRID);
constexpr F16Form FORM_K7     = f16_form<F16K7, 0>(CLS_ONE);
constexpr F16Form FORM_DC     = f16_form<F16DC, 0>(CLS_TRANSPOSED);
constexpr F16Form FORM_K1N    = f16_form<F16K1N, 0>(CLS_ONE);
constexpr F16Form FORM_K3N    = f16_form<F16K3H, 0>(CLS_ONE);
constexpr F16Form FORM_K3S2N  = f16_form<F16K3S2N, 0>(CLS_ONE);
constexpr F16Form FORM_K5N    = f16_form<F16K5N, 0>(CLS_ONE);
constexpr F16Form FORM_K5D2N  = f16_form<F16K5D2N, 0>(CLS_SUBGRID);
constexpr F16Form FORM_K7N    = f16_form<F16K7N, 0>(CLS_ONE);
constexpr F16Form FORM_DCN    = f16_form<F16DCN, 0>(CLS_TRANSPOSED);
// split mode (snvc_f16x3_conv3d_*); true: the statistics epilogue
constexpr F16Form FORM_K3X    = f16_form<F16K3X, 0, 3, 2>(CLS_ONE, true);
constexpr F16Form FORM_K3X2   = f16_form<F16K3X2, 0, 2>(CLS_ONE, true);
constexpr F16Form FORM_K3XS   = f16_form<F16K3XS, 0, 3, 2>(CLS_ONE, true);
constexpr F16Form FORM_K3X2S  = f16_form<F16K3X2S, 0, 2>(CLS_ONE, true);
constexpr F16Form FORM_K3XT   = f16_form<F16K3XT, 0, 3, 2>(CLS_ONE, true);
constexpr F16Form FORM_K3S2X  = f16_form<F16K3S2X, 0, 2>(CLS_ONE, true);
constexpr F16Form FORM_K3S2XT = f16_form<F16K3S2XT, 0, 2>(CLS_ONE, true);
constexpr F16Form FORM_DCX    = f16_form<F16DCX, 0, 2, 4>(CLS_TRANSPOSED, true);
constexpr F16Form FORM_DCXT   = f16_form<F16DCXT, 0, 2, 4>(CLS_TRANSPOSED, true);
constexpr F16Form FORM_DCXN   = f16_form<F16DCXN, 0, 2, 4>(CLS_TRANSPOSED, true);
constexpr F16Form FORM_K1X    = f16_form<F16K1X, 0, 2>(CLS_ONE);
constexpr F16Form FORM_K5X    = f16_form<F16K5X, 0, 2>(CLS_ONE);
constexpr F16Form FORM_K5D2X  = f16_form<F16K5D2X, 0, 2>(CLS_SUBGRID);
constexpr F16Form FORM_K7X    = f16_form<F16K7X, 0, 2>(CLS_ONE);
constexpr F16Form FORM_K3XH   = f16_form<F16K3X, 1>(CLS_ONE);              // the one-channel occupancy head
constexpr const char *kQ16Split = "snvc_f16x3_conv3d_forward: the 16x16x32 form writes a split C8 tensor, no side head";
constexpr F16Form FORM_K5XQ   = q16s_form<Q16SCfg<5, 1>>(TO_C8, kQ16Split);
constexpr F16Form FORM_K5D2XQ = q16s_form<Q16SCfg<5, 2>>(TO_C8, kQ16Split);
constexpr F16Form FORM_K7XQ   = q16s_form<Q16SCfg<7, 1>>(TO_C8, kQ16Split);
// [cb (64 channels)][chunk][quad][co half (4)][hi | lo][lane][8]; a whole chunk of padding: the last chunk's phase H never reads ahead, but
// stays in bounds if it did
constexpr F16Form FORM_K3S2XQ =
    q16_form({27, 1, X3S2Cfg::NQ, 4, 2, 1}, X3S2Cfg::TD, X3S2Cfg::TH, X3S2Cfg::NQ, CLS_ONE, GRID_PERSISTENT, false, false,
             "snvc_f16x3_conv3d_forward: the stride-2 16x16x32 form writes a split C8 tensor, no residual / head")
        .on(TO_C8, launch_x3s2q);
// four taps x one channel group per MFMA, [cb][chunk][quad][co half][hi | lo][lane][8]: one segment of all 27 taps
constexpr F16Form FORM_K3XQ =
    q16_form({27, 1, X3QCfg::NQ, 2, 2, 1}, X3QCfg::TD, X3QCfg::TH, X3QCfg::PF, CLS_ONE, GRID_JOBS, false, true,
             "snvc_f16x3_conv3d_forward: the 16x16x32 form has no split residual, no side head beside a float32 result")
        .on(TO_SRC_HEAD, launch_x3q_src<3>).on(TO_SRC, launch_x3q_src<0>).on(TO_F32, launch_x3q<2>).on(TO_HEAD, launch_x3q<3>).on(TO_C8, launch_x3q<0>);

struct F16Plan {
    const F16Form *form;
    int nchunks, cblocks;
    int64_t block_halves;      // packed halves of one class (without padding)
    int64_t class_stride() const { return block_halves + (int64_t)form->pad_frags * 64 * 8; }
};

// the form of a non-transposed layer with more than one output channel; NULL: none for this (ksize, stride, dilation)
const F16Form *plain_form(int key, int Cout, int algo) {
    const bool narrow = Cout == 32;      // one 32-channel block: the MI = 1 forms
    if (algo & SNVC_ALGO_X3_Q16) {       // 16x16x32 form, two blocks per workgroup (one for Cout = 32 * odd)
        const bool two = Cout % 64 == 0;
        if (key == 711) return two ? &FORM_K7Q : &FORM_K7QN;
        if (key == 512) return two ? &FORM_K5D2Q : &FORM_K5D2QN;
        if (key == 511) return two ? &FORM_K5Q : &FORM_K5QN;
    }
    switch (key) {
        case 111: return narrow ? &FORM_K1N : &FORM_K1;
        case 311: return narrow ? &FORM_K3N : &FORM_K3;
        case 321: return narrow ? &FORM_K3S2N : &FORM_K3S2;
        case 511: return narrow ? &FORM_K5N : &FORM_K5;
        case 512: return narrow ? &FORM_K5D2N : &FORM_K5D2;
        case 711: return narrow ? &FORM_K7N : &FORM_K7;
        default: return nullptr;
    }
}

const F16Form *split_form(int key, int Cout, int algo) {
    const bool q16 = algo & SNVC_ALGO_X3_Q16;      // the 16x16x32 forms
    switch (key) {
        case 111: return &FORM_K1X;
        case 321: return q16 ? &FORM_K3S2XQ : (algo & SNVC_ALGO_X3_SMALL) ? &FORM_K3S2XT : &FORM_K3S2X;
        case 511: return q16 ? &FORM_K5XQ : &FORM_K5X;
        case 512: return q16 ? &FORM_K5D2XQ : &FORM_K5D2X;
        case 711: return q16 ? &FORM_K7XQ : &FORM_K7X;
        case 311:
            if (q16) return &FORM_K3XQ;
            if (algo & SNVC_ALGO_X3_SMALL) return &FORM_K3XT;
            if (algo & SNVC_ALGO_X3_NARROW) return &FORM_K3X;
            if (algo & SNVC_ALGO_X3_SERIAL) return Cout == 32 ? &FORM_K3XS : &FORM_K3X2S;
            return Cout == 32 ? &FORM_K3X : &FORM_K3X2;
        default: return nullptr;
    }
}

int make_f16_plan(const snvc_conv3d_desc &d, F16Plan &p, bool split = false) {
#define SNVC_F16_WHO(msg) (split ? "snvc_f16x3_conv3d: " msg : "snvc_f16_conv3d: " msg)
    if (d.N < 0 || d.Cin <= 0 || d.Cout <= 0 || d.Din <= 0 || d.Hin <= 0 || d.Win <= 0)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d: sizes must be positive");
    if (d.Cin % 8 != 0) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16_conv3d: Cin must be a multiple of 8 (C8 layout)");
    if (!split && d.Cout != 1 && d.Cout % 32 != 0)
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16_conv3d: Cout must be a multiple of 32, or 1 (fp32 plane output)");
    const F16Form *f;
    if (d.transposed) {
        if (d.ksize != 3 || d.stride != 2 || d.pad != 1 || d.dilation != 1 || (split && d.Cout % 32 != 0))
            return fail(SNVC_ERR_UNSUPPORTED, split ? "snvc_f16x3_conv3d: transposed layers: k3,s2,p1,op1 with Cout % 32 == 0"
                                                    : "snvc_f16_conv3d: transposed conv supports k3,s2,p1,op1 only");
        if (d.Dout != 2 * d.Din || d.Hout != 2 * d.Hin || d.Wout != 2 * d.Win)
            return fail(SNVC_ERR_INVALID_ARGUMENT, SNVC_F16_WHO("transposed output must be 2x the input"));
        if (d.Cout == 1) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16_conv3d: transposed conv to one channel");
        if (split) f = d.Cout % 64 == 0 ? ((d.algo & SNVC_ALGO_X3_SMALL) ? &FORM_DCXT : &FORM_DCX) : &FORM_DCXN;
        else f = d.Cout == 32 ? &FORM_DCN : &FORM_DC;
    } else {
        if (d.pad != d.dilation * (d.ksize - 1) / 2) return fail(SNVC_ERR_UNSUPPORTED, SNVC_F16_WHO("pad must equal dilation*(ksize-1)/2"));
        const int eff = d.dilation * (d.ksize - 1) + 1;
        if (d.Dout != (d.Din + 2 * d.pad - eff) / d.stride + 1 || d.Hout != (d.Hin + 2 * d.pad - eff) / d.stride + 1 ||
            d.Wout != (d.Win + 2 * d.pad - eff) / d.stride + 1)
            return fail(SNVC_ERR_INVALID_ARGUMENT, SNVC_F16_WHO("output size does not match the convolution arithmetic"));
        const int key = d.ksize * 100 + d.stride * 10 + d.dilation;
        if (d.Cout == 1) {
            if (key != 311) return fail(SNVC_ERR_UNSUPPORTED, SNVC_F16_WHO("one-channel output is built for k3/s1 only"));
            f = split ? &FORM_K3XH : &FORM_K3H;
        } else {
            if (split && key == 321 && d.Cout % 64 != 0) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d: stride-2 layers need Cout % 64 == 0");
            if (split && key != 321 && d.Cout % 32 != 0) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d: Cout % 32 == 0");
            f = split ? split_form(key, d.Cout, d.algo) : plain_form(key, d.Cout, d.algo);
            if (!f) return fail(SNVC_ERR_UNSUPPORTED, SNVC_F16_WHO("(ksize,stride,dilation) not in {(1,1,1),(3,1,1),(3,2,1),(5,1,1),(5,1,2),(7,1,1)}"));
        }
    }
    p.form = f;
    p.nchunks = ceil_div(d.Cin / 8, f->KCG);
    p.cblocks = ceil_div(d.Cout, 32 * f->MI);
    p.block_halves = (int64_t)p.cblocks * p.nchunks * f->chunk_frags * 64 * 8;
    if (p.cblocks > 65535 || d.N > 65535) return fail(SNVC_ERR_UNSUPPORTED, SNVC_F16_WHO("too many channel blocks or samples"));
    return SNVC_OK;
#undef SNVC_F16_WHO
}

// The launch geometry of a planned layer: fills a's class, sub-grid, pad and tile fields, and returns the counts and the grid that the
// forward calls check and launch with -- and that the statistics workspace is sized by.
F16Geom f16_geometry(const snvc_conv3d_desc &d, const F16Plan &p, F16Args &a) {
    const F16Form &f = *p.form;
    const bool transposed = f.cls_mode == CLS_TRANSPOSED, subgrid = f.cls_mode == CLS_SUBGRID;      // (depth, height) parity classes share ONE packed weight block
    a.N = d.N; a.cls_mode = f.cls_mode; a.cls_wstride = p.class_stride();
    a.isd = a.ish = 1; a.iod = a.ioh = 0; a.offd = a.offh = a.offw = 0;
    if (transposed) {
        a.nd = d.Din; a.nh = d.Hin; a.nw = d.Win;
        a.osd = a.osh = a.osw = 2;
        a.pad_d = a.pad_h = a.pad_w = 0;
    } else if (subgrid) {
        a.nd = (d.Dout + 1) / 2; a.nh = (d.Hout + 1) / 2; a.nw = d.Wout;     // the largest class; the kernel trims the others
        a.osd = a.osh = 2; a.osw = 1;
        a.isd = a.ish = 2;
        a.pad_d = a.pad_h = d.pad / 2; a.pad_w = d.pad;
    } else {
        a.nd = d.Dout; a.nh = d.Hout; a.nw = d.Wout;
        a.osd = a.osh = a.osw = 1;
        a.pad_d = a.pad_h = a.pad_w = d.pad;
    }
    a.tiles_d = ceil_div(a.nd, f.TD); a.tiles_h = ceil_div(a.nh, f.TH); a.tiles_w = ceil_div(a.nw, 32);
    F16Geom g{};
    g.classes = transposed ? 8 : (subgrid ? 4 : 1);
    g.ntiles = (int64_t)a.tiles_d * a.tiles_h * a.tiles_w;
    const int64_t gx = transposed ? 2 * g.ntiles : g.ntiles, gz = transposed ? 4 : g.classes;
    g.grid = dim3((unsigned)gx, (unsigned)p.cblocks, (unsigned)(d.N * gz));
    g.stats_slots = gz * gx * 4;
    if (f.grid == GRID_JOBS) {           // channel block fastest: a slot per tile and wave
        g.jobs = g.ntiles * p.cblocks;
        g.grid = dim3((unsigned)g.jobs, 1, (unsigned)d.N);
        g.stats_slots = g.ntiles * 4;
    } else if (f.grid == GRID_PERSISTENT) {
        g.jobs = g.ntiles * p.cblocks * d.N;
    }
    return g;
}

// the one call site of pack_q16s_weights_kernel: total halves of [cb][chunk] blocks in layout q (NT = 4 NQ tap slots per segment)
void pack_q16(const Q16Layout &q, const float *w, void *packed, int Cout, int Cin, float wmul, int64_t total, hipStream_t st) {
    pack_q16s_weights_kernel<<<(unsigned)ceil_div<int64_t>(total, 256), 256, 0, st>>>(w, reinterpret_cast<_Float16 *>(packed), Cout, Cin, q.K3, q.NSEG, 4 * q.NQ,
                                                                                    q.NQ, Cin / 8, q.NH, q.NPL, q.PASSES, wmul, total);
}

}  // namespace
}  // namespace snvc

extern "C" {

static int64_t f16_packed_bytes(const snvc_conv3d_desc *d, bool split) {
    snvc::F16Plan p;
    if (!d || snvc::make_f16_plan(*d, p, split) != SNVC_OK) return -1;
    return 2 * p.class_stride() * (d->transposed ? 8 : 1);
}

int64_t snvc_f16_conv3d_packed_weight_bytes(const snvc_conv3d_desc *d) { return f16_packed_bytes(d, false); }
int64_t snvc_f16x3_conv3d_packed_weight_bytes(const snvc_conv3d_desc *d) { return f16_packed_bytes(d, true); }

static int f16_pack_common(const snvc_conv3d_desc *d, const float *weight, void *packed, bool split, float wmul, void *stream,
                           const char *who) {
    using namespace snvc;
    F16Plan p;
    if (!d) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_pack_weights: null desc");
    int rc = make_f16_plan(*d, p, split);
    if (rc) return rc;
    if (!weight || !packed) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_pack_weights: null pointer");
    const F16Form &f = *p.form;
    const int classes = d->transposed ? 8 : 1;
    if (hipMemsetAsync(packed, 0, (size_t)(2 * p.class_stride() * classes), as_stream(stream)) != hipSuccess)   // the ring's read-ahead padding
        return fail(SNVC_ERR_HIP, "snvc_f16_conv3d_pack_weights: hipMemsetAsync failed");
    if (f.q16.NQ) {
        pack_q16(f.q16, weight, packed, d->Cout, d->Cin, wmul, p.block_halves, as_stream(stream));
        return check_launch(who);
    }
    for (int c = 0; c < classes; ++c) {
        PackArgs a = f.pack;
        a.w = weight;
        a.out = reinterpret_cast<_Float16 *>(packed) + c * p.class_stride();
        a.Cout = d->Cout; a.Cin = d->Cin; a.K = d->ksize;
        a.transposed = d->transposed; a.pd = (c >> 2) & 1; a.ph = (c >> 1) & 1; a.pw = c & 1;
        a.nchunks = p.nchunks; a.cblocks = p.cblocks; a.total = p.block_halves;
        a.wmul = wmul;
        if (a.dyn) {        // compact per class: 2 * pairs k-steps per chunk
            const int T = (1 + a.pd) * (1 + a.ph) * (1 + a.pw);
            a.NS = 2 * (T > 1 ? T / 2 : 1);
            a.total = (int64_t)p.cblocks * p.nchunks * a.NS * a.MI * 2 * 64 * 8;
        }
        pack_f16_weights_kernel<<<(unsigned)ceil_div<int64_t>(a.total, 256), 256, 0, as_stream(stream)>>>(a);
    }
    return check_launch(who);
}

int snvc_f16_conv3d_pack_weights(const snvc_conv3d_desc *d, const float *weight, void *packed, void *stream) {
    return f16_pack_common(d, weight, packed, false, 1.0f, stream, "snvc_f16_conv3d_pack_weights");
}

int snvc_f16x3_conv3d_pack_weights(const snvc_conv3d_desc *d, const float *weight, void *packed, float wmul, void *stream) {
    return f16_pack_common(d, weight, packed, true, wmul, stream, "snvc_f16x3_conv3d_pack_weights");
}

int snvc_f16_conv3d_forward(const snvc_conv3d_desc *d, const void *x, const void *packed_weight, const float *scale,
                            const float *bias, const void *residual, void *y, float *y_f32, void *stream) {
    using namespace snvc;
    F16Plan p;
    if (!d) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_forward: null desc");
    int rc = make_f16_plan(*d, p);
    if (rc) return rc;
    if (d->N == 0) return SNVC_OK;
    const bool plane = d->Cout == 1;
    if (!x || !packed_weight || (plane ? !y_f32 : !y))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_forward: null pointer");
    if ((scale == nullptr) != (bias == nullptr))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_forward: scale and bias must both be given or both be NULL");
    const int resflags = d->flags & (SNVC_EPI_ADD_PRE | SNVC_EPI_ADD_POST);
    if (resflags && (!residual || plane))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_forward: residual flag without a C8 residual");
    if (resflags == (SNVC_EPI_ADD_PRE | SNVC_EPI_ADD_POST))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_forward: ADD_PRE and ADD_POST are exclusive");
    if (!plane && (d->flags & SNVC_EPI_SIGMOID))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16_conv3d_forward: Sigmoid is built for the one-channel fp32 output only");
    const int64_t in_sp = (int64_t)d->Din * d->Hin * d->Win, out_sp = (int64_t)d->Dout * d->Hout * d->Wout;
    if ((int64_t)(d->Cin / 8 + 2) * in_sp >= ((int64_t)1 << 31) || out_sp >= ((int64_t)1 << 31))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16_conv3d_forward: one sample must stay below 2^31 pieces");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual) |
         reinterpret_cast<uintptr_t>(packed_weight)) & 15)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_forward: C8 tensors must be 16-byte aligned");
    if ((d->x_batch_stride | d->y_batch_stride | d->res_batch_stride) % 8)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16_conv3d_forward: batch strides must be multiples of 8 elements");

    F16Args a{};
    a.x = reinterpret_cast<const _Float16 *>(x);
    a.wp = reinterpret_cast<const _Float16 *>(packed_weight);
    a.scale = scale; a.bias = bias;
    a.res = resflags ? reinterpret_cast<const _Float16 *>(residual) : nullptr;
    a.y = reinterpret_cast<_Float16 *>(y); a.y_f32 = y_f32;
    a.res_mul = 1.0f;
    a.CGin = d->Cin / 8;
    a.Cout = d->Cout;
    a.Din = d->Din; a.Hin = d->Hin; a.Win = d->Win;
    a.Dout = d->Dout; a.Hout = d->Hout; a.Wout = d->Wout;
    a.nchunks = p.nchunks; a.flags = d->flags;
    a.x_bs = d->x_batch_stride ? d->x_batch_stride : (int64_t)d->Cin * in_sp;
    a.y_bs = d->y_batch_stride ? d->y_batch_stride : (int64_t)d->Cout * out_sp;
    a.r_bs = d->res_batch_stride ? d->res_batch_stride : (int64_t)d->Cout * out_sp;
    a.yf_bs = out_sp;
    const F16Geom g = f16_geometry(*d, p, a);
    if (g.ntiles >= ((int64_t)1 << 30) || (int64_t)d->N * g.classes > 65535)
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16_conv3d_forward: too many tiles or samples");
    const F16Launch launch = p.form->launch[plane ? TO_PLANE : TO_C8];
    if (!launch) return fail(SNVC_ERR_UNSUPPORTED, p.form->unsupported);
    launch(a, g, as_stream(stream));
    return check_launch("snvc_f16_conv3d_forward");
}

// One call of a split layer: what the five entry points below set, everything else null or zero.
struct F16x3Call {
    const void *x_hi = nullptr, *x_lo = nullptr, *packed_weight = nullptr;
    const float *scale = nullptr, *bias = nullptr;
    const void *res_hi = nullptr, *res_lo = nullptr;      // the split residual of ADD_PRE / ADD_POST
    const float *res_f32 = nullptr;                       // a float32 result's float32 NCDHW residual (added after the activation, no flag)
    void *y_hi = nullptr, *y_lo = nullptr;
    float *y_f32 = nullptr;
    const float *head = nullptr;
    float *y_head = nullptr;
    float head_mul = 0.0f, res_mul = 0.0f;
    int *overflow = nullptr;
    const void *tail_w = nullptr;                         // EPI 4: the result is contracted with a one-channel transposed layer's taps, not stored
    float *t_out = nullptr;
    float tail_mul = 0.0f;
    double *stats = nullptr;                              // the statistics epilogue's workspace; stats_slots: its slots per sample (out)
    int64_t *stats_slots = nullptr;
    const float *x_mul = nullptr;
    const snvc::F16SrcArgs *src = nullptr;                // the fused sheared first layer: the image's producer
    const snvc_wedge_desc *in_alias = nullptr;            // the input pair's duplicate wedge tiles were not written (snvc_alias.h)
    bool hg_skip = false;                                 // with in_alias: the result's own duplicate tiles are not computed (snvc_hgdedup.h)
    const snvc_wedge_desc *hg_in = nullptr;               // the input pair is such a result; hg_in: the descriptor its producer was given
    void *stream = nullptr;
};

static int f16x3_forward(const snvc_conv3d_desc *d, const F16x3Call &c) {
    using namespace snvc;
    F16Plan p;
    if (!d) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: null desc");
    int rc = make_f16_plan(*d, p, true);
    if (rc) return rc;
    if (d->N == 0) return SNVC_OK;
    const F16Form &f = *p.form;
    const bool tail = c.tail_w != nullptr;
    if (tail && (!c.t_out || !f.launch[TO_TAIL] || p.cblocks != 1 || d->Cout != 32 * f.MI || (reinterpret_cast<uintptr_t>(c.tail_w) & 15)))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_deconv3d_tail_forward: a transposed split layer whose 32 or 64 output channels sit in one block");
    const bool plane = d->Cout == 1;              // the occupancy head: y_f32 is then the fp32 plane [N][1][D][H][W] (Sigmoid honoured)
    const bool to_f32 = c.y_f32 != nullptr;
    if (plane && !to_f32) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: a one-channel layer writes y_f32");
    if ((!c.src && (!c.x_hi || !c.x_lo)) || !c.packed_weight || (!tail && !to_f32 && (!c.y_hi || !c.y_lo)))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: null pointer");
    if ((c.scale == nullptr) != (c.bias == nullptr))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: scale and bias must both be given or both be NULL");
    // r6: a float32 result takes a float32 NCDHW residual of its own shape and batch stride, added after the activation: it stands for
    // ADD_POST (the data gradients of the training step add a skip connection's gradient this way)
    const int flags = c.res_f32 ? (d->flags & ~SNVC_EPI_ADD_POST) : d->flags;
    const int resflags = flags & (SNVC_EPI_ADD_PRE | SNVC_EPI_ADD_POST);
    if (c.res_f32 && !plane && d->res_batch_stride && d->res_batch_stride != (d->y_batch_stride ? d->y_batch_stride : (int64_t)d->Cout * d->Dout * d->Hout * d->Wout))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: a float32 residual shares the result's batch stride");
    if ((resflags && (!c.res_hi || !c.res_lo)) || ((resflags || c.res_f32) && plane))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: residual flag without a split residual");
    if (resflags == (SNVC_EPI_ADD_PRE | SNVC_EPI_ADD_POST))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: ADD_PRE and ADD_POST are exclusive");
    if (d->flags & ~(SNVC_EPI_RELU | SNVC_EPI_ADD_PRE | SNVC_EPI_ADD_POST | (plane ? SNVC_EPI_SIGMOID : 0)))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d_forward: RELU / ADD_PRE / ADD_POST only (SIGMOID with the one-channel output)");
    if ((c.head != nullptr) != (c.y_head != nullptr))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: head and y_head go together");
    if (c.head && (!f.launch[TO_HEAD] || d->Cout != 32 || to_f32))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d_forward: the side head is built for 32-channel stride-1 layers with a split output");
    const int64_t in_sp = (int64_t)d->Din * d->Hin * d->Win, out_sp = (int64_t)d->Dout * d->Hout * d->Wout;
    if ((int64_t)(d->Cin / 8 + 2) * in_sp >= ((int64_t)1 << 31) || out_sp >= ((int64_t)1 << 31))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d_forward: one sample must stay below 2^31 pieces");
    if ((reinterpret_cast<uintptr_t>(c.x_hi) | reinterpret_cast<uintptr_t>(c.x_lo) | reinterpret_cast<uintptr_t>(c.y_hi) |
         reinterpret_cast<uintptr_t>(c.y_lo) | reinterpret_cast<uintptr_t>(c.res_hi) | reinterpret_cast<uintptr_t>(c.res_lo) |
         reinterpret_cast<uintptr_t>(c.packed_weight) | reinterpret_cast<uintptr_t>(c.scale) | reinterpret_cast<uintptr_t>(c.bias) |
         reinterpret_cast<uintptr_t>(c.head)) & 15)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: C8 tensors and the per-channel vectors must be 16-byte aligned");
    if ((d->x_batch_stride | (c.res_f32 ? 0 : d->res_batch_stride)) % 8 || (!to_f32 && d->y_batch_stride % 8))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward: batch strides must be multiples of 8 elements");
    F16SrcArgs b{};             // an F16Args for every form; the fused source's fields behind it
    if (c.src) b = *c.src;
    F16Args &a = b;
    a = F16Args{};
    a.x = reinterpret_cast<const _Float16 *>(c.x_hi); a.x_lo = reinterpret_cast<const _Float16 *>(c.x_lo);
    a.wp = reinterpret_cast<const _Float16 *>(c.packed_weight);
    a.scale = c.scale; a.bias = c.bias;
    a.res = resflags ? reinterpret_cast<const _Float16 *>(c.res_hi) : nullptr;
    a.res_lo = resflags ? reinterpret_cast<const _Float16 *>(c.res_lo) : nullptr;
    a.y = reinterpret_cast<_Float16 *>(c.y_hi); a.y_lo = reinterpret_cast<_Float16 *>(c.y_lo); a.y_f32 = c.y_f32;
    a.head = c.head; a.y_head = c.y_head; a.head_mul = c.head_mul; a.res_mul = c.res_mul; a.overflow = c.overflow;
    a.res_f32 = c.res_f32;
    a.stats = c.stats;
    a.x_mul = to_f32 ? c.x_mul : nullptr;
    a.tail_w = reinterpret_cast<const _Float16 *>(c.tail_w); a.t_out = c.t_out; a.tail_mul = c.tail_mul;
    a.t_bs = (int64_t)27 * 8 * d->Din * d->Hin * d->Win;
    a.CGin = d->Cin / 8; a.Cout = d->Cout;
    a.Din = d->Din; a.Hin = d->Hin; a.Win = d->Win;
    a.Dout = d->Dout; a.Hout = d->Hout; a.Wout = d->Wout;
    a.nchunks = p.nchunks; a.flags = flags;
    a.x_bs = d->x_batch_stride ? d->x_batch_stride : 2 * (int64_t)d->Cin * in_sp;
    a.y_bs = d->y_batch_stride ? d->y_batch_stride : 2 * (int64_t)d->Cout * out_sp;
    a.r_bs = d->res_batch_stride ? d->res_batch_stride : 2 * (int64_t)d->Cout * out_sp;
    a.yf_bs = plane ? out_sp : (d->y_batch_stride ? d->y_batch_stride : (int64_t)d->Cout * out_sp);
    const F16Geom g = f16_geometry(*d, p, a);
    if (g.ntiles >= ((int64_t)1 << 30) || (int64_t)d->N * g.classes > 65535)
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d_forward: too many tiles or samples");
    hipStream_t st = as_stream(c.stream);
    if (c.stats_slots) {        // the statistics epilogue (r6): only the forms that write float32 through the shared epilogue, 256 threads
        if (!(to_f32 && !plane && !tail && f.stats))
            return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d_forward_stats: this layer's kernel form has no statistics epilogue");
        *c.stats_slots = g.stats_slots;
        if (!c.stats) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward_stats: null workspace");
        // whole tiles outside a smaller parity class return early: their slots must read as zero (one class: every workgroup writes its slots)
        if (g.classes > 1) {
            const hipError_t e = hipMemsetAsync(c.stats, 0, (size_t)d->N * g.stats_slots * ((d->Cout + 31) / 32) * 64 * sizeof(double), st);
            if (e != hipSuccess) return fail(SNVC_ERR_HIP, "snvc_f16x3_conv3d_forward_stats: hipMemsetAsync failed");
        }
    }
    if (c.src && !f.launch[TO_SRC])
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_fused_first_conv3d_forward: a 3x3x3 stride-1 layer on the 16x16x32 form (SNVC_ALGO_X3_Q16)");
    const F16Call call = tail ? TO_TAIL : plane ? TO_PLANE : to_f32 ? TO_F32 : c.head ? (c.src ? TO_SRC_HEAD : TO_HEAD) : (c.src ? TO_SRC : TO_C8);
    if (!f.launch[call] || (resflags && !f.split_res)) return fail(SNVC_ERR_UNSUPPORTED, f.unsupported);
    if (g.jobs >= ((int64_t)1 << 30)) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d_forward: too many tiles");
    if (c.src && to_f32) return fail(SNVC_ERR_UNSUPPORTED, "snvc_fused_first_conv3d_forward: a split C8 output");
    // the wedge's duplicate tiles are skipped and copied back only where the copy is all 16-byte accesses (the side head's rows: W % 4
    // == 0) and there is a duplicate at all; otherwise the launch computes every tile.  SRC_NO_COPY: nothing is copied, so only the
    // second condition counts (a reader that aliases is right either way: computed duplicates hold the representative's bits)
    if ((b.v_flags & SRC_DEDUP) && ((!(b.v_flags & SRC_NO_COPY) && c.y_head && (d->Wout % 4 || (reinterpret_cast<uintptr_t>(c.y_head) & 15))) ||
                                    wedge_ranges(a.Din, a.Win, b.v_q, b.v_m0, b.v_off, nullptr, nullptr, 0).dups == 0))
        b.v_flags &= ~SRC_DEDUP;
    if (c.hg_skip) {            // the stride-2 layer behind conv2: <1>'s read, and its own duplicate tiles are no jobs of the walk
        if (!c.in_alias || &f != &FORM_K3S2XQ || call != TO_C8)
            return fail(SNVC_ERR_UNSUPPORTED, "snvc_hgdedup_f16x3_conv3d_forward: built for the stride-2 3x3x3 layer on the 16x16x32 form (SNVC_ALGO_X3_Q16) with a split C8 result");
        if (c.in_alias->D != d->Din || c.in_alias->W != d->Win || (c.in_alias->q != 1 && c.in_alias->q != 2))
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_f16x3_conv3d_forward: in_alias describes a [Din][.][Win] tensor, q = 1 | 2");
        int64_t first[1], last[1];
        if (hg_ranges(*c.in_alias, first, last, 0).ncols > HG_COLS)
            return fail(SNVC_ERR_UNSUPPORTED, "snvc_hgdedup_f16x3_conv3d_forward: more tile columns with duplicates than the live walk has runs (snvc_hgdedup_max_columns)");
        F16LiveArgs lv{};
        static_cast<F16Args &>(lv) = a;
        lv.in_alias = *c.in_alias;
        if (!hg_live_walk(lv.in_alias, a.tiles_d, a.tiles_h, a.tiles_w, lv.live)) {      // no duplicate: the aliased launch itself
            launch_x3s2q_alias(lv, g, st);
        } else {
            F16Geom gl = g;
            gl.jobs = (int64_t)lv.live.live_tiles * p.cblocks * d->N;
            launch_x3s2q_live(lv, gl, st);
        }
        return check_launch("snvc_hgdedup_f16x3_conv3d_forward");
    }
    if (c.hg_in) {              // the stride-1 layer behind it: the remap sits in the image fill's geometry, every tile is computed and written
        if (&f != &FORM_K3XQ || call != TO_C8 || resflags)
            return fail(SNVC_ERR_UNSUPPORTED, "snvc_hgdedup_reader_f16x3_conv3d_forward: built for the stride-1 3x3x3 layer on the 16x16x32 form (SNVC_ALGO_X3_Q16) with a split C8 result, no residual");
        if ((c.hg_in->D - 1) / 2 + 1 != d->Din || (c.hg_in->W - 1) / 2 + 1 != d->Win || c.hg_in->D < 1 || c.hg_in->W < 1 || (c.hg_in->q != 1 && c.hg_in->q != 2))
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_reader_f16x3_conv3d_forward: in_desc describes the [2 Din][.][2 Win] tensor in front of the stride-2 layer, q = 1 | 2");
        int64_t first[1], last[1];
        if (hg_ranges(*c.hg_in, first, last, 0).dups == 0) {      // every row was written
            f.launch[call](b, g, st);
        } else {
            F16AliasArgs al{};
            static_cast<F16Args &>(al) = a;
            al.in_alias = *c.hg_in;
            launch_x3q_hg_alias(al, g, st);
        }
        return check_launch("snvc_hgdedup_reader_f16x3_conv3d_forward");
    }
    if (c.in_alias) {           // one reader form is built; the aliased rows are whole rows of the representative's plane: nothing else moves
        if (&f != &FORM_K3S2XQ || call != TO_C8)
            return fail(SNVC_ERR_UNSUPPORTED, "snvc_alias_f16x3_conv3d_forward: built for the stride-2 3x3x3 layer on the 16x16x32 form (SNVC_ALGO_X3_Q16) with a split C8 result");
        if (c.in_alias->D != d->Din || c.in_alias->W != d->Win || (c.in_alias->q != 1 && c.in_alias->q != 2))
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_alias_f16x3_conv3d_forward: in_alias describes a [Din][.][Win] tensor, q = 1 | 2");
        F16AliasArgs al{};
        static_cast<F16Args &>(al) = a;
        al.in_alias = *c.in_alias;
        launch_x3s2q_alias(al, g, st);
        return check_launch("snvc_alias_f16x3_conv3d_forward");
    }
    f.launch[call](b, g, st);
    if ((b.v_flags & SRC_DEDUP) && !(b.v_flags & SRC_NO_COPY)) launch_wedge_copy(b, st);
    return check_launch("snvc_f16x3_conv3d_forward");
}

int snvc_f16x3_conv3d_forward(const snvc_conv3d_desc *d, const void *x_hi, const void *x_lo, const void *packed_weight,
                              const float *scale, const float *bias, const void *res_hi, const void *res_lo, void *y_hi,
                              void *y_lo, float *y_f32, const float *head, float *y_head, float head_mul, float res_mul,
                              int *overflow, void *stream) {
    F16x3Call c;
    c.x_hi = x_hi; c.x_lo = x_lo; c.packed_weight = packed_weight; c.scale = scale; c.bias = bias;
    c.res_hi = res_hi; c.res_lo = res_lo; c.y_hi = y_hi; c.y_lo = y_lo; c.y_f32 = y_f32;
    c.head = head; c.y_head = y_head; c.head_mul = head_mul; c.res_mul = res_mul; c.overflow = overflow; c.stream = stream;
    // r6: with y_f32 and ADD_POST alone, res_hi without res_lo is the float32 residual (include/snvc_hip.h)
    if (d && (d->flags & (SNVC_EPI_ADD_PRE | SNVC_EPI_ADD_POST)) == SNVC_EPI_ADD_POST && y_f32 && d->Cout != 1 && res_hi && !res_lo) {
        c.res_f32 = static_cast<const float *>(res_hi);
        c.res_hi = nullptr;
    }
    return f16x3_forward(d, c);
}

// snvc_fused_first_conv3d_forward | snvc_dedup_fused_first_conv3d_forward (dedup: the wedge's duplicate tiles are copied, not computed)
static int fused_first_forward(const snvc_conv3d_desc *d, const void *packed_weight, const float *scale, const float *bias, void *y_hi,
                               void *y_lo, const float *head, float *y_head, float head_mul, int *overflow, const float *gi,
                               int64_t pitch, int64_t lp, const float *p_il, const float *v_scale, const float *v_bias, int q, int m0,
                               int off, int off2, int v_flags, int dedup, void *stream) {      // dedup: 0 | SRC_DEDUP | SRC_DEDUP | SRC_NO_COPY
    using namespace snvc;
    if (!d || !gi || !p_il || !v_scale || !v_bias) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fused_first_conv3d_forward: null pointer");
    if (d->transposed || d->ksize != 3 || d->stride != 1 || d->pad != 1 || d->dilation != 1 || d->Cin % 8 || d->Din < 1 || d->Hin < 1 || d->Win < 1 ||
        (q != 1 && q != 2) || (v_flags & ~SNVC_EPI_RELU))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_fused_first_conv3d_forward: a 3x3x3 / stride 1 / pad 1 layer, Cin % 8 == 0, q = 1 | 2");
    if ((reinterpret_cast<uintptr_t>(gi) | reinterpret_cast<uintptr_t>(p_il) | reinterpret_cast<uintptr_t>(v_scale) | reinterpret_cast<uintptr_t>(v_bias)) & 31)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fused_first_conv3d_forward: gi / p_il / v_scale / v_bias must be 32-byte aligned");
    // every G | G' index of a voxel of the tensor stays inside a (zero-padded) row of gi
    const int64_t D = d->Din, H = d->Hin, W = d->Win, CG = d->Cin / 8;
    const int64_t lo_g = -(D - 1) - m0 + off, hi_g = (int64_t)q * (W - 2) - m0 + off;
    const int64_t lo_c = (int64_t)q * (W - 1) - (D - 1) - m0 + off2, hi_c = (int64_t)q * (W - 1) - m0 + off2;
    if (lp < 0 || pitch <= 0 || lp + lo_c < 0 || lp + hi_c >= pitch || (W > 1 && (lp + lo_g < 0 || lp + hi_g >= pitch)))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fused_first_conv3d_forward: pitch / lp do not cover the G indices of this shape");
    if (6 * CG * H * pitch * 32 >= ((int64_t)1 << 31) || 3 * CG * H * W * 32 >= ((int64_t)1 << 31))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_fused_first_conv3d_forward: one sample of gi / p_il must stay below 2 GiB");
    F16SrcArgs s{};
    s.gi = gi; s.p_il = p_il; s.v_scale = v_scale; s.v_bias = v_bias; s.gi_bs = 6 * CG * H * pitch * 8;
    s.v_pitch = (int)pitch; s.v_lp = (int)lp; s.v_q = q; s.v_m0 = m0; s.v_off = off; s.v_off2 = off2;
    s.v_flags = v_flags | dedup;
    F16x3Call c;
    c.packed_weight = packed_weight; c.scale = scale; c.bias = bias; c.y_hi = y_hi; c.y_lo = y_lo;
    c.head = head; c.y_head = y_head; c.head_mul = head_mul; c.res_mul = 1.0f; c.overflow = overflow; c.src = &s; c.stream = stream;
    return f16x3_forward(d, c);
}

int snvc_fused_first_conv3d_forward(const snvc_conv3d_desc *d, const void *packed_weight, const float *scale, const float *bias, void *y_hi,
                                    void *y_lo, const float *head, float *y_head, float head_mul, int *overflow, const float *gi,
                                    int64_t pitch, int64_t lp, const float *p_il, const float *v_scale, const float *v_bias, int q, int m0,
                                    int off, int off2, int v_flags, void *stream) {
    return fused_first_forward(d, packed_weight, scale, bias, y_hi, y_lo, head, y_head, head_mul, overflow, gi, pitch, lp, p_il, v_scale, v_bias,
                               q, m0, off, off2, v_flags, 0, stream);
}

int snvc_dedup_abi_version(void) { return 1; }

int snvc_dedup_fused_first_conv3d_forward(const snvc_conv3d_desc *d, const void *packed_weight, const float *scale, const float *bias,
                                          void *y_hi, void *y_lo, const float *head, float *y_head, float head_mul, int *overflow,
                                          const float *gi, int64_t pitch, int64_t lp, const float *p_il, const float *v_scale,
                                          const float *v_bias, int q, int m0, int off, int off2, int v_flags, void *stream) {
    return fused_first_forward(d, packed_weight, scale, bias, y_hi, y_lo, head, y_head, head_mul, overflow, gi, pitch, lp, p_il, v_scale, v_bias,
                               q, m0, off, off2, v_flags, snvc::SRC_DEDUP, stream);
}

int64_t snvc_dedup_fused_first_tiles(const snvc_conv3d_desc *d, int q, int m0, int off, int64_t *first_td, int64_t *last_td, int max_tw) {
    using namespace snvc;
    if (!d || d->Din < 1 || d->Win < 1 || (q != 1 && q != 2) || max_tw < 0 || (max_tw > 0 && (!first_td || !last_td))) {
        fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_dedup_fused_first_tiles: a desc, q = 1 | 2, and max_tw entries to write");
        return -1;
    }
    for (int tw = 0; tw < max_tw; ++tw) first_td[tw] = last_td[tw] = -1;
    return wedge_ranges((int)d->Din, (int)d->Win, q, m0, off, first_td, last_td, max_tw).dups;
}

// ---- include/snvc_alias.h: the duplicates are neither computed nor copied; the readers look at the representative's rows
int snvc_alias_abi_version(void) { return 1; }

int64_t snvc_alias_depth(const snvc_wedge_desc *w, int64_t d, int64_t x) {
    using namespace snvc;
    if (!w || (w->q != 1 && w->q != 2) || d < 0 || d >= w->D || x < 0 || x >= w->W) {
        fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_alias_depth: a desc with q = 1 | 2 and (d, w) inside [0, D) x [0, W)");
        return -1;
    }
    return wedge_alias_depth(*w, (int)d, (int)x);
}

int snvc_alias_fused_first_conv3d_forward(const snvc_conv3d_desc *d, const void *packed_weight, const float *scale, const float *bias,
                                          void *y_hi, void *y_lo, const float *head, float *y_head, float head_mul, int *overflow,
                                          const float *gi, int64_t pitch, int64_t lp, const float *p_il, const float *v_scale,
                                          const float *v_bias, int q, int m0, int off, int off2, int v_flags, void *stream) {
    return fused_first_forward(d, packed_weight, scale, bias, y_hi, y_lo, head, y_head, head_mul, overflow, gi, pitch, lp, p_il, v_scale, v_bias,
                               q, m0, off, off2, v_flags, snvc::SRC_DEDUP | snvc::SRC_NO_COPY, stream);
}

int snvc_alias_f16x3_conv3d_forward(const snvc_conv3d_desc *d, const void *x_hi, const void *x_lo, const void *packed_weight,
                                    const float *scale, const float *bias, void *y_hi, void *y_lo, int *overflow,
                                    const snvc_wedge_desc *in_alias, void *stream) {
    F16x3Call c;
    c.x_hi = x_hi; c.x_lo = x_lo; c.packed_weight = packed_weight; c.scale = scale; c.bias = bias;
    c.y_hi = y_hi; c.y_lo = y_lo; c.head_mul = 1.0f; c.res_mul = 1.0f; c.overflow = overflow; c.in_alias = in_alias; c.stream = stream;
    return f16x3_forward(d, c);
}

// ---- include/snvc_hgdedup.h: the hourglass's first stride-2 layer does not compute its own duplicates; the stride-1 layer behind it aliases
int snvc_hgdedup_abi_version(void) { return 1; }
int snvc_hgdedup_max_columns(void) { return snvc::HG_COLS; }

static bool hgdedup_desc_ok(const snvc_wedge_desc *w) { return w && w->D >= 1 && w->W >= 1 && (w->q == 1 || w->q == 2); }

int snvc_hgdedup_tile_pure(const snvc_wedge_desc *w, int64_t od0, int64_t ow0) {
    using namespace snvc;
    if (!hgdedup_desc_ok(w) || od0 < 0 || od0 >= (w->D - 1) / 2 + 1 || (od0 & 1) || ow0 < 0 || ow0 >= (w->W - 1) / 2 + 1 || (ow0 & 31)) {
        fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_tile_pure: a desc with q = 1 | 2 and a tile origin (od0 % 2 == 0, ow0 % 32 == 0) inside the stride-2 result");
        return -1;
    }
    return hg_tile_pure(*w, (int)od0, (int)ow0) ? 1 : 0;
}

int64_t snvc_hgdedup_tiles(const snvc_wedge_desc *w, int64_t *first_td, int64_t *last_td, int max_tw) {
    using namespace snvc;
    if (!hgdedup_desc_ok(w) || max_tw < 0 || (max_tw > 0 && (!first_td || !last_td))) {
        fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_tiles: a desc with q = 1 | 2, and max_tw entries to write");
        return -1;
    }
    return hg_ranges(*w, first_td, last_td, max_tw).dups;
}

int64_t snvc_hgdedup_depth(const snvc_wedge_desc *w, int64_t od, int64_t ow) {
    using namespace snvc;
    if (!hgdedup_desc_ok(w) || od < 0 || od >= (w->D - 1) / 2 + 1 || ow < 0 || ow >= (w->W - 1) / 2 + 1) {
        fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_depth: a desc with q = 1 | 2 and (od, ow) inside the stride-2 result [(D - 1) / 2 + 1) x [(W - 1) / 2 + 1)");
        return -1;
    }
    return hg_alias_depth(*w, (int)od, (int)ow);
}

int64_t snvc_hgdedup_live_tile(const snvc_wedge_desc *w, int64_t tiles_h, int64_t index, int64_t *td, int64_t *th, int64_t *tw) {
    using namespace snvc;
    HgLive lv{};
    if (!hgdedup_desc_ok(w) || tiles_h < 1 || tiles_h > 65535) {
        fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_live_tile: a desc with q = 1 | 2 and 1 .. 65535 tile rows");
        return -1;
    }
    const int tiles_d = ceil_div((w->D - 1) / 2 + 1, X3S2Cfg::TD), tiles_w = ceil_div((w->W - 1) / 2 + 1, 32);
    if (!hg_live_walk(*w, tiles_d, (int)tiles_h, tiles_w, lv)) return 0;
    if (index >= 0 && index < lv.live_tiles && td && th && tw) {
        int a, b, c;
        hg_live_tile(lv, (int)tiles_h, tiles_w, (int)index, a, b, c);
        *td = a; *th = b; *tw = c;
    }
    return lv.live_tiles;
}

int snvc_hgdedup_f16x3_conv3d_forward(const snvc_conv3d_desc *d,const void *x_hi, const void *x_lo, const void *packed_weight,
                                      const float *scale, const float *bias, void *y_hi, void *y_lo, int *overflow,
                                      const snvc_wedge_desc *in_alias, void *stream) {
    if (!in_alias) return snvc::fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_f16x3_conv3d_forward: null in_alias");
    F16x3Call c;
    c.x_hi = x_hi; c.x_lo = x_lo; c.packed_weight = packed_weight; c.scale = scale; c.bias = bias;
    c.y_hi = y_hi; c.y_lo = y_lo; c.head_mul = 1.0f; c.res_mul = 1.0f; c.overflow = overflow; c.in_alias = in_alias; c.hg_skip = true;
    c.stream = stream;
    return f16x3_forward(d, c);
}

int snvc_hgdedup_reader_f16x3_conv3d_forward(const snvc_conv3d_desc *d, const void *x_hi, const void *x_lo, const void *packed_weight,
                                             const float *scale, const float *bias, void *y_hi, void *y_lo, int *overflow,
                                             const snvc_wedge_desc *in_desc, void *stream) {
    if (!in_desc) return snvc::fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hgdedup_reader_f16x3_conv3d_forward: null in_desc");
    F16x3Call c;
    c.x_hi = x_hi; c.x_lo = x_lo; c.packed_weight = packed_weight; c.scale = scale; c.bias = bias;
    c.y_hi = y_hi; c.y_lo = y_lo; c.head_mul = 1.0f; c.res_mul = 1.0f; c.overflow = overflow; c.hg_in = in_desc; c.stream = stream;
    return f16x3_forward(d, c);
}

int64_t snvc_f16x3_conv3d_stats_workspace_bytes(const snvc_conv3d_desc *d) {
    using namespace snvc;
    F16Plan p;
    if (!d || d->N < 0 || make_f16_plan(*d, p, true)) return -1;
    const int64_t groups = (d->Cout + 31) / 32;
    F16Args a{};
    const int64_t slots = f16_geometry(*d, p, a).stats_slots;      // of the grid that f16x3_forward launches
    return (d->N * slots * groups * 64 + conv_stats_fold_scratch_doubles(d->N, (int)groups, slots) + d->N * (int64_t)d->Cout * 2) * (int64_t)sizeof(double);
}

int snvc_f16x3_conv3d_forward_f32(const snvc_conv3d_desc *d, const void *x_hi, const void *x_lo, const void *packed_weight,
                                  const float *scale, const float *bias, const float *x_mul, const float *res_f32, float *y_f32,
                                  float out_mul, void *stream) {
    using namespace snvc;
    if (!d || !y_f32) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward_f32: null pointer");
    if (d->flags & (SNVC_EPI_ADD_PRE | SNVC_EPI_ADD_POST)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward_f32: the residual is res_f32 (added after the activation), no flag");
    F16x3Call c;
    c.x_hi = x_hi; c.x_lo = x_lo; c.packed_weight = packed_weight; c.scale = scale; c.bias = bias; c.x_mul = x_mul;
    c.res_f32 = res_f32; c.y_f32 = y_f32; c.head_mul = out_mul; c.res_mul = 1.0f; c.stream = stream;
    return f16x3_forward(d, c);
}

int snvc_f16x3_conv3d_forward_stats(const snvc_conv3d_desc *d, const void *x_hi, const void *x_lo, const void *packed_weight,
                                    const float *scale, const float *bias, const float *x_mul, float *y_f32, float head_mul, const float *gamma,
                                    const float *beta, float *bn_scale, float *bn_shift, float *mean, float *var, void *workspace,
                                    float eps, void *stream) {
    using namespace snvc;
    if (!d || !y_f32 || !bn_scale || !bn_shift || !workspace)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv3d_forward_stats: null pointer");
    if (d->N <= 0 || d->flags || d->Cout % 32) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv3d_forward_stats: whole 32-channel groups, no epilogue flags");
    double *stats = static_cast<double *>(workspace);
    int64_t slots = 0;
    F16x3Call c;
    c.x_hi = x_hi; c.x_lo = x_lo; c.packed_weight = packed_weight; c.scale = scale; c.bias = bias; c.x_mul = x_mul;
    c.y_f32 = y_f32; c.head_mul = head_mul; c.res_mul = 1.0f; c.stats = stats; c.stats_slots = &slots; c.stream = stream;
    int rc = f16x3_forward(d, c);
    if (rc) return rc;
    const int groups = d->Cout / 32;
    double *scratch = stats + d->N * slots * groups * 64;
    double *partial = scratch + conv_stats_fold_scratch_doubles(d->N, groups, slots);
    launch_conv_stats_fold(stats, scratch, partial, d->N, d->Cout, groups, slots, as_stream(stream));
    rc = check_launch("snvc_f16x3_conv3d_forward_stats(fold)");
    if (rc) return rc;
    launch_norm_finalize(partial, gamma, beta, bn_scale, bn_shift, mean, var, d->N, d->Cout, (int64_t)d->Dout * d->Hout * d->Wout, 1, eps,
                         as_stream(stream));
    return check_launch("snvc_f16x3_conv3d_forward_stats(finalize)");
}

// workgroups of a scale launch over n floats (split_scale_kernel: few workgroups, the launch's time is its chain of atomics)
static int split_scale_blocks(int64_t n) {
    const int64_t blocks = snvc::ceil_div<int64_t>(n > 0 ? n : 1, 256 * 4 * 16);
    return (int)(blocks < 1 ? 1 : (blocks > 48 ? 48 : blocks));
}

int snvc_f16x3_split_scale(const float *x, int64_t n, void *scratch8, float *out_mul, void *stream) {
    using namespace snvc;
    if (n < 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_split_scale: negative size");
    if (!out_mul || !scratch8 || (n > 0 && !x)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_split_scale: null pointer");
    if (reinterpret_cast<uintptr_t>(x) & 15) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_split_scale: x must be 16-byte aligned");
    const int blocks = split_scale_blocks(n);
    split_scale_kernel<<<blocks, 256, 0, as_stream(stream)>>>(x, n, reinterpret_cast<unsigned *>(scratch8), out_mul);
    return check_launch("snvc_f16x3_split_scale");
}

// ---- depth-1 (2D) split layers: 3x7 and 3x3, stride 1, "same" padding, Cin % 8 == 0, Cout % 32 == 0
static int x2q_nq(int kh, int kw) { return (kh * kw + 3) / 4; }

int64_t snvc_f16x3_conv2d_packed_weight_bytes(int cout, int cin, int kh, int kw) {
    if (cout <= 0 || cin <= 0 || cout % 32 || cin % 8 || kh != 3 || (kw != 3 && kw != 7)) return -1;
    return 2 * ((int64_t)(cout / 32) * (cin / 8) * x2q_nq(kh, kw) + 2) * 4 * 64 * 8;      // + the weight ring's read-ahead
}

int snvc_f16x3_conv2d_pack_weights(const float *weight, int cout, int cin, int kh, int kw, void *packed, float wmul, void *stream) {
    using namespace snvc;
    const int64_t bytes = snvc_f16x3_conv2d_packed_weight_bytes(cout, cin, kh, kw);
    if (bytes < 0) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv2d: 3x7 or 3x3 kernels, Cin % 8 == 0, Cout % 32 == 0");
    if (!weight || !packed) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv2d_pack_weights: null pointer");
    if (hipMemsetAsync(packed, 0, (size_t)bytes, as_stream(stream)) != hipSuccess)
        return fail(SNVC_ERR_HIP, "snvc_f16x3_conv2d_pack_weights: hipMemsetAsync failed");
    const int nq = x2q_nq(kh, kw);
    const int64_t total = (int64_t)(cout / 32) * (cin / 8) * nq * 4 * 64 * 8;
    // [cb][chunk][quad][co half][hi | lo][lane][8] over the (kh, kw) raster: the 3x3x3 form's layout with K3 = kh * kw taps
    pack_q16({kh * kw, 1, nq, 2, 2, 1}, weight, packed, cout, cin, wmul, total, as_stream(stream));
    return check_launch("snvc_f16x3_conv2d_pack_weights");
}

// the interleaved second output of a depth-1 layer (include/snvc_fused.h): C = Cout / 3 channels in 3 classes
struct snvc_il_out {
    float *y_il;
    int64_t bs, pitch, lp, cls0, classes;
    int mode;
};

static int fail_as(int code, const char *who, const char *what) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return snvc::fail(code, msg);
}

// Checks a depth-1 layer's call and fills its argument record (b; the il fields only with `il`) and its jobs per sample (0: N == 0,
// nothing to launch) -- no launch: f16x3_conv2d_forward queues the layer's own launch behind it, snvc_prep_pooled_x3 pools three
// records.  `who` / `who_il` name the entry point in the messages.
static int f16x3_conv2d_setup(const char *who, const char *who_il, const void *x_hi, const void *x_lo, const void *packed_weight,
                              const float *scale, const float *bias, float *y, int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int kh,
                              int kw, float out_mul, const float *x_mul_dev, int flags, const snvc_il_out *il, snvc::F16IlArgs &b,
                              int64_t &jobs) {
    using namespace snvc;
    jobs = 0;
    if (N < 0 || H <= 0 || W <= 0 || snvc_f16x3_conv2d_packed_weight_bytes((int)Cout, (int)Cin, kh, kw) < 0)
        return fail_as(SNVC_ERR_UNSUPPORTED, who, "3x7 or 3x3 kernels, Cin % 8 == 0, Cout % 32 == 0");
    if (N == 0) return SNVC_OK;
    if (!x_hi || !x_lo || !packed_weight || !y) return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "null pointer");
    if ((scale == nullptr) != (bias == nullptr))
        return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "scale and bias must both be given or both be NULL");
    if (flags & ~SNVC_EPI_RELU) return fail_as(SNVC_ERR_UNSUPPORTED, who, "only SNVC_EPI_RELU");
    if ((reinterpret_cast<uintptr_t>(x_hi) | reinterpret_cast<uintptr_t>(x_lo) | reinterpret_cast<uintptr_t>(packed_weight)) & 15)
        return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "C8 tensors must be 16-byte aligned");
    const int64_t hw = H * W;
    if ((Cin / 8 + 2) * hw >= ((int64_t)1 << 31) || N > 65535) return fail_as(SNVC_ERR_UNSUPPORTED, who, "tensor too large");
    F16Args a{};
    a.x = reinterpret_cast<const _Float16 *>(x_hi); a.x_lo = reinterpret_cast<const _Float16 *>(x_lo);
    a.wp = reinterpret_cast<const _Float16 *>(packed_weight);
    a.scale = scale; a.bias = bias; a.y_f32 = y; a.head_mul = out_mul; a.x_mul = x_mul_dev;
    a.CGin = (int)(Cin / 8); a.Cout = (int)Cout; a.nchunks = (int)(Cin / 8); a.flags = flags;
    a.Din = a.Dout = 1; a.Hin = a.Hout = (int)H; a.Win = a.Wout = (int)W;
    a.nd = 1; a.nh = (int)H; a.nw = (int)W;
    a.pad_d = 0; a.pad_h = (kh - 1) / 2; a.pad_w = (kw - 1) / 2;
    a.tiles_d = 1; a.tiles_h = (int)ceil_div<int64_t>(H, 16); a.tiles_w = (int)ceil_div<int64_t>(W, 32);
    a.x_bs = 2 * Cin * hw; a.yf_bs = Cout * hw; a.N = (int)N;
    const int64_t nj = (int64_t)a.tiles_h * a.tiles_w * (Cout / 32);
    if (nj >= ((int64_t)1 << 30)) return fail_as(SNVC_ERR_UNSUPPORTED, who, "too many tiles");
    b = F16IlArgs{};
    static_cast<F16Args &>(b) = a;
    if (il) {
        const int64_t C = Cout / 3, need = il->classes * ((C + 7) / 8) * H * il->pitch * 8;
        if (!il->y_il || Cout % 3 || il->mode < 0 || il->mode > 2 || (il->mode != 1 && C % 8) || il->lp < 0 || il->lp + W > il->pitch || il->cls0 < 0 || il->cls0 + 3 > il->classes ||
            need > il->bs || need >= ((int64_t)1 << 31) || (reinterpret_cast<uintptr_t>(il->y_il) & 31) || il->bs % 8)
            return fail_as(SNVC_ERR_INVALID_ARGUMENT, who_il, "the interleaved output does not hold the layer's result");
        b.y_il = il->y_il; b.il_bs = il->bs; b.il_mode = il->mode; b.il_C = (int)C; b.il_pitch = (int)il->pitch; b.il_lp = (int)il->lp;
        b.il_cls0 = (int)il->cls0;
    }
    jobs = nj;
    return SNVC_OK;
}

static int f16x3_conv2d_forward(const void *x_hi, const void *x_lo, const void *packed_weight, const float *scale, const float *bias,
                                float *y, int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int kh, int kw, float out_mul,
                                const float *x_mul_dev, int flags, void *stream, const snvc_il_out *il) {
    using namespace snvc;
    F16IlArgs b;
    int64_t jobs;
    const int rc = f16x3_conv2d_setup("snvc_f16x3_conv2d_forward", "snvc_fused", x_hi, x_lo, packed_weight, scale, bias, y, N, Cin, Cout, H, W, kh, kw,
                                      out_mul, x_mul_dev, flags, il, b, jobs);
    if (rc || !jobs) return rc;
    const F16Args &a = b;
    const dim3 grid((unsigned)jobs, 1, (unsigned)N);
    hipStream_t st = as_stream(stream);
    if (il) {
        if (kw == 7) {
            using C7 = X2QCfg<3, 7>;
            launch_lds<conv2d_x3q_kernel<C7, 1>>(grid, 256, C7::LDS_BYTES, st, b);
        } else {
            using C3 = X2QCfg<3, 3>;
            launch_lds<conv2d_x3q_kernel<C3, 1>>(grid, 256, C3::LDS_BYTES, st, b);
        }
    } else if (kw == 7) {
        using C = X2QCfg<3, 7>;
        launch_lds<conv2d_x3q_kernel<C>>(grid, 256, C::LDS_BYTES, st, a);
    } else {
        using C = X2QCfg<3, 3>;
        launch_lds<conv2d_x3q_kernel<C>>(grid, 256, C::LDS_BYTES, st, a);
    }
    return check_launch("snvc_f16x3_conv2d_forward");
}

int snvc_f16x3_conv2d_forward(const void *x_hi, const void *x_lo, const void *packed_weight, const float *scale, const float *bias,
                              float *y, int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int kh, int kw, float out_mul,
                              const float *x_mul_dev, int flags, void *stream) {
    return f16x3_conv2d_forward(x_hi, x_lo, packed_weight, scale, bias, y, N, Cin, Cout, H, W, kh, kw, out_mul, x_mul_dev, flags, stream, nullptr);
}

// The sheared first layer's whole 2D prep in ONE host call (five launches: scale, Rq -> G, Rq' -> G'): behind the step's one host
// sync the GPU is empty, and five Python-level launches of 5-20 us kernels starve it (measured: +0.08-0.14 ms per step against
// the same kernels queued by a host that runs ahead).
static int sheared_prep_x3(const float *right, int64_t N, int64_t C, int64_t H, int64_t W, int q, int64_t WU, int off, int64_t WU2, int off2,
                           const void *packed_g, const void *packed_col, int64_t Cout3, float out_mul_g, float out_mul_col, void *rq_split,
                           void *rq2_split, void *scratch8, float *mul_dev, float *g, float *gcol, void *stream, float *gi, int64_t pitch,
                           int64_t lp) {
    using namespace snvc;
    const int64_t gi_bs = 6 * (C / 8) * H * pitch * 8;
    const snvc_il_out il_g{gi, gi_bs, pitch, lp, 0, 6, 0}, il_col{gi, gi_bs, pitch, lp, 3, 6, 0};
    if (!right || !packed_g || !packed_col || !rq_split || !rq2_split || !scratch8 || !mul_dev || !g || !gcol)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_sheared_prep_x3: null pointer");
    if (N <= 0 || C % 8 || Cout3 % 32) return fail(SNVC_ERR_UNSUPPORTED, "snvc_sheared_prep_x3: C % 8 == 0, 3 * Cout % 32 == 0");
    int rc = snvc_f16x3_split_scale(right, N * C * H * W, scratch8, mul_dev, stream);
    if (rc) return rc;
    const int64_t G = C / 8;
    _Float16 *a = reinterpret_cast<_Float16 *>(rq_split), *b = reinterpret_cast<_Float16 *>(rq2_split);
    rc = snvc_sheared_upsample_split(right, a, a + G * H * WU * 8, mul_dev, N, C, H, W, q, WU, off, stream);
    if (rc) return rc;
    rc = f16x3_conv2d_forward(a, a + G * H * WU * 8, packed_g, nullptr, nullptr, g, N, C, Cout3, H, WU, 3, 7, out_mul_g, mul_dev, 0, stream,
                              gi ? &il_g : nullptr);
    if (rc) return rc;
    rc = snvc_sheared_upsample_split(right, b, b + G * H * WU2 * 8, mul_dev, N, C, H, W, q, WU2, off2, stream);
    if (rc) return rc;
    return f16x3_conv2d_forward(b, b + G * H * WU2 * 8, packed_col, nullptr, nullptr, gcol, N, C, Cout3, H, WU2, 3, 7, out_mul_col, mul_dev, 0,
                                stream, gi ? &il_col : nullptr);
}

int snvc_sheared_prep_x3(const float *right, int64_t N, int64_t C, int64_t H, int64_t W, int q, int64_t WU, int off, int64_t WU2, int off2,
                         const void *packed_g, const void *packed_col, int64_t Cout3, float out_mul_g, float out_mul_col, void *rq_split,
                         void *rq2_split, void *scratch8, float *mul_dev, float *g, float *gcol, void *stream) {
    return sheared_prep_x3(right, N, C, H, W, q, WU, off, WU2, off2, packed_g, packed_col, Cout3, out_mul_g, out_mul_col, rq_split, rq2_split,
                           scratch8, mul_dev, g, gcol, stream, nullptr, 0, 0);
}

int snvc_fused_sheared_prep_x3(const float *right, int64_t N, int64_t C, int64_t H, int64_t W, int q, int64_t WU, int off, int64_t WU2,
                               int off2, const void *packed_g, const void *packed_col, int64_t Cout3, float out_mul_g, float out_mul_col,
                               void *rq_split, void *rq2_split, void *scratch8, float *mul_dev, float *g, float *gcol, float *gi,
                               int64_t pitch, int64_t lp, void *stream) {
    if (!gi || Cout3 != 3 * C) return snvc::fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fused_sheared_prep_x3: gi is NULL or Cout3 != 3 * C");
    return sheared_prep_x3(right, N, C, H, W, q, WU, off, WU2, off2, packed_g, packed_col, Cout3, out_mul_g, out_mul_col, rq_split, rq2_split,
                           scratch8, mul_dev, g, gcol, stream, gi, pitch, lp);
}

int snvc_fused_abi_version(void) { return 1; }

int64_t snvc_fused_il_index(int mode, int64_t oc, int64_t C, int64_t H, int64_t pitch, int64_t lp, int64_t cls0, int64_t h, int64_t x) {
    if ((mode != 0 && mode != 1) || C <= 0 || oc < 0 || oc >= 3 * C || H <= 0 || h < 0 || h >= H || lp < 0 || x < 0 || lp + x >= pitch || cls0 < 0)
        return -1;
    return snvc::il_index<int64_t>(mode, oc, C, H, pitch, lp, cls0, h, x);
}

int snvc_fused_planes_from_f32(const float *x, int64_t N, int64_t C, int64_t H, int64_t W, const void *packed, int64_t cout, float out_mul,
                               float *y, float *p_il, void *ws_split, void *scratch8, float *mul_dev, void *stream) {
    using namespace snvc;
    if (!x || !packed || !y || !p_il || !ws_split || !scratch8 || !mul_dev)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fused_planes_from_f32: null pointer");
    if (N <= 0 || C % 8 || cout != 3 * C) return fail(SNVC_ERR_UNSUPPORTED, "snvc_fused_planes_from_f32: C % 8 == 0, cout == 3 * C");
    int rc = snvc_f16x3_split_scale(x, N * C * H * W, scratch8, mul_dev, stream);
    if (rc) return rc;
    _Float16 *a = reinterpret_cast<_Float16 *>(ws_split);
    rc = snvc_f16x3_from_ncdhw(x, a, a + C * H * W, N, C, H * W, 0, 0, 1.0f, mul_dev, stream);
    if (rc) return rc;
    const snvc_il_out il{p_il, 3 * (C / 8) * H * W * 8, W, 0, 0, 3, 1};
    return f16x3_conv2d_forward(a, a + C * H * W, packed, nullptr, nullptr, y, N, C, cout, H, W, 3, 3, out_mul, mul_dev, 0, stream, &il);
}

// ---- the pooled prep (include/snvc_prep.h)
int snvc_prep_abi_version(void) { return 1; }

int snvc_prep_pool_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t WU, int64_t WU2, snvc_prep_pool_plan_t *plan) {
    using namespace snvc;
    const char *who = "snvc_prep_pool_plan";
    if (!plan) return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "null pointer");
    if (N <= 0 || C <= 0 || C % 8 || (3 * C) % 32) return fail_as(SNVC_ERR_UNSUPPORTED, who, "N > 0, C % 8 == 0, 3 * C % 32 == 0");
    if (H <= 0 || W <= 0 || WU <= 0 || WU2 <= 0) return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "bad sizes");
    const int64_t G = C / 8, widths[3] = {WU, WU2, W};
    if (N > 65535 || G > 65535 || N * C * H * (WU > W ? (WU > WU2 ? WU : WU2) : (W > WU2 ? W : WU2)) >= ((int64_t)1 << 40))
        return fail_as(SNVC_ERR_UNSUPPORTED, who, "tensor too large");
    snvc_prep_pool_plan_t p{};
    p.a_blocks[0] = p.a_blocks[1] = split_scale_blocks(N * C * H * W);
    p.b_row_blocks = ceil_div<int64_t>(H * W, 256);
    for (int i = 0; i < 3; ++i) {
        p.b_items[i] = N * G * H * widths[i];
        p.b_blocks[i] = i < 2 ? ceil_div<int64_t>(p.b_items[i], 256) : N * G * p.b_row_blocks;
        p.c_jobs[i] = ceil_div<int64_t>(H, 16) * ceil_div<int64_t>(widths[i], 32) * (3 * C / 32);
    }
    p.c_samples = N;
    if (p.b_blocks[0] + p.b_blocks[1] + p.b_blocks[2] >= ((int64_t)1 << 31) || p.c_jobs[0] + p.c_jobs[1] + p.c_jobs[2] >= ((int64_t)1 << 30))
        return fail_as(SNVC_ERR_UNSUPPORTED, who, "too many blocks");
    *plan = p;
    return SNVC_OK;
}

int64_t snvc_prep_plain_plane(int64_t row, int64_t C) {
    return C > 0 && row >= 0 && row < 3 * C ? snvc::il_plain_plane<int64_t>(row, C) : -1;
}

int snvc_prep_pool_locate(const snvc_prep_pool_plan_t *plan, int stage, int64_t block, int64_t *local) {
    if (!plan || !local || stage < 0 || stage > 2 || block < 0) return -1;
    const int64_t *cnt = stage == 0 ? plan->a_blocks : stage == 1 ? plan->b_blocks : plan->c_jobs;
    const int64_t end0 = cnt[0], end1 = cnt[0] + cnt[1], end = end1 + (stage == 0 ? 0 : cnt[2]);
    if (block >= end) return -1;
    int l;
    const int sub = snvc::pool_range3((int)block, (int)end0, (int)end1, l);
    *local = l;
    return sub;
}

int snvc_prep_pooled_x3(const float *right, int64_t N, int64_t C, int64_t H, int64_t W, int q, int64_t WU, int off, int64_t WU2, int off2,
                        const void *packed_g, const void *packed_col, int64_t Cout3, float out_mul_g, float out_mul_col, void *rq_split,
                        void *rq2_split, float *mul_right, float *g, float *gcol, float *gi, int64_t pitch, int64_t lp, const float *left,
                        const void *packed_left, int64_t cout_left, float out_mul_left, float *planes, float *p_il, void *left_split,
                        float *mul_left, void *scratch16, int left_rows, int pool, void *stream) {
    using namespace snvc;
    const char *who = "snvc_prep_pooled_x3";
    // every check of snvc_fused_sheared_prep_x3 and snvc_fused_planes_from_f32 and of the calls they make, before the first launch
    if (!right || !packed_g || !packed_col || !rq_split || !rq2_split || !mul_right || !g || !gcol || !left || !packed_left || !planes || !p_il ||
        !left_split || !mul_left || !scratch16)
        return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "null pointer");
    if (!gi || Cout3 != 3 * C) return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "gi is NULL or Cout3 != 3 * C");
    if (N <= 0 || C <= 0 || C % 8 || Cout3 % 32 || cout_left != 3 * C)
        return fail_as(SNVC_ERR_UNSUPPORTED, who, "N > 0, C % 8 == 0, 3 * C % 32 == 0, cout_left == 3 * C");
    if (H <= 0 || W <= 0 || (q != 1 && q != 2) || WU <= 0 || WU2 <= 0) return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "bad sizes (q in {1,2})");
    if (pool & ~(SNVC_PREP_POOL_AB | SNVC_PREP_POOL_C)) return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "unknown pool bits");
    if (left_rows != 0 && left_rows != 1) return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "left_rows is 0 (class-minor) or 1 (class-major)");
    if ((reinterpret_cast<uintptr_t>(right) | reinterpret_cast<uintptr_t>(left)) & 15)
        return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "right / left must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(rq_split) | reinterpret_cast<uintptr_t>(rq2_split) | reinterpret_cast<uintptr_t>(left_split)) & 15)
        return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "the split workspaces must be 16-byte aligned");
    snvc_prep_pool_plan_t plan;
    int rc = snvc_prep_pool_plan(N, C, H, W, WU, WU2, &plan);
    if (rc) return fail_as(rc, who, "C % 8 == 0, 3 * C % 32 == 0, a shape whose three grids stay below their limits");
    const int64_t G = C / 8, S = H * W, n = N * C * S;
    _Float16 *a = reinterpret_cast<_Float16 *>(rq_split), *b = reinterpret_cast<_Float16 *>(rq2_split), *l = reinterpret_cast<_Float16 *>(left_split);
    _Float16 *a_lo = a + G * H * WU * 8, *b_lo = b + G * H * WU2 * 8, *l_lo = l + C * S;
    const int64_t gi_bs = 6 * G * H * pitch * 8;
    const snvc_il_out il_g{gi, gi_bs, pitch, lp, 0, 6, 0}, il_col{gi, gi_bs, pitch, lp, 3, 6, 0}, il_left{p_il, 3 * G * S * 8, W, 0, 0, 3, left_rows ? 2 : 1};
    X2QPoolArgs pa;
    int64_t jobs[3];
    rc = f16x3_conv2d_setup(who, who, a, a_lo, packed_g, nullptr, nullptr, g, N, C, Cout3, H, WU, 3, 7, out_mul_g, mul_right, 0, &il_g, pa.g, jobs[0]);
    if (rc) return rc;
    rc = f16x3_conv2d_setup(who, who, b, b_lo, packed_col, nullptr, nullptr, gcol, N, C, Cout3, H, WU2, 3, 7, out_mul_col, mul_right, 0, &il_col,
                            pa.gcol, jobs[1]);
    if (rc) return rc;
    rc = f16x3_conv2d_setup(who, who, l, l_lo, packed_left, nullptr, nullptr, planes, N, C, cout_left, H, W, 3, 3, out_mul_left, mul_left, 0, &il_left,
                            pa.left, jobs[2]);
    if (rc) return rc;
    if (jobs[0] != plan.c_jobs[0] || jobs[1] != plan.c_jobs[1] || jobs[2] != plan.c_jobs[2])
        return fail_as(SNVC_ERR_INVALID_ARGUMENT, who, "internal: the plan and the layers disagree on their jobs");
    hipStream_t st = as_stream(stream);
    unsigned *scratch = reinterpret_cast<unsigned *>(scratch16);
    if (pool & SNVC_PREP_POOL_AB) {
        split_scale_pair_kernel<<<(unsigned)(plan.a_blocks[0] + plan.a_blocks[1]), 256, 0, st>>>(right, n, mul_right, left, n, mul_left, scratch,
                                                                                                 (unsigned)plan.a_blocks[0]);
        rc = check_launch("snvc_prep_pooled_x3(scales)");
        if (rc) return rc;
        SplitProducersArgs sp{};
        sp.right = right; sp.left = left; sp.mul_right = mul_right; sp.mul_left = mul_left;
        sp.rq_hi = a; sp.rq_lo = a_lo; sp.rq2_hi = b; sp.rq2_lo = b_lo; sp.l_hi = l; sp.l_lo = l_lo;
        sp.C = (int)C; sp.H = (int)H; sp.W = (int)W; sp.q = q; sp.WU = (int)WU; sp.off = off; sp.WU2 = (int)WU2; sp.off2 = off2;
        sp.total = plan.b_items[0]; sp.total2 = plan.b_items[1]; sp.S = S;
        sp.end_rq = (int)plan.b_blocks[0]; sp.end_rq2 = (int)(plan.b_blocks[0] + plan.b_blocks[1]);
        sp.row_blocks = (int)plan.b_row_blocks; sp.groups = (int)G;
        split_producers_kernel<<<(unsigned)(plan.b_blocks[0] + plan.b_blocks[1] + plan.b_blocks[2]), 256, 0, st>>>(sp);
        rc = check_launch("snvc_prep_pooled_x3(split pairs)");
        if (rc) return rc;
    } else {
        rc = snvc_f16x3_split_scale(right, n, scratch, mul_right, stream);
        if (!rc) rc = snvc_f16x3_split_scale(left, n, scratch + 2, mul_left, stream);
        if (!rc) rc = snvc_sheared_upsample_split(right, a, a_lo, mul_right, N, C, H, W, q, WU, off, stream);
        if (!rc) rc = snvc_sheared_upsample_split(right, b, b_lo, mul_right, N, C, H, W, q, WU2, off2, stream);
        if (!rc) rc = snvc_f16x3_from_ncdhw(left, l, l_lo, N, C, S, 0, 0, 1.0f, mul_left, stream);
        if (rc) return rc;
    }
    using C7 = X2QCfg<3, 7>;
    using C3 = X2QCfg<3, 3>;
    if (pool & SNVC_PREP_POOL_C) {
        pa.end_g = (int)jobs[0]; pa.end_gcol = (int)(jobs[0] + jobs[1]);
        constexpr int lds_bytes = C7::LDS_BYTES > C3::LDS_BYTES ? C7::LDS_BYTES : C3::LDS_BYTES;
        launch_lds<conv2d_x3q_pool_kernel>(dim3((unsigned)(jobs[0] + jobs[1] + jobs[2]), 1, (unsigned)N), 256, lds_bytes, st, pa);
    } else {
        launch_lds<conv2d_x3q_kernel<C7, 1>>(dim3((unsigned)jobs[0], 1, (unsigned)N), 256, C7::LDS_BYTES, st, pa.g);
        launch_lds<conv2d_x3q_kernel<C7, 1>>(dim3((unsigned)jobs[1], 1, (unsigned)N), 256, C7::LDS_BYTES, st, pa.gcol);
        launch_lds<conv2d_x3q_kernel<C3, 1>>(dim3((unsigned)jobs[2], 1, (unsigned)N), 256, C3::LDS_BYTES, st, pa.left);
    }
    return check_launch("snvc_prep_pooled_x3(layers)");
}

// n_layers depth-1 split layers of ONE fp32 [N][C][H][W] input in one host call: its scale, its split pair (ws: N*2*C*H*W halves), then
// the layers (same kernel size, their own packed weights / output channels / results).  The left half's depth-class planes (one
// 3x3 layer) and the any-shift path's P / Q layers (two 3x3 layers of the right feature) go through here.
int snvc_f16x3_conv2d_from_f32(const float *x, int64_t N, int64_t C, int64_t H, int64_t W, int kh, int kw, int n_layers,
                               const void *const *packed, const int64_t *cout, const float *out_mul, float *const *y, void *ws_split,
                               void *scratch8, float *mul_dev, void *stream) {
    using namespace snvc;
    if (!x || !packed || !cout || !out_mul || !y || !ws_split || !scratch8 || !mul_dev || n_layers < 1 || n_layers > 8)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_conv2d_from_f32: null pointer or layer count outside 1..8");
    if (N <= 0 || C % 8) return fail(SNVC_ERR_UNSUPPORTED, "snvc_f16x3_conv2d_from_f32: C % 8 == 0");
    int rc = snvc_f16x3_split_scale(x, N * C * H * W, scratch8, mul_dev, stream);
    if (rc) return rc;
    _Float16 *a = reinterpret_cast<_Float16 *>(ws_split);
    rc = snvc_f16x3_from_ncdhw(x, a, a + C * H * W, N, C, H * W, 0, 0, 1.0f, mul_dev, stream);
    if (rc) return rc;
    for (int i = 0; i < n_layers; ++i) {
        rc = snvc_f16x3_conv2d_forward(a, a + C * H * W, packed[i], nullptr, nullptr, y[i], N, C, cout[i], H, W, kh, kw, out_mul[i], mul_dev, 0, stream);
        if (rc) return rc;
    }
    return SNVC_OK;
}

int64_t snvc_f16x3_tail_packed_weight_bytes(int cin) {
    return cin > 0 && cin % 32 == 0 ? (int64_t)(cin / 32) * 2 * 2 * 64 * 8 * 2 : -1;
}

int snvc_f16x3_tail_pack_weights(const float *weight, int cin, void *packed, float wmul, void *stream) {
    using namespace snvc;
    if (!weight || !packed || cin <= 0 || cin % 32 != 0)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_tail_pack_weights: weight [Cin][27] with Cin % 32 == 0");
    const int total = (cin / 32) * 2 * 2 * 64 * 8;
    pack_tail_weights_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, as_stream(stream)>>>(weight, reinterpret_cast<_Float16 *>(packed), cin, wmul, total);
    return check_launch("snvc_f16x3_tail_pack_weights");
}

int snvc_f16x3_deconv3d_tail_forward(const snvc_conv3d_desc *d, const void *x_hi, const void *x_lo, const void *packed_weight,
                                     const float *scale, const float *bias, const void *res_hi, const void *res_lo, float res_mul,
                                     const void *tail_packed, float *t_out, float tail_mul, int *overflow, void *stream) {
    using namespace snvc;
    if (!tail_packed || !t_out) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_f16x3_deconv3d_tail_forward: null pointer");
    F16x3Call c;
    c.x_hi = x_hi; c.x_lo = x_lo; c.packed_weight = packed_weight; c.scale = scale; c.bias = bias; c.res_hi = res_hi; c.res_lo = res_lo;
    c.head_mul = 1.0f; c.res_mul = res_mul; c.overflow = overflow; c.tail_w = tail_packed; c.t_out = t_out; c.tail_mul = tail_mul; c.stream = stream;
    return f16x3_forward(d, c);
}

static int tail_gather(const float *t, const float *bias, const float *residual, float *y, int64_t n, int64_t nd, int64_t nh, int64_t nw,
                       const snvc_wedge_desc *res_alias, void *stream) {
    using namespace snvc;
    if (res_alias && (!residual || res_alias->D != 4 * nd || res_alias->W != 4 * nw || (res_alias->q != 1 && res_alias->q != 2)))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_alias_deconv_tail_gather: res_alias describes the residual [4 nd][.][4 nw], q = 1 | 2");
    if (n < 0 || nd <= 0 || nh <= 0 || nw <= 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_deconv_tail_gather: sizes must be positive");
    if (n == 0) return SNVC_OK;
    if (!t || !y) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_deconv_tail_gather: null pointer");
    if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual)) & 15)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_deconv_tail_gather: y / residual must be 16-byte aligned");
    const int64_t threads = 16 * nd * nh * nw, out_vox = 64 * nd * nh * nw;
    if (threads >= ((int64_t)1 << 31) * 255 || n > 65535 || 27 * 8 * nd * nh * nw >= ((int64_t)1 << 40))
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_deconv_tail_gather: tensor too large");
    const dim3 grid((unsigned)ceil_div<int64_t>(threads, 256), (unsigned)n);
    if (res_alias)
        deconv_tail_gather_alias_kernel<<<grid, 256, 0, as_stream(stream)>>>(t, bias, residual, y, (int)nd, (int)nh, (int)nw,
                                                                             27 * 8 * nd * nh * nw, out_vox, out_vox, *res_alias);
    else
        deconv_tail_gather_kernel<<<grid, 256, 0, as_stream(stream)>>>(t, bias, residual, y, (int)nd, (int)nh, (int)nw, 27 * 8 * nd * nh * nw,
                                                                       out_vox, out_vox);
    return check_launch("snvc_deconv_tail_gather");
}

int snvc_deconv_tail_gather(const float *t, const float *bias, const float *residual, float *y, int64_t n, int64_t nd, int64_t nh,
                            int64_t nw, void *stream) {
    return tail_gather(t, bias, residual, y, n, nd, nh, nw, nullptr, stream);
}

int snvc_alias_deconv_tail_gather(const float *t, const float *bias, const float *residual, float *y, int64_t n, int64_t nd, int64_t nh,
                                  int64_t nw, const snvc_wedge_desc *res_alias, void *stream) {
    return tail_gather(t, bias, residual, y, n, nd, nh, nw, res_alias, stream);
}

}  // extern "C"
