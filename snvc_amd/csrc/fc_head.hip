// The fully-connected box head (include/snvc_fc.h; DESIGN.md "FC box head"): a residual MLP of Linear + BatchNorm1d +
// activation (+ dropout) layers that maps the coordinate head's [N, 18] output to a five-number BEV box.
//
// Every product is v_mfma_f32_16x16x4_f32: exact float32 products, float32 accumulation.  Lane l = 16 q + r of a wave holds
// A[row r][k q], B[k q][col r] and the four results D[row 4 q + i][col r], i = 0 .. 3.
//
// Four kernels:
//   eval_kernel          the whole network for one tile of 16 rows; activations live in two LDS buffers laid out k-major
//                        ([k][16 rows], so a wave's A operand of a k-step is 64 consecutive floats and its four results are one
//                        16-byte store); weights stream from the packed buffer, whose slabs are laid out the same way.  The four
//                        waves own the 16-neuron slabs s = wave, wave + 4, ...
//   train_fwd_kernel     one layer for one slab of 16 neurons and all N rows: the products, then the batch statistics, the
//                        normalisation, activation, dropout and residual in the owner.
//   bwd_params_kernel    the same ownership: dropout / activation / BatchNorm backward, then dW = dz^T x for the slab.
//   bwd_input_kernel     one tile of 16 rows: dx = dz W (+ skip).
// Sums over rows are taken by 16 threads per neuron over the rows g, g + 16, ... each, then over g = 0 .. 15 in that order.
#include <cmath>

#include "common.hpp"
#include "snvc_fc.h"

namespace snvc {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kThreads = 256, kWaves = kThreads / kWave, kTile = 16;
constexpr float kLeakySlope = 0.01f;      // nn.LeakyReLU's default

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ float act(float y, float slope) { return y > 0.0f ? y : slope * y; }

// ---------------------------------------------------------------------------------------------------- eval
// One slab's 16 x 16 result: src is a k-major LDS buffer of kp rows of 16, w the slab's [kp][16] weights.  k-step s reads
// element 64 s + lane of both.  Four accumulators keep four MFMAs in flight.
__device__ __forceinline__ f32x4 slab_product(const float *src, const float *__restrict__ w, int kp, int lane) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    const int steps = kp >> 2;
    int s = 0;
    for (; s + 4 <= steps; s += 4) {
        const int at = s * 64 + lane;
        const float w0 = w[at], w1 = w[at + 64], w2 = w[at + 128], w3 = w[at + 192];
        a0 = mfma(src[at], w0, a0);
        a1 = mfma(src[at + 64], w1, a1);
        a2 = mfma(src[at + 128], w2, a2);
        a3 = mfma(src[at + 192], w3, a3);
    }
    for (; s < steps; ++s) a0 = mfma(src[s * 64 + lane], w[s * 64 + lane], a0);
    return (a0 + a1) + (a2 + a3);
}

// One Linear + folded norm + activation from src to dst (both k-major LDS); add: dst += result (the residual, in place).
__device__ __forceinline__ void lds_layer(const float *src, float *dst, const float *__restrict__ w, const float *__restrict__ shift,
                                          int kp, int width, float slope, bool add) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    for (int s = wave; s < width / kTile; s += kWaves) {
        f32x4 v = slab_product(src, w + (size_t)s * kp * kTile, kp, lane);
        const int n = s * kTile + r;
        const float sh = shift[n];
        f32x4 *at = reinterpret_cast<f32x4 *>(dst + n * kTile + q * 4);
        for (int i = 0; i < 4; ++i) v[i] = act(v[i] + sh, slope);
        if (add) v += *at;
        *at = v;
    }
}

__global__ void __launch_bounds__(kThreads)
eval_kernel(const float *__restrict__ x, const float *__restrict__ packed, float *__restrict__ out, int64_t N, int in, int width,
            int blocks, int outs, float slope, int representation) {
    extern __shared__ float lds[];
    const int in_p = (in + 3) & ~3, out_p = (outs + 15) & ~15;
    float *X = lds, *Y = lds + kTile * width;         // Y holds max(width, in_p) rows of 16
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    for (int i = threadIdx.x; i < in_p * kTile; i += kThreads) {
        const int r = i & 15, k = i >> 4;
        Y[i] = (k < in && row0 + r < N) ? x[(row0 + r) * in + k] : 0.0f;      // rows past N and the K pad are zeros
    }
    __syncthreads();
    const float *w = packed;
    lds_layer(Y, X, w, w + (size_t)in_p * width, in_p, width, slope, false);
    w += (size_t)in_p * width + width;
    __syncthreads();
    for (int b = 0; b < blocks; ++b) {
        lds_layer(X, Y, w, w + (size_t)width * width, width, width, slope, false);
        w += (size_t)width * width + width;
        __syncthreads();
        lds_layer(Y, X, w, w + (size_t)width * width, width, width, slope, true);     // each wave adds into its own columns of X
        w += (size_t)width * width + width;
        __syncthreads();
    }
    if (representation) {
        for (int i = threadIdx.x; i < width * kTile; i += kThreads) {
            const int n = i % width, r = i / width;
            if (row0 + r < N) out[(row0 + r) * width + n] = X[n * kTile + r];
        }
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const float *shift = w + (size_t)width * out_p;
    for (int s = wave; s < out_p / kTile; s += kWaves) {
        const f32x4 v = slab_product(X, w + (size_t)s * width * kTile, width, lane);
        const int n = s * kTile + r;
        const float sh = shift[n];
        for (int i = 0; i < 4; ++i) {
            const int64_t row = row0 + q * 4 + i;
            if (row < N && n < outs) out[row * outs + n] = v[i] + sh;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- column sums
// The sum over g = 0 .. 15, in that order, of the 16 partial sums of the calling thread's neuron; every thread gets it.
__device__ __forceinline__ float column_sum(float partial, float (*red)[kTile]) {
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
    __syncthreads();                 // the previous use of red is over
    red[g][c] = partial;
    __syncthreads();
    float s = 0.0f;
    for (int k = 0; k < kTile; ++k) s += red[k][c];
    return s;
}

// ---------------------------------------------------------------------------------------------------- training forward
__global__ void __launch_bounds__(kThreads)
train_fwd_kernel(const float *__restrict__ x, const float *__restrict__ weight, const float *__restrict__ bias,
                 const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ running_mean,
                 float *__restrict__ running_var, int64_t *__restrict__ tracked, const uint8_t *__restrict__ mask,
                 const float *__restrict__ residual, float *xhat, float *__restrict__ mean_out, float *__restrict__ istd_out,
                 float *__restrict__ out, int64_t N, int K, int M, float eps, float momentum, float keep_scale, float slope) {
    __shared__ float red[kTile][kTile];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int n0 = blockIdx.x * kTile;
    float *z = gamma ? xhat : out;
    {
        const int n = n0 + r;
        const float b = n < M ? bias[n] : 0.0f;
        for (int64_t t = wave; t * kTile < N; t += kWaves) {
            const int64_t arow = t * kTile + r;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < K; k0 += 4) {
                const int k = k0 + q;
                const float a = (arow < N && k < K) ? x[arow * K + k] : 0.0f;
                const float w = (n < M && k < K) ? weight[(int64_t)n * K + k] : 0.0f;
                acc = mfma(a, w, acc);
            }
            for (int i = 0; i < 4; ++i) {
                const int64_t row = t * kTile + q * 4 + i;
                if (row < N && n < M) z[row * M + n] = acc[i] + b;
            }
        }
    }
    if (!gamma) return;
    __syncthreads();                 // the slab's z is complete (M is a multiple of 16 here)
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4, n = n0 + c;
    float s = 0.0f;
    for (int64_t row = g; row < N; row += kTile) s += z[row * M + n];
    const float mean = column_sum(s, red) / (float)N;
    s = 0.0f;
    for (int64_t row = g; row < N; row += kTile) {
        const float d = z[row * M + n] - mean;
        s += d * d;
    }
    const float sq = column_sum(s, red);
    const float var = sq / (float)N, istd = 1.0f / sqrtf(var + eps);
    if (g == 0) {
        mean_out[n] = mean;
        istd_out[n] = istd;
        running_mean[n] = (1.0f - momentum) * running_mean[n] + momentum * mean;
        running_var[n] = (1.0f - momentum) * running_var[n] + momentum * (sq / (float)(N - 1));
    }
    if (tracked && blockIdx.x == 0 && threadIdx.x == 0) *tracked += 1;
    const float ga = gamma[n], be = beta[n];
    for (int64_t row = g; row < N; row += kTile) {
        const int64_t at = row * M + n;
        const float xh = (z[at] - mean) * istd;
        xhat[at] = xh;
        float y = act(fmaf(ga, xh, be), slope);
        if (mask) y = mask[at] ? y * keep_scale : 0.0f;
        if (residual) y += residual[at];
        out[at] = y;
    }
}

// ---------------------------------------------------------------------------------------------------- training backward
// The gradient at the BatchNorm's output for one element: dropout, then the activation at y = gamma * xhat + beta (the same
// fmaf as the forward).
__device__ __forceinline__ float grad_at_norm(float dy, float xh, float ga, float be, const uint8_t *mask, int64_t at,
                                              float keep_scale, float slope) {
    float g = dy;
    if (mask) g = mask[at] ? g * keep_scale : 0.0f;
    return fmaf(ga, xh, be) > 0.0f ? g : slope * g;
}

__global__ void __launch_bounds__(kThreads)
bwd_params_kernel(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ xhat,
                  const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ istd,
                  const uint8_t *__restrict__ mask, float *dz, float *__restrict__ dgamma, float *__restrict__ dbeta,
                  float *__restrict__ dweight, float *__restrict__ dbias, int64_t N, int K, int M, float keep_scale, float slope) {
    __shared__ float red[kTile][kTile];
    const int n0 = blockIdx.x * kTile;
    const int c = threadIdx.x & 15, g = threadIdx.x >> 4, n = n0 + c;
    const float *d = dy;             // what dW contracts with
    if (gamma) {
        const float ga = gamma[n], be = beta[n], is = istd[n];
        float sb = 0.0f, sg = 0.0f;
        for (int64_t row = g; row < N; row += kTile) {
            const int64_t at = row * M + n;
            const float xh = xhat[at], gy = grad_at_norm(dy[at], xh, ga, be, mask, at, keep_scale, slope);
            sb += gy;
            sg += gy * xh;
        }
        const float db = column_sum(sb, red), dg = column_sum(sg, red);
        const float mb = db / (float)N, mg = dg / (float)N, scale = ga * is;
        float sz = 0.0f;
        for (int64_t row = g; row < N; row += kTile) {
            const int64_t at = row * M + n;
            const float xh = xhat[at], gy = grad_at_norm(dy[at], xh, ga, be, mask, at, keep_scale, slope);
            const float v = scale * ((gy - mb) - xh * mg);
            dz[at] = v;
            sz += v;
        }
        const float dbi = column_sum(sz, red);
        if (g == 0) {
            dgamma[n] = dg;
            dbeta[n] = db;
            dbias[n] = dbi;
        }
        d = dz;
    } else {
        float sz = 0.0f;
        if (n < M)
            for (int64_t row = g; row < N; row += kTile) sz += dy[row * M + n];
        const float dbi = column_sum(sz, red);
        if (g == 0 && n < M) dbias[n] = dbi;
    }
    __syncthreads();                 // the slab's dz is complete
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    for (int kt = wave; kt * kTile < K; kt += kWaves) {
        const int k = kt * kTile + r, nn = n0 + r;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int64_t r0 = 0; r0 < N; r0 += 4) {
            const int64_t row = r0 + q;
            const float a = (row < N && nn < M) ? d[row * M + nn] : 0.0f;
            const float b = (row < N && k < K) ? x[row * K + k] : 0.0f;
            acc = mfma(a, b, acc);
        }
        for (int i = 0; i < 4; ++i) {
            const int no = n0 + q * 4 + i;
            if (no < M && k < K) dweight[(int64_t)no * K + k] = acc[i];
        }
    }
}

__global__ void __launch_bounds__(kThreads)
bwd_input_kernel(const float *__restrict__ dz, const float *__restrict__ weight, const float *skip, float *dx, int64_t N, int K,
                 int M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * kTile, arow = row0 + r;
    for (int kt = wave; kt * kTile < K; kt += kWaves) {
        const int k = kt * kTile + r;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int nb = 0; nb < M; nb += 4) {
            const int n = nb + q;
            const float a = (arow < N && n < M) ? dz[arow * M + n] : 0.0f;
            const float b = (n < M && k < K) ? weight[(int64_t)n * K + k] : 0.0f;
            acc = mfma(a, b, acc);
        }
        for (int i = 0; i < 4; ++i) {
            const int64_t row = row0 + q * 4 + i;
            if (row < N && k < K) dx[row * K + k] = skip ? acc[i] + skip[row * K + k] : acc[i];
        }
    }
}

inline bool width_ok(int64_t v) { return v >= 1 && v <= SNVC_FC_MAX_WIDTH; }

// N rows of a layer [K] -> [M]: sizes the kernels index with int and launch grids hold
inline int layer_sizes_ok(const char *what, int64_t N, int64_t K, int64_t M) {
    if (N < 0 || !width_ok(K) || !width_ok(M)) return fail(SNVC_ERR_INVALID_ARGUMENT, what);
    if (N > INT32_MAX / 2) return fail(SNVC_ERR_UNSUPPORTED, what);
    return SNVC_OK;
}

}  // namespace
}  // namespace snvc

extern "C" {

int snvc_fc_abi_version(void) { return 1; }

int64_t snvc_fc_packed_floats(int64_t input_size, int64_t num_neurons, int64_t num_blocks, int64_t output_size) {
    using namespace snvc;
    if (!width_ok(input_size) || !width_ok(num_neurons) || !width_ok(output_size) || num_neurons % 16 != 0 || num_blocks < 0 ||
        num_blocks > 1024)
        return -1;
    const int64_t in_p = (input_size + 3) / 4 * 4, out_p = (output_size + 15) / 16 * 16, w = num_neurons;
    return in_p * w + w + 2 * num_blocks * (w * w + w) + w * out_p + out_p;
}

int snvc_fc_eval_forward(const float *x, const float *packed, float *out, int64_t N, int64_t input_size, int64_t num_neurons,
                         int64_t num_blocks, int64_t output_size, int leaky, int representation, void *stream) {
    using namespace snvc;
    if (snvc_fc_packed_floats(input_size, num_neurons, num_blocks, output_size) < 0)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_eval_forward: sizes must be 1 .. 1024, num_neurons a multiple of 16");
    if (N < 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_eval_forward: negative N");
    if (N > INT32_MAX / 2) return fail(SNVC_ERR_UNSUPPORTED, "snvc_fc_eval_forward: more than 2^30 rows in one call");
    if (N == 0) return SNVC_OK;
    if (!x || !packed || !out) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_eval_forward: null pointer");
    if (!aligned(16, packed) || !aligned(4, x, out))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_eval_forward: a pointer is not aligned");
    const int64_t in_p = (input_size + 3) / 4 * 4;
    const size_t bytes = sizeof(float) * kTile * (size_t)(num_neurons + (in_p > num_neurons ? in_p : num_neurons));
    launch_lds<eval_kernel>(dim3((unsigned)ceil_div<int64_t>(N, kTile)), dim3(kThreads), bytes, as_stream(stream), x, packed, out, N,
                            (int)input_size, (int)num_neurons, (int)num_blocks, (int)output_size, leaky ? kLeakySlope : 0.0f,
                            representation);
    return check_launch("snvc_fc_eval_forward");
}

int snvc_fc_train_layer_forward(const float *x, const float *weight, const float *bias, const float *gamma, const float *beta,
                                float *running_mean, float *running_var, int64_t *num_batches_tracked, const uint8_t *mask,
                                const float *residual, float *xhat, float *mean, float *istd, float *out, int64_t N, int64_t K,
                                int64_t M, float eps, float momentum, float keep_scale, int leaky, void *stream) {
    using namespace snvc;
    const int rc = layer_sizes_ok("snvc_fc_train_layer_forward: N >= 0 and K, M in 1 .. 1024, N below 2^30", N, K, M);
    if (rc != SNVC_OK) return rc;
    if (!x || !weight || !bias || !out) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_forward: null pointer");
    if (gamma) {
        if (M % 16 != 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_forward: a normalised layer's width must be a multiple of 16");
        if (N < 2) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_forward: batch statistics need more than one row");
        if (!beta || !running_mean || !running_var || !xhat || !mean || !istd)
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_forward: null pointer");
        if (!aligned(8, num_batches_tracked)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_forward: a pointer is not aligned");
    }
    if (!aligned(4, x, weight, bias, gamma, beta, running_mean, running_var, residual, xhat, mean, istd, out))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_forward: a pointer is not aligned");
    if (N == 0) return SNVC_OK;
    train_fwd_kernel<<<dim3((unsigned)ceil_div<int64_t>(M, kTile)), kThreads, 0, as_stream(stream)>>>(
        x, weight, bias, gamma, beta, running_mean, running_var, num_batches_tracked, mask, residual, xhat, mean, istd, out, N, (int)K,
        (int)M, eps, momentum, keep_scale, leaky ? kLeakySlope : 0.0f);
    return check_launch("snvc_fc_train_layer_forward");
}

int snvc_fc_train_layer_backward_params(const float *dy, const float *x, const float *xhat, const float *gamma, const float *beta,
                                        const float *istd, const uint8_t *mask, float *dz, float *dgamma, float *dbeta,
                                        float *dweight, float *dbias, int64_t N, int64_t K, int64_t M, float keep_scale, int leaky,
                                        void *stream) {
    using namespace snvc;
    const int rc = layer_sizes_ok("snvc_fc_train_layer_backward_params: N >= 0 and K, M in 1 .. 1024, N below 2^30", N, K, M);
    if (rc != SNVC_OK) return rc;
    if (N == 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_backward_params: no rows");
    if (!dy || !x || !dweight || !dbias) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_backward_params: null pointer");
    if (gamma) {
        if (M % 16 != 0)
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_backward_params: a normalised layer's width must be a multiple of 16");
        if (!xhat || !beta || !istd || !dz || !dgamma || !dbeta)
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_backward_params: null pointer");
    }
    if (!aligned(4, dy, x, xhat, gamma, beta, istd, dz, dgamma, dbeta, dweight, dbias))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_backward_params: a pointer is not aligned");
    bwd_params_kernel<<<dim3((unsigned)ceil_div<int64_t>(M, kTile)), kThreads, 0, as_stream(stream)>>>(
        dy, x, xhat, gamma, beta, istd, mask, dz, dgamma, dbeta, dweight, dbias, N, (int)K, (int)M, keep_scale, leaky ? kLeakySlope : 0.0f);
    return check_launch("snvc_fc_train_layer_backward_params");
}

int snvc_fc_train_layer_backward_input(const float *dz, const float *weight, const float *skip, float *dx, int64_t N, int64_t K,
                                       int64_t M, void *stream) {
    using namespace snvc;
    const int rc = layer_sizes_ok("snvc_fc_train_layer_backward_input: N >= 0 and K, M in 1 .. 1024, N below 2^30", N, K, M);
    if (rc != SNVC_OK) return rc;
    if (N == 0) return SNVC_OK;
    if (!dz || !weight || !dx) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_backward_input: null pointer");
    if (!aligned(4, dz, weight, skip, dx)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_fc_train_layer_backward_input: a pointer is not aligned");
    bwd_input_kernel<<<dim3((unsigned)ceil_div<int64_t>(N, kTile)), kThreads, 0, as_stream(stream)>>>(dz, weight, skip, dx, N, (int)K,
                                                                                                     (int)M);
    return check_launch("snvc_fc_train_layer_backward_input");
}

}  // extern "C"
