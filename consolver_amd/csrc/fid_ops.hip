// Kernels of FID (fid.cpp; the reference's fid_test.py: cleanfid.fid.compute_fid) that the logit-cosine reward does not have:
//
//   * the front end: clean-fid resizes every channel as a PIL mode-"F" image with BICUBIC straight to 299 x 299.  That is ImagingResample's 32-bit float
//     path: the horizontal pass first, its result stored as float32, then the vertical pass; the taps stay in double (image_front_end.h, pil_taps_f64) and
//     every output is `ss = 0.0; ss += pixel * k[x]` in double, ascending from xmin, rounded to float32 once.  The product and the sum are rounded
//     separately (__dmul_rn / __dadd_rn: no contraction into an FMA), as the host library's are.  The result is clipped to [0, 255], normalised and written
//     as the network's NHWC-8 fp16 rows; one thread per output pixel (plain kernels: 64 images of 512 x 512 are 0.1 GFLOP next to the network's 730);
//   * the two pools of the 2015 graph: 3x3 stride 1 pad 1 where the padding does not take part (the average divides by the taps inside the image);
//   * the statistics, all in fp64: sum[j] += sum_r f[r][j] and outer[i][j] += sum_r f[r][i] f[r][j] on v_mfma_f64_16x16x4_f64, and the finalize
//     mu = sum / N, sigma = (outer - N mu mu^T) / (N - 1).  Every output element is owned by one wave that walks the rows in order: no atomics, a call
//     is bitwise reproducible, and since the accumulator starts from the value already in `outer` a second call continues the first call's chain.
#include "ops.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

// ---- front end ----------------------------------------------------------------------------------------------------------------------------------------------
// the value PIL sees: a uint8 pixel as it is; a float one as evaluation.tensor_to_uint8_hwc writes it to the PNG: round(clamp(x, 0, 1) * 255), fp32, half to even
__device__ __forceinline__ float pixel255(unsigned char v) { return (float)v; }
__device__ __forceinline__ float pixel255(float v) {
    float x = v > 0.0f ? v : 0.0f;                // (NaN -> 0)
    x = x < 1.0f ? x : 1.0f;
    return rintf(x * 255.0f);
}
__device__ __forceinline__ float pixel255(f16 v) { return pixel255((float)v); }

struct FloatTab { const int* lo; const int* cnt; const double* kk; int ksize; };

// horizontal pass: tmp[bc][y][x] (x < out) from src[bc][y][W]
template <typename T>
__global__ __launch_bounds__(256) void fid_hresize_kernel(const T* __restrict__ src, long total, int W, int out, FloatTab th, float* __restrict__ tmp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % out);
    const long row = i / out;                                       // bc * H + y
    const T* p = src + row * W + th.lo[x];
    const double* kk = th.kk + (long)x * th.ksize;
    const int n = th.cnt[x];
    double ss = 0.0;
    for (int j = 0; j < n; ++j) ss = __dadd_rn(ss, __dmul_rn((double)pixel255(p[j]), kk[j]));
    tmp[i] = (float)ss;
}

// vertical pass + clip + normalise: one thread per output pixel, its three channels -> one 16-byte row of the network's input
__global__ __launch_bounds__(256) void fid_vresize_kernel(const float* __restrict__ tmp, long total, int H, int out, FloatTab tv, float m0, float m1, float m2,
                                                          float s0, float s1, float s2, f16* __restrict__ patches, float* __restrict__ resized) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % out);
    const long t = i / out;
    const int y = (int)(t % out);
    const long b = t / out;
    const double* kk = tv.kk + (long)y * tv.ksize;
    const int n = tv.cnt[y], lo = tv.lo[y];
    const float mean[3] = {m0, m1, m2}, sd[3] = {s0, s1, s2};
    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* col = tmp + ((b * 3 + c) * H + lo) * out + x;
        double ss = 0.0;
        for (int j = 0; j < n; ++j) ss = __dadd_rn(ss, __dmul_rn((double)col[(long)j * out], kk[j]));
        float v = (float)ss;
        v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        if (resized) resized[((b * 3 + c) * out + y) * out + x] = v;
        o[c] = (f16)((v - mean[c]) / sd[c]);
    }
    *reinterpret_cast<f16x8*>(patches + i * 8) = o;
}

// ---- pools ----------------------------------------------------------------------------------------------------------------------------------------------------
template <bool MAX>
__global__ __launch_bounds__(256) void fid_pool_kernel(const f16* __restrict__ x, int H, int W, int C8, long total, f16* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    long t = i / C8;
    const int px = (int)(t % W); t /= W;
    const int py = (int)(t % H);
    const long b = t / H;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    f16x8 m = *reinterpret_cast<const f16x8*>(x + i * 8);          // the centre tap is always inside
    int taps = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = py + k / 3 - 1, xx = px + k % 3 - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const f16x8 v = *reinterpret_cast<const f16x8*>(x + (((b * H + yy) * W + xx) * C8 + c8) * 8);
        ++taps;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (MAX) m[e] = v[e] > m[e] ? v[e] : m[e];
            else s[e] += (float)v[e];
        }
    }
    if (!MAX) {
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = (f16)(s[e] / (float)taps);
    }
    *reinterpret_cast<f16x8*>(out + i * 8) = m;
}

// ---- statistics ----------------------------------------------------------------------------------------------------------------------------------------------
// sum: a workgroup owns 64 columns; thread (phase p = tid >> 6, column tid & 63) adds the rows r = p (mod 4) in ascending order, the four partial sums are
// added in the fixed order ((p0 + p1) + p2) + p3 and then to sum[j]
__global__ __launch_bounds__(256) void fid_sum_kernel(const float* __restrict__ f, long n, int d, double* __restrict__ sum) {
    __shared__ double part[4][64];
    const int cl = threadIdx.x & 63, p = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + cl;
    double s = 0.0;
    if (j < d)
        for (long r = p; r < n; r += 4) s += (double)f[r * d + j];
    part[p][cl] = s;
    __syncthreads();
    if (p == 0 && j < d) sum[j] += ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
}

// outer: D = A B + C on v_mfma_f64_16x16x4_f64 with A[i][k] = f[r0 + k][i0 + i], B[k][j] = f[r0 + k][j0 + j] (k: 4 rows of f per instruction).  Operands as
// the f32 16x16x4 form, one f64 per lane: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; C / D: 4 f64 per lane, col = l & 15,
// row = (l >> 4) + 4 reg (NOT the f32 row formula).  A wave owns a 32 x 32 tile of `outer` (2 x 2 instruction tiles), a workgroup of four waves 64 x 64;
// d % 16 == 0, so a 16-wide tile is inside the matrix or outside it as a whole: outside, it loads nothing and stores nothing.  The operands come straight
// from global memory (16 consecutive floats of one row per 16 lanes); rows past n contribute zeros.
constexpr int ST = 2;
__global__ __launch_bounds__(256) void fid_outer_kernel(const float* __restrict__ f, long n, int d, double* __restrict__ outer) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 64 + (wave >> 1) * 32, j0 = blockIdx.x * 64 + (wave & 1) * 32;
    if (i0 >= d || j0 >= d) return;                                  // whole waves leave; there is no barrier below
    const int c = lane & 15, k = lane >> 4;
    bool iv[ST], jv[ST];
#pragma unroll
    for (int t = 0; t < ST; ++t) { iv[t] = i0 + t * 16 < d; jv[t] = j0 + t * 16 < d; }
    f64x4 acc[ST][ST];
#pragma unroll
    for (int a = 0; a < ST; ++a)
#pragma unroll
        for (int b = 0; b < ST; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[a][b][r] = (iv[a] && jv[b]) ? outer[(long)(i0 + a * 16 + k + 4 * r) * d + j0 + b * 16 + c] : 0.0;
#pragma unroll 4
    for (long r0 = 0; r0 < n; r0 += 4) {
        const long r = r0 + k;
        const bool rv = r < n;
        const float* row = f + (rv ? r : 0) * d;
        double av[ST], bv[ST];
#pragma unroll
        for (int t = 0; t < ST; ++t) {
            av[t] = (rv && iv[t]) ? (double)row[i0 + t * 16 + c] : 0.0;
            bv[t] = (rv && jv[t]) ? (double)row[j0 + t * 16 + c] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < ST; ++a)
#pragma unroll
            for (int b = 0; b < ST; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < ST; ++a)
#pragma unroll
        for (int b = 0; b < ST; ++b) {
            if (!(iv[a] && jv[b])) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) outer[(long)(i0 + a * 16 + k + 4 * r) * d + j0 + b * 16 + c] = acc[a][b][r];
        }
}

__global__ __launch_bounds__(256) void fid_finalize_kernel(const double* __restrict__ sum, const double* __restrict__ outer, double N, int d,
                                                           double* __restrict__ mu, double* __restrict__ sigma) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)d * d) return;
    const int col = (int)(i % d), row = (int)(i / d);
    const double mi = sum[row] / N, mj = sum[col] / N;
    if (row == 0) mu[col] = mj;
    sigma[i] = (outer[i] - N * mi * mj) / (N - 1.0);
}

}  // namespace

int launch_fid_front_end(const void* images, int dtype, int B, int H, int W, const FidResizePlan& pl, const float* mean, const float* stdv, float* tmp,
                         f16* patches, float* resized, hipStream_t s) {
    if (!images || !tmp || !patches || !mean || !stdv) CS_FAIL(CS_E_ARG, "fid front end: null pointer");
    if (dtype != CS_F16 && dtype != CS_F32 && dtype != CS_U8) CS_FAIL(CS_E_UNSUPPORTED, "fid front end: images must be uint8, fp16 or fp32");
    if (B <= 0) return B < 0 ? CS_E_SHAPE : CS_OK;
    if (H < 1 || W < 1 || pl.out < 1 || pl.h_ksize < 1 || pl.v_ksize < 1 || !pl.h_lo || !pl.v_lo) CS_FAIL(CS_E_SHAPE, "fid front end: bad plan for a %d x %d image", H, W);
    const FloatTab th{pl.h_lo, pl.h_cnt, pl.h_kk, pl.h_ksize}, tv{pl.v_lo, pl.v_cnt, pl.v_kk, pl.v_ksize};
    const long n1 = (long)B * 3 * H * pl.out, n2 = (long)B * pl.out * pl.out;
    if (n1 > 0x7fffffffL * 256 || n2 > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "fid front end: batch too large");
    if (dtype == CS_U8) hipLaunchKernelGGL(fid_hresize_kernel<unsigned char>, dim3(blocks_for(n1)), dim3(256), 0, s, (const unsigned char*)images, n1, W, pl.out, th, tmp);
    else if (dtype == CS_F16) hipLaunchKernelGGL(fid_hresize_kernel<f16>, dim3(blocks_for(n1)), dim3(256), 0, s, (const f16*)images, n1, W, pl.out, th, tmp);
    else hipLaunchKernelGGL(fid_hresize_kernel<float>, dim3(blocks_for(n1)), dim3(256), 0, s, (const float*)images, n1, W, pl.out, th, tmp);
    CS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fid_vresize_kernel, dim3(blocks_for(n2)), dim3(256), 0, s, tmp, n2, H, pl.out, tv, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2],
                       patches, resized);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

static int launch_fid_pool(bool max, const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "fid pool: null pointer");
    if (out == x) CS_FAIL(CS_E_ARG, "fid pool: out must not alias x");
    if (B < 0 || H < 1 || W < 1 || C < 8 || C % 8) CS_FAIL(CS_E_SHAPE, "fid pool: C %% 8 == 0 and positive sizes required");
    const long total = (long)B * H * W * (C / 8);
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "fid pool: too large for one launch");
    if (max) hipLaunchKernelGGL(fid_pool_kernel<true>, dim3(blocks_for(total)), dim3(256), 0, s, x, H, W, C / 8, total, out);
    else hipLaunchKernelGGL(fid_pool_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, s, x, H, W, C / 8, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
int launch_fid_avgpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) { return launch_fid_pool(false, x, B, H, W, C, out, s); }
int launch_fid_maxpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) { return launch_fid_pool(true, x, B, H, W, C, out, s); }

int launch_fid_stats_accumulate(const float* f, long n, int d, double* sum, double* outer, hipStream_t s) {
    if (!f || !sum || !outer) CS_FAIL(CS_E_ARG, "fid stats: null pointer");
    if (d < 16 || d > 4096 || d % 16 || n < 1) CS_FAIL(CS_E_SHAPE, "fid stats: d = %d must be a multiple of 16 in 16 .. 4096 and n = %ld >= 1", d, n);
    const unsigned g = (unsigned)((d + 63) / 64);
    hipLaunchKernelGGL(fid_sum_kernel, dim3(g), dim3(256), 0, s, f, n, d, sum);
    CS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fid_outer_kernel, dim3(g, g), dim3(256), 0, s, f, n, d, outer);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_fid_stats_finalize(const double* sum, const double* outer, long N, int d, double* mu, double* sigma, hipStream_t s) {
    if (!sum || !outer || !mu || !sigma) CS_FAIL(CS_E_ARG, "fid stats: null pointer");
    if (d < 1 || N < 2) CS_FAIL(CS_E_SHAPE, "fid stats: the covariance needs N >= 2 (N = %ld)", N);
    hipLaunchKernelGGL(fid_finalize_kernel, dim3(blocks_for((long)d * d)), dim3(256), 0, s, sum, outer, (double)N, d, mu, sigma);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
