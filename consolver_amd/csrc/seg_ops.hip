// Kernels of the SegFormer segmentation reward (segformer.cpp; edit_ppo/reward_model.py:110-117, 425-481) that are not GEMM / attention / LayerNorm: the glue of
// transformers' SegformerForSemanticSegmentation (MiT encoder + all-MLP head) and the reward's tail.  All tensors are token-major NHWC fp16 unless noted; every
// kernel computes in fp32 and rounds once on the store.
//
//   * seg_dwconv_gelu_kernel: the Mix-FFN's depthwise 3x3 conv (pad 1) + bias + erf-GELU on [B][H][W][C].  The one kernel here that moves real traffic (stage 1 of
//     B4 at 512 x 512: 16384 x 256 halfs in and out per image and layer).  A lane owns 8 channels (16 bytes) of one output column and walks down a band of rows
//     with a 3 x 3 window of f16x8 vectors in registers: per output row it loads the three vectors of the row below and reuses the six above.  A workgroup is
//     32 columns x 8 channel vectors (64 channels), so the 64 lanes of a wave read 4 pixels x 128 contiguous bytes; the left / right neighbour loads are the
//     loads of the adjacent lanes and hit in the vector L1, so a row of the strip comes from HBM once per workgroup.  The nine weight vectors and the bias stay
//     in registers (f16x8, converted at use).  No LDS, no barrier: columns past W and rows past H are predicated, any H x W.
//   * seg_im2col_kernel: the rows of a k x k / stride / pad convolution over the first C channels of an NHWC image in F.unfold order (column c k k + ky k + kx),
//     zero padded to the GEMM's k step -- the 7x7 stride-4 pad-3 overlapped patch embedding of stage 1 over the front end's 8-channel normalised image;
//   * seg_patchify_kernel: the kernel = stride = sr gather of the sequence reduction (column (ky sr + kx) C + c: 16-byte copies);
//   * seg_bilinear_kernel: torch's bilinear resize, align_corners = False, written into a column slice of the head's concat buffer;
//   * seg_relu_kernel: the head's ReLU behind linear_fuse (the implicit GEMM has no activation epilogue), in place;
//   * seg_argmax_kernel (one wave per row, ties to the lowest class), seg_logits_kernel (fp16 [M][ld] -> fp32 [B][classes][HW]) and seg_agreement_kernel
//     (100 x mean(pred == target) per sample, the target shared by the batch when its stride is 0).
#include "ops.h"

namespace {

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

__device__ __forceinline__ f16x8 ld8(const f16* p) { return *reinterpret_cast<const f16x8*>(p); }

constexpr int DW_COLS = 32;          // output columns of a workgroup (x 8 channel vectors = 256 lanes)

__global__ __launch_bounds__(256) void seg_dwconv_gelu_kernel(const f16* __restrict__ x, const f16* __restrict__ w, const f16* __restrict__ bias, int H, int W, int C,
                                                              int band, int cgroups, f16* __restrict__ out) {
    const int cg = blockIdx.x % cgroups, strip = blockIdx.x / cgroups;
    const int px = strip * DW_COLS + (threadIdx.x >> 3);
    if (px >= W) return;                                            // (no barrier below)
    const int c = (cg * 8 + (threadIdx.x & 7)) * 8;
    const int y0 = blockIdx.y * band, y1 = min(y0 + band, H);
    const long img = (long)blockIdx.z * H * W;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    f16x8 wk[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wk[t] = ld8(w + (long)t * C + c);
    const f16x8 bv = bias ? ld8(bias + c) : zero;
    const bool left = px > 0, right = px + 1 < W;
    f16x8 top[3], mid[3], bot[3];
    auto load_row = [&](int y, f16x8* r) {
        if (y < 0 || y >= H) { r[0] = zero; r[1] = zero; r[2] = zero; return; }
        const f16* p = x + (img + (long)y * W + px) * C + c;
        r[0] = left ? ld8(p - C) : zero;
        r[1] = ld8(p);
        r[2] = right ? ld8(p + C) : zero;
    };
    load_row(y0 - 1, top);
    load_row(y0, mid);
    for (int y = y0; y < y1; ++y) {
        load_row(y + 1, bot);
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = (float)bv[e];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                a += (float)top[j][e] * (float)wk[j][e] + (float)mid[j][e] * (float)wk[3 + j][e] + (float)bot[j][e] * (float)wk[6 + j][e];
            o[e] = (f16)(0.5f * a * (1.0f + erff(a * 0.70710678118654752f)));
        }
        *reinterpret_cast<f16x8*>(out + (img + (long)y * W + px) * C + c) = o;
#pragma unroll
        for (int j = 0; j < 3; ++j) { top[j] = mid[j]; mid[j] = bot[j]; }
    }
}

__global__ __launch_bounds__(256) void seg_im2col_kernel(const f16* __restrict__ x, int H, int W, int Cs, int C, int k, int stride, int pad, int Ho, int Wo, int Kp,
                                                         long total, f16* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % Kp);
    long t = i / Kp;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    f16 v = (f16)0.0f;
    if (j < C * k * k) {
        const int c = j / (k * k), r = j - c * k * k, ky = r / k, kx = r - ky * k;
        const int y = oy * stride - pad + ky, xx = ox * stride - pad + kx;
        if (y >= 0 && y < H && xx >= 0 && xx < W) v = x[((b * H + y) * W + xx) * Cs + c];
    }
    out[i] = v;
}

__global__ __launch_bounds__(256) void seg_patchify_kernel(const f16* __restrict__ x, int H, int W, int C8, int sr, int Ho, int Wo, long total, f16* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    long t = i / C8;
    const int kx = (int)(t % sr); t /= sr;
    const int ky = (int)(t % sr); t /= sr;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    *reinterpret_cast<f16x8*>(out + i * 8) = ld8(x + (((b * H + oy * sr + ky) * W + ox * sr + kx) * C8 + c8) * 8);
}

// torch upsample_bilinear2d, align_corners = False: source = max(scale (dst + 0.5) - 0.5, 0), scale = in / out, the index arithmetic and the blend in fp32
__global__ __launch_bounds__(256) void seg_bilinear_kernel(const f16* __restrict__ x, int Hi, int Wi, int C8, int Ho, int Wo, float sy, float sx, long total,
                                                           f16* __restrict__ out, long ld, int col) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    const long row = i / C8;
    long t = row;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    const float fy = fmaxf(sy * ((float)oy + 0.5f) - 0.5f, 0.f), fx = fmaxf(sx * ((float)ox + 0.5f) - 0.5f, 0.f);
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < Hi - 1 ? y0 : Hi - 1; x0 = x0 < Wi - 1 ? x0 : Wi - 1;
    const int y1 = y0 + (y0 < Hi - 1 ? 1 : 0), x1 = x0 + (x0 < Wi - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.0f - ly, hx = 1.0f - lx;
    const f16* base = x + (b * Hi * Wi * C8 + c8) * 8;
    const f16x8 v00 = ld8(base + ((long)y0 * Wi + x0) * C8 * 8), v01 = ld8(base + ((long)y0 * Wi + x1) * C8 * 8);
    const f16x8 v10 = ld8(base + ((long)y1 * Wi + x0) * C8 * 8), v11 = ld8(base + ((long)y1 * Wi + x1) * C8 * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)(hy * (hx * (float)v00[e] + lx * (float)v01[e]) + ly * (hx * (float)v10[e] + lx * (float)v11[e]));
    *reinterpret_cast<f16x8*>(out + row * ld + col + c8 * 8) = o;
}

// one wave per row: lane l looks at classes l, l + 64, ... in increasing order (a later one wins only when strictly larger), then the (value, index) pairs are
// reduced with the smaller index winning a tie -- torch.argmax's answer
__global__ __launch_bounds__(256) void seg_argmax_kernel(const f16* __restrict__ x, long M, long ld, int n, int* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const f16* p = x + row * ld;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int c = lane; c < n; c += 64) {
        const float v = (float)p[c];
        if (v > best || idx == 0x7fffffff) { best = v; idx = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (oi != 0x7fffffff && (idx == 0x7fffffff || ov > best || (ov == best && oi < idx))) { best = ov; idx = oi; }
    }
    if (lane == 0) out[row] = idx;
}

__global__ __launch_bounds__(256) void seg_logits_kernel(const f16* __restrict__ x, long HW, long ld, int n, long total, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long p = i % HW, t = i / HW;
    const int c = (int)(t % n);
    const long b = t / n;
    out[i] = (float)x[(b * HW + p) * ld + c];
}

__global__ __launch_bounds__(256) void seg_relu_kernel(f16* __restrict__ x, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    f16x8 v = ld8(x + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] > (f16)0.0f ? v[e] : (f16)0.0f;
    *reinterpret_cast<f16x8*>(x + i * 8) = v;
}

__global__ __launch_bounds__(256) void seg_agreement_kernel(const int* __restrict__ pred, const int* __restrict__ tgt, long tgt_stride, long n, float* __restrict__ out) {
    __shared__ int part[4];
    const int* a = pred + (long)blockIdx.x * n;
    const int* t = tgt + (long)blockIdx.x * tgt_stride;
    int cnt = 0;
    for (long i = threadIdx.x; i < n; i += 256) cnt += a[i] == t[i] ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(part[0] + part[1] + part[2] + part[3]) / (float)n * 100.0f;
}

}  // namespace

int launch_seg_dwconv_gelu(const f16* x, int B, int H, int W, int C, const f16* w, const f16* bias, f16* out, hipStream_t s) {
    if (!x || !w || !out) CS_FAIL(CS_E_ARG, "seg dwconv: x, w, out required");
    if (out == x) CS_FAIL(CS_E_ARG, "seg dwconv: out must not alias x");
    if (C < 64 || C % 64 || C > 2048) CS_FAIL(CS_E_SHAPE, "seg dwconv: C = %d must be a multiple of 64 up to 2048", C);
    if (B < 0 || H < 0 || W < 0 || B > 65535) CS_FAIL(CS_E_SHAPE, "seg dwconv: bad size");
    if (B == 0 || H == 0 || W == 0) return CS_OK;
    const int cgroups = C / 64, strips = (W + DW_COLS - 1) / DW_COLS;
    // rows per workgroup: long bands amortise the two halo rows; short ones give the chip enough workgroups
    int band = 32;
    while (band > 4 && (long)B * cgroups * strips * ((H + band - 1) / band) < 2048) band >>= 1;
    const int bands = (H + band - 1) / band;
    if (bands > 65535 || (long)cgroups * strips > 0x7fffffffL) CS_FAIL(CS_E_SHAPE, "seg dwconv: image too large for one launch");
    hipLaunchKernelGGL(seg_dwconv_gelu_kernel, dim3((unsigned)(cgroups * strips), (unsigned)bands, (unsigned)B), dim3(256), 0, s, x, w, bias, H, W, C, band, cgroups, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_seg_im2col(const f16* x, int B, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, f16* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "seg im2col: null pointer");
    if (B < 0 || H < 1 || W < 1 || C < 1 || Cs < C || k < 1 || stride < 1 || pad < 0 || Kp < C * k * k || H + 2 * pad < k || W + 2 * pad < k)
        CS_FAIL(CS_E_SHAPE, "seg im2col: bad size");
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const long total = (long)B * Ho * Wo * Kp;
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "seg im2col: too large for one launch");
    hipLaunchKernelGGL(seg_im2col_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, H, W, Cs, C, k, stride, pad, Ho, Wo, Kp, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_seg_patchify(const f16* x, int B, int H, int W, int C, int sr, f16* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "seg patchify: null pointer");
    if (B < 0 || C < 8 || C % 8 || sr < 1 || H < sr || W < sr) CS_FAIL(CS_E_SHAPE, "seg patchify: C %% 8 == 0 and H, W >= sr required");
    const int Ho = H / sr, Wo = W / sr;
    const long total = (long)B * Ho * Wo * sr * sr * (C / 8);
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "seg patchify: too large for one launch");
    hipLaunchKernelGGL(seg_patchify_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, H, W, C / 8, sr, Ho, Wo, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_seg_bilinear(const f16* x, int B, int Hi, int Wi, int C, int Ho, int Wo, f16* out, long ld, int col, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "seg bilinear: null pointer");
    if (C < 8 || C % 8 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || B < 0) CS_FAIL(CS_E_SHAPE, "seg bilinear: C %% 8 == 0 and positive sizes required");
    if (col < 0 || col % 8 || ld % 8 || (long)col + C > ld) CS_FAIL(CS_E_SHAPE, "seg bilinear: the slice [%d, %d) does not fit a row of %ld (multiples of 8)", col, col + C, ld);
    const long total = (long)B * Ho * Wo * (C / 8);
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "seg bilinear: too large for one launch");
    hipLaunchKernelGGL(seg_bilinear_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, Hi, Wi, C / 8, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo, total, out, ld, col);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_seg_argmax(const f16* x, long M, long ld, int n, int* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "seg argmax: null pointer");
    if (M < 0 || n < 1 || ld < n) CS_FAIL(CS_E_SHAPE, "seg argmax: n = %d classes in rows of %ld", n, ld);
    if (M == 0) return CS_OK;
    if ((M + 3) / 4 > 0x7fffffffL) CS_FAIL(CS_E_SHAPE, "seg argmax: too many rows for one launch");
    hipLaunchKernelGGL(seg_argmax_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, M, ld, n, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_seg_logits(const f16* x, int B, long HW, long ld, int n, float* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "seg logits: null pointer");
    if (B < 0 || HW < 0 || n < 1 || ld < n) CS_FAIL(CS_E_SHAPE, "seg logits: bad size");
    const long total = (long)B * n * HW;
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "seg logits: too large for one launch");
    hipLaunchKernelGGL(seg_logits_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, HW, ld, n, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_seg_relu(f16* x, long n, hipStream_t s) {
    if (!x || n % 8) CS_FAIL(CS_E_ARG, "seg relu: x required, n %% 8 == 0");
    if (n <= 0) return CS_OK;
    if (n / 8 > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "seg relu: too large for one launch");
    hipLaunchKernelGGL(seg_relu_kernel, dim3(blocks_for(n / 8)), dim3(256), 0, s, x, n / 8);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_seg_agreement(const int* pred, const int* target, long target_stride, int B, long n, float* out, hipStream_t s) {
    if (!pred || !target || !out) CS_FAIL(CS_E_ARG, "seg agreement: null pointer");
    if (B < 0 || n < 1 || target_stride < 0) CS_FAIL(CS_E_SHAPE, "seg agreement: bad size");
    if (B == 0) return CS_OK;
    hipLaunchKernelGGL(seg_agreement_kernel, dim3(B), dim3(256), 0, s, pred, target, target_stride, n, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
