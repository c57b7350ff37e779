// Kernels of the Depth Anything depth-map reward (depth.cpp; edit_ppo/reward_model.py:359-422) behind the shared ViT encoder: the DPT neck and head of
// transformers' DepthAnythingForDepthEstimation and the reward's post-processing.
//
//   * dpt_conv_kernel: 3x3 (pad 1) / 1x1 convolution to a NARROW output (32 or 64 channels) on v_mfma_f32_16x16x32_f16.  The implicit-GEMM kernels of igemm.hip
//     need N % 128 == 0 or N % 160 == 0 and Cin % 64 == 0; the neck's layers have N = 64 or 32 and Cin = 32 .. 384.  Here the output pixels are the MFMA's N
//     dimension and the filters its M dimension (D^T = W X^T), so that a lane ends up with 4 consecutive channels of ONE pixel: 8-byte NHWC stores, 8-byte
//     residual loads.  Both operands are read straight from global memory in the fragment layout (lane = (row | column) & 15, k slice lane >> 4: 16 contiguous
//     bytes of one pixel's / one filter tap's channels), zero for the padding ring and the rows past the end; a wave multiplies two 16-pixel tiles against every
//     filter fragment it loads.  The filters of a layer are 18 .. 442 KB and stay in L2; no LDS, no barrier, any H x W.  The neck is a quarter of the backbone's
//     work, so this kernel is written for every shape first.
//   * the align_corners = True bilinear resize (NHWC), the pixel-shuffle store of the reassemble stage's transposed convs (kernel = stride: one GEMM, then this
//     permutation), the head's 1x1 conv to one channel + ReLU in fp32, torch's bicubic resize of the fp32 depth map and the per-map min / max normalisation.
#include "ops.h"

namespace {

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

template <int COUT>
__global__ __launch_bounds__(256) void dpt_conv_kernel(const f16* __restrict__ x, int H, int W, int Cin, long M, const f16* __restrict__ w, int taps,
                                                       const f16* __restrict__ bias, const f16* __restrict__ res, const f16* __restrict__ res2, int relu_in,
                                                       int relu_out, f16* __restrict__ out) {
    constexpr int NT = COUT / 16, MT = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const long m_base = ((long)blockIdx.x * 4 + wave) * (16 * MT);
    if (m_base >= M) return;                                    // whole waves leave; there is no barrier below
    int py[MT], px[MT];
    long pb[MT];                                                // first pixel of the sample
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const long m = m_base + mt * 16 + col;
        pv[mt] = m < M;
        const long mm = pv[mt] ? m : 0;
        px[mt] = (int)(mm % W);
        const long t = mm / W;
        py[mt] = (int)(t % H);
        pb[mt] = (t / H) * (long)H * W;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const long K = (long)taps * Cin;                            // row length of w
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int tap = 0; tap < taps; ++tap) {
        const int dy = taps == 9 ? tap / 3 - 1 : 0, dx = taps == 9 ? tap % 3 - 1 : 0;
        const f16* xp[MT];
        bool ok[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int yy = py[mt] + dy, xx = px[mt] + dx;
            ok[mt] = pv[mt] && yy >= 0 && yy < H && xx >= 0 && xx < W;
            xp[mt] = x + (ok[mt] ? (pb[mt] + (long)yy * W + xx) * Cin : 0) + kq * 8;
        }
        const f16* wp = w + (long)col * K + (long)tap * Cin + kq * 8;
        for (int c0 = 0; c0 < Cin; c0 += 32) {
            f16x8 a[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                a[mt] = ok[mt] ? *reinterpret_cast<const f16x8*>(xp[mt] + c0) : zero;
                if (relu_in) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) a[mt][e] = a[mt][e] > (f16)0.0f ? a[mt][e] : (f16)0.0f;
                }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const f16x8 wf = *reinterpret_cast<const f16x8*>(wp + (long)nt * 16 * K + c0);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, a[mt], acc[mt][nt], 0, 0, 0);
            }
        }
    }
    // D: column = pixel (lane & 15), rows = filters 4 (lane >> 4) + r of the 16-filter tile
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (!pv[mt]) continue;
        const long m = m_base + mt * 16 + col;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int ch = nt * 16 + kq * 4;
            f32x4 v = acc[mt][nt];
            if (bias) {
                const f16x4 bv = *reinterpret_cast<const f16x4*>(bias + ch);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)bv[r];
            }
            if (res) {
                const f16x4 rv = *reinterpret_cast<const f16x4*>(res + m * COUT + ch);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
            }
            if (res2) {
                const f16x4 rv = *reinterpret_cast<const f16x4*>(res2 + m * COUT + ch);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)rv[r];
            }
            f16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (f16)((relu_out && !(v[r] > 0.f)) ? 0.f : v[r]);
            *reinterpret_cast<f16x4*>(out + m * COUT + ch) = o;
        }
    }
}

// torch upsample_bilinear2d, align_corners = True: source = dst * (in - 1) / (out - 1) (0 when out == 1), the scale and the blend in fp32
__global__ __launch_bounds__(256) void dpt_bilinear_kernel(const f16* __restrict__ x, int Hi, int Wi, int C8, int Ho, int Wo, float sy, float sx, long total,
                                                           f16* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    long t = i / C8;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    const float fy = sy * (float)oy, fx = sx * (float)ox;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 < Hi - 1 ? y0 : Hi - 1; x0 = x0 < Wi - 1 ? x0 : Wi - 1;
    const int y1 = y0 + (y0 < Hi - 1 ? 1 : 0), x1 = x0 + (x0 < Wi - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0, hy = 1.0f - ly, hx = 1.0f - lx;
    const f16* base = x + b * (long)Hi * Wi * C8 * 8 + c8 * 8;
    const f16x8 v00 = *reinterpret_cast<const f16x8*>(base + ((long)y0 * Wi + x0) * C8 * 8), v01 = *reinterpret_cast<const f16x8*>(base + ((long)y0 * Wi + x1) * C8 * 8);
    const f16x8 v10 = *reinterpret_cast<const f16x8*>(base + ((long)y1 * Wi + x0) * C8 * 8), v11 = *reinterpret_cast<const f16x8*>(base + ((long)y1 * Wi + x1) * C8 * 8);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)(hy * (hx * (float)v00[e] + lx * (float)v01[e]) + ly * (hx * (float)v10[e] + lx * (float)v11[e]));
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
}

__global__ __launch_bounds__(256) void dpt_pixel_shuffle_kernel(const f16* __restrict__ y, int Gh, int Gw, int k, int C8, int skip, long total, f16* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    long t = i / C8;
    const int Sh = Gh * k, Sw = Gw * k;
    const int ox = (int)(t % Sw); t /= Sw;
    const int oy = (int)(t % Sh);
    const long b = t / Sh;
    const int gy = oy / k, ky = oy - gy * k, gx = ox / k, kx = ox - gx * k;
    const long row = b * ((long)skip + (long)Gh * Gw) + skip + (long)gy * Gw + gx;
    *reinterpret_cast<f16x8*>(out + i * 8) = *reinterpret_cast<const f16x8*>(y + (row * k * k + ky * k + kx) * C8 * 8 + c8 * 8);
}

__global__ __launch_bounds__(256) void dpt_head_kernel(const f16* __restrict__ x, long M, int C8, const f16* __restrict__ w, const f16* __restrict__ bias, float scale,
                                                       float* __restrict__ out) {
    const long m = (long)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float acc = bias ? (float)bias[0] : 0.f;
    for (int c = 0; c < C8; ++c) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(x + (m * C8 + c) * 8), ww = *reinterpret_cast<const f16x8*>(w + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (float)v[e] * (float)ww[e];
    }
    out[m] = (acc > 0.f ? acc : 0.f) * scale;
}

// torch upsample_bicubic2d, align_corners = False: source = (dst + 0.5) * in / out - 0.5, cubic convolution with A = -0.75 on the four clamped neighbours
__device__ __forceinline__ void cubic_coeffs(float t, float* k) {
    const float A = -0.75f;
    const float a = t + 1.0f, b = 1.0f - t, c = 2.0f - t;
    k[0] = ((A * a - 5.0f * A) * a + 8.0f * A) * a - 4.0f * A;
    k[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    k[2] = ((A + 2.0f) * b - (A + 3.0f)) * b * b + 1.0f;
    k[3] = ((A * c - 5.0f * A) * c + 8.0f * A) * c - 4.0f * A;
}
__global__ __launch_bounds__(256) void dpt_bicubic_kernel(const float* __restrict__ x, int Hi, int Wi, int Ho, int Wo, float sy, float sx, long total,
                                                          float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % Wo);
    const long t = i / Wo;
    const int oy = (int)(t % Ho);
    const float* src = x + (t / Ho) * (long)Hi * Wi;
    const float ry = sy * ((float)oy + 0.5f) - 0.5f, rx = sx * ((float)ox + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    const int iy = (int)fy, ix = (int)fx;
    float ky[4], kx[4];
    cubic_coeffs(ry - fy, ky);
    cubic_coeffs(rx - fx, kx);
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int yy = min(max(iy - 1 + a, 0), Hi - 1);
        float r = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) r += kx[b] * src[(long)yy * Wi + min(max(ix - 1 + b, 0), Wi - 1)];
        acc += ky[a] * r;
    }
    out[i] = acc;
}

// one workgroup of 1024 threads per map: min / max, then (x - min) / (max - min + 1e-8) in place
__global__ __launch_bounds__(1024) void dpt_minmax_normalize_kernel(float* __restrict__ x, long n) {
    __shared__ float smin[16], smax[16];
    float* p = x + (long)blockIdx.x * n;
    float lo = INFINITY, hi = -INFINITY;
    for (long i = threadIdx.x; i < n; i += 1024) { const float v = p[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    hi = wave_max(hi);
    lo = -wave_max(-lo);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { smin[wave] = lo; smax[wave] = hi; }
    __syncthreads();
    lo = smin[0]; hi = smax[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) { lo = fminf(lo, smin[k]); hi = fmaxf(hi, smax[k]); }
    const float d = hi - lo + 1e-8f;
    for (long i = threadIdx.x; i < n; i += 1024) p[i] = (p[i] - lo) / d;
}

}  // namespace

int launch_dpt_conv(const DptConvArgs& a, hipStream_t s) {
    if (!a.x || !a.w || !a.out) CS_FAIL(CS_E_ARG, "dpt conv: x, w, out required");
    if (a.taps != 1 && a.taps != 9) CS_FAIL(CS_E_ARG, "dpt conv: taps must be 1 or 9");
    if (a.Cout != 32 && a.Cout != 64) CS_FAIL(CS_E_SHAPE, "dpt conv: Cout = %d must be 32 or 64", a.Cout);
    if (a.Cin < 32 || a.Cin % 32) CS_FAIL(CS_E_SHAPE, "dpt conv: Cin = %d must be a multiple of 32", a.Cin);
    if (a.out == a.x) CS_FAIL(CS_E_ARG, "dpt conv: out must not alias x");
    if (a.B < 0 || a.H < 0 || a.W < 0) CS_FAIL(CS_E_SHAPE, "dpt conv: negative size");
    const long M = (long)a.B * a.H * a.W;
    if (M == 0) return CS_OK;
    const long blocks = (M + 127) / 128;
    if (blocks > 0x7fffffffL) CS_FAIL(CS_E_SHAPE, "dpt conv: too many pixels for one launch");
    if (a.Cout == 32)
        hipLaunchKernelGGL(dpt_conv_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, s, a.x, a.H, a.W, a.Cin, M, a.w, a.taps, a.bias, a.res, a.res2, a.relu_in, a.relu_out, a.out);
    else
        hipLaunchKernelGGL(dpt_conv_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, s, a.x, a.H, a.W, a.Cin, M, a.w, a.taps, a.bias, a.res, a.res2, a.relu_in, a.relu_out, a.out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_dpt_bilinear(const f16* x, int B, int Hi, int Wi, int C, int Ho, int Wo, f16* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "dpt bilinear: null pointer");
    if (C < 8 || C % 8 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || B < 0) CS_FAIL(CS_E_SHAPE, "dpt bilinear: C %% 8 == 0 and positive sizes required");
    const long total = (long)B * Ho * Wo * (C / 8);
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "dpt bilinear: too large for one launch");
    const float sy = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f, sx = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
    hipLaunchKernelGGL(dpt_bilinear_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, Hi, Wi, C / 8, Ho, Wo, sy, sx, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_dpt_pixel_shuffle(const f16* y, int B, int G, int k, int C, int skip, f16* out, hipStream_t s) {
    return launch_dpt_pixel_shuffle_hw(y, B, G, G, k, C, skip, out, s);
}

int launch_dpt_pixel_shuffle_hw(const f16* y, int B, int Gh, int Gw, int k, int C, int skip, f16* out, hipStream_t s) {
    if (!y || !out) CS_FAIL(CS_E_ARG, "dpt pixel shuffle: null pointer");
    if (C < 8 || C % 8 || Gh < 1 || Gw < 1 || k < 1 || skip < 0 || B < 0) CS_FAIL(CS_E_SHAPE, "dpt pixel shuffle: C %% 8 == 0 and positive sizes required");
    const long total = (long)B * Gh * k * Gw * k * (C / 8);
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "dpt pixel shuffle: too large for one launch");
    hipLaunchKernelGGL(dpt_pixel_shuffle_kernel, dim3(blocks_for(total)), dim3(256), 0, s, y, Gh, Gw, k, C / 8, skip, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_dpt_head(const f16* x, long M, int C, const f16* w, const f16* bias, float scale, float* out, hipStream_t s) {
    if (!x || !w || !out) CS_FAIL(CS_E_ARG, "dpt head: null pointer");
    if (C < 8 || C % 8 || C > 64 || M < 0) CS_FAIL(CS_E_SHAPE, "dpt head: C = %d must be a multiple of 8 up to 64", C);
    if (M == 0) return CS_OK;
    if (M > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "dpt head: too large for one launch");
    hipLaunchKernelGGL(dpt_head_kernel, dim3(blocks_for(M)), dim3(256), 0, s, x, M, C / 8, w, bias, scale, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_dpt_bicubic(const float* x, int B, int Hi, int Wi, int Ho, int Wo, float* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "dpt bicubic: null pointer");
    if (Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || B < 0) CS_FAIL(CS_E_SHAPE, "dpt bicubic: positive sizes required");
    const long total = (long)B * Ho * Wo;
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "dpt bicubic: too large for one launch");
    hipLaunchKernelGGL(dpt_bicubic_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, Hi, Wi, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_dpt_minmax_normalize(float* x, int B, long n, hipStream_t s) {
    if (!x) CS_FAIL(CS_E_ARG, "dpt normalize: null pointer");
    if (B < 0 || n < 1) CS_FAIL(CS_E_SHAPE, "dpt normalize: bad size");
    if (B == 0) return CS_OK;
    hipLaunchKernelGGL(dpt_minmax_normalize_kernel, dim3(B), dim3(1024), 0, s, x, n);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
