// Kernels of the Inception-v3 logit-cosine reward (inception.cpp; edit_ppo/reward_model.py:98-108, 319-356): torchvision's Inception3 is 94 convolutions
// (each followed by BatchNorm and ReLU), three max pools, nine average pools and one linear layer.  All tensors are NHWC fp16 unless noted; every kernel
// computes in fp32 and rounds once on the store.
//
//   * incep_conv_kernel: ONE implicit-GEMM convolution for all ten filter forms of the network (1x1, 3x3 at stride 1 | 2 with or without padding, 5x5, 1x7, 7x1,
//     1x3, 3x1) on v_mfma_f32_16x16x32_f16.  The implicit-GEMM kernels of igemm.hip take 1x1 and 3x3 pad 1 with channel counts in 64s, even grids and a dense
//     [M][N] output; this network has grids of 149 .. 8 (and 1 x 1 at the smallest image), channel counts such as 48, 80 and 448, and every branch of a block
//     writes a column slice of the block's concatenated output.  The arrangement is dpt_conv_kernel's (dpt_ops.hip), generalised: output pixels are the MFMA's
//     N dimension and filters its M dimension (D^T = W X^T), so a lane ends with 4 consecutive channels of ONE pixel and stores 8 bytes into the slice
//     out[m][col + n]; both operands come straight from global memory in the fragment layout (lane = (pixel | filter) & 15, k slice lane >> 4: 16 contiguous
//     bytes of one pixel's / one tap's channels).  A wave owns 32 output pixels x up to 64 filters (2 x 4 accumulator tiles) and walks taps x channels in
//     steps of 32 channels.  What makes it general:
//       - a pixel's window position is y = oy stride - pad_h + ky, x = ox stride - pad_w + kx; a tap outside the image, a pixel row past M and a k slice past
//         Cin (Cin = 8, 48, 80 are no multiples of 32) load nothing and contribute zeros -- no address outside a tensor is formed into a load;
//       - channels creal .. Cin of an input pixel are masked to zero after the load (the first layer reads the front end's 8-channel rows, 3 real);
//       - the last filter chunk may hold fewer than four 16-filter tiles (Cout = 48, 96, 160, 288, 320, 448): the tile count is uniform per workgroup.
//     Layers with Cin % 32 == 0 and no padding channels (all but five of the 94) take the instantiation without the last two guards: unconditional loads
//     (a tap outside the image is zeroed by a bit mask, a filter tile past Cout re-reads the last filter row and is not stored), the next channel step's six
//     fragments in flight while a step's eight MFMAs run.  The epilogue is
//     relu(acc + bias) with the BatchNorm-folded fp32 bias.  The filters of a layer (at most 1.5 MB) stay in L2; no LDS, no barrier.
//   * incep_maxpool_kernel (3x3 stride 2, every window inside the image) into a concat slice; incep_avgpool_kernel (3x3 stride 1 pad 1, always / 9);
//   * incep_mean_kernel + incep_fc_kernel: the global mean in fp32 and fc on it -- the pooled features are never rounded to fp16.
#include "ops.h"

namespace {

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

__device__ __forceinline__ f16x8 ld8(const f16* p) { return *reinterpret_cast<const f16x8*>(p); }

// v where m is all ones, zeros where m is 0
__device__ __forceinline__ f16x8 mask8(f16x8 v, unsigned m) {
    u32x4 b = __builtin_bit_cast(u32x4, v);
    b &= u32x4{m, m, m, m};
    return __builtin_bit_cast(f16x8, b);
}

constexpr int CV_MT = 2, CV_NT = 4;          // a wave's tile: 16 CV_MT pixels x 16 CV_NT filters

struct ConvParams {
    const f16* x; const f16* w; const float* bias; f16* out;
    long M, ld;
    int H, W, Cin, creal, Cout, kh, kw, stride, pad_h, pad_w, Ho, Wo, col;
};

// FULL: Cin % 32 == 0 and every channel real -- no k-slice guard and no channel mask, every load unconditional (a tap outside the image reads the tensor's
// first pixel and is replaced by zeros; a filter tile past Cout reads the last filter row and is dropped by the epilogue) and a software-pipelined channel loop
template <bool FULL>
__global__ __launch_bounds__(256) void incep_conv_kernel(const ConvParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, kq = lane >> 4;
    const long m_base = ((long)blockIdx.x * 4 + wave) * (16 * CV_MT);
    if (m_base >= p.M) return;                                  // whole waves leave; there is no barrier below
    const int n0 = blockIdx.y * (16 * CV_NT);
    const int ntiles = min(CV_NT, (p.Cout - n0) / 16);          // >= 1 by the grid's size
    int iy0[CV_MT], ix0[CV_MT];
    long pb[CV_MT];                                             // first pixel of the sample
    bool pv[CV_MT];
#pragma unroll
    for (int mt = 0; mt < CV_MT; ++mt) {
        const long m = m_base + mt * 16 + col;
        pv[mt] = m < p.M;
        const long mm = pv[mt] ? m : 0;
        const int ox = (int)(mm % p.Wo);
        const long t = mm / p.Wo;
        const int oy = (int)(t % p.Ho);
        iy0[mt] = oy * p.stride - p.pad_h; ix0[mt] = ox * p.stride - p.pad_w;
        pb[mt] = (t / p.Ho) * (long)p.H * p.W;
    }
    f32x4 acc[CV_MT][CV_NT];
#pragma unroll
    for (int mt = 0; mt < CV_MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < CV_NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int Cin = p.Cin;
    const long K = (long)p.kh * p.kw * Cin;                     // row length of w
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool mask = p.creal < Cin;
    const f16* wrow = p.w + (long)(n0 + col) * K + kq * 8;
    long wtile[CV_NT];                                          // FULL: offset of this lane's filter row in tile nt from wrow, clamped into the tensor
#pragma unroll
    for (int nt = 0; nt < CV_NT; ++nt) wtile[nt] = (long)(min(n0 + nt * 16 + col, p.Cout - 1) - (n0 + col)) * K;
    for (int ky = 0; ky < p.kh; ++ky) {
        for (int kx = 0; kx < p.kw; ++kx) {
            const f16* xp[CV_MT];
            bool ok[CV_MT];
#pragma unroll
            for (int mt = 0; mt < CV_MT; ++mt) {
                const int yy = iy0[mt] + ky, xx = ix0[mt] + kx;
                ok[mt] = pv[mt] && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;
                xp[mt] = p.x + (ok[mt] ? (pb[mt] + (long)yy * p.W + xx) * Cin : 0) + kq * 8;
            }
            const f16* wp = wrow + (long)(ky * p.kw + kx) * Cin;
            if constexpr (FULL) {
                // the six fragments of a channel step are loaded together and the next step's are in flight while this step's MFMAs run
                unsigned am[CV_MT];
                f16x8 av[CV_MT], wv[CV_NT];
#pragma unroll
                for (int mt = 0; mt < CV_MT; ++mt) { am[mt] = ok[mt] ? 0xffffffffu : 0u; av[mt] = ld8(xp[mt]); }
#pragma unroll
                for (int nt = 0; nt < CV_NT; ++nt) wv[nt] = ld8(wp + wtile[nt]);
                for (int c0 = 0; c0 < Cin; c0 += 32) {
                    f16x8 an[CV_MT], wn[CV_NT];
#pragma unroll
                    for (int mt = 0; mt < CV_MT; ++mt) an[mt] = av[mt];
#pragma unroll
                    for (int nt = 0; nt < CV_NT; ++nt) wn[nt] = wv[nt];
                    if (c0 + 32 < Cin) {                        // (uniform)
#pragma unroll
                        for (int mt = 0; mt < CV_MT; ++mt) an[mt] = ld8(xp[mt] + c0 + 32);
#pragma unroll
                        for (int nt = 0; nt < CV_NT; ++nt) wn[nt] = ld8(wp + wtile[nt] + c0 + 32);
                    }
                    f16x8 a[CV_MT];
#pragma unroll
                    for (int mt = 0; mt < CV_MT; ++mt) a[mt] = mask8(av[mt], am[mt]);
#pragma unroll
                    for (int nt = 0; nt < CV_NT; ++nt)
#pragma unroll
                        for (int mt = 0; mt < CV_MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[nt], a[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
                    for (int mt = 0; mt < CV_MT; ++mt) av[mt] = an[mt];
#pragma unroll
                    for (int nt = 0; nt < CV_NT; ++nt) wv[nt] = wn[nt];
                }
            } else {
                for (int c0 = 0; c0 < Cin; c0 += 32) {
                    const bool inb = c0 + kq * 8 < Cin;         // this lane's 8 channels exist (Cin % 8 == 0: all or none)
                    f16x8 a[CV_MT];
#pragma unroll
                    for (int mt = 0; mt < CV_MT; ++mt) a[mt] = (ok[mt] && inb) ? ld8(xp[mt] + c0) : zero;
                    if (mask) {
#pragma unroll
                        for (int mt = 0; mt < CV_MT; ++mt)
#pragma unroll
                            for (int e = 0; e < 8; ++e) a[mt][e] = c0 + kq * 8 + e < p.creal ? a[mt][e] : (f16)0.0f;
                    }
#pragma unroll
                    for (int nt = 0; nt < CV_NT; ++nt) {
                        if (nt < ntiles) {
                            const f16x8 wf = inb ? ld8(wp + (long)nt * 16 * K + c0) : zero;
#pragma unroll
                            for (int mt = 0; mt < CV_MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, a[mt], acc[mt][nt], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // D: column = pixel (lane & 15), rows = filters 4 (lane >> 4) + r of the 16-filter tile
#pragma unroll
    for (int mt = 0; mt < CV_MT; ++mt) {
        if (!pv[mt]) continue;
        f16* orow = p.out + (m_base + mt * 16 + col) * p.ld + p.col;
#pragma unroll
        for (int nt = 0; nt < CV_NT; ++nt) {
            if (nt >= ntiles) continue;
            const int ch = n0 + nt * 16 + kq * 4;
            f16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = (f16)fmaxf(acc[mt][nt][r] + (p.bias ? p.bias[ch + r] : 0.f), 0.f);
            *reinterpret_cast<f16x4*>(orow + ch) = o;
        }
    }
}

__global__ __launch_bounds__(256) void incep_maxpool_kernel(const f16* __restrict__ x, int H, int W, int C8, int Ho, int Wo, long total, f16* __restrict__ out,
                                                            long ld, int col) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    const long row = i / C8;
    long t = row;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const long b = t / Ho;
    const f16* base = x + (((b * H + oy * 2) * W + ox * 2) * C8 + c8) * 8;          // windows lie inside the image: 2 (Ho - 1) + 2 <= H - 1
    f16x8 m = ld8(base);
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        const f16x8 v = ld8(base + ((long)(k / 3) * W + k % 3) * C8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
    }
    *reinterpret_cast<f16x8*>(out + row * ld + col + c8 * 8) = m;
}

__global__ __launch_bounds__(256) void incep_avgpool_kernel(const f16* __restrict__ x, int H, int W, int C8, long total, f16* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    long t = i / C8;
    const int px = (int)(t % W); t /= W;
    const int py = (int)(t % H);
    const long b = t / H;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = py + k / 3 - 1, xx = px + k % 3 - 1;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const f16x8 v = ld8(x + (((b * H + yy) * W + xx) * C8 + c8) * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
    }
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)(s[e] / 9.0f);
    *reinterpret_cast<f16x8*>(out + i * 8) = o;
}

__global__ __launch_bounds__(256) void incep_mean_kernel(const f16* __restrict__ x, long HW, int C8, long total, float* __restrict__ mean) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    const long b = i / C8;
    const f16* p = x + (b * HW * C8 + c8) * 8;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long r = 0; r < HW; ++r) {
        const f16x8 v = ld8(p + r * C8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) mean[i * 8 + e] = s[e] / (float)HW;
}

// one wave per logit
__global__ __launch_bounds__(256) void incep_fc_kernel(const float* __restrict__ mean, const f16* __restrict__ w, const float* __restrict__ bias, int C, int N,
                                                       long total, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= total) return;
    const int n = (int)(i % N);
    const float* m = mean + (i / N) * C;
    const f16* wr = w + (long)n * C;
    float s = 0.f;
    for (int k = lane * 8; k < C; k += 512) {
        const f16x8 wv = ld8(wr + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += m[k + e] * (float)wv[e];
    }
    s = wave_sum(s);
    if (lane == 0) out[i] = s + (bias ? bias[n] : 0.f);
}

}  // namespace

int launch_incep_conv(const IncepConvArgs& a, hipStream_t s) {
    if (!a.x || !a.w || !a.out) CS_FAIL(CS_E_ARG, "incep conv: x, w, out required");
    if (a.Cin < 8 || a.Cin % 8 || a.creal < 1 || a.creal > a.Cin) CS_FAIL(CS_E_SHAPE, "incep conv: Cin = %d must be a multiple of 8 with 1 .. Cin real channels (%d)", a.Cin, a.creal);
    if (a.Cout < 16 || a.Cout % 16) CS_FAIL(CS_E_SHAPE, "incep conv: Cout = %d must be a multiple of 16", a.Cout);
    if (a.kh < 1 || a.kh > 7 || a.kw < 1 || a.kw > 7 || (a.stride != 1 && a.stride != 2) || a.pad_h < 0 || a.pad_w < 0 || a.pad_h >= a.kh || a.pad_w >= a.kw)
        CS_FAIL(CS_E_SHAPE, "incep conv: filter %d x %d, stride %d, pad (%d, %d): filters up to 7 x 7, stride 1 | 2, pad < filter", a.kh, a.kw, a.stride, a.pad_h, a.pad_w);
    if (a.B < 0 || a.H < 1 || a.W < 1 || a.H + 2 * a.pad_h < a.kh || a.W + 2 * a.pad_w < a.kw) CS_FAIL(CS_E_SHAPE, "incep conv: a %d x %d image holds no %d x %d window", a.H, a.W, a.kh, a.kw);
    if (a.col < 0 || a.col % 8 || a.ld % 8 || (long)a.col + a.Cout > a.ld) CS_FAIL(CS_E_SHAPE, "incep conv: the slice [%d, %d) does not fit a row of %ld (multiples of 8)", a.col, a.col + a.Cout, a.ld);
    ConvParams p{};
    p.Ho = incep_out_size(a.H, a.kh, a.stride, a.pad_h); p.Wo = incep_out_size(a.W, a.kw, a.stride, a.pad_w);
    p.M = (long)a.B * p.Ho * p.Wo;
    if (p.M == 0) return CS_OK;
    const long gx = (p.M + 4 * 16 * CV_MT - 1) / (4 * 16 * CV_MT);
    if (gx > 0x7fffffffL) CS_FAIL(CS_E_SHAPE, "incep conv: too many pixels for one launch");
    p.x = a.x; p.w = a.w; p.bias = a.bias; p.out = a.out; p.ld = a.ld; p.col = a.col;
    p.H = a.H; p.W = a.W; p.Cin = a.Cin; p.creal = a.creal; p.Cout = a.Cout; p.kh = a.kh; p.kw = a.kw; p.stride = a.stride; p.pad_h = a.pad_h; p.pad_w = a.pad_w;
    const dim3 grid((unsigned)gx, (unsigned)((a.Cout + 16 * CV_NT - 1) / (16 * CV_NT)));
    if (a.Cin % 32 == 0 && a.creal == a.Cin) hipLaunchKernelGGL(incep_conv_kernel<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(incep_conv_kernel<false>, grid, dim3(256), 0, s, p);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_incep_maxpool(const f16* x, int B, int H, int W, int C, f16* out, long ld, int col, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "incep maxpool: null pointer");
    if (B < 0 || H < 3 || W < 3 || C < 8 || C % 8) CS_FAIL(CS_E_SHAPE, "incep maxpool: C %% 8 == 0 and H, W >= 3 required");
    if (col < 0 || col % 8 || ld % 8 || (long)col + C > ld) CS_FAIL(CS_E_SHAPE, "incep maxpool: the slice [%d, %d) does not fit a row of %ld (multiples of 8)", col, col + C, ld);
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const long total = (long)B * Ho * Wo * (C / 8);
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "incep maxpool: too large for one launch");
    hipLaunchKernelGGL(incep_maxpool_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, H, W, C / 8, Ho, Wo, total, out, ld, col);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_incep_avgpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) {
    if (!x || !out) CS_FAIL(CS_E_ARG, "incep avgpool: null pointer");
    if (out == x) CS_FAIL(CS_E_ARG, "incep avgpool: out must not alias x");
    if (B < 0 || H < 1 || W < 1 || C < 8 || C % 8) CS_FAIL(CS_E_SHAPE, "incep avgpool: C %% 8 == 0 and positive sizes required");
    const long total = (long)B * H * W * (C / 8);
    if (total == 0) return CS_OK;
    if (total > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "incep avgpool: too large for one launch");
    hipLaunchKernelGGL(incep_avgpool_kernel, dim3(blocks_for(total)), dim3(256), 0, s, x, H, W, C / 8, total, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_incep_mean(const f16* x, int B, long HW, int C, float* mean, hipStream_t s) {
    if (!x || !mean) CS_FAIL(CS_E_ARG, "incep mean: null pointer");
    if (B < 0 || HW < 1 || C < 8 || C % 8) CS_FAIL(CS_E_SHAPE, "incep mean: C %% 8 == 0 and positive sizes required");
    if (B == 0) return CS_OK;
    const long t1 = (long)B * (C / 8);
    if (t1 > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "incep mean: too large for one launch");
    hipLaunchKernelGGL(incep_mean_kernel, dim3(blocks_for(t1)), dim3(256), 0, s, x, HW, C / 8, t1, mean);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_incep_head(const f16* x, int B, long HW, int C, const f16* w, const float* bias, int N, float* mean, float* logits, hipStream_t s) {
    if (!x || !w || !mean || !logits) CS_FAIL(CS_E_ARG, "incep head: null pointer");
    if (B < 0 || HW < 1 || C < 8 || C % 8 || N < 1) CS_FAIL(CS_E_SHAPE, "incep head: C %% 8 == 0 and positive sizes required");
    if (B == 0) return CS_OK;
    const long t1 = (long)B * (C / 8), t2 = (long)B * N;
    if (t1 > 0x7fffffffL * 256 || (t2 + 3) / 4 > 0x7fffffffL) CS_FAIL(CS_E_SHAPE, "incep head: too large for one launch");
    const int rc = launch_incep_mean(x, B, HW, C, mean, s);
    if (rc != CS_OK) return rc;
    hipLaunchKernelGGL(incep_fc_kernel, dim3((unsigned)((t2 + 3) / 4)), dim3(256), 0, s, mean, w, bias, C, N, t2, logits);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
