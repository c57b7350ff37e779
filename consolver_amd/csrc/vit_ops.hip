// Kernels of the DINOv2 and CLIP image-similarity rewards (vit.cpp, clip_vision.cpp; edit_ppo/reward_model.py:217-257, 512-552) that are not GEMM / attention /
// LayerNorm:
//
//   * the image front end: ToPILImage's quantisation, PIL's two-pass fixed-point bicubic resize restricted to the center-crop window, the processor's
//     rescale + normalise, written straight as the patch-embedding GEMM's A operand [B * tokens][K padded to 64];
//   * token assembly (CLS row + position table), exact (erf) GELU, the final LayerNorm on the CLS rows only, and the reward tail
//     F.normalize -> F.cosine_similarity -> (cos + 1) * 50;
//   * CLIP's two ends: token assembly fused with pre_layrnorm (one wave per token row, the sum and the normalisation in fp32 registers, one rounding), and
//     post_layernorm of the CLS row + the bias-free visual_projection (one workgroup per image, the normalised row in LDS, one wave per output column).
//
// Everything here is bandwidth- or latency-trivial next to the encoder's GEMMs (one image = 46 GFLOP): plain one-thread-per-output kernels, integer
// arithmetic identical to PIL's (22 fractional bits, accumulator seeded with 2^21, arithmetic shift, clip to 8 bits), so the uint8 crop is bit-exact.
#include "ops.h"

namespace {

constexpr int RS_BITS = 22;

// ToPILImage on a float tensor: x.mul(255).byte() -- the product is rounded in the tensor's OWN dtype, the conversion truncates.  The clamp to [0, 1]
// in front is unconditional here (the reference clamps when min < 0; decode_latents never leaves [0, 1]); NaN -> 0.
__device__ __forceinline__ int quant255(f16 v) {
    f16 x = v > (f16)0.0f ? v : (f16)0.0f;
    x = x < (f16)1.0f ? x : (f16)1.0f;
    const f16 p = x * (f16)255.0f;        // v_mul_f16: one rounding to fp16, as torch's half multiply
    return (int)(float)p;
}
__device__ __forceinline__ int quant255(float v) {
    float x = v > 0.0f ? v : 0.0f;
    x = x < 1.0f ? x : 1.0f;
    return (int)(x * 255.0f);
}
__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> RS_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct ResizeTab { const int* lo; const int* cnt; const int* kk; int ksize; };     // per output index of the crop window: first input index, taps, fixed-point taps

// horizontal pass: tmp[bc][r][x] for input rows row0 .. row0 + nrows (the rows the vertical pass of the crop window reads), x in the crop window
template <typename T>
__global__ __launch_bounds__(256) void vit_hresize_kernel(const T* __restrict__ src, int BC, int H, int W, int row0, int nrows, int cw, ResizeTab th,
                                                          unsigned char* __restrict__ tmp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)BC * nrows * cw) return;
    const int x = (int)(i % cw);
    const long t = i / cw;
    const int r = (int)(t % nrows), bc = (int)(t / nrows);
    const T* row = src + ((long)bc * H + (row0 + r)) * W + th.lo[x];
    const int* kk = th.kk + (long)x * th.ksize;
    const int n = th.cnt[x];
    int acc = 1 << (RS_BITS - 1);
    for (int j = 0; j < n; ++j) acc += quant255(row[j]) * kk[j];
    tmp[i] = (unsigned char)clip8(acc);
}

// vertical pass + normalise + patch rows: A[(b * Gh * Gw + py * Gw + px)][c * P * P + ky * P + kx], columns K .. Kpad zero (the window is P Gh rows of cw = P Gw
// columns; the square crop has Gh = Gw)
__global__ __launch_bounds__(256) void vit_vresize_patch_kernel(const unsigned char* __restrict__ tmp, int B, int row0, int nrows, int cw, ResizeTab tv, int P, int Gh,
                                                                int Gw, int K, int Kpad, float m0, float m1, float m2, float s0, float s1, float s2, double rescale,
                                                                f16* __restrict__ patches, unsigned char* __restrict__ crop) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * Gh * Gw * Kpad) return;
    const int k = (int)(i % Kpad);
    if (k >= K) { patches[i] = (f16)0.0f; return; }
    const long t = i / Kpad;
    const int p = (int)(t % (Gh * Gw)), b = (int)(t / (Gh * Gw));
    const int c = k / (P * P), r = k - c * P * P, ky = r / P, kx = r - ky * P;
    const int y = (p / Gw) * P + ky, x = (p % Gw) * P + kx;
    const unsigned char* col = tmp + ((long)(b * 3 + c) * nrows + (tv.lo[y] - row0)) * cw + x;
    const int* kk = tv.kk + (long)y * tv.ksize;
    const int n = tv.cnt[y];
    int acc = 1 << (RS_BITS - 1);
    for (int j = 0; j < n; ++j) acc += (int)col[(long)j * cw] * kk[j];
    const int u = clip8(acc);
    if (crop) crop[((long)(b * 3 + c) * (P * Gh) + y) * cw + x] = (unsigned char)u;
    const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
    const float v = (float)((double)u * rescale);        // the processor rescales in double and rounds to fp32, then normalises in fp32
    patches[i] = (f16)((v - mean) / sd);
}

// x[b][0] = cls + pos[0]; x[b][1 + p] = pe[b * NP + p] + pos[1 + p]   (fp32 add, one rounding); 8 channels per thread
__global__ __launch_bounds__(256) void vit_tokens_kernel(const f16* __restrict__ pe, const f16* __restrict__ cls, const f16* __restrict__ pos, f16* __restrict__ x,
                                                         int B, int NP, int D) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int D8 = D / 8;
    if (i >= (long)B * (NP + 1) * D8) return;
    const int d = (int)(i % D8) * 8;
    const long row = i / D8;
    const int t = (int)(row % (NP + 1)), b = (int)(row / (NP + 1));
    const f16x8 a = t == 0 ? *reinterpret_cast<const f16x8*>(cls + d) : *reinterpret_cast<const f16x8*>(pe + ((long)b * NP + t - 1) * D + d);
    const f16x8 q = *reinterpret_cast<const f16x8*>(pos + (long)t * D + d);
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f16)((float)a[e] + (float)q[e]);
    *reinterpret_cast<f16x8*>(x + row * D + d) = o;
}

// torch upsample_bicubic2d (align_corners = False, size given: scale = in / out per axis) of the trained position grid [s][s][D] fp32 to [gh][gw][D], written as
// rows 1 .. gh gw of the fp16 table launch_vit_tokens reads (row 0 zero: the packed CLS token carries the class row).  fp32 arithmetic in the order of
// torch's CPU kernel, one rounding to fp16.  Which of its multiply-adds that kernel's build fuses was found by comparing its weights and sums bit for bit
// (an fp32 emulation of every candidate against F.interpolate): source = fma(scale, dst + 0.5, -0.5); lambda = source - floor(source); of the A = -0.75
// coefficients the outer polynomial's first two steps are fused and nothing else; each sum of four terms starts from the SECOND product and takes the first,
// third and fourth as fmas, over x inside the sum over y.  With that the table is torch's fp32 result bit for bit, rounded once.
// Contraction is switched off so that exactly the fmas written here are fused.  One thread per 8 channels of one output position: 16 clamped taps of 32
// bytes each, consecutive lanes on consecutive channels.
__device__ __forceinline__ void pos_cubic_coeffs(float t, float* k) {
#pragma clang fp contract(off)
    const float A = -0.75f;
    const float a = t + 1.0f, b = 1.0f - t, c = b + 1.0f;
    k[0] = fmaf(fmaf(A, a, -5.0f * A), a, 8.0f * A) * a - 4.0f * A;
    k[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    k[2] = ((A + 2.0f) * b - (A + 3.0f)) * b * b + 1.0f;
    k[3] = fmaf(fmaf(A, c, -5.0f * A), c, 8.0f * A) * c - 4.0f * A;
}
__global__ __launch_bounds__(256) void vit_pos_interp_kernel(const float* __restrict__ grid, int s, int gh, int gw, int D8, float sy, float sx, long total,
                                                             f16* __restrict__ table) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int d = (int)(i % D8) * 8;
    const long row = i / D8;
    f16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row > 0) {
        const int p = (int)(row - 1), oy = p / gw, ox = p - oy * gw;
        const float ry = fmaf(sy, (float)oy + 0.5f, -0.5f), rx = fmaf(sx, (float)ox + 0.5f, -0.5f);
        const float fy = floorf(ry), fx = floorf(rx);
        const int iy = (int)fy, ix = (int)fx;
        float ky[4], kx[4];
        pos_cubic_coeffs(fminf(fmaxf(ry - fy, 0.0f), 1.0f), ky);
        pos_cubic_coeffs(fminf(fmaxf(rx - fx, 0.0f), 1.0f), kx);
        // a sum of four terms is t1 w1 first, then fma(t0, w0, .), fma(t2, w2, .), fma(t3, w3, .): the order of that build, over x and over y alike
        float acc[8];
#pragma unroll
        for (int aa = 0; aa < 4; ++aa) {
            const int a = aa == 0 ? 1 : (aa == 1 ? 0 : aa);
            const int yy = min(max(iy - 1 + a, 0), s - 1);
            float r[8];
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                const int b = bb == 0 ? 1 : (bb == 1 ? 0 : bb);
                const float* src = grid + ((long)yy * s + min(max(ix - 1 + b, 0), s - 1)) * (D8 * 8) + d;
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    r[e] = bb ? fmaf(v0[e], kx[b], r[e]) : v0[e] * kx[b];
                    r[e + 4] = bb ? fmaf(v1[e], kx[b], r[e + 4]) : v1[e] * kx[b];
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = aa ? fmaf(r[e], ky[a], acc[e]) : r[e] * ky[a];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f16)acc[e];
    }
    *reinterpret_cast<f16x8*>(table + i * 8) = o;
}

// x <- 0.5 x (1 + erf(x / sqrt 2)) in place (nn.GELU, the "gelu" activation of the Dinov2 MLP)
__global__ __launch_bounds__(256) void gelu_erf_kernel(f16* __restrict__ x, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    f16x8 v = *reinterpret_cast<const f16x8*>(x + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = (float)v[e];
        v[e] = (f16)(0.5f * f * (1.0f + erff(f * 0.70710678118654752f)));
    }
    *reinterpret_cast<f16x8*>(x + i * 8) = v;
}

// final LayerNorm on row 0 of every sample only: out[b][D] fp32 (one wave per sample, two passes over the row in fp32)
__global__ __launch_bounds__(64) void vit_cls_layer_norm_kernel(const f16* __restrict__ x, long sample_stride, const f16* __restrict__ g, const f16* __restrict__ be,
                                                                float eps, int D, float* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const f16* row = x + (long)b * sample_stride;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += (float)row[d];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) { const float c = (float)row[d] - mean; q += c * c; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    for (int d = lane; d < D; d += 64) out[(long)b * D + d] = ((float)row[d] - mean) * rstd * (float)g[d] + (float)be[d];
}

// reward tail: a = F.normalize(pred), t = F.normalize(target) (eps 1e-12); cos = a.t / (max(|a|, 1e-8) max(|t|, 1e-8)); out = (cos + 1) * 50
__global__ __launch_bounds__(64) void cosine_reward_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, long tgt_stride, int D, float* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* a = pred + (long)b * D;
    const float* t = tgt + (long)b * tgt_stride;
    float na = 0.f, nt = 0.f;
    for (int d = lane; d < D; d += 64) { na += a[d] * a[d]; nt += t[d] * t[d]; }
    const float ia = 1.0f / fmaxf(sqrtf(wave_sum(na)), 1e-12f), it = 1.0f / fmaxf(sqrtf(wave_sum(nt)), 1e-12f);
    float dot = 0.f, ma = 0.f, mt = 0.f;
    for (int d = lane; d < D; d += 64) {
        const float u = a[d] * ia, v = t[d] * it;
        dot += u * v; ma += u * u; mt += v * v;
    }
    dot = wave_sum(dot); ma = wave_sum(ma); mt = wave_sum(mt);
    if (lane == 0) out[b] = (dot / (fmaxf(sqrtf(ma), 1e-8f) * fmaxf(sqrtf(mt), 1e-8f)) + 1.0f) * 50.0f;
}

// CLIP vision embeddings + pre_layrnorm: row (b, t) = (t == 0 ? cls : pe[b * NP + t - 1]) + pos[t], then LayerNorm over D -- one wave per row, the row in fp32
// registers from the 16-byte loads to the one fp16 store (lane l holds the 8-channel chunks l, l + 64, ...: NCH of them, D <= 512 NCH).  Mean first, then the
// variance of the centred values.
template <int NCH>
__global__ __launch_bounds__(256) void clipv_tokens_ln_kernel(const f16* __restrict__ pe, const f16* __restrict__ cls, const f16* __restrict__ pos,
                                                              const f16* __restrict__ g, const f16* __restrict__ be, float eps, f16* __restrict__ x,
                                                              long rows, int NP, int D) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                  // (whole waves leave: no barrier below)
    const int t = (int)(row % (NP + 1));
    const long b = row / (NP + 1);
    const f16* src = t == 0 ? cls : pe + (b * NP + t - 1) * D;
    const f16* prow = pos + (long)t * D;
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int d = (j * 64 + lane) * 8;
        if (d < D) {
            const f16x8 a = *reinterpret_cast<const f16x8*>(src + d), q = *reinterpret_cast<const f16x8*>(prow + d);
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[j][e] = (float)a[e] + (float)q[e]; s += v[j][e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = 0.f;
        }
    }
    const float mean = wave_sum(s) / (float)D;
    float q2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if ((j * 64 + lane) * 8 < D) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[j][e] -= mean; q2 += v[j][e] * v[j][e]; }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q2) / (float)D + eps);
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int d = (j * 64 + lane) * 8;
        if (d < D) {
            const f16x8 gg = *reinterpret_cast<const f16x8*>(g + d), bb = *reinterpret_cast<const f16x8*>(be + d);
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (f16)(v[j][e] * rstd * (float)gg[e] + (float)bb[e]);
            *reinterpret_cast<f16x8*>(x + row * D + d) = o;
        }
    }
}

// CLIP vision head: out[b][p] = sum_d LayerNorm(x[b * sample_stride + d])[d] * w[p][d]   (post_layernorm of the CLS row, visual_projection without bias).
// One workgroup of 8 waves per image: every wave takes the row's statistics itself (2 KB, no cross-wave reduction), the workgroup writes the normalised
// row to LDS in fp32, then wave w forms the columns w, w + 8, ... as lane-strided dot products with 16-byte weight loads and fp32 accumulation.
constexpr int HEAD_WAVES = 8;
__global__ __launch_bounds__(HEAD_WAVES * 64) void clipv_head_kernel(const f16* __restrict__ x, long sample_stride, const f16* __restrict__ g,
                                                                     const f16* __restrict__ be, float eps, const f16* __restrict__ w, int D, int P,
                                                                     float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float clipv_head_row[];               // [D]
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const f16* row = x + (long)b * sample_stride;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += (float)row[d];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) { const float c = (float)row[d] - mean; q += c * c; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    for (int d = threadIdx.x; d < D; d += HEAD_WAVES * 64) clipv_head_row[d] = ((float)row[d] - mean) * rstd * (float)g[d] + (float)be[d];
    __syncthreads();
    for (int p = wave; p < P; p += HEAD_WAVES) {
        const f16* wr = w + (long)p * D;
        float acc = 0.f;
        for (int d = lane * 8; d < D; d += 512) {
            const f16x8 ww = *reinterpret_cast<const f16x8*>(wr + d);
            const f32x4 n0 = *reinterpret_cast<const f32x4*>(clipv_head_row + d), n1 = *reinterpret_cast<const f32x4*>(clipv_head_row + d + 4);
            acc += n0[0] * (float)ww[0] + n0[1] * (float)ww[1] + n0[2] * (float)ww[2] + n0[3] * (float)ww[3]
                 + n1[0] * (float)ww[4] + n1[1] * (float)ww[5] + n1[2] * (float)ww[6] + n1[3] * (float)ww[7];
        }
        acc = wave_sum(acc);
        if (lane == 0) out[(long)b * P + p] = acc;
    }
}

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int launch_vit_front_end(const void* images, int dtype, int B, int H, int W, const VitResizePlan& pl, const float* mean, const float* stdv, double rescale,
                         int P, int G, int Kpad, unsigned char* tmp, f16* patches, unsigned char* crop, hipStream_t s) {
    return launch_vit_front_end_hw(images, dtype, B, H, W, pl, mean, stdv, rescale, P, G, G, Kpad, tmp, patches, crop, s);
}

int launch_vit_front_end_hw(const void* images, int dtype, int B, int H, int W, const VitResizePlan& pl, const float* mean, const float* stdv, double rescale,
                            int P, int Gh, int Gw, int Kpad, unsigned char* tmp, f16* patches, unsigned char* crop, hipStream_t s) {
    if (!images || !tmp || !patches || !mean || !stdv) CS_FAIL(CS_E_ARG, "vit front end: null pointer");
    if (dtype != CS_F16 && dtype != CS_F32) CS_FAIL(CS_E_UNSUPPORTED, "vit front end: images must be fp16 or fp32");
    if (B <= 0) return B < 0 ? CS_E_SHAPE : CS_OK;
    if (P < 1 || Gh < 1 || Gw < 1 || (long)P * Gh > 0x7fff || (long)P * Gw > 0x7fff) CS_FAIL(CS_E_SHAPE, "vit front end: bad patch grid %d x %d of %d", Gh, Gw, P);
    const int cw = P * Gw, K = 3 * P * P;
    // bounds of everything the two kernels index, checked on the host copy of the plan (vit.cpp builds both from one table)
    if (pl.row0 < 0 || pl.nrows <= 0 || pl.row0 + pl.nrows > H || pl.col_hi > W || pl.col_lo < 0 || Kpad < K || Kpad % 8)
        CS_FAIL(CS_E_SHAPE, "vit front end: resize plan does not fit a %d x %d image", H, W);
    const ResizeTab th{pl.h_lo, pl.h_cnt, pl.h_kk, pl.h_ksize}, tv{pl.v_lo, pl.v_cnt, pl.v_kk, pl.v_ksize};
    const long n1 = (long)B * 3 * pl.nrows * cw, n2 = (long)B * Gh * Gw * Kpad;
    if (n1 > 0x7fffffffL * 256 || n2 > 0x7fffffffL * 256) CS_FAIL(CS_E_SHAPE, "vit front end: batch too large");
    if (dtype == CS_F16) hipLaunchKernelGGL(vit_hresize_kernel<f16>, dim3(blocks_for(n1)), dim3(256), 0, s, (const f16*)images, B * 3, H, W, pl.row0, pl.nrows, cw, th, tmp);
    else hipLaunchKernelGGL(vit_hresize_kernel<float>, dim3(blocks_for(n1)), dim3(256), 0, s, (const float*)images, B * 3, H, W, pl.row0, pl.nrows, cw, th, tmp);
    CS_CHECK_LAUNCH();
    hipLaunchKernelGGL(vit_vresize_patch_kernel, dim3(blocks_for(n2)), dim3(256), 0, s, tmp, B, pl.row0, pl.nrows, cw, tv, P, Gh, Gw, K, Kpad, mean[0], mean[1], mean[2],
                       stdv[0], stdv[1], stdv[2], rescale, patches, crop);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_vit_tokens(const f16* pe, const f16* cls, const f16* pos, f16* x, int B, int NP, int D, hipStream_t s) {
    if (!pe || !cls || !pos || !x || D % 8) CS_FAIL(CS_E_ARG, "vit tokens: pointers required, D %% 8 == 0");
    if (B <= 0) return B < 0 ? CS_E_SHAPE : CS_OK;
    hipLaunchKernelGGL(vit_tokens_kernel, dim3(blocks_for((long)B * (NP + 1) * (D / 8))), dim3(256), 0, s, pe, cls, pos, x, B, NP, D);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_vit_pos_interp(const float* grid, int s, int gh, int gw, int D, f16* table, hipStream_t st) {
    if (!grid || !table) CS_FAIL(CS_E_ARG, "vit position table: null pointer");
    if (s < 1 || gh < 1 || gw < 1 || D < 8 || D % 8 || (long)gh * gw >= 0x7fffffffL / D) CS_FAIL(CS_E_SHAPE, "vit position table: bad grid %d -> %d x %d at D = %d", s, gh, gw, D);
    const long total = ((long)gh * gw + 1) * (D / 8);
    hipLaunchKernelGGL(vit_pos_interp_kernel, dim3(blocks_for(total)), dim3(256), 0, st, grid, s, gh, gw, D / 8, (float)s / (float)gh, (float)s / (float)gw, total, table);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_gelu_erf(f16* x, long n, hipStream_t s) {
    if (!x || n % 8) CS_FAIL(CS_E_ARG, "gelu: x required, n %% 8 == 0");
    if (n <= 0) return CS_OK;
    hipLaunchKernelGGL(gelu_erf_kernel, dim3(blocks_for(n / 8)), dim3(256), 0, s, x, n / 8);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_vit_cls_layer_norm(const f16* x, long sample_stride, const f16* g, const f16* b, float eps, int B, int D, float* out, hipStream_t s) {
    if (!x || !g || !b || !out) CS_FAIL(CS_E_ARG, "vit cls layer norm: null pointer");
    if (B <= 0) return B < 0 ? CS_E_SHAPE : CS_OK;
    hipLaunchKernelGGL(vit_cls_layer_norm_kernel, dim3(B), dim3(64), 0, s, x, sample_stride, g, b, eps, D, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_clipv_tokens_ln(const f16* pe, const f16* cls, const f16* pos, const f16* g, const f16* b, float eps, f16* x, int B, int NP, int D, hipStream_t s) {
    if (!pe || !cls || !pos || !g || !b || !x) CS_FAIL(CS_E_ARG, "clip vision tokens: null pointer");
    if (D < 128 || D % 128 || D > 2048 || NP < 1) CS_FAIL(CS_E_SHAPE, "clip vision tokens: D = %d must be a multiple of 128 up to 2048", D);
    if (B <= 0) return B < 0 ? CS_E_SHAPE : CS_OK;
    const long rows = (long)B * (NP + 1);
    if ((rows + 3) / 4 > 0x7fffffffL) CS_FAIL(CS_E_SHAPE, "clip vision tokens: batch too large");
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    switch ((D + 511) / 512) {
        case 1: hipLaunchKernelGGL(clipv_tokens_ln_kernel<1>, grid, block, 0, s, pe, cls, pos, g, b, eps, x, rows, NP, D); break;
        case 2: hipLaunchKernelGGL(clipv_tokens_ln_kernel<2>, grid, block, 0, s, pe, cls, pos, g, b, eps, x, rows, NP, D); break;
        case 3: hipLaunchKernelGGL(clipv_tokens_ln_kernel<3>, grid, block, 0, s, pe, cls, pos, g, b, eps, x, rows, NP, D); break;
        default: hipLaunchKernelGGL(clipv_tokens_ln_kernel<4>, grid, block, 0, s, pe, cls, pos, g, b, eps, x, rows, NP, D); break;
    }
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_clipv_head(const f16* x, long sample_stride, const f16* g, const f16* b, float eps, const f16* w, int B, int D, int P, float* out, hipStream_t s) {
    if (!x || !g || !b || !w || !out) CS_FAIL(CS_E_ARG, "clip vision head: null pointer");
    if (D < 8 || D % 8 || D > 8192 || P < 1 || sample_stride < D) CS_FAIL(CS_E_SHAPE, "clip vision head: D = %d must be a multiple of 8 up to 8192, P = %d positive", D, P);
    if (B <= 0) return B < 0 ? CS_E_SHAPE : CS_OK;
    hipLaunchKernelGGL(clipv_head_kernel, dim3(B), dim3(HEAD_WAVES * 64), (size_t)D * sizeof(float), s, x, sample_stride, g, b, eps, w, D, P, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int launch_cosine_reward(const float* pred, const float* target, long target_stride, int B, int D, float* out, hipStream_t s) {
    if (!pred || !target || !out || D <= 0) CS_FAIL(CS_E_ARG, "cosine reward: null pointer");
    if (B <= 0) return B < 0 ? CS_E_SHAPE : CS_OK;
    hipLaunchKernelGGL(cosine_reward_kernel, dim3(B), dim3(64), 0, s, pred, target, target_stride, D, out);
    CS_CHECK_LAUNCH();
    return CS_OK;
}
