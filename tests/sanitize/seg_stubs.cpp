// Host-only stand-ins for the launchers of seg_ops.hip (tests/sanitize/seg_harness.cpp; TEST INFRASTRUCTURE, never linked into libconsolver_hip.so), next to
// stubs.cpp: every stub touches the first and last byte of each tensor the real kernel would read or write, sizes from the launch arguments.
#include "../../consolver_amd/csrc/ops.h"

static volatile unsigned char g_seg_sink;
static void rd(const void* p, size_t bytes) { if (p && bytes) { g_seg_sink = ((const volatile unsigned char*)p)[0]; g_seg_sink = ((const volatile unsigned char*)p)[bytes - 1]; } }
static void wr(void* p, size_t bytes) { if (p && bytes) { ((volatile unsigned char*)p)[0] = 1; ((volatile unsigned char*)p)[bytes - 1] = 1; } }

int launch_seg_dwconv_gelu(const f16* x, int B, int H, int W, int C, const f16* w, const f16* bias, f16* out, hipStream_t) {
    const size_t n = (size_t)B * H * W * C * 2;
    rd(x, n); rd(w, (size_t)9 * C * 2); rd(bias, (size_t)C * 2); wr(out, n); return CS_OK;
}
int launch_seg_im2col(const f16* x, int B, int H, int W, int Cs, int, int k, int stride, int pad, int Kp, f16* out, hipStream_t) {
    const size_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    rd(x, (size_t)B * H * W * Cs * 2); wr(out, (size_t)B * Ho * Wo * Kp * 2); return CS_OK;
}
int launch_seg_patchify(const f16* x, int B, int H, int W, int C, int sr, f16* out, hipStream_t) {
    rd(x, (size_t)B * H * W * C * 2); wr(out, (size_t)B * (H / sr) * (W / sr) * sr * sr * C * 2); return CS_OK;
}
int launch_seg_bilinear(const f16* x, int B, int Hi, int Wi, int C, int Ho, int Wo, f16* out, long ld, int col, hipStream_t) {
    rd(x, (size_t)B * Hi * Wi * C * 2);
    wr(out + col, (((size_t)B * Ho * Wo - 1) * ld + C) * 2); return CS_OK;
}
int launch_seg_relu(f16* x, long n, hipStream_t) { wr(x, (size_t)n * 2); return CS_OK; }
int launch_seg_argmax(const f16* x, long M, long ld, int n, int* out, hipStream_t) { rd(x, ((size_t)(M - 1) * ld + n) * 2); wr(out, (size_t)M * 4); return CS_OK; }
int launch_seg_logits(const f16* x, int B, long HW, long ld, int n, float* out, hipStream_t) {
    rd(x, (((size_t)B * HW - 1) * ld + n) * 2); wr(out, (size_t)B * n * HW * 4); return CS_OK;
}
int launch_seg_agreement(const int* pred, const int* target, long target_stride, int B, long n, float* out, hipStream_t) {
    rd(pred, (size_t)B * n * 4); rd(target, ((size_t)(B - 1) * target_stride + n) * 4); wr(out, (size_t)B * 4); return CS_OK;
}
