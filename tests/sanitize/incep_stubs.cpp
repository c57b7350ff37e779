// Host-only stand-ins for the launchers of incep_ops.hip (tests/sanitize/incep_harness.cpp; TEST INFRASTRUCTURE, never linked into libconsolver_hip.so), next to
// stubs.cpp: every stub touches the first and last byte of each tensor the real kernel would read or write, sizes from the launch arguments.
#include "../../consolver_amd/csrc/ops.h"

static volatile unsigned char g_incep_sink;
static void rd(const void* p, size_t bytes) { if (p && bytes) { g_incep_sink = ((const volatile unsigned char*)p)[0]; g_incep_sink = ((const volatile unsigned char*)p)[bytes - 1]; } }
static void wr(void* p, size_t bytes) { if (p && bytes) { ((volatile unsigned char*)p)[0] = 1; ((volatile unsigned char*)p)[bytes - 1] = 1; } }

int launch_incep_conv(const IncepConvArgs& a, hipStream_t) {
    const size_t Ho = incep_out_size(a.H, a.kh, a.stride, a.pad_h), Wo = incep_out_size(a.W, a.kw, a.stride, a.pad_w);
    rd(a.x, (size_t)a.B * a.H * a.W * a.Cin * 2); rd(a.w, (size_t)a.Cout * a.kh * a.kw * a.Cin * 2); rd(a.bias, (size_t)a.Cout * 4);
    wr(a.out + a.col, (((size_t)a.B * Ho * Wo - 1) * a.ld + a.Cout) * 2); return CS_OK;
}
int launch_incep_maxpool(const f16* x, int B, int H, int W, int C, f16* out, long ld, int col, hipStream_t) {
    const size_t Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    rd(x, (size_t)B * H * W * C * 2); wr(out + col, (((size_t)B * Ho * Wo - 1) * ld + C) * 2); return CS_OK;
}
int launch_incep_avgpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t) {
    const size_t n = (size_t)B * H * W * C * 2;
    rd(x, n); wr(out, n); return CS_OK;
}
int launch_incep_head(const f16* x, int B, long HW, int C, const f16* w, const float* bias, int N, float* mean, float* logits, hipStream_t) {
    rd(x, (size_t)B * HW * C * 2); rd(w, (size_t)N * C * 2); rd(bias, (size_t)N * 4); wr(mean, (size_t)B * C * 4); wr(logits, (size_t)B * N * 4); return CS_OK;
}
