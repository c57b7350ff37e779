// Host-only stand-ins for the launchers fid.cpp calls beyond those of incep_stubs.cpp (tests/sanitize/fid_harness.cpp; TEST INFRASTRUCTURE, never linked into
// libconsolver_hip.so): every stub touches the first and last byte of each tensor the real kernel would read or write, sizes from the launch arguments -- the
// resize tables included, and for every output index of a table the first and last input element its taps reach.
#include "../../consolver_amd/csrc/ops.h"

#include <cstdlib>

static volatile unsigned char g_fid_sink;
static void rd(const void* p, size_t bytes) { if (p && bytes) { g_fid_sink = ((const volatile unsigned char*)p)[0]; g_fid_sink = ((const volatile unsigned char*)p)[bytes - 1]; } }
static void wr(void* p, size_t bytes) { if (p && bytes) { ((volatile unsigned char*)p)[0] = 1; ((volatile unsigned char*)p)[bytes - 1] = 1; } }

int launch_incep_mean(const f16* x, int B, long HW, int C, float* mean, hipStream_t) {
    rd(x, (size_t)B * HW * C * 2); wr(mean, (size_t)B * C * 4); return CS_OK;
}
int launch_fid_front_end(const void* images, int dtype, int B, int H, int W, const FidResizePlan& pl, const float* mean, const float* stdv, float* tmp, f16* patches,
                         float* resized, hipStream_t) {
    const size_t S = (size_t)pl.out, esz = dtype == CS_U8 ? 1 : (dtype == CS_F16 ? 2 : 4);
    rd(images, (size_t)B * 3 * H * W * esz); rd(mean, 3 * 4); rd(stdv, 3 * 4);
    rd(pl.h_lo, S * 4); rd(pl.h_cnt, S * 4); rd(pl.h_kk, S * pl.h_ksize * 8); rd(pl.v_lo, S * 4); rd(pl.v_cnt, S * 4); rd(pl.v_kk, S * pl.v_ksize * 8);
    for (size_t i = 0; i < S; ++i) {                    // the taps stay inside the image and inside their table row
        if (pl.h_lo[i] < 0 || pl.h_cnt[i] < 1 || pl.h_lo[i] + pl.h_cnt[i] > W || pl.h_cnt[i] > pl.h_ksize) abort();
        if (pl.v_lo[i] < 0 || pl.v_cnt[i] < 1 || pl.v_lo[i] + pl.v_cnt[i] > H || pl.v_cnt[i] > pl.v_ksize) abort();
    }
    wr(tmp, (size_t)B * 3 * H * S * 4); wr(patches, (size_t)B * S * S * 8 * 2); wr(resized, (size_t)B * 3 * S * S * 4);
    return CS_OK;
}
int launch_fid_avgpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t) {
    const size_t n = (size_t)B * H * W * C * 2;
    rd(x, n); wr(out, n); return CS_OK;
}
int launch_fid_maxpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t) {
    const size_t n = (size_t)B * H * W * C * 2;
    rd(x, n); wr(out, n); return CS_OK;
}
int launch_fid_stats_accumulate(const float* f, long n, int d, double* sum, double* outer, hipStream_t) {
    rd(f, (size_t)n * d * 4); wr(sum, (size_t)d * 8); wr(outer, (size_t)d * d * 8); return CS_OK;
}
int launch_fid_stats_finalize(const double* sum, const double* outer, long, int d, double* mu, double* sigma, hipStream_t) {
    rd(sum, (size_t)d * 8); rd(outer, (size_t)d * d * 8); wr(mu, (size_t)d * 8); wr(sigma, (size_t)d * d * 8); return CS_OK;
}
