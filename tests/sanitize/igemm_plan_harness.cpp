// Stand-alone driver of igemm_plan (consolver_amd/csrc/igemm_plan.h) for tests/test_igemm_plan.py: TEST INFRASTRUCTURE, compiled host-only with
// -fsanitize=address,undefined and never linked into libconsolver_hip.so.
//
// stdin, one case per line (integers):
//     B Hi Wi Ho Wo c0 c1 taps stride upsample pad_after_only N geglu lo8 ln_groups pointer_mask splitk_ws_bytes [knob value]...
// pointer_mask: bit i set = the i-th optional pointer of IgemmArgs is non-null, in the order of PTR below.  Every non-null pointer points into a POISONED buffer:
// a plan that dereferenced one would be an AddressSanitizer error (the plan may only test them for null).  Knobs: the cs_set_tuning names the router reads.
// stdout, one line per case:
//     rc family tile_cols variant splits gn_done row_groups slot grid_x grid_y block lds splitk_bytes | error text
// splitk_bytes: what the launch writes into splitk_ws ([splits][M][N] fp32 partial sums), 0 when the plan does not split.
#include "../../consolver_amd/csrc/igemm_plan.h"
#include <sanitizer/asan_interface.h>
#include <cstring>
#include <cstdlib>
#include <string>

static char g_error[1024];
void cs_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_error, sizeof g_error, fmt, ap); va_end(ap); }

enum PTR { P_A0, P_W, P_OUT, P_A1, P_BIAS, P_TEMB, P_RES, P_RES_LO, P_OUT_LO, P_A0_LO, P_A1_LO, P_ROW_STATS, P_ROW_STATS_GROUPS, P_GN_STATS, P_LN_STATS, P_LN_S, P_LN_B, P_W_UP_SUB, P_SPLITK_WS, P_COUNT };
struct Knob { const char* key; int TuneSet::* var; };
static const Knob KNOBS[] = {{"conv_halo", &TuneSet::halo}, {"conv_lw", &TuneSet::conv_lw}, {"gemm_big", &TuneSet::biggemm}, {"gemm_w8", &TuneSet::gemm_w8}, {"gemm_lw", &TuneSet::gemm_lw},
                             {"gemm_as", &TuneSet::gemm_as}, {"gn_fuse", &TuneSet::gn_fuse}, {"xcd_grid", &TuneSet::xcd_grid}, {"epi_fast", &TuneSet::epi_fast}, {"debug", &TuneSet::debug},
                             {"gemm_gm", &TuneSet::gemm_gm}};

int main() {
    alignas(64) static char poisoned[64 * P_COUNT];
    ASAN_POISON_MEMORY_REGION(poisoned, sizeof poisoned);
    char line[4096];
    while (fgets(line, sizeof line, stdin)) {
        char* tok = strtok(line, " \t\n");
        if (!tok || tok[0] == '#') continue;
        long long v[17]; int n = 0;
        for (; tok && n < 17; tok = strtok(nullptr, " \t\n")) v[n++] = atoll(tok);
        if (n != 17) { fprintf(stderr, "igemm_plan_harness: a case needs 17 integers, got %d\n", n); return 2; }
        TuneSet t;
        for (; tok; tok = strtok(nullptr, " \t\n")) {
            const char* val = strtok(nullptr, " \t\n");
            const Knob* k = nullptr;
            for (const Knob& c : KNOBS) if (!strcmp(c.key, tok)) k = &c;
            if (!k || !val) { fprintf(stderr, "igemm_plan_harness: unknown knob '%s' or no value\n", tok); return 2; }
            t.*(k->var) = atoi(val);
        }
        auto ptr = [&](int i) -> void* { return (v[15] >> i & 1) ? (void*)(poisoned + 64 * i) : nullptr; };
        IgemmArgs a{};
        a.B = (int)v[0]; a.Hi = (int)v[1]; a.Wi = (int)v[2]; a.Ho = (int)v[3]; a.Wo = (int)v[4]; a.c0 = (int)v[5]; a.c1 = (int)v[6]; a.taps = (int)v[7]; a.stride = (int)v[8];
        a.upsample = (int)v[9]; a.pad_after_only = (int)v[10]; a.N = (int)v[11]; a.geglu = (int)v[12]; a.lo8 = (int)v[13]; a.ln_groups = (int)v[14]; a.ln_eps = 1e-5f;
        a.a0 = (const f16*)ptr(P_A0); a.w = (const f16*)ptr(P_W); a.out = (f16*)ptr(P_OUT); a.a1 = (const f16*)ptr(P_A1); a.bias = (const f16*)ptr(P_BIAS);
        a.temb = (const f16*)ptr(P_TEMB); a.temb_stride = a.N; a.res = (const f16*)ptr(P_RES); a.res_lo = (const f16*)ptr(P_RES_LO); a.out_lo = (f16*)ptr(P_OUT_LO);
        a.a0_lo = (const f16*)ptr(P_A0_LO); a.a1_lo = (const f16*)ptr(P_A1_LO); a.row_stats = (float*)ptr(P_ROW_STATS); a.row_stats_groups = (int*)ptr(P_ROW_STATS_GROUPS);
        a.gn_stats = (float*)ptr(P_GN_STATS); a.ln_stats = (const float*)ptr(P_LN_STATS); a.ln_s = (const float*)ptr(P_LN_S); a.ln_b = (const float*)ptr(P_LN_B);
        a.w_up_sub = (const f16*)ptr(P_W_UP_SUB); a.splitk_ws = (float*)ptr(P_SPLITK_WS); a.splitk_ws_bytes = (size_t)v[16];
        g_error[0] = 0;
        IgemmPlan pl;
        const int rc = igemm_plan(a, t, &pl);
        const IgemmRoute& r = pl.route;
        const size_t ws = pl.uses_splitk_ws ? (size_t)r.splits * pl.M * a.N * sizeof(float) : 0;
        printf("%d %d %d %d %d %d %d %d %d %d %d %zu %zu | %s\n", rc, r.family, r.tile_cols, r.variant, r.splits, r.gn_done, r.row_groups, pl.slot, pl.grid_x, pl.grid_y, pl.block, pl.lds, ws, g_error);
    }
    return 0;
}
