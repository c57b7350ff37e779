// launch_igemm's decision as a pure host function: igemm_plan(args, knobs) validates the arguments, chooses the kernel family and instantiation and works out the
// launch geometry; launch_igemm (igemm.hip) fills the kernel parameters from the plan and launches.  Nothing here calls HIP, reads tune(), writes t_igemm_route or
// dereferences a pointer of IgemmArgs (pointers are only tested for null), so the whole routing can be asked on the host: tests/test_igemm_plan.py drives it from a
// stand-alone program, the sanitizer harness's launch_igemm stub (tests/sanitize/stubs.cpp) asks it for the layouts the real router picks.
#pragma once
#include "ops.h"

// ---- constants the decision shares with the kernels of igemm.hip ----------------------------------------------------------------------------------------------------
constexpr int BM = 128;             // igemm_kernel's row tile
constexpr int BK = 64;              // k step of every kernel: 64 halfs = one 128-byte LDS row
constexpr int HALO_ROWS_MAX = 400;  // conv3_halo_kernel / conv3_lw_kernel: halo rows of a tile that fit one halo buffer
constexpr size_t CONV_LDS_MAX = 2 * (HALO_ROWS_MAX * 128) + 3 * (160 * 128);      // two halo buffers + three 160-row weight buffers = 160 KiB exactly: the whole LDS of a CU
constexpr int AS_SLICE = 32 * 640, AS_RING = 3, AS_PATCH = 8192;
// gemm_as_kernel's dynamic LDS: the ring, eight patches, 512 x (rstd, mean rstd), the (b' | s) tables (or the bias)
inline size_t gemm_as_lds(int N) { return (size_t)AS_RING * AS_SLICE + 8 * AS_PATCH + 512 * 8 + (size_t)N * 8; }
constexpr int AS_MAX_N = (160 * 1024 - AS_RING * AS_SLICE - 8 * AS_PATCH - 512 * 8) / 8;      // = 4096
// extra dynamic LDS of the folded-LayerNorm consumer instantiations (ln_tile_prologue): 256 rows x 8 B + the (b' | s) tables
constexpr size_t LN_LDS_W8 = 256 * 8 + 2 * 2 * 160 * 4, LN_LDS_LW = 256 * 8 + 2 * 160 * 4;
constexpr size_t gemm_big_lds(int bn) { return 2 * (256 * BK * 2 + (size_t)bn * BK * 2); }       // two stages of a 256 x bn tile (gemm_big_kernel, gemm_w8_kernel)
constexpr size_t GEMM_LW_LDS = 3 * (256 * BK * 2 + 160 * BK * 2);                                  // gemm_lw_kernel: three 52 KB stages

// ---- kernel families (IgemmRoute::family) and the numbering of their instantiations (IgemmRoute::variant; the kernel tables of igemm.hip are in this order) ---------
enum IgemmFamily { FAM_NONE, FAM_IGEMM, FAM_HALO, FAM_CONV_LW, FAM_SUB, FAM_BIG, FAM_W8, FAM_GEMM_LW, FAM_AS };
// igemm_kernel<BN, CONV3, GEGLU, LNM, EPI>: variant = LNM | EPI << 2 | GEGLU << 4 | CONV3 << 5 (LNM 1 folded-LayerNorm consumer, 2 row-statistics producer; EPI 1 byte
// lo planes).  The forms that exist, GEGLU ones last: the 160-column tiles have the first IK_FORMS_160 (igemm_kernel's GEGLU form is the 128-column one).
enum IgemmKernelForm { IK_PLAIN, IK_LN, IK_STATS, IK_LO8, IK_LO8_STATS, IK_CONV3, IK_GEGLU, IK_GEGLU_LN, IK_FORMS, IK_FORMS_160 = IK_GEGLU };
constexpr int IK_VARIANT[IK_FORMS] = {0, 1, 2, 1 << 2, 2 | 1 << 2, 1 << 5, 1 << 4, 1 | 1 << 4};
inline int igemm_kernel_form(bool conv3, bool geglu, int lnm, bool lo8) {
    if (conv3) return IK_CONV3;
    if (geglu) return lnm == 1 ? IK_GEGLU_LN : IK_GEGLU;
    if (lo8) return lnm == 2 ? IK_LO8_STATS : IK_LO8;
    return lnm;                     // IK_PLAIN, IK_LN, IK_STATS
}
inline int igemm_kernel_slot(int bn, int form) { return bn == 128 ? form : IK_FORMS + form; }          // 128-column forms, then the 160-column ones
// conv3_halo_kernel<UP, BN, KH, SCHED>: variant = 1 with the fused upsample; the table holds the four tile widths, plain then upsample each
inline int halo_slot(int bn, bool up) { return 2 * (bn == 320 ? 0 : bn == 256 ? 1 : bn == 160 ? 2 : 3) + (up ? 1 : 0); }
// conv3_lw_kernel<UP, BN, TRACE, FAST>.  FAST: immediate-offset LDS addressing on 16 x 16 patches; FAST8: 8 x 8 images, four per tile; TRACE: the stamped instantiations
enum ConvLwVariant { LW_FAST160, LW_PLAIN160, LW_UP160, LW_TRACE_FAST160, LW_TRACE160, LW_UP_FAST160, LW_FAST128, LW_PLAIN128, LW_UP128, LW_UP_FAST128, LW_FAST8, LW_VARIANTS };
inline int conv_lw_variant(int bn, bool up, bool fast, bool fast8, bool trace) {
    if (fast8) return LW_FAST8;
    if (bn == 128) return up ? (fast ? LW_UP_FAST128 : LW_UP128) : (fast ? LW_FAST128 : LW_PLAIN128);
    if (trace) return fast ? LW_TRACE_FAST160 : LW_TRACE160;
    if (up) return fast ? LW_UP_FAST160 : LW_UP160;
    return fast ? LW_FAST160 : LW_PLAIN160;
}
// conv3_lw_kernel in the sub-pixel form: 16 x 16 input patches at 160 columns, 8 x 8 images at 160 columns, 16 x 16 patches at 128 columns
enum SubVariant { SUB_16_160, SUB_8_160, SUB_16_128, SUB_VARIANTS };
inline int sub_variant(int bn, bool p16) { return bn == 128 ? SUB_16_128 : p16 ? SUB_16_160 : SUB_8_160; }
// gemm_big_kernel<GEGLU, BNX>: variant = 1 with GEGLU (320 columns only); table: <false, 320>, <true, 320>, <false, 160>
inline int gemm_big_slot(int bn, bool geglu) { return bn == 160 ? 2 : geglu ? 1 : 0; }
// gemm_w8_kernel<GEGLU, LNM, EPI> (EPI 2: residual + its lo plane in, no lo plane out) and gemm_lw_kernel<LNM, EPI>
enum W8Variant { W8_PLAIN, W8_GEGLU, W8_LN, W8_GEGLU_LN, W8_STATS, W8_LO8, W8_LO8_STATS, W8_EPI2, W8_VARIANTS };
inline int w8_variant(bool geglu, int lnm, int epi) {
    if (epi == 1) return lnm == 2 ? W8_LO8_STATS : W8_LO8;
    if (epi == 2 && lnm == 0) return W8_EPI2;
    return lnm == 2 ? W8_STATS : 2 * lnm + (geglu ? 1 : 0);       // W8_PLAIN, W8_GEGLU, W8_LN, W8_GEGLU_LN
}
enum GemmLwVariant { GLW_PLAIN, GLW_LN, GLW_STATS, GLW_LO8, GLW_LO8_STATS, GLW_EPI2, GLW_VARIANTS };
inline int gemm_lw_variant(int lnm, int epi) {
    if (epi == 1) return lnm == 2 ? GLW_LO8_STATS : GLW_LO8;
    return epi == 2 && lnm == 0 ? GLW_EPI2 : lnm;               // GLW_PLAIN, GLW_LN, GLW_STATS
}
// gemm_as_kernel<GEGLU, LNM>: plain, GEGLU, folded LayerNorm, both
enum AsVariant { AS_PLAIN, AS_GEGLU, AS_LN, AS_GEGLU_LN, AS_VARIANTS };
inline int as_variant(bool geglu, int lnm) { return 2 * lnm + (geglu ? 1 : 0); }

struct IgemmPlan {          // (value-initialised by igemm_plan: everything a route does not set is 0)
    IgemmRoute route;       // family, tile_cols, variant, splits, gn_done, row_groups as the record will say (fallback is the launcher's: it tells what ran BEHIND the kernel)
    int slot;               // index into the family's kernel table: the variant, except for igemm_kernel_slot / halo_slot / gemm_big_slot
    int grid_x, grid_y, block; size_t lds;
    int M, tiles_n, nblk, gm, pn, KT, KTh, lo8;             // IgemmParams fields the route fixes
    // the kernels get gn_stats (statistics wanted, allowed and the knob on; whether they were left: route.gn_done) | splits > 1: fp32 partial sums through splitk_ws,
    // a reduce kernel behind the launch | the sub-pixel form reads w_up_sub instead of w
    bool gn_by_epilogue, uses_splitk_ws, uses_w_up_sub;
    int HALO_W, HALO_IMG, NHALO, NQ, tw_shift, trw_shift, PX, PP, sched;        // halo / loader-wave / sub-pixel geometry (HaloParams); zero for the GEMM families
};

// the split-K reduce also leaves the GroupNorm statistics (splitk_reduce_stats_kernel): statistics for the kernels, one 64-row slot per sample
inline bool splitk_reduce_leaves_stats(bool gn_stats, int HoWo, int M, int N, int debug) { return gn_stats && HoWo == 64 && M % 64 == 0 && N % 32 == 0 && !(debug & 64); }      // (debug bit 64: A/B against the statistics pass)

// tile_of's pn for a launch of tiles_m x tiles_n tiles that reads a_bytes of activations and w_bytes of weights once each algorithmically: per-XCD L2s mean the
// contiguous order fetches a + 8 w, an (8 / pn) x pn grid pn a + (8 / pn) w.  Switch only for a clear gain (the contiguous order has the banded walk, IgemmParams::gm).
inline int choose_xcd_grid(const TuneSet& t, int tiles_m, int tiles_n, double a_bytes, double w_bytes) {
    if (!t.xcd_grid) return 0;
    int best = 0; double best_cost = 0.85 * (a_bytes + 8.0 * w_bytes);
    for (int pn = 2; pn <= 8; pn *= 2) {
        const int px = 8 / pn;
        if (tiles_n % pn || tiles_m % px) continue;
        const double cost = pn * a_bytes + px * w_bytes;
        if (cost < best_cost) { best_cost = cost; best = pn; }
    }
    return best;
}

// what the validation derives from the arguments for the routes.  lnm: the epilogue instantiation, 1 folded-LayerNorm consumer, 2 row-statistics producer, 0 neither;
// epi: the epilogue family (igemm_epilogue_f32, EPI), 1 = byte lo planes, 2 = a residual with an fp16 lo plane and no lo plane out (FAST 4)
// want_320: the 256 x 320 tiles are the ones for this layer (a linear / 1x1 layer with N % 320 == 0 whose tiles fill the chip, or forced, or GEGLU with N % 128 != 0)
struct IgemmFacts { int cin, lnm, epi; bool conv3, split_a, stats_ok, as_ok, want_320; double a_bytes, w_bytes; };

// gemm_as_kernel (knob gemm_as): a K = 320 linear layer with a bias or folded-LayerNorm epilogue (GEGLU or not) and nothing else -- one A source, no lo plane, no
// time embedding / residual / lo plane out / statistics -- N a multiple of the 32-row weight slice that fits the LDS tables (which also keeps the weight buffer's
// 32-bit offsets in range), debug off.  The activation-size condition is gemm_w8_kernel's 32-bit-offset rule, kept so that the two routes cover the same shapes;
// this kernel itself reaches activations and outputs through 64-bit pointers.
// Auto: at least 192 512-row workgroups (the 64 x 64 level at batch >= 24; below that the 256 x 320 / 256 x 160 tiles have more workgroups to fill the chip with)
// and N >= 960 (QKV, the GEGLU projection): the N = 320 projections are at the HBM roof on gemm_w8_kernel and stay there.
inline bool as_eligible(const IgemmArgs& a, const TuneSet& t) {
    const long long m = (long long)a.B * a.Ho * a.Wo;
    return t.gemm_as != 0 && a.taps == 1 && a.c1 == 0 && a.c0 == 320 && !a.a0_lo && !a.temb && !a.res && !a.out_lo && !a.row_stats && !a.gn_stats &&
           a.N > 0 && a.N % 32 == 0 && a.N <= AS_MAX_N && !t.debug && (double)m * 640 < 4.0e9 && (t.gemm_as == 2 || ((m + 511) / 512 >= 192 && a.N >= 960));
}

// every refusal that does not depend on the route, in the order the error codes are pinned by, and the plan fields every route shares; *empty: nothing to launch
// (CS_OK, or CS_E_SHAPE for B < 0)
inline int igemm_validate(const IgemmArgs& a, const TuneSet& t, IgemmFacts* f, IgemmPlan* pl, bool* empty) {
    const int cin = a.c0 + a.c1;
    *empty = true;
    if (!a.a0 || !a.w || !a.out) CS_FAIL(CS_E_ARG, "igemm: a0, w, out required");
    if (a.taps != 1 && a.taps != 9) CS_FAIL(CS_E_ARG, "igemm: taps must be 1 or 9");
    if (cin % BK || a.c0 % BK || (a.c1 && !a.a1)) CS_FAIL(CS_E_SHAPE, "igemm: channels (%d,%d) must be multiples of %d", a.c0, a.c1, BK);
    if (a.B <= 0 || a.Ho <= 0 || a.Wo <= 0) return (a.B < 0) ? CS_E_SHAPE : CS_OK;
    *empty = false;
    if (a.taps == 1 && (a.stride != 1 || a.upsample || a.Hi != a.Ho || a.Wi != a.Wo)) CS_FAIL(CS_E_ARG, "igemm: 1x1 needs stride 1, no upsample");
    f->as_ok = as_eligible(a, t);
    if (!f->as_ok && a.geglu && (a.N % 256) && (a.N % 320)) CS_FAIL(CS_E_SHAPE, "igemm: GEGLU needs N %% 256 == 0 or N %% 320 == 0 (N=%d)", a.N);
    if (a.pad_after_only && !(a.taps == 9 && a.stride == 2)) CS_FAIL(CS_E_ARG, "igemm: pad_after_only is the stride-2 3x3 form");
    if (a.ln_stats) {
        if (a.taps != 1 || a.c1 || a.temb || a.res || a.out_lo || a.row_stats || a.gn_stats)
            CS_FAIL(CS_E_ARG, "igemm: a folded LayerNorm (ln_stats) is the epilogue of a plain linear layer (one source, no temb / residual / lo plane / statistics)");
        if (!a.ln_s || !a.ln_b || a.ln_groups < 1) CS_FAIL(CS_E_ARG, "igemm: ln_stats needs ln_s, ln_b and ln_groups >= 1");
    }
    if (a.row_stats && (a.geglu || a.gn_stats)) CS_FAIL(CS_E_ARG, "igemm: row_stats excludes GEGLU and gn_stats");
    if (a.row_stats && !a.row_stats_groups) CS_FAIL(CS_E_ARG, "igemm: row_stats needs row_stats_groups (the layout the chosen kernel wrote is returned there)");
    f->split_a = a.a0_lo != nullptr;
    if (f->split_a) {
        if (a.taps != 1 || a.geglu) CS_FAIL(CS_E_ARG, "igemm: a split-fp16 A operand (a0_lo) is built for 1x1 / linear layers without GEGLU");
        if (a.c1 && !a.a1_lo) CS_FAIL(CS_E_ARG, "igemm: a0_lo without a1_lo");
    }
    if (a.geglu && a.out_lo) CS_FAIL(CS_E_ARG, "igemm: the GEGLU epilogue writes no lo plane");
    const bool res_lo = a.res && a.res_lo;
    pl->lo8 = (a.lo8 && (res_lo || a.out_lo)) ? 1 : 0;
    if (pl->lo8 && (a.taps != 1 || a.temb || a.geglu || a.ln_stats)) CS_FAIL(CS_E_ARG, "igemm: 8-bit lo planes (lo8) are built for plain 1x1 / linear layers (the transformer hidden state)");
    f->cin = cin; f->conv3 = a.taps == 9; pl->M = a.B * a.Ho * a.Wo; pl->gm = 1;
    pl->KTh = a.taps * (cin / BK); pl->KT = f->split_a ? 2 * pl->KTh : pl->KTh;        // split A: the lo k steps re-read the same weight columns (Ktot, the row length of w, stays)
    f->lnm = a.ln_stats ? 1 : (a.row_stats && !f->conv3 ? 2 : 0);
    f->epi = (a.taps == 1 && !a.geglu && !a.ln_stats && !a.temb) ? (pl->lo8 ? 1 : (res_lo && !a.out_lo && (t.epi_fast & 2)) ? 2 : 0) : 0;
    // GroupNorm statistics of the output: by the epilogue where the chosen kernel runs one (not the split-K forms), else by the launcher's statistics pass
    pl->gn_by_epilogue = f->stats_ok = a.gn_stats && !a.geglu && (a.Ho * a.Wo) % 64 == 0 && t.gn_fuse != 0;
    f->a_bytes = 2.0 * a.B * a.Hi * a.Wi * cin; f->w_bytes = 2.0 * a.N * a.taps * cin;
    f->want_320 = t.biggemm && !f->conv3 && a.N % 320 == 0 && ((pl->M + 255) / 256 * (a.N / 320) >= 192 || t.biggemm == 2 || (a.geglu && a.N % 128));
    if (f->as_ok) return CS_OK;
    if (a.N % 128 && a.N % 160) CS_FAIL(CS_E_SHAPE, "igemm: N=%d must be a multiple of 128 or 160", a.N);
    if (a.geglu && f->conv3) CS_FAIL(CS_E_ARG, "igemm: GEGLU epilogue only for linear layers");
    return CS_OK;
}

// ---- the routes, in the order they are tried.  One that declines returns false and leaves the plan untouched ---------------------------------------------------------
inline void plan_launch(IgemmPlan* pl, int family, int tile_cols, int variant, int slot, int grid_x, int grid_y, int block, size_t lds) {
    pl->route.family = family; pl->route.tile_cols = tile_cols; pl->route.variant = variant; pl->route.splits = grid_y; pl->slot = slot;
    pl->grid_x = grid_x; pl->grid_y = grid_y; pl->block = block; pl->lds = lds;
}
inline void plan_halo(IgemmPlan* pl, int halo_w, int halo_h, int ipt, int tw_shift, int trw_shift, int PX, int PP) {
    pl->HALO_W = halo_w; pl->HALO_IMG = halo_h * halo_w; pl->NHALO = ipt * pl->HALO_IMG; pl->NQ = (pl->NHALO + 7) / 8;
    pl->tw_shift = tw_shift; pl->trw_shift = trw_shift; pl->PX = PX; pl->PP = PP;
}

inline bool as_route(const IgemmArgs& a, const IgemmFacts& f, IgemmPlan* pl) {
    if (!f.as_ok) return false;
    const int v = as_variant(a.geglu, f.lnm);
    plan_launch(pl, FAM_AS, 32, v, v, (pl->M + 511) / 512, 1, 512, gemm_as_lds(a.N));
    return true;
}

// nearest-x2 upsample + 3x3 conv in the sub-pixel form (conv3_lw_kernel<.., SUB>): tiles over INPUT pixels, four phases, 4 of 9 taps each with the filter's taps
// pre-summed (a.w_up_sub from conv_up_fold_pack_host: one more fp16 rounding of the weights, which is why the caller decides -- knob up_fold)
inline bool sub_pixel(const IgemmArgs& a, const TuneSet& t, const IgemmFacts& f, IgemmPlan* pl) {
    if (!igemm_sub_pixel(a, t)) return false;
    const int bn = a.N % 160 == 0 ? 160 : 128;                          // (the VAE decoder's 256 / 512-wide upsamplers: 128-column tiles)
    const bool p16 = a.Wi % 16 == 0 && a.Hi % 16 == 0;                   // (else 8 x 8)
    const int TW = p16 ? 16 : 8, TRW = p16 ? 256 : 64, IPT = 256 / TRW, PX = a.Wi / TW, PP = PX * (a.Hi / TW);
    const int tiles_m = 4 * (PP == 1 ? (a.B + IPT - 1) / IPT : a.B * PP), tiles_n = a.N / bn, v = sub_variant(bn, p16);
    plan_halo(pl, TW + 2, TW + 2, IPT, p16 ? 4 : 3, p16 ? 8 : 6, PX, PP);
    plan_launch(pl, FAM_SUB, bn, v, v, tiles_m * tiles_n, 1, 512, 2 * ((size_t)pl->NQ * 1024) + 3 * ((size_t)bn * 128));
    pl->tiles_n = tiles_n; pl->nblk = tiles_m * tiles_n; pl->pn = choose_xcd_grid(t, tiles_m, tiles_n, f.a_bytes, f.w_bytes * 16.0 / 9.0);
    pl->uses_w_up_sub = true; pl->route.gn_done = f.stats_ok;            // (row statistics of a conv output: the launcher's pass)
    return true;
}

// stride-1 3x3 convs on halo tiles: a patch of TW = min(Wo, 16) x TH = min(Ho, 256 / TW) output pixels per image (both powers of two dividing the image), 256 / (TW TH)
// images per tile.  conv3_lw_kernel (loader waves, 256 pixels x 160 | 128 channels per workgroup) wherever the channel count allows it, else conv3_halo_kernel: 256 x
// 320 | 256 tiles with the k32 inner step when they still fill the chip (SD1.5's 320- and 640-wide layers at 64 x 64 / 32 x 32, the VAE's 256 / 512 channels; knob
// conv_halo 3 forces, 4 forbids: tests / A-B), else 160 | 128 columns.  Small images split the channel chunks to fill the chip.
inline bool halo_or_lw(const IgemmArgs& a, const TuneSet& t, const IgemmFacts& f, IgemmPlan* pl) {
    const int Wo = a.upsample ? 2 * a.Wi : a.Wi, Ho = a.upsample ? 2 * a.Hi : a.Hi;
    const int TW = Wo >= 16 ? 16 : Wo, THmax = TW ? 256 / TW : 0, TH = Ho < THmax ? Ho : THmax;
    const bool geom_ok = (TW == 8 || TW == 16) && TH >= 2 && (TH & (TH - 1)) == 0 && Wo % TW == 0 && Ho % TH == 0 && Ho == a.Ho && Wo == a.Wo &&
                         (!a.upsample || (TH % 2 == 0 && TW % 2 == 0 && TW / 2 + 2 >= 10));
    if (!(t.halo && f.conv3 && a.stride == 1 && a.c1 == 0 && !a.geglu && geom_ok)) return false;
    const int TRW = TH * TW, IPT = 256 / TRW, PX = Wo / TW, PP = PX * (Ho / TH), NC = f.cin / BK;
    const int tiles_m = PP == 1 ? (a.B + IPT - 1) / IPT : a.B * PP;
    // (conv3_lw_kernel's padded halo rows read g_zero_region + chunk offset: the region covers LW_ZERO_CHUNKS 64-channel chunks, wider inputs take the halo kernels)
    const bool lw_cin_ok = NC <= LW_ZERO_CHUNKS, lw160 = t.conv_lw != 0 && a.N % 160 == 0 && lw_cin_ok;
    const bool lw = lw160 || (t.conv_lw != 0 && t.conv_lw != 3 && a.N % 128 == 0 && lw_cin_ok);             // the VAE's widths 128 / 256 / 512 (conv_lw = 3: BN 160 only)
    int bn = a.N % 160 == 0 ? 160 : 128;
    bool wide = false;
    if (lw) bn = lw160 ? 160 : 128;
    else if (a.N % 320 == 0 && t.halo != 4 && (tiles_m * (a.N / 320) >= 192 || t.halo == 3)) { bn = 320; wide = true; }
    else if (a.N % 256 == 0 && t.halo != 4 && (tiles_m * (a.N / 256) >= 192 || t.halo == 3)) { bn = 256; wide = true; }
    const int tiles_n = a.N / bn;
    int splits = 1;
    if (tiles_m * tiles_n < 160 && a.splitk_ws)
        while (splits < 8 && tiles_m * tiles_n * splits < 192 && NC % (splits * 2) == 0 && (size_t)(splits * 2) * pl->M * a.N * sizeof(float) <= a.splitk_ws_bytes) splits *= 2;
    const int tin_w = a.upsample ? TW / 2 : TW, tin_h = a.upsample ? TH / 2 : TH, nhalo = IPT * (tin_h + 2) * (tin_w + 2), nq = (nhalo + 7) / 8;
    const bool pays = tiles_m * tiles_n * splits >= 160;
    if (!((pays || t.halo == 2 || t.halo == 3) && nhalo <= HALO_ROWS_MAX && nq <= 64 && (PP == 1 || IPT == 1))) return false;
    int trw_shift = 0; while ((1 << trw_shift) < TRW) ++trw_shift;
    plan_halo(pl, tin_w + 2, tin_h + 2, IPT, TW == 16 ? 4 : 3, trw_shift, PX, PP);
    if (lw) {
        // FAST: plain conv on 16 x 16 patches (every UNet level down to 16 x 16, the VAE): immediate-offset LDS addressing
        const bool trace = (t.debug & 16384) != 0;      // timing experiments: the stamped instantiations (plain conv only)
        const bool fast = TW == 16 && TH == 16 && t.conv_lw != 2 && (a.upsample ? (pl->HALO_W == 10 && nq == 13) : (pl->HALO_W == 18 && nq == 41));
        const bool fast8 = bn == 160 && TW == 8 && TH == 8 && !a.upsample && IPT == 4 && PP == 1 && pl->HALO_W == 10 && nq == 50 && t.conv_lw != 2 && !trace;
        const int v = conv_lw_variant(bn, a.upsample != 0, fast, fast8, trace && !a.upsample);
        plan_launch(pl, FAM_CONV_LW, bn, v, v, tiles_m * tiles_n, splits, 512, 2 * ((size_t)nq * 1024) + 3 * ((size_t)bn * 128));
    } else {
        // the k32-step kernels (BN 320 / 256) run schedule 2 (priority + interleaved DMA for the staggered group: -6 ... -11 %, profiles/r02_ab_conv_sched.txt), the
        // k64-step kernels (BN 160 / 128: 16 x 16 and 8 x 8 images) the lock-step schedule 0 (schedule 2 cost them 3 %: 0.207 -> 0.213 ms)
        pl->sched = wide ? 2 : 0;
        plan_launch(pl, FAM_HALO, bn, a.upsample ? 1 : 0, halo_slot(bn, a.upsample != 0), tiles_m * tiles_n, splits, 512, 2 * (HALO_ROWS_MAX * 128) + 3 * ((size_t)bn * (wide ? 64 : 128)));
    }
    pl->tiles_n = tiles_n; pl->nblk = tiles_m * tiles_n; pl->pn = choose_xcd_grid(t, tiles_m, tiles_n, f.a_bytes, f.w_bytes);
    pl->uses_splitk_ws = splits > 1;
    pl->route.gn_done = f.stats_ok && (splits == 1 || splitk_reduce_leaves_stats(true, a.Ho * a.Wo, pl->M, a.N, t.debug));       // (row statistics of a conv output: the launcher's pass)
    return true;
}

// the 256-row tiles of the linear / 1x1 layers (8 waves; knob gemm_big: 0 never, 1 when the tile count fills the chip, 2 / 3 force the 320 / 160-wide form)
inline void plan_tiles_256(const IgemmArgs& a, const TuneSet& t, const IgemmFacts& f, int bn, int row_group_cols, IgemmPlan* pl) {
    const int tiles_m = (pl->M + 255) / 256, tn = a.N / bn;
    pl->tiles_n = tn; pl->nblk = tiles_m * tn; pl->pn = choose_xcd_grid(t, tiles_m, tn, f.a_bytes, f.w_bytes);
    pl->gm = t.gemm_gm >= 0 ? (t.gemm_gm > 1 ? t.gemm_gm : 1) : (tn >= 12 ? 4 : 1);
    pl->route.gn_done = f.stats_ok; pl->route.row_groups = a.row_stats ? a.N / row_group_cols : 0;
}
// 256 x 320: gemm_w8_kernel (the hand-scheduled k loop) whenever 32-bit byte offsets reach every operand row, else gemm_big_kernel<., 320> -- which has no lo-plane
// staging, no LayerNorm epilogues and no byte planes: those forms decline.  GEGLU with N % 128 != 0 (320, 960, ...) runs here whatever the tile count: the generic
// tiles cannot take it (igemm_kernel's GEGLU form is the 128-column one).
inline bool tiles_256x320(const IgemmArgs& a, const TuneSet& t, const IgemmFacts& f, IgemmPlan* pl) {
    if (!f.want_320) return false;
    const int nblk = (pl->M + 255) / 256 * (a.N / 320);
    const bool off32 = (double)pl->M * (a.c0 > a.c1 ? a.c0 : a.c1) * 2 < 4.0e9 && (double)a.N * a.taps * f.cin * 2 < 4.0e9, w8 = t.gemm_w8 && off32 && !t.debug;
    if (!w8 && (f.split_a || f.lnm || f.epi == 1)) return false;
    const int v = w8 ? w8_variant(a.geglu != 0, f.lnm, f.epi) : (a.geglu ? 1 : 0);
    plan_launch(pl, w8 ? FAM_W8 : FAM_BIG, 320, v, w8 ? v : gemm_big_slot(320, a.geglu != 0), nblk, 1, 512, gemm_big_lds(320) + (w8 ? LN_LDS_W8 : 0));
    plan_tiles_256(a, t, f, 320, 160, pl);              // gemm_w8 / gemm_big<., 320>: 64 x 160 wave tiles
    return true;
}
// too few 256 x 320 tiles: 256 x 160, gemm_lw_kernel (loader waves) or gemm_big_kernel<false, 160> (plain epilogues only).  A form the 320-wide kernels were
// wanted for and declined goes to the generic tiles, not here.
inline bool tiles_256x160(const IgemmArgs& a, const TuneSet& t, const IgemmFacts& f, IgemmPlan* pl) {
    if (!(t.biggemm && !f.conv3 && !a.geglu && a.N % 160 == 0) || f.want_320) return false;
    const int nblk = (pl->M + 255) / 256 * (a.N / 160);
    if (!(nblk >= 192 || t.biggemm == 3)) return false;
    const bool lw = t.gemm_lw && !t.debug;
    if (!lw && (f.split_a || f.lnm || f.epi == 1)) return false;
    const int v = lw ? gemm_lw_variant(f.lnm, f.epi) : 0;
    plan_launch(pl, lw ? FAM_GEMM_LW : FAM_BIG, 160, v, lw ? v : gemm_big_slot(160, false), nblk, 1, 512, lw ? GEMM_LW_LDS + LN_LDS_LW : gemm_big_lds(160));
    plan_tiles_256(a, t, f, 160, lw ? 160 : 80, pl);    // gemm_lw: 64 x 160 wave tiles; gemm_big<., 160>: 64 x 80
    return true;
}

// igemm_kernel, 128 x 128 | 160 tiles: takes everything the others declined, except GEGLU with N % 128 != 0
inline int generic_tiles(const IgemmArgs& a, const TuneSet& t, const IgemmFacts& f, IgemmPlan* pl) {
    // the GEGLU form of igemm_kernel is the 128-column one: with N % 128 != 0 (160-column tiles) it would leave the columns behind 128 tiles_n unwritten
    if (a.geglu && a.N % 128) CS_FAIL(CS_E_SHAPE, "igemm: GEGLU with N %% 128 != 0 (N=%d) needs the 256 x 320 tiles (knob gemm_big != 0)", a.N);
    const int bn = a.N % 128 == 0 ? 128 : 160, tiles_m = (pl->M + BM - 1) / BM, tiles_n = a.N / bn, nblk = tiles_m * tiles_n;
    // few tiles and a long k loop (stride-2 convs into the 16 x 16 / 8 x 8 levels, the 8 x 8 linears): split K to fill the chip
    int splits = 1;
    if (a.splitk_ws && !a.geglu && nblk < 192)
        while (splits < 8 && nblk * splits < 256 && pl->KT % (splits * 2) == 0 && pl->KT / (splits * 2) >= 8 && (size_t)(splits * 2) * pl->M * a.N * sizeof(float) <= a.splitk_ws_bytes) splits *= 2;
    // (split-K: raw partial sums leave the main kernel; the reduce kernel applies a folded LayerNorm and the byte planes itself and leaves no row statistics)
    const int form = igemm_kernel_form(f.conv3, a.geglu != 0, splits > 1 ? 0 : f.lnm, f.epi == 1 && splits == 1);
    plan_launch(pl, FAM_IGEMM, bn, IK_VARIANT[form], igemm_kernel_slot(bn, form), nblk, splits, 256, 2 * (BM * BK * 2 + (size_t)bn * BK * 2));
    pl->tiles_n = tiles_n; pl->nblk = nblk; pl->pn = choose_xcd_grid(t, tiles_m, tiles_n, f.a_bytes, f.w_bytes);
    pl->uses_splitk_ws = splits > 1;
    pl->route.gn_done = f.stats_ok && (splits == 1 || splitk_reduce_leaves_stats(true, a.Ho * a.Wo, pl->M, a.N, t.debug));
    pl->route.row_groups = (a.row_stats && splits == 1 && !f.conv3) ? a.N / (bn / 2) : 0;              // 64 x bn / 2 wave tiles
    return CS_OK;
}

// CS_OK with the plan filled (route.family 0: an empty shape, nothing to launch), or the error code with the error text set
inline int igemm_plan(const IgemmArgs& a, const TuneSet& t, IgemmPlan* pl) {
    *pl = IgemmPlan();
    IgemmFacts f;
    bool empty;
    const int rc = igemm_validate(a, t, &f, pl, &empty);
    if (rc != CS_OK || empty) return rc;
    if (as_route(a, f, pl) || sub_pixel(a, t, f, pl) || halo_or_lw(a, t, f, pl) || tiles_256x320(a, t, f, pl) || tiles_256x160(a, t, f, pl)) return CS_OK;
    return generic_tiles(a, t, f, pl);
}
