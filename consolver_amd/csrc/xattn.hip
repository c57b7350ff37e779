// Fused cross-attention sub-block of the SD1.5 transformer block at C = 320 (8 heads x 40), the 64 x 64 level:
//
//     h_out = h + to_out( softmax(scale * to_q(LayerNorm2(h)) K^T) V ) + b_out        (K, V: the cached projections of the <= 80 text keys)
//
// replaces four kernels of the unfused executor (ln_kernel, gemm_big to_q, attn_kernel with 77 keys, gemm_big to_out + residual) whose
// only job besides ~54 MFLOP per 128 rows is to move three [M, 320] intermediates through HBM (LayerNorm output, q, attention output:
// 6 x 84 MB per block at batch 32).  Here a workgroup owns a tile of token rows (one wave per 16 of them) and keeps all three in LDS:
//
//   phase 0  rows -> registers -> LayerNorm (fp32 statistics, two-pass variance) -> fp16 tile XT in LDS, in the k-block layout the
//            GEMM fragment reads want: [5 blocks of 64 columns][tile rows][128 B], 16-byte chunk index XOR (row >> 1) & 7;
//   phase 1  q = XT Wq^T : Wq streamed by LDS-DMA through two weight stages (the first one issued before phase 0), wave tile 64 x 80;
//            accumulators -> fp16 (rounded as stored q, then pre-scaled by scale * log2 e and rounded again, the unfused kernels' two
//            rounding points) -> written over XT;
//   phase 2  the V rows of the sample, fetched into registers earlier, -> LDS (the weight stages, free between the GEMMs); rows >= Nk and
//            the pad chunks zero.  (K stays in global / L2: a key row's 8 consecutive channels are one 16-byte load in MFMA A layout);
//   phase 3  each wave takes 16 query rows and loops over the 8 heads: S^T = K Q^T (10 MFMAs), masked softmax over <= 80 keys in
//            registers, O^T = V^T P^T (9 MFMAs, V^T through the transposing LDS read), normalised O -> fp16 -> written over the
//            head's q columns of XT (dead by then);
//   phase 3' K fragments of the NEXT head are loaded while the current head computes;
//   phase 4  out = XT Wo^T as phase 1, + bias -> fp16 -> LDS patch -> + residual (h re-read, L2-hot) -> fp16 -> 640-byte row stores.
//
// The phases are the functions below (ln_rows, gemm_320, store_q, load_v / store_v, attn_head, epilogue), shared by two kernels:
//
//                      xattn_block_kernel (knob xattn_tile = 128)          xattn64_kernel (xattn_tile = 64, the default)
//   tile rows / waves  128 / 8 as 2 (rows) x 4 (columns)                   64 / 4 as 1 x 4
//   LDS                160 KB, one workgroup per CU                        80 KB, two workgroups per CU
//     XT               80 KB                                               40 KB
//     weight stages    2 x 40 KB                                           2 x 20 KB
//     epilogue patch   XT + the first 2 KB of stage 0                      XT + the first KB of stage 0
//     row statistics   stage 1                                             stage 1
//   weight stage       k64: [320 rows][128 B], chunk XOR (row >> 1) & 7    k32: [320 rows][64 B], chunk XOR (row >> 2) & 3
//   V tile             all 8 heads at once, [96 keys][672 B]               two halves of 4 heads, [96 keys][352 B] each
//   V loads issued     before the LayerNorm's row loads                    after the LayerNorm (earlier spilled), half 1 under half 0's heads
//
// With 160 KB a CU runs its four 128-row tiles strictly one after another and inside a tile every phase is exposed: all eight waves load rows, then
// all normalise, then all multiply, then all sit in the attention phase's dependent chains, then all store (profiles/r04_xattn_ablation.txt: 232 us
// per launch against a memory floor of 76 us and ~70 us of matrix work).  Two 64-row workgroups share a CU and drift apart, so one's loads / stores
// run under the other's MFMA and softmax phases.  The per-wave work is the same in both, which is why it is written once.
// The arithmetic class (fp16 storage points, fp32 accumulation) is the unfused path's; the softmax here subtracts the true row maximum
// (the unfused kernel's max-free steady state is for thousands of keys).
#include "ops.h"


namespace {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
__device__ __forceinline__ void glds16(const void* src, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_wave_base, 16, 0, 0);
}
typedef __fp16 hf4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) hf4* lds_hf4_ptr;
__device__ __forceinline__ u32x2 tr_read(const char* lds_addr) {
    hf4 r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_hf4_ptr)lds_addr);
    union { hf4 a; u32x2 b; } u; u.a = r;
    return u.b;
}
__device__ __forceinline__ unsigned pk(float a, float b) { union { f16x2 v; unsigned u; } x; x.v = f16x2{(f16)a, (f16)b}; return x.u; }
__device__ __forceinline__ f16x8 frag_of(u32x4 v) { union { u32x4 u; f16x8 f; } x; x.u = v; return x.f; }

struct XattnParams {
    const f16* h;        // [M_in rows][320] block input (residual stream)
    f16* out;            // [M rows][320]; may alias h
    const f16* h_lo; f16* out_lo;   // SPLIT: lo planes of the split-fp16 residual stream (XattnArgs::h_lo / out_lo)
    float* row_stats;    // optional [M][2]: (sum, sum of squares) of every output row (XattnArgs::row_stats)
    const f16* ln_g; const f16* ln_b; float ln_eps;
    const f16* wq;       // [320][320]
    const f16* wo; const f16* bo;
    const f16* kv;       // [B][Nk][640]: k = cols 0..319, v = cols 320..639
    int M, HW, Nk;       // rows of this launch, rows per sample, keys (<= 80)
    float c;             // scale * log2(e)
    int debug;           // xattn_block_kernel only, timing experiments (results wrong): bit 0 skip the attention phase, 1 skip the to_out GEMM, 2 skip the to_q GEMM,
                         // 3 skip the LayerNorm phase's loads, 4 skip the epilogue's residual loads and stores
};

constexpr int C = 320, DH = 40, NH = 8;
constexpr int VROWS = 96;                         // key rows of a V tile incl. zero padding
constexpr int PROW = 656;                         // epilogue patch row stride (bytes)
// the geometry of a TM-row tile (TM = 128 or 64; the table in the header)
template <int TM> constexpr int THREADS = 4 * TM;                  // one wave per 16 rows
template <int TM> constexpr int XT_BYTES = 5 * TM * 128;           // 81920 / 40960
template <int TM> constexpr int KSTAGE = TM == 128 ? 64 : 32;      // k columns of a weight stage
template <int TM> constexpr int WST = C * KSTAGE<TM> * 2;          // 40960 / 20480 per weight stage
template <int TM> constexpr int LDS_BYTES = XT_BYTES<TM> + 2 * WST<TM>;   // 163840 / 81920
template <int HEADS> constexpr int VCH = 5 * HEADS + 2;            // 16-byte chunks of a V tile row: the heads' data + 2 zero chunks ...
template <int HEADS> constexpr int VS = 16 * VCH<HEADS>;           // ... which make the row stride an odd multiple of 32 B: 672 (8 heads) / 352 (4 heads)

template <int TM>
__device__ __forceinline__ int xt_addr(int row, int col) {      // byte address of element (row, col) in XT (col multiple of 4 for 8-byte access)
    return (col >> 6) * (TM * 128) + row * 128 + ((((col & 63) >> 3) ^ ((row >> 1) & 7)) << 4) + ((col & 7) << 1);
}

// max / sum over the lanes {l, l ^ 16, l ^ 32, l ^ 48} with the gfx950 permlane swaps (pure VALU, no LDS round trip)
__device__ __forceinline__ float group_max(float v) {
    unsigned u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    u = __float_as_uint(v);
    r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float group_sum(float v) {
    unsigned u = __float_as_uint(v);
    auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    u = __float_as_uint(v);
    r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---------------- phase 0: LayerNorm of the wave's 16 rows (tile rows 16 w ..) -> XT.  DBG: the debug bits are compiled in ------------------
// (p by value here and in the epilogue: with a reference the kernels spilled more scalars, 254 v_readlane in xattn64_kernel against 112)
template <int TM, bool DBG>
__device__ __forceinline__ void ln_rows(const XattnParams p, char* XT, int w, int lane, int m_blk) {
    const bool act = lane < 40;                  // 40 chunks of 8 channels per row
    f16x8 raw[16];                                // all 16 rows of the wave in flight at once: one memory round trip
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int m = m_blk + 16 * w + u;
        raw[u] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (act && m < p.M && !(DBG && (p.debug & 8))) raw[u] = *reinterpret_cast<const f16x8*>(p.h + (size_t)m * C + lane * 8);
    }
    float gam[8], bet[8];
    if (act) {
        const f16x8 gv = *reinterpret_cast<const f16x8*>(p.ln_g + lane * 8), bv = *reinterpret_cast<const f16x8*>(p.ln_b + lane * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) { gam[k] = (float)gv[k]; bet[k] = (float)bv[k]; }
    }
    // the 16 rows' reductions run as 16 independent butterflies (a row-at-a-time loop serialised 16 x 2 x 6 dependent cross-lane steps)
    float mean[16], rstd[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (float)raw[u][k];
        mean[u] = s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int u = 0; u < 16; ++u) mean[u] += __shfl_xor(mean[u], o, 64);
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        mean[u] *= (1.0f / C);
        float q = 0.f;
        if (act) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float d = (float)raw[u][k] - mean[u]; q += d * d; }
        }
        rstd[u] = q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int u = 0; u < 16; ++u) rstd[u] += __shfl_xor(rstd[u], o, 64);
    if (act) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const float rs = rsqrtf(rstd[u] * (1.0f / C) + p.ln_eps);
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o[k] = pk(((float)raw[u][2 * k] - mean[u]) * rs * gam[2 * k] + bet[2 * k],
                          ((float)raw[u][2 * k + 1] - mean[u]) * rs * gam[2 * k + 1] + bet[2 * k + 1]);
            *reinterpret_cast<u32x4*>(XT + xt_addr<TM>(16 * w + u, lane * 8)) = o;
        }
    }
}

// ---------------- phases 1 and 4: the out-tile GEMM ------------------------------------------------------------------------------------
// acc[i][j] (n-tile i of the wave's 80 columns from col0, m-tile j of its 64 rows from row0) = XT(rows) . W^T, K = 320, in steps of one weight stage:
// the [320 rows][KSTAGE k] weight slab of a step is staged by LDS-DMA into one of two stages, one barrier per step.  (Weights straight from global into
// registers - no stage, no barrier - were measured too: 49 us per GEMM against 20 us staged; a lane group's 16-byte pieces of 16 different rows make
// poor vector-memory requests.)
// One template for both stage sizes: a stage row is CH = KSTAGE / 8 chunks of 16 bytes (8 at k64, 4 at k32), a 1 KB DMA piece 64 / CH rows of it (8 / 16),
// the chunk index is XORed with (row >> SH) & (CH - 1), SH = 1 / 2 (conflict-free ds_read_b128 fragments either way), and the waves take 5 pieces each.
// Written as two functions the loops differed in exactly these constants and in whether a stage holds one or two k32 steps, so the constants are named
// here once and the addressing below is spelled in them.
template <int TM> constexpr int W_CH = KSTAGE<TM> / 8;
template <int TM> constexpr int W_SH = TM == 128 ? 1 : 2;
// wave wv's j-th piece is number wv + (TM / 16) j; lane -> (row lane / CH of the piece, LDS chunk lane % CH), source chunk = LDS chunk ^ the row's swizzle.
// (The source pointer keeps a function of its own, with the piece number spelled out at both uses: the same arithmetic with the piece number in a
// variable shared by row and LDS offset compiled xattn_block_kernel to 100 bytes of scratch per lane against 52.)
template <int TM>
__device__ __forceinline__ const f16* w_piece_src(const f16* __restrict__ w, int wv, int lane, int j) {
    constexpr int CH = W_CH<TM>;
    const int r = (64 / CH) * (wv + (TM / 16) * j) + lane / CH;
    return w + (size_t)r * C + ((lane % CH) ^ ((r >> W_SH<TM>) & (CH - 1))) * 8;
}
template <int TM>
__device__ __forceinline__ void stage_w(const f16* __restrict__ w, char* WS, int wv, int lane, int kt, int buf) {
#pragma unroll
    for (int j = 0; j < 5; ++j) glds16(w_piece_src<TM>(w, wv, lane, j) + kt * KSTAGE<TM>, WS + buf * WST<TM> + (wv + (TM / 16) * j) * 1024);
}
template <int TM, bool PRESTAGED>
__device__ __forceinline__ void gemm_320(const f16* __restrict__ w, char* smem, int wv, int lane, int row0, int col0, f32x4 (&acc)[5][4]) {
    constexpr int CH = W_CH<TM>, ROWB = 16 * CH, KS = KSTAGE<TM> / 32, NST = C / KSTAGE<TM>;    // k32 MFMA steps per stage, stages per GEMM
    char* const XT = smem;
    char* const WS = smem + XT_BYTES<TM>;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int swz = (lane >> 1) & 7;                            // XT fragment: row i16 of a 16-row m-tile, chunk ^ (row >> 1) & 7
    const int wswz = (lane >> W_SH<TM>) & (CH - 1);             // weight fragment: row i16 of a 16-row n-tile, chunk ^ (row >> SH) & (CH - 1)
    if (!PRESTAGED) stage_w<TM>(w, WS, wv, lane, 0, 0);        // (PRESTAGED: the caller issued stage 0 before its own work)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < NST; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < NST) stage_w<TM>(w, WS, wv, lane, kt + 1, buf ^ 1);
        const char* tb = WS + buf * WST<TM> + col0 * ROWB;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k32 = kt * KS + ks;                       // XT's k-block (64 columns) k32 >> 1, its half k32 & 1
            const char* ta = XT + (k32 >> 1) * (TM * 128) + row0 * 128;
            const int fo = (lane & 15) * 128 + ((((k32 & 1) * 4 + (lane >> 4)) ^ swz) << 4);
            const int wfo = (lane & 15) * ROWB + (((ks * 4 + (lane >> 4)) ^ wswz) << 4);
            f16x8 fa[4], fw[5];
#pragma unroll
            for (int j = 0; j < 4; ++j) fa[j] = *reinterpret_cast<const f16x8*>(ta + j * 2048 + fo);
#pragma unroll
            for (int i = 0; i < 5; ++i) fw[i] = *reinterpret_cast<const f16x8*>(tb + i * (16 * ROWB) + wfo);
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fw[i], fa[j], acc[i][j], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

// the to_q accumulators -> fp16 -> pre-scaled -> over XT
template <int TM>
__device__ __forceinline__ void store_q(char* XT, const f32x4 (&acc)[5][4], float c, int row0, int col0, int g, int i16) {
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = col0 + i * 16 + 4 * g, m = row0 + j * 16 + i16;
            float qv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) qv[r] = (float)(f16)acc[i][j][r] * c;      // q as the unfused path stores it, then scaled
            *reinterpret_cast<u32x2*>(XT + xt_addr<TM>(m, n)) = u32x2{pk(qv[0], qv[1]), pk(qv[2], qv[3])};
        }
}

// ---------------- phase 2: a V tile of HEADS heads, [96 key rows][VCH chunks], through the workgroup's registers ------------------------
// vsrc: the first of the heads' V columns in key row 0 of the sample.  Loads and LDS writes are apart: the tile lives in the weight stages.
template <int NT, int HEADS> constexpr int V_PER_THREAD = (VROWS * VCH<HEADS> + NT - 1) / NT;      // 8 (512 threads, 8 heads) / 9 (256 threads, 4 heads)
template <int NT, int HEADS>
__device__ __forceinline__ void load_v(const f16* vsrc, int Nk, int tid, u32x4 (&vt)[V_PER_THREAD<NT, HEADS>]) {
#pragma unroll
    for (int k = 0; k < V_PER_THREAD<NT, HEADS>; ++k) {
        const int id = tid + NT * k, row = id / VCH<HEADS>, ch = id - row * VCH<HEADS>;
        vt[k] = u32x4{0, 0, 0, 0};
        if (id < VROWS * VCH<HEADS> && row < Nk && ch < 5 * HEADS) vt[k] = *reinterpret_cast<const u32x4*>(vsrc + (size_t)row * (2 * C) + ch * 8);
    }
}
template <int NT, int HEADS>
__device__ __forceinline__ void store_v(char* VT, int tid, const u32x4 (&vt)[V_PER_THREAD<NT, HEADS>]) {
#pragma unroll
    for (int k = 0; k < V_PER_THREAD<NT, HEADS>; ++k) {
        const int id = tid + NT * k, row = id / VCH<HEADS>, ch = id - row * VCH<HEADS>;
        if (id < VROWS * VCH<HEADS>) *reinterpret_cast<u32x4*>(VT + row * VS<HEADS> + ch * 16) = vt[k];
    }
}

// ---------------- phase 3: one head for the wave's 16 queries ------------------------------------------------------------------------------
// K fragments of head hd (A operand: lane = key row kt*16 + i16, k = 8 g + j; the head's channels 32..39 in the g = 0 lanes of the second k-step)
__device__ __forceinline__ void load_k_frag(const f16* kbase, int Nk, int hd, int g, int i16, u32x4 (&kf)[5][2]) {
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
        const int key = kt * 16 + i16;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 t = {0, 0, 0, 0};
            if (key < Nk && (ks == 0 || g == 0))
                t = *reinterpret_cast<const u32x4*>(kbase + (size_t)key * (2 * C) + hd * DH + ks * 32 + 8 * g);
            kf[kt][ks] = t;
        }
    }
}
// kf holds head hd's K fragments on entry and head hd + 1's on return; VT is a V tile of row stride V_STRIDE in which the head is number v_head
template <int TM, int V_STRIDE>
__device__ __forceinline__ void attn_head(char* XT, const char* VT, const f16* kbase, int Nk, int hd, int v_head, int qrow, int g, int i16, u32x4 (&kf)[5][2]) {
    // Q fragments of this head (B operand: lane = query column, k = 8 g + j)
    f16x8 qf[2];
    {
        const int c0 = hd * DH + 8 * g;                               // ks = 0: channels 0..31 of the head
        qf[0] = *reinterpret_cast<const f16x8*>(XT + xt_addr<TM>(qrow, c0));
        u32x4 z = {0, 0, 0, 0};
        if (g == 0) z = *reinterpret_cast<const u32x4*>(XT + xt_addr<TM>(qrow, hd * DH + 32));
        qf[1] = frag_of(z);
    }
    f32x4 s[5];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag_of(kf[kt][0]), qf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag_of(kf[kt][1]), qf[1], s[kt], 0, 0, 0);
    }
    if (hd + 1 < NH) load_k_frag(kbase, Nk, hd + 1, g, i16, kf);      // next head's K while this head's softmax / P V run
    // masked softmax over the keys of query i16 (lane holds keys kt*16 + 4g + r)
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (kt * 16 + 4 * g + r >= Nk) s[kt][r] = -INFINITY;
            mx = fmaxf(mx, s[kt][r]);
        }
    mx = group_max(mx);
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(s[kt][r] - mx); s[kt][r] = e; l += e; }
    l = group_sum(l);
    // P fragments (B operand of the second product; MFMA k index 8g + j <-> key t2*32 + (j < 4 ? 4g + j : 16 + 4g + j - 4))
    f16x8 pf[3];
#pragma unroll
    for (int t2 = 0; t2 < 3; ++t2) {
        u32x4 f;
        f[0] = pk(s[2 * t2][0], s[2 * t2][1]); f[1] = pk(s[2 * t2][2], s[2 * t2][3]);
        if (2 * t2 + 1 < 5) { f[2] = pk(s[2 * t2 + 1][0], s[2 * t2 + 1][1]); f[3] = pk(s[2 * t2 + 1][2], s[2 * t2 + 1][3]); }
        else { f[2] = 0; f[3] = 0; }
        pf[t2] = frag_of(f);
    }
    f32x4 o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t2 = 0; t2 < 3; ++t2)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const char* addr = VT + (32 * t2 + 4 * g + (i16 >> 2)) * V_STRIDE + (v_head * DH + a * 16 + 4 * (i16 & 3)) * 2;
            const u32x2 lo = tr_read(addr);
            const u32x2 hi = tr_read(addr + 16 * V_STRIDE);
            o[a] = __builtin_amdgcn_mfma_f32_16x16x32_f16(frag_of(u32x4{lo[0], lo[1], hi[0], hi[1]}), pf[t2], o[a], 0, 0, 0);
        }
    // O^T: lane holds channels a*16 + 4g + r of query i16 -> fp16 over the head's (consumed) q columns
    const float inv = 1.0f / l;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int d = a * 16 + 4 * g;
        if (d < DH)
            *reinterpret_cast<u32x2*>(XT + xt_addr<TM>(qrow, hd * DH + d)) = u32x2{pk(o[a][0] * inv, o[a][1] * inv), pk(o[a][2] * inv, o[a][3] * inv)};
    }
}

// ---------------- phase 4, after the to_out GEMM: + bias -> fp16 -> LDS patch -> + residual -> fp16 -> row stores, row statistics ------------------
// SPLIT: the residual stream is split-fp16 (value = h + h_lo).  The LayerNorm reads the hi plane (its output is an fp16 MFMA operand either way: a
// branch-level rounding); the residual add here takes hi + lo and writes both planes, which is where the stream's precision lives.
template <int SPLIT, int TM, bool DBG>
__device__ __forceinline__ void epilogue(const XattnParams p, char* smem, const f32x4 (&acc)[5][4], int tid, int row0, int col0, int g, int i16, int m_blk) {
    constexpr int NT = THREADS<TM>;
    char* const patch = smem;                    // [TM rows][PROW]: all of XT and the first 2 KB / 1 KB of weight stage 0 (free: gemm_320 ends with a barrier)
    char* const stats = smem + XT_BYTES<TM> + WST<TM>;
    static_assert(TM * PROW <= XT_BYTES<TM> + WST<TM>, "the epilogue patch may reach into weight stage 0 but not beyond it");
    static_assert(TM * 40 * 8 <= WST<TM>, "the row-statistics scratch is weight stage 1");
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int n = col0 + i * 16 + 4 * g;
        const f16x4 bv = *reinterpret_cast<const f16x4*>(p.bo + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = row0 + j * 16 + i16;
            *reinterpret_cast<u32x2*>(patch + m * PROW + n * 2) =
                u32x2{pk(acc[i][j][0] + (float)bv[0], acc[i][j][1] + (float)bv[1]), pk(acc[i][j][2] + (float)bv[2], acc[i][j][3] + (float)bv[3])};
        }
    }
    __syncthreads();
    // TM rows x 40 chunks, 10 items per thread: all residual loads of the thread first, then the patch reads, then the stores
    const bool io = !(DBG && (p.debug & 16));
    f16x8 res[10], resl[SPLIT == 1 ? 10 : 1];
    u32x2 resl8[SPLIT == 2 ? 10 : 1];                 // lo8: the lo planes are one e5m2 byte per element (IgemmArgs::lo8)
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const int id = tid + NT * k, row = id / 40, ch = id - row * 40, m = m_blk + row;
        res[k] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (m < p.M && io) res[k] = *reinterpret_cast<const f16x8*>(p.h + (size_t)m * C + ch * 8);
        if constexpr (SPLIT == 1) {
            resl[k] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (m < p.M) resl[k] = *reinterpret_cast<const f16x8*>(p.h_lo + (size_t)m * C + ch * 8);
        }
        if constexpr (SPLIT == 2) {
            resl8[k] = u32x2{0, 0};
            if (m < p.M) resl8[k] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned char*>(p.h_lo) + (size_t)m * C + ch * 8);
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const int id = tid + NT * k, row = id / 40, ch = id - row * 40, m = m_blk + row;
        const f16x8 v = *reinterpret_cast<const f16x8*>(patch + row * PROW + ch * 16);
        f16x8 o;
        float s1 = 0.f, s2 = 0.f;
        if constexpr (SPLIT == 1) {
            f16x8 l;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (float)v[e] + (float)res[k][e] + (float)resl[k][e];
                o[e] = (f16)f; l[e] = (f16)(f - (float)o[e]);
                s1 += f; s2 = __builtin_fmaf(f, f, s2);
            }
            if (m < p.M) *reinterpret_cast<f16x8*>(p.out_lo + (size_t)m * C + ch * 8) = l;
        } else if constexpr (SPLIT == 2) {
            typedef float f2 __attribute__((ext_vector_type(2)));
            const f2 l01 = __builtin_amdgcn_cvt_pk_f32_bf8((int)resl8[k][0], false), l23 = __builtin_amdgcn_cvt_pk_f32_bf8((int)resl8[k][0], true);
            const f2 l45 = __builtin_amdgcn_cvt_pk_f32_bf8((int)resl8[k][1], false), l67 = __builtin_amdgcn_cvt_pk_f32_bf8((int)resl8[k][1], true);
            const float lv[8] = {l01[0], l01[1], l23[0], l23[1], l45[0], l45[1], l67[0], l67[1]};
            float d[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (float)v[e] + (float)res[k][e] + lv[e];
                o[e] = (f16)f; d[e] = f - (float)o[e];
                s1 += f; s2 = __builtin_fmaf(f, f, s2);
            }
            int w0 = __builtin_amdgcn_cvt_pk_bf8_f32(d[0], d[1], 0, false); w0 = __builtin_amdgcn_cvt_pk_bf8_f32(d[2], d[3], w0, true);
            int w1 = __builtin_amdgcn_cvt_pk_bf8_f32(d[4], d[5], 0, false); w1 = __builtin_amdgcn_cvt_pk_bf8_f32(d[6], d[7], w1, true);
            if (m < p.M) *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned char*>(p.out_lo) + (size_t)m * C + ch * 8) = u32x2{(unsigned)w0, (unsigned)w1};
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float f = (float)v[e] + (float)res[k][e]; o[e] = (f16)f; s1 += f; s2 = __builtin_fmaf(f, f, s2); }
        }
        if (m < p.M && io) *reinterpret_cast<f16x8*>(p.out + (size_t)m * C + ch * 8) = o;
        // row statistics for norm3 folded into the GEGLU GEMM: the item's partial sums go to weight stage 1 (free since the to_out GEMM's last barrier; the
        // patch reaches into stage 0 only), [TM rows][40 chunks] float2 = one stage exactly
        if (p.row_stats) *reinterpret_cast<float2*>(stats + (row * 40 + ch) * 8) = float2{s1, s2};
    }
    if (p.row_stats) {                               // (uniform branch)
        __syncthreads();
        if (tid < TM && m_blk + tid < p.M) {
            float a1 = 0.f, a2 = 0.f;
            const char* src = stats + tid * 320;
#pragma unroll
            for (int c2 = 0; c2 < 20; ++c2) { const f32x4 t = *reinterpret_cast<const f32x4*>(src + c2 * 16); a1 += t[0] + t[2]; a2 += t[1] + t[3]; }
            *reinterpret_cast<float2*>(p.row_stats + (size_t)(m_blk + tid) * 2) = float2{a1, a2};
        }
    }
}

// 128-row tiles, 8 waves as 2 (rows) x 4 (columns), one workgroup per CU; the only kernel with the debug bits
template <int SPLIT>
__global__ __launch_bounds__(512, 2) void xattn_block_kernel(XattnParams p) {
    constexpr int TM = 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const XT = smem;
    char* const VT = smem + XT_BYTES<TM>;           // V tile [96][672 B] (the weight stages between the GEMMs)
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = (w >> 2) * 64, col0 = (w & 3) * 80;       // the wave's GEMM tile
    const int g = lane >> 4, i16 = lane & 15;
    const int m_blk = blockIdx.x * TM;
    const int b = m_blk / p.HW;                      // the tile lies inside one sample (HW % 128 == 0)
    const f16* const kbase = p.kv + (size_t)b * p.Nk * (2 * C);

    // phase 0: LayerNorm -> XT
    stage_w<TM>(p.wq, VT, w, lane, 0, 0);           // Wq's first k-step lands while the LayerNorm runs (VT = the weight stages for now)
    u32x4 vt[8];
    load_v<512, NH>(kbase + C, p.Nk, tid, vt);      // the V loads fly under the LayerNorm; their LDS writes wait until the to_q GEMM has released the stages
    ln_rows<TM, true>(p, XT, w, lane, m_blk);
    __syncthreads();

    // phases 1, 2: q = LN(h) Wq^T -> XT; V -> LDS
    f32x4 acc[5][4];
    if (!(p.debug & 4)) gemm_320<TM, true>(p.wq, smem, w, lane, row0, col0, acc);       // ends with a barrier: XT and the stages are free
    else { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); for (int i = 0; i < 5; ++i) for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{1.f, 1.f, 1.f, 1.f}; }
    store_q<TM>(XT, acc, p.c, row0, col0, g, i16);
    store_v<512, NH>(VT, tid, vt);
    __syncthreads();

    // phase 3: attention, 16 queries per wave, heads in sequence
    if (!(p.debug & 1)) {
        u32x4 kf[5][2];
        load_k_frag(kbase, p.Nk, 0, g, i16, kf);
#pragma unroll
        for (int hd = 0; hd < NH; ++hd) attn_head<TM, VS<NH>>(XT, VT, kbase, p.Nk, hd, hd, 16 * w + i16, g, i16, kf);
    }
    __syncthreads();

    // phase 4: out = O Wo^T + bias + h
    if (!(p.debug & 2)) gemm_320<TM, false>(p.wo, smem, w, lane, row0, col0, acc);     // ends with a barrier: XT becomes the epilogue patch
    epilogue<SPLIT, TM, true>(p, smem, acc, tid, row0, col0, g, i16, m_blk);
}

// 64-row tiles, 4 waves as 1 x 4, two workgroups per CU: the default.  No debug bits.
template <int SPLIT>
__global__ __launch_bounds__(256, 2) void xattn64_kernel(XattnParams p) {
    constexpr int TM = 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const XT = smem;
    char* const VT = smem + XT_BYTES<TM>;           // V half tile [96][352 B] (the weight stages between the GEMMs)
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // 0..3: LayerNorm rows 16 w.., GEMM columns 80 w.., attention queries 16 w..
    const int g = lane >> 4, i16 = lane & 15;
    const int m_blk = blockIdx.x * TM;
    const int b = m_blk / p.HW;                      // the tile lies inside one sample (HW % 64 == 0)
    const f16* const kbase = p.kv + (size_t)b * p.Nk * (2 * C);

    // phase 0: LayerNorm -> XT
    stage_w<TM>(p.wq, VT, w, lane, 0, 0);           // Wq's first k-step lands while the LayerNorm runs (VT = the weight stages for now)
    ln_rows<TM, false>(p, XT, w, lane, m_blk);
    __syncthreads();

    // phase 1: q = LN(h) Wq^T -> XT
    u32x4 vt[9];
    load_v<256, NH / 2>(kbase + C, p.Nk, tid, vt);  // V half 0 travels under the to_q GEMM (issued here, not next to the LayerNorm's 16 row loads: with both in flight phase 0 spilled 34 registers)
    f32x4 acc[5][4];
    gemm_320<TM, true>(p.wq, smem, w, lane, 0, 80 * w, acc);       // ends with a barrier: XT and the stages are free
    store_q<TM>(XT, acc, p.c, 0, 80 * w, g, i16);

    // phases 2, 3 per half of the heads: V half -> LDS, then attention over its four heads, 16 queries per wave
    u32x4 kf[5][2];
    load_k_frag(kbase, p.Nk, 0, g, i16, kf);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        if (hh == 1) __syncthreads();                 // every wave is done with V half 0
        store_v<256, NH / 2>(VT, tid, vt);
        if (hh == 0) load_v<256, NH / 2>(kbase + C + (NH / 2) * DH, p.Nk, tid, vt);   // the second half's rows travel while the first half's heads compute
        __syncthreads();
#pragma unroll
        for (int hl = 0; hl < NH / 2; ++hl) attn_head<TM, VS<NH / 2>>(XT, VT, kbase, p.Nk, (NH / 2) * hh + hl, hl, 16 * w + i16, g, i16, kf);
    }
    __syncthreads();

    // phase 4: out = O Wo^T + bias + h
    gemm_320<TM, false>(p.wo, smem, w, lane, 0, 80 * w, acc);     // ends with a barrier: XT becomes the epilogue patch
    epilogue<SPLIT, TM, false>(p, smem, acc, tid, 0, 80 * w, g, i16, m_blk);
}

typedef void (*xattn_kernel_t)(XattnParams);
// the three stream forms of one tile size: dynamic-LDS limit once per process, then the launch of form 0 plain / 1 split-fp16 / 2 lo8
template <int TM>
int launch_tile(xattn_kernel_t const (&kernel)[3], int form, const XattnParams& p, hipStream_t s) {
    static bool configured = false;
    if (!configured) {
        for (xattn_kernel_t k : kernel) CS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES<TM>));
        configured = true;
    }
    hipLaunchKernelGGL(kernel[form], dim3(p.M / TM), dim3(THREADS<TM>), LDS_BYTES<TM>, s, p);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

}  // namespace

int launch_xattn_block(const XattnArgs& a, hipStream_t s) {
    const bool tile64 = tune().xattn_tile == 64 && a.HW % 64 == 0;      // the default: 64-row tiles, two workgroups per CU
    if (!a.h || !a.out || !a.ln_g || !a.ln_b || !a.wq || !a.wo || !a.bo || !a.kv) CS_FAIL(CS_E_ARG, "xattn_block: null pointer");
    if (a.C != 320 || a.heads != 8) CS_FAIL(CS_E_UNSUPPORTED, "xattn_block: built for C = 320, 8 heads (got C = %d, heads = %d)", a.C, a.heads);
    if (a.Nk < 1 || a.Nk > 80) CS_FAIL(CS_E_SHAPE, "xattn_block: 1 <= Nk <= 80 (got %d)", a.Nk);
    if (a.HW % 128 && !tile64) CS_FAIL(CS_E_SHAPE, "xattn_block: rows per sample must be a multiple of %d", 128);
    if (a.M <= 0) return a.M < 0 ? CS_E_SHAPE : CS_OK;
    if (a.M % a.HW) CS_FAIL(CS_E_SHAPE, "xattn_block: M must be a whole number of samples");
    XattnParams p;
    if ((a.h_lo == nullptr) != (a.out_lo == nullptr)) CS_FAIL(CS_E_ARG, "xattn_block: h_lo and out_lo go together");
    p.h = a.h; p.out = a.out; p.h_lo = a.h_lo; p.out_lo = a.out_lo; p.row_stats = a.row_stats; p.ln_g = a.ln_g; p.ln_b = a.ln_b; p.ln_eps = a.ln_eps; p.wq = a.wq; p.wo = a.wo; p.bo = a.bo; p.kv = a.kv;
    p.M = a.M; p.HW = a.HW; p.Nk = a.Nk; p.c = a.scale * 1.4426950408889634f; p.debug = tune().debug;
    const int form = a.h_lo ? (a.lo8 ? 2 : 1) : 0;
    if (tile64) return launch_tile<64>({xattn64_kernel<0>, xattn64_kernel<1>, xattn64_kernel<2>}, form, p, s);
    return launch_tile<128>({xattn_block_kernel<0>, xattn_block_kernel<1>, xattn_block_kernel<2>}, form, p, s);
}
