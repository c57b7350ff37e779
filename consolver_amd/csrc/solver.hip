// ConsistencySolver update kernels (HBM-bound streaming + latency-bound policy MLP).
//
//   cs_lms_ddim_step  : CFG combine + coefficient fix-up + linear-multistep combine + DDIM
//                       (scheduler_ppo.py:165-175,253-283,306-332; denoise_ppo.py:96-100)
//   cs_lms_euler_step : same with the flow-matching Euler epilogue
//                       (edit_ppo/scheduler_fmppo.py:400-436)
//   cs_dpm_multistep_step : CFG combine + model-output conversion + Multistep DPM-Solver update (orders 1, 2)
//   cs_linear_step : CFG combine + model-output conversion + an n-term linear update, n <= 4 (DEIS, iPNDM)
//   cs_unipc_step : CFG combine + x0 conversion + UniPC corrector of the previous update + predictor (bh1 / bh2, orders 1, 2)
//   cs_fm_general_step : the flow-matching baselines' update (Euler / Heun / dpm-solver / multistep, edit_ppo/scheduler_fm.py:405-482)
//   cs_true_cfg_combine : true classifier-free guidance of the Kontext edit, neg + scale * (pos - neg) (edit_ppo/pipeline.py:1115)
//   cs_factor_probs   : FactorNetPPO.forward_ (factor_net_ppo.py:137-157)
//   cs_cosine_features: compute_cosine_similarity (factor_net_ppo.py:108-130)
//   cs_sample_actions / cs_gather_actions / cs_action_probs / cs_step_masks / cs_stack_history
//
// Arithmetic is fp32 in the reference's operation order (file is built with
// -ffp-contract=off so that a*b+c is two roundings like torch's separate ops);
// half/bfloat I/O is converted on load and rounded once on store.
#include "common.h"
#include <type_traits>

namespace {

// ---------------------------------------------------------------- element I/O
// A dtype's element, its 16-byte vector width and its conversions; round(v) is the image of an fp32 value in the dtype.
template <typename T> struct Io;
template <> struct Io<float> {
    static constexpr int VEC = 4;
    typedef float elem_t;
    __device__ static float to_f32(float v) { return v; }
    __device__ static float from_f32(float v) { return v; }
    __device__ static float round(float v) { return v; }
};
template <> struct Io<f16> {
    static constexpr int VEC = 8;
    typedef f16 elem_t;
    __device__ static float to_f32(f16 v) { return (float)v; }
    __device__ static f16 from_f32(float v) { return (f16)v; }
    __device__ static float round(float v) { return (float)(f16)v; }
};
struct bf16_tag {};
template <> struct Io<bf16_tag> {
    static constexpr int VEC = 8;
    typedef u16 elem_t;
    __device__ static float to_f32(u16 v) { return bf16_to_f32(v); }
    __device__ static u16 from_f32(float v) { return f32_to_bf16(v); }
    __device__ static float round(float v) { return bf16_to_f32(f32_to_bf16(v)); }
};

template <typename E, int N> using Vec = E __attribute__((ext_vector_type(N)));

// W consecutive elements of dtype T as they lie in memory: one element (W == 1, the tail), else 16-byte vectors -- two of them for 8 values of an
// fp32 state beside 8-wide 16-bit model outputs, and a single 8-byte one for 4 16-bit values (the low-precision copy of a 4-wide fp32 result).
// load and unpack are separate so that a step issues every load before it converts the first value: one round trip to memory per iteration.
template <typename T, int W>
struct Raw {
    typedef typename Io<T>::elem_t E;
    static constexpr int L = W < Io<T>::VEC ? W : Io<T>::VEC, N = W / L;
    static_assert(W == 1 || W == 4 || W == 8, "one element, or the vector width of a 32-bit / 16-bit dtype");
    typedef Vec<E, L> vec_t;
    vec_t r[N];
    __device__ __forceinline__ void load(const void* p, int64_t i) {
        const vec_t* q = reinterpret_cast<const vec_t*>(reinterpret_cast<const E*>(p) + i);
#pragma unroll
        for (int k = 0; k < N; ++k) r[k] = q[k];
    }
    __device__ __forceinline__ float get(int j) const { return Io<T>::to_f32(r[j / L][j % L]); }
    __device__ __forceinline__ void unpack(float (&o)[W]) const {
#pragma unroll
        for (int k = 0; k < N; ++k)
#pragma unroll
            for (int j = 0; j < L; ++j) o[k * L + j] = Io<T>::to_f32(r[k][j]);
    }
};
// ... and the way back: each value rounded once to T, the same vectors stored
template <typename T, int W>
__device__ __forceinline__ void store(void* p, int64_t i, const float (&o)[W]) {
    typedef Raw<T, W> R;
    typename R::vec_t* q = reinterpret_cast<typename R::vec_t*>(reinterpret_cast<typename R::E*>(p) + i);
#pragma unroll
    for (int k = 0; k < R::N; ++k) {
        typename R::vec_t v;
#pragma unroll
        for (int j = 0; j < R::L; ++j) v[j] = Io<T>::from_f32(o[k * R::L + j]);
        q[k] = v;
    }
}
// the low-precision copy of a result (x_out_lp of the args structs) as fp16 (lp_bf16 == 0) or bf16: the 16-bit view of an fp32 state, what
// `x.to(model dtype)` would round the stored result to
template <int W>
__device__ __forceinline__ void store_lp(void* p, int64_t i, const float (&o)[W], int lp_bf16) {
    if (lp_bf16) store<bf16_tag, W>(p, i, o); else store<f16, W>(p, i, o);
}

// classifier-free guidance on the model output: e := u + g (e - u), rounded to the model dtype like torch's 16-bit ops
template <typename TI, int W>
__device__ __forceinline__ void cfg_combine(float (&e)[W], const float (&u)[W], float g) {
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = Io<TI>::round(u[j] + g * (e[j] - u[j]));
}
// the "converted model output" (x0 / eps prediction) of the dpm and unipc steps: e := conv_x x + conv_e e, rounded to the model dtype like the combined eps
template <typename TI, int W>
__device__ __forceinline__ void convert_output(float (&e)[W], const float (&x)[W], float conv_x, float conv_e) {
#pragma unroll
    for (int j = 0; j < W; ++j) e[j] = Io<TI>::round(conv_x * x[j] + conv_e * e[j]);
}

// ---------------------------------------------------------------- the streaming skeleton
// Every update kernel is this one: grid (gx, nb) walks nb ranges of n elements, a grid-stride body of F::V elements per lane and the n % F::V
// elements of the tail, which block x = 0 of each range handles.  F is the solver: its Params, its per-range set-up F(p, range), its vector width V
// and one step<W>(p, i) that loads (raw, every tensor before the first conversion), combines, updates and stores W elements at i.  The tail is
// step<1>, so body and tail are the same code.  The per-sample kernels (lms, dpm) run it with nb = B, n = elems; the others have no per-sample
// coefficient and run one flat range nb = 1, n = B * elems, where the vector body stays 16-byte aligned whatever elems is.
// TI is the model outputs' dtype (eps, history, converted outputs), TX the sample's and TO the result's: each TI, or fp32 beside 16-bit model
// outputs (scheduler_fmppo.py:354 upcasts the sample, not the model output).
template <typename F>
__global__ __launch_bounds__(256) void stream_kernel(typename F::Params p, int64_t n) {
    const F f(p, blockIdx.y);
    const int64_t base = (int64_t)blockIdx.y * n, nvec = n / F::V;
    // the tail is fewer than V elements, one per thread; it comes first so that nothing of it is live across the body's loop (with the tail as a
    // loop after the body the fp32 lms kernel runs out of SGPRs and loses a wave per SIMD)
    const int64_t t = nvec * F::V + threadIdx.x;
    if (blockIdx.x == 0 && t < n) f.template step<1>(p, base + t);
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x)
        f.template step<F::V>(p, base + v * F::V);
}

// ---------------------------------------------------------------- linear multistep + DDIM / Euler
struct StepParams {
    const void* x; const void* ec; const void* eu; float g;
    const void* hist[CS_MAX_ORDER];
    int m, order, scaler;
    const float* actions; int astride;
    void* x_out; void* eps_out;
    float sat, s1mat, sap, s1map; int vpred; float dt;
    void* x_lp;  // optional 16-bit copy of an fp32 result (CsStepArgs::x_out_lp)
    int lp_bf16; // ... as bf16 (else fp16)
};

// coefficient fix-up, identical for every thread of a sample (b is block-uniform)
__device__ __forceinline__ void make_coeffs(const StepParams& p, int b, float (&c)[CS_MAX_ORDER], float& sc0, float& sc1) {
    const float* a = p.actions + (int64_t)b * p.astride;
#pragma unroll
    for (int k = 0; k < CS_MAX_ORDER; ++k) c[k] = 0.f;
    if (p.m > 1) {
        // list [a0+1, a1, ..., a_{order-2}, placeholder]; entry m-1 := 1 - sum(first m-1)
#pragma unroll
        for (int k = 0; k < CS_MAX_ORDER - 1; ++k)
            if (k < p.m - 1) c[k] = (k == 0) ? (a[0] + 1.0f) : a[k];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < CS_MAX_ORDER - 1; ++k)
            if (k < p.m - 1) s = s + c[k];
#pragma unroll
        for (int k = 1; k < CS_MAX_ORDER; ++k)
            if (k == p.m - 1) c[k] = 1.0f - s;
    }
    sc0 = (p.scaler >= 1) ? a[p.order - 1] + 1.0f : 1.0f;
    sc1 = (p.scaler >= 2) ? a[p.order] + 1.0f : 1.0f;
}

// h[k].get(j) is element j of history entry k: loaded, and converted and read here, for k < m - 1 only
template <typename TI, bool EULER, int W>
__device__ __forceinline__ float solve_one(const StepParams& p, float x, float e0, const Raw<TI, W> (&h)[CS_MAX_ORDER - 1], int j, const float (&c)[CS_MAX_ORDER],
                                           float sc0, float sc1) {
    float eff;
    if (p.m == 1) {
        eff = e0;
    } else {
        eff = c[0] * e0;
#pragma unroll
        for (int k = 1; k < CS_MAX_ORDER; ++k)
            if (k < p.m) eff = eff + c[k] * h[k - 1].get(j);
    }
    if (p.scaler >= 1) eff = eff * sc0;
    if (p.scaler >= 2) x = x * sc1;
    if (EULER) {
        // scheduler_fmppo.py:429 `sample + dt * effective_model_output`: with ONE history entry and no scale the effective
        // output is the bf16 / f16 model output itself and dt is a 0-d fp32 tensor, so torch runs the product as a 16-bit op
        // (dt cast to the model dtype, product rounded to it) before the fp32 add; otherwise the [B,1,1] fp32 coefficients
        // have promoted everything to fp32.
        if (p.m == 1 && p.scaler == 0) return x + Io<TI>::round(Io<TI>::round(p.dt) * eff);
        return x + p.dt * eff;
    }
    if (p.vpred) eff = p.sat * eff + p.s1mat * x;
    float x0 = (x - p.s1mat * eff) / p.sat;
    return p.sap * x0 + p.s1map * eff;
}

template <typename TI, typename TX, typename TO, bool EULER>
struct LmsStep {
    typedef StepParams Params;
    static constexpr int V = Io<TI>::VEC;
    float c[CS_MAX_ORDER], sc0, sc1;
    __device__ __forceinline__ LmsStep(const StepParams& p, int b) { make_coeffs(p, b, c, sc0, sc1); }
    template <int W>
    __device__ __forceinline__ void step(const StepParams& p, int64_t i) const {
        Raw<TX, W> rx;
        Raw<TI, W> re, ru, rh[CS_MAX_ORDER - 1];
        rx.load(p.x, i);
        re.load(p.ec, i);
        if (p.eu) ru.load(p.eu, i);                          // (every branch on p is block-uniform; a tensor that is not loaded is not read either)
        float x[W], e[W], u[W], o[W];
        rx.unpack(x); re.unpack(e);
        if (p.eu) { ru.unpack(u); cfg_combine<TI>(e, u, p.g); }
        // the history is loaded after the combine: two trips to memory per iteration, not one as in the other steps.  It is the order this update
        // has always had, and the one its HBM-bound figure is known to hold with: at 2.3 GB (fp32, 4096 x 16384, m = 4, CFG, 16-bit copy) 4 of 8
        // processes ran 3 - 10 % below 5.85 TB/s with every load issued first, 2 of 20 with this order, on a machine where the figure drifts
#pragma unroll
        for (int k = 0; k < CS_MAX_ORDER - 1; ++k)
            if (k < p.m - 1) rh[k].load(p.hist[k], i);
        if (p.eps_out) store<TI, W>(p.eps_out, i, e);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = solve_one<TI, EULER>(p, x[j], e[j], rh, j, c, sc0, sc1);
        store<TO, W>(p.x_out, i, o);
        if (p.x_lp) store_lp<W>(p.x_lp, i, o, p.lp_bf16);
    }
};

// ---------------------------------------------------------------- Multistep DPM-Solver
// Every variant (dpmsolver / dpmsolver++, epsilon / v prediction, first / second order, midpoint / heun) is the same linear update per
// element; the variant lives in five host scalars (scheduling_dpm.py).  m0 is the "converted model output" of this step (the history entry
// of the next one), rounded to the model dtype like the combined eps; m1 is the previous step's m0 (NULL at first order).
struct DpmParams {
    const void* x; const void* ec; const void* eu; float g;
    const void* m1;
    void* x_out; void* m_out;
    float conv_x, conv_e, cx, c0, c1;
    void* x_lp;  // as StepParams::x_lp
    int lp_bf16;
};

__device__ __forceinline__ float dpm_one(const DpmParams& p, float x, float m0, float m1) {
    float r = p.cx * x + p.c0 * m0;
    if (p.m1) r = r + p.c1 * m1;
    return r;
}

template <typename TI, typename TX, typename TO>
struct DpmStep {
    typedef DpmParams Params;
    static constexpr int V = Io<TI>::VEC;
    __device__ __forceinline__ DpmStep(const DpmParams&, int) {}
    template <int W>
    __device__ __forceinline__ void step(const DpmParams& p, int64_t i) const {
        Raw<TX, W> rx;
        Raw<TI, W> re, ru, r1;
        rx.load(p.x, i);
        re.load(p.ec, i);
        if (p.eu) ru.load(p.eu, i);
        if (p.m1) r1.load(p.m1, i);                          // (dpm_one reads m1 under the same condition)
        float x[W], e[W], u[W], h[W], o[W];
        rx.unpack(x); re.unpack(e);
        if (p.eu) { ru.unpack(u); cfg_combine<TI>(e, u, p.g); }
        if (p.m1) r1.unpack(h);
        convert_output<TI>(e, x, p.conv_x, p.conv_e);
        if (p.m_out) store<TI, W>(p.m_out, i, e);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = dpm_one(p, x[j], e[j], h[j]);
        store<TO, W>(p.x_out, i, o);
        if (p.x_lp) store_lp<W>(p.x_lp, i, o, p.lp_bf16);
    }
};

// ---------------------------------------------------------------- n-term linear update (DEIS, iPNDM)
// x' = cx xb + c[0] m0 + c[1] hist[0] + ... + c[terms - 1] hist[terms - 2], left to right: DEIS up to order 3 and iPNDM's Adams-Bashforth
// combinations up to four terms, all variant logic in host scalars (scheduling_deis.py, scheduling_pndm.py).  m0 is the converted model output
// as in the dpm step, except that the identity conversion is skipped; xb is x, or a saved sample that the update restarts from (iPNDM's
// second forward at the first grid point).
struct LinParams {
    const void* x; const void* ec; const void* eu; float g;
    const void* xb;
    const void* hist[CS_LIN_MAX_TERMS - 1];
    int terms, convert;
    void* x_out; void* m_out;
    float conv_x, conv_e, cx, c[CS_LIN_MAX_TERMS];
    void* x_lp;  // as StepParams::x_lp
    int lp_bf16;
};

// h[k].get(j) is element j of history entry k: loaded, and converted and read here, for k < terms - 1 only
template <typename TI, int W>
__device__ __forceinline__ float lin_one(const LinParams& p, float xb, float m0, const Raw<TI, W> (&h)[CS_LIN_MAX_TERMS - 1], int j) {
    float r = p.cx * xb + p.c[0] * m0;
#pragma unroll
    for (int k = 1; k < CS_LIN_MAX_TERMS; ++k)
        if (k < p.terms) r = r + p.c[k] * h[k - 1].get(j);
    return r;
}

template <typename TI, typename TX, typename TO>
struct LinStep {
    typedef LinParams Params;
    static constexpr int V = Io<TI>::VEC;
    __device__ __forceinline__ LinStep(const LinParams&, int) {}
    template <int W>
    __device__ __forceinline__ void step(const LinParams& p, int64_t i) const {
        Raw<TX, W> rx, rb;
        Raw<TI, W> re, ru, rh[CS_LIN_MAX_TERMS - 1];
        rx.load(p.x, i);
        if (p.xb) rb.load(p.xb, i);
        re.load(p.ec, i);
        if (p.eu) ru.load(p.eu, i);
#pragma unroll
        for (int k = 0; k < CS_LIN_MAX_TERMS - 1; ++k)
            if (k < p.terms - 1) rh[k].load(p.hist[k], i);   // (lin_one reads entry k under the same condition)
        float x[W], b[W], e[W], u[W], o[W];
        rx.unpack(x); re.unpack(e);
        if (p.eu) { ru.unpack(u); cfg_combine<TI>(e, u, p.g); }
        if (p.convert) convert_output<TI>(e, x, p.conv_x, p.conv_e);
        if (p.m_out) store<TI, W>(p.m_out, i, e);
        if (p.xb) rb.unpack(b);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = lin_one<TI>(p, p.xb ? b[j] : x[j], e[j], rh, j);
        store<TO, W>(p.x_out, i, o);
        if (p.x_lp) store_lp<W>(p.x_lp, i, o, p.lp_bf16);
    }
};

// ---------------------------------------------------------------- UniPC (bh1 / bh2, orders 1 and 2, x0 prediction)
// One step of UniPC is the corrector of the PREVIOUS update (it needs this step's model output) followed by this step's predictor.  Both are
// linear in the same tensors, so the step is one pass: the variant lives in nine host scalars (scheduling_unipc.py).  x is the predicted sample
// (the previous predictor's output), x_last the previous step's corrected sample, m0 / m1 the converted outputs of the two previous steps.
// The state (x, x_last, x_c, x_next) has the result's dtype TO: launch_unipc_step checks it.
struct UnipcParams {
    const void* x; const void* ec; const void* eu; float g;
    const void* x_last; const void* m0; const void* m1;
    void* x_out; void* m_out; void* x_last_out;
    float conv_x, conv_e, a_x, a_0, a_1, a_n, p_x, p_0, p_1;
    int corr;    // apply the corrector (else x_c = x)
    void* x_lp;  // as StepParams::x_lp
    int lp_bf16;
};

// x_c is rounded to the dtype it is stored in before the predictor reads it: the pass is a corrector launch followed by a predictor launch.
// A history value that is not read arrives as zero (its coefficient is zero as well: the term adds an exact 0), so the update has no branch.
template <typename TO>
__device__ __forceinline__ void unipc_one(const UnipcParams& p, float x, float xl, float mn, float m0, float m1, float& xc, float& xn) {
    const float c = Io<TO>::round(p.a_x * xl + p.a_0 * m0 + p.a_1 * m1 + p.a_n * mn);
    xc = p.corr ? c : x;
    xn = p.p_x * xc + p.p_0 * mn + p.p_1 * m0;
}

template <typename TI, typename TO>
struct UnipcStep {
    typedef UnipcParams Params;
    static constexpr int V = Io<TI>::VEC;
    __device__ __forceinline__ UnipcStep(const UnipcParams&, int) {}
    template <int W>
    __device__ __forceinline__ void step(const UnipcParams& p, int64_t i) const {
        Raw<TO, W> rx, rxl = {};
        Raw<TI, W> re, ru, r0 = {}, r1 = {};                 // (unipc_one takes a history value that is not read as zero)
        rx.load(p.x, i);
        re.load(p.ec, i);
        if (p.eu) ru.load(p.eu, i);
        if (p.corr) rxl.load(p.x_last, i);
        if (p.m0) r0.load(p.m0, i);
        if (p.m1) r1.load(p.m1, i);
        float x[W], xl[W], e[W], u[W], h0[W], h1[W], oc[W], on[W];
        rx.unpack(x); rxl.unpack(xl); re.unpack(e); r0.unpack(h0); r1.unpack(h1);
        if (p.eu) { ru.unpack(u); cfg_combine<TI>(e, u, p.g); }
        convert_output<TI>(e, x, p.conv_x, p.conv_e);
#pragma unroll
        for (int j = 0; j < W; ++j) unipc_one<TO>(p, x[j], xl[j], e[j], h0[j], h1[j], oc[j], on[j]);
        store<TI, W>(p.m_out, i, e);
        if (p.x_last_out) store<TO, W>(p.x_last_out, i, oc);
        store<TO, W>(p.x_out, i, on);
        if (p.x_lp) store_lp<W>(p.x_lp, i, on, p.lp_bf16);
    }
};

// ---------------------------------------------------------------- flow-matching baselines (edit_ppo/scheduler_fm.py:405-482)
// Every branch of the Euler / Heun / dpm-solver / multistep step is x' = cast_out(x_base + c * w) with w = v2 or v1 + v2; which base, whether
// v1 is read and the scalar c are decided on the host (scheduling_fm.py).  c is a 0-d fp32 tensor in the reference, so with a 16-bit model
// output `v1 + v2` and `c * w` are 16-bit ops (c cast to the model dtype, each result rounded to it) before the fp32 add -- the m == 1 form
// of solve_one.
struct FmParams { const void* x; const void* v2; const void* v1; float c; void* x_out; };

template <typename TI>
__device__ __forceinline__ float fm_one(const FmParams& p, float x, float v2, float v1) {
    const float w = p.v1 ? Io<TI>::round(v1 + v2) : v2;
    return x + Io<TI>::round(Io<TI>::round(p.c) * w);
}

template <typename TI, typename TX, typename TO>
struct FmStep {
    typedef FmParams Params;
    static constexpr int V = Io<TI>::VEC;
    __device__ __forceinline__ FmStep(const FmParams&, int) {}
    template <int W>
    __device__ __forceinline__ void step(const FmParams& p, int64_t i) const {
        Raw<TX, W> rx;
        Raw<TI, W> r2, r1;
        rx.load(p.x, i);
        r2.load(p.v2, i);
        if (p.v1) r1.load(p.v1, i);                          // (fm_one reads v1 under the same condition)
        float x[W], e[W], h[W], o[W];
        rx.unpack(x); r2.unpack(e);
        if (p.v1) r1.unpack(h);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = fm_one<TI>(p, x[j], e[j], h[j]);
        store<TO, W>(p.x_out, i, o);
    }
};

// ---------------------------------------------------------------- true classifier-free guidance (edit_ppo/pipeline.py:1115)
// out = cast_out(neg + scale * (pos - neg)): the value rounded ONCE to the output dtype (the rule of cfg_combine), not the reference's
// three 16-bit ops.  The three fp32 operations are carried with their rounding errors (two-sum for the difference and the sum, an fma for the product's
// error), so what is rounded at the end is the exact value to ~2^-45: where 4 pos and 3 neg cancel, the plain fp32 expression is off by several units of an
// fp32 -- or of a subnormal fp16 -- result.  Memory-bound: the ~20 flops per element are free.
__device__ __forceinline__ float true_cfg_one(float p, float n, float s) {
    const float d = p - n, db = d - p, de = (p - (d - db)) + (-n - db);          // d + de = p - n
    const float m = s * d, me = __builtin_fmaf(s, d, -m);                        // m + me = s * d
    const float r = n + m, rb = r - n, re = (n - (r - rb)) + (m - rb);           // r + re = n + m
    const float c = re + (me + s * de);
    return fabsf(c) < INFINITY ? r + c : r;                                      // (inf / NaN operands: the plain expression's result)
}

struct CfgParams { const void* pos; const void* neg; void* out; float scale; };

// V elements per lane: 8 with a 16-bit output (one 16-byte store; fp32 inputs as two 16-byte loads each), 4 for fp32 -> fp32.  Every lane reads its
// elements before it writes them and the vector body and the tail cover disjoint ranges, so out may be pos or neg when the element sizes are equal.
template <typename TX, typename TO>
struct TrueCfg {
    typedef CfgParams Params;
    static constexpr int V = Io<TO>::VEC;
    __device__ __forceinline__ TrueCfg(const CfgParams&, int) {}
    template <int W>
    __device__ __forceinline__ void step(const CfgParams& p, int64_t i) const {
        Raw<TX, W> ra, rb;
        ra.load(p.pos, i);
        rb.load(p.neg, i);
        float a[W], b[W], o[W];
        ra.unpack(a); rb.unpack(b);
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = true_cfg_one(a[j], b[j], p.scale);
        store<TO, W>(p.out, i, o);
    }
};

// ---------------------------------------------------------------- launchers
template <typename T> struct Tag { typedef T type; };
#define TYPE_OF(tag) typename decltype(tag)::type

// the one dtype ladder: f(Tag<T>{}) for a dtype code
template <typename F>
int with_dtype(int code, F&& f) {
    if (code == CS_F32) return f(Tag<float>{});
    if (code == CS_F16) return f(Tag<f16>{});
    if (code == CS_BF16) return f(Tag<bf16_tag>{});
    CS_FAIL(CS_E_DTYPE, "bad dtype %d", code);
}
// f(TI, TX, TO) of an update: the sample and the result have the model outputs' dtype io, or are fp32 beside 16-bit model outputs
template <typename F>
int with_step_dtypes(int io, bool x_f32, bool out_f32, F&& f) {
    return with_dtype(io, [&](auto ti) {
        const Tag<float> f32;
        if (x_f32) return out_f32 ? f(ti, f32, f32) : f(ti, f32, ti);
        return out_f32 ? f(ti, ti, f32) : f(ti, ti, ti);
    });
}

// what every update entry point refuses in the same words.  *empty: nothing to launch -- the entry point returns CS_OK for it once its own
// shape-independent checks have passed.
template <typename A>
int refuse_common(const A* a, bool* empty) {
    if (!a) CS_FAIL(CS_E_ARG, "args is NULL");
    if (a->B < 0 || a->elems < 0) CS_FAIL(CS_E_SHAPE, "negative shape");
    if constexpr (!std::is_same<A, CsFmStepArgs>::value)      // (the fm step writes no 16-bit copy)
        if (a->x_out_lp && (a->out_dtype != CS_F32 || (a->lp_dtype != CS_F16 && a->lp_dtype != CS_BF16)))
            CS_FAIL(CS_E_ARG, "x_out_lp is the 16-bit copy (lp_dtype CS_F16 or CS_BF16) of an fp32 result (out_dtype CS_F32)");
    const int io = a->io_dtype, od = a->out_dtype;
    const bool pair_ok = (io == CS_F32 && od == CS_F32) || (io == CS_F16 && (od == CS_F16 || od == CS_F32)) || (io == CS_BF16 && (od == CS_BF16 || od == CS_F32));
    if (!pair_ok) CS_FAIL(CS_E_DTYPE, "unsupported io/out dtype pair (%d,%d)", io, od);
    *empty = (a->B == 0 || a->elems == 0);
    return CS_OK;
}
// x_is_f32 of the args structs: an fp32 sample beside 16-bit model outputs
template <typename A>
bool x_f32(const A* a) { return a->x_is_f32 != 0 && a->io_dtype != CS_F32; }

// memory-bound: cap the grid at ~8 blocks per CU overall (2048 blocks over the nb ranges) and grid-stride the rest
template <typename F>
int launch_stream(const typename F::Params& p, int nb, int64_t n, void* stream) {
    int64_t gx = (n / F::V + 255) / 256;
    int cap = (2048 + nb - 1) / nb; if (cap < 1) cap = 1;
    if (gx > cap) gx = cap; if (gx < 1) gx = 1;
    hipLaunchKernelGGL(stream_kernel<F>, dim3((unsigned)gx, nb), dim3(256), 0, (hipStream_t)stream, p, n);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

template <bool EULER>
int launch_step(const CsStepArgs* a, void* stream) {
    bool empty;
    if (int rc = refuse_common(a, &empty)) return rc;
    if (!empty && (!a->x || !a->eps_text || !a->x_out)) CS_FAIL(CS_E_ARG, "x, eps_text and x_out are required");
    if (a->order_dim < 1 || a->order_dim > CS_MAX_ORDER) CS_FAIL(CS_E_ARG, "order_dim %d out of range [1,%d]", a->order_dim, CS_MAX_ORDER);
    if (a->scaler_dim < 0 || a->scaler_dim > 2) CS_FAIL(CS_E_UNSUPPORTED, "scaler_dim %d > 2 is not implemented (scheduler_ppo.py:280)", a->scaler_dim);
    if (a->m < 1 || a->m > a->order_dim) CS_FAIL(CS_E_ARG, "history length m=%d not in [1, order_dim=%d]", a->m, a->order_dim);
    if (empty) return CS_OK;
    if ((a->m > 1 || a->scaler_dim > 0) && !a->actions) CS_FAIL(CS_E_ARG, "actions required when m > 1 or scaler_dim > 0");
    if (a->actions && a->actions_stride < a->order_dim + a->scaler_dim - 1) CS_FAIL(CS_E_SHAPE, "actions_stride %d < order+scaler-1", a->actions_stride);
    if (a->eps_uncond && !a->eps_out) CS_FAIL(CS_E_ARG, "eps_out is required with CFG (the combined eps is the history entry)");
    for (int k = 0; k < a->m - 1; ++k)
        if (!a->hist[k]) CS_FAIL(CS_E_ARG, "hist[%d] is NULL but m=%d", k, a->m);
    StepParams p;
    p.x = a->x; p.ec = a->eps_text; p.eu = a->eps_uncond; p.g = a->guidance;
    for (int k = 0; k < CS_MAX_ORDER; ++k) p.hist[k] = a->hist[k];
    p.m = a->m; p.order = a->order_dim; p.scaler = a->scaler_dim;
    p.actions = a->actions; p.astride = a->actions_stride;
    p.x_out = a->x_out; p.eps_out = a->eps_out;
    p.sat = a->sqrt_at; p.s1mat = a->sqrt_1mat; p.sap = a->sqrt_ap; p.s1map = a->sqrt_1map;
    p.vpred = a->v_prediction; p.dt = a->dt;
    p.x_lp = a->x_out_lp; p.lp_bf16 = a->lp_dtype == CS_BF16;
    return with_step_dtypes(a->io_dtype, x_f32(a), a->out_dtype == CS_F32, [&](auto ti, auto tx, auto to) {
        return launch_stream<LmsStep<TYPE_OF(ti), TYPE_OF(tx), TYPE_OF(to), EULER>>(p, a->B, a->elems, stream);
    });
}

int launch_dpm_step(const CsDpmStepArgs* a, void* stream) {
    bool empty;
    if (int rc = refuse_common(a, &empty)) return rc;
    if (!empty && (!a->x || !a->eps_text || !a->x_out)) CS_FAIL(CS_E_ARG, "x, eps_text and x_out are required");
    if (x_f32(a) && a->out_dtype != CS_F32) CS_FAIL(CS_E_DTYPE, "an fp32 sample gives an fp32 result (out_dtype %d)", a->out_dtype);
    if (empty) return CS_OK;
    const bool identity = (a->conv_x == 0.f && a->conv_e == 1.f);
    if ((a->eps_uncond || !identity) && !a->m_out)
        CS_FAIL(CS_E_ARG, "m_out is required with CFG or a model-output conversion (the converted output is the history entry)");
    DpmParams p;
    p.x = a->x; p.ec = a->eps_text; p.eu = a->eps_uncond; p.g = a->guidance;
    p.m1 = a->m_prev;
    p.x_out = a->x_out; p.m_out = a->m_out;
    p.conv_x = a->conv_x; p.conv_e = a->conv_e; p.cx = a->cx; p.c0 = a->c0; p.c1 = a->c1;
    p.x_lp = a->x_out_lp; p.lp_bf16 = a->lp_dtype == CS_BF16;
    // per sample like launch_step, so a ragged b * elems is accepted and no alignment is checked
    return with_step_dtypes(a->io_dtype, x_f32(a), a->out_dtype == CS_F32, [&](auto ti, auto tx, auto to) {
        return launch_stream<DpmStep<TYPE_OF(ti), TYPE_OF(tx), TYPE_OF(to)>>(p, a->B, a->elems, stream);
    });
}

int launch_lin_step(const CsLinStepArgs* a, void* stream) {
    bool empty;
    if (int rc = refuse_common(a, &empty)) return rc;
    if (!empty && (!a->x || !a->eps_text || !a->x_out)) CS_FAIL(CS_E_ARG, "x, eps_text and x_out are required");
    const int io = a->io_dtype, od = a->out_dtype;
    if (a->x_is_f32 && io == CS_F32) CS_FAIL(CS_E_DTYPE, "x_is_f32 marks an fp32 sample beside 16-bit model outputs (io_dtype %d is fp32 already)", io);
    if (x_f32(a) && od != CS_F32) CS_FAIL(CS_E_DTYPE, "an fp32 sample gives an fp32 result (out_dtype %d)", od);
    if (a->terms < 1 || a->terms > CS_LIN_MAX_TERMS) CS_FAIL(CS_E_ARG, "terms %d out of range [1,%d]", a->terms, CS_LIN_MAX_TERMS);
    if (empty) return CS_OK;
    for (int k = 0; k < a->terms - 1; ++k)
        if (!a->hist[k]) CS_FAIL(CS_E_ARG, "hist[%d] is NULL but terms=%d", k, a->terms);
    const bool identity = (a->conv_x == 0.f && a->conv_e == 1.f);
    if ((a->eps_uncond || !identity) && !a->m_out)
        CS_FAIL(CS_E_ARG, "m_out is required with CFG or a model-output conversion (the converted output is the history entry)");
    LinParams p;
    p.x = a->x; p.ec = a->eps_text; p.eu = a->eps_uncond; p.g = a->guidance;
    p.xb = a->x_base;
    // a history tensor is read only where a term uses it
    for (int k = 0; k < CS_LIN_MAX_TERMS - 1; ++k) p.hist[k] = k < a->terms - 1 ? a->hist[k] : nullptr;
    p.terms = a->terms; p.convert = !identity;
    p.x_out = a->x_out; p.m_out = a->m_out;
    p.conv_x = a->conv_x; p.conv_e = a->conv_e; p.cx = a->cx;
    for (int k = 0; k < CS_LIN_MAX_TERMS; ++k) p.c[k] = a->c[k];
    p.x_lp = a->x_out_lp; p.lp_bf16 = a->lp_dtype == CS_BF16;
    uintptr_t bits = (uintptr_t)a->x | (uintptr_t)a->x_base | (uintptr_t)a->eps_text | (uintptr_t)a->eps_uncond | (uintptr_t)a->x_out | (uintptr_t)a->m_out;
    bool out_aliased = a->x_out == a->x || a->x_out == a->x_base || a->x_out == a->eps_text || a->x_out == a->eps_uncond, m_aliased = false;
    for (int k = 0; k < a->terms - 1; ++k) {
        bits |= (uintptr_t)p.hist[k];
        out_aliased = out_aliased || a->x_out == p.hist[k];
        m_aliased = m_aliased || (a->m_out && a->m_out == p.hist[k]);
    }
    if (out_aliased) CS_FAIL(CS_E_ARG, "x_out aliases an input");
    if (m_aliased) CS_FAIL(CS_E_ARG, "m_out aliases a history entry that this step reads");
    // 16-byte loads / stores on every tensor (two per lane on an fp32 state next to 16-bit outputs; the 16-bit copy of a 4-wide fp32 result is 8 bytes)
    if ((bits & 15) || ((uintptr_t)a->x_out_lp & (io == CS_F32 ? 7 : 15)))
        CS_FAIL(CS_E_ARG, "x, x_base, eps_*, hist, m_out, x_out and x_out_lp must be 16-byte aligned");
    return with_step_dtypes(io, x_f32(a), od == CS_F32, [&](auto ti, auto tx, auto to) {
        return launch_stream<LinStep<TYPE_OF(ti), TYPE_OF(tx), TYPE_OF(to)>>(p, 1, (int64_t)a->B * a->elems, stream);
    });
}

int launch_unipc_step(const CsUnipcStepArgs* a, void* stream) {
    bool empty;
    if (int rc = refuse_common(a, &empty)) return rc;
    if (!empty && (!a->x || !a->eps_text || !a->x_out || !a->m_out)) CS_FAIL(CS_E_ARG, "x, eps_text, x_out and m_out are required");
    const int io = a->io_dtype, od = a->out_dtype;
    if (a->x_is_f32 && io == CS_F32) CS_FAIL(CS_E_DTYPE, "x_is_f32 marks an fp32 sample beside 16-bit model outputs (io_dtype %d is fp32 already)", io);
    // x_c has the sample's dtype (it is the next step's x_last), so the result dtype is the sample's
    if ((a->x_is_f32 != 0) != (io != CS_F32 && od == CS_F32)) CS_FAIL(CS_E_DTYPE, "out_dtype %d is not the sample's dtype (x_is_f32 = %d, io_dtype %d)", od, a->x_is_f32, io);
    if (empty) return CS_OK;
    if (a->use_corr && !a->x_last) CS_FAIL(CS_E_ARG, "x_last is required with the corrector");
    if (((a->use_corr && a->a_0 != 0.f) || a->p_1 != 0.f) && !a->m_prev0) CS_FAIL(CS_E_ARG, "m_prev0 is NULL but a_0 or p_1 is not zero");
    if (a->use_corr && a->a_1 != 0.f && !a->m_prev1) CS_FAIL(CS_E_ARG, "m_prev1 is NULL but a_1 is not zero");
    UnipcParams p;
    p.x = a->x; p.ec = a->eps_text; p.eu = a->eps_uncond; p.g = a->guidance;
    p.corr = a->use_corr != 0;
    p.x_last = p.corr ? a->x_last : nullptr;
    // a history tensor is read only where a coefficient uses it
    p.m0 = ((p.corr && a->a_0 != 0.f) || a->p_1 != 0.f) ? a->m_prev0 : nullptr;
    p.m1 = (p.corr && a->a_1 != 0.f) ? a->m_prev1 : nullptr;
    p.x_out = a->x_out; p.m_out = a->m_out; p.x_last_out = a->x_last_out;
    p.conv_x = a->conv_x; p.conv_e = a->conv_e;
    p.a_x = a->a_x; p.a_0 = a->a_0; p.a_1 = a->a_1; p.a_n = a->a_n; p.p_x = a->p_x; p.p_0 = a->p_0; p.p_1 = a->p_1;
    p.x_lp = a->x_out_lp; p.lp_bf16 = a->lp_dtype == CS_BF16;
    // 16-byte loads / stores on every tensor (two per lane on an fp32 state next to 16-bit outputs; the 16-bit copy of a 4-wide fp32 result is 8 bytes)
    if ((((uintptr_t)a->eps_text | (uintptr_t)a->eps_uncond | (uintptr_t)p.m0 | (uintptr_t)p.m1 | (uintptr_t)a->m_out | (uintptr_t)a->x | (uintptr_t)p.x_last |
          (uintptr_t)a->x_out | (uintptr_t)a->x_last_out) & 15) || ((uintptr_t)a->x_out_lp & (a->x_is_f32 ? 15 : 7)))
        CS_FAIL(CS_E_ARG, "x, x_last, eps_*, m_prev*, m_out, x_out, x_last_out and x_out_lp must be 16-byte aligned");
    return with_step_dtypes(io, false, od == CS_F32, [&](auto ti, auto, auto to) {      // (the sample's dtype is the result's: checked above)
        return launch_stream<UnipcStep<TYPE_OF(ti), TYPE_OF(to)>>(p, 1, (int64_t)a->B * a->elems, stream);
    });
}

int launch_fm_step(const CsFmStepArgs* a, void* stream) {
    bool empty;
    if (int rc = refuse_common(a, &empty)) return rc;
    if (!empty && (!a->x_base || !a->v2 || !a->x_out)) CS_FAIL(CS_E_ARG, "x_base, v2 and x_out are required");
    if (empty) return CS_OK;
    const int io = a->io_dtype, od = a->out_dtype;
    const FmParams p{a->x_base, a->v2, a->v1, a->c, a->x_out};
    // 16-byte loads / stores on the model outputs; an fp32 base or result beside them needs its element's 4 bytes only (the hardware splits a
    // 16-byte access that is not aligned, as it does for the samples of a ragged per-sample launch)
    if ((((uintptr_t)a->v2 | (uintptr_t)a->v1) & 15) || ((uintptr_t)a->x_base & (x_f32(a) ? 3 : 15)) || ((uintptr_t)a->x_out & (io != CS_F32 && od == CS_F32 ? 3 : 15)))
        CS_FAIL(CS_E_ARG, "x_base, v1, v2 and x_out must be 16-byte aligned");
    return with_step_dtypes(io, x_f32(a), od == CS_F32, [&](auto ti, auto tx, auto to) {
        return launch_stream<FmStep<TYPE_OF(ti), TYPE_OF(tx), TYPE_OF(to)>>(p, 1, (int64_t)a->B * a->elems, stream);
    });
}

int launch_true_cfg(const void* pos, const void* neg, int in_dtype, float scale, void* out, int out_dtype, int64_t n, void* stream) {
    if (n < 0) CS_FAIL(CS_E_SHAPE, "negative length");
    const bool pair_ok = (in_dtype == CS_F32 && (out_dtype == CS_F32 || out_dtype == CS_F16 || out_dtype == CS_BF16)) ||
                         ((in_dtype == CS_F16 || in_dtype == CS_BF16) && out_dtype == in_dtype);
    if (!pair_ok) CS_FAIL(CS_E_DTYPE, "unsupported in/out dtype pair (%d,%d)", in_dtype, out_dtype);
    if (n == 0) return CS_OK;
    if (!pos || !neg || !out) CS_FAIL(CS_E_ARG, "pos, neg and out are required");
    const bool mixed = in_dtype == CS_F32 && out_dtype != CS_F32;
    // one 16-byte load / store per lane and tensor; the fp32 side of a mixed pair needs its element's 4 bytes only (launch_fm_step's rule)
    if ((((uintptr_t)pos | (uintptr_t)neg) & (mixed ? 3 : 15)) || ((uintptr_t)out & 15))
        CS_FAIL(CS_E_ARG, "pos, neg and out must be 16-byte aligned (fp32 inputs beside a 16-bit output: 4-byte)");
    if (mixed && (out == pos || out == neg)) CS_FAIL(CS_E_ARG, "out may alias pos or neg only when the element sizes are equal");
    const CfgParams p{pos, neg, out, scale};
    return with_dtype(out_dtype, [&](auto to) {
        if (in_dtype == CS_F32) return launch_stream<TrueCfg<float, TYPE_OF(to)>>(p, 1, n, stream);
        return launch_stream<TrueCfg<TYPE_OF(to), TYPE_OF(to)>>(p, 1, n, stream);
    });
}

// ---------------------------------------------------------------- policy MLP
// one workgroup per DISTINCT conditioning row; weights (<= ~1 MB) stay in L2.  When one row is
// broadcast to all B samples (x_row_stride == 0, no cosine features: every sampling step), a single
// workgroup evaluates the MLP once and writes the B identical probability rows.  Each wave keeps
// RW weight rows in flight (one 16-byte load per lane and row when hidden % 4 == 0) so the layer is
// a few L2 round trips instead of hidden / waves dependent ones.
template <int RW>
__device__ __forceinline__ void dense_rows(const float* __restrict__ w, const float* __restrict__ bias, const float* in_lds,
                                           float* out_lds, int rows, int K, int wave, int nw, int lane, bool relu, float post) {
    const bool vec = (K & 3) == 0 && ((uintptr_t)w & 15) == 0;
    for (int j0 = wave * RW; j0 < rows; j0 += nw * RW) {
        float acc[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[r] = 0.f;
        if (vec) {
            for (int k = lane * 4; k < K; k += 256) {
                f32x4 wv[RW];
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const int j = j0 + r < rows ? j0 + r : rows - 1;
                    wv[r] = *reinterpret_cast<const f32x4*>(w + (int64_t)j * K + k);
                }
                const f32x4 xv = *reinterpret_cast<const f32x4*>(in_lds + k);
#pragma unroll
                for (int r = 0; r < RW; ++r) acc[r] += xv[0] * wv[r][0] + xv[1] * wv[r][1] + xv[2] * wv[r][2] + xv[3] * wv[r][3];
            }
        } else {
            for (int k = lane; k < K; k += 64) {
                const float xv = in_lds[k];
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                    const int j = j0 + r < rows ? j0 + r : rows - 1;
                    acc[r] += xv * w[(int64_t)j * K + k];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == 0 && j0 + r < rows) {
                const float o = (v + bias[j0 + r]) * post;
                out_lds[j0 + r] = relu ? fmaxf(o, 0.f) : o;
            }
        }
    }
}

__global__ __launch_bounds__(1024) void factor_probs_kernel(CsFactorNet n, const float* x, int xstride, const float* cosf, float* probs,
                                                            int rows_out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* in = sm;                               // [in_dim] (<= 16)
    float* h0 = sm + 16;                          // [H] (padded to a multiple of 4)
    const int Hp = (n.hidden + 3) & ~3;
    float* h1 = h0 + Hp;                          // [H]
    float* lg = h1 + Hp;                          // [A*K] logits, then probabilities
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    if (tid < n.in_dim) in[tid] = (tid < 2) ? x[(int64_t)b * xstride + tid] * n.input_scale
                                            : cosf[(int64_t)b * (n.in_dim - 2) + tid - 2];
    __syncthreads();
    for (int j = tid; j < n.hidden; j += blockDim.x) {
        float acc = 0.f;
        for (int k = 0; k < n.in_dim; ++k) acc += in[k] * n.w0[j * n.in_dim + k];
        h0[j] = fmaxf(acc + n.b0[j], 0.f);
    }
    __syncthreads();
    dense_rows<8>(n.w1, n.b1, h0, h1, n.hidden, n.hidden, wave, nw, lane, true, 1.f);
    __syncthreads();
    const int AK = n.action_dims * n.num_actions;
    dense_rows<4>(n.w2, n.b2, h1, lg, AK, n.hidden, wave, nw, lane, false, n.inv_temperature);
    __syncthreads();
    for (int a = wave; a < n.action_dims; a += nw) {
        float* row = lg + a * n.num_actions;
        float mx = -INFINITY;
        for (int k = lane; k < n.num_actions; k += 64) mx = fmaxf(mx, row[k]);
        mx = wave_max(mx);
        float s = 0.f;
        for (int k = lane; k < n.num_actions; k += 64) s += expf(row[k] - mx);
        s = wave_sum(s);
        for (int k = lane; k < n.num_actions; k += 64) row[k] = expf(row[k] - mx) / s;
    }
    __syncthreads();
    // rows_out == 1: this workgroup's own row; > 1: the broadcast row written to every sample
    float* out = probs + (int64_t)b * AK;
    for (int r = wave; r < rows_out; r += nw)
        for (int k = lane; k < AK; k += 64) out[(int64_t)r * AK + k] = lg[k];
}

struct HistPtrs { const void* p[CS_MAX_ORDER]; };

// CFG form (eu != null): hist[0] is the TEXT branch and the newest history entry is the combined eps u + g (c - u), rounded to
// the model dtype exactly as the update kernels round it (cfg_combine); it is formed on the fly and the blocks of feature 1 also write it to
// eps_out (every launch has them, whatever m is), so the update kernel that follows takes it as an already combined eps.
// W elements at t of a thread's three partial sums; hi == nullptr: feature i is not formed (i >= m), only the combined eps is written
template <typename T, int W>
__device__ __forceinline__ void cosine_acc(const void* h0, const void* hi, const void* eu, float g, void* eps_out, int64_t t, float& dot, float& na, float& nb) {
    Raw<T, W> rc, ru, ra;
    rc.load(h0, t);
    if (eu) ru.load(eu, t);
    if (hi) ra.load(hi, t);
    float a[W], c[W], u[W];
    rc.unpack(c);
    if (eu) {
        ru.unpack(u);
        cfg_combine<T>(c, u, g);
        if (eps_out) store<T, W>(eps_out, t, c);
    }
    if (hi) {
        ra.unpack(a);
#pragma unroll
        for (int j = 0; j < W; ++j) { dot += a[j] * c[j]; na += a[j] * a[j]; nb += c[j] * c[j]; }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cosine_kernel(HistPtrs h, int m, int order, int64_t elems, float* out, const void* eu, float g, void* eps_out) {
    // grid (order-1, B): cos(hist[i], hist[0]), i = blockIdx.x + 1
    const int i = blockIdx.x + 1, b = blockIdx.y;
    __shared__ float red[3][4];
    float dot = 0.f, na = 0.f, nb = 0.f;
    const bool writer = eps_out != nullptr && i == 1;
    if (i < m || writer) {
        constexpr int V = Io<T>::VEC;
        const int64_t base = (int64_t)b * elems, nvec = elems / V;
        const void* hi = i < m ? h.p[i] : nullptr;
        void* eo = writer ? eps_out : nullptr;
        for (int64_t v = threadIdx.x; v < nvec; v += blockDim.x) cosine_acc<T, V>(h.p[0], hi, eu, g, eo, base + v * V, dot, na, nb);
        for (int64_t t = nvec * V + threadIdx.x; t < elems; t += blockDim.x) cosine_acc<T, 1>(h.p[0], hi, eu, g, eo, base + t, dot, na, nb);
    }
    dot = wave_sum(dot); na = wave_sum(na); nb = wave_sum(nb);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = dot; red[1][wave] = na; red[2][wave] = nb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float d = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        float a = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        float c = red[2][0] + red[2][1] + red[2][2] + red[2][3];
        float r = 0.f;
        if (i < m) r = d / (fmaxf(sqrtf(a), 1e-8f) * fmaxf(sqrtf(c), 1e-8f));
        out[(int64_t)b * (order - 1) + (i - 1)] = r;
    }
}

__global__ void sample_kernel(const float* probs, const float* uni, const int64_t* idx_in, const float* av,
                              int B, int A, int K, int64_t* idx, float* actions, float* aprobs) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * A) return;
    const int a = t % A;
    const float* p = probs + (int64_t)t * K;
    int k;
    if (idx_in) {
        k = (int)idx_in[t];
        k = k < 0 ? 0 : (k >= K ? K - 1 : k);
    } else {
        const float u = uni[t];
        float c = 0.f; k = K - 1;
        for (int j = 0; j < K; ++j) { c += p[j]; if (u < c) { k = j; break; } }
        // never return a zero-probability bin because of rounding at the tail
        while (k > 0 && p[k] <= 0.f) --k;
    }
    if (idx) idx[t] = k;
    if (actions) actions[t] = av[a * K + k];
    if (aprobs) aprobs[t] = p[k];
}

__global__ void action_probs_kernel(const float* probs, const float* actions, const float* av, int B, int A, int K,
                                    float* sel, float* ent) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * A) return;
    const int a = t % A;
    const float* p = probs + (int64_t)t * K;
    const float act = actions[t];
    int best = 0; float bd = fabsf(act - av[a * K]);
    float s = 0.f;
    for (int j = 0; j < K; ++j) {
        float d = fabsf(act - av[a * K + j]);
        if (d < bd) { bd = d; best = j; }
        s += p[j];
    }
    float h = 0.f;
    // torch.distributions.Categorical(probs=p).entropy(): -sum q log(clamp(q, eps, 1 - eps)) with q = p / sum p
    // (the same clamp the PPO gradient kernel differentiates, ppo.hip policy_row_kernel)
    for (int j = 0; j < K; ++j) { float q = p[j] / s; h -= q * logf(fminf(fmaxf(q, 1.1920929e-07f), 1.f - 1.1920929e-07f)); }
    if (sel) sel[t] = p[best];
    if (ent) ent[t] = h / logf((float)K);
}

__global__ void masks_kernel(int B, int A, int m, int order, float* masks) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * A) return;
    const int a = t % A;
    masks[t] = (a >= m - 1 && a < order - 1) ? 0.f : 1.f;
}

// W elements of plane k of the stacked history: a copy of hist[k], zeros where src == nullptr (k >= m)
template <typename T, int W>
__device__ __forceinline__ void stack_copy(const void* src, int64_t s, void* out, int64_t d) {
    Raw<T, W> r = {};
    if (src) r.load(src, s);
    float a[W];
    r.unpack(a);
    store<T, W>(out, d, a);
}

template <typename T>
__global__ __launch_bounds__(256) void stack_kernel(HistPtrs h, int m, int order, int64_t elems, void* out) {
    // grid (chunks, order, B)
    const int k = blockIdx.y, b = blockIdx.z;
    constexpr int V = Io<T>::VEC;
    const int64_t nvec = elems / V;
    const int64_t src = (int64_t)b * elems, dst = ((int64_t)b * order + k) * elems;
    const void* hk = k < m ? h.p[k] : nullptr;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x)
        stack_copy<T, V>(hk, src + v * V, out, dst + v * V);
    if (blockIdx.x == 0)
        for (int64_t t = nvec * V + threadIdx.x; t < elems; t += blockDim.x) stack_copy<T, 1>(hk, src + t, out, dst + t);
}

}  // namespace

extern "C" {

int cs_lms_ddim_step(const CsStepArgs* args, void* stream) { return launch_step<false>(args, stream); }
int cs_lms_euler_step(const CsStepArgs* args, void* stream) { return launch_step<true>(args, stream); }
int cs_dpm_multistep_step(const CsDpmStepArgs* args, void* stream) { return launch_dpm_step(args, stream); }
int cs_unipc_step(const CsUnipcStepArgs* args, void* stream) { return launch_unipc_step(args, stream); }
int cs_linear_step(const CsLinStepArgs* args, void* stream) { return launch_lin_step(args, stream); }
int cs_fm_general_step(const CsFmStepArgs* args, void* stream) { return launch_fm_step(args, stream); }
int cs_true_cfg_combine(const void* pos, const void* neg, int in_dtype, float scale, void* out, int out_dtype, int64_t n, void* stream) {
    return launch_true_cfg(pos, neg, in_dtype, scale, out, out_dtype, n, stream);
}

int cs_factor_probs(const CsFactorNet* n, const float* x, int x_row_stride, const float* cos_feat, int B, float* probs, void* stream) {
    if (!n) CS_FAIL(CS_E_ARG, "net is NULL");
    if (B < 0) CS_FAIL(CS_E_SHAPE, "negative batch");
    if (B == 0) return CS_OK;
    if (!x || !probs) CS_FAIL(CS_E_ARG, "x and probs are required");
    if (!n->w0 || !n->b0 || !n->w1 || !n->b1 || !n->w2 || !n->b2) CS_FAIL(CS_E_ARG, "missing weight pointer");
    if (n->in_dim < 2 || n->in_dim > 16) CS_FAIL(CS_E_SHAPE, "in_dim %d not in [2,16]", n->in_dim);
    if (n->hidden < 1 || n->hidden > 1024) CS_FAIL(CS_E_SHAPE, "hidden %d not in [1,1024]", n->hidden);
    if (n->action_dims < 1 || n->action_dims > CS_MAX_ACTION_DIMS) CS_FAIL(CS_E_SHAPE, "action_dims %d out of range", n->action_dims);
    if (n->num_actions < 1 || n->num_actions > 1024) CS_FAIL(CS_E_SHAPE, "num_actions %d out of range", n->num_actions);
    if (n->in_dim > 2 && !cos_feat) CS_FAIL(CS_E_ARG, "use_conv=True requires epsilon (factor_net_ppo.py:109-110)");
    const size_t Hp = ((size_t)n->hidden + 3) & ~(size_t)3;
    size_t lds = (16 + 2 * Hp + (size_t)n->action_dims * n->num_actions) * sizeof(float);
    if (lds > 64 * 1024) CS_FAIL(CS_E_SHAPE, "policy net too large for one workgroup (%zu B LDS)", lds);
    // one broadcast conditioning row and no per-sample features: evaluate once, write B rows
    const bool bcast = (x_row_stride == 0 && n->in_dim == 2 && B > 1);
    const int threads = n->hidden >= 128 ? 1024 : 256;
    hipLaunchKernelGGL(factor_probs_kernel, dim3(bcast ? 1 : B), dim3(threads), lds, (hipStream_t)stream, *n, x,
                       x_row_stride, cos_feat, probs, bcast ? B : 1);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int cs_cosine_features_cfg(const void* const* hist, int m, int order, int B, int64_t elems, int dtype, const void* eps_uncond, float guidance,
                           void* eps_out, float* out, void* stream) {
    if (B <= 0 || elems <= 0) return B < 0 || elems < 0 ? CS_E_SHAPE : CS_OK;
    if (!hist || !out) CS_FAIL(CS_E_ARG, "use_conv=True requires epsilon (factor_net_ppo.py:109-110)");
    if (order < 2 || order > CS_MAX_ORDER || m < 1 || m > order) CS_FAIL(CS_E_ARG, "bad order/m (%d,%d)", order, m);
    if (eps_uncond && !eps_out) CS_FAIL(CS_E_ARG, "eps_out is required with eps_uncond (the combined eps is the history entry)");
    if (!eps_uncond && eps_out) CS_FAIL(CS_E_ARG, "eps_out without eps_uncond");
    HistPtrs h;
    for (int k = 0; k < CS_MAX_ORDER; ++k) h.p[k] = (k < m) ? hist[k] : nullptr;
    for (int k = 0; k < m; ++k) if (!h.p[k]) CS_FAIL(CS_E_ARG, "hist[%d] is NULL", k);
    dim3 grid(order - 1, B), block(256);
    hipStream_t s = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) -> int {
        hipLaunchKernelGGL(cosine_kernel<TYPE_OF(t)>, grid, block, 0, s, h, m, order, elems, out, eps_uncond, guidance, eps_out);
        CS_CHECK_LAUNCH();
        return CS_OK;
    });
}

int cs_cosine_features(const void* const* hist, int m, int order, int B, int64_t elems, int dtype, float* out, void* stream) {
    return cs_cosine_features_cfg(hist, m, order, B, elems, dtype, nullptr, 0.f, nullptr, out, stream);
}

static int launch_sample(const float* probs, const float* uni, const int64_t* idx_in, const float* av, int B, int A, int K,
                         int64_t* idx, float* actions, float* aprobs, void* stream) {
    if (B < 0 || A < 1 || K < 1) CS_FAIL(CS_E_SHAPE, "bad shape B=%d A=%d K=%d", B, A, K);
    if (B == 0) return CS_OK;
    if (!probs || !av) CS_FAIL(CS_E_ARG, "probs and action_values are required");
    int n = B * A;
    hipLaunchKernelGGL(sample_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, probs, uni, idx_in, av, B, A, K, idx, actions, aprobs);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int cs_sample_actions(const float* probs, const float* uniforms, const float* action_values, int B, int A, int K,
                      int64_t* idx, float* actions, float* action_probs, void* stream) {
    if (B > 0 && !uniforms) CS_FAIL(CS_E_ARG, "uniforms is NULL");
    return launch_sample(probs, uniforms, nullptr, action_values, B, A, K, idx, actions, action_probs, stream);
}

int cs_gather_actions(const float* probs, const int64_t* idx, const float* action_values, int B, int A, int K,
                      float* actions, float* action_probs, void* stream) {
    if (B > 0 && !idx) CS_FAIL(CS_E_ARG, "idx is NULL");
    return launch_sample(probs, nullptr, idx, action_values, B, A, K, nullptr, actions, action_probs, stream);
}

int cs_action_probs(const float* probs, const float* actions, const float* action_values, int B, int A, int K,
                    float* selected, float* entropy, void* stream) {
    if (B < 0 || A < 1 || K < 1) CS_FAIL(CS_E_SHAPE, "bad shape");
    if (B == 0) return CS_OK;
    if (!probs || !actions || !action_values) CS_FAIL(CS_E_ARG, "probs, actions and action_values are required");
    int n = B * A;
    hipLaunchKernelGGL(action_probs_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, probs, actions, action_values, B, A, K, selected, entropy);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int cs_step_masks(int B, int A, int m, int order, float* masks, void* stream) {
    if (B < 0 || A < 1) CS_FAIL(CS_E_SHAPE, "bad shape");
    if (B == 0) return CS_OK;
    if (!masks) CS_FAIL(CS_E_ARG, "masks is NULL");
    int n = B * A;
    hipLaunchKernelGGL(masks_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, B, A, m, order, masks);
    CS_CHECK_LAUNCH();
    return CS_OK;
}

int cs_stack_history(const void* const* hist, int m, int order, int B, int64_t elems, int dtype, void* out, void* stream) {
    if (B <= 0 || elems <= 0) return B < 0 || elems < 0 ? CS_E_SHAPE : CS_OK;
    if (!hist || !out) CS_FAIL(CS_E_ARG, "hist and out are required");
    if (order < 1 || order > CS_MAX_ORDER || m < 0 || m > order) CS_FAIL(CS_E_ARG, "bad order/m");
    HistPtrs h;
    for (int k = 0; k < CS_MAX_ORDER; ++k) h.p[k] = (k < m) ? hist[k] : nullptr;
    const int vec = dtype == CS_F32 ? 4 : 8;
    int gx = (int)((elems / vec + 255) / 256); if (gx < 1) gx = 1; if (gx > 64) gx = 64;
    dim3 grid(gx, order, B), block(256);
    hipStream_t s = (hipStream_t)stream;
    return with_dtype(dtype, [&](auto t) -> int {
        hipLaunchKernelGGL(stack_kernel<TYPE_OF(t)>, grid, block, 0, s, h, m, order, elems, out);
        CS_CHECK_LAUNCH();
        return CS_OK;
    });
}

}  // extern "C"
