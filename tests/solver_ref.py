"""CPU references, case lists and seeded inputs for consolver_amd/csrc/solver.hip (tests/test_solver_forms_gpu.py runs the kernels on them; tests/test_solver_ref.py
checks this module on the CPU, on the same inputs).

Two forms of every streaming kernel (lms = cs_lms_ddim_step / cs_lms_euler_step, dpm, unipc, fm), over inputs that are representable in the io dtype:

``*_exact``   the kernel's operation order in numpy fp32: one fp32 operation or one round-to-nearest-even conversion per step, scalars rounded to fp32 first (what
              ``ctypes.c_float`` does).  solver.hip is built with -ffp-contract=off, so the GPU is expected to give the same bits.  Coefficient fix-up, combine,
              CFG and the conversions are ``oracle.solver_oracle``'s (coefficients, lms_combine, cfg_combine, round_like); the DDIM / Euler epilogues are written
              out here because the kernel takes the four square roots / dt as arguments (test_solver_ref.py holds them to ddim_update and FMPPOSchedulerOracle).
``*_fp64``    the plain operation in float64 with the documented rounding points applied to the exact values: the CFG combine and the converted model output
              rounded to the io dtype, the UniPC corrector to the state dtype, the 16-bit product (and sum) of the m == 1 Euler / fm form, the result to the
              out dtype (and the 16-bit copy from the fp32 result).  Returns (reference, bound) per output.

The bound (class T).  Every fp32 operation of the path rounds once: its result differs from the exact result of the same operation on the same operands by at most
2^-24 |result| (+ 2^-150 in the subnormal range).  Carrying that forward operation by operation gives, for a value v computed from operands with errors e_a, e_b,
    add / sub:  e = e_a + e_b + 2^-24 |v|          mul:  e = |a| e_b + |b| e_a + e_a e_b + 2^-24 |v|          div:  e = (e_a + |v| e_b) / (|b| - e_b) + 2^-24 |v|
(each incoming error also times 1 + 2^-23 for the second-order term).  Unrolled, that is a sum over the n roundings of the path of 2^-24 times the magnitude of one
partial result, each of which is at most the sum of the absolute values of the terms: never more than n 2^-24 sum |terms|, and tighter where terms are small.
At a rounding point to a 16-bit grid the exact value v and the fp32 value (within e of it) round to the same grid point unless a rounding boundary lies within e of v;
rounding is monotonic, so the error after the point is max(|rnd(v + e) - rnd(v)|, |rnd(v - e) - rnd(v)|): zero for nearly every element, one grid step for the
few next to a tie.  (A bound without this term fails about one fp16 element in 4000; with a whole grid step everywhere it would pass a kernel that skips the
rounding.)  The final rounding is one more such point, and the acceptance adds half an ulp of the out dtype on top.

cosine_kernel and the entropy of action_probs_kernel reduce in an order of their own; `cosine_emulated` / `entropy_emulated` restate that order in fp32
(per-thread strided partial sums, the 6 butterfly steps of wave_sum, the 4 waves added left to right; the sequential loop of action_probs_kernel) so that
`cosine_bound` / `entropy_bound` are proven on the CPU before the GPU is held to them:

cosine:  |got - ref| <= (2 k + 4) 2^-24,  k = V ceil(nvec / 256) + (1 if elems % V else 0) + 10.  Each of the three sums (dot, |a|^2, |c|^2) is a sum of products
         in which one value passes through at most k roundings (V per pass of the thread's loop and one product rounding folded in, one for the tail element, 6
         butterfly steps, 3 wave additions, rounded up to 10): relative error k 2^-24 against the sum of |terms|, which for the norms is the sum itself and for the
         dot is at most |a||c| by Cauchy-Schwarz, i.e. at most 1 in units of the result.  Numerator k, denominator 2 x k / 2 through the square roots, and sqrt,
         max, multiply and divide round once each: (2 k + 4) 2^-24.  Loose on purpose; the exact-valued cases (0, 1) are what catch a dropped element.
entropy: |got - ref| <= ((2 K + 8) H + (K + 2)) 2^-24 / ln K + 2 2^-24 |ref|,  H = sum q |ln q|.  The sum s carries K roundings and the division one, so q is
         off by (K + 1) 2^-24 relative, which moves q ln q by (K + 1) 2^-24 (q |ln q| + q); logf is allowed 2 ulp (an assumption), the product rounds once and
         the K running subtractions round to at most 2^-24 H each partial sum: (2 K + 8) H + (K + 2) sum q, sum q = 1; the division by logf(K) and logf(K)
         itself are the last term.  Largest err / bound measured on an MI355X (gfx950): 0.122 (K = 11; 0.089 at K = 2, 0.022 at K = 161); the CPU emulation
         (numpy's log) gives 0.069 on the same rows.
"""
import math

import numpy as np

from oracle import solver_oracle as so

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
DTYPES = ("f32", "f16", "bf16")
VEC = {"f32": 4, "f16": 8, "bf16": 8}
#           significand bits, exponent of the smallest normal, largest finite
_GRID = {"f32": (24, -126, float(np.finfo(np.float32).max)), "f16": (11, -14, 65504.0), "bf16": (8, -126, float.fromhex("0x1.fep127"))}
CS_E_ARG, CS_E_SHAPE, CS_E_DTYPE = -1, -2, -3


def f32(s):
    return F32(s)


def rnd(x, dt):
    """fp32 -> dt -> fp32, round to nearest even (the oracle's)"""
    with np.errstate(over="ignore"):
        return so.round_like(x, dt)


def spacing(x, dt):
    """distance between neighbouring values of dt's grid at |x| (float64)"""
    p, emin, _ = _GRID[dt]
    _, e = np.frexp(np.abs(np.asarray(x, F64)))                # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - p, emin + 1 - p))


def rnd64(x, dt):
    """float64 -> dt's grid, ONE round to nearest even, as float64 (no pass through fp32)"""
    x = np.asarray(x, F64)
    q = spacing(x, dt)
    r = np.rint(x / q) * q                                     # x / q is exact (a power of two), rint is half-to-even
    return np.where(np.abs(r) > _GRID[dt][2], np.copysign(np.inf, r), r)


# ----------------------------------------------------------------------------------------------------------------- error-carrying float64
class T:
    """a float64 value of the exact operation and a bound on |fp32 kernel value - v| (module docstring)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, F64), np.asarray(e, F64)

    @staticmethod
    def _fl(v, e):
        """the error after the operation's own rounding; with exact operands (e == 0) the kernel value IS fp32(v), so the error is known exactly -- zero when
        the result fits fp32, as the CFG combine of short 16-bit values with g = 7.5 mostly does: its many exact ties round the same way on both sides"""
        with np.errstate(over="ignore", invalid="ignore"):
            own = np.abs(v.astype(F32).astype(F64) - v)
        return np.where(e == 0, np.where(np.isfinite(own), own, np.inf), e * (1 + 2 * U) + U * np.abs(v) + 2.0 ** -150)

    def __add__(self, o):
        v = self.v + o.v
        return T(v, T._fl(v, self.e + o.e))

    def __sub__(self, o):
        v = self.v - o.v
        return T(v, T._fl(v, self.e + o.e))

    def __mul__(self, o):
        v = self.v * o.v
        return T(v, T._fl(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e))

    def __truediv__(self, o):
        v = self.v / o.v
        return T(v, T._fl(v, (self.e + np.abs(v) * o.e) / (np.abs(o.v) - o.e)))

    def rnd(self, dt):
        if dt == "f32" and not np.any(self.e):
            return T(rnd64(self.v, dt))
        v = rnd64(self.v, dt)
        with np.errstate(invalid="ignore"):
            e = np.maximum(np.abs(rnd64(self.v + self.e, dt) - v), np.abs(rnd64(self.v - self.e, dt) - v))
        return T(v, np.where(np.isfinite(e), e, np.inf))

    def result(self, dt):
        """(reference, bound) of an output tensor of dtype dt"""
        r = self.rnd(dt)
        return r.v, r.e + 0.5 * spacing(r.v, dt)


def col(a):
    return np.asarray(a, F64)[:, None]


def within(got, ref_bound):
    """worst |got - ref| / bound over the elements (got: anything castable to float64); inf where got is not finite but ref is"""
    ref, bound = ref_bound
    got = np.asarray(got, F64)
    both_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid="ignore"):
        r = np.where(both_inf, 0.0, np.abs(got - ref) / bound)
    return float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0


# ----------------------------------------------------------------------------------------------------------------- lms_step_kernel
def cfg_exact(ec, eu, g, io):
    return ec if eu is None else rnd(so.cfg_combine(eu, ec, f32(g)), io)


def cfg_fp64(ec, eu, g, io):
    if eu is None:
        return T(ec)
    u, c = T(eu), T(ec)
    return (u + T(F64(f32(g))) * (c - u)).rnd(io)


def _actions_or_empty(c):
    return np.zeros((c["B"], 0), F32) if c.get("actions") is None else c["actions"]


def lms_exact(c):
    """c: a case dict of make_lms.  Returns dict(x_out, eps_out?, x_out_lp?) as fp32 arrays holding values of the tensors' dtypes."""
    io, m, order, scaler = c["io"], c["m"], c["order"], c["scaler"]
    x = c["x"]
    e = cfg_exact(c["ec"], c["eu"], c["g"], io)
    coef, scal = so.coefficients(_actions_or_empty(c), m, order, scaler)
    eff = so.lms_combine([e] + c["hist"][:m - 1], coef)
    if scaler >= 1:
        eff = (eff * scal[:, 0:1]).astype(F32)
    if scaler >= 2:
        x = (x * scal[:, 1:2]).astype(F32)
    if c["euler"]:
        dt = f32(c["dt"])
        if m == 1 and scaler == 0:
            r = (x + rnd((rnd(dt, io) * eff).astype(F32), io)).astype(F32)
        else:
            r = (x + (dt * eff).astype(F32)).astype(F32)
    else:
        sat, s1mat, sap, s1map = (f32(v) for v in c["ddim"])
        if c["vpred"]:
            eff = ((sat * eff).astype(F32) + (s1mat * x).astype(F32)).astype(F32)
        x0 = ((x - (s1mat * eff).astype(F32)).astype(F32) / sat).astype(F32)
        r = ((sap * x0).astype(F32) + (s1map * eff).astype(F32)).astype(F32)
    out = dict(x_out=rnd(r, c["out"]))
    if c["eu"] is not None:
        out["eps_out"] = e
    if c["lp"]:
        out["x_out_lp"] = rnd(r, c["lp"])
    return out


def lms_fp64(c):
    io, m, order, scaler = c["io"], c["m"], c["order"], c["scaler"]
    a = _actions_or_empty(c)
    one = T(1.0)
    x = T(c["x"])
    e = cfg_fp64(c["ec"], c["eu"], c["g"], io)
    if m == 1:
        eff = e
    else:
        cs = [T(col(a[:, 0])) + one] + [T(col(a[:, k])) for k in range(1, m - 1)]
        s = T(np.zeros((c["B"], 1)))
        for ck in cs:
            s = s + ck
        cs.append(one - s)
        eff = cs[0] * e
        for k in range(1, m):
            eff = eff + cs[k] * T(c["hist"][k - 1])
    if scaler >= 1:
        eff = eff * (T(col(a[:, order - 1])) + one)
    if scaler >= 2:
        x = x * (T(col(a[:, order])) + one)
    if c["euler"]:
        dt = T(F64(f32(c["dt"])))
        r = x + (dt.rnd(io) * eff).rnd(io) if (m == 1 and scaler == 0) else x + dt * eff
    else:
        sat, s1mat, sap, s1map = (T(F64(f32(v))) for v in c["ddim"])
        if c["vpred"]:
            eff = sat * eff + s1mat * x
        x0 = (x - s1mat * eff) / sat
        r = sap * x0 + s1map * eff
    out = dict(x_out=r.result(c["out"]))
    if c["eu"] is not None:
        out["eps_out"] = (e.v, e.e + 0.5 * spacing(e.v, io))
    if c["lp"]:
        out["x_out_lp"] = r.rnd("f32").result(c["lp"])
    return out


# ----------------------------------------------------------------------------------------------------------------- dpm_step_kernel
def dpm_exact(c):
    io, x = c["io"], c["x"]
    conv_x, conv_e, cx, c0, c1 = (f32(v) for v in c["scal"])
    e = cfg_exact(c["ec"], c["eu"], c["g"], io)
    m0 = rnd(((conv_x * x).astype(F32) + (conv_e * e).astype(F32)).astype(F32), io)
    r = ((cx * x).astype(F32) + (c0 * m0).astype(F32)).astype(F32)
    if c["m1"] is not None:
        r = (r + (c1 * c["m1"]).astype(F32)).astype(F32)
    out = dict(x_out=rnd(r, c["out"]))
    if c["want_m_out"]:
        out["m_out"] = m0
    if c["lp"]:
        out["x_out_lp"] = rnd(r, c["lp"])
    return out


def dpm_fp64(c):
    io, x = c["io"], T(c["x"])
    conv_x, conv_e, cx, c0, c1 = (T(F64(f32(v))) for v in c["scal"])
    e = cfg_fp64(c["ec"], c["eu"], c["g"], io)
    m0 = (conv_x * x + conv_e * e).rnd(io)
    r = cx * x + c0 * m0
    if c["m1"] is not None:
        r = r + c1 * T(c["m1"])
    out = dict(x_out=r.result(c["out"]))
    if c["want_m_out"]:
        out["m_out"] = (m0.v, m0.e + 0.5 * spacing(m0.v, io))
    if c["lp"]:
        out["x_out_lp"] = r.rnd("f32").result(c["lp"])
    return out


# ----------------------------------------------------------------------------------------------------------------- unipc_step_kernel
def _unipc_reads(c):
    """(m0 is read, m1 is read): launch_unipc_step's rule; a history tensor that is not read counts as zero"""
    _, _, (a_x, a_0, a_1, a_n), (p_x, p_0, p_1), corr = c["scal"]
    return (corr and f32(a_0) != 0) or f32(p_1) != 0, corr and f32(a_1) != 0


def unipc_exact(c):
    io, st, x = c["io"], c["out"], c["x"]
    conv_x, conv_e = f32(c["scal"][0]), f32(c["scal"][1])
    a_x, a_0, a_1, a_n = (f32(v) for v in c["scal"][2])
    p_x, p_0, p_1 = (f32(v) for v in c["scal"][3])
    corr = c["scal"][4]
    rd0, rd1 = _unipc_reads(c)
    z = np.zeros_like(x)
    m0, m1, xl = (c["m0"] if rd0 else z), (c["m1"] if rd1 else z), (c["x_last"] if corr else z)
    e = cfg_exact(c["ec"], c["eu"], c["g"], io)
    mn = rnd(((conv_x * x).astype(F32) + (conv_e * e).astype(F32)).astype(F32), io)
    cc = ((a_x * xl).astype(F32) + (a_0 * m0).astype(F32)).astype(F32)
    cc = (cc + (a_1 * m1).astype(F32)).astype(F32)
    cc = rnd((cc + (a_n * mn).astype(F32)).astype(F32), st)
    xc = cc if corr else x
    r = ((p_x * xc).astype(F32) + (p_0 * mn).astype(F32)).astype(F32)
    r = (r + (p_1 * m0).astype(F32)).astype(F32)
    out = dict(x_out=rnd(r, st), m_out=mn)
    if c["want_x_last_out"]:
        out["x_last_out"] = xc
    if c["lp"]:
        out["x_out_lp"] = rnd(r, c["lp"])
    return out


def unipc_fp64(c):
    io, st, x = c["io"], c["out"], T(c["x"])
    conv_x, conv_e = T(F64(f32(c["scal"][0]))), T(F64(f32(c["scal"][1])))
    a_x, a_0, a_1, a_n = (T(F64(f32(v))) for v in c["scal"][2])
    p_x, p_0, p_1 = (T(F64(f32(v))) for v in c["scal"][3])
    corr = c["scal"][4]
    rd0, rd1 = _unipc_reads(c)
    z = np.zeros_like(c["x"])
    m0, m1, xl = T(c["m0"] if rd0 else z), T(c["m1"] if rd1 else z), T(c["x_last"] if corr else z)
    e = cfg_fp64(c["ec"], c["eu"], c["g"], io)
    mn = (conv_x * x + conv_e * e).rnd(io)
    xc = (((a_x * xl + a_0 * m0) + a_1 * m1) + a_n * mn).rnd(st) if corr else x
    r = (p_x * xc + p_0 * mn) + p_1 * m0
    out = dict(x_out=r.result(st), m_out=(mn.v, mn.e + 0.5 * spacing(mn.v, io)))
    if c["want_x_last_out"]:
        out["x_last_out"] = (xc.v, xc.e + 0.5 * spacing(xc.v, st))
    if c["lp"]:
        out["x_out_lp"] = r.rnd("f32").result(c["lp"])
    return out


# ----------------------------------------------------------------------------------------------------------------- fm_step_kernel
def fm_exact(c):
    io = c["io"]
    w = c["v2"] if c["v1"] is None else rnd((c["v1"] + c["v2"]).astype(F32), io)
    r = (c["x"] + rnd((rnd(f32(c["c"]), io) * w).astype(F32), io)).astype(F32)
    return dict(x_out=rnd(r, c["out"]))


def fm_fp64(c):
    io = c["io"]
    w = T(c["v2"]) if c["v1"] is None else (T(c["v1"]) + T(c["v2"])).rnd(io)
    r = T(c["x"]) + (T(F64(f32(c["c"]))).rnd(io) * w).rnd(io)
    return dict(x_out=r.result(c["out"]))


EXACT = dict(lms=lms_exact, dpm=dpm_exact, unipc=unipc_exact, fm=fm_exact)
FP64 = dict(lms=lms_fp64, dpm=dpm_fp64, unipc=unipc_fp64, fm=fm_fp64)


# ----------------------------------------------------------------------------------------------------------------- inputs of the streaming kernels
def _seed(name):
    """a stable integer of a string (hash() is salted per process)"""
    s = 0
    for ch in name:
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def tensor(rng, B, elems, dt, scale=1.0):
    return rnd((rng.standard_normal((B, elems)) * scale).astype(F32), dt)


def actions_for(rng, B, cols, extra=0):
    """distinct per sample, from [-0.5, 0.5]; `extra` further columns hold 1e6 (never read)"""
    a = (rng.permutation(B * max(cols, 1)).reshape(B, max(cols, 1))[:, :cols] / max(B * cols - 1, 1) - 0.5).astype(F32)
    return np.concatenate([a, np.full((B, extra), 1e6, F32)], 1)


def small_shapes(io):
    """tail only; body + tail at both vector widths with samples 1, 2 off vector alignment; no tail, two blocks, the last one partly filled"""
    return [(3, 3 if io == "f32" else 5), (3, 269), (2, 2056)]


def grid_stride_shape(io):
    """cap = ceil(2048 / 64) = 32 blocks per sample and the grid needs 33: the second pass runs once, and there is a tail"""
    return (64, 32773 if io == "f32" else 65549)


FLAT_GRID_STRIDE = (1, 8 * 256 * 2048 + 8 + 5)      # unipc / fm (cap 2048 blocks flat), bf16

# (io, out, x_is_f32, lp)
DTYPE_FORMS = ([("f32", "f32", 0, lp) for lp in (None, "f16", "bf16")] + [("f16", "f16", 0, None), ("bf16", "bf16", 0, None)] +
               [(io, "f32", xf, lp) for io in ("f16", "bf16") for xf in (0, 1) for lp in (None, "f16", "bf16")])
# unipc: the state (x, x_last, x_c, x_out) has the out dtype, and x_is_f32 says exactly "fp32 state beside 16-bit model outputs"
UNIPC_FORMS = [f for f in DTYPE_FORMS if f[2] == int(f[0] != "f32" and f[1] == "f32")]
FM_FORMS = [f[:3] for f in DTYPE_FORMS if f[3] is None]


def form_id(f):
    return "-".join(str(v) for v in f)


def ddim_scalars(which):
    """PPOScheduler._ddim_scalars (scaled_linear, trailing, 8 steps) at an interior step / at the last step (prev_t < 0)"""
    from consolver_amd import PPOScheduler
    sch = PPOScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing", order_dim=4, scaler_dim=0,
                       factor_net_kwargs=dict(hidden_dim=8, num_actions=3))
    sch.set_timesteps(8)
    t = int(sch._timesteps[3 if which == "interior" else -1])
    return sch._ddim_scalars(t, t - 1000 // 8)


def euler_dt(which):
    """sigma[i + 1] - sigma[i] of FMPPOScheduler (8 steps, shift 3) at an interior step / at the last step"""
    from consolver_amd import FMPPOScheduler
    sch = FMPPOScheduler(shift=3.0, order_dim=4, scaler_dim=0, factor_net_kwargs=dict(hidden_dim=8, num_actions=3))
    sch.set_timesteps(8)
    i = 3 if which == "interior" else 7
    return float(F32(sch._sigmas[i + 1] - sch._sigmas[i]))


_SCAL_CACHE = {}


def cached(key, fn):
    if key not in _SCAL_CACHE:
        _SCAL_CACHE[key] = fn()
    return _SCAL_CACHE[key]


def make_lms(name, B, elems, form, *, euler, m=3, order=4, scaler=2, vpred=0, cfg=1, which="interior", extra_cols=0, dt=None):
    io, out, xf, lp = form
    rng = np.random.default_rng(_seed(name))
    c = dict(kernel="lms", name=name, B=B, elems=elems, io=io, out=out, x_is_f32=xf, lp=lp, euler=euler, m=m, order=order, scaler=scaler, vpred=vpred)
    c["x"] = tensor(rng, B, elems, "f32" if xf else io)
    c["ec"] = tensor(rng, B, elems, io)
    c["eu"] = tensor(rng, B, elems, io) if cfg else None
    c["g"] = 7.5 if cfg else 1.0
    c["hist"] = [tensor(rng, B, elems, io) for _ in range(m - 1)]
    cols = order + scaler - 1
    c["actions"] = actions_for(rng, B, cols, extra_cols) if (cols or extra_cols) else None
    c["actions_stride"] = cols + extra_cols
    c["ddim"] = cached(("ddim", which), lambda: ddim_scalars(which))
    c["dt"] = cached(("dt", which), lambda: euler_dt(which)) if dt is None else dt
    return c


def history_list(euler):
    """m x scaler x v-prediction (DDIM only) x CFG"""
    return [dict(m=m, scaler=s, vpred=v, cfg=g) for m in (1, 2, 3, 4) for s in (0, 1, 2) for v in ((0,) if euler else (0, 1)) for g in (0, 1)]


def lms_form_cases(form, euler):
    """the dtype form x the three small shapes at order_dim 4, m 3, scaler 2, CFG on"""
    tag = f"lms-{'euler' if euler else 'ddim'}-{form_id(form)}"
    return [make_lms(f"{tag}-{B}x{n}", B, n, form, euler=euler, which="interior" if k != 1 else "last") for k, (B, n) in enumerate(small_shapes(form[0]))]


def lms_history_cases(form, euler):
    tag = f"lms-hist-{'euler' if euler else 'ddim'}-{form_id(form)}"
    return [make_lms(f"{tag}-m{h['m']}s{h['scaler']}v{h['vpred']}g{h['cfg']}", 3, 269, form, euler=euler, **h) for h in history_list(euler)]


LMS_HISTORY_FORMS_DDIM = [("f32", "f32", 0, None), ("f16", "f32", 1, None)]
LMS_HISTORY_FORMS_EULER = LMS_HISTORY_FORMS_DDIM + [("f16", "f16", 0, None), ("bf16", "bf16", 0, None)]


def lms_extra_cases():
    """order_dim 8 with m in {1, 7, 8}; order_dim 1 (the baselines' form, no actions); actions_stride = order + scaler + 1 with 1e6 in the two extra columns"""
    f = ("f16", "f32", 1, None)
    cs = [make_lms(f"lms-order8-m{m}-{'euler' if eu else 'ddim'}", 3, 269, f, euler=eu, m=m, order=8, scaler=2) for m in (1, 7, 8) for eu in (0, 1)]
    cs += [make_lms(f"lms-order1-{'euler' if eu else 'ddim'}-{form_id(ff)}", 3, 269, ff, euler=eu, m=1, order=1, scaler=0)
           for eu in (0, 1) for ff in (f, ("f32", "f32", 0, None), ("bf16", "bf16", 0, None))]
    cs += [make_lms(f"lms-stride-{'euler' if eu else 'ddim'}-{form_id(ff)}", 3, 269, ff, euler=eu, m=4, order=4, scaler=2, extra_cols=2)
           for eu in (0, 1) for ff in (f, ("f32", "f32", 0, None))]
    return cs


def lms_grid_stride_cases():
    return [make_lms(f"lms-gridstride-{form_id(f)}", *grid_stride_shape(f[0]), f, euler=0, m=2, order=4, scaler=2)
            for f in (("f16", "f16", 0, None), ("f16", "f32", 1, None))]


def probe_row():
    """the rounding probe's x: +-0, exact ties of the fp16 and the bf16 grid with even and odd lower neighbours, values whose fp16 image is subnormal,
    65504, 65519.99 (-> 65504 in fp16) and 65520 (the tie to 65536: fp16 inf).  269 values: the list, repeated, so that body and tail both see it."""
    h, b = 2.0 ** -11, 2.0 ** -8                                 # half a grid step at 1.0: fp16 (10 fraction bits), bf16 (7)
    vals = [0.0, -0.0, 1 + h, 1 + 3 * h, -(1 + h), -(1 + 3 * h), 1 + b, 1 + 3 * b, -(1 + b), -(1 + 3 * b), 1 + h + 2.0 ** -23, 1 + h - 2.0 ** -23,
            1 + b + 2.0 ** -23, 1 + b - 2.0 ** -23, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25 * (1 + 2.0 ** -20), 3e-6, -3e-6, 6.1e-5,
            2.0 ** -14 - 2.0 ** -25, 65504.0, 65519.99, 65520.0, -65520.0, 65519.996, 1e-30, 3.0e38, 2.0 ** -127, 0.1, -1 / 3]
    row = np.array(vals, F32)
    return np.resize(row, 269)


def lms_probe_cases():
    cs = []
    for lp in ("f16", "bf16"):
        c = make_lms(f"lms-probe-{lp}", 3, 269, ("f16", "f32", 1, lp), euler=1, m=1, order=4, scaler=0, cfg=0, dt=0.0)
        c["x"] = np.stack([probe_row(), -probe_row(), np.roll(probe_row(), 5)]).astype(F32)
        c["ec"] = rnd(np.clip(c["ec"], -4, 4), "f16")
        cs.append(c)
    return cs


def dpm_scalars(kind, which, order):
    """DPMSolverMultistepScheduler.step_scalars: kind 'identity' (dpmsolver, epsilon: conv_x 0, conv_e 1) or 'real' (dpmsolver++), 10 steps, at step 4 / the last"""
    from consolver_amd.scheduling_dpm import DPMSolverMultistepScheduler
    kw = dict(algorithm_type="dpmsolver", final_sigmas_type="sigma_min") if kind == "identity" else dict(algorithm_type="dpmsolver++")
    sch = DPMSolverMultistepScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", solver_order=2, **kw)
    sch.set_timesteps(10)
    return tuple(float(v) for v in sch.step_scalars(4 if which == "interior" else 9, first_order=(order == 1)))


def make_dpm(name, B, elems, form, *, order, cfg, kind, which):
    io, out, xf, lp = form
    rng = np.random.default_rng(_seed(name))
    c = dict(kernel="dpm", name=name, B=B, elems=elems, io=io, out=out, x_is_f32=xf, lp=lp)
    c["x"] = tensor(rng, B, elems, "f32" if xf else io)
    c["ec"] = tensor(rng, B, elems, io)
    c["eu"] = tensor(rng, B, elems, io) if cfg else None
    c["g"] = 7.5 if cfg else 1.0
    c["m1"] = tensor(rng, B, elems, io) if order == 2 else None
    c["scal"] = cached(("dpm", kind, which, order), lambda: dpm_scalars(kind, which, order))
    c["want_m_out"] = bool(cfg or kind != "identity" or order == 2)        # m_out may be absent only without CFG and conversion: run that once per shape
    return c


DPM_VARIANTS = [dict(order=o, cfg=g, kind=k, which=w) for o, w in ((1, "interior"), (2, "interior"), (1, "last")) for g in (0, 1) for k in ("identity", "real")]


def dpm_form_cases(form):
    tag = f"dpm-{form_id(form)}"
    return [make_dpm(f"{tag}-{B}x{n}-o{v['order']}g{v['cfg']}{v['kind']}{v['which']}", B, n, form, **v) for B, n in small_shapes(form[0]) for v in DPM_VARIANTS]


def dpm_grid_stride_cases():
    return [make_dpm(f"dpm-gridstride-{form_id(f)}", *grid_stride_shape(f[0]), f, order=2, cfg=1, kind="real", which="interior")
            for f in (("f16", "f16", 0, None), ("f16", "f32", 1, "bf16"))]


def unipc_scalars(which, order, corr):
    """UniPCMultistepScheduler.step_scalars (bh2, 10 steps) at step 4 with corrector and predictor of `order`, or at the last step (order-2 corrector, first-order
    predictor to sigma = 0)"""
    from consolver_amd.scheduling_unipc import UniPCMultistepScheduler
    sch = UniPCMultistepScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", solver_order=2)
    sch.set_timesteps(10)
    if which == "last":
        cx, ce, a, p, uc = sch.step_scalars(9, corr_order=2, this_order=1, use_corr=True)
    else:
        cx, ce, a, p, uc = sch.step_scalars(4, corr_order=order, this_order=order, use_corr=bool(corr))
    return float(cx), float(ce), tuple(float(v) for v in a), tuple(float(v) for v in p), bool(uc)


def make_unipc(name, B, elems, form, *, order, corr, which, x_last_out):
    io, out, xf, lp = form
    rng = np.random.default_rng(_seed(name))
    c = dict(kernel="unipc", name=name, B=B, elems=elems, io=io, out=out, x_is_f32=xf, lp=lp)
    c["x"], c["x_last"] = tensor(rng, B, elems, out), tensor(rng, B, elems, out)
    c["ec"], c["eu"], c["g"] = tensor(rng, B, elems, io), tensor(rng, B, elems, io), 7.5
    c["m0"], c["m1"] = tensor(rng, B, elems, io), tensor(rng, B, elems, io)
    c["scal"] = cached(("unipc", which, order, corr), lambda: unipc_scalars(which, order, corr))
    c["want_x_last_out"] = bool(x_last_out)
    return c


UNIPC_VARIANTS = ([dict(order=o, corr=u, which="interior", x_last_out=l) for o in (1, 2) for u in (0, 1) for l in (0, 1)] +
                  [dict(order=2, corr=1, which="last", x_last_out=1)])


def unipc_form_cases(form):
    tag = f"unipc-{form_id(form)}"
    return [make_unipc(f"{tag}-{B}x{n}-o{v['order']}c{v['corr']}{v['which']}l{v['x_last_out']}", B, n, form, **v)
            for B, n in small_shapes(form[0]) for v in UNIPC_VARIANTS]


def unipc_grid_stride_cases():
    return [make_unipc("unipc-gridstride", *FLAT_GRID_STRIDE, ("bf16", "bf16", 0, None), order=2, corr=1, which="interior", x_last_out=1)]


def fm_scalars(with_v1, which):
    """the scalar c of FlowMatchGeneralDiscreteScheduler.step_plan over a 4-step run: Euler's dt, or (v1 read) Heun's second stage 0.5 * prev_dt"""
    from consolver_amd.scheduling_fm import FlowMatchGeneralDiscreteScheduler
    sch = FlowMatchGeneralDiscreteScheduler(shift=3.0, type="heun" if with_v1 else "euler")
    sch.set_timesteps(4)
    plans = []
    sch._step_index = 0
    for _ in range(4):
        p = sch.step_plan()
        plans.append(p)
        sch.commit_plan(p, None, None)
    p = plans[1 if which == "interior" else 3]
    assert bool(p.use_v1) == bool(with_v1)
    return float(p.c)


def make_fm(name, B, elems, form, *, with_v1, which):
    io, out, xf = form
    rng = np.random.default_rng(_seed(name))
    c = dict(kernel="fm", name=name, B=B, elems=elems, io=io, out=out, x_is_f32=xf, lp=None)
    c["x"] = tensor(rng, B, elems, "f32" if xf else io)
    c["v2"] = tensor(rng, B, elems, io)
    c["v1"] = tensor(rng, B, elems, io) if with_v1 else None
    c["c"] = cached(("fm", with_v1, which), lambda: fm_scalars(with_v1, which))
    return c


def fm_form_cases(form):
    tag = f"fm-{form_id(form)}"
    return [make_fm(f"{tag}-{B}x{n}-v{v}{w}", B, n, form, with_v1=v, which=w) for B, n in small_shapes(form[0]) for v in (0, 1) for w in ("interior", "last")]


def fm_grid_stride_cases():
    return [make_fm("fm-gridstride", *FLAT_GRID_STRIDE, ("bf16", "bf16", 0), with_v1=1, which="interior")]


# ----------------------------------------------------------------------------------------------------------------- cosine_kernel
COSINE_SHAPES = [(3, 5), (3, 269), (2, 2061)]            # the last: the second pass of the 256-thread loop (257 / 515 vectors) and a tail
COSINE_ORDERS = [(order, m) for order in (2, 4, 8) for m in sorted({1, 2, order})]


def cosine_k(elems, dt):
    V = VEC[dt]
    return V * math.ceil((elems // V) / 256) + (1 if elems % V else 0) + 10


def cosine_bound(elems, dt):
    return (2 * cosine_k(elems, dt) + 4) * U


def cosine_inputs(name, B, elems, dt, m, cfg):
    rng = np.random.default_rng(_seed(name))
    hist = [tensor(rng, B, elems, dt) for _ in range(m)]
    eu = tensor(rng, B, elems, dt) if cfg else None
    return hist, eu, (3.0 if cfg else 0.0)


def cosine_fp64(hist, m, order, eu, g, dt):
    """(features [B, order - 1] float64, combined eps or None): the features of the combined eps, rounded to dt at the exact value"""
    c0 = cfg_fp64(hist[0], eu, g, dt).v if eu is not None else np.asarray(hist[0], F64)
    B = c0.shape[0]
    out = np.zeros((B, order - 1))
    nc = np.maximum(np.sqrt((c0 * c0).sum(-1)), 1e-8)
    for i in range(1, m):
        a = np.asarray(hist[i], F64)
        out[:, i - 1] = (a * c0).sum(-1) / (np.maximum(np.sqrt((a * a).sum(-1)), 1e-8) * nc)
    return out, (cfg_exact(hist[0], eu, g, dt) if eu is not None else None)


def _block_sum(prod, elems, V):
    """cosine_kernel's reduction of prod[B, elems] (fp32 products): thread t adds vectors t, t + 256, ... element by element, then tail element nvec V + t;
    wave_sum's butterfly (xor 32, 16, .., 1); the four waves left to right"""
    B = prod.shape[0]
    nvec = elems // V
    acc = np.zeros((B, 256), F32)
    passes = math.ceil(nvec / 256)
    body = np.zeros((B, passes * 256 * V), F32)
    body[:, :nvec * V] = prod[:, :nvec * V]
    body = body.reshape(B, passes, 256, V)
    live = (np.arange(passes * 256).reshape(passes, 256) < nvec)
    for p in range(passes):
        for j in range(V):
            acc = np.where(live[p][None], (acc + body[:, p, :, j]).astype(F32), acc)
    tail = elems - nvec * V
    if tail:
        acc[:, :tail] = (acc[:, :tail] + prod[:, nvec * V:]).astype(F32)
    lanes = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[:, lanes ^ o]).astype(F32)
    w = acc[:, ::64]
    return (((w[:, 0] + w[:, 1]).astype(F32) + w[:, 2]).astype(F32) + w[:, 3]).astype(F32)


def cosine_emulated(hist, m, order, eu, g, dt):
    c0 = cfg_exact(hist[0], eu, g, dt) if eu is not None else np.asarray(hist[0], F32)
    B, elems = c0.shape
    out = np.zeros((B, order - 1), F32)
    for i in range(1, m):
        a = np.asarray(hist[i], F32)
        d, na, nc = (_block_sum((p * q).astype(F32), elems, VEC[dt]) for p, q in ((a, c0), (a, a), (c0, c0)))
        out[:, i - 1] = (d / (np.maximum(np.sqrt(na), F32(1e-8)) * np.maximum(np.sqrt(nc), F32(1e-8))).astype(F32)).astype(F32)
    return out


def one_hot_positions(B, elems, dt):
    """(sample, element): the first element of sample 1, the last lane of the last vector, the last tail element"""
    V = VEC[dt]
    pos = [(1 % B, 0), (B - 1, elems - 1)]
    if elems >= V:
        pos.append((B - 1, (elems // V) * V - 1))
    return pos


# ----------------------------------------------------------------------------------------------------------------- stack / masks
STACK_ORDERS = [(order, m) for order in (1, 4, 8) for m in sorted({0, 1, order})]
STACK_GRID_STRIDE = {"f32": (1, 65536 + 4 + 3), "f16": (1, 131072 + 8 + 5)}       # the first sizes past the 64-block cap


def stack_exact(hist, m, order):
    B, elems = hist[0].shape if hist else (0, 0)
    out = np.zeros((B, order, elems), F32)
    for k in range(m):
        out[:, k] = hist[k]
    return out


def masks_exact(B, A, m, order):
    a = np.arange(A)
    return np.broadcast_to(np.where((a >= m - 1) & (a < order - 1), 0.0, 1.0).astype(F32), (B, A)).copy()


MASK_CASES = [(B, order + d, m, order) for order in range(1, 9) for m in range(1, order + 1) for d in (-1, 1, 2) if order + d >= 1 for B in (1, 43)]


# ----------------------------------------------------------------------------------------------------------------- sample / action_probs
def sample_exact(probs, uni, av):
    """probs [B, A, K], uni [B, A], av [A, K] fp32 -> (idx, actions, action_probs): c += p[j] in order, first u < c; then back over bins with p <= 0"""
    B, A, K = probs.shape
    idx = np.zeros((B, A), np.int64)
    for b in range(B):
        for a in range(A):
            p, u, c, k = probs[b, a], uni[b, a], F32(0), K - 1
            for j in range(K):
                c = F32(c + p[j])
                if u < c:
                    k = j
                    break
            while k > 0 and p[k] <= 0:
                k -= 1
            idx[b, a] = k
    return (idx,) + gather_exact(probs, idx, av)


def gather_exact(probs, idx, av):
    B, A, K = probs.shape
    k = np.clip(idx, 0, K - 1)
    return (np.take_along_axis(np.broadcast_to(av, (B, A, K)), k[..., None], 2)[..., 0].astype(F32), np.take_along_axis(probs, k[..., None], 2)[..., 0].astype(F32))


def sample_case(K, A, BA, seed=0):
    """probs with zero bins at the head, in the middle and at the tail of some rows, one row that sums below 1; uniforms that hit a partial sum exactly, lie
    above a row's fp32 total, are 0 and just below 1"""
    assert BA % A == 0
    B = BA // A
    rng = np.random.default_rng(1000 * K + 10 * A + BA + seed)
    p = rng.random((B, A, K)).astype(F32) + F32(0.01)
    rows = p.reshape(-1, K)
    n = rows.shape[0]
    for r in range(n):
        if K >= 4:
            if r % 4 == 0:
                rows[r, :K // 4] = 0
            if r % 4 == 1:
                rows[r, K // 3:K // 3 + max(1, K // 5)] = 0
            if r % 4 == 2:
                rows[r, K - max(1, K // 4):] = 0
        elif K == 2 and r % 3 != 0:
            rows[r, r % 2] = 0
    rows /= rows.sum(-1, keepdims=True)
    if n > 1:
        rows[1::5] *= F32(0.5)                                   # rows that sum to 0.5
    p = rows.reshape(B, A, K).astype(F32)
    u = rng.random((B, A)).astype(F32)
    uf = u.reshape(-1)
    rows = p.reshape(-1, K)
    csum = np.zeros((n, K), F32)
    c = np.zeros(n, F32)
    for j in range(K):
        c = (c + rows[:, j]).astype(F32)
        csum[:, j] = c
    for r in range(n):
        if r % 4 == 0:
            uf[r] = csum[r, (r // 4) % K]                        # exactly a partial sum: u < c is false there, the next bin with mass is taken
        elif r % 4 == 1:
            uf[r] = np.nextafter(csum[r, -1], F32(2))            # above the row's fp32 total: K - 1, then back over empty bins
        elif r % 8 == 2:
            uf[r] = 0.0
        elif r % 8 == 6:
            uf[r] = np.nextafter(F32(1), F32(0))
    av = np.stack([so.torch_linspace_f32(-1 - a, 1 + a, K) for a in range(A)]).astype(F32)
    return p, uf.reshape(B, A).astype(F32), av


# B * A in {1, 129} where A divides it; with A = 9 the nearest sizes (one row of 9; 135 = 15 x 9, two blocks)
SAMPLE_CASES = ([(K, A, BA) for K in (1, 2, 11, 161) for A in (1, 3, 9) for BA in (1, 129) if BA % A == 0] +
                [(K, 9, BA) for K in (1, 2, 11, 161) for BA in (9, 135)] + [(11, 3, 3)])


def sel_exact(probs, actions, av):
    """action_probs_kernel's sel: the probability of the nearest grid value, the first strict minimum of |act - av[j]|"""
    B, A, K = probs.shape
    sel = np.zeros((B, A), F32)
    for b in range(B):
        for a in range(A):
            best, bd = 0, np.abs(F32(actions[b, a] - av[a, 0]))
            for j in range(K):
                d = np.abs(F32(actions[b, a] - av[a, j]))
                if d < bd:
                    bd, best = d, j
            sel[b, a] = probs[b, a, best]
    return sel


EPS32 = F32(1.1920929e-07)


def entropy_fp64(probs):
    p = np.asarray(probs, F64)
    q = p / p.sum(-1, keepdims=True)
    return -(q * np.log(np.clip(q, F64(EPS32), F64(F32(1) - EPS32)))).sum(-1) / math.log(probs.shape[-1])


def entropy_bound(probs):
    p = np.asarray(probs, F64)
    K = p.shape[-1]
    q = p / p.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        H = np.where(q > 0, q * np.abs(np.log(q)), 0.0).sum(-1)
    return ((2 * K + 8) * H + (K + 2)) * U / math.log(K) + 2 * U * np.abs(entropy_fp64(probs))


def entropy_emulated(probs):
    """action_probs_kernel's loop in fp32: s += p[j]; q = p[j] / s; h -= q * logf(clamp(q)); h / logf(K)"""
    p = np.asarray(probs, F32)
    K = p.shape[-1]
    s = np.zeros(p.shape[:-1], F32)
    for j in range(K):
        s = (s + p[..., j]).astype(F32)
    h = np.zeros_like(s)
    for j in range(K):
        q = (p[..., j] / s).astype(F32)
        h = (h - (q * np.log(np.clip(q, EPS32, F32(1) - EPS32)).astype(F32)).astype(F32)).astype(F32)
    return (h / np.log(F32(K))).astype(F32)


def action_probs_case(K, seed=0):
    """probs [B, 3, K]: random rows, rows with exact zeros, a one-hot row, an unnormalised row (sum 0.5), a uniform row; actions on the grid, halfway between two
    grid values, outside the grid; the grid of dimension 2 repeats a value"""
    rng = np.random.default_rng(77 * K + seed)
    A, B = 3, 6
    p = rng.random((B, A, K)).astype(F32) + F32(1e-3)
    p[1, :, ::2] = 0
    p[2] = 0
    p[2, :, K // 2] = 1
    p /= p.sum(-1, keepdims=True)
    p[3] *= F32(0.5)
    p[4] = F32(1.0 / K)
    av = np.stack([np.arange(K, dtype=F32) * F32(0.25) - F32(1), so.torch_linspace_f32(-2, 0, K), so.torch_linspace_f32(-1, 1, K)]).astype(F32)
    av[2, K // 2:] = np.roll(av[2, K // 2:], 1) if K > 2 else av[2, K // 2:]
    if K > 2:
        av[2, 1] = av[2, 0]                                      # a repeated grid value: the lower index wins
    act = np.zeros((B, A), F32)
    for b in range(B):
        j = (b * 3) % K
        act[b, 0] = av[0, j] + (F32(0.125) if (b % 2 == 0 and j + 1 < K) else F32(0))     # exactly halfway between av[0, j] and av[0, j + 1]: j wins
        act[b, 1] = av[1, j] + F32(rng.standard_normal() * 0.01)
        act[b, 2] = av[2, 0] if b % 2 else F32(rng.uniform(-1.5, 1.5))
    return p.astype(F32), act, av
