"""CPU references and input families for the fused cross-attention block tests (tests/test_xattn_ref.py, tests/test_xattn_forms_gpu.py): test infrastructure,
not a fallback.  The block (consolver_amd/csrc/xattn.hip, C = 320, 8 heads x 40, at most 80 keys) is

    out (+ out_lo) = h (+ h_lo) + (softmax(scale * (LayerNorm(h) Wq^T) K^T) V) Wo^T + bo,      kv[b] = (K | V) [Nk][640] of sample b = row // HW.

Every function takes the SAME rounded fp16 inputs the kernel sees (an `Inputs`).  The LayerNorm reads the hi plane only, in every stream form.

* ``xattn_fp64``     -- the block in float64: the attention output O [M, 320] and the branch O Wo^T + bo [M, 320]: what the op is supposed to compute.
* ``xattn_emulated`` -- the same math with the kernel's rounding points (line numbers of xattn.hip, xattn_block_kernel; xattn64_kernel repeats them at
  506-560, 575, 626-662, 681 and 712-731).  It is the YARDSTICK for the tolerances of the GPU tests (how far from fp64 an implementation with these roundings
  lands), not a second implementation to debug against:
    1. LayerNorm: fp32 statistics -- mean = sum * (1.0f / C) (192), two-pass variance sum (x - mean)^2 (196), rs = rsqrtf(var * (1.0f / C) + eps) (207) -- and the
       output ((x - mean) * rs) * gamma + beta rounded to fp16 by `pk(...)` into XT (211-213);
    2. q = LN(h) Wq^T in fp32 MFMA accumulators, rounded to fp16, multiplied in fp32 by c = float(scale) * 1.4426950408889634f (765) and rounded to fp16 again:
       `qv[r] = (float)(f16)acc[i][j][r] * p.c` (230), then `pk(qv[0], qv[1])` (231);
    3. the scores S = q K^T are fp32 MFMA accumulators (274-275); keys >= Nk are -inf (284);
    4. P = exp2(S - true row maximum) (287, 292) is rounded to fp16 for P V (299-300);
    5. the denominator l adds the UNROUNDED fp32 exponentials (`l += e`, 292) -- ``denominator="rounded"`` is the other choice, for the tests that tell them apart;
    6. P V in fp32 (314), O * (1.0f / l) rounded to fp16 (317, 322);
    7. the branch: O Wo^T in fp32, `acc + bias` rounded to fp16 into the epilogue patch (341);
    8. f = patch + h (+ h_lo) in fp32, left to right (372 / 385 / 394); out = f16(f), out_lo = f16(f - out) (373), lo8 = e5m2(f - out) (386, 389-390).
  Not carried: the order of the fp32 sums (MFMA accumulation, the LayerNorm butterflies, l), the last bit of v_exp_f32 and rsqrtf, whether the compiler
  contracts the LayerNorm's last multiply-add (emulated as one fma), and the double rounding to fp16 that follows from each of them -- all at 2^-24 of the value
  before an fp16 rounding of 2^-11, i.e. they move an fp16 result only where the fp32 value sits within 2^-13 ulp of a tie.

Reading the branch off the output (``recover_branch`` / ``recovery_term``).  In the split form the kernel forms t = fl32(v + h), f = fl32(t + h_lo) with v the fp16
patch value, and stores hi = f16(f), lo = f16(f - hi).  |t - (v + h)| <= 2^-24 |t| and |f - (t + h_lo)| <= 2^-24 |f|, and |t| <= |f| + |h_lo| (1 + 2^-24), so
|f - (v + h + h_lo)| <= 2^-24 (2 |f| + |h_lo|) to first order.  d = f - hi is exact in fp32 (|d| <= 2^-11 |f| and d is a multiple of f's fp32 ulp), and
lo = f16(d) is off by at most 2^-11 |d| <= 2^-22 |f| while d is an fp16 normal, by at most 2^-25 (half the fp16 subnormal spacing) below that.  hi + lo - (h + h_lo)
is exact in float64, hence

    |hi + lo - (h + h_lo) - v| <= (2^-22 + 2 * 2^-24) |f| + 2^-24 |h_lo| + 2^-25,

evaluated with |hi + lo| (1 + 2^-20) for |f|.  Every bound on a recovered branch adds the norm of this term over the columns it covers, relative to the reference.
With Wo = I and bo = 0 the patch is f16(O) = O itself, so every (row, head) of the attention output is observable.

Input families (``make_case``), generated on the CPU from a seed and shared by the CPU and the GPU tests:
  gauss     the inputs of test_xattn_block_fused_kernel: unit-Gaussian h (split into hi + lo) and kv, gamma = 1 + 0.1 N, beta = 0.05 N, Wq, Wo = N / sqrt(320), bo = 0.05 N;
  dc        h = 30 + N(0, 1): fp16 ulp 2^-5, a non-zero h_lo: the two-pass variance and the residual add far from zero;
  peaky     the K half of kv multiplied by 6 (softmax close to one-hot in most rows);
  last      row Nk - 1 of kv (K and V) multiplied by 8: a dropped or mis-masked final key is an O(1) error;
  selector  exact: gamma = 0, beta = 1 (every LayerNorm row is exactly 1), Wq = I, K = +16 on the head slice of ONE key j*(b, head) and -16 elsewhere (scores
            +-146: P is exactly one-hot, l = 1), V integers in [-8, 8], Wo on a 1/16 grid (|Wo| <= 1/4), bo and h on a 1/8 grid: O[row, head] = V[b, j*, head] and
            the branch and f are exact in fp32.  ``lo_grid``: h_lo = k 2^-14, |k| <= 8 (e5m2 values), so that most of the output's lo plane is non-zero;
  nk1       exact: Nk = 1, Gaussian gamma, beta, Wq and (rounded to the 1/8 grid) h; V, Wo, bo as in selector: O = V[b, 0] whatever q is;
  qround    exact, and decided by the SECOND rounding of q: beta = 1 except one channel m of every head where it is 1 + 2^-10; Wq = I plus one entry t in the row of
            another channel n of the head, so that acc_n = 1 + t (exact) with f16(f16(1 + t) c) != f16((1 + t) c) (t is searched for, ``qround_t``).  Key j_A has K = 2^13
            on channel n, key j_B on channel m, every other key -2^13 on both.  With both roundings q_n = q_m, the two scores are EQUAL, P = (1, 1), l = 2 and
            O = (V[j_A] + V[j_B]) / 2 exactly; with one rounding they differ by a whole number j >= 1 and O = (V[j_A] + 2^-j V[j_B]) / (1 + 2^-j) or its mirror;
  denom     decided by which exponentials the denominator adds: selector's q, key j* with K = 0 and every other key with K = -a on one channel, a chosen
            (``denom_a``) so that all the other keys share ONE score -x (exact in fp32) whose exp2 is ~0.45 fp16 ulp away from its fp16 rounding; V[j*] Gaussian, every other
            V row zero, h = 0 (with Wo = I, bo = 0 the hi plane is O itself).  Then O = V[j*] / (1 + (Nk - 1) 2^-x): the numerator is exact, so the result is a correctly rounded fp16 of V[j*] / l up to the fp32 error of l
            (<= 80 * 2^-24 + 2^-22 relative), while a denominator from the rounded P is off by (Nk - 1) (f16(2^-x) - 2^-x) / l, about 4e-4, in EVERY element with one sign.
"""
import math

import torch

C, NH, DH = 320, 8, 40
LOG2E = 1.4426950408889634
EPS = 1e-5
SCALE = float(torch.tensor(DH ** -0.5, dtype=torch.float32))          # the ABI takes a float
F16_ULP = 2.0 ** -10
E5M2 = torch.float8_e5m2
NK_ALL = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 76, 77, 79, 80)
SHAPES = ((1, 64), (3, 64), (2, 128), (1, 192), (2, 256))
FAMILIES = ("gauss", "dc", "peaky", "last", "selector", "nk1")


def c32():
    """p.c as the launcher forms it: float(scale) * 1.4426950408889634f in fp32"""
    return torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)


class Inputs:
    __slots__ = ("B", "HW", "Nk", "h", "h_lo", "gamma", "beta", "wq", "wo", "bo", "kv")

    @property
    def M(self):
        return self.B * self.HW

    def with_lo(self, h_lo):
        o = Inputs()
        for k in self.__slots__:
            setattr(o, k, getattr(self, k))
        o.h_lo = h_lo
        return o


def lo8_of(x):
    """fp16 / fp32 tensor -> the e5m2 bytes torch holds for it"""
    return x.float().to(E5M2).view(torch.uint8)


def lo8_value(b):
    return b.view(E5M2).float()


def _heads(t, B):
    """[B * n, 320] -> [B, 8, n, 40]"""
    return t.reshape(B, -1, NH, DH).transpose(1, 2)


def _rows(t):
    """[B, 8, n, 40] -> [B * n, 320]"""
    return t.transpose(1, 2).reshape(-1, C)


def xattn_fp64(x):
    """(O [M, 320], branch [M, 320]) in float64"""
    h = x.h.double()
    mu = h.mean(-1, keepdim=True)
    var = ((h - mu) ** 2).mean(-1, keepdim=True)
    ln = (h - mu) / torch.sqrt(var + float(torch.tensor(EPS, dtype=torch.float32))) * x.gamma.double() + x.beta.double()
    q = _heads(ln @ x.wq.double().T, x.B)
    k, v = _heads(x.kv[..., :C].double().reshape(-1, C), x.B), _heads(x.kv[..., C:].double().reshape(-1, C), x.B)
    s2 = (q @ k.transpose(-1, -2)) * (SCALE * LOG2E)
    p = torch.exp2(s2 - s2.amax(-1, keepdim=True))
    o = _rows((p @ v) / p.sum(-1, keepdim=True))
    return o, o @ x.wo.double().T + x.bo.double()


def _sum32(t):
    """one fp32 rounding of an exact sum (the order of the kernel's fp32 sums is not carried)"""
    return t.double().sum(-1, keepdim=True).float()


def _mm32(a, b):
    """fp16 operands, fp32 accumulator: products exact, one rounding of the sum"""
    return (a.double() @ b.double()).float()


def xattn_emulated(x, lo8=False, denominator="unrounded", q_roundings=2):
    """dict: O (fp16, [M, 320]), patch (fp16: the branch as the epilogue holds it), f (fp32), out (fp16), out_lo (fp16; None in the plain form), lo8 (uint8, when asked).
    x.h_lo None: plain form; lo8: x.h_lo holds e5m2 values (as fp16) and the lo plane leaves as bytes.  denominator / q_roundings: the kernel's choices by default; the
    other ones exist so that the CPU tests can show which GPU test tells them apart."""
    f32 = torch.float32
    h = x.h.float()
    inv_c = torch.tensor(1.0 / C, dtype=f32)
    mean = _sum32(h) * inv_c                                                             # 1
    d = h - mean
    rs = torch.rsqrt(_sum32(d * d) * inv_c + torch.tensor(EPS, dtype=f32))
    ln = ((d * rs * x.gamma.float()).double() + x.beta.double()).float().half()
    acc = _mm32(ln, x.wq.T)                                                              # 2
    q = ((acc.half().float() if q_roundings == 2 else acc) * c32()).half()
    qh, kh, vh = _heads(q, x.B), _heads(x.kv[..., :C].reshape(-1, C), x.B), _heads(x.kv[..., C:].reshape(-1, C), x.B)
    s = _mm32(qh, kh.transpose(-1, -2))                                                  # 3
    e = torch.exp2(s - s.amax(-1, keepdim=True))                                         # 4
    p = e.half()
    l = _sum32(p if denominator == "rounded" else e)                                     # 5
    o = (_mm32(p, vh) * (1.0 / l)).half()                                                # 6
    O = _rows(o)
    patch = (_mm32(O, x.wo.T) + x.bo.float()).half()                                     # 7
    f = patch.float() + h                                                                # 8
    r = {"O": O, "patch": patch}
    if x.h_lo is not None:
        f = f + x.h_lo.float()
    out = f.half()
    r.update(f=f, out=out, out_lo=None)
    if x.h_lo is not None:
        dlt = f - out.float()
        r["out_lo"] = dlt.half()
        if lo8:
            r["lo8"] = dlt.to(E5M2).view(torch.uint8)
    return r


def split_planes(f, lo8=False):
    """torch's own split of an fp32 value: (fp16, fp16) or (fp16, e5m2 bytes)"""
    hi = f.half()
    d = f.float() - hi.float()
    return hi, (d.to(E5M2).view(torch.uint8) if lo8 else d.half())


# ---- errors and the recovery of the branch ---------------------------------------------------------------------------------------------------------------
def err_heads(got, ref):
    """relative L2 per (row, head): [M, 8] float64"""
    g, r = got.double().reshape(-1, NH, DH), ref.double().reshape(-1, NH, DH)
    return (g - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-300)


def err_rows(got, ref):
    """relative L2 per row over the 320 columns: [M] float64"""
    return (got.double() - ref.double()).norm(dim=-1) / ref.double().norm(dim=-1).clamp_min(1e-300)


def recover_branch(out, out_lo, h, h_lo):
    """out + out_lo - (h + h_lo) in float64 (exact): the fp16 patch value up to recovery_term"""
    return (out.double() + out_lo.double()) - (h.double() + h_lo.double())


def recovery_term(out, out_lo, h_lo):
    """elementwise bound on |recover_branch - patch| (derived in the header)"""
    f = (out.double() + out_lo.double()).abs() * (1 + 2.0 ** -20)
    return (2.0 ** -22 + 2 * 2.0 ** -24) * f + 2.0 ** -24 * h_lo.double().abs() + 2.0 ** -25


def term_heads(term, ref):
    return term.reshape(-1, NH, DH).norm(dim=-1) / ref.double().reshape(-1, NH, DH).norm(dim=-1).clamp_min(1e-300)


def term_rows(term, ref):
    return term.norm(dim=-1) / ref.double().norm(dim=-1).clamp_min(1e-300)


def is_nearest_f16(hi, x):
    """bool tensor: hi is A nearest fp16 of the float64 value x (no worse than either of its fp16 neighbours; either side of a tie passes)"""
    bits = hi.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag, sign = bits & 0x7FFF, bits & 0x8000
    up = (mag + 1) | sign
    dn = torch.where(mag > 0, (mag - 1) | sign, (sign ^ 0x8000) | 1)
    val = lambda b: torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16).view(torch.float16).double()
    e = (x - hi.double()).abs()
    return (e <= (x - val(up)).abs()) & (e <= (x - val(dn)).abs())


def half_ulp(v, mant_bits, min_exp):
    """half the spacing of a format with `mant_bits` stored mantissa bits and smallest normal 2^min_exp, in the binade of |v| (float64 tensor in, float64 out)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** min_exp))).clamp_min(min_exp)
    return torch.exp2(e - mant_bits - 1)


# ---- input families -------------------------------------------------------------------------------------------------------------------------------------------
def _base(B, HW, Nk, g):
    x = Inputs()
    x.B, x.HW, x.Nk = B, HW, Nk
    x.gamma = (1 + 0.1 * torch.randn(C, generator=g)).half()
    x.beta = (0.05 * torch.randn(C, generator=g)).half()
    x.wq = (torch.randn(C, C, generator=g) * C ** -0.5).half()
    x.wo = (torch.randn(C, C, generator=g) * C ** -0.5).half()
    x.bo = (0.05 * torch.randn(C, generator=g)).half()
    x.kv = torch.randn(B, Nk, 2 * C, generator=g).half()
    h32 = torch.randn(B * HW, C, generator=g)
    x.h = h32.half()
    x.h_lo = (h32 - x.h.float()).half()
    return x, h32


def default_jstar(B, Nk, t=0):
    """the selected key of (sample b, head hd), distinct across the heads of a sample where Nk allows; over t = 0 .. ceil(80 / B) - 1 every head visits every position"""
    b, hd = torch.arange(B)[:, None], torch.arange(NH)[None, :]
    return (t + -(-80 // B) * b + 10 * hd) % Nk


def _grid_tail(x, g):
    """selector's exact tail: integer V, Wo on the 1/16 grid (|Wo| <= 1/4), bo on the 1/8 grid"""
    x.kv[..., C:] = torch.randint(-8, 9, (x.B, x.Nk, C), generator=g).half()
    x.wo = (torch.randint(-4, 5, (C, C), generator=g).float() / 16).half()
    x.bo = (torch.randint(-8, 9, (C,), generator=g).float() / 8).half()


def _grid_h(x, g, lo_grid):
    x.h = (torch.randint(-32, 33, (x.M, C), generator=g).float() / 8).half()
    x.h_lo = (torch.randint(-8, 9, (x.M, C), generator=g).float() * 2.0 ** -14).half() if lo_grid else torch.zeros(x.M, C, dtype=torch.float16)


def selector_k(B, Nk, jstar):
    """K half [B, Nk, 320]: +16 on the head slice of key jstar[b, hd], -16 elsewhere"""
    k = torch.full((B, Nk, NH, DH), -16.0)
    b, hd = torch.meshgrid(torch.arange(B), torch.arange(NH), indexing="ij")
    k[b, jstar, hd] = 16.0
    return k.reshape(B, Nk, C).half()


def selector_closed_form(x, jstar):
    """(O, f) of the selector family in float64: O[row, head] = V[b, j*(b, head), head], f = fp16(O Wo^T + bo) + h + h_lo"""
    v = x.kv[..., C:].double().reshape(x.B, x.Nk, NH, DH)
    b, hd = torch.meshgrid(torch.arange(x.B), torch.arange(NH), indexing="ij")
    o = v[b, jstar, hd].reshape(x.B, 1, C).expand(x.B, x.HW, C).reshape(-1, C)
    return o, _tail_closed_form(x, o)


def _tail_closed_form(x, o):
    patch = (o @ x.wo.double().T + x.bo.double()).float().half()    # exact in fp32 (and in float64): ONE rounding, to fp16
    return patch.double() + x.h.double() + (x.h_lo.double() if x.h_lo is not None else 0.0)


_QT = []


def qround_t():
    """the smallest t = 2^-11 + k 2^-14 (fp16; 1 + t exact in fp32, f16(1 + t) = 1 + 2^-10) for which the two roundings of q and a single one disagree"""
    if not _QT:
        for k in range(1, 8):
            t = torch.tensor(2.0 ** -11 + k * 2.0 ** -14, dtype=torch.float32)
            a = 1 + t
            two, one = (a.half().float() * c32()).half(), (a * c32()).half()
            if float(a.half()) == 1 + 2.0 ** -10 and float(two) != float(one):
                _QT.append((float(t), float(two), float(one)))
                break
        assert _QT, "no coupling t separates one rounding of q from two"
    return _QT[0]


_DA = []


def denom_a():
    """(a, x, eps): K = -a on one channel of the other keys gives them the score -x = -(q a) (exact in fp32, q = f16(c) as in selector) with 2^-x in [1/2, 1) and
    |f16(2^-x) - 2^-x| >= 0.4 fp16 ulp of 2^-x"""
    if not _DA:
        q = float(c32().half())
        best = None
        for k in range(1, int(1024 / q) + 1):                    # x = q a < 1
            a = k / 1024.0                                       # (not every such a is an fp16 value: checked through .half())
            if float(torch.tensor(a).half()) != a:
                continue
            xx = q * a
            if not (0.0 < xx < 1.0) or float(torch.tensor(xx, dtype=torch.float64).float()) != xx:
                continue
            e = 2.0 ** -xx
            off = abs(float(torch.tensor(e, dtype=torch.float64).half()) - e) / 2.0 ** -11      # in fp16 ulps of [1/2, 1)
            if 0.40 <= off <= 0.47 and (best is None or xx > best[1]):      # the largest x: 2^-x just above 1/2, where an fp16 ulp is relatively largest
                best = (a, xx, e)
        assert best, "no score with a badly rounding exponential"
        _DA.append(best)
    return _DA[0]


class Case:
    __slots__ = ("family", "x", "ref_o", "ref_branch", "emu", "emu_o", "emu_branch", "jstar", "exact_o", "exact_f")


_CASES = {}


def make_case(family, B, HW, Nk, seed=0, identity_out=False, lo_grid=False, jstar=None):
    """inputs, the fp64 reference, the emulator's result on the split form and its own worst errors, computed once per case and shared (nothing may write to it).
    identity_out: Wo = I, bo = 0 (the patch is O itself)."""
    key = (family, B, HW, Nk, seed, identity_out, lo_grid, None if jstar is None else tuple(jstar.flatten().tolist()))
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(100003 * seed + 7919 * FAM_ID[family] + 131 * B + 17 * HW + Nk)
    x, h32 = _base(B, HW, Nk, g)
    c = Case()
    c.family, c.jstar, c.exact_o, c.exact_f = family, None, None, None
    if family == "dc":
        h32 = h32 + 30.0
        x.h = h32.half()
        x.h_lo = (h32 - x.h.float()).half()
    elif family == "peaky":
        x.kv[..., :C] = (6.0 * x.kv[..., :C].float()).half()
    elif family == "last":
        x.kv[:, Nk - 1] = (8.0 * x.kv[:, Nk - 1].float()).half()
    elif family in ("selector", "qround", "denom"):
        x.gamma, x.beta, x.wq = torch.zeros(C).half(), torch.ones(C).half(), torch.eye(C).half()
        _grid_tail(x, g)
        _grid_h(x, g, lo_grid)
        c.jstar = default_jstar(B, Nk) if jstar is None else jstar
        if family == "selector":
            x.kv[..., :C] = selector_k(B, Nk, c.jstar)
        elif family == "qround":
            assert Nk >= 2
            n, m, n2 = 5, 33, 17                                  # channels of the head: n in the first k32 step of the score MFMA, m in the second, n2 the coupled one
            t, _, _ = qround_t()
            jb = (c.jstar + 1 + (torch.arange(NH)[None, :] % max(Nk - 1, 1))) % Nk
            jb = torch.where(jb == c.jstar, (jb + 1) % Nk, jb)
            bt = x.beta.reshape(NH, DH).clone(); bt[:, m] = 1 + 2.0 ** -10; x.beta = bt.reshape(C)
            wq = x.wq.clone()
            for hd in range(NH):
                wq[hd * DH + n, hd * DH + n2] = t
            x.wq = wq
            k = torch.zeros(B, Nk, NH, DH)
            k[..., n] = -8192.0; k[..., m] = -8192.0
            bb, hh = torch.meshgrid(torch.arange(B), torch.arange(NH), indexing="ij")
            k[bb, c.jstar, hh, n] = 8192.0; k[bb, c.jstar, hh, m] = 0.0
            k[bb, jb, hh, m] = 8192.0; k[bb, jb, hh, n] = 0.0
            x.kv[..., :C] = k.reshape(B, Nk, C).half()
            v = x.kv[..., C:].double().reshape(B, Nk, NH, DH)
            c.exact_o = (0.5 * (v[bb, c.jstar, hh] + v[bb, jb, hh])).reshape(B, 1, C).expand(B, HW, C).reshape(-1, C)
            c.exact_f = _tail_closed_form(x, c.exact_o)
            c.jstar = torch.stack([c.jstar, jb])
        else:
            a, _, _ = denom_a()
            x.h, x.h_lo = torch.zeros_like(x.h), torch.zeros_like(x.h_lo)      # h = 0 (the LayerNorm row is still exactly beta): with Wo = I the hi plane IS O
            bb, hh = torch.meshgrid(torch.arange(B), torch.arange(NH), indexing="ij")
            k = torch.zeros(B, Nk, NH, DH)
            k[..., 7] = -a
            k[bb, c.jstar, hh, 7] = 0.0
            x.kv[..., :C] = k.reshape(B, Nk, C).half()
            vg = torch.randn(B, NH, DH, generator=g).half()
            v = torch.zeros(B, Nk, NH, DH, dtype=torch.float16)
            v[bb, c.jstar, hh] = vg
            x.kv[..., C:] = v.reshape(B, Nk, C)
        if family == "selector":
            c.exact_o, c.exact_f = selector_closed_form(x, c.jstar)
    elif family == "nk1":
        assert Nk == 1
        _grid_tail(x, g)
        x.h = (torch.round(h32 * 8) / 8).half()
        x.h_lo = (torch.randint(-8, 9, (x.M, C), generator=g).float() * 2.0 ** -14).half() if lo_grid else torch.zeros(x.M, C, dtype=torch.float16)
        c.exact_o = x.kv[:, 0, C:].double().reshape(B, 1, C).expand(B, HW, C).reshape(-1, C)
        c.exact_f = _tail_closed_form(x, c.exact_o)
    else:
        assert family == "gauss", family
    if identity_out:
        x.wo, x.bo = torch.eye(C).half(), torch.zeros(C).half()
        if c.exact_o is not None:
            c.exact_f = _tail_closed_form(x, c.exact_o)
    c.x = x
    c.ref_o, c.ref_branch = xattn_fp64(x)
    c.emu = xattn_emulated(x)
    c.emu_o = float(err_heads(c.emu["O"], c.ref_o).max())
    c.emu_branch = float(err_rows(c.emu["patch"], c.ref_branch).max())
    _CASES[key] = c
    return c


FAM_ID = {f: i for i, f in enumerate(FAMILIES + ("qround", "denom"))}


def denom_expected(c):
    """float64 O of the denom family: V[j*] / (1 + (Nk - 1) 2^-x)"""
    _, xx, e = denom_a()
    x = c.x
    v = x.kv[..., C:].double().reshape(x.B, x.Nk, NH, DH)
    bb, hh = torch.meshgrid(torch.arange(x.B), torch.arange(NH), indexing="ij")
    o = v[bb, c.jstar, hh] / (1.0 + (x.Nk - 1) * e)
    return o.reshape(x.B, 1, C).expand(x.B, x.HW, C).reshape(-1, C)


DENOM_NOISE = 80 * 2.0 ** -24 + 2.0 ** -22          # relative fp32 error of V[j*] * (1 / l): l's <= 80-term sum, the exponential, the reciprocal and the product


def denom_check(o16, c):
    """(worst elementwise excess over half an fp16 ulp + the fp32 noise, in units of the bound; |mean signed relative error|; its bound) of an fp16 O against the closed form.
    The rounding errors of the final fp16 rounding are zero-mean over the N elements (uniform in +-half an ulp: sigma <= 2^-11 / sqrt(3) relative), so their mean stays
    below 6 sigma / sqrt(N); a denominator from the rounded P shifts EVERY element by the same relative amount (about 4e-4 at Nk = 80)."""
    want = denom_expected(c)
    got = o16.double()
    tol = half_ulp(want * (1 + DENOM_NOISE), 10, -14) + DENOM_NOISE * want.abs()         # got = f16(y), |y - want| <= noise: half an ulp of y's binade, plus the noise
    excess = float((((got - want).abs() - tol) / tol).max())
    first = slice(None, None, c.x.HW)                                                     # the rows of a sample share q, hence O: one row per sample is the independent set
    nz = want[first].abs() >= 2.0 ** -14
    rel = ((got[first] - want[first]) / want[first])[nz]
    bound = DENOM_NOISE + 6 * (2.0 ** -11 / math.sqrt(3)) / math.sqrt(rel.numel())
    return excess, abs(float(rel.mean())), bound
