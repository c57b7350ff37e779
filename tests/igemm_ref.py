"""Float64 references, input families, bounds and case lists for csrc/igemm.hip (every conv3x3 / conv1x1 / linear route of igemm_plan, csrc/igemm_plan.h) and the small-Cout
conv_out kernels of csrc/misc.hip.  Plain torch on the CPU; shares no code with consolver_amd/ops.py.  Yardstick of tests/test_igemm_forms_gpu.py, pinned on the
CPU by tests/test_igemm_ref.py.

References
    conv_fp64    NHWC in and out through F.conv2d in double, in this order: concat on channels, nearest x2, zero padding (1,1,1,1) or (0,1,0,1), the conv, bias,
                 the per-sample time embedding (1 or B rows), the residual as res + res_lo.  Also S = conv(|x|, |w|) + |bias| + |temb| + |res| + |res_lo|.
    linear_fp64  x [M, K] (+ x_lo: the split A operand, value x + x_lo) times w [N, K]; GEGLU reads w / bias in the PACKED order of cs_op_geglu_pack -- row blocks of
                 (16 value | 16 gate) -- and returns value x erf-GELU(gate) in the natural column order: out[:, 16 P + i] = v x gelu(g) of packed rows 32 P + i and
                 32 P + 16 + i.

Exact family
    x in {-2 .. 2}, w in {-1, 0, 1}, bias and temb in {-3 .. 3}, res in {-8 .. 8}, lo planes in quarters {-1 .. 1}; x and w thinned with K (density()) so that the
    sums stay small.  Every reference value is then a multiple of 1/4 (an integer without lo planes) of magnitude below 2048 -- check_exact() ASSERTS that on the
    reference.  Such values and all their partial sums have at most 13 significant bits: every fp32 sum is exact in any order, split-K partials included, so
    the kernel's fp32 value equals the reference and its output must equal rnd16(reference) bit for bit (the reference itself without lo planes: integers
    below 2048 are fp16 numbers); a lo plane out must equal reference - rnd16(reference), which is exact in fp16.

Random family, per element (after flux_ref.g2_values)
    |out - rnd16(ref)|  <=  g S + ulp16(|ref| + g S),      g = (Ktot + A + splits) 2^-23,   A = number of epilogue addends (bias, temb, res, res_lo).
    Why: the kernel's fp32 value f is a sum of Ktot exact products and A addends in some order, over `splits` partial accumulators: |f - ref| <= g S with one
    relative 2^-23 per operation (2^-23, not 2^-24: the matrix core's internal rounding is not assumed to be round-to-nearest).  Rounding to fp16 is monotone, so
    rnd16(f) lies between rnd16(ref - g S) and rnd16(ref + g S): within g S + one ulp16 at |ref| + g S of rnd16(ref).  Both epilogue paths (the fp16 patch for
    bias only, the fp32 patch for temb / res / lo planes) round the fp32 value ONCE, so one rule serves both.
    Split outputs (hi, lo):  |hi + lo - ref| <= g S + 2^-21 |ref|  and  |lo| <= ulp16(hi)  (hi = rnd16(f), lo = rnd16(f - hi): |f - hi| <= ulp16(f) / 2 and the
    rounding of lo is 2^-11 of that, 2^-22 |f|; 2^-21 leaves a factor two).
    Sub-pixel form: the 1 / 2 / 4 taps that land on one input pixel are summed in fp32 and rounded to fp16 once on the host: a summed weight is off by at most
    2^-11 (sum of its |taps|) (+ 3 fp32 additions, 2^-22), so the result by at most (2^-11 + 2^-22) conv(|x|, |w|): `extra` of bound().

GEGLU (random family): value v = x w_v + b_v and gate t = x w_g + b_g are fp32 sums with |v32 - v| <= g S_v and |t32 - t| <= g S_g.  The kernel's G(t) = gelu_erf4(t)
    (csrc/igemm.hip): x Phi(x), Phi = 1/2 + c Q(c^2), c = clamp(x, +-4.5), Q of degree 9 in u = c^2.  Its comment states |x Phi_poly(x) - gelu(x)| <= 8.2e-5 in exact
    arithmetic.  That holds inside the clamp (and up to |x| = 10.6); beyond it Phi_poly is frozen at P0 = Phi_poly(-4.5) = 1/2 - 4.5 Q(20.25) = 7.75e-6 (resp. 1 - P0)
    while the true Phi goes on to 0 (resp. 1), so the error is |x| P0 at most: Epoly(x) = max(8.2e-5, |x| P0), P0 from the coefficients.  Evaluated in fp32: Horner
    with 9 steps is off by at most 18 x 2^-24 Qabs(u) (Qabs = the polynomial of the |coefficients|; Higham, gamma_2n), the rounding of u = c c moves Q by at most 9 x 2^-24 Qabs(u), c Q + 1/2 and the final product add 3 roundings of values <= 1: in all
    E(t) = Epoly(t) + |t| (32 x 2^-24 |c| Qabs(c^2) + 2^-22).  erf-GELU's derivative lies in [-0.13, 1.13] (pinned by test_igemm_ref), so
        |v32 G(t32) - v gelu(t)| <= g S_v (|gelu(t)| + d) + |v| d + 2^-23 |v gelu(t)|,   d = 1.13 g S_g + E(|t| + g S_g),
    and the output is within that + one ulp16 of rnd16(ref).  Nothing here is measured from the kernel.

GroupNorm statistics (gn_stats [B, HoWo / 64, N / 2, 2]): which pixels a slot holds is the kernel's business (LinearRows: 64 consecutive rows, PatchRows: a quarter
    patch, SubRows: phase-major), so the check is on totals: per (sample, channel pair) the sum over slots of (sum, sum of squares) equals the (sum, sum of squares)
    of the STORED fp16 output.  Exactly when the totals are integers below 2^24 (asserted on the reference in the exact family), else within
    128 (HoWo / 64) 2^-24 sum(out^2) -- the number of elements times the fp32 unit roundoff times the sum of squares.  The kernels STORE their slot (they do not
    accumulate; igemm_epilogue_impl, splitk_reduce_stats_kernel and the statistics pass alike), so the test pre-fills the buffer with NaN and every slot must have
    been written.

Row statistics (row_stats [M, G, 2], G from the route record): per row and column group the (sum, sum of squares) of hi + lo over the group's N / G columns, same
    two rules with N / G elements.
"""
import math

import torch
import torch.nn.functional as F

from tests.flux_ref import F16, NAN, ulp_at, rnd

GELU_ERF_DERIV_MAX = 1.13
GELU_POLY_ERR = 8.2e-5
# the coefficients of Q in gelu_erf4 (csrc/igemm.hip), lowest degree first
GELU_Q = (3.989399076e-01, -6.646580249e-02, 9.930972010e-03, -1.158194733e-03, 1.050455248e-04, -7.229871699e-06, 3.595010583e-07, -1.199396227e-08,
          2.374692942e-10, -2.092490677e-12)


def rnd16(x):
    return rnd(x, F16)


def ulp16(x):
    return ulp_at(x, F16)


def pack(w):
    """[N, Cin, kh, kw] -> [N, kh * kw * Cin] fp16, tap-major / channel-minor: the row layout the kernels read"""
    return w.reshape(w.shape[0], w.shape[1], -1).permute(0, 2, 1).reshape(w.shape[0], -1).contiguous().to(F16)


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def conv_fp64(x0, x1, w, bias, temb, res, res_lo, taps=9, stride=1, upsample=False, pad_after_only=False):
    """x0 [B, H, W, c0] (x1 [B, H, W, c1] or None), w [N, c0 + c1, k, k] (k = 3 for taps 9, 1 for taps 1) -> (ref, S), both float64 [B, Ho, Wo, N]"""
    x = _nchw(x0) if x1 is None else torch.cat([_nchw(x0), _nchw(x1)], 1)
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    if taps == 9:
        x = F.pad(x, (0, 1, 0, 1) if pad_after_only else (1, 1, 1, 1))
    wd = w.double()
    assert wd.shape[-1] == (3 if taps == 9 else 1)
    y = F.conv2d(x, wd, stride=stride).permute(0, 2, 3, 1)
    S = F.conv2d(x.abs(), wd.abs(), stride=stride).permute(0, 2, 3, 1)
    if bias is not None:
        y, S = y + bias.double(), S + bias.double().abs()
    if temb is not None:
        t = temb.double()[:, None, None, :]                       # 1 or B rows
        y, S = y + t, S + t.abs()
    if res is not None:
        r = res.double() + (res_lo.double() if res_lo is not None else 0.0)
        y, S = y + r, S + res.double().abs() + (res_lo.double().abs() if res_lo is not None else 0.0)
    return y.contiguous(), S.contiguous()


def conv_im2col(x0, x1, w, bias, temb, res, res_lo, taps=9, stride=1, upsample=False, pad_after_only=False):
    """the same value as conv_fp64 from explicit loops over output pixels and taps (tests/test_igemm_ref.py compares the two)"""
    x = x0.double() if x1 is None else torch.cat([x0.double(), x1.double()], -1)
    B, H, W, Cc = x.shape
    Hs, Ws = (2 * H, 2 * W) if upsample else (H, W)                 # the image the filter slides over
    k = 3 if taps == 9 else 1
    lo = 0 if (pad_after_only or taps == 1) else 1
    Ho = (Hs + (2 if taps == 9 and not pad_after_only else (1 if taps == 9 else 0)) - k) // stride + 1
    Wo = (Ws + (2 if taps == 9 and not pad_after_only else (1 if taps == 9 else 0)) - k) // stride + 1
    wd = w.double()
    out = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float64)
    for yo in range(Ho):
        for xo in range(Wo):
            for dy in range(k):
                for dx in range(k):
                    yi, xi = yo * stride - lo + dy, xo * stride - lo + dx
                    if not (0 <= yi < Hs and 0 <= xi < Ws):
                        continue
                    px = x[:, yi // 2, xi // 2] if upsample else x[:, yi, xi]
                    out[:, yo, xo] += px @ wd[:, :, dy, dx].T
    if bias is not None:
        out += bias.double()
    if temb is not None:
        for b in range(B):
            out[b] += temb.double()[b if temb.shape[0] > 1 else 0]
    if res is not None:
        out += res.double()
        if res_lo is not None:
            out += res_lo.double()
    return out


def gelu_erf_fp64(x):
    return 0.5 * x * (1.0 + torch.special.erf(x / math.sqrt(2.0)))


def gelu_poly_err(t):
    """E(t) of the module docstring: bound of |gelu_erf4(t) in fp32 - gelu(t)| for an fp32 t"""
    c = t.abs().clamp(max=4.5)
    u = c * c
    qabs = torch.zeros_like(u)
    for a in reversed(GELU_Q):
        qabs = qabs * u + abs(a)
    q0 = 0.0
    for a in reversed(GELU_Q):
        q0 = q0 * 20.25 + a
    p0 = 0.5 - 4.5 * q0                                               # Phi_poly(-4.5)
    return torch.clamp(t.abs() * p0, min=GELU_POLY_ERR) + t.abs() * (32 * 2.0 ** -24 * c * qabs + 2.0 ** -22)


class Lin:
    pass


def linear_fp64(x, x_lo, w, bias, res, res_lo, geglu=False):
    """-> Lin with ref, S (float64 [M, N], GEGLU [M, N / 2]) and, GEGLU, the parts v, t, Sv, St the bound needs"""
    o = Lin()
    a = x.double() + (x_lo.double() if x_lo is not None else 0.0)
    aabs = x.double().abs() + (x_lo.double().abs() if x_lo is not None else 0.0)
    wd = w.double()
    y, S = a @ wd.T, aabs @ wd.abs().T
    if bias is not None:
        y, S = y + bias.double(), S + bias.double().abs()
    if geglu:
        N = w.shape[0]
        rows = torch.arange(N // 2)
        vi = (rows // 16) * 32 + rows % 16
        o.v, o.t, o.Sv, o.St = y[:, vi], y[:, vi + 16], S[:, vi], S[:, vi + 16]
        o.ref, o.S = o.v * gelu_erf_fp64(o.t), None
        return o
    if res is not None:
        y = y + res.double() + (res_lo.double() if res_lo is not None else 0.0)
        S = S + res.double().abs() + (res_lo.double().abs() if res_lo is not None else 0.0)
    o.ref, o.S = y, S
    return o


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------------------------------
def gfac(Ktot, addends, splits=1):
    return (Ktot + addends + splits) * 2.0 ** -23


def bound(ref, S, g, extra=0.0):
    """per-element bound of |out - rnd16(ref)| (module docstring); extra: an additional absolute error of the fp32 value (sub-pixel weights)"""
    e = g * S + extra
    return e + ulp16(ref.abs() + e)


def ratio(out, ref, bnd):
    """worst |out - rnd16(ref)| / bound over the elements; NaN / inf in out give inf"""
    out = out.double()
    if not bool(torch.isfinite(out).all()):
        return float("inf")
    return float(((out - rnd16(ref)).abs() / bnd).max())


def split_ratio(hi, lo, ref, S, g):
    """worst of |hi + lo - ref| / (g S + 2^-21 |ref|) and |lo| / ulp16(hi)"""
    hi, lo = hi.double(), lo.double()
    if not bool(torch.isfinite(hi).all() and torch.isfinite(lo).all()):
        return float("inf")
    a = float(((hi + lo - ref).abs() / (g * S + 2.0 ** -21 * ref.abs())).max())
    b = float((lo.abs() / ulp16(hi)).max())
    return max(a, b)


def geglu_bound(o, g):
    d = GELU_ERF_DERIV_MAX * g * o.St + gelu_poly_err(o.t.abs() + g * o.St)
    gl = gelu_erf_fp64(o.t).abs()
    e = g * o.Sv * (gl + d) + o.v.abs() * d + 2.0 ** -23 * o.ref.abs()
    return e + ulp16(o.ref.abs() + e)


def gn_totals(out):
    """out [B, Ho, Wo, N] (stored fp16 values) -> float64 [B, N / 2, 2]: (sum, sum of squares) per sample and channel pair"""
    B, N = out.shape[0], out.shape[-1]
    o = out.double().reshape(B, -1, N // 2, 2)
    return torch.stack([o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))], -1)


def gn_check(st, out, exact):
    """st [B, slots, N / 2, 2] fp32 against the stored output: None when it holds, else a message"""
    if not bool(torch.isfinite(st).all()):
        return "a statistics slot was not written (NaN left)"
    got, want = st.double().sum(dim=1), gn_totals(out)
    if exact:
        assert float(want.abs().max()) < 2.0 ** 24
        return None if torch.equal(got, want) else f"totals differ by {float((got - want).abs().max())} (exact family)"
    n = out.shape[1] * out.shape[2] * 2
    tol = n * 2.0 ** -24 * want[..., 1:2]
    bad = (got - want).abs() > tol
    return None if not bool(bad.any()) else f"totals off by {float(((got - want).abs() / tol).max()):.2f} x the tolerance"


def row_totals(v, G):
    """v float64 [M, N] -> [M, G, 2]"""
    M, N = v.shape
    g = v.reshape(M, G, N // G)
    return torch.stack([g.sum(-1), (g * g).sum(-1)], -1)


def row_check(rs_flat, v, G, exact):
    """rs_flat: the statistics buffer as the kernel wrote it, [M][G][2] contiguous from its start; v = hi + lo float64 [M, N]"""
    M, N = v.shape
    got = rs_flat.reshape(-1)[:M * G * 2].double().reshape(M, G, 2)
    if not bool(torch.isfinite(got).all()):
        return "a row-statistics entry was not written (NaN left)"
    want = row_totals(v, G)
    if exact:
        assert float(want.abs().max()) < 2.0 ** 24
        return None if torch.equal(got, want) else f"row statistics differ by {float((got - want).abs().max())} (exact family)"
    tol = (N // G) * 2.0 ** -24 * want[..., 1:2]
    bad = (got - want).abs() > tol
    return None if not bool(bad.any()) else f"row statistics off by {float(((got - want).abs() / tol).max()):.2f} x the tolerance"


# ---- input families -------------------------------------------------------------------------------------------------------------------------------------------
def density(K):
    """P(nonzero) of the exact family's x and w: a term x w has variance (2 d)(2/3 d), so a sum of K of them has sigma <= sqrt(4/3 x 100) = 11.5 (after
    flux_ref.density_for)"""
    return min(1.0, math.sqrt(100.0 / K))


class Family:
    def __init__(self, family, seed):
        assert family in ("exact", "random")
        self.exact, self.g = family == "exact", torch.Generator().manual_seed(seed)

    def _int(self, lo, hi, shape, d=1.0):
        v = torch.randint(lo, hi + 1, shape, generator=self.g).float()
        return v * (torch.rand(shape, generator=self.g) < d) if d < 1.0 else v

    def x(self, shape, K):
        return (self._int(-2, 2, shape, density(K)) if self.exact else torch.randn(shape, generator=self.g)).to(F16)

    def w(self, shape, K):
        """shape [N, Cin, k, k] or [N, K]; K = the length of the sum"""
        return (self._int(-1, 1, shape, density(K)) if self.exact else torch.randn(shape, generator=self.g) * K ** -0.5).to(F16)

    def vec(self, shape, scale=0.5):
        return (self._int(-3, 3, shape) if self.exact else torch.randn(shape, generator=self.g) * scale).to(F16)

    def res(self, shape):
        return (self._int(-8, 8, shape) if self.exact else torch.randn(shape, generator=self.g)).to(F16)

    def lo(self, hi):
        """the lo plane of a split tensor: quarters in the exact family, below half an ulp of hi otherwise"""
        if self.exact:
            return (self._int(-4, 4, hi.shape) / 4).to(F16)
        return ((torch.rand(hi.shape, generator=self.g) - 0.5).double() * ulp16(hi.double())).to(F16)


def check_exact(ref, quarters=False):
    """the exact family's condition on a reference: multiples of 1 (1/4 with lo planes) of magnitude below 2048"""
    q = ref * (4.0 if quarters else 1.0)
    assert torch.equal(q, q.round()), "exact family: the reference is not on the grid"
    assert float(ref.abs().max()) < 2048.0, f"exact family: |reference| reaches {float(ref.abs().max())}"


# ---- cases (shared by the CPU pin and the GPU module) ----------------------------------------------------------------------------------------------------------
class ConvCase:
    """one conv launch: geometry, epilogue flags, knobs, and the route the dispatcher must take (None fields are not asserted)"""
    def __init__(self, name, B, H, W, c0, N, c1=0, taps=9, stride=1, up=False, bias=True, temb=0, res=False, gn=False, splitk=True, knobs=(), family="generic",
                 cols=None, variant=None, splits=1, gn_done=None, fallback=0, api="conv2d"):
        self.__dict__.update(locals())
        del self.__dict__["self"]

    def __repr__(self):
        return self.name

    @property
    def cin(self):
        return self.c0 + self.c1

    @property
    def out_hw(self):
        if self.up:
            return 2 * self.H, 2 * self.W
        return (self.H // 2, self.W // 2) if self.stride == 2 else (self.H, self.W)

    def inputs(self, family, seed=0):
        """CPU tensors of one family: dict(x0, x1, w [N, cin, k, k], bias, temb, res)"""
        f = Family(family, 7919 * seed + 13)
        k = 3 if self.taps == 9 else 1
        K = self.taps * self.cin
        Ho, Wo = self.out_hw
        d = dict(x0=f.x((self.B, self.H, self.W, self.c0), K), x1=f.x((self.B, self.H, self.W, self.c1), K) if self.c1 else None,
                 w=f.w((self.N, self.cin, k, k), K), bias=f.vec((self.N,)) if self.bias else None,
                 temb=f.vec((self.B if self.temb == "B" else 1, self.N)) if self.temb else None,
                 res=f.res((self.B, Ho, Wo, self.N)) if self.res else None)
        return d

    def reference(self, d, res_lo=None):
        return conv_fp64(d["x0"], d["x1"], d["w"], d["bias"], d["temb"], d["res"], res_lo, self.taps, self.stride, self.up, self.api == "conv_down")

    @property
    def addends(self):
        return int(self.bias) + int(bool(self.temb)) + int(self.res)


HALO0 = (("conv_halo", 0),)
HALO = (("conv_halo", 2), ("conv_lw", 0))
WIDE = (("conv_halo", 3), ("conv_lw", 0))
LW = (("conv_halo", 2), ("conv_lw", 1))
LWP = (("conv_halo", 2), ("conv_lw", 2))


def _generic_cases():
    c = []
    geo = [(1, 1, 1), (1, 1, 3), (1, 3, 5), (1, 3, 43), (2, 8, 16), (1, 16, 8), (3, 5, 7)]
    chans = [(64, 0), (192, 0), (64, 128), (128, 64)]
    epis = [dict(bias=True), dict(bias=False), dict(temb=1), dict(temb="B"), dict(res=True), dict(temb="B", res=True)]
    i = 0
    for B, H, W in geo:                                               # every geometry x every channel form, N and the epilogue forms rotating through them
        for c0, c1 in chans:
            N = (128, 160, 640)[i % 3]
            e = epis[i % len(epis)]
            c.append(ConvCase(f"g{B}x{H}x{W}_c{c0}+{c1}_n{N}_{i % len(epis)}", B, H, W, c0, N, c1=c1, knobs=HALO0, cols=128 if N % 128 == 0 else 160, variant=32, **e))
            i += 1
    for j, e in enumerate(epis):                                      # every epilogue form at the M = 129 geometry and at 3 samples, both tile widths
        c.append(ConvCase(f"g_m129_e{j}", 1, 3, 43, 64, 160, knobs=HALO0, cols=160, variant=32, **e))
        c.append(ConvCase(f"g_b3_e{j}", 3, 5, 7, 64, 128, knobs=HALO0, cols=128, variant=32, **e))
    # GroupNorm statistics from the generic epilogue (LinearRows: 64 consecutive rows per slot)
    c.append(ConvCase("g_gn_2x8x16", 2, 8, 16, 64, 128, gn=True, res=True, knobs=HALO0, cols=128, variant=32, gn_done=1))
    c.append(ConvCase("g_gn_3x8x8_n160", 3, 8, 8, 64, 160, gn=True, splitk=False, knobs=HALO0, cols=160, variant=32, gn_done=1))
    return c


def _stride_up_cases():
    c = []
    for H, W in [(2, 2), (4, 6), (16, 8), (6, 10)]:
        c.append(ConvCase(f"s2_{H}x{W}", 2, H, W, 64, 128, stride=2, temb="B", knobs=HALO0, cols=128, variant=32))
        c.append(ConvCase(f"s2_{H}x{W}_n160", 1, H, W, 192, 160, stride=2, res=True, knobs=HALO0, cols=160, variant=32))
    for H, W in [(1, 1), (3, 5), (4, 8)]:
        c.append(ConvCase(f"up_{H}x{W}", 2, H, W, 64, 160, c1=128, up=True, knobs=HALO0, cols=160, variant=32))
        c.append(ConvCase(f"up_{H}x{W}_c128+64", 1, H, W, 128, 128, c1=64, up=True, res=True, knobs=HALO0, cols=128, variant=32))
    c.append(ConvCase("down_16x8", 2, 16, 8, 64, 128, stride=2, api="conv_down", cols=128, variant=32))
    c.append(ConvCase("down_5x7", 1, 5, 7, 128, 160, stride=2, api="conv_down", cols=160, variant=32))      # odd sizes: the floor is right for this padding
    return c


def _generic_splitk_cases():
    c = []
    for cin, sp in [(128, 2), (256, 4), (512, 8)]:
        c.append(ConvCase(f"gsk_c{cin}", 1, 16, 16, cin, 128, stride=2, temb=1, res=True, knobs=HALO0, cols=128, variant=32, splits=sp))
        c.append(ConvCase(f"gsk_c{cin}_gn", 1, 16, 16, cin, 160, stride=2, gn=True, knobs=HALO0, cols=160, variant=32, splits=sp, gn_done=1))     # HoWo = 64: the reduce leaves the statistics
    c.append(ConvCase("gsk_16x32_gn", 1, 16, 32, 128, 128, stride=2, gn=True, knobs=HALO0, cols=128, variant=32, splits=2, gn_done=0, fallback=1))        # HoWo = 128: statistics pass
    c.append(ConvCase("gsk_b2_gn", 2, 16, 16, 256, 128, stride=2, gn=True, res=True, knobs=HALO0, cols=128, variant=32, splits=4, gn_done=1))
    return c


HALO_GEO = [(1, 8, 8), (4, 8, 8), (5, 8, 8), (1, 16, 8), (3, 8, 16), (1, 32, 8), (1, 64, 8), (2, 16, 16), (1, 16, 32), (1, 32, 16), (1, 48, 80)]
HALO_UP_GEO = [(3, 4, 8), (1, 8, 8), (1, 8, 16), (2, 16, 8)]


def _halo_cases():
    c = []
    epis = [dict(bias=True), dict(temb="B"), dict(res=True), dict(temb=1, res=True), dict(gn=True)]
    for i, (B, H, W) in enumerate(HALO_GEO):
        N, cin = (128, 160)[i % 2], (64, 128)[(i // 2) % 2]
        # (cin 128 would split its two chunks when the scratch is there: splitk=False keeps these the unsplit kernels)
        c.append(ConvCase(f"h{B}x{H}x{W}_c{cin}_n{N}", B, H, W, cin, N, knobs=HALO, family="halo", cols=N, variant=0, splitk=False, **epis[i % len(epis)]))
        Nw = (256, 320)[i % 2]
        c.append(ConvCase(f"hw{B}x{H}x{W}_n{Nw}", B, H, W, 64, Nw, knobs=WIDE, family="halo", cols=Nw, variant=0, splitk=False, **epis[(i + 1) % len(epis)]))
    for i, (B, H, W) in enumerate(HALO_UP_GEO):
        N = (160, 128)[i % 2]
        c.append(ConvCase(f"hup{B}x{H}x{W}_n{N}", B, H, W, 64, N, up=True, knobs=HALO, family="halo", cols=N, variant=1, splitk=False, gn=i == 1))
        Nw = (320, 256)[i % 2]
        c.append(ConvCase(f"hwup{B}x{H}x{W}_n{Nw}", B, H, W, 128, Nw, up=True, knobs=WIDE, family="halo", cols=Nw, variant=1, splitk=False))
    for cin, sp in [(128, 2), (256, 4), (512, 8)]:
        c.append(ConvCase(f"hsk8_c{cin}", 1, 8, 8, cin, 160, temb=1, res=True, gn=True, knobs=HALO, family="halo", cols=160, variant=0, splits=sp, gn_done=1))
        c.append(ConvCase(f"hsk16_c{cin}", 1, 16, 16, cin, 128, gn=cin == 256, knobs=HALO, family="halo", cols=128, variant=0, splits=sp,
                          gn_done=0 if cin == 256 else None, fallback=1 if cin == 256 else 0))
    return c


def _lw_cases():
    c = []
    A = lambda *a, **k: c.append(ConvCase(*a, family="conv3_lw", **k))
    A("lw_fast160", 2, 16, 16, 64, 160, temb="B", knobs=LW, cols=160, variant=0, splitk=False)
    A("lw_fast160_res_gn", 1, 16, 32, 128, 160, res=True, gn=True, knobs=LW, cols=160, variant=0, splitk=False, gn_done=1)
    A("lw_fast160_48x80", 1, 48, 80, 64, 160, knobs=LW, cols=160, variant=0)
    A("lw_plain160", 2, 16, 16, 64, 160, temb="B", res=True, knobs=LWP, cols=160, variant=1, splitk=False)
    A("lw_plain160_8x16", 3, 8, 16, 64, 160, res=True, knobs=LW, cols=160, variant=1, splitk=False)        # TH = 8: not the FAST geometry
    A("lw_plain160_64x8", 1, 64, 8, 64, 160, temb=1, knobs=LW, cols=160, variant=1, splitk=False)
    A("lw_fast8_b5", 5, 8, 8, 64, 160, temb="B", res=True, gn=True, knobs=LW, cols=160, variant=10, gn_done=1)
    A("lw_fast8_b4", 4, 8, 8, 128, 320, res=True, knobs=LW, cols=160, variant=10, splitk=False)
    A("lw_8x8_plain", 5, 8, 8, 64, 160, temb="B", knobs=LWP, cols=160, variant=1)
    A("lw_fast128", 1, 16, 16, 64, 128, res=True, knobs=LW, cols=128, variant=6)
    A("lw_fast128_n256", 1, 32, 16, 64, 256, gn=True, knobs=LW, cols=128, variant=6, gn_done=1)
    A("lw_plain128", 1, 16, 16, 64, 128, temb=1, knobs=LWP, cols=128, variant=7)
    A("lw_plain128_8x8", 5, 8, 8, 64, 128, res=True, knobs=LW, cols=128, variant=7)
    A("lw_up_fast160", 2, 8, 8, 64, 160, up=True, knobs=LW, cols=160, variant=5)
    A("lw_up_fast160_8x16", 1, 8, 16, 128, 160, up=True, gn=True, knobs=LW, cols=160, variant=5, splitk=False, gn_done=1)
    A("lw_up_plain160", 3, 4, 8, 64, 160, up=True, knobs=LW, cols=160, variant=2)
    A("lw_up_plain160_knob", 1, 8, 8, 64, 160, up=True, knobs=LWP, cols=160, variant=2)
    A("lw_up_fast128", 1, 8, 8, 64, 128, up=True, knobs=LW, cols=128, variant=9)
    A("lw_up_plain128", 3, 4, 8, 64, 128, up=True, knobs=LW, cols=128, variant=8)
    for cin, sp in [(128, 2), (256, 4), (512, 8)]:
        A(f"lw_sk8_c{cin}", 1, 8, 8, cin, 160, temb=1, res=True, gn=True, knobs=LW, cols=160, variant=10, splits=sp, gn_done=1)
    A("lw_sk16_c256", 1, 16, 16, 256, 128, res=True, knobs=LW, cols=128, variant=6, splits=4)
    A("lw_n640_is_160", 1, 16, 16, 64, 640, knobs=LW, cols=160, variant=0)                                # N = 640: 160-column tiles here ...
    c.append(ConvCase("generic_n640_is_128", 1, 16, 16, 64, 640, knobs=HALO0, cols=128, variant=32))         # ... and 128-column tiles on the generic kernel
    return c


GENERIC_CASES = _generic_cases()
STRIDE_UP_CASES = _stride_up_cases()
GENERIC_SPLITK_CASES = _generic_splitk_cases()
HALO_CASES = _halo_cases()
LW_CASES = _lw_cases()
ALL_CONV_CASES = GENERIC_CASES + STRIDE_UP_CASES + GENERIC_SPLITK_CASES + HALO_CASES + LW_CASES

SUB_CASES = [   # B, Hi, Wi, cin, N, sub-table index
    (1, 16, 16, 64, 160, 0), (5, 16, 16, 64, 160, 0), (1, 16, 32, 128, 160, 0), (1, 8, 8, 64, 160, 1), (5, 8, 8, 128, 320, 1), (1, 16, 32, 64, 128, 2), (2, 16, 16, 64, 256, 2),
]

LINEAR_M = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 321, 513)
LINEAR_K = (64, 128, 320)
# route name -> (knobs, N, family, tile columns, variant, row-statistics groups of N)
LINEAR_ROUTES = {
    "generic128": ((("gemm_big", 0),), 256, "generic", 128, 0),
    "generic160": ((("gemm_big", 0),), 320, "generic", 160, 0),
    "big320": ((("gemm_big", 2), ("gemm_w8", 0)), 320, "gemm_big", 320, 0),
    "w8": ((("gemm_big", 2), ("gemm_w8", 1)), 320, "gemm_w8", 320, 0),
    "big160": ((("gemm_big", 3), ("gemm_lw", 0)), 160, "gemm_big", 160, 0),
    "lw": ((("gemm_big", 3), ("gemm_lw", 1)), 160, "gemm_lw", 160, 0),
}
# GEGLU: (knobs, N, family, tile columns, variant)
GEGLU_ROUTES = [
    ((("gemm_big", 0),), 256, "generic", 128, 16), ((("gemm_big", 0),), 512, "generic", 128, 16),
    ((), 320, "gemm_w8", 320, 1),                                    # N % 128 != 0: the 320-column kernels whatever the tile count
    ((("gemm_big", 2), ("gemm_w8", 0)), 320, "gemm_big", 320, 1), ((("gemm_big", 2), ("gemm_w8", 1)), 320, "gemm_w8", 320, 1),
    ((("gemm_big", 2), ("gemm_w8", 1)), 640, "gemm_w8", 320, 1),
]
CONV_OUT_CASES = [   # B, H, W, cin, cout
    (2, 16, 16, 64, 3), (1, 16, 32, 128, 3), (1, 16, 16, 64, 4), (2, 16, 32, 64, 4), (1, 16, 16, 128, 8), (1, 16, 32, 64, 8), (2, 16, 16, 64, 16), (1, 16, 32, 64, 16),
    (2, 8, 8, 64, 4), (1, 5, 7, 40, 3),                              # off the patch kernels (one wave per pixel)
]
