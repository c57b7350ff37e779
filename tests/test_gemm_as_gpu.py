"""gemm_as_kernel (csrc/igemm.hip): the K = 320 linear layers with the activations stationary in registers, route family "gemm_as" (knob gemm_as; 2 = take it
whenever the layer is eligible).  Every case forces the route, asserts it with ops.igemm_last_route() (family, 32-column slices, variant 2 LNM + GEGLU), keeps NaN
margins around the output and restores the knobs in a finally.

Shapes: K = 320; M = 1, 63, 64, 65 (the edge of a wave's 64 rows), 511, 512, 513 (the edge of a workgroup's 512), 1100 (two full workgroups and a ragged third);
N = 32, 64, 96 (one slice, one full 64-column patch, a patch and a half) and 960 (QKV); GEGLU N = 64, 320, 640 in packed columns (one slice = 16 outputs: half a
patch, two patches and a half, five).

Bounds (random family; per element, RATIO = worst |out - rnd16(ref)| / bound, asserted <= 1 -- tests/igemm_ref.py):
  * bias / no bias: igemm_ref.bound with g = gfac(320, addends), the rule of the gemm_w8 family these layers ran on;  GEGLU: igemm_ref.geglu_bound, likewise;
  * folded LayerNorm: the reference is  ref = rstd (y - mean s) + b'  in float64 from the operands the kernel reads (fp16 x and W', fp32 s, b' and row statistics
    (s1, s2); mean = s1 / C, var = s2 / C - mean^2, rstd = (var + eps)^-1/2).  The kernel's fp32 arithmetic (ln_tile_prologue + the epilogue) is
        mean32 = s1 * fl(1 / C)                               relative error dm <= 2^-23 (two roundings)
        var32  = fma(-mean32, mean32, s2 * fl(1 / C))         absolute error dv <= 2^-23 s2 / C + 2^-22 mean^2 + 2^-24 var
        rstd32 = v_rsq_f32(max(var32, 0) + eps)               relative error dr <= dv / (var + eps) + 2^-24 + 2^-23   (the add, one ulp of the instruction; dv taken
                                                                whole, not halved, for the second-order terms)
        mr32   = mean32 * rstd32                              relative error dm + dr + 2^-24
        val    = fma(acc, rstd32, fma(-mr32, s, b'))          |acc - y| <= g S,  g = gfac(320, 0)
    so  |val - ref| <= e = rstd g S + dr rstd |y| + (dm + dr + 2^-24) |mean rstd s| + 2^-24 (|b' - mean rstd s| + |ref|)  and the bound is e + ulp16(|ref| + e).
    With GEGLU the value and gate columns each carry that e, which enters igemm_ref.geglu_bound in the place of g S_v and g S_g (called with g = 1, S = e).
Nothing in these bounds is measured from the kernel.

Bit identity: where gemm_w8_kernel takes the shape (N % 320 == 0; knobs gemm_big 2, gemm_w8 1, gemm_as 0) the two outputs are equal bit for bit -- same MFMA shape,
k steps 0 .. 9 in order into one accumulator chain, the same epilogue expressions -- on random data and on rows with a DC offset of which a few are scaled by 100.
"""
import pytest
import torch

from consolver_amd import ops
from tests import igemm_ref as R
from tests.test_igemm_forms_gpu import guarded, margins_intact, same_bits, dev, route_is, report, knobs, DEV, F16

pytestmark = pytest.mark.gpu
K = 320
MS = (1, 63, 64, 65, 511, 512, 513, 1100)
AS = (("gemm_as", 2),)
W8 = (("gemm_big", 2), ("gemm_w8", 1), ("gemm_as", 0))
EPS = 1e-5


def run(x, w, bias, M, N, geglu=False, ln=None, kn=AS):
    """one launch under the knobs kn into a NaN-guarded buffer -> (buffer, output view, route); ln = (s, b', statistics) on the device"""
    obuf, out = guarded(M, N // 2 if geglu else N)
    try:
        with knobs(kn):
            if ln is None:
                ops.linear(x, w, bias, geglu=geglu, out=out)
            else:
                ops.linear_ln(x, w, ln[0], ln[1], ln[2], 1, eps=EPS, geglu=geglu, out=out)
            route = ops.igemm_last_route()
    finally:
        ops.reset_tuning()
    torch.cuda.synchronize()
    return obuf, out, route


def ln_operands(f, M, N, geglu, x=None):
    """a folded-LayerNorm layer: raw rows x, folded weights / s / b' (packed for GEGLU) and the row statistics the kernel reads"""
    if x is None:
        x = (torch.randn((M, K), generator=f.g) * 1.5 + 0.3).to(F16)
    w, b = f.w((N, K), K), f.vec((N,))
    gam, bet = (1.0 + 0.1 * torch.randn(K, generator=f.g)).to(F16), (0.1 * torch.randn(K, generator=f.g)).to(F16)
    if geglu:
        w, b = ops.geglu_pack(w, b)
    wf, sf, bf = ops.ln_fold_pack(w, b, gam, bet)
    xd = dev(x)
    return x, xd, wf, sf, bf, ops.row_stats(xd)


def ln_reference(x, wf, sf, bf, st):
    """-> (ref, e) float64 [M, N]: the module docstring's reference and error term, columns in the order of wf's rows"""
    s1, s2 = st[:, 0, 0].cpu().double()[:, None], st[:, 0, 1].cpu().double()[:, None]
    mean = s1 / K
    var = (s2 / K - mean * mean).clamp_min(0.0)
    rstd = (var + EPS).rsqrt()
    y, S = x.double() @ wf.double().T, x.double().abs() @ wf.double().abs().T
    s, b = sf.double()[None, :], bf.double()[None, :]
    inner = b - mean * rstd * s
    ref = rstd * y + inner
    dm = 2.0 ** -23
    dv = 2.0 ** -23 * s2 / K + 2.0 ** -22 * mean * mean + 2.0 ** -24 * var
    dr = dv / (var + EPS) + 2.0 ** -24 + 2.0 ** -23
    e = rstd * R.gfac(K, 0) * S + dr * rstd * y.abs() + (dm + dr + 2.0 ** -24) * (mean * rstd * s).abs() + 2.0 ** -24 * (inner.abs() + ref.abs())
    return ref, e


def geglu_parts(y, e_or_s, N):
    """packed columns (16 value | 16 gate) -> igemm_ref.Lin with v, t, Sv, St, ref in the natural output order"""
    rows = torch.arange(N // 2)
    vi = (rows // 16) * 32 + rows % 16
    o = R.Lin()
    o.v, o.t, o.Sv, o.St = y[:, vi], y[:, vi + 16], e_or_s[:, vi], e_or_s[:, vi + 16]
    o.ref, o.S = o.v * R.gelu_erf_fp64(o.t), None
    return o


def test_0_one_workgroup_plain_first():
    """the smallest launch, alone and first: one workgroup, two slices, one patch flush -- a barrier or wait mistake shows here under this test's own time limit"""
    f = R.Family("random", 7)
    x, w, b = f.x((64, K), K), f.w((64, K), K), f.vec((64,))
    o = R.linear_fp64(x, None, w, b, None, None)
    obuf, out, route = run(dev(x), dev(w), dev(b), 64, 64)
    route_is(route, "gemm_as", 32, 0, 1)
    assert margins_intact(obuf)
    report("gemm_as", "M 64 N 64 bias", R.ratio(out.cpu(), o.ref, R.bound(o.ref, o.S, R.gfac(K, 1))))


@pytest.mark.parametrize("N", (32, 64, 96, 960))
@pytest.mark.parametrize("form", ("bias", "nobias", "ln"))
def test_plain_forms_at_every_row_edge(form, N):
    for M in MS:
        for family in (("exact", "random") if form != "ln" else ("random",)):
            f = R.Family(family, 100 * M + N)
            if form == "ln":
                x, xd, wf, sf, bf, st = ln_operands(f, M, N, False)
                ref, e = ln_reference(x, wf, sf, bf, st)
                obuf, out, route = run(xd, dev(wf), None, M, N, ln=(dev(sf), dev(bf), st))
                route_is(route, "gemm_as", 32, 2, 1)
                assert margins_intact(obuf), (form, M, N)
                report("gemm_as_ln", f"M {M} N {N}", R.ratio(out.cpu(), ref, e + R.ulp16(ref.abs() + e)))
                continue
            x, w = f.x((M, K), K), f.w((N, K), K)
            b = f.vec((N,)) if form == "bias" else None
            o = R.linear_fp64(x, None, w, b, None, None)
            obuf, out, route = run(dev(x), dev(w), dev(b), M, N)
            route_is(route, "gemm_as", 32, 0, 1)
            assert margins_intact(obuf), (form, M, N)
            if family == "exact":
                R.check_exact(o.ref)
                assert same_bits(out, o.ref.to(F16)), (form, M, N, int((out.cpu().double() != o.ref).sum()))
            else:
                report("gemm_as", f"{form} M {M} N {N}", R.ratio(out.cpu(), o.ref, R.bound(o.ref, o.S, R.gfac(K, int(b is not None)))))


@pytest.mark.parametrize("N", (64, 320, 640))
@pytest.mark.parametrize("form", ("bias", "ln"))
def test_geglu_forms_at_every_row_edge(form, N):
    for M in MS:
        f = R.Family("random", 100 * M + N + 1)
        if form == "ln":
            x, xd, wf, sf, bf, st = ln_operands(f, M, N, True)
            y, e = ln_reference(x, wf, sf, bf, st)
            o = geglu_parts(y, e, N)
            obuf, out, route = run(xd, dev(wf), None, M, N, geglu=True, ln=(dev(sf), dev(bf), st))
            route_is(route, "gemm_as", 32, 3, 1)
            assert margins_intact(obuf), (form, M, N)
            report("gemm_as_ln_geglu", f"M {M} N {N}", R.ratio(out.cpu(), o.ref, R.geglu_bound(o, 1.0)))
            continue
        x, w, b = f.x((M, K), K), f.w((N, K), K), f.vec((N,))
        wp, bp = ops.geglu_pack(w, b)
        o = R.linear_fp64(x, None, wp, bp, None, None, geglu=True)
        obuf, out, route = run(dev(x), dev(wp), dev(bp), M, N, geglu=True)
        route_is(route, "gemm_as", 32, 1, 1)
        assert margins_intact(obuf), (form, M, N)
        report("gemm_as_geglu", f"M {M} N {N}", R.ratio(out.cpu(), o.ref, R.geglu_bound(o, R.gfac(K, 1))))


def outlier_rows(f, M):
    """rows with a DC offset, a few of them scaled by 100"""
    h = torch.randn((M, K), generator=f.g) + 3.0
    for r in {0, M // 3, M - 1}:
        h[r] *= 100.0
    return h.to(F16)


@pytest.mark.parametrize("data", ("random", "outliers"))
@pytest.mark.parametrize("form,N,variant,w8_variant", [("bias", 960, 0, 0), ("nobias", 960, 0, 0), ("ln", 960, 2, 2), ("geglu", 320, 1, 1), ("geglu", 640, 1, 1),
                                                       ("ln_geglu", 320, 3, 3), ("ln_geglu", 640, 3, 3)])
def test_bit_identical_to_gemm_w8(form, N, variant, w8_variant, data):
    geglu = "geglu" in form
    for M in MS:
        f = R.Family("random", 7 * M + N)
        x = outlier_rows(f, M) if data == "outliers" else None
        if form.startswith("ln"):
            x, xd, wf, sf, bf, st = ln_operands(f, M, N, geglu, x=x)
            args = (xd, dev(wf), None, M, N)
            kw = dict(geglu=geglu, ln=(dev(sf), dev(bf), st))
        else:
            x = f.x((M, K), K) if x is None else x
            w, b = f.w((N, K), K), (f.vec((N,)) if form != "nobias" else None)
            if geglu:
                w, b = ops.geglu_pack(w, b)
            args = (dev(x), dev(w), dev(b), M, N)
            kw = dict(geglu=geglu)
        abuf, a_out, a_route = run(*args, **kw)
        wbuf, w_out, w_route = run(*args, kn=W8, **kw)
        route_is(a_route, "gemm_as", 32, variant, 1)
        route_is(w_route, "gemm_w8", 320, w8_variant, 1)
        assert margins_intact(abuf, wbuf), (form, M, N)
        if data == "random" or form.startswith("ln"):          # (rows x 100 through a plain layer overflow fp16, in both kernels alike: the bits below still have to agree)
            assert bool(torch.isfinite(w_out).all()), (form, M, N)
        assert same_bits(a_out, w_out), (form, data, M, N, int((a_out != w_out).sum()))


def test_ineligible_layers_keep_their_route():
    """gemm_as = 2 changes nothing for K = 640, a concatenated A, a residual epilogue or a lo-plane A: the route and the output bits of gemm_as = 0"""
    f = R.Family("random", 99)
    M, N = 600, 320
    x6, w6, b = f.x((M, 640), 640), f.w((N, 640), 640), f.vec((N,))
    x, w, res = f.x((M, K), K), f.w((N, K), K), f.res((M, N))
    x_lo = f.lo(x)
    xa, xb = f.x((3, 5, 9, 192), K), f.x((3, 5, 9, 128), K)

    def launches(out):
        return {
            "K 640": lambda: ops.linear(dev(x6), dev(w6), dev(b), out=out),
            "residual": lambda: ops.linear(dev(x), dev(w), dev(b), res=dev(res), out=out),
            "lo-plane A": lambda: ops.linear_x2(dev(x), dev(w), dev(b), x_lo=dev(x_lo), want_lo=False, splitk=False, out=out),
        }

    for what in ("K 640", "residual", "lo-plane A", "concat A"):
        got = []
        for v in (2, 0):
            obuf, out = guarded(3, 5, 9, N) if what == "concat A" else guarded(M, N)
            try:
                with knobs((("gemm_as", v),)):
                    if what == "concat A":
                        ops.conv2d(dev(xa), dev(w), dev(b), x1=dev(xb), taps=1, out=out)
                    else:
                        launches(out)[what]()
                    route = ops.igemm_last_route()
            finally:
                ops.reset_tuning()
            torch.cuda.synchronize()
            assert margins_intact(obuf), what
            assert bool(torch.isfinite(out).all()), what
            got.append((route, out))
        assert got[0][0].family != "gemm_as" and got[0][0] == got[1][0], (what, got[0][0], got[1][0])
        assert same_bits(got[0][1], got[1][1]), what
