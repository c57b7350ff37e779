"""CPU checks of tests/igemm_ref.py, the yardstick of tests/test_igemm_forms_gpu.py: conv_fp64 equals an independent loop-over-taps restatement for every flag
combination, the exact family's range conditions hold on the reference of EVERY conv case (and of the widest channel counts the UNet has), the GEGLU column order
equals torch's gelu on unpacked weights, the derivative / polynomial constants of the GEGLU bound hold, and the bound itself admits a float32 torch evaluation of
the same inputs (ratio <= 1), so that the reference alone stays within the rule."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import igemm_ref as R


def _tiny(family, B, H, W, c0, c1, N, taps, stride, up, temb_rows, with_res, lo, seed):
    f = R.Family(family, seed)
    k = 3 if taps == 9 else 1
    K = taps * (c0 + c1)
    x0, x1 = f.x((B, H, W, c0), K), (f.x((B, H, W, c1), K) if c1 else None)
    w, bias = f.w((N, c0 + c1, k, k), K), f.vec((N,))
    temb = f.vec((temb_rows, N)) if temb_rows else None
    Hs, Ws = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = ((Hs + 1) // 2, (Ws + 1) // 2) if stride == 2 else (Hs, Ws)
    res = f.res((B, Ho, Wo, N)) if with_res else None
    res_lo = f.lo(res) if (with_res and lo) else None
    return x0, x1, w, bias, temb, res, res_lo


FLAGS = [(taps, stride, up, pao) for taps, stride, up, pao in itertools.product((9, 1), (1, 2), (False, True), (False, True))
         if not (taps == 1 and (stride == 2 or up or pao)) and not (pao and stride != 2) and not (up and stride == 2)]


@pytest.mark.parametrize("taps,stride,up,pao", FLAGS)
def test_conv_fp64_equals_a_loop_over_pixels_and_taps(taps, stride, up, pao):
    seed = 0
    for (B, H, W), (c0, c1), temb_rows, with_res, lo in itertools.product([(1, 1, 1), (2, 3, 5), (3, 4, 2)], [(8, 0), (8, 16), (16, 8)], (0, 1, "B"),
                                                                           (False, True), (False, True)):
        if lo and not with_res:
            continue
        seed += 1
        a = _tiny("random", B, H, W, c0, c1, 8, taps, stride, up, B if temb_rows == "B" else temb_rows, with_res, lo, seed)
        if pao:                                                     # (0, 1, 0, 1) padding: floor(H / 2) rows
            Ho, Wo = H // 2, W // 2
            if Ho == 0 or Wo == 0:
                continue
            a = a[:5] + ((a[5][:, :Ho, :Wo].contiguous(), a[6][:, :Ho, :Wo].contiguous() if a[6] is not None else None) if with_res else (None, None))
        ref, S = R.conv_fp64(*a, taps=taps, stride=stride, upsample=up, pad_after_only=pao)
        loop = R.conv_im2col(*a, taps=taps, stride=stride, upsample=up, pad_after_only=pao)
        assert ref.shape == loop.shape
        assert float((ref - loop).abs().max()) <= 1e-12 * float(S.max())
        assert bool((S >= ref.abs() - 1e-12).all())


def test_stride_2_pad_1_gives_the_ceiling_and_pad_after_only_the_floor():
    a = _tiny("random", 1, 5, 7, 8, 0, 8, 9, 2, False, 0, False, False, 1)
    assert R.conv_fp64(*a, taps=9, stride=2)[0].shape == (1, 3, 4, 8)
    assert R.conv_fp64(*a, taps=9, stride=2, pad_after_only=True)[0].shape == (1, 2, 3, 8)


def test_pack_is_tap_major_channel_minor():
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).reshape(2, 3, 3, 3)
    p = R.pack(w)
    assert p.shape == (2, 27)
    for n, c, dy, dx in itertools.product(range(2), range(3), range(3), range(3)):
        assert float(p[n, (dy * 3 + dx) * 3 + c]) == float(w[n, c, dy, dx])


@pytest.mark.parametrize("case", R.ALL_CONV_CASES, ids=repr)
def test_every_exact_conv_case_keeps_the_family_conditions(case):
    d = case.inputs("exact")
    ref, S = case.reference(d)
    R.check_exact(ref)
    assert tuple(ref.shape) == (case.B, *case.out_hw, case.N)
    if case.gn:
        assert float(R.gn_totals(R.rnd16(ref)).abs().max()) < 2.0 ** 24
    for t in d.values():
        if t is not None:
            assert torch.equal(t.float(), t.float().round()) and float(t.abs().max()) <= 8
    assert len({c.name for c in R.ALL_CONV_CASES}) == len(R.ALL_CONV_CASES)


@pytest.mark.parametrize("cin", [1280, 2560])
def test_exact_family_at_the_widest_channel_counts(cin):
    f = R.Family("exact", cin)
    K = 9 * cin
    x, w = f.x((1, 8, 8, cin), K), f.w((64, cin, 3, 3), K)
    ref, _ = R.conv_fp64(x, None, w, f.vec((64,)), f.vec((1, 64)), f.res((1, 8, 8, 64)), None)
    R.check_exact(ref)
    assert float(ref.abs().max()) > 16                              # (not thinned to nothing)
    lo = f.lo(ref)
    assert torch.equal(lo.double() * 4, (lo.double() * 4).round()) and float(lo.abs().max()) <= 1


def test_geglu_column_order_against_torch_gelu_on_unpacked_weights():
    from consolver_amd import ops                                   # (cs_op_geglu_pack: host memory only; the packer, nothing else)
    f = R.Family("random", 5)
    M, K, Hd = 7, 64, 48
    x, w, b = f.x((M, K), K), f.w((2 * Hd, K), K), f.vec((2 * Hd,))
    wp, bp = ops.geglu_pack(w, b)
    o = R.linear_fp64(x, None, wp, bp, None, None, geglu=True)
    y = x.double() @ w.double().T + b.double()
    want = y[:, :Hd] * F.gelu(y[:, Hd:])
    assert o.ref.shape == (M, Hd)
    assert torch.allclose(o.ref, want, rtol=1e-12, atol=1e-14)
    assert torch.allclose(o.v, y[:, :Hd], rtol=0, atol=1e-12) and torch.allclose(o.t, y[:, Hd:], rtol=0, atol=1e-12)


def test_gelu_constants_of_the_geglu_bound():
    x = torch.linspace(-12, 12, 480001, dtype=torch.float64)
    phi = 0.5 * (1 + torch.special.erf(x / 2 ** 0.5))
    d = phi + x * torch.exp(-x * x / 2) / (2 * torch.pi) ** 0.5
    assert 1.128 < float(d.max()) < R.GELU_ERF_DERIV_MAX and -0.13 < float(d.min()) < -0.128
    # the polynomial in float64 stays within the stated 8.2e-5 of erf-GELU, and its fp32 Horner evaluation within gelu_poly_err
    def poly(t, dt):
        t = t.to(dt)
        c = t.clamp(-4.5, 4.5)
        u = c * c
        q = torch.full_like(u, R.GELU_Q[-1])
        for a in reversed(R.GELU_Q[:-1]):
            q = q * u + a
        return t * (c * q + 0.5)
    inside = x.abs() <= 10.5
    assert float((poly(x, torch.float64) - R.gelu_erf_fp64(x)).abs()[inside].max()) <= R.GELU_POLY_ERR
    xw = torch.linspace(-200, 200, 400001, dtype=torch.float64)       # beyond the clamp the error grows with |x|: |x| Phi_poly(-4.5)
    assert bool(((poly(xw, torch.float64) - R.gelu_erf_fp64(xw)).abs() <= torch.clamp(xw.abs() * 7.75e-6, min=R.GELU_POLY_ERR)).all())
    xf = torch.linspace(-12, 12, 200001).float()
    assert bool(((poly(xf, torch.float32).double() - R.gelu_erf_fp64(xf.double())).abs() <= R.gelu_poly_err(xf.double())).all())
    assert float(R.gelu_poly_err(torch.tensor([1.0], dtype=torch.float64))) < 8.4e-5          # the evaluation term is idle where the data lives


BOUND_CASES = [c for c in R.ALL_CONV_CASES if c.name in ("g1x3x43_c64+128_n640_2", "g3x5x7_c192+0_n128_1", "s2_16x8", "up_3x5", "gsk_c512", "h1x64x8_c64_n128", "lw_fast8_b5",
                                                         "lw_up_plain160", "down_5x7", "g_m129_e5")]


@pytest.mark.parametrize("case", BOUND_CASES, ids=repr)
def test_bound_admits_a_float32_conv(case):
    """the rule applied to torch's own float32 evaluation of the same inputs: ratio <= 1 (any order of the sums is covered by g S)"""
    d = case.inputs("random")
    ref, S = case.reference(d)
    got, _ = R.conv_fp64(*[d[k] for k in ("x0", "x1", "w", "bias", "temb", "res")], None, case.taps, case.stride, case.up, case.api == "conv_down")
    x = torch.cat([d["x0"], d["x1"]], -1) if d["x1"] is not None else d["x0"]
    xs = x.float().permute(0, 3, 1, 2)
    if case.up:
        xs = F.interpolate(xs, scale_factor=2.0, mode="nearest")
    if case.taps == 9:
        xs = F.pad(xs, (0, 1, 0, 1) if case.api == "conv_down" else (1, 1, 1, 1))
    y = F.conv2d(xs, d["w"].float(), stride=case.stride).permute(0, 2, 3, 1)
    for t in (d["bias"], d["temb"][:, None, None, :] if d["temb"] is not None else None, d["res"]):
        if t is not None:
            y = y + t.float()
    g = R.gfac(case.taps * case.cin, case.addends, case.splits or 1)
    r = R.ratio(y.half(), ref, R.bound(ref, S, g))
    assert r <= 1.0, r
    assert torch.equal(got, ref)
    if case.taps * case.cin <= 1152:                                # (g S stays below an ulp for short sums: three ulps off is outside the rule somewhere)
        assert R.ratio(R.rnd16(ref) + 3 * R.ulp16(ref), ref, R.bound(ref, S, g)) > 1.0


def test_bound_admits_a_float32_linear_geglu_and_split():
    f = R.Family("random", 9)
    M, K, N = 65, 320, 256
    x, w, b = f.x((M, K), K), f.w((N, K), K), f.vec((N,))
    res = f.res((M, N))
    res_lo = f.lo(res)
    o = R.linear_fp64(x, None, w, b, res, res_lo)
    g = R.gfac(K, 3)
    v = x.float() @ w.float().T + b.float() + res.float() + res_lo.float()
    hi = v.half()
    lo = (v - hi.float()).half()
    assert R.ratio(hi, o.ref, R.bound(o.ref, o.S, g)) <= 1.0
    assert R.split_ratio(hi, lo, o.ref, o.S, g) <= 1.0
    assert R.split_ratio(hi, lo + 4 * R.ulp16(lo.double()).half(), o.ref, o.S, g) > 1.0
    assert R.row_check(R.row_totals(v.double(), 2).float(), hi.double() + lo.double(), 2, False) is None
    og = R.linear_fp64(x, None, w, b, None, None, geglu=True)
    y = x.float() @ w.float().T + b.float()
    rows = torch.arange(N // 2)
    vi = (rows // 16) * 32 + rows % 16
    out = (y[:, vi] * F.gelu(y[:, vi + 16])).half()
    assert R.ratio(out, og.ref, R.geglu_bound(og, R.gfac(K, 1))) <= 1.0


def test_statistics_rules_catch_a_missing_slot_and_a_wrong_total():
    out = torch.randn(2, 8, 16, 64).half()
    t = R.gn_totals(out)                                             # [B, N / 2, 2]
    st = torch.zeros(2, 2, 32, 2)
    st[:, 0] = t.float()
    assert R.gn_check(st, out, False) is None
    bad = st.clone(); bad[1, 1, 3, 0] = float("nan")
    assert "not written" in R.gn_check(bad, out, False)
    bad = st.clone(); bad[0, 0, 5, 1] *= 1.001
    assert R.gn_check(bad, out, False) is not None
    oi = torch.randint(-8, 9, (1, 8, 8, 64)).half()
    sti = R.gn_totals(oi).float()[:, None]
    assert R.gn_check(sti, oi, True) is None
    sti[0, 0, 0, 0] += 1
    assert R.gn_check(sti, oi, True) is not None
