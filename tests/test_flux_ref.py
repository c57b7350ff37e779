"""CPU checks of tests/flux_ref.py, the yardsticks of tests/test_flux_gemm2_forms_gpu.py and tests/test_flux_glue_ops_gpu.py: each emulator lands within T's rounding
of its float64 reference, the row-map helper equals a plain loop, the derived GELU / LayerNorm / sinusoid bounds hold for an independent fp32 evaluation, and the
exact family's conditions (integer branch values and references inside T's exact range) hold on the reference of EVERY exact case, before any GPU run."""
import math

import pytest
import torch

from tests import flux_ref as R

DT = list(R.DTYPES.items())


@pytest.mark.parametrize("seg,stride,off", [(0, 0, 0), (0, 0, 5), (208, 248, 40), (40, 248, 0), (1, 3, 2), (2176, 2200, 8)])
def test_rowmap_equals_a_plain_loop(seg, stride, off):
    for M in (1, 7, 416, 4352):
        assert R.rowmap(torch.arange(M), seg, stride, off).tolist() == R.rowmap_loop(M, seg, stride, off)


def test_ulp_at_is_the_spacing_of_T():
    for name, dt in DT:
        x = torch.tensor([1.0, 1.5, 2.0, 3.99, 0.37, 100.0, 255.0, 2.0 ** -20])
        xt = x.to(dt)
        up = (xt.view(torch.int16) + 1).view(dt)
        assert torch.equal(R.ulp_at(xt.double(), dt), up.double() - xt.double()), name
        assert float(R.ulp_at(torch.tensor(0.0), dt)) == (2.0 ** -24 if dt == R.F16 else 2.0 ** -133)
        assert R.ulp(dt) == float(R.ulp_at(torch.tensor(1.0), dt))


def test_gelu_derivative_and_fast_form_bounds():
    x = torch.linspace(-12, 12, 480001, dtype=torch.float64)
    s = torch.sigmoid(2 * R._C0 * (x + 0.044715 * x ** 3))
    d = s + x * s * (1 - s) * 2 * R._C0 * (1 + 3 * 0.044715 * x ** 2)
    assert 1.128 < float(d.max()) < R.GELU_DERIV_MAX and -0.13 < float(d.min()) < -0.128
    assert torch.allclose(R.gelu_fp64(x), torch.nn.functional.gelu(x, approximate="tanh"), rtol=1e-13, atol=1e-15)
    # the kernel's fast form evaluated in fp32 by torch (exact exp2 and reciprocal roundings instead of the hardware's 1 ulp) stays inside the bound
    xf = torch.linspace(-12, 12, 200001).float()
    t = xf * xf
    fast = xf * (1.0 / (1.0 + torch.exp2(xf * (-2.302208198 - 0.1029432397 * t))))
    assert bool(((fast.double() - R.gelu_fp64(xf.double())).abs() <= R.gelu_fast_err(xf.double())).all())
    assert float(R.gelu_fast_err(torch.tensor([-3.0, 0.5, 4.0], dtype=torch.float64)).max()) < 2.0 ** -19        # |x| 2^-22 at most here: far below the bf16 / f16 rounding of the result


@pytest.mark.parametrize("name,dt", DT)
def test_every_exact_case_keeps_the_family_conditions(name, dt):
    for cname, (build, rows) in R.exact_cases(dt).items():
        bufs, probs = build()
        written = {}
        for p in probs:
            o = R.check_exact_conditions(bufs, p, dt, R.pair_rows(p, rows))
            if rows is None:
                seen = written.setdefault(p.out, torch.zeros(bufs[p.out].shape[0], dtype=torch.int32))
                seen[o.crow] += 1
                assert o.crow.max() < bufs[p.out].shape[0] - R.GUARD and bool(torch.isfinite(bufs[p.a][R.rowmap(o.m, *p.a_map), :p.K]).all()), cname
            # the emulator IS the reference in this family
            assert torch.equal(o.emu, rnd_t(o.ref, dt)), cname
            if p.out_lo:
                assert torch.equal(o.emu_lo, rnd_t(o.ref - rnd_t(o.ref, dt), dt)), cname
        for seen in written.values():
            assert int(seen.max()) == 1, cname                                    # every row written at most once across the problems
        if cname in ("embed_pair", "qkv_pair"):
            assert all(int(seen[:-R.GUARD].min()) == 1 for seen in written.values()), cname   # ... and exactly once where the pair covers the buffer


def rnd_t(x, dt):
    return x.to(dt).double()


@pytest.mark.parametrize("name,dt", DT)
def test_gemm2_emulator_is_within_T_rounding_of_float64(name, dt):
    fam = R.Family("random", dt, 5)
    for bufs, probs in (R.case_out(fam, False), R.case_out(fam, True), R.case_single_mlp(fam), R.case_plain(fam, 65, 192), R.case_head(fam, 264)):
        for p in probs:
            o = R.g2_values(bufs, p, dt)
            assert bool(torch.isfinite(o.ref).all()) and bool((o.bound > 0).all())
            gabs = bufs[p.gate][torch.div(o.m, p.rps, rounding_mode="floor"), p.gate_off:p.gate_off + p.N].double().abs() if p.gate else 1.0
            if p.out_lo:                                                          # one rounding of the sum; hi + lo is fp32-class
                assert bool(((o.emu - o.ref).abs() <= 0.5 * R.ulp_at(o.emu, dt) + 2.0 ** -23 * (gabs * o.v.abs() + o.ref.abs())).all())
                assert bool(((o.emu + o.emu_lo - o.ref).abs() <= o.bound_sum).all())
                assert bool((o.emu_lo.abs() <= 0.5 * R.ulp_at(o.emu, dt) * 1.001).all())
            else:                                                                 # the branch's rounding times the gate, and the sum's own
                slack = 1.001 * (gabs * (0.5 * R.ulp_at(o.emu_branch, dt) + 2.0 ** -23 * o.branch.abs()) + 0.5 * R.ulp_at(o.emu, dt) + 2.0 ** -23 * o.ref.abs())
                assert bool(((o.emu - o.ref).abs() <= slack).all())


@pytest.mark.parametrize("name,dt", DT)
def test_qk_norm_rope_emulator(name, dt):
    g = torch.Generator().manual_seed(3)
    rows, seq, heads, dh = 63, 31, 3, 128
    ld = 3 * heads * dh + 16
    buf = torch.randn(rows, ld, generator=g).to(dt)
    wq, wk, wqc, wkc = ((1 + 0.3 * torch.randn(dh, generator=g)).to(dt) for _ in range(4))
    cos, sin = R.rope_tables(seq, dh, 1)
    a = (buf, rows, seq, heads, dh, 8, heads * dh + 16, wq, wk, wqc, wkc, 7, cos, sin, 1e-6)
    for ref, emu, w in zip(R.qk_norm_rope_ref(*a), R.qk_norm_rope_ref(*a, dtype=dt), (wq, wk)):
        # three roundings of values of magnitude <= max |w| max |x rsqrt| <= |w|_max sqrt(dh): 2.5 ulp of the head's largest output is generous
        assert bool(((emu - ref).abs().amax(-1) <= 2.5 * R.ulp_at(ref.abs().amax(-1), dt) * 2).all())
        assert float((emu - ref).abs().max()) > 0
    # no context rows or null context weights: the image weights everywhere; context weights reach exactly the rows with pos < ctx_rows
    img = R.qk_norm_rope_ref(*a[:11], 0, *a[12:])
    null = R.qk_norm_rope_ref(*a[:9], None, None, 7, *a[12:])
    ctx = R.qk_norm_rope_ref(*a)
    assert torch.equal(img[0], null[0]) and torch.equal(img[1], null[1])
    pos = torch.arange(rows) % seq
    assert torch.equal(ctx[0][pos >= 7], img[0][pos >= 7]) and not torch.equal(ctx[0][pos < 7], img[0][pos < 7])
    # rotation keeps the norm of every pair
    x = buf[:rows, 8:8 + heads * dh].double().reshape(rows, heads, dh)
    n = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * wq.double()
    assert torch.allclose((img[0] ** 2).reshape(rows, heads, dh // 2, 2).sum(-1), (n ** 2).reshape(rows, heads, dh // 2, 2).sum(-1), rtol=1e-6)      # (the tables are fp32)


@pytest.mark.parametrize("name,dt", DT)
@pytest.mark.parametrize("C", [8, 520, 4096])
def test_ln_modulate_emulator_and_fp32_bound(name, dt, C):
    M = 37
    x, x_lo, rps, mod = R.ln_inputs(M, C, dt, 9, True)
    shift, scale = mod[:, :C], mod[:, C:2 * C]
    ref = R.ln_modulate_fp64(x, x_lo, rps, shift, scale, 1e-6)
    y, y_lo = R.ln_modulate_emulated(x, x_lo, rps, shift, scale, 1e-6, dt)
    assert bool(((y - ref).abs() <= 0.5 * R.ulp_at(y, dt) + 2.0 ** -23 * ref.abs()).all())
    bound = R.ln_fp32_bound(x, x_lo, rps, shift, scale, 1e-6, dt)
    assert bool(((y + y_lo - ref).abs() <= bound).all())
    # an independent fp32 evaluation (torch) is inside the fp32-class bound, and the bound is far below T's rounding of y wherever |y| is not tiny
    xs = x.float() + x_lo.float()
    b = torch.div(torch.arange(M), rps, rounding_mode="floor")
    mean = xs.mean(-1, keepdim=True)
    o32 = (xs - mean) * torch.rsqrt(((xs - mean) ** 2).mean(-1, keepdim=True) + 1e-6) * (1.0 + scale[b]) + shift[b]
    assert bool(((o32.double() - ref).abs() <= bound).all())
    big = (ref.abs() > 0.25)[:M - 1]                      # (the last row's large mean costs it three digits: its bound is about T's rounding in f16)
    assert float((bound / R.ulp_at(ref, dt))[:M - 1][big].max()) < 0.5
    assert float(x[M - 1].float().mean()) > 60 and float(x[M - 1].float().std()) < 1


def test_small_linear_and_sinusoid_bounds():
    g = torch.Generator().manual_seed(4)
    for K in (8, 520, 3072):
        x = torch.randn(3, K, generator=g).clamp(-4, 4)
        w = (torch.randn(6, K, generator=g) * K ** -0.5).to(torch.bfloat16)
        bias = torch.randn(6, generator=g).to(torch.bfloat16)
        for si in (0, 1):
            for so in (0, 1):
                ref, S, pre = R.small_linear_fp64(x, w, bias, si, so)
                xx = torch.nn.functional.silu(x) if si else x
                o32 = xx @ w.float().T + bias.float()
                o32 = torch.nn.functional.silu(o32) if so else o32
                assert bool(((o32.double() - ref).abs() <= R.small_linear_bound(K, S, pre, so)).all())
    s = torch.linspace(-20, 20, 4001, dtype=torch.float64)
    d = torch.sigmoid(s) * (1 + s * (1 - torch.sigmoid(s)))
    assert float(d.abs().max()) < 1.1
    t = torch.tensor([0.0, 1e-3, 0.5, 1.0])
    ref, a = R.sinusoid_fp64(t, 1000.0, 256)
    assert ref.shape == (4, 256) and float(a.max()) == 1000.0 and bool((ref[0, :128] == 1).all()) and bool((ref[0, 128:] == 0).all())
    k = torch.arange(128, dtype=torch.float32)
    a32 = t[:, None] * 1000.0 * torch.exp(-9.210340371976184 * k / 128.0)[None, :]
    o32 = torch.cat((torch.cos(a32), torch.sin(a32)), -1)
    bound = torch.cat((R.sinusoid_bound(a),) * 2, -1)
    assert bool(((o32.double() - ref).abs() <= bound).all()) and float(bound.max()) < 1.6e-3
    assert math.isclose(float(R.sinusoid_bound(torch.tensor(1000.0, dtype=torch.float64))), 1000 * 26 * 2.0 ** -24 + 4 * 2.0 ** -24)
