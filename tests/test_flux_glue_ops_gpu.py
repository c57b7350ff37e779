"""The glue of the FLUX DiT (flux_ops.hip, small_linear in gemm2.hip) op by op against float64: qk_norm_rope, ln_modulate, small_linear, sinusoid, add3, cast,
planes_to_f32.  References, emulators and the derived bounds: tests/flux_ref.py (verified on the CPU by tests/test_flux_ref.py).

Acceptance of the two 16-bit ops, per row (per row and head for RoPE), as in tests/test_attention_forms_gpu.py:
    max |out - float64|  <=  2 x max |emulator - float64| of that row  +  1 ulp_T of the row's largest output.
The emulator applies the kernel's rounding points to exact arithmetic; the kernel adds fp32 noise that can move a rounding by one ulp.  Everything the op must not
touch (V and pad columns and rows past `rows` of the qkv buffer, rows past M) holds NaN or data and is compared bit for bit.
Worst err / bound seen on an MI355X (every case prints its own as RATIO): qk_norm_rope 0.46, ln_modulate 0.26 per row and 0.40 for y + y_lo against the fp32-class
bound, small_linear 0.11 (K = 8; below 0.003 from K = 256 on), sinusoid 0.23."""
import pytest
import torch

from consolver_amd import _lib as L
from tests import flux_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CS_E_ARG, CS_E_SHAPE = -1, -2
DT = list(R.DTYPES.items())
EPS = 1e-6


def st():
    return L.stream_ptr(DEV)


def rows_ok(out, ref, emu, dtype, what):
    """the per-row acceptance on [..., row, dim] float64 tensors; prints the worst err / bound before it asserts"""
    err, emu_err = (out - ref).abs().amax(-1), (emu - ref).abs().amax(-1)
    bound = 2.0 * emu_err + R.ulp_at(ref.abs().amax(-1), dtype)
    worst = float((err / bound).max())
    print(f"RATIO {what}: {worst:.3f}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, (what, worst)


# ---- qk_norm_rope ---------------------------------------------------------------------------------------------------------------------------------------------
def _rope(buf, rows, seq, heads, dh, q_col, k_col, w, ctx_rows, cos, sin, dt):
    dev = buf.to(DEV)
    wd = [t.to(DEV) if t is not None else None for t in w]
    c, s = cos.to(DEV), sin.to(DEV)
    L.check(L.lib().cs_op_qk_norm_rope(L.ptr(dev), buf.shape[1], rows, seq, heads, dh, q_col, k_col, *(L.ptr(t) for t in wd), ctx_rows, L.ptr(c), L.ptr(s), EPS,
                                       L.dtype_code(dt), st()))
    torch.cuda.synchronize()
    return dev.cpu()


@pytest.mark.parametrize("rows", [1, 62, 63])
@pytest.mark.parametrize("dh,heads", [(128, 3), (128, 4), (64, 5)])
@pytest.mark.parametrize("name,dt", DT)
def test_qk_norm_rope_rows_heads_and_context_weights(name, dt, dh, heads, rows):
    """two rows per wave (odd and even counts, one row), ragged head groups (3 heads at two per wave, 5 at four), context weights on the rows with row % seq < ctx_rows
    of EVERY sample (rows = 62 / 63 are two samples of seq = 31, and one row of a third), in place beside V at ld = 3 D + 16 with q / k away from columns 0 / D"""
    seq, Dm = 31, heads * dh
    ld, q_col, k_col = 3 * Dm + 16, 8, Dm + 16
    g = torch.Generator().manual_seed(100 * dh + 10 * heads + rows)
    buf = torch.full((rows + 3, ld), float("nan"), dtype=dt)
    buf[:rows, q_col:q_col + Dm] = (torch.randn(rows, Dm, generator=g) * (0.2 + 3 * torch.rand(rows, 1, generator=g))).to(dt)
    buf[:rows, k_col:k_col + Dm] = (torch.randn(rows, Dm, generator=g) * (0.2 + 3 * torch.rand(rows, 1, generator=g))).to(dt)
    buf[:rows, k_col + Dm:k_col + 2 * Dm - 8] = torch.randn(rows, Dm - 8, generator=g).to(dt)          # V; the columns left over stay NaN
    w = [(1 + 0.3 * torch.randn(dh, generator=g)).to(dt) for _ in range(4)]                             # wq, wk, wq_ctx, wk_ctx: all distinct
    cos, sin = R.rope_tables(seq, dh, rows)
    untouched = torch.ones(buf.shape, dtype=torch.bool)
    untouched[:rows, q_col:q_col + Dm] = False
    untouched[:rows, k_col:k_col + Dm] = False
    for ctx_rows, wsel in ((0, w), (7, w), (31, w), (7, w[:2] + [None, None]), (31, [w[0], w[1], None, w[3]])):
        out = _rope(buf, rows, seq, heads, dh, q_col, k_col, wsel, ctx_rows, cos, sin, dt)
        assert torch.equal(out.view(torch.int16)[untouched], buf.view(torch.int16)[untouched]), "V, pad columns or rows past `rows` changed"
        a = (buf, rows, seq, heads, dh, q_col, k_col, *wsel, ctx_rows, cos, sin, EPS)
        ref, emu = R.qk_norm_rope_ref(*a), R.qk_norm_rope_ref(*a, dtype=dt)
        for i, col in enumerate((q_col, k_col)):
            got = out[:rows, col:col + Dm].double().reshape(rows, heads, dh)
            rows_ok(got, ref[i], emu[i], dt, f"qk_norm_rope {'qk'[i]} dh {dh} heads {heads} rows {rows} ctx {ctx_rows} {'null ctx w ' if wsel[2] is None else ''}{name}")


def test_qk_norm_rope_rejections():
    dt = R.BF16
    w = torch.ones(264, dtype=dt, device=DEV)
    tab = torch.zeros(4, 132, device=DEV)
    for dh in (24, 48, 264):
        buf = torch.full((4, 3 * dh), float("nan"), dtype=dt, device=DEV)
        rc = L.lib().cs_op_qk_norm_rope(L.ptr(buf), 3 * dh, 4, 4, 1, dh, 0, dh, L.ptr(w), L.ptr(w), None, None, 0, L.ptr(tab), L.ptr(tab), EPS, 2, st())
        assert rc == CS_E_SHAPE and f"head dim {dh} unsupported" in L.lib().cs_last_error().decode()
        assert bool(buf.isnan().all())
    buf = torch.full((4, 384), float("nan"), dtype=dt, device=DEV)
    for c, s in ((None, tab), (tab, None)):
        rc = L.lib().cs_op_qk_norm_rope(L.ptr(buf), 384, 4, 4, 1, 128, 0, 128, L.ptr(w), L.ptr(w), None, None, 0, L.ptr(c), L.ptr(s), EPS, 2, st())
        assert rc == CS_E_ARG and "null pointer" in L.lib().cs_last_error().decode()
    torch.cuda.synchronize()
    assert bool(buf.isnan().all())


# ---- ln_modulate ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 5, 1000])
@pytest.mark.parametrize("C", [8, 512, 520, 1536, 2568, 3072, 4096])
@pytest.mark.parametrize("name,dt", DT)
def test_ln_modulate_every_width_form(name, dt, C, M):
    """C / 8 = 1, 64, 65, 192, 321, 384, 512 vectors: the MAXV = 1, 1, 2, 4, 6, 6, 8 kernels, with ragged lanes at 8, 520 and 2568; rows_per_sample that does not
    divide M, mod_stride = 2 C + 24; one plane, split input, split input and output.  The last row (M > 1) has mean 64 and deviation 0.3."""
    x, x_lo, rps, mod = R.ln_inputs(M, C, dt, 1000 * C + M, True)
    shift, scale = mod[:, :C], mod[:, C:2 * C]
    modd = mod.to(DEV)
    sh, sc, stride = modd.data_ptr(), modd.data_ptr() + 4 * C, mod.shape[1]
    xd, xld = x.to(DEV), x_lo.to(DEV)
    code = L.dtype_code(dt)
    for form in ("one plane", "split in", "split in and out"):
        lo = None if form == "one plane" else x_lo
        y = torch.full((M + 2, C), float("nan"), dtype=dt, device=DEV)
        yl = torch.full((M + 2, C), float("nan"), dtype=dt, device=DEV)
        L.check(L.lib().cs_op_ln_modulate(L.ptr(xd), L.ptr(xld) if lo is not None else None, L.ptr(y), L.ptr(yl) if form == "split in and out" else None, M, C, rps,
                                          sh, sc, stride, EPS, code, st()))
        torch.cuda.synchronize()
        y, yl = y.cpu(), yl.cpu()
        assert bool(y[M:].isnan().all()) and bool(yl[M if form == "split in and out" else 0:].isnan().all())
        ref = R.ln_modulate_fp64(x, lo, rps, shift, scale, EPS)
        emu, emu_lo = R.ln_modulate_emulated(x, lo, rps, shift, scale, EPS, dt)
        rows_ok(y[:M].double(), ref, emu, dt, f"ln_modulate C {C} M {M} {form} {name}")
        if form == "split in and out":
            got = y[:M].double() + yl[:M].double()
            bound = R.ln_fp32_bound(x, lo, rps, shift, scale, EPS, dt)
            worst = float(((got - ref).abs() / bound).max())
            print(f"RATIO ln_modulate y + y_lo C {C} M {M} {name}: {worst:.3f}")
            assert bool(torch.isfinite(yl[:M]).all()) and worst <= 1.0
            # y is the one rounding of y + y_lo: a nearest value of T (y_lo is itself rounded to T, so it may land exactly on the tie)
            assert bool((yl[:M].double().abs() <= 0.5 * R.ulp_at(y[:M].double(), dt)).all()), "y is not the rounding of y + y_lo"
    if M == 5:                                                                  # the one-plane entry point of the executor reaches the same kernels
        y = torch.full((M, C), float("nan"), dtype=dt, device=DEV)
        y2 = torch.full((M, C), float("nan"), dtype=dt, device=DEV)
        L.check(L.lib().cs_op_ln_modulate_x2(L.ptr(xd), L.ptr(xld), L.ptr(y), M, C, rps, sh, sc, stride, EPS, code, st()))
        L.check(L.lib().cs_op_ln_modulate(L.ptr(xd), L.ptr(xld), L.ptr(y2), None, M, C, rps, sh, sc, stride, EPS, code, st()))
        torch.cuda.synchronize()
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16))


def test_ln_modulate_rejections():
    dt = R.BF16
    x = torch.zeros(4, 4104, dtype=dt, device=DEV)
    mod = torch.zeros(1, 2 * 4104, device=DEV)
    y = torch.full((4, 4104), float("nan"), dtype=dt, device=DEV)
    for C in (12, 4104):
        rc = L.lib().cs_op_ln_modulate(L.ptr(x), None, L.ptr(y), None, 4, C, 4, L.ptr(mod), L.ptr(mod), 2 * C, EPS, 2, st())
        assert rc == CS_E_SHAPE and f"C={C} unsupported" in L.lib().cs_last_error().decode()
    rc = L.lib().cs_op_ln_modulate(L.ptr(x), None, L.ptr(y), L.ptr(y), 4, 512, 4, L.ptr(mod), L.ptr(mod), 1024, EPS, 2, st())
    assert rc == CS_E_ARG and "x_lo required" in L.lib().cs_last_error().decode()
    torch.cuda.synchronize()
    assert bool(y.isnan().all())


# ---- small_linear ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 256, 520, 768, 3072])
@pytest.mark.parametrize("name,dt", DT)
def test_small_linear_against_the_fp32_accumulation_bound(name, dt, K):
    """K / 8 = 1, 32, 65, 96, 384 vectors over 64 lanes (one lane, half a wave, a lane tail, whole rounds); N = 1, 6, 257 outputs at four per workgroup; R = 1, 3;
    the four SiLU combinations; null bias.  fp32 out against float64 within (K + 2) 2^-23 S (flux_ref.small_linear_bound)."""
    g = torch.Generator().manual_seed(K)
    worst = 0.0
    for N in (1, 6, 257):
        for Rr in (1, 3):
            x = torch.randn(Rr, K, generator=g).clamp(-4, 4)
            w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt)
            bias = torch.randn(N, generator=g).to(dt)
            xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
            for si, so, b in ((0, 0, bias), (1, 0, bias), (0, 1, bias), (1, 1, bias), (1, 1, None)):
                out = torch.full((Rr * N + 4,), float("nan"), device=DEV)
                L.check(L.lib().cs_op_small_linear(L.ptr(xd), Rr, K, L.ptr(wd), L.ptr(bd) if b is not None else None, N, L.ptr(out), si, so, L.dtype_code(dt), st()))
                torch.cuda.synchronize()
                out = out.cpu()
                ref, S, pre = R.small_linear_fp64(x, w, b, si, so)
                ratio = float(((out[:Rr * N].reshape(Rr, N).double() - ref).abs() / R.small_linear_bound(K, S, pre, so)).max())
                assert bool(out[Rr * N:].isnan().all()) and ratio <= 1.0, (N, Rr, si, so, b is None, ratio)
                worst = max(worst, ratio)
    print(f"RATIO small_linear K {K} {name}: {worst:.3f}")
    out = torch.full((8,), float("nan"), device=DEV)
    assert L.lib().cs_op_small_linear(L.ptr(xd), 1, 12, L.ptr(wd), None, 1, L.ptr(out), 0, 0, L.dtype_code(dt), st()) == CS_E_SHAPE
    torch.cuda.synchronize()
    assert bool(out.isnan().all())


# ---- sinusoid, add3, cast, planes -------------------------------------------------------------------------------------------------------------------------------
def test_sinusoid_layout_and_argument_bound():
    """C = 256, [cos | sin]; the bound is the fp32 rounding of the argument t 1000 f_k (26 * 2^-24 |a|, 1.5e-3 at 1000: flux_ref.sinusoid_bound)"""
    t = torch.tensor([0.0, 1e-3, 0.5, 1.0])
    out = torch.full((4 * 256 + 8,), float("nan"), device=DEV)
    td = t.to(DEV)
    L.check(L.lib().cs_op_sinusoid_f32(L.ptr(td), 1000.0, 4, 256, L.ptr(out), st()))
    torch.cuda.synchronize()
    out = out.cpu()
    ref, a = R.sinusoid_fp64(t, 1000.0, 256)
    bound = torch.cat((R.sinusoid_bound(a),) * 2, -1)
    ratio = (out[:1024].reshape(4, 256).double() - ref).abs() / bound
    print(f"RATIO sinusoid: {float(ratio.max()):.3f}")
    assert bool(out[1024:].isnan().all()) and float(ratio.max()) <= 1.0
    assert bool((out[:128] == 1).all()) and bool((out[128:256] == 0).all())               # t = 0: cos | sin


@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_add3_cast_and_planes_are_bit_exact(n):
    g = torch.Generator().manual_seed(n)
    a, b, c = (torch.randn(n, generator=g) * 10 ** torch.randint(-3, 4, (n,), generator=g).float() for _ in range(3))
    ad, bd, cd = a.to(DEV), b.to(DEV), c.to(DEV)
    for bb, want in ((bd, (a + b) + c), (None, a + c)):
        out = torch.full((n + 3,), float("nan"), device=DEV)
        L.check(L.lib().cs_op_add3_f32(L.ptr(ad), L.ptr(bb), L.ptr(cd), L.ptr(out), n, st()))
        torch.cuda.synchronize()
        assert torch.equal(out[:n].cpu(), want) and bool(out[n:].isnan().all())
    for name, dt in DT:
        x = torch.cat((a[: n - 1], torch.tensor([1.0 + R.ulp(dt) / 2])))                   # a tie: round to nearest even
        out = torch.full((n + 3,), float("nan"), dtype=dt, device=DEV)
        xd = x.to(DEV)
        L.check(L.lib().cs_op_cast_f32(L.ptr(xd), L.ptr(out), n, L.dtype_code(dt), st()))
        hi = (a * 3).to(dt)
        lo = (a * 3 - hi.float()).to(dt)
        f32 = torch.full((n + 3,), float("nan"), device=DEV)
        hd, ld = hi.to(DEV), lo.to(DEV)
        L.check(L.lib().cs_op_planes_to_f32(L.ptr(hd), L.ptr(ld), L.ptr(f32), n, L.dtype_code(dt), st()))
        torch.cuda.synchronize()
        assert torch.equal(out[:n].cpu().view(torch.int16), x.to(dt).view(torch.int16)) and bool(out[n:].isnan().all()), name
        assert torch.equal(f32[:n].cpu(), hi.float() + lo.float()) and bool(f32[n:].isnan().all()), name
