"""The three small T5 encoder kernels of csrc/flux_ops.hip through the C ABI, each on its own against an exact or float64 reference: cs_op_rms_norm
(elementwise, one rounding), cs_op_gated_mul (bit-identical to the rounded fp32 product), cs_op_embed_rows (bit-identical gather, ids clamped).  The T5 model
tests reach them only under a whole-tensor bound in which one wrong row or one wrong vector disappears."""
import pytest
import torch

from consolver_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CS_E_SHAPE = -2
DTYPES = [torch.float16, torch.bfloat16]


def _sync_ok(rc):
    L.check(rc)
    torch.cuda.synchronize()


# ---- cs_op_rms_norm ------------------------------------------------------------------------------------------------------------------------------------
# C: both sides of every vectors-per-lane step of the launcher (C / 8 vectors over 64 lanes: 1, 2, 4, 8 per lane) and the largest row; M: the four-rows-per-workgroup tail
@pytest.mark.parametrize("C_", [8, 512, 520, 1024, 1032, 2048, 2056, 4096])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_rms_norm_elementwise(dt, C_):
    """y = x rsqrt(mean(x^2) + eps) w in fp32 with ONE rounding to T: every element within half an ulp of the float64 value (2^-11 f16, 2^-8 bf16, times
    1 + 1e-3 for the fp32 arithmetic in front of the rounding) plus T's smallest normal"""
    half_ulp = 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8
    tiny = torch.finfo(dt).tiny
    eps = 1e-6
    for M in (1, 3, 4, 5, 257):
        g = torch.Generator().manual_seed(1000 * M + C_)
        x = (1.0 + 3.0 * torch.randn(M, C_, generator=g))
        if M >= 3:
            x[1, C_ // 2] = 1e3            # one outlier element
            x[2] = 0                       # an all-zero row: rsqrt(eps) times zero
        x, w = x.to(dt), (1.0 + 0.2 * torch.randn(C_, generator=g)).to(dt)
        out = torch.full((M, C_), float("nan"), dtype=dt, device=DEV)
        xg, wg = x.to(DEV), w.to(DEV)
        _sync_ok(L.lib().cs_op_rms_norm(L.ptr(xg), L.ptr(wg), L.ptr(out), M, C_, eps, L.dtype_code(dt), L.stream_ptr(DEV)))
        xd = x.double()
        ref = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps) * w.double()
        err = (out.cpu().double() - ref).abs()
        tol = half_ulp * ref.abs() * (1 + 1e-3) + tiny
        worst = float((err / tol).max())
        print(f"rms_norm {dt} C {C_} M {M}: max err / tol {worst:.3f}")
        assert torch.isfinite(out).all()
        assert worst <= 1.0, (M, C_, worst)
        if M >= 3:
            assert bool((out[2] == 0).all())


@pytest.mark.parametrize("C_", [4104, 12])
def test_rms_norm_rejects(C_):
    x = torch.zeros(2, C_, dtype=torch.float16, device=DEV)
    out = torch.full_like(x, 3.0)
    assert L.lib().cs_op_rms_norm(L.ptr(x), L.ptr(x), L.ptr(out), 2, C_, 1e-6, 1, L.stream_ptr(DEV)) == CS_E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---- cs_op_gated_mul ----------------------------------------------------------------------------------------------------------------------------------
def _pow_range(n, g, dt):
    """+- 2^u, u uniform in [-6, 6]: products stay in T's normal range"""
    mag = torch.exp2(12.0 * torch.rand(n, generator=g) - 6.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(dt)


@pytest.mark.parametrize("n", [8, 2040, 2048, 2056, 8 * 100003])
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
def test_gated_mul_is_the_rounded_fp32_product(dt, n):
    """the fp32 product of two 11-bit (8-bit) significands is exact and the pack rounds to nearest even: bit-identical to (a.float() * b.float()).to(T);
    also in place (out = a), as the T5 encoder calls it"""
    g = torch.Generator().manual_seed(n)
    a, b = _pow_range(n, g, dt), _pow_range(n, g, dt)
    want = (a.float() * b.float()).to(dt)
    assert torch.isfinite(want).all() and float(want.float().abs().min()) >= float(torch.finfo(dt).tiny)
    ad, bd = a.to(DEV), b.to(DEV)
    out = torch.full((n,), float("nan"), dtype=dt, device=DEV)
    _sync_ok(L.lib().cs_op_gated_mul(L.ptr(ad), L.ptr(bd), L.ptr(out), n, L.dtype_code(dt), L.stream_ptr(DEV)))
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    _sync_ok(L.lib().cs_op_gated_mul(L.ptr(ad), L.ptr(bd), L.ptr(ad), n, L.dtype_code(dt), L.stream_ptr(DEV)))
    assert torch.equal(ad.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(bd.cpu().view(torch.int16), b.view(torch.int16))


def test_gated_mul_rejects_a_count_that_is_no_multiple_of_8():
    a = torch.ones(16, dtype=torch.float16, device=DEV)
    out = torch.full_like(a, 3.0)
    assert L.lib().cs_op_gated_mul(L.ptr(a), L.ptr(a), L.ptr(out), 12, 1, L.stream_ptr(DEV)) == CS_E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---- cs_op_embed_rows -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [1, 1000])
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("C_", [8, 4096])
def test_embed_rows_is_a_clamped_gather(C_, rows, vocab):
    """out[r] = table[clamp(ids[r], 0, vocab - 1)], bit for bit; ids -1 and vocab map to rows 0 and vocab - 1 (the kernel's clamp, pinned here)"""
    g = torch.Generator().manual_seed(C_ + rows + vocab)
    table = torch.randint(-32768, 32767, (vocab, C_), generator=g, dtype=torch.int16)       # any bit pattern, NaNs included
    if rows == 1:
        id_sets = [[0], [vocab - 1], [-1], [vocab]]
    else:
        ids = torch.randint(0, vocab, (rows,), generator=g)
        ids[:4] = torch.tensor([0, vocab - 1, -1, vocab])
        ids[-1] = vocab
        id_sets = [ids.tolist()]
    td = table.to(DEV)
    for ids in id_sets:
        idt = torch.tensor(ids, dtype=torch.int64)
        idg = idt.to(DEV)
        out = torch.full((rows, C_), 0x7FD5, dtype=torch.int16, device=DEV)
        _sync_ok(L.lib().cs_op_embed_rows(L.ptr(idg), L.ptr(td), L.ptr(out), rows, C_, vocab, L.stream_ptr(DEV)))
        assert torch.equal(out.cpu(), table[idt.clamp(0, vocab - 1)]), ids[:4]
