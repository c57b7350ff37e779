"""Every form of attn_kernel / attn40_lw_kernel (csrc/attention.hip) through the C ABI -- cs_op_attention, cs_op_attention_ex, cs_op_attention_causal,
cs_op_attention_bias -- against a float64 reference of the same rounded inputs, per ROW and head, at the tile edges, on the running-max rescale path, on the
fp16-overflow redo, through strided operands with NaN sentinels around them, under the scheduling knobs, and at the launcher's rejections.

Assertions (tests/attention_ref.py holds the references and the input families):
  (a) max over rows of err_row <= 2 x (the emulator's worst row on the same inputs) + 1 ulp of T, err_row = relative L2 of one query row of one head against
      fp64.  The emulator carries every rounding to T the kernel has (Q (scale log2 e), P, one final rounding; the denominator from the rounded P at head
      dim 40 and from the fp32 exponentials elsewhere -- attention.hip sums `ps += e` in front of the pack2 lines); what is left is fp32 summation order and
      v_exp_f32's last bit, two orders below T's epsilon.  The factor is that argument, not a fit.
  (b) the project's whole-tensor bounds on unit-Gaussian inputs (2e-3; head dim 128: 3e-3 f16, 2e-2 bf16);
  (c) every output element finite, with `out` pre-filled with NaN: every row of every head is written.

The emulator's own worst rows against fp64 (tests/test_attention_ref.py, B = 2, H = 3, one query block and a row x 261 keys; max over the families):
  f16   head dim 40: 7.7e-4   64: 7.9e-4 (causal 7.1e-4, bias 1.3e-3)   80: 9.9e-4   160: 6.1e-4   128: 1.2e-3     (bounds 2e-3; 3e-3 at 128)
  bf16  head dim 64 bias: 1.2e-2   128: 1.0e-2                                                                      (bound 2e-2)
  unit-Gaussian alone: f16 4.9e-4 .. 6.3e-4, bf16 4.2e-3 .. 4.3e-3; the edge family (a dominant last key) is the worst of most lines.  The outlier family is
  not in these lines: over ALL its rows the emulator reaches 2.1e-3 (head dim 40), 2.3e-3 (128 f16) and 1.7e-2 (128 bf16) -- to the other queries the 6 x key is
  a score of sigma 6, and the rounding of Q (scale log2 e) to T moves competing scores -- and 5.6e-4 / 6.9e-4 / 4.7e-3 on the two rows test 3 names.

Launch sizes: B H = 6 gives 6 workgroups below one query block and 12 above (the XCD remap's r = 6 with n < 8 and r = 4 with n = 12); the H = 4 cases give 8.

attn_qt40 = 2 against 4 (QT40_BIT_IDENTICAL below, from the GPU run): bit-identical on the Gaussian, edge and rise inputs -- a row's arithmetic does not depend
on how many query tiles its wave holds, and on "rise" every workgroup of either form redoes its rows -- and NOT on the outlier inputs: the redo is block-uniform,
the outlier's block is rows 0..255 with four query tiles per wave and 0..127 with two, so rows 128..255 come from the redo loop in one form and from the fast path
in the other (another reference maximum, other roundings of P; both inside (a)).
Causal with bf16 cannot be reached through the ABI (cs_op_attention_causal takes no dtype), so that rejection has no test."""
import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import ops
from tests import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H = 2, 3
FILL = 0x7FD5              # a NaN bit pattern in f16 and in bf16
ALL_FORMS = {**R.FORMS, **R.LW_FORMS}
CS_E_SHAPE, CS_E_UNSUPPORTED = -2, -6


def launch(name, qv, kv, vv, ov, Bn, Hn, Nq, Nk, bias2=None, knobs=None, dh=None, dtype=None):
    """one call of the form's entry point on views (pointer + row stride in elements); returns the ABI's code"""
    kind, fdh, fdt, _, fknobs = ALL_FORMS[name]
    dh, dtype = dh or fdh, dtype or fdt
    l, st = L.lib(), L.stream_ptr(qv.device)
    args = (L.ptr(qv), qv.stride(-2), L.ptr(kv), kv.stride(-2), L.ptr(vv), vv.stride(-2), L.ptr(ov), ov.stride(-2))
    try:
        for key, val in {**fknobs, **(knobs or {})}.items():
            ops.set_tuning(key, val)
        if kind == "causal":
            return l.cs_op_attention_causal(*args, Bn, Hn, Nq, dh, dh ** -0.5, st)
        if kind == "bias":
            return l.cs_op_attention_bias(*args, Bn, Hn, Nq, dh, dh ** -0.5, L.ptr(bias2), L.dtype_code(dtype), st)
        if dh in (64, 128) or dtype != torch.float16:
            return l.cs_op_attention_ex(*args, Bn, Hn, Nq, Nk, dh, dh ** -0.5, L.dtype_code(dtype), st)
        return l.cs_op_attention(*args, Bn, Hn, Nq, Nk, dh, dh ** -0.5, st)
    finally:
        ops.reset_tuning()


def nan_like(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def run_dense(name, c, knobs=None):
    q, k, v = c.q.to(DEV), c.k.to(DEV), c.v.to(DEV)
    out = nan_like(q.shape, q.dtype)
    bias2 = R.bias_for_abi(c.bias).to(DEV) if c.bias is not None else None
    L.check(launch(name, q, k, v, out, q.shape[0], c.H, q.shape[1], k.shape[1], bias2, knobs))
    torch.cuda.synchronize()
    return out.cpu()


def check_rows(out, c, what, rows=None, whole=None):
    """(c) and (a), on every row or on `rows`; (b) when `whole` is given.  Prints the figures before it asserts."""
    e = R.err_rows(out, c.ref, c.H)
    bound = 2.0 * c.emu_max + R.ulp(out.dtype)
    worst = float(e.max()) if rows is None else float(e[:, list(rows)].max())
    print(f"{what}: max row err {float(e.max()):.3e}" + (f" rows {list(rows)} {worst:.3e}" if rows is not None else "")
          + f"  emulator {c.emu_max:.3e}  bound {bound:.3e}" + (f"  whole {R.rel_l2(out, c.ref):.3e}" if whole else ""))
    assert torch.isfinite(out).all(), what
    assert worst <= bound, (what, worst, bound)
    if whole:
        assert R.rel_l2(out, c.ref) < whole, (what, R.rel_l2(out, c.ref), whole)


def case_for(name, Nq, Nk, family, Hn=H, Bn=B):
    kind, dh, dt, _, _ = ALL_FORMS[name]
    return R.make_case(kind, dh, dt, Bn, Hn, Nq, Nk, family)


# ---- 1. tile edges ------------------------------------------------------------------------------------------------------------------------------------
def _edge_shapes(name):
    kind, _, _, rows, _ = ALL_FORMS[name]
    if name in R.LW_FORMS:
        return [(256, 64, H), (256, 128, H), (512, 192, H), (256, 128, 4)]
    if kind == "bias":
        return [(n, n, H) for n in (4, 60, 64, 68, 132)] + [(68, 68, 4)]
    if kind == "causal":
        return [(n, n, H) for n in (1, 17, 63, 64, 65, 127, 129, 257)] + [(65, 65, 4)]
    return [(nq, nk, H) for nq in (1, 17, rows - 1, rows + 1) for nk in (1, 63, 64, 65, 129)] + [(rows - 1, 65, 4)]


EDGE = [(name, nq, nk, h) for name in ALL_FORMS for nq, nk, h in _edge_shapes(name)]


@pytest.mark.parametrize("name,Nq,Nk,Hn", EDGE, ids=[f"{n}-{a}x{b}-H{h}" for n, a, b, h in EDGE])
def test_tile_edges_with_a_dominant_last_key(name, Nq, Nk, Hn):
    """the last key (causal: the diagonal key of every third row) carries >= 0.2 of every row's weight and a value pattern of its own: a ragged mask, a causal
    diagonal or a bias guard that is off by one moves whole rows by tens of percent"""
    c = case_for(name, Nq, Nk, "edge", Hn)
    check_rows(run_dense(name, c), c, f"edge {name} {Nq}x{Nk} H{Hn}")


@pytest.mark.parametrize("name", list(ALL_FORMS))
def test_unit_gaussian_rows_and_whole_tensor(name):
    kind, dh, dt, rows, _ = ALL_FORMS[name]
    Nq, Nk = (512, 192) if name in R.LW_FORMS else R.rescale_shape(kind, rows)
    c = case_for(name, Nq, Nk, "gauss")
    check_rows(run_dense(name, c), c, f"gauss {name}", whole=R.whole_tensor_bound(dh, dt))


# ---- 2. the running-max rescale ------------------------------------------------------------------------------------------------------------------------
RESCALE = [(name, fam) for name, (kind, dh, _, _, _) in R.FORMS.items() for fam in R.rescale_families(kind, dh)]


@pytest.mark.parametrize("name,family", RESCALE, ids=[f"{n}-{f}" for n, f in RESCALE])
def test_running_max_rescale(name, family):
    """the reference maximum moves (m_run += delta, l_run *= alpha, o_acc *= alpha) at every tile (rise), never (fall: P of later tiles underflows), for one query
    of a wave only (one: the decision is wave-uniform, the other queries take delta = max(mx, 0)), by 2^10 with the fast paths of head dims 40 / 128 still on
    (moderate), or away from a first tile whose bias is -1e4 (neg_tile0)"""
    kind, dh, dt, rows, _ = R.FORMS[name]
    Nq, Nk = R.rescale_shape(kind, rows)
    c = case_for(name, Nq, Nk, family)
    if family in ("rise", "fall") and kind != "causal":        # the construction does what it says: >= 12 log2 units per tile, in every row
        s2 = R.scores_log2(c.q, c.k, c.H, c.scale, False, c.bias)
        tmax = torch.stack([s2[..., i:i + 64].amax(-1) for i in range(0, Nk, 64)], -1)
        d = tmax[..., 1:] - tmax[..., :-1]
        assert float((d if family == "rise" else -d).min()) >= 12.0
    check_rows(run_dense(name, c), c, f"rescale {name} {family}")


# ---- 3. the redo after an overflow of P ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dh40", "dh40_qt2", "dh40_lw1", "dh40_lw2", "dh128_f16", "dh128_bf16"])
def test_outlier_key_redo_rows(name):
    """key 200 = 6 x query 5: 2^16 above the first tile's maximum for that query (f16: P overflows, the block -- loader-wave kernel: the wave -- redoes its rows
    with running maxima; bf16: no overflow, same result).  Asserted on the outlier's row, on a row of another wave of the same workgroup, and on all rows."""
    kind, dh, dt, rows, _ = ALL_FORMS[name]
    Nq, Nk = (256, 256) if name in R.LW_FORMS else (rows + 1, 261)
    c = case_for(name, Nq, Nk, "outlier")
    out = run_dense(name, c)
    check_rows(out, c, f"outlier {name}", rows=(5, 5 + rows // 4))
    check_rows(out, c, f"outlier {name} all rows")


# ---- 4. strides and sentinels, all inside one allocation --------------------------------------------------------------------------------------------------
def _stride_shape(name):
    kind, _, _, rows, _ = ALL_FORMS[name]
    return 256 if name in R.LW_FORMS else 132 if kind == "bias" else rows + 1


@pytest.mark.parametrize("name", list(ALL_FORMS))
def test_fused_qkv_buffer(name):
    """q, k, v as column slices of one [B][N][3 H dh] buffer: same bits as the dense call"""
    N = _stride_shape(name)
    c = case_for(name, N, N, "edge")
    Cw = c.H * c.dh
    qkv = torch.cat([c.q, c.k, c.v], -1).to(DEV).contiguous()
    out = nan_like((B, N, Cw), qkv.dtype)
    bias2 = R.bias_for_abi(c.bias).to(DEV) if c.bias is not None else None
    L.check(launch(name, qkv[:, :, :Cw], qkv[:, :, Cw:2 * Cw], qkv[:, :, 2 * Cw:], out, B, c.H, N, N, bias2))
    torch.cuda.synchronize()
    check_rows(out.cpu(), c, f"fused {name}")
    assert torch.equal(out.cpu(), run_dense(name, c))


@pytest.mark.parametrize("name", list(ALL_FORMS))
def test_nan_padding_columns(name):
    """H = 1 with row strides dh + 8 and NaN in the eight extra columns of q, k and v: the clamped Q loads and the dh / 8 chunks per staged K / V row never
    let a padding value into a product"""
    kind = ALL_FORMS[name][0]
    N = _stride_shape(name)
    Nk = N if kind != "plain" or name in R.LW_FORMS else 65
    c = case_for(name, N, Nk, "edge", Hn=1)
    dh = c.dh
    bufs = []
    for t in (c.q, c.k, c.v):
        w = nan_like((B, t.shape[1], dh + 8), t.dtype)
        w[:, :, :dh] = t.to(DEV)
        bufs.append(w)
    out = nan_like((B, N, dh), c.q.dtype)
    bias2 = R.bias_for_abi(c.bias).to(DEV) if c.bias is not None else None
    L.check(launch(name, bufs[0][:, :, :dh], bufs[1][:, :, :dh], bufs[2][:, :, :dh], out, B, 1, N, Nk, bias2))
    torch.cuda.synchronize()
    check_rows(out.cpu(), c, f"nan columns {name}")


@pytest.mark.parametrize("name", list(ALL_FORMS))
def test_nan_rows_behind_kv_and_output_slice(name):
    """k and v of the last batch are followed, in the same allocation, by 64 rows of NaN (ragged Nk where the form allows: the staging guard of the last tile;
    loader-wave form: the loader's clamp past the last tile); `out` is a column slice of a wider buffer filled with a NaN bit pattern: the columns around it
    keep their bits, every element inside is written (ragged Nq, B = 2)"""
    kind = ALL_FORMS[name][0]
    N = _stride_shape(name)
    Nk = N if kind != "plain" or name in R.LW_FORMS else 65
    c = case_for(name, N, Nk, "edge")
    Cw = c.H * c.dh
    kv = []
    for t in (c.k, c.v):
        w = nan_like((B * Nk + 64, Cw), t.dtype)
        w[:B * Nk] = t.to(DEV).reshape(B * Nk, Cw)
        kv.append(w[:B * Nk].view(B, Nk, Cw))
    wide = torch.full((B, N, Cw + 16), FILL, dtype=torch.int16, device=DEV).view(c.q.dtype)
    bias2 = R.bias_for_abi(c.bias).to(DEV) if c.bias is not None else None
    L.check(launch(name, c.q.to(DEV), kv[0], kv[1], wide[:, :, 8:8 + Cw], B, c.H, N, Nk, bias2))
    torch.cuda.synchronize()
    bits = wide.view(torch.int16).cpu()
    assert bool((bits[:, :, :8] == FILL).all()) and bool((bits[:, :, 8 + Cw:] == FILL).all())
    check_rows(wide[:, :, 8:8 + Cw].cpu().contiguous(), c, f"nan rows / out slice {name}")


# ---- 5. knobs -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dh40", "dh40_lw1", "dh64", "dh64_causal", "dh64_bias_bf16", "dh128_f16", "dh128_bf16"])
def test_attn_prio_changes_scheduling_only(name):
    kind, _, _, rows, _ = ALL_FORMS[name]
    Nq, Nk = (256, 128) if name in R.LW_FORMS else R.rescale_shape(kind, rows)
    c = case_for(name, Nq, Nk, "gauss")
    a, b = run_dense(name, c, {"attn_prio": 0}), run_dense(name, c, {"attn_prio": 1})
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("Nq,Nk", [(256, 64), (256, 128), (512, 192)])
def test_attn_lw_2_is_bit_identical_to_attn_kernel(Nq, Nk):
    for family in ("gauss", "edge"):
        c = case_for("dh40", Nq, Nk, family)
        assert torch.equal(run_dense("dh40_lw2", c), run_dense("dh40", c)), family


QT40_BIT_IDENTICAL = {"gauss": True, "edge": True, "rise": True, "outlier": False}      # see the header


@pytest.mark.parametrize("family", ["gauss", "edge", "rise", "outlier"])
def test_attn_qt40_2_and_4(family):
    """both instantiations satisfy (a) on the same inputs and reference, and agree bit for bit exactly where the header says"""
    c = case_for("dh40", 257, 261, family)
    a, b = run_dense("dh40", c), run_dense("dh40_qt2", c)
    check_rows(a, c, f"qt40=4 {family}")
    check_rows(b, c, f"qt40=2 {family}")
    print(f"attn_qt40 2 vs 4, {family}: bit-identical {torch.equal(a, b)}")
    assert torch.equal(a, b) == QT40_BIT_IDENTICAL[family]


# ---- 6. rejections ------------------------------------------------------------------------------------------------------------------------------------------
def _reject(code, rc, out):
    torch.cuda.synchronize()
    assert rc == code, (rc, L.lib().cs_last_error().decode())
    assert bool((out.view(torch.int16) == FILL).all())


def _filled(shape, dtype=torch.float16):
    return torch.full(shape, FILL, dtype=torch.int16, device=DEV).view(dtype)


def test_rejections_return_their_code_and_leave_out_alone():
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt, device=DEV)
    # the biased form with N % 4 != 0 (the bias rows are read four keys wide)
    q, out = z(B, 6, H * 64), _filled((B, 6, H * 64))
    _reject(CS_E_UNSUPPORTED, launch("dh64_bias_f16", q, q, q, out, B, H, 6, 6, torch.zeros(H, 6, 6, device=DEV)), out)
    # head dim 48
    q, out = z(B, 16, H * 48), _filled((B, 16, H * 48))
    _reject(CS_E_UNSUPPORTED, launch("dh80", q, q, q, out, B, H, 16, 16, dh=48), out)
    # a row stride that is not a multiple of 8 elements, for each operand
    wide, out = z(B, 16, H * 80 + 4), _filled((B, 16, H * 80))
    q = z(B, 16, H * 80)
    for views in ((wide[:, :, :H * 80], q, q), (q, wide[:, :, :H * 80], q), (q, q, wide[:, :, :H * 80])):
        _reject(CS_E_SHAPE, launch("dh80", *views, out, B, H, 16, 16), out)
    outw = _filled((B, 16, H * 80 + 4))
    _reject(CS_E_SHAPE, launch("dh80", q, q, q, outw[:, :, :H * 80], B, H, 16, 16), outw)
    # bf16 outside head dims 64 (bias) / 128
    q, out = z(B, 16, H * 40, dt=torch.bfloat16), _filled((B, 16, H * 40), torch.bfloat16)
    _reject(CS_E_UNSUPPORTED, launch("dh40", q, q, q, out, B, H, 16, 16, dtype=torch.bfloat16), out)
