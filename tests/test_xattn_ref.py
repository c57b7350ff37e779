"""The yardstick of tests/test_xattn_forms_gpu.py, checked on the CPU: the emulator of the fused cross-attention block's rounding points (tests/xattn_ref.py)
against the float64 reference per (row, head) of the attention output and per row of the branch, the exact families against their closed forms bit for bit, the
bound on the branch recovered from a split output, and -- on the emulator, never on a GPU -- that the wrong kernels the GPU tests are meant to catch are caught:
a dropped last key, two swapped V rows, a denominator from the rounded P, a single rounding of q, and sample 0's kv for every sample.

The measured maxima are printed (pytest -s) and copied into the header of the GPU test file."""
import pytest
import torch

from tests import xattn_ref as R

B, HW = 2, 128
BOUND_FAMILIES = ("gauss", "dc", "peaky", "last")


@pytest.mark.parametrize("Nk", [13, 77, 80])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulator_against_fp64(family, Nk):
    """the two figures the GPU tests double: worst (row, head) of O (Wo = I: the patch is O) and worst row of the branch (random Wo, bo)"""
    if family == "nk1":
        Nk = 1
    co, cb = R.make_case(family, B, HW, Nk, identity_out=True), R.make_case(family, B, HW, Nk)
    assert torch.isfinite(co.ref_o).all() and torch.isfinite(cb.ref_branch).all()
    print(f"emulator vs fp64  {family:9s} Nk {Nk:2d}: worst (row, head) of O {co.emu_o:.3e}   worst row of the branch {cb.emu_branch:.3e}")
    # an implementation with exactly the documented roundings stays, in its worst row, inside a few fp16 ulps where the softmax is smooth, and inside 1 % where one key
    # carries a row (peaky, last: the rounding of q moves competing scores of size 2^5 by 2^-11 of their size)
    assert co.emu_o < (2e-3 if family in ("gauss", "dc") else 1.2e-2 if family in ("peaky", "last") else 1e-12)
    assert cb.emu_branch < (1.5e-3 if family in ("gauss", "dc") else 8e-3 if family in ("peaky", "last") else 1e-3)


def _exact_products(x, o):
    """the fp32 products of an exact family are exact: float64 and fp32 agree on O Wo^T + bo, and on LN Wq^T where LN is the constant beta"""
    br = o @ x.wo.double().T + x.bo.double()
    assert torch.equal(br, br.float().double())
    assert torch.equal(br, (o.float() @ x.wo.float().T + x.bo.float()).double())


@pytest.mark.parametrize("lo_grid", [False, True])
@pytest.mark.parametrize("family,Nk", [("selector", 80), ("selector", 77), ("selector", 5), ("nk1", 1), ("qround", 80), ("qround", 2), ("qround", 33)])
def test_exact_families_equal_their_closed_form(family, Nk, lo_grid):
    c = R.make_case(family, 3, 64, Nk, lo_grid=lo_grid)
    x, e = c.x, c.emu
    _exact_products(x, c.exact_o)
    if family != "nk1":
        q = x.beta.double() @ x.wq.double().T
        assert torch.equal(q, (x.beta.float() @ x.wq.float().T).double())
    assert torch.equal(e["O"].double(), c.exact_o)
    assert torch.equal(e["f"].double(), c.exact_f)                          # f is exact in fp32
    for lo8 in (False, True):
        y = x.with_lo(R.lo8_value(R.lo8_of(x.h_lo)).half()) if lo8 else x
        assert torch.equal(y.h_lo, x.h_lo)                                  # the lo grid holds e5m2 values: both split forms see the same stream
        got = R.xattn_emulated(y, lo8=lo8)
        hi, lo = R.split_planes(c.exact_f.float(), lo8)
        assert torch.equal(got["out"], hi) and torch.equal(got["lo8"] if lo8 else got["out_lo"], lo)
        if lo_grid:
            assert float((lo != 0).float().mean()) > 0.5, float((lo != 0).float().mean())      # the lo plane is exercised
    plain = R.xattn_emulated(x.with_lo(None))
    assert plain["out_lo"] is None and torch.equal(plain["out"], (c.exact_f - x.h_lo.double()).float().half())


def test_selector_sweep_visits_every_key_and_head():
    """default_jstar over t = 0 .. ceil(80 / B) - 1 puts the selected key of EVERY head on every position"""
    for Bn, Nk in ((3, 80), (2, 80), (3, 77), (2, 77)):
        seen = torch.zeros(R.NH, Nk, dtype=torch.bool)
        for t in range(-(-80 // Bn)):
            j = R.default_jstar(Bn, Nk, t)
            seen[torch.arange(R.NH)[None, :].expand(Bn, R.NH), j] = True
        assert bool(seen.all()), (Bn, Nk)


@pytest.mark.parametrize("family", BOUND_FAMILIES)
def test_branch_recovery_bound_holds_on_emulated_split_outputs(family):
    for identity in (True, False):
        c = R.make_case(family, B, HW, 77, identity_out=identity)
        e, x = c.emu, c.x
        rec = R.recover_branch(e["out"], e["out_lo"], x.h, x.h_lo)
        term = R.recovery_term(e["out"], e["out_lo"], x.h_lo)
        d = (rec - e["patch"].double()).abs()
        print(f"recovery {family:6s} identity {identity}: worst |recovered - patch| / bound {float((d / term).max()):.3f}   worst term / |patch| per row {float(R.term_rows(term, e['patch']).max()):.2e}")
        assert bool((d <= term).all())
        assert float((d / term).max()) > 0.01                               # ... and is not vacuous


# ---- the wrong kernels, on the emulator --------------------------------------------------------------------------------------------------------------------------
def _bound_o(c):
    return 2.0 * c.emu_o + R.F16_ULP


def _bound_branch(c):
    return 2.0 * c.emu_branch + R.F16_ULP


def _with_kv(x, kv):
    y = x.with_lo(x.h_lo)
    y.kv, y.Nk = kv.contiguous(), kv.shape[1]
    return y


@pytest.mark.parametrize("Nk", [2, 13, 17, 77, 80])
def test_a_dropped_last_key_breaks_the_last_family(Nk):
    """GPU tests 1 and 2 (family "last"): every branch row and most (row, head) pairs leave the bound by more than an order of magnitude"""
    co, cb = R.make_case("last", B, HW, Nk, identity_out=True), R.make_case("last", B, HW, Nk)
    eo = R.err_heads(R.xattn_emulated(_with_kv(co.x, co.x.kv[:, :Nk - 1]))["O"], co.ref_o)
    eb = R.err_rows(R.xattn_emulated(_with_kv(cb.x, cb.x.kv[:, :Nk - 1]))["patch"], cb.ref_branch)
    whole = float((R.xattn_fp64(_with_kv(cb.x, cb.x.kv[:, :Nk - 1]))[1] - cb.ref_branch).norm() / cb.ref_branch.norm())
    print(f"dropped key {Nk - 1}: (row, head) max {float(eo.max()):.2e} median {float(eo.median()):.2e} bound {_bound_o(co):.2e};  branch rows min {float(eb.min()):.2e} bound {_bound_branch(cb):.2e};  whole {whole:.2f}")
    assert float(eb.min()) >= 9e-3 and whole >= 0.4
    assert float(eo.max()) > 10 * _bound_o(co) and float(eb.max()) > 10 * _bound_branch(cb)
    assert float((eo > _bound_o(co)).double().mean(0).min()) > 0.2           # in every head, a good part of the rows


@pytest.mark.parametrize("family", ["gauss", "last"])
def test_swapped_v_rows_and_sample_0_kv_break_the_bounds(family):
    """GPU tests 1 and 2 on any family (and test 3 exactly: the selector sweep reads every V row of every head by position)"""
    c = R.make_case(family, B, HW, 77, identity_out=True)
    kv = c.x.kv.clone()
    kv[:, [20, 21], R.C:] = kv[:, [21, 20], R.C:]
    e = R.err_heads(R.xattn_emulated(_with_kv(c.x, kv))["O"], c.ref_o)
    print(f"{family}: V rows 20 / 21 swapped: worst (row, head) {float(e.max()):.2e} bound {_bound_o(c):.2e}")
    assert float(e.max()) > 10 * _bound_o(c)
    kv0 = c.x.kv[:1].expand(B, -1, -1)
    e = R.err_heads(R.xattn_emulated(_with_kv(c.x, kv0))["O"], c.ref_o)
    print(f"{family}: kv of sample 0 for every sample: worst (row, head) of sample 1 {float(e[HW:].max()):.2e}, min {float(e[HW:].min()):.2e}")
    assert float(e[:HW].max()) <= _bound_o(c) and float(e[HW:].min()) > 10 * _bound_o(c)
    s = R.make_case("selector", B, HW, 80, lo_grid=True)
    kv = s.x.kv.clone()
    j = int(s.jstar[1, 6])
    kv[1, [j, (j + 1) % 80], R.C:] = kv[1, [(j + 1) % 80, j], R.C:]
    assert not torch.equal(R.xattn_emulated(_with_kv(s.x, kv))["out"], s.emu["out"])


def test_a_denominator_from_the_rounded_p_fails_the_denom_family():
    """GPU test 3b: inside the 2 x emulator + ulp bounds of tests 1 and 2 by construction (a relative 4e-4), and outside BOTH checks of the denom family"""
    for Bn, hw, Nk in ((2, 128, 80), (3, 64, 77), (1, 192, 80)):
        c = R.make_case("denom", Bn, hw, Nk, identity_out=True)
        good = R.denom_check(c.emu["O"], c)
        bad = R.denom_check(R.xattn_emulated(c.x, denominator="rounded")["O"], c)
        print(f"denom B {Bn} Nk {Nk}: unrounded: excess {good[0]:+.3f} |mean| {good[1]:.2e};  rounded: excess {bad[0]:+.3f} |mean| {bad[1]:.2e};  bound on |mean| {good[2]:.2e}")
        assert good[0] <= 0 and good[1] <= good[2]
        assert bad[0] > 0 and bad[1] > 3 * bad[2]
    g = R.make_case("gauss", B, HW, 77, identity_out=True)
    e = R.err_heads(R.xattn_emulated(g.x, denominator="rounded")["O"], g.ref_o)
    assert float(e.max()) <= _bound_o(g)                                    # (which is why the family exists)


def test_a_single_rounding_of_q_fails_the_qround_family():
    """GPU test 3: O moves by O(1) in every head (the two tied keys get weights 2 : 1 or more instead of 1 : 1)"""
    t, two, one = R.qround_t()
    assert two != one and round(abs(two - one) * 8192) >= 1                # the scores differ by that whole number
    for Nk in (2, 33, 80):
        c = R.make_case("qround", B, HW, Nk, lo_grid=True)
        bad = R.xattn_emulated(c.x, q_roundings=1)
        d = (bad["O"].double() - c.exact_o).reshape(-1, R.NH, R.DH).abs().amax(-1)
        assert not torch.equal(bad["out"], c.emu["out"])
        assert float(d.min()) >= 1.0 / 6 - 1e-3, float(d.min())              # every (row, head): max |V_A - V_B| / 6 at the least (integer V rows that differ somewhere)
    g = R.make_case("gauss", B, HW, 77, identity_out=True)
    e = R.err_heads(R.xattn_emulated(g.x, q_roundings=1)["O"], g.ref_o)
    assert float(e.max()) <= _bound_o(g)


def test_fp64_reference_matches_torch():
    c = R.make_case("gauss", 2, 64, 13)
    x = c.x
    ln = torch.nn.functional.layer_norm(x.h.double(), (R.C,), x.gamma.double(), x.beta.double(), float(torch.tensor(R.EPS)))
    q = (ln @ x.wq.double().T).view(2, 64, 8, 40).transpose(1, 2)
    k, v = (t.double().view(2, 13, 8, 40).transpose(1, 2) for t in (x.kv[..., :R.C], x.kv[..., R.C:]))
    o = (torch.softmax(q @ k.transpose(-1, -2) * R.SCALE, -1) @ v).transpose(1, 2).reshape(-1, R.C)
    assert float((o - c.ref_o).abs().max()) < 1e-12
    assert float((o @ x.wo.double().T + x.bo.double() - c.ref_branch).abs().max()) < 1e-12
