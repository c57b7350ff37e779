"""cs_linear_step (consolver_amd/csrc/solver.hip), element by element, through the C ABI: bit for bit against the fp32 replica of tests/lin_ref.py (`lin_exact`)
and within the derived bound of the float64 form (`lin_fp64`).  Every output is a 16-byte-aligned slice of a NaN-filled buffer with 64 elements of margin on each
side (the harness of tests/test_solver_forms_gpu.py); the margins are all NaN after the call, and a refused call leaves the whole buffer NaN.  History tensors
past terms - 1 are handed over as pointers to NaN-filled tensors: the kernel must not read them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from consolver_amd import _lib as L
from tests import lin_ref as LR
from tests import solver_ref as R
from tests.test_solver_forms_gpu import CODE, DEV, Guarded, dev, p, st

pytestmark = pytest.mark.gpu


def build(c):
    """(args struct, {output name: Guarded}, tensors to keep alive) of a case of tests/lin_ref.py"""
    B, n, io, out = c["B"], c["elems"], c["io"], c["out"]
    shape = (B, n)
    xdt = "f32" if c["x_is_f32"] else io
    outs = {"x_out": Guarded(shape, out)}
    if c["lp"]:
        outs["x_out_lp"] = Guarded(shape, c["lp"])
    if c["want_m_out"]:
        outs["m_out"] = Guarded(shape, io)
    keep = []

    def d(a, dt):
        t = dev(a, dt)
        keep.append(t)
        return p(t)
    a = L.CsLinStepArgs()
    a.x, a.eps_text, a.eps_uncond, a.guidance, a.x_base = d(c["x"], xdt), d(c["ec"], io), d(c["eu"], io), c["g"], d(c["xb"], xdt)
    nan = np.full(shape, np.nan, np.float32)
    for k in range(LR.MAX_TERMS - 1):
        a.hist[k] = d(c["hist"][k] if k < c["terms"] - 1 else nan, io)
    a.terms = c["terms"]
    a.m_out = p(outs.get("m_out"))
    a.conv_x, a.conv_e, a.cx = c["scal"][:3]
    for k, v in enumerate(c["scal"][3]):
        a.c[k] = v
    for k in range(c["terms"], LR.MAX_TERMS):
        a.c[k] = float("nan")                                     # a coefficient past terms is not used
    a.B, a.elems, a.io_dtype, a.out_dtype, a.x_is_f32, a.x_out = B, n, CODE[io], CODE[out], c["x_is_f32"], p(outs["x_out"])
    a.x_out_lp, a.lp_dtype = p(outs.get("x_out_lp")), CODE[c["lp"] or "f32"]
    return a, outs, keep


def run_case(c):
    """launch, then every output: margins, torch.equal with the replica, every element within the bound of the float64 form.  Returns the worst err / bound."""
    a, outs, keep = build(c)
    L.check(L.lib().cs_linear_step(C.byref(a), st()))
    torch.cuda.synchronize()
    ex, rf = LR.lin_exact(c), LR.lin_fp64(c)
    assert set(ex) == set(outs) == set(rf), (c["name"], sorted(ex), sorted(outs))
    worst = 0.0
    for name, gd in outs.items():
        assert gd.margins_intact(), (c["name"], name, "wrote outside the tensor")
        got = gd.numpy()
        if not torch.equal(torch.from_numpy(got), torch.from_numpy(ex[name])):
            bad = np.flatnonzero(~((got == ex[name]).reshape(-1)))
            i = int(bad[0])
            raise AssertionError(f"{c['name']} {name}: {len(bad)} of {got.size} elements differ from the fp32 replica; first at flat index {i} "
                                 f"(sample {i // c['elems']}, element {i % c['elems']}): got {got.reshape(-1)[i]!r}, want {ex[name].reshape(-1)[i]!r}")
        r = R.within(got, rf[name])
        assert r <= 1.0, (c["name"], name, "err / bound vs float64", r)
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("form", R.DTYPE_FORMS, ids=R.form_id)
def test_lin_dtype_forms(form):
    """(io, out, x_is_f32, lp) x terms 1..4 x CFG x identity / real conversion x x_base absent / present x tail only / body + tail / two blocks"""
    cases = LR.lin_form_cases(form)
    worst = max(run_case(c) for c in cases)
    print(f"{len(cases)} cases bit-exact; worst err / bound vs float64 {worst:.3f}")


def test_lin_grid_stride():
    """8 * 256 * 2048 + 13 bf16 elements: one block more of work than the grid's cap, so the loop's second pass runs once; four terms, CFG, conversion, x_base"""
    worst = max(run_case(c) for c in LR.lin_grid_stride_cases())
    print(f"grid stride: worst err / bound vs float64 {worst:.3f}")


def test_identity_without_cfg_needs_no_m_out_and_copies_into_one_that_is_given():
    c = LR.make_lin("lin-mout", 3, 269, ("f16", "f32", 1, "f16"), terms=3, cfg=0, kind="identity", xbase=0, m_out=False)
    assert "m_out" not in LR.lin_exact(c)
    run_case(c)
    c = dict(c, want_m_out=True)
    a, outs, keep = build(c)
    L.check(L.lib().cs_linear_step(C.byref(a), st()))
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(outs["m_out"].numpy()), torch.from_numpy(c["ec"]))


def refused(c, code, mutate):
    a, outs, keep = build(c)
    extra = mutate(a, c) or []
    assert L.lib().cs_linear_step(C.byref(a), st()) == code, c["name"]
    torch.cuda.synchronize()
    for gd in list(outs.values()) + list(extra):
        assert gd.untouched(), c["name"]


def test_refusals_leave_outputs_untouched():
    """full-size device tensors, so that a missing refusal would be a valid launch that writes the outputs"""
    shape = (3, 269)
    c16 = LR.make_lin("refuse-lin", *shape, ("f16", "f16", 0, None), terms=3, cfg=1, kind="real", xbase=1)
    c32 = LR.make_lin("refuse-lin-f32", *shape, ("f32", "f32", 0, None), terms=3, cfg=1, kind="real", xbase=1)
    cx32 = LR.make_lin("refuse-lin-xf32", *shape, ("f16", "f32", 1, None), terms=3, cfg=1, kind="real", xbase=1)

    def set_(**kw):
        def m(a, c):
            for k, v in kw.items():
                setattr(a, k, v)
        return m
    for t in (0, -1, 5):
        refused(c16, R.CS_E_ARG, set_(terms=t))

    def null_hist(k):
        def m(a, c):
            a.hist[k] = None
        return m
    refused(c16, R.CS_E_ARG, null_hist(0))
    refused(c16, R.CS_E_ARG, null_hist(1))
    refused(c32, R.CS_E_DTYPE, set_(x_is_f32=1))                                 # x_is_f32 with fp32 io
    refused(cx32, R.CS_E_DTYPE, set_(out_dtype=CODE["f16"]))                     # an fp32 sample gives an fp32 result
    refused(c16, R.CS_E_DTYPE, set_(out_dtype=CODE["bf16"]))                     # the dtype pairs the dpm launcher refuses
    refused(c32, R.CS_E_DTYPE, set_(out_dtype=CODE["f16"]))
    refused(c16, R.CS_E_DTYPE, set_(io_dtype=7))

    def add_lp(a, c):
        g = Guarded(shape, "f16")
        a.x_out_lp, a.lp_dtype = g.ptr, CODE["f16"]
        return [g]
    refused(c16, R.CS_E_ARG, add_lp)                                             # an lp copy without an fp32 result

    def add_lp_f32(a, c):
        g = add_lp(a, c)
        a.lp_dtype = CODE["f32"]
        return g
    refused(c32, R.CS_E_ARG, add_lp_f32)                                         # ... or one that is not 16 bits wide
    refused(c16, R.CS_E_ARG, set_(m_out=None))                                   # CFG / a conversion without m_out
    refused(LR.make_lin("refuse-lin-conv", *shape, ("f16", "f16", 0, None), terms=2, cfg=0, kind="real", xbase=0), R.CS_E_ARG, set_(m_out=None))
    refused(c16, R.CS_E_ARG, set_(x=None))
    refused(c16, R.CS_E_ARG, set_(x_out=None))
    refused(c16, R.CS_E_SHAPE, set_(B=-1))
    # aliasing: x_out on an input, m_out on a history entry that is read
    refused(c16, R.CS_E_ARG, lambda a, c: setattr(a, "x_out", a.x_base))
    refused(c16, R.CS_E_ARG, lambda a, c: setattr(a, "m_out", a.hist[1]))
    assert L.lib().cs_linear_step(None, st()) == R.CS_E_ARG


def test_unread_history_entry_may_alias_m_out_and_empty_batch_is_a_no_op():
    c = LR.make_lin("lin-alias", 3, 269, ("f16", "f16", 0, None), terms=2, cfg=1, kind="identity", xbase=0)
    a, outs, keep = build(c)
    a.hist[2] = a.m_out                                                          # hist[2] is not read at terms = 2
    L.check(L.lib().cs_linear_step(C.byref(a), st()))
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(outs["x_out"].numpy()), torch.from_numpy(LR.lin_exact(c)["x_out"]))
    a, outs, keep = build(c)
    a.B = 0
    a.x = a.eps_text = a.x_out = None
    L.check(L.lib().cs_linear_step(C.byref(a), st()))
    torch.cuda.synchronize()
    assert all(g.untouched() for g in outs.values())
