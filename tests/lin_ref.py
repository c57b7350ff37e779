"""CPU references, case lists and seeded inputs of cs_linear_step (consolver_amd/csrc/solver.hip), in the forms of tests/solver_ref.py, whose helpers they are
built from (rnd, rnd64, spacing, within, the error-carrying float64 class T, DTYPE_FORMS, small_shapes).  tests/test_lin_step_gpu.py runs the kernel on them.

``lin_exact``  the kernel's operation order in numpy fp32: one fp32 operation or one round-to-nearest-even conversion per step, scalars rounded to fp32 first.
               solver.hip is built with -ffp-contract=off, so the GPU is expected to give the same bits:
                   eps = eu is None ? ec : rnd_io(eu + g (ec - eu));   m0 = identity ? eps : rnd_io(conv_x x + conv_e eps);
                   r = cx xb + c[0] m0;  r = r + c[k] hist[k - 1], k = 1 .. terms - 1;   x_out = rnd_out(r);   x_out_lp = rnd_lp(r)
``lin_fp64``   the same operation in float64 with the documented rounding points (the CFG combine and the conversion to the io dtype, the result to the out
               dtype, the 16-bit copy from the fp32 result) applied to the exact values.  Returns (reference, bound) per output.

The bound is solver_ref's class T carried through the operations above: each of the path's fp32 operations -- the CFG combine's three, the conversion's three,
then one product and one sum per term, 2 terms + 1 in all -- contributes 2^-24 of the magnitude of its own result to everything computed from it, a rounding
point to a 16-bit grid moves a value by at most one grid step and only where a rounding boundary lies within the error carried so far, and the acceptance
adds half an ulp of the output dtype.  With four terms and CFG that is 15 roundings in front of the last one.
"""
import numpy as np

from tests import solver_ref as R
from tests.solver_ref import F32, F64, T, cfg_exact, cfg_fp64, f32, rnd, spacing

MAX_TERMS = 4


def _identity(c):
    return f32(c["scal"][0]) == 0 and f32(c["scal"][1]) == 1


def lin_exact(c):
    """c: a case dict of make_lin.  Returns dict(x_out, m_out?, x_out_lp?) as fp32 arrays holding values of the tensors' dtypes."""
    io, x = c["io"], c["x"]
    conv_x, conv_e, cx = (f32(v) for v in c["scal"][:3])
    cs = [f32(v) for v in c["scal"][3]]
    e = cfg_exact(c["ec"], c["eu"], c["g"], io)
    m0 = e if _identity(c) else rnd(((conv_x * x).astype(F32) + (conv_e * e).astype(F32)).astype(F32), io)
    xb = x if c["xb"] is None else c["xb"]
    r = ((cx * xb).astype(F32) + (cs[0] * m0).astype(F32)).astype(F32)
    for k in range(1, c["terms"]):
        r = (r + (cs[k] * c["hist"][k - 1]).astype(F32)).astype(F32)
    out = dict(x_out=rnd(r, c["out"]))
    if c["want_m_out"]:
        out["m_out"] = m0
    if c["lp"]:
        out["x_out_lp"] = rnd(r, c["lp"])
    return out


def lin_fp64(c):
    io, x = c["io"], T(c["x"])
    conv_x, conv_e, cx = (T(F64(f32(v))) for v in c["scal"][:3])
    cs = [T(F64(f32(v))) for v in c["scal"][3]]
    e = cfg_fp64(c["ec"], c["eu"], c["g"], io)
    m0 = e if _identity(c) else (conv_x * x + conv_e * e).rnd(io)
    xb = x if c["xb"] is None else T(c["xb"])
    r = cx * xb + cs[0] * m0
    for k in range(1, c["terms"]):
        r = r + cs[k] * T(c["hist"][k - 1])
    out = dict(x_out=r.result(c["out"]))
    if c["want_m_out"]:
        out["m_out"] = (m0.v, m0.e + 0.5 * spacing(m0.v, io))
    if c["lp"]:
        out["x_out_lp"] = r.rnd("f32").result(c["lp"])
    return out


# ----------------------------------------------------------------------------------------------------------------- inputs
def lin_scalars(terms, kind):
    """(conv_x, conv_e, cx, [c_0 .. c_(terms-1)]) of real steps of 8-step runs on SD1.5's schedule.  'identity': PNDMScheduler at forwards 0, 2, 3, 5 (one to
    four model outputs; conv (0, 1)).  'real': DEISMultistepScheduler under v prediction (the conversion sigma x + alpha v) at steps 0, 1, 4 for one to
    three terms; with four terms, that conversion in front of iPNDM's four-term combination."""
    from consolver_amd import DEISMultistepScheduler, PNDMScheduler, SD15_DEIS_KWARGS, SD15_PNDM_KWARGS
    p = PNDMScheduler(**SD15_PNDM_KWARGS)
    p.set_timesteps(8)
    cx, cs, _ = p.step_scalars({1: 0, 2: 2, 3: 3, 4: 5}[terms])
    if kind == "identity":
        return 0.0, 1.0, float(cx), [float(v) for v in cs]
    d = DEISMultistepScheduler(**dict(SD15_DEIS_KWARGS, solver_order=3, prediction_type="v_prediction"))
    d.set_timesteps(8)
    conv_x, conv_e, dcx, dcs = d.step_scalars({1: 0, 2: 1, 3: 4, 4: 4}[terms])
    if terms < 4:
        cx, cs = dcx, dcs
    assert len(cs) == terms
    return float(conv_x), float(conv_e), float(cx), [float(v) for v in cs]


def make_lin(name, B, elems, form, *, terms, cfg, kind, xbase, m_out=True):
    """m_out may be absent only without CFG and conversion (``m_out=False`` is honoured there alone)"""
    io, out, xf, lp = form
    rng = np.random.default_rng(R._seed(name))
    c = dict(kernel="lin", name=name, B=B, elems=elems, io=io, out=out, x_is_f32=xf, lp=lp, terms=terms)
    xdt = "f32" if xf else io
    c["x"] = R.tensor(rng, B, elems, xdt)
    c["xb"] = R.tensor(rng, B, elems, xdt) if xbase else None
    c["ec"] = R.tensor(rng, B, elems, io)
    c["eu"] = R.tensor(rng, B, elems, io) if cfg else None
    c["g"] = 7.5 if cfg else 1.0
    c["hist"] = [R.tensor(rng, B, elems, io) for _ in range(terms - 1)]
    c["scal"] = R.cached(("lin", terms, kind), lambda: lin_scalars(terms, kind))
    c["want_m_out"] = bool(cfg or kind != "identity" or m_out)
    return c


LIN_VARIANTS = [dict(terms=t, cfg=g, kind=k, xbase=b) for t in range(1, MAX_TERMS + 1) for g in (0, 1) for k in ("identity", "real") for b in (0, 1)]


def lin_form_cases(form):
    """terms 1..4 x CFG x identity / real conversion x x_base absent / present, x the three small shapes; m_out absent where it may be, on the middle shape"""
    tag = f"lin-{R.form_id(form)}"
    return [make_lin(f"{tag}-{B}x{n}-t{v['terms']}g{v['cfg']}{v['kind']}b{v['xbase']}", B, n, form, m_out=(n != 269), **v)
            for B, n in R.small_shapes(form[0]) for v in LIN_VARIANTS]


def lin_grid_stride_cases():
    """one flat range past the 2048-block cap: the loop's second pass runs once, and there is a tail"""
    return [make_lin("lin-gridstride", *R.FLAT_GRID_STRIDE, ("bf16", "bf16", 0, None), terms=4, cfg=1, kind="real", xbase=1)]
