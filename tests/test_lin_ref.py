"""tests/lin_ref.py on the CPU, on the inputs the GPU test uses: the fp32 replica of cs_linear_step lies within the derived bound of the float64 form, and
its parts are what they claim to be."""
import numpy as np
import pytest

from tests import lin_ref as LR
from tests import solver_ref as R


@pytest.mark.parametrize("form", R.DTYPE_FORMS, ids=R.form_id)
def test_replica_within_the_float64_bound(form):
    worst = 0.0
    for c in LR.lin_form_cases(form):
        ex, rf = LR.lin_exact(c), LR.lin_fp64(c)
        assert set(ex) == set(rf) == {"x_out"} | ({"m_out"} if c["want_m_out"] else set()) | ({"x_out_lp"} if c["lp"] else set()), c["name"]
        for name in ex:
            r = R.within(ex[name], rf[name])
            assert r <= 1.0, (c["name"], name, r)
            worst = max(worst, r)
    print(f"{R.form_id(form)}: worst err / bound {worst:.3f}")


def test_cases_cover_what_they_say():
    cases = LR.lin_form_cases(("f16", "f32", 1, "f16"))
    assert len(cases) == 3 * 4 * 2 * 2 * 2
    assert {c["terms"] for c in cases} == {1, 2, 3, 4} and {len(c["hist"]) for c in cases} == {0, 1, 2, 3}
    assert any(c["xb"] is None for c in cases) and any(c["xb"] is not None for c in cases)
    assert any(not c["want_m_out"] for c in cases) and all(c["want_m_out"] for c in cases if c["eu"] is not None or not LR._identity(c))
    for c in cases:
        assert len(c["scal"][3]) == c["terms"] and all(np.isfinite(c["scal"][3])) and np.isfinite(c["scal"][:3]).all()
        assert LR._identity(c) == (c["scal"][:2] == (0.0, 1.0))


def test_replica_is_the_plain_formula_where_nothing_rounds():
    """small integers and dyadic coefficients: every fp32 operation is exact, so the replica equals the formula evaluated in float64"""
    rng = np.random.default_rng(0)
    t = lambda: rng.integers(-8, 9, size=(2, 11)).astype(np.float32)
    x, xb, ec, eu, h = t(), t(), t(), t(), [t(), t(), t()]
    c = dict(io="f32", out="f32", x_is_f32=0, lp="f16", terms=4, x=x, xb=xb, ec=ec, eu=eu, g=2.0, hist=h, scal=(0.5, 0.25, 2.0, [1.0, -0.5, 0.25, 4.0]),
             want_m_out=True)
    e = eu + 2.0 * (ec - eu)
    m0 = 0.5 * x + 0.25 * e
    want = 2.0 * xb + m0 - 0.5 * h[0] + 0.25 * h[1] + 4.0 * h[2]
    ex = LR.lin_exact(c)
    assert np.array_equal(ex["m_out"], m0) and np.array_equal(ex["x_out"], want) and np.array_equal(ex["x_out_lp"], want)
    ex = LR.lin_exact(dict(c, xb=None, terms=2, eu=None, g=1.0, scal=(0.0, 1.0, 2.0, [1.0, -0.5])))
    assert np.array_equal(ex["m_out"], ec) and np.array_equal(ex["x_out"], 2.0 * x + ec - 0.5 * h[0])
