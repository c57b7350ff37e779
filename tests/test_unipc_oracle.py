"""CPU tests of UniPC: the oracle (tests/unipc_oracle.py) against anchors that do not rest on memory of diffusers, UniPCMultistepScheduler's
host scalars against the oracle, its config and refusals, and the argument checks of cs_unipc_step (no GPU: they run before any launch)."""
import ctypes

import numpy as np
import pytest

from consolver_amd import SD15_UNIPC_KWARGS, UniPCMultistepScheduler, _lib
from tests.dpm_oracle import DPMSolverOracle
from tests.unipc_oracle import UniPCOracle, combo_id, combos

SD15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
SHAPE = (2, 3, 5, 7)


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def max_rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1.0))


def trajectories(a, b, n, seed=0):
    """both oracles on the same noise and the same state-independent eps; the worst difference of the samples over the steps"""
    rng = np.random.default_rng(seed)
    a.set_timesteps(n); b.set_timesteps(n)
    assert np.array_equal(a.timesteps, b.timesteps) and np.array_equal(a.sigmas, b.sigmas)
    xa = xb = rng.standard_normal(SHAPE)
    worst = 0.0
    for _ in range(n):
        e = rng.standard_normal(SHAPE)
        xa, xb = a.step(e, xa), b.step(e, xb)
        worst = max(worst, max_rel(xa, xb))
    return worst


# ------------------------------------------------------------------------------------------------ anchors of the oracle
@pytest.mark.parametrize("n", [5, 8, 16])
@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("st", ["bh1", "bh2"])
def test_order1_without_corrector_is_dpmsolverpp_order1(st, pt, n):
    """(a) UniP-1 is DDIM in the x0 form whatever B(h) is: the dpmsolver++ order-1 run of tests/dpm_oracle.py (which the golden-pinned DDIM anchors) on the same grid"""
    u = UniPCOracle(**SD15, solver_order=1, solver_type=st, prediction_type=pt, disable_corrector=range(n))
    d = DPMSolverOracle(**SD15, solver_order=1, algorithm_type="dpmsolver++", prediction_type=pt, final_sigmas_type="sigma_min")
    err = trajectories(u, d, n)
    print("unipc order 1 vs dpm++ order 1", st, pt, n, err)
    assert err <= 1e-12


@pytest.mark.parametrize("n", [5, 8, 16])
def test_order2_bh2_without_corrector_is_dpmsolverpp_2m_midpoint(n):
    """(b) with rho_p = 1/2 and B(h) = expm1(-h), UniP-2 is DPM-Solver++ 2M midpoint; UniPC's lower_order_final makes the last step first order at every n
    (euler_at_final on the DPM side)"""
    u = UniPCOracle(**SD15, solver_order=2, solver_type="bh2", disable_corrector=range(n))
    d = DPMSolverOracle(**SD15, solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", final_sigmas_type="sigma_min", euler_at_final=True)
    err = trajectories(u, d, n)
    print("unipc order 2 bh2 vs dpm++ 2M", n, err)
    assert err <= 1e-12


def exact_step(o, s, t, x_s, c):
    """x_t = sigma_t / sigma_s x_s + sigma_t int_{lambda_s}^{lambda_t} e^lambda m(lambda) dlambda for m = c0 + c1 lambda + c2 lambda^2, in closed form
    (sigma here is the VP one, sigma alpha of the oracle's parametrisation)"""
    _, sg_s = o.alpha_sigma(o.sigmas[s])
    _, sg_t = o.alpha_sigma(o.sigmas[t])
    F = lambda l: np.exp(l) * (c[0] + c[1] * (l - 1.0) + c[2] * (l * l - 2.0 * l + 2.0))
    return sg_t / sg_s * x_s + sg_t * (F(o.lam(t)) - F(o.lam(s)))


@pytest.mark.parametrize("st", ["bh1", "bh2"])
@pytest.mark.parametrize("n", [5, 8, 16])
def test_solved_corrector_is_exact_for_quadratic_model_outputs(n, st):
    """(c) UniC-2 interpolates m at lambda_{i-2}, lambda_{i-1} and lambda_i: with rho_c = solve(R, b) the update is the exact solution when m is a quadratic
    in lambda, for both B(h); the first-order predictor is exact for a constant m."""
    rng = np.random.default_rng(n)
    o = UniPCOracle(**SD15, solver_order=2, solver_type=st)
    o.set_timesteps(n)
    x = rng.standard_normal(SHAPE)
    worst = 0.0
    for i in range(2, n):
        c = [rng.standard_normal(SHAPE) for _ in range(3)]
        m = lambda k: c[0] + c[1] * o.lam(k) + c[2] * o.lam(k) ** 2
        o.step_index = i
        o.model_outputs = [m(i - 2), m(i - 1)]
        got = o.corrector(m(i), x, 2)
        worst = max(worst, max_rel(got, exact_step(o, i - 1, i, x, c)))
    for i in range(n):
        c0 = rng.standard_normal(SHAPE)
        o.step_index = i
        o.model_outputs = [None, c0]
        worst = max(worst, max_rel(o.predictor(x, 1), exact_step(o, i, i + 1, x, [c0, 0.0, 0.0])))
    print("unipc exactness", st, n, worst)
    assert worst <= 1e-12


def test_hard_coded_half_cases():
    """(d) the order-2 predictor and the order-1 corrector take rho = 1/2 instead of solving: NOT exact for a linear m (nothing to assert there); under bh2 the order-1
    corrector is the trapezoid  sigma_t / sigma_s x_last - alpha_t expm1(-h) (m0 + m_new) / 2."""
    rng = np.random.default_rng(3)
    n = 8
    o = UniPCOracle(**SD15, solver_order=2, solver_type="bh2")
    o.set_timesteps(n)
    x, m0, m_new = (rng.standard_normal(SHAPE) for _ in range(3))
    for i in range(1, n):
        o.step_index = i
        o.model_outputs = [None, m0]
        got = o.corrector(m_new, x, 1)
        alpha_t, sg_t = o.alpha_sigma(o.sigmas[i])
        _, sg_s = o.alpha_sigma(o.sigmas[i - 1])
        h = o.lam(i) - o.lam(i - 1)
        want = sg_t / sg_s * x - alpha_t * np.expm1(-h) * (m0 + m_new) / 2.0
        assert max_rel(got, want) <= 1e-12, i
    # the defect of the order-2 predictor for a linear m on this grid, step 2 -> 3: measured, not asserted exact
    c = [rng.standard_normal(SHAPE), rng.standard_normal(SHAPE), 0.0]
    o.step_index = 2
    o.model_outputs = [c[0] + c[1] * o.lam(1), c[0] + c[1] * o.lam(2)]
    defect = max_rel(o.predictor(x, 2), exact_step(o, 2, 3, x, c))
    print("order-2 predictor defect for linear m, n = 8, step 2 -> 3:", defect)
    assert defect > 1e-9


# ------------------------------------------------------------------------------------------------ scheduler against oracle
class ScalarRun:
    """UniPCMultistepScheduler.step_scalars applied in numpy fp64, with the state the kernel path keeps (two converted outputs, last_sample)"""
    def __init__(self, sch):
        self.s, self.m, self.last, self.i = sch, [], None, 0

    def step(self, eps, x):
        conv_x, conv_e, (a_x, a_0, a_1, a_n), (p_x, p_0, p_1), use_corr = self.s.step_scalars(self.i)
        m_new = conv_x * x + conv_e * eps
        m0 = self.m[0] if len(self.m) > 0 else 0.0
        m1 = self.m[1] if len(self.m) > 1 else 0.0
        assert (len(self.m) > 0 or (a_0 == 0.0 and p_1 == 0.0)) and (len(self.m) > 1 or a_1 == 0.0)
        x_c = a_x * self.last + a_0 * m0 + a_1 * m1 + a_n * m_new if use_corr else x
        x_next = p_x * x_c + p_0 * m_new + p_1 * m0
        self.m, self.last, self.i = [m_new] + self.m[:1], x_c, self.i + 1
        return m_new, x_c, x_next


@pytest.mark.parametrize("n", [5, 16])
@pytest.mark.parametrize("combo", list(combos(16)), ids=combo_id)
def test_step_scalars_reproduce_the_oracle(combo, n):
    rng = np.random.default_rng(11)
    kw = dict(SD15, **combo)
    s, o = UniPCMultistepScheduler(**kw), UniPCOracle(**kw)
    s.set_timesteps(n); o.set_timesteps(n)
    assert np.array_equal(s.timesteps.numpy(), o.timesteps) and np.array_equal(s.sigmas.numpy().astype(np.float64), o.sigmas)
    r = ScalarRun(s)
    x = xo = rng.standard_normal(SHAPE)
    worst = 0.0
    for i in range(n):
        e = rng.standard_normal(SHAPE)
        m_new, x_c, x = r.step(e, x)
        xo = o.step(e, xo)
        worst = max(worst, rel_l2(m_new, o.last_converted()), rel_l2(x_c, o.corrected), rel_l2(x, xo))
    print("unipc scalars vs oracle", combo_id(combo), n, worst)
    assert worst < 1e-6


@pytest.mark.parametrize("order", [1, 2])
def test_final_sigma_zero_last_step_returns_the_x0_prediction(order):
    n = 5
    s = UniPCMultistepScheduler(**SD15, solver_order=order, final_sigmas_type="zero")
    o = UniPCOracle(**SD15, solver_order=order, final_sigmas_type="zero")
    s.set_timesteps(n); o.set_timesteps(n)
    assert s.sigmas[-1] == 0.0
    *_, (p_x, p_0, p_1), _ = s.step_scalars(n - 1)
    assert (p_x, p_0, p_1) == (0.0, 1.0, 0.0)
    rng = np.random.default_rng(5)
    r = ScalarRun(s)
    x = xo = rng.standard_normal(SHAPE)
    for i in range(n):
        e = rng.standard_normal(SHAPE)
        m_new, _, x = r.step(e, x)
        xo = o.step(e, xo)
        assert rel_l2(x, xo) < 1e-6
    assert np.array_equal(x, m_new)


# ------------------------------------------------------------------------------------------------ config and errors
def test_config_round_trip_defaults_and_history_slots():
    s = UniPCMultistepScheduler()
    c = s.config
    assert (c.solver_order, c.prediction_type, c.predict_x0, c.solver_type, c.lower_order_final, list(c.disable_corrector), c.timestep_spacing, c.steps_offset,
            c.final_sigmas_type, c.thresholding, c.use_karras_sigmas) == (2, "epsilon", True, "bh2", True, [], "linspace", 0, "sigma_min", False, False)
    s = UniPCMultistepScheduler(**SD15_UNIPC_KWARGS, solver_type="bh1", disable_corrector=[0, 2])
    t = UniPCMultistepScheduler.from_config(s.config)
    pub = lambda c: {k: v for k, v in dict(c).items() if not k.startswith("_")}
    assert pub(t.config) == pub(s.config) and t.config.steps_offset == 1 and t.config.beta_schedule == "scaled_linear"
    s.set_timesteps(6); t.set_timesteps(6)
    assert s.step_scalars(3) == t.step_scalars(3) and s.step_scalars(3)[-1] is False and s.step_scalars(2)[-1] is True
    assert s.history_slots == 3 and UniPCMultistepScheduler(solver_order=1).history_slots == 2
    assert s.step_index is None and s.last_sample is None and len(s) == 1000 and s.init_noise_sigma == 1.0


def test_refusals():
    for kw in (dict(solver_order=3), dict(predict_x0=False), dict(thresholding=True), dict(use_karras_sigmas=True), dict(solver_type="logrho")):
        with pytest.raises(NotImplementedError):
            UniPCMultistepScheduler(**kw)
    for kw in (dict(final_sigmas_type="zero", lower_order_final=False), dict(final_sigmas_type="one"), dict(prediction_type="sample"), dict(timestep_spacing="x")):
        with pytest.raises(ValueError):
            UniPCMultistepScheduler(**kw)
    s = UniPCMultistepScheduler()
    with pytest.raises(ValueError):
        s.step_scalars(0)                                                      # before set_timesteps
    with pytest.raises(ValueError):
        s.set_timesteps(0)


# ------------------------------------------------------------------------------------------------ C ABI
def test_unipc_struct_layout_and_argument_errors():
    """argument validation happens before any launch -> usable without a GPU (as test_struct_layout_matches_header)"""
    assert ctypes.sizeof(_lib.CsUnipcStepArgs) % 8 == 0
    assert ctypes.sizeof(_lib.CsUnipcStepArgs) == 7 * 8 + 2 * 8 + 4 * 4 + 4 * 8 + 4 + 9 * 4
    l = _lib.lib()
    assert l.cs_unipc_step(None, None) == -1
    a = _lib.CsUnipcStepArgs()
    a.B, a.elems = 1, 8
    a.io_dtype = a.out_dtype = _lib.CS_F32
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"required" in l.cs_last_error()
    a.x = a.eps_text = a.x_out = a.m_out = 16
    a.B = -1
    assert l.cs_unipc_step(ctypes.byref(a), None) == -2
    a.B = 1
    a.x_is_f32 = 1                                                             # fp32 io has no separate fp32 sample
    assert l.cs_unipc_step(ctypes.byref(a), None) == -3
    a.x_is_f32, a.out_dtype = 0, _lib.CS_F16                                   # fp32 io gives an fp32 result
    assert l.cs_unipc_step(ctypes.byref(a), None) == -3
    a.io_dtype, a.out_dtype = _lib.CS_F16, _lib.CS_F32                         # an fp32 result beside 16-bit outputs is an fp32 sample
    assert l.cs_unipc_step(ctypes.byref(a), None) == -3
    a.io_dtype = a.out_dtype = _lib.CS_F32
    a.x_out_lp, a.lp_dtype = 16, _lib.CS_F32
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"x_out_lp" in l.cs_last_error()
    a.x_out_lp = None
    a.use_corr = 1                                                             # the corrector without x_last
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"x_last" in l.cs_last_error()
    a.x_last, a.a_0 = 16, 0.5                                                  # a non-zero coefficient without its history tensor
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"m_prev0" in l.cs_last_error()
    a.a_0, a.p_1 = 0.0, 0.5
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"m_prev0" in l.cs_last_error()
    a.m_prev0, a.a_1 = 16, 0.25
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"m_prev1" in l.cs_last_error()
    a.m_prev1 = 16
    a.x = 20                                                                   # 4-byte aligned only
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"aligned" in l.cs_last_error()
    a.x, a.m_prev1 = 16, 24
    assert l.cs_unipc_step(ctypes.byref(a), None) == -1 and b"aligned" in l.cs_last_error()
    a.B = 0
    assert l.cs_unipc_step(ctypes.byref(a), None) == 0                         # empty batch is a no-op
    a.B, a.elems = 1, 0
    assert l.cs_unipc_step(ctypes.byref(a), None) == 0
