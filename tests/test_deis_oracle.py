"""CPU tests of DEIS: the host scalars of consolver_amd/scheduling_deis.py and the independent restatement tests/deis_oracle.py against quadrature of the
Lagrange basis in log rho, against the first-order DPM-Solver, against the exact solution for a model output that is a polynomial in log rho, and
against each other."""
import numpy as np
import pytest
from scipy.integrate import quad

from consolver_amd import SD15_DEIS_KWARGS, SD15_MULTISTEP_DPM_KWARGS, DEISMultistepScheduler, DPMSolverMultistepScheduler
from oracle import solver_oracle as so
from tests.deis_oracle import DEISOracle, expected_orders

GRIDS = {4: [999, 749, 500, 250], 8: [999, 874, 749, 624, 500, 375, 250, 125]}
ORDERS = {(3, 8): [1, 2, 3, 3, 3, 3, 2, 1], (3, 4): [1, 2, 2, 1], (3, 20): [1, 2] + [3] * 18,
          (2, 8): [1, 2, 2, 2, 2, 2, 2, 1], (2, 4): [1, 2, 2, 1], (2, 20): [1] + [2] * 19,
          (1, 8): [1] * 8, (1, 4): [1] * 4, (1, 20): [1] * 20}


def sched(n, **kw):
    s = DEISMultistepScheduler(**dict(SD15_DEIS_KWARGS, **kw))
    s.set_timesteps(n)
    return s


def alpha(rho):
    return 1.0 / np.sqrt(rho * rho + 1.0)


@pytest.mark.parametrize("n", [4, 8])
def test_grid_and_sigma_tables(n):
    s = sched(n)
    assert s.timesteps.tolist() == GRIDS[n] and s.num_inference_steps == n
    ac = so.alphas_cumprod(so.make_betas("scaled_linear", 0.00085, 0.012)).astype(np.float64)
    rho = np.sqrt((1 - ac) / ac)
    want = np.concatenate([rho[GRIDS[n]], rho[:1]]).astype(np.float32)          # integer timesteps: the interpolation is a look-up; the last is timestep 0's
    assert s._sigmas.dtype == np.float32 and np.array_equal(s._sigmas, want) and np.array_equal(s.sigmas.numpy(), want)
    o = DEISOracle(**{k: v for k, v in SD15_DEIS_KWARGS.items()})
    o.set_timesteps(n)
    assert np.array_equal(o.timesteps, GRIDS[n]) and np.array_equal(o.sigmas, want.astype(np.float64))
    assert s.config.solver_order == 2 and s.config.algorithm_type == "deis" and s.config.solver_type == "logrho" and s.config.lower_order_final
    assert s.config.timestep_spacing == "linspace" and s.config.prediction_type == "epsilon" and s.config.steps_offset == 1
    assert s.factor_net is None and s.history_slots == 2 and sched(n, solver_order=3).history_slots == 3


@pytest.mark.parametrize("key", sorted(ORDERS), ids=lambda k: f"order{k[0]}-n{k[1]}")
def test_order_per_step(key):
    order, n = key
    s = sched(n, solver_order=order)
    assert [s._order(i, min(i, order)) for i in range(n)] == ORDERS[key] == expected_orders(order, n)
    assert [len(s.step_scalars(i)[3]) for i in range(n)] == ORDERS[key]
    o = DEISOracle(**dict(SD15_DEIS_KWARGS, solver_order=order))
    o.set_timesteps(n)
    x = np.ones(3)
    for _ in range(n):
        x = o.step(np.ones(3), x)
    assert o.orders == ORDERS[key]
    if n >= 15:                                                                   # no lower orders at the end of a long run unless lower_order_final says so
        assert [sched(n, solver_order=order, lower_order_final=False)._order(i, min(i, order)) for i in range(n)] == ORDERS[key]
    else:
        s = sched(n, solver_order=order, lower_order_final=False)
        assert [s._order(i, min(i, order)) for i in range(n)] == [min(i + 1, order) for i in range(n)]


def lagrange(j, nodes):
    def f(rho):
        u, v = np.log(rho), 1.0
        for k, uk in enumerate(nodes):
            if k != j:
                v *= (u - uk) / (nodes[j] - uk)
        return v
    return f


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("n", [4, 8])
def test_step_scalars_against_quadrature(n, order):
    """c_j = alpha_t int_{rho_s0}^{rho_t} L_j(log rho) d rho on every step that has the history for it, 1e-12 relative (measured <= 1e-14; the two decades cover
    quad's own round-off); and sum C_j = rho_t - rho_s0, the exactness for a constant model output"""
    s = sched(n, solver_order=3)
    rho = s._sigmas.astype(np.float64)
    worst = 0.0
    for i in range(order - 1, n):
        conv_x, conv_e, cx, cs = s.step_scalars(i, order)
        assert (conv_x, conv_e) == (0.0, 1.0) and len(cs) == order
        a_t = alpha(rho[i + 1])
        assert abs(cx / (a_t / alpha(rho[i])) - 1) <= 1e-15
        nodes = [np.log(rho[i - j]) for j in range(order)]
        for j in range(order):
            want, _ = quad(lagrange(j, nodes), rho[i], rho[i + 1], epsabs=0.0, epsrel=2e-14, limit=200)
            rel = abs(cs[j] / (a_t * want) - 1)
            worst = max(worst, rel)
            assert rel <= 1e-12, (i, j, cs[j], a_t * want)
        assert abs(sum(cs) / (a_t * (rho[i + 1] - rho[i])) - 1) <= 1e-13, i
    print(f"n={n} order={order}: worst relative difference to quadrature {worst:.2e}")


@pytest.mark.parametrize("n", [4, 8])
def test_first_order_is_the_dpm_solver_step(n):
    s = sched(n)
    d = DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS)
    d.set_timesteps(n)
    assert np.array_equal(s._sigmas, d._sigmas)
    for i in range(n):
        conv_x, conv_e, cx, cs = s.step_scalars(i, 1)
        dx, de, dcx, dc0, dc1 = d.step_scalars(i, first_order=True)
        assert (conv_x, conv_e) == (dx, de) == (0.0, 1.0) and dc1 == 0.0 and len(cs) == 1
        assert abs(cx / dcx - 1) <= 1e-14 and abs(cs[0] / dc0 - 1) <= 1e-14, (i, cx, dcx, cs[0], dc0)


@pytest.mark.parametrize("order", [2, 3])
def test_exact_for_a_polynomial_in_log_rho(order):
    """eps(rho) = a + b log rho (+ c log^2 rho) per element: with the history at its exact values one step of order 2 (3) gives alpha_t (x / alpha_s0 +
    int eps d rho), from the scheduler's scalars and from the oracle's step"""
    n, rng = 8, np.random.default_rng(order)
    s = sched(n, solver_order=3)
    rho = s._sigmas.astype(np.float64)
    a, b, c = rng.standard_normal((3, 16))
    if order == 2:
        c = 0 * c

    def eps(r):
        return a + b * np.log(r) + c * np.log(r) ** 2

    def prim(r):
        u = np.log(r)
        return a * r + b * r * (u - 1) + c * r * (u * u - 2 * u + 2)
    for i in range(order - 1, n):
        x = rng.standard_normal(16)
        want = alpha(rho[i + 1]) * (x / alpha(rho[i]) + prim(rho[i + 1]) - prim(rho[i]))
        _, _, cx, cs = s.step_scalars(i, order)
        got = cx * x + sum(ck * eps(rho[i - k]) for k, ck in enumerate(cs))
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), i
        o = DEISOracle(**dict(SD15_DEIS_KWARGS, solver_order=3))
        o.set_timesteps(n)
        o.step_index, o.lower_order_nums = i, 3
        o.model_outputs = [eps(rho[i - k]) if i - k >= 0 else None for k in (3, 2, 1)]
        if i >= n - 2:                                                            # (the last steps of a short run lower the order: call the update itself)
            o.model_outputs = o.model_outputs[1:] + [eps(rho[i])]
            got_o = o.second_order_update(x) if order == 2 else o.third_order_update(x)
        else:
            o.solver_order = order
            got_o = o.step(eps(rho[i]), x)
            assert o.orders == [order]
        assert np.abs(got_o - want).max() <= 1e-12 * np.abs(want).max(), i


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("n", [4, 8, 20])
def test_scheduler_scalars_equal_the_oracle_step(n, order, pred):
    """the collapsed coefficients (three shared antiderivatives) against the list-based ind_fn form on random fp64 tensors, every step of a free-running trajectory"""
    kw = dict(SD15_DEIS_KWARGS, solver_order=order, prediction_type=pred)
    s, o = DEISMultistepScheduler(**kw), DEISOracle(**kw)
    s.set_timesteps(n), o.set_timesteps(n)
    rng = np.random.default_rng(n + order)
    x, hist = rng.standard_normal((2, 4, 5)), []
    for i in range(n):
        e = rng.standard_normal(x.shape)
        want = o.step(e, x)
        conv_x, conv_e, cx, cs = s.step_scalars(i)
        assert len(cs) == o.orders[-1]
        m0 = conv_x * x + conv_e * e
        got = cx * x + sum(c * m for c, m in zip(cs, [m0] + hist))
        hist = [m0] + hist
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), i
        x = want


def test_v_prediction_conversion():
    s = sched(8, prediction_type="v_prediction")
    rho = s._sigmas.astype(np.float64)
    for i in range(8):
        conv_x, conv_e, _, _ = s.step_scalars(i)
        a = alpha(rho[i])
        assert abs(conv_x - rho[i] * a) <= 1e-15 and abs(conv_e - a) <= 1e-15   # m = sigma_s x + alpha_s v
    o = DEISOracle(**dict(SD15_DEIS_KWARGS, prediction_type="v_prediction"))
    o.set_timesteps(8)
    x, v = np.array([0.3, -1.0]), np.array([2.0, 0.5])
    assert np.allclose(o.convert_model_output(v, x), rho[0] * alpha(rho[0]) * x + alpha(rho[0]) * v, rtol=1e-15)


def test_refusals():
    for kw in (dict(prediction_type="sample"), dict(thresholding=True), dict(use_karras_sigmas=True), dict(algorithm_type="dpmsolver++"),
               dict(solver_type="midpoint"), dict(solver_order=4)):
        with pytest.raises(NotImplementedError):
            DEISMultistepScheduler(**dict(SD15_DEIS_KWARGS, **kw))
    for kw in (dict(prediction_type="noise"), dict(timestep_spacing="even")):
        with pytest.raises(ValueError):
            DEISMultistepScheduler(**dict(SD15_DEIS_KWARGS, **kw))
    s = DEISMultistepScheduler(**SD15_DEIS_KWARGS)
    with pytest.raises(ValueError):
        s.step_scalars(0)                                                         # before set_timesteps
    s.set_timesteps(8)
    with pytest.raises(ValueError):
        s.step_scalars(0, 2)                                                      # no history for a second-order first step
    with pytest.raises(ValueError):
        s.set_timesteps(0)
