"""Host side of the Multistep DPM-Solver scheduler (no GPU): grids, sigma tables and the five per-step scalars of
consolver_amd/scheduling_dpm.py against tests/dpm_oracle.py, and the oracle itself against two anchors that do not rest on
a restatement from memory: the golden-pinned DDIM of oracle/solver_oracle.py and the order of convergence."""
import numpy as np
import pytest

from consolver_amd.scheduling_dpm import DPMSolverMultistepScheduler, SD15_MULTISTEP_DPM_KWARGS
from oracle import solver_oracle as so
from tests.dpm_oracle import COMBOS, DPMSolverOracle, combo_id, run

SD15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def eps_model(x, t):
    return 0.9 * np.tanh(x) + 1e-5 * t


def test_integer_grids_are_exact():
    def grid(n, **kw):
        for cls in (DPMSolverMultistepScheduler, DPMSolverOracle):
            s = cls(**SD15, **kw)
            s.set_timesteps(n)
            yield np.asarray(s.timesteps).tolist()
    for g in grid(40, algorithm_type="dpmsolver", final_sigmas_type="sigma_min"):
        assert len(g) == 40 and g[:4] == [999, 974, 949, 924] and g[-3:] == [75, 50, 25]
    for g in grid(8):
        assert g == [999, 874, 749, 624, 500, 375, 250, 125]
    for g in grid(8, timestep_spacing="leading", steps_offset=1):
        assert g == [889, 778, 667, 556, 445, 334, 223, 112]
    for g in grid(8, timestep_spacing="trailing"):
        assert g == [999, 874, 749, 624, 499, 374, 249, 124]
    s = DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS)
    s.set_timesteps(40)
    assert s.timesteps.dtype.is_floating_point is False and s.timesteps.tolist()[:2] == [999, 974]      # the reference call sites: linspace (class default)


def test_sigma_tables():
    want = [14.614653, 7.2973566, 4.0817323, 2.4925318, 1.6182793, 1.0724864, 0.69579905, 0.39998198, 0.02916753]
    for cls in (DPMSolverMultistepScheduler, DPMSolverOracle):
        s = cls(**SD15, final_sigmas_type="sigma_min")
        s.set_timesteps(8)
        sig = np.asarray(s.sigmas, np.float64)
        assert sig.shape == (9,)
        np.testing.assert_allclose(sig, want, rtol=1e-6)
        z = cls(**SD15, final_sigmas_type="zero")
        z.set_timesteps(8)
        zs = np.asarray(z.sigmas, np.float64)
        assert zs.shape == (9,) and zs[-1] == 0.0
        np.testing.assert_allclose(zs[:-1], want[:-1], rtol=1e-6)
    s = DPMSolverMultistepScheduler(**SD15, final_sigmas_type="sigma_min")
    s.set_timesteps(8)
    assert str(s.sigmas.dtype) == "torch.float32"


def test_oracle_order_one_dpmsolver_is_the_golden_pinned_ddim():
    """anchor 1: dpmsolver, order 1, trailing, sigma_min is eta = 0 DDIM with prev_t = t - T // n (the final step lands on alphas_cumprod[0])."""
    n = 8
    x = np.random.default_rng(0).standard_normal((2, 4, 8, 8))
    o = DPMSolverOracle(**SD15, algorithm_type="dpmsolver", solver_order=1, timestep_spacing="trailing", final_sigmas_type="sigma_min")
    xs = run(o, eps_model, x, n)
    ac = so.alphas_cumprod(so.make_betas("scaled_linear", 0.00085, 0.012)).astype(np.float64)
    assert o.timesteps.tolist() == so.sd_timesteps(n, spacing="trailing").tolist()
    xd = x
    worst = 0.0
    for i, t in enumerate(so.sd_timesteps(n, spacing="trailing")):
        pt = so.sd_prev_timestep(int(t), n)
        xd = so.ddim_update(xd, eps_model(xd, int(t)), ac[int(t)], ac[pt] if pt >= 0 else ac[0])
        worst = max(worst, rel_l2(xs[i], xd))
    print("dpm order-1 oracle vs DDIM oracle: worst rel-L2 over the trajectory", worst)
    assert worst <= 1e-6, worst


@pytest.fixture(scope="module")
def convergence_reference():
    x = np.random.default_rng(1).standard_normal((2, 4, 8, 8))
    o = DPMSolverOracle(**SD15, algorithm_type="dpmsolver", solver_order=2, timestep_spacing="trailing", final_sigmas_type="sigma_min")
    return x, run(o, eps_model, x, 999)[-1]


@pytest.mark.parametrize("alg,order", [("dpmsolver", 1), ("dpmsolver++", 1), ("dpmsolver", 2), ("dpmsolver++", 2)])
def test_oracle_order_of_convergence(convergence_reference, alg, order):
    """anchor 2: against the 999-step order-2 run, halving the step divides the error by ~2 at order 1 and by >= 3 at order 2
    (a wrong D1 coefficient or r0 makes the method first order)."""
    x, ref = convergence_reference
    errs = []
    for n in (10, 20, 40, 80):
        o = DPMSolverOracle(**SD15, algorithm_type=alg, solver_order=order, timestep_spacing="trailing", final_sigmas_type="sigma_min")
        errs.append(rel_l2(run(o, eps_model, x, n)[-1], ref))
    ratios = [errs[i] / errs[i + 1] for i in range(3)]
    print(alg, "order", order, "errors", errs, "ratios", ratios)
    for r in ratios:
        if order == 1:
            assert 1.8 <= r <= 2.2, ratios
        else:
            assert r >= 3.0, ratios


@pytest.mark.parametrize("n", [5, 16])
@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_host_scalars_reproduce_the_oracle_step(combo, n):
    """the five fp32 scalars the kernel gets, applied in numpy fp64 (m0 = conv_x x + conv_e eps; x' = cx x + c0 m0 + c1 m1), give the oracle's step at every
    step: first-order first step, first-order last step at n = 5, second-order last step at n = 16 under sigma_min."""
    rng = np.random.default_rng(n)
    s = DPMSolverMultistepScheduler(**SD15, **combo)
    o = DPMSolverOracle(**SD15, **combo)
    s.set_timesteps(n); o.set_timesteps(n)
    assert s.timesteps.tolist() == o.timesteps.tolist()
    x = rng.standard_normal((2, 3, 5, 7))
    m1 = None
    for i in range(n):
        eps = rng.standard_normal(x.shape)
        conv_x, conv_e, cx, c0, c1 = [np.float64(np.float32(v)) for v in s.step_scalars(i)]
        m0 = conv_x * x + conv_e * eps
        first = combo["solver_order"] == 1 or i == 0 or (i == n - 1 and (n < 15 or combo["final_sigmas_type"] == "zero"))
        assert (c1 == 0.0) == first, (i, c1)
        got = cx * x + c0 * m0 + (c1 * m1 if not first else 0.0)
        want = o.step(eps, x)
        assert rel_l2(m0, o.last_converted()) < 1e-6, i
        assert rel_l2(got, want) < 1e-6, (i, rel_l2(got, want))
        x, m1 = want, m0
    if n == 16 and combo["solver_order"] == 2 and combo["final_sigmas_type"] == "sigma_min":
        assert s.step_scalars(n - 1)[4] != 0.0                                  # the last step is second order


@pytest.mark.parametrize("kw", [dict(solver_order=3), dict(thresholding=True), dict(use_karras_sigmas=True), dict(use_lu_lambdas=True),
                                dict(use_exponential_sigmas=True), dict(algorithm_type="sde-dpmsolver"), dict(algorithm_type="sde-dpmsolver++"),
                                dict(variance_type="learned"), dict(algorithm_type="dpmsolver", final_sigmas_type="zero")],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_refused_constructor_arguments_raise(kw):
    with pytest.raises((NotImplementedError, ValueError)):
        DPMSolverMultistepScheduler(**kw)


def test_protocol_surface_without_a_gpu():
    import torch
    s = DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS)
    assert s.order == 1 and s.init_noise_sigma == 1.0 and s.config.algorithm_type == "dpmsolver" and s.config.get("solver_order") == 2
    assert s.config.timestep_spacing == "linspace" and s.config.steps_offset == 1 and s.config.get("missing", 7) == 7
    x = torch.zeros(1, 4, 8, 8)
    assert s.scale_model_input(x, 10) is x
    with pytest.raises(ValueError):
        s.step(x, 999, x)                                                      # before set_timesteps
    t = DPMSolverMultistepScheduler.from_config(s.config, algorithm_type="dpmsolver++", final_sigmas_type="zero")      # from_pretrained-style override
    assert t.config.algorithm_type == "dpmsolver++" and t.config.beta_schedule == "scaled_linear"
    import consolver_amd
    assert consolver_amd.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
