"""CPU tests of iPNDM: the host scalars of consolver_amd/scheduling_pndm.py and the independent list-based restatement tests/pndm_oracle.py against the DDIM
transfer, against the defining property of the Adams-Bashforth weights, and against each other."""
import numpy as np
import pytest

from consolver_amd import SD15_PNDM_KWARGS, PNDMScheduler
from consolver_amd.scheduling_pndm import PLMS_WEIGHTS
from oracle import solver_oracle as so
from tests.pndm_oracle import PNDMOracle, ddim_transfer

TABLES = {8: [876, 751, 751, 626, 501, 376, 251, 126, 1], 4: [751, 501, 501, 251, 1]}
AC = so.alphas_cumprod(so.make_betas("scaled_linear", 0.00085, 0.012)).astype(np.float64)


def pair(n, **kw):
    kw = dict(SD15_PNDM_KWARGS, **kw)
    s, o = PNDMScheduler(**kw), PNDMOracle(**kw)
    s.set_timesteps(n), o.set_timesteps(n)
    return s, o


@pytest.mark.parametrize("n", [4, 8])
def test_timestep_tables(n):
    s, o = pair(n)
    assert s.timesteps.tolist() == TABLES[n] == o.timesteps.tolist() and len(s.timesteps) == n + 1 and s.num_inference_steps == n
    assert s.config.skip_prk_steps and not s.config.set_alpha_to_one and s.config.steps_offset == 1
    assert s.config.timestep_spacing == "leading" and s.config.prediction_type == "epsilon" and s.factor_net is None


def test_transfer_is_the_ddim_transfer():
    """the transfer formula of _get_prev_sample against (x - sqrt(1 - a_t) eps) / sqrt(a_t) moved to a_p, on random vectors, 1e-13; and the first forward's scalars"""
    rng = np.random.default_rng(0)
    _, o = pair(8)
    for t in (876, 751, 126, 1):
        x, e = rng.standard_normal((2, 64))
        p = t - 125
        want = ddim_transfer(x, e, AC[t], AC[p] if p >= 0 else AC[0])
        assert np.abs(o.get_prev_sample(x, t, p, e) - want).max() <= 1e-13
    s, _ = pair(8)
    cx, cs, restart = s.step_scalars(0)
    x, e = rng.standard_normal((2, 64))
    assert not restart and len(cs) == 1 and np.abs(cx * x + cs[0] * e - ddim_transfer(x, e, AC[876], AC[751])).max() <= 1e-13


def test_weight_sets():
    """each set sums to 1, and the m-term set integrates polynomials of degree < m in the step index exactly over one step: sum_j w_j (-j)^d = 1 / (d + 1)"""
    for m, w in PLMS_WEIGHTS.items():
        assert len(w) == m and abs(sum(w) - 1) <= 1e-15
        for d in range(m):
            assert abs(sum(wj * (-j) ** d for j, wj in enumerate(w)) - 1.0 / (d + 1)) <= 1e-14, (m, d)
    # ... and so do the scheduler's coefficients: their sum is the plain transfer's, at every forward (the mean of two at forward 1 included)
    s, _ = pair(8)
    for k in range(9):
        t, p = (876, 751) if k == 1 else (TABLES[8][k], TABLES[8][k] - 125)
        a_t, a_p = AC[t], AC[p] if p >= 0 else AC[0]
        K = -(a_p - a_t) / (a_t * np.sqrt(1 - a_p) + np.sqrt(a_t * (1 - a_t) * a_p))
        cx, cs, _ = s.step_scalars(k)
        assert len(cs) == (2 if k == 1 else min(max(k, 1), 4)) and abs(sum(cs) / K - 1) <= 1e-14 and abs(cx / np.sqrt(a_p / a_t) - 1) <= 1e-15


def test_second_forward_restarts_from_the_saved_sample():
    rng = np.random.default_rng(1)
    s, o = pair(8)
    x0, e0, e1 = rng.standard_normal((3, 32))
    x1 = o.step(e0, x0)
    assert len(o.ets) == 1 and np.array_equal(o.cur_sample, x0)
    x2 = o.step(e1, x1 + 100.0)                                                   # the sample handed in is not used
    assert len(o.ets) == 1 and np.array_equal(o.ets[0], e0)                       # ... and the output is not appended
    assert np.abs(x2 - ddim_transfer(x0, (e0 + e1) / 2, AC[876], AC[751])).max() <= 1e-13
    cx, cs, restart = s.step_scalars(1)
    assert restart and len(cs) == 2 and cs[0] == cs[1]
    assert np.abs(cx * x0 + cs[0] * e1 + cs[1] * e0 - x2).max() <= 1e-13
    assert [s.step_scalars(k)[2] for k in range(9)] == [k == 1 for k in range(9)]
    e2 = rng.standard_normal(32)
    o.step(e2, x2)
    assert len(o.ets) == 2 and np.array_equal(o.ets[0], e0) and np.array_equal(o.ets[1], e2)


@pytest.mark.parametrize("n", [4, 8])
def test_constant_model_output(n):
    """with a constant eps the improved-Euler forward repeats the first result, and every combination is eps itself: each later step is the plain transfer"""
    rng = np.random.default_rng(2)
    _, o = pair(n)
    x, e = rng.standard_normal((2, 32))
    xs = [x]
    for _ in range(n + 1):
        xs.append(o.step(e, xs[-1]))
    assert np.abs(xs[2] - xs[1]).max() <= 1e-15
    r = 1000 // n
    for k in range(2, n + 1):
        t = TABLES[n][k]
        want = ddim_transfer(xs[k], e, AC[t], AC[t - r] if t - r >= 0 else AC[0])
        assert np.abs(xs[k + 1] - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), k


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("n", [4, 8])
def test_host_scalars_equal_the_oracle_step(n, pred):
    """the collapsed coefficients against the list-based step_plms on random fp64 tensors, all n + 1 forwards of a free-running trajectory"""
    s, o = pair(n, prediction_type=pred)
    rng = np.random.default_rng(n)
    x, ets, cur = rng.standard_normal((2, 4, 5)), [], None
    for k in range(n + 1):
        e = rng.standard_normal(x.shape)
        want = o.step(e, x)
        cx, cs, restart = s.step_scalars(k)
        if k == 0:
            cur = x
        hist = ets[::-1][:1] if restart else ets[::-1][:3]
        assert len(cs) == len(hist) + 1
        got = cx * (cur if restart else x) + sum(c * m for c, m in zip(cs, [e] + hist))
        if not restart:
            ets = ets[-3:] + [e]
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), k
        x = want
    assert len(o.ets) == min(n, 4) and o.counter == n + 1


def test_last_forward_uses_the_first_alpha():
    s, o = pair(8)
    rng = np.random.default_rng(3)
    x, e = rng.standard_normal((2, 16))
    assert np.abs(o.get_prev_sample(x, 1, 1 - 125, e) - ddim_transfer(x, e, AC[1], AC[0])).max() <= 1e-13
    cx, cs, _ = s.step_scalars(8)
    assert abs(cx / np.sqrt(AC[0] / AC[1]) - 1) <= 1e-15
    s1, o1 = pair(8, set_alpha_to_one=True)
    assert abs(s1.step_scalars(8)[0] / np.sqrt(1.0 / AC[1]) - 1) <= 1e-15
    assert np.abs(o1.get_prev_sample(x, 1, -124, e) - ddim_transfer(x, e, AC[1], 1.0)).max() <= 1e-13


def reads_and_writes(n, slots):
    """(forward, slot written, slots read) of SDSamplingEngine's ring: forward i writes slot i % slots; the history is the scheduler's rule"""
    ets, out = [], []
    for i in range(n + 1):
        read = ets[::-1][:1] if i == 1 else ets[::-1][:3]
        out.append((i, i % slots, [j % slots for j in read]))
        if i != 1:
            ets = ets[-3:] + [i]
    return out


def test_ring_slots():
    """history_slots = 5: the slot a forward writes is never one it reads; four are too few (forward 4 would write the slot of forward 0, which it reads)"""
    assert PNDMScheduler.history_slots == 5
    for n in range(2, 21):
        assert all(w not in r for _, w, r in reads_and_writes(n, 5)), n
    assert [i for i, w, r in reads_and_writes(8, 4) if w in r] == [4]


def test_refusals():
    with pytest.raises(NotImplementedError):
        PNDMScheduler(**dict(SD15_PNDM_KWARGS, skip_prk_steps=False))
    with pytest.raises(NotImplementedError):
        PNDMScheduler()                                                           # the class default is the Runge-Kutta warm-up
    with pytest.raises(ValueError):
        PNDMScheduler(**dict(SD15_PNDM_KWARGS, prediction_type="sample"))
    s = PNDMScheduler(**SD15_PNDM_KWARGS)
    with pytest.raises(ValueError):
        s.step_scalars(0)
    with pytest.raises(ValueError):
        s.set_timesteps(1001)
