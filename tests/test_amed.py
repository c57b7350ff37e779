"""CPU tests of AMEDSolverScheduler against tests/golden/amed_solver.npz (the reference's AMED plugin run on the CPU, tools/make_amed_golden.py) with the reference's
tables (tests/golden/amed_schedules.json), its errors, and the public surface of the two comparison solvers (make_scheduler, the argument parser)."""
import json
import os

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import AMEDSolverScheduler, SD15_AMED_KWARGS
from consolver_amd import generate as gen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCHEDULES = os.path.join(GOLDEN, "amed_schedules.json")


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def amed():
    with open(SCHEDULES, "r", encoding="utf-8") as f:
        return np.load(os.path.join(GOLDEN, "amed_solver.npz")), json.load(f)


def test_fixture_holds_settings_only(amed):
    _, tables = amed
    assert sorted(tables, key=int) == ["4", "6", "8", "10", "14"]
    for n, t in tables.items():
        assert sorted(t) == ["amed", "grad_scale", "time_scale"] and all(len(v) == int(n) + 1 for v in t.values())
        assert all(isinstance(v, int) for v in t["amed"]) and all(isinstance(v, float) for v in t["grad_scale"] + t["time_scale"])


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("entry", ["timesteps", "table"])
def test_grid_matches_the_plugin(amed, n, entry):
    """the model timesteps bit-exactly (the argmin search of the time scales, in the plugin's fp32), the sigmas to rtol 1e-6 (this package's alphas_cumprod is a
    sequential fp32 cumprod and differs from torch's in the last bit: 8.9e-7 at most on these entries)"""
    g, tables = amed
    t = tables[str(n)]
    s = AMEDSolverScheduler(**SD15_AMED_KWARGS)
    if entry == "timesteps":                                   # the plugin's entry point (gen_ppo.py:289-306)
        s.scale_dirs, s.scale_times = t["grad_scale"], t["time_scale"]
        s.set_timesteps(num_inference_steps=n, timesteps=t["amed"])
    else:                                                      # the engine's: a stored table found by its step count
        s.load_schedules(SCHEDULES)
        s.set_timesteps(n)
    assert s.timesteps.dtype == torch.int64 and np.array_equal(s.timesteps.numpy(), g[f"n{n}_timesteps"])
    assert not np.array_equal(s.timesteps.numpy(), np.asarray(t["amed"][:-1]))             # the odd positions moved
    assert np.array_equal(s.timesteps.numpy()[::2], np.asarray(t["amed"][:-1])[::2])
    np.testing.assert_allclose(s.sigmas.numpy(), g[f"n{n}_sigmas"], rtol=1e-6, atol=0)
    assert s.num_inference_steps == n and s.step_index is None and s.sigmas[-1] > 0


@pytest.mark.parametrize("n", [4, 8])
def test_scalars_reproduce_every_golden_step(amed, n):
    """step_scalars applied in numpy fp64 to the golden's own inputs: every ``prev`` < 1e-6 rel-L2 (the bound tests/test_fm_baselines.py holds its fp32 reference goldens
    to).  First step first order, middle steps second order, last step first order (final_sigmas_type "zero"); direction terms times grad_scale[i]."""
    g, tables = amed
    s = AMEDSolverScheduler(**SD15_AMED_KWARGS).load_schedules(SCHEDULES)
    s.set_timesteps(n)
    m_prev = None
    for i in range(n):
        x, e = g[f"n{n}_s{i}_x"].astype(np.float64), g[f"n{n}_s{i}_eps"].astype(np.float64)
        conv_x, conv_e, cx, c0, c1 = s.step_scalars(i)
        assert (c1 == 0.0) == (i == 0 or i == n - 1)
        m0 = conv_x * x + conv_e * e
        prev = cx * x + c0 * m0 + (c1 * m_prev if c1 != 0.0 else 0.0)
        err = rel_l2(prev, g[f"n{n}_s{i}_prev"])
        print("amed scalars vs plugin", n, i, err)
        assert err < 1e-6, (i, err)
        if i + 1 < n:
            assert np.array_equal(g[f"n{n}_s{i}_prev"], g[f"n{n}_s{i + 1}_x"])
        m_prev = m0
    # the scale is on the direction terms only
    p = consolver_amd.DPMSolverMultistepScheduler(**SD15_AMED_KWARGS)
    p.set_timesteps(n)
    p._sigmas = s._sigmas
    for i in range(n):
        a, b = s.step_scalars(i), p.step_scalars(i)
        k = tables[str(n)]["grad_scale"][i]
        assert a[:3] == b[:3] and a[3] == k * b[3] and a[4] == k * b[4]


def test_without_a_table_it_is_the_parent(amed):
    s, p = AMEDSolverScheduler(**SD15_AMED_KWARGS), consolver_amd.DPMSolverMultistepScheduler(**SD15_AMED_KWARGS)
    s.set_timesteps(6); p.set_timesteps(6)
    assert np.array_equal(s.timesteps.numpy(), p.timesteps.numpy()) and np.array_equal(s.sigmas.numpy(), p.sigmas.numpy())
    assert all(s.step_scalars(i) == p.step_scalars(i) for i in range(6))
    c = s.config
    assert (c.algorithm_type, c.solver_type, c.solver_order, c.final_sigmas_type) == ("dpmsolver++", "midpoint", 2, "zero")
    t = AMEDSolverScheduler.from_config(s.config)
    assert t.config.beta_schedule == "scaled_linear" and t.config.steps_offset == 1
    with pytest.raises(NotImplementedError):
        AMEDSolverScheduler(solver_order=3)


def test_value_errors(amed, tmp_path):
    _, tables = amed
    t = tables["4"]
    s = AMEDSolverScheduler(**SD15_AMED_KWARGS)
    with pytest.raises(ValueError):
        s.set_timesteps()                                                      # neither a step count nor timesteps
    with pytest.raises(ValueError):
        s.set_timesteps(timesteps=t["amed"])                                   # scale_dirs / scale_times not set
    s.scale_dirs = t["grad_scale"]
    with pytest.raises(ValueError):
        s.set_timesteps(timesteps=t["amed"])                                   # scale_times missing
    s.scale_times = t["time_scale"][:2]
    with pytest.raises(ValueError):
        s.set_timesteps(timesteps=t["amed"])                                   # mismatched lengths
    s.scale_times = t["time_scale"]
    for bad in ([999], [999, 500.5, 0], [0, 500, 999], [999, 1000, 0], [999, 500, 500, 0]):
        with pytest.raises(ValueError):
            s.set_timesteps(timesteps=bad)
    with pytest.raises(ValueError):
        s.set_schedule(t["amed"], t["grad_scale"][:3], t["time_scale"])
    s.set_schedule(t["amed"], t["grad_scale"], t["time_scale"])
    with pytest.raises(ValueError):
        s.set_timesteps(6)                                                     # no table of that length
    s.set_timesteps(4)
    for name, tab in (("nokey", {"4": {"amed": t["amed"], "grad_scale": t["grad_scale"]}}), ("count", {"5": t})):
        path = str(tmp_path / f"{name}.json")
        with open(path, "w") as f:
            json.dump(tab, f)
        with pytest.raises(ValueError):
            AMEDSolverScheduler(**SD15_AMED_KWARGS).load_schedules(path)


def test_make_scheduler_and_parser():
    assert gen.SOLVERS == ("consistencysolver", "multistep-dpmsolver", "ddim", "unipc", "amed")
    u = gen.make_scheduler("unipc")
    assert isinstance(u, consolver_amd.UniPCMultistepScheduler) and u.factor_net is None and u.history_slots == 3
    assert (u.config.steps_offset, u.config.beta_schedule, u.config.solver_type, u.config.solver_order) == (1, "scaled_linear", "bh2", 2)
    a = gen.make_scheduler("amed", amed_schedule=SCHEDULES)
    assert isinstance(a, AMEDSolverScheduler) and a.factor_net is None
    a.set_timesteps(8)
    assert a.timesteps.tolist()[0] == 999 and a.num_inference_steps == 8
    with pytest.raises(ValueError):
        gen.make_scheduler("amed")
    with pytest.raises(ValueError):
        gen.make_scheduler("deis")
    args = gen.parse_args(["--out", "o", "--solver", "unipc"])
    assert args.solver == "unipc" and args.amed_schedule is None
    args = gen.parse_args(["--out", "o", "--solver", "amed", "--amed-schedule", SCHEDULES])
    assert args.solver == "amed" and args.amed_schedule == SCHEDULES
    for bad in (["--solver", "amed"], ["--solver", "unipc", "--amed-schedule", SCHEDULES], ["--solver", "unipc", "--policy", "p.ckpt"],
                ["--solver", "unipc", "--use_conv"], ["--solver", "amed", "--amed-schedule", SCHEDULES, "--policy", "p.ckpt"],
                ["--solver", "amed", "--amed-schedule", SCHEDULES, "--use_conv"], ["--solver", "deis"]):
        with pytest.raises(SystemExit):
            gen.parse_args(["--out", "o"] + bad)
