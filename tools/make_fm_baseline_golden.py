"""Writes tests/golden/flux_fm_baselines.npz: the reference's FlowMatchGeneralDiscreteScheduler (edit_ppo/scheduler_fm.py), run step by
step on the CPU, for 4 types x {fp32, bf16} x n in {4, 5}.

Build container only: the reference tree is imported read-only through ``oracle/ref_stubs.py`` (stand-ins for the diffusers names it
imports); nothing of it is copied, only the arrays it computes are stored.

    python tools/make_fm_baseline_golden.py

Per case ``{type}_{f32|bf16}_n{n}``: ``_sigmas`` [n + 1], ``_timesteps`` [n] of the run's schedule (``sigmas = linspace(1, 1/n, n)``,
``mu = 1.15``, dynamic shifting) and per step i ``_s{i}_x`` (the sample passed in), ``_s{i}_v`` (the model output) and ``_s{i}_prev``
(the returned ``prev_sample``); bf16 values are stored as fp32.  One shape, [3, 5, 67]: 335 elements per sample, 1005 in all, so the 8-wide
and the 4-wide vector bodies and both scalar tails run.  The model output is a closed form of the sample, the timestep and seeded noise
(as in the rollout fixtures of oracle/make_golden.py) and is stored, not recomputed by the tests.  n = 5 ends on a first stage for Heun and
dpm-solver, which takes the ``idx + 2`` clamp of scheduler_fm.py:417.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "flux_fm_baselines.npz")
TYPES = ("euler", "heun", "dpm-solver", "dpm-solver-multistep")
SHAPE = (3, 5, 67)


def model_output(x, t, noise):
    return (0.9 * np.tanh(x) + 1e-5 * float(t) + 0.05 * noise).astype(np.float32)


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_stubs
    ref_stubs.install("flux")
    import torch
    torch.set_num_threads(1)
    torch.set_grad_enabled(False)
    with ref_stubs.quiet():
        from scheduler_fm import FlowMatchGeneralDiscreteScheduler
    fx = {"types": np.asarray(TYPES), "shape": np.asarray(SHAPE, np.int64)}
    for ti, typ in enumerate(TYPES):
        for dt in ("f32", "bf16"):
            tdt = torch.bfloat16 if dt == "bf16" else torch.float32
            for n in (4, 5):
                key = f"{typ}_{dt}_n{n}"
                s = FlowMatchGeneralDiscreteScheduler(shift=3.0, use_dynamic_shifting=True, type=typ)
                s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=1.15)
                s.set_begin_index(0)
                fx[f"{key}_sigmas"], fx[f"{key}_timesteps"] = s.sigmas.numpy().copy(), s.timesteps.numpy().copy()
                rng = np.random.default_rng(7000 + 100 * ti + 10 * (dt == "bf16") + n)
                x = torch.from_numpy(rng.standard_normal(SHAPE).astype(np.float32)).to(tdt)
                for i, t in enumerate(s.timesteps):
                    v = torch.from_numpy(model_output(x.float().numpy(), float(t), rng.standard_normal(SHAPE).astype(np.float32))).to(tdt)
                    prev = s.step(v, t, x, return_dict=False)[0]
                    assert prev.dtype == tdt and s.step_index == i + 1
                    fx[f"{key}_s{i}_x"], fx[f"{key}_s{i}_v"], fx[f"{key}_s{i}_prev"] = x.float().numpy().copy(), v.float().numpy().copy(), prev.float().numpy().copy()
                    x = prev
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
