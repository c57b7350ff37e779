"""Writes tests/golden/amed_schedules.json and tests/golden/amed_solver.npz: the reference's AMED tables and its AMED plugin
(diffusers_amed_plugin_dpmpp.py) run step by step on the CPU.

Build container only: the reference tree is read where it lies; nothing of it is copied, only the tables (settings) and the arrays
it computes are stored.

    python tools/make_amed_golden.py

``amed_schedules.json``: the ``SCHEDULES`` literal of the reference's gen_ppo.py (lines 24-52), parsed with ``ast`` -- that file imports
diffusers, accelerate and a COCO path at module level and cannot be imported.  {"<n>": {"amed": [...], "grad_scale": [...], "time_scale": [...]}}.

``amed_solver.npz``: for n = 4 and n = 8, ``n{n}_timesteps`` [n] (the model timesteps after the time-scale search), ``n{n}_sigmas`` [n + 1] and
per step i ``n{n}_s{i}_x`` (the sample passed in), ``n{n}_s{i}_eps`` (the model output) and ``n{n}_s{i}_prev`` (the returned ``prev_sample``),
fp32, shape [3, 5, 67] (as tests/golden/flux_fm_baselines.npz).  The model output is the closed form of tools/make_fm_baseline_golden.py
and is stored, not recomputed by the tests.

The plugin subclasses diffusers' DPMSolverMultistepScheduler, which is not installed.  ``oracle/ref_stubs.install("sd")`` provides the
diffusers names the reference's own schedulers import; the three more the plugin imports are added here.  The base class is this tool's
adapter: the few members the plugin's ``set_timesteps`` / ``step`` use and do not override (diffusers 0.26.3's, from memory: the x0
conversion of ``dpmsolver++`` with epsilon prediction, alpha = 1 / sqrt(sigma^2 + 1)); the beta table is the one the reference's own
PPOScheduler computes for SD1.5.  Every update formula, the timestep search, the lower-order rule and the scale factors are the plugin's.
"""
import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPE = (3, 5, 67)
STEPS = (4, 8)


def model_output(x, t, noise):
    return (0.9 * np.tanh(x) + 1e-5 * float(t) + 0.05 * noise).astype(np.float32)


def read_schedules(ref_root):
    with open(os.path.join(ref_root, "gen_ppo.py"), "r", encoding="utf-8") as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "SCHEDULES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise RuntimeError("gen_ppo.py has no SCHEDULES literal")


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_stubs
    ref_stubs.install("sd")
    import torch
    torch.set_num_threads(1)
    torch.set_grad_enabled(False)

    schedules = read_schedules(ref_stubs.REF_ROOT)
    for n, t in schedules.items():
        assert set(t) == {"amed", "grad_scale", "time_scale"} and len(t["amed"]) == n + 1 == len(t["grad_scale"]) == len(t["time_scale"])
    path = os.path.join(GOLDEN, "amed_schedules.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump({str(n): schedules[n] for n in sorted(schedules)}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")

    with ref_stubs.quiet():
        from scheduler_ppo import PPOScheduler
        ac = PPOScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                          factor_net_kwargs=dict(num_actions=3, hidden_dim=4)).alphas_cumprod.clone()

    class BaseAdapter:
        """stands in for diffusers.DPMSolverMultistepScheduler: what the plugin inherits and does not override"""
        def __init__(self):
            self.alphas_cumprod = ac
            self.config = types.SimpleNamespace(solver_order=2, algorithm_type="dpmsolver++", solver_type="midpoint", prediction_type="epsilon",
                                                lower_order_final=True, euler_at_final=False, final_sigmas_type="zero")
            self.num_inference_steps = None
            self._step_index = None

        @property
        def step_index(self):
            return self._step_index

        def _init_step_index(self, timestep):
            idx = (self.timesteps == timestep).nonzero()
            self._step_index = (idx[1] if len(idx) > 1 else idx[0]).item()

        def _sigma_to_alpha_sigma_t(self, sigma):
            alpha_t = 1 / ((sigma ** 2 + 1) ** 0.5)
            return alpha_t, sigma * alpha_t

        def convert_model_output(self, model_output, sample=None):
            alpha_t, sigma_t = self._sigma_to_alpha_sigma_t(self.sigmas[self.step_index])
            return (sample - sigma_t * model_output) / alpha_t

    d = sys.modules["diffusers"]
    d.DPMSolverMultistepScheduler = BaseAdapter
    sys.modules["diffusers.utils"].deprecate = lambda *a, **k: None
    tu = types.ModuleType("diffusers.utils.torch_utils")
    tu.randn_tensor = None                            # (the SDE variants' noise: not reached)
    sys.modules["diffusers.utils.torch_utils"] = tu
    sys.modules["diffusers.utils"].torch_utils = tu
    from diffusers_amed_plugin_dpmpp import DPMSolverMultistepScheduler as AMEDPlugin

    fx = {"shape": np.asarray(SHAPE, np.int64), "steps": np.asarray(STEPS, np.int64)}
    for n in STEPS:
        t = schedules[n]
        s = AMEDPlugin()
        s.scale_dirs, s.scale_times = t["grad_scale"], t["time_scale"]
        s.set_timesteps(num_inference_steps=n, timesteps=t["amed"])
        assert len(s.timesteps) == n and len(s.sigmas) == n + 1
        fx[f"n{n}_timesteps"], fx[f"n{n}_sigmas"] = s.timesteps.numpy().astype(np.int64), s.sigmas.numpy().astype(np.float32)
        rng = np.random.default_rng(8000 + n)
        x = torch.from_numpy(rng.standard_normal(SHAPE).astype(np.float32))
        for i, ts in enumerate(s.timesteps):
            e = torch.from_numpy(model_output(x.numpy(), float(ts), rng.standard_normal(SHAPE).astype(np.float32)))
            prev = s.step(e, ts, x, return_dict=False)[0]
            assert prev.dtype == torch.float32 and s.step_index == i + 1
            fx[f"n{n}_s{i}_x"], fx[f"n{n}_s{i}_eps"], fx[f"n{n}_s{i}_prev"] = x.numpy().copy(), e.numpy().copy(), prev.numpy().copy()
            x = prev
    path = os.path.join(GOLDEN, "amed_solver.npz")
    np.savez_compressed(path, **fx)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
