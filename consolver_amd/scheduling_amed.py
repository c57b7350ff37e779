"""AMEDSolverScheduler -- the AMED-plugin form of DPM-Solver++ (Zhou et al. 2024, AMED-Solver), HIP-backed.

The scheduler the reference builds for ``type == "amed"`` (gen_ppo.py:157-163, 289-306): its vendored subclass of diffusers'
DPMSolverMultistepScheduler (diffusers_amed_plugin_dpmpp.py) with a learned table per step count -- the timesteps, a
"gradient scale" per step that multiplies the direction terms of the update, and a "time scale" per step that moves the
timestep the MODEL sees at odd positions:

    scheduler.scale_dirs, scheduler.scale_times = grad_scale, time_scale
    pipeline(..., num_inference_steps=n, timesteps=table)

What the plugin decides is restated here on the parent's kernel (cs_dpm_multistep_step): the update is linear in the same
five scalars, the gradient scale multiplies ``c0`` and ``c1``.  The learned tables are the reference's and are NOT part of
this package: pass them in (``set_schedule``, ``load_schedules``; ``generate --amed-schedule FILE.json``).
tests/golden/amed_solver.npz pins the timesteps, the sigmas and every step's result to the plugin's own output.
"""
import json

import numpy as np
import torch

from .scheduling_dpm import DPMSolverMultistepScheduler

# what gen_ppo.py:160-163 resolves to on SD1.5's scheduler_config.json: the class defaults (dpmsolver++, midpoint, order 2, final_sigmas_type "zero") on SD1.5's betas
SD15_AMED_KWARGS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1)


class AMEDSolverScheduler(DPMSolverMultistepScheduler):
    """``set_timesteps(timesteps=table)`` with ``scale_dirs`` / ``scale_times`` set is the plugin's entry point; ``set_schedule`` stores a table so
    that ``set_timesteps(n, device)`` (what SDSamplingEngine calls) finds it by its step count.  With neither it is the parent class."""

    _amed = False                                     # the current grid is a table's (else the parent's)

    @property
    def _tables(self):
        """n -> (timesteps [n + 1], scale_dirs, scale_times); not part of the config (the constructor is the parent's)"""
        return self.__dict__.setdefault("_amed_tables", {})

    def set_schedule(self, timesteps, scale_dirs, scale_times):
        """store the table of ``len(timesteps) - 1`` steps"""
        ts, dirs, times = self._checked(timesteps, scale_dirs, scale_times)
        self._tables[len(ts) - 1] = (ts, dirs, times)

    def load_schedules(self, path):
        """a JSON file {"<n>": {"amed": [...], "grad_scale": [...], "time_scale": [...]}, ...} (the layout of tests/golden/amed_schedules.json)"""
        with open(path, "r", encoding="utf-8") as f:
            tables = json.load(f)
        for n, t in tables.items():
            for k in ("amed", "grad_scale", "time_scale"):
                if k not in t:
                    raise ValueError(f"{path}: the table of {n} steps has no {k!r}")
            if len(t["amed"]) - 1 != int(n):
                raise ValueError(f"{path}: the table filed under {n} steps has {len(t['amed']) - 1}")
            self.set_schedule(t["amed"], t["grad_scale"], t["time_scale"])
        return self

    def _checked(self, timesteps, scale_dirs, scale_times):
        T = self.config.num_train_timesteps
        if scale_dirs is None or scale_times is None:
            raise ValueError("scale_dirs and scale_times must be set before set_timesteps(timesteps=...)")
        ts = np.asarray(timesteps)
        if ts.ndim != 1 or len(ts) < 2 or not np.array_equal(ts, ts.astype(np.int64)):
            raise ValueError("the AMED timesteps are at least two integers: the model timesteps and the final one")
        ts = ts.astype(np.int64)
        if ts.min() < 0 or ts.max() >= T or np.any(np.diff(ts) >= 0):
            raise ValueError(f"the AMED timesteps must decrease inside [0, {T})")
        n = len(ts) - 1
        if len(scale_dirs) < n or len(scale_times) < n or len(scale_times) > n + 1:
            raise ValueError(f"{n} steps need {n} (or {n + 1}) scale_dirs and scale_times, got {len(scale_dirs)} and {len(scale_times)}")
        return ts, [float(v) for v in scale_dirs], [float(v) for v in scale_times]

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        if timesteps is None:
            if num_inference_steps is None:
                raise ValueError("set_timesteps needs num_inference_steps or timesteps")
            if not self._tables:                      # the plugin calls super() here
                self._amed = False
                return super().set_timesteps(num_inference_steps, device)
            if int(num_inference_steps) not in self._tables:
                raise ValueError(f"no AMED table of {num_inference_steps} steps is stored (stored: {sorted(self._tables)})")
            ts, dirs, times = self._tables[int(num_inference_steps)]
        else:
            ts, dirs, times = self._checked(timesteps, getattr(self, "scale_dirs", None), getattr(self, "scale_times", None))
        self.scale_dirs, self.scale_times = dirs, times
        n = len(ts) - 1
        # plugin lines 50-59, in its fp32: the sigmas are integer lookups (the last one is the sigma of the final timestep, not zero); the model timestep of an odd
        # position is the one whose sigma is nearest to scale_time x sigma, searched strictly between its neighbours
        all_sigmas = np.sqrt((1.0 - self._ac) / self._ac).astype(np.float32)
        sig = all_sigmas[ts]
        model_ts = ts[:-1].copy()
        for i in range(1, min(len(times), n), 2):
            target = np.float32(sig[i] * np.float32(times[i]))
            source = all_sigmas[ts[i + 1] + 1:ts[i - 1]]
            if len(source) == 0:
                raise ValueError(f"no timestep lies strictly between the AMED timesteps {ts[i + 1]} and {ts[i - 1]}")
            model_ts[i] = ts[i + 1] + 1 + int(np.argmin(np.abs(source - target)))
        self._sigmas = sig.astype(np.float32)
        self.sigmas = torch.from_numpy(self._sigmas)
        self.num_inference_steps = n
        self._timesteps = model_ts
        key = ("amed", tuple(model_ts.tolist()), None if device is None else str(torch.device(device)))
        if self._grid_key != key or device is None:
            self.timesteps = torch.from_numpy(model_ts).to(device)
            self._grid_key = key
        self._step_index = None
        self._lower_order_nums = 0
        self._m = []
        self._amed = True

    def step_scalars(self, i, first_order=None):
        """the parent's scalars with the direction terms times ``scale_dirs[i]`` (plugin lines 121, 205-209, 417); ``cx`` and the conversion are untouched"""
        conv_x, conv_e, cx, c0, c1 = super().step_scalars(i, first_order)
        if self._amed:
            g = self.scale_dirs[i]
            c0, c1 = g * c0, g * c1
        return conv_x, conv_e, cx, c0, c1
