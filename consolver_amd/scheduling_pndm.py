"""PNDMScheduler -- iPNDM: the pseudo linear multistep method (Liu et al. 2022) without its Runge-Kutta warm-up, HIP-backed.

The scheduler the reference builds for ``type == "ipndm"`` (gen_ppo.py:144-148):

    PNDMScheduler.from_pretrained(sd15, subfolder="scheduler")

which is the class SD1.5's ``scheduler_config.json`` was written for (``skip_prk_steps=True``, ``set_alpha_to_one=False``,
``steps_offset=1``; ``timestep_spacing="leading"`` and ``prediction_type="epsilon"`` are class defaults).  diffusers is not
installed and the reference does not vendor the class, so the timestep table with its repeated second entry, the branches of
``step_plms`` and the transfer formula are a restatement of diffusers 0.26.3 FROM MEMORY (DESIGN.md lists what rests on memory
and what anchors it): the transfer is algebraically the eta = 0 DDIM transfer, the weight sets are the Adams-Bashforth ones,
and tests/pndm_oracle.py restates the list-based algorithm independently (tests/test_pndm_oracle.py).

``set_timesteps(n)`` gives n + 1 timesteps, so a pipeline runs n + 1 forwards: the second one repeats the first transfer with
the mean of the two model outputs (improved Euler) from the saved first sample, and its output does not enter the history.
Every branch is linear in the sample and up to four model outputs, so all of it is host arithmetic (fp64, passed as fp32) and
the device work per step is ONE kernel (cs_linear_step).  The position in the trajectory is a host counter: the repeated
timestep makes a look-up by value ambiguous.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._scheduler_base import ConfigMixin, KARRAS_COMPATIBLES, SchedulerMixin, register_to_config
from .scheduling_deis import fill_lin_history
from .scheduling_dpm import SigmaGridMixin
from .scheduling_ppo import SolverOutput, fill_cfg, fill_io, result_tensor, step_inputs

# what the reference call site resolves to on SD1.5's scheduler_config.json (from memory, see the module docstring)
SD15_PNDM_KWARGS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, set_alpha_to_one=False,
                        steps_offset=1)

# Adams-Bashforth weights by the number of model outputs in the history, newest first
PLMS_WEIGHTS = {1: (1.0,), 2: (3.0 / 2.0, -1.0 / 2.0), 3: (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0), 4: (55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0)}


class PNDMScheduler(SigmaGridMixin, SchedulerMixin, ConfigMixin):
    _compatibles = list(KARRAS_COMPATIBLES)
    order = 1
    prev_sample_dtype = None      # as DPMSolverMultistepScheduler.prev_sample_dtype
    factor_net = None             # no policy (SDSamplingEngine probes it)
    # SDSamplingEngine writes forward i's combined eps to ring slot i % history_slots.  Forward 1's is dropped and forward 0's is kept, so forward 4
    # reads those of forwards 3, 2 and 0: with four slots it would write the slot of forward 0.  From forward 5 on the three read are the three before.
    history_slots = 5

    @register_to_config
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon", timestep_spacing="leading", steps_offset=0):
        if not skip_prk_steps:
            raise NotImplementedError("skip_prk_steps=False (the Runge-Kutta warm-up steps) is not implemented")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon` or `v_prediction`")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"{timestep_spacing} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        self._init_tables(beta_schedule, beta_start, beta_end, num_train_timesteps, trained_betas)
        self._final_ac = 1.0 if set_alpha_to_one else float(self._ac[0])
        self.final_alpha_cumprod = torch.tensor(self._final_ac)
        self.counter = 0
        self.ets = []                                 # model outputs (CFG-combined), oldest first; at most four
        self._cur = None                              # cur_sample: allocated once per (shape, dtype, device), kept across set_timesteps
        self._t_mismatch = None

    def set_timesteps(self, num_inference_steps, device=None):
        cfg = self.config
        T, n = cfg.num_train_timesteps, int(num_inference_steps)
        if n < 1 or n > T:
            raise ValueError(f"`num_inference_steps` ({num_inference_steps}) must be in [1, `num_train_timesteps`={T}]")
        if cfg.timestep_spacing == "linspace":
            base = np.linspace(0, T - 1, n).round().astype(np.int64)
        elif cfg.timestep_spacing == "leading":
            base = (np.arange(0, n) * (T // n)).round().astype(np.int64) + cfg.steps_offset
        else:
            base = np.round(np.arange(T, 0, -T / n))[::-1].astype(np.int64) - 1
        # the pseudo linear multistep table: the second timestep (counted from the noisy end) twice
        ts = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
        if len(ts) != n + 1 or ts.min() < 0 or ts.max() >= T:
            raise ValueError(f"timestep grid for n={n} leaves [0, {T}) or has {len(ts)} entries")
        self.num_inference_steps = n
        self._timesteps = ts
        # (the device grid is kept across calls with the same n / device: no H2D copy, and a captured graph's addresses stay valid)
        key = (n, None if device is None else str(torch.device(device)))
        if self._grid_key != key or device is None:
            self.timesteps = torch.from_numpy(ts).to(device)
            self._grid_key = key
        self.counter = 0
        self.ets = []

    @property
    def step_index(self):
        return self.counter if self.num_inference_steps is not None else None

    def verify_timesteps(self):
        """raise if a step that was handed a CUDA timestep from outside ``scheduler.timesteps`` was driven with another value than the
        counter's (one device->host read; every other kind of timestep is checked in ``step`` itself)"""
        m, self._t_mismatch = self._t_mismatch, None
        if m is not None and int(m.item()) != 0:
            raise RuntimeError("PNDMScheduler.step was called with CUDA timesteps that are not consecutive entries of scheduler.timesteps")

    def _check_timestep(self, timestep, k):
        want = int(self._timesteps[k])
        ts = self.timesteps
        if isinstance(timestep, torch.Tensor) and timestep.is_cuda:
            if ts.is_cuda and ts.device == timestep.device and timestep.dtype == ts.dtype:
                off, es = timestep.data_ptr() - ts.data_ptr(), ts.element_size()
                if 0 <= off < ts.numel() * es and off % es == 0:     # an element of scheduler.timesteps: no device->host read
                    if off // es != k:
                        raise ValueError(f"forward {k} was handed scheduler.timesteps[{off // es}]")
                    return
            bad = (timestep.reshape(-1)[:1] != want).to(torch.int32)
            self._t_mismatch = bad if self._t_mismatch is None else self._t_mismatch + bad
            return
        if int(timestep) != want:
            raise ValueError(f"forward {k} of set_timesteps({self.num_inference_steps}) is at timestep {want}, got {int(timestep)}")

    # ------------------------------------------------------------------ host scalars
    def _ac_at(self, t):
        return np.float64(self._ac[t]) if t >= 0 else np.float64(self._final_ac)

    def step_scalars(self, k, history=None):
        """(cx, [c_0 ..], restart) of forward k in fp64:  x' = cx xb + c_0 e + c_1 ets[-1] + ... , where e is this forward's model output and
        xb the sample -- the saved first sample when ``restart`` (forward 1).  ``history``: the number of model outputs in the update, by
        default that of a trajectory that started at forward 0 (host arithmetic only: usable without a GPU)."""
        cfg = self.config
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None'. Call 'set_timesteps' first.")
        r = cfg.num_train_timesteps // self.num_inference_steps
        t = int(self._timesteps[k])
        prev_t = t - r
        restart = k == 1
        if restart:
            prev_t, t = t, t + r                      # the repeated timestep: redo the first transfer
            w = (0.5, 0.5)                            # improved Euler: the mean of this model output and the first
        else:
            w = PLMS_WEIGHTS[min(k, 4) if k >= 2 else 1] if history is None else PLMS_WEIGHTS[history]
        a_t, a_p = self._ac_at(t), self._ac_at(prev_t)
        cx = np.sqrt(a_p / a_t)
        K = -(a_p - a_t) / (a_t * np.sqrt(1.0 - a_p) + np.sqrt(a_t * (1.0 - a_t) * a_p))
        if cfg.prediction_type == "v_prediction":     # eff <- sqrt(a_t) eff + sqrt(1 - a_t) x, applied to the combined output and the sample used
            cx, K = cx + K * np.sqrt(1.0 - a_t), K * np.sqrt(a_t)
        return cx, [K * np.float64(v) for v in w], restart

    # ------------------------------------------------------------------ step
    def step(self, model_output, timestep, sample, return_dict=True, *, eps_uncond=None, guidance_scale=1.0, eps_out=None, out=None,
             out_lp=None, **_ignored):
        """``DPMSolverMultistepScheduler.step``'s signature and dtype rules (diffusers' ``step_plms``).  ``eps_out`` receives the combined eps,
        the history entry; the scheduler keeps references to up to four of them -- the first forward's and the three newest -- so a caller
        that passes its own buffers rotates at least ``history_slots``."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None'. Call 'set_timesteps' first.")
        model_output, sample = step_inputs(model_output, sample, self.prev_sample_dtype)
        if sample.shape != model_output.shape:
            raise ValueError(f"sample {tuple(sample.shape)} and model_output {tuple(model_output.shape)} differ in shape")
        k = self.counter
        if k > self.num_inference_steps:
            raise ValueError(f"forward {k} is past the {self.num_inference_steps + 1} forwards of set_timesteps({self.num_inference_steps})")
        self._check_timestep(timestep, k)
        dev = model_output.device
        restart = k == 1
        hist = self.ets[::-1][:1] if restart else self.ets[::-1][:3]
        cx, cs, _ = self.step_scalars(k, None if restart else len(hist) + 1)
        eps_uncond = self._checked_eps_uncond(eps_uncond, model_output)
        if eps_uncond is None:
            m0 = model_output if eps_out is None else eps_out           # (with eps_out the kernel copies the model output into it)
        else:
            m0 = eps_out if eps_out is not None else torch.empty_like(model_output)
        m_out = None if m0 is model_output else m0
        if m_out is not None:
            self._check_eps_out(m_out, model_output)
        if any(m0.data_ptr() == m.data_ptr() for m in hist) and m0.numel():
            raise ValueError(f"this step's model output (or step(eps_out=...)) is a history entry the step still reads; rotate at least history_slots = {self.history_slots} buffers")
        prev = result_tensor(out, sample, contiguous_like_sample=True)
        if k == 0 or restart:
            if self._cur is None or self._cur.shape != sample.shape or self._cur.dtype != sample.dtype or self._cur.device != dev:
                if restart:
                    raise ValueError("the sample changed shape, dtype or device since the previous step; call set_timesteps")
                self._cur = torch.empty_like(sample)
            if k == 0:
                self._cur.copy_(sample)               # cur_sample: the second forward restarts from it
        a = L.CsLinStepArgs()
        fill_cfg(a, sample, model_output, eps_uncond, guidance_scale)
        a.x_base = self._cur.data_ptr() if restart else None
        fill_lin_history(a, hist, model_output)
        a.m_out = m_out.data_ptr() if m_out is not None else None
        fill_io(a, sample, model_output, prev, sample.dtype, out_lp)
        a.conv_x, a.conv_e, a.cx = 0.0, 1.0, float(cx)
        for j, c in enumerate(cs):
            a.c[j] = float(c)
        L.check(L.lib().cs_linear_step(C.byref(a), L.stream_ptr(dev)))
        if not restart:
            self.ets = self.ets[-3:] + [m0]
        self.counter += 1
        return (prev,) if not return_dict else SolverOutput(prev_sample=prev)
