"""DPMSolverMultistepScheduler -- the Multistep DPM-Solver (orders 1 and 2), HIP-backed.

The scheduler both reference call sites build (gen_pretrain/generate_data.py:86-91, the 40-step teacher of the training
pairs; gen_ppo.py:149-155, ``type == "multistep-dpmsolver"``, the strongest training-free baseline of the results table):

    DPMSolverMultistepScheduler.from_pretrained(sd15, subfolder="scheduler", algorithm_type="dpmsolver", final_sigmas_type="sigma_min")

diffusers is not installed and the reference does not vendor the class, so the arithmetic is a restatement of the
published algorithm (Lu et al., DPM-Solver / DPM-Solver++) in diffusers 0.26.3's parametrisation, FROM MEMORY: the
constructor defaults, the keys of SD1.5's ``scheduler_config.json`` (no ``timestep_spacing``: the class default applies)
and the fp32 upcast of the sample inside ``step``.  tests/dpm_oracle.py restates it independently; the tests anchor both
to the golden-pinned DDIM path and to the order of convergence.

Every variant (``dpmsolver`` / ``dpmsolver++``, epsilon / v prediction, first / second order, midpoint / heun) is one
linear update per element, so all variant logic is host arithmetic (fp64, passed as fp32) and the device work per step
is ONE kernel (cs_dpm_multistep_step): optional CFG combine, conversion of the model output (m0, the history entry),
the update, and the optional 16-bit copy of an fp32 result.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import tables
from ._scheduler_base import ConfigMixin, KARRAS_COMPATIBLES, SchedulerMixin, register_to_config
from .scheduling_ppo import SolverOutput, fill_cfg, fill_io, result_tensor, step_inputs

# what the two reference call sites resolve to on SD1.5's scheduler_config.json (from memory, see the module docstring)
SD15_MULTISTEP_DPM_KWARGS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1,
                                 algorithm_type="dpmsolver", final_sigmas_type="sigma_min")


class SigmaGridMixin:
    """what the sigma-parametrised multistep schedulers (this module, scheduling_unipc.py, scheduling_amed.py) share: the beta tables, the
    timestep / sigma grid of diffusers 0.26.3's ``set_timesteps``, the step counter and the protocol stubs.  The class needs ``config`` with
    ``num_train_timesteps``, ``timestep_spacing`` and ``steps_offset``; ``final_sigmas_type`` is read where the class has it."""

    def _init_tables(self, beta_schedule, beta_start, beta_end, num_train_timesteps, trained_betas):
        self._betas = tables.make_betas(beta_schedule, beta_start, beta_end, num_train_timesteps, trained_betas)
        self._ac = tables.alphas_cumprod(self._betas)
        self.betas = torch.from_numpy(self._betas)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.from_numpy(self._ac)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self._timesteps = np.arange(0, num_train_timesteps, dtype=np.int64)[::-1].copy()
        self.timesteps = torch.from_numpy(self._timesteps)
        self.sigmas = None
        self._sigmas = None
        self._step_index = None
        self._lower_order_nums = 0
        self._m = []                                  # converted model outputs, newest first
        self._grid_key = None

    # ------------------------------------------------------------------ protocol
    @property
    def step_index(self):
        return self._step_index

    def __len__(self):
        return self.config.num_train_timesteps

    def scale_model_input(self, sample, timestep=None):
        return sample

    def verify_timesteps(self):
        """nothing to verify: after the first step the grid position is a host counter (as in diffusers)."""

    def _set_grid(self, num_inference_steps, device=None):
        """the timestep grid of ``timestep_spacing`` and its sigmas (interpolated, plus the final sigma); resets the step counter and the history"""
        cfg = self.config
        T, n = cfg.num_train_timesteps, int(num_inference_steps)
        if n < 1 or n > T:
            raise ValueError(f"`num_inference_steps` ({num_inference_steps}) must be in [1, `num_train_timesteps`={T}]")
        if cfg.timestep_spacing == "linspace":
            ts = np.linspace(0, T - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        elif cfg.timestep_spacing == "leading":
            ts = (np.arange(0, n + 1) * (T // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) + cfg.steps_offset
        else:
            ts = (np.round(np.arange(T, 0, -T / n)) - 1).astype(np.int64)
        if len(ts) != n or ts.min() < 0 or ts.max() >= T:
            raise ValueError(f"timestep grid for n={n} leaves [0, {T}) or has {len(ts)} entries")
        ac = self._ac.astype(np.float64)
        s = np.sqrt((1.0 - ac) / ac)
        sig = np.interp(ts, np.arange(T), s)
        last = s[0] if cfg.get("final_sigmas_type", "sigma_min") == "sigma_min" else 0.0      # (a class without the key, DEIS, ends on the sigma of timestep 0)
        self._sigmas = np.concatenate([sig, [last]]).astype(np.float32)
        self.sigmas = torch.from_numpy(self._sigmas)
        self.num_inference_steps = n
        self._timesteps = ts
        # (the device grid is kept across calls with the same n / device: no H2D copy, steps are found by address)
        key = (n, None if device is None else str(torch.device(device)))
        if self._grid_key != key or device is None:
            self.timesteps = torch.from_numpy(ts).to(device)
            self._grid_key = key
        self._step_index = None
        self._lower_order_nums = 0
        self._m = []

    def _init_step_index(self, timestep):
        ts = self.timesteps
        if isinstance(timestep, torch.Tensor) and timestep.is_cuda:
            if ts.is_cuda and ts.device == timestep.device and timestep.dtype == ts.dtype:
                off, es = timestep.data_ptr() - ts.data_ptr(), ts.element_size()
                if 0 <= off < ts.numel() * es and off % es == 0:     # an element of scheduler.timesteps: no device->host read
                    return off // es
            timestep = timestep.item()
        idx = np.nonzero(self._timesteps == int(timestep))[0]
        if len(idx) == 0:
            raise ValueError(f"timestep {int(timestep)} is not on the grid of set_timesteps({self.num_inference_steps})")
        return int(idx[1 if len(idx) > 1 else 0])

    def _begin_step(self, model_output, timestep, sample):
        """what ``step`` checks and normalises before it plans the update: -> (model_output, sample, step index), ``DDIMBaselineScheduler.step``'s
        dtype rules"""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None'. Call 'set_timesteps' first.")
        model_output, sample = step_inputs(model_output, sample, self.prev_sample_dtype)
        if sample.shape != model_output.shape:
            raise ValueError(f"sample {tuple(sample.shape)} and model_output {tuple(model_output.shape)} differ in shape")
        if self._step_index is None:
            self._step_index = self._init_step_index(timestep)
        i = self._step_index
        if i >= self.num_inference_steps:
            raise ValueError(f"step {i} is past the {self.num_inference_steps} steps of set_timesteps")
        return model_output, sample, i

    @staticmethod
    def _checked_eps_uncond(eps_uncond, model_output):
        if eps_uncond is not None:
            eps_uncond = L.require_cuda(eps_uncond, "eps_uncond").contiguous()
            if eps_uncond.shape != model_output.shape or eps_uncond.dtype != model_output.dtype:
                raise ValueError("eps_uncond must have the model output's shape and dtype")
        return eps_uncond

    @staticmethod
    def _check_eps_out(m, model_output):
        if m.shape != model_output.shape or m.dtype != model_output.dtype or not m.is_contiguous():
            raise ValueError("step(eps_out=...) must be contiguous with the model output's shape and dtype")

    @staticmethod
    def _alpha_sigma_lambda(sigma):
        sigma = np.float64(sigma)
        alpha = 1.0 / np.sqrt(sigma * sigma + 1.0)
        sh = sigma * alpha
        with np.errstate(divide="ignore"):
            lam = np.log(alpha) - np.log(sh)
        return alpha, sh, lam


class DPMSolverMultistepScheduler(SigmaGridMixin, SchedulerMixin, ConfigMixin):
    _compatibles = list(KARRAS_COMPATIBLES)
    order = 1
    prev_sample_dtype = None      # as HistoryMixin.prev_sample_dtype: torch.float32 promotes a 16-bit sample
    factor_net = None             # no policy (SDSamplingEngine probes it)

    @register_to_config
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                 algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, euler_at_final=False,
                 use_karras_sigmas=False, use_lu_lambdas=False, use_exponential_sigmas=False, final_sigmas_type="zero",
                 lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0):
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order}: orders 1 and 2 are implemented")
        if thresholding:
            raise NotImplementedError("thresholding is not implemented (a per-sample quantile, not a linear update)")
        if use_karras_sigmas or use_lu_lambdas or use_exponential_sigmas:
            raise NotImplementedError("the Karras / Lu / exponential sigma options are not implemented")
        if algorithm_type in ("sde-dpmsolver", "sde-dpmsolver++"):
            raise NotImplementedError(f"algorithm_type={algorithm_type!r}: the SDE variants are not implemented")
        if algorithm_type not in ("dpmsolver", "dpmsolver++"):
            raise NotImplementedError(f"{algorithm_type} is not implemented for {self.__class__}")
        if variance_type is not None:
            raise NotImplementedError("variance_type (learned-variance model outputs) is not implemented")
        if lambda_min_clipped != -float("inf"):
            raise NotImplementedError("lambda_min_clipped is not implemented")
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"{solver_type} is not implemented for {self.__class__}")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon` or `v_prediction`")
        if final_sigmas_type not in ("zero", "sigma_min"):
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {final_sigmas_type}")
        if algorithm_type == "dpmsolver" and final_sigmas_type == "zero":
            raise ValueError(f"`final_sigmas_type` {final_sigmas_type} is not supported for `algorithm_type` {algorithm_type}. "
                             "Please choose `sigma_min` instead.")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"{timestep_spacing} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        self._init_tables(beta_schedule, beta_start, beta_end, num_train_timesteps, trained_betas)

    def set_timesteps(self, num_inference_steps, device=None):
        self._set_grid(num_inference_steps, device)

    # ------------------------------------------------------------------ host scalars
    def _first_order(self, i, lower_order_nums):
        cfg, n = self.config, self.num_inference_steps
        final = (i == n - 1) and (cfg.euler_at_final or (cfg.lower_order_final and n < 15) or cfg.final_sigmas_type == "zero")
        return cfg.solver_order == 1 or lower_order_nums < 1 or final

    def step_scalars(self, i, first_order=None):
        """(conv_x, conv_e, cx, c0, c1) of step i in fp64:  m0 = conv_x x + conv_e eps,  x' = cx x + c0 m0 + c1 m1  (c1 = 0 at first order).
        ``first_order=None``: as in a trajectory that started at step 0 (host arithmetic only: usable without a GPU)."""
        cfg = self.config
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None'. Call 'set_timesteps' first.")
        if first_order is None:
            first_order = self._first_order(i, min(i, cfg.solver_order))
        pp, vpred = cfg.algorithm_type == "dpmsolver++", cfg.prediction_type == "v_prediction"
        a_s, s_s, l_s = self._alpha_sigma_lambda(self._sigmas[i])
        a_t, s_t, l_t = self._alpha_sigma_lambda(self._sigmas[i + 1])
        h = l_t - l_s
        if pp:
            conv = (a_s, -s_s) if vpred else (1.0 / a_s, -s_s / a_s)
            cx, k0 = s_t / s_s, -a_t * np.expm1(-h)
        else:
            conv = (s_s, a_s) if vpred else (0.0, 1.0)
            cx, k0 = a_t / a_s, -s_t * np.expm1(h)
        if first_order or h == 0.0:                   # (h = 0: a grid that ends ON sigma_min, e.g. trailing with n = T; the step is the identity and k1 = 0)
            return conv[0], conv[1], cx, k0, 0.0
        _, _, l_r = self._alpha_sigma_lambda(self._sigmas[i - 1])
        r0 = (l_s - l_r) / h
        if cfg.solver_type == "midpoint":
            k1 = 0.5 * k0
        elif pp:
            k1 = a_t * (np.expm1(-h) / h + 1.0)
        else:
            k1 = -s_t * (np.expm1(h) / h - 1.0)
        return conv[0], conv[1], cx, k0 + k1 / r0, -k1 / r0

    # ------------------------------------------------------------------ step
    def step(self, model_output, timestep, sample, return_dict=True, *, eps_uncond=None, guidance_scale=1.0, eps_out=None, out=None,
             out_lp=None, **_ignored):
        """``DDIMBaselineScheduler.step``'s signature and dtype rules.  ``eps_out`` receives the converted model output m0 (the
        history entry: the combined eps for ``dpmsolver``, the x0 prediction for ``dpmsolver++``); the scheduler keeps a
        reference to it for the next step, so a caller that passes its own buffers rotates at least ``solver_order`` of them."""
        model_output, sample, i = self._begin_step(model_output, timestep, sample)
        dev = model_output.device
        first = self._first_order(i, self._lower_order_nums)
        conv_x, conv_e, cx, c0, c1 = self.step_scalars(i, first)
        eps_uncond = self._checked_eps_uncond(eps_uncond, model_output)
        m_prev = None
        if not first:
            m_prev = self._m[0]
            if m_prev.shape != model_output.shape or m_prev.dtype != model_output.dtype or m_prev.device != dev:
                raise ValueError("the model output changed shape, dtype or device since the previous step; call set_timesteps")
        identity = (np.float32(conv_x) == 0.0 and np.float32(conv_e) == 1.0)
        if eps_uncond is None and identity:
            m0 = model_output if eps_out is None else eps_out           # (with eps_out the kernel copies the model output into it)
        else:
            m0 = eps_out if eps_out is not None else torch.empty_like(model_output)
        m_out = None if m0 is model_output else m0
        if m_out is not None:
            self._check_eps_out(m_out, model_output)
        prev = result_tensor(out, sample, contiguous_like_sample=True)
        a = L.CsDpmStepArgs()
        fill_cfg(a, sample, model_output, eps_uncond, guidance_scale)
        a.m_prev = m_prev.data_ptr() if m_prev is not None else None
        a.m_out = m_out.data_ptr() if m_out is not None else None
        fill_io(a, sample, model_output, prev, sample.dtype, out_lp)
        a.conv_x, a.conv_e, a.cx, a.c0, a.c1 = float(conv_x), float(conv_e), float(cx), float(c0), float(c1)
        L.check(L.lib().cs_dpm_multistep_step(C.byref(a), L.stream_ptr(dev)))
        self._m = [m0] + self._m[:self.config.solver_order - 1]
        if self._lower_order_nums < self.config.solver_order:
            self._lower_order_nums += 1
        self._step_index += 1
        return (prev,) if not return_dict else SolverOutput(prev_sample=prev)
