"""UniPCMultistepScheduler -- UniPC (Zhao et al. 2023), bh1 / bh2, orders 1 and 2, x0 prediction, HIP-backed.

The scheduler the reference builds for ``type == "unipc"`` (gen_ppo.py:133-137):

    UniPCMultistepScheduler.from_pretrained(sd15, subfolder="scheduler")

diffusers is not installed and the reference does not vendor the class, so the config keys, their defaults, the order
of operations inside ``step`` and the last sigma are a restatement of diffusers 0.26.3 FROM MEMORY (DESIGN.md lists
what rests on memory and what anchors it).  The coefficients themselves are anchored algebraically: tests/unipc_oracle.py
restates the algorithm independently, and tests/test_unipc_oracle.py ties it to the golden-pinned DDIM path, to
DPM-Solver++ 2M and to the exact solution for a polynomial model output.

A step applies the corrector to the PREVIOUS update (it needs the model output just computed, converted at the
predicted sample) and then the predictor from the corrected sample.  Both are linear in the same tensors, so all
variant logic is host arithmetic (fp64, passed as fp32) and the device work per step is ONE kernel (cs_unipc_step):
optional CFG combine, conversion, corrector, predictor, and the optional 16-bit copy of an fp32 result.  The timestep
and sigma grid is scheduling_dpm's (SigmaGridMixin).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._scheduler_base import ConfigMixin, KARRAS_COMPATIBLES, SchedulerMixin, register_to_config
from .scheduling_dpm import SigmaGridMixin
from .scheduling_ppo import SolverOutput, fill_cfg, fill_io, result_tensor

# what the reference call site resolves to on SD1.5's scheduler_config.json (from memory, see the module docstring)
SD15_UNIPC_KWARGS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1)


class UniPCMultistepScheduler(SigmaGridMixin, SchedulerMixin, ConfigMixin):
    _compatibles = list(KARRAS_COMPATIBLES)
    order = 1
    prev_sample_dtype = None      # as DPMSolverMultistepScheduler.prev_sample_dtype
    factor_net = None             # no policy (SDSamplingEngine probes it)

    @register_to_config
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                 predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=[], solver_p=None,
                 use_karras_sigmas=False, timestep_spacing="linspace", steps_offset=0, final_sigmas_type="sigma_min"):
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order={solver_order}: orders 1 and 2 are implemented")
        if not predict_x0:
            raise NotImplementedError("predict_x0=False (the noise-prediction form) is not implemented")
        if thresholding:
            raise NotImplementedError("thresholding is not implemented (a per-sample quantile, not a linear update)")
        if use_karras_sigmas:
            raise NotImplementedError("the Karras sigma option is not implemented")
        if solver_p is not None:
            raise NotImplementedError("solver_p (another scheduler as the predictor) is not implemented")
        if solver_type not in ("bh1", "bh2"):
            raise NotImplementedError(f"{solver_type} is not implemented for {self.__class__}")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon` or `v_prediction`")
        if final_sigmas_type not in ("zero", "sigma_min"):
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {final_sigmas_type}")
        if final_sigmas_type == "zero" and not lower_order_final:
            raise ValueError("`final_sigmas_type` 'zero' needs `lower_order_final`: only the first-order update has a limit at sigma = 0")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"{timestep_spacing} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        self._disable_corrector = frozenset(int(i) for i in disable_corrector)
        self.history_slots = solver_order + 1         # a step reads two converted outputs and writes a third (SDSamplingEngine sizes its ring by it)
        self._init_tables(beta_schedule, beta_start, beta_end, num_train_timesteps, trained_betas)
        self._this_order = 0                          # the order of the previous step's predictor: what its corrector runs with
        self._last = None                             # last_sample: allocated once per (shape, dtype, device), kept across set_timesteps
        self._have_last = False

    def set_timesteps(self, num_inference_steps, device=None):
        self._set_grid(num_inference_steps, device)
        self._this_order = 0
        self._have_last = False

    @property
    def last_sample(self):
        return self._last if self._have_last else None

    # ------------------------------------------------------------------ host scalars
    def _order(self, i, lower_order_nums):
        cfg = self.config
        o = min(cfg.solver_order, self.num_inference_steps - i) if cfg.lower_order_final else cfg.solver_order
        return min(o, lower_order_nums + 1)

    def _bh(self, s0, t, r1, corrector, order):
        """(cx, k0, k1, kn) of one UniPC update of ``order`` over the grid step s0 -> t:  x_t = cx x + k0 m0 + k1 m1 + kn m_t, where m0 is the
        converted output at s0, m1 the one before it (at lambda_s0 + r1 h; order 2) and m_t the one at t (corrector only)."""
        a_s, s_s, l_s = self._alpha_sigma_lambda(self._sigmas[s0])
        a_t, s_t, l_t = self._alpha_sigma_lambda(self._sigmas[t])
        if s_t == 0.0:                                # final sigma zero: h = inf, h_phi_1 = -1; first order only (the constructor checks lower_order_final)
            if order != 1 or corrector:
                raise ValueError("a step to sigma = 0 is a first-order predictor step")
            return 0.0, 1.0, 0.0, 0.0
        h = l_t - l_s
        if h == 0.0:                                  # a grid that ends ON sigma_min: the step is the identity
            return 1.0, 0.0, 0.0, 0.0
        hh = -h
        h_phi_1 = np.expm1(hh)
        B_h = h_phi_1 if self.config.solver_type == "bh2" else hh
        rks = ([r1] if order == 2 else []) + [1.0]
        R, b = [], []
        h_phi_k, f = h_phi_1 / hh - 1.0, 1.0
        for j in range(1, order + 1):
            R.append(np.power(rks, j - 1))
            b.append(h_phi_k * f / B_h)
            f *= j + 1
            h_phi_k = h_phi_k / hh - 1.0 / f
        R, b = np.asarray(R, np.float64), np.asarray(b, np.float64)
        if corrector:
            rhos = np.array([0.5]) if order == 1 else np.linalg.solve(R, b)
        else:
            rhos = np.array([0.5]) if order == 2 else np.zeros(0)
        cx, k0, k1, kn = s_t / s_s, -a_t * h_phi_1, 0.0, 0.0
        if order == 2:                                # rho_0 D1, D1 = (m1 - m0) / r1
            k1 = -a_t * B_h * rhos[0] / r1
            k0 -= k1
        if corrector:                                 # rho_last (m_t - m0)
            kn = -a_t * B_h * rhos[-1]
            k0 -= kn
        return cx, k0, k1, kn

    def _r1(self, s0, t):
        """r of the history entry before s0, relative to the step s0 -> t"""
        l = [self._alpha_sigma_lambda(self._sigmas[k])[2] for k in (s0 - 1, s0, t)]
        with np.errstate(divide="ignore", invalid="ignore"):
            return (l[0] - l[1]) / (l[2] - l[1])

    def step_scalars(self, i, corr_order=None, this_order=None, use_corr=None):
        """(conv_x, conv_e, (a_x, a_0, a_1, a_n), (p_x, p_0, p_1), use_corr) of step i in fp64:
            m_new = conv_x x + conv_e eps;  x_c = a_x x_last + a_0 m_prev0 + a_1 m_prev1 + a_n m_new (x_c = x without the corrector);
            x_next = p_x x_c + p_0 m_new + p_1 m_prev0.
        The orders default to those of a trajectory that started at step 0 (host arithmetic only: usable without a GPU)."""
        cfg = self.config
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None'. Call 'set_timesteps' first.")
        if corr_order is None:
            corr_order = self._order(i - 1, min(i - 1, cfg.solver_order)) if i > 0 else 0
        if this_order is None:
            this_order = self._order(i, min(i, cfg.solver_order))
        if use_corr is None:
            use_corr = i > 0 and (i - 1) not in self._disable_corrector
        a_s, s_s, _ = self._alpha_sigma_lambda(self._sigmas[i])
        conv = (a_s, -s_s) if cfg.prediction_type == "v_prediction" else (1.0 / a_s, -s_s / a_s)
        a = (1.0, 0.0, 0.0, 0.0)
        if use_corr:
            a = self._bh(i - 1, i, self._r1(i - 1, i) if corr_order == 2 else None, True, corr_order)
        px, p0, p1, _ = self._bh(i, i + 1, self._r1(i, i + 1) if this_order == 2 else None, False, this_order)
        return conv[0], conv[1], a, (px, p0, p1), bool(use_corr)

    # ------------------------------------------------------------------ step
    def step(self, model_output, timestep, sample, return_dict=True, *, eps_uncond=None, guidance_scale=1.0, eps_out=None, out=None,
             out_lp=None, **_ignored):
        """``DPMSolverMultistepScheduler.step``'s signature and dtype rules.  ``sample`` is the previous call's result (the predicted
        sample).  ``eps_out`` receives the converted model output (the x0 prediction, the history entry); the scheduler keeps references
        to the last ``solver_order`` of them, so a caller that passes its own buffers rotates at least ``history_slots``."""
        model_output, sample, i = self._begin_step(model_output, timestep, sample)
        dev = model_output.device
        use_corr = i > 0 and (i - 1) not in self._disable_corrector and self._have_last
        corr_order = self._this_order
        this_order = self._order(i, self._lower_order_nums)
        conv_x, conv_e, (a_x, a_0, a_1, a_n), (p_x, p_0, p_1), use_corr = self.step_scalars(i, corr_order, this_order, use_corr)
        eps_uncond = self._checked_eps_uncond(eps_uncond, model_output)
        need =2 if (use_corr and a_1 != 0.0) else 1 if ((use_corr and a_0 != 0.0) or p_1 != 0.0) else 0
        if need > len(self._m):
            raise ValueError(f"step {i} reads {need} earlier converted outputs, {len(self._m)} are kept; start a trajectory at the first timestep")
        for m in self._m[:need]:
            if m.shape != model_output.shape or m.dtype != model_output.dtype or m.device != dev:
                raise ValueError("the model output changed shape, dtype or device since the previous step; call set_timesteps")
        m_new = eps_out if eps_out is not None else torch.empty_like(model_output)
        self._check_eps_out(m_new, model_output)
        if any(m_new.data_ptr() == m.data_ptr() for m in self._m[:need]) and m_new.numel():
            raise ValueError(f"step(eps_out=...) is a converted output this step still reads; rotate at least history_slots = {self.history_slots} buffers")
        prev = result_tensor(out, sample, contiguous_like_sample=True)
        if self._last is None or self._last.shape != sample.shape or self._last.dtype != sample.dtype or self._last.device != dev:
            if use_corr:
                raise ValueError("the sample changed shape, dtype or device since the previous step; call set_timesteps")
            self._last = torch.empty_like(sample)
        a = L.CsUnipcStepArgs()
        fill_cfg(a, sample, model_output, eps_uncond, guidance_scale)
        a.use_corr = int(use_corr)
        a.x_last = self._last.data_ptr() if use_corr else None
        a.m_prev0 = self._m[0].data_ptr() if need >= 1 else None
        a.m_prev1 = self._m[1].data_ptr() if need >= 2 else None
        a.m_out, a.x_last_out = m_new.data_ptr(), self._last.data_ptr()      # (x_last is updated in place)
        fill_io(a, sample, model_output, prev, sample.dtype, out_lp)
        a.conv_x, a.conv_e = float(conv_x), float(conv_e)
        a.a_x, a.a_0, a.a_1, a.a_n = float(a_x), float(a_0), float(a_1), float(a_n)
        a.p_x, a.p_0, a.p_1 = float(p_x), float(p_0), float(p_1)
        L.check(L.lib().cs_unipc_step(C.byref(a), L.stream_ptr(dev)))
        self._m = [m_new] + self._m[:self.config.solver_order - 1]
        self._have_last = True
        self._this_order = this_order
        if self._lower_order_nums < self.config.solver_order:
            self._lower_order_nums += 1
        self._step_index += 1
        return (prev,) if not return_dict else SolverOutput(prev_sample=prev)
