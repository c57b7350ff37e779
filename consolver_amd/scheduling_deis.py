"""DEISMultistepScheduler -- DEIS (Zhang & Chen 2022), the log-rho multistep variant, orders 1 to 3, HIP-backed.

The scheduler the reference builds for ``type == "deis"`` (gen_ppo.py:139-143):

    DEISMultistepScheduler.from_pretrained(sd15, subfolder="scheduler")

diffusers is not installed and the reference does not vendor the class, so the config keys, their defaults
(``solver_order=2``, ``algorithm_type="deis"``, ``solver_type="logrho"``, ``lower_order_final=True``, linspace spacing, the last
sigma that of timestep 0), the order chosen per step and the identity conversion of an epsilon model output are a
restatement of diffusers 0.26.3 FROM MEMORY (DESIGN.md lists what rests on memory and what anchors it).  The coefficients
are anchored algebraically: they are the integrals of the Lagrange basis in log rho, tests/deis_oracle.py restates them in
diffusers' own form (``ind_fn`` differences), and tests/test_deis_oracle.py holds both to quadrature, to the first-order
DPM-Solver and to the exact solution for a model output that is a polynomial in log rho.

With rho = sigma / alpha (the entries of ``_sigmas``), m the converted model output, s0 the current grid point, t the next
and s1, s2 the previous ones, an update of order q is

    x_t = alpha_t (x / alpha_s0 + sum_{j < q} C_j m_sj),     C_j = int_{rho_s0}^{rho_t} L_j(log rho) d rho,

L_j the Lagrange basis on the nodes log rho_s0 .. log rho_s(q-1).  All of it is host arithmetic (fp64, passed as fp32) and
the device work per step is ONE kernel (cs_linear_step): optional CFG combine, conversion of the model output, the update
with up to three model outputs, and the optional 16-bit copy of an fp32 result.  The timestep and sigma grid is
scheduling_dpm's (SigmaGridMixin).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._scheduler_base import ConfigMixin, KARRAS_COMPATIBLES, SchedulerMixin, register_to_config
from .scheduling_dpm import SigmaGridMixin
from .scheduling_ppo import SolverOutput, fill_cfg, fill_io, result_tensor

# what the reference call site resolves to on SD1.5's scheduler_config.json (from memory, see the module docstring)
SD15_DEIS_KWARGS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", steps_offset=1)


def fill_lin_history(a, hist, model_output):
    """the history pointers of a CsLinStepArgs: ``hist`` newest first, every entry shaped like the model output"""
    for k, m in enumerate(hist):
        if m.shape != model_output.shape or m.dtype != model_output.dtype or m.device != model_output.device:
            raise ValueError("the model output changed shape, dtype or device since the previous step; call set_timesteps")
        a.hist[k] = m.data_ptr()
    a.terms = len(hist) + 1


def logrho_integrals(r0, r1, nodes):
    """[C_j] = int_{r0}^{r1} L_j(log rho) d rho for the Lagrange basis on ``nodes`` (values of log rho, one to three of them), fp64, from
    the antiderivatives rho, rho (log rho - 1) and rho (log^2 rho - 2 log rho + 2)"""
    r0, r1 = np.float64(r0), np.float64(r1)
    u = [np.float64(v) for v in nodes]
    l0, l1 = np.log(r0), np.log(r1)
    d0 = r1 - r0
    d1 = r1 * (l1 - 1.0) - r0 * (l0 - 1.0)
    d2 = r1 * (l1 * l1 - 2.0 * l1 + 2.0) - r0 * (l0 * l0 - 2.0 * l0 + 2.0)
    if len(u) == 1:
        return [d0]
    if len(u) == 2:
        return [(d1 - u[1] * d0) / (u[0] - u[1]), (d1 - u[0] * d0) / (u[1] - u[0])]
    out = []
    for j in range(3):
        a, b = (u[k] for k in range(3) if k != j)
        out.append((d2 - (a + b) * d1 + a * b * d0) / ((u[j] - a) * (u[j] - b)))
    return out


class DEISMultistepScheduler(SigmaGridMixin, SchedulerMixin, ConfigMixin):
    _compatibles = list(KARRAS_COMPATIBLES)
    order = 1
    prev_sample_dtype = None      # as DPMSolverMultistepScheduler.prev_sample_dtype
    factor_net = None             # no policy (SDSamplingEngine probes it)

    @register_to_config
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                 algorithm_type="deis", solver_type="logrho", lower_order_final=True, use_karras_sigmas=False,
                 timestep_spacing="linspace", steps_offset=0):
        if solver_order not in (1, 2, 3):
            raise NotImplementedError(f"solver_order={solver_order}: orders 1, 2 and 3 are implemented")
        if thresholding:
            raise NotImplementedError("thresholding is not implemented (a per-sample quantile, not a linear update)")
        if use_karras_sigmas:
            raise NotImplementedError("the Karras sigma option is not implemented")
        if algorithm_type != "deis":
            raise NotImplementedError(f"{algorithm_type} is not implemented for {self.__class__}")
        if solver_type != "logrho":
            raise NotImplementedError(f"{solver_type} is not implemented for {self.__class__}")
        if prediction_type == "sample":
            raise NotImplementedError("prediction_type 'sample' is not implemented")
        if prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon` or `v_prediction`")
        if timestep_spacing not in ("linspace", "leading", "trailing"):
            raise ValueError(f"{timestep_spacing} is not supported. Please make sure to choose one of 'linspace', 'leading' or 'trailing'.")
        self.history_slots = solver_order             # a step reads solver_order - 1 converted outputs and writes one more (SDSamplingEngine sizes its ring by it)
        self._init_tables(beta_schedule, beta_start, beta_end, num_train_timesteps, trained_betas)

    def set_timesteps(self, num_inference_steps, device=None):
        self._set_grid(num_inference_steps, device)   # (no final_sigmas_type in this class's config: the last sigma is that of timestep 0)

    # ------------------------------------------------------------------ host scalars
    def _order(self, i, lower_order_nums):
        """the order of step i with ``lower_order_nums`` earlier steps behind it (diffusers' rule)"""
        cfg, n = self.config, self.num_inference_steps
        short = cfg.lower_order_final and n < 15
        if cfg.solver_order == 1 or lower_order_nums < 1 or (short and i == n - 1):
            return 1
        if cfg.solver_order == 2 or lower_order_nums < 2 or (short and i == n - 2):
            return 2
        return 3

    def step_scalars(self, i, order=None):
        """(conv_x, conv_e, cx, [c_0 .. c_(order-1)]) of step i in fp64:  m0 = conv_x x + conv_e eps,  x' = cx x + c_0 m0 + c_1 m1 + c_2 m2.
        ``order=None``: as in a trajectory that started at step 0 (host arithmetic only: usable without a GPU)."""
        cfg = self.config
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None'. Call 'set_timesteps' first.")
        if order is None:
            order = self._order(i, min(i, cfg.solver_order))
        if order < 1 or order > 3 or order > i + 1:
            raise ValueError(f"step {i} has no update of order {order}")
        rho = self._sigmas.astype(np.float64)
        a_s, s_s, _ = self._alpha_sigma_lambda(rho[i])
        a_t, _, _ = self._alpha_sigma_lambda(rho[i + 1])
        conv = (s_s, a_s) if cfg.prediction_type == "v_prediction" else (0.0, 1.0)
        cs = logrho_integrals(rho[i], rho[i + 1], [np.log(rho[i - j]) for j in range(order)])
        return conv[0], conv[1], a_t / a_s, [a_t * c for c in cs]

    # ------------------------------------------------------------------ step
    def step(self, model_output, timestep, sample, return_dict=True, *, eps_uncond=None, guidance_scale=1.0, eps_out=None, out=None,
             out_lp=None, **_ignored):
        """``DPMSolverMultistepScheduler.step``'s signature and dtype rules.  ``eps_out`` receives the converted model output (the history
        entry: the combined eps, or sigma x + alpha v under v prediction); the scheduler keeps references to the last ``solver_order`` of
        them, so a caller that passes its own buffers rotates at least ``history_slots``."""
        model_output, sample, i = self._begin_step(model_output, timestep, sample)
        dev = model_output.device
        order = self._order(i, self._lower_order_nums)
        conv_x, conv_e, cx, cs = self.step_scalars(i, order)
        eps_uncond = self._checked_eps_uncond(eps_uncond, model_output)
        if order - 1 > len(self._m):
            raise ValueError(f"step {i} reads {order - 1} earlier converted outputs, {len(self._m)} are kept; start a trajectory at the first timestep")
        hist = self._m[:order - 1]
        identity = (np.float32(conv_x) == 0.0 and np.float32(conv_e) == 1.0)
        if eps_uncond is None and identity:
            m0 = model_output if eps_out is None else eps_out           # (with eps_out the kernel copies the model output into it)
        else:
            m0 = eps_out if eps_out is not None else torch.empty_like(model_output)
        m_out = None if m0 is model_output else m0
        if m_out is not None:
            self._check_eps_out(m_out, model_output)
            if any(m_out.data_ptr() == m.data_ptr() for m in hist) and m_out.numel():
                raise ValueError(f"step(eps_out=...) is a converted output this step still reads; rotate at least history_slots = {self.history_slots} buffers")
        prev = result_tensor(out, sample, contiguous_like_sample=True)
        a = L.CsLinStepArgs()
        fill_cfg(a, sample, model_output, eps_uncond, guidance_scale)
        fill_lin_history(a, hist, model_output)
        a.m_out = m_out.data_ptr() if m_out is not None else None
        fill_io(a, sample, model_output, prev, sample.dtype, out_lp)
        a.conv_x, a.conv_e, a.cx = float(conv_x), float(conv_e), float(cx)
        for k, c in enumerate(cs):
            a.c[k] = float(c)
        L.check(L.lib().cs_linear_step(C.byref(a), L.stream_ptr(dev)))
        self._m = [m0] + self._m[:self.config.solver_order - 1]
        if self._lower_order_nums < self.config.solver_order:
            self._lower_order_nums += 1
        self._step_index += 1
        return (prev,) if not return_dict else SolverOutput(prev_sample=prev)
