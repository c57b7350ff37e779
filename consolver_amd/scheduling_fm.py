"""FlowMatchGeneralDiscreteScheduler -- the FLUX-side comparison solvers (Euler, Heun, dpm-solver, multistep dpm-solver), HIP-backed.

Drop-in for the reference's ``FlowMatchGeneralDiscreteScheduler`` (edit_ppo/scheduler_fm.py:46-583, run by
edit_ppo/generate_pretrain.py:118-122 with ``type=...``): the constructor arguments of :90-107, ``set_timesteps(num_inference_steps=None,
device=None, sigmas=None, mu=None, timesteps=None)``, ``set_begin_index``, ``step_index``, ``scale_noise``,
``from_pretrained(repo, subfolder=..., type=...)`` and ``step(model_output, timestep, sample, ..., return_dict)``.  The sigma schedule is
``tables.flux_sigma_schedule``, the table code of ``FMPPOScheduler``.

Every branch of the reference's ``step`` (:405-482) is ``x' = cast(x_base + c * w)``:

    ==============================================  ==================  =========  ==================================
    branch                                          x_base              w          c
    ==============================================  ==================  =========  ==================================
    Euler and every first stage (:410,422,442,469)  this step's sample  v          dt
    Heun second stage (:430)                        the saved sample    v1 + v2    0.5 dt_saved
    dpm-solver second stage (:452), multistep (:480)  the saved sample  v2         dt_saved + (sigma_next - sigma)
    ==============================================  ==================  =========  ==================================

``step_plan`` decides the row on the host (``FmStepPlan``), ONE kernel (cs_fm_general_step) applies it, ``commit_plan`` keeps what the next
step needs.  The saved sample and model output are references to the caller's tensors, as in the reference (no copies), so a caller that
reuses those buffers (``out=`` aliasing a tensor handed in earlier) changes the saved state exactly as it would there.  All state is on the
host: ``step`` neither syncs the device nor reads a device tensor.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from ._scheduler_base import ConfigMixin, SchedulerMixin, register_to_config
from .scheduling_fmppo import FlowMatchScheduleMixin
from .scheduling_ppo import SolverOutput, fill_io, step_inputs

FM_SOLVER_TYPES = ("euler", "heun", "dpm-solver", "dpm-solver-multistep")

# base: "sample" (this step's) | "saved"; use_v1: w = v1 + v2 with the saved model output; c: the fp32 host scalar;
# save: None | "all" (sample, model output, dt) | "sample" (sample and dt: the multistep hand-over); dt: the value ``save`` stores
FmStepPlan = collections.namedtuple("FmStepPlan", "base use_v1 c save dt")


class FlowMatchGeneralDiscreteScheduler(FlowMatchScheduleMixin, SchedulerMixin, ConfigMixin):
    """``class FlowMatchGeneralDiscreteScheduler(SchedulerMixin, ConfigMixin)`` of edit_ppo/scheduler_fm.py:46."""
    _compatibles = []
    order = 1

    @register_to_config
    def __init__(self, num_train_timesteps=1000, shift=1.0, use_dynamic_shifting=False, base_shift=0.5, max_shift=1.15,
                 base_image_seq_len=256, max_image_seq_len=4096, invert_sigmas=False, shift_terminal=None, use_karras_sigmas=False,
                 use_exponential_sigmas=False, use_beta_sigmas=False, time_shift_type="exponential", stochastic_sampling=False,
                 type="euler"):
        if type not in FM_SOLVER_TYPES:
            raise ValueError(f"unknown type {type!r}; expected one of {FM_SOLVER_TYPES}")       # (the reference leaves prev_sample unbound, :486-488)
        self._init_schedule()
        self.type = type
        self.prev_model_output = self.prev_sample = self.prev_dt = None

    def set_timesteps(self, num_inference_steps=None, device=None, sigmas=None, mu=None, timesteps=None):
        """scheduler_fm.py:259-359, and the saved sample / model output / dt are dropped.  The reference means to drop them too (:140-144), but
        that definition is shadowed by the one at :259 and never runs, so there a scheduler reused after a run that ended on a first stage (odd
        n with Heun or dpm-solver) or started mid-pair would read the previous run's state; here such a step raises."""
        self._set_schedule(num_inference_steps, device, sigmas, mu, timesteps)
        self.prev_model_output = self.prev_sample = self.prev_dt = None

    # ------------------------------------------------------------------ the step, in three parts
    def step_plan(self):
        """The update of the step at ``step_index`` as an ``FmStepPlan``: host fp32 arithmetic on the sigma table only (scheduler_fm.py:405-482)."""
        i, sig = self._step_index, self._sigmas
        if i is None:
            raise ValueError("step_index is None: call set_begin_index() or step() with one of scheduler.timesteps")
        if not 0 <= i < len(sig) - 1:
            raise IndexError(f"step {i} of a {len(sig) - 1}-step schedule")
        d = np.float32(sig[i + 1] - sig[i])
        if self.type == "euler":
            return FmStepPlan("sample", False, d, None, None)
        first = (i == 0) if self.type == "dpm-solver-multistep" else (i % 2 == 0)
        if first:
            if self.type == "heun":                     # the predictor spans both intervals; the last sigma when the pair runs off the table (:417)
                d = np.float32(sig[min(i + 2, len(sig) - 1)] - sig[i])
            return FmStepPlan("sample", False, d, "all", d)
        if self.prev_dt is None:
            raise ValueError(f"step {i} of type {self.type!r} is a second stage but no first stage was run since set_timesteps")
        if self.type == "heun":
            return FmStepPlan("saved", True, np.float32(np.float32(0.5) * self.prev_dt), None, None)
        c = np.float32(self.prev_dt + d)
        if self.type == "dpm-solver":
            return FmStepPlan("saved", False, c, None, None)
        return FmStepPlan("saved", False, c, "sample", d)

    def commit_plan(self, plan, sample, model_output):
        """what scheduler_fm.py keeps after the update (:419-421, :482-483) -- references, not copies -- and ``step_index += 1``."""
        if plan.save is not None:
            self.prev_sample, self.prev_dt = sample, plan.dt
            if plan.save == "all":
                self.prev_model_output = model_output
        self._step_index += 1

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None,
             per_token_timesteps=None, return_dict=True, *, out=None):
        """scheduler_fm.py:384-493.  ``s_churn``, ``s_tmin``, ``s_tmax``, ``s_noise``, ``generator`` and ``per_token_timesteps`` are accepted and
        ignored, as there.  ``prev_sample`` has the model output's dtype (:488); ``out``: the tensor to write it to."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None'. Call 'set_timesteps' first.")
        if self._step_index is None:
            self._init_step_index(timestep)
        model_output, sample = step_inputs(model_output, sample)        # (an fp32 sample is consumed as fp32: :401 upcasts it)
        plan = self.step_plan()
        base = sample if plan.base == "sample" else self.prev_sample
        v1 = self.prev_model_output if plan.use_v1 else None
        if base.shape != model_output.shape or (v1 is not None and (v1.shape != model_output.shape or v1.dtype != model_output.dtype)):
            raise ValueError("the saved sample / model output of the first stage do not match this step's model output")
        prev = out if out is not None else torch.empty_like(model_output)
        if prev.dtype != model_output.dtype or prev.shape != model_output.shape or not prev.is_contiguous():
            raise ValueError(f"step(out=...) must be a contiguous {model_output.dtype} tensor of shape {tuple(model_output.shape)}")
        a = L.CsFmStepArgs()
        a.x_base, a.v2, a.v1 = base.data_ptr(), model_output.data_ptr(), v1.data_ptr() if v1 is not None else None
        a.c = float(plan.c)
        fill_io(a, base, model_output, prev, model_output.dtype)
        L.check(L.lib().cs_fm_general_step(C.byref(a), L.stream_ptr(model_output.device)))
        self.commit_plan(plan, sample, model_output)
        return (prev,) if not return_dict else SolverOutput(prev_sample=prev)
