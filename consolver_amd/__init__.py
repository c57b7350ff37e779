"""consolver_amd -- MI355X-native ConsistencySolver sampling engine (hot path only).

Public surface mirrors the reference's plugin API for this path:
``PPOScheduler`` (scheduler_ppo.py), ``FMPPOScheduler`` (edit_ppo/scheduler_fmppo.py),
``FactorNetPPO`` (factor_net_ppo.py / edit_ppo/factor_net_ppo.py) and the denoiser behind
``unet(latents, t, encoder_hidden_states=..., return_dict=False)[0]``.  Everything computes in
hand-written HIP kernels behind ``include/consolver_hip.h``; there is no CPU fallback.
"""
from .scheduling_ppo import PPOScheduler, SolverOutput  # noqa: F401
from ._scheduler_base import HAVE_DIFFUSERS, SolverConfig  # noqa: F401
from .scheduling_fmppo import FMPPOScheduler  # noqa: F401
from .scheduling_fm import FlowMatchGeneralDiscreteScheduler  # noqa: F401
from .factor_net import FactorNetPPO, FluxFactorNetPPO  # noqa: F401
from .scheduling_dpm import DPMSolverMultistepScheduler, SD15_MULTISTEP_DPM_KWARGS  # noqa: F401
from .scheduling_unipc import UniPCMultistepScheduler, SD15_UNIPC_KWARGS  # noqa: F401
from .scheduling_amed import AMEDSolverScheduler, SD15_AMED_KWARGS  # noqa: F401
from .scheduling_deis import DEISMultistepScheduler, SD15_DEIS_KWARGS  # noqa: F401
from .scheduling_pndm import PNDMScheduler, SD15_PNDM_KWARGS  # noqa: F401
from .fid import FIDStatistics, HipFIDInception, compute_fid, frechet_distance, load_fid_inception  # noqa: F401
from .ppo_flux import (as_rollout_noise, collect_rollout_flux, compute_advantages_flux, decode_latents_flux,  # noqa: F401
                       train_iteration_flux)

__version__ = "0.1.0"
