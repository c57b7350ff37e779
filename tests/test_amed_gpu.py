"""GPU tests of AMEDSolverScheduler: the kernel path (cs_dpm_multistep_step with the scaled direction terms) against the reference plugin's own output
(tests/golden/amed_solver.npz), and the engine around it."""
import json
import os

import numpy as np
import pytest
import torch

from consolver_amd import AMEDSolverScheduler, SD15_AMED_KWARGS
from consolver_amd.engine import SDSamplingEngine
from consolver_amd.synth import synthetic_prompt_embeds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCHEDULES = os.path.join(GOLDEN, "amed_schedules.json")
REDUCED = dict(layers_per_block=1, sample_size=16)


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("n", [4, 8])
def test_kernel_path_reproduces_the_plugin(n):
    """every step of the golden run, fed the golden's own sample and model output (fp32, [3, 5, 67]); the scheduler keeps its own history: ``prev`` < 1e-6 rel-L2"""
    g = np.load(os.path.join(GOLDEN, "amed_solver.npz"))
    with open(SCHEDULES, "r", encoding="utf-8") as f:
        t = json.load(f)[str(n)]
    s = AMEDSolverScheduler(**SD15_AMED_KWARGS)
    s.scale_dirs, s.scale_times = t["grad_scale"], t["time_scale"]
    s.set_timesteps(num_inference_steps=n, device=DEV, timesteps=t["amed"])
    assert s.timesteps.is_cuda and np.array_equal(s.timesteps.cpu().numpy(), g[f"n{n}_timesteps"])
    for i, ts in enumerate(s.timesteps):
        x, e = (torch.from_numpy(g[f"n{n}_s{i}_{k}"]).to(DEV) for k in ("x", "eps"))
        prev = s.step(e, ts, x, return_dict=False)[0]
        err = rel_l2(prev.cpu().numpy(), g[f"n{n}_s{i}_prev"])
        print("amed kernel vs plugin", n, i, err)
        assert prev.dtype == torch.float32 and err < 1e-6, (i, err)
    assert s.step_index == n


def test_engine_runs_the_table_and_the_unet_sees_the_rescaled_timesteps():
    from tests._models import get_unet
    unet, _ = get_unet(REDUCED, seed=5)
    g = np.load(os.path.join(GOLDEN, "amed_solver.npz"))
    B, n = 2, 4
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half().to(DEV), synthetic_prompt_embeds(B, seed=1002).half().to(DEV)
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(46)).half().to(DEV)
    sch = AMEDSolverScheduler(**SD15_AMED_KWARGS).load_schedules(SCHEDULES)
    eng = SDSamplingEngine(unet, sch, guidance_scale=3.0)
    lat = eng.generate(pe, ne, latents=noise, num_inference_steps=n).clone()
    assert lat.shape == (B, 4, 16, 16) and bool(torch.isfinite(lat).all())
    assert np.array_equal(eng._t_dev.cpu().numpy(), g["n4_timesteps"].astype(np.float32))       # what the UNet is called with: the odd positions moved
    assert sch.step_index == n and len(eng._bufs["ring"]) == 2
    graph = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True)
    assert torch.equal(lat, graph)
    with pytest.raises(ValueError):
        eng.generate(pe, ne, latents=noise, num_inference_steps=5)             # no table of 5 steps
