"""Writes tests/golden/flux_true_cfg.npz: the Kontext edit loop under TRUE classifier-free guidance (edit_ppo/pipeline.py:1074-1119: two DiT
branches, ``noise_pred = neg + true_cfg_scale * (noise_pred - neg)`` in the model dtype, then ``scheduler.step``) run on the CPU with the
reference's own schedulers around a closed-form bf16 "DiT".

Build container only: the reference tree is imported read-only through ``oracle/ref_stubs.py``; nothing of it is copied, only the arrays it
computes are stored.  The loop below is this tree's restatement of those lines; the schedulers are the reference's classes.

    python tools/make_flux_true_cfg_golden.py

Sizes: B = 2, 24 tokens x 64 (a 4 x 6 packed grid), n = 4 steps, true_cfg_scale = 4.  Schedulers: ``fmppo`` (FMPPOScheduler, order 2, the policy's
draws replaced by recorded indices) and the four FlowMatchGeneralDiscreteScheduler types.  Per scheduler ``{name}_lat`` [n + 1, B, 24, 64]: the
initial latents and the latents after every step (bf16 values stored as fp32); ``{name}_sigmas`` / ``{name}_timesteps``; for fmppo also ``fmppo_idx``
[n - 1 draws, B, 1] and the policy weights ``fmppo_w_*``.  ``mu``, ``scale`` and ``names`` are shared.

The two branches (``dit``): pos = 0.9 tanh(x) + 0.1 sigma, neg = 0.7 tanh(x) - 0.05, evaluated in fp32 on the bf16 latents and the bf16
``timestep / 1000`` the loop hands over, rounded to bf16.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "flux_true_cfg.npz")
NAMES = ("fmppo", "euler", "heun", "dpm-solver", "dpm-solver-multistep")
B, TOKENS, N, SCALE = 2, 24, 4, 4.0


def dit(torch, x, sigma, negative):
    """the closed-form branches; x bf16 [B, L, 64], sigma bf16 [B] -> bf16"""
    th = torch.tanh(x.float())
    v = (0.7 * th - 0.05) if negative else (0.9 * th + 0.1 * sigma.float()[:, None, None])
    return v.to(torch.bfloat16)


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_stubs
    ref_stubs.install("flux")
    import torch
    torch.set_num_threads(1)
    torch.set_grad_enabled(False)
    from oracle.make_golden import ForcedMultinomial
    from consolver_amd.tables import calculate_shift
    with ref_stubs.quiet():
        from scheduler_fmppo import FMPPOScheduler
        from scheduler_fm import FlowMatchGeneralDiscreteScheduler
    mu = calculate_shift(TOKENS, 256, 4096, 0.5, 1.15)
    fx = {"names": np.asarray(NAMES), "mu": np.float64(mu), "scale": np.float32(SCALE)}
    x0 = torch.from_numpy(np.random.default_rng(8100).standard_normal((B, TOKENS, 64)).astype(np.float32)).to(torch.bfloat16)
    for name in NAMES:
        with ref_stubs.quiet():
            if name == "fmppo":
                s = FMPPOScheduler(shift=3.0, use_dynamic_shifting=True, order_dim=2, scaler_dim=0, mu_dim=0,
                                   factor_net_kwargs=dict(hidden_dim=32, num_actions=11))
                g = torch.Generator().manual_seed(8200)
                for p in s.factor_net.parameters():
                    p.copy_(torch.randn(p.shape, generator=g) * 0.05)
                for k, v in s.factor_net.state_dict().items():
                    fx[f"fmppo_w_{k}"] = v.numpy().copy()
            else:
                s = FlowMatchGeneralDiscreteScheduler(shift=3.0, use_dynamic_shifting=True, type=name)
        s.set_timesteps(sigmas=np.linspace(1.0, 1 / N, N), mu=mu)
        s.set_begin_index(0)
        fx[f"{name}_sigmas"], fx[f"{name}_timesteps"] = s.sigmas.numpy().copy(), s.timesteps.numpy().copy()
        latents, traj = x0.clone(), [x0.float().numpy().copy()]
        with ForcedMultinomial(torch, np.random.default_rng(8300)) as fm, ref_stubs.quiet():
            for t in s.timesteps:                                             # edit_ppo/pipeline.py:1074-1119, restated
                timestep = t.expand(latents.shape[0]).to(latents.dtype)
                noise_pred = dit(torch, latents, timestep / 1000, negative=False)
                neg_noise_pred = dit(torch, latents, timestep / 1000, negative=True)
                noise_pred = neg_noise_pred + SCALE * (noise_pred - neg_noise_pred)
                assert noise_pred.dtype == torch.bfloat16
                latents = s.step(noise_pred, t, latents, return_dict=False)[0]
                assert latents.dtype == torch.bfloat16
                traj.append(latents.float().numpy().copy())
        fx[f"{name}_lat"] = np.stack(traj)
        if name == "fmppo":
            fx["fmppo_idx"] = np.stack([l.reshape(B, -1) for l in fm.log])
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
