"""Writes tests/golden/flux_ppo_update.npz: what the FLUX-Kontext PPO trainer (edit_ppo/train_ppo.py:247-421) computes between the rollout
and the next rollout, evaluated by the reference's own code on the CPU.

Build container only: the reference tree is imported read-only through ``oracle/ref_stubs.py``; nothing of it is copied, only the arrays it
computes are stored.

    python tools/make_flux_ppo_golden.py

(a) ``u{i}_*``: the policy update.  The reference's edit_ppo ``FactorNetPPO`` (softmax(logits / 0.01), no input scale, the mu grid) under
    torch autograd with the loop's loss (:356-379), ``clip_grad_norm_`` and ``torch.optim.AdamW`` for two epochs on one batch, laid out like
    ``sd_ppo_update.npz`` (oracle/make_golden.py): ``_cfg`` = [order_dim, scaler_dim, mu_dim, K, H, R], ``_hyper``, ``_x``, ``_actions``,
    ``_old_probs``, ``_adv``, ``_w_{name}`` and per epoch ``_e{ep}_loss``, ``_e{ep}_grad_{name}``, ``_e{ep}_norm``, ``_e{ep}_after_{name}``.
    The last layer is scaled so that the T = 0.01 softmax is saturated in some rows and not in others: ``_sat_share`` is the share of
    probabilities below 1.19e-7 (fp32 epsilon, where ``Categorical``'s clamp acts), ``_sat_rows`` the share of rows holding one.
    Even rows replay the most likely bin, odd rows a random one (mostly a probability that underflowed: the ``1e-9`` of the log decides).
(b) ``a{i}_*``: the advantage expression of :326-341 in torch: ``_rewards`` [B, 1], ``_base`` (the python float ``.item()`` hands over),
    ``_clip_hi``, ``_n``, ``_masks`` [B (n-1), A], ``_out``.  ``a_cases`` lists (B, n, A, base case) per index.
(c) ``pack_in`` [2, 64, 64] / ``pack_out``: the reference's ``_pack_latents`` (edit_ppo/pipeline.py:589-594, executed from its source, the
    module itself needs diffusers) applied to an ALREADY packed tensor, as edit_ppo/denoise_diffusion.py:51 does with a stored teacher noise.
"""
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "flux_ppo_update.npz")
UPDATE_CASES = [(2, 0, 0, 11, 32, 40), (3, 1, 1, 7, 24, 21), (2, 0, 0, 11, 32, 1)]        # order_dim, scaler_dim, mu_dim, K, H, R
LAST_LAYER_SCALE = (0.04, 0.022, 0.04)      # logits differ by ~0.1: x 100 -> some rows saturate, some do not
ADV_SHAPES = [(10, 2, 1), (10, 5, 1), (5, 3, 3), (2, 2, 1), (300, 4, 2)]
ADV_BASES = ("below", "above", "equal", "hundred", "over_hi", "flat_below", "flat_above", "low_hi")
F32_EPS = 1.1920929e-07


def reference_pack_latents():
    """the reference's ``_pack_latents`` static method, compiled from its source file"""
    from oracle import ref_stubs
    path = os.path.join(ref_stubs.REF_ROOT, "edit_ppo", "pipeline.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "_pack_latents")
    fn.decorator_list = []
    ns = {}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["_pack_latents"]


def main():
    sys.path.insert(0, ROOT)
    from oracle import ref_stubs
    ref_stubs.install("flux")
    import torch
    torch.set_num_threads(1)
    with ref_stubs.quiet():
        from factor_net_ppo import FactorNetPPO
    fx = {}

    # ---------------------------------------------------------------- (a) policy update
    for ui, (o, sc, mu, K, H, R) in enumerate(UPDATE_CASES):
        with ref_stubs.quiet():
            net = FactorNetPPO(hidden_dim=H, num_actions=K, order_dim=o, scaler_dim=sc, mu_dim=mu)
        g = torch.Generator().manual_seed(5000 + ui)
        with torch.no_grad():
            for name, p in net.named_parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.5 / max(1.0, float(p.shape[-1]) ** 0.5) * 4.0)
            net.mlp[4].weight.mul_(LAST_LAYER_SCALE[ui])
            net.mlp[4].bias.mul_(0.5 * LAST_LAYER_SCALE[ui])
        w0 = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
        A = o + sc + mu - 1
        rng = np.random.default_rng(5100 + ui)
        # conds["x"] of the FLUX scheduler: (sigma_i, sigma_{i+1}) rounded through bf16 (scheduler_fmppo.py:383)
        s0 = rng.uniform(0.25, 1.0, size=(R, 1))
        x = torch.from_numpy(np.concatenate([s0, s0 * rng.uniform(0.3, 0.95, size=(R, 1))], 1).astype(np.float32)).to(torch.bfloat16).float().numpy()
        conds = {"x": torch.from_numpy(x)}
        av = net.action_values.numpy()
        with torch.no_grad():
            p0 = net.forward_(conds).numpy()                                   # [R, A, K]
        idx = rng.integers(0, K, size=(R, A))
        idx[0::2] = p0.argmax(-1)[0::2]
        actions = np.take_along_axis(np.broadcast_to(av, (R, A, K)), idx[..., None], 2)[..., 0].astype(np.float32)
        with torch.no_grad():
            cur, _ = net.get_action_probs(conds, torch.from_numpy(actions))
        old = np.clip(cur.numpy() * rng.uniform(0.55, 1.6, size=(R, A)), 1e-8, 1.0).astype(np.float32)
        adv = (rng.standard_normal((R, 1)) * 1.5).astype(np.float32) * (rng.random((R, A)) > 0.25).astype(np.float32)
        sat = p0 < F32_EPS
        fx[f"u{ui}_sat_share"], fx[f"u{ui}_sat_rows"] = np.float64(sat.mean()), np.float64(sat.any(axis=(1, 2)).mean())
        if R > 1:
            assert 0.0 < sat.any(axis=(1, 2)).mean() < 1.0, (ui, sat.any(axis=(1, 2)).mean())
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)
        clip_range, entropy_coef, max_norm = 0.2, 0.01, 1.0
        for ep in range(2):
            curr_probs, entropy = net(conds, torch.from_numpy(actions))
            log_probs = (curr_probs + 1e-9).log().sum(dim=1).unsqueeze(1)
            old_log_probs = (torch.from_numpy(old) + 1e-9).log().sum(dim=1).unsqueeze(1)
            ratio = (log_probs - old_log_probs).exp()
            clipped_ratio = torch.clamp(ratio, 1 - clip_range, 1 + clip_range)
            a = torch.from_numpy(adv)
            loss = (-torch.min(a * ratio, a * clipped_ratio)).mean() + (-entropy_coef * entropy.mean())
            loss.backward()
            fx[f"u{ui}_e{ep}_loss"] = np.float32(loss.item())
            for k, prm in net.named_parameters():
                fx[f"u{ui}_e{ep}_grad_{k}"] = prm.grad.detach().numpy().copy()
            fx[f"u{ui}_e{ep}_norm"] = np.float32(torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm).item())
            opt.step()
            opt.zero_grad()
            for k, v in net.state_dict().items():
                fx[f"u{ui}_e{ep}_after_{k}"] = v.detach().numpy().copy()
        fx[f"u{ui}_cfg"] = np.asarray([o, sc, mu, K, H, R], np.int64)
        fx[f"u{ui}_hyper"] = np.asarray([1e-3, 0.9, 0.999, 1e-2, 1e-8, clip_range, entropy_coef, max_norm], np.float64)
        fx[f"u{ui}_x"], fx[f"u{ui}_actions"], fx[f"u{ui}_old_probs"], fx[f"u{ui}_adv"] = x, actions, old, adv
        for k, v in w0.items():
            fx[f"u{ui}_w_{k}"] = v
        print(f"update case {ui}: saturated share {sat.mean():.3f}, rows with one {sat.any(axis=(1, 2)).mean():.3f}, "
              f"losses {fx[f'u{ui}_e0_loss']:.5f} {fx[f'u{ui}_e1_loss']:.5f}, norms {fx[f'u{ui}_e0_norm']:.4f} {fx[f'u{ui}_e1_norm']:.4f}")

    # ---------------------------------------------------------------- (b) advantages
    torch.set_grad_enabled(False)
    cases = [(B, n, A, bc) for (B, n, A) in ADV_SHAPES for bc in ADV_BASES] + [(1, 4, 2, "below")]
    for ai, (B, num_inference, A, bc) in enumerate(cases):
        rng = np.random.default_rng(6000 + ai)
        r = rng.normal(20, 4, (B, 1)).astype(np.float32)
        if bc.startswith("flat"):
            r[:] = 20.5                       # sums of up to 300 of them are exact in fp32: mean = 20.5 and std = 0 in any summation order
        rewards = torch.from_numpy(r)
        mean, clip_hi = float(rewards.mean()), 100.0
        rewards_base = {"below": mean - 3.0, "above": mean + 2.5, "equal": mean, "hundred": 100.0, "over_hi": 150.0, "flat_below": 19.0,
                        "flat_above": 21.0, "low_hi": mean + 6.0}[bc]
        if bc == "low_hi":
            clip_hi = float(np.float32(mean + 4.0))      # the cap below the base: clip_hi wins
        masks = torch.from_numpy((rng.random((B * (num_inference - 1), A)) > 0.3).astype(np.float32))
        advantages = (rewards - rewards.mean().clip(rewards_base, clip_hi)) / (rewards.std() + 1e-8)
        advantages = advantages.repeat(1, (num_inference - 1)).reshape(advantages.shape[0] * (num_inference - 1), -1)
        advantages = advantages * masks
        fx[f"a{ai}_rewards"], fx[f"a{ai}_base"], fx[f"a{ai}_clip_hi"] = r, np.float64(rewards_base), np.float64(clip_hi)
        fx[f"a{ai}_n"], fx[f"a{ai}_masks"], fx[f"a{ai}_out"] = np.int64(num_inference), masks.numpy(), advantages.numpy()
    fx["a_cases"] = np.asarray([f"{B},{n},{A},{bc}" for B, n, A, bc in cases])

    # ---------------------------------------------------------------- (c) the pack of a packed tensor
    pack = reference_pack_latents()
    S = 16
    packed = torch.from_numpy(np.random.default_rng(7).standard_normal((2, (S // 2) ** 2, 64)).astype(np.float32)).to(torch.bfloat16).float()
    fx["pack_in"], fx["pack_out"] = packed.numpy(), pack(packed, 2, 16, S, S).contiguous().numpy()
    np.savez_compressed(OUT, **fx)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
