"""FLUX-Kontext PPO trainer body: shared-prefix rollout -> decode -> reward -> baseline advantage -> policy update.

The FLUX twin of ``ppo.py``: mirror of the loop body of edit_ppo/train_ppo.py:247-421 with the reference's names.

* ``as_rollout_noise`` = what edit_ppo/denoise_diffusion.py:51 does to a stored teacher noise (see its docstring: a finding, not a choice).
* ``decode_latents_flux`` = edit_ppo/utils.py:11-27 on ``vae.flux_decode_latents``, sized by the pipe instead of the constant 1024.
* ``compute_advantages_flux`` = :326-341.  NOT the SD formula (train_ppo.py:376-390, ``ppo.compute_advantages``): the batch mean is raised to
  the reward of a one-row plain-Euler rollout from the same noise (``rewards.mean().clip(rewards_base, 100.0)``) and there is no ``x 10``.
  ``cs_ppo_advantages_baseline`` reads ``rewards_base`` from device memory, so no host sync sits between reward and update (the reference
  pulls it to the host with ``.item()``, :324).
* ``collect_rollout_flux`` = :285-347 for one batch: ONE ``rollout_flux.denoise_diffusion`` call advances the B policy trajectories and the
  baseline trajectory (the reference makes two calls, :290-311), nothing is decoded to PIL, the latents are decoded once each (the reference
  decodes the prediction twice and B copies of the teacher latents, :313-315 and denoise_diffusion.py:163-166).
* ``train_iteration_flux`` = :258-389: ``repeat_random_sample_flux`` -> step count from ``range(2, 6)`` drawn by rank 0 and broadcast
  (:275-283) -> ``collect_rollout_flux`` -> ``ppo_epochs`` calls of ``ppo.PolicyTrainer.step`` (reused unchanged: ``cs_ppo_policy_grads``
  reads the FLUX net's ``inv_temperature`` = 100 and unit input scale from its ``CsFactorNet``).

Everything runs in the HIP library; there is no CPU fallback.
"""
import random

import torch

from . import _lib as L
from .ppo import calculate_reward
from .rollout_flux import denoise_diffusion
from .vae import flux_decode_latents

NUM_INFERENCE_CHOICES = tuple(range(2, 6))          # edit_ppo/train_ppo.py:277


def as_rollout_noise(noise, latent_channels=16, S=None, noise_layout="reference"):
    """The dataset's PACKED teacher noise ``[B, L, 4 C]`` (edit_pretrain/generate.py:81 stores the packed initial latents, and so does
    ``generate_flux_teacher``) -> the ``[B, C, S, S]`` tensor ``rollout_flux.denoise_diffusion`` packs.  A 4-D tensor passes through.

    ``noise_layout="reference"`` (default): the plain view of the stored memory as ``[B, C, S, S]``.  The reference hands the stored tensor
    to ``denoise_diffusion``, which calls ``pipe._pack_latents(noise, B, 16, 128, 128)`` on it (edit_ppo/denoise_diffusion.py:51,
    pipeline.py:589-594): a ``view`` of the ALREADY packed tensor as ``[B, 16, 64, 2, 64, 2]`` followed by the pack permutation.  The student
    therefore does not start from the teacher's initial latents but from a fixed permutation of their elements (still unit Gaussian noise, but
    another sample than the one the teacher latents it is rewarded against were generated from).  This layout reproduces that element order
    exactly, because the published solver was trained with it.

    ``noise_layout="packed"``: ``unpack_latents`` of the stored tensor, so the rollout's pack restores it unchanged and the student starts from
    the teacher's own initial latents."""
    if noise.dim() == 4:
        return noise
    if noise.dim() != 3:
        raise ValueError(f"noise must be [B, C, S, S] or packed [B, L, 4 C], got {tuple(noise.shape)}")
    B, Ltok, ch = noise.shape
    if ch != 4 * latent_channels:
        raise ValueError(f"packed noise has {ch} channels per token, expected 4 x {latent_channels}")
    side = int(round(Ltok ** 0.5))
    if S is None:
        S = 2 * side
    if (S // 2) ** 2 != Ltok or S % 2:
        raise ValueError(f"{Ltok} tokens do not tile a {S} x {S} latent")
    if noise_layout == "reference":
        return noise.contiguous().view(B, latent_channels, S, S)
    if noise_layout == "packed":
        from .flux import unpack_latents
        return unpack_latents(noise.contiguous(), 8 * S, 8 * S, 8)
    raise ValueError(f"unknown noise_layout {noise_layout!r}: 'reference' or 'packed'")


def decode_latents_flux(pipe, packed, batch_size=8):
    """edit_ppo/utils.py:11-27: packed ``[B, L, 64]`` latents -> images ``[B, 3, 8 S, 8 S]`` in [0, 1].  The size is the pipe's VAE's."""
    side = pipe.vae_scale_factor * pipe.vae.config.sample_size
    return flux_decode_latents(pipe.vae, packed.to(torch.float16), height=side, width=side, vae_scale_factor=pipe.vae_scale_factor,
                               batch_size=batch_size)


def compute_advantages_flux(rewards, rewards_base, masks, num_inference_steps, clip_hi=100.0):
    """edit_ppo/train_ppo.py:326-341: rewards [B, 1], rewards_base (a device tensor holding one value, or a number) ->
    ``(r - clamp(mean(r), rewards_base, clip_hi)) / (std(r) + 1e-8)`` tiled over the n - 1 recorded steps and masked, [B (n-1), A]."""
    L.require_cuda(rewards, "rewards")
    r = rewards.reshape(-1).to(torch.float32).contiguous()
    if isinstance(rewards_base, torch.Tensor):
        if rewards_base.numel() != 1:
            raise ValueError("rewards_base holds one value (the reward of the one-row baseline rollout)")
        base = rewards_base.reshape(1).to(device=r.device, dtype=torch.float32).contiguous()
    else:
        base = torch.full((1,), float(rewards_base), dtype=torch.float32, device=r.device)
    B, steps = r.shape[0], num_inference_steps - 1
    m = masks.reshape(B * steps, -1).to(torch.float32).contiguous()
    out = torch.empty_like(m)
    L.check(L.lib().cs_ppo_advantages_baseline(L.ptr(r), L.ptr(base), float(clip_hi), B, steps, m.shape[1], L.ptr(m), L.ptr(out),
                                               L.stream_ptr(r.device)))
    return out


def collect_rollout_flux(pipe, noise_scheduler, base_scheduler, noise, text, image, target_latents, cfg=2.5, num_inference_steps=4,
                         reward_type="image_psnr", reward_model=None, reward_model_processor=None, decode_batch_size=8,
                         identical_inputs=False, noise_layout="reference", forward_batch_size=None, clip_hi=100.0):
    """edit_ppo/train_ppo.py:285-347 for one batch.  ``noise``: ``[B, 16, S, S]`` or the dataset's packed ``[B, L, 64]`` (``as_rollout_noise``);
    ``target_latents``: the teacher's packed final latents ``[B, L, 64]``; ``text``: prompts or a dict of precomputed embeddings; ``image``: the
    reference images.  ``identical_inputs=True``: the B rows are copies of one sample (``repeat_random_sample_flux``): the rollout shares the
    DiT forwards whose inputs cannot differ yet and the teacher image is decoded once.
    Returns dict(conds, actions, probs, masks, advantages, rewards, model_pred, rewards_base [1, 1] on the device, latents_base, forward_rows)
    with the records flattened to ``[B (n-1), ...]``."""
    n = num_inference_steps
    vae = pipe.vae
    noise = as_rollout_noise(noise, vae.config.latent_channels, vae.config.sample_size, noise_layout)
    stats = {}
    model_pred, _, conds, probs, actions, masks, latents_base = denoise_diffusion(
        noise_scheduler, pipe, noise, text, image, cfg=float(cfg), num_inference_steps=n, identical_inputs=identical_inputs,
        baseline_scheduler=base_scheduler, decode=False, forward_batch_size=forward_batch_size, stats=stats)
    B = model_pred.shape[0]
    pred_img = decode_latents_flux(pipe, model_pred, decode_batch_size)
    pred_img_base = decode_latents_flux(pipe, latents_base, 1)
    if identical_inputs and B > 1:
        target_one = decode_latents_flux(pipe, target_latents[:1], 1)
        # calculate_dino_reward / calculate_clip_reward take one shared target as [1,3,H,W]
        target_img = target_one if reward_type in ("dino", "clip") else target_one.expand(B, -1, -1, -1).contiguous()
    else:
        target_img = decode_latents_flux(pipe, target_latents, decode_batch_size)
        target_one = target_img[:1]
    rewards = calculate_reward(reward_type, reward_model, reward_model_processor, pred_img, target_img, noise.device)
    rewards_base = calculate_reward(reward_type, reward_model, reward_model_processor, pred_img_base, target_one, noise.device)
    flat = lambda v: v.reshape(v.shape[0] * (n - 1), *v.shape[2:])
    conds = {k: flat(v) for k, v in conds.items()}
    actions, probs, masks = (t.reshape(B * (n - 1), -1) for t in (actions, probs, masks))
    advantages = compute_advantages_flux(rewards, rewards_base, masks, n, clip_hi=clip_hi)
    return dict(conds=conds, actions=actions, probs=probs, masks=masks, advantages=advantages, rewards=rewards, model_pred=model_pred,
                rewards_base=rewards_base, latents_base=latents_base, forward_rows=stats["forward_rows"])


def draw_num_inference_steps(dist=None, rng=None, device="cpu", choices=NUM_INFERENCE_CHOICES):
    """edit_ppo/train_ppo.py:275-283: rank 0 draws the step count, every other rank holds 0, and an int32 broadcast from rank 0 hands every
    rank the same number (the ranks' policy gradients are averaged, so they must describe rollouts of the same length)."""
    rng = rng or random
    if dist is None:
        return rng.choice(list(choices))
    n = rng.choice(list(choices)) if dist.get_rank() == 0 else 0
    t = torch.tensor([n], dtype=torch.int32, device=device)
    dist.broadcast(t, src=0)
    return int(t.item())


def train_iteration_flux(trainer, pipe, noise_scheduler, base_scheduler, batch, cfg=2.5, num_inference_steps=None, ppo_epochs=4,
                         reward_type="image_psnr", dist=None, rng=None, share_identical=True, reward_model=None, reward_model_processor=None,
                         text_embeds=None, noise_layout="reference", forward_batch_size=None, decode_batch_size=8):
    """One iteration of the loop body (edit_ppo/train_ppo.py:258-389).  ``batch`` = (image, text, noise, teacher latents, reference image) as
    ``FluxTeacherPairDataset`` collates it (noise and teacher latents packed ``[B, L, 64]``, reference image in [0, 1]), already on the GPU.  ``text_embeds``: a dict
    ``{"prompt_embeds" [B, T, D], "pooled_prompt_embeds" [B, P]}`` of per-item embeddings used in place of the prompts (they follow the item
    that was picked).  With ``dist`` rank 0 draws the step count for all ranks and the gradients are averaged over the ranks
    (``launch.average_gradients`` inside ``PolicyTrainer.step``).
    Returns dict(loss, norm, reward, reward_base, num_inference_steps, forward_rows, index (the item that was repeated), rollout)."""
    from .ppo_data import repeat_random_sample_flux
    _, text, noise, tch, ref, i = repeat_random_sample_flux(batch, return_index=True)
    B = noise.shape[0]
    if text_embeds is not None:
        text = {k: v[i:i + 1].expand(B, *v.shape[1:]).contiguous() if (torch.is_tensor(v) and v.dim() > 1 and v.shape[0] == B and k != "text_ids")
                else v for k, v in text_embeds.items()}
    n = num_inference_steps or draw_num_inference_steps(dist, rng, noise.device)
    # the dataset's reference image is in [0, 1]; the reference's image_processor.preprocess normalises such a tensor to [-1, 1]
    # (do_normalize), ours passes tensors through
    ref = ref * 2 - 1
    # the B rows are copies of one sample by construction (data_processing.py:93-104): share what cannot differ
    roll = collect_rollout_flux(pipe, noise_scheduler, base_scheduler, noise, text, ref, tch, cfg=cfg, num_inference_steps=n,
                                reward_type=reward_type, reward_model=reward_model, reward_model_processor=reward_model_processor,
                                decode_batch_size=decode_batch_size, identical_inputs=share_identical, noise_layout=noise_layout,
                                forward_batch_size=forward_batch_size)
    loss = norm = None
    for _ in range(ppo_epochs):
        loss, norm = trainer.step(roll["conds"], roll["actions"], roll["probs"], roll["advantages"], dist=dist)
    return dict(loss=loss, norm=norm, reward=roll["rewards"].mean(), reward_base=roll["rewards_base"].reshape(()), num_inference_steps=n,
                forward_rows=roll["forward_rows"], index=i, rollout=roll)
