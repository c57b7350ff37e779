"""FLUX-Kontext PPO rollout -- mirror of ``edit_ppo/denoise_diffusion.denoise_diffusion``
(edit_ppo/denoise_diffusion.py:11-176): same arguments, same return value

    (latents_output, pred_images, conds_{x, epsilon}, probs_, actions_, masks_)      (:170-174)
    (latents_output, pred_images)                            with use_naive_scheduler   (:175-176)

with trajectory records for steps ``i > 0`` only (:152-157).  ``pipe`` is driven through the same surface the
reference uses (``encode_prompt``, ``image_processor``, ``_pack_latents``, ``prepare_latents``, ``transformer``,
``_unpack_latents``, ``vae``): ``consolver_amd.pipeline.FluxKontextEditPipeline`` provides it on the HIP
components, and any object with that surface works.

Differences in mechanism, not in results:
* when ``pipe.transformer`` is the HIP DiT the joint input ``cat([latents, image_latents], 1)`` (:102) is never
  materialised (the embedder reads both buffers, ``image_latents=``) and the prediction comes back for the latent
  rows only (the reference slices ``noise_pred[:, :L]``, :145);
* height / width come from the noise tensor (``8 * noise.shape[-2:]``) instead of the hard-coded 1024 (:33-34) -- the same
  value for the reference's 128 x 128 latents;
* ``text`` may also be a dict ``{"prompt_embeds", "pooled_prompt_embeds"[, "text_ids"]}`` of precomputed embeddings
  (tokenizer assets are not part of this repo);
* ``gradient_checkpointing`` is rejected: the rollout is inference-only (``@torch.no_grad()``, :10).

Keyword-only extensions for the trainer (``ppo_flux.collect_rollout_flux``); each defaults to the path above:
* ``identical_inputs=True``: the caller states that the B rows of ``noise`` / ``text`` / ``image`` are copies of ONE sample, what the trainer
  feeds this function (``repeat_random_sample``, edit_ppo/data_processing.py:93-104).  It is checked on the device (``ValueError`` otherwise).
  The B trajectories then diverge only through their sampled actions, and step 0 of ``FMPPOScheduler`` takes none unless there is a scale action
  (scheduler_fmppo.py:413-414).  With the HIP DiT the forwards ``i < shared_steps`` (``2 if scaler_dim == 0 else 1``) run on row 0 and are
  broadcast; every returned tensor keeps its full-batch shape.  The reference image is then encoded once (row 0) and broadcast as well.
* ``baseline_scheduler``: a policy-free scheduler (``FlowMatchGeneralDiscreteScheduler(type="euler")``, the reference's ``pipe.scheduler``).  The
  same loop also advances a ONE-row trajectory from ``noise[:1]`` with it -- the ``use_naive_scheduler=True`` call of edit_ppo/train_ppo.py:290-300
  -- and the return value gains ``latents_base`` as a 7th element.  Its forward 0 is the rollout's forward 0; its forward 1 is the rollout's
  shared forward 1 when ``identical_inputs`` holds with ``scaler_dim == 0`` and step 0 of both schedulers returned the same bits (compared on the
  device); every other forward is its own, on one row.  Next to rows that may differ, row 0's reference image is encoded on its own (the VAE
  encoder's bits depend on the batch it runs in), so ``latents_base`` has the bits of that separate one-row call.
* ``decode=False`` skips the VAE decode and the PIL conversion: ``pred_images`` is ``None``.
* ``forward_batch_size``: at most that many rows per DiT call.
* ``stats``: a dict that receives ``forward_rows``, the rows of every DiT call in order.  Per rollout they add up to ``n B`` unshared and
  ``s + (n - s) B`` shared (``s = shared_steps``), plus ``n - 1`` (``n - s`` when forward 1 is reused) for the baseline's own forwards.
"""
import numpy as np
import torch

from . import _lib as L
from .tables import calculate_shift


@torch.no_grad()
def denoise_diffusion(scheduler, pipe, noise, text, image, cfg=2.5, num_inference_steps=28, gradient_checkpointing=False,
                      use_naive_scheduler=False, *, identical_inputs=False, baseline_scheduler=None, decode=True, forward_batch_size=None,
                      stats=None):
    if gradient_checkpointing:
        raise NotImplementedError("inference-only rollout: the denoiser is frozen")
    if use_naive_scheduler and (identical_inputs or baseline_scheduler is not None):
        raise ValueError("identical_inputs / baseline_scheduler belong to the policy rollout, not to use_naive_scheduler=True")
    L.require_cuda(noise, "noise")
    device, dtype = noise.device, noise.dtype
    guidance_scale = cfg
    height, width = noise.shape[-2] * pipe.vae_scale_factor, noise.shape[-1] * pipe.vae_scale_factor

    if isinstance(text, dict):
        prompt_embeds, pooled_prompt_embeds = text["prompt_embeds"].to(device), text["pooled_prompt_embeds"].to(device)
        text_ids = text.get("text_ids")
        if text_ids is None:
            text_ids = torch.zeros(prompt_embeds.shape[1], 3, device=device, dtype=dtype)
        batch_size = prompt_embeds.shape[0]
    else:
        if isinstance(text, str):
            text = [text]
        batch_size = len(text)
        prompt_embeds, pooled_prompt_embeds, text_ids = pipe.encode_prompt(prompt=text, prompt_2=None, device=device,
                                                                           num_images_per_prompt=1, max_sequence_length=512)

    image = pipe.image_processor.preprocess(image).to(device=device, dtype=dtype)

    dit = pipe.transformer
    native = getattr(dit, "is_consolver_hip", False)
    base = baseline_scheduler
    shared_steps = 0
    if identical_inputs and native and batch_size > 1:
        # the caller's statement is checked once per rollout (one small device->host read), as in rollout.denoise_diffusion
        rows_same = lambda t: t.shape[0] == 1 or bool(torch.equal(t[:1].expand_as(t), t))
        if not (rows_same(noise) and rows_same(prompt_embeds) and rows_same(pooled_prompt_embeds) and rows_same(image)
                and (isinstance(text, dict) or len(set(text)) == 1)):
            raise ValueError("identical_inputs=True, but the rows of noise / prompt embeddings are not copies of one sample")
        shared_steps = 2 if scheduler.config.scaler_dim == 0 else 1

    num_channels_latents = pipe.transformer.config.in_channels // 4
    noise = pipe._pack_latents(noise, batch_size, num_channels_latents, height // 8, width // 8)

    def prepare(img, lat):
        return pipe.prepare_latents(image=img, batch_size=lat.shape[0], num_channels_latents=num_channels_latents, height=height, width=width,
                                    dtype=dtype, device=device, generator=None, latents=lat)

    # The VAE encoder does not give one row the bits it gives that row inside a batch (its kernels are chosen by the batch's size), and a
    # forward can only stand for another whose inputs have the same bits.  So copies of one sample get ONE encode of row 0, broadcast; and
    # with a baseline next to rows that may differ, row 0 -- the baseline's reference image -- is encoded on its own, like the separate
    # one-row call it replaces, and the other rows together.
    if shared_steps or (base is not None and batch_size > 1 and image.shape[0] == 1):
        lat1, il1, latent_ids, image_ids = prepare(image[:1], noise[:1])
        initial_latents = noise if not shared_steps else lat1.expand(batch_size, -1, -1).contiguous()
        image_latents = None if il1 is None else il1.expand(batch_size, -1, -1).contiguous()
    elif base is not None and batch_size > 1:
        lat0, il0, latent_ids, image_ids = prepare(image[:1], noise[:1])
        lat_rest, il_rest, _, _ = prepare(image[1:], noise[1:])
        initial_latents = torch.cat([lat0, lat_rest])
        image_latents = None if il0 is None else torch.cat([il0, il_rest])
    else:
        initial_latents, image_latents, latent_ids, image_ids = prepare(image, noise)
    if image_ids is not None:
        latent_ids = torch.cat([latent_ids, image_ids], dim=0)

    guidance = None
    if pipe.transformer.config.guidance_embeds:
        guidance = torch.full([batch_size], guidance_scale, device=device, dtype=torch.float32)

    # sigma schedule with the resolution-dependent shift (:74-91; retrieve_timesteps == scheduler.set_timesteps(sigmas=, mu=))
    sigmas = np.linspace(1.0, 1 / num_inference_steps, num_inference_steps)
    image_seq_len = initial_latents.shape[1]
    cfgget = scheduler.config.get
    mu = calculate_shift(image_seq_len, cfgget("base_image_seq_len", 256), cfgget("max_image_seq_len", 4096),
                         cfgget("base_shift", 0.5), cfgget("max_shift", 1.15))
    scheduler.set_timesteps(sigmas=sigmas, mu=mu, device=device)
    timesteps = scheduler.timesteps

    if base is not None:
        base.set_timesteps(sigmas=sigmas, mu=mu, device=device)
        if not np.array_equal(np.asarray(base.timesteps.cpu()), np.asarray(timesteps.cpu())):
            raise ValueError("baseline_scheduler does not produce the rollout's timesteps: its forwards cannot be shared")
    # trajectory records of the steps i > 0 (:152-157), one list per field
    rec = {"x": [], "epsilon": [], "probs": [], "actions": [], "masks": []}
    record_prev = getattr(scheduler, "record_conds", None)
    if record_prev is not None and not use_naive_scheduler:
        scheduler.record_conds = True           # conds['epsilon'] is materialised only for the rollout
    # t.expand(B).to(dtype) / 1000 for every step at once: the per-step scalar stays a device slice (no host sync)
    ts_model = timesteps.to(dtype) / 1000
    latents = initial_latents
    n_lat_tokens = latents.size(1)
    common = dict(txt_ids=text_ids, img_ids=latent_ids, return_dict=False)
    forward_rows = []

    def forward(lat, i, lo=0, hi=batch_size):
        """the DiT on rows [lo, hi) of the conditioning, ``forward_batch_size`` rows at a time; ``lat`` holds those rows' latents"""
        step = forward_batch_size or (hi - lo)
        outs = []
        for s in range(lo, hi, step):
            e = min(s + step, hi)
            kw = dict(common, guidance=None if guidance is None else guidance[s:e], pooled_projections=pooled_prompt_embeds[s:e],
                      encoder_hidden_states=prompt_embeds[s:e], timestep=ts_model[i].expand(e - s))
            x, il = lat[s - lo:e - lo], None if image_latents is None else image_latents[s:e]
            if native and il is not None:
                # [latents | image_latents] read in place; the prediction comes back for the latent rows only
                outs.append(dit(hidden_states=x, image_latents=il, **kw)[0])
            elif il is not None:
                outs.append(dit(hidden_states=torch.cat([x, il], dim=1), **kw)[0][:, :n_lat_tokens])
            else:
                outs.append(dit(hidden_states=x, **kw)[0])
            forward_rows.append(e - s)
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    lat_base = latents[:1] if base is not None else None
    try:
        for i, t in enumerate(timesteps):
            if i < shared_steps:
                # every row carries the same latents: one row through the DiT, broadcast to the batch (the scheduler's records keep B rows)
                v1 = forward(latents[:1], i, 0, 1)
                velocity = v1.expand(batch_size, -1, -1).contiguous()
            else:
                velocity = forward(latents, i)
                v1 = velocity[:1]
            if base is not None:
                # forward 0 is the baseline's own forward 0 (same noise, same conditioning); forward 1 too while its input has the same bits
                # (no action at step 0 without a scale action: both schedulers take the same Euler step; checked, one small device->host read)
                reuse = i == 0 or (i == 1 and shared_steps == 2 and bool(torch.equal(lat_base, latents[:1])))
                v_base = v1 if reuse else forward(lat_base, i, 0, 1)
                lat_base = base.step(v_base, t, lat_base, return_dict=False)[0]
            stepped = scheduler.step(velocity, t, latents, return_dict=False)
            latents = stepped[0]
            if not use_naive_scheduler and i > 0:
                _, actions, probs, conds, masks = stepped
                for key, val in (("x", conds["x"]), ("epsilon", conds["epsilon"]), ("probs", probs), ("actions", actions), ("masks", masks)):
                    rec[key].append(val.unsqueeze(1))
    finally:
        if record_prev is not None:
            scheduler.record_conds = record_prev
    latents_output = latents
    if stats is not None:
        stats["forward_rows"] = forward_rows

    # decode (:163-166)
    pred_images = None
    if decode:
        lat = pipe._unpack_latents(latents, height, width, pipe.vae_scale_factor)
        lat = (lat / pipe.vae.config.scaling_factor) + pipe.vae.config.shift_factor
        pred_images = pipe.vae.decode(lat, return_dict=False)[0]
        pred_images = pipe.image_processor.postprocess(pred_images, output_type="pil")

    if use_naive_scheduler:
        return latents_output, pred_images
    stacked = {key: torch.cat(vals, dim=1) for key, vals in rec.items()}
    out = (latents_output, pred_images, {"x": stacked["x"], "epsilon": stacked["epsilon"]}, stacked["probs"], stacked["actions"], stacked["masks"])
    return out if base is None else out + (lat_base,)
