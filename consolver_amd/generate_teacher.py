"""Teacher-pair generator: prompts -> 40-step Multistep-DPM-Solver latents -> ``{rank}_{idx:08d}.txt/.png`` + ``noise_*.pth`` + ``latent_*.pth``.

Mirror of gen_pretrain/generate_data.py:144-258 (readme "Generate training samples") on the native engine: the scheduler of
its ``load_pipeline`` (:86-91, ``scheduling_dpm.SD15_MULTISTEP_DPM_KWARGS``), 40 steps at CFG 3, batches of 24, per-batch
generator seed ``seed + batch_idx`` (:164) and the file set ``ppo_data.TeacherPairDataset`` reads (:189-213).  One process
per GPU, contiguous shards (``launch.shard_bounds``), no data-path collective.

    python -m torch.distributed.run --nproc-per-node 8 -m consolver_amd.generate_teacher --prompt-cache prompts.safetensors \\
        --unet unet.safetensors --vae vae.safetensors --generation_path train_coco/

The reference seeds every device alike, so the same batch index draws the same noise on every rank; ``--seed-stride S``
adds ``rank * S`` to the seed (default 0: the reference's behaviour).
"""
import argparse
import time

import torch

from . import evaluation, launch, ppo_data
from .generate import _load_sd, prepare_latents


def generate_teacher_pairs(prompts, prompt_embeds, negative_prompt_embeds, engine, generation_path, rank=0, world=1, num_inference_steps=40,
                           batch_size=24, seed=0, seed_stride=0, device=None, use_graph=False):
    """this rank's shard of ``prompts`` (generate_data.py:232-236 with ``launch.shard_bounds``), in batches (:159-213).  ``engine``: an
    ``SDSamplingEngine`` with a VAE around the teacher's scheduler.  Returns the number of pairs written."""
    if engine.vae is None:
        raise RuntimeError("the teacher-pair generator decodes every latent: SDSamplingEngine(..., vae=...)")
    lo, hi = launch.shard_bounds(len(prompts), world, rank)
    prompts, pe_all = prompts[lo:hi], prompt_embeds[lo:hi]
    ne_all = negative_prompt_embeds[lo:hi] if negative_prompt_embeds is not None else None
    device = device or torch.device("cuda", torch.cuda.current_device())
    S = engine.unet.config["sample_size"]
    shape = (engine.unet.config["in_channels"], S, S)
    done = 0
    for batch_idx, start in enumerate(range(0, len(prompts), batch_size)):
        batch = prompts[start:start + batch_size]
        pe = pe_all[start:start + batch_size].to(device)
        ne = ne_all[start:start + batch_size].to(device) if ne_all is not None else None
        noise = prepare_latents(len(batch), shape, seed + batch_idx + rank * seed_stride, device)
        images = engine.generate(pe, ne, latents=noise, num_inference_steps=num_inference_steps,
                                 use_graph=use_graph and len(batch) == batch_size, output_type="pt")
        latents = engine.last_latents.to(torch.float16)            # the reference's pipeline dtype
        if torch.isnan(latents).any():
            raise ValueError(f"teacher latents of batch {batch_idx} on rank {rank} contain NaN")        # generate_data.py:209
        noise_cpu, latents_cpu = noise.cpu(), latents.cpu()
        for j, prompt in enumerate(batch):
            index = start + j
            ppo_data.save_teacher_pair(generation_path, ppo_data.teacher_pair_id(rank, index), prompt, noise_cpu[j], latents_cpu[j])
            evaluation.save_generation(generation_path, rank, index, images[j], prompt)
        done += len(batch)
    return done


def main(argv=None, *, unet=None, vae=None):
    """``unet`` / ``vae``: already loaded HIP handles to run on instead of building them from the arguments."""
    import consolver_amd
    from .engine import SDSamplingEngine
    from .synth import synthetic_prompt_embeds, synthetic_unet_state_dict, synthetic_vae_state_dict
    from .text_encoder import load_prompt_cache
    from .unet import HipUNet2DConditionModel
    from .vae import HipAutoencoderKL
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--generation_path", "--generation-path", dest="generation_path", required=True)
    ap.add_argument("--num_inference_steps", "--num-inference-steps", dest="num_inference_steps", type=int, default=40)
    ap.add_argument("--cfg", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=24)
    ap.add_argument("--num_samples", "--num-samples", dest="num_samples", type=int, default=None, help="use only the first N prompts")
    ap.add_argument("--prompt-cache")
    ap.add_argument("--unet"), ap.add_argument("--vae")
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic prompts with seeded random weights")
    ap.add_argument("--residual", default="f16x2", choices=["f16", "f16x2", "residual_fp32"])
    ap.add_argument("--seed-stride", type=int, default=0, help="added to the seed once per rank (0: every rank draws the same noise, as in the reference)")
    args = ap.parse_args(argv)
    rank, world, local, dist = launch.init_distributed()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    given = unet is not None and vae is not None
    if not given:
        unet, vae = HipUNet2DConditionModel(device=dev, residual=args.residual), HipAutoencoderKL(device=dev)
    if args.synthetic:
        if not given:
            unet.load_state_dict(synthetic_unet_state_dict(unet.manifest()))
            vae.load_state_dict(synthetic_vae_state_dict(vae.manifest()))
        prompts = [f"synthetic prompt {i}" for i in range(args.synthetic)]
        pe, ne = synthetic_prompt_embeds(args.synthetic, seed=1001).half(), synthetic_prompt_embeds(args.synthetic, seed=1002).half()
    else:
        if not args.prompt_cache or (not given and not (args.unet and args.vae)):
            ap.error("pass --prompt-cache, --unet and --vae, or --synthetic N")
        if not given:
            unet.load_state_dict(_load_sd(args.unet))
            vae.load_state_dict(_load_sd(args.vae))
        prompts, pe, ne = load_prompt_cache(args.prompt_cache)
    if args.num_samples is not None:
        prompts, pe, ne = prompts[:args.num_samples], pe[:args.num_samples], ne[:args.num_samples]
    sch = consolver_amd.DPMSolverMultistepScheduler(**consolver_amd.SD15_MULTISTEP_DPM_KWARGS)
    eng = SDSamplingEngine(unet, sch, guidance_scale=args.cfg, vae=vae)
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    n = generate_teacher_pairs(prompts, pe, ne, eng, args.generation_path, rank, world, args.num_inference_steps, args.batch_size, args.seed,
                               args.seed_stride, device=dev)
    torch.cuda.synchronize()
    secs = launch.reduce_max_seconds(dist, time.perf_counter() - t0, device=dev)
    report = launch.gather_report(dist, n, 0.0, device=dev)
    if rank == 0:
        total = sum(c for c, _ in report)
        print(f"{total} teacher pairs in {secs:.2f} s = {total / secs:.2f} pairs/s on {world} GPU(s); per rank: {[c for c, _ in report]}")
    if dist is not None:
        dist.destroy_process_group()
    return {"pairs": n, "seconds": secs, "steps": args.num_inference_steps}


if __name__ == "__main__":
    main()
