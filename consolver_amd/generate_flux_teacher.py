"""FLUX teacher-pair generator: reference images + prompts -> 28-step Euler edits -> initial / final packed latents + edited images.

Mirror of edit_ppo/edit_pretrain/generate.py on the native engine.  Under ``--data DIR`` it reads ``ref_images/{i}.png`` and
``prompts/{i}.txt`` for i in [0, --count) (an index with either file missing is skipped, :38-44), draws the noise with generator seed 42
(:76), runs 28 steps at guidance 2.5 with the Euler scheduler (``FlowMatchGeneralDiscreteScheduler(type="euler")``, the pipeline's stock
scheduler there) and writes what ``ppo_data.FluxTeacherPairDataset`` (edit_ppo/data_processing.py) reads back:

    DIR/initial_noises/{i}.pt   packed [1, L, 64] latents in the model dtype (torch.save)          (:81)
    DIR/obtained_noises/{i}.pt  the same after the last step                                       (:133)
    DIR/edited_images/{i}.png   their decoded image                                                (:142)

The text side needs third-party weights and tokenizers: the T5 / CLIP embeddings of prompt i come from an instruction cache under the key
``str(i)`` (``generate_flux.save_instruction_cache``).  One process per GPU, contiguous index shards (``launch.shard_bounds``), no data-path
collective.  NaN latents raise.

    python -m torch.distributed.run --nproc-per-node 8 -m consolver_amd.generate_flux_teacher --data data/ \\
        --instruction-cache prompts.safetensors --transformer dit.safetensors --vae vae.safetensors
"""
import argparse
import os
import time

import torch

from . import launch, ppo_data
from .flux import pack_latents
from .generate import prepare_latents
from .generate_flux import load_instruction_embeds, load_models, make_scheduler, preprocess_image, synthetic_inputs
from .vae import encode_image_latents, flux_decode_latents


def generate_flux_teacher_pairs(data_dir, indices, engine, vae, cache, device, num_inference_steps=28, seed=42):
    """edit_pretrain/generate.py:35-144 for ``indices``.  ``engine``: a ``FluxKontextSamplingEngine`` around the teacher's scheduler;
    ``cache``: an open instruction cache.  Returns the indices written."""
    from PIL import Image
    S = vae.config.sample_size                               # latent side; image side = 8 S
    done = []
    for i in indices:
        img_path, prompt_path = os.path.join(data_dir, "ref_images", f"{i}.png"), os.path.join(data_dir, "prompts", f"{i}.txt")
        if not os.path.exists(img_path) or not os.path.exists(prompt_path):
            continue
        image = preprocess_image(img_path, 8 * S).to(device, torch.float16)
        image_latents = pack_latents(encode_image_latents(vae, image)).to(torch.bfloat16)
        initial = pack_latents(prepare_latents(1, (vae.config.latent_channels, S, S), seed, device, torch.bfloat16))
        pe, pooled = load_instruction_embeds(cache, str(i), device)
        latents = engine.generate(initial, image_latents, pe, pooled, latent_hw=(S // 2, S // 2), num_inference_steps=num_inference_steps)
        img = flux_decode_latents(vae, latents.to(torch.float16), height=8 * S, width=8 * S)[0]
        arr = (img.float().clamp(0, 1).permute(1, 2, 0) * 255.0).round().to(torch.uint8).cpu().numpy()
        ppo_data.save_flux_teacher_pair(data_dir, i, initial, latents, Image.fromarray(arr))      # (raises on NaN latents)
        done.append(i)
    return done


def synthetic_tree(n, data_dir, work_dir, joint_attention_dim, pooled_projection_dim, image_size):
    """n seeded reference images and prompts under ``data_dir``; returns their instruction cache (keys "0" .. "n-1") under ``work_dir``."""
    from PIL import Image
    entries, image_dir, cache_path = synthetic_inputs(n, work_dir, joint_attention_dim, pooled_projection_dim, image_size, key="{}")
    os.makedirs(os.path.join(data_dir, "ref_images"), exist_ok=True)
    os.makedirs(os.path.join(data_dir, "prompts"), exist_ok=True)
    for i, e in enumerate(entries):
        Image.open(os.path.join(image_dir, e["file_name"])).save(os.path.join(data_dir, "ref_images", f"{i}.png"))
        with open(os.path.join(data_dir, "prompts", f"{i}.txt"), "w") as f:
            f.write(e["instruction"])
    return cache_path


def main(argv=None, *, transformer=None, vae=None):
    """``transformer`` / ``vae``: already loaded HIP handles to run on instead of building them from the arguments."""
    import tempfile
    from safetensors import safe_open
    from .flux import FluxKontextSamplingEngine
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="the tree holding ref_images/ and prompts/; the outputs are written next to them")
    ap.add_argument("--instruction-cache")
    ap.add_argument("--transformer"), ap.add_argument("--vae")
    ap.add_argument("--count", type=int, default=2000, help="indices 0 .. count-1 are tried (generate.py:35)")
    ap.add_argument("--num_inference_steps", "--num-inference-steps", "--steps", dest="num_inference_steps", type=int, default=28)
    ap.add_argument("--guidance", type=float, default=2.5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--synthetic", type=int, default=0, help="write N seeded reference images and prompts to --data first (seeded random weights unless given)")
    args = ap.parse_args(argv)
    if not args.synthetic and not args.instruction_cache:
        ap.error("pass --instruction-cache, or --synthetic N")
    rank, world, local, dist = launch.init_distributed()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    transformer, vae = load_models(args, ap, dev, transformer, vae)
    eng = FluxKontextSamplingEngine(transformer, make_scheduler("euler"), guidance_scale=args.guidance)
    with tempfile.TemporaryDirectory() as work:
        cache_path, count = args.instruction_cache, args.count
        if args.synthetic:
            count = args.synthetic
            # every rank writes the same seeded tree cache; only rank 0 writes into --data
            cache_path = synthetic_tree(args.synthetic, args.data if rank == 0 else os.path.join(work, "data"), work,
                                        transformer.config["joint_attention_dim"], transformer.config["pooled_projection_dim"], 8 * vae.config.sample_size)
        if dist is not None:
            dist.barrier()
        lo, hi = launch.shard_bounds(count, world, rank)
        t0 = time.perf_counter()
        with safe_open(cache_path, framework="pt", device="cpu") as cache:
            done = generate_flux_teacher_pairs(args.data, range(lo, hi), eng, vae, cache, dev, args.num_inference_steps, args.seed)
        torch.cuda.synchronize()
    secs = launch.reduce_max_seconds(dist, time.perf_counter() - t0, device=dev)
    report = launch.gather_report(dist, len(done), 0.0, device=dev)
    if rank == 0:
        total = sum(c for c, _ in report)
        print(f"{total} FLUX teacher pairs in {secs:.2f} s = {total / secs:.2f} pairs/s on {world} GPU(s); per rank: {[c for c, _ in report]}")
    if dist is not None:
        dist.destroy_process_group()
    return {"pairs": len(done), "indices": done, "seconds": secs, "steps": args.num_inference_steps}


if __name__ == "__main__":
    main()
