"""Sharded FLUX-Kontext edit driver: JSONL instructions + reference images -> edited images.

Mirror of ``edit_ppo/generate_ours.py`` (:30-189) on the native engine: the same JSONL entry fields (``key``, ``category``,
``file_name``, ``instruction``), the same output layout ``OUTPUT_DIR/<category>/<key>/{ref_image.jpg, instruction.txt,
edited_image.jpg}``, ceil-sized chunks per GPU (:176-177), one process per GPU, generator seed 0 per entry (:92).

Per entry (edit_ppo/pipeline.py:613-623, 1009-1150): reference image -> VAE encoder (posterior mode, shift, scale) -> packed
image latents; seeded noise -> packed latents; 8-step FMPPOScheduler loop around the DiT; unpack -> VAE decoder -> pixels.
The text side (T5-XXL + CLIP embeddings of the instruction) needs third-party weights and tokenizers: it is read from an
embedding cache (``save_instruction_cache``): ``{key}.prompt_embeds`` [512, 4096] and ``{key}.pooled`` [768] in one safetensors file.

True classifier-free guidance (edit_ppo/pipeline.py:1100-1115): ``--true_cfg_scale S`` (> 1) with ``--negative-embeds FILE`` (one negative
prompt's ``prompt_embeds`` [T, D] and ``pooled`` [768] shared by every entry, ``save_negative_embeds``) runs the negative-prompt branch in every
step, with every ``--solver``.
"""
import json
import os
import re
import shutil
from math import ceil

import numpy as np
import torch

from . import launch
from .flux import pack_latents
from .vae import encode_image_latents, flux_decode_latents


def sanitize_folder_name(name):
    """generate_ours.py:28-32: every non-alphanumeric character of the stripped category becomes "_"; empty -> "Unknown"."""
    if not name:
        return "Unknown"
    return re.sub(r"[^a-zA-Z0-9]", "_", name.strip())


def ensure_unique_path(path):
    """generate_ours.py:40-48: append _1, _2, ... when the file exists."""
    if not os.path.exists(path):
        return path
    base, ext = os.path.splitext(path)
    i = 1
    while os.path.exists(f"{base}_{i}{ext}"):
        i += 1
    return f"{base}_{i}{ext}"


def load_jsonl(path):
    """generate_ours.py:152-163: invalid lines are skipped."""
    data = []
    with open(path) as f:
        for line in f:
            try:
                data.append(json.loads(line.strip()))
            except json.JSONDecodeError:
                continue
    return data


def chunk_entries(data, num_gpus):
    """generate_ours.py:176-177."""
    chunk_size = ceil(len(data) / num_gpus) if data else 0
    return [data[i:i + chunk_size] for i in range(0, len(data), chunk_size)] if chunk_size else []


def save_instruction_cache(path, embeds):
    """embeds: {key: (prompt_embeds [T, 4096], pooled [768])}"""
    from safetensors.torch import save_file
    t = {}
    for k, (pe, pooled) in embeds.items():
        t[f"{k}.prompt_embeds"] = pe.detach().to("cpu", torch.bfloat16).contiguous()
        t[f"{k}.pooled"] = pooled.detach().to("cpu", torch.bfloat16).contiguous()
    save_file(t, path, metadata={"format": "consolver_amd.instruction_cache.v1"})


def save_negative_embeds(path, prompt_embeds, pooled):
    """the one negative prompt of a driver run (``--negative-embeds``): prompt_embeds [T, D] and pooled [768]"""
    from safetensors.torch import save_file
    save_file({"prompt_embeds": prompt_embeds.detach().to("cpu", torch.bfloat16).contiguous(),
               "pooled": pooled.detach().to("cpu", torch.bfloat16).contiguous()}, path, metadata={"format": "consolver_amd.negative_embeds.v1"})


def load_negative_embeds(path, device):
    """-> (negative_prompt_embeds [1, T, D], negative_pooled_prompt_embeds [1, 768]) on ``device``"""
    from safetensors import safe_open
    with safe_open(path, framework="pt", device="cpu") as f:
        return f.get_tensor("prompt_embeds").to(device)[None], f.get_tensor("pooled").to(device)[None]


def load_instruction_embeds(cache, key, device):
    return cache.get_tensor(f"{key}.prompt_embeds").to(device)[None], cache.get_tensor(f"{key}.pooled").to(device)[None]


def preprocess_image(path, size):
    """reference image -> [1, 3, size, size] in [-1, 1] (pipeline image_processor: resize + normalise)."""
    from PIL import Image
    img = Image.open(path).convert("RGB").resize((size, size), Image.LANCZOS)
    x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0
    return (x * 2 - 1)[None]


def process_instruction(entry, engine, vae, cache, image_dir, output_dir, device, num_inference_steps=8, seed=0, negative=None, true_cfg_scale=1.0):
    """generate_ours.py:50-104 for one entry; returns the edited-image path (or None when the reference image is missing).
    ``negative``: (negative_prompt_embeds [1, T, D], negative_pooled_prompt_embeds [1, 768]) for true CFG at ``true_cfg_scale`` > 1."""
    from PIL import Image
    key, category, file_name, instruction = entry["key"], entry["category"], entry["file_name"], entry["instruction"]
    src = os.path.join(image_dir, os.path.basename(file_name))
    if not os.path.exists(src):
        return None
    sub = os.path.join(output_dir, sanitize_folder_name(category), key)
    os.makedirs(sub, exist_ok=True)
    shutil.copy(src, ensure_unique_path(os.path.join(sub, "ref_image.jpg")))
    with open(ensure_unique_path(os.path.join(sub, "instruction.txt")), "w") as f:
        f.write(instruction)
    S = vae.config.sample_size                               # latent side; image side = 8 S
    image = preprocess_image(src, 8 * S).to(device, torch.float16)
    image_latents = pack_latents(encode_image_latents(vae, image)).to(torch.bfloat16)
    gen = torch.Generator().manual_seed(seed)                # generator=torch.manual_seed(0), generate_ours.py:92
    noise = torch.randn(1, vae.config.latent_channels, S, S, generator=gen).to(device)
    latents = pack_latents(noise).to(torch.bfloat16)
    pe, pooled = load_instruction_embeds(cache, key, device)
    cfg_kw = {} if negative is None else dict(negative_prompt_embeds=negative[0], negative_pooled_prompt_embeds=negative[1], true_cfg_scale=true_cfg_scale)
    out = engine.generate(latents, image_latents, pe, pooled, latent_hw=(S // 2, S // 2), num_inference_steps=num_inference_steps, **cfg_kw)
    img = flux_decode_latents(vae, out.to(torch.float16), height=8 * S, width=8 * S)[0]
    arr = (img.float().clamp(0, 1).permute(1, 2, 0) * 255.0).round().to(torch.uint8).cpu().numpy()
    dst = ensure_unique_path(os.path.join(sub, "edited_image.jpg"))
    Image.fromarray(arr).save(dst)
    return dst


def worker(entries, engine, vae, cache_path, image_dir, output_dir, device, num_inference_steps=8, negative=None, true_cfg_scale=1.0):
    """generate_ours.py:107-148 with the models already built for this process."""
    from safetensors import safe_open
    done = 0
    with safe_open(cache_path, framework="pt", device="cpu") as cache:
        for entry in entries:
            done += process_instruction(entry, engine, vae, cache, image_dir, output_dir, device, num_inference_steps,
                                        negative=negative, true_cfg_scale=true_cfg_scale) is not None
    return done


def shard_for_rank(data, world, rank):
    chunks = chunk_entries(data, world)
    return chunks[rank] if rank < len(chunks) else []


FLUX_SOLVERS = ("consistencysolver", "euler", "heun", "dpm-solver", "dpm-solver-multistep")
# generate_ours.py:122-134: the learned solver's policy as the reference driver builds it
FLUX_POLICY_KWARGS = dict(order_dim=2, scaler_dim=0, mu_dim=0, factor_net_kwargs=dict(embedding_dim=1024, hidden_dim=256, num_actions=11))


def make_scheduler(solver, **policy_kwargs):
    """the scheduler of generate_ours.py:127-134 (``"consistencysolver"``; ``policy_kwargs`` override ``FLUX_POLICY_KWARGS``) or of
    generate_pretrain.py:118-122 (``type = solver``), on FLUX.1-Kontext's published scheduler config.  The baselines have no policy."""
    import consolver_amd
    from .scheduling_fmppo import KONTEXT_SCHEDULER_CONFIG
    if solver == "consistencysolver":
        return consolver_amd.FMPPOScheduler.from_config(dict(KONTEXT_SCHEDULER_CONFIG), **{**FLUX_POLICY_KWARGS, **policy_kwargs})
    if solver not in FLUX_SOLVERS:
        raise ValueError(f"unknown solver {solver!r}; expected one of {FLUX_SOLVERS}")
    if policy_kwargs:
        raise ValueError(f"solver {solver!r} has no policy: unexpected {sorted(policy_kwargs)}")
    return consolver_amd.FlowMatchGeneralDiscreteScheduler.from_config(dict(KONTEXT_SCHEDULER_CONFIG), type=solver)


def synthetic_inputs(n, work_dir, joint_attention_dim, pooled_projection_dim, image_size, seq_len=64, seed=1001, key="synthetic_{}"):
    """n seeded stand-ins for a dataset (no checkpoints or datasets exist offline): reference images, JSONL-style entries (keys
    ``key.format(i)``) and their instruction cache under ``work_dir``.  Returns (entries, image_dir, cache_path)."""
    from PIL import Image
    image_dir, cache_path = os.path.join(work_dir, "images"), os.path.join(work_dir, "instructions.safetensors")
    os.makedirs(image_dir, exist_ok=True)
    rng, g = np.random.default_rng(seed), torch.Generator().manual_seed(seed)
    entries, embeds = [], {}
    for i in range(n):
        Image.fromarray(rng.integers(0, 255, (image_size, image_size, 3), dtype=np.uint8)).save(os.path.join(image_dir, f"{i}.jpg"))
        entries.append(dict(key=key.format(i), category="synthetic", file_name=f"{i}.jpg", instruction=f"synthetic instruction {i}"))
        embeds[entries[-1]["key"]] = (torch.randn(seq_len, joint_attention_dim, generator=g), torch.randn(pooled_projection_dim, generator=g))
    save_instruction_cache(cache_path, embeds)
    return entries, image_dir, cache_path


def _load_sd(path):
    from safetensors.torch import load_file
    return load_file(path) if path.endswith(".safetensors") else torch.load(path, map_location="cpu")


def load_models(args, ap, dev, transformer=None, vae=None):
    """the DiT and the FLUX VAE (with its encoder) of a driver run: the handles passed in, else built from ``--transformer`` / ``--vae`` state
    dicts, else (``--synthetic``) full-size networks with seeded random weights."""
    from .flux import HipFluxTransformer2DModel
    from .synth import synthetic_flux_state_dict, synthetic_vae_state_dict
    from .vae import FLUX_VAE_CONFIG, HipAutoencoderKL
    if transformer is not None and vae is not None:
        return transformer, vae
    if not args.synthetic and not (args.transformer and args.vae):
        ap.error("pass --transformer and --vae, or --synthetic N")
    transformer = HipFluxTransformer2DModel(device=dev)
    vae = HipAutoencoderKL(dict(FLUX_VAE_CONFIG, with_encoder=True), device=dev)
    # (the 11.9 B synthetic parameters are drawn on the device in the model dtype: 24 GB there instead of 48 GB of host fp32)
    transformer.load_state_dict(_load_sd(args.transformer) if args.transformer else
                                synthetic_flux_state_dict(transformer.manifest(), device=dev, dtype=transformer.dtype))
    vae.load_state_dict(_load_sd(args.vae) if args.vae else synthetic_vae_state_dict(vae.manifest()))
    return transformer, vae


def parse_args(argv=None):
    """-> (parser, args) of ``python -m consolver_amd.generate_flux``; argument conflicts are parser errors (SystemExit)"""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--jsonl"), ap.add_argument("--image-dir"), ap.add_argument("--instruction-cache")
    ap.add_argument("--transformer"), ap.add_argument("--vae"), ap.add_argument("--policy")
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic entries (seeded images and embeddings; seeded random weights unless given)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--guidance", type=float, default=2.5)
    ap.add_argument("--solver", default="consistencysolver", choices=FLUX_SOLVERS,
                    help="the learned solver (default) or a comparison method of generate_pretrain.py (scheduler type); those have no policy")
    ap.add_argument("--true_cfg_scale", type=float, default=1.0,
                    help="> 1: true classifier-free guidance, a second DiT branch on the negative prompt in every step (needs --negative-embeds or --synthetic)")
    ap.add_argument("--negative-embeds", help="safetensors file with the negative prompt's prompt_embeds [T, D] and pooled [768] (save_negative_embeds)")
    args = ap.parse_args(argv)
    if args.solver != "consistencysolver" and args.policy:
        ap.error(f"--policy belongs to the learned solver; --solver {args.solver} has no policy")
    if not args.synthetic and not (args.jsonl and args.image_dir and args.instruction_cache):
        ap.error("pass --jsonl, --image-dir and --instruction-cache, or --synthetic N")
    if args.true_cfg_scale > 1.0 and not args.synthetic and not args.negative_embeds:
        ap.error("--true_cfg_scale > 1 needs the negative prompt's embeddings: pass --negative-embeds FILE")
    return ap, args


def main(argv=None, *, transformer=None, vae=None):
    """``python -m consolver_amd.generate_flux``: generate_ours.py / generate_pretrain.py as one command, one process per GPU
    (``launch``).  ``transformer`` / ``vae``: already loaded HIP handles to run on instead of building them from the arguments."""
    import tempfile
    import time
    from .flux import FluxKontextSamplingEngine
    ap, args = parse_args(argv)
    rank, world, local, dist = launch.init_distributed()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    transformer, vae = load_models(args, ap, dev, transformer, vae)
    sch = make_scheduler(args.solver)
    if getattr(sch, "factor_net", None) is not None:
        if args.policy:
            sch.factor_net.load_state_dict(torch.load(args.policy, map_location="cpu"))
        sch.factor_net.to(dev)
    eng = FluxKontextSamplingEngine(transformer, sch, guidance_scale=args.guidance)
    with tempfile.TemporaryDirectory() as work:
        if args.synthetic:
            data, image_dir, cache = synthetic_inputs(args.synthetic, work, transformer.config["joint_attention_dim"],
                                                      transformer.config["pooled_projection_dim"], 8 * vae.config.sample_size)
        else:
            data, image_dir, cache = load_jsonl(args.jsonl), args.image_dir, args.instruction_cache
        negative = None
        if args.true_cfg_scale > 1.0:
            if args.negative_embeds:
                negative = load_negative_embeds(args.negative_embeds, dev)
            else:       # --synthetic: one seeded negative embedding of the synthetic instructions' shape
                g = torch.Generator().manual_seed(2002)
                negative = (torch.randn(1, 64, transformer.config["joint_attention_dim"], generator=g).to(dev, torch.bfloat16),
                            torch.randn(1, transformer.config["pooled_projection_dim"], generator=g).to(dev, torch.bfloat16))
        if dist is not None:
            dist.barrier()
        t0 = time.perf_counter()
        n = worker(shard_for_rank(data, world, rank), eng, vae, cache, image_dir, args.out, dev, num_inference_steps=args.steps,
                   negative=negative, true_cfg_scale=args.true_cfg_scale)
        torch.cuda.synchronize()
    secs = launch.reduce_max_seconds(dist, time.perf_counter() - t0, device=dev)
    report = launch.gather_report(dist, n, 0.0, device=dev)
    if rank == 0:
        total = sum(c for c, _ in report)
        print(f"{total} edits in {secs:.2f} s = {total / secs:.2f} edits/s on {world} GPU(s); per rank: {[c for c, _ in report]}")
    if dist is not None:
        dist.destroy_process_group()
    return {"edits": n, "seconds": secs, "solver": args.solver, "steps": args.steps, "true_cfg_scale": args.true_cfg_scale if negative is not None else 1.0}


__all__ = ["sanitize_folder_name", "ensure_unique_path", "load_jsonl", "chunk_entries", "shard_for_rank", "save_instruction_cache", "save_negative_embeds", "load_negative_embeds", "parse_args",
           "process_instruction", "worker", "launch", "FLUX_SOLVERS", "make_scheduler", "main"]


if __name__ == "__main__":
    main()
