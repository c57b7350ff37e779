"""FLUX-Kontext PPO training driver: teacher pairs -> shared-prefix rollouts -> baseline advantage -> policy update -> checkpoints.

Mirror of edit_ppo/train_ppo.py as edit_ppo/run_ppo.sh starts it, on the native engine, with the arguments of that script that mean
something here under their names there.  Per step (``ppo_flux.train_iteration_flux``): a batch of ``--train_batch_size`` teacher pairs, one of
them repeated over the batch, a step count from 2..5 (rank 0 draws it for all ranks), one rollout call that also advances the plain-Euler
baseline, decode, reward, advantages, ``--ppo_epochs`` optimisation steps.  The learning rate is constant (the reference's default schedule).

    python -m torch.distributed.run --nproc-per-node 8 -m consolver_amd.train_flux_ppo --data_dir data/ --instruction-cache prompts.safetensors \\
        --transformer dit.safetensors --vae vae.safetensors --output_dir outputs/kontext --reward_type dino --reward_weights dinov2.safetensors

The text side needs third-party weights and tokenizers: the T5 / CLIP embeddings of pair ``i`` come from an instruction cache under the key
``str(i)`` (``generate_flux.save_instruction_cache``), as for ``generate_flux_teacher``.  ``--synthetic N`` first writes N seeded reference
images and prompts and their 28-step (``--teacher_steps``) Euler teacher pairs with the synthetic path of ``generate_flux_teacher`` and trains on
them with seeded random weights: the driver then runs with nothing downloaded.

One JSON line per step on rank 0: ``{"step", "loss", "norm", "reward", "reward_base", "n", "lr"}``.  Checkpoints are
``<output_dir>/checkpoint-<step>/model.ckpt`` (``PolicyTrainer.save_checkpoint``, the reference's format); ``--resume_from_checkpoint latest``
picks the highest step there.  ``--save_samples`` writes the step's images as the reference names them (:412-416) and is the only thing that
decodes to PIL.  One process per GPU (``launch``); the ranks' gradients are averaged (``launch.average_gradients``).
"""
import argparse
import json
import os
import random
import tempfile

import torch

from . import launch, ppo_data
from .generate_flux import load_instruction_embeds, load_models, make_scheduler
from .ppo import PolicyTrainer
from .ppo_flux import train_iteration_flux


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data_dir", help="the teacher-pair tree (generate_flux_teacher); with --synthetic: where to write it (default: a temporary directory)")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--instruction-cache", "--instruction_cache", dest="instruction_cache")
    ap.add_argument("--transformer"), ap.add_argument("--vae")
    ap.add_argument("--resolution", type=int, default=None, help="image side; must be the VAE's (default: 8 x its sample_size; 1024 for FLUX)")
    ap.add_argument("--train_batch_size", type=int, default=10)
    ap.add_argument("--max_train_steps", type=int, default=1001)
    ap.add_argument("--learning_rate", type=float, default=1e-4)
    ap.add_argument("--adam_beta1", type=float, default=0.9)
    ap.add_argument("--adam_beta2", type=float, default=0.999)
    ap.add_argument("--adam_weight_decay", type=float, default=1e-2)
    ap.add_argument("--adam_epsilon", type=float, default=1e-8)
    ap.add_argument("--max_grad_norm", type=float, default=1.0)
    ap.add_argument("--ppo_epochs", type=int, default=4)
    ap.add_argument("--clip_range", type=float, default=0.2)
    ap.add_argument("--entropy_coef", type=float, default=0.01)
    ap.add_argument("--cfg", type=float, default=2.5)
    ap.add_argument("--order_dim", type=int, default=2)
    ap.add_argument("--scaler_dim", type=int, default=0)
    ap.add_argument("--mu_dim", type=int, default=0)
    ap.add_argument("--factor_embedding_dim", type=int, default=1024)
    ap.add_argument("--factor_hidden_dim", type=int, default=256)
    ap.add_argument("--factor_num_actions", type=int, default=11)
    ap.add_argument("--reward_type", default="image_psnr")
    ap.add_argument("--reward_weights", help="state dict of the reward model (dino / clip)")
    ap.add_argument("--checkpointing_steps", type=int, default=100)
    ap.add_argument("--resume_from_checkpoint", default=None, help='a checkpoint directory name under --output_dir, or "latest"')
    ap.add_argument("--seed", type=int, default=None, help="the rank is added (train_ppo.py: set_seed(args.seed + process_index))")
    ap.add_argument("--save_samples", action="store_true")
    ap.add_argument("--noise_layout", default="reference", choices=("reference", "packed"), help="see ppo_flux.as_rollout_noise")
    ap.add_argument("--forward_batch_size", type=int, default=None, help="at most this many rows per DiT call")
    ap.add_argument("--no_share", action="store_true", help="run every forward at full batch (for comparison)")
    ap.add_argument("--synthetic", type=int, default=0, help="build N seeded teacher pairs first and train on them (seeded random weights unless given)")
    ap.add_argument("--teacher_steps", type=int, default=28, help="steps of the --synthetic teacher")
    args = ap.parse_args(argv)
    if not args.synthetic and not (args.data_dir and args.instruction_cache):
        ap.error("pass --data_dir and --instruction-cache, or --synthetic N")
    return args, ap


def latest_checkpoint(output_dir):
    """the ``checkpoint-<step>`` directory with the highest step (train_ppo.py:213-219), or None"""
    if not os.path.isdir(output_dir):
        return None
    dirs = [d for d in os.listdir(output_dir) if d.startswith("checkpoint-") and d.split("-")[1].isdigit()]
    return max(dirs, key=lambda d: int(d.split("-")[1])) if dirs else None


def load_batch(ds, indices, cache, device):
    """``FluxTeacherPairDataset`` items collated like the reference's DataLoader does, on the GPU, and their instruction embeddings"""
    items = [ds[j] for j in indices]
    image, text, noise, tch, ref = zip(*items)
    keys = [os.path.splitext(ds.img_names[j])[0] for j in indices]
    emb = [load_instruction_embeds(cache, k, device) for k in keys]
    text_embeds = {"prompt_embeds": torch.cat([e[0] for e in emb]), "pooled_prompt_embeds": torch.cat([e[1] for e in emb])}
    batch = (torch.stack(image).to(device), list(text), torch.stack(noise).to(device), torch.stack(tch).to(device), torch.stack(ref).to(device))
    return batch, text_embeds


def save_samples(samples_dir, pipe, roll, text, global_step, rank, n):
    """edit_ppo/train_ppo.py:412-416"""
    from PIL import Image
    from .evaluation import tensor_to_uint8_hwc
    from .ppo_flux import decode_latents_flux
    os.makedirs(samples_dir, exist_ok=True)
    pred = decode_latents_flux(pipe, roll["model_pred"])
    B = pred.shape[0]
    adv = roll["advantages"].reshape(B, n - 1, -1)[:, 0, 0].tolist()       # advantages_origin: one value per trajectory (step 1 is never masked)
    i = 0
    for i in range(min(10, B)):
        Image.fromarray(tensor_to_uint8_hwc(pred[i])).save(os.path.join(samples_dir, f"{global_step}_{rank}_{i}_{adv[i]: .3f}_{n}step.jpg"))
    target = decode_latents_flux(pipe, roll["target_latents"][:1], 1)
    Image.fromarray(tensor_to_uint8_hwc(target[0])).save(os.path.join(samples_dir, f"target_{global_step}_{rank}_{i}.jpg"))
    with open(os.path.join(samples_dir, f"conds_{global_step}_{rank}_{i}.txt"), "w") as f:
        f.write(text)


def main(argv=None, *, transformer=None, vae=None, reward_model=None, reward_model_processor=None):
    """``transformer`` / ``vae`` / ``reward_model``: already loaded HIP handles to run on instead of building them from the arguments."""
    from safetensors import safe_open
    from .flux import FluxKontextSamplingEngine
    from .pipeline import FluxKontextEditPipeline
    from . import generate_flux_teacher as gft
    args, ap = parse_args(argv)
    rank, world, local, dist = launch.init_distributed()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.seed is not None:
        random.seed(args.seed + rank)
        torch.manual_seed(args.seed + rank)
    transformer, vae = load_models(args, ap, dev, transformer, vae)
    side = 8 * vae.config.sample_size
    if args.resolution is not None and args.resolution != side:
        ap.error(f"--resolution {args.resolution}: the VAE is built for {side} x {side} images")
    noise_scheduler = make_scheduler("consistencysolver", order_dim=args.order_dim, scaler_dim=args.scaler_dim, mu_dim=args.mu_dim,
                                     factor_net_kwargs=dict(embedding_dim=args.factor_embedding_dim, hidden_dim=args.factor_hidden_dim,
                                                            num_actions=args.factor_num_actions))
    noise_scheduler.factor_net.to(dev)
    if dist is not None:                        # every rank starts from rank 0's policy (what DDP does at construction)
        for p in noise_scheduler.factor_net.parameters():
            dist.broadcast(p.data, src=0)
    base_scheduler = make_scheduler("euler")                                    # the reference's pipe.scheduler
    pipe = FluxKontextEditPipeline(transformer, noise_scheduler, vae, guidance_scale=args.cfg)
    if args.reward_type != "image_psnr" and reward_model is None:
        from .generate_flux import _load_sd
        from .reward_model import load_reward_model
        reward_model, reward_model_processor = load_reward_model(args.reward_type, device=dev)
        if not args.reward_weights:
            ap.error(f"--reward_type {args.reward_type} needs --reward_weights")
        reward_model.load_state_dict(_load_sd(args.reward_weights))
    trainer = PolicyTrainer(noise_scheduler.factor_net, lr=args.learning_rate, betas=(args.adam_beta1, args.adam_beta2),
                            weight_decay=args.adam_weight_decay, eps=args.adam_epsilon, max_grad_norm=args.max_grad_norm,
                            clip_range=args.clip_range, entropy_coef=args.entropy_coef)
    global_step = 0
    if args.resume_from_checkpoint:
        name = latest_checkpoint(args.output_dir) if args.resume_from_checkpoint == "latest" else os.path.basename(args.resume_from_checkpoint)
        if name is None:
            if rank == 0:
                print(f"Checkpoint '{args.resume_from_checkpoint}' does not exist. Starting a new training run.")
        else:
            trainer.load_checkpoint(os.path.join(args.output_dir, name))
            global_step = int(name.split("-")[1])
    first_step = global_step
    logs = []
    with tempfile.TemporaryDirectory() as work:
        data_dir, cache_path = args.data_dir, args.instruction_cache
        if args.synthetic:
            data_dir = data_dir or os.path.join(work, "data")
            # every rank writes the same seeded tree cache; only rank 0 writes the pairs into the shared directory
            mine = data_dir if (rank == 0 or not args.data_dir) else os.path.join(work, "data")
            cache_path = gft.synthetic_tree(args.synthetic, mine, work, transformer.config["joint_attention_dim"],
                                            transformer.config["pooled_projection_dim"], side)
            if rank == 0 or not args.data_dir:
                eng = FluxKontextSamplingEngine(transformer, make_scheduler("euler"), guidance_scale=args.cfg)
                with safe_open(cache_path, framework="pt", device="cpu") as cache:
                    gft.generate_flux_teacher_pairs(mine, range(args.synthetic), eng, vae, cache, dev, args.teacher_steps)
        if dist is not None:
            dist.barrier()
        ds = ppo_data.FluxTeacherPairDataset(data_dir, (side, side), strict=True)
        if len(ds) == 0:
            raise RuntimeError(f"no teacher pairs under {data_dir}")
        order_rng = random.Random((args.seed or 0) + rank)                       # the DataLoader's shuffle
        samples_dir = os.path.join(args.output_dir, "samples")
        with safe_open(cache_path, framework="pt", device="cpu") as cache:
            while global_step < args.max_train_steps:
                indices = [order_rng.randrange(len(ds)) for _ in range(args.train_batch_size)]
                batch, text_embeds = load_batch(ds, indices, cache, dev)
                out = train_iteration_flux(trainer, pipe, noise_scheduler, base_scheduler, batch, cfg=args.cfg, ppo_epochs=args.ppo_epochs,
                                           reward_type=args.reward_type, dist=dist, share_identical=not args.no_share, reward_model=reward_model,
                                           reward_model_processor=reward_model_processor, text_embeds=text_embeds, noise_layout=args.noise_layout,
                                           forward_batch_size=args.forward_batch_size)
                global_step += 1
                n = out["num_inference_steps"]
                log = {"step": global_step, "loss": float(out["loss"]), "norm": float(out["norm"]), "reward": float(out["reward"]),
                       "reward_base": float(out["reward_base"]), "n": n, "lr": args.learning_rate}
                logs.append(log)
                if rank == 0:
                    print(json.dumps(log), flush=True)
                    if global_step % args.checkpointing_steps == 0:
                        trainer.save_checkpoint(args.output_dir, global_step)
                if args.save_samples:
                    i = out["index"]
                    save_samples(samples_dir, pipe, dict(out["rollout"], target_latents=batch[3][i:i + 1]), batch[1][i], global_step, rank, n)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return {"first_step": first_step, "global_step": global_step, "logs": logs, "trainer": trainer}


if __name__ == "__main__":
    main()
