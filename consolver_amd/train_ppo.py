"""SD1.5 PPO training driver: teacher pairs -> grouped rollouts -> reward -> advantages -> policy update -> checkpoints.

Mirror of train_ppo.py:45-469 as run_ppo.sh starts it (configuration 5 of BASELINE.json), on the native engine.  The arguments of that script that mean
something here keep their names and the defaults of config.py; the rest of its command line is accepted and ignored with one line saying so, and the
combinations that are not reproduced are refused (``parse_args``).  Per step (``ppo.train_iteration``): a batch of ``--train_batch_size`` teacher pairs, one of
them repeated over the batch (``repeat_random_sample``), a step count n from 2..15, one rollout, decode, reward, advantages, ``--ppo_epochs`` optimisation
steps.  The learning rate is constant: the reference's loop never calls ``lr_scheduler.step()``.

    python -m torch.distributed.run --nproc-per-node 8 -m consolver_amd.train_ppo --data_dir train_coco/ --prompt-cache prompts.safetensors \\
        --unet unet.safetensors --vae vae.safetensors --output_dir outputs/depth --reward_type depth --reward_weights depth_anything.safetensors \\
        --train_batch_size 80 --order_dim 4 --scaler_dim 0 --factor_embedding_dim 1024 --factor_hidden_dim 256 --factor_num_actions 11

``--data_dir`` is a ``generate_teacher`` tree; each pair's prompt embeddings come from the prompt cache (``text_encoder.save_prompt_cache``), looked up by the
pair's prompt text.  ``--synthetic N`` first writes N seeded teacher pairs (``generate_teacher.generate_teacher_pairs``, ``--teacher_steps`` steps, synthetic
weights unless given, the synthetic embeddings with seeds 1001 / 1002) and trains on them: the driver then runs with nothing downloaded.

What the rollout shares (both on by default; ``--no_share`` / ``--no_group`` switch them off for comparison runs): the B rows are copies of one sample, so the
denoiser runs on one row per group of rows with equal action histories (``rollout.denoise_diffusion(group_rows=True)``), and the one teacher image goes through
the reward network once (``ppo.collect_rollout(share_target=True)``).

``--seed`` seeds ``random`` and torch identically on every rank (train_ppo.py:72-73, not ``seed + rank``): the draw of n agrees across ranks without a
broadcast.  One JSON line per step on rank 0: ``{"step", "loss", "norm", "reward", "n", "lr", "forward_rows"}``; every 10th step also ``"param_sum"``
(train_ppo.py:452-455), all-gathered over the ranks, and the run stops if the ranks disagree.  Checkpoints are ``<output_dir>/checkpoint-<step>/model.ckpt``
(``PolicyTrainer.save_checkpoint``, the reference's format) with ``trainer_state.pt`` next to it: the Adam moments, the step count and the ``random`` / torch
CPU / torch GPU generator states.  ``--resume_from_checkpoint`` continues exactly from a checkpoint that has the state file, and loads the policy alone from
one that has not (a reference-made ``model.ckpt``).  One process per GPU (``launch``); the ranks' gradients are averaged (``launch.average_gradients``).  The
reference's closing ``save_pretrained`` (:466-469) has no counterpart: the last checkpoint is the result.
"""
import argparse
import json
import math
import os
import random
import tempfile

import torch

from . import launch, ppo_data
from .ppo import PolicyTrainer, train_iteration

STATE_FILE = "trainer_state.pt"
# flags of run_ppo.sh with nothing behind them here: name -> argparse keywords
IGNORED = {"--pretrained_teacher_model": dict(type=str), "--tracker_project_name": dict(type=str), "--enable_xformers_memory_efficient_attention": dict(action="store_true"),
           "--mixed_precision": dict(type=str), "--max_train_samples": dict(type=int), "--dataloader_num_workers": dict(type=int),
           "--validation_steps": dict(type=int), "--checkpoints_total_limit": dict(type=int), "--report_to": dict(type=str), "--loss_type": dict(type=str),
           "--gradient_checkpointing": dict(action="store_true"), "--use_8bit_adam": dict(action="store_true")}
REWARD_LOADERS = {"dino": "load_dino_reward", "clip": "load_clip_reward", "depth": "load_depth_reward", "segmentation": "load_segmentation_reward",
                  "inception": "load_inception_reward"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data_dir", help="the teacher-pair tree (generate_teacher); with --synthetic: where to write it (default: a temporary directory)")
    ap.add_argument("--prompt-cache", "--prompt_cache", dest="prompt_cache")
    ap.add_argument("--unet"), ap.add_argument("--vae")
    ap.add_argument("--reward_weights", help="state dict of the reward model (every --reward_type but image_psnr)")
    ap.add_argument("--residual", default="f16x2", choices=["f16", "f16x2", "residual_fp32"])
    ap.add_argument("--synthetic", type=int, default=0, help="build N seeded teacher pairs first and train on them (seeded random weights unless given)")
    ap.add_argument("--teacher_steps", type=int, default=40, help="steps of the --synthetic teacher")
    ap.add_argument("--no_share", action="store_true", help="treat the B rows as unrelated: every forward at full batch, the teacher image once per row (for comparison)")
    ap.add_argument("--no_group", action="store_true", help="do not group rows with equal action histories (for comparison)")
    # config.py, under its names and defaults
    ap.add_argument("--output_dir", default="lcm-xl-distilled")
    ap.add_argument("--resolution", type=int, default=None, help="image side; must be 8 x the VAE's sample_size (512 for SD1.5)")
    ap.add_argument("--train_batch_size", type=int, default=16)
    ap.add_argument("--num_train_epochs", type=int, default=100)
    ap.add_argument("--max_train_steps", type=int, default=None, help="overrides --num_train_epochs")
    ap.add_argument("--learning_rate", type=float, default=1e-4)
    ap.add_argument("--lr_scheduler", default="constant")
    ap.add_argument("--gradient_accumulation_steps", type=int, default=1)
    ap.add_argument("--adam_beta1", type=float, default=0.9)
    ap.add_argument("--adam_beta2", type=float, default=0.999)
    ap.add_argument("--adam_weight_decay", type=float, default=1e-2)
    ap.add_argument("--adam_epsilon", type=float, default=1e-8)
    ap.add_argument("--max_grad_norm", type=float, default=1.0)
    ap.add_argument("--ppo_epochs", type=int, default=4)
    ap.add_argument("--clip_range", type=float, default=0.2)
    ap.add_argument("--entropy_coef", type=float, default=0.01)
    ap.add_argument("--cfg", type=float, default=3.0)
    ap.add_argument("--order_dim", type=int, default=4)
    ap.add_argument("--scaler_dim", type=int, default=2)
    ap.add_argument("--use_conv", action="store_true")
    ap.add_argument("--factor_embedding_dim", type=int, default=4)
    ap.add_argument("--factor_hidden_dim", type=int, default=4)
    ap.add_argument("--factor_num_actions", type=int, default=4)
    ap.add_argument("--reward_type", default="depth")
    ap.add_argument("--ppo_type", default="discrete")
    ap.add_argument("--checkpointing_steps", type=int, default=500)
    ap.add_argument("--resume_from_checkpoint", default=None, help='a checkpoint directory name under --output_dir, or "latest"')
    ap.add_argument("--seed", type=int, default=None, help="the same on every rank (train_ppo.py:72-73)")
    for flag, kw in IGNORED.items():
        ap.add_argument(flag, default=None, help="accepted for run_ppo.sh's command line; ignored", **kw)
    args = ap.parse_args(argv)
    if args.ppo_type != "discrete":
        ap.error(f"--ppo_type {args.ppo_type}: only 'discrete' exists (the reference imports a module for the other one that is not part of it)")
    if args.gradient_accumulation_steps != 1:
        ap.error("--gradient_accumulation_steps other than 1: in the reference it interacts with the per-epoch optimizer.step() under accelerator.accumulate, "
                 "and that combination is not reproduced")
    if args.lr_scheduler != "constant":
        ap.error(f"--lr_scheduler {args.lr_scheduler}: the reference's loop never calls lr_scheduler.step(), so its rate is constant whatever is asked for; "
                 "only 'constant' is accepted")
    if not args.synthetic and not (args.data_dir and args.prompt_cache):
        ap.error("pass --data_dir and --prompt-cache, or --synthetic N")
    return args, ap


def ignored_note(args):
    """the one line about the accepted-and-ignored flags that were given, or None"""
    given = [f for f in IGNORED if getattr(args, f[2:]) not in (None, False)]
    if not given:
        return None
    note = "ignored (nothing behind them on the native engine): " + " ".join(given)
    if args.use_8bit_adam:
        note += "; --use_8bit_adam: the update is fp32 AdamW (cs_adamw_step)"
    return note


def check_resolution(ap, resolution, sample_size):
    side = 8 * sample_size
    if resolution is not None and resolution != side:
        ap.error(f"--resolution {resolution}: the VAE is built for {side} x {side} images")
    return side


def latest_checkpoint(output_dir):
    """the ``checkpoint-<step>`` directory with the highest step (train_ppo.py:291-297), or None; names that are not of that form are ignored"""
    if not os.path.isdir(output_dir):
        return None
    dirs = [d for d in os.listdir(output_dir) if d.startswith("checkpoint-") and d[len("checkpoint-"):].isdigit() and os.path.isdir(os.path.join(output_dir, d))]
    return max(dirs, key=lambda d: int(d[len("checkpoint-"):])) if dirs else None


def batch_indices(global_step, rank, world, n_items, batch_size):
    """The dataset items of rank ``rank`` at 0-based step ``global_step``: the unshuffled dataset in batches of ``batch_size`` (train_ppo.py:234-240), batch
    ``(global_step * world + rank) mod ceil(n_items / batch_size)``, so the ranks of one step take consecutive batches and the sequence goes on where it was
    after a resume.  A short last batch wraps round to the first items, so every batch has ``batch_size`` rows.  Both the interleaving and the wrap are this
    project's choice: the reference's prepared DataLoader shards batches over the ranks in its own way and hands out a short last batch."""
    if n_items < 1 or batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"batch_indices: n_items={n_items} batch_size={batch_size} rank={rank} world={world}")
    n_batches = (n_items + batch_size - 1) // batch_size
    b = (global_step * world + rank) % n_batches
    return [(b * batch_size + j) % n_items for j in range(batch_size)]


def prompt_rows(prompt_index, texts):
    """rows of the prompt cache for the pairs' prompt texts; a prompt the cache does not hold is an error that names it"""
    rows = []
    for t in texts:
        i = prompt_index.get(t.strip())
        if i is None:
            raise KeyError(f"the prompt cache has no entry for the teacher pair's prompt {t!r}")
        rows.append(i)
    return rows


def load_batch(ds, indices, prompt_index, pe_all, ne_all, device):
    """``TeacherPairDataset`` items collated like the reference's DataLoader does, on the GPU, and their cached prompt embeddings"""
    text, noise, tch = ppo_data.collate_teacher_pairs([ds[j] for j in indices])
    rows = prompt_rows(prompt_index, text)
    pe = pe_all[rows].to(device)
    ne = ne_all[rows].to(device) if ne_all is not None else None
    return (text, noise.to(device), tch.to(device)), pe, ne


def check_param_sums(sums):
    """train_ppo.py:452-455 prints one parameter sum per process and leaves the comparison to the reader; here differing sums stop the run"""
    if any(s != sums[0] for s in sums):
        raise RuntimeError(f"the ranks' policies have diverged: parameter sums per rank {list(sums)}")
    return sums[0]


def save_trainer_state(ckpt_dir, trainer, device):
    state = trainer.state_dict()
    state.update(random_state=random.getstate(), torch_rng_state=torch.get_rng_state(), cuda_rng_state=torch.cuda.get_rng_state(device))
    torch.save(state, os.path.join(ckpt_dir, STATE_FILE))


def load_trainer_state(ckpt_dir, trainer, device):
    """-> True if the checkpoint held the state file (exact continuation), False if it is a policy-only checkpoint"""
    path = os.path.join(ckpt_dir, STATE_FILE)
    if not os.path.exists(path):
        return False
    state = torch.load(path, map_location="cpu", weights_only=False)
    trainer.load_state_dict(state)
    random.setstate(state["random_state"])
    torch.set_rng_state(state["torch_rng_state"])
    torch.cuda.set_rng_state(state["cuda_rng_state"], device)
    return True


def main(argv=None, *, unet=None, vae=None, reward_model=None, reward_model_processor=None):
    """``unet`` / ``vae`` / ``reward_model``: already loaded HIP handles to run on instead of building them from the arguments."""
    import consolver_amd
    from . import generate_teacher as gt
    from .engine import SDSamplingEngine
    from .generate import _load_sd
    from .synth import synthetic_prompt_embeds, synthetic_unet_state_dict, synthetic_vae_state_dict
    from .text_encoder import load_prompt_cache
    from .unet import HipUNet2DConditionModel
    from .vae import HipAutoencoderKL
    args, ap = parse_args(argv)
    rank, world, local, dist = launch.init_distributed()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    say = print if rank == 0 else (lambda *a, **k: None)
    note = ignored_note(args)
    if note:
        say(note, flush=True)
    if args.seed is not None:
        random.seed(args.seed)
        torch.manual_seed(args.seed)
    given = unet is not None and vae is not None
    if not given:
        if not args.synthetic and not (args.unet and args.vae):
            ap.error("pass --unet and --vae, or --synthetic N")
        unet, vae = HipUNet2DConditionModel(device=dev, residual=args.residual), HipAutoencoderKL(device=dev)
        unet.load_state_dict(_load_sd(args.unet) if args.unet else synthetic_unet_state_dict(unet.manifest()))
        vae.load_state_dict(_load_sd(args.vae) if args.vae else synthetic_vae_state_dict(vae.manifest()))
    check_resolution(ap, args.resolution, vae.config.sample_size)
    noise_scheduler = consolver_amd.PPOScheduler(
        beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, steps_offset=1, timestep_spacing="trailing",
        order_dim=args.order_dim, scaler_dim=args.scaler_dim, use_conv=args.use_conv, ppo_type=args.ppo_type,
        factor_net_kwargs=dict(embedding_dim=args.factor_embedding_dim, hidden_dim=args.factor_hidden_dim, num_actions=args.factor_num_actions))
    noise_scheduler.factor_net.to(dev)
    if dist is not None:                        # every rank starts from rank 0's policy (what DDP does at construction)
        for p in noise_scheduler.factor_net.parameters():
            dist.broadcast(p.data, src=0)
    if args.reward_type != "image_psnr" and reward_model is None:
        from . import reward_model as rm
        if args.reward_type not in REWARD_LOADERS:
            ap.error(f"--reward_type {args.reward_type}: expected image_psnr or one of {sorted(REWARD_LOADERS)}")
        if not args.reward_weights:
            ap.error(f"--reward_type {args.reward_type} needs --reward_weights")
        reward_model, reward_model_processor = getattr(rm, REWARD_LOADERS[args.reward_type])(dev)
        reward_model.load_state_dict(_load_sd(args.reward_weights))
    trainer = PolicyTrainer(noise_scheduler.factor_net, lr=args.learning_rate, betas=(args.adam_beta1, args.adam_beta2),
                            weight_decay=args.adam_weight_decay, eps=args.adam_epsilon, max_grad_norm=args.max_grad_norm,
                            clip_range=args.clip_range, entropy_coef=args.entropy_coef)
    if rank == 0:
        os.makedirs(args.output_dir, exist_ok=True)
    logs = []
    with tempfile.TemporaryDirectory() as work:
        data_dir = args.data_dir
        if args.synthetic:
            data_dir = data_dir or os.path.join(work, "data")
            prompts = [f"synthetic prompt {i}" for i in range(args.synthetic)]
            pe_all, ne_all = synthetic_prompt_embeds(args.synthetic, seed=1001).half(), synthetic_prompt_embeds(args.synthetic, seed=1002).half()
            if rank == 0 or not args.data_dir:          # a shared --data_dir is written by rank 0 alone; a temporary one by every rank, identically
                teacher = SDSamplingEngine(unet, consolver_amd.DPMSolverMultistepScheduler(**consolver_amd.SD15_MULTISTEP_DPM_KWARGS),
                                           guidance_scale=args.cfg, vae=vae)
                gt.generate_teacher_pairs(prompts, pe_all, ne_all, teacher, data_dir, num_inference_steps=args.teacher_steps,
                                          batch_size=min(24, args.synthetic), device=dev)
        else:
            prompts, pe_all, ne_all = load_prompt_cache(args.prompt_cache)
        if dist is not None:
            dist.barrier()
        ds = ppo_data.TeacherPairDataset(data_dir, strict=True)
        if len(ds) == 0:
            raise RuntimeError(f"no teacher pairs under {data_dir}")
        prompt_index = {p.strip(): i for i, p in enumerate(prompts)}
        n_batches = (len(ds) + args.train_batch_size - 1) // args.train_batch_size
        max_steps = args.max_train_steps if args.max_train_steps is not None else args.num_train_epochs * math.ceil(n_batches / world)
        # resume last: the generator states of the checkpoint replace whatever the set-up above consumed
        global_step = 0
        if args.resume_from_checkpoint:
            name = latest_checkpoint(args.output_dir) if args.resume_from_checkpoint == "latest" else os.path.basename(args.resume_from_checkpoint)
            if name is None:
                say(f"Checkpoint '{args.resume_from_checkpoint}' does not exist. Starting a new training run.")
            else:
                ckpt = os.path.join(args.output_dir, name)
                trainer.load_checkpoint(ckpt)
                exact = load_trainer_state(ckpt, trainer, dev)
                global_step = int(name.split("-")[1])
                say(f"Resuming from checkpoint {name}" + ("" if exact else f": no {STATE_FILE} there (a policy-only checkpoint), so the Adam moments start "
                                                                            "at zero and the random streams are not continued"), flush=True)
        first_step = global_step
        share = not args.no_share
        while global_step < max_steps:
            batch, pe, ne = load_batch(ds, batch_indices(global_step, rank, world, len(ds), args.train_batch_size), prompt_index, pe_all, ne_all, dev)
            out = train_iteration(trainer, None, noise_scheduler, unet, vae, batch, None, cfg=args.cfg, ppo_epochs=args.ppo_epochs,
                                  reward_type=args.reward_type, dist=dist, prompt_embeds=pe, negative_prompt_embeds=ne, share_identical=share,
                                  reward_model=reward_model, reward_model_processor=reward_model_processor,
                                  group_rows=share and not args.no_group, share_target=share)
            global_step += 1
            log = {"step": global_step, "loss": float(out["loss"]), "norm": float(out["norm"]), "reward": float(out["reward"]),
                   "n": out["num_inference_steps"], "lr": args.learning_rate, "forward_rows": list(out["forward_rows"])}
            if global_step % 10 == 0:
                mine = sum(p.detach().sum().item() for p in noise_scheduler.factor_net.parameters())
                log["param_sum"] = check_param_sums([r[0] for r in launch.gather_rank_records(dist, [mine], device=dev)])
            logs.append(log)
            if rank == 0:
                print(json.dumps(log), flush=True)
                if global_step % args.checkpointing_steps == 0:
                    save_trainer_state(trainer.save_checkpoint(args.output_dir, global_step), trainer, dev)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return {"first_step": first_step, "global_step": global_step, "logs": logs, "trainer": trainer}


if __name__ == "__main__":
    main()
