"""FLUX-Kontext PPO iteration at the reference trainer's own setting (edit_ppo/run_ppo.sh): B = 10 copies of one teacher pair, 1024 x 1024
(4096 + 4096 tokens per row), order_dim 2, no scale action, n = 2..5, 4 PPO epochs, full-size DiT and FLUX VAE with synthetic weights.

Times ``ppo_flux.train_iteration_flux`` with ``identical_inputs`` off and on, alternated within every round on one GPU, for the ``image_psnr``
and the ``dino`` reward, and writes the DiT rows actually run (``forward_rows``), the median milliseconds and the ratio next to the row-count
ratio.  No threshold is asserted: the file is the record.

    python tools/bench_flux_rollout.py --out profiles/flux_ppo_iteration_bench.txt [--rounds 3] [--forward-batch-size N]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consolver_amd import generate_flux as gf, ppo, ppo_flux                      # noqa: E402
from consolver_amd.flux import HipFluxTransformer2DModel                          # noqa: E402
from consolver_amd.pipeline import FluxKontextEditPipeline                        # noqa: E402
from consolver_amd.reward_model import load_reward_model                          # noqa: E402
from consolver_amd.synth import synthetic_dinov2_state_dict, synthetic_flux_state_dict, synthetic_vae_state_dict     # noqa: E402
from consolver_amd.vae import FLUX_VAE_CONFIG, HipAutoencoderKL                   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--steps", type=int, nargs="+", default=[2, 3, 4, 5])
    ap.add_argument("--rewards", nargs="+", default=["image_psnr", "dino"])
    ap.add_argument("--forward-batch-size", type=int, default=None, help="at most this many rows per DiT call (when the full batch does not fit)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.batch
    t0 = time.perf_counter()
    dit = HipFluxTransformer2DModel(device=dev)
    dit.load_state_dict(synthetic_flux_state_dict(dit.manifest(), device=dev, dtype=dit.dtype))
    vae = HipAutoencoderKL(dict(FLUX_VAE_CONFIG, with_encoder=True), device=dev)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest()))
    S = vae.config.sample_size
    sch = gf.make_scheduler("consistencysolver")                                   # order_dim 2, scaler_dim 0, mu_dim 0, hidden 256, 11 bins
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in sch.factor_net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3 / max(1.0, p.shape[-1] ** 0.5))
        sch.factor_net.mlp[4].weight.mul_(0.05)
    sch.factor_net.to(dev)
    base = gf.make_scheduler("euler")
    pipe = FluxKontextEditPipeline(dit, sch, vae)
    tr = ppo.PolicyTrainer(sch.factor_net, lr=1e-4)
    models = {"image_psnr": (None, None)}
    if "dino" in args.rewards:
        dino, proc = load_reward_model("dino", device=dev)
        dino.load_state_dict(synthetic_dinov2_state_dict(dino.manifest(), seed=7))
        models["dino"] = (dino, proc)
    L = (S // 2) ** 2
    rep = lambda t: t.to(dev).repeat(B, *[1] * (t.dim() - 1))
    ref = torch.rand(1, 3, 8 * S, 8 * S, generator=g)
    batch = (rep(ref * 2 - 1), ["synthetic instruction"] * B, rep(torch.randn(1, L, 64, generator=g).to(torch.bfloat16)),
             rep((torch.randn(1, L, 64, generator=g) * 0.6).to(torch.bfloat16)), rep(ref))
    emb = {"prompt_embeds": rep(torch.randn(1, 512, dit.config["joint_attention_dim"], generator=g).to(torch.bfloat16)),
           "pooled_prompt_embeds": rep(torch.randn(1, dit.config["pooled_projection_dim"], generator=g).to(torch.bfloat16))}
    torch.cuda.synchronize()
    print(f"models ready in {time.perf_counter() - t0:.1f} s", flush=True)

    def iteration(n, shared, reward):
        model, proc = models[reward]
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = ppo_flux.train_iteration_flux(tr, pipe, sch, base, batch, num_inference_steps=n, ppo_epochs=4, reward_type=reward, reward_model=model,
                                            reward_model_processor=proc, share_identical=shared, text_embeds=emb,
                                            forward_batch_size=args.forward_batch_size)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    for shared in (False, True):                                                   # warm-up: workspaces, first launches
        iteration(2, shared, args.rewards[0])
    ms, rows, last = {}, {}, {}
    for rnd in range(args.rounds):
        for reward in args.rewards:
            for n in args.steps:
                for shared in (False, True):                                       # alternated: both modes see the same clocks
                    t, out = iteration(n, shared, reward)
                    ms.setdefault((reward, n, shared), []).append(t)
                    rows[n, shared] = out["forward_rows"]
                    last[reward, n, shared] = out
        print(f"round {rnd} done", flush=True)
    lines = [f"FLUX-Kontext PPO iteration (ppo_flux.train_iteration_flux), tools/bench_flux_rollout.py, one MI355X (gfx950), bf16 DiT (full size, synthetic "
             f"weights), FLUX VAE, {8 * S} x {8 * S}",
             f"B = {B} copies of one teacher pair, order_dim 2, scaler_dim 0, 4 PPO epochs, plain-Euler baseline row in the same loop; identical_inputs off / on "
             f"alternated within each of {args.rounds} rounds, median (min ... max) of wall-clock ms per iteration",
             f"forward_batch_size = {args.forward_batch_size or 'none (all rows of a forward in one DiT call)'}",
             "rows: DiT rows run per iteration (sum of forward_rows); 'reference' = the reference's two full rollouts, n (B + 1)"]
    records = []
    for reward in args.rewards:
        lines.append(f"  reward {reward}")
        for n in args.steps:
            off, on = ms[reward, n, False], ms[reward, n, True]
            r_off, r_on = sum(rows[n, False]), sum(rows[n, True])
            m_off, m_on = statistics.median(off), statistics.median(on)
            lines.append(f"    n = {n}: rows {n * (B + 1):3d} reference, {r_off:3d} off, {r_on:3d} on (on / off {r_on / r_off:.3f})   "
                         f"ms off {m_off:8.1f} ({min(off):.1f} ... {max(off):.1f})   on {m_on:8.1f} ({min(on):.1f} ... {max(on):.1f})   on / off {m_on / m_off:.3f}")
            records.append({"reward": reward, "n": n, "B": B, "rows_reference": n * (B + 1), "forward_rows_off": rows[n, False], "forward_rows_on": rows[n, True],
                            "ms_off": off, "ms_on": on, "ms_ratio": m_on / m_off, "row_ratio": r_on / r_off,
                            "reward_mean_on": float(last[reward, n, True]["reward"]), "reward_base_on": float(last[reward, n, True]["reward_base"]),
                            "loss_on": float(last[reward, n, True]["loss"])})
    lines.append("  not measured: real checkpoints (synthetic weights everywhere), more than one GPU, the data loader (the batch is resident)")
    text = "\n".join(lines + [json.dumps(r) for r in records]) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
