"""Grouped against ungrouped SD1.5 PPO rollout at run_ppo.sh's settings, in one process, the two modes alternating: B = 80 copies of one sample, 11 bins,
order_dim 4, scaler_dim 0, CFG 3, full-size synthetic UNet / VAE, a zero-initialised (uniform) policy, the same seed for both modes of a repetition (so both
draw the same actions).  Measures n = 3 and n = 8: ``forward_rows``, the rollout time, and for n = 8 the whole ``ppo.train_iteration`` with ``image_psnr``
(1 PPO epoch as in run_ppo.sh, learning rate 0 so that the policy stays uniform over the repetitions).  Checks that the row counts are the number of distinct
action histories in front of each forward and that both modes return the same records.  Writes ``profiles/sd_ppo_grouped_rollout.txt`` (``--out``).

    python tools/bench_sd_ppo.py [--reps 3] [--out profiles/sd_ppo_grouped_rollout.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import consolver_amd  # noqa: E402
from consolver_amd import ppo, rollout  # noqa: E402
from consolver_amd.synth import synthetic_prompt_embeds, synthetic_unet_state_dict, synthetic_vae_state_dict  # noqa: E402
from consolver_amd.unet import HipUNet2DConditionModel  # noqa: E402
from consolver_amd.vae import HipAutoencoderKL  # noqa: E402

B, K, CFG = 80, 11, 3.0


def expected_rows(actions, masks):
    """distinct action histories in front of each forward, from the records (scaler_dim 0: step 0 has no live action)"""
    acts = (actions * masks).cpu().tolist()                  # [B][n - 1][A]
    hist, rows = [()] * B, [1, 1]
    for i in range(len(acts[0])):
        hist = [h + tuple(acts[b][i]) for b, h in enumerate(hist)]
        rows.append(len(set(hist)))
    return rows[:len(acts[0]) + 1]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sd_ppo_grouped_rollout.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    unet = HipUNet2DConditionModel(device=dev)
    unet.load_state_dict(synthetic_unet_state_dict(unet.manifest()))
    vae = HipAutoencoderKL(device=dev)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest()))
    sch = consolver_amd.PPOScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing", order_dim=4, scaler_dim=0,
                                     factor_net_kwargs=dict(embedding_dim=1024, hidden_dim=256, num_actions=K))
    with torch.no_grad():
        for p in sch.factor_net.parameters():
            p.zero_()
    sch.factor_net.to(dev)
    trainer = ppo.PolicyTrainer(sch.factor_net, lr=0.0)
    g = torch.Generator().manual_seed(0)
    pe, ne = (synthetic_prompt_embeds(1, seed=s).half().to(dev).repeat(B, 1, 1) for s in (1001, 1002))
    noise = torch.randn(1, 4, 64, 64, generator=g).half().to(dev).repeat(B, 1, 1, 1)
    teacher = (torch.randn(1, 4, 64, 64, generator=g) * 0.18215).half().to(dev).repeat(B, 1, 1, 1)
    batch = (["p"] * B, noise, teacher)

    def roll(n, grouped, seed):
        torch.manual_seed(seed)
        stats = {}
        out = rollout.denoise_diffusion(None, sch, unet, noise, ["p"] * B, None, cfg=CFG, num_inference_steps=n, prompt_embeds=pe, negative_prompt_embeds=ne,
                                        identical_inputs=True, group_rows=grouped, stats=stats)
        return out, stats["forward_rows"]

    def iteration(grouped, seed):
        torch.manual_seed(seed)
        return ppo.train_iteration(trainer, None, sch, unet, vae, batch, None, cfg=CFG, num_inference_steps=8, ppo_epochs=1, reward_type="image_psnr",
                                   prompt_embeds=pe, negative_prompt_embeds=ne, group_rows=grouped, share_target=grouped)

    lines = [f"SD1.5 PPO rollout, grouped against ungrouped, one process, modes alternating; {torch.cuda.get_device_name(0)}",
             f"B = {B} copies of one sample, {K} bins, order_dim 4, scaler_dim 0, CFG {CFG:g}, full-size synthetic UNet and VAE, uniform policy, {args.reps} repetitions",
             "times: host clock around the call, device synchronised before and after; ms; median (min .. max)", ""]
    ok = True
    for n in (3, 8):
        for grouped in (False, True):                        # every shape of the timed window once, untimed
            roll(n, grouped, 100)
        t = {False: [], True: []}
        rows = {False: [], True: []}
        for r in range(args.reps):
            outs = {}
            for grouped in ((False, True) if r % 2 == 0 else (True, False)):
                (out, fr), ms = timed(lambda: roll(n, grouped, r))
                t[grouped].append(ms)
                rows[grouped].append(fr)
                outs[grouped] = out
            same = all(torch.equal(outs[False][k], outs[True][k]) for k in (2, 3, 4)) and torch.equal(outs[False][1]["x"], outs[True][1]["x"])
            want = expected_rows(outs[True][3], outs[True][4])
            rule = rows[True][-1] == want
            rel = float((outs[True][0].float() - outs[False][0].float()).norm() / outs[False][0].float().norm())
            lines.append(f"n = {n} rep {r}: forward_rows grouped {rows[True][-1]} ungrouped {rows[False][-1]}; distinct histories {want}: "
                         f"{'match' if rule else 'MISMATCH'}; records equal: {same}; latents rel-L2 grouped vs ungrouped {rel:.3e}")
            ok = ok and same and rule
        med = {m: statistics.median(t[m]) for m in t}
        for m in (False, True):
            lines.append(f"n = {n} rollout {'grouped  ' if m else 'ungrouped'}: {med[m]:9.1f} ({min(t[m]):.1f} .. {max(t[m]):.1f}); denoiser rows per rollout "
                         f"{statistics.mean(sum(fr) for fr in rows[m]):.1f}")
        lines.append(f"n = {n} rollout grouped / ungrouped: {med[True] / med[False]:.3f}")
        ok = ok and med[True] <= med[False]
        lines.append("")
    for grouped in (False, True):
        iteration(grouped, 100)
    t = {False: [], True: []}
    for r in range(args.reps):
        for grouped in ((False, True) if r % 2 == 0 else (True, False)):
            out, ms = timed(lambda: iteration(grouped, r))
            t[grouped].append(ms)
    med = {m: statistics.median(t[m]) for m in t}
    for m in (False, True):
        lines.append(f"n = 8 train_iteration (rollout, 80 + 1 decodes, image_psnr, 1 PPO epoch) {'grouped + shared target' if m else 'ungrouped, tiled target  '}: "
                     f"{med[m]:9.1f} ({min(t[m]):.1f} .. {max(t[m]):.1f})")
    lines.append(f"n = 8 train_iteration grouped / ungrouped: {med[True] / med[False]:.3f}")
    lines += ["", "not measured here: more than one GPU, real checkpoints, the depth reward at full size"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if not ok:
        raise SystemExit("the row counts, the records or the times are not what the grouping promises: see above")


if __name__ == "__main__":
    main()
