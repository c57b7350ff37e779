"""Times the DINOv2 reward (reward_type "dino") on config 5's batch: 80 predicted + 80 teacher images at 512 x 512 fp16, split into front end
(quantise + PIL-exact resize + crop + normalise + patch rows), encoder (12 layers, 257 tokens per image) and tail (normalise, cosine, scale), and, in the
same process, the VAE decode of those 160 images for scale.  Synthetic weights; medians of ``--reps`` runs after ``--warmup``; one JSON line at the end.

    python tools/bench_dino_reward.py [--batch 80] [--reps 7] [--out profiles/dino_reward_bench.txt]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from consolver_amd.reward_model import load_reward_model, cosine_reward
from consolver_amd.synth import synthetic_dinov2_state_dict, synthetic_vae_state_dict
from consolver_amd.vae import HipAutoencoderKL, decode_latents

DEV = "cuda:0"


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-vae", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, n = a.batch, 2 * a.batch
    model, proc = load_reward_model("dino", device=DEV)
    model.load_state_dict(synthetic_dinov2_state_dict(model.manifest()))
    images = torch.rand(n, 3, a.size, a.size, device=DEV, dtype=torch.float16)
    patches = model.preprocess(images)
    feats = model.encode_patches(patches)
    res = {"batch_pairs": B, "images": n, "size": a.size}
    res["front_end_ms"] = timed(lambda: model.preprocess(images), a.warmup, a.reps)
    res["encoder_ms"] = timed(lambda: model.encode_patches(patches), a.warmup, a.reps)
    res["tail_ms"] = timed(lambda: cosine_reward(feats[:B], feats[B:]), a.warmup, a.reps)
    res["reward_total_ms"] = res["front_end_ms"] + res["encoder_ms"] + res["tail_ms"]
    res["encoder_tflop"] = model.flops(n) / 1e12
    res["encoder_tflops"] = model.flops(n) / res["encoder_ms"] / 1e9
    if not a.no_vae:
        vae = HipAutoencoderKL({}, device=DEV)
        vae.load_state_dict(synthetic_vae_state_dict(vae.manifest()))
        lat = torch.randn(n, 4, a.size // 8, a.size // 8, device=DEV, dtype=torch.float16) * 0.18
        res["vae_decode_ms"] = timed(lambda: decode_latents(vae, lat, 8), 1, 3)
        res["vae_decode_tflop"] = vae.flops(n) / 1e12
        res["reward_over_decode"] = res["reward_total_ms"] / res["vae_decode_ms"]
    lines = [f"dino reward, {n} images ({B} pred + {B} target) at {a.size}^2 fp16, synthetic weights, medians of {a.reps}",
             f"  front end  {res['front_end_ms']:9.3f} ms", f"  encoder    {res['encoder_ms']:9.3f} ms  ({res['encoder_tflop']:.2f} TFLOP, {res['encoder_tflops']:.0f} TFLOP/s)",
             f"  tail       {res['tail_ms']:9.3f} ms", f"  total      {res['reward_total_ms']:9.3f} ms"]
    if not a.no_vae:
        lines.append(f"  VAE decode of the same {n} images {res['vae_decode_ms']:9.3f} ms ({res['vae_decode_tflop']:.0f} TFLOP): reward / decode = {res['reward_over_decode']:.3f}")
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
