"""Times the CLIP reward (reward_type "clip") for B pred / target pairs at 512 x 512 fp16, split into front end (quantise + PIL-exact resize + crop +
normalise + patch rows), tower (embeddings + pre_layrnorm, 24 layers at 257 tokens per image, post_layernorm + projection) and tail (normalise, cosine,
scale).  Synthetic weights; medians of ``--reps`` runs after ``--warmup``; the tower's rate as a fraction of the fp16 MFMA peak from ``flops()``; one JSON
line at the end.

    python tools/bench_clip_reward.py [--batch 16] [--reps 7] [--out profiles/clip_reward_bench.txt]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from consolver_amd.reward_model import load_reward_model, cosine_reward
from consolver_amd.synth import synthetic_clip_vision_state_dict

DEV = "cuda:0"
PEAK_F16_TFLOPS = 2500.0


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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, n = a.batch, 2 * a.batch
    model, proc = load_reward_model("clip", device=DEV)
    model.load_state_dict(synthetic_clip_vision_state_dict(model.manifest()))
    images = torch.rand(n, 3, a.size, a.size, device=DEV, dtype=torch.float16)
    patches = model.preprocess(images)
    feats = model.encode_patches(patches)
    res = {"batch_pairs": B, "images": n, "size": a.size}
    res["front_end_ms"] = timed(lambda: model.preprocess(images), a.warmup, a.reps)
    res["tower_ms"] = timed(lambda: model.encode_patches(patches), a.warmup, a.reps)
    res["tail_ms"] = timed(lambda: cosine_reward(feats[:B], feats[B:]), a.warmup, a.reps)
    res["reward_total_ms"] = res["front_end_ms"] + res["tower_ms"] + res["tail_ms"]
    res["tower_tflop"] = model.flops(n) / 1e12
    res["tower_tflops"] = model.flops(n) / res["tower_ms"] / 1e9
    res["tower_frac_of_fp16_mfma_peak"] = res["tower_tflops"] / PEAK_F16_TFLOPS
    lines = [f"clip reward, {n} images ({B} pred + {B} target) at {a.size}^2 fp16, ViT-L/14, synthetic weights, medians of {a.reps}",
             f"  front end  {res['front_end_ms']:9.3f} ms",
             f"  tower      {res['tower_ms']:9.3f} ms  ({res['tower_tflop']:.2f} TFLOP, {res['tower_tflops']:.0f} TFLOP/s, "
             f"{100 * res['tower_frac_of_fp16_mfma_peak']:.1f} % of the fp16 MFMA peak)",
             f"  tail       {res['tail_ms']:9.3f} ms", f"  total      {res['reward_total_ms']:9.3f} ms"]
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
