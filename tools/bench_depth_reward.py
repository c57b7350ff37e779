"""Times the Depth Anything depth-PSNR reward (reward_type "depth") on a batch of predicted + teacher images at 512 x 512 fp16, split into front end
(quantise + PIL-exact resize to 518 x 518 + normalise + patch rows), model (DINOv2-small backbone at 1370 tokens tapped four times, DPT neck and head),
post-processing (bicubic to 512 x 512, min / max normalisation) and tail (PSNR).  Synthetic weights; medians of ``--reps`` runs after ``--warmup``; one JSON
line at the end.

    python tools/bench_depth_reward.py [--batch 8] [--reps 7] [--out profiles/depth_reward_bench.txt]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from consolver_amd.ppo import depth_psnr_tail
from consolver_amd.reward_model import calculate_depth_reward, load_depth_reward
from consolver_amd.synth import synthetic_depth_anything_state_dict

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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, n = a.batch, 2 * a.batch
    model, proc = load_depth_reward(device=DEV)
    model.load_state_dict(synthetic_depth_anything_state_dict(model.manifest()))
    images = torch.rand(n, 3, a.size, a.size, device=DEV, dtype=torch.float16)
    patches = model.preprocess(images)
    depth = model.depth_from_patches(patches)
    maps = model.post_process(depth, a.size, a.size)
    res = {"batch_pairs": B, "images": n, "size": a.size, "max_batch": model.max_batch}
    res["front_end_ms"] = timed(lambda: model.preprocess(images), a.warmup, a.reps)
    res["model_ms"] = timed(lambda: model.depth_from_patches(patches), a.warmup, a.reps)
    res["post_process_ms"] = timed(lambda: model.post_process(depth, a.size, a.size), a.warmup, a.reps)
    res["tail_ms"] = timed(lambda: depth_psnr_tail(maps[:B], maps[B:]), a.warmup, a.reps)
    res["reward_call_ms"] = timed(lambda: calculate_depth_reward(model, proc, images[:B], images[B:], DEV), a.warmup, a.reps)
    res["model_tflop"] = model.flops(n) / 1e12
    res["model_tflops"] = model.flops(n) / res["model_ms"] / 1e9
    res["workspace_mb_per_image"] = int(model._fn("workspace_bytes")(model._h, 1)) / 1e6
    lines = [f"depth reward, {n} images ({B} pred + {B} target) at {a.size}^2 fp16, synthetic weights, medians of {a.reps}",
             f"  front end     {res['front_end_ms']:9.3f} ms",
             f"  model         {res['model_ms']:9.3f} ms  ({res['model_tflop']:.2f} TFLOP, {res['model_tflops']:.0f} TFLOP/s)",
             f"  post-process  {res['post_process_ms']:9.3f} ms", f"  tail          {res['tail_ms']:9.3f} ms",
             f"  calculate_depth_reward, whole call {res['reward_call_ms']:9.3f} ms", json.dumps(res)]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
