"""Times one of the model rewards of the PPO trainer on a batch of predicted + teacher images at 512 x 512 fp16, split into its stages.  Synthetic weights;
medians of ``--reps`` runs after ``--warmup``; one JSON line at the end.

    python tools/bench_reward.py --reward dino  [--batch 80] [--reps 7] [--no-vae] [--out profiles/dino_reward_bench.txt]
    python tools/bench_reward.py --reward clip  [--batch 16] [--reps 7] [--out profiles/clip_reward_bench.txt]
    python tools/bench_reward.py --reward depth [--batch 8]  [--reps 7] [--height 880 --width 1184] [--out profiles/depth_reward_bench.txt]
    python tools/bench_reward.py --reward segmentation [--batch 4] [--reps 7] [--height 880 --width 1184] [--out profiles/segmentation_reward_bench.txt]
    python tools/bench_reward.py --reward inception [--batch 4] [--reps 7] [--out profiles/inception_reward_bench.txt]

* ``dino`` (config 5's batch, 80 + 80 images): front end (quantise + PIL-exact resize + crop + normalise + patch rows), encoder (12 layers, 257 tokens per
  image), tail (normalise, cosine, scale) and, in the same process, the VAE decode of those 160 images for scale.
* ``clip``: the same front end, the tower (embeddings + pre_layrnorm, 24 layers at 257 tokens per image, post_layernorm + projection) with its rate as a
  fraction of the fp16 MFMA peak from ``flops()``, the tail.
* ``depth``: front end (resize to 518 x 518), model (DINOv2-small backbone at 1370 tokens tapped four times, DPT neck and head), post-processing (bicubic to
  512 x 512, min / max normalisation), tail (PSNR) and the whole ``calculate_depth_reward`` call.
* ``segmentation``: front end (bilinear resize to 512 x 512: the identity at this size), the MiT-B4 encoder stage by stage (the forward stopped after 1 .. 4
  stages, differenced), the head, argmax + agreement, the whole ``calculate_segmentation_reward`` call; and the depthwise 3x3 + GELU kernel alone at the
  stage-1 shape with the bytes it must move (input + output once) over its time, next to the HBM copy rate of the micro-architecture guide.
* ``inception``: front end (bicubic resize to 299 + crop), Inception-v3 part by part (the forward stopped after the stem, Mixed_5, Mixed_6, Mixed_7,
  differenced), the head, the whole ``calculate_inception_reward`` call; and the convolution kernel alone at three of the network's shapes with its rate.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from consolver_amd import synth
from consolver_amd.ppo import depth_psnr_tail
from consolver_amd import _lib as L
from consolver_amd.reward_model import (calculate_depth_reward, calculate_inception_reward, calculate_segmentation_reward, cosine_reward, load_depth_reward,
                                        load_inception_reward, load_reward_model, load_segmentation_reward, mask_agreement)

DEV = "cuda:0"
PEAK_F16_TFLOPS = 2500.0
HBM_COPY_TBS = 6.29                # measured float4 copy rate of the MI355X (8.0 TB/s spec)
DEFAULT_BATCH = {"dino": 80, "clip": 16, "depth": 8, "segmentation": 4, "inception": 4}


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


def image_hw(a):
    """--height / --width (depth and segmentation: any aspect ratio), each defaulting to --size"""
    return a.height or a.size, a.width or a.size


def random_images(a, n):
    h, w = image_hw(a)
    return torch.rand(n, 3, h, w, device=DEV, dtype=torch.float16)


def bench_features(a, res, B, n):
    """dino / clip: front end, encoder (clip: "tower"), cosine tail"""
    enc = "encoder" if a.reward == "dino" else "tower"
    model, _ = load_reward_model(a.reward, device=DEV)
    state_dict = synth.synthetic_dinov2_state_dict if a.reward == "dino" else synth.synthetic_clip_vision_state_dict
    model.load_state_dict(state_dict(model.manifest()))
    images = random_images(a, n)
    patches = model.preprocess(images)
    feats = model.encode_patches(patches)
    res["front_end_ms"] = timed(lambda: model.preprocess(images), a.warmup, a.reps)
    res[enc + "_ms"] = timed(lambda: model.encode_patches(patches), a.warmup, a.reps)
    res["tail_ms"] = timed(lambda: cosine_reward(feats[:B], feats[B:]), a.warmup, a.reps)
    res["reward_total_ms"] = res["front_end_ms"] + res[enc + "_ms"] + res["tail_ms"]
    res[enc + "_tflop"] = model.flops(n) / 1e12
    res[enc + "_tflops"] = model.flops(n) / res[enc + "_ms"] / 1e9
    rate = f"({res[enc + '_tflop']:.2f} TFLOP, {res[enc + '_tflops']:.0f} TFLOP/s"
    if a.reward == "clip":
        res["tower_frac_of_fp16_mfma_peak"] = res["tower_tflops"] / PEAK_F16_TFLOPS
        rate += f", {100 * res['tower_frac_of_fp16_mfma_peak']:.1f} % of the fp16 MFMA peak"
    lines = [f"  front end  {res['front_end_ms']:9.3f} ms", f"  {enc:<9s}  {res[enc + '_ms']:9.3f} ms  {rate})",
             f"  tail       {res['tail_ms']:9.3f} ms", f"  total      {res['reward_total_ms']:9.3f} ms"]
    if a.reward == "dino" and not a.no_vae:
        from consolver_amd.vae import HipAutoencoderKL, decode_latents
        vae = HipAutoencoderKL({}, device=DEV)
        vae.load_state_dict(synth.synthetic_vae_state_dict(vae.manifest()))
        lat = torch.randn(n, 4, a.size // 8, a.size // 8, device=DEV, dtype=torch.float16) * 0.18
        res["vae_decode_ms"] = timed(lambda: decode_latents(vae, lat, 8), 1, 3)
        res["vae_decode_tflop"] = vae.flops(n) / 1e12
        res["reward_over_decode"] = res["reward_total_ms"] / res["vae_decode_ms"]
        lines.append(f"  VAE decode of the same {n} images {res['vae_decode_ms']:9.3f} ms ({res['vae_decode_tflop']:.0f} TFLOP): reward / decode = {res['reward_over_decode']:.3f}")
    return lines


def bench_depth(a, res, B, n):
    model, proc = load_depth_reward(device=DEV)
    model.load_state_dict(synth.synthetic_depth_anything_state_dict(model.manifest()))
    images = random_images(a, n)
    h, w = image_hw(a)
    lines = []
    if h == w:                                          # the square entry points
        front_end, run = (lambda: model.preprocess(images)), model.depth_from_patches
        patches, flops = front_end(), model.flops
        res["workspace_mb_per_image"] = int(model._fn("workspace_bytes")(model._h, 1)) / 1e6
        res["calls_hold"] = model.max_batch
    else:                                               # the `_hw` entry points at the processed size of an h x w image
        size = model.processed_size(h, w)
        gh, gw = size[0] // model.patch, size[1] // model.patch
        front_end, run = (lambda: model.preprocess_hw(images)[0]), (lambda p: model.depth_from_patches_hw(p, size))
        patches, flops = front_end(), (lambda k: model.flops_hw(k, size))
        res["processed_size"], res["patch_grid"] = list(size), [gh, gw]
        res["workspace_mb_per_image"] = int(L.lib().cs_depth_workspace_bytes_hw(model._h, 1, size[0], size[1])) / 1e6
        res["calls_hold"] = max(1, min(model.max_batch, int(model.workspace_budget // (res["workspace_mb_per_image"] * 1e6))))
        # the position-table kernel alone, as a cache miss runs it (the handle keeps the table afterwards)
        D, s = model.config["hidden_size"], model.config["image_size"] // model.patch
        grid, table = torch.randn(s, s, D, device=DEV), torch.empty(1 + gh * gw, D, device=DEV, dtype=torch.float16)
        st = L.stream_ptr(DEV)
        res["position_table_kernel_ms"] = timed(lambda: L.check(L.lib().cs_op_vit_pos_interp(L.ptr(grid), s, gh, gw, D, L.ptr(table), st)), a.warmup, a.reps)
        lines.append(f"  {h} x {w} -> {size[0]} x {size[1]}: {gh} x {gw} = {gh * gw} patches against {s} x {s} = {s * s} at the processor's own size; position table "
                     f"{s} x {s} -> {gh} x {gw} on a cache miss: {res['position_table_kernel_ms']:.4f} ms (kernel alone)")
    depth = run(patches)
    maps = model.post_process(depth, h, w)
    res["max_batch"] = model.max_batch
    res["front_end_ms"] = timed(front_end, a.warmup, a.reps)
    res["model_ms"] = timed(lambda: run(patches), a.warmup, a.reps)
    res["post_process_ms"] = timed(lambda: model.post_process(depth, h, w), a.warmup, a.reps)
    res["tail_ms"] = timed(lambda: depth_psnr_tail(maps[:B], maps[B:]), a.warmup, a.reps)
    res["reward_call_ms"] = timed(lambda: calculate_depth_reward(model, proc, images[:B], images[B:], DEV), a.warmup, a.reps)
    res["model_tflop"] = flops(n) / 1e12
    res["model_tflops"] = flops(n) / res["model_ms"] / 1e9
    return lines + [f"  front end     {res['front_end_ms']:9.3f} ms",
                    f"  model         {res['model_ms']:9.3f} ms  ({res['model_tflop']:.2f} TFLOP, {res['model_tflops']:.0f} TFLOP/s)",
                    f"  post-process  {res['post_process_ms']:9.3f} ms", f"  tail          {res['tail_ms']:9.3f} ms",
                    f"  calculate_depth_reward, whole call {res['reward_call_ms']:9.3f} ms"]


def bench_segmentation(a, res, B, n):
    model, proc = load_segmentation_reward(device=DEV)
    model.load_state_dict(synth.synthetic_segformer_state_dict(model.manifest()))
    images = random_images(a, n)
    patches = model._front_end(images)                  # a non-square image is stretched to the processor's size: the model's shapes do not change
    _, masks = model._run(patches, False, True)
    lib = L.lib()
    res["max_batch"] = model.max_batch
    res["front_end_ms"] = timed(lambda: model._front_end(images), a.warmup, a.reps)
    upto = []
    try:
        for parts in range(1, 6):                      # the forward stopped after stage 1 .. 4, then with the head
            L.check(lib.cs_seg_set_stage_limit(model._h, parts))
            upto.append(timed(lambda: model._run(patches, False, False), a.warmup, a.reps))
    finally:
        L.check(lib.cs_seg_set_stage_limit(model._h, 5))
    for i in range(4):
        res[f"stage{i + 1}_ms"] = upto[i] - (upto[i - 1] if i else 0.0)
    res["head_ms"] = upto[4] - upto[3]
    res["model_ms"] = upto[4]
    res["argmax_agreement_ms"] = timed(lambda: (model._run(patches, False, True), mask_agreement(masks[:B], masks[B:])), a.warmup, a.reps) - upto[4]
    res["reward_call_ms"] = timed(lambda: calculate_segmentation_reward(model, proc, images[:B], images[B:], DEV), a.warmup, a.reps)
    res["model_tflop"] = model.flops(n) / 1e12
    res["model_tflops"] = model.flops(n) / res["model_ms"] / 1e9
    res["workspace_mb_per_image"] = int(model._fn("workspace_bytes")(model._h, 1)) / 1e6
    # the depthwise 3x3 + GELU kernel alone at the stage-1 shape: [n][size / 4][size / 4][4 * 64] halfs in, the same out
    g, C = model.grid, 4 * model.config["hidden_sizes"][0]
    x = torch.randn(n, g, g, C, device=DEV, dtype=torch.float16)
    w, bias, out = torch.randn(9, C, device=DEV, dtype=torch.float16) / 3, torch.randn(C, device=DEV, dtype=torch.float16), torch.empty_like(x)
    st = L.stream_ptr(DEV)
    res["dwconv_stage1_ms"] = timed(lambda: L.check(lib.cs_op_seg_dwconv_gelu(L.ptr(x), n, g, g, C, L.ptr(w), L.ptr(bias), L.ptr(out), st)), a.warmup, a.reps)
    res["dwconv_stage1_mbytes"] = 2 * x.numel() * 2 / 1e6
    res["dwconv_stage1_tbs"] = res["dwconv_stage1_mbytes"] / res["dwconv_stage1_ms"] / 1e3
    res["hbm_copy_tbs"] = HBM_COPY_TBS
    return [f"  front end     {res['front_end_ms']:9.3f} ms"] + [f"  stage {i + 1}       {res[f'stage{i + 1}_ms']:9.3f} ms" for i in range(4)] + [
        f"  head          {res['head_ms']:9.3f} ms",
        f"  model         {res['model_ms']:9.3f} ms  ({res['model_tflop']:.2f} TFLOP, {res['model_tflops']:.0f} TFLOP/s)",
        f"  argmax + agreement {res['argmax_agreement_ms']:9.3f} ms",
        f"  calculate_segmentation_reward, whole call {res['reward_call_ms']:9.3f} ms",
        f"  depthwise 3x3 + GELU alone, [{n}][{g}][{g}][{C}]: {res['dwconv_stage1_ms']:.4f} ms for {res['dwconv_stage1_mbytes']:.1f} MB in + out = "
        f"{res['dwconv_stage1_tbs']:.2f} TB/s (HBM copy rate of the micro-architecture guide: {HBM_COPY_TBS} TB/s measured, 8.0 spec; a tensor of this size can "
        f"stay in the 256 MB Infinity Cache between two calls)"]


def bench_inception(a, res, B, n):
    model, proc = load_inception_reward(device=DEV)
    model.load_state_dict(synth.synthetic_inception_state_dict(model.manifest()))
    images = random_images(a, n)
    patches = model.preprocess(images)
    feats = model.encode_patches(patches)
    lib = L.lib()
    res["max_batch"] = model.max_batch
    res["front_end_ms"] = timed(lambda: model.preprocess(images), a.warmup, a.reps)
    upto, names = [], ("stem", "mixed_5", "mixed_6", "mixed_7", "head")
    try:
        for parts in range(1, 6):                      # the forward stopped after the stem, Mixed_5, Mixed_6, Mixed_7, then with the head
            L.check(lib.cs_incep_set_stage_limit(model._h, parts))
            upto.append(timed(lambda: model.encode_patches(patches), a.warmup, a.reps))
    finally:
        L.check(lib.cs_incep_set_stage_limit(model._h, 5))
    for i, k in enumerate(names):
        res[k + "_ms"] = upto[i] - (upto[i - 1] if i else 0.0)
    res["model_ms"] = upto[4]
    res["tail_ms"] = timed(lambda: cosine_reward(feats[:B], feats[B:]), a.warmup, a.reps)
    res["reward_call_ms"] = timed(lambda: calculate_inception_reward(model, proc, images[:B], images[B:], DEV), a.warmup, a.reps)
    res["model_tflop"] = model.flops(n) / 1e12
    res["model_tflops"] = model.flops(n) / res["model_ms"] / 1e9
    res["workspace_mb_per_image"] = int(model._fn("workspace_bytes")(model._h, 1)) / 1e6
    lines = [f"  front end     {res['front_end_ms']:9.3f} ms"] + [f"  {k:<12s}  {res[k + '_ms']:9.3f} ms" for k in names] + [
        f"  model         {res['model_ms']:9.3f} ms  ({res['model_tflop']:.3f} TFLOP, {res['model_tflops']:.1f} TFLOP/s)",
        f"  tail          {res['tail_ms']:9.3f} ms",
        f"  calculate_inception_reward, whole call {res['reward_call_ms']:9.3f} ms"]
    # the convolution kernel alone at three shapes of the network: (grid, Cin, Cout, kh, kw, stride, pad_h, pad_w)
    st = L.stream_ptr(DEV)
    for name, (g, ci, co, kh, kw, stride, ph, pw) in (("conv2b_3x3_147", (147, 32, 64, 3, 3, 1, 1, 1)), ("mixed5_3x3_35", (35, 96, 96, 3, 3, 1, 1, 1)),
                                                      ("mixed6_1x7_17", (17, 192, 192, 1, 7, 1, 0, 3)), ("mixed7_1x1_8", (8, 2048, 448, 1, 1, 1, 0, 0))):
        x = torch.randn(n, g, g, ci, device=DEV, dtype=torch.float16)
        w = torch.randn(co, kh * kw, ci, device=DEV, dtype=torch.float16) / (kh * kw * ci) ** 0.5
        bias = torch.randn(co, device=DEV)
        go = (g + 2 * ph - kh) // stride + 1
        out = torch.empty(n * go * go, co, device=DEV, dtype=torch.float16)
        ms = timed(lambda: L.check(lib.cs_op_incep_conv(L.ptr(x), n, g, g, ci, ci, L.ptr(w), L.ptr(bias), co, kh, kw, stride, ph, pw, L.ptr(out), co, 0, st)),
                   a.warmup, a.reps)
        res[f"conv_{name}_ms"] = ms
        res[f"conv_{name}_tflops"] = 2.0 * n * go * go * co * ci * kh * kw / ms / 1e9
        lines.append(f"  conv kernel alone, {name}: [{n}][{g}][{g}][{ci}] -> {co}, {kh} x {kw}: {ms:.4f} ms = {res[f'conv_{name}_tflops']:.1f} TFLOP/s")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reward", choices=sorted(DEFAULT_BATCH), required=True)
    ap.add_argument("--batch", type=int, default=None, help="pred / target pairs (default: 80 dino, 16 clip, 8 depth, 4 segmentation, 4 inception)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--height", type=int, default=None, help="depth / segmentation: image height (default --size)")
    ap.add_argument("--width", type=int, default=None, help="depth / segmentation: image width (default --size)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-vae", action="store_true", help="dino: skip the VAE decode of the same images")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = a.batch if a.batch is not None else DEFAULT_BATCH[a.reward]
    n = 2 * B
    h, w = image_hw(a)
    res = {"batch_pairs": B, "images": n, "size": a.size, "height": h, "width": w}
    stages = {"depth": bench_depth, "segmentation": bench_segmentation, "inception": bench_inception}.get(a.reward, bench_features)(a, res, B, n)
    model_name = {"clip": ", ViT-L/14", "segmentation": ", SegFormer-B4", "inception": ", Inception-v3 at 299"}.get(a.reward, "")
    shape = f"{h}^2" if h == w else f"{h} x {w}"
    lines = [f"{a.reward} reward, {n} images ({B} pred + {B} target) at {shape} fp16{model_name}, synthetic weights, medians of {a.reps}"] + stages
    lines.append(json.dumps(res))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
