"""Writes tests/golden/depth_reward_hw.npz: the Depth Anything depth-PSNR reward on NON-SQUARE images evaluated by the INSTALLED third-party packages -- PIL's
resize through transformers' DPTImageProcessor (the PIL class; ``keep_aspect_ratio``, ``ensure_multiple_of = 14``), transformers'
DepthAnythingForDepthEstimation on the reduced config of tools/make_depth_golden.py (its position table interpolated by transformers to the image's patch
grid), and the processor's post_process_depth_estimation.  Everything that is not about the aspect ratio -- weights, processor, models, the stored fields and
the fixture conditions -- is that tool's.  Host only.

Cases: (name, processor size, image height, image width, dtype).  The processed sizes and patch grids:
    s126_h64x96   126   64 x  96 fp16 ->  84 x 126   6 x 9   (both axes up; maps 24x36 / 12x18 / 6x9 / 3x5)
    s126_f100x36  126  100 x  36 fp32 -> 126 x  42   9 x 3   (both axes up on a 1:2.8 image; the training grid's height; maps 36x12 / 18x6 / 9x3 / 5x2)
    s70_h96x64     70   96 x  64 fp16 -> 112 x  70   8 x 5   (height up past the processor's size: 105 / 14 = 7.5 rounds half-even to 8)
    s70_f150x90    70  150 x  90 fp32 -> 112 x  70   8 x 5   (both axes down)
(100 x 36 at size 70 gives a 5 x 2 grid whose coarsest map is one column wide: torch's bf16 evaluation of that graph is ill-conditioned there -- relative
errors of 0.3 and NaN on the first seeds tried -- so it cannot serve as the comparator and the case is not stored; the front-end tests cover that input.)
Per case a pred image and a target = pred + noise; stored as tools/make_depth_golden.py stores them.

Fixture conditions (asserted, as there): for every fp32 reference map the share of pixels <= 0 after the bicubic step is at most 0.5, max - min >= 1.0, and the
reward lies in (5, 40) -- so the torch-bf16 comparator stored next to each case is itself well-conditioned.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("s126_h64x96", 126, 64, 96, "float16"), ("s126_f100x36", 126, 100, 36, "float32"), ("s70_h96x64", 70, 96, 64, "float16"),
         ("s70_f150x90", 70, 150, 90, "float32"))
IMAGE_SEEDS = (100, 100, 100, 100)      # tests.vit_oracle.synthetic_image seeds (one per case) whose fp32 reference maps meet the fixture conditions
TARGET_NOISE = 0.15


def base():
    """tools/make_depth_golden.py: the reduced config, the seeded weights, the installed processor and models"""
    spec = importlib.util.spec_from_file_location("make_depth_golden", os.path.join(ROOT, "tools", "make_depth_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_images(i, h, w, dtype, seed=None):
    """(pred, target) [3,h,w] in [0,1]"""
    from tests.vit_oracle import synthetic_image
    seed = IMAGE_SEEDS[i] if seed is None else seed
    pred = synthetic_image(seed, h, w, torch.float32)
    g = torch.Generator().manual_seed(seed + 100)
    target = (pred + TARGET_NOISE * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    return pred.to(getattr(torch, dtype)), target.to(getattr(torch, dtype))


def conditions(raw, reward):
    """(zero share, range, reward) of the reference's raw maps [2,H,W] and whether they meet the fixture conditions"""
    mn, mx = raw.amin((1, 2)), raw.amax((1, 2))
    zero_share, rng = float((raw <= 0).float().mean((1, 2)).max()), float((mx - mn).min())
    return (zero_share, rng, float(reward)), zero_share <= 0.5 and rng >= 1.0 and 5.0 < float(reward) < 40.0


def build_case(b, models, i, name, size, h, w, dtype, seed=None):
    """the stored fields of one case, and its fixture conditions"""
    from PIL import Image
    from tests import depth_oracle as do
    from tests import vit_oracle as vo
    if size not in models:
        sd = b.state_dict(size)
        models[size] = (b.hf_model(b.reduced_config(size), sd), b.hf_model(b.reduced_config(size), sd).to(torch.bfloat16), b.hf_processor(size))
    model, model_bf16, proc = models[size]
    pils = [Image.fromarray(vo.to_uint8_hwc(t)) for t in case_images(i, h, w, dtype, seed)]
    pv = proc(images=pils, return_tensors="pt")["pixel_values"]
    u8 = proc(images=pils, return_tensors="pt", do_rescale=False, do_normalize=False)["pixel_values"]
    o = model(pixel_values=pv)
    post = proc.post_process_depth_estimation(o, target_sizes=[(h, w)] * 2)
    raw = torch.stack([p["predicted_depth"] for p in post]).float()
    mn, mx = raw.amin((1, 2), keepdim=True), raw.amax((1, 2), keepdim=True)
    maps = (raw - mn) / (mx - mn + 1e-8)
    reward = do.depth_reward(maps[:1], maps[1:])
    ob = model_bf16(pixel_values=pv.to(torch.bfloat16)).predicted_depth
    maps_b = do.normalized_maps(ob.float(), h, w)
    reward_b = do.depth_reward(maps_b[:1], maps_b[1:])
    out = {f"{name}_size": np.array(pv.shape[-2:], np.int64),
           f"{name}_u8": u8[0].numpy().astype(np.uint8),
           f"{name}_depth": o.predicted_depth.numpy().astype(np.float32),
           f"{name}_maps": maps.numpy().astype(np.float32),
           f"{name}_reward": reward.numpy().astype(np.float32),
           f"{name}_depth_bf16": ob.view(torch.int16).numpy().view(np.uint16),
           f"{name}_reward_bf16": reward_b.numpy().astype(np.float32),
           f"{name}_bf16_errors": np.array([b.rel_l2(ob.float(), o.predicted_depth), b.rel_l2(maps_b, maps), float((reward_b - reward).abs().max())], np.float64)}
    return out, conditions(raw, reward)


def build_fixture():
    b = base()
    out = {"weight_seed": np.array(b.WEIGHT_SEED, np.int64), "cases": np.array([c[0] for c in CASES])}
    models = {}
    with torch.no_grad():
        for i, (name, size, h, w, dtype) in enumerate(CASES):
            fields, ((zero_share, rng, reward), ok) = build_case(b, models, i, name, size, h, w, dtype)
            assert ok, (name, zero_share, rng, reward)
            out.update(fields)
            e = fields[name + "_bf16_errors"]
            print(f"{name}: processed {tuple(int(v) for v in fields[name + '_size'])} zero share {zero_share:.3f} range {rng:.3f} reward {reward:.4f} | bf16: depth rel-L2 {e[0]:.3e} "
                  f"maps rel-L2 {e[1]:.3e} reward error {e[2]:.3e}")
    return out


def main():
    path = os.path.join(ROOT, "tests", "golden", "depth_reward_hw.npz")
    np.savez_compressed(path, **build_fixture())
    print("depth_reward_hw.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
