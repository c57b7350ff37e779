"""Writes tests/golden/depth_reward.npz: the Depth Anything depth-PSNR reward (edit_ppo/reward_model.py:92-96, 359-422) evaluated by the INSTALLED third-party
packages -- PIL's resize through transformers' DPTImageProcessor (the PIL class) with the published constants of depth-anything/Depth-Anything-V2-Small-hf,
transformers' DepthAnythingForDepthEstimation on a reduced config, and the processor's post_process_depth_estimation -- plus
tests/golden/depth_anything_v2_small_manifest.json (names / shapes of the V2-Small model).

The script depends on transformers and PIL only: ``ToPILImage`` (``x.mul(255).byte()``, torchvision) and the reward's tail arithmetic are restated
(tests/vit_oracle.py: to_uint8_hwc; tests/depth_oracle.py: depth_reward).  Weights and input images are seeded
(consolver_amd.synth.synthetic_depth_anything_state_dict, tests.vit_oracle.synthetic_image), so the fixture stores results, not inputs.  Host only.

Reduced config: hidden 128, 2 heads, 4 layers, out_indices (1, 2, 3, 4), reassemble_hidden_size 128; the position grid is the processor's size (no interpolation).
Cases: (name, processor size, image height = width, dtype).  Size 126 is a 9 x 9 patch grid (maps 36 / 18 / 9 / 5: the odd 9 -> 5 stride-2 conv and the 5 -> 9 sized
upsample), size 70 a 5 x 5 one (20 / 10 / 5 / 3).  Per case a pred image and a target = pred + noise.  Stored per case: the processor's uint8 resized image of pred,
``predicted_depth`` of both, the normalised maps at the images' size, the reward; and of the same graph evaluated by torch in bf16 (class comparator) its
``predicted_depth`` (bf16 bit patterns: lossless at half the size), its reward, and the relative L2 errors of its depth and of its normalised maps.

Fixture conditions (asserted; a degenerate oracle must not be written): the head ends in a ReLU and every map is min / max normalised, so a reference map that
is almost all zeros would make rounding noise the whole signal.  For every fp32 reference map: the share of pixels <= 0 after the bicubic step is at most 0.5,
max - min >= 1.0, and the reward lies in (5, 40).
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT_SEED = 11
CASES = (("s126_h64", 126, 64, "float16"), ("s126_f96", 126, 96, "float32"), ("s70_h96", 70, 96, "float16"), ("s70_f64", 70, 64, "float32"))
IMAGE_SEEDS = (100, 108, 102, 109)      # tests.vit_oracle.synthetic_image seeds whose fp32 reference maps meet the fixture conditions below (103 at size 70: zero share 0.86)
TARGET_NOISE = 0.15


def reduced_config(size):
    from tests.depth_oracle import REDUCED
    return dict(REDUCED, image_size=size)


def case_images(i, hw, dtype):
    """(pred, target) [3,hw,hw] in [0,1]"""
    from tests.vit_oracle import synthetic_image
    dt = getattr(torch, dtype)
    pred = synthetic_image(IMAGE_SEEDS[i], hw, hw, torch.float32)
    g = torch.Generator().manual_seed(IMAGE_SEEDS[i] + 100)
    target = (pred + TARGET_NOISE * torch.randn(3, hw, hw, generator=g)).clamp(0, 1)
    return pred.to(dt), target.to(dt)


def state_dict(size):
    from consolver_amd.synth import synthetic_depth_anything_state_dict
    from tests import depth_oracle as do
    return synthetic_depth_anything_state_dict(do.manifest(reduced_config(size)), seed=WEIGHT_SEED)


def hf_processor(size):
    try:
        from transformers.models.dpt.image_processing_pil_dpt import DPTImageProcessorPil as P
    except ImportError:
        from transformers import DPTImageProcessor as P
    from tests.depth_oracle import PROCESSOR as C
    return P(do_resize=True, size={"height": size, "width": size}, keep_aspect_ratio=True, ensure_multiple_of=14, resample=3, do_rescale=True,
             rescale_factor=C["rescale_factor"], do_normalize=True, image_mean=list(C["image_mean"]), image_std=list(C["image_std"]), do_pad=False)


def hf_config(cfg):
    from transformers import DepthAnythingConfig, Dinov2Config
    from tests.depth_oracle import DEPTH_ANYTHING_V2_SMALL
    c = dict(DEPTH_ANYTHING_V2_SMALL)
    c.update(cfg)
    bc = Dinov2Config(hidden_size=c["hidden_size"], num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"], mlp_ratio=c["mlp_ratio"],
                      image_size=c["image_size"], patch_size=c["patch_size"], layer_norm_eps=c["layer_norm_eps"], out_indices=list(c["out_indices"]),
                      apply_layernorm=True, reshape_hidden_states=False)
    return DepthAnythingConfig(backbone_config=bc, reassemble_hidden_size=c["hidden_size"], neck_hidden_sizes=list(c["neck_hidden_sizes"]),
                               fusion_hidden_size=c["fusion_hidden_size"], head_hidden_size=c["head_hidden_size"])


def hf_model(cfg, sd):
    from transformers import DepthAnythingForDepthEstimation
    m = DepthAnythingForDepthEstimation(hf_config(cfg)).eval()
    m.load_state_dict(sd, strict=True)
    return m


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def build_fixture():
    from PIL import Image
    from tests import depth_oracle as do
    from tests import vit_oracle as vo
    out = {"weight_seed": np.array(WEIGHT_SEED, np.int64), "cases": np.array([c[0] for c in CASES])}
    models = {}
    with torch.no_grad():
        for i, (name, size, hw, dtype) in enumerate(CASES):
            if size not in models:
                sd = state_dict(size)
                models[size] = (hf_model(reduced_config(size), sd), hf_model(reduced_config(size), sd).to(torch.bfloat16), hf_processor(size))
            model, model_bf16, proc = models[size]
            pils = [Image.fromarray(vo.to_uint8_hwc(t)) for t in case_images(i, hw, dtype)]
            pv = proc(images=pils, return_tensors="pt")["pixel_values"]
            u8 = proc(images=pils, return_tensors="pt", do_rescale=False, do_normalize=False)["pixel_values"]
            assert tuple(pv.shape) == (2, 3, size, size)
            o = model(pixel_values=pv)
            post = proc.post_process_depth_estimation(o, target_sizes=[(hw, hw)] * 2)
            raw = torch.stack([p["predicted_depth"] for p in post]).float()
            mn, mx = raw.amin((1, 2), keepdim=True), raw.amax((1, 2), keepdim=True)
            maps = (raw - mn) / (mx - mn + 1e-8)
            reward = do.depth_reward(maps[:1], maps[1:])
            # the fixture conditions
            zero_share, rng = float((raw <= 0).float().mean((1, 2)).max()), float((mx - mn).min())
            assert zero_share <= 0.5, (name, zero_share)
            assert rng >= 1.0, (name, rng)
            assert 5.0 < float(reward) < 40.0, (name, float(reward))
            ob = model_bf16(pixel_values=pv.to(torch.bfloat16)).predicted_depth
            maps_b = do.normalized_maps(ob.float(), hw, hw)
            reward_b = do.depth_reward(maps_b[:1], maps_b[1:])
            out[f"{name}_u8"] = u8[0].numpy().astype(np.uint8)
            out[f"{name}_depth"] = o.predicted_depth.numpy().astype(np.float32)
            out[f"{name}_maps"] = maps.numpy().astype(np.float32)
            out[f"{name}_reward"] = reward.numpy().astype(np.float32)
            out[f"{name}_depth_bf16"] = ob.view(torch.int16).numpy().view(np.uint16)
            out[f"{name}_reward_bf16"] = reward_b.numpy().astype(np.float32)
            out[f"{name}_bf16_errors"] = np.array([rel_l2(ob.float(), o.predicted_depth), rel_l2(maps_b, maps), float((reward_b - reward).abs().max())], np.float64)
            print(f"{name}: zero share {zero_share:.3f} range {rng:.3f} reward {float(reward):.4f} | bf16: depth rel-L2 {out[name + '_bf16_errors'][0]:.3e} "
                  f"maps rel-L2 {out[name + '_bf16_errors'][1]:.3e} reward error {out[name + '_bf16_errors'][2]:.3e}")
    return out


def write_manifest(path):
    """the tools/make_manifests.py format, from the executor's own manifest (cs_depth_create is host only)"""
    from consolver_amd.reward_model import HipDepthAnythingModel
    m = HipDepthAnythingModel(device="cpu").manifest()
    n = sum(int(math.prod(s)) for _, s in m)
    with open(path, "w") as f:
        json.dump({"params": n, "tensors": [[k, list(s)] for k, s in m]}, f, separators=(",", ":"))
    return len(m), n


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    fx = build_fixture()
    np.savez_compressed(os.path.join(gold, "depth_reward.npz"), **fx)
    print("depth_reward.npz", os.path.getsize(os.path.join(gold, "depth_reward.npz")), "bytes")
    print("depth_anything_v2_small", "%d tensors %d parameters" % write_manifest(os.path.join(gold, "depth_anything_v2_small_manifest.json")))


if __name__ == "__main__":
    main()
