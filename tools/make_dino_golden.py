"""Writes tests/golden/dino_reward.npz: the DINOv2 image-similarity reward (edit_ppo/reward_model.py:217-257) evaluated by the INSTALLED third-party
packages -- PIL's resize, transformers' BitImageProcessor (the class ``facebook/dinov2-base`` names) with that checkpoint's published constants, and
transformers' Dinov2Model on a reduced config -- plus tests/golden/dinov2_base_manifest.json (names / shapes of the base model, 86,580,480 parameters).

torchvision is not installed, so the reference module cannot be imported; ``ToPILImage`` (``x.mul(255).byte()``) and the six lines of tail arithmetic are
restated from reading them (tests/vit_oracle.py: to_uint8_hwc, dino_reward).  Weights and input images are seeded (consolver_amd.synth.synthetic_dinov2_state_dict,
tests.vit_oracle.synthetic_image), so the fixture stores results, not inputs.  Host only.

Cases: (name, height, width, dtype); per case a pred image and a target = pred + noise.  Stored per case: the processor's uint8 crop of pred, CLS features of
pred and target in fp32, the reward, and the same graph evaluated by torch in bf16 (class comparator).  ``pixel_values`` are stored for the first case.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REDUCED = dict(hidden_size=128, num_hidden_layers=3, num_attention_heads=2, mlp_ratio=4, image_size=518, patch_size=14)
WEIGHT_SEED = 11
CASES = (("h512", 512, 512, "float16"), ("f512", 512, 512, "float32"), ("h1024", 1024, 1024, "float16"), ("f1024", 1024, 1024, "float32"))
TARGET_NOISE = 0.15


def case_images(i, h, w, dtype):
    """(pred, target) [3,h,w] in [0,1]"""
    from tests.vit_oracle import synthetic_image
    dt = getattr(torch, dtype)
    pred = synthetic_image(100 + i, h, w, torch.float32)
    g = torch.Generator().manual_seed(200 + i)
    target = (pred + TARGET_NOISE * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    return pred.to(dt), target.to(dt)


def hf_processor(**kw):
    from transformers import BitImageProcessor
    from tests.vit_oracle import PROCESSOR as P
    return BitImageProcessor(do_resize=True, size={"shortest_edge": P["shortest_edge"]}, resample=3, do_center_crop=True,
                             crop_size={"height": P["crop_size"], "width": P["crop_size"]}, do_rescale=True, rescale_factor=P["rescale_factor"],
                             do_normalize=True, image_mean=list(P["image_mean"]), image_std=list(P["image_std"]), do_convert_rgb=True, **kw)


def hf_model(cfg, sd):
    from transformers import Dinov2Config, Dinov2Model
    m = Dinov2Model(Dinov2Config(hidden_size=cfg["hidden_size"], num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                                 mlp_ratio=cfg["mlp_ratio"], image_size=cfg["image_size"], patch_size=cfg["patch_size"])).eval()
    m.load_state_dict(sd, strict=True)
    return m


def build_fixture():
    from PIL import Image
    from consolver_amd.synth import synthetic_dinov2_state_dict
    from tests import vit_oracle as vo
    sd = synthetic_dinov2_state_dict(vo.dinov2_manifest(REDUCED), seed=WEIGHT_SEED)
    model = hf_model(REDUCED, sd)
    model_bf16 = hf_model(REDUCED, sd).to(torch.bfloat16)
    proc, proc_u8 = hf_processor(), hf_processor()
    out = {"cfg": np.array([REDUCED[k] for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "mlp_ratio", "image_size", "patch_size")], np.int64),
           "weight_seed": np.array(WEIGHT_SEED, np.int64), "cases": np.array([c[0] for c in CASES])}
    with torch.no_grad():
        for i, (name, h, w, dtype) in enumerate(CASES):
            pils = [Image.fromarray(vo.to_uint8_hwc(t)) for t in case_images(i, h, w, dtype)]
            pv = proc(images=pils, return_tensors="pt")["pixel_values"]
            crop = proc_u8(images=pils, return_tensors="pt", do_rescale=False, do_normalize=False)["pixel_values"]
            cls = model(pixel_values=pv).last_hidden_state[:, 0]
            cls_bf16 = model_bf16(pixel_values=pv.to(torch.bfloat16)).last_hidden_state[:, 0].float()
            out[f"{name}_crop"] = crop[0].numpy().astype(np.uint8)
            if i == 0:
                out[f"{name}_pixel_values"] = pv[0].numpy().astype(np.float32)
            out[f"{name}_cls"] = cls.numpy()
            out[f"{name}_reward"] = vo.dino_reward(cls[:1], cls[1:]).numpy()
            out[f"{name}_cls_bf16"] = cls_bf16.numpy()
            out[f"{name}_reward_bf16"] = vo.dino_reward(cls_bf16[:1], cls_bf16[1:]).numpy()
    return out


def write_manifest(path):
    """the tools/make_manifests.py format, from the executor's own manifest (cs_vit_create is host only)"""
    from consolver_amd.reward_model import HipDinov2Model
    m = HipDinov2Model(device="cpu").manifest()
    n = sum(int(math.prod(s)) for _, s in m)
    with open(path, "w") as f:
        json.dump({"params": n, "tensors": [[k, list(s)] for k, s in m]}, f, separators=(",", ":"))
    return len(m), n


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    fx = build_fixture()
    np.savez_compressed(os.path.join(gold, "dino_reward.npz"), **fx)
    print("dino_reward.npz", os.path.getsize(os.path.join(gold, "dino_reward.npz")), "bytes;", {c[0]: float(fx[c[0] + "_reward"][0, 0]) for c in CASES},
          "bf16:", {c[0]: float(fx[c[0] + "_reward_bf16"][0, 0]) for c in CASES})
    print("dinov2_base", "%d tensors %d parameters" % write_manifest(os.path.join(gold, "dinov2_base_manifest.json")))


if __name__ == "__main__":
    main()
