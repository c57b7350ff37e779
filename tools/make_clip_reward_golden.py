"""Writes tests/golden/clip_reward.npz: the CLIP image-similarity reward (edit_ppo/reward_model.py:512-552) evaluated by the INSTALLED third-party
packages -- PIL's resize, transformers' CLIPImageProcessor with the published ``openai/clip-vit-large-patch14`` constants, and transformers'
CLIPVisionModelWithProjection on a reduced config -- plus tests/golden/clip_vit_l14_vision_manifest.json (names / shapes of the ViT-L/14 vision tower and its
projection, 303,966,208 parameters in 392 tensors).

torchvision is not installed, so the reference module cannot be imported; ``ToPILImage`` (``x.mul(255).byte()``) and the tail arithmetic are restated from
reading them (tests/vit_oracle.py: to_uint8_hwc; tests/clip_vision_oracle.py: clip_reward).  Weights and input images are seeded
(consolver_amd.synth.synthetic_clip_vision_state_dict, tests.vit_oracle.synthetic_image), so the fixture stores results, not inputs.  Host only.

Cases: (name, height, width, dtype); per case a pred image and a target = pred + noise.  Stored per case: the processor's uint8 crop of pred, ``image_embeds``
of pred and target in fp32, the reward, and the same graph evaluated by torch in bf16 (class comparator).  ``pixel_values`` are stored for the first case.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REDUCED = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, image_size=224, patch_size=14, projection_dim=64)
WEIGHT_SEED = 13
CASES = (("h512", 512, 512, "float16"), ("f512", 512, 512, "float32"), ("h1024", 1024, 1024, "float16"), ("f1024", 1024, 1024, "float32"))
TARGET_NOISE = 0.15


def case_images(i, h, w, dtype):
    """(pred, target) [3,h,w] in [0,1]"""
    from tests.vit_oracle import synthetic_image
    dt = getattr(torch, dtype)
    pred = synthetic_image(700 + i, h, w, torch.float32)
    g = torch.Generator().manual_seed(800 + i)
    target = (pred + TARGET_NOISE * torch.randn(3, h, w, generator=g)).clamp(0, 1)
    return pred.to(dt), target.to(dt)


def hf_processor(**kw):
    from transformers import CLIPImageProcessor
    from tests.clip_vision_oracle import PROCESSOR as P
    return CLIPImageProcessor(do_resize=True, size={"shortest_edge": P["shortest_edge"]}, resample=3, do_center_crop=True,
                              crop_size={"height": P["crop_size"], "width": P["crop_size"]}, do_rescale=True, rescale_factor=P["rescale_factor"],
                              do_normalize=True, image_mean=list(P["image_mean"]), image_std=list(P["image_std"]), do_convert_rgb=True, **kw)


def hf_model(cfg, sd):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    m = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=cfg["hidden_size"], intermediate_size=cfg["intermediate_size"],
                                                       num_hidden_layers=cfg["num_hidden_layers"], num_attention_heads=cfg["num_attention_heads"],
                                                       image_size=cfg["image_size"], patch_size=cfg["patch_size"], projection_dim=cfg["projection_dim"],
                                                       hidden_act="quick_gelu", layer_norm_eps=1e-5)).eval()
    m.load_state_dict(sd, strict=True)
    return m


def build_fixture():
    from PIL import Image
    from consolver_amd.synth import synthetic_clip_vision_state_dict
    from tests import clip_vision_oracle as co
    sd = synthetic_clip_vision_state_dict(co.clip_manifest(REDUCED), seed=WEIGHT_SEED)
    model = hf_model(REDUCED, sd)
    model_bf16 = hf_model(REDUCED, sd).to(torch.bfloat16)
    proc, proc_u8 = hf_processor(), hf_processor()
    keys = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "image_size", "patch_size", "projection_dim")
    out = {"cfg": np.array([REDUCED[k] for k in keys], np.int64), "weight_seed": np.array(WEIGHT_SEED, np.int64), "cases": np.array([c[0] for c in CASES])}
    with torch.no_grad():
        for i, (name, h, w, dtype) in enumerate(CASES):
            pils = [Image.fromarray(co.to_uint8_hwc(t)) for t in case_images(i, h, w, dtype)]
            pv = proc(images=pils, return_tensors="pt")["pixel_values"]
            crop = proc_u8(images=pils, return_tensors="pt", do_rescale=False, do_normalize=False)["pixel_values"]
            emb = model(pixel_values=pv).image_embeds
            emb_bf16 = model_bf16(pixel_values=pv.to(torch.bfloat16)).image_embeds.float()
            out[f"{name}_crop"] = crop[0].numpy().astype(np.uint8)
            if i == 0:
                out[f"{name}_pixel_values"] = pv[0].numpy().astype(np.float32)
            out[f"{name}_embeds"] = emb.numpy()
            out[f"{name}_reward"] = co.clip_reward(emb[:1], emb[1:]).numpy()
            out[f"{name}_embeds_bf16"] = emb_bf16.numpy()
            out[f"{name}_reward_bf16"] = co.clip_reward(emb_bf16[:1], emb_bf16[1:]).numpy()
    return out


def hf_full_manifest():
    """[(name, shape)] of transformers' CLIPVisionModelWithProjection at the ViT-L/14 config, on the meta device (no memory)"""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from tests.clip_vision_oracle import CLIP_VIT_L14 as c
    with torch.device("meta"):
        m = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_size=c["hidden_size"], intermediate_size=c["intermediate_size"],
                                                           num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"],
                                                           image_size=c["image_size"], patch_size=c["patch_size"], projection_dim=c["projection_dim"],
                                                           hidden_act="quick_gelu"))
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def write_manifest(path):
    """the tools/make_manifests.py format, from the executor's own manifest (cs_clipv_create is host only), checked against transformers'"""
    from consolver_amd.reward_model import HipCLIPVisionModel
    m = HipCLIPVisionModel(device="cpu").manifest()
    assert m == hf_full_manifest(), "the executor's manifest is not transformers' state dict"
    n = sum(int(math.prod(s)) for _, s in m)
    with open(path, "w") as f:
        json.dump({"params": n, "tensors": [[k, list(s)] for k, s in m]}, f, separators=(",", ":"))
    return len(m), n


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    fx = build_fixture()
    np.savez_compressed(os.path.join(gold, "clip_reward.npz"), **fx)
    print("clip_reward.npz", os.path.getsize(os.path.join(gold, "clip_reward.npz")), "bytes;", {c[0]: float(fx[c[0] + "_reward"][0, 0]) for c in CASES},
          "bf16:", {c[0]: float(fx[c[0] + "_reward_bf16"][0, 0]) for c in CASES})
    print("clip_vit_l14_vision", "%d tensors %d parameters" % write_manifest(os.path.join(gold, "clip_vit_l14_vision_manifest.json")))


if __name__ == "__main__":
    main()
