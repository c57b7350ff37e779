"""Writes tests/golden/segformer_reward.npz: the SegFormer mask-agreement reward (edit_ppo/reward_model.py:110-117, 425-481) evaluated by the INSTALLED
third-party packages -- PIL's resize through transformers' Segformer image processor (the PIL class) with the published constants of
nvidia/segformer-b4-finetuned-ade-512-512 and transformers' SegformerForSemanticSegmentation on a reduced config -- plus
tests/golden/segformer_b4_manifest.json (names / shapes of the B4 model).

The script depends on transformers and PIL only: ``ToPILImage`` (``x.mul(255).byte()``, torchvision) and the reward's tail are restated
(tests/vit_oracle.py: to_uint8_hwc; tests/segformer_oracle.py: masks, seg_reward).  Weights and input images are seeded
(consolver_amd.synth.synthetic_segformer_state_dict, tests.vit_oracle.synthetic_image), so the fixture stores results, not inputs.  Host only.

Reduced config: the B4 widths, heads and sr ratios with depths (1, 1, 2, 1), decoder width 256, 150 labels.  Cases: (name, processor size, image height = width,
dtype).  Size 128 gives grids 32 / 16 / 8 / 4 and 16 keys, size 160 grids 40 / 20 / 10 / 5 and 25 keys (a ragged key tile); ``s128_f128`` is an image of the
processor's own size (PIL returns a copy); the others are bilinear upscales.  Per case a pred image and a target = pred + 0.15 noise.

Stored per case: the processor's uint8 resized image of pred; of pred and target the fp32 class masks (uint8), the top-2 logit margin, the reward; the fp32
logits ON A PIXEL LATTICE (every LATTICE-th row and column of the quarter-size grid and the last one: 150 classes x every pixel x 8 images is 6 MB, over the
limit for a committed file); and of the same model in bf16 (class comparator) the masks, the reward, its logits on the lattice for pred as bit patterns, the
relative L2 error of its full logits and its share of pixels whose class differs from the fp32 mask.

Fixture conditions (asserted; a degenerate oracle must not be written): every fp32 mask uses at least 8 classes, the pred / target agreement lies in
(0.2, 0.9), and the bf16 comparator disagrees with the fp32 mask on at least 0.3 % of the pixels of every image.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT_SEED = 21
CASES = (("s128_h64", 128, 64, "float16"), ("s128_f128", 128, 128, "float32"), ("s160_f96", 160, 96, "float32"), ("s160_h64", 160, 64, "float16"))
IMAGE_SEEDS = (200, 201, 202, 203)
TARGET_NOISE = 0.15
LATTICE = 4


def lattice(g):
    """the rows / columns of a g x g grid whose logits are stored"""
    return np.unique(np.append(np.arange(0, g, LATTICE), g - 1))


def reduced_config(size):
    from tests.segformer_oracle import REDUCED
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
    from consolver_amd.synth import synthetic_segformer_state_dict
    from tests import segformer_oracle as so
    return synthetic_segformer_state_dict(so.manifest(reduced_config(size)), seed=WEIGHT_SEED)


def hf_processor(size):
    from transformers.models.segformer.image_processing_pil_segformer import SegformerImageProcessorPil as P
    from tests.segformer_oracle import PROCESSOR as C
    return P(do_resize=True, size={"height": size, "width": size}, resample=2, do_rescale=True, rescale_factor=C["rescale_factor"], do_normalize=True,
             image_mean=list(C["image_mean"]), image_std=list(C["image_std"]), do_reduce_labels=False)


def hf_config(cfg):
    from transformers import SegformerConfig
    from tests.segformer_oracle import SEGFORMER_B4
    c = dict(SEGFORMER_B4)
    c.update(cfg)
    return SegformerConfig(num_encoder_blocks=4, depths=list(c["depths"]), sr_ratios=list(c["sr_ratios"]), hidden_sizes=list(c["hidden_sizes"]),
                           patch_sizes=[7, 3, 3, 3], strides=[4, 2, 2, 2], num_attention_heads=list(c["num_attention_heads"]),
                           mlp_ratios=[c["mlp_ratio"]] * 4, decoder_hidden_size=c["decoder_hidden_size"], num_labels=c["num_labels"])


def hf_model(cfg, sd):
    from transformers import SegformerForSemanticSegmentation
    m = SegformerForSemanticSegmentation(hf_config(cfg)).eval()
    m.load_state_dict(sd, strict=True)
    return m


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def build_fixture():
    from PIL import Image
    from tests import segformer_oracle as so
    from tests import vit_oracle as vo
    out = {"weight_seed": np.array(WEIGHT_SEED, np.int64), "cases": np.array([c[0] for c in CASES]), "lattice": np.array(LATTICE, np.int64)}
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
            g = size // 4
            assert tuple(pv.shape) == (2, 3, size, size)
            logits = model(pixel_values=pv).logits.float()
            assert tuple(logits.shape) == (2, 150, g, g)
            m = so.masks(logits)
            reward = so.seg_reward(m[:1], m[1:])
            lb = model_bf16(pixel_values=pv.to(torch.bfloat16)).logits
            mb = so.masks(lb)
            reward_b = so.seg_reward(mb[:1], mb[1:])
            # the fixture conditions
            classes = [int(torch.unique(x).numel()) for x in m]
            agreement = float(reward) / 100
            differ = [float((mb[k] != m[k]).float().mean()) for k in range(2)]
            assert min(classes) >= 8, (name, classes)
            assert 0.2 < agreement < 0.9, (name, agreement)
            assert min(differ) >= 0.003, (name, differ)
            idx = torch.from_numpy(lattice(g))
            out[f"{name}_u8"] = u8[0].numpy().astype(np.uint8)
            out[f"{name}_logits"] = logits[:, :, idx][:, :, :, idx].numpy().astype(np.float32)
            out[f"{name}_masks"] = m.numpy().astype(np.uint8)
            out[f"{name}_margin"] = so.top2_margin(logits).numpy().astype(np.float32)
            out[f"{name}_reward"] = reward.numpy().astype(np.float32)
            out[f"{name}_logits_bf16"] = lb[:1, :, idx][:, :, :, idx].contiguous().view(torch.int16).numpy().view(np.uint16)
            out[f"{name}_masks_bf16"] = mb.numpy().astype(np.uint8)
            out[f"{name}_reward_bf16"] = reward_b.numpy().astype(np.float32)
            out[f"{name}_bf16_errors"] = np.array([rel_l2(lb.float(), logits), max(differ), float((reward_b - reward).abs().max())], np.float64)
            print(f"{name}: classes {classes} agreement {agreement:.4f} | bf16: logits rel-L2 {out[name + '_bf16_errors'][0]:.3e} mask disagreement "
                  f"{differ[0]:.4f} / {differ[1]:.4f} reward error {out[name + '_bf16_errors'][2]:.3e}")
    return out


def write_manifest(path):
    """the tools/make_manifests.py format, from the executor's own manifest (cs_seg_create is host only)"""
    from consolver_amd.reward_model import HipSegformerModel
    m = HipSegformerModel(device="cpu").manifest()
    n = sum(int(math.prod(s)) for _, s in m)
    with open(path, "w") as f:
        json.dump({"params": n, "tensors": [[k, list(s)] for k, s in m]}, f, separators=(",", ":"))
    return len(m), n


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    fx = build_fixture()
    np.savez_compressed(os.path.join(gold, "segformer_reward.npz"), **fx)
    print("segformer_reward.npz", os.path.getsize(os.path.join(gold, "segformer_reward.npz")), "bytes")
    print("segformer_b4", "%d tensors %d elements" % write_manifest(os.path.join(gold, "segformer_b4_manifest.json")))


if __name__ == "__main__":
    main()
