"""Writes tests/golden/inception_reward.npz: the Inception-v3 logit-cosine reward (edit_ppo/reward_model.py:98-108, 319-356) -- the uint8 crops from the
INSTALLED PIL under torchvision's transform rules, and the logits / rewards of the fp32 restatement (tests/inception_oracle.py) on seeded, calibrated
weights -- plus tests/golden/inception_v3_manifest.json (names / shapes of the evaluated network, torchvision's state-dict order without AuxLogits).

torchvision is not installed: ``Resize(size, BICUBIC)`` is ``img.resize((nw, nh), BICUBIC)`` with the short side ``size`` and the long side
``int(size * long / short)``; ``CenterCrop(size)`` is ``img.crop`` at ``int(round((n - size) / 2.0))`` (Python's round half to even), both restated here on
PIL images.  Weights and images are seeded (consolver_amd.synth.synthetic_inception_state_dict, ``case_images``), so the fixture stores results, not inputs.
Host only.

Weights: the synthetic recipe, then every BatchNorm's running statistics set to the batch statistics of 16 fixed images at the case's size
(inception_oracle.calibrate_batch_norm).  Without that the network is degenerate: the reward of any pair is above 99.9 (stored per case as
``<name>_reward_uncalibrated``; the host test asserts it).

Cases: (name, size, (height, width), dtype, noise amplitude).  Full widths; size 107 gives a last grid of 2 x 2, 139 one of 3 x 3.  ``s107_own`` is an image of
the transform's own size (PIL returns a copy); ``s107_land`` resizes to 107 x 144 (n - size = 37 = 1 mod 4: both crop rules give 18) and ``s107_port`` to
146 x 107 (n - size = 39 = 3 mod 4: torchvision 20, the floor rule 19).  Per case a target image and pred = target + amplitude x noise.

Stored per case: the uint8 crops of pred and target, the fp32 logits of both, the reward, the uncalibrated reward, and of the same model in bf16 (the
comparator) the per-image relative L2 error of the logits and the reward.

Fixture conditions (asserted; a degenerate oracle must not be written): the largest reward among the cases is in [95, 99.9), the smallest at most 80.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT_SEED = 11
CASES = (("s107_own", 107, (107, 107), "float32", 0.01), ("s107_land", 107, (80, 108), "float32", 0.01), ("s107_port", 107, (131, 96), "float16", 0.8),
         ("s139_sq", 139, (160, 160), "float16", 0.8), ("s139_land", 139, (100, 150), "float32", 0.05))
IMAGE_SEEDS = (300, 301, 308, 303, 304)


def smooth_image(seed, h, w, grid=(6, 7)):
    """[3,h,w] in [0,1]: a random field of ``grid`` values (6 x 7: the fixture's), bicubic"""
    g = torch.Generator().manual_seed(seed)
    return F.interpolate(torch.rand(1, 3, *grid, generator=g), size=(h, w), mode="bicubic", align_corners=False)[0].clamp(0, 1)


def noisy_pair(seed, hw, amplitude, dtype="float32", grid=(6, 7)):
    """(pred, target) [3,h,w] in [0,1]: target smooth, pred = target + amplitude x N(0, 1), clamped"""
    dt = getattr(torch, dtype)
    target = smooth_image(seed, *hw, grid)
    g = torch.Generator().manual_seed(seed + 100)
    pred = (target + amplitude * torch.randn(3, *hw, generator=g)).clamp(0, 1)
    return pred.to(dt), target.to(dt)


def case_images(i):
    _, _, hw, dtype, amp = CASES[i]
    return noisy_pair(IMAGE_SEEDS[i], hw, amp, dtype)


def plain_state_dict():
    from consolver_amd.synth import synthetic_inception_state_dict
    from tests import inception_oracle as io
    return synthetic_inception_state_dict(io.manifest(), seed=WEIGHT_SEED)


_CALIBRATED = {}


def state_dict(size, n_images=16):
    """the seeded weights with the BatchNorm statistics of ``n_images`` calibration images at ``size`` (cached)"""
    from tests import inception_oracle as io
    if (size, n_images) not in _CALIBRATED:
        _, pv = io.preprocess(io.calibration_images(size, n_images), size)
        _CALIBRATED[(size, n_images)] = io.calibrate_batch_norm(plain_state_dict(), pv)
    return _CALIBRATED[(size, n_images)]


def pil_crop(image, size):
    """[3,H,W] float tensor in [0,1] -> uint8 [3,size,size]: ToPILImage, Resize(size, BICUBIC), CenterCrop(size) on the installed PIL"""
    from PIL import Image
    from tests.vit_oracle import to_uint8_hwc
    img = Image.fromarray(to_uint8_hwc(image))
    w, h = img.size
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    img = img.resize((nw, nh), Image.BICUBIC)
    top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
    img = img.crop((left, top, left + size, top + size))
    return np.ascontiguousarray(np.asarray(img, dtype=np.uint8).transpose(2, 0, 1))


def main():
    from tests import inception_oracle as io
    out = {"cases": np.array([c[0] for c in CASES])}
    rewards = []
    plain = io.InceptionOracle(plain_state_dict())
    for i, (name, size, hw, dtype, amp) in enumerate(CASES):
        pred, target = case_images(i)
        u8 = np.stack([pil_crop(pred, size), pil_crop(target, size)])
        u8_restated, pv = io.preprocess(torch.stack([pred, target]), size)
        assert np.array_equal(u8, u8_restated), name              # the restated resize and crop are PIL's
        sd = state_dict(size)
        logits = io.InceptionOracle(sd)(pv)
        lb = io.InceptionOracle(sd, torch.bfloat16)(pv)
        reward = io.inception_reward(logits[:1], logits[1:])
        lp = plain(pv)
        out[f"{name}_u8"] = u8
        out[f"{name}_logits"] = logits.numpy()
        out[f"{name}_reward"] = reward.numpy()
        out[f"{name}_reward_uncalibrated"] = io.inception_reward(lp[:1], lp[1:]).numpy()
        out[f"{name}_bf16_error"] = ((lb - logits).norm(dim=1) / logits.norm(dim=1)).numpy()
        out[f"{name}_reward_bf16"] = io.inception_reward(lb[:1], lb[1:]).numpy()
        rewards.append(reward.item())
        print(name, "reward", rewards[-1], "uncalibrated", out[f"{name}_reward_uncalibrated"].item(), "bf16", out[f"{name}_bf16_error"], out[f"{name}_reward_bf16"].item())
    assert 95 <= max(rewards) < 99.9 and min(rewards) <= 80, rewards
    golden = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(golden, "inception_reward.npz"), **out)
    m = io.manifest()
    with open(os.path.join(golden, "inception_v3_manifest.json"), "w") as f:
        json.dump({"params": io.param_count(), "aux_params": io.AUX_PARAMS, "tensors": [[k, list(s)] for k, s in m]}, f)
    print("wrote", os.path.getsize(os.path.join(golden, "inception_reward.npz")), "bytes")


if __name__ == "__main__":
    main()
