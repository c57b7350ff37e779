"""Evaluation harness: image writers of the batch generator and the paired-directory scorer.

Mirrors, by name and output schema:
* gen_ppo.py:205-212,318-325 -- ``{device_id}_{index:08d}.png`` + ``.txt`` (prompt) per generated image;
* compute_reward.py:52-78 ``find_image_pairs``, :81-95 ``load_image_tensor``, :332-365 ``calculate_statistics``,
  :447-462 the results JSON (``statistics`` / ``raw_scores`` / ``config``).
Scored on the GPU: the arithmetic-only reward (``image_psnr``, edit_ppo/reward_model.py:484-509; cs_image_psnr) and, given a model,
the DINOv2 and CLIP image-similarity rewards (``dino``, :217-257; ``clip``, :512-552), the depth-map PSNR (``depth``, :359-422), the SegFormer mask
agreement (``segmentation``, :425-481) and the Inception-v3 logit cosine (``inception``, :319-356; all in consolver_amd/reward_model.py).  The chat-model rewards (llava, qwen_vl) are not implemented.  PNG encode/decode is PIL (host I/O).
"""
import json
import os
from pathlib import Path

import numpy as np
import torch

from . import ppo


def generation_paths(out_dir, device_id, index):
    stem = os.path.join(out_dir, f"{device_id}_{index:08d}")       # gen_ppo.py:321-323
    return stem + ".png", stem + ".txt"


def tensor_to_uint8_hwc(image):
    """[3,H,W] in [0,1] (decode_latents output) -> uint8 [H,W,3], rounding like ``pipe.image_processor.postprocess``
    / ``numpy_to_pil``: (x * 255).round()."""
    x = image.detach().float().clamp(0, 1).cpu()
    return (x.permute(1, 2, 0) * 255.0).round().to(torch.uint8).numpy()


def save_generation(out_dir, device_id, index, image, prompt):
    """one generated image + its prompt, the batch generator's naming (gen_ppo.py:318-325)."""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    png, txt = generation_paths(out_dir, device_id, index)
    Image.fromarray(tensor_to_uint8_hwc(image)).save(png)
    with open(txt, "w") as f:
        f.write(prompt)
    return png, txt


def find_image_pairs(root_dir1, root_dir2, *args):
    """compute_reward.py:52-78: PNG files with the same relative path under both roots."""
    root1, root2 = Path(root_dir1), Path(root_dir2)
    pairs = []
    for p in sorted(root1.rglob("*.png")):
        q = root2 / p.relative_to(root1)
        if q.exists():
            pairs.append((str(p), str(q)))
    return pairs


def load_image_tensor(image_path, device):
    """compute_reward.py:81-95: RGB, [3,H,W] float32 in [0,1] (ToTensor = uint8 / 255)."""
    from PIL import Image
    arr = np.asarray(Image.open(image_path).convert("RGB"), dtype=np.uint8)
    return (torch.from_numpy(arr.copy()).permute(2, 0, 1).float() / 255.0).to(device)


def calculate_statistics(results):
    """compute_reward.py:332-365 (population std, like np.std)."""
    stats = {}
    for reward_type, scores in results.items():
        if len(scores) > 0:
            a = np.array(scores)
            stats[reward_type] = {"mean": float(np.mean(a)), "std": float(np.std(a)), "min": float(np.min(a)), "max": float(np.max(a)),
                                  "median": float(np.median(a)), "count": len(scores)}
        else:
            stats[reward_type] = {"mean": 0.0, "std": 0.0, "min": 0.0, "max": 0.0, "median": 0.0, "count": 0}
    return stats


def score_image_pairs(image_pairs, reward_types=("image_psnr",), batch_size=16, device="cuda:0", reward_models=None):
    """-> {reward_type: [score per pair]} (compute_reward.py:98-330).  ``reward_models``: {reward_type: (model, processor)} as returned by
    ``reward_model.load_reward_model`` / ``load_depth_reward`` / ``load_segmentation_reward`` / ``load_inception_reward`` for the rewards that need a network ("dino", "clip", "depth",
    "segmentation", "inception").  The pairs of a chunk may differ in size (``group_by_size``); the scores come back in input order."""
    results = {}
    reward_models = reward_models or {}
    for rt in reward_types:
        scores = []
        model, processor = reward_models.get(rt, (None, None))
        for s in range(0, len(image_pairs), batch_size):
            chunk = image_pairs[s:s + batch_size]
            a = [load_image_tensor(p, device) for p, _ in chunk]
            b = [load_image_tensor(q, device) for _, q in chunk]
            out = [None] * len(chunk)
            for idx in group_by_size(a, b, chunk):
                r = ppo.calculate_reward(rt, model, processor, torch.stack([a[i] for i in idx]), torch.stack([b[i] for i in idx]), device).flatten().cpu()
                for i, v in zip(idx, r):
                    out[i] = float(v)
            scores.extend(out)
        results[rt] = scores
    return results


def group_by_size(a, b, names=None):
    """the positions of a chunk's pairs grouped by image size, each group in input order, the groups in order of first appearance: images of one size stack
    into one batch (edits made at their inputs' aspect ratios come in many sizes).  A pair whose two images differ in size cannot be compared: ValueError
    naming it (``names[i]``: its two files)."""
    groups = {}
    for i, (x, y) in enumerate(zip(a, b)):
        if tuple(x.shape) != tuple(y.shape):
            what = f"{names[i][0]} and {names[i][1]}" if names is not None else f"pair {i}"
            raise ValueError(f"{what}: the two images of a pair differ in size ({tuple(x.shape[-2:])} vs {tuple(y.shape[-2:])})")
        groups.setdefault(tuple(x.shape), []).append(i)
    return list(groups.values())


def write_results(output_path, results, config):
    """compute_reward.py:447-462."""
    data = {"statistics": calculate_statistics(results), "raw_scores": results, "config": config}
    with open(output_path, "w", encoding="utf-8") as f:
        json.dump(data, f, indent=2, ensure_ascii=False)
    return data
