"""Writes tests/golden/fid.npz: the FID front end's inputs with the INSTALLED PIL's answers, and the features of the fp32 restatement
(tests/fid_oracle.py) on seeded, calibrated weights.  Host only.

Resize cases (name, height, width), two different uint8 images each:
  up37x53       upscale, the axes differ; the images have hard edges, so the bicubic overshoots and the clip to [0, 255] acts;
  copy300x299   the width is 299 already: the horizontal pass is a copy;
  own299        both sides are 299: PIL returns a copy;
  down96x640    width scale 2.14: support 4.28, 11 taps; the height is upscaled.
The images are blocks of random grey levels of random sizes (hard edges: overshoot; they deflate well), the first of a case under a low-amplitude
sinusoidal texture, so the file stays small with the inputs themselves in it.

Stored: per case the uint8 inputs [2,H,W,3] and PIL's resized, clipped output for the rows ROWS (first, every 9th, last: a full 299 x 299 x 3 fp32 image is
1 MB) as [2,3,len(ROWS),299] fp32; the oracle's pool3 features of the 8 images [8,2048] fp32 and, of the same network in bf16, their per-image relative L2
error.  Weights: consolver_amd.synth.synthetic_fid_inception_state_dict, BatchNorm statistics calibrated on 8 images (fid_oracle.calibrated_state_dict).

Also the generator of the end-to-end sets of the GPU test (``e2e_set``): 12 images of 64 x 80 per noise level, made here so that the levels are chosen in
one place; ``main`` asserts that the oracle's FID between the two levels is far above the error of a bf16 evaluation of the same features.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHT_SEED = 11
CALIBRATION_IMAGES = 8
RESIZE_CASES = (("up37x53", 37, 53), ("copy300x299", 300, 299), ("own299", 299, 299), ("down96x640", 96, 640))
ROWS = np.unique(np.r_[np.arange(0, 299, 9), 298])
E2E_LEVELS = (0.05, 0.5)            # noise amplitudes of the two end-to-end sets
E2E_COUNT, E2E_HW = 12, (64, 80)


def block_image(seed, h, w):
    """uint8 [h,w,3]: random grey levels in random blocks (0 and 255 among them); an even seed adds a sinusoidal texture of amplitude 6"""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 3), np.float64)
    y = 0
    while y < h:
        bh = int(rng.integers(3, 24))
        x = 0
        while x < w:
            bw = int(rng.integers(3, 24))
            level = rng.choice([0.0, 255.0, float(rng.integers(0, 256))], p=[0.25, 0.25, 0.5])
            img[y:y + bh, x:x + bw] = level + rng.integers(-20, 21, size=3)
            x += bw
        y += bh
    yy, xx = np.mgrid[0:h, 0:w]
    if seed % 2 == 0:
        img += (6 * np.sin(0.37 * xx + 0.11 * yy + seed))[:, :, None]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def case_images(i):
    """uint8 [2,H,W,3] of resize case i"""
    _, h, w = RESIZE_CASES[i]
    return np.stack([block_image(1000 + 2 * i, h, w), block_image(1001 + 2 * i, h, w)])


def fixture_images():
    """the 8 fixture images as uint8 [3,H,W] tensors, in case order"""
    return [torch.from_numpy(im).permute(2, 0, 1).contiguous() for i in range(len(RESIZE_CASES)) for im in case_images(i)]


_STATE = {}


def state_dict():
    """the seeded weights with calibrated BatchNorm statistics (cached)"""
    from consolver_amd.synth import synthetic_fid_inception_state_dict
    from tests import fid_oracle as fo
    if "sd" not in _STATE:
        _STATE["sd"] = fo.calibrated_state_dict(synthetic_fid_inception_state_dict(fo.manifest(), seed=WEIGHT_SEED), CALIBRATION_IMAGES)
    return _STATE["sd"]


def e2e_set(level, seed=0):
    """[12,3,64,80] fp32 in [0,1]: smooth random fields + ``level`` x N(0, 1), clamped"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4000 + seed)
    low = torch.rand(E2E_COUNT, 3, 4, 5, generator=g)
    clean = F.interpolate(low, size=E2E_HW, mode="bicubic", align_corners=False)
    return (clean + level * torch.randn(E2E_COUNT, 3, *E2E_HW, generator=g)).clamp(0, 1)


def main():
    from tests import fid_oracle as fo
    out = {"cases": np.array([c[0] for c in RESIZE_CASES]), "rows": ROWS.astype(np.int32)}
    for i, (name, h, w) in enumerate(RESIZE_CASES):
        u8 = case_images(i)
        full = np.stack([fo.pil_resize(im) for im in u8])
        raw = np.stack([fo.two_pass_resize(im, clip=False) for im in u8])
        assert np.array_equal(np.clip(raw, 0, 255), full), name                      # the restatement is PIL's
        print(name, "before the clip:", raw.min(), "..", raw.max())
        if name.startswith("up"):
            assert raw.min() < -5 and raw.max() > 260                                  # the clip acts
        out[f"{name}_u8"] = u8
        out[f"{name}_rows"] = np.ascontiguousarray(full[:, :, ROWS])
    sd = state_dict()
    _, pv = fo.preprocess(fixture_images())
    feats = fo.FIDInceptionOracle(sd)(pv)
    fb = fo.FIDInceptionOracle(sd, torch.bfloat16)(pv)
    spread = float((feats[0] - feats[1]).norm() / feats[1].norm())
    assert spread > 0.05, spread                                                      # the features depend on the image
    out["features"] = feats.numpy()
    out["features_bf16_error"] = ((fb - feats).norm(dim=1) / feats.norm(dim=1)).numpy()
    print("bf16 comparator error per image", out["features_bf16_error"], "image 0 vs 1", spread)
    # the end-to-end sets: the oracle's FID between the two noise levels against what a bf16 evaluation of the features moves it by
    fa, fbb, ea, eb = [], [], [], []
    for level, (f32, b16) in zip(E2E_LEVELS, ((fa, ea), (fbb, eb))):
        _, pv = fo.preprocess(list(e2e_set(level)))
        f32.append(fo.FIDInceptionOracle(sd)(pv).numpy())
        b16.append(fo.FIDInceptionOracle(sd, torch.bfloat16)(pv).numpy())
    fid = fo.frechet_distance(*fo.statistics(fa[0]), *fo.statistics(fbb[0]))
    fid_b = fo.frechet_distance(*fo.statistics(ea[0]), *fo.statistics(eb[0]))
    print("end to end: oracle FID", fid, "bf16 features", fid_b)
    assert fid > 10 * abs(fid - fid_b), (fid, fid_b)
    path = os.path.join(ROOT, "tests", "golden", "fid.npz")
    np.savez_compressed(path, **out)
    print("wrote", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 838 * 1024


if __name__ == "__main__":
    main()
