"""CPU restatement of FID as consolver_amd.fid computes it (the reference's fid_test.py: ``cleanfid.fid.compute_fid``): test infrastructure, not a fallback.

* ``pil_resize``          -- clean-fid's resize with PIL ITSELF: each channel ``Image.fromarray(x.astype(np.float32), mode="F").resize((299, 299), BICUBIC)``, clipped
  to [0, 255];
* ``two_pass_resize``     -- the same stated as two passes with double taps (horizontal first, stored as float32, then vertical; ``ss += pixel * k`` in double,
  ascending; a side that is 299 already is copied): what the HIP front end implements, checked bit for bit against PIL in tests/test_fid_oracle.py;
* ``FIDInceptionOracle``  -- the wiring of tests/inception_oracle.py with the 2015 graph's pools: ``F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)`` in the
  pool branches, ``F.max_pool2d(x, 3, 1, 1)`` in Mixed_7c's, and the [B, 2048] global mean as the output (no ``fc``).  Evaluated in float64 on the fp32
  weights by default, like ``InceptionOracle`` (the same figures on every host);
* ``statistics``          -- ``np.mean`` / ``np.cov(rowvar=False)`` in fp64;
* ``frechet_distance``    -- the ``eigh`` route.

cleanfid is not installed: the 299, the clip and (x - 128) / 128 are restated from memory.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import inception_oracle as io

SIZE, DIM = 299, 2048
MEAN = STD = 128.0


def to_uint8_hwc(image):
    """[3,H,W] uint8, or float in [0,1] -> uint8 [H,W,3]: ``evaluation.tensor_to_uint8_hwc``'s rule, round(clamp(x, 0, 1) * 255)"""
    if image.dtype == torch.uint8:
        return image.permute(1, 2, 0).contiguous().numpy()
    return (image.float().clamp(0, 1).permute(1, 2, 0) * 255.0).round().to(torch.uint8).numpy()


def pil_resize(img_u8, size=SIZE):
    """uint8 [H,W,3] -> fp32 [3,size,size] on the 0 .. 255 scale: PIL's mode-"F" bicubic per channel, clipped"""
    from PIL import Image
    out = [np.asarray(Image.fromarray(img_u8[:, :, c].astype(np.float32), mode="F").resize((size, size), Image.BICUBIC), dtype=np.float32) for c in range(3)]
    return np.clip(np.stack(out), 0, 255)


def _cubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def float_taps(n_in, n_out):
    """PIL's precompute_coeffs for BICUBIC: [(xmin, taps float64)] per output index"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    out = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = np.array([_cubic((x + xmin - center + 0.5) * ss) for x in range(n)], dtype=np.float64)
        tot = 0.0
        for v in w:
            tot += v
        out.append((xmin, w / tot if tot != 0.0 else w))
    return out


def _pass(x, n_out):
    """x float32 [rows, n_in] -> float32 [rows, n_out]: one pass along the last axis, double accumulation in ascending order"""
    if x.shape[1] == n_out:
        return x.copy()
    out = np.empty((x.shape[0], n_out), np.float32)
    for i, (xmin, k) in enumerate(float_taps(x.shape[1], n_out)):
        ss = np.zeros(x.shape[0], np.float64)
        for j in range(len(k)):
            ss = ss + x[:, xmin + j].astype(np.float64) * k[j]
        out[:, i] = ss.astype(np.float32)
    return out


def two_pass_resize(img_u8, size=SIZE, clip=True):
    """uint8 [H,W,3] -> fp32 [3,size,size]: the restatement of ``pil_resize``"""
    out = []
    for c in range(3):
        h = _pass(img_u8[:, :, c].astype(np.float32), size)
        out.append(np.ascontiguousarray(_pass(np.ascontiguousarray(h.T), size).T))
    r = np.stack(out)
    return np.clip(r, 0, 255) if clip else r


def normalize(resized, mean=MEAN, std=STD):
    """fp32 [.., 3, s, s] on the 0 .. 255 scale -> the network's input in fp32"""
    return (torch.as_tensor(resized, dtype=torch.float32) - mean) / std


def preprocess(images):
    """a list / stack of [3,H,W] tensors (uint8 or float in [0,1]) -> (resized [B,3,299,299] fp32 numpy, network input [B,3,299,299] fp32 tensor)"""
    resized = np.stack([pil_resize(to_uint8_hwc(im)) for im in images])
    return resized, normalize(resized)


def avg_pool_valid(x):
    """3x3 stride 1 pad 1, the sum divided by the taps inside the image"""
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def max_pool_same(x):
    """3x3 stride 1 pad 1; padding does not take part"""
    return F.max_pool2d(x, 3, 1, 1)


def manifest():
    """the inception manifest without fc: 94 BasicConv2d x 6 = 564 entries"""
    return [(k, s) for k, s in io.manifest() if not k.startswith("fc.")]


class _PoolBranchInput:
    """what ``walk`` hands a ``branch_pool`` conv: the unpooled tensor; the conv knows the block's name and with it the pool's rule"""

    def __init__(self, x):
        self.x = x


class FIDInceptionOracle(io.InceptionOracle):
    def avgpool(self, x):
        return _PoolBranchInput(x)

    def conv(self, name, x, cout, k, stride, pad):
        if isinstance(x, _PoolBranchInput):
            assert name.endswith(".branch_pool")
            x = max_pool_same(x.x) if name.startswith("Mixed_7c.") else avg_pool_valid(x.x)
        return super().conv(name, x, cout, k, stride, pad)

    @torch.no_grad()
    def __call__(self, pixel_values):
        """network input [B,3,299,299] -> pool3 features [B, 2048] fp32"""
        x = io.walk(self, pixel_values.to(self.dtype))
        assert x.shape[1:] == (DIM, 8, 8)
        return F.adaptive_avg_pool2d(x, 1).flatten(1).float()


def calibrated_state_dict(sd, n_images=8):
    """``sd`` with every BatchNorm's running statistics set on ``n_images`` calibration images resized by this front end (inception_oracle's calibration)"""
    _, pv = preprocess(list(io.calibration_images(SIZE, n_images)))
    return io.calibrate_batch_norm(sd, pv)


def statistics(features):
    """[n, d] -> (mu, sigma) fp64"""
    f = np.asarray(features, np.float64)
    return f.mean(0), np.cov(f, rowvar=False)


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """the eigh route: tr sqrt(s1 s2) = sum sqrt(eig(s1^(1/2) s2 s1^(1/2)))"""
    w, v = np.linalg.eigh(sigma1)
    root = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    m = root @ sigma2 @ root
    tr = np.sqrt(np.clip(np.linalg.eigvalsh((m + m.T) / 2), 0, None)).sum()
    d = mu1 - mu2
    return float(d @ d + np.trace(sigma1) + np.trace(sigma2) - 2 * tr)
