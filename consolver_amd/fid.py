"""FID on the HIP library: the first column of the reference's results table (``fid_test.py``: ``cleanfid.fid.compute_fid(generated_dir, "coco/val2017")``).

Three pieces, each a C entry point family of include/consolver_hip.h:

* the front end (``cs_fid_preprocess``): every channel as a PIL mode-``"F"`` image, ``BICUBIC`` straight to 299 x 299 in floating point, clipped to
  [0, 255], then ``(v - mean) / std``.  A float tensor in [0, 1] is quantised first as ``round(clamp(x, 0, 1) * 255)`` (``evaluation.tensor_to_uint8_hwc``),
  so a tensor and the PNG written from it give the same features;
* ``HipFIDInception`` (``cs_fid_forward``): the FID variant of Inception-v3 -- the 2015 TF graph's pooling rules under torchvision's state-dict names, which is
  the naming of pytorch-fid's ``pt_inception-2015-12-05`` checkpoint -- giving the 2048-d ``pool3`` features in fp32;
* ``FIDStatistics`` (``cs_fid_stats_accumulate`` / ``cs_fid_stats_finalize``): sum and outer-product accumulators and the mean / covariance in fp64 on the GPU.

``frechet_distance`` is host numpy in fp64 (a 2048 x 2048 matrix square root, once per evaluation).

Restated from memory -- ``cleanfid`` is not installed here and is not part of the reference tree: the fixed 299, the clip to [0, 255], the default
normalisation (x - 128) / 128 (configurable: ``image_mean`` / ``image_std``), the pooling differences of the FID network and the 1008-class ``fc`` of its
checkpoint.  No real checkpoint has been loaded: there are no weights here; the tests run calibrated synthetic ones.

``python -m consolver_amd.fid GEN_DIR GT_DIR_OR_NPZ --weights CHECKPOINT [--save-stats PATH]`` prints ``FID for {GEN_DIR}: {fid:.2f}``, the line of ``fid_test.py``.
"""
import argparse
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from .reward_model import _HipImageModel

FID_INCEPTION_CONFIG = dict(image_size=299, feature_dim=2048, image_mean=(128.0, 128.0, 128.0), image_std=(128.0, 128.0, 128.0))
IMAGE_EXTENSIONS = ("png", "jpg", "jpeg")
_IMAGE_DT = {torch.uint8: L.CS_U8, torch.float16: L.CS_F16, torch.float32: L.CS_F32}


class HipFIDInception(_HipImageModel):
    """The FID Inception-v3.  ``features(images)`` -> [B, 2048] fp32 for images [B,3,H,W], uint8 or float16 / float32 in [0,1], any H, W >= 1.
    ``load_state_dict`` takes torchvision's names; ``fc.*`` and ``AuxLogits.*`` of a checkpoint are ignored."""
    workspace_budget = 1024 << 20         # bytes of workspace one call may take: max_batch is sized from it (5.4 MB per image)
    _prefix = "fid"

    def __init__(self, config=None, device="cuda:0"):
        cfg = dict(FID_INCEPTION_CONFIG)
        cfg.update(config or {})
        if cfg["image_size"] != 299 or cfg["feature_dim"] != 2048:
            raise ValueError("the FID network takes 299 x 299 images and gives 2048 features")
        self.config = cfg
        self.device = torch.device(device)
        c = L.CsFidConfig((C.c_float * 3)(*cfg["image_mean"]), (C.c_float * 3)(*cfg["image_std"]))
        h = C.c_void_p()
        L.check(L.lib().cs_fid_create(C.byref(c), C.byref(h)))
        self._init_handle(h, cfg["image_size"], 1)
        self._feature_dim = cfg["feature_dim"]
        self.max_batch = max(1, min(_HipImageModel.max_batch, self.workspace_budget // int(self._fn("workspace_bytes")(h, 1))))

    def preprocess(self, images, return_resized=False):
        """[B,3,H,W] uint8, or fp16 / fp32 in [0,1] -> the network's input rows [B * 299 * 299, 8] fp16 and, with ``return_resized``, the resized and clipped
        image [B,3,299,299] fp32 on the 0 .. 255 scale (what clean-fid hands its normalisation)."""
        L.require_cuda(images, "images")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be [B,3,H,W], got {tuple(images.shape)}")
        if images.dtype not in _IMAGE_DT:
            raise TypeError(f"images must be uint8, float16 or float32, got {images.dtype}")
        images = images.contiguous()
        B, _, H, W = images.shape
        S = self.crop
        patches = torch.empty(B * S * S, self.patch_cols, dtype=torch.float16, device=images.device)
        resized = torch.empty(B, 3, S, S, dtype=torch.float32, device=images.device) if return_resized else None
        if B:
            need = int(self._fn("preprocess_workspace_bytes")(self._h, B, H, W))
            if self._pws is None or self._pws.numel() < need or self._pws.device != images.device:
                self._pws = torch.empty(need, dtype=torch.uint8, device=images.device)
            with torch.cuda.device(images.device):          # the resize tables of a new image size are allocated on the current device
                L.check(self._fn("preprocess")(self._h, L.ptr(images), _IMAGE_DT[images.dtype], B, H, W, L.ptr(patches), L.ptr(resized), L.ptr(self._pws),
                                                self._pws.numel(), L.stream_ptr(images.device)))
        return (patches, resized) if return_resized else patches

    def encode_patches(self, patches):
        """the rows of ``preprocess`` -> pool3 features [B, 2048] fp32"""
        return self._forward(patches, self._feature_dim)

    @torch.no_grad()
    def features(self, images):
        """[B,3,H,W] -> pool3 features [B, 2048] fp32; at most ``max_batch`` images are resized at a time"""
        if images.shape[0] <= self.max_batch:
            return self.encode_patches(self.preprocess(images))
        return torch.cat([self.encode_patches(self.preprocess(images[s:s + self.max_batch])) for s in range(0, images.shape[0], self.max_batch)])


def load_fid_inception(device="cuda:0", config=None):
    """the FID network's shapes and clean-fid's normalisation constants; the caller loads the weights (pytorch-fid's checkpoint under torchvision's names)"""
    return HipFIDInception(config, device=device)


class FIDStatistics:
    """Running feature statistics in fp64 on ``device``: ``sum`` [d], ``outer`` [d,d] = sum of f f^T, and the row count ``n``.  ``update`` and ``finalize`` run
    HIP kernels.  Holding, ``merge`` and the files work on any device: ranks shard a directory, each saves its partial (``save_partial``), and one process
    loads and merges them -- no collective is used."""

    def __init__(self, d=2048, device="cuda:0"):
        if d < 16 or d > 4096 or d % 16:
            raise ValueError("d must be a multiple of 16 in 16 .. 4096")
        self.d, self.device, self.n = int(d), torch.device(device), 0
        self.sum = torch.zeros(d, dtype=torch.float64, device=self.device)
        self.outer = torch.zeros(d, d, dtype=torch.float64, device=self.device)

    def update(self, features):
        """adds the rows of ``features`` [n, d] fp32 (a CUDA tensor on this object's device)"""
        L.require_cuda(features, "features")
        L.require_cuda(self.sum, "the statistics")
        if features.dim() != 2 or features.shape[1] != self.d or features.dtype != torch.float32 or features.device != self.sum.device:
            raise ValueError(f"features must be [n, {self.d}] float32 on {self.sum.device}, got {tuple(features.shape)} {features.dtype} on {features.device}")
        n = features.shape[0]
        if n:
            features = features.contiguous()
            L.check(L.lib().cs_fid_stats_accumulate(L.ptr(features), n, self.d, L.ptr(self.sum), L.ptr(self.outer), L.stream_ptr(features.device)))
            self.n += n
        return self

    def merge(self, other):
        """adds another object's ``sum``, ``outer`` and ``n``"""
        if other.d != self.d:
            raise ValueError(f"feature widths differ: {self.d} vs {other.d}")
        self.sum += other.sum.to(self.sum.device)
        self.outer += other.outer.to(self.outer.device)
        self.n += other.n
        return self

    def finalize(self):
        """-> (mu [d], sigma [d,d]) numpy fp64: mu = sum / n, sigma = (outer - n mu mu^T) / (n - 1)"""
        L.require_cuda(self.sum, "the statistics")
        mu, sigma = torch.empty_like(self.sum), torch.empty_like(self.outer)
        L.check(L.lib().cs_fid_stats_finalize(L.ptr(self.sum), L.ptr(self.outer), self.n, self.d, L.ptr(mu), L.ptr(sigma), L.stream_ptr(self.sum.device)))
        return mu.cpu().numpy(), sigma.cpu().numpy()

    def save(self, path):
        """the finished statistics as ``.npz``: ``mu``, ``sigma``, ``n``"""
        mu, sigma = self.finalize()
        save_statistics(path, mu, sigma, self.n)

    @staticmethod
    def load(path):
        """-> (mu, sigma, n) of a file written by ``save``"""
        return load_statistics(path)

    def save_partial(self, path):
        """the accumulators as ``.npz``: ``sum``, ``outer``, ``n``"""
        with open(path, "wb") as f:
            np.savez(f, sum=self.sum.cpu().numpy(), outer=self.outer.cpu().numpy(), n=np.int64(self.n))

    @classmethod
    def load_partial(cls, path, device="cuda:0"):
        with np.load(path, allow_pickle=False) as z:
            s = cls(int(z["sum"].shape[0]), device)
            s.sum.copy_(torch.from_numpy(z["sum"]))
            s.outer.copy_(torch.from_numpy(z["outer"]))
            s.n = int(z["n"])
        return s


def save_statistics(path, mu, sigma, n):
    with open(path, "wb") as f:
        np.savez(f, mu=np.asarray(mu, np.float64), sigma=np.asarray(sigma, np.float64), n=np.int64(n))


def load_statistics(path):
    with np.load(path, allow_pickle=False) as z:
        return z["mu"].astype(np.float64), z["sigma"].astype(np.float64), int(z["n"])


def _have_scipy():
    try:
        import scipy.linalg  # noqa: F401
        return True
    except ImportError:
        return False


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6, method=None):
    """|mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr sqrt(sigma1 sigma2), on the host in fp64.

    ``method="sqrtm"`` (the default when scipy is importable): ``scipy.linalg.sqrtm(sigma1 @ sigma2)`` as clean-fid does; a result that is not finite is
    redone with ``eps * I`` added to both covariances; a diagonal imaginary part above 1e-3 raises ``ValueError``, otherwise the real part is used.
    ``method="eigh"``: sigma1^(1/2) by ``eigh``, then the eigenvalues of the symmetric sigma1^(1/2) sigma2 sigma1^(1/2), which has the spectrum of
    sigma1 sigma2; negative eigenvalues (rounding; rank-deficient input) are clipped to 0."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape or sigma1.shape != (mu1.shape[0], mu1.shape[0]):
        raise ValueError("mean / covariance shapes differ")
    if method is None:
        method = "sqrtm" if _have_scipy() else "eigh"
    diff = mu1 - mu2
    if method == "sqrtm":
        from scipy import linalg
        covmean = linalg.sqrtm(sigma1.dot(sigma2))
        if isinstance(covmean, tuple):          # (older scipy: disp=False form)
            covmean = covmean[0]
        if not np.isfinite(covmean).all():
            offset = np.eye(sigma1.shape[0]) * eps
            covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
        if np.iscomplexobj(covmean):
            if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
                raise ValueError(f"imaginary component {np.max(np.abs(covmean.imag))}")
            covmean = covmean.real
        tr_covmean = float(np.trace(covmean))
    elif method == "eigh":
        w, v = np.linalg.eigh(sigma1)
        root = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
        m = root @ sigma2 @ root
        tr_covmean = float(np.sqrt(np.clip(np.linalg.eigvalsh((m + m.T) / 2), 0, None)).sum())
    else:
        raise ValueError(f"method must be 'sqrtm' or 'eigh', got {method!r}")
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean)


def list_images(root):
    """every ``png`` / ``jpg`` / ``jpeg`` file (any letter case) under ``root``, recursively, sorted by path"""
    out = []
    for base, _, files in os.walk(root):
        out += [os.path.join(base, f) for f in files if f.rsplit(".", 1)[-1].lower() in IMAGE_EXTENSIONS and "." in f]
    return sorted(out)


def _load_uint8(path):
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1)


def directory_statistics(root, model, batch_size=64, device="cuda:0", paths=None):
    """``FIDStatistics`` of the images under ``root`` (or of ``paths``): decoded by PIL on the host, batched in listing order (a batch ends where the image
    size changes), resized and evaluated on the GPU"""
    paths = list_images(root) if paths is None else list(paths)
    if not paths:
        raise ValueError(f"no png / jpg / jpeg images under {root}")
    stats = FIDStatistics(model.config["feature_dim"], device)
    batch = []

    def flush():
        if batch:
            stats.update(model.features(torch.stack(batch).to(device)))
            batch.clear()
    for p in paths:
        im = _load_uint8(p)
        if batch and (len(batch) == batch_size or im.shape != batch[0].shape):
            flush()
        batch.append(im)
    flush()
    return stats


def _statistics_of(source, model, batch_size, device):
    if os.path.isdir(source):
        if model is None:
            raise ValueError(f"{source} is a directory: a HipFIDInception with loaded weights is needed")
        mu, sigma = directory_statistics(source, model, batch_size, device).finalize()
        return mu, sigma
    mu, sigma, _ = load_statistics(source)
    return mu, sigma


def compute_fid(a, b, model=None, batch_size=64, device="cuda:0", method=None):
    """FID between ``a`` and ``b``, each a directory of images or a ``.npz`` of saved statistics (``FIDStatistics.save``)"""
    mu1, s1 = _statistics_of(a, model, batch_size, device)
    mu2, s2 = _statistics_of(b, model, batch_size, device)
    return frechet_distance(mu1, s1, mu2, s2, method=method)


def main(argv=None, model=None):
    """the command line; ``model``: a loaded ``HipFIDInception`` to use instead of building one from ``--weights`` (library callers)"""
    ap = argparse.ArgumentParser(description="FID of a directory of generated images against a directory or saved statistics (fid_test.py)")
    ap.add_argument("gen_dir")
    ap.add_argument("gt", help="directory of images, or an .npz written by --save-stats")
    ap.add_argument("--weights", help="state dict of the FID Inception (torch.load; torchvision's names, pytorch-fid's pt_inception-2015-12-05)")
    ap.add_argument("--synthetic-weights", action="store_true", help="seeded random weights: a dry run of the pipeline, not a FID")
    ap.add_argument("--save-stats", help="write the statistics of GT here (.npz) for later runs")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--method", choices=("sqrtm", "eigh"), default=None)
    args = ap.parse_args(argv)
    if model is None and (os.path.isdir(args.gen_dir) or os.path.isdir(args.gt)):
        model = load_fid_inception(args.device)
        if args.weights:
            model.load_state_dict(torch.load(args.weights, map_location="cpu"))
        elif args.synthetic_weights:
            from .synth import synthetic_fid_inception_state_dict
            model.load_state_dict(synthetic_fid_inception_state_dict(model.manifest()))
        else:
            ap.error("--weights is required to evaluate a directory of images")
    mu1, s1 = _statistics_of(args.gen_dir, model, args.batch_size, args.device)
    if args.save_stats and os.path.isdir(args.gt):
        gt = directory_statistics(args.gt, model, args.batch_size, args.device)
        gt.save(args.save_stats)
        mu2, s2 = gt.finalize()
    else:
        mu2, s2 = _statistics_of(args.gt, model, args.batch_size, args.device)
    fid = frechet_distance(mu1, s1, mu2, s2, method=args.method)
    print(f"FID for {args.gen_dir}: {fid:.2f}")
    return fid


if __name__ == "__main__":
    main()
