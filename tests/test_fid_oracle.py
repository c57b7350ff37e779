"""FID on the host: the restatement (tests/fid_oracle.py) against the committed fixture and against PIL / torch themselves, the Fréchet distance of
consolver_amd.fid, and the host side of its statistics object and directory listing.  No GPU."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from consolver_amd import fid
from consolver_amd.synth import synthetic_fid_inception_state_dict
from tests import fid_oracle as fo
from tests import inception_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _generator():
    spec = importlib.util.spec_from_file_location("make_fid_golden", os.path.join(ROOT, "tools", "make_fid_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- fixture ------------------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_inputs_and_pil_rows_reproduce(golden):
    g, gen = golden["fid"], _generator()
    assert list(g["cases"]) == [c[0] for c in gen.RESIZE_CASES] and np.array_equal(g["rows"], gen.ROWS)
    assert g["rows"][0] == 0 and g["rows"][-1] == 298
    for i, (name, h, w) in enumerate(gen.RESIZE_CASES):
        u8 = g[f"{name}_u8"]
        assert u8.shape == (2, h, w, 3) and np.array_equal(u8, gen.case_images(i)) and not np.array_equal(u8[0], u8[1])
        for k in range(2):
            assert np.array_equal(fo.pil_resize(u8[k])[:, g["rows"]], g[f"{name}_rows"][k]), name        # the installed PIL gives the stored rows


def test_two_pass_double_tap_restatement_is_pil_bit_for_bit(golden):
    """horizontal pass first, stored as float32, then vertical; double taps, double accumulation ascending; a side of 299 copied: equal to
    Image.resize on mode "F" on every fixture input, and the clip is live on the upscale (results before it leave [0, 255] by more than 5)"""
    g, gen = golden["fid"], _generator()
    for name, h, w in gen.RESIZE_CASES:
        for im in g[f"{name}_u8"]:
            raw = fo.two_pass_resize(im, clip=False)
            assert np.array_equal(np.clip(raw, 0, 255), fo.pil_resize(im)), name
            if name == "up37x53":
                assert raw.min() < -5 and raw.max() > 260
            if name == "own299":
                assert np.array_equal(raw, im.transpose(2, 0, 1).astype(np.float32))
    k = fo.float_taps(640, 299)
    assert int(np.ceil(2.0 * 640 / 299)) * 2 + 1 == 11 and 8 <= max(len(t) for _, t in k) <= 11        # scale 2.14: PIL's ksize is 11
    assert all(abs(t.sum() - 1) < 1e-15 for _, t in k)


def test_float_input_is_quantised_like_the_png_writer():
    from consolver_amd.evaluation import tensor_to_uint8_hwc
    x = torch.rand(3, 9, 7, generator=torch.Generator().manual_seed(0)) * 1.2 - 0.1
    x[0, 0, :4] = torch.tensor([0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255])                        # ties: half to even
    assert np.array_equal(fo.to_uint8_hwc(x), tensor_to_uint8_hwc(x))
    assert np.array_equal(fo.to_uint8_hwc(x.half()), tensor_to_uint8_hwc(x.half()))


def test_oracle_features_reproduce_the_fixture(golden):
    g, gen = golden["fid"], _generator()
    _, pv = fo.preprocess(gen.fixture_images())
    feats = fo.FIDInceptionOracle(gen.state_dict())(pv)
    assert feats.shape == (8, fo.DIM) and feats.dtype == torch.float32
    np.testing.assert_allclose(feats.numpy(), g["features"], rtol=1e-4, atol=1e-5)
    f = g["features"]
    assert np.linalg.norm(f[0] - f[1]) / np.linalg.norm(f[1]) > 0.05                                   # the features depend on the image
    assert g["features_bf16_error"].max() < 0.5


# ---- network ------------------------------------------------------------------------------------------------------------------------------------------------
def test_pool_rules_are_torchs():
    x = torch.randn(2, 8, 5, 7, generator=torch.Generator().manual_seed(1)) - 3.0                      # all negative at the border: zero padding would show
    assert torch.equal(fo.avg_pool_valid(x), F.avg_pool2d(x, 3, 1, 1, count_include_pad=False))
    assert torch.equal(fo.max_pool_same(x), F.max_pool2d(x, 3, 1, 1))
    ones = torch.ones(1, 1, 4, 4)
    assert torch.equal(fo.avg_pool_valid(ones), ones)                                                  # 4 / 4, 6 / 6, 9 / 9
    s = F.avg_pool2d(ones, 3, 1, 1) * 9                                                                # taps inside the image
    assert s[0, 0, 0, 0] == 4 and s[0, 0, 0, 1] == 6 and s[0, 0, 1, 1] == 9
    assert float(fo.max_pool_same(x).max()) < 0                                                        # padding is absent, not zero
    one = torch.randn(1, 8, 1, 1)
    assert torch.equal(fo.avg_pool_valid(one), one) and torch.equal(fo.max_pool_same(one), one)


def test_oracle_uses_the_max_pool_in_mixed_7c_only():
    seen = []

    class Spy(fo.FIDInceptionOracle):
        def conv(self, name, x, cout, k, stride, pad):
            if isinstance(x, fo._PoolBranchInput):
                seen.append(name)
            return super().conv(name, x, cout, k, stride, pad)
    sd = synthetic_fid_inception_state_dict(fo.manifest(), seed=3)
    pv = torch.randn(1, 3, 299, 299, generator=torch.Generator().manual_seed(2))
    a = Spy(sd, torch.float32)(pv)
    assert seen == [p + ".branch_pool" for p in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7b", "Mixed_7c")]
    b = io.InceptionOracle.__call__                                                                     # torchvision's pools give other features
    sd_fc = dict(sd, **{"fc.weight": torch.eye(fo.DIM), "fc.bias": torch.zeros(fo.DIM)})
    tv = b(io.InceptionOracle(sd_fc, torch.float32), pv)
    assert a.shape == (1, fo.DIM) and not torch.allclose(a, tv, rtol=1e-3, atol=1e-4)


def test_manifest_is_the_inception_one_without_fc():
    m = fo.manifest()
    assert len(m) == 564 and not any(k.startswith("fc.") or k.startswith("AuxLogits.") for k, _ in m)
    assert m == io.manifest()[:-2]
    model = fid.HipFIDInception()                                                                       # create is host only
    assert [(k, tuple(s)) for k, s in model.manifest()] == [(k, tuple(s)) for k, s in m]
    assert abs(model.flops(1) / (io.config_flops(299) - 2.0 * 2048 * 1000) - 1) < 1e-9
    assert model.patch_cols == 8 and model.num_tokens == 64
    sd = synthetic_fid_inception_state_dict(model.manifest())
    assert set(sd) == {k for k, _ in m}


# ---- Fréchet distance -------------------------------------------------------------------------------------------------------------------------------------------
def _random_stats(d, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d)) @ rng.normal(size=(d, d)) / np.sqrt(d) + rng.normal(size=d)
    return fo.statistics(x)


@pytest.mark.parametrize("d", [64, 128])
def test_frechet_distance(d):
    mu1, s1 = _random_stats(d, 4 * d, d)
    mu2, s2 = _random_stats(d, 4 * d, d + 1)
    for method in ("sqrtm", "eigh"):
        assert abs(fid.frechet_distance(mu1, s1, mu1, s1, method=method)) <= 1e-9 * np.trace(s1), method                     # identical statistics
    a, b = np.random.default_rng(d).uniform(0.1, 3.0, size=(2, d))
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((mu1 - mu2) ** 2).sum()
    for method in ("sqrtm", "eigh"):
        assert abs(fid.frechet_distance(mu1, np.diag(a), mu2, np.diag(b), method=method) / want - 1) <= 1e-10, method       # diagonal covariances
    fs, fe = fid.frechet_distance(mu1, s1, mu2, s2, method="sqrtm"), fid.frechet_distance(mu1, s1, mu2, s2, method="eigh")
    assert fs > 0 and abs(fs / fe - 1) <= 1e-9                                                                               # the two routes, full rank
    assert abs(fe / fo.frechet_distance(mu1, s1, mu2, s2) - 1) <= 1e-12                                                      # the oracle's is the eigh route
    assert fid.frechet_distance(mu1, s1, mu2, s2) == fs                                                                      # scipy is importable here: the default
    mu3, s3 = _random_stats(d, d // 4, d + 2)                                                                                # n < d: rank deficient
    mu4, s4 = _random_stats(d, d // 4, d + 3)
    r = fid.frechet_distance(mu3, s3, mu4, s4, method="eigh")
    assert np.isfinite(r) and r > 0
    assert abs(fid.frechet_distance(mu3, s3, mu3, s3, method="eigh")) <= 1e-6 * np.trace(s3)
    with pytest.raises(ValueError):
        fid.frechet_distance(mu1, s1, mu2[:-1], s2[:-1, :-1])
    with pytest.raises(ValueError):
        fid.frechet_distance(mu1, s1, mu2, s2, method="cholesky")


def test_sqrtm_route_refuses_a_complex_root():
    s1 = np.diag([1.0, 1.0])
    s2 = np.diag([-1.0, -4.0])                                                                         # no covariance: the root of the product is imaginary
    with pytest.raises(ValueError):
        fid.frechet_distance(np.zeros(2), s1, np.zeros(2), s2, method="sqrtm")


# ---- statistics object (host side) ---------------------------------------------------------------------------------------------------------------------------------
def _partial(x, tmp_path, name):
    """a FIDStatistics on the host holding the accumulators of x, through the partial file"""
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        np.savez(f, sum=x.sum(0), outer=x.T @ x, n=np.int64(x.shape[0]))
    return fid.FIDStatistics.load_partial(p, device="cpu")


def test_merge_of_two_halves_is_the_concatenation(tmp_path):
    x = np.random.default_rng(0).integers(-8, 9, size=(23, 48)).astype(np.float64)                      # integers: every sum is exact
    a, b, whole = _partial(x[:10], tmp_path, "a.npz"), _partial(x[10:], tmp_path, "b.npz"), _partial(x, tmp_path, "w.npz")
    assert a.merge(b) is a and a.n == 23 and a.d == 48
    assert torch.equal(a.sum, whole.sum) and torch.equal(a.outer, whole.outer)
    a.save_partial(str(tmp_path / "m.npz"))
    back = fid.FIDStatistics.load_partial(str(tmp_path / "m.npz"), device="cpu")
    assert back.n == 23 and torch.equal(back.sum, a.sum) and torch.equal(back.outer, a.outer) and back.sum.dtype == torch.float64
    with pytest.raises(ValueError):
        a.merge(fid.FIDStatistics(16, device="cpu"))
    with pytest.raises(RuntimeError):
        a.finalize()                                                                                   # the finalize is a HIP kernel: no host fallback
    with pytest.raises(ValueError):
        fid.FIDStatistics(24, device="cpu")


def test_saved_statistics_round_trip_exactly(tmp_path):
    mu, sigma = _random_stats(32, 100, 5)
    p = str(tmp_path / "stats.npz")
    fid.save_statistics(p, mu, sigma, 100)
    mu2, sigma2, n = fid.FIDStatistics.load(p)
    assert n == 100 and np.array_equal(mu, mu2) and np.array_equal(sigma, sigma2) and mu2.dtype == np.float64
    with np.load(p) as z:
        assert sorted(z.files) == ["mu", "n", "sigma"]
    q = str(tmp_path / "other.npz")
    fid.save_statistics(q, mu + 1, sigma, 100)
    assert abs(fid.compute_fid(p, q) / 32 - 1) < 1e-9                                                  # two .npz files need no model: |delta mu|^2 = 32
    with pytest.raises(ValueError):
        fid.compute_fid(str(tmp_path), q)                                                              # a directory needs a model


def test_directory_listing(tmp_path):
    for rel in ("b/2.png", "b/10.PNG", "a.jpg", "c/d/e.jpeg", "z.txt", "c/notes.json", "png", "c/x.bmp"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    got = [os.path.relpath(p, tmp_path) for p in fid.list_images(str(tmp_path))]
    assert got == sorted(["b/2.png", "b/10.PNG", "a.jpg", "c/d/e.jpeg"])
    assert got == ["a.jpg", "b/10.PNG", "b/2.png", "c/d/e.jpeg"]
