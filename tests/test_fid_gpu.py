"""FID on the HIP library, everything through the C ABI: the float bicubic front end against PIL, the two pools against torch, the fp64 statistics against
numpy, the pool3 features against tests/fid_oracle.py (the fp32 weights evaluated in float64), and the whole path -- tensors, PNG directories, the CLI.

Bounds.
* Resize: the fp32 output against PIL's, max |diff| <= 1e-4.  Derived: the two double sums can differ from the host's by ~1e-13, so each pass can move a
  float32 by one ulp (3.05e-5 below 512); the second pass has sum |k| < 1.4, hence <= 1.4 x 3.05e-5 + 3.05e-5 = 7.3e-5.  The normalised rows are fp16
  values of magnitude <= 1: half an ulp is 2^-12; asserted within 2^-11 + 2^-15 of the oracle's fp32 values as the other front ends are.
* Pools: one fp16 rounding of an fp32 sum: rel-L2 <= 5e-4 and max |error| <= (2^-11 + 2^-15) max |reference| (test_inception_reward_gpu.py's); the max is exact.
* Statistics: integer-valued features give sums that fp64 holds exactly in any order: bitwise equal to numpy.  Random fp32 features: a sum of n products in
  any order is within n 2^-53 sum |f_i f_j| of the exact value, numpy's too, hence the 2 n 2^-53 sum |f_i f_j| between them.
* Features: (a) the largest per-image rel-L2 against the oracle is smaller than that of torch's bf16 evaluation of the same graph on the same inputs, (b) it
  is at most the figure measured on an MI355X + 10 %.
"""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from consolver_amd import _lib as L
from consolver_amd import evaluation, fid
from tests import fid_oracle as fo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIZE_ABS = 1e-4
F16_REL_L2 = 5e-4
F16_MAX_REL = 2.0 ** -11 + 2.0 ** -15

# measured on an MI355X (the first run of this file on the tree that added it, pytest -s); the asserted bounds are these + 10 %
MEASURED_FIXTURE_FEATURES = 1.136e-2 # largest per-image feature rel-L2 on the 8 fixture images (3.2e-3 .. 1.14e-2; torch bf16 on the same images: 3.3e-2 .. 8.4e-2)
MEASURED_FULL_FEATURES = 1.976e-2    # ... on the 512 x 512 pair (smooth 8.5e-3, noisy 1.98e-2; torch bf16: 6.6e-2, 1.40e-1)
MEASURED_E2E_MU = 4.657e-3           # |mu - oracle mu| / |oracle mu|, the larger of the two sets
MEASURED_E2E_SIGMA = 6.620e-2        # Frobenius, relative (12 samples: the covariance of 2048 features is noisier than its mean)
MEASURED_E2E_FID = 2.159e-3          # |FID - oracle FID| / oracle FID: 2606.90 against 2612.54


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _generator():
    spec = importlib.util.spec_from_file_location("make_fid_golden", os.path.join(ROOT, "tools", "make_fid_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _front_end():
    return fid.HipFIDInception(device=DEV)               # the front end needs no weights


@functools.lru_cache(maxsize=None)
def _model():
    """(HIP model, fp32 oracle, bf16 comparator) on the generator's calibrated weights"""
    sd = _generator().state_dict()
    model = fid.load_fid_inception(DEV)
    model.load_state_dict(sd)
    return model, fo.FIDInceptionOracle(sd), fo.FIDInceptionOracle(sd, torch.bfloat16)


# ---- front end ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_resize_matches_pil(golden, case):
    g, gen = golden["fid"], _generator()
    name, h, w = gen.RESIZE_CASES[case]
    model = _front_end()
    u8 = torch.from_numpy(g[f"{name}_u8"]).permute(0, 3, 1, 2).contiguous().to(DEV)                    # [2,3,H,W]
    patches, resized = model.preprocess(u8, return_resized=True)
    assert resized.shape == (2, 3, 299, 299) and patches.shape == (2 * 299 * 299, 8)
    got = resized.cpu().numpy()
    rows = g["rows"]
    d_rows = float(np.abs(got[:, :, rows] - g[f"{name}_rows"]).max())
    want = np.stack([fo.pil_resize(im) for im in g[f"{name}_u8"]])                                     # the installed PIL, every row
    d_all = float(np.abs(got - want).max())
    print(name, "max |diff| to the stored rows", d_rows, "to PIL", d_all, "bit-identical pixels", float((got == want).mean()))
    assert d_rows <= RESIZE_ABS and d_all <= RESIZE_ABS
    assert got.min() >= 0 and got.max() <= 255
    if name == "up37x53":
        assert (got == 0).any() and (got == 255).any()                                                 # the clip acted
    # uint8, fp32 and fp16 inputs of the same image: identical output
    for x in (u8.float() / 255, (u8.float() / 255).half()):
        p2, r2 = model.preprocess(x, return_resized=True)
        assert torch.equal(r2, resized) and torch.equal(p2, patches), x.dtype
    # the normalised rows
    pv = model.patches_to_pixel_values(patches).float().cpu()
    d = float((pv - fo.normalize(want)).abs().max())
    print(name, "normalised rows max abs", d)
    assert d <= F16_MAX_REL and bool((patches[:, 3:] == 0).all())


def test_front_end_arguments():
    model = _front_end()
    x = torch.rand(2, 3, 5, 1, device=DEV)                                                             # a one-pixel side
    p, r = model.preprocess(x, return_resized=True)
    want = np.stack([fo.pil_resize(fo.to_uint8_hwc(im.cpu())) for im in x])
    assert float(np.abs(r.cpu().numpy() - want).max()) <= RESIZE_ABS
    y = torch.tensor([-1.0, 0.5 / 255, 1.5 / 255, 2.0, float("nan")], device=DEV).reshape(1, 1, 1, 5).expand(1, 3, 299, 5).contiguous()
    r = model.preprocess(y, return_resized=True)[1]
    assert r.shape == (1, 3, 299, 299) and bool(torch.isfinite(r).all())
    assert model.preprocess(x[:0]).shape == (0, 8)
    with pytest.raises(TypeError):
        model.preprocess(x.bfloat16())
    with pytest.raises(ValueError):
        model.preprocess(x[:, :2])
    with pytest.raises(RuntimeError):
        model.preprocess(x.cpu())
    with pytest.raises(RuntimeError):
        fid.HipFIDInception(device=DEV).features(x)                                                    # weights not loaded


# ---- pools ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (8, 8), (17, 17), (35, 35)])
@pytest.mark.parametrize("C", [8, 288])
def test_pools_leave_the_padding_out(H, W, C):
    B = 2
    x = (torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * 100 + W + C)) - 1.5).half()   # mostly negative: zero padding would win the max
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    for op, ref in (("avg", F.avg_pool2d(x.float(), 3, 1, 1, count_include_pad=False)), ("max", F.max_pool2d(x.float(), 3, 1, 1))):
        out = torch.full((B, H, W, C), float("nan"), dtype=torch.float16, device=DEV)
        L.check(getattr(L.lib(), f"cs_op_fid_{op}pool")(L.ptr(xd), B, H, W, C, L.ptr(out), L.stream_ptr(DEV)))
        got = out.permute(0, 3, 1, 2).float().cpu()
        if op == "max":
            assert torch.equal(got, ref)
        else:
            e, m = rel_l2(got.numpy(), ref.numpy()), float((got - ref).abs().max())
            print(f"avgpool {H}x{W} C {C} rel-L2 {e:.3e} max abs {m:.3e}")
            assert e <= F16_REL_L2 and m <= F16_MAX_REL * float(ref.abs().max()) + 1e-7
    assert L.lib().cs_op_fid_avgpool(L.ptr(xd), B, H, W, C, L.ptr(xd), L.stream_ptr(DEV)) != 0         # aliasing
    assert L.lib().cs_op_fid_maxpool(L.ptr(xd), B, H, W, 12, L.ptr(out), L.stream_ptr(DEV)) != 0       # C % 8


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _guarded(count):
    """a float64 buffer of `count` zeros with GUARD sentinel words on either side -> (whole buffer, the interior view)"""
    buf = torch.full((count + 2 * GUARD,), -7.25, dtype=torch.float64, device=DEV)
    buf[GUARD:GUARD + count] = 0
    return buf, buf[GUARD:GUARD + count]


def _accumulate(x, sum_, outer):
    xd = x if x.is_cuda else x.to(DEV)
    L.check(L.lib().cs_fid_stats_accumulate(L.ptr(xd), xd.shape[0], xd.shape[1], L.ptr(sum_), L.ptr(outer), L.stream_ptr(DEV)))


@pytest.mark.parametrize("n,d", [(1, 16), (3, 48), (67, 272), (5, 2048)])
def test_accumulate_is_exact_on_integers(n, d):
    x = torch.randint(-8, 9, (n, d), generator=torch.Generator().manual_seed(n + d)).float()
    sb, s = _guarded(d)
    ob, o = _guarded(d * d)
    _accumulate(x, s, o)
    x64 = x.double().numpy()
    assert np.array_equal(s.cpu().numpy(), x64.sum(0))
    assert np.array_equal(o.cpu().numpy().reshape(d, d), x64.T @ x64)
    _accumulate(x, s, o)                                                                               # a second call adds
    assert np.array_equal(s.cpu().numpy(), 2 * x64.sum(0)) and np.array_equal(o.cpu().numpy().reshape(d, d), 2 * (x64.T @ x64))
    for b, count in ((sb, d), (ob, d * d)):
        assert bool((b[:GUARD] == -7.25).all()) and bool((b[GUARD + count:] == -7.25).all())           # nothing outside sum and outer is written


def test_accumulate_on_random_features():
    n, d = 67, 272
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(5)) * 3 + 0.5
    x64 = x.double().numpy()
    bound = 2 * n * 2.0 ** -53 * (np.abs(x64).T @ np.abs(x64))
    s, o = _guarded(d)[1], _guarded(d * d)[1]
    _accumulate(x, s, o)
    got = o.cpu().numpy().reshape(d, d)
    err = np.abs(got - x64.T @ x64)
    print("outer: largest error / bound", float((err / bound).max()))
    assert (err <= bound).all() and np.array_equal(got, got.T)
    assert (np.abs(s.cpu().numpy() - x64.sum(0)) <= 2 * n * 2.0 ** -53 * np.abs(x64).sum(0)).all()
    # two runs are bitwise equal
    s2, o2 = _guarded(d)[1], _guarded(d * d)[1]
    _accumulate(x, s2, o2)
    assert torch.equal(s, s2) and torch.equal(o, o2)
    # two calls against one call on the concatenation: inside the bound at any split; a split at a multiple of 4 rows continues the same chain of
    # instructions, so `outer` is bitwise equal
    for split in (30, 64):
        s3, o3 = _guarded(d)[1], _guarded(d * d)[1]
        _accumulate(x[:split].contiguous(), s3, o3)
        _accumulate(x[split:].contiguous(), s3, o3)
        assert (np.abs(o3.cpu().numpy().reshape(d, d) - x64.T @ x64) <= bound).all()
        assert (np.abs(s3.cpu().numpy() - x64.sum(0)) <= 2 * n * 2.0 ** -53 * np.abs(x64).sum(0)).all()
        if split % 4 == 0:
            assert torch.equal(o3, o)


def test_finalize_matches_numpy_and_refusals():
    n, d = 40, 48
    x = torch.rand(n, d, generator=torch.Generator().manual_seed(9)) * 2
    st = fid.FIDStatistics(d, DEV)
    st.update(x[:13].to(DEV)).update(x[13:].to(DEV))
    assert st.n == n
    mu, sigma = st.finalize()
    want_mu, want_sigma = fo.statistics(x.numpy())
    assert mu.dtype == np.float64 and sigma.shape == (d, d)
    assert np.abs(mu - want_mu).max() <= 1e-12 and np.abs(sigma - want_sigma).max() <= 1e-10 * np.abs(want_sigma).max()
    # merge: two objects against one
    a, b = fid.FIDStatistics(d, DEV).update(x[:13].to(DEV)), fid.FIDStatistics(d, DEV).update(x[13:].to(DEV))
    mu2, sigma2 = a.merge(b).finalize()
    assert np.abs(sigma2 - want_sigma).max() <= 1e-10 * np.abs(want_sigma).max() and np.abs(mu2 - want_mu).max() <= 1e-12
    lib, p, q = L.lib(), L.ptr(st.sum), L.ptr(st.outer)
    xd = x.to(DEV)
    bad = torch.zeros(8 * 24, dtype=torch.float32, device=DEV)
    assert lib.cs_fid_stats_accumulate(L.ptr(bad), 8, 24, p, q, L.stream_ptr(DEV)) != 0                # d = 24
    assert lib.cs_fid_stats_accumulate(L.ptr(xd), 0, d, p, q, L.stream_ptr(DEV)) != 0                  # n = 0
    assert lib.cs_fid_stats_accumulate(None, n, d, p, q, L.stream_ptr(DEV)) != 0
    m, s = torch.empty(d, dtype=torch.float64, device=DEV), torch.empty(d, d, dtype=torch.float64, device=DEV)
    assert lib.cs_fid_stats_finalize(p, q, 1, d, L.ptr(m), L.ptr(s), L.stream_ptr(DEV)) != 0           # N = 1
    assert lib.cs_fid_stats_finalize(p, q, n, 24, L.ptr(m), L.ptr(s), L.stream_ptr(DEV)) != 0
    with pytest.raises(ValueError):
        st.update(x.to(DEV)[:, :32])
    with pytest.raises(RuntimeError):
        st.update(x)                                                                                   # a host tensor


# ---- features ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_features(golden):
    """the 8 fixture images (four sizes, uint8) on the calibrated weights against the stored oracle features.  Measured on an MI355X: see
    MEASURED_FIXTURE_FEATURES."""
    g, gen = golden["fid"], _generator()
    model = _model()[0]
    images = gen.fixture_images()
    got = torch.cat([model.features(torch.stack(images[i:i + 2]).to(DEV)) for i in range(0, 8, 2)]).cpu()
    assert got.shape == (8, 2048) and got.dtype == torch.float32
    want = torch.from_numpy(g["features"])
    e = ((got - want).norm(dim=1) / want.norm(dim=1)).tolist()
    eb = g["features_bf16_error"].tolist()
    print("fixture feature rel-L2 per image", [f"{x:.3e}" for x in e], "bf16 comparator", [f"{x:.3e}" for x in eb])
    assert max(e) < max(eb)
    assert max(e) <= 1.1 * MEASURED_FIXTURE_FEATURES


def test_full_size_pair_features():
    """a smooth and a noisy 512 x 512 image (float tensors).  Measured on an MI355X: see MEASURED_FULL_FEATURES."""
    model, oracle, comparator = _model()
    g = torch.Generator().manual_seed(77)
    clean = F.interpolate(torch.rand(1, 3, 3, 3, generator=g), size=(512, 512), mode="bicubic", align_corners=False)[0].clamp(0, 1)
    images = torch.stack([clean, (clean + 0.2 * torch.randn(3, 512, 512, generator=g)).clamp(0, 1)])
    _, pv = fo.preprocess(list(images))
    want = oracle(pv)
    eb = ((comparator(pv) - want).norm(dim=1) / want.norm(dim=1)).tolist()
    got = model.features(images.to(DEV)).cpu()
    e = ((got - want).norm(dim=1) / want.norm(dim=1)).tolist()
    print("512 x 512 pair feature rel-L2", [f"{x:.3e}" for x in e], "bf16 comparator", [f"{x:.3e}" for x in eb])
    assert torch.equal(model.features(images.half().to(DEV)).cpu(), model.features((images.half().float()).to(DEV)).cpu())
    assert max(e) < max(eb)
    assert max(e) <= 1.1 * MEASURED_FULL_FEATURES
    model.max_batch, keep = 1, model.max_batch                                                         # chunking
    try:
        assert torch.equal(model.features(images.to(DEV)).cpu(), got)
    finally:
        model.max_batch = keep


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e():
    """the two sets of 12 images at the generator's noise levels -> (sets, HIP features, HIP (mu, sigma), oracle (mu, sigma))"""
    gen = _generator()
    model, oracle, _ = _model()
    sets = [gen.e2e_set(level) for level in gen.E2E_LEVELS]
    feats, hip, orc = [], [], []
    for x in sets:
        f = model.features(x.to(DEV))
        st = fid.FIDStatistics(2048, DEV)
        st.update(f[:5]).update(f[5:])
        feats.append(f)
        hip.append(st.finalize())
        orc.append(fo.statistics(oracle(fo.preprocess(list(x))[1]).numpy()))
    return sets, feats, hip, orc


def test_end_to_end_statistics_and_distance():
    """Measured on an MI355X: see MEASURED_E2E_*."""
    _, feats, hip, orc = _e2e()
    e_mu = max(rel_l2(h[0], o[0]) for h, o in zip(hip, orc))
    e_sigma = max(rel_l2(h[1], o[1]) for h, o in zip(hip, orc))
    got = fid.frechet_distance(*hip[0], *hip[1], method="eigh")
    want = fo.frechet_distance(*orc[0], *orc[1])
    err = abs(got - want)
    print(f"end to end: mu rel-L2 {e_mu:.3e} sigma rel-F {e_sigma:.3e} FID {got:.4f} oracle {want:.4f} relative error {err / want:.3e}")
    # the statistics kernels themselves: the HIP features' own numpy statistics
    for f, h in zip(feats, hip):
        mu, sigma = fo.statistics(f.cpu().numpy())
        assert np.abs(h[0] - mu).max() <= 1e-12 * np.abs(mu).max() and np.abs(h[1] - sigma).max() <= 1e-10 * np.abs(sigma).max()
    same = fid.frechet_distance(*hip[0], *hip[0], method="eigh")
    print("FID(A, A)", same, "tr sigma", np.trace(hip[0][1]))
    assert abs(same) <= 1e-6 * np.trace(hip[0][1])
    assert want > 10 * err                                                                             # the distance is resolved
    assert e_mu <= 1.1 * MEASURED_E2E_MU and e_sigma <= 1.1 * MEASURED_E2E_SIGMA
    assert err / want <= 1.1 * MEASURED_E2E_FID


def test_directories_and_cli(tmp_path, capsys):
    sets, feats, hip, _ = _e2e()
    model = _model()[0]
    dirs = []
    for k, x in enumerate(sets):
        d = str(tmp_path / f"set{k}" / "nested")
        for i, im in enumerate(x):
            evaluation.save_generation(d, 0, i, im, "x")                                               # PNG + a .txt next to it
        dirs.append(str(tmp_path / f"set{k}"))
    want = fid.frechet_distance(*hip[0], *hip[1], method="eigh")
    # PNG files of the tensors give the tensors' features: with the same batches the distance is the same number
    st = [fid.directory_statistics(d, model, 12, DEV) for d in dirs]
    for s, f in zip(st, feats):
        ref = fid.FIDStatistics(2048, DEV).update(f)
        assert s.n == 12 and torch.equal(s.sum, ref.sum) and torch.equal(s.outer, ref.outer)
    got = fid.compute_fid(dirs[0], dirs[1], model, batch_size=12, device=DEV, method="eigh")
    ref = fid.frechet_distance(*fid.FIDStatistics(2048, DEV).update(feats[0]).finalize(), *fid.FIDStatistics(2048, DEV).update(feats[1]).finalize(), method="eigh")
    print("directories", got, "tensors", ref, "two-chunk statistics", want)
    assert got == ref and abs(got / want - 1) <= 1e-9
    # saved statistics in place of a directory
    npz = str(tmp_path / "set1.npz")
    st[1].save(npz)
    assert abs(fid.compute_fid(dirs[0], npz, model, batch_size=12, device=DEV, method="eigh") / got - 1) <= 1e-12
    # ranks: partial files merged by one process
    a, b = fid.directory_statistics(None, model, 12, DEV, fid.list_images(dirs[0])[:7]), fid.directory_statistics(None, model, 12, DEV, fid.list_images(dirs[0])[7:])
    a.save_partial(str(tmp_path / "r0.npz"))
    b.save_partial(str(tmp_path / "r1.npz"))
    merged = fid.FIDStatistics.load_partial(str(tmp_path / "r0.npz"), DEV).merge(fid.FIDStatistics.load_partial(str(tmp_path / "r1.npz"), DEV))
    mu, sigma = merged.finalize()
    assert merged.n == 12 and np.abs(sigma - hip[0][1]).max() <= 1e-10 * np.abs(hip[0][1]).max() and np.abs(mu - hip[0][0]).max() <= 1e-12 * np.abs(mu).max()
    # the CLI prints the reference's line: two directories (the loaded model handed in), then saved statistics alone (no model)
    capsys.readouterr()
    saved = str(tmp_path / "gt.npz")
    value = fid.main([dirs[0], dirs[1], "--method", "eigh", "--batch-size", "12", "--device", DEV, "--save-stats", saved], model=model)
    line = capsys.readouterr().out.strip()
    assert line == f"FID for {dirs[0]}: {value:.2f}" and re.fullmatch(r"FID for .+: \d+\.\d\d", line) and value == got
    npz0 = str(tmp_path / "set0.npz")
    st[0].save(npz0)
    value = fid.main([npz0, saved, "--method", "eigh"])
    assert capsys.readouterr().out.strip() == f"FID for {npz0}: {value:.2f}" and abs(value / got - 1) <= 1e-12
    with pytest.raises(SystemExit):
        fid.main([dirs[0], npz])                                                                       # a directory needs --weights
