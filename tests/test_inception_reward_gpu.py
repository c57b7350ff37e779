"""Inception-v3 logit-cosine reward (reward_type "inception", edit_ppo/reward_model.py:98-108, 319-356) on the HIP library, everything through the C ABI: the
kernels of incep_ops.hip one by one against torch, the image front end against the committed PIL fixture, the model and the reward against
tests/inception_oracle.py (the fp32 weights evaluated in float64; the fixture's calibrated weights at sizes 107 and 139, and 299 from 512 x 512 images), and the reward's argument forms.

Op-level bounds, derived (as in test_segmentation_reward_gpu.py): every kernel accumulates in fp32 and rounds ONCE to fp16 on the store, the operands of the
reference are the same fp16 values, so an output element carries a relative error of at most 2^-11 (half an fp16 ulp) plus fp32 summation noise of a few
2^-24.  Hence rel-L2 <= 2^-11 = 4.9e-4, asserted as 5e-4, and max |error| <= (2^-11 + 2^-15) max |reference|.  The max pool is exact.  The head is fp32
throughout: rel-L2 <= 1e-5.

Model-level rule.  The network is sensitive (94 BatchNorm-renormalised ReLU layers with random filters amplify a perturbation; torch's own bf16 evaluation
is 0.17 .. 0.47 rel-L2 from fp32 on the fixture cases), so: (a) the logits' rel-L2 against the fp32 oracle is smaller than that of the same graph evaluated
by torch in bf16 on the same inputs, and at most the figure measured on an MI355X + 10 %; (b) |reward - oracle reward| <= 100 (e_pred + e_target) with e the
per-image logit rel-L2 of the same test (for unit vectors |delta cos| <= 2 (e_a + e_b), and the reward is 50 cos); (c) model(pixel_values) equals
image_features.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from consolver_amd import _lib as L
from consolver_amd import ppo
from consolver_amd.reward_model import HipInceptionV3, InceptionImageProcessor, calculate_inception_reward, load_inception_reward
from tests import inception_oracle as io

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_REL_L2 = 5e-4                       # one fp16 rounding of an fp32-accumulated value: 2^-11 = 4.9e-4
F16_MAX_REL = 2.0 ** -11 + 2.0 ** -15   # ... per element, relative to the largest reference magnitude

# the largest per-image logits rel-L2 against the fp32 oracle measured on an MI355X (see the docstrings of the parity tests); the asserted bounds are these + 10 %
MEASURED_FIXTURE_LOGITS = {107: 7.111e-2, 139: 5.923e-2}      # torch bf16 on the same images: 4.750e-1, 3.518e-1
MEASURED_FULL_LOGITS = 1.555e-2         # torch bf16 on the same image: 1.198e-1
FULL_AMPLITUDE = 0.2                    # noise of the full-size pair: the oracle's reward must lie in (70, 97)
FULL_GRID = (3, 3)                      # the random field behind the full-size clean image (see test_oracle_gaps_exceed_the_reward_bound)
ORDER_AMPLITUDES = (0.05, 0.2, 0.8)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _generator():
    spec = importlib.util.spec_from_file_location("make_inception_golden", os.path.join(ROOT, "tools", "make_inception_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _model(size, n_images=16):
    """(HIP model, fp32 oracle, bf16 comparator) on the calibrated weights of the generator"""
    sd = _generator().state_dict(size, n_images)
    model, _ = load_inception_reward(DEV, dict(image_size=size))
    model.load_state_dict(sd)
    return model, io.InceptionOracle(sd), io.InceptionOracle(sd, torch.bfloat16)


def _check_f16(got, want, what):
    got, want = got.float().cpu(), want.float()
    e, m = rel_l2(got.numpy(), want.numpy()), float((got - want).abs().max())
    print(what, f"rel-L2 {e:.3e} max abs {m:.3e} (max |ref| {float(want.abs().max()):.3f})")
    assert e <= F16_REL_L2, (what, e)
    assert m <= F16_MAX_REL * float(want.abs().max()) + 1e-7, (what, m)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV)


# ---- op level ---------------------------------------------------------------------------------------------------------------------------------------
FORMS = {"1x1": (1, 1, 1, 0, 0), "3x3": (3, 3, 1, 0, 0), "3x3s2": (3, 3, 2, 0, 0), "3x3p1": (3, 3, 1, 1, 1), "5x5p2": (5, 5, 1, 2, 2), "1x7": (1, 7, 1, 0, 3),
         "7x1": (7, 1, 1, 3, 0), "1x3": (1, 3, 1, 0, 1), "3x1": (3, 1, 1, 1, 0)}
SIZES = ((3, 3), (5, 7), (8, 8), (17, 17), (35, 33))
CHANNELS = ((8, 32), (48, 64), (80, 192), (192, 48), (768, 160), (448, 384))


@pytest.mark.parametrize("form", list(FORMS))
def test_conv_matches_torch_in_a_concat_slice(form):
    """cs_op_incep_conv vs relu(F.conv2d(x.float(), w16.float(), stride, padding) + bias) in fp32 on the fp16 operands, B = 2.  Every spatial size of SIZES
    the form admits (an unpadded 3 x 3 fits 3 x 3 with one output pixel; the 7-tap filters run at 8 x 8 and larger), so: one-pixel outputs, odd grids, a
    ragged last 32-pixel tile, more than one workgroup (35 x 33 x 2 = 2310 pixels).  Every (Cin, Cout) of CHANNELS: K per tap no multiple of 32 (8, 48, 80),
    ragged last filter chunk (192, 48, 160), and Cin = 8 with 3 real channels whose other 5 hold NaN.  Written at column offsets 0 and 32 of a row 48
    wider than Cout that is pre-filled with a sentinel, the slice itself NaN: the slice is fully written and nothing outside it changes."""
    kh, kw, stride, ph, pw = FORMS[form]
    B, lib = 2, L.lib()
    g = torch.Generator().manual_seed(kh * 100 + kw * 10 + stride + ph)
    ran = 0
    for H, W in SIZES:
        if H + 2 * ph < kh or W + 2 * pw < kw or (max(kh, kw) == 7 and min(H, W) < 8):
            continue
        for cin, cout in CHANNELS:
            creal = 3 if cin == 8 else cin
            x = torch.randn(B, cin, H, W, generator=g).half()
            w = (torch.randn(cout, creal, kh, kw, generator=g) / (creal * kh * kw) ** 0.5).half()
            bias = 0.5 * torch.randn(cout, generator=g)
            want = F.relu(F.conv2d(x[:, :creal].float(), w.float(), None, stride, (ph, pw)) + bias[None, :, None, None])
            Ho, Wo = want.shape[2:]
            if creal < cin:
                x[:, creal:] = float("nan")                     # the padding channels: never used
            wp = torch.zeros(cout, kh * kw, cin, dtype=torch.float16)
            wp[:, :, :creal] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, creal)
            xd, wd, bd = _nhwc(x), wp.to(DEV), bias.to(DEV)
            ld = cout + 48
            for col in (0, 32):
                buf = torch.full((B * Ho * Wo, ld), 7.0, dtype=torch.float16, device=DEV)
                buf[:, col:col + cout] = float("nan")
                L.check(lib.cs_op_incep_conv(L.ptr(xd), B, H, W, cin, creal, L.ptr(wd), L.ptr(bd), cout, kh, kw, stride, ph, pw, L.ptr(buf), ld, col,
                                             L.stream_ptr(DEV)))
                got = buf[:, col:col + cout].reshape(B, Ho, Wo, cout).permute(0, 3, 1, 2)
                _check_f16(got, want, f"conv {form} {H}x{W} {cin}->{cout} at column {col}")
                keep = torch.ones(ld, dtype=torch.bool)
                keep[col:col + cout] = False
                assert bool((buf[:, keep.to(DEV)] == 7.0).all())
                ran += 1
    assert ran >= 2 * 2 * len(CHANNELS)


def test_conv_refuses_what_it_cannot_index():
    lib, x = L.lib(), torch.zeros(64, dtype=torch.float16, device=DEV)
    p = L.ptr(x)
    for args in ((1, 2, 2, 8, 8, p, None, 16, 3, 3, 1, 0, 0, p, 16, 0),        # a 2 x 2 image holds no unpadded 3 x 3 window
                 (1, 4, 4, 12, 12, p, None, 16, 1, 1, 1, 0, 0, p, 16, 0),      # Cin % 8
                 (1, 4, 4, 8, 8, p, None, 24, 1, 1, 1, 0, 0, p, 24, 0),        # Cout % 16
                 (1, 4, 4, 8, 8, p, None, 16, 1, 1, 3, 0, 0, p, 16, 0),        # stride 3
                 (1, 4, 4, 8, 8, p, None, 16, 1, 1, 1, 0, 0, p, 16, 8)):       # the slice leaves the row
        assert lib.cs_op_incep_conv(p, *args, L.stream_ptr(DEV)) != 0


@pytest.mark.parametrize("H,W", [(7, 7), (9, 8), (35, 35)])
def test_max_pool_into_a_concat_slice_is_exact(H, W):
    B, C, ld = 2, 288, 768
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * W)).half()
    want = F.max_pool2d(x.float(), 3, 2).half()
    Ho, Wo = want.shape[2:]
    xd = _nhwc(x)
    for col in (0, 480):
        buf = torch.full((B * Ho * Wo, ld), 7.0, dtype=torch.float16, device=DEV)
        buf[:, col:col + C] = float("nan")
        L.check(L.lib().cs_op_incep_maxpool(L.ptr(xd), B, H, W, C, L.ptr(buf), ld, col, L.stream_ptr(DEV)))
        assert torch.equal(buf[:, col:col + C].reshape(B, Ho, Wo, C).permute(0, 3, 1, 2).cpu(), want)
        keep = torch.ones(ld, dtype=torch.bool)
        keep[col:col + C] = False
        assert bool((buf[:, keep.to(DEV)] == 7.0).all())


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8), (17, 17)])
def test_avg_pool_divides_by_nine_everywhere(H, W):
    B, C = 2, 192
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H * 10 + W)).half()
    want = F.avg_pool2d(x.float(), 3, 1, 1)                     # count_include_pad = True: always / 9
    out = torch.full((B, H, W, C), float("nan"), dtype=torch.float16, device=DEV)
    xd = _nhwc(x)
    L.check(L.lib().cs_op_incep_avgpool(L.ptr(xd), B, H, W, C, L.ptr(out), L.stream_ptr(DEV)))
    _check_f16(out.permute(0, 3, 1, 2), want, f"avgpool {H}x{W}")


@pytest.mark.parametrize("G", [1, 2, 8])
def test_head_is_fp32(G):
    """global mean + fc vs torch in fp32 on the same fp16 activations and fp16 weights: the mean is not rounded to fp16 on the way (rel-L2 <= 1e-5)"""
    B, C, N = 3, 2048, 1000
    g = torch.Generator().manual_seed(G)
    x = torch.randn(B, C, G, G, generator=g).half()
    w = (torch.randn(N, C, generator=g) / C ** 0.5).half()
    bias = 0.05 * torch.randn(N, generator=g)
    want = F.linear(x.float().mean((2, 3)), w.float(), bias)
    mean = torch.empty(B, C, dtype=torch.float32, device=DEV)
    out = torch.full((B, N), float("nan"), dtype=torch.float32, device=DEV)
    xd, wd, bd = _nhwc(x), w.to(DEV), bias.to(DEV)
    L.check(L.lib().cs_op_incep_head(L.ptr(xd), B, G * G, C, L.ptr(wd), L.ptr(bd), N, L.ptr(mean), L.ptr(out), L.stream_ptr(DEV)))
    e = rel_l2(out.cpu().numpy(), want.numpy())
    print(f"head {G}x{G} rel-L2 {e:.3e}")
    assert e <= 1e-5
    assert rel_l2(mean.cpu().numpy(), x.float().mean((2, 3)).numpy()) <= 1e-6


# ---- front end ----------------------------------------------------------------------------------------------------------------------------------------
def test_front_end_is_bit_identical_to_pil(golden):
    """torchvision's Resize + CenterCrop on the installed PIL (stored) vs cs_incep_preprocess: the uint8 crops equal on every case -- the square ones, and the
    two non-square ones on either side of the round-half-even crop offset; pixel values within 2^-10 of ToTensor + Normalize in fp32"""
    g, gen = golden["inception_reward"], _generator()
    for i, (name, size, hw, dtype, amp) in enumerate(gen.CASES):
        model = _model(size)[0]
        pred, target = gen.case_images(i)
        patches, crop = model.preprocess(torch.stack([pred, target]).to(DEV), return_crop=True)
        assert np.array_equal(crop.cpu().numpy(), g[f"{name}_u8"]), name
        want = torch.stack([io.normalize_uint8(c) for c in g[f"{name}_u8"]])
        d = float((model.patches_to_pixel_values(patches).float().cpu() - want).abs().max())
        print(name, "pixel values max abs", d)
        assert d <= 2.0 ** -10 and bool((patches[:, 3:] == 0).all()), name


# ---- model ----------------------------------------------------------------------------------------------------------------------------------------------
def _parity(model, oracle, comparator, images, what):
    """rules (a) .. (c) on a [2n,3,H,W] stack of (preds, targets) -> (per-image errors, HIP rewards, oracle rewards)"""
    n = images.shape[0] // 2
    _, pv = io.preprocess(images, model.crop)
    want = oracle(pv)
    eb = ((comparator(pv) - want).norm(dim=1) / want.norm(dim=1)).tolist()
    got = model.image_features(images.to(DEV))
    e = ((got.cpu() - want).norm(dim=1) / want.norm(dim=1)).tolist()
    print(what, "logit rel-L2 per image", [f"{x:.3e}" for x in e], "bf16 comparator", [f"{x:.3e}" for x in eb])
    assert max(e) < max(eb), (what, e, eb)
    patches = model.preprocess(images.to(DEV))
    assert torch.equal(model(pixel_values=model.patches_to_pixel_values(patches)), got)                  # (c)
    r = calculate_inception_reward(model, model.processor, images[:n].to(DEV), images[n:].to(DEV)).cpu()
    ro = io.inception_reward(want[:n], want[n:])
    for k in range(n):
        bound = 100 * (e[k] + e[n + k])
        print(what, "reward", float(r[k]), "oracle", float(ro[k]), "bound", bound)
        assert abs(float(r[k]) - float(ro[k])) <= bound + 1e-4, (what, k)                              # (b)
    return e, r, ro


@pytest.mark.parametrize("size", [107, 139])
def test_fixture_logits_and_rewards(golden, size):
    """The calibrated fixture weights at full widths (last grid 2 x 2 at 107, 3 x 3 at 139) on the fixture cases.  Measured on an MI355X, per image: 1.7e-2 ..
    7.1e-2 (107) and 2.1e-2 .. 5.9e-2 (139), a sixth to an eighth of the bf16 comparator's figure for the same image; the rewards are within 0.08 of the
    oracle's, far inside rule (b)."""
    g, gen = golden["inception_reward"], _generator()
    model, oracle, comparator = _model(size)
    worst = 0.0
    for i, (name, s, hw, dtype, amp) in enumerate(gen.CASES):
        if s != size:
            continue
        pred, target = gen.case_images(i)
        e, r, ro = _parity(model, oracle, comparator, torch.stack([pred, target]), name)
        np.testing.assert_allclose(ro.numpy(), g[f"{name}_reward"], rtol=1e-5, atol=1e-4)
        worst = max(worst, max(e))
    print(f"size {size}: largest logit rel-L2 {worst:.3e}")
    assert worst <= 1.1 * MEASURED_FIXTURE_LOGITS[size]


def test_full_size_pair_from_512():
    """299 from 512 x 512 fp16 images (grids 149 .. 8), weights calibrated on the 16 images at 299.  Measured on an MI355X: 1.56e-2 (the noisy image) and
    5.77e-3 (the smooth one), bf16 comparator 1.20e-1 and 5.36e-2; reward 90.304 against the oracle's 90.287."""
    gen = _generator()
    model, oracle, comparator = _model(299)
    assert abs(model.flops(1) / io.config_flops(299) - 1) < 0.01
    pred, target = gen.noisy_pair(400, (512, 512), FULL_AMPLITUDE, "float16", FULL_GRID)
    e, r, ro = _parity(model, oracle, comparator, torch.stack([pred, target]), "full size")
    assert 70 < float(ro[0]) < 97
    assert max(e) <= 1.1 * MEASURED_FULL_LOGITS


@functools.lru_cache(maxsize=None)
def _noise_ladder():
    """a clean 512 x 512 image and itself + noise of amplitude 0.05, 0.2, 0.8, at 299 -> (HIP rewards, oracle rewards, rule (b) bounds), three each"""
    gen = _generator()
    model, oracle, _ = _model(299)
    preds = torch.stack([gen.noisy_pair(400, (512, 512), a, "float16", FULL_GRID)[0] for a in ORDER_AMPLITUDES])
    clean = gen.noisy_pair(400, (512, 512), 0.0, "float16", FULL_GRID)[1][None]
    _, pv = io.preprocess(torch.cat([preds, clean]), 299)
    want = oracle(pv)
    ro = io.inception_reward(want[:3], want[3:]).flatten().tolist()
    got = model.image_features(torch.cat([preds, clean]).to(DEV)).cpu()
    e = ((got - want).norm(dim=1) / want.norm(dim=1)).tolist()
    r = calculate_inception_reward(model, None, preds.to(DEV), clean.to(DEV)).flatten().tolist()
    bounds = [100 * (e[k] + e[3]) for k in range(3)]
    print("order: HIP", r, "oracle", ro, "logit rel-L2", e, "bounds", bounds)
    return r, ro, bounds


def test_rewards_order_with_the_noise():
    """rewards of a clean image against itself + noise of amplitude 0.05, 0.2, 0.8: strictly decreasing, as the oracle's are, each within rule (b) of the
    oracle's.  Measured on an MI355X: 98.583 / 90.304 / 81.403 against the oracle's 98.589 / 90.287 / 81.494."""
    r, ro, bounds = _noise_ladder()
    assert r[0] > r[1] > r[2] and ro[0] > ro[1] > ro[2]
    assert all(abs(r[k] - ro[k]) <= bounds[k] + 1e-4 for k in range(3))


def test_oracle_gaps_exceed_the_reward_bound():
    """The oracle's own gaps against what rule (b) allows the HIP rewards to move (the sum of the two neighbours' bounds): only then does parity IMPLY the
    order asserted above.  Rule (b) is loose (the HIP rewards are within 0.1 of the oracle's, the bounds are 1 .. 3), so this constrains the test network and
    the image more than the kernels.  Two things make it hold.  The weights are calibrated on all 16 images, as the fixture's are: on two images the reward
    saturates near 77 from amplitude 0.2 on (gap to 0.8: 0.6) and the logit error of a smooth image is 2.7e-2; on 16 the reward falls steadily with the
    noise.  The clean image is a 3 x 3 random field (FULL_GRID), smoother than the fixture's 6 x 7: the fewer edges, the smaller the logit error of the
    clean image, which enters every bound (5.8e-3 against 1.1e-2).  Chosen on the host, from the oracle and an fp16-rounding emulation of the graph, before
    the GPU run; over four field seeds x three noise seeds the smaller gap was 1.2 .. 1.9 times what it has to exceed.  Measured on an MI355X: gaps
    8.30 and 8.79 against 3.39 and 4.96."""
    r, ro, bounds = _noise_ladder()
    print("gaps", ro[0] - ro[1], ro[1] - ro[2], "have to exceed", bounds[0] + bounds[1], bounds[1] + bounds[2])
    assert ro[0] - ro[1] > bounds[0] + bounds[1] and ro[1] - ro[2] > bounds[1] + bounds[2]


# ---- argument forms ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_forms():
    gen = _generator()
    model = _model(107)[0]
    proc = model.processor
    a = torch.stack([gen.noisy_pair(500 + k, (96, 120), 0.1)[0] for k in range(3)]).to(DEV)
    t = gen.noisy_pair(500, (96, 120), 0.0)[1][None].to(DEV)
    shared = calculate_inception_reward(model, proc, a, t)
    assert shared.shape == (3, 1) and shared.dtype == torch.float32
    assert torch.equal(shared, calculate_inception_reward(model, proc, a, t.expand(3, -1, -1, -1).contiguous()))          # shared target vs tiled
    assert torch.equal(shared, calculate_inception_reward(model, proc, a, t))                                             # two calls bit-identical
    assert torch.equal(shared, ppo.calculate_reward("inception", model, proc, a, t, DEV))
    mixed = calculate_inception_reward(model, proc, a, t.half())                                                          # mixed dtypes: each quantised in its own
    assert mixed.shape == (3, 1) and bool(torch.isfinite(mixed).all())
    assert calculate_inception_reward(model, proc, a[:0], t).shape == (0, 1)                                              # B = 0
    same = calculate_inception_reward(model, proc, a, a.clone())
    assert float((same - 100).abs().max()) <= 1e-4                                                                        # identical images
    feats = model.image_features(a)
    model.max_batch, keep = 2, model.max_batch
    try:
        assert torch.equal(model.image_features(a), torch.cat([model.image_features(a[:2]), model.image_features(a[2:])]))   # chunking
        assert torch.equal(model.image_features(a), feats)
    finally:
        model.max_batch = keep
    with pytest.raises(TypeError):
        calculate_inception_reward(model, proc, a.bfloat16(), t.bfloat16())
    with pytest.raises(ValueError):
        calculate_inception_reward(model, InceptionImageProcessor(139), a, t)
    with pytest.raises(RuntimeError):
        model.to("cpu")


def test_score_image_pairs_accepts_inception(tmp_path):
    from consolver_amd import evaluation
    gen = _generator()
    model = _model(107)[0]
    pairs = []
    for k in range(2):
        p, t = gen.noisy_pair(600 + k, (96, 112), 0.2)
        a, _ = evaluation.save_generation(str(tmp_path / "a"), 0, k, p, "x")
        b, _ = evaluation.save_generation(str(tmp_path / "b"), 0, k, t, "x")
        pairs.append((a, b))
    res = evaluation.score_image_pairs(pairs, ("image_psnr", "inception"), batch_size=2, device=DEV, reward_models={"inception": (model, model.processor)})
    assert len(res["image_psnr"]) == 2 and len(res["inception"]) == 2 and all(0 <= v <= 100 for v in res["inception"])
    a = torch.stack([evaluation.load_image_tensor(p, DEV) for p, _ in pairs])
    b = torch.stack([evaluation.load_image_tensor(q, DEV) for _, q in pairs])
    assert res["inception"] == [float(v) for v in calculate_inception_reward(model, None, a, b).flatten().cpu()]
