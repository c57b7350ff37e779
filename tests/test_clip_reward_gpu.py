"""CLIP image-similarity reward (reward_type "clip", edit_ppo/reward_model.py:512-552) on the HIP library: the image front end against the committed
PIL / transformers fixture, the two kernels of its own (embeddings + pre_layrnorm, post_layernorm + visual_projection) against fp64 arithmetic on the same
fp16 operands, the tower and the reward against the fixture (reduced model) and against tests/clip_vision_oracle.py in fp32 (ViT-L/14 width with 2 layers,
and the full 24 layers, synthetic weights), the dispatcher, reward ordering, one training iteration and the paired-directory scorer.

Bounds: the parity bounds are the figures measured on an MI355X + 10 % (the suite's convention; the measured values are in the docstrings of the tests
that assert them), and each figure must also be smaller than the error of the same graph evaluated by torch in bf16 on the same inputs.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import _lib as L
from consolver_amd import ppo
from consolver_amd.reward_model import HipCLIPVisionModel, ClipImageProcessor, load_reward_model, calculate_clip_reward, cosine_reward
from consolver_amd.synth import synthetic_clip_vision_state_dict
from tests import clip_vision_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCED = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, projection_dim=64)
WIDE2 = dict(num_hidden_layers=2)                                    # ViT-L/14 width (1024 / 16 heads / 4096 / 768), two layers

# measured on an MI355X: feature rel-L2, max reward error (see the docstrings of the parity tests); the asserted bounds are these + 10 %
MEASURED_REDUCED_FEATURE, MEASURED_REDUCED_REWARD = 8.255e-4, 1.450e-4          # torch bf16 on the same inputs: 7.278e-3, 2.945e-3
MEASURED_WIDE2_FEATURE, MEASURED_WIDE2_REWARD = 7.800e-4, 1.526e-4              # torch bf16 on the same inputs: 7.009e-3, 9.384e-4
MEASURED_FULL_FEATURE, MEASURED_FULL_REWARD = 1.479e-3, 5.493e-4                # torch bf16 on the same inputs: 1.217e-2, 6.722e-3
MEASURED_ORDERING_REWARD = 5.493e-4             # the ordering test's rewards go down to 98.5, further from 100 than the parity pairs': torch bf16 there 4.875e-3
REDUCED_FEATURE_REL_L2, REDUCED_REWARD_ERR = MEASURED_REDUCED_FEATURE * 1.1, MEASURED_REDUCED_REWARD * 1.1
WIDE2_FEATURE_REL_L2, WIDE2_REWARD_ERR = MEASURED_WIDE2_FEATURE * 1.1, MEASURED_WIDE2_REWARD * 1.1
FULL_FEATURE_REL_L2, FULL_REWARD_ERR = MEASURED_FULL_FEATURE * 1.1, MEASURED_FULL_REWARD * 1.1
ORDERING_REWARD_ERR = MEASURED_ORDERING_REWARD * 1.1


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _generator():
    spec = importlib.util.spec_from_file_location("make_clip_reward_golden", os.path.join(ROOT, "tools", "make_clip_reward_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pairs(n, seed=300):
    """n pred images (512^2 fp16) and targets = pred + noise of growing amplitude"""
    preds, targets = [], []
    for i, amp in enumerate((0.05, 0.3, 0.1, 0.6, 0.02, 0.15, 0.2, 0.4)[:n]):
        p = co.synthetic_image(seed + i, 512, 512, torch.float16)
        g = torch.Generator().manual_seed(seed + 100 + i)
        preds.append(p)
        targets.append((p.float() + amp * torch.randn(3, 512, 512, generator=g)).clamp(0, 1).half())
    return torch.stack(preds), torch.stack(targets)


@pytest.fixture(scope="module")
def reduced(golden):
    g = golden["clip_reward"]
    m = HipCLIPVisionModel(REDUCED, device=DEV)
    assert m.manifest() == co.clip_manifest(REDUCED)
    m.load_state_dict(synthetic_clip_vision_state_dict(m.manifest(), seed=int(g["weight_seed"])))
    return m


@pytest.fixture(scope="module")
def wide2():
    """the ViT-L/14 width with two layers, seeded synthetic weights, and its fp32 oracle"""
    model, proc = load_reward_model("clip", device=DEV, config=WIDE2)
    sd = synthetic_clip_vision_state_dict(model.manifest(), seed=7)
    model.load_state_dict(sd)
    return model, proc, sd, co.ClipVisionOracle(sd, WIDE2)


# ---- 1. front end ----------------------------------------------------------------------------------------------------------------------------------
def test_front_end_is_bit_identical_to_pil_and_within_half_an_fp16_ulp(golden, reduced):
    """uint8 crop == the fixture's (PIL through the installed CLIPImageProcessor) and the oracle's, fp16 and fp32 inputs at 512^2 and 1024^2; the normalised
    fp16 output within 2^-10 of the fp32 pixel_values (the fp16 half-ulp at |v| < 4; CLIP's normalisation produces |v| < 2.2)."""
    g = golden["clip_reward"]
    gen = _generator()
    for i, (name, h, w, dtype) in enumerate(gen.CASES):
        pred, target = gen.case_images(i, h, w, dtype)
        patches, crop = reduced.preprocess(torch.stack([pred, target]).to(DEV), return_crop=True)
        assert crop.dtype == torch.uint8 and crop.shape == (2, 3, 224, 224) and patches.shape == (512, 640) and patches.dtype == torch.float16
        assert np.array_equal(crop[0].cpu().numpy(), g[f"{name}_crop"]), name
        want_crops, want_pv = co.preprocess(torch.stack([pred, target]))
        assert np.array_equal(crop.cpu().numpy(), want_crops), name
        if f"{name}_pixel_values" in g.files:
            assert np.array_equal(want_pv[0].numpy(), g[f"{name}_pixel_values"])
        pv = reduced.patches_to_pixel_values(patches).float().cpu()
        assert float(want_pv.abs().max()) < 4.0
        err = float((pv - want_pv).abs().max())
        print("clip front end", name, "max abs error of the fp16 pixel_values", err)
        assert err <= 2.0 ** -10, (name, err)
        assert float(patches[:, 588:].abs().max()) == 0.0
    # a non-square image follows the processor's output-size rule (shortest edge 224: 512 x 768 -> 224 x 336); values outside [0, 1] are clamped
    img = co.synthetic_image(9, 512, 768, torch.float32)
    _, crop = reduced.preprocess((img[None] * 1.5 - 0.2).to(DEV), return_crop=True)
    assert np.array_equal(crop[0].cpu().numpy(), co.crop_uint8(co.to_uint8_hwc((img * 1.5 - 0.2).clamp(0, 1))))
    assert reduced.preprocess(img[None][:0].to(DEV)).shape == (0, 640)
    assert reduced.image_features(img[None][:0].to(DEV)).shape == (0, 64)


# ---- 2. the two kernels --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,NP,D", [(1, 256, 128), (3, 5, 128), (1, 5, 640), (3, 256, 1024), (1, 6, 1536), (2, 3, 2048)])
def test_tokens_ln_kernel(B, NP, D):
    """launch_clipv_tokens_ln against fp64 arithmetic on the same fp16 operands.  The kernel sums and normalises in fp32 and rounds once, so an output is within
    half an fp16 ulp of its fp32 value (2^-11 relative; 2^-25 absolute below the normal range), and the fp32 value within the evaluation error of a LayerNorm
    whose sums run over D / 64 (rounded up to 8) elements per lane and 6 reduction levels: with n = D / 64 + 8, eps = 2^-24, A the row's mean |x| and sigma
    its standard deviation, the mean is off by at most n eps A (that is n eps (A / sigma) |gamma| in y) and the centred, scaled value by n eps (|y| + 1).
    One row carries an offset of 200 (A / sigma ~ 150): E[x^2] - mean^2 in fp32 would miss the bound there by a factor of ten or more.
    Rows: B (NP + 1) -- 6, 18 and 7 are not multiples of the 4 rows of a workgroup; D = 128 uses a quarter of the lanes, 640 and 1536 leave a lane's last
    chunk empty for part of the wave, 2048 is the widest row built."""
    g = torch.Generator().manual_seed(D + NP)
    pe = torch.randn(B * NP, D, generator=g).half()
    cls, pos = (0.5 * torch.randn(D, generator=g)).half(), (0.5 * torch.randn(NP + 1, D, generator=g)).half()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).half(), (0.05 * torch.randn(D, generator=g)).half()
    pe[0, :] += 200.0
    out = torch.full((B * (NP + 1) + 1, D), 7.0, dtype=torch.float16, device=DEV)          # one guard row behind the output
    dpe, dcls, dpos, dg, db = (t.to(DEV) for t in (pe, cls, pos, gamma, beta))
    L.check(L.lib().cs_op_clipv_tokens_ln(L.ptr(dpe), L.ptr(dcls), L.ptr(dpos), L.ptr(dg), L.ptr(db), 1e-5, L.ptr(out), B, NP, D, L.stream_ptr(out.device)))
    x = torch.cat([cls.double().expand(B, 1, D), pe.double().view(B, NP, D)], 1) + pos.double()
    want = torch.nn.functional.layer_norm(x, (D,), gamma.double(), beta.double(), 1e-5).view(-1, D)
    got = out.cpu().double()
    assert bool((got[-1] == 7.0).all())
    xr = x.view(-1, D)
    n, eps = D / 64 + 8, 2.0 ** -24
    ratio = (xr.abs().mean(1) / xr.std(1, unbiased=False))[:, None]
    tol = 2.0 ** -11 * want.abs().clamp(min=2.0 ** -14) + n * eps * (ratio * gamma.double().abs() + want.abs() + 1)
    worst = float(((got[:-1] - want).abs() / tol).max())
    print(f"tokens_ln B={B} NP={NP} D={D}: max error / tolerance {worst:.3f}")
    assert worst <= 1.0
    assert L.lib().cs_op_clipv_tokens_ln(L.ptr(dpe), L.ptr(dcls), L.ptr(dpos), L.ptr(dg), L.ptr(db), 1e-5, L.ptr(out), B, NP, D + 64, L.stream_ptr(out.device)) != 0
    L.check(L.lib().cs_op_clipv_tokens_ln(L.ptr(dpe), L.ptr(dcls), L.ptr(dpos), L.ptr(dg), L.ptr(db), 1e-5, L.ptr(out), 0, NP, D, L.stream_ptr(out.device)))


@pytest.mark.parametrize("B,D,P", [(1, 128, 64), (3, 128, 72), (1, 1024, 72), (3, 1024, 768), (2, 640, 1), (1, 1024, 7)])
def test_head_kernel(B, D, P):
    """launch_clipv_head against fp64 arithmetic on the same fp16 operands; P = 72, 7 and 1 are not multiples of the wave size or the 8 waves of the workgroup.
    fp32 throughout: the normalised row carries a few 2^-24 of relative error, a lane adds D / 64 products in turn and the wave reduction adds 6 levels, so the
    error of an output is below (D / 64 + 16) 2^-24 sum_d |n_d w_pd|."""
    g = torch.Generator().manual_seed(D + P)
    T = 3
    x = (2.0 * torch.randn(B, T, D, generator=g) + 1.0).half()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).half(), (0.05 * torch.randn(D, generator=g)).half()
    w = (torch.randn(P, D, generator=g) * D ** -0.5).half()
    out = torch.full((B * P + 1,), 7.0, dtype=torch.float32, device=DEV)
    dx, dg, db, dw = (t.to(DEV) for t in (x, gamma, beta, w))
    L.check(L.lib().cs_op_clipv_head(L.ptr(dx), T * D, L.ptr(dg), L.ptr(db), 1e-5, L.ptr(dw), B, D, P, L.ptr(out), L.stream_ptr(out.device)))
    n = torch.nn.functional.layer_norm(x[:, 0].double(), (D,), gamma.double(), beta.double(), 1e-5)
    want = n @ w.double().T
    tol = (D / 64 + 16) * 2.0 ** -24 * (n.abs() @ w.double().abs().T)
    got = out.cpu().double()
    assert float(got[-1]) == 7.0
    worst = float(((got[:-1].view(B, P) - want).abs() / tol).max())
    print(f"head B={B} D={D} P={P}: max error / tolerance {worst:.3f}")
    assert worst <= 1.0
    L.check(L.lib().cs_op_clipv_head(L.ptr(dx), T * D, L.ptr(dg), L.ptr(db), 1e-5, L.ptr(dw), 0, D, P, L.ptr(out), L.stream_ptr(out.device)))
    assert L.lib().cs_op_clipv_head(L.ptr(dx), T * D, L.ptr(dg), L.ptr(db), 1e-5, L.ptr(dw), B, D, 0, L.ptr(out), L.stream_ptr(out.device)) != 0


def test_one_layer_model_with_a_projection_that_is_no_multiple_of_the_wave():
    """hidden 128, one layer, projection 72, batch 3 through cs_clipv_forward vs the fp32 oracle: closer than torch bf16 on the same inputs (no measured
    bound: the kernels' own bounds are the two tests above)"""
    cfg = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2, projection_dim=72)
    m = HipCLIPVisionModel(cfg, device=DEV)
    sd = synthetic_clip_vision_state_dict(m.manifest(), seed=21)
    m.load_state_dict(sd)
    pv = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(22))
    got = m.get_image_features(pixel_values=pv.to(DEV), attention_mask=None).cpu()
    assert got.shape == (3, 72) and got.dtype == torch.float32
    want, bf = co.ClipVisionOracle(sd, cfg)(pv), co.ClipVisionOracle(sd, cfg, torch.bfloat16)(pv).float()
    f, fb = rel_l2(got.numpy(), want.numpy()), rel_l2(bf.numpy(), want.numpy())
    print(f"clip one layer, P=72: feature rel-L2 {f:.3e} (bf16 {fb:.3e})")
    assert f < fb


# ---- 3 - 5. parity ----------------------------------------------------------------------------------------------------------------------------------------
def _reduced_errors(golden, reduced):
    g = golden["clip_reward"]
    gen = _generator()
    got_f, want_f, bf_f, got_r, want_r, bf_r = [], [], [], [], [], []
    for i, (name, h, w, dtype) in enumerate(gen.CASES):
        pred, target = gen.case_images(i, h, w, dtype)
        feats = reduced.image_features(torch.stack([pred, target]).to(DEV))
        assert feats.dtype == torch.float32 and feats.shape == (2, 64)
        r = calculate_clip_reward(reduced, None, pred[None].to(DEV), target[None].to(DEV), DEV)
        assert r.shape == (1, 1) and r.dtype == torch.float32
        got_f.append(feats.cpu().numpy()); want_f.append(g[f"{name}_embeds"]); bf_f.append(g[f"{name}_embeds_bf16"])
        got_r.append(r.cpu().numpy()); want_r.append(g[f"{name}_reward"]); bf_r.append(g[f"{name}_reward_bf16"])
    cat = np.concatenate
    return (rel_l2(cat(got_f), cat(want_f)), float(np.abs(cat(got_r) - cat(want_r)).max()),
            rel_l2(cat(bf_f), cat(want_f)), float(np.abs(cat(bf_r) - cat(want_r)).max()))


def test_reduced_model_matches_transformers_fixture(golden, reduced):
    """HIP (fp16 storage, fp32 accumulation) vs transformers CLIPVisionModelWithProjection in fp32 on the reduced config, images through the whole path (front
    end included).  Measured: feature rel-L2 8.255e-4, max reward error 1.450e-4; torch bf16 on the same inputs (stored in the fixture): 7.278e-3, 2.945e-3."""
    f, r, bf, br = _reduced_errors(golden, reduced)
    print(f"clip reduced: feature rel-L2 {f:.3e} (bf16 {bf:.3e}), max reward error {r:.3e} (bf16 {br:.3e})")
    assert f < bf and r < br, (f, bf, r, br)
    assert f <= REDUCED_FEATURE_REL_L2, f
    assert r <= REDUCED_REWARD_ERR, r


def _parity(model, proc, sd, orc, cfg, pred, target):
    B = pred.shape[0]
    feats = model.image_features(torch.cat([pred, target]).to(DEV)).cpu()
    rewards = ppo.calculate_reward("clip", model, proc, pred.to(DEV), target.to(DEV), DEV).cpu()
    _, pv = co.preprocess(torch.cat([pred, target]))
    want = orc(pv)
    want_r = co.clip_reward(want[:B], want[B:])
    bf = co.ClipVisionOracle(sd, cfg, torch.bfloat16)(pv).float()
    bf_r = co.clip_reward(bf[:B], bf[B:])
    return (rel_l2(feats.numpy(), want.numpy()), float((rewards - want_r).abs().max()), rel_l2(bf.numpy(), want.numpy()), float((bf_r - want_r).abs().max()),
            want_r.flatten().tolist())


def test_full_width_two_layers_matches_fp32_oracle(wide2):
    """4 images (2 pred / target pairs, 512^2 fp16) through front end + the ViT-L/14-wide tower with 2 layers + tail vs tests/clip_vision_oracle.py in fp32: the
    kernel selection of the real model (1024-wide GEMMs, 16 heads, the 16-element-per-lane embedding kernel, the 768-column head).
    Measured: feature rel-L2 7.800e-4, max reward error 1.526e-4 (rewards 99.995, 99.828); torch bf16 on the same inputs: 7.009e-3, 9.384e-4."""
    model, proc, sd, orc = wide2
    pred, target = _pairs(2)
    f, r, fb, rb, rewards = _parity(model, proc, sd, orc, WIDE2, pred, target)
    print(f"clip wide2: feature rel-L2 {f:.3e} (bf16 {fb:.3e}), max reward error {r:.3e} (bf16 {rb:.3e}); rewards {rewards}")
    assert f < fb and r < rb, (f, fb, r, rb)
    assert f <= WIDE2_FEATURE_REL_L2, f
    assert r <= WIDE2_REWARD_ERR, r


def test_full_vit_l14_depth_matches_fp32_oracle():
    """the whole ViT-L/14 (24 layers, 304 M synthetic parameters), 2 pred / target pairs at 512^2 fp16 vs the fp32 oracle.
    Measured: feature rel-L2 1.479e-3, max reward error 5.493e-4 (rewards 99.994, 99.726); torch bf16 on the same inputs: 1.217e-2, 6.722e-3.
    The CPU oracle takes about 3 s for the 4 images in fp32 and bf16 together, so both pairs are kept."""
    model, proc = load_reward_model("clip", device=DEV)
    sd = synthetic_clip_vision_state_dict(model.manifest(), seed=8)
    model.load_state_dict(sd)
    assert abs(model.flops(1) / co.config_flops() - 1.0) < 0.01
    pred, target = _pairs(2, seed=320)
    f, r, fb, rb, rewards = _parity(model, proc, sd, co.ClipVisionOracle(sd), None, pred, target)
    print(f"clip ViT-L/14: feature rel-L2 {f:.3e} (bf16 {fb:.3e}), max reward error {r:.3e} (bf16 {rb:.3e}); rewards {rewards}")
    assert f < fb and r < rb, (f, fb, r, rb)
    assert f <= FULL_FEATURE_REL_L2, f
    assert r <= FULL_REWARD_ERR, r


# ---- 6. dispatcher -----------------------------------------------------------------------------------------------------------------------------------------
def test_dispatch_shape_range_identity_and_shared_target(wide2):
    model, proc, sd, orc = wide2
    pred, target = _pairs(3)
    pred, target = pred.to(DEV), target.to(DEV)
    r = ppo.calculate_reward("clip", model, proc, pred, target, DEV)
    assert r.shape == (3, 1) and r.dtype == torch.float32 and bool(((r >= 0) & (r <= 100)).all())
    same = ppo.calculate_reward("clip", model, proc, pred, pred, DEV)
    assert float((same - 100.0).abs().max()) <= WIDE2_REWARD_ERR
    # one target shared by the batch ([1,3,H,W], encoded once) == the expanded batch: other encoder batch shapes for the same inputs, so each side is within
    # the reward bound of the exact value
    shared = calculate_clip_reward(model, proc, pred, target[:1], DEV)
    expanded = ppo.calculate_reward("clip", model, proc, pred, target[:1].expand(3, -1, -1, -1).contiguous(), DEV)
    print("clip shared target vs expanded batch: max reward difference", float((shared - expanded).abs().max()))
    assert float((shared - expanded).abs().max()) <= 2 * WIDE2_REWARD_ERR
    # fp32 images take the fp32 quantisation path; a pred / target dtype mix is encoded in two passes
    assert calculate_clip_reward(model, proc, pred.float(), target, DEV).shape == (3, 1)
    assert ppo.calculate_reward("clip", model, proc, pred[:0], target[:0], DEV).shape == (0, 1)
    with pytest.raises(TypeError):
        ppo.calculate_reward("clip", model, proc, pred.bfloat16(), target.bfloat16(), DEV)        # ToPILImage in bf16 is another quantisation: not built
    with pytest.raises(NotImplementedError):
        ppo.calculate_reward("clip", None, None, pred, target, DEV)                               # the eager transformers path is not implemented
    with pytest.raises(ValueError):
        ppo.calculate_reward("clip", model, ClipImageProcessor(image_mean=(0.5, 0.5, 0.5)), pred, target, DEV)
    with pytest.raises(ValueError):
        ppo.calculate_reward("clip", model, proc, pred, target[:2], DEV)
    with pytest.raises(RuntimeError):
        model.to("cpu")
    assert model.to(DEV) is model and model.eval() is model
    for rt in ("depth", "inception", "segmentation", "llava", "qwen_vl"):
        with pytest.raises(NotImplementedError):
            ppo.calculate_reward(rt, model, proc, pred, target, DEV)


# ---- 7. ordering --------------------------------------------------------------------------------------------------------------------------------------------
ORDERING_AMPS = (0.1, 0.3, 0.6, 1.0, 1.5)


def test_reward_ordering(wide2):
    """a target plus noise of growing amplitude in normalised space: the HIP rewards are strictly ordered like the oracle's.  The amplitudes separate the
    oracle's rewards (99.991, 99.914, 99.615, 99.105, 98.451: smallest gap 7.65e-2) by more than twice the reward bounds asserted here and in the width test
    (asserted).  Measured: max reward error 5.493e-4 (at the reward 98.45); torch bf16 on the same inputs: 4.875e-3."""
    model, proc, sd, orc = wide2
    _, pv = co.preprocess(co.synthetic_image(500, 512, 512, torch.float32)[None])
    g = torch.Generator().manual_seed(501)
    noisy = torch.cat([pv + a * torch.randn(pv.shape, generator=g) for a in ORDERING_AMPS])
    n = len(ORDERING_AMPS)
    want_f = orc(torch.cat([noisy, pv]))
    want = co.clip_reward(want_f[:-1], want_f[-1:].expand(n, -1))
    bf_f = co.ClipVisionOracle(sd, WIDE2, torch.bfloat16)(torch.cat([noisy, pv])).float()
    bf_err = float((co.clip_reward(bf_f[:-1], bf_f[-1:].expand(n, -1)) - want).abs().max())
    gaps = (want[:-1] - want[1:]).flatten()
    print("clip oracle rewards", want.flatten().tolist(), "min gap", float(gaps.min()))
    assert float(gaps.min()) > 2 * max(WIDE2_REWARD_ERR, ORDERING_REWARD_ERR)                     # the case separates the rewards by more than the error allowed
    feats = model.get_image_features(pixel_values=torch.cat([noisy, pv]).to(DEV))
    assert feats.shape == (n + 1, 768) and feats.dtype == torch.float32
    got = cosine_reward(feats[:-1], feats[-1:])
    err = float((got.cpu() - want).abs().max())
    print("clip hip rewards", got.flatten().tolist(), f"max error {err:.3e} (bf16 {bf_err:.3e})")
    assert bool((got[:-1] > got[1:]).all())
    assert err < bf_err and err <= ORDERING_REWARD_ERR, (err, bf_err)


# ---- 8. training iteration -----------------------------------------------------------------------------------------------------------------------------------
def test_train_iteration_with_clip_reward(reduced):
    """train_ppo.py:322-437 with reward_type "clip" on the reduced UNet / VAE of the PPO tests and the reduced tower (128^2 decoded images: the front end
    upscales to 224): finite loss and gradient norm, reward in range; collect_rollout's rewards are the dispatcher's on the decoded images, bit for bit."""
    from consolver_amd.vae import HipAutoencoderKL, decode_latents
    from consolver_amd.synth import synthetic_vae_state_dict, synthetic_prompt_embeds
    import random
    from tests._models import get_unet
    unet, _ = get_unet(dict(layers_per_block=1, sample_size=16), seed=5)
    vae = HipAutoencoderKL(dict(layers_per_block=1, sample_size=16), device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=6))
    sch = consolver_amd.PPOScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing",
                                     order_dim=4, scaler_dim=0, factor_net_kwargs=dict(hidden_dim=32, num_actions=11))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in sch.factor_net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    sch.factor_net.to(DEV)
    sch.factor_net.sampler = "inverse_cdf"
    B = 4
    batch = ([f"p{i}" for i in range(B)], torch.randn(B, 4, 16, 16, generator=g).half().to(DEV),
             (torch.randn(B, 4, 16, 16, generator=g) * 0.18215).half().to(DEV))
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half().to(DEV), synthetic_prompt_embeds(B, seed=1002).half().to(DEV)
    tr = ppo.PolicyTrainer(sch.factor_net, lr=1e-3)
    proc = reduced.processor
    out = ppo.train_iteration(tr, None, sch, unet, vae, batch, None, cfg=3.0, num_inference_steps=4, ppo_epochs=2, reward_type="clip", prompt_embeds=pe,
                              negative_prompt_embeds=ne, rng=random.Random(0), reward_model=reduced, reward_model_processor=proc)
    assert torch.isfinite(out["loss"]) and torch.isfinite(out["norm"]) and 0.0 <= float(out["reward"]) <= 100.0
    assert tr.step_count == 2
    tgt = batch[2][:1].expand(B, -1, -1, -1).contiguous()
    roll = ppo.collect_rollout(None, sch, unet, vae, batch[1], batch[0], None, tgt, num_inference_steps=3, reward_type="clip", reward_model=reduced,
                               reward_model_processor=proc, prompt_embeds=pe, negative_prompt_embeds=ne, identical_inputs=False)
    assert roll["rewards"].shape == (B, 1) and bool(((roll["rewards"] >= 0) & (roll["rewards"] <= 100)).all()) and bool(torch.isfinite(roll["advantages"]).all())
    # the rollout's reward is the dispatcher's on the images the rollout decoded (same decode batches, same encoder batch: bit-identical)
    pred_img, tgt_img = decode_latents(vae, roll["model_pred"], batch_size=8), decode_latents(vae, tgt, batch_size=8)
    assert torch.equal(calculate_clip_reward(reduced, proc, pred_img, tgt_img, DEV), roll["rewards"])
    # identical_inputs: the teacher image is decoded once and handed over as [1,3,H,W] (encoded once)
    rep = ppo.collect_rollout(None, sch, unet, vae, batch[1][:1].expand(B, -1, -1, -1).contiguous(), [batch[0][0]] * B, None, tgt, num_inference_steps=3,
                              reward_type="clip", reward_model=reduced, reward_model_processor=proc, prompt_embeds=pe[:1].expand(B, -1, -1).contiguous(),
                              negative_prompt_embeds=ne[:1].expand(B, -1, -1).contiguous(), identical_inputs=True)
    assert rep["rewards"].shape == (B, 1) and bool(((rep["rewards"] >= 0) & (rep["rewards"] <= 100)).all())
    shared = calculate_clip_reward(reduced, proc, decode_latents(vae, rep["model_pred"], batch_size=8), decode_latents(vae, tgt[:1], batch_size=1), DEV)
    assert torch.equal(shared, rep["rewards"])


# ---- 9. scorer ---------------------------------------------------------------------------------------------------------------------------------------------
def test_score_image_pairs_with_clip(tmp_path, reduced):
    from consolver_amd import evaluation as ev
    for i in range(3):
        a = co.synthetic_image(600 + i, 96, 96)
        b = (a + 0.1 * i * torch.randn(3, 96, 96, generator=torch.Generator().manual_seed(i))).clamp(0, 1)
        ev.save_generation(str(tmp_path / "a"), 0, i, a, "p")
        ev.save_generation(str(tmp_path / "b"), 0, i, b, "p")
    pairs = ev.find_image_pairs(str(tmp_path / "a"), str(tmp_path / "b"))
    res = ev.score_image_pairs(pairs, reward_types=("image_psnr", "clip"), batch_size=2, device=DEV, reward_models={"clip": (reduced, reduced.processor)})
    assert len(res["clip"]) == 3 and abs(res["clip"][0] - 100.0) < 1e-3 and all(0 <= v <= 100 for v in res["clip"])
    with pytest.raises(NotImplementedError):
        ev.score_image_pairs(pairs, reward_types=("clip",), device=DEV)
