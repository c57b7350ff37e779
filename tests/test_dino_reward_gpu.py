"""DINOv2 image-similarity reward (reward_type "dino", edit_ppo/reward_model.py:217-257) on the HIP library: the image front end against the committed
PIL / transformers fixture, the encoder and the reward against the fixture (reduced model) and against tests/vit_oracle.py in fp32 (full dinov2-base shape,
synthetic weights), reward ordering and advantages, the dispatcher, the unmasked head-64 attention op, and one training iteration.

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
from consolver_amd.reward_model import HipDinov2Model, DinoImageProcessor, load_reward_model, calculate_dino_reward
from consolver_amd.synth import synthetic_dinov2_state_dict
from tests import vit_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCED = dict(hidden_size=128, num_hidden_layers=3, num_attention_heads=2)

# measured on an MI355X: feature rel-L2, max reward error (see the docstrings of the two parity tests); the asserted bounds are these + 10 %
MEASURED_REDUCED_FEATURE, MEASURED_REDUCED_REWARD = 7.689e-4, 2.747e-4          # torch bf16 on the same inputs: 7.387e-3, 2.968e-3
MEASURED_BASE_FEATURE, MEASURED_BASE_REWARD = 1.168e-3, 8.011e-4                # torch bf16 on the same inputs: 1.033e-2, 1.255e-2
REDUCED_FEATURE_REL_L2 = MEASURED_REDUCED_FEATURE * 1.1
REDUCED_REWARD_ERR = MEASURED_REDUCED_REWARD * 1.1
BASE_FEATURE_REL_L2 = MEASURED_BASE_FEATURE * 1.1
BASE_REWARD_ERR = MEASURED_BASE_REWARD * 1.1


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _generator():
    spec = importlib.util.spec_from_file_location("make_dino_golden", os.path.join(ROOT, "tools", "make_dino_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def reduced(golden):
    g = golden["dino_reward"]
    m = HipDinov2Model(REDUCED, device=DEV)
    assert m.manifest() == vo.dinov2_manifest(REDUCED)
    m.load_state_dict(synthetic_dinov2_state_dict(m.manifest(), seed=int(g["weight_seed"])))
    return m


@pytest.fixture(scope="module")
def base():
    """the facebook/dinov2-base shape with seeded synthetic weights (consolver_amd.synth.synthetic_dinov2_state_dict), and its fp32 oracle"""
    model, proc = load_reward_model("dino", device=DEV)
    sd = synthetic_dinov2_state_dict(model.manifest(), seed=7)
    model.load_state_dict(sd)
    return model, proc, sd, vo.Dinov2Oracle(sd)


def test_front_end_is_bit_identical_to_pil_and_within_half_an_fp16_ulp(golden, reduced):
    """uint8 crop == the fixture's (PIL through the installed processor), fp16 and fp32 inputs at 512^2 and 1024^2; the normalised fp16 output within 2^-10 of the
    fp32 pixel_values (the fp16 half-ulp at |v| < 4; the normalisation produces |v| < 2.65)."""
    g = golden["dino_reward"]
    gen = _generator()
    for i, (name, h, w, dtype) in enumerate(gen.CASES):
        pred, target = gen.case_images(i, h, w, dtype)
        patches, crop = reduced.preprocess(torch.stack([pred, target]).to(DEV), return_crop=True)
        assert crop.dtype == torch.uint8 and crop.shape == (2, 3, 224, 224) and patches.shape == (512, 640) and patches.dtype == torch.float16
        assert np.array_equal(crop[0].cpu().numpy(), g[f"{name}_crop"]), name
        want_crops, want_pv = vo.preprocess(torch.stack([pred, target]))
        assert np.array_equal(crop.cpu().numpy(), want_crops), name
        if f"{name}_pixel_values" in g.files:
            assert np.array_equal(want_pv[0].numpy(), g[f"{name}_pixel_values"])
        pv = reduced.patches_to_pixel_values(patches).float().cpu()
        err = float((pv - want_pv).abs().max())
        print("front end", name, "max abs error of the fp16 pixel_values", err)
        assert err <= 2.0 ** -10, (name, err)
        assert float(patches[:, 588:].abs().max()) == 0.0
    # a non-square image follows the processor's output-size rule; values outside [0, 1] are clamped
    img = vo.synthetic_image(9, 512, 768, torch.float32)
    _, crop = reduced.preprocess((img[None] * 1.5 - 0.2).to(DEV), return_crop=True)
    assert np.array_equal(crop[0].cpu().numpy(), vo.crop_uint8(vo.to_uint8_hwc((img * 1.5 - 0.2).clamp(0, 1))))
    assert reduced.preprocess(img[None][:0].to(DEV)).shape == (0, 640)


def _reduced_errors(golden, reduced):
    g = golden["dino_reward"]
    gen = _generator()
    got_f, want_f, bf_f, got_r, want_r, bf_r = [], [], [], [], [], []
    for i, (name, h, w, dtype) in enumerate(gen.CASES):
        pred, target = gen.case_images(i, h, w, dtype)
        feats = reduced.image_features(torch.stack([pred, target]).to(DEV))
        assert feats.dtype == torch.float32 and feats.shape == (2, 128)
        r = calculate_dino_reward(reduced, None, pred[None].to(DEV), target[None].to(DEV), DEV)
        assert r.shape == (1, 1) and r.dtype == torch.float32
        got_f.append(feats.cpu().numpy()); want_f.append(g[f"{name}_cls"]); bf_f.append(g[f"{name}_cls_bf16"])
        got_r.append(r.cpu().numpy()); want_r.append(g[f"{name}_reward"]); bf_r.append(g[f"{name}_reward_bf16"])
    cat = np.concatenate
    return (rel_l2(cat(got_f), cat(want_f)), float(np.abs(cat(got_r) - cat(want_r)).max()),
            rel_l2(cat(bf_f), cat(want_f)), float(np.abs(cat(bf_r) - cat(want_r)).max()))


def test_reduced_model_matches_transformers_fixture(golden, reduced):
    """HIP (fp16 storage, fp32 accumulation) vs transformers Dinov2Model in fp32 on the reduced config, images through the whole path (front end included).
    Measured: feature rel-L2 7.689e-4, max reward error 2.747e-4; torch bf16 on the same inputs (stored in the fixture): 7.387e-3, 2.968e-3."""
    f, r, bf, br = _reduced_errors(golden, reduced)
    print(f"dino reduced: feature rel-L2 {f:.3e} (bf16 {bf:.3e}), max reward error {r:.3e} (bf16 {br:.3e})")
    assert f < bf and r < br, (f, bf, r, br)
    assert f <= REDUCED_FEATURE_REL_L2, f
    assert r <= REDUCED_REWARD_ERR, r


def _base_pairs():
    preds, targets = [], []
    for i, amp in enumerate((0.02, 0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.6)):
        p = vo.synthetic_image(300 + i, 512, 512, torch.float16)
        g = torch.Generator().manual_seed(400 + i)
        preds.append(p)
        targets.append((p.float() + amp * torch.randn(3, 512, 512, generator=g)).clamp(0, 1).half())
    return torch.stack(preds), torch.stack(targets)


def test_full_dinov2_base_matches_fp32_oracle(base):
    """16 images (8 pred / target pairs, 512^2 fp16) through front end + 12-layer encoder + tail vs tests/vit_oracle.py in fp32.
    Measured: feature rel-L2 1.168e-3, max reward error 8.011e-4; torch bf16 on the same inputs: 1.033e-2, 1.255e-2."""
    model, proc, sd, orc = base
    pred, target = _base_pairs()
    B = pred.shape[0]
    feats = model.image_features(torch.cat([pred, target]).to(DEV)).cpu()
    rewards = ppo.calculate_reward("dino", model, proc, pred.to(DEV), target.to(DEV), DEV).cpu()
    _, pv = vo.preprocess(torch.cat([pred, target]))
    want = orc.cls(pv)
    want_r = vo.dino_reward(want[:B], want[B:])
    bf = vo.Dinov2Oracle(sd, dtype=torch.bfloat16).cls(pv).float()
    bf_r = vo.dino_reward(bf[:B], bf[B:])
    f, r = rel_l2(feats.numpy(), want.numpy()), float((rewards - want_r).abs().max())
    fb, rb = rel_l2(bf.numpy(), want.numpy()), float((bf_r - want_r).abs().max())
    print(f"dino base: feature rel-L2 {f:.3e} (bf16 {fb:.3e}), max reward error {r:.3e} (bf16 {rb:.3e}); rewards {want_r.flatten().tolist()}")
    assert f < fb and r < rb, (f, fb, r, rb)
    assert f <= BASE_FEATURE_REL_L2, f
    assert r <= BASE_REWARD_ERR, r
    assert abs(model.flops(1) / 1e9 - 46.3) < 0.5


def test_reward_ordering_and_advantages(base):
    """a target plus noise of growing amplitude in normalised space: the HIP rewards are strictly ordered like the oracle's, and compute_advantages of them
    matches compute_advantages of the oracle's rewards within what a reward error of BASE_REWARD_ERR (test 3's measured reward error + 10 %) can do to
    (r - mean) / (std + eps) * 10.  Measured: max reward error 8.62e-4, advantages max error 3.1e-3 against a derived bound of 2.7e-2 (reward std 1.379)."""
    model, proc, sd, orc = base
    amps = (0.05, 0.1, 0.2, 0.35, 0.5, 0.8, 1.2)
    _, pv = vo.preprocess(vo.synthetic_image(500, 512, 512, torch.float32)[None])
    g = torch.Generator().manual_seed(501)
    noisy = torch.cat([pv + a * torch.randn(pv.shape, generator=g) for a in amps])
    want_f = orc.cls(torch.cat([noisy, pv]))
    want = vo.dino_reward(want_f[:-1], want_f[-1:].expand(len(amps), -1))
    gaps = (want[:-1] - want[1:]).flatten()
    print("oracle rewards", want.flatten().tolist(), "min gap", float(gaps.min()))
    assert float(gaps.min()) > 2 * BASE_REWARD_ERR                      # the case separates the rewards by more than the error allowed
    out = model(pixel_values=torch.cat([noisy, pv]).to(DEV))
    feats = out.last_hidden_state[:, 0, :]
    assert feats.shape == (len(amps) + 1, 768) and torch.equal(feats, out.pooler_output)
    from consolver_amd.reward_model import cosine_reward
    got = cosine_reward(feats[:-1], feats[-1:])
    print("hip rewards", got.flatten().tolist(), "max error", float((got.cpu() - want).abs().max()))
    assert bool((got[:-1] > got[1:]).all())
    assert float((got.cpu() - want).abs().max()) <= BASE_REWARD_ERR
    n, B, E = 4, len(amps), BASE_REWARD_ERR
    masks = torch.ones(B, n - 1, 3, device=DEV)
    adv, adv_want = ppo.compute_advantages(got, masks, n).cpu(), ppo.compute_advantages(want.to(DEV), masks, n).cpu()
    # adv = 10 c / (std + eps), c = r - mean, std unbiased.  |delta r| <= E  =>  |delta c_i| <= 2 E,  |delta std| <= |delta c|_2 / sqrt(B - 1) <= E sqrt(B / (B - 1));
    # |delta adv_i| <= 10 (|delta c_i| + |z_i| |delta std|) / (std - |delta std|),  z = c / std
    std = float(want.std())
    dstd = E * (B / (B - 1)) ** 0.5
    zmax = float(((want - want.mean()) / std).abs().max())
    bound = 10 * (2 * E + zmax * dstd) / (std - dstd)
    err = float((adv - adv_want).abs().max())
    print(f"advantages: max error {err:.3e}, bound {bound:.3e} (reward std {std:.3f})")
    assert err <= bound, (err, bound)


def test_dispatch_shape_range_identity_and_batch_invariance(base):
    model, proc, sd, orc = base
    pred, target = _base_pairs()
    pred, target = pred[:3].to(DEV), target[:3].to(DEV)
    r = ppo.calculate_reward("dino", model, proc, pred, target, DEV)
    assert r.shape == (3, 1) and r.dtype == torch.float32 and bool(((r >= 0) & (r <= 100)).all())
    same = ppo.calculate_reward("dino", model, proc, pred, pred, DEV)
    assert float((same - 100.0).abs().max()) <= BASE_REWARD_ERR
    for i in range(3):
        one = ppo.calculate_reward("dino", model, proc, pred[i:i + 1], target[i:i + 1], DEV)
        print("row", i, float(r[i, 0]), float(one[0, 0]))
        # the same pair in another batch: the GEMM / attention kernels are chosen by the row count, so not bit-identical by contract; both values are
        # within the reward bound of the exact one, and their difference is rounding noise well inside it
        assert abs(float(one[0, 0]) - float(r[i, 0])) <= BASE_REWARD_ERR, (i, float(one[0, 0]), float(r[i, 0]))
    # one target shared by the batch ([1,3,H,W]) == the expanded batch; fp32 images take the fp32 quantisation path
    shared = calculate_dino_reward(model, proc, pred, target[:1], DEV)
    expanded = ppo.calculate_reward("dino", model, proc, pred, target[:1].expand(3, -1, -1, -1).contiguous(), DEV)
    assert float((shared - expanded).abs().max()) <= BASE_REWARD_ERR
    assert ppo.calculate_reward("dino", model, proc, pred[:0], target[:0], DEV).shape == (0, 1)
    with pytest.raises(TypeError):
        ppo.calculate_reward("dino", None, None, pred, target, DEV)
    with pytest.raises(TypeError):
        ppo.calculate_reward("dino", model, proc, pred.bfloat16(), target.bfloat16(), DEV)        # ToPILImage in bf16 is another quantisation: not built
    with pytest.raises(RuntimeError):
        model.to("cpu")
    assert model.to(DEV) is model and model.eval() is model
    with pytest.raises(ValueError):
        ppo.calculate_reward("dino", model, DinoImageProcessor(crop_size={"height": 196, "width": 196}), pred, target, DEV)
    with pytest.raises(NotImplementedError):
        ppo.calculate_reward("depth", model, proc, pred, target, DEV)


@pytest.mark.parametrize("B,H,N", [(2, 12, 257), (1, 2, 64)])
def test_unmasked_attention_head64(B, H, N):
    g = torch.Generator().manual_seed(N)
    q, k, v = (torch.randn(B, N, H * 64, generator=g).half().to(DEV) for _ in range(3))
    out = torch.empty_like(q)
    L.check(L.lib().cs_op_attention(L.ptr(q), H * 64, L.ptr(k), H * 64, L.ptr(v), H * 64, L.ptr(out), H * 64, B, H, N, N, 64, 0.125, L.stream_ptr(q.device)))
    qf, kf, vf = (t.float().cpu().view(B, N, H, 64).transpose(1, 2) for t in (q, k, v))
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * 0.125, -1) @ vf).transpose(1, 2).reshape(B, N, H * 64)
    assert rel_l2(out.float().cpu().numpy(), ref.numpy()) < 2e-3
    assert float((out.float().cpu() - ref).abs().max()) < 1e-2


def test_train_iteration_with_dino_reward(reduced):
    """train_ppo.py:322-437 with reward_type "dino" on the reduced UNet / VAE of the PPO tests and the reduced encoder (128^2 decoded images: the front end
    upscales to 256): finite loss and gradient norm, reward in range; collect_rollout's rewards are the dispatcher's on the decoded images, and the shared-target form agrees with the expanded batch."""
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
    out = ppo.train_iteration(tr, None, sch, unet, vae, batch, None, cfg=3.0, num_inference_steps=4, ppo_epochs=2, reward_type="dino", prompt_embeds=pe,
                              negative_prompt_embeds=ne, rng=random.Random(0), reward_model=reduced, reward_model_processor=proc)
    assert torch.isfinite(out["loss"]) and torch.isfinite(out["norm"]) and 0.0 <= float(out["reward"]) <= 100.0
    assert tr.step_count == 2
    roll = ppo.collect_rollout(None, sch, unet, vae, batch[1], batch[0], None, batch[2][:1].expand(B, -1, -1, -1).contiguous(), num_inference_steps=3,
                               reward_type="dino", reward_model=reduced, reward_model_processor=proc, prompt_embeds=pe, negative_prompt_embeds=ne,
                               identical_inputs=False)
    assert roll["rewards"].shape == (B, 1) and bool(((roll["rewards"] >= 0) & (roll["rewards"] <= 100)).all()) and bool(torch.isfinite(roll["advantages"]).all())
    # the rollout's reward is the dispatcher's on the images the rollout decoded (same decode batches, same encoder batch: bit-identical)
    tgt = batch[2][:1].expand(B, -1, -1, -1).contiguous()
    pred_img, tgt_img = decode_latents(vae, roll["model_pred"], batch_size=8), decode_latents(vae, tgt, batch_size=8)
    assert torch.equal(calculate_dino_reward(reduced, proc, pred_img, tgt_img, DEV), roll["rewards"])
    # the same target image passed once ([1,3,H,W], encoded once): other encoder batch shapes for the same inputs, so each side is within the reduced
    # model's reward bound of the exact value
    shared = calculate_dino_reward(reduced, proc, pred_img, tgt_img[:1], DEV)
    print("shared target vs expanded batch: max reward difference", float((shared - roll["rewards"]).abs().max()))
    assert float((shared - roll["rewards"]).abs().max()) <= 2 * REDUCED_REWARD_ERR


def test_score_image_pairs_with_dino(tmp_path, reduced):
    from consolver_amd import evaluation as ev
    for i in range(3):
        a = vo.synthetic_image(600 + i, 96, 96)
        b = (a + 0.1 * i * torch.randn(3, 96, 96, generator=torch.Generator().manual_seed(i))).clamp(0, 1)
        ev.save_generation(str(tmp_path / "a"), 0, i, a, "p")
        ev.save_generation(str(tmp_path / "b"), 0, i, b, "p")
    pairs = ev.find_image_pairs(str(tmp_path / "a"), str(tmp_path / "b"))
    res = ev.score_image_pairs(pairs, reward_types=("image_psnr", "dino"), batch_size=2, device=DEV, reward_models={"dino": (reduced, reduced.processor)})
    assert len(res["dino"]) == 3 and abs(res["dino"][0] - 100.0) < 1e-3 and all(0 <= v <= 100 for v in res["dino"])
    with pytest.raises(TypeError):
        ev.score_image_pairs(pairs, reward_types=("dino",), device=DEV)
