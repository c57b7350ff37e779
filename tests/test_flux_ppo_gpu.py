"""GPU tests of the FLUX-Kontext PPO trainer: the baseline-advantage kernel and PolicyTrainer on a FluxFactorNetPPO against the reference's own
results (tests/golden/flux_ppo_update.npz), step 0 of the two schedulers, the shared-prefix rollout, collect_rollout_flux /
train_iteration_flux on reduced networks and the train_flux_ppo driver."""
import os
import random

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import generate_flux as gf
from consolver_amd import generate_flux_teacher as gft
from consolver_amd import ppo, ppo_data, ppo_flux
from consolver_amd.flux import HipFluxTransformer2DModel, pack_latents
from consolver_amd.pipeline import FluxKontextEditPipeline
from consolver_amd.rollout_flux import denoise_diffusion
from consolver_amd.scheduling_fm import FlowMatchGeneralDiscreteScheduler
from consolver_amd.synth import synthetic_flux_state_dict, synthetic_vae_state_dict
from tests import test_flux_ppo_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(num_layers=2, num_single_layers=2, num_heads=4, joint_attention_dim=256)       # the reduced DiT of tests/test_fm_baselines_gpu.py


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(DEV, dtype)


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---------------------------------------------------------------------------------------------------------------- advantage kernel
@pytest.mark.parametrize("B,n,A", [(10, 2, 1), (10, 5, 1), (5, 3, 3), (2, 2, 1), (300, 4, 2)])
def test_baseline_advantages_match_reference(golden, B, n, A):
    """cs_ppo_advantages_baseline against the reference's torch expression (edit_ppo/train_ppo.py:326-341) for every base case; the
    tolerance is the one tests/test_ppo_gpu.py::test_advantages_match_oracle applies to the SD kernel"""
    g = golden["flux_ppo_update"]
    mine = [(ai, bc) for ai, b_, n_, a_, bc in ref.advantage_cases(g) if (int(b_), int(n_), int(a_)) == (B, n, A)]
    assert sorted(bc for _, bc in mine) == sorted(["below", "above", "equal", "hundred", "over_hi", "flat_below", "flat_above", "low_hi"])
    for ai, bc in mine:
        r, masks, base, hi = g[f"a{ai}_rewards"], g[f"a{ai}_masks"], float(g[f"a{ai}_base"]), float(g[f"a{ai}_clip_hi"])
        assert (masks == 0).any() or masks.size < 4
        got = ppo_flux.compute_advantages_flux(cu(r), cu([[base]]), cu(masks).reshape(B, n - 1, A), n, clip_hi=hi)      # base read from the device
        assert got.shape == (B * (n - 1), A) and got.dtype == torch.float32
        np.testing.assert_allclose(got.cpu().numpy(), g[f"a{ai}_out"], rtol=2e-5, atol=2e-5, err_msg=f"case {ai} {bc}")
        np.testing.assert_allclose(got.cpu().numpy(), ref.advantages_restated(r, base, masks, n, hi), rtol=2e-5, atol=2e-5, err_msg=f"case {ai} {bc}")
        again = ppo_flux.compute_advantages_flux(cu(r), base, cu(masks), n, clip_hi=hi)                                  # ... or handed over as a number
        assert torch.equal(got, again)                                                                                  # one workgroup, no atomics


def test_baseline_advantages_single_trajectory_is_nan_like_torch_std(golden):
    g = golden["flux_ppo_update"]
    ai = len(g["a_cases"]) - 1
    assert g["a_cases"][ai].startswith("1,") and np.isnan(g[f"a{ai}_out"]).all()
    got = ppo_flux.compute_advantages_flux(cu(g[f"a{ai}_rewards"]), float(g[f"a{ai}_base"]), cu(g[f"a{ai}_masks"]), int(g[f"a{ai}_n"]))
    assert got.shape == g[f"a{ai}_out"].shape and torch.isnan(got).all()
    with pytest.raises(ValueError):
        ppo_flux.compute_advantages_flux(cu([[1.0], [2.0]]), cu([1.0, 2.0]), cu(np.ones((2, 1))), 2)


# ---------------------------------------------------------------------------------------------------------------- policy update
def test_flux_policy_update_matches_reference_autograd_and_adamw(golden):
    """PolicyTrainer (cs_ppo_policy_grads / cs_clip_grad_norm / cs_adamw_step), unchanged, on a FluxFactorNetPPO (softmax(logits / 0.01), no
    input scale, the mu grid) against the reference's edit_ppo FactorNetPPO under autograd, clip_grad_norm_ and AdamW: two epochs, rows
    whose softmax is saturated next to rows where it is not.  Tolerances: tests/test_ppo_gpu.py's for the SD net."""
    g = golden["flux_ppo_update"]
    for ui in range(3):
        o, sc, mu, K, H, R = [int(v) for v in g[f"u{ui}_cfg"]]
        net = consolver_amd.FluxFactorNetPPO(hidden_dim=H, num_actions=K, order_dim=o, scaler_dim=sc, mu_dim=mu)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in ref.golden_weights(g, ui).items()})
        net.to(DEV)
        lr, b1, b2, wd, eps, clip_range, entropy_coef, max_norm = [float(v) for v in g[f"u{ui}_hyper"]]
        tr = ppo.PolicyTrainer(net, lr=lr, betas=(b1, b2), weight_decay=wd, eps=eps, max_grad_norm=max_norm, clip_range=clip_range,
                               entropy_coef=entropy_coef)
        conds = {"x": cu(g[f"u{ui}_x"], torch.bfloat16)}                   # the dtype the rollout records them in
        actions, old, adv = cu(g[f"u{ui}_actions"]), cu(g[f"u{ui}_old_probs"]), cu(g[f"u{ui}_adv"])
        assert actions.shape == (R, o + sc + mu - 1)
        for ep in range(2):
            loss = float(tr.compute_grads(conds, actions, old, adv))
            want_loss = float(g[f"u{ui}_e{ep}_loss"])
            print(f"case {ui} epoch {ep}: loss {loss:.6f} (reference {want_loss:.6f})")
            assert abs(loss - want_loss) < 5e-5 * max(1.0, abs(want_loss)), (ui, ep, loss, want_loss)
            for k, gv in tr.grad_views().items():
                want = g[f"u{ui}_e{ep}_grad_{k}"]
                err = np.linalg.norm(gv.cpu().numpy() - want) / max(np.linalg.norm(want), 1e-12)
                print(f"  grad {k}: rel-L2 {err:.3e}")
                assert err < 1e-4, (ui, ep, k, err)
            loss2, norm = tr.step(conds, actions, old, adv)
            assert abs(float(loss2) - want_loss) < 5e-5 * max(1.0, abs(want_loss))
            assert abs(float(norm) - float(g[f"u{ui}_e{ep}_norm"])) < 1e-4 * max(1.0, float(norm))
            for k, v in net.state_dict().items():
                want = g[f"u{ui}_e{ep}_after_{k}"]
                assert np.abs(v.cpu().numpy() - want).max() < 3e-6 + 5e-5 * np.abs(want).max(), (ui, ep, k)


# ---------------------------------------------------------------------------------------------------------------- step 0
def policy_scheduler(scaler_dim=0, order_dim=2, hidden=64, seed=11):
    s = gf.make_scheduler("consistencysolver", order_dim=order_dim, scaler_dim=scaler_dim, mu_dim=0,
                          factor_net_kwargs=dict(hidden_dim=hidden, num_actions=11))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in s.factor_net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3 / max(1.0, p.shape[-1] ** 0.5))
        s.factor_net.mlp[4].weight.mul_(0.05)                              # T = 0.01: keep several bins likely, so the rows' actions differ
    s.factor_net.to(DEV)
    return s


@pytest.mark.parametrize("n", [4, 5])
def test_step0_of_policy_and_euler_schedulers_is_bit_identical(golden, n):
    """what sharing forward 1 with the baseline rests on: without a scale action step 0 of FMPPOScheduler takes no action
    (scheduler_fmppo.py:413-414) and is the Euler step, rounded the same way"""
    g = golden["flux_fm_baselines"]
    for x, v in ((cu(g[f"euler_bf16_n{n}_s0_x"], torch.bfloat16), cu(g[f"euler_bf16_n{n}_s0_v"], torch.bfloat16)),
                 (cu(g[f"euler_f32_n{n}_s0_x"]), cu(g[f"euler_bf16_n{n}_s0_v"], torch.bfloat16))):       # an fp32 sample next to bf16 model output
        assert x.shape == (3, 5, 67)
        a = consolver_amd.FMPPOScheduler(shift=3.0, use_dynamic_shifting=True, order_dim=2, scaler_dim=0, mu_dim=0,
                                         factor_net_kwargs=dict(hidden_dim=32, num_actions=11))
        a.factor_net.to(DEV)
        b = FlowMatchGeneralDiscreteScheduler(shift=3.0, use_dynamic_shifting=True, type="euler")
        for s in (a, b):
            s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=1.15, device=DEV)
        pa = a.step(v, a.timesteps[0], x, return_dict=False)[0]
        pb = b.step(v, b.timesteps[0], x, return_dict=False)[0]
        assert pa.dtype == pb.dtype == torch.bfloat16 and torch.equal(pa, pb), float((pa.float() - pb.float()).abs().max())
        assert not torch.equal(pa.float(), x.float())


# ---------------------------------------------------------------------------------------------------------------- rollout
@pytest.fixture(scope="module")
def nets():
    """the reduced DiT (SMALL) and the reduced FLUX VAE (sample_size 16: 128 x 128 images, L = 64 tokens) with seeded weights, and one
    sample's inputs"""
    from consolver_amd.vae import HipAutoencoderKL, FLUX_VAE_CONFIG
    m = HipFluxTransformer2DModel(dict(SMALL, dtype=torch.bfloat16), device=DEV)
    sd = {k: v.to(torch.bfloat16).float() for k, v in synthetic_flux_state_dict(m.manifest(), seed=4).items()}
    m.load_state_dict(sd)
    vcfg = dict(FLUX_VAE_CONFIG); vcfg.update(layers_per_block=1, sample_size=16, with_encoder=True)
    vae = HipAutoencoderKL(vcfg, device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=9))
    g = torch.Generator().manual_seed(7)
    one = dict(noise=torch.randn(1, 16, 16, 16, generator=g).to(torch.bfloat16).to(DEV),
               image=torch.tanh(torch.randn(1, 3, 128, 128, generator=g)).to(DEV),
               pe=torch.randn(1, 64, 256, generator=g).to(torch.bfloat16).to(DEV),
               pooled=torch.randn(1, 768, generator=g).to(torch.bfloat16).to(DEV))
    return dict(m=m, sd=sd, vae=vae, one=one)


def batch_of(one, B):
    rep = lambda t: t.repeat(B, *[1] * (t.dim() - 1))
    return rep(one["noise"]), {"prompt_embeds": rep(one["pe"]), "pooled_prompt_embeds": rep(one["pooled"])}, rep(one["image"])


def expected_rows(B, n, scaler_dim, shared, baseline):
    s = min(2 if scaler_dim == 0 else 1, n) if shared else 0
    own_base = (n - max(s, 1)) if baseline else 0              # the baseline always reuses forward 0, and forward 1 when it is shared
    return s + (n - s) * B + own_base


def oracle_rollout(nets, sch_w, noise, text, image, pipe, n, idx, scaler_dim):
    """the rollout in fp32 on the CPU (FluxOracle inside oracle.solver_oracle.flux_rollout) with replayed action indices"""
    from oracle import solver_oracle as so
    from oracle.flux_oracle import FluxOracle
    B = noise.shape[0]
    packed, il, lat_ids, img_ids = pipe.prepare_latents(image=image, batch_size=B, dtype=torch.bfloat16, device=torch.device(DEV),
                                                        latents=pack_latents(noise))
    ids = torch.cat([lat_ids, img_ids]).float().cpu().numpy()
    txt_ids = np.zeros((text["prompt_embeds"].shape[1], 3), np.float32)
    if "orc" not in nets:
        nets["orc"] = FluxOracle(nets["sd"], nets["m"].config)
    torch.set_num_threads(16)
    pe, pooled = text["prompt_embeds"].float().cpu(), text["pooled_prompt_embeds"].float().cpu()
    v_model = lambda h, ts: nets["orc"](torch.from_numpy(h), torch.from_numpy(ts), torch.full((B,), 2.5), pooled, pe, txt_ids, ids).numpy()
    s_or = so.FMPPOSchedulerOracle(shift=3.0, use_dynamic_shifting=True, order_dim=2, scaler_dim=scaler_dim, mu_dim=0, num_actions=11, weights=sch_w)
    return so.flux_rollout(s_or, v_model, packed.float().cpu().numpy(), il.float().cpu().numpy(), n, idx, io_dtype="bf16")[0]


@pytest.mark.parametrize("n,scaler_dim", [(2, 0), (4, 0), (2, 1), (4, 1)])
def test_rollout_shares_the_identical_prefix(nets, n, scaler_dim):
    """B = 3 copies of one sample, same torch RNG state, identical_inputs off and on: the DiT rows actually run follow the rule, the records
    are equal, and so are the latents (or, where the kernels take another route for one row than for three, both paths are as close to the
    fp32 oracle loop)"""
    B = 3
    sch = policy_scheduler(scaler_dim)
    pipe = FluxKontextEditPipeline(nets["m"], sch, nets["vae"])
    noise, text, image = batch_of(nets["one"], B)
    outs, rows = {}, {}
    for shared in (False, True):
        torch.manual_seed(1234)
        stats = {}
        outs[shared] = denoise_diffusion(sch, pipe, noise, text, image, cfg=2.5, num_inference_steps=n, identical_inputs=shared, decode=False,
                                         stats=stats)
        rows[shared] = stats["forward_rows"]
        assert len(outs[shared]) == 6 and outs[shared][1] is None
    assert rows[False] == [B] * n and sum(rows[False]) == expected_rows(B, n, scaler_dim, False, False)
    s = 2 if scaler_dim == 0 else 1
    assert rows[True] == [1] * s + [B] * (n - s) and sum(rows[True]) == expected_rows(B, n, scaler_dim, True, False)
    (lat_a, _, conds_a, probs_a, act_a, masks_a), (lat_b, _, conds_b, probs_b, act_b, masks_b) = outs[False], outs[True]
    assert lat_b.shape == (B, 64, 64) and conds_b["x"].shape == (B, n - 1, 2) and conds_b["epsilon"].shape == (B, n - 1, 2, 64, 64)
    assert probs_b.shape == act_b.shape == masks_b.shape == (B, n - 1, 1 + scaler_dim)
    assert torch.equal(act_a, act_b) and torch.equal(probs_a, probs_b) and torch.equal(masks_a, masks_b) and torch.equal(conds_a["x"], conds_b["x"])
    if n > 2:
        assert len({tuple(r) for r in act_b.reshape(B, -1).tolist()}) > 1              # the rows did take different actions
    if torch.equal(lat_a, lat_b):
        print(f"n={n} scaler_dim={scaler_dim}: shared and unshared latents are bit-identical")
        return
    # the kernels pick another route for one row than for three: hold both paths to the fp32 oracle loop with replayed indices
    w = {k: v.cpu().numpy().copy() for k, v in sch.factor_net.state_dict().items()}
    idx = np.random.default_rng(3).integers(0, 11, size=(n, B, 1 + scaler_dim))
    err = {}
    for shared in (False, True):
        sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx]
        lat = denoise_diffusion(sch, pipe, noise, text, image, cfg=2.5, num_inference_steps=n, identical_inputs=shared, decode=False)[0]
        if "want" not in err:
            err["want"] = oracle_rollout(nets, w, noise, text, image, pipe, n, idx, scaler_dim)
        err[shared] = rel_l2(lat.float().cpu().numpy(), err["want"])
    sch.factor_net.forced_action_idx = None
    print(f"n={n} scaler_dim={scaler_dim}: rel-L2 vs the fp32 oracle loop: unshared {err[False]:.4e}, shared {err[True]:.4e}")
    assert err[True] <= 1.10 * err[False], (err[True], err[False])


def test_rollout_rejects_rows_that_are_not_copies(nets):
    sch = policy_scheduler(0)
    pipe = FluxKontextEditPipeline(nets["m"], sch, nets["vae"])
    noise, text, image = batch_of(nets["one"], 3)
    bad = noise.clone(); bad[1, 0, 0, 0] += 1.0
    with pytest.raises(ValueError, match="identical_inputs=True, but the rows of noise / prompt embeddings are not copies of one sample"):
        denoise_diffusion(sch, pipe, bad, text, image, num_inference_steps=2, identical_inputs=True, decode=False)
    bad_text = dict(text, pooled_prompt_embeds=text["pooled_prompt_embeds"].clone())
    bad_text["pooled_prompt_embeds"][2, 5] += 1.0
    with pytest.raises(ValueError, match="not copies"):
        denoise_diffusion(sch, pipe, noise, bad_text, image, num_inference_steps=2, identical_inputs=True, decode=False)
    bad_image = image.clone(); bad_image[1, 0, 0, 0] = 0.5
    with pytest.raises(ValueError, match="not copies"):
        denoise_diffusion(sch, pipe, noise, text, bad_image, num_inference_steps=2, identical_inputs=True, decode=False)
    with pytest.raises(ValueError):
        denoise_diffusion(gf.make_scheduler("euler"), pipe, noise, text, image, num_inference_steps=2, use_naive_scheduler=True, identical_inputs=True)


@pytest.mark.parametrize("n,scaler_dim,shared", [(4, 0, True), (2, 0, True), (4, 1, True), (4, 0, False)])
def test_baseline_trajectory_is_the_separate_naive_call(nets, n, scaler_dim, shared):
    """``baseline_scheduler``: latents_base is bit-equal to the reference's second call (use_naive_scheduler=True on one row, edit_ppo/train_ppo.py
    :290-300), the policy trajectories are unchanged, and the forwards it did not need were not run"""
    B = 3
    sch = policy_scheduler(scaler_dim)
    pipe = FluxKontextEditPipeline(nets["m"], sch, nets["vae"])
    noise, text, image = batch_of(nets["one"], B)
    torch.manual_seed(99)
    plain = denoise_diffusion(sch, pipe, noise, text, image, num_inference_steps=n, identical_inputs=shared, decode=False)
    torch.manual_seed(99)
    stats = {}
    out = denoise_diffusion(sch, pipe, noise, text, image, num_inference_steps=n, identical_inputs=shared, decode=False,
                            baseline_scheduler=gf.make_scheduler("euler"), stats=stats)
    assert len(out) == 7 and out[6].shape == (1, 64, 64) and out[6].dtype == torch.bfloat16
    assert torch.equal(out[4], plain[4]) and torch.equal(out[3], plain[3])
    if shared:                                  # (unshared, row 0's image is encoded on its own next to a baseline: other bits than inside the batch)
        assert torch.equal(out[0], plain[0])
    assert sum(stats["forward_rows"]) == expected_rows(B, n, scaler_dim, shared, True), stats["forward_rows"]
    if shared and scaler_dim == 0:
        assert sum(stats["forward_rows"]) == 2 + (n - 2) * (B + 1)
    one_text = {k: v[:1] for k, v in text.items()}
    naive = denoise_diffusion(gf.make_scheduler("euler"), pipe, noise[:1], one_text, image[:1], num_inference_steps=n, use_naive_scheduler=True,
                              decode=False)
    assert len(naive) == 2 and naive[1] is None
    assert torch.equal(out[6], naive[0]), float((out[6].float() - naive[0].float()).abs().max())


def test_decode_switch(nets):
    sch = policy_scheduler(0)
    pipe = FluxKontextEditPipeline(nets["m"], sch, nets["vae"])
    noise, text, image = batch_of(nets["one"], 2)
    torch.manual_seed(5)
    a = denoise_diffusion(sch, pipe, noise, text, image, num_inference_steps=3)
    torch.manual_seed(5)
    b = denoise_diffusion(sch, pipe, noise, text, image, num_inference_steps=3, decode=False)
    assert len(a[1]) == 2 and a[1][0].size == (128, 128) and b[1] is None
    assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])


# ---------------------------------------------------------------------------------------------------------------- trainer body
class DecodeCounter:
    """counts the rows of every VAE decoder call"""

    def __init__(self, vae):
        self.vae, self.rows, self.orig = vae, [], vae.decode_into

    def __enter__(self):
        def counted(lat, out, *a, **k):
            self.rows.append(int(lat.shape[0]))
            return self.orig(lat, out, *a, **k)
        self.vae.decode_into = counted
        return self

    def __exit__(self, *exc):
        del self.vae.decode_into


@pytest.fixture(scope="module")
def pairs(nets, tmp_path_factory):
    """three teacher pairs written by generate_flux_teacher's synthetic path and read back by FluxTeacherPairDataset: a collated batch with
    3-D packed noise, on the GPU, and per-item embeddings"""
    data = tmp_path_factory.mktemp("flux_pairs")
    res = gft.main(["--data", str(data), "--synthetic", "3", "--steps", "2"], transformer=nets["m"], vae=nets["vae"])
    assert res["pairs"] == 3
    ds = ppo_data.FluxTeacherPairDataset(str(data), (128, 128), strict=True)
    image, text, noise, tch, refimg = zip(*[ds[i] for i in range(3)])
    batch = (torch.stack(image).to(DEV), list(text), torch.stack(noise).to(DEV), torch.stack(tch).to(DEV), torch.stack(refimg).to(DEV))
    assert batch[2].shape == batch[3].shape == (3, 64, 64) and batch[2].dtype == torch.bfloat16
    g = torch.Generator().manual_seed(21)
    emb = {"prompt_embeds": torch.randn(3, 64, 256, generator=g).to(torch.bfloat16).to(DEV),
           "pooled_prompt_embeds": torch.randn(3, 768, generator=g).to(torch.bfloat16).to(DEV)}
    return batch, emb


def check_rollout_dict(roll, B, n, A=1):
    R = B * (n - 1)
    assert roll["conds"]["x"].shape == (R, 2) and roll["conds"]["epsilon"].shape == (R, 2, 64, 64)
    assert roll["actions"].shape == roll["probs"].shape == roll["masks"].shape == roll["advantages"].shape == (R, A)
    assert roll["rewards"].shape == (B, 1) and roll["rewards_base"].shape == (1, 1) and roll["rewards_base"].is_cuda
    assert roll["model_pred"].shape == (B, 64, 64) and roll["latents_base"].shape == (1, 64, 64)
    r = roll["rewards"].cpu().numpy().astype(np.float64)
    want = ref.advantages_restated(r, float(roll["rewards_base"]), roll["masks"].cpu().numpy(), n)
    # fp32 against float64 on rewards that lie close together: the kernel's mean and every r - centre carry a rounding error of up to one
    # ulp of |r| (2^-23 |r|), which the division by std magnifies; std itself inherits the same relative error from the r - mean it squares.
    # 2 ulp on the difference + 2 ulp through std, doubled for the summation order: 8 x 2^-23 max|r| / std, next to the kernel test's 2e-5.
    tol = 2e-5 + 8 * 2.0 ** -23 * np.abs(r).max() / max(r.std(ddof=1), 1e-30)
    print(f"advantages: max |r| {np.abs(r).max():.4f}, std {r.std(ddof=1):.3e}, tolerance {tol:.3e}, max error {np.abs(roll['advantages'].cpu().numpy() - want).max():.3e}")
    np.testing.assert_allclose(roll["advantages"].cpu().numpy(), want, rtol=tol, atol=tol)


@pytest.mark.parametrize("identical", [True, False])
def test_collect_rollout_flux_reduced_networks(nets, pairs, identical):
    """edit_ppo/train_ppo.py:285-347 on the reduced networks with image_psnr: field shapes, advantages = the restatement applied to the returned
    rewards and rewards_base, the decoder calls (teacher decoded once when the rows are copies), and the rewards against the decoded latents"""
    batch, emb = pairs
    B, n = 3, 3
    _, text, noise, tch, refimg = ppo_data.repeat_random_sample_flux(batch, index=1)
    text = {k: v[1:2].expand(B, *v.shape[1:]).contiguous() for k, v in emb.items()}
    sch = policy_scheduler(0)
    pipe = FluxKontextEditPipeline(nets["m"], sch, nets["vae"])
    with DecodeCounter(nets["vae"]) as dc:
        roll = ppo_flux.collect_rollout_flux(pipe, sch, gf.make_scheduler("euler"), noise, text, refimg * 2 - 1, tch, num_inference_steps=n,
                                             identical_inputs=identical)
    assert noise.dim() == 3                                                   # the dataset's packed noise went in as it is
    check_rollout_dict(roll, B, n)
    assert dc.rows == ([B, 1, 1] if identical else [B, 1, B]), dc.rows        # prediction, baseline, teacher
    assert sum(roll["forward_rows"]) == expected_rows(B, n, 0, identical, True)
    pred = ppo_flux.decode_latents_flux(pipe, roll["model_pred"])
    # (the decoder's bits depend on the batch it runs in: the check decodes the teacher the way the mode under test does)
    tgt = ppo_flux.decode_latents_flux(pipe, tch[:1], 1).expand(B, -1, -1, -1).contiguous() if identical else ppo_flux.decode_latents_flux(pipe, tch)
    assert pred.shape == (B, 3, 128, 128) and float(pred.min()) >= 0 and float(pred.max()) <= 1
    assert torch.equal(roll["rewards"], ppo.calculate_reward("image_psnr", None, None, pred, tgt))
    base_img = ppo_flux.decode_latents_flux(pipe, roll["latents_base"])
    assert torch.equal(roll["rewards_base"], ppo.calculate_reward("image_psnr", None, None, base_img, tgt[:1]))
    # the student starts from the reference's permutation of the stored noise, or (noise_layout="packed") from the teacher's own latents
    same = ppo_flux.collect_rollout_flux(pipe, sch, gf.make_scheduler("euler"), noise, text, refimg * 2 - 1, tch, num_inference_steps=2,
                                         identical_inputs=identical, noise_layout="packed")
    own = ppo_flux.collect_rollout_flux(pipe, sch, gf.make_scheduler("euler"), pack_latents(ppo_flux.as_rollout_noise(noise, 16, 16)), text,
                                        refimg * 2 - 1, tch, num_inference_steps=2, identical_inputs=identical, noise_layout="packed")
    assert not torch.equal(same["latents_base"], own["latents_base"])


def test_collect_rollout_flux_with_dino_reward(nets, pairs, golden):
    from consolver_amd.reward_model import HipDinov2Model
    from consolver_amd.synth import synthetic_dinov2_state_dict
    from tests.test_dino_reward_gpu import REDUCED
    dino = HipDinov2Model(REDUCED, device=DEV)
    dino.load_state_dict(synthetic_dinov2_state_dict(dino.manifest(), seed=int(golden["dino_reward"]["weight_seed"])))
    batch, emb = pairs
    B, n = 3, 4
    _, text, noise, tch, refimg = ppo_data.repeat_random_sample_flux(batch, index=0)
    text = {k: v[0:1].expand(B, *v.shape[1:]).contiguous() for k, v in emb.items()}
    sch = policy_scheduler(0)
    pipe = FluxKontextEditPipeline(nets["m"], sch, nets["vae"])
    with DecodeCounter(nets["vae"]) as dc:
        roll = ppo_flux.collect_rollout_flux(pipe, sch, gf.make_scheduler("euler"), noise, text, refimg * 2 - 1, tch, num_inference_steps=n,
                                             reward_type="dino", reward_model=dino, reward_model_processor=dino.processor, identical_inputs=True)
    check_rollout_dict(roll, B, n)
    assert dc.rows == [B, 1, 1] and float(roll["rewards"].min()) >= 0 and float(roll["rewards"].max()) <= 100
    assert sum(roll["forward_rows"]) == 2 + (n - 2) * (B + 1)


def test_train_iteration_flux_on_a_dataset_batch(nets, pairs):
    """edit_ppo/train_ppo.py:258-389 in one call, fed what FluxTeacherPairDataset collates (3-D packed noise): parameters move, the loss is finite.
    The same batch handed to rollout_flux.denoise_diffusion unconverted does not run: its pack wants [B, 16, S, S]."""
    batch, emb = pairs
    sch = policy_scheduler(0, hidden=32)
    pipe = FluxKontextEditPipeline(nets["m"], sch, nets["vae"])
    before = [p.detach().clone() for p in sch.factor_net.parameters()]
    tr = ppo.PolicyTrainer(sch.factor_net, lr=1e-3)
    torch.manual_seed(3)
    random.seed(3)
    out = ppo_flux.train_iteration_flux(tr, pipe, sch, gf.make_scheduler("euler"), batch, ppo_epochs=2, text_embeds=emb, rng=random.Random(0))
    n = out["num_inference_steps"]
    assert 2 <= n <= 5 and tr.step_count == 2 and 0 <= out["index"] < 3
    assert torch.isfinite(out["loss"]) and torch.isfinite(out["norm"]) and torch.isfinite(out["reward"]) and torch.isfinite(out["reward_base"])
    assert out["reward_base"].is_cuda and out["reward_base"].dim() == 0
    assert sum(out["forward_rows"]) == 2 + (n - 2) * 4
    check_rollout_dict(out["rollout"], 3, n)
    out3 = ppo_flux.train_iteration_flux(tr, pipe, sch, gf.make_scheduler("euler"), batch, ppo_epochs=1, text_embeds=emb, num_inference_steps=3,
                                         share_identical=False)
    assert out3["num_inference_steps"] == 3 and sum(out3["forward_rows"]) == 3 * 3 + 2 and tr.step_count == 3
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, sch.factor_net.parameters()))
    _, _, noise, _, refimg = ppo_data.repeat_random_sample_flux(batch, index=0)
    text = {k: v[:1].expand(3, *v.shape[1:]).contiguous() for k, v in emb.items()}
    with pytest.raises((ValueError, RuntimeError)):
        denoise_diffusion(sch, pipe, noise, text, refimg * 2 - 1, num_inference_steps=2)


# ---------------------------------------------------------------------------------------------------------------- driver
def test_train_flux_ppo_driver_runs_and_resumes(nets, tmp_path, capsys):
    import json
    from consolver_amd import train_flux_ppo as drv
    out_dir = tmp_path / "out"
    common = ["--synthetic", "2", "--output_dir", str(out_dir), "--train_batch_size", "3", "--ppo_epochs", "2", "--teacher_steps", "2",
              "--factor_hidden_dim", "32", "--checkpointing_steps", "1", "--learning_rate", "1e-3", "--seed", "5"]
    res = drv.main(common + ["--max_train_steps", "2", "--save_samples"], transformer=nets["m"], vae=nets["vae"])
    assert res["first_step"] == 0 and res["global_step"] == 2 and len(res["logs"]) == 2
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines] == [1, 2]
    for l in lines:
        assert set(l) >= {"loss", "norm", "reward", "reward_base", "n"} and 2 <= l["n"] <= 5 and all(np.isfinite(l[k]) for k in ("loss", "norm", "reward", "reward_base"))
    assert sorted(d for d in os.listdir(out_dir) if d.startswith("checkpoint-")) == ["checkpoint-1", "checkpoint-2"]
    names = os.listdir(out_dir / "samples")
    for step, n in ((1, lines[0]["n"]), (2, lines[1]["n"])):
        assert sum(f.startswith(f"{step}_0_") and f.endswith(f"_{n}step.jpg") for f in names) == 3
        assert f"target_{step}_0_2.jpg" in names and f"conds_{step}_0_2.txt" in names
    # the checkpoint is the reference's format and holds the trainer's parameters
    net = consolver_amd.FluxFactorNetPPO(hidden_dim=32, num_actions=11, order_dim=2, scaler_dim=0, mu_dim=0).to(DEV)
    ppo.PolicyTrainer(net).load_checkpoint(str(out_dir / "checkpoint-2"))
    for k, v in net.state_dict().items():
        assert torch.equal(v, res["trainer"].net.state_dict()[k]), k
    # resume from "latest": one more step, starting from step 2's parameters
    res2 = drv.main(common + ["--max_train_steps", "3", "--resume_from_checkpoint", "latest"], transformer=nets["m"], vae=nets["vae"])
    assert res2["first_step"] == 2 and res2["global_step"] == 3 and len(res2["logs"]) == 1 and res2["logs"][0]["step"] == 3
    assert os.path.isfile(out_dir / "checkpoint-3" / "model.ckpt")
    assert any(not torch.equal(v, res2["trainer"].net.state_dict()[k]) for k, v in net.state_dict().items() if k != "action_values")
    with pytest.raises(SystemExit):
        drv.main(["--output_dir", str(out_dir)], transformer=nets["m"], vae=nets["vae"])
