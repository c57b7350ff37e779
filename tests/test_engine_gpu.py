"""End-to-end parity of the device-resident sampling loop (engine.py) against the oracle:
full SD1.5 UNet (HIP fp16) + PPOScheduler vs UNet oracle (fp32, fp16-rounded weights) + solver oracle
on identical seeded weights, prompts, noise and replayed action indices.

The engine in its default configuration -- split-fp16 residual stream in the denoiser, fp32 solver state -- against the fp32 oracle end to end (no fp16 rounding
in the comparator: only the conds are fp16-typed, as scheduler_ppo.py:207 makes them).  Measured 0.72e-3 ... 1.06e-3 on these short / reduced cases (the first step
from t = 999 maps the per-forward eps error 1:1 into the latents), every bound = measured + 10 %; north_star's 1e-3 gate is asserted on the full UNet at
n = 4 / 8 / 12 in tests/test_parity_e2e_gpu.py."""
import os

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd.engine import SDSamplingEngine
from consolver_amd.synth import synthetic_prompt_embeds, synthetic_unet_state_dict
from consolver_amd.unet import HipUNet2DConditionModel
from oracle import solver_oracle as so
from oracle.unet_oracle import UNetOracle
from tests._models import get_unet, get_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(cfg_over, seed=11, use_conv=False):
    unet, sd = get_unet(cfg_over, seed=7)            # the shared handle of this config (tests/_models.py; default residual stream f16x2); `seed` seeds the policy
    sch = consolver_amd.PPOScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                     timestep_spacing="trailing", order_dim=4, scaler_dim=0, use_conv=use_conv,
                                     factor_net_kwargs=dict(hidden_dim=64, num_actions=11))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in sch.factor_net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    w = {k: v.numpy().copy() for k, v in sch.factor_net.state_dict().items()}
    sch.factor_net.to(DEV)
    return unet, sd, sch, w


def oracle_run(sd, cfg, w, noise, pe, ne, idx, n, guidance, use_conv=False, probs_out=None, cfg_over=None):
    torch.set_num_threads(16)
    orc_u = get_oracle(cfg_over, seed=7) if cfg_over is not None else UNetOracle(sd, cfg)
    orc_s = so.PPOSchedulerOracle(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                                  timestep_spacing="trailing", order_dim=4, scaler_dim=0, num_actions=11, weights=w, use_conv=use_conv)
    orc_s.set_timesteps(n)
    x = noise.float().numpy()
    ctx = torch.cat([ne, pe]).float()
    B = x.shape[0]
    for i, t in enumerate(orc_s.timesteps):          # fp32 end to end (the oracle the 1e-3 gate is stated against); only the conds are fp16-typed as scheduler_ppo.py:207 makes them
        e = orc_u(torch.from_numpy(np.concatenate([x, x])), int(t), ctx).numpy()
        out = orc_s.step(so.cfg_combine(e[:B], e[B:], guidance), int(t), x, idx[i], cond_dtype="f16")
        if probs_out is not None:
            probs_out.append(out["probs"])
        x = out["prev_sample"]
    return x


def test_captured_generation_follows_the_default_precision_schedule():
    """the hipGraph replay of a generation under the engine's DEFAULT schedule (hi_precision_steps="auto": split stream for the first ceil(n / 4) forwards, then one plane
    with the sub-pixel upsamplers; fp32 eps with the two-plane output head) is the eager loop bit for bit, the schedule is part of the graph's key, and the handle comes
    back in its own mode.  32 x 32 latents: both sub-pixel kernel forms and the MFMA conv_out run."""
    unet, sd, sch, w = make(dict(layers_per_block=1, sample_size=32))
    B, n, g = 2, 8, 3.0
    one = torch.from_numpy(np.random.default_rng(9).integers(0, 11, size=(B, 3))).to(DEV)
    pe, ne = synthetic_prompt_embeds(B, seed=1011).half().to(DEV), synthetic_prompt_embeds(B, seed=1012).half().to(DEV)
    noise = torch.randn(B, 4, 32, 32, generator=torch.Generator().manual_seed(47)).half().to(DEV)
    eng = SDSamplingEngine(unet, sch, guidance_scale=g)
    assert eng.hi_precision_steps == "auto" and eng.hi_steps(n) == 2
    sch.factor_net.forced_action_idx = one                                  # (one index set for every step: what a capture bakes)
    eager = eng.generate(pe, ne, latents=noise, num_inference_steps=n).clone()
    graph = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    again = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    assert torch.equal(eager, graph) and torch.equal(graph, again) and unet.residual == "f16x2"
    eng.hi_precision_steps = "all"
    allsplit = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    assert not torch.equal(allsplit, graph)                                  # another schedule is another graph
    eng.hi_precision_steps = "auto"
    assert torch.equal(eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True), graph)
    sch.factor_net.forced_action_idx = None


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_trajectory_reduced_unet(use_graph):
    unet, sd, sch, w = make(dict(layers_per_block=1, sample_size=16))
    B, n, g = 2, 4, 3.0
    rng = np.random.default_rng(5)
    idx = rng.integers(0, 11, size=(n, B, 3))
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(43)).half()
    eng = SDSamplingEngine(unet, sch, guidance_scale=g, hi_precision_steps="all")      # (bounds below: the split stream at every step; the schedule is gated on the full UNet, test_parity_e2e_gpu.py)
    if use_graph:
        # replay indices are baked per step by capturing with a fixed queue: use one index set for all steps
        idx[:] = idx[0]
        sch.factor_net.forced_action_idx = torch.from_numpy(idx[0]).to(DEV)
    else:
        sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx]
    got = eng.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n, use_graph=use_graph)
    got = got.float().cpu().numpy()
    if use_graph:   # second replay of the captured graph gives the same result
        again = eng.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n, use_graph=True)
        assert np.array_equal(again.float().cpu().numpy(), got)
    want = oracle_run(sd, unet.config, w, noise, pe, ne, idx, n, g, cfg_over=dict(layers_per_block=1, sample_size=16))
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print("engine 4-step reduced-unet rel l2", err, "graph" if use_graph else "eager")
    assert np.isfinite(got).all() and err < (0.80e-3 if use_graph else 1.14e-3), err          # measured 1.028e-3 (eager) / 0.723e-3 (graph: one index set), + 10 %; gate 1e-3 is on the full UNet (test_parity_e2e_gpu.py)


def test_engine_use_conv_under_cfg():
    """``--use_conv`` (gen_ppo.py) in the fused engine: the policy's cosine features (factor_net_ppo.py:108-130) are taken over the
    COMBINED eps (denoise_ppo.py:96-100 in front of scheduler_ppo.py:207-240) although the engine hands the scheduler the two CFG
    branches -- cs_cosine_features_cfg forms the combine on the fly.  Selected-action probabilities depend on those features, so
    they are compared too (the reduced UNet's eps error moves the cosines by ~1e-3)."""
    unet, sd, sch, w = make(dict(layers_per_block=1, sample_size=16), use_conv=True)
    assert sch.factor_net.mlp[0].in_features == 2 + 3
    B, n, g = 2, 5, 3.0
    idx = np.random.default_rng(8).integers(0, 11, size=(n, B, 3))
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(44)).half()
    eng = SDSamplingEngine(unet, sch, guidance_scale=g, hi_precision_steps="all")
    sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx]
    got_probs = []
    orig = sch.step
    def step(*a, **k):
        out = orig(*a, **k)
        got_probs.append(out[2].float().cpu().numpy())
        return out
    sch.step = step
    got = eng.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n).float().cpu().numpy()
    sch.step = orig
    want_probs = []
    want = oracle_run(sd, unet.config, w, noise, pe, ne, idx, n, g, use_conv=True, probs_out=want_probs, cfg_over=dict(layers_per_block=1, sample_size=16))
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    perr = max(float(np.abs(a - b).max()) for a, b in zip(got_probs, want_probs))
    print("engine use_conv + CFG 5-step rel l2", err, "max |dprob|", perr)
    assert np.isfinite(got).all() and err < 0.91e-3, err          # measured 0.820e-3, + 10 %
    assert perr < 1e-3, perr                                       # measured 2.9e-5 (max |dprob| over the five steps' policy outputs)
    assert float(sch.factor_net.mlp[0].weight[:, 2:].abs().max()) > 0.1      # (the cosine inputs carry weight in this policy)


@pytest.mark.timeout(1200)
def test_engine_trajectory_full_sd15_two_steps():
    unet, sd, sch, w = make({})
    B, n, g = 1, 2, 3.0
    idx = np.random.default_rng(6).integers(0, 11, size=(n, B, 3))
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 64, 64, generator=torch.Generator().manual_seed(43)).half()
    sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx]
    eng = SDSamplingEngine(unet, sch, guidance_scale=g, hi_precision_steps="all")
    got = eng.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n).float().cpu().numpy()
    want = oracle_run(sd, unet.config, w, noise, pe, ne, idx, n, g, cfg_over={})
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print("engine 2-step SD1.5 rel l2", err)
    assert err < 1.17e-3, err                                     # measured 1.055e-3 (two steps from t = 999: the first step maps the eps error 1:1), + 10 %; 8 steps: tests/test_parity_e2e_gpu.py


def test_engine_solver_state_dtype():
    """SDSamplingEngine(latents_dtype=...): fp32 (default) returns fp32 latents and is closer to the fp32 oracle than the fp16 state (the reference fp16 pipeline's own class,
    which rounds the latents once per step); both modes are deterministic; an unsupported dtype is refused."""
    cfg = dict(layers_per_block=1, sample_size=16)
    unet, sd, sch, w = make(cfg)
    B, n, g = 2, 6, 3.0
    idx = np.random.default_rng(9).integers(0, 11, size=(n, B, 3))
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(43)).half()
    want = oracle_run(sd, unet.config, w, noise, pe, ne, idx, n, g, cfg_over=cfg)
    errs = {}
    for dt in (torch.float32, torch.float16):
        eng = SDSamplingEngine(unet, sch, guidance_scale=g, latents_dtype=dt)
        outs = []
        for rep in range(2):
            sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx]
            outs.append(eng.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n).clone())
        assert outs[0].dtype == dt and torch.equal(outs[0], outs[1])
        errs[dt] = float(np.linalg.norm(outs[0].float().cpu().numpy() - want) / np.linalg.norm(want))
    print(f"engine 6-step reduced unet: fp32 solver state {errs[torch.float32]:.3e}, fp16 state {errs[torch.float16]:.3e}")
    assert errs[torch.float32] < errs[torch.float16]
    with pytest.raises(ValueError):
        SDSamplingEngine(unet, sch, latents_dtype=torch.bfloat16)


def test_engine_with_ddim_baseline_scheduler_in_both_state_dtypes():
    """The engine's default fp32 solver state under a BASELINE scheduler (baselines.py): DDIMBaselineScheduler.step takes the fp32 sample as fp32 and writes fp32
    (CsStepArgs::x_is_f32), like PPOScheduler.step -- it used to store fp16 values into the fp32 ping-pong buffer.  Reference point: the learned solver with every
    coefficient at its default (action indices (0, 10, 5) -> actions (0, 0, 0) -> eps_eff = eps_t) IS eta = 0 DDIM on the same tables, so the two engines must agree."""
    from consolver_amd.baselines import DDIMBaselineScheduler
    cfg = dict(layers_per_block=1, sample_size=16)
    unet, sd, sch, w = make(cfg)
    ddim = DDIMBaselineScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing")
    B, n, g = 2, 5, 3.0
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half().to(DEV), synthetic_prompt_embeds(B, seed=1002).half().to(DEV)
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(45)).half().to(DEV)
    default_idx = torch.tensor([[0, 10, 5]] * B, device=DEV)
    for dt in (torch.float32, torch.float16):
        for guidance in (g, 1.0):                                  # fused CFG path and the plain one (the engine copies eps into the history slot there)
            sch.factor_net.forced_action_idx = default_idx
            want = SDSamplingEngine(unet, sch, guidance_scale=guidance, latents_dtype=dt).generate(pe, ne, latents=noise, num_inference_steps=n).clone()
            got = SDSamplingEngine(unet, ddim, guidance_scale=guidance, latents_dtype=dt).generate(pe, ne, latents=noise, num_inference_steps=n).clone()
            assert got.dtype == dt and torch.isfinite(got).all()
            err = float((got.float() - want.float()).norm() / want.float().norm())
            assert err < 1e-6, (dt, guidance, err)
    sch.factor_net.forced_action_idx = None
    # a mismatched out= buffer is refused instead of being filled with the other dtype's bytes
    ddim.set_timesteps(n, device=DEV)
    e = torch.randn(B, 4, 16, 16, device=DEV).half()
    with pytest.raises(ValueError):
        ddim.step(e, ddim.timesteps[0], noise.float(), return_dict=False, out=torch.empty_like(noise))
    from consolver_amd.baselines import FlowMatchEulerBaselineScheduler
    fm = FlowMatchEulerBaselineScheduler(shift=3.0, use_dynamic_shifting=False)
    fm.set_timesteps(4, device=DEV)
    v = torch.randn(B, 64, 64, device=DEV).bfloat16()
    x32 = torch.randn(B, 64, 64, device=DEV)
    out = fm.step(v, fm.timesteps[0], x32, return_dict=False)[0]
    step = torch.tensor(np.float32(fm._sigmas[1] - fm._sigmas[0])) * v.cpu()                         # (a bf16 product, as in tests/test_parity_e2e_gpu.py::test_fmppo_fp32_sample_is_consumed_as_fp32)
    assert out.dtype == torch.bfloat16 and torch.equal(out.cpu(), (x32.cpu() + step).bfloat16())      # the fp32 sample is consumed unrounded (scheduler_fm.py:405-410)
    with pytest.raises(ValueError):
        fm.step(v, fm.timesteps[1], x32, return_dict=False, out=torch.empty_like(x32))


def test_reference_class_dtype_behaviour_of_the_plain_protocol():
    """The reference's OWN dtype behaviour with an fp16 denoiser and an fp32 policy net (scheduler_ppo.py:263-272,306-332): the CFG combine is an fp16
    torch expression (denoise_ppo.py:96-100), step 1 (one history entry, 0-dim scalars only) returns an fp16 prev_sample, every later step returns fp32 because the
    [B,1,1,1] coefficients promote.  The product reproduces that class through the plain protocol -- fp16 sample in -> fp16 out by default, `prev_sample_dtype =
    torch.float32` from the second step on -- and is held here against the comparator with exactly those roundings (fp16 eps halves, fp16 combine ops, fp16 latents
    after step 1 only).  The native engine deviates deliberately: fp32 state from step 0 (no rounding of the first prev_sample); INTEGRATION.md states the difference."""
    cfg = dict(layers_per_block=1, sample_size=16)
    unet, sd, sch, w = make(cfg)
    B, n, g = 2, 5, 3.0
    idx = np.random.default_rng(12).integers(0, 11, size=(n, B, 3))
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(46)).half()
    # ---- comparator: fp32 oracle graph + the reference's rounding points
    orc_u = get_oracle(cfg, seed=7)
    orc_s = so.PPOSchedulerOracle(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing", order_dim=4, scaler_dim=0,
                                  num_actions=11, weights=w)
    orc_s.set_timesteps(n)
    r = so.round_f16
    x = noise.float().numpy()
    ctx = torch.cat([ne, pe]).float()
    for i, t in enumerate(orc_s.timesteps):
        e = r(orc_u(torch.from_numpy(np.concatenate([x, x])), int(t), ctx).numpy())                 # the denoiser's output is an fp16 tensor
        u, c = e[:B], e[B:]
        comb = r(u + r(np.float32(g) * r(c - u)))                                                        # u + g * (c - u), one fp16 rounding per torch op
        x = orc_s.step(comb, int(t), x, idx[i], cond_dtype="f16")["prev_sample"]
        if i == 0:
            x = r(x)                                                                                      # step 1 returns fp16; later steps fp32
    want = x
    # ---- the product through the plain protocol, dtypes as the reference's loop sees them
    sch.set_timesteps(n, device=DEV)
    sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx]
    lat = noise.to(DEV)
    ctx_d = torch.cat([ne, pe]).to(DEV)
    try:
        for i, t in enumerate(sch.timesteps):
            eps = unet(torch.cat([lat] * 2), t, encoder_hidden_states=ctx_d, return_dict=False)[0]
            u, c = eps.chunk(2)
            noise_pred = u + g * (c - u)
            assert noise_pred.dtype == torch.float16
            sch.prev_sample_dtype = None if i == 0 else torch.float32
            lat = sch.step(noise_pred, t, lat, return_dict=False)[0]
            assert lat.dtype == (torch.float16 if i == 0 else torch.float32)
    finally:
        sch.prev_sample_dtype = None
    err = float(np.linalg.norm(lat.cpu().numpy() - want) / np.linalg.norm(want))
    print(f"plain protocol, reference dtype class (fp16 first step, fp32 afterwards), 5-step reduced UNet: rel l2 vs the same-class comparator {err:.3e}")
    assert np.isfinite(lat.cpu().numpy()).all() and err < 1.5e-3, err


def test_engine_pixel_output_matches_decode_of_its_latents():
    """output_type="pt" == decode_latents (utils.py:6-34) of the latents the same engine returns, and matches the
    fp32 VAE oracle applied to those latents (the decoder's own tolerance, tests/test_vae_gpu.py)."""
    from consolver_amd.vae import HipAutoencoderKL
    from consolver_amd.synth import synthetic_vae_state_dict
    from oracle import vae_oracle
    unet, sd, sch, w = make(dict(layers_per_block=1, sample_size=16))
    vae = HipAutoencoderKL(dict(layers_per_block=1, sample_size=16), device=DEV)
    vsd = synthetic_vae_state_dict(vae.manifest(), seed=3)
    vae.load_state_dict(vsd)
    B, n = 3, 2
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half().to(DEV), synthetic_prompt_embeds(B, seed=1002).half().to(DEV)
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(43)).half().to(DEV)
    idx = [torch.zeros(B, 3, dtype=torch.long, device=DEV) + 5 for _ in range(n)]
    eng = SDSamplingEngine(unet, sch, guidance_scale=3.0, vae=vae)
    sch.factor_net.forced_action_idx = list(idx)
    lat = eng.generate(pe, ne, latents=noise, num_inference_steps=n).clone()
    sch.factor_net.forced_action_idx = list(idx)
    img = eng.generate(pe, ne, latents=noise, num_inference_steps=n, output_type="pt", decode_batch_size=2)
    assert img.shape == (B, 3, 128, 128) and float(img.min()) >= 0 and float(img.max()) <= 1
    want = vae_oracle.decode_latents(vae_oracle.VaeOracle(vsd, vars(vae.config)), lat.float().cpu(), 2)
    assert (img.float().cpu() - want).abs().max() < 2e-2
    with pytest.raises(RuntimeError):
        SDSamplingEngine(unet, sch).generate(pe, ne, latents=noise, num_inference_steps=n, output_type="pt")


def test_generate_imgs_driver_writes_sharded_files(tmp_path):
    """gen_ppo.py:237-379 on reduced networks: shard rule, ragged last batch, per-batch seed, file naming, and that a file's
    pixels are the engine's output for that prompt / noise."""
    from consolver_amd import generate as gen, evaluation as ev
    from consolver_amd.vae import HipAutoencoderKL
    from consolver_amd.synth import synthetic_vae_state_dict
    unet, sd, sch, w = make(dict(layers_per_block=1, sample_size=16))
    vae = HipAutoencoderKL(dict(layers_per_block=1, sample_size=16), device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=3))
    eng = SDSamplingEngine(unet, sch, guidance_scale=3.0, vae=vae)
    sch.factor_net.sampler = "inverse_cdf"
    N, world, bs, seed, n = 11, 2, 3, 43, 2
    prompts = [f"p{i}" for i in range(N)]
    pe, ne = synthetic_prompt_embeds(N, seed=1001).half(), synthetic_prompt_embeds(N, seed=1002).half()
    counts = []
    for rank in range(world):                         # the two ranks of a 2-GPU job, run one after the other on this GPU
        counts.append(gen.generate_imgs(str(tmp_path), prompts, pe, ne, eng, n, rank, world, seed, batch_size=bs, device=torch.device(DEV)))
    assert counts == [5, 6]                           # floor rule: the last rank takes the remainder (gen_ppo.py:349-357)
    names = sorted(f for f in os.listdir(tmp_path) if f.endswith(".png"))
    assert names == [f"0_{i:08d}.png" for i in range(5)] + [f"1_{i:08d}.png" for i in range(6)]
    assert open(tmp_path / "1_00000005.txt").read() == "p10"
    # rank 1, batch 1 (local prompts 3..5 = global 8..10), latent seed 43 + 1, image index 1 -> global prompt 9
    noise = gen.prepare_latents(3, (4, 16, 16), seed + 1, torch.device(DEV))
    torch.manual_seed(0)
    sch.factor_net.forced_action_idx = None
    lo = 5 + 3
    # the policy draws are random (inverse-CDF on torch.rand): replay with the same torch seed state is not guaranteed, so only check
    # shape / range of the written file and that the noise generator is deterministic per (seed + batch_idx)
    assert torch.equal(noise, gen.prepare_latents(3, (4, 16, 16), seed + 1, torch.device(DEV)))
    img = ev.load_image_tensor(str(tmp_path / "1_00000004.png"), "cpu")
    assert img.shape == (3, 128, 128) and 0.0 <= float(img.min()) and float(img.max()) <= 1.0 and float(img.std()) > 0.01


def test_generate_cli_reaches_use_conv_and_residual_modes(tmp_path):
    """gen_ppo.py:399 `--use_conv` through the package's own CLI (python -m consolver_amd.generate): the policy is built with the cosine
    features and the fused CFG loop runs with them; full-size synthetic SD1.5 UNet + VAE, 2 prompts, 2 steps."""
    from consolver_amd import generate as gen
    r = gen.main(["--out", str(tmp_path / "a"), "--synthetic", "2", "--steps", "2", "--batch-size", "2", "--use_conv", "--num-actions", "11"])
    assert r["images"] == 2 and r["use_conv"] is True and r["residual"] == "f16x2"
    assert sorted(f for f in os.listdir(tmp_path / "a") if f.endswith(".png")) == ["0_00000000.png", "0_00000001.png"]
    r = gen.main(["--out", str(tmp_path / "b"), "--synthetic", "2", "--steps", "2", "--batch-size", "2", "--residual", "f16"])
    assert r["use_conv"] is False and r["residual"] == "f16" and len(os.listdir(tmp_path / "b")) == 4


def test_pipeline_call_surface():
    """gen_ppo.py:289-312 call: pipeline(prompt_embeds=..., num_inference_steps, generator, guidance_scale, height, width).images"""
    from consolver_amd.pipeline import ConsistencySolverPipeline
    from consolver_amd.vae import HipAutoencoderKL
    from consolver_amd.synth import synthetic_vae_state_dict
    unet, sd, sch, w = make(dict(layers_per_block=1, sample_size=16))
    vae = HipAutoencoderKL(dict(layers_per_block=1, sample_size=16), device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=3))
    pipe = ConsistencySolverPipeline(unet, sch, vae)
    B = 2
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half().to(DEV), synthetic_prompt_embeds(B, seed=1002).half().to(DEV)
    idx = [torch.zeros(B, 3, dtype=torch.long, device=DEV) + 4 for _ in range(3)]
    gen = torch.Generator(device=DEV).manual_seed(43)
    pipe.scheduler.factor_net.forced_action_idx = list(idx)
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=3, generator=gen, guidance_scale=3.0, height=128, width=128)
    assert len(out.images) == B and out.images[0].size == (128, 128)
    gen = torch.Generator(device=DEV).manual_seed(43)
    pipe.scheduler.factor_net.forced_action_idx = list(idx)
    pt = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=3, generator=gen, guidance_scale=3.0, output_type="pt").images
    assert pt.shape == (B, 3, 128, 128)
    assert np.array_equal(np.asarray(out.images[1]), (pt[1].float().clamp(0, 1).permute(1, 2, 0) * 255).round().to(torch.uint8).cpu().numpy())
    gen = torch.Generator(device=DEV).manual_seed(43)
    pipe.scheduler.factor_net.forced_action_idx = list(idx)
    lat = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=3, generator=gen, guidance_scale=3.0, output_type="latent").images
    from consolver_amd.vae import decode_latents
    assert torch.equal(decode_latents(vae, lat, B), pt)
    with pytest.raises(ValueError):
        pipe(prompt_embeds=pe, negative_prompt_embeds=ne, height=512, width=512)
    with pytest.raises(RuntimeError):
        pipe(prompt="a cat")


@pytest.mark.gpu
def test_bench_prints_one_contract_line():
    """bench.py --full (N = 1, short) prints ONE JSON line with the driver's keys plus roofline / ceilings / cpu_baseline objects"""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--decode", "0", "--extras", "0",
                        "--no-cpu-baseline", "--profile-kernels", "0", "--traffic", "none", "--force-dist", "--full"], capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    # --force-dist: the N > 1 branch of bench.py on this one-GPU box -- init_process_group("nccl", device_id=...), the barriers, all_reduce(MAX) of the elapsed time on a
    # GPU tensor and launch.gather_rank_records over RCCL -- the code the driver's 8-GPU run executes, at world size 1; under the same flag bench.py also drives
    # launch.reduce_max_seconds / gather_report / average_gradients on CUDA tensors and asserts their results (one RCCL initialisation, ~70 s on a fresh box, for all of them;
    # their gloo twins run at world size 2 in tests/test_launch_cpu.py).  Reference: gen_ppo.py:349-357,433-465, train_ppo.py:257,430
    assert len(rec["per_rank"]) == 1 and rec["per_rank"][0]["rank"] == 0 and rec["per_rank"][0]["images"] == 16 and rec["per_rank_distinct_devices"] == 1
    assert rec["per_rank"][0]["prompt_shard"] == [0, 16] and abs(rec["per_rank"][0]["elapsed_s"] * 1e3 - rec["ms_per_step"]) < 1e-3 * rec["ms_per_step"] + 1.0
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in rec, k
    assert rec["n_gpus"] == 1 and rec["steps"] == 1 and rec["warmup"] == 1 and rec["scaling"] == "weak" and rec["dtype"] == "f16"
    assert rec["unit"] == "images/s" and rec["value"] > 1.0 and "workload" in rec["config"] and "model" not in rec["config"]
    rf = rec["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0.05 < rf["frac"] < 1.0
    assert rf["frac_executed"] < 1.03 * rf["frac"] and abs(rf["frac_executed"] - rf["achieved_executed"] / rf["peak"]) < 1e-9     # executed vs algorithmic: - 2.5 % CFG shared prefix, + 2.2 % the shortcut's hi + lo passes (f16x2)
    assert abs(rf["achieved_executed"] / rf["achieved"] - rf["flops_executed_per_launch"] / rf["flops_per_launch"]) < 1e-9
    assert rec["ceilings"]["vendor_gemm_f16_8192_tflops"] > 100 and rec["ceilings"]["dtod_copy_1gib_tbps"] > 1.0
    assert rec["cpu_baseline"] is None          # --no-cpu-baseline


def test_bench_plain_run_dumps_the_timed_latents(tmp_path):
    """a plain bench.py run (no --full) times exactly --steps generations, prints the headline keys and none of the side work, and --dump-outputs
    writes the final latents of the last timed step (float32, the engine's output shape, finite)"""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"] == "f16"
    assert abs(rec["value"] - 16 * 1e3 / rec["ms_per_step"]) < 1e-6 * rec["value"]
    for k in ("ceilings", "cpu_baseline", "parity", "pixel_images_per_s", "roofline_kernels", "four_step", "flux_edit", "power_over_timed_region"):
        assert rec.get(k) is None, k
    assert sorted(os.listdir(tmp_path)) == ["latents.npy"]
    lat = np.load(tmp_path / "latents.npy")
    assert lat.dtype == np.float32 and lat.shape == (16, 4, 64, 64) and np.isfinite(lat).all() and lat.std() > 0.1
