"""GPU tests of the Multistep DPM-Solver: the update kernel (cs_dpm_multistep_step) through DPMSolverMultistepScheduler.step against
tests/dpm_oracle.py, the engine around it against UNetOracle + the oracle, the teacher-pair generator and the CLIs."""
import os

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import DPMSolverMultistepScheduler, SD15_MULTISTEP_DPM_KWARGS
from consolver_amd.engine import SDSamplingEngine
from consolver_amd.synth import synthetic_prompt_embeds
from oracle import solver_oracle as so
from tests.dpm_oracle import COMBOS, DPMSolverOracle, combo_id

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SD15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
REDUCED = dict(layers_per_block=1, sample_size=16)
PP = dict(SD15, algorithm_type="dpmsolver++", final_sigmas_type="zero")      # the class defaults on SD1.5's betas


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def cu(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)


def pair(n, **kw):
    s, o = DPMSolverMultistepScheduler(**kw), DPMSolverOracle(**kw)
    s.set_timesteps(n, device=DEV); o.set_timesteps(n)
    return s, o


def per_step_errors(kw, n, shape, dtype=torch.float32, steps=None, seed=0):
    """worst rel-L2 of prev_sample (and of the converted output m0) over the steps: both sides start every step from the same state (the oracle's, rounded to
    ``dtype``) and get the same ``dtype``-representable random eps; the scheduler keeps its own history."""
    rng = np.random.default_rng(seed)
    s, o = pair(n, **kw)
    name = "f16" if dtype == torch.float16 else None
    rnd = (lambda a: so.round_like(np.asarray(a, np.float32), name)) if name else (lambda a: np.asarray(a, np.float32))
    x = rnd(rng.standard_normal(shape))
    worst = worst_m = 0.0
    for i, t in enumerate(s.timesteps[:steps]):
        e = rnd(rng.standard_normal(shape))
        m_out = torch.empty(shape, dtype=dtype, device=DEV)
        got = s.step(cu(e, dtype), t, cu(x, dtype), return_dict=False, eps_out=m_out)[0]
        want = o.step(e, x)
        assert got.dtype == dtype and got.shape == tuple(shape)
        worst = max(worst, rel_l2(got.float().cpu().numpy(), want))
        worst_m = max(worst_m, rel_l2(m_out.float().cpu().numpy(), o.last_converted()))
        x = rnd(want)
    return worst, worst_m


@pytest.mark.parametrize("n", [5, 16])
@pytest.mark.parametrize("combo", COMBOS, ids=combo_id)
def test_step_matches_oracle_fp32(combo, n):
    """every variant, every step (first-order first step, first-order last step at n = 5, second-order last step at n = 16 under sigma_min): fp32 in and out,
    < 1e-6 like the sibling kernel (test_ddim_baseline_scheduler_matches_oracle).  105 elements per sample: sample 1 starts off a vector boundary."""
    for shape in ((2, 3, 5, 7), (3, 4, 16, 16)):
        err, err_m = per_step_errors(dict(SD15, **combo), n, shape)
        print("dpm fp32 per-step", combo_id(combo), n, shape, err, err_m)
        assert err < 1e-6 and err_m < 1e-6, (shape, err, err_m)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", [(3, 5), (3, 1027), (1, 4, 16, 16), (64, 73728)], ids=["lt_one_vector", "1027", "B1", "grid_stride"])
def test_shape_edges_second_order(shape, dtype):
    """fewer elements than one vector, a ragged tail behind full vectors, one sample, and more vectors than the capped grid holds (cap ceil(2048 / 64) = 32 blocks of 256
    threads; 73 728 elements are 72 / 36 blocks' worth in fp32 / fp16): three steps of an n = 16 run, so the second and third are second order."""
    bound = 1e-6 if dtype == torch.float32 else 1e-3
    for kw in (dict(SD15_MULTISTEP_DPM_KWARGS), PP):
        err, err_m = per_step_errors(kw, 16, shape, dtype, steps=3)
        print("dpm shape edge", kw["algorithm_type"], shape, dtype, err, err_m)
        assert err < bound and err_m < bound, (kw["algorithm_type"], err, err_m)


def test_empty_batch_and_errors():
    s = DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS)
    z = torch.zeros(0, 4, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        s.step(z, 999, z)                                                       # before set_timesteps
    s.set_timesteps(4, device=DEV)
    out = s.step(z, s.timesteps[0], z, return_dict=True)
    assert out.prev_sample.shape == (0, 4, 8, 8) and set(out) == {"prev_sample"}
    assert s.step(z, s.timesteps[1], z, return_dict=False)[0].shape == (0, 4, 8, 8)
    # out= of the wrong dtype is refused; so is a CPU tensor (there is no CPU path)
    s.set_timesteps(4, device=DEV)
    x, e16 = torch.randn(2, 4, 8, 8, device=DEV), torch.randn(2, 4, 8, 8, device=DEV).half()
    with pytest.raises(ValueError):
        s.step(e16, s.timesteps[0], x, out=torch.empty_like(e16))              # the fp32 sample gives an fp32 result
    with pytest.raises(ValueError):
        s.step(e16, s.timesteps[0], x.half(), out=torch.empty_like(x))
    with pytest.raises(RuntimeError):
        s.step(e16.cpu(), s.timesteps[0], x)
    # the C ABI refuses a conversion or CFG without m_out, by code
    import ctypes as C
    from consolver_amd import _lib as L
    a = L.CsDpmStepArgs()
    e = torch.randn(2, 4, 8, 8, device=DEV)
    xo = torch.empty_like(x)
    a.x, a.eps_text, a.x_out, a.B, a.elems = x.data_ptr(), e.data_ptr(), xo.data_ptr(), 2, 256
    a.io_dtype = a.out_dtype = L.CS_F32
    a.conv_x, a.conv_e, a.cx, a.c0 = 1.0, -1.0, 1.0, 0.5
    assert L.lib().cs_dpm_multistep_step(C.byref(a), L.stream_ptr(torch.device(DEV))) < 0
    a.conv_x, a.conv_e, a.eps_uncond = 0.0, 1.0, e.data_ptr()
    assert L.lib().cs_dpm_multistep_step(C.byref(a), L.stream_ptr(torch.device(DEV))) < 0
    assert L.lib().cs_dpm_multistep_step(None, L.stream_ptr(torch.device(DEV))) < 0
    a.B = 0
    assert L.lib().cs_dpm_multistep_step(C.byref(a), L.stream_ptr(torch.device(DEV))) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("kw", [dict(SD15_MULTISTEP_DPM_KWARGS), PP], ids=["dpmsolver", "dpmsolver++"])
def test_fused_cfg_equals_the_combined_eps(kw):
    """step(c, eps_uncond=u, guidance_scale=3) == step(u + 3 (c - u)) (< 2e-6, the bound of the same property in test_properties_full_size), at a first- and a
    second-order step; the ring slot handed in as eps_out holds m0: the combined eps (dpmsolver) or the x0 prediction (dpmsolver++)."""
    torch.manual_seed(2)
    shape = (3, 4, 16, 16)
    a = DPMSolverMultistepScheduler(**kw); b = DPMSolverMultistepScheduler(**kw); o = DPMSolverOracle(**kw)
    a.set_timesteps(16, device=DEV); b.set_timesteps(16, device=DEV); o.set_timesteps(16)
    x = torch.randn(shape, device=DEV)
    ring = [torch.empty(shape, device=DEV) for _ in range(2)]
    for i in range(3):
        u, c = torch.randn(shape, device=DEV), torch.randn(shape, device=DEV)
        comb = u + 3.0 * (c - u)
        fused = a.step(c, a.timesteps[i], x, return_dict=False, eps_uncond=u, guidance_scale=3.0, eps_out=ring[i % 2])[0]
        plain = b.step(comb, b.timesteps[i], x, return_dict=False)[0]
        want = o.step(comb.cpu().numpy(), x.cpu().numpy())
        assert rel_l2(fused.cpu().numpy(), plain.cpu().numpy()) < 2e-6, i
        assert rel_l2(fused.cpu().numpy(), want) < 2e-6, i
        assert rel_l2(ring[i % 2].cpu().numpy(), o.last_converted()) < 2e-6, i
        if kw["algorithm_type"] == "dpmsolver":
            assert rel_l2(ring[i % 2].cpu().numpy(), comb.cpu().numpy()) < 2e-6
        x = fused


def test_dtypes():
    rng = np.random.default_rng(4)
    shape, n = (3, 4, 16, 16), 8
    f16 = lambda a: so.round_like(np.asarray(a, np.float32), "f16")
    # fp16 sample and outputs, free running for 8 steps against the unrounded oracle on the same fp16 eps
    for kw in (dict(SD15_MULTISTEP_DPM_KWARGS), PP):
        s, o = pair(n, **kw)
        x0 = f16(rng.standard_normal(shape))
        xg, xo = cu(x0, torch.float16), x0
        for i, t in enumerate(s.timesteps):
            e = f16(rng.standard_normal(shape))
            xg = s.step(cu(e, torch.float16), t, xg, return_dict=False)[0]
            xo = o.step(e, xo)
            assert xg.dtype == torch.float16
            err = rel_l2(xg.float().cpu().numpy(), xo)
            print("dpm fp16 trajectory", kw["algorithm_type"], i, err)
            assert err < 1e-3, (kw["algorithm_type"], i, err)
    # fp32 sample next to fp16 outputs (the engine's fp16-eps form), CFG: fp32 result, fp32-class against the oracle fed the same fp16-rounded combined eps;
    # out_lp is the fp16 rounding of the result, written in the same pass
    s, o = pair(n, **SD15_MULTISTEP_DPM_KWARGS)
    x0 = rng.standard_normal(shape).astype(np.float32)
    xg, xo = cu(x0), x0
    lp = torch.empty(shape, dtype=torch.float16, device=DEV)
    for i, t in enumerate(s.timesteps):
        eu = f16(rng.standard_normal(shape))
        ec = f16(eu + 0.3 * rng.standard_normal(shape))
        prev = s.step(cu(ec, torch.float16), t, xg, return_dict=False, eps_uncond=cu(eu, torch.float16), guidance_scale=3.0, out_lp=lp)[0]
        assert prev.dtype == torch.float32
        want = o.step(f16(so.cfg_combine(eu, ec, 3.0)), xo)
        err = rel_l2(prev.cpu().numpy(), want)
        print("dpm fp32 state / fp16 eps", i, err)
        assert err < 2e-6, (i, err)
        assert torch.equal(lp, prev.to(torch.float16))
        xg, xo = prev, np.asarray(prev.cpu().numpy(), np.float64)
    # a 16-bit sample keeps its dtype unless prev_sample_dtype asks for the promotion
    s.set_timesteps(n, device=DEV)
    e16, x16 = cu(f16(rng.standard_normal(shape)), torch.float16), cu(f16(x0), torch.float16)
    p16 = s.step(e16, s.timesteps[0], x16, return_dict=False)[0]
    s.set_timesteps(n, device=DEV)
    s.prev_sample_dtype = torch.float32
    p32 = s.step(e16, s.timesteps[0], x16, return_dict=False)[0]
    assert p16.dtype == torch.float16 and p32.dtype == torch.float32 and torch.equal(p16, p32.to(torch.float16))


def test_two_identical_calls_are_bit_identical():
    torch.manual_seed(5)
    shape = (2, 3, 5, 7)
    outs = []
    x, es = torch.randn(shape, device=DEV), [torch.randn(shape, device=DEV) for _ in range(3)]
    for _ in range(2):
        s = DPMSolverMultistepScheduler(**PP)
        s.set_timesteps(16, device=DEV)
        y = x
        for i in range(3):
            y = s.step(es[i], s.timesteps[i], y, return_dict=False)[0]
        outs.append(y)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- engine
def reduced_models():
    from consolver_amd.synth import synthetic_vae_state_dict
    from consolver_amd.vae import HipAutoencoderKL
    from tests._models import get_unet
    unet, _ = get_unet(REDUCED, seed=5)
    if "vae" not in reduced_models.__dict__:
        vae = HipAutoencoderKL(dict(REDUCED), device=DEV)
        vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=6))
        reduced_models.vae = vae
    return unet, reduced_models.vae


def engine_inputs(B, seed=43):
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()
    return pe, ne, noise


# measured on the MI355X (reduced UNet, B = 2, CFG 3, default engine: fp32 state and eps, precision schedule "auto"), rel-L2 of the final latents against
# UNetOracle + the solver oracle in fp32 on the CPU:   n = 16: DPM-Solver 5.775e-4, DDIM 6.183e-4;   n = 5: DPM-Solver 8.847e-4, DDIM 9.577e-4.   Bound = measured + 10 %.
ENGINE_BOUND = {16: 6.35e-4, 5: 9.73e-4}


@pytest.mark.parametrize("n", [16, 5])
def test_engine_against_unet_oracle_and_ddim_comparator(n):
    """n = 16 is the smallest n whose last step is second order; n = 5 is warm-up plus the lower-order final step.  DDIMBaselineScheduler on the same model, noise and n
    is the comparator: both are linear updates of the same eps with coefficients of the same size, so a DPM error above 1.5 x the DDIM error is a defect."""
    from consolver_amd.baselines import DDIMBaselineScheduler
    from tests._models import get_oracle
    unet, _ = reduced_models()
    B, g = 2, 3.0
    pe, ne, noise = engine_inputs(B)
    orc_u = get_oracle(REDUCED, seed=5)
    ctx = torch.cat([ne, pe]).float()

    def eps_oracle(x, t):
        e = orc_u(torch.from_numpy(np.concatenate([x, x]).astype(np.float32)), int(t), ctx).numpy()
        return so.cfg_combine(e[:B], e[B:], g)

    eng = SDSamplingEngine(unet, DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS), guidance_scale=g)
    got = eng.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n).float().cpu().numpy()
    o = DPMSolverOracle(**SD15_MULTISTEP_DPM_KWARGS)
    o.set_timesteps(n)
    x = noise.float().numpy().astype(np.float64)
    for t in o.timesteps:
        x = o.step(eps_oracle(x, t), x)
    err = rel_l2(got, x)

    eng_d = SDSamplingEngine(unet, DDIMBaselineScheduler(**SD15, timestep_spacing="trailing"), guidance_scale=g)
    got_d = eng_d.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n).float().cpu().numpy()
    ac = so.alphas_cumprod(so.make_betas("scaled_linear", 0.00085, 0.012))
    xd = noise.float().numpy()
    for t in so.sd_timesteps(n, spacing="trailing"):
        pt = so.sd_prev_timestep(int(t), n)
        xd = so.ddim_update(xd, eps_oracle(xd, t).astype(np.float32), ac[int(t)], ac[pt] if pt >= 0 else ac[0])
    err_d = rel_l2(got_d, xd)
    print(f"engine n={n}: dpm-solver rel-L2 {err:.4e}, ddim comparator rel-L2 {err_d:.4e}, ratio {err / err_d:.3f}")
    assert np.isfinite(got).all()
    assert err <= 1.5 * err_d, (err, err_d)
    assert err < ENGINE_BOUND[n], err


@pytest.mark.parametrize("latents_dtype", [torch.float32, torch.float16], ids=["f32_state", "f16_state"])
def test_engine_graph_is_bit_identical_to_eager(latents_dtype):
    """nothing is sampled in this solver: the captured generation is the eager one bit for bit, and so is its second replay (n = 16: both orders, precision schedule on)"""
    unet, _ = reduced_models()
    B, n = 2, 16
    pe, ne, noise = [t.to(DEV) for t in engine_inputs(B, seed=44)]
    eng = SDSamplingEngine(unet, DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS), guidance_scale=3.0, latents_dtype=latents_dtype)
    eager = eng.generate(pe, ne, latents=noise, num_inference_steps=n).clone()
    graph = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    again = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    assert eager.dtype == latents_dtype and bool(torch.isfinite(eager).all())
    assert torch.equal(eager, graph) and torch.equal(graph, again)
    # without CFG the scheduler is handed the ring slot itself (no eps_out)
    eng1 = SDSamplingEngine(unet, DPMSolverMultistepScheduler(**PP), guidance_scale=1.0, latents_dtype=latents_dtype)
    e1 = eng1.generate(pe, latents=noise, num_inference_steps=5).clone()
    g1 = eng1.generate(pe, latents=noise, num_inference_steps=5, use_graph=True).clone()
    assert bool(torch.isfinite(e1).all()) and torch.equal(e1, g1)


# ---------------------------------------------------------------------------------------------------- teacher pairs, CLIs, pipeline
def test_teacher_pair_generator(tmp_path):
    from consolver_amd import generate as gen, ppo
    from consolver_amd.generate_teacher import generate_teacher_pairs
    from consolver_amd.ppo_data import TeacherPairDataset, collate_teacher_pairs
    unet, vae = reduced_models()
    eng = SDSamplingEngine(unet, DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS), guidance_scale=3.0, vae=vae)
    N, world, bs, seed, n = 5, 2, 2, 7, 16
    prompts = [f"prompt {i}" for i in range(N)]
    pe, ne = synthetic_prompt_embeds(N, seed=1001).half(), synthetic_prompt_embeds(N, seed=1002).half()
    out = str(tmp_path)
    counts = [generate_teacher_pairs(prompts, pe, ne, eng, out, rank=r, world=world, num_inference_steps=n, batch_size=bs, seed=seed, device=torch.device(DEV))
              for r in range(world)]
    assert counts == [2, 3]                                   # rank 1: a full batch and a ragged one
    ids = ["0_00000000", "0_00000001", "1_00000000", "1_00000001", "1_00000002"]
    want = sorted([f"{i}.txt" for i in ids] + [f"{i}.png" for i in ids] + [f"noise_{i}.pth" for i in ids] + [f"latent_{i}.pth" for i in ids])
    assert sorted(os.listdir(out)) == want
    ds = TeacherPairDataset(out, strict=True)
    assert ds.ids == ids
    samples = [ds[i] for i in range(len(ds))]
    assert [s[0] for s in samples] == prompts
    for text, noise, latent in samples:
        assert noise.dtype == torch.float16 and latent.dtype == torch.float16 and noise.shape == latent.shape == (4, 16, 16) and not noise.is_cuda
    # the same noise on both ranks (seed + batch_idx), bit for bit; the latent is the fp16 cast of engine.generate on that noise
    for b, sl in ((0, slice(2, 4)), (1, slice(4, 5))):        # rank 1's two batches
        drawn = gen.prepare_latents(sl.stop - sl.start, (4, 16, 16), seed + b, torch.device(DEV))
        assert torch.equal(torch.stack([samples[i][1] for i in range(sl.start, sl.stop)]), drawn.cpu())
        lat = eng.generate(pe[sl].to(DEV), ne[sl].to(DEV), latents=drawn, num_inference_steps=n).to(torch.float16).cpu()
        assert torch.equal(torch.stack([samples[i][2] for i in range(sl.start, sl.stop)]), lat)
    assert torch.equal(samples[0][1], samples[2][1])          # rank 0 batch 0 and rank 1 batch 0 drew the same noise
    from consolver_amd import evaluation as ev
    img = ev.load_image_tensor(os.path.join(out, "1_00000002.png"), "cpu")
    assert img.shape == (3, 128, 128) and float(img.std()) > 0.01
    # the trainer consumes them: one image_psnr rollout against the stored latents
    text, noise, target = collate_teacher_pairs(samples[2:])
    assert noise.shape == target.shape == (3, 4, 16, 16)
    sch = consolver_amd.PPOScheduler(**SD15, timestep_spacing="trailing", order_dim=4, scaler_dim=0, factor_net_kwargs=dict(hidden_dim=32, num_actions=11))
    sch.factor_net.to(DEV)
    roll = ppo.collect_rollout(None, sch, unet, vae, noise.to(DEV), text, None, target.to(DEV), cfg=3.0, num_inference_steps=4, decode_batch_size=2,
                               prompt_embeds=pe[2:].to(DEV), negative_prompt_embeds=ne[2:].to(DEV))
    assert roll["rewards"].shape == (3, 1) and bool(torch.isfinite(roll["rewards"]).all()) and bool(torch.isfinite(roll["advantages"]).all())


def test_cli_generate_teacher_and_solver_switch(tmp_path):
    """python -m consolver_amd.generate_teacher / generate --solver, in process (on the reduced models: the full-size synthetic ones take 13 s to build)"""
    from consolver_amd import generate as gen, generate_teacher as gt
    unet, vae = reduced_models()
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = gt.main(["--generation_path", a, "--synthetic", "3", "--num_inference_steps", "16", "--batch-size", "2"], unet=unet, vae=vae)
    assert r["pairs"] == 3 and r["steps"] == 16 and len(os.listdir(a)) == 12
    r = gt.main(["--generation_path", b, "--synthetic", "3", "--num_inference_steps", "16", "--batch-size", "2", "--seed-stride", "1000"], unet=unet, vae=vae)
    for i in range(3):                                        # rank 0: the stride changes nothing
        for kind in ("noise", "latent"):
            assert torch.equal(torch.load(os.path.join(a, f"{kind}_0_{i:08d}.pth")), torch.load(os.path.join(b, f"{kind}_0_{i:08d}.pth")))
    assert torch.equal(torch.load(os.path.join(a, "noise_0_00000000.pth")), gen.prepare_latents(2, (4, 16, 16), 0, torch.device(DEV))[0].cpu())
    # rank 1 of 2 with the stride draws seed + batch_idx + 1000
    eng = SDSamplingEngine(unet, DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS), guidance_scale=3.0, vae=vae)
    pe, ne = synthetic_prompt_embeds(4, seed=1001).half(), synthetic_prompt_embeds(4, seed=1002).half()
    c = str(tmp_path / "c")
    gt.generate_teacher_pairs([f"p{i}" for i in range(4)], pe, ne, eng, c, rank=1, world=2, num_inference_steps=2, batch_size=2, seed=0, seed_stride=1000,
                              device=torch.device(DEV))
    n1 = torch.load(os.path.join(c, "noise_1_00000000.pth"))
    assert torch.equal(n1, gen.prepare_latents(2, (4, 16, 16), 1000, torch.device(DEV))[0].cpu())
    assert not torch.equal(n1, gen.prepare_latents(2, (4, 16, 16), 0, torch.device(DEV))[0].cpu())
    # generate --solver
    for solver in ("multistep-dpmsolver", "ddim"):
        d = str(tmp_path / solver)
        r = gen.main(["--out", d, "--synthetic", "2", "--steps", "8", "--batch-size", "2", "--solver", solver], unet=unet, vae=vae)
        assert r["images"] == 2 and r["solver"] == solver and r["use_conv"] is False
        assert sorted(f for f in os.listdir(d) if f.endswith(".png")) == ["0_00000000.png", "0_00000001.png"]
    with pytest.raises(SystemExit):
        gen.main(["--out", str(tmp_path / "x"), "--synthetic", "2", "--solver", "ddim", "--use_conv"], unet=unet, vae=vae)


def test_pipeline_result_carries_init_and_final_latents():
    from consolver_amd.pipeline import ConsistencySolverPipeline
    unet, vae = reduced_models()
    pipe = ConsistencySolverPipeline(unet, DPMSolverMultistepScheduler(**SD15_MULTISTEP_DPM_KWARGS), vae)
    B = 2
    pe, ne, noise = [t.to(DEV) for t in engine_inputs(B, seed=45)]
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=noise, num_inference_steps=5, guidance_scale=3.0, output_type="pt")
    assert out.images.shape == (B, 3, 128, 128)
    assert out.init_latent.shape == out.generate_latent.shape == (B, 4, 16, 16) and not out.init_latent.is_cuda and not out.generate_latent.is_cuda
    assert torch.equal(out.init_latent, noise.cpu()) and bool(torch.isfinite(out.generate_latent).all())
    lat = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=noise, num_inference_steps=5, guidance_scale=3.0, output_type="latent")
    assert torch.equal(lat.images.cpu(), lat.generate_latent) and torch.equal(lat.generate_latent, out.generate_latent)
    tup = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=noise, num_inference_steps=5, guidance_scale=3.0, output_type="pt", return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 2 and tup[1] is None          # the tuple form is unchanged
