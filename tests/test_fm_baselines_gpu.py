"""GPU tests of the FLUX flow-matching baselines: the update kernel (cs_fm_general_step) through FlowMatchGeneralDiscreteScheduler.step
against the reference's own steps (tests/golden/flux_fm_baselines.npz), the edit engine around a policy-free scheduler, and the drivers
(generate_flux --solver, generate_flux_teacher, FluxTeacherPairDataset)."""
import os

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import generate_flux as gf
from consolver_amd import generate_flux_teacher as gft
from consolver_amd import ppo_data
from consolver_amd.baselines import FlowMatchEulerBaselineScheduler
from consolver_amd.flux import HipFluxTransformer2DModel, FluxKontextSamplingEngine, pack_latents, prepare_latent_image_ids
from consolver_amd.scheduling_fm import FM_SOLVER_TYPES, FlowMatchGeneralDiscreteScheduler
from consolver_amd.synth import synthetic_flux_state_dict
from consolver_amd.tables import calculate_shift

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(num_layers=2, num_single_layers=2, num_heads=4, joint_attention_dim=256)
CASES = [(typ, dt, n) for typ in FM_SOLVER_TYPES for dt in ("f32", "bf16") for n in (4, 5)]


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def cu(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV).to(dtype)


def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def make(typ, n):
    """``typ`` None: the Euler baseline that predates the general scheduler"""
    kw = dict(shift=3.0, use_dynamic_shifting=True)
    s = FlowMatchEulerBaselineScheduler(**kw) if typ is None else FlowMatchGeneralDiscreteScheduler(type=typ, **kw)
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=1.15, device=DEV)
    s.set_begin_index(0)
    return s


def numpy_step(s, x, v):
    """one step of ``s`` on numpy arrays in fp32: the plan applied by hand (pinned to the fp32 goldens by tests/test_fm_baselines.py)"""
    if s.step_index is None:
        s._init_step_index(None)
    p = s.step_plan()
    base = x if p.base == "sample" else s.prev_sample
    w = (s.prev_model_output + v).astype(np.float32) if p.use_v1 else v
    out = (base + (np.float32(p.c) * w).astype(np.float32)).astype(np.float32)
    s.commit_plan(p, x, v)
    return out


# ---------------------------------------------------------------------------------------------------------------- per step
@pytest.mark.parametrize("typ,dt,n", CASES)
def test_every_step_vs_reference_golden(golden, typ, dt, n):
    """sample and model output of every step are the golden's, so the saved state of a second stage is the golden's own"""
    g, k = golden["flux_fm_baselines"], f"{typ}_{dt}_n{n}"
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    s, first = make(typ, n), None
    for i, t in enumerate(s.timesteps):
        prev = s.step(cu(g[f"{k}_s{i}_v"], tdt), t, cu(g[f"{k}_s{i}_x"], tdt), return_dict=False)[0]
        assert prev.dtype == tdt and prev.shape == (3, 5, 67)
        first = prev if first is None else first
        got, want = prev.float().cpu().numpy(), g[f"{k}_s{i}_prev"]
        err, frac = rel_l2(got, want), float(np.mean(got != want))
        print(k, i, "rel-L2", err, "differing", frac)
        if dt == "bf16":
            assert err < 2e-3 and frac < 0.02, (k, i, err, frac)
        else:
            assert err < 1e-6, (k, i, err)
    assert s.step_index == n
    out = make(typ, n).step(cu(g[f"{k}_s0_v"], tdt), s.timesteps[0], cu(g[f"{k}_s0_x"], tdt))
    assert set(out) == {"prev_sample"} and torch.equal(out.prev_sample, first)


@pytest.mark.parametrize("typ", FM_SOLVER_TYPES)
def test_fp32_base_next_to_bf16_model_outputs(golden, typ):
    """an fp32 sample (scheduler_fm.py:401 upcasts it) is read as fp32 and the result rounded ONCE: x' = bf16(x_f32 + bf16(bf16(c) * w)),
    every operation a single fp32 operation or a round-to-nearest-even conversion, so the comparison is exact"""
    g, n = golden["flux_fm_baselines"], 4
    s, ref = make(typ, n), make(typ, n)
    ref._init_step_index(None)
    for i, t in enumerate(s.timesteps):
        x, v = g[f"{typ}_f32_n{n}_s{i}_x"], g[f"{typ}_bf16_n{n}_s{i}_v"]       # x: not representable in bf16
        assert not np.array_equal(bf16_round(x), x)
        p = ref.step_plan()
        base = x if p.base == "sample" else ref.prev_sample
        w = bf16_round(ref.prev_model_output + v) if p.use_v1 else v
        want = bf16_round(base + bf16_round(bf16_round(np.float32(p.c)) * w))
        ref.commit_plan(p, x, v)
        prev = s.step(cu(v, torch.bfloat16), t, cu(x), return_dict=False)[0]
        assert prev.dtype == torch.bfloat16
        assert np.array_equal(prev.float().cpu().numpy(), want), (typ, i, float(np.mean(prev.float().cpu().numpy() != want)))


@pytest.mark.parametrize("typ", FM_SOLVER_TYPES)
def test_out_argument_gives_the_same_result(golden, typ):
    g, k = golden["flux_fm_baselines"], f"{typ}_bf16_n5"
    a, b = make(typ, 5), make(typ, 5)
    for i, t in enumerate(a.timesteps):
        x, v = cu(g[f"{k}_s{i}_x"], torch.bfloat16), cu(g[f"{k}_s{i}_v"], torch.bfloat16)
        buf = torch.full_like(v, float("nan"))
        got = b.step(v, t, x, return_dict=False, out=buf)[0]
        assert got is buf and torch.equal(buf, a.step(v, t, x, return_dict=False)[0])
    with pytest.raises(ValueError, match="out="):
        make(typ, 5).step(v, a.timesteps[0], x, out=torch.empty_like(v, dtype=torch.float32))


@pytest.mark.parametrize("dt,n", [(dt, n) for dt in ("f32", "bf16") for n in (4, 5)])
def test_euler_type_is_bit_identical_to_the_euler_baseline(golden, dt, n):
    g, k = golden["flux_fm_baselines"], f"euler_{dt}_n{n}"
    tdt = torch.bfloat16 if dt == "bf16" else torch.float32
    a, b = make("euler", n), make(None, n)
    for i, t in enumerate(a.timesteps):
        x, v = cu(g[f"{k}_s{i}_x"], tdt), cu(g[f"{k}_s{i}_v"], tdt)
        assert torch.equal(a.step(v, t, x, return_dict=False)[0], b.step(v, t, x, return_dict=False)[0])
    x32 = cu(g[f"euler_f32_n{n}_s0_x"])                                      # ... and with an fp32 sample next to a 16-bit output
    v = cu(g[f"euler_bf16_n{n}_s0_v"], torch.bfloat16)
    assert torch.equal(make("euler", n).step(v, a.timesteps[0], x32, return_dict=False)[0],
                       make(None, n).step(v, a.timesteps[0], x32, return_dict=False)[0])


@pytest.mark.parametrize("io", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("x_f32", [False, True])
@pytest.mark.parametrize("with_v1", [False, True])
def test_c_abi_dtype_pairs(io, out_f32, x_f32, with_v1):
    """the io / out dtype pairs and the fp32 base the scheduler does not reach (fp16; an fp32 result), through the C ABI on [3, 335]: every
    operation is a single fp32 operation or a round-to-nearest-even conversion, so the comparison with the same formula on the CPU is exact"""
    import ctypes as C
    from consolver_amd import _lib as L
    g = torch.Generator().manual_seed(11)
    rnd = lambda t: t.to(io).float()
    x = torch.randn(3, 335, generator=g)
    x = x if x_f32 else rnd(x)
    v2, v1, c = rnd(torch.randn(3, 335, generator=g)), rnd(torch.randn(3, 335, generator=g)), -0.2371
    w = rnd(v1 + v2) if with_v1 else v2
    want = x + rnd(rnd(torch.tensor(c)) * w)
    want = want if out_f32 else rnd(want)
    dx, dv2, dv1 = x.to(DEV) if x_f32 else x.to(DEV).to(io), v2.to(DEV).to(io), v1.to(DEV).to(io)
    out = torch.full((3, 335), float("nan"), device=DEV, dtype=torch.float32 if out_f32 else io)
    a = L.CsFmStepArgs()
    a.x_base, a.v2, a.v1, a.x_out = dx.data_ptr(), dv2.data_ptr(), dv1.data_ptr() if with_v1 else None, out.data_ptr()
    a.c, a.B, a.elems, a.io_dtype, a.out_dtype, a.x_is_f32 = c, 3, 335, L.dtype_code(io), L.dtype_code(out.dtype), int(x_f32)
    L.check(L.lib().cs_fm_general_step(C.byref(a), L.stream_ptr(torch.device(DEV))))
    assert torch.equal(out.float().cpu(), want)


# ---------------------------------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def dit():
    """the reduced DiT of tests/test_flux_gpu.py::test_flux_edit_loop_with_fmppo_scheduler and its inputs (8 x 16 packed grid, B = 1, bf16)"""
    m = HipFluxTransformer2DModel(dict(SMALL, dtype=torch.bfloat16), device=DEV)
    sd = {k: v.to(torch.bfloat16).float() for k, v in synthetic_flux_state_dict(m.manifest(), seed=4).items()}
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(2)
    lat = pack_latents(torch.randn(1, 16, 16, 32, generator=g)).to(torch.bfloat16).to(DEV)
    img = pack_latents(torch.randn(1, 16, 16, 32, generator=g)).to(torch.bfloat16).to(DEV)
    enc = torch.randn(1, 64, 256, generator=g).to(torch.bfloat16).to(DEV)
    pooled = torch.randn(1, 768, generator=g).to(torch.bfloat16).to(DEV)
    return dict(m=m, sd=sd, lat=lat, img=img, enc=enc, pooled=pooled, oracle={}, euler_err={})


def hand_loop(d, sch, n, guidance_scale=2.5):
    """FluxKontextSamplingEngine.generate written out around the model and scheduler.step"""
    lat = d["lat"]
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=calculate_shift(lat.shape[1]), device=DEV)
    sch.set_begin_index(0)
    ids = np.concatenate([prepare_latent_image_ids(8, 16), prepare_latent_image_ids(8, 16, first=1.0)], 0)
    txt_ids = np.zeros((d["enc"].shape[1], 3), np.float32)
    guidance = torch.full([1], guidance_scale, device=DEV, dtype=torch.float32)
    sig = (sch.timesteps.to(lat.dtype) / 1000).to(torch.float32)
    x = lat
    for i, t in enumerate(sch.timesteps):
        v = d["m"](x, sig[i:i + 1].expand(1), guidance=guidance, pooled_projections=d["pooled"], encoder_hidden_states=d["enc"], txt_ids=txt_ids,
                   img_ids=ids, image_latents=d["img"])[0]
        x = sch.step(v, t, x, return_dict=False)[0]
    return x


def oracle_loop(d, typ, n, guidance_scale=2.5):
    """the same loop in fp32 on the CPU: FluxOracle as the velocity model, the golden-pinned numpy step plan as the solver; once per (type, n)"""
    if (typ, n) in d["oracle"]:
        return d["oracle"][typ, n]
    from oracle.flux_oracle import FluxOracle
    if "orc" not in d:
        d["orc"] = FluxOracle(d["sd"], d["m"].config)
    orc = d["orc"]
    torch.set_num_threads(16)
    s = gf.make_scheduler(typ)
    lat, il = d["lat"].float().cpu().numpy(), d["img"].float().cpu()
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=calculate_shift(lat.shape[1]))
    s.set_begin_index(0)
    ids = np.concatenate([prepare_latent_image_ids(8, 16), prepare_latent_image_ids(8, 16, first=1.0)], 0)
    txt_ids = np.zeros((d["enc"].shape[1], 3), np.float32)
    sig = (s.timesteps.to(torch.bfloat16) / 1000).to(torch.float32)       # the engine's model-dtype timestep
    x = lat
    for i in range(n):
        h = torch.cat([torch.from_numpy(x), il], 1)
        v = orc(h, sig[i:i + 1], torch.full((1,), guidance_scale), d["pooled"].float().cpu(), d["enc"].float().cpu(), txt_ids, ids).numpy()[:, :x.shape[1]]
        x = numpy_step(s, x, np.ascontiguousarray(v, dtype=np.float32))
    d["oracle"][typ, n] = x
    return x


# final-latent rel-L2 of the engine (bf16 DiT, bf16 latents between steps) against the fp32 oracle loop: measured value + 10 %
ENGINE_BOUNDS = {("euler", 4): 3.634e-3, ("euler", 5): 4.038e-3,                                # measured 3.3036e-3 / 3.6707e-3
                 ("heun", 4): 3.161e-3, ("heun", 5): 3.420e-3,                                  # 2.8737e-3 / 3.1091e-3 (0.870 / 0.847 of Euler's)
                 ("dpm-solver", 4): 3.270e-3, ("dpm-solver", 5): 3.350e-3,                      # 2.9725e-3 / 3.0454e-3 (0.900 / 0.830)
                 ("dpm-solver-multistep", 4): 3.283e-3, ("dpm-solver-multistep", 5): 3.579e-3}  # 2.9849e-3 / 3.2539e-3 (0.904 / 0.886)


@pytest.mark.parametrize("typ,n", [(typ, n) for typ in FM_SOLVER_TYPES for n in (4, 5)])
def test_engine_runs_every_baseline_and_matches_the_oracle(dit, typ, n):
    """(a) the engine around a policy-free scheduler is the loop written by hand, bit for bit; (b) its final latents against the fp32
    oracle loop; (c) that error within 2 x Euler's on the same model, noise and n: a two-interval update adds half as many forward errors,
    each scaled by twice the interval -- sqrt(2) in quadrature -- and the rest is headroom for propagation through the model."""
    sch = gf.make_scheduler(typ)
    eng = FluxKontextSamplingEngine(dit["m"], sch, guidance_scale=2.5)
    out = eng.generate(dit["lat"], dit["img"], dit["enc"], dit["pooled"], latent_hw=(8, 16), num_inference_steps=n)
    assert out.shape == dit["lat"].shape and out.dtype == torch.bfloat16 and torch.isfinite(out.float()).all() and sch.step_index == n
    assert torch.equal(out, hand_loop(dit, gf.make_scheduler(typ), n))
    with pytest.raises(ValueError, match="policy"):
        eng.generate(dit["lat"], dit["img"], dit["enc"], dit["pooled"], latent_hw=(8, 16), num_inference_steps=n, record=True)
    err = rel_l2(out.float().cpu().numpy(), oracle_loop(dit, typ, n))
    if n not in dit["euler_err"]:
        e = FluxKontextSamplingEngine(dit["m"], gf.make_scheduler("euler"), guidance_scale=2.5)
        eo = e.generate(dit["lat"], dit["img"], dit["enc"], dit["pooled"], latent_hw=(8, 16), num_inference_steps=n)
        dit["euler_err"][n] = rel_l2(eo.float().cpu().numpy(), oracle_loop(dit, "euler", n))
    euler = dit["euler_err"][n]
    print(f"engine {typ} n={n}: rel-L2 vs oracle {err:.4e}, euler {euler:.4e}, ratio {err / euler:.3f}")
    assert err <= 2.0 * euler, (typ, n, err, euler)
    assert err < ENGINE_BOUNDS[typ, n], (typ, n, err)


def test_engine_with_fmppo_scheduler_is_unchanged(dit):
    """the body of tests/test_flux_gpu.py::test_flux_edit_loop_with_fmppo_scheduler, and the engine against the loop written by hand with
    a forced action index: bit-identical"""
    def sched():
        s = consolver_amd.FMPPOScheduler.from_pretrained("x", subfolder="scheduler", order_dim=2, scaler_dim=0, mu_dim=0,
                                                         factor_net_kwargs=dict(hidden_dim=64, num_actions=11))
        s.factor_net.to(DEV)
        s.factor_net.forced_action_idx = torch.zeros(1, 1, dtype=torch.long, device=DEV) + 3
        return s
    sch = sched()
    lat, img, enc, pooled = dit["lat"], dit["img"], dit["enc"], dit["pooled"]
    eng = FluxKontextSamplingEngine(dit["m"], sch, guidance_scale=2.5)
    out = eng.generate(lat, img, enc, pooled, latent_hw=(8, 16), num_inference_steps=4)
    assert out.shape == lat.shape and out.dtype == torch.bfloat16 and torch.isfinite(out.float()).all()
    assert sch.step_index == 4 and float((out.float() - lat.float()).abs().mean()) > 1e-3 and sch.record_conds is False
    assert torch.equal(out, hand_loop(dit, sched(), 4))
    out2, conds, probs, actions, masks = eng.generate(lat, img, enc, pooled, latent_hw=(8, 16), num_inference_steps=4, record=True)
    assert torch.equal(out2, out) and sch.record_conds is False
    assert conds["x"].shape == (1, 3, 2) and conds["epsilon"].shape == (1, 3, 2, 128, 64)
    assert probs.shape == actions.shape == masks.shape == (1, 3, 1) and float(masks.min()) == 1.0
    sig = sch.sigmas.cpu()
    assert torch.allclose(conds["x"][0, :, 0].float().cpu(), sig[1:4].to(torch.bfloat16).float())
    # the one baseline that existed before steps to a 1-tuple as well
    e = FluxKontextSamplingEngine(dit["m"], FlowMatchEulerBaselineScheduler(shift=3.0, use_dynamic_shifting=True), guidance_scale=2.5)
    assert torch.equal(e.generate(lat, img, enc, pooled, latent_hw=(8, 16), num_inference_steps=4), hand_loop(dit, gf.make_scheduler("euler"), 4))
    with pytest.raises(ValueError, match="policy"):
        e.generate(lat, img, enc, pooled, latent_hw=(8, 16), num_inference_steps=4, record=True)


# ---------------------------------------------------------------------------------------------------------------- drivers
def test_teacher_pair_generator_dataset_and_solver_driver(dit, tmp_path):
    from PIL import Image
    from safetensors import safe_open
    from consolver_amd.generate import prepare_latents
    from consolver_amd.vae import HipAutoencoderKL, FLUX_VAE_CONFIG, encode_image_latents
    from consolver_amd.synth import synthetic_vae_state_dict
    vcfg = dict(FLUX_VAE_CONFIG); vcfg.update(layers_per_block=1, sample_size=16, with_encoder=True)
    vae = HipAutoencoderKL(vcfg, device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=9))
    data = tmp_path / "data"
    os.makedirs(data / "ref_images"); os.makedirs(data / "prompts")
    rng, g = np.random.default_rng(0), torch.Generator().manual_seed(5)
    for i in range(3):
        Image.fromarray(rng.integers(0, 255, (96, 160, 3), dtype=np.uint8)).save(data / "ref_images" / f"{i}.png")
        if i != 1:                                           # index 1 has no prompt: skipped
            with open(data / "prompts" / f"{i}.txt", "w") as f:
                f.write(f"make it {i}")
    embeds = {str(i): (torch.randn(64, 256, generator=g), torch.randn(768, generator=g)) for i in range(3)}
    cache_path = str(tmp_path / "emb.safetensors")
    gf.save_instruction_cache(cache_path, embeds)
    res = gft.main(["--data", str(data), "--instruction-cache", cache_path, "--count", "3", "--steps", "3"], transformer=dit["m"], vae=vae)
    assert res["pairs"] == 2 and res["indices"] == [0, 2] and res["steps"] == 3
    assert sorted(os.listdir(data)) == ["edited_images", "initial_noises", "obtained_noises", "prompts", "ref_images"]
    assert sorted(os.listdir(data / "initial_noises")) == sorted(os.listdir(data / "obtained_noises")) == ["0.pt", "2.pt"]
    assert sorted(os.listdir(data / "edited_images")) == ["0.png", "2.png"]
    # replay of index 0 by hand
    initial, obtained = torch.load(data / "initial_noises" / "0.pt"), torch.load(data / "obtained_noises" / "0.pt")
    assert initial.shape == obtained.shape == (1, 64, 64) and initial.dtype == obtained.dtype == torch.bfloat16 and not initial.is_cuda
    noise = pack_latents(prepare_latents(1, (16, 16, 16), 42, torch.device(DEV), torch.bfloat16))
    assert torch.equal(initial, noise.cpu())
    il = pack_latents(encode_image_latents(vae, gf.preprocess_image(str(data / "ref_images" / "0.png"), 128).to(DEV, torch.float16))).to(torch.bfloat16)
    with safe_open(cache_path, framework="pt", device="cpu") as cache:
        pe, pooled = gf.load_instruction_embeds(cache, "0", torch.device(DEV))
    eng = FluxKontextSamplingEngine(dit["m"], gf.make_scheduler("euler"), guidance_scale=2.5)
    assert torch.equal(obtained, eng.generate(noise, il, pe, pooled, latent_hw=(8, 8), num_inference_steps=3).cpu())
    assert Image.open(data / "edited_images" / "0.png").size == (128, 128)
    # the dataset reads the tree back
    ds = ppo_data.FluxTeacherPairDataset(str(data), (128, 128), strict=True)
    assert len(ds) == 2
    image, text, n0, l0, ref = ds[0]
    assert text == "make it 0" and torch.equal(n0, initial[0]) and torch.equal(l0, obtained[0])
    assert image.shape == ref.shape == (3, 128, 128) and float(image.min()) >= -1 and float(ref.min()) >= 0 and float(ref.max()) <= 1
    assert ds[1][1] == "make it 2"
    # generate_flux --solver: the reference layout from a baseline; --policy belongs to the learned solver
    out_dir = tmp_path / "out"
    res = gf.main(["--synthetic", "2", "--solver", "heun", "--out", str(out_dir), "--steps", "3"], transformer=dit["m"], vae=vae)
    assert res["edits"] == 2 and res["solver"] == "heun"
    assert sorted(os.listdir(out_dir)) == ["synthetic"] and sorted(os.listdir(out_dir / "synthetic")) == ["synthetic_0", "synthetic_1"]
    for key in ("synthetic_0", "synthetic_1"):
        assert sorted(os.listdir(out_dir / "synthetic" / key)) == ["edited_image.jpg", "instruction.txt", "ref_image.jpg"]
        assert Image.open(out_dir / "synthetic" / key / "edited_image.jpg").size == (128, 128)
    with pytest.raises(SystemExit) as e:
        gf.main(["--synthetic", "1", "--solver", "heun", "--policy", "p.ckpt", "--out", str(out_dir)], transformer=dit["m"], vae=vae)
    assert e.value.code != 0
