"""GPU tests of UniPC: the fused corrector + predictor kernel (cs_unipc_step) through the C ABI against tests/unipc_oracle.py, UniPCMultistepScheduler.step around
it, and the engine against UNetOracle + the oracle with DDIM as the comparator."""
import ctypes as C

import numpy as np
import pytest
import torch

from consolver_amd import SD15_UNIPC_KWARGS, UniPCMultistepScheduler
from consolver_amd import _lib as L
from consolver_amd.engine import SDSamplingEngine
from consolver_amd.synth import synthetic_prompt_embeds
from oracle import solver_oracle as so
from tests.unipc_oracle import UniPCOracle, combo_id, combos

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SD15 = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
REDUCED = dict(layers_per_block=1, sample_size=16)
# (io dtype, state dtype, CFG) and the per-step rel-L2 bound of the sibling kernel (tests/test_dpm_gpu.py)
MODES = {"f32": (torch.float32, torch.float32, False, 1e-6), "f32_state_f16_eps_cfg": (torch.float16, torch.float32, True, 2e-6),
         "f16": (torch.float16, torch.float16, False, 1e-3)}


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rnd(a, dtype):
    return so.round_like(np.asarray(a, np.float32), "f16" if dtype == torch.float16 else None)


def cu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV).to(dtype)


def abi_step(s, i, x, eps, eps_u, g, x_last, m0, m1, io, st, corr_order, this_order, use_corr, inplace=False, lp=True):
    """one cs_unipc_step call on device tensors with the scalars of UniPCMultistepScheduler.step_scalars; a tensor whose coefficient is zero is passed as NULL.
    Returns (m_out, x_c, x_next, lp copy or None)."""
    conv_x, conv_e, (a_x, a_0, a_1, a_n), (p_x, p_0, p_1), use_corr = s.step_scalars(i, corr_order, this_order, use_corr)
    a = L.CsUnipcStepArgs()
    B = x.shape[0]
    m_out, x_out = torch.empty_like(eps), torch.empty_like(x)
    x_c = x_last if (inplace and use_corr) else torch.empty_like(x)
    a.x, a.eps_text, a.eps_uncond, a.guidance = x.data_ptr(), eps.data_ptr(), (eps_u.data_ptr() if eps_u is not None else None), float(g)
    a.use_corr = int(use_corr)
    a.x_last = x_last.data_ptr() if use_corr else None
    a.m_prev0 = m0.data_ptr() if ((use_corr and a_0 != 0.0) or p_1 != 0.0) else None
    a.m_prev1 = m1.data_ptr() if (use_corr and a_1 != 0.0) else None
    a.B, a.elems = B, x.numel() // max(B, 1)
    a.io_dtype, a.out_dtype, a.x_is_f32 = L.dtype_code(io), L.dtype_code(st), int(st == torch.float32 and io != torch.float32)
    a.x_out, a.m_out, a.x_last_out = x_out.data_ptr(), m_out.data_ptr(), x_c.data_ptr()
    out_lp = None
    if lp and st == torch.float32:
        out_lp = torch.empty(x.shape, dtype=torch.float16, device=DEV)
        a.x_out_lp, a.lp_dtype = out_lp.data_ptr(), L.CS_F16
    a.conv_x, a.conv_e, a.a_x, a.a_0, a.a_1, a.a_n, a.p_x, a.p_0, a.p_1 = (float(v) for v in (conv_x, conv_e, a_x, a_0, a_1, a_n, p_x, p_0, p_1))
    L.check(L.lib().cs_unipc_step(C.byref(a), L.stream_ptr(torch.device(DEV))))
    nulls = (a.x_last is None, a.m_prev0 is None, a.m_prev1 is None)
    return m_out, x_c, x_out, out_lp, nulls


def per_step_errors(kw, n, shape, mode, steps=None, seed=0):
    """worst rel-L2 of (m_new, x_c, x_next) over the steps.  Both sides start every step from the same state: the oracle's sample, last_sample and converted outputs
    are rounded to the dtypes the kernel stores them in after every step, and both get the same representable eps.  With 16-bit model outputs the kernel's m_new is
    first held elementwise to the half-ulp of the oracle's value (plus the fp32 error of the conversion) and then handed to the oracle as its rounded history entry
    (``round_m``): a value that sits on a rounding boundary may round either way, and x_c / x_next are judged on the same entry."""
    io, st, cfg, _ = MODES[mode]
    rng = np.random.default_rng(seed)
    s, o = UniPCMultistepScheduler(**kw), UniPCOracle(**kw)
    s.set_timesteps(n, device=DEV); o.set_timesteps(n)
    x = rnd(rng.standard_normal(shape), st)
    worst = [0.0, 0.0, 0.0]
    null_log = []
    zero = np.zeros(shape, np.float32)
    for i in range(n if steps is None else steps):
        if cfg:
            eu = rnd(rng.standard_normal(shape), io)
            ec = rnd(eu + 0.3 * rng.standard_normal(shape), io)
            e = rnd(so.cfg_combine(eu, ec, 3.0), io)
        else:
            eu, ec = None, rnd(rng.standard_normal(shape), io)
            e = ec
        hist = [m for m in o.model_outputs[::-1] if m is not None]
        use_corr = i > 0 and (i - 1) not in kw.get("disable_corrector", [])
        corr_order = o.this_order or 0
        this_order = min(min(kw.get("solver_order", 2), n - i), o.lower_order_nums + 1)
        m_out, x_c, x_next, lp, nulls = abi_step(
            s, i, cu(x, st), cu(ec, io), cu(eu, io) if cfg else None, 3.0 if cfg else 1.0, cu(o.last_sample if o.last_sample is not None else zero, st),
            cu(hist[0] if len(hist) > 0 else zero, io), cu(hist[1] if len(hist) > 1 else zero, io), io, st, corr_order, this_order, use_corr)
        null_log.append(nulls)
        km = m_out.float().cpu().numpy().astype(np.float64)

        def round_m(m):
            if io == torch.float32:
                return rnd(m, io)
            a_s, s_s = o.alpha_sigma(o.sigmas[i])
            size = (np.abs(x) + s_s * np.abs(e)) / a_s if kw.get("prediction_type", "epsilon") == "epsilon" else a_s * np.abs(x) + s_s * np.abs(e)
            assert np.all(np.abs(km - m) <= 2.0 ** -11 * np.abs(m) + 3 * 2.0 ** -24 * size + 2.0 ** -25), i
            return km
        want = o.step(e, x, round_m=round_m)
        assert o.this_order == this_order
        worst[0] = max(worst[0], rel_l2(km, o.last_converted()))
        worst[1] = max(worst[1], rel_l2(x_c.float().cpu().numpy(), o.corrected))
        worst[2] = max(worst[2], rel_l2(x_next.float().cpu().numpy(), want))
        assert x_next.dtype == st and x_c.dtype == st and m_out.dtype == io
        if lp is not None:
            assert torch.equal(lp, x_next.to(torch.float16)), i                 # the copy is the 16-bit rounding of x_out, exactly
        # the next step reads what the kernel stores: the oracle continues from the rounded state
        x = rnd(want, st)
        o.last_sample = np.asarray(rnd(o.last_sample, st), np.float64)
    return worst, null_log


@pytest.mark.parametrize("n", [5, 16])
@pytest.mark.parametrize("combo", list(combos(16)), ids=combo_id)
@pytest.mark.parametrize("mode", list(MODES))
def test_step_matches_oracle(mode, combo, n):
    """every variant, every step, in the three dtype forms: m_new, x_c and x_next within the sibling kernel's bounds (fp32 in and out < 1e-6; fp32 state beside fp16 outputs
    with CFG 3 < 2e-6; fp16 in and out < 1e-3 per step).  105 elements per sample, 210 in all: vector body and scalar tail at both widths.  The first step, and a step whose
    corrector is disabled, run with NULL x_last / m_prev1."""
    kw = dict(SD15, **combo)
    worst, nulls = per_step_errors(kw, n, (2, 3, 5, 7), mode)
    print("unipc per-step", mode, combo_id(combo), n, worst)
    assert max(worst) < MODES[mode][3], worst
    assert nulls[0] == (True, True, True)                                       # first step: no corrector, first-order predictor
    dc = combo["disable_corrector"]
    if combo["solver_order"] == 2 and not dc:
        assert nulls[1] == (False, False, True) and nulls[2] == (False, False, False)      # order-1 corrector, then the full form
        assert nulls[n - 1] == (False, False, False)                            # last step: order-2 corrector + first-order predictor
    if len(dc) > 1:
        assert nulls[n - 1][0] and nulls[n - 1][2]                              # corrector off on the last step: x_last and m_prev1 are NULL


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (3, 5, 67), (1, 3), (1, 64)], ids=["2x105", "3x335", "elems3", "B1_elems64"])
def test_shapes_and_dtypes(shape, mode):
    """[3, 5, 67]: 1005 elements, the 4-wide and the 8-wide vector bodies and both scalar tails; 3 elements per sample: below every vector width; one sample of 64: no
    tail.  Five steps of an n = 16 run (first step, order-1 corrector, then the full second-order form), bh2 and bh1, epsilon and v prediction."""
    bound = MODES[mode][3]
    for kw in (dict(SD15_UNIPC_KWARGS), dict(SD15_UNIPC_KWARGS, solver_type="bh1", prediction_type="v_prediction")):
        worst, _ = per_step_errors(kw, 16, shape, mode, steps=5, seed=1)
        print("unipc shapes", shape, mode, kw.get("solver_type", "bh2"), worst)
        assert max(worst) < bound, worst


def test_x_last_in_place_is_bit_identical_and_empty_batch_is_a_no_op():
    torch.manual_seed(3)
    s = UniPCMultistepScheduler(**SD15_UNIPC_KWARGS)
    s.set_timesteps(8, device=DEV)
    for io, st in ((torch.float32, torch.float32), (torch.float16, torch.float32), (torch.float16, torch.float16)):
        shape = (3, 5, 67)
        x, xl = torch.randn(shape, device=DEV).to(st), torch.randn(shape, device=DEV).to(st)
        e, m0, m1 = (torch.randn(shape, device=DEV).to(io) for _ in range(3))
        out = abi_step(s, 3, x, e, None, 1.0, xl.clone(), m0, m1, io, st, 2, 2, True)
        xl_in = xl.clone()
        inp = abi_step(s, 3, x, e, None, 1.0, xl_in, m0, m1, io, st, 2, 2, True, inplace=True)
        assert inp[1] is xl_in and not torch.equal(xl_in, xl)
        for a, b in zip(out[:4], inp[:4]):
            assert (a is None and b is None) or torch.equal(a, b)
    # B = 0: nothing is launched, nothing is written
    z = torch.zeros(0, 4, 8, 8, device=DEV)
    m_out, x_c, x_out, _, _ = abi_step(s, 0, z, z, None, 1.0, z, z, z, torch.float32, torch.float32, 0, 1, False)
    assert x_out.shape == (0, 4, 8, 8)
    s.set_timesteps(4, device=DEV)
    assert s.step(z, s.timesteps[0], z, return_dict=False)[0].shape == (0, 4, 8, 8)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kw", [dict(SD15_UNIPC_KWARGS), dict(SD15_UNIPC_KWARGS, solver_type="bh1", disable_corrector=[2])], ids=["bh2", "bh1_dc2"])
def test_scheduler_step_free_running(kw):
    """UniPCMultistepScheduler.step keeps the state itself (two converted outputs, last_sample updated in place, the orders): 8 free-running fp32 steps with fused CFG
    against the oracle on the combined eps, < 2e-6 per step relative to a restart from the oracle's state (the errors of earlier steps are carried, so the bound is on
    the trajectory: 8 steps x 2e-6)."""
    rng = np.random.default_rng(6)
    shape, n = (3, 4, 16, 16), 8
    s, o = UniPCMultistepScheduler(**kw), UniPCOracle(**kw)
    s.set_timesteps(n, device=DEV); o.set_timesteps(n)
    x0 = rng.standard_normal(shape).astype(np.float32)
    xg, xo = cu(x0, torch.float32), x0
    ring = [torch.empty(shape, device=DEV) for _ in range(s.history_slots)]
    lp = torch.empty(shape, dtype=torch.float16, device=DEV)
    for i, t in enumerate(s.timesteps):
        eu = rng.standard_normal(shape).astype(np.float32)
        ec = (eu + 0.3 * rng.standard_normal(shape)).astype(np.float32)
        out = s.step(cu(ec, torch.float32), t, xg, eps_uncond=cu(eu, torch.float32), guidance_scale=3.0, eps_out=ring[i % 3], out_lp=lp)
        xg = out.prev_sample
        xo = o.step(so.cfg_combine(eu, ec, 3.0), xo)
        err = [rel_l2(xg.cpu().numpy(), xo), rel_l2(ring[i % 3].cpu().numpy(), o.last_converted()), rel_l2(s.last_sample.cpu().numpy(), o.corrected)]
        print("unipc scheduler free-running", i, err)
        assert max(err) < 2e-6 * (i + 1), (i, err)
        assert torch.equal(lp, xg.to(torch.float16)) and s.step_index == i + 1
    with pytest.raises(ValueError):
        s.step(cu(ec, torch.float32), s.timesteps[-1], xg)                      # past the last step
    # a caller that hands in a history entry the step still reads is refused
    s.set_timesteps(n, device=DEV)
    x = cu(x0, torch.float32)
    x = s.step(cu(ec, torch.float32), s.timesteps[0], x, eps_out=ring[0]).prev_sample
    with pytest.raises(ValueError):
        s.step(cu(ec, torch.float32), s.timesteps[1], x, eps_out=ring[0])
    with pytest.raises(RuntimeError):
        s.step(cu(ec, torch.float32).cpu(), s.timesteps[1], x)


# ---------------------------------------------------------------------------------------------------------------- engine
def engine_inputs(B, seed=43):
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()
    return pe, ne, noise


@pytest.mark.parametrize("n", [5, 8])
def test_engine_against_unet_oracle_and_ddim_comparator(n):
    """reduced UNet, B = 2, CFG 3, SD15_UNIPC_KWARGS: final latents against UNetOracle + the UniPC oracle in fp32 on the CPU, within the project's 1e-3 latent gate and
    within 1.5 x the error of DDIMBaselineScheduler on the same model, noise and n (the comparator rule of tests/test_dpm_gpu.py)."""
    from consolver_amd.baselines import DDIMBaselineScheduler
    from tests._models import get_oracle, get_unet
    unet, _ = get_unet(REDUCED, seed=5)
    B, g = 2, 3.0
    pe, ne, noise = engine_inputs(B)
    orc_u = get_oracle(REDUCED, seed=5)
    ctx = torch.cat([ne, pe]).float()

    def eps_oracle(x, t):
        e = orc_u(torch.from_numpy(np.concatenate([x, x]).astype(np.float32)), int(t), ctx).numpy()
        return so.cfg_combine(e[:B], e[B:], g)

    eng = SDSamplingEngine(unet, UniPCMultistepScheduler(**SD15_UNIPC_KWARGS), guidance_scale=g)
    got = eng.generate(pe.to(DEV), ne.to(DEV), latents=noise.to(DEV), num_inference_steps=n).float().cpu().numpy()
    o = UniPCOracle(**SD15_UNIPC_KWARGS)
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
    print(f"engine n={n}: unipc rel-L2 {err:.4e}, ddim comparator rel-L2 {err_d:.4e}, ratio {err / err_d:.3f}")
    assert np.isfinite(got).all()
    assert err <= 1e-3, err
    assert err <= 1.5 * err_d, (err, err_d)


@pytest.mark.parametrize("latents_dtype", [torch.float32, torch.float16], ids=["f32_state", "f16_state"])
def test_engine_graph_is_bit_identical_to_eager(latents_dtype):
    """nothing is sampled in this solver and last_sample keeps its address across set_timesteps: the captured generation is the eager one bit for bit, and so is its
    second replay; the engine's ring has history_slots = 3 entries."""
    from tests._models import get_unet
    unet, _ = get_unet(REDUCED, seed=5)
    B, n = 2, 8
    pe, ne, noise = [t.to(DEV) for t in engine_inputs(B, seed=44)]
    sch = UniPCMultistepScheduler(**SD15_UNIPC_KWARGS)
    eng = SDSamplingEngine(unet, sch, guidance_scale=3.0, latents_dtype=latents_dtype)
    eager = eng.generate(pe, ne, latents=noise, num_inference_steps=n).clone()
    assert len(eng._bufs["ring"]) == 3
    last = sch.last_sample.data_ptr()
    graph = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    again = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    assert eager.dtype == latents_dtype and bool(torch.isfinite(eager).all())
    assert torch.equal(eager, graph) and torch.equal(graph, again) and sch.last_sample.data_ptr() == last
    # without CFG the scheduler is handed the ring slot itself (no eps_out)
    eng1 = SDSamplingEngine(unet, UniPCMultistepScheduler(**SD15_UNIPC_KWARGS), guidance_scale=1.0, latents_dtype=latents_dtype)
    e1 = eng1.generate(pe, latents=noise, num_inference_steps=5).clone()
    g1 = eng1.generate(pe, latents=noise, num_inference_steps=5, use_graph=True).clone()
    assert bool(torch.isfinite(e1).all()) and torch.equal(e1, g1)


def test_cli_generate_solver_unipc(tmp_path):
    import os
    from consolver_amd import generate as gen
    from consolver_amd.synth import synthetic_vae_state_dict
    from consolver_amd.vae import HipAutoencoderKL
    from tests._models import get_unet
    unet, _ = get_unet(REDUCED, seed=5)
    vae = HipAutoencoderKL(dict(REDUCED), device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=6))
    d = str(tmp_path / "unipc")
    r = gen.main(["--out", d, "--synthetic", "2", "--steps", "8", "--batch-size", "2", "--solver", "unipc"], unet=unet, vae=vae)
    assert r["images"] == 2 and r["solver"] == "unipc" and r["use_conv"] is False
    assert sorted(f for f in os.listdir(d) if f.endswith(".png")) == ["0_00000000.png", "0_00000001.png"]
