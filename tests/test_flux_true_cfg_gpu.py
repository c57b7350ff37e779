"""FLUX-Kontext true classifier-free guidance on the GPU (edit_ppo/pipeline.py:937-969, 1100-1115): the combine kernel against fp64, the DiT's
latent-row broadcast against the materialised batch, the engine's off- and on-path, the loop against the reference's own schedulers
(tests/golden/flux_true_cfg.npz), the precision of the combine on the network, and the pipeline / driver surface.

Stated bounds (measured on an MI355X, + 10 %, also in DESIGN.md "FLUX-Kontext: true classifier-free guidance"):
  * golden replay, per-step relative L2 of the latents against the reference's three-rounding loop: GOLDEN_BOUND below (per scheduler);
  * the combined v from fp32 head outputs against the fp32 oracle's fp64 combine: F32_COMBINE_BOUND below."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import _lib as L
from consolver_amd import generate_flux as gf
from consolver_amd.flux import (HipFluxTransformer2DModel, FluxKontextSamplingEngine, pack_latents, prepare_latent_image_ids,
                                true_cfg_combine)
from consolver_amd.scheduling_fm import FlowMatchGeneralDiscreteScheduler
from consolver_amd.synth import synthetic_flux_state_dict
from consolver_amd.tables import calculate_shift

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(num_layers=2, num_single_layers=2, num_heads=4, joint_attention_dim=256)      # the SMALL DiT of tests/test_flux_gpu.py
NAMES = ("fmppo", "euler", "heun", "dpm-solver", "dpm-solver-multistep")

# measured maximum over the steps, per scheduler, + 10 %: see test_engine_two_forward_path_vs_reference_golden
GOLDEN_BOUND = {"fmppo": 9.4e-4, "euler": 8.7e-4, "heun": 1.42e-3, "dpm-solver": 1.39e-3, "dpm-solver-multistep": 2.11e-3}
# measured 2.855e-3, + 10 %: see test_combine_precision_on_the_network
F32_COMBINE_BOUND = 3.15e-3


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
def _ordered(t):
    """the dtype's bit patterns as integers that count representable values (adjacent values differ by 1)"""
    i = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).to(torch.int64)
    mask = 0x7fffffff if t.dtype == torch.float32 else 0x7fff
    return torch.where(i < 0, -(i & mask), i)


def _check_against_fp64(out, pos, neg, scale, what):
    want = (neg.double() + scale * (pos.double() - neg.double())).to(out.dtype)
    ulps = (_ordered(out) - _ordered(want)).abs()
    share = float((ulps > 0).double().mean())
    print(f"true_cfg_combine {what}: max ulp distance {int(ulps.max())}, differing share {share:.2e}")
    assert int(ulps.max()) <= 1 and share <= 1e-3, (what, int(ulps.max()), share)


PAIRS = [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16), (torch.float32, torch.bfloat16), (torch.float32, torch.float16),
         (torch.float32, torch.float32)]


@pytest.mark.parametrize("scale", [1.5, 4.0])
@pytest.mark.parametrize("n", [3 * 24 * 64, 8 * 5 + 3, 5])           # several blocks of vectors | vector body + tail | tail only
@pytest.mark.parametrize("idt,odt", PAIRS)
def test_combine_kernel_matches_fp64_rounded_once(idt, odt, n, scale):
    g = torch.Generator().manual_seed(n + int(10 * scale))
    pos = torch.randn(n, generator=g).to(idt).to(DEV)
    neg = (pos.float().cpu() + 0.3 * torch.randn(n, generator=g)).to(idt).to(DEV)           # |pos - neg| ~ 0.3 |pos|
    out = true_cfg_combine(pos, neg, scale, out_dtype=odt)
    assert out.dtype == odt and out.shape == pos.shape
    _check_against_fp64(out, pos, neg, scale, f"{idt} -> {odt} n={n} s={scale}")
    # pos == neg: out == pos, whatever the scale
    assert torch.equal(true_cfg_combine(pos, pos.clone(), scale, out_dtype=odt), pos.to(odt))
    assert torch.equal(true_cfg_combine(pos, pos.clone(), 7.5, out_dtype=odt), pos.to(odt))
    if idt == odt:                                                                            # out may be pos or neg when the element sizes are equal
        p2, n2 = pos.clone(), neg.clone()
        assert true_cfg_combine(p2, neg, scale, out=p2) is p2 and torch.equal(p2, out)
        assert true_cfg_combine(pos, n2, scale, out=n2) is n2 and torch.equal(n2, out)


@pytest.mark.parametrize("odt", [torch.bfloat16, torch.float16])
def test_combine_kernel_fp32_inputs_on_a_4_byte_boundary(odt):
    """the fp32 side of a mixed pair needs 4-byte alignment only: element loads instead of 16-byte ones, the same values"""
    n = 8 * 300 + 3
    g = torch.Generator().manual_seed(5)
    buf_p, buf_n = torch.randn(n + 1, generator=g).to(DEV), torch.randn(n + 1, generator=g).to(DEV)
    pos, neg = buf_p[1:], buf_n[1:]
    assert pos.data_ptr() % 16 == 4 and pos.is_contiguous()
    out = true_cfg_combine(pos, neg, 4.0, out_dtype=odt)
    _check_against_fp64(out, pos, neg, 4.0, f"fp32 (+4 B) -> {odt}")
    assert torch.equal(out, true_cfg_combine(pos.clone(), neg.clone(), 4.0, out_dtype=odt))
    with pytest.raises(RuntimeError):                                                          # the 16-bit side keeps the 16-byte rule
        true_cfg_combine(pos.to(odt).clone(), neg.to(odt).clone(), 4.0, out=torch.empty(n + 1, dtype=odt, device=DEV)[1:])


# ---------------------------------------------------------------------------------------------------------------- shared model
@pytest.fixture(scope="module")
def dit():
    m = HipFluxTransformer2DModel(dict(SMALL, dtype=torch.bfloat16), device=DEV)
    sd = synthetic_flux_state_dict(m.manifest(), seed=4)
    sd = {k: v.to(torch.bfloat16).float() for k, v in sd.items()}        # the oracle sees the same rounded weights
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(2)
    B = 2
    d = dict(m=m, sd=sd, B=B,
             lat=pack_latents(torch.randn(B, 16, 16, 32, generator=g)).to(torch.bfloat16).to(DEV),        # 8 x 16 packed grid: 128 tokens
             img=pack_latents(torch.randn(B, 16, 16, 32, generator=g)).to(torch.bfloat16).to(DEV),        # 128 reference tokens
             enc=torch.randn(B, 64, 256, generator=g).to(torch.bfloat16).to(DEV), pooled=torch.randn(B, 768, generator=g).to(torch.bfloat16).to(DEV),
             nenc=torch.randn(B, 64, 256, generator=g).to(torch.bfloat16).to(DEV), npooled=torch.randn(B, 768, generator=g).to(torch.bfloat16).to(DEV))
    d["ids"] = np.concatenate([prepare_latent_image_ids(8, 16), prepare_latent_image_ids(8, 16, first=1.0)], 0)
    d["txt_ids"] = np.zeros((64, 3), np.float32)
    return d


def _fmppo(B):
    sch = consolver_amd.FMPPOScheduler.from_pretrained("x", subfolder="scheduler", order_dim=2, scaler_dim=0, mu_dim=0,
                                                       factor_net_kwargs=dict(hidden_dim=64, num_actions=11))
    sch.factor_net.to(DEV)
    sch.factor_net.forced_action_idx = torch.zeros(B, 1, dtype=torch.long, device=DEV) + 3       # one index set for every step
    return sch


# ---------------------------------------------------------------------------------------------------------------- 2. row broadcast
@pytest.mark.parametrize("R", [1, 2])
def test_dit_broadcasts_latent_rows_bit_for_bit(dit, R):
    m, G = dit["m"], 2
    assert m.broadcasts_latent_rows
    lat, img = dit["lat"][:R], dit["img"][:R]
    enc = torch.cat([dit["enc"][:R], dit["nenc"][:R]]); pooled = torch.cat([dit["pooled"][:R], dit["npooled"][:R]])
    t = torch.full((G * R,), 0.9567, device=DEV); gd = torch.full((G * R,), 2.5, device=DEV)
    kw = dict(guidance=gd, pooled_projections=pooled, encoder_hidden_states=enc, txt_ids=dit["txt_ids"])
    for odt in (torch.bfloat16, torch.float32):
        got = m(lat, t, img_ids=dit["ids"], image_latents=img, out_dtype=odt, **kw)[0].clone()
        want = m(lat.repeat(G, 1, 1), t, img_ids=dit["ids"], image_latents=img.repeat(G, 1, 1), out_dtype=odt, **kw)[0].clone()
        assert got.shape == (G * R, 128, 64) and got.dtype == odt and torch.isfinite(got.float()).all()
        assert torch.equal(got, want), odt
        assert not torch.equal(got[:R], got[R:])                                              # the text rows differ
        # without reference-image tokens (the embedder's single-problem launch)
        got1 = m(lat, t, img_ids=dit["ids"][:128], out_dtype=odt, **kw)[0].clone()
        want1 = m(lat.repeat(G, 1, 1), t, img_ids=dit["ids"][:128], out_dtype=odt, **kw)[0].clone()
        assert got1.shape == (G * R, 128, 64) and torch.equal(got1, want1), odt


def test_dit_row_count_that_does_not_divide_raises(dit):
    m = dit["m"]
    enc3 = torch.cat([dit["enc"], dit["nenc"][:1]]); pooled3 = torch.cat([dit["pooled"], dit["npooled"][:1]])
    t = torch.full((3,), 0.9567, device=DEV)
    with pytest.raises(ValueError, match="multiple"):
        m(dit["lat"], t, guidance=t, pooled_projections=pooled3, encoder_hidden_states=enc3, txt_ids=dit["txt_ids"], img_ids=dit["ids"],
          image_latents=dit["img"])
    rc = L.lib().cs_flux_forward_joint_rows(m._h, L.ptr(dit["lat"]), 128, L.ptr(dit["img"]), 128, 2, 3, L.ptr(enc3), 64, L.ptr(pooled3.float()),
                                            L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), L.ptr(t), 0, None)
    assert rc == -2 and b"multiple" in L.lib().cs_last_error()                                 # CS_E_SHAPE before anything is launched


# ---------------------------------------------------------------------------------------------------------------- 3. engine, off
class _CountRows:
    """the transformer behind a wrapper that notes every forward's text rows"""

    def __init__(self, m):
        self._m, self.rows = m, []

    def __getattr__(self, k):
        return getattr(self._m, k)

    def __call__(self, *a, **kw):
        self.rows.append(kw["encoder_hidden_states"].shape[0])
        return self._m(*a, **kw)


def test_engine_off_path_is_the_unguided_loop(dit):
    B, n = dit["B"], 4
    tr = _CountRows(dit["m"])
    sch = _fmppo(B)
    eng = FluxKontextSamplingEngine(tr, sch, guidance_scale=2.5)
    args = (dit["lat"], dit["img"], dit["enc"], dit["pooled"])
    base = eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n).clone()
    assert tr.rows == [B] * n and sch.step_index == n
    for kw in (dict(true_cfg_scale=1.0, negative_prompt_embeds=dit["nenc"], negative_pooled_prompt_embeds=dit["npooled"]),
               dict(true_cfg_scale=4.0),
               dict(true_cfg_scale=4.0, negative_prompt_embeds=dit["nenc"]),                  # one of the two negative tensors is not enough (:937-940)
               dict(true_cfg_scale=4.0, true_cfg_dtype=torch.float32)):
        tr.rows.clear()
        out = eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, **kw)
        assert torch.equal(out, base), kw
        assert tr.rows == [B] * n and sch.step_index == n, kw


# ---------------------------------------------------------------------------------------------------------------- 4. engine, on
def _by_hand(dit, sch, n, scale, f32):
    """one broadcast forward, cs_true_cfg_combine, sch.step -- per step"""
    m, B, lat = dit["m"], dit["B"], dit["lat"]
    sch.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=calculate_shift(lat.shape[1], 256, 4096, 0.5, 1.15), device=DEV)
    sch.set_begin_index(0)
    sig = (sch.timesteps.to(torch.bfloat16) / 1000).to(torch.float32)
    enc2, pooled2 = torch.cat([dit["enc"], dit["nenc"]]), torch.cat([dit["pooled"], dit["npooled"]])
    gd = torch.full((2 * B,), 2.5, device=DEV)
    x, vs = lat, []
    for i, t in enumerate(sch.timesteps):
        both = m(x, sig[i:i + 1].expand(2 * B).contiguous(), guidance=gd, pooled_projections=pooled2, encoder_hidden_states=enc2, txt_ids=dit["txt_ids"],
                 img_ids=dit["ids"], image_latents=dit["img"], out_dtype=torch.float32 if f32 else torch.bfloat16)[0]
        assert both.dtype == (torch.float32 if f32 else torch.bfloat16) and both.shape == (2 * B, 128, 64)
        v = torch.empty(B, 128, 64, dtype=torch.bfloat16, device=DEV)
        L.check(L.lib().cs_true_cfg_combine(L.ptr(both[:B]), L.ptr(both[B:]), L.dtype_code(both.dtype), C.c_float(scale), L.ptr(v), L.CS_BF16,
                                            v.numel(), L.stream_ptr(v.device)))
        vs.append(v)
        x = sch.step(v, t, x, return_dict=False)[0]
    return x, vs


@pytest.mark.parametrize("cfg_dtype", [torch.float32, torch.bfloat16])
def test_engine_on_path_equals_forward_combine_step_by_hand(dit, cfg_dtype):
    B, n = dit["B"], 4
    tr = _CountRows(dit["m"])
    sch = _fmppo(B)
    eng = FluxKontextSamplingEngine(tr, sch, guidance_scale=2.5)
    args = (dit["lat"], dit["img"], dit["enc"], dit["pooled"])
    neg = dict(negative_prompt_embeds=dit["nenc"], negative_pooled_prompt_embeds=dit["npooled"], true_cfg_scale=4.0, true_cfg_dtype=cfg_dtype)
    unguided = eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n).clone()
    tr.rows.clear()
    out = eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, **neg).clone()
    assert tr.rows == [2 * B] * n and sch.step_index == n                                     # ONE forward of [prompt | negative] rows per step
    assert out.shape == unguided.shape and out.dtype == torch.bfloat16 and torch.isfinite(out.float()).all()
    assert float((out.float() - unguided.float()).abs().mean()) > 1e-3
    want, vs = _by_hand(dit, sch, n, 4.0, cfg_dtype == torch.float32)
    assert torch.equal(out, want)
    if cfg_dtype == torch.float32:                                                             # None = fp32 on the HIP model's split stream
        assert torch.equal(eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, **dict(neg, true_cfg_dtype=None)), want)
    # records: the usual shapes, and the history holds the COMBINED v
    out2, conds, probs, actions, masks = eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, record=True, **neg)
    assert torch.equal(out2, want)
    assert conds["x"].shape == (B, n - 1, 2) and conds["epsilon"].shape == (B, n - 1, 2, 128, 64)
    assert probs.shape == actions.shape == masks.shape == (B, n - 1, 1)
    assert torch.equal(conds["epsilon"][:, 0, 0], vs[1])


def test_engine_true_cfg_dtype_errors_and_foreign_callable(dit):
    B, n = dit["B"], 2
    args = (dit["lat"], dit["img"], dit["enc"], dit["pooled"])
    neg = dict(negative_prompt_embeds=dit["nenc"], negative_pooled_prompt_embeds=dit["npooled"], true_cfg_scale=4.0)
    m = dit["m"]
    eng = FluxKontextSamplingEngine(m, gf.make_scheduler("euler"), guidance_scale=2.5)
    with pytest.raises(ValueError, match="true_cfg_dtype"):
        eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, true_cfg_dtype=torch.float16, **neg)
    one = eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, true_cfg_dtype=torch.bfloat16, **neg).clone()
    # a callable that does not broadcast latent rows gets two forwards per step; no fp32 there
    rows = []

    def foreign(*a, **kw):
        rows.append(kw["encoder_hidden_states"].shape[0])
        return m(*a, **kw)
    eng2 = FluxKontextSamplingEngine(foreign, gf.make_scheduler("euler"), guidance_scale=2.5)
    two = eng2.generate(*args, latent_hw=(8, 16), num_inference_steps=n, **neg)
    assert rows == [B] * (2 * n)
    # same arithmetic per row; the batch of the GEMMs differs (2 B rows against B), so only closeness is asserted: two bf16 roundings apart at most
    assert rel_l2(two.float(), one.float()) < 2e-2
    with pytest.raises(ValueError, match="float32"):
        eng2.generate(*args, latent_hw=(8, 16), num_inference_steps=n, true_cfg_dtype=torch.float32, **neg)
    m.set_residual_precision("plain")
    try:
        with pytest.raises(ValueError, match="float32"):
            eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, true_cfg_dtype=torch.float32, **neg)
        out = eng.generate(*args, latent_hw=(8, 16), num_inference_steps=n, **neg)            # None: the model dtype on the one-plane stream
        assert torch.isfinite(out.float()).all()
    finally:
        m.set_residual_precision("split")


# ---------------------------------------------------------------------------------------------------------------- 5. reference golden
class _ClosedFormDiT:
    """the two closed-form branches of tools/make_flux_true_cfg_golden.py in torch on the GPU; the branch is told by the sign of the text rows"""

    def __init__(self):
        self.seen = []

    def __call__(self, x, timestep, encoder_hidden_states=None, **_kw):
        negative = bool(encoder_hidden_states[0, 0, 0] < 0)
        if not negative:
            self.seen.append(x.float().cpu().numpy())
        th = torch.tanh(x.float())
        v = (0.7 * th - 0.05) if negative else (0.9 * th + 0.1 * timestep.float()[:, None, None])
        return (v.to(torch.bfloat16),)


@pytest.mark.parametrize("name", NAMES)
def test_engine_two_forward_path_vs_reference_golden(golden, name):
    """the loop of edit_ppo/pipeline.py:1074-1119 run with the reference's schedulers (the fixture) against engine.generate on the same closed-form
    branches.  The intended difference: the reference rounds `pos - neg`, `scale * d` and `neg + p` to bf16 each, this tree rounds the value once.
    Measured per-step relative L2 of the latents (MI355X), after steps 1, 2, 3, 4:
        fmppo                 1.81e-4  4.08e-4  5.94e-4  8.53e-4
        euler                 1.81e-4  3.14e-4  5.56e-4  7.85e-4
        heun                  4.42e-4  4.05e-4  1.29e-3  8.36e-4
        dpm-solver            1.81e-4  4.52e-4  5.50e-4  1.26e-3
        dpm-solver-multistep  1.81e-4  4.52e-4  8.40e-4  1.92e-3
    Every figure is below the 2e-3 (half a bf16 unit per element) above which something other than the roundings would differ; the differences add up
    along the trajectory and the multistep update's last step extrapolates them.  GOLDEN_BOUND: each scheduler's maximum + 10 %."""
    g = golden["flux_true_cfg"]
    lat = g[f"{name}_lat"]
    n, B = lat.shape[0] - 1, lat.shape[1]
    if name == "fmppo":
        sch = consolver_amd.FMPPOScheduler(shift=3.0, use_dynamic_shifting=True, order_dim=2, scaler_dim=0, mu_dim=0,
                                           factor_net_kwargs=dict(hidden_dim=32, num_actions=11))
        sch.factor_net.load_state_dict({k[len("fmppo_w_"):]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith("fmppo_w_")})
        sch.factor_net.to(DEV)
        sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in g["fmppo_idx"]]
    else:
        sch = FlowMatchGeneralDiscreteScheduler(shift=3.0, use_dynamic_shifting=True, type=name)
    tr = _ClosedFormDiT()
    eng = FluxKontextSamplingEngine(tr, sch, guidance_scale=2.5)
    ones = torch.ones(B, 8, 16, dtype=torch.bfloat16, device=DEV)
    x0 = torch.from_numpy(lat[0]).to(torch.bfloat16).to(DEV)
    out = eng.generate(x0, None, ones, ones[:, 0], latent_hw=(4, 6), num_inference_steps=n, negative_prompt_embeds=-ones,
                       negative_pooled_prompt_embeds=-ones[:, 0], true_cfg_scale=float(g["scale"]), true_cfg_dtype=torch.bfloat16)
    np.testing.assert_allclose(sch.sigmas.cpu().numpy(), g[f"{name}_sigmas"], rtol=2e-7)
    assert len(tr.seen) == n and sch.step_index == n
    traj = tr.seen[1:] + [out.float().cpu().numpy()]                  # the latents after steps 1 .. n
    errs = [float(np.linalg.norm(traj[i].astype(np.float64) - lat[i + 1]) / np.linalg.norm(lat[i + 1].astype(np.float64))) for i in range(n)]
    print(f"true CFG vs the reference's loop, {name}: per-step rel L2 " + " ".join(f"{e:.3e}" for e in errs))
    assert np.array_equal(tr.seen[0], lat[0])
    assert max(errs) < GOLDEN_BOUND[name], (name, errs)


# ---------------------------------------------------------------------------------------------------------------- 6. precision
def test_combine_precision_on_the_network(dit):
    """SMALL DiT, one forward pair, s = 4: the combined v (bf16) from the head's fp32 outputs and from its bf16 outputs, against the fp32 FluxOracle
    run on both text rows and combined in fp64.  Measured (MI355X): err_f32 2.855e-3, err_bf16 4.210e-3 (relative L2; both results end in one bf16
    rounding) -> fp32 stays the default where the split stream can deliver it; F32_COMBINE_BOUND = err_f32 + 10 %."""
    from oracle.flux_oracle import FluxOracle
    m, s = dit["m"], 4.0
    lat, img = dit["lat"][:1], dit["img"][:1]
    enc = torch.cat([dit["enc"][:1], dit["nenc"][:1]]); pooled = torch.cat([dit["pooled"][:1], dit["npooled"][:1]])
    t = torch.full((2,), 0.9567); gd = torch.full((2,), 2.5)
    kw = dict(guidance=gd.to(DEV), pooled_projections=pooled, encoder_hidden_states=enc, txt_ids=dit["txt_ids"], img_ids=dit["ids"], image_latents=img)
    v32 = m(lat, t.to(DEV), out_dtype=torch.float32, **kw)[0].clone()
    v16 = m(lat, t.to(DEV), out_dtype=torch.bfloat16, **kw)[0].clone()
    got32 = true_cfg_combine(v32[:1], v32[1:], s, out_dtype=torch.bfloat16)
    got16 = true_cfg_combine(v16[:1], v16[1:], s)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    hs = torch.cat([lat, img], 1).float().cpu().repeat(2, 1, 1)
    want = FluxOracle(dit["sd"], m.config)(hs, t, gd, pooled.float().cpu(), enc.float().cpu(), dit["txt_ids"], dit["ids"])[:, :128].double()
    want = want[1:] + s * (want[:1] - want[1:])
    err_f32, err_bf16 = rel_l2(got32, want), rel_l2(got16, want)
    print(f"true CFG combine on the SMALL DiT, s = {s}: from fp32 heads {err_f32:.3e}, from bf16 heads {err_bf16:.3e}")
    assert err_f32 < err_bf16, (err_f32, err_bf16)
    assert err_f32 <= F32_COMBINE_BOUND, err_f32


# ---------------------------------------------------------------------------------------------------------------- 7. pipeline, driver
@pytest.fixture(scope="module")
def small_vae():
    from consolver_amd.vae import HipAutoencoderKL, FLUX_VAE_CONFIG
    from consolver_amd.synth import synthetic_vae_state_dict
    vcfg = dict(FLUX_VAE_CONFIG); vcfg.update(layers_per_block=1, sample_size=16, with_encoder=True)
    vae = HipAutoencoderKL(vcfg, device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=9))
    return vae


def test_pipeline_honours_the_negative_prompt_arguments(dit, small_vae):
    from PIL import Image
    from consolver_amd.pipeline import FluxKontextEditPipeline
    from consolver_amd.synth import synthetic_clip_state_dict
    from consolver_amd.text_encoder import HipCLIPTextModel, HipT5EncoderModel
    from consolver_amd.vae import encode_image_latents, flux_decode_latents
    m, vae = dit["m"], small_vae
    clip = HipCLIPTextModel(dict(num_hidden_layers=1, vocab_size=500), device=DEV)
    clip.load_state_dict(synthetic_clip_state_dict(clip.manifest(), seed=2))
    t5 = HipT5EncoderModel(dict(num_layers=1, vocab_size=300, d_model=256, num_heads=4, d_ff=512), device=DEV)
    g = torch.Generator().manual_seed(3)
    t5.load_state_dict({n: (1.0 + 0.1 * torch.randn(s, generator=g)) if n.endswith("layer_norm.weight") else torch.randn(s, generator=g) * (0.5 / s[-1] ** 0.5)
                        for n, s in t5.manifest()})
    pipe = FluxKontextEditPipeline(m, gf.make_scheduler("euler"), vae, text_encoder=clip, text_encoder_2=t5)
    ref = Image.fromarray(np.random.default_rng(0).integers(0, 255, (90, 120, 3), dtype=np.uint8))
    ids_t5, nids_t5 = torch.randint(0, 300, (1, 64), generator=g), torch.randint(0, 300, (1, 64), generator=g)
    ids_clip, nids_clip = torch.randint(0, 499, (1, 77), generator=g), torch.randint(0, 499, (1, 77), generator=g)
    ids_clip[:, -1] = 499; nids_clip[:, -1] = 499
    call = lambda **kw: pipe(image=ref, input_ids_t5=ids_t5, input_ids_clip=ids_clip, num_inference_steps=3, guidance_scale=2.5,
                             generator=torch.manual_seed(0), output_type="pt", **kw).images.clone()
    plain = call()
    guided = call(negative_input_ids_t5=nids_t5, negative_input_ids_clip=nids_clip, true_cfg_scale=4)
    assert guided.shape == plain.shape == (1, 3, 128, 128) and torch.isfinite(guided).all()
    assert float((guided.float() - plain.float()).abs().mean()) > 1e-3
    assert torch.equal(call(true_cfg_scale=4), plain)                                          # no negative input: unguided, like the reference
    assert torch.equal(call(negative_input_ids_t5=nids_t5, negative_input_ids_clip=nids_clip), plain)        # scale 1: off
    # by hand: encode both prompts, engine.generate, decode
    pe, pooled, _ = pipe.encode_prompt(input_ids_t5=ids_t5, input_ids_clip=ids_clip)
    ne, npooled, _ = pipe.encode_prompt(input_ids_t5=nids_t5, input_ids_clip=nids_clip)
    assert torch.equal(call(negative_prompt_embeds=ne, negative_pooled_prompt_embeds=npooled, true_cfg_scale=4), guided)
    arr = np.asarray(ref.convert("RGB").resize((128, 128), Image.LANCZOS), dtype=np.uint8)
    image = (torch.from_numpy(arr.copy()).permute(2, 0, 1).float() / 255.0 * 2 - 1)[None].to(DEV, torch.float16)
    il = pack_latents(encode_image_latents(vae, image)).to(torch.bfloat16)
    noise = torch.randn(1, 16, 16, 16, generator=torch.manual_seed(0)).to(DEV)
    eng = FluxKontextSamplingEngine(m, gf.make_scheduler("euler"), guidance_scale=2.5)
    out = eng.generate(pack_latents(noise).to(torch.bfloat16), il, pe.to(torch.bfloat16), pooled.to(torch.bfloat16), latent_hw=(8, 8), num_inference_steps=3,
                       negative_prompt_embeds=ne.to(torch.bfloat16), negative_pooled_prompt_embeds=npooled.to(torch.bfloat16), true_cfg_scale=4.0)
    assert torch.equal(flux_decode_latents(vae, out.to(torch.float16), height=128, width=128), guided)
    # a negative prompt string cannot be encoded without tokenizers: the same error as `prompt`
    with pytest.raises(RuntimeError, match="tokenizers"):
        call(negative_prompt="x", true_cfg_scale=4)
    with pytest.raises(RuntimeError, match="tokenizers"):
        call(negative_prompt="x")


def test_driver_true_cfg_flag_changes_the_edits(dit, small_vae, tmp_path):
    from PIL import Image
    base = ["--synthetic", "2", "--steps", "2", "--solver", "euler"]                              # (a policy-free solver: the two runs differ by the flag alone)
    res0 = gf.main(base + ["--out", str(tmp_path / "plain")], transformer=dit["m"], vae=small_vae)
    res1 = gf.main(base + ["--out", str(tmp_path / "cfg"), "--true_cfg_scale", "4"], transformer=dit["m"], vae=small_vae)
    assert res0["edits"] == res1["edits"] == 2 and res0["true_cfg_scale"] == 1.0 and res1["true_cfg_scale"] == 4.0
    for key in ("synthetic_0", "synthetic_1"):
        a = np.asarray(Image.open(tmp_path / "plain" / "synthetic" / key / "edited_image.jpg").convert("RGB"), np.float32)
        b = np.asarray(Image.open(tmp_path / "cfg" / "synthetic" / key / "edited_image.jpg").convert("RGB"), np.float32)
        assert a.shape == b.shape == (128, 128, 3) and np.abs(a - b).mean() > 0.5
    # the negative prompt from a file: the same embedding gives the same images
    g = torch.Generator().manual_seed(2002)
    ne, npooled = torch.randn(1, 64, 256, generator=g), torch.randn(1, 768, generator=g)
    gf.save_negative_embeds(str(tmp_path / "neg.safetensors"), ne[0], npooled[0])
    res2 = gf.main(base + ["--out", str(tmp_path / "file"), "--true_cfg_scale", "4", "--negative-embeds", str(tmp_path / "neg.safetensors")],
                   transformer=dit["m"], vae=small_vae)
    assert res2["edits"] == 2
    for key in ("synthetic_0", "synthetic_1"):
        b = np.asarray(Image.open(tmp_path / "cfg" / "synthetic" / key / "edited_image.jpg").convert("RGB"))
        c = np.asarray(Image.open(tmp_path / "file" / "synthetic" / key / "edited_image.jpg").convert("RGB"))
        assert np.array_equal(b, c)
