"""CPU-side checks of the FLUX flow-matching baselines (scheduling_fm.py): the schedule and the host step plan against the reference's own
output (tests/golden/flux_fm_baselines.npz, tools/make_fm_baseline_golden.py), the argument errors of cs_fm_general_step, the scheduler
factory, and the FLUX teacher-pair dataset."""
import ctypes
import os

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import _lib, ppo_data
from consolver_amd import generate_flux as gf
from consolver_amd.scheduling_fm import FM_SOLVER_TYPES, FlowMatchGeneralDiscreteScheduler

CASES = [(typ, dt, n) for typ in FM_SOLVER_TYPES for dt in ("f32", "bf16") for n in (4, 5)]


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make(typ, n, device=None):
    s = FlowMatchGeneralDiscreteScheduler(shift=3.0, use_dynamic_shifting=True, type=typ)
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=1.15, device=device)
    s.set_begin_index(0)
    return s


def numpy_step(s, x, v):
    """one step of ``s`` on numpy arrays in fp32: the plan applied by hand, the state kept through commit_plan"""
    if s.step_index is None:
        s._init_step_index(s.timesteps[0])
    p = s.step_plan()
    base = x if p.base == "sample" else s.prev_sample
    w = (s.prev_model_output + v).astype(np.float32) if p.use_v1 else v
    out = (base + (np.float32(p.c) * w).astype(np.float32)).astype(np.float32)
    s.commit_plan(p, x, v)
    return out


@pytest.mark.parametrize("typ,dt,n", CASES)
def test_schedule_tables_bit_exact(golden, typ, dt, n):
    g, k = golden["flux_fm_baselines"], f"{typ}_{dt}_n{n}"
    s = make(typ, n)
    assert s.sigmas.dtype == torch.float32 and np.array_equal(s.sigmas.numpy(), g[f"{k}_sigmas"])
    assert s.timesteps.dtype == torch.float32 and np.array_equal(s.timesteps.numpy(), g[f"{k}_timesteps"])
    assert s.num_inference_steps == n and s.step_index is None and s.begin_index == 0


@pytest.mark.parametrize("typ,n", [(typ, n) for typ in FM_SOLVER_TYPES for n in (4, 5)])
def test_step_plan_in_numpy_reproduces_every_fp32_golden_step(golden, typ, n):
    g, k = golden["flux_fm_baselines"], f"{typ}_f32_n{n}"
    assert tuple(g["shape"]) == (3, 5, 67) and list(g["types"]) == list(FM_SOLVER_TYPES)
    s = make(typ, n)
    for i in range(n):
        x, v = g[f"{k}_s{i}_x"], g[f"{k}_s{i}_v"]
        got = numpy_step(s, x, v)
        err = rel_l2(got, g[f"{k}_s{i}_prev"])
        print(k, i, err)
        assert err < 1e-6, (k, i, err)
        if i + 1 < n:
            assert np.array_equal(g[f"{k}_s{i + 1}_x"], g[f"{k}_s{i}_prev"])       # the golden is one trajectory
    assert s.step_index == n


def test_step_plan_rows():
    """which base, whether v1 is read, c and what is kept, per type (scheduler_fm.py:405-482), incl. the idx + 2 clamp at odd n"""
    f = np.float32
    for n in (4, 5):
        sig = make("euler", n)._sigmas
        plans = {}
        for typ in FM_SOLVER_TYPES:
            s = make(typ, n)
            s._init_step_index(None)
            plans[typ] = []
            for i in range(n):
                p = s.step_plan()
                plans[typ].append(p)
                s.commit_plan(p, ("x", i), ("v", i))
                assert isinstance(p.c, np.float32)
        d = [f(sig[i + 1] - sig[i]) for i in range(n)]
        assert [(p.base, p.use_v1, p.c, p.save) for p in plans["euler"]] == [("sample", False, d[i], None) for i in range(n)]
        for i, p in enumerate(plans["heun"]):
            if i % 2 == 0:
                two = f(sig[min(i + 2, n)] - sig[i])
                assert (p.base, p.use_v1, p.c, p.save, p.dt) == ("sample", False, two, "all", two)
            else:
                assert (p.base, p.use_v1, p.c, p.save) == ("saved", True, f(f(0.5) * plans["heun"][i - 1].dt), None)
        for i, p in enumerate(plans["dpm-solver"]):
            want = ("sample", False, d[i], "all") if i % 2 == 0 else ("saved", False, f(d[i - 1] + d[i]), None)
            assert (p.base, p.use_v1, p.c, p.save) == want
        for i, p in enumerate(plans["dpm-solver-multistep"]):
            want = ("sample", False, d[0], "all", d[0]) if i == 0 else ("saved", False, f(d[i - 1] + d[i]), "sample", d[i])
            assert tuple(p) == want
    # the state is references to what the caller passed, and set_timesteps drops it
    s = make("dpm-solver-multistep", 4)
    x0, v0, x1, v1 = object(), object(), object(), object()
    s._init_step_index(None)
    s.commit_plan(s.step_plan(), x0, v0)
    assert s.prev_sample is x0 and s.prev_model_output is v0
    s.commit_plan(s.step_plan(), x1, v1)
    assert s.prev_sample is x1 and s.prev_model_output is v0 and s.step_index == 2
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / 4, 4), mu=1.15)
    assert s.prev_sample is None and s.prev_model_output is None and s.prev_dt is None and s.step_index is None
    # a second stage without its first stage (a run that starts mid-pair) is an error, not a read of stale state
    s = make("heun", 4)
    s.set_begin_index(1)
    s._init_step_index(None)
    with pytest.raises(ValueError, match="second stage"):
        s.step_plan()


def test_scheduler_protocol_and_config():
    s = FlowMatchGeneralDiscreteScheduler.from_pretrained("black-forest-labs/FLUX.1-Kontext-dev", subfolder="scheduler", type="heun")
    assert s.type == "heun" and s.config.type == "heun" and s.config.shift == 3.0 and s.config.use_dynamic_shifting
    assert len(s) == 1000 and s.order == 1 and s.step_index is None
    assert consolver_amd.FlowMatchGeneralDiscreteScheduler is FlowMatchGeneralDiscreteScheduler
    with pytest.raises(ValueError, match="mu"):
        s.set_timesteps(4)
    with pytest.raises(ValueError, match="unknown type"):
        FlowMatchGeneralDiscreteScheduler(type="rk4")
    with pytest.raises(ValueError, match="set_timesteps"):
        s.step(None, 0.0, None)
    s = make("euler", 4)
    with pytest.raises(RuntimeError, match="CUDA"):          # no CPU path
        s.step(torch.zeros(1, 8), s.timesteps[0], torch.zeros(1, 8))
    # scale_noise: the forward process on the run's sigma table
    x, noise = torch.ones(2, 3), torch.full((2, 3), 3.0)
    sig = s.sigmas[1]
    s2 = make("euler", 4)
    s2.set_begin_index(1)
    assert torch.allclose(s2.scale_noise(x, s2.timesteps[1:2].repeat(2), noise), sig * noise + (1 - sig) * x)
    # a static-shift config works without mu
    s = FlowMatchGeneralDiscreteScheduler(shift=3.0, type="dpm-solver")
    s.set_timesteps(5)
    assert s.sigmas.shape == (6,) and float(s.sigmas[-1]) == 0.0


def test_fm_general_step_argument_errors():
    """argument validation happens before any launch -> usable without a GPU"""
    if not os.path.exists(_lib.LIB_PATH):
        from consolver_amd.build import build
        build()
    l = _lib.lib()
    assert ctypes.sizeof(_lib.CsFmStepArgs) == 3 * 8 + 4 + 4 + 8 + 3 * 4 + 4 + 8
    assert l.cs_fm_general_step(None, None) == -1 and b"NULL" in l.cs_last_error()
    a = _lib.CsFmStepArgs()
    a.B, a.elems = 1, 8
    assert l.cs_fm_general_step(ctypes.byref(a), None) == -1 and b"required" in l.cs_last_error()
    a.x_base = a.v2 = a.x_out = 64
    a.io_dtype, a.out_dtype = _lib.CS_F32, _lib.CS_BF16
    assert l.cs_fm_general_step(ctypes.byref(a), None) == -3 and b"dtype pair" in l.cs_last_error()
    a.io_dtype, a.out_dtype = _lib.CS_U8, _lib.CS_U8
    assert l.cs_fm_general_step(ctypes.byref(a), None) == -3
    a.io_dtype, a.out_dtype = _lib.CS_BF16, _lib.CS_BF16
    a.v2 = 66                                                       # a 16-bit tensor that is not 16-byte aligned
    assert l.cs_fm_general_step(ctypes.byref(a), None) == -1 and b"aligned" in l.cs_last_error()
    a.v2, a.B = 64, -1
    assert l.cs_fm_general_step(ctypes.byref(a), None) == -2
    a.B, a.elems = 0, 8
    assert l.cs_fm_general_step(ctypes.byref(a), None) == 0         # an empty batch is a no-op
    a.B, a.elems = 3, 0
    assert l.cs_fm_general_step(ctypes.byref(a), None) == 0
    a.x_base = a.v2 = a.x_out = None
    assert l.cs_fm_general_step(ctypes.byref(a), None) == 0         # ... whatever the pointers


def test_flux_solvers_and_make_scheduler():
    assert gf.FLUX_SOLVERS == ("consistencysolver", "euler", "heun", "dpm-solver", "dpm-solver-multistep")
    for solver in gf.FLUX_SOLVERS[1:]:
        s = gf.make_scheduler(solver)
        assert type(s) is FlowMatchGeneralDiscreteScheduler and s.type == solver and not hasattr(s, "factor_net")
        assert s.config.shift == 3.0 and s.config.use_dynamic_shifting and s.config.max_shift == 1.15
        with pytest.raises(ValueError, match="no policy"):
            gf.make_scheduler(solver, order_dim=2)
    s = gf.make_scheduler("consistencysolver")
    assert type(s) is consolver_amd.FMPPOScheduler and s.config.order_dim == 2 and s.config.scaler_dim == 0 and s.factor_net.num_actions == 11
    s = gf.make_scheduler("consistencysolver", order_dim=3, factor_net_kwargs=dict(hidden_dim=16, num_actions=5))
    assert s.config.order_dim == 3 and s.factor_net.num_actions == 5
    with pytest.raises(ValueError, match="unknown solver"):
        gf.make_scheduler("ddim")


def _write_pair(root, i, rng, size=(24, 40), latent=None):
    from PIL import Image
    for d in ppo_data.FLUX_PAIR_DIRS.values():
        os.makedirs(os.path.join(root, d), exist_ok=True)
    edited, ref = rng.integers(0, 255, size + (3,), dtype=np.uint8), rng.integers(0, 255, (30, 30, 3), dtype=np.uint8)
    Image.fromarray(edited).save(os.path.join(root, "edited_images", f"{i}.png"))
    Image.fromarray(ref).save(os.path.join(root, "ref_images", f"{i}.png"))
    with open(os.path.join(root, "prompts", f"{i}.txt"), "w") as f:
        f.write(f"  make it {i}\n")
    g = torch.Generator().manual_seed(i)
    noise = torch.randn(1, 6, 64, generator=g).to(torch.bfloat16)
    latent = torch.randn(1, 6, 64, generator=g).to(torch.bfloat16) if latent is None else latent
    torch.save(noise, os.path.join(root, "initial_noises", f"{i}.pt"))
    torch.save(latent, os.path.join(root, "obtained_noises", f"{i}.pt"))
    return edited, ref, noise, latent


def test_flux_teacher_pair_dataset_round_trip(tmp_path):
    from PIL import Image
    root, rng = str(tmp_path), np.random.default_rng(0)
    edited, ref, noise, latent = _write_pair(root, 0, rng)
    _write_pair(root, 1, rng, latent=torch.full((1, 6, 64), float("nan")).to(torch.bfloat16))      # a broken item: NaN latents
    _write_pair(root, 2, rng)
    os.remove(os.path.join(root, "prompts", "2.txt"))                                               # a broken item: no prompt
    ds = ppo_data.FluxTeacherPairDataset(root, (16, 24))
    assert len(ds) == 3 and ds.img_names == ["0.png", "1.png", "2.png"]
    image, text, n0, l0, r0 = ds[0]
    assert text == "make it 0" and image.shape == r0.shape == (3, 16, 24) and image.dtype == r0.dtype == torch.float32
    assert n0.shape == l0.shape == (6, 64) and n0.dtype == torch.bfloat16 and torch.equal(n0, noise[0]) and torch.equal(l0, latent[0])
    want = np.asarray(Image.fromarray(edited).resize((24, 16), Image.LANCZOS), np.float32) / 255.0
    assert torch.allclose(image, torch.from_numpy(want).permute(2, 0, 1) * 2 - 1, rtol=0, atol=1e-6)      # (x - 0.5) / 0.5 against 2 x - 1: an ulp
    want = np.asarray(Image.fromarray(ref).resize((24, 16), Image.LANCZOS), np.float32) / 255.0
    assert torch.equal(r0, torch.from_numpy(want).permute(2, 0, 1)) and 0.0 <= float(r0.min()) and float(r0.max()) <= 1.0
    assert -1.0 <= float(image.min()) and float(image.max()) <= 1.0
    for broken in (1, 2):                                    # retried on a random index until item 0 comes up
        got = ds[broken]
        assert got[1] == "make it 0" and torch.equal(got[3], latent[0])
    strict = ppo_data.FluxTeacherPairDataset(root, (16, 24), strict=True)
    with pytest.raises(ValueError, match="NaN"):
        strict[1]
    with pytest.raises(FileNotFoundError):
        strict[2]
    # an int size is a square
    assert ppo_data.FluxTeacherPairDataset(root, 8)[0][0].shape == (3, 8, 8)


def test_repeat_random_sample_flux():
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(3, 3, 4, 4, generator=g), ["a", "b", "c"], torch.randn(3, 6, 64, generator=g), torch.randn(3, 6, 64, generator=g),
             torch.rand(3, 3, 4, 4, generator=g))
    image, text, noise, tch, ref, i = ppo_data.repeat_random_sample_flux(batch, return_index=True)
    assert 0 <= i < 3 and text == [batch[1][i]] * 3
    for got, src in ((image, batch[0]), (noise, batch[2]), (tch, batch[3]), (ref, batch[4])):
        assert got.shape == src.shape and all(torch.equal(got[j], src[i]) for j in range(3))
    out = ppo_data.repeat_random_sample_flux(batch, index=2)
    assert len(out) == 5 and out[1] == ["c"] * 3 and torch.equal(out[4][0], batch[4][2])
