"""GPU tests of DEISMultistepScheduler and PNDMScheduler (iPNDM): ``step`` around cs_linear_step, and SDSamplingEngine with both.

Trajectories.  The model outputs are fixed seeded tensors per forward, not functions of the sample, so chaining tests/lin_ref.py's ``lin_exact`` (the fp32 replica
of the kernel's operation order) on the CPU with the schedulers' own host scalars reproduces every step BIT FOR BIT: the sample, the history entry (the combined
eps, or the converted output under v prediction) and the 16-bit copy, in fp16 / fp16 and with an fp32 state beside fp16 outputs, with and without CFG, all n steps
of DEIS at orders 2 and 3 and all n + 1 forwards of iPNDM, whose history lives in a ring of ``history_slots`` buffers as in the engine.  The scalars themselves
are held to the independent oracles on the CPU (tests/test_deis_oracle.py, tests/test_pndm_oracle.py).

Engine, on the suite's reduced UNet: ``generate`` equals a hand-written loop over ``scheduler.timesteps`` (torch.equal), runs n forwards for DEIS and n + 1 for
iPNDM, and its captured graph replays to the eager result bit for bit; a UniPC run through the changed loop is still the hand-driven ``step`` sequence.

Shown to bite with three scratch mutants (not committed) on an MI355X, the two of solver.hip run against tests/test_lin_step_gpu.py and this module (59 tests), the
scheduler's against this module (38):
    c[2] and c[3] swapped in lin_one (solver.hip): 35 tests fail -- all 17 of test_lin_dtype_forms, test_lin_grid_stride and the m_out test there (at terms = 3 the
        test hands over NaN as c[3]); here the order-3, n = 8 DEIS trajectories in every mode, both v-prediction ones and every iPNDM trajectory (four terms from forward 4 on);
    x_base ignored in LinStep::step (solver.hip): 28 tests fail -- all 17 of test_lin_dtype_forms and test_lin_grid_stride there; here every iPNDM trajectory (at forward 1)
        and the ring-of-four test, which runs the first four forwards; every DEIS test passes, as it must;
    PNDMScheduler.step appending the second forward's output to its history: 10 tests fail -- every iPNDM trajectory and the ring-of-four test, at forward 1, where the
        scheduler's history has two entries against the chain's one (without that check, at forward 2, which would combine three outputs instead of two); the engine
        tests pass, as both sides of their comparison run the mutant.
"""
import numpy as np
import pytest
import torch

from consolver_amd import (SD15_DEIS_KWARGS, SD15_PNDM_KWARGS, SD15_UNIPC_KWARGS, DEISMultistepScheduler, PNDMScheduler, UniPCMultistepScheduler)
from consolver_amd.engine import SDSamplingEngine
from consolver_amd.synth import synthetic_prompt_embeds
from tests import lin_ref as LR
from tests import solver_ref as R
from tests.test_solver_forms_gpu import DEV, TD, dev

pytestmark = pytest.mark.gpu
REDUCED = dict(layers_per_block=1, sample_size=16)
SHAPES = [(2, 4, 8, 8), (3, 4, 5, 7)]
# (io dtype, state dtype, 16-bit copy)
MODES = {"f16": ("f16", "f16", None), "f32_state_f16_eps_lp": ("f16", "f32", "f16")}
G = 3.0


def same(t, a):
    """a device tensor holds exactly the values of the numpy array [B, elems]"""
    return torch.equal(t.float().cpu().reshape(a.shape), torch.from_numpy(a))


def case(io, st, lp, x, xb, ec, eu, hist, scal):
    return dict(io=io, out=st, x_is_f32=int(st == "f32" and io != "f32"), lp=lp, terms=len(hist) + 1, x=x, xb=xb, ec=ec, eu=eu, g=G if eu is not None else 1.0,
                hist=hist, scal=scal, want_m_out=True)


class Trajectory:
    """the device side of one run: the sample, the ring of history buffers, the 16-bit copy; ``step`` drives scheduler.step and compares with lin_exact's outputs"""

    def __init__(self, sch, shape, mode, cfg, name, slots=None):
        self.io, self.st, self.lp = MODES[mode]
        self.sch, self.shape, self.cfg = sch, shape, cfg
        self.B, self.elems = shape[0], int(np.prod(shape[1:]))
        self.rng = np.random.default_rng(R._seed(name))
        self.x = R.tensor(self.rng, self.B, self.elems, self.st)
        self.xg = dev(self.x, self.st).view(shape)
        self.ring = [torch.empty(shape, dtype=TD[self.io], device=DEV) for _ in range(slots or sch.history_slots)]
        self.lpbuf = torch.empty(shape, dtype=TD[self.lp], device=DEV) if self.lp else None

    def outputs(self):
        ec = R.tensor(self.rng, self.B, self.elems, self.io)
        return ec, (R.tensor(self.rng, self.B, self.elems, self.io) if self.cfg else None)

    def step(self, i, t, ec, eu, want, use_slot):
        slot = self.ring[i % len(self.ring)] if use_slot else None
        out = self.sch.step(dev(ec, self.io).view(self.shape), t, self.xg, eps_uncond=dev(eu, self.io).view(self.shape) if eu is not None else None,
                            guidance_scale=G if eu is not None else 1.0, eps_out=slot, out_lp=self.lpbuf)
        self.xg = out.prev_sample
        assert self.xg.dtype == TD[self.st] and same(self.xg, want["x_out"]), (i, "sample")
        if use_slot:
            assert same(slot, want["m_out"]), (i, "history entry")
        if self.lp:
            assert same(self.lpbuf, want["x_out_lp"]), (i, "16-bit copy")
        self.x = want["x_out"]


def deis_run(shape, mode, cfg, order, n, pred="epsilon"):
    s = DEISMultistepScheduler(**dict(SD15_DEIS_KWARGS, solver_order=order, prediction_type=pred))
    s.set_timesteps(n, device=DEV)
    tr = Trajectory(s, shape, mode, cfg, f"deis-{shape}-{mode}-{cfg}-{order}-{n}-{pred}")
    hist, orders = [], []
    for i, t in enumerate(s.timesteps):
        ec, eu = tr.outputs()
        conv_x, conv_e, cx, cs = s.step_scalars(i)
        orders.append(len(cs))
        want = LR.lin_exact(case(tr.io, tr.st, tr.lp, tr.x, None, ec, eu, hist[:len(cs) - 1], (conv_x, conv_e, cx, cs)))
        tr.step(i, t, ec, eu, want, use_slot=bool(cfg or pred != "epsilon"))
        hist = [want["m_out"]] + hist
        assert s.step_index == i + 1
    with pytest.raises(ValueError):
        s.step(tr.xg.to(TD[tr.io]), s.timesteps[-1], tr.xg)                       # past the last step
    return orders


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("cfg", [0, 1], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("mode", list(MODES))
def test_deis_trajectory_bit_for_bit(mode, cfg, order, n):
    for shape in SHAPES:
        orders = deis_run(shape, mode, cfg, order, n)
    assert orders == {(2, 4): [1, 2, 2, 1], (3, 4): [1, 2, 2, 1], (2, 8): [1, 2, 2, 2, 2, 2, 2, 1], (3, 8): [1, 2, 3, 3, 3, 3, 2, 1]}[(order, n)]


@pytest.mark.parametrize("mode", list(MODES))
def test_deis_v_prediction_trajectory_bit_for_bit(mode):
    """the conversion m = sigma x + alpha v runs in the kernel, and the history holds the converted outputs"""
    deis_run(SHAPES[1], mode, 1, 3, 8, pred="v_prediction")
    deis_run(SHAPES[1], mode, 0, 3, 8, pred="v_prediction")


def pndm_run(shape, mode, cfg, n, pred="epsilon", slots=None, forwards=None):
    s = PNDMScheduler(**dict(SD15_PNDM_KWARGS, prediction_type=pred))
    s.set_timesteps(n, device=DEV)
    assert len(s.timesteps) == n + 1
    tr = Trajectory(s, shape, mode, cfg, f"pndm-{shape}-{mode}-{cfg}-{n}-{pred}", slots)
    ets, cur = [], None
    for k, t in enumerate(s.timesteps[:forwards]):
        ec, eu = tr.outputs()
        cx, cs, restart = s.step_scalars(k)
        if k == 0:
            cur = tr.x
        hist = ets[::-1][:1] if restart else ets[::-1][:3]
        assert len(cs) == len(hist) + 1 and restart == (k == 1)
        want = LR.lin_exact(case(tr.io, tr.st, tr.lp, tr.x, cur if restart else None, ec, eu, hist, (0.0, 1.0, cx, cs)))
        tr.step(k, t, ec, eu, want, use_slot=bool(cfg))
        if not restart:                                                           # the second forward's output does not enter the history
            ets = ets[-3:] + [want["m_out"]]
        assert s.step_index == k + 1 and len(s.ets) == len(ets)
    return s, tr


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("cfg", [0, 1], ids=["nocfg", "cfg"])
@pytest.mark.parametrize("mode", list(MODES))
def test_pndm_trajectory_bit_for_bit(mode, cfg, n):
    """all n + 1 forwards; under CFG the history lives in a ring of history_slots = 5 buffers that forward i writes at i % 5, as in the engine"""
    for shape in SHAPES:
        s, tr = pndm_run(shape, mode, cfg, n)
        assert len(tr.ring) == 5
        with pytest.raises(ValueError):
            s.step(tr.xg.to(TD[tr.io]), s.timesteps[-1], tr.xg)                   # past the last forward


def test_pndm_v_prediction_trajectory_bit_for_bit():
    pndm_run(SHAPES[1], "f32_state_f16_eps_lp", 1, 8, pred="v_prediction")


def test_pndm_ring_of_four_is_refused_at_the_fifth_forward():
    """with four slots forward 4 would write the slot of forward 0, which it still reads: the scheduler refuses before any launch"""
    s, tr = pndm_run(SHAPES[0], "f16", 1, 8, slots=4, forwards=4)
    ec, eu = tr.outputs()
    keep = [m.clone() for m in tr.ring]
    with pytest.raises(ValueError, match="history_slots"):
        s.step(dev(ec, "f16").view(tr.shape), s.timesteps[4], tr.xg, eps_uncond=dev(eu, "f16").view(tr.shape), guidance_scale=G, eps_out=tr.ring[0])
    assert all(torch.equal(a, b) for a, b in zip(keep, tr.ring)) and s.step_index == 4


def test_pndm_timestep_is_checked_where_that_costs_no_device_read():
    s = PNDMScheduler(**SD15_PNDM_KWARGS)
    s.set_timesteps(8, device=DEV)
    x = torch.randn(2, 4, 8, 8, device=DEV, dtype=torch.float16)

    def e():
        return torch.randn_like(x)                                                # (a new tensor per forward: the history keeps references)
    with pytest.raises(ValueError):
        s.step(e(), s.timesteps[1], x)                                            # an element of scheduler.timesteps, but not forward 0's
    with pytest.raises(ValueError):
        s.step(e(), 751, x)                                                       # a host integer that is not forward 0's timestep
    assert s.step_index == 0
    x = s.step(e(), 876, x).prev_sample                                           # host integers pass where they are the counter's
    x = s.step(e(), s.timesteps[1], x).prev_sample
    x = s.step(e(), torch.tensor(751), x).prev_sample                             # 751 twice: the position is the counter, not a look-up
    s.verify_timesteps()
    s.step(e(), torch.tensor(626, device=DEV), x)                                 # a foreign CUDA tensor is compared on the device ...
    s.verify_timesteps()
    s.step(e(), torch.tensor(626, device=DEV), x)                                 # (forward 4 is at 501)
    with pytest.raises(RuntimeError):
        s.verify_timesteps()                                                      # ... and read here
    first = e()
    s.set_timesteps(8, device=DEV)
    x = s.step(first, s.timesteps[0], x).prev_sample
    with pytest.raises(ValueError, match="history"):
        s.step(first, s.timesteps[1], x)                                          # the model output overwrote a history entry that is still read


# ---------------------------------------------------------------------------------------------------------------- engine
def engine_inputs(B, seed=43):
    pe, ne = synthetic_prompt_embeds(B, seed=1001).half(), synthetic_prompt_embeds(B, seed=1002).half()
    noise = torch.randn(B, 4, 16, 16, generator=torch.Generator().manual_seed(seed)).half()
    return [t.to(DEV) for t in (pe, ne, noise)]


def hand_loop(unet, sch, pe, ne, noise, n, g):
    """one forward per entry of scheduler.timesteps: fp32 solver state and fp32 eps, the denoiser reads the state's fp16 copy"""
    B = pe.shape[0]
    ctx = torch.cat([ne, pe]).to(torch.float16).contiguous()
    sch.set_timesteps(n, device=DEV)
    x = noise.float()
    for i, t in enumerate(sch.timesteps):
        eps = unet(x.half(), t, encoder_hidden_states=ctx, dup=2, reuse_kv=(i > 0), out_dtype=torch.float32)[0]
        x = sch.step(eps[B:], t, x, return_dict=False, eps_uncond=eps[:B], guidance_scale=g)[0]
    return x


def make(kind):
    if kind == "deis":
        return DEISMultistepScheduler(**dict(SD15_DEIS_KWARGS, solver_order=3))
    if kind == "ipndm":
        return PNDMScheduler(**SD15_PNDM_KWARGS)
    return UniPCMultistepScheduler(**SD15_UNIPC_KWARGS)


@pytest.mark.parametrize("kind", ["deis", "ipndm", "unipc"])
def test_engine_equals_the_hand_written_loop(kind):
    """... for the two new schedulers, and for UniPC: nothing changes for a scheduler whose timesteps are num_inference_steps long"""
    from tests._models import get_unet
    unet, _ = get_unet(REDUCED, seed=5, residual="f16")
    n, g = 8, 3.0
    pe, ne, noise = engine_inputs(2)
    sch = make(kind)
    eng = SDSamplingEngine(unet, sch, guidance_scale=g)
    eng.forward_events = []
    got = eng.generate(pe, ne, latents=noise, num_inference_steps=n).clone()
    assert len(eng.forward_events) == (n + 1 if kind == "ipndm" else n) == len(sch.timesteps)
    assert len(eng._bufs["ring"]) == sch.history_slots == {"deis": 3, "ipndm": 5, "unipc": 3}[kind]
    want = hand_loop(unet, make(kind), pe, ne, noise, n, g)
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()) and torch.equal(got, want)


@pytest.mark.parametrize("latents_dtype", [torch.float32, torch.float16], ids=["f32_state", "f16_state"])
@pytest.mark.parametrize("kind", ["deis", "ipndm"])
def test_engine_graph_is_bit_identical_to_eager(kind, latents_dtype):
    """neither step reads the device: the captured generation is the eager one bit for bit, and so is its second replay; with and without CFG"""
    from tests._models import get_unet
    unet, _ = get_unet(REDUCED, seed=5)
    n = 8
    pe, ne, noise = engine_inputs(2, seed=44)
    eng = SDSamplingEngine(unet, make(kind), guidance_scale=3.0, latents_dtype=latents_dtype)
    eager = eng.generate(pe, ne, latents=noise, num_inference_steps=n).clone()
    graph = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    again = eng.generate(pe, ne, latents=noise, num_inference_steps=n, use_graph=True).clone()
    assert eager.dtype == latents_dtype and bool(torch.isfinite(eager).all())
    assert torch.equal(eager, graph) and torch.equal(graph, again)
    eng1 = SDSamplingEngine(unet, make(kind), guidance_scale=1.0, latents_dtype=latents_dtype)      # without CFG the scheduler is handed the ring slot itself
    e1 = eng1.generate(pe, latents=noise, num_inference_steps=5).clone()
    g1 = eng1.generate(pe, latents=noise, num_inference_steps=5, use_graph=True).clone()
    assert bool(torch.isfinite(e1).all()) and torch.equal(e1, g1)


@pytest.mark.parametrize("kind", ["deis", "ipndm"])
def test_cli_generate_type(kind, tmp_path):
    import os
    from consolver_amd import generate as gen
    from consolver_amd.synth import synthetic_vae_state_dict
    from consolver_amd.vae import HipAutoencoderKL
    from tests._models import get_unet
    unet, _ = get_unet(REDUCED, seed=5)
    vae = HipAutoencoderKL(dict(REDUCED), device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=6))
    d = str(tmp_path / kind)
    r = gen.main(["--out", d, "--synthetic", "2", "--steps", "8", "--batch-size", "2", "--type", kind], unet=unet, vae=vae)
    assert r["images"] == 2 and r["solver"] == kind and r["use_conv"] is False
    assert sorted(f for f in os.listdir(d) if f.endswith(".png")) == ["0_00000000.png", "0_00000001.png"]
