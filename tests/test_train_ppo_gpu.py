"""SD1.5 PPO trainer on the GPU: cs_gather_rows, cs_image_psnr_bcast, the grouped rollout (row counts, records, values against the fp32 CPU oracle loop), the
shared reward target, and the train_ppo driver (steps, checkpoints, exact resume, the parameter-sum check).  Reduced networks of tests/test_ppo_gpu.py:
layers_per_block=1, sample_size=16, and the reduced VAE."""
import importlib.util
import os
import shutil

import numpy as np
import pytest
import torch

import consolver_amd
from consolver_amd import _lib as L
from consolver_amd import ppo, rollout
from consolver_amd import train_ppo as tp
from oracle import solver_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = dict(layers_per_block=1, sample_size=16)


# ---- cs_gather_rows -------------------------------------------------------------------------------------------------------------------------------
def _gather(src, rows_src, index, elems, dst):
    return L.lib().cs_gather_rows(L.ptr(src), rows_src, L.ptr(index), index.numel(), elems, L.dtype_code(src.dtype), L.ptr(dst), L.stream_ptr(src.device))


def _rows(rows, elems, dtype, seed, misaligned=False):
    """[rows, elems] of distinct values; ``misaligned``: a view one element into its buffer, so its address is no multiple of 16"""
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(rows * elems + 1, generator=g).to(dtype).to(DEV)
    return (flat[1:] if misaligned else flat[:-1]).view(rows, elems)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("elems", [1, 7, 8, 1024, 4 * 16 * 16])
def test_gather_rows_matches_indexing(dtype, elems):
    rows_src = 5
    for misaligned in (False, True):
        src = _rows(rows_src, elems, dtype, 3 + elems, misaligned)
        assert (src.data_ptr() % 16 != 0) == misaligned
        for index in ([4, 0, 0], [0, 1, 2, 3, 4], [2, 2, 4, 0, 1, 1, 3, 4, 2]):               # fewer, as many and more rows than the source has; repeats
            idx = torch.tensor(index, dtype=torch.int64, device=DEV)
            dst = torch.full((len(index), elems), 7.0, dtype=dtype, device=DEV)
            assert _gather(src, rows_src, idx, elems, dst) == 0
            assert torch.equal(dst, src[idx]), (dtype, elems, misaligned, index)
            assert torch.equal(rollout.gather_rows(src, idx), src[idx])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("elems,misaligned", [(1024, False), (1024, True), (7, False)])
@pytest.mark.parametrize("bad", [5, -1, 2 ** 40])
def test_gather_rows_out_of_range_index_is_a_nan_row(dtype, elems, misaligned, bad):
    rows_src = 5
    src = _rows(rows_src, elems, dtype, 11, misaligned)
    index = [3, bad, 0, 4]
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    dst = torch.zeros(len(index), elems, dtype=dtype, device=DEV)
    assert _gather(src, rows_src, idx, elems, dst) == 0
    assert bool(torch.isnan(dst[1]).all())
    for r in (0, 2, 3):
        assert torch.equal(dst[r], src[index[r]])


def test_gather_rows_argument_errors():
    src = _rows(5, 64, torch.float32, 1)
    idx = torch.tensor([1, 0, 3], dtype=torch.int64, device=DEV)
    dst = torch.full((3, 64), 7.0, device=DEV)
    lib, st = L.lib(), L.stream_ptr(torch.device(DEV))
    call = lambda s, rs, i, ro, e, dt, d: lib.cs_gather_rows(L.ptr(s), rs, L.ptr(i), ro, e, dt, L.ptr(d), st)
    CS_E_ARG, CS_E_DTYPE = -1, -3
    assert call(None, 5, idx, 3, 64, 0, dst) == CS_E_ARG
    assert call(src, 5, None, 3, 64, 0, dst) == CS_E_ARG
    assert call(src, 5, idx, 3, 64, 0, None) == CS_E_ARG
    assert call(src, 5, idx, 3, 64, 0, src) == CS_E_ARG                    # dst is src
    assert call(src, 5, idx, 3, 64, 0, src[2:]) == CS_E_ARG                # dst begins inside src
    assert call(src[2:], 3, idx, 3, 64, 0, src) == CS_E_ARG                # src begins inside dst
    assert call(src, 5, idx, 3, 64, 3, dst) == CS_E_DTYPE and call(src, 5, idx, 3, 64, 9, dst) == CS_E_DTYPE
    assert call(src, -1, idx, 3, 64, 0, dst) == CS_E_ARG and call(src, 5, idx, -3, 64, 0, dst) == CS_E_ARG and call(src, 5, idx, 3, -64, 0, dst) == CS_E_ARG
    assert "overlaps" in lib.cs_last_error().decode() or "negative" in lib.cs_last_error().decode()
    # adjacent, not overlapping: rows 0-1 of one buffer into rows 2-4
    assert call(src, 2, idx.clamp(max=1), 3, 64, 0, src[2:]) == 0 and torch.equal(src[2:], src[:2][idx.clamp(max=1)])
    # nothing to do: no launch, no pointer is looked at
    assert call(None, 5, None, 0, 64, 0, None) == 0 and call(None, 5, None, 3, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())                                          # no refused call wrote anything


# ---- cs_image_psnr_bcast --------------------------------------------------------------------------------------------------------------------------
def _psnr_call(name, pred, target, *extra):
    B, elems = pred.shape[0], pred[0].numel()
    lib = L.lib()
    out = torch.empty(B, 1, dtype=torch.float32, device=pred.device)
    ws = torch.empty(int(lib.cs_psnr_workspace_bytes(B)), dtype=torch.uint8, device=pred.device)
    L.check(getattr(lib, name)(L.ptr(pred), L.ptr(target), B, elems, 0 if pred.dtype == torch.float32 else 1, 100.0, L.ptr(out), L.ptr(ws), ws.numel(),
                               L.stream_ptr(pred.device), *extra))
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("shape", [(4, 3, 64, 64), (3, 3, 20, 24), (2, 3, 8, 12)])
def test_image_psnr_bcast_equals_image_psnr(shape, dtype):
    g = torch.Generator().manual_seed(5)
    pred = torch.rand(shape, generator=g).to(dtype).to(DEV)
    target = (pred.float().cpu() + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1).to(dtype).to(DEV)
    elems = pred[0].numel()
    tiled = target[:1].expand(shape[0], -1, -1, -1).contiguous()
    want_shared = _psnr_call("cs_image_psnr", pred, tiled)
    assert torch.equal(_psnr_call("cs_image_psnr_bcast", pred, target[:1].contiguous(), 0), want_shared)
    assert torch.equal(_psnr_call("cs_image_psnr_bcast", pred, target, elems), _psnr_call("cs_image_psnr", pred, target))
    # through the Python entry: a [1, ...] target is shared
    assert torch.equal(ppo.calculate_image_psnr_reward(None, pred, target[:1]), want_shared)
    assert torch.equal(ppo.calculate_image_psnr_reward(None, pred, target), _psnr_call("cs_image_psnr", pred, target))
    assert float(want_shared.min()) > 0 and float(want_shared[0]) != float(want_shared[1])
    with pytest.raises(RuntimeError):
        _psnr_call("cs_image_psnr_bcast", pred, target, elems - 8)


# ---- grouped rollout ------------------------------------------------------------------------------------------------------------------------------
B, K, N_STEPS, CFG = 6, 3, 5, 3.0


def _forced_indices(scaler_dim):
    """[n][B, A] bin indices: the masked dims are filled with values that differ between rows (they must not split a group); the dims a step uses are
    chosen so that the forwards see 1, then a few, then B groups."""
    A = 3 + scaler_dim
    idx = np.random.default_rng(4).integers(0, K, size=(N_STEPS, B, A))
    idx[1, :, 0] = [0, 0, 0, 1, 1, 1] if scaler_dim == 0 else 2                 # step 1 uses coefficient 0
    idx[2, :, 0], idx[2, :, 1] = 0, [0, 0, 1, 0, 1, 1]                           # step 2 uses coefficients 0 and 1
    idx[3, :, 0] = [0, 1, 0, 0, 0, 1]                                            # steps 3 and 4 use all three
    idx[3, :, 1], idx[3, :, 2] = 1, 2
    if scaler_dim:
        idx[0, :, 3] = [0, 0, 0, 1, 1, 1]                                        # the scale acts from step 0
        idx[1:, :, 3] = 1
    return idx


class _Case:
    pass


_CASES = {}


def _case(scaler_dim):
    """both rollouts (grouped and not) and the oracle loop for one scaler_dim, computed once per process and left unchanged"""
    if scaler_dim in _CASES:
        return _CASES[scaler_dim]
    from consolver_amd.synth import synthetic_prompt_embeds
    from tests._models import get_oracle, get_unet
    unet, _ = get_unet(NET, seed=5)
    sch = consolver_amd.PPOScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing",
                                     order_dim=4, scaler_dim=scaler_dim, factor_net_kwargs=dict(hidden_dim=32, num_actions=K))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in sch.factor_net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    w = {k: v.numpy().copy() for k, v in sch.factor_net.state_dict().items()}
    sch.factor_net.to(DEV)
    idx = _forced_indices(scaler_dim)
    pe, ne = synthetic_prompt_embeds(1, seed=1001).half().expand(B, -1, -1).contiguous(), synthetic_prompt_embeds(1, seed=1002).half().expand(B, -1, -1).contiguous()
    noise = torch.randn(1, 4, 16, 16, generator=g).half().expand(B, -1, -1, -1).contiguous()
    c = _Case()
    c.idx, c.sch, c.unet, c.noise, c.pe, c.ne = idx, sch, unet, noise, pe, ne
    c.runs = {}
    for grouped in (False, True):
        sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx]
        stats = {}
        out = rollout.denoise_diffusion(None, sch, unet, noise.to(DEV), ["a"] * B, None, cfg=CFG, num_inference_steps=N_STEPS, prompt_embeds=pe.to(DEV),
                                        negative_prompt_embeds=ne.to(DEV), identical_inputs=True, group_rows=grouped, stats=stats)
        c.runs[grouped] = (out, stats["forward_rows"])
    sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in idx[:3]]
    stats = {}
    c.short = (rollout.denoise_diffusion(None, sch, unet, noise.to(DEV), ["a"] * B, None, cfg=CFG, num_inference_steps=3, prompt_embeds=pe.to(DEV),
                                         negative_prompt_embeds=ne.to(DEV), identical_inputs=True, group_rows=True, stats=stats), stats["forward_rows"])
    sch.factor_net.forced_action_idx = None
    # the fp32 CPU oracle loop; equal input rows go through the oracle network once (the loop itself keeps all B rows)
    uo = get_oracle(NET, seed=5)
    ctx = torch.cat([ne[:1], pe[:1]]).float()

    def eps_model(lat2, t):
        lat = lat2[:B]
        uniq, inv = np.unique(lat.reshape(B, -1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        U = uniq.shape[0]
        x = torch.from_numpy(uniq.reshape(U, 4, 16, 16))
        e = uo(torch.cat([x, x]), int(t), torch.cat([ctx[:1].expand(U, -1, -1), ctx[1:].expand(U, -1, -1)])).numpy()
        return np.concatenate([e[:U][inv], e[U:][inv]])
    so_s = so.PPOSchedulerOracle(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing",
                                 order_dim=4, scaler_dim=scaler_dim, num_actions=K, weights=w)
    c.oracle = so.sd_rollout(so_s, eps_model, noise.float().numpy(), N_STEPS, CFG, idx, cond_dtype="f16")
    c.action_values = w["action_values"]
    _CASES[scaler_dim] = c
    return c


def _expected_forward_rows(c, scaler_dim, actions, masks):
    """the number of distinct action histories in front of every forward, from the returned records (steps 1..n-1; step 0 is not recorded: its only live
    dims are the scale dims, taken from the indices that were replayed), capped nowhere: it reaches B and stays"""
    acts, msk = actions.cpu().numpy(), masks.cpu().numpy()                       # [B, n-1, A]
    n, A = acts.shape[1] + 1, acts.shape[2]
    step0 = np.zeros((B, A), np.float32)
    if scaler_dim:
        step0[:, 3:] = c.idx[0][:, 3:]                                           # a bin stands for its action value, one to one
    hists = [[() for _ in range(B)]]                                             # hists[f][b]: what row b has done before forward f
    for i in range(n):
        used = step0 if i == 0 else acts[:, i - 1] * msk[:, i - 1]
        hists.append([h + tuple(float(v) for v in used[b]) for b, h in enumerate(hists[-1])])
    return [len(set(h)) for h in hists[:n]], hists


@pytest.mark.parametrize("scaler_dim", [0, 1])
def test_grouped_rollout_row_counts_and_records(scaler_dim):
    c = _case(scaler_dim)
    (lat_g, conds_g, probs_g, actions_g, masks_g, _), rows_g = c.runs[True]
    (lat_f, conds_f, probs_f, actions_f, masks_f, _), rows_f = c.runs[False]
    want, hists = _expected_forward_rows(c, scaler_dim, actions_g, masks_g)
    print("scaler_dim", scaler_dim, "forward_rows grouped", rows_g, "ungrouped", rows_f, "expected", want)
    assert rows_g == want
    assert any(1 < u < B for u in want) and want[-1] == B and want[0] == 1       # the case covers a partial grouping and the hand-over to the full batch
    assert rows_f == [1] * (2 if scaler_dim == 0 else 1) + [B] * (N_STEPS - (2 if scaler_dim == 0 else 1))
    assert torch.equal(actions_g, actions_f) and torch.equal(probs_g, probs_f) and torch.equal(masks_g, masks_f) and torch.equal(conds_g["x"], conds_f["x"])
    assert conds_g["epsilon"].shape == conds_f["epsilon"].shape == (B, N_STEPS - 1, 4, 4, 16, 16) and lat_g.shape == (B, 4, 16, 16)
    assert bool(torch.isfinite(lat_g).all())
    # rows of one group carry the same tensors, bit for bit: the eps of forward f (the newest history entry recorded at step f) for every f ...
    pairs = 0
    for f in range(1, N_STEPS):
        for a in range(B):
            for b in range(a + 1, B):
                if hists[f][a] == hists[f][b]:
                    assert torch.equal(conds_g["epsilon"][a, f - 1, 0], conds_g["epsilon"][b, f - 1, 0]), (f, a, b)
                    pairs += 1
    assert pairs > 0
    # ... and the latents: this rollout ends with every row on its own, so the same replay cut off after 3 steps, where groups are left
    (lat_s, _, _, actions_s, masks_s, _), rows_s = c.short
    want_s, hists_s = _expected_forward_rows(c, scaler_dim, actions_s, masks_s)
    assert rows_s == want_s and len(set(hists_s[3])) < B
    pairs = 0
    for a in range(B):
        for b in range(a + 1, B):
            same = hists_s[3][a] == hists_s[3][b]
            assert bool(torch.equal(lat_s[a], lat_s[b])) == same, (a, b)
            pairs += same
    assert pairs > 0


def test_group_rows_needs_identical_inputs():
    c = _case(0)
    with pytest.raises(ValueError, match="identical_inputs"):
        rollout.denoise_diffusion(None, c.sch, c.unet, c.noise.to(DEV), ["a"] * B, None, cfg=CFG, num_inference_steps=N_STEPS, prompt_embeds=c.pe.to(DEV),
                                  negative_prompt_embeds=c.ne.to(DEV), identical_inputs=False, group_rows=True)
    other = c.noise.clone()
    other[1] += 1
    with pytest.raises(ValueError, match="copies of one sample"):
        rollout.denoise_diffusion(None, c.sch, c.unet, other.to(DEV), ["a"] * B, None, cfg=CFG, num_inference_steps=N_STEPS, prompt_embeds=c.pe.to(DEV),
                                  negative_prompt_embeds=c.ne.to(DEV), identical_inputs=True, group_rows=True)


@pytest.mark.parametrize("scaler_dim", [0, 1])
def test_grouped_rollout_values_against_the_oracle_loop(scaler_dim):
    """the latents of both rollouts against the fp32 CPU oracle loop: grouping may send a forward down another kernel route (U rows, not B), so the two are not
    bit-identical by contract; the grouped run's error is at most 1.10 x the ungrouped run's (the factor tests/test_flux_ppo_gpu.py uses for the same question)."""
    c = _case(scaler_dim)
    lat_o, conds_o, probs_o, actions_o, masks_o = c.oracle
    err = {}
    for grouped in (False, True):
        (lat, conds, probs, actions, masks, _), _ = c.runs[grouped]
        np.testing.assert_array_equal(actions.cpu().numpy(), actions_o)
        np.testing.assert_array_equal(masks.cpu().numpy(), masks_o)
        err[grouped] = float(np.linalg.norm(lat.float().cpu().numpy() - lat_o) / np.linalg.norm(lat_o))
    print(f"scaler_dim {scaler_dim}: latents rel-L2 vs the oracle loop: grouped {err[True]:.4e}, ungrouped {err[False]:.4e}")
    assert err[False] < 1e-2, err                    # the bound of test_collect_rollout_reduced_networks: the comparator itself is sound
    assert err[True] <= 1.10 * err[False], err


# ---- shared reward target -------------------------------------------------------------------------------------------------------------------------
def _vae():
    from consolver_amd.synth import synthetic_vae_state_dict
    from consolver_amd.vae import HipAutoencoderKL
    vae = HipAutoencoderKL(dict(NET), device=DEV)
    vae.load_state_dict(synthetic_vae_state_dict(vae.manifest(), seed=6))
    return vae


def _collect(c, vae, teacher, **kw):
    c.sch.factor_net.forced_action_idx = [torch.from_numpy(i).to(DEV) for i in c.idx]
    try:
        return ppo.collect_rollout(None, c.sch, c.unet, vae, c.noise.to(DEV), ["a"] * B, None, teacher, cfg=CFG, num_inference_steps=N_STEPS, decode_batch_size=4,
                                   prompt_embeds=c.pe.to(DEV), negative_prompt_embeds=c.ne.to(DEV), identical_inputs=True, **kw)
    finally:
        c.sch.factor_net.forced_action_idx = None


def test_shared_target_image_psnr_and_depth(monkeypatch):
    from consolver_amd import reward_model as rm
    c, vae = _case(0), _vae()
    g = torch.Generator().manual_seed(9)
    teacher = (torch.randn(1, 4, 16, 16, generator=g) * 0.18215).half().expand(B, -1, -1, -1).contiguous().to(DEV)
    tiled = _collect(c, vae, teacher)
    shared = _collect(c, vae, teacher, share_target=True, group_rows=True)
    assert shared["forward_rows"] == c.runs[True][1] and tiled["forward_rows"] == c.runs[False][1]
    assert torch.equal(_collect(c, vae, teacher, share_target=True)["rewards"], tiled["rewards"])
    assert tiled["rewards"].shape == (B, 1) and bool(torch.isfinite(tiled["rewards"]).all())
    # depth: the reward function is handed ONE target row, and the rewards agree with the tiled call within the reduced model's reward bound against its
    # oracle (tests/test_depth_reward_gpu.py: 1.1 x 6.966e-3; the row count picks the kernels, so not bit-identical by contract)
    spec = importlib.util.spec_from_file_location("make_depth_golden", os.path.join(ROOT, "tools", "make_depth_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    model = rm.HipDepthAnythingModel(gen.reduced_config(126), device=DEV)
    model.load_state_dict(gen.state_dict(126))
    seen = []
    real = rm.calculate_depth_reward

    def spy(reward_model, processor, model_pred, target, device=None):
        seen.append((tuple(model_pred.shape), tuple(target.shape)))
        return real(reward_model, processor, model_pred, target, device)
    monkeypatch.setattr(rm, "calculate_depth_reward", spy)
    d_tiled = _collect(c, vae, teacher, reward_type="depth", reward_model=model, reward_model_processor=model.processor)
    d_shared = _collect(c, vae, teacher, reward_type="depth", reward_model=model, reward_model_processor=model.processor, share_target=True)
    assert seen == [((B, 3, 128, 128), (B, 3, 128, 128)), ((B, 3, 128, 128), (1, 3, 128, 128))], seen
    diff = float((d_tiled["rewards"] - d_shared["rewards"]).abs().max())
    print("depth rewards tiled", d_tiled["rewards"].flatten().tolist(), "shared", d_shared["rewards"].flatten().tolist(), "max difference", diff)
    assert bool(torch.isfinite(d_shared["rewards"]).all()) and d_shared["rewards"].shape == (B, 1)
    assert diff <= 1.1 * 6.966e-3, diff


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------------
def _driver_args(out_dir, steps, *extra):
    return ["--synthetic", "4", "--train_batch_size", "4", "--max_train_steps", str(steps), "--reward_type", "image_psnr", "--teacher_steps", "3",
            "--checkpointing_steps", "2", "--output_dir", str(out_dir), "--seed", "7", "--scaler_dim", "0", "--order_dim", "4", "--factor_hidden_dim", "32",
            "--factor_embedding_dim", "32", "--factor_num_actions", "3", "--ppo_epochs", "2", "--learning_rate", "1e-3"] + list(extra)


@pytest.fixture(scope="module")
def nets():
    from tests._models import get_unet
    return get_unet(NET, seed=5)[0], _vae()


@pytest.fixture(scope="module")
def four_steps(nets, tmp_path_factory):
    """4 steps in one run, checkpoints at 2 and 4"""
    out = tmp_path_factory.mktemp("train_ppo_whole")
    return tp.main(_driver_args(out, 4), unet=nets[0], vae=nets[1]), out


def _trainer_tensors(tr):
    return [p.detach().clone() for p in tr.params] + [tr.exp_avg.clone(), tr.exp_avg_sq.clone()]


def test_driver_takes_steps_and_writes_checkpoints(four_steps):
    res, out = four_steps
    assert res["first_step"] == 0 and res["global_step"] == 4 and [l["step"] for l in res["logs"]] == [1, 2, 3, 4]
    for log in res["logs"]:
        assert set(log) == {"step", "loss", "norm", "reward", "n", "lr", "forward_rows"}
        assert all(np.isfinite(log[k]) for k in ("loss", "norm", "reward")) and 2 <= log["n"] <= 15 and log["lr"] == 1e-3
        rows = log["forward_rows"]
        assert len(rows) == log["n"] and rows[0] == 1 and all(a <= b for a, b in zip(rows, rows[1:])) and max(rows) <= 4
        if log["n"] >= 3:
            assert rows[1] == 1 and rows[2] <= 3                     # forward 2 sees at most num_actions rows
    assert sorted(d for d in os.listdir(out) if d.startswith("checkpoint-")) == ["checkpoint-2", "checkpoint-4"]
    for d in ("checkpoint-2", "checkpoint-4"):
        assert sorted(os.listdir(out / d)) == ["model.ckpt", tp.STATE_FILE]
    sd = torch.load(out / "checkpoint-4" / "model.ckpt", map_location="cpu")
    net = res["trainer"].net
    assert sorted(sd) == sorted(net.state_dict()) and all(torch.equal(sd[k], v.cpu()) for k, v in net.state_dict().items())
    assert res["trainer"].step_count == 8


def test_resume_continues_exactly(four_steps, nets, tmp_path):
    whole, _ = four_steps
    first = tp.main(_driver_args(tmp_path, 2), unet=nets[0], vae=nets[1])
    assert first["global_step"] == 2 and first["logs"] == whole["logs"][:2]
    second = tp.main(_driver_args(tmp_path, 4, "--resume_from_checkpoint", "latest"), unet=nets[0], vae=nets[1])
    assert second["first_step"] == 2 and second["global_step"] == 4
    assert second["logs"] == whole["logs"][2:]
    for a, b in zip(_trainer_tensors(second["trainer"]), _trainer_tensors(whole["trainer"])):
        assert torch.equal(a, b)
    assert second["trainer"].step_count == whole["trainer"].step_count == 8
    assert not torch.equal(second["trainer"].exp_avg, first["trainer"].exp_avg)


def test_policy_only_checkpoint_and_param_sum_check(four_steps, nets, tmp_path, capsys):
    """a directory that holds only model.ckpt (what the reference writes): the policy is loaded, the moments start at zero, the log says so; one step from
    there, to step 10, carries the parameter sum that the cross-rank check passed at world size 1"""
    whole, out = four_steps
    os.makedirs(tmp_path / "checkpoint-9")
    shutil.copy(out / "checkpoint-4" / "model.ckpt", tmp_path / "checkpoint-9" / "model.ckpt")
    os.makedirs(tmp_path / "checkpoint-abc")
    res = tp.main(_driver_args(tmp_path, 9, "--resume_from_checkpoint", "latest"), unet=nets[0], vae=nets[1])
    assert res["first_step"] == res["global_step"] == 9 and res["logs"] == []
    tr = res["trainer"]
    assert tr.step_count == 0 and float(tr.exp_avg.abs().max()) == 0.0 and float(tr.exp_avg_sq.abs().max()) == 0.0
    for a, b in zip(tr.params, whole["trainer"].params):
        assert torch.equal(a, b)
    assert "policy-only checkpoint" in capsys.readouterr().out
    res = tp.main(_driver_args(tmp_path, 10, "--resume_from_checkpoint", "checkpoint-9"), unet=nets[0], vae=nets[1])
    (log,) = res["logs"]
    assert log["step"] == 10 and set(log) == {"step", "loss", "norm", "reward", "n", "lr", "forward_rows", "param_sum"}
    assert abs(log["param_sum"] - sum(float(p.detach().sum()) for p in res["trainer"].net.parameters())) <= 1e-4 * max(1.0, abs(log["param_sum"]))
    assert sorted(os.listdir(tmp_path / "checkpoint-10")) == ["model.ckpt", tp.STATE_FILE]
    with pytest.raises(RuntimeError, match="diverged"):
        tp.check_param_sums([log["param_sum"], log["param_sum"] + 1e-3])
