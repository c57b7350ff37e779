"""CPU tests of the FLUX-Kontext PPO trainer's arithmetic against tests/golden/flux_ppo_update.npz (tools/make_flux_ppo_golden.py: the
reference's edit_ppo FactorNetPPO under autograd + AdamW, its advantage expression, its pack of a packed noise), and of the step-count
broadcast in two real gloo processes.  The restatements here (``advantages_restated``) are what tests/test_flux_ppo_gpu.py holds the kernels to."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from consolver_amd import ppo_flux
from consolver_amd.flux import pack_latents
from oracle import solver_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def advantages_restated(rewards, rewards_base, masks, n, clip_hi=100.0):
    """edit_ppo/train_ppo.py:326-341 in float64: (r - clamp(mean, base, hi)) / (std_unbiased + 1e-8), tiled over n - 1 steps, masked"""
    r = np.asarray(rewards, np.float64).reshape(-1, 1)
    B = r.shape[0]
    center = min(max(r.mean(), float(rewards_base)), float(clip_hi))
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((r - r.mean()) ** 2).sum() / (B - 1)) if B > 1 else np.float64("nan")
    adv = (r - center) / (std + 1e-8)
    return np.repeat(adv, n - 1, axis=0) * np.asarray(masks, np.float64).reshape(B * (n - 1), -1)


def advantage_cases(g):
    return [(ai, *c.split(",")) for ai, c in enumerate(g["a_cases"])]


def test_advantage_restatement_matches_reference_expression(golden):
    g = golden["flux_ppo_update"]
    cases = advantage_cases(g)
    assert len(cases) == 41 and {c[4] for c in cases} == {"below", "above", "equal", "hundred", "over_hi", "flat_below", "flat_above", "low_hi"}
    for ai, B, n, A, bc in cases:
        B, n, A = int(B), int(n), int(A)
        want = g[f"a{ai}_out"]
        got = advantages_restated(g[f"a{ai}_rewards"], g[f"a{ai}_base"], g[f"a{ai}_masks"], n, g[f"a{ai}_clip_hi"])
        assert want.shape == got.shape == (B * (n - 1), A) and int(g[f"a{ai}_n"]) == n
        if B == 1:
            assert np.isnan(want).all() and np.isnan(got).all()
            continue
        assert (g[f"a{ai}_masks"] == 0).any() or B * (n - 1) * A < 4
        np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5, err_msg=f"case {ai} {bc}")
        # what each base case is there for
        if bc in ("hundred", "over_hi"):
            assert (got <= 0).all()                                  # centre = 100 (clip_hi wins over a base of 150): every PSNR-sized reward is below it
        if bc == "flat_below":
            assert (got == 0).all()                                  # std = 0 and centre = mean: 0 / 1e-8
        if bc == "flat_above":
            assert np.allclose(got[g[f"a{ai}_masks"] > 0], (20.5 - 21.0) / 1e-8)      # the 1e-8 decides
        if bc == "low_hi":
            assert float(g[f"a{ai}_clip_hi"]) < float(g[f"a{ai}_base"])


def test_as_rollout_noise_layouts(golden):
    g = golden["flux_ppo_update"]
    packed, want = torch.from_numpy(g["pack_in"]), torch.from_numpy(g["pack_out"])
    assert packed.shape == (2, 64, 64)
    x = ppo_flux.as_rollout_noise(packed, 16, 16)
    assert x.shape == (2, 16, 16, 16) and x.data_ptr() == packed.data_ptr()             # a view of the stored tensor
    assert torch.equal(pack_latents(x), want)                                           # the reference's element order, to the bit
    assert not torch.equal(want, packed)                                                # ... which is NOT the teacher's initial latents
    assert torch.equal(torch.sort(want.flatten())[0], torch.sort(packed.flatten())[0])  # but a permutation of them
    y = ppo_flux.as_rollout_noise(packed, 16, 16, noise_layout="packed")
    assert y.shape == (2, 16, 16, 16) and torch.equal(pack_latents(y), packed)          # round trip
    four = torch.randn(2, 16, 16, 16)
    assert ppo_flux.as_rollout_noise(four, 16, 16) is four
    bf = packed.to(torch.bfloat16)
    assert torch.equal(pack_latents(ppo_flux.as_rollout_noise(bf, 16, 16)).float(), want)
    with pytest.raises(ValueError):
        ppo_flux.as_rollout_noise(packed, 16, 16, noise_layout="nope")
    with pytest.raises(ValueError):
        ppo_flux.as_rollout_noise(packed[:, :60], 16, 16)
    with pytest.raises(ValueError):
        ppo_flux.as_rollout_noise(packed, 4, 16)


def golden_weights(g, ui, ep=None):
    pre = f"u{ui}_w_" if ep is None else f"u{ui}_e{ep}_after_"
    return {k[len(pre):]: np.asarray(g[k]) for k in g.files if k.startswith(pre)}


def test_flux_policy_gradient_oracle_matches_reference_autograd(golden):
    """oracle/solver_oracle.ppo_policy_grads(variant="flux") against the reference's autograd at T = 0.01, in rows that are saturated and rows
    that are not; the second epoch starts from the golden's own parameters after the first"""
    g = golden["flux_ppo_update"]
    assert [tuple(int(v) for v in g[f"u{ui}_cfg"]) for ui in range(3)] == [(2, 0, 0, 11, 32, 40), (3, 1, 1, 7, 24, 21), (2, 0, 0, 11, 32, 1)]
    for ui in range(3):
        share, rows = float(g[f"u{ui}_sat_share"]), float(g[f"u{ui}_sat_rows"])
        assert share > 0.05 and (int(g[f"u{ui}_cfg"][5]) == 1 or 0.0 < rows < 1.0), (ui, share, rows)
        clip_range, entropy_coef = float(g[f"u{ui}_hyper"][5]), float(g[f"u{ui}_hyper"][6])
        for ep in range(2):
            w = golden_weights(g, ui, None if ep == 0 else 0)
            loss, grads = so.ppo_policy_grads(w, g[f"u{ui}_x"], g[f"u{ui}_actions"], g[f"u{ui}_old_probs"], g[f"u{ui}_adv"], variant="flux",
                                              clip_range=clip_range, entropy_coef=entropy_coef)
            want_loss = float(g[f"u{ui}_e{ep}_loss"])
            print(f"case {ui} epoch {ep}: loss {loss:.6f} (reference {want_loss:.6f})")
            assert abs(loss - want_loss) < 5e-5 * max(1.0, abs(want_loss)), (ui, ep, loss, want_loss)
            for k, gv in grads.items():
                want = g[f"u{ui}_e{ep}_grad_{k}"]
                err = np.linalg.norm(gv.astype(np.float64) - want) / max(np.linalg.norm(want), 1e-12)
                print(f"  grad {k}: rel-L2 {err:.3e}")
                assert err < 1e-4, (ui, ep, k, err)
            total, _ = so.clip_grad_norm(grads, float(g[f"u{ui}_hyper"][7]))
            assert abs(total - float(g[f"u{ui}_e{ep}_norm"])) < 1e-4 * max(1.0, total)


WORKER = r'''
import os, random, sys, torch
sys.path.insert(0, %r)
from consolver_amd import launch, ppo_flux
rank, world, local, dist = launch.init_distributed("gloo")
assert dist is not None and world == 2
rng = random.Random(100 + 17 * rank)            # the ranks' generators differ: only rank 0's draw may count
got = [ppo_flux.draw_num_inference_steps(dist, rng) for _ in range(12)]
dist.barrier()
dist.destroy_process_group()
open(os.path.join(os.path.dirname(os.path.abspath(__file__)), f"rank{rank}.txt"), "w").write(",".join(map(str, got)))
'''


def test_step_count_broadcast_two_process_gloo(tmp_path):
    """edit_ppo/train_ppo.py:275-283: both ranks of train_iteration_flux's step-count draw see rank 0's number"""
    script = tmp_path / "worker.py"
    script.write_text(WORKER % ROOT)
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", port, str(script)],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    rng = random.Random(100)
    want = [rng.choice(list(range(2, 6))) for _ in range(12)]
    assert len(set(want)) > 1 and all(2 <= n <= 5 for n in want)
    assert (tmp_path / "rank0.txt").read_text() == (tmp_path / "rank1.txt").read_text() == ",".join(map(str, want))
    # without a process group the draw is local
    assert ppo_flux.draw_num_inference_steps(None, random.Random(100)) == want[0]
