"""CPU-side checks of FLUX-Kontext true classifier-free guidance: the argument errors of cs_true_cfg_combine (returned before any launch), the
driver's parser, and the reference-made fixture (tests/golden/flux_true_cfg.npz, tools/make_flux_true_cfg_golden.py).  The engine, the row
broadcast of the DiT and the kernel's arithmetic need the GPU: tests/test_flux_true_cfg_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

from consolver_amd import _lib
from consolver_amd import generate_flux as gf

NAMES = ("fmppo", "euler", "heun", "dpm-solver", "dpm-solver-multistep")


def test_true_cfg_combine_argument_errors():
    """argument validation happens before any launch -> usable without a GPU"""
    if not os.path.exists(_lib.LIB_PATH):
        from consolver_amd.build import build
        build()
    l = _lib.lib()
    F32, F16, BF16, U8 = _lib.CS_F32, _lib.CS_F16, _lib.CS_BF16, _lib.CS_U8
    call = lambda pos, neg, idt, out, odt, n: l.cs_true_cfg_combine(pos, neg, idt, 4.0, out, odt, n, None)
    # NULL pointers with n > 0
    for pos, neg, out in ((None, 64, 128), (64, None, 128), (64, 128, None)):
        assert call(pos, neg, BF16, out, BF16, 8) == -1 and b"required" in l.cs_last_error()
    # alignment: 16 bytes, except the fp32 inputs of a mixed pair (4 bytes)
    assert call(66, 128, BF16, 256, BF16, 8) == -1 and b"aligned" in l.cs_last_error()
    assert call(64, 136, F16, 256, F16, 8) == -1 and b"aligned" in l.cs_last_error()
    assert call(64, 128, BF16, 258, BF16, 8) == -1 and b"aligned" in l.cs_last_error()
    assert call(68, 128, F32, 256, F32, 8) == -1 and b"aligned" in l.cs_last_error()          # fp32 -> fp32 is no mixed pair
    assert call(66, 128, F32, 256, BF16, 8) == -1 and b"aligned" in l.cs_last_error()         # 2 bytes off: not even an fp32 element
    assert call(68, 132, F32, 250, BF16, 8) == -1 and b"aligned" in l.cs_last_error()         # the 16-bit side keeps the 16-byte rule
    # aliasing with unequal element sizes
    assert call(64, 128, F32, 64, BF16, 8) == -1 and b"alias" in l.cs_last_error()
    assert call(64, 128, F32, 128, F16, 8) == -1 and b"alias" in l.cs_last_error()
    # negative length
    assert call(64, 128, BF16, 256, BF16, -1) == -2
    # dtype pairs: the same 16-bit type in and out, fp32 in with any of the three out
    for idt, odt in ((BF16, F16), (F16, BF16), (BF16, F32), (F16, F32), (U8, U8), (F32, U8), (U8, BF16), (7, 7)):
        assert call(64, 128, idt, 256, odt, 8) == -3 and b"dtype pair" in l.cs_last_error(), (idt, odt)
    # n == 0 is a no-op whatever the pointers
    assert call(None, None, BF16, None, BF16, 0) == 0
    assert call(3, 5, F32, 7, F16, 0) == 0


def test_driver_parser_true_cfg_flags(capsys):
    base = ["--out", "o", "--jsonl", "j", "--image-dir", "d", "--instruction-cache", "c"]
    _, a = gf.parse_args(base)
    assert a.true_cfg_scale == 1.0 and a.negative_embeds is None                              # off by default
    with pytest.raises(SystemExit):
        gf.parse_args(base + ["--true_cfg_scale", "4"])
    assert "--negative-embeds" in capsys.readouterr().err
    _, a = gf.parse_args(base + ["--true_cfg_scale", "4", "--negative-embeds", "F"])
    assert a.true_cfg_scale == 4.0 and a.negative_embeds == "F"
    _, a = gf.parse_args(["--out", "o", "--synthetic", "2", "--true_cfg_scale", "4"])
    assert a.true_cfg_scale == 4.0 and a.synthetic == 2 and a.negative_embeds is None
    _, a = gf.parse_args(base + ["--negative-embeds", "F"])                                     # the file alone does not switch guidance on
    assert a.true_cfg_scale == 1.0
    for solver in gf.FLUX_SOLVERS:                                                              # both flags with every solver
        _, a = gf.parse_args(["--out", "o", "--synthetic", "1", "--solver", solver, "--true_cfg_scale", "2.5", "--negative-embeds", "F"])
        assert a.solver == solver and a.true_cfg_scale == 2.5


def test_negative_embeds_file_round_trip(tmp_path):
    import torch
    g = torch.Generator().manual_seed(0)
    pe, pooled = torch.randn(7, 32, generator=g), torch.randn(768, generator=g)
    path = str(tmp_path / "neg.safetensors")
    gf.save_negative_embeds(path, pe, pooled)
    pe2, pooled2 = gf.load_negative_embeds(path, "cpu")
    assert pe2.shape == (1, 7, 32) and pooled2.shape == (1, 768) and pe2.dtype == torch.bfloat16
    assert torch.equal(pe2[0], pe.to(torch.bfloat16)) and torch.equal(pooled2[0], pooled.to(torch.bfloat16))


def test_golden_file_has_the_five_trajectories(golden):
    g = golden["flux_true_cfg"]
    assert tuple(g["names"]) == NAMES and float(g["scale"]) == 4.0
    x0 = g["fmppo_lat"][0]
    for name in NAMES:
        lat = g[f"{name}_lat"]
        assert lat.shape == (5, 2, 24, 64) and lat.dtype == np.float32 and np.isfinite(lat).all()
        assert np.array_equal(lat[0], x0)                                                       # one initial noise for all five
        assert np.array_equal(lat.view(np.uint32) & 0xffff, np.zeros(lat.shape, np.uint32))     # bf16 values
        assert g[f"{name}_sigmas"].shape == (5,) and g[f"{name}_timesteps"].shape == (4,)
        assert all(np.abs(lat[i + 1] - lat[i]).mean() > 1e-3 for i in range(4))                 # every step moved
    assert g["fmppo_idx"].shape[1:] == (2, 1) and g["fmppo_idx"].min() >= 0 and g["fmppo_idx"].max() < 11
    assert not np.array_equal(g["euler_lat"][-1], g["heun_lat"][-1])
