"""Host-side checks of the Depth Anything depth-PSNR reward (reward_type "depth", edit_ppo/reward_model.py:92-96, 359-422): the fp32 restatement
(tests/depth_oracle.py) against the committed fixture of the installed transformers / PIL (tools/make_depth_golden.py), the executor's weight manifest against
the committed one and against transformers' own state dict, the loaders and dispatchers, the refusal of non-square inputs, and the register budget of
dpt_ops.hip.  No GPU."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import ppo
from consolver_amd.reward_model import (DEPTH_ANYTHING_V2_SMALL_CONFIG, DepthImageProcessor, HipDepthAnythingModel, calculate_depth_reward, load_depth_reward,
                                        load_reward_model)
from tests import depth_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"


def _generator():
    spec = importlib.util.spec_from_file_location("make_depth_golden", os.path.join(ROOT, "tools", "make_depth_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        from consolver_amd.build import build
        build()


def test_restatement_equals_the_transformers_fixture(golden):
    """tests/depth_oracle.py vs the installed DPTImageProcessor + DepthAnythingForDepthEstimation + post_process_depth_estimation (stored): the uint8 image
    exactly, predicted_depth and the normalised maps to rtol = atol = 1e-5, the reward to 1e-4; and the fixture is not degenerate."""
    g = golden["depth_reward"]
    gen = _generator()
    assert [str(c) for c in g["cases"]] == [c[0] for c in gen.CASES]
    oracles = {}
    for i, (name, size, hw, dtype) in enumerate(gen.CASES):
        if size not in oracles:
            oracles[size] = do.DepthAnythingOracle(gen.state_dict(size), gen.reduced_config(size))
        pred, target = gen.case_images(i, hw, dtype)
        u8, pv = do.preprocess(torch.stack([pred, target]), size)
        assert np.array_equal(u8[0], g[f"{name}_u8"]), name
        depth = oracles[size](pv)
        np.testing.assert_allclose(depth.numpy(), g[f"{name}_depth"], rtol=1e-5, atol=1e-5, err_msg=name)
        maps = do.normalized_maps(depth, hw, hw)
        np.testing.assert_allclose(maps.numpy(), g[f"{name}_maps"], rtol=1e-5, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(do.depth_reward(maps[:1], maps[1:]).numpy(), g[f"{name}_reward"], atol=1e-4, err_msg=name)
        # the fixture conditions, on what is stored
        raw = torch.nn.functional.interpolate(torch.from_numpy(g[f"{name}_depth"])[:, None], size=(hw, hw), mode="bicubic", align_corners=False)[:, 0]
        assert float((raw <= 0).float().mean((1, 2)).max()) <= 0.5 and float((raw.amax((1, 2)) - raw.amin((1, 2))).min()) >= 1.0
        assert 5.0 < float(g[f"{name}_reward"][0, 0]) < 40.0
        # the comparator's stored figures are what its stored depth gives
        bf = torch.from_numpy(g[f"{name}_depth_bf16"].view(np.int16).copy()).view(torch.bfloat16).float()
        mb = do.normalized_maps(bf, hw, hw)
        np.testing.assert_allclose(do.depth_reward(mb[:1], mb[1:]).numpy(), g[f"{name}_reward_bf16"], atol=1e-4)


def test_manifest_matches_committed_and_transformers():
    _ensure_built()
    model = HipDepthAnythingModel(device="cpu")
    got = model.manifest()
    with open(os.path.join(ROOT, "tests", "golden", "depth_anything_v2_small_manifest.json")) as f:
        committed = json.load(f)
    want = [(k, tuple(s)) for k, s in committed["tensors"]]
    assert got == want
    assert got == do.manifest()
    assert committed["params"] == sum(int(np.prod(s)) for _, s in want)
    gen = _generator()
    from transformers import DepthAnythingForDepthEstimation
    with torch.device("meta"):
        hf = DepthAnythingForDepthEstimation(gen.hf_config({}))
    assert [(k, tuple(v.shape)) for k, v in hf.state_dict().items()] == want
    # the reduced shapes of the fixture
    for size in (126, 70):
        cfg = gen.reduced_config(size)
        assert HipDepthAnythingModel(cfg, device="cpu").manifest() == do.manifest(cfg)


def test_loaders_and_dispatchers():
    _ensure_built()
    model, proc = load_depth_reward(device="cpu")
    assert isinstance(model, HipDepthAnythingModel) and type(proc) is DepthImageProcessor
    assert proc.constants()[0] == 518 and model.num_tokens == 1370 and model.patch_cols == 640 and model.config == DEPTH_ANYTHING_V2_SMALL_CONFIG
    assert abs(model.flops(1) / 1e9 - 117.0) < 1.0
    with pytest.raises(NotImplementedError, match="load_depth_reward"):
        load_reward_model("depth")
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        calculate_depth_reward(object(), None, x, x, "cpu")
    with pytest.raises(NotImplementedError):
        ppo.calculate_reward("depth", None, None, x, x, "cpu")
    with pytest.raises(RuntimeError):
        HipDepthAnythingModel(dict(fusion_hidden_size=128), device="cpu")
    with pytest.raises(RuntimeError):
        HipDepthAnythingModel(dict(out_indices=(3, 3, 9, 12)), device="cpu")
    with pytest.raises(RuntimeError):
        HipDepthAnythingModel(dict(image_size=504), device="cpu", processor=DepthImageProcessor())        # the position table is not interpolated


def test_non_square_inputs_are_refused():
    _ensure_built()
    model, _ = load_depth_reward(device="cpu")
    lib = L.lib()
    rc = lib.cs_depth_preprocess(model._h, None, L.CS_F32, 1, 64, 96, None, None, None, 0, None)
    assert rc != 0 and lib.cs_error_string(rc) == b"not implemented" and b"square" in lib.cs_last_error()
    assert lib.cs_depth_preprocess(model._h, None, L.CS_F32, 0, 64, 64, None, None, None, 0, None) == 0          # an empty batch of squares is fine
    with pytest.raises(ValueError):
        DepthImageProcessor({"height": 518, "width": 392})
    with pytest.raises(ValueError):
        do.preprocess(torch.zeros(1, 3, 64, 96), 126)


def test_dpt_kernels_do_not_spill(tmp_path):
    """every kernel of dpt_ops.hip: 0 bytes of scratch on the cross-compiled assembly"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "dpt_ops.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-x", "hip", os.path.join(ROOT, "consolver_amd", "csrc", "dpt_ops.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    names = set()
    for b in blocks:
        name = b.split("\n")[0].split()[0]
        names.add(name)
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
    for k in ("dpt_conv_kernel", "dpt_bilinear_kernel", "dpt_pixel_shuffle_kernel", "dpt_head_kernel", "dpt_bicubic_kernel", "dpt_minmax_normalize_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == 7                                       # the conv is built for 32 and 64 output channels
