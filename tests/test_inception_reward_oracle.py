"""Host-side checks of the Inception-v3 logit-cosine reward (reward_type "inception", edit_ppo/reward_model.py:98-108, 319-356): the wiring of the fp32
restatement (tests/inception_oracle.py) against torchvision's published parameter counts, the restatement against the committed fixture
(tools/make_inception_golden.py: crops from the installed PIL, logits and rewards on calibrated weights), the executor's weight manifest against the committed
one, the FLOP count, torchvision's crop offset, the loaders and dispatchers, and the register budget of incep_ops.hip.  No GPU."""
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import ppo, synth
from consolver_amd.reward_model import (INCEPTION_V3_CONFIG, HipInceptionV3, InceptionImageProcessor, calculate_inception_reward, load_inception_reward,
                                        load_reward_model)
from tests import inception_oracle as io
from tests import vit_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"


def _generator():
    spec = importlib.util.spec_from_file_location("make_inception_golden", os.path.join(ROOT, "tools", "make_inception_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        from consolver_amd.build import build
        build()


def test_manifest_matches_committed_and_the_published_counts():
    _ensure_built()
    model = HipInceptionV3(device="cpu")
    got = model.manifest()
    with open(os.path.join(ROOT, "tests", "golden", "inception_v3_manifest.json")) as f:
        committed = json.load(f)
    want = [(k, tuple(s)) for k, s in committed["tensors"]]
    assert got == want and got == io.manifest()
    assert len(got) == 566 and sum(k.endswith(".conv.weight") for k, _ in got) == 94          # 94 BasicConv2d x 6 entries + fc.weight, fc.bias
    params = sum(int(np.prod(s)) for k, s in want if "running_" not in k and "num_batches" not in k)
    assert params == io.param_count() == committed["params"] == 23_834_568
    assert params + io.AUX_PARAMS == 27_161_264 and io.AUX_PARAMS == 3_326_696               # torchvision's published inception_v3 figure
    # AuxLogits, summed: conv0 768 -> 128 1x1 + BatchNorm, conv1 128 -> 768 5x5 + BatchNorm, fc 768 -> 1000
    assert 768 * 128 + 2 * 128 + 128 * 768 * 25 + 2 * 768 + 768 * 1000 + 1000 == io.AUX_PARAMS
    for size in (75, 107, 139):
        assert HipInceptionV3(dict(image_size=size), device="cpu").manifest() == want         # the widths are the architecture's


def test_flops_match_the_config_count():
    _ensure_built()
    model = HipInceptionV3(device="cpu")
    assert abs(model.flops(1) / io.config_flops(299) - 1) < 0.01
    assert abs(io.config_flops(299) / 11.42e9 - 1) < 0.01
    assert model.flops(3) == pytest.approx(3 * model.flops(1), rel=1e-12)
    assert abs(HipInceptionV3(dict(image_size=107), device="cpu").flops(1) / io.config_flops(107) - 1) < 0.01
    assert model.num_tokens == 64 and HipInceptionV3(dict(image_size=107), device="cpu").num_tokens == 4 and HipInceptionV3(dict(image_size=139), device="cpu").num_tokens == 9


def test_restatement_equals_the_fixture_and_the_fixture_is_not_degenerate(golden):
    """tests/inception_oracle.py vs the stored results: the uint8 crops (from the installed PIL) exactly, logits and rewards to rtol = atol = 1e-5.  And the
    fixture shows what it is meant to: the largest reward of its cases is in [95, 99.9), the smallest at most 80 -- while the plain, uncalibrated recipe gives
    more than 99.9 on every pair, however different (why calibrate_batch_norm exists)."""
    g, gen = golden["inception_reward"], _generator()
    assert [str(c) for c in g["cases"]] == [c[0] for c in gen.CASES]
    assert {c[1] for c in gen.CASES} == {107, 139} and any(c[2] == (c[1], c[1]) for c in gen.CASES)          # both grids, one image of the transform's own size
    plain = io.InceptionOracle(gen.plain_state_dict())
    rewards = []
    for i, (name, size, hw, dtype, amp) in enumerate(gen.CASES):
        pred, target = gen.case_images(i)
        u8, pv = io.preprocess(torch.stack([pred, target]), size)
        assert np.array_equal(u8, g[f"{name}_u8"]), name
        logits = io.InceptionOracle(gen.state_dict(size))(pv)
        np.testing.assert_allclose(logits.numpy(), g[f"{name}_logits"], rtol=1e-5, atol=1e-5, err_msg=name)
        reward = io.inception_reward(logits[:1], logits[1:])
        np.testing.assert_allclose(reward.numpy(), g[f"{name}_reward"], rtol=1e-5, atol=1e-5, err_msg=name)
        rewards.append(g[f"{name}_reward"].item())
        lp = plain(pv)
        uncal = io.inception_reward(lp[:1], lp[1:]).item()
        assert uncal > 99.9 and abs(uncal - g[f"{name}_reward_uncalibrated"].item()) < 1e-3, name
        assert float(g[f"{name}_bf16_error"].max()) > 0.1, name          # the comparator is far from fp32 on this network: rule (a) of the GPU test has room
    assert 95 <= max(rewards) < 99.9 and min(rewards) <= 80, rewards


def test_center_crop_is_torchvisions_round_half_even(golden):
    """the two non-square cases: the stored PIL crop is the window at int(round((n - size) / 2.0)) of the resized image; n - size = 37 (1 mod 4) gives the
    floor rule's 18 as well, n - size = 39 (3 mod 4) gives 20 where the floor rule gives 19 -- and the floor rule's crop differs from PIL's there"""
    g, gen = golden["inception_reward"], _generator()
    seen = {}
    for i, (name, size, hw, dtype, amp) in enumerate(gen.CASES):
        if hw[0] == hw[1]:
            continue
        pred, _ = gen.case_images(i)
        img = vo.to_uint8_hwc(pred)
        nh, nw = vo.resize_output_size(hw[0], hw[1], size)
        n = max(nh, nw)
        r = vo.pil_bicubic_resize(img, nh, nw)
        off, floor = io.crop_offset(n, size), (n - size) // 2
        def window(o):
            return r[o:o + size, :size] if nh > nw else r[:size, o:o + size]
        assert np.array_equal(window(off).transpose(2, 0, 1), g[f"{name}_u8"][0]), name
        seen[(n - size) % 4] = (off, floor)
        if off != floor:
            assert not np.array_equal(window(floor).transpose(2, 0, 1), g[f"{name}_u8"][0]), name
    assert seen[1][0] == seen[1][1] and seen[3][0] == seen[3][1] + 1
    assert [io.crop_offset(299 + d, 299) for d in (0, 1, 2, 3, 37, 39)] == [0, 0, 1, 2, 18, 20]


def test_calibration_sets_the_batch_statistics():
    gen = _generator()
    sd0 = gen.plain_state_dict()
    _, pv = io.preprocess(io.calibration_images(75, 4), 75)
    sd = io.calibrate_batch_norm(sd0, pv)
    assert set(sd) == set(sd0)
    changed = [k for k in sd if not torch.equal(sd[k], sd0[k])]
    assert len(changed) == 2 * 94 and all("running_" in k for k in changed)
    y = torch.nn.functional.conv2d(pv.double(), sd["Conv2d_1a_3x3.conv.weight"].double(), None, 2)
    np.testing.assert_allclose(sd["Conv2d_1a_3x3.bn.running_mean"].numpy(), y.mean((0, 2, 3)).numpy(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(sd["Conv2d_1a_3x3.bn.running_var"].numpy(), y.var((0, 2, 3), unbiased=False).numpy(), rtol=1e-4, atol=1e-7)


def test_load_state_dict_ignores_auxlogits_and_rejects_missing_and_misshapen_tensors():
    _ensure_built()
    model = HipInceptionV3(dict(image_size=75), device="cpu")
    sd = synth.synthetic_inception_state_dict(model.manifest(), seed=3)
    assert sd["Mixed_6c.branch7x7dbl_3.bn.num_batches_tracked"].dtype == torch.int64 and 0.5 <= float(sd["Mixed_7a.branch3x3_2.bn.running_var"].min())
    missing = dict(sd)
    del missing["Mixed_6c.branch7x7dbl_3.conv.weight"]
    with pytest.raises(KeyError):
        model.load_state_dict(missing)
    bad = dict(sd)
    bad["fc.weight"] = bad["fc.weight"][:999]
    with pytest.raises(ValueError):
        model.load_state_dict(bad)
    lib = L.lib()
    w = torch.zeros(128, 768, 1, 1)
    sh = (L.C.c_int64 * 4)(128, 768, 1, 1)
    assert lib.cs_incep_set_weight(model._h, b"AuxLogits.conv0.conv.weight", L.C.c_void_p(w.data_ptr()), sh, 4) == 0          # accepted, ignored
    assert lib.cs_incep_num_weights(model._h) == 566
    sh = (L.C.c_int64 * 4)(160, 160, 7, 2)
    rc = lib.cs_incep_set_weight(model._h, b"Mixed_6c.branch7x7dbl_2.conv.weight", L.C.c_void_p(w.data_ptr()), sh, 4)
    assert rc != 0 and b"dim 3 is 2, expected 1" in lib.cs_last_error()
    assert lib.cs_incep_set_weight(model._h, b"Mixed_9z.conv.weight", L.C.c_void_p(w.data_ptr()), sh, 4) != 0
    assert lib.cs_incep_finalize(model._h) != 0 and b"missing weight" in lib.cs_last_error()


def test_loaders_and_dispatchers():
    _ensure_built()
    model, proc = load_inception_reward(device="cpu")
    assert isinstance(model, HipInceptionV3) and type(proc) is InceptionImageProcessor and proc.resample == 3
    assert proc.constants() == (299, 299, 1 / 255, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    assert model.patch_cols == 8 and model.config == INCEPTION_V3_CONFIG and model.max_batch >= 8
    with pytest.raises(NotImplementedError, match="load_inception_reward"):
        load_reward_model("inception")
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        calculate_inception_reward(object(), None, x, x, "cpu")
    with pytest.raises(NotImplementedError):
        ppo.calculate_reward("inception", None, None, x, x, "cpu")
    with pytest.raises(NotImplementedError):
        ppo.calculate_reward("inception", object(), None, x, x, "cpu")
    assert ppo._MODEL_REWARDS["inception"] == "calculate_inception_reward"
    with pytest.raises(ValueError):
        HipInceptionV3(dict(image_size=74), device="cpu")                                      # the last grid would be empty
    cfg, h = L.CsIncepConfig(74, 1000, (L.C.c_float * 3)(0.5, 0.5, 0.5), (L.C.c_float * 3)(0.2, 0.2, 0.2), 1 / 255), L.C.c_void_p()
    assert L.lib().cs_incep_create(L.C.byref(cfg), L.C.byref(h)) != 0 and b"75" in L.lib().cs_last_error()
    with pytest.raises(ValueError):
        HipInceptionV3(dict(image_size=139), device="cpu", processor=InceptionImageProcessor())          # the processor's 299 against a 139 model
    lib = L.lib()
    assert lib.cs_incep_set_stage_limit(model._h, 3) == 0 and lib.cs_incep_set_stage_limit(model._h, 6) != 0 and lib.cs_incep_set_stage_limit(model._h, 5) == 0
    # a resized side shorter than the crop cannot happen under the shortest-edge rule; an empty batch of any shape is fine, a bad size is refused
    assert lib.cs_incep_preprocess(model._h, None, L.CS_F32, 0, 64, 96, None, None, None, 0, None) == 0
    assert lib.cs_incep_forward(model._h, None, 1, None, None, 0, None) != 0 and b"finalize" in lib.cs_last_error()


def test_the_four_other_handles_keep_the_floor_crop_rule():
    """image_front_end.h: the crop-offset rule is a member set next to the filter; its default is (n - C) / 2"""
    src = open(os.path.join(ROOT, "consolver_amd", "csrc", "image_front_end.h")).read()
    assert "CropRule crop_rule = CROP_FLOOR;" in src
    for f in ("vit.cpp", "clip_vision.cpp", "depth.cpp", "segformer.cpp"):
        assert "crop_rule" not in open(os.path.join(ROOT, "consolver_amd", "csrc", f)).read()
    assert "CROP_ROUND_HALF_EVEN" in open(os.path.join(ROOT, "consolver_amd", "csrc", "inception.cpp")).read()


def test_incep_kernels_do_not_spill(tmp_path):
    """every kernel of incep_ops.hip: 0 bytes of scratch, read from the resource usage the compiler reports for the gfx950 code object"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "incep_ops.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S",
                        "-Rpass-analysis=kernel-resource-usage", "-x", "hip", os.path.join(ROOT, "consolver_amd", "csrc", "incep_ops.hip"), "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    names = set()
    for b in blocks:
        name = b.split("\n")[0].split()[0]
        names.add(name)
        scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"
    for k in ("incep_conv_kernel", "incep_maxpool_kernel", "incep_avgpool_kernel", "incep_mean_kernel", "incep_fc_kernel"):
        assert any(k in n for n in names), (k, names)
    assert len(names) == 6          # the convolution has two instantiations (guarded / unguarded channel loop)
