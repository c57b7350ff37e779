"""Host-side checks of the depth and segmentation rewards on images of any aspect ratio: the size rule (``DepthImageProcessor.output_size`` and
cs_depth_processed_size on a CPU handle) against the installed DPT processor, the fp32 restatement (tests/depth_oracle_hw.py) against the committed fixture
of the installed transformers / PIL (tools/make_depth_hw_golden.py), the fixture's regeneration, the Segformer processor's stretch, and the grouping of
``evaluation.score_image_pairs``.  No GPU."""
import ctypes as C
import importlib.util
import itertools
import os

import numpy as np
import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import evaluation as ev
from consolver_amd import ppo
from consolver_amd.reward_model import DepthImageProcessor, load_depth_reward
from tests import depth_oracle as do
from tests import depth_oracle_hw as dh
from tests import vit_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (36, 64, 90, 96, 100, 112, 350, 512, 518, 672, 700, 768, 880, 1024, 1184, 1568)
# the issue's table: input (h, w) -> processed (h, w) at size 518; none of them may be beyond the limit
TABLE_518 = {(880, 1184): (518, 700), (1184, 880): (700, 518), (512, 768): (518, 784), (672, 1568): (518, 1204), (64, 96): (350, 518), (100, 36): (518, 182),
             (1024, 1024): (518, 518)}
TABLE_56 = {(64, 96): (56, 84), (64, 90): (56, 84), (48, 112): (56, 126)}


def _generator():
    spec = importlib.util.spec_from_file_location("make_depth_hw_golden", os.path.join(ROOT, "tools", "make_depth_hw_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ensure_built():
    if not os.path.exists(L.LIB_PATH):
        from consolver_amd.build import build
        build()


@pytest.mark.parametrize("size,table", [(518, TABLE_518), (56, TABLE_56)])
def test_size_rule_matches_the_installed_processor(size, table):
    """every ordered pair of SIDES: ``output_size`` (no limit of its own) and cs_depth_processed_size equal the shape of the installed DPT processor's
    pixel_values.  The pairs the library refuses are beyond the limit stated in include/consolver_hip.h (a processed side above 3 x size, or under one
    patch): they are counted, each is checked to BE beyond it, and no row of the issue's table is among them."""
    _ensure_built()
    gen = _generator()
    hf = gen.base().hf_processor(size)
    model, proc = load_depth_reward(device="cpu", config=dict(image_size=size))
    assert type(proc) is DepthImageProcessor
    lib = L.lib()
    refused = []
    for h, w in itertools.product(SIDES, SIDES):
        want = tuple(hf(images=[np.zeros((h, w, 3), np.uint8)], return_tensors="np")["pixel_values"].shape[-2:])
        rule = proc.output_size(h, w)
        assert rule == dh.output_size(h, w, size)
        assert rule == want, (h, w, rule, want)
        oh, ow = C.c_int(), C.c_int()
        rc = lib.cs_depth_processed_size(model._h, h, w, C.byref(oh), C.byref(ow))
        if rc:
            assert lib.cs_error_string(rc) == b"not implemented"
            assert max(want) > 3 * size or min(want) < 14, (h, w, want)
            assert lib.cs_depth_preprocess_workspace_bytes_hw(model._h, 1, h, w) == 0
            assert lib.cs_depth_preprocess_hw(model._h, None, L.CS_F32, 1, h, w, None, None, None, None, None, 0, None) == rc          # ... before any pointer is read
            refused.append((h, w))
            continue
        assert max(want) <= 3 * size and min(want) >= 14
        assert (oh.value, ow.value) == want, (h, w, (oh.value, ow.value), want)
        assert model.processed_size(h, w) == want
        assert lib.cs_depth_workspace_bytes_hw(model._h, 1, *want) > 0 and lib.cs_depth_flops_hw(model._h, 1, *want) > 0
    print(f"size {size}: {len(refused)} of {len(SIDES) ** 2} pairs are beyond the limit: {refused}")
    for hw, want in table.items():
        assert hw not in refused and proc.output_size(*hw) == want, hw
    assert len(refused) == {518: 8, 56: 122}[size]          # counted on the rule itself: a change of the limit shows here


def test_square_call_is_the_hw_call_on_the_host():
    """the per-call workspace and FLOPs at (size, size) are the square entry points', and the hw entry points refuse what is not whole patches"""
    _ensure_built()
    model, _ = load_depth_reward(device="cpu")
    lib = L.lib()
    for b in (1, 3):
        assert lib.cs_depth_workspace_bytes_hw(model._h, b, 518, 518) == lib.cs_depth_workspace_bytes(model._h, b)
        assert lib.cs_depth_flops_hw(model._h, b, 518, 518) == lib.cs_depth_flops(model._h, b)
    assert lib.cs_depth_workspace_bytes_hw(model._h, 1, 518, 700) > lib.cs_depth_workspace_bytes(model._h, 1)
    # 37 x 50 tokens against 37 x 37: everything grows with the tokens, attention's scores with their square
    assert 50 / 37 < model.flops_hw(1, (518, 700)) / model.flops(1) < (50 / 37) ** 2
    for bad in ((518, 701), (0, 518), (518, 14 * 112), (7, 518)):
        assert lib.cs_depth_workspace_bytes_hw(model._h, 1, *bad) == 0
        rc = lib.cs_depth_forward_hw(model._h, None, 1, bad[0], bad[1], None, None, 0, None)
        assert rc != 0 and lib.cs_error_string(rc) == b"not implemented"
    # the square entry points keep refusing, and say where to go
    rc = lib.cs_depth_preprocess(model._h, None, L.CS_F32, 1, 64, 96, None, None, None, 0, None)
    assert rc != 0 and b"square" in lib.cs_last_error() and b"cs_depth_preprocess_hw" in lib.cs_last_error()
    assert lib.cs_depth_processed_size(None, 64, 96, None, None) != 0


def test_restatement_equals_the_transformers_fixture(golden):
    """tests/depth_oracle_hw.py vs the installed DPTImageProcessor + DepthAnythingForDepthEstimation (position table interpolated by transformers) +
    post_process_depth_estimation (stored), at the bounds tests/test_depth_reward_oracle.py uses for the square fixture: the uint8 image exactly,
    predicted_depth and the normalised maps to rtol = atol = 1e-5, the reward to 1e-4; and the fixture is not degenerate."""
    g = golden["depth_reward_hw"]
    gen = _generator()
    b = gen.base()
    assert [str(c) for c in g["cases"]] == [c[0] for c in gen.CASES]
    oracles = {}
    for i, (name, size, h, w, dtype) in enumerate(gen.CASES):
        if size not in oracles:
            oracles[size] = dh.DepthAnythingOracleHW(b.state_dict(size), b.reduced_config(size))
        pred, target = gen.case_images(i, h, w, dtype)
        u8, pv = dh.preprocess(torch.stack([pred, target]), size)
        assert tuple(g[f"{name}_size"]) == dh.output_size(h, w, size) == tuple(u8.shape[-2:]) and u8.shape[-2] != u8.shape[-1]
        assert np.array_equal(u8[0], g[f"{name}_u8"]), name
        depth = oracles[size](pv)
        np.testing.assert_allclose(depth.numpy(), g[f"{name}_depth"], rtol=1e-5, atol=1e-5, err_msg=name)
        maps = do.normalized_maps(depth, h, w)
        np.testing.assert_allclose(maps.numpy(), g[f"{name}_maps"], rtol=1e-5, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(do.depth_reward(maps[:1], maps[1:]).numpy(), g[f"{name}_reward"], atol=1e-4, err_msg=name)
        # the fixture conditions, on what is stored
        raw = torch.nn.functional.interpolate(torch.from_numpy(g[f"{name}_depth"])[:, None], size=(h, w), mode="bicubic", align_corners=False)[:, 0]
        assert gen.conditions(raw, g[f"{name}_reward"][0, 0])[1], name
        # the comparator's stored figures are what its stored depth gives, and it is well-conditioned: an order of magnitude above fp16's error, no more
        bf = torch.from_numpy(g[f"{name}_depth_bf16"].view(np.int16).copy()).view(torch.bfloat16).float()
        mb = do.normalized_maps(bf, h, w)
        np.testing.assert_allclose(do.depth_reward(mb[:1], mb[1:]).numpy(), g[f"{name}_reward_bf16"], atol=1e-4)
        assert np.all(np.isfinite(g[f"{name}_bf16_errors"])) and 1e-3 < g[f"{name}_bf16_errors"][0] < 5e-2, name
    # the square grid goes through the restatement unchanged
    sd = b.state_dict(70)
    pv = torch.randn(1, 3, 70, 70, generator=torch.Generator().manual_seed(0))
    assert torch.equal(dh.DepthAnythingOracleHW(sd, b.reduced_config(70))(pv), do.DepthAnythingOracle(sd, b.reduced_config(70))(pv))


def test_fixture_regenerates(golden):
    """integers exactly; results of fp32 matmuls to round-off (the BLAS blocking may differ between hosts); the bf16 comparator's depth within two bf16 ulps
    of its largest value.  The comparator's derived error figures move with those ulps and are only required to be finite here (the restatement test pins them
    to their stored depth)."""
    pytest.importorskip("transformers")
    pytest.importorskip("PIL.Image")
    g = golden["depth_reward_hw"]
    fx = _generator().build_fixture()
    assert sorted(fx) == sorted(g.files)
    for k in g.files:
        a, b = np.asarray(fx[k]), np.asarray(g[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k.endswith("_depth_bf16"):
            fa, fb = (torch.from_numpy(v.view(np.int16).copy()).view(torch.bfloat16).float().numpy() for v in (a, b))
            assert float(np.abs(fa - fb).max()) <= 2 * 2.0 ** -8 * float(np.abs(fb).max()), k
        elif k.endswith("_bf16_errors") or k.endswith("_reward_bf16"):
            assert np.all(np.isfinite(a)), k
        elif k.endswith("_reward"):
            np.testing.assert_allclose(a, b, atol=1e-4, err_msg=k)
        elif a.dtype == np.float32:
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5, err_msg=k)
        else:
            assert np.array_equal(a, b), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "depth_reward_hw.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "depth_reward.npz"))


@pytest.mark.parametrize("h,w", [(64, 96), (200, 120)])
def test_segformer_processor_stretches_to_a_square(h, w):
    """what cs_seg_preprocess_hw restates: the installed SegformerImageProcessor resizes ANY input to size x size with PIL BILINEAR, each axis on its own scale
    -- equal to Image.resize((size, size), BILINEAR) and to the fixed-point restatement the GPU test compares the kernel with"""
    from PIL import Image
    from tests import segformer_oracle as so
    try:
        from transformers.models.segformer.image_processing_pil_segformer import SegformerImageProcessorPil as P
    except ImportError:
        from transformers import SegformerImageProcessor as P
    size = 128
    proc = P(do_resize=True, size={"height": size, "width": size}, resample=2, do_rescale=False, do_normalize=False, do_reduce_labels=False)
    img = vo.to_uint8_hwc(vo.synthetic_image(7, h, w))
    got = np.asarray(proc(images=[Image.fromarray(img)], return_tensors="np")["pixel_values"][0])
    want = np.asarray(Image.fromarray(img).resize((size, size), Image.BILINEAR)).transpose(2, 0, 1)
    assert got.shape == (3, size, size) and np.array_equal(got.astype(np.uint8), want)
    assert np.array_equal(so.pil_bilinear_resize(img, size, size).transpose(2, 0, 1), want)


def test_score_image_pairs_groups_by_size(tmp_path, monkeypatch):
    """the host logic of ``score_image_pairs``: a chunk of mixed sizes is scored in groups of one size, every group one call, the scores in input order; a
    pair of two sizes raises with its files named.  The reward itself is replaced (image_psnr needs the GPU): the mean of pred, which identifies the image."""
    sizes = [(8, 12), (12, 8), (8, 12), (8, 8), (12, 8), (8, 12), (8, 8)]
    for i, (h, w) in enumerate(sizes):
        a = torch.full((3, h, w), (i + 1) / 16.0)
        ev.save_generation(str(tmp_path / "a"), 0, i, a, "p")
        ev.save_generation(str(tmp_path / "b"), 0, i, a, "p")
    pairs = ev.find_image_pairs(str(tmp_path / "a"), str(tmp_path / "b"))
    assert len(pairs) == len(sizes)
    want = [float(ev.load_image_tensor(p, "cpu").mean()) for p, _ in pairs]
    assert len(set(want)) == len(want) and [tuple(ev.load_image_tensor(p, "cpu").shape[1:]) for p, _ in pairs] == sizes
    calls = []

    def fake_reward(rt, model, processor, a, b, device):
        assert a.shape == b.shape and a.dim() == 4
        calls.append(tuple(a.shape))
        return a.mean((1, 2, 3)).reshape(-1, 1)
    monkeypatch.setattr(ppo, "calculate_reward", fake_reward)
    res = ev.score_image_pairs(pairs, reward_types=("image_psnr",), batch_size=4, device="cpu")
    assert res["image_psnr"] == pytest.approx(want, abs=1e-7)
    # chunk 1 = pairs 0..3: sizes (8,12) x2, (12,8), (8,8); chunk 2 = pairs 4..6: one of each
    assert calls == [(2, 3, 8, 12), (1, 3, 12, 8), (1, 3, 8, 8), (1, 3, 12, 8), (1, 3, 8, 12), (1, 3, 8, 8)]
    assert ev.group_by_size([torch.zeros(3, 4, 5), torch.zeros(3, 5, 4), torch.zeros(3, 4, 5)], [torch.zeros(3, 4, 5), torch.zeros(3, 5, 4), torch.zeros(3, 4, 5)]) == [[0, 2], [1]]
    # a pair of two sizes
    mixed = [(pairs[0][0], pairs[1][1])]
    with pytest.raises(ValueError) as e:
        ev.score_image_pairs(mixed, reward_types=("image_psnr",), device="cpu")
    assert mixed[0][0] in str(e.value) and mixed[0][1] in str(e.value)
