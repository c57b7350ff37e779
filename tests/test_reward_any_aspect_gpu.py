"""The depth and segmentation rewards on images of any aspect ratio, on the HIP library: the position-table kernel against torch, the two-axis front ends
against PIL, the two-size pixel shuffle against conv_transpose2d, the reduced depth model on non-square images against the committed transformers fixture
(tools/make_depth_hw_golden.py), square images through the `_hw` entry points against the square entry points bit for bit, one full-shape case against the fp32
oracle, the two reward functions on non-square pairs, the argument forms of the `_hw` calls, and ``score_image_pairs`` on a directory of two sizes.

Bounds.  The position kernel runs torch's own fp32 sequence and rounds once: an element is within one fp16 ulp of torch's fp32 value rounded to fp16; the share
of elements that differ at all is printed and bounded by what was measured (none).  The front ends are integer arithmetic: exact.  The model-level bounds are the figures measured on an
MI355X + 10 % (the suite's convention; the values are in the docstrings of the tests that assert them), and each figure must also be smaller than the error of
the same graph evaluated by torch in bf16 on the same inputs.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from consolver_amd import _lib as L
from consolver_amd import ops, ppo
from consolver_amd.reward_model import (HipDepthAnythingModel, HipSegformerModel, calculate_depth_reward, calculate_segmentation_reward, load_depth_reward)
from consolver_amd.synth import synthetic_depth_anything_state_dict
from tests import depth_oracle as do
from tests import depth_oracle_hw as dh
from tests import segformer_oracle as so
from tests import vit_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_REL_L2 = 5e-4                       # one fp16 rounding of an fp32-accumulated value: 2^-11 = 4.9e-4
F16_MAX_REL = 2.0 ** -11 + 2.0 ** -15   # ... per element, relative to the largest reference magnitude

# measured on an MI355X (see the docstrings of the tests that assert them); the asserted bounds are these + 10 %
MEASURED_POS_NOT_BIT_EQUAL = 0.0                                                                             # share of table elements not bit-equal to torch's: none in any of the five cases
MEASURED_REDUCED_DEPTH, MEASURED_REDUCED_MAPS, MEASURED_REDUCED_REWARD = 1.159e-3, 1.108e-3, 5.302e-3       # torch bf16 on the same inputs: 1.153e-2, 1.141e-2, 7.133e-2
MEASURED_FULL_MAPS, MEASURED_FULL_REWARD = 1.846e-3, 4.396e-3                                                # torch bf16 on the same inputs: 1.638e-2, 4.676e-2
SQUARE_REDUCED_REWARD = 6.966e-3        # tests/test_depth_reward_gpu.py: MEASURED_REDUCED_REWARD, the bound (+ 10 %) of the square tests' reward checks

FRONT_END_INPUTS = ((64, 96, "float16"), (96, 64, "float32"), (100, 36, "float16"), (150, 90, "float32"))   # an upscale and a downscale on each axis at 70 and 126


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pair(seed, h, w, dtype, amp=0.15):
    p = vo.synthetic_image(seed, h, w, torch.float32)
    g = torch.Generator().manual_seed(seed + 100)
    return p.to(dtype), (p + amp * torch.randn(3, h, w, generator=g)).clamp(0, 1).to(dtype)


def _f16_steps(a, b):
    """the distance of two fp16 tensors in representable values (0 = bit-equal up to the sign of zero)"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs()


# ---- the position-table kernel ------------------------------------------------------------------------------------------------------------------------
def _pos_reference(grid, gh, gw):
    """[s,s,D] fp32 -> F.interpolate's [gh*gw, D] fp32, as transformers calls it"""
    out = F.interpolate(grid.permute(2, 0, 1)[None], size=(gh, gw), mode="bicubic", align_corners=False)
    return out[0].permute(1, 2, 0).reshape(gh * gw, -1)


@pytest.mark.parametrize("s,gh,gw,D", [(5, 5, 7, 64), (5, 7, 5, 64), (5, 3, 9, 64), (5, 9, 3, 64), (37, 37, 50, 384)])
def test_position_kernel_matches_torch(s, gh, gw, D):
    """cs_op_vit_pos_interp vs F.interpolate(bicubic, align_corners=False, size=) in fp32 on the CPU: up and down on each axis at a 5 x 5 grid, and the
    V2-Small table to the grid of an 880 x 1184 image.  Every element within one fp16 ulp of torch's value rounded to fp16; row 0 zero.
    Measured on an MI355X: no element differs in any of the five cases (share 0, largest distance 0 fp16 steps).  The kernel follows the fp32 operation order of
    torch's CPU kernel (csrc/vit_ops.hip says which multiply-adds are fused and in which order the four terms of a sum are taken), so the asserted share is 0."""
    g = torch.Generator().manual_seed(s * 1000 + gh * 10 + gw)
    grid = torch.randn(s, s, D, generator=g) * 0.5
    want = _pos_reference(grid, gh, gw).half()
    gd = grid.to(DEV).contiguous()
    table = torch.full((1 + gh * gw, D), 7.0, dtype=torch.float16, device=DEV)
    L.check(L.lib().cs_op_vit_pos_interp(L.ptr(gd), s, gh, gw, D, L.ptr(table), L.stream_ptr(DEV)))
    table = table.cpu()
    assert bool((table[0] == 0).all())
    steps = _f16_steps(table[1:], want)
    share = float((steps != 0).float().mean())
    print(f"position table {s} -> {gh} x {gw}, D = {D}: {share:.3e} of {steps.numel()} elements not bit-equal, largest distance {int(steps.max())} fp16 steps")
    assert int(steps.max()) <= 1
    assert share <= max(MEASURED_POS_NOT_BIT_EQUAL * 1.1, 0.0)


# ---- op level: the two-size pixel shuffle -----------------------------------------------------------------------------------------------------------------
def _check_f16(got, want, what):
    got, want = got.float().cpu(), want.float()
    e, m = rel_l2(got.numpy(), want.numpy()), float((got - want).abs().max())
    print(what, f"rel-L2 {e:.3e} max abs {m:.3e} (max |ref| {float(want.abs().max()):.3f})")
    assert e <= F16_REL_L2, (what, e)
    assert m <= F16_MAX_REL * float(want.abs().max()) + 1e-7, (what, m)


@pytest.mark.parametrize("Gh,Gw", [(5, 7), (7, 5)])
def test_pixel_shuffle_hw_matches_conv_transpose(Gh, Gw):
    """tests/test_depth_reward_gpu.py's G-parametrised check at a Gh x Gw token grid: one linear layer over the token rows (CLS row included) + the pixel-shuffle
    store vs F.conv_transpose2d in fp32 on the same fp16 operands, k = 4 and 2; k = 1 (dropping the CLS rows) exactly; and the square form equals the old op"""
    g = torch.Generator().manual_seed(Gh * 10 + Gw)
    B, T, D = 2, Gh * Gw + 1, 128
    lib = L.lib()
    for k, Cc in ((4, 64), (2, 96)):
        tok = torch.randn(B, T, D, generator=g).half()
        wt = (torch.randn(D, Cc, k, k, generator=g) * D ** -0.5).half()
        bias = torch.randn(Cc, generator=g).half()
        want = F.conv_transpose2d(tok[:, 1:].float().reshape(B, Gh, Gw, D).permute(0, 3, 1, 2), wt.float(), bias.float(), stride=k)
        wf = wt.permute(2, 3, 1, 0).reshape(k * k * Cc, D).contiguous()
        y = ops.linear(tok.reshape(B * T, D).to(DEV), wf.to(DEV), bias.repeat(k * k).to(DEV))
        out = torch.empty(B, Gh * k, Gw * k, Cc, dtype=torch.float16, device=DEV)
        L.check(lib.cs_op_dpt_pixel_shuffle_hw(L.ptr(y), B, Gh, Gw, k, Cc, 1, L.ptr(out), L.stream_ptr(DEV)))
        _check_f16(out.permute(0, 3, 1, 2), want, f"reassemble grid {Gh} x {Gw} k {k}")
    tok = torch.randn(B, T, 192, generator=g).half().to(DEV)
    out = torch.empty(B, Gh, Gw, 192, dtype=torch.float16, device=DEV)
    L.check(lib.cs_op_dpt_pixel_shuffle_hw(L.ptr(tok), B, Gh, Gw, 1, 192, 1, L.ptr(out), L.stream_ptr(DEV)))
    assert torch.equal(out.reshape(B, Gh * Gw, 192), tok[:, 1:])
    sq = torch.randn(B, Gh * Gh + 1, 4 * 64, generator=g).half().to(DEV)
    a, b = (torch.empty(B, Gh * 2, Gh * 2, 64, dtype=torch.float16, device=DEV) for _ in range(2))
    L.check(lib.cs_op_dpt_pixel_shuffle_hw(L.ptr(sq), B, Gh, Gh, 2, 64, 1, L.ptr(a), L.stream_ptr(DEV)))
    L.check(lib.cs_op_dpt_pixel_shuffle(L.ptr(sq), B, Gh, 2, 64, 1, L.ptr(b), L.stream_ptr(DEV)))
    assert torch.equal(a, b)


# ---- the reduced depth model ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reduced():
    """the fixtures' reduced model at its two processor sizes, with the state dict it was loaded from"""
    b = _tool("make_depth_golden")
    out = {}
    for size in (126, 70):
        m = HipDepthAnythingModel(b.reduced_config(size), device=DEV)
        sd = b.state_dict(size)
        m.load_state_dict(sd)
        out[size] = (m, sd)
    return out


def test_position_table_of_the_handle(reduced):
    """the training grid launches nothing and returns the packed table; another grid is interpolated once, then served from the handle's cache, and is what the
    kernel gives for the trained grid"""
    model, sd = reduced[126]
    pos = sd["backbone.embeddings.position_embeddings"][0].float()
    table, launched = model.position_table(9, 9)
    assert not launched and table.shape == (82, 128)
    assert bool((table[0] == 0).all()) and torch.equal(table[1:].cpu(), pos[1:].half())
    first, launched = model.position_table(6, 9)
    assert launched and first.shape == (55, 128)
    again, launched = model.position_table(6, 9)
    assert not launched and torch.equal(first, again)
    want = _pos_reference(pos[1:].reshape(9, 9, 128), 6, 9).half()
    assert int(_f16_steps(first[1:].cpu(), want).max()) <= 1 and bool((first[0] == 0).all())
    # a full cache is emptied, not grown: 16 further grids, then the first one is interpolated again
    for gw in range(10, 26):
        assert model.position_table(9, gw)[1]
    assert model.position_table(9, 25)[1] is False
    assert model.position_table(6, 9)[1] is True
    with pytest.raises(RuntimeError, match="not implemented"):
        model.position_table(9, 28)                  # 28 patches = 392 > 3 x 126


def test_depth_front_end_is_bit_identical_to_pil(reduced):
    """PIL BICUBIC straight to the processed size, both axes on their own scale: the uint8 image equals PIL's own Image.resize and the fixed-point restatement,
    pixel_values within 2^-10 of the fp32 processor (the fp16 half-ulp at |v| < 4); sizes 70 and 126 x the four inputs (fp16 and fp32 quantisation paths)"""
    from PIL import Image
    for size in (70, 126):
        model = reduced[size][0]
        for i, (h, w, dtype) in enumerate(FRONT_END_INPUTS):
            imgs = torch.stack(_pair(500 + i, h, w, getattr(torch, dtype)))
            oh, ow = dh.output_size(h, w, size)
            patches, got_size, u8 = model.preprocess_hw(imgs.to(DEV), return_crop=True)
            assert got_size == (oh, ow) == model.processed_size(h, w)
            assert u8.dtype == torch.uint8 and u8.shape == (2, 3, oh, ow) and patches.shape == (2 * (oh // 14) * (ow // 14), 640)
            want_u8, want_pv = dh.preprocess(imgs, size)
            pil = np.stack([np.asarray(Image.fromarray(vo.to_uint8_hwc(im)).resize((ow, oh), Image.BICUBIC)).transpose(2, 0, 1) for im in imgs])
            assert np.array_equal(want_u8, pil), (size, h, w)
            assert np.array_equal(u8.cpu().numpy(), pil), (size, h, w)
            pv = model.patches_to_pixel_values(patches, (oh, ow)).float().cpu()
            assert float((pv - want_pv).abs().max()) <= 2.0 ** -10, (size, h, w)
            assert bool((patches[:, 588:] == 0).all())
            assert torch.equal(model.pixel_values_to_patches(model.patches_to_pixel_values(patches, (oh, ow))), patches)
    with pytest.raises(RuntimeError, match="square"):          # the square patch-row API keeps its refusal
        reduced[126][0].preprocess(torch.zeros(1, 3, 64, 96, device=DEV))


def test_fixture_front_end(golden, reduced):
    g = golden["depth_reward_hw"]
    gen = _tool("make_depth_hw_golden")
    for i, (name, size, h, w, dtype) in enumerate(gen.CASES):
        pred, target = gen.case_images(i, h, w, dtype)
        _, got_size, u8 = reduced[size][0].preprocess_hw(torch.stack([pred, target]).to(DEV), return_crop=True)
        assert got_size == tuple(g[f"{name}_size"]) and np.array_equal(u8[0].cpu().numpy(), g[f"{name}_u8"]), name


def test_reduced_model_matches_transformers_fixture(golden, reduced):
    """HIP (fp16 storage, fp32 accumulation, position table interpolated on the device) vs transformers DepthAnythingForDepthEstimation +
    post_process_depth_estimation in fp32 on the reduced config, non-square images through the whole path, the four fixture cases taken together.
    Measured: predicted_depth rel-L2 1.159e-3, normalised maps rel-L2 1.108e-3, max reward error 5.302e-3; torch bf16 on the same inputs (stored in the
    fixture): 1.153e-2, 1.141e-2, 7.133e-2."""
    g = golden["depth_reward_hw"]
    gen = _tool("make_depth_hw_golden")
    d, dw, db, m, mw, mb, r, rw, rb = ([] for _ in range(9))
    for i, (name, size, h, w, dtype) in enumerate(gen.CASES):
        model = reduced[size][0]
        oh, ow = (int(v) for v in g[f"{name}_size"])
        pred, target = gen.case_images(i, h, w, dtype)
        imgs = torch.stack([pred, target]).to(DEV)
        depth = model.predicted_depth(imgs)
        assert depth.shape == (2, oh, ow) and depth.dtype == torch.float32
        patches, size_hw = model.preprocess_hw(imgs)
        assert torch.equal(model(pixel_values=model.patches_to_pixel_values(patches, size_hw)).predicted_depth, depth)
        maps = model.normalized_depth(imgs)
        assert maps.shape == (2, h, w) and float(maps.min()) == 0.0 and abs(float(maps.max()) - 1.0) < 1e-6
        assert torch.equal(maps, model.post_process(depth, h, w))
        rew = ppo.calculate_reward("depth", model, model.processor, imgs[:1], imgs[1:], DEV)
        assert rew.shape == (1, 1) and rew.dtype == torch.float32
        bf = torch.from_numpy(g[f"{name}_depth_bf16"].view(np.int16).copy()).view(torch.bfloat16).float()
        d.append(depth.cpu().numpy().ravel()); dw.append(g[f"{name}_depth"].ravel()); db.append(bf.numpy().ravel())
        m.append(maps.cpu().numpy().ravel()); mw.append(g[f"{name}_maps"].ravel()); mb.append(do.normalized_maps(bf, h, w).numpy().ravel())
        r.append(rew.cpu().numpy().ravel()); rw.append(g[f"{name}_reward"].ravel()); rb.append(g[f"{name}_reward_bf16"].ravel())
        print(name, "depth rel-L2", rel_l2(d[-1], dw[-1]), "maps rel-L2", rel_l2(m[-1], mw[-1]), "reward", float(r[-1][0]), "want", float(rw[-1][0]),
              "| bf16:", g[f"{name}_bf16_errors"].tolist())
        # each case on its own is below its stored comparator, and the reward within the square tests' bound
        assert rel_l2(d[-1], dw[-1]) < g[f"{name}_bf16_errors"][0] and rel_l2(m[-1], mw[-1]) < g[f"{name}_bf16_errors"][1], name
        assert abs(float(r[-1][0]) - float(rw[-1][0])) < g[f"{name}_bf16_errors"][2], name
        assert abs(float(r[-1][0]) - float(rw[-1][0])) <= SQUARE_REDUCED_REWARD * 1.1, name
    cat = np.concatenate
    ed, em, er = rel_l2(cat(d), cat(dw)), rel_l2(cat(m), cat(mw)), float(np.abs(cat(r) - cat(rw)).max())
    bd, bm, br = rel_l2(cat(db), cat(dw)), rel_l2(cat(mb), cat(mw)), float(np.abs(cat(rb) - cat(rw)).max())
    print(f"depth reduced, non-square: predicted_depth rel-L2 {ed:.3e} (bf16 {bd:.3e}), maps rel-L2 {em:.3e} (bf16 {bm:.3e}), max reward error {er:.3e} (bf16 {br:.3e})")
    assert ed < bd and em < bm and er < br, (ed, bd, em, bm, er, br)
    assert ed <= MEASURED_REDUCED_DEPTH * 1.1 and em <= MEASURED_REDUCED_MAPS * 1.1 and er <= MEASURED_REDUCED_REWARD * 1.1, (ed, em, er)


def test_square_inputs_through_the_hw_entry_points_are_bit_identical(reduced):
    """patches, the uint8 image, predicted_depth and the maps of square images: the `_hw` entry points give what the square ones give, bit for bit"""
    for size, hw, dtype in ((126, 64, torch.float16), (70, 96, torch.float32), (126, 126, torch.float32)):
        model = reduced[size][0]
        imgs = torch.stack(_pair(520 + hw, hw, hw, dtype)).to(DEV)
        p0, u0 = model.preprocess(imgs, return_crop=True)
        p1, size_hw, u1 = model.preprocess_hw(imgs, return_crop=True)
        assert size_hw == (size, size) and torch.equal(p0, p1) and torch.equal(u0, u1)
        d0, d1 = model.depth_from_patches(p0), model.depth_from_patches_hw(p1, size_hw)
        assert torch.equal(d0, d1)
        lib, out = L.lib(), torch.empty(2, hw + 3, hw, dtype=torch.float32, device=DEV)
        L.check(lib.cs_depth_normalized_maps_hw(model._h, L.ptr(d1), 2, size, size, hw + 3, hw, L.ptr(out), L.stream_ptr(DEV)))
        assert torch.equal(out, model.post_process(d0, hw + 3, hw))
        assert model.flops_hw(2, size_hw) == model.flops(2)


# ---- the full shape ---------------------------------------------------------------------------------------------------------------------------------------
def test_full_size_non_square_matches_fp32_oracle():
    """V2-Small with seeded synthetic weights, one pred / target pair at 512 x 768 fp16: 518 x 784, 37 x 56 tokens, maps 148x224 / 74x112 / 37x56 / 19x28, vs
    tests/depth_oracle_hw.py in fp32 on the CPU (and the same graph in bf16: the class comparator).
    Measured: maps rel-L2 1.846e-3, reward error 4.396e-3 (oracle reward 22.072, zero share 0.33, range 2.60); torch bf16 on the same inputs: 1.638e-2, 4.676e-2."""
    model, proc = load_depth_reward(device=DEV)
    sd = synthetic_depth_anything_state_dict(model.manifest(), seed=7)
    model.load_state_dict(sd)
    pred, target = _pair(300, 512, 768, torch.float16)
    imgs = torch.stack([pred, target])
    assert model.processed_size(512, 768) == (518, 784)
    maps = model.normalized_depth(imgs.to(DEV)).cpu()
    rew = ppo.calculate_reward("depth", model, proc, pred[None].to(DEV), target[None].to(DEV), DEV).cpu()
    assert maps.shape == (2, 512, 768)
    _, pv = dh.preprocess(imgs, 518)
    assert pv.shape == (2, 3, 518, 784)
    want_d = dh.DepthAnythingOracleHW(sd)(pv)
    want = do.normalized_maps(want_d, 512, 768)
    want_r = do.depth_reward(want[:1], want[1:])
    raw = F.interpolate(want_d[:, None], size=(512, 768), mode="bicubic", align_corners=False)[:, 0]
    zero_share, rng = float((raw <= 0).float().mean((1, 2)).max()), float((raw.amax((1, 2)) - raw.amin((1, 2))).min())
    print(f"oracle: zero share {zero_share:.3f}, range {rng:.3f}, reward {float(want_r):.4f}")
    assert zero_share <= 0.5 and rng >= 1.0 and 5.0 < float(want_r) < 40.0              # the oracle is not degenerate
    bf = do.normalized_maps(dh.DepthAnythingOracleHW(sd, dtype=torch.bfloat16)(pv).float(), 512, 768)
    bf_r = do.depth_reward(bf[:1], bf[1:])
    em, er = rel_l2(maps.numpy(), want.numpy()), float((rew - want_r).abs().max())
    bm, br = rel_l2(bf.numpy(), want.numpy()), float((bf_r - want_r).abs().max())
    print(f"depth full size 512 x 768: maps rel-L2 {em:.3e} (bf16 {bm:.3e}), reward error {er:.3e} (bf16 {br:.3e}); reward {float(rew):.4f}")
    assert em < bm and er < br, (em, bm, er, br)
    assert em <= MEASURED_FULL_MAPS * 1.1 and er <= MEASURED_FULL_REWARD * 1.1, (em, er)


# ---- segmentation -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg():
    """the segmentation fixture's reduced model at processor size 128: (HIP model, fp32 oracle)"""
    gen = _tool("make_segformer_golden")
    cfg = gen.reduced_config(128)
    m = HipSegformerModel(cfg, device=DEV)
    sd = gen.state_dict(128)
    m.load_state_dict(sd)
    return m, so.SegformerOracle(sd, cfg)


def _seg_reference(imgs, size):
    """what the Segformer processor does with any image: PIL BILINEAR to size x size, each axis on its own scale"""
    u8 = np.stack([np.ascontiguousarray(so.pil_bilinear_resize(vo.to_uint8_hwc(im), size, size).transpose(2, 0, 1)) for im in imgs])
    return u8, torch.from_numpy(np.stack([vo.normalize_uint8(c, so.PROCESSOR) for c in u8]))


@pytest.mark.parametrize("h,w,dtype", [(64, 96, torch.float16), (200, 120, torch.float32)])
def test_segmentation_front_end_and_reward_on_non_square_images(seg, h, w, dtype):
    """the stretch to 128 x 128 is bit-identical to PIL's Image.resize, pixel_values within 2^-10; the masks and the reward of a non-square pair against the
    fp32 oracle on the same pixels, at the square tests' reward bound (100 x the share of mask pixels that differ from the oracle's); identical images give 100"""
    from PIL import Image
    model, oracle = seg
    imgs = torch.stack(_pair(540 + h, h, w, dtype))
    patches, u8 = model.preprocess_hw(imgs.to(DEV), return_crop=True)
    assert u8.shape == (2, 3, 128, 128) and patches.shape == (2 * 128 * 128, 8)
    want_u8, want_pv = _seg_reference(imgs, 128)
    pil = np.stack([np.asarray(Image.fromarray(vo.to_uint8_hwc(im)).resize((128, 128), Image.BILINEAR)).transpose(2, 0, 1) for im in imgs])
    assert np.array_equal(want_u8, pil) and np.array_equal(u8.cpu().numpy(), pil)
    pv = model.patches_to_pixel_values(patches).float().cpu()
    assert float((pv - want_pv).abs().max()) <= 2.0 ** -10 and bool((patches[:, 3:] == 0).all())
    masks = model.masks(imgs.to(DEV)).cpu().long()
    wm = so.masks(oracle(want_pv))
    share = (masks != wm).float().mean((1, 2))
    rew = ppo.calculate_reward("segmentation", model, model.processor, imgs[:1].to(DEV), imgs[1:].to(DEV), DEV).cpu()
    want_r = so.seg_reward(wm[:1], wm[1:])
    print(f"segmentation {h} x {w}: differing share {share.tolist()}, reward {float(rew):.4f} (oracle {float(want_r):.4f})")
    assert rew.shape == (1, 1) and abs(float(rew) - float(want_r)) <= 100 * float(share.sum()) + 1e-4
    same = calculate_segmentation_reward(model, model.processor, imgs.to(DEV), imgs.to(DEV), DEV)
    assert same.shape == (2, 1) and bool((same == 100.0).all())
    with pytest.raises(RuntimeError, match="square"):          # the square patch-row API keeps its refusal
        model.preprocess(imgs.to(DEV))


# ---- argument forms -----------------------------------------------------------------------------------------------------------------------------------------
def test_argument_forms(reduced):
    model = reduced[126][0]
    proc = model.processor
    h, w = 64, 96
    pairs = [_pair(560 + i, h, w, torch.float16) for i in range(3)]
    pred, target = torch.stack([p for p, _ in pairs]).to(DEV), torch.stack([t for _, t in pairs]).to(DEV)
    r = ppo.calculate_reward("depth", model, proc, pred, target, DEV)
    assert r.shape == (3, 1) and r.dtype == torch.float32 and bool((r > 0).all())
    assert torch.equal(r, calculate_depth_reward(model, proc, pred, target, DEV))
    # identical images: mse = 0 -> 10 log10(1 / 1e-8) = 80
    same = ppo.calculate_reward("depth", model, proc, pred, pred, DEV)
    assert float((same - 80.0).abs().max()) <= 1e-3
    # a [1,3,H,W] target, the fp32 quantisation path, the empty batch
    assert calculate_depth_reward(model, proc, pred, target[:1], DEV).shape == (3, 1)
    assert calculate_depth_reward(model, proc, pred.float(), target, DEV).shape == (3, 1)
    assert ppo.calculate_reward("depth", model, proc, pred[:0], target[:0], DEV).shape == (0, 1)
    assert model.predicted_depth(pred[:0]).shape == (0, 84, 126)
    # a chunked call equals a whole call: the same images in another batch shape (kernels are chosen by the row count, so rounding noise inside the reduced
    # model's bound; measured 0.0), and the first chunk is bit-identical to a call of its own
    both = torch.cat([pred, target])
    whole = model.normalized_depth(both)
    saved, model.max_batch = model.max_batch, 4
    try:
        chunked = model.normalized_depth(both)
        first = model.normalized_depth(both[:4])
    finally:
        model.max_batch = saved
    e = rel_l2(chunked.cpu().numpy(), whole.cpu().numpy())
    print("chunked vs whole: maps rel-L2", e)
    assert e <= 1.1 * MEASURED_REDUCED_MAPS and torch.equal(chunked[:4], first)
    # refusals return before any launch: a size beyond the limit, a workspace too small, NULL pointers
    lib = L.lib()
    with pytest.raises(RuntimeError, match="not implemented"):
        model.predicted_depth(torch.zeros(1, 3, 126, 504, device=DEV))         # stays 126 x 504: 36 patches wide, the limit is 27
    with pytest.raises(RuntimeError, match="not implemented"):
        model(pixel_values=torch.zeros(1, 3, 126, 392, device=DEV))
    with pytest.raises(ValueError):
        model(pixel_values=torch.zeros(1, 3, 126, 100, device=DEV))
    patches, (oh, ow) = model.preprocess_hw(pred)
    need = lib.cs_depth_workspace_bytes_hw(model._h, 3, oh, ow)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((3, oh, ow), -1.0, dtype=torch.float32, device=DEV)
    st = L.stream_ptr(DEV)
    call = lambda p, n, o, w_, nb: lib.cs_depth_forward_hw(model._h, L.ptr(p), n, oh, ow, L.ptr(o), L.ptr(w_), nb, st)
    assert call(patches, 3, out, ws, need - 1) != 0 and b"workspace" in lib.cs_last_error()
    assert call(None, 3, out, ws, need) != 0 and call(patches, 3, None, ws, need) != 0 and call(patches, 3, out, None, need) != 0
    assert lib.cs_depth_forward_hw(None, L.ptr(patches), 3, oh, ow, L.ptr(out), L.ptr(ws), need, st) != 0
    assert call(patches, -1, out, ws, need) != 0
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())                                             # nothing ran
    assert call(patches, 0, out, ws, need) == 0 and call(None, 0, None, None, 0) == 0          # the empty batch
    pw = lib.cs_depth_preprocess_workspace_bytes_hw(model._h, 3, h, w)
    pws = torch.empty(pw, dtype=torch.uint8, device=DEV)
    pre = lambda im, n, p, w_, nb: lib.cs_depth_preprocess_hw(model._h, L.ptr(im), L.CS_F16, n, h, w, None, None, L.ptr(p), None, L.ptr(w_), nb, st)
    assert pre(pred, 3, patches, pws, 16) != 0 and pre(None, 3, patches, pws, pw) != 0 and pre(pred, 3, None, pws, pw) != 0 and pre(pred, 3, patches, None, pw) != 0
    oh2, ow2 = C.c_int(), C.c_int()
    assert lib.cs_depth_preprocess_hw(model._h, None, L.CS_F16, 0, h, w, C.byref(oh2), C.byref(ow2), None, None, None, 0, st) == 0 and (oh2.value, ow2.value) == (oh, ow)
    assert call(patches, 3, out, ws, need) == 0                                  # and the call itself is fine
    torch.cuda.synchronize()
    assert torch.equal(out, model.depth_from_patches_hw(patches, (oh, ow)))
    with pytest.raises(TypeError):
        model.preprocess_hw(pred.bfloat16())


def test_score_image_pairs_with_two_sizes(tmp_path, reduced):
    from consolver_amd import evaluation as ev
    model = reduced[70][0]
    sizes = [(96, 64), (64, 96), (96, 64), (96, 96)]
    for i, (h, w) in enumerate(sizes):
        a = vo.synthetic_image(600 + i, h, w)
        b = (a + 0.1 * i * torch.randn(3, h, w, generator=torch.Generator().manual_seed(i))).clamp(0, 1)
        ev.save_generation(str(tmp_path / "a"), 0, i, a, "p")
        ev.save_generation(str(tmp_path / "b"), 0, i, b, "p")
    pairs = ev.find_image_pairs(str(tmp_path / "a"), str(tmp_path / "b"))
    res = ev.score_image_pairs(pairs, reward_types=("image_psnr", "depth"), batch_size=3, device=DEV, reward_models={"depth": (model, model.processor)})
    assert len(res["depth"]) == 4 and abs(res["depth"][0] - 80.0) < 1e-3 and all(0 < v < 80.0 for v in res["depth"][1:])
    # input order: each score is the one its pair gets on its own
    for i, pair in enumerate(pairs):
        alone = ev.score_image_pairs([pair], reward_types=("depth",), device=DEV, reward_models={"depth": (model, model.processor)})["depth"][0]
        assert abs(alone - res["depth"][i]) <= 1.1 * SQUARE_REDUCED_REWARD, (i, alone, res["depth"][i])
    with pytest.raises(ValueError, match="differ in size"):
        ev.score_image_pairs([(pairs[0][0], pairs[1][1])], reward_types=("depth",), device=DEV, reward_models={"depth": (model, model.processor)})
