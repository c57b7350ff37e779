"""Depth Anything depth-PSNR reward (reward_type "depth", edit_ppo/reward_model.py:92-96, 359-422) on the HIP library, everything through the C ABI: the kernels
of dpt_ops.hip one by one against torch in fp32, the image front end against the committed PIL / transformers fixture, the model and the reward against the
fixture (reduced model, two processor sizes) and against tests/depth_oracle.py in fp32 (full V2-Small shape, synthetic weights), and the reward's argument forms.

Op-level bounds, derived: every kernel accumulates in fp32 and rounds ONCE to fp16 on the store, the operands of the reference are the same fp16 values, so an
output element v carries a relative error of at most 2^-11 (half an fp16 ulp) plus fp32 summation noise (<= K 2^-24 of the terms' magnitude: 1e-4 of the former
at K = 3456).  Hence rel-L2 <= 2^-11 = 4.9e-4, asserted as 5e-4, and max |error| <= (2^-11 + 2^-15) max |reference|.  The fp32 kernels (bicubic, normalise)
differ from torch by the order of a handful of fp32 operations: 1e-5 / 1e-6 of the value range.

Model-level bounds: the figures measured on an MI355X + 10 % (the suite's convention; the measured values are in the docstrings of the tests that assert them),
and each figure must also be smaller than the error of the same graph evaluated by torch in bf16 on the same inputs.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from consolver_amd import _lib as L
from consolver_amd import ops, ppo
from consolver_amd.reward_model import DepthImageProcessor, HipDepthAnythingModel, calculate_depth_reward, load_depth_reward
from consolver_amd.synth import synthetic_depth_anything_state_dict
from tests import depth_oracle as do
from tests import vit_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_REL_L2 = 5e-4                       # one fp16 rounding of an fp32-accumulated value: 2^-11 = 4.9e-4
F16_MAX_REL = 2.0 ** -11 + 2.0 ** -15   # ... per element, relative to the largest reference magnitude

# measured on an MI355X (see the docstrings of the two parity tests); the asserted bounds are these + 10 %
MEASURED_REDUCED_DEPTH, MEASURED_REDUCED_MAPS, MEASURED_REDUCED_REWARD = 1.106e-3, 1.034e-3, 6.966e-3       # torch bf16 on the same inputs: 1.102e-2, 1.112e-2, 8.070e-2
MEASURED_FULL_MAPS, MEASURED_FULL_REWARD = 2.473e-3, 6.477e-3                                                # torch bf16 on the same inputs: 1.546e-2, 8.171e-3


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _generator():
    spec = importlib.util.spec_from_file_location("make_depth_golden", os.path.join(ROOT, "tools", "make_depth_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_f16(got, want, what):
    got, want = got.float().cpu(), want.float()
    e, m = rel_l2(got.numpy(), want.numpy()), float((got - want).abs().max())
    print(what, f"rel-L2 {e:.3e} max abs {m:.3e} (max |ref| {float(want.abs().max()):.3f})")
    assert e <= F16_REL_L2, (what, e)
    assert m <= F16_MAX_REL * float(want.abs().max()) + 1e-7, (what, m)


# ---- op level ---------------------------------------------------------------------------------------------------------------------------------------
def _dpt_conv(x, w, bias, taps, relu_in, relu_out, res, res2):
    """x [B,H,W,Cin] fp16 NHWC, w [Cout, taps, Cin] fp16 -> [B,H,W,Cout] fp16 through cs_op_dpt_conv"""
    B, H, W, Cin = x.shape
    out = torch.empty(B, H, W, w.shape[0], dtype=torch.float16, device=x.device)
    L.check(L.lib().cs_op_dpt_conv(L.ptr(x), B, H, W, Cin, L.ptr(w), L.ptr(bias), w.shape[0], taps, int(relu_in), int(relu_out), L.ptr(res), L.ptr(res2),
                                   L.ptr(out), L.stream_ptr(x.device)))
    return out


CONV_CHANNELS = ((32, 32, 32), (64, 64, 32), (64, 64, 64), (192, 192, 64), (384, 384, 64), (48, 64, 64))      # (Cin, Cin as stored, Cout): 48 is zero-padded to 64
CONV_FLAGS = ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 1, 1, 1, 1))   # relu_in, bias, res, res2, relu_out


@pytest.mark.parametrize("H,W", [(3, 3), (5, 5), (9, 9), (19, 19), (37, 37), (20, 36)])
def test_narrow_conv_matches_torch(H, W):
    """cs_op_dpt_conv (3x3 pad 1 and the one-tap form) vs F.conv2d in fp32 on the fp16-rounded operands: B = 2, sizes that are no multiple of the 16-pixel MFMA
    tile or of the 128-pixel workgroup (B H W = 18 .. 2738: a part of one tile, and 22 workgroups with a ragged last one), every (Cin, Cout) the neck has, each
    epilogue flag alone and all together."""
    B = 2
    g = torch.Generator().manual_seed(H * 100 + W)
    for cin, cpad, cout in CONV_CHANNELS:
        x = torch.zeros(B, cpad, H, W)
        x[:, :cin] = torch.randn(B, cin, H, W, generator=g)
        x = x.half()
        res, res2 = (torch.randn(B, cout, H, W, generator=g).half() for _ in range(2))
        bias = torch.randn(cout, generator=g).half()
        xd, rd, r2d, bd = x.permute(0, 2, 3, 1).contiguous().to(DEV), res.permute(0, 2, 3, 1).contiguous().to(DEV), res2.permute(0, 2, 3, 1).contiguous().to(DEV), bias.to(DEV)
        for taps in (9, 1):
            k = 3 if taps == 9 else 1
            w = (torch.randn(cout, cin, k, k, generator=g) * (cin * taps) ** -0.5).half()
            wp = torch.zeros(cout, taps, cpad, dtype=torch.float16)
            wp[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, taps, cin)
            wd = wp.to(DEV)
            conv = {ri: F.conv2d(F.relu(x[:, :cin].float()) if ri else x[:, :cin].float(), w.float(), None, padding=k // 2) for ri in (0, 1)}
            for ri, hb, hr, hr2, ro in CONV_FLAGS:
                want = conv[ri] + (bias.float()[None, :, None, None] if hb else 0) + (res.float() if hr else 0) + (res2.float() if hr2 else 0)
                want = F.relu(want) if ro else want
                got = _dpt_conv(xd, wd, bd if hb else None, taps, ri, ro, rd if hr else None, r2d if hr2 else None)
                _check_f16(got.permute(0, 3, 1, 2), want, f"conv {H}x{W} {cin}->{cout} taps {taps} flags {(ri, hb, hr, hr2, ro)}")


@pytest.mark.parametrize("si,so,C", [(5, 9, 64), (9, 18, 64), (72, 126, 32)])
def test_bilinear_align_corners_matches_torch(si, so, C):
    g = torch.Generator().manual_seed(si)
    x = torch.randn(2, C, si, si, generator=g).half()
    want = F.interpolate(x.float(), size=(so, so), mode="bilinear", align_corners=True)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.empty(2, so, so, C, dtype=torch.float16, device=DEV)
    L.check(L.lib().cs_op_dpt_bilinear(L.ptr(xd), 2, si, si, C, so, so, L.ptr(out), L.stream_ptr(DEV)))
    _check_f16(out.permute(0, 3, 1, 2), want, f"bilinear {si}->{so}")


@pytest.mark.parametrize("so", [64, 200])
def test_bicubic_and_normalise_match_torch(so):
    """cs_op_dpt_bicubic vs F.interpolate(bicubic, align_corners=False) on fp32 maps 126 -> 64 (down, no antialias) and 126 -> 200, then the min / max
    normalisation; a ReLU-ed input, as the head's output is"""
    g = torch.Generator().manual_seed(so)
    x = F.relu(torch.randn(2, 126, 126, generator=g) + 0.3) * 3
    want = F.interpolate(x[:, None], size=(so, so), mode="bicubic", align_corners=False)[:, 0]
    xd = x.to(DEV)
    out = torch.empty(2, so, so, dtype=torch.float32, device=DEV)
    L.check(L.lib().cs_op_dpt_bicubic(L.ptr(xd), 2, 126, 126, so, so, L.ptr(out), L.stream_ptr(DEV)))
    e = float((out.cpu() - want).abs().max())
    print(f"bicubic 126->{so}: max abs error {e:.3e} (max |ref| {float(want.abs().max()):.3f})")
    assert e <= 1e-5 * float(want.abs().max())
    mn, mx = want.amin((1, 2), keepdim=True), want.amax((1, 2), keepdim=True)
    wantn = (want - mn) / (mx - mn + 1e-8)
    nd = want.to(DEV).contiguous()
    L.check(L.lib().cs_op_dpt_minmax_normalize(L.ptr(nd), 2, so * so, L.stream_ptr(DEV)))
    en = float((nd.cpu() - wantn).abs().max())
    print(f"normalise {so}^2: max abs error {en:.3e}")
    assert en <= 1e-6 and float(nd.min()) == 0.0 and float(nd.max()) <= 1.0


@pytest.mark.parametrize("G", [5, 9])
def test_pixel_shuffle_reassemble_matches_conv_transpose(G):
    """a kernel = stride transposed conv as ONE linear layer + the pixel-shuffle store: cs_op_linear over the token rows (CLS row included, as the executor runs
    it) with the weight rows ordered (ky, kx, out channel), then cs_op_dpt_pixel_shuffle, vs F.conv_transpose2d in fp32 on the same fp16 operands (a map from the
    token's D = 128 channels to the k x k output pixels' C, which is what the projection folded into the transposed conv is); k = 4 with 64 channels and k = 2
    with 96 (the two reassemble layers), and k = 1 (dropping the CLS rows) exactly."""
    g = torch.Generator().manual_seed(G)
    B, T, D = 2, G * G + 1, 128
    for k, C in ((4, 64), (2, 96)):
        tok = torch.randn(B, T, D, generator=g).half()
        wt = (torch.randn(D, C, k, k, generator=g) * D ** -0.5).half()           # ConvTranspose2d: [in, out, k, k]
        bias = torch.randn(C, generator=g).half()
        want = F.conv_transpose2d(tok[:, 1:].float().reshape(B, G, G, D).permute(0, 3, 1, 2), wt.float(), bias.float(), stride=k)
        wf = wt.permute(2, 3, 1, 0).reshape(k * k * C, D).contiguous()            # row (ky k + kx) C + co, column ci
        y = ops.linear(tok.reshape(B * T, D).to(DEV), wf.to(DEV), bias.repeat(k * k).to(DEV))
        out = torch.empty(B, G * k, G * k, C, dtype=torch.float16, device=DEV)
        L.check(L.lib().cs_op_dpt_pixel_shuffle(L.ptr(y), B, G, k, C, 1, L.ptr(out), L.stream_ptr(DEV)))
        _check_f16(out.permute(0, 3, 1, 2), want, f"reassemble grid {G} k {k}")
    tok = torch.randn(B, T, 192, generator=g).half().to(DEV)
    out = torch.empty(B, G, G, 192, dtype=torch.float16, device=DEV)
    L.check(L.lib().cs_op_dpt_pixel_shuffle(L.ptr(tok), B, G, 1, 192, 1, L.ptr(out), L.stream_ptr(DEV)))
    assert torch.equal(out.reshape(B, G * G, 192), tok[:, 1:])


def test_head_projection_matches_torch():
    g = torch.Generator().manual_seed(3)
    M, C = 2 * 37 * 37 + 5, 32
    x, w, b = torch.randn(M, C, generator=g).half(), (torch.randn(C, generator=g) * C ** -0.5).half(), torch.tensor([0.1]).half()
    want = F.relu(x.float() @ w.float() + b.float()) * 2.5
    out = torch.empty(M, dtype=torch.float32, device=DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    L.check(L.lib().cs_op_dpt_head(L.ptr(xd), M, C, L.ptr(wd), L.ptr(bd), 2.5, L.ptr(out), L.stream_ptr(DEV)))
    assert float((out.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())              # fp32 sums of 32 exact products in another order


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reduced():
    """the fixture's reduced model at its two processor sizes"""
    gen = _generator()
    out = {}
    for size in (126, 70):
        m = HipDepthAnythingModel(gen.reduced_config(size), device=DEV)
        assert m.manifest() == do.manifest(gen.reduced_config(size))
        m.load_state_dict(gen.state_dict(size))
        out[size] = m
    return out


def test_front_end_is_bit_identical_to_pil(golden, reduced):
    g = golden["depth_reward"]
    gen = _generator()
    for i, (name, size, hw, dtype) in enumerate(gen.CASES):
        pred, target = gen.case_images(i, hw, dtype)
        patches, u8 = reduced[size].preprocess(torch.stack([pred, target]).to(DEV), return_crop=True)
        assert u8.dtype == torch.uint8 and u8.shape == (2, 3, size, size) and patches.shape == (2 * (size // 14) ** 2, 640)
        assert np.array_equal(u8[0].cpu().numpy(), g[f"{name}_u8"]), name
        want_u8, want_pv = do.preprocess(torch.stack([pred, target]), size)
        assert np.array_equal(u8.cpu().numpy(), want_u8), name
        pv = reduced[size].patches_to_pixel_values(patches).float().cpu()
        assert float((pv - want_pv).abs().max()) <= 2.0 ** -10, name              # the fp16 half-ulp at |v| < 4
    with pytest.raises(RuntimeError, match="square"):
        reduced[126].preprocess(torch.zeros(1, 3, 64, 96, device=DEV))


def test_reduced_model_matches_transformers_fixture(golden, reduced):
    """HIP (fp16 storage, fp32 accumulation) vs transformers DepthAnythingForDepthEstimation + post_process_depth_estimation in fp32 on the reduced config, images
    through the whole path (front end included), the four fixture cases taken together.
    Measured: predicted_depth rel-L2 1.106e-3, normalised maps rel-L2 1.034e-3, max reward error 6.966e-3; torch bf16 on the same inputs (stored in the
    fixture): 1.102e-2, 1.112e-2, 8.070e-2."""
    g = golden["depth_reward"]
    gen = _generator()
    d, dw, db, m, mw, mb, r, rw, rb = ([] for _ in range(9))
    for i, (name, size, hw, dtype) in enumerate(gen.CASES):
        model = reduced[size]
        pred, target = gen.case_images(i, hw, dtype)
        imgs = torch.stack([pred, target]).to(DEV)
        depth = model.predicted_depth(imgs)
        assert depth.shape == (2, size, size) and depth.dtype == torch.float32
        assert torch.equal(model(pixel_values=model.patches_to_pixel_values(model.preprocess(imgs))).predicted_depth, depth)
        maps = model.normalized_depth(imgs)
        assert maps.shape == (2, hw, hw) and float(maps.min()) == 0.0 and abs(float(maps.max()) - 1.0) < 1e-6
        rew = calculate_depth_reward(model, None, imgs[:1], imgs[1:], DEV)
        assert rew.shape == (1, 1) and rew.dtype == torch.float32
        bf = torch.from_numpy(g[f"{name}_depth_bf16"].view(np.int16).copy()).view(torch.bfloat16).float()
        d.append(depth.cpu().numpy().ravel()); dw.append(g[f"{name}_depth"].ravel()); db.append(bf.numpy().ravel())
        m.append(maps.cpu().numpy().ravel()); mw.append(g[f"{name}_maps"].ravel()); mb.append(do.normalized_maps(bf, hw, hw).numpy().ravel())
        r.append(rew.cpu().numpy().ravel()); rw.append(g[f"{name}_reward"].ravel()); rb.append(g[f"{name}_reward_bf16"].ravel())
        print(name, "depth rel-L2", rel_l2(d[-1], dw[-1]), "maps rel-L2", rel_l2(m[-1], mw[-1]), "reward", float(r[-1][0]), "want", float(rw[-1][0]),
              "| bf16:", g[f"{name}_bf16_errors"].tolist())
    cat = np.concatenate
    ed, em, er = rel_l2(cat(d), cat(dw)), rel_l2(cat(m), cat(mw)), float(np.abs(cat(r) - cat(rw)).max())
    bd, bm, br = rel_l2(cat(db), cat(dw)), rel_l2(cat(mb), cat(mw)), float(np.abs(cat(rb) - cat(rw)).max())
    print(f"depth reduced: predicted_depth rel-L2 {ed:.3e} (bf16 {bd:.3e}), maps rel-L2 {em:.3e} (bf16 {bm:.3e}), max reward error {er:.3e} (bf16 {br:.3e})")
    assert ed < bd and em < bm and er < br, (ed, bd, em, bm, er, br)
    assert ed <= MEASURED_REDUCED_DEPTH * 1.1 and em <= MEASURED_REDUCED_MAPS * 1.1 and er <= MEASURED_REDUCED_REWARD * 1.1, (ed, em, er)


@pytest.fixture(scope="module")
def full():
    """the Depth-Anything-V2-Small shape with seeded synthetic weights"""
    model, proc = load_depth_reward(device=DEV)
    sd = synthetic_depth_anything_state_dict(model.manifest(), seed=7)
    model.load_state_dict(sd)
    return model, proc, sd


def _full_pair(i=0, amp=0.15):
    p = vo.synthetic_image(300 + i, 512, 512, torch.float16)
    g = torch.Generator().manual_seed(400 + i)
    return p, (p.float() + amp * torch.randn(3, 512, 512, generator=g)).clamp(0, 1).half()


def test_full_size_matches_fp32_oracle(full):
    """one pred / target pair at 512^2 fp16 through the front end, the 12-layer backbone at 1370 tokens, the neck at 148 / 74 / 37 / 19, the head at 518^2 and the
    post-processing, vs tests/depth_oracle.py in fp32 on the CPU (and the same graph in bf16: the class comparator).
    Measured: maps rel-L2 2.473e-3, reward error 6.477e-3 (oracle reward 21.916, zero share 0.34, range 2.36); torch bf16 on the same inputs: 1.546e-2, 8.171e-3."""
    model, proc, sd = full
    pred, target = _full_pair()
    imgs = torch.stack([pred, target])
    maps = model.normalized_depth(imgs.to(DEV)).cpu()
    rew = ppo.calculate_reward("depth", model, proc, pred[None].to(DEV), target[None].to(DEV), DEV).cpu()
    _, pv = do.preprocess(imgs, 518)
    want_d = do.DepthAnythingOracle(sd)(pv)
    want = do.normalized_maps(want_d, 512, 512)
    want_r = do.depth_reward(want[:1], want[1:])
    raw = F.interpolate(want_d[:, None], size=(512, 512), mode="bicubic", align_corners=False)[:, 0]
    zero_share, rng = float((raw <= 0).float().mean((1, 2)).max()), float((raw.amax((1, 2)) - raw.amin((1, 2))).min())
    print(f"oracle: zero share {zero_share:.3f}, range {rng:.3f}, reward {float(want_r):.4f}")
    assert zero_share <= 0.5 and rng >= 1.0 and 5.0 < float(want_r) < 40.0              # the oracle is not degenerate
    bf = do.normalized_maps(do.DepthAnythingOracle(sd, dtype=torch.bfloat16)(pv).float(), 512, 512)
    bf_r = do.depth_reward(bf[:1], bf[1:])
    em, er = rel_l2(maps.numpy(), want.numpy()), float((rew - want_r).abs().max())
    bm, br = rel_l2(bf.numpy(), want.numpy()), float((bf_r - want_r).abs().max())
    print(f"depth full size: maps rel-L2 {em:.3e} (bf16 {bm:.3e}), reward error {er:.3e} (bf16 {br:.3e}); reward {float(rew):.4f}")
    assert em < bm and er < br, (em, bm, er, br)
    assert em <= MEASURED_FULL_MAPS * 1.1 and er <= MEASURED_FULL_REWARD * 1.1, (em, er)
    assert abs(model.flops(1) / 1e9 - 117.0) < 1.0


def test_argument_forms(reduced):
    model = reduced[126]
    proc = model.processor
    gen = _generator()
    pairs = [gen.case_images(i, 64, "float16") for i in range(3)]
    pred, target = torch.stack([p for p, _ in pairs]).to(DEV), torch.stack([t for _, t in pairs]).to(DEV)
    r = ppo.calculate_reward("depth", model, proc, pred, target, DEV)
    assert r.shape == (3, 1) and r.dtype == torch.float32 and bool((r > 0).all())
    # bit-identical across two calls
    assert torch.equal(r, ppo.calculate_reward("depth", model, proc, pred, target, DEV))
    # a [1,3,H,W] target == the tiled target.  The same image in another batch: the GEMM / attention kernels are chosen by the row count, so not bit-identical
    # by contract; the difference is rounding noise inside the reduced model's reward bound
    shared = calculate_depth_reward(model, proc, pred, target[:1], DEV)
    tiled = calculate_depth_reward(model, proc, pred, target[:1].expand(3, -1, -1, -1).contiguous(), DEV)
    print("shared vs tiled target", shared.flatten().tolist(), tiled.flatten().tolist(), "max difference", float((shared - tiled).abs().max()))
    assert float((shared - tiled).abs().max()) <= 1.1 * MEASURED_REDUCED_REWARD                 # measured: 0.0
    # fp32 images take the fp32 quantisation path; mixed dtypes run two passes
    assert calculate_depth_reward(model, proc, pred.float(), target, DEV).shape == (3, 1)
    # B = 0
    assert ppo.calculate_reward("depth", model, proc, pred[:0], target[:0], DEV).shape == (0, 1)
    # identical images: mse = 0 -> 10 log10(1 / 1e-8) = 80, no upper clamp
    same = ppo.calculate_reward("depth", model, proc, pred, pred, DEV)
    assert float((same - 80.0).abs().max()) <= 1e-3
    # a batch larger than max_batch == the chunked result
    whole = model.normalized_depth(torch.cat([pred, target]))
    saved, model.max_batch = model.max_batch, 4
    try:
        chunked = model.normalized_depth(torch.cat([pred, target]))
    finally:
        model.max_batch = saved
    e = rel_l2(chunked.cpu().numpy(), whole.cpu().numpy())
    print("chunked vs whole: maps rel-L2", e)
    assert e <= 1.1 * MEASURED_REDUCED_MAPS                     # other batch shapes for the same images, as above; measured: 0.0
    assert torch.equal(chunked[:4], model.normalized_depth(torch.cat([pred, target])[:4]))
    with pytest.raises(TypeError):
        ppo.calculate_reward("depth", model, proc, pred.bfloat16(), target.bfloat16(), DEV)
    with pytest.raises(NotImplementedError):
        ppo.calculate_reward("depth", None, None, pred, target, DEV)
    with pytest.raises(ValueError):
        ppo.calculate_reward("depth", model, DepthImageProcessor({"height": 70, "width": 70}), pred, target, DEV)
    with pytest.raises(RuntimeError):
        model.to("cpu")
    assert model.to(DEV) is model and model.eval() is model


def test_score_image_pairs_with_depth(tmp_path, reduced):
    from consolver_amd import evaluation as ev
    model = reduced[70]
    for i in range(3):
        a = vo.synthetic_image(600 + i, 96, 96)
        b = (a + 0.1 * i * torch.randn(3, 96, 96, generator=torch.Generator().manual_seed(i))).clamp(0, 1)
        ev.save_generation(str(tmp_path / "a"), 0, i, a, "p")
        ev.save_generation(str(tmp_path / "b"), 0, i, b, "p")
    pairs = ev.find_image_pairs(str(tmp_path / "a"), str(tmp_path / "b"))
    res = ev.score_image_pairs(pairs, reward_types=("image_psnr", "depth"), batch_size=2, device=DEV, reward_models={"depth": (model, model.processor)})
    assert len(res["depth"]) == 3 and abs(res["depth"][0] - 80.0) < 1e-3 and all(0 < v < 80.0 for v in res["depth"][1:])
    with pytest.raises(NotImplementedError):
        ev.score_image_pairs(pairs, reward_types=("depth",), device=DEV)
