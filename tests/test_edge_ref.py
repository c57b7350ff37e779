"""tests/edge_ref.py on the CPU: every float64 reference against independent torch code, and every emulator against the bound its GPU test
(tests/test_edge_ops_gpu.py) states, on exactly the case lists and inputs that test uses -- so that a bound missed on the GPU is the kernel's doing, not the
reference's."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import edge_ref as R


def close(a, b, tol=1e-12):
    return float((a.double() - b.double()).abs().max()) <= tol * max(1.0, float(b.double().abs().max()))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# ---- references against independent torch code ------------------------------------------------------------------------------------------------------------------
def test_sinusoid_is_the_diffusers_timestep_embedding():
    """diffusers get_timestep_embedding(flip_sin_to_cos=True, downscale_freq_shift=0, scale=1, max_period=10000), in float64"""
    for C0 in (320, 32):
        t = R.timesteps(5)
        half = C0 // 2
        exponent = -math.log(10000) * torch.arange(0, half, dtype=torch.float64) / (half - 0)
        emb = t.double()[:, None] * torch.exp(exponent)[None, :]
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=-1)
        emb = torch.cat([emb[:, half:], emb[:, :half]], dim=-1)
        ref = R.sinusoid_fp64(t, C0)
        assert close(ref, emb)
        assert bool((ref[0, :half] == 1).all()) and bool((ref[0, half:] == 0).all())                  # t = 0: cos | sin
        # an fp32 evaluation, stored fp16, passes the acceptance rule per row and per frequency
        f = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * torch.arange(half, dtype=torch.float32) / half)
        a32 = t[:, None] * f[None, :]
        got = torch.cat((torch.cos(a32), torch.sin(a32)), -1).to(R.F16).double()
        emu = R.rnd(ref)
        for dim in (-1, 0):
            assert bool(((got - ref).abs().amax(dim) <= R.rule_bound(ref, emu, dim)).all())


def test_time_embedding_is_two_linear_layers_with_silu():
    for C0, D in R.TIME_DIMS:
        w1, b1, w2, b2 = R.time_weights(C0, D, C0)
        t = R.timesteps(5)
        emb, h1, out = R.time_embedding_fp64(t, C0, w1, b1, w2, b2)
        want = F.silu(F.linear(F.silu(F.linear(emb, w1.double(), b1.double())), w2.double(), b2.double()))
        assert close(out, want)
        e_emb, e_h1, e_out = R.time_embedding_emulated(t, C0, w1, b1, w2, b2)
        for e in (e_emb, e_h1, e_out):
            assert torch.equal(e, e.to(R.F16).double())                                                 # every stage is an fp16 tensor
        assert float((e_out - out).abs().max()) < 4e-3 * float(out.abs().max())


def test_rowvec_linear_reference_and_the_negative_row():
    for K in R.ROWVEC_K:
        x, w, b = R.rowvec_inputs(K, 5, 3, K)
        assert close(R.rowvec_linear_fp64(x, w, b, False), F.linear(x.double(), w.double(), b.double()))
        assert close(R.rowvec_linear_fp64(x, w, None, True), F.silu(F.linear(x.double(), w.double())))
        x, w, _ = R.rowvec_negative_inputs(K, 5)
        pre = R.rowvec_linear_fp64(x, w, None, False)
        assert float(pre.max()) < -29 and float(pre.min()) > -31
        out = R.rnd(R.rowvec_linear_fp64(x, w, None, True))
        assert bool((out == 0).all()) and bool(torch.signbit(out.to(R.F16)).all())                     # tiny and negative: -0 in fp16


@pytest.mark.parametrize("n_lat,B", R.CONV_IN_LAT)
def test_conv_in_reference_is_conv2d_of_latent_b_mod_n(n_lat, B):
    for (H, W) in R.CONV_IN_HW:
        for integer in (True, False):
            lat, w, bias = R.conv_in_inputs(n_lat, B, H, W, 8, 7, integer)
            ref = R.conv_in_fp64(lat, n_lat, B, w, bias)
            want = F.conv2d(lat[:n_lat].double()[torch.arange(B) % n_lat], w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
            assert close(ref, want)
            if n_lat < B:                                                                               # reading sample b instead is a gross error
                wrong = F.conv2d(lat.double(), w.double(), bias.double(), padding=1).permute(0, 2, 3, 1)
                assert float((wrong - ref).abs().amax((1, 2, 3)).max()) > 1.0


@pytest.mark.parametrize("Cout", R.CONV_IN_COUT)
def test_conv_in_integer_sums_are_exact_and_two_planes_hold_21_bits(Cout):
    for n_lat, B in R.CONV_IN_LAT:
        for (H, W) in R.CONV_IN_HW:
            lat, w, bias = R.conv_in_inputs(n_lat, B, H, W, Cout, 100 * H + W + B, True)
            ref = R.conv_in_fp64(lat, n_lat, B, w, bias)
            hi, lo = R.conv_in_emulated(ref)
            assert float(ref.abs().max()) <= 2048 and torch.equal(hi, ref) and bool((lo == 0).all())
            lat, w, bias = R.conv_in_inputs(n_lat, B, H, W, Cout, 100 * H + W + B, False)
            ref = R.conv_in_fp64(lat, n_lat, B, w, bias)
            hi, lo = R.conv_in_emulated(ref)
            assert bool(((hi + lo - ref).abs().amax(-1) <= 2.0 ** -21 * ref.abs().amax(-1)).all())


def test_conv_in_grid_stride_case_is_exact():
    n_lat, B, H, W, Cout = R.CONV_IN_STRIDE_CASE
    assert B * H * W > 4096 * 256
    lat, w, bias = R.conv_in_inputs(n_lat, B, H, W, Cout, 3, True)
    ref = R.conv_in_fp64(lat, n_lat, B, w, bias, torch.float32)
    assert float(ref.abs().max()) <= 2048 and torch.equal(ref, ref.round())


def test_embed_reference_clamps_and_wraps():
    ids, tok, pos = R.embed_inputs(7, 3, 8, 1)
    assert {-1, R.EMBED_VOCAB, 2 ** 40, 0, R.EMBED_VOCAB - 1} <= set(ids.tolist())
    out = R.embed_tokens_ref(ids, tok, pos)
    for r, i in enumerate(ids.tolist()):
        want = (tok[min(max(i, 0), R.EMBED_VOCAB - 1)].double() + pos[r % 7].double()).to(R.F16)
        assert torch.equal(out[r], want)


@pytest.mark.parametrize("n", R.GELU_N)
def test_gelu_references_and_element_bound(n):
    x = R.gelu_inputs(n)
    assert x.numel() == n
    fin = x.double().abs() < 1e4
    assert close(R.gelu_erf_fp64(x)[fin], F.gelu(x.double())[fin])
    assert close(R.quick_gelu_fp64(x), x.double() * torch.sigmoid(1.702 * x.double()))
    for ref in (R.gelu_erf_fp64(x), R.quick_gelu_fp64(x)):
        assert bool(torch.isfinite(ref).all())
        assert bool(((R.rnd(ref) - ref).abs() <= R.gelu_element_bound(x, ref)).all())
    # the fp32 formula 0.5 x (1 + erf(x / sqrt 2)) as torch evaluates it stays inside the element bound too (the tail where 1 + erf cancels)
    g32 = (0.5 * x.float() * (1.0 + torch.erf(x.float() * 0.70710678118654752))).to(R.F16).double()
    assert bool(((g32 - R.gelu_erf_fp64(x)).abs() <= R.gelu_element_bound(x, R.gelu_erf_fp64(x))).all())


@pytest.mark.parametrize("cols", R.SOFTMAX_REG_COLS + R.SOFTMAX_BLOCK_COLS)
def test_softmax_reference_and_sum_bound(cols):
    rows = 2
    for scale in R.SOFTMAX_SCALES:
        for kind in R.SOFTMAX_KINDS:
            x = R.softmax_rows(rows, cols, scale, kind, cols)
            ref = R.row_softmax_fp64(x, scale)
            assert close(ref, torch.softmax(x.double() * R.f32(scale), -1))
            emu = R.rnd(ref)
            assert bool(torch.isfinite(emu).all()) and float(emu.min()) >= 0 and float(emu.max()) <= 1
            assert bool(((emu.sum(-1) - 1).abs() <= R.softmax_sum_bound(ref)).all())
            assert bool((R.softmax_sum_bound(ref) <= 0.5 * cols * R.ulp_at(ref.amax(-1)) + 2.0 ** -15).all())
            if kind == "constant":
                assert bool((emu == R.rnd(torch.tensor(1.0 / cols, dtype=torch.float64))).all())
            if kind.startswith("peak"):
                top = ref.argmax(-1)
                assert float(ref.amax(-1).min()) > 0.99 and int(top[0]) == {"peak_first": 0, "peak_last": cols - 1, "peak_mid": min(cols - 1, 515)}[kind]


def test_pixel_references():
    x, w, b = R.pixel_inputs(2, 16, 257, 16, 1)
    want = F.conv2d((x.double() * R.f32(R.SD_SCALE) + R.f32(0.25)).reshape(2, 16, 257, 1), w.double()[:, :, None, None], b.double()).reshape(2, 16, 257)
    assert close(R.pixel_linear_fp64(x, w, b, R.SD_SCALE, 0.25), want)
    assert close(R.latent_fp64(x, w, b, R.SD_SCALE, 0.25), want.transpose(1, 2))
    assert torch.equal(R.latent_fp64(x, None, None, 1.0, 0.0), x.double().transpose(1, 2))
    for form, Cin, Cout in R.AFFINE_FORMS:
        x, w, b = R.pixel_inputs(2, Cin, 257, Cout, 2)
        ww, bb = (w, b) if form == "w" else (None, None)
        ref = R.pixel_affine_fp64(x, Cout, ww, bb, R.AFFINE_SCALE, R.AFFINE_SHIFT)
        acc = F.conv2d(x.double().reshape(2, Cin, 257, 1), w.double()[:, :, None, None], b.double()).reshape(2, Cout, 257) if form == "w" else x.double()[:, :Cout]
        assert close(ref, (acc - 1.5) * 0.5)
        other = acc * 0.5 - 1.5                                                                          # the other order is far outside the acceptance bound
        assert float((other - ref).abs().min()) > 100 * float(R.rule_bound(ref, R.rnd(ref)).max())


@pytest.mark.parametrize("case", R.CONV_DOWN_CASES)
def test_conv_down_reference_is_the_padded_stride2_conv(case):
    B, H, W, Cin, N = case
    for integer in (True, False):
        x, w, bias = R.conv_down_inputs(*case, 5, integer)
        xn = x.double().permute(0, 3, 1, 2)
        ref = R.conv_down_fp64(x, w, bias)
        assert ref.shape == (B, H // 2, W // 2, N)
        assert close(ref, F.conv2d(F.pad(xn, (0, 1, 0, 1)), w.double(), bias.double(), stride=2).permute(0, 2, 3, 1))
        sym = R.conv_down_fp64(x, w, bias, pad_lo=1)
        assert close(sym, F.conv2d(xn, w.double(), bias.double(), stride=2, padding=1).permute(0, 2, 3, 1))
        if integer:
            assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 2048
            assert torch.equal(R.conv_down_fp64(x, w, bias, dtype=torch.float32).double(), ref)
        else:                                                                                           # the symmetric pad is another function altogether
            assert rel_l2(sym, ref) > 10 * 1e-3 and float((sym - ref).abs().max()) > 10 * 4e-3 * float(ref.abs().max())


@pytest.mark.parametrize("C", R.GN_SPLIT_C)
def test_group_norm_reference_and_split_order_emulator(C):
    for HW in R.GN_SPLIT_HW:
        assert R.gn_splits(HW, 256) == {9: 1, 64: 64, 576: 64, 1600: 64, 4096: 256}[HW]
        for dc in (False, True):
            x0, _, g, b = R.gn_inputs(2, HW, C, 0, HW + C, dc)
            ref = R.group_norm_fp64(x0, 32, g, b, 1e-6, True)
            assert close(ref, F.silu(F.group_norm(x0.double().transpose(1, 2), 32, g.double(), b.double(), 1e-6)).transpose(1, 2), 1e-10)
            emu = R.gn_emulated(x0, None, 32, g, b, 1e-6, True, 256)
            assert rel_l2(emu, ref) < 1e-3 and float((emu - ref).abs().max()) < 6e-3
            if dc:                                                                                      # |mean| / sigma of every group is about 20
                xg = x0.double().reshape(2, HW, 32, C // 32)
                assert float((xg.mean((1, 3)).abs() / xg.std((1, 3))).min()) > 10


@pytest.mark.parametrize("c0,c1", R.GN_TABLE_C)
def test_group_norm_emulator_two_sources(c0, c1):
    for HW in R.GN_TABLE_HW:
        for dc in (False, True):
            x0, x1, g, b = R.gn_inputs(2, HW, c0, c1, HW, dc)
            x = torch.cat((x0, x1), -1) if c1 else x0
            ref = R.group_norm_fp64(x, 32, g, b, 1e-6, False)
            emu = R.gn_emulated(x0, x1, 32, g, b, 1e-6, False, 16)
            assert rel_l2(emu, ref) < 1e-3 and float((emu - ref).abs().max()) < 6e-3


def test_layer_norm_reference():
    for C in R.LN_C:
        x, g, b = R.ln_inputs(17, C, C)
        ref = R.layer_norm_fp64(x, g, b)
        assert close(ref, F.layer_norm(x.double(), (C,), g.double(), b.double()), 1e-10)
        assert rel_l2(R.rnd(ref), ref) < 1e-3
