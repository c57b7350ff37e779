"""The kernels at the edges of the SD1.5 denoiser, the VAE and the CLIP text encoder op by op against float64: time embedding and rowvec_linear, conv_in,
embed_tokens, quick_gelu / gelu_erf, row_softmax (both kernels), latent_to_nhwc64 / pixel_linear / pixel_affine, the pad-after-only stride-2 conv, GroupNorm with 256
splits and through the LDS-table apply kernel, LayerNorm at every width form.  References, emulators, case lists and inputs: tests/edge_ref.py (verified on the CPU
by tests/test_edge_ref.py).

Acceptance, per output row (per pixel for the convs and the pixel ops), as in tests/test_flux_glue_ops_gpu.py:
    max |out - float64|  <=  2 x max |emulator - float64| of that row  +  1 ulp_fp16 of the row's largest output.
Every case prints its worst err / bound as RATIO.  Ops without rounding-sensitive arithmetic (embed_tokens, integer-valued convs, identity transposes, pad channels)
are compared bit for bit.  Every output lives inside a NaN-filled buffer whose margins, and every element the op must not write, are compared bit for bit.

Worst err / bound seen on an MI355X.  0.25 is an error of half an ulp against the bound's two: the kernel lands on the emulator's rounding.
    sinusoid 0.251 per row, 0.258 per frequency; time embedding linear_1 0.248, linear_2 0.250, the chain from t 0.284; rowvec_linear 0.250;
    conv_in 0.250, out + out_lo against 2^-21 of the pixel's largest output 0.975 (Cout 8; 0.869 at 128, 0.833 at 320);
    quick_gelu and gelu_erf 0.500 per element (the whole-vector rule is idle at 0.000 once +-65504 sets the row's ulp: the per-element bound is the one that bites);
    row_softmax 0.250 register kernel, 0.248 block kernel, 0.243 both ways across the 8192 boundary; row sums 0.877 (520 columns) and 0.044 (block kernel);
    latent_to_nhwc64, pixel_linear, pixel_affine 0.250; GroupNorm 256 splits 0.250 and 0.324 DC-heavy, LDS-table kernel 0.250 and 0.300 DC-heavy;
    LayerNorm 0.250.
The DC-heavy GroupNorm inputs (group mean 20 sigma, single-pass fp32 statistics) stay inside the split-order emulator's bound: no finding there.

Not told apart by any output: WHICH softmax kernel runs at cols = 8192.  Both are valid there and agree to the bound, so a dispatch that sends 8192 to the block
kernel passes this module.
"""
import math

import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import ops
from tests import edge_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CS_E_ARG, CS_E_SHAPE = -1, -2
G = 64                               # NaN halfs in front of and behind every output
NAN_BITS = 0x7E00


def st():
    return L.stream_ptr(DEV)


def guarded(*shape, fill=None):
    """(buffer, view): a NaN-filled fp16 buffer with G halfs of margin around a view of `shape` (holding `fill` when given)"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * G,), R.NAN, dtype=R.F16, device=DEV)
    view = buf[G:G + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def margins_intact(buf):
    bits = buf.view(torch.int16)
    return bool((bits[:G] == NAN_BITS).all()) and bool((bits[-G:] == NAN_BITS).all())


def same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int16), b.cpu().contiguous().view(torch.int16))


def worst_ratio(out, ref, emu, dim=-1):
    return float(((out - ref).abs().amax(dim) / R.rule_bound(ref, emu, dim)).max())


def rows_ok(out, ref, emu, what, dim=-1):
    """the acceptance rule on float64 tensors, rows along `dim`; prints the worst err / bound before it asserts; returns it"""
    worst = worst_ratio(out, ref, emu, dim)
    print(f"RATIO {what}: {worst:.3f}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, (what, worst)
    return worst


# ---- time embedding, rowvec_linear ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bt", R.TIME_BT)
@pytest.mark.parametrize("C0,D", R.TIME_DIMS)
def test_time_embedding_every_stage(C0, D, Bt):
    """the sinusoid (read back from scratch) per row AND per frequency -- cos in [0, C0 / 2), sin behind, so a swap of the halves or of one frequency is a gross
    error --, each linear layer on the very fp16 input the kernel read, and the whole chain from t"""
    t = R.timesteps(Bt)
    w = R.time_weights(C0, D, C0)
    wd = [x.to(DEV) for x in w]
    obuf, out = guarded(Bt, D)
    sbuf, scratch = guarded(Bt * (C0 + D))
    ops.time_embedding(t.to(DEV), *wd, out=out, scratch=scratch)
    torch.cuda.synchronize()
    assert margins_intact(obuf) and margins_intact(sbuf)
    emb, h1, o = scratch[:Bt * C0].view(Bt, C0).cpu(), scratch[Bt * C0:].view(Bt, D).cpu(), out.cpu()
    r_emb, r_h1, r_out = R.time_embedding_fp64(t, C0, *w)
    e_emb, e_h1, e_out = R.time_embedding_emulated(t, C0, *w)
    what = f"C0 {C0} D {D} Bt {Bt}"
    rows_ok(emb.double(), r_emb, e_emb, f"sinusoid per row {what}")
    rows_ok(emb.double(), r_emb, e_emb, f"sinusoid per frequency {what}", dim=0)
    assert bool((emb[0, :C0 // 2] == 1).all()) and bool((emb[0, C0 // 2:] == 0).all())               # t = 0: cos | sin
    if Bt > 1:                                                                                       # t = 1, frequency 0: cos(1) | sin(1)
        assert abs(float(emb[1, 0]) - math.cos(1.0)) < 1e-3 and abs(float(emb[1, C0 // 2]) - math.sin(1.0)) < 1e-3
    ref = R.rowvec_linear_fp64(emb, w[0], w[1], True)
    rows_ok(h1.double(), ref, R.rnd(ref), f"time_embedding linear_1 {what}")
    ref = R.rowvec_linear_fp64(h1, w[2], w[3], True)
    rows_ok(o.double(), ref, R.rnd(ref), f"time_embedding linear_2 {what}")
    rows_ok(o.double(), r_out, e_out, f"time_embedding from t {what}")


@pytest.mark.parametrize("K", R.ROWVEC_K)
def test_rowvec_linear_lane_and_column_tails(K):
    """K / 8 = 1, 40, 64, 65, 160 vectors over 64 lanes; N = 1, 3, 4, 5, 1282 columns at four per workgroup; R = 1, 3; null bias; SiLU on and off"""
    worst = 0.0
    for N in R.ROWVEC_N:
        for Rr in R.ROWVEC_R:
            x, w, bias = R.rowvec_inputs(K, N, Rr, 1000 * K + 10 * N + Rr)
            xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
            for b in (bias, None):
                for silu in (False, True):
                    obuf, out = guarded(Rr, N)
                    ops.rowvec_linear(xd, wd, bd if b is not None else None, silu, out=out)
                    torch.cuda.synchronize()
                    assert margins_intact(obuf)
                    ref = R.rowvec_linear_fp64(x, w, b, silu)
                    got = out.cpu().double()
                    ratio = worst_ratio(got, ref, R.rnd(ref))
                    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (K, N, Rr, b is None, silu, ratio)
                    worst = max(worst, ratio)
    print(f"RATIO rowvec_linear K {K}: {worst:.3f}")
    x, w, _ = R.rowvec_negative_inputs(K, 5)                                                          # pre-activations about -30: SiLU is -3e-12, -0 in fp16
    obuf, out = guarded(1, 5)
    ops.rowvec_linear(x.to(DEV), w.to(DEV), None, True, out=out)
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert bool(torch.isfinite(got).all()) and float(got.max()) <= 0.0 and float(got.min()) >= -R.F16_TINY and margins_intact(obuf)
    obuf, out = guarded(1, 5)
    xd, wd = x.to(DEV), w.to(DEV)
    rc = L.lib().cs_op_rowvec_linear(L.ptr(xd), 1, 12, L.ptr(wd), None, 1, L.ptr(out), 0, st())
    torch.cuda.synchronize()
    assert rc == CS_E_SHAPE and bool(obuf.isnan().all())


# ---- conv_in ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", R.CONV_IN_COUT)
def test_conv_in_latent_sharing_and_lo_plane(Cout):
    """sample b reads latent b % n_lat (the latent buffer holds B samples, the ones past n_lat with other data and another offset); 1-pixel and non-square images;
    integer data bit for bit with a +0 lo plane; random data by the acceptance rule, hi + lo to 2^-21 of the pixel's largest output, and out unchanged without
    the lo plane"""
    worst, worst_sum = 0.0, 0.0
    for n_lat, B in R.CONV_IN_LAT:
        for (H, W) in R.CONV_IN_HW:
            seed = 100 * H + W + B
            lat, w, bias = R.conv_in_inputs(n_lat, B, H, W, Cout, seed, True)
            wp = ops.pack_conv_weight(w).to(DEV)
            obuf, out = guarded(B, H, W, Cout)
            lbuf, lo = guarded(B, H, W, Cout)
            ops.conv_in(lat.to(DEV)[:n_lat], wp, bias.to(DEV), B=B, out=out, out_lo=lo)
            torch.cuda.synchronize()
            ref = R.conv_in_fp64(lat, n_lat, B, w, bias)
            assert same_bits(out, ref.to(R.F16)), (n_lat, B, H, W, "integer conv")
            assert bool((lo.view(torch.int16) == 0).all()), "lo plane of an exact result must be +0"
            assert margins_intact(obuf) and margins_intact(lbuf)

            lat, w, bias = R.conv_in_inputs(n_lat, B, H, W, Cout, seed, False)
            wp, latd, bd = ops.pack_conv_weight(w).to(DEV), lat.to(DEV), bias.to(DEV)
            obuf, out = guarded(B, H, W, Cout)
            lbuf, lo = guarded(B, H, W, Cout)
            ops.conv_in(latd[:n_lat], wp, bd, B=B, out=out, out_lo=lo)
            obuf1, out1 = guarded(B, H, W, Cout)
            ops.conv_in(latd[:n_lat], wp, bd, B=B, out=out1)
            torch.cuda.synchronize()
            assert margins_intact(obuf) and margins_intact(lbuf) and margins_intact(obuf1)
            assert same_bits(out, out1), "out depends on out_lo"
            ref = R.conv_in_fp64(lat, n_lat, B, w, bias)
            e_hi, _ = R.conv_in_emulated(ref)
            hi, lo64 = out.cpu().double(), lo.cpu().double()
            ratio = worst_ratio(hi, ref, e_hi)
            rsum = float(((hi + lo64 - ref).abs().amax(-1) / (2.0 ** -21 * ref.abs().amax(-1))).max())
            assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo64).all()) and ratio <= 1.0 and rsum <= 1.0, (n_lat, B, H, W, ratio, rsum)
            assert bool((lo64.abs() <= 0.5 * R.ulp_at(hi)).all()), "out is not the rounding of out + out_lo"
            worst, worst_sum = max(worst, ratio), max(worst_sum, rsum)
    print(f"RATIO conv_in Cout {Cout}: {worst:.3f}")
    print(f"RATIO conv_in out + out_lo Cout {Cout}: {worst_sum:.3f}")


def test_conv_in_second_pass_of_the_grid_stride_loop():
    """B H W = 5 * 512 * 512 > 4096 workgroups * 256 threads: the only shape whose pixels past 2^20 come from the loop's second pass; integer data, every bit"""
    n_lat, B, H, W, Cout = R.CONV_IN_STRIDE_CASE
    lat, w, bias = R.conv_in_inputs(n_lat, B, H, W, Cout, 3, True)
    obuf, out = guarded(B, H, W, Cout)
    ops.conv_in(lat.to(DEV), ops.pack_conv_weight(w).to(DEV), bias.to(DEV), B=B, out=out)
    torch.cuda.synchronize()
    ref = R.conv_in_fp64(lat, n_lat, B, w, bias, torch.float32)
    assert margins_intact(obuf) and same_bits(out, ref.to(R.F16))


def test_conv_in_refuses_a_weight_table_beyond_the_default_lds():
    """72 Cout bytes of weights in dynamic LDS: 912 channels (65664 bytes) is past the 64 KB a launch gets without opting in; refused on the host, nothing runs"""
    lat = torch.zeros(1, 4, 2, 2, dtype=R.F16, device=DEV)
    w = torch.zeros(912, 9, 4, dtype=R.F16, device=DEV)
    obuf, out = guarded(1, 2, 2, 912)
    rc = L.lib().cs_op_conv_in(L.ptr(lat), 1, 1, 2, 2, L.ptr(w), L.ptr(w), 912, L.ptr(out), None, st())
    assert rc == CS_E_SHAPE and "conv_in: Cout=912 unsupported" in L.lib().cs_last_error().decode()
    torch.cuda.synchronize()
    assert bool(obuf.isnan().all())


# ---- embed_tokens -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.EMBED_C)
@pytest.mark.parametrize("L_", R.EMBED_L)
def test_embed_tokens_clamp_and_position_wrap(L_, C):
    """ids -1, vocab and 2^40 read rows 0 and vocab - 1; row r adds position r % L (B = 3 wraps twice); bit for bit"""
    for B in R.EMBED_B:
        ids, tok, pos = R.embed_inputs(L_, B, C, 10 * L_ + B)
        obuf, out = guarded(B * L_, C)
        ops.embed_tokens(ids.to(DEV), tok.to(DEV), pos.to(DEV), out=out)
        torch.cuda.synchronize()
        assert margins_intact(obuf) and same_bits(out, R.embed_tokens_ref(ids, tok, pos)), (L_, B, C)


# ---- quick_gelu, gelu_erf -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.GELU_N)
@pytest.mark.parametrize("name", ["quick_gelu", "gelu_erf"])
def test_gelu_in_place_values_and_tail(name, n):
    """the whole vector as one row of the acceptance rule, every element against one ulp of its own value + 2^-22 |x| (edge_ref.gelu_element_bound), finite at
    +-65504, and the 8 finite values and the NaN margin behind element n untouched"""
    op, fn = (ops.quick_gelu_, R.quick_gelu_fp64) if name == "quick_gelu" else (ops.gelu_erf_, R.gelu_erf_fp64)
    x = R.gelu_inputs(n)
    tail = torch.linspace(-3, 3, 8).to(R.F16)
    buf, view = guarded(n + 8, fill=torch.cat((x, tail)).to(DEV))
    op(view, n)
    torch.cuda.synchronize()
    assert margins_intact(buf) and same_bits(view[n:], tail), "elements past n changed"
    got, ref = view[:n].cpu().double(), fn(x)
    assert bool(torch.isfinite(got).all())
    rows_ok(got, ref, R.rnd(ref), f"{name} n {n} whole vector")
    el = float(((got - ref).abs() / R.gelu_element_bound(x, ref)).max())
    print(f"RATIO {name} n {n} per element: {el:.3f}")
    assert el <= 1.0
    big = x.double().abs() == R.F16_MAX
    assert bool((got[big & (x.double() > 0)] == R.F16_MAX).all()) and bool((got[big & (x.double() < 0)] == 0).all())


def test_gelu_refusals():
    buf, view = guarded(16)
    for f, code in ((L.lib().cs_op_quick_gelu, CS_E_SHAPE), (L.lib().cs_op_gelu_erf, CS_E_ARG)):      # a count that is no multiple of 8: each launcher's own code
        assert f(L.ptr(view), 12, st()) == code
        assert f(L.ptr(view), 0, st()) == 0
    torch.cuda.synchronize()
    assert bool(buf.isnan().all())


# ---- row_softmax --------------------------------------------------------------------------------------------------------------------------------------------------
def _softmax_case(rows, cols, scale, kind):
    x = R.softmax_rows(rows, cols, scale, kind, 7 * cols + rows)
    buf, view = guarded(rows, cols, fill=x.to(DEV))
    ops.row_softmax_(view, scale)
    torch.cuda.synchronize()
    assert margins_intact(buf)
    got, ref = view.cpu().double(), R.row_softmax_fp64(x, scale)
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0, (rows, cols, scale, kind)
    ratio = worst_ratio(got, ref, R.rnd(ref))
    rsum = float(((got.sum(-1) - 1.0).abs() / R.softmax_sum_bound(ref)).max())
    assert ratio <= 1.0 and rsum <= 1.0, (rows, cols, scale, kind, ratio, rsum)
    if kind == "constant":
        assert bool((got == float(torch.tensor(1.0 / cols).to(R.F16))).all()), (rows, cols, scale)
    return ratio, rsum


def _softmax_all(rows_list, cols, scale, what):
    worst, worst_sum = 0.0, 0.0
    for rows in rows_list:
        for kind in R.SOFTMAX_KINDS:
            a, b = _softmax_case(rows, cols, scale, kind)
            worst, worst_sum = max(worst, a), max(worst_sum, b)
    print(f"RATIO row_softmax {what} cols {cols} scale {scale:.4f}: {worst:.3f}")
    print(f"RATIO row_softmax {what} sum cols {cols} scale {scale:.4f}: {worst_sum:.3f}")


@pytest.mark.parametrize("scale", R.SOFTMAX_SCALES)
@pytest.mark.parametrize("cols", R.SOFTMAX_REG_COLS)
def test_row_softmax_register_kernel(cols, scale):
    """cols / 8 = 1, 8, 63, 64, 65, 512, 1024 vectors over 64 lanes x 16 registers (8192 fills them); rows = 1, 3, 4, 5 at four per workgroup"""
    _softmax_all(R.SOFTMAX_REG_ROWS, cols, scale, "register")


@pytest.mark.parametrize("scale", R.SOFTMAX_SCALES)
@pytest.mark.parametrize("cols", R.SOFTMAX_BLOCK_COLS)
def test_row_softmax_block_kernel(cols, scale):
    """the first width past the register kernel (8200: 1025 vectors over 256 threads), 16384, and the widest (65536)"""
    _softmax_all(R.SOFTMAX_BLOCK_ROWS, cols, scale, "block")


@pytest.mark.parametrize("scale", R.SOFTMAX_SCALES)
def test_row_softmax_kernels_agree_across_the_8192_boundary(scale):
    """the same 8192 logits through the register kernel and, with eight more at -65504 (weight exactly 0), through the block kernel"""
    rows = 3
    x = R.softmax_rows(rows, 8192, scale, "gaussian", 11)
    x2 = torch.cat((x, torch.full((rows, 8), -R.F16_MAX, dtype=R.F16)), -1)
    b1, v1 = guarded(rows, 8192, fill=x.to(DEV))
    b2, v2 = guarded(rows, 8200, fill=x2.to(DEV))
    ops.row_softmax_(v1, scale)
    ops.row_softmax_(v2, scale)
    torch.cuda.synchronize()
    assert margins_intact(b1) and margins_intact(b2)
    ref = R.row_softmax_fp64(x, scale)
    g1, g2 = v1.cpu().double(), v2.cpu().double()
    assert bool((g2[:, 8192:] == 0).all())
    rows_ok(g1, ref, R.rnd(ref), f"row_softmax 8192 register scale {scale:.4f}")
    rows_ok(g2[:, :8192], ref, R.rnd(ref), f"row_softmax 8200 block scale {scale:.4f}")
    assert bool(((g1 - g2[:, :8192]).abs().amax(-1) <= R.rule_bound(ref, R.rnd(ref))).all())


def test_row_softmax_refusals():
    buf, view = guarded(2, 16)
    for cols in (12, 65544):
        rc = L.lib().cs_op_row_softmax(L.ptr(view), 1, cols, 1.0, st())
        assert rc == CS_E_SHAPE and f"cols={cols} unsupported" in L.lib().cs_last_error().decode()
    assert L.lib().cs_op_row_softmax(L.ptr(view), 0, 16, 1.0, st()) == 0
    torch.cuda.synchronize()
    assert bool(buf.isnan().all())


# ---- latent_to_nhwc64, pixel_linear, pixel_affine -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.LATENT_C)
def test_latent_to_nhwc64_forms_and_zero_padding(C):
    """identity form (scale 1 / 0.18215, with and without a shift), the C -> C post-quant form, HW = 1, 255, 256, 257 around one workgroup; channels C .. 63 of
    every pixel are +0 in a NaN-filled output; scale 1 and shift 0 is the transpose, bit for bit"""
    worst = 0.0
    for HW in R.PIXEL_HW:
        for B in R.LATENT_B:
            x, w, b = R.pixel_inputs(B, C, HW, C, 100 * C + HW + B)
            xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
            for form, ww, scale, shift in (("identity", None, R.SD_SCALE, 0.0), ("identity + shift", None, R.SD_SCALE, 0.25), ("w", w, R.SD_SCALE, 0.25),
                                           ("transpose", None, 1.0, 0.0)):
                obuf, out = guarded(B, HW, 64)
                ops.latent_to_nhwc64(xd, wd if ww is not None else None, bd if ww is not None else None, scale, shift, out=out)
                torch.cuda.synchronize()
                assert margins_intact(obuf)
                assert bool((out[..., C:].contiguous().view(torch.int16) == 0).all()), (C, HW, B, form, "pad channels must be +0")
                if form == "transpose":
                    assert same_bits(out[..., :C], x.transpose(1, 2)), (C, HW, B)
                    continue
                ref = R.latent_fp64(x, ww, b if ww is not None else None, scale, shift)
                got = out[..., :C].cpu().double()
                ratio = worst_ratio(got, ref, R.rnd(ref))
                assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (C, HW, B, form, ratio)
                worst = max(worst, ratio)
    print(f"RATIO latent_to_nhwc64 C {C}: {worst:.3f}")


def test_latent_to_nhwc64_refusals():
    x = torch.zeros(1, 72, 4, dtype=R.F16, device=DEV)
    obuf, out = guarded(1, 4, 64)
    for C in (0, 65):
        assert L.lib().cs_op_latent_to_nhwc64(L.ptr(x), None, None, L.ptr(out), 1, C, 4, 1.0, 0.0, st()) == CS_E_SHAPE
    assert L.lib().cs_op_latent_to_nhwc64(L.ptr(x), L.ptr(x), None, L.ptr(out), 1, 4, 4, 1.0, 0.0, st()) == CS_E_ARG
    torch.cuda.synchronize()
    assert bool(obuf.isnan().all())


@pytest.mark.parametrize("C", R.PIXEL_LINEAR_C)
def test_pixel_linear_against_w_times_scaled_input(C):
    worst = 0.0
    for HW in R.PIXEL_HW:
        for B in (1, 2):
            x, w, b = R.pixel_inputs(B, C, HW, C, 10 * C + HW + B)
            obuf, out = guarded(B, C, HW)
            ops.pixel_linear(x.to(DEV), w.to(DEV), b.to(DEV), R.SD_SCALE, 0.25, out=out)
            torch.cuda.synchronize()
            assert margins_intact(obuf)
            ref = R.pixel_linear_fp64(x, w, b, R.SD_SCALE, 0.25)
            got = out.cpu().double()
            ratio = worst_ratio(got, ref, R.rnd(ref), dim=1)
            assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (C, HW, B, ratio)
            worst = max(worst, ratio)
    print(f"RATIO pixel_linear C {C}: {worst:.3f}")


@pytest.mark.parametrize("form,Cin,Cout", R.AFFINE_FORMS)
def test_pixel_affine_subtracts_the_shift_before_it_scales(form, Cin, Cout):
    """(acc - 1.5) * 0.5: the other order, acc * 0.5 - 1.5, is 0.75 away (hundreds of times the bound: tests/test_edge_ref.py)"""
    worst = 0.0
    for HW in R.PIXEL_HW:
        for B in (1, 2):
            x, w, b = R.pixel_inputs(B, Cin, HW, Cout, 10 * Cin + HW + B)
            ww, bb = (w, b) if form == "w" else (None, None)
            obuf, out = guarded(B, Cout, HW)
            ops.pixel_affine(x.to(DEV), Cout, ww.to(DEV) if ww is not None else None, bb.to(DEV) if bb is not None else None, R.AFFINE_SCALE, R.AFFINE_SHIFT, out=out)
            torch.cuda.synchronize()
            assert margins_intact(obuf)
            ref = R.pixel_affine_fp64(x, Cout, ww, bb, R.AFFINE_SCALE, R.AFFINE_SHIFT)
            got = out.cpu().double()
            ratio = worst_ratio(got, ref, R.rnd(ref), dim=1)
            assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (form, Cin, Cout, HW, B, ratio)
            worst = max(worst, ratio)
    print(f"RATIO pixel_affine {form} {Cin} -> {Cout}: {worst:.3f}")


def test_pixel_affine_identity_form_refuses_more_outputs_than_inputs():
    x = torch.zeros(1, 4, 4, dtype=R.F16, device=DEV)
    obuf, out = guarded(1, 8, 4)
    rc = L.lib().cs_op_pixel_affine(L.ptr(x), 4, None, None, 8, L.ptr(out), 1, 4, 1.0, 0.0, st())
    assert rc == CS_E_SHAPE and "identity form needs Cout <= Cin" in L.lib().cs_last_error().decode()
    torch.cuda.synchronize()
    assert bool(obuf.isnan().all())


# ---- conv_down ----------------------------------------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("case", R.CONV_DOWN_CASES)
def test_conv_down_pads_after_the_image_only(case):
    """F.conv2d(F.pad(x, (0, 1, 0, 1)), stride=2): integer data bit for bit; random data at test_conv2d's tolerances, the last output row and column (the ones that
    see the zero pad) on their own, and far from the symmetric-pad conv of the same inputs"""
    B, H, W, Cin, N = case
    x, w, bias = R.conv_down_inputs(*case, 5, True)
    obuf, out = guarded(B, H // 2, W // 2, N)
    ops.conv_down(x.to(DEV), ops.pack_conv_weight(w).to(DEV), bias.to(DEV), out=out)
    torch.cuda.synchronize()
    assert margins_intact(obuf) and same_bits(out, R.conv_down_fp64(x, w, bias).to(R.F16))

    x, w, bias = R.conv_down_inputs(*case, 5, False)
    xd, wp, bd = x.to(DEV), ops.pack_conv_weight(w).to(DEV), bias.to(DEV)
    obuf, out = guarded(B, H // 2, W // 2, N)
    ops.conv_down(xd, wp, bd, out=out)
    sym = ops.conv2d(xd, wp, bd, stride=2)
    torch.cuda.synchronize()
    assert margins_intact(obuf)
    ref, got, sym = R.conv_down_fp64(x, w, bias), out.cpu().double(), sym.cpu().double()
    top = float(ref.abs().max())
    assert _rel_l2(got, ref) < 1e-3 and float((got - ref).abs().max()) < 4e-3 * top
    border = torch.zeros(H // 2, W // 2, dtype=torch.bool)
    border[-1, :] = True
    border[:, -1] = True
    assert _rel_l2(got[:, border], ref[:, border]) < 1e-3
    assert float((got[:, border] - ref[:, border]).abs().max()) < 4e-3 * float(ref[:, border].abs().max())
    assert _rel_l2(sym, got) > 10 * 1e-3 and float((sym - got).abs().max()) > 10 * 4e-3 * top


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------------------------------
def _gn_check(got, x, x0, x1, g, b, eps, silu, smax, what, dc):
    ref = R.group_norm_fp64(x, 32, g, b, eps, silu)
    assert _rel_l2(got, ref) < 1e-3 and float((got - ref).abs().max()) < 6e-3, what                     # test_group_norm's tolerances
    emu = R.gn_emulated(x0, x1, 32, g, b, eps, silu, smax)
    ratio = worst_ratio(got, ref, emu)
    assert bool(torch.isfinite(got).all()) and ratio <= 1.0, (what, "DC-heavy" if dc else "", ratio)
    return ratio


@pytest.mark.parametrize("HW", R.GN_SPLIT_HW)
@pytest.mark.parametrize("C", R.GN_SPLIT_C)
def test_group_norm_with_256_splits(C, HW):
    """the VAE's call: splits = 256 (S = 1, 64, 64, 64, 256 row ranges at HW = 9, 64, 576, 1600, 4096), 4 / 8 / 16 channels per group, eps 1e-6; B = 1, 3; SiLU
    on and off; plain inputs and DC-heavy ones (group mean about 20 sigma: the statistics are single-pass fp32 sums) against the split-order emulator"""
    worst = {False: 0.0, True: 0.0}
    for B in R.GN_SPLIT_B:
        for dc in (False, True):
            x0, _, g, b = R.gn_inputs(B, HW, C, 0, HW + C + B, dc)
            for silu in (False, True):
                obuf, out = guarded(B, HW, C)
                ops.group_norm_splits(x0.to(DEV), g.to(DEV), b.to(DEV), 256, 32, 1e-6, silu, out=out)
                torch.cuda.synchronize()
                assert margins_intact(obuf)
                worst[dc] = max(worst[dc], _gn_check(out.cpu().double(), x0, x0, None, g, b, 1e-6, silu, 256, (C, HW, B, silu), dc))
    print(f"RATIO group_norm splits 256 C {C} HW {HW}: {worst[False]:.3f}")
    print(f"RATIO group_norm splits 256 DC-heavy C {C} HW {HW}: {worst[True]:.3f}")


@pytest.mark.parametrize("HW", [64, 1600, 4096])
def test_group_norm_splits_workspace_holds_one_partial_sum_per_split(HW):
    """that the requested split count is the one that ran: the workspace (ops.h, GroupNormArgs) holds partial[B][S][C / 2][2] = (sum, sum of squares) of every channel
    pair over each of the S = 64 / 64 / 256 row ranges, then nothing up to float B * 256 * C, where the (scale, shift) table [B][C][2] sits, and nothing behind it"""
    B, C, smax = 2, 128, 256
    S = R.gn_splits(HW, smax)
    x0, _, g, b = R.gn_inputs(B, HW, C, 0, HW, False)
    nbytes = int(L.lib().cs_op_group_norm_workspace_splits(B, C, smax))
    assert nbytes >= B * (smax + 1) * C * 2 * 4 and nbytes % 256 == 0
    ws = torch.full((nbytes // 4 + G,), R.NAN, dtype=torch.float32, device=DEV)
    ops.group_norm_splits(x0.to(DEV), g.to(DEV), b.to(DEV), smax, 32, 1e-6, False, ws=ws)
    torch.cuda.synchronize()
    w = ws.cpu()
    part = w[:B * S * C].view(B, S, C // 2, 2).double()
    assert bool(torch.isfinite(part).all()), "fewer partial sums than splits"
    xs = x0.double().reshape(B, S, HW // S, C // 2, 2)
    assert bool(((part[..., 0] - xs.sum((2, 4))).abs() <= 2e-5 * xs.abs().sum((2, 4)) + 1e-6).all())
    assert bool(((part[..., 1] - (xs * xs).sum((2, 4))).abs() <= 2e-5 * (xs * xs).sum((2, 4)) + 1e-6).all())
    off = B * smax * C
    assert bool(w[B * S * C:off].isnan().all()) and bool(w[off + 2 * B * C:].isnan().all())
    table = w[off:off + 2 * B * C].view(B, C, 2).double()
    xg = x0.double().reshape(B, HW, 32, C // 32)
    mean = xg.mean((1, 3)).repeat_interleave(C // 32, -1)
    rstd = torch.rsqrt(xg.var((1, 3), unbiased=False) + 1e-6).repeat_interleave(C // 32, -1)
    sc = g.double()[None, :] * rstd
    assert bool(((table[..., 0] - sc).abs() <= 1e-4 * sc.abs()).all())
    assert bool(((table[..., 1] - (b.double()[None, :] - mean * sc)).abs() <= 1e-4 * (1 + (mean * sc).abs())).all())


@pytest.mark.parametrize("c0,c1", R.GN_TABLE_C)
def test_group_norm_lds_table_apply_kernel(c0, c1):
    """more than 2560 channels: the column kernel's 320 threads cannot hold a row, gn_apply_kernel with the (scale, shift) table in LDS runs; one source of 2688
    channels (84 per group) and two sources 2048 + 640; HW = 4, 16, 100"""
    worst = {False: 0.0, True: 0.0}
    for HW in R.GN_TABLE_HW:
        for dc in (False, True):
            x0, x1, g, b = R.gn_inputs(2, HW, c0, c1, HW, dc)
            x = torch.cat((x0, x1), -1) if c1 else x0
            for silu in (False, True):
                out = ops.group_norm(x0.to(DEV), g.to(DEV), b.to(DEV), 32, 1e-6, silu, x1=x1.to(DEV) if c1 else None)
                torch.cuda.synchronize()
                worst[dc] = max(worst[dc], _gn_check(out.cpu().double(), x, x0, x1, g, b, 1e-6, silu, 16, (c0, c1, HW, silu), dc))
    print(f"RATIO group_norm LDS table {c0} + {c1}: {worst[False]:.3f}")
    print(f"RATIO group_norm LDS table DC-heavy {c0} + {c1}: {worst[True]:.3f}")


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.LN_C)
def test_layer_norm_every_width_form_and_row_tail(C):
    """C / 8 = 1, 65, 161, 193, 256 vectors: ln_kernel<1,4>, <2,2>, <3,1>, <4,1> (and <4,1> full), each with a part-filled last round of lanes but the last; M = 1 .. 17
    around the 16 / 8 / 4 rows a workgroup covers; rows past M stay NaN"""
    worst = 0.0
    for M in R.LN_M:
        x, g, b = R.ln_inputs(M, C, 100 * C + M)
        obuf, out = guarded(M, C)
        xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
        L.check(L.lib().cs_op_layer_norm(L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(out), M, C, 1e-5, st()))
        torch.cuda.synchronize()
        assert margins_intact(obuf), (C, M)
        ref, got = R.layer_norm_fp64(x, g, b), out.cpu().double()
        assert bool(torch.isfinite(got).all()) and _rel_l2(got, ref) < 1e-3, (C, M)                   # test_layer_norm's tolerance, and per row
        assert float(((got - ref).norm(dim=-1) / ref.norm(dim=-1)).max()) < 1e-3, (C, M)
        worst = max(worst, worst_ratio(got, ref, R.rnd(ref)))
    print(f"RATIO layer_norm C {C}: {worst:.3f}")
    assert worst <= 1.0


def test_layer_norm_refuses_more_than_2048_channels():
    x = torch.zeros(2, 2056, dtype=R.F16, device=DEV)
    obuf, out = guarded(2, 2056)
    rc = L.lib().cs_op_layer_norm(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(out), 2, 2056, 1e-5, st())
    assert rc == CS_E_SHAPE and "C=2056 unsupported" in L.lib().cs_last_error().decode()
    torch.cuda.synchronize()
    assert bool(obuf.isnan().all())
