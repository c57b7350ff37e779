"""HIP UNet forward (cs_unet_forward through the C ABI) vs the torch-fp32 oracle restatement.

The oracle is "parity unpinned" w.r.t. diffusers (see oracle/unet_oracle.py); what is pinned here is
that the HIP kernels compute the same function as the fp32 restatement on identical seeded weights.
Tolerance: per-forward relative L2 of the eps output in the default residual-stream mode (f16x2): 0.87e-3 ... 0.89e-3 (1.06e-3 on 8 x 8 latents), every
bound = measured + 10 % (round 5; the f16 stream measures 1.5e-3 ... 1.6e-3).  What that error is made of and how it compares with a torch-fp16 evaluation of the
same graph: tests/test_parity_e2e_gpu.py; the 1e-3 gate itself is on the 8-step latents there.
"""
import pytest
import torch

from consolver_amd.unet import HipUNet2DConditionModel, SD15_CONFIG
from consolver_amd.synth import synthetic_unet_state_dict, synthetic_prompt_embeds
from oracle.unet_oracle import UNetOracle
from tests._models import get_unet, get_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def build(cfg_over):
    # one build per (config, seed) and pytest process (tests/_models.py); default residual stream (f16x2)
    u, _ = get_unet(cfg_over, seed=7)
    return u, get_oracle(cfg_over, seed=7)


def test_reduced_unet_matches_oracle():
    # full SD1.5 widths and head dims, one layer per block, 16x16 latents: every kernel shape class
    # (BN 128/160, stride 2, upsample, concat, dh 40/80/160, Nk=77) in a forward the CPU oracle runs in seconds
    u, orc = build(dict(layers_per_block=1, sample_size=16))
    g = torch.Generator().manual_seed(3)
    lat = torch.randn(2, 4, 16, 16, generator=g)
    ctx = synthetic_prompt_embeds(4, seed=11)
    t = 749
    got = u(lat.half().to(DEV), t, encoder_hidden_states=ctx.half().to(DEV), dup=2)[0]
    want = orc(torch.cat([lat.half().float()] * 2), t, ctx.half().float())
    assert got.shape == (4, 4, 16, 16) and got.dtype == torch.float16
    err = rel_l2(got, want)
    print('reduced unet rel l2', err)
    assert err < 0.99e-3, err            # default stream (f16x2): measured 0.892e-3, + 10 %  (f16 stream: 1.48e-3)
    # cached cross-attention K/V (second step, same ctx) and per-sample timesteps give the same function
    got2 = u(lat.half().to(DEV), torch.full((4,), float(t), device=DEV), encoder_hidden_states=ctx.half().to(DEV), dup=2, reuse_kv=True)[0]
    assert rel_l2(got2, want) < 0.99e-3
    # un-duplicated batch path == dual batch path on the conditional half
    got3 = u(lat.half().to(DEV), t, encoder_hidden_states=ctx[2:].half().to(DEV), dup=1, reuse_kv=False)[0]
    assert torch.equal(got3, got[2:])
    assert abs(u.flops(1) / 1e9 - orc_flops_estimate(u.config)) / orc_flops_estimate(u.config) < 0.02


def orc_flops_estimate(cfg):
    """independent MAC count of the restated graph (conv/linear/attention only), GFLOP per sample"""
    c = cfg["block_out_channels"]; S = cfg["sample_size"]; L = cfg["ctx_len"]; cd = cfg["cross_attention_dim"]
    mac = 0
    def res(cin, cout, hw):
        return hw * 9 * cin * cout + hw * 9 * cout * cout + (hw * cin * cout if cin != cout else 0) + 4 * c[0] * cout
    def xf(C, hw):
        return (2 * hw * C * C + 4 * hw * C * C + 2 * hw * hw * C + hw * C * C + 2 * L * cd * C + 2 * hw * L * C + hw * C * C
                + hw * C * 8 * C + hw * 4 * C * C)
    hw = S * S
    mac += hw * 9 * 4 * c[0] + c[0] * 4 * c[0] + 16 * c[0] * c[0]
    ch = c[0]; skips = [ch]
    for i in range(4):
        for j in range(cfg["layers_per_block"]):
            mac += res(ch, c[i], hw); ch = c[i]
            if cfg["down_has_attn"][i]:
                mac += xf(ch, hw)
            skips.append(ch)
        if i < 3:
            hw //= 4; mac += hw * 9 * ch * ch; skips.append(ch)
    mac += 2 * res(ch, ch, hw) + xf(ch, hw)
    for i in range(4):
        co = c[3 - i]
        for j in range(cfg["layers_per_block"] + 1):
            mac += res(ch + skips.pop(), co, hw); ch = co
            if cfg["up_has_attn"][i]:
                mac += xf(ch, hw)
        if i < 3:
            hw *= 4; mac += hw * 9 * ch * ch
    mac += hw * 9 * ch * 4
    return 2 * mac / 1e9


def test_sd15_flops_match_survey():
    u = HipUNet2DConditionModel(device=DEV)
    assert abs(orc_flops_estimate(u.config) - 803.27) / 803.27 < 0.01        # SURVEY 2c / BASELINE.md: 803.27 GFLOP


@pytest.mark.timeout(900)
def test_full_sd15_unet_matches_oracle_cfg_batch():
    u, orc = build({})
    assert abs(u.flops(1) / 1e9 - 803.27) < 0.02 and abs(u.flops(32) / 32e9 - 803.27) < 0.02       # the reference graph's count, per sample at any batch, whatever the knobs
    from consolver_amd import ops as _ops
    _ops.set_tuning("conv_in_mfma", 0)
    assert abs(u.flops(32) / 32e9 - 803.27) < 0.02
    _ops.set_tuning("conv_in_mfma", 1)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, 4, 64, 64, generator=g)
    ctx = synthetic_prompt_embeds(2, seed=13)
    got = u(lat.half().to(DEV), 499, encoder_hidden_states=ctx.half().to(DEV), dup=2)[0]
    torch.set_num_threads(16)
    want = orc(torch.cat([lat.half().float()] * 2), 499, ctx.half().float())
    err = rel_l2(got, want)
    print('sd15 unet rel l2', err)
    assert err < 0.96e-3, err            # default stream (f16x2): measured 0.872e-3, + 10 % (f16 stream 1.59e-3; a plain torch-fp16 evaluation of the same graph: 2.9e-3, tests/test_parity_e2e_gpu.py)
    assert torch.isfinite(got).all()
    # determinism
    again = u(lat.half().to(DEV), 499, encoder_hidden_states=ctx.half().to(DEV), dup=2)[0]
    assert torch.equal(got, again)


@pytest.mark.timeout(900)
def test_cfg_shared_prefix_matches_full_dual_batch():
    """CFG dual batch (dup = 2, one timestep): the layers in front of the first cross attention are evaluated once for both
    halves (unet.cpp `Run::xformer` with `n_share`).  Same function of the same inputs -> the result must equal the full dual
    batch: bit for bit at the benchmark's shape (the per-sample kernels and their tile / split choices are the same at batch 16
    and 32), and to fp16 rounding on a reduced model where the smaller prefix batch may pick another split-K factor."""
    from consolver_amd import ops
    try:
        for cfg_over, n_lat, exact in ((dict(layers_per_block=1, sample_size=16), 3, False), ({}, 16, True)):
            u, _ = build(cfg_over)
            S = u.config["sample_size"]
            g = torch.Generator().manual_seed(9)
            lat = torch.randn(n_lat, 4, S, S, generator=g).half().to(DEV)
            ctx = synthetic_prompt_embeds(2 * n_lat, seed=21).half().to(DEV)
            ops.set_tuning("cfg_share", 0)
            full = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
            ops.set_tuning("cfg_share", 1)
            shared = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
            again = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=True)[0]
            assert torch.equal(shared, again)
            err = rel_l2(shared, full)
            print("cfg shared prefix vs full dual batch: rel l2", err, "bit-identical" if torch.equal(shared, full) else "")
            assert torch.isfinite(shared).all()
            if exact:
                assert torch.equal(shared, full)
            else:
                assert err < 1e-3, err
            assert not torch.equal(shared[:n_lat], shared[n_lat:])          # the halves do diverge after the shared prefix
            # per-sample timesteps (the halves could differ): the shared path is not taken, results equal the full batch
            tt = torch.full((2 * n_lat,), 499.0, device=DEV)
            assert torch.equal(u(lat, tt, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0], full)
            # the executed count differs from the reference graph's by what the execution pads, doubles or shares: conv_in on the MFMA conv runs 64 input channels for 4 (+),
            # the resnet shortcut's hi + lo k passes in the f16x2 mode (+ 2.2 %), one time MLP per forward instead of one per sample (-), the CFG-shared prefix (- 2.5 %)
            assert abs(u.flops_executed(2 * n_lat, 1) / u.flops(2 * n_lat) - 1.0) < 3e-2
            assert u.flops_executed(n_lat, 2) < u.flops_executed(2 * n_lat, 1)
    finally:
        ops.set_tuning("cfg_share", 1)


def test_fused_cross_attention_block_matches_the_four_kernel_path():
    """cs_unet_forward with the fused cross-attention sub-block (xattn.hip, default at C = 320) against the same forward with
    LayerNorm / to_q / attention / to_out as four kernels: same roundings up to the softmax formulation."""
    from consolver_amd import ops
    u, orc = build(dict(layers_per_block=1, sample_size=16))
    g = torch.Generator().manual_seed(4)
    lat = torch.randn(2, 4, 16, 16, generator=g).half().to(DEV)
    ctx = synthetic_prompt_embeds(4, seed=17).half().to(DEV)
    try:
        ops.set_tuning("xattn_fused", 0)
        four = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
        ops.set_tuning("xattn_fused", 1)
        fused = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
    finally:
        ops.set_tuning("xattn_fused", 1)
    want = orc(torch.cat([lat.cpu().float()] * 2), 499, ctx.cpu().float())
    e_ff, e_fused, e_four = rel_l2(fused, four), rel_l2(fused, want), rel_l2(four, want)
    print(f"fused vs four kernels {e_ff:.3e}; vs fp32 oracle: fused {e_fused:.3e}, four kernels {e_four:.3e}")
    assert e_ff < 1.25 * (e_fused ** 2 + e_four ** 2) ** 0.5          # two independent roundings of the same fp32 function
    assert e_fused < 1.15 * e_four + 1e-4          # the fusion costs no accuracy
    assert e_fused < 1.05e-3 and e_four < 1.05e-3          # measured 0.955e-3 / 0.951e-3, + 10 %


def test_group_norm_statistics_from_the_producers_match_the_statistics_pass():
    """cs_unet_forward with the GroupNorm statistics taken from the producing conv / 1x1 epilogues (gn_fuse = 1, default) against the same
    forward with a statistics pass per GroupNorm: the same sums in a different order."""
    from consolver_amd import ops
    for cfg_over, n_lat in ((dict(layers_per_block=1, sample_size=16), 2), ({}, 1)):
        u, orc = build(cfg_over)
        S = u.config["sample_size"]
        g = torch.Generator().manual_seed(5)
        lat = torch.randn(n_lat, 4, S, S, generator=g).half().to(DEV)
        ctx = synthetic_prompt_embeds(2 * n_lat, seed=19).half().to(DEV)
        try:
            ops.set_tuning("gn_fuse", 0)
            sep = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
            ops.set_tuning("gn_fuse", 1)
            fused = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
        finally:
            ops.set_tuning("gn_fuse", 1)
        want = orc(torch.cat([lat.cpu().float()] * 2), 499, ctx.cpu().float())
        e_fs, e_f, e_s = rel_l2(fused, sep), rel_l2(fused, want), rel_l2(sep, want)
        print(f"sample_size {S}: fused vs pass {e_fs:.3e}; vs fp32 oracle: fused {e_f:.3e}, pass {e_s:.3e}")
        assert torch.isfinite(fused).all()
        assert e_fs < 1.25 * (e_f ** 2 + e_s ** 2) ** 0.5              # two rounding realisations of the same fp32 function (any perturbation decorrelates the fp16 roundings downstream)
        assert e_f < 1.1 * e_s + 1e-4


@pytest.mark.parametrize("sample_size,n_lat", [(24, 3), (8, 5), (40, 1)])
def test_unet_at_sizes_where_only_some_levels_take_the_fused_paths(sample_size, n_lat):
    """latent sizes that are not powers of two / tiny: 24 x 24 (576 = 9 x 64 pixels: statistics epilogue through the generic conv kernel, 12 x 12
    and below fall back to the statistics pass), 8 x 8 (every level below 64 pixels but the first), 40 x 40 -- against the fp32 oracle."""
    u, orc = build(dict(layers_per_block=1, sample_size=sample_size))
    g = torch.Generator().manual_seed(13)
    lat = torch.randn(n_lat, 4, sample_size, sample_size, generator=g)
    ctx = synthetic_prompt_embeds(2 * n_lat, seed=23)
    got = u(lat.half().to(DEV), 301, encoder_hidden_states=ctx.half().to(DEV), dup=2, reuse_kv=False)[0]
    want = orc(torch.cat([lat.half().float()] * 2), 301, ctx.half().float())
    err = rel_l2(got, want)
    print(f"sample_size {sample_size}: rel l2 vs fp32 oracle {err:.3e}")
    bound = {24: 0.87e-3, 8: 1.17e-3, 40: 0.88e-3}[sample_size]          # measured 0.783e-3 / 1.060e-3 / 0.797e-3 (default stream), + 10 %
    assert torch.isfinite(got).all() and err < bound, err


def test_output_head_on_two_planes_with_the_fp32_output():
    """round 6 (knob head_x2, default 1): with the split stream the final GroupNorm + SiLU writes hi + lo planes and conv_out multiplies both -- one fp16 plane of that tensor
    was the last one-plane station of the stream's value in front of eps.  The fp32 output (the native engine's) is the sum of the two products, the model-dtype output
    (the plain protocol's) its one rounding.  16 x 16 and 32 x 32 latents (the MFMA conv_out's patch shapes); the one-plane stream is untouched."""
    for size in (16, 32):
        cfg = dict(layers_per_block=1, sample_size=size)
        u, _ = get_unet(cfg, seed=7)
        orc = get_oracle(cfg, seed=7)
        g = torch.Generator().manual_seed(9)
        lat = torch.randn(1, 4, size, size, generator=g).half()
        ctx = synthetic_prompt_embeds(2, seed=17).half()
        t = 999
        want = orc(torch.cat([lat.float()] * 2), t, ctx.float())
        run = lambda **kw: u(lat.to(DEV), t, encoder_hidden_states=ctx.to(DEV), dup=2, reuse_kv=False, **kw)[0].clone()
        try:
            u.set_tuning("head_x2", 0); one32 = run(out_dtype=torch.float32); one16 = run()
            u.set_tuning("head_x2", 1); two32 = run(out_dtype=torch.float32); two16 = run()
            assert torch.equal(run(out_dtype=torch.float32), two32)
            assert torch.equal(two32.half(), two16) and torch.equal(one32.half(), one16)      # either way the fp16 output is the rounding of the fp32 one
            e1, e2 = rel_l2(one32, want), rel_l2(two32, want)
            e1h, e2h = rel_l2(one16, want), rel_l2(two16, want)
            print(f"\n{size} x {size}: eps vs the fp32 oracle: fp32 output: one-plane head {e1:.4e}, hi + lo head {e2:.4e}; fp16 output: {e1h:.4e}, {e2h:.4e}")
            assert not torch.equal(one32, two32) and e2 < e1 and e2h < e1h, (e1, e2, e1h, e2h)
            assert rel_l2(two32, one32) < 5e-4                                 # (a 2^-12-class correction)
            u.set_residual_precision("f16")
            a = run(out_dtype=torch.float32); u.set_tuning("head_x2", 0); b = run(out_dtype=torch.float32)
            assert torch.equal(a, b)                                           # one-plane stream: no lo plane anywhere
            u.set_residual_precision("f16x2")
        finally:
            u.clear_tuning()


def test_upsamplers_in_the_subpixel_form_on_the_one_plane_stream():
    """round 6 (knob up_fold, default 1): in forwards whose residual stream is one fp16 plane the upsamplers run the sub-pixel form on pre-summed taps
    (cs_op_conv_up_sub: 4 / 9 of the multiplies; the summed weights are rounded to fp16 once more).  32 x 32 latents: the 8 x 8 -> 16 x 16 upsampler takes the
    four-images-per-tile form, 16 x 16 -> 32 x 32 the one-patch form, 4 x 4 -> 8 x 8 stays on the fused-upsample kernel.  Against the fp32 oracle the two forms are
    the same forward (the one-plane stream's own error is 1.5e-3); the split stream does not use the form unless asked (up_fold = 2)."""
    cfg = dict(layers_per_block=1, sample_size=32)
    u, _ = get_unet(cfg, seed=7, residual="f16")
    orc = get_oracle(cfg, seed=7)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, 4, 32, 32, generator=g).half()
    ctx = synthetic_prompt_embeds(2, seed=13).half()
    t = 401
    want = orc(torch.cat([lat.float()] * 2), t, ctx.float())
    run = lambda: u(lat.to(DEV), t, encoder_hidden_states=ctx.to(DEV), dup=2, reuse_kv=False)[0].clone()
    try:
        u.set_tuning("up_fold", 0); plain = run(); fl0 = u.flops_executed(1, dup=2)
        u.set_tuning("up_fold", 1); sub = run(); fl1 = u.flops_executed(1, dup=2)
        assert torch.equal(run(), sub)
        e0, e1 = rel_l2(plain, want), rel_l2(sub, want)
        print(f"\none-plane forward vs the fp32 oracle: fused-upsample kernels {e0:.3e}, sub-pixel upsamplers {e1:.3e}; between them {rel_l2(sub, plain):.3e}")
        assert not torch.equal(sub, plain)
        assert e1 < 1.1 * e0 and e0 < 1.8e-3, (e0, e1)
        # executed FLOPs: the two eligible upsamplers at 4 / 9 (8 x 8 -> 16 x 16 at 1280 channels, 16 x 16 -> 32 x 32 at 640; CFG batch 2)
        saved = 2 * 2.0 * 9 * (16 * 16 * 1280 * 1280 + 32 * 32 * 640 * 640) * 5.0 / 9.0
        assert abs((fl0 - fl1) - saved) < 1e-6 * fl0, (fl0 - fl1, saved)
        # the split stream keeps the exact filters
        u.set_residual_precision("f16x2")
        a = run(); u.set_tuning("up_fold", 0); b = run()
        assert torch.equal(a, b)
        u.set_tuning("up_fold", 2); c = run()
        assert not torch.equal(c, a) and rel_l2(c, want) < 1.05 * rel_l2(a, want) + 2e-5, (rel_l2(c, want), rel_l2(a, want))
    finally:
        u.clear_tuning()


@pytest.mark.parametrize("residual", ["f16x2", "f16"])
def test_forward_does_not_read_uninitialised_workspace(residual):
    """every byte the forward reads from its workspace must have been written by THIS forward (or be the cached cross-attention K/V): the workspace is
    filled with random bytes between two runs and the outputs must be bit-identical.  (Round 4: the MFMA conv_in left GroupNorm statistics for the
    first CFG half only, and the last up block normalised the skip connection at full batch with whatever the arena held.)"""
    for cfg, S in ((dict(layers_per_block=1, sample_size=16), 16), (dict(layers_per_block=1, sample_size=32), 32)):
        u, _ = get_unet(cfg, seed=3, residual=residual)
        lat = torch.randn(2, 4, S, S, generator=torch.Generator().manual_seed(1)).half().to(DEV)
        ctx = synthetic_prompt_embeds(4, seed=11).half().to(DEV)
        for dup, c in ((2, ctx), (1, ctx[:2].contiguous())):
            a = u(lat, 749, encoder_hidden_states=c, dup=dup, reuse_kv=False)[0].clone()
            for fill in (0xFF, 0x7B):                                    # 0xFFFF halfs are NaNs, 0x7B7B large finite values
                u._ws.fill_(fill)
                b = u(lat, 749, encoder_hidden_states=c, dup=dup, reuse_kv=False)[0].clone()
                assert torch.isfinite(b.float()).all() and torch.equal(a, b), (S, dup, fill)


def test_fp32_output_is_the_unrounded_fp16_output_and_threads_keep_their_knob_sets():
    """(a) cs_unet_set_output_dtype (round 6): the fp32 eps is the conv_out accumulator the fp16 eps is rounded from -- rounding it gives the fp16 output bit for bit,
    on both conv_out kernels and on the one-wave-per-pixel fallback; the handle switches back and forth.  (With head_x2, the default on the split stream, both outputs
    additionally carry the product with the lo plane of conv_out's operand where the MFMA kernel runs -- the fp16 one is rounded from the sum: checked with the knob off and on.)
    (b) per-handle knobs are a per-THREAD set (ops.h, TuneSet): a
    thread running a handle with overrides does not change what another thread's forwards on a plain handle see."""
    import threading
    from consolver_amd import ops
    for S in (32, 8):                                                   # 16 x 16 patch kernels / the fallback kernel
        cfg = dict(layers_per_block=1, sample_size=S)
        u, _ = get_unet(cfg, seed=3)
        lat = torch.randn(2, 4, S, S, generator=torch.Generator().manual_seed(2)).half().to(DEV)
        ctx = synthetic_prompt_embeds(4, seed=31).half().to(DEV)
        for mfma in (1, 0):
            ops.set_tuning("conv_out_mfma", mfma); ops.set_tuning("head_x2", 0)
            try:
                y16 = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
                y32 = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False, out_dtype=torch.float32)[0].clone()
                again = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
                ops.set_tuning("head_x2", 1)
                z32 = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False, out_dtype=torch.float32)[0].clone()
                z16 = u(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
            finally:
                ops.set_tuning("conv_out_mfma", 1); ops.set_tuning("head_x2", 1)
            assert y16.dtype == torch.float16 and y32.dtype == torch.float32 and torch.equal(y32.half(), y16) and torch.equal(again, y16)
            assert float((y32 - y16.float()).abs().max()) > 0             # (the fp32 tensor does carry the bits the fp16 one drops)
            assert torch.equal(z32.half(), z16) and rel_l2(z32, y32) < 5e-4      # both outputs are roundings of ONE fp32 value; the two-plane head is a 2^-12-class correction of it
            assert torch.equal(z32, y32) == (not (mfma == 1 and S % 16 == 0))      # ... applied exactly where the MFMA conv_out runs
    with pytest.raises(ValueError):
        u(lat, 499, encoder_hidden_states=ctx, dup=2, out=torch.empty(4, 4, 8, 8, device=DEV, dtype=torch.bfloat16))
    # ---- (b)
    cfg = dict(layers_per_block=1, sample_size=32)
    a, sd = get_unet(cfg, seed=3)
    b = HipUNet2DConditionModel(cfg, device=DEV)
    b.load_state_dict(sd)
    b.set_tuning("xattn_fused", 0).set_tuning("ln_fold", 0)
    lat = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(2)).half().to(DEV)
    ctx = synthetic_prompt_embeds(4, seed=31).half().to(DEV)
    run = lambda m: m(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
    base, alt = run(a), run(b)
    assert not torch.equal(base, alt)
    bad = []

    def worker(m, want, n):
        torch.cuda.set_device(0)
        for _ in range(n):
            if not torch.equal(run(m), want):
                bad.append(m is b)
    ts = [threading.Thread(target=worker, args=(a, base, 12)), threading.Thread(target=worker, args=(b, alt, 12))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad, bad


def test_two_handles_run_different_knob_sets_in_one_process():
    """cs_unet_set_tuning (round 5): kernel-selection knobs per HANDLE.  Two models of the same weights, one with the fused cross-attention block and the folded LayerNorm
    switched off for itself: each reproduces, bit for bit, what the process-wide knobs give when set to its values -- in either call order, with the process-wide state
    untouched afterwards; unknown keys / out-of-range values are rejected."""
    from consolver_amd import ops, _lib as L
    cfg = dict(layers_per_block=1, sample_size=32)
    a, sd = get_unet(cfg, seed=3)
    b = HipUNet2DConditionModel(cfg, device=DEV)
    b.load_state_dict(sd)
    lat = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(2)).half().to(DEV)
    ctx = synthetic_prompt_embeds(4, seed=31).half().to(DEV)
    run = lambda m: m(lat, 499, encoder_hidden_states=ctx, dup=2, reuse_kv=False)[0].clone()
    base = run(a)
    ops.set_tuning("xattn_fused", 0); ops.set_tuning("ln_fold", 0)
    want_alt = run(a)
    ops.set_tuning("xattn_fused", 1); ops.set_tuning("ln_fold", 1)
    assert not torch.equal(base, want_alt)
    b.set_tuning("xattn_fused", 0).set_tuning("ln_fold", 0)
    for order in ((a, b), (b, a), (b, b, a)):
        outs = [run(m) for m in order]
        for m, o in zip(order, outs):
            assert torch.equal(o, want_alt if m is b else base)
    v = __import__("ctypes").c_int()
    for k in ("xattn_fused", "ln_fold"):
        L.check(L.lib().cs_get_tuning(k.encode(), __import__("ctypes").byref(v)))
        assert v.value == 1                                            # the process-wide state is as it was
    with pytest.raises(RuntimeError):
        b.set_tuning("no_such_knob", 1)
    with pytest.raises(RuntimeError):
        b.set_tuning("ln_fold", 7)
    b.clear_tuning()
    assert torch.equal(run(b), base)
