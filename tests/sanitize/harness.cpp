// Sanitizer harness for the HOST side of libconsolver_hip (the reference has no sanitizer story; this is ours).
// Built by tests/test_sanitize_host.py with -fsanitize=address,undefined -fno-gpu-sanitize from the real unet.cpp / vae.cpp / flux.cpp / clip.cpp / vit.cpp / clip_vision.cpp / depth.cpp / ops_api.cpp /
// api.cpp (and through them weights.h, the weight store of every handle, and encoder.h, the CLIP / ViT layer loop) plus tests/sanitize/stubs.cpp (host malloc as
// device memory, launch stubs that touch every tensor's first and last byte).  Drives, without a GPU:
//   weight registration and repacking, finalize, the dry-run workspace sizing (every execution variant, both residual-stream modes), forwards through the
//   first-fit arena with a workspace of EXACTLY the size the library asked for, the profiling event pool, and the error paths;
//   the CLIP, ViT, CLIP vision and Depth Anything handles at their smallest legal shapes; a finalize with one weight missing on each of the seven handles.
#include "../../include/consolver_hip.h"
#include "../../include/consolver_hip_ops.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" int g_stub_fail_memcpy_async;       // stubs.cpp
static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s  (last error: %s)\n", __FILE__, __LINE__, #cond, cs_last_error()); ++g_fail; } } while (0)

static CsUNetConfig unet_config() {
    CsUNetConfig c{};
    c.in_channels = 4; c.out_channels = 4;
    const int boc[4] = {320, 320, 640, 640};
    for (int i = 0; i < 4; ++i) { c.block_out_channels[i] = boc[i]; c.down_has_attn[i] = i < 3; c.up_has_attn[i] = i > 0; }
    c.layers_per_block = 1; c.num_heads = 8; c.cross_attention_dim = 768; c.norm_num_groups = 32; c.sample_size = 32; c.ctx_len = 77;
    return c;
}
static CsVaeConfig vae_config() {
    CsVaeConfig c{};
    c.latent_channels = 4; c.out_channels = 3;
    const int boc[4] = {128, 128, 256, 256};
    for (int i = 0; i < 4; ++i) c.block_out_channels[i] = boc[i];
    c.layers_per_block = 1; c.norm_num_groups = 32; c.sample_size = 16; c.use_post_quant_conv = 1; c.with_encoder = 1; c.use_quant_conv = 1;
    return c;
}
static CsFluxConfig flux_config() {
    CsFluxConfig c{};
    c.in_channels = 64; c.num_layers = 2; c.num_single_layers = 2; c.num_heads = 2; c.head_dim = 128; c.joint_attention_dim = 256; c.pooled_projection_dim = 64;
    c.guidance_embeds = 1; c.axes_dims_rope[0] = 16; c.axes_dims_rope[1] = 56; c.axes_dims_rope[2] = 56; c.dtype = CS_BF16;
    return c;
}
// CLIP and ViT at the smallest shapes their create accepts: hidden 128 = 2 heads of 64, 2 layers, MLP width 128 (ViT: a 3 x 3 training grid, so the position
// table is interpolated to the crop's 2 x 2)
static CsClipConfig clip_config() {
    CsClipConfig c{};
    c.vocab_size = 50; c.hidden_size = 128; c.intermediate_size = 128; c.num_hidden_layers = 2; c.num_attention_heads = 2; c.max_position_embeddings = 8; c.layer_norm_eps = 1e-5f;
    return c;
}
static CsVitConfig vit_config() {
    CsVitConfig c{};
    c.hidden_size = 128; c.num_hidden_layers = 2; c.num_attention_heads = 2; c.mlp_ratio = 1; c.image_size = 42; c.patch_size = 14; c.layer_norm_eps = 1e-6f;
    c.resize_shortest_edge = 28; c.crop_size = 28; c.rescale_factor = 1.0 / 255;
    for (int i = 0; i < 3; ++i) { c.image_mean[i] = 0.5f; c.image_std[i] = 0.25f; }
    return c;
}
// the CLIP vision tower at its smallest shapes, with a projection width that is no multiple of anything
static CsClipVisionConfig clipv_config() {
    CsClipVisionConfig c{};
    c.hidden_size = 128; c.intermediate_size = 128; c.num_hidden_layers = 2; c.num_attention_heads = 2; c.image_size = 28; c.patch_size = 14; c.projection_dim = 24;
    c.layer_norm_eps = 1e-5f; c.resize_shortest_edge = 28; c.crop_size = 28; c.rescale_factor = 1.0 / 255;
    for (int i = 0; i < 3; ++i) { c.image_mean[i] = 0.5f; c.image_std[i] = 0.25f; }
    return c;
}
// Depth Anything at the smallest shapes that take every branch: an odd patch grid (G = 5: the stride-2 map is (G - 1) / 2 + 1 = 3, not G / 2), a tap after every
// layer, neck widths that are padded (48 -> 64, 192 -> 256) and ones that are not
static CsDepthConfig depth_config() {
    CsDepthConfig c{};
    c.hidden_size = 128; c.num_hidden_layers = 4; c.num_attention_heads = 2; c.mlp_ratio = 1; c.image_size = 70; c.patch_size = 14; c.layer_norm_eps = 1e-6f;
    const int nh[4] = {48, 96, 192, 384};
    for (int i = 0; i < 4; ++i) { c.out_indices[i] = i + 1; c.neck_hidden_sizes[i] = nh[i]; }
    c.fusion_hidden_size = 64; c.head_hidden_size = 32; c.max_depth = 1.f; c.size = 70; c.rescale_factor = 1.0 / 255;
    for (int i = 0; i < 3; ++i) { c.image_mean[i] = 0.5f; c.image_std[i] = 0.25f; }
    return c;
}

static void unet_part() {
    CsUNetConfig c = unet_config();
    CsUNet* u = nullptr;
    EXPECT(cs_unet_create(nullptr, &u) != CS_OK);
    CsUNetConfig bad = c; bad.block_out_channels[1] = 100;
    EXPECT(cs_unet_create(&bad, &u) != CS_OK);
    EXPECT(cs_unet_create(&c, &u) == CS_OK);
    EXPECT(cs_unet_workspace_bytes(u, 2) == 0);                       // not finalized
    EXPECT(cs_unet_forward(u, &c, 1, 1, nullptr, 1, &c, &c, &c, 16, 0, nullptr) != CS_OK);
    const int n = cs_unet_num_weights(u);
    EXPECT(n > 100);
    int64_t shape[4]; int nd = 0;
    EXPECT(cs_unet_weight_name(u, -1, shape, &nd) == nullptr && cs_unet_weight_name(u, n, shape, &nd) == nullptr);
    std::vector<float> buf;
    for (int i = 0; i < n; ++i) {
        const char* name = cs_unet_weight_name(u, i, shape, &nd);
        size_t cnt = 1; for (int k = 0; k < nd; ++k) cnt *= (size_t)shape[k];
        buf.assign(cnt, 0.01f);
        if (i == 3) {                                                 // error paths on a real tensor
            int64_t wrong[4] = {shape[0] + 1, shape[1], shape[2], shape[3]};
            EXPECT(cs_unet_set_weight(u, name, buf.data(), wrong, nd) != CS_OK);
            EXPECT(cs_unet_set_weight(u, name, buf.data(), shape, nd + 1) != CS_OK);
            EXPECT(cs_unet_set_weight(u, "no.such.tensor", buf.data(), shape, nd) != CS_OK);
            EXPECT(cs_unet_set_weight(u, name, nullptr, shape, nd) != CS_OK);
        }
        if (i == n - 1) EXPECT(cs_unet_finalize(u) != CS_OK);          // one tensor still missing
        EXPECT(cs_unet_set_weight(u, name, buf.data(), shape, nd) == CS_OK);
    }
    EXPECT(cs_unet_finalize(u) == CS_OK && cs_unet_finalize(u) == CS_OK);
    EXPECT(cs_unet_set_weight(u, "conv_in.bias", buf.data(), shape, 1) != CS_OK);   // packed already
    EXPECT(cs_unet_flops(u, 2) > 0 && cs_unet_flops_executed(u, 2, 2) > 0 && cs_unet_flops_executed(u, 2, 2) < cs_unet_flops_executed(u, 4, 1));
    // per-handle knobs: validated against the knob table, applied around the forwards below, dropped again
    EXPECT(cs_unet_set_tuning(u, "no_such_knob", 1) != CS_OK && cs_unet_set_tuning(u, "ln_fold", 9) != CS_OK && cs_unet_set_tuning(nullptr, "ln_fold", 0) != CS_OK);
    EXPECT(cs_unet_set_tuning(u, "ln_fold", 0) == CS_OK && cs_unet_set_tuning(u, "xattn_fused", 0) == CS_OK);
    EXPECT(cs_unet_set_residual_precision(u, 7) != CS_OK);

    const int S = c.sample_size;
    for (int mode : {CS_RESIDUAL_F16, CS_RESIDUAL_F16X2}) {
        EXPECT(cs_unet_set_residual_precision(u, mode) == CS_OK && cs_unet_get_residual_precision(u) == mode);
        for (int B : {1, 2, 3, 6}) {
            const size_t wsb = cs_unet_workspace_bytes(u, B);
            EXPECT(wsb > 0);
            char* ws = (char*)malloc(wsb);                            // exactly what the library asked for: one byte past it is an ASan error
            std::vector<char> lat((size_t)B * 4 * S * S * 2), ctx((size_t)B * 77 * 768 * 2), out((size_t)B * 4 * S * S * 2);
            std::vector<float> t(B, 499.f);
            struct K { const char* key; int v; };
            const std::vector<std::vector<K>> variants = {{}, {{"cfg_share", 0}}, {{"xattn_fused", 0}}, {{"gn_fuse", 0}}, {{"cfg_share", 0}, {"xattn_fused", 0}, {"gn_fuse", 0}},
                                                          {{"x2_split_a", 0}}, {{"x2_split_a", 3}}, {{"ln_fold", 0}}, {{"ln_fold", 0}, {"xattn_fused", 0}, {"cfg_share", 0}}, {{"conv_in_mfma", 0}}, {{"conv_in_mfma", 0}, {"cfg_share", 0}}, {{"gemm_w8", 0}, {"gemm_lw", 0}, {"conv_lw", 0}}};
            for (auto& var : variants) {
                for (auto& k : var) EXPECT(cs_set_tuning(k.key, k.v) == CS_OK);
                EXPECT(cs_unet_forward(u, lat.data(), B, 1, t.data(), 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_OK);
                EXPECT(cs_unet_forward(u, lat.data(), B, 1, t.data(), B, ctx.data(), out.data(), ws, wsb, 1, nullptr) == CS_OK);      // per-sample timesteps, cached K/V
                if (B % 2 == 0) EXPECT(cs_unet_forward(u, lat.data(), B / 2, 2, t.data(), 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_OK);   // CFG dual batch
                EXPECT(cs_reset_tuning() == CS_OK);
            }
            // profiling pool (events created on first use, reused afterwards)
            EXPECT(cs_unet_set_profiling(u, 1) == CS_OK);
            for (int rep = 0; rep < 2; ++rep) EXPECT(cs_unet_forward(u, lat.data(), B, 1, t.data(), 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_OK);
            double ms, fl, by; int ln;
            for (int i = 0; i < cs_unet_profile_entries(u); ++i) EXPECT(cs_unet_profile_entry(u, i, &ms, &fl, &by, &ln) != nullptr);
            EXPECT(cs_unet_profile_entry(u, 99, &ms, &fl, &by, &ln) == nullptr);
            EXPECT(cs_unet_set_profiling(u, 0) == CS_OK);
            // error paths of the run itself
            EXPECT(cs_unet_forward(u, lat.data(), B, 1, t.data(), 1, ctx.data(), out.data(), ws, wsb / 2, 0, nullptr) != CS_OK);        // arena runs dry mid-forward
            EXPECT(cs_unet_forward(u, lat.data(), B, 1, t.data(), 1, ctx.data(), out.data(), ws, 1024, 0, nullptr) != CS_OK);
            EXPECT(cs_unet_forward(u, lat.data(), B, 3, t.data(), 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) != CS_OK);
            EXPECT(cs_unet_forward(u, nullptr, B, 1, t.data(), 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) != CS_OK);
            EXPECT(cs_unet_forward(u, lat.data(), B, 1, t.data(), B + 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) != CS_OK);
            EXPECT(cs_unet_forward(u, lat.data(), 0, 1, t.data(), 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_OK);            // empty batch: no-op
            free(ws);
        }
    }
    EXPECT(cs_unet_clear_tuning(u) == CS_OK);
    // a workspace sized in one residual mode is refused (not overrun) in the other
    EXPECT(cs_unet_set_residual_precision(u, CS_RESIDUAL_F16) == CS_OK);
    const size_t small = cs_unet_workspace_bytes(u, 2);
    EXPECT(cs_unet_set_residual_precision(u, CS_RESIDUAL_F16X2) == CS_OK);
    EXPECT(cs_unet_workspace_bytes(u, 2) > small);
    {
        char* ws = (char*)malloc(small);
        std::vector<char> lat(2 * 4 * S * S * 2), ctx(2 * 77 * 768 * 2), out(2 * 4 * S * S * 2); float t = 1.f;
        EXPECT(cs_unet_forward(u, lat.data(), 2, 1, &t, 1, ctx.data(), out.data(), ws, small, 0, nullptr) != CS_OK);
        free(ws);
    }
    // round 6, with the handle's own overrides cleared (folded LayerNorms on): byte lo planes of the transformer hidden state (knob lo8: the arena hands out HALF-size
    // planes, the stubs touch exactly that many bytes), per-block unfold masks (cs_unet_calibrate_ln_fold's result), the fp32 output tensor, the calibration forward
    for (int B : {2, 4}) {
        for (unsigned mask : {0u, 0x5u, 0xffffu}) {
            EXPECT(cs_unet_set_ln_unfold_mask(u, mask) == CS_OK && cs_unet_get_ln_unfold_mask(u) == mask);
            const size_t wsb = cs_unet_workspace_bytes(u, B);
            char* ws = (char*)malloc(wsb);
            std::vector<char> lat((size_t)B * 4 * S * S * 2), ctx((size_t)B * 77 * 768 * 2), out((size_t)B * 4 * S * S * 2), out32((size_t)B * 4 * S * S * 4);
            float t = 499.f;
            for (const char* k : {"", "lo8", "cfg_share", "xattn_fused", "x2_sc_skip"}) {
                if (*k) EXPECT(cs_set_tuning(k, 0) == CS_OK);
                EXPECT(cs_unet_forward(u, lat.data(), B, 1, &t, 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_OK);
                EXPECT(cs_unet_forward(u, lat.data(), B / 2, 2, &t, 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_OK);
                EXPECT(cs_reset_tuning() == CS_OK);
            }
            EXPECT(cs_unet_set_output_dtype(u, 9) != CS_OK && cs_unet_set_output_dtype(u, CS_F32) == CS_OK && cs_unet_get_output_dtype(u) == CS_F32);
            EXPECT(cs_unet_forward(u, lat.data(), B / 2, 2, &t, 1, ctx.data(), out32.data(), ws, wsb, 0, nullptr) == CS_OK);
            EXPECT(cs_unet_set_output_dtype(u, CS_F16) == CS_OK);
            if (mask == 0u) {
                unsigned m = 77; float worst = -1.f;
                EXPECT(cs_unet_calibrate_ln_fold(u, lat.data(), B / 2, 2, &t, 1, ctx.data(), out.data(), ws, wsb, 4.0f, nullptr, &m, &worst) == CS_OK && m != 77u && worst >= 0.f);   // (the stubs touch the statistics, they do not compute them)
                EXPECT(cs_unet_set_ln_unfold_mask(u, 0) == CS_OK);
                EXPECT(cs_unet_calibrate_ln_fold(u, lat.data(), B / 2, 2, &t, 1, ctx.data(), out.data(), ws, wsb, 0.0f, nullptr, &m, &worst) != CS_OK);
                EXPECT(cs_unet_calibrate_ln_fold(nullptr, lat.data(), B / 2, 2, &t, 1, ctx.data(), out.data(), ws, wsb, 4.0f, nullptr, &m, &worst) != CS_OK);
            }
            free(ws);
        }
    }
    EXPECT(cs_unet_set_ln_unfold_mask(u, 0) == CS_OK);
    // a failed device copy fails the forward: the CFG dual batch duplicates conv_in's output (conv_in_mfma) and, on the unfused cross-attention path, the
    // shared prefix's residual stream; a half left uninitialised must not come back as CS_OK
    for (int mode : {CS_RESIDUAL_F16, CS_RESIDUAL_F16X2}) {
        EXPECT(cs_unet_set_residual_precision(u, mode) == CS_OK);
        const size_t wsb = cs_unet_workspace_bytes(u, 2);
        char* ws = (char*)malloc(wsb);
        std::vector<char> lat(4 * S * S * 2), ctx(2 * 77 * 768 * 2), out(2 * 4 * S * S * 2); float t = 499.f;
        for (bool prefix_copy_only : {false, true}) {
            if (prefix_copy_only) EXPECT(cs_set_tuning("conv_in_mfma", 0) == CS_OK && cs_set_tuning("xattn_fused", 0) == CS_OK);
            g_stub_fail_memcpy_async = 1;
            EXPECT(cs_unet_forward(u, lat.data(), 1, 2, &t, 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_E_HIP);
            g_stub_fail_memcpy_async = 0;
            EXPECT(cs_unet_forward(u, lat.data(), 1, 2, &t, 1, ctx.data(), out.data(), ws, wsb, 0, nullptr) == CS_OK);
            EXPECT(cs_reset_tuning() == CS_OK);
        }
        free(ws);
    }
    cs_unet_destroy(u);
    cs_unet_destroy(nullptr);
}

static void vae_part() {
    const CsVaeConfig c = vae_config();
    CsVae* v = nullptr;
    EXPECT(cs_vae_create(&c, &v) == CS_OK);
    if (!v) return;
    const int n = cs_vae_num_weights(v);
    int64_t shape[4]; int nd = 0; std::vector<float> buf;
    for (int i = 0; i < n; ++i) {
        const char* name = cs_vae_weight_name(v, i, shape, &nd);
        size_t cnt = 1; for (int k = 0; k < nd; ++k) cnt *= (size_t)shape[k];
        buf.assign(cnt, 0.01f);
        EXPECT(cs_vae_set_weight(v, name, buf.data(), shape, nd) == CS_OK);
    }
    EXPECT(cs_vae_set_weight(v, "decoder.no_such", buf.data(), shape, nd) != CS_OK);
    EXPECT(cs_vae_finalize(v) == CS_OK);
    for (int gn_fuse : {1, 0})
        for (int B : {1, 3}) {
            EXPECT(cs_set_tuning("gn_fuse", 1) == CS_OK);              // the workspace is sized with the knob ON and must serve both settings
            const size_t wsb = cs_vae_workspace_bytes(v, B), web = cs_vae_encode_workspace_bytes(v, B);
            EXPECT(wsb > 0 && web > 0);
            EXPECT(cs_set_tuning("gn_fuse", gn_fuse) == CS_OK);
            EXPECT(cs_vae_workspace_bytes(v, B) == wsb);               // ... and does not depend on it
            const int S = c.sample_size;
            std::vector<char> lat((size_t)B * 4 * S * S * 2), img((size_t)B * 3 * 64 * S * S * 2);
            char* ws = (char*)malloc(wsb);
            EXPECT(cs_vae_decode(v, lat.data(), B, 1.0f / 0.18215f, 0.f, img.data(), 1, ws, wsb, nullptr) == CS_OK);
            EXPECT(cs_vae_decode(v, lat.data(), B, 1.0f, 0.f, img.data(), 1, ws, wsb / 4, nullptr) != CS_OK);
            free(ws);
            ws = (char*)malloc(web);
            EXPECT(cs_vae_encode(v, img.data(), B, 0.18215f, 0.f, lat.data(), ws, web, nullptr) == CS_OK);
            free(ws);
        }
    EXPECT(cs_reset_tuning() == CS_OK);
    cs_vae_destroy(v);
}

static void flux_part() {
    const CsFluxConfig c = flux_config();
    CsFlux* f = nullptr;
    EXPECT(cs_flux_create(&c, &f) == CS_OK);
    if (!f) return;
    const int n = cs_flux_num_weights(f);
    int64_t shape[4]; int nd = 0; std::vector<unsigned short> buf;
    for (int i = 0; i < n; ++i) {
        const char* name = cs_flux_weight_name(f, i, shape, &nd);
        size_t cnt = 1; for (int k = 0; k < nd; ++k) cnt *= (size_t)shape[k];
        buf.assign(cnt, 0x3c00);
        if (i == 5) { int64_t wrong[2] = {shape[0] + 1, shape[1]}; EXPECT(cs_flux_set_weight(f, name, buf.data(), 0, wrong, nd) != CS_OK); }
        EXPECT(cs_flux_set_weight(f, name, buf.data(), 0, shape, nd) == CS_OK);
    }
    EXPECT(cs_flux_finalize(f) == CS_OK);
    EXPECT(cs_flux_set_residual_precision(f, 5) != CS_OK && cs_flux_get_residual_precision(f) == CS_RESIDUAL_F16X2);       // default: split hidden-state stream
    for (int mode : {CS_RESIDUAL_F16X2, CS_RESIDUAL_F16})
    for (int B : {1, 2}) {
        EXPECT(cs_flux_set_residual_precision(f, mode) == CS_OK && cs_flux_get_residual_precision(f) == mode);
        const int T = 64, Lq = 256, Li = 256, D2 = c.head_dim / 2;
        const size_t wsb = cs_flux_workspace_bytes(f, B, T, Lq + Li);
        EXPECT(wsb > 0 && cs_flux_flops(f, B, T, Lq + Li) > 0);
        char* ws = (char*)malloc(wsb);
        std::vector<char> lat((size_t)B * Lq * 64 * 2), img((size_t)B * Li * 64 * 2), enc((size_t)B * T * 256 * 2), out((size_t)B * (Lq + Li) * 64 * 2);
        std::vector<float> pooled(B * 64, 0.1f), ts(B, 0.5f), gd(B, 2.5f), rc((size_t)(T + Lq + Li) * D2, 1.f), rs((size_t)(T + Lq + Li) * D2, 0.f);
        EXPECT(cs_flux_forward_joint(f, lat.data(), Lq, img.data(), Li, B, enc.data(), T, pooled.data(), ts.data(), gd.data(), rc.data(), rs.data(), out.data(), ws, wsb, nullptr) == CS_OK);
        std::vector<char> hid((size_t)B * (Lq + Li) * 64 * 2);
        EXPECT(cs_flux_forward(f, hid.data(), B, Lq + Li, enc.data(), T, pooled.data(), ts.data(), gd.data(), rc.data(), rs.data(), out.data(), ws, wsb, nullptr) == CS_OK);
        EXPECT(cs_flux_forward(f, hid.data(), B, Lq + Li, enc.data(), T, pooled.data(), ts.data(), gd.data(), rc.data(), rs.data(), out.data(), ws, wsb / 3, nullptr) != CS_OK);
        free(ws);
        // round 6: the fp32 output (the output head's two planes summed; split stream only): its own workspace query, an fp32 `out`, refused on the one-plane stream
        EXPECT(cs_flux_set_output_dtype(f, 77) != CS_OK && cs_flux_set_output_dtype(f, CS_F32) == CS_OK && cs_flux_get_output_dtype(f) == CS_F32);
        {
            const size_t wsb32 = cs_flux_workspace_bytes(f, B, T, Lq + Li);
            char* ws32 = (char*)malloc(wsb32);
            std::vector<char> out32((size_t)B * (Lq + Li) * 64 * 4);
            const int rc32 = cs_flux_forward_joint(f, lat.data(), Lq, img.data(), Li, B, enc.data(), T, pooled.data(), ts.data(), gd.data(), rc.data(), rs.data(), out32.data(), ws32, wsb32, nullptr);
            EXPECT((rc32 == CS_OK) == (mode == CS_RESIDUAL_F16X2));
            free(ws32);
        }
        EXPECT(cs_flux_set_output_dtype(f, c.dtype) == CS_OK && cs_flux_get_output_dtype(f) == c.dtype);
    }
    cs_flux_destroy(f);
}

// the sequence every float handle goes through before its first run: the error paths of set_weight on a real tensor, every weight set, finalize (twice), a set
// after finalize.  set(name, data, shape, ndim) and finalize() are the handle's own entry points
template <typename NameAt, typename Set, typename Finalize>
static void load_all_weights(int n, NameAt name_at, Set set, Finalize finalize) {
    int64_t shape[4]; int nd = 0;
    std::vector<float> buf;
    EXPECT(n > 10 && name_at(-1, shape, &nd) == nullptr && name_at(n, shape, &nd) == nullptr);
    for (int i = 0; i < n; ++i) {
        const char* name = name_at(i, shape, &nd);
        size_t cnt = 1; for (int k = 0; k < nd; ++k) cnt *= (size_t)shape[k];
        buf.assign(cnt, 0.01f);
        if (i == 3) {
            int64_t wrong[4] = {shape[0] + 1, shape[1], shape[2], shape[3]};
            EXPECT(set(name, buf.data(), wrong, nd) == CS_E_SHAPE);
            EXPECT(set(name, buf.data(), shape, nd + 1) == CS_E_SHAPE);
            EXPECT(set("no.such.tensor", buf.data(), shape, nd) == CS_E_ARG);
            EXPECT(set(name, nullptr, shape, nd) == CS_E_ARG && set(nullptr, buf.data(), shape, nd) == CS_E_ARG && set(name, buf.data(), nullptr, nd) == CS_E_ARG);
        }
        EXPECT(set(name, buf.data(), shape, nd) == CS_OK);
    }
    EXPECT(finalize() == CS_OK && finalize() == CS_OK);
    const char* first = name_at(0, shape, &nd);
    buf.assign(1 << 16, 0.f);
    EXPECT(set(first, buf.data(), shape, nd) == CS_E_STATE);          // packed already
}

static void clip_part() {
    const CsClipConfig c = clip_config();
    CsClip* h = nullptr;
    CsClipConfig bad = c; bad.hidden_size = 192;
    EXPECT(cs_clip_create(&bad, &h) != CS_OK && cs_clip_create(nullptr, &h) != CS_OK);
    EXPECT(cs_clip_create(&c, &h) == CS_OK);
    if (!h) return;
    const int B = 2, T = 8;
    const size_t wsb = cs_clip_workspace_bytes(h, B, T);
    char* ws = (char*)malloc(wsb);
    std::vector<int64_t> ids((size_t)B * T, 7);
    std::vector<char> out((size_t)B * T * c.hidden_size * 2);
    EXPECT(cs_clip_encode(h, ids.data(), B, T, out.data(), ws, wsb, nullptr) == CS_E_STATE);        // not finalized
    EXPECT(cs_clip_set_weight(nullptr, "x", nullptr, nullptr, 0) == CS_E_ARG);
    load_all_weights(cs_clip_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_clip_weight_name(h, i, sh, nd); },
                     [&](const char* n, const float* d, const int64_t* sh, int nd) { return cs_clip_set_weight(h, n, d, sh, nd); }, [&] { return cs_clip_finalize(h); });
    EXPECT(wsb > 0 && cs_clip_workspace_bytes(h, B, T) == wsb && cs_clip_flops(h, B, T) > 0);
    EXPECT(cs_clip_encode(h, ids.data(), B, T, out.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_clip_encode(h, ids.data(), B, T, out.data(), ws, wsb - 1, nullptr) != CS_OK);
    EXPECT(cs_clip_encode(h, ids.data(), B, T + 1, out.data(), ws, wsb, nullptr) == CS_E_SHAPE);   // past max_position_embeddings
    EXPECT(cs_clip_encode(h, nullptr, B, T, out.data(), ws, wsb, nullptr) != CS_OK);
    EXPECT(cs_clip_encode(h, ids.data(), 0, T, out.data(), ws, wsb, nullptr) == CS_OK);             // empty batch: no-op
    free(ws);
    cs_clip_destroy(h);
    cs_clip_destroy(nullptr);
}

static void vit_part() {
    const CsVitConfig c = vit_config();
    CsVit* h = nullptr;
    CsVitConfig bad = c; bad.crop_size = 30;
    EXPECT(cs_vit_create(&bad, &h) != CS_OK && cs_vit_create(nullptr, &h) != CS_OK);
    EXPECT(cs_vit_create(&c, &h) == CS_OK);
    if (!h) return;
    const int B = 2, NP = 4, Kpad = cs_vit_patch_cols(h);
    EXPECT(Kpad == 640 && cs_vit_num_tokens(h) == NP + 1);
    const size_t wsb = cs_vit_workspace_bytes(h, B);
    char* ws = (char*)malloc(wsb);
    std::vector<char> patches((size_t)B * NP * Kpad * 2);
    std::vector<float> cls((size_t)B * c.hidden_size), reward(B);
    EXPECT(cs_vit_forward(h, patches.data(), B, cls.data(), ws, wsb, nullptr) == CS_E_STATE);       // not finalized
    EXPECT(cs_vit_set_weight(nullptr, "x", nullptr, nullptr, 0) == CS_E_ARG);
    load_all_weights(cs_vit_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_vit_weight_name(h, i, sh, nd); },
                     [&](const char* n, const float* d, const int64_t* sh, int nd) { return cs_vit_set_weight(h, n, d, sh, nd); }, [&] { return cs_vit_finalize(h); });
    EXPECT(wsb > 0 && cs_vit_workspace_bytes(h, B) == wsb && cs_vit_flops(h, B) > 0);
    {   // the front end on an image that is resized and cropped, its workspace exactly what the library asked for
        const int H = 40, W = 56;
        const size_t pwb = cs_vit_preprocess_workspace_bytes(h, B, H, W);
        char* pws = (char*)malloc(pwb);
        std::vector<float> img((size_t)B * 3 * H * W, 0.5f);
        std::vector<unsigned char> crop((size_t)B * 3 * c.crop_size * c.crop_size);
        EXPECT(pwb > 0 && cs_vit_preprocess(h, img.data(), CS_F32, B, H, W, patches.data(), crop.data(), pws, pwb, nullptr) == CS_OK);
        EXPECT(cs_vit_preprocess(h, img.data(), CS_F32, B, 14, 14 * 3, patches.data(), nullptr, pws, pwb, nullptr) == CS_OK);      // a second size: a second table
        EXPECT(cs_vit_preprocess(h, img.data(), CS_F32, B, H, W, patches.data(), nullptr, pws, 16, nullptr) != CS_OK);
        free(pws);
    }
    EXPECT(cs_vit_forward(h, patches.data(), B, cls.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_vit_forward(h, patches.data(), B, cls.data(), ws, wsb - 1, nullptr) != CS_OK);
    EXPECT(cs_vit_forward(h, nullptr, B, cls.data(), ws, wsb, nullptr) != CS_OK);
    EXPECT(cs_vit_forward(h, patches.data(), 0, cls.data(), ws, wsb, nullptr) == CS_OK);            // empty batch: no-op
    EXPECT(cs_cosine_reward(cls.data(), cls.data(), B, c.hidden_size, 0, reward.data(), nullptr) == CS_OK);
    free(ws);
    cs_vit_destroy(h);
    cs_vit_destroy(nullptr);
}

static void clipv_part() {
    const CsClipVisionConfig c = clipv_config();
    CsClipVision* h = nullptr;
    CsClipVisionConfig bad = c; bad.crop_size = 14;
    EXPECT(cs_clipv_create(&bad, &h) == CS_E_UNSUPPORTED && cs_clipv_create(nullptr, &h) != CS_OK);
    EXPECT(cs_clipv_create(&c, &h) == CS_OK);
    if (!h) return;
    const int B = 2, NP = 4, Kpad = cs_clipv_patch_cols(h);
    EXPECT(Kpad == 640 && cs_clipv_num_tokens(h) == NP + 1);
    const size_t wsb = cs_clipv_workspace_bytes(h, B);
    char* ws = (char*)malloc(wsb);
    std::vector<char> patches((size_t)B * NP * Kpad * 2);
    std::vector<float> embeds((size_t)B * c.projection_dim);
    EXPECT(cs_clipv_forward(h, patches.data(), B, embeds.data(), ws, wsb, nullptr) == CS_E_STATE);       // not finalized
    EXPECT(cs_clipv_set_weight(nullptr, "x", nullptr, nullptr, 0) == CS_E_ARG);
    load_all_weights(cs_clipv_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_clipv_weight_name(h, i, sh, nd); },
                     [&](const char* n, const float* d, const int64_t* sh, int nd) { return cs_clipv_set_weight(h, n, d, sh, nd); }, [&] { return cs_clipv_finalize(h); });
    EXPECT(wsb > 0 && cs_clipv_workspace_bytes(h, B) == wsb && cs_clipv_flops(h, B) > 0);
    {   // the front end on an image that is resized and cropped, its workspace exactly what the library asked for
        const int H = 40, W = 56;
        const size_t pwb = cs_clipv_preprocess_workspace_bytes(h, B, H, W);
        char* pws = (char*)malloc(pwb);
        std::vector<float> img((size_t)B * 3 * H * W, 0.5f);
        std::vector<unsigned char> crop((size_t)B * 3 * c.crop_size * c.crop_size);
        EXPECT(pwb > 0 && cs_clipv_preprocess(h, img.data(), CS_F32, B, H, W, patches.data(), crop.data(), pws, pwb, nullptr) == CS_OK);
        EXPECT(cs_clipv_preprocess(h, img.data(), CS_F32, B, 14, 14 * 3, patches.data(), nullptr, pws, pwb, nullptr) == CS_OK);      // a second size: a second table
        EXPECT(cs_clipv_preprocess(h, img.data(), CS_F32, B, H, W, patches.data(), nullptr, pws, 16, nullptr) != CS_OK);
        EXPECT(cs_clipv_preprocess(h, nullptr, CS_F32, B, H, W, patches.data(), nullptr, pws, pwb, nullptr) == CS_E_ARG);
        EXPECT(cs_clipv_preprocess(h, nullptr, CS_F32, 0, H, W, nullptr, nullptr, nullptr, 0, nullptr) == CS_OK);                   // empty batch: no-op
        free(pws);
    }
    EXPECT(cs_clipv_forward(h, patches.data(), B, embeds.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_clipv_forward(h, patches.data(), B, embeds.data(), ws, wsb - 1, nullptr) != CS_OK);
    EXPECT(cs_clipv_forward(h, nullptr, B, embeds.data(), ws, wsb, nullptr) != CS_OK);
    EXPECT(cs_clipv_forward(h, patches.data(), B, nullptr, ws, wsb, nullptr) != CS_OK && cs_clipv_forward(h, patches.data(), B, embeds.data(), nullptr, wsb, nullptr) != CS_OK);
    EXPECT(cs_clipv_forward(nullptr, patches.data(), B, embeds.data(), ws, wsb, nullptr) == CS_E_ARG && cs_clipv_forward(h, patches.data(), -1, embeds.data(), ws, wsb, nullptr) == CS_E_ARG);
    EXPECT(cs_clipv_forward(h, patches.data(), 0, embeds.data(), ws, wsb, nullptr) == CS_OK);            // empty batch: no-op
    free(ws);
    cs_clipv_destroy(h);
    cs_clipv_destroy(nullptr);
}

static void depth_part() {
    const CsDepthConfig c = depth_config();
    CsDepth* h = nullptr;
    CsDepthConfig bad = c; bad.out_indices[2] = 2;
    EXPECT(cs_depth_create(&bad, &h) == CS_E_ARG && cs_depth_create(nullptr, &h) != CS_OK);
    bad = c; bad.size = 84;
    EXPECT(cs_depth_create(&bad, &h) == CS_E_UNSUPPORTED);
    EXPECT(cs_depth_create(&c, &h) == CS_OK);
    if (!h) return;
    const int B = 2, S = c.size, NP = 25, Kpad = cs_depth_patch_cols(h);
    EXPECT(Kpad == 640 && cs_depth_num_tokens(h) == NP + 1);
    const size_t wsb = cs_depth_workspace_bytes(h, B);
    char* ws = (char*)malloc(wsb);
    std::vector<char> patches((size_t)B * NP * Kpad * 2);
    std::vector<float> depth((size_t)B * S * S);
    EXPECT(cs_depth_forward(h, patches.data(), B, depth.data(), ws, wsb, nullptr) == CS_E_STATE);        // not finalized
    EXPECT(cs_depth_set_weight(nullptr, "x", nullptr, nullptr, 0) == CS_E_ARG);
    load_all_weights(cs_depth_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_depth_weight_name(h, i, sh, nd); },
                     [&](const char* n, const float* d, const int64_t* sh, int nd) { return cs_depth_set_weight(h, n, d, sh, nd); }, [&] { return cs_depth_finalize(h); });
    EXPECT(wsb > 0 && cs_depth_workspace_bytes(h, B) == wsb && cs_depth_flops(h, B) > 0);
    {   // the front end on a square image that is resized (up, then down), its workspace exactly what the library asked for; other shapes are refused
        const int H = 40;
        const size_t pwb = cs_depth_preprocess_workspace_bytes(h, B, H, H);
        char* pws = (char*)malloc(pwb);
        std::vector<float> img((size_t)B * 3 * 96 * 96, 0.5f);
        std::vector<unsigned char> crop((size_t)B * 3 * S * S);
        EXPECT(pwb > 0 && cs_depth_preprocess(h, img.data(), CS_F32, B, H, H, patches.data(), crop.data(), pws, pwb, nullptr) == CS_OK);
        EXPECT(cs_depth_preprocess(h, img.data(), CS_F32, B, H, H, patches.data(), nullptr, pws, 16, nullptr) != CS_OK);
        EXPECT(cs_depth_preprocess(h, img.data(), CS_F32, B, H, 56, patches.data(), nullptr, pws, pwb, nullptr) == CS_E_UNSUPPORTED);   // not square
        EXPECT(cs_depth_preprocess(h, img.data(), CS_F32, 0, H, 56, patches.data(), nullptr, pws, pwb, nullptr) == CS_E_UNSUPPORTED);   // ... refused before the empty batch returns
        EXPECT(cs_depth_preprocess(h, nullptr, CS_F32, B, H, H, patches.data(), nullptr, pws, pwb, nullptr) == CS_E_ARG);
        EXPECT(cs_depth_preprocess(h, nullptr, CS_F32, 0, H, H, nullptr, nullptr, nullptr, 0, nullptr) == CS_OK);                        // empty batch: no-op
        free(pws);
        const size_t pwb2 = cs_depth_preprocess_workspace_bytes(h, B, 96, 96);
        pws = (char*)malloc(pwb2);
        EXPECT(pwb2 > pwb && cs_depth_preprocess(h, img.data(), CS_F32, B, 96, 96, patches.data(), nullptr, pws, pwb2, nullptr) == CS_OK);   // a second size: a second table
        free(pws);
    }
    EXPECT(cs_depth_forward(h, patches.data(), B, depth.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_depth_forward(h, patches.data(), B, depth.data(), ws, wsb - 1, nullptr) != CS_OK);
    EXPECT(cs_depth_forward(h, nullptr, B, depth.data(), ws, wsb, nullptr) != CS_OK);
    EXPECT(cs_depth_forward(h, patches.data(), B, nullptr, ws, wsb, nullptr) != CS_OK && cs_depth_forward(h, patches.data(), B, depth.data(), nullptr, wsb, nullptr) != CS_OK);
    EXPECT(cs_depth_forward(nullptr, patches.data(), B, depth.data(), ws, wsb, nullptr) == CS_E_ARG && cs_depth_forward(h, patches.data(), -1, depth.data(), ws, wsb, nullptr) == CS_E_ARG);
    EXPECT(cs_depth_forward(h, patches.data(), 0, depth.data(), ws, wsb, nullptr) == CS_OK);             // empty batch: no-op
    {   // the post-processing to a size that is not the model's
        const int H = 40, W = 56;
        std::vector<float> maps((size_t)B * H * W);
        EXPECT(cs_depth_normalized_maps(h, depth.data(), B, H, W, maps.data(), nullptr) == CS_OK);
        EXPECT(cs_depth_normalized_maps(h, depth.data(), B, 0, W, maps.data(), nullptr) == CS_E_ARG && cs_depth_normalized_maps(h, nullptr, B, H, W, maps.data(), nullptr) == CS_E_ARG);
        EXPECT(cs_depth_normalized_maps(nullptr, depth.data(), B, H, W, maps.data(), nullptr) == CS_E_ARG && cs_depth_normalized_maps(h, depth.data(), 0, H, W, maps.data(), nullptr) == CS_OK);
    }
    free(ws);
    cs_depth_destroy(h);
    cs_depth_destroy(nullptr);
}

// every weight but the last one set: finalize refuses with CS_E_STATE and names the tensor; what was staged is released by destroy (leak checking)
template <typename NameAt, typename Set, typename Finalize>
static void finalize_with_one_missing(int n, NameAt name_at, Set set, Finalize finalize) {
    int64_t shape[4]; int nd = 0;
    for (int i = 0; i + 1 < n; ++i) {
        const char* name = name_at(i, shape, &nd);
        size_t cnt = 1; for (int k = 0; k < nd; ++k) cnt *= (size_t)shape[k];
        EXPECT(set(name, cnt, shape, nd) == CS_OK);
    }
    const std::string last = name_at(n - 1, shape, &nd);
    EXPECT(finalize() == CS_E_STATE && std::string(cs_last_error()) == "missing weight '" + last + "'");
}

static void missing_weight_part() {
    std::vector<float> buf;
    std::vector<unsigned short> buf16;
    {
        const CsUNetConfig c = unet_config(); CsUNet* h = nullptr;
        EXPECT(cs_unet_create(&c, &h) == CS_OK);
        finalize_with_one_missing(cs_unet_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_unet_weight_name(h, i, sh, nd); },
                                  [&](const char* n, size_t cnt, const int64_t* sh, int nd) { buf.assign(cnt, 0.01f); return cs_unet_set_weight(h, n, buf.data(), sh, nd); },
                                  [&] { return cs_unet_finalize(h); });
        cs_unet_destroy(h);
    }
    {
        const CsVaeConfig c = vae_config(); CsVae* h = nullptr;
        EXPECT(cs_vae_create(&c, &h) == CS_OK);
        finalize_with_one_missing(cs_vae_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_vae_weight_name(h, i, sh, nd); },
                                  [&](const char* n, size_t cnt, const int64_t* sh, int nd) { buf.assign(cnt, 0.01f); return cs_vae_set_weight(h, n, buf.data(), sh, nd); },
                                  [&] { return cs_vae_finalize(h); });
        cs_vae_destroy(h);
    }
    {
        const CsClipConfig c = clip_config(); CsClip* h = nullptr;
        EXPECT(cs_clip_create(&c, &h) == CS_OK);
        finalize_with_one_missing(cs_clip_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_clip_weight_name(h, i, sh, nd); },
                                  [&](const char* n, size_t cnt, const int64_t* sh, int nd) { buf.assign(cnt, 0.01f); return cs_clip_set_weight(h, n, buf.data(), sh, nd); },
                                  [&] { return cs_clip_finalize(h); });
        cs_clip_destroy(h);
    }
    {
        const CsVitConfig c = vit_config(); CsVit* h = nullptr;
        EXPECT(cs_vit_create(&c, &h) == CS_OK);
        finalize_with_one_missing(cs_vit_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_vit_weight_name(h, i, sh, nd); },
                                  [&](const char* n, size_t cnt, const int64_t* sh, int nd) { buf.assign(cnt, 0.01f); return cs_vit_set_weight(h, n, buf.data(), sh, nd); },
                                  [&] { return cs_vit_finalize(h); });
        cs_vit_destroy(h);
    }
    {
        const CsClipVisionConfig c = clipv_config(); CsClipVision* h = nullptr;
        EXPECT(cs_clipv_create(&c, &h) == CS_OK);
        finalize_with_one_missing(cs_clipv_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_clipv_weight_name(h, i, sh, nd); },
                                  [&](const char* n, size_t cnt, const int64_t* sh, int nd) { buf.assign(cnt, 0.01f); return cs_clipv_set_weight(h, n, buf.data(), sh, nd); },
                                  [&] { return cs_clipv_finalize(h); });
        cs_clipv_destroy(h);
    }
    {
        const CsDepthConfig c = depth_config(); CsDepth* h = nullptr;
        EXPECT(cs_depth_create(&c, &h) == CS_OK);
        finalize_with_one_missing(cs_depth_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_depth_weight_name(h, i, sh, nd); },
                                  [&](const char* n, size_t cnt, const int64_t* sh, int nd) { buf.assign(cnt, 0.01f); return cs_depth_set_weight(h, n, buf.data(), sh, nd); },
                                  [&] { return cs_depth_finalize(h); });
        cs_depth_destroy(h);
    }
    {
        const CsFluxConfig c = flux_config(); CsFlux* h = nullptr;
        EXPECT(cs_flux_create(&c, &h) == CS_OK);
        finalize_with_one_missing(cs_flux_num_weights(h), [&](int i, int64_t* sh, int* nd) { return cs_flux_weight_name(h, i, sh, nd); },
                                  [&](const char* n, size_t cnt, const int64_t* sh, int nd) { buf16.assign(cnt, 0x3c00); return cs_flux_set_weight(h, n, buf16.data(), 0, sh, nd); },
                                  [&] { return cs_flux_finalize(h); });
        cs_flux_destroy(h);
    }
}

int main() {
    EXPECT(cs_abi_version() == 2);
    EXPECT(cs_set_tuning("conv_lw", 5) != CS_OK && cs_set_tuning("no_such_knob", 1) != CS_OK && cs_set_tuning("attn_qt40", 3) != CS_OK);
    int v = -7;
    EXPECT(cs_get_tuning("conv_lw", &v) == CS_OK && v == 1);
    unet_part();
    vae_part();
    flux_part();
    clip_part();
    vit_part();
    clipv_part();
    depth_part();
    missing_weight_part();
    if (g_fail) { fprintf(stderr, "%d expectation(s) failed\n", g_fail); return 1; }
    printf("sanitize harness: ok\n");
    return 0;
}
