// Depth Anything V2 depth estimator: the depth maps of the depth-PSNR reward (reward_type "depth": edit_ppo/reward_model.py:92-96, 359-422).
//
// Replaces, for a batch of decoded images [B,3,H,W] in [0,1]:  ToPILImage -> the DPT image processor of depth-anything/Depth-Anything-V2-Small-hf (PIL bicubic
// resize to 518 x 518 for a square input, rescale, normalise) -> transformers DepthAnythingForDepthEstimation (DINOv2 backbone with the final LayerNorm applied to
// the hidden states after `out_indices` layers; reassemble stage; neck convs; four fusion layers; three-conv head) -> post_process_depth_estimation (bicubic to
// H x W) -> per-map min / max normalisation.  The front end is the DINOv2 reward's (vit_ops.hip) with resize edge = crop = size; the layer stack is encoder.h's
// loop run in ranges between the taps; the neck and the head are dpt_ops.hip (NHWC fp16, fp32 accumulation).  Packing, all in fp32 with one rounding to fp16:
//   * LayerScale into out-proj / fc2 (pack_pre_ln_layer);
//   * each reassemble layer's 1x1 projection INTO its transposed conv (kernel = stride k: one tap per output pixel, so projection + resize is one linear map from
//     the token to its k x k output pixels): one GEMM [tokens][D] x [k k C][D]^T through launch_igemm, then the pixel-shuffle store;
//   * channel counts the kernels cannot take are zero-padded in the weights of the layer that produces them and of the one that consumes them (48 -> 64 for the
//     narrow conv's 32-channel k step; 192 -> 256 for the GEMM's 128-column tile).
#include "depth_model.h"
#include "../../include/consolver_hip_ops.h"

using depth_model::DConv;
using depth_model::Fusion;
using depth_model::RK;

namespace {

const TowerNames NAMES = {"depth", "depth", "depth handle is NULL"};

// stored channel count of reassembled map i: a multiple of 32 (the narrow conv's k step) whose GEMM width k k cp fits launch_igemm; map 3 is also the
// stride-2 conv's input and output (Cin % 64, N % 128 or N % 160)
int padded_channels(int C, int k, bool conv_operand) {
    for (int cp = (C + 31) / 32 * 32;; cp += 32) {
        const int n = k * k * cp;
        if ((n % 128 == 0 || n % 160 == 0) && (!conv_operand || cp % 64 == 0)) return cp;
    }
}

void build_manifest(CsDepth* c) {          // transformers DepthAnythingForDepthEstimation.state_dict() order
    WeightManifest& m = c->tower.weights;
    const int D = c->tower.D, F = c->F;
    image_tower::expect_dinov2_backbone(m, "backbone.", D, c->tower.I, c->tower.P, c->cfg.image_size / c->cfg.patch_size, c->cfg.num_hidden_layers);
    for (int i = 0; i < 4; ++i) {
        const std::string p = "neck.reassemble_stage.layers." + std::to_string(i);
        const int C = c->cfg.neck_hidden_sizes[i];
        m.expect(p + ".projection.weight", {C, D, 1, 1}); m.expect(p + ".projection.bias", {C});
        if (i == 2) continue;                                                  // factor 1: identity
        const int k = i == 3 ? 3 : RK[i];
        m.expect(p + ".resize.weight", {C, C, k, k}); m.expect(p + ".resize.bias", {C});
    }
    for (int i = 0; i < 4; ++i) m.expect("neck.convs." + std::to_string(i) + ".weight", {F, c->cfg.neck_hidden_sizes[i], 3, 3});
    for (int i = 0; i < 4; ++i) {
        const std::string p = "neck.fusion_stage.layers." + std::to_string(i);
        m.expect(p + ".projection.weight", {F, F, 1, 1}); m.expect(p + ".projection.bias", {F});
        for (const char* r : {".residual_layer1", ".residual_layer2"})          // (layer 0's residual_layer1 is in the checkpoint; its forward has no skip input)
            for (const char* q : {".convolution1", ".convolution2"}) {
                m.expect(p + r + q + ".weight", {F, F, 3, 3}); m.expect(p + r + q + ".bias", {F});
            }
    }
    m.expect("head.conv1.weight", {F / 2, F, 3, 3}); m.expect("head.conv1.bias", {F / 2});
    m.expect("head.conv2.weight", {c->HH, F / 2, 3, 3}); m.expect("head.conv2.bias", {c->HH});
    m.expect("head.conv3.weight", {1, c->HH, 1, 1}); m.expect("head.conv3.bias", {1});
}

// [co][ci][kh][kw] -> [copad][kh kw][cipad], zero padded
std::vector<float> pack_conv_padded(const HostTensor<float>& t, int copad, int cipad) {
    const int64_t co = t.shape[0], ci = t.shape[1], kk = t.shape[2] * t.shape[3];
    std::vector<float> o((size_t)copad * kk * cipad, 0.f);
    for (int64_t n = 0; n < co; ++n)
        for (int64_t ch = 0; ch < ci; ++ch)
            for (int64_t k = 0; k < kk; ++k) o[((size_t)n * kk + k) * cipad + ch] = t.data[(n * ci + ch) * kk + k];
    return o;
}
std::vector<float> pad_vector(const std::vector<float>& v, int n) {
    std::vector<float> o((size_t)n, 0.f);
    std::copy(v.begin(), v.end(), o.begin());
    return o;
}

// the backbone's layers up to the last tap (the ones behind it feed nothing), then the neck and the head with the folds of the header comment
bool pack(CsDepth* c) {
    WeightStore<float>& W = c->tower.weights;
    auto T = [&](const std::string& n) -> const std::vector<float>& { return W.at(n).data; };
    const int D = c->tower.D, F = c->F;
    bool ok = image_tower::pack_dinov2_backbone(c->tower, "backbone.", c->cfg.image_size / c->cfg.patch_size, c->cfg.out_indices[3]);
    if (ok) {          // the trained grid without its class row, in fp32: what cs_depth_forward_hw interpolates for another grid
        const auto& pos = T("backbone.embeddings.position_embeddings");
        c->pos_grid = W.upload_f32(std::vector<float>(pos.begin() + D, pos.end()));
        ok = c->pos_grid != nullptr;
    }
    for (int i = 0; i < 4 && ok; ++i) {
        // reassemble layer i as one linear map: row (ky k + kx) cp + co of the GEMM = sum_ci resize[ci][co][ky][kx] projection[ci][:] (k = 1: the projection itself)
        const std::string p = "neck.reassemble_stage.layers." + std::to_string(i);
        const int C = c->cfg.neck_hidden_sizes[i], k = RK[i], cp = c->cp[i];
        const auto& pw = T(p + ".projection.weight");
        const auto& pb = T(p + ".projection.bias");
        std::vector<float> w((size_t)k * k * cp * D, 0.f), b((size_t)k * k * cp, 0.f);
        if (k == 1) {
            std::copy(pw.begin(), pw.end(), w.begin());
            std::copy(pb.begin(), pb.end(), b.begin());
        } else {
            const auto& rw = T(p + ".resize.weight");          // ConvTranspose2d: [in][out][k][k]
            const auto& rb = T(p + ".resize.bias");
            std::vector<double> acc(D);
            for (int t = 0; t < k * k; ++t)
                for (int co = 0; co < C; ++co) {
                    std::fill(acc.begin(), acc.end(), 0.0);
                    double bacc = rb[co];
                    for (int ci = 0; ci < C; ++ci) {
                        const double r = rw[((size_t)ci * C + co) * k * k + t];
                        bacc += r * pb[ci];
                        const float* prow = pw.data() + (size_t)ci * D;
                        for (int d = 0; d < D; ++d) acc[d] += r * prow[d];
                    }
                    float* dst = w.data() + ((size_t)t * cp + co) * D;
                    for (int d = 0; d < D; ++d) dst[d] = (float)acc[d];
                    b[(size_t)t * cp + co] = (float)bacc;
                }
        }
        c->reasm[i].w = W.upload(w); c->reasm[i].b = W.upload(b);
        c->neck[i].w = W.upload(pack_conv_padded(W.at("neck.convs." + std::to_string(i) + ".weight"), F, cp));
        ok = c->reasm[i].w && c->reasm[i].b && c->neck[i].w;
    }
    if (ok) {
        const std::string p = "neck.reassemble_stage.layers.3.resize";
        c->down.w = W.upload(pack_conv_padded(W.at(p + ".weight"), c->cp[3], c->cp[3])); c->down.b = W.upload(pad_vector(T(p + ".bias"), c->cp[3]));
        ok = c->down.w && c->down.b;
    }
    auto conv = [&](const std::string& p, int co, int ci, DConv& d) {
        d.w = W.upload(pack_conv_padded(W.at(p + ".weight"), co, ci)); d.b = W.upload(T(p + ".bias"));
        return d.w && d.b;
    };
    for (int i = 0; i < 4 && ok; ++i) {
        const std::string p = "neck.fusion_stage.layers." + std::to_string(i);
        Fusion& f = c->fus[i];
        ok = conv(p + ".projection", F, F, f.proj) && conv(p + ".residual_layer2.convolution1", F, F, f.r2c1) && conv(p + ".residual_layer2.convolution2", F, F, f.r2c2);
        if (ok && i) ok = conv(p + ".residual_layer1.convolution1", F, F, f.r1c1) && conv(p + ".residual_layer1.convolution2", F, F, f.r1c2);
    }
    if (ok) ok = conv("head.conv1", F / 2, F, c->head1) && conv("head.conv2", c->HH, F / 2, c->head2) && conv("head.conv3", 1, c->HH, c->head3);
    return ok;
}

}  // namespace

extern "C" {

int cs_depth_create(const CsDepthConfig* cfg, CsDepth** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    const int mlp = cfg->mlp_ratio < 1 ? 0 : cfg->hidden_size * cfg->mlp_ratio;
    int rc = image_tower::check_encoder_config(NAMES.who, "hidden / MLP size", 0, cfg->hidden_size, mlp, cfg->num_attention_heads, cfg->num_hidden_layers, cfg->patch_size,
                                               cfg->image_size);
    if (rc != CS_OK) return rc;
    if (cfg->size != cfg->image_size) CS_FAIL(CS_E_UNSUPPORTED, "depth: the processor's size %d must equal image_size %d (the position table is not interpolated)",
                                              cfg->size, cfg->image_size);
    if (cfg->size > 2048) CS_FAIL(CS_E_SHAPE, "depth: size %d is larger than 2048", cfg->size);
    if ((rc = image_tower::check_image_std(NAMES.who, cfg->image_std)) != CS_OK) return rc;
    for (int i = 0; i < 4; ++i) {
        if (cfg->out_indices[i] < 1 || cfg->out_indices[i] > cfg->num_hidden_layers || (i && cfg->out_indices[i] <= cfg->out_indices[i - 1]))
            CS_FAIL(CS_E_ARG, "depth: out_indices must increase within 1 .. num_hidden_layers");
        if (cfg->neck_hidden_sizes[i] < 1 || cfg->neck_hidden_sizes[i] > 4096) CS_FAIL(CS_E_ARG, "depth: bad neck_hidden_sizes");
    }
    if (cfg->fusion_hidden_size != 64) CS_FAIL(CS_E_UNSUPPORTED, "depth: fusion_hidden_size %d (built for 64)", cfg->fusion_hidden_size);
    if (cfg->head_hidden_size != 32 && cfg->head_hidden_size != 64) CS_FAIL(CS_E_UNSUPPORTED, "depth: head_hidden_size %d (built for 32 and 64)", cfg->head_hidden_size);
    CsDepth* c = new CsDepth();
    c->cfg = *cfg;
    c->tower.init(cfg->hidden_size, mlp, cfg->num_attention_heads, cfg->layer_norm_eps, cfg->patch_size, cfg->size, cfg->size, cfg->image_mean, cfg->image_std,
                  cfg->rescale_factor);
    c->S = cfg->size; c->F = cfg->fusion_hidden_size; c->HH = cfg->head_hidden_size;
    const int G = c->tower.G;
    c->g[0] = 4 * G; c->g[1] = 2 * G; c->g[2] = G; c->g[3] = (G - 1) / 2 + 1;
    for (int i = 0; i < 4; ++i) c->cp[i] = padded_channels(cfg->neck_hidden_sizes[i], RK[i], i == 3);
    build_manifest(c);
    *out = c;
    return CS_OK;
}

void cs_depth_destroy(CsDepth* c) {
    if (!c) return;
    for (auto& kv : c->pos_tables) (void)hipFree(kv.second);
    c->tower.free_device();
    delete c;
}

int cs_depth_num_weights(const CsDepth* c) { return c ? c->tower.weights.count() : 0; }

const char* cs_depth_weight_name(const CsDepth* c, int i, int64_t* shape4, int* ndim) { return c ? c->tower.weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_depth_set_weight(CsDepth* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    return image_tower::set_weight(tower_of(c), name, data, shape, ndim);
}

int cs_depth_finalize(CsDepth* c) { return image_tower::finalize(NAMES, tower_of(c), [&] { return pack(c); }); }

int cs_depth_patch_cols(const CsDepth* c) { return c ? c->tower.Kpad : 0; }
int cs_depth_num_tokens(const CsDepth* c) { return c ? c->tower.T : 0; }

size_t cs_depth_workspace_bytes(const CsDepth* c, int batch) {
    if (!c || batch <= 0) return 0;
    return depth_model::workspace_bytes(c, depth_model::make_grid(c, c->S, c->S), batch);
}

double cs_depth_flops(const CsDepth* c, int batch) { return c ? depth_model::flops(c, depth_model::make_grid(c, c->S, c->S), batch) : 0; }

size_t cs_depth_preprocess_workspace_bytes(const CsDepth* c, int batch, int height, int width) {
    return image_tower::preprocess_workspace_bytes(tower_of(c), batch, height, width);
}

int cs_depth_preprocess(CsDepth* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (c && batch >= 0 && height != width)          // (behind the null-handle and negative-size refusals, in front of the empty batch's return)
        CS_FAIL(CS_E_UNSUPPORTED, "depth: %d x %d image: this entry point takes square inputs only (they resize to %d x %d); cs_depth_preprocess_hw takes any aspect ratio", height, width, c->S,
                c->S);
    return image_tower::preprocess(NAMES, tower_of(c), images, dtype, batch, height, width, patches, crop_u8, workspace, workspace_bytes, stream);
}

int cs_depth_forward(CsDepth* c, const void* patches, int batch, float* predicted_depth, void* workspace, size_t workspace_bytes, void* stream) {
    bool run = false;
    int rc = image_tower::begin_forward(NAMES, tower_of(c), batch, patches && predicted_depth && workspace, workspace_bytes, cs_depth_workspace_bytes(c, batch), &run);
    if (!run) return rc;
    const depth_model::DepthGrid g = depth_model::make_grid(c, c->S, c->S);
    if (depth_model::too_large(c, g, batch)) CS_FAIL(CS_E_SHAPE, "depth: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const int G = c->tower.G;
    return depth_model::forward(c, g, c->tower.pos, patches, batch, predicted_depth, workspace, s,
                                [&](const f16* y, int k, int C, f16* out) { return launch_dpt_pixel_shuffle(y, batch, G, k, C, 1, out, s); });
}

int cs_depth_normalized_maps(CsDepth* c, const float* predicted_depth, int batch, int height, int width, float* maps, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "depth handle is NULL");
    if (batch < 0 || height < 1 || width < 1) CS_FAIL(CS_E_ARG, "depth: bad size");
    if (batch == 0) return CS_OK;
    if (!predicted_depth || !maps) CS_FAIL(CS_E_ARG, "null pointer");
    int rc = launch_dpt_bicubic(predicted_depth, batch, c->S, c->S, height, width, maps, (hipStream_t)stream);
    if (rc == CS_OK) rc = launch_dpt_minmax_normalize(maps, batch, (long)height * width, (hipStream_t)stream);
    return rc;
}

int cs_op_dpt_conv(const void* x, int B, int H, int W, int Cin, const void* w, const void* bias, int Cout, int taps, int relu_in, int relu_out,
                   const void* res, const void* res2, void* out, void* stream) {
    DptConvArgs a{};
    a.x = (const f16*)x; a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.w = (const f16*)w; a.bias = (const f16*)bias; a.Cout = Cout; a.taps = taps;
    a.relu_in = relu_in; a.relu_out = relu_out; a.res = (const f16*)res; a.res2 = (const f16*)res2; a.out = (f16*)out;
    return launch_dpt_conv(a, (hipStream_t)stream);
}
int cs_op_dpt_bilinear(const void* x, int B, int Hi, int Wi, int C, int Ho, int Wo, void* out, void* stream) {
    return launch_dpt_bilinear((const f16*)x, B, Hi, Wi, C, Ho, Wo, (f16*)out, (hipStream_t)stream);
}
int cs_op_dpt_pixel_shuffle(const void* y, int B, int G, int k, int C, int skip, void* out, void* stream) {
    return launch_dpt_pixel_shuffle((const f16*)y, B, G, k, C, skip, (f16*)out, (hipStream_t)stream);
}
int cs_op_dpt_head(const void* x, int64_t M, int C, const void* w, const void* bias, float scale, float* out, void* stream) {
    return launch_dpt_head((const f16*)x, (long)M, C, (const f16*)w, (const f16*)bias, scale, out, (hipStream_t)stream);
}
int cs_op_dpt_bicubic(const float* x, int B, int Hi, int Wi, int Ho, int Wo, float* out, void* stream) {
    return launch_dpt_bicubic(x, B, Hi, Wi, Ho, Wo, out, (hipStream_t)stream);
}
int cs_op_dpt_minmax_normalize(float* x, int B, int64_t n, void* stream) { return launch_dpt_minmax_normalize(x, B, (long)n, (hipStream_t)stream); }

}  // extern "C"
