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
#include "encoder.h"
#include "image_front_end.h"
#include "consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

#include <cmath>

namespace {
struct DConv { f16* w = nullptr; f16* b = nullptr; };
struct Fusion { DConv proj, r1c1, r1c2, r2c1, r2c2; };
constexpr int RK[4] = {4, 2, 1, 1};      // reassemble_factors 4, 2, 1, 0.5: the first two are transposed convs with kernel = stride, the last a stride-2 3x3 conv
}  // namespace

struct CsDepth {
    CsDepthConfig cfg;
    int G = 0, NP = 0, T = 0, K = 0, Kpad = 0, I = 0, S = 0, F = 0, HH = 0;   // patch grid, patches, tokens, patch-row length (and padded), MLP width, image size, fusion / head widths
    int g[4] = {0, 0, 0, 0};               // sizes of the four reassembled maps: 4 G, 2 G, G, (G - 1) / 2 + 1
    int cp[4] = {0, 0, 0, 0};              // their channel counts as stored (neck_hidden_sizes padded)
    WeightStore<float> weights;            // fp32 staging: every fold is formed in fp32 and rounded once at upload
    f16 *wpatch = nullptr, *bpatch = nullptr, *cls = nullptr, *pos = nullptr, *lnfg = nullptr, *lnfb = nullptr;
    std::vector<PreLnLayer> layers;
    DConv reasm[4];                        // projection (folded with the transposed conv): [k k cp][D]
    DConv down;                            // reassemble layer 3's stride-2 3x3 conv [cp3][9][cp3]
    DConv neck[4];                         // neck.convs [F][9][cp]
    Fusion fus[4];
    DConv head1, head2, head3;
    image_front_end::PlanCache plans;
};

namespace {

// stored channel count of reassembled map i: a multiple of 32 (the narrow conv's k step) whose GEMM width k k cp fits launch_igemm; map 3 is also the
// stride-2 conv's input and output (Cin % 64, N % 128 or N % 160)
int padded_channels(int C, int k, bool conv_operand) {
    for (int cp = (C + 31) / 32 * 32;; cp += 32) {
        const int n = k * k * cp;
        if ((n % 128 == 0 || n % 160 == 0) && (!conv_operand || cp % 64 == 0)) return cp;
    }
}

void build_manifest(CsDepth* c) {          // transformers DepthAnythingForDepthEstimation.state_dict() order
    WeightManifest& m = c->weights;
    const int D = c->cfg.hidden_size, I = c->I, P = c->cfg.patch_size, g = c->cfg.image_size / P, F = c->F;
    const std::string bb = "backbone.";
    m.expect(bb + "embeddings.cls_token", {1, 1, D});
    m.expect(bb + "embeddings.mask_token", {1, D});
    m.expect(bb + "embeddings.position_embeddings", {1, (int64_t)g * g + 1, D});
    m.expect(bb + "embeddings.patch_embeddings.projection.weight", {D, 3, P, P});
    m.expect(bb + "embeddings.patch_embeddings.projection.bias", {D});
    for (int l = 0; l < c->cfg.num_hidden_layers; ++l) {
        const std::string p = bb + "encoder.layer." + std::to_string(l);
        m.expect(p + ".norm1.weight", {D}); m.expect(p + ".norm1.bias", {D});
        for (const char* q : {".attention.attention.query", ".attention.attention.key", ".attention.attention.value", ".attention.output.dense"}) {
            m.expect(p + q + ".weight", {D, D}); m.expect(p + q + ".bias", {D});
        }
        m.expect(p + ".layer_scale1.lambda1", {D});
        m.expect(p + ".norm2.weight", {D}); m.expect(p + ".norm2.bias", {D});
        m.expect(p + ".mlp.fc1.weight", {I, D}); m.expect(p + ".mlp.fc1.bias", {I});
        m.expect(p + ".mlp.fc2.weight", {D, I}); m.expect(p + ".mlp.fc2.bias", {D});
        m.expect(p + ".layer_scale2.lambda1", {D});
    }
    m.expect(bb + "layernorm.weight", {D}); m.expect(bb + "layernorm.bias", {D});
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

// workspace carve-up (fp16 elements): the encoder stack | patch embeddings | normalised tap | reassemble GEMM output | reassembled map | map 3 after its
// stride-2 conv | the four neck features | three rotating buffers for the fusion stage and the head
struct Layout { size_t pe, tap, gemm, map, down, f[4], x, y, z, total; };
Layout layout(const CsDepth* c, size_t B) {
    const size_t D = c->cfg.hidden_size, rows = B * c->T, F = c->F;
    Layout L;
    size_t o = pre_ln_workspace_elems(rows, D, c->I);
    L.pe = o; o += B * c->NP * D;
    L.tap = o; o += rows * D;
    size_t nmax = 0, mmax = 0;
    for (int i = 0; i < 4; ++i) {
        nmax = std::max(nmax, (size_t)RK[i] * RK[i] * c->cp[i]);
        mmax = std::max(mmax, (size_t)c->G * RK[i] * c->G * RK[i] * c->cp[i]);
    }
    L.gemm = o; o += rows * nmax;
    L.map = o; o += B * mmax;
    L.down = o; o += B * c->g[3] * c->g[3] * c->cp[3];
    for (int i = 0; i < 4; ++i) { L.f[i] = o; o += B * c->g[i] * c->g[i] * F; }
    const size_t up = (size_t)2 * c->g[0], big = std::max(up * up * F, (size_t)c->S * c->S * std::max(F / 2, (size_t)c->HH));
    L.x = o; o += B * big; L.y = o; o += B * big; L.z = o; o += B * big;
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

int cs_depth_create(const CsDepthConfig* cfg, CsDepth** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    if (cfg->hidden_size < 128 || cfg->hidden_size % 128 || cfg->mlp_ratio < 1 || (cfg->hidden_size * cfg->mlp_ratio) % 128)
        CS_FAIL(CS_E_SHAPE, "depth: hidden / MLP size must be multiples of 128");
    if (cfg->num_attention_heads < 1 || cfg->hidden_size != cfg->num_attention_heads * 64) CS_FAIL(CS_E_UNSUPPORTED, "depth: built for heads of dim 64");
    if (cfg->num_hidden_layers < 1 || cfg->patch_size < 1 || cfg->image_size < cfg->patch_size || cfg->image_size % cfg->patch_size) CS_FAIL(CS_E_ARG, "depth: bad config");
    if (cfg->size != cfg->image_size) CS_FAIL(CS_E_UNSUPPORTED, "depth: the processor's size %d must equal image_size %d (the position table is not interpolated)",
                                              cfg->size, cfg->image_size);
    if (cfg->size > 2048) CS_FAIL(CS_E_SHAPE, "depth: size %d is larger than 2048", cfg->size);
    for (int i = 0; i < 4; ++i) {
        if (cfg->out_indices[i] < 1 || cfg->out_indices[i] > cfg->num_hidden_layers || (i && cfg->out_indices[i] <= cfg->out_indices[i - 1]))
            CS_FAIL(CS_E_ARG, "depth: out_indices must increase within 1 .. num_hidden_layers");
        if (cfg->neck_hidden_sizes[i] < 1 || cfg->neck_hidden_sizes[i] > 4096) CS_FAIL(CS_E_ARG, "depth: bad neck_hidden_sizes");
        if (!(cfg->image_std[i % 3] > 0.f)) CS_FAIL(CS_E_ARG, "depth: image_std must be positive");
    }
    if (cfg->fusion_hidden_size != 64) CS_FAIL(CS_E_UNSUPPORTED, "depth: fusion_hidden_size %d (built for 64)", cfg->fusion_hidden_size);
    if (cfg->head_hidden_size != 32 && cfg->head_hidden_size != 64) CS_FAIL(CS_E_UNSUPPORTED, "depth: head_hidden_size %d (built for 32 and 64)", cfg->head_hidden_size);
    CsDepth* c = new CsDepth();
    c->cfg = *cfg;
    c->S = cfg->size; c->G = cfg->size / cfg->patch_size; c->NP = c->G * c->G; c->T = c->NP + 1;
    c->K = 3 * cfg->patch_size * cfg->patch_size; c->Kpad = (c->K + 63) / 64 * 64; c->I = cfg->hidden_size * cfg->mlp_ratio;
    c->F = cfg->fusion_hidden_size; c->HH = cfg->head_hidden_size;
    c->g[0] = 4 * c->G; c->g[1] = 2 * c->G; c->g[2] = c->G; c->g[3] = (c->G - 1) / 2 + 1;
    for (int i = 0; i < 4; ++i) c->cp[i] = padded_channels(cfg->neck_hidden_sizes[i], RK[i], i == 3);
    build_manifest(c);
    *out = c;
    return CS_OK;
}

void cs_depth_destroy(CsDepth* c) {
    if (!c) return;
    c->weights.free_device();
    c->plans.free_device();
    delete c;
}

int cs_depth_num_weights(const CsDepth* c) { return c ? c->weights.count() : 0; }

const char* cs_depth_weight_name(const CsDepth* c, int i, int64_t* shape4, int* ndim) { return c ? c->weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_depth_set_weight(CsDepth* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!c) CS_FAIL(CS_E_ARG, "null argument");
    return c->weights.set(name, data, shape, ndim);
}

int cs_depth_finalize(CsDepth* c) {
    if (!c) CS_FAIL(CS_E_ARG, "null");
    WeightStore<float>& W = c->weights;
    if (W.finalized) return CS_OK;
    if (const std::string* n = W.first_missing()) CS_FAIL(CS_E_STATE, "missing weight '%s'", n->c_str());
    const std::string bb = "backbone.";
    auto T = [&](const std::string& n) -> const std::vector<float>& { return W.at(n).data; };
    const int D = c->cfg.hidden_size, K = c->K, Kpad = c->Kpad, F = c->F;
    {   // patch projection [D][3 P P] -> [D][Kpad]
        const auto& w = T(bb + "embeddings.patch_embeddings.projection.weight");
        std::vector<float> wp((size_t)D * Kpad, 0.f);
        for (int n = 0; n < D; ++n) std::copy(w.begin() + (size_t)n * K, w.begin() + (size_t)(n + 1) * K, wp.begin() + (size_t)n * Kpad);
        c->wpatch = W.upload(wp); c->bpatch = W.upload(T(bb + "embeddings.patch_embeddings.projection.bias"));
    }
    {   // the position table as it is (the grid is the training grid); the class row pre-added to the CLS token in fp32
        const auto& pos = T(bb + "embeddings.position_embeddings");
        const auto& cls = T(bb + "embeddings.cls_token");
        std::vector<float> cls0(D), table((size_t)c->T * D, 0.f);
        for (int d = 0; d < D; ++d) cls0[d] = cls[d] + pos[d];
        std::copy(pos.begin() + D, pos.end(), table.begin() + D);
        c->cls = W.upload(cls0); c->pos = W.upload(table);
    }
    c->lnfg = W.upload(T(bb + "layernorm.weight")); c->lnfb = W.upload(T(bb + "layernorm.bias"));
    bool ok = c->wpatch && c->bpatch && c->cls && c->pos && c->lnfg && c->lnfb;
    c->layers.resize(c->cfg.out_indices[3]);                    // the layers behind the last tap feed nothing
    for (size_t l = 0; l < c->layers.size() && ok; ++l) {
        const std::string p = bb + "encoder.layer." + std::to_string(l);
        ok = pack_pre_ln_layer<float>(W, {p + ".attention.attention.query", p + ".attention.attention.key", p + ".attention.attention.value", p + ".attention.output.dense",
                                          p + ".norm1", p + ".norm2", p + ".mlp.fc1", p + ".mlp.fc2"},
                                      &W.at(p + ".layer_scale1.lambda1").data, &W.at(p + ".layer_scale2.lambda1").data, c->layers[l]);
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
    if (!ok) CS_FAIL(CS_E_HIP, "depth: weight upload failed (hipMalloc/hipMemcpy)");
    W.release_host();
    W.finalized = true;
    return CS_OK;
}

int cs_depth_patch_cols(const CsDepth* c) { return c ? c->Kpad : 0; }
int cs_depth_num_tokens(const CsDepth* c) { return c ? c->T : 0; }

size_t cs_depth_workspace_bytes(const CsDepth* c, int batch) {
    if (!c || batch <= 0) return 0;
    return layout(c, (size_t)batch).total * sizeof(f16) + 4096;
}

double cs_depth_flops(const CsDepth* c, int batch) {
    if (!c) return 0;
    const double D = c->cfg.hidden_size, F = c->F, B = batch;
    double f = 2.0 * B * c->NP * (double)c->K * D + pre_ln_flops(c->cfg.out_indices[3], batch, c->T, D, c->I);
    for (int i = 0; i < 4; ++i) {
        const double px = (double)c->g[i] * c->g[i];
        f += 2.0 * B * c->T * D * RK[i] * RK[i] * c->cp[i];                                   // reassemble GEMM
        f += 2.0 * B * px * 9 * c->cp[i] * F;                                                 // neck conv
        const int lvl = 3 - i;                                                                // fusion layer `lvl` runs at this map's size
        const double nxt = i ? (double)c->g[i - 1] * c->g[i - 1] : 4.0 * px;
        f += (lvl ? 4 : 2) * 2.0 * B * px * 9 * F * F + 2.0 * B * nxt * F * F;
    }
    f += 2.0 * B * c->g[3] * c->g[3] * 9.0 * c->cp[3] * c->cp[3];                             // the stride-2 conv
    f += 2.0 * B * 4.0 * c->g[0] * c->g[0] * 9 * F * (F / 2) + 2.0 * B * c->S * (double)c->S * (9.0 * (F / 2) * c->HH + c->HH);
    return f;
}

size_t cs_depth_preprocess_workspace_bytes(const CsDepth* c, int batch, int height, int width) {
    if (!c || batch <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)batch * 3 * height * c->S + 256;          // the horizontal pass's rows (at most every input row) x size columns, uint8
}

int cs_depth_preprocess(CsDepth* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "depth handle is NULL");
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (height != width) CS_FAIL(CS_E_UNSUPPORTED, "depth: %d x %d image: only square inputs are built (the processor's keep_aspect_ratio rule then gives %d x %d)",
                                 height, width, c->S, c->S);
    if (batch == 0) return CS_OK;
    if (!images || !patches || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    const image_front_end::Plan* pl = nullptr;
    const int rc = c->plans.get_plan("depth", c->S, c->S, height, width, &pl);          // shortest edge = crop = size: the whole image, no crop
    if (rc != CS_OK) return rc;
    if (workspace_bytes < (size_t)batch * 3 * pl->dev.nrows * c->S) CS_FAIL(CS_E_ARG, "depth: preprocess workspace too small");
    return launch_vit_front_end(images, dtype, batch, height, width, pl->dev, c->cfg.image_mean, c->cfg.image_std, c->cfg.rescale_factor,
                                c->cfg.patch_size, c->G, c->Kpad, (unsigned char*)workspace, (f16*)patches, crop_u8, (hipStream_t)stream);
}

int cs_depth_forward(CsDepth* c, const void* patches, int batch, float* predicted_depth, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "depth handle is NULL");
    if (!c->weights.finalized) CS_FAIL(CS_E_STATE, "cs_depth_finalize has not been called");
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!patches || !predicted_depth || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    if (workspace_bytes < cs_depth_workspace_bytes(c, batch)) CS_FAIL(CS_E_ARG, "depth: workspace too small");
    const int D = c->cfg.hidden_size, I = c->I, H = c->cfg.num_attention_heads, Tn = c->T, F = c->F, B = batch, G = c->G;
    const Layout L = layout(c, (size_t)B);
    if ((long)B * Tn > 0x7fffffffL / std::max(std::max(I, 3 * D), 16 * c->cp[0]) || (long)B * c->S * c->S > 0x7fffffffL / 64)
        CS_FAIL(CS_E_SHAPE, "depth: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const long rows = (long)B * Tn;
    const PreLnWorkspace w = carve_pre_ln(workspace, rows, D, I);
    f16* base = (f16*)workspace;
    f16 *pe = base + L.pe, *tap = base + L.tap, *gemm = base + L.gemm, *map = base + L.map, *down = base + L.down;
    f16* f[4] = {base + L.f[0], base + L.f[1], base + L.f[2], base + L.f[3]};
    f16 *X = base + L.x, *Y = base + L.y, *Z = base + L.z;
    auto conv = [&](const f16* x, int size, int cin, const DConv& cv, int cout, int taps, int relu_in, int relu_out, const f16* res, const f16* res2, f16* out) {
        DptConvArgs a{};
        a.x = x; a.B = B; a.H = size; a.W = size; a.Cin = cin; a.w = cv.w; a.bias = cv.b; a.Cout = cout; a.taps = taps;
        a.relu_in = relu_in; a.relu_out = relu_out; a.res = res; a.res2 = res2; a.out = out;
        return launch_dpt_conv(a, s);
    };
    // pre-activation residual unit: out = conv2(relu(conv1(relu(x)))) + x (+ skip); tmp holds the inner activation
    auto rcu = [&](const f16* x, int size, const DConv& c1, const DConv& c2, const f16* skip, f16* tmp, f16* out) {
        const int rc = conv(x, size, F, c1, F, 9, 1, 0, nullptr, nullptr, tmp);
        return rc != CS_OK ? rc : conv(tmp, size, F, c2, F, 9, 1, 0, x, skip, out);
    };

    // ---- backbone, tapped after out_indices[i] layers: final LayerNorm -> reassemble layer i -> neck conv i ----
    int rc = linear((const f16*)patches, B * c->NP, c->Kpad, c->wpatch, c->bpatch, D, nullptr, pe, s);
    if (rc == CS_OK) rc = launch_vit_tokens(pe, c->cls, c->pos, w.x, B, c->NP, D, s);
    size_t done = 0;
    for (int i = 0; i < 4 && rc == CS_OK; ++i) {
        const int k = RK[i], cp = c->cp[i];
        rc = run_pre_ln_layers(c->layers, w, B, Tn, D, I, H, c->cfg.layer_norm_eps, 0, launch_gelu_erf, s, done, (size_t)c->cfg.out_indices[i]);
        done = (size_t)c->cfg.out_indices[i];
        if (rc == CS_OK) rc = launch_layer_norm(w.x, c->lnfg, c->lnfb, tap, (int)rows, D, c->cfg.layer_norm_eps, s);
        if (rc == CS_OK) rc = linear(tap, (int)rows, D, c->reasm[i].w, c->reasm[i].b, k * k * cp, nullptr, gemm, s);
        if (rc == CS_OK) rc = launch_dpt_pixel_shuffle(gemm, B, G, k, cp, 1, map, s);               // drops the CLS rows
        const f16* src = map;
        if (i == 3 && rc == CS_OK) {
            IgemmArgs a{};
            a.a0 = map; a.c0 = cp; a.B = B; a.Hi = G; a.Wi = G; a.Ho = c->g[3]; a.Wo = c->g[3]; a.taps = 9; a.stride = 2; a.N = cp;
            a.w = c->down.w; a.bias = c->down.b; a.out = down;
            rc = launch_igemm(a, s);
            src = down;
        }
        if (rc == CS_OK) rc = conv(src, c->g[i], cp, c->neck[i], F, 9, 0, 0, nullptr, nullptr, f[i]);
    }
    // ---- fusion stage, coarse to fine: X holds the fused state ----
    for (int l = 0; l < 4 && rc == CS_OK; ++l) {
        const int i = 3 - l, size = c->g[i], next = i ? c->g[i - 1] : 2 * size;
        const Fusion& fu = c->fus[l];
        const f16* h = f[i];
        if (l) { rc = rcu(f[i], size, fu.r1c1, fu.r1c2, X, Y, Z); h = Z; }                         // Z = fused + residual_layer1(feature)
        if (rc == CS_OK) rc = rcu(h, size, fu.r2c1, fu.r2c2, nullptr, Y, X);                        // X = residual_layer2(h)
        if (rc == CS_OK) rc = launch_dpt_bilinear(X, B, size, size, F, next, next, Y, s);
        if (rc == CS_OK) rc = conv(Y, next, F, fu.proj, F, 1, 0, 0, nullptr, nullptr, X);
    }
    // ---- head ----
    const int up = 2 * c->g[0];
    if (rc == CS_OK) rc = conv(X, up, F, c->head1, F / 2, 9, 0, 0, nullptr, nullptr, Y);
    if (rc == CS_OK) rc = launch_dpt_bilinear(Y, B, up, up, F / 2, c->S, c->S, Z, s);
    if (rc == CS_OK) rc = conv(Z, c->S, F / 2, c->head2, c->HH, 9, 0, 1, nullptr, nullptr, Y);
    if (rc == CS_OK) rc = launch_dpt_head(Y, (long)B * c->S * c->S, c->HH, c->head3.w, c->head3.b, c->cfg.max_depth, predicted_depth, s);
    return rc;
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
