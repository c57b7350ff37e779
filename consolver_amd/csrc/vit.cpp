// DINOv2 image encoder + the image-similarity reward around it (reward_type "dino": edit_ppo/reward_model.py:59-64, 217-257; run_ppo.sh:30).
//
// Replaces, for a batch of decoded images [B,3,H,W] in [0,1]:  ToPILImage -> the facebook/dinov2-base processor (PIL bicubic resize to shortest edge 256, center
// crop 224, rescale, normalise) -> transformers Dinov2Model (14 x 14 patch conv, CLS token, position table bicubically interpolated from its 37 x 37 training grid,
// 12 pre-LN layers with LayerScale and exact GELU, final LayerNorm) -> CLS row -> F.normalize / cosine_similarity -> (cos + 1) * 50.
// The encoder is encoder.h's layer loop (implicit-GEMM MFMA linears, flash attention at head dim 64 -- here unmasked, 257 tokens) with the LayerScale vectors folded
// into the out-projection / fc2 weights and biases at pack time (fp32 product, one rounding to fp16); the front end and the tail are vit_ops.hip.
#include "encoder.h"
#include "image_front_end.h"
#include "consolver_hip.h"

#include <cmath>

struct CsVit {
    CsVitConfig cfg;
    int G = 0, NP = 0, T = 0, K = 0, Kpad = 0, I = 0;      // patch grid of the crop, patches, tokens, patch-row length (and padded), MLP width
    WeightStore<float> weights;                            // fp32 staging: the LayerScale product is formed in fp32 and rounded once at upload
    f16 *wpatch = nullptr, *bpatch = nullptr, *cls = nullptr, *pos = nullptr, *lnfg = nullptr, *lnfb = nullptr;
    std::vector<PreLnLayer> layers;
    image_front_end::PlanCache plans;                      // resize tables per input (height, width), bounded (image_front_end.h)
};

namespace {

void build_manifest(CsVit* c) {          // transformers Dinov2Model.state_dict() order
    WeightManifest& m = c->weights;
    const int D = c->cfg.hidden_size, I = c->I, P = c->cfg.patch_size, g = c->cfg.image_size / P;
    m.expect("embeddings.cls_token", {1, 1, D});
    m.expect("embeddings.mask_token", {1, D});                                   // in the published count; pre-training only, unused by the forward
    m.expect("embeddings.position_embeddings", {1, (int64_t)g * g + 1, D});
    m.expect("embeddings.patch_embeddings.projection.weight", {D, 3, P, P});
    m.expect("embeddings.patch_embeddings.projection.bias", {D});
    for (int l = 0; l < c->cfg.num_hidden_layers; ++l) {
        const std::string p = "encoder.layer." + std::to_string(l);
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
    m.expect("layernorm.weight", {D}); m.expect("layernorm.bias", {D});
}

// torch F.interpolate(mode="bicubic", align_corners=False) of the [s][s][D] position grid to [g][g][D] (cubic convolution, A = -0.75, clamped reads)
void cubic_taps(double t, double* k) {
    const double A = -0.75;
    auto c1 = [&](double x) { return ((A + 2) * x - (A + 3)) * x * x + 1; };
    auto c2 = [&](double x) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; };
    k[0] = c2(t + 1); k[1] = c1(t); k[2] = c1(1 - t); k[3] = c2(2 - t);
}
std::vector<float> interpolate_positions(const float* grid, int s, int g, int D) {
    std::vector<float> out((size_t)g * g * D);
    const double scale = (double)s / g;
    for (int oy = 0; oy < g; ++oy) {
        const double sy = scale * (oy + 0.5) - 0.5; const int iy = (int)std::floor(sy); double ky[4]; cubic_taps(sy - iy, ky);
        for (int ox = 0; ox < g; ++ox) {
            const double sx = scale * (ox + 0.5) - 0.5; const int ix = (int)std::floor(sx); double kx[4]; cubic_taps(sx - ix, kx);
            for (int d = 0; d < D; ++d) {
                double acc = 0;
                for (int a = 0; a < 4; ++a) {
                    const int y = std::min(std::max(iy - 1 + a, 0), s - 1);
                    double r = 0;
                    for (int b = 0; b < 4; ++b) r += kx[b] * grid[((size_t)y * s + std::min(std::max(ix - 1 + b, 0), s - 1)) * D + d];
                    acc += ky[a] * r;
                }
                out[((size_t)oy * g + ox) * D + d] = (float)acc;
            }
        }
    }
    return out;
}

}  // namespace

extern "C" {

int cs_vit_create(const CsVitConfig* cfg, CsVit** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    if (cfg->hidden_size < 128 || cfg->hidden_size % 128 || cfg->mlp_ratio < 1 || (cfg->hidden_size * cfg->mlp_ratio) % 128)
        CS_FAIL(CS_E_SHAPE, "vit: hidden / MLP size must be multiples of 128");
    if (cfg->num_attention_heads < 1 || cfg->hidden_size != cfg->num_attention_heads * 64) CS_FAIL(CS_E_UNSUPPORTED, "vit: built for heads of dim 64");
    if (cfg->num_hidden_layers < 1 || cfg->patch_size < 1 || cfg->image_size < cfg->patch_size || cfg->image_size % cfg->patch_size) CS_FAIL(CS_E_ARG, "vit: bad config");
    if (cfg->crop_size < cfg->patch_size || cfg->crop_size % cfg->patch_size || cfg->resize_shortest_edge < cfg->crop_size)
        CS_FAIL(CS_E_ARG, "vit: crop_size must be a multiple of patch_size and at most resize_shortest_edge");
    for (int i = 0; i < 3; ++i) if (!(cfg->image_std[i] > 0.f)) CS_FAIL(CS_E_ARG, "vit: image_std must be positive");
    CsVit* c = new CsVit();
    c->cfg = *cfg;
    c->G = cfg->crop_size / cfg->patch_size; c->NP = c->G * c->G; c->T = c->NP + 1;
    c->K = 3 * cfg->patch_size * cfg->patch_size; c->Kpad = (c->K + 63) / 64 * 64; c->I = cfg->hidden_size * cfg->mlp_ratio;
    build_manifest(c);
    *out = c;
    return CS_OK;
}

void cs_vit_destroy(CsVit* c) {
    if (!c) return;
    c->weights.free_device();
    c->plans.free_device();
    delete c;
}

int cs_vit_num_weights(const CsVit* c) { return c ? c->weights.count() : 0; }

const char* cs_vit_weight_name(const CsVit* c, int i, int64_t* shape4, int* ndim) { return c ? c->weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_vit_set_weight(CsVit* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!c) CS_FAIL(CS_E_ARG, "null argument");
    return c->weights.set(name, data, shape, ndim);
}

int cs_vit_finalize(CsVit* c) {
    if (!c) CS_FAIL(CS_E_ARG, "null");
    WeightStore<float>& W = c->weights;
    if (W.finalized) return CS_OK;
    if (const std::string* n = W.first_missing()) CS_FAIL(CS_E_STATE, "missing weight '%s'", n->c_str());
    auto T = [&](const char* n) -> const std::vector<float>& { return W.at(n).data; };
    const int D = c->cfg.hidden_size, K = c->K, Kpad = c->Kpad, s = c->cfg.image_size / c->cfg.patch_size, G = c->G;
    {   // patch projection [D][3 P P] -> [D][Kpad]
        const auto& w = T("embeddings.patch_embeddings.projection.weight");
        std::vector<float> wp((size_t)D * Kpad, 0.f);
        for (int n = 0; n < D; ++n) std::copy(w.begin() + (size_t)n * K, w.begin() + (size_t)(n + 1) * K, wp.begin() + (size_t)n * Kpad);
        c->wpatch = W.upload(wp); c->bpatch = W.upload(T("embeddings.patch_embeddings.projection.bias"));
    }
    {   // position table of the crop's grid: the class row as is (pre-added to the CLS token in fp32), the patch grid interpolated when the crop is not the training size
        const auto& pos = T("embeddings.position_embeddings");
        const auto& cls = T("embeddings.cls_token");
        std::vector<float> cls0(D), table((size_t)c->T * D, 0.f);
        for (int d = 0; d < D; ++d) cls0[d] = cls[d] + pos[d];
        if (G == s) std::copy(pos.begin() + D, pos.end(), table.begin() + D);
        else { const auto g = interpolate_positions(pos.data() + D, s, G, D); std::copy(g.begin(), g.end(), table.begin() + D); }
        c->cls = W.upload(cls0); c->pos = W.upload(table);
    }
    c->lnfg = W.upload(T("layernorm.weight")); c->lnfb = W.upload(T("layernorm.bias"));
    bool ok = c->wpatch && c->bpatch && c->cls && c->pos && c->lnfg && c->lnfb;
    c->layers.resize(c->cfg.num_hidden_layers);
    for (int l = 0; l < c->cfg.num_hidden_layers && ok; ++l) {
        const std::string p = "encoder.layer." + std::to_string(l);
        ok = pack_pre_ln_layer<float>(W, {p + ".attention.attention.query", p + ".attention.attention.key", p + ".attention.attention.value", p + ".attention.output.dense",
                                          p + ".norm1", p + ".norm2", p + ".mlp.fc1", p + ".mlp.fc2"},
                                      &W.at(p + ".layer_scale1.lambda1").data, &W.at(p + ".layer_scale2.lambda1").data, c->layers[l]);
    }
    if (!ok) CS_FAIL(CS_E_HIP, "vit: weight upload failed (hipMalloc/hipMemcpy)");
    W.release_host();
    W.finalized = true;
    return CS_OK;
}

int cs_vit_patch_cols(const CsVit* c) { return c ? c->Kpad : 0; }
int cs_vit_num_tokens(const CsVit* c) { return c ? c->T : 0; }

size_t cs_vit_workspace_bytes(const CsVit* c, int batch) {
    if (!c || batch <= 0) return 0;
    const size_t D = c->cfg.hidden_size;
    return (pre_ln_workspace_elems((size_t)batch * c->T, D, c->I) + (size_t)batch * c->NP * D) * sizeof(f16) + 4096;       // the encoder stack's, patch embeddings
}

double cs_vit_flops(const CsVit* c, int batch) {
    if (!c) return 0;
    const double D = c->cfg.hidden_size;
    return 2.0 * batch * c->NP * (double)c->K * D + pre_ln_flops(c->cfg.num_hidden_layers, batch, c->T, D, c->I);
}

size_t cs_vit_preprocess_workspace_bytes(const CsVit* c, int batch, int height, int width) {
    if (!c || batch <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)batch * 3 * height * c->cfg.crop_size + 256;          // the horizontal pass's rows (at most every input row) x crop columns, uint8
}

int cs_vit_preprocess(CsVit* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "vit is NULL");
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!images || !patches || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    const image_front_end::Plan* pl = nullptr;
    const int rc = c->plans.get_plan("vit", c->cfg.resize_shortest_edge, c->cfg.crop_size, height, width, &pl);
    if (rc != CS_OK) return rc;
    if (workspace_bytes < (size_t)batch * 3 * pl->dev.nrows * c->cfg.crop_size) CS_FAIL(CS_E_ARG, "vit: preprocess workspace too small");
    return launch_vit_front_end(images, dtype, batch, height, width, pl->dev, c->cfg.image_mean, c->cfg.image_std, c->cfg.rescale_factor,
                                c->cfg.patch_size, c->G, c->Kpad, (unsigned char*)workspace, (f16*)patches, crop_u8, (hipStream_t)stream);
}

int cs_vit_forward(CsVit* c, const void* patches, int batch, float* cls_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "vit is NULL");
    if (!c->weights.finalized) CS_FAIL(CS_E_STATE, "cs_vit_finalize has not been called");
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!patches || !cls_out || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    if (workspace_bytes < cs_vit_workspace_bytes(c, batch)) CS_FAIL(CS_E_ARG, "vit: workspace too small");
    if ((long)batch * c->T > 0x7fffffffL / std::max(c->I, 3 * c->cfg.hidden_size)) CS_FAIL(CS_E_SHAPE, "vit: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const int D = c->cfg.hidden_size, I = c->I, H = c->cfg.num_attention_heads, Tn = c->T;
    const long rows = (long)batch * Tn;
    const PreLnWorkspace w = carve_pre_ln(workspace, rows, D, I);
    f16* pe = w.end;
    int rc = linear((const f16*)patches, batch * c->NP, c->Kpad, c->wpatch, c->bpatch, D, nullptr, pe, s);
    if (rc == CS_OK) rc = launch_vit_tokens(pe, c->cls, c->pos, w.x, batch, c->NP, D, s);
    if (rc == CS_OK) rc = run_pre_ln_layers(c->layers, w, batch, Tn, D, I, H, c->cfg.layer_norm_eps, 0, launch_gelu_erf, s);
    if (rc == CS_OK) rc = launch_vit_cls_layer_norm(w.x, (long)Tn * D, c->lnfg, c->lnfb, c->cfg.layer_norm_eps, batch, D, cls_out, s);
    return rc;
}

int cs_cosine_reward(const float* pred, const float* target, int batch, int dim, int64_t target_stride, float* out, void* stream) {
    if (batch < 0 || dim <= 0 || target_stride < 0) CS_FAIL(CS_E_ARG, "cosine reward: bad size");
    if (batch == 0) return CS_OK;
    return launch_cosine_reward(pred, target, (long)target_stride, batch, dim, out, (hipStream_t)stream);
}

}  // extern "C"
