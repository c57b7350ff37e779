// CLIP vision tower + projection: the image features of the CLIP image-similarity reward (reward_type "clip": edit_ppo/reward_model.py:128-134, 512-552).
//
// Replaces, for a batch of decoded images [B,3,H,W] in [0,1]:  ToPILImage -> the openai/clip-vit-large-patch14 processor (PIL bicubic resize to shortest edge
// 224, center crop 224, rescale, normalise) -> transformers CLIPModel.get_image_features (bias-free 14 x 14 patch conv, class embedding, learned position
// table, pre_layrnorm, 24 pre-LN layers with quick-GELU, post_layernorm of the CLS row, bias-free visual_projection) -> image_embeds [B, 768] fp32.
// The front end is the DINOv2 reward's (vit_ops.hip, with this processor's constants), the layer stack is encoder.h's loop (unmasked, quick-GELU, head dim 64);
// what CLIP has of its own are the two ends: launch_clipv_tokens_ln (embeddings + pre_layrnorm in one pass) and launch_clipv_head.
#include "encoder.h"
#include "image_front_end.h"
#include "consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

struct CsClipVision {
    CsClipVisionConfig cfg;
    int G = 0, NP = 0, T = 0, K = 0, Kpad = 0;             // patch grid, patches, tokens, patch-row length (and padded)
    WeightStore<float> weights;                            // fp32 staging, rounded once at upload
    f16 *wpatch = nullptr, *cls = nullptr, *pos = nullptr, *preg = nullptr, *preb = nullptr, *postg = nullptr, *postb = nullptr, *wproj = nullptr;
    std::vector<PreLnLayer> layers;
    image_front_end::PlanCache plans;                      // resize tables per input (height, width), bounded (image_front_end.h)
};

namespace {

const char* const VM = "vision_model.";

void build_manifest(CsClipVision* c) {          // transformers CLIPVisionModelWithProjection.state_dict() order (CLIPModel's vision part under the same names)
    WeightManifest& m = c->weights;
    const int D = c->cfg.hidden_size, I = c->cfg.intermediate_size, P = c->cfg.patch_size;
    const std::string v = VM;
    m.expect(v + "embeddings.class_embedding", {D});
    m.expect(v + "embeddings.patch_embedding.weight", {D, 3, P, P});
    m.expect(v + "embeddings.position_embedding.weight", {c->T, D});
    m.expect(v + "pre_layrnorm.weight", {D}); m.expect(v + "pre_layrnorm.bias", {D});
    for (int l = 0; l < c->cfg.num_hidden_layers; ++l) {
        const std::string p = v + "encoder.layers." + std::to_string(l);
        for (const char* q : {".self_attn.k_proj", ".self_attn.v_proj", ".self_attn.q_proj", ".self_attn.out_proj"}) {
            m.expect(p + q + ".weight", {D, D}); m.expect(p + q + ".bias", {D});
        }
        m.expect(p + ".layer_norm1.weight", {D}); m.expect(p + ".layer_norm1.bias", {D});
        m.expect(p + ".mlp.fc1.weight", {I, D}); m.expect(p + ".mlp.fc1.bias", {I});
        m.expect(p + ".mlp.fc2.weight", {D, I}); m.expect(p + ".mlp.fc2.bias", {D});
        m.expect(p + ".layer_norm2.weight", {D}); m.expect(p + ".layer_norm2.bias", {D});
    }
    m.expect(v + "post_layernorm.weight", {D}); m.expect(v + "post_layernorm.bias", {D});
    m.expect("visual_projection.weight", {c->cfg.projection_dim, D});
}

}  // namespace

extern "C" {

int cs_clipv_create(const CsClipVisionConfig* cfg, CsClipVision** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    if (cfg->hidden_size < 128 || cfg->hidden_size % 128 || cfg->hidden_size > 2048 || cfg->intermediate_size < 128 || cfg->intermediate_size % 128)
        CS_FAIL(CS_E_SHAPE, "clip vision: hidden (up to 2048) / intermediate size must be multiples of 128");
    if (cfg->num_attention_heads < 1 || cfg->hidden_size != cfg->num_attention_heads * 64) CS_FAIL(CS_E_UNSUPPORTED, "clip vision: built for heads of dim 64");
    if (cfg->num_hidden_layers < 1 || cfg->patch_size < 1 || cfg->image_size < cfg->patch_size || cfg->image_size % cfg->patch_size || cfg->projection_dim < 1)
        CS_FAIL(CS_E_ARG, "clip vision: bad config");
    if (cfg->crop_size != cfg->image_size) CS_FAIL(CS_E_UNSUPPORTED, "clip vision: crop_size %d must equal image_size %d (CLIP's position table is not interpolated)",
                                                   cfg->crop_size, cfg->image_size);
    if (cfg->resize_shortest_edge < cfg->crop_size) CS_FAIL(CS_E_ARG, "clip vision: crop_size must be at most resize_shortest_edge");
    for (int i = 0; i < 3; ++i) if (!(cfg->image_std[i] > 0.f)) CS_FAIL(CS_E_ARG, "clip vision: image_std must be positive");
    CsClipVision* c = new CsClipVision();
    c->cfg = *cfg;
    c->G = cfg->crop_size / cfg->patch_size; c->NP = c->G * c->G; c->T = c->NP + 1;
    c->K = 3 * cfg->patch_size * cfg->patch_size; c->Kpad = (c->K + 63) / 64 * 64;
    build_manifest(c);
    *out = c;
    return CS_OK;
}

void cs_clipv_destroy(CsClipVision* c) {
    if (!c) return;
    c->weights.free_device();
    c->plans.free_device();
    delete c;
}

int cs_clipv_num_weights(const CsClipVision* c) { return c ? c->weights.count() : 0; }

const char* cs_clipv_weight_name(const CsClipVision* c, int i, int64_t* shape4, int* ndim) { return c ? c->weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_clipv_set_weight(CsClipVision* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!c) CS_FAIL(CS_E_ARG, "null argument");
    return c->weights.set(name, data, shape, ndim);
}

int cs_clipv_finalize(CsClipVision* c) {
    if (!c) CS_FAIL(CS_E_ARG, "null");
    WeightStore<float>& W = c->weights;
    if (W.finalized) return CS_OK;
    if (const std::string* n = W.first_missing()) CS_FAIL(CS_E_STATE, "missing weight '%s'", n->c_str());
    const std::string v = VM;
    auto T = [&](const std::string& n) -> const std::vector<float>& { return W.at(v + n).data; };
    const int D = c->cfg.hidden_size, K = c->K, Kpad = c->Kpad;
    {   // patch projection [D][3 P P] -> [D][Kpad] (no bias in CLIP)
        const auto& w = T("embeddings.patch_embedding.weight");
        std::vector<float> wp((size_t)D * Kpad, 0.f);
        for (int n = 0; n < D; ++n) std::copy(w.begin() + (size_t)n * K, w.begin() + (size_t)(n + 1) * K, wp.begin() + (size_t)n * Kpad);
        c->wpatch = W.upload(wp);
    }
    c->cls = W.upload(T("embeddings.class_embedding")); c->pos = W.upload(T("embeddings.position_embedding.weight"));
    c->preg = W.upload(T("pre_layrnorm.weight")); c->preb = W.upload(T("pre_layrnorm.bias"));
    c->postg = W.upload(T("post_layernorm.weight")); c->postb = W.upload(T("post_layernorm.bias"));
    c->wproj = W.upload(W.at("visual_projection.weight").data);
    bool ok = c->wpatch && c->cls && c->pos && c->preg && c->preb && c->postg && c->postb && c->wproj;
    c->layers.resize(c->cfg.num_hidden_layers);
    for (int l = 0; l < c->cfg.num_hidden_layers && ok; ++l) {
        const std::string p = v + "encoder.layers." + std::to_string(l);
        ok = pack_pre_ln_layer<float>(W, {p + ".self_attn.q_proj", p + ".self_attn.k_proj", p + ".self_attn.v_proj", p + ".self_attn.out_proj",
                                          p + ".layer_norm1", p + ".layer_norm2", p + ".mlp.fc1", p + ".mlp.fc2"}, nullptr, nullptr, c->layers[l]);
    }
    if (!ok) CS_FAIL(CS_E_HIP, "clip vision: weight upload failed (hipMalloc/hipMemcpy)");
    W.release_host();
    W.finalized = true;
    return CS_OK;
}

int cs_clipv_patch_cols(const CsClipVision* c) { return c ? c->Kpad : 0; }
int cs_clipv_num_tokens(const CsClipVision* c) { return c ? c->T : 0; }

size_t cs_clipv_workspace_bytes(const CsClipVision* c, int batch) {
    if (!c || batch <= 0) return 0;
    const size_t D = c->cfg.hidden_size;
    return (pre_ln_workspace_elems((size_t)batch * c->T, D, c->cfg.intermediate_size) + (size_t)batch * c->NP * D) * sizeof(f16) + 4096;   // the encoder stack's, patch embeddings
}

double cs_clipv_flops(const CsClipVision* c, int batch) {
    if (!c) return 0;
    const double D = c->cfg.hidden_size;
    return 2.0 * batch * c->NP * (double)c->K * D + pre_ln_flops(c->cfg.num_hidden_layers, batch, c->T, D, c->cfg.intermediate_size)
         + 2.0 * batch * D * c->cfg.projection_dim;
}

size_t cs_clipv_preprocess_workspace_bytes(const CsClipVision* c, int batch, int height, int width) {
    if (!c || batch <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)batch * 3 * height * c->cfg.crop_size + 256;          // the horizontal pass's rows (at most every input row) x crop columns, uint8
}

int cs_clipv_preprocess(CsClipVision* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "clip vision handle is NULL");
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!images || !patches || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    const image_front_end::Plan* pl = nullptr;
    const int rc = c->plans.get_plan("clip vision", c->cfg.resize_shortest_edge, c->cfg.crop_size, height, width, &pl);
    if (rc != CS_OK) return rc;
    if (workspace_bytes < (size_t)batch * 3 * pl->dev.nrows * c->cfg.crop_size) CS_FAIL(CS_E_ARG, "clip vision: preprocess workspace too small");
    return launch_vit_front_end(images, dtype, batch, height, width, pl->dev, c->cfg.image_mean, c->cfg.image_std, c->cfg.rescale_factor,
                                c->cfg.patch_size, c->G, c->Kpad, (unsigned char*)workspace, (f16*)patches, crop_u8, (hipStream_t)stream);
}

int cs_clipv_forward(CsClipVision* c, const void* patches, int batch, float* image_embeds, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "clip vision handle is NULL");
    if (!c->weights.finalized) CS_FAIL(CS_E_STATE, "cs_clipv_finalize has not been called");
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!patches || !image_embeds || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    if (workspace_bytes < cs_clipv_workspace_bytes(c, batch)) CS_FAIL(CS_E_ARG, "clip vision: workspace too small");
    const int D = c->cfg.hidden_size, I = c->cfg.intermediate_size, H = c->cfg.num_attention_heads, Tn = c->T;
    if ((long)batch * Tn > 0x7fffffffL / std::max(I, 3 * D)) CS_FAIL(CS_E_SHAPE, "clip vision: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const long rows = (long)batch * Tn;
    const PreLnWorkspace w = carve_pre_ln(workspace, rows, D, I);
    f16* pe = w.end;
    int rc = linear((const f16*)patches, batch * c->NP, c->Kpad, c->wpatch, nullptr, D, nullptr, pe, s);             // CLIP's patch conv has no bias
    if (rc == CS_OK) rc = launch_clipv_tokens_ln(pe, c->cls, c->pos, c->preg, c->preb, c->cfg.layer_norm_eps, w.x, batch, c->NP, D, s);
    if (rc == CS_OK) rc = run_pre_ln_layers(c->layers, w, batch, Tn, D, I, H, c->cfg.layer_norm_eps, 0, launch_quick_gelu, s);
    if (rc == CS_OK) rc = launch_clipv_head(w.x, (long)Tn * D, c->postg, c->postb, c->cfg.layer_norm_eps, c->wproj, batch, D, c->cfg.projection_dim, image_embeds, s);
    return rc;
}

int cs_op_clipv_tokens_ln(const void* pe, const void* cls, const void* pos, const void* gamma, const void* beta, float eps, void* x, int B, int NP, int D,
                          void* stream) {
    return launch_clipv_tokens_ln((const f16*)pe, (const f16*)cls, (const f16*)pos, (const f16*)gamma, (const f16*)beta, eps, (f16*)x, B, NP, D, (hipStream_t)stream);
}

int cs_op_clipv_head(const void* x, int64_t sample_stride, const void* gamma, const void* beta, float eps, const void* w, int B, int D, int P, float* out,
                     void* stream) {
    return launch_clipv_head((const f16*)x, (long)sample_stride, (const f16*)gamma, (const f16*)beta, eps, (const f16*)w, B, D, P, out, (hipStream_t)stream);
}

}  // extern "C"
