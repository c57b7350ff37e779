// CLIP vision tower + projection: the image features of the CLIP image-similarity reward (reward_type "clip": edit_ppo/reward_model.py:128-134, 512-552).
//
// Replaces, for a batch of decoded images [B,3,H,W] in [0,1]:  ToPILImage -> the openai/clip-vit-large-patch14 processor (PIL bicubic resize to shortest edge
// 224, center crop 224, rescale, normalise) -> transformers CLIPModel.get_image_features (bias-free 14 x 14 patch conv, class embedding, learned position
// table, pre_layrnorm, 24 pre-LN layers with quick-GELU, post_layernorm of the CLS row, bias-free visual_projection) -> image_embeds [B, 768] fp32.
// The front end is the DINOv2 reward's (vit_ops.hip, with this processor's constants), the layer stack is encoder.h's loop (unmasked, quick-GELU, head dim 64);
// what CLIP has of its own are the two ends: launch_clipv_tokens_ln (embeddings + pre_layrnorm in one pass) and launch_clipv_head.
#include "image_tower.h"
#include "consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

struct CsClipVision {
    CsClipVisionConfig cfg;
    ImageTower tower;                                      // its final LayerNorm is post_layernorm
    f16 *preg = nullptr, *preb = nullptr, *wproj = nullptr;
};

namespace {

const TowerNames NAMES = {"clip vision", "clipv", "clip vision handle is NULL"};
const char* const VM = "vision_model.";

void build_manifest(CsClipVision* c) {          // transformers CLIPVisionModelWithProjection.state_dict() order (CLIPModel's vision part under the same names)
    WeightManifest& m = c->tower.weights;
    const int D = c->cfg.hidden_size, I = c->cfg.intermediate_size, P = c->cfg.patch_size;
    const std::string v = VM;
    m.expect(v + "embeddings.class_embedding", {D});
    m.expect(v + "embeddings.patch_embedding.weight", {D, 3, P, P});
    m.expect(v + "embeddings.position_embedding.weight", {c->tower.T, D});
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

bool pack(CsClipVision* c) {
    ImageTower& t = c->tower;
    WeightStore<float>& W = t.weights;
    const std::string v = VM;
    auto T = [&](const std::string& n) -> const std::vector<float>& { return W.at(v + n).data; };
    t.wpatch = image_tower::pack_patch_projection(t, v + "embeddings.patch_embedding.weight");          // no bias in CLIP
    t.cls = W.upload(T("embeddings.class_embedding")); t.pos = W.upload(T("embeddings.position_embedding.weight"));
    c->preg = W.upload(T("pre_layrnorm.weight")); c->preb = W.upload(T("pre_layrnorm.bias"));
    t.lnfg = W.upload(T("post_layernorm.weight")); t.lnfb = W.upload(T("post_layernorm.bias"));
    c->wproj = W.upload(W.at("visual_projection.weight").data);
    bool ok = t.wpatch && t.cls && t.pos && c->preg && c->preb && t.lnfg && t.lnfb && c->wproj;
    t.layers.resize(c->cfg.num_hidden_layers);
    for (int l = 0; l < c->cfg.num_hidden_layers && ok; ++l) {
        const std::string p = v + "encoder.layers." + std::to_string(l);
        ok = pack_pre_ln_layer<float>(W, {p + ".self_attn.q_proj", p + ".self_attn.k_proj", p + ".self_attn.v_proj", p + ".self_attn.out_proj",
                                          p + ".layer_norm1", p + ".layer_norm2", p + ".mlp.fc1", p + ".mlp.fc2"}, nullptr, nullptr, t.layers[l]);
    }
    return ok;
}

}  // namespace

extern "C" {

int cs_clipv_create(const CsClipVisionConfig* cfg, CsClipVision** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    int rc = image_tower::check_encoder_config(NAMES.who, "hidden (up to 2048) / intermediate size", 2048, cfg->hidden_size, cfg->intermediate_size, cfg->num_attention_heads,
                                               cfg->num_hidden_layers, cfg->patch_size, cfg->image_size);          // (launch_clipv_head holds a row of at most 2048)
    if (rc != CS_OK) return rc;
    if (cfg->projection_dim < 1) CS_FAIL(CS_E_ARG, "clip vision: bad config");
    if (cfg->crop_size != cfg->image_size) CS_FAIL(CS_E_UNSUPPORTED, "clip vision: crop_size %d must equal image_size %d (CLIP's position table is not interpolated)",
                                                   cfg->crop_size, cfg->image_size);
    if (cfg->resize_shortest_edge < cfg->crop_size) CS_FAIL(CS_E_ARG, "clip vision: crop_size must be at most resize_shortest_edge");
    if ((rc = image_tower::check_image_std(NAMES.who, cfg->image_std)) != CS_OK) return rc;
    CsClipVision* c = new CsClipVision();
    c->cfg = *cfg;
    c->tower.init(cfg->hidden_size, cfg->intermediate_size, cfg->num_attention_heads, cfg->layer_norm_eps, cfg->patch_size, cfg->resize_shortest_edge, cfg->crop_size,
                  cfg->image_mean, cfg->image_std, cfg->rescale_factor);
    build_manifest(c);
    *out = c;
    return CS_OK;
}

void cs_clipv_destroy(CsClipVision* c) {
    if (!c) return;
    c->tower.free_device();
    delete c;
}

int cs_clipv_num_weights(const CsClipVision* c) { return c ? c->tower.weights.count() : 0; }

const char* cs_clipv_weight_name(const CsClipVision* c, int i, int64_t* shape4, int* ndim) { return c ? c->tower.weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_clipv_set_weight(CsClipVision* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    return image_tower::set_weight(tower_of(c), name, data, shape, ndim);
}

int cs_clipv_finalize(CsClipVision* c) { return image_tower::finalize(NAMES, tower_of(c), [&] { return pack(c); }); }

int cs_clipv_patch_cols(const CsClipVision* c) { return c ? c->tower.Kpad : 0; }
int cs_clipv_num_tokens(const CsClipVision* c) { return c ? c->tower.T : 0; }

size_t cs_clipv_workspace_bytes(const CsClipVision* c, int batch) { return !c || batch <= 0 ? 0 : c->tower.workspace_elems((size_t)batch) * sizeof(f16) + 4096; }

double cs_clipv_flops(const CsClipVision* c, int batch) {
    return c ? c->tower.flops(c->cfg.num_hidden_layers, batch) + 2.0 * batch * (double)c->cfg.hidden_size * c->cfg.projection_dim : 0;
}

size_t cs_clipv_preprocess_workspace_bytes(const CsClipVision* c, int batch, int height, int width) {
    return image_tower::preprocess_workspace_bytes(tower_of(c), batch, height, width);
}

int cs_clipv_preprocess(CsClipVision* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return image_tower::preprocess(NAMES, tower_of(c), images, dtype, batch, height, width, patches, crop_u8, workspace, workspace_bytes, stream);
}

int cs_clipv_forward(CsClipVision* c, const void* patches, int batch, float* image_embeds, void* workspace, size_t workspace_bytes, void* stream) {
    bool run = false;
    int rc = image_tower::begin_forward(NAMES, tower_of(c), batch, patches && image_embeds && workspace, workspace_bytes, cs_clipv_workspace_bytes(c, batch), &run);
    if (!run) return rc;
    const ImageTower& t = c->tower;
    if (t.too_many_rows(batch)) CS_FAIL(CS_E_SHAPE, "clip vision: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const PreLnWorkspace w = carve_pre_ln(workspace, (long)batch * t.T, t.D, t.I);
    f16* pe = w.end;
    rc = linear((const f16*)patches, batch * t.NP, t.Kpad, t.wpatch, nullptr, t.D, nullptr, pe, s);             // CLIP's patch conv has no bias
    if (rc == CS_OK) rc = launch_clipv_tokens_ln(pe, t.cls, t.pos, c->preg, c->preb, t.eps, w.x, batch, t.NP, t.D, s);
    if (rc == CS_OK) rc = run_pre_ln_layers(t.layers, w, batch, t.T, t.D, t.I, t.heads, t.eps, 0, launch_quick_gelu, s);
    if (rc == CS_OK) rc = launch_clipv_head(w.x, (long)t.T * t.D, t.lnfg, t.lnfb, t.eps, c->wproj, batch, t.D, c->cfg.projection_dim, image_embeds, s);
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
