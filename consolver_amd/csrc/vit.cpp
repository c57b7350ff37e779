// DINOv2 image encoder + the image-similarity reward around it (reward_type "dino": edit_ppo/reward_model.py:59-64, 217-257; run_ppo.sh:30).
//
// Replaces, for a batch of decoded images [B,3,H,W] in [0,1]:  ToPILImage -> the facebook/dinov2-base processor (PIL bicubic resize to shortest edge 256, center
// crop 224, rescale, normalise) -> transformers Dinov2Model (14 x 14 patch conv, CLS token, position table bicubically interpolated from its 37 x 37 training grid,
// 12 pre-LN layers with LayerScale and exact GELU, final LayerNorm) -> CLS row -> F.normalize / cosine_similarity -> (cos + 1) * 50.
// The encoder is encoder.h's layer loop (implicit-GEMM MFMA linears, flash attention at head dim 64 -- here unmasked, 257 tokens) with the LayerScale vectors folded
// into the out-projection / fc2 weights and biases at pack time (fp32 product, one rounding to fp16); the front end and the tail are vit_ops.hip.
// Everything up to the tail is image_tower.h's (shared with clip_vision.cpp and depth.cpp): checks, manifest, packing, front end, patch embed -> tokens.
#include "image_tower.h"
#include "consolver_hip.h"

struct CsVit {
    CsVitConfig cfg;
    ImageTower tower;      // the whole model but its tail: the CLS row's final LayerNorm
};

namespace {
const TowerNames NAMES = {"vit", "vit", "vit is NULL"};
}

extern "C" {

int cs_vit_create(const CsVitConfig* cfg, CsVit** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    const int mlp = cfg->mlp_ratio < 1 ? 0 : cfg->hidden_size * cfg->mlp_ratio;
    int rc = image_tower::check_encoder_config(NAMES.who, "hidden / MLP size", 0, cfg->hidden_size, mlp, cfg->num_attention_heads, cfg->num_hidden_layers, cfg->patch_size,
                                               cfg->image_size);
    if (rc != CS_OK) return rc;
    if (cfg->crop_size < cfg->patch_size || cfg->crop_size % cfg->patch_size || cfg->resize_shortest_edge < cfg->crop_size)
        CS_FAIL(CS_E_ARG, "vit: crop_size must be a multiple of patch_size and at most resize_shortest_edge");
    if ((rc = image_tower::check_image_std(NAMES.who, cfg->image_std)) != CS_OK) return rc;
    CsVit* c = new CsVit();
    c->cfg = *cfg;
    c->tower.init(cfg->hidden_size, mlp, cfg->num_attention_heads, cfg->layer_norm_eps, cfg->patch_size, cfg->resize_shortest_edge, cfg->crop_size, cfg->image_mean,
                  cfg->image_std, cfg->rescale_factor);
    image_tower::expect_dinov2_backbone(c->tower.weights, "", cfg->hidden_size, mlp, cfg->patch_size, cfg->image_size / cfg->patch_size, cfg->num_hidden_layers);
    *out = c;
    return CS_OK;
}

void cs_vit_destroy(CsVit* c) {
    if (!c) return;
    c->tower.free_device();
    delete c;
}

int cs_vit_num_weights(const CsVit* c) { return c ? c->tower.weights.count() : 0; }

const char* cs_vit_weight_name(const CsVit* c, int i, int64_t* shape4, int* ndim) { return c ? c->tower.weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_vit_set_weight(CsVit* c, const char* name, const float* data, const int64_t* shape, int ndim) { return image_tower::set_weight(tower_of(c), name, data, shape, ndim); }

int cs_vit_finalize(CsVit* c) {
    return image_tower::finalize(NAMES, tower_of(c), [&] { return image_tower::pack_dinov2_backbone(c->tower, "", c->cfg.image_size / c->cfg.patch_size, c->cfg.num_hidden_layers); });
}

int cs_vit_patch_cols(const CsVit* c) { return c ? c->tower.Kpad : 0; }
int cs_vit_num_tokens(const CsVit* c) { return c ? c->tower.T : 0; }

size_t cs_vit_workspace_bytes(const CsVit* c, int batch) { return !c || batch <= 0 ? 0 : c->tower.workspace_elems((size_t)batch) * sizeof(f16) + 4096; }

double cs_vit_flops(const CsVit* c, int batch) { return c ? c->tower.flops(c->cfg.num_hidden_layers, batch) : 0; }

size_t cs_vit_preprocess_workspace_bytes(const CsVit* c, int batch, int height, int width) { return image_tower::preprocess_workspace_bytes(tower_of(c), batch, height, width); }

int cs_vit_preprocess(CsVit* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                      void* workspace, size_t workspace_bytes, void* stream) {
    return image_tower::preprocess(NAMES, tower_of(c), images, dtype, batch, height, width, patches, crop_u8, workspace, workspace_bytes, stream);
}

int cs_vit_forward(CsVit* c, const void* patches, int batch, float* cls_out, void* workspace, size_t workspace_bytes, void* stream) {
    bool run = false;
    int rc = image_tower::begin_forward(NAMES, tower_of(c), batch, patches && cls_out && workspace, workspace_bytes, cs_vit_workspace_bytes(c, batch), &run);
    if (!run) return rc;
    const ImageTower& t = c->tower;
    if (t.too_many_rows(batch)) CS_FAIL(CS_E_SHAPE, "vit: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const PreLnWorkspace w = carve_pre_ln(workspace, (long)batch * t.T, t.D, t.I);
    rc = image_tower::embed_patches(t, patches, batch, w.end, w.x, s);
    if (rc == CS_OK) rc = run_pre_ln_layers(t.layers, w, batch, t.T, t.D, t.I, t.heads, t.eps, 0, launch_gelu_erf, s);
    if (rc == CS_OK) rc = launch_vit_cls_layer_norm(w.x, (long)t.T * t.D, t.lnfg, t.lnfb, t.eps, batch, t.D, cls_out, s);
    return rc;
}

int cs_cosine_reward(const float* pred, const float* target, int batch, int dim, int64_t target_stride, float* out, void* stream) {
    if (batch < 0 || dim <= 0 || target_stride < 0) CS_FAIL(CS_E_ARG, "cosine reward: bad size");
    if (batch == 0) return CS_OK;
    return launch_cosine_reward(pred, target, (long)target_stride, batch, dim, out, (hipStream_t)stream);
}

}  // extern "C"
