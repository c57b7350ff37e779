// CLIP text encoder (the prompt front-end of the SD1.5 path).
//
// Replaces `text_encoder(input_ids)[0]` (denoise_ppo.py:25-50, gen_pretrain/pipeline.py:402-517): third-party
// transformers CLIPTextModel (CLIP ViT-L/14 text tower for SD1.5: 12 pre-LN layers, width 768, 12 heads of 64, MLP 3072
// with quick_gelu, causal mask, learned positions, final LayerNorm).  Tokens are [rows = B * 77] x width fp16;
// every linear runs through the implicit-GEMM MFMA kernels, attention through the flash kernel's causal head-64 form.
// It runs once per prompt batch (6.6 GMAC per prompt), i.e. < 0.1 % of an 8-step generation.
#include "encoder.h"
#include "consolver_hip.h"

struct CsClip {
    CsClipConfig cfg;
    WeightStore<f16> weights;
    f16 *tok = nullptr, *pos = nullptr, *lnfg = nullptr, *lnfb = nullptr;
    std::vector<PreLnLayer> layers;
};

namespace {

void build_manifest(CsClip* c) {
    WeightManifest& m = c->weights;
    const int D = c->cfg.hidden_size, I = c->cfg.intermediate_size;
    m.expect("embeddings.token_embedding.weight", {c->cfg.vocab_size, D});
    m.expect("embeddings.position_embedding.weight", {c->cfg.max_position_embeddings, D});
    for (int l = 0; l < c->cfg.num_hidden_layers; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l);
        for (const char* q : {".self_attn.k_proj", ".self_attn.v_proj", ".self_attn.q_proj", ".self_attn.out_proj"}) {
            m.expect(p + q + ".weight", {D, D}); m.expect(p + q + ".bias", {D});
        }
        m.expect(p + ".layer_norm1.weight", {D}); m.expect(p + ".layer_norm1.bias", {D});
        m.expect(p + ".mlp.fc1.weight", {I, D}); m.expect(p + ".mlp.fc1.bias", {I});
        m.expect(p + ".mlp.fc2.weight", {D, I}); m.expect(p + ".mlp.fc2.bias", {D});
        m.expect(p + ".layer_norm2.weight", {D}); m.expect(p + ".layer_norm2.bias", {D});
    }
    m.expect("final_layer_norm.weight", {D}); m.expect("final_layer_norm.bias", {D});
}

}  // namespace

extern "C" {

int cs_clip_create(const CsClipConfig* cfg, CsClip** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    if (cfg->hidden_size % 128 || cfg->intermediate_size % 128) CS_FAIL(CS_E_SHAPE, "clip: hidden / intermediate size must be multiples of 128");
    if (cfg->num_attention_heads < 1 || cfg->hidden_size != cfg->num_attention_heads * 64) CS_FAIL(CS_E_UNSUPPORTED, "clip: built for heads of dim 64");
    if (cfg->num_hidden_layers < 1 || cfg->vocab_size < 1 || cfg->max_position_embeddings < 1) CS_FAIL(CS_E_ARG, "clip: bad config");
    CsClip* c = new CsClip();
    c->cfg = *cfg;
    build_manifest(c);
    *out = c;
    return CS_OK;
}

void cs_clip_destroy(CsClip* c) {
    if (!c) return;
    c->weights.free_device();
    delete c;
}

int cs_clip_num_weights(const CsClip* c) { return c ? c->weights.count() : 0; }

const char* cs_clip_weight_name(const CsClip* c, int i, int64_t* shape4, int* ndim) { return c ? c->weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_clip_set_weight(CsClip* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!c) CS_FAIL(CS_E_ARG, "null argument");
    return c->weights.set(name, data, shape, ndim);
}

int cs_clip_finalize(CsClip* c) {
    if (!c) CS_FAIL(CS_E_ARG, "null");
    WeightStore<f16>& W = c->weights;
    if (W.finalized) return CS_OK;
    if (const std::string* n = W.first_missing()) CS_FAIL(CS_E_STATE, "missing weight '%s'", n->c_str());
    c->tok = W.upload(W.at("embeddings.token_embedding.weight").data); c->pos = W.upload(W.at("embeddings.position_embedding.weight").data);
    c->lnfg = W.upload(W.at("final_layer_norm.weight").data); c->lnfb = W.upload(W.at("final_layer_norm.bias").data);
    bool ok = c->tok && c->pos && c->lnfg && c->lnfb;
    c->layers.resize(c->cfg.num_hidden_layers);
    for (int l = 0; l < c->cfg.num_hidden_layers && ok; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l);
        ok = pack_pre_ln_layer<f16>(W, {p + ".self_attn.q_proj", p + ".self_attn.k_proj", p + ".self_attn.v_proj", p + ".self_attn.out_proj", p + ".layer_norm1",
                                        p + ".layer_norm2", p + ".mlp.fc1", p + ".mlp.fc2"}, nullptr, nullptr, c->layers[l]);
    }
    if (!ok) CS_FAIL(CS_E_HIP, "clip: weight upload failed (hipMalloc/hipMemcpy)");
    W.release_host();
    W.finalized = true;
    return CS_OK;
}

size_t cs_clip_workspace_bytes(const CsClip* c, int batch, int seq_len) {
    if (!c || batch <= 0 || seq_len <= 0) return 0;
    return pre_ln_workspace_elems((size_t)batch * seq_len, c->cfg.hidden_size, c->cfg.intermediate_size) * sizeof(f16) + 4096;
}

double cs_clip_flops(const CsClip* c, int batch, int seq_len) {
    if (!c) return 0;
    return pre_ln_flops(c->cfg.num_hidden_layers, batch, seq_len, c->cfg.hidden_size, c->cfg.intermediate_size);
}

int cs_clip_encode(CsClip* c, const int64_t* input_ids, int batch, int seq_len, void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "clip is NULL");
    if (!c->weights.finalized) CS_FAIL(CS_E_STATE, "cs_clip_finalize has not been called");
    if (batch < 0 || seq_len < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0 || seq_len == 0) return CS_OK;
    if (seq_len > c->cfg.max_position_embeddings) CS_FAIL(CS_E_SHAPE, "clip: sequence of %d tokens exceeds max_position_embeddings %d", seq_len, c->cfg.max_position_embeddings);
    if (!input_ids || !out || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    if (workspace_bytes < cs_clip_workspace_bytes(c, batch, seq_len)) CS_FAIL(CS_E_ARG, "clip: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int D = c->cfg.hidden_size, I = c->cfg.intermediate_size, H = c->cfg.num_attention_heads;
    const long rows = (long)batch * seq_len;
    const PreLnWorkspace w = carve_pre_ln(workspace, rows, D, I);
    int rc = launch_embed_tokens(input_ids, c->tok, c->pos, w.x, rows, seq_len, D, c->cfg.vocab_size, s);
    if (rc == CS_OK) rc = run_pre_ln_layers(c->layers, w, batch, seq_len, D, I, H, c->cfg.layer_norm_eps, 1, launch_quick_gelu, s);
    if (rc == CS_OK) rc = launch_layer_norm(w.x, c->lnfg, c->lnfb, (f16*)out, (int)rows, D, c->cfg.layer_norm_eps, s);
    return rc;
}

}  // extern "C"
