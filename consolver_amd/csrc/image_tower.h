// The image tower of the three reward handles (vit.cpp: DINOv2; clip_vision.cpp: CLIP; depth.cpp: Depth Anything's DINOv2 backbone), stated once (host only):
// a ViT over the processor's crop -- PIL-exact front end (image_front_end.h + launch_vit_front_end), patch projection as a GEMM over Kpad-padded patch rows,
// CLS + position table, encoder.h's pre-LN layer loop at head dim 64 -- with its weight store and the checks every C entry point of such a handle makes.
// A handle holds one ImageTower as its member `tower` and adds what its model has of its own: a manifest and a head.
#pragma once
#include "encoder.h"
#include "image_front_end.h"

#include <cmath>

// how a handle family names itself in error messages: "<who>: ...", "cs_<prefix>_finalize ...", and the text for a null handle
struct TowerNames { const char* who; const char* prefix; const char* null_handle; };

struct ImageTower {
    int D = 0, I = 0, heads = 0; float eps = 0.f;           // hidden size, MLP width, attention heads (of dim 64), LayerNorm eps
    int P = 0, G = 0, NP = 0, T = 0, K = 0, Kpad = 0;       // patch size, patch grid of the crop, patches, tokens, patch-row length (and padded to the GEMM's k step)
    int edge = 0, crop = 0;                                 // the processor: resize to this shortest edge, center crop
    float mean[3] = {0, 0, 0}, stdv[3] = {1, 1, 1}; double rescale = 0;   // normalise (x * rescale - mean) / stdv
    WeightStore<float> weights;                             // fp32 staging: every fold is formed in fp32 and rounded once at upload
    f16 *wpatch = nullptr, *bpatch = nullptr;               // patch projection [D][Kpad] (CLIP: no bias)
    f16 *cls = nullptr, *pos = nullptr;                     // class token, position table [T][D]
    f16 *lnfg = nullptr, *lnfb = nullptr;                   // the final LayerNorm
    std::vector<PreLnLayer> layers;
    image_front_end::PlanCache plans;                       // resize tables per input (height, width), bounded (image_front_end.h)

    void init(int hidden, int mlp, int nheads, float ln_eps, int patch, int resize_edge, int crop_size, const float* m, const float* s, double rescale_factor) {
        D = hidden; I = mlp; heads = nheads; eps = ln_eps; P = patch; edge = resize_edge; crop = crop_size; rescale = rescale_factor;
        std::copy(m, m + 3, mean); std::copy(s, s + 3, stdv);
        G = crop / P; NP = G * G; T = NP + 1; K = 3 * P * P; Kpad = (K + 63) / 64 * 64;
    }
    void free_device() { weights.free_device(); plans.free_device(); }
    // the encoder stack's buffers and the patch embeddings behind them (fp16 elements); a handle's own buffers follow
    size_t workspace_elems(size_t batch) const { return pre_ln_workspace_elems(batch * T, D, I) + batch * NP * D; }
    double flops(int nlayers, int batch) const { return 2.0 * batch * NP * (double)K * D + pre_ln_flops(nlayers, batch, T, D, I); }
    // batch * tokens * (the widest row any kernel of the call indexes) must fit an int
    bool too_many_rows(int batch, int widest = 0) const { return (long)batch * T > 0x7fffffffL / std::max(std::max(I, 3 * D), widest); }
};

template <typename Handle> ImageTower* tower_of(Handle* c) { return c ? &c->tower : nullptr; }
template <typename Handle> const ImageTower* tower_of(const Handle* c) { return c ? &c->tower : nullptr; }

namespace image_tower {

// ---- create: the checks on what the encoder and the processor can take (a handle adds its own between them) ------------------------------------------
// `widths` words the two sizes in the message ("hidden / MLP size"); max_hidden: a head kernel's limit on the hidden size, 0 for none
inline int check_encoder_config(const char* who, const char* widths, int max_hidden, int hidden, int mlp, int heads, int layers, int patch, int image_size) {
    if (hidden < 128 || hidden % 128 || (max_hidden && hidden > max_hidden) || mlp < 128 || mlp % 128) CS_FAIL(CS_E_SHAPE, "%s: %s must be multiples of 128", who, widths);
    if (heads < 1 || hidden != heads * 64) CS_FAIL(CS_E_UNSUPPORTED, "%s: built for heads of dim 64", who);
    if (layers < 1 || patch < 1 || image_size < patch || image_size % patch) CS_FAIL(CS_E_ARG, "%s: bad config", who);
    return CS_OK;
}
inline int check_image_std(const char* who, const float* image_std) {
    for (int i = 0; i < 3; ++i) if (!(image_std[i] > 0.f)) CS_FAIL(CS_E_ARG, "%s: image_std must be positive", who);
    return CS_OK;
}

// ---- the DINOv2 backbone: manifest and packing ------------------------------------------------------------------------------------------------------
// transformers Dinov2Model.state_dict() order under `prefix`; train_grid: the patch grid the position table was trained at (image_size / patch_size)
inline void expect_dinov2_backbone(WeightManifest& m, const std::string& prefix, int D, int I, int P, int train_grid, int layers) {
    m.expect(prefix + "embeddings.cls_token", {1, 1, D});
    m.expect(prefix + "embeddings.mask_token", {1, D});                                   // in the published count; pre-training only, unused by the forward
    m.expect(prefix + "embeddings.position_embeddings", {1, (int64_t)train_grid * train_grid + 1, D});
    m.expect(prefix + "embeddings.patch_embeddings.projection.weight", {D, 3, P, P});
    m.expect(prefix + "embeddings.patch_embeddings.projection.bias", {D});
    for (int l = 0; l < layers; ++l) {
        const std::string p = prefix + "encoder.layer." + std::to_string(l);
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
    m.expect(prefix + "layernorm.weight", {D}); m.expect(prefix + "layernorm.bias", {D});
}

// torch F.interpolate(mode="bicubic", align_corners=False) of the [s][s][D] position grid to [g][g][D] (cubic convolution, A = -0.75, clamped reads)
inline void cubic_taps(double t, double* k) {
    const double A = -0.75;
    auto c1 = [&](double x) { return ((A + 2) * x - (A + 3)) * x * x + 1; };
    auto c2 = [&](double x) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; };
    k[0] = c2(t + 1); k[1] = c1(t); k[2] = c1(1 - t); k[3] = c2(2 - t);
}
inline std::vector<float> interpolate_positions(const float* grid, int s, int g, int D) {
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

// patch projection [D][3 P P] -> [D][Kpad], zero padded: the GEMM's B operand over the front end's patch rows
inline f16* pack_patch_projection(ImageTower& t, const std::string& weight_name) {
    const auto& w = t.weights.at(weight_name).data;
    std::vector<float> wp((size_t)t.D * t.Kpad, 0.f);
    for (int n = 0; n < t.D; ++n) std::copy(w.begin() + (size_t)n * t.K, w.begin() + (size_t)(n + 1) * t.K, wp.begin() + (size_t)n * t.Kpad);
    return t.weights.upload(wp);
}

// the tensors of expect_dinov2_backbone onto the device: the patch projection; the position table of the crop's grid with its class row pre-added to the CLS
// token in fp32 and the patch grid interpolated when the crop's grid is not the training grid; the final LayerNorm; the first layers_to_pack layers (a handle
// that taps the stack packs no layer behind its last tap) with the LayerScale vectors folded into out-proj / fc2.  False when an upload fails
inline bool pack_dinov2_backbone(ImageTower& t, const std::string& prefix, int train_grid, int layers_to_pack) {
    WeightStore<float>& W = t.weights;
    auto at = [&](const char* n) -> const std::vector<float>& { return W.at(prefix + n).data; };
    const int D = t.D, s = train_grid, G = t.G;
    t.wpatch = pack_patch_projection(t, prefix + "embeddings.patch_embeddings.projection.weight");
    t.bpatch = W.upload(at("embeddings.patch_embeddings.projection.bias"));
    {
        const auto& pos = at("embeddings.position_embeddings");
        const auto& cls = at("embeddings.cls_token");
        std::vector<float> cls0(D), table((size_t)t.T * D, 0.f);
        for (int d = 0; d < D; ++d) cls0[d] = cls[d] + pos[d];
        if (G == s) std::copy(pos.begin() + D, pos.end(), table.begin() + D);
        else { const auto g = interpolate_positions(pos.data() + D, s, G, D); std::copy(g.begin(), g.end(), table.begin() + D); }
        t.cls = W.upload(cls0); t.pos = W.upload(table);
    }
    t.lnfg = W.upload(at("layernorm.weight")); t.lnfb = W.upload(at("layernorm.bias"));
    bool ok = t.wpatch && t.bpatch && t.cls && t.pos && t.lnfg && t.lnfb;
    t.layers.resize(layers_to_pack);
    for (int l = 0; l < layers_to_pack && ok; ++l) {
        const std::string p = prefix + "encoder.layer." + std::to_string(l);
        ok = pack_pre_ln_layer<float>(W, {p + ".attention.attention.query", p + ".attention.attention.key", p + ".attention.attention.value", p + ".attention.output.dense",
                                          p + ".norm1", p + ".norm2", p + ".mlp.fc1", p + ".mlp.fc2"},
                                      &W.at(p + ".layer_scale1.lambda1").data, &W.at(p + ".layer_scale2.lambda1").data, t.layers[l]);
    }
    return ok;
}

// ---- the weight protocol's entry points --------------------------------------------------------------------------------------------------------------
inline int set_weight(ImageTower* t, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!t) CS_FAIL(CS_E_ARG, "null argument");
    return t->weights.set(name, data, shape, ndim);
}
// cs_X_finalize around the handle's packing (pack() -> false when an upload failed): a second call is a no-op, a missing tensor is named
template <typename Pack> int finalize(const TowerNames& nm, ImageTower* t, Pack pack) {
    if (!t) CS_FAIL(CS_E_ARG, "null");
    WeightStore<float>& W = t->weights;
    if (W.finalized) return CS_OK;
    if (const std::string* n = W.first_missing()) CS_FAIL(CS_E_STATE, "missing weight '%s'", n->c_str());
    if (!pack()) CS_FAIL(CS_E_HIP, "%s: weight upload failed (hipMalloc/hipMemcpy)", nm.who);
    W.release_host();
    W.finalized = true;
    return CS_OK;
}

// ---- front end: cs_X_preprocess_workspace_bytes / cs_X_preprocess -----------------------------------------------------------------------------------------
inline size_t preprocess_workspace_bytes(const ImageTower* t, int batch, int height, int width) {
    if (!t || batch <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)batch * 3 * height * t->crop + 256;          // the horizontal pass's rows (at most every input row) x crop columns, uint8
}
inline int preprocess(const TowerNames& nm, ImageTower* t, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!t) CS_FAIL(CS_E_ARG, "%s", nm.null_handle);
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!images || !patches || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    const image_front_end::Plan* pl = nullptr;
    const int rc = t->plans.get_plan(nm.who, t->edge, t->crop, height, width, &pl);
    if (rc != CS_OK) return rc;
    if (workspace_bytes < (size_t)batch * 3 * pl->dev.nrows * t->crop) CS_FAIL(CS_E_ARG, "%s: preprocess workspace too small", nm.who);
    return launch_vit_front_end(images, dtype, batch, height, width, pl->dev, t->mean, t->stdv, t->rescale, t->P, t->G, t->Kpad, (unsigned char*)workspace,
                                (f16*)patches, crop_u8, (hipStream_t)stream);
}

// the front end of a processor that resizes the whole image to out_h x out_w (no crop), behind the handle's own size rule: the argument checks of `preprocess`,
// the two-axis plan, the workspace check.  *plan is set when the call has work to do; otherwise the return value is the call's
inline size_t preprocess_hw_workspace_bytes(int batch, int height, int out_w) { return (size_t)batch * 3 * height * out_w + 256; }
inline int begin_preprocess_hw(const TowerNames& nm, ImageTower* t, const void* images, int batch, int height, int width, int out_h, int out_w, const void* patches,
                               const void* workspace, size_t workspace_bytes, const image_front_end::Plan** plan) {
    *plan = nullptr;
    if (!t) CS_FAIL(CS_E_ARG, "%s", nm.null_handle);
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!images || !patches || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    const image_front_end::Plan* pl = nullptr;
    const int rc = t->plans.get_plan_hw(nm.who, height, width, out_h, out_w, &pl);
    if (rc != CS_OK) return rc;
    if (workspace_bytes < (size_t)batch * 3 * pl->dev.nrows * out_w) CS_FAIL(CS_E_ARG, "%s: preprocess workspace too small", nm.who);
    *plan = pl;
    return CS_OK;
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------------------------
// the argument checks of cs_X_forward.  *run is set when the call has work to do; otherwise the return value is the call's (CS_OK for an empty batch).
// pointers_ok: none of the caller's buffers is null; need: cs_X_workspace_bytes of this batch
inline int begin_forward(const TowerNames& nm, const ImageTower* t, int batch, bool pointers_ok, size_t workspace_bytes, size_t need, bool* run) {
    *run = false;
    if (!t) CS_FAIL(CS_E_ARG, "%s", nm.null_handle);
    if (!t->weights.finalized) CS_FAIL(CS_E_STATE, "cs_%s_finalize has not been called", nm.prefix);
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!pointers_ok) CS_FAIL(CS_E_ARG, "null pointer");
    if (workspace_bytes < need) CS_FAIL(CS_E_ARG, "%s: workspace too small", nm.who);
    *run = true;
    return CS_OK;
}
// patch rows [batch * NP][Kpad] -> patch embeddings pe -> tokens x [batch * T][D] with the CLS row and the position table added (DINOv2)
inline int embed_patches(const ImageTower& t, const void* patches, int batch, f16* pe, f16* x, hipStream_t s) {
    const int rc = linear((const f16*)patches, batch * t.NP, t.Kpad, t.wpatch, t.bpatch, t.D, nullptr, pe, s);
    return rc != CS_OK ? rc : launch_vit_tokens(pe, t.cls, t.pos, x, batch, t.NP, t.D, s);
}

}  // namespace image_tower
