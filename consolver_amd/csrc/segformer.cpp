// SegFormer semantic segmentation: the class masks of the mask-agreement reward (reward_type "segmentation": edit_ppo/reward_model.py:110-117, 425-481).
//
// Replaces, for a batch of decoded images [B,3,H,H] in [0,1]:  ToPILImage -> the Segformer image processor of nvidia/segformer-b4-finetuned-ade-512-512 (PIL
// BILINEAR resize to size x size, rescale, normalise, no crop) -> transformers SegformerForSemanticSegmentation (MiT encoder: four stages of overlapped patch
// embedding + LayerNorm, blocks of efficient self-attention and Mix-FFN, a final LayerNorm per stage; all-MLP head) -> argmax over the classes at a quarter of
// the processor's size.  The front end is the DINOv2 reward's (vit_ops.hip) with the bilinear tap tables, patch size 1 and rows of 8 halfs: the normalised
// image as NHWC-8.  Every linear layer runs on the MFMA kernels: launch_igemm where the output width is a multiple of 128 or 160 (the stride-2 3x3 embeddings
// directly, taps = 9), launch_dpt_conv (taps = 1) for the 64-wide layers of stage 1.  What is SegFormer's own is seg_ops.hip.  Packing, in fp32 with one rounding:
//   * the 7x7 stride-4 embedding as a linear over im2col rows (F.unfold order, K = 147 zero-padded to 192);
//   * the sequence reduction conv (kernel = stride = sr) as a linear over the patchify rows, weight [C][ky kx][ci]; key and value fused to one [2C][C] linear;
//   * the depthwise filter [4C][1][3][3] as [9][4C];
//   * BatchNorm2d (eval) folded into the bias-free linear_fuse: W' = W gamma / sqrt(var + eps), b' = beta - mean gamma / sqrt(var + eps);
//   * the classifier's rows zero-padded to the GEMM's tile (150 -> 160).
// Every nn.LayerNorm of the model has torch's default eps = 1e-5 (config.layer_norm_eps is not used by them), and so has the BatchNorm.
#include "image_tower.h"
#include "consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

namespace {
struct Lin { f16* w = nullptr; f16* b = nullptr; };
struct Block { Lin ln1, q, kv, o, sr, srln, ln2, fc1, dw, fc2; };
struct Stage { Lin pe, peln, ln; std::vector<Block> blocks; };
constexpr float LN_EPS = 1e-5f, BN_EPS = 1e-5f;
constexpr int PE_K = 192;                  // 3 * 7 * 7 = 147 padded to the GEMMs' k step
}  // namespace

struct CsSeg {
    CsSegConfig cfg;
    ImageTower tower;                      // the front end (plans, processor constants) and the weight store; the encoder fields are unused
    int S = 0, Dd = 0, NL = 0, NLp = 0, mlp = 0;
    int g[4] = {0, 0, 0, 0}, C[4] = {0, 0, 0, 0}, nk[4] = {0, 0, 0, 0};      // per stage: grid edge, width, key tokens per image
    Stage st[4];
    Lin proj[4], fuse, cls;
    int parts = 5;                         // cs_seg_set_stage_limit: the forward stops after this many of (stage 1 .. 4, head); timing tools only
};

namespace {

const TowerNames NAMES = {"segformer", "seg", "segformer handle is NULL"};

bool gemm_width(int n) { return n % 128 == 0 || n % 160 == 0; }

void build_manifest(CsSeg* c) {            // transformers SegformerForSemanticSegmentation.state_dict() order
    WeightManifest& m = c->tower.weights;
    auto wb = [&](const std::string& p, std::vector<int64_t> shape) { const int64_t n = shape[0]; m.expect(p + ".weight", std::move(shape)); m.expect(p + ".bias", {n}); };
    for (int i = 0; i < 4; ++i) {
        const int C = c->C[i], I = C * c->mlp, sr = c->cfg.sr_ratios[i];
        const std::string s = "segformer.stages." + std::to_string(i);
        if (i == 0) wb(s + ".patch_embeddings.proj", {C, 3, 7, 7}); else wb(s + ".patch_embeddings.proj", {C, c->C[i - 1], 3, 3});
        wb(s + ".patch_embeddings.layer_norm", {C});
        for (int l = 0; l < c->cfg.depths[i]; ++l) {
            const std::string p = s + ".blocks." + std::to_string(l);
            wb(p + ".layernorm_before", {C});
            for (const char* q : {".attention.q_proj", ".attention.k_proj", ".attention.v_proj", ".attention.o_proj"}) wb(p + q, {C, C});
            if (sr > 1) { wb(p + ".attention.sequence_reduction.sequence_reduction", {C, C, sr, sr}); wb(p + ".attention.sequence_reduction.layer_norm", {C}); }
            wb(p + ".layernorm_after", {C});
            wb(p + ".mlp.fc1", {I, C});
            wb(p + ".mlp.dwconv.dwconv", {I, 1, 3, 3});
            wb(p + ".mlp.fc2", {C, I});
        }
        wb(s + ".layer_norm", {C});
    }
    for (int i = 0; i < 4; ++i) wb("decode_head.linear_projections." + std::to_string(i) + ".proj", {c->Dd, c->C[i]});
    m.expect("decode_head.linear_fuse.weight", {c->Dd, 4 * c->Dd, 1, 1});
    wb("decode_head.batch_norm", {c->Dd});
    m.expect("decode_head.batch_norm.running_mean", {c->Dd}); m.expect("decode_head.batch_norm.running_var", {c->Dd});
    m.expect("decode_head.batch_norm.num_batches_tracked", {});               // in the state dict; eval mode never reads it
    wb("decode_head.classifier", {c->NL, c->Dd, 1, 1});
}

// [co][ci][kh][kw] -> [co][kh kw][ci]
std::vector<float> pack_taps(const HostTensor<float>& t) {
    const int64_t co = t.shape[0], ci = t.shape[1], kk = t.shape[2] * t.shape[3];
    std::vector<float> o((size_t)co * kk * ci);
    for (int64_t n = 0; n < co; ++n)
        for (int64_t ch = 0; ch < ci; ++ch)
            for (int64_t k = 0; k < kk; ++k) o[((size_t)n * kk + k) * ci + ch] = t.data[(n * ci + ch) * kk + k];
    return o;
}

// workspace carve-up (fp16 elements).  x: hidden state | n: its LayerNorm | q (also a patch embedding before its LayerNorm) | a: attention output | p: im2col /
// patchify rows | r, kn, kv: reduced sequence, its LayerNorm, keys | values | h1, h2: the Mix-FFN's wide activations | f[i]: stage outputs | pj: a head
// projection, then the fused features | cat: the head's concat | lg: fp16 logits [rows][NLp] (cs_seg_masks reads them)
struct Layout { size_t x, n, q, a, p, r, kn, kv, h1, h2, f[4], pj, cat, lg, total; };
Layout layout(const CsSeg* c, size_t B) {
    size_t rc = 0, kc = 0;
    for (int i = 0; i < 4; ++i) {
        rc = std::max(rc, (size_t)c->g[i] * c->g[i] * c->C[i]);
        kc = std::max(kc, (size_t)c->nk[i] * c->C[i]);
    }
    const size_t r0 = (size_t)c->g[0] * c->g[0];
    Layout L;
    size_t o = 0;
    auto take = [&](size_t per_image) { const size_t at = o; o += B * ((per_image + 63) / 64 * 64); return at; };
    L.x = take(rc); L.n = take(rc); L.q = take(rc); L.a = take(rc);
    L.p = take(std::max(rc, r0 * PE_K));
    L.r = take(kc); L.kn = take(kc); L.kv = take(2 * kc);
    L.h1 = take(rc * c->mlp); L.h2 = take(rc * c->mlp);
    for (int i = 0; i < 4; ++i) L.f[i] = take((size_t)c->g[i] * c->g[i] * c->C[i]);
    L.pj = take(r0 * c->Dd); L.cat = take(r0 * 4 * c->Dd); L.lg = take(r0 * c->NLp);
    L.total = o;
    return L;
}

bool pack(CsSeg* c) {
    WeightStore<float>& W = c->tower.weights;
    auto T = [&](const std::string& n) -> const std::vector<float>& { return W.at(n).data; };
    auto up = [&](const std::string& p, Lin& l) { l.w = W.upload(T(p + ".weight")); l.b = W.upload(T(p + ".bias")); return l.w && l.b; };
    bool ok = true;
    for (int i = 0; i < 4 && ok; ++i) {
        const int C = c->C[i], sr = c->cfg.sr_ratios[i];
        const std::string s = "segformer.stages." + std::to_string(i);
        Stage& st = c->st[i];
        if (i == 0) {
            const auto& w = T(s + ".patch_embeddings.proj.weight");
            std::vector<float> wp((size_t)C * PE_K, 0.f);
            for (int n = 0; n < C; ++n) std::copy(w.begin() + (size_t)n * 147, w.begin() + (size_t)(n + 1) * 147, wp.begin() + (size_t)n * PE_K);
            st.pe.w = W.upload(wp);
        } else st.pe.w = W.upload(pack_taps(W.at(s + ".patch_embeddings.proj.weight")));
        st.pe.b = W.upload(T(s + ".patch_embeddings.proj.bias"));
        ok = st.pe.w && st.pe.b && up(s + ".patch_embeddings.layer_norm", st.peln) && up(s + ".layer_norm", st.ln);
        st.blocks.resize(c->cfg.depths[i]);
        for (int l = 0; l < c->cfg.depths[i] && ok; ++l) {
            const std::string p = s + ".blocks." + std::to_string(l);
            Block& b = st.blocks[l];
            std::vector<float> kvw = T(p + ".attention.k_proj.weight"), kvb = T(p + ".attention.k_proj.bias");
            kvw.insert(kvw.end(), T(p + ".attention.v_proj.weight").begin(), T(p + ".attention.v_proj.weight").end());
            kvb.insert(kvb.end(), T(p + ".attention.v_proj.bias").begin(), T(p + ".attention.v_proj.bias").end());
            b.kv.w = W.upload(kvw); b.kv.b = W.upload(kvb);
            ok = b.kv.w && b.kv.b && up(p + ".layernorm_before", b.ln1) && up(p + ".attention.q_proj", b.q) && up(p + ".attention.o_proj", b.o) &&
                 up(p + ".layernorm_after", b.ln2) && up(p + ".mlp.fc1", b.fc1) && up(p + ".mlp.fc2", b.fc2);
            if (ok && sr > 1) {
                const std::string q = p + ".attention.sequence_reduction";
                b.sr.w = W.upload(pack_taps(W.at(q + ".sequence_reduction.weight"))); b.sr.b = W.upload(T(q + ".sequence_reduction.bias"));
                ok = b.sr.w && b.sr.b && up(q + ".layer_norm", b.srln);
            }
            if (ok) {
                const auto& dw = T(p + ".mlp.dwconv.dwconv.weight");           // [I][1][3][3] -> [9][I]
                const size_t I = (size_t)C * c->mlp;
                std::vector<float> t(9 * I);
                for (size_t ch = 0; ch < I; ++ch) for (int k = 0; k < 9; ++k) t[(size_t)k * I + ch] = dw[ch * 9 + k];
                b.dw.w = W.upload(t); b.dw.b = W.upload(T(p + ".mlp.dwconv.dwconv.bias"));
                ok = b.dw.w && b.dw.b;
            }
        }
    }
    for (int i = 0; i < 4 && ok; ++i) ok = up("decode_head.linear_projections." + std::to_string(i) + ".proj", c->proj[i]);
    if (ok) {
        const int Dd = c->Dd;
        const auto &w = T("decode_head.linear_fuse.weight"), &g = T("decode_head.batch_norm.weight"), &be = T("decode_head.batch_norm.bias");
        const auto &mu = T("decode_head.batch_norm.running_mean"), &var = T("decode_head.batch_norm.running_var");
        std::vector<float> fw(w.size()), fb(Dd);
        for (int n = 0; n < Dd; ++n) {
            const float sc = g[n] / std::sqrt(var[n] + BN_EPS);
            for (int k = 0; k < 4 * Dd; ++k) fw[(size_t)n * 4 * Dd + k] = w[(size_t)n * 4 * Dd + k] * sc;
            fb[n] = be[n] - mu[n] * sc;
        }
        c->fuse.w = W.upload(fw); c->fuse.b = W.upload(fb);
        std::vector<float> cw((size_t)c->NLp * Dd, 0.f), cb((size_t)c->NLp, 0.f);
        std::copy(T("decode_head.classifier.weight").begin(), T("decode_head.classifier.weight").end(), cw.begin());
        std::copy(T("decode_head.classifier.bias").begin(), T("decode_head.classifier.bias").end(), cb.begin());
        c->cls.w = W.upload(cw); c->cls.b = W.upload(cb);
        ok = c->fuse.w && c->fuse.b && c->cls.w && c->cls.b;
    }
    return ok;
}

// out [M][N] = x [M][K] w^T + b (+ res): the 64-wide layers on the narrow MFMA conv (1x1), the others on the implicit GEMM
int lin(const f16* x, long M, int K, const Lin& l, int N, const f16* res, f16* out, hipStream_t s) {
    if (N != 64) return linear(x, (int)M, K, l.w, l.b, N, res, out, s);
    DptConvArgs a{};
    a.x = x; a.B = 1; a.H = (int)M; a.W = 1; a.Cin = K; a.w = l.w; a.bias = l.b; a.Cout = 64; a.taps = 1; a.res = res; a.out = out;
    return launch_dpt_conv(a, s);
}

}  // namespace

extern "C" {

int cs_seg_create(const CsSegConfig* cfg, CsSeg** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    if (cfg->size < 32 || cfg->size % 32 || cfg->size > 2048) CS_FAIL(CS_E_SHAPE, "segformer: size %d must be a multiple of 32 up to 2048 (the four stages halve a size / 4 grid)", cfg->size);
    if (cfg->mlp_ratio < 1 || cfg->num_labels < 1 || cfg->num_labels > 4096) CS_FAIL(CS_E_ARG, "segformer: bad config");
    if (!gemm_width(cfg->decoder_hidden_size) || cfg->decoder_hidden_size > 4096) CS_FAIL(CS_E_SHAPE, "segformer: decoder_hidden_size %d must be a multiple of 128 or 160", cfg->decoder_hidden_size);
    int rc = image_tower::check_image_std(NAMES.who, cfg->image_std);
    if (rc != CS_OK) return rc;
    for (int i = 0; i < 4; ++i) {
        const int C = cfg->hidden_sizes[i], I = C * cfg->mlp_ratio, g = cfg->size >> (2 + i), sr = cfg->sr_ratios[i];
        if (cfg->num_attention_heads[i] < 1 || C != cfg->num_attention_heads[i] * 64) CS_FAIL(CS_E_UNSUPPORTED, "segformer: built for heads of dim 64 (stage %d: %d / %d)", i, C, cfg->num_attention_heads[i]);
        if (C != 64 && !gemm_width(C)) CS_FAIL(CS_E_SHAPE, "segformer: hidden size %d of stage %d must be 64 or a multiple of 128 or 160", C, i);
        if (!gemm_width(I) || I > 2048) CS_FAIL(CS_E_SHAPE, "segformer: Mix-FFN width %d of stage %d must be a multiple of 128 or 160 up to 2048", I, i);
        if (cfg->depths[i] < 1) CS_FAIL(CS_E_ARG, "segformer: depths must be positive");
        // the head-64 attention kernel takes any Nq and Nk >= 1 (ragged key tiles are masked); the reduction needs a whole kernel inside the grid
        if (sr < 1 || sr > g) CS_FAIL(CS_E_SHAPE, "segformer: sr_ratio %d of stage %d does not fit its %d x %d grid", sr, i, g, g);
    }
    CsSeg* c = new CsSeg();
    c->cfg = *cfg;
    c->S = cfg->size; c->Dd = cfg->decoder_hidden_size; c->NL = cfg->num_labels; c->mlp = cfg->mlp_ratio;
    for (c->NLp = 128; c->NLp < c->NL || !gemm_width(c->NLp); c->NLp += 32) {}
    for (int i = 0; i < 4; ++i) {
        c->C[i] = cfg->hidden_sizes[i]; c->g[i] = cfg->size >> (2 + i);
        const int k = c->g[i] / cfg->sr_ratios[i];
        c->nk[i] = k * k;
    }
    // the front end: the whole image resized to S x S with PIL BILINEAR, written as rows of one pixel (patch size 1), 3 channels zero-padded to 8 halfs
    ImageTower& t = c->tower;
    t.P = 1; t.G = c->S; t.NP = c->S * c->S; t.T = c->g[0] * c->g[0]; t.K = 3; t.Kpad = 8; t.edge = t.crop = c->S; t.rescale = cfg->rescale_factor;
    std::copy(cfg->image_mean, cfg->image_mean + 3, t.mean); std::copy(cfg->image_std, cfg->image_std + 3, t.stdv);
    t.plans.filter = image_front_end::PIL_BILINEAR;
    build_manifest(c);
    *out = c;
    return CS_OK;
}

void cs_seg_destroy(CsSeg* c) {
    if (!c) return;
    c->tower.free_device();
    delete c;
}

int cs_seg_num_weights(const CsSeg* c) { return c ? c->tower.weights.count() : 0; }

const char* cs_seg_weight_name(const CsSeg* c, int i, int64_t* shape4, int* ndim) { return c ? c->tower.weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_seg_set_weight(CsSeg* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    static const int64_t scalar[1] = {1};
    return image_tower::set_weight(tower_of(c), name, data, ndim == 0 && !shape ? scalar : shape, ndim);          // (a 0-d tensor has no shape to point at)
}

int cs_seg_finalize(CsSeg* c) { return image_tower::finalize(NAMES, tower_of(c), [&] { return pack(c); }); }

int cs_seg_patch_cols(const CsSeg* c) { return c ? c->tower.Kpad : 0; }
int cs_seg_num_tokens(const CsSeg* c) { return c ? c->tower.T : 0; }

size_t cs_seg_workspace_bytes(const CsSeg* c, int batch) {
    if (!c || batch <= 0) return 0;
    return layout(c, (size_t)batch).total * sizeof(f16) + 4096;
}

double cs_seg_flops(const CsSeg* c, int batch) {
    if (!c) return 0;
    double f = 0;
    for (int i = 0; i < 4; ++i) {
        const double R = (double)c->g[i] * c->g[i], C = c->C[i], I = C * c->mlp, Nk = c->nk[i], sr = c->cfg.sr_ratios[i];
        f += 2.0 * R * (i ? 9.0 * c->C[i - 1] : 147.0) * C;
        double b = 2.0 * R * C * C * 2 + 2.0 * Nk * C * 2 * C + 4.0 * R * Nk * C + 4.0 * R * C * I + 2.0 * 9 * R * I;
        if (sr > 1) b += 2.0 * Nk * sr * sr * C * C;
        f += c->cfg.depths[i] * b + 2.0 * R * C * c->Dd;
    }
    const double R0 = (double)c->g[0] * c->g[0];
    f += 2.0 * R0 * 4 * c->Dd * c->Dd + 2.0 * R0 * c->Dd * c->NL;
    return f * batch;
}

size_t cs_seg_preprocess_workspace_bytes(const CsSeg* c, int batch, int height, int width) {
    return image_tower::preprocess_workspace_bytes(tower_of(c), batch, height, width);
}

int cs_seg_preprocess(CsSeg* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (c && batch >= 0 && height != width)
        CS_FAIL(CS_E_UNSUPPORTED, "segformer: %d x %d image: this entry point takes square inputs only; cs_seg_preprocess_hw stretches any image to %d x %d", height, width,
                c->S, c->S);
    return image_tower::preprocess(NAMES, tower_of(c), images, dtype, batch, height, width, patches, crop_u8, workspace, workspace_bytes, stream);
}

// the processor stretches every image to S x S (both axes on their own scale), so the output is the square one's and the plan is all that differs
int cs_seg_preprocess_hw(CsSeg* c, const void* images, int dtype, int batch, int height, int width, int* out_h, int* out_w, void* patches, unsigned char* crop_u8,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (c && out_h) *out_h = c->S;
    if (c && out_w) *out_w = c->S;
    const image_front_end::Plan* pl = nullptr;
    const int rc = image_tower::begin_preprocess_hw(NAMES, tower_of(c), images, batch, height, width, c ? c->S : 0, c ? c->S : 0, patches, workspace, workspace_bytes, &pl);
    if (!pl) return rc;
    const ImageTower& t = c->tower;
    return launch_vit_front_end(images, dtype, batch, height, width, pl->dev, t.mean, t.stdv, t.rescale, t.P, t.G, t.Kpad, (unsigned char*)workspace, (f16*)patches,
                                crop_u8, (hipStream_t)stream);
}

int cs_seg_forward(CsSeg* c, const void* patches, int batch, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    bool run = false;
    int rc = image_tower::begin_forward(NAMES, tower_of(c), batch, patches && workspace, workspace_bytes, cs_seg_workspace_bytes(c, batch), &run);
    if (!run) return rc;
    const int B = batch, Dd = c->Dd, mlp = c->mlp;
    const long r0 = (long)B * c->g[0] * c->g[0];
    if (r0 > 0x7fffffffL / std::max(std::max(4 * Dd, PE_K), std::max(c->NLp, c->C[0] * mlp)) || (long)B * c->S * c->S > 0x7fffffffL / 8 || B > 65535)
        CS_FAIL(CS_E_SHAPE, "segformer: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const Layout L = layout(c, (size_t)B);
    f16* base = (f16*)workspace;
    f16 *X = base + L.x, *N = base + L.n, *Q = base + L.q, *A = base + L.a, *P = base + L.p, *R = base + L.r, *KN = base + L.kn, *KV = base + L.kv;
    f16 *H1 = base + L.h1, *H2 = base + L.h2, *PJ = base + L.pj, *CAT = base + L.cat, *LG = base + L.lg;
    f16* F[4] = {base + L.f[0], base + L.f[1], base + L.f[2], base + L.f[3]};

    for (int i = 0; i < std::min(4, c->parts) && rc == CS_OK; ++i) {
        const int C = c->C[i], I = C * mlp, g = c->g[i], sr = c->cfg.sr_ratios[i], heads = C / 64, nk = c->nk[i];
        const long rows = (long)B * g * g, krows = (long)B * nk;
        const Stage& st = c->st[i];
        // ---- overlapped patch embedding + LayerNorm ----
        if (i == 0) {
            rc = launch_seg_im2col((const f16*)patches, B, c->S, c->S, 8, 3, 7, 4, 3, PE_K, P, s);
            if (rc == CS_OK) rc = lin(P, rows, PE_K, st.pe, C, nullptr, Q, s);
        } else {
            IgemmArgs a{};
            a.a0 = F[i - 1]; a.c0 = c->C[i - 1]; a.B = B; a.Hi = c->g[i - 1]; a.Wi = c->g[i - 1]; a.Ho = g; a.Wo = g; a.taps = 9; a.stride = 2; a.N = C;
            a.w = st.pe.w; a.bias = st.pe.b; a.out = Q;
            rc = launch_igemm(a, s);
        }
        if (rc == CS_OK) rc = launch_layer_norm(Q, st.peln.w, st.peln.b, X, (int)rows, C, LN_EPS, s);
        // ---- blocks ----
        for (size_t l = 0; l < st.blocks.size() && rc == CS_OK; ++l) {
            const Block& b = st.blocks[l];
            rc = launch_layer_norm(X, b.ln1.w, b.ln1.b, N, (int)rows, C, LN_EPS, s);
            if (rc == CS_OK) rc = lin(N, rows, C, b.q, C, nullptr, Q, s);
            const f16* kin = N;
            if (sr > 1) {
                if (rc == CS_OK) rc = launch_seg_patchify(N, B, g, g, C, sr, P, s);
                if (rc == CS_OK) rc = lin(P, krows, sr * sr * C, b.sr, C, nullptr, R, s);
                if (rc == CS_OK) rc = launch_layer_norm(R, b.srln.w, b.srln.b, KN, (int)krows, C, LN_EPS, s);
                kin = KN;
            }
            if (rc == CS_OK) rc = linear(kin, (int)krows, C, b.kv.w, b.kv.b, 2 * C, nullptr, KV, s);
            if (rc == CS_OK) {
                AttnArgs a{};
                a.q = Q; a.q_stride = C; a.k = KV; a.k_stride = 2 * C; a.v = KV + C; a.v_stride = 2 * C; a.out = A; a.out_stride = C;
                a.B = B; a.H = heads; a.Nq = g * g; a.Nk = nk; a.dh = 64; a.scale = 0.125f;
                rc = launch_attention(a, s);
            }
            if (rc == CS_OK) rc = lin(A, rows, C, b.o, C, X, X, s);
            if (rc == CS_OK) rc = launch_layer_norm(X, b.ln2.w, b.ln2.b, N, (int)rows, C, LN_EPS, s);
            if (rc == CS_OK) rc = linear(N, (int)rows, C, b.fc1.w, b.fc1.b, I, nullptr, H1, s);
            if (rc == CS_OK) rc = launch_seg_dwconv_gelu(H1, B, g, g, I, b.dw.w, b.dw.b, H2, s);
            if (rc == CS_OK) rc = lin(H2, rows, I, b.fc2, C, X, X, s);
        }
        if (rc == CS_OK) rc = launch_layer_norm(X, st.ln.w, st.ln.b, F[i], (int)rows, C, LN_EPS, s);
    }
    if (c->parts < 5) return rc;
    // ---- all-MLP head: per-stage projection, resize into the concat (stage 4 first), fuse (+ BatchNorm) + ReLU, classifier ----
    for (int i = 0; i < 4 && rc == CS_OK; ++i) {
        rc = linear(F[i], (int)((long)B * c->g[i] * c->g[i]), c->C[i], c->proj[i].w, c->proj[i].b, Dd, nullptr, PJ, s);
        if (rc == CS_OK) rc = launch_seg_bilinear(PJ, B, c->g[i], c->g[i], Dd, c->g[0], c->g[0], CAT, 4L * Dd, (3 - i) * Dd, s);
    }
    if (rc == CS_OK) rc = linear(CAT, (int)r0, 4 * Dd, c->fuse.w, c->fuse.b, Dd, nullptr, PJ, s);
    if (rc == CS_OK) rc = launch_seg_relu(PJ, r0 * Dd, s);
    if (rc == CS_OK) rc = linear(PJ, (int)r0, Dd, c->cls.w, c->cls.b, c->NLp, nullptr, LG, s);
    if (rc == CS_OK && logits) rc = launch_seg_logits(LG, B, (long)c->g[0] * c->g[0], c->NLp, c->NL, logits, s);
    return rc;
}

int cs_seg_set_stage_limit(CsSeg* c, int parts) {
    if (!c) CS_FAIL(CS_E_ARG, "segformer handle is NULL");
    if (parts < 1 || parts > 5) CS_FAIL(CS_E_ARG, "segformer: the stage limit is 1 .. 4 stages or 5 (with the head)");
    c->parts = parts;
    return CS_OK;
}

int cs_seg_masks(CsSeg* c, int batch, const void* workspace, size_t workspace_bytes, int* masks, void* stream) {
    bool run = false;
    const int rc = image_tower::begin_forward(NAMES, tower_of(c), batch, workspace && masks, workspace_bytes, cs_seg_workspace_bytes(c, batch), &run);
    if (!run) return rc;
    return launch_seg_argmax((const f16*)workspace + layout(c, (size_t)batch).lg, (long)batch * c->g[0] * c->g[0], c->NLp, c->NL, masks, (hipStream_t)stream);
}

int cs_seg_agreement(const int* pred, const int* target, int64_t target_stride, int batch, int64_t n, float* out, void* stream) {
    return launch_seg_agreement(pred, target, (long)target_stride, batch, (long)n, out, (hipStream_t)stream);
}

int cs_op_seg_dwconv_gelu(const void* x, int B, int H, int W, int C, const void* w, const void* bias, void* out, void* stream) {
    return launch_seg_dwconv_gelu((const f16*)x, B, H, W, C, (const f16*)w, (const f16*)bias, (f16*)out, (hipStream_t)stream);
}
int cs_op_seg_im2col(const void* x, int B, int H, int W, int Cs, int C, int k, int stride, int pad, int Kp, void* out, void* stream) {
    return launch_seg_im2col((const f16*)x, B, H, W, Cs, C, k, stride, pad, Kp, (f16*)out, (hipStream_t)stream);
}
int cs_op_seg_patchify(const void* x, int B, int H, int W, int C, int sr, void* out, void* stream) {
    return launch_seg_patchify((const f16*)x, B, H, W, C, sr, (f16*)out, (hipStream_t)stream);
}
int cs_op_seg_bilinear(const void* x, int B, int Hi, int Wi, int C, int Ho, int Wo, void* out, int64_t ld, int col, void* stream) {
    return launch_seg_bilinear((const f16*)x, B, Hi, Wi, C, Ho, Wo, (f16*)out, (long)ld, col, (hipStream_t)stream);
}
int cs_op_seg_argmax(const void* x, int64_t M, int64_t ld, int n, int* out, void* stream) {
    return launch_seg_argmax((const f16*)x, (long)M, (long)ld, n, out, (hipStream_t)stream);
}
int cs_op_seg_logits(const void* x, int B, int64_t HW, int64_t ld, int n, float* out, void* stream) {
    return launch_seg_logits((const f16*)x, B, (long)HW, (long)ld, n, out, (hipStream_t)stream);
}
int cs_op_seg_relu(void* x, int64_t n, void* stream) { return launch_seg_relu((f16*)x, (long)n, (hipStream_t)stream); }

}  // extern "C"
