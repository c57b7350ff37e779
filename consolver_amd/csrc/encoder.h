// The pre-LN transformer encoder of the CLIP text tower and the DINOv2 ViT, stated once (host only): per layer
//   LN -> fused QKV -> head-64 flash attention -> out-proj + residual -> LN -> fc1 -> activation -> fc2 + residual
// over token-major [rows = batch * tokens][D] fp16; every linear runs through the implicit-GEMM MFMA kernels.  The two models differ in the mask and the
// activation (CLIP: causal, quick-GELU; ViT: unmasked, erf-GELU) and in the ViT's LayerScale vectors, folded into out-proj / fc2 at pack time.
#pragma once
#include "weights.h"

struct PreLnLayer { f16 *ln1g, *ln1b, *wqkv, *bqkv, *wo, *bo, *ln2g, *ln2b, *w1, *b1, *w2, *b2; };
// one layer's tensor names without the ".weight" / ".bias" suffix
struct PreLnNames { std::string q, k, v, out, ln1, ln2, fc1, fc2; };

inline int linear(const f16* x, int M, int K, const f16* w, const f16* b, int N, const f16* res, f16* out, hipStream_t s) {
    IgemmArgs a{};
    a.a0 = x; a.c0 = K; a.B = 1; a.Hi = M; a.Wi = 1; a.Ho = M; a.Wo = 1; a.taps = 1; a.stride = 1; a.N = N; a.w = w; a.bias = b; a.res = res; a.out = out;
    return launch_igemm(a, s);
}

// rows of w [N][K] (a bias [N]: K = 1) times lambda[N]: LayerScale folded into the linear layer in front of it
template <typename E> std::vector<E> scale_rows(const std::vector<E>& w, const std::vector<E>& lam, int K) {
    std::vector<E> o(w.size());
    for (size_t i = 0; i < w.size(); ++i) o[i] = w[i] * lam[i / K];
    return o;
}

// q | k | v fused to one [3D, D] linear; scale1 / scale2 (null: none) are folded into out-proj / fc2 in the store's element type
template <typename E> bool pack_pre_ln_layer(WeightStore<E>& W, const PreLnNames& n, const std::vector<E>* scale1, const std::vector<E>* scale2, PreLnLayer& L) {
    std::vector<E> w, b;
    for (const std::string* q : {&n.q, &n.k, &n.v}) {
        const auto& tw = W.at(*q + ".weight").data; w.insert(w.end(), tw.begin(), tw.end());
        const auto& tb = W.at(*q + ".bias").data; b.insert(b.end(), tb.begin(), tb.end());
    }
    auto up = [&](const std::string& name, const std::vector<E>* lam) {
        const HostTensor<E>& t = W.at(name);
        return lam ? W.upload(scale_rows(t.data, *lam, t.shape.size() == 2 ? (int)t.shape[1] : 1)) : W.upload(t.data);
    };
    L.wqkv = W.upload(w); L.bqkv = W.upload(b);
    L.wo = up(n.out + ".weight", scale1); L.bo = up(n.out + ".bias", scale1);
    L.ln1g = up(n.ln1 + ".weight", nullptr); L.ln1b = up(n.ln1 + ".bias", nullptr);
    L.ln2g = up(n.ln2 + ".weight", nullptr); L.ln2b = up(n.ln2 + ".bias", nullptr);
    L.w1 = up(n.fc1 + ".weight", nullptr); L.b1 = up(n.fc1 + ".bias", nullptr);
    L.w2 = up(n.fc2 + ".weight", scale2); L.b2 = up(n.fc2 + ".bias", scale2);
    return L.wqkv && L.bqkv && L.wo && L.bo && L.ln1g && L.ln1b && L.ln2g && L.ln2b && L.w1 && L.b1 && L.w2 && L.b2;
}

// the stack's workspace: x | normed | qkv | mlp (the attention output reuses normed); a caller's own buffers follow at `end`
struct PreLnWorkspace { f16 *x, *n, *qkv, *h, *end; };
inline size_t pre_ln_workspace_elems(size_t rows, size_t D, size_t I) { return rows * (D + D + 3 * D + I); }
inline PreLnWorkspace carve_pre_ln(void* workspace, long rows, int D, int I) {
    PreLnWorkspace w;
    w.x = (f16*)workspace; w.n = w.x + rows * D; w.qkv = w.n + rows * D; w.h = w.qkv + rows * 3 * D; w.end = w.h + rows * I;
    return w;
}
inline double pre_ln_flops(int layers, int batch, int tokens, double D, double I) {
    const double rows = (double)batch * tokens;
    return layers * (2.0 * rows * D * (4 * D + 2 * I) + 4.0 * batch * (double)tokens * tokens * D);
}

// x [batch * tokens][D] in place through the layers first .. last - 1 (default: every layer; a caller that taps the hidden state between layers runs the stack in
// ranges); activation: launch_quick_gelu or launch_gelu_erf.  Returns the first code that is not CS_OK
inline int run_pre_ln_layers(const std::vector<PreLnLayer>& layers, const PreLnWorkspace& w, int batch, int tokens, int D, int I, int heads, float eps, int causal,
                             int (*activation)(f16*, long, hipStream_t), hipStream_t s, size_t first = 0, size_t last = (size_t)-1) {
    const long rows = (long)batch * tokens;
    f16 *x = w.x, *n = w.n, *qkv = w.qkv, *h = w.h;
    int rc = CS_OK;
    for (size_t l = first; l < std::min(last, layers.size()) && rc == CS_OK; ++l) {
        const PreLnLayer& L = layers[l];
        rc = launch_layer_norm(x, L.ln1g, L.ln1b, n, (int)rows, D, eps, s);
        if (rc == CS_OK) rc = linear(n, (int)rows, D, L.wqkv, L.bqkv, 3 * D, nullptr, qkv, s);
        if (rc == CS_OK) {
            AttnArgs a{};
            a.q = qkv; a.q_stride = 3 * D; a.k = qkv + D; a.k_stride = 3 * D; a.v = qkv + 2 * D; a.v_stride = 3 * D; a.out = n; a.out_stride = D;
            a.B = batch; a.H = heads; a.Nq = tokens; a.Nk = tokens; a.dh = 64; a.scale = 0.125f; a.causal = causal;
            rc = launch_attention(a, s);
        }
        if (rc == CS_OK) rc = linear(n, (int)rows, D, L.wo, L.bo, D, x, x, s);                          // (LayerScale folded;) + residual
        if (rc == CS_OK) rc = launch_layer_norm(x, L.ln2g, L.ln2b, n, (int)rows, D, eps, s);
        if (rc == CS_OK) rc = linear(n, (int)rows, D, L.w1, L.b1, I, nullptr, h, s);
        if (rc == CS_OK) rc = activation(h, rows * I, s);
        if (rc == CS_OK) rc = linear(h, (int)rows, I, L.w2, L.b2, D, x, x, s);                          // (LayerScale folded;) + residual
    }
    return rc;
}
