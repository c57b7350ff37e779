// The Depth Anything handle and its forward at one patch grid, shared by depth.cpp (the square entry points: the training grid) and depth_hw.cpp (the `_hw`
// entry points: any gh x gw within the limits of consolver_hip.h).  Host only.  The forward is written once over a DepthGrid; the square call is its (G, G) case
// with the packed position table, so both paths launch the same kernels in the same order.
#pragma once
#include "image_tower.h"
#include "consolver_hip.h"

#include <map>
#include <utility>

namespace depth_model {
struct DConv { f16* w = nullptr; f16* b = nullptr; };
struct Fusion { DConv proj, r1c1, r1c2, r2c1, r2c2; };
constexpr int RK[4] = {4, 2, 1, 1};      // reassemble_factors 4, 2, 1, 0.5: the first two are transposed convs with kernel = stride, the last a stride-2 3x3 conv
constexpr size_t MAX_POS_TABLES = 16;    // interpolated position tables kept per handle (emptied when full, as image_front_end::PlanCache)
constexpr int MAX_SIDE_FACTOR = 3;       // a processed side is at most this many times the processor's size (CS_DEPTH_MAX_SIDE_FACTOR)
}  // namespace depth_model

struct CsDepth {
    CsDepthConfig cfg;
    ImageTower tower;                      // the DINOv2 backbone, its processor resizing to edge = crop = size: the whole image, no crop
    int S = 0, F = 0, HH = 0;              // image size, fusion / head widths
    int g[4] = {0, 0, 0, 0};               // sizes of the four reassembled maps: 4 G, 2 G, G, (G - 1) / 2 + 1
    int cp[4] = {0, 0, 0, 0};              // their channel counts as stored (neck_hidden_sizes padded)
    depth_model::DConv reasm[4];           // projection (folded with the transposed conv): [k k cp][D]
    depth_model::DConv down;               // reassemble layer 3's stride-2 3x3 conv [cp3][9][cp3]
    depth_model::DConv neck[4];            // neck.convs [F][9][cp]
    depth_model::Fusion fus[4];
    depth_model::DConv head1, head2, head3;
    float* pos_grid = nullptr;             // the trained position grid [G][G][D] in fp32 (in the weight store's allocations)
    std::map<std::pair<int, int>, f16*> pos_tables;      // per (gh, gw) other than the training grid: [1 + gh gw][D], at most MAX_POS_TABLES (depth_hw.cpp)
};

namespace depth_model {

// one call's geometry: the processed image, its patch grid, the four reassembled maps
struct DepthGrid {
    int oh, ow, gh, gw, NP, T;
    int mh[4], mw[4];
};
inline DepthGrid make_grid(const CsDepth* c, int out_h, int out_w) {
    DepthGrid g{};
    g.oh = out_h; g.ow = out_w; g.gh = out_h / c->tower.P; g.gw = out_w / c->tower.P; g.NP = g.gh * g.gw; g.T = g.NP + 1;
    g.mh[0] = 4 * g.gh; g.mh[1] = 2 * g.gh; g.mh[2] = g.gh; g.mh[3] = (g.gh - 1) / 2 + 1;
    g.mw[0] = 4 * g.gw; g.mw[1] = 2 * g.gw; g.mw[2] = g.gw; g.mw[3] = (g.gw - 1) / 2 + 1;
    return g;
}

// workspace carve-up (fp16 elements): the encoder stack | patch embeddings | normalised tap | reassemble GEMM output | reassembled map | map 3 after its
// stride-2 conv | the four neck features | three rotating buffers for the fusion stage and the head
struct Layout { size_t pe, tap, gemm, map, down, f[4], x, y, z, total; };
inline Layout layout(const CsDepth* c, const DepthGrid& g, size_t B) {
    const ImageTower& t = c->tower;
    const size_t D = t.D, rows = B * g.T, F = c->F;
    Layout L;
    L.pe = pre_ln_workspace_elems(rows, D, t.I);
    size_t o = L.pe + B * g.NP * D;           // ... with the patch embeddings
    L.tap = o; o += rows * D;
    size_t nmax = 0, mmax = 0;
    for (int i = 0; i < 4; ++i) {
        nmax = std::max(nmax, (size_t)RK[i] * RK[i] * c->cp[i]);
        mmax = std::max(mmax, (size_t)g.gh * RK[i] * g.gw * RK[i] * c->cp[i]);
    }
    L.gemm = o; o += rows * nmax;
    L.map = o; o += B * mmax;
    L.down = o; o += B * g.mh[3] * g.mw[3] * c->cp[3];
    for (int i = 0; i < 4; ++i) { L.f[i] = o; o += B * g.mh[i] * g.mw[i] * F; }
    const size_t big = std::max((size_t)4 * g.mh[0] * g.mw[0] * F, (size_t)g.oh * g.ow * std::max(F / 2, (size_t)c->HH));
    L.x = o; o += B * big; L.y = o; o += B * big; L.z = o; o += B * big;
    L.total = o;
    return L;
}
inline size_t workspace_bytes(const CsDepth* c, const DepthGrid& g, int batch) { return layout(c, g, (size_t)batch).total * sizeof(f16) + 4096; }

inline double flops(const CsDepth* c, const DepthGrid& g, int batch) {
    const ImageTower& t = c->tower;
    const double D = t.D, F = c->F, B = batch;
    double f = 2.0 * B * g.NP * (double)t.K * D + pre_ln_flops(c->cfg.out_indices[3], batch, g.T, t.D, t.I);
    for (int i = 0; i < 4; ++i) {
        const double px = (double)g.mh[i] * g.mw[i];
        f += 2.0 * B * g.T * D * RK[i] * RK[i] * c->cp[i];                                          // reassemble GEMM
        f += 2.0 * B * px * 9 * c->cp[i] * F;                                                 // neck conv
        const int lvl = 3 - i;                                                                // fusion layer `lvl` runs at this map's size
        const double nxt = i ? (double)g.mh[i - 1] * g.mw[i - 1] : 4.0 * px;
        f += (lvl ? 4 : 2) * 2.0 * B * px * 9 * F * F + 2.0 * B * nxt * F * F;
    }
    f += 2.0 * B * g.mh[3] * g.mw[3] * 9.0 * c->cp[3] * c->cp[3];                             // the stride-2 conv
    f += 2.0 * B * 4.0 * g.mh[0] * g.mw[0] * 9 * F * (F / 2) + 2.0 * B * g.oh * (double)g.ow * (9.0 * (F / 2) * c->HH + c->HH);
    return f;
}

// batch * (rows or pixels) * (the widest row any kernel of the call indexes) must fit an int
inline bool too_large(const CsDepth* c, const DepthGrid& g, int B) {
    const ImageTower& t = c->tower;
    return (long)B * g.T > 0x7fffffffL / std::max(std::max(t.I, 3 * t.D), 16 * c->cp[0]) || (long)B * g.oh * g.ow > 0x7fffffffL / 64;
}

// patches [B * NP][Kpad] -> predicted_depth [B][oh][ow] fp32 at grid g with position table pos [T][D]; the arguments are checked by the caller.
// shuffle(y, k, C, out): the pixel-shuffle store of the caller's grid (the square entry point and the _hw one name their own launcher)
template <typename Shuffle>
int forward(const CsDepth* c, const DepthGrid& g, const f16* pos, const void* patches, int B, float* predicted_depth, void* workspace, hipStream_t s, Shuffle shuffle) {
    const ImageTower& t = c->tower;
    const int D = t.D, I = t.I, H = t.heads, Tn = g.T, F = c->F;
    const Layout L = layout(c, g, (size_t)B);
    const long rows = (long)B * Tn;
    const PreLnWorkspace w = carve_pre_ln(workspace, rows, D, I);
    f16* base = (f16*)workspace;
    f16 *pe = base + L.pe, *tap = base + L.tap, *gemm = base + L.gemm, *map = base + L.map, *down = base + L.down;
    f16* f[4] = {base + L.f[0], base + L.f[1], base + L.f[2], base + L.f[3]};
    f16 *X = base + L.x, *Y = base + L.y, *Z = base + L.z;
    auto conv = [&](const f16* x, int h, int wd, int cin, const DConv& cv, int cout, int taps, int relu_in, int relu_out, const f16* res, const f16* res2, f16* out) {
        DptConvArgs a{};
        a.x = x; a.B = B; a.H = h; a.W = wd; a.Cin = cin; a.w = cv.w; a.bias = cv.b; a.Cout = cout; a.taps = taps;
        a.relu_in = relu_in; a.relu_out = relu_out; a.res = res; a.res2 = res2; a.out = out;
        return launch_dpt_conv(a, s);
    };
    // pre-activation residual unit: out = conv2(relu(conv1(relu(x)))) + x (+ skip); tmp holds the inner activation
    auto rcu = [&](const f16* x, int h, int wd, const DConv& c1, const DConv& c2, const f16* skip, f16* tmp, f16* out) {
        const int rc = conv(x, h, wd, F, c1, F, 9, 1, 0, nullptr, nullptr, tmp);
        return rc != CS_OK ? rc : conv(tmp, h, wd, F, c2, F, 9, 1, 0, x, skip, out);
    };

    // ---- backbone, tapped after out_indices[i] layers: final LayerNorm -> reassemble layer i -> neck conv i ----
    int rc = linear((const f16*)patches, B * g.NP, t.Kpad, t.wpatch, t.bpatch, D, nullptr, pe, s);
    if (rc == CS_OK) rc = launch_vit_tokens(pe, t.cls, pos, w.x, B, g.NP, D, s);
    size_t done = 0;
    for (int i = 0; i < 4 && rc == CS_OK; ++i) {
        const int k = RK[i], cp = c->cp[i];
        rc = run_pre_ln_layers(t.layers, w, B, Tn, D, I, H, t.eps, 0, launch_gelu_erf, s, done, (size_t)c->cfg.out_indices[i]);
        done = (size_t)c->cfg.out_indices[i];
        if (rc == CS_OK) rc = launch_layer_norm(w.x, t.lnfg, t.lnfb, tap, (int)rows, D, t.eps, s);
        if (rc == CS_OK) rc = linear(tap, (int)rows, D, c->reasm[i].w, c->reasm[i].b, k * k * cp, nullptr, gemm, s);
        if (rc == CS_OK) rc = shuffle(gemm, k, cp, map);                                            // drops the CLS rows
        const f16* src = map;
        if (i == 3 && rc == CS_OK) {
            IgemmArgs a{};
            a.a0 = map; a.c0 = cp; a.B = B; a.Hi = g.gh; a.Wi = g.gw; a.Ho = g.mh[3]; a.Wo = g.mw[3]; a.taps = 9; a.stride = 2; a.N = cp;
            a.w = c->down.w; a.bias = c->down.b; a.out = down;
            rc = launch_igemm(a, s);
            src = down;
        }
        if (rc == CS_OK) rc = conv(src, g.mh[i], g.mw[i], cp, c->neck[i], F, 9, 0, 0, nullptr, nullptr, f[i]);
    }
    // ---- fusion stage, coarse to fine: X holds the fused state ----
    for (int l = 0; l < 4 && rc == CS_OK; ++l) {
        const int i = 3 - l, h = g.mh[i], wd = g.mw[i], nh = i ? g.mh[i - 1] : 2 * h, nw = i ? g.mw[i - 1] : 2 * wd;
        const Fusion& fu = c->fus[l];
        const f16* hs = f[i];
        if (l) { rc = rcu(f[i], h, wd, fu.r1c1, fu.r1c2, X, Y, Z); hs = Z; }                       // Z = fused + residual_layer1(feature)
        if (rc == CS_OK) rc = rcu(hs, h, wd, fu.r2c1, fu.r2c2, nullptr, Y, X);                      // X = residual_layer2(h)
        if (rc == CS_OK) rc = launch_dpt_bilinear(X, B, h, wd, F, nh, nw, Y, s);
        if (rc == CS_OK) rc = conv(Y, nh, nw, F, fu.proj, F, 1, 0, 0, nullptr, nullptr, X);
    }
    // ---- head ----
    const int uh = 2 * g.mh[0], uw = 2 * g.mw[0];
    if (rc == CS_OK) rc = conv(X, uh, uw, F, c->head1, F / 2, 9, 0, 0, nullptr, nullptr, Y);
    if (rc == CS_OK) rc = launch_dpt_bilinear(Y, B, uh, uw, F / 2, g.oh, g.ow, Z, s);
    if (rc == CS_OK) rc = conv(Z, g.oh, g.ow, F / 2, c->head2, c->HH, 9, 0, 1, nullptr, nullptr, Y);
    if (rc == CS_OK) rc = launch_dpt_head(Y, (long)B * g.oh * g.ow, c->HH, c->head3.w, c->head3.b, c->cfg.max_depth, predicted_depth, s);
    return rc;
}

}  // namespace depth_model
