// The Inception-v3 network of the two handles that run it (inception.cpp: torchvision's classifier, the logit-cosine reward; fid.cpp: the FID variant with the
// 2015 graph's pooling rules and the pool3 output), stated once (host only).  The network is ONE walk that states the wiring once and is run in three modes:
// at create it registers the state-dict names, sizes the workspace buffers and counts the FLOPs; at finalize it folds and uploads the weights; in the
// forward it launches.  Every convolution runs on incep_conv_kernel (incep_ops.hip), each branch writing its column slice of the block's concatenated output.
// What differs between the two networks is a policy `Pools` of two launchers with launch_incep_avgpool's signature:
//   * Pools::avgpool  -- the 3x3 stride-1 pad-1 pool in front of branch_pool in Mixed_5b..5d, 6b..6e and 7b;
//   * Pools::pool_7c  -- the same place in Mixed_7c (torchvision: the same average pool; the FID variant: a max pool).
// A translation unit links only the launchers its own policy names.  Packing, in double with one rounding:
//   * conv [co][ci][kh][kw] -> [co][kh kw][ci8] (ci8 = ci rounded up to 8: the first layer's 3 channels), scaled by gamma / sqrt(var + 1e-3) -> fp16;
//   * bias = beta - mean gamma / sqrt(var + 1e-3) -> fp32.
#pragma once
#include "image_tower.h"

namespace incep_net {

constexpr double BN_EPS = 1e-3;
struct ConvW { f16* w = nullptr; float* b = nullptr; };
struct Ten { int buf, H, W, C; };              // a dense NHWC tensor in workspace buffer `buf`
enum { BUF_IN = -1, BUF_A = 0, BUF_B, BUF_T0, BUF_T1, NBUF };
enum Mode { PLAN, PACK, RUN };

// what a handle holds of the network; a handle derives from it and adds its config and its head
struct Net {
    ImageTower tower;                      // the front end (plans, processor constants) and the weight store; the encoder fields are unused
    int S = 0;                             // input edge
    size_t need[NBUF] = {0, 0, 0, 0};      // fp16 elements per image of every workspace buffer
    double flops1 = 0;                     // per image
    std::vector<ConvW> convs;              // in walk order
};

// one pass over the network in a mode
template <typename Pools>
struct Walk {
    Net* c; Mode mode;
    int B = 0; const f16* input = nullptr; f16* bufs[NBUF] = {nullptr, nullptr, nullptr, nullptr}; hipStream_t s = nullptr;
    size_t next = 0;                       // index into c->convs
    int rc = CS_OK; bool ok = true;

    const f16* ptr(const Ten& t) const { return t.buf == BUF_IN ? input : bufs[t.buf]; }

    // BasicConv2d `name` over x into the columns col .. col + cout of the [.., ld] tensor in buffer dst; returns the output's grid
    Ten conv(const Ten& x, const std::string& name, int cout, int kh, int kw, int stride, int ph, int pw, int dst, int ld, int col) {
        const int Ho = incep_out_size(x.H, kh, stride, ph), Wo = incep_out_size(x.W, kw, stride, pw);
        const int creal = x.buf == BUF_IN ? 3 : x.C;
        const Ten out{dst, Ho, Wo, ld};
        if (mode == PLAN) {
            WeightManifest& m = c->tower.weights;
            m.expect(name + ".conv.weight", {cout, creal, kh, kw});
            for (const char* q : {".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"}) m.expect(name + q, {cout});
            m.expect(name + ".bn.num_batches_tracked", {});                 // in the state dict; eval mode never reads it
            c->need[dst] = std::max(c->need[dst], (size_t)Ho * Wo * ld);
            c->flops1 += 2.0 * Ho * Wo * (double)cout * creal * kh * kw;
            c->convs.emplace_back();
        } else if (mode == PACK) {
            if (!ok) return out;
            WeightStore<float>& W = c->tower.weights;
            const auto &w = W.at(name + ".conv.weight").data, &g = W.at(name + ".bn.weight").data, &be = W.at(name + ".bn.bias").data;
            const auto &mu = W.at(name + ".bn.running_mean").data, &var = W.at(name + ".bn.running_var").data;
            const int taps = kh * kw, ci = x.C;
            std::vector<float> wp((size_t)cout * taps * ci, 0.f), bp(cout);
            for (int n = 0; n < cout; ++n) {
                const double sc = (double)g[n] / std::sqrt((double)var[n] + BN_EPS);
                for (int ch = 0; ch < creal; ++ch)
                    for (int k = 0; k < taps; ++k) wp[((size_t)n * taps + k) * ci + ch] = (float)(w[((size_t)n * creal + ch) * taps + k] * sc);
                bp[n] = (float)((double)be[n] - (double)mu[n] * sc);
            }
            ConvW& cw = c->convs[next];
            cw.w = W.upload(wp); cw.b = W.upload_f32(bp);
            ok = cw.w && cw.b;
        } else if (rc == CS_OK) {
            const ConvW& cw = c->convs[next];
            IncepConvArgs a{};
            a.x = ptr(x); a.B = B; a.H = x.H; a.W = x.W; a.Cin = x.C; a.creal = creal;
            a.w = cw.w; a.bias = cw.b; a.Cout = cout; a.kh = kh; a.kw = kw; a.stride = stride; a.pad_h = ph; a.pad_w = pw;
            a.out = bufs[dst]; a.ld = ld; a.col = col;
            rc = launch_incep_conv(a, s);
        }
        ++next;
        return out;
    }
    Ten conv1(const Ten& x, const std::string& name, int cout, int dst) { return conv(x, name, cout, 1, 1, 1, 0, 0, dst, cout, 0); }
    Ten maxpool(const Ten& x, int dst, int ld, int col) {
        const int Ho = (x.H - 3) / 2 + 1, Wo = (x.W - 3) / 2 + 1;
        if (mode == PLAN) c->need[dst] = std::max(c->need[dst], (size_t)Ho * Wo * ld);
        else if (mode == RUN && rc == CS_OK) rc = launch_incep_maxpool(ptr(x), B, x.H, x.W, x.C, bufs[dst], ld, col, s);
        return Ten{dst, Ho, Wo, ld};
    }
    // the 3x3 stride-1 pad-1 pool of a pool branch; last: Mixed_7c's
    Ten pool(const Ten& x, int dst, bool last = false) {
        if (mode == PLAN) c->need[dst] = std::max(c->need[dst], (size_t)x.H * x.W * x.C);
        else if (mode == RUN && rc == CS_OK)
            rc = last ? Pools::pool_7c(ptr(x), B, x.H, x.W, x.C, bufs[dst], s) : Pools::avgpool(ptr(x), B, x.H, x.W, x.C, bufs[dst], s);
        return Ten{dst, x.H, x.W, x.C};
    }
    static int other(int buf) { return buf == BUF_A ? BUF_B : BUF_A; }

    // torchvision's blocks; each reads x (buffer A or B) and writes its concatenation into the other one
    Ten inception_a(const Ten& x, const std::string& p, int pool_features) {
        const int o = other(x.buf), ld = 224 + pool_features;
        conv(x, p + ".branch1x1", 64, 1, 1, 1, 0, 0, o, ld, 0);
        Ten t = conv1(x, p + ".branch5x5_1", 48, BUF_T0);
        conv(t, p + ".branch5x5_2", 64, 5, 5, 1, 2, 2, o, ld, 64);
        t = conv1(x, p + ".branch3x3dbl_1", 64, BUF_T0);
        t = conv(t, p + ".branch3x3dbl_2", 96, 3, 3, 1, 1, 1, BUF_T1, 96, 0);
        conv(t, p + ".branch3x3dbl_3", 96, 3, 3, 1, 1, 1, o, ld, 128);
        t = pool(x, BUF_T0);
        return conv(t, p + ".branch_pool", pool_features, 1, 1, 1, 0, 0, o, ld, 224);
    }
    Ten inception_b(const Ten& x, const std::string& p) {
        const int o = other(x.buf), ld = 384 + 96 + x.C;
        conv(x, p + ".branch3x3", 384, 3, 3, 2, 0, 0, o, ld, 0);
        Ten t = conv1(x, p + ".branch3x3dbl_1", 64, BUF_T0);
        t = conv(t, p + ".branch3x3dbl_2", 96, 3, 3, 1, 1, 1, BUF_T1, 96, 0);
        conv(t, p + ".branch3x3dbl_3", 96, 3, 3, 2, 0, 0, o, ld, 384);
        return maxpool(x, o, ld, 480);
    }
    Ten inception_c(const Ten& x, const std::string& p, int c7) {
        const int o = other(x.buf), ld = 768;
        conv(x, p + ".branch1x1", 192, 1, 1, 1, 0, 0, o, ld, 0);
        Ten t = conv1(x, p + ".branch7x7_1", c7, BUF_T0);
        t = conv(t, p + ".branch7x7_2", c7, 1, 7, 1, 0, 3, BUF_T1, c7, 0);
        conv(t, p + ".branch7x7_3", 192, 7, 1, 1, 3, 0, o, ld, 192);
        t = conv1(x, p + ".branch7x7dbl_1", c7, BUF_T0);
        t = conv(t, p + ".branch7x7dbl_2", c7, 7, 1, 1, 3, 0, BUF_T1, c7, 0);
        t = conv(t, p + ".branch7x7dbl_3", c7, 1, 7, 1, 0, 3, BUF_T0, c7, 0);
        t = conv(t, p + ".branch7x7dbl_4", c7, 7, 1, 1, 3, 0, BUF_T1, c7, 0);
        conv(t, p + ".branch7x7dbl_5", 192, 1, 7, 1, 0, 3, o, ld, 384);
        t = pool(x, BUF_T0);
        return conv(t, p + ".branch_pool", 192, 1, 1, 1, 0, 0, o, ld, 576);
    }
    Ten inception_d(const Ten& x, const std::string& p) {
        const int o = other(x.buf), ld = 320 + 192 + x.C;
        Ten t = conv1(x, p + ".branch3x3_1", 192, BUF_T0);
        conv(t, p + ".branch3x3_2", 320, 3, 3, 2, 0, 0, o, ld, 0);
        t = conv1(x, p + ".branch7x7x3_1", 192, BUF_T0);
        t = conv(t, p + ".branch7x7x3_2", 192, 1, 7, 1, 0, 3, BUF_T1, 192, 0);
        t = conv(t, p + ".branch7x7x3_3", 192, 7, 1, 1, 3, 0, BUF_T0, 192, 0);
        conv(t, p + ".branch7x7x3_4", 192, 3, 3, 2, 0, 0, o, ld, 320);
        return maxpool(x, o, ld, 512);
    }
    Ten inception_e(const Ten& x, const std::string& p, bool last) {
        const int o = other(x.buf), ld = 2048;
        conv(x, p + ".branch1x1", 320, 1, 1, 1, 0, 0, o, ld, 0);
        Ten t = conv1(x, p + ".branch3x3_1", 384, BUF_T0);
        conv(t, p + ".branch3x3_2a", 384, 1, 3, 1, 0, 1, o, ld, 320);
        conv(t, p + ".branch3x3_2b", 384, 3, 1, 1, 1, 0, o, ld, 704);
        t = conv1(x, p + ".branch3x3dbl_1", 448, BUF_T0);
        t = conv(t, p + ".branch3x3dbl_2", 384, 3, 3, 1, 1, 1, BUF_T1, 384, 0);
        conv(t, p + ".branch3x3dbl_3a", 384, 1, 3, 1, 0, 1, o, ld, 1088);
        conv(t, p + ".branch3x3dbl_3b", 384, 3, 1, 1, 1, 0, o, ld, 1472);
        t = pool(x, BUF_T0, last);
        return conv(t, p + ".branch_pool", 192, 1, 1, 1, 0, 0, o, ld, 1856);
    }

    // the whole network up to the last grid [B][8][8][2048] (at 299); `parts`: stop after this many of (stem, Mixed_5, Mixed_6, Mixed_7)
    Ten run(int parts) {
        Ten t{BUF_IN, c->S, c->S, 8};
        t = conv(t, "Conv2d_1a_3x3", 32, 3, 3, 2, 0, 0, BUF_A, 32, 0);
        t = conv(t, "Conv2d_2a_3x3", 32, 3, 3, 1, 0, 0, BUF_B, 32, 0);
        t = conv(t, "Conv2d_2b_3x3", 64, 3, 3, 1, 1, 1, BUF_A, 64, 0);
        t = maxpool(t, BUF_B, 64, 0);
        t = conv(t, "Conv2d_3b_1x1", 80, 1, 1, 1, 0, 0, BUF_A, 80, 0);
        t = conv(t, "Conv2d_4a_3x3", 192, 3, 3, 1, 0, 0, BUF_B, 192, 0);
        t = maxpool(t, BUF_A, 192, 0);
        if (parts < 2) return t;
        t = inception_a(t, "Mixed_5b", 32);
        t = inception_a(t, "Mixed_5c", 64);
        t = inception_a(t, "Mixed_5d", 64);
        if (parts < 3) return t;
        t = inception_b(t, "Mixed_6a");
        t = inception_c(t, "Mixed_6b", 128);
        t = inception_c(t, "Mixed_6c", 160);
        t = inception_c(t, "Mixed_6d", 160);
        t = inception_c(t, "Mixed_6e", 192);
        if (parts < 4) return t;
        t = inception_d(t, "Mixed_7a");
        t = inception_e(t, "Mixed_7b", false);
        return inception_e(t, "Mixed_7c", true);
    }
};

// workspace carve-up (bytes): the four activation buffers, then the fp32 means [B][2048] of the last grid
struct Layout { size_t buf[NBUF], mean, total; };
inline Layout layout(const Net* c, size_t B) {
    Layout L;
    size_t o = 0;
    for (int i = 0; i < NBUF; ++i) { L.buf[i] = o; o += (B * c->need[i] * sizeof(f16) + 255) / 256 * 256; }
    L.mean = o; o += (B * 2048 * sizeof(float) + 255) / 256 * 256;
    L.total = o;
    return L;
}

}  // namespace incep_net
