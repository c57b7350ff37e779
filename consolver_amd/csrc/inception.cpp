// Inception-v3 classifier logits: the features of the logit-cosine reward (reward_type "inception": edit_ppo/reward_model.py:98-108, 319-356).
//
// Replaces, for a batch of decoded images [B,3,H,W] in [0,1]:  ToPILImage -> Resize(size, BICUBIC) -> CenterCrop(size) -> ToTensor -> Normalize ->
// torchvision inception_v3(aux_logits=True, transform_input=False).eval() -> the [B, 1000] logits of fc (AuxLogits is never evaluated in eval mode; dropout is
// the identity).  The front end is the DINOv2 reward's (vit_ops.hip) with patch size 1 and rows of 8 halfs -- the normalised crop as NHWC-8 -- and
// torchvision's crop offset (image_front_end::CROP_ROUND_HALF_EVEN); non-square inputs are taken.  The network is ONE walk (walk()) that states the wiring
// once and is run in three modes: at create it registers the state-dict names, sizes the workspace buffers and counts the FLOPs; at finalize it folds and
// uploads the weights; in the forward it launches.  Every convolution runs on incep_conv_kernel (incep_ops.hip), each branch writing its column slice of the
// block's concatenated output.  Packing, in double with one rounding:
//   * conv [co][ci][kh][kw] -> [co][kh kw][ci8] (ci8 = ci rounded up to 8: the first layer's 3 channels), scaled by gamma / sqrt(var + 1e-3) -> fp16;
//   * bias = beta - mean gamma / sqrt(var + 1e-3) -> fp32;
//   * fc.weight -> fp16, fc.bias -> fp32.
#include "image_tower.h"
#include "consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

namespace {
constexpr double BN_EPS = 1e-3;
struct ConvW { f16* w = nullptr; float* b = nullptr; };
struct Ten { int buf, H, W, C; };              // a dense NHWC tensor in workspace buffer `buf`
enum { BUF_IN = -1, BUF_A = 0, BUF_B, BUF_T0, BUF_T1, NBUF };
enum Mode { PLAN, PACK, RUN };
}  // namespace

struct CsIncep {
    CsIncepConfig cfg;
    ImageTower tower;                      // the front end (plans, processor constants) and the weight store; the encoder fields are unused
    int S = 0, NC = 0, last_hw = 0;
    size_t need[NBUF] = {0, 0, 0, 0};      // fp16 elements per image of every workspace buffer
    double flops1 = 0;                     // per image
    std::vector<ConvW> convs;              // in walk order
    f16* fcw = nullptr; float* fcb = nullptr;
    int parts = 5;                         // cs_incep_set_stage_limit: the forward stops after this many of (stem, Mixed_5, Mixed_6, Mixed_7, head); timing tools only
};

namespace {

const TowerNames NAMES = {"inception", "incep", "inception handle is NULL"};

// one pass over the network in a mode
struct Walk {
    CsIncep* c; Mode mode;
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
    Ten avgpool(const Ten& x, int dst) {
        if (mode == PLAN) c->need[dst] = std::max(c->need[dst], (size_t)x.H * x.W * x.C);
        else if (mode == RUN && rc == CS_OK) rc = launch_incep_avgpool(ptr(x), B, x.H, x.W, x.C, bufs[dst], s);
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
        t = avgpool(x, BUF_T0);
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
        t = avgpool(x, BUF_T0);
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
    Ten inception_e(const Ten& x, const std::string& p) {
        const int o = other(x.buf), ld = 2048;
        conv(x, p + ".branch1x1", 320, 1, 1, 1, 0, 0, o, ld, 0);
        Ten t = conv1(x, p + ".branch3x3_1", 384, BUF_T0);
        conv(t, p + ".branch3x3_2a", 384, 1, 3, 1, 0, 1, o, ld, 320);
        conv(t, p + ".branch3x3_2b", 384, 3, 1, 1, 1, 0, o, ld, 704);
        t = conv1(x, p + ".branch3x3dbl_1", 448, BUF_T0);
        t = conv(t, p + ".branch3x3dbl_2", 384, 3, 3, 1, 1, 1, BUF_T1, 384, 0);
        conv(t, p + ".branch3x3dbl_3a", 384, 1, 3, 1, 0, 1, o, ld, 1088);
        conv(t, p + ".branch3x3dbl_3b", 384, 3, 1, 1, 1, 0, o, ld, 1472);
        t = avgpool(x, BUF_T0);
        return conv(t, p + ".branch_pool", 192, 1, 1, 1, 0, 0, o, ld, 1856);
    }

    // the whole network up to the last grid [B][8][8][2048] (at 299); `parts` as in cs_incep_set_stage_limit
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
        t = inception_e(t, "Mixed_7b");
        return inception_e(t, "Mixed_7c");
    }
};

// workspace carve-up (bytes): the four activation buffers, then the head's fp32 means [B][2048]
struct Layout { size_t buf[NBUF], mean, total; };
Layout layout(const CsIncep* c, size_t B) {
    Layout L;
    size_t o = 0;
    for (int i = 0; i < NBUF; ++i) { L.buf[i] = o; o += (B * c->need[i] * sizeof(f16) + 255) / 256 * 256; }
    L.mean = o; o += (B * 2048 * sizeof(float) + 255) / 256 * 256;
    L.total = o;
    return L;
}

}  // namespace

extern "C" {

int cs_incep_create(const CsIncepConfig* cfg, CsIncep** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    // 75: the smallest image whose last grid is 1 x 1 (75 -> 37, 35, 35, 17, 17, 15, 7 | 7 | 3 | 1)
    if (cfg->image_size < 75 || cfg->image_size > 2048) CS_FAIL(CS_E_SHAPE, "inception: image_size %d must be 75 .. 2048", cfg->image_size);
    if (cfg->num_classes < 1 || cfg->num_classes > 65536) CS_FAIL(CS_E_ARG, "inception: bad config");
    const int rc = image_tower::check_image_std(NAMES.who, cfg->image_std);
    if (rc != CS_OK) return rc;
    CsIncep* c = new CsIncep();
    c->cfg = *cfg;
    c->S = cfg->image_size; c->NC = cfg->num_classes;
    Walk w{c, PLAN};
    const Ten last = w.run(5);
    c->last_hw = last.H * last.W;
    c->tower.weights.expect("fc.weight", {c->NC, 2048});
    c->tower.weights.expect("fc.bias", {c->NC});
    c->flops1 += 2.0 * 2048 * c->NC;
    // the front end: shortest edge -> S (PIL BICUBIC), torchvision's center crop S x S, written as rows of one pixel (patch size 1), 3 channels zero-padded to 8 halfs
    ImageTower& t = c->tower;
    t.P = 1; t.G = c->S; t.NP = c->S * c->S; t.T = c->last_hw; t.K = 3; t.Kpad = 8; t.edge = t.crop = c->S; t.rescale = cfg->rescale_factor;
    std::copy(cfg->image_mean, cfg->image_mean + 3, t.mean); std::copy(cfg->image_std, cfg->image_std + 3, t.stdv);
    t.plans.filter = image_front_end::PIL_BICUBIC;
    t.plans.crop_rule = image_front_end::CROP_ROUND_HALF_EVEN;
    *out = c;
    return CS_OK;
}

void cs_incep_destroy(CsIncep* c) {
    if (!c) return;
    c->tower.free_device();
    delete c;
}

int cs_incep_num_weights(const CsIncep* c) { return c ? c->tower.weights.count() : 0; }

const char* cs_incep_weight_name(const CsIncep* c, int i, int64_t* shape4, int* ndim) { return c ? c->tower.weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_incep_set_weight(CsIncep* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    static const int64_t scalar[1] = {1};
    if (c && name && std::string(name).rfind("AuxLogits.", 0) == 0) return CS_OK;                                 // in a real checkpoint; eval mode never evaluates it
    return image_tower::set_weight(tower_of(c), name, data, ndim == 0 && !shape ? scalar : shape, ndim);          // (a 0-d tensor has no shape to point at)
}

int cs_incep_finalize(CsIncep* c) {
    return image_tower::finalize(NAMES, tower_of(c), [&] {
        Walk w{c, PACK};
        w.run(5);
        if (!w.ok) return false;
        WeightStore<float>& W = c->tower.weights;
        c->fcw = W.upload(W.at("fc.weight").data); c->fcb = W.upload_f32(W.at("fc.bias").data);
        return c->fcw && c->fcb;
    });
}

int cs_incep_patch_cols(const CsIncep* c) { return c ? c->tower.Kpad : 0; }
int cs_incep_num_tokens(const CsIncep* c) { return c ? c->tower.T : 0; }

size_t cs_incep_workspace_bytes(const CsIncep* c, int batch) {
    if (!c || batch <= 0) return 0;
    return layout(c, (size_t)batch).total + 4096;
}

double cs_incep_flops(const CsIncep* c, int batch) { return c ? c->flops1 * batch : 0; }

size_t cs_incep_preprocess_workspace_bytes(const CsIncep* c, int batch, int height, int width) {
    return image_tower::preprocess_workspace_bytes(tower_of(c), batch, height, width);
}

int cs_incep_preprocess(CsIncep* c, const void* images, int dtype, int batch, int height, int width, void* patches, unsigned char* crop_u8,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return image_tower::preprocess(NAMES, tower_of(c), images, dtype, batch, height, width, patches, crop_u8, workspace, workspace_bytes, stream);
}

int cs_incep_forward(CsIncep* c, const void* patches, int batch, float* logits, void* workspace, size_t workspace_bytes, void* stream) {
    bool run = false;
    const int rc = image_tower::begin_forward(NAMES, tower_of(c), batch, patches && workspace && logits, workspace_bytes, cs_incep_workspace_bytes(c, batch), &run);
    if (!run) return rc;
    if (batch > 0x7fffffffL / ((long)c->S * c->S)) CS_FAIL(CS_E_SHAPE, "inception: batch too large for one call");
    const Layout L = layout(c, (size_t)batch);
    Walk w{c, RUN};
    w.B = batch; w.input = (const f16*)patches; w.s = (hipStream_t)stream;
    for (int i = 0; i < NBUF; ++i) w.bufs[i] = (f16*)((char*)workspace + L.buf[i]);
    const Ten last = w.run(c->parts);
    if (w.rc != CS_OK || c->parts < 5) return w.rc;
    return launch_incep_head(w.ptr(last), batch, (long)last.H * last.W, last.C, c->fcw, c->fcb, c->NC, (float*)((char*)workspace + L.mean), logits, w.s);
}

int cs_incep_set_stage_limit(CsIncep* c, int parts) {
    if (!c) CS_FAIL(CS_E_ARG, "inception handle is NULL");
    if (parts < 1 || parts > 5) CS_FAIL(CS_E_ARG, "inception: the stage limit is 1 .. 4 stages or 5 (with the head)");
    c->parts = parts;
    return CS_OK;
}

int cs_op_incep_conv(const void* x, int B, int H, int W, int Cin, int Creal, const void* w, const float* bias, int Cout, int KH, int KW, int stride,
                     int pad_h, int pad_w, void* out, int64_t ld, int col, void* stream) {
    IncepConvArgs a{};
    a.x = (const f16*)x; a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.creal = Creal; a.w = (const f16*)w; a.bias = bias; a.Cout = Cout; a.kh = KH; a.kw = KW;
    a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w; a.out = (f16*)out; a.ld = (long)ld; a.col = col;
    return launch_incep_conv(a, (hipStream_t)stream);
}
int cs_op_incep_maxpool(const void* x, int B, int H, int W, int C, void* out, int64_t ld, int col, void* stream) {
    return launch_incep_maxpool((const f16*)x, B, H, W, C, (f16*)out, (long)ld, col, (hipStream_t)stream);
}
int cs_op_incep_avgpool(const void* x, int B, int H, int W, int C, void* out, void* stream) {
    return launch_incep_avgpool((const f16*)x, B, H, W, C, (f16*)out, (hipStream_t)stream);
}
int cs_op_incep_head(const void* x, int B, int64_t HW, int C, const void* w, const float* bias, int N, float* mean, float* logits, void* stream) {
    return launch_incep_head((const f16*)x, B, (long)HW, C, (const f16*)w, bias, N, mean, logits, (hipStream_t)stream);
}

}  // extern "C"
