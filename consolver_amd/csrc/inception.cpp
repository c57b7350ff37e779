// Inception-v3 classifier logits: the features of the logit-cosine reward (reward_type "inception": edit_ppo/reward_model.py:98-108, 319-356).
//
// Replaces, for a batch of decoded images [B,3,H,W] in [0,1]:  ToPILImage -> Resize(size, BICUBIC) -> CenterCrop(size) -> ToTensor -> Normalize ->
// torchvision inception_v3(aux_logits=True, transform_input=False).eval() -> the [B, 1000] logits of fc (AuxLogits is never evaluated in eval mode; dropout is
// the identity).  The front end is the DINOv2 reward's (vit_ops.hip) with patch size 1 and rows of 8 halfs -- the normalised crop as NHWC-8 -- and
// torchvision's crop offset (image_front_end::CROP_ROUND_HALF_EVEN); non-square inputs are taken.  The network is the walk of incep_walk.h (the wiring, the
// BatchNorm fold and the conv packing, shared with the FID variant in fid.cpp) with torchvision's pools: every pool branch is the average pool that divides
// by 9.  On top of it: fc.weight -> fp16, fc.bias -> fp32.
#include "incep_walk.h"
#include "consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

using namespace incep_net;

struct CsIncep : Net {
    CsIncepConfig cfg;
    int NC = 0, last_hw = 0;
    f16* fcw = nullptr; float* fcb = nullptr;
    int parts = 5;                         // cs_incep_set_stage_limit: the forward stops after this many of (stem, Mixed_5, Mixed_6, Mixed_7, head); timing tools only
};

namespace {

const TowerNames NAMES = {"inception", "incep", "inception handle is NULL"};

// torchvision: F.avg_pool2d(x, 3, 1, 1) in every pool branch, Mixed_7c included
struct TorchvisionPools {
    static int avgpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) { return launch_incep_avgpool(x, B, H, W, C, out, s); }
    static int pool_7c(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) { return launch_incep_avgpool(x, B, H, W, C, out, s); }
};
using IncepWalk = Walk<TorchvisionPools>;

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
    IncepWalk w{c, PLAN};
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
        IncepWalk w{c, PACK};
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
    IncepWalk w{c, RUN};
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
