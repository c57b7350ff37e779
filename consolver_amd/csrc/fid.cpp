// FID: the pool3 features of the FID variant of Inception-v3 behind clean-fid's resize, and the fp64 feature statistics (the reference's fid_test.py:
// cleanfid.fid.compute_fid(generated_dir, "coco/val2017")).
//
// The network is the walk of incep_walk.h -- the same 94 BatchNorm-folded convolutions on incep_conv_kernel under the same torchvision state-dict names, which
// is the naming of pytorch-fid's pt_inception-2015-12-05 checkpoint -- with the 2015 TF graph's pooling rules (fid_ops.hip): every 3x3 average pool of a pool
// branch divides by the taps inside the image, Mixed_7c's pool branch is a max pool.  The output is the global mean of the last 8 x 8 x 2048 grid in fp32; fc
// is not evaluated and is not in the manifest ("fc.*", 1008 classes in that checkpoint, and "AuxLogits.*" are accepted and ignored).  The input is 299 x 299.
// The front end is PIL's mode-"F" bicubic resize straight to 299 x 299 on its own plan of the plan cache (image_front_end.h, get_float_plan).
#include "incep_walk.h"
#include "consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

using namespace incep_net;

struct CsFid : Net {
    CsFidConfig cfg;
    int last_hw = 0;
};

namespace {

constexpr int FID_SIZE = 299;
const TowerNames NAMES = {"fid", "fid", "fid handle is NULL"};

// the 2015 graph: count_include_pad = False in every average pool, a max pool in Mixed_7c
struct FidPools {
    static int avgpool(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) { return launch_fid_avgpool(x, B, H, W, C, out, s); }
    static int pool_7c(const f16* x, int B, int H, int W, int C, f16* out, hipStream_t s) { return launch_fid_maxpool(x, B, H, W, C, out, s); }
};
using FidWalk = Walk<FidPools>;

bool ignored_weight(const char* name) {
    const std::string n(name);
    return n.rfind("AuxLogits.", 0) == 0 || n.rfind("fc.", 0) == 0;
}

}  // namespace

extern "C" {

int cs_fid_create(const CsFidConfig* cfg, CsFid** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    const int rc = image_tower::check_image_std(NAMES.who, cfg->image_std);
    if (rc != CS_OK) return rc;
    CsFid* c = new CsFid();
    c->cfg = *cfg;
    c->S = FID_SIZE;
    FidWalk w{c, PLAN};
    const Ten last = w.run(4);
    c->last_hw = last.H * last.W;
    // the front end's constants: rows of one pixel, 3 channels zero-padded to 8 halfs; mean / std on the 0 .. 255 scale
    ImageTower& t = c->tower;
    t.P = 1; t.G = c->S; t.NP = c->S * c->S; t.T = c->last_hw; t.K = 3; t.Kpad = 8; t.edge = t.crop = c->S; t.rescale = 1.0;
    std::copy(cfg->image_mean, cfg->image_mean + 3, t.mean); std::copy(cfg->image_std, cfg->image_std + 3, t.stdv);
    *out = c;
    return CS_OK;
}

void cs_fid_destroy(CsFid* c) {
    if (!c) return;
    c->tower.free_device();
    delete c;
}

int cs_fid_num_weights(const CsFid* c) { return c ? c->tower.weights.count() : 0; }

const char* cs_fid_weight_name(const CsFid* c, int i, int64_t* shape4, int* ndim) { return c ? c->tower.weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_fid_set_weight(CsFid* c, const char* name, const float* data, const int64_t* shape, int ndim) {
    static const int64_t scalar[1] = {1};
    if (c && name && ignored_weight(name)) return CS_OK;                                                          // in the checkpoint; never evaluated
    return image_tower::set_weight(tower_of(c), name, data, ndim == 0 && !shape ? scalar : shape, ndim);          // (a 0-d tensor has no shape to point at)
}

int cs_fid_finalize(CsFid* c) {
    return image_tower::finalize(NAMES, tower_of(c), [&] {
        FidWalk w{c, PACK};
        w.run(4);
        return w.ok;
    });
}

int cs_fid_patch_cols(const CsFid* c) { return c ? c->tower.Kpad : 0; }
int cs_fid_num_tokens(const CsFid* c) { return c ? c->tower.T : 0; }

size_t cs_fid_workspace_bytes(const CsFid* c, int batch) {
    if (!c || batch <= 0) return 0;
    return layout(c, (size_t)batch).total + 4096;
}

double cs_fid_flops(const CsFid* c, int batch) { return c ? c->flops1 * batch : 0; }

size_t cs_fid_preprocess_workspace_bytes(const CsFid* c, int batch, int height, int width) {
    if (!c || batch <= 0 || height <= 0 || width <= 0) return 0;
    return (size_t)batch * 3 * height * FID_SIZE * sizeof(float) + 256;          // the horizontal pass: every input row x 299 columns, fp32
}

int cs_fid_preprocess(CsFid* c, const void* images, int dtype, int batch, int height, int width, void* patches, float* resized_f32, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "%s", NAMES.null_handle);
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    if (batch == 0) return CS_OK;
    if (!images || !patches || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    if (dtype != CS_U8 && dtype != CS_F16 && dtype != CS_F32) CS_FAIL(CS_E_DTYPE, "fid: images must be uint8, fp16 or fp32");
    if (height < 1 || width < 1) CS_FAIL(CS_E_SHAPE, "fid: bad image size %d x %d", height, width);
    if (batch > 0x7fffffffL / ((long)FID_SIZE * FID_SIZE)) CS_FAIL(CS_E_SHAPE, "fid: batch too large for one call");
    if (workspace_bytes < (size_t)batch * 3 * height * FID_SIZE * sizeof(float)) CS_FAIL(CS_E_ARG, "fid: preprocess workspace too small");
    const image_front_end::FloatPlan* pl = nullptr;
    const int rc = c->tower.plans.get_float_plan(NAMES.who, FID_SIZE, height, width, &pl);
    if (rc != CS_OK) return rc;
    return launch_fid_front_end(images, dtype, batch, height, width, pl->dev, c->tower.mean, c->tower.stdv, (float*)workspace, (f16*)patches, resized_f32,
                                (hipStream_t)stream);
}

int cs_fid_forward(CsFid* c, const void* patches, int batch, float* features, void* workspace, size_t workspace_bytes, void* stream) {
    bool run = false;
    const int rc = image_tower::begin_forward(NAMES, tower_of(c), batch, patches && workspace && features, workspace_bytes, cs_fid_workspace_bytes(c, batch), &run);
    if (!run) return rc;
    if (batch > 0x7fffffffL / ((long)c->S * c->S)) CS_FAIL(CS_E_SHAPE, "fid: batch too large for one call");
    const Layout L = layout(c, (size_t)batch);
    FidWalk w{c, RUN};
    w.B = batch; w.input = (const f16*)patches; w.s = (hipStream_t)stream;
    for (int i = 0; i < NBUF; ++i) w.bufs[i] = (f16*)((char*)workspace + L.buf[i]);
    const Ten last = w.run(4);
    if (w.rc != CS_OK) return w.rc;
    return launch_incep_mean(w.ptr(last), batch, (long)last.H * last.W, last.C, features, w.s);
}

int cs_fid_stats_accumulate(const float* feats, int64_t n, int d, double* sum, double* outer, void* stream) {
    if (!feats || !sum || !outer) CS_FAIL(CS_E_ARG, "fid stats: null pointer");
    if (d < 16 || d > 4096 || d % 16) CS_FAIL(CS_E_SHAPE, "fid stats: d = %d must be a multiple of 16 in 16 .. 4096", d);
    if (n < 1 || n > 0x7fffffffL) CS_FAIL(CS_E_SHAPE, "fid stats: n = %lld rows (1 .. 2^31 - 1 per call)", (long long)n);
    return launch_fid_stats_accumulate(feats, (long)n, d, sum, outer, (hipStream_t)stream);
}

int cs_fid_stats_finalize(const double* sum, const double* outer, int64_t n_total, int d, double* mu, double* sigma, void* stream) {
    if (!sum || !outer || !mu || !sigma) CS_FAIL(CS_E_ARG, "fid stats: null pointer");
    if (d < 16 || d > 4096 || d % 16) CS_FAIL(CS_E_SHAPE, "fid stats: d = %d must be a multiple of 16 in 16 .. 4096", d);
    if (n_total < 2) CS_FAIL(CS_E_SHAPE, "fid stats: the covariance needs N >= 2 (N = %lld)", (long long)n_total);
    return launch_fid_stats_finalize(sum, outer, (long)n_total, d, mu, sigma, (hipStream_t)stream);
}

int cs_op_fid_avgpool(const void* x, int B, int H, int W, int C, void* out, void* stream) {
    return launch_fid_avgpool((const f16*)x, B, H, W, C, (f16*)out, (hipStream_t)stream);
}
int cs_op_fid_maxpool(const void* x, int B, int H, int W, int C, void* out, void* stream) {
    return launch_fid_maxpool((const f16*)x, B, H, W, C, (f16*)out, (hipStream_t)stream);
}

}  // extern "C"
