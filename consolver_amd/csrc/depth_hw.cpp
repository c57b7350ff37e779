// Depth Anything at the input's aspect ratio: the `_hw` entry points of the depth handle (depth.cpp holds the square ones and the packing; depth_model.h the
// handle and the forward both share).
//
//   * the size rule is the DPT processor's with keep_aspect_ratio and ensure_multiple_of = patch size: scale_h = S / H, scale_w = S / W, the one closer to 1 for
//     both axes, each side round-half-even(scale * side / P) * P -- in double, operation by operation as the processor's Python does it;
//   * the front end is PIL's two-pass fixed-point bicubic straight to out_h x out_w (image_front_end.h: get_plan_hw), written as patch rows of a gh x gw grid;
//   * the position table of a grid other than the training grid is interpolated ON THE DEVICE from the fp32 grid the handle keeps (vit_ops.hip:
//     launch_vit_pos_interp) on the first call at that grid, and kept; the training grid reads the packed table and launches nothing;
//   * the backbone, the neck and the head are depth_model::forward at (gh, gw).
// Limits (consolver_hip.h): each processed side is 1 patch .. CS_DEPTH_MAX_SIDE_FACTOR * size; beyond them every entry point answers CS_E_UNSUPPORTED before
// any allocation or launch.
#include "depth_model.h"
#include "../../include/consolver_hip_ops.h"

#include <cmath>

using depth_model::DepthGrid;

namespace {

const TowerNames NAMES = {"depth", "depth", "depth handle is NULL"};
constexpr int MAX_INPUT_SIDE = 16384;

// the processor's constrain_to_multiple_of with no bounds: Python's round() of a double is round-half-even, which nearbyint is in the default rounding mode
int constrain(double val, int multiple) { return (int)(std::nearbyint(val / multiple) * multiple); }

// 0 when the processed size is within the limits (then *oh, *ow are set), else an error code with the message set
int processed_size(const CsDepth* c, int H, int W, int* oh, int* ow) {
    if (H < 1 || W < 1 || H > MAX_INPUT_SIDE || W > MAX_INPUT_SIDE) CS_FAIL(CS_E_UNSUPPORTED, "depth: image size %d x %d is outside 1 .. %d", H, W, MAX_INPUT_SIDE);
    const int P = c->tower.P;
    double sh = (double)c->S / H, sw = (double)c->S / W;
    if (std::fabs(1 - sw) < std::fabs(1 - sh)) sh = sw; else sw = sh;          // scale as little as possible
    const double vh = sh * H, vw = sw * W, lim = (double)depth_model::MAX_SIDE_FACTOR * c->S;
    if (!(vh <= 2 * lim) || !(vw <= 2 * lim)) CS_FAIL(CS_E_UNSUPPORTED, "depth: a %d x %d image resizes to more than %d times the processor's size %d", H, W, depth_model::MAX_SIDE_FACTOR, c->S);
    const int h = constrain(vh, P), w = constrain(vw, P);
    if (h < P || w < P || h > lim || w > lim)
        CS_FAIL(CS_E_UNSUPPORTED, "depth: a %d x %d image resizes to %d x %d: each side must be %d .. %d (%d times the processor's size)", H, W, h, w, P, (int)lim,
                depth_model::MAX_SIDE_FACTOR);
    *oh = h; *ow = w;
    return CS_OK;
}

// a processed size handed back by the caller (cs_depth_forward_hw, cs_depth_normalized_maps_hw): whole patches within the limits
int check_processed(const CsDepth* c, int oh, int ow) {
    const int P = c->tower.P, lim = depth_model::MAX_SIDE_FACTOR * c->S;
    if (oh < P || ow < P || oh % P || ow % P || oh > lim || ow > lim)
        CS_FAIL(CS_E_UNSUPPORTED, "depth: processed size %d x %d: each side must be a multiple of the patch size %d within %d .. %d", oh, ow, P, P, lim);
    return CS_OK;
}

// the position table [1 + gh gw][D] of a grid: the packed one for the training grid, else the handle's cached interpolation (made on `s` on a miss; the call
// then waits for it, so that a later call on another stream may read the table).  *launched (optional): whether this call ran the kernel
int position_table(CsDepth* c, int gh, int gw, hipStream_t s, const f16** out, int* launched) {
    if (launched) *launched = 0;
    const ImageTower& t = c->tower;
    if (gh == t.G && gw == t.G) { *out = t.pos; return CS_OK; }
    auto it = c->pos_tables.find({gh, gw});
    if (it != c->pos_tables.end()) { *out = it->second; return CS_OK; }
    if (c->pos_tables.size() >= depth_model::MAX_POS_TABLES) {          // a full cache is emptied: hipFree waits for the kernels that still read a table
        for (auto& kv : c->pos_tables) CS_CHECK_HIP(hipFree(kv.second));
        c->pos_tables.clear();
    }
    f16* d = nullptr;
    CS_CHECK_HIP(hipMalloc((void**)&d, ((size_t)gh * gw + 1) * t.D * sizeof(f16)));
    int rc = launch_vit_pos_interp(c->pos_grid, t.G, gh, gw, t.D, d, s);
    if (rc == CS_OK && hipStreamSynchronize(s) != hipSuccess) { cs_set_error("depth: position table interpolation failed"); rc = CS_E_HIP; }
    if (rc != CS_OK) { (void)hipFree(d); return rc; }
    c->pos_tables[{gh, gw}] = d;
    if (launched) *launched = 1;
    *out = d;
    return CS_OK;
}

}  // namespace

extern "C" {

int cs_depth_processed_size(const CsDepth* c, int height, int width, int* out_h, int* out_w) {
    if (!c || !out_h || !out_w) CS_FAIL(CS_E_ARG, "depth: handle / out_h / out_w is NULL");
    return processed_size(c, height, width, out_h, out_w);
}

size_t cs_depth_preprocess_workspace_bytes_hw(const CsDepth* c, int batch, int height, int width) {
    int oh = 0, ow = 0;
    if (!c || batch <= 0 || processed_size(c, height, width, &oh, &ow) != CS_OK) return 0;
    return image_tower::preprocess_hw_workspace_bytes(batch, height, ow);
}

int cs_depth_preprocess_hw(CsDepth* c, const void* images, int dtype, int batch, int height, int width, int* out_h, int* out_w, void* patches, unsigned char* crop_u8,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "depth handle is NULL");
    if (batch < 0) CS_FAIL(CS_E_ARG, "negative size");
    int oh = 0, ow = 0;
    int rc = processed_size(c, height, width, &oh, &ow);          // (in front of the empty batch's return, as the square entry point's refusal)
    if (rc != CS_OK) return rc;
    if (out_h) *out_h = oh;
    if (out_w) *out_w = ow;
    const image_front_end::Plan* pl = nullptr;
    rc = image_tower::begin_preprocess_hw(NAMES, &c->tower, images, batch, height, width, oh, ow, patches, workspace, workspace_bytes, &pl);
    if (!pl) return rc;
    const ImageTower& t = c->tower;
    return launch_vit_front_end_hw(images, dtype, batch, height, width, pl->dev, t.mean, t.stdv, t.rescale, t.P, oh / t.P, ow / t.P, t.Kpad, (unsigned char*)workspace,
                                   (f16*)patches, crop_u8, (hipStream_t)stream);
}

size_t cs_depth_workspace_bytes_hw(const CsDepth* c, int batch, int out_h, int out_w) {
    if (!c || batch <= 0 || check_processed(c, out_h, out_w) != CS_OK) return 0;
    return depth_model::workspace_bytes(c, depth_model::make_grid(c, out_h, out_w), batch);
}

double cs_depth_flops_hw(const CsDepth* c, int batch, int out_h, int out_w) {
    if (!c || check_processed(c, out_h, out_w) != CS_OK) return 0;
    return depth_model::flops(c, depth_model::make_grid(c, out_h, out_w), batch);
}

int cs_depth_forward_hw(CsDepth* c, const void* patches, int batch, int out_h, int out_w, float* predicted_depth, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "depth handle is NULL");
    int rc = check_processed(c, out_h, out_w);
    if (rc != CS_OK) return rc;
    const DepthGrid g = depth_model::make_grid(c, out_h, out_w);
    bool run = false;
    rc = image_tower::begin_forward(NAMES, &c->tower, batch, patches && predicted_depth && workspace, workspace_bytes, batch > 0 ? depth_model::workspace_bytes(c, g, batch) : 0,
                                    &run);
    if (!run) return rc;
    if (depth_model::too_large(c, g, batch)) CS_FAIL(CS_E_SHAPE, "depth: batch too large for one call");
    hipStream_t s = (hipStream_t)stream;
    const f16* pos = nullptr;
    if ((rc = position_table(c, g.gh, g.gw, s, &pos, nullptr)) != CS_OK) return rc;
    return depth_model::forward(c, g, pos, patches, batch, predicted_depth, workspace, s,
                                [&](const f16* y, int k, int C, f16* out) { return launch_dpt_pixel_shuffle_hw(y, batch, g.gh, g.gw, k, C, 1, out, s); });
}

int cs_depth_normalized_maps_hw(CsDepth* c, const float* predicted_depth, int batch, int in_h, int in_w, int height, int width, float* maps, void* stream) {
    if (!c) CS_FAIL(CS_E_ARG, "depth handle is NULL");
    if (batch < 0 || height < 1 || width < 1 || in_h < 1 || in_w < 1) CS_FAIL(CS_E_ARG, "depth: bad size");
    if (batch == 0) return CS_OK;
    if (!predicted_depth || !maps) CS_FAIL(CS_E_ARG, "null pointer");
    int rc = launch_dpt_bicubic(predicted_depth, batch, in_h, in_w, height, width, maps, (hipStream_t)stream);
    if (rc == CS_OK) rc = launch_dpt_minmax_normalize(maps, batch, (long)height * width, (hipStream_t)stream);
    return rc;
}

int cs_depth_position_table(CsDepth* c, int gh, int gw, void* table, int* kernel_launched, void* stream) {
    if (!c || !table) CS_FAIL(CS_E_ARG, "depth: handle / table is NULL");
    if (!c->tower.weights.finalized) CS_FAIL(CS_E_STATE, "cs_depth_finalize has not been called");
    int rc = check_processed(c, gh * c->tower.P, gw * c->tower.P);
    if (rc != CS_OK) return rc;
    const f16* pos = nullptr;
    if ((rc = position_table(c, gh, gw, (hipStream_t)stream, &pos, kernel_launched)) != CS_OK) return rc;
    CS_CHECK_HIP(hipMemcpyAsync(table, pos, ((size_t)gh * gw + 1) * c->tower.D * sizeof(f16), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CS_OK;
}

int cs_op_dpt_pixel_shuffle_hw(const void* y, int B, int Gh, int Gw, int k, int C, int skip, void* out, void* stream) {
    return launch_dpt_pixel_shuffle_hw((const f16*)y, B, Gh, Gw, k, C, skip, (f16*)out, (hipStream_t)stream);
}
int cs_op_vit_pos_interp(const float* grid, int s, int gh, int gw, int D, void* table, void* stream) {
    return launch_vit_pos_interp(grid, s, gh, gw, D, (f16*)table, (hipStream_t)stream);
}

}  // extern "C"
