// The resize plans of the image front end (launch_vit_front_end), used through image_tower.h by the executors whose processor is "PIL bicubic resize to a
// shortest edge, center crop, rescale, normalise" (vit.cpp: DINOv2; clip_vision.cpp: CLIP; depth.cpp: Depth Anything, edge = crop = size).  Host only: PIL's tap tables for the crop window of one (height, width),
// built in double as ImagingResample does, uploaded once per size and kept in a bounded cache that the handle owns.
#pragma once
#include "ops.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

namespace image_front_end {

// one pass of PIL's ImagingResample (BICUBIC: Keys cubic a = -0.5, support 2 * max(scale, 1); BILINEAR: the triangle filter, support max(scale, 1)) for output
// indices win0 .. win0 + win: taps normalised in double, converted as int(+-0.5 + k 2^22)
enum Filter { PIL_BILINEAR = 2, PIL_BICUBIC = 3 };          // PIL.Image.Resampling values
// where the center crop's window starts in a resized side of n: transformers' (n - C) / 2, or torchvision's int(round((n - C) / 2.0)) with Python's
// round-half-to-even (they differ when n - C = 3 (mod 4): 39 -> 19 | 20)
enum CropRule { CROP_FLOOR = 0, CROP_ROUND_HALF_EVEN = 1 };
inline int crop_offset(int n, int C, CropRule rule) {
    const int d = n - C, k = d / 2;
    return (rule == CROP_ROUND_HALF_EVEN && (d & 1) && (k & 1)) ? k + 1 : k;
}
struct Taps { std::vector<int> lo, cnt, kk; int ksize; };
struct TapsF64 { std::vector<int> lo, cnt; std::vector<double> kk; int ksize; };      // the taps as precompute_coeffs leaves them: normalised, in double
inline double pil_cubic(double x) {
    const double a = -0.5;
    x = std::fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
inline double pil_triangle(double x) {
    x = std::fabs(x);
    return x < 1.0 ? 1.0 - x : 0.0;
}
inline TapsF64 pil_taps_f64(int in, int out, int win0, int win, Filter filter = PIL_BICUBIC) {
    TapsF64 t;
    const double scale = (double)in / out, fs = std::max(scale, 1.0), support = (filter == PIL_BILINEAR ? 1.0 : 2.0) * fs, ww = 1.0 / fs;
    t.ksize = (int)std::ceil(support) * 2 + 1;
    t.lo.resize(win); t.cnt.resize(win); t.kk.assign((size_t)win * t.ksize, 0.0);
    std::vector<double> w(t.ksize);
    for (int i = 0; i < win; ++i) {
        const double center = (win0 + i + 0.5) * scale;
        const int xmin = std::max((int)(center - support + 0.5), 0), n = std::min((int)(center + support + 0.5), in) - xmin;
        double tot = 0;
        for (int x = 0; x < n; ++x) {
            const double a = (x + xmin - center + 0.5) * ww;
            w[x] = filter == PIL_BILINEAR ? pil_triangle(a) : pil_cubic(a);
            tot += w[x];
        }
        for (int x = 0; x < n; ++x) t.kk[(size_t)i * t.ksize + x] = tot != 0.0 ? w[x] / tot : w[x];
        t.lo[i] = xmin; t.cnt[i] = n;
    }
    return t;
}
// the 8-bit path: the same taps converted as int(+-0.5 + k 2^22)
inline Taps pil_taps(int in, int out, int win0, int win, Filter filter = PIL_BICUBIC) {
    TapsF64 f = pil_taps_f64(in, out, win0, win, filter);
    Taps t;
    t.ksize = f.ksize; t.lo = std::move(f.lo); t.cnt = std::move(f.cnt); t.kk.resize(f.kk.size());
    for (size_t i = 0; i < f.kk.size(); ++i) {
        const double k = f.kk[i];
        t.kk[i] = k < 0 ? (int)(-0.5 + k * (1 << 22)) : (int)(0.5 + k * (1 << 22));
    }
    return t;
}
// one side of a mode-"F" resize to `out`: PIL runs no pass over a side that has the size already (the pixels are copied), stated as one tap of 1.0
inline TapsF64 pil_float_side(int in, int out) {
    if (in != out) return pil_taps_f64(in, out, 0, out, PIL_BICUBIC);
    TapsF64 t;
    t.ksize = 1; t.lo.resize(out); t.cnt.assign(out, 1); t.kk.assign(out, 1.0);
    for (int i = 0; i < out; ++i) t.lo[i] = i;
    return t;
}

struct Plan { VitResizePlan dev; };
struct FloatPlan { FidResizePlan dev; };

// resize tables per input (height, width), at most MAX_PLANS of them (a directory of many image sizes must not grow device memory without bound: when the
// cache is full it is emptied -- hipFree waits for the kernels that still read a table).  Like every handle here the owner serves one thread at a time, and the
// tables live on the device that is current when a size is first seen: callers run a handle on one device (the Python wrapper selects the tensor's).
struct PlanCache {
    static constexpr size_t MAX_PLANS = 16;
    Filter filter = PIL_BICUBIC;                            // the processor's resample (set once, before the first plan)
    CropRule crop_rule = CROP_FLOOR;                        // the processor's center-crop offset (set once, next to filter)
    std::map<std::pair<int, int>, Plan> plans;
    std::map<std::pair<int, int>, FloatPlan> float_plans;   // get_float_plan's; the bound and the allocations are shared with `plans`
    std::map<std::tuple<int, int, int, int>, Plan> hw_plans;   // get_plan_hw's, per (H, W, out_h, out_w); the same bound and allocations
    std::vector<void*> plan_allocs;

    // a full cache is emptied before a new table is allocated
    int make_room() {
        if (plans.size() + float_plans.size() + hw_plans.size() < MAX_PLANS) return CS_OK;
        for (void* q : plan_allocs) CS_CHECK_HIP(hipFree(q));
        plan_allocs.clear(); plans.clear(); float_plans.clear(); hw_plans.clear();
        return CS_OK;
    }

    // the plan of an H x W input for the processor (shortest edge `edge`, center crop C); `who` names the executor in error messages
    int get_plan(const char* who, int edge, int C, int H, int W, const Plan** out) {
        auto it = plans.find({H, W});
        if (it != plans.end()) { *out = &it->second; return CS_OK; }
        if (H < 1 || W < 1) CS_FAIL(CS_E_SHAPE, "%s: bad image size %d x %d", who, H, W);
        // the processor's output-size rule (default_to_square = False): the short side becomes `edge`, the long side int(edge * long / short)
        const int shrt = std::min(H, W), lng = std::max(H, W), nl = (int)((double)((int64_t)edge * lng) / shrt);
        const int nh = H <= W ? edge : nl, nw = H <= W ? nl : edge;
        if (nh < C || nw < C) CS_FAIL(CS_E_UNSUPPORTED, "%s: resized image %d x %d is smaller than the %d crop (the processor would pad)", who, nh, nw, C);
        const Taps th = pil_taps(W, nw, crop_offset(nw, C, crop_rule), C, filter), tv = pil_taps(H, nh, crop_offset(nh, C, crop_rule), C, filter);
        Plan p{};
        const int rc = upload(who, H, W, th, tv, &p);
        if (rc != CS_OK) return rc;
        *out = &(plans[{H, W}] = p);
        return CS_OK;
    }
    // the plan of an H x W input resized straight to out_h x out_w on the integer-tap uint8 path: the two axes on independent scales, no crop window (what
    // Image.resize((out_w, out_h)) does; a side that has its size already gets the identity taps, which the fixed-point pass reproduces exactly)
    int get_plan_hw(const char* who, int H, int W, int out_h, int out_w, const Plan** out) {
        auto it = hw_plans.find({H, W, out_h, out_w});
        if (it != hw_plans.end()) { *out = &it->second; return CS_OK; }
        if (H < 1 || W < 1 || out_h < 1 || out_w < 1) CS_FAIL(CS_E_SHAPE, "%s: bad image size %d x %d -> %d x %d", who, H, W, out_h, out_w);
        const Taps th = pil_taps(W, out_w, 0, out_w, filter), tv = pil_taps(H, out_h, 0, out_h, filter);
        Plan p{};
        const int rc = upload(who, H, W, th, tv, &p);
        if (rc != CS_OK) return rc;
        *out = &(hw_plans[{H, W, out_h, out_w}] = p);
        return CS_OK;
    }
    // the two tap tables of an H x W input onto the device as one allocation (a full cache is emptied first), and the input rows / columns they read
    int upload(const char* who, int H, int W, const Taps& th, const Taps& tv, Plan* out) {
        Plan p{};
        int row0 = H, row1 = 0, col0 = W, col1 = 0;
        for (size_t i = 0; i < tv.lo.size(); ++i) { row0 = std::min(row0, tv.lo[i]); row1 = std::max(row1, tv.lo[i] + tv.cnt[i]); }
        for (size_t i = 0; i < th.lo.size(); ++i) { col0 = std::min(col0, th.lo[i]); col1 = std::max(col1, th.lo[i] + th.cnt[i]); }
        std::vector<int> all;
        auto put = [&](const std::vector<int>& v) { const size_t o = all.size(); all.insert(all.end(), v.begin(), v.end()); return o; };
        const size_t o0 = put(th.lo), o1 = put(th.cnt), o2 = put(th.kk), o3 = put(tv.lo), o4 = put(tv.cnt), o5 = put(tv.kk);
        const int rc = make_room();
        if (rc != CS_OK) return rc;
        int* d = nullptr;
        CS_CHECK_HIP(hipMalloc((void**)&d, all.size() * sizeof(int)));
        if (hipMemcpy(d, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); CS_FAIL(CS_E_HIP, "%s: resize table upload failed", who); }
        plan_allocs.push_back(d);
        p.dev = VitResizePlan{d + o0, d + o1, d + o2, th.ksize, d + o3, d + o4, d + o5, tv.ksize, row0, row1 - row0, col0, col1};
        *out = p;
        return CS_OK;
    }
    // the plan of an H x W mode-"F" image resized straight to out x out (clean-fid's resize): both axes independent, no crop window, double taps
    int get_float_plan(const char* who, int out_size, int H, int W, const FloatPlan** out) {
        auto it = float_plans.find({H, W});
        if (it != float_plans.end()) { *out = &it->second; return CS_OK; }
        if (H < 1 || W < 1 || out_size < 1) CS_FAIL(CS_E_SHAPE, "%s: bad image size %d x %d", who, H, W);
        const TapsF64 th = pil_float_side(W, out_size), tv = pil_float_side(H, out_size);
        // one allocation: the doubles first (8-byte aligned), then the ints
        const size_t nd = th.kk.size() + tv.kk.size(), ni = 4 * (size_t)out_size;
        std::vector<unsigned char> all(nd * sizeof(double) + ni * sizeof(int));
        double* hd = (double*)all.data();
        int* hi = (int*)(all.data() + nd * sizeof(double));
        std::copy(th.kk.begin(), th.kk.end(), hd); std::copy(tv.kk.begin(), tv.kk.end(), hd + th.kk.size());
        std::copy(th.lo.begin(), th.lo.end(), hi); std::copy(th.cnt.begin(), th.cnt.end(), hi + out_size);
        std::copy(tv.lo.begin(), tv.lo.end(), hi + 2 * out_size); std::copy(tv.cnt.begin(), tv.cnt.end(), hi + 3 * out_size);
        const int rc = make_room();
        if (rc != CS_OK) return rc;
        unsigned char* d = nullptr;
        CS_CHECK_HIP(hipMalloc((void**)&d, all.size()));
        if (hipMemcpy(d, all.data(), all.size(), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); CS_FAIL(CS_E_HIP, "%s: resize table upload failed", who); }
        plan_allocs.push_back(d);
        const double* dd = (const double*)d;
        const int* di = (const int*)(d + nd * sizeof(double));
        FloatPlan p{};
        p.dev = FidResizePlan{di, di + out_size, dd, th.ksize, di + 2 * out_size, di + 3 * out_size, dd + th.kk.size(), tv.ksize, out_size};
        *out = &(float_plans[{H, W}] = p);
        return CS_OK;
    }
    // the owner's destroy: nothing reads a table any more
    void free_device() {
        for (void* p : plan_allocs) (void)hipFree(p);
        plan_allocs.clear(); plans.clear(); float_plans.clear(); hw_plans.clear();
    }
};

}  // namespace image_front_end
