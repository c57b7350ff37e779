// The resize plans of the image front end (launch_vit_front_end), used through image_tower.h by the executors whose processor is "PIL bicubic resize to a
// shortest edge, center crop, rescale, normalise" (vit.cpp: DINOv2; clip_vision.cpp: CLIP; depth.cpp: Depth Anything, edge = crop = size).  Host only: PIL's tap tables for the crop window of one (height, width),
// built in double as ImagingResample does, uploaded once per size and kept in a bounded cache that the handle owns.
#pragma once
#include "ops.h"

#include <algorithm>
#include <cmath>
#include <map>
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
inline Taps pil_taps(int in, int out, int win0, int win, Filter filter = PIL_BICUBIC) {
    Taps t;
    const double scale = (double)in / out, fs = std::max(scale, 1.0), support = (filter == PIL_BILINEAR ? 1.0 : 2.0) * fs, ww = 1.0 / fs;
    t.ksize = (int)std::ceil(support) * 2 + 1;
    t.lo.resize(win); t.cnt.resize(win); t.kk.assign((size_t)win * t.ksize, 0);
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
        for (int x = 0; x < n; ++x) {
            const double k = tot != 0.0 ? w[x] / tot : w[x];
            t.kk[(size_t)i * t.ksize + x] = k < 0 ? (int)(-0.5 + k * (1 << 22)) : (int)(0.5 + k * (1 << 22));
        }
        t.lo[i] = xmin; t.cnt[i] = n;
    }
    return t;
}

struct Plan { VitResizePlan dev; };

// resize tables per input (height, width), at most MAX_PLANS of them (a directory of many image sizes must not grow device memory without bound: when the
// cache is full it is emptied -- hipFree waits for the kernels that still read a table).  Like every handle here the owner serves one thread at a time, and the
// tables live on the device that is current when a size is first seen: callers run a handle on one device (the Python wrapper selects the tensor's).
struct PlanCache {
    static constexpr size_t MAX_PLANS = 16;
    Filter filter = PIL_BICUBIC;                            // the processor's resample (set once, before the first plan)
    CropRule crop_rule = CROP_FLOOR;                        // the processor's center-crop offset (set once, next to filter)
    std::map<std::pair<int, int>, Plan> plans;
    std::vector<void*> plan_allocs;

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
        int row0 = H, row1 = 0, col0 = W, col1 = 0;
        for (int i = 0; i < C; ++i) {
            row0 = std::min(row0, tv.lo[i]); row1 = std::max(row1, tv.lo[i] + tv.cnt[i]);
            col0 = std::min(col0, th.lo[i]); col1 = std::max(col1, th.lo[i] + th.cnt[i]);
        }
        std::vector<int> all;
        auto put = [&](const std::vector<int>& v) { const size_t o = all.size(); all.insert(all.end(), v.begin(), v.end()); return o; };
        const size_t o0 = put(th.lo), o1 = put(th.cnt), o2 = put(th.kk), o3 = put(tv.lo), o4 = put(tv.cnt), o5 = put(tv.kk);
        if (plans.size() >= MAX_PLANS) {
            for (void* q : plan_allocs) CS_CHECK_HIP(hipFree(q));
            plan_allocs.clear(); plans.clear();
        }
        int* d = nullptr;
        CS_CHECK_HIP(hipMalloc((void**)&d, all.size() * sizeof(int)));
        if (hipMemcpy(d, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); CS_FAIL(CS_E_HIP, "%s: resize table upload failed", who); }
        plan_allocs.push_back(d);
        p.dev = VitResizePlan{d + o0, d + o1, d + o2, th.ksize, d + o3, d + o4, d + o5, tv.ksize, row0, row1 - row0, col0, col1};
        *out = &(plans[{H, W}] = p);
        return CS_OK;
    }
    // the owner's destroy: nothing reads a table any more
    void free_device() {
        for (void* p : plan_allocs) (void)hipFree(p);
        plan_allocs.clear(); plans.clear();
    }
};

}  // namespace image_front_end
