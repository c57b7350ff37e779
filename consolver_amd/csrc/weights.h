// Weight plumbing shared by the model handles (host only): the manifest of expected tensors with the validation every cs_X_set_weight runs, the host
// staging store with its uploads (UNet / VAE / CLIP: fp16, rounded once when a tensor is set; ViT: fp32, rounded once at upload, after its LayerScale
// fold), and the conv / norm packing the UNet and the VAE share.  CsFlux stages its tensors on the device and takes the manifest part only.
#pragma once
#include "ops.h"

#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

// ordered names and expected shapes of a handle's state dict
struct WeightManifest {
    std::vector<std::string> names;
    std::map<std::string, std::vector<int64_t>> shapes;
    bool finalized = false;

    void expect(const std::string& n, std::vector<int64_t> shape) { names.push_back(n); shapes[n] = std::move(shape); }
    int count() const { return (int)names.size(); }
    // cs_X_weight_name: shape_out has room for cap dims, the ones past the rank are 1
    const char* name_at(int i, int64_t* shape_out, int cap, int* ndim) const {
        if (i < 0 || i >= count()) return nullptr;
        const auto& sh = shapes.at(names[i]);
        if (ndim) *ndim = (int)sh.size();
        if (shape_out) for (size_t k = 0; k < (size_t)cap; ++k) shape_out[k] = k < sh.size() ? sh[k] : 1;
        return names[i].c_str();
    }
    // the validation half of cs_X_set_weight; elems = the tensor's element count
    int check(const char* name, const void* data, const int64_t* shape, int ndim, size_t* elems) const {
        if (!name || !data || !shape) CS_FAIL(CS_E_ARG, "null argument");
        if (finalized) CS_FAIL(CS_E_STATE, "weights are already packed");
        auto it = shapes.find(name);
        if (it == shapes.end()) CS_FAIL(CS_E_ARG, "unexpected tensor name '%s'", name);
        if ((int)it->second.size() != ndim) CS_FAIL(CS_E_SHAPE, "%s: rank %d, expected %zu", name, ndim, it->second.size());
        size_t n = 1;
        for (int k = 0; k < ndim; ++k) {
            if (shape[k] != it->second[k]) CS_FAIL(CS_E_SHAPE, "%s: dim %d is %lld, expected %lld", name, k, (long long)shape[k], (long long)it->second[k]);
            n *= (size_t)shape[k];
        }
        *elems = n;
        return CS_OK;
    }
    // cs_X_finalize: the first expected tensor `have` (a map keyed by name) lacks, or null
    template <typename Map> const std::string* first_missing(const Map& have) const {
        for (auto& n : names) if (!have.count(n)) return &n;
        return nullptr;
    }
};

// device memory of at least 256 bytes, recorded in `owned` (freed with the handle); null when the allocation fails
inline void* device_alloc(size_t bytes, std::vector<void*>& owned) {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(bytes, 256)) != hipSuccess) return nullptr;
    owned.push_back(d);
    return d;
}

template <typename E> struct HostTensor { std::vector<int64_t> shape; std::vector<E> data; };

// manifest + host staging in element type E + the device allocations the packed weights live in
template <typename E> struct WeightStore : WeightManifest {
    std::map<std::string, HostTensor<E>> host;
    std::vector<void*> dev_allocs;

    int set(const char* name, const float* data, const int64_t* shape, int ndim) {
        size_t n = 0;
        const int rc = check(name, data, shape, ndim, &n);
        if (rc != CS_OK) return rc;
        HostTensor<E> t; t.shape.assign(shape, shape + ndim); t.data.resize(n);
        for (size_t i = 0; i < n; ++i) t.data[i] = (E)data[i];
        host[name] = std::move(t);
        return CS_OK;
    }
    const std::string* first_missing() const { return WeightManifest::first_missing(host); }
    const HostTensor<E>& at(const std::string& n) const { return host.at(n); }

    void* upload_bytes(const void* src, size_t bytes) {
        void* d = device_alloc(bytes, dev_allocs);
        if (d && hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
    // device fp16 copy of host elements (fp32 staging is rounded here, once); null when the allocation or the copy fails
    f16* upload(const std::vector<E>& h) {
        if constexpr (std::is_same<E, f16>::value) return (f16*)upload_bytes(h.data(), h.size() * sizeof(f16));
        else { const std::vector<f16> t(h.begin(), h.end()); return (f16*)upload_bytes(t.data(), t.size() * sizeof(f16)); }
    }
    float* upload_f32(const std::vector<float>& v) { return (float*)upload_bytes(v.data(), v.size() * sizeof(float)); }      // (the LN-fold vectors)
    void release_host() { host.clear(); }
    void free_device() { for (void* p : dev_allocs) (void)hipFree(p); dev_allocs.clear(); }
};

// ---- conv / norm packing of the UNet and the VAE (fp16 staging) ----------------------------------------------------------
typedef WeightStore<f16> F16Store;

struct Conv { f16* w = nullptr; f16* b = nullptr; int cin = 0, cout = 0, taps = 1; f16* w_sub = nullptr; };     // w_sub: an upsampler's sub-pixel filters (IgemmArgs::w_up_sub)
struct Norm { f16* g = nullptr; f16* b = nullptr; int c = 0; float eps = 1e-5f; };

// [Cout][Cin][kh][kw] -> [Cout][kh*kw][Cin]
inline std::vector<f16> pack_conv(const HostTensor<f16>& t) {
    const int64_t co = t.shape[0], ci = t.shape[1], kk = t.shape.size() == 4 ? t.shape[2] * t.shape[3] : 1;
    std::vector<f16> o((size_t)co * ci * kk);
    for (int64_t n = 0; n < co; ++n)
        for (int64_t c = 0; c < ci; ++c)
            for (int64_t k = 0; k < kk; ++k) o[(n * kk + k) * ci + c] = t.data[(n * ci + c) * kk + k];
    return o;
}
inline bool make_conv(F16Store& W, const std::string& p, Conv& c) {
    const HostTensor<f16>& w = W.at(p + ".weight");
    c.cout = (int)w.shape[0]; c.cin = (int)w.shape[1]; c.taps = w.shape.size() == 4 ? (int)(w.shape[2] * w.shape[3]) : 1;
    c.w = W.upload(pack_conv(w)); c.b = W.upload(W.at(p + ".bias").data);
    return c.w && c.b;
}
// 3x3 conv whose few input channels are zero-padded to 64 (the operand then arrives as NHWC-64): [co][ci][3][3] -> [co][9][64]
inline bool make_conv_padded64(F16Store& W, const std::string& p, Conv& c) {
    const HostTensor<f16>& w = W.at(p + ".weight");
    const int64_t co = w.shape[0], ci = w.shape[1];
    std::vector<f16> o((size_t)co * 9 * 64, (f16)0.f);
    for (int64_t n = 0; n < co; ++n) for (int64_t ch = 0; ch < ci; ++ch) for (int64_t k = 0; k < 9; ++k) o[(n * 9 + k) * 64 + ch] = w.data[(n * ci + ch) * 9 + k];
    c.cout = (int)co; c.cin = 64; c.taps = 9;
    c.w = W.upload(o); c.b = W.upload(W.at(p + ".bias").data);
    return c.w && c.b;
}
inline bool make_norm(F16Store& W, const std::string& p, Norm& n, float eps) {
    n.c = (int)W.at(p + ".weight").shape[0]; n.eps = eps;
    n.g = W.upload(W.at(p + ".weight").data); n.b = W.upload(W.at(p + ".bias").data);
    return n.g && n.b;
}
