// AddressSanitizer / UBSan harness for the HOST side of the FID executor (fid.cpp with incep_walk.h / weights.h / image_tower.h / image_front_end.h).
// Built by tests/test_sanitize_fid.py with -fsanitize=address,undefined -fno-gpu-sanitize from the real sources, linked against stubs.cpp, incep_stubs.cpp and
// fid_stubs.cpp (host malloc for device memory; launch stubs that touch the first and last byte of every tensor), run as a stand-alone program:
//   create -> set_weight (fc.* and AuxLogits.* ignored) -> finalize -> preprocess at the sizes of the GPU tests and at one-pixel sides, with more sizes than the
//   plan cache holds -> workspace_bytes -> forward on a workspace of EXACTLY the requested size; the statistics entry points and their refusals; the error
//   paths; a finalize with one weight missing; destroy.
#include "../../include/consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s  (last error: %s)\n", __FILE__, __LINE__, #cond, cs_last_error()); ++g_fail; } } while (0)

static CsFidConfig fid_config() {
    CsFidConfig c{};
    for (int i = 0; i < 3; ++i) { c.image_mean[i] = 128.f; c.image_std[i] = 128.f; }
    return c;
}

// every tensor of the manifest (skip: one index left out), then finalize
static int load_weights(CsFid* h, int skip) {
    std::vector<float> buf;
    const int n = cs_fid_num_weights(h);
    for (int i = 0; i < n; ++i) {
        int64_t sh[4]; int nd = -1;
        const char* name = cs_fid_weight_name(h, i, sh, &nd);
        EXPECT(name && nd >= 0 && nd <= 4);
        if (i == skip) continue;
        size_t cnt = 1;
        for (int k = 0; k < nd; ++k) cnt *= (size_t)sh[k];
        buf.assign(cnt, std::string(name).find("running_var") != std::string::npos ? 1.0f : 0.01f);
        EXPECT(cs_fid_set_weight(h, name, buf.data(), nd ? sh : nullptr, nd) == CS_OK);
        if (i == 0) {
            int64_t bad[4] = {sh[0] + 1, sh[1], sh[2], sh[3]};
            EXPECT(cs_fid_set_weight(h, name, buf.data(), bad, nd) == CS_E_SHAPE && cs_fid_set_weight(h, "no.such.tensor", buf.data(), sh, nd) == CS_E_ARG);
            int64_t fc[2] = {1008, 2048};
            EXPECT(cs_fid_set_weight(h, "fc.weight", buf.data(), fc, 2) == CS_OK && cs_fid_set_weight(h, "fc.bias", buf.data(), fc, 1) == CS_OK);   // accepted, ignored
            EXPECT(cs_fid_set_weight(h, "AuxLogits.fc.bias", buf.data(), sh, 1) == CS_OK);
        }
    }
    return cs_fid_finalize(h);
}

static void preprocess(CsFid* h, int B, int H, int W, int dtype, bool want_f32) {
    const size_t esz = dtype == CS_U8 ? 1 : (dtype == CS_F16 ? 2 : 4);
    const size_t pwb = cs_fid_preprocess_workspace_bytes(h, B, H, W);
    void* pws = malloc(pwb);
    std::vector<unsigned char> img((size_t)B * 3 * H * W * esz, 0);
    std::vector<unsigned short> patches((size_t)B * 299 * 299 * 8);
    std::vector<float> f32(want_f32 ? (size_t)B * 3 * 299 * 299 : 0);
    EXPECT(pwb > 0 && cs_fid_preprocess(h, img.data(), dtype, B, H, W, patches.data(), want_f32 ? f32.data() : nullptr, pws, pwb, nullptr) == CS_OK);
    EXPECT(cs_fid_preprocess(h, img.data(), dtype, B, H, W, patches.data(), nullptr, pws, 16, nullptr) != CS_OK);
    free(pws);
}

int main() {
    CsFid* h = nullptr;
    CsFidConfig bad = fid_config();
    EXPECT(cs_fid_create(nullptr, &h) != CS_OK && cs_fid_create(&bad, nullptr) != CS_OK);
    bad.image_std[1] = 0.f; EXPECT(cs_fid_create(&bad, &h) == CS_E_ARG);
    const CsFidConfig c = fid_config();
    EXPECT(cs_fid_create(&c, &h) == CS_OK && h);
    EXPECT(cs_fid_patch_cols(h) == 8 && cs_fid_num_tokens(h) == 64 && cs_fid_num_weights(h) == 564);
    const int B = 2;
    const size_t wsb = cs_fid_workspace_bytes(h, B);
    EXPECT(wsb > 0 && cs_fid_workspace_bytes(h, 0) == 0 && cs_fid_workspace_bytes(nullptr, B) == 0);
    void* ws = malloc(wsb);                                          // exactly the requested size: one byte past the end is an ASan error
    std::vector<unsigned short> patches((size_t)B * 299 * 299 * 8);
    std::vector<float> feats((size_t)B * 2048);
    EXPECT(cs_fid_forward(h, patches.data(), B, feats.data(), ws, wsb, nullptr) == CS_E_STATE);              // not finalized
    EXPECT(load_weights(h, -1) == CS_OK && cs_fid_finalize(h) == CS_OK);
    EXPECT(cs_fid_flops(h, B) > 0 && cs_fid_workspace_bytes(h, B) == wsb);
    // the front end: the test sizes, one-pixel sides, every dtype; 20 more sizes overflow the plan cache (16) and empty it
    preprocess(h, B, 37, 53, CS_U8, true);
    preprocess(h, B, 300, 299, CS_F32, false);
    preprocess(h, B, 299, 299, CS_F16, true);
    preprocess(h, B, 96, 640, CS_U8, false);
    preprocess(h, 1, 1, 1, CS_F32, true);
    preprocess(h, 1, 5, 1, CS_U8, false);
    preprocess(h, 1, 1, 700, CS_U8, false);
    for (int k = 0; k < 20; ++k) preprocess(h, 1, 40 + 7 * k, 300 - 11 * k, CS_U8, false);
    preprocess(h, B, 37, 53, CS_U8, true);                                                                      // rebuilt after the cache was emptied
    {
        std::vector<float> img(3 * 8 * 8, 0.5f);
        char pws[64];
        EXPECT(cs_fid_preprocess(nullptr, img.data(), CS_F32, 1, 8, 8, patches.data(), nullptr, pws, sizeof pws, nullptr) == CS_E_ARG);
        EXPECT(cs_fid_preprocess(h, nullptr, CS_F32, 1, 8, 8, patches.data(), nullptr, pws, sizeof pws, nullptr) == CS_E_ARG);
        EXPECT(cs_fid_preprocess(h, img.data(), CS_BF16, 1, 8, 8, patches.data(), nullptr, pws, sizeof pws, nullptr) == CS_E_DTYPE);
        EXPECT(cs_fid_preprocess(h, img.data(), CS_F32, 1, 0, 8, patches.data(), nullptr, pws, sizeof pws, nullptr) == CS_E_SHAPE);
        EXPECT(cs_fid_preprocess(h, img.data(), CS_F32, -1, 8, 8, patches.data(), nullptr, pws, sizeof pws, nullptr) == CS_E_ARG);
        EXPECT(cs_fid_preprocess(h, nullptr, CS_F32, 0, 8, 8, nullptr, nullptr, nullptr, 0, nullptr) == CS_OK);                  // empty batch: no-op
        EXPECT(cs_fid_preprocess_workspace_bytes(h, 0, 8, 8) == 0 && cs_fid_preprocess_workspace_bytes(nullptr, 1, 8, 8) == 0);
    }
    EXPECT(cs_fid_forward(h, patches.data(), B, feats.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_fid_forward(h, patches.data(), B, feats.data(), ws, wsb - 1, nullptr) != CS_OK);
    EXPECT(cs_fid_forward(h, nullptr, B, feats.data(), ws, wsb, nullptr) != CS_OK && cs_fid_forward(h, patches.data(), B, feats.data(), nullptr, wsb, nullptr) != CS_OK);
    EXPECT(cs_fid_forward(h, patches.data(), B, nullptr, ws, wsb, nullptr) != CS_OK);
    EXPECT(cs_fid_forward(nullptr, patches.data(), B, feats.data(), ws, wsb, nullptr) == CS_E_ARG && cs_fid_forward(h, patches.data(), -1, feats.data(), ws, wsb, nullptr) == CS_E_ARG);
    EXPECT(cs_fid_forward(h, patches.data(), 0, feats.data(), ws, wsb, nullptr) == CS_OK);
    free(ws);
    cs_fid_destroy(h);
    {                                                                                                // the statistics: exact-size buffers, the refusals
        const int d = 48; const int64_t n = 5;
        std::vector<float> f((size_t)n * d, 1.f);
        std::vector<double> sum(d), outer((size_t)d * d), mu(d), sigma((size_t)d * d);
        EXPECT(cs_fid_stats_accumulate(f.data(), n, d, sum.data(), outer.data(), nullptr) == CS_OK);
        EXPECT(cs_fid_stats_finalize(sum.data(), outer.data(), n, d, mu.data(), sigma.data(), nullptr) == CS_OK);
        EXPECT(cs_fid_stats_accumulate(f.data(), n, 24, sum.data(), outer.data(), nullptr) == CS_E_SHAPE);
        EXPECT(cs_fid_stats_accumulate(f.data(), n, 0, sum.data(), outer.data(), nullptr) == CS_E_SHAPE && cs_fid_stats_accumulate(f.data(), n, 4112, sum.data(), outer.data(), nullptr) == CS_E_SHAPE);
        EXPECT(cs_fid_stats_accumulate(f.data(), 0, d, sum.data(), outer.data(), nullptr) == CS_E_SHAPE && cs_fid_stats_accumulate(f.data(), -3, d, sum.data(), outer.data(), nullptr) == CS_E_SHAPE);
        EXPECT(cs_fid_stats_accumulate(nullptr, n, d, sum.data(), outer.data(), nullptr) == CS_E_ARG && cs_fid_stats_accumulate(f.data(), n, d, nullptr, outer.data(), nullptr) == CS_E_ARG);
        EXPECT(cs_fid_stats_finalize(sum.data(), outer.data(), 1, d, mu.data(), sigma.data(), nullptr) == CS_E_SHAPE);
        EXPECT(cs_fid_stats_finalize(sum.data(), outer.data(), n, 24, mu.data(), sigma.data(), nullptr) == CS_E_SHAPE);
        EXPECT(cs_fid_stats_finalize(sum.data(), outer.data(), n, d, nullptr, sigma.data(), nullptr) == CS_E_ARG);
    }
    {                                                                                                // the op entry points reach their launchers
        std::vector<unsigned short> x(2 * 3 * 3 * 8), y(2 * 3 * 3 * 8);
        EXPECT(cs_op_fid_avgpool(x.data(), 2, 3, 3, 8, y.data(), nullptr) == CS_OK && cs_op_fid_maxpool(x.data(), 2, 3, 3, 8, y.data(), nullptr) == CS_OK);
    }
    {                                                                                                // finalize with a weight missing names it
        EXPECT(cs_fid_create(&c, &h) == CS_OK);
        EXPECT(load_weights(h, cs_fid_num_weights(h) / 2) == CS_E_STATE && strstr(cs_last_error(), "missing weight"));
        cs_fid_destroy(h);
    }
    cs_fid_destroy(nullptr);
    if (g_fail) { fprintf(stderr, "fid sanitize harness: %d failures\n", g_fail); return 1; }
    printf("fid sanitize harness: ok\n");
    return 0;
}
