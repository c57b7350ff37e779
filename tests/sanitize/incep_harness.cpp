// AddressSanitizer / UBSan harness for the HOST side of the Inception-v3 executor (inception.cpp with weights.h / image_tower.h / image_front_end.h).
// Built by tests/test_sanitize_inception.py with -fsanitize=address,undefined -fno-gpu-sanitize from the real sources, linked against stubs.cpp and
// incep_stubs.cpp (host malloc for device memory; launch stubs that touch the first and last byte of every tensor), run as a stand-alone program:
//   create -> set_weight -> finalize -> preprocess -> workspace_bytes -> forward on a workspace of EXACTLY the requested size, at the smallest legal image
//   (75: last grid 1 x 1), at the fixture's 107 with a non-square input on the round-half-even crop offset, and at 299; the error paths; a finalize with one
//   weight missing; destroy.
#include "../../include/consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s  (last error: %s)\n", __FILE__, __LINE__, #cond, cs_last_error()); ++g_fail; } } while (0)

static CsIncepConfig incep_config(int size) {
    CsIncepConfig c{};
    c.image_size = size; c.num_classes = 1000; c.rescale_factor = 1.0 / 255;
    for (int i = 0; i < 3; ++i) { c.image_mean[i] = 0.5f; c.image_std[i] = 0.25f; }
    return c;
}

// every tensor of the manifest (skip: one index left out), then finalize
static int load_weights(CsIncep* h, int skip) {
    std::vector<float> buf;
    const int n = cs_incep_num_weights(h);
    for (int i = 0; i < n; ++i) {
        int64_t sh[4]; int nd = -1;
        const char* name = cs_incep_weight_name(h, i, sh, &nd);
        EXPECT(name && nd >= 0 && nd <= 4);
        if (i == skip) continue;
        size_t cnt = 1;
        for (int k = 0; k < nd; ++k) cnt *= (size_t)sh[k];
        buf.assign(cnt, std::string(name).find("running_var") != std::string::npos ? 1.0f : 0.01f);
        EXPECT(cs_incep_set_weight(h, name, buf.data(), nd ? sh : nullptr, nd) == CS_OK);
        if (i == 0) {
            int64_t bad[4] = {sh[0] + 1, sh[1], sh[2], sh[3]};
            EXPECT(cs_incep_set_weight(h, name, buf.data(), bad, nd) == CS_E_SHAPE && cs_incep_set_weight(h, "no.such.tensor", buf.data(), sh, nd) == CS_E_ARG);
            EXPECT(cs_incep_set_weight(h, "AuxLogits.fc.bias", buf.data(), sh, 1) == CS_OK);                 // accepted, ignored
        }
    }
    return cs_incep_finalize(h);
}

static void run(int size, int B, int H, int W, int last) {
    const CsIncepConfig c = incep_config(size);
    CsIncep* h = nullptr;
    EXPECT(cs_incep_create(&c, &h) == CS_OK && h);
    EXPECT(cs_incep_patch_cols(h) == 8 && cs_incep_num_tokens(h) == last * last && cs_incep_num_weights(h) == 566);
    const size_t wsb = cs_incep_workspace_bytes(h, B);
    EXPECT(wsb > 0 && cs_incep_workspace_bytes(h, 0) == 0 && cs_incep_workspace_bytes(nullptr, B) == 0);
    void* ws = malloc(wsb);                                          // exactly the requested size: one byte past the end is an ASan error
    std::vector<unsigned short> patches((size_t)B * size * size * 8);
    std::vector<float> logits((size_t)B * 1000);
    EXPECT(cs_incep_forward(h, patches.data(), B, logits.data(), ws, wsb, nullptr) == CS_E_STATE);          // not finalized
    EXPECT(load_weights(h, -1) == CS_OK && cs_incep_finalize(h) == CS_OK);
    EXPECT(cs_incep_flops(h, B) > 0 && cs_incep_workspace_bytes(h, B) == wsb);
    {
        const size_t pwb = cs_incep_preprocess_workspace_bytes(h, B, H, W);
        void* pws = malloc(pwb);
        std::vector<float> img((size_t)B * 3 * H * W, 0.5f);
        std::vector<unsigned char> u8((size_t)B * 3 * size * size);
        EXPECT(pwb > 0 && cs_incep_preprocess(h, img.data(), CS_F32, B, H, W, patches.data(), u8.data(), pws, pwb, nullptr) == CS_OK);
        {                                                                                                                       // the transposed shape, its own workspace
            const size_t tb = cs_incep_preprocess_workspace_bytes(h, B, W, H);
            void* tws = malloc(tb);
            EXPECT(tb > 0 && cs_incep_preprocess(h, img.data(), CS_F32, B, W, H, patches.data(), nullptr, tws, tb, nullptr) == CS_OK);
            free(tws);
        }
        EXPECT(cs_incep_preprocess(h, img.data(), CS_F32, B, H, W, patches.data(), nullptr, pws, 16, nullptr) != CS_OK);
        EXPECT(cs_incep_preprocess(h, nullptr, CS_F32, B, H, W, patches.data(), nullptr, pws, pwb, nullptr) == CS_E_ARG);
        EXPECT(cs_incep_preprocess(h, img.data(), CS_F32, B, 0, W, patches.data(), nullptr, pws, pwb, nullptr) != CS_OK);
        EXPECT(cs_incep_preprocess(h, nullptr, CS_F32, 0, H, W, nullptr, nullptr, nullptr, 0, nullptr) == CS_OK);              // empty batch: no-op
        free(pws);
    }
    EXPECT(cs_incep_forward(h, patches.data(), B, logits.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_incep_forward(h, patches.data(), B, logits.data(), ws, wsb - 1, nullptr) != CS_OK);
    EXPECT(cs_incep_forward(h, nullptr, B, logits.data(), ws, wsb, nullptr) != CS_OK && cs_incep_forward(h, patches.data(), B, logits.data(), nullptr, wsb, nullptr) != CS_OK);
    EXPECT(cs_incep_forward(h, patches.data(), B, nullptr, ws, wsb, nullptr) != CS_OK);
    EXPECT(cs_incep_forward(nullptr, patches.data(), B, logits.data(), ws, wsb, nullptr) == CS_E_ARG && cs_incep_forward(h, patches.data(), -1, logits.data(), ws, wsb, nullptr) == CS_E_ARG);
    EXPECT(cs_incep_forward(h, patches.data(), 0, logits.data(), ws, wsb, nullptr) == CS_OK);
    for (int parts = 1; parts <= 4; ++parts)
        EXPECT(cs_incep_set_stage_limit(h, parts) == CS_OK && cs_incep_forward(h, patches.data(), B, logits.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_incep_set_stage_limit(h, 0) == CS_E_ARG && cs_incep_set_stage_limit(h, 6) == CS_E_ARG && cs_incep_set_stage_limit(h, 5) == CS_OK);
    free(ws);
    cs_incep_destroy(h);
}

int main() {
    CsIncep* h = nullptr;
    CsIncepConfig bad = incep_config(299);
    EXPECT(cs_incep_create(nullptr, &h) != CS_OK);
    bad.image_size = 74; EXPECT(cs_incep_create(&bad, &h) == CS_E_SHAPE);                              // the last grid would be empty
    bad = incep_config(299); bad.num_classes = 0; EXPECT(cs_incep_create(&bad, &h) == CS_E_ARG);
    bad = incep_config(299); bad.image_std[1] = 0.f; EXPECT(cs_incep_create(&bad, &h) == CS_E_ARG);
    run(75, 2, 75, 75, 1);
    run(107, 1, 131, 96, 2);                                                                          // resizes to 146 x 107: crop offset 20 (round half even)
    run(299, 1, 320, 512, 8);
    EXPECT(cs_incep_set_stage_limit(nullptr, 1) == CS_E_ARG);
    {                                                                                                // finalize with a weight missing names it
        const CsIncepConfig c = incep_config(75);
        EXPECT(cs_incep_create(&c, &h) == CS_OK);
        EXPECT(load_weights(h, cs_incep_num_weights(h) / 2) == CS_E_STATE && strstr(cs_last_error(), "missing weight"));
        cs_incep_destroy(h);
    }
    cs_incep_destroy(nullptr);
    if (g_fail) { fprintf(stderr, "incep sanitize harness: %d failures\n", g_fail); return 1; }
    printf("incep sanitize harness: ok\n");
    return 0;
}
