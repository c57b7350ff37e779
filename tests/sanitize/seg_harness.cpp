// AddressSanitizer / UBSan harness for the HOST side of the SegFormer executor (segformer.cpp with weights.h / encoder.h / image_tower.h / image_front_end.h).
// Built by tests/test_sanitize_segformer.py with -fsanitize=address,undefined -fno-gpu-sanitize from the real sources, linked against stubs.cpp and
// seg_stubs.cpp (host malloc for device memory; launch stubs that touch the first and last byte of every tensor), run as a stand-alone program:
//   create -> set_weight -> finalize -> preprocess -> workspace_bytes -> forward + masks on a workspace of EXACTLY the requested size, at the smallest legal
//   shape (size 32: grids 8 / 4 / 2 / 1, sr ratios 8 / 4 / 2 / 1, one key per stage) and at the fixture's ragged one (size 160: 25 keys); the error paths;
//   a finalize with one weight missing; destroy.
#include "../../include/consolver_hip.h"
#include "../../include/consolver_hip_ops.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s  (last error: %s)\n", __FILE__, __LINE__, #cond, cs_last_error()); ++g_fail; } } while (0)

static CsSegConfig seg_config(int size) {
    CsSegConfig c{};
    const int hs[4] = {64, 128, 320, 512}, heads[4] = {1, 2, 5, 8}, sr[4] = {8, 4, 2, 1}, depths[4] = {1, 1, 2, 1};
    for (int i = 0; i < 4; ++i) { c.hidden_sizes[i] = hs[i]; c.num_attention_heads[i] = heads[i]; c.sr_ratios[i] = sr[i]; c.depths[i] = depths[i]; }
    c.mlp_ratio = 4; c.decoder_hidden_size = 128; c.num_labels = 150; c.size = size; c.rescale_factor = 1.0 / 255;
    for (int i = 0; i < 3; ++i) { c.image_mean[i] = 0.5f; c.image_std[i] = 0.25f; }
    return c;
}

// every tensor of the manifest (skip: one index left out), then finalize
static int load_weights(CsSeg* h, int skip) {
    std::vector<float> buf;
    const int n = cs_seg_num_weights(h);
    for (int i = 0; i < n; ++i) {
        int64_t sh[4]; int nd = -1;
        const char* name = cs_seg_weight_name(h, i, sh, &nd);
        EXPECT(name && nd >= 0 && nd <= 4);
        if (i == skip) continue;
        size_t cnt = 1;
        for (int k = 0; k < nd; ++k) cnt *= (size_t)sh[k];
        buf.assign(cnt, std::string(name).find("running_var") != std::string::npos ? 1.0f : 0.01f);
        EXPECT(cs_seg_set_weight(h, name, buf.data(), nd ? sh : nullptr, nd) == CS_OK);
        if (i == 0) {
            int64_t bad[4] = {sh[0] + 1, sh[1], sh[2], sh[3]};
            EXPECT(cs_seg_set_weight(h, name, buf.data(), bad, nd) == CS_E_SHAPE && cs_seg_set_weight(h, "no.such.tensor", buf.data(), sh, nd) == CS_E_ARG);
        }
    }
    return cs_seg_finalize(h);
}

static void run(int size, int B) {
    const CsSegConfig c = seg_config(size);
    CsSeg* h = nullptr;
    EXPECT(cs_seg_create(&c, &h) == CS_OK && h);
    const int g = size / 4;
    EXPECT(cs_seg_patch_cols(h) == 8 && cs_seg_num_tokens(h) == g * g);
    const size_t wsb = cs_seg_workspace_bytes(h, B);
    EXPECT(wsb > 0 && cs_seg_workspace_bytes(h, 0) == 0 && cs_seg_workspace_bytes(nullptr, B) == 0);
    void* ws = malloc(wsb);                                          // exactly the requested size: one byte past the end is an ASan error
    std::vector<unsigned short> patches((size_t)B * size * size * 8);
    std::vector<float> logits((size_t)B * 150 * g * g);
    std::vector<int> masks((size_t)B * g * g);
    EXPECT(cs_seg_forward(h, patches.data(), B, logits.data(), ws, wsb, nullptr) == CS_E_STATE);          // not finalized
    EXPECT(load_weights(h, -1) == CS_OK && cs_seg_finalize(h) == CS_OK);
    EXPECT(cs_seg_flops(h, B) > 0 && cs_seg_workspace_bytes(h, B) == wsb);
    {
        const int H = size == 32 ? 48 : size;                        // a downscale / the processor's own size
        const size_t pwb = cs_seg_preprocess_workspace_bytes(h, B, H, H);
        void* pws = malloc(pwb);
        std::vector<float> img((size_t)B * 3 * H * H, 0.5f);
        std::vector<unsigned char> u8((size_t)B * 3 * size * size);
        EXPECT(pwb > 0 && cs_seg_preprocess(h, img.data(), CS_F32, B, H, H, patches.data(), u8.data(), pws, pwb, nullptr) == CS_OK);
        EXPECT(cs_seg_preprocess(h, img.data(), CS_F32, B, H, H, patches.data(), nullptr, pws, 16, nullptr) != CS_OK);
        EXPECT(cs_seg_preprocess(h, img.data(), CS_F32, B, H, H - 8, patches.data(), nullptr, pws, pwb, nullptr) == CS_E_UNSUPPORTED);     // not square
        EXPECT(cs_seg_preprocess(h, nullptr, CS_F32, B, H, H, patches.data(), nullptr, pws, pwb, nullptr) == CS_E_ARG);
        EXPECT(cs_seg_preprocess(h, nullptr, CS_F32, 0, H, H, nullptr, nullptr, nullptr, 0, nullptr) == CS_OK);                          // empty batch: no-op
        free(pws);
    }
    EXPECT(cs_seg_forward(h, patches.data(), B, logits.data(), ws, wsb, nullptr) == CS_OK);
    EXPECT(cs_seg_masks(h, B, ws, wsb, masks.data(), nullptr) == CS_OK);
    EXPECT(cs_seg_forward(h, patches.data(), B, nullptr, ws, wsb, nullptr) == CS_OK);                      // masks only: no fp32 logits
    EXPECT(cs_seg_forward(h, patches.data(), B, logits.data(), ws, wsb - 1, nullptr) != CS_OK && cs_seg_masks(h, B, ws, wsb - 1, masks.data(), nullptr) != CS_OK);
    EXPECT(cs_seg_forward(h, nullptr, B, logits.data(), ws, wsb, nullptr) != CS_OK && cs_seg_forward(h, patches.data(), B, logits.data(), nullptr, wsb, nullptr) != CS_OK);
    EXPECT(cs_seg_forward(nullptr, patches.data(), B, logits.data(), ws, wsb, nullptr) == CS_E_ARG && cs_seg_forward(h, patches.data(), -1, logits.data(), ws, wsb, nullptr) == CS_E_ARG);
    EXPECT(cs_seg_forward(h, patches.data(), 0, logits.data(), ws, wsb, nullptr) == CS_OK && cs_seg_masks(h, 0, ws, wsb, masks.data(), nullptr) == CS_OK);
    EXPECT(cs_seg_masks(h, B, ws, wsb, nullptr, nullptr) != CS_OK);
    EXPECT(cs_seg_set_stage_limit(h, 0) == CS_E_ARG && cs_seg_set_stage_limit(h, 2) == CS_OK && cs_seg_forward(h, patches.data(), B, nullptr, ws, wsb, nullptr) == CS_OK &&
           cs_seg_set_stage_limit(h, 5) == CS_OK);
    std::vector<float> out(B);
    EXPECT(cs_seg_agreement(masks.data(), masks.data(), (int64_t)g * g, B, (int64_t)g * g, out.data(), nullptr) == CS_OK);
    EXPECT(cs_seg_agreement(masks.data(), masks.data(), 0, B, (int64_t)g * g, out.data(), nullptr) == CS_OK);
    free(ws);
    cs_seg_destroy(h);
}

int main() {
    CsSeg* h = nullptr;
    CsSegConfig bad = seg_config(32);
    EXPECT(cs_seg_create(nullptr, &h) != CS_OK);
    bad.size = 48; EXPECT(cs_seg_create(&bad, &h) == CS_E_SHAPE);                                    // not a multiple of 32
    bad = seg_config(32); bad.num_attention_heads[2] = 4; EXPECT(cs_seg_create(&bad, &h) == CS_E_UNSUPPORTED);
    bad = seg_config(32); bad.hidden_sizes[1] = 192; bad.num_attention_heads[1] = 3; EXPECT(cs_seg_create(&bad, &h) == CS_E_SHAPE);
    bad = seg_config(32); bad.sr_ratios[3] = 2; EXPECT(cs_seg_create(&bad, &h) == CS_E_SHAPE);        // a 1 x 1 grid has no 2 x 2 kernel
    run(32, 2);
    run(160, 1);
    {                                                                                                // finalize with a weight missing names it
        const CsSegConfig c = seg_config(32);
        EXPECT(cs_seg_create(&c, &h) == CS_OK);
        EXPECT(load_weights(h, cs_seg_num_weights(h) / 2) == CS_E_STATE && strstr(cs_last_error(), "missing weight"));
        cs_seg_destroy(h);
    }
    cs_seg_destroy(nullptr);
    if (g_fail) { fprintf(stderr, "seg sanitize harness: %d failures\n", g_fail); return 1; }
    printf("seg sanitize harness: ok\n");
    return 0;
}
