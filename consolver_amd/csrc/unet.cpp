// SD1.5 UNet2DConditionModel forward executor on top of the HIP ops (igemm / attention / norms).
//
// Replaces the third-party call `unet(latents, t, encoder_hidden_states=...)[0]`
// (denoise_ppo.py:89-94, gen_pretrain/pipeline.py:1058-1066; diffusers==0.26.3 UNet2DConditionModel
// with the SD1.5 config of SURVEY Appendix C).  Weights arrive by their diffusers state-dict names and
// are repacked once into MFMA-friendly fp16 layouts; activations are NHWC fp16 for the whole
// forward, so conv <-> transformer transitions are free ([B,H,W,C] == [B,HW,C]).
//
// Graph-level fusions done here (beyond the per-kernel epilogues):
//   * CFG dual batch without torch.cat: sample b reads latent b % n_lat in conv_in;
//   * skip-concat never materialised for the shortcut conv (two-source A operand); GroupNorm reads the
//     two sources and writes the single normalised tensor the 3x3 conv consumes;
//   * nearest-x2 upsample fused into the following conv's gather;
//   * q/k/v projections fused into one GEMM; cross-attention K/V of the text context (independent of
//     latents and timestep) cached across solver steps;
//   * all 22 time_emb_proj layers evaluated by one tiny-M linear over concatenated weights.
#include "weights.h"

#include <memory>
#include <cstring>
#include <cmath>

// the sub-pixel form of nearest-x2 upsample + 3x3 conv (pad 1): output pixel (2 y + py, 2 x + px) reads input rows {y - 1 + py, y + py} and columns
// {x - 1 + px, x + px}; neighbour (a, b) of phase (py, px) carries the SUM of the filter taps that land on it:
//   rows:    py = 0: a = 0 <- dy {0}, a = 1 <- dy {1, 2};    py = 1: a = 0 <- dy {0, 1}, a = 1 <- dy {2}       (same for columns with px, b, dx)
// w [N][9 Cin] (tap-major) -> out [4 phases = 2 py + px][N][4 Cin] (neighbour-major: 2 a + b), summed in fp32 and rounded to fp16 ONCE.
void conv_up_fold_pack_host(const f16* w, int N, int Cin, f16* out) {
    for (int ph = 0; ph < 4; ++ph) {
        const int py = ph >> 1, px = ph & 1;
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const int dy0 = py == 0 ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 2), dy1 = py == 0 ? (a == 0 ? 0 : 2) : (a == 0 ? 1 : 2);
                const int dx0 = px == 0 ? (b == 0 ? 0 : 1) : (b == 0 ? 0 : 2), dx1 = px == 0 ? (b == 0 ? 0 : 2) : (b == 0 ? 1 : 2);
                for (int n = 0; n < N; ++n) {
                    f16* dst = out + ((size_t)ph * N + n) * (4 * Cin) + (size_t)(2 * a + b) * Cin;
                    const f16* src = w + (size_t)n * (9 * Cin);
                    for (int c = 0; c < Cin; ++c) {
                        float acc = 0.f;
                        for (int dy = dy0; dy <= dy1; ++dy)
                            for (int dx = dx0; dx <= dx1; ++dx) acc += (float)src[(size_t)(dy * 3 + dx) * Cin + c];
                        dst[c] = (f16)acc;
                    }
                }
            }
    }
}

// LN(h) W^T + b = rstd (h W'^T - mean s) + b':  W' = fp16(W diag(gamma)), s = row sums of W' (of the ROUNDED values: it cancels exactly what the MFMAs summed),
// b' = W beta + b.  Host memory; w [N][K] fp16 rows, bias may be null.  Shared by the executor's weight packing and cs_op_ln_fold_pack.
void ln_fold_pack_host(const f16* w, const f16* bias, const f16* gamma, const f16* beta, int N, int K, f16* w_out, float* s_out, float* b_out) {
    for (int n = 0; n < N; ++n) {
        double s = 0.0, b = bias ? (double)(float)bias[n] : 0.0;
        for (int k = 0; k < K; ++k) {
            const float wk = (float)w[(size_t)n * K + k];
            const f16 r = (f16)(wk * (float)gamma[k]);
            w_out[(size_t)n * K + k] = r;
            s += (double)(float)r;
            b += (double)wk * (double)(float)beta[k];
        }
        s_out[n] = (float)s; b_out[n] = (float)b;
    }
}

namespace {

struct Resnet { Norm n1, n2; Conv c1, c2, sc; bool has_sc = false; int cin = 0, cout = 0, temb_off = 0; int sc_index = -1; };      // sc_index: position among the shortcut convs in creation order (knob x2_sc_skip)
struct LnLinear { f16* w = nullptr; float* s = nullptr; float* b = nullptr; };     // a linear layer with the LayerNorm in front of it folded in (IgemmArgs::ln_*)
struct Xformer {
    Norm gn, ln1, ln2, ln3;
    LnLinear f_qkv, f_q2, f_ff1;                                                    // norm1 -> to_q | to_k | to_v, norm2 -> attn2.to_q, norm3 -> GEGLU proj
    Conv proj_in, proj_out;
    f16 *wqkv = nullptr, *wo1 = nullptr, *bo1 = nullptr;
    f16 *wq2 = nullptr, *wkv2 = nullptr, *wo2 = nullptr, *bo2 = nullptr;
    f16 *wff1 = nullptr, *bff1 = nullptr, *wff2 = nullptr, *bff2 = nullptr;
    int c = 0; size_t kv_off = 0;   // offset (halfs, per batch row of 1 sample... scaled at run time) into the KV cache
    int index = 0;                  // position among the transformer blocks in creation order (cs_unet_calibrate_ln_fold: bit of ln_unfold_mask, slot of the calibration buffer)
};

// first-fit allocator over the caller's workspace (host bookkeeping only; deterministic, so the
// same sequence of calls yields the same addresses -> graph-capture safe)
struct Arena {
    char* base = nullptr; size_t cap = 0; bool dry = false; size_t peak = 0;
    struct Blk { size_t off, size; bool used; };
    std::vector<Blk> blks;
    void reset(char* b, size_t c, bool d) { base = b; cap = c; dry = d; peak = 0; blks.clear(); blks.push_back({0, d ? (size_t)1 << 46 : c, false}); }
    void* alloc(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        for (size_t i = 0; i < blks.size(); ++i) {
            if (!blks[i].used && blks[i].size >= bytes) {
                if (blks[i].size > bytes) { blks.insert(blks.begin() + i + 1, {blks[i].off + bytes, blks[i].size - bytes, false}); blks[i].size = bytes; }
                blks[i].used = true;
                peak = std::max(peak, blks[i].off + bytes);
                return base + blks[i].off;
            }
        }
        return nullptr;
    }
    void free(void* p) {
        if (!p) return;
        const size_t off = (char*)p - base;
        for (size_t i = 0; i < blks.size(); ++i) {
            if (blks[i].off == off && blks[i].used) {
                blks[i].used = false;
                if (i + 1 < blks.size() && !blks[i + 1].used) { blks[i].size += blks[i + 1].size; blks.erase(blks.begin() + i + 1); }
                if (i > 0 && !blks[i - 1].used) { blks[i - 1].size += blks[i].size; blks.erase(blks.begin() + i); }
                return;
            }
        }
    }
};

// A residual-stream tensor.  CS_RESIDUAL_F16: one fp16 plane, lo == nullptr.  CS_RESIDUAL_F16X2 (the default): value = hi + lo, two fp16 planes
// (22 significant bits): the epilogues that add onto the stream take hi + lo in fp32 and store both planes (IgemmArgs::res_lo / out_lo), the norms
// read hi + lo, and a GEMM that consumes the stream directly (shortcut 1x1, down / upsample conv, proj_out) reads the hi plane -- which is exactly
// the fp16 tensor of the one-plane mode, so no kernel's operand path changes.
// lo8 (round 6): the lo plane holds ONE BYTE per element (e5m2: the fp16 lo value rounded to its top byte, IgemmArgs::lo8) -- the transformer blocks' hidden state,
// whose lo plane is only ever added (to_out / cross-attention / feed-forward epilogues), never a GEMM operand.
struct St {
    f16* hi = nullptr; f16* lo = nullptr; bool lo8 = false;
    St() {}
    St(f16* h, f16* l = nullptr, bool l8 = false) : hi(h), lo(l), lo8(l8 && l) {}
    St at(size_t off) const { return St(hi + off, lo ? (lo8 ? reinterpret_cast<f16*>(reinterpret_cast<unsigned char*>(lo) + off) : lo + off) : nullptr, lo8); }
};

enum ProfClass { P_CONV3 = 0, P_GEMM, P_ATTN_SELF, P_ATTN_CROSS, P_GROUPNORM, P_LAYERNORM, P_MISC, P_COUNT };
const char* kProfNames[P_COUNT] = {"conv3x3_igemm", "gemm_1x1_linear", "attention_self", "attention_cross", "groupnorm_silu", "layernorm", "misc"};

}  // namespace

struct CsUNet {
    CsUNetConfig cfg;
    F16Store weights;                  // host staging in fp16: a tensor is rounded once, when it is set
    // packed
    Conv conv_in, conv_out; Norm norm_out;
    Conv conv_in64;                    // conv_in with the input channels zero-padded to 64 ([Cout][9][64]) for the MFMA path
    f16 *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
    f16 *tp_w = nullptr, *tp_b = nullptr; int tp_total = 0;
    std::vector<Resnet> down_res[4], up_res[4]; std::vector<Xformer> down_att[4], up_att[4];
    Conv down_samp[4], up_samp[4]; bool has_down[4] = {}, has_up[4] = {};
    Resnet mid_res[2]; Xformer mid_att;
    size_t kv_halfs_per_token = 0;
    int n_shortcuts = 0, n_xformers = 0;
    // cs_unet_calibrate_ln_fold: transformer blocks (bit = Xformer::index) whose LayerNorms run UNFOLDED (ln_kernel on hi + lo, plain GEMMs) although ln_fold is on: their
    // hidden states carry a DC offset of several sigma, where the folded form -- rstd (h_fp16 W' - mean s) -- cancels in fp16-rounded operands
    unsigned ln_unfold_mask = 0;
    float* calib = nullptr;             // device [3 * n_xformers] sums over rows of mean^2 / var (written only during a calibration forward)
    // run state
    Arena arena;
    bool profiling = false;
    struct Ev { int cls; hipEvent_t a, b; double flops, bytes; };
    std::vector<Ev> evs; size_t ev_used = 0;
    double prof_ms[P_COUNT] = {}, prof_flops[P_COUNT] = {}, prof_bytes[P_COUNT] = {}; int prof_launches[P_COUNT] = {};
    double dry_flops = 0;
    int residual = CS_RESIDUAL_F16X2;   // cs_unet_set_residual_precision (default: the mode that meets the 1e-3 latent gate)
    int out_dtype = CS_F16;             // cs_unet_set_output_dtype: CS_F16 (the model dtype, what the reference's UNet returns) or CS_F32 (the native engine's choice)
    std::map<std::string, int> tune;    // cs_unet_set_tuning: knob values THIS handle's forwards run with (on top of the process-wide cs_set_tuning state)
};

namespace {

void expect_tensor(CsUNet* u, const std::string& n, std::vector<int64_t> shape) { u->weights.expect(n, std::move(shape)); }

void expect_resnet(CsUNet* u, const std::string& p, int cin, int cout) {
    expect_tensor(u, p + ".norm1.weight", {cin}); expect_tensor(u, p + ".norm1.bias", {cin});
    expect_tensor(u, p + ".conv1.weight", {cout, cin, 3, 3}); expect_tensor(u, p + ".conv1.bias", {cout});
    expect_tensor(u, p + ".time_emb_proj.weight", {cout, 4 * u->cfg.block_out_channels[0]}); expect_tensor(u, p + ".time_emb_proj.bias", {cout});
    expect_tensor(u, p + ".norm2.weight", {cout}); expect_tensor(u, p + ".norm2.bias", {cout});
    expect_tensor(u, p + ".conv2.weight", {cout, cout, 3, 3}); expect_tensor(u, p + ".conv2.bias", {cout});
    if (cin != cout) { expect_tensor(u, p + ".conv_shortcut.weight", {cout, cin, 1, 1}); expect_tensor(u, p + ".conv_shortcut.bias", {cout}); }
}

void expect_xformer(CsUNet* u, const std::string& p, int c) {
    const int cd = u->cfg.cross_attention_dim;
    expect_tensor(u, p + ".norm.weight", {c}); expect_tensor(u, p + ".norm.bias", {c});
    expect_tensor(u, p + ".proj_in.weight", {c, c, 1, 1}); expect_tensor(u, p + ".proj_in.bias", {c});
    const std::string t = p + ".transformer_blocks.0";
    for (const char* ln : {".norm1", ".norm2", ".norm3"}) { expect_tensor(u, t + ln + ".weight", {c}); expect_tensor(u, t + ln + ".bias", {c}); }
    for (const char* q : {".attn1.to_q.weight", ".attn1.to_k.weight", ".attn1.to_v.weight", ".attn1.to_out.0.weight"}) expect_tensor(u, t + q, {c, c});
    expect_tensor(u, t + ".attn1.to_out.0.bias", {c});
    expect_tensor(u, t + ".attn2.to_q.weight", {c, c});
    expect_tensor(u, t + ".attn2.to_k.weight", {c, cd}); expect_tensor(u, t + ".attn2.to_v.weight", {c, cd});
    expect_tensor(u, t + ".attn2.to_out.0.weight", {c, c}); expect_tensor(u, t + ".attn2.to_out.0.bias", {c});
    expect_tensor(u, t + ".ff.net.0.proj.weight", {8 * c, c}); expect_tensor(u, t + ".ff.net.0.proj.bias", {8 * c});
    expect_tensor(u, t + ".ff.net.2.weight", {c, 4 * c}); expect_tensor(u, t + ".ff.net.2.bias", {c});
    expect_tensor(u, p + ".proj_out.weight", {c, c, 1, 1}); expect_tensor(u, p + ".proj_out.bias", {c});
}

// channel bookkeeping of the diffusers UNet: (in, out) of every resnet in order
struct Topology {
    std::vector<std::pair<int, int>> down[4], up[4];
    std::vector<int> skip_ch;   // channels of the skip stack in push order
};

Topology topology(const CsUNetConfig& c) {
    Topology t;
    const int* bc = c.block_out_channels;
    int ch = bc[0];
    t.skip_ch.push_back(ch);
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < c.layers_per_block; ++j) { t.down[i].push_back({ch, bc[i]}); ch = bc[i]; t.skip_ch.push_back(ch); }
        if (i < 3) t.skip_ch.push_back(ch);
    }
    std::vector<int> skips = t.skip_ch;
    int rev[4] = {bc[3], bc[2], bc[1], bc[0]};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            const int sk = skips.back(); skips.pop_back();
            t.up[i].push_back({ch + sk, rev[i]});   // concat(h, skip)
            ch = rev[i];
        }
    }
    return t;
}

void build_manifest(CsUNet* u) {
    const CsUNetConfig& c = u->cfg;
    const int c0 = c.block_out_channels[0], td = 4 * c0;
    expect_tensor(u, "conv_in.weight", {c0, c.in_channels, 3, 3}); expect_tensor(u, "conv_in.bias", {c0});
    expect_tensor(u, "time_embedding.linear_1.weight", {td, c0}); expect_tensor(u, "time_embedding.linear_1.bias", {td});
    expect_tensor(u, "time_embedding.linear_2.weight", {td, td}); expect_tensor(u, "time_embedding.linear_2.bias", {td});
    Topology t = topology(c);
    for (int i = 0; i < 4; ++i) {
        const std::string b = "down_blocks." + std::to_string(i);
        for (size_t j = 0; j < t.down[i].size(); ++j) {
            expect_resnet(u, b + ".resnets." + std::to_string(j), t.down[i][j].first, t.down[i][j].second);
            if (c.down_has_attn[i]) expect_xformer(u, b + ".attentions." + std::to_string(j), c.block_out_channels[i]);
        }
        if (i < 3) { const int ch = c.block_out_channels[i]; expect_tensor(u, b + ".downsamplers.0.conv.weight", {ch, ch, 3, 3}); expect_tensor(u, b + ".downsamplers.0.conv.bias", {ch}); }
    }
    const int cm = c.block_out_channels[3];
    expect_resnet(u, "mid_block.resnets.0", cm, cm);
    expect_xformer(u, "mid_block.attentions.0", cm);
    expect_resnet(u, "mid_block.resnets.1", cm, cm);
    for (int i = 0; i < 4; ++i) {
        const std::string b = "up_blocks." + std::to_string(i);
        const int ch = c.block_out_channels[3 - i];
        for (size_t j = 0; j < t.up[i].size(); ++j) {
            expect_resnet(u, b + ".resnets." + std::to_string(j), t.up[i][j].first, t.up[i][j].second);
            if (c.up_has_attn[i]) expect_xformer(u, b + ".attentions." + std::to_string(j), ch);
        }
        if (i < 3) { expect_tensor(u, b + ".upsamplers.0.conv.weight", {ch, ch, 3, 3}); expect_tensor(u, b + ".upsamplers.0.conv.bias", {ch}); }
    }
    expect_tensor(u, "conv_norm_out.weight", {c0}); expect_tensor(u, "conv_norm_out.bias", {c0});
    expect_tensor(u, "conv_out.weight", {c.out_channels, c0, 3, 3}); expect_tensor(u, "conv_out.bias", {c.out_channels});
}

// ------------------------------------------------------------------------- packing helpers
std::vector<f16> concat_rows(std::initializer_list<const HostTensor<f16>*> ts) {
    std::vector<f16> o;
    for (auto t : ts) o.insert(o.end(), t->data.begin(), t->data.end());
    return o;
}
bool make_resnet(CsUNet* u, const std::string& p, Resnet& r, std::vector<f16>& tpw, std::vector<f16>& tpb) {
    F16Store& W = u->weights;
    bool ok = make_norm(W, p + ".norm1", r.n1, 1e-5f) && make_conv(W, p + ".conv1", r.c1) && make_norm(W, p + ".norm2", r.n2, 1e-5f) &&
              make_conv(W, p + ".conv2", r.c2);
    r.cin = r.c1.cin; r.cout = r.c1.cout;
    r.has_sc = W.host.count(p + ".conv_shortcut.weight") > 0;
    if (r.has_sc) { ok = ok && make_conv(W, p + ".conv_shortcut", r.sc); r.sc_index = u->n_shortcuts++; }
    r.temb_off = (int)tpb.size();
    const HostTensor<f16>& tw = W.at(p + ".time_emb_proj.weight");
    tpw.insert(tpw.end(), tw.data.begin(), tw.data.end());
    const HostTensor<f16>& tb = W.at(p + ".time_emb_proj.bias");
    tpb.insert(tpb.end(), tb.data.begin(), tb.data.end());
    return ok;
}
// LN(h) W^T + b = rstd (h W'^T - mean s) + b':  W' = fp16(W diag(gamma)), s = row sums of W' (of the ROUNDED values: it cancels exactly what the MFMAs summed),
// b' = W beta + b.  w: [N][K] fp16 rows, bias may be empty.
bool make_ln_linear(F16Store& W, const std::vector<f16>& w, const std::vector<f16>& bias, const HostTensor<f16>& gamma, const HostTensor<f16>& beta, int N, int K, LnLinear& out) {
    std::vector<f16> wf((size_t)N * K);
    std::vector<float> sv(N), bv(N);
    ln_fold_pack_host(w.data(), bias.empty() ? nullptr : bias.data(), gamma.data.data(), beta.data.data(), N, K, wf.data(), sv.data(), bv.data());
    out.w = W.upload(wf); out.s = W.upload_f32(sv); out.b = W.upload_f32(bv);
    return out.w && out.s && out.b;
}

bool make_xformer(CsUNet* u, const std::string& p, Xformer& x) {
    F16Store& W = u->weights;
    const std::string t = p + ".transformer_blocks.0";
    bool ok = make_norm(W, p + ".norm", x.gn, 1e-6f) && make_conv(W, p + ".proj_in", x.proj_in) && make_conv(W, p + ".proj_out", x.proj_out) &&
              make_norm(W, t + ".norm1", x.ln1, 1e-5f) && make_norm(W, t + ".norm2", x.ln2, 1e-5f) && make_norm(W, t + ".norm3", x.ln3, 1e-5f);
    x.c = x.gn.c;
    const std::vector<f16> wqkv_h = concat_rows({&W.at(t + ".attn1.to_q.weight"), &W.at(t + ".attn1.to_k.weight"), &W.at(t + ".attn1.to_v.weight")});
    x.wqkv = W.upload(wqkv_h);
    ok = ok && make_ln_linear(W, wqkv_h, {}, W.at(t + ".norm1.weight"), W.at(t + ".norm1.bias"), 3 * x.c, x.c, x.f_qkv) &&
         make_ln_linear(W, W.at(t + ".attn2.to_q.weight").data, {}, W.at(t + ".norm2.weight"), W.at(t + ".norm2.bias"), x.c, x.c, x.f_q2);
    x.wo1 = W.upload(W.at(t + ".attn1.to_out.0.weight").data); x.bo1 = W.upload(W.at(t + ".attn1.to_out.0.bias").data);
    x.wq2 = W.upload(W.at(t + ".attn2.to_q.weight").data);
    x.wkv2 = W.upload(concat_rows({&W.at(t + ".attn2.to_k.weight"), &W.at(t + ".attn2.to_v.weight")}));
    x.wo2 = W.upload(W.at(t + ".attn2.to_out.0.weight").data); x.bo2 = W.upload(W.at(t + ".attn2.to_out.0.bias").data);
    // GEGLU: rows [0,4C) value, [4C,8C) gate  ->  blocks of (16 value | 16 gate) rows
    const HostTensor<f16>& w1 = W.at(t + ".ff.net.0.proj.weight"); const HostTensor<f16>& b1 = W.at(t + ".ff.net.0.proj.bias");
    const int64_t C = x.c, H4 = 4 * C;
    std::vector<f16> pw((size_t)8 * C * C), pb((size_t)8 * C);
    for (int64_t P = 0; P < H4 / 16; ++P)
        for (int64_t i = 0; i < 16; ++i) {
            std::memcpy(&pw[(32 * P + i) * C], &w1.data[(16 * P + i) * C], C * sizeof(f16));
            std::memcpy(&pw[(32 * P + 16 + i) * C], &w1.data[(H4 + 16 * P + i) * C], C * sizeof(f16));
            pb[32 * P + i] = b1.data[16 * P + i]; pb[32 * P + 16 + i] = b1.data[H4 + 16 * P + i];
        }
    x.wff1 = W.upload(pw); x.bff1 = W.upload(pb);
    ok = ok && make_ln_linear(W, pw, pb, W.at(t + ".norm3.weight"), W.at(t + ".norm3.bias"), (int)(8 * C), (int)C, x.f_ff1);      // (row-wise: commutes with the GEGLU row permutation)
    x.wff2 = W.upload(W.at(t + ".ff.net.2.weight").data); x.bff2 = W.upload(W.at(t + ".ff.net.2.bias").data);
    x.kv_off = u->kv_halfs_per_token; u->kv_halfs_per_token += 2 * (size_t)x.c;
    x.index = u->n_xformers++;
    return ok && x.wqkv && x.wo1 && x.bo1 && x.wq2 && x.wkv2 && x.wo2 && x.bo2 && x.wff1 && x.bff1 && x.wff2 && x.bff2;
}

// ------------------------------------------------------------------------- run context
struct Run {
    CsUNet* u;
    const TuneSet& knobs;          // this call's knobs (run_forward installs the same set for the launchers)
    hipStream_t s; bool dry; int B; int rc = CS_OK;
    const f16* ctx = nullptr; f16* kv = nullptr; const f16* tproj = nullptr; int tstride = 0;
    float* gn_ws = nullptr;
    float* sk_ws = nullptr; size_t sk_bytes = 0;
    bool split = false;            // CS_RESIDUAL_F16X2: residual-stream tensors carry a lo plane
    // the transformer hidden state's lo plane as bytes: only where every consumer of that plane adds it (folded LayerNorms: ln_kernel reads an fp16 lo plane;
    // proj_out not reading hi + lo as its operand)
    bool fold_of(const Xformer& X) const { return knobs.ln_fold != 0 && !((u->ln_unfold_mask >> X.index) & 1u); }
    bool h_lo8(bool fold) const { return split && knobs.lo8 != 0 && fold && !(knobs.x2_split_a & 2); }
    St salloc_h(size_t elems, bool fold) { St t; t.hi = alloc(elems); t.lo8 = h_lo8(fold); t.lo = split ? alloc(t.lo8 ? (elems + 1) / 2 : elems) : nullptr; return t; }
    float* calib = nullptr;        // calibration forward: per (block, LayerNorm) sums of mean^2 / var over the rows of the hidden state in front of that LayerNorm
    void calib_point(const Xformer& X, int which, const float* rs, int M, int G, int C, float eps) {
        if (!calib || !rs) return;
        float* dst = calib + 3 * X.index + which;
        launch(P_MISC, 0, 0, [&] { return launch_ln_dc_ratio(rs, M, G, C, eps, dst, s); });
    }
    bool count_executed = false;   // dry run behind cs_unet_flops_executed: count what is ISSUED (padding included), not the reference graph's FLOPs
    // row statistics [M][<= C / 64 groups][2] floats a producer leaves for a folded LayerNorm (IgemmArgs::row_stats)
    float* alloc_rowstats(int M, int C) { return (float*)alloc((size_t)M * (C / 64) * 2 * 2); }

    f16* alloc(size_t halfs) {
        void* p = u->arena.alloc(halfs * sizeof(f16));
        if (!p && rc == CS_OK) {
            cs_set_error("unet: workspace too small (request %zu B, arena %zu B, peak so far %zu B, batch %d)", halfs * sizeof(f16), u->arena.cap,
                         u->arena.peak, B);
            rc = CS_E_ARG;
        }
        // after a failed allocation nothing is launched any more (rc), but the walk goes on taking offsets from what it got: hand out a poison
        // base that is never dereferenced instead of null (offsets from a null pointer are undefined behaviour)
        return p ? (f16*)p : reinterpret_cast<f16*>((uintptr_t)1 << 41);
    }
    // GroupNorm statistics a producer left for a tensor (IgemmArgs::gn_stats): tensor -> partial sums, alive as long as the tensor
    struct StatRec { float* stats; int S; };
    std::map<const void*, StatRec> stat_of;
    void release(const void* p) {
        auto it = stat_of.find(p);
        if (it != stat_of.end()) { u->arena.free(it->second.stats); stat_of.erase(it); }
        u->arena.free(const_cast<void*>(p));
    }
    // residual-stream tensors: hi plane (+ lo plane in the split mode)
    St salloc(size_t halfs) { St t; t.hi = alloc(halfs); t.lo = split ? alloc(halfs) : nullptr; return t; }
    void srelease(const St& t) { release(t.hi); u->arena.free(t.lo); }
    bool stats_fusable(int HW, int C) const { return knobs.gn_fuse != 0 && HW % 64 == 0 && C % 2 == 0; }
    // partial-sum buffer for a [Bt][HW][C] tensor about to be produced (Bt samples); registered under `out` by the caller
    float* alloc_stats(int Bt, int HW, int C) { return (float*)alloc((size_t)Bt * (HW / 64) * C * 2); }      // C/2 pairs x 2 floats = C floats = 2C halfs

    // one launch's lo planes are of one kind (IgemmArgs::lo8 covers res_lo and out_lo): mixing them is an executor bug, caught here
    int lo8_of(const St& res, const St& out) {
        if (res.lo && out.lo && res.lo8 != out.lo8 && rc == CS_OK) { cs_set_error("unet: a launch with an fp16 and an 8-bit lo plane"); rc = CS_E_STATE; }
        return ((res.lo && res.lo8) || (out.lo && out.lo8)) ? 1 : 0;
    }
    template <typename F> void launch(int cls, double flops, double bytes, F&& f) {
        if (dry) { u->dry_flops += flops; return; }
        if (rc != CS_OK) return;
        if (u->profiling) {
            if (u->ev_used == u->evs.size()) { CsUNet::Ev e; e.cls = cls; hipEventCreate(&e.a); hipEventCreate(&e.b); u->evs.push_back(e); }
            CsUNet::Ev& e = u->evs[u->ev_used++]; e.cls = cls; e.flops = flops; e.bytes = bytes;
            hipEventRecord(e.a, s);
            rc = f();
            hipEventRecord(e.b, s);
        } else {
            rc = f();
        }
    }
    // a device-to-device copy on the stream, under the same rule as a launch (none in a dry run or after an error); a failed one fails the forward
    void copy(void* dst, const void* src, size_t bytes) {
        if (dry || rc != CS_OK) return;
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) { cs_set_error("unet: device copy of %zu B failed: %s", bytes, hipGetErrorString(e)); rc = CS_E_HIP; }
    }

    // want_stats: the output feeds a GroupNorm (or a skip connection that does): its statistics come out of the epilogue.
    // stats_into: write them into this (larger) buffer instead of a fresh one, nothing registered (two launches filling one tensor).
    void conv(const Conv& c, const f16* a0, int c0, const f16* a1, int c1, int Hi, int Wi, int Ho, int Wo, int stride, int up,
              const f16* temb, St res, St out, bool want_stats = false, float* stats_into = nullptr, const f16* a0_lo = nullptr, const f16* a1_lo = nullptr,
              float* row_stats = nullptr, int* row_groups = nullptr, double algo_flops = -1.0) {
        IgemmArgs a{};
        a.a0_lo = a0_lo; a.a1_lo = a0_lo ? a1_lo : nullptr;
        a.row_stats = row_stats; a.row_stats_groups = row_groups;
        if (stats_into) a.gn_stats = stats_into;
        else if (want_stats && stats_fusable(Ho * Wo, c.cout)) {
            a.gn_stats = alloc_stats(B, Ho * Wo, c.cout);
            if (a.gn_stats) stat_of[out.hi] = {a.gn_stats, Ho * Wo / 64};
        }
        a.a0 = a0; a.a1 = a1; a.c0 = c0; a.c1 = c1; a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.taps = c.taps; a.stride = stride;
        a.upsample = up; a.N = c.cout; a.w = c.w; a.bias = c.b; a.temb = temb; a.temb_stride = tstride; a.res = res.hi; a.out = out.hi; a.geglu = 0;
        a.res_lo = res.lo; a.out_lo = out.lo; a.lo8 = lo8_of(res, out);
        a.splitk_ws = sk_ws; a.splitk_ws_bytes = sk_bytes;
        // an upsampler in its sub-pixel form: pre-summed taps are one more fp16 rounding of the weights (~2^-12 of the output, straight onto the stream):
        // in the forwards that run on one fp16 plane, whose stream is rounded to fp16 sixty times anyway; the split stream keeps the exact filter.
        // Whether the shape takes that form is the launcher's rule (igemm_sub_pixel), which the executed-FLOP count asks too
        if (up && c.w_sub && (knobs.up_fold == 2 || (knobs.up_fold == 1 && !split)) && !res.hi && !temb) a.w_up_sub = c.w_sub;
        const double M = (double)B * Ho * Wo;
        const double bytes = 2.0 * (M * (c0 + c1) + (double)c.cout * c.taps * (c0 + c1) + M * c.cout * ((res.hi ? 2 : 1) + (res.lo ? 1 : 0) + (out.lo ? 1 : 0)));
        // algo_flops: the REFERENCE graph's count for this layer where the executed form pads it (conv_in on the MFMA conv runs 64 input channels for 4):
        // cs_unet_flops is the algorithmic count of SURVEY 8(d), independent of how a layer is executed
        launch(c.taps == 9 ? P_CONV3 : P_GEMM, (algo_flops >= 0 && !count_executed) ? algo_flops : igemm_flops(a) * ((count_executed && a.a0_lo) ? 2.0 : (count_executed && igemm_sub_pixel(a, knobs)) ? 4.0 / 9.0 : 1.0), bytes, [&] { return launch_igemm(a, s); });
    }
    void linear(const f16* x, int M, int K, const f16* w, const f16* b, int N, St res, St out, int geglu, float* row_stats = nullptr, int* row_groups = nullptr) {
        IgemmArgs a{};
        a.row_stats = row_stats; a.row_stats_groups = row_groups;
        a.a0 = x; a.c0 = K; a.B = 1; a.Hi = M; a.Wi = 1; a.Ho = M; a.Wo = 1; a.taps = 1; a.stride = 1; a.N = N; a.w = w; a.bias = b; a.res = res.hi; a.out = out.hi; a.geglu = geglu;
        a.res_lo = res.lo; a.out_lo = out.lo; a.lo8 = lo8_of(res, out);
        a.splitk_ws = sk_ws; a.splitk_ws_bytes = sk_bytes;
        const double lob = a.lo8 ? 0.5 : 1.0;                // (a lo8 plane is half the bytes of an fp16 one)
        const double bytes = 2.0 * ((double)M * K + (double)N * K + (double)M * (geglu ? N / 2 : N) * ((res.hi ? 2 : 1) + (res.lo ? lob : 0) + (out.lo ? lob : 0)));
        launch(P_GEMM, igemm_flops(a), bytes, [&] { return launch_igemm(a, s); });
    }
    // out = LayerNorm(h) W^T + b with the LayerNorm folded in: x is the RAW hidden state (hi plane), stats / G what its producer left
    void linear_ln(const f16* x, int M, int K, const LnLinear& L, const float* stats, int G, float eps, int N, f16* out, int geglu) {
        IgemmArgs a{};
        a.a0 = x; a.c0 = K; a.B = 1; a.Hi = M; a.Wi = 1; a.Ho = M; a.Wo = 1; a.taps = 1; a.stride = 1; a.N = N; a.w = L.w; a.out = out; a.geglu = geglu;
        a.ln_stats = stats; a.ln_groups = G; a.ln_eps = eps; a.ln_s = L.s; a.ln_b = L.b;
        a.splitk_ws = sk_ws; a.splitk_ws_bytes = sk_bytes;
        const double bytes = 2.0 * ((double)M * K + (double)N * K + (double)M * (geglu ? N / 2 : N));
        launch(P_GEMM, igemm_flops(a), bytes, [&] { return launch_igemm(a, s); });
    }
    void group_norm(const Norm& n, St s0, int c0, St s1, int c1, int HW, bool silu, f16* out, f16* out_lo = nullptr) {
        GroupNormArgs a{};
        a.out_lo = out_lo;
        const f16* x0 = s0.hi; const f16* x1 = s1.hi;
        a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1; a.x0_lo = s0.lo; a.x1_lo = s1.lo; a.B = B; a.HW = HW; a.groups = u->cfg.norm_num_groups; a.eps = n.eps; a.silu = silu;
        a.gamma = n.g; a.beta = n.b; a.partial = gn_ws; a.out = out;
        auto i0 = stat_of.find(x0);
        if (i0 != stat_of.end()) { a.stats0 = i0->second.stats; a.S0 = i0->second.S; }
        auto i1 = x1 ? stat_of.find(x1) : stat_of.end();
        if (i1 != stat_of.end()) { a.stats1 = i1->second.stats; a.S1 = i1->second.S; }
        const double passes = 2.0 + ((a.stats0 ? 0.0 : (double)c0) + (x1 && !a.stats1 ? (double)c1 : 0.0) + (s0.lo ? (double)c0 : 0.0) + (s1.lo ? (double)c1 : 0.0)) / (double)(c0 + c1);
        launch(P_GROUPNORM, 0, 2.0 * passes * B * HW * (double)(c0 + c1), [&] { return launch_group_norm(a, s); });
    }
    void layer_norm(const Norm& n, St x, int M, f16* out) {
        launch(P_LAYERNORM, 0, 2.0 * (x.lo ? 3.0 : 2.0) * M * (double)n.c, [&] { return launch_layer_norm(x.hi, n.g, n.b, out, M, n.c, n.eps, s, x.lo); });
    }
    void attention(bool cross, const f16* q, int qs, const f16* k, int ks, const f16* v, int vs, f16* out, int os, int Nq, int Nk, int C) {
        AttnArgs a{};
        a.q = q; a.q_stride = qs; a.k = k; a.k_stride = ks; a.v = v; a.v_stride = vs; a.out = out; a.out_stride = os;
        a.B = B; a.H = u->cfg.num_heads; a.Nq = Nq; a.Nk = Nk; a.dh = C / u->cfg.num_heads; a.scale = 1.0f / sqrtf((float)a.dh);
        const double fl = 4.0 * B * (double)Nq * Nk * C;
        launch(cross ? P_ATTN_CROSS : P_ATTN_SELF, fl, 2.0 * B * ((double)Nq * C * 2 + (double)Nk * C * 2), [&] { return launch_attention(a, s); });
    }

    // fused LN2 -> to_q -> cross attention -> to_out + residual (xattn.hip); h_in may equal h_out
    // (an UNFOLDED block -- cs_unet_calibrate_ln_fold: DC-heavy hidden state -- also leaves the fused kernel: its LayerNorm reads the hi plane, the LayerNorm kernel hi + lo)
    bool xattn_fusable(const Xformer& X, int HW) const {
        return knobs.xattn_fused != 0 && X.c == 320 && u->cfg.num_heads == 8 && HW % 128 == 0 && u->cfg.ctx_len <= 80 && !((u->ln_unfold_mask >> X.index) & 1u);
    }
    void xattn_fused(const Xformer& X, St h_in, St h_out, const f16* kvl, int HW, float* row_stats = nullptr) {
        XattnArgs a{};
        a.row_stats = row_stats;
        a.h = h_in.hi; a.out = h_out.hi; a.h_lo = h_in.lo; a.out_lo = h_out.lo; a.lo8 = lo8_of(h_in, h_out); a.ln_g = X.ln2.g; a.ln_b = X.ln2.b; a.ln_eps = X.ln2.eps; a.wq = X.wq2; a.wo = X.wo2; a.bo = X.bo2; a.kv = kvl;
        a.M = B * HW; a.HW = HW; a.Nk = u->cfg.ctx_len; a.C = X.c; a.heads = u->cfg.num_heads; a.scale = 1.0f / sqrtf((float)(X.c / u->cfg.num_heads));
        const double M = (double)B * HW, fl = 4.0 * M * X.c * X.c + 4.0 * M * u->cfg.ctx_len * X.c;
        launch(P_ATTN_CROSS, fl, 2.0 * ((h_in.lo ? (a.lo8 ? 4.0 : 5.0) : 3.0) * M * X.c), [&] { return launch_xattn_block(a, s); });
    }

    // x: [B,HW,Cx] (+ optional skip [B,HW,Cs]) -> new tensor [B,HW,Cout]
    St resnet(const Resnet& r, St x, int cx, St skip, int cs, int H, int W) {
        const int HW = H * W; const size_t M = (size_t)B * HW;
        f16* n1 = alloc(M * (cx + cs));
        group_norm(r.n1, x, cx, skip, cs, HW, true, n1);
        f16* h1 = alloc(M * r.cout);
        conv(r.c1, n1, cx + cs, nullptr, 0, H, W, H, W, 1, 0, tproj + r.temb_off, St(), St(h1), true);      // -> norm2
        release(n1);
        f16* n2 = alloc(M * r.cout);
        group_norm(r.n2, St(h1), r.cout, St(), 0, HW, true, n2);
        release(h1);
        St out = salloc(M * r.cout);
        St res = x;
        if (r.has_sc) {                                      // split mode: the 1x1 multiplies hi + lo of [x | skip] (two passes of its k loop over the same weights)
            // (x2_sc_skip: the shortcuts whose hi + lo operand buys the least per microsecond read the hi plane only -- tools/sim_precision_r06.py)
            const bool sa = split && (knobs.x2_split_a & 1) && !((knobs.x2_sc_skip >> r.sc_index) & 1) && x.lo && (!cs || skip.lo);
            conv(r.sc, x.hi, cx, skip.hi, cs, H, W, H, W, 1, 0, nullptr, St(), out, false, nullptr, sa ? x.lo : nullptr, sa ? skip.lo : nullptr);
            res = out;
        }
        conv(r.c2, n2, r.cout, nullptr, 0, H, W, H, W, 1, 0, nullptr, res, out, true);                     // -> the next block's GroupNorm / a skip
        release(n2);
        return out;
    }

    // ---- transformer block; in-place on a fresh output: returns new tensor [B,HW,C] ----------------------------------------------------------------------
    // CFG dual batch, shared prefix (n_share = n_lat > 0): with classifier-free guidance the two halves of the batch (unconditional | text,
    // gen_pretrain/pipeline.py:1054) carry the SAME latents and the same timestep; they differ only in the text context, which first enters at the
    // cross-attention of the first transformer block.  Everything before that point -- conv_in, the first resnet, and GroupNorm / proj_in / LayerNorm / QKV /
    // self-attention / to_out / LayerNorm2 / to_q of the first transformer block -- is the same function of the same inputs for sample b and sample b + n_lat,
    // so it is computed once at batch n_lat (x: ONE half) and the residual stream is duplicated right before the two halves diverge.  Bit-identical to running
    // the full batch (the kernels are batch-independent per sample); ~1/32 of the forward's FLOPs are not executed.
    // (The allocation sequence of each case is what cs_unet_workspace_bytes measured: the first-fit arena's peak depends on it.)
    St xformer(const Xformer& X, St x, int H, int W, int n_share = 0) {
        const int C = X.c, HW = H * W, L = u->cfg.ctx_len;
        const int Bfull = B, Bp = n_share ? n_share : B, halves = n_share ? 2 : 1;     // Bp: the batch of the prefix and of each half's own launches
        const int M = Bfull * HW, M1 = Bp * HW;
        B = Bp;
        f16* g = alloc((size_t)M1 * C);
        group_norm(X.gn, x, C, St(), 0, HW, false, g);
        // folded LayerNorms: every layer that writes the hidden state leaves its row statistics in rs (G column groups), the next LayerNorm's consumer reads them
        const bool fold = fold_of(X);
        St h = salloc_h((size_t)M1 * C, fold);
        float* rs = fold ? alloc_rowstats(M, C) : nullptr; int G = 1;                  // (full batch: the halves' statistics land side by side later)
        conv(X.proj_in, g, C, nullptr, 0, H, W, H, W, 1, 0, nullptr, St(), h, false, nullptr, nullptr, nullptr, rs, &G);
        calib_point(X, 0, rs, M1, G, C, X.ln1.eps);
        // self attention
        f16* qkv = alloc((size_t)M1 * 3 * C);
        if (fold) linear_ln(h.hi, M1, C, X.f_qkv, rs, G, X.ln1.eps, 3 * C, qkv, 0);
        else { layer_norm(X.ln1, h, M1, g); linear(g, M1, C, X.wqkv, nullptr, 3 * C, St(), St(qkv), 0); }
        attention(false, qkv, 3 * C, qkv + C, 3 * C, qkv + 2 * C, 3 * C, g, C, HW, HW, C);
        release(qkv);
        linear(g, M1, C, X.wo1, X.bo1, C, h, h, 0, rs, &G);
        // cross attention (K/V of the text context are cached in kv): the fused sub-block runs its own norm2 / to_q inside the kernel and leaves the statistics
        // norm3's consumer needs; the unfused one runs to_q on the prefix
        const bool fused = xattn_fusable(X, HW);
        f16* q = nullptr;
        if (!fused) {
            calib_point(X, 1, rs, M1, G, C, X.ln2.eps);
            q = alloc((size_t)M1 * C);
            if (fold) linear_ln(h.hi, M1, C, X.f_q2, rs, G, X.ln2.eps, C, q, 0);
            else { layer_norm(X.ln2, h, M1, g); linear(g, M1, C, X.wq2, nullptr, C, St(), St(q), 0); }
        }
        // ---- the halves diverge: each half attends to its own K/V on its own copy of the residual stream (the fused sub-block reads the shared stream and
        // writes each half's copy: no duplication copy)
        const St hp = h;
        if (n_share) { release(g); h = salloc_h((size_t)M * C, fold); g = alloc((size_t)M * C); }
        const f16* kvl = kv + X.kv_off * (size_t)Bfull * L;
        for (int half = 0; half < halves; ++half) {
            const size_t o = (size_t)half * M1 * C;
            const f16* kvh = kvl + (size_t)half * Bp * L * 2 * C;
            if (fused) {
                xattn_fused(X, hp, h.at(o), kvh, HW, rs ? rs + (size_t)half * M1 * 2 : nullptr);
            } else {
                if (n_share) { copy(h.hi + o, hp.hi, (size_t)M1 * C * sizeof(f16)); if (h.lo) copy(h.at(o).lo, hp.lo, (size_t)M1 * C * (h.lo8 ? 1 : sizeof(f16))); }
                attention(true, q, C, kvh, 2 * C, kvh + C, 2 * C, g + o, C, HW, L, C);
            }
        }
        if (q) release(q);
        if (n_share) srelease(hp);
        B = Bfull;
        if (fused) G = 1;
        else linear(g, M, C, X.wo2, X.bo2, C, h, h, 0, rs, &G);
        // feed forward (GEGLU fused into the first GEMM's epilogue)
        calib_point(X, 2, rs, M, G, C, X.ln3.eps);
        f16* ff = alloc((size_t)M * 4 * C);
        if (fold) linear_ln(h.hi, M, C, X.f_ff1, rs, G, X.ln3.eps, 8 * C, ff, 1);
        else { layer_norm(X.ln3, h, M, g); linear(g, M, C, X.wff1, X.bff1, 8 * C, St(), St(ff), 1); }
        const bool po = split && (knobs.x2_split_a & 2);
        linear(ff, M, 4 * C, X.wff2, X.bff2, C, h, po ? h : St(h.hi), 0);      // the hidden after the feed-forward has one consumer, proj_out's operand: hi plane only unless proj_out reads hi + lo
        release(ff);
        // proj_out + residual with the block input, which exists once per half: one launch per half, one statistics buffer for the full batch
        St out(g, split ? alloc((size_t)M * C) : nullptr);
        float* st = stats_fusable(HW, C) ? alloc_stats(Bfull, HW, C) : nullptr;
        B = Bp;
        for (int half = 0; half < halves; ++half) {
            const size_t o = (size_t)half * M1 * C;
            conv(X.proj_out, h.hi + o, C, nullptr, 0, H, W, H, W, 1, 0, nullptr, x, out.at(o), false, st ? st + (size_t)half * Bp * (HW / 64) * C : nullptr,
                 po ? h.lo + o : nullptr);
        }
        B = Bfull;
        if (st) stat_of[g] = {st, HW / 64};
        srelease(h); u->arena.free(rs);
        return out;
    }
};

size_t kv_cache_bytes(const CsUNet* u, int B) { return ((u->kv_halfs_per_token * (size_t)B * u->cfg.ctx_len * sizeof(f16)) + 255) & ~(size_t)255; }
size_t sk_ws_bytes(const CsUNet*, int B) { return ((size_t)B * (8u << 20)) + (16u << 20); }
size_t gn_ws_bytes(const CsUNet* u, int B) {
    const int cmax = 2 * u->cfg.block_out_channels[3];
    return (((size_t)B * (GN_SPLITS + 1) * cmax * 2 * sizeof(float)) + 255) & ~(size_t)255;
}

// the knobs one call of this handle runs with: one copy of the process-wide set, the handle's own overrides on top
TuneSet handle_tune(const CsUNet* u) {
    TuneSet k = tune_snapshot();
    for (auto& kv : u->tune) tune_apply(k, kv.first.c_str(), kv.second);
    return k;
}

// k: the knobs of the whole forward, for the executor and (installed here) every launcher it calls
int run_forward(CsUNet* u, const TuneSet& k, bool dry, const f16* latents, int n_lat, int dup, const float* t, int nt, const f16* ctx, f16* out,
                char* ws, size_t ws_bytes, int kv_valid, hipStream_t s, bool count_executed = false, float* calib = nullptr) {
    TuneScope scope(&k);
    const CsUNetConfig& c = u->cfg;
    const int B = n_lat * dup;
    const size_t kvb = kv_cache_bytes(u, B), gnb = gn_ws_bytes(u, B) + sk_ws_bytes(u, B);
    if (!dry && ws_bytes < kvb + gnb) CS_FAIL(CS_E_ARG, "unet: workspace too small (%zu < %zu)", ws_bytes, kvb + gnb);
    if (dry) ws = reinterpret_cast<char*>((uintptr_t)1 << 40);      // a base that is never dereferenced (offsets from a null pointer are undefined behaviour)
    u->arena.reset(ws + kvb + gnb, dry ? 0 : ws_bytes - kvb - gnb, dry);
    u->dry_flops = 0;
    Run R{u, k, s, dry, B};
    R.split = u->residual == CS_RESIDUAL_F16X2; R.count_executed = count_executed; R.calib = dry ? nullptr : calib;
    R.ctx = ctx; R.kv = (f16*)ws; R.gn_ws = (float*)(ws + kvb);
    R.sk_ws = (float*)(ws + kvb + gn_ws_bytes(u, B)); R.sk_bytes = sk_ws_bytes(u, B);
    const int c0 = c.block_out_channels[0], td = 4 * c0, L = c.ctx_len;
    int H = c.sample_size, W = c.sample_size;

    // ---- time embedding + all time_emb_proj at once ----------------------------------------------
    f16* tscratch = R.alloc((size_t)nt * (c0 + td));
    f16* temb = R.alloc((size_t)nt * td);
    f16* tproj = R.alloc((size_t)nt * u->tp_total);
    // (algorithmic count: the reference graph broadcasts the timestep to the batch and runs the time MLP and every time_emb_proj per SAMPLE; executed: per distinct timestep)
    const double nt_fl = count_executed ? (double)nt : (double)B;
    R.launch(P_MISC, 2.0 * nt_fl * ((double)c0 * td + (double)td * td), 0, [&] { return launch_time_embedding(t, nt, c0, td, u->t_w1, u->t_b1, u->t_w2, u->t_b2, tscratch, temb, s); });
    R.launch(P_MISC, 2.0 * nt_fl * (double)td * u->tp_total, 2.0 * td * u->tp_total, [&] { return launch_rowvec_linear(temb, nt, td, u->tp_w, u->tp_b, u->tp_total, tproj, 0, s); });
    R.tproj = tproj; R.tstride = (nt == 1) ? 0 : u->tp_total;

    // ---- cross-attention K/V of the context (cached across solver steps) --------------------------
    if (!kv_valid) {
        auto kvproj = [&](const Xformer& X) {
            f16* dst = R.kv + X.kv_off * (size_t)B * L;
            R.linear(ctx, B * L, c.cross_attention_dim, X.wkv2, nullptr, 2 * X.c, St(), St(dst), 0);
        };
        for (int i = 0; i < 4; ++i) { for (auto& X : u->down_att[i]) kvproj(X); for (auto& X : u->up_att[i]) kvproj(X); }
        kvproj(u->mid_att);
    }

    // ---- down path -----------------------------------------------------------------------------------
    std::vector<std::pair<St, int>> skips;
    St h = R.salloc((size_t)B * H * W * c0);
    // CFG dual batch with one timestep: the first resnet and the first transformer block up to its cross attention are shared
    const bool share = (dup == 2 && nt == 1 && c.down_has_attn[0] && k.cfg_share != 0 && !u->down_res[0].empty());
    if (k.conv_in_mfma && c.in_channels <= 64 && (H * W) % 64 == 0) {
        // latents -> NHWC-64 (n_lat samples), then the MFMA conv over them; the dual batch's second half is a copy (sample b reads latent b % n_lat)
        f16* z = R.alloc((size_t)n_lat * H * W * 64);
        R.launch(P_MISC, 0, 2.0 * n_lat * H * W * 64, [&] { return launch_latent_to_nhwc64(latents, nullptr, nullptr, z, n_lat, c.in_channels, H * W, 1.0f, 0.0f, s); });
        // GroupNorm statistics of the output from the conv epilogue, in a buffer for the FULL batch: the tensor is also a skip connection that the last up block
        // normalises at batch B, so the second half's statistics are copied along with the tensor
        float* st = R.stats_fusable(H * W, c0) ? R.alloc_stats(B, H * W, c0) : nullptr;
        const int Bkeep = R.B;
        R.B = n_lat;
        R.conv(u->conv_in64, z, 64, nullptr, 0, H, W, H, W, 1, 0, nullptr, St(), h, false, st, nullptr, nullptr, nullptr, nullptr,
               2.0 * Bkeep * H * W * 9.0 * c.in_channels * c0);      // (the graph's conv_in: 4 input channels, full batch -- as the conv_in_kernel branch counts it)
        R.B = Bkeep;
        R.release(z);
        if (dup == 2) {
            const size_t half = (size_t)n_lat * H * W * c0;
            // (round 6 tried these three copies on a side stream -- forked here, joined in front of the last up resnet, their only full-batch reader: the forward got
            //  0.15 ms SLOWER, 29.35 -> 29.50 ms alternating on one box (profiles/r06_ab_copy_async.txt): a second queue's blit kernels take CU slots and bandwidth
            //  from the conv they run beside, and the fork / join events are not free.  In line they cost 30 us.)
            R.copy(h.hi + half, h.hi, half * sizeof(f16));
            if (h.lo) R.copy(h.lo + half, h.lo, half * sizeof(f16));
            if (st) { const size_t sh = (size_t)n_lat * (H * W / 64) * c0; R.copy(st + sh, st, sh * sizeof(float)); }
        }
        if (st) R.stat_of[h.hi] = {st, H * W / 64};
    } else {
        R.launch(P_MISC, 2.0 * B * H * W * 9.0 * c.in_channels * c0, 2.0 * B * H * W * c0 * (h.lo ? 2 : 1), [&] { return launch_conv_in(latents, n_lat, B, c.in_channels, H, W, u->conv_in.w, u->conv_in.b, c0, h.hi, s, h.lo); });
    }
    int ch = c0;
    skips.push_back({h, ch});
    for (int i = 0; i < 4; ++i) {
        for (size_t j = 0; j < u->down_res[i].size(); ++j) {
            St r;
            if (share && i == 0 && j == 0) {
                R.B = n_lat;                                          // h holds [uncond | text] copies of the same tensor: use the first
                St r1 = R.resnet(u->down_res[0][0], h, ch, St(), 0, H, W);
                R.B = B;
                ch = u->down_res[0][0].cout;
                r = R.xformer(u->down_att[0][0], r1, H, W, n_lat);
                R.srelease(r1);
            } else {
                r = R.resnet(u->down_res[i][j], h, ch, St(), 0, H, W);
                ch = u->down_res[i][j].cout;
                if (c.down_has_attn[i]) { St a = R.xformer(u->down_att[i][j], r, H, W); R.srelease(r); r = a; }
            }
            h = r; skips.push_back({h, ch});
        }
        if (u->has_down[i]) {
            St d = R.salloc((size_t)B * (H / 2) * (W / 2) * ch);
            R.conv(u->down_samp[i], h.hi, ch, nullptr, 0, H, W, H / 2, W / 2, 2, 0, nullptr, St(), d, true);
            H /= 2; W /= 2; h = d; skips.push_back({h, ch});
        }
    }
    // ---- mid ---------------------------------------------------------------------------------------
    {
        St r = R.resnet(u->mid_res[0], h, ch, St(), 0, H, W);   // h stays alive: it is on the skip stack
        St a = R.xformer(u->mid_att, r, H, W); R.srelease(r);
        St r2 = R.resnet(u->mid_res[1], a, ch, St(), 0, H, W); R.srelease(a);
        h = r2;
    }
    // ---- up path -----------------------------------------------------------------------------------
    for (int i = 0; i < 4; ++i) {
        for (size_t j = 0; j < u->up_res[i].size(); ++j) {
            auto sk = skips.back(); skips.pop_back();
            St r = R.resnet(u->up_res[i][j], h, ch, sk.first, sk.second, H, W);
            R.srelease(h); R.srelease(sk.first);
            ch = u->up_res[i][j].cout;
            if (c.up_has_attn[i]) { St a = R.xformer(u->up_att[i][j], r, H, W); R.srelease(r); r = a; }
            h = r;
        }
        if (u->has_up[i]) {
            St d = R.salloc((size_t)B * (2 * H) * (2 * W) * ch);
            R.conv(u->up_samp[i], h.hi, ch, nullptr, 0, H, W, 2 * H, 2 * W, 1, 1, nullptr, St(), d, true);
            R.srelease(h); H *= 2; W *= 2; h = d;
        }
    }
    // ---- out ---------------------------------------------------------------------------------------
    f16* n = R.alloc((size_t)B * H * W * ch);
    // split stream (knob head_x2): the head's GroupNorm + SiLU output is conv_out's operand -- one fp16 plane of it was the last one-plane station of the stream's value
    // in front of eps (3.5 % of the per-forward error, tools/sim_precision_head.py).  Two planes, conv_out multiplies both: a second 25 us pass over the lo plane on top of
    // the first pass's fp32 result; the output (fp32 for the native engine, the model dtype for the plain protocol) is rounded from that once.
    const bool head2_shape = R.split && H % 16 == 0 && W % 16 == 0 && ch % 64 == 0;
    const bool head2 = head2_shape && k.head_x2 != 0 && k.conv_out_mfma != 0;
    // (the workspace query -- dry -- reserves the head's lo plane and the 16-bit output's fp32 scratch whatever the knobs and the output dtype are at that moment)
    f16* n_lo = (head2 || (dry && head2_shape)) ? R.alloc((size_t)B * H * W * ch) : nullptr;
    float* head32 = ((head2 && u->out_dtype != CS_F32) || (dry && head2_shape)) ? (float*)R.alloc((size_t)B * H * W * c.out_channels * 2) : nullptr;
    R.group_norm(u->norm_out, h, ch, St(), 0, H * W, true, n, head2 ? n_lo : nullptr);
    R.srelease(h);
    R.launch(P_MISC, 2.0 * B * H * W * 9.0 * ch * c.out_channels * ((head2 && R.count_executed) ? 2.0 : 1.0), 2.0 * B * H * W * ch * (head2 ? 2.0 : 1.0),
             [&] { return launch_conv_out(n, B, ch, H, W, u->conv_out.w, u->conv_out.b, c.out_channels, out, s, u->out_dtype == CS_F32, head2 ? n_lo : nullptr, head32); });
    if (head32) R.release(head32);
    if (n_lo) R.release(n_lo);
    R.release(n); R.release(tscratch); R.release(temb); R.release(tproj);
    return R.rc;
}

}  // namespace

extern "C" {

int cs_unet_create(const CsUNetConfig* cfg, CsUNet** out) {
    if (!cfg || !out) CS_FAIL(CS_E_ARG, "cfg/out is NULL");
    if (cfg->in_channels != 4 || cfg->out_channels != 4) CS_FAIL(CS_E_UNSUPPORTED, "only 4 latent channels are built");
    for (int i = 0; i < 4; ++i)
        if (cfg->block_out_channels[i] % 64 || (cfg->block_out_channels[i] % 160 && cfg->block_out_channels[i] % 128))
            CS_FAIL(CS_E_SHAPE, "block_out_channels[%d]=%d must be a multiple of 64 and of 128 or 160", i, cfg->block_out_channels[i]);
    if (cfg->cross_attention_dim % 64) CS_FAIL(CS_E_SHAPE, "cross_attention_dim must be a multiple of 64");
    for (int i = 0; i < 4; ++i) {
        const int dh = cfg->block_out_channels[i] / cfg->num_heads;
        if (dh != 40 && dh != 80 && dh != 160) CS_FAIL(CS_E_UNSUPPORTED, "head dim %d not built", dh);
    }
    if (cfg->sample_size % 8) CS_FAIL(CS_E_SHAPE, "sample_size must be a multiple of 8");
    CsUNet* u = new CsUNet();
    u->cfg = *cfg;
    build_manifest(u);
    *out = u;
    return CS_OK;
}

void cs_unet_destroy(CsUNet* u) {
    if (!u) return;
    u->weights.free_device();
    for (auto& e : u->evs) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    delete u;
}

int cs_unet_num_weights(const CsUNet* u) { return u ? u->weights.count() : 0; }

const char* cs_unet_weight_name(const CsUNet* u, int i, int64_t* shape4, int* ndim) { return u ? u->weights.name_at(i, shape4, 4, ndim) : nullptr; }

int cs_unet_set_weight(CsUNet* u, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!u) CS_FAIL(CS_E_ARG, "null argument");
    return u->weights.set(name, data, shape, ndim);
}

int cs_unet_finalize(CsUNet* u) {
    if (!u) CS_FAIL(CS_E_ARG, "null");
    F16Store& W = u->weights;
    if (W.finalized) return CS_OK;
    if (const std::string* n = W.first_missing()) CS_FAIL(CS_E_STATE, "missing weight '%s'", n->c_str());
    const CsUNetConfig& c = u->cfg;
    bool ok = true;
    std::vector<f16> tpw, tpb;
    ok = ok && make_conv(W, "conv_in", u->conv_in) && make_conv(W, "conv_out", u->conv_out) && make_norm(W, "conv_norm_out", u->norm_out, 1e-5f);
    ok = ok && make_conv_padded64(W, "conv_in", u->conv_in64);
    u->t_w1 = W.upload(W.at("time_embedding.linear_1.weight").data); u->t_b1 = W.upload(W.at("time_embedding.linear_1.bias").data);
    u->t_w2 = W.upload(W.at("time_embedding.linear_2.weight").data); u->t_b2 = W.upload(W.at("time_embedding.linear_2.bias").data);
    Topology t = topology(c);
    for (int i = 0; i < 4 && ok; ++i) {
        const std::string b = "down_blocks." + std::to_string(i);
        u->down_res[i].resize(t.down[i].size());
        if (c.down_has_attn[i]) u->down_att[i].resize(t.down[i].size());
        for (size_t j = 0; j < t.down[i].size() && ok; ++j) {
            ok = ok && make_resnet(u, b + ".resnets." + std::to_string(j), u->down_res[i][j], tpw, tpb);
            if (c.down_has_attn[i]) ok = ok && make_xformer(u, b + ".attentions." + std::to_string(j), u->down_att[i][j]);
        }
        u->has_down[i] = i < 3;
        if (i < 3) ok = ok && make_conv(W, b + ".downsamplers.0.conv", u->down_samp[i]);
    }
    ok = ok && make_resnet(u, "mid_block.resnets.0", u->mid_res[0], tpw, tpb) && make_xformer(u, "mid_block.attentions.0", u->mid_att) &&
         make_resnet(u, "mid_block.resnets.1", u->mid_res[1], tpw, tpb);
    for (int i = 0; i < 4 && ok; ++i) {
        const std::string b = "up_blocks." + std::to_string(i);
        u->up_res[i].resize(t.up[i].size());
        if (c.up_has_attn[i]) u->up_att[i].resize(t.up[i].size());
        for (size_t j = 0; j < t.up[i].size() && ok; ++j) {
            ok = ok && make_resnet(u, b + ".resnets." + std::to_string(j), u->up_res[i][j], tpw, tpb);
            if (c.up_has_attn[i]) ok = ok && make_xformer(u, b + ".attentions." + std::to_string(j), u->up_att[i][j]);
        }
        u->has_up[i] = i < 3;
        if (i < 3) {
            ok = ok && make_conv(W, b + ".upsamplers.0.conv", u->up_samp[i]);
            // the same filter in its sub-pixel form (4 phases x 4 summed taps: 16 / 9 of the bytes), for the forwards that run on one fp16 plane (knob up_fold)
            Conv& uc = u->up_samp[i];
            if (ok && uc.taps == 9 && uc.cout % 160 == 0 && uc.cin % 64 == 0) {
                std::vector<f16> sub((size_t)4 * uc.cout * 4 * uc.cin);
                conv_up_fold_pack_host(pack_conv(W.at(b + ".upsamplers.0.conv.weight")).data(), uc.cout, uc.cin, sub.data());
                uc.w_sub = W.upload(sub);
                ok = ok && uc.w_sub;
            }
        }
    }
    u->tp_total = (int)tpb.size();
    u->tp_w = W.upload(tpw); u->tp_b = W.upload(tpb);
    if (!ok || !u->t_w1 || !u->t_b1 || !u->t_w2 || !u->t_b2 || !u->tp_w || !u->tp_b) CS_FAIL(CS_E_HIP, "weight upload failed (hipMalloc/hipMemcpy)");
    W.release_host();
    W.finalized = true;
    return CS_OK;
}

size_t cs_unet_workspace_bytes(const CsUNet* cu, int batch) {
    CsUNet* u = const_cast<CsUNet*>(cu);
    if (!u || !u->weights.finalized || batch <= 0) return 0;
    // the arena's peak depends on the execution variant (CFG shared prefix on / off, fused cross-attention block on / off): the workspace
    // covers all of them, whatever the knobs say now, so that toggling a knob later never outgrows a workspace sized earlier
    // (the knobs it does not enumerate come from the process-wide set)
    const TuneSet base = tune_snapshot();
    size_t peak = 0;
    for (int variant = 0; variant < 32; ++variant) {         // (every knob that changes the allocation sequence: the first-fit arena's peak depends on the holes it leaves)
        TuneSet v = base;
        v.xattn_fused = variant & 1; v.gn_fuse = (variant >> 1) & 1; v.ln_fold = (variant >> 2) & 1; v.conv_in_mfma = (variant >> 3) & 1; v.lo8 = variant >> 4;
        v.cfg_share = 1;
        run_forward(u, v, true, nullptr, batch, 1, nullptr, batch /* worst case: per-sample timesteps */, nullptr, nullptr, nullptr, 0, 0, nullptr);
        peak = std::max(peak, u->arena.peak);
        if (batch % 2 == 0) {
            for (int share = 0; share < 2; ++share) {          // (first-fit: the CFG dual batch with and without the shared prefix leaves different holes)
                v.cfg_share = share;
                run_forward(u, v, true, nullptr, batch / 2, 2, nullptr, 1, nullptr, nullptr, nullptr, 0, 0, nullptr);
                peak = std::max(peak, u->arena.peak);
            }
        }
    }
    return kv_cache_bytes(u, batch) + gn_ws_bytes(u, batch) + sk_ws_bytes(u, batch) + peak + 4096;
}

double cs_unet_flops_executed(const CsUNet* cu, int n_lat, int dup) {
    CsUNet* u = const_cast<CsUNet*>(cu);
    if (!u || !u->weights.finalized || n_lat <= 0 || (dup != 1 && dup != 2)) return 0;
    run_forward(u, handle_tune(u), true, nullptr, n_lat, dup, nullptr, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, true);     // (what THIS handle's forwards execute)
    return u->dry_flops;
}

double cs_unet_flops(const CsUNet* cu, int batch) {
    CsUNet* u = const_cast<CsUNet*>(cu);
    if (!u || !u->weights.finalized || batch <= 0) return 0;
    run_forward(u, handle_tune(u), true, nullptr, batch, 1, nullptr, 1, nullptr, nullptr, nullptr, 0, 0, nullptr);
    return u->dry_flops;
}

int cs_unet_forward(CsUNet* u, const void* latents, int n_lat, int dup, const float* timesteps, int n_timesteps, const void* ctx,
                    void* out, void* workspace, size_t workspace_bytes, int kv_cache_valid, void* stream) {
    if (!u) CS_FAIL(CS_E_ARG, "unet is NULL");
    if (!u->weights.finalized) CS_FAIL(CS_E_STATE, "cs_unet_finalize has not been called");
    if (n_lat < 0 || (dup != 1 && dup != 2)) CS_FAIL(CS_E_ARG, "bad n_lat/dup");
    if (n_lat == 0) return CS_OK;
    if (!latents || !timesteps || !ctx || !out || !workspace) CS_FAIL(CS_E_ARG, "null pointer");
    if (n_timesteps != 1 && n_timesteps != n_lat * dup) CS_FAIL(CS_E_SHAPE, "n_timesteps must be 1 or the batch size");
    u->ev_used = 0;
    const int rc = run_forward(u, handle_tune(u), false, (const f16*)latents, n_lat, dup, timesteps, n_timesteps, (const f16*)ctx, (f16*)out, (char*)workspace,
                               workspace_bytes, kv_cache_valid, (hipStream_t)stream);
    if (rc == CS_OK && u->profiling) {
        CS_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
        for (int k = 0; k < P_COUNT; ++k) { u->prof_ms[k] = u->prof_flops[k] = u->prof_bytes[k] = 0; u->prof_launches[k] = 0; }
        for (size_t i = 0; i < u->ev_used; ++i) {
            float ms = 0; hipEventElapsedTime(&ms, u->evs[i].a, u->evs[i].b);
            const int k = u->evs[i].cls;
            u->prof_ms[k] += ms; u->prof_flops[k] += u->evs[i].flops; u->prof_bytes[k] += u->evs[i].bytes; u->prof_launches[k]++;
        }
    }
    return rc;
}

int cs_unet_calibrate_ln_fold(CsUNet* u, const void* latents, int n_lat, int dup, const float* timesteps, int n_timesteps, const void* ctx, void* out,
                              void* workspace, size_t workspace_bytes, float bound, void* stream, unsigned* mask_out, float* worst_ratio_out) {
    if (!u) CS_FAIL(CS_E_ARG, "unet is NULL");
    if (!u->weights.finalized) CS_FAIL(CS_E_STATE, "cs_unet_finalize has not been called");
    if (n_lat <= 0 || (dup != 1 && dup != 2) || !latents || !timesteps || !ctx || !out || !workspace) CS_FAIL(CS_E_ARG, "calibrate_ln_fold: bad arguments");
    if (n_timesteps != 1 && n_timesteps != n_lat * dup) CS_FAIL(CS_E_SHAPE, "n_timesteps must be 1 or the batch size");
    if (!(bound > 0.f)) CS_FAIL(CS_E_ARG, "calibrate_ln_fold: bound must be positive");
    const int nslots = 3 * u->n_xformers;
    if (u->n_xformers > 32) CS_FAIL(CS_E_UNSUPPORTED, "calibrate_ln_fold: more than 32 transformer blocks");
    if (nslots == 0) { if (mask_out) *mask_out = 0; if (worst_ratio_out) *worst_ratio_out = 0.f; return CS_OK; }
    if (!u->calib) {
        void* d = nullptr;
        CS_CHECK_HIP(hipMalloc(&d, nslots * sizeof(float)));
        u->weights.dev_allocs.push_back(d); u->calib = (float*)d;
    }
    hipStream_t s = (hipStream_t)stream;
    // measured on the FOLDED graph (every producer of the hidden state leaves its row statistics): the mask is cleared for the calibration forward
    const unsigned keep = u->ln_unfold_mask;
    u->ln_unfold_mask = 0;
    CS_CHECK_HIP(hipMemsetAsync(u->calib, 0, nslots * sizeof(float), s));
    u->ev_used = 0;
    TuneSet k = handle_tune(u);
    k.ln_fold = 1; k.cfg_share = 0;              // (every row of the batch through every statistics point)
    const int rc = run_forward(u, k, false, (const f16*)latents, n_lat, dup, timesteps, n_timesteps, (const f16*)ctx, (f16*)out, (char*)workspace, workspace_bytes, 0, s,
                               false, u->calib);
    if (rc != CS_OK) { u->ln_unfold_mask = keep; return rc; }
    std::vector<float> host(nslots);
    CS_CHECK_HIP(hipStreamSynchronize(s));
    CS_CHECK_HIP(hipMemcpy(host.data(), u->calib, nslots * sizeof(float), hipMemcpyDeviceToHost));
    // slot = sum over the hidden state's rows of mean^2 / var; the rows of a level: B * HW -- recovered per block from its level below
    unsigned mask = 0; float worst = 0.f;
    auto visit = [&](const Xformer& X, int HW) {
        const double rows = (double)n_lat * dup * HW;
        for (int k = 0; k < 3; ++k) {
            const float ratio = (float)std::sqrt((double)host[3 * X.index + k] / rows);      // RMS over rows of |mean| / sigma
            worst = std::max(worst, ratio);
            if (ratio > bound) mask |= 1u << X.index;
        }
    };
    {
        int H = u->cfg.sample_size;
        for (int i = 0; i < 4; ++i) { for (auto& X : u->down_att[i]) visit(X, H * H); if (u->has_down[i]) H /= 2; }
        visit(u->mid_att, H * H);
        for (int i = 0; i < 4; ++i) { for (auto& X : u->up_att[i]) visit(X, H * H); if (u->has_up[i]) H *= 2; }
    }
    u->ln_unfold_mask = mask;
    if (mask_out) *mask_out = mask;
    if (worst_ratio_out) *worst_ratio_out = worst;
    return CS_OK;
}
int cs_unet_set_ln_unfold_mask(CsUNet* u, unsigned mask) { if (!u) CS_FAIL(CS_E_ARG, "unet is NULL"); u->ln_unfold_mask = mask; return CS_OK; }
unsigned cs_unet_get_ln_unfold_mask(const CsUNet* u) { return u ? u->ln_unfold_mask : 0u; }

int cs_unet_set_tuning(CsUNet* u, const char* key, int value) {
    if (!u || !key) CS_FAIL(CS_E_ARG, "unet / key is NULL");
    TuneSet scratch;                                     // known knob, value in range?  (validated on a scratch set: the process-wide one is not touched)
    const int rc = tune_apply(scratch, key, value);
    if (rc != CS_OK) return rc;
    u->tune[key] = value;
    return CS_OK;
}
int cs_unet_clear_tuning(CsUNet* u) { if (!u) CS_FAIL(CS_E_ARG, "unet is NULL"); u->tune.clear(); return CS_OK; }

int cs_unet_set_residual_precision(CsUNet* u, int mode) {
    if (!u) CS_FAIL(CS_E_ARG, "unet is NULL");
    if (mode != CS_RESIDUAL_F16 && mode != CS_RESIDUAL_F16X2) CS_FAIL(CS_E_ARG, "residual precision %d: CS_RESIDUAL_F16 (0) or CS_RESIDUAL_F16X2 (1)", mode);
    u->residual = mode;
    return CS_OK;
}
int cs_unet_get_residual_precision(const CsUNet* u) { return u ? u->residual : -1; }

int cs_unet_set_output_dtype(CsUNet* u, int dtype) {
    if (!u) CS_FAIL(CS_E_ARG, "unet is NULL");
    if (dtype != CS_F16 && dtype != CS_F32) CS_FAIL(CS_E_DTYPE, "unet output dtype %d: CS_F16 or CS_F32", dtype);
    u->out_dtype = dtype;
    return CS_OK;
}
int cs_unet_get_output_dtype(const CsUNet* u) { return u ? u->out_dtype : -1; }

int cs_unet_set_profiling(CsUNet* u, int on) { if (!u) return CS_E_ARG; u->profiling = on != 0; return CS_OK; }
int cs_unet_profile_entries(const CsUNet* u) { return u ? P_COUNT : 0; }
const char* cs_unet_profile_entry(const CsUNet* u, int i, double* ms, double* flops, double* bytes, int* launches) {
    if (!u || i < 0 || i >= P_COUNT) return nullptr;
    if (ms) *ms = u->prof_ms[i];
    if (flops) *flops = u->prof_flops[i];
    if (bytes) *bytes = u->prof_bytes[i];
    if (launches) *launches = u->prof_launches[i];
    return kProfNames[i];
}

}  // extern "C"
