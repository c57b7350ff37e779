/*
 * consolver_hip.h -- C ABI of libconsolver_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the ConsistencySolver sampling hot path of
 * G-U-N/consolver.  The reference is pure Python on top of torch/diffusers and
 * has no FFI of its own; the entry points below are what a Python (ctypes),
 * C++ or cgo/JNI host would bind to replace, one for one, the arithmetic inside
 *
 *   scheduler_ppo.py:178-299      PPOScheduler.step            -> cs_lms_ddim_step
 *   scheduler_ppo.py:306-332      PPOScheduler._get_prev_sample   (fused into the above)
 *   scheduler_ppo.py:165-175      set_default_coefficients        (fused into the above)
 *   denoise_ppo.py:96-100         CFG combine u + g (c - u)       (fused into the above)
 *   edit_ppo/scheduler_fmppo.py:306-455  FMPPOScheduler.step   -> cs_lms_euler_step
 *   factor_net_ppo.py:137-157     FactorNetPPO.forward_        -> cs_factor_probs
 *   factor_net_ppo.py:108-130     compute_cosine_similarity    -> cs_cosine_features
 *   factor_net_ppo.py:159-168     sample_action (gather part)  -> cs_sample_actions / cs_gather_actions
 *   factor_net_ppo.py:170-184     get_action_probs             -> cs_action_probs
 *   scheduler_ppo.py:222-232      zero-padded history stack    -> cs_stack_history
 *   denoise_ppo.py:89-94          unet(latents, t, ctx)[0]     -> cs_unet_forward
 *                                 (third-party diffusers UNet2DConditionModel, SD1.5 config)
 *
 * Conventions
 *   - every pointer is a BORROWED DEVICE pointer unless its name ends in _host;
 *   - every call is asynchronous on the hipStream_t passed as `stream`
 *     (void* so that the header needs no HIP include);
 *   - no allocation, no host synchronisation, no global state in the compute
 *     entry points (they are graph-capturable); cs_unet_create/destroy own
 *     device memory for packed weights;
 *   - return value: 0 = CS_OK, negative = error (see below);
 *     cs_last_error() returns a thread-local human readable message.
 */
#ifndef CONSOLVER_HIP_H
#define CONSOLVER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_ABI_VERSION 2
#define CS_MAX_ORDER 8        /* order_dim <= 8 */
#define CS_MAX_ACTION_DIMS 16 /* order + scaler + mu - 1 */

enum { CS_OK = 0, CS_E_ARG = -1, CS_E_SHAPE = -2, CS_E_DTYPE = -3, CS_E_HIP = -4, CS_E_STATE = -5, CS_E_UNSUPPORTED = -6 };
enum { CS_F32 = 0, CS_F16 = 1, CS_BF16 = 2, CS_U8 = 3 };   /* CS_U8: image input of cs_fid_preprocess only */

int cs_abi_version(void);
const char* cs_error_string(int code);
const char* cs_last_error(void);
/* name of the device the library was built for ("gfx950") */
const char* cs_target_arch(void);

/* ------------------------------------------------------------------------
 * Policy network (FactorNetPPO) : Linear-ReLU-Linear-ReLU-Linear + softmax
 * ---------------------------------------------------------------------- */
typedef struct CsFactorNet {
    const float* w0; const float* b0; /* [hidden, in_dim], [hidden]             */
    const float* w1; const float* b1; /* [hidden, hidden], [hidden]             */
    const float* w2; const float* b2; /* [action_dims*num_actions, hidden], [.] */
    int in_dim;        /* 2 (+ order_dim-1 when use_conv)                        */
    int hidden;        /* <= 1024                                                */
    int action_dims;   /* A <= CS_MAX_ACTION_DIMS                                */
    int num_actions;   /* K <= 1024                                              */
    float input_scale;     /* 1/999 for SD (factor_net_ppo.py:106), 1 for FLUX  */
    float inv_temperature; /* 1 for SD, 100 for FLUX (softmax(logits/0.01))     */
} CsFactorNet;

/* probs[B, A, K] = softmax(MLP(cat(x * input_scale, cos_feat)) * inv_temperature).
 * x: [B, 2] fp32.  cos_feat: [B, in_dim-2] fp32 or NULL when in_dim == 2.
 * x_row_stride = 0 broadcasts one conditioning row to all B samples. */
int cs_factor_probs(const CsFactorNet* net, const float* x, int x_row_stride, const float* cos_feat,
                    int B, float* probs, void* stream);

/* cos(eps[k], eps[0]) for k = 1..order-1 over the flattened sample; slots k >= m
 * (zero padded in the reference) give 0.  hist[k]: [B, elems] newest first.
 * out: [B, order-1] fp32. */
int cs_cosine_features(const void* const* hist_host, int m, int order, int B, int64_t elems,
                       int dtype, float* out, void* stream);

/* The same under classifier-free guidance with the combine fused (denoise_ppo.py:96-100 in
 * front of scheduler_ppo.py:207-240): hist[0] is the TEXT branch, eps_uncond the other one,
 * and the newest history entry is e = eps_uncond + guidance * (hist[0] - eps_uncond) rounded
 * to `dtype` exactly as cs_lms_ddim_step rounds it.  e is formed on the fly for the features
 * and written to eps_out [B, elems] (required), which the caller then passes to the update
 * kernel as an already combined eps.  eps_uncond == NULL: identical to cs_cosine_features. */
int cs_cosine_features_cfg(const void* const* hist_host, int m, int order, int B, int64_t elems,
                           int dtype, const void* eps_uncond, float guidance, void* eps_out,
                           float* out, void* stream);

/* inverse-CDF categorical sampling from probs[B,A,K] with caller supplied
 * uniforms[B,A] in [0,1).  Writes idx[B,A] (int64), actions[B,A] = action_values[a, idx],
 * action_probs[B,A] = probs[b,a,idx].  Any output pointer may be NULL. */
int cs_sample_actions(const float* probs, const float* uniforms, const float* action_values,
                      int B, int A, int K, int64_t* idx, float* actions, float* action_probs, void* stream);

/* same gather with caller supplied indices (replay / torch.multinomial output). */
int cs_gather_actions(const float* probs, const int64_t* idx, const float* action_values,
                      int B, int A, int K, float* actions, float* action_probs, void* stream);

/* PPO re-evaluation (factor_net_ppo.py:170-184): nearest-bin index of each action,
 * selected probability and normalised entropy H/ln K.  All [B, A] fp32. */
int cs_action_probs(const float* probs, const float* actions, const float* action_values,
                    int B, int A, int K, float* selected, float* entropy, void* stream);

/* masks[B, A] = 1 except columns [m-1, order-1) = 0 (scheduler_ppo.py:248-249). */
int cs_step_masks(int B, int A, int m, int order, float* masks, void* stream);

/* out[B, order, elems] = stack(hist newest first) zero padded (scheduler_ppo.py:222-232). */
int cs_stack_history(const void* const* hist_host, int m, int order, int B, int64_t elems,
                     int dtype, void* out, void* stream);

/* ------------------------------------------------------------------------
 * Fused solver update
 * ---------------------------------------------------------------------- */
typedef struct CsStepArgs {
    const void* x;            /* [B, elems] current sample                          */
    const void* eps_text;     /* [B, elems] model output (conditional branch)       */
    const void* eps_uncond;   /* [B, elems] unconditional branch, or NULL (no CFG)  */
    float guidance;           /* eps = u + guidance * (c - u)                       */
    const void* hist[CS_MAX_ORDER]; /* hist[k] = eps_{t-1-k}, k < m-1 (newest first) */
    int m;                    /* history length AFTER pushing the new eps, 1..order */
    int order_dim, scaler_dim;
    const float* actions;     /* [B, actions_stride] sampled grid values, device    */
    int actions_stride;
    int B;
    int64_t elems;            /* elements per sample                                */
    int io_dtype;             /* dtype of x, eps_*, hist, eps_out                   */
    int out_dtype;            /* dtype of x_out                                     */
    void* x_out;              /* [B, elems]                                         */
    void* eps_out;            /* [B, elems] CFG-combined eps (next steps' history)
                                 required when eps_uncond != NULL, else optional     */
    /* DDIM scalars (host fp32, scheduler_ppo.py:309-312): sqrt(a_t), sqrt(1-a_t),
       sqrt(a_prev), sqrt(1-a_prev) */
    float sqrt_at, sqrt_1mat, sqrt_ap, sqrt_1map;
    int v_prediction;
    /* Euler (flow matching): dt = sigma_next - sigma (scheduler_fmppo.py:376) */
    float dt;
    /* nonzero: x is fp32 while eps_* / hist stay io_dtype (scheduler_fmppo.py:354 upcasts the sample
       before the update and rounds only the result); ABI version 2 */
    int x_is_f32;
    /* optional (may be NULL): a second, 16-bit copy of an fp32 result (out_dtype = CS_F32), [B, elems] in lp_dtype (CS_F16 | CS_BF16) -- the view of an fp32 solver
       state that the denoiser reads at the next step, written in the same pass instead of by a cast kernel per step; ABI version 3 */
    void* x_out_lp;
    int lp_dtype;
} CsStepArgs;

int cs_lms_ddim_step(const CsStepArgs* args, void* stream);
int cs_lms_euler_step(const CsStepArgs* args, void* stream);

/* ------------------------------------------------------------------------
 * Multistep DPM-Solver update (orders 1 and 2; consolver_amd/scheduling_dpm.py).
 * Every variant is one linear update per element; the variant is in five host scalars:
 *     eps = eps_uncond ? round_io(u + guidance * (c - u)) : c
 *     m0  = round_io(conv_x * x + conv_e * eps)        the converted model output, written to m_out
 *     x'  = cx * x + c0 * m0 + c1 * m_prev             (c1 * m_prev only when m_prev != NULL)
 * Pointer and dtype fields mean what they mean in CsStepArgs.
 * ---------------------------------------------------------------------- */
typedef struct CsDpmStepArgs {
    const void* x;            /* [B, elems] current sample (io_dtype, or fp32 when x_is_f32) */
    const void* eps_text;     /* [B, elems] model output (conditional branch)       */
    const void* eps_uncond;   /* [B, elems] unconditional branch, or NULL (no CFG)  */
    float guidance;
    const void* m_prev;       /* [B, elems] the previous step's m0, or NULL (first order) */
    int B;
    int64_t elems;            /* elements per sample                                */
    int io_dtype;             /* dtype of eps_*, m_prev, m_out (and of x unless x_is_f32) */
    int out_dtype;            /* dtype of x_out                                     */
    int x_is_f32;
    void* x_out;              /* [B, elems]                                         */
    void* m_out;              /* [B, elems] m0; required when eps_uncond != NULL or
                                 (conv_x, conv_e) != (0, 1), else optional           */
    void* x_out_lp;           /* optional 16-bit copy of an fp32 result, as CsStepArgs::x_out_lp */
    int lp_dtype;
    float conv_x, conv_e, cx, c0, c1;
} CsDpmStepArgs;

int cs_dpm_multistep_step(const CsDpmStepArgs* args, void* stream);

/* ------------------------------------------------------------------------
 * n-term linear update (DEIS, iPNDM; consolver_amd/scheduling_deis.py, scheduling_pndm.py).
 * A multistep update with up to four model outputs and host coefficients:
 *     eps = eps_uncond ? round_io(u + guidance * (c - u)) : c
 *     m0  = round_io(conv_x * x + conv_e * eps)        skipped when (conv_x, conv_e) == (0, 1); written to m_out
 *     xb  = x_base ? x_base : x
 *     x'  = cx * xb + c[0] * m0 + c[1] * hist[0] + ... + c[terms - 1] * hist[terms - 2]
 * in fp32, left to right, rounded once to out_dtype.  Pointer, dtype and x_out_lp fields mean what they
 * mean in CsDpmStepArgs.  A tensor whose pointer is NULL is not read; hist[k] with k >= terms - 1 is not read.
 * All [B, elems] tensors are contiguous and 16-byte aligned (one flat range of B * elems elements).
 * Aliasing: x_out aliases no input; m_out aliases no history entry that is read.
 * Refused before any launch: terms outside 1..CS_LIN_MAX_TERMS, a NULL among the first terms - 1 history
 * pointers, x_is_f32 with fp32 io, an fp32 sample with a 16-bit result, and what cs_dpm_multistep_step refuses.
 * ---------------------------------------------------------------------- */
#define CS_LIN_MAX_TERMS 4
typedef struct CsLinStepArgs {
    const void* x;            /* [B, elems] current sample (io_dtype, or fp32 when x_is_f32) */
    const void* eps_text;     /* [B, elems] model output (conditional branch)       */
    const void* eps_uncond;   /* [B, elems] unconditional branch, or NULL (no CFG)  */
    float guidance;
    const void* x_base;       /* [B, elems] the sample the update starts from (dtype of x), or NULL: x */
    const void* hist[CS_LIN_MAX_TERMS - 1]; /* earlier converted outputs, newest first; the first terms - 1 are read */
    int terms;                /* model outputs in the update, 1..CS_LIN_MAX_TERMS   */
    int B;
    int64_t elems;            /* elements per sample                                */
    int io_dtype;             /* dtype of eps_*, hist, m_out (and of x, x_base unless x_is_f32) */
    int out_dtype;            /* dtype of x_out                                     */
    int x_is_f32;             /* the sample is fp32 beside 16-bit model outputs (an error with fp32 io) */
    void* x_out;              /* [B, elems]                                         */
    void* m_out;              /* [B, elems] m0; required when eps_uncond != NULL or
                                 (conv_x, conv_e) != (0, 1), else optional           */
    void* x_out_lp;           /* optional 16-bit copy of an fp32 result, as CsStepArgs::x_out_lp */
    int lp_dtype;
    float conv_x, conv_e, cx;
    float c[CS_LIN_MAX_TERMS];
} CsLinStepArgs;

int cs_linear_step(const CsLinStepArgs* args, void* stream);

/* ------------------------------------------------------------------------
 * UniPC update (bh1 / bh2, orders 1 and 2, x0 prediction; consolver_amd/scheduling_unipc.py).
 * One step is the corrector of the PREVIOUS update, which needs this step's model output, and this
 * step's predictor from the corrected sample -- one pass, the variant in nine host scalars:
 *     eps    = eps_uncond ? round_io(u + guidance * (c - u)) : c
 *     m_new  = round_io(conv_x * x + conv_e * eps)     the converted output at the PREDICTED sample x, written to m_out
 *     x_c    = use_corr ? round_out(a_x * x_last + a_0 * m_prev0 + a_1 * m_prev1 + a_n * m_new) : x
 *     x_next = p_x * x_c + p_0 * m_new + p_1 * m_prev0
 * (a term whose coefficient is zero is not read).  Pointer and dtype fields mean what they mean in
 * CsDpmStepArgs; x_last and x_last_out have the dtype of x, which is out_dtype.  All [B, elems] tensors are
 * contiguous and 16-byte aligned.
 * Aliasing: x_last_out may be x_last (each element is read, then written, by the same thread); x_out
 * aliases none of the inputs; m_out aliases none of m_prev0, m_prev1.
 * ---------------------------------------------------------------------- */
typedef struct CsUnipcStepArgs {
    const void* x;            /* [B, elems] this step's sample: the previous predictor's output (io_dtype, or fp32 when x_is_f32) */
    const void* eps_text;     /* [B, elems] model output (conditional branch)       */
    const void* eps_uncond;   /* [B, elems] unconditional branch, or NULL (no CFG)  */
    float guidance;
    const void* x_last;       /* [B, elems] the previous step's corrected sample; may be NULL iff use_corr == 0 */
    const void* m_prev0;      /* [B, elems] m_new of step i - 1; may be NULL iff a_0 == 0 (or use_corr == 0) and p_1 == 0 */
    const void* m_prev1;      /* [B, elems] m_new of step i - 2; may be NULL iff a_1 == 0 (or use_corr == 0) */
    int B;
    int64_t elems;            /* elements per sample                                */
    int io_dtype;             /* dtype of eps_*, m_prev*, m_out (and of x, x_last unless x_is_f32) */
    int out_dtype;            /* dtype of x_out and x_last_out: the sample's        */
    int x_is_f32;             /* the sample is fp32 beside 16-bit model outputs (an error with fp32 io) */
    int use_corr;
    void* x_out;              /* [B, elems] x_next                                  */
    void* m_out;              /* [B, elems] m_new (required: the conversion is never the identity) */
    void* x_last_out;         /* [B, elems] x_c, the next step's x_last; NULL: not stored */
    void* x_out_lp;           /* optional 16-bit copy of an fp32 x_next, as CsStepArgs::x_out_lp */
    int lp_dtype;
    float conv_x, conv_e, a_x, a_0, a_1, a_n, p_x, p_0, p_1;
} CsUnipcStepArgs;

int cs_unipc_step(const CsUnipcStepArgs* args, void* stream);

/* ------------------------------------------------------------------------
 * Flow-matching baseline update (consolver_amd/scheduling_fm.py; edit_ppo/scheduler_fm.py:405-482).
 * Every branch of the Euler, Heun, dpm-solver and multistep steps is
 *     w  = v1 ? round_io(v1 + v2) : v2
 *     x' = cast_out(x_base + round_io(round_io(c) * w))
 * (round_io is the identity for fp32 io).  Which sample is the base, whether v1 is read and the
 * scalar c are the host's step plan.  [B, elems] tensors are contiguous and 16-byte aligned.
 * ---------------------------------------------------------------------- */
typedef struct CsFmStepArgs {
    const void* x_base;       /* [B, elems] this step's or the saved sample (io_dtype, or fp32 when x_is_f32) */
    const void* v2;           /* [B, elems] this step's model output                */
    const void* v1;           /* [B, elems] the saved model output, or NULL         */
    float c;                  /* dt | 0.5 dt_saved | dt_saved + (sigma_next - sigma) */
    int B;
    int64_t elems;            /* elements per sample                                */
    int io_dtype;             /* dtype of v1, v2 (and of x_base unless x_is_f32)    */
    int out_dtype;            /* dtype of x_out: io_dtype, or CS_F32                */
    int x_is_f32;             /* as CsStepArgs::x_is_f32                            */
    void* x_out;              /* [B, elems]                                         */
} CsFmStepArgs;

int cs_fm_general_step(const CsFmStepArgs* args, void* stream);

/* True classifier-free guidance of the Kontext edit (edit_ppo/pipeline.py:1100-1115), between the two DiT forwards and an unchanged scheduler step:
 *     out[i] = round_to_out_dtype(neg[i] + scale * (pos[i] - neg[i]))
 * evaluated in fp32 with the operations' rounding errors carried along and rounded ONCE (to nearest even): the exact value's rounding, not the
 * reference's three 16-bit ops.  Dtype pairs: the same 16-bit type in and out, or CS_F32 in with CS_F16 / CS_BF16 / CS_F32 out (the DiT's fp32
 * head output, cs_flux_set_output_dtype); anything else is CS_E_DTYPE.  pos and neg are typically the two halves of one [2 R, L, 64] forward output.
 * n < 0: CS_E_SHAPE.  n == 0: no-op whatever the pointers.  A NULL pointer, or one that is not 16-byte aligned (fp32 inputs beside a 16-bit
 * output: 4-byte), is CS_E_ARG.  out may be pos or neg (exactly, not a shifted overlap) ONLY when input and output elements have the same size;
 * with fp32 in and 16 bits out that is CS_E_ARG.  All codes are returned before any launch. */
int cs_true_cfg_combine(const void* pos, const void* neg, int in_dtype /* CS_F32 | CS_F16 | CS_BF16 */, float scale,
                        void* out, int out_dtype /* CS_F16 | CS_BF16 | CS_F32 */, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * SD1.5 UNet2DConditionModel forward (denoiser).  See DESIGN.md for the
 * activation layout (NHWC fp16) and the kernels behind it.
 * ---------------------------------------------------------------------- */
typedef struct CsUNetConfig {
    int in_channels, out_channels;     /* 4, 4                        */
    int block_out_channels[4];         /* 320, 640, 1280, 1280        */
    int layers_per_block;              /* 2                           */
    int num_heads;                     /* 8 (attention_head_dim)      */
    int cross_attention_dim;           /* 768                         */
    int norm_num_groups;               /* 32                          */
    int sample_size;                   /* 64 (latent H = W)           */
    int ctx_len;                       /* 77                          */
    int down_has_attn[4];              /* 1,1,1,0                     */
    int up_has_attn[4];                /* 0,1,1,1                     */
} CsUNetConfig;

typedef struct CsUNet CsUNet;

int cs_unet_create(const CsUNetConfig* cfg, CsUNet** out);
void cs_unet_destroy(CsUNet* u);
/* Upload one tensor by its diffusers state-dict name (e.g.
 * "down_blocks.0.resnets.0.conv1.weight").  data_host: fp32 host memory in the
 * PyTorch layout.  The library repacks into its own fp16 device layout. */
int cs_unet_set_weight(CsUNet* u, const char* name, const float* data_host, const int64_t* shape, int ndim);
/* number of tensors the config expects / names, for manifest checks */
int cs_unet_num_weights(const CsUNet* u);
const char* cs_unet_weight_name(const CsUNet* u, int i, int64_t* shape4, int* ndim);
/* all weights present? pack; must be called once before forward */
int cs_unet_finalize(CsUNet* u);
size_t cs_unet_workspace_bytes(const CsUNet* u, int batch);
/* FLOPs of one forward at `batch` samples: the REFERENCE GRAPH's algorithmic count (2*MAC; SURVEY 8(d): batch x 803.27 GFLOP for SD1.5), independent of
 * every execution knob (conv_in is counted at its 4 input channels even when it runs zero-padded on the MFMA conv; the time MLP per sample) */
double cs_unet_flops(const CsUNet* u, int batch);
/* FLOPs actually executed by cs_unet_forward(n_lat, dup): with dup = 2 and one timestep the layers in front of the first
 * cross attention are evaluated once for both CFG halves (same latents, same timestep; bit-identical results), so this is
 * slightly below cs_unet_flops(n_lat * dup), which stays the algorithmic count of the reference graph. */
double cs_unet_flops_executed(const CsUNet* u, int n_lat, int dup);

/* latents: [n_lat, C, H, W] (NCHW, fp16).  The effective batch is
 * n_lat * dup (dup = 2 for the CFG dual batch, sample b reads latent b % n_lat;
 * gen_pretrain/pipeline.py:1054).  timesteps: device fp32 [1] or [batch].
 * ctx: [batch, ctx_len, cross_attention_dim] fp16.  out: [batch, C, H, W] fp16.
 * kv_cache_valid != 0 reuses the cross-attention K/V computed by a previous
 * call with the same ctx (they do not depend on latents or t). */
int cs_unet_forward(CsUNet* u, const void* latents, int n_lat, int dup, const float* timesteps,
                    int n_timesteps, const void* ctx, void* out, void* workspace, size_t workspace_bytes,
                    int kv_cache_valid, void* stream);

/* Storage precision of the UNet's RESIDUAL STREAM (resnet outputs, transformer hidden states, proj_out / down / upsample / conv_in
 * outputs) between kernels.  Every GEMM operand is fp16 in both modes (the reference pipeline's own dtype, gen_ppo.py:193-195).
 *   CS_RESIDUAL_F16X2 (default) two fp16 planes per stream tensor, value = hi + lo (22 significant bits): adds onto the stream are carried in fp32
 *                     (hi + lo in, hi + lo out), norms read hi + lo, the resnet shortcut 1x1 multiplies hi + lo (two passes of its k loop), the other GEMMs
 *                     that consume the stream directly read the hi plane.  This is the mode that meets north_star's 1e-3 latent gate against the fp32
 *                     oracle (8-step latents 0.90e-3, tests/test_parity_e2e_gpu.py); it costs the lo planes' bytes (~9 % of the forward).
 *   CS_RESIDUAL_F16   one fp16 tensor per stream tensor: the arithmetic class of the reference's own fp16 pipeline; the 8-step latents land 1.4e-3
 *                     (relative L2) from an fp32 evaluation of the same graph, because every add onto the stream rounds it.
 * Switching changes cs_unet_workspace_bytes(): query it again. */
#define CS_RESIDUAL_F16   0
#define CS_RESIDUAL_F16X2 1
int cs_unet_set_residual_precision(CsUNet* u, int mode);
/* dtype of cs_unet_forward's `out` tensor: CS_F16 (default: the model dtype, what the reference's `unet(...)[0]` returns, denoise_ppo.py:89-94) or CS_F32: conv_out
 * stores its fp32 accumulator unrounded.  The native engine asks for CS_F32: an fp16 eps tensor carries 2.8e-4 of relative rounding, and the CFG combine
 * u + g (c - u) of two such tensors (rounded again as the history entry) more -- both gone from the 1e-3 latent budget for 128 KiB per image and step. */
int cs_unet_set_output_dtype(CsUNet* u, int dtype);
int cs_unet_get_output_dtype(const CsUNet* u);
/* The folded LayerNorm (knob ln_fold, default on) evaluates LN(h) W^T as rstd (h_fp16 W'^T - mean s) + b': exact algebra, but on hidden states whose rows sit many
 * sigma away from zero the two terms cancel in fp16-rounded operands (error ~ 1.6e-4 x |mean| / sigma on that layer's output; synthetic N(0, 1/fan_in) weights
 * never get there, a trained checkpoint's outlier channels can).  cs_unet_calibrate_ln_fold runs ONE forward on representative inputs (same arguments as
 * cs_unet_forward, which it also performs: `out` is valid afterwards), measures per transformer block the RMS over rows of |mean| / sigma of the hidden state in front
 * of each of its LayerNorms -- from the row statistics the producers leave anyway -- and marks the blocks above `bound` (4.0 is the measured default: there the
 * folded form's error is about twice an fp16 LayerNorm output's rounding) to run UNFOLDED from then on (LayerNorm kernel on hi + lo, plain GEMMs) while every other
 * block keeps the fold.  One device -> host read, at load time; the mask is part of the handle (get / set for checkpoints whose mask is known) and changes
 * cs_unet_workspace_bytes(): query it again. */
int cs_unet_calibrate_ln_fold(CsUNet* u, const void* latents, int n_lat, int dup, const float* timesteps, int n_timesteps, const void* ctx, void* out,
                              void* workspace, size_t workspace_bytes, float bound, void* stream, unsigned* mask_out, float* worst_ratio_out);
int cs_unet_set_ln_unfold_mask(CsUNet* u, unsigned mask);
unsigned cs_unet_get_ln_unfold_mask(const CsUNet* u);
/* Kernel-selection knobs for THIS handle (keys and ranges: cs_set_tuning in consolver_hip_ops.h): cs_unet_forward runs with the process-wide values overridden by the
 * handle's entries for the duration of its host call -- a per-thread knob set, the process-wide one is not written -- so two handles in one process can run
 * different knob sets concurrently.  The workspace size does not depend on them (cs_unet_workspace_bytes covers every variant).  Unknown keys and
 * out-of-range values are rejected.  cs_unet_clear_tuning drops the handle's overrides. */
int cs_unet_set_tuning(CsUNet* u, const char* key, int value);
int cs_unet_clear_tuning(CsUNet* u);
int cs_unet_get_residual_precision(const CsUNet* u);

/* per-kernel-class profile of the last forward recorded with events
 * (enable with cs_unet_set_profiling(u, 1); adds synchronisation -- never in a timed run) */
int cs_unet_set_profiling(CsUNet* u, int on);
int cs_unet_profile_entries(const CsUNet* u);
const char* cs_unet_profile_entry(const CsUNet* u, int i, double* ms, double* flops, double* bytes, int* launches);

/* ------------------------------------------------------------------------
 * FLUX.1-Kontext DiT forward (FluxTransformer2DModel): replaces the third-party call
 *   transformer(hidden_states, timestep / 1000, guidance, pooled_projections, encoder_hidden_states,
 *               txt_ids, img_ids)[0]        (edit_ppo/pipeline.py:1087-1097, edit_ppo/denoise_diffusion.py:135-144)
 * ---------------------------------------------------------------------- */
typedef struct CsFluxConfig {
    int in_channels;           /* 64  (packed 2x2 latents)   */
    int num_layers;            /* 19  double-stream blocks   */
    int num_single_layers;     /* 38  single-stream blocks   */
    int num_heads;             /* 24                         */
    int head_dim;              /* 128                        */
    int joint_attention_dim;   /* 4096 (T5)                  */
    int pooled_projection_dim; /* 768  (CLIP pooled)         */
    int guidance_embeds;       /* 1                          */
    int axes_dims_rope[3];     /* 16, 56, 56                 */
    int dtype;                 /* CS_BF16 (reference) or CS_F16 */
} CsFluxConfig;

typedef struct CsFlux CsFlux;

int cs_flux_create(const CsFluxConfig* cfg, CsFlux** out);
void cs_flux_destroy(CsFlux* f);
int cs_flux_num_weights(const CsFlux* f);
const char* cs_flux_weight_name(const CsFlux* f, int i, int64_t* shape2, int* ndim);
/* data: 16-bit elements in the model dtype, diffusers layout; on_device != 0: device pointer (copied). */
int cs_flux_set_weight(CsFlux* f, const char* name, const void* data, int on_device, const int64_t* shape, int ndim);
int cs_flux_finalize(CsFlux* f);
size_t cs_flux_workspace_bytes(const CsFlux* f, int batch, int txt_len, int img_len);
double cs_flux_flops(const CsFlux* f, int batch, int txt_len, int img_len);
/* hidden_states [B, img_len, in_channels], encoder_hidden_states [B, txt_len, joint_attention_dim] (model dtype);
 * pooled_f32 [B, pooled_projection_dim], timestep [B] (= sigma, i.e. t/1000), guidance [B]: device fp32;
 * rope_cos / rope_sin [txt_len + img_len, head_dim/2] device fp32 (host-computed from txt_ids/img_ids,
 * edit_ppo/pipeline.py:574-585); out [B, img_len, in_channels]. */
int cs_flux_forward(CsFlux* f, const void* hidden_states, int batch, int img_len, const void* encoder_hidden_states, int txt_len,
                    const float* pooled_f32, const float* timestep, const float* guidance, const float* rope_cos, const float* rope_sin,
                    void* out, void* workspace, size_t workspace_bytes, void* stream);
/* The Kontext edit step (edit_ppo/pipeline.py:1080-1098, edit_ppo/denoise_diffusion.py:102,135-145) without the per-step
 * `torch.cat([latents, image_latents], dim=1)` and without the `[:, :latents.size(1)]` slice copy: the image sequence is
 * [latents [B, lat_len, C] | image_latents [B, image_len, C]] read from the two buffers in place, rope tables cover
 * txt_len + lat_len + image_len tokens, workspace = cs_flux_workspace_bytes(f, batch, txt_len, lat_len + image_len),
 * out [B, lat_len, C] = the prediction for the latent rows only.  image_len = 0: same as cs_flux_forward. */
int cs_flux_forward_joint(CsFlux* f, const void* latents, int lat_len, const void* image_latents, int image_len, int batch,
                          const void* encoder_hidden_states, int txt_len, const float* pooled_f32, const float* timestep,
                          const float* guidance, const float* rope_cos, const float* rope_sin, void* out, void* workspace,
                          size_t workspace_bytes, void* stream);
/* cs_flux_forward_joint with the latent rows shared between groups of the batch (true classifier-free guidance: [prompt | negative prompt] rows
 * of the SAME latents): latents [latent_rows, lat_len, C] and image_latents [latent_rows, image_len, C], everything else -- encoder_hidden_states,
 * pooled_f32, timestep, guidance, out, the workspace size -- `batch` rows, batch a positive multiple of latent_rows (else CS_E_SHAPE).  Row b of the
 * batch reads latent row b % latent_rows: only the x_embedder reads these buffers, through its row map, so the result equals the call on the
 * repeated tensors bit for bit.  latent_rows == batch is cs_flux_forward_joint. */
int cs_flux_forward_joint_rows(CsFlux* f, const void* latents, int lat_len, const void* image_latents, int image_len, int latent_rows, int batch,
                               const void* encoder_hidden_states, int txt_len, const float* pooled_f32, const float* timestep,
                               const float* guidance, const float* rope_cos, const float* rope_sin, void* out, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Storage of the DiT's hidden-state (residual) stream between kernels, as for the UNet (CS_RESIDUAL_* above): CS_RESIDUAL_F16X2 (default) keeps the image / text /
 * joint hidden states as two planes of the model dtype (value = hi + lo): the 57 + 38 gated-residual epilogues add in fp32 and write both planes, the adaLN
 * LayerNorms read both; every GEMM operand stays a plain 16-bit tensor.  CS_RESIDUAL_F16: one plane -- the reference bf16 pipeline's own arithmetic class.  At
 * full depth (19 + 38 blocks, bf16) the one-plane stream is 1.16e-2 of the forward's 1.2e-2 relative error against an fp32 evaluation (tools/sim_precision_flux.py).
 * Changes the workspace size: query cs_flux_workspace_bytes after switching. */
int cs_flux_set_residual_precision(CsFlux* f, int mode);
int cs_flux_get_residual_precision(const CsFlux* f);
/* dtype of cs_flux_forward(_joint)'s `out`: the model dtype (default: what the reference's `transformer(...)[0]` returns, edit_ppo/pipeline.py:1087-1097) or CS_F32.
 * With the split stream the output head keeps its two tensors -- the modulated LayerNorm output and proj_out's result -- as hi + lo planes (round 6: they were the
 * last one-plane stations of the stream's value, 3.42e-3 -> 2.5e-3 per forward at full depth): the model-dtype `out` is the hi plane, the fp32 `out` the sum of
 * the two.  CS_F32 with CS_RESIDUAL_F16 (one plane) is refused at the forward. */
int cs_flux_set_output_dtype(CsFlux* f, int dtype);
int cs_flux_get_output_dtype(const CsFlux* f);

/* ------------------------------------------------------------------------
 * AutoencoderKL decoder (SD1.5 VAE): latents -> images.  Replaces
 * `vae.decode(latents / vae.config.scaling_factor).sample` and the
 * `(image / 2 + 0.5).clamp(0, 1)` that follows it in decode_latents
 * (utils.py:6-34; gen_pretrain/pipeline.py:589-593).
 * ---------------------------------------------------------------------- */
typedef struct CsVaeConfig {
    int latent_channels, out_channels; /* 4, 3                          */
    int block_out_channels[4];         /* 128, 256, 512, 512            */
    int layers_per_block;              /* 2 (decoder blocks hold 3)     */
    int norm_num_groups;               /* 32                            */
    int sample_size;                   /* 64 (latent H = W); FLUX 128   */
    int use_post_quant_conv;           /* 1 (SD1.5); 0 for the FLUX VAE (16 latent channels) */
    int with_encoder;                  /* 1: also load "encoder.*" [+ "quant_conv.*"] and enable cs_vae_encode */
    int use_quant_conv;                /* 1 (SD1.5); 0 for the FLUX VAE */
} CsVaeConfig;

typedef struct CsVae CsVae;

int cs_vae_create(const CsVaeConfig* cfg, CsVae** out);
void cs_vae_destroy(CsVae* v);
/* tensors by their diffusers AutoencoderKL state-dict names ("post_quant_conv.weight",
 * "decoder.up_blocks.0.resnets.0.conv1.weight", ...); fp32 host memory, PyTorch layout */
int cs_vae_set_weight(CsVae* v, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_vae_num_weights(const CsVae* v);
const char* cs_vae_weight_name(const CsVae* v, int i, int64_t* shape4, int* ndim);
int cs_vae_finalize(CsVae* v);
size_t cs_vae_workspace_bytes(const CsVae* v, int batch);
double cs_vae_flops(const CsVae* v, int batch);
/* latents: [batch, 4, h, w] NCHW fp16 (device).  The decoder input is
 * latents * in_scale + in_shift (in_scale = 1 / scaling_factor, utils.py:21).
 * images: [batch, 3, 8h, 8w] NCHW fp16; postprocess != 0 applies
 * (x / 2 + 0.5).clamp(0, 1) (utils.py:29) in the last kernel. */
int cs_vae_decode(CsVae* v, const void* latents, int batch, float in_scale, float in_shift, void* images,
                  int postprocess, void* workspace, size_t workspace_bytes, void* stream);
/* Encoder (edit_ppo/pipeline.py:613-623, `retrieve_latents(vae.encode(image), sample_mode="argmax")`):
 * images [batch, 3, 8h, 8w] NCHW fp16 in [-1, 1] -> latents [batch, L, h, w] fp16 =
 * (mode of the posterior - out_shift) * out_scale   (FLUX: shift_factor, scaling_factor). */
size_t cs_vae_encode_workspace_bytes(const CsVae* v, int batch);
int cs_vae_encode(CsVae* v, const void* images, int batch, float out_scale, float out_shift, void* latents,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * PPO rollout consumer arithmetic (train_ppo.py:352-427)
 * ---------------------------------------------------------------------- */
/* Per-image PSNR of two image batches [B, elems] (fp16 or fp32, values in [0,1]):
 * clamp(10 log10(1 / (mean((pred - target)^2) + 1e-8)), 0, clamp_hi) -> out[B] fp32.
 * clamp_hi = 100 is calculate_image_psnr_reward (edit_ppo/reward_model.py:484-509);
 * clamp_hi <= 0 means "clamp(min=0) only", the PSNR tail of the depth reward (:404-422). */
size_t cs_psnr_workspace_bytes(int batch);
int cs_image_psnr(const void* pred, const void* target, int B, int64_t elems, int dtype, float clamp_hi,
                  float* out, void* workspace, size_t workspace_bytes, void* stream);
/* cs_image_psnr with target row b at target + b * target_stride elements: target_stride = 0 is ONE target image shared by all B
 * predictions (the trainer's B copies of one teacher image), target_stride = elems is cs_image_psnr.  The same two kernels. */
int cs_image_psnr_bcast(const void* pred, const void* target, int B, int64_t elems, int dtype, float clamp_hi,
                        float* out, void* workspace, size_t workspace_bytes, void* stream, int64_t target_stride);
/* dst[r][:] = src[index[r]][:] for r < rows_out, rows of `elems` elements of dtype CS_F32 | CS_F16 | CS_BF16 (the grouped rollout: the
 * representative latents of each group of equal rows, and a group's denoiser output handed to each of its rows).  16-byte vectors when
 * elems * element size is a multiple of 16 and both pointers are 16-byte aligned, one element per lane otherwise.  dst must not overlap
 * src (CS_E_ARG).  An index outside [0, rows_src) is never turned into an address: that row of dst is filled with NaN.
 * rows_out == 0 or elems == 0: no-op.  Argument errors are negative codes before any launch. */
int cs_gather_rows(const void* src, int rows_src, const int64_t* index, int rows_out, int64_t elems, int dtype, void* dst, void* stream);
/* advantages[(b, j), a] = (r[b] - mean(r)) / (std_unbiased(r) + 1e-8) * 10 * masks[(b, j), a],
 * j over the recorded steps (n - 1) (train_ppo.py:376-390).  All fp32. */
int cs_ppo_advantages(const float* rewards, int B, int recorded_steps, int A, const float* masks,
                      float* out, void* stream);
/* The FLUX trainer's form (edit_ppo/train_ppo.py:326-341): advantages[(b, j), a] =
 * (r[b] - min(max(mean(r), *base_reward), clip_hi)) / (std_unbiased(r) + 1e-8) * masks[(b, j), a] -- no x 10.
 * base_reward: ONE fp32 on the device (the reward of the baseline rollout), so no host sync sits
 * between reward and update.  One workgroup, no atomics: deterministic.  All fp32. */
int cs_ppo_advantages_baseline(const float* rewards, const float* base_reward, float clip_hi, int B,
                               int recorded_steps, int A, const float* masks, float* out, void* stream);
/* value of the clipped surrogate + entropy bonus (train_ppo.py:408-421); inputs [R, A] fp32,
 * loss: one fp32 on the device. */
int cs_ppo_loss(const float* curr_probs, const float* old_probs, const float* entropy,
                const float* advantages, int R, int A, float clip_range, float entropy_coef,
                float* loss, void* stream);

/* ------------------------------------------------------------------------
 * PPO policy update (train_ppo.py:404-437): gradients of the loss with respect to the
 * factor net, clip_grad_norm_, AdamW.  All fp32 device memory.
 * ---------------------------------------------------------------------- */
/* number of trainable parameters = floats in the packed gradient vector, laid out in state-dict
 * order: mlp.0.weight [H, in], mlp.0.bias, mlp.2.weight [H, H], mlp.2.bias, mlp.4.weight [A K, H], mlp.4.bias */
size_t cs_policy_param_count(const CsFactorNet* net);
size_t cs_policy_workspace_bytes(const CsFactorNet* net, int R);
/* x [R, 2] (timestep pairs, un-normalised), cos_feat [R, in_dim - 2] or NULL, actions / old_probs / advantages [R, A],
 * action_values [A, K] -> grads (packed, see above) = d loss / d params, loss (one float, may be NULL) with
 * loss = -mean min(adv rho, adv clip(rho, 1 +- clip_range)) - entropy_coef mean(H / ln K) (train_ppo.py:408-427). */
int cs_ppo_policy_grads(const CsFactorNet* net, const float* x, const float* cos_feat, const float* actions,
                        const float* action_values, const float* old_probs, const float* advantages, int R,
                        float clip_range, float entropy_coef, float* grads, float* loss,
                        void* workspace, size_t workspace_bytes, void* stream);
/* torch.nn.utils.clip_grad_norm_ over one packed vector (train_ppo.py:432-435); total_norm may be NULL */
int cs_clip_grad_norm(float* grads, int64_t n, float max_norm, float* total_norm, void* stream);
/* one torch.optim.AdamW step on one tensor (train_ppo.py:223-229,436); step counts from 1 */
int cs_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------------
 * CLIP text encoder (prompt front-end): replaces `text_encoder(input_ids)[0]`
 * (denoise_ppo.py:25-50; third-party transformers CLIPTextModel).
 * ---------------------------------------------------------------------- */
typedef struct CsClipConfig {
    int vocab_size;                /* 49408 */
    int hidden_size;               /* 768   */
    int intermediate_size;         /* 3072  */
    int num_hidden_layers;         /* 12    */
    int num_attention_heads;       /* 12 (head dim 64) */
    int max_position_embeddings;   /* 77    */
    float layer_norm_eps;          /* 1e-5  */
} CsClipConfig;

typedef struct CsClip CsClip;

int cs_clip_create(const CsClipConfig* cfg, CsClip** out);
void cs_clip_destroy(CsClip* c);
/* tensors by their transformers CLIPTextModel names without the "text_model." prefix
 * ("embeddings.token_embedding.weight", "encoder.layers.0.self_attn.q_proj.weight", ...); fp32 host memory */
int cs_clip_set_weight(CsClip* c, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_clip_num_weights(const CsClip* c);
const char* cs_clip_weight_name(const CsClip* c, int i, int64_t* shape4, int* ndim);
int cs_clip_finalize(CsClip* c);
size_t cs_clip_workspace_bytes(const CsClip* c, int batch, int seq_len);
double cs_clip_flops(const CsClip* c, int batch, int seq_len);
/* input_ids: [batch, seq_len] int64 (device).  out: last_hidden_state [batch, seq_len, hidden] fp16
 * (after final_layer_norm), i.e. element [0] of the reference's text_encoder(...) output. */
int cs_clip_encode(CsClip* c, const int64_t* input_ids, int batch, int seq_len, void* out,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * DINOv2 image-similarity reward (reward_type "dino": edit_ppo/reward_model.py:217-257;
 * third-party transformers Dinov2Model + the facebook/dinov2-base image processor).
 * ---------------------------------------------------------------------- */
typedef struct CsVitConfig {
    int hidden_size;               /* 768   */
    int num_hidden_layers;         /* 12    */
    int num_attention_heads;       /* 12 (head dim 64) */
    int mlp_ratio;                 /* 4     */
    int image_size;                /* 518: the position table's training grid is (image_size / patch_size)^2 */
    int patch_size;                /* 14    */
    float layer_norm_eps;          /* 1e-6  */
    /* the processor's constants */
    int resize_shortest_edge;      /* 256 (PIL BICUBIC) */
    int crop_size;                 /* 224 (center crop; the encoder then sees (crop_size / patch_size)^2 + 1 tokens) */
    float image_mean[3];           /* 0.485, 0.456, 0.406 */
    float image_std[3];            /* 0.229, 0.224, 0.225 */
    double rescale_factor;         /* 1 / 255: the processor rescales in double, rounds to fp32, then normalises in fp32 */
} CsVitConfig;

typedef struct CsVit CsVit;

/* host only: builds the weight manifest, touches no GPU */
int cs_vit_create(const CsVitConfig* cfg, CsVit** out);
void cs_vit_destroy(CsVit* v);
/* tensors by their transformers Dinov2Model state-dict names ("embeddings.cls_token", "encoder.layer.0.attention.attention.query.weight",
 * "encoder.layer.0.layer_scale1.lambda1", ..., "embeddings.mask_token" included: it is part of the checkpoint, unused by the forward); fp32 host memory */
int cs_vit_set_weight(CsVit* v, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_vit_num_weights(const CsVit* v);
const char* cs_vit_weight_name(const CsVit* v, int i, int64_t* shape4, int* ndim);
int cs_vit_finalize(CsVit* v);
size_t cs_vit_workspace_bytes(const CsVit* v, int batch);
double cs_vit_flops(const CsVit* v, int batch);
/* row length of the patch matrix (3 * patch_size^2 padded to a multiple of 64) and tokens per image */
int cs_vit_patch_cols(const CsVit* v);
int cs_vit_num_tokens(const CsVit* v);
size_t cs_vit_preprocess_workspace_bytes(const CsVit* v, int batch, int height, int width);
/* images: [batch, 3, height, width] CS_F16 or CS_F32 (device), values clamped to [0, 1].  ToPILImage (x * 255 in the tensor's dtype,
 * truncated) -> PIL's fixed-point bicubic resize to shortest edge resize_shortest_edge -> center crop -> rescale, normalise.
 * patches: [batch * (crop/patch)^2, cs_vit_patch_cols] fp16, the encoder's input.  crop_u8 (may be NULL): the resized and cropped
 * uint8 image [batch, 3, crop, crop], bit-identical to PIL's.  Sizes whose resized image is smaller than the crop: CS_E_UNSUPPORTED.
 * The first call with a new (height, width) builds that size's tap tables on the host and uploads them (hipMalloc + a synchronous copy on the
 * current device; not capturable into a graph); the handle keeps the tables of the last 16 sizes at most.  One thread per handle. */
int cs_vit_preprocess(CsVit* v, const void* images, int dtype, int batch, int height, int width, void* patches,
                      unsigned char* crop_u8, void* workspace, size_t workspace_bytes, void* stream);
/* patches from cs_vit_preprocess -> cls_out [batch, hidden] fp32 = last_hidden_state[:, 0] (after the final LayerNorm) */
int cs_vit_forward(CsVit* v, const void* patches, int batch, float* cls_out, void* workspace, size_t workspace_bytes,
                   void* stream);
/* out[b] = (cosine_similarity(normalize(pred[b]), normalize(target[b])) + 1) * 50, all fp32; target rows are target_stride floats
 * apart (0: one target row for the whole batch) */
int cs_cosine_reward(const float* pred, const float* target, int batch, int dim, int64_t target_stride, float* out,
                     void* stream);

/* ------------------------------------------------------------------------
 * CLIP image-similarity reward (reward_type "clip": edit_ppo/reward_model.py:128-134, 512-552;
 * third-party transformers CLIPModel.get_image_features + the openai/clip-vit-large-patch14 image processor).
 * ---------------------------------------------------------------------- */
typedef struct CsClipVisionConfig {
    int hidden_size;               /* 1024  */
    int intermediate_size;         /* 4096  */
    int num_hidden_layers;         /* 24    */
    int num_attention_heads;       /* 16 (head dim 64) */
    int image_size;                /* 224: the position table has (image_size / patch_size)^2 + 1 rows, no interpolation */
    int patch_size;                /* 14    */
    int projection_dim;            /* 768   */
    float layer_norm_eps;          /* 1e-5  */
    /* the processor's constants */
    int resize_shortest_edge;      /* 224 (PIL BICUBIC) */
    int crop_size;                 /* 224 (center crop; must equal image_size) */
    float image_mean[3];           /* 0.48145466, 0.4578275, 0.40821073 */
    float image_std[3];            /* 0.26862954, 0.26130258, 0.27577711 */
    double rescale_factor;         /* 1 / 255: the processor rescales in double, rounds to fp32, then normalises in fp32 */
} CsClipVisionConfig;

typedef struct CsClipVision CsClipVision;

/* host only: builds the weight manifest, touches no GPU */
int cs_clipv_create(const CsClipVisionConfig* cfg, CsClipVision** out);
void cs_clipv_destroy(CsClipVision* v);
/* tensors by their transformers CLIPModel / CLIPVisionModelWithProjection state-dict names ("vision_model.embeddings.class_embedding",
 * "vision_model.pre_layrnorm.weight" -- transformers' own spelling --, "vision_model.encoder.layers.0.self_attn.k_proj.weight", ...,
 * "visual_projection.weight"); fp32 host memory */
int cs_clipv_set_weight(CsClipVision* v, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_clipv_num_weights(const CsClipVision* v);
const char* cs_clipv_weight_name(const CsClipVision* v, int i, int64_t* shape4, int* ndim);
int cs_clipv_finalize(CsClipVision* v);
size_t cs_clipv_workspace_bytes(const CsClipVision* v, int batch);
double cs_clipv_flops(const CsClipVision* v, int batch);
/* row length of the patch matrix (3 * patch_size^2 padded to a multiple of 64) and tokens per image */
int cs_clipv_patch_cols(const CsClipVision* v);
int cs_clipv_num_tokens(const CsClipVision* v);
size_t cs_clipv_preprocess_workspace_bytes(const CsClipVision* v, int batch, int height, int width);
/* the image front end of cs_vit_preprocess with this handle's processor constants (same contract) */
int cs_clipv_preprocess(CsClipVision* v, const void* images, int dtype, int batch, int height, int width, void* patches,
                        unsigned char* crop_u8, void* workspace, size_t workspace_bytes, void* stream);
/* patches from cs_clipv_preprocess -> image_embeds [batch, projection_dim] fp32 = visual_projection(post_layernorm(CLS row)) */
int cs_clipv_forward(CsClipVision* v, const void* patches, int batch, float* image_embeds, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------
 * Depth Anything V2 depth-map PSNR reward (reward_type "depth": edit_ppo/reward_model.py:92-96, 359-422;
 * third-party transformers DepthAnythingForDepthEstimation + the depth-anything/Depth-Anything-V2-Small-hf DPT image processor).
 * ---------------------------------------------------------------------- */
typedef struct CsDepthConfig {
    /* backbone: DINOv2 */
    int hidden_size;               /* 384   */
    int num_hidden_layers;         /* 12    */
    int num_attention_heads;       /* 6 (head dim 64) */
    int mlp_ratio;                 /* 4     */
    int image_size;                /* 518: the position table's grid (image_size / patch_size)^2; must equal `size` (the table is used as it is) */
    int patch_size;                /* 14    */
    float layer_norm_eps;          /* 1e-6  */
    int out_indices[4];            /* 3, 6, 9, 12: the hidden states (after that many layers, final LayerNorm applied) the neck reads; increasing */
    /* neck and head */
    int neck_hidden_sizes[4];      /* 48, 96, 192, 384 */
    int fusion_hidden_size;        /* 64 (the only width built) */
    int head_hidden_size;          /* 32 (32 or 64) */
    float max_depth;               /* 1 (depth_estimation_type "relative": ReLU x max_depth) */
    /* the processor's constants */
    int size;                      /* 518: PIL BICUBIC resize to size x size (keep_aspect_ratio, ensure_multiple_of = patch_size: square inputs only) */
    float image_mean[3];           /* 0.485, 0.456, 0.406 */
    float image_std[3];            /* 0.229, 0.224, 0.225 */
    double rescale_factor;         /* 1 / 255 */
} CsDepthConfig;

typedef struct CsDepth CsDepth;

/* host only: builds the weight manifest, touches no GPU */
int cs_depth_create(const CsDepthConfig* cfg, CsDepth** out);
void cs_depth_destroy(CsDepth* d);
/* tensors by their transformers DepthAnythingForDepthEstimation state-dict names ("backbone.embeddings.cls_token", ...,
 * "neck.reassemble_stage.layers.0.resize.weight", "neck.fusion_stage.layers.0.residual_layer1.convolution1.weight", "head.conv3.bias"); fp32 host memory */
int cs_depth_set_weight(CsDepth* d, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_depth_num_weights(const CsDepth* d);
const char* cs_depth_weight_name(const CsDepth* d, int i, int64_t* shape4, int* ndim);
int cs_depth_finalize(CsDepth* d);
size_t cs_depth_workspace_bytes(const CsDepth* d, int batch);
double cs_depth_flops(const CsDepth* d, int batch);
int cs_depth_patch_cols(const CsDepth* d);
int cs_depth_num_tokens(const CsDepth* d);
size_t cs_depth_preprocess_workspace_bytes(const CsDepth* d, int batch, int height, int width);
/* the image front end of cs_vit_preprocess with the DPT processor's rule: the whole image resized to size x size, no crop.  height != width (where the
 * processor's keep_aspect_ratio rule gives another shape): CS_E_UNSUPPORTED -- the output shape of this entry point implies the square grid;
 * cs_depth_preprocess_hw takes any aspect ratio.  crop_u8 (may be NULL): the resized uint8 image [batch, 3, size, size] */
int cs_depth_preprocess(CsDepth* d, const void* images, int dtype, int batch, int height, int width, void* patches,
                        unsigned char* crop_u8, void* workspace, size_t workspace_bytes, void* stream);
/* patches from cs_depth_preprocess -> predicted_depth [batch, size, size] fp32 */
int cs_depth_forward(CsDepth* d, const void* patches, int batch, float* predicted_depth, void* workspace, size_t workspace_bytes,
                     void* stream);
/* post_process_depth_estimation + the reward's normalisation: predicted_depth [batch, size, size] fp32 -> torch-style bicubic (align_corners = False) to
 * height x width -> per map (d - min) / (max - min + 1e-8): maps [batch, height, width] fp32 */
int cs_depth_normalized_maps(CsDepth* d, const float* predicted_depth, int batch, int height, int width, float* maps, void* stream);

/* ---- images of any aspect ratio: the `_hw` entry points.  The square entry points above are their (size, size) case, bit for bit. ----
 * Size rule: the DPT processor's with keep_aspect_ratio and ensure_multiple_of = patch_size.  scale_h = size / height, scale_w = size / width; the scale
 * closer to 1 serves both axes; each side becomes round-half-even(scale * side / patch_size) * patch_size (in double, as the processor computes it).
 * 880 x 1184 -> 518 x 700, 512 x 768 -> 518 x 784, 64 x 96 -> 350 x 518.
 * Limits: height and width 1 .. 16384; each processed side 1 patch .. CS_DEPTH_MAX_SIDE_FACTOR * size (size 518: up to 1554, a 111-patch side; every aspect
 * ratio up to 3:1 of images no smaller than the processor's size is inside, 672 x 1568 -> 518 x 1204 = 37 x 86 patches).  Beyond them every entry point
 * below answers CS_E_UNSUPPORTED (the size_t ones 0) before any allocation or launch. */
#define CS_DEPTH_MAX_SIDE_FACTOR 3
int cs_depth_processed_size(const CsDepth* d, int height, int width, int* out_h, int* out_w);
size_t cs_depth_preprocess_workspace_bytes_hw(const CsDepth* d, int batch, int height, int width);
/* PIL BICUBIC on the uint8 image straight to out_h x out_w (the two axes on independent scales, no crop; bit-identical to Image.resize), rescale, normalise:
 * patches [batch * (out_h / patch) * (out_w / patch)][patch_cols] fp16.  out_h / out_w (may be NULL): the processed size.  crop_u8 (may be NULL): the resized
 * uint8 image [batch, 3, out_h, out_w].  The resize tables of an image size are built on its first call and kept (a bounded cache, shared with the square
 * entry point's). */
int cs_depth_preprocess_hw(CsDepth* d, const void* images, int dtype, int batch, int height, int width, int* out_h, int* out_w, void* patches,
                           unsigned char* crop_u8, void* workspace, size_t workspace_bytes, void* stream);
/* workspace and FLOPs of one cs_depth_forward_hw call at a processed size (multiples of patch_size within the limits) */
size_t cs_depth_workspace_bytes_hw(const CsDepth* d, int batch, int out_h, int out_w);
double cs_depth_flops_hw(const CsDepth* d, int batch, int out_h, int out_w);
/* patches from cs_depth_preprocess_hw -> predicted_depth [batch, out_h, out_w] fp32.  A patch grid other than the training grid reads a position table that
 * is interpolated on the device (torch's bicubic, align_corners = False, fp32 arithmetic, one rounding to fp16) from the trained fp32 grid the handle keeps,
 * on the first call at that grid: one hipMalloc, one kernel and a stream synchronisation then; the handle keeps at most 16 tables and empties the cache when it
 * is full.  The training grid reads the packed table and launches nothing more than cs_depth_forward. */
int cs_depth_forward_hw(CsDepth* d, const void* patches, int batch, int out_h, int out_w, float* predicted_depth, void* workspace, size_t workspace_bytes,
                        void* stream);
/* cs_depth_normalized_maps for predicted_depth [batch, in_h, in_w] */
int cs_depth_normalized_maps_hw(CsDepth* d, const float* predicted_depth, int batch, int in_h, int in_w, int height, int width, float* maps, void* stream);
/* the position table [1 + gh * gw][hidden_size] fp16 the forward reads at a gh x gw patch grid (row 0, the class row, is zero: the packed CLS token carries
 * it), copied to `table` (device memory); *kernel_launched (may be NULL): 1 when this call interpolated the table, 0 for the training grid or a cached table */
int cs_depth_position_table(CsDepth* d, int gh, int gw, void* table, int* kernel_launched, void* stream);

/* ------------------------------------------------------------------------
 * SegFormer mask-agreement reward (reward_type "segmentation": edit_ppo/reward_model.py:110-117, 425-481;
 * third-party transformers SegformerForSemanticSegmentation + the nvidia/segformer-b4-finetuned-ade-512-512 Segformer image processor).
 * Every LayerNorm of the model and its BatchNorm use eps = 1e-5 (the torch defaults; config.layer_norm_eps is not read by them).
 * ---------------------------------------------------------------------- */
typedef struct CsSegConfig {
    /* MiT encoder, four stages */
    int hidden_sizes[4];           /* 64, 128, 320, 512: each 64 or a multiple of 128 or 160 */
    int depths[4];                 /* 3, 8, 27, 3 */
    int num_attention_heads[4];    /* 1, 2, 5, 8 (head dim 64 in every stage) */
    int sr_ratios[4];              /* 8, 4, 2, 1: kernel = stride of the sequence reduction in front of keys / values (1: none) */
    int mlp_ratio;                 /* 4 */
    /* all-MLP head */
    int decoder_hidden_size;       /* 768 */
    int num_labels;                /* 150 */
    /* the processor's constants */
    int size;                      /* 512: PIL BILINEAR resize to size x size (square inputs only), a multiple of 32 */
    float image_mean[3];           /* 0.485, 0.456, 0.406 */
    float image_std[3];            /* 0.229, 0.224, 0.225 */
    double rescale_factor;         /* 1 / 255 */
} CsSegConfig;

typedef struct CsSeg CsSeg;

/* host only: builds the weight manifest, touches no GPU */
int cs_seg_create(const CsSegConfig* cfg, CsSeg** out);
void cs_seg_destroy(CsSeg* g);
/* tensors by their transformers SegformerForSemanticSegmentation state-dict names ("segformer.stages.0.patch_embeddings.proj.weight", ...,
 * "decode_head.classifier.bias"); fp32 host memory.  "decode_head.batch_norm.num_batches_tracked" (0-d: ndim 0) is accepted and ignored */
int cs_seg_set_weight(CsSeg* g, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_seg_num_weights(const CsSeg* g);
const char* cs_seg_weight_name(const CsSeg* g, int i, int64_t* shape4, int* ndim);
int cs_seg_finalize(CsSeg* g);
size_t cs_seg_workspace_bytes(const CsSeg* g, int batch);
double cs_seg_flops(const CsSeg* g, int batch);
/* row length of the front end's output (one pixel per row: 3 channels zero-padded to 8 halfs) and stage-1 tokens per image ((size / 4)^2) */
int cs_seg_patch_cols(const CsSeg* g);
int cs_seg_num_tokens(const CsSeg* g);
size_t cs_seg_preprocess_workspace_bytes(const CsSeg* g, int batch, int height, int width);
/* the image front end of cs_vit_preprocess with the Segformer processor's rule: the whole image resized to size x size with PIL BILINEAR, no crop; `patches`
 * is the normalised image [batch * size * size][8] fp16 (NHWC, channels 3 .. 7 zero).  height != width: CS_E_UNSUPPORTED (cs_seg_preprocess_hw takes any
 * aspect ratio).  crop_u8 (may be NULL): the resized
 * uint8 image [batch, 3, size, size] (an input of the processor's own size comes out byte-identical) */
int cs_seg_preprocess(CsSeg* g, const void* images, int dtype, int batch, int height, int width, void* patches,
                      unsigned char* crop_u8, void* workspace, size_t workspace_bytes, void* stream);
/* the same for an image of any aspect ratio: the Segformer processor stretches it to size x size (PIL BILINEAR, the two axes on independent scales, bit-identical
 * to Image.resize), so *out_h = *out_w = size (may be NULL), the outputs have the square call's shapes and cs_seg_forward takes them as they are.  Workspace:
 * cs_seg_preprocess_workspace_bytes of the same height and width */
int cs_seg_preprocess_hw(CsSeg* g, const void* images, int dtype, int batch, int height, int width, int* out_h, int* out_w, void* patches,
                         unsigned char* crop_u8, void* workspace, size_t workspace_bytes, void* stream);
/* patches from cs_seg_preprocess -> logits [batch, num_labels, size / 4, size / 4] fp32 (NULL: not written; the fp16 logits stay in the workspace for cs_seg_masks) */
int cs_seg_forward(CsSeg* g, const void* patches, int batch, float* logits, void* workspace, size_t workspace_bytes,
                   void* stream);
/* timing tools: cs_seg_forward returns after `parts` of (stage 1, 2, 3, 4, head); 5 (the default) runs everything, less leaves logits and masks undefined */
int cs_seg_set_stage_limit(CsSeg* g, int parts);
/* argmax over the classes of the logits the last cs_seg_forward of this batch size left in `workspace` (a tie goes to the lowest class): masks
 * [batch, size / 4, size / 4] int32 */
int cs_seg_masks(CsSeg* g, int batch, const void* workspace, size_t workspace_bytes, int* masks, void* stream);
/* the reward's tail: out[b] = 100 * mean(pred[b] == target[b]) fp32 over n pixels; int32 device masks, target rows target_stride ints apart (0: one target
 * shared by the batch) */
int cs_seg_agreement(const int* pred, const int* target, int64_t target_stride, int batch, int64_t n, float* out, void* stream);

/* ------------------------------------------------------------------------
 * Inception-v3 logit-cosine reward (reward_type "inception": edit_ppo/reward_model.py:98-108, 319-356; third-party torchvision
 * inception_v3(aux_logits=True, transform_input=False) in eval mode behind Resize(size, BICUBIC) + CenterCrop(size) + ToTensor + Normalize).
 * The widths are the architecture's; every BatchNorm has eps = 1e-3 and is folded into its convolution at finalize.  AuxLogits is never evaluated.
 * ---------------------------------------------------------------------- */
typedef struct CsIncepConfig {
    int image_size;                /* 299: the resize's shortest edge and the center crop (75 .. 2048) */
    int num_classes;               /* 1000 */
    float image_mean[3];           /* 0.485, 0.456, 0.406 */
    float image_std[3];            /* 0.229, 0.224, 0.225 */
    double rescale_factor;         /* 1 / 255 */
} CsIncepConfig;

typedef struct CsIncep CsIncep;

/* host only: builds the weight manifest, touches no GPU */
int cs_incep_create(const CsIncepConfig* cfg, CsIncep** out);
void cs_incep_destroy(CsIncep* g);
/* tensors by their torchvision Inception3 state-dict names ("Conv2d_1a_3x3.conv.weight", "Conv2d_1a_3x3.bn.running_var", ..., "fc.bias"); fp32 host memory.
 * "....bn.num_batches_tracked" (0-d: ndim 0) and every "AuxLogits.*" tensor of a real checkpoint are accepted and ignored */
int cs_incep_set_weight(CsIncep* g, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_incep_num_weights(const CsIncep* g);
const char* cs_incep_weight_name(const CsIncep* g, int i, int64_t* shape4, int* ndim);
int cs_incep_finalize(CsIncep* g);
size_t cs_incep_workspace_bytes(const CsIncep* g, int batch);
double cs_incep_flops(const CsIncep* g, int batch);
/* row length of the front end's output (one pixel per row: 3 channels zero-padded to 8 halfs) and positions of the last grid per image */
int cs_incep_patch_cols(const CsIncep* g);
int cs_incep_num_tokens(const CsIncep* g);
size_t cs_incep_preprocess_workspace_bytes(const CsIncep* g, int batch, int height, int width);
/* the image front end of cs_vit_preprocess with torchvision's rules: PIL BICUBIC resize of the shortest edge to image_size, center crop at
 * int(round((n - image_size) / 2.0)) (round half to even), any height x width whose resized sides reach image_size; `patches` is the normalised image
 * [batch * image_size * image_size][8] fp16 (NHWC, channels 3 .. 7 zero).  crop_u8 (may be NULL): the cropped uint8 image [batch, 3, image_size, image_size] */
int cs_incep_preprocess(CsIncep* g, const void* images, int dtype, int batch, int height, int width, void* patches,
                        unsigned char* crop_u8, void* workspace, size_t workspace_bytes, void* stream);
/* patches from cs_incep_preprocess -> the logits of fc [batch, num_classes] fp32 */
int cs_incep_forward(CsIncep* g, const void* patches, int batch, float* logits, void* workspace, size_t workspace_bytes,
                     void* stream);
/* timing tools: cs_incep_forward returns after `parts` of (stem, Mixed_5, Mixed_6, Mixed_7, head); 5 (the default) runs everything, less leaves logits undefined */
int cs_incep_set_stage_limit(CsIncep* g, int parts);

/* ------------------------------------------------------------------------
 * FID (the first column of the reference's results table; fid_test.py: cleanfid.fid.compute_fid(generated_dir, "coco/val2017")).
 * Three pieces: clean-fid's resize (every channel a PIL mode-"F" image, BICUBIC straight to 299 x 299 in floating point, clipped to [0, 255]), the FID
 * variant of Inception-v3 (pytorch-fid's pt_inception-2015-12-05: torchvision's state-dict names; 3x3 average pools that divide by the taps inside the
 * image; a max pool in Mixed_7c's pool branch; the 2048-d pool3 output) and fp64 feature statistics.  cleanfid is not installed here: the 299, the clip and
 * the (x - 128) / 128 default are restated from memory.
 * ---------------------------------------------------------------------- */
typedef struct CsFidConfig {
    float image_mean[3];           /* 128, 128, 128: on the 0 .. 255 scale of the resized image */
    float image_std[3];            /* 128, 128, 128 */
} CsFidConfig;

typedef struct CsFid CsFid;

/* host only: builds the weight manifest (cs_incep_*'s without fc), touches no GPU */
int cs_fid_create(const CsFidConfig* cfg, CsFid** out);
void cs_fid_destroy(CsFid* g);
/* as cs_incep_set_weight; "fc.*" (1008 classes in that checkpoint) and "AuxLogits.*" are accepted and ignored */
int cs_fid_set_weight(CsFid* g, const char* name, const float* data_host, const int64_t* shape, int ndim);
int cs_fid_num_weights(const CsFid* g);
const char* cs_fid_weight_name(const CsFid* g, int i, int64_t* shape4, int* ndim);
int cs_fid_finalize(CsFid* g);
size_t cs_fid_workspace_bytes(const CsFid* g, int batch);
double cs_fid_flops(const CsFid* g, int batch);
int cs_fid_patch_cols(const CsFid* g);      /* 8 */
int cs_fid_num_tokens(const CsFid* g);      /* 64: the last grid is 8 x 8 */
size_t cs_fid_preprocess_workspace_bytes(const CsFid* g, int batch, int height, int width);
/* images [batch, 3, height, width], CS_U8 or CS_F16 / CS_F32 in [0, 1] (quantised first as round(clamp(x, 0, 1) * 255), half to even), any height, width
 * >= 1.  PIL's ImagingResample for 32-bit float images to 299 x 299: horizontal pass first, stored as fp32, then the vertical pass; double taps (not the
 * 2^22 fixed point of the uint8 path), double accumulation ascending from xmin; a side that is 299 already is a copy.  The result is clipped to [0, 255];
 * `patches` is ((v - image_mean[c]) / image_std[c]) as [batch * 299 * 299][8] fp16 (NHWC, channels 3 .. 7 zero).  resized_f32 (may be NULL): the clipped
 * image before normalisation [batch, 3, 299, 299] fp32 */
int cs_fid_preprocess(CsFid* g, const void* images, int dtype, int batch, int height, int width, void* patches, float* resized_f32,
                      void* workspace, size_t workspace_bytes, void* stream);
/* patches from cs_fid_preprocess -> the pool3 features [batch, 2048] fp32: the mean of the last 8 x 8 x 2048 grid, never rounded to fp16 */
int cs_fid_forward(CsFid* g, const void* patches, int batch, float* features, void* workspace, size_t workspace_bytes, void* stream);

/* feature statistics in fp64 (device pointers): sum[j] += sum_r f[r][j], outer[i][j] += sum_r f[r][i] f[r][j] over the n rows of feats [n][d] fp32; the whole
 * symmetric matrix is written.  Every output element is owned by one workgroup that walks the rows in order (no atomics): a call is bitwise reproducible.
 * d a multiple of 16 in 16 .. 4096, n >= 1: anything else is CS_E_SHAPE before a launch */
int cs_fid_stats_accumulate(const float* feats, int64_t n, int d, double* sum, double* outer, void* stream);
/* mu = sum / N, sigma = (outer - N mu mu^T) / (N - 1); N < 2 is refused (CS_E_SHAPE) */
int cs_fid_stats_finalize(const double* sum, const double* outer, int64_t n_total, int d, double* mu, double* sigma, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CONSOLVER_HIP_H */
