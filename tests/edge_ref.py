"""CPU references for the per-op tests of the kernels at the edges of the SD1.5 denoiser, the VAE and the CLIP text encoder (csrc/misc.hip, gelu_erf in
vit_ops.hip, the VAE-only arms of norm.hip and igemm.hip): tests/test_edge_ref.py pins them on the CPU, tests/test_edge_ops_gpu.py compares the kernels with
them.  Test infrastructure, not a fallback.

As in tests/flux_ref.py every op has two forms over the SAME fp16-rounded inputs the kernel sees, both float64:

* ``*_fp64``      -- the plain operation: what the op is supposed to compute;
* ``*_emulated``  -- the same formula with the kernel's rounding points applied to exact arithmetic (``rnd``: float64 -> fp32 -> fp16).  The yardstick of the
  acceptance rule  max |out - fp64| <= 2 max |emulated - fp64| + 1 ulp_fp16 of the row's largest output,  not a second implementation to debug against.

Rounding points:
  sinusoid            [cos | sin](t f_k), f_k = exp(-ln(1e4) k / (C0 / 2)), stored fp16;
  time embedding      emb fp16 -> h1 = f16(silu(W1 emb + b1)) -> out = f16(silu(W2 h1 + b2)): three fp16 stores;
  rowvec_linear, conv_in, pixel_linear, pixel_affine, latent_to_nhwc64, row_softmax, quick_gelu, gelu_erf, LayerNorm
                      fp32 arithmetic, ONE rounding of the result; conv_in's lo plane is f16(acc - f16(acc));
  GroupNorm           the statistics are single-pass fp32 sums (sum, sum of squares) accumulated per thread over the rows of a split, then over the threads
                      that share a column, the two channels of a pair, and the (split, pair) items of a group; mean = a / n, var = q / n - mean^2;
                      gn_emulated() adds in that order in fp32 and rounds y = x sc + sh once.
Not carried: the order of the other fp32 sums, the last bits of v_exp_f32 / v_rcp_f32 / v_rsq_f32, fused multiply-adds.

The module also holds the case lists and the input generators of the GPU tests, so that tests/test_edge_ref.py can check on the CPU, on exactly those inputs,
that every emulator stays inside the bound its test states.
"""
import math

import torch

from tests.flux_ref import rnd as _rnd, ulp_at as _ulp_at

F16 = torch.float16
NAN = float("nan")
F16_MAX = 65504.0
F16_TINY = 2.0 ** -24                 # the smallest fp16 subnormal


def ulp_at(x):
    return _ulp_at(x, F16)


def rnd(x):
    """float64 -> fp32 -> fp16 -> float64: the one rounding of a kernel that computes in fp32"""
    return _rnd(x, F16)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def silu64(x):
    return x * torch.sigmoid(x)


def rule_bound(ref, emu, dim=-1):
    """the acceptance bound per row: 2 max |emu - ref| + 1 ulp of the row's largest |ref|"""
    return 2.0 * (emu - ref).abs().amax(dim) + ulp_at(ref.abs().amax(dim))


# ---- time embedding, rowvec_linear ----------------------------------------------------------------------------------------------------------------------------
T_VALUES = (0.0, 1.0, 500.5, 999.0)
TIME_DIMS = ((320, 1280), (32, 64))
TIME_BT = (1, 2, 5)
ROWVEC_K = (8, 320, 512, 520, 1280)
ROWVEC_N = (1, 3, 4, 5, 1282)
ROWVEC_R = (1, 3)


def timesteps(Bt):
    return torch.tensor([T_VALUES[i % len(T_VALUES)] for i in range(Bt)], dtype=torch.float32)


def sinusoid_fp64(t, C0):
    """[Bt][C0] = [cos | sin](t f_k), f_k = exp(-ln(1e4) k / half)"""
    half = C0 // 2
    a = t.double()[:, None] * torch.exp(-math.log(1e4) * torch.arange(half, dtype=torch.float64) / half)[None, :]
    return torch.cat((torch.cos(a), torch.sin(a)), -1)


def rowvec_linear_fp64(x, w, bias, silu):
    v = x.double() @ w.double().T + (bias.double() if bias is not None else 0.0)
    return silu64(v) if silu else v


def time_weights(C0, D, seed):
    g = gen(seed)
    w1 = (torch.randn(D, C0, generator=g) * C0 ** -0.5).to(F16)
    w2 = (torch.randn(D, D, generator=g) * D ** -0.5).to(F16)
    b1, b2 = (torch.randn(D, generator=g) * 0.5).to(F16), (torch.randn(D, generator=g) * 0.5).to(F16)
    return w1, b1, w2, b2


def time_embedding_fp64(t, C0, w1, b1, w2, b2):
    """(emb, h1, out) without any rounding in between"""
    emb = sinusoid_fp64(t, C0)
    h1 = rowvec_linear_fp64(emb, w1, b1, True)
    return emb, h1, rowvec_linear_fp64(h1, w2, b2, True)


def time_embedding_emulated(t, C0, w1, b1, w2, b2):
    emb = rnd(sinusoid_fp64(t, C0))
    h1 = rnd(rowvec_linear_fp64(emb, w1, b1, True))
    return emb, h1, rnd(rowvec_linear_fp64(h1, w2, b2, True))


def rowvec_inputs(K, N, R, seed):
    g = gen(seed)
    x = torch.randn(R, K, generator=g).to(F16)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(F16)
    bias = torch.randn(N, generator=g).to(F16)
    return x, w, bias


def rowvec_negative_inputs(K, N):
    """one row whose pre-activations are all about -30 (x = 1, w = -30 / K + noise): SiLU gives about -3e-12, which fp16 stores as -0"""
    g = gen(K + N)
    x = torch.ones(1, K).to(F16)
    w = (-30.0 / K + 0.01 * torch.randn(N, K, generator=g) * K ** -0.5).to(F16)
    return x, w, None


# ---- conv_in ----------------------------------------------------------------------------------------------------------------------------------------------------
CONV_IN_LAT = ((1, 1), (2, 2), (2, 4), (3, 6))              # (n_lat, B)
CONV_IN_HW = ((1, 1), (2, 3), (5, 7), (8, 8), (16, 24))
CONV_IN_COUT = (8, 128, 320)
CONV_IN_STRIDE_CASE = (5, 5, 512, 512, 8)                   # n_lat, B, H, W, Cout: B H W > 4096 * 256, the grid-stride loop runs twice


def conv_in_inputs(n_lat, B, H, W, Cout, seed, integer):
    """lat [B][4][H][W]: the first n_lat samples are the latents, the samples behind them hold OTHER data (a kernel that reads sample b instead of b % n_lat stays
    inside the buffer and is grossly wrong); every sample carries its own constant offset.  integer: every sum is an integer below 2048, exact in fp16."""
    g = gen(seed)
    off = torch.arange(1, B + 1, dtype=torch.float32)[:, None, None, None]
    if integer:
        lat = torch.randint(-2, 3, (B, 4, H, W), generator=g).float() + off
        w = torch.randint(-1, 2, (Cout, 4, 3, 3), generator=g).float()
        bias = torch.randint(-4, 5, (Cout,), generator=g).float()
    else:
        lat = torch.randn(B, 4, H, W, generator=g) + 0.5 * off
        w = torch.randn(Cout, 4, 3, 3, generator=g) / 6.0
        bias = torch.randn(Cout, generator=g) * 0.1
    return lat.to(F16), w.to(F16), bias.to(F16)


def conv_in_fp64(lat, n_lat, B, w, bias, dtype=torch.float64):
    """NHWC [B][H][W][Cout]: 3x3 pad 1 over latent b % n_lat, written as nine shifted products (not F.conv2d: tests/test_edge_ref.py compares the two)"""
    src = lat[:n_lat].to(dtype)[torch.arange(B) % n_lat]
    _, _, H, W = src.shape
    xp = torch.zeros(B, 4, H + 2, W + 2, dtype=dtype)
    xp[:, :, 1:-1, 1:-1] = src
    out = bias.to(dtype)[None, None, None, :].expand(B, H, W, -1).clone()
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("bchw,oc->bhwo", xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx].to(dtype))
    return out


def conv_in_emulated(ref):
    """(hi, lo): hi = f16(acc), lo = f16(acc - hi) of the fp32 accumulator"""
    acc = ref.float().double()
    hi = rnd(acc)
    return hi, rnd(acc - hi)


# ---- embed_tokens -------------------------------------------------------------------------------------------------------------------------------------------------
EMBED_L = (1, 7, 77)
EMBED_B = (1, 3)
EMBED_C = (8, 768)
EMBED_VOCAB = 50


def embed_inputs(L, B, C, seed):
    """ids [B L] with the out-of-range values -1, vocab, 2^40 and the two ends 0, vocab - 1 spread over the rows (as many as fit)"""
    g = gen(seed)
    rows = B * L
    ids = torch.randint(0, EMBED_VOCAB, (rows,), generator=g)
    edge = torch.tensor([-1, EMBED_VOCAB, 2 ** 40, 0, EMBED_VOCAB - 1])
    k = min(rows, 5)
    ids[torch.linspace(0, rows - 1, k).long()] = edge[:k]
    tok = torch.randn(EMBED_VOCAB, C, generator=g).to(F16)
    pos = torch.randn(L, C, generator=g).to(F16)
    return ids, tok, pos


def embed_tokens_ref(ids, tok, pos):
    """fp16, bit for bit: the sum of two fp16 values is exact in fp32, so there is one rounding"""
    rows, L = ids.numel(), pos.shape[0]
    return (tok[ids.clamp(0, tok.shape[0] - 1)].float() + pos[torch.arange(rows) % L].float()).to(F16)


# ---- quick_gelu, gelu_erf -----------------------------------------------------------------------------------------------------------------------------------------
GELU_N = (8, 2048, 2056)


def gelu_inputs(n):
    """a grid over [-12, 12] around the special values (+-0, +-65504, the smallest subnormal, +-6e-5), n elements"""
    special = torch.tensor([0.0, -0.0, F16_MAX, -F16_MAX, F16_TINY, 6e-5, -6e-5], dtype=torch.float64)
    if n <= 8:
        return torch.cat((special, torch.tensor([-1.5], dtype=torch.float64)))[:n].to(F16)
    return torch.cat((special, torch.linspace(-12, 12, n - len(special), dtype=torch.float64))).to(F16)


def quick_gelu_fp64(x):
    return x.double() * torch.sigmoid(1.702 * x.double())


def gelu_erf_fp64(x):
    return 0.5 * x.double() * (1.0 + torch.erf(x.double() / math.sqrt(2.0)))


def gelu_element_bound(x, ref):
    """per element: one ulp of the result (the rounding, and a rounding moved by fp32 noise) plus 2^-22 |x|: 0.5 x (1 + erf) and x / (1 + exp) multiply x by a factor
    in [0, 1] that fp32 carries to about 3 * 2^-24 ABSOLUTE (1 + erf cancels in the negative tail), i.e. 1.5 * 2^-24 |x|; 2^-22 |x| leaves room for the product"""
    return ulp_at(ref) + 2.0 ** -22 * x.double().abs()


# ---- row_softmax --------------------------------------------------------------------------------------------------------------------------------------------------
SOFTMAX_REG_COLS = (8, 64, 504, 512, 520, 4096, 8192)
SOFTMAX_REG_ROWS = (1, 3, 4, 5)
SOFTMAX_BLOCK_COLS = (8200, 16384, 65536)
SOFTMAX_BLOCK_ROWS = (1, 2)
SOFTMAX_SCALES = (1.0, 512 ** -0.5)
SOFTMAX_KINDS = ("gaussian", "constant", "peak_first", "peak_last", "peak_mid", "extremes")


def softmax_rows(rows, cols, scale, kind, seed):
    """[rows][cols] fp16 logits of one kind.  gaussian: scaled logits N(0, 2^2); constant: 1.5; peak_*: one element 30 above the rest AFTER scaling, at column 0,
    cols - 1, or column 515 (the last one when the row is shorter); extremes: +65504 and -65504 among gaussians."""
    g = gen(seed)
    x = torch.randn(rows, cols, generator=g) * ((2.0 if kind == "gaussian" else 1.0) / scale)
    if kind == "constant":
        x[:] = 1.5
    elif kind.startswith("peak"):
        x = x * 0.1
        col = {"peak_first": 0, "peak_last": cols - 1, "peak_mid": min(cols - 1, 515)}[kind]
        x[:, col] = x.amax(-1) + 30.0 / scale
    elif kind == "extremes":
        x[:, cols // 3] = F16_MAX
        x[:, cols - 1 - cols // 5] = -F16_MAX
    return x.clamp(-F16_MAX, F16_MAX).to(F16)


def row_softmax_fp64(x, scale):
    return torch.softmax(x.double() * f32(scale), -1)


def softmax_sum_bound(ref):
    """|sum of the fp16 outputs - 1| per row: every output is the rounding of p_i (1 + d) with |d| <= 2^-15 common to the row (at most 256 + 10 fp32 adds per lane and
    across lanes, 2.7e-5 with the exponential's own error): sum_i ulp(p_i) / 2 + 2^-15.  Never more than the cols * ulp(max) / 2 of a plain count."""
    return 0.5 * ulp_at(ref).sum(-1) + 2.0 ** -15


# ---- latent_to_nhwc64, pixel_linear, pixel_affine -----------------------------------------------------------------------------------------------------------------
PIXEL_HW = (1, 255, 256, 257)
LATENT_C = (3, 4, 16, 64)
LATENT_B = (1, 2)
PIXEL_LINEAR_C = (4, 16)
SD_SCALE = 1.0 / 0.18215
# pixel_affine: (acc - shift) * scale against acc * scale - shift differ by shift (scale - 1) = 0.75: hundreds of ulps of the O(1) results
AFFINE_SHIFT, AFFINE_SCALE = 1.5, 0.5
AFFINE_FORMS = (("identity", 8, 4), ("identity", 32, 16), ("w", 8, 4))


def pixel_inputs(B, Cin, HW, Cout, seed):
    g = gen(seed)
    x = torch.randn(B, Cin, HW, generator=g).to(F16)
    w = (torch.randn(Cout, Cin, generator=g) * Cin ** -0.5).to(F16)
    b = (torch.randn(Cout, generator=g) * 0.3).to(F16)
    return x, w, b


def f32(v):
    """a Python float as the kernel receives it"""
    return float(torch.tensor(v, dtype=torch.float32))


def latent_fp64(x, w, b, in_scale, in_shift):
    """NHWC [B][HW][C]: z = x scale + shift, then w z + b"""
    z = x.double().transpose(1, 2) * f32(in_scale) + f32(in_shift)
    return z @ w.double().T + b.double() if w is not None else z


def pixel_linear_fp64(x, w, b, in_scale, in_shift):
    """NCHW [B][C][HW]"""
    return latent_fp64(x, w, b, in_scale, in_shift).transpose(1, 2)


def pixel_affine_fp64(x, Cout, w, b, out_scale, out_shift):
    acc = torch.einsum("oc,bcp->bop", w.double(), x.double()) + b.double()[None, :, None] if w is not None else x.double()[:, :Cout]
    return (acc - f32(out_shift)) * f32(out_scale)


# ---- conv_down ----------------------------------------------------------------------------------------------------------------------------------------------------
CONV_DOWN_CASES = ((2, 16, 16, 64, 128), (1, 8, 24, 128, 256), (3, 4, 4, 64, 160), (1, 32, 32, 128, 128), (5, 6, 10, 64, 128))     # B, H, W, Cin, N


def conv_down_inputs(B, H, W, Cin, N, seed, integer):
    """NHWC x, w [N][Cin][3][3], bias.  integer: ternary data thinned so that the sums (9 Cin terms) stay far inside fp16's exact integers"""
    g = gen(seed)
    if integer:
        keep = (100.0 / (9 * Cin)) ** 0.5
        tern = lambda *s: (torch.randint(-1, 2, s, generator=g) * (torch.rand(s, generator=g) < keep)).float()
        return tern(B, H, W, Cin).to(F16), tern(N, Cin, 3, 3).to(F16), torch.randint(-4, 5, (N,), generator=g).float().to(F16)
    x = torch.randn(B, H, W, Cin, generator=g).to(F16)
    w = (torch.randn(N, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).to(F16)
    return x, w, (torch.randn(N, generator=g) * 0.1).to(F16)


def conv_down_fp64(x, w, bias, pad_lo=0, dtype=torch.float64):
    """NHWC [B][H / 2][W / 2][N]: out(y, x) = sum over taps of in(2 y + ky - pad_lo, 2 x + kx - pad_lo), zero outside the image.  pad_lo = 0 is the encoder's
    (0, 1, 0, 1) pad, pad_lo = 1 the symmetric one."""
    B, H, W, Cin = x.shape
    Ho, Wo = H // 2, W // 2
    xp = torch.zeros(B, H + 2, W + 2, Cin, dtype=dtype)
    xp[:, pad_lo:pad_lo + H, pad_lo:pad_lo + W] = x.to(dtype)
    out = bias.to(dtype)[None, None, None, :].expand(B, Ho, Wo, -1).clone()
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] @ w[:, :, ky, kx].to(dtype).T
    return out


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------------------------------
GN_SPLIT_C = (128, 256, 512)
GN_SPLIT_HW = (9, 64, 576, 1600, 4096)
GN_SPLIT_B = (1, 3)
GN_TABLE_C = ((2688, 0), (2048, 640))
GN_TABLE_HW = (4, 16, 100)


def gn_inputs(B, HW, c0, c1, seed, dc=False):
    """x0, x1, gamma, beta.  dc: every group has its own mean of about +-10 over a deviation of 0.5 (20 sigma)"""
    g = gen(seed)
    C = c0 + c1
    x = torch.randn(B, HW, C, generator=g) * 2 + 0.5
    if dc:
        cpg = C // 32
        mean = (10.0 + torch.randn(B, 1, 32, generator=g)) * (torch.randint(0, 2, (B, 1, 32), generator=g) * 2 - 1)
        x = 0.5 * torch.randn(B, HW, C, generator=g) + mean.repeat_interleave(cpg, -1)
    x = x.to(F16)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(F16), (0.1 * torch.randn(C, generator=g)).to(F16)
    return x[..., :c0].contiguous(), (x[..., c0:].contiguous() if c1 else None), gamma, beta


def group_norm_fp64(x, groups, gamma, beta, eps, silu):
    """x [B][HW][C] (the concatenation)"""
    B, HW, C = x.shape
    xg = x.double().reshape(B, HW, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xg - mean) * torch.rsqrt(var + eps)).reshape(B, HW, C) * gamma.double() + beta.double()
    return silu64(y) if silu else y


def gn_splits(HW, smax):
    S = smax
    while S > 1 and HW % S:
        S >>= 1
    return S


def _wave_sum32(v):
    """v [..., 64] fp32: the xor butterfly (32, 16, ..., 1)"""
    n = 64
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def gn_stats_emulated(x, S):
    """partial [B][S][C / 2][2] fp32 of x [B][HW][C]: a thread (column of 8 channels, row slot rr of R = 256 / (C / 8)) adds its rows r = rr, rr + R, ... of the split
    in fp32, the R slots of a column are added in order, then the two channels of a pair"""
    B, HW, C = x.shape
    CV = C // 8
    R = max(1, 256 // CV)
    rows = HW // S
    xs = x.float().reshape(B, S, rows, C)
    its = (rows + R - 1) // R
    pad = torch.zeros(B, S, its * R - rows, C)
    xs = torch.cat((xs, pad), 2).reshape(B, S, its, R, C)
    s1 = torch.zeros(B, S, R, C)
    s2 = torch.zeros(B, S, R, C)
    for i in range(its):
        s1 = s1 + xs[:, :, i]
        s2 = s2 + xs[:, :, i] * xs[:, :, i]
    a, q = s1[:, :, 0], s2[:, :, 0]
    for j in range(1, R):
        a, q = a + s1[:, :, j], q + s2[:, :, j]
    return torch.stack((a[..., 0::2] + a[..., 1::2], q[..., 0::2] + q[..., 1::2]), -1)


def gn_finalize_emulated(p0, c0, p1, c1, groups, HW, eps):
    """(mean, rstd) fp32 [B][groups]: thread tid of 256 adds the (split, pair) items tid, tid + 256, ... of the group, the wave butterfly, the four waves in order"""
    B, S0 = p0.shape[:2]
    S1 = p1.shape[1] if p1 is not None else 0
    Smax = max(S0, S1)
    Ctot = c0 + c1
    cpg = Ctot // groups
    ppg, q0 = cpg // 2, c0 // 2
    mean, rstd = torch.zeros(B, groups), torch.zeros(B, groups)
    for g in range(groups):
        n_items = Smax * ppg
        items = torch.zeros(B, (n_items + 255) // 256 * 256, 2)
        for j in range(ppg):
            pr = g * ppg + j
            if pr < q0:
                items[:, j:S0 * ppg:ppg] = p0[:, :, pr]
            elif S1:
                items[:, j:S1 * ppg:ppg] = p1[:, :, pr - q0]
        items = items.reshape(B, -1, 256, 2)
        acc = torch.zeros(B, 256, 2)
        for i in range(items.shape[1]):
            acc = acc + items[:, i]
        w = _wave_sum32(acc.reshape(B, 4, 64, 2).transpose(-1, -2))                    # [B][4 waves][2]
        tot = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        n = torch.tensor(float(cpg) * float(HW), dtype=torch.float32)
        m = tot[:, 0] / n
        mean[:, g] = m
        rstd[:, g] = torch.rsqrt((tot[:, 1] / n - m * m).clamp_min(0.0) + torch.tensor(eps, dtype=torch.float32))
    return mean, rstd


def gn_emulated(x0, x1, groups, gamma, beta, eps, silu, smax):
    """the kernel's statistics (fp32, split order) and one rounding of y"""
    B, HW, c0 = x0.shape
    c1 = x1.shape[-1] if x1 is not None else 0
    S = gn_splits(HW, smax)
    p0 = gn_stats_emulated(x0, S)
    p1 = gn_stats_emulated(x1, S) if c1 else None
    mean, rstd = gn_finalize_emulated(p0, c0, p1, c1, groups, HW, eps)
    cpg = (c0 + c1) // groups
    sc = gamma.float()[None, :] * rstd.repeat_interleave(cpg, -1)
    sh = beta.float()[None, :] - mean.repeat_interleave(cpg, -1) * sc
    x = torch.cat((x0, x1), -1) if c1 else x0
    y = x.double() * sc.double()[:, None, :] + sh.double()[:, None, :]
    return rnd(silu64(y) if silu else y)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------------------------------
LN_C = (8, 520, 1288, 1544, 2048)
LN_M = (1, 3, 4, 5, 15, 16, 17)


def ln_inputs(M, C, seed):
    g = gen(seed)
    x = (torch.randn(M, C, generator=g) * 3 + 1).to(F16)
    return x, (1 + 0.2 * torch.randn(C, generator=g)).to(F16), (0.1 * torch.randn(C, generator=g)).to(F16)


def layer_norm_fp64(x, gamma, beta, eps=1e-5):
    xs = x.double()
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    return (xs - mean) * torch.rsqrt(var + eps) * gamma.double() + beta.double()
