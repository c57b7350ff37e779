"""CPU references for the attention op tests (tests/test_attention_ref.py, tests/test_attention_forms_gpu.py): test infrastructure, not a fallback.

Both functions take the SAME rounded inputs the kernel sees -- q [B, Nq, H*dh], k / v [B, Nk, H*dh] of dtype T (float16 or bfloat16), heads interleaved
per row as in the C ABI -- and return float64 [B, Nq, H*dh].

* ``attention_fp64``     -- plain softmax(scale Q K^T + bias + mask) V in float64: what the op is supposed to compute.
* ``attention_emulated`` -- the same math with the rounding points of attn_kernel (consolver_amd/csrc/attention.hip).  It is the YARDSTICK for the
  tolerances of the GPU tests (how far from fp64 an implementation with these roundings lands), not a second implementation to debug against:
    1. Q (scale log2 e) is rounded to T: the product is taken in fp32 with c = float(scale) * 1.4426950408889634f (launch_attention, `p.c = ...`) and packed
       back to T when the Q fragments are built ("fold scale*log2(e) into Q", `v[e] = ok ? pack2<T>(tof(..) * p.c, ..)`);
    2. scores S = Q' K^T (+ bias log2 e, fp32) are fp32 MFMA accumulators;
    3. P = exp2(S - rowmax) is rounded to T when the fragments of the second product are packed (`f[0] = pack2<T>(s[2 * t2][t][0], ...)`);
    4. the denominator.  Head dim 40 (ONES: a column of ones in the padded V tile, also attn40_lw_kernel) takes it from the P V MFMA itself, i.e. it is
       the sum of the ROUNDED P (`l = __shfl(o_acc[DH / 16][t][...])` in the epilogue).  Every other form keeps l_run, which adds the fp32 exponentials
       BEFORE they are packed (`const float e = __builtin_amdgcn_exp2f(s[kt][t][r]); ... if (!ONES) ps += e;` then `l_run[t] += ps`, in front of the pack2
       lines): the sum of the UNROUNDED P.  ``denominator`` selects which; by default it follows the head dim as the kernel does;
    5. P V is accumulated in fp32;
    6. O / l is rounded to T once (`pack2<T>(o_acc[a][t][0] * inv, ...)` in the epilogue).
  Not carried: the order of the fp32 sums, v_exp_f32's last bit, and the kernel's reference maximum (it trails the true row maximum by up to 2^8, or is the
  first tile's on the fast paths of head dims 40 / 128) -- a power-of-two-like shift of P that moves no rounding point except where P leaves T's normal range.
"""
import math

import torch

LOG2E = 1.4426950408889634


def bias_for_abi(bias):
    """natural-log bias [H, N, N] -> the fp32 tensor of bias * log2(e) that cs_op_attention_bias takes"""
    return (bias.double() * LOG2E).float().contiguous()


def _split(q, k, v, H):
    B, Nq, C = q.shape
    Nk = k.shape[1]
    dh = C // H
    return (q.reshape(B, Nq, H, dh).transpose(1, 2), k.reshape(B, Nk, H, dh).transpose(1, 2), v.reshape(B, Nk, H, dh).transpose(1, 2))


def _masked(s2, causal):
    if causal:
        Nq, Nk = s2.shape[-2:]
        s2 = s2.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool).triu(1), float("-inf"))
    return s2


def scores_log2(q, k, H, scale, causal=False, bias=None):
    """float64 [B, H, Nq, Nk]: log2(e) (scale q.k + bias) + mask, from the exact values of the inputs (and of the fp32 ABI bias)"""
    qh, kh, _ = _split(q, k, k, H)
    s2 = (qh.double() @ kh.double().transpose(-1, -2)) * (float(scale) * LOG2E)
    if bias is not None:
        s2 = s2 + bias_for_abi(bias).double()
    return _masked(s2, causal)


def attention_fp64(q, k, v, H, scale, causal=False, bias=None):
    _, _, vh = _split(q, k, v, H)
    s2 = scores_log2(q, k, H, scale, causal, bias)
    p = torch.exp2(s2 - s2.amax(-1, keepdim=True))
    o = (p @ vh.double()) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(q.shape)


def attention_emulated(q, k, v, H, scale, causal=False, bias=None, dtype=None, denominator=None):
    dtype = dtype or q.dtype
    assert q.dtype == k.dtype == v.dtype == dtype and dtype in (torch.float16, torch.bfloat16)
    qh, kh, vh = _split(q, k, v, H)
    if denominator is None:
        denominator = "rounded" if qh.shape[-1] == 40 else "unrounded"
    c = torch.tensor(float(scale), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qs = (qh.float() * c).to(dtype)                                                     # 1
    s = (qs.double() @ kh.double().transpose(-1, -2)).float()                           # 2 (products of T values are exact; one rounding of the sum)
    if bias is not None:
        s = s + bias_for_abi(bias)
    s = _masked(s, causal)
    p32 = torch.exp2(s - s.amax(-1, keepdim=True))
    p = p32.to(dtype)                                                                   # 3
    l = (p if denominator == "rounded" else p32).double().sum(-1, keepdim=True)         # 4
    o = (p.double() @ vh.double()).float()                                              # 5
    o = (o * (1.0 / l.float())).to(dtype)                                               # 6
    return o.double().transpose(1, 2).reshape(q.shape)


def err_rows(out, ref, H):
    """per-row, per-head relative L2 of out against ref: [B, Nq, H] float64"""
    B, N, C = ref.shape
    o, r = out.double().reshape(B, N, H, C // H), ref.double().reshape(B, N, H, C // H)
    return (o - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-300)


def rel_l2(out, ref):
    return float((out.double() - ref.double()).norm() / ref.double().norm())


def ulp(dtype):
    """one ulp of T, relative (the spacing at 1.0)"""
    return 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7


# ---- input families shared by the CPU yardstick test and the GPU tests ------------------------------------------------------------------------------
def gaussian(B, H, Nq, Nk, dh, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, n, H * dh, generator=g).to(dtype) for n in (Nq, Nk, Nk))


def bias_tensor(H, N, seed, last4=6.0):
    """T5-like bias in natural-log units: N(0, 2^2), plus `last4` on the last four keys of every row (the keys the kernel's four-wide guard decides on)"""
    g = torch.Generator().manual_seed(seed)
    b = 2.0 * torch.randn(H, N, N, generator=g)
    b[:, :, max(N - 4, 0):] += last4
    return b


def plant_dominant_last_key(q, k, v, H, scale, bias=None):
    """In place: q[..., head column 0] = 2, key Nk-1 = (a, 0, 0, ...) with a such that it carries softmax weight >= 0.2 in EVERY row (checked), and a
    distinct pattern in v[:, Nk-1].  Returns the smallest weight of the last key over all rows."""
    B, Nq, C = q.shape
    Nk, dh = k.shape[1], C // H
    q.view(B, Nq, H, dh)[..., 0] = 2
    kv, vv = k.view(B, Nk, H, dh), v.view(B, Nk, H, dh)
    kv[:, Nk - 1] = 0
    vv[:, Nk - 1] = (4.0 * (-1.0) ** torch.arange(dh) + 0.25 * torch.arange(H)[:, None]).to(v.dtype)
    if Nk == 1:
        return 1.0
    s2 = scores_log2(q, k, H, scale, False, bias)                 # the last key's q.k part is 0 here, its bias part already in
    rest = torch.logsumexp(s2[..., :-1] / LOG2E, -1)               # natural log of the other keys' mass, [B, H, Nq]
    need = (rest - s2[..., -1] / LOG2E).amax()                    # q.k score (natural units) that gives weight 1/2 in the hardest row ...
    a = math.ceil(max(float(need), 0.0) / (2.0 * scale) * 8) / 8   # ... from scale * 2 * a; a multiple of 1/8 (exact in both dtypes below 32, at most 1/4 % off above)
    kv[:, Nk - 1, :, 0] = a
    s2 = scores_log2(q, k, H, scale, False, bias)
    w = torch.softmax(s2 / LOG2E, -1)[..., -1]
    assert float(w.min()) >= 0.2, float(w.min())
    return float(w.min())


def plant_dominant_diagonal(q, k, H, stride=3, beta=1.25):
    """In place, for the causal form: key i = beta q_i for every stride-th row i (and the last), so that key i carries most of query i's weight while
    the rows between have no dominant key.  Returns the planted rows."""
    N = q.shape[1]
    rows = sorted(set(range(0, N, stride)) | {N - 1})
    k[:, rows] = (beta * q[:, rows].float()).to(k.dtype)
    return rows


def add_tile_ramp(k, H, col, step_log2, scale, q_col_value=2.0, first_tile=0, max_steps=None):
    """In place: k[:, j, head column col] += t(j) with t chosen so that a query whose column `col` is q_col_value sees its scores move by step_log2
    (log2 units) from each 64-key tile to the next, starting behind tile `first_tile` and for at most `max_steps` tiles; step < 0 falls."""
    B, Nk, C = k.shape
    dh = C // H
    tile = (torch.arange(Nk) // 64 - first_tile).clamp(0, max_steps).double()
    t = tile * step_log2 / (q_col_value * float(scale) * LOG2E)
    kv = k.view(B, Nk, H, dh)
    kv[..., col] = (kv[..., col].double() + t[None, :, None]).to(k.dtype)


# ---- one builder for every case family: inputs, fp64 reference and the emulator's own error, computed once per case and shared -------------------------
class Case:
    __slots__ = ("q", "k", "v", "bias", "H", "dh", "scale", "causal", "ref", "emu_rows", "emu_max", "rows")


_CASES = {}


def make_case(kind, dh, dtype, B, H, Nq, Nk, family, seed=0):
    """kind: "plain" | "causal" | "bias" (Nq == Nk for the last two).  family:
      "gauss"     unit-Gaussian q, k, v;
      "edge"      dominant last key (causal: dominant diagonal keys on every third row), bias with +6 on the last four keys;
      "rise" / "fall"   the row maximum moves by 20 log2 units (biased form, whose bias adds noise of its own: 32; at least 12 after the noise of the tile maxima) from each 64-key tile to the next, for every query;
      "one"       ... for ONE query only (row Nq // 2 + 5), along a head column every other query has zero in;
      "moderate"  one step of 10 log2 units behind the second tile (below the fp16 range of P: the fast paths of head dims 40 / 128 stay on);
      "neg_tile0" (bias) -1e4 on the whole first key tile;
      "outlier"   key 200 (or Nk - 3) = 6 x query 5: 2^16 above the first tile's maximum for that query only.
    The result is cached: tests that run the same inputs through several kernels share one reference, and nothing may write to it."""
    key = (kind, dh, dtype, B, H, Nq, Nk, family, seed)
    if key in _CASES:
        return _CASES[key]
    c = Case()
    c.H, c.dh, c.scale, c.causal, c.rows = H, dh, dh ** -0.5, kind == "causal", ()
    assert kind == "plain" or Nq == Nk
    q, k, v = gaussian(B, H, Nq, Nk, dh, dtype, 1000 * seed + 7 * Nq + Nk + dh)
    c.bias = bias_tensor(H, Nq, seed + Nq) if kind == "bias" else None
    if family == "edge":
        if kind == "causal":
            c.rows = tuple(plant_dominant_diagonal(q, k, H))
        else:
            plant_dominant_last_key(q, k, v, H, c.scale, c.bias)
    elif family in ("rise", "fall", "moderate"):
        q.view(B, Nq, H, dh)[..., 0] = 2
        if family == "moderate":
            add_tile_ramp(k, H, 0, 10.0, c.scale, first_tile=1, max_steps=1)
        else:
            add_tile_ramp(k, H, 0, (32.0 if kind == "bias" else 20.0) * (1 if family == "rise" else -1), c.scale)
    elif family == "one":
        r = Nq // 2 + 5
        q.view(B, Nq, H, dh)[..., 1] = 0
        q.view(B, Nq, H, dh)[:, r, :, 1] = 2
        k.view(B, Nk, H, dh)[..., 1] = 0
        add_tile_ramp(k, H, 1, 20.0, c.scale)
        c.rows = (r,)
    elif family == "neg_tile0":
        c.bias[:, :, :64] = -1e4
    elif family == "outlier":
        pos = 200 if Nk > 200 else Nk - 3
        k[:, pos] = (6.0 * q[:, 5].float()).to(dtype)
        c.rows = (5, pos)
    else:
        assert family == "gauss", family
    c.q, c.k, c.v = q, k, v
    c.ref = attention_fp64(q, k, v, H, c.scale, c.causal, c.bias)
    c.emu_rows = err_rows(attention_emulated(q, k, v, H, c.scale, c.causal, c.bias, dtype), c.ref, H)
    c.emu_max = float(c.emu_rows.max())
    _CASES[key] = c
    return c


# the forms of attn_kernel / attn40_lw_kernel the tests walk: name -> (kind, head dim, dtype, ROWS = query rows per workgroup, knobs)
F16, BF16 = torch.float16, torch.bfloat16
FORMS = {
    "dh40": ("plain", 40, F16, 256, {"attn_lw": 0}),
    "dh40_qt2": ("plain", 40, F16, 128, {"attn_lw": 0, "attn_qt40": 2}),
    "dh64": ("plain", 64, F16, 128, {}),
    "dh64_causal": ("causal", 64, F16, 128, {}),
    "dh64_bias_f16": ("bias", 64, F16, 128, {}),
    "dh64_bias_bf16": ("bias", 64, BF16, 128, {}),
    "dh80": ("plain", 80, F16, 128, {}),
    "dh160": ("plain", 160, F16, 64, {}),
    "dh128_f16": ("plain", 128, F16, 128, {}),
    "dh128_bf16": ("plain", 128, BF16, 128, {}),
}
LW_FORMS = {"dh40_lw1": ("plain", 40, F16, 256, {"attn_lw": 1}), "dh40_lw2": ("plain", 40, F16, 256, {"attn_lw": 2})}


def whole_tensor_bound(dh, dtype):
    """the project's whole-tensor relative L2 bounds (test_attention: 2e-3; the FLUX head dim 128 tests: 3e-3 for f16, 2e-2 for bf16)"""
    return 2e-2 if dtype == BF16 else (3e-3 if dh == 128 else 2e-3)


def rescale_shape(kind, rows):
    """(Nq, Nk) of the rescale-path cases: one query block and one row, four full key tiles and a ragged fifth (the biased form needs N % 4 == 0)"""
    return (261, 261) if kind == "causal" else (260, 260) if kind == "bias" else (rows + 1, 4 * 64 + 5)


def rescale_families(kind, dh):
    fam = ["rise", "fall", "one"]
    if dh in (40, 128):
        fam.append("moderate")
    if kind == "bias":
        fam.append("neg_tile0")
    return fam
