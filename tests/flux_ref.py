"""CPU references for the FLUX DiT op tests (tests/test_flux_ref.py, tests/test_flux_gemm2_forms_gpu.py, tests/test_flux_glue_ops_gpu.py): test infrastructure,
not a fallback.

Every reference takes the SAME rounded inputs the kernel sees and returns float64.  Each op has two forms:

* ``*_fp64``      -- the plain operation in float64: what the op is supposed to compute;
* ``*_emulated``  -- the same math with the kernel's rounding points applied (``rnd``: float64 -> fp32 -> T, the path a value takes in the kernel).  The YARDSTICK
  for the tolerances (how far from float64 an implementation with these roundings lands), not a second implementation to debug against.

Rounding points (file: consolver_amd/csrc/gemm2.hip, flux_ops.hip):
  gemm2, plain epilogue   v = sum_k a w + bias in fp32 (the accumulators start from the bias); b = T(act(v)); out = T(res + gate * b) with the multiply and the add in
                          fp32 (without gate and residual out = b, no second rounding);
  gemm2, split epilogue   v stays fp32; f = (res + res_lo) + gate * v in fp32; hi = T(f); lo = T(f - hi).  The split-K tail reduce adds res and res_lo one after the
                          other to gate * v instead of adding their sum: another fp32 order, same rounding points;
  qk_norm_rope            T(x * rsqrt(mean x^2 + eps)), times weight, rounded to T, rotated with the fp32 cos / sin, rounded to T;
  ln_modulate             one rounding of (x - mean) rstd (1 + scale) + shift; y_lo = T(o - y);
  small_linear            fp32 throughout (weights T), SiLU by the fast exponential.
Not carried: the order of the fp32 sums, the last bits of v_exp_f32 / v_rcp_f32 / v_rsq_f32.

GELU (act = 1) in the kernel is x * rcp(1 + exp2(x (c1 + c2 x^2))), c1 = -2 log2(e) sqrt(2/pi), c2 = 0.044715 c1, which is x sigmoid(2u) = 0.5 x (1 + tanh u),
u = sqrt(2/pi) (x + 0.044715 x^3), in exact arithmetic.  Two figures bound what the fast form and an error dv of its argument add (both derived, nothing measured):
  derivative   d/dx [x s(2u)] = s + x s (1 - s) 2u', s = sigmoid(2u).  The tanh form's derivative has its maximum 1.1290 near x = 1.45 and its minimum -0.1290 near
               x = -1.45 (tests/test_flux_ref.py walks a grid); GELU_DERIV_MAX = 1.13 bounds |gelu(v + dv) - gelu(v)| <= 1.13 |dv|.
  fast form    the exponent arg = x (c1 + c2 x^2) takes four fp32 roundings (x^2, c2 t, c1 + ., x * .) on top of the two rounded constants: |d arg| <= 6 * 2^-24 |arg|,
               so exp2 is off by a factor 1 + |arg| ln2 6 2^-24, plus 1 ulp (2^-23) of v_exp_f32.  y = x / (1 + e) moves by e / (1 + e) of e's relative error, then
               1 + e rounds (2^-24), v_rcp_f32 has 1 ulp (2^-23) and the product rounds (2^-24):
                   |dy| <= |y| ( e / (1 + e) (|arg| ln2 6 2^-24 + 2^-23) + 2^-22 )   (+ 1e-37 where e over- or underflows fp32: y is 0 or x there).
"""
import functools
import math

import torch

F16, BF16 = torch.float16, torch.bfloat16
DTYPES = {"bf16": BF16, "f16": F16}
NAN = float("nan")
GUARD = 8                          # NaN rows behind every output buffer

# the FLUX block shapes, shrunk: segments end inside 64-row wave strips and inside 256-row tiles
D, B, T, I1, I2 = 256, 2, 40, 136, 72
I = I1 + I2                        # 208 image tokens (two embedders)
S = T + I                          # 248 joint tokens


def mant(dtype):
    return 10 if dtype == F16 else 7


def ulp(dtype):
    """one ulp of T, relative (the spacing at 1.0)"""
    return 2.0 ** -mant(dtype)


def ulp_at(x, dtype):
    """the spacing of T at |x| (float64 tensor), subnormal spacing at and near zero"""
    x = torch.as_tensor(x, dtype=torch.float64).abs()
    emin = -14 if dtype == F16 else -126
    _, e = torch.frexp(x)                                              # x = m 2^e, 0.5 <= m < 1
    e = torch.where(x == 0, torch.full_like(e, emin), (e - 1).clamp_min(emin))
    return torch.ldexp(torch.ones_like(x), e - mant(dtype))


def rnd(x, dtype):
    """float64 -> fp32 -> T -> float64: one rounding point of a kernel that computes in fp32"""
    return x.float().to(dtype).double()


def exact_limit(dtype):
    """integers up to here are exact in T (the exact family keeps the reference and the branch value inside)"""
    return 256.0 if dtype == BF16 else 2048.0


# ---- row map ------------------------------------------------------------------------------------------------------------------------------------------------
def rowmap(r, seg, stride, off):
    """rowmap() of gemm2.hip on a tensor of rows: (r / seg) * stride + r % seg + off, or r + off when seg == 0"""
    r = torch.as_tensor(r, dtype=torch.long)
    return torch.div(r, seg, rounding_mode="floor") * stride + r % seg + off if seg else r + off


def rowmap_loop(M, seg, stride, off):
    """the same as a plain loop over segments"""
    out = []
    if not seg:
        return [m + off for m in range(M)]
    s = 0
    while len(out) < M:
        out += [s * stride + off + j for j in range(min(seg, M - len(out)))]
        s += 1
    return out


# ---- gemm2 --------------------------------------------------------------------------------------------------------------------------------------------------
GELU_DERIV_MAX = 1.13
_C0 = math.sqrt(2.0 / math.pi)


def gelu_fp64(x):
    return x * torch.sigmoid(2.0 * _C0 * (x + 0.044715 * x ** 3))


def gelu_fast_err(x):
    """bound of |kernel gelu_tanh(x) - gelu_fp64(x)| for an fp32 x (module docstring)"""
    arg = -2.0 * math.log2(math.e) * _C0 * (x + 0.044715 * x ** 3)
    e = torch.exp2(arg.clamp(-1000, 1000))
    y = x / (1.0 + e)
    return y.abs() * (e / (1.0 + e) * (arg.abs() * math.log(2.0) * 6 * 2.0 ** -24 + 2.0 ** -23) + 2.0 ** -22) + 1e-37


class G2:
    """one gemm2 problem over named CPU buffers (2-D tensors [rows][ld]); maps are (seg_rows, seg_stride, row_off)"""
    def __init__(self, a, M, K, N, w, out, bias=None, lda=0, a_map=(0, 0, 0), ldc=0, col_off=0, c_map=(0, 0, 0), res=None, res_lo=None, out_lo=None,
                 gate=None, gate_off=0, rps=0, act=0):
        self.__dict__.update(locals())
        del self.__dict__["self"]


class G2Values:
    pass


def g2_values(bufs, p, dtype, exact=False, rows=None):
    """float64 reference, emulation and bounds of problem p on logical rows `rows` (default all).  exact: fp32 matmul (every sum of the exact family is an integer
    below 2^24, so it is exact and a lot faster than float64)."""
    o = G2Values()
    m = torch.arange(p.M) if rows is None else torch.as_tensor(rows, dtype=torch.long)
    mm = torch.float32 if exact else torch.float64
    A = bufs[p.a][rowmap(m, *p.a_map), :p.K].to(mm)
    W = bufs[p.w][:p.N].to(mm)
    bias = bufs[p.bias].double() if p.bias else torch.zeros(p.N, dtype=torch.float64)
    v = (A @ W.T).double() + bias
    o.S = (A.abs() @ W.abs().T).double() + bias.abs()
    o.m, o.crow, o.cols = m, rowmap(m, *p.c_map), slice(p.col_off, p.col_off + p.N)
    take = lambda name: bufs[name][o.crow, o.cols].double()
    res = take(p.res) if p.res else None
    res_lo = take(p.res_lo) if p.res_lo else None
    gate = bufs[p.gate][torch.div(m, p.rps, rounding_mode="floor"), p.gate_off:p.gate_off + p.N].double() if p.gate else None
    gabs = gate.abs() if gate is not None else 1.0
    one = lambda t: t if t is not None else 0.0
    o.v = v
    o.branch = gelu_fp64(v) if p.act else v
    o.ref = (one(res) + one(res_lo)) + (gate * o.branch if gate is not None else o.branch)
    v32 = v.float().double()
    g = (p.K + 2) * 2.0 ** -23
    if p.out_lo:                                                           # split epilogue
        f = (res + res_lo) + (gate * v32 if gate is not None else v32)
        o.emu_branch = v32
        o.emu = rnd(f, dtype)
        o.emu_lo = rnd(f - o.emu, dtype)
        # hi + lo against float64: the branch's accumulation, three fp32 roundings (res + res_lo, gate * v, the sum) and the rounding of lo (|lo| <= ulp_T(f))
        o.bound_sum = gabs * g * o.S + 2.0 ** -22 * (res.abs() + res_lo.abs() + gabs * v.abs()) + ulp_at(ulp_at(o.ref, dtype), dtype)
    else:
        o.emu_branch = rnd(gelu_fp64(v32) if p.act else v32, dtype)
        o.emu = o.emu_branch if gate is None and res is None else rnd(one(res) + (gate * o.emu_branch if gate is not None else o.emu_branch), dtype)
        o.emu_lo = None
    berr = g * o.S
    if p.act:
        berr = GELU_DERIV_MAX * berr + gelu_fast_err(v32)
    o.bound = gabs * (berr + ulp_at(o.emu_branch, dtype)) + ulp_at(o.emu, dtype)
    return o


# ---- input families -----------------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def density_for(K):
    """P(nonzero) of the exact family's x and w: the branch value is a sum of K terms of {-1, 0, 1} with variance K density^2 <= 100 (sigma 10), so that it stays
    far inside the exact range over millions of elements"""
    return min(2.0 / 3.0, math.sqrt(100.0 / K))


class Family:
    """tensors of one family (exact | random), dtype T, drawn from one generator"""
    def __init__(self, family, dtype, seed):
        self.family, self.dtype, self.g = family, dtype, _gen(seed)

    @property
    def exact(self):
        return self.family == "exact"

    def _tern(self, shape, density):
        return (torch.randint(-1, 2, shape, generator=self.g) * (torch.rand(shape, generator=self.g) < density * 1.5)).float()    # P(nonzero) = 2/3 * 1.5 density

    def x(self, rows, K, density=None):
        if self.exact:
            return self._tern((rows, K), density or density_for(K)).to(self.dtype)
        return torch.randn(rows, K, generator=self.g).to(self.dtype)

    def w(self, N, K, density=None):
        """[ceil(N / 256) * 256][K] with zero rows behind N (the compiler-scheduled loop reads them)"""
        w = torch.zeros((N + 255) // 256 * 256, K, dtype=self.dtype)
        w[:N] = self._tern((N, K), density or density_for(K)).to(self.dtype) if self.exact else (torch.randn(N, K, generator=self.g) * K ** -0.5).to(self.dtype)
        return w

    def vec(self, N):
        return (torch.randint(-4, 5, (N,), generator=self.g).float() if self.exact else torch.randn(N, generator=self.g)).to(self.dtype)

    def res(self, rows, N):
        return (torch.randint(-8, 9, (rows, N), generator=self.g).float() if self.exact else torch.randn(rows, N, generator=self.g)).to(self.dtype)

    def res_lo(self, hi):
        """the lo plane of a split stream: quarters in the exact family, below half an ulp of hi otherwise"""
        if self.exact:
            return (torch.randint(-4, 5, hi.shape, generator=self.g).float() / 4).to(self.dtype)
        return ((torch.rand(hi.shape, generator=self.g) - 0.5).double() * ulp_at(hi.double(), self.dtype)).to(self.dtype)

    def gate(self, nb, stride):
        """fp32 [nb][stride]; small powers of two (both signs) in the exact family"""
        if self.exact:
            pw = torch.tensor([0.25, 0.5, 1.0, 2.0, -0.5, -1.0, -2.0])
            return pw[torch.randint(0, len(pw), (nb, stride), generator=self.g)]
        return torch.randn(nb, stride, generator=self.g)


def nan_buf(rows, ld, dtype):
    return torch.full((rows, ld), NAN, dtype=dtype)


def mapped(data, total_rows, cmap):
    """a NaN buffer [total_rows + GUARD][ld] with `data`'s rows at their mapped places"""
    buf = nan_buf(total_rows + GUARD, data.shape[1], data.dtype)
    buf[rowmap(torch.arange(data.shape[0]), *cmap)] = data
    return buf


def with_guard(data):
    return torch.cat([data, nan_buf(GUARD, data.shape[1], data.dtype)])


# ---- the gemm2 cases: name -> (bufs, [problems]) ------------------------------------------------------------------------------------------------------------
def case_embed(fam, single=False):
    """x_embedder pair: K = 64 (one k-step), two problems into the [I1 | I2] token ranges of every sample, split form without a gate onto zeroed planes"""
    K, N = 64, 2 * D
    bufs = {"x1": fam.x(B * I1, K), "x2": fam.x(B * I2, K), "w1": fam.w(N, K), "w2": fam.w(N, K), "b1": fam.vec(N), "b2": fam.vec(N)}
    m1, m2 = (I1, I, 0), (I2, I, I1)
    for name in ("hi", "lo"):
        bufs[name] = with_guard(torch.zeros(B * I, N, dtype=fam.dtype))
        if single:
            bufs[name][rowmap(torch.arange(B * I2), *m2)] = NAN            # rows no map reaches
    p1 = G2("x1", B * I1, K, N, "w1", "hi", bias="b1", c_map=m1, res="hi", res_lo="lo", out_lo="lo")
    p2 = G2("x2", B * I2, K, N, "w2", "hi", bias="b2", c_map=m2, res="hi", res_lo="lo", out_lo="lo")
    return bufs, [p1] if single else [p1, p2]


def case_qkv(fam):
    """qkv pair: image and context rows into one [B S][3 D] buffer, every row written exactly once"""
    K, N = D, 3 * D
    bufs = {"xi": fam.x(B * I, K), "xc": fam.x(B * T, K), "wi": fam.w(N, K), "wc": fam.w(N, K), "bi": fam.vec(N), "bc": fam.vec(N),
            "qkv": nan_buf(B * S + GUARD, N, fam.dtype)}
    return bufs, [G2("xi", B * I, K, N, "wi", "qkv", bias="bi", c_map=(I, S, T)), G2("xc", B * T, K, N, "wc", "qkv", bias="bc", c_map=(T, S, 0))]


def case_out(fam, split):
    """out pair: A read through the [ctx | img] map of the attention output, gated residual in place on the image / context streams.  Image rows 192..255 are a
    wave strip that straddles the two samples (I = 208), 256..319 one that lies wholly in sample 1."""
    K = N = D
    GS = 6 * D + 8                                                          # gate_stride > N; the gate starts at column 2 D of the modulation row
    bufs = {"att": fam.x(B * S, K), "wi": fam.w(N, K), "wc": fam.w(N, K), "bi": fam.vec(N), "bc": fam.vec(N),
            "img": with_guard(fam.res(B * I, N)), "ctx": with_guard(fam.res(B * T, N)), "gi": fam.gate(B, GS), "gc": fam.gate(B, GS)}
    lo = [{}, {}]
    if split:
        bufs["img_lo"], bufs["ctx_lo"] = with_guard(fam.res_lo(bufs["img"][:B * I])), with_guard(fam.res_lo(bufs["ctx"][:B * T]))
        lo = [dict(res_lo="img_lo", out_lo="img_lo"), dict(res_lo="ctx_lo", out_lo="ctx_lo")]
    return bufs, [G2("att", B * I, K, N, "wi", "img", bias="bi", lda=D, a_map=(I, S, T), res="img", gate="gi", gate_off=2 * D, rps=I, **lo[0]),
                  G2("att", B * T, K, N, "wc", "ctx", bias="bc", lda=D, a_map=(T, S, 0), res="ctx", gate="gc", gate_off=2 * D, rps=T, **lo[1])]


def case_single_mlp(fam):
    """single block, first half: GELU(mlp) of the normed hidden state (read at lda = 5 D from a buffer whose other columns are finite and distinct) into columns
    [D, 5 D) of `cat`, beside the attention output in columns [0, D), which must stay as they are"""
    bufs = {"hn": fam.x(B * S, 5 * D), "w": fam.w(4 * D, D), "b": fam.vec(4 * D), "cat": nan_buf(B * S + GUARD, 5 * D, fam.dtype)}
    bufs["cat"][:B * S, :D] = fam.x(B * S, D)
    return bufs, [G2("hn", B * S, D, 4 * D, "w", "cat", bias="b", lda=5 * D, ldc=5 * D, col_off=D, act=1)]


def case_single_out(fam, split, cat=None):
    """single block, second half: the gated out projection reads all 5 D columns of `cat`, residual in place on the joint stream"""
    K, N, GS = 5 * D, D, 3 * D + 8
    bufs = {"cat": cat[:B * S].clone() if cat is not None else fam.x(B * S, K), "w": fam.w(N, K), "b": fam.vec(N), "hs": with_guard(fam.res(B * S, N)),
            "g": fam.gate(B, GS)}
    lo = {}
    if split:
        bufs["hs_lo"] = with_guard(fam.res_lo(bufs["hs"][:B * S]))
        lo = dict(res_lo="hs_lo", out_lo="hs_lo")
    return bufs, [G2("cat", B * S, K, N, "w", "hs", bias="b", lda=5 * D, res="hs", gate="g", gate_off=2 * D, rps=S, **lo)]


def case_head(fam, N, second=False, planes=None):
    """proj_out: N = 64 (a quarter of a tile) or 264 (a tile and one 8-column chunk), split form without a gate, run twice onto zeroed planes: with the bias, then
    (second) without one on top of the first result"""
    K, M = D, B * I
    bufs = {"y": fam.x(M, K), "w": fam.w(N, K), "b": fam.vec(N)}
    bufs["hi"], bufs["lo"] = planes if planes else (with_guard(torch.zeros(M, N, dtype=fam.dtype)), with_guard(torch.zeros(M, N, dtype=fam.dtype)))
    return bufs, [G2("y", M, K, N, "w", "hi", bias=None if second else "b", res="hi", res_lo="lo", out_lo="lo")]


def case_plain(fam, M, K, N=256, gated=False, split=False):
    """one problem, identity maps: the k-step counts (K = 64, 128, 192, 320: prologue only, and the odd / even exits of both k loops) and the M edges"""
    bufs = {"x": fam.x(M, K), "w": fam.w(N, K), "b": fam.vec(N)}
    kw = {}
    if gated:
        bufs["out"] = with_guard(fam.res(M, N))
        bufs["g"] = fam.gate((M + 99) // 100, N + 8)
        kw = dict(res="out", gate="g", rps=100)
        if split:
            bufs["out_lo"] = with_guard(fam.res_lo(bufs["out"][:M]))
            kw.update(res_lo="out_lo", out_lo="out_lo")
    else:
        bufs["out"] = nan_buf(M + GUARD, N, fam.dtype)
    return bufs, [G2("x", M, K, N, "w", "out", bias="b", **kw)]


def case_banded(fam):
    """24 column tiles (bands of 4 row tiles, row tile fastest) and 6 row tiles, the last band 2 tiles high and the last tile 10 rows"""
    return case_plain(fam, 5 * 256 + 10, 64, 6144)


TAIL_M, TAIL_N, TAIL_K, TAIL_SEG = 17 * 256, 16 * 256, 6144, 17 * 128          # 272 tiles: 256 in the main launch, the last row tile's 16 in the split-K tail


def tail_rows(M=TAIL_M, tail_from=16 * 256):
    """reference rows of the split-K cases: all rows of the tail tiles, the first and last row of every row tile, one in eight of the rest"""
    r = set(range(tail_from, M)) | set(range(0, M, 8))
    for t in range(0, M, 256):
        r |= {t, min(t + 255, M - 1)}
    return torch.tensor(sorted(r))


@functools.lru_cache(maxsize=None)
def _tail_operands():
    """x, w of the split-K cases as fp32 integers (exact in both dtypes), shared by every case that uses them"""
    fam = Family("exact", torch.float32, 77)
    return fam.x(TAIL_M, TAIL_K), fam.w(TAIL_N, TAIL_K), fam.vec(TAIL_N)


def case_tail(dtype, split, pair=False):
    """17 x 16 tiles at K = 6144: the launch splits into 256 full-K tiles and a tail of 16 tiles computed as k ranges into fp32 partials (g2_tail_splits), with a
    row map on C (two samples of 2176 rows, 24 gap rows between them) and a gate; the tile of rows 2048..2303 straddles the samples.
    pair: the same rows as two problems of 16 and 1 row tiles, so that the tail is all of the second problem."""
    x, w, b = _tail_operands()
    fam = Family("exact", dtype, 78 + split)
    cm = (TAIL_SEG, TAIL_SEG + 24, 8)
    total = 2 * (TAIL_SEG + 24) + 8
    bufs = {"x": x.to(dtype), "w": w.to(dtype), "b": b.to(dtype), "out": mapped(fam.res(TAIL_M, TAIL_N), total, cm), "g": fam.gate(2, TAIL_N + 8)}
    lo = {}
    if split:
        bufs["out_lo"] = mapped(fam.res_lo(torch.zeros(TAIL_M, TAIL_N, dtype=dtype)), total, cm)
        lo = dict(res_lo="out_lo", out_lo="out_lo")
    if not pair:
        return bufs, [G2("x", TAIL_M, TAIL_K, TAIL_N, "w", "out", bias="b", c_map=cm, res="out", gate="g", rps=TAIL_SEG, **lo)]
    # two problems over the same buffers: rows [0, 4096) and [4096, 4352); the second reads A and writes C from row 4096 on (a_map / c_map offsets), and its
    # gate rows are those of sample 1 (4096 >= 2176), passed as their own one-row gate
    bufs["g1"] = bufs["g"][1:2].clone()
    M0 = 16 * 256
    c1 = (0, 0, int(rowmap(M0, *cm)))
    return bufs, [G2("x", M0, TAIL_K, TAIL_N, "w", "out", bias="b", c_map=cm, res="out", gate="g", rps=TAIL_SEG, **lo),
                  G2("x", TAIL_M - M0, TAIL_K, TAIL_N, "w", "out", bias="b", a_map=(0, 0, M0), c_map=c1, res="out", gate="g1", rps=TAIL_M, **lo)]


KSTEPS = (64, 128, 192, 320)
M_EDGES = (1, 63, 64, 65, 255, 256, 257, 513)


def exact_cases(dtype):
    """every exact-family case of tests/test_flux_gemm2_forms_gpu.py: name -> (builder, reference rows or None).  tests/test_flux_ref.py verifies the family's
    conditions on all of them on the CPU."""
    f = lambda seed: Family("exact", dtype, seed)
    c = {"embed_pair": (lambda: case_embed(f(1)), None), "embed_single": (lambda: case_embed(f(1), single=True), None), "qkv_pair": (lambda: case_qkv(f(2)), None),
         "out_pair_plain": (lambda: case_out(f(3), False), None), "out_pair_split": (lambda: case_out(f(3), True), None),
         "single_out_plain": (lambda: case_single_out(f(4), False), None), "single_out_split": (lambda: case_single_out(f(4), True), None),
         "head_64": (lambda: case_head(f(5), 64), None), "head_264": (lambda: case_head(f(6), 264), None), "banded": (lambda: case_banded(f(7)), None)}
    for K in KSTEPS:
        c[f"ksteps_{K}"] = (lambda K=K: case_plain(f(10 + K), 300, K), None)
    for M in M_EDGES:
        c[f"m_{M}_plain"] = (lambda M=M: case_plain(f(20 + M), M, 128, gated=True), None)
        c[f"m_{M}_split"] = (lambda M=M: case_plain(f(20 + M), M, 128, gated=True, split=True), None)
    c["tail_plain"] = (lambda: case_tail(dtype, False), tail_rows())
    c["tail_split"] = (lambda: case_tail(dtype, True), tail_rows())
    c["tail_pair"] = (lambda: case_tail(dtype, True, pair=True), tail_rows())
    return c


def pair_rows(p, rows):
    """the logical rows of problem p among the reference rows of a tail pair (problem 1 starts at logical row a_map offset)"""
    if rows is None:
        return None
    off = p.a_map[2] if not p.a_map[0] else 0
    r = rows[(rows >= off) & (rows < off + p.M)] - off
    return r


def check_exact_conditions(bufs, p, dtype, rows=None):
    """the exact family's conditions on the reference (never on an output): integer branch values inside T's exact range, a final value inside it too, and every
    value equal to its fp32 evaluation.  Returns the g2_values."""
    o = g2_values(bufs, p, dtype, exact=True, rows=rows)
    lim = exact_limit(dtype)
    assert not p.act
    assert bool((o.v == o.v.round()).all()) and float(o.v.abs().max()) <= lim, float(o.v.abs().max())
    assert float(o.ref.abs().max()) <= lim, float(o.ref.abs().max())
    assert torch.equal(o.ref.float().double(), o.ref) and torch.equal(rnd(o.v, dtype), o.v)
    return o


# ---- qk_norm_rope -------------------------------------------------------------------------------------------------------------------------------------------
def qk_norm_rope_ref(buf, rows, seq, heads, dh, q_col, k_col, wq, wk, wq_ctx, wk_ctx, ctx_rows, cos, sin, eps, dtype=None):
    """(q, k) float64 [rows][heads][dh] after the op; dtype given: with the kernel's rounding points"""
    pos = torch.arange(rows) % seq
    ctx = (pos < ctx_rows)[:, None, None]
    c, s = cos[pos].double()[:, None, :], sin[pos].double()[:, None, :]
    out = []
    for col, wi, wc in ((q_col, wq, wq_ctx), (k_col, wk, wk_ctx)):
        x = buf[:rows, col:col + heads * dh].double().reshape(rows, heads, dh)
        w = torch.where(ctx, (wc if wc is not None else wi).double()[None, None, :], wi.double()[None, None, :])
        r = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
        n = rnd(rnd(x * r.float().double(), dtype) * w, dtype) if dtype else x * r * w
        a, b = n[..., 0::2], n[..., 1::2]
        o = torch.stack((a * c - b * s, b * c + a * s), -1).reshape(rows, heads, dh)
        out.append(rnd(o, dtype) if dtype else o)
    return out


def rope_tables(seq, dh, seed):
    """fp32 cos / sin [seq][dh / 2] of distinct angles per position (position 0 is NOT the identity, so a wrong position shows)"""
    ang = torch.rand(seq, dh // 2, generator=_gen(seed), dtype=torch.float64) * 2 * math.pi
    return torch.cos(ang).float(), torch.sin(ang).float()


# ---- ln_modulate --------------------------------------------------------------------------------------------------------------------------------------------
def ln_modulate_fp64(x, x_lo, rps, shift, scale, eps):
    """float64 [M][C]: LayerNorm without affine of x (+ x_lo), times 1 + scale[m / rps], plus shift[m / rps]; shift / scale fp32 [nb][C]"""
    xs = x.double() + (x_lo.double() if x_lo is not None else 0.0)
    b = torch.div(torch.arange(x.shape[0]), rps, rounding_mode="floor")
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    return (xs - mean) * torch.rsqrt(var + eps) * (1.0 + scale.double()[b]) + shift.double()[b]


def ln_modulate_emulated(x, x_lo, rps, shift, scale, eps, dtype):
    """(y, y_lo) float64: one rounding, y_lo = T(o - y)"""
    o = ln_modulate_fp64(x, x_lo, rps, shift, scale, eps)
    y = rnd(o, dtype)
    return y, rnd(o - y, dtype)


def ln_fp32_bound(x, x_lo, rps, shift, scale, eps, dtype):
    """per element: how far an fp32 evaluation of ln_modulate, stored as y + y_lo, may be from float64.  With u = 2^-24:
      sums     each lane adds at most 8 ceil(C / 512) terms and the 64 lane sums are combined in at most 63 more adds: gamma = (8 ceil(C / 512) + 66) u;
      mean     dm <= (gamma + u) A, A = mean |x + x_lo| (u: the fp32 sum of the two planes);
      d        e_d <= dm + 2 u (|x| + |d|);
      var      a common shift dm of every d adds dm^2 (the d sum to zero), the elements' own roundings at most 4 u A sd: rho <= gamma + 4 u + (dm / sd)^2 + 4 u A / sd;
      rstd     rho / 2 + 8 u (rsqrt's ulps, the division by C, eps);
      o        |1 + s| e_d / sd + |z (1 + s)| (rho / 2 + 8 u + 4 u) + 2 u (|o| + |shift|);
      y_lo     |y_lo| <= ulp_T(o), rounded to T: ulp_T(ulp_T(o))."""
    u = 2.0 ** -24
    xs = x.double() + (x_lo.double() if x_lo is not None else 0.0)
    C = x.shape[1]
    b = torch.div(torch.arange(x.shape[0]), rps, rounding_mode="floor")
    s1, h = (1.0 + scale.double()[b]).abs(), shift.double()[b].abs()
    mean = xs.mean(-1, keepdim=True)
    d = xs - mean
    sd = torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    gamma = (8 * ((C + 511) // 512) + 66) * u
    A = xs.abs().mean(-1, keepdim=True)
    dm = (gamma + u) * A
    e_d = dm + 2 * u * (xs.abs() + d.abs())
    rho = gamma + 4 * u + (dm / sd) ** 2 + 4 * u * A / sd
    o = ln_modulate_fp64(x, x_lo, rps, shift, scale, eps)
    return s1 * e_d / sd + (d / sd).abs() * s1 * (rho / 2 + 12 * u) + 2 * u * (o.abs() + h) + ulp_at(ulp_at(o, dtype), dtype)


def ln_inputs(M, C, dtype, seed, split):
    """x (and x_lo), shift / scale rows with mod_stride = 2 C + 24 > 2 C, rows_per_sample that does not divide M (M > 1).  The last row has a large mean and a
    small variance (64 + 0.3 N(0, 1): a few spacings of T)."""
    g = _gen(seed)
    x = (torch.randn(M, C, generator=g) * (0.5 + torch.rand(M, 1, generator=g) * 4) + torch.randn(M, 1, generator=g)).to(dtype)
    if M > 1:
        x[M - 1] = (64.0 + 0.3 * torch.randn(C, generator=g)).to(dtype)
    x_lo = ((torch.rand(M, C, generator=g) - 0.5).double() * ulp_at(x.double(), dtype)).to(dtype) if split else None
    rps = 1 if M == 1 else (2 if M < 10 else 333)
    nb = (M + rps - 1) // rps
    mod = torch.randn(nb, 2 * C + 24, generator=g) * 0.5
    return x, x_lo, rps, mod


# ---- small_linear, sinusoid ---------------------------------------------------------------------------------------------------------------------------------
def silu64(x):
    return x * torch.sigmoid(x)


def small_linear_fp64(x, w, bias, silu_in, silu_out):
    """(out, S, pre): float64 out [R][N], S = sum_k |x_k w_k| + |bias| of the accumulation bound, pre = the value in front of the output SiLU"""
    xx = silu64(x.double()) if silu_in else x.double()
    bb = bias.double() if bias is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    pre = xx @ w.double().T + bb
    S = xx.abs() @ w.double().abs().T + bb.abs()
    return (silu64(pre) if silu_out else pre), S, pre


def small_linear_bound(K, S, pre, silu_out):
    """(K + 2) 2^-23 S: K - 1 adds and one product rounding per term are K 2^-24 S; the other half holds the input SiLU, whose fast form x / (1 + exp(-x)) is off by
    at most (|x| + 4) 2^-24 relative (|x| 2^-24 from the rounded exponent, an ulp each of v_exp_f32 and of the division) -- the inputs stay inside |x| <= 4, and
    K >= 8.  The output SiLU passes an error through with |silu'| <= 1.1 and adds (|v| + 4) 2^-24 |silu(v)| of its own."""
    bound = (K + 2) * 2.0 ** -23 * S
    if silu_out:
        bound = 1.1 * bound + (pre.abs() + 4) * 2.0 ** -24 * silu64(pre).abs() + 1e-37
    return bound


def sinusoid_fp64(t, mult, C):
    """[R][C] = [cos | sin] of t mult exp(-ln(1e4) k / (C / 2)); returns (out, angle)"""
    half = C // 2
    a = t.double()[:, None] * mult * torch.exp(-math.log(1e4) * torch.arange(half, dtype=torch.float64) / half)[None, :]
    return torch.cat((torch.cos(a), torch.sin(a)), -1), a


def sinusoid_bound(a):
    """fp32 error of the argument: the exponent -ln(1e4) k / half carries the rounded constant and one product rounding (the division by a power of two is exact),
    2 * 2^-24 * 9.21 absolute, i.e. 18.4 * 2^-24 relative in exp; expf within 2 ulp (4 * 2^-24); t * mult and * f round once each (2 * 2^-24): 26 * 2^-24 |a| in
    all, 1.5e-3 at |a| = 1000.  cos and sin have slope <= 1 and are themselves within 4 * 2^-24."""
    return a.abs() * 26 * 2.0 ** -24 + 4 * 2.0 ** -24
