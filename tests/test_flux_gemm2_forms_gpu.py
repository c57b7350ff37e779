"""gemm2.hip through cs_op_gemm2_ex, element by element, in the call shapes of flux.cpp: row maps on A and C, lda / ldc / column offset, gates per sample, the
split residual stream, pairs, N below a tile, one k-step, the banded tile order and the split-K tail.  References and bounds: tests/flux_ref.py (verified on the
CPU by tests/test_flux_ref.py).

Every case fills what the op must not touch (gap rows between segments, 8 guard rows behind every output buffer, columns beside a column offset) with NaN or data
and compares the WHOLE buffer: bit-unchanged outside the written region, every element inside it checked.  Both k loops (gemm2_w8 = 1 hand-scheduled, 0 compiler-
scheduled) run on the same inputs and must agree bit for bit.

  exact family   x, w in {-1, 0, 1}, small-integer bias / residual, quarter-integer lo planes, power-of-two gates: every sum is exact in fp32 whatever its order, so
                 the output must EQUAL the float64 reference cast to T (hi) and T(reference - hi) (lo).  The range conditions are asserted on the reference.
  random family  |out - emulator| <= |gate| (g S + ulp_T(branch)) + ulp_T(out) per element, S = sum_k |a_k w_k| + |bias| in float64, g = (K + 2) 2^-23: the worst
                 case of an fp32 accumulation of K products and the bias in any order, at 2^-23 per operation because the matrix core's internal rounding is not
                 assumed to be round-to-nearest.  An accumulation error can move the branch value's rounding to T by one ulp_T(branch), scaled by the gate; the sum's
                 own rounding can move by one ulp_T(out).  The split form is also held, as hi + lo, to the fp32-class bound of flux_ref.g2_values (bound_sum).
                 GELU: g S is multiplied by the derivative bound 1.13 and the fast form's own error is added; both are derived in flux_ref's docstring:
                     d/dx [x s(2u)] = s + x s (1 - s) 2u' has its extremes 1.1290 / -0.1290 near x = +-1.45;
                     |dy| <= |y| (e / (1 + e) (|arg| ln2 6 2^-24 + 2^-23) + 2^-22) for y = x / (1 + e), e = exp2(arg), arg = x (c1 + c2 x^2) in fp32.
Every random case prints its worst err / bound (RATIO).  Seen on an MI355X: out against the emulator 0.97 at most (out pair, plain, bf16: a branch value whose
rounding the accumulation order moved by one ulp, times the gate), GELU 0.49, hi + lo against float64 0.20.

Not reachable: a pair of two dtypes (launch_gemm2_pair rejects it, cs_op_gemm2_ex passes one dtype for both problems)."""
import ctypes as C

import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import ops
from tests import flux_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x7FD5              # a NaN bit pattern in f16 and in bf16
CS_E_ARG, CS_E_SHAPE = -1, -2
DT = list(R.DTYPES.items())


def _structs(dev, bufs, p):
    assert (p.lda or p.K) == bufs[p.a].shape[1] and (p.ldc or p.N) == bufs[p.out].shape[1]
    ptr = lambda name: dev[name].data_ptr() if name else None
    gate = dev[p.gate].data_ptr() + 4 * p.gate_off if p.gate else None
    prob = L.CsGemm2Problem(ptr(p.a), p.M, p.K, ptr(p.w), ptr(p.bias), p.N, ptr(p.res), gate, bufs[p.gate].shape[1] if p.gate else 0, p.rps, p.act,
                            ptr(p.out), p.ldc, p.col_off)
    addr = L.CsGemm2Addressing(p.lda, p.a_map[0], p.a_map[1], p.a_map[2], p.c_map[0], p.c_map[1], p.c_map[2], ptr(p.res_lo), ptr(p.out_lo))
    return prob, addr


def launch(dev, bufs, probs, dtype, ws=None):
    """one cs_op_gemm2_ex call for one problem or a pair; returns the ABI's code"""
    s = [_structs(dev, bufs, p) for p in probs]
    b = (C.byref(s[1][0]), C.byref(s[1][1])) if len(s) > 1 else (None, None)
    return L.lib().cs_op_gemm2_ex(C.byref(s[0][0]), C.byref(s[0][1]), *b, L.dtype_code(dtype), L.ptr(ws), ws.numel() if ws is not None else 0, L.stream_ptr(DEV))


def written_names(probs):
    return sorted({n for p in probs for n in (p.out, p.out_lo) if n})


def run_both_loops(bufs, probs, dtype, ws=None):
    """the case through the hand-scheduled and the compiler-scheduled k loop on fresh copies of the buffers: bit-identical; returns the outputs on the CPU"""
    names = written_names(probs)
    dev = {k: v.to(DEV) for k, v in bufs.items() if k not in names}
    outs = []
    for w8 in (1, 0):
        dev.update({k: bufs[k].to(DEV) for k in names})
        try:
            ops.set_tuning("gemm2_w8", w8)
            L.check(launch(dev, bufs, probs, dtype, ws))
        finally:
            ops.reset_tuning()
        torch.cuda.synchronize()
        outs.append({k: dev[k].cpu() for k in names})
    for k in names:
        assert torch.equal(outs[0][k].view(torch.int16), outs[1][k].view(torch.int16)), f"gemm2_w8 1 and 0 differ in {k}"
    return outs[0]


def check(bufs, probs, outs, dtype, family, what, rows=None):
    """every element of every written buffer (on the reference rows where `rows` is given); prints the random family's worst err / bound before it asserts"""
    mask = {k: torch.zeros(bufs[k].shape, dtype=torch.bool) for k in outs}
    worst = worst_sum = 0.0
    for p in probs:
        r = R.pair_rows(p, rows)
        if family == "exact":
            o = R.check_exact_conditions(bufs, p, dtype, r)
            hi = o.ref.to(dtype)
            got = outs[p.out][o.crow, o.cols]
            bad = (got != hi) | got.isnan()
            assert not bool(bad.any()), (what, "hi", int(bad.sum()), o.m[bad.any(1)][:8].tolist())
            if p.out_lo:
                lo = (o.ref - hi.double()).to(dtype)
                bad = (outs[p.out_lo][o.crow, o.cols] != lo) | outs[p.out_lo][o.crow, o.cols].isnan()
                assert not bool(bad.any()), (what, "lo", int(bad.sum()), o.m[bad.any(1)][:8].tolist())
        else:
            o = R.g2_values(bufs, p, dtype, rows=r)
            got = outs[p.out][o.crow, o.cols].double()
            assert bool(torch.isfinite(got).all()), what
            ratio = (got - o.emu).abs() / o.bound
            worst = max(worst, float(ratio.max()))
            if p.out_lo:
                lo = outs[p.out_lo][o.crow, o.cols].double()
                assert bool(torch.isfinite(lo).all()), what
                rs = (got + lo - o.ref).abs() / o.bound_sum
                worst_sum = max(worst_sum, float(rs.max()))
                assert bool((lo.abs() <= R.ulp_at(got, dtype)).all()), what
        allrows = R.rowmap(torch.arange(p.M), *p.c_map)
        for k in (p.out, p.out_lo):
            if k:
                assert not bool(mask[k][allrows, o.cols].any()), (what, "two problems write the same element")
                mask[k][allrows, o.cols] = True
    if family != "exact":
        print(f"RATIO {what}: out vs emulator {worst:.3f}" + (f"  hi + lo vs float64 {worst_sum:.3f}" if worst_sum else ""))
        assert worst <= 1.0 and worst_sum <= 1.0, (what, worst, worst_sum)
    for k, m in mask.items():
        keep = ~m
        assert torch.equal(outs[k].view(torch.int16)[keep], bufs[k].view(torch.int16)[keep]), (what, k, "touched outside the written region")
        assert bool(torch.isfinite(outs[k][m]).all()), (what, k, "an element inside the written region was left as it was")


def workspace():
    nb = L.lib().cs_op_gemm2_workspace(17 * 16, R.TAIL_K)
    assert nb == 16 * 4 * 256 * 256 * 4                       # 16 tail tiles as 4 k ranges of 24 k-steps
    return torch.empty(nb, dtype=torch.uint8, device=DEV)


# ---- 1. the exact family: every form without GELU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", list(R.exact_cases(R.BF16)))
@pytest.mark.parametrize("name,dt", DT)
def test_exact_family_equals_the_float64_reference(name, dt, cname):
    build, rows = R.exact_cases(dt)[cname]
    bufs, probs = build()
    outs = run_both_loops(bufs, probs, dt, workspace() if cname.startswith("tail") else None)
    check(bufs, probs, outs, dt, "exact", f"{cname} {name}", rows)


# ---- 2. the random family -------------------------------------------------------------------------------------------------------------------------------------
def _random_cases(dt):
    f = lambda seed: R.Family("random", dt, seed)
    c = {"embed_pair": lambda: R.case_embed(f(1)), "embed_single": lambda: R.case_embed(f(1), single=True), "qkv_pair": lambda: R.case_qkv(f(2)),
         "out_pair_plain": lambda: R.case_out(f(3), False), "out_pair_split": lambda: R.case_out(f(3), True),
         "single_out_plain": lambda: R.case_single_out(f(4), False), "single_out_split": lambda: R.case_single_out(f(4), True)}
    for K in R.KSTEPS:
        c[f"ksteps_{K}"] = lambda K=K: R.case_plain(f(10 + K), 300, K)
    for M in (1, 65, 257):
        c[f"m_{M}_plain"] = lambda M=M: R.case_plain(f(20 + M), M, 128, gated=True)
        c[f"m_{M}_split"] = lambda M=M: R.case_plain(f(20 + M), M, 128, gated=True, split=True)
    return c


@pytest.mark.parametrize("cname", list(_random_cases(R.BF16)))
@pytest.mark.parametrize("name,dt", DT)
def test_random_family_within_the_accumulation_bound(name, dt, cname):
    bufs, probs = _random_cases(dt)[cname]()
    outs = run_both_loops(bufs, probs, dt)
    check(bufs, probs, outs, dt, "random", f"{cname} {name}")


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name,dt", DT)
def test_single_block_gelu_beside_attention_then_out_projection(name, dt, split):
    """GELU(mlp) at ldc = 5 D, column offset D: columns [0, D) keep the attention output bit for bit; then the gated projection reads all 5 D columns of that buffer"""
    fam = R.Family("random", dt, 40)
    bufs, probs = R.case_single_mlp(fam)
    outs = run_both_loops(bufs, probs, dt)
    check(bufs, probs, outs, dt, "random", f"single_mlp_gelu {name}")
    assert torch.equal(outs["cat"][:R.B * R.S, :R.D].view(torch.int16), bufs["cat"][:R.B * R.S, :R.D].view(torch.int16))
    bufs2, probs2 = R.case_single_out(fam, split, cat=outs["cat"])
    outs2 = run_both_loops(bufs2, probs2, dt)
    check(bufs2, probs2, outs2, dt, "random", f"single_out_after_gelu {'split' if split else 'plain'} {name}")


@pytest.mark.parametrize("family", ["exact", "random"])
@pytest.mark.parametrize("N", [64, 264])
@pytest.mark.parametrize("name,dt", DT)
def test_head_runs_twice_onto_zeroed_planes_then_planes_to_f32(name, dt, N, family):
    bufs, probs = R.case_head(R.Family(family, dt, 50 + N), N)
    outs = run_both_loops(bufs, probs, dt)
    check(bufs, probs, outs, dt, family, f"head_{N} first {name}")
    bufs2, probs2 = R.case_head(R.Family(family, dt, 50 + N), N, second=True, planes=(outs["hi"], outs["lo"]))
    assert probs2[0].bias is None
    outs2 = run_both_loops(bufs2, probs2, dt)
    check(bufs2, probs2, outs2, dt, family, f"head_{N} second, null bias {name}")
    M = R.B * R.I
    hi, lo = outs2["hi"][:M].contiguous().to(DEV), outs2["lo"][:M].contiguous().to(DEV)
    f32 = torch.full((M * N + 8,), float("nan"), device=DEV)
    L.check(L.lib().cs_op_planes_to_f32(L.ptr(hi), L.ptr(lo), L.ptr(f32), M * N, L.dtype_code(dt), L.stream_ptr(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(f32[:M * N].cpu(), (outs2["hi"][:M].float() + outs2["lo"][:M].float()).reshape(-1)) and bool(f32[M * N:].isnan().all())


# ---- 3. rejections: a code and a message, nothing launched ----------------------------------------------------------------------------------------------------
def test_rejections_return_their_code_and_leave_out_alone():
    dt = R.BF16
    M, K, N = 64, 128, 256
    z = lambda *s, d=dt: torch.zeros(*s, dtype=d, device=DEV)
    filled = lambda *s: torch.full(s, FILL, dtype=torch.int16, device=DEV).view(dt)
    base = {"x": z(M, K + 64), "w": z(N, K + 64), "b": z(N), "g": z(1, N, d=torch.float32)}

    def reject(code, text, two=False, **kw):
        dev = dict(base, out=filled(M + 8, N + 64), lo=filled(M + 8, N + 64))
        args = dict(a="x", M=M, K=K, N=N, w="w", out="out", bias="b", lda=K + 64, ldc=N + 64)
        args.update(kw)
        p = R.G2(**args)
        good = R.G2("x", M, K, N, "w", "out", bias="b", lda=K + 64, ldc=N + 64)
        s = [_raw(dev, q) for q in ([good, p] if two else [p])]
        b = (C.byref(s[1][0]), C.byref(s[1][1])) if two else (None, None)
        rc = L.lib().cs_op_gemm2_ex(C.byref(s[0][0]), C.byref(s[0][1]), *b, L.dtype_code(dt), None, 0, L.stream_ptr(DEV))
        torch.cuda.synchronize()
        msg = L.lib().cs_last_error().decode()
        assert rc == code and text in msg, (kw, rc, msg)
        assert bool((dev["out"].view(torch.int16) == FILL).all()) and bool((dev["lo"].view(torch.int16) == FILL).all()), kw

    def _raw(dev, p):
        ptr = lambda name: dev[name].data_ptr() if name else None
        prob = L.CsGemm2Problem(ptr(p.a), p.M, p.K, ptr(p.w), ptr(p.bias), p.N, ptr(p.res), ptr(p.gate), N if p.gate else 0, p.rps, p.act, ptr(p.out), p.ldc, p.col_off)
        return prob, L.CsGemm2Addressing(p.lda, *p.a_map, *p.c_map, ptr(p.res_lo), ptr(p.out_lo))

    for two in (False, True):                                                     # alone, and as the second problem of a pair (the first is fine)
        reject(CS_E_SHAPE, "K=96 must be a multiple of 64", two, K=96)
        for bad in (dict(N=N - 4), dict(lda=K + 68), dict(ldc=N + 68), dict(col_off=4)):
            reject(CS_E_SHAPE, "multiples of 8", two, **bad)
        reject(CS_E_ARG, "res_lo and out_lo go together", two, res="out", res_lo="lo")
        reject(CS_E_ARG, "rows_per_sample required with gate", two, res="out", gate="g")
    # (a pair whose problems differ in activation or in the split form runs as two launches: those rejections are checked on one problem)
    reject(CS_E_ARG, "res_lo and out_lo go together", res_lo="lo", out_lo="lo")                       # ... and need res
    reject(CS_E_ARG, "excludes an activation", res="out", res_lo="lo", out_lo="lo", act=1)
    reject(CS_E_ARG, "act must be 0 (none) or 1", act=2)
    # a null problem
    assert L.lib().cs_op_gemm2_ex(None, None, None, None, 2, None, 0, L.stream_ptr(DEV)) == CS_E_ARG
