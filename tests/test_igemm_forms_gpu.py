"""csrc/igemm.hip route by route against float64: every conv3x3 / conv1x1 / linear route of launch_igemm (decided by igemm_plan, csrc/igemm_plan.h), the split-K reduce kernels, the GroupNorm and
row statistics the epilogues leave, and the small-Cout conv_out kernels of csrc/misc.hip.  References, input families, bounds and the case lists: tests/igemm_ref.py
(pinned on the CPU by tests/test_igemm_ref.py).

Every case
  * runs with its outputs (and statistics buffers) inside NaN-filled buffers whose margins, and every element the op must not write, are compared bit for bit;
  * asserts with ops.igemm_last_route() that the dispatcher took the kernel the case is for (family, tile columns, variant as numbered by the index functions of
    csrc/igemm_plan.h, split-K factor, who left the statistics);
  * exact family (small integers, every fp32 sum exact in any order): EVERY output element equals the reference bit for bit;
  * random family: prints RATIO = worst |out - rnd16(ref)| / bound over the elements and asserts it <= 1.0, the bound derived per element in tests/igemm_ref.py;
  * restores the knobs with ops.reset_tuning() in a finally.

Route table (knobs -> what the record must say; the shapes are in tests/igemm_ref.py; the variant numbers are the enums next to the named index functions of
csrc/igemm_plan.h, which tests/test_igemm_plan.py asserts for the same cases on the CPU):
    conv_halo 0                              generic igemm_kernel<128 | 160, CONV3> (N = 640: 128 columns); split-K 2 / 4 / 8 at 16 x 16 -> 8 x 8 stride 2 with
                                             cin 128 / 256 / 512; splitk_reduce_stats_kernel when HoWo = 64, else splitk_reduce_kernel + the statistics pass
    conv_halo 2, conv_lw 0                   conv3_halo_kernel<UP, 128 | 160, 1>; conv_halo 3: <UP, 256 | 320, 2>; split over chunks 2 / 4 / 8 at cin 128 / 256 / 512
    conv_halo 2, conv_lw 1 | 2               conv3_lw_kernel, conv_lw_variant (ConvLwVariant): 0 FAST 160, 1 plain 160, 2 upsample plain 160, 5 upsample FAST 160, 6 FAST 128, 7 plain 128,
                                             8 upsample plain 128, 9 upsample FAST 128, 10 fast8 (8 x 8, four images per tile); N = 640 -> 160 columns
    cs_op_conv_up_sub                        sub_variant (SubVariant): 0 f1 160 (16 x 16 input patches), 1 f2 160 (8 x 8), 2 f1 128
    gemm_big 0                               igemm_kernel<128 | 160> (igemm_kernel_form / IK_VARIANT: LNM | EPI << 2 | GEGLU << 4)
    gemm_big 2, gemm_w8 0 | 1                gemm_big_kernel<., 320> | gemm_w8_kernel, w8_variant (W8Variant): 0 plain, 1 GEGLU, 4 row statistics, 7 residual + lo plane in, no lo plane out
    gemm_big 3, gemm_lw 0 | 1                gemm_big_kernel<false, 160> | gemm_lw_kernel, gemm_lw_variant (GemmLwVariant): 0 plain, 2 row statistics, 5 residual + lo plane in, no lo plane out
Every row of the table was confirmed by the record on an MI355X: no listed shape took another route.  The reduce kernels: splitk_reduce_stats_kernel behind the
HoWo = 64 split-K cases with statistics (generic, halo and loader-wave), splitk_reduce_kernel behind the others.

Worst RATIO seen per route family on an MI355X (0.98 = one fp16 ulp off rnd16(ref) at a short sum, where the fp32 value sits next to a rounding boundary):
    generic 0.980 (3x3 and 1x1 / linear), halo 0.668, conv3_lw 0.714, sub_pixel 0.338, gemm_big 0.980, gemm_w8 0.980, gemm_lw 0.980, conv_out 0.485;
    GEGLU: generic 0.901, gemm_big 0.888, gemm_w8 0.895; split outputs (the worse of the hi rule and the hi + lo rule): generic 0.946, gemm_w8 0.946, gemm_lw 0.937;
    3x3 with split planes (generic, halo, conv3_lw incl. split-K) 0.500: |lo| at half an ulp of hi.
Wall time of the module on an MI355X: 4.6 s for its 177 tests (the slowest 0.25 s).

What the module found: GEGLU with N % 128 != 0 (N = 320, 960) and too few rows to fill the 320-column kernels went to the generic tiles, which counted
160-column tiles and launched the 128-column GEGLU kernel: output columns 128 tiles_n .. N / 2 were never written.  igemm_plan sends that shape to the
320-column kernels and refuses it when gemm_big is 0 (test_geglu_on_each_route_that_has_it, test_refusals_leave_the_output_untouched).

Variants no case reaches: LW_TRACE_FAST160 / LW_TRACE160 (the stamped conv3_lw instantiations: debug bit 16384 only); W8_LN / W8_GEGLU_LN / GLW_LN (the folded-LayerNorm
consumers) and W8_LO8 / W8_LO8_STATS / GLW_LO8 / GLW_LO8_STATS (8-bit lo planes) belong to tests/test_ln_fold_gpu.py and tests/test_residual_x2_gpu.py.
"""
import math

import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import ops
from tests import igemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CS_E_ARG, CS_E_SHAPE = -1, -2
G = 64                               # NaN elements in front of and behind every output
F16, F32 = torch.float16, torch.float32
_WORST = {}                          # route family -> worst RATIO of this run (printed by every case)


def guarded(*shape, dtype=F16):
    """(buffer, view): a NaN-filled buffer with G elements of margin around a view of `shape`"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * G,), R.NAN, dtype=dtype, device=DEV)
    return buf, buf[G:G + n].view(*shape)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


_NAN_BITS = {F16: bits(torch.full((1,), R.NAN, dtype=F16))[0].item(), F32: bits(torch.full((1,), R.NAN, dtype=F32))[0].item()}


def margins_intact(*bufs):
    for buf in bufs:
        b = bits(buf)
        if not (bool((b[:G] == _NAN_BITS[buf.dtype]).all()) and bool((b[-G:] == _NAN_BITS[buf.dtype]).all())):
            return False
    return True


def untouched(buf):
    return bool((bits(buf) == _NAN_BITS[buf.dtype]).all())


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def dev(t):
    return t.to(DEV) if t is not None else None


def route_is(route, family, cols=None, variant=None, splits=None, gn_done=None, fallback=None, row_groups=None):
    want = dict(family=family, tile_cols=cols, variant=variant, splits=splits, gn_done=gn_done, fallback=fallback, row_groups=row_groups)
    bad = {k: (getattr(route, k), v) for k, v in want.items() if v is not None and getattr(route, k) != v}
    assert not bad, f"route {route}: (got, want) {bad}"


def report(fam, what, ratio):
    _WORST[fam] = max(_WORST.get(fam, 0.0), ratio)
    print(f"RATIO {fam} {what}: {ratio:.3f} (worst {fam} so far {_WORST[fam]:.3f})")
    assert ratio <= 1.0, (what, ratio)


class knobs:
    def __init__(self, pairs):
        self.pairs = pairs

    def __enter__(self):
        for k, v in self.pairs:
            ops.set_tuning(k, v)

    def __exit__(self, *a):
        ops.reset_tuning()


# ---- 3x3 convs: generic, stride 2 / upsample, split-K, halo, loader-wave ------------------------------------------------------------------------------------------
def run_conv_case(case):
    Ho, Wo = case.out_hw
    for family in ("exact", "random"):
        d = case.inputs(family)
        ref, S = case.reference(d)
        exact = family == "exact"
        if exact:
            R.check_exact(ref)
        obuf, out = guarded(case.B, Ho, Wo, case.N)
        sbuf, st = guarded(case.B, Ho * Wo // 64, case.N // 2, 2, dtype=F32) if case.gn else (None, None)
        x0, x1, wp, bias, temb, res = dev(d["x0"]), dev(d["x1"]), R.pack(d["w"]).to(DEV), dev(d["bias"]), dev(d["temb"]), dev(d["res"])
        try:
            with knobs(case.knobs):
                if case.api == "conv_down":
                    ops.conv_down(x0, wp, bias, out=out)
                else:
                    ops.conv2d(x0, wp, bias, x1=x1, taps=case.taps, stride=case.stride, upsample=case.up, temb=temb, res=res, splitk=case.splitk, gn_stats=case.gn,
                               out=out, st=st)
                route = ops.igemm_last_route()
        finally:
            ops.reset_tuning()
        torch.cuda.synchronize()
        route_is(route, case.family, case.cols, case.variant, case.splits, case.gn_done, case.fallback)
        assert margins_intact(obuf) and (sbuf is None or margins_intact(sbuf)), case
        got = out.cpu()
        if exact:
            assert same_bits(got, ref.to(F16)), (case, "exact family", int((got.double() != ref).sum()), "elements differ")
        else:
            g = R.gfac(case.taps * case.cin, case.addends, route.splits)
            report(case.family, f"{case}", R.ratio(got, ref, R.bound(ref, S, g)))
        if case.gn:
            msg = R.gn_check(st.cpu(), got, exact)
            assert msg is None, (case, family, msg)


@pytest.mark.parametrize("case", R.GENERIC_CASES, ids=repr)
def test_generic_conv3(case):
    """igemm_kernel<., CONV3>: 1-pixel and 1-row images (every tap but the centre padding), M < 16, M = 129, non-square images, both concat orders, every epilogue form"""
    run_conv_case(case)


@pytest.mark.parametrize("case", R.STRIDE_UP_CASES, ids=repr)
def test_generic_conv3_stride_2_upsample_and_pad_after_only(case):
    run_conv_case(case)


@pytest.mark.parametrize("case", R.GENERIC_SPLITK_CASES, ids=repr)
def test_generic_conv3_split_k(case):
    """2, 4 and 8 splits told apart by the record; both reduce kernels"""
    run_conv_case(case)


@pytest.mark.parametrize("case", R.HALO_CASES, ids=repr)
def test_halo_conv3(case):
    """conv3_halo_kernel: four / two images per tile with ragged last tiles, TW = 8 with two patches per image, non-square images and fused upsamples, the wide
    tiles, the split over channel chunks"""
    run_conv_case(case)


@pytest.mark.parametrize("case", R.LW_CASES, ids=repr)
def test_loader_wave_conv3(case):
    """conv3_lw_kernel: every reachable ConvLwVariant by its number"""
    run_conv_case(case)


def test_halo_and_loader_wave_kernels_are_bit_identical_on_random_data():
    """same tile, same k order: conv3_lw and conv3_halo must agree bit for bit (the exact family cannot tell an accumulation-order change)"""
    case = R.ConvCase("ident", 5, 8, 8, 128, 160, temb="B", res=True, splitk=False)
    d = case.inputs("random")
    args = (dev(d["x0"]), R.pack(d["w"]).to(DEV), dev(d["bias"]))
    outs = []
    try:
        for kn, fam in ((R.HALO, "halo"), (R.LW, "conv3_lw"), (R.LWP, "conv3_lw")):
            with knobs(kn):
                outs.append(ops.conv2d(*args, temb=dev(d["temb"]), res=dev(d["res"]), splitk=False))
                route_is(ops.igemm_last_route(), fam, 160)
    finally:
        ops.reset_tuning()
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])


# ---- sub-pixel upsample ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hi,Wi,cin,N,idx", R.SUB_CASES)
def test_sub_pixel_upsample(B, Hi, Wi, cin, N, idx):
    """cs_op_conv_up_sub against the fused-upsample reference: exact family bit for bit, random family within the rule + the rounding of the summed weights;
    statistics by the totals rule (SubRows is phase-major)"""
    case = R.ConvCase(f"sub{B}x{Hi}x{Wi}_c{cin}_n{N}", B, Hi, Wi, cin, N, up=True, gn=True)
    for family in ("exact", "random"):
        d = case.inputs(family)
        ref, S = case.reference(d)
        exact = family == "exact"
        if exact:
            R.check_exact(ref)
        wp = R.pack(d["w"])
        ws = ops.conv_up_fold_pack(wp.reshape(N, -1))
        obuf, out = guarded(B, 2 * Hi, 2 * Wi, N)
        sbuf, st = guarded(B, 4 * Hi * Wi // 64, N // 2, 2, dtype=F32)
        try:
            ops.conv_up_sub(dev(d["x0"]), wp.to(DEV), ws.to(DEV), dev(d["bias"]), gn_stats=True, out=out, st=st)
            route = ops.igemm_last_route()
        finally:
            ops.reset_tuning()
        torch.cuda.synchronize()
        route_is(route, "sub_pixel", 128 if idx == 2 else 160, idx, 1, 1, 0)
        assert margins_intact(obuf, sbuf)
        got = out.cpu()
        if exact:
            assert same_bits(got, ref.to(F16))
        else:
            sconv = S - d["bias"].double().abs()
            report("sub_pixel", f"{case}", R.ratio(got, ref, R.bound(ref, S, R.gfac(9 * cin, 1), extra=(2.0 ** -11 + 2.0 ** -22) * sconv)))
        msg = R.gn_check(st.cpu(), got, exact)
        assert msg is None, (case, family, msg)


# ---- 1x1 and linear -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.LINEAR_ROUTES))
def test_linear_routes_at_every_row_edge(name):
    """M = 1 .. 513 (ragged row tiles of 128 and 256, full FAST waves beside a ragged one at 321) x K = 64, 128, 320; bias / residual / nothing rotating"""
    kn, N, fam, cols, variant = R.LINEAR_ROUTES[name]
    i = 0
    for K in R.LINEAR_K:
        for M in R.LINEAR_M:
            for family in ("exact", "random"):
                f = R.Family(family, 1000 * K + M)
                x, w = f.x((M, K), K), f.w((N, K), K)
                bias = f.vec((N,)) if i % 3 != 2 else None
                res = f.res((M, N)) if i % 3 == 1 else None
                o = R.linear_fp64(x, None, w, bias, res, None)
                obuf, out = guarded(M, N)
                try:
                    with knobs(kn):
                        ops.linear(dev(x), dev(w), dev(bias), res=dev(res), out=out)
                        route = ops.igemm_last_route()
                finally:
                    ops.reset_tuning()
                torch.cuda.synchronize()
                route_is(route, fam, cols, variant, 1)
                assert margins_intact(obuf), (name, M, K)
                if family == "exact":
                    R.check_exact(o.ref)
                    assert same_bits(out, o.ref.to(F16)), (name, M, K, int((out.cpu().double() != o.ref).sum()))
                else:
                    g = R.gfac(K, int(bias is not None) + int(res is not None))
                    report(fam, f"{name} M {M} K {K}", R.ratio(out.cpu(), o.ref, R.bound(o.ref, o.S, g)))
            i += 1


@pytest.mark.parametrize("name", list(R.LINEAR_ROUTES))
def test_conv1x1_concat_and_temb_through_every_route(name):
    """the channel concat of a 1x1 (both orders), time embedding per sample, residual; B x H x W rows with a ragged last tile"""
    kn, N, fam, cols, variant = R.LINEAR_ROUTES[name]
    for j, (c0, c1) in enumerate([(64, 128), (128, 64), (64, 0)]):
        case = R.ConvCase(f"{name}_1x1_{c0}+{c1}", 3, 5, 9, c0, N, c1=c1, taps=1, temb="B" if j != 1 else 0, res=j != 0)
        for family in ("exact", "random"):
            d = case.inputs(family)
            ref, S = case.reference(d)
            obuf, out = guarded(3, 5, 9, N)
            try:
                with knobs(kn):
                    ops.conv2d(dev(d["x0"]), R.pack(d["w"]).to(DEV), dev(d["bias"]), x1=dev(d["x1"]), taps=1, temb=dev(d["temb"]), res=dev(d["res"]), out=out)
                    route = ops.igemm_last_route()
            finally:
                ops.reset_tuning()
            torch.cuda.synchronize()
            route_is(route, fam, cols, variant, 1)
            assert margins_intact(obuf)
            if family == "exact":
                R.check_exact(ref)
                assert same_bits(out, ref.to(F16)), case
            else:
                report(fam, f"{case}", R.ratio(out.cpu(), ref, R.bound(ref, S, R.gfac(case.cin, case.addends))))


@pytest.mark.parametrize("kn,N,fam,cols,variant", R.GEGLU_ROUTES)
def test_geglu_on_each_route_that_has_it(kn, N, fam, cols, variant):
    """value x erf-GELU(gate) on packed weights.  No bit-exact family exists here (the GELU of an integer is no fp16 number): the exact family's inputs make value and
    gate exact integers, which leaves the polynomial's own error and the final rounding in the rule; the random family adds the accumulation terms.  N = 320 under
    the default knobs: the 320-column kernels take it whatever the tile count (the generic tiles have no GEGLU form for N % 128 != 0)."""
    for M in (1, 65, 257, 321):
        for K in (64, 320):
            for family in ("exact", "random"):
                f = R.Family(family, 31 * M + K)
                x, w, b = f.x((M, K), K), f.w((N, K), K), f.vec((N,))
                wp, bp = ops.geglu_pack(w, b)
                o = R.linear_fp64(x, None, wp, bp, None, None, geglu=True)
                obuf, out = guarded(M, N // 2)
                try:
                    with knobs(kn):
                        ops.linear(dev(x), wp.to(DEV), bp.to(DEV), geglu=True, out=out)
                        route = ops.igemm_last_route()
                finally:
                    ops.reset_tuning()
                torch.cuda.synchronize()
                route_is(route, fam, cols, variant, 1)
                assert margins_intact(obuf), (N, M, K)
                report(fam + "_geglu", f"N {N} M {M} K {K} {family}", R.ratio(out.cpu(), o.ref, R.geglu_bound(o, R.gfac(K, 1))))


# route name -> (knobs, N, family, cols, {form: variant}, row-statistics groups)
X2_ROUTES = {
    "generic128": ((("gemm_big", 0),), 256, "generic", 128, dict(plain=0, stats=2, epi2=0), 4),
    "generic160": ((("gemm_big", 0),), 320, "generic", 160, dict(plain=0, stats=2, epi2=0), 4),
    "w8": ((("gemm_big", 2), ("gemm_w8", 1)), 320, "gemm_w8", 320, dict(plain=0, stats=4, epi2=7), 2),
    "lw": ((("gemm_big", 3), ("gemm_lw", 1)), 160, "gemm_lw", 160, dict(plain=0, stats=2, epi2=5), 1),
}


@pytest.mark.parametrize("name", list(X2_ROUTES))
def test_split_residual_forms_epi_fast_on_and_off(name):
    """linear_x2 / conv2d_x2(1x1): res, res + res_lo, out_lo, the split A operand, no lo plane out, row statistics; epi_fast 0 and 3 bit-identical"""
    kn, N, fam, cols, variants, groups = X2_ROUTES[name]
    forms = [dict(res=True, lo_in=False, lo_out=False, a_lo=False, stats=False), dict(res=True, lo_in=True, lo_out=True, a_lo=False, stats=False),
             dict(res=False, lo_in=False, lo_out=True, a_lo=False, stats=False), dict(res=True, lo_in=True, lo_out=True, a_lo=True, stats=False),
             dict(res=True, lo_in=True, lo_out=False, a_lo=False, stats=False), dict(res=True, lo_in=True, lo_out=True, a_lo=False, stats=True)]
    K = 128
    for M in (65, 321):
        for fi, fm in enumerate(forms):
            for family in ("exact", "random"):
                f = R.Family(family, 100 * M + fi)
                x, w, bias = f.x((M, K), K), f.w((N, K), K), f.vec((N,))
                x_lo = f.lo(x) if fm["a_lo"] else None
                res = f.res((M, N)) if fm["res"] else None
                res_lo = f.lo(res) if fm["lo_in"] else None
                o = R.linear_fp64(x, x_lo, w, bias, res, res_lo)
                exact = family == "exact"
                if exact:
                    R.check_exact(o.ref, quarters=True)
                prev = None
                for ef in (0, 3):
                    obuf, out = guarded(M, N)
                    lbuf, out_lo = guarded(M, N) if fm["lo_out"] else (None, None)
                    sbuf, st = guarded(M, N // 64, 2, dtype=F32) if fm["stats"] else (None, None)
                    try:
                        with knobs(kn + (("epi_fast", ef),)):
                            if fi % 2 == 0:
                                r = ops.linear_x2(dev(x), dev(w), dev(bias), res=dev(res), res_lo=dev(res_lo), splitk=False, want_lo=fm["lo_out"], x_lo=dev(x_lo),
                                                  row_stats=fm["stats"], out=out, out_lo=out_lo, st=st)
                            else:
                                r = ops.conv2d_x2(dev(x).view(1, M, 1, K), dev(w), dev(bias), taps=1, res=dev(res).view(1, M, 1, N), res_lo=dev(res_lo).view(1, M, 1, N),
                                                  splitk=False, want_lo=fm["lo_out"], x0_lo=dev(x_lo).view(1, M, 1, K) if x_lo is not None else None, row_stats=fm["stats"],
                                                  out=out.view(1, M, 1, N), out_lo=out_lo.view(1, M, 1, N) if out_lo is not None else None, st=st)
                            route = ops.igemm_last_route()
                    finally:
                        ops.reset_tuning()
                    torch.cuda.synchronize()
                    epi2 = fm["res"] and fm["lo_in"] and not fm["lo_out"] and ef == 3
                    route_is(route, fam, cols, variants["stats"] if fm["stats"] else variants["epi2"] if epi2 else variants["plain"], 1,
                             row_groups=(N // (cols // 2) if fam == "generic" else N // 160) if fm["stats"] else None, fallback=0)
                    assert margins_intact(*[b for b in (obuf, lbuf, sbuf) if b is not None]), (name, M, fm)
                    hi = out.cpu()
                    lo = out_lo.cpu() if out_lo is not None else None
                    what = f"{name} M {M} form {fi} epi_fast {ef}"
                    if exact:
                        assert same_bits(hi, R.rnd16(o.ref).to(F16)), what
                        if lo is not None:
                            assert same_bits(lo, (o.ref - R.rnd16(o.ref)).to(F16)), what
                    else:
                        A = 1 + int(fm["res"]) + int(fm["lo_in"])
                        g = R.gfac(K * (2 if fm["a_lo"] else 1), A)
                        report(fam + "_x2", what, R.ratio(hi, o.ref, R.bound(o.ref, o.S, g)))
                        if lo is not None:
                            report(fam + "_x2", what + " hi + lo", R.split_ratio(hi, lo, o.ref, o.S, g))
                    if fm["stats"]:
                        Gr = r[2][1]
                        assert Gr == route.row_groups
                        flat = st.cpu().reshape(-1)
                        msg = R.row_check(flat, hi.double() + lo.double(), Gr, exact)
                        assert msg is None, (what, msg)
                        assert bool(torch.isnan(flat[M * Gr * 2:]).all())                     # nothing behind the [M][G][2] block
                    cur = (bits(hi), bits(lo) if lo is not None else None, bits(st) if st is not None else None)
                    if prev is not None:
                        assert all(a is None or torch.equal(a, b) for a, b in zip(prev, cur)), (what, "epi_fast 0 and 3 differ")
                    prev = cur


CONV3_X2 = [("generic", R.HALO0, "generic", 160, 32, 1, (3, 5, 7)), ("halo", R.HALO, "halo", 160, 0, 1, (5, 8, 8)), ("lw_fast", R.LW, "conv3_lw", 160, 0, 1, (2, 16, 16)),
            ("lw_fast8", R.LW, "conv3_lw", 160, 10, 1, (5, 8, 8)), ("lw_fast128", R.LW, "conv3_lw", 128, 6, 1, (1, 16, 32)), ("lw_split", R.LW, "conv3_lw", 160, 10, 2, (1, 8, 8))]


@pytest.mark.parametrize("name,kn,fam,N,variant,splits,geo", CONV3_X2)
def test_conv3_split_residual_planes(name, kn, fam, N, variant, splits, geo):
    """conv2d_x2 on a 3x3: res + res_lo in, hi + lo out (the FAST 2 epilogue of conv3_lw beside a ragged last tile, the generic code elsewhere, the reduce kernel
    behind a split); epi_fast 0 and 3 bit-identical"""
    B, H, W = geo
    cin = 128
    case = R.ConvCase(f"x2_{name}", B, H, W, cin, N, res=True, splitk=splits > 1)
    for family in ("exact", "random"):
        d = case.inputs(family)
        res_lo = R.Family(family, 5).lo(d["res"])
        ref, S = case.reference(d, res_lo)
        if family == "exact":
            R.check_exact(ref, quarters=True)
        prev = None
        for ef in (0, 3):
            obuf, out = guarded(B, H, W, N)
            lbuf, out_lo = guarded(B, H, W, N)
            try:
                with knobs(kn + (("epi_fast", ef),)):
                    ops.conv2d_x2(dev(d["x0"]), R.pack(d["w"]).to(DEV), dev(d["bias"]), res=dev(d["res"]), res_lo=dev(res_lo), splitk=splits > 1, out=out, out_lo=out_lo)
                    route = ops.igemm_last_route()
            finally:
                ops.reset_tuning()
            torch.cuda.synchronize()
            route_is(route, fam, N, variant, splits)
            assert margins_intact(obuf, lbuf), (name, ef)
            hi, lo = out.cpu(), out_lo.cpu()
            if family == "exact":
                assert same_bits(hi, R.rnd16(ref).to(F16)) and same_bits(lo, (ref - R.rnd16(ref)).to(F16)), (name, ef)
            else:
                g = R.gfac(9 * cin, 3, splits)
                report(fam + "_x2", f"{case} epi_fast {ef}", max(R.ratio(hi, ref, R.bound(ref, S, g)), R.split_ratio(hi, lo, ref, S, g)))
            cur = (bits(hi), bits(lo))
            assert prev is None or (torch.equal(prev[0], cur[0]) and torch.equal(prev[1], cur[1])), (name, "epi_fast 0 and 3 differ")
            prev = cur


def test_linear_x2_split_k_through_the_reduce_kernel_and_the_row_statistics_pass():
    """K = 1024 on the generic tiles: two splits, splitk_reduce_kernel writes both planes, the row statistics come from row_stats_kernel (G = 1)"""
    M, K, N = 65, 1024, 256
    for family in ("exact", "random"):
        f = R.Family(family, 77)
        x, w, bias, res = f.x((M, K), K), f.w((N, K), K), f.vec((N,)), f.res((M, N))
        res_lo = f.lo(res)
        o = R.linear_fp64(x, None, w, bias, res, res_lo)
        obuf, out = guarded(M, N)
        lbuf, out_lo = guarded(M, N)
        sbuf, st = guarded(M, N // 64, 2, dtype=F32)
        try:
            with knobs((("gemm_big", 0),)):
                _, _, (_, Gr) = ops.linear_x2(dev(x), dev(w), dev(bias), res=dev(res), res_lo=dev(res_lo), splitk=True, row_stats=True, out=out, out_lo=out_lo, st=st)
                route = ops.igemm_last_route()
        finally:
            ops.reset_tuning()
        torch.cuda.synchronize()
        route_is(route, "generic", 128, 0, 2, row_groups=0, fallback=2)
        assert Gr == 1 and margins_intact(obuf, lbuf, sbuf)
        hi, lo = out.cpu(), out_lo.cpu()
        if family == "exact":
            R.check_exact(o.ref, quarters=True)
            assert same_bits(hi, R.rnd16(o.ref).to(F16)) and same_bits(lo, (o.ref - R.rnd16(o.ref)).to(F16))
        else:
            g = R.gfac(K, 3, 2)
            report("generic_x2", "split-K 2", max(R.ratio(hi, o.ref, R.bound(o.ref, o.S, g)), R.split_ratio(hi, lo, o.ref, o.S, g)))
        flat = st.cpu().reshape(-1)
        msg = R.row_check(flat, hi.double() + lo.double(), 1, family == "exact")
        assert msg is None, msg
        assert bool(torch.isnan(flat[M * 2:]).all())


def test_row_stats_op():
    for M, Cc in ((1, 64), (5, 320), (131, 1280)):
        for family in ("exact", "random"):
            f = R.Family(family, M)
            x = f.res((M, Cc))
            x_lo = f.lo(x)
            for lo in (None, x_lo):
                sbuf, st = guarded(M, 1, 2, dtype=F32)
                xd, lod = dev(x), dev(lo)
                L.check(L.lib().cs_op_row_stats(L.ptr(xd), L.ptr(lod), M, Cc, L.ptr(st), L.stream_ptr(DEV)))
                torch.cuda.synchronize()
                assert margins_intact(sbuf)
                msg = R.row_check(st.cpu(), x.double() + (lo.double() if lo is not None else 0.0), 1, family == "exact")
                assert msg is None, (M, Cc, family, msg)


# ---- conv_out (csrc/misc.hip) ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,cin,cout", R.CONV_OUT_CASES)
def test_conv_out_both_modes(B, H, W, cin, cout):
    case = R.ConvCase(f"conv_out{B}x{H}x{W}_c{cin}_o{cout}", B, H, W, cin, cout)
    for family in ("exact", "random"):
        d = case.inputs(family)
        ref, S = case.reference(d)
        ref, S = ref.permute(0, 3, 1, 2).contiguous(), S.permute(0, 3, 1, 2).contiguous()
        if family == "exact":
            R.check_exact(ref)
        for mode in (1, 0):
            obuf, out = guarded(B, cout, H, W)
            try:
                with knobs((("conv_out_mfma", mode),)):
                    ops.conv_out(dev(d["x0"]), R.pack(d["w"]).reshape(cout, 9, cin).to(DEV), dev(d["bias"]), out=out)
            finally:
                ops.reset_tuning()
            torch.cuda.synchronize()
            assert margins_intact(obuf), (case, mode)
            if family == "exact":
                assert same_bits(out, ref.to(F16)), (case, mode, int((out.cpu().double() != ref).sum()))
            else:
                report("conv_out", f"{case} mfma {mode}", R.ratio(out.cpu(), ref, R.bound(ref, S, R.gfac(9 * cin, 1))))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def _raw_conv2d(x0, c0, B, Hi, Wi, taps, stride, w, N, out, entry="cs_op_conv2d", x0_lo=None):
    lib, st = L.lib(), L.stream_ptr(DEV)
    if entry == "cs_op_conv2d":
        return lib.cs_op_conv2d(L.ptr(x0), c0, None, 0, B, Hi, Wi, taps, stride, 0, L.ptr(w), None, N, None, 0, None, L.ptr(out), None, 0, st)
    if entry == "cs_op_conv2d_gn":
        gst = torch.zeros(B * 64 * N, dtype=F32, device=DEV)
        return lib.cs_op_conv2d_gn(L.ptr(x0), c0, None, 0, B, Hi, Wi, taps, stride, 0, L.ptr(w), None, N, None, 0, None, L.ptr(out), None, 0, L.ptr(gst), st)
    return lib.cs_op_conv2d_x2(L.ptr(x0), L.ptr(x0_lo), c0, None, None, 0, B, Hi, Wi, taps, stride, 0, L.ptr(w), None, N, None, 0, None, None, L.ptr(out), None,
                               None, None, None, 0, st)


def test_refusals_leave_the_output_untouched():
    x = torch.zeros(1, 9, 9, 64, dtype=F16, device=DEV)
    w = torch.zeros(640, 9 * 64, dtype=F16, device=DEV)
    # (what, call, the code the source gives, refused inside the launcher: the route record then says that nothing was launched)
    cases = [("N = 192", lambda o: _raw_conv2d(x, 64, 1, 8, 8, 9, 1, w, 192, o), CS_E_SHAPE, True),
             ("c0 = 32", lambda o: _raw_conv2d(x, 32, 1, 8, 8, 9, 1, w, 128, o), CS_E_SHAPE, True),
             ("taps 1 with stride 2", lambda o: _raw_conv2d(x, 64, 1, 8, 8, 1, 2, w, 128, o), CS_E_ARG, True),
             ("a0_lo on a 3x3", lambda o: _raw_conv2d(x, 64, 1, 8, 8, 9, 1, w, 128, o, "cs_op_conv2d_x2", x0_lo=x), CS_E_ARG, True),
             ("GEGLU at N = 384", lambda o: L.lib().cs_op_linear(L.ptr(x), 64, 64, L.ptr(w), None, 384, None, L.ptr(o), 1, L.stream_ptr(DEV)), CS_E_SHAPE, True),
             ("stride 2, 9 x 8", lambda o: _raw_conv2d(x, 64, 1, 9, 8, 9, 2, w, 128, o), CS_E_SHAPE, False),
             ("stride 2, 8 x 9", lambda o: _raw_conv2d(x, 64, 1, 8, 9, 9, 2, w, 128, o), CS_E_SHAPE, False),
             ("stride 2, 9 x 9, conv2d_gn", lambda o: _raw_conv2d(x, 64, 1, 9, 9, 9, 2, w, 128, o, "cs_op_conv2d_gn"), CS_E_SHAPE, False),
             ("stride 2, 7 x 8, conv2d_x2", lambda o: _raw_conv2d(x, 64, 1, 7, 8, 9, 2, w, 128, o, "cs_op_conv2d_x2"), CS_E_SHAPE, False)]
    for what, call, code, in_launcher in cases:
        obuf, _ = guarded(1, 8, 8, 640)
        rc = call(obuf[G:])
        torch.cuda.synchronize()
        assert rc == code, (what, rc, L.lib().cs_last_error().decode())
        assert untouched(obuf), what
        assert not in_launcher or ops.igemm_last_route().family == "none", what
    # GEGLU with N % 128 != 0 has no kernel on the generic tiles: refused when the 320-column kernels are switched off, and routed to them otherwise
    try:
        with knobs((("gemm_big", 0),)):
            obuf, _ = guarded(64, 160)
            rc = L.lib().cs_op_linear(L.ptr(x), 64, 64, L.ptr(w), None, 320, None, L.ptr(obuf[G:]), 1, L.stream_ptr(DEV))
            torch.cuda.synchronize()
            assert rc == CS_E_SHAPE and untouched(obuf) and ops.igemm_last_route().family == "none"
    finally:
        ops.reset_tuning()


def test_empty_batch_launches_nothing_and_reports_one_row_group():
    """B = 0 with row statistics asked for: CS_OK, no kernel and no statistics pass (the record stays at "none", nothing is written), and the layout returned is the
    statistics pass's one group (IgemmArgs::row_stats, ops.h)"""
    import ctypes
    x = torch.zeros(1, 8, 8, 64, dtype=F16, device=DEV)
    w = torch.zeros(128, 64, dtype=F16, device=DEV)
    obuf, _ = guarded(1, 8, 8, 128)
    sbuf, _ = guarded(64, 2, 2, dtype=F32)
    groups = ctypes.c_int(-7)
    rc = L.lib().cs_op_conv2d_x2(L.ptr(x), None, 64, None, None, 0, 0, 8, 8, 1, 1, 0, L.ptr(w), None, 128, None, 0, None, None, L.ptr(obuf[G:]), None,
                                 L.ptr(sbuf[G:]), ctypes.byref(groups), None, 0, L.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and groups.value == 1 and ops.igemm_last_route().family == "none"
    assert untouched(obuf) and untouched(sbuf)


def test_conv_down_floors_odd_sizes_by_definition():
    """pad (0, 1, 0, 1), stride 2: floor(H / 2) rows IS the conv's size (tests/igemm_ref.py conv_fp64 with pad_after_only); the pad-1 entry points refuse odd sizes
    instead of dropping the last row (test_refusals_leave_the_output_untouched)"""
    case = [c for c in R.STRIDE_UP_CASES if c.name == "down_5x7"][0]
    assert case.out_hw == (2, 3)
    run_conv_case(case)
