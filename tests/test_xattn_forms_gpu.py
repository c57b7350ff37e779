"""The six instantiations of the fused cross-attention block (csrc/xattn.hip: xattn_block_kernel<0|1|2> on 128-row tiles, xattn64_kernel<0|1|2> on 64-row tiles; 0 plain
fp16 stream, 1 split-fp16, 2 hi + e5m2 lo8; the two tile sizes are two kernel bodies over one set of per-wave phase functions and differ in the wave grid, the
weight-stage geometry of the GEMMs and V as one tile or two half tiles) through the C ABI -- cs_op_xattn_block, cs_op_xattn_block_x2, cs_op_xattn_block_lo8 -- against a float64 reference of the
same rounded inputs, per (row, head) of the attention output and per row of the branch, at every mask boundary of the key layout, on exact families whose planes are
known bit for bit, across the forms bit for bit, on the row statistics, and at the launcher's rejections.  tests/xattn_ref.py holds the references and the families.

Every buffer the kernel addresses is an interior view of a larger allocation whose margins (128 rows = one whole tile on either side) hold the byte 0x7F -- a NaN in
fp16 (0x7F7F) and in e5m2 -- and so do the output views before the call.  kv is followed by NaN rows right behind the last sample's Nk keys.  Every run asserts that all
margins kept their bytes, that the inputs did (out of place), and that every addressed output element was written and is finite.

Assertions:
  1 / 2  the branch is read off the split form's output, out + out_lo - (h + h_lo) (with Wo = I, bo = 0 it is the attention output O itself).  Per (row, head) of O, and
         per row of the branch with random Wo, bo:  err - recovery term <= 2 x (the emulator's worst on the same inputs) + one fp16 ulp,  err = relative L2 against fp64.
         The emulator carries every rounding to fp16 the kernel has; what it lacks (fp32 summation order, the last bit of v_exp_f32 and rsqrtf) is two orders below fp16
         epsilon.  The factor is that argument, not a fit.  Family "last" walks Nk over every boundary of the key layout (a lane holds keys kt*16 + 4g + r).
  3      selector (swept so that the selected key of every head visits all 80 positions: both V halves of the 64-row kernel, the zero rows of the V tile, the half-empty
         third P fragment), nk1 and qround: out, out_lo and the lo8 bytes equal torch's own split of the exact f, bit for bit, in all six instantiations.
         qround is decided by the second rounding of q.  3b, denom: O is a correctly rounded fp16 of V[j*] / l up to the fp32 error of l, and its mean signed error is zero
         up to that error and 6 sigma of the rounding noise -- a denominator from the ROUNDED P is 4e-4 off with one sign.
  4      bit for bit at every shape: tile 64 == tile 128; plain == the split form's hi plane at h_lo = 0; the lo8 form's hi plane == the split form's on the same
         represented stream; in place == out of place; row_stats requested or not.  hi is A nearest fp16 of hi + lo; lo8 against the split form's lo, see _lo8_close.
  5      row_stats = (sum f, sum f^2) against float64 sums of the split form's hi + lo: |error| <= (n + 1) 2^-24 sum |terms|, n = 320 (any order of n fp32 additions, and one
         more rounding for the product).
  6      the launcher's codes, each with the output buffers untouched; M = 0 is CS_OK and writes nothing.

The emulator's own worst figures against fp64 (tests/test_xattn_ref.py, B = 2, HW = 128; (row, head) of O / row of the branch):
             Nk = 13               Nk = 77               Nk = 80
  gauss      9.1e-4 / 5.6e-4       1.24e-3 / 6.9e-4      1.21e-3 / 6.4e-4
  dc         1.04e-3 / 6.4e-4      1.12e-3 / 6.8e-4      9.8e-4 / 6.4e-4
  peaky      5.6e-3 / 1.9e-3       5.8e-3 / 2.1e-3       4.6e-3 / 1.9e-3
  last       8.0e-3 / 3.1e-3       8.3e-3 / 3.4e-3       8.5e-3 / 4.6e-3
  selector   6e-88 / 0             5e-88 / 0             6e-88 / 0             (fp64's P is one-hot to 2^-292; the branch is exact)          nk1: 0 / 0
  peaky and last are fp16-class too: one key carries the row, and the rounding of q to fp16 moves competing scores of size 2^5 by 2^-11 of their size.

What the kernels measured on an MI355X (pytest -s; err - recovery term, worst over the cases below; next to it the emulator's worst over the SAME cases, and the
largest kernel / bound ratio of any single case):
                          tile 64                                   tile 128
  O (row, head)  gauss    1.139e-3  (emulator 1.140e-3; 0.35)       1.045e-3  (1.048e-3; 0.34)
                 dc       1.103e-3  (1.152e-3; 0.34)                1.064e-3  (1.102e-3; 0.34)
                 peaky    5.975e-3  (5.976e-3; 0.46)                5.631e-3  (5.632e-3; 0.46)
                 last     1.187e-2  (1.188e-2; 0.48)                1.187e-2  (1.188e-2; 0.48)          (all 20 Nk values; the worst is Nk = 79)
  branch row     gauss    6.885e-4  (6.897e-4; 0.29)                6.687e-4  (6.704e-4; 0.29)
                 dc       6.983e-4  (7.571e-4; 0.28)                6.983e-4  (7.571e-4; 0.28)
                 peaky    2.069e-3  (2.070e-3; 0.40)                2.069e-3  (2.070e-3; 0.40)
                 last     5.553e-3  (5.554e-3; 0.46)                5.553e-3  (5.554e-3; 0.46)
  (tile 64 runs the HW = 64 and 192 shapes on top of tile 128's.)  The kernel sits on the emulator to three digits and more: the bound's factor 2 is unused.
  The recovery term is at most 5.1e-6 of a (row, head) norm (dc: 1.1e-4).
  Exact families: all 12 selector sweeps (27 or 40 launches each) and all 35 (family, shape) cases equal the closed form bit for bit in every form and tile; the lo
  planes of the h_lo-grid variants are 92 - 93 % non-zero.  denom: no element past half an fp16 ulp + the fp32 noise; |mean signed error| 1.5e-6 .. 2.1e-5 against bounds of
  6.0e-5 .. 1.0e-4 (the emulator with the rounded-P denominator: 3.9e-4 .. 4.2e-4).
  Form identities: held bit for bit at all five shapes on both families (tile 64 == 128, plain == split hi at h_lo = 0, lo8 hi == split hi, in place, row_stats on / off).
  Row statistics: at most 0.012 of the summation bound.
"""
import pytest
import torch

from consolver_amd import _lib as L
from consolver_amd import ops
from tests import xattn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0x7F                 # every byte of a guarded allocation: NaN as fp16 (0x7F7F) and as e5m2
G = 128                     # margin rows on either side of every view: one whole tile
PLAIN, SPLIT, LO8 = 0, 1, 2
FORM_NAME = {PLAIN: "plain", SPLIT: "split", LO8: "lo8"}
CS_OK, CS_E_ARG, CS_E_SHAPE, CS_E_UNSUPPORTED = 0, -1, -2, -6
C = R.C


class Guarded:
    """[rows, cols] of `dtype` inside an allocation with G rows of FILL bytes before and after it"""

    def __init__(self, rows, cols, dtype, data=None):
        size = torch.empty(0, dtype=dtype).element_size()
        self.rows = rows
        self.whole = torch.full((rows + 2 * G, cols * size), FILL, dtype=torch.uint8, device=DEV)
        self.view = self.whole[G:G + rows].view(dtype)
        if data is not None:
            self.view.copy_(data.reshape(rows, cols))

    def margins_intact(self):
        return bool((self.whole[:G] == FILL).all()) and bool((self.whole[G + self.rows:] == FILL).all())

    def untouched(self):
        return bool((self.whole == FILL).all())

    def cpu(self):
        return self.view.cpu()


class Result:
    __slots__ = ("hi", "lo", "stats", "rc")


def _tiles(HW):
    return (64, 128) if HW % 128 == 0 else (64,)


def run(x, form, tile, inplace=False, stats=False, expect=CS_OK, plain_entry=False, M=None, HW=None, Nk=None, Cc=C, heads=R.NH, null=None, drop=None):
    """one call of the form's entry point on guarded views.  form LO8 sends x.h_lo through torch's e5m2 conversion (the callers pass e5m2 values where they compare forms).
    expect != CS_OK: the code is asserted and every output allocation must be untouched.  M / HW / Nk / Cc / heads override what is PASSED (the buffers keep x's sizes);
    null names an argument passed as NULL; drop = "h_lo" / "out_lo" passes that one plane as NULL."""
    ops.set_tuning("xattn_tile", tile)
    rows = x.M
    h = Guarded(rows, C, torch.float16, x.h)
    lo_dtype = torch.uint8 if form == LO8 else torch.float16
    h_lo = None
    if form != PLAIN:
        h_lo = Guarded(rows, C, lo_dtype, R.lo8_of(x.h_lo) if form == LO8 else x.h_lo)
    kv = Guarded(x.B * x.Nk, 2 * C, torch.float16, x.kv)
    w = {k: getattr(x, k).to(DEV).contiguous() for k in ("gamma", "beta", "wq", "wo", "bo")}
    out = h if inplace else Guarded(rows, C, torch.float16)
    out_lo = None if form == PLAIN else h_lo if inplace else Guarded(rows, C, lo_dtype)
    rs = Guarded(rows, 2, torch.float32) if stats else None
    p = {"h": h.view, "h_lo": h_lo.view if h_lo else None, "out": out.view, "out_lo": out_lo.view if out_lo else None, "kv": kv.view, **w}
    if null:
        p[null] = None
    if drop:
        p[drop] = None
    st = L.stream_ptr(torch.device(DEV))
    a = (x.Nk if Nk is None else Nk, L.ptr(p["wo"]), L.ptr(p["bo"]), rows if M is None else M, x.HW if HW is None else HW, Cc, heads, R.SCALE)
    if plain_entry:
        assert form == PLAIN and not stats
        rc = L.lib().cs_op_xattn_block(L.ptr(p["h"]), L.ptr(p["gamma"]), L.ptr(p["beta"]), R.EPS, L.ptr(p["wq"]), L.ptr(p["kv"]), *a, L.ptr(p["out"]), st)
    else:
        fn = L.lib().cs_op_xattn_block_lo8 if form == LO8 else L.lib().cs_op_xattn_block_x2
        rc = fn(L.ptr(p["h"]), L.ptr(p["h_lo"]), L.ptr(p["gamma"]), L.ptr(p["beta"]), R.EPS, L.ptr(p["wq"]), L.ptr(p["kv"]), *a, L.ptr(p["out"]), L.ptr(p["out_lo"]),
                L.ptr(rs.view if rs else None), st)
    torch.cuda.synchronize()
    guards = [g for g in (h, h_lo, kv, out, out_lo, rs) if g is not None]
    assert all(g.margins_intact() for g in guards), "a margin was written"
    r = Result()
    r.rc, r.hi, r.lo, r.stats = rc, None, None, None
    if expect != CS_OK or (M is not None and M <= 0):
        assert rc == expect, (rc, expect, L.lib().cs_last_error().decode())
        assert all(g.untouched() for g in (out, out_lo, rs) if g is not None and not inplace), "a rejected call wrote to its outputs"
        return r
    assert rc == CS_OK, (rc, L.lib().cs_last_error().decode())
    assert torch.equal(kv.cpu(), x.kv.reshape(-1, 2 * C))
    if not inplace:
        assert torch.equal(h.cpu(), x.h)
        assert h_lo is None or torch.equal(h_lo.cpu(), R.lo8_of(x.h_lo) if form == LO8 else x.h_lo)
    r.hi = out.cpu()
    assert torch.isfinite(r.hi).all(), "an output element was not written"
    if out_lo is not None:
        r.lo = out_lo.cpu()
        assert torch.isfinite(R.lo8_value(r.lo) if form == LO8 else r.lo).all(), "a lo element was not written"
    if rs is not None:
        r.stats = rs.cpu()
        assert bool((r.stats.view(torch.int32) != 0x7F7F7F7F).all()) and torch.isfinite(r.stats).all(), "a row statistic was not written"
    return r


def reject_tile_128(x, form=SPLIT):
    """HW % 128 != 0 under xattn_tile = 128 is a rejection, asserted where the other shapes run the 128-row kernel"""
    if x.HW % 128:
        run(x, form, 128, expect=CS_E_SHAPE)


# ---- 1 / 2. attention per (row, head), branch per row ----------------------------------------------------------------------------------------------------------------
LAST = [(2, 128, nk) for nk in R.NK_ALL] + [(1, 64, 77), (3, 64, 5), (1, 192, 80), (2, 256, 33), (3, 64, 80), (1, 192, 17), (2, 256, 64)]
OTHER = [(2, 128, 13), (3, 64, 77), (2, 256, 80), (1, 192, 16), (1, 64, 1), (2, 128, 65)]
ROWS = [("last", *s) for s in LAST] + [(f, *s) for f in ("gauss", "dc", "peaky") for s in OTHER]
IDS = [f"{f}-B{b}-HW{hw}-Nk{nk}" for f, b, hw, nk in ROWS]


def _bounded(family, Bn, HW, Nk, identity):
    c = R.make_case(family, Bn, HW, Nk, identity_out=identity)
    x = c.x
    ref, emu = (c.ref_o, c.emu_o) if identity else (c.ref_branch, c.emu_branch)
    bound = 2.0 * emu + R.F16_ULP
    reject_tile_128(x)
    for tile in _tiles(HW):
        r = run(x, SPLIT, tile)
        rec = R.recover_branch(r.hi, r.lo, x.h, x.h_lo)
        term = R.recovery_term(r.hi, r.lo, x.h_lo)
        if identity:
            e, t = R.err_heads(rec, ref), R.term_heads(term, ref)
        else:
            e, t = R.err_rows(rec, ref), R.term_rows(term, ref)
        worst = float((e - t).max())
        print(f"xattn {'O (row, head)' if identity else 'branch row'} {family:6s} B {Bn} HW {HW:3d} Nk {Nk:2d} tile {tile:3d}: kernel {worst:.3e} (recovery term <= {float(t.max()):.1e})"
              f"  emulator {emu:.3e}  bound {bound:.3e}")
        assert worst <= bound, (family, Bn, HW, Nk, tile, worst, bound)


@pytest.mark.parametrize("family,Bn,HW,Nk", ROWS, ids=IDS)
def test_attention_per_row_and_head(family, Bn, HW, Nk):
    """Wo = I, bo = 0: the recovered branch is the fp16 attention output; no (row, head) pair is left out"""
    _bounded(family, Bn, HW, Nk, True)


@pytest.mark.parametrize("family,Bn,HW,Nk", ROWS, ids=IDS)
def test_branch_per_row(family, Bn, HW, Nk):
    _bounded(family, Bn, HW, Nk, False)


# ---- 3. exact families ---------------------------------------------------------------------------------------------------------------------------------------------
def _expect_planes(r, x, f, form, what):
    """out / out_lo / lo8 against torch's split of the exact f (float64; plain form: f without h_lo, one plane)"""
    hi, lo = R.split_planes(f.float(), form == LO8)
    assert torch.equal(r.hi, hi), (what, float((r.hi != hi).float().mean()))
    if form != PLAIN:
        assert torch.equal(r.lo, lo), (what, float((r.lo != lo).float().mean()))


@pytest.mark.parametrize("Nk", [80, 77])
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("form", [PLAIN, SPLIT, LO8], ids=list(FORM_NAME.values()))
def test_selector_sweep(form, tile, Nk):
    """the selected key of EVERY head visits every position (tests/test_xattn_ref.py checks the sweep's coverage); the split forms run on the h_lo grid"""
    Bn, HW = (3, 64) if tile == 64 else (2, 128)
    c = R.make_case("selector", Bn, HW, Nk, lo_grid=form != PLAIN)
    nz = 0.0
    for t in range(-(-80 // Bn)):
        j = R.default_jstar(Bn, Nk, t)
        x = c.x.with_lo(None if form == PLAIN else c.x.h_lo)
        x.kv = c.x.kv.clone()
        x.kv[..., :C] = R.selector_k(Bn, Nk, j)
        r = run(x, form, tile)
        _expect_planes(r, x, R.selector_closed_form(x, j)[1], form, (t, j.tolist()))
        if form != PLAIN:
            nz = float((r.lo != 0).float().mean())
            assert nz > 0.5
    print(f"xattn selector sweep {FORM_NAME[form]} tile {tile} Nk {Nk}: {-(-80 // Bn)} launches bit-identical to the closed form; lo plane {100 * nz:.0f} % non-zero")


EXACT = [("selector", 80, False), ("selector", 49, True), ("nk1", 1, False), ("nk1", 1, True), ("qround", 80, True), ("qround", 2, False), ("qround", 33, True)]


@pytest.mark.parametrize("Bn,HW", R.SHAPES)
@pytest.mark.parametrize("family,Nk,lo_grid", EXACT)
def test_exact_families(family, Nk, lo_grid, Bn, HW):
    c = R.make_case(family, Bn, HW, Nk, lo_grid=lo_grid)
    for form in (PLAIN, SPLIT, LO8):
        x = c.x.with_lo(None) if form == PLAIN else c.x
        f = c.exact_f - (c.x.h_lo.double() if form == PLAIN else 0.0)
        reject_tile_128(x, form)
        for tile in _tiles(HW):
            _expect_planes(run(x, form, tile), x, f, form, (family, FORM_NAME[form], tile))
    print(f"xattn exact {family} Nk {Nk} lo grid {lo_grid} B {Bn} HW {HW}: all forms and tiles bit-identical to the closed form")


@pytest.mark.parametrize("Bn,HW,Nk", [(2, 128, 80), (3, 64, 77), (1, 192, 80), (2, 256, 48)])
def test_denominator_adds_the_unrounded_exponentials(Bn, HW, Nk):
    """3b: h = 0, Wo = I, bo = 0: the hi plane is O and the lo plane zero, in every form"""
    c = R.make_case("denom", Bn, HW, Nk, identity_out=True)
    for form in (PLAIN, SPLIT, LO8):
        x = c.x.with_lo(None) if form == PLAIN else c.x
        reject_tile_128(x, form)
        for tile in _tiles(HW):
            r = run(x, form, tile)
            assert form == PLAIN or bool((r.lo == 0).all())
            excess, mean, bound = R.denom_check(r.hi, c)
            print(f"xattn denom B {Bn} HW {HW} Nk {Nk} {FORM_NAME[form]} tile {tile}: worst element {excess:+.3f} of its bound past it; |mean signed error| {mean:.2e} bound {bound:.2e}")
            assert excess <= 0 and mean <= bound


# ---- 4. form identities -----------------------------------------------------------------------------------------------------------------------------------------------
def _lo8_close(lo8, lo16):
    """d = f - hi is exact in fp32.  The split form stores lo16 = f16(d): |lo16 - d| <= half an fp16 ulp of d (2^-25 below the normals).  The lo8 form stores lo8 = e5m2(d):
    |lo8 - d| <= half an e5m2 ulp of d (2^-3 of its binade; 2^-17 below the normals).  Rounding never crosses a power of two downwards, so the binade of the STORED value is
    d's or the next one up, and half an ulp taken there bounds both: |lo8 - lo16| <= half_ulp_e5m2(lo8) + half_ulp_f16(lo16)."""
    a, b = R.lo8_value(lo8).double(), lo16.double()
    return bool(((a - b).abs() <= R.half_ulp(a, 2, -14) + R.half_ulp(b, 10, -14)).all())


IDENT = [(f, b, hw, nk) for f in ("gauss", "dc") for (b, hw), nk in zip(R.SHAPES, (77, 13, 80, 5, 33))]


@pytest.mark.parametrize("family,Bn,HW,Nk", IDENT)
def test_form_identities_bit_for_bit(family, Bn, HW, Nk):
    x = R.make_case(family, Bn, HW, Nk).x
    x0 = x.with_lo(torch.zeros_like(x.h_lo))
    x8 = x.with_lo(R.lo8_value(R.lo8_of(x.h_lo)).half())           # the stream an 8-bit lo plane represents; every e5m2 value is an fp16 value
    reject_tile_128(x)
    per_tile = {}
    for tile in _tiles(HW):
        s, p, s0, l8, s8 = run(x, SPLIT, tile), run(x, PLAIN, tile), run(x0, SPLIT, tile), run(x8, LO8, tile), run(x8, SPLIT, tile)
        assert torch.equal(p.hi, s0.hi)                                                     # plain == split hi at h_lo = 0
        assert torch.equal(run(x, PLAIN, tile, plain_entry=True).hi, p.hi)                  # cs_op_xattn_block == cs_op_xattn_block_x2 without lo planes
        assert torch.equal(l8.hi, s8.hi)                                                    # lo8 hi == split hi on the same represented stream
        assert _lo8_close(l8.lo, s8.lo)
        for form, xx, base in ((PLAIN, x, p), (SPLIT, x, s), (LO8, x8, l8)):
            for kw in (dict(inplace=True), dict(stats=True), dict(inplace=True, stats=True)):
                r = run(xx, form, tile, **kw)
                assert torch.equal(r.hi, base.hi) and (form == PLAIN or torch.equal(r.lo, base.lo)), (FORM_NAME[form], kw)
        assert bool(R.is_nearest_f16(s.hi, s.hi.double() + s.lo.double()).all())
        assert bool(R.is_nearest_f16(l8.hi, l8.hi.double() + R.lo8_value(l8.lo).double()).all())
        per_tile[tile] = (p, s, l8)
    if len(per_tile) == 2:
        for a, b in zip(per_tile[64], per_tile[128]):
            assert torch.equal(a.hi, b.hi) and (a.lo is None or torch.equal(a.lo, b.lo))    # tile 64 == tile 128
    print(f"xattn identities {family} B {Bn} HW {HW} Nk {Nk}: held bit for bit on tiles {list(per_tile)}")


# ---- 5. row statistics ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,Bn,HW,Nk", [("dc", 2, 128, 77), ("gauss", 2, 128, 80), ("dc", 1, 192, 13), ("peaky", 3, 64, 33)])
@pytest.mark.parametrize("form", [PLAIN, SPLIT, LO8], ids=list(FORM_NAME.values()))
def test_row_statistics(form, family, Bn, HW, Nk):
    x = R.make_case(family, Bn, HW, Nk).x
    xs = x.with_lo(torch.zeros_like(x.h_lo)) if form == PLAIN else x.with_lo(R.lo8_value(R.lo8_of(x.h_lo)).half()) if form == LO8 else x
    reject_tile_128(xs, form)
    for tile in _tiles(HW):
        s = run(xs, SPLIT, tile)                                    # the split form on the stream this form sees: hi + lo is f to 2^-22
        f = s.hi.double() + s.lo.double()
        r = run(xs.with_lo(None) if form == PLAIN else xs, form, tile, stats=True)
        e1, e2 = (r.stats[:, 0].double() - f.sum(1)).abs(), (r.stats[:, 1].double() - (f * f).sum(1)).abs()
        b1, b2 = (C + 1) * 2.0 ** -24 * f.abs().sum(1), (C + 1) * 2.0 ** -24 * (f * f).sum(1)
        print(f"xattn row_stats {family} {FORM_NAME[form]} tile {tile} B {Bn} HW {HW}: worst |error| / bound: sum {float((e1 / b1).max()):.3f}  sum of squares {float((e2 / b2).max()):.3f}")
        assert bool((e1 <= b1).all()) and bool((e2 <= b2).all())


# ---- 6. the launcher ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [64, 128])
def test_launcher_rejections_leave_the_outputs_alone(tile):
    x = R.make_case("gauss", 2, 128, 77).x             # (sizes such that even a call that SHOULD have been rejected would stay inside the guarded allocations)
    x192 = R.make_case("gauss", 1, 192, 13).x
    for form in (PLAIN, SPLIT, LO8):
        xf = x.with_lo(None) if form == PLAIN else x
        kw = dict(stats=True)
        run(xf, form, tile, expect=CS_E_UNSUPPORTED, Cc=640, **kw)
        run(xf, form, tile, expect=CS_E_UNSUPPORTED, Cc=312, **kw)
        run(xf, form, tile, expect=CS_E_UNSUPPORTED, heads=5, **kw)
        run(xf, form, tile, expect=CS_E_UNSUPPORTED, heads=16, **kw)
        run(xf, form, tile, expect=CS_E_SHAPE, Nk=0, **kw)
        run(xf, form, tile, expect=CS_E_SHAPE, Nk=81, **kw)
        run(xf, form, tile, expect=CS_E_SHAPE, Nk=-1, **kw)
        run(xf, form, tile, expect=CS_E_SHAPE, HW=96, M=192, **kw)            # HW % 64 != 0
        run(xf, form, tile, expect=CS_E_SHAPE, HW=32, M=64, **kw)
        run(xf, form, tile, expect=CS_E_SHAPE, HW=128, M=192, **kw)           # M is not a whole number of samples
        run(xf, form, tile, expect=CS_E_SHAPE, M=-128, **kw)
        run(xf, form, tile, expect=CS_OK, M=0, **kw)                          # nothing to do, nothing written
        for name in ("h", "out", "gamma", "beta", "wq", "wo", "bo", "kv"):
            run(xf, form, tile, expect=CS_E_ARG, null=name, **kw)
        if form != PLAIN:
            run(xf, form, tile, expect=CS_E_ARG, drop="h_lo", **kw)
            run(xf, form, tile, expect=CS_E_ARG, drop="out_lo", **kw)
        x2 = x192.with_lo(None) if form == PLAIN else x192
        if tile == 128:
            run(x2, form, tile, expect=CS_E_SHAPE, **kw)                      # HW = 192 needs the 64-row kernel
        else:
            run(x2, form, tile, **kw)
