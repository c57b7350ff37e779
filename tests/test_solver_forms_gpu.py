"""Every kernel of consolver_amd/csrc/solver.hip but the policy MLP and true_cfg, element by element, through the C ABI: the streaming updates (lms DDIM / Euler, dpm,
unipc, fm) bit for bit against the fp32 replicas of tests/solver_ref.py (`*_exact`) and within the derived bound of the float64 forms (`*_fp64`); the glue kernels
(cosine features, stack, masks, sample / gather, action_probs) against exact replicas or, where they reduce in an order of their own, against float64 with the bounds
of tests/solver_ref.py (proven on the CPU by tests/test_solver_ref.py).  References, bounds, case lists and inputs all come from tests/solver_ref.py.

Every output is a 16-byte-aligned slice of a NaN-filled buffer with 64 elements of margin on each side; the margins are all NaN after the call.  One test moves
a base pointer off 16-byte alignment (test_fm_fp32_state_on_a_4_byte_boundary: the fp32 side of fm's mixed pair, one float); otherwise the only misalignment is
the one a ragged b * elems gives the per-sample kernels (lms, dpm, cosine, stack).

Measured on an MI355X (gfx950; solver.hip built with -O3 -ffp-contract=off):
    Bit-exact against the fp32 replica, every output tensor of every case: lms DDIM and Euler in all 17 (io, out, x_is_f32, lp) forms, the 48 / 24 history forms
    (the m == 1, scaler 0 16-bit product in fp16 and bf16 included), order_dim 8 and 1, the wider actions_stride, the rounding probe, the grid-stride second pass;
    dpm, unipc and fm in all their forms and in the grid-stride case.  No form fell back to the float64 bound alone, and solver.hip needed no fix: the division
    of the DDIM epilogue is correctly rounded, nothing is contracted, body and tail agree, f32_to_bf16 rounds ties and subnormals to nearest even.
    Worst err / bound against float64: 1.000 (an element that sits on the allowance of a tie), typically 0.44 - 0.67 with a 16-bit result.
    cosine features, worst err / bound: 0.068 at (3, 5), 0.014 at (3, 269), 0.003 at (2, 2061) -- the same figures as the CPU emulation of the kernel's order.
    entropy, worst err / bound: 0.089 (K = 2), 0.122 (K = 11), 0.022 (K = 161); the 2 ulp allowed for logf are an assumption that this leaves a factor 8 unused.
Shown to bite with three scratch mutants of solver.hip (not committed), each run against this module and against the solver tests that existed before it
(test_solver_gpu, test_engine_gpu, test_dpm_gpu, test_unipc_gpu, test_amed_gpu, test_fm_baselines_gpu):
    the tail's CFG rounding dropped in lms_step_kernel: 35 tests here fail, first test_lms_dtype_forms[f16-f16-0-None-ddim] (4 of 15 elements at (3, 5)); the earlier tests pass;
    store_lp1 writing the unrounded high half as bf16: 20 tests here fail, among them test_lms_rounding_probe and test_lms_dtype_forms[f32-f32-0-bf16-ddim]; the earlier tests pass;
    the coefficient sum started at c[1]: 43 tests here fail, first test_lms_dtype_forms[f32-f32-0-bf16-ddim] and test_lms_ddim_history_forms (earlier tests not run).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from consolver_amd import _lib as L
from tests import solver_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = 64
TD = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f32": 0, "f16": 1, "bf16": 2}


def st():
    return L.stream_ptr(torch.device(DEV))


def dev(a, dt="f32"):
    """a numpy fp32 array holding dt-representable values -> a device tensor of dtype dt (exact)"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(TD[dt]).to(DEV)


class Guarded:
    """a NaN-filled buffer with G elements of margin around n elements of dtype dt (torch dtype or name); off: elements by which the tensor is moved off
    16-byte alignment"""

    def __init__(self, shape, dt, off=0):
        self.dt = TD.get(dt, dt)
        n = int(np.prod(shape))
        if self.dt == torch.int64:
            self.buf = torch.full((n + 2 * G + off,), -77, dtype=self.dt, device=DEV)
        else:
            self.buf = torch.full((n + 2 * G + off,), float("nan"), dtype=self.dt, device=DEV)
        self.lo, self.hi = G + off, G + off + n
        self.view = self.buf[self.lo:self.hi].view(*shape)
        assert self.view.data_ptr() % 16 == off * self.buf.element_size()

    @property
    def ptr(self):
        return self.view.data_ptr()

    def margins_intact(self):
        m = torch.cat([self.buf[:self.lo], self.buf[self.hi:]])
        return bool((m == -77).all()) if self.dt == torch.int64 else bool(torch.isnan(m).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def numpy(self):
        v = self.view.cpu()
        return v.numpy() if self.dt == torch.int64 else v.float().numpy()


def p(t):
    return None if t is None else (t.ptr if isinstance(t, Guarded) else t.data_ptr())


# ----------------------------------------------------------------------------------------------------------------- the streaming kernels
def build(c):
    """(function, args struct, {output name: Guarded}, tensors to keep alive) of a case of tests/solver_ref.py"""
    k, B, n, io, out = c["kernel"], c["B"], c["elems"], c["io"], c["out"]
    shape = (B, n)
    xdt = "f32" if c["x_is_f32"] else io
    off = c.get("x_off", 0)                     # elements by which x and x_out are moved off 16-byte alignment
    outs = {"x_out": Guarded(shape, out, off)}
    if c["lp"]:
        outs["x_out_lp"] = Guarded(shape, c["lp"])
    keep = []

    def d(a, dt, off=0):
        t = dev(a, dt)
        if t is not None and off:
            buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
            assert buf.data_ptr() % 16 == 0
            t = buf[off:].view(t.shape).copy_(t)
        keep.append(t)
        return p(t)
    if k == "lms":
        a = L.CsStepArgs()
        a.x, a.eps_text, a.eps_uncond, a.guidance = d(c["x"], xdt), d(c["ec"], io), d(c["eu"], io), c["g"]
        for i, h in enumerate(c["hist"]):
            a.hist[i] = d(h, io)
        a.m, a.order_dim, a.scaler_dim = c["m"], c["order"], c["scaler"]
        a.actions, a.actions_stride = d(c["actions"], "f32"), c["actions_stride"]
        if c["eu"] is not None:
            outs["eps_out"] = Guarded(shape, io)
        a.eps_out = p(outs.get("eps_out"))
        a.sqrt_at, a.sqrt_1mat, a.sqrt_ap, a.sqrt_1map = c["ddim"]
        a.v_prediction, a.dt = c["vpred"], c["dt"]
        fn = L.lib().cs_lms_euler_step if c["euler"] else L.lib().cs_lms_ddim_step
    elif k == "dpm":
        a = L.CsDpmStepArgs()
        a.x, a.eps_text, a.eps_uncond, a.guidance, a.m_prev = d(c["x"], xdt), d(c["ec"], io), d(c["eu"], io), c["g"], d(c["m1"], io)
        if c["want_m_out"]:
            outs["m_out"] = Guarded(shape, io)
        a.m_out = p(outs.get("m_out"))
        a.conv_x, a.conv_e, a.cx, a.c0, a.c1 = c["scal"]
        fn = L.lib().cs_dpm_multistep_step
    elif k == "unipc":
        a = L.CsUnipcStepArgs()
        conv_x, conv_e, ca, cp, corr = c["scal"]
        rd0, rd1 = R._unipc_reads(c)
        nan = np.full(shape, np.nan, np.float32)                  # a history tensor that is not read may hold anything
        a.x, a.eps_text, a.eps_uncond, a.guidance = d(c["x"], out), d(c["ec"], io), d(c["eu"], io), c["g"]
        a.x_last, a.m_prev0, a.m_prev1 = d(c["x_last"] if corr else nan, out), d(c["m0"] if rd0 else nan, io), d(c["m1"] if rd1 else nan, io)
        a.use_corr = int(corr)
        outs["m_out"] = Guarded(shape, io)
        if c["want_x_last_out"]:
            outs["x_last_out"] = Guarded(shape, out)
        a.m_out, a.x_last_out = p(outs["m_out"]), p(outs.get("x_last_out"))
        a.conv_x, a.conv_e = conv_x, conv_e
        a.a_x, a.a_0, a.a_1, a.a_n = ca
        a.p_x, a.p_0, a.p_1 = cp
        fn = L.lib().cs_unipc_step
    else:
        a = L.CsFmStepArgs()
        a.x_base, a.v2, a.v1, a.c = d(c["x"], xdt, off), d(c["v2"], io), d(c["v1"], io), c["c"]
        fn = L.lib().cs_fm_general_step
    a.B, a.elems, a.io_dtype, a.out_dtype, a.x_is_f32, a.x_out = B, n, CODE[io], CODE[out], c["x_is_f32"], p(outs["x_out"])
    if k != "fm":
        a.x_out_lp, a.lp_dtype = p(outs.get("x_out_lp")), CODE[c["lp"] or "f32"]
    return fn, a, outs, keep


def run_case(c):
    """launch, then every output: margins, torch.equal with the replica, every element within the bound of the float64 form.  Returns the worst err / bound."""
    fn, a, outs, keep = build(c)
    L.check(fn(C.byref(a), st()))
    torch.cuda.synchronize()
    ex, rf = R.EXACT[c["kernel"]](c), R.FP64[c["kernel"]](c)
    assert set(ex) == set(outs) == set(rf), (c["name"], sorted(ex), sorted(outs))
    worst = 0.0
    for name, gd in outs.items():
        assert gd.margins_intact(), (c["name"], name, "wrote outside the tensor")
        got = gd.numpy()
        same = torch.equal(torch.from_numpy(got), torch.from_numpy(ex[name]))
        if not same:
            bad = np.flatnonzero(~((got == ex[name]).reshape(-1)))
            i = int(bad[0])
            raise AssertionError(f"{c['name']} {name}: {len(bad)} of {got.size} elements differ from the fp32 replica; first at flat index {i} "
                                 f"(sample {i // c['elems']}, element {i % c['elems']}): got {got.reshape(-1)[i]!r}, want {ex[name].reshape(-1)[i]!r}")
        r = R.within(got, rf[name])
        assert r <= 1.0, (c["name"], name, "err / bound vs float64", r)
        worst = max(worst, r)
    return worst


def run_cases(cases):
    worst = max(run_case(c) for c in cases)
    print(f"{len(cases)} cases bit-exact; worst err / bound vs float64 {worst:.3f}")


@pytest.mark.parametrize("euler", (0, 1), ids=("ddim", "euler"))
@pytest.mark.parametrize("form", R.DTYPE_FORMS, ids=R.form_id)
def test_lms_dtype_forms(form, euler):
    """(io, out, x_is_f32, lp) x tail only / body + tail off alignment / two blocks, at order_dim 4, m 3, scaler 2, CFG on"""
    run_cases(R.lms_form_cases(form, euler))


@pytest.mark.parametrize("form", R.LMS_HISTORY_FORMS_DDIM, ids=R.form_id)
def test_lms_ddim_history_forms(form):
    """m 1..4 x scaler 0..2 x v-prediction x CFG at (3, 269)"""
    run_cases(R.lms_history_cases(form, 0))


@pytest.mark.parametrize("form", R.LMS_HISTORY_FORMS_EULER, ids=R.form_id)
def test_lms_euler_history_forms(form):
    """m 1..4 x scaler 0..2 x CFG at (3, 269); f16/f16 and bf16/bf16 pin the m == 1, scaler 0 16-bit product in both 16-bit types"""
    run_cases(R.lms_history_cases(form, 1))


def test_lms_order_and_stride_forms():
    """order_dim 8 with m in {1, 7, 8}; order_dim 1 without actions; actions_stride = order + scaler + 1 with 1e6 in the columns that must not be read"""
    run_cases(R.lms_extra_cases())


def test_lms_rounding_probe():
    """Euler, dt = 0, m = 1, fp32 x: the result is x itself and the 16-bit copy its round-to-nearest-even image (ties to even and odd neighbours, subnormal fp16
    images, 65504 / 65519.99 / 65520, +-0), in the vector body and in the tail"""
    for c in R.lms_probe_cases():
        run_case(c)
        fn, a, outs, keep = build(c)
        L.check(fn(C.byref(a), st()))
        torch.cuda.synchronize()
        x = torch.from_numpy(c["x"])
        assert torch.equal(outs["x_out"].view.cpu(), x)
        with np.errstate(over="ignore"):
            assert torch.equal(outs["x_out_lp"].view.cpu(), x.to(TD[c["lp"]]))


@pytest.mark.parametrize("i", (0, 1), ids=("f16-f16", "f16-f32-xf32"))
def test_lms_grid_stride(i):
    """(64, 65549): 33 blocks of work per sample on a grid capped at 32, so the loop's second pass runs once; ragged, so samples start off alignment"""
    run_cases(R.lms_grid_stride_cases()[i:i + 1])


@pytest.mark.parametrize("form", R.DTYPE_FORMS, ids=R.form_id)
def test_dpm_dtype_forms(form):
    """orders 1 / 2 x CFG x identity / dpmsolver++ conversion, scalars of step 4 and of the last step of a 10-step run, x the three small shapes"""
    run_cases(R.dpm_form_cases(form))


@pytest.mark.parametrize("i", (0, 1), ids=("f16-f16", "f16-f32-xf32-lp"))
def test_dpm_grid_stride(i):
    run_cases(R.dpm_grid_stride_cases()[i:i + 1])


@pytest.mark.parametrize("form", R.UNIPC_FORMS, ids=R.form_id)
def test_unipc_dtype_forms(form):
    """use_corr x orders 1 / 2 x x_last_out absent / present + the last step, x the three small shapes; history tensors that are not read hold NaN"""
    run_cases(R.unipc_form_cases(form))


def test_unipc_grid_stride():
    run_cases(R.unipc_grid_stride_cases())


@pytest.mark.parametrize("form", R.FM_FORMS, ids=lambda f: R.form_id(f))
def test_fm_dtype_forms(form):
    run_cases(R.fm_form_cases(form))


def test_fm_grid_stride():
    run_cases(R.fm_grid_stride_cases())


@pytest.mark.parametrize("io", ("f16", "bf16"))
def test_fm_fp32_state_on_a_4_byte_boundary(io):
    """the fp32 side of a mixed pair needs 4-byte alignment only: 16-bit v2 / v1, x_is_f32 = 1 and an fp32 result at (3, 269), with x_base and x_out one float
    past a 16-byte boundary inside their buffers; Euler and Heun form, bit for bit, margins intact"""
    run_cases([dict(R.make_fm(f"fm-off4-{io}-v{v}", 3, 269, (io, "f32", 1), with_v1=v, which="interior"), x_off=1) for v in (0, 1)])


# ----------------------------------------------------------------------------------------------------------------- refusals
def refused(c, code, mutate):
    fn, a, outs, keep = build(c)
    extra = mutate(a, c) or []
    assert fn(C.byref(a), st()) == code, c["name"]
    torch.cuda.synchronize()
    for gd in list(outs.values()) + list(extra):
        assert gd.untouched(), c["name"]


def test_refusals_leave_outputs_untouched():
    """full-size device tensors, so that a missing refusal would be a valid launch that writes the outputs"""
    shape = (3, 269)
    lms = R.make_lms("refuse-lms", *shape, ("f16", "f16", 0, None), euler=0)
    dpm = R.make_dpm("refuse-dpm", *shape, ("f16", "f16", 0, None), order=2, cfg=1, kind="real", which="interior")
    uni = R.make_unipc("refuse-unipc", *shape, ("f16", "f16", 0, None), order=2, corr=1, which="interior", x_last_out=1)
    fm = R.make_fm("refuse-fm", *shape, ("f16", "f16", 0), with_v1=1, which="interior")

    def to_bf16_out(a, c):
        a.out_dtype = CODE["bf16"]
    for c in (lms, dict(lms, euler=1), dpm, uni, fm):
        refused(c, R.CS_E_DTYPE, to_bf16_out)

    def add_lp(a, c):
        g = Guarded(shape, "f16")
        a.x_out_lp, a.lp_dtype = g.ptr, CODE["f16"]
        return [g]
    for c in (lms, dict(lms, euler=1), dpm, uni):
        refused(c, R.CS_E_ARG, add_lp)

    def drop_eps_out(a, c):
        if c["kernel"] == "lms":
            a.eps_out = None
        else:
            a.m_out = None
    for c in (lms, dict(lms, euler=1), dpm):
        refused(c, R.CS_E_ARG, drop_eps_out)

    def x_is_f32(a, c):
        a.x_is_f32 = 1
    refused(R.make_unipc("refuse-unipc-f32", *shape, ("f32", "f32", 0, None), order=2, corr=1, which="interior", x_last_out=1), R.CS_E_DTYPE, x_is_f32)

    hist, _, _ = R.cosine_inputs("refuse-cos", *shape, "f16", 2, 0)
    hd = [dev(h, "f16") for h in hist]
    hp = (C.c_void_p * L.CS_MAX_ORDER)(*[t.data_ptr() for t in hd])
    eps_out, feat = Guarded(shape, "f16"), Guarded((3, 3), "f32")
    assert L.lib().cs_cosine_features_cfg(hp, 2, 4, 3, 269, CODE["f16"], None, 3.0, eps_out.ptr, feat.ptr, st()) == R.CS_E_ARG
    torch.cuda.synchronize()
    assert eps_out.untouched() and feat.untouched()


# ----------------------------------------------------------------------------------------------------------------- cosine_kernel
def cosine_call(hist, m, order, dt, eu=None, g=0.0):
    B, elems = hist[0].shape
    hd = [dev(h, dt) for h in hist[:m]]
    hp = (C.c_void_p * L.CS_MAX_ORDER)(*[t.data_ptr() for t in hd])
    feat = Guarded((B, order - 1), "f32")
    if eu is None:
        eps_out = None
        L.check(L.lib().cs_cosine_features(hp, m, order, B, elems, CODE[dt], feat.ptr, st()))
    else:
        ud, eps_out = dev(eu, dt), Guarded((B, elems), dt)
        L.check(L.lib().cs_cosine_features_cfg(hp, m, order, B, elems, CODE[dt], ud.data_ptr(), g, eps_out.ptr, feat.ptr, st()))
    torch.cuda.synchronize()
    assert feat.margins_intact() and (eps_out is None or eps_out.margins_intact())
    return feat.numpy().astype(np.float64), eps_out


@pytest.mark.parametrize("B,elems", R.COSINE_SHAPES)
@pytest.mark.parametrize("dt", R.DTYPES)
def test_cosine_features(dt, B, elems):
    """plain and CFG form x order in {2, 4, 8} x m in {1, 2, order}: zero features at i >= m, the combined eps bit for bit (m == 1 included), random inputs within
    (2 k + 4) 2^-24 of float64"""
    worst = 0.0
    for order, m in R.COSINE_ORDERS:
        for cfg in (0, 1):
            hist, eu, g = R.cosine_inputs(f"cos-{dt}-{B}x{elems}-{order}-{m}-{cfg}", B, elems, dt, m, cfg)
            ref, eps = R.cosine_fp64(hist, m, order, eu, g, dt)
            got, eps_out = cosine_call(hist, m, order, dt, eu, g)
            assert (got[:, m - 1:] == 0).all(), (order, m, cfg)
            if cfg:
                assert torch.equal(torch.from_numpy(eps_out.numpy()), torch.from_numpy(eps)), (order, m, "combined eps")
            r = float(np.abs(got - ref).max()) / R.cosine_bound(elems, dt)
            assert r <= 1.0, (order, m, cfg, r)
            worst = max(worst, r)
    print(f"cosine {dt} {B}x{elems}: worst err / bound {worst:.4f}")


@pytest.mark.parametrize("dt", R.DTYPES)
def test_cosine_exact_values(dt):
    """a zero history entry gives exactly 0; one-hot pairs at the first element of sample 1, the last lane of the last vector and the last tail element give exactly
    1.0 (0 if the kernel skips the position)"""
    for B, elems in R.COSINE_SHAPES:
        hist, _, _ = R.cosine_inputs(f"cos0-{dt}-{B}x{elems}", B, elems, dt, 3, 0)
        hist[1] = np.zeros_like(hist[1])
        got, _ = cosine_call(hist, 3, 4, dt)
        assert (got[:, 0] == 0).all() and (got[:, 1] != 0).all() and (got[:, 2] == 0).all()
        for b, pos in R.one_hot_positions(B, elems, dt):
            a = np.zeros((B, elems), np.float32)
            a[b, pos] = 1
            got, _ = cosine_call([a, a.copy()], 2, 2, dt)
            assert got[b, 0] == 1.0 and (np.delete(got[:, 0], b) == 0).all(), (B, elems, b, pos, got)
            got, eps_out = cosine_call([a, a.copy()], 2, 2, dt, eu=a.copy(), g=3.0)      # u + g (c - u) = c
            assert got[b, 0] == 1.0 and torch.equal(torch.from_numpy(eps_out.numpy()), torch.from_numpy(a)), (B, elems, b, pos, "cfg")


# ----------------------------------------------------------------------------------------------------------------- stack / masks
def stack_check(B, elems, dt, order, m, name):
    rng = np.random.default_rng(R._seed(name))
    hist = [R.tensor(rng, B, elems, dt) for _ in range(max(m, 1))]
    hd = [dev(h, dt) for h in hist]
    hp = (C.c_void_p * L.CS_MAX_ORDER)(*[t.data_ptr() for t in hd[:m]])
    out = Guarded((B, order, elems), dt)
    L.check(L.lib().cs_stack_history(hp, m, order, B, elems, CODE[dt], out.ptr, st()))
    torch.cuda.synchronize()
    assert out.margins_intact(), name
    want = np.zeros((B, order, elems), np.float32)
    for k in range(m):
        want[:, k] = hist[k]
    assert torch.equal(torch.from_numpy(out.numpy()), torch.from_numpy(want)), name


@pytest.mark.parametrize("dt", R.DTYPES)
def test_stack_history(dt):
    """the gather bit for bit and zero planes for k >= m: order in {1, 4, 8} x m in {0, 1, order} x the three small shapes"""
    for B, elems in R.small_shapes(dt):
        for order, m in R.STACK_ORDERS:
            stack_check(B, elems, dt, order, m, f"stack-{dt}-{B}x{elems}-{order}-{m}")


@pytest.mark.parametrize("dt", sorted(R.STACK_GRID_STRIDE))
def test_stack_history_grid_stride(dt):
    """the first sizes past the 64-block cap: the kernel's own grid-stride loop runs a second pass, and there is a tail"""
    B, elems = R.STACK_GRID_STRIDE[dt]
    stack_check(B, elems, dt, 4, 2, f"stack-gridstride-{dt}")


def test_step_masks():
    for B, A, m, order in R.MASK_CASES:
        out = Guarded((B, A), "f32")
        L.check(L.lib().cs_step_masks(B, A, m, order, out.ptr, st()))
        torch.cuda.synchronize()
        assert out.margins_intact() and np.array_equal(out.numpy(), R.masks_exact(B, A, m, order)), (B, A, m, order)


# ----------------------------------------------------------------------------------------------------------------- sample / gather / action_probs
@pytest.mark.parametrize("K,A,BA", R.SAMPLE_CASES, ids=lambda v: str(v))
def test_sample_actions(K, A, BA):
    """the inverse-CDF walk bit for bit: zero bins at the head, in the middle and at the tail, u equal to a partial sum, u above the fp32 total of a row that sums
    to 0.5; no returned bin has probability 0.  cs_gather_actions clamps indices -3 and K + 2."""
    B = BA // A
    pr, u, av = R.sample_case(K, A, BA)
    idx_w, act_w, ap_w = R.sample_exact(pr, u, av)
    dp, du, dav = dev(pr), dev(u), dev(av)
    idx, act, ap = Guarded((B, A), torch.int64), Guarded((B, A), "f32"), Guarded((B, A), "f32")
    L.check(L.lib().cs_sample_actions(dp.data_ptr(), du.data_ptr(), dav.data_ptr(), B, A, K, idx.ptr, act.ptr, ap.ptr, st()))
    torch.cuda.synchronize()
    assert idx.margins_intact() and act.margins_intact() and ap.margins_intact()
    assert np.array_equal(idx.numpy(), idx_w) and np.array_equal(act.numpy(), act_w) and np.array_equal(ap.numpy(), ap_w)
    assert (ap.numpy() > 0).all()
    gi = idx_w.copy()
    gi.reshape(-1)[0::3] = -3
    gi.reshape(-1)[1::3] = K + 2
    act_w, ap_w = R.gather_exact(pr, gi, av)
    dgi = torch.from_numpy(gi).to(DEV)
    act, ap = Guarded((B, A), "f32"), Guarded((B, A), "f32")
    L.check(L.lib().cs_gather_actions(dp.data_ptr(), dgi.data_ptr(), dav.data_ptr(), B, A, K, act.ptr, ap.ptr, st()))
    torch.cuda.synchronize()
    assert act.margins_intact() and ap.margins_intact()
    assert np.array_equal(act.numpy(), act_w) and np.array_equal(ap.numpy(), ap_w)


@pytest.mark.parametrize("K", (2, 11, 161))
def test_action_probs(K):
    """sel bit for bit (an action halfway between two grid values and a repeated grid value: the lower index wins); the entropy of rows with exact zeros, a one-hot
    row, a row that sums to 0.5 and a uniform row within ((2 K + 8) H + K + 2) 2^-24 / ln K + 2 2^-24 |ref| of float64 (2 ulp allowed for logf)"""
    pr, actn, av = R.action_probs_case(K)
    B, A, _ = pr.shape
    dp, da, dav = dev(pr), dev(actn), dev(av)
    sel, ent = Guarded((B, A), "f32"), Guarded((B, A), "f32")
    L.check(L.lib().cs_action_probs(dp.data_ptr(), da.data_ptr(), dav.data_ptr(), B, A, K, sel.ptr, ent.ptr, st()))
    torch.cuda.synchronize()
    assert sel.margins_intact() and ent.margins_intact()
    assert np.array_equal(sel.numpy(), R.sel_exact(pr, actn, av))
    ref, bound = R.entropy_fp64(pr), R.entropy_bound(pr)
    ratio = float((np.abs(ent.numpy().astype(np.float64) - ref) / bound).max())
    print(f"entropy K={K}: worst err / bound {ratio:.4f}")
    assert ratio <= 1.0
