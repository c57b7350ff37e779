"""tests/solver_ref.py on the CPU, on the inputs of tests/test_solver_forms_gpu.py: every `*_exact` replica stays within the derived bound of its `*_fp64` form
(and the bound is not vacuous: a replica with one rounding point dropped, or a grid step of slack, fails it), equals oracle/solver_oracle.py bit for bit where
that restates the same step (PPOSchedulerOracle.step, FMPPOSchedulerOracle.step with its m == 1 16-bit product rule, ddim_update, cfg_combine), and the cosine
and entropy bounds hold for fp32 emulations that sum in the kernels' order."""
import numpy as np
import pytest

from oracle import solver_oracle as so
from tests import solver_ref as R

F32 = np.float32


def stream_groups():
    g = {}
    for euler in (0, 1):
        for f in R.DTYPE_FORMS:
            g[f"lms-{'euler' if euler else 'ddim'}-{R.form_id(f)}"] = (lambda f=f, euler=euler: R.lms_form_cases(f, euler))
        for f in (R.LMS_HISTORY_FORMS_EULER if euler else R.LMS_HISTORY_FORMS_DDIM):
            g[f"lms-hist-{'euler' if euler else 'ddim'}-{R.form_id(f)}"] = (lambda f=f, euler=euler: R.lms_history_cases(f, euler))
    g["lms-extra"] = R.lms_extra_cases
    g["lms-probe"] = R.lms_probe_cases
    g["lms-gridstride"] = R.lms_grid_stride_cases
    for f in R.DTYPE_FORMS:
        g[f"dpm-{R.form_id(f)}"] = (lambda f=f: R.dpm_form_cases(f))
    g["dpm-gridstride"] = R.dpm_grid_stride_cases
    for f in R.UNIPC_FORMS:
        g[f"unipc-{R.form_id(f)}"] = (lambda f=f: R.unipc_form_cases(f))
    g["unipc-gridstride"] = R.unipc_grid_stride_cases
    for f in R.FM_FORMS:
        g[f"fm-{R.form_id(f)}"] = (lambda f=f: R.fm_form_cases(f))
    g["fm-gridstride"] = R.fm_grid_stride_cases
    return g


GROUPS = stream_groups()


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_exact_within_bound_of_fp64(group):
    worst, flips, n16 = 0.0, 0, 0
    for c in GROUPS[group]():
        ex, rf = R.EXACT[c["kernel"]](c), R.FP64[c["kernel"]](c)
        assert set(ex) == set(rf), c["name"]
        for k in ex:
            assert ex[k].shape == (c["B"], c["elems"]) and ex[k].dtype == F32
            r = R.within(ex[k], rf[k])
            assert r <= 1.0, (c["name"], k, r)
            worst = max(worst, r)
            dt = {"x_out": c["out"], "x_out_lp": c["lp"], "x_last_out": c["out"]}.get(k, c["io"])
            if dt != "f32":
                fin = np.isfinite(rf[k][0])
                flips += int((rf[k][1][fin] > 0.75 * R.spacing(rf[k][0][fin], dt)).sum())
                n16 += int(fin.sum())
    print(f"{group}: worst err / bound {worst:.3f}; {flips} of {n16} 16-bit elements carry a grid step of allowance")
    # the bound is half an ulp except next to a tie: from one fp16 element in 2^12 per rounding point to about 1 in 70 for the 16-bit copy of a DDIM result
    # (the division by sqrt(alpha_t) carries ~50 fp32 ulps)
    assert flips <= 8 + n16 // 20, (flips, n16)


def test_bound_is_not_vacuous(monkeypatch):
    """a replica that skips the CFG rounding, or cuts the 16-bit copy from the high half of the fp32 result (truncation), leaves the bound"""
    c = R.lms_form_cases(("f16", "f32", 1, "bf16"), 0)[1]
    ex, rf = R.lms_exact(c), R.lms_fp64(c)
    assert max(R.within(ex[k], rf[k]) for k in ex) <= 1.0
    trunc = (ex["x_out"].view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    assert R.within(trunc, rf["x_out_lp"]) > 1.0
    monkeypatch.setattr(R, "cfg_exact", lambda ec, eu, g, io: so.cfg_combine(eu, ec, F32(g)))
    assert R.within(R.lms_exact(c)["x_out"], rf["x_out"]) > 1.0


def test_rnd64_is_one_rounding():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 5, 4000), R.probe_row().astype(np.float64)]).astype(F32)
    for dt in ("f16", "bf16"):
        assert np.array_equal(R.rnd64(x.astype(np.float64), dt), R.rnd(x, dt).astype(np.float64))
    # a value that rounds differently through fp32: just above the fp16 tie 1 + 2^-11, by less than half an fp32 ulp
    v = 1 + 2.0 ** -11 + 2.0 ** -30
    assert R.rnd64(v, "f16") == 1 + 2.0 ** -10 and float(R.rnd(F32(v), "f16")) == 1.0


# ----------------------------------------------------------------------------------------------------------------- against oracle/solver_oracle.py
@pytest.fixture
def replay(monkeypatch):
    """the oracle schedulers' step with the policy replaced by given actions: everything after the actions is the oracle's own code"""
    box = {}
    monkeypatch.setattr(so, "factor_net_probs", lambda w, x, stack, **kw: np.zeros((x.shape[0], kw["action_dims"], kw["num_actions"]), F32))
    monkeypatch.setattr(so, "gather_actions", lambda probs, av, idx: (box["actions"], np.zeros_like(box["actions"])))
    return box


@pytest.mark.parametrize("h", R.history_list(0), ids=lambda h: "m{m}s{scaler}v{vpred}g{cfg}".format(**h))
def test_lms_ddim_exact_equals_oracle_step(replay, h):
    n, i = 8, 3
    orc = so.PPOSchedulerOracle(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", timestep_spacing="trailing", order_dim=4,
                                scaler_dim=h["scaler"], prediction_type="v_prediction" if h["vpred"] else "epsilon", num_actions=3)
    orc.set_timesteps(n)
    t = int(orc.timesteps[i])
    c = R.make_lms("oracle-ddim-%s" % h, 3, 269, ("f32", "f32", 0, None), euler=0, order=4, **h)
    a_t, a_p = orc.alphas_cumprod[t], orc.alphas_cumprod[t - 1000 // n]
    c["ddim"] = tuple(float(v) for v in (np.sqrt(a_t), np.sqrt(F32(1) - a_t), np.sqrt(a_p), np.sqrt(F32(1) - a_p)))
    assert c["ddim"] == R.ddim_scalars("interior")               # the case lists use the product scheduler's scalars: the same four numbers
    replay["actions"] = c["actions"]
    e = R.cfg_exact(c["ec"], c["eu"], c["g"], "f32")
    if c["eu"] is not None:
        assert np.array_equal(e, so.cfg_combine(c["eu"], c["ec"], c["g"]))
    for old in c["hist"][::-1]:
        orc.step(old, t, c["x"], None)
    want = orc.step(e, t, c["x"], None)["prev_sample"]
    assert np.array_equal(R.lms_exact(c)["x_out"], want)


@pytest.mark.parametrize("io", R.DTYPES)
@pytest.mark.parametrize("h", R.history_list(1), ids=lambda h: "m{m}s{scaler}g{cfg}".format(**h))
def test_lms_euler_exact_equals_oracle_step(replay, h, io):
    """FMPPOSchedulerOracle.step, with its m == 1, scaler 0 rule: dt cast to the model dtype and the product rounded to it"""
    i = 3
    orc = so.FMPPOSchedulerOracle(shift=3.0, order_dim=4, scaler_dim=h["scaler"], mu_dim=0, num_actions=3)
    orc.set_timesteps(8)
    for out in ("f32", io):
        c = R.make_lms("oracle-euler-%s-%s" % (h, io), 3, 269, (io, out, int(io != "f32"), None), euler=1, order=4, **h)
        assert F32(c["dt"]) == F32(orc.sigmas[i + 1] - orc.sigmas[i])
        replay["actions"] = c["actions"]
        orc.ets, orc.step_index = [], None
        e = R.cfg_exact(c["ec"], c["eu"], c["g"], io)
        for old in c["hist"][::-1]:
            orc.step(old, c["x"], None, io_dtype=io, begin_index=i - (h["m"] - 1))
        o = orc.step(e, c["x"], None, io_dtype=io, begin_index=i)
        assert orc.step_index == i + 1
        assert np.array_equal(R.lms_exact(c)["x_out"], o["prev_sample_f32"] if out == "f32" else o["prev_sample"])
    if h["m"] == 1 and h["scaler"] == 0 and io != "f32":
        plain = (c["x"] + F32(c["dt"]) * e).astype(F32)
        assert not np.array_equal(R.rnd(plain, io), R.lms_exact(c)["x_out"])      # the rule is visible on these inputs


def test_ddim_epilogue_equals_oracle():
    for v in (0, 1):
        c = R.make_lms("oracle-epilogue", 3, 269, ("f32", "f32", 0, None), euler=0, m=1, order=4, scaler=0, cfg=0, vpred=v)
        a_t, a_p = F32(0.31), F32(0.62)
        c["ddim"] = tuple(float(s) for s in (np.sqrt(a_t), np.sqrt(F32(1) - a_t), np.sqrt(a_p), np.sqrt(F32(1) - a_p)))
        assert np.array_equal(R.lms_exact(c)["x_out"], so.ddim_update(c["x"], c["ec"], a_t, a_p, "v_prediction" if v else "epsilon"))


def test_coefficient_order_matters_on_these_inputs():
    """the cases can tell a coefficient sum that starts at c[1] from the kernel's (it leaves c[m-1] off by c[0])"""
    c = R.make_lms("coef", 3, 269, ("f32", "f32", 0, None), euler=0, m=3, order=4, scaler=0)
    good = R.lms_exact(c)["x_out"]
    bad = dict(c, actions=c["actions"].copy())
    bad["actions"][:, 0] += F32(0.25)
    assert not np.array_equal(R.lms_exact(bad)["x_out"], good)
    assert len({tuple(r) for r in c["actions"]}) == 3 and np.abs(c["actions"]).max() <= 0.5


def test_actions_extra_columns_hold_a_million():
    c = [c for c in R.lms_extra_cases() if "stride" in c["name"]][0]
    assert c["actions_stride"] == c["order"] + c["scaler"] + 1 and (c["actions"][:, -2:] == 1e6).all() and np.abs(c["actions"][:, :-2]).max() <= 0.5


def test_probe_row_contents():
    r = R.probe_row()
    assert np.signbit(r[1]) and r[0] == 0 and r[1] == 0 and 65520.0 in r and 65504.0 in r
    assert np.isinf(R.rnd(F32(65520.0), "f16")) and R.rnd(F32(65519.99), "f16") == 65504.0
    h = 2.0 ** -11
    assert R.rnd(F32(1 + h), "f16") == 1.0 and R.rnd(F32(1 + 3 * h), "f16") == F32(1 + 4 * h)            # ties: to the even neighbour, down and up
    assert R.rnd(F32(1 + 2.0 ** -8), "bf16") == 1.0 and R.rnd(F32(1 + 3 * 2.0 ** -8), "bf16") == F32(1 + 2.0 ** -6)
    assert 0 < R.rnd(F32(3e-6), "f16") < 2.0 ** -14                                                       # a subnormal fp16 image


# ----------------------------------------------------------------------------------------------------------------- cosine / entropy bounds
@pytest.mark.parametrize("dt", R.DTYPES)
@pytest.mark.parametrize("B,elems", R.COSINE_SHAPES)
def test_cosine_bound_holds_for_the_kernel_order(dt, B, elems):
    worst = 0.0
    for order, m in R.COSINE_ORDERS:
        for cfg in (0, 1):
            hist, eu, g = R.cosine_inputs(f"cos-{dt}-{B}x{elems}-{order}-{m}-{cfg}", B, elems, dt, m, cfg)
            ref, _ = R.cosine_fp64(hist, m, order, eu, g, dt)
            emu = R.cosine_emulated(hist, m, order, eu, g, dt)
            assert (emu[:, m - 1:] == 0).all() and (ref[:, m - 1:] == 0).all()
            worst = max(worst, float(np.abs(emu - ref).max()) / R.cosine_bound(elems, dt))
    print(f"cosine {dt} {B}x{elems}: emulation err / bound {worst:.4f}")
    assert worst <= 1.0


def test_cosine_exact_values_in_the_kernel_order():
    for dt in R.DTYPES:
        for B, elems in R.COSINE_SHAPES:
            for b, pos in R.one_hot_positions(B, elems, dt):
                a = np.zeros((B, elems), F32)
                a[b, pos] = 1
                out = R.cosine_emulated([a, a.copy()], 2, 2, None, 0.0, dt)
                assert out[b, 0] == 1.0 and (np.delete(out[:, 0], b) == 0).all()


@pytest.mark.parametrize("K", (2, 11, 161))
def test_entropy_bound_holds_for_the_kernel_order(K):
    p, _, _ = R.action_probs_case(K)
    ref, emu, bound = R.entropy_fp64(p), R.entropy_emulated(p), R.entropy_bound(p)
    ratio = float((np.abs(emu - ref) / bound).max())
    print(f"entropy K={K}: emulation err / bound {ratio:.4f}")
    assert ratio <= 1.0
    assert np.allclose(ref[4], 1.0, atol=1e-12) and (ref[2] < 1e-6).all()                                   # the uniform and the one-hot row
    assert np.allclose(R.entropy_fp64(p[3] * 2), ref[3], atol=1e-7)                                        # the unnormalised row is normalised first
    assert np.array_equal(emu, so.normalized_entropy(p)) or float(np.abs(emu - so.normalized_entropy(p)).max()) <= 4 * K * 2.0 ** -24


def test_discrete_replicas_match_the_oracle():
    for K, A, BA in R.SAMPLE_CASES[:12]:
        p, u, av = R.sample_case(K, A, BA)
        idx, act, ap = R.sample_exact(p, u, av)
        a2, p2 = so.gather_actions(p, av, idx)
        assert np.array_equal(act, a2) and np.array_equal(ap, p2) and (ap > 0).all()
    for K in (2, 11, 161):
        p, act, av = R.action_probs_case(K)
        k = so.nearest_bins(act, av)
        assert np.array_equal(R.sel_exact(p, act, av), np.take_along_axis(p, k[..., None], 2)[..., 0])
    for B, A, m, order in R.MASK_CASES:
        assert np.array_equal(R.masks_exact(B, A, m, order), so.masks_for(B, A, m, order))


def test_sample_case_reaches_its_edges():
    p, u, av = R.sample_case(11, 3, 129)
    rows, uf = p.reshape(-1, 11), u.reshape(-1)
    assert (rows[::4, 0] == 0).any() and (rows[2::4, -1] == 0).any() and (rows[1::4, 3] == 0).any()
    tot = np.zeros(len(rows), F32)
    for j in range(11):
        tot = (tot + rows[:, j]).astype(F32)
    assert (uf[1::4] > tot[1::4]).all() and (tot[1::5] < 0.51).all()
    idx, _, ap = R.sample_exact(p, u, av)
    assert (ap > 0).all() and idx.min() >= 0 and idx.max() <= 10


def test_running_bound_is_within_the_counted_bound():
    """the operation-by-operation bound never exceeds (number of fp32 roundings) x 2^-24 x (sum of |terms|): dpm, fp32, second order, no CFG --
    out = cx x + c0 (conv_x x + conv_e e) + c1 m1 has 3 roundings in m0 and 5 after it"""
    c = R.make_dpm("counted", 3, 269, ("f32", "f32", 0, None), order=2, cfg=0, kind="real", which="interior")
    conv_x, conv_e, cx, c0, c1 = (abs(float(F32(v))) for v in c["scal"])
    x, e, m1 = (np.abs(c[k]).astype(np.float64) for k in ("x", "ec", "m1"))
    terms = cx * x + c0 * (conv_x * x + conv_e * e) + c1 * m1
    ref, bound = R.dpm_fp64(c)["x_out"]
    assert ((bound - 0.5 * R.spacing(ref, "f32")) <= 8 * R.U * terms * (1 + 1e-6)).all()
