"""K1 (fused CFG + LMS combine + DDIM/Euler) bandwidth: algorithmic bytes / kernel time vs HBM peak.

Algorithmic bytes per step: passes = [x] + [eps_u, eps_c] + [hist m-1] + [x'] + [eps store].

``--dpm``: the Multistep DPM-Solver update (cs_dpm_multistep_step) in the engine's form -- fp32 state, fp16 model outputs, CFG, second order, the fp16
copy of the result in the same pass -- next to cs_lms_ddim_step with a history of 2 on the same tensors (the same 18 bytes per element), and a 1 GiB
device copy (read + write bytes, what bench.py --full reports as dtod_copy_1gib_tbps) as the rate both are a share of.  The two kernels are timed
as hipGraph replays of 500 captured launches (a Python launch loop measures the host's enqueue rate at this size), alternating, median of 5.

``--unipc``: the fused UniPC corrector + predictor (cs_unipc_step) in the engine's form -- fp32 state, fp16 model outputs, CFG, second order, x_last
updated in place, the fp16 copy of the result in the same pass: 16 bytes read and 12 written per element -- next to cs_dpm_multistep_step (18 bytes per
element) on the same tensors and the 1 GiB device copy, timed in the same run by the same captured-graph method as ``--dpm``.

``--lin``: the n-term linear update of DEIS and iPNDM (cs_linear_step) in the engine's form -- fp32 state, fp16 model outputs, CFG, the fp16 copy of
the result in the same pass -- at B = 16 and 80 of SD's 4 x 64 x 64 latents for terms = 1..4 (16 + 2 (terms - 1) bytes per element), and at terms = 2
alternating in the same process with cs_dpm_multistep_step at order 2 on the same tensors (the same 18 bytes per element), by the captured-graph method
of ``--dpm``, next to the 1 GiB device copy.

``--fm``: the flow-matching baselines' update (cs_fm_general_step; Euler form x + dt v, Heun form x + c (v1 + v2)) at FLUX's packed latent size
[1, 4096, 64] bf16 next to cs_lms_euler_step with a history of one on the same tensors, timed the same way in the same run as the 1 GiB copy.  At
0.5 MB per tensor the kernels are launch-latency-bound: the figure is microseconds per launch, not a share of a roofline."""
import ctypes as C, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consolver_amd import _lib as L

dev = torch.device("cuda:0")
lib = L.lib()

def run(B, elems, dtype, m, cfg=True, euler=False, iters=50):
    t = lambda: torch.randn(B, elems, device=dev).to(dtype)
    x, eu, ec, out, eo = t(), t(), t(), t(), t()
    hist = [t() for _ in range(m - 1)]
    actions = torch.rand(B, 3, device=dev)
    a = L.CsStepArgs()
    a.x, a.eps_text, a.eps_uncond, a.guidance = x.data_ptr(), ec.data_ptr(), (eu.data_ptr() if cfg else None), 3.0
    for k, h in enumerate(hist): a.hist[k] = h.data_ptr()
    a.m, a.order_dim, a.scaler_dim = m, 4, 0
    a.actions, a.actions_stride, a.B, a.elems = actions.data_ptr(), 3, B, elems
    a.io_dtype = a.out_dtype = L.dtype_code(dtype)
    a.x_out, a.eps_out = out.data_ptr(), (eo.data_ptr() if cfg else None)
    a.sqrt_at, a.sqrt_1mat, a.sqrt_ap, a.sqrt_1map, a.dt = 0.3, 0.95, 0.5, 0.86, -0.1
    fn = lib.cs_lms_euler_step if euler else lib.cs_lms_ddim_step
    st = L.stream_ptr(dev)
    for _ in range(3): L.check(fn(C.byref(a), st))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): L.check(fn(C.byref(a), st))
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / iters * 1e3
    passes = 1 + (2 if cfg else 1) + (m - 1) + 1 + (1 if cfg else 0)
    nbytes = passes * B * elems * x.element_size()
    return dict(B=B, elems=elems, dtype=str(dtype).split(".")[-1], m=m, cfg=cfg, euler=euler, us=round(us, 2),
                MB=round(nbytes / 1e6, 2), GBps=round(nbytes / us / 1e3, 1), frac_of_8TBps=round(nbytes / us / 1e3 / 8000, 3))

def time_us(fn, iters):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def graph_us(fn, launches=500, replays=10):
    """kernel time without the host's launch path: ``launches`` back-to-back launches captured into one hipGraph, replayed ``replays`` times"""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3): fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches): fn()
    return time_us(g.replay, replays) / launches


def run_dpm(B=32, elems=4 * 64 * 64):
    h = lambda: torch.randn(B, elems, device=dev).half()
    x, out = torch.randn(B, elems, device=dev), torch.empty(B, elems, device=dev)
    eu, ec, m1, mo, lp = h(), h(), h(), h(), h()
    d = L.CsDpmStepArgs()
    d.x, d.eps_text, d.eps_uncond, d.guidance, d.m_prev = x.data_ptr(), ec.data_ptr(), eu.data_ptr(), 3.0, m1.data_ptr()
    d.B, d.elems, d.io_dtype, d.out_dtype, d.x_is_f32 = B, elems, L.CS_F16, L.CS_F32, 1
    d.x_out, d.m_out, d.x_out_lp, d.lp_dtype = out.data_ptr(), mo.data_ptr(), lp.data_ptr(), L.CS_F16
    d.conv_x, d.conv_e, d.cx, d.c0, d.c1 = 0.0, 1.0, 1.02, -0.21, 0.07
    actions = torch.rand(B, 3, device=dev)
    a = L.CsStepArgs()
    a.x, a.eps_text, a.eps_uncond, a.guidance = x.data_ptr(), ec.data_ptr(), eu.data_ptr(), 3.0
    a.hist[0] = m1.data_ptr()
    a.m, a.order_dim, a.scaler_dim = 2, 2, 0
    a.actions, a.actions_stride, a.B, a.elems = actions.data_ptr(), 3, B, elems
    a.io_dtype, a.out_dtype, a.x_is_f32 = L.CS_F16, L.CS_F32, 1
    a.x_out, a.eps_out, a.x_out_lp, a.lp_dtype = out.data_ptr(), mo.data_ptr(), lp.data_ptr(), L.CS_F16
    a.sqrt_at, a.sqrt_1mat, a.sqrt_ap, a.sqrt_1map = 0.3, 0.95, 0.5, 0.86
    nbytes = (4 + 2 + 2 + 2 + 4 + 2 + 2) * B * elems          # x, eps_u, eps_c, m1 | x', m0, fp16 copy of x'
    src = torch.randn(1 << 28, device=dev); dst = torch.empty_like(src)
    copy_gbps = 2.0 * (1 << 30) / time_us(lambda: dst.copy_(src), 20) / 1e3
    del src, dst
    kernels = (("cs_dpm_multistep_step", lib.cs_dpm_multistep_step, d), ("cs_lms_ddim_step_m2", lib.cs_lms_ddim_step, a))
    times = {name: [] for name, _, _ in kernels}
    for _ in range(5):                                        # alternate the two kernels; report the median window
        for name, fn, args in kernels:
            times[name].append(graph_us(lambda: L.check(fn(C.byref(args), L.stream_ptr(dev)))))
    rows = []
    for name, _, _ in kernels:
        us = sorted(times[name])[2]
        rows.append(dict(kernel=name, B=B, elems=elems, state="float32", outputs="float16", cfg=True, order=2, us=round(us, 2),
                         us_min_max=[round(min(times[name]), 2), round(max(times[name]), 2)], MB=round(nbytes / 1e6, 2),
                         GBps=round(nbytes / us / 1e3, 1), copy_1gib_GBps=round(copy_gbps, 1), share_of_copy_rate=round(nbytes / us / 1e3 / copy_gbps, 3)))
    return rows


def run_unipc(B=32, elems=4 * 64 * 64):
    h = lambda: torch.randn(B, elems, device=dev).half()
    x, xl, out = torch.randn(B, elems, device=dev), torch.randn(B, elems, device=dev), torch.empty(B, elems, device=dev)
    eu, ec, m0, m1, mo, lp = h(), h(), h(), h(), h(), h()
    u = L.CsUnipcStepArgs()
    u.x, u.eps_text, u.eps_uncond, u.guidance = x.data_ptr(), ec.data_ptr(), eu.data_ptr(), 3.0
    u.x_last, u.m_prev0, u.m_prev1, u.use_corr = xl.data_ptr(), m0.data_ptr(), m1.data_ptr(), 1
    u.B, u.elems, u.io_dtype, u.out_dtype, u.x_is_f32 = B, elems, L.CS_F16, L.CS_F32, 1
    u.x_out, u.m_out, u.x_last_out, u.x_out_lp, u.lp_dtype = out.data_ptr(), mo.data_ptr(), xl.data_ptr(), lp.data_ptr(), L.CS_F16
    # (a_x + a_0 + a_1 + a_n = 1 and |a_x| < 1: x_last, rewritten in place 500 times per replay, stays bounded)
    u.conv_x, u.conv_e, u.a_x, u.a_0, u.a_1, u.a_n, u.p_x, u.p_0, u.p_1 = 1.05, -0.31, 0.8, 0.05, -0.02, 0.17, 0.8, 0.27, -0.07
    d = L.CsDpmStepArgs()
    d.x, d.eps_text, d.eps_uncond, d.guidance, d.m_prev = x.data_ptr(), ec.data_ptr(), eu.data_ptr(), 3.0, m0.data_ptr()
    d.B, d.elems, d.io_dtype, d.out_dtype, d.x_is_f32 = B, elems, L.CS_F16, L.CS_F32, 1
    d.x_out, d.m_out, d.x_out_lp, d.lp_dtype = out.data_ptr(), mo.data_ptr(), lp.data_ptr(), L.CS_F16
    d.conv_x, d.conv_e, d.cx, d.c0, d.c1 = 1.05, -0.31, 0.8, 0.27, -0.07
    src = torch.randn(1 << 28, device=dev); dst = torch.empty_like(src)
    copy_gbps = 2.0 * (1 << 30) / time_us(lambda: dst.copy_(src), 20) / 1e3
    del src, dst
    # bytes per element: x, x_last, eps_u, eps_c, m_prev0, m_prev1 | x', x_c, m_new, fp16 copy of x'   and   x, eps_u, eps_c, m_prev | x', m0, fp16 copy
    kernels = (("cs_unipc_step", lib.cs_unipc_step, u, 28), ("cs_dpm_multistep_step", lib.cs_dpm_multistep_step, d, 18))
    times = {name: [] for name, _, _, _ in kernels}
    for _ in range(5):                                        # alternate the two kernels; report the median window
        for name, fn, args, _ in kernels:
            times[name].append(graph_us(lambda: L.check(fn(C.byref(args), L.stream_ptr(dev)))))
    rows = []
    for name, _, _, bpe in kernels:
        us, nbytes = sorted(times[name])[2], bpe * B * elems
        rows.append(dict(kernel=name, B=B, elems=elems, state="float32", outputs="float16", cfg=True, order=2, bytes_per_elem=bpe, us=round(us, 2),
                         us_min_max=[round(min(times[name]), 2), round(max(times[name]), 2)], MB=round(nbytes / 1e6, 2),
                         GBps=round(nbytes / us / 1e3, 1), copy_1gib_GBps=round(copy_gbps, 1), share_of_copy_rate=round(nbytes / us / 1e3 / copy_gbps, 3)))
    rows.append(dict(unipc_over_dpm_time=round(rows[0]["us"] / rows[1]["us"], 3), bytes_ratio=round(28 / 18, 3)))
    return rows


def run_fm(B=1, elems=4096 * 64):
    t = lambda: torch.randn(B, elems, device=dev).bfloat16()
    x, v, v1, out = t(), t(), t(), t()
    f = L.CsFmStepArgs()
    f.x_base, f.v2, f.v1, f.c, f.x_out = x.data_ptr(), v.data_ptr(), None, -0.1, out.data_ptr()
    f.B, f.elems, f.io_dtype, f.out_dtype = B, elems, L.CS_BF16, L.CS_BF16
    fh = L.CsFmStepArgs.from_buffer_copy(f)
    fh.v1 = v1.data_ptr()
    actions = torch.zeros(B, 1, device=dev)
    a = L.CsStepArgs()
    a.x, a.eps_text, a.m, a.order_dim, a.scaler_dim = x.data_ptr(), v.data_ptr(), 1, 2, 0
    a.actions, a.actions_stride, a.B, a.elems = actions.data_ptr(), 1, B, elems
    a.io_dtype = a.out_dtype = L.CS_BF16
    a.x_out, a.dt = out.data_ptr(), -0.1
    src = torch.randn(1 << 28, device=dev); dst = torch.empty_like(src)
    copy_gbps = 2.0 * (1 << 30) / time_us(lambda: dst.copy_(src), 20) / 1e3
    del src, dst
    kernels = (("cs_fm_general_step", lib.cs_fm_general_step, f, 3), ("cs_fm_general_step_v1", lib.cs_fm_general_step, fh, 4),
               ("cs_lms_euler_step_m1", lib.cs_lms_euler_step, a, 3))
    times = {name: [] for name, _, _, _ in kernels}
    for _ in range(5):                                        # alternate the kernels; report the median window
        for name, fn, args, _ in kernels:
            times[name].append(graph_us(lambda: L.check(fn(C.byref(args), L.stream_ptr(dev)))))
    rows = []
    for name, _, _, passes in kernels:
        us, nbytes = sorted(times[name])[2], passes * B * elems * 2
        rows.append(dict(kernel=name, B=B, elems=elems, dtype="bfloat16", us=round(us, 2), us_min_max=[round(min(times[name]), 2), round(max(times[name]), 2)],
                         MB=round(nbytes / 1e6, 2), GBps=round(nbytes / us / 1e3, 1), copy_1gib_GBps=round(copy_gbps, 1)))
    return rows


def run_lin(elems=4 * 64 * 64):
    src = torch.randn(1 << 28, device=dev); dst = torch.empty_like(src)
    copy_gbps = 2.0 * (1 << 30) / time_us(lambda: dst.copy_(src), 20) / 1e3
    del src, dst
    rows = []
    for B in (16, 80):
        h = lambda: torch.randn(B, elems, device=dev).half()
        x, out = torch.randn(B, elems, device=dev), torch.empty(B, elems, device=dev)
        eu, ec, mo, lp = h(), h(), h(), h()
        hist = [h() for _ in range(3)]
        d = L.CsDpmStepArgs()
        d.x, d.eps_text, d.eps_uncond, d.guidance, d.m_prev = x.data_ptr(), ec.data_ptr(), eu.data_ptr(), 3.0, hist[0].data_ptr()
        d.B, d.elems, d.io_dtype, d.out_dtype, d.x_is_f32 = B, elems, L.CS_F16, L.CS_F32, 1
        d.x_out, d.m_out, d.x_out_lp, d.lp_dtype = out.data_ptr(), mo.data_ptr(), lp.data_ptr(), L.CS_F16
        d.conv_x, d.conv_e, d.cx, d.c0, d.c1 = 0.0, 1.0, 1.02, -0.21, 0.07
        lins = {}
        for terms in (1, 2, 3, 4):
            a = L.CsLinStepArgs()
            a.x, a.eps_text, a.eps_uncond, a.guidance = x.data_ptr(), ec.data_ptr(), eu.data_ptr(), 3.0
            for k in range(terms - 1): a.hist[k] = hist[k].data_ptr()
            a.terms, a.B, a.elems, a.io_dtype, a.out_dtype, a.x_is_f32 = terms, B, elems, L.CS_F16, L.CS_F32, 1
            a.x_out, a.m_out, a.x_out_lp, a.lp_dtype = out.data_ptr(), mo.data_ptr(), lp.data_ptr(), L.CS_F16
            a.conv_x, a.conv_e, a.cx = 0.0, 1.0, 1.02
            for k, c in enumerate((-0.21, 0.07, -0.03, 0.01)[:terms]): a.c[k] = c
            lins[terms] = a
        # x, eps_u, eps_c, hist | x', m0, fp16 copy of x'
        kernels = [("cs_dpm_multistep_step_o2", lib.cs_dpm_multistep_step, d, 18), ("cs_linear_step_t2", lib.cs_linear_step, lins[2], 18)]
        kernels += [(f"cs_linear_step_t{t}", lib.cs_linear_step, lins[t], 16 + 2 * (t - 1)) for t in (1, 3, 4)]
        times = {name: [] for name, _, _, _ in kernels}
        for _ in range(5):                                    # alternate the kernels; report the median window and the spread
            for name, fn, args, _ in kernels:
                times[name].append(graph_us(lambda: L.check(fn(C.byref(args), L.stream_ptr(dev)))))
        for name, _, _, bpe in kernels:
            us, nbytes = sorted(times[name])[2], bpe * B * elems
            rows.append(dict(kernel=name, B=B, elems=elems, state="float32", outputs="float16", cfg=True, bytes_per_elem=bpe, us=round(us, 2),
                             us_min_max=[round(min(times[name]), 2), round(max(times[name]), 2)], MB=round(nbytes / 1e6, 2),
                             GBps=round(nbytes / us / 1e3, 1), copy_1gib_GBps=round(copy_gbps, 1), share_of_copy_rate=round(nbytes / us / 1e3 / copy_gbps, 3)))
        dpm, lin = times["cs_dpm_multistep_step_o2"], times["cs_linear_step_t2"]
        rows.append(dict(B=B, lin_t2_over_dpm_o2_time=round(sorted(lin)[2] / sorted(dpm)[2], 3), dpm_spread=round(max(dpm) / min(dpm), 3),
                         lin_spread=round(max(lin) / min(lin), 3)))
    return rows


if "--lin" in sys.argv:
    for r in run_lin(): print(json.dumps(r))
    sys.exit(0)

if "--fm" in sys.argv:
    for r in run_fm(): print(json.dumps(r))
    sys.exit(0)

if "--unipc" in sys.argv:
    for r in run_unipc(): print(json.dumps(r))
    sys.exit(0)

if "--dpm" in sys.argv:
    for r in run_dpm(): print(json.dumps(r))
    sys.exit(0)

rows = [run(16, 16384, torch.float16, 4),            # configs[1]: batch 16, steady state step
        run(80, 16384, torch.float16, 4),            # configs[4]: PPO rollout batch
        run(1, 262144, torch.bfloat16, 2, cfg=False, euler=True),   # configs[3]: FLUX packed latents
        run(4096, 16384, torch.float16, 4),          # 1 GB working set: what the kernel sustains when HBM-bound
        run(2048, 262144, torch.bfloat16, 2, cfg=False, euler=True)]
for r in rows: print(json.dumps(r))


def policy_us(B, hidden=256, K=11, order=4, iters=200):
    """policy MLP + softmax (cs_factor_probs) per sampling step: one conditioning row broadcast to B samples"""
    import consolver_amd
    net = consolver_amd.FactorNetPPO(hidden_dim=hidden, num_actions=K, order_dim=order, scaler_dim=0)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape) * 0.5)
    net.to(dev)
    row = torch.tensor([[874.0, 749.0]], device=dev)
    rows = row.repeat(B, 1).contiguous()
    out = {}
    for name, fn in (("broadcast_row", lambda: net.probs_from(row, batch=B)), ("per_row", lambda: net.probs_from(rows))):
        for _ in range(5): fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters): fn()
        e1.record(); torch.cuda.synchronize()
        out[name + "_us"] = round(e0.elapsed_time(e1) / iters * 1e3, 2)     # includes the host-side launch path
    return dict(kernel="factor_probs", B=B, hidden=hidden, **out)

print(json.dumps(policy_us(16)))
print(json.dumps(policy_us(80)))
