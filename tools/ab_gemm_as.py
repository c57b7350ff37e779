"""FF1 L0 and QKV L0 (M = 131072, K = 320): knob gemm_as 0 against 2, alternating, with an output hash"""
import hashlib, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from consolver_amd import ops
dev = "cuda:0"
torch.manual_seed(0)
def rnd(*s, scale=1.0): return (torch.randn(*s, device=dev) * scale).half()
def timeit(fn, iters=30):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3
M, C = 131072, 320
x = rnd(M, C); gam, bet = rnd(C) * 0.1 + 1, rnd(C, scale=0.1)
st = ops.row_stats(x)
w, b = rnd(8 * C, C, scale=C ** -0.5), rnd(8 * C)
wp, bp = ops.geglu_pack(w, b)
wf, sf, bf = (t.to(dev) for t in ops.ln_fold_pack(wp, bp, gam, bet))
wq = rnd(3 * C, C, scale=C ** -0.5)
qf, qs, qb = (t.to(dev) for t in ops.ln_fold_pack(wq, None, gam, bet))
ff1 = lambda: ops.linear_ln(x, wf, sf, bf, st, 1, geglu=True)
qkv = lambda: ops.linear_ln(x, qf, qs, qb, st, 1)
for rep in range(3):
    for knob in (0, 2):
        ops.set_tuning("gemm_as", knob)
        for tag, fn in (("ff1 geglu N 2560", ff1), ("qkv N 960", qkv)):
            o = fn(); r = ops.igemm_last_route()
            h = hashlib.sha1(o.cpu().numpy().tobytes()).hexdigest()[:12]
            print(f"rep {rep} gemm_as {knob} {tag:18s} {timeit(fn):8.1f} us  route {r.family}/{r.variant}  sha {h}", flush=True)
ops.reset_tuning()
