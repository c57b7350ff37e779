"""FLUX-Kontext edit under true classifier-free guidance at the full model size on one MI355X: 19 + 38 blocks, 512 text + 4096 latent + 4096
reference tokens, 8 steps, bf16, synthetic weights (no checkpoint exists offline: every number here is on seeded random weights).

Measured, each in a fresh child process that loads the weights and warms every shape up before the timed rounds:
  * the unguided edit of this tree, and -- with ``--parent-tree DIR`` (a built checkout of the parent commit) -- of the parent build, run before
    and after this tree's child so that the spread between two runs of the same code is on record;
  * this tree's edit with ``true_cfg_scale = 4``: one forward of 2 text rows over the 1 latent row (the default) against two 1-row forwards per
    step, alternated within every round;
  * the combine kernel alone (fp32 heads -> bf16, the engine's default) with its achieved bandwidth, 10 bytes per element;
  * ``cs_flux_workspace_bytes`` at B = 1 and B = 2.
Times are device events around whole edits, median over the rounds.  No threshold is asserted: the file is the record.

    python tools/bench_flux_true_cfg.py --out profiles/flux_true_cfg_bench.txt [--parent-tree DIR] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, LQ, STEPS, SCALE = 512, 4096, 8, 4.0


def child(tree, what, rounds):
    sys.path.insert(0, tree)
    import torch
    from consolver_amd import _lib as L
    from consolver_amd import generate_flux as gf
    from consolver_amd.flux import FluxKontextSamplingEngine, HipFluxTransformer2DModel, pack_latents
    from consolver_amd.synth import synthetic_flux_state_dict
    dev = torch.device("cuda:0")
    m = HipFluxTransformer2DModel(device=dev)
    m.load_state_dict(synthetic_flux_state_dict(m.manifest(), device=dev, dtype=m.dtype))
    g = torch.Generator().manual_seed(43)
    lat = pack_latents(torch.randn(1, 16, 128, 128, generator=g)).to(torch.bfloat16).to(dev)
    img = pack_latents(torch.randn(1, 16, 128, 128, generator=g)).to(torch.bfloat16).to(dev)
    ln = lambda x: torch.nn.functional.layer_norm(x, (4096,))
    enc, nenc = (ln(torch.randn(1, T, 4096, generator=g)).to(torch.bfloat16).to(dev) for _ in range(2))
    pooled, npooled = (torch.randn(1, 768, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        return a.elapsed_time(b)

    sch = gf.make_scheduler("euler")                                                # policy-free: the same work in every run
    eng = FluxKontextSamplingEngine(m, sch, guidance_scale=2.5)
    runs = {"unguided": lambda: eng.generate(lat, img, enc, pooled, latent_hw=(64, 64), num_inference_steps=STEPS)}
    res = {"tree": tree, "what": what}
    if what == "cfg":
        class TwoForwards:                                                           # the same handle without the row broadcast: two forwards per step
            broadcasts_latent_rows = False

            def __getattr__(self, k):
                return getattr(m, k)

            def __call__(self, *a, **kw):
                return m(*a, **kw)
        eng2 = FluxKontextSamplingEngine(TwoForwards(), sch, guidance_scale=2.5)
        neg = dict(negative_prompt_embeds=nenc, negative_pooled_prompt_embeds=npooled, true_cfg_scale=SCALE)
        runs["cfg_one_forward"] = lambda: eng.generate(lat, img, enc, pooled, latent_hw=(64, 64), num_inference_steps=STEPS, **neg)
        runs["cfg_two_forwards"] = lambda: eng2.generate(lat, img, enc, pooled, latent_hw=(64, 64), num_inference_steps=STEPS, **neg)
    for fn in runs.values():                                                         # warm-up of every shape (also sizes the workspaces)
        timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():                                                   # alternated within the round
            ms[k].append(timed(fn))
    res["ms_per_edit"] = ms
    if what == "cfg":
        from consolver_amd.flux import true_cfg_combine
        n = LQ * 64
        both = torch.randn(2, LQ, 64, device=dev)
        out = torch.empty(1, LQ, 64, dtype=torch.bfloat16, device=dev)
        reps = 2000
        for _ in range(20):
            true_cfg_combine(both[:1], both[1:], SCALE, out=out)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            true_cfg_combine(both[:1], both[1:], SCALE, out=out)
        b.record(); torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        res["combine"] = {"elements": n, "us_per_call_back_to_back": us, "bytes": 10 * n, "GB_per_s": 10 * n / (us * 1e-6) / 1e9,
                          "note": "back-to-back launches from Python: an upper bound of the kernel's time (launch-bound at 2.6 MB per call)"}
        res["workspace_bytes"] = {f"B={b_}": int(L.lib().cs_flux_workspace_bytes(m._h, b_, T, 2 * LQ)) for b_ in (1, 2)}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its unguided edit is timed too")
    ap.add_argument("--child", nargs=2, metavar=("TREE", "WHAT"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.rounds)
    plan = [(HERE, "cfg")]
    if args.parent_tree:
        plan = [(os.path.abspath(args.parent_tree), "unguided")] + plan + [(os.path.abspath(args.parent_tree), "unguided")]
    results = []
    for tree, what in plan:                                                          # one fresh process per build; a failed child ends the run
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, what, "--rounds", str(args.rounds)],
                           stdout=subprocess.PIPE, text=True, timeout=540)
        if p.returncode != 0:
            sys.exit(f"child {tree} {what} failed with {p.returncode}")
        results.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
        print(f"done: {what} on {tree}", flush=True)
    med = lambda v: statistics.median(v)
    lines = [f"FLUX-Kontext edit, full size (19 + 38 blocks, {T} text + {LQ} latent + {LQ} reference tokens), {STEPS} steps, bf16, Euler, synthetic weights, one MI355X",
             f"median of {args.rounds} rounds after a warm-up of every shape; ms per edit / ms per step"]
    this = next(r for r in results if r["what"] == "cfg")
    for r in results:
        tag = "this tree" if r["tree"] == HERE else "parent build"
        for k, v in r["ms_per_edit"].items():
            lines.append(f"  {tag:12s} {k:18s} {med(v):9.1f} / {med(v) / STEPS:8.2f}   rounds: " + " ".join(f"{x:.1f}" for x in v))
    u, c1, c2 = (med(this["ms_per_edit"][k]) for k in ("unguided", "cfg_one_forward", "cfg_two_forwards"))
    lines.append(f"true CFG (scale {SCALE}) over unguided, this tree: one 2-row forward {c1 / u:.3f} x, two 1-row forwards {c2 / u:.3f} x; one / two = {c1 / c2:.4f}")
    cb = this["combine"]
    lines.append(f"combine kernel, fp32 heads -> bf16, {cb['elements']} elements ({cb['bytes']} bytes): {cb['us_per_call_back_to_back']:.2f} us per call back to back "
                 f"= {cb['GB_per_s']:.0f} GB/s ({cb['note']}); {cb['us_per_call_back_to_back'] * 1e-3 / (c1 / STEPS) * 100:.4f} % of a guided step")
    lines.append("workspace bytes: " + ", ".join(f"{k}: {v} ({v / 2 ** 30:.2f} GiB)" for k, v in this["workspace_bytes"].items()))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
