"""Times the FID path on 64 images at 512 x 512 (uint8, as decoded PNGs arrive), split into its stages, and writes profiles/fid_bench.txt.  Synthetic
weights; medians of ``--reps`` runs after ``--warmup``; one JSON line at the end.

    python tools/bench_fid.py [--batch 64] [--reps 7] [--out profiles/fid_bench.txt]

* front end (mode-"F" bicubic resize to 299 x 299, clip, normalise) and the feature forward (``cs_fid_forward``), images / s of the two together;
* ``cs_fid_stats_accumulate`` at n = batch and n = 4096, d = 2048, each against the feature forward of the SAME batch in this run (the statistics are judged
  by that ratio; n = 4096 is set against 4096 / batch forwards), with its fp64 rate;
* ``cs_fid_stats_finalize``;
* the host Fréchet distance on two random full-rank 2048-d covariances, both routes, wall clock.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from consolver_amd import fid, synth

DEV = "cuda:0"


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, d = a.batch, 2048
    model = fid.load_fid_inception(DEV)
    model.load_state_dict(synth.synthetic_fid_inception_state_dict(model.manifest()))
    images = torch.randint(0, 256, (B, 3, a.size, a.size), dtype=torch.uint8, device=DEV)
    res = {"images": B, "size": a.size, "max_batch": model.max_batch}
    res["front_end_ms"] = timed(lambda: model.preprocess(images), a.warmup, a.reps)
    patches = model.preprocess(images)
    res["forward_ms"] = timed(lambda: model.encode_patches(patches), a.warmup, a.reps)
    res["features_ms"] = timed(lambda: model.features(images), a.warmup, a.reps)
    res["images_per_s"] = B / res["features_ms"] * 1e3
    res["forward_tflops"] = model.flops(B) / res["forward_ms"] / 1e9
    feats = model.features(images)
    st = fid.FIDStatistics(d, DEV)
    res["accumulate_n_batch_ms"] = timed(lambda: st.update(feats), a.warmup, a.reps)
    big = torch.randn(4096, d, device=DEV)
    res["accumulate_n4096_ms"] = timed(lambda: st.update(big), a.warmup, a.reps)
    res["accumulate_n4096_f64_tflops"] = 2.0 * 4096 * d * d / res["accumulate_n4096_ms"] / 1e9
    res["accumulate_share_of_forward"] = res["accumulate_n_batch_ms"] / res["forward_ms"]
    res["accumulate_n4096_share_of_forward"] = res["accumulate_n4096_ms"] / (res["forward_ms"] * 4096 / B)
    mu, sigma = torch.empty_like(st.sum), torch.empty_like(st.outer)
    from consolver_amd import _lib as L
    res["finalize_ms"] = timed(lambda: L.check(L.lib().cs_fid_stats_finalize(L.ptr(st.sum), L.ptr(st.outer), st.n, d, L.ptr(mu), L.ptr(sigma), L.stream_ptr(DEV))),
                               a.warmup, a.reps)
    rng = np.random.default_rng(0)
    stats = []
    for k in range(2):
        x = rng.normal(size=(3 * d, d)) @ (rng.normal(size=(d, d)) / np.sqrt(d)) + rng.normal(size=d)
        stats.append((x.mean(0), np.cov(x, rowvar=False)))
    vals = {}
    for method in ("sqrtm", "eigh"):
        t = time.perf_counter()
        vals[method] = fid.frechet_distance(*stats[0], *stats[1], method=method)
        res[f"distance_{method}_s"] = time.perf_counter() - t
    res["distance_routes_relative_difference"] = abs(vals["sqrtm"] / vals["eigh"] - 1)
    share, share_big = res["accumulate_share_of_forward"], res["accumulate_n4096_share_of_forward"]
    lines = [f"FID path, {B} uint8 images at {a.size}^2, FID Inception-v3 at 299, synthetic weights, medians of {a.reps}",
             f"  front end (float bicubic to 299, clip, normalise)   {res['front_end_ms']:8.3f} ms",
             f"  feature forward                                      {res['forward_ms']:8.3f} ms  ({model.flops(B) / 1e12:.3f} TFLOP, {res['forward_tflops']:.1f} TFLOP/s)",
             f"  features(images), both                               {res['features_ms']:8.3f} ms  = {res['images_per_s']:.0f} images / s",
             f"  stats accumulate, n = {B}, d = {d}                    {res['accumulate_n_batch_ms']:8.3f} ms  = {100 * share:.2f} % of the forward of the same {B} images",
             f"  stats accumulate, n = 4096, d = {d}                  {res['accumulate_n4096_ms']:8.3f} ms  = {res['accumulate_n4096_f64_tflops']:.2f} TFLOP/s fp64, "
             f"{100 * share_big:.2f} % of the {4096 // B} forwards that make 4096 rows",
             f"  stats finalize, d = {d}                              {res['finalize_ms']:8.3f} ms",
             f"  host distance, sqrtm route                           {res['distance_sqrtm_s']:8.2f} s",
             f"  host distance, eigh route                            {res['distance_eigh_s']:8.2f} s   (relative difference of the two: {res['distance_routes_relative_difference']:.1e})",
             "  remark: " + ("accumulate costs more than 5 % of the feature forward at n = batch: a call writes the whole 2048 x 2048 fp64 matrix (32 MB read + 32 MB written) "
                             "whatever n is; fewer, larger updates amortise it" if share > 0.05 else
                             "accumulate stays under 5 % of the feature forward of the same images"),
             "  not measured: real checkpoint weights (none available: synthetic weights throughout); JPEG / PNG decoding on the host"]
    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
