"""Background removal (merge.segment_plane, csrc/slplane.inl) on wall + object
clouds of a 1080p and a 4K view, at the reference's defaults
(distance_threshold 50, ransac_n 3, 1000 iterations).

    python scripts/background_bench.py                       # time + sweep + CPU baseline
    python scripts/background_bench.py --mode trace          # + one rocprofv3 kernel-trace run per size
    python scripts/background_bench.py --mode one --n N      # one call (what the trace run wraps)

``time`` prints one JSON line per size: device-event time per call (median of
``--reps``), the iterations run, a sweep of the batch schedule, and the only
CPU baseline there is here: the NumPy restatement tests/plane_oracle.py on
this host at the same N (NOT Open3D, which is not installed).

``trace`` starts ``rocprofv3 --kernel-trace --stats`` on a fresh child (``--mode
one``), reads its kernel statistics and prints per-kernel time, the split into
scoring (k_plane_hyp / k_plane_score / k_plane_fold_cnt), refinement
(k_plane_err / k_plane_flags / k_plane_sums / k_plane_fold_sum) and compaction
(scan + compact kernels), and k_plane_score's achieved bytes/s and f64 op/s
from its shapes against the chip's peaks.
"""
import argparse
import csv
import functools
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = {"1080p": 1920 * 1080, "4k": 3840 * 2160}
# MI355X peaks.  HBM: 8.0 TB/s spec (about 6.3 TB/s achievable).  f64 VALU:
# 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 f64 instructions-lanes / s
# (the public 78.6 TFLOP/s vector-FP64 figure counts an FMA as two; this code
# is uncontracted, so one op per instruction).
PEAK_BYTES, PEAK_F64 = 8.0e12, 39.3e12
SCORE_OPS_PER_POINT_PLANE = 7  # 3 mul + 3 add + 1 compare (|.| is an operand modifier)
THR, ITERS, SEED = 50.0, 1000, 7


@functools.lru_cache(maxsize=1)
def scene(n):
    from tests import plane_oracle as po
    return po.wall_scene(n, 0.6, rng_seed=1)[0]


def run_one(n, batch, reps):
    import torch

    from structured_light_for_3d_model_replication_amd import merge
    dev = merge._engine(None).device
    P = torch.from_numpy(scene(n)).to(dev)
    out = merge.segment_plane(P, THR, 3, ITERS, seed=SEED, batch=batch)  # warm-up: scratch pool, code objects
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = merge.segment_plane(P, THR, 3, ITERS, seed=SEED, batch=batch)
        e1.record()
        torch.cuda.synchronize(dev)
        ms.append(e0.elapsed_time(e1))
    return ms, out


def mode_time(a):
    from tests import plane_oracle as po
    for name, n in SIZES.items():
        if a.only and name != a.only:
            continue
        ms, (model, inl, info) = run_one(n, 0, a.reps)
        line = {"size": name, "points": n, "threshold": THR, "num_iterations": ITERS, "seed": SEED,
                "iterations_run": info["iterations"], "inliers": int(inl.shape[0]),
                "segment_plane_ms_median": statistics.median(ms), "segment_plane_ms_all": ms,
                "clock": "device events around the blocking call (host walk and copies included)"}
        sweep = {}
        for b in a.sweep:
            m2, (_, _, i2) = run_one(n, b, a.reps)
            assert i2["iterations"] == info["iterations"]
            sweep[str(b)] = {"ms_median": statistics.median(m2), "ms_min": min(m2), "ms_max": max(m2)}
        sweep["0 (default)"] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
        line["batch_sweep"] = sweep
        if a.cpu:
            P = scene(n)
            t0 = time.perf_counter()
            em, ei, eit = po.segment_plane(P, THR, 3, ITERS, seed=SEED)
            dt = time.perf_counter() - t0
            line["cpu_baseline"] = {"what": "tests/plane_oracle.py (NumPy restatement, same host, same N; not Open3D)",
                                    "seconds": dt, "iterations_run": eit,
                                    "bit_identical": bool(np.array_equal(em, model) and
                                                          np.array_equal(ei, inl.cpu().numpy()))}
        print(json.dumps(line), flush=True)


PHASES = {"scoring": ("k_plane_hyp", "k_plane_score", "k_plane_fold_cnt"),
          "refinement": ("k_plane_err", "k_plane_flags", "k_plane_sums", "k_plane_fold_sum"),
          "compaction": ("k_tile_sums", "k_scan1", "k_tile_scan", "k_compact_index")}


def mode_trace(a):
    for name, n in SIZES.items():
        if a.only and name != a.only:
            continue
        out = os.path.join(a.out, f"trace_{name}")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "trace", "--",
               sys.executable, os.path.abspath(__file__), "--mode", "one", "--n", str(n)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.timeout)
        if r.returncode:
            print(r.stdout[-2000:])
            raise SystemExit(r.returncode)
        info = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        kern, phase, calls = {}, {k: 0.0 for k in PHASES}, {}
        scored = 0.0
        # the child runs the call twice (warm-up + one, identical work): per call = total / 2
        for r_ in csv.DictReader(open(files[0])):
            nm = r_["Kernel_Name"]
            short = next((k for ks in PHASES.values() for k in ks if k + "(" in nm or k + "<" in nm), None)
            if short is None:
                continue
            us = (int(r_["End_Timestamp"]) - int(r_["Start_Timestamp"])) / 2e3
            kern[short] = kern.get(short, 0.0) + us
            calls[short] = calls.get(short, 0) + 0.5
            phase[next(p for p, ks in PHASES.items() if short in ks)] += us
            if short == "k_plane_fold_cnt":  # one workgroup per scored hypothesis
                scored += int(r_["Grid_Size_X"]) / int(r_["Workgroup_Size_X"]) / 2
        info["scored"], info["score_launches"] = scored, calls.get("k_plane_score", 0)
        score_s = kern.get("k_plane_score", 0.0) * 1e-6
        passes = info["score_launches"]
        line = {"size": name, "points": n, "iterations_run": info["iterations"], "hypotheses_scored": info["scored"],
                "score_launches": passes, "kernel_us_per_call": kern, "launches_per_call": calls,
                "phase_us_per_call": phase,
                "clock": "rocprofv3 --kernel-trace --stats: kernel durations summed (no gaps, no host time)"}
        if score_s > 0:
            by = passes * n * 24.0  # every launch streams the cloud once; partials are < 1 % of that
            ops = float(info["scored"]) * n * SCORE_OPS_PER_POINT_PLANE
            line["k_plane_score"] = {
                "bytes_per_s": by / score_s, "fraction_of_hbm_peak_8TBs": by / score_s / PEAK_BYTES,
                "f64_ops_per_s": ops / score_s, "fraction_of_f64_valu_peak_39.3T": ops / score_s / PEAK_F64,
                "bound": "f64 VALU" if ops / PEAK_F64 > by / PEAK_BYTES else "HBM"}
        print(json.dumps(line), flush=True)


def mode_one(a):
    ms, (_, inl, info) = run_one(a.n, 0, 1)
    print(json.dumps({"iterations": info["iterations"], "ms": ms[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("time", "trace", "one"), default="time")
    ap.add_argument("--n", type=int, default=SIZES["1080p"])
    ap.add_argument("--only", choices=tuple(SIZES), default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", type=int, nargs="*", default=[16, 32, 64, 128, 256, 1000])
    ap.add_argument("--no-cpu", dest="cpu", action="store_false")
    ap.add_argument("--out", default="build/background")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    {"time": mode_time, "trace": mode_trace, "one": mode_one}[a.mode](a)


if __name__ == "__main__":
    main()
