"""Reading one view's PLY into device memory: today's host reader plus the
upload (ply.read_ply -- np.loadtxt on one core -- then the tensors to the
device; for a file with normals also ply.read_normals, a second parse, as the
drop-ins did) against ply.read_cloud_device (the body uploaded through a
pinned buffer and parsed by sl_parse_ply_ascii / sl_unpack_ply_binary).

    python scripts/ply_read_bench.py                      # 1.0 M and 8.29 M points (a 4K view)
    python scripts/ply_read_bench.py --points 200000 --reps 3 --out profiles/ply_read/bench.jsonl

For each size two files of the same cloud: the reference's ASCII layout
(ply.save_ply: "%.4f %.4f %.4f %d %d %d") and the 51-byte binary layout
(ply.save_ply_open3d with normals).  Prints one JSON line per file: seconds of
both readers (median of ``--reps`` after one warm-up, wall time around
blocking calls, the page cache warm), the device path split into the file
read, the upload and the kernels (each waited for, so their sum exceeds
nothing the unsplit call overlaps), the points per second, and whether the two
results are bit-identical.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-250, 250, n), rng.uniform(-180, 180, n), rng.normal(600.0, 40.0, n)], 1)
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    return P, rng.integers(0, 256, (n, 3)).astype(np.uint8), N


def median_of(fn, reps):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=int, nargs="*", default=[1_000_000, 8_290_000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args(argv)
    import torch

    from structured_light_for_3d_model_replication_amd import ply
    dev = torch.device("cuda", 0)

    def host(path, normals):
        P, C = ply.read_ply(path)
        out = [torch.from_numpy(P).to(dev), torch.from_numpy(C).to(dev)]
        if normals:
            out.append(torch.from_numpy(ply.read_normals(path)).to(dev))
        torch.cuda.synchronize(dev)
        return out

    def device(path, normals, times=None):
        c = ply.read_cloud_device(path, device=dev, times=times)
        torch.cuda.synchronize(dev)
        assert c["info"]["path"] == "device", c["info"]
        return [c["points"], c["colors"]] + ([c["normals"]] if normals else [])

    with tempfile.TemporaryDirectory() as tmp:
        for n in a.points:
            P, C, N = cloud(n)
            files = {"ascii_%.4f": (os.path.join(tmp, "a.ply"), False), "binary_51B": (os.path.join(tmp, "b.ply"), True)}
            ply.save_ply(P, C, files["ascii_%.4f"][0])
            ply.save_ply_open3d(P, C, files["binary_51B"][0], normals=N)
            for layout, (path, normals) in files.items():
                t_host, want = median_of(lambda: host(path, normals), a.reps)
                t_dev, got = median_of(lambda: device(path, normals), a.reps)
                parts = []
                for _ in range(a.reps):
                    t = {}
                    device(path, normals, t)
                    parts.append(t)
                same = all(torch.equal(w.view(torch.int64) if w.dtype == torch.float64 else w,
                                       g.view(torch.int64) if g.dtype == torch.float64 else g)
                           for w, g in zip(want, got))
                line = {"layout": layout, "points": n, "file_bytes": os.path.getsize(path), "reps": a.reps,
                        "host_read_plus_upload_s": round(t_host, 5), "read_cloud_device_s": round(t_dev, 5),
                        "speedup": round(t_host / t_dev, 2),
                        "device_file_read_s": round(statistics.median(p["read_s"] for p in parts), 5),
                        "device_h2d_s": round(statistics.median(p["h2d_s"] for p in parts), 5),
                        "device_kernels_s": round(statistics.median(p["kernels_s"] for p in parts), 5),
                        "host_mpts_per_s": round(n / t_host / 1e6, 3), "device_mpts_per_s": round(n / t_dev / 1e6, 3),
                        "bit_identical": bool(same)}
                print(json.dumps(line), flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
                del want, got
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
