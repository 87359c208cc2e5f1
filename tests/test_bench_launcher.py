"""bench.py's multi-rank launch, on CPU (gloo): ``--gpus N`` without
torch.distributed.run must start N ranks itself, report n_gpus == N and gather
every rank's cloud to rank 0 in view order (``--selftest``: the launch, timing
and gather plumbing with a stand-in per-rank cloud, no kernels)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                       timeout=240, env=env, cwd=REPO)
    return p


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("n,scaling,views,expect", [(2, "weak", 3, 6000), (3, "strong", 7, 7000)])
def test_gpus_n_starts_n_ranks(n, scaling, views, expect):
    p = _run(["--gpus", str(n), "--selftest", "--backend", "gloo", "--steps", "2", "--scaling", scaling,
              "--views", str(views)])
    assert p.returncode == 0, p.stderr[-2000:]
    r = _json_line(p.stdout)
    assert r["n_gpus"] == n
    assert r["gathered_points"] == expect
    assert sum(r["counts"]) == expect and len(r["counts"]) == n
    assert r["view_order_ok"]
    # the N-GPU line's self-validating block: communicator size, every rank's
    # timing and points, the gather's own view of the counts, bytes and rate
    m = r["multi_gpu"]
    assert m["comm_size"] == n and m["gather_counts_len"] == n
    assert len(m["per_rank_s"]) == n and all(s >= 0 for s in m["per_rank_s"])
    assert m["per_rank_points"] == m["gather_counts"] == r["counts"]
    assert m["gather_bytes_to_root"] == 15 * (expect - r["counts"][0])
    # what the gather must move, stated before it runs
    assert m["bytes_per_point"] == 15 and m["expected_gather_bytes_to_root"] == m["gather_bytes_to_root"]
    assert m["gather_ms"] > 0 and m["gather_GBps"] > 0
    # the strong-scaled config-3 leg (36 views sharded over the N ranks)
    sc = m["strong_c3"]
    assert sc["comm_size"] == n and sc["views_total"] == 36
    assert sc["per_rank_views"] == [len(range(-(-r * 36 // n), -(-(r + 1) * 36 // n))) for r in range(n)]
    assert sum(sc["per_rank_views"]) == 36
    assert sc["gather_counts"] == [1000 * v for v in sc["per_rank_views"]] == sc["per_rank_points"]
    assert len(sc["per_rank_ms_per_step"]) == n and sc["ms_per_step"] == max(sc["per_rank_ms_per_step"])
    assert sc["px_per_s"] > 0 and sc["gather_bytes_to_root"] == 15 * 1000 * (36 - sc["per_rank_views"][0])
    assert sc["expected_gather_bytes_to_root"] == sc["gather_bytes_to_root"]
    # the shard imbalance's bound on strong-scaling efficiency: 36 / (N x max views)
    assert sc["ideal_strong_efficiency"] == pytest.approx(36 / (n * max(sc["per_rank_views"])))
    assert sc["ideal_strong_efficiency"] == pytest.approx({2: 1.0, 3: 1.0}[n])


def test_gpus_disagreeing_with_world_size_is_an_error():
    p = _run(["--gpus", "2", "--selftest", "--backend", "gloo", "--steps", "1"],
             {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0
    assert "disagrees with WORLD_SIZE" in p.stderr


def test_streams_defaults_per_config():
    """--streams defaults to the per-config measured best."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    assert bench.parse([]).streams is None
    assert bench.parse(["--streams", "3"]).streams == 3
    assert bench.CONFIGS["c1"]["streams"] == 4 and bench.CONFIGS["c5"]["streams"] == 3
    # c1's lanes on high-priority streams (a hardware queue each), the others at the default
    assert bench.CONFIGS["c1"]["lane_priority"] == -1 and bench.parse([]).lane_priority is None
    # timed steps: 20 (the driver's command passes --steps itself), c1 200 (its window's fill and drain)
    assert bench.parse([]).steps == 20 and bench.parse(["--config", "c1"]).steps == 200
    assert bench.parse(["--config", "c1", "--steps", "20"]).steps == 20
    assert all(bench.CONFIGS[c]["lane_priority"] == -1 for c in ("c4", "c5"))  # 3 lanes need 3 queues
    assert all("lane_priority" not in bench.CONFIGS[c] for c in ("c2", "c3"))
    assert bench.CONFIGS["c3"]["streams"] == 2 and bench.CONFIGS["c4"]["streams"] == 3  # measured, DESIGN 5.2 / 6.2
    # c2: two lanes over a ring of distinct resident views (round 5: 2 lanes
    # 114 vs 121 us per step once the maps and xyz left with nt stores)
    assert bench.CONFIGS["c2"]["streams"] == 2 and bench.CONFIGS["c2"]["ring"] == 3
    # c1's control window: distinct views whose inputs exceed the 256 MiB Infinity Cache
    c1 = bench.CONFIGS["c1"]
    assert c1["ring_control"] * c1["H"] * c1["W"] * (2 + 2 * 10 + 3) > 2 ** 28
    assert c1["ring_control"] % c1["streams"] == 0 and bench.parse([]).ring_control is None


def test_headline_is_the_reference_arithmetic():
    """The headline xyz mode is the reference's f64 arithmetic (sl_system.py:
    614-648); f32-fast is only ever the secondary; a pre-roll is declared."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    a = bench.parse([])
    assert a.xyz == "exact" and a.preroll_ms >= 100 and a.gather == "torch"
    assert bench.parse(["--xyz", "fast"]).xyz == "fast"
    assert bench.CONFIGS["c4"]["views"] == 45 and bench.CONFIGS["c5"]["views"] == 45
    assert bench.CONFIGS["c3"]["views"] == 36
    s = bench.spread([3.0, 1.0, 2.0])
    assert s["min"] == 1.0 and s["median"] == 2.0 and s["max"] == 3.0 and s["steps"] == [3.0, 1.0, 2.0]


def test_pool_rejects_zero_lanes():
    from structured_light_for_3d_model_replication_amd import core
    with pytest.raises(ValueError):
        core.ReconstructorPool(lanes=0)


def test_bench_defaults_next_stats_and_graph():
    """The headline defaults: next-stats (sl_stack_next) and the hipGraph window, both switchable."""
    import bench
    a = bench.parse([])
    assert a.next_stats and a.graph and a.xyz == "exact"
    assert a.verify and a.single_shot >= 20 and a.strong_leg
    a = bench.parse(["--no-next-stats", "--no-graph", "--no-verify", "--no-strong-leg", "--single-shot", "0"])
    assert not a.next_stats and not a.graph and not a.verify and not a.strong_leg and a.single_shot == 0


def test_full_and_dump_outputs_switches():
    """A plain run is the headline window alone: --full (off by default) turns
    the other legs on, each still behind its own switch; --dump-outputs names
    a directory."""
    import bench
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d", "--steps", "7"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 7 and a.verify and a.cpu_baseline


def test_dump_outputs_writes_float_arrays_and_seeded_samples(tmp_path, monkeypatch):
    """bench.dump_outputs on a stand-in result: small arrays whole, arrays
    over the per-array budget as the same sorted sample on every call, maps
    sampled at the same elements and xyz / bgr at the same rows; only the
    cloud's view_offsets[-1] rows count."""
    import numpy as np
    import torch

    import bench
    from structured_light_for_3d_model_replication_amd import core
    V, H, W, n = 2, 30, 50, 1700
    g = torch.Generator().manual_seed(5)
    col = torch.randint(0, 2048, (V, H, W), dtype=torch.int32, generator=g)
    res = {"col_map": col, "row_map": col + 1, "mask": col % 2 == 0,
           "cloud": core.Cloud(torch.randn((V * H * W, 3), generator=g), torch.randint(0, 256, (V * H * W, 3), generator=g).to(torch.uint8),
                               torch.tensor([0, 700, n]))}

    def load(d):
        return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    info = bench.dump_outputs(str(tmp_path / "whole"), res)
    w = load(tmp_path / "whole")
    assert sorted(w) == ["bgr", "col_map", "mask", "row_map", "view_offsets", "xyz"]
    assert all(v.dtype == (np.float64 if k == "view_offsets" else np.float32) for k, v in w.items())
    np.testing.assert_array_equal(w["col_map"], col.numpy())
    np.testing.assert_array_equal(w["mask"], (col % 2 == 0).numpy())
    np.testing.assert_array_equal(w["xyz"], res["cloud"].xyz[:n].numpy())
    np.testing.assert_array_equal(w["bgr"], res["cloud"].bgr[:n].numpy())
    np.testing.assert_array_equal(w["view_offsets"], [0, 700, n])
    assert info["xyz"] == {"shape": [n, 3], "of": n}

    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 4 * 600)  # 600 map elements, 200 cloud rows
    bench.dump_outputs(str(tmp_path / "s1"), res)
    bench.dump_outputs(str(tmp_path / "s2"), res)
    s1, s2 = load(tmp_path / "s1"), load(tmp_path / "s2")
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k])
    assert s1["col_map"].shape == (600,) and s1["xyz"].shape == (200, 3) and s1["bgr"].shape == (200, 3)
    np.testing.assert_array_equal(s1["row_map"], s1["col_map"] + 1)  # the same elements
    np.testing.assert_array_equal(s1["mask"], s1["col_map"] % 2 == 0)
    # the sample is a sorted subset of the whole array's elements / rows
    flat = col.numpy().reshape(-1)
    idx, rows = bench.dump_sample(flat.size, 1), bench.dump_sample(n, 3)
    assert len(np.unique(idx)) == 600 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < flat.size
    assert len(np.unique(rows)) == 200 and np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < n
    assert bench.dump_sample(600, 1) is None and bench.dump_sample(200, 3) is None
    np.testing.assert_array_equal(s1["col_map"], flat[idx])
    np.testing.assert_array_equal(s1["xyz"], res["cloud"].xyz[:n].numpy()[rows])
    np.testing.assert_array_equal(s1["bgr"], res["cloud"].bgr[:n].numpy()[rows])


def test_committed_traffic_profiles_match_the_configs():
    """bench.py attaches <bench.TRAFFIC_DIR>/traffic_<config>.json (the
    directory bench.py itself reads by default) to a line only when the profile's workload is the line's (config, views per GPU,
    decide path, exact xyz): every config of the bench but c1 has one that
    matches, with calibrated per-kernel bytes that add up."""
    sys.path.insert(0, REPO)
    import bench
    for name in ("c2", "c3", "c4", "c5"):
        path = os.path.join(REPO, bench.TRAFFIC_DIR, f"traffic_{name}.json")
        tj = json.load(open(path))
        assert tj["config"] == name and tj["views"] == bench.CONFIGS[name]["views"], name
        assert tj["decide"] is True and tj["xyz"] == "exact" and tj["calibration"], name
        assert abs(sum(tj["kernels"].values()) - tj["bytes_per_step"]) <= 1e-6 * tj["bytes_per_step"], name
        assert "k_decode" in tj["kernels"] and "k_cloud" in tj["kernels"], name
        c = bench.CONFIGS[name]
        S = c.get("streams", 1)
        want_ring = S * -(-c["ring"] // S) if "ring" in c else 1  # bench.py: the ring rounded up to the lanes
        assert tj.get("ring", 1) == want_ring, name


def test_ideal_strong_efficiency_of_the_c3_shards():
    """the 8-GPU strong leg is capped by its 5-vs-4-view shards."""
    sys.path.insert(0, REPO)
    import bench
    assert bench.ideal_strong_efficiency(36, 8) == pytest.approx(0.9)
    assert [bench.ideal_strong_efficiency(36, n) for n in (1, 2, 3, 4)] == [1.0, 1.0, 1.0, 1.0]
