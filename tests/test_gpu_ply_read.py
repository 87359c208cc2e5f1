"""PLY clouds read on the GPU (ply.read_cloud_device: sl_parse_ply_ascii,
sl_unpack_ply_binary) against today's host reader (ply.read_ply /
read_normals, the yardstick), bit for bit -- the bit patterns are compared, so
-0.0 and 0.0 stay apart -- and ``info`` with them: a file the rule set accepts
(tests/ply_read_oracle.py, proved on the CPU in tests/test_ply_read_oracle.py)
must come through the device path, so no test passes by falling back."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from structured_light_for_3d_model_replication_amd import _lib, ply
from tests import ply_read_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.ply")))
COLOURS = ("red", "green", "blue")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_as_host(f, got):
    """got (read_cloud_device's dict) == read_ply / read_normals of the file."""
    P, C = ply.read_ply(f)
    N = ply.read_normals(f)
    assert got["points"].dtype == torch.float64 and tuple(got["points"].shape) == P.shape
    np.testing.assert_array_equal(_bits(got["points"].cpu().numpy()), _bits(P))
    if all(c in ply._read_columns(f) for c in COLOURS):
        assert got["colors"].dtype == torch.uint8
        np.testing.assert_array_equal(got["colors"].cpu().numpy(), C)
    else:
        assert got["colors"] is None and not C.any()
    assert (got["normals"] is None) == (N is None)
    if N is not None:
        assert got["normals"].dtype == torch.float64
        np.testing.assert_array_equal(_bits(got["normals"].cpu().numpy()), _bits(N))


def _check_device(f, undecided=0):
    got = ply.read_cloud_device(f)
    assert got["info"] == {"path": "device", "undecided": undecided, "status": 0}
    assert got["points"].is_cuda
    _same_as_host(f, got)
    return got


def _file(tmp_path, name, data):
    f = str(tmp_path / f"{name}.ply")
    with open(f, "wb") as fh:
        fh.write(data)
    return f


# ---- 1: the golden files and a large-magnitude %.4f cloud ----
@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_golden_file(path):
    _check_device(path)


def test_six_golden_files():
    assert len(GOLDEN) == 6


def test_large_fixed_point_cloud(tmp_path):
    P, C = cases.big_cloud()
    f = str(tmp_path / "big.ply")
    ply.save_ply(P, C, f)
    _check_device(f)


# ---- 2: tier edges ----
def test_tier_edges(tmp_path):
    case = cases.tier_case()
    _check_device(_file(tmp_path, case.name, case.data), undecided=case.undecided)
    # which tokens the kernel left to the host: the undecided list itself
    eng = ply._io_engine(None)
    body = torch.frombuffer(bytearray(case.body), dtype=torch.uint8).cuda()
    ntok = len(case.tiers)
    table = torch.full((ntok,), 7.0, dtype=torch.float64, device="cuda")
    und = torch.full((64, 3), -1, dtype=torch.int64, device="cuda")
    k, code = ctypes.c_int64(), ctypes.c_int(-1)
    with eng._lock:
        _lib.check(eng._L.sl_parse_ply_ascii(eng._ctx, body.data_ptr(), body.numel(), case.n, 3, table.data_ptr(),
                                             und.data_ptr(), 64, ctypes.byref(k), ctypes.byref(code),
                                             torch.cuda.current_stream().cuda_stream), eng._ctx, "parse")
    assert code.value == 0 and k.value == case.undecided
    u = und.cpu().numpy()[: k.value]
    assert sorted(u[:, 0]) == [i for i, t in enumerate(case.tiers) if t == "undecided"]
    toks = case.body.split()
    for t, off, ln in u:
        assert case.body[off:off + ln] == toks[t]
    np.testing.assert_array_equal(_bits(table.cpu().numpy()), _bits([float(t) for t in toks]))


# ---- 3: shapes ----
@pytest.mark.parametrize("case", cases.shape_cases(), ids=lambda c: c.name)
def test_shape(case, tmp_path):
    got = _check_device(_file(tmp_path, case.name, case.data))
    assert len(got["points"]) == case.n


# ---- 4: whole-file conditions ----
@pytest.mark.parametrize("case", cases.host_cases(), ids=lambda c: c.name)
def test_whole_file_condition(case, tmp_path, monkeypatch):
    f = _file(tmp_path, case.name, case.data)
    monkeypatch.setattr(ply, "_UNDECIDED_CAP", case.cap)
    try:
        ply.read_ply(f)
    except Exception as e:  # noqa: BLE001 -- whatever today's reader raises is the file's
        with pytest.raises(type(e)):
            ply.read_cloud_device(f)
        return
    got = ply.read_cloud_device(f)
    assert got["info"] == {"path": "host", "undecided": case.undecided, "status": case.status}
    _same_as_host(f, got)


def test_header_the_device_path_does_not_take(tmp_path):
    f = _file(tmp_path, "big_endian", cases.header(1, cases.XYZ, "binary_big_endian") + b"\0" * 12)
    with pytest.raises(ValueError):
        ply.read_ply(f)
    with pytest.raises(ValueError):
        ply.read_cloud_device(f)


# ---- 5: binary ----
@pytest.mark.parametrize("n", [0, 1, 4097])
@pytest.mark.parametrize("layout", ["save_ply", "open3d", "open3d_normals"])
def test_binary(layout, n, tmp_path):
    rng = np.random.default_rng(n + 3)
    P = rng.normal(0, 300, (n, 3))
    C = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    f = str(tmp_path / "b.ply")
    if layout == "save_ply":
        ply.save_ply(P, C, f, binary=True)
    else:
        ply.save_ply_open3d(P, C, f, normals=rng.normal(0, 1, (n, 3)) if layout == "open3d_normals" else None)
    stride = {"save_ply": 15, "open3d": 27, "open3d_normals": 51}[layout]
    assert os.path.getsize(f) - open(f, "rb").read().find(b"end_header\n") - 11 == n * stride
    _check_device(f)


def test_binary_small_types_at_odd_offsets(tmp_path):
    _check_device(_file(tmp_path, "odd", cases.binary_odd_file()))


# ---- 6: the drop-ins load through it, once per file ----
def _host_reader(filename, device=None, stream=None):
    P, C = ply.read_ply(filename)
    N = ply.read_normals(filename)
    has = all(c in ply._read_columns(filename) for c in COLOURS)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return {"points": to(P), "colors": to(C) if has else None, "normals": None if N is None else to(N),
            "info": {"path": "host", "undecided": 0, "status": 0}}


def test_drop_ins_read_each_file_once(tmp_path, monkeypatch):
    import builtins

    from structured_light_for_3d_model_replication_amd.processing import ProcessingLogic
    rng = np.random.default_rng(11)
    P = np.concatenate([rng.normal(0, 5, (600, 3)), rng.normal(0, 200, (12, 3))])
    C = rng.integers(0, 256, (len(P), 3)).astype(np.uint8)
    src, mesh_src = str(tmp_path / "view.ply"), str(tmp_path / "merged.ply")
    ply.save_ply(P, C, src)
    Nn = rng.normal(0, 1, P.shape)
    ply.save_ply_open3d(P, C, mesh_src, normals=Nn / np.linalg.norm(Nn, axis=1, keepdims=True), binary=False)
    opened = []

    def counting_open(file, *a, **k):
        opened.append(str(file))
        return builtins.open(file, *a, **k)

    monkeypatch.setattr(ply, "open", counting_open, raising=False)
    kept = ProcessingLogic.remove_outliers(src, return_obj=True)
    Pm, Nm = ProcessingLogic._load_for_meshing(mesh_src)
    assert opened.count(src) == 1 and opened.count(mesh_src) == 1
    assert ply.read_cloud_device(src)["info"]["path"] == "device"
    assert ply.read_cloud_device(mesh_src)["info"]["path"] == "device"

    monkeypatch.setattr(ply, "read_cloud_device", _host_reader)
    kept_h = ProcessingLogic.remove_outliers(src, return_obj=True)
    Ph, Nh = ProcessingLogic._load_for_meshing(mesh_src)
    assert 0 < len(kept.points) < len(P)
    np.testing.assert_array_equal(_bits(kept.points.cpu().numpy()), _bits(kept_h.points.cpu().numpy()))
    np.testing.assert_array_equal(kept.colors.cpu().numpy(), kept_h.colors.cpu().numpy())
    np.testing.assert_array_equal(_bits(Pm.cpu().numpy()), _bits(Ph.cpu().numpy()))
    np.testing.assert_array_equal(_bits(Nm.cpu().numpy()), _bits(Nh.cpu().numpy()))
