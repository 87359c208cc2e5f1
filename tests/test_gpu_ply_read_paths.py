"""The device PLY reader on the paths tests/test_gpu_ply_read.py never reaches:
bodies past one pass of k_ply_scan, both sides of the run-of-blanks rule, the
host's fetch of undecided tokens in several runs, a fresh context on a side
stream, the scratch the reader shares with the cloud writer, the binary types'
special values, the header and column routes of ply.py, and bodies that end
flush with a load or a chunk.  The yardstick is that module's: the host reader's
bit patterns, and ``info`` -- an accepted file must come through the device path.
Every case's precondition is proved on the CPU in tests/test_ply_read_oracle.py."""
import numpy as np
import pytest
import torch

from structured_light_for_3d_model_replication_amd import _lib, ply
from tests import ply_read_cases as cases
from tests import ply_read_oracle as oracle
from tests.test_gpu_ply_read import _bits, _check_device, _file, _same_as_host

pytestmark = pytest.mark.gpu


def _check_host(f, status, undecided=0):
    got = ply.read_cloud_device(f)
    assert got["info"] == {"path": "host", "undecided": undecided, "status": status}
    _same_as_host(f, got)
    return got


def _check_raises(f, exc, status, monkeypatch):
    """Both readers raise `exc`; the device reader on the host path, for `status`."""
    seen, real = [], ply._host_cloud

    def host_cloud(filename, dev, st, undecided=0):
        seen.append(st)
        return real(filename, dev, st, undecided)

    monkeypatch.setattr(ply, "_host_cloud", host_cloud)
    with pytest.raises(exc):
        ply.read_ply(f)
    with pytest.raises(exc):
        ply.read_cloud_device(f)
    assert seen == [status]


# ---- 1: beyond one scan pass ----
@pytest.mark.parametrize("nb", [1024, 1025])
def test_dense_body(nb, tmp_path):
    case = cases.dense_case(nb)
    got = _check_device(_file(tmp_path, case.name, case.data))
    assert len(got["points"]) == case.n


def test_sparse_body(tmp_path):
    case = cases.sparse_case()
    got = _check_device(_file(tmp_path, case.name, case.data))
    assert len(got["points"]) == case.n


# ---- 2: the run of blanks looked through for a line break ----
@pytest.mark.parametrize("shape", cases.RUN_SHAPES)
def test_run_max_blanks_are_looked_through(shape, tmp_path):
    case = cases.run_case(shape, oracle.RUN_MAX)
    _check_device(_file(tmp_path, case.name, case.data))


@pytest.mark.parametrize("shape", cases.RUN_SHAPES)
def test_one_blank_past_run_max_goes_to_the_host(shape, tmp_path):
    case = cases.run_case(shape, oracle.RUN_MAX + 1)
    assert case.status == oracle.RAGGED_LINE == _lib.SL_PLY_RAGGED_LINE
    _check_host(_file(tmp_path, case.name, case.data), case.status)


# ---- 3: undecided tokens in several runs ----
def test_undecided_runs(tmp_path):
    case = cases.undecided_runs_case()
    _check_device(_file(tmp_path, case.name, case.data), undecided=case.undecided)


def test_undecided_span_limit(tmp_path):
    case = cases.undecided_span_case()
    _check_device(_file(tmp_path, case.name, case.data), undecided=case.undecided)


def test_undecided_list_exactly_full(tmp_path, monkeypatch):
    case = cases.undecided_runs_case()
    monkeypatch.setattr(ply, "_UNDECIDED_CAP", case.undecided)
    _check_device(_file(tmp_path, case.name, case.data), undecided=case.undecided)


def test_undecided_list_one_short(tmp_path, monkeypatch):
    case = cases.undecided_runs_case()
    monkeypatch.setattr(ply, "_UNDECIDED_CAP", case.undecided - 1)
    assert oracle.UNDECIDED_OVERFLOW == _lib.SL_PLY_UNDECIDED_OVERFLOW
    _check_host(_file(tmp_path, case.name, case.data), oracle.UNDECIDED_OVERFLOW, undecided=case.undecided)


def test_undecided_capacity_zero(tmp_path, monkeypatch):
    case = cases.shape_cases_by_name()["rows257_cols6"]
    monkeypatch.setattr(ply, "_UNDECIDED_CAP", 0)
    _check_device(_file(tmp_path, case.name, case.data))


# ---- 4: streams and contexts ----
def _stream_files(tmp_path):
    tier, dense = cases.tier_case(), cases.dense_case(1025)
    return {"tier_edges": (_file(tmp_path, "tier_edges", tier.data), tier.undecided),
            "binary_odd": (_file(tmp_path, "binary_odd", cases.binary_odd_file()), 0),
            "dense_1025": (_file(tmp_path, "dense_1025", dense.data), 0),
            "one_row": (_file(tmp_path, "one_row", cases.one_row_file()), 0)}


@pytest.mark.parametrize("name", ["tier_edges", "binary_odd", "dense_1025"])
def test_first_call_of_a_fresh_context_on_a_side_stream(name, tmp_path, monkeypatch):
    f, undecided = _stream_files(tmp_path)[name]
    monkeypatch.setattr(ply, "_WRITERS", {})
    side = torch.cuda.Stream()
    got = ply.read_cloud_device(f, stream=side)  # the context's first call: all its scratch is new
    assert len(ply._WRITERS) == 1
    assert got["info"] == {"path": "device", "undecided": undecided, "status": 0}
    side.synchronize()
    _same_as_host(f, got)


def _reads_and_writes_interleaved(tmp_path):
    """Reader and cloud writer share d_ply_bsum / d_ply_boff: sizes that shrink and grow, in one context."""
    files = _stream_files(tmp_path)
    clouds = {n: cases.write_cloud(n, n) for n in (300000, 3)}
    dev = {n: (torch.from_numpy(P).cuda(), torch.from_numpy(C).cuda()) for n, (P, C) in clouds.items()}
    torch.cuda.synchronize()

    def read(name):
        f, undecided = files[name]
        _check_device(f, undecided=undecided)

    def write(n):
        got, want = str(tmp_path / f"device_{n}.ply"), str(tmp_path / f"host_{n}.ply")
        ply.save_ply_device(*dev[n], got)
        ply.save_ply(*clouds[n], want)
        assert open(got, "rb").read() == open(want, "rb").read()

    read("dense_1025")
    read("one_row")
    write(300000)
    read("tier_edges")
    write(3)
    read("dense_1025")
    read("one_row")
    return files, dev


def test_reader_and_writer_share_a_context(tmp_path, monkeypatch):
    monkeypatch.setattr(ply, "_WRITERS", {})
    _reads_and_writes_interleaved(tmp_path)
    assert len(ply._WRITERS) == 1


def test_reader_and_writer_share_a_context_on_a_side_stream(tmp_path, monkeypatch):
    monkeypatch.setattr(ply, "_WRITERS", {})
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        kept = _reads_and_writes_interleaved(tmp_path)
        side.synchronize()
    assert len(ply._WRITERS) == 1
    del kept


# ---- 5: binary values ----
@pytest.mark.parametrize("kind", ["float", "double"])
def test_binary_specials(kind, tmp_path):
    got = _check_device(_file(tmp_path, f"specials_{kind}", cases.binary_specials_file(kind)))
    bits = cases.specials_bits(kind)
    want = bits if kind == "double" else \
        np.array([[cases.widen_f32_bits(int(v)) for v in row] for row in bits], dtype=np.uint64)
    table = torch.cat([got["points"], got["normals"]], 1).cpu().numpy()
    np.testing.assert_array_equal(table.view(np.uint64), want)  # subnormals, signed zeros and NaN payloads survive


@pytest.mark.parametrize("type_name", cases.INT_TYPES)
def test_binary_int_extremes(type_name, tmp_path):
    for n in cases.INT_ROWS:
        data, V = cases.int_extremes(type_name, n)
        got = _check_device(_file(tmp_path, f"{type_name}_{n}", data))
        np.testing.assert_array_equal(_bits(got["points"].cpu().numpy()), _bits(V[:, :3].astype(np.float64)))


def test_binary_body_one_byte_short(tmp_path, monkeypatch):
    f = _file(tmp_path, "short", cases.binary_plain_file(delta=-1))
    _check_raises(f, ValueError, ply.SL_PLY_HEADER, monkeypatch)


def test_binary_body_seven_bytes_long(tmp_path):
    got = _check_device(_file(tmp_path, "long", cases.binary_plain_file(delta=7)))
    P, C = ply.read_ply(_file(tmp_path, "exact", cases.binary_plain_file()))
    assert P.shape == (5, 3)
    np.testing.assert_array_equal(_bits(got["points"].cpu().numpy()), _bits(P))
    np.testing.assert_array_equal(got["colors"].cpu().numpy(), C)


def test_binary_property_name_twice(tmp_path, monkeypatch):
    f = _file(tmp_path, "twice", cases.binary_x_twice_file())
    _check_raises(f, ValueError, ply.SL_PLY_HEADER, monkeypatch)


# ---- 6: header and column routes ----
@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_header_longer_than_the_first_probe(fmt, tmp_path):
    got = _check_device(_file(tmp_path, "long_header", cases.long_header_file(fmt)))
    assert len(got["points"]) == 257 and got["colors"] is not None


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_scattered_columns(fmt, tmp_path):
    got = _check_device(_file(tmp_path, "scattered", cases.scattered_file(fmt)))
    assert got["normals"] is not None and got["colors"] is not None
    assert all(got[k].is_contiguous() for k in ("points", "normals", "colors"))


def test_ascii_property_name_twice(tmp_path):
    case = cases.x_twice_case()
    got = _check_device(_file(tmp_path, case.name, case.data))
    last = np.array([float(t) for t in case.body.split()]).reshape(case.n, 4)[:, 3]
    np.testing.assert_array_equal(_bits(got["points"][:, 0].cpu().numpy()), _bits(last))  # the last x wins


def test_no_vertices_but_rows(tmp_path):
    got = _check_host(_file(tmp_path, "n0", cases.n0_two_rows_file()), oracle.TOKEN_COUNT)
    assert tuple(got["points"].shape) == (0, 3)


@pytest.mark.filterwarnings("ignore:loadtxt. input contained no data")
def test_vertices_but_no_body(tmp_path, monkeypatch):
    _check_raises(_file(tmp_path, "n2", cases.n2_empty_file()), IndexError, oracle.TOKEN_COUNT, monkeypatch)


def test_face_element_behind_the_vertices(tmp_path, monkeypatch):
    _check_raises(_file(tmp_path, "face", cases.face_element_file()), ValueError, ply.SL_PLY_HEADER, monkeypatch)


# ---- 7: ends and starts ----
@pytest.mark.parametrize("case", cases.end_cases(), ids=lambda c: c.name)
def test_body_end(case, tmp_path):
    got = _check_device(_file(tmp_path, case.name, case.data))
    assert len(got["points"]) == case.n
