"""ASCII PLY writer, byte-identical to the reference's.

Format of server/sl_system.py:671-691 (== multi_point_cloud_process.py:121-131,
Old/process_cloud.py:200-219): ASCII header, then per point
``"%.4f %.4f %.4f %d %d %d\\n"`` with the colour swapped from BGR to RGB.

The reference formats one point per Python f-string (~0.3 Mpt/s).  Here the
text is produced by libslgpu's host formatter (``sl_format_ply`` /
``sl_write_ply``): correctly rounded %.4f (ties to even, as CPython's
``PyOS_double_to_string``) from exact 128-bit integer arithmetic, on several
threads.  ``tests/test_ply_io.py`` pins the bytes against the reference's own
PLY output and against CPython's formatting on edge values.

Reading: ``read_ply`` / ``read_normals`` parse a vertex-only PLY on the host
(NumPy); ``read_cloud_device`` reads the file once and parses the body on the
GPU (``sl_parse_ply_ascii`` / ``sl_unpack_ply_binary``, csrc/slplyread.inl) to
the same values bit for bit, leaving every file it does not fully understand
to the host reader.  ``tests/test_gpu_ply_read.py`` compares the two.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

from . import _lib

_THREADS = max(1, min(16, os.cpu_count() or 1))


def _arrays(points, colors):
    P = np.asarray(points)
    if P.dtype not in (np.float32, np.float64):
        P = P.astype(np.float64)
    P = np.ascontiguousarray(P)
    C = np.ascontiguousarray(np.asarray(colors, dtype=np.uint8))
    n = len(P)
    if len(C) != n:
        raise ValueError("points and colors differ in length")
    if n and (P.shape[1:] != (3,) or C.shape[1:] != (3,)):
        raise ValueError("points and colors must be (N, 3)")
    return P, C, n, (_lib.SL_XYZ_F32 if P.dtype == np.float32 else _lib.SL_XYZ_F64)


def ply_text(points, colors) -> str:
    """The PLY file content as a str."""
    P, C, n, dt = _arrays(points, colors)
    L = _lib.load()
    ln = ctypes.c_int64()
    _lib.check(L.sl_format_ply(P.ctypes.data, dt, C.ctypes.data, n, _THREADS, None, 0, ctypes.byref(ln)),
               None, "sl_format_ply")
    buf = ctypes.create_string_buffer(ln.value)
    _lib.check(L.sl_format_ply(P.ctypes.data, dt, C.ctypes.data, n, _THREADS, buf, ln.value, ctypes.byref(ln)),
               None, "sl_format_ply")
    return buf.raw[: ln.value].decode("ascii")


def save_ply(points, colors, filename, binary: bool = False) -> None:
    """save_ply(points, colors, filename) of multi_point_cloud_process.py:121.

    ``binary=True`` writes binary_little_endian with the same properties
    (float32 xyz, uchar RGB): what Open3D's write_point_cloud writes by default.
    """
    P, C, n, dt = _arrays(points, colors)
    fn = _lib.load().sl_write_ply_binary if binary else _lib.load().sl_write_ply
    _lib.check(fn(os.fsencode(filename), P.ctypes.data, dt, C.ctypes.data, n, _THREADS), None,
               f"cannot write {filename}")


_WRITERS: dict = {}  # device -> a context of its own for device-side PLY formatting and parsing (its scratch, its lock)
_WRITERS_LOCK = threading.Lock()


def save_ply_device(xyz, bgr, filename, stream=None) -> None:
    """save_ply of a cloud in GPU memory (torch tensors: xyz (n, 3) float32 /
    float64, bgr (n, 3) uint8): the text is formatted on the GPU by the same
    digit code as the host formatter (one thread per point), copied back in
    chunks and written -- byte-identical to save_ply(xyz.cpu(), bgr.cpu(),
    filename), without the points' D2H or any host formatting.  A context of
    its own per device keeps the writer off the decoding contexts' locks."""
    _io_engine(xyz.device).write_ply(filename, xyz, bgr, stream)


def save_ply_open3d(points, colors, filename, normals=None, binary: bool = True) -> None:
    """The file o3d.io.write_point_cloud writes for a cloud with points,
    optional normals and colours (processing.py:181): binary little-endian
    (``binary=False``: ASCII) with ``comment Created by Open3D``, double x y z,
    double nx ny nz, uchar red green blue.  ``colors`` are BGR uint8 (written
    as RGB).  Layout restated from Open3D's FilePLY.cpp; unpinned (no Open3D
    in this image)."""
    P = np.ascontiguousarray(np.asarray(points, dtype=np.float64)).reshape(-1, 3)
    C = np.ascontiguousarray(np.asarray(colors, dtype=np.uint8)).reshape(-1, 3)
    n = len(P)
    if len(C) != n or (normals is not None and len(normals) != n):
        raise ValueError("points, colors and normals differ in length")
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    if normals is not None:
        fields += [("nx", "<f8"), ("ny", "<f8"), ("nz", "<f8")]
    fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(n, dtype=np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = P[:, 0], P[:, 1], P[:, 2]
    if normals is not None:
        Nn = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        rec["nx"], rec["ny"], rec["nz"] = Nn[:, 0], Nn[:, 1], Nn[:, 2]
    rec["red"], rec["green"], rec["blue"] = C[:, 2], C[:, 1], C[:, 0]
    tnames = {"<f8": "double", "u1": "uchar"}
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", "comment Created by Open3D",
            f"element vertex {n}"] + [f"property {tnames[t]} {nm}" for nm, t in fields] + ["end_header", ""]
    with open(filename, "wb") as f:
        f.write("\n".join(head).encode("ascii"))
        if binary:
            rec.tofile(f)
        else:
            # rply's ASCII writer: "%g" for doubles, "%d" for uchar, space-separated
            cols = [rec[nm] for nm, _ in fields]
            for i in range(n):
                f.write((" ".join(f"{float(c[i]):g}" if c.dtype.kind == "f" else str(int(c[i])) for c in cols)
                         + "\n").encode("ascii"))


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1",
              "uint8": "u1", "char": "i1", "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2",
              "uint16": "<u2", "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


def read_normals(filename):
    """nx ny nz of a vertex-only PLY (float64 (N,3)), or None when absent."""
    cols = _read_columns(filename)
    if not all(c in cols for c in ("nx", "ny", "nz")):
        return None
    return np.stack([cols["nx"], cols["ny"], cols["nz"]], 1).astype(np.float64)


def _read_columns(filename):
    """{property: column} of a vertex-only PLY (ASCII or binary_little_endian)."""
    with open(filename, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{filename}: not a PLY file")
    head = data[:end].decode("ascii").split("\n")
    fmt, n, props = None, 0, []
    for line in head:
        t = line.split()
        if not t:
            continue
        if t[0] == "format":
            fmt = t[1]
        elif t[0] == "element":
            if t[1] != "vertex":
                raise ValueError(f"{filename}: only vertex elements are supported")
            n = int(t[2])
        elif t[0] == "property":
            if t[1] == "list":
                raise ValueError(f"{filename}: list properties are not supported")
            props.append((t[2], _PLY_TYPES[t[1]]))
    body = data[end + len(b"end_header\n"):]
    names = [p for p, _ in props]
    if fmt == "ascii":
        rows = np.loadtxt(body.decode("ascii").splitlines(), dtype=np.float64, ndmin=2) if n else \
            np.zeros((0, len(props)))
        cols = {p: rows[:, i] for i, p in enumerate(names)}
    elif fmt == "binary_little_endian":
        rec = np.frombuffer(body, dtype=np.dtype(props), count=n)
        cols = {p: rec[p] for p in names}
    else:
        raise ValueError(f"{filename}: unsupported format {fmt}")
    return cols


def read_ply(filename):
    """-> (points float64 (N,3), colors uint8 (N,3) BGR) of a vertex-only PLY
    (ASCII or binary_little_endian), as o3d.io.read_point_cloud feeds
    processing.py:116-182.  Colour is swapped back to BGR, the reference's
    in-memory order; a file without colour gives zeros."""
    cols = _read_columns(filename)
    n = len(cols["x"])
    P = np.stack([cols["x"], cols["y"], cols["z"]], 1).astype(np.float64)
    if all(c in cols for c in ("red", "green", "blue")):
        C = np.stack([cols["blue"], cols["green"], cols["red"]], 1).astype(np.uint8)
    else:
        C = np.zeros((n, 3), np.uint8)
    return P, C


# ------------------------------------------------------------ device reader ----
_UNDECIDED_CAP = 1 << 16  # entries of the undecided list (tokens the host converts with strtod)
_HEAD_PROBE = 1 << 16     # the header is looked for in this many leading bytes first
SL_PLY_HEADER = 7         # info["status"]: the header / layout is not one the device path takes


def _io_engine(device):
    """The PLY I/O context of a device (save_ply_device's)."""
    import torch

    from . import core
    dev = torch.device(device if device is not None else "cuda")
    if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    with _WRITERS_LOCK:
        key = str(dev)
        if key not in _WRITERS:
            _WRITERS[key] = core.Reconstructor(dev)
        return _WRITERS[key]


def _read_pinned(filename):
    """The file's bytes, read once, straight into a pinned buffer -> (uint8 tensor, its numpy view, size)."""
    import torch
    with open(filename, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        buf = torch.empty(max(size, 1), dtype=torch.uint8, pin_memory=True)
        view = buf.numpy()
        mv, got = memoryview(view), 0
        while got < size:
            k = f.readinto(mv[got:size])
            if not k:
                break
            got += k
    return buf, view, got


def _device_layout(view, size):
    """The header by _read_columns' rules -> (fmt, n, props, body offset), or
    None when the device path does not take the file (the host reader then
    returns or raises what it always did)."""
    probe = view[:min(size, _HEAD_PROBE)].tobytes()
    end = probe.find(b"end_header\n")
    if end < 0 and size > _HEAD_PROBE:
        probe = view[:size].tobytes()
        end = probe.find(b"end_header\n")
    if not probe.startswith(b"ply") or end < 0:
        return None
    try:
        head = probe[:end].decode("ascii").split("\n")
        fmt, n, props = None, 0, []
        for line in head:
            t = line.split()
            if not t:
                continue
            if t[0] == "format":
                fmt = t[1]
            elif t[0] == "element":
                if t[1] != "vertex":
                    return None
                n = int(t[2])
            elif t[0] == "property":
                if t[1] == "list":
                    return None
                props.append((t[2], _PLY_TYPES[t[1]]))
    except (ValueError, KeyError, IndexError):
        return None
    names = [p for p, _ in props]
    if fmt not in ("ascii", "binary_little_endian") or n < 0 or not all(c in names for c in "xyz"):
        return None
    if fmt == "binary_little_endian" and len(set(names)) != len(names):
        return None  # np.dtype refuses duplicate names
    return fmt, n, props, end + len(b"end_header\n")


def _host_cloud(filename, dev, status, undecided=0):
    """read_ply + read_normals of the file (one parse), on the device."""
    import torch
    cols = _read_columns(filename)
    P = np.stack([cols["x"], cols["y"], cols["z"]], 1).astype(np.float64)
    C = N = None
    if all(c in cols for c in ("red", "green", "blue")):
        C = np.stack([cols["blue"], cols["green"], cols["red"]], 1).astype(np.uint8)
    if all(c in cols for c in ("nx", "ny", "nz")):
        N = np.stack([cols["nx"], cols["ny"], cols["nz"]], 1).astype(np.float64)
    to = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return {"points": to(P), "colors": to(C), "normals": to(N),
            "info": {"path": "host", "undecided": int(undecided), "status": int(status)}}


def read_cloud_device(filename, device=None, stream=None, *, times=None):
    """A vertex-only PLY (ASCII or binary_little_endian) read once and parsed
    on the GPU -> {"points": f64 [N,3], "colors": u8 [N,3] BGR or None,
    "normals": f64 [N,3] or None, "info": {"path", "undecided", "status"}},
    tensors on ``device``.  Values are ``read_ply`` / ``read_normals``' bit for
    bit.

    The header is parsed here (``_read_columns``' rules); the body goes through
    a pinned buffer to the device, where sl_parse_ply_ascii converts every
    token correctly rounded (undecided ones through the host's strtod:
    ``info["undecided"]``) or sl_unpack_ply_binary widens the records.  A file
    the device path does not take -- ``info["status"]`` says why (SL_PLY_*) --
    is read by ``_read_columns`` instead (``info["path"] == "host"``): its
    values and its exceptions are then that reader's.

    ``times`` (a dict, measurement only): filled with the seconds of the file
    read, the upload and the kernels, each waited for.
    """
    import time

    import torch
    eng = _io_engine(device)
    dev = eng.device
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    t0 = time.perf_counter()
    buf, view, size = _read_pinned(filename)
    t1 = time.perf_counter()
    lay = _device_layout(view, size)
    if lay is None:
        return _host_cloud(filename, dev, SL_PLY_HEADER)
    fmt, n, props, off = lay
    names = [p for p, _ in props]
    ncol, nbody = len(props), size - off
    rec = np.dtype(props) if fmt != "ascii" else None
    if rec is not None and nbody < n * rec.itemsize:
        return _host_cloud(filename, dev, SL_PLY_HEADER)
    if rec is not None:
        nbody = n * rec.itemsize
    with torch.cuda.stream(st):
        body = torch.empty(max(nbody, 1), dtype=torch.uint8, device=dev)
        if nbody:
            body[:nbody].copy_(buf[off:off + nbody], non_blocking=True)
        if times is not None:
            st.synchronize()
        t2 = time.perf_counter()
        table = torch.empty((n, ncol), dtype=torch.float64, device=dev)
        status, n_und = _lib.SL_PLY_ACCEPTED, 0
        if fmt == "ascii":
            cap = _UNDECIDED_CAP
            und = torch.empty((max(cap, 1), 3), dtype=torch.int64, device=dev)
            k, code = ctypes.c_int64(), ctypes.c_int()
            with eng._lock:
                _lib.check(eng._L.sl_parse_ply_ascii(eng._ctx, body.data_ptr(), nbody, n, ncol, table.data_ptr(),
                                                     und.data_ptr(), cap, ctypes.byref(k), ctypes.byref(code),
                                                     st.cuda_stream), eng._ctx, "sl_parse_ply_ascii")
            status, n_und = code.value, k.value
        else:
            offs = (ctypes.c_int * ncol)(*[rec.fields[p][1] for p in names])
            types = (ctypes.c_int * ncol)(*[_lib.SL_PLY_TYPE[t] for _, t in props])
            with eng._lock:
                _lib.check(eng._L.sl_unpack_ply_binary(eng._ctx, body.data_ptr(), n, rec.itemsize, ncol, offs, types,
                                                       table.data_ptr(), st.cuda_stream), eng._ctx,
                           "sl_unpack_ply_binary")
        if status != _lib.SL_PLY_ACCEPTED:
            return _host_cloud(filename, dev, status, n_und)
        at = {p: i for i, p in enumerate(names)}  # a name given twice: the last column, as the host's dict

        def take(*cols):
            if not all(c in at for c in cols):
                return None
            i = [at[c] for c in cols]
            if i[1] == i[0] + 1 and i[2] == i[0] + 2:
                return table[:, i[0]:i[0] + 3].contiguous()
            return table[:, i].contiguous()

        P, N, C = take("x", "y", "z"), take("nx", "ny", "nz"), take("blue", "green", "red")
        if C is not None:
            if not bool(((C >= 0) & (C <= 255) & (C == C.floor())).all()):  # the host's astype(uint8) decides
                return _host_cloud(filename, dev, _lib.SL_PLY_COLOUR_RANGE, n_und)
            C = C.to(torch.uint8)
        if times is not None:
            st.synchronize()
            times.update(read_s=t1 - t0, h2d_s=t2 - t1, kernels_s=time.perf_counter() - t2)
    return {"points": P, "colors": C, "normals": N,
            "info": {"path": "device", "undecided": int(n_und), "status": int(status)}}
