"""PLY files for the device reader's tests (tests/test_ply_read_oracle.py proves
each case's precondition on the CPU, tests/test_gpu_ply_read.py reads them on
the GPU).  Every case is the file's bytes plus what the rule set
(tests/ply_read_oracle.py) must say about it."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from tests import ply_read_oracle as oracle

XYZ = [("float", "x"), ("float", "y"), ("float", "z")]
RGB = [("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
NORMALS = [("double", "nx"), ("double", "ny"), ("double", "nz")]
XYZ_D = [("double", "x"), ("double", "y"), ("double", "z")]
LAYOUTS = {3: XYZ, 6: XYZ + RGB, 9: XYZ_D + NORMALS + RGB}  # 9: save_ply_open3d's ASCII form

CHUNK = 4096  # bytes of the body per workgroup (csrc/slplyread.inl kPlyrChunk)


def header(n, props, fmt="ascii") -> bytes:
    lines = ["ply", f"format {fmt} 1.0", f"element vertex {n}"] + [f"property {t} {p}" for t, p in props]
    return ("\n".join(lines) + "\nend_header\n").encode("ascii")


@dataclass
class Case:
    name: str
    n: int
    props: list
    body: bytes
    status: int = oracle.ACCEPTED  # what the rule set says of the body
    undecided: int = 0
    cap: int = 1 << 16             # the undecided list's capacity the case is read with
    tiers: list = field(default_factory=list)  # expected tier per token (tier cases only)

    @property
    def data(self) -> bytes:
        return header(self.n, self.props) + self.body

    @property
    def colour_cols(self):
        names = [p for _, p in self.props]
        return [names.index(c) for c in ("red", "green", "blue") if c in names]


# ---- tier edges: (token, tier) ----
TIER_TOKENS = [
    ("9007199254740991", "exact"),       # M = 2^53 - 1
    ("9007199254740992", "exact"),       # M = 2^53
    ("9007199254740993", "undecided"),   # M = 2^53 + 1
    ("900719925474.0992", "exact"),      # M = 2^53 behind a point
    ("-900719925474.0993", "undecided"),
    ("1e22", "exact"),
    ("1e-22", "exact"),
    ("1e23", "undecided"),
    ("1e-23", "undecided"),
    ("9007199254740992e22", "exact"),    # both limits at once
    ("9007199254740991e-22", "exact"),
    ("123.456e24", "exact"),             # p = 24 - 3 = 21
    ("1.5e23", "exact"),                 # p = 22
    ("1.5e24", "undecided"),
    ("1234567890123456789012345", "undecided"),  # 25 digits
    ("0.1234567890123456789012345", "undecided"),
    ("0.00000000000000000000001", "undecided"),  # M = 1, p = -23
    ("0.0000000000000000000001", "exact"),       # M = 1, p = -22
    ("000123.4500", "exact"),
    ("+1.5", "exact"),
    (".5", "exact"),
    ("5.", "exact"),
    ("-.5", "exact"),
    ("1e5", "exact"),
    ("1E-5", "exact"),
    ("1.5e+3", "exact"),
    ("0.3000", "exact"),
    ("0.7000", "exact"),
    ("-0.0000", "exact"),
    ("0", "exact"),
    ("-0", "exact"),
    ("0e0", "exact"),
    ("00000000000000000000000001", "exact"),  # leading zeros drop out
    ("1e400", "undecided"),                    # strtod: inf
    ("1e-400", "undecided"),                   # strtod: 0.0
    ("179769313486231570000000000000000000000e270", "undecided"),
]


def tier_case() -> Case:
    toks = [t for t, _ in TIER_TOKENS]
    tiers = [k for _, k in TIER_TOKENS]
    while len(toks) % 3:
        toks.append("0")
        tiers.append("exact")
    body = "".join(" ".join(toks[i:i + 3]) + "\n" for i in range(0, len(toks), 3)).encode("ascii")
    return Case("tier_edges", len(toks) // 3, XYZ, body, undecided=tiers.count("undecided"), tiers=tiers)


# ---- shapes ----
def _rows(n, ncol, seed):
    """n text rows of a layout: %.4f xyz (+ colours), or %g doubles with normals (exponents among them)."""
    rng = np.random.default_rng(seed)
    P = rng.normal(0.0, 300.0, (n, 3))
    P[::7] *= 1e-6  # %g: exponents; %.4f: "0.0000", "-0.0000"
    C = rng.integers(0, 256, (n, 3))
    if ncol == 3:
        return ["%.4f %.4f %.4f" % tuple(p) for p in P]
    if ncol == 6:
        return ["%.4f %.4f %.4f %d %d %d" % (*p, *c) for p, c in zip(P, C)]
    Nn = rng.normal(0.0, 1.0, (n, 3))
    Nn /= np.linalg.norm(Nn, axis=1, keepdims=True)
    return [" ".join(f"{float(v):g}" for v in (*p, *q)) + " %d %d %d" % tuple(c) for p, q, c in zip(P, Nn, C)]


ROW_COUNTS = (0, 1, 255, 256, 257, 4097)


def shape_cases():
    out = []
    for ncol in (3, 6, 9):
        for n in ROW_COUNTS:
            rows = _rows(n, ncol, 100 * ncol + n % 97)
            out.append(Case(f"rows{n}_cols{ncol}", n, LAYOUTS[ncol], "".join(r + "\n" for r in rows).encode("ascii")))
    rows = _rows(257, 6, 5)
    lf = "".join(r + "\n" for r in rows)
    out.append(Case("no_final_newline", 257, LAYOUTS[6], lf[:-1].encode("ascii")))
    out.append(Case("crlf", 257, LAYOUTS[6], lf.replace("\n", "\r\n").encode("ascii")))
    out.append(Case("tabs_and_runs", 257, LAYOUTS[6],
                    "".join("  " + r.replace(" ", " \t  ", 2).replace(" ", "   ") + " \t\n" for r in rows)
                    .encode("ascii")))
    out.append(Case("blank_lines", 257, LAYOUTS[6],
                    ("\n\n" + "".join(r + ("\n\n" if i % 3 else "\n \t \n\r\n") for i, r in enumerate(rows)) + "\n\n")
                    .encode("ascii")))
    out.append(straddle_case())
    return out


def straddle_case() -> Case:
    """Tokens across a 16-byte load edge and across a workgroup's chunk edge,
    placed with spaces: each "-123.4567" starts 3 bytes before the edge."""
    rows, body = [], b""
    for k, edge in enumerate((16 * 5, 16 * 9 + 16, CHUNK, 2 * CHUNK, 3 * CHUNK + 16 * 7)):
        start = edge - 3
        pad = start - len(body)
        assert pad >= 0
        row = f"-123.4567 {k}.2500 0.{k}001".encode("ascii")
        body += b" " * pad + row + b"\n"
        rows.append(row)
        assert body[start:start + 9] == b"-123.4567" and start // 16 != (start + 8) // 16
    assert len(body) > 3 * CHUNK
    return Case("straddle_edges", len(rows), XYZ, body)


# ---- whole-file conditions: the host reader's result (or exception) is the file's ----
def host_cases():
    r6 = "1.5000 2.5000 3.5000 10 20 30\n"
    und = "".join(f"1e{30 + i} 2 3\n" for i in range(5))
    return [
        Case("nan", 2, XYZ, b"1 2 3\nnan 5 6\n", oracle.BAD_BYTE),
        Case("dangling_exponent", 2, XYZ, b"1 2 3\n4 1e 6\n", oracle.BAD_TOKEN),
        Case("two_points", 2, XYZ, b"1 2 3\n4 1.2.3 6\n", oracle.BAD_TOKEN),
        Case("ragged_right_total", 2, XYZ, b"1 2 3 4\n5 6\n", oracle.RAGGED_LINE),
        Case("one_token_short", 2, XYZ, b"1 2 3\n4 5\n", oracle.TOKEN_COUNT),
        Case("one_row_more", 2, XYZ, b"1 2 3\n4 5 6\n7 8 9\n", oracle.TOKEN_COUNT),
        Case("colour_256", 2, XYZ + RGB, (r6 + "1 2 3 0 256 0\n").encode("ascii"), oracle.COLOUR_RANGE),
        Case("colour_fraction", 2, XYZ + RGB, (r6 + "1 2 3 0 12.5 0\n").encode("ascii"), oracle.COLOUR_RANGE),
        Case("hash_comment", 2, XYZ, b"1 2 3 # first\n4 5 6\n", oracle.BAD_BYTE),
        Case("undecided_overflow", 5, XYZ, und.encode("ascii"), oracle.UNDECIDED_OVERFLOW, undecided=5, cap=4),
    ]


def accepted_cases():
    return [tier_case()] + shape_cases()


def big_cloud(n=1000, seed=4):
    """Points for save_ply's %.4f with |x| up to 8.9e11: the significand reaches 8.9e15, below 2^53."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-8.9e11, 8.9e11, (n, 3))
    P[0] = (8.9e11 - 0.00005, -8.9e11 + 0.00005, 0.00004)
    return P, rng.integers(0, 256, (n, 3)).astype(np.uint8)


# ---- binary: every type of ply._PLY_TYPES but uint at odd offsets ----
ODD_PROPS = [("char", "pad"), ("double", "x"), ("short", "y"), ("int", "z"), ("ushort", "nx"), ("float", "ny"),
             ("char", "nz"), ("uchar", "red"), ("ushort", "green"), ("uchar", "blue"), ("uint", "tail")]
_NP = {"char": "i1", "double": "<f8", "short": "<i2", "int": "<i4", "ushort": "<u2", "float": "<f4",
       "uchar": "u1", "uint": "<u4"}


def binary_odd_file(n=257, seed=9) -> bytes:
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=np.dtype([(p, _NP[t]) for t, p in ODD_PROPS]))
    assert rec.dtype.itemsize == 30 and rec.dtype.fields["x"][1] == 1 and rec.dtype.fields["z"][1] == 11
    rec["pad"] = rng.integers(-128, 128, n)
    rec["x"] = rng.normal(0, 1e3, n)
    rec["y"] = rng.integers(-32768, 32768, n)
    rec["z"] = rng.integers(-2 ** 31, 2 ** 31, n)
    rec["nx"] = rng.integers(0, 65536, n)
    rec["ny"] = rng.normal(0, 1, n).astype(np.float32)
    rec["nz"] = rng.integers(-128, 128, n)
    rec["red"] = rng.integers(0, 256, n)
    rec["green"] = rng.integers(0, 256, n)  # a ushort colour within 0..255
    rec["blue"] = rng.integers(0, 256, n)
    rec["tail"] = rng.integers(0, 2 ** 32, n)
    return header(n, ODD_PROPS, "binary_little_endian") + rec.tobytes()
