"""tests/bpa_oracle.py, the CPU statement of ball pivoting the GPU is checked
against (tests/test_gpu_bpa.py): its neighbourhood form against its brute-force
definition form, and properties of every case's mesh checked in this file's own
arithmetic (np.cross, np.linalg, math.fsum -- none of the oracle's helpers)."""
import math

import numpy as np
import pytest

from tests import bpa_oracle as bo

SMALL = [name for name in bo.CASES if len(bo.CASES[name]()[0]) <= 80]


def test_the_small_cases_are_there():
    assert {"empty", "one_point", "two_points", "triangle_above", "triangle_below", "strict_closed", "strict_open",
            "patch", "patch_flipped", "patch_one_incompatible", "single_cell", "lattice"} <= set(SMALL)


@pytest.mark.parametrize("name", SMALL)
def test_brute_force_equals_the_neighbourhood_form(name):
    s = bo.solved(name)
    for r, want in zip(s["radii"], s["candidates"]):
        np.testing.assert_array_equal(bo.candidates_brute(s["P"], s["N"], r), want)
    # and with the classes of the finished mesh: inner vertices are no candidates' vertices
    cls = bo.vertex_classes(s["T"], len(s["P"]))
    r = s["radii"][-1]
    got = bo.candidates(s["P"], s["N"], r, cls)
    np.testing.assert_array_equal(bo.candidates_brute(s["P"], s["N"], r, cls), got)
    assert not (cls[got] == bo.INNER).any()


def _edges(T):
    S = np.sort(T, 1)
    return [tuple(e) for t in S.tolist() for e in ((t[0], t[1]), (t[1], t[2]), (t[0], t[2]))]


def _ball_centre(p0, p1, p2, r):
    """The centre of the ball of radius r through the three points on the side of (p1 - p0) x (p2 - p0):
    the circumcentre from the perpendicular-bisector equations (a linear solve), not the barycentric form."""
    e1, e2 = p1 - p0, p2 - p0
    n = np.cross(e1, e2)
    A = np.stack([e1, e2, n])
    rhs = np.array([0.5 * math.fsum(e1 * e1), 0.5 * math.fsum(e2 * e2), 0.0])
    u = np.linalg.solve(A, rhs)  # cc - p0
    h2 = r * r - math.fsum(u * u)
    return p0 + u + n / math.sqrt(math.fsum(n * n)) * math.sqrt(max(h2, 0.0)), h2


@pytest.mark.parametrize("name", sorted(bo.CASES))
def test_mesh_properties(name):
    s = bo.solved(name)
    P, N, T, info = s["P"], s["N"], s["T"], s["info"]
    assert T.dtype == np.int32 and T.shape == (len(T), 3)
    assert sum(info["triangles"]) == len(T) and sum(info["passes"]) == len(info["triangles"]) == len(info["dropped"])
    assert info["converged"]
    # no edge has more than two triangles, no sorted triple appears twice
    counts = {}
    for e in _edges(T):
        counts[e] = counts.get(e, 0) + 1
    assert max(counts.values(), default=0) <= 2
    assert sum(1 for v in counts.values() if v == 1) == info["border_edges"]
    assert len({tuple(t) for t in np.sort(T, 1).tolist()}) == len(T)
    # per pass: which radius appended the triangle
    radius_of = np.repeat(np.repeat(s["radii"], info["passes"]), info["triangles"])
    assert len(radius_of) == len(T)
    for t, r in zip(T.tolist(), radius_of.tolist()):
        p0, p1, p2 = P[t[0]], P[t[1]], P[t[2]]
        n = np.cross(p1 - p0, p2 - p0)
        assert all(float(n @ N[v]) > 0.0 for v in t)  # the winding agrees with all three vertex normals
        o, h2 = _ball_centre(p0, p1, p2, r)
        assert h2 >= -1e-9 * r * r  # the circumradius is at most r
        d = P - o
        d2 = np.einsum("ij,ij->i", d, d)
        d2[t] = np.inf
        # f64 rounding is about 1e-15 relative: the margin only forgives rounding
        assert (d2 >= r * r * (1.0 - 1e-9)).all()


def test_trivial_cases():
    for name in ("empty", "one_point", "two_points", "triangle_below", "strict_closed"):
        assert len(bo.solved(name)["T"]) == 0
    assert bo.solved("triangle_above")["T"].tolist() == [[0, 1, 2]]
    assert bo.ball_pivoting(bo._TRI, -bo._up(3), [0.61])[0].tolist() == [[0, 2, 1]]


def test_strict_boundary():
    """The pair at distance exactly 2 r is no neighbour; one ulp more radius and it is."""
    assert bo.solved("strict_closed")["radii"] == [1.0]
    assert len(bo.solved("strict_closed")["candidates"][0]) == 0
    assert bo.solved("strict_open")["radii"] == [np.nextafter(1.0, 2.0)]
    assert bo.solved("strict_open")["T"].tolist() == [[0, 1, 2]]


def test_flipped_normals_swap_the_winding():
    a, b = bo.solved("patch")["T"], bo.solved("patch_flipped")["T"]
    assert len(a) > 60
    np.testing.assert_array_equal(b, a[:, [0, 2, 1]])


def test_one_incompatible_normal_removes_its_triangles():
    a, b = bo.solved("patch")["T"], bo.solved("patch_one_incompatible")["T"]
    v = bo.PATCH_ODD_VERTEX
    at_v = (a == v).any(1)
    assert 3 <= at_v.sum() < len(a)
    np.testing.assert_array_equal(b, a[~at_v])


def test_the_sphere_closes():
    s = bo.solved("sphere_1500")
    n, T = len(s["P"]), s["T"]
    assert n == 1500 and len(T) == 2 * n - 4
    counts = {}
    for e in _edges(T):
        counts[e] = counts.get(e, 0) + 1
    assert set(counts.values()) == {2} and len(counts) == 3 * n - 6  # V - E + F = 2
    assert s["info"]["border_edges"] == 0
    p0, p1, p2 = (s["P"][T[:, a]] for a in range(3))
    area = 0.5 * np.linalg.norm(np.cross(p1 - p0, p2 - p0), axis=1).sum()
    assert 12.4 < area < 4.0 * math.pi


def test_the_cases_reach_their_rules():
    # rule 5 drops triangles on the jittered grid and between the two sheets
    assert any(d > 0 for d in bo.solved("jittered_grid")["info"]["dropped"])
    assert len(bo.solved("jittered_grid")["P"]) == 38 * 38
    # the hole: open after the first radius (its passes end), filled by more than one pass of the second
    info = bo.solved("hole_fill")["info"]
    first = info["passes"][0]
    assert info["passes"][1] >= 3 and all(t > 0 for t in info["triangles"][first:first + 2])
    s = bo.solved("hole_fill")
    T1 = s["T"][:sum(info["triangles"][:first])]
    counts = {}
    for e in _edges(T1):
        counts[e] = counts.get(e, 0) + 1
    rim = [e for e, v in counts.items() if v == 1
           and all(np.hypot(*(s["P"][u][:2] - 6.0)) < 3.0 for u in e)]
    assert len(rim) >= 6  # a hole of six or more sides
    final = {}
    for e in _edges(s["T"]):
        final[e] = final.get(e, 0) + 1
    assert all(final[e] == 2 for e in rim)  # the second radius has closed it
    # the seed rule: at the second radius there are candidates with no edge in the mesh that are not all orphans
    cls = bo.vertex_classes(T1, len(s["P"]))
    C = bo.candidates(s["P"], s["N"], s["radii"][1], cls)
    have = set(_edges(T1))
    loose = [t for t in C.tolist() if not any(e in have for e in _edges(np.array([t])))]
    assert loose and all((cls[t] != bo.ORPHAN).any() for t in loose)
    # the dense blob: every neighbourhood holds every point, several staging tiles of 64
    s = bo.solved("dense_blob")
    d = s["P"][:, None, :] - s["P"][None, :, :]
    assert len(s["P"]) == 400 and (np.einsum("ijk,ijk->ij", d, d) < 4.0 * s["radii"][0] ** 2).all()
    # the shuffled sheet's second radius: more candidates than one sort tile (4096) holds, in whatever order
    # they arrive; ordered by their third index, rows 4095 and 4096 share it, and many share their first two
    C = np.sort(bo.solved("shuffled")["candidates"][1], 1)
    third = np.sort(C[:, 2], kind="stable")
    assert len(C) > 4096 and third[4095] == third[4096]
    assert len(np.unique(C[:, :2], axis=0)) < len(C) - 1000
    # the duplicates: zero distances
    P = bo.solved("duplicates")["P"]
    assert len(np.unique(P, axis=0)) < len(P)
    # the lattice: exact integers
    assert (bo.solved("lattice")["P"] == np.round(bo.solved("lattice")["P"])).all()
    # two sheets closer than 2 r, opposite normals
    s = bo.solved("two_sheets")
    assert 0.9 < 2 * s["radii"][0] and (s["N"][:, 2] > 0).any() and (s["N"][:, 2] < 0).any()
    # a triangle never joins the two sheets
    assert (np.ptp(s["N"][s["T"]][:, :, 2], axis=1) == 0).all()
