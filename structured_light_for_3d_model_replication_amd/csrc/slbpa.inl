// libslgpu.so, part 2h -- ball-pivoting surface meshing, included at the end of
// slmerge.hip (one translation unit: it shares that file's scratch pool, scan,
// triple sort and search grid, and slprim.inl's finite check and stage clock).
// The reference's reconstruct_stl(mode="surface")
// (server/processing.py:220-237) is Open3D's create_from_point_cloud_ball_pivoting,
// a sequential front that pivots one edge at a time.  It is restated here in an
// order-free form: the surface a ball of radius r can roll over is the set of
// triangles that have an empty r-ball on the side of their normals, and that set
// can be enumerated per point from the point's 2r-neighbourhood alone.  Open3D is
// not in this image, so parity with it is UNPINNED and tests/bpa_oracle.py is the
// CPU restatement the tests check against, exactly.
//
// All arithmetic is f64, uncontracted, in the operation order written.
// d2(u, v) = ((dx dx + dy dy) + dz dz), r2 = r r, R4 = 4 r2.
//
// Candidate triangle at radius r: cloud indices i < j < k, p0, p1, p2 = P[i],
// P[j], P[k], with
//   neighbours     d2(p1, p0) < R4, d2(p2, p0) < R4, d2(p1, p2) < R4 (the strict
//                  nanoflann test);
//   circumcentre   (Open3D's barycentric form) a = d2(p1, p2), b = d2(p2, p0),
//                  c = d2(p0, p1), wa = a ((b + c) - a), wb = b ((a + c) - b),
//                  wc = c ((a + b) - c), s = (wa + wb) + wc > 0,
//                  cc = (p0 (wa / s) + p1 (wb / s)) + p2 (wc / s),
//                  h = r2 - d2(cc, p0) >= 0;
//   normals        e1 = p1 - p0, e2 = p2 - p0, n = (e1y e2z - e1z e2y, e1z e2x -
//                  e1x e2z, e1x e2y - e1y e2x), ln = sqrt((nx nx + ny ny) + nz nz)
//                  > 0; dv = (nx Nv.x + ny Nv.y) + nz Nv.z for v = i, j, k: all
//                  > 0 -> sign +1, all < 0 -> sign -1, else no candidate;
//   ball centre    o = cc + (n / ln) (sign sqrt(h));
//   emptiness      no point q other than i, j, k (by index) among the points with
//                  d2(q, p0) < R4 -- the 2r-neighbourhood of the smallest-index
//                  vertex, which contains every point inside the ball -- has
//                  d2(q, o) < r2;
//   winding        (i, j, k) for sign +1, (i, k, j) for sign -1: the face normal
//                  is on the ball's side;
//   rank           the lexicographic order of the sorted triple (i, j, k).
//
// Vertex classes against the mesh so far (Open3D's vertex types): 0 orphan (in
// no triangle), 1 border (on an edge with exactly one triangle), 2 inner (used,
// on no such edge).  sl_ball_pivot_candidates enumerates the candidates whose
// three vertices are all non-inner, in rank order.
//
// A pass at radius r over the mesh M (mesh.py keeps this bookkeeping on the
// device; everything is judged against the snapshot of M, so nothing depends on
// an order):
//   1. the candidates whose three vertices are all non-inner;
//   2. without those whose sorted triple is in M;
//   3. without those that have an edge with two or more triangles in M;
//   4. without those that have no edge in M, unless all three vertices are
//      orphans (the seed rule);
//   5. per edge, the survivors on it in rank order: only the first 2 -
//      count_M(edge) stay; a triangle dropped at any of its edges is dropped (one
//      application is enough: dropping only lowers counts), so no edge ever has
//      more than two triangles;
//   6. the survivors are appended to M in rank order.
// A radius: passes until one appends nothing, or max_passes of them.  Radii in
// the order given; the vertices are the cloud's points.
// Limitation: inputs that are not in general position (exact lattices with
// co-spherical quads) are decided by rounding -- deterministic and equal to the
// oracle, but a quad may be covered by both diagonals.
//
// Enumeration (k_bpa).  The live queries (the non-inner points) are compacted in
// the search grid's cell-sorted order; one wave64 (a one-wave workgroup) per live
// query i.  The wave walks the nine z-column runs of i's 27 cells (edge >= 2r),
// 64 positions at a time, and stages by ballot compaction every point with
// d2 < R4 into LDS: coordinates and cloud index (bit 31: inner).  LDS is what
// limits the waves a CU holds, and a surface's 2r-ball holds about 12, 50 and
// 200 points at the multipliers 1, 2 and 4, so the kernel runs in two tiers: every
// query with room for kCapFirst staged points (7.5 KB: 21 waves a CU), and the
// queries whose neighbourhood is larger once more with room for kCap (30 KB: 5
// waves a CU).  A neighbourhood of more than kCap points is reported, never
// truncated.  The
// staged non-inner points of index > i are compacted once more; the lanes take
// the pairs of that list by a linear pair number, do the geometric tests and
// fetch the three normals from global memory only for the pairs that pass them.
// The survivors of a batch of 64 pairs are taken one after the other: the wave
// tests the staged neighbourhood as blockers 64 at a time and leaves at the first
// hit.  What is left is appended through one atomic per batch to a capacity
// buffer (the count goes on past the capacity: the caller re-runs with the exact
// size), and slmerge.hip's sort_triples (two stable radix sorts: by k, then by i n
// + j, the flip bit masked off i) brings the output into rank order, so two runs
// give identical arrays.  All loop bounds are
// wave-uniform.

namespace {
namespace bpa {

constexpr int kW = 64;       // one wave per workgroup
constexpr int kCap = 1024;   // staged neighbourhood: 3 x 8 KB of coordinates, 4 KB of indices, 2 KB of slots
#ifndef SLBPA_FIRST_CAP      // (a measurement build sets it to 1024: one tier)
#define SLBPA_FIRST_CAP 256
#endif
constexpr int kCapFirst = SLBPA_FIRST_CAP;  // the first tier's
constexpr uint32_t kInner = 0x80000000u;

// ms: grid, enumeration, ordering; live queries, candidates, largest neighbourhood (when too large), second-tier queries
thread_local double tls_stats[7];

__device__ __forceinline__ double bcast(double v, int src) {
  const int lo = __shfl(__double2loint(v), src, kW), hi = __shfl(__double2hiint(v), src, kW);
  return __hiloint2double(hi, lo);
}

// flag[t] = 1 where the point at sorted position t is a query (not inner)
__global__ __launch_bounds__(kT) void k_bpa_live(const uint32_t* sidx, const uint8_t* vclass, int64_t n,
                                                 uint32_t* flag) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t < n) flag[t] = (!vclass || vclass[sidx[t]] != 2) ? 1u : 0u;
}

// raw: uint32 [3 cap]: (i | flip << 31, j, k), i < j < k.  cnt[0]: appended (beyond cap: counted only);
// cnt[1]: the largest neighbourhood above kCap (0: none); cnt[2]: the queries whose neighbourhood is
// above CAP < kCap, appended to redo[] for the next tier.
template <int CAP>
__global__ __launch_bounds__(kW) void k_bpa(SearchGrid sg, const int64_t* live, const uint8_t* vclass,
                                            const double* nrm, double r2, double R4, uint32_t* raw, uint32_t cap,
                                            uint32_t* cnt, int64_t* redo) {
  __shared__ double s_x[CAP], s_y[CAP], s_z[CAP];
  __shared__ uint32_t s_id[CAP];
  __shared__ uint16_t s_el[CAP];
  const int lane = threadIdx.x;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int64_t qp = live[blockIdx.x];
  const double q0 = sg.sxyz[3 * qp], q1 = sg.sxyz[3 * qp + 1], q2 = sg.sxyz[3 * qp + 2];
  const uint32_t qi = sg.sidx[qp];
  const int64_t cell = find_cell(sg.ukeys, sg.m, sg.skeys[qp]);
  if (cell < 0) return;  // (cannot happen: the key is a point's)
  // ---- stage the 2r-neighbourhood
  int n_nb = 0;
  for (int e = 0; e < 9; ++e) {
    const int32_t* nb = sg.nbr + 27 * cell + 3 * e;
    const int c0 = nb[0], c1 = nb[1], c2 = nb[2];
    const int first = c0 >= 0 ? c0 : (c1 >= 0 ? c1 : c2);
    const int last = c2 >= 0 ? c2 : (c1 >= 0 ? c1 : c0);
    if (first < 0) continue;
    const int64_t a = sg.ustart[first];
    const int64_t b = static_cast<int64_t>(last) + 1 < sg.m ? static_cast<int64_t>(sg.ustart[last + 1]) : sg.n;
    for (int64_t t0 = a; t0 < b; t0 += kW) {
      const int64_t t = t0 + lane;
      bool in = false;
      double x = 0.0, y = 0.0, z = 0.0;
      if (t < b) {
        x = sg.sxyz[3 * t];
        y = sg.sxyz[3 * t + 1];
        z = sg.sxyz[3 * t + 2];
        const double d0 = x - q0, d1 = y - q1, d2 = z - q2;
        in = (d0 * d0 + d1 * d1) + d2 * d2 < R4;
      }
      const unsigned long long m = __ballot(in);
      const int slot = n_nb + __popcll(m & below);
      if (in && slot < CAP) {
        const uint32_t id = sg.sidx[t];
        s_x[slot] = x;
        s_y[slot] = y;
        s_z[slot] = z;
        s_id[slot] = id | ((vclass && vclass[id] == 2) ? kInner : 0u);
      }
      n_nb += __popcll(m);
    }
  }
  if (n_nb > CAP) {  // wave-uniform
    if (lane == 0) {
      if (CAP < kCap) redo[atomicAdd(cnt + 2, 1u)] = qp;
      else atomicMax(cnt + 1, static_cast<uint32_t>(n_nb));
    }
    return;
  }
  __syncthreads();
  // ---- the staged non-inner points of index > i
  int n_el = 0;
  for (int u0 = 0; u0 < n_nb; u0 += kW) {
    const int u = u0 + lane;
    const bool el = u < n_nb && !(s_id[u] & kInner) && s_id[u] > qi;
    const unsigned long long m = __ballot(el);
    if (el) s_el[n_el + __popcll(m & below)] = static_cast<uint16_t>(u);
    n_el += __popcll(m);
  }
  __syncthreads();
  if (n_el < 2) return;
  const double ni0 = nrm[3 * static_cast<int64_t>(qi)], ni1 = nrm[3 * static_cast<int64_t>(qi) + 1],
               ni2 = nrm[3 * static_cast<int64_t>(qi) + 2];
  const int n_pairs = n_el * (n_el - 1) / 2;  // <= 1023 * 1022 / 2
  for (int f0 = 0; f0 < n_pairs; f0 += kW) {
    const int f = f0 + lane;
    bool ok = f < n_pairs;
    uint32_t j = 0, k = 0;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
    bool flip = false;
    if (ok) {
      // pair number f -> (ua < ub): f = ub (ub - 1) / 2 + ua
      int ub = static_cast<int>((1.0 + sqrt(1.0 + 8.0 * static_cast<double>(f))) * 0.5);
      while (ub * (ub - 1) / 2 > f) --ub;
      while ((ub + 1) * ub / 2 <= f) ++ub;
      const int ua = f - ub * (ub - 1) / 2;
      int sa = s_el[ua], sb = s_el[ub];
      if (s_id[sa] > s_id[sb]) {
        const int t = sa;
        sa = sb;
        sb = t;
      }
      j = s_id[sa];
      k = s_id[sb];
      const double x1 = s_x[sa], y1 = s_y[sa], z1 = s_z[sa];
      const double x2 = s_x[sb], y2 = s_y[sb], z2 = s_z[sb];
      double u0 = x1 - x2, u1 = y1 - y2, u2 = z1 - z2;
      const double a = (u0 * u0 + u1 * u1) + u2 * u2;  // d2(p1, p2)
      ok = a < R4;
      if (ok) {
        u0 = x2 - q0, u1 = y2 - q1, u2 = z2 - q2;
        const double b = (u0 * u0 + u1 * u1) + u2 * u2;  // d2(p2, p0)
        u0 = q0 - x1, u1 = q1 - y1, u2 = q2 - z1;
        const double c = (u0 * u0 + u1 * u1) + u2 * u2;  // d2(p0, p1)
        const double wa = a * ((b + c) - a), wb = b * ((a + c) - b), wc = c * ((a + b) - c);
        const double s = (wa + wb) + wc;
        ok = s > 0.0;
        if (ok) {
          const double fa = wa / s, fb = wb / s, fc = wc / s;
          const double cc0 = (q0 * fa + x1 * fb) + x2 * fc, cc1 = (q1 * fa + y1 * fb) + y2 * fc,
                       cc2 = (q2 * fa + z1 * fb) + z2 * fc;
          u0 = cc0 - q0, u1 = cc1 - q1, u2 = cc2 - q2;
          const double h = r2 - ((u0 * u0 + u1 * u1) + u2 * u2);
          const double e10 = x1 - q0, e11 = y1 - q1, e12 = z1 - q2;
          const double e20 = x2 - q0, e21 = y2 - q1, e22 = z2 - q2;
          const double n0 = e11 * e22 - e12 * e21, n1 = e12 * e20 - e10 * e22, n2 = e10 * e21 - e11 * e20;
          const double ln = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
          ok = h >= 0.0 && ln > 0.0;
          if (ok) {
            const double* nj = nrm + 3 * static_cast<int64_t>(j);
            const double* nk = nrm + 3 * static_cast<int64_t>(k);
            const double di = (n0 * ni0 + n1 * ni1) + n2 * ni2;
            const double dj = (n0 * nj[0] + n1 * nj[1]) + n2 * nj[2];
            const double dk = (n0 * nk[0] + n1 * nk[1]) + n2 * nk[2];
            const bool pos = di > 0.0 && dj > 0.0 && dk > 0.0;
            flip = di < 0.0 && dj < 0.0 && dk < 0.0;
            ok = pos || flip;
            const double w = (flip ? -1.0 : 1.0) * sqrt(h);
            o0 = cc0 + (n0 / ln) * w;
            o1 = cc1 + (n1 / ln) * w;
            o2 = cc2 + (n2 / ln) * w;
          }
        }
      }
    }
    // ---- emptiness: the survivors one after the other, the staged points 64 at a time
    unsigned long long todo = __ballot(ok);
    while (todo) {
      const int src = __ffsll(todo) - 1;
      todo &= todo - 1;
      const double c0 = bcast(o0, src), c1 = bcast(o1, src), c2 = bcast(o2, src);
      const uint32_t bj = __shfl(j, src, kW), bk = __shfl(k, src, kW);
      bool hit = false;
      for (int u0 = 0; u0 < n_nb && !hit; u0 += kW) {
        const int u = u0 + lane;
        bool inside = false;
        if (u < n_nb) {
          const uint32_t id = s_id[u] & ~kInner;
          const double d0 = s_x[u] - c0, d1 = s_y[u] - c1, d2 = s_z[u] - c2;
          inside = id != qi && id != bj && id != bk && (d0 * d0 + d1 * d1) + d2 * d2 < r2;
        }
        hit = __any(inside);
      }
      if (hit && lane == src) ok = false;
    }
    const unsigned long long keep = __ballot(ok);
    if (keep) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(cnt, static_cast<uint32_t>(__popcll(keep)));
      base = __shfl(base, 0, kW);
      const uint32_t at = base + static_cast<uint32_t>(__popcll(keep & below));
      if (ok && at < cap && at >= base) {  // (at >= base: the counter has not wrapped)
        raw[3 * static_cast<int64_t>(at)] = qi | (flip ? kInner : 0u);
        raw[3 * static_cast<int64_t>(at) + 1] = j;
        raw[3 * static_cast<int64_t>(at) + 2] = k;
      }
    }
  }
}

// raw[perm[t]] with its flip bit applied: the winding
__global__ __launch_bounds__(kT) void k_bpa_emit(const uint32_t* raw, const uint32_t* perm, int64_t m, int32_t* tri) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= m) return;
  const int64_t s = perm[t];
  const uint32_t i = raw[3 * s], j = raw[3 * s + 1], k = raw[3 * s + 2];
  const bool flip = (i & kInner) != 0;
  tri[3 * t] = static_cast<int32_t>(i & ~kInner);
  tri[3 * t + 1] = static_cast<int32_t>(flip ? k : j);
  tri[3 * t + 2] = static_cast<int32_t>(flip ? j : k);
}

}  // namespace bpa
}  // namespace

extern "C" {

int sl_ball_pivot_max_neighbours(void) { return bpa::kCap; }

int sl_ball_pivot_candidates(sl_ctx* c, const double* xyz, const double* normals, int64_t n, double radius,
                             const uint8_t* vclass, int32_t* triangles, int64_t capacity, int64_t* count,
                             void* stream) {
  using namespace bpa;
  if (!c) return SL_EINVAL;
  if (n < 0 || capacity < 0 || !count || (n && (!xyz || !normals)) || (capacity && !triangles))
    return slgpu_fail(c, SL_EINVAL, "sl_ball_pivot_candidates: bad sizes or NULL arguments");
  if (!(radius > 0.0) || !std::isfinite(radius))
    return slgpu_fail(c, SL_EINVAL, "sl_ball_pivot_candidates: radius must be positive and finite");
  if (n >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  *count = 0;
  for (double& v : tls_stats) v = 0.0;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = prim::require_finite(c, xyz, n, "sl_ball_pivot_candidates: non-finite point coordinates", s);
  if (r) return r;
  prim::StageClock clock(s);
  SearchGridBufs sg;
  r = build_search_grid(c, xyz, n, 2.0 * radius, GridTable::kNeighbours,
                        "sl_ball_pivot_candidates: non-finite point coordinates", &sg, s);
  if (r) return r;
  // the live queries, in cell-sorted order
  DBuf<uint32_t> flag, pos, cnt;
  DBuf<int64_t> live, redo;
  MTRY(c, flag.alloc(n));
  MTRY(c, pos.alloc(n));
  MTRY(c, live.alloc(n));
  MTRY(c, cnt.alloc(3));
  hipLaunchKernelGGL(k_bpa_live, dim3(blocks(n)), dim3(kT), 0, s, sg.view.sidx, vclass, n, flag.p);
  MTRY(c, hipGetLastError());
  int64_t n_live = 0;
  r = compact_indices(c, flag.p, n, pos.p, live.p, &n_live, s);
  if (r) return r;
  MTRY(c, clock.lap(&tls_stats[0]));
  tls_stats[3] = static_cast<double>(n_live);
  if (n_live == 0) return SL_OK;
  const int64_t cap = std::min<int64_t>(capacity, 0xffffffffll);
  DBuf<uint32_t> raw;
  MTRY(c, raw.alloc(3 * cap));
  MTRY(c, redo.alloc(n_live));
  MTRY(c, hipMemsetAsync(cnt.p, 0, 3 * sizeof(uint32_t), s));
  const double r2 = radius * radius;
  uint32_t h[3] = {0, 0, 0};
  if (kCapFirst < kCap) {
    hipLaunchKernelGGL(k_bpa<kCapFirst>, dim3(static_cast<unsigned>(n_live)), dim3(kW), 0, s, sg.view, live.p, vclass,
                       normals, r2, 4.0 * r2, raw.p, static_cast<uint32_t>(cap), cnt.p, redo.p);
    MTRY(c, hipGetLastError());
    MTRY(c, hipMemcpyAsync(h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, s));
    MTRY(c, hipStreamSynchronize(s));
  }
  // the second tier: the queries the first had no room for (h[2] <= n_live; redo[] is complete: the copy
  // above is behind the kernel on the stream)
  const int64_t n_big = kCapFirst < kCap ? static_cast<int64_t>(h[2]) : n_live;
  if (n_big) {
    hipLaunchKernelGGL(k_bpa<kCap>, dim3(static_cast<unsigned>(n_big)), dim3(kW), 0, s, sg.view,
                       kCapFirst < kCap ? redo.p : live.p, vclass, normals, r2, 4.0 * r2, raw.p,
                       static_cast<uint32_t>(cap), cnt.p, static_cast<int64_t*>(nullptr));
    MTRY(c, hipGetLastError());
    MTRY(c, hipMemcpyAsync(h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, s));
  }
  MTRY(c, clock.lap(&tls_stats[1]));
  if (h[1]) {
    tls_stats[5] = static_cast<double>(h[1]);
    char msg[160];
    snprintf(msg, sizeof(msg),
             "sl_ball_pivot_candidates: a point has %u points within twice the radius; the limit is %d", h[1], kCap);
    return slgpu_fail(c, SL_EINVAL, msg);
  }
  const int64_t m = h[0];
  *count = m;
  tls_stats[4] = static_cast<double>(m);
  tls_stats[6] = static_cast<double>(n_big);
  if (m == 0 || m > cap) return SL_OK;  // m > capacity: nothing is written; the caller re-runs at capacity >= m
  DBuf<uint64_t> key;
  DBuf<uint32_t> perm;
  MTRY(c, key.alloc(m));
  MTRY(c, perm.alloc(m));
  r = sort_triples(c, raw.p, m, static_cast<uint64_t>(n), ~kInner, key.p, perm.p, s);  // rank order
  if (r) return r;
  hipLaunchKernelGGL(k_bpa_emit, dim3(blocks(m)), dim3(kT), 0, s, raw.p, perm.p, m, triangles);
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_stats[2]));
  return SL_OK;
}

int sl_ball_pivot_candidates_stats(double* stats, int capacity) {
  return prim::copy_stats(bpa::tls_stats, stats, capacity);
}

}  // extern "C"
