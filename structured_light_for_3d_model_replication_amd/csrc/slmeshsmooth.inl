// libslgpu.so, part 2l -- mesh smoothing, included at the end of slmerge.hip
// after the mesh writers (slmeshwrite.inl) and the colour transfer
// (slmeshcolor.inl), of which it names nothing (one translation unit: it shares
// slmerge.hip's scratch pool, radix sort, key runs and their starts, and
// slprim.inl's side table, input checks and stage clock).  Open3D users take the terraces of a scanned mesh out
// with TriangleMesh::FilterSmoothTaubin; that call, FilterSmoothSimple,
// FilterSmoothLaplacian and the ComputeAdjacencyList they rest on are restated
// here, for the vertices alone (normals and colours are not filtered).  Open3D
// is not in this image, so parity with it is UNPINNED and
// tests/meshsmooth_oracle.py is the CPU restatement the tests check against,
// exactly.
//
// Input: vertices f64 [V][3], triangles int32 [T][3]; V < 2^31, 6 T < 2^32 (the
// CSR's entries and scans are 32-bit: prim::bad_csr_sizes).  k_mc_check reads every index before anything is
// indexed: one outside 0 .. V-1 is SL_EINDEX, never a load.  A non-finite vertex
// coordinate is SL_EINVAL.
//
//   adjacency
//     N(v)     the set of indices that share a triangle with v: (a, b, c) inserts
//              b and c into N(a), a and c into N(b), a and b into N(c).  As in
//              Open3D's inserts, a triangle that repeats an index puts v into its
//              own set: (a, a, b) gives N(a) = {a, b}.
//     CSR      row_start int64 [V+1], neighbours int32 [M]: row v is
//              neighbours[row_start[v] .. row_start[v+1]), ascending, no
//              duplicates; a vertex of no triangle has an empty row.
//     multiplicity of {u, w}, u != w: the number of (triangle, side) pairs whose
//              side is {u, w} -- its run length among the 3 T sorted sides.
//     boundary a vertex with an incident edge of multiplicity exactly 1.
//   simple filter, one iteration, per axis, f64, uncontracted:
//              s = p_v; s = s + p_j for j in N(v) ascending; p'_v = s / (1 + |N(v)|).
//   Laplacian step with factor l: sum = (0, 0, 0), tw = 0; for j in N(v) ascending
//              d = p_v - p_j; dist = sqrt((dx dx + dy dy) + dz dz);
//              w = 1.0 / (dist + 1e-12); tw = tw + w; sum_a = sum_a + w p_j,a;
//              then p'_v,a = p_v,a + l (sum_a / tw - p_v,a).
//   filter_smooth_laplacian(iterations, lambda): that step `iterations` times.
//   filter_smooth_taubin(iterations, lambda, mu): a lambda step, then a mu step,
//              per iteration.
//   Every step reads only the previous step's positions (Jacobi).  iterations = 0
//   is a copy.
//   DEVIATIONS.  Open3D walks an unordered_set, so its last bits depend on the hash
//   order: here the fold runs in ascending neighbour index.  Open3D divides 0 / 0
//   for a vertex with an empty row in the Laplacian step: here such a vertex keeps
//   its position (the simple filter divides by 1 and needs no exception).  With
//   fixed_boundary (an extension; off is Open3D's behaviour) a boundary vertex
//   keeps its position in every step; its neighbours still read it.
//
// Adjacency on the device.  The directed pairs (v, w) and (w, v) hold the same
// information, so only the 3 T undirected sides are sorted: prim::sort_sides'
// table, of which the keys alone are read (min V + max holds both ends).
// key_runs flags the run heads and scans them and k_seg_starts gathers the unique sides' keys and first positions -- a side's
// run length is its multiplicity, so boundary costs nothing beyond the sort.
// The unique sides in key order are every vertex's UPPER neighbours (w >= v, v
// itself when a triangle repeats it), ascending.  The LOWER neighbours are the
// transpose: k_ms_tkeys keys every unique side by its larger end (a side {a, a}
// by V, so it sorts behind all others) with the smaller end as value, and a second,
// stable radix_sort over the bits V has leaves them by (larger, smaller).  With
// ub[v] = the unique sides whose smaller end is below v and lb[v] = the
// transposed ones whose larger end is (two binary searches per vertex), row v
// is its lower neighbours followed by its upper ones, row_start[v] = lb[v] +
// ub[v], the transposed entry at position p with larger end w goes to p + ub[w]
// and the unique side e with smaller end u to e + lb[u + 1]: one scatter, no
// scan of its own.  (The route over the 6 T directed pairs, one sort and a
// compaction, gave the same CSR in 28.1 ms where this takes 18.8 ms on the
// depth-10 mesh: DESIGN.md 5.14, profiles/mesh_smooth/ab_csr_route.jsonl.)
//
// Smoothing on the device.  One thread per vertex walks its row: the f64 fold
// order is part of the definition, so a row's sum is never split across lanes.
// Positions are plain 8-byte loads of the AoS array; a step writes the other
// buffer of a ping-pong pair from the scratch pool, the last step the caller's
// output; a lambda step and a mu step are separate launches (the kernel boundary
// is the global dependency).  No atomics, no waits, every loop bounded by a row
// length.

namespace {
namespace msm {

thread_local double tls_ms[4];  // keys, sort, CSR, iterations of the last call

using prim::require_finite, prim::require_indices, prim::bad_csr_sizes;

__global__ __launch_bounds__(kT) void k_ms_simple(const double* __restrict__ in, const int64_t* __restrict__ row_start,
                                                  const int32_t* __restrict__ nb, const uint8_t* __restrict__ fixed,
                                                  int64_t n_v, double* __restrict__ out) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n_v) return;
  double s0 = in[3 * v], s1 = in[3 * v + 1], s2 = in[3 * v + 2];
  if (!(fixed && fixed[v])) {
    const int64_t a = row_start[v], b = row_start[v + 1];
    for (int64_t j = a; j < b; ++j) {
      const int64_t q = nb[j];
      s0 = s0 + in[3 * q];
      s1 = s1 + in[3 * q + 1];
      s2 = s2 + in[3 * q + 2];
    }
    const double cnt = static_cast<double>(1 + (b - a));
    s0 = s0 / cnt;
    s1 = s1 / cnt;
    s2 = s2 / cnt;
  }
  out[3 * v] = s0;
  out[3 * v + 1] = s1;
  out[3 * v + 2] = s2;
}

__global__ __launch_bounds__(kT) void k_ms_laplacian(const double* __restrict__ in,
                                                     const int64_t* __restrict__ row_start,
                                                     const int32_t* __restrict__ nb,
                                                     const uint8_t* __restrict__ fixed, int64_t n_v, double factor,
                                                     double* __restrict__ out) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n_v) return;
  double p0 = in[3 * v], p1 = in[3 * v + 1], p2 = in[3 * v + 2];
  const int64_t a = row_start[v], b = row_start[v + 1];
  if (b > a && !(fixed && fixed[v])) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, tw = 0.0;
    for (int64_t j = a; j < b; ++j) {
      const int64_t q = nb[j];
      const double q0 = in[3 * q], q1 = in[3 * q + 1], q2 = in[3 * q + 2];
      const double d0 = p0 - q0, d1 = p1 - q1, d2 = p2 - q2;
      const double dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
      const double w = 1.0 / (dist + 1e-12);
      tw = tw + w;
      s0 = s0 + w * q0;
      s1 = s1 + w * q1;
      s2 = s2 + w * q2;
    }
    p0 = p0 + factor * (s0 / tw - p0);
    p1 = p1 + factor * (s1 / tw - p1);
    p2 = p2 + factor * (s2 / tw - p2);
  }
  out[3 * v] = p0;
  out[3 * v + 1] = p1;
  out[3 * v + 2] = p2;
}

// The unique sides transposed: key = the larger end (V for a side {a, a}: it sorts last), value = the smaller.
__global__ __launch_bounds__(kT) void k_ms_tkeys(const uint64_t* ukeys, int64_t n_e, uint64_t n_v, uint64_t* tkeys,
                                                 uint32_t* tvals) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (e >= n_e) return;
  const uint64_t u = ukeys[e] / n_v, w = ukeys[e] - u * n_v;
  tkeys[e] = u == w ? n_v : w;
  tvals[e] = static_cast<uint32_t>(u);
}

// v = 0 .. V: ub[v] = the unique sides whose smaller end is below v, lb[v] = the transposed ones whose larger end
// is; row v = its lower neighbours, then v itself and its upper ones, so row_start[v] = lb[v] + ub[v].
__global__ __launch_bounds__(kT) void k_ms_rows(const uint64_t* ukeys, const uint64_t* tkeys, int64_t n_e,
                                                uint64_t n_v, uint32_t* ub, uint32_t* lb, int64_t* row_start) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v > static_cast<int64_t>(n_v)) return;
  const uint64_t want = static_cast<uint64_t>(v) * n_v;
  int64_t lo = 0, hi = n_e;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ukeys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  const int64_t u = lo;
  lo = 0, hi = n_e;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (tkeys[mid] < static_cast<uint64_t>(v)) lo = mid + 1;
    else hi = mid;
  }
  ub[v] = static_cast<uint32_t>(u);
  lb[v] = static_cast<uint32_t>(lo);
  row_start[v] = u + lo;
}

// The entries: transposed position p (larger end w) -> nb[p + ub[w]]; unique side e (smaller end u) ->
// nb[e + lb[u + 1]].  boundary: a side of one (triangle, side) pair with two different ends marks both.
__global__ __launch_bounds__(kT) void k_ms_emit(const uint64_t* ukeys, const uint32_t* starts, const uint64_t* tkeys,
                                                const uint32_t* tvals, int64_t n_e, int64_t n3, uint64_t n_v,
                                                const uint32_t* ub, const uint32_t* lb, int32_t* nb,
                                                uint8_t* boundary) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (e >= n_e) return;
  const uint64_t w = tkeys[e];
  if (w < n_v) nb[e + ub[w]] = static_cast<int32_t>(tvals[e]);
  const uint64_t u = ukeys[e] / n_v, h = ukeys[e] - u * n_v;
  nb[e + lb[u + 1]] = static_cast<int32_t>(h);
  if (boundary && u != h) {
    const int64_t end = e + 1 < n_e ? static_cast<int64_t>(starts[e + 1]) : n3;
    if (end - starts[e] == 1) boundary[u] = boundary[h] = 1;
  }
}

// The unique sides of a mesh in key order and transposed: what both entry points turn into the CSR.
struct Sides {
  DBuf<uint64_t> ukeys, tkeys;   // [n_e]: min V + max ascending; the larger end (V for {a, a}) ascending
  DBuf<uint32_t> starts, tvals;  // [n_e]: a unique side's first sorted position; the transposed sides' smaller ends
  int64_t n3 = 0, n_e = 0;       // sides, unique sides (the CSR has at most 2 n_e entries)
};

// The side table (its values are not read: the keys hold both ends), the runs and the transposed sort (n_t > 0,
// indices checked).  The first two stages are timed here, stage 1 being both sorts and the runs between them; the
// clock runs on.
int sorted_sides(sl_ctx* c, const int32_t* tris, int64_t n_t, uint64_t nv, Sides& S, prim::StageClock& clock,
                 hipStream_t s) {
  prim::SideTable table;
  int r = prim::sort_sides(c, tris, n_t, nv, table, nullptr, nullptr, nullptr, clock, &tls_ms[0], nullptr, s);
  if (r) return r;
  S.n3 = table.n3;
  const uint64_t* keys = table.keys.p;
  DBuf<uint32_t> flag, seg;
  MTRY(c, flag.alloc(S.n3));
  MTRY(c, seg.alloc(S.n3));
  r = key_runs(c, keys, S.n3, flag.p, seg.p, &S.n_e, s);
  if (r) return r;
  MTRY(c, S.starts.alloc(S.n_e));
  MTRY(c, S.ukeys.alloc(S.n_e));
  MTRY(c, S.tkeys.alloc(S.n_e));
  MTRY(c, S.tvals.alloc(S.n_e));
  hipLaunchKernelGGL(k_seg_starts, dim3(blocks(S.n3)), dim3(kT), 0, s, flag.p, seg.p, keys, S.n3, S.starts.p,
                     S.ukeys.p);
  hipLaunchKernelGGL(k_ms_tkeys, dim3(blocks(S.n_e)), dim3(kT), 0, s, S.ukeys.p, S.n_e, nv, S.tkeys.p, S.tvals.p);
  MTRY(c, hipGetLastError());
  r = radix_sort(c, S.tkeys.p, S.tvals.p, S.n_e, key_bits(nv), s);  // stable: (larger, smaller) ascending
  if (r) return r;
  MTRY(c, clock.lap(&tls_ms[1]));
  return SL_OK;
}

// row_start [V+1], neighbours [room for 2 S.n_e], boundary u8 [V] (may be NULL) from the sides; the entry count
// (row_start[V]) -> *m once the stream is idle.
int emit_csr(sl_ctx* c, const Sides& S, int64_t n_v, int64_t* row_start, int32_t* neighbours, uint8_t* boundary,
             int64_t* m, hipStream_t s) {
  const uint64_t nv = static_cast<uint64_t>(n_v);
  DBuf<uint32_t> ub, lb;
  MTRY(c, ub.alloc(n_v + 1));
  MTRY(c, lb.alloc(n_v + 1));
  hipLaunchKernelGGL(k_ms_rows, dim3(blocks(n_v + 1)), dim3(kT), 0, s, S.ukeys.p, S.tkeys.p, S.n_e, nv, ub.p, lb.p,
                     row_start);
  if (boundary) MTRY(c, hipMemsetAsync(boundary, 0, static_cast<size_t>(n_v), s));
  hipLaunchKernelGGL(k_ms_emit, dim3(blocks(S.n_e)), dim3(kT), 0, s, S.ukeys.p, S.starts.p, S.tkeys.p, S.tvals.p,
                     S.n_e, S.n3, nv, ub.p, lb.p, neighbours, boundary);
  MTRY(c, hipGetLastError());
  MTRY(c, hipMemcpyAsync(m, row_start + n_v, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

}  // namespace msm
}  // namespace

extern "C" {

int sl_mesh_adjacency(sl_ctx* c, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                      int64_t* row_start, int32_t* neighbours, uint8_t* boundary, int64_t* n_neighbours,
                      void* stream) {
  using namespace msm;
  if (!c) return SL_EINVAL;
  if (bad_csr_sizes(n_vertices, n_triangles) || !n_neighbours || !row_start ||
      (n_triangles && (!triangles || !neighbours)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_adjacency: bad sizes or NULL arguments");
  *n_neighbours = 0;
  for (double& v : tls_ms) v = 0.0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n_triangles, n_vertices, "triangle index out of range", s);
  if (r) return r;
  if (n_triangles == 0) {  // every row is empty
    MTRY(c, hipMemsetAsync(row_start, 0, sizeof(int64_t) * static_cast<size_t>(n_vertices + 1), s));
    if (boundary && n_vertices) MTRY(c, hipMemsetAsync(boundary, 0, static_cast<size_t>(n_vertices), s));
    MTRY(c, hipStreamSynchronize(s));
    return SL_OK;
  }
  prim::StageClock clock(s);
  Sides S;
  r = sorted_sides(c, triangles, n_triangles, static_cast<uint64_t>(n_vertices), S, clock, s);
  if (r) return r;
  r = emit_csr(c, S, n_vertices, row_start, neighbours, boundary, n_neighbours, s);
  if (r) return r;
  MTRY(c, clock.lap(&tls_ms[2]));
  return SL_OK;
}

int sl_mesh_smooth(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                   int64_t n_triangles, int method, int iterations, double lambda, double mu, int fixed_boundary,
                   double* out_vertices, void* stream) {
  using namespace msm;
  if (!c) return SL_EINVAL;
  if (bad_csr_sizes(n_vertices, n_triangles) || (n_vertices && (!vertices || !out_vertices)) ||
      (n_triangles && !triangles))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_smooth: bad sizes or NULL arguments");
  if (method < 0 || method > 2) return slgpu_fail(c, SL_EINVAL, "sl_mesh_smooth: method must be 0, 1 or 2");
  if (iterations < 0) return slgpu_fail(c, SL_EINVAL, "sl_mesh_smooth: iterations must not be negative");
  if ((method >= 1 && !std::isfinite(lambda)) || (method == 2 && !std::isfinite(mu)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_smooth: non-finite lambda or mu");
  for (double& v : tls_ms) v = 0.0;
  const int64_t n = n_vertices;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n_triangles, n, "triangle index out of range", s);
  if (r) return r;
  if (n == 0) return SL_OK;
  r = require_finite(c, vertices, n, "sl_mesh_smooth: non-finite vertex coordinates", s);
  if (r) return r;
  const int64_t steps = static_cast<int64_t>(iterations) * (method == 2 ? 2 : 1);
  if (steps == 0 || n_triangles == 0) {  // nothing moves: no step, or every row empty (s / 1; kept)
    MTRY(c, hipMemcpyAsync(out_vertices, vertices, sizeof(double) * 3 * static_cast<size_t>(n),
                           hipMemcpyDeviceToDevice, s));
    MTRY(c, hipStreamSynchronize(s));
    return SL_OK;
  }
  prim::StageClock clock(s);
  DBuf<int64_t> row_start;
  DBuf<int32_t> nb;
  DBuf<uint8_t> fixed;
  {
    Sides S;
    r = sorted_sides(c, triangles, n_triangles, static_cast<uint64_t>(n), S, clock, s);
    if (r) return r;
    int64_t m = 0;
    MTRY(c, row_start.alloc(n + 1));
    MTRY(c, nb.alloc(2 * S.n_e));
    if (fixed_boundary) MTRY(c, fixed.alloc(n));
    r = emit_csr(c, S, n, row_start.p, nb.p, fixed.p, &m, s);
    if (r) return r;
    MTRY(c, clock.lap(&tls_ms[2]));
  }
  DBuf<double> ping, pong;  // the last step writes out_vertices, the ones before it alternate between these
  if (steps >= 2) MTRY(c, ping.alloc(3 * n));
  if (steps >= 3) MTRY(c, pong.alloc(3 * n));
  const double* src = vertices;
  for (int64_t k = 0; k < steps; ++k) {
    double* dst = k + 1 == steps ? out_vertices : (k & 1) ? pong.p : ping.p;
    if (method == 0) {
      hipLaunchKernelGGL(k_ms_simple, dim3(blocks(n)), dim3(kT), 0, s, src, row_start.p, nb.p, fixed.p, n, dst);
    } else {
      const double factor = (method == 2 && (k & 1)) ? mu : lambda;
      hipLaunchKernelGGL(k_ms_laplacian, dim3(blocks(n)), dim3(kT), 0, s, src, row_start.p, nb.p, fixed.p, n, factor,
                         dst);
    }
    MTRY(c, hipGetLastError());
    src = dst;
  }
  MTRY(c, clock.lap(&tls_ms[3]));
  return SL_OK;
}

int sl_mesh_smooth_stats(double* stage_ms, int capacity) {
  return prim::copy_stats(msm::tls_ms, stage_ms, capacity);
}

}  // extern "C"
