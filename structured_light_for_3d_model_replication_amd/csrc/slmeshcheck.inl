// libslgpu.so, part 2m -- mesh checks, included at the end of slmerge.hip (one
// translation unit: it uses that file's scratch pool, radix and triple sorts,
// scan and row compaction, slprim.inl's side table, union-find, rotated triples,
// triangle area, input checks and stage clock, and the C entry point sl_ordered_sum).  Open3D users
// ask a TriangleMesh is_edge_manifold, is_vertex_manifold, is_orientable,
// is_watertight, get_non_manifold_edges, get_non_manifold_vertices,
// orient_triangles, get_surface_area, get_volume, remove_degenerate_triangles
// and remove_duplicated_triangles.  They are restated here in order-free forms;
// Open3D is not in this image, so parity with it is UNPINNED, its loops are
// quoted from memory, and tests/meshcheck_oracle.py is the definition the tests
// check against, exactly.
//
// Input: triangles int32 [T][3], n_vertices V, vertices f64 [V][3] for the
// measures; V < 2^31, 3 T < 2^32 (prim::bad_sizes).  prim::require_indices
// reads every index before anything is indexed: one outside 0 .. V-1 is
// SL_EINDEX ("... triangle index out of range"), never a load.
//
//   sides     (a, b, c) has the sides a->b, b->c, c->a.  A side's key is min V +
//             max (slprim.inl's side table), its direction bit is from < to.  A triangle
//             with two equal indices is DEGENERATE; it still gives its three
//             sides to the edge counts, as Open3D's edges_to_triangles map does:
//             (a, a, b) gives {a, a} once and {a, b} twice.
//   edges     m = the sides with one key.  m = 1 boundary; m = 2 regular, and
//             CONSISTENT iff the two direction bits differ; m >= 3 non-manifold.
//             get_non_manifold_edges(allow_boundary_edges = true): the m >= 3
//             edges; false: the m = 1 edges too.  Rows (min, max) in ascending
//             key order.  DEVIATION: Open3D returns hash order.
//             is_edge_manifold(allow_boundary_edges) iff that list is empty.
//   vertices  Degenerate triangles take no part (DEVIATION: Open3D's loop lets
//             (v, w, w) add a self-link at v and dereferences an empty map for
//             (v, v, w)).  A corner is (t, k), index 3 t + k.  Two corners at one
//             vertex v are joined iff their triangles share an edge that contains
//             v; v is non-manifold iff its corners fall into more than one class.
//             On a mesh without degenerate triangles this is Open3D's search over
//             the link graph of v (non-manifold iff the search does not reach
//             every link vertex): the corners are the link's edges, joined where
//             they meet in a link vertex.  Ascending vertex index (Open3D's order).
//   orientable  iff no edge has m >= 3 and there is a flip bit per triangle that
//             makes every m = 2 edge consistent (both sides of one triangle: iff
//             their directions differ; two loops {v, v}: never, a flip does not
//             turn a loop).  This is Open3D's OrientTriangles rule that no
//             directed edge may occur twice.
//   orient_triangles  components are connected through m = 2 edges; in each the
//             smallest triangle index keeps its winding; a flipped (a, b, c) is
//             (a, c, b).  DEVIATIONS: Open3D seeds a component from an
//             unordered_set; when the mesh is not orientable the triangles come
//             back unchanged (Open3D leaves them half flipped).
//   watertight  edge-manifold without boundary, vertex-manifold, no inconsistent
//             edge, as given (no flips are searched).  DEVIATION: Open3D also
//             tests self-intersection (an O(T^2) pair loop); that is not built.
//   measures  f64, uncontracted.  A_t = prim::tri_area(v0, v1, v2), half the length
//             of (v1 - v0) x (v2 - v0).
//             W_t = ((x0 c0 + y0 c1) + z0 c2) / 6.0, c = v1 x v2, c0 = y1 z2 - z1
//             y2, c1 = z1 x2 - x1 z2, c2 = x1 y2 - y1 x2.  Area and signed volume
//             are the ordered sums (slplane.inl) of A_t and W_t in triangle order.
//             The signed volume is positive iff the windings face outward.
//   removals  remove_degenerate: the triangles with two equal indices go, the rest
//             keep their order.  remove_duplicated: prim::k_sc_tris' rotation
//             (sl_mesh_simplify_clustering's: the strictly smallest index first;
//             the opposite winding is another triple); the first occurrence of
//             every rotated triple is kept, in input order, stored AS GIVEN
//             (DEVIATION: Open3D stores the rotated form).
//
// One sort per sl_mesh_check: prim::sort_sides' table of three (key, 3 t + k)
// pairs per triangle; everything else looks at run neighbours.  The triangle,
// side and direction bit of a sorted entry come back from its value by one gather.
//   k_mk_classify   a run's head asks prim::run_sides (i - 1, i + 1 and i + 2) for
//             m = 1, 2 or >= 3.  Counters are integer atomics, one per wave and
//             counter, by ballot.  The edge list: flags, scan_flags, a gather.
//   k_mk_corner_union   entry i unites its two corners with those of the nearest
//             earlier entry of its run whose triangle is not degenerate (the
//             chain connects the run's non-degenerate entries; the walk back over
//             degenerate ones is bounded by the run's start), prim::unite on
//             3 T words.  After the kernel boundary a corner that is its own
//             parent is a class: one integer atomic per class to nroots[v].
//   k_mk_parity_union   the orientation, below.
//
// Parity union-find: why it is wait-free and never wrong.  One word per
// triangle, (ancestor << 1) | parity to that ancestor, starting as (t << 1): a
// root with parity 0.  slprim.inl's argument holds for the ancestors: a root a
// is hooked under a SMALLER root b by atomicCAS(word[a], a << 1, (b << 1) | p)
// and only roots are hooked, so ancestors only decrease, no cycle forms and a
// component's final root is its smallest triangle.  What is new is p.  Every
// hook fixes, once and for ever, the parity between a and b; the parity from x
// to any ancestor g of x is the XOR along the one path of hook edges from x up
// to g, whatever words are read on the way: it is a FACT about (x, g) that no
// later write changes.  So
//   - a stale read of word[x] returns an older (ancestor, parity) pair, which
//     is still a true pair: the walk costs more steps and never a wrong parity;
//   - path halving replaces word[x] by (g << 1) | parity(x, g) for a strictly
//     smaller ancestor g through atomicMin on the packed word: the ancestor is
//     in the high bits, so the minimum is the pair of the smaller ancestor, and
//     two pairs of one ancestor are the same word;
//   - a thread that walked from t1 to a with parity pa and from t2 to b with pb
//     needs flip(t1) ^ flip(t2) = rel, so it hooks a (the larger) under b with p =
//     pa ^ pb ^ rel.  A failed CAS returns a's true word; the thread continues
//     from THAT pair (pa ^= its parity, a = its ancestor, strictly lower);
//   - both walks ending in one node means a shared ancestor, true even when read
//     stale; then pa ^ pb is the parity between t1 and t2 the unions so far
//     imply, and pa ^ pb != rel raises the not-orientable flag.
// No thread waits on another and every loop is bounded by a strictly decreasing
// index.  After the kernel boundary the words are walked with plain loads:
// flip[t] is the parity to the root, and the root, the component's smallest
// triangle, has parity 0 and keeps its winding.

namespace {
namespace mck {

enum { kUnique, kBoundary, kNonManifold, kInconsistent, kDegenerate, kOdd, kCounters };

thread_local double tls_ms[7];  // side keys, sort, classify + edge list, corners, parity unions, flips, measures

using prim::require_finite, prim::require_indices;
using prim::wave_add, prim::Side, prim::side_of, prim::bad_sizes;

__device__ __forceinline__ bool degenerate(const int32_t* tris, int64_t t) {
  const int32_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
  return a == b || b == c || c == a;
}

// the corner of side s at vertex v (one of its two ends; they differ)
__device__ __forceinline__ uint32_t corner_at(const Side& s, uint32_t v) {
  return s.from == v ? 3u * s.t + s.k : 3u * s.t + (s.k == 2u ? 0u : s.k + 1u);
}

// One thread per sorted position: a run's head classifies its edge.  flag (may be NULL): 1 at the heads that go
// into the edge list.
__global__ __launch_bounds__(kT) void k_mk_classify(const uint64_t* keys, const uint32_t* vals, const int32_t* tris,
                                                    int64_t n3, int allow_boundary, unsigned long long* cnt,
                                                    uint32_t* flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  const bool live = i < n3;
  int m = 0;  // the sides of the run that starts here
  bool odd = false;
  if (live) {
    m = prim::run_sides(keys, i, n3);
    if (m == 2) {
      const Side a = side_of(tris, vals[i]), b = side_of(tris, vals[i + 1]);
      odd = (a.from < a.to) == (b.from < b.to);
    }
    if (flag) flag[i] = (m == 3 || (m == 1 && !allow_boundary)) ? 1u : 0u;
  }
  wave_add(cnt + kUnique, m != 0);
  wave_add(cnt + kBoundary, m == 1);
  wave_add(cnt + kNonManifold, m == 3);
  wave_add(cnt + kInconsistent, odd);
}

__global__ __launch_bounds__(kT) void k_mk_edge_list(const uint64_t* keys, const uint32_t* flag, const uint32_t* pos,
                                                     int64_t n3, uint64_t n_v, int32_t* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= n3 || !flag[i]) return;
  const uint64_t k = keys[i], lo = k / n_v;
  out[2 * static_cast<int64_t>(pos[i])] = static_cast<int32_t>(lo);
  out[2 * static_cast<int64_t>(pos[i]) + 1] = static_cast<int32_t>(k - lo * n_v);
}

__global__ __launch_bounds__(kT) void k_mk_corner_union(const uint64_t* keys, const uint32_t* vals,
                                                        const int32_t* tris, int64_t n3, uint32_t* parent) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < 1 || i >= n3) return;
  const uint64_t k = keys[i];
  if (keys[i - 1] != k) return;
  const Side a = side_of(tris, vals[i]);
  if (degenerate(tris, a.t)) return;
  int64_t j = i - 1;  // the nearest earlier entry of the run whose triangle is not degenerate
  while (j >= 0 && keys[j] == k && degenerate(tris, vals[j] / 3u)) --j;
  if (j < 0 || keys[j] != k) return;
  const Side b = side_of(tris, vals[j]);
  prim::unite(parent, corner_at(a, a.from), corner_at(b, a.from));
  prim::unite(parent, corner_at(a, a.to), corner_at(b, a.to));
}

// After the unions (a kernel boundary: plain loads): a corner of a non-degenerate triangle that is its own parent is
// one class of its vertex.
__global__ __launch_bounds__(kT) void k_mk_corner_roots(const uint32_t* parent, const int32_t* tris, int64_t n3,
                                                        uint32_t* nroots) {
  const int64_t x = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (x >= n3 || parent[x] != static_cast<uint32_t>(x) || degenerate(tris, x / 3)) return;
  atomicAdd(nroots + tris[x], 1u);
}

__global__ __launch_bounds__(kT) void k_mk_vertex_flags(const uint32_t* nroots, int64_t n_v, uint32_t* flag) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v < n_v) flag[v] = nroots[v] > 1u ? 1u : 0u;
}

__global__ __launch_bounds__(kT) void k_mk_vertex_list(const uint32_t* flag, const uint32_t* pos, int64_t n_v,
                                                       int32_t* out) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v < n_v && flag[v]) out[pos[v]] = static_cast<int32_t>(v);
}

// -> a node that is (or, read stale, was) the root of x's tree; *par ^= the parity of x to it.  Halves the path.
__device__ __forceinline__ uint32_t find_parity(uint32_t* word, uint32_t x, uint32_t* par) {
  for (;;) {
    const uint32_t w = prim::ld_parent(word + x), a = w >> 1;
    if (a == x) return x;
    const uint32_t wa = prim::ld_parent(word + a), g = wa >> 1;
    *par ^= w & 1u;
    if (g == a) return a;
    atomicMin(word + x, (g << 1) | ((w ^ wa) & 1u));  // g < a < x: a smaller ancestor of x and the parity to it
    *par ^= wa & 1u;
    x = g;
  }
}

// flip(a) ^ flip(b) = rel from now on, or *odd when the unions so far say otherwise.
__device__ __forceinline__ void unite_parity(uint32_t* word, uint32_t a, uint32_t b, uint32_t rel,
                                             unsigned long long* odd) {
  uint32_t pa = 0u, pb = 0u;
  for (;;) {
    a = find_parity(word, a, &pa);
    b = find_parity(word, b, &pb);
    if (a == b) {
      if ((pa ^ pb) != rel) atomicOr(odd, 1ull);
      return;
    }
    if (a < b) {
      uint32_t t = a;
      a = b;
      b = t;
      t = pa;
      pa = pb;
      pb = t;
    }
    const uint32_t old = atomicCAS(word + a, a << 1, (b << 1) | (pa ^ pb ^ rel));  // the larger root under the smaller
    if (old == (a << 1)) return;
    pa ^= old & 1u;  // a had been hooked already: go on from its true pair (ancestor < a)
    a = old >> 1;
  }
}

// One thread per run of exactly two sides (at its first entry).
__global__ __launch_bounds__(kT) void k_mk_parity_union(const uint64_t* keys, const uint32_t* vals,
                                                        const int32_t* tris, int64_t n3, uint32_t* word,
                                                        unsigned long long* cnt) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= n3 || prim::run_sides(keys, i, n3) != 2) return;
  const Side a = side_of(tris, vals[i]), b = side_of(tris, vals[i + 1]);
  const uint32_t rel = (a.from < a.to) == (b.from < b.to) ? 1u : 0u;
  if (a.t == b.t || a.from == a.to) {  // one triangle, or two loops {v, v} (rel = 1): no flip changes the pair
    if (rel) atomicOr(cnt + kOdd, 1ull);
    return;
  }
  unite_parity(word, a.t, b.t, rel, cnt + kOdd);
}

// After the unions (plain loads): the parity to the root is the flip; apply = 0 copies.
__global__ __launch_bounds__(kT) void k_mk_orient(const uint32_t* word, const int32_t* tris, int64_t n_t, int apply,
                                                  int32_t* out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  uint32_t x = static_cast<uint32_t>(t), p = 0u;
  if (apply)
    for (uint32_t w = word[x]; (w >> 1) != x; w = word[x]) {  // strictly decreasing
      p ^= w & 1u;
      x = w >> 1;
    }
  const int32_t b = tris[3 * t + 1], c = tris[3 * t + 2];
  out[3 * t] = tris[3 * t];
  out[3 * t + 1] = p ? c : b;
  out[3 * t + 2] = p ? b : c;
}

__global__ __launch_bounds__(kT) void k_mk_measure(const double* verts, const int32_t* tris, int64_t n_t, double* area,
                                                   double* vol) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  const prim::D3 p0 = prim::ld3(verts, tris[3 * t]), p1 = prim::ld3(verts, tris[3 * t + 1]),
                 p2 = prim::ld3(verts, tris[3 * t + 2]);
  area[t] = prim::tri_area(p0, p1, p2);
  const double c0 = p1.y * p2.z - p1.z * p2.y, c1 = p1.z * p2.x - p1.x * p2.z, c2 = p1.x * p2.y - p1.y * p2.x;
  vol[t] = ((p0.x * c0 + p0.y * c1) + p0.z * c2) / 6.0;
}

__global__ __launch_bounds__(kT) void k_mk_keep(const int32_t* tris, int64_t n_t, uint32_t* keep) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t < n_t) keep[t] = degenerate(tris, t) ? 0u : 1u;
}

}  // namespace mck
}  // namespace

extern "C" {

int sl_mesh_check(sl_ctx* c, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                  int allow_boundary_edges, int64_t* counts, int32_t* edges, int32_t* vertices, int32_t* oriented,
                  void* stream) {
  using namespace mck;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !counts || (n_triangles && !triangles))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_check: bad sizes or NULL arguments");
  for (int i = 0; i < 8; ++i) counts[i] = 0;
  counts[6] = 1;  // no triangles: orientable
  for (double& v : tls_ms) v = 0.0;
  const int64_t n = n_triangles, n3 = 3 * n_triangles;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n, n_vertices, "sl_mesh_check: triangle index out of range", s);
  if (r) return r;
  prim::StageClock clock(s);
  const uint64_t nv = static_cast<uint64_t>(n_vertices);
  prim::SideTable S;
  DBuf<uint32_t> parent, word;
  DBuf<unsigned long long> cnt;
  MTRY(c, parent.alloc(n3));
  MTRY(c, word.alloc(n));
  MTRY(c, cnt.alloc(kCounters));
  MTRY(c, hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * kCounters, s));
  r = prim::sort_sides(c, triangles, n, nv, S, parent.p, word.p, cnt.p + kDegenerate, clock, &tls_ms[0], &tls_ms[1], s);
  if (r) return r;
  {
    DBuf<uint32_t> flag, pos;
    if (edges) {
      MTRY(c, flag.alloc(n3));
      MTRY(c, pos.alloc(n3));
    }
    hipLaunchKernelGGL(k_mk_classify, dim3(blocks(n3)), dim3(kT), 0, s, S.keys.p, S.vals.p, triangles, n3,
                       allow_boundary_edges, cnt.p, flag.p);
    MTRY(c, hipGetLastError());
    if (edges) {
      int64_t rows = 0;
      r = scan_flags(c, flag.p, n3, pos.p, &rows, s);
      if (r) return r;
      hipLaunchKernelGGL(k_mk_edge_list, dim3(blocks(n3)), dim3(kT), 0, s, S.keys.p, flag.p, pos.p, n3, nv, edges);
      MTRY(c, hipGetLastError());
    }
    MTRY(c, clock.lap(&tls_ms[2]));
  }
  {
    DBuf<uint32_t> nroots, flag, pos;
    MTRY(c, nroots.alloc(n_vertices));
    MTRY(c, flag.alloc(n_vertices));
    MTRY(c, pos.alloc(n_vertices));
    MTRY(c, hipMemsetAsync(nroots.p, 0, sizeof(uint32_t) * n_vertices, s));
    hipLaunchKernelGGL(k_mk_corner_union, dim3(blocks(n3)), dim3(kT), 0, s, S.keys.p, S.vals.p, triangles, n3,
                       parent.p);
    hipLaunchKernelGGL(k_mk_corner_roots, dim3(blocks(n3)), dim3(kT), 0, s, parent.p, triangles, n3, nroots.p);
    hipLaunchKernelGGL(k_mk_vertex_flags, dim3(blocks(n_vertices)), dim3(kT), 0, s, nroots.p, n_vertices, flag.p);
    MTRY(c, hipGetLastError());
    r = scan_flags(c, flag.p, n_vertices, pos.p, &counts[4], s);
    if (r) return r;
    if (vertices && counts[4]) {
      hipLaunchKernelGGL(k_mk_vertex_list, dim3(blocks(n_vertices)), dim3(kT), 0, s, flag.p, pos.p, n_vertices,
                         vertices);
      MTRY(c, hipGetLastError());
    }
    MTRY(c, clock.lap(&tls_ms[3]));
  }
  hipLaunchKernelGGL(k_mk_parity_union, dim3(blocks(n3)), dim3(kT), 0, s, S.keys.p, S.vals.p, triangles, n3, word.p,
                     cnt.p);
  MTRY(c, hipGetLastError());
  unsigned long long h[kCounters];
  MTRY(c, hipMemcpyAsync(h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, s));
  MTRY(c, clock.lap(&tls_ms[4]));
  counts[0] = static_cast<int64_t>(h[kUnique]);
  counts[1] = static_cast<int64_t>(h[kBoundary]);
  counts[2] = static_cast<int64_t>(h[kNonManifold]);
  counts[3] = static_cast<int64_t>(h[kInconsistent]);
  counts[5] = static_cast<int64_t>(h[kDegenerate]);
  counts[6] = h[kNonManifold] == 0 && h[kOdd] == 0 ? 1 : 0;
  counts[7] = counts[2] + (allow_boundary_edges ? 0 : counts[1]);
  if (oriented) {
    hipLaunchKernelGGL(k_mk_orient, dim3(blocks(n)), dim3(kT), 0, s, word.p, triangles, n, static_cast<int>(counts[6]),
                       oriented);
    MTRY(c, hipGetLastError());
    MTRY(c, clock.lap(&tls_ms[5]));
  }
  return SL_OK;
}

int sl_mesh_check_stats(double* stage_ms, int capacity) {
  return prim::copy_stats(mck::tls_ms, stage_ms, capacity);
}

int sl_mesh_measure(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                    int64_t n_triangles, double* area, double* volume, void* stream) {
  using namespace mck;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !area || !volume || (n_triangles && !triangles) ||
      (n_vertices && !vertices))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_measure: bad sizes or NULL arguments");
  *area = *volume = 0.0;
  for (double& v : tls_ms) v = 0.0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n_triangles, n_vertices, "sl_mesh_measure: triangle index out of range", s);
  if (r) return r;
  if (n_vertices) {
    r = require_finite(c, vertices, n_vertices, "sl_mesh_measure: non-finite vertex coordinates", s);
    if (r) return r;
  }
  if (n_triangles == 0) return SL_OK;
  prim::StageClock clock(s);
  DBuf<double> a, w;
  MTRY(c, a.alloc(n_triangles));
  MTRY(c, w.alloc(n_triangles));
  hipLaunchKernelGGL(k_mk_measure, dim3(blocks(n_triangles)), dim3(kT), 0, s, vertices, triangles, n_triangles, a.p,
                     w.p);
  MTRY(c, hipGetLastError());
  r = sl_ordered_sum(c, a.p, n_triangles, 1, 0, area, stream);
  if (r) return r;
  r = sl_ordered_sum(c, w.p, n_triangles, 1, 0, volume, stream);
  if (r) return r;
  MTRY(c, clock.lap(&tls_ms[6]));
  return SL_OK;
}

int sl_mesh_remove_degenerate(sl_ctx* c, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                              int32_t* out_triangles, int64_t* out_n_triangles, void* stream) {
  using namespace mck;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !out_n_triangles || (n_triangles && (!triangles || !out_triangles)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_remove_degenerate: bad sizes or NULL arguments");
  *out_n_triangles = 0;
  const int64_t n = n_triangles;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n, n_vertices, "sl_mesh_remove_degenerate: triangle index out of range", s);
  if (r) return r;
  DBuf<uint32_t> keep, pos;
  MTRY(c, keep.alloc(n));
  MTRY(c, pos.alloc(n));
  hipLaunchKernelGGL(k_mk_keep, dim3(blocks(n)), dim3(kT), 0, s, triangles, n, keep.p);
  MTRY(c, hipGetLastError());
  r = compact_rows<int32_t, 3>(c, triangles, n, keep.p, pos.p, out_triangles, out_n_triangles, s);
  if (r) return r;
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_remove_duplicated_triangles(sl_ctx* c, const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                        int32_t* out_triangles, int64_t* out_n_triangles, void* stream) {
  using namespace mck;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !out_n_triangles || (n_triangles && (!triangles || !out_triangles)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_remove_duplicated_triangles: bad sizes or NULL arguments");
  *out_n_triangles = 0;
  const int64_t n = n_triangles;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n, n_vertices,
                          "sl_mesh_remove_duplicated_triangles: triangle index out of range", s);
  if (r) return r;
  DBuf<uint64_t> keys;
  DBuf<uint32_t> rot, ok, vals, head, pos;
  MTRY(c, rot.alloc(3 * n));
  MTRY(c, ok.alloc(n));
  MTRY(c, keys.alloc(n));
  MTRY(c, vals.alloc(n));
  MTRY(c, head.alloc(n));
  MTRY(c, pos.alloc(n));
  hipLaunchKernelGGL(prim::k_sc_tris, dim3(blocks(n)), dim3(kT), 0, s, triangles, n,
                     static_cast<const uint32_t*>(nullptr), rot.p, ok.p);
  MTRY(c, hipGetLastError());
  r = sort_triples(c, rot.p, n, static_cast<uint64_t>(n_vertices), 0xffffffffu, keys.p, vals.p, s);
  if (r) return r;
  hipLaunchKernelGGL(prim::k_sc_heads, dim3(blocks(n)), dim3(kT), 0, s, rot.p, vals.p, n, head.p);
  MTRY(c, hipGetLastError());
  r = compact_rows<int32_t, 3>(c, triangles, n, head.p, pos.p, out_triangles, out_n_triangles, s);  // as given
  if (r) return r;
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

}  // extern "C"
