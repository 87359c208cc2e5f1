// libslgpu.so, part 2n -- mesh hole filling, included at the end of slmerge.hip (one translation unit: it uses that
// file's scratch pool, scan and bounds, and slprim.inl's side table, union-find, input checks and stage clock).
// mesh.check can say that a mesh has holes; this closes the ones that are plain loops.  Open3D's tensor
// fill_holes(hole_size) is not in this image: parity with it is UNPINNED, the definitions below are this library's
// own, and tests/meshfill_oracle.py restates them; the results equal it exactly.  Nothing depends on the order in
// which sides, loops or vertices are visited, or on the order of the atomics.
//
// Input: as sl_mesh_check (triangles int32 [T][3], V < 2^31, 3 T < 2^32), vertices f64 [V][3].
// prim::require_indices and prim::require_finite run before anything is indexed.
//
//   boundary side  a side a->b of a triangle whose edge key has one side in all (slmeshcheck.inl's m = 1, with its
//             treatment of degenerate triangles: (a, a, b) gives the self-loop a->a).
//   simple vertex  exactly one boundary side leaves it and exactly one enters it.
//   component  two boundary sides are joined iff they share an end vertex, in either role.  Its LABEL is its
//             smallest vertex index (components share no vertex: labels are unique), its SIZE n its number of
//             sides, its EXTENT the diagonal of the axis-aligned box of its vertices, sqrt((dx dx + dy dy) + dz dz),
//             f64, uncontracted (min and max are exact in any order).
//   simple loop  a component every vertex of which is simple: one cycle.
//   eligible  a simple loop with 3 <= n <= 2^22 (n = 1 is the self-loop of a degenerate triangle; n = 2 cannot
//             occur, both sides would have one key), n <= max_hole_edges and extent <= hole_size where those are
//             given.  Everything else -- components with a non-simple vertex, such as two holes that touch or the
//             open fans at a non-manifold vertex, and the loops over a limit -- is left as it is and counted.
//   cap       n = 3, a->b->c->a with a the label: the one triangle (a, c, b), no new vertex.  n > 3: one new vertex
//             at the loop's centroid and per side a->b the triangle (b, a, centre), wound against the side, so a
//             consistent mesh stays consistent.  DEVIATION: a centroid fan, not a minimal-area triangulation.
//   centroid  by fixed point, as slmeshwrite.inl's vertex normals: lo = the component-wise minimum over ALL V
//             vertices, e = the largest component of max - lo, s = 2^(40 - k) with e < 2^k (frexp; e = 0: s = 1; k
//             is taken as at least -983 so that s is finite; an infinite e is SL_EINVAL).  Every loop vertex adds
//             llrint((x - lo) s) per component to an int64 sum S (below 2^40 each, at most 2^22 of them); the
//             centre is lo + (double(S) / double(n)) / s.
//   order     the old V vertices first, untouched, then the new ones in ascending label of their loops; the old T
//             triangles first, untouched, then the new ones in ascending from-vertex a of their sides (the one
//             triangle of an n = 3 loop at its label).  A simple loop's vertices each leave once and no two loops
//             share one, so both orders are flags over the V vertices and a scan: no second sort.
//
// Steps.  prim::sort_sides leaves the sorted side table.  k_mf_flag marks the runs of one side (prim::run_sides);
// scan_flags numbers them; k_mf_sides writes the (from, to) rows, counts the sides that leave and enter every
// vertex (integer atomics) and keeps the smallest side at each vertex by atomicMin.  k_mf_union: side j unites with
// the representative side of each of its two ends (prim::unite: the smallest side of a component is its root).
// After the kernel boundary k_mf_gather walks to the root (prim::root_of) and accumulates per root: the bad flag,
// the label (atomicMin), the size, the box as order-preserving integer images of the doubles (atomicMin / atomicMax),
// the three fixed-point sums and the sum of the vertex indices (of a triangle loop a, b, c the side a->b finds c as
// that sum - a - b).  k_mf_roots decides per root, k_mf_tflags raises the from-vertices, two scans, k_mf_emit writes.

namespace {
namespace mfl {

enum { kComponents, kSimple, kFilled, kNotSimple, kOverLimit, kNewVertices, kNewTriangles, kCounters };
enum { kSkip = 0u, kTriangle = 1u, kFan = 2u };
constexpr unsigned long long kMaxLoopSides = 1ull << 22;
// per root: acc[kAcc r + ...] and info[kInfo r + ...]
enum { aMin = 0, aMax = 3, aSum = 6, aIndex = 9, kAcc = 10 };
enum { iBad = 0, iLabel = 1, iSize = 2, kInfo = 3 };

thread_local double tls_ms[6];  // side keys, sort, boundary sides, unions, per-loop sums, caps

using prim::bad_sizes, prim::require_finite, prim::require_indices, prim::wave_add;

// An integer whose unsigned order is the order of the (finite) doubles, and back.
__device__ __forceinline__ unsigned long long image(double x) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x));
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double unimage(unsigned long long u) {
  return __longlong_as_double(static_cast<long long>((u >> 63) ? (u & ~(1ull << 63)) : ~u));
}

__global__ __launch_bounds__(kT) void k_mf_flag(const uint64_t* keys, int64_t n3, uint32_t* flag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < n3) flag[i] = prim::run_sides(keys, i, n3) == 1 ? 1u : 0u;
}

// The flagged sides as rows j = pos[i]; the per-vertex degrees and smallest side; row j's accumulators start empty.
__global__ __launch_bounds__(kT) void k_mf_sides(const uint32_t* vals, const int32_t* tris, const uint32_t* flag,
                                                 const uint32_t* pos, int64_t n3, uint32_t* from, uint32_t* to,
                                                 uint32_t* parent, uint32_t* deg_out, uint32_t* deg_in, uint32_t* rep,
                                                 uint32_t* info, unsigned long long* acc) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= n3 || !flag[i]) return;
  const uint32_t j = pos[i];
  const prim::Side sd = prim::side_of(tris, vals[i]);
  from[j] = sd.from;
  to[j] = sd.to;
  parent[j] = j;
  atomicAdd(deg_out + sd.from, 1u);
  atomicAdd(deg_in + sd.to, 1u);
  atomicMin(rep + sd.from, j);
  atomicMin(rep + sd.to, j);
  uint32_t* fi = info + static_cast<int64_t>(kInfo) * j;
  fi[iBad] = 0u;
  fi[iLabel] = 0xffffffffu;
  fi[iSize] = 0u;
  unsigned long long* a = acc + static_cast<int64_t>(kAcc) * j;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[aMin + k] = ~0ull;
    a[aMax + k] = 0ull;
    a[aSum + k] = 0ull;
  }
  a[aIndex] = 0ull;
}

__global__ __launch_bounds__(kT) void k_mf_union(const uint32_t* from, const uint32_t* to, const uint32_t* rep,
                                                 int64_t nb, uint32_t* parent) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= nb) return;
  prim::unite(parent, static_cast<uint32_t>(j), rep[from[j]]);
  prim::unite(parent, static_cast<uint32_t>(j), rep[to[j]]);
}

// After the unions (a kernel boundary: plain loads).  verts may be NULL: no box and no sums.
__global__ __launch_bounds__(kT) void k_mf_gather(const uint32_t* from, const uint32_t* to, const uint32_t* parent,
                                                  const uint32_t* deg_out, const uint32_t* deg_in,
                                                  const double* verts, int64_t nb, double lo0, double lo1, double lo2,
                                                  double s, uint32_t* root, uint32_t* info, unsigned long long* acc) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= nb) return;
  const uint32_t r = prim::root_of(parent, static_cast<uint32_t>(j));
  root[j] = r;
  const uint32_t a = from[j], b = to[j];
  uint32_t* fi = info + static_cast<int64_t>(kInfo) * r;
  if (deg_out[a] != 1u || deg_in[a] != 1u || deg_out[b] != 1u || deg_in[b] != 1u) atomicOr(fi + iBad, 1u);
  atomicMin(fi + iLabel, a < b ? a : b);
  atomicAdd(fi + iSize, 1u);
  unsigned long long* ac = acc + static_cast<int64_t>(kAcc) * r;
  atomicAdd(ac + aIndex, static_cast<unsigned long long>(a));
  if (!verts) return;
  const double lo[3] = {lo0, lo1, lo2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double xa = verts[3 * static_cast<int64_t>(a) + k], xb = verts[3 * static_cast<int64_t>(b) + k];
    const unsigned long long ia = image(xa), ib = image(xb);
    atomicMin(ac + aMin + k, ia < ib ? ia : ib);
    atomicMax(ac + aMax + k, ia < ib ? ib : ia);
    atomicAdd(ac + aSum + k, static_cast<unsigned long long>(llrint((xa - lo[k]) * s)));  // the from-vertex alone
  }
}

// One live thread per root: the extent, what the component gets, the counters, the flags at its label.
// max_edges < 0, hole_size < 0: no limit.  has_box = 0: no extent (no vertices were given).
__global__ __launch_bounds__(kT) void k_mf_roots(const uint32_t* root, const uint32_t* info,
                                                 const unsigned long long* acc, int64_t nb, int has_box,
                                                 long long max_edges, double hole_size, uint32_t* what, double* extent,
                                                 uint32_t* cflag, uint32_t* vflag, unsigned long long* cnt) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  const bool live = j < nb && root[j] == static_cast<uint32_t>(j);
  bool simple = false, fill = false, fan = false;
  unsigned long long n = 0;
  if (live) {
    const uint32_t* fi = info + static_cast<int64_t>(kInfo) * j;
    const unsigned long long* ac = acc + static_cast<int64_t>(kAcc) * j;
    n = fi[iSize];
    simple = fi[iBad] == 0u;
    double ext = 0.0;
    if (has_box) {
      const double dx = unimage(ac[aMax]) - unimage(ac[aMin]), dy = unimage(ac[aMax + 1]) - unimage(ac[aMin + 1]),
                   dz = unimage(ac[aMax + 2]) - unimage(ac[aMin + 2]);
      ext = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    extent[j] = ext;
    fill = simple && n >= 3ull && n <= kMaxLoopSides && (max_edges < 0 || n <= static_cast<unsigned long long>(max_edges)) &&
           (hole_size < 0.0 || ext <= hole_size);
    fan = fill && n > 3ull;
    what[j] = fan ? kFan : (fill ? kTriangle : kSkip);
    cflag[fi[iLabel]] = 1u;
    if (fan) vflag[fi[iLabel]] = 1u;
  }
  wave_add(cnt + kComponents, live);
  wave_add(cnt + kSimple, simple);
  wave_add(cnt + kFilled, fill);
  wave_add(cnt + kNotSimple, live && !simple);
  wave_add(cnt + kOverLimit, simple && !fill);
  wave_add(cnt + kNewVertices, fan);
}

// The from-vertices that get a triangle: every side of a fan, the side that leaves the label of a triangle loop.
__global__ __launch_bounds__(kT) void k_mf_tflags(const uint32_t* from, const uint32_t* root, const uint32_t* info,
                                                  const uint32_t* what, int64_t nb, uint32_t* tflag,
                                                  unsigned long long* cnt) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  bool emit = false;
  if (j < nb) {
    const uint32_t r = root[j], w = what[r];
    emit = w == kFan || (w == kTriangle && from[j] == info[static_cast<int64_t>(kInfo) * r + iLabel]);
    if (emit) tflag[from[j]] = 1u;
  }
  wave_add(cnt + kNewTriangles, emit);
}

__global__ __launch_bounds__(kT) void k_mf_emit(const uint32_t* from, const uint32_t* to, const uint32_t* root,
                                                const uint32_t* info, const unsigned long long* acc,
                                                const uint32_t* what, const uint32_t* vpos, const uint32_t* tpos,
                                                int64_t nb, int64_t n_v, int64_t n_t, double lo0, double lo1,
                                                double lo2, double s, double* out_verts, int32_t* out_tris) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= nb) return;
  const uint32_t r = root[j], w = what[r], a = from[j], b = to[j];
  const uint32_t label = info[static_cast<int64_t>(kInfo) * r + iLabel];
  const unsigned long long* ac = acc + static_cast<int64_t>(kAcc) * r;
  if (w == kFan) {
    const int64_t centre = n_v + vpos[label];
    int32_t* o = out_tris + 3 * (n_t + tpos[a]);
    o[0] = static_cast<int32_t>(b);
    o[1] = static_cast<int32_t>(a);
    o[2] = static_cast<int32_t>(centre);
    if (static_cast<uint32_t>(j) == r) {
      const double n = static_cast<double>(info[static_cast<int64_t>(kInfo) * r + iSize]), lo[3] = {lo0, lo1, lo2};
#pragma unroll
      for (int k = 0; k < 3; ++k)
        out_verts[3 * centre + k] = lo[k] + (static_cast<double>(static_cast<long long>(ac[aSum + k])) / n) / s;
    }
  } else if (w == kTriangle && a == label) {
    int32_t* o = out_tris + 3 * (n_t + tpos[a]);
    o[0] = static_cast<int32_t>(a);
    o[1] = static_cast<int32_t>(ac[aIndex] - a - b);  // the third vertex of a->b->c->a
    o[2] = static_cast<int32_t>(b);
  }
}

// One row per component at the rank of its label.
__global__ __launch_bounds__(kT) void k_mf_rows(const uint32_t* root, const uint32_t* info, const double* extent,
                                                const uint32_t* cpos, int64_t nb, int32_t* out_label,
                                                int64_t* out_size, uint8_t* out_simple, double* out_extent) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= nb || root[j] != static_cast<uint32_t>(j)) return;
  const uint32_t* fi = info + static_cast<int64_t>(kInfo) * j;
  const int64_t row = cpos[fi[iLabel]];
  out_label[row] = static_cast<int32_t>(fi[iLabel]);
  out_size[row] = static_cast<int64_t>(fi[iSize]);
  out_simple[row] = fi[iBad] ? 0 : 1;
  if (out_extent) out_extent[row] = extent[j];
}

struct Request {  // what the one pass below is asked for (NULL: not written)
  long long max_edges = -1;
  double hole_size = -1.0;
  int32_t* out_label = nullptr;
  int64_t* out_size = nullptr;
  uint8_t* out_simple = nullptr;
  double* out_extent = nullptr;
  double* out_verts = nullptr;
  int32_t* out_tris = nullptr;
};

// The boundary components of a checked mesh (n >= 1 triangles) and, when asked for, their rows or their caps.
int run(sl_ctx* c, const double* verts, int64_t n_v, const int32_t* tris, int64_t n, const Request& q,
        int64_t* counts, hipStream_t s) {
  const int64_t n3 = 3 * n;
  prim::StageClock clock(s);
  prim::SideTable S;
  DBuf<uint32_t> flag, pos;
  int r = prim::sort_sides(c, tris, n, static_cast<uint64_t>(n_v), S, nullptr, nullptr, nullptr, clock, &tls_ms[0],
                           &tls_ms[1], s);
  if (r) return r;
  MTRY(c, flag.alloc(n3));
  MTRY(c, pos.alloc(n3));
  hipLaunchKernelGGL(k_mf_flag, dim3(blocks(n3)), dim3(kT), 0, s, S.keys.p, n3, flag.p);
  MTRY(c, hipGetLastError());
  int64_t nb = 0;
  r = scan_flags(c, flag.p, n3, pos.p, &nb, s);
  if (r) return r;
  counts[7] = nb;
  if (nb == 0) {
    MTRY(c, clock.lap(&tls_ms[2]));
    return SL_OK;
  }
  // the origin and the power of two of the fixed-point sums
  double lo[3] = {0.0, 0.0, 0.0}, scale = 1.0;
  if (verts) {
    double b[6];
    r = bounds(c, verts, n_v, b, s);
    if (r) return r;
    double e = 0.0;
    for (int k = 0; k < 3; ++k) {
      lo[k] = b[k];
      e = std::max(e, b[3 + k] - b[k]);
    }
    if (!std::isfinite(e)) return slgpu_fail(c, SL_EINVAL, "sl_mesh_fill_holes: the extent of the vertices is not finite");
    if (e > 0.0) {
      int k = 0;
      (void)frexp(e, &k);
      scale = ldexp(1.0, 40 - std::max(k, -983));
    }
  }
  DBuf<uint32_t> from, to, parent, root, deg, rep, info, what, vflags;
  DBuf<unsigned long long> acc, cnt;
  DBuf<double> extent;
  MTRY(c, from.alloc(nb));
  MTRY(c, to.alloc(nb));
  MTRY(c, parent.alloc(nb));
  MTRY(c, root.alloc(nb));
  MTRY(c, deg.alloc(2 * n_v));
  MTRY(c, rep.alloc(n_v));
  MTRY(c, info.alloc(kInfo * nb));
  MTRY(c, what.alloc(nb));
  MTRY(c, acc.alloc(kAcc * nb));
  MTRY(c, extent.alloc(nb));
  MTRY(c, cnt.alloc(kCounters));
  MTRY(c, vflags.alloc(3 * n_v));  // the labels of all components, of the fans, the from-vertices of the new triangles
  uint32_t *deg_out = deg.p, *deg_in = deg.p + n_v, *cflag = vflags.p, *vflag = vflags.p + n_v,
           *tflag = vflags.p + 2 * n_v;
  MTRY(c, hipMemsetAsync(deg.p, 0, sizeof(uint32_t) * 2 * n_v, s));
  MTRY(c, hipMemsetAsync(rep.p, 0xff, sizeof(uint32_t) * n_v, s));
  MTRY(c, hipMemsetAsync(vflags.p, 0, sizeof(uint32_t) * 3 * n_v, s));
  MTRY(c, hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long) * kCounters, s));
  hipLaunchKernelGGL(k_mf_sides, dim3(blocks(n3)), dim3(kT), 0, s, S.vals.p, tris, flag.p, pos.p, n3, from.p, to.p,
                     parent.p, deg_out, deg_in, rep.p, info.p, acc.p);
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[2]));
  hipLaunchKernelGGL(k_mf_union, dim3(blocks(nb)), dim3(kT), 0, s, from.p, to.p, rep.p, nb, parent.p);
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[3]));
  hipLaunchKernelGGL(k_mf_gather, dim3(blocks(nb)), dim3(kT), 0, s, from.p, to.p, parent.p, deg_out, deg_in, verts, nb,
                     lo[0], lo[1], lo[2], scale, root.p, info.p, acc.p);
  hipLaunchKernelGGL(k_mf_roots, dim3(blocks(nb)), dim3(kT), 0, s, root.p, info.p, acc.p, nb, verts ? 1 : 0,
                     q.max_edges, q.hole_size, what.p, extent.p, cflag, vflag, cnt.p);
  hipLaunchKernelGGL(k_mf_tflags, dim3(blocks(nb)), dim3(kT), 0, s, from.p, root.p, info.p, what.p, nb, tflag, cnt.p);
  MTRY(c, hipGetLastError());
  unsigned long long h[kCounters];
  MTRY(c, hipMemcpyAsync(h, cnt.p, sizeof(h), hipMemcpyDeviceToHost, s));
  MTRY(c, clock.lap(&tls_ms[4]));
  for (int i = 0; i < kCounters; ++i) counts[i] = static_cast<int64_t>(h[i]);
  DBuf<uint32_t> vpos, tpos;
  if (q.out_label) {
    int64_t rows = 0;
    MTRY(c, vpos.alloc(n_v));
    r = scan_flags(c, cflag, n_v, vpos.p, &rows, s);
    if (r) return r;
    if (rows != counts[kComponents]) return slgpu_fail(c, SL_EHIP, "sl_mesh_boundary_loops: the labels are not unique");
    hipLaunchKernelGGL(k_mf_rows, dim3(blocks(nb)), dim3(kT), 0, s, root.p, info.p, extent.p, vpos.p, nb, q.out_label,
                       q.out_size, q.out_simple, verts ? q.out_extent : nullptr);
    MTRY(c, hipGetLastError());
  }
  if (q.out_tris && counts[kNewTriangles]) {
    int64_t new_v = 0, new_t = 0;
    MTRY(c, vpos.alloc(n_v));
    MTRY(c, tpos.alloc(n_v));
    r = scan_flags(c, vflag, n_v, vpos.p, &new_v, s);
    if (r) return r;
    r = scan_flags(c, tflag, n_v, tpos.p, &new_t, s);
    if (r) return r;
    if (new_v != counts[kNewVertices] || new_t != counts[kNewTriangles])
      return slgpu_fail(c, SL_EHIP, "sl_mesh_fill_holes: the caps' flags do not match their counts");
    hipLaunchKernelGGL(k_mf_emit, dim3(blocks(nb)), dim3(kT), 0, s, from.p, to.p, root.p, info.p, acc.p, what.p, vpos.p,
                       tpos.p, nb, n_v, n, lo[0], lo[1], lo[2], scale, q.out_verts, q.out_tris);
    MTRY(c, hipGetLastError());
  }
  MTRY(c, clock.lap(&tls_ms[5]));
  return SL_OK;
}

// The checks both entry points make before anything is indexed.
int checked(sl_ctx* c, const double* verts, int64_t n_v, const int32_t* tris, int64_t n, const char* index_msg,
            const char* finite_msg, hipStream_t s) {
  int r = require_indices(c, tris, n, n_v, index_msg, s);
  if (r) return r;
  return verts && n_v ? require_finite(c, verts, n_v, finite_msg, s) : SL_OK;
}

}  // namespace mfl
}  // namespace

extern "C" {

int sl_mesh_boundary_loops(sl_ctx* c, const int32_t* triangles, int64_t n_triangles, const double* vertices,
                           int64_t n_vertices, int32_t* out_label, int64_t* out_size, uint8_t* out_simple,
                           double* out_extent, int64_t* counts, void* stream) {
  using namespace mfl;
  if (!c) return SL_EINVAL;
  const bool rows = out_label || out_size || out_simple || out_extent;
  if (bad_sizes(n_vertices, n_triangles) || !counts || (n_triangles && !triangles) ||
      (rows && (!out_label || !out_size || !out_simple)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_boundary_loops: bad sizes or NULL arguments");
  for (int i = 0; i < 8; ++i) counts[i] = 0;
  for (double& v : tls_ms) v = 0.0;
  if (n_triangles == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = checked(c, vertices, n_vertices, triangles, n_triangles, "sl_mesh_boundary_loops: triangle index out of range",
                  "sl_mesh_boundary_loops: non-finite vertex coordinates", s);
  if (r) return r;
  Request q;
  q.out_label = out_label;
  q.out_size = out_size;
  q.out_simple = out_simple;
  q.out_extent = out_extent;
  return run(c, vertices, n_vertices, triangles, n_triangles, q, counts, s);
}

int sl_mesh_fill_holes(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                       int64_t n_triangles, int64_t max_hole_edges, double hole_size, double* out_vertices,
                       int32_t* out_triangles, int64_t* counts, void* stream) {
  using namespace mfl;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !counts || (n_triangles && !triangles) || (n_vertices && !vertices) ||
      (!out_vertices != !out_triangles) || hole_size != hole_size)
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_fill_holes: bad sizes, NULL arguments or a NaN hole_size");
  for (int i = 0; i < 8; ++i) counts[i] = 0;
  for (double& v : tls_ms) v = 0.0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = checked(c, vertices, n_vertices, triangles, n_triangles, "sl_mesh_fill_holes: triangle index out of range",
                  "sl_mesh_fill_holes: non-finite vertex coordinates", s);
  if (r) return r;
  if (out_vertices) {  // the old vertices and triangles are a prefix of the outputs
    if (n_vertices)
      MTRY(c, hipMemcpyAsync(out_vertices, vertices, sizeof(double) * 3 * n_vertices, hipMemcpyDeviceToDevice, s));
    if (n_triangles)
      MTRY(c, hipMemcpyAsync(out_triangles, triangles, sizeof(int32_t) * 3 * n_triangles, hipMemcpyDeviceToDevice, s));
  }
  if (n_triangles) {
    Request q;
    q.max_edges = max_hole_edges < 0 ? -1 : static_cast<long long>(max_hole_edges);
    q.hole_size = hole_size < 0.0 ? -1.0 : hole_size;
    q.out_verts = out_vertices;
    q.out_tris = out_triangles;
    r = run(c, vertices, n_vertices, triangles, n_triangles, q, counts, s);
    if (r) return r;
  }
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_fill_stats(double* stage_ms, int capacity) {
  return prim::copy_stats(mfl::tls_ms, stage_ms, capacity);
}

}  // extern "C"
