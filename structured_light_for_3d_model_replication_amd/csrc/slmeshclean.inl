// libslgpu.so, part 2i -- mesh clean-up after the density trim, included at the
// end of slmerge.hip (one translation unit: it shares that file's scratch pool,
// radix and triple sorts, scan, key runs, row compaction, bounds and voxel grid,
// and slprim.inl's side table, lock-free union-find, triangle area, input checks
// and stage clock).  Open3D users clean a Poisson mesh with
// TriangleMesh::ClusterConnectedTriangles + RemoveTrianglesByMask +
// RemoveUnreferencedVertices and make it coarser with
// SimplifyVertexClustering(voxel_size, Average).  They are restated here; Open3D
// is not in this image, so parity with it is UNPINNED and
// tests/meshclean_oracle.py is the CPU restatement the tests check against,
// exactly.
//
// Input: vertices f64 [V][3], triangles int32 [T][3]; V < 2^31, 3 T < 2^32 (sort
// values and scans are 32-bit).  k_mc_check reads every index before anything is
// indexed: one outside 0 .. V-1 is SL_EINDEX, never a load.
//
//   connected components
//     edges    of (a, b, c): the unordered pairs {a, b}, {b, c}, {c, a} (Open3D's
//              GetOrderedEdge), key min V + max (below 2^62);
//     adjacent two triangles with an edge in common (a shared vertex alone does
//              not connect; an edge of three or more triangles connects them all;
//              (a, a, b) has the edge {a, a} and is otherwise ordinary);
//     cluster  a connected component of that graph;
//     label    the rank of the cluster's smallest triangle index among all
//              clusters' smallest triangle indices, 0, 1, 2, ... -- what Open3D's
//              loop (triangle indices ascending, breadth-first from the first
//              unlabelled one) assigns;
//     count    the cluster's triangles (int64);
//     area     A_t = prim::tri_area(v_a, v_b, v_c): half the length of (v_b - v_a)
//              x (v_c - v_a), f64, uncontracted.  A cluster's area is taken over its
//              triangles in ascending index in blocks of kBlock = 64 consecutive
//              members counted from its first member; a block is a left fold from
//              0.0 and the block sums are a left fold from 0.0 (the kIcpBlock
//              shape).  DEVIATION: Open3D adds in breadth-first order, so its last
//              bits can differ.
//   remove_triangles_by_mask   the masked triangles go, the rest keep their order;
//              vertices are untouched.
//   remove_unreferenced_vertices   the vertices of no triangle go, the rest keep
//              their order, the triangles are re-indexed.
//   simplify_vertex_clustering (contraction Average)
//     grid     bounds over ALL vertices, lo_a = min_a - voxel_size 0.5, voxel =
//              floor((v_a - lo_a) / voxel_size) per axis: sl_voxel_downsample's
//              grid, limits and messages;
//     index    of a voxel: the rank of its smallest member vertex index among all
//              occupied voxels' smallest member indices (Open3D's first-encounter
//              numbering, not key order); a voxel of unreferenced vertices alone
//              still gets a vertex;
//     vertex   the members summed in ascending vertex index from 0.0, divided by
//              the count (k_voxel_avg's arithmetic).  DEVIATION: Open3D iterates
//              an unordered_set here, so its last bits depend on the hash order;
//     triangles in input order: the three indices mapped; dropped if two are
//              equal; rotated cyclically so that the smallest comes first (the
//              orientation is kept, and the opposite orientation is a different
//              triple); the first occurrence of every rotated triple is kept.
//              DEVIATION: output in input order of those first occurrences
//              (Open3D: the order of an unordered_set).
//     The result is in general not manifold: that is the algorithm.
//
// Components on the device.  prim::sort_sides leaves the sorted side table,
// three (key, 3 t + k) pairs per triangle; one thread per sorted position i > 0
// with key[i] == key[i-1] unites the triangles value / 3 of i and i - 1 (run
// neighbours suffice: the chain connects the whole run; the two equal sides of
// one degenerate triangle name the same triangle and are skipped).  parent[] is
// indexed by triangle and starts as the identity.  The union-find is slprim.inl's,
// and the argument in that file's header holds unchanged and is what keeps this
// wait-free: a component's final root is its smallest triangle index whatever
// the interleaving, no workgroup waits on another, and every loop is bounded by
// a strictly decreasing index (the wave folds of the counts by a strictly
// shrinking ballot).  After the kernel boundary the trees are walked with plain loads; the root IS
// the smallest index, so the labels are the flag / scan rank of the roots in
// index order with no min pass.  Counts are integer atomics, one per wave and
// label.  Areas (only when asked for): a stable sort of the triangles by label,
// one thread per triangle for A_t, one per 64-block, one per cluster.
//
// Simplification on the device.  cells() sorts the vertices by voxel key (stable:
// a run's first entry is its smallest index) and leaves the sorted keys' head
// flags and their scan; the heads' flags at their vertex index are scanned for
// the first-encounter rank; one thread per voxel averages.  The mapped, rotated
// triangles that survive are compacted in input order, then sorted by
// sort_triples (stable, value = compacted position: by c, then by a V' + b, up
// to 93 key bits in all); a run head is flagged at its compacted position, the
// flags are scanned and the heads gathered: input order of first occurrences.

namespace {
namespace mcl {

constexpr int kBlock = 64;  // members per area block

thread_local double tls_ms[6];  // edge keys, sort, union, flatten + rank, counts, areas of the last clustering

using prim::require_finite, prim::require_indices, prim::bad_sizes;  // require_indices: k_mc_check

// vals: 3 t + k of the sorted sides
__global__ __launch_bounds__(kT) void k_mc_union(const uint64_t* keys, const uint32_t* vals, int64_t n3,
                                                 uint32_t* parent) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < 1 || i >= n3 || keys[i] != keys[i - 1]) return;
  const uint32_t a = vals[i] / 3u, b = vals[i - 1] / 3u;
  if (a != b) prim::unite(parent, a, b);
}

// After the unions: root[t], and flag[t] = 1 for the roots.
__global__ __launch_bounds__(kT) void k_mc_roots(const uint32_t* parent, int64_t n_t, uint32_t* root, uint32_t* flag) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  const uint32_t x = prim::root_of(parent, static_cast<uint32_t>(t));
  root[t] = x;
  flag[t] = x == static_cast<uint32_t>(t) ? 1u : 0u;
}

__global__ __launch_bounds__(kT) void k_mc_labels(const uint32_t* root, const uint32_t* pos, int64_t n_t,
                                                  int32_t* labels) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t < n_t) labels[t] = static_cast<int32_t>(pos[root[t]]);
}

// counts[label] += 1 per triangle: one atomic per wave and label (neighbours in index mostly share one; a
// cluster of millions otherwise queues them all on one word).  Every lane of the wave takes part; an
// iteration retires its leader, so the ballot shrinks strictly.
__global__ __launch_bounds__(kT) void k_mc_counts(const int32_t* labels, int64_t n_t, unsigned long long* counts) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool pending = t < n_t;
  const int32_t l = pending ? labels[t] : -1;
  for (;;) {
    const unsigned long long m = __ballot(pending);
    if (!m) break;  // wave-uniform
    const int leader = __ffsll(m) - 1;
    const int32_t L = __shfl(l, leader);
    const bool mine = pending && l == L;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) atomicAdd(counts + L, static_cast<unsigned long long>(__popcll(same)));
    pending = pending && !mine;
  }
}

__global__ __launch_bounds__(kT) void k_mc_label_keys(const int32_t* labels, int64_t n_t, uint64_t* keys,
                                                      uint32_t* vals) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  keys[t] = static_cast<uint64_t>(labels[t]);
  vals[t] = static_cast<uint32_t>(t);
}

// A_t of the triangle at sorted position p.
__global__ __launch_bounds__(kT) void k_mc_area(const double* verts, const int32_t* tris, const uint32_t* order,
                                                int64_t n_t, double* area) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (p >= n_t) return;
  const int64_t t = order[p];
  area[p] = prim::tri_area(prim::ld3(verts, tris[3 * t]), prim::ld3(verts, tris[3 * t + 1]),
                           prim::ld3(verts, tris[3 * t + 2]));
}

// nb[c]: the 64-blocks of cluster c (starts: its first sorted position).
__global__ __launch_bounds__(kT) void k_mc_nblocks(const uint32_t* starts, int64_t n_c, int64_t n_t, uint32_t* nb) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (c >= n_c) return;
  const int64_t a = starts[c], b = c + 1 < n_c ? static_cast<int64_t>(starts[c + 1]) : n_t;
  nb[c] = static_cast<uint32_t>((b - a + kBlock - 1) / kBlock);
}

// One thread per block: the left fold from 0.0 of its (up to) 64 areas.  boff: the exclusive scan of nb (every
// cluster has a block, so it is strictly increasing: the block's cluster is the last c with boff[c] <= j).
__global__ __launch_bounds__(kT) void k_mc_block_fold(const double* area, const uint32_t* starts, const uint32_t* boff,
                                                      int64_t n_c, int64_t n_t, int64_t n_b, double* bsum) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= n_b) return;
  int64_t lo = 0, hi = n_c;  // boff[lo] <= j < boff[hi] (boff[n_c] = n_b)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(boff[mid]) <= j) lo = mid;
    else hi = mid;
  }
  const int64_t end = lo + 1 < n_c ? static_cast<int64_t>(starts[lo + 1]) : n_t;
  const int64_t a = static_cast<int64_t>(starts[lo]) + (j - boff[lo]) * kBlock, b = min<int64_t>(end, a + kBlock);
  double s = 0.0;
  for (int64_t p = a; p < b; ++p) s += area[p];
  bsum[j] = s;
}

__global__ __launch_bounds__(kT) void k_mc_cluster_fold(const double* bsum, const uint32_t* boff, int64_t n_c,
                                                        int64_t n_b, double* out) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (c >= n_c) return;
  const int64_t a = boff[c], b = c + 1 < n_c ? static_cast<int64_t>(boff[c + 1]) : n_b;
  double s = 0.0;
  for (int64_t j = a; j < b; ++j) s += bsum[j];
  out[c] = s;
}

// ---- unreferenced vertices
// ref[v] = 1 for every referenced vertex (the same word from every writer; indices were checked)
__global__ __launch_bounds__(kT) void k_mc_mark(const int32_t* tris, int64_t n3, uint32_t* ref) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < n3) ref[tris[i]] = 1u;
}

__global__ __launch_bounds__(kT) void k_mc_remap(const int32_t* tris, int64_t n3, const uint32_t* map, int32_t* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < n3) out[i] = static_cast<int32_t>(map[tris[i]]);
}

// ---- vertex clustering
// flag[v] = 1 for the smallest member of every voxel (idx: the vertices in stable voxel-key order)
__global__ __launch_bounds__(kT) void k_sc_first(const uint32_t* ustart, const uint32_t* idx, int64_t m,
                                                 uint32_t* flag) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (s < m) flag[idx[ustart[s]]] = 1u;
}

// vmap[v]: the new index of v's voxel: the rank of the voxel's smallest member (head / before: the run heads
// of the sorted keys and their exclusive scan, so the run of position p is before[p] + head[p] - 1)
__global__ __launch_bounds__(kT) void k_sc_map(const uint32_t* head, const uint32_t* before, const uint32_t* ustart,
                                               const uint32_t* idx, const uint32_t* rank, int64_t n, uint32_t* vmap) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (p < n) vmap[idx[p]] = rank[idx[ustart[before[p] + head[p] - 1u]]];
}

// One voxel per thread, k_voxel_avg's sums (ascending vertex index from 0.0, / count), stored at the new index.
__global__ __launch_bounds__(kT) void k_sc_avg(const uint32_t* ustart, int64_t m, int64_t n, const uint32_t* idx,
                                               const uint32_t* rank, const double* xyz, double* out) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (s >= m) return;
  const int64_t a = ustart[s], b = s + 1 < m ? static_cast<int64_t>(ustart[s + 1]) : n;
  double p0 = 0.0, p1 = 0.0, p2 = 0.0;
  for (int64_t j = a; j < b; ++j) {
    const int64_t i = idx[j];
    p0 += xyz[3 * i];
    p1 += xyz[3 * i + 1];
    p2 += xyz[3 * i + 2];
  }
  const double cnt = static_cast<double>(b - a);
  const int64_t o = rank[idx[a]];
  out[3 * o] = p0 / cnt;
  out[3 * o + 1] = p1 / cnt;
  out[3 * o + 2] = p2 / cnt;
}

}  // namespace mcl
}  // namespace

extern "C" {

int sl_mesh_cluster_triangles(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                              int64_t n_triangles, int32_t* triangle_clusters, int64_t* cluster_n_triangles,
                              double* cluster_area, int64_t* n_clusters, void* stream) {
  using namespace mcl;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !n_clusters ||
      (n_triangles && (!triangles || !triangle_clusters || !cluster_n_triangles)) || (cluster_area && n_vertices && !vertices))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_cluster_triangles: bad sizes or NULL arguments");
  *n_clusters = 0;
  for (double& v : tls_ms) v = 0.0;
  const int64_t n = n_triangles, n3 = 3 * n_triangles;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n, n_vertices, "sl_mesh_cluster_triangles: triangle index out of range", s);
  if (r) return r;
  if (cluster_area) {
    r = require_finite(c, vertices, n_vertices, "sl_mesh_cluster_triangles: non-finite vertex coordinates", s);
    if (r) return r;
  }
  prim::StageClock clock(s);
  DBuf<uint32_t> parent, root, flag, pos;
  MTRY(c, parent.alloc(n));
  {
    prim::SideTable S;
    hipLaunchKernelGGL(prim::k_clu_init, dim3(blocks(n)), dim3(kT), 0, s, n, parent.p);  // in stage 0, with the keys
    r = prim::sort_sides(c, triangles, n, static_cast<uint64_t>(n_vertices), S, nullptr, nullptr, nullptr, clock,
                         &tls_ms[0], &tls_ms[1], s);
    if (r) return r;
    hipLaunchKernelGGL(k_mc_union, dim3(blocks(n3)), dim3(kT), 0, s, S.keys.p, S.vals.p, n3, parent.p);
    MTRY(c, hipGetLastError());
    MTRY(c, clock.lap(&tls_ms[2]));
  }
  MTRY(c, root.alloc(n));
  MTRY(c, flag.alloc(n));
  MTRY(c, pos.alloc(n));
  hipLaunchKernelGGL(k_mc_roots, dim3(blocks(n)), dim3(kT), 0, s, parent.p, n, root.p, flag.p);
  MTRY(c, hipGetLastError());
  int64_t clusters = 0;
  r = scan_flags(c, flag.p, n, pos.p, &clusters, s);
  if (r) return r;
  hipLaunchKernelGGL(k_mc_labels, dim3(blocks(n)), dim3(kT), 0, s, root.p, pos.p, n, triangle_clusters);
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[3]));
  MTRY(c, hipMemsetAsync(cluster_n_triangles, 0, sizeof(int64_t) * clusters, s));
  hipLaunchKernelGGL(k_mc_counts, dim3(blocks(n)), dim3(kT), 0, s, triangle_clusters, n,
                     reinterpret_cast<unsigned long long*>(cluster_n_triangles));
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[4]));
  if (cluster_area) {
    DBuf<uint64_t> keys, ukeys;
    DBuf<uint32_t> order, seg, starts, nb, boff;
    DBuf<double> area, bsum;
    MTRY(c, keys.alloc(n));
    MTRY(c, order.alloc(n));
    hipLaunchKernelGGL(k_mc_label_keys, dim3(blocks(n)), dim3(kT), 0, s, triangle_clusters, n, keys.p, order.p);
    MTRY(c, hipGetLastError());
    r = radix_sort(c, keys.p, order.p, n, key_bits(static_cast<uint64_t>(clusters - 1)), s);
    if (r) return r;
    // every label 0 .. clusters - 1 occurs, so the run of label l is segment l
    MTRY(c, seg.alloc(n));
    MTRY(c, starts.alloc(clusters));
    MTRY(c, ukeys.alloc(clusters));
    int64_t runs = 0;
    r = key_runs(c, keys.p, n, flag.p, seg.p, &runs, s);
    if (r) return r;
    if (runs != clusters) return slgpu_fail(c, SL_EHIP, "sl_mesh_cluster_triangles: label runs and clusters differ");
    hipLaunchKernelGGL(k_seg_starts, dim3(blocks(n)), dim3(kT), 0, s, flag.p, seg.p, keys.p, n, starts.p, ukeys.p);
    MTRY(c, area.alloc(n));
    hipLaunchKernelGGL(k_mc_area, dim3(blocks(n)), dim3(kT), 0, s, vertices, triangles, order.p, n, area.p);
    MTRY(c, nb.alloc(clusters));
    MTRY(c, boff.alloc(clusters));
    hipLaunchKernelGGL(k_mc_nblocks, dim3(blocks(clusters)), dim3(kT), 0, s, starts.p, clusters, n, nb.p);
    MTRY(c, hipGetLastError());
    int64_t n_b = 0;
    r = scan_flags(c, nb.p, clusters, boff.p, &n_b, s);
    if (r) return r;
    MTRY(c, bsum.alloc(n_b));
    hipLaunchKernelGGL(k_mc_block_fold, dim3(blocks(n_b)), dim3(kT), 0, s, area.p, starts.p, boff.p, clusters, n, n_b,
                       bsum.p);
    hipLaunchKernelGGL(k_mc_cluster_fold, dim3(blocks(clusters)), dim3(kT), 0, s, bsum.p, boff.p, clusters, n_b,
                       cluster_area);
    MTRY(c, hipGetLastError());
    MTRY(c, clock.lap(&tls_ms[5]));
  }
  *n_clusters = clusters;
  return SL_OK;
}

int sl_mesh_cluster_triangles_stats(double* stage_ms, int capacity) {
  return prim::copy_stats(mcl::tls_ms, stage_ms, capacity);
}

int sl_mesh_remove_triangles(sl_ctx* c, const int32_t* triangles, int64_t n_triangles, const uint8_t* mask,
                             int32_t* out_triangles, int64_t* out_n_triangles, void* stream) {
  using namespace mcl;
  if (!c) return SL_EINVAL;
  if (bad_sizes(0, n_triangles) || !out_n_triangles || (n_triangles && (!triangles || !mask || !out_triangles)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_remove_triangles: bad sizes or NULL arguments");
  *out_n_triangles = 0;
  const int64_t n = n_triangles;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  DBuf<uint32_t> keep, pos;
  MTRY(c, keep.alloc(n));
  MTRY(c, pos.alloc(n));
  hipLaunchKernelGGL(k_keep_unmasked, dim3(blocks(n)), dim3(kT), 0, s, mask, n, keep.p);
  MTRY(c, hipGetLastError());
  int r = compact_rows<int32_t, 3>(c, triangles, n, keep.p, pos.p, out_triangles, out_n_triangles, s);
  if (r) return r;
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_remove_unreferenced(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                                int64_t n_triangles, double* out_vertices, int32_t* out_triangles,
                                int64_t* out_n_vertices, void* stream) {
  using namespace mcl;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !out_n_vertices || (n_vertices && (!vertices || !out_vertices)) ||
      (n_triangles && (!triangles || !out_triangles)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_remove_unreferenced: bad sizes or NULL arguments");
  *out_n_vertices = 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, n_triangles, n_vertices, "sl_mesh_remove_unreferenced: triangle index out of range",
                          s);
  if (r) return r;
  if (n_vertices == 0) return SL_OK;
  const int64_t n3 = 3 * n_triangles;
  DBuf<uint32_t> ref, pos;
  MTRY(c, ref.alloc(n_vertices));
  MTRY(c, pos.alloc(n_vertices));
  MTRY(c, hipMemsetAsync(ref.p, 0, sizeof(uint32_t) * n_vertices, s));
  if (n3) hipLaunchKernelGGL(k_mc_mark, dim3(blocks(n3)), dim3(kT), 0, s, triangles, n3, ref.p);
  MTRY(c, hipGetLastError());
  r = compact_rows<double, 3>(c, vertices, n_vertices, ref.p, pos.p, out_vertices, out_n_vertices, s);
  if (r) return r;
  if (n3) hipLaunchKernelGGL(k_mc_remap, dim3(blocks(n3)), dim3(kT), 0, s, triangles, n3, pos.p, out_triangles);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_simplify_clustering(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                                int64_t n_triangles, double voxel_size, double* out_vertices, int32_t* out_triangles,
                                int64_t* out_n_vertices, int64_t* out_n_triangles, void* stream) {
  using namespace mcl;
  if (!c) return SL_EINVAL;
  if (bad_sizes(n_vertices, n_triangles) || !out_n_vertices || !out_n_triangles ||
      (n_vertices && (!vertices || !out_vertices)) || (n_triangles && (!triangles || !out_triangles)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_simplify_clustering: bad sizes or NULL arguments");
  if (!(voxel_size > 0.0)) return slgpu_fail(c, SL_EINVAL, "voxel_size <= 0.");
  *out_n_vertices = *out_n_triangles = 0;
  const int64_t n = n_vertices, nt = n_triangles;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_indices(c, triangles, nt, n, "sl_mesh_simplify_clustering: triangle index out of range", s);
  if (r) return r;
  if (n == 0) return SL_OK;
  r = require_finite(c, vertices, n, "sl_mesh_simplify_clustering: non-finite vertex coordinates", s);
  if (r) return r;
  double b[6];
  r = bounds(c, vertices, n, b, s);
  if (r) return r;
  Grid g;  // sl_voxel_downsample's
  r = voxel_grid(c, b, voxel_size, &g);
  if (r) return r;
  DBuf<uint32_t> vmap;
  MTRY(c, vmap.alloc(n));
  int64_t m = 0;
  {
    DBuf<uint64_t> keys, ukeys;
    DBuf<uint32_t> idx, ustart, flag, seg, first, rank;  // flag, seg: the sorted keys' run heads and their scan
    r = cells(c, vertices, n, g, keys, idx, ukeys, ustart, &m, s, &flag, &seg);
    if (r) return r;
    MTRY(c, first.alloc(n));
    MTRY(c, rank.alloc(n));
    int64_t runs = 0;
    MTRY(c, hipMemsetAsync(first.p, 0, sizeof(uint32_t) * n, s));
    hipLaunchKernelGGL(k_sc_first, dim3(blocks(m)), dim3(kT), 0, s, ustart.p, idx.p, m, first.p);
    MTRY(c, hipGetLastError());
    r = scan_flags(c, first.p, n, rank.p, &runs, s);
    if (r) return r;
    hipLaunchKernelGGL(k_sc_map, dim3(blocks(n)), dim3(kT), 0, s, flag.p, seg.p, ustart.p, idx.p, rank.p, n,
                       vmap.p);
    hipLaunchKernelGGL(k_sc_avg, dim3(blocks(m)), dim3(kT), 0, s, ustart.p, m, n, idx.p, rank.p, vertices,
                       out_vertices);
    MTRY(c, hipGetLastError());
    MTRY(c, hipStreamSynchronize(s));
  }
  *out_n_vertices = m;
  if (nt == 0) return SL_OK;
  DBuf<uint32_t> rot, ok, pos, tri;
  MTRY(c, rot.alloc(3 * nt));
  MTRY(c, ok.alloc(nt));
  MTRY(c, pos.alloc(nt));
  hipLaunchKernelGGL(prim::k_sc_tris, dim3(blocks(nt)), dim3(kT), 0, s, triangles, nt, vmap.p, rot.p, ok.p);
  MTRY(c, hipGetLastError());
  int64_t live = 0;
  r = scan_flags(c, ok.p, nt, pos.p, &live, s);
  if (r) return r;
  if (live == 0) return SL_OK;
  MTRY(c, tri.alloc(3 * live));
  hipLaunchKernelGGL((k_compact_rows<uint32_t, 3>), dim3(blocks(nt)), dim3(kT), 0, s, rot.p, nt, ok.p, pos.p, tri.p);
  MTRY(c, hipGetLastError());
  DBuf<uint64_t> keys;
  DBuf<uint32_t> vals, head, hpos;
  MTRY(c, keys.alloc(live));
  MTRY(c, vals.alloc(live));
  MTRY(c, head.alloc(live));
  MTRY(c, hpos.alloc(live));
  r = sort_triples(c, tri.p, live, static_cast<uint64_t>(m), 0xffffffffu, keys.p, vals.p, s);
  if (r) return r;
  hipLaunchKernelGGL(prim::k_sc_heads, dim3(blocks(live)), dim3(kT), 0, s, tri.p, vals.p, live, head.p);
  MTRY(c, hipGetLastError());
  // the first occurrences in input order (the indices are below 2^31: the same bits as int32)
  r = compact_rows<uint32_t, 3>(c, tri.p, live, head.p, hpos.p, reinterpret_cast<uint32_t*>(out_triangles),
                                out_n_triangles, s);
  if (r) return r;
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

}  // extern "C"
