// libslgpu.so, part 2g -- density clustering for the per-view clean-up, included
// at the end of slmerge.hip (one translation unit: it shares that file's scratch
// pool, scan, search grid and kNN pyramid, and slprim.inl's union-find, fold_min,
// finite check and stage clock).  The reference's second cleaning
// recipe (Old/StatisticalOutlierRemoval.py, remove_outliers_keep_color2) is
// compute_nearest_neighbor_distance, cluster_dbscan(eps, min_points) + "keep the
// largest cluster", and remove_radius_outlier(nb_points, radius): Open3D calls.
// They are restated here; Open3D is not in this image, so parity with it is
// UNPINNED and tests/cluster_oracle.py is the CPU restatement the tests check
// against, exactly.
//
//   neighbourhood: j is a neighbour of i iff ((dx dx + dy dy) + dz dz) < eps eps,
//     f64, uncontracted, in that order, i itself included -- the strict nanoflann
//     radius test of sl_radius_search / grid_nn, without a max_nn.
//   DBSCAN (PointCloud::ClusterDBSCAN is a sequential loop -- indices ascending,
//     breadth-first expansion, a point first labelled noise re-claimed as a
//     border point; this is its order-free form, which gives the same labels):
//     core    a point whose neighbour count (itself included) is >= min_points;
//     cluster a connected component of the graph on the core points with an edge
//             between neighbours;
//     label   the rank of the cluster's smallest core index among all clusters'
//             smallest core indices: 0, 1, 2, ...;
//     border  a non-core point with a core neighbour takes the SMALLEST label
//             among its core neighbours' clusters (clusters are fully expanded in
//             label order, so the lowest-labelled one reaches it first);
//     noise   a non-core point with no core neighbour: -1.
//     Labels are int32 (Open3D's IntVector).
//   radius count: min(count, cap) of every point (cap <= 0: the exact count).
//     remove_radius_outlier(nb_points, radius) keeps i iff count > nb_points.
//   nearest-neighbour distance: sqrt(d2) of the second entry of the exact 2-NN
//     (itself included; ties by (d2, index), so a duplicated point gives 0); 0 for
//     a cloud of one point.
//
// Traversal (k_ball).  Queries in the search grid's cell-sorted order, 64 per
// one-wave workgroup.  The wave walks its queries' cells one after the other
// (the lanes of that cell are active); for a cell, the 27 neighbour cells of
// edge >= eps are nine runs of consecutive sorted positions (the three cells of a
// z column are neighbours in key order), and every run is staged through LDS in
// tiles of kTile candidates, so a cell of several thousand points is read once
// per workgroup and not once per thread.  All loop bounds are wave-uniform.  A
// wave leaves a cell once none of its active lanes needs more: a count that has
// reached cap, a border point that has found label 0.  Counting is integer and
// the border label a minimum, so no result depends on the visiting order.
//
// Union-find (the clusters).  parent[], like the core flags, is indexed by SORTED
// POSITION (a tile's words are then one contiguous read; indexed by point index
// the two gathers per candidate were most of the pass) and starts as the
// identity.  One traversal unites every core point with its core neighbours of
// lower position (every edge is seen from its later end).  The union-find is
// slprim.inl's (find_root / unite), and that file's header holds the argument
// that it is wait-free and that a stale read of a parent word costs steps and
// never a wrong union; a component's final root is its smallest core position
// whatever the interleaving.  Here "both ends share an ancestor" is the test
// that skips the distance computation.  The cluster's smallest core INDEX,
// which the labels rank, is one atomicMin per core point into its root's slot
// after the unions.  After the launch (a kernel boundary makes everything
// visible) the trees are walked with plain loads to the roots, each root's
// smallest point index is found and those are ranked by the flag / scan
// passes, and a second traversal gives every border point its minimum core
// label.  Nothing on the host iterates until convergence.

namespace {
namespace clu {

using prim::find_root, prim::ld_parent, prim::unite, prim::k_clu_init, prim::require_finite, prim::StageClock;

constexpr int kW = 64;     // one wave per workgroup
constexpr int kTile = 256;  // candidates staged per pass (8 KB of LDS with the two words per candidate)
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kNoLabel = 0x7fffffff;

enum Mode { kCount = 0, kUnion = 1, kBorder = 2 };

thread_local double tls_ms[5];  // grid, count, union, flatten + rank, border of the last sl_cluster_dbscan

// scnt, parent and slab are indexed by SORTED POSITION, so a tile's words are one contiguous read.
// kCount:  min(count, lim) (lim <= 0: the count) -> out[point index] and / or out_pos[position].
// kUnion:  core points (scnt >= lim) united with their core neighbours of lower position.
// kBorder: out[point index] = the smallest slab[] among the core neighbours of the non-core points
//          that have a neighbour besides themselves (the other points' labels are already in out).
template <int MODE>
__global__ __launch_bounds__(kW) void k_ball(SearchGrid sg, double r2, int lim, const int32_t* scnt,
                                             uint32_t* parent, const int32_t* slab, int32_t* out,
                                             int32_t* out_pos) {
  __shared__ double s_p[3 * kTile];
  __shared__ uint32_t s_a[kTile];  // kUnion: the candidate's index (kNone: not core); kBorder: its label
  __shared__ uint32_t s_b[kTile];  // kUnion: the candidate's parent when the tile was staged
  const int lane = threadIdx.x;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kW;
  const int64_t j = j0 + lane;
  const int64_t jend = min<int64_t>(sg.n, j0 + kW);
  const bool in = j < sg.n;
  const double q0 = in ? sg.sxyz[3 * j] : 0.0, q1 = in ? sg.sxyz[3 * j + 1] : 0.0, q2 = in ? sg.sxyz[3 * j + 2] : 0.0;
  const uint32_t qi = in ? sg.sidx[j] : 0u;
  const int mycell = in ? static_cast<int>(find_cell(sg.ukeys, sg.m, sg.skeys[j])) : -1;
  bool live = in && mycell >= 0;
  if (MODE == kUnion) live = live && scnt[j] >= lim;
  if (MODE == kBorder) live = live && scnt[j] < lim && scnt[j] > 1;
  const uint32_t me = static_cast<uint32_t>(j);
  int acc = 0;           // kCount
  int best = kNoLabel;   // kBorder
  uint32_t myroot = me;  // kUnion: an ancestor of this point
  if (MODE == kUnion && live) myroot = find_root(parent, me);
  bool pending = live;
  for (;;) {
    const unsigned long long pm = __ballot(pending);
    if (!pm) break;
    const int c = __shfl(mycell, __ffsll(pm) - 1, kW);  // the next query cell (wave-uniform)
    const bool act = pending && mycell == c;
    pending = pending && !act;
    bool stop = false;
    for (int e = 0; e < 9 && !stop; ++e) {
      // the z column (dx, dy, -1..1): consecutive keys, so consecutive occupied cells and one run of
      // positions.  Counts and border labels: the queries' own column first, then the four that share a
      // face with it (a capped count or a label 0 is usually settled there).  Unions: ascending keys, so
      // a point first meets far, lower cells that earlier waves have already joined into one tree, takes
      // that root, and skips the rest by the parent test (own column first measured 1.6 times slower).
      const int e3 = MODE == kUnion ? e : static_cast<int>((0x862075314ull >> (4 * e)) & 15ull);  // 4 1 3 5 7 0 2 6 8
      const int32_t* nb = sg.nbr + 27 * static_cast<int64_t>(c) + 3 * e3;
      const int c0 = nb[0], c1 = nb[1], c2 = nb[2];
      const int first = c0 >= 0 ? c0 : (c1 >= 0 ? c1 : c2);
      const int last = c2 >= 0 ? c2 : (c1 >= 0 ? c1 : c0);
      if (first < 0) continue;
      const int64_t a = sg.ustart[first];
      int64_t b = static_cast<int64_t>(last) + 1 < sg.m ? static_cast<int64_t>(sg.ustart[last + 1]) : sg.n;
      if (MODE == kUnion) b = min<int64_t>(b, jend - 1);  // only candidates below a query of this wave
      for (int64_t t0 = a; t0 < b; t0 += kTile) {
        bool busy = act;
        if (MODE == kCount) busy = act && !(lim > 0 && acc >= lim);
        if (MODE == kBorder) busy = act && best != 0;
        if (!__any(busy)) {  // no active lane needs another candidate
          stop = true;
          break;
        }
        const int len = static_cast<int>(min<int64_t>(kTile, b - t0));
        __syncthreads();  // the previous tile has been read
        for (int u = lane; u < 3 * len; u += kW) s_p[u] = sg.sxyz[3 * t0 + u];
        uint32_t tile_par = kNone;  // kUnion: the parent of this lane's staged core candidates, if they share one
        bool tile_one = true;
        if (MODE != kCount)
          for (int u = lane; u < len; u += kW) {
            if (MODE == kUnion) {
              const bool core = scnt[t0 + u] >= lim;
              const uint32_t p = core ? ld_parent(parent + t0 + u) : kNone;
              s_a[u] = core ? static_cast<uint32_t>(t0 + u) : kNone;
              s_b[u] = p;
              if (core) {
                tile_one = tile_one && (tile_par == kNone || tile_par == p);
                tile_par = p;
              }
            } else {
              const int l = slab[t0 + u];
              s_a[u] = static_cast<uint32_t>(l < 0 ? kNoLabel : l);
            }
          }
        __syncthreads();
        if (MODE == kUnion) {
          // a tile without a core candidate, or one whose core candidates all hang under the root every
          // active query of the wave has: nothing to unite (wave-uniform)
          const unsigned long long hm = __ballot(tile_par != kNone);
          if (hm == 0) continue;
          const uint32_t one = __shfl(tile_par, __ffsll(hm) - 1, kW);
          if (__all(tile_one && (tile_par == kNone || tile_par == one) && (!act || myroot == one))) continue;
        }
        for (int u = 0; busy && u < len; ++u) {
          if (MODE == kUnion) {
            if (t0 + u >= j) break;  // later ends see this edge
            const uint32_t id = s_a[u];
            if (id == kNone || id == myroot || s_b[u] == myroot) continue;  // not core, or one tree already
          }
          if (MODE == kBorder && static_cast<int>(s_a[u]) >= best) continue;
          const double d0 = q0 - s_p[3 * u], d1 = q1 - s_p[3 * u + 1], d2 = q2 - s_p[3 * u + 2];
          const double dd = (d0 * d0 + d1 * d1) + d2 * d2;  // nanoflann L2_Adaptor order
          if (!(dd < r2)) continue;
          if (MODE == kCount) ++acc;
          if (MODE == kUnion) {
            const uint32_t id = s_a[u];
            myroot = unite(parent, myroot, id);
            if (id != myroot) atomicMin(parent + id, myroot);  // later tiles see the root at once
          }
          if (MODE == kBorder) best = static_cast<int>(s_a[u]);
        }
      }
    }
  }
  if (!live) return;
  if (MODE == kCount) {
    const int v = (lim > 0 && acc > lim) ? lim : acc;
    if (out) out[qi] = v;
    if (out_pos) out_pos[j] = v;
  }
  if (MODE == kUnion && myroot != me) atomicMin(parent + me, myroot);
  if (MODE == kBorder) out[qi] = best == kNoLabel ? -1 : best;
}

// After the unions (a kernel boundary: plain loads), by sorted position: every core point's root
// (kNone: not core), and per root the smallest point index of its component (low[] starts all ones).
__global__ __launch_bounds__(kT) void k_clu_roots(const uint32_t* parent, const int32_t* scnt, int min_points,
                                                  const uint32_t* sidx, int64_t n, uint32_t* root, uint32_t* low) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  const bool core = t < n && scnt[t] >= min_points;
  const uint32_t x = core ? prim::root_of(parent, static_cast<uint32_t>(t)) : kNone;
  if (t < n) root[t] = x;
  // neighbours in position mostly share a root: one atomic per wave and root, not one per point (a
  // cluster of millions otherwise queues them all on one word).  Every lane of the wave calls.
  prim::fold_min<uint32_t>(low, x, core ? sidx[t] : kNone, core);
}

// flag[i] = 1 for the point that is the smallest core index of its cluster (every i is written once).
__global__ __launch_bounds__(kT) void k_clu_heads(const uint32_t* root, const uint32_t* low, const uint32_t* sidx,
                                                  int64_t n, uint32_t* flag) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n) return;
  const uint32_t i = sidx[t], r = root[t];
  flag[i] = (r != kNone && low[r] == i) ? 1u : 0u;
}

// A core point's label: the rank of its cluster's smallest core index among all clusters' (pos: the
// exclusive scan of the heads); -1 for the others.  -> slab (by position) and out (by point index).
__global__ __launch_bounds__(kT) void k_clu_label(const uint32_t* root, const uint32_t* low, const uint32_t* pos,
                                                  const uint32_t* sidx, int64_t n, int32_t* slab, int32_t* out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n) return;
  const uint32_t r = root[t];
  const int32_t l = r == kNone ? -1 : static_cast<int32_t>(pos[low[r]]);
  slab[t] = l;
  out[sidx[t]] = l;
}

__global__ __launch_bounds__(kT) void k_clu_scale(double* v, int64_t n, double f) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < n) v[i] = v[i] * f;
}

unsigned wave_blocks(int64_t n) { return static_cast<unsigned>((n + kW - 1) / kW); }

}  // namespace clu
}  // namespace

extern "C" {

int sl_radius_count(sl_ctx* c, const double* xyz, int64_t n, double radius, int cap, int32_t* out_cnt, void* stream) {
  using namespace clu;
  if (!c) return SL_EINVAL;
  if (n < 0 || (n && (!xyz || !out_cnt))) return slgpu_fail(c, SL_EINVAL, "sl_radius_count: bad sizes or NULL arguments");
  if (!(radius > 0.0) || !std::isfinite(radius)) return slgpu_fail(c, SL_EINVAL, "sl_radius_count: radius must be positive");
  if (n >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_finite(c, xyz, n, "sl_radius_count: non-finite point coordinates", s);
  if (r) return r;
  SearchGridBufs sg;
  r = build_search_grid(c, xyz, n, radius, GridTable::kNeighbours, "sl_radius_count: non-finite point coordinates", &sg,
                        s);
  if (r) return r;
  hipLaunchKernelGGL(k_ball<kCount>, dim3(wave_blocks(n)), dim3(kW), 0, s, sg.view, radius * radius, cap,
                     static_cast<const int32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                     static_cast<const int32_t*>(nullptr), out_cnt, static_cast<int32_t*>(nullptr));
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_cluster_dbscan(sl_ctx* c, const double* xyz, int64_t n, double eps, int min_points, int32_t* labels,
                      int64_t* n_clusters, void* stream) {
  using namespace clu;
  if (!c) return SL_EINVAL;
  if (n < 0 || (n && (!xyz || !labels))) return slgpu_fail(c, SL_EINVAL, "sl_cluster_dbscan: bad sizes or NULL arguments");
  if (!(eps > 0.0) || !std::isfinite(eps)) return slgpu_fail(c, SL_EINVAL, "sl_cluster_dbscan: eps must be positive");
  if (min_points < 1) return slgpu_fail(c, SL_EINVAL, "sl_cluster_dbscan: min_points must be at least 1");
  if (n >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  if (n_clusters) *n_clusters = 0;
  for (double& v : tls_ms) v = 0.0;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_finite(c, xyz, n, "sl_cluster_dbscan: non-finite point coordinates", s);
  if (r) return r;
  StageClock clock(s);
  SearchGridBufs sg;
  r = build_search_grid(c, xyz, n, eps, GridTable::kNeighbours, "sl_cluster_dbscan: non-finite point coordinates", &sg,
                        s);
  if (r) return r;
  MTRY(c, clock.lap(&tls_ms[0]));
  const double r2 = eps * eps;
  const unsigned gw = wave_blocks(n), gv = blocks(n);
  const SearchGrid& v = sg.view;
  DBuf<int32_t> scnt, slab;              // by sorted position: the capped counts, the core points' labels
  DBuf<uint32_t> parent, root, low, flag, pos;
  MTRY(c, scnt.alloc(n));
  MTRY(c, slab.alloc(n));
  MTRY(c, parent.alloc(n));
  MTRY(c, root.alloc(n));
  MTRY(c, low.alloc(n));
  MTRY(c, flag.alloc(n));
  MTRY(c, pos.alloc(n));
  // core flags: the count needs to reach min_points only
  hipLaunchKernelGGL(k_ball<kCount>, dim3(gw), dim3(kW), 0, s, v, r2, min_points,
                     static_cast<const int32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                     static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr), scnt.p);
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[1]));
  hipLaunchKernelGGL(k_clu_init, dim3(gv), dim3(kT), 0, s, n, parent.p);
  hipLaunchKernelGGL(k_ball<kUnion>, dim3(gw), dim3(kW), 0, s, v, r2, min_points, scnt.p, parent.p,
                     static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                     static_cast<int32_t*>(nullptr));
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[2]));
  // roots, each cluster's smallest core index, their rank, the core points' labels
  MTRY(c, hipMemsetAsync(low.p, 0xff, sizeof(uint32_t) * n, s));
  hipLaunchKernelGGL(k_clu_roots, dim3(gv), dim3(kT), 0, s, parent.p, scnt.p, min_points, v.sidx, n, root.p, low.p);
  hipLaunchKernelGGL(k_clu_heads, dim3(gv), dim3(kT), 0, s, root.p, low.p, v.sidx, n, flag.p);
  MTRY(c, hipGetLastError());
  int64_t clusters = 0;
  r = scan_flags(c, flag.p, n, pos.p, &clusters, s);
  if (r) return r;
  hipLaunchKernelGGL(k_clu_label, dim3(gv), dim3(kT), 0, s, root.p, low.p, pos.p, v.sidx, n, slab.p, labels);
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[3]));
  hipLaunchKernelGGL(k_ball<kBorder>, dim3(gw), dim3(kW), 0, s, v, r2, min_points, scnt.p,
                     static_cast<uint32_t*>(nullptr), slab.p, labels, static_cast<int32_t*>(nullptr));
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(&tls_ms[4]));
  if (n_clusters) *n_clusters = clusters;
  return SL_OK;
}

int sl_cluster_dbscan_stats(double* stage_ms, int capacity) {
  return prim::copy_stats(clu::tls_ms, stage_ms, capacity);
}

int sl_nearest_neighbor_distance(sl_ctx* c, const double* xyz, int64_t n, double* out, void* stream) {
  using namespace clu;
  if (!c) return SL_EINVAL;
  if (n < 0 || (n && (!xyz || !out)))
    return slgpu_fail(c, SL_EINVAL, "sl_nearest_neighbor_distance: bad sizes or NULL arguments");
  if (n >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = require_finite(c, xyz, n, "sl_nearest_neighbor_distance: non-finite point coordinates", s);
  if (r) return r;
  // the exact 2-NN of the statistical outlier filter: the mean of sqrt(0) (the point itself, or a
  // duplicate of lower rank) and sqrt(d2) over kk = min(2, n) entries; times kk gives sqrt(d2) back
  // exactly (a division and a multiplication by 2)
  r = knn_mean_dist(c, xyz, n, 2, 2, out, s);
  if (r) return r;
  hipLaunchKernelGGL(k_clu_scale, dim3(blocks(n)), dim3(kT), 0, s, out, n, n >= 2 ? 2.0 : 1.0);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

}  // extern "C"
