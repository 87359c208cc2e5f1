// libslgpu.so, part 2k -- vertex colours for a mesh, included at the end of
// slmerge.hip (one translation unit: it uses that file's scratch pool, search
// grid, sort and compaction).  The colour transfer alone: the coloured PLY that
// takes its result is written by slmeshwrite.inl.
// Open3D's create_from_point_cloud_poisson returns vertex_colors when the cloud
// has colours, ball pivoting keeps the input points' colours, and
// o3d.io.write_triangle_mesh writes them as uchar red green blue.  Open3D is not
// in this image: parity is UNPINNED; tests/meshcolor_oracle.py is the CPU form
// the results equal exactly.  DEVIATION: Open3D's Poisson colours come from its
// octree's data field; here a vertex takes an inverse-squared-distance blend of
// its nearest cloud samples, which depends on no order.
//
// transfer_colors(cloud P[n] f64, C[n] BGR u8, queries Q[m] f64, radius r > 0,
// k in 1..16, max_tiers, fill) -> out[m] BGR u8, tier[m] u8:
//   distance     d2(q, p) = ((dx dx + dy dy) + dz dz) in f64, uncontracted.
//   tier radius  r_t = r 2^t (ldexp: exact).  A tier whose r_t r_t is not finite
//                is not run.
//   tier         a query's tier is the smallest t whose open ball d2 < r_t r_t
//                holds a cloud point (grid_nn's strict test).
//   tier limit   t_max = the smallest t with r_t > diag, diag = sqrt((ex ex + ey
//                ey) + ez ez) of the joint bounding box of the cloud and the
//                finite queries; tiers 0 .. t_max run, or 0 .. max_tiers - 1 when
//                that ends sooner (max_tiers < 0: no cap).
//   candidates   in the ball of its tier, up to k points of the least (d2, index).
//   exact hit    the first has d2 == 0: its colour (the lowest index among
//                coincident points).
//   blend        otherwise w_i = d2_first / d2_i (the first is exactly 1, all lie
//                in (0, 1]); den and the three num_c are left folds from 0.0 in
//                candidate order, den = den + w_i, num_c = num_c + w_i double(C[i]
//                [c]); the channel is u8(clamp(rint(num_c / den), 0, 255)), ties
//                to even.
//   unresolved   a non-finite query, an empty cloud, a query with no point by the
//                last tier: `fill` and tier 255.
//   errors       a non-finite cloud coordinate, a radius that is not finite and
//                positive, k outside 1..16: SL_EINVAL; counts from 2^31: SL_EINVAL
//                ("at most 2^31 - 1 points").  m == 0 returns at once; n == 0
//                fills.
//
// Per tier: the cloud's SearchGrid with cells of edge >= r_t (build_search_grid:
// the dense table, or the binary search beyond its limit), the still-unresolved
// queries keyed by their (clamped) cell of that grid and radix-sorted, so that
// neighbouring lanes walk the same cells; one thread per query with its k best
// in a sorted register list (k_normals' list); colour and tier written at the
// query's own index, the rest compacted (compact_rows) for the next tier.  No
// floating-point atomics, nothing spins, no result depends on arrival order.
// Upper tiers: balls that hold many points for few queries.  When the 27 cells
// around a query hold 512 points on average the tier runs one wave per query
// instead (k_vc_query_wave): each lane keeps the k best of every 64th point of
// a cell, and the wave draws the least (d2, index) among the lanes' heads k
// times by a shuffle reduction -- the same candidates in the same order, so the
// same bits.  Not done: staging the candidate cells through LDS for the lower
// tiers (one wave per run of queries in a cell, slcluster.inl's shape);
// DESIGN.md 5.13 says what was measured without it.

namespace {
namespace mcol {

constexpr int kColK = 16;       // largest k
constexpr int kStatTiers = 16;  // tiers the stats list one by one
constexpr int kStats = 5 + kStatTiers;

thread_local double tls_stats[kStats];  // tiers run, filled, grid ms, query ms, resolved per tier, wave tiers

// out = fill, tier = 255, flag = the query is finite, iota = its index
__global__ __launch_bounds__(kT) void k_vc_init(const double* __restrict__ q, int64_t m, uint8_t f0, uint8_t f1,
                                                uint8_t f2, uint8_t* __restrict__ out, uint8_t* __restrict__ tier,
                                                uint32_t* __restrict__ flag, uint32_t* __restrict__ iota) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= m) return;
  out[3 * i] = f0;
  out[3 * i + 1] = f1;
  out[3 * i + 2] = f2;
  if (tier) tier[i] = 255;
  flag[i] = (isfinite(q[3 * i]) && isfinite(q[3 * i + 1]) && isfinite(q[3 * i + 2])) ? 1u : 0u;
  iota[i] = static_cast<uint32_t>(i);
}

__device__ __forceinline__ int64_t clamped_cell(double v, double lo, double h, int64_t n) {
  const double f = floor((v - lo) / h);
  return static_cast<int64_t>(fmin(fmax(f, 0.0), static_cast<double>(n - 1)));
}

// the key of the cloud-grid cell nearest to every unresolved query (its own cell when it lies inside the grid)
__global__ __launch_bounds__(kT) void k_vc_keys(const double* __restrict__ q, const uint32_t* __restrict__ act,
                                                int64_t ma, Grid g, uint64_t* __restrict__ keys) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= ma) return;
  const int64_t i = act[j];
  const int64_t ix = clamped_cell(q[3 * i], g.lo0, g.h, g.nx), iy = clamped_cell(q[3 * i + 1], g.lo1, g.h, g.ny),
                iz = clamped_cell(q[3 * i + 2], g.lo2, g.h, g.nz);
  keys[j] = static_cast<uint64_t>((ix * g.ny + iy) * g.nz + iz);
}

// The first occupied cell whose key is at least `key` (m: none).
__device__ __forceinline__ int64_t first_cell_from(const uint64_t* ukeys, int64_t m, uint64_t key) {
  int64_t a = 0, b = m;
  while (a < b) {
    const int64_t c = (a + b) >> 1;
    if (ukeys[c] < key) a = c + 1;
    else b = c;
  }
  return a;
}

// grid_nn's candidates, the points of the 27 cells around q, taken as nine columns: the up to three cells of one
// (x, y) have consecutive keys, so their points are one run of the sorted cloud, found by one search of the
// occupied cells' keys (or three reads of the dense table) instead of three.  Every `step`-th point of a run from
// its `first`-th on: the KM best by (d2, index) of those inside the open ball into the sorted lists -> how many
// were inside.
template <int KM>
__device__ __forceinline__ int walk(double q0, double q1, double q2, const SearchGrid& sg, double r2, int first,
                                    int step, double (&bd)[KM], uint32_t (&bi)[KM]) {
  const Grid& g = sg.g;
#pragma unroll
  for (int e = 0; e < KM; ++e) {
    bd[e] = INFINITY;
    bi[e] = 0xffffffffu;
  }
  int found = 0;
  const double f0 = floor((q0 - g.lo0) / g.h), f1 = floor((q1 - g.lo1) / g.h), f2 = floor((q2 - g.lo2) / g.h);
  // a query more than a cell outside the grid has no candidate cell
  if (!(f0 >= -1.0 && f0 <= static_cast<double>(g.nx) && f1 >= -1.0 && f1 <= static_cast<double>(g.ny) && f2 >= -1.0 &&
        f2 <= static_cast<double>(g.nz)))
    return 0;
  const int64_t ix = static_cast<int64_t>(f0), iy = static_cast<int64_t>(f1), iz = static_cast<int64_t>(f2);
  const int64_t d_lo = iz > 0 ? iz - 1 : 0, d_hi = iz + 1 < g.nz ? iz + 1 : g.nz - 1;  // (iz in -1 .. nz: never empty)
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy) {
      const int64_t a = ix + dx, b = iy + dy;
      if (a < 0 || a >= g.nx || b < 0 || b >= g.ny) continue;
      const uint64_t base = static_cast<uint64_t>((a * g.ny + b) * g.nz);
      int64_t c0 = -1, c1 = -1;  // the column's first and last occupied cell
      if (sg.dense) {
        for (int64_t d = d_lo; d <= d_hi; ++d) {
          const int64_t cc = sg.dense[base + static_cast<uint64_t>(d)];
          if (cc < 0) continue;
          if (c0 < 0) c0 = cc;
          c1 = cc;
        }
      } else {
        const uint64_t key_hi = base + static_cast<uint64_t>(d_hi);
        const int64_t cc = first_cell_from(sg.ukeys, sg.m, base + static_cast<uint64_t>(d_lo));
        if (cc < sg.m && sg.ukeys[cc] <= key_hi) {
          c0 = c1 = cc;
          while (c1 + 1 < sg.m && sg.ukeys[c1 + 1] <= key_hi) ++c1;
        }
      }
      if (c0 < 0) continue;
      const int64_t t1 = c1 + 1 < sg.m ? static_cast<int64_t>(sg.ustart[c1 + 1]) : sg.n;
      for (int64_t t = static_cast<int64_t>(sg.ustart[c0]) + first; t < t1; t += step) {
        const double d0 = q0 - sg.sxyz[3 * t], d1 = q1 - sg.sxyz[3 * t + 1], d2 = q2 - sg.sxyz[3 * t + 2];
        const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
        if (!(dd < r2)) continue;
        ++found;
        const uint32_t id = sg.sidx[t];
        if (dd < bd[KM - 1] || (dd == bd[KM - 1] && id < bi[KM - 1])) {
          double v = dd;
          uint32_t vi = id;
#pragma unroll
          for (int e = 0; e < KM; ++e) {
            const bool lt = v < bd[e] || (v == bd[e] && vi < bi[e]);
            const double od = bd[e];
            const uint32_t oi = bi[e];
            bd[e] = lt ? v : od;
            bi[e] = lt ? vi : oi;
            v = lt ? od : v;
            vi = lt ? oi : vi;
          }
        }
      }
    }
  return found;
}

// The header's fold, one candidate at a time in (d2, index) order.
struct Blend {
  double first = 0.0, den = 0.0, num[3] = {0.0, 0.0, 0.0};
  uint32_t hit = 0xffffffffu;  // the first candidate's index when its d2 is 0
  int cnt = 0;
  __device__ __forceinline__ void add(double dd, uint32_t id, const uint8_t* __restrict__ bgr) {
    if (cnt == 0) {
      first = dd;
      if (dd == 0.0) hit = id;
    }
    ++cnt;
    if (hit != 0xffffffffu) return;
    const double w = first / dd;
    den = den + w;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) num[ch] = num[ch] + w * static_cast<double>(bgr[3 * static_cast<int64_t>(id) + ch]);
  }
  __device__ __forceinline__ void store(const uint8_t* __restrict__ bgr, uint8_t* __restrict__ out) const {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      out[ch] = hit != 0xffffffffu ? bgr[3 * static_cast<int64_t>(hit) + ch]
                                   : static_cast<uint8_t>(fmin(fmax(rint(num[ch] / den), 0.0), 255.0));
  }
};

// One unresolved query per thread, in cell order, its KM best in a sorted register list.  A query with a point in
// its ball writes colour and tier; unres[j] says whether it stays for the next tier.
template <int KM>
__global__ __launch_bounds__(kT) void k_vc_query(const double* __restrict__ q, const uint32_t* __restrict__ act,
                                                 int64_t ma, SearchGrid sg, const uint8_t* __restrict__ bgr, double r2,
                                                 int k, int tier_no, uint8_t* __restrict__ out,
                                                 uint8_t* __restrict__ tier, uint32_t* __restrict__ unres) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= ma) return;
  const int64_t qi = act[j];
  double bd[KM];
  uint32_t bi[KM];
  const int found = walk<KM>(q[3 * qi], q[3 * qi + 1], q[3 * qi + 2], sg, r2, 0, 1, bd, bi);
  unres[j] = found ? 0u : 1u;
  if (!found) return;
  const int cnt = found < k ? found : k;
  Blend bl;
#pragma unroll
  for (int e = 0; e < KM; ++e)
    if (e < cnt) bl.add(bd[e], bi[e], bgr);
  bl.store(bgr, out + 3 * qi);
  if (tier) tier[qi] = static_cast<uint8_t>(tier_no);
}

// The same result with one wave per query, for tiers whose balls hold many points and whose queries are few:
// lane l takes every 64th point of each cell into a list of its own, then the wave draws the least (d2, index)
// among the lists' heads k times (a shuffle reduction; every point is in one lane's list, so the winner is one
// lane, which drops its head) and folds the winners in that order.  Nothing waits on another wave.
template <int KM>
__global__ __launch_bounds__(kT) void k_vc_query_wave(const double* __restrict__ q, const uint32_t* __restrict__ act,
                                                      int64_t ma, SearchGrid sg, const uint8_t* __restrict__ bgr,
                                                      double r2, int k, int tier_no, uint8_t* __restrict__ out,
                                                      uint8_t* __restrict__ tier, uint32_t* __restrict__ unres) {
  const int lane = threadIdx.x & 63;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * (kT / 64) + (threadIdx.x >> 6);
  if (j >= ma) return;  // (wave-uniform)
  const int64_t qi = act[j];
  double bd[KM];
  uint32_t bi[KM];
  (void)walk<KM>(q[3 * qi], q[3 * qi + 1], q[3 * qi + 2], sg, r2, lane, 64, bd, bi);
  Blend bl;
  for (int e = 0; e < k; ++e) {
    double v = bd[0];
    uint32_t vi = bi[0];
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const double ov = __shfl_xor(v, o);
      const uint32_t oi = __shfl_xor(vi, o);
      const bool lt = ov < v || (ov == v && oi < vi);
      v = lt ? ov : v;
      vi = lt ? oi : vi;
    }
    if (vi == 0xffffffffu) break;  // every list is empty (wave-uniform)
    if (bi[0] == vi) {
#pragma unroll
      for (int f = 0; f + 1 < KM; ++f) {
        bd[f] = bd[f + 1];
        bi[f] = bi[f + 1];
      }
      bd[KM - 1] = INFINITY;
      bi[KM - 1] = 0xffffffffu;
    }
    bl.add(v, vi, bgr);
  }
  if (lane) return;
  unres[j] = bl.cnt ? 0u : 1u;
  if (!bl.cnt) return;
  bl.store(bgr, out + 3 * qi);
  if (tier) tier[qi] = static_cast<uint8_t>(tier_no);
}

// A tier goes to the wave kernel when the 27 cells around a query hold kWavePoints points on average: the results
// are the same, so the choice is about time alone.
constexpr int64_t kWavePoints = 512;

template <int KM>
void launch_query(bool wave, const double* q, const uint32_t* act, int64_t ma, const SearchGrid& sg, const uint8_t* bgr,
                  double r2, int k, int tier_no, uint8_t* out, uint8_t* tier, uint32_t* unres, hipStream_t s) {
  if (wave)
    hipLaunchKernelGGL((k_vc_query_wave<KM>), dim3(blocks(64 * ma)), dim3(kT), 0, s, q, act, ma, sg, bgr, r2, k, tier_no,
                       out, tier, unres);
  else
    hipLaunchKernelGGL((k_vc_query<KM>), dim3(blocks(ma)), dim3(kT), 0, s, q, act, ma, sg, bgr, r2, k, tier_no, out,
                       tier, unres);
}

}  // namespace mcol
}  // namespace

extern "C" {

int sl_mesh_transfer_colors(sl_ctx* c, const double* cloud_xyz, const uint8_t* cloud_bgr, int64_t n,
                            const double* query_xyz, int64_t m, double radius, int k, int max_tiers,
                            const uint8_t* fill_bgr, uint8_t* out_bgr, uint8_t* out_tier, void* stream) {
  using namespace mcol;
  if (!c) return SL_EINVAL;
  if (n < 0 || m < 0 || !fill_bgr || (n && (!cloud_xyz || !cloud_bgr)) || (m && (!query_xyz || !out_bgr)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_transfer_colors: bad sizes or NULL arguments");
  if (n >= (1ll << 31) || m >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  if (!(std::isfinite(radius) && radius > 0.0))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_transfer_colors: radius must be finite and > 0");
  if (k < 1 || k > kColK) return slgpu_fail(c, SL_EINVAL, "sl_mesh_transfer_colors: k must be 1..16");
  for (double& v : tls_stats) v = 0.0;
  if (m == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  DBuf<uint32_t> flag, pos, iota, act_a, act_b;
  MTRY(c, flag.alloc(m));
  MTRY(c, pos.alloc(m));
  MTRY(c, iota.alloc(m));
  MTRY(c, act_a.alloc(m));
  MTRY(c, act_b.alloc(m));
  hipLaunchKernelGGL(k_vc_init, dim3(blocks(m)), dim3(kT), 0, s, query_xyz, m, fill_bgr[0], fill_bgr[1], fill_bgr[2],
                     out_bgr, out_tier, flag.p, iota.p);
  MTRY(c, hipGetLastError());
  tls_stats[1] = static_cast<double>(m);
  if (n == 0) {
    MTRY(c, hipStreamSynchronize(s));
    return SL_OK;
  }
  int r = prim::require_finite(c, cloud_xyz, n, "non-finite cloud coordinates", s);
  if (r) return r;
  uint32_t *act = act_a.p, *next = act_b.p;
  int64_t ma = 0;
  r = compact_rows<uint32_t, 1>(c, iota.p, m, flag.p, pos.p, act, &ma, s);
  if (r) return r;
  if (ma == 0) {
    MTRY(c, hipStreamSynchronize(s));
    return SL_OK;
  }
  // the joint bounding box of the cloud and the finite queries -> t_max
  double bc[6], bq[6];
  {
    DBuf<double> aq;
    MTRY(c, aq.alloc(3 * ma));
    hipLaunchKernelGGL(k_gather_sorted, dim3(blocks(ma)), dim3(kT), 0, s, query_xyz, act, ma, aq.p);
    MTRY(c, hipGetLastError());
    r = bounds(c, aq.p, ma, bq, s);
    if (r) return r;
  }
  r = bounds(c, cloud_xyz, n, bc, s);
  if (r) return r;
  double e[3];
  for (int a = 0; a < 3; ++a) e[a] = std::max(bc[3 + a], bq[3 + a]) - std::min(bc[a], bq[a]);
  const double diag = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  int t_max = 0;
  while (!(ldexp(radius, t_max) > diag) && t_max < 4096) ++t_max;
  DBuf<uint64_t> keys;
  MTRY(c, keys.alloc(m));
  const int64_t finite = ma;
  for (int t = 0; t <= t_max && (max_tiers < 0 || t < max_tiers) && ma > 0; ++t) {
    const double rt = ldexp(radius, t), r2 = rt * rt;
    if (!std::isfinite(r2)) break;
    prim::StageClock clock(s);
    double ms = 0.0;
    SearchGridBufs sb;
    r = build_search_grid(c, cloud_xyz, n, rt, GridTable::kDense, "non-finite cloud coordinates", &sb, s);
    if (r) return r;
    MTRY(c, clock.lap(&ms));
    tls_stats[2] += ms;
    const Grid& g = sb.view.g;
    hipLaunchKernelGGL(k_vc_keys, dim3(blocks(ma)), dim3(kT), 0, s, query_xyz, act, ma, g, keys.p);
    MTRY(c, hipGetLastError());
    r = radix_sort(c, keys.p, act, ma, key_bits(static_cast<uint64_t>((g.nx * g.ny) * g.nz - 1)), s);
    if (r) return r;
    const bool wave = 27 * n >= kWavePoints * sb.view.m;
    if (k <= 4)
      launch_query<4>(wave, query_xyz, act, ma, sb.view, cloud_bgr, r2, k, t, out_bgr, out_tier, flag.p, s);
    else if (k <= 8)
      launch_query<8>(wave, query_xyz, act, ma, sb.view, cloud_bgr, r2, k, t, out_bgr, out_tier, flag.p, s);
    else
      launch_query<16>(wave, query_xyz, act, ma, sb.view, cloud_bgr, r2, k, t, out_bgr, out_tier, flag.p, s);
    if (wave) tls_stats[4 + kStatTiers] += 1.0;
    MTRY(c, hipGetLastError());
    int64_t left = 0;
    r = compact_rows<uint32_t, 1>(c, act, ma, flag.p, pos.p, next, &left, s);
    if (r) return r;
    MTRY(c, clock.lap(&ms));
    tls_stats[3] += ms;
    if (t < kStatTiers) tls_stats[4 + t] = static_cast<double>(ma - left);
    tls_stats[0] = static_cast<double>(t + 1);
    std::swap(act, next);
    ma = left;
  }
  tls_stats[1] = static_cast<double>((m - finite) + ma);
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_transfer_colors_stats(double* stats, int capacity) {
  return prim::copy_stats(mcol::tls_stats, stats, capacity);
}

}  // extern "C"
