// libslgpu.so, part 2c -- background removal of the per-view clean-up
// (server/processing.py:25-52, page 2 of the reference GUI): Open3D's
// PointCloud::SegmentPlane, included at the end of slmerge.hip (one translation
// unit: it shares that file's scan / compact kernels and scratch pool,
// and slprim.inl's draw and the chunk shape, tree and fold kernel of the
// ordered sum defined below).  Open3D is not in this image: the algorithm is restated
// from its published source (geometry/PointCloudSegmentation.cpp), parity with
// Open3D is UNPINNED, and tests/plane_oracle.py is the CPU restatement the
// tests check against bit for bit.  All arithmetic is f64, uncontracted, in
// the order written here.
//
//   draw: iteration i samples point prim::draw(seed, ransac_n * i + k, n),
//     k = 0 .. ransac_n - 1.  Duplicates are not redrawn (deviation 1: Open3D
//     samples without replacement).
//   hypothesis, ransac_n == 3: e0 = p1 - p0, e1 = p2 - p0, n = e0 x e1 =
//     (e0y e1z - e0z e1y, e0z e1x - e0x e1z, e0x e1y - e0y e1x),
//     len = sqrt((nx^2 + ny^2) + nz^2); len == 0: invalid, skipped; else
//     n /= len, d = -((nx p0x + ny p0y) + nz p0z).  ransac_n in 4 .. 16: the
//     fit below over the samples in draw order, every sum 0.0 + v0 + v1 + ...
//   score: dist = |((a x + b y) + c z) + d|, inlier iff dist < threshold;
//     count = inliers, err = ordered sum of the inliers' dist, fitness =
//     count / n, rmse = err / sqrt(count) (0 for count 0).
//   walk: iteration i runs iff i < num_iterations and double(i) <= k (k starts
//     at num_iterations); a valid hypothesis replaces the best (initially
//     (0, 0)) iff count > best.count or (count == best.count and rmse <
//     best.rmse); then k = min(log(1 - probability) / log(1 - pow(fitness,
//     ransac_n)), num_iterations) for fitness < 1, else 0 (host, std::log /
//     std::pow).  k depends on the counts alone and a tie recomputes the same
//     k, so the hot pass computes counts only; err is computed once the walk
//     has stopped, for the hypotheses that tie the final best count -- the
//     winner is the earliest of them with the least rmse, which is what the
//     walk keeps.
//   result: the inliers of the best hypothesis in ascending index; plane_model
//     is the fit below over them.  No hypothesis ever best: plane (0, 0, 0, 0)
//     and no inliers (deviation 2).
//   fit (GetPlaneFromPoints): centroid = ordered sums of x, y, z / m; with r =
//     p - centroid the ordered sums xx xy xz yy yz zz; det_x = yy zz - yz yz,
//     det_y = xx zz - xz xz, det_z = xx yy - xy xy; the normal by the largest:
//     det_x > det_y && det_x > det_z: (det_x, xz yz - xy zz, xy yz - xz yy);
//     else det_y > det_z: (xz yz - xy zz, det_y, xy xz - yz xx); else
//     (xy yz - xz yy, xy xz - yz xx, det_z); len as above, len == 0: (0, 0, 0,
//     0); else n /= len, d = -((nx cx + ny cy) + nz cz).
//   ORDERED SUM (err, centroid, moments -- the one definition): over all n
//     points in index order, padded to a multiple of 4096, non-members
//     contributing +0.0.  In chunk c, lane l (0 .. 255) adds its 16 rows
//     v[4096 c + 256 r + l], r = 0 .. 15, to 0.0 left to right; then the tree
//     a[l] += a[l + s] for s = 128, 64, .., 1; the chunk sums a[0] are added
//     to 0.0 left to right.  One workgroup = one chunk, whatever the grid or
//     the hypothesis batch.

namespace {
namespace pln {

using prim::kChunk, prim::kRows, prim::tree_sum, prim::k_plane_fold_sum;  // the ordered sum's shared pieces
constexpr int kMaxH = 256;            // planes per scoring launch
constexpr int kMaxBatch = 4096;       // hypotheses per host round trip
constexpr int kMaxRn = 16;

// the fit's last step: plane from the centroid c[3] and the moments
// m = xx xy xz yy yz zz; false (and a zero plane) for a zero normal
__host__ __device__ inline bool plane_from_moments(const double* c, const double* m, double* pl) {
  const double xx = m[0], xy = m[1], xz = m[2], yy = m[3], yz = m[4], zz = m[5];
  const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
  double nx, ny, nz;
  if (det_x > det_y && det_x > det_z) {
    nx = det_x;
    ny = xz * yz - xy * zz;
    nz = xy * yz - xz * yy;
  } else if (det_y > det_z) {
    nx = xz * yz - xy * zz;
    ny = det_y;
    nz = xy * xz - yz * xx;
  } else {
    nx = xy * yz - xz * yy;
    ny = xy * xz - yz * xx;
    nz = det_z;
  }
  const double len = sqrt((nx * nx + ny * ny) + nz * nz);
  if (len == 0.0) {
    pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
    return false;
  }
  nx /= len;
  ny /= len;
  nz /= len;
  pl[0] = nx;
  pl[1] = ny;
  pl[2] = nz;
  pl[3] = -((nx * c[0] + ny * c[1]) + nz * c[2]);
  return true;
}

// One thread per hypothesis it0 + h of a batch: draw, fit -> planes[h][4], valid[h].
__global__ __launch_bounds__(kT) void k_plane_hyp(const double* __restrict__ xyz, int64_t n, uint64_t seed, int rn,
                                                  int64_t it0, int count, double* __restrict__ planes,
                                                  uint8_t* __restrict__ valid) {
  const int h = static_cast<int>(blockIdx.x) * kT + static_cast<int>(threadIdx.x);
  if (h >= count) return;
  const uint64_t base = static_cast<uint64_t>(rn) * static_cast<uint64_t>(it0 + h);
  const uint64_t un = static_cast<uint64_t>(n);
  double pl[4];
  bool ok;
  if (rn == 3) {
    const prim::D3 p0 = prim::ld3(xyz, prim::draw(seed, base, un));
    const prim::D3 p1 = prim::ld3(xyz, prim::draw(seed, base + 1, un));
    const prim::D3 p2 = prim::ld3(xyz, prim::draw(seed, base + 2, un));
    const double e0x = p1.x - p0.x, e0y = p1.y - p0.y, e0z = p1.z - p0.z;
    const double e1x = p2.x - p0.x, e1y = p2.y - p0.y, e1z = p2.z - p0.z;
    double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    ok = !(len == 0.0);
    if (ok) {
      nx /= len;
      ny /= len;
      nz /= len;
      pl[0] = nx;
      pl[1] = ny;
      pl[2] = nz;
      pl[3] = -((nx * p0.x + ny * p0.y) + nz * p0.z);
    } else {
      pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
    }
  } else {
    double c[3] = {0.0, 0.0, 0.0}, m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < rn; ++k) {
      const prim::D3 p = prim::ld3(xyz, prim::draw(seed, base + k, un));
      c[0] += p.x;
      c[1] += p.y;
      c[2] += p.z;
    }
    const double dm = static_cast<double>(rn);
    c[0] /= dm;
    c[1] /= dm;
    c[2] /= dm;
    for (int k = 0; k < rn; ++k) {
      const prim::D3 p = prim::ld3(xyz, prim::draw(seed, base + k, un));
      const double rx = p.x - c[0], ry = p.y - c[1], rz = p.z - c[2];
      m[0] += rx * rx;
      m[1] += rx * ry;
      m[2] += rx * rz;
      m[3] += ry * ry;
      m[4] += ry * rz;
      m[5] += rz * rz;
    }
    ok = plane_from_moments(c, m, pl);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) planes[4 * h + k] = pl[k];
  valid[h] = ok ? 1 : 0;
}

// The workgroup's chunk into registers: lane l's row r is point 4096 c + 256 r
// + l.  Every row goes through LDS so that the global loads are consecutive
// doubles (the cloud is [n][3]); points past n are NaN (never inliers).
__device__ __forceinline__ void load_chunk(const double* __restrict__ xyz, int64_t n, double* s_row,
                                           double (&x)[kRows], double (&y)[kRows], double (&z)[kRows]) {
  const int t = threadIdx.x;
  const int64_t e_end = 3 * n;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int64_t e0 = 3 * (static_cast<int64_t>(blockIdx.x) * kChunk + static_cast<int64_t>(r) * kT);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int64_t e = e0 + j * kT + t;
      s_row[j * kT + t] = e < e_end ? xyz[e] : NAN;
    }
    __syncthreads();
    x[r] = s_row[3 * t];
    y[r] = s_row[3 * t + 1];
    z[r] = s_row[3 * t + 2];
    __syncthreads();
  }
}

// The hot pass: one workgroup streams its chunk once and counts its inliers
// under each of the batch's H (<= kMaxH) planes -> part[h][chunk].  The plane
// is wave-uniform (scalar loads); a row's inliers are one ballot's popcount.
__global__ __launch_bounds__(kT) void k_plane_score(const double* __restrict__ xyz, int64_t n,
                                                    const double* __restrict__ planes, int H, double thr,
                                                    uint32_t* __restrict__ part, int64_t chunks) {
  __shared__ double s_row[3 * kT];
  __shared__ uint32_t s_c[kT / 64][kMaxH];
  double x[kRows], y[kRows], z[kRows];
  load_chunk(xyz, n, s_row, x, y, z);
  const int t = threadIdx.x, w = t >> 6;
  for (int h = 0; h < H; ++h) {
    const double a = planes[4 * h], b = planes[4 * h + 1], c = planes[4 * h + 2], d = planes[4 * h + 3];
    uint32_t cnt = 0u;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const double dist = fabs(((a * x[r] + b * y[r]) + c * z[r]) + d);
      cnt += static_cast<uint32_t>(__popcll(__ballot(dist < thr)));
    }
    if ((t & 63) == 0) s_c[w][h] = cnt;
  }
  __syncthreads();
  for (int h = t; h < H; h += kT) {
    uint32_t sum = 0u;
#pragma unroll
    for (int k = 0; k < kT / 64; ++k) sum += s_c[k][h];
    part[static_cast<int64_t>(h) * chunks + blockIdx.x] = sum;
  }
}

// counts of plane blockIdx.x over the chunks (integers: any order)
__global__ __launch_bounds__(kT) void k_plane_fold_cnt(const uint32_t* __restrict__ part, int64_t chunks,
                                                       int64_t* __restrict__ cnt) {
  __shared__ int64_t s[kT];
  const uint32_t* row = part + static_cast<int64_t>(blockIdx.x) * chunks;
  int64_t sum = 0;
  for (int64_t c = threadIdx.x; c < chunks; c += kT) sum += row[c];
  s[threadIdx.x] = sum;
  __syncthreads();
  for (int w = kT / 2; w > 0; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[blockIdx.x] = s[0];
}

// err of T (<= kMaxH) planes: the chunk's ordered partial of the inliers'
// dist -> part[h][chunk] (run only for the hypotheses that tie the best count).
__global__ __launch_bounds__(kT) void k_plane_err(const double* __restrict__ xyz, int64_t n,
                                                  const double* __restrict__ planes, int T, double thr,
                                                  double* __restrict__ part, int64_t chunks) {
  __shared__ double s_row[3 * kT];
  __shared__ double s[kT];
  double x[kRows], y[kRows], z[kRows];
  load_chunk(xyz, n, s_row, x, y, z);
  for (int h = 0; h < T; ++h) {
    const double a = planes[4 * h], b = planes[4 * h + 1], c = planes[4 * h + 2], d = planes[4 * h + 3];
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const double dist = fabs(((a * x[r] + b * y[r]) + c * z[r]) + d);
      acc = acc + (dist < thr ? dist : 0.0);
    }
    tree_sum(s, acc);
    if (threadIdx.x == 0) part[static_cast<int64_t>(h) * chunks + blockIdx.x] = s[0];
    __syncthreads();
  }
}

// inlier flags under the best plane, and their complement
__global__ __launch_bounds__(kT) void k_plane_flags(const double* __restrict__ xyz, int64_t n, double a, double b,
                                                    double c, double d, double thr, uint32_t* __restrict__ flag,
                                                    uint32_t* __restrict__ nflag) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= n) return;
  const double dist = fabs(((a * xyz[3 * i] + b * xyz[3 * i + 1]) + c * xyz[3 * i + 2]) + d);
  const uint32_t f = dist < thr ? 1u : 0u;
  flag[i] = f;
  if (nflag) nflag[i] = 1u - f;
}

// The fit's ordered sums over the flagged points, per chunk -> part[k][chunk]:
// MOM == 0: x, y, z (3 rows); MOM == 1: xx xy xz yy yz zz of p - (cx, cy, cz).
template <int MOM>
__global__ __launch_bounds__(kT) void k_plane_sums(const double* __restrict__ xyz, const uint32_t* __restrict__ flag,
                                                   int64_t n, double cx, double cy, double cz,
                                                   double* __restrict__ part, int64_t chunks) {
  constexpr int K = MOM ? 6 : 3;
  __shared__ double s[kT];
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kChunk + threadIdx.x;
#pragma unroll 4
  for (int r = 0; r < kRows; ++r) {
    const int64_t i = base + static_cast<int64_t>(r) * kT;
    const bool in = i < n && flag[i] != 0u;
    double v[K];
    if (in) {
      const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
      if (MOM) {
        const double rx = px - cx, ry = py - cy, rz = pz - cz;
        v[0] = rx * rx;
        v[1] = rx * ry;
        v[2] = rx * rz;
        v[K - 3] = ry * ry;
        v[K - 2] = ry * rz;
        v[K - 1] = rz * rz;
      } else {
        v[0] = px;
        v[1] = py;
        v[2] = pz;
      }
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = acc[k] + v[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    tree_sum(s, acc[k]);
    if (threadIdx.x == 0) part[static_cast<int64_t>(k) * chunks + blockIdx.x] = s[0];
    __syncthreads();
  }
}

// select_by_index(invert = true): flag = 1 everywhere, then 0 at every listed index
__global__ __launch_bounds__(kT) void k_fill_ones(uint32_t* __restrict__ flag, int64_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < n) flag[i] = 1u;
}

__global__ __launch_bounds__(kT) void k_unmark(const int64_t* __restrict__ index, int64_t m, int64_t n,
                                               uint32_t* __restrict__ flag) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (j >= m) return;
  const int64_t i = index[j];
  if (i >= 0 && i < n) flag[i] = 0u;  // (an index out of range is the caller's IndexError; never a store)
}

// hypotheses per host round trip when the caller leaves the choice (batch 0):
// the fastest of the sweep 16 .. 1000 at 4K (scripts/background_bench.py); a
// schedule growing 32, 64, 128, 256 measured within run-to-run spread of it
constexpr int kDefaultBatch = 64;

}  // namespace pln
}  // namespace

extern "C" {

int sl_segment_plane(sl_ctx* c, const double* xyz, int64_t n, double distance_threshold, int ransac_n,
                     int num_iterations, double probability, uint64_t seed, int batch, double* plane_model,
                     int64_t* inlier_index, int64_t* n_inliers, int64_t* rest_index, int* iterations, void* stream) {
  using namespace pln;
  if (!c) return SL_EINVAL;
  if (ransac_n < 3 || ransac_n > kMaxRn) return slgpu_fail(c, SL_EINVAL, "sl_segment_plane: ransac_n must be 3..16");
  if (n < ransac_n) return slgpu_fail(c, SL_EINVAL, "sl_segment_plane: fewer points than ransac_n");
  if (n >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  if (num_iterations < 0) return slgpu_fail(c, SL_EINVAL, "sl_segment_plane: num_iterations < 0");
  if (!(probability > 0.0 && probability < 1.0))
    return slgpu_fail(c, SL_EINVAL, "sl_segment_plane: probability must be inside (0, 1)");
  if (batch < 0 || !xyz || !plane_model || !inlier_index || !n_inliers)
    return slgpu_fail(c, SL_EINVAL, "sl_segment_plane: bad batch or NULL arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  const int64_t chunks = (n + kChunk - 1) / kChunk;
  const int cap = std::max(kMaxH, std::min(batch > 0 ? batch : kMaxH, kMaxBatch));
  DBuf<double> planes, dpart, dsum;
  DBuf<uint8_t> valid;
  DBuf<uint32_t> cpart, flag, nflag, pos;
  DBuf<int64_t> cnt;
  MTRY(c, planes.alloc(4 * cap));
  MTRY(c, valid.alloc(cap));
  MTRY(c, cpart.alloc(cap * chunks));
  MTRY(c, cnt.alloc(cap));
  std::vector<double> hplanes(4 * static_cast<size_t>(cap));
  std::vector<uint8_t> hvalid(static_cast<size_t>(cap));
  std::vector<int64_t> hcnt(static_cast<size_t>(cap));

  // the walk, on counts (see the header: k and the final best count need no err)
  const double dn = static_cast<double>(n), log_p = std::log(1.0 - probability);
  double k = static_cast<double>(num_iterations);
  int64_t it = 0, best_cnt = 0;
  std::vector<double> ties;  // planes of the hypotheses at best_cnt, in iteration order
  while (it < num_iterations && static_cast<double>(it) <= k) {
    int64_t H = std::min<int64_t>(std::min(batch > 0 ? batch : kDefaultBatch, kMaxBatch), num_iterations - it);
    H = std::min<int64_t>(H, static_cast<int64_t>(std::floor(k)) + 1 - it);  // none past k
    hipLaunchKernelGGL(k_plane_hyp, dim3(blocks(H)), dim3(kT), 0, s, xyz, n, seed, ransac_n, it, static_cast<int>(H),
                       planes.p, valid.p);
    for (int64_t g = 0; g < H; g += kMaxH)
      hipLaunchKernelGGL(k_plane_score, dim3(static_cast<unsigned>(chunks)), dim3(kT), 0, s, xyz, n, planes.p + 4 * g,
                         static_cast<int>(std::min<int64_t>(kMaxH, H - g)), distance_threshold, cpart.p + g * chunks,
                         chunks);
    hipLaunchKernelGGL(k_plane_fold_cnt, dim3(static_cast<unsigned>(H)), dim3(kT), 0, s, cpart.p, chunks, cnt.p);
    MTRY(c, hipGetLastError());
    MTRY(c, hipMemcpyAsync(hplanes.data(), planes.p, sizeof(double) * 4 * H, hipMemcpyDeviceToHost, s));
    MTRY(c, hipMemcpyAsync(hvalid.data(), valid.p, H, hipMemcpyDeviceToHost, s));
    MTRY(c, hipMemcpyAsync(hcnt.data(), cnt.p, sizeof(int64_t) * H, hipMemcpyDeviceToHost, s));
    MTRY(c, hipStreamSynchronize(s));
    int64_t x = 0;
    for (; x < H && static_cast<double>(it + x) <= k; ++x) {
      if (!hvalid[x]) continue;
      const int64_t cx = hcnt[x];
      if (cx > best_cnt) {
        best_cnt = cx;
        ties.clear();
        const double fitness = static_cast<double>(cx) / dn;
        k = fitness < 1.0 ? std::min(log_p / std::log(1.0 - std::pow(fitness, static_cast<double>(ransac_n))),
                                     static_cast<double>(num_iterations))
                          : 0.0;
      }
      if (cx == best_cnt && cx > 0) ties.insert(ties.end(), hplanes.begin() + 4 * x, hplanes.begin() + 4 * x + 4);
    }
    it += x;
    if (x < H) break;
  }
  if (iterations) *iterations = static_cast<int>(it);

  // the best among the ties: the earliest with the least rmse
  double best[4] = {0.0, 0.0, 0.0, 0.0};
  const int64_t nt = static_cast<int64_t>(ties.size() / 4);
  if (nt == 1) {
    memcpy(best, ties.data(), sizeof(best));
  } else if (nt > 1) {
    MTRY(c, dpart.alloc(kMaxH * chunks));
    MTRY(c, dsum.alloc(kMaxH));
    std::vector<double> herr(kMaxH);
    const double root = std::sqrt(static_cast<double>(best_cnt));
    double best_rmse = 0.0;
    for (int64_t g = 0; g < nt; g += kMaxH) {
      const int T = static_cast<int>(std::min<int64_t>(kMaxH, nt - g));
      MTRY(c, hipMemcpyAsync(planes.p, ties.data() + 4 * g, sizeof(double) * 4 * T, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_plane_err, dim3(static_cast<unsigned>(chunks)), dim3(kT), 0, s, xyz, n, planes.p, T,
                         distance_threshold, dpart.p, chunks);
      hipLaunchKernelGGL(k_plane_fold_sum, dim3(T), dim3(kT), 0, s, dpart.p, chunks, dsum.p);
      MTRY(c, hipGetLastError());
      MTRY(c, hipMemcpyAsync(herr.data(), dsum.p, sizeof(double) * T, hipMemcpyDeviceToHost, s));
      MTRY(c, hipStreamSynchronize(s));  // (also: ties' planes are read by the copy above until here)
      for (int j = 0; j < T; ++j) {
        const double rmse = herr[j] / root;
        if ((g == 0 && j == 0) || rmse < best_rmse) {
          best_rmse = rmse;
          memcpy(best, ties.data() + 4 * (g + j), sizeof(best));
        }
      }
    }
  }

  // inliers (and the rest) in ascending index; no best: a threshold nothing is below
  MTRY(c, flag.alloc(n));
  MTRY(c, pos.alloc(n));
  if (rest_index) MTRY(c, nflag.alloc(n));
  hipLaunchKernelGGL(k_plane_flags, dim3(blocks(n)), dim3(kT), 0, s, xyz, n, best[0], best[1], best[2], best[3],
                     nt ? distance_threshold : -1.0, flag.p, nflag.p);
  MTRY(c, hipGetLastError());
  int64_t m = 0;
  int r = compact_indices(c, flag.p, n, pos.p, inlier_index, &m, s);
  if (r) return r;
  if (nt && m != best_cnt) return slgpu_fail(c, SL_EHIP, "sl_segment_plane: inlier count changed between passes");
  *n_inliers = m;

  // plane_model: the fit over the inliers
  plane_model[0] = plane_model[1] = plane_model[2] = plane_model[3] = 0.0;
  if (m > 0) {
    if (!dpart.p) MTRY(c, dpart.alloc(kMaxH * chunks));
    if (!dsum.p) MTRY(c, dsum.alloc(kMaxH));
    double cen[3], mom[6];
    hipLaunchKernelGGL(k_plane_sums<0>, dim3(static_cast<unsigned>(chunks)), dim3(kT), 0, s, xyz, flag.p, n, 0.0, 0.0,
                       0.0, dpart.p, chunks);
    hipLaunchKernelGGL(k_plane_fold_sum, dim3(3), dim3(kT), 0, s, dpart.p, chunks, dsum.p);
    MTRY(c, hipGetLastError());
    MTRY(c, hipMemcpyAsync(cen, dsum.p, sizeof(cen), hipMemcpyDeviceToHost, s));
    MTRY(c, hipStreamSynchronize(s));
    for (int a = 0; a < 3; ++a) cen[a] /= static_cast<double>(m);
    hipLaunchKernelGGL(k_plane_sums<1>, dim3(static_cast<unsigned>(chunks)), dim3(kT), 0, s, xyz, flag.p, n, cen[0],
                       cen[1], cen[2], dpart.p, chunks);
    hipLaunchKernelGGL(k_plane_fold_sum, dim3(6), dim3(kT), 0, s, dpart.p, chunks, dsum.p);
    MTRY(c, hipGetLastError());
    MTRY(c, hipMemcpyAsync(mom, dsum.p, sizeof(mom), hipMemcpyDeviceToHost, s));
    MTRY(c, hipStreamSynchronize(s));
    plane_from_moments(cen, mom, plane_model);
  }
  if (rest_index) {
    int64_t rest = 0;
    if ((r = compact_indices(c, nflag.p, n, pos.p, rest_index, &rest, s))) return r;
  }
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_index_complement(sl_ctx* c, const int64_t* index, int64_t m, int64_t n, int64_t* out_index, int64_t* out_n,
                        void* stream) {
  using namespace pln;
  if (!c) return SL_EINVAL;
  if (m < 0 || n < 0 || n >= (1ll << 31) || (m && !index) || !out_n || (n && !out_index))
    return slgpu_fail(c, SL_EINVAL, "sl_index_complement: bad sizes or NULL arguments");
  *out_n = 0;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  DBuf<uint32_t> flag, pos;
  MTRY(c, flag.alloc(n));
  MTRY(c, pos.alloc(n));
  hipLaunchKernelGGL(k_fill_ones, dim3(blocks(n)), dim3(kT), 0, s, flag.p, n);
  if (m) hipLaunchKernelGGL(k_unmark, dim3(blocks(m)), dim3(kT), 0, s, index, m, n, flag.p);
  MTRY(c, hipGetLastError());
  const int r = compact_indices(c, flag.p, n, pos.p, out_index, out_n, s);
  if (r) return r;
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

}  // extern "C"
