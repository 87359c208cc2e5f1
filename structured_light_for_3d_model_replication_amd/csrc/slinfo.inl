// Information matrix of a registered pair of clouds for the pose graph of the
// loop-closing 360 merge (Old/new360Merge.py:90-92): Open3D's
// GetInformationMatrixFromPointClouds restated (parity with Open3D is unpinned:
// not in this image; tests/posegraph_oracle.py is the CPU restatement, bit for
// bit).  Every source point is moved by `transformation` (k_transform's order;
// an exactly-identity matrix moves nothing), its correspondence is grid_nn's
// (the nearest target with d^2 < max_distance^2, lowest index on ties), and a
// correspondence with the target point (x, y, z) adds G^T G,
//   r1 = (0, z, -y, 1, 0, 0)   r2 = (-z, 0, x, 0, 1, 0)   r3 = (y, -x, 0, 0, 0, 1),
// entry (a, c) as (r1[a] r1[c] + r2[a] r2[c]) + r3[a] r3[c].  Summation order
// (the ICP's): source points in blocks of kIcpBlock consecutive indices, a left
// fold inside each block that skips unmatched points, the blocks' partial sums
// folded left to right on the host.
//
// Kernel shape.  The views are full-resolution clouds, so one thread per
// 64-point block (k_icp_fold's shape) would run n / 64 threads.  Here one
// wave64 owns one block: each lane moves its point, searches the grid and
// leaves the matched target's coordinates (or "none") in LDS; then lanes 0..20
// each fold one of the 21 upper-triangle entries over the 64 slots in index
// order -- every lane reads the same slot, an LDS broadcast -- and store one
// row of 21 doubles.  No moved copy of the cloud and no corr / dist2 arrays go
// through device memory.  A lane picks its entry's six factors from {0, 1, +-x,
// +-y, +-z} by selects on codes it decodes once, so the fold does not diverge.
namespace {
namespace info {

constexpr int kEntries = 21;  // upper triangle of the 6x6 matrix, row-major

struct Pose {  // the top three rows of the 4x4, row-major (a kernel argument)
  double m[12];
};

// factor codes: 0: 0, 1: 1, 2: x, 3: -x, 4: y, 5: -y, 6: z, 7: -z
__device__ __forceinline__ double factor(int code, double x, double y, double z) {
  const double v = code < 2 ? static_cast<double>(code) : (code < 4 ? x : (code < 6 ? y : z));
  return (code & 1) && code > 1 ? -v : v;
}

// row j of G, column a, as a factor code
__device__ __forceinline__ int g_code(int j, int a) {
  // r1 = (0, z, -y, 1, 0, 0), r2 = (-z, 0, x, 0, 1, 0), r3 = (y, -x, 0, 0, 0, 1): three bits per entry
  constexpr uint32_t rows[3] = {0u | 6u << 3 | 5u << 6 | 1u << 9, 7u | 2u << 6 | 1u << 12, 4u | 3u << 3 | 1u << 15};
  const uint32_t r = j == 0 ? rows[0] : (j == 1 ? rows[1] : rows[2]);
  return static_cast<int>((r >> (3 * a)) & 7u);
}

// *flag = 1 when one of the n values is not finite.  build_search_grid's bounds
// (fmin / fmax) see an infinity and skip a NaN, so the target is checked here
// before any of its points is keyed into a cell.
__global__ __launch_bounds__(kT) void k_info_nonfinite(const double* v, int64_t n, unsigned* flag) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * kT)
    if (!isfinite(v[i])) *flag = 1;
}

// One wave per kIcpBlock source points (kT / 64 blocks per workgroup) ->
// part[block][21].  The grid is ceil(n / kT) workgroups, so every wave whose
// block starts below n has a row of part.
__global__ __launch_bounds__(kT) void k_info_fold(const double* src, int64_t n, Pose P, int moved, const double* tgt,
                                                  SearchGrid tg, double r2, double* part) {
  static_assert(kIcpBlock == 64, "one wave64 per block of source points");
  __shared__ double sx[kT], sy[kT], sz[kT];
  __shared__ int32_t sok[kT];
  const int tid = threadIdx.x;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + tid;
  double x = 0.0, y = 0.0, z = 0.0;
  int32_t ok = 0;
  if (i < n) {
    double q0 = src[3 * i], q1 = src[3 * i + 1], q2 = src[3 * i + 2];
    if (moved) {
      const double a = q0, b = q1, c = q2;
      q0 = ((P.m[0] * a + P.m[1] * b) + P.m[2] * c) + P.m[3];
      q1 = ((P.m[4] * a + P.m[5] * b) + P.m[6] * c) + P.m[7];
      q2 = ((P.m[8] * a + P.m[9] * b) + P.m[10] * c) + P.m[11];
    }
    double d2;
    const int64_t j = grid_nn(q0, q1, q2, tg, r2, &d2);
    if (j >= 0) {
      ok = 1;
      x = tgt[3 * j];
      y = tgt[3 * j + 1];
      z = tgt[3 * j + 2];
    }
  }
  sx[tid] = x;
  sy[tid] = y;
  sz[tid] = z;
  sok[tid] = ok;
  __syncthreads();
  const int lane = tid & 63, base = tid & ~63;
  const int64_t b = (static_cast<int64_t>(blockIdx.x) * kT + base) / kIcpBlock;
  if (lane >= kEntries || b * kIcpBlock >= n) return;
  int a = 0, rest = lane;  // entry `lane` of the upper triangle -> (a, c)
  while (rest >= 6 - a) {
    rest -= 6 - a;
    ++a;
  }
  const int c = a + rest;
  const int a1 = g_code(0, a), c1 = g_code(0, c), a2 = g_code(1, a), c2 = g_code(1, c), a3 = g_code(2, a),
            c3 = g_code(2, c);
  double acc = 0.0;
  for (int k = 0; k < kIcpBlock; ++k) {
    if (!sok[base + k]) continue;  // (the same for every lane of the wave)
    const double px = sx[base + k], py = sy[base + k], pz = sz[base + k];
    acc += (factor(a1, px, py, pz) * factor(c1, px, py, pz) + factor(a2, px, py, pz) * factor(c2, px, py, pz)) +
           factor(a3, px, py, pz) * factor(c3, px, py, pz);
  }
  part[kEntries * b + lane] = acc;
}

}  // namespace info
}  // namespace

extern "C" int sl_information_matrix(sl_ctx* c, const double* source, int64_t n_src, const double* target,
                                     int64_t n_tgt, double max_distance, const double* transformation,
                                     double* information, int64_t* correspondences, void* stream) {
  using namespace info;
  if (!c) return SL_EINVAL;
  if (n_src < 0 || n_tgt < 0 || !transformation || !information || (n_src && !source) || (n_tgt && !target))
    return slgpu_fail(c, SL_EINVAL, "sl_information_matrix: bad sizes or NULL arguments");
  if (n_src >= (1ll << 31) || n_tgt >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  if (!(max_distance > 0.0)) return slgpu_fail(c, SL_EINVAL, "max_correspondence_distance must be > 0");
  for (int k = 0; k < 36; ++k) information[k] = 0.0;
  if (correspondences) *correspondences = 0;
  if (n_src == 0 || n_tgt == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = prim::require_clear(c, SL_EINVAL, "non-finite target coordinates", s, [&](unsigned* bad) {
    const unsigned g = static_cast<unsigned>(std::min<int64_t>(2048, (3 * n_tgt + kT - 1) / kT));
    hipLaunchKernelGGL(k_info_nonfinite, dim3(g), dim3(kT), 0, s, target, 3 * n_tgt, bad);
  });
  if (r) return r;
  SearchGridBufs tg;
  r = build_search_grid(c, target, n_tgt, max_distance, GridTable::kDense, "non-finite target coordinates",
                                  &tg, s);
  if (r) return r;
  const int64_t nb = (n_src + kIcpBlock - 1) / kIcpBlock;
  DBuf<double> part;
  MTRY(c, part.alloc(kEntries * nb));
  Pose P;
  memcpy(P.m, transformation, sizeof(P.m));
  bool ident = true;
  for (int i = 0; i < 16; ++i) ident = ident && transformation[i] == ((i % 5 == 0) ? 1.0 : 0.0);
  hipLaunchKernelGGL(k_info_fold, dim3(blocks(n_src)), dim3(kT), 0, s, source, n_src, P, ident ? 0 : 1, target,
                     tg.view, max_distance * max_distance, part.p);
  MTRY(c, hipGetLastError());
  std::vector<double> hpart(static_cast<size_t>(kEntries * nb));
  MTRY(c, hipMemcpyAsync(hpart.data(), part.p, sizeof(double) * hpart.size(), hipMemcpyDeviceToHost, s));
  MTRY(c, hipStreamSynchronize(s));
  double sums[kEntries];
  for (int k = 0; k < kEntries; ++k) sums[k] = 0.0;
  for (int64_t b = 0; b < nb; ++b)
    for (int k = 0; k < kEntries; ++k) sums[k] = sums[k] + hpart[static_cast<size_t>(kEntries * b + k)];
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int cc = a; cc < 6; ++cc, ++k) information[6 * a + cc] = information[6 * cc + a] = sums[k];
  if (correspondences) *correspondences = static_cast<int64_t>(information[21]);  // entry (3, 3): 1 per correspondence
  return SL_OK;
}
