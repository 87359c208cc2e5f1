// libslgpu.so, part 2d -- Poisson meshing, the fourth step of the reference's
// workflow (server/processing.py:185-311: create_from_point_cloud_poisson,
// remove_vertices_by_mask, write_triangle_mesh), included at the end of
// slmerge.hip (one translation unit: it shares that file's scan and row
// compaction and scratch pool, and slprim.inl's pieces of the ordered sum that
// slplane.inl's header defines).  Open3D's Poisson is the
// adaptive-octree variant and is not in this image; this is Kazhdan's FFT
// Poisson reconstruction on a dense periodic grid, parity with Open3D is
// UNPINNED, and tests/mesh_oracle.py is the CPU restatement the tests check
// against: bit for bit for every stage but the FFT solve.  f64 and f32
// arithmetic is uncontracted, in the order written here.
//
//   box (host f64): lo, hi of the points; c = (lo + hi) / 2; L = scale *
//     max(hi - lo) (L = 1 when that is not > 0); R = 2^depth; h = L / R; o = c -
//     L / 2.  Node (i, j, k) sits at o + h (i, j, k); its linear index is (i R +
//     j) R + k.  The grid is periodic: every node index is taken & (R - 1).
//   cell of a point p: g = (p - o) / h, i0 = floor(g), f = g - i0.  Corner c
//     (0 .. 7) is node i0 + (c & 1, c >> 1 & 1, c >> 2 & 1) with weight w_c =
//     (wx wy) wz, w_a = f_a where the corner's offset is 1, else 1 - f_a.
//   splat: 64-bit FIXED-POINT INTEGER ATOMIC ADDS (so the sums do not depend on
//     the order the points arrive in): fix(v) = llrint(v 2^30) (ties to even)
//     for |v 2^30| < 2^62, else 0; every corner adds fix(w_c) to its node's
//     weight sum and fix(w_c n_a) to its three vector sums (wrapping 64-bit).
//     Then W, V_a = float(double(sum) 2^-30).
//   divergence (f32): s = ((V_x[i+1] - V_x[i-1]) + (V_y[j+1] - V_y[j-1])) +
//     (V_z[k+1] - V_z[k-1]); div = float(double(s) / (2 h)).
//   solve (f32, torch.fft / rocFFT; tolerance, not bits): chi^ = rfftn(div) /
//     lambda, lambda = ((c_i + c_j) + c_k) / float(h h), c_k = float(2 cos(2 pi
//     k / R) - 2); chi^(0) = 0; chi = irfftn(chi^).
//   sample (trilinear, f64): 0.0 + w_0 double(G[corner 0]) + .. + w_7
//     double(G[corner 7]), left to right.  iso = ORDERED SUM (slplane.inl) of
//     the points' chi samples / n.  The density of a vertex is the sample of W
//     at its position.  get_center = the ordered sums of x, y, z / n.
//   extraction: marching tetrahedra over all R^3 cubes; cube (i, j, k) has the
//     corners c = 0 .. 7 at node (i, j, k) + offsets(c), wrapped.  v = double(chi)
//     - iso; a node is inside iff v < 0.  The six Kuhn tetrahedra of a cube are
//     the axis permutations in lexicographic order, tetrahedron (a1, a2, a3) =
//     corners (0, bit a1, bit a1 | bit a2, 7):
//       t0 (x,y,z) 0 1 3 7   t1 (x,z,y) 0 1 5 7   t2 (y,x,z) 0 2 3 7
//       t3 (y,z,x) 0 2 6 7   t4 (z,x,y) 0 4 5 7   t5 (z,y,x) 0 4 6 7
//     t0, t3, t4 are positively oriented.  Every tetrahedron edge joins a cube
//     corner ca to a corner cb that contains it; it is OWNED by the node of ca,
//     with direction d = cb - ca (1 .. 7, the offset bits).  A crossed edge
//     (inside(a) != inside(b), a the owner) carries one vertex x = p_a + (p_b -
//     p_a) (v_a / (v_a - v_b)), p_a = o + h (i, j, k), p_b = o + h ((i, j, k) +
//     offsets(d)) -- positions do not wrap, node R lies at o + h R.  Vertices
//     are numbered ascending by (owner node, d).
//     Triangles, by the mask m of a tetrahedron's inside corners (bit q: its
//     q-th corner), over its edges e0 .. e5 = 01 02 03 12 13 23:
//       1: 0 1 2     2: 0 4 3     3: 1 2 4, 1 4 3   4: 1 3 5     5: 2 0 3, 2 3 5
//       6: 0 4 5, 0 5 1           7: 2 4 5          8: 2 5 4     9: 0 1 5, 0 5 4
//       10: 3 0 2, 3 2 5          11: 1 5 3         12: 1 3 4, 1 4 2
//       13: 0 3 4    14: 0 2 1    (0, 15: none)
//     as listed for t0, t3, t4 and with the last two vertices swapped for t1,
//     t2, t5: the geometric normal points to the outside (v >= 0) corners.
//     Triangles are ordered by (cube, tetrahedron, position in the row).
//   trim: remove_vertices_by_mask drops the masked vertices and every triangle
//     that has one; survivors keep their order and are re-indexed.

namespace {
namespace msh {

constexpr double kFix = 1073741824.0;                 // 2^30
constexpr double kFixMax = 4611686018427387904.0;     // 2^62

__constant__ int8_t kTetCorner[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7},
                                        {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ int8_t kEdgeA[6] = {0, 0, 0, 1, 1, 2};
__constant__ int8_t kEdgeB[6] = {1, 2, 3, 2, 3, 3};
// row m: triangle count, then its edges
__constant__ int8_t kCase[16][7] = {{0, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 2, 0, 0, 0}, {1, 0, 4, 3, 0, 0, 0},
                                    {2, 1, 2, 4, 1, 4, 3}, {1, 1, 3, 5, 0, 0, 0}, {2, 2, 0, 3, 2, 3, 5},
                                    {2, 0, 4, 5, 0, 5, 1}, {1, 2, 4, 5, 0, 0, 0}, {1, 2, 5, 4, 0, 0, 0},
                                    {2, 0, 1, 5, 0, 5, 4}, {2, 3, 0, 2, 3, 2, 5}, {1, 1, 5, 3, 0, 0, 0},
                                    {2, 1, 3, 4, 1, 4, 2}, {1, 0, 3, 4, 0, 0, 0}, {1, 0, 2, 1, 0, 0, 0},
                                    {0, 0, 0, 0, 0, 0, 0}};

struct Box {
  double o[3];
  double h;
  int bits;  // depth: R = 1 << bits
};

__device__ __forceinline__ int64_t fix(double v) {
  const double t = v * kFix;
  return fabs(t) < kFixMax ? llrint(t) : 0;
}

// The cell of p: the wrapped linear node index and the weight of each corner.
// Indices are masked, so any p (NaN, far outside) still addresses the grid.
__device__ __forceinline__ void corners(const Box& b, double px, double py, double pz, int64_t* lin, double* w) {
  const double p[3] = {px, py, pz};
  uint64_t i0[3];
  double f[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double g = (p[a] - b.o[a]) / b.h;
    const double fl = floor(g);
    f[a] = g - fl;
    i0[a] = fabs(fl) < 9.0e18 ? static_cast<uint64_t>(static_cast<int64_t>(fl)) : 0ull;
  }
  const uint64_t mask = (1ull << b.bits) - 1ull;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint64_t i = (i0[0] + (c & 1)) & mask, j = (i0[1] + ((c >> 1) & 1)) & mask,
                   k = (i0[2] + ((c >> 2) & 1)) & mask;
    lin[c] = static_cast<int64_t>((((i << b.bits) | j) << b.bits) | k);
    const double wx = (c & 1) ? f[0] : 1.0 - f[0];
    const double wy = (c & 2) ? f[1] : 1.0 - f[1];
    const double wz = (c & 4) ? f[2] : 1.0 - f[2];
    w[c] = (wx * wy) * wz;
  }
}

__global__ __launch_bounds__(kT) void k_mesh_splat(const double* __restrict__ xyz, const double* __restrict__ nrm,
                                                   int64_t n, Box b, unsigned long long* __restrict__ acc) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (p >= n) return;
  int64_t lin[8];
  double w[8];
  corners(b, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2], lin, w);
  const double nx = nrm[3 * p], ny = nrm[3 * p + 1], nz = nrm[3 * p + 2];
  const int64_t n3 = int64_t{1} << (3 * b.bits);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    atomicAdd(acc + lin[c], static_cast<unsigned long long>(fix(w[c])));
    atomicAdd(acc + n3 + lin[c], static_cast<unsigned long long>(fix(w[c] * nx)));
    atomicAdd(acc + 2 * n3 + lin[c], static_cast<unsigned long long>(fix(w[c] * ny)));
    atomicAdd(acc + 3 * n3 + lin[c], static_cast<unsigned long long>(fix(w[c] * nz)));
  }
}

__global__ __launch_bounds__(kT) void k_mesh_unfix(const int64_t* __restrict__ acc, int64_t count,
                                                   float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < count) out[i] = static_cast<float>(static_cast<double>(acc[i]) * (1.0 / kFix));
}

__global__ __launch_bounds__(kT) void k_mesh_div(const float* __restrict__ V, int bits, double two_h,
                                                 float* __restrict__ div) {
  const int64_t n3 = int64_t{1} << (3 * bits), m = (int64_t{1} << bits) - 1;
  const int64_t lin = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (lin >= n3) return;
  const int64_t k = lin & m, j = (lin >> bits) & m, i = lin >> (2 * bits);
  auto at = [&](int64_t ii, int64_t jj, int64_t kk) { return ((((ii & m) << bits) | (jj & m)) << bits) | (kk & m); };
  const float dx = V[at(i + 1, j, k)] - V[at(i - 1, j, k)];
  const float dy = V[n3 + at(i, j + 1, k)] - V[n3 + at(i, j - 1, k)];
  const float dz = V[2 * n3 + at(i, j, k + 1)] - V[2 * n3 + at(i, j, k - 1)];
  const float s = (dx + dy) + dz;
  div[lin] = static_cast<float>(static_cast<double>(s) / two_h);
}

__global__ __launch_bounds__(kT) void k_mesh_sample(const float* __restrict__ G, Box b,
                                                    const double* __restrict__ xyz, int64_t n,
                                                    double* __restrict__ out) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (p >= n) return;
  int64_t lin[8];
  double w[8];
  corners(b, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2], lin, w);
  double acc = 0.0;
#pragma unroll
  for (int c = 0; c < 8; ++c) acc = acc + w[c] * static_cast<double>(G[lin[c]]);
  out[p] = acc;
}

// The ordered sum's chunk partials of v[stride i + offset], i < n -> part[chunk].
__global__ __launch_bounds__(kT) void k_osum_part(const double* __restrict__ v, int64_t n, int64_t stride,
                                                  int64_t offset, double* __restrict__ part) {
  __shared__ double s[kT];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * prim::kChunk + threadIdx.x;
  double acc = 0.0;
#pragma unroll 4
  for (int r = 0; r < prim::kRows; ++r) {
    const int64_t i = base + static_cast<int64_t>(r) * kT;
    acc = acc + (i < n ? v[stride * i + offset] : 0.0);
  }
  prim::tree_sum(s, acc);
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(kT) void k_orient(const double* __restrict__ xyz, double* __restrict__ nrm, int64_t n,
                                               double lx, double ly, double lz) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (p >= n) return;
  const double dx = lx - xyz[3 * p], dy = ly - xyz[3 * p + 1], dz = lz - xyz[3 * p + 2];
  double nx = nrm[3 * p], ny = nrm[3 * p + 1], nz = nrm[3 * p + 2];
  if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
    const double len = sqrt((dx * dx + dy * dy) + dz * dz);
    if (len == 0.0) {
      nx = 0.0, ny = 0.0, nz = 1.0;
    } else {
      nx = dx / len, ny = dy / len, nz = dz / len;
    }
  } else if ((nx * dx + ny * dy) + nz * dz < 0.0) {
    nx = -nx, ny = -ny, nz = -nz;
  } else {
    return;
  }
  nrm[3 * p] = nx;
  nrm[3 * p + 1] = ny;
  nrm[3 * p + 2] = nz;
}

__device__ __forceinline__ int64_t node_at(int64_t i, int64_t j, int64_t k, int c, int bits) {
  const int64_t m = (int64_t{1} << bits) - 1;
  return ((((i + (c & 1)) & m) << bits | ((j + ((c >> 1) & 1)) & m)) << bits) | ((k + ((c >> 2) & 1)) & m);
}

// bit c: corner c of cube `lin` is inside
__device__ __forceinline__ uint32_t cube_inside(const float* __restrict__ chi, double iso, int64_t lin, int bits) {
  const int64_t m = (int64_t{1} << bits) - 1;
  const int64_t k = lin & m, j = (lin >> bits) & m, i = lin >> (2 * bits);
  uint32_t in = 0u;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    in |= (static_cast<double>(chi[node_at(i, j, k, c, bits)]) - iso < 0.0 ? 1u : 0u) << c;
  return in;
}

// Per node: the mask of its crossed owned edges (bit d - 1) and their count;
// per cube: its triangle count.  (A node's owned edges end at its cube's corners.)
__global__ __launch_bounds__(kT) void k_mesh_count(const float* __restrict__ chi, double iso, int bits,
                                                   uint8_t* __restrict__ emask, uint32_t* __restrict__ vcnt,
                                                   uint32_t* __restrict__ tcnt) {
  const int64_t n3 = int64_t{1} << (3 * bits);
  const int64_t lin = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (lin >= n3) return;
  const uint32_t in = cube_inside(chi, iso, lin, bits);
  const uint32_t cross = ((in & 1u) ? ~in : in) & 0xFEu;  // corners that differ from corner 0
  emask[lin] = static_cast<uint8_t>(cross >> 1);
  vcnt[lin] = static_cast<uint32_t>(__popc(cross));
  uint32_t t = 0u;
  if (in != 0u && in != 0xFFu) {
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      uint32_t m = 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) m |= ((in >> kTetCorner[q][r]) & 1u) << r;
      t += static_cast<uint32_t>(kCase[m][0]);
    }
  }
  tcnt[lin] = t;
}

__global__ __launch_bounds__(kT) void k_mesh_emit_v(const float* __restrict__ chi, double iso, Box b,
                                                    const uint8_t* __restrict__ emask,
                                                    const uint32_t* __restrict__ vpos, int64_t n_v,
                                                    double* __restrict__ verts) {
  const int bits = b.bits;
  const int64_t n3 = int64_t{1} << (3 * bits), m = (int64_t{1} << bits) - 1;
  const int64_t lin = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (lin >= n3) return;
  const uint32_t em = emask[lin];
  if (!em) return;
  const int64_t k = lin & m, j = (lin >> bits) & m, i = lin >> (2 * bits);
  const double va = static_cast<double>(chi[lin]) - iso;
  const int64_t idx[3] = {i, j, k};
  int64_t at = vpos[lin];
  for (int d = 1; d < 8; ++d) {
    if (!((em >> (d - 1)) & 1u)) continue;
    const double vb = static_cast<double>(chi[node_at(i, j, k, d, bits)]) - iso;
    const double t = va / (va - vb);
    if (at < n_v) {  // (always: the counts and this pass read the same field)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double pa = b.o[a] + b.h * static_cast<double>(idx[a]);
        const double pb = b.o[a] + b.h * static_cast<double>(idx[a] + ((d >> a) & 1));
        verts[3 * at + a] = pa + (pb - pa) * t;
      }
    }
    ++at;
  }
}

__global__ __launch_bounds__(kT) void k_mesh_emit_t(const float* __restrict__ chi, double iso, int bits,
                                                    const uint8_t* __restrict__ emask,
                                                    const uint32_t* __restrict__ vpos,
                                                    const uint32_t* __restrict__ tpos, int64_t n_t,
                                                    int32_t* __restrict__ tris) {
  const int64_t n3 = int64_t{1} << (3 * bits), mk = (int64_t{1} << bits) - 1;
  const int64_t lin = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (lin >= n3) return;
  const uint32_t in = cube_inside(chi, iso, lin, bits);
  if (in == 0u || in == 0xFFu) return;
  const int64_t k = lin & mk, j = (lin >> bits) & mk, i = lin >> (2 * bits);
  int64_t at = tpos[lin];
  for (int q = 0; q < 6; ++q) {
    uint32_t m = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) m |= ((in >> kTetCorner[q][r]) & 1u) << r;
    const int nt = kCase[m][0];
    const bool odd = q == 1 || q == 2 || q == 5;
    for (int x = 0; x < nt; ++x, ++at) {
      if (at >= n_t) return;  // (never: see k_mesh_emit_v)
      for (int s = 0; s < 3; ++s) {
        const int e = kCase[m][1 + 3 * x + (odd && s ? 3 - s : s)];
        const int ca = kTetCorner[q][kEdgeA[e]], cb = kTetCorner[q][kEdgeB[e]];
        const int64_t owner = node_at(i, j, k, ca, bits);
        const uint32_t below = static_cast<uint32_t>(emask[owner]) & ((1u << ((cb ^ ca) - 1)) - 1u);
        tris[3 * at + s] = static_cast<int32_t>(vpos[owner] + static_cast<uint32_t>(__popc(below)));
      }
    }
  }
}

// remove_vertices_by_mask
__global__ __launch_bounds__(kT) void k_mesh_keep_t(const int32_t* __restrict__ tris, int64_t n_t, int64_t n_v,
                                                    const uint32_t* __restrict__ keep, uint32_t* __restrict__ tkeep) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  uint32_t ok = 1u;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int64_t v = tris[3 * t + s];
    ok &= (v >= 0 && v < n_v) ? keep[v] : 0u;  // (an index outside the mesh drops the triangle; never a load)
  }
  tkeep[t] = ok;
}

__global__ __launch_bounds__(kT) void k_mesh_gather_t(const int32_t* __restrict__ tris, int64_t n_t,
                                                      const uint32_t* __restrict__ tkeep,
                                                      const uint32_t* __restrict__ tpos,
                                                      const uint32_t* __restrict__ pos, int32_t* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t || !tkeep[t]) return;
  const int64_t o = tpos[t];
#pragma unroll
  for (int s = 0; s < 3; ++s) out[3 * o + s] = static_cast<int32_t>(pos[tris[3 * t + s]]);
}

bool make_box(int depth, const double* origin, double h, Box* b) {
  if (depth < 1 || depth > 10 || !origin || !(h > 0.0) || !std::isfinite(h)) return false;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(origin[a])) return false;
    b->o[a] = origin[a];
  }
  b->h = h;
  b->bits = depth;
  return true;
}

constexpr const char* kBadBox = "mesh: depth must be 1..10, origin and h finite, h > 0";

}  // namespace msh
}  // namespace

extern "C" {

int sl_mesh_splat(sl_ctx* c, const double* xyz, const double* normals, int64_t n, int depth, const double* origin,
                  double h, int64_t* acc, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  Box b;
  if (!make_box(depth, origin, h, &b)) return slgpu_fail(c, SL_EINVAL, kBadBox);
  if (n < 0 || n >= (1ll << 31) || (n && (!xyz || !normals)) || !acc)
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_splat: bad sizes or NULL arguments");
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  hipLaunchKernelGGL(k_mesh_splat, dim3(blocks(n)), dim3(kT), 0, s, xyz, normals, n, b,
                     reinterpret_cast<unsigned long long*>(acc));
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_unfix(sl_ctx* c, const int64_t* acc, int64_t count, float* out, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  if (count < 0 || (count && (!acc || !out))) return slgpu_fail(c, SL_EINVAL, "sl_mesh_unfix: bad arguments");
  if (count == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  constexpr int64_t kSlice = int64_t{1} << 30;  // a launch holds fewer than 2^32 threads
  for (int64_t at = 0; at < count; at += kSlice) {
    const int64_t m = std::min(kSlice, count - at);
    hipLaunchKernelGGL(k_mesh_unfix, dim3(blocks(m)), dim3(kT), 0, s, acc + at, m, out + at);
  }
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_divergence(sl_ctx* c, const float* V, int depth, double h, float* div, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  const double zero[3] = {0.0, 0.0, 0.0};
  Box b;
  if (!make_box(depth, zero, h, &b)) return slgpu_fail(c, SL_EINVAL, kBadBox);
  if (!V || !div) return slgpu_fail(c, SL_EINVAL, "sl_mesh_divergence: NULL arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  hipLaunchKernelGGL(k_mesh_div, dim3(blocks(int64_t{1} << (3 * depth))), dim3(kT), 0, s, V, depth, 2.0 * h, div);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_sample(sl_ctx* c, const float* grid, int depth, const double* origin, double h, const double* xyz,
                   int64_t n, double* out, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  Box b;
  if (!make_box(depth, origin, h, &b)) return slgpu_fail(c, SL_EINVAL, kBadBox);
  if (n < 0 || !grid || (n && (!xyz || !out))) return slgpu_fail(c, SL_EINVAL, "sl_mesh_sample: bad arguments");
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  hipLaunchKernelGGL(k_mesh_sample, dim3(blocks(n)), dim3(kT), 0, s, grid, b, xyz, n, out);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_ordered_sum(sl_ctx* c, const double* v, int64_t n, int64_t stride, int64_t offset, double* sum, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  if (n < 0 || stride < 1 || offset < 0 || offset >= stride || (n && !v) || !sum)
    return slgpu_fail(c, SL_EINVAL, "sl_ordered_sum: bad arguments");
  *sum = 0.0;
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  const int64_t chunks = (n + prim::kChunk - 1) / prim::kChunk;
  DBuf<double> part, out;
  MTRY(c, part.alloc(chunks));
  MTRY(c, out.alloc(1));
  hipLaunchKernelGGL(k_osum_part, dim3(static_cast<unsigned>(chunks)), dim3(kT), 0, s, v, n, stride, offset, part.p);
  hipLaunchKernelGGL(prim::k_plane_fold_sum, dim3(1), dim3(kT), 0, s, part.p, chunks, out.p);
  MTRY(c, hipGetLastError());
  MTRY(c, hipMemcpyAsync(sum, out.p, sizeof(double), hipMemcpyDeviceToHost, s));
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_orient_normals(sl_ctx* c, const double* xyz, double* normals, int64_t n, const double* location,
                      void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  if (n < 0 || !location || (n && (!xyz || !normals)))
    return slgpu_fail(c, SL_EINVAL, "sl_orient_normals: bad arguments");
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  hipLaunchKernelGGL(k_orient, dim3(blocks(n)), dim3(kT), 0, s, xyz, normals, n, location[0], location[1],
                     location[2]);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_extract_count(sl_ctx* c, const float* chi, int depth, double iso, uint8_t* emask, uint32_t* vpos,
                          uint32_t* tpos, int64_t* n_vertices, int64_t* n_triangles, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  if (depth < 1 || depth > 10) return slgpu_fail(c, SL_EINVAL, kBadBox);
  if (!chi || !emask || !vpos || !tpos || !n_vertices || !n_triangles)
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_extract_count: NULL arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  const int64_t n3 = int64_t{1} << (3 * depth);
  hipLaunchKernelGGL(k_mesh_count, dim3(blocks(n3)), dim3(kT), 0, s, chi, iso, depth, emask, vpos, tpos);
  MTRY(c, hipGetLastError());
  // the scans are 32-bit: a depth-10 field that crosses iso in most of its cubes
  // (up to 7 vertices and 12 triangles each) is beyond them; emit never stores
  // past the totals returned here
  int r = scan_flags(c, vpos, n3, vpos, n_vertices, s);
  if (r) return r;
  r = scan_flags(c, tpos, n3, tpos, n_triangles, s);
  if (r) return r;
  if (*n_vertices >= (1ll << 31) || *n_triangles >= (1ll << 31))
    return slgpu_fail(c, SL_ECAPACITY, "sl_mesh_extract_count: more than 2^31 - 1 vertices or triangles");
  return SL_OK;
}

int sl_mesh_extract_emit(sl_ctx* c, const float* chi, int depth, double iso, const double* origin, double h,
                         const uint8_t* emask, const uint32_t* vpos, const uint32_t* tpos, int64_t n_vertices,
                         int64_t n_triangles, double* vertices, int32_t* triangles, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  Box b;
  if (!make_box(depth, origin, h, &b)) return slgpu_fail(c, SL_EINVAL, kBadBox);
  if (!chi || !emask || !vpos || !tpos || n_vertices < 0 || n_triangles < 0 || (n_vertices && !vertices) ||
      (n_triangles && !triangles))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_extract_emit: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  const int64_t n3 = int64_t{1} << (3 * depth);
  if (n_vertices)
    hipLaunchKernelGGL(k_mesh_emit_v, dim3(blocks(n3)), dim3(kT), 0, s, chi, iso, b, emask, vpos, n_vertices,
                       vertices);
  if (n_triangles)
    hipLaunchKernelGGL(k_mesh_emit_t, dim3(blocks(n3)), dim3(kT), 0, s, chi, iso, depth, emask, vpos, tpos,
                       n_triangles, triangles);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_remove_vertices(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                            int64_t n_triangles, const uint8_t* mask, double* out_vertices, int32_t* out_triangles,
                            int64_t* out_n_vertices, int64_t* out_n_triangles, void* stream) {
  using namespace msh;
  if (!c) return SL_EINVAL;
  if (n_vertices < 0 || n_triangles < 0 || n_vertices >= (1ll << 31) || n_triangles >= (1ll << 31) ||
      !out_n_vertices || !out_n_triangles || (n_vertices && (!vertices || !mask || !out_vertices)) ||
      (n_triangles && (!triangles || !out_triangles)))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_remove_vertices: bad sizes or NULL arguments");
  *out_n_vertices = *out_n_triangles = 0;
  if (n_vertices == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  DBuf<uint32_t> keep, pos, tkeep, tpos;
  MTRY(c, keep.alloc(n_vertices));
  MTRY(c, pos.alloc(n_vertices));
  hipLaunchKernelGGL(k_keep_unmasked, dim3(blocks(n_vertices)), dim3(kT), 0, s, mask, n_vertices, keep.p);
  MTRY(c, hipGetLastError());
  int r = compact_rows<double, 3>(c, vertices, n_vertices, keep.p, pos.p, out_vertices, out_n_vertices, s);
  if (r) return r;
  if (n_triangles) {
    MTRY(c, tkeep.alloc(n_triangles));
    MTRY(c, tpos.alloc(n_triangles));
    hipLaunchKernelGGL(k_mesh_keep_t, dim3(blocks(n_triangles)), dim3(kT), 0, s, triangles, n_triangles, n_vertices,
                       keep.p, tkeep.p);
    MTRY(c, hipGetLastError());
    r = scan_flags(c, tkeep.p, n_triangles, tpos.p, out_n_triangles, s);
    if (r) return r;
    hipLaunchKernelGGL(k_mesh_gather_t, dim3(blocks(n_triangles)), dim3(kT), 0, s, triangles, n_triangles, tkeep.p,
                       tpos.p, pos.p, out_triangles);
    MTRY(c, hipGetLastError());
  }
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

}  // extern "C"
