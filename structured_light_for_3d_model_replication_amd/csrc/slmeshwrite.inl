// libslgpu.so, part 2j -- writing a triangle mesh from device memory, included at
// the end of slmerge.hip (one translation unit: it shares that file's scratch
// pool and slprim.inl's index check).  o3d.io.write_triangle_mesh for
// ``.stl`` and ``.ply`` after compute_vertex_normals(): the records are packed
// on the device and streamed to the file through a small ring of pinned chunks.
// Open3D is not in this image, so its PLY layout and its NormalizeNormals rule
// are restated from memory and UNPINNED; tests/mesh_oracle.py (STL, triangle
// normals) and tests/meshwrite_oracle.py (vertex normals, PLY) are the CPU
// forms the results equal byte for byte.
//
// Input: vertices f64 [V][3], triangles int32 [T][3]; V, T < 2^31.  Every index
// is read by k_mc_check before the file is opened: one outside 0 .. V-1 is
// SL_EINDEX, the path is not touched.
//
//   triangle normal   e1 = p1 - p0, e2 = p2 - p0, n = e1 x e2 (n0 = e1y e2z - e1z
//              e2y, n1 = e1z e2x - e1x e2z, n2 = e1x e2y - e1y e2x), ln = sqrt((n0 n0
//              + n1 n1) + n2 n2), n / ln, or +0 three times when ln == 0; f64,
//              uncontracted, sqrt and division correctly rounded: the bits of the
//              host writer and of mesh_oracle.triangle_normals.
//   vertex normal     every triangle adds q_c = llrint(n_c 2^40) (ties to even; 0
//              unless |n_c 2^40| < 2^62, so a NaN adds nothing) of its unit normal to
//              the three sums of each of its three vertices: wrapping 64-bit
//              integer atomics.  s_c = double(sum_c) (nearest even); a vertex with
//              three zero sums (in no triangle, or normals that cancel) gets (0, 0,
//              1), every other s / sqrt((sx sx + sy sy) + sz sz): the scale cancels
//              and is not divided out.  DEVIATION: Open3D adds the f64 unit normals
//              in triangle order, which is a traversal; fixed-point sums stand in
//              for them, so the result does not depend on any order and repeats.
//   STL record        50 bytes: float(n), float(p0), float(p1), float(p2) (f64 ->
//              f32 to nearest even, overflow to +-inf, -0 kept), a zero uint16.
//   PLY               "ply / format binary_little_endian 1.0 / comment Created by
//              Open3D / element vertex V / property double x y z nx ny nz /
//              element face T / property list uchar uint vertex_indices /
//              end_header", V records of six doubles (48 bytes), T records of the
//              byte 3 and three uint32 (13 bytes).
//   coloured PLY      with vertex colours (BGR u8 [V][3]; slmeshcolor.inl makes
//              them) "property uchar red / green / blue" follow nz and a vertex
//              record has 51 bytes: the six doubles, then red green blue.
//
// Packing.  None of 50, 13 and 51 is a multiple of 4: a thread per record storing
// to global memory would scatter 1- and 2-byte stores.  A workgroup of 256 threads
// builds the image of 256 records in LDS (12 800 B / 3 328 B / 13 056 B,
// multiples of 16) and, after one barrier, stores it lane-linear in 16-byte lines
// (1 KiB per wave store) to the 16-byte-aligned slot.  The LDS writes are free of
// bank conflicts (ds_write_b32: bank = dword mod 32 within a 32-lane half):
//   STL   two records are 25 dwords.  The even record of pair p is dwords 25 p ..
//         25 p + 11 and the low half of dword 25 p + 12, which is its zero
//         attribute; the odd one starts in the high half of that dword and ends
//         with its own zero attribute in the high half of dword 25 p + 24.  Both
//         attributes being constants, the even record's thread writes 12 whole
//         dwords and the odd one's 13, from its own floats alone.  Threads 0..127
//         take the even records and 128..255 the odd ones, so a wave writes one
//         dword per lane at a stride of 25 dwords: 32 consecutive p give 32
//         different banks.
//   PLY   faces and coloured vertices, one packer (pack_quarters over slrecord.h's
//         put_record_at).  Four records of REC bytes are REC dwords; record r
//         starts at byte (REC r) mod 4 of a dword: r mod 4 for a face, (3 r) mod 4
//         for a vertex.  Wave k takes the records with r mod 4 == k (r = 4 lane +
//         k), so the shape of a record's writes -- leading bytes up to the dword
//         boundary, whole dwords, trailing bytes -- is wave-uniform and the lanes'
//         stride is REC dwords, 13 or 51: odd, so conflict-free again.  The
//         partial dwords are written as 1- and 2-byte LDS stores by the two
//         records that share them.
// The threads of a wave read every second (fourth) index triple; the waves of
// the workgroup touch the same lines, which the vector cache serves.
//
// Streaming.  The body never exists as a whole: the records go through the context's ring of chunk slots
// (slstream.h states the order), kRing slots of one chunk (default 655 360 triangles, 32 768 000 B; they grow only
// when a larger chunk is asked for, up to kMaxChunkTriangles).  Chunk k is packed into device slot k mod kRing.
// Staging is kRing (slot + slot) bytes whatever T is; the PLY writer also holds the 24 V bytes of the vertex sums.

#include <string>

#include "slrecord.h"

namespace {
namespace mwr {

constexpr int64_t kChunkTriangles = 655360;                      // 32 768 000 B of STL records
constexpr int64_t kMaxChunkTriangles = 8 * kChunkTriangles;
constexpr int kStlRec = 50, kFaceRec = 13, kVertexRec = 48, kColRec = 51;
// 16-byte lines of a workgroup's image: 800, 208, 816
constexpr int kStlLines = kT * kStlRec / 16, kFaceLines = kT * kFaceRec / 16, kColLines = kT * kColRec / 16;
constexpr double kVnFix = 1099511627776.0;                       // 2^40
constexpr double kVnFixMax = 4611686018427387904.0;              // 2^62

thread_local double tls_ms[3];  // waiting for chunks to land, writing them, the whole call

// The corners of triangle t and its unit normal (the header's arithmetic).
__device__ __forceinline__ void tri_normal(const double* __restrict__ verts, const int32_t* __restrict__ tris, int64_t t,
                                           double* p, double* n) {
  const int64_t a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p[k] = verts[3 * a + k];
    p[3 + k] = verts[3 * b + k];
    p[6 + k] = verts[3 * c + k];
  }
  const double e10 = p[3] - p[0], e11 = p[4] - p[1], e12 = p[5] - p[2];
  const double e20 = p[6] - p[0], e21 = p[7] - p[1], e22 = p[8] - p[2];
  const double n0 = e11 * e22 - e12 * e21, n1 = e12 * e20 - e10 * e22, n2 = e10 * e21 - e11 * e20;
  const double ln = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  const bool flat = ln == 0.0;
  n[0] = flat ? 0.0 : n0 / ln;
  n[1] = flat ? 0.0 : n1 / ln;
  n[2] = flat ? 0.0 : n2 / ln;
}

__global__ __launch_bounds__(kT) void k_mw_tri_normals(const double* __restrict__ verts,
                                                       const int32_t* __restrict__ tris, int64_t n_t,
                                                       double* __restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  double p[9], n[3];
  tri_normal(verts, tris, t, p, n);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 * t + k] = n[k];
}

__device__ __forceinline__ int64_t vn_fix(double v) {
  const double t = v * kVnFix;
  return fabs(t) < kVnFixMax ? llrint(t) : 0;
}

// sums[v][c] += vn_fix(n_c) for the three vertices of every triangle (wrapping)
__global__ __launch_bounds__(kT) void k_mw_vn_add(const double* __restrict__ verts, const int32_t* __restrict__ tris,
                                                  int64_t n_t, unsigned long long* __restrict__ sums) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  double p[9], n[3];
  tri_normal(verts, tris, t, p, n);
  unsigned long long q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) q[k] = static_cast<unsigned long long>(vn_fix(n[k]));
  if (!(q[0] | q[1] | q[2])) return;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int64_t v = tris[3 * t + j];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (q[k]) atomicAdd(sums + 3 * v + k, q[k]);
  }
}

__device__ __forceinline__ void vn_of(const int64_t* __restrict__ sums, int64_t v, double* n) {
  const double sx = static_cast<double>(sums[3 * v]), sy = static_cast<double>(sums[3 * v + 1]),
               sz = static_cast<double>(sums[3 * v + 2]);
  if (sx == 0.0 && sy == 0.0 && sz == 0.0) {
    n[0] = n[1] = 0.0;
    n[2] = 1.0;
    return;
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  n[0] = sx / len;
  n[1] = sy / len;
  n[2] = sz / len;
}

__global__ __launch_bounds__(kT) void k_mw_vn_norm(const int64_t* __restrict__ sums, int64_t n_v,
                                                   double* __restrict__ out) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n_v) return;
  double n[3];
  vn_of(sums, v, n);
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 * v + k] = n[k];
}

// Store the first `bytes` bytes (rounded up to whole 16-byte lines) of the workgroup's LDS image.
__device__ __forceinline__ void store_lines(const uint4* img, int bytes, uint4* __restrict__ out) {
  const int lines = (bytes + 15) >> 4;
  for (int i = threadIdx.x; i < lines; i += kT) out[i] = img[i];
}

// STL records of the triangles t0 .. t0 + count - 1 -> out (16-byte aligned, room for whole workgroups).
__global__ __launch_bounds__(kT) void k_mw_pack_stl(const double* __restrict__ verts, const int32_t* __restrict__ tris,
                                                    int64_t t0, int64_t count, uint4* __restrict__ out) {
  __shared__ uint4 img4[kStlLines];
  uint32_t* img = reinterpret_cast<uint32_t*>(img4);
  const int t = threadIdx.x;
  const int odd = t >> 7, pair = t & 127, r = 2 * pair + odd;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kT;
  uint32_t f[12];
  if (first + r < count) {
    double p[9], n[3];
    tri_normal(verts, tris, t0 + first + r, p, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) f[k] = __float_as_uint(static_cast<float>(n[k]));
#pragma unroll
    for (int k = 0; k < 9; ++k) f[3 + k] = __float_as_uint(static_cast<float>(p[k]));
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) f[k] = 0u;
  }
  uint32_t* o = img + 25 * pair;
  if (!odd) {  // (wave-uniform)
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = f[k];
  } else {
    o[12] = f[0] << 16;  // the low half: the even record's attribute
#pragma unroll
    for (int k = 0; k < 11; ++k) o[13 + k] = (f[k] >> 16) | (f[k + 1] << 16);
    o[24] = f[11] >> 16;  // the high half: this record's attribute
  }
  __syncthreads();
  const int live = static_cast<int>(min<int64_t>(kT, count - first));
  store_lines(img4, live * kStlRec, out + static_cast<int64_t>(blockIdx.x) * kStlLines);
}

// The quarter-interleaved packers' common part (the header's PLY paragraph): thread t has record r = 4 (t mod 64) +
// t / 64 of the workgroup's 256 records of REC bytes.  fill(i, w) puts record i < count of the chunk into w as
// dwords in memory order; a record past count stays zero.  After the barrier the live records' lines go to `out`.
template <int REC, class Fill>
__device__ __forceinline__ void pack_quarters(uint4 (&img4)[kT * REC / 16], int64_t count, uint4* __restrict__ out,
                                              Fill fill) {
  const int t = threadIdx.x, r = 4 * (t & 63) + (t >> 6);
  const int64_t first = static_cast<int64_t>(blockIdx.x) * kT;
  uint32_t w[(REC + 3) / 4 + 1] = {};
  if (first + r < count) fill(first + r, w);
  slrecord::put_record_at<REC>(reinterpret_cast<unsigned char*>(img4), r, w);  // (wave-uniform shapes)
  __syncthreads();
  const int live = static_cast<int>(min<int64_t>(kT, count - first));
  store_lines(img4, live * REC, out + static_cast<int64_t>(blockIdx.x) * (kT * REC / 16));
}

// PLY face records of the triangles t0 .. t0 + count - 1 -> out (as k_mw_pack_stl): the byte 3, then a b c.
__global__ __launch_bounds__(kT) void k_mw_pack_faces(const int32_t* __restrict__ tris, int64_t t0, int64_t count,
                                                      uint4* __restrict__ out) {
  __shared__ uint4 img4[kFaceLines];
  pack_quarters<kFaceRec>(img4, count, out, [&](int64_t i, uint32_t (&w)[5]) {
    const int64_t g = t0 + i;
    const uint32_t a = static_cast<uint32_t>(tris[3 * g]), b = static_cast<uint32_t>(tris[3 * g + 1]),
                   c = static_cast<uint32_t>(tris[3 * g + 2]);
    w[0] = 3u | (a << 8);
    w[1] = (a >> 24) | (b << 8);
    w[2] = (b >> 24) | (c << 8);
    w[3] = c >> 24;
  });
}

// PLY vertex records of the vertices v0 .. v0 + count - 1: x y z nx ny nz, one double per thread.
__global__ __launch_bounds__(kT) void k_mw_pack_vertices(const double* __restrict__ verts,
                                                         const int64_t* __restrict__ sums, int64_t v0, int64_t count,
                                                         double* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= 6 * count) return;
  const int64_t v = v0 + i / 6;
  const int k = static_cast<int>(i % 6);
  if (k < 3) {
    out[i] = verts[3 * v + k];
  } else {
    double n[3];
    vn_of(sums, v, n);
    out[i] = n[k - 3];
  }
}

// Coloured PLY vertex records of the vertices v0 .. v0 + count - 1 -> out (as k_mw_pack_stl): x y z nx ny nz, then
// red green blue from the BGR storage.
__global__ __launch_bounds__(kT) void k_vc_pack_vertices(const double* __restrict__ verts,
                                                         const int64_t* __restrict__ sums,
                                                         const uint8_t* __restrict__ bgr, int64_t v0, int64_t count,
                                                         uint4* __restrict__ out) {
  __shared__ uint4 img4[kColLines];
  pack_quarters<kColRec>(img4, count, out, [&](int64_t i, uint32_t (&w)[14]) {
    const int64_t v = v0 + i;
    double n[3];
    vn_of(sums, v, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint64_t p = static_cast<uint64_t>(__double_as_longlong(verts[3 * v + k]));
      const uint64_t u = static_cast<uint64_t>(__double_as_longlong(n[k]));
      w[2 * k] = static_cast<uint32_t>(p);
      w[2 * k + 1] = static_cast<uint32_t>(p >> 32);
      w[6 + 2 * k] = static_cast<uint32_t>(u);
      w[7 + 2 * k] = static_cast<uint32_t>(u >> 32);
    }
    w[12] = static_cast<uint32_t>(bgr[3 * v + 2]) | (static_cast<uint32_t>(bgr[3 * v + 1]) << 8) |
            (static_cast<uint32_t>(bgr[3 * v]) << 16);
  });
}

// ---- host
bool bad_mesh(const double* vertices, int64_t n_v, const int32_t* triangles, int64_t n_t) {
  return n_v < 0 || n_t < 0 || n_v >= (1ll << 31) || n_t >= (1ll << 31) || (n_v && !vertices) || (n_t && !triangles);
}

// chunk_triangles: 0 the default, else rounded up to whole workgroups; -1 when out of range
int64_t chunk_of(int64_t chunk_triangles) {
  if (chunk_triangles == 0) return kChunkTriangles;
  if (chunk_triangles < 0 || chunk_triangles > kMaxChunkTriangles) return -1;
  return (chunk_triangles + kT - 1) / kT * kT;
}

// sums[v][c] of the header (zeroed here) on `s`
int vertex_sums(sl_ctx* c, const double* vertices, int64_t n_v, const int32_t* triangles, int64_t n_t, int64_t* sums,
                hipStream_t s) {
  if (n_v) MTRY(c, hipMemsetAsync(sums, 0, sizeof(int64_t) * 3 * static_cast<size_t>(n_v), s));
  if (n_t)
    hipLaunchKernelGGL(k_mw_vn_add, dim3(blocks(n_t)), dim3(kT), 0, s, vertices, triangles, n_t,
                       reinterpret_cast<unsigned long long*>(sums));
  MTRY(c, hipGetLastError());
  return SL_OK;
}

// The PLY writer of `what`: the index check, the vertex sums, the header, then the vertex chunks and the face chunks.
// bgr NULL: the plain 48-byte vertex records; else the 51-byte ones with their three property lines after nz.  A
// slot holds chunk faces, and chunk 50 / 48 plain vertices (the STL writer's slots) or chunk coloured ones.
int write_ply(sl_ctx* c, const char* what, const char* path, const double* vertices, int64_t n_vertices,
              const int32_t* triangles, int64_t n_triangles, const uint8_t* bgr, int64_t chunk_triangles,
              hipStream_t s) {
  const std::string name(what);
  const int64_t chunk = chunk_of(chunk_triangles);
  if (bad_mesh(vertices, n_vertices, triangles, n_triangles) || chunk < 0)
    return slgpu_fail(c, SL_EINVAL, (name + ": bad sizes or NULL arguments").c_str());
  for (double& v : tls_ms) v = 0.0;
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = prim::require_indices(c, triangles, n_triangles, n_vertices, (name + ": triangle index out of range").c_str(),
                               s);
  if (r) return r;
  const int vrec = bgr ? kColRec : kVertexRec;
  const int64_t vchunk = bgr ? chunk : chunk * kStlRec / kVertexRec;
  slstream::Ring* ring = slgpu_file_ring(c);
  MTRY(c, slstream::ring_reserve(ring, std::max(chunk * kStlRec, vchunk * vrec)));
  DBuf<int64_t> sums;
  MTRY(c, sums.alloc(3 * n_vertices));
  r = vertex_sums(c, vertices, n_vertices, triangles, n_triangles, sums.p, s);
  if (r) return r;
  char head[640];
  const int hl = snprintf(head, sizeof(head),
                          "ply\nformat binary_little_endian 1.0\ncomment Created by Open3D\nelement vertex %lld\n"
                          "property double x\nproperty double y\nproperty double z\n"
                          "property double nx\nproperty double ny\nproperty double nz\n%s"
                          "element face %lld\nproperty list uchar uint vertex_indices\nend_header\n",
                          static_cast<long long>(n_vertices),
                          bgr ? "property uchar red\nproperty uchar green\nproperty uchar blue\n" : "",
                          static_cast<long long>(n_triangles));
  const int64_t nvc = (n_vertices + vchunk - 1) / vchunk, nfc = (n_triangles + chunk - 1) / chunk;
  auto v_in = [&](int64_t k) { return std::min(vchunk, n_vertices - k * vchunk); };
  auto f_in = [&](int64_t k) { return std::min(chunk, n_triangles - k * chunk); };
  return slstream::write_chunks(
      c, what, path, head, static_cast<size_t>(hl), ring, nvc + nfc,
      [&](int64_t k, char* dev) {
        if (k >= nvc)
          hipLaunchKernelGGL(k_mw_pack_faces, dim3(blocks(f_in(k - nvc))), dim3(kT), 0, s, triangles,
                             (k - nvc) * chunk, f_in(k - nvc), reinterpret_cast<uint4*>(dev));
        else if (bgr)
          hipLaunchKernelGGL(k_vc_pack_vertices, dim3(blocks(v_in(k))), dim3(kT), 0, s, vertices, sums.p, bgr,
                             k * vchunk, v_in(k), reinterpret_cast<uint4*>(dev));
        else
          hipLaunchKernelGGL(k_mw_pack_vertices, dim3(blocks(6 * v_in(k))), dim3(kT), 0, s, vertices, sums.p,
                             k * vchunk, v_in(k), reinterpret_cast<double*>(dev));
      },
      [&](int64_t k) { return k < nvc ? v_in(k) * vrec : f_in(k - nvc) * kFaceRec; }, s, tls_ms);
}

}  // namespace mwr
}  // namespace

extern "C" {

int sl_mesh_triangle_normals(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                             int64_t n_triangles, double* out, void* stream) {
  using namespace mwr;
  if (!c) return SL_EINVAL;
  if (bad_mesh(vertices, n_vertices, triangles, n_triangles) || (n_triangles && !out))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_triangle_normals: bad sizes or NULL arguments");
  if (n_triangles == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = prim::require_indices(c, triangles, n_triangles, n_vertices,
                               "sl_mesh_triangle_normals: triangle index out of range", s);
  if (r) return r;
  hipLaunchKernelGGL(k_mw_tri_normals, dim3(blocks(n_triangles)), dim3(kT), 0, s, vertices, triangles, n_triangles,
                     out);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_mesh_vertex_normals(sl_ctx* c, const double* vertices, int64_t n_vertices, const int32_t* triangles,
                           int64_t n_triangles, double* out, void* stream) {
  using namespace mwr;
  if (!c) return SL_EINVAL;
  if (bad_mesh(vertices, n_vertices, triangles, n_triangles) || (n_vertices && !out))
    return slgpu_fail(c, SL_EINVAL, "sl_mesh_vertex_normals: bad sizes or NULL arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = prim::require_indices(c, triangles, n_triangles, n_vertices,
                               "sl_mesh_vertex_normals: triangle index out of range", s);
  if (r) return r;
  if (n_vertices == 0) return SL_OK;
  DBuf<int64_t> sums;
  MTRY(c, sums.alloc(3 * n_vertices));
  r = vertex_sums(c, vertices, n_vertices, triangles, n_triangles, sums.p, s);
  if (r) return r;
  hipLaunchKernelGGL(k_mw_vn_norm, dim3(blocks(n_vertices)), dim3(kT), 0, s, sums.p, n_vertices, out);
  MTRY(c, hipGetLastError());
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_write_stl_device(sl_ctx* c, const char* path, const double* vertices, int64_t n_vertices,
                        const int32_t* triangles, int64_t n_triangles, int64_t chunk_triangles, void* stream) {
  using namespace mwr;
  if (!c) return SL_EINVAL;
  const int64_t chunk = chunk_of(chunk_triangles);
  if (bad_mesh(vertices, n_vertices, triangles, n_triangles) || chunk < 0)
    return slgpu_fail(c, SL_EINVAL, "sl_write_stl_device: bad sizes or NULL arguments");
  for (double& v : tls_ms) v = 0.0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));
  int r = prim::require_indices(c, triangles, n_triangles, n_vertices, "sl_write_stl_device: triangle index out of range",
                               s);
  if (r) return r;
  slstream::Ring* ring = slgpu_file_ring(c);
  MTRY(c, slstream::ring_reserve(ring, chunk * kStlRec));
  char head[84] = {};
  const uint32_t count = static_cast<uint32_t>(n_triangles);
  memcpy(head + 80, &count, 4);
  const int64_t n_chunks = (n_triangles + chunk - 1) / chunk;
  auto in_chunk = [&](int64_t k) { return std::min(chunk, n_triangles - k * chunk); };
  return slstream::write_chunks(
      c, "sl_write_stl_device", path, head, sizeof(head), ring, n_chunks,
      [&](int64_t k, char* dev) {
        hipLaunchKernelGGL(k_mw_pack_stl, dim3(blocks(in_chunk(k))), dim3(kT), 0, s, vertices, triangles, k * chunk,
                           in_chunk(k), reinterpret_cast<uint4*>(dev));
      },
      [&](int64_t k) { return in_chunk(k) * kStlRec; }, s, tls_ms);
}

int sl_write_mesh_ply_device(sl_ctx* c, const char* path, const double* vertices, int64_t n_vertices,
                             const int32_t* triangles, int64_t n_triangles, int64_t chunk_triangles, void* stream) {
  if (!c) return SL_EINVAL;
  return mwr::write_ply(c, "sl_write_mesh_ply_device", path, vertices, n_vertices, triangles, n_triangles, nullptr,
                        chunk_triangles, static_cast<hipStream_t>(stream));
}

int sl_write_mesh_ply_colors_device(sl_ctx* c, const char* path, const double* vertices, int64_t n_vertices,
                                    const int32_t* triangles, int64_t n_triangles, const uint8_t* bgr,
                                    int64_t chunk_triangles, void* stream) {
  if (!c) return SL_EINVAL;
  if (n_vertices > 0 && !bgr)
    return slgpu_fail(c, SL_EINVAL, "sl_write_mesh_ply_colors_device: bad sizes or NULL arguments");
  static const uint8_t no_vertices[3] = {};  // V <= 0 and no colours: nothing reads them, the file is a coloured one
  return mwr::write_ply(c, "sl_write_mesh_ply_colors_device", path, vertices, n_vertices, triangles, n_triangles,
                        bgr ? bgr : no_vertices, chunk_triangles, static_cast<hipStream_t>(stream));
}

int sl_mesh_write_stats(double* stage_ms, int capacity) {
  return prim::copy_stats(mwr::tls_ms, stage_ms, capacity);
}

}  // extern "C"
