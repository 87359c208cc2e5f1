// libslgpu.so, part 2a -- the primitives the feature files share, included at
// the end of slmerge.hip before the first of them (one translation unit: it uses
// that file's scratch pool and launch helpers).  What belongs here: a small
// device or host piece that MORE THAN ONE feature file uses.  Nothing here is an
// algorithm of its own or names a feature's namespace; a feature file names
// slmerge.hip proper and prim::, never another feature (DESIGN.md, Appendix C.1
// lists every piece's users).  Kernels keep the names they had where they came
// from: profiles and the benches' kernel groups know them by those.
//
// Lock-free union-find: why it is wait-free (the one statement of the argument).
// parent[] starts as the identity (k_clu_init).  A root is hooked under a SMALLER
// root by atomicCAS(parent[a], a, b), b < a, and only roots are hooked, so
// parents only decrease, no cycle can form, and a component's final root is its
// smallest member whatever the interleaving.  Path halving lowers a non-root's
// parent to an ancestor by atomicMin.
// Stale reads.  Within a launch the L1s and the per-XCD L2s are not coherent;
// parent words are read by agent-scope relaxed atomic loads, and even those may
// return an older value.  An older value of parent[x] is x itself or an older
// ancestor of x (a word only ever moves down its own ancestor chain), so:
//   - find_root() walks strictly decreasing indices and ends at a point that WAS
//     a root: no wait, no spin;
//   - a hook on a point that is no longer a root fails its CAS, which returns
//     the true parent, and the loop continues from THAT value (never from a
//     plain re-read), so every retry is strictly lower: progress without
//     waiting on another workgroup;
//   - "both ends share an ancestor" is true of stale ancestors only if it is
//     true: ancestors are never un-made.
// A stale read therefore costs steps and never a wrong union; the atomics
// themselves act on the one copy at the device's coherence point.  After the
// launch (a kernel boundary makes everything visible) the trees are walked with
// plain loads.
//
// Ordered sum: slplane.inl's header DEFINES the summation order (chunks of
// kChunk points, kRows rows a lane, tree_sum, the chunk sums left to right);
// the pieces of it that slmesh.inl's sl_ordered_sum needs as well live here.

#include <time.h>

namespace {
namespace prim {

// ---------------------------------------------------------------- fold_min ----
constexpr int kFold = 4;  // labels a wave folds before its remaining lanes go alone

// atomicMin(dst[label], key) of every pending lane.  Called by all lanes of the
// wave together (no lane has returned); lanes that share the first pending lane's
// label fold into one atomic, kFold times, then every lane left goes alone.
template <typename T>
__device__ __forceinline__ void fold_min(T* dst, uint32_t label, T key, bool pending) {
  const int lane = threadIdx.x & 63;
  for (int it = 0; it < kFold; ++it) {
    const unsigned long long m = __ballot(pending);
    if (!m) return;  // wave-uniform
    const int leader = __ffsll(m) - 1;
    const uint32_t L = __shfl(label, leader);
    const bool mine = pending && label == L;
    T v = mine ? key : static_cast<T>(~static_cast<T>(0));
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const T t = __shfl_xor(v, o);
      v = t < v ? t : v;
    }
    if (lane == leader) atomicMin(dst + L, v);
    pending = pending && !mine;
  }
  if (pending) atomicMin(dst + label, key);
}

// -------------------------------------------------------------- union-find ----
__device__ __forceinline__ uint32_t ld_parent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A point that is (or, read stale, was) the root of x's tree; halves the path.
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = ld_parent(parent + x);
    if (p == x) return x;
    const uint32_t g = ld_parent(parent + p);
    if (g == p) return p;
    atomicMin(parent + x, g);  // g <= p < x: an ancestor of x
    x = g;
  }
}

// One tree for a and b; returns a point that is an ancestor of both.
__device__ __forceinline__ uint32_t unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return a;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = atomicCAS(parent + a, a, b);  // the larger root under the smaller
    if (old == a) return b;
    a = old;  // a had been hooked already: go on from its true parent (< a)
  }
}

__global__ __launch_bounds__(kT) void k_clu_init(int64_t n, uint32_t* parent) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < n) parent[i] = static_cast<uint32_t>(i);
}

// -------------------------------------------------------------- StageClock ----
// Host milliseconds of a stage, read once the stream is idle.
struct StageClock {
  hipStream_t s;
  double t0;
  static double now() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e3 * static_cast<double>(ts.tv_sec) + 1e-6 * static_cast<double>(ts.tv_nsec);
  }
  explicit StageClock(hipStream_t st) : s(st), t0(now()) {}
  hipError_t lap(double* ms) {
    const hipError_t e = hipStreamSynchronize(s);
    const double t = now();
    *ms = t - t0;
    t0 = t;
    return e;
  }
};

// ---------------------------------------------------------- input checks ----
// Zero one word, let `launch(word)` queue a kernel that raises it on a bad
// input, read it back: `code` with the caller's `msg` when it was raised.
template <typename Launch>
int require_clear(sl_ctx* c, int code, const char* msg, hipStream_t s, Launch launch) {
  DBuf<unsigned> bad;
  MTRY(c, bad.alloc(1));
  MTRY(c, hipMemsetAsync(bad.p, 0, sizeof(unsigned), s));
  launch(bad.p);
  MTRY(c, hipGetLastError());
  unsigned h = 0;
  MTRY(c, hipMemcpyAsync(&h, bad.p, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  MTRY(c, hipStreamSynchronize(s));
  return h ? slgpu_fail(c, code, msg) : SL_OK;
}

__global__ __launch_bounds__(kT) void k_clu_finite(const double* xyz, int64_t n3, unsigned* bad) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i < n3 && !isfinite(xyz[i])) atomicOr(bad, 1u);
}

// SL_EINVAL with `msg` when a coordinate is not finite.
int require_finite(sl_ctx* c, const double* xyz, int64_t n, const char* msg, hipStream_t s) {
  return require_clear(c, SL_EINVAL, msg, s, [&](unsigned* bad) {
    hipLaunchKernelGGL(k_clu_finite, dim3(blocks(3 * n)), dim3(kT), 0, s, xyz, 3 * n, bad);
  });
}

__global__ __launch_bounds__(kT) void k_mc_check(const int32_t* tris, int64_t n3, int64_t n_v, unsigned* bad) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= n3) return;
  const int64_t v = tris[i];
  if (v < 0 || v >= n_v) atomicOr(bad, 1u);
}

// SL_EINDEX with `msg` when an index is outside 0 .. n_v - 1 (nothing is indexed here).
int require_indices(sl_ctx* c, const int32_t* tris, int64_t n_t, int64_t n_v, const char* msg, hipStream_t s) {
  if (n_t == 0) return SL_OK;
  return require_clear(c, SL_EINDEX, msg, s, [&](unsigned* bad) {
    hipLaunchKernelGGL(k_mc_check, dim3(blocks(3 * n_t)), dim3(kT), 0, s, tris, 3 * n_t, n_v, bad);
  });
}

// -------------------------------------------------------------------- draw ----
struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 ld3(const double* p, int64_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// the n-th random index below nc of the RANSACs (splitmix64 of seed + (n + 1) golden)
__device__ __forceinline__ int64_t draw(uint64_t seed, uint64_t n, uint64_t nc) {
  uint64_t z = seed + (n + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return static_cast<int64_t>(((z >> 32) * nc) >> 32);
}

// ------------------------------------------------------------- ordered sum ----
constexpr int kRows = 16;           // rows of a chunk each lane holds
constexpr int kChunk = kT * kRows;  // 4096 points

// The tree of the ordered sum over the workgroup's 256 lane sums -> s[0].
__device__ __forceinline__ void tree_sum(double* s, double v) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int w = kT / 2; w > 0; w >>= 1) {
    if (t < w) s[t] = s[t] + s[t + w];
    __syncthreads();
  }
}

// row blockIdx.x of part[rows][chunks]: the chunk sums added to 0.0 left to right
__global__ __launch_bounds__(kT) void k_plane_fold_sum(const double* __restrict__ part, int64_t chunks,
                                                       double* __restrict__ out) {
  __shared__ double s[kT];
  const double* row = part + static_cast<int64_t>(blockIdx.x) * chunks;
  double acc = 0.0;
  for (int64_t c0 = 0; c0 < chunks; c0 += kT) {
    if (c0 + threadIdx.x < chunks) s[threadIdx.x] = row[c0 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = static_cast<int>(min<int64_t>(kT, chunks - c0));
      for (int j = 0; j < m; ++j) acc = acc + s[j];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// ------------------------------------------------------- rotated triples ----
// (sl_mesh_simplify_clustering's and sl_mesh_remove_duplicated_triangles' test for "the same triangle")
// rot[t]: the mapped triple (vmap NULL: the triple itself) rotated so that its strictly smallest index comes first
// (a triple whose smallest index occurs twice stays as it is); ok[t] = 0 when two are equal
__global__ __launch_bounds__(kT) void k_sc_tris(const int32_t* tris, int64_t n_t, const uint32_t* vmap, uint32_t* rot,
                                                uint32_t* ok) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (t >= n_t) return;
  uint32_t a = static_cast<uint32_t>(tris[3 * t]), b = static_cast<uint32_t>(tris[3 * t + 1]),
           c = static_cast<uint32_t>(tris[3 * t + 2]);
  if (vmap) {
    a = vmap[a];
    b = vmap[b];
    c = vmap[c];
  }
  uint32_t r0 = a, r1 = b, r2 = c;
  if (b < a && b < c) {
    r0 = b;
    r1 = c;
    r2 = a;
  } else if (c < a && c < b) {
    r0 = c;
    r1 = a;
    r2 = b;
  }
  rot[3 * t] = r0;
  rot[3 * t + 1] = r1;
  rot[3 * t + 2] = r2;
  ok[t] = (a != b && b != c && c != a) ? 1u : 0u;
}

// head[j] = 1 for the first occurrence (the smallest position: the sorts are stable) of every triple
__global__ __launch_bounds__(kT) void k_sc_heads(const uint32_t* tri, const uint32_t* vals, int64_t n, uint32_t* head) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (i >= n) return;
  const int64_t j = vals[i];
  bool first = i == 0;
  if (!first) {
    const int64_t q = vals[i - 1];
    first = tri[3 * j] != tri[3 * q] || tri[3 * j + 1] != tri[3 * q + 1] || tri[3 * j + 2] != tri[3 * q + 2];
  }
  head[j] = first ? 1u : 0u;
}

// ------------------------------------------------------ triangle sides ----
// The sorted side table of a mesh: what the components, the adjacency, the checks and the boundary loops all start
// from.  (a, b, c) has the sides a->b, b->c, c->a; a side's key is min V + max (below 2^62), its value 3 t + k.  The
// sort is stable and by key alone, so a run holds one undirected edge's sides in ascending 3 t + k.
// Limits: bad_sizes (V < 2^31 for the keys, 3 T < 2^32 for the values); the adjacency's CSR can hold two entries per
// side and asks for bad_csr_sizes (6 T < 2^32) instead.
//
// dst += the lanes of the wave with p set: one atomic per wave.  Called by all lanes of the wave together.
__device__ __forceinline__ void wave_add(unsigned long long* dst, bool p) {
  const unsigned long long m = __ballot(p);
  if (m && (threadIdx.x & 63) == __ffsll(m) - 1) atomicAdd(dst, static_cast<unsigned long long>(__popcll(m)));
}

struct Side {
  uint32_t t, k, from, to;
};
// the side a sorted value 3 t + k names
__device__ __forceinline__ Side side_of(const int32_t* tris, uint32_t val) {
  Side s;
  s.t = val / 3u;
  s.k = val - 3u * s.t;
  s.from = static_cast<uint32_t>(tris[val]);
  s.to = static_cast<uint32_t>(tris[s.k == 2u ? val - 2u : val + 1u]);
  return s;
}

// Three (key, 3 t + k) pairs per triangle.  Optional (NULL: skipped): the corner parents and the parity words start
// as roots, *n_degenerate += the triangles with two equal indices.
__global__ __launch_bounds__(kT) void k_mk_sides(const int32_t* tris, int64_t n_t, uint64_t n_v, uint64_t* keys,
                                                 uint32_t* vals, uint32_t* parent, uint32_t* word,
                                                 unsigned long long* n_degenerate) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  const bool live = t < n_t;
  bool deg = false;
  if (live) {
    const uint64_t a = static_cast<uint64_t>(tris[3 * t]), b = static_cast<uint64_t>(tris[3 * t + 1]),
                   c = static_cast<uint64_t>(tris[3 * t + 2]);
    keys[3 * t] = a < b ? a * n_v + b : b * n_v + a;
    keys[3 * t + 1] = b < c ? b * n_v + c : c * n_v + b;
    keys[3 * t + 2] = c < a ? c * n_v + a : a * n_v + c;
    const uint32_t v = static_cast<uint32_t>(3 * t);
    vals[3 * t] = v;
    vals[3 * t + 1] = v + 1u;
    vals[3 * t + 2] = v + 2u;
    if (parent) {
      parent[3 * t] = v;
      parent[3 * t + 1] = v + 1u;
      parent[3 * t + 2] = v + 2u;
    }
    if (word) word[t] = static_cast<uint32_t>(t) << 1;
    deg = a == b || b == c || c == a;
  }
  if (n_degenerate) wave_add(n_degenerate, deg);
}

bool bad_sizes(int64_t n_v, int64_t n_t) {
  return n_v < 0 || n_t < 0 || n_v >= (1ll << 31) || 3 * n_t >= (1ll << 32);
}
bool bad_csr_sizes(int64_t n_v, int64_t n_t) { return bad_sizes(n_v, n_t) || 6 * n_t >= (1ll << 32); }

struct SideTable {
  DBuf<uint64_t> keys;  // [n3] ascending
  DBuf<uint32_t> vals;  // [n3] 3 t + k
  int64_t n3 = 0;
};

// The table of n_t > 0 triangles whose indices were checked; the three optional pointers are k_mk_sides'.  Two laps
// of the caller's clock: *keys_ms takes what was queued since its last lap and k_mk_sides, *sort_ms the sort
// (NULL: no second lap, the caller's stage goes on).
int sort_sides(sl_ctx* c, const int32_t* tris, int64_t n_t, uint64_t n_v, SideTable& S, uint32_t* corner_parent,
               uint32_t* parity_word, unsigned long long* n_degenerate, StageClock& clock, double* keys_ms,
               double* sort_ms, hipStream_t s) {
  S.n3 = 3 * n_t;
  MTRY(c, S.keys.alloc(S.n3));
  MTRY(c, S.vals.alloc(S.n3));
  hipLaunchKernelGGL(k_mk_sides, dim3(blocks(n_t)), dim3(kT), 0, s, tris, n_t, n_v, S.keys.p, S.vals.p, corner_parent,
                     parity_word, n_degenerate);
  MTRY(c, hipGetLastError());
  MTRY(c, clock.lap(keys_ms));
  const int r = radix_sort(c, S.keys.p, S.vals.p, S.n3, key_bits(n_v * n_v - 1), s);  // only the bits the keys have
  if (r) return r;
  if (sort_ms) MTRY(c, clock.lap(sort_ms));
  return SL_OK;
}

// 0 when sorted position i < n3 is not the first of its run, else the run's sides: 1, 2, or 3 for three and more.
// Reads keys[i - 1 .. i + 2] at most.
__device__ __forceinline__ int run_sides(const uint64_t* keys, int64_t i, int64_t n3) {
  const uint64_t k = keys[i];
  if (i > 0 && keys[i - 1] == k) return 0;
  if (i + 1 >= n3 || keys[i + 1] != k) return 1;
  return i + 2 < n3 && keys[i + 2] == k ? 3 : 2;
}

// ------------------------------------------------------------ small pieces ----
// x's root by plain loads: valid only after the kernel boundary that follows the unions (the header above).
__device__ __forceinline__ uint32_t root_of(const uint32_t* parent, uint32_t x) {
  for (uint32_t p = parent[x]; p != x; p = parent[x]) x = p;  // strictly decreasing
  return x;
}

// A_t = 0.5 sqrt((n0 n0 + n1 n1) + n2 n2), n = (p1 - p0) x (p2 - p0), f64, uncontracted: the one triangle area.
__device__ __forceinline__ double tri_area(const D3& p0, const D3& p1, const D3& p2) {
  const double e10 = p1.x - p0.x, e11 = p1.y - p0.y, e12 = p1.z - p0.z;
  const double e20 = p2.x - p0.x, e21 = p2.y - p0.y, e22 = p2.z - p0.z;
  const double n0 = e11 * e22 - e12 * e21, n1 = e12 * e20 - e10 * e22, n2 = e10 * e21 - e11 * e20;
  return 0.5 * sqrt((n0 * n0 + n1 * n1) + n2 * n2);
}

// The body of every sl_*_stats(double*, int): the thread's last N figures, zeros behind them.
template <int N>
int copy_stats(const double (&tls)[N], double* out, int capacity) {
  if (capacity < 0 || (capacity && !out)) return SL_EINVAL;
  for (int i = 0; i < capacity; ++i) out[i] = i < N ? tls[i] : 0.0;
  return SL_OK;
}

}  // namespace prim
}  // namespace
