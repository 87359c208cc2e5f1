// libslgpu.so, part 2e -- consistent tangent-plane normal orientation, included
// at the end of slmerge.hip (one translation unit: it shares that file's scratch
// pool, scan and row compaction and slprim.inl's fold_min).  The reference calls Open3D's orient_normals_consistent_
// tangent_plane(100) (server/processing.py:201, :282): a minimum spanning tree
// of a Riemannian graph (Delaunay-EMST edges plus kNN edges, weight 1 - |ni.nj|)
// walked from the highest point.  This is a restatement on the kNN graph ALONE
// (no Delaunay, so no guarantee that the graph is connected: every connected
// component is oriented by its own root); parity with Open3D is UNPINNED and
// tests/orient_oracle.py is the CPU restatement the tests check against, bit for
// bit.  f64 arithmetic is uncontracted, in the order written here.
//
//   graph: sl_radius_search's idx [n][k] / cnt [n].  Slot s = i k + j names the
//     directed entry (i, idx[i][j]); every slot with j < cnt[i] and idx[i][j] != i
//     is an UNDIRECTED edge candidate between its two points (n k < 2^32).
//   weight: dot = (nx mx + ny my) + nz mz;  w = 1 - |dot| where that is > 0, else
//     0.  Both slots of an edge listed from both ends carry the same weight.
//   order: (w, slot), a strict total order over the slots, so the minimum
//     spanning forest is unique as a SET OF SLOTS whatever algorithm finds it.
//   parity: an edge flips iff dot < 0 (a dot of exactly 0 does not).
//   root, per component: the point of largest z + 0.0 (lowest index on ties); the
//     component is negated iff the root's nz < 0; every other point's sign is the
//     XOR of the flipping edges on its tree path to the root.  Each output normal
//     is exactly +n or -n.
//
// Boruvka with parity-carrying union-find, so no tree is rooted or walked on the
// device.  Every vertex holds ONE packed 32-bit word (label << 1) | parity: label
// is an ancestor (between rounds: its component's representative), parity its
// sign relative to that ancestor; one word, so any read sees a consistent pair.
// A round:
//   (a) scan: one thread per slot (the int32 rows are read contiguously, any k).
//       Weights do not change from round to round, so one pass before the rounds
//       stores every slot's key -- the weight's bit pattern, the sign bit (free:
//       w >= 0) carrying "flips", all ones for a slot that is no edge -- and the
//       rounds stream 8 bytes a slot where they would gather two normals (n k
//       u64 of scratch, the size of sl_radius_search's d2).
//       A slot whose ends carry different labels is a candidate of BOTH ends'
//       components (a kNN row need not be listed back, and the cut property
//       needs every edge that crosses).  Pass 1: atomicMin of the weight's bit
//       pattern per component (non-negative doubles order as u64); pass 2:
//       atomicMin of the slot among the candidates equal to that minimum.  Lanes
//       of a wave that share a label fold their keys first (late rounds: few
//       components, one atomic per wave).  A row with no candidate never has one
//       again (labels only merge) and is skipped from then on.
//   (b) hook: a representative with a winning slot takes the other end's
//       representative as parent, parity par(u) ^ flip ^ par(v); when two
//       components chose the same slot the lower representative stays root.
//       With a strict order those pairs are the only cycles.  The hooked vertex
//       keeps the slot: a vertex is hooked at most once, so the tree list is the
//       compaction of that array (ordered by vertex, the same in every run).
//   (c, d) pointer jumping with parity XOR, one jump per launch over all vertices
//       (a vertex hangs one level below its old representative, so relabelling is
//       the last jump), repeated by the host while a launch changed a word.
//       WITHIN a launch a word read from another workgroup may be stale (the
//       L1s and the per-XCD L2s are not coherent): a stale word is an older
//       ancestor with the parity to THAT ancestor, still a valid pair, so it
//       costs a step and never a wrong sign; roots are not written while
//       jumping, so "my parent is a root" is never read wrongly.  Kernel
//       boundaries make everything visible.
// The host reads one counter per round (hooks; 0 or a spanning tree ends the
// loop) and one flag per jump; rounds and jumps per round are each bounded by
// ceil(log2 n) + 2 and exceeding a bound is an error: nothing spins.

namespace {
namespace ort {

constexpr uint32_t kNone = 0xffffffffu;
constexpr unsigned long long kNoEdge = ~0ull;
constexpr unsigned long long kFlipBit = 1ull << 63;

using prim::fold_min;  // one atomicMin per wave and label

struct Stats {
  int rounds = 0;
  int jumps[40] = {};
};
thread_local Stats tls_stats;

__device__ __forceinline__ double dot3(const double* __restrict__ nrm, uint32_t i, uint32_t j) {
  const double* a = nrm + 3 * static_cast<int64_t>(i);
  const double* b = nrm + 3 * static_cast<int64_t>(j);
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ unsigned long long weight_bits(double dot) {
  const double w = 1.0 - fabs(dot);
  return static_cast<unsigned long long>(__double_as_longlong(w > 0.0 ? w : 0.0));
}

// z + 0.0 (so -0.0 ties with 0.0) as bits that order like the doubles
__device__ __forceinline__ unsigned long long z_bits(double z) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(z + 0.0));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__global__ __launch_bounds__(kT) void k_ort_init(int64_t n, uint32_t* word, uint8_t* alive, uint32_t* tslot) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n) return;
  word[v] = static_cast<uint32_t>(v) << 1;
  alive[v] = 1;
  tslot[v] = kNone;
}

// Every slot's key: the weight's bits | the flip bit, or kNoEdge (beyond cnt, an
// index outside [0, n), or the point itself).
__global__ __launch_bounds__(kT) void k_ort_keys(const double* __restrict__ nrm, int64_t n,
                                                 const int32_t* __restrict__ idx, const int32_t* __restrict__ cnt,
                                                 uint32_t k, uint64_t total, unsigned long long* __restrict__ wkey) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * kT + threadIdx.x;
  if (s >= total) return;
  const uint32_t i = static_cast<uint32_t>(s) / k;
  const uint32_t jj = static_cast<uint32_t>(s) - i * k;
  unsigned long long key = kNoEdge;
  if (static_cast<int64_t>(jj) < static_cast<int64_t>(cnt[i])) {
    const int32_t j = idx[s];
    if (j >= 0 && j < n && static_cast<uint32_t>(j) != i) {
      const double dot = dot3(nrm, i, static_cast<uint32_t>(j));
      key = weight_bits(dot) | (dot < 0.0 ? kFlipBit : 0ull);
    }
  }
  wkey[s] = key;
}

// PASS 1: cw[label] = the smallest weight of the component's candidates, and the
// rows that still have a candidate -> alive_next.  PASS 2: cs[label] = the
// smallest slot among the candidates whose weight equals cw[label].
template <int PASS>
__global__ __launch_bounds__(kT) void k_ort_scan(const unsigned long long* __restrict__ wkey,
                                                 const int32_t* __restrict__ idx, uint32_t k, uint64_t total,
                                                 const uint32_t* __restrict__ word,
                                                 const uint8_t* __restrict__ alive, uint8_t* alive_next,
                                                 unsigned long long* cw, uint32_t* cs) {
  const uint64_t s = static_cast<uint64_t>(blockIdx.x) * kT + threadIdx.x;
  bool cand = false;
  uint32_t la = 0, lb = 0;
  unsigned long long wb = 0;
  if (s < total) {
    const uint32_t i = static_cast<uint32_t>(s) / k;
    if (alive[i]) {
      const unsigned long long key = wkey[s];
      if (key != kNoEdge) {  // so idx[s] is a point other than i
        la = word[i] >> 1;
        lb = word[idx[s]] >> 1;
        if (la != lb) {
          cand = true;
          wb = key & ~kFlipBit;
          if (PASS == 1) alive_next[i] = 1;
        }
      }
    }
  }
  if (PASS == 1) {
    fold_min(cw, la, wb, cand);
    fold_min(cw, lb, wb, cand);
  } else {
    fold_min(cs, la, static_cast<uint32_t>(s), cand && cw[la] == wb);
    fold_min(cs, lb, static_cast<uint32_t>(s), cand && cw[lb] == wb);
  }
}

// word: the labels of the round's start (read only); out: the same with the
// hooked representatives re-parented.
__global__ __launch_bounds__(kT) void k_ort_hook(const unsigned long long* __restrict__ wkey, int64_t n,
                                                 const int32_t* __restrict__ idx, uint32_t k,
                                                 const uint32_t* __restrict__ word, const uint32_t* __restrict__ cs,
                                                 uint32_t* __restrict__ out, uint32_t* __restrict__ tslot,
                                                 unsigned* hooks) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n) return;
  const uint32_t me = static_cast<uint32_t>(v);
  uint32_t w = word[v];
  if ((w >> 1) == me) {
    const uint32_t s = cs[v];
    if (s != kNone) {
      const uint32_t i = s / k, j = static_cast<uint32_t>(idx[s]);
      const uint32_t wi = word[i], wj = word[j];
      const uint32_t other = (wi >> 1) == me ? (wj >> 1) : (wi >> 1);
      if (!(cs[other] == s && me < other)) {
        const uint32_t flip = static_cast<uint32_t>(wkey[s] >> 63);
        w = (other << 1) | ((wi ^ wj ^ flip) & 1u);
        tslot[v] = s;
        atomicAdd(hooks, 1u);
      }
    }
  }
  out[v] = w;
}

// One jump, in place.  word is read and written by other workgroups in this
// launch: see (c, d) above for why a stale read is harmless.
__global__ __launch_bounds__(kT) void k_ort_jump(int64_t n, uint32_t* word, unsigned* changed) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n) return;
  const uint32_t w = word[v], a = w >> 1;
  if (a == static_cast<uint32_t>(v)) return;
  const uint32_t wa = word[a];
  if ((wa >> 1) == a) return;  // the parent is a root
  word[v] = (wa & ~1u) | ((w ^ wa) & 1u);
  *changed = 1u;
}

// STEP 1: cz[label] = min of ~z_bits (the largest z).  STEP 2: ci[label] = the
// lowest index among the points of that z.
template <int STEP>
__global__ __launch_bounds__(kT) void k_ort_root(const double* __restrict__ xyz, int64_t n,
                                                 const uint32_t* __restrict__ word, unsigned long long* cz,
                                                 uint32_t* ci) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  const bool in = v < n;
  const uint32_t l = in ? word[v] >> 1 : 0u;
  const unsigned long long zb = in ? ~z_bits(xyz[3 * v + 2]) : 0ull;
  if (STEP == 1)
    fold_min(cz, l, zb, in);
  else
    fold_min(ci, l, static_cast<uint32_t>(v), in && cz[l] == zb);
}

// per representative: whether its component is negated as a whole, relative to
// the representative's own sign
__global__ __launch_bounds__(kT) void k_ort_sign(const double* __restrict__ nrm, int64_t n,
                                                 const uint32_t* __restrict__ word, const uint32_t* __restrict__ ci,
                                                 uint8_t* __restrict__ cflip, unsigned* comps) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n || (word[v] >> 1) != static_cast<uint32_t>(v)) return;
  const uint32_t r = ci[v];
  cflip[v] = static_cast<uint8_t>((word[r] & 1u) ^ (nrm[3 * static_cast<int64_t>(r) + 2] < 0.0 ? 1u : 0u));
  atomicAdd(comps, 1u);
}

__global__ __launch_bounds__(kT) void k_ort_apply(double* __restrict__ nrm, int64_t n,
                                                  const uint32_t* __restrict__ word,
                                                  const uint8_t* __restrict__ cflip) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v >= n) return;
  const uint32_t w = word[v];
  if (((w & 1u) ^ cflip[w >> 1]) == 0u) return;
  nrm[3 * v] = -nrm[3 * v];
  nrm[3 * v + 1] = -nrm[3 * v + 1];
  nrm[3 * v + 2] = -nrm[3 * v + 2];
}

__global__ __launch_bounds__(kT) void k_ort_tree_flag(const uint32_t* __restrict__ tslot, int64_t n,
                                                      uint32_t* __restrict__ flag) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x;
  if (v < n) flag[v] = tslot[v] != kNone ? 1u : 0u;
}

int read_u32(sl_ctx* c, const unsigned* dev, unsigned* host, hipStream_t s) {
  MTRY(c, hipMemcpyAsync(host, dev, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  MTRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

}  // namespace ort
}  // namespace

extern "C" {

int sl_orient_normals_mst(sl_ctx* c, const double* xyz, double* normals, int64_t n, const int32_t* idx,
                          const int32_t* cnt, int k, uint32_t* tree_slots, int64_t* n_tree, int64_t* n_components,
                          void* stream) {
  using namespace ort;
  if (!c) return SL_EINVAL;
  if (n < 0 || k < 1 || !n_tree || !n_components || (n && (!xyz || !normals || !idx || !cnt)))
    return slgpu_fail(c, SL_EINVAL, "sl_orient_normals_mst: bad sizes or NULL arguments");
  if (n >= (1ll << 31)) return slgpu_fail(c, SL_EINVAL, "at most 2^31 - 1 points");
  if (static_cast<uint64_t>(n) * static_cast<uint64_t>(k) >= (1ull << 32))
    return slgpu_fail(c, SL_EINVAL, "sl_orient_normals_mst: n * k must be below 2^32");
  *n_tree = *n_components = 0;
  tls_stats = Stats();
  if (n == 0) return SL_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  PoolStream pool_stream(s);
  MTRY(c, hipSetDevice(slgpu_device(c)));

  int bound = 2;  // ceil(log2 n) + 2
  while ((int64_t{1} << (bound - 2)) < n) ++bound;
  const uint64_t total = static_cast<uint64_t>(n) * static_cast<uint64_t>(k);
  const unsigned gv = blocks(n), gs = static_cast<unsigned>((total + kT - 1) / kT);
  const uint32_t uk = static_cast<uint32_t>(k);

  DBuf<uint32_t> wa, wb, cs, tslot;
  DBuf<unsigned long long> cw, wkey;
  DBuf<uint8_t> al0, al1;
  DBuf<unsigned> ctr;  // [0]: components, [1 + r]: hooks of round r, then one flag per jump
  const int n_ctr = 1 + bound + bound * bound;
  MTRY(c, wa.alloc(n));
  MTRY(c, wb.alloc(n));
  MTRY(c, cs.alloc(n));
  MTRY(c, tslot.alloc(n));
  MTRY(c, cw.alloc(n));
  MTRY(c, wkey.alloc(static_cast<int64_t>(total)));
  MTRY(c, al0.alloc(n));
  MTRY(c, al1.alloc(n));
  MTRY(c, ctr.alloc(n_ctr));
  MTRY(c, hipMemsetAsync(ctr.p, 0, sizeof(unsigned) * n_ctr, s));
  uint32_t *word = wa.p, *next = wb.p;
  uint8_t *alive = al0.p, *alive_next = al1.p;
  hipLaunchKernelGGL(k_ort_init, dim3(gv), dim3(kT), 0, s, n, word, alive, tslot.p);
  hipLaunchKernelGGL(k_ort_keys, dim3(gs), dim3(kT), 0, s, normals, n, idx, cnt, uk, total, wkey.p);
  MTRY(c, hipGetLastError());

  int64_t hooked = 0;
  int round = 0;
  for (;; ++round) {
    if (hooked == n - 1) break;  // one spanning tree
    if (round == bound)
      return slgpu_fail(c, SL_EHIP, "sl_orient_normals_mst: internal error: the round bound was exceeded");
    MTRY(c, hipMemsetAsync(cw.p, 0xff, sizeof(unsigned long long) * n, s));
    MTRY(c, hipMemsetAsync(cs.p, 0xff, sizeof(uint32_t) * n, s));
    MTRY(c, hipMemsetAsync(alive_next, 0, static_cast<size_t>(n), s));
    hipLaunchKernelGGL(k_ort_scan<1>, dim3(gs), dim3(kT), 0, s, wkey.p, idx, uk, total, word, alive, alive_next,
                       cw.p, cs.p);
    hipLaunchKernelGGL(k_ort_scan<2>, dim3(gs), dim3(kT), 0, s, wkey.p, idx, uk, total, word, alive, alive_next,
                       cw.p, cs.p);
    unsigned* hooks = ctr.p + 1 + round;
    hipLaunchKernelGGL(k_ort_hook, dim3(gv), dim3(kT), 0, s, wkey.p, n, idx, uk, word, cs.p, next, tslot.p, hooks);
    MTRY(c, hipGetLastError());
    unsigned h = 0;
    int r = read_u32(c, hooks, &h, s);
    if (r) return r;
    if (h == 0) break;  // no component has a candidate: `word` already is the result
    hooked += h;
    std::swap(word, next);
    std::swap(alive, alive_next);
    int step = 0;
    for (;; ++step) {
      if (step == bound)
        return slgpu_fail(c, SL_EHIP, "sl_orient_normals_mst: internal error: the jump bound was exceeded");
      unsigned* changed = ctr.p + 1 + bound + round * bound + step;
      hipLaunchKernelGGL(k_ort_jump, dim3(gv), dim3(kT), 0, s, n, word, changed);
      MTRY(c, hipGetLastError());
      unsigned ch = 0;
      r = read_u32(c, changed, &ch, s);
      if (r) return r;
      if (!ch) break;
    }
    if (round < 40) tls_stats.jumps[round] = step + 1;  // launches, the one that changed nothing included
    tls_stats.rounds = round + 1;
  }

  // roots, component signs, the normals; cw / cs / alive_next are free again
  MTRY(c, hipMemsetAsync(cw.p, 0xff, sizeof(unsigned long long) * n, s));
  MTRY(c, hipMemsetAsync(cs.p, 0xff, sizeof(uint32_t) * n, s));
  hipLaunchKernelGGL(k_ort_root<1>, dim3(gv), dim3(kT), 0, s, xyz, n, word, cw.p, cs.p);
  hipLaunchKernelGGL(k_ort_root<2>, dim3(gv), dim3(kT), 0, s, xyz, n, word, cw.p, cs.p);
  hipLaunchKernelGGL(k_ort_sign, dim3(gv), dim3(kT), 0, s, normals, n, word, cs.p, alive_next, ctr.p);
  hipLaunchKernelGGL(k_ort_apply, dim3(gv), dim3(kT), 0, s, normals, n, word, alive_next);
  MTRY(c, hipGetLastError());
  unsigned comps = 0;
  int r = read_u32(c, ctr.p, &comps, s);
  if (r) return r;
  if (static_cast<int64_t>(comps) + hooked != n)
    return slgpu_fail(c, SL_EHIP, "sl_orient_normals_mst: internal error: components and tree edges do not add up");
  if (tree_slots && hooked) {
    int64_t t = 0;
    hipLaunchKernelGGL(k_ort_tree_flag, dim3(gv), dim3(kT), 0, s, tslot.p, n, next);
    MTRY(c, hipGetLastError());
    r = scan_flags(c, next, n, cs.p, &t, s);
    if (r) return r;
    if (t != hooked)
      return slgpu_fail(c, SL_EHIP, "sl_orient_normals_mst: internal error: the tree list is incomplete");
    // (the scan's total is `hooked`, so every flagged row's position is below it: tree_slots' size)
    hipLaunchKernelGGL((k_compact_rows<uint32_t, 1>), dim3(gv), dim3(kT), 0, s, tslot.p, n, next, cs.p, tree_slots);
    MTRY(c, hipGetLastError());
    MTRY(c, hipStreamSynchronize(s));
  }
  *n_tree = hooked;
  *n_components = comps;
  return SL_OK;
}

int sl_orient_normals_mst_stats(int* rounds, int* jumps, int capacity) {
  using namespace ort;
  if (!rounds || capacity < 0 || (capacity && !jumps)) return SL_EINVAL;
  *rounds = tls_stats.rounds;
  for (int i = 0; i < capacity; ++i) jumps[i] = i < 40 ? tls_stats.jumps[i] : 0;
  return SL_OK;
}

}  // extern "C"
