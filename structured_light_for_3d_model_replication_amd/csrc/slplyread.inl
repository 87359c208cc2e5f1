// ------------------------------------------------------------- PLY reader ----
// The body of a vertex-only PLY parsed on the device into a table
// f64 [n_vertex][n_properties] (sl_parse_ply_ascii, sl_unpack_ply_binary):
// the reading half of the k_ply_* writer above, included from slgpu.hip.
//
// ASCII.  The body is a white-space separated token stream (as rply reads
// it; white space: ' ' \t \r \n).  A byte starts a token when it is no white
// space and the byte before it is (or it is the body's first byte).
//   k_plyr_count    16 bytes per thread in one load, kPlyrChunk bytes per
//                   workgroup: the token starts of the chunk, and whether a
//                   byte is outside the alphabet 0-9 + - . e E and white space
//   k_ply_scan      (the writer's) each chunk's first token number, the total
//   k_plyr_offsets  every token's byte offset at its number; a token starts a
//                   line when a line break lies in the white space before it,
//                   and with n_rows x n_cols tokens every non-blank line holds
//                   n_cols of them exactly when token t starts a line <=>
//                   t % n_cols == 0 -- checked here, nothing is stored
//   k_plyr_parse    one thread per token
// Grammar: [+-]? digits [. digits]? ([eE] [+-]? digits)?, a digit at least in
// the mantissa ("5." and ".5" are inside).  The decimal significand M (leading
// zeros drop out by themselves) and the net power of ten p give the value
// +-M * 10^p.  M never wraps: a digit that would take it past 2^53 marks the
// token undecided instead.
// Exact tier (Clinger): M <= 2^53 and |p| <= 22.  double(M) and 10^|p| are
// both exact binary64 numbers, so double(M) / 10^|p| (p < 0), double(M) * 10^p
// (p > 0) or double(M) is ONE correctly rounded IEEE operation on exact
// operands: the correctly rounded value of the token, what strtod and Python's
// float() return.  (Never M * (1 / 10^|p|): two roundings, wrong by one ulp on
// more than a quarter of the %.4f tokens of a cloud.)  The sign goes on last:
// "-0.0000" is -0.0.
// Undecided tokens (inside the grammar, outside the tier) are appended as
// (token number, byte offset, length) through an atomic counter; the host
// converts exactly those with strtod and patches the table.  The entries carry
// their token number: the append order does not matter.
// Everything else -- a byte outside the alphabet ("nan", "inf", '#'), a token
// outside the grammar, a token count other than n_rows x n_cols, a non-blank
// line without exactly n_cols tokens, an undecided list that overflows -- is
// a status code: the caller reads that file on the host.
//
// All byte and token numbers are int64 (a 4K view's body passes 2^28 bytes, a
// merged cloud's 2^31).
namespace {

constexpr int kPlyrChunk = kPlyBlock * 16;  // bytes per workgroup: one 16-byte load per thread
constexpr int kPlyrRunMax = 1 << 16;        // the longest run of blanks looked through for a line break
constexpr uint64_t kPlyrTwo53 = 1ull << 53;

// status bits in state[0] (atomicOr); state[2..3]: the undecided counter (64 bit)
constexpr unsigned kPlyrBadByte = 1u, kPlyrBadToken = 2u, kPlyrRagged = 4u;

__device__ const double kPlyrPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                          1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

__device__ __forceinline__ bool plyr_ws(unsigned c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }
__device__ __forceinline__ bool plyr_digit(unsigned c) { return c - '0' < 10u; }
__device__ __forceinline__ bool plyr_tokc(unsigned c) {
  return plyr_digit(c) || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E';
}

// The 16 bytes at `base` (16-byte aligned; past n_bytes: blanks): bit j of the
// result is set when byte base + j starts a token; *bad: a byte outside the
// alphabet.
__device__ inline unsigned plyr_starts(const uint8_t* body, int64_t n_bytes, int64_t base, bool* bad) {
  *bad = false;
  if (base >= n_bytes) return 0u;
  uint8_t b[16];
  if (base + 16 <= n_bytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(body + base);
    memcpy(b, &v, 16);
  } else {
    const int m = static_cast<int>(n_bytes - base);
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = j < m ? body[base + j] : static_cast<uint8_t>(' ');
  }
  bool pw = base == 0 || plyr_ws(body[base - 1]);
  unsigned mask = 0u;
  bool any_bad = false;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned ch = b[j];
    const bool w = plyr_ws(ch);
    any_bad |= !w && !plyr_tokc(ch);
    if (!w && pw) mask |= 1u << j;
    pw = w;
  }
  *bad = any_bad;
  return mask;
}

__global__ __launch_bounds__(kPlyBlock) void k_plyr_count(const uint8_t* body, int64_t n_bytes, unsigned* bsum,
                                                           unsigned* state) {
  __shared__ unsigned s_w[kPlyBlock / 64];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kPlyrChunk + static_cast<int64_t>(threadIdx.x) * 16;
  bool bad;
  const unsigned mask = plyr_starts(body, n_bytes, base, &bad);
  if (bad) atomicOr(state, kPlyrBadByte);
  unsigned total;
  (void)ply_block_scan(static_cast<unsigned>(__popc(mask)), s_w, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kPlyBlock) void k_plyr_offsets(const uint8_t* body, int64_t n_bytes,
                                                             const int64_t* boff, int64_t n_tok, int n_cols,
                                                             int64_t* tok_off, unsigned* state) {
  __shared__ unsigned s_w[kPlyBlock / 64];
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kPlyrChunk + static_cast<int64_t>(threadIdx.x) * 16;
  bool bad;
  unsigned mask = plyr_starts(body, n_bytes, base, &bad);
  const unsigned cnt = static_cast<unsigned>(__popc(mask));
  unsigned total;
  const unsigned incl = ply_block_scan(cnt, s_w, &total);
  int64_t t = boff[blockIdx.x] + (incl - cnt);
  while (mask) {
    const int j = __ffs(mask) - 1;
    mask &= mask - 1u;
    const int64_t pos = base + j;
    // a line break in the white space before the token (the body's first token starts a line)
    bool line_start = true, known = true;
    int64_t k = pos - 1;
    for (int steps = 0; k >= 0; --k, ++steps) {
      const unsigned ch = body[k];
      if (ch == '\n' || ch == '\r') break;
      if (!(ch == ' ' || ch == '\t')) {
        line_start = false;
        break;
      }
      if (steps >= kPlyrRunMax) {  // not looked through: the host reads such a file
        known = false;
        break;
      }
    }
    if (t < n_tok) {
      tok_off[t] = pos;
      if (!known || line_start != (t % n_cols == 0)) atomicOr(state, kPlyrRagged);
    }
    ++t;
  }
}

__global__ __launch_bounds__(256) void k_plyr_parse(const uint8_t* body, int64_t n_bytes, const int64_t* tok_off,
                                                     int64_t n_tok, double* table, int64_t* und, int64_t und_cap,
                                                     unsigned* state) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= n_tok) return;
  const int64_t s = tok_off[t];
  int64_t i = s;
  auto at = [&](int64_t q) -> unsigned { return q < n_bytes ? body[q] : static_cast<unsigned>(' '); };
  unsigned ch = at(i);
  bool neg = false;
  if (ch == '+' || ch == '-') {
    neg = ch == '-';
    ch = at(++i);
  }
  uint64_t M = 0;
  int64_t frac = 0;  // digits of M behind the point
  bool any = false, big = false, ok = true;
  while (plyr_digit(ch)) {
    const unsigned d = ch - '0';
    any = true;
    if (!big) {
      if (M > (kPlyrTwo53 - d) / 10u) big = true;  // M * 10 + d would pass 2^53
      else M = M * 10u + d;
    }
    ch = at(++i);
  }
  if (ch == '.') {
    ch = at(++i);
    while (plyr_digit(ch)) {
      const unsigned d = ch - '0';
      any = true;
      if (!big) {
        if (M > (kPlyrTwo53 - d) / 10u) {
          big = true;
        } else {
          M = M * 10u + d;
          ++frac;
        }
      }
      ch = at(++i);
    }
  }
  ok = any;
  int64_t ex = 0;
  if (ok && (ch == 'e' || ch == 'E')) {
    ch = at(++i);
    bool eneg = false;
    if (ch == '+' || ch == '-') {
      eneg = ch == '-';
      ch = at(++i);
    }
    ok = plyr_digit(ch);
    while (plyr_digit(ch)) {
      if (ex < 1000000) ex = ex * 10 + (ch - '0');  // saturates far outside the tier
      ch = at(++i);
    }
    if (eneg) ex = -ex;
  }
  if (!ok || !plyr_ws(ch)) {  // "1e", "1.2.3", "-", "e5": outside the grammar
    atomicOr(state, kPlyrBadToken);
    return;
  }
  const int64_t p = ex - frac;
  if (!big && p >= -22 && p <= 22) {
    double v = static_cast<double>(M);  // exact: M <= 2^53
    if (p < 0) v = v / kPlyrPow10[-p];
    else if (p > 0) v = v * kPlyrPow10[p];
    table[t] = neg ? -v : v;
    return;
  }
  table[t] = 0.0;
  const unsigned long long slot = atomicAdd(reinterpret_cast<unsigned long long*>(state + 2), 1ull);
  if (static_cast<int64_t>(slot) < und_cap) {
    und[3 * slot] = t;
    und[3 * slot + 1] = s;
    und[3 * slot + 2] = i - s;
  }
}

__global__ __launch_bounds__(256) void k_plyr_patch(double* table, const int64_t* und, const double* val, int64_t k) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e < k) table[und[3 * e]] = val[e];
}

// Binary records: element (row, col) read bytewise at row * stride +
// off[col] (fields are unaligned) and widened to f64.  cols: off[n_cols],
// then type[n_cols] (SL_PLY_*).
__global__ __launch_bounds__(256) void k_plyr_unpack(const uint8_t* body, int64_t n_rows, int64_t stride, int n_cols,
                                                      const int* cols, double* table) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= n_rows * n_cols) return;
  const int64_t row = e / n_cols;
  const int col = static_cast<int>(e - row * n_cols);
  const uint8_t* p = body + row * stride + cols[col];
  uint64_t raw = 0;  // little endian
  const int type = cols[n_cols + col];
  const int size = type == SL_PLY_F64 ? 8 : (type == SL_PLY_F32 || type == SL_PLY_I32 || type == SL_PLY_U32) ? 4
                   : (type == SL_PLY_I16 || type == SL_PLY_U16) ? 2 : 1;
  for (int b = 0; b < size; ++b) raw |= static_cast<uint64_t>(p[b]) << (8 * b);
  double v;
  switch (type) {
    case SL_PLY_F64: v = __builtin_bit_cast(double, raw); break;
    case SL_PLY_F32: v = static_cast<double>(__builtin_bit_cast(float, static_cast<uint32_t>(raw))); break;
    case SL_PLY_I8: v = static_cast<double>(static_cast<int8_t>(raw)); break;
    case SL_PLY_I16: v = static_cast<double>(static_cast<int16_t>(raw)); break;
    case SL_PLY_I32: v = static_cast<double>(static_cast<int32_t>(raw)); break;
    default: v = static_cast<double>(raw); break;  // U8, U16, U32
  }
  table[e] = v;
}

int plyr_type_size(int type) {
  switch (type) {
    case SL_PLY_F64: return 8;
    case SL_PLY_F32: case SL_PLY_I32: case SL_PLY_U32: return 4;
    case SL_PLY_I16: case SL_PLY_U16: return 2;
    case SL_PLY_U8: case SL_PLY_I8: return 1;
    default: return 0;
  }
}

}  // namespace

extern "C" {

int sl_parse_ply_ascii(sl_ctx* c, const uint8_t* body_dev, int64_t n_bytes, int64_t n_rows, int n_cols,
                       double* table_dev, int64_t* undecided_dev, int64_t undecided_cap, int64_t* n_undecided,
                       int* status, void* stream) {
  if (!c) return SL_EINVAL;
  if (!status || !n_undecided || n_bytes < 0 || n_rows < 0 || n_cols < 1 || undecided_cap < 0 ||
      (n_bytes > 0 && !body_dev) || (undecided_cap > 0 && !undecided_dev) || n_rows > INT64_MAX / n_cols ||
      (n_rows > 0 && !table_dev))
    return fail(c, SL_EINVAL, "sl_parse_ply_ascii: bad arguments");
  if (reinterpret_cast<uintptr_t>(body_dev) % 16)
    return fail(c, SL_EINVAL, "sl_parse_ply_ascii: body_dev must be 16-byte aligned");
  *status = SL_PLY_ACCEPTED;
  *n_undecided = 0;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n_tok = n_rows * n_cols;
  const int64_t nb = (n_bytes + kPlyrChunk - 1) / kPlyrChunk;
  if (nb > INT32_MAX) return fail(c, SL_EINVAL, "sl_parse_ply_ascii: body too large");
  if (nb == 0) {  // no bytes, no tokens
    if (n_tok) *status = SL_PLY_TOKEN_COUNT;
    return SL_OK;
  }
  int r = grow(c, &c->d_ply_bsum, &c->cap_ply_bsum, nb + 1, s, true);
  if (r) return r;
  r = grow(c, &c->d_ply_boff, &c->cap_ply_boff, nb + 1, s, true);
  if (r) return r;
  r = grow(c, &c->d_plyr_state, &c->cap_plyr_state, 4, s, true);
  if (r) return r;
  r = zero_async(c, c->d_plyr_state, 4, s);
  if (r) return r;
  hipLaunchKernelGGL(k_plyr_count, dim3(static_cast<unsigned>(nb)), dim3(kPlyBlock), 0, s, body_dev, n_bytes,
                     c->d_ply_bsum, c->d_plyr_state);
  hipLaunchKernelGGL(k_ply_scan, dim3(1), dim3(1024), 0, s, c->d_ply_bsum, nb, c->d_ply_boff);
  HIP_TRY(c, hipGetLastError());
  int64_t total = 0;
  unsigned st[4] = {0, 0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(&total, c->d_ply_boff + nb, sizeof(total), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(st, c->d_plyr_state, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (st[0] & kPlyrBadByte) {
    *status = SL_PLY_BAD_BYTE;
    return SL_OK;
  }
  if (total != n_tok) {
    *status = SL_PLY_TOKEN_COUNT;
    return SL_OK;
  }
  if (n_tok == 0) return SL_OK;
  r = grow(c, &c->d_plyr_tok, &c->cap_plyr_tok, n_tok, s, true);
  if (r) return r;
  hipLaunchKernelGGL(k_plyr_offsets, dim3(static_cast<unsigned>(nb)), dim3(kPlyBlock), 0, s, body_dev, n_bytes,
                     c->d_ply_boff, n_tok, n_cols, c->d_plyr_tok, c->d_plyr_state);
  const int64_t pb = (n_tok + 255) / 256;
  if (pb > INT32_MAX) return fail(c, SL_EINVAL, "sl_parse_ply_ascii: too many tokens");
  hipLaunchKernelGGL(k_plyr_parse, dim3(static_cast<unsigned>(pb)), dim3(256), 0, s, body_dev, n_bytes,
                     c->d_plyr_tok, n_tok, table_dev, undecided_dev, undecided_cap, c->d_plyr_state);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(st, c->d_plyr_state, sizeof(st), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  uint64_t n_und;
  memcpy(&n_und, st + 2, sizeof(n_und));
  if (st[0] & kPlyrBadToken) {
    *status = SL_PLY_BAD_TOKEN;
    return SL_OK;
  }
  if (st[0] & kPlyrRagged) {
    *status = SL_PLY_RAGGED_LINE;
    return SL_OK;
  }
  *n_undecided = static_cast<int64_t>(n_und);
  if (static_cast<int64_t>(n_und) > undecided_cap) {
    *status = SL_PLY_UNDECIDED_OVERFLOW;
    return SL_OK;
  }
  if (n_und == 0) return SL_OK;
  // the undecided tokens through strtod: their bytes back in runs of
  // neighbouring tokens, the values into the table at their token numbers
  const int64_t k = static_cast<int64_t>(n_und);
  std::vector<int64_t> und(static_cast<size_t>(3 * k));
  HIP_TRY(c, hipMemcpyAsync(und.data(), undecided_dev, und.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  std::vector<int64_t> order(static_cast<size_t>(k));
  for (int64_t e = 0; e < k; ++e) {
    order[e] = e;
    const int64_t off = und[3 * e + 1], len = und[3 * e + 2];
    if (und[3 * e] < 0 || und[3 * e] >= n_tok || off < 0 || len < 1 || off > n_bytes - len)
      return fail(c, SL_EHIP, "sl_parse_ply_ascii: corrupt undecided list");
  }
  std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return und[3 * a + 1] < und[3 * b + 1]; });
  std::vector<double> val(static_cast<size_t>(k));
  std::vector<char> run;
  std::string tok;
  for (int64_t a = 0; a < k;) {
    const int64_t lo = und[3 * order[a] + 1];
    int64_t hi = lo + und[3 * order[a] + 2], b = a + 1;
    while (b < k && und[3 * order[b] + 1] - hi < 4096 && und[3 * order[b] + 1] + und[3 * order[b] + 2] - lo < (1 << 24)) {
      hi = std::max(hi, und[3 * order[b] + 1] + und[3 * order[b] + 2]);
      ++b;
    }
    run.resize(static_cast<size_t>(hi - lo));
    HIP_TRY(c, hipMemcpyAsync(run.data(), body_dev + lo, run.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    for (; a < b; ++a) {
      const int64_t e = order[a];
      tok.assign(run.data() + (und[3 * e + 1] - lo), static_cast<size_t>(und[3 * e + 2]));
      val[e] = strtod(tok.c_str(), nullptr);
    }
  }
  r = grow(c, &c->d_plyr_val, &c->cap_plyr_val, k, s, true);
  if (r) return r;
  HIP_TRY(c, hipMemcpyAsync(c->d_plyr_val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_plyr_patch, dim3(static_cast<unsigned>((k + 255) / 256)), dim3(256), 0, s, table_dev,
                     undecided_dev, c->d_plyr_val, k);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(s));
  return SL_OK;
}

int sl_unpack_ply_binary(sl_ctx* c, const uint8_t* body_dev, int64_t n_rows, int64_t stride, int n_cols,
                         const int* col_offset, const int* col_type, double* table_dev, void* stream) {
  if (!c) return SL_EINVAL;
  if (n_rows < 0 || stride < 1 || n_cols < 1 || !col_offset || !col_type || n_rows > INT64_MAX / stride ||
      n_rows > INT64_MAX / n_cols || (n_rows > 0 && (!body_dev || !table_dev)))
    return fail(c, SL_EINVAL, "sl_unpack_ply_binary: bad arguments");
  std::vector<int> cols(static_cast<size_t>(2 * n_cols));
  for (int j = 0; j < n_cols; ++j) {
    const int size = plyr_type_size(col_type[j]);
    if (!size || col_offset[j] < 0 || col_offset[j] > stride - size)
      return fail(c, SL_EINVAL, "sl_unpack_ply_binary: a property lies outside the record or has no known type");
    cols[j] = col_offset[j];
    cols[n_cols + j] = col_type[j];
  }
  if (n_rows == 0) return SL_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t blocks = (n_rows * n_cols + 255) / 256;
  if (blocks > INT32_MAX) return fail(c, SL_EINVAL, "sl_unpack_ply_binary: table too large");
  int r = grow(c, &c->d_plyr_cols, &c->cap_plyr_cols, 2 * n_cols, s, true);
  if (r) return r;
  HIP_TRY(c, hipMemcpyAsync(c->d_plyr_cols, cols.data(), cols.size() * sizeof(int), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_plyr_unpack, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, body_dev, n_rows, stride,
                     n_cols, c->d_plyr_cols, table_dev);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(s));  // cols (host) was read by the copy; the table is ready
  return SL_OK;
}

}  // extern "C"
