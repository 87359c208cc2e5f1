// csrc/slrecord.h's put_record_at, the mesh writers' record packer, checked on the host alone: this program is built
// by a plain C++ compiler with the address and undefined-behaviour sanitizers (tests/test_host_record.py).  For the
// 13-byte PLY face and the 51-byte coloured PLY vertex it packs n records into an image that was filled with a canary,
// once in ascending and once in descending record order, and requires the byte-wise concatenation of the records and
// an untouched canary after them both times: a store that spills into a neighbour's bytes is overwritten by the
// neighbour in one order and survives in the other.  Exit status 0: every check held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "slrecord.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      ++failures;                                     \
      printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                            \
      printf("\n");                                   \
    }                                                 \
  } while (0)

constexpr unsigned char kCanary = 0xA5;
constexpr int kSlack = 64;  // canary bytes after the last record

// The face record of triangle r, field by field: the byte 3, then a b c, whose four bytes all differ.
void face_record(int r, unsigned char* rec) {
  const uint32_t a = 0x04030201u + 0x01010101u * static_cast<uint32_t>(r % 50), b = a ^ 0xf0e0d0c0u, c = ~a;
  rec[0] = 3;
  memcpy(rec + 1, &a, 4);
  memcpy(rec + 5, &b, 4);
  memcpy(rec + 9, &c, 4);
  // the dwords k_mw_pack_faces builds are these bytes
  const uint32_t w[4] = {3u | (a << 8), (a >> 24) | (b << 8), (b >> 24) | (c << 8), c >> 24};
  unsigned char as_bytes[16];
  memcpy(as_bytes, w, 16);
  CHECK(memcmp(as_bytes, rec, 13) == 0, "face %d: the shifted dwords are not the record", r);
}

// The coloured vertex record of vertex r: x y z nx ny nz, then red green blue.
void vertex_record(int r, unsigned char* rec) {
  for (int k = 0; k < 6; ++k) {
    const double v = (k < 3 ? 1.0e3 : -1.0) / (7.0 * r + k + 1.0);  // every byte of the mantissa in use
    memcpy(rec + 8 * k, &v, 8);
  }
  for (int k = 0; k < 3; ++k) rec[48 + k] = static_cast<unsigned char>(37 * r + 85 * k + 1);
}

template <int REC>
void check(int n, void (*record)(int, unsigned char*)) {
  constexpr int kWords = (REC + 3) / 4 + 1;
  std::vector<unsigned char> want(static_cast<size_t>(n) * REC);
  for (int r = 0; r < n; ++r) record(r, want.data() + static_cast<size_t>(r) * REC);
  const size_t size = (want.size() + kSlack + 15) / 16 * 16;
  for (int descending = 0; descending < 2; ++descending) {
    // allocated storage of its own: the sanitizer sees a store past `size`, the canary one past the records
    unsigned char* img = static_cast<unsigned char*>(aligned_alloc(16, size));
    memset(img, kCanary, size);
    for (int j = 0; j < n; ++j) {
      const int r = descending ? n - 1 - j : j;
      uint32_t w[kWords] = {};
      memcpy(w, want.data() + static_cast<size_t>(r) * REC, REC);
      slrecord::put_record_at<REC>(img, r, w);
    }
    size_t bad = 0;
    while (bad < want.size() && img[bad] == want[bad]) ++bad;
    CHECK(bad == want.size(), "REC %d, %d records, %s: byte %zu (record %zu, byte %zu of it) is %02x, not %02x", REC, n,
          descending ? "descending" : "ascending", bad, bad / REC, bad % REC, img[bad], want[bad]);
    size_t at = want.size();
    while (at < size && img[at] == kCanary) ++at;
    CHECK(at == size, "REC %d, %d records, %s: byte %zu past the last record was written", REC, n,
          descending ? "descending" : "ascending", at - want.size());
    free(img);
  }
}

}  // namespace

int main() {
  const int counts[] = {1, 2, 3, 4, 5, 16, 17, 255, 256};
  for (int n : counts) {
    check<13>(n, face_record);
    check<51>(n, vertex_record);
  }
  printf("put_record_at: %d failed checks\n", failures);
  return failures ? 1 : 0;
}
