// libslgpu.so -- one record whose length is no multiple of 4 into an image of packed records, without touching a
// neighbour's bytes: the mesh writers' LDS packer (slmeshwrite.inl states who takes which record and why the
// dword stores meet no bank conflict).  The record is held as dwords, w[(REC + 3) / 4 + 1]: its bytes in memory
// order and one padding dword past them, so that a read of the four bytes from any byte of the record stays in w.
// Record r starts at byte REC r of the image, i.e. HEAD = (4 - REC r) mod 4 bytes before a dword boundary, and is
// stored as
//   head   a 1-byte and/or a 2-byte store up to the boundary,
//   body   (REC - HEAD) / 4 aligned dword stores,
//   tail   a 2-byte and/or a 1-byte store,
// never outside its own REC bytes and never wider than the address's alignment: the two records that share a
// dword write disjoint bytes of it, in any order.  No HIP is needed: a plain host compiler compiles this file
// (tests/host/record_pack_check.cpp runs it on the CPU).
#pragma once

#include <stdint.h>

#include <utility>

#ifdef __HIPCC__
#define SLRECORD_FN __device__ __forceinline__
#else
#define SLRECORD_FN inline
#endif

namespace slrecord {

// Bytes I .. I + 3 of the record (those past it come from the padding and are dropped by every caller).
template <int I, int N>
SLRECORD_FN uint32_t rec_bytes(const uint32_t (&w)[N]) {
  constexpr int d = I / 4, sh = 8 * (I % 4);
  static_assert(I >= 0 && d + (sh ? 1 : 0) < N, "the record's padding dword is missing");
  if constexpr (sh == 0) return w[d];
  else return (w[d] >> sh) | (w[d + 1] << (32 - sh));
}

template <int HEAD, int N, int... W>
SLRECORD_FN void put_dwords(unsigned char* o, const uint32_t (&w)[N], std::integer_sequence<int, W...>) {
  ((*reinterpret_cast<uint32_t*>(o + HEAD + 4 * W) = rec_bytes<HEAD + 4 * W>(w)), ...);
}

// One REC-byte record at o, which lies HEAD bytes before a dword boundary.
template <int REC, int HEAD, int N>
SLRECORD_FN void put_record(unsigned char* o, const uint32_t (&w)[N]) {
  static_assert(HEAD >= 0 && HEAD < 4 && REC >= HEAD, "HEAD is the distance to the next dword boundary");
  static_assert(N >= (REC + 3) / 4 + 1, "w holds the record and one padding dword");
  if constexpr ((HEAD & 1) != 0) o[0] = static_cast<unsigned char>(rec_bytes<0>(w));
  if constexpr ((HEAD & 2) != 0)
    *reinterpret_cast<uint16_t*>(o + (HEAD & 1)) = static_cast<uint16_t>(rec_bytes<(HEAD & 1)>(w));
  constexpr int words = (REC - HEAD) / 4, tail = (REC - HEAD) % 4, at = HEAD + 4 * words;
  put_dwords<HEAD>(o, w, std::make_integer_sequence<int, words>());
  if constexpr ((tail & 2) != 0) *reinterpret_cast<uint16_t*>(o + at) = static_cast<uint16_t>(rec_bytes<at>(w));
  if constexpr ((tail & 1) != 0) o[at + (tail & 2)] = static_cast<unsigned char>(rec_bytes<at + (tail & 2)>(w));
}

// Record r of the image of packed REC-byte records at img (dword-aligned).  The shape depends on (REC r) mod 4
// alone: with r = 4 lane + k that is (REC k) mod 4, the same for every lane of a wave.
template <int REC, int N>
SLRECORD_FN void put_record_at(unsigned char* img, int r, const uint32_t (&w)[N]) {
  unsigned char* o = img + REC * r;
  switch ((REC * r) & 3) {  // the start's byte within its dword
    case 0: put_record<REC, 0>(o, w); break;
    case 1: put_record<REC, 3>(o, w); break;
    case 2: put_record<REC, 2>(o, w); break;
    default: put_record<REC, 1>(o, w); break;
  }
}

}  // namespace slrecord
