// Changed-block masks of a frame (shmring.h: kWantSlotBlocks; slot_mirror.h).
//
// A frame is cut into blocks of kBlockCols pixel columns x band_rows stored
// rows on an absolute grid from row 0 and column 0.  Band k holds stored rows
// [k * band_rows, (k + 1) * band_rows) -- the last band may be partial -- and
// is one little-endian uint16 word; bit c of it covers pixel columns
// [64c, 64c + 63].  band_rows is a power of two.  Producer, loader and kernel
// share the limits below; this header is host only and never looks at pixels.
#pragma once

#include <cstdint>

namespace btn {
namespace blocks {

constexpr int kBlockCols = 64;     // pixel columns per block (64-byte lines for 3- and 4-byte pixels alike)
constexpr int kMaxWidth = 1024;    // 16 column blocks: one uint16 per band
constexpr int kMaxBands = 30;      // what one image may take of the kernel's argument space (kernels.h)

inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int bands(int H, int band_rows) { return (H + band_rows - 1) / band_rows; }

// Can frames of this size carry a mask at all?
inline bool width_ok(int W) { return W > 0 && W % kBlockCols == 0 && W <= kMaxWidth; }

// A usable grid for an H x W frame.
inline bool geometry_ok(int H, int W, int band_rows) {
  return H > 0 && width_ok(W) && pow2(band_rows) && bands(H, band_rows) <= kMaxBands;
}

// The band height a producer (and a loader that builds a mask from a
// rectangle) uses: the smallest power of two whose band count fits -- 16 for
// 480 rows, 2 for 48: the bands of a small frame stay about as fine, against
// its height, as those of a large one.
inline int band_rows_for(int H) {
  int r = 1;
  while (bands(H, r) > kMaxBands) r *= 2;
  return r;
}

// Bits of the column blocks that pixel columns [a, b] touch (0 <= a <= b < kMaxWidth).
inline uint16_t column_bits(int a, int b) {
  return uint16_t((2u << (unsigned(b) / kBlockCols)) - (1u << (unsigned(a) / kBlockCols)));
}

// Every column block of a W-pixel row.
inline uint16_t all_columns(int W) { return column_bits(0, W - 1); }

// Pixels the set blocks of `mask` (bands(H, band_rows) words) cover.
inline int64_t pixels(const uint16_t* mask, int H, int band_rows) {
  int64_t n = 0;
  for (int k = 0, nb = bands(H, band_rows); k < nb; ++k) {
    const int rows = (k + 1) * band_rows <= H ? band_rows : H - k * band_rows;
    n += int64_t(__builtin_popcount(mask[k])) * kBlockCols * rows;
  }
  return n;
}

}  // namespace blocks
}  // namespace btn
