// The `rgb_a` frame layout of the shared-memory ring (csrc/transport/shmring.h):
// an RGBA frame stored as H*W*3 bytes of packed RGB (row-major, the frame's own
// row order) followed by its H*W alpha bytes at byte offset H*W*3.  A consumer
// that decodes RGB only reads the first three quarters of the slot in place;
// every other consumer rebuilds the interleaved H x W x 4 frame with
// interleave_rgb_a().  Header-only: the producer (cubesim), the GPU loader and
// the `_native` module (CPU dataset path) share it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace btn {
namespace planar {

constexpr const char* kName = "rgb_a";

// May a frame of this shape be stored as rgb_a?  RGBA only, and the alpha
// plane must start 16-byte aligned (the decode kernel's vector loads of the
// RGB part then never touch it).
inline bool supported(int64_t h, int64_t w, int64_t c) {
  return c == 4 && h > 0 && w > 0 && h <= (int64_t(1) << 20) && w <= (int64_t(1) << 20) && (h * w * 3) % 16 == 0;
}

// Does an rgb_a frame of h x w pixels at byte offset `off` end at or before
// `slot_end` (both offsets into the same segment)?  Overflow-free.
inline bool rgb_a_valid(int64_t h, int64_t w, int64_t off, uint64_t slot_end) {
  if (!supported(h, w, 4) || off < 0) return false;
  const uint64_t bytes = uint64_t(h) * uint64_t(w) * 4;   // < 2^42
  return uint64_t(off) <= slot_end && bytes <= slot_end - uint64_t(off);
}

// dst[4 p + k] = rgb[3 p + k] (k < 3), dst[4 p + 3] = a[p], for p < npix.
// dst must not overlap the sources.
inline void interleave_rgb_a(uint8_t* dst, const uint8_t* rgb, const uint8_t* a, size_t npix) {
  for (size_t p = 0; p < npix; ++p) {
    dst[4 * p] = rgb[3 * p];
    dst[4 * p + 1] = rgb[3 * p + 1];
    dst[4 * p + 2] = rgb[3 * p + 2];
    dst[4 * p + 3] = a[p];
  }
}

}  // namespace planar
}  // namespace btn
