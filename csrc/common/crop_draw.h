// The crop window of every image of a stream (ops.Crop): drawn by the stream
// loader in arrival order (csrc/gpu/loader.cpp), exposed to Python as
// _native.crop_draw and mirrored in pure Python by ops.crop_windows.
//
// A window is (y0, x0, m): the upper-left corner of an h x w window in the
// upright H x W image, and whether the window is mirrored left-right.
//   random  three splitmix64 draws z per image, integer arithmetic only:
//             y0 = ((z >> 32) * (H - h + 1)) >> 32
//             x0 = (((z >> 32) * ((W - w) / x_align + 1)) >> 32) * x_align
//             m  = (z >> 40) < uint32(mirror * 2^24)
//   center  y0 = (H - h) / 2, x0 = (W - w) / 2 rounded down to x_align, m = 0
//   fixed   the given origin, m = 0
// center and fixed draw nothing.  The stream is seeded like the colour
// jitter's, with its own constant, so the two never share a state.
#pragma once

#include <cstdint>

namespace btn {
namespace crop {

enum Mode : int { kRandom = 0, kCenter = 1, kFixed = 2 };

struct Spec {
  int h = 0, w = 0;
  int mode = kRandom;
  int oy = 0, ox = 0;    // kFixed: the origin
  double mirror = 0.0;   // kRandom: probability of a mirrored window
  int x_align = 1;       // kRandom / kCenter: x0 is a multiple of it
};

struct Window {
  int y0 = 0, x0 = 0, m = 0;
};

inline uint64_t seed_state(uint64_t seed) { return seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull; }

inline uint64_t splitmix64(uint64_t& state) {
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the window fits the frame (and a fixed origin keeps it inside)
inline bool fits(const Spec& s, int H, int W) {
  if (s.h < 1 || s.w < 1 || s.h > H || s.w > W || s.x_align < 1) return false;
  if (s.mode == kFixed) return s.oy >= 0 && s.ox >= 0 && s.oy + s.h <= H && s.ox + s.w <= W;
  return true;
}

// next window of the stream; fits(s, H, W) must hold
inline Window draw(uint64_t& state, const Spec& s, int H, int W) {
  Window r;
  if (s.mode == kFixed) {
    r.y0 = s.oy, r.x0 = s.ox;
  } else if (s.mode == kCenter) {
    r.y0 = (H - s.h) / 2;
    r.x0 = (W - s.w) / 2 / s.x_align * s.x_align;
  } else {
    const uint64_t ny = uint64_t(H - s.h + 1), nx = uint64_t((W - s.w) / s.x_align + 1);
    r.y0 = int(((splitmix64(state) >> 32) * ny) >> 32);
    r.x0 = int(((splitmix64(state) >> 32) * nx) >> 32) * s.x_align;
    r.m = uint32_t(splitmix64(state) >> 40) < uint32_t(s.mirror * 16777216.0) ? 1 : 0;
  }
  return r;
}

}  // namespace crop
}  // namespace btn
