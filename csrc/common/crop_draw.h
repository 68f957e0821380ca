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

// The window of every image of a resized-crop stream (ops.ResizedCrop): drawn
// where the crop window is drawn, exposed as _native.resized_crop_draw and
// mirrored in pure Python by ops.resized_windows.
//
// A window is (y0, x0, h, w, m): an h x w window of the upright H x W image,
// resized to the configured output size, and whether the OUTPUT is mirrored.
//   random  five splitmix64 words z1..z5 per image.  With u(z) = (z >> 11) *
//           2^-53 and only +, -, *, / and sqrt in double (all correctly
//           rounded, so every language agrees bit for bit):
//             s = smin + u(z1) * (smax - smin)          fraction of the area
//             v = 2 u(z2);  r = v < 1 ? 1 + v (rmax - 1)
//                                     : 1 / (1 + (v - 1) (1 / rmin - 1))
//             A = s * double(H * W)
//             w = clamp(int(floor(sqrt(A * r) + 0.5)), 1, W)
//             h = clamp(int(floor(sqrt(A / r) + 0.5)), 1, H)
//             y0 = ((z3 >> 32) * (H - h + 1)) >> 32
//             x0 = ((z4 >> 32) * (W - w + 1)) >> 32
//             m  = (z5 >> 40) < uint32(mirror * 2^24)
//           A fixed number of draws per image, clamped rather than rejected,
//           aspect piecewise reciprocal-uniform about 1: not torchvision's
//           sampler.
//   center  the largest centred window of the output's aspect, m = 0
//   full    the whole frame, m = 0
//   fixed   the given window, m = 0
// Only random draws.  Seeded like the crop's stream, with its own constant.
namespace resized {

enum Mode : int { kRandom = 0, kCenter = 1, kFull = 2, kFixed = 3 };

struct Spec {
  int oh = 0, ow = 0;
  int mode = kRandom;
  double smin = 0.08, smax = 1.0;
  double rmin = 0.75, rmax = 4.0 / 3.0;
  int wy0 = 0, wx0 = 0, wh = 0, ww = 0;   // kFixed: the window
  double mirror = 0.0;                    // kRandom: probability of a mirrored output
};

struct Window {
  int y0 = 0, x0 = 0, h = 0, w = 0, m = 0;
};

inline uint64_t seed_state(uint64_t seed) { return seed * 0x9E3779B97F4A7C15ull + 0xA0761D6478BD642Full; }

// the spec itself is legal (whatever the frame)
inline bool valid(const Spec& s) {
  if (s.oh < 1 || s.ow < 1 || s.oh > 32767 || s.ow > 32767 || s.mode < kRandom || s.mode > kFixed) return false;
  if (!(s.smin > 0.0 && s.smin <= s.smax && s.smax <= 1.0)) return false;
  if (!(s.rmin > 0.0 && s.rmin <= 1.0 && 1.0 <= s.rmax)) return false;
  if (!(s.mirror >= 0.0 && s.mirror <= 1.0)) return false;
  if (s.mode == kFixed && (s.wy0 < 0 || s.wx0 < 0 || s.wh < 1 || s.ww < 1)) return false;
  return true;
}

// every window of the spec lies inside an H x W frame (only a fixed one can leave it)
inline bool fits(const Spec& s, int H, int W) {
  if (H < 1 || W < 1) return false;
  if (s.mode == kFixed) return s.wy0 >= 0 && s.wx0 >= 0 && s.wh >= 1 && s.ww >= 1 && s.wy0 + s.wh <= H && s.wx0 + s.ww <= W;
  return true;
}

// next window of the stream; valid(s) and fits(s, H, W) must hold
inline Window draw(uint64_t& state, const Spec& s, int H, int W) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  Window r;
  if (s.mode == kFixed) {
    r.y0 = s.wy0, r.x0 = s.wx0, r.h = s.wh, r.w = s.ww;
  } else if (s.mode == kFull) {
    r.h = H, r.w = W;
  } else if (s.mode == kCenter) {
    if (int64_t(W) * s.oh >= int64_t(H) * s.ow) {
      r.h = H;
      r.w = int(int64_t(H) * s.ow / s.oh);
      if (r.w < 1) r.w = 1;
    } else {
      r.w = W;
      r.h = int(int64_t(W) * s.oh / s.ow);
      if (r.h < 1) r.h = 1;
    }
    r.y0 = (H - r.h) / 2, r.x0 = (W - r.w) / 2;
  } else {
    auto u = [&state]() { return double(crop::splitmix64(state) >> 11) * (1.0 / 9007199254740992.0); };
    const double sa = s.smin + u() * (s.smax - s.smin);
    const double v = 2.0 * u();
    const double ar = v < 1.0 ? 1.0 + v * (s.rmax - 1.0) : 1.0 / (1.0 + (v - 1.0) * (1.0 / s.rmin - 1.0));
    const double A = sa * double(int64_t(H) * W);
    const double fw = __builtin_floor(__builtin_sqrt(A * ar) + 0.5), fh = __builtin_floor(__builtin_sqrt(A / ar) + 0.5);
    r.w = fw < 1.0 ? 1 : (fw > double(W) ? W : int(fw));
    r.h = fh < 1.0 ? 1 : (fh > double(H) ? H : int(fh));
    r.y0 = int(((crop::splitmix64(state) >> 32) * uint64_t(H - r.h + 1)) >> 32);
    r.x0 = int(((crop::splitmix64(state) >> 32) * uint64_t(W - r.w + 1)) >> 32);
    r.m = uint32_t(crop::splitmix64(state) >> 40) < uint32_t(s.mirror * 16777216.0) ? 1 : 0;
  }
  return r;
}

}  // namespace resized
}  // namespace btn
