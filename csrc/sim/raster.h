// Headless CPU renderer for the blendtorch stand-in producers.
//
// Blender/Eevee is not available in this stack, so the producers that feed
// the benchmark and the tests render their scenes here instead.  The scene
// model covers what the reference's example scenes contain
// (reference: examples/datagen/cube.blend, falling_cubes.blend -- camera,
// point light, ground plane, one or more boxes):
//   * a pinhole camera with Blender's conventions (looks down its local -Z,
//     +Y up, sensor_fit AUTO, focal length in pixels = lens/sensor * max(W,H));
//   * a point light with inverse-square falloff plus ambient term;
//   * an infinite-ish ground plane (square of half-size `plane_half`) that
//     receives box shadows (shadow rays against each oriented box);
//   * convex boxes drawn by rasterising their front faces with per-pixel
//     Lambert shading.
// Projection helpers follow btb.Camera (reference: pkg_blender/blendtorch/btb/
// camera.py:84-162): NDC in [-1,1], pixel = (ndc+1)/2 * [W,H] with the y axis
// flipped for the upper-left origin -- no half-pixel offset.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace btn {
namespace sim {

struct Vec3 {
  double x = 0, y = 0, z = 0;
};

using Mat3 = std::array<double, 9>;   // row major

Mat3 euler_xyz(double rx, double ry, double rz);   // Blender 'XYZ' euler: Rz*Ry*Rx
Vec3 mul(const Mat3& m, const Vec3& v);
Vec3 mul_t(const Mat3& m, const Vec3& v);          // m^T v

struct Camera {
  int width = 640, height = 480;
  double lens_mm = 50.0, sensor_mm = 36.0;
  double clip_start = 0.1, clip_end = 100.0;
  Vec3 loc;
  Mat3 rot;      // camera-to-world rotation
  double focal_px() const;
  // world -> pixel (upper-left origin); returns false if behind the camera.
  bool project(const Vec3& w, double* px, double* py, double* depth = nullptr) const;
};

struct Box {
  Vec3 center;
  Vec3 half{1, 1, 1};
  Mat3 rot;                                   // local-to-world
  std::array<float, 3> albedo{0.8f, 0.8f, 0.8f};
  // The 8 corners in Blender's default-cube vertex order.
  std::array<Vec3, 8> corners() const;
};

struct Light {
  Vec3 loc;
  double power = 1000.0;   // W-ish; scaled so the default scene is well exposed
};

struct Scene {
  Camera cam;
  Light light;
  double ambient = 0.08;
  double plane_z = -2.0;
  double plane_half = 10.0;
  std::array<float, 3> plane_albedo{0.8f, 0.8f, 0.8f};
  std::array<float, 3> world{0.051f, 0.051f, 0.051f};
  std::vector<Box> boxes;
};

// The default-cube scene of examples/datagen/cube.blend (640x480, camera at
// (7.359,-6.926,4.958) with Blender's default rotation, light at
// (4.076,1.005,5.904), ground plane at z=-2).
Scene cube_scene();
// examples/datagen/falling_cubes.blend stand-in: 7 boxes, raised camera.
Scene falling_cubes_scene();

// Bounding rectangle (image coordinates, row 0 = top, inclusive) of every
// pixel a frame wrote over the background.  A buffer that is rendered into
// again and again (a shared-memory ring slot) keeps the rectangle its last
// frame left; the next render restores the background inside it only,
// instead of copying the whole background.  `known` false = the buffer's
// content is unknown (fresh slot): full background copy.
// With `lo` / `hi` sized to the image height, each row also keeps the span
// it wrote (a box and its shadow cover ~57 % of their bounding rectangle, so
// a restore over the row spans moves that much less memory).
// `shadow` (sized to the image height by a render of a one-box scene, else
// empty) keeps what lets the next render leave shadow bytes alone that are
// shadow already: per image row the interval [a, b] the frame's shadow fill
// covered on a plane_dense_ row (a > b: none) and the extent [f0, f1] of its
// face spans.  After the frame every pixel of [a, b] outside [f0, f1] holds
// the shadow colour.  Whoever writes into the buffer besides render() calls
// foreign(): that row's record is dropped.
struct DirtyRect {
  struct ShadowRow {
    int a = 1, b = 0, f0 = 1 << 30, f1 = -1;
  };
  int x0 = 1 << 30, y0 = 1 << 30, x1 = -1, y1 = -1;
  bool known = false;
  std::vector<int> lo, hi;   // per image row [lo, hi]; empty = rectangle only
  std::vector<ShadowRow> shadow;
  bool empty() const { return x1 < x0 || y1 < y0; }
  // pixels [a, b] of image row y were written by someone other than render()
  void foreign(int y, int a, int b) {
    add(y, a, b);
    if (!shadow.empty()) shadow[static_cast<unsigned>(y)] = ShadowRow();
  }
  void reset() { x0 = y0 = 1 << 30, x1 = y1 = -1; }
  void add(int y, int a, int b) {
    y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
    x0 = a < x0 ? a : x0, x1 = b > x1 ? b : x1;
    if (!lo.empty()) {
      int& l = lo[static_cast<unsigned>(y)];
      int& h = hi[static_cast<unsigned>(y)];
      l = a < l ? a : l, h = b > h ? b : h;
    }
  }
};

// What a render into a buffer of known content changed, in STORED rows (a
// lower-left frame stores image row y at H - 1 - y): the union of the
// rectangle the render restored (`before`) and the one it left (`after`).
// Every byte outside it is what the buffer held before.  Empty: y1 < y0.
struct StoredRect {
  int y0 = 0, y1 = -1, x0 = 0, x1 = -1;
  bool empty() const { return y1 < y0 || x1 < x0; }
};
inline StoredRect changed_rect(const DirtyRect& before, const DirtyRect& after, int H, bool lower_left) {
  DirtyRect u;
  if (!before.empty()) u.add(before.y0, before.x0, before.x1), u.add(before.y1, before.x0, before.x1);
  if (!after.empty()) u.add(after.y0, after.x0, after.x1), u.add(after.y1, after.x0, after.x1);
  StoredRect r;
  if (u.empty()) return r;
  r.x0 = u.x0, r.x1 = u.x1;
  r.y0 = lower_left ? H - 1 - u.y1 : u.y0;
  r.y1 = lower_left ? H - 1 - u.y0 : u.y1;
  return r;
}

// The 64-column x band_rows blocks (csrc/common/block_mask.h) that the pixels
// a frame left over the background touch: `d`'s per-row spans (the rectangle
// where it keeps none), OR-ed into out[ceil(H / band_rows)] in STORED rows.
// The caller clears `out`; band_rows = 1 << band_log2, W <= 1024.  What a
// render into a buffer of known content changed lies in the union of the
// blocks of the record it found and of the one it left.
inline void span_blocks(const DirtyRect& d, int H, bool lower_left, int band_log2, uint16_t* out) {
  if (d.empty()) return;
  const bool rows = d.lo.size() == std::size_t(H) && d.hi.size() == std::size_t(H);
  const int y0 = d.y0 < 0 ? 0 : d.y0, y1 = d.y1 > H - 1 ? H - 1 : d.y1;
  for (int y = y0; y <= y1; ++y) {
    const int a = rows ? d.lo[std::size_t(y)] : d.x0, b = rows ? d.hi[std::size_t(y)] : d.x1;
    if (a > b || a < 0) continue;
    const int sy = lower_left ? H - 1 - y : y;
    out[sy >> band_log2] |= uint16_t((2u << (unsigned(b) >> 6)) - (1u << (unsigned(a) >> 6)));
  }
}

// Frame renderer.  Camera, light and ground plane are static for the life of
// a Renderer, so their shading (the whole background) is computed once and
// cached together with each pixel's ground-plane hit point; a frame then costs
// one background copy, span fills of the boxes' projected shadow hulls and
// scan conversion of the boxes' front faces.
// Output: H*W*channels bytes, row-major HWC uint8, channels 3 or 4 (alpha =
// 255); `lower_left` stores row 0 = bottom image row (OpenGL readback order).
class Renderer {
 public:
  Renderer(const Scene& s, int channels, bool lower_left);
  // dirty: the rectangle `out`'s previous frame left (updated to this
  // frame's); nullptr = `out` holds anything, copy the whole background.
  // written: the blocks (csrc/common/block_mask.h; band_rows = 1 << band_log2,
  // W <= 1024) that a store of this call touched, transient stores included,
  // OR-ed into written[ceil(H / band_rows)] in STORED rows; the caller clears
  // it.  Every byte outside them is what `out` held before the call.  On a
  // buffer of known content that is less than the blocks of both frames'
  // spans (span_blocks): shadow pixels the previous frame left as shadow are
  // not stored again.  Unknown content: every block.
  void render(const Scene& s, uint8_t* out, DirtyRect* dirty = nullptr, uint16_t* written = nullptr,
              int band_log2 = 0);
  int width() const { return W_; }
  int height() const { return H_; }
  int channels() const { return C_; }
  // the stored bytes of a frame without boxes (what a DirtyRect restores)
  const std::vector<uint8_t>& background() const { return background_; }

 private:
  void put(uint8_t* out, int x, int y, float r, float g, float b) const;
  int W_, H_, C_;
  bool lower_left_;
  std::vector<uint8_t> background_;     // final HWC bytes, boxes absent
  std::vector<float> plane_xy_;         // per pixel ground hit (x,y); NaN = no hit
  // per image row: the ground plane covers pixels [plane_x0_, plane_x1_] and
  // nothing else (plane_dense_ = 1), or the row needs the per-pixel test
  std::vector<int> plane_x0_, plane_x1_;
  std::vector<uint8_t> plane_dense_;
  uint8_t shadow_rgb_[3];
  uint8_t shadow_pat3_[96];              // 32 packed-RGB shadow pixels (vector fills)
  std::vector<float> depth_;             // 1/depth per pixel, zero outside depth_rect_
  DirtyRect depth_rect_;                // pixels of depth_ the last frame wrote
  // Restore after draw (one box, buffer of known content): the frame is drawn
  // first and records, per image row, the intervals it wrote in full (the
  // shadow's interval on plane_dense_ rows, every face span); the previous
  // frame's span is then restored minus those.  The cube turns in place under
  // a fixed light, so most of the old span is overwritten anyway and never
  // copied from the background first.
  static constexpr int kMaxCover = 8;    // 1 shadow + 3 front faces x 2 triangles, and one spare
  static constexpr uint8_t kRowRestored = 0xff;   // cover_n_: the row took the old order (restored before its draw)
  std::vector<int> cover_;               // per row kMaxCover x [x0, x1]
  std::vector<uint8_t> cover_n_;         // per row: intervals recorded, or kRowRestored
  std::vector<int> prev_lo_, prev_hi_;   // the previous frame's row spans while this frame draws
  std::vector<DirtyRect::ShadowRow> prev_shadow_;   // and its shadow record (DirtyRect::shadow)
};

// Which fill bodies render() uses: "avx2" (8 tone-table indices per op, a
// gather and a byte shuffle per 8 pixels, 32-byte pattern stores for the
// shadow) where the CPU has it, else "scalar" (the 4-wide SSE index code with
// one store per pixel).  BLENDTORCH_RASTER_ISA=scalar|avx2 picks one; it is
// read once.  Both write the same bytes.
const char* raster_isa();

// Triangle-mesh rendering (z-buffered, two-sided Lambert from a directional
// light + ambient) over a uniform background -- used for parametric shapes
// (the densityopt supershapes).  verts: N x 3 world coordinates; tris:
// M x 3 vertex indices.  Output HWC u8 (linear values tone-mapped like the
// box renderer), row 0 = top unless lower_left.
struct MeshStyle {
  std::array<float, 3> albedo{0.8f, 0.8f, 0.8f};
  std::array<float, 3> background{0.05f, 0.05f, 0.05f};
  Vec3 light_dir{-0.4, -0.6, -0.7};   // direction the light travels
  double ambient = 0.15;
};
void render_mesh(const Camera& cam, const std::vector<float>& verts, const std::vector<int>& tris,
                 const MeshStyle& style, uint8_t* out, int channels, bool lower_left);

// One-shot convenience wrapper (builds a Renderer per call).
void render(const Scene& s, uint8_t* out, int channels, bool lower_left);

}  // namespace sim
}  // namespace btn
