// Stand-alone check of the blocks Renderer::render reports as stored into
// (raster.h: `written`) and of the shadow pixels it leaves alone
// (DirtyRect::shadow).  Build with raster.cpp and physics.cpp; the fill
// bodies follow BLENDTORCH_RASTER_ISA, so it is run once per ISA.
//
// Cube scene at 128x48 and 192x96, C = 3 and 4, both row orders, 3 and 8
// rotating slots, 400 random poses each; the runs with 3 slots also stamp the
// first 16 stored bytes the way cubesim --stamp does.  Every 37th frame is
// drawn a second time into the same slot with the same pose.  For every frame:
//   * the slot equals a full render (plus the stamp);
//   * a copy of the slot brought up to date only inside the reported blocks
//     equals the slot;
//   * with every byte outside the mask replaced by a sentinel beforehand (two
//     sentinels, a store may write either value), no such byte changes;
//   * the mask is a subset of the blocks of both frames' spans;
//   * a repeated pose reports no block that holds nothing but shadow.
// Over each run the mean mask share must lie strictly below the span masks'.
// Then a falling_cubes lap (several boxes, the non-deferred path): the mask
// of every frame equals the span union.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../common/block_mask.h"
#include "../sim/physics.h"
#include "../sim/raster.h"

using namespace btn;

namespace {

long long g_fail = 0;
void fail(const char* what, const char* tag, long long frame) {
  if (++g_fail <= 20) std::printf("FAIL %s: %s at frame %lld\n", tag, what, frame);
}

struct Grid {
  int W, H, C, band_rows, band_log2, nbands;
  Grid(int w, int h, int c) : W(w), H(h), C(c) {
    band_rows = blocks::band_rows_for(H), nbands = blocks::bands(H, band_rows);
    for (band_log2 = 0; (1 << band_log2) < band_rows;) ++band_log2;
    if (!blocks::geometry_ok(H, W, band_rows)) std::printf("bad geometry\n"), std::exit(2);
  }
  // f(byte offset, byte count) for every set (inside) or clear block
  template <class F>
  void for_blocks(const uint16_t* mask, bool inside, F&& f) const {
    for (int y = 0; y < H; ++y)
      for (int c = 0; c < W / blocks::kBlockCols; ++c)
        if (((mask[y >> band_log2] >> c) & 1) == (inside ? 1 : 0))
          f((size_t(y) * W + size_t(c) * blocks::kBlockCols) * size_t(C), size_t(blocks::kBlockCols) * size_t(C));
  }
  double share(const uint16_t* mask) const { return double(blocks::pixels(mask, H, band_rows)) / (double(W) * H); }
};

struct Slot {
  std::vector<uint8_t> bytes, mirror;
  sim::DirtyRect rec;
  uint16_t span[blocks::kMaxBands] = {};
};

struct Totals {
  double mask = 0, span = 0;
  long long frames = 0, kept_blocks = 0;
};

// One frame into `sl`, with every check; returns the mask in `wr`.
void frame_checks(const Grid& g, sim::Renderer& r, const sim::Scene& scene, Slot& sl, bool lower_left, bool stamp,
                  long long seq, bool expect_span_union, const char* tag, Totals& tot, uint16_t* wr) {
  const size_t n = size_t(g.W) * g.H * g.C;
  const std::vector<uint8_t> pre = sl.bytes;
  const sim::DirtyRect rec_before = sl.rec;
  const bool was_known = sl.rec.known;
  std::memset(wr, 0, sizeof(uint16_t) * blocks::kMaxBands);
  r.render(scene, sl.bytes.data(), &sl.rec, wr, g.band_log2);
  uint8_t st[16] = {'B', 'T', 7, 0, 0, 0, 0, 0};
  if (stamp) {
    const uint64_t q = uint64_t(seq);
    std::memcpy(st + 8, &q, 8);
    std::memcpy(sl.bytes.data(), st, sizeof(st));
    const int last = (int(sizeof(st)) + g.C - 1) / g.C - 1;
    sl.rec.foreign(lower_left ? g.H - 1 : 0, 0, last);
    wr[0] |= blocks::column_bits(0, last);
  }
  // a full render of the same pose
  std::vector<uint8_t> full(n);
  r.render(scene, full.data());
  if (stamp) std::memcpy(full.data(), st, sizeof(st));
  if (std::memcmp(full.data(), sl.bytes.data(), n) != 0) fail("incremental render differs from the full one", tag, seq);
  // the block mirror
  if (!was_known) sl.mirror = sl.bytes;
  else g.for_blocks(wr, true, [&](size_t o, size_t len) { std::memcpy(sl.mirror.data() + o, sl.bytes.data() + o, len); });
  if (sl.mirror != sl.bytes) fail("block mirror differs from the slot", tag, seq);
  // the span masks
  uint16_t cur[blocks::kMaxBands] = {}, uni[blocks::kMaxBands] = {};
  sim::span_blocks(sl.rec, g.H, lower_left, g.band_log2, cur);
  for (int k = 0; k < g.nbands; ++k) uni[k] = uint16_t(sl.span[k] | cur[k]);
  std::memcpy(sl.span, cur, sizeof(cur));
  if (!was_known) {
    for (int k = 0; k < g.nbands; ++k)
      if (wr[k] != blocks::all_columns(g.W)) fail("a fresh slot must report every block", tag, seq);
    return;
  }
  for (int k = 0; k < g.nbands; ++k) {
    if (wr[k] & ~uni[k]) fail("mask is no subset of the span mask", tag, seq);
    if (expect_span_union && wr[k] != uni[k]) fail("mask differs from the span union", tag, seq);
    tot.kept_blocks += __builtin_popcount(unsigned(uni[k] & ~wr[k]));
  }
  tot.mask += g.share(wr), tot.span += g.share(uni), ++tot.frames;
  // no store outside the mask (the render alone: the stamp lies inside it by construction)
  uint16_t rmask[blocks::kMaxBands];
  for (const uint8_t sentinel : {uint8_t(0xa5), uint8_t(0x5a)}) {
    std::vector<uint8_t> probe = pre;
    g.for_blocks(wr, false, [&](size_t o, size_t len) { std::memset(probe.data() + o, sentinel, len); });
    sim::DirtyRect rec_probe = rec_before;
    std::memset(rmask, 0, sizeof(rmask));
    r.render(scene, probe.data(), &rec_probe, rmask, g.band_log2);
    long long bad = 0;
    g.for_blocks(wr, false, [&](size_t o, size_t len) {
      for (size_t k = o; k < o + len; ++k) bad += probe[k] != sentinel;
    });
    if (bad) fail("a store outside the mask", tag, seq);
    // and what the render decides does not depend on the slot's bytes
    for (int k = 0; k < g.nbands; ++k)
      if (rmask[k] & ~wr[k]) fail("the mask depends on the slot's content", tag, seq);
  }
}

void cube_run(int W, int H, int C, bool lower_left, int nslots, uint64_t seed) {
  char tag[128];
  std::snprintf(tag, sizeof(tag), "cube %dx%d C=%d %s slots=%d isa=%s", W, H, C, lower_left ? "lower-left" : "upper-left",
                nslots, sim::raster_isa());
  const Grid g(W, H, C);
  sim::Scene scene = sim::cube_scene();
  scene.cam.width = W, scene.cam.height = H;
  sim::Renderer r(scene, C, lower_left);
  std::vector<Slot> slots(static_cast<size_t>(nslots));
  for (Slot& s : slots) s.bytes.assign(size_t(W) * H * C, 0x33), s.mirror = s.bytes;
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double pi = 3.14159265358979323846;
  const bool stamp = nslots == 3;
  Totals tot;
  long long repeats = 0, seq = 0, repeat_blocks = 0, repeat_span_blocks = 0;
  uint16_t wr[blocks::kMaxBands];
  for (int i = 0; i < 400; ++i) {
    scene.boxes[0].rot = sim::euler_xyz(pi * U(rng), pi * U(rng), pi * U(rng));
    Slot& sl = slots[size_t(i % nslots)];
    frame_checks(g, r, scene, sl, lower_left, stamp, seq++, false, tag, tot, wr);
    if (i % 37 != 36) continue;
    // the same pose again: nothing but the old face extent (and the stamp) is stored
    frame_checks(g, r, scene, sl, lower_left, stamp, seq++, false, tag, tot, wr);
    // (a row's span minus the shadow that stays: the face extent, what lies
    // between it and the shadow, and rows whose shadow takes the per-pixel test)
    uint16_t faces[blocks::kMaxBands] = {};
    for (int y = 0; y < H; ++y) {
      const sim::DirtyRect::ShadowRow& sr = sl.rec.shadow[size_t(y)];
      for (int x = std::max(sl.rec.lo[size_t(y)], 0); x <= sl.rec.hi[size_t(y)]; ++x)
        if (!(x >= sr.a && x <= sr.b) || (x >= sr.f0 && x <= sr.f1))
          faces[(lower_left ? H - 1 - y : y) >> g.band_log2] |= blocks::column_bits(x, x);
    }
    if (stamp) faces[0] |= blocks::column_bits(0, (16 + C - 1) / C - 1);
    for (int k = 0; k < g.nbands; ++k) {
      if (wr[k] & ~faces[k]) fail("a repeated pose stored into a block that holds shadow only", tag, seq);
      repeat_blocks += __builtin_popcount(unsigned(wr[k])), repeat_span_blocks += __builtin_popcount(unsigned(sl.span[k]));
    }
    ++repeats;
  }
  if (!(tot.mask < tot.span)) fail("mean mask share is not below the span masks'", tag, -1);
  if (!(repeat_blocks < repeat_span_blocks)) fail("repeated poses report no less than their spans", tag, -1);
  std::printf("%s: frames=%lld mask_share=%.4f span_share=%.4f kept_blocks=%lld repeats=%lld (%lld of %lld span blocks)\n", tag,
              tot.frames, tot.mask / double(tot.frames), tot.span / double(tot.frames), tot.kept_blocks, repeats, repeat_blocks,
              repeat_span_blocks);
}

void falling_run(int W, int H, int C, bool lower_left) {
  char tag[128];
  std::snprintf(tag, sizeof(tag), "falling_cubes %dx%d C=%d %s isa=%s", W, H, C, lower_left ? "lower-left" : "upper-left",
                sim::raster_isa());
  const Grid g(W, H, C);
  sim::Scene scene = sim::falling_cubes_scene();
  scene.cam.width = W, scene.cam.height = H;
  std::mt19937_64 rng(11);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double pi = 3.14159265358979323846;
  for (auto& b : scene.boxes) b.albedo = {float(U(rng)), float(U(rng)), float(U(rng))};
  sim::Renderer r(scene, C, lower_left);
  sim::RigidWorld physics(scene.plane_z);
  std::vector<Slot> slots(3);
  for (Slot& s : slots) s.bytes.assign(size_t(W) * H * C, 0x33), s.mirror = s.bytes;
  Totals tot;
  uint16_t wr[blocks::kMaxBands];
  for (int frame = 0; frame <= 100; ++frame) {   // one lap: the drop, then 100 steps
    if (frame == 0) {
      for (auto& b : scene.boxes) {
        b.center = {-3 + 6 * U(rng), -3 + 6 * U(rng), 6 + 6 * U(rng)};
        b.rot = sim::euler_xyz(-pi + 2 * pi * U(rng), -pi + 2 * pi * U(rng), -pi + 2 * pi * U(rng));
      }
      physics.reset(scene.boxes);
    } else {
      physics.step(scene.boxes, 1.0 / 60.0);
    }
    frame_checks(g, r, scene, slots[size_t(frame % 3)], lower_left, false, frame, true, tag, tot, wr);
  }
  std::printf("%s: frames=%lld mask_share=%.4f span_share=%.4f\n", tag, tot.frames, tot.mask / double(tot.frames),
              tot.span / double(tot.frames));
}

}  // namespace

int main() {
  uint64_t seed = 1;
  for (const auto& wh : {std::pair<int, int>{128, 48}, std::pair<int, int>{192, 96}})
    for (int C : {3, 4})
      for (bool lower_left : {false, true})
        for (int nslots : {3, 8}) cube_run(wh.first, wh.second, C, lower_left, nslots, seed++);
  falling_run(192, 96, 3, true);
  falling_run(128, 48, 4, false);
  std::printf("checks: failed=%lld isa=%s\n", g_fail, sim::raster_isa());
  std::printf(g_fail ? "FAIL\n" : "PASS\n");
  return g_fail ? 1 : 0;
}
