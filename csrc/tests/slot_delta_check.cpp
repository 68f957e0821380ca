// Stand-alone check of the slot-delta report and the slot-mirror bookkeeping
// (csrc/sim/raster.h: changed_rect, csrc/gpu/slot_mirror.h), meant to be built
// with -fsanitize=address,undefined (tests/test_slot_delta_sanitized.py):
//   * rendering: 6 x K frames into K = 4 rotating 64x48 buffers (a ring's
//     life), 3 and 4 channels, both row orders, the Cube and the falling_cubes
//     scene, stamped like cubesim --stamp.  A byte mirror per buffer is
//     updated only inside the rectangle a consumer would be told about -- as
//     reported, and widened as the loader widens it -- and must equal the
//     buffer after every frame;
//   * mutation: the same with every rectangle shrunk by one pixel must NOT
//     stay equal (the check can fail);
//   * bookkeeping: base match / mismatch, first use, invalidate, empty
//     rectangle, a rectangle that leaves the frame, the byte budget, widening
//     at both frame edges.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../gpu/slot_mirror.h"
#include "../sim/raster.h"

using namespace btn;
namespace mir = btn::gpu::mirror;

namespace {

int g_failed = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++g_failed;                                                       \
    }                                                                   \
  } while (0)

struct Tally {
  long reported = 0, widened = 0, shrunk = 0;
};

void copy_region(uint8_t* dst, const uint8_t* src, const mir::Region& r, int W, int C) {
  for (int y = r.y0; !r.empty() && y <= r.y1; ++y) {
    const size_t o = (size_t(y) * W + size_t(r.x0)) * size_t(C);
    std::memcpy(dst + o, src + o, size_t(r.x1 - r.x0 + 1) * size_t(C));
  }
}

long differing(const uint8_t* a, const uint8_t* b, size_t n) {
  long d = 0;
  for (size_t k = 0; k < n; ++k) d += a[k] != b[k];
  return d;
}

Tally render_mirrors(bool falling, int C, bool lower_left) {
  constexpr int K = 4, W = 64, H = 48;
  sim::Scene scene = falling ? sim::falling_cubes_scene() : sim::cube_scene();
  scene.cam.width = W, scene.cam.height = H;
  const size_t n = size_t(W) * H * size_t(C);
  sim::Renderer r(scene, C, lower_left);
  // exact-size heap buffers: a copy past either end is an ASan report
  std::vector<std::unique_ptr<uint8_t[]>> buf, m_rep, m_wide, m_shr;
  for (int k = 0; k < K; ++k) {
    buf.emplace_back(new uint8_t[n]), m_rep.emplace_back(new uint8_t[n]);
    m_wide.emplace_back(new uint8_t[n]), m_shr.emplace_back(new uint8_t[n]);
    std::memset(buf[size_t(k)].get(), 0x5a, n);   // a slot that held anything
  }
  std::vector<sim::DirtyRect> dirty(K);
  std::mt19937_64 rng(uint64_t(17 + C + (lower_left ? 100 : 0) + (falling ? 1000 : 0)));
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double pi = 3.14159265358979323846;
  Tally t;
  for (int i = 0; i < 6 * K; ++i) {
    for (auto& b : scene.boxes) {
      if (falling) b.center = {-3 + 6 * U(rng), -3 + 6 * U(rng), 6 * U(rng)};
      b.rot = sim::euler_xyz(pi * U(rng), pi * U(rng), pi * U(rng));
    }
    const size_t k = size_t(i % K);
    sim::DirtyRect before;
    const bool was_known = dirty[k].known;
    before.x0 = dirty[k].x0, before.y0 = dirty[k].y0, before.x1 = dirty[k].x1, before.y1 = dirty[k].y1;
    uint8_t* out = buf[k].get();
    r.render(scene, out, &dirty[k]);
    // cubesim --stamp: 16 bytes at the start of the first stored row
    uint8_t st[16] = {'B', 'T', 0, 0, 0, 0, 0, 0};
    const uint64_t seq = uint64_t(i);
    std::memcpy(st + 8, &seq, 8);
    std::memcpy(out, st, sizeof(st));
    dirty[k].add(lower_left ? H - 1 : 0, 0, (int(sizeof(st)) + C - 1) / C - 1);
    if (!was_known) {   // a slot's first frame is taken whole
      std::memcpy(m_rep[k].get(), out, n);
      std::memcpy(m_wide[k].get(), out, n);
      std::memcpy(m_shr[k].get(), out, n);
    } else {
      const sim::StoredRect c = sim::changed_rect(before, dirty[k], H, lower_left);
      mir::Delta d;
      d.rect.y0 = c.y0, d.rect.y1 = c.y1, d.rect.x0 = c.x0, d.rect.x1 = c.x1;
      CHECK(mir::delta_valid(d, H, W));
      copy_region(m_rep[k].get(), out, d.rect, W, C);
      copy_region(m_wide[k].get(), out, mir::widen(d.rect, W), W, C);
      mir::Region s = d.rect;
      s.y0 += 1, s.y1 -= 1, s.x0 += 1, s.x1 -= 1;
      copy_region(m_shr[k].get(), out, s, W, C);
    }
    t.reported += differing(m_rep[k].get(), out, n);
    t.widened += differing(m_wide[k].get(), out, n);
    t.shrunk += differing(m_shr[k].get(), out, n);
  }
  return t;
}

void bookkeeping() {
  const int H = 480, W = 640;
  mir::Ring ring(4);
  mir::Delta d;
  d.base_gen = 7;
  d.rect.y0 = 100, d.rect.y1 = 200, d.rect.x0 = 70, d.rect.x1 = 130;
  bool used = true;
  // first use: nothing held, whole frame; afterwards the mirror holds the generation
  mir::Region r = ring.decide(1, 7, nullptr, H, W, &used);
  CHECK(!used && r.whole(H, W) && ring.holds(1, 7) && !ring.holds(1, 8) && !ring.holds(0, 7));
  // base match: the reported rectangle, widened to 64-pixel blocks
  r = ring.decide(1, 9, &d, H, W, &used);
  CHECK(used && r.y0 == 100 && r.y1 == 200 && r.x0 == 64 && r.x1 == 191 && ring.holds(1, 9));
  CHECK(r.pixels() == int64_t(101) * 128);
  // base mismatch (the mirror holds 9, the report refers to 7)
  r = ring.decide(1, 11, &d, H, W, &used);
  CHECK(!used && r.whole(H, W) && ring.holds(1, 11));
  // invalidate: a matching base no longer counts
  d.base_gen = 11;
  ring.invalidate(1);
  CHECK(!ring.holds(1, 11));
  r = ring.decide(1, 12, &d, H, W, &used);
  CHECK(!used && r.whole(H, W));
  // empty rectangle: nothing from the host
  d.base_gen = 12;
  d.rect = mir::Region();
  CHECK(mir::delta_valid(d, H, W));
  r = ring.decide(1, 13, &d, H, W, &used);
  CHECK(used && r.empty() && r.pixels() == 0 && ring.holds(1, 13));
  // a rectangle that leaves the frame is refused, and never used
  d.base_gen = 13;
  d.rect.y0 = 0, d.rect.y1 = H, d.rect.x0 = 0, d.rect.x1 = 10;
  CHECK(!mir::delta_valid(d, H, W));
  d.rect.y1 = 10, d.rect.x1 = W;
  CHECK(!mir::delta_valid(d, H, W));
  d.rect.x0 = -1, d.rect.x1 = 10;
  CHECK(!mir::delta_valid(d, H, W));
  d.rect.x0 = 11;
  CHECK(!mir::delta_valid(d, H, W));   // x1 < x0 with rows present
  r = ring.decide(1, 14, &d, H, W, &used);
  CHECK(!used && r.whole(H, W));
  // a slot outside the ring: whole frame, nothing recorded
  r = ring.decide(9, 1, nullptr, H, W, &used);
  CHECK(!used && r.whole(H, W) && !ring.holds(9, 1));
  // widening at both frame edges, and for rows that are no multiple of 64 pixels
  mir::Region e;
  e.y0 = 0, e.y1 = H - 1, e.x0 = 3, e.x1 = 70;
  r = mir::widen(e, W);
  CHECK(r.x0 == 0 && r.x1 == 127 && r.y0 == 0 && r.y1 == H - 1);
  e.x0 = 600, e.x1 = W - 1;
  r = mir::widen(e, W);
  CHECK(r.x0 == 576 && r.x1 == W - 1);
  e.x0 = 64, e.x1 = 127;
  r = mir::widen(e, W);
  CHECK(r.x0 == 64 && r.x1 == 127);   // already aligned: unchanged
  r = mir::widen(e, 100);
  CHECK(r.x0 == 0 && r.x1 == 99);
  r = mir::widen(e, 160);
  CHECK(r.x0 == 0 && r.x1 == 159);
  CHECK(mir::widen(mir::Region(), W).empty());
  // the byte budget
  mir::Budget b(1000);
  CHECK(b.reserve(600) && !b.reserve(401) && b.reserve(400) && !b.reserve(1) && b.used() == 1000);
  mir::Budget none(1);
  CHECK(!none.reserve(2) && none.used() == 0);
  mir::Budget big(~size_t(0));
  CHECK(big.reserve(~size_t(0) - 1) && !big.reserve(2));   // no wrap-around into "fits"
}

}  // namespace

int main() {
  Tally all;
  for (int falling = 0; falling < 2; ++falling)
    for (int C = 3; C <= 4; ++C)
      for (int ll = 0; ll < 2; ++ll) {
        const Tally t = render_mirrors(falling != 0, C, ll != 0);
        CHECK(t.reported == 0 && t.widened == 0);
        CHECK(t.shrunk > 0);   // the mutation is caught in every configuration
        all.reported += t.reported, all.widened += t.widened, all.shrunk += t.shrunk;
      }
  bookkeeping();
  std::printf("mirror_mismatched=%ld widened_mismatched=%ld shrunk_detected=%d failed=%d\n", all.reported,
              all.widened, all.shrunk > 0 ? 1 : 0, g_failed);
  return g_failed == 0 ? 0 : 1;
}
