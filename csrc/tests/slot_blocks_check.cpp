// Stand-alone check of the changed-block report (csrc/sim/raster.h:
// span_blocks, csrc/common/block_mask.h), the slot mirror's block decision
// (csrc/gpu/slot_mirror.h: blocks_from_report, rect_blocks, decide_blocks) and
// the descriptor scan's 11th element (csrc/codec/pickle_codec.h), meant to be
// built with -fsanitize=address,undefined (tests/test_slot_blocks_sanitized.py):
//   * rendering: 8 x K random poses into K = 3 rotating buffers of 128x48,
//     256x40 and 640x96, 3 and 4 channels, both row orders, the Cube and the
//     falling_cubes scene, stamped like cubesim --stamp.  A byte mirror per
//     buffer is updated only inside the set blocks of the mask a producer
//     would send (the union of the blocks of the slot's previous spans and
//     the new ones) -- through the decision of a mirror::Ring, which also
//     sees frames whose report it has to refuse -- and must equal the buffer
//     after every frame; the mask lies inside the blocks of the widened
//     rectangle;
//   * mutation: the same with the lowest set bit of every mask cleared must
//     NOT stay equal (the check can fail);
//   * W % 64 != 0 (96x48): no grid, no mask; the decision is not asked;
//   * bookkeeping: reported mask, rectangle fallback, all ones, another grid,
//     malformed reports, partial last band, pixel counts;
//   * scan: every message, with and without the element, truncated at every
//     length and with its mask length field mutated, scanned from an exactly
//     sized heap copy and compared with parse().
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../codec/pickle_codec.h"
#include "../common/block_mask.h"
#include "../gpu/slot_mirror.h"
#include "../sim/raster.h"

using namespace btn;
namespace mir = btn::gpu::mirror;

namespace {

int g_failed = 0;
long g_parse_threw = 0;   // inputs the scan accepted and parse() refused
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++g_failed;                                                       \
    }                                                                   \
  } while (0)

struct Tally {
  long masked = 0, cleared = 0, frames = 0, reports = 0, scans = 0;
  double fraction = 0;
};

void copy_blocks(uint8_t* dst, const uint8_t* src, const mir::BlockMask& m, int H, int W, int C) {
  for (int y = 0; y < H; ++y) {
    const unsigned word = m.w[y / m.band_rows];
    for (int c = 0; c < W / 64; ++c)
      if ((word >> c) & 1u) {
        const size_t o = (size_t(y) * W + size_t(64 * c)) * size_t(C);
        std::memcpy(dst + o, src + o, size_t(64) * size_t(C));
      }
  }
}

long differing(const uint8_t* a, const uint8_t* b, size_t n) {
  long d = 0;
  for (size_t k = 0; k < n; ++k) d += a[k] != b[k];
  return d;
}

// every set bit of `a` is set in `b` (same grid)
bool inside(const mir::BlockMask& a, const mir::BlockMask& b, int H) {
  if (a.band_rows != b.band_rows) return false;
  for (int k = 0; k < blocks::bands(H, a.band_rows); ++k)
    if (a.w[k] & ~b.w[k]) return false;
  return true;
}

// the descriptor message a producer writes for this report
codec::Bytes message(uint32_t gen, const mir::Delta& d, int H, int W, int C, int band_rows, const uint8_t* le, size_t nle) {
  codec::Writer w(4);
  w.begin_dict();
  w.key("btid");
  w.integer(1);
  w.key("frameid");
  w.integer(int64_t(gen));
  w.key("_btshm");
  w.begin_tuple();
  w.str("blendtorch-1-0");
  w.integer(2);
  w.integer(4096);
  w.integer(H), w.integer(W), w.integer(C);
  w.str("image");
  w.integer(int64_t(gen));
  w.none();
  w.begin_tuple();
  w.integer(int64_t(d.base_gen));
  w.integer(d.rect.y0), w.integer(d.rect.y1), w.integer(d.rect.x0), w.integer(d.rect.x1);
  w.end_tuple();
  if (le) {
    w.begin_tuple();
    w.integer(band_rows);
    w.bytes(le, nle);
    w.end_tuple();
  }
  w.end_tuple();
  w.end_dict();
  return w.finish();
}

// scan an exactly sized heap copy; what it says about element 11 must be what parse() says
bool scan_agrees(const uint8_t* data, size_t n, bool* accepted, mir::BlockReport* out = nullptr,
                 std::unique_ptr<uint8_t[]>* keep = nullptr) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(copy.get(), data, n);
  codec::DescriptorScan sc;
  *accepted = codec::scan_descriptor(copy.get(), n, "image", &sc);
  if (!*accepted) return true;
  bool ok = true;
  try {
    codec::VPtr root = codec::parse(copy.get(), n);
    const codec::Value* d = root ? root->get("_btshm") : nullptr;
    if (!d || d->kind != codec::Value::TUPLE || int(d->items.size()) != sc.elems) return false;
    const bool has = d->items.size() == 11 && d->items[10]->kind == codec::Value::TUPLE && d->items[10]->items.size() == 2 &&
                     d->items[10]->items[0]->kind == codec::Value::INT && d->items[10]->items[1]->kind == codec::Value::BYTES;
    if (sc.band_rows > 0) {
      ok = has && d->items[10]->items[0]->i == sc.band_rows && d->items[10]->items[1]->len == sc.mask_bytes &&
           sc.mask >= copy.get() && sc.mask + sc.mask_bytes <= copy.get() + n &&
           std::memcmp(d->items[10]->items[1]->ptr(copy.get()), sc.mask, sc.mask_bytes) == 0;
    }
  } catch (const std::exception&) {
    // The scan checks the target of a SETITEM(S) / APPEND(S) only at the top level, so a mutation
    // that plants such an opcode deeper is accepted by the scan and refused by parse() (as in
    // fuzz_descriptor_scan.cpp).  Counted and reported, never silent: an unmutated message that
    // ends here is a failure (main), and the count over the mutations is bounded by the test.
    ++g_parse_threw;
  }
  if (out) out->band_rows = sc.band_rows, out->mask = sc.mask, out->bytes = sc.mask_bytes;
  if (keep) *keep = std::move(copy);
  return ok;
}

Tally render_mirrors(bool falling, int C, bool lower_left, int W, int H) {
  constexpr int K = 3;
  sim::Scene scene = falling ? sim::falling_cubes_scene() : sim::cube_scene();
  scene.cam.width = W, scene.cam.height = H;
  const size_t n = size_t(W) * H * size_t(C);
  sim::Renderer r(scene, C, lower_left);
  const int band_rows = blocks::band_rows_for(H), nb = blocks::bands(H, band_rows);
  int band_log2 = 0;
  while ((1 << band_log2) < band_rows) ++band_log2;
  const bool grid = blocks::geometry_ok(H, W, band_rows);
  // exact-size heap buffers: a copy past either end is an ASan report
  std::vector<std::unique_ptr<uint8_t[]>> buf, m_blk, m_clr;
  for (int k = 0; k < K; ++k) {
    buf.emplace_back(new uint8_t[n]), m_blk.emplace_back(new uint8_t[n]), m_clr.emplace_back(new uint8_t[n]);
    std::memset(buf[size_t(k)].get(), 0x5a, n);   // a slot that held anything
    std::memset(m_blk[size_t(k)].get(), 0xa5, n);
    std::memset(m_clr[size_t(k)].get(), 0xa5, n);
  }
  std::vector<sim::DirtyRect> dirty(K);
  std::vector<std::vector<uint16_t>> prev(K, std::vector<uint16_t>(size_t(nb), uint16_t(0)));
  std::vector<uint32_t> gen(K, 0u);
  mir::Ring ring(K);
  std::mt19937_64 rng(uint64_t(23 + C + W + (lower_left ? 100 : 0) + (falling ? 1000 : 0)));
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double pi = 3.14159265358979323846;
  Tally t;
  uint32_t next_gen = 1;
  for (int i = 0; i < 8 * K; ++i) {
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
    const uint32_t g = next_gen++;
    t.frames++;
    if (!grid) {   // W % 64 != 0: a producer sends no mask and a loader keeps the rectangle path
      CHECK(!blocks::width_ok(W));
      mir::BlockReport none;
      mir::BlockMask m;
      none.band_rows = band_rows;
      uint8_t z[2 * blocks::kMaxBands] = {};
      none.mask = z, none.bytes = size_t(2 * nb);
      CHECK(!mir::blocks_from_report(none, H, W, &m));
      continue;
    }
    // the producer: this frame's blocks, OR-ed with the ones the slot's last frame left
    uint16_t cur[blocks::kMaxBands] = {};
    sim::span_blocks(dirty[k], H, lower_left, band_log2, cur);
    uint8_t le[2 * blocks::kMaxBands];
    for (int b = 0; b < nb; ++b) {
      const uint16_t u = uint16_t(prev[k][size_t(b)] | cur[b]);
      le[2 * b] = uint8_t(u & 0xff), le[2 * b + 1] = uint8_t(u >> 8);
      prev[k][size_t(b)] = cur[b];
    }
    mir::Delta d;
    mir::BlockMask reported;
    bool has_report = false;
    std::unique_ptr<uint8_t[]> held;
    if (was_known) {
      const sim::StoredRect c = sim::changed_rect(before, dirty[k], H, lower_left);
      d.base_gen = gen[k];
      d.rect.y0 = c.y0, d.rect.y1 = c.y1, d.rect.x0 = c.x0, d.rect.x1 = c.x1;
      CHECK(mir::delta_valid(d, H, W));
      // through the wire: written, scanned, validated
      const codec::Bytes msg = message(g, d, H, W, C, band_rows, le, size_t(2 * nb));
      bool accepted = false;
      mir::BlockReport br;
      CHECK(scan_agrees(msg.data(), msg.size(), &accepted, &br, &held) && accepted);
      t.scans++;
      has_report = mir::blocks_from_report(br, H, W, &reported);
      CHECK(has_report);
      if (has_report) CHECK(inside(reported, mir::rect_blocks(mir::widen(d.rect, W), H), H));
    }
    // every 7th frame the consumer misses the slot's generation (a torn read): the report must be refused
    if (i % 7 == 6) ring.invalidate(uint32_t(k));
    bool used = false, masked = false;
    const mir::BlockMask m = ring.decide_blocks(uint32_t(k), g, was_known ? &d : nullptr, has_report ? &reported : nullptr, H,
                                                W, &used, &masked);
    CHECK(ring.holds(uint32_t(k), g));
    if (!used) CHECK(m.pixels(H) == int64_t(H) * W);
    copy_blocks(m_blk[k].get(), out, m, H, W, C);
    mir::BlockMask cl = m;
    if (masked) {
      t.reports++;
      t.fraction += double(m.pixels(H)) / (double(H) * W);
      for (int b = 0; b < nb; ++b)
        if (cl.w[b]) {
          cl.w[b] = uint16_t(cl.w[b] & (cl.w[b] - 1));
          break;
        }
    }
    copy_blocks(m_clr[k].get(), out, cl, H, W, C);
    gen[k] = g;
    t.masked += differing(m_blk[k].get(), out, n);
    t.cleared += differing(m_clr[k].get(), out, n);
  }
  return t;
}

void bookkeeping() {
  const int H = 480, W = 640;
  CHECK(blocks::band_rows_for(480) == 16 && blocks::bands(480, 16) == 30 && blocks::band_rows_for(40) == 2 && blocks::band_rows_for(30) == 1);
  CHECK(blocks::band_rows_for(241) == 16 && blocks::band_rows_for(240) == 8 && blocks::band_rows_for(2000) == 128);
  CHECK(blocks::geometry_ok(480, 640, 16) && !blocks::geometry_ok(480, 640, 8) && !blocks::geometry_ok(480, 640, 24));
  CHECK(!blocks::geometry_ok(480, 600, 16) && !blocks::geometry_ok(480, 1088, 16) && blocks::geometry_ok(480, 1024, 16));
  CHECK(blocks::column_bits(0, 63) == 1 && blocks::column_bits(64, 64) == 2 && blocks::column_bits(63, 64) == 3);
  CHECK(blocks::all_columns(640) == 0x3ff && blocks::all_columns(1024) == 0xffff && blocks::column_bits(960, 1023) == 0x8000);
  mir::Ring ring(4);
  mir::Delta d;
  d.base_gen = 7;
  d.rect.y0 = 100, d.rect.y1 = 200, d.rect.x0 = 70, d.rect.x1 = 130;
  mir::BlockMask rep;
  rep.band_rows = 16;
  rep.w[7] = 0x6, rep.w[12] = 0x2;
  bool used = true, masked = true;
  // first use: all ones
  mir::BlockMask m = ring.decide_blocks(1, 7, nullptr, nullptr, H, W, &used, &masked);
  CHECK(!used && !masked && m.band_rows == 16 && m.pixels(H) == int64_t(H) * W && ring.holds(1, 7));
  for (int k = 0; k < 30; ++k) CHECK(m.w[k] == 0x3ff);
  // base match with a mask: the mask
  m = ring.decide_blocks(1, 9, &d, &rep, H, W, &used, &masked);
  CHECK(used && masked && m.w[7] == 0x6 && m.w[12] == 0x2 && m.pixels(H) == 3 * 64 * 16 && ring.holds(1, 9));
  // base match without one: the widened rectangle's blocks (rows 100..200 -> bands 6..12, columns 64..191)
  d.base_gen = 9;
  m = ring.decide_blocks(1, 10, &d, nullptr, H, W, &used, &masked);
  CHECK(used && !masked && m.band_rows == 16 && m.pixels(H) == 7 * 16 * 128);
  for (int k = 0; k < 30; ++k) CHECK(m.w[k] == (k >= 6 && k <= 12 ? 0x6 : 0));
  // a mask on another grid: the rectangle
  d.base_gen = 10;
  mir::BlockMask other = rep;
  other.band_rows = 32;
  m = ring.decide_blocks(1, 11, &d, &other, H, W, &used, &masked);
  CHECK(used && !masked && m.band_rows == 16 && m.w[6] == 0x6);
  // base mismatch, invalidate: all ones whatever the report says
  m = ring.decide_blocks(1, 12, &d, &rep, H, W, &used, &masked);
  CHECK(!used && !masked && m.pixels(H) == int64_t(H) * W);
  d.base_gen = 12;
  ring.invalidate(1);
  m = ring.decide_blocks(1, 13, &d, &rep, H, W, &used, &masked);
  CHECK(!used && !masked && m.w[0] == 0x3ff);
  // an empty rectangle and an empty mask: nothing from the host
  d.base_gen = 13;
  d.rect = mir::Region();
  m = ring.decide_blocks(1, 14, &d, nullptr, H, W, &used, &masked);
  CHECK(used && !masked && m.pixels(H) == 0);
  d.base_gen = 14;
  mir::BlockMask zero;
  zero.band_rows = 16;
  m = ring.decide_blocks(1, 15, &d, &zero, H, W, &used, &masked);
  CHECK(used && masked && m.pixels(H) == 0);
  // a slot outside the ring: all ones, nothing recorded
  m = ring.decide_blocks(9, 1, &d, &rep, H, W, &used, &masked);
  CHECK(!used && m.pixels(H) == int64_t(H) * W && !ring.holds(9, 1));
  // reports: the length, the grid, bits past the last column block
  uint8_t le[2 * blocks::kMaxBands + 2] = {};
  le[14] = 0x06, le[61] = 0x00;
  mir::BlockReport br;
  br.band_rows = 16, br.mask = le, br.bytes = 60;
  mir::BlockMask got;
  CHECK(mir::blocks_from_report(br, H, W, &got) && got.band_rows == 16 && got.w[7] == 0x6 && got.pixels(H) == 2 * 64 * 16);
  br.bytes = 58;
  CHECK(!mir::blocks_from_report(br, H, W, &got));
  br.bytes = 62;
  CHECK(!mir::blocks_from_report(br, H, W, &got));
  br.bytes = 60, br.band_rows = 8;
  CHECK(!mir::blocks_from_report(br, H, W, &got));   // 60 bands
  br.band_rows = 24;
  CHECK(!mir::blocks_from_report(br, H, W, &got));   // no power of two
  br.band_rows = 0;
  CHECK(!mir::blocks_from_report(br, H, W, &got));
  br.band_rows = 16, br.mask = nullptr;
  CHECK(!mir::blocks_from_report(br, H, W, &got));
  br.mask = le, le[15] = 0x04;   // bit 10 of word 7: column block 10 of 10
  CHECK(!mir::blocks_from_report(br, H, W, &got));
  le[15] = 0x02;                 // bit 9: the last one
  CHECK(mir::blocks_from_report(br, H, W, &got) && got.w[7] == 0x206);
  CHECK(!mir::blocks_from_report(br, H, 600, &got) && !mir::blocks_from_report(br, H, 1088, &got));
  // a partial last band counts its own rows: H = 40, bands of 16, 16 and 8 rows
  mir::BlockMask p;
  p.band_rows = 16;
  p.w[2] = 0x1;
  CHECK(p.pixels(40) == 8 * 64);
  p.w[0] = 0x5;
  CHECK(p.pixels(40) == 8 * 64 + 2 * 16 * 64);
  mir::Region e;
  e.y0 = 31, e.y1 = 32, e.x0 = 64, e.x1 = 127;
  const mir::BlockMask rb = mir::rect_blocks(e, 40);   // grid of 2 rows: bands 15 and 16
  CHECK(rb.band_rows == 2 && rb.w[15] == 0x2 && rb.w[16] == 0x2 && rb.w[14] == 0 && rb.w[17] == 0 && rb.pixels(40) == 2 * 2 * 64);
  e.y0 = 100, e.y1 = 200;
  const mir::BlockMask rc = mir::rect_blocks(e, 250);  // grid of 16 rows, the last band holds 10: bands 6..12
  CHECK(rc.band_rows == 16 && rc.w[5] == 0 && rc.w[6] == 0x2 && rc.w[12] == 0x2 && rc.w[13] == 0 && rc.pixels(250) == 7 * 16 * 64);
}

// the scan over hostile variants of a message that carries the element
long scan_mutations() {
  mir::Delta d;
  d.base_gen = 5;
  d.rect.y0 = 3, d.rect.y1 = 40, d.rect.x0 = 10, d.rect.x1 = 200;
  uint8_t le[60];
  for (int i = 0; i < 60; ++i) le[i] = uint8_t(i * 7);
  long n = 0;
  bool acc = false;
  for (int with = 0; with < 2; ++with) {
    const codec::Bytes msg = message(6, d, 480, 640, 3, 16, with ? le : nullptr, 60);
    mir::BlockReport br;
    CHECK(scan_agrees(msg.data(), msg.size(), &acc, &br) && acc);
    CHECK((br.band_rows == 16 && br.bytes == 60) == (with == 1));
    for (size_t cut = 0; cut < msg.size(); ++cut, ++n) {
      CHECK(scan_agrees(msg.data(), cut, &acc));
      CHECK(!acc);
    }
    std::mt19937_64 rng(99 + uint64_t(with));
    for (int k = 0; k < 4000; ++k, ++n) {
      std::vector<uint8_t> m(msg.begin(), msg.end());
      // mutations aimed at the tail, where elements 10 and 11 lie
      const size_t lo = m.size() > 110 ? m.size() - 110 : 0;
      const int edits = 1 + int(rng() % 3);
      for (int e = 0; e < edits; ++e) {
        const size_t at = lo + size_t(rng() % (m.size() - lo));
        if (rng() % 2) m[at] = uint8_t(rng());
        else m[at] ^= uint8_t(1u << (rng() % 8));
      }
      CHECK(scan_agrees(m.data(), m.size(), &acc));
    }
  }
  // elements of other types in the 11th place: accepted, no mask
  for (int variant = 0; variant < 3; ++variant) {
    codec::Writer w(4);
    w.begin_dict();
    w.key("_btshm");
    w.begin_tuple();
    w.str("s"), w.integer(0), w.integer(0), w.integer(480), w.integer(640), w.integer(3), w.str("image"), w.integer(2);
    w.none();
    w.begin_tuple();
    for (int i = 0; i < 5; ++i) w.integer(i == 2 ? -1 : 0);
    w.end_tuple();
    if (variant == 0) w.none();
    else if (variant == 1) w.integer(16);
    else {
      w.begin_tuple();
      w.integer(16), w.str("not bytes");
      w.end_tuple();
    }
    w.end_tuple();
    w.end_dict();
    const codec::Bytes msg = w.finish();
    mir::BlockReport br;
    CHECK(scan_agrees(msg.data(), msg.size(), &acc, &br) && acc && br.band_rows == 0);
    ++n;
  }
  return n;
}

}  // namespace

int main() {
  Tally all;
  const int sizes[4][2] = {{128, 48}, {256, 40}, {640, 96}, {96, 48}};
  for (const auto& wh : sizes)
    for (int falling = 0; falling < 2; ++falling)
      for (int C = 3; C <= 4; ++C)
        for (int ll = 0; ll < 2; ++ll) {
          const Tally t = render_mirrors(falling != 0, C, ll != 0, wh[0], wh[1]);
          CHECK(t.masked == 0);
          if (wh[0] % 64 == 0) CHECK(t.cleared > 0 && t.reports > 0);   // the mutation is caught in every configuration
          else CHECK(t.reports == 0 && t.scans == 0);
          all.masked += t.masked, all.cleared += t.cleared, all.frames += t.frames, all.reports += t.reports;
          all.fraction += t.fraction, all.scans += t.scans;
        }
  bookkeeping();
  CHECK(g_parse_threw == 0);   // every message written here, unmutated, parses
  const long mutated = scan_mutations();
  std::printf("frames=%ld reports=%ld mean_fraction=%.3f scans=%ld mutated=%ld parse_threw=%ld\n", all.frames, all.reports,
              all.fraction / double(all.reports > 0 ? all.reports : 1), all.scans, mutated, g_parse_threw);
  std::printf("mask_mismatched=%ld cleared_detected=%d failed=%d\n", all.masked, all.cleared > 0 ? 1 : 0, g_failed);
  return g_failed == 0 ? 0 : 1;
}
