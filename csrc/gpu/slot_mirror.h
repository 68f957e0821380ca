// Slot mirror bookkeeping (host only, no HIP calls).
//
// The loader reads every ring slot again and again, and the producer rewrites
// only part of a slot between two uses.  With a byte copy of every slot in
// HBM (the "slot mirror") a decode needs only the rewritten part from the
// host.  The producer reports that part in descriptor element 10
// (shmring.h: kWantSlotDelta): (base_gen, y0, y1, x0, x1) -- every byte
// outside stored rows [y0, y1] x pixel columns [x0, x1] equals what the slot
// held when it was published with generation base_gen.
//
// A producer asked with kWantSlotBlocks adds element 11, (band_rows, mask):
// the same statement for the blocks of a 64-column x band_rows grid that are
// not set in the mask (csrc/common/block_mask.h) -- about two thirds of the
// widened rectangle's bytes for the cube frames.
//
// This header keeps, per mapped ring, which generation the mirror holds for
// every slot, and decides per frame which region or blocks the kernel has to
// read from the host (kernels.h: decode_delta, decode_delta_blocks -- one
// kernel body with two inside tests).  It never looks at pixels.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../common/block_mask.h"

namespace btn {
namespace gpu {
namespace mirror {

// Region of a frame in stored rows x pixel columns, inclusive.  Empty: y1 < y0.
struct Region {
  int y0 = 0, y1 = -1, x0 = 0, x1 = -1;
  bool empty() const { return y1 < y0 || x1 < x0; }
  int64_t pixels() const { return empty() ? 0 : int64_t(y1 - y0 + 1) * (x1 - x0 + 1); }
  bool whole(int H, int W) const { return y0 == 0 && x0 == 0 && y1 == H - 1 && x1 == W - 1; }
};

// Descriptor element 10.
struct Delta {
  uint32_t base_gen = 0;
  Region rect;
};

// A reported rectangle is either empty (y1 < y0: nothing changed) or lies in the frame.
inline bool delta_valid(const Delta& d, int H, int W) {
  const Region& r = d.rect;
  if (r.y1 < r.y0) return true;
  return r.y0 >= 0 && r.y1 < H && r.x0 >= 0 && r.x0 <= r.x1 && r.x1 < W;
}

// The kernel takes a lane's whole pixel group from one side, so a region
// starts and ends on multiples of kAlign pixels (or at the frame's edge):
// every run of region bytes then starts and ends on a 64-byte line for 3-
// and 4-byte pixels alike.
constexpr int kAlign = 64;

inline Region widen(const Region& r, int W) {
  if (r.empty()) return Region();
  Region o = r;
  if (W % kAlign != 0) {   // rows do not start on a block boundary: full rows
    o.x0 = 0, o.x1 = W - 1;
    return o;
  }
  o.x0 = r.x0 / kAlign * kAlign;
  o.x1 = (r.x1 / kAlign + 1) * kAlign - 1;
  if (o.x1 > W - 1) o.x1 = W - 1;
  return o;
}

// Descriptor element 11 as it lies in the message: `bytes` / 2 little-endian
// uint16 words, one per band of band_rows stored rows (csrc/common/block_mask.h).
struct BlockReport {
  int band_rows = 0;
  const uint8_t* mask = nullptr;
  size_t bytes = 0;
};

// A block mask on a grid of its own: bands(H, band_rows) words.
struct BlockMask {
  int band_rows = 0;
  uint16_t w[blocks::kMaxBands] = {};
  int64_t pixels(int H) const { return blocks::pixels(w, H, band_rows); }
};

// A reported mask that fits the frame -- a grid the kernel takes, one word per
// band, no bit past the last column block -- into *out.  False: malformed,
// which means "no mask" (the rectangle still holds), not an error.
inline bool blocks_from_report(const BlockReport& b, int H, int W, BlockMask* out) {
  if (!b.mask || !blocks::geometry_ok(H, W, b.band_rows)) return false;
  const int nb = blocks::bands(H, b.band_rows);
  if (b.bytes != size_t(2 * nb)) return false;
  const unsigned cols = blocks::all_columns(W);
  BlockMask m;
  m.band_rows = b.band_rows;
  for (int k = 0; k < nb; ++k) {
    const unsigned w = unsigned(b.mask[2 * k]) | (unsigned(b.mask[2 * k + 1]) << 8);
    if (w & ~cols) return false;
    m.w[k] = uint16_t(w);
  }
  *out = m;
  return true;
}

// The blocks a (widened) region touches, on the grid blocks::band_rows_for(H).
inline BlockMask rect_blocks(const Region& r, int H) {
  BlockMask m;
  m.band_rows = blocks::band_rows_for(H);
  if (r.empty()) return m;
  const uint16_t bits = blocks::column_bits(r.x0, r.x1);
  for (int k = r.y0 / m.band_rows; k <= r.y1 / m.band_rows; ++k) m.w[k] = bits;
  return m;
}

// HBM the mirrors of one loader may take.
class Budget {
 public:
  explicit Budget(size_t max_bytes = 0) : max_(max_bytes) {}
  bool reserve(size_t bytes) {
    if (bytes > max_ || used_ > max_ - bytes) return false;
    used_ += bytes;
    return true;
  }
  void release(size_t bytes) { used_ -= bytes <= used_ ? bytes : used_; }
  size_t used() const { return used_; }

 private:
  size_t max_, used_ = 0;
};

// One ring: the generation the mirror holds per slot.
class Ring {
 public:
  explicit Ring(uint32_t nslots = 0) : gen_(nslots, 0), held_(nslots, 0) {}
  uint32_t nslots() const { return uint32_t(gen_.size()); }
  bool holds(uint32_t slot, uint32_t gen) const { return slot < gen_.size() && held_[slot] && gen_[slot] == gen; }
  void invalidate(uint32_t slot) {
    if (slot < held_.size()) held_[slot] = 0;
  }
  // The region of generation `gen` of `slot` to read from the host: the
  // reported rectangle, widened, when the mirror holds the generation the
  // report is relative to; else the whole frame.  Afterwards the mirror
  // holds `gen` (the caller queues the kernel that makes it so).
  // *from_delta: the report was used.
  Region decide(uint32_t slot, uint32_t gen, const Delta* d, int H, int W, bool* from_delta = nullptr) {
    if (accept(slot, gen, d, H, W, from_delta)) return widen(d->rect, W);
    return Region{0, H - 1, 0, W - 1};
  }
  // decide() in blocks (decode_delta_blocks): the mask to read from the host,
  // always on the grid blocks::band_rows_for(H), one grid per launch -- the
  // reported one (blocks_from_report), when the mirror holds the generation
  // the report is relative to and the report is on that grid; else one built
  // from the reported rectangle, widened; else all ones.  The frame must admit a grid (blocks::width_ok(W)).
  // *from_delta: a report was used; *from_blocks: its mask was.
  BlockMask decide_blocks(uint32_t slot, uint32_t gen, const Delta* d, const BlockMask* reported, int H, int W,
                          bool* from_delta = nullptr, bool* from_blocks = nullptr) {
    BlockMask m;
    const bool use = accept(slot, gen, d, H, W, from_delta);
    const bool fine = use && reported && reported->band_rows == blocks::band_rows_for(H) && blocks::width_ok(W);
    if (fine) {
      m = *reported;
    } else if (use) {
      m = rect_blocks(widen(d->rect, W), H);
    } else {
      m.band_rows = blocks::band_rows_for(H);
      for (int k = 0, nb = blocks::bands(H, m.band_rows); k < nb; ++k) m.w[k] = blocks::all_columns(W);
    }
    if (from_blocks) *from_blocks = fine;
    return m;
  }

 private:
  // The step both decisions share: is the report usable (the mirror holds the
  // generation it is relative to, and its rectangle lies in the frame)?  Then
  // the mirror holds `gen` for the slot.
  bool accept(uint32_t slot, uint32_t gen, const Delta* d, int H, int W, bool* from_delta) {
    const bool use = d && holds(slot, d->base_gen) && delta_valid(*d, H, W);
    if (slot < gen_.size()) gen_[slot] = gen, held_[slot] = 1;
    if (from_delta) *from_delta = use;
    return use;
  }

  std::vector<uint32_t> gen_;
  std::vector<uint8_t> held_;
};

}  // namespace mirror
}  // namespace gpu
}  // namespace btn
