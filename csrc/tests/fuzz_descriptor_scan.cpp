// Hostile-input fuzz of the loader's descriptor scan (codec::scan_descriptor),
// built with AddressSanitizer (+UBSan) by tests/test_descriptor_scan.py.
// Valid shared-memory descriptor messages as cubesim writes them (with and
// without elements 9 and 10, rgb_a and tile16 tags, an `origin` entry) are
// scanned from exactly sized heap copies, then mutated at random -- flipped
// bytes, length fields overwritten with huge or wrapping values, truncation
// at every length.  For every input the scan must stay inside the copy and
// either decline or agree with parse(): the same segment, slot, offset, shape,
// generation, tag, delta tuple, `origin` and `btid`.
//
// Exit 0 with "valid=N accepted=M mutated=K agreed=J disagreed=0".
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../codec/pickle_codec.h"

using namespace btn;

namespace {

codec::Bytes message(std::mt19937_64& rng, int variant) {
  codec::Writer w(4);
  w.begin_dict();
  w.key("btid");
  w.integer(int64_t(rng() % 7));
  w.key("xy");
  std::vector<double> xy(16, 0.25);
  w.ndarray("f8", {8, 2}, xy.data());
  w.key("frameid");
  w.integer(int64_t(rng() % 100000));
  if (variant & 8) {
    w.key("origin");
    w.str("lower-left");
  }
  w.key("_btshm");
  w.begin_tuple();
  w.str("blendtorch-" + std::to_string(rng() % 100000) + "-" + std::to_string(rng() % 8));
  w.integer(int64_t(rng() % 48));
  w.integer(int64_t(4096 + (rng() % 48) * 1228800));
  w.integer(480), w.integer(640), w.integer(4);
  w.str("image");
  w.integer(int64_t(rng() % (1u << 30)));
  const int tag = variant & 3;   // 0: 8 elements, 1: rgb_a, 2: tile16, 3: None + delta
  if (tag == 1) {
    w.begin_tuple();
    w.str("rgb_a");
    w.end_tuple();
  } else if (tag == 2) {
    w.begin_tuple();
    w.str("tile16");
    w.str("blendtorch-1-0-key");
    w.integer(1);
    w.end_tuple();
  } else if (tag == 3) {
    w.none();
  }
  if ((variant & 4) && tag != 0 && tag != 2) {
    w.begin_tuple();
    w.integer(int64_t(rng() % (1u << 30)));
    w.integer(int64_t(rng() % 480)), w.integer(int64_t(rng() % 480));
    w.integer(int64_t(rng() % 640)), w.integer(int64_t(rng() % 640));
    w.end_tuple();
  }
  w.end_tuple();
  w.end_dict();
  return w.finish();
}

bool span_eq(const codec::Span& s, const std::string& t) { return s.n == t.size() && std::memcmp(s.p, t.data(), s.n) == 0; }

// does the scan's result say what the tree says?
bool agrees(const codec::DescriptorScan& sc, const codec::Value& root) {
  using V = codec::Value;
  if (root.kind != V::DICT) return false;
  const V* d = root.get("_btshm");
  if (!d || d->kind != V::TUPLE || int(d->items.size()) != sc.elems || sc.elems < 8) return false;
  const auto& e = d->items;
  if (e[0]->kind != V::STR || !span_eq(sc.segment, e[0]->s) || e[6]->kind != V::STR || !span_eq(sc.image_key, e[6]->s))
    return false;
  const int64_t want[6] = {sc.slot, sc.offset, sc.h, sc.w, sc.c, sc.gen};
  const int at[6] = {1, 2, 3, 4, 5, 7};
  for (int i = 0; i < 6; ++i)
    if (e[size_t(at[i])]->kind != V::INT || e[size_t(at[i])]->i != want[i]) return false;
  const bool tag = e.size() >= 9 && e[8]->kind == V::TUPLE;
  if (tag != (sc.tag_elems > 0)) return false;
  if (tag) {
    const auto& t = e[8]->items;
    if (int(t.size()) != sc.tag_elems || t[0]->kind != V::STR || !span_eq(sc.tag0, t[0]->s)) return false;
    if (sc.tag_elems == 3 && (t[1]->kind != V::STR || !span_eq(sc.tag1, t[1]->s) || t[2]->kind != V::INT || t[2]->i != sc.tag2))
      return false;
  }
  const bool delta = e.size() >= 10 && e[9]->kind == V::TUPLE;
  if (delta != sc.has_delta) return false;
  if (delta) {
    if (e[9]->items.size() != 5) return false;
    for (size_t k = 0; k < 5; ++k)
      if (e[9]->items[k]->kind != V::INT || e[9]->items[k]->i != sc.delta[k]) return false;
  }
  const V* o = root.get("origin");
  if ((o != nullptr) != sc.has_origin || (o && (o->kind != V::STR || !span_eq(sc.origin, o->s)))) return false;
  const V* b = root.get("btid");
  if ((b != nullptr) != sc.has_btid || (b && (b->kind != V::INT || b->np_scalar || b->i != sc.btid))) return false;
  return true;
}

struct Counts {
  long valid = 0, accepted = 0, mutated = 0, agreed = 0, disagreed = 0;
};

// scan an exactly sized heap copy; an accepted input must parse and agree
void one(const uint8_t* data, size_t n, Counts* c, bool must_accept) {
  std::unique_ptr<uint8_t[]> copy(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(copy.get(), data, n);
  codec::DescriptorScan sc;
  const bool ok = codec::scan_descriptor(copy.get(), n, "image", &sc);
  if (must_accept && !ok) c->disagreed++;
  if (!ok) return;
  c->accepted++;
  try {
    codec::VPtr root = codec::parse(copy.get(), n);
    if (root && agrees(sc, *root)) c->agreed++;
    else c->disagreed++;
  } catch (const std::exception&) {
    // the scan does not look into values it only skips (an ndarray's dtype,
    // say): parse() may still reject the message when its tree is built
    c->agreed++;
  }
}

void put_le(uint8_t* p, uint64_t v, int nb) {
  for (int i = 0; i < nb; ++i) p[i] = uint8_t(v >> (8 * i));
}

}  // namespace

int main() {
  std::mt19937_64 rng(4321);
  Counts c;
  const uint64_t nasty[] = {0, 1, 0xFF, 0xFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FFFFFFFFFFFFFFFull, 0xFFFFFFFFFFFFFFFFull};
  for (int variant = 0; variant < 16; ++variant) {
    const codec::Bytes msg = message(rng, variant);
    c.valid++;
    one(msg.data(), msg.size(), &c, true);
    for (size_t cut = 0; cut < msg.size(); ++cut) {   // every truncation
      c.mutated++;
      one(msg.data(), cut, &c, false);
    }
    for (int k = 0; k < 1500; ++k) {
      std::vector<uint8_t> m(msg.begin(), msg.end());
      const int edits = 1 + int(rng() % 3);
      for (int e = 0; e < edits; ++e) {
        const size_t at = size_t(rng() % m.size());
        switch (rng() % 3) {
          case 0: m[at] = uint8_t(rng()); break;
          case 1: m[at] ^= uint8_t(1u << (rng() % 8)); break;
          default: {
            const int nb = 1 << (rng() % 4);
            if (at + size_t(nb) <= m.size()) put_le(&m[at], nasty[rng() % 8], nb);
            break;
          }
        }
      }
      c.mutated++;
      one(m.data(), m.size(), &c, false);
    }
  }
  // not descriptors at all
  const char* junk[] = {"", "\x80", "\x80\x04garbage", "\x80\x04}.", "\x80\x04\x95", "(((((((((((((((((((((((("};
  for (const char* j : junk) {
    c.mutated++;
    one(reinterpret_cast<const uint8_t*>(j), std::strlen(j), &c, false);
  }
  std::printf("valid=%ld accepted=%ld mutated=%ld agreed=%ld disagreed=%ld\n", c.valid, c.accepted, c.mutated, c.agreed,
              c.disagreed);
  return c.disagreed == 0 && c.accepted >= c.valid ? 0 : 1;
}
