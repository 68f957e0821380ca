// cubesim -- headless stand-in for a Blender instance running
// examples/datagen/cube.blend.py (or falling_cubes.blend.py).
//
// Launch contract is the one BlenderLauncher hands to Blender scripts
// (reference: pkg_pytorch/blendtorch/btt/launcher.py:114-122, parsed by
// pkg_blender/blendtorch/btb/arguments.py:5-47):
//
//   cubesim [--] -btid I -btseed S -btsockets DATA=tcp://host:port [script args]
//
// Script args:  --scene cube|falling_cubes   --mode rgb|rgba   --origin
// upper-left|lower-left   --frame-range A B   --frames N (-1 = forever)
// --sndhwm N   --linger MS   --fps F (0 = unthrottled)   --socket NAME
// --fault none|exit|stall|garbage --fault-after N   --rotation RX RY RZ   --verbose
// --resolution WxH   --stamp (integrity tests: btid/seq in the first 16 image bytes)
// --lease-ms N       shm ring lease (default 30000): unclaimed slots reclaimed after starving N ms
// --shm N (render into an N-slot shared-memory ring, send descriptors only)
// --codec tile16 (shm frames as key-frame deltas, csrc/codec/tiledelta.h)
// --shm-layout auto|interleaved|planar  (RGBA shm frames, codec none; env
//   BLENDTORCH_SHM_LAYOUT): planar = packed RGB then the alpha plane (`rgb_a`,
//   csrc/common/planar_alpha.h); auto (default) follows the ring's consumer
//   hint frame by frame (shmring.h); where the layout does not apply (RGB
//   frames, tile16, H*W*3 % 16 != 0) frames stay interleaved
// --render-threads N (env BLENDTORCH_RENDER_THREADS): frames are drawn by N
//   workers and retired in order, so the stream is the same for any N (only
//   slot indices may differ); default min(2, CPUs this process may run on)
//   for a shared-memory ring with codec none -- used only while a consumer
//   has set the ring's kWantSlotDelta hint -- else 1; tile16 always 1
// --bench N (no sockets: render N frames into 8 rotating buffers, full vs
// incremental (DirtyRect) rendering, and report the byte mismatches -- 0;
// with --shm-layout planar the incremental frames are rgb_a slots, compared
// byte for byte in HWC order against the full 4-channel render; also 0: the
// bytes by which mirrors fed only the reported rectangle / blocks differ from
// their slot, and the bytes a render stores outside the blocks it reports;
// mask_share / span_mask_share: the mean share of the frame those blocks
// cover, and the blocks of both frames' spans)
//
// Every frame it publishes, on a bound PUSH socket with SNDHWM/LINGER/
// IMMEDIATE as btb.DataPublisher does (reference: btb/publisher.py:21-43),
// the pickled dict {'btid', 'image' (HxWxC u8), 'xy' (8*nboxes x 2 f8),
// 'frameid'} -- the same keys cube.blend.py publishes (reference:
// examples/datagen/cube.blend.py:17-24).  Pixels are rendered straight into
// the pickle payload, so a frame costs one render and zero extra copies
// before the kernel socket buffer.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <sched.h>
#include <unistd.h>
#include <map>
#include <mutex>
#include <optional>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../codec/pickle_codec.h"
#include "../codec/tiledelta.h"
#include "../common/block_mask.h"
#include "../common/planar_alpha.h"
#include "../transport/shmring.h"
#include "../transport/zmtp.h"
#include "physics.h"
#include "raster.h"

using namespace btn;

namespace {

std::atomic<bool> g_stop{false};
void on_signal(int) { g_stop = true; }

struct Args {
  int btid = 0;
  long long btseed = 0;
  std::map<std::string, std::string> sockets;
  std::string scene = "cube";
  std::string mode = "rgb";
  std::string origin = "upper-left";
  std::string socket = "DATA";
  int frame_start = 0, frame_end = 100;
  long long frames = -1;
  int sndhwm = 10;
  long linger = 0;
  double fps = 0;
  std::string fault = "none";
  long long fault_after = -1;
  bool verbose = false;
  int shm_slots = 0;        // >0: images go through a shared-memory ring
  std::string codec = "none";   // shm frames: none (raw HWC) | tile16 (key-frame delta, tiledelta.h)
  std::string shm_layout = "auto";   // RGBA shm frames: auto (ring hint) | interleaved | planar (rgb_a)
  bool fixed_rotation = false;
  double rot[3] = {0, 0, 0};
  int width = 0, height = 0;   // 0: the scene's resolution (640x480)
  bool stamp = false;          // integrity tests: (btid, seq) written into the first image row
  long lease_ms = 30000;       // shm ring: reclaim unclaimed slots after starving this long (shmring.h)
  long long bench = 0;         // >0: offline render benchmark / incremental-render check
  int render_threads = 0;      // 0: by rule (see above); N: that many render workers
};

[[noreturn]] void usage(const char* msg) {
  std::fprintf(stderr, "cubesim: %s\n", msg);
  std::exit(2);
}

Args parse(int argc, char** argv) {
  Args a;
  // BlenderLauncher(shm_slots=N) exports BLENDTORCH_SHM_SLOTS; --shm overrides
  if (const char* e = std::getenv("BLENDTORCH_SHM_SLOTS")) a.shm_slots = std::atoi(e);
  if (const char* e = std::getenv("BLENDTORCH_SHM_CODEC")) a.codec = e;   // BlenderLauncher(shm_codec=...)
  if (const char* e = std::getenv("BLENDTORCH_SHM_LAYOUT")) a.shm_layout = e;
  if (const char* e = std::getenv("BLENDTORCH_RENDER_THREADS")) a.render_threads = std::atoi(e);
  std::vector<std::string> v;
  int start = 1;
  for (int i = 1; i < argc; ++i)
    if (std::strcmp(argv[i], "--") == 0) {
      start = i + 1;
      break;
    }
  for (int i = start; i < argc; ++i) v.push_back(argv[i]);
  auto need = [&](size_t i) {
    if (i + 1 >= v.size()) usage(("missing value for " + v[i]).c_str());
    return v[i + 1];
  };
  for (size_t i = 0; i < v.size(); ++i) {
    const std::string& k = v[i];
    if (k == "-btid") a.btid = std::stoi(need(i)), ++i;
    else if (k == "-btseed") a.btseed = std::stoll(need(i)), ++i;
    else if (k == "-btsockets") {
      while (i + 1 < v.size() && v[i + 1].rfind("-", 0) != 0) {
        ++i;
        auto eq = v[i].find('=');
        if (eq == std::string::npos) usage("-btsockets expects NAME=ADDRESS");
        a.sockets[v[i].substr(0, eq)] = v[i].substr(eq + 1);
      }
    } else if (k == "--scene") a.scene = need(i), ++i;
    else if (k == "--mode") a.mode = need(i), ++i;
    else if (k == "--origin") a.origin = need(i), ++i;
    else if (k == "--socket") a.socket = need(i), ++i;
    else if (k == "--frame-range") {
      a.frame_start = std::stoi(need(i));
      a.frame_end = std::stoi(need(i + 1));
      i += 2;
    } else if (k == "--frames") a.frames = std::stoll(need(i)), ++i;
    else if (k == "--sndhwm") a.sndhwm = std::stoi(need(i)), ++i;
    else if (k == "--linger") a.linger = std::stol(need(i)), ++i;
    else if (k == "--fps") a.fps = std::stod(need(i)), ++i;
    else if (k == "--fault") a.fault = need(i), ++i;
    else if (k == "--fault-after") a.fault_after = std::stoll(need(i)), ++i;
    else if (k == "--verbose") a.verbose = true;
    else if (k == "--stamp") a.stamp = true;
    else if (k == "--lease-ms") a.lease_ms = std::stol(need(i)), ++i;
    else if (k == "--shm") a.shm_slots = std::stoi(need(i)), ++i;
    else if (k == "--codec") a.codec = need(i), ++i;
    else if (k == "--shm-layout") a.shm_layout = need(i), ++i;
    else if (k == "--bench") a.bench = std::stoll(need(i)), ++i;
    else if (k == "--render-threads") a.render_threads = std::stoi(need(i)), ++i;
    else if (k == "--resolution") {
      // WxH: render size (render.resolution_x/_y); the camera's field of view is kept
      const std::string r = need(i);
      const auto x = r.find('x');
      if (x == std::string::npos) usage("--resolution expects WxH");
      a.width = std::stoi(r.substr(0, x));
      a.height = std::stoi(r.substr(x + 1));
      if (a.width < 1 || a.height < 1) usage("bad --resolution");
      ++i;
    }
    else if (k == "--rotation") {
      if (i + 3 >= v.size()) usage("--rotation needs rx ry rz");
      for (int r = 0; r < 3; ++r) a.rot[r] = std::stod(v[i + 1 + r]);
      a.fixed_rotation = true;
      i += 3;
    }
    // unknown args are ignored, as Blender scripts ignore the remainder
  }
  if (a.mode != "rgb" && a.mode != "rgba") usage("--mode must be rgb or rgba");
  if (a.codec != "none" && a.codec != btn::tiledelta::kName) usage("--codec must be none or tile16");
  if (a.shm_layout != "auto" && a.shm_layout != "interleaved" && a.shm_layout != "planar")
    usage("--shm-layout must be auto, interleaved or planar");
  if (a.origin != "upper-left" && a.origin != "lower-left") usage("bad --origin");
  return a;
}

// Recycles frame storage: a sent frame's buffer returns here once the IO
// thread has written it, so steady state allocates nothing.
struct FramePool {
  std::mutex mu;
  std::vector<codec::Bytes*> free;
  codec::Bytes take() {
    std::lock_guard<std::mutex> lk(mu);
    if (free.empty()) return {};
    codec::Bytes v(std::move(*free.back()));
    delete free.back();
    free.pop_back();
    return v;
  }
  void give(codec::Bytes* v) {
    std::lock_guard<std::mutex> lk(mu);
    if (free.size() < 64) free.push_back(v);
    else delete v;
  }
};
FramePool g_pool;

zmtp::Frame frame_from_vector(codec::Bytes&& v) {
  auto* owned = new codec::Bytes(std::move(v));
  auto b = std::make_shared<Buffer>();
  b->data = owned->data();
  b->capacity = owned->size();
  b->owner = owned;
  b->release = [](void* o, Buffer*) { g_pool.give(static_cast<codec::Bytes*>(o)); };
  zmtp::Frame f;
  f.size = owned->size();
  f.buf = std::move(b);
  return f;
}

// --bench N: the render loop without sockets.  Every frame is rendered twice,
// once in full into a scratch buffer and once incrementally into the next of
// 8 rotating buffers (a ring slot's life; the full renders rotate over 8
// buffers of their own); both timings and the number of
// differing bytes (must be 0) are printed.
// A slot's alpha plane in the rgb_a layout.  raster.h guarantees alpha = 255
// everywhere, so the plane is written only when the slot last held something
// else (and by --stamp).
void fill_alpha_plane(uint8_t* slot, size_t npix) { std::memset(slot + npix * 3, 255, npix); }

template <class Pose>
int bench(const Args& a, sim::Scene& scene, sim::Renderer& r, Pose& pose, sim::Renderer* planar) {
  const size_t n = size_t(r.width()) * r.height() * r.channels();
  const size_t npix = size_t(r.width()) * r.height();
  constexpr int kSlots = 8;
  std::vector<std::vector<uint8_t>> slots(kSlots, std::vector<uint8_t>(n));
  std::vector<sim::DirtyRect> dirty(kSlots);
  std::vector<std::vector<uint8_t>> fulls(kSlots, std::vector<uint8_t>(n));   // as cold as the slots
  // a byte mirror per slot, updated only inside the rectangle a consumer
  // would be told about (changed_rect: descriptor element 10): it must stay
  // equal to the slot
  std::vector<std::vector<uint8_t>> mirrors(kSlots, std::vector<uint8_t>(n));
  // and one updated only inside the blocks the render reports (element 11)
  std::vector<std::vector<uint8_t>> block_mirrors(kSlots, std::vector<uint8_t>(n));
  const int mc = planar ? 3 : r.channels();      // channels of the bytes a rectangle covers (rgb_a: the RGB part)
  const bool lower_left = a.origin == "lower-left";
  const int W = r.width(), H = r.height();
  const int band_rows = blocks::band_rows_for(H), nbands = blocks::bands(H, band_rows);
  int band_log2 = 0;
  while ((1 << band_log2) < band_rows) ++band_log2;
  const bool blocks_ok = blocks::geometry_ok(H, W, band_rows);   // else: no masks, the block figures stay 0
  // visits the bytes [o, o + len) of every set (inside) or clear block of `mask`
  auto for_blocks = [&](const uint16_t* mask, bool inside, auto&& f) {
    for (int y = 0; y < H; ++y)
      for (int c = 0; c < W / blocks::kBlockCols; ++c)
        if (((mask[y >> band_log2] >> c) & 1) == (inside ? 1 : 0))
          f((size_t(y) * W + size_t(c) * blocks::kBlockCols) * size_t(mc), size_t(blocks::kBlockCols) * size_t(mc));
  };
  std::vector<uint16_t> span_prev(size_t(kSlots) * blocks::kMaxBands, uint16_t(0));
  std::vector<uint8_t> probe(n);
  double t_full = 0, t_inc = 0, mask_share = 0, span_share = 0;
  long long mismatches = 0, mirror_mismatches = 0, block_mirror_mismatches = 0, stores_outside = 0, masked = 0;
  uint64_t h = 1469598103934665603ull;   // FNV-1a over every incremental frame
  int frame = a.frame_start;
  for (long long i = 0; i < a.bench; ++i) {
    pose(frame);
    frame = frame >= a.frame_end ? a.frame_start : frame + 1;
    const uint8_t* full = fulls[size_t(i % kSlots)].data();
    // both renders report their blocks: the same bookkeeping in either timing
    uint16_t wr_full[blocks::kMaxBands] = {}, wr[blocks::kMaxBands] = {};
    sim::DirtyRect& rec = dirty[size_t(i % kSlots)];
    const sim::DirtyRect rec_before = rec;   // (the record only: the slot stays cold)
    const bool was_known = rec.known;
    auto t0 = std::chrono::steady_clock::now();
    r.render(scene, fulls[size_t(i % kSlots)].data(), nullptr, blocks_ok ? wr_full : nullptr, band_log2);
    auto t1 = std::chrono::steady_clock::now();
    uint8_t* out = slots[size_t(i % kSlots)].data();
    if (planar) {
      if (!rec.known) fill_alpha_plane(out, npix);
      planar->render(scene, out, &rec, blocks_ok ? wr : nullptr, band_log2);
    } else {
      r.render(scene, out, &rec, blocks_ok ? wr : nullptr, band_log2);
    }
    auto t2 = std::chrono::steady_clock::now();
    t_full += std::chrono::duration<double, std::milli>(t1 - t0).count();
    t_inc += std::chrono::duration<double, std::milli>(t2 - t1).count();
    uint8_t* mir = mirrors[size_t(i % kSlots)].data();
    if (blocks_ok) {
      uint16_t cur[blocks::kMaxBands] = {};
      sim::span_blocks(rec, H, lower_left, band_log2, cur);
      uint16_t* sp = &span_prev[size_t(i % kSlots) * blocks::kMaxBands];
      if (was_known) {
        uint16_t u[blocks::kMaxBands];
        for (int k = 0; k < nbands; ++k) u[k] = uint16_t(sp[k] | cur[k]);
        span_share += double(blocks::pixels(u, H, band_rows)) / double(npix);
        mask_share += double(blocks::pixels(wr, H, band_rows)) / double(npix);
        ++masked;
        // no store outside the mask: the slot as it was (the rectangle mirror,
        // not yet brought up to date), every byte outside the mask replaced by
        // a sentinel, rendered with a copy of the record the slot had -- with
        // two sentinels, since a store may write either value
        for (const uint8_t sentinel : {uint8_t(0xa5), uint8_t(0x5a)}) {
          std::memcpy(probe.data(), mir, n);
          for_blocks(wr, false, [&](size_t o, size_t len) { std::memset(probe.data() + o, sentinel, len); });
          sim::DirtyRect rec_probe = rec_before;
          (planar ? planar : &r)->render(scene, probe.data(), &rec_probe);
          for_blocks(wr, false, [&](size_t o, size_t len) {
            for (size_t k = o; k < o + len; ++k) stores_outside += probe[k] != sentinel;
          });
        }
      }
      std::memcpy(sp, cur, sizeof(cur));
      uint8_t* bm = block_mirrors[size_t(i % kSlots)].data();
      if (!was_known) std::memcpy(bm, out, n);
      else for_blocks(wr, true, [&](size_t o, size_t len) { std::memcpy(bm + o, out + o, len); });
      for (size_t k = 0; k < n; ++k) block_mirror_mismatches += bm[k] != out[k];
    }
    {
      if (!was_known) {
        std::memcpy(mir, out, n);   // a slot's first frame is taken whole
      } else {
        const sim::StoredRect c = sim::changed_rect(rec_before, rec, r.height(), lower_left);
        for (int y = c.y0; !c.empty() && y <= c.y1; ++y) {
          const size_t o = (size_t(y) * r.width() + size_t(c.x0)) * size_t(mc);
          std::memcpy(mir + o, out + o, size_t(c.x1 - c.x0 + 1) * size_t(mc));
        }
      }
      for (size_t k = 0; k < n; ++k) mirror_mismatches += mir[k] != out[k];
    }
    // compared (and hashed) in the frame's logical HWC byte order; a planar
    // slot is read where it lies, so both layouts touch the same memory here
    for (size_t k = 0; k < n; ++k) {
      const uint8_t v = !planar ? out[k] : ((k & 3) == 3 ? out[npix * 3 + (k >> 2)] : out[(k >> 2) * 3 + (k & 3)]);
      mismatches += v != full[k];
      h = (h ^ v) * 1099511628211ull;
    }
  }
  std::printf("{\"frames\": %lld, \"full_ms\": %.4f, \"incremental_ms\": %.4f, \"mismatched_bytes\": %lld, "
              "\"mirror_mismatched_bytes\": %lld, \"block_mirror_mismatched_bytes\": %lld, "
              "\"stores_outside_mask\": %lld, \"mask_share\": %.4f, \"span_mask_share\": %.4f, "
              "\"checksum\": \"%016llx\", \"isa\": \"%s\"}\n",
              a.bench, t_full / a.bench, t_inc / a.bench, mismatches, mirror_mismatches, block_mirror_mismatches,
              stores_outside, mask_share / double(std::max(masked, 1ll)), span_share / double(std::max(masked, 1ll)),
              (unsigned long long)h, sim::raster_isa());
  return mismatches == 0 && mirror_mismatches == 0 && block_mirror_mismatches == 0 && stores_outside == 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
  Args a = parse(argc, argv);
  if (a.bench <= 0 && !a.sockets.count(a.socket)) usage(("no -btsockets entry named " + a.socket).c_str());
  std::signal(SIGTERM, on_signal);
  std::signal(SIGINT, on_signal);

  sim::Scene scene = a.scene == "falling_cubes" ? sim::falling_cubes_scene() : sim::cube_scene();
  if (a.width > 0) scene.cam.width = a.width, scene.cam.height = a.height;
  const int W = scene.cam.width, H = scene.cam.height, C = a.mode == "rgba" ? 4 : 3;
  std::mt19937_64 rng(uint64_t(a.btseed));
  std::uniform_real_distribution<double> U(0.0, 1.0);
  const double pi = 3.14159265358979323846;
  if (a.scene == "falling_cubes") {
    for (auto& b : scene.boxes)
      b.albedo = {float(U(rng)), float(U(rng)), float(U(rng))};
  }

  sim::RigidWorld physics(scene.plane_z);
  // pre_animation / pre_frame: randomise the pose(s)
  auto pose = [&](int frame) {
    if (a.scene == "falling_cubes") {
      // pre_animation: re-drop every cube at a random pose, as
      // falling_cubes.blend.py does (xyz ~ U((-3,-3,6),(3,3,12)), euler ~ U(-pi,pi));
      // every later frame advances the rigid-body world by one scene frame
      if (frame == a.frame_start) {
        for (auto& b : scene.boxes) {
          b.center = {-3 + 6 * U(rng), -3 + 6 * U(rng), 6 + 6 * U(rng)};
          b.rot = sim::euler_xyz(-pi + 2 * pi * U(rng), -pi + 2 * pi * U(rng), -pi + 2 * pi * U(rng));
        }
        physics.reset(scene.boxes);
      } else {
        physics.step(scene.boxes, 1.0 / 60.0);
      }
    } else if (a.fixed_rotation) {
      scene.boxes[0].rot = sim::euler_xyz(a.rot[0], a.rot[1], a.rot[2]);
    } else {
      scene.boxes[0].rot = sim::euler_xyz(pi * U(rng), pi * U(rng), pi * U(rng));
    }
  };
  const bool lower_left = a.origin == "lower-left";
  // one Renderer per stored layout, built when first used: the frame's own
  // channels (interleaved), and 3 channels for the RGB part of rgb_a slots
  std::unique_ptr<sim::Renderer> renderer_hwc, renderer_rgb;
  auto renderer = [&]() -> sim::Renderer& {
    if (!renderer_hwc) renderer_hwc.reset(new sim::Renderer(scene, C, lower_left));
    return *renderer_hwc;
  };
  auto planar_renderer = [&]() -> sim::Renderer& {
    if (!renderer_rgb) renderer_rgb.reset(new sim::Renderer(scene, 3, lower_left));
    return *renderer_rgb;
  };
  const bool planar_ok = planar::supported(H, W, C);
  if (a.bench > 0)
    return bench(a, scene, renderer(), pose, a.shm_layout == "planar" && planar_ok ? &planar_renderer() : nullptr);

  auto sock = zmtp::Context::global().socket(zmtp::PUSH);
  sock->setsockopt(zmtp::SNDHWM, a.sndhwm);
  sock->setsockopt(zmtp::LINGER, a.linger);
  sock->setsockopt(zmtp::IMMEDIATE, 1);
  sock->bind(a.sockets[a.socket]);

  const zmtp::Socket::Interrupt intr = [] { return g_stop.load(); };
  std::unique_ptr<shm::Segment> seg, key_seg;
  // key-frame delta codec: the background goes once into a segment of its
  // own, every frame into its slot as a tile map + the tiles that differ
  bool tiled = a.shm_slots > 0 && a.codec == tiledelta::kName && tiledelta::supported(H, W, C);
  if (a.shm_slots > 0) {
    const std::string name = "blendtorch-" + std::to_string(::getpid()) + "-" + std::to_string(a.btid);
    try {
      const size_t raw = size_t(W) * H * C;
      seg.reset(shm::Segment::create(name, uint32_t(a.shm_slots), tiled ? std::max(raw, tiledelta::max_bytes(H, W, C)) : raw));
      if (tiled) {
        key_seg.reset(shm::Segment::create(name + "-key", 1, raw));
        const int k = key_seg->acquire(0);
        std::memcpy(key_seg->slot(uint32_t(k)), renderer().background().data(), raw);
        key_seg->publish(uint32_t(k));   // stays published: consumers only read it
      }
    } catch (const std::exception& e) {
      // e.g. a small /dev/shm: fall back to inline payloads
      std::fprintf(stderr, "cubesim[%d]: shared memory disabled (%s)\n", a.btid, e.what());
      seg.reset(), key_seg.reset(), tiled = false;
    }
  }
  std::vector<uint8_t> tiled_frame(tiled ? size_t(W) * H * C : 0);   // the full frame, rendered incrementally
  sim::DirtyRect tiled_dirty;
  // what each ring slot's last frame drew over the background: a slot is
  // re-rendered by restoring that rectangle only (BLENDTORCH_FULL_RENDER=1: off)
  const char* full_env = std::getenv("BLENDTORCH_FULL_RENDER");
  const bool incremental = !(full_env && std::atoi(full_env) != 0);
  std::vector<sim::DirtyRect> slot_dirty(seg ? size_t(a.shm_slots) : 0);
  // which layout each slot last held: a slot whose layout changes holds
  // unknown content (full background copy; alpha plane filled for rgb_a)
  enum SlotLayout : uint8_t { kUnknown = 0, kInterleaved = 1, kPlanar = 2 };
  std::vector<uint8_t> slot_layout(seg ? size_t(a.shm_slots) : 0, uint8_t(kUnknown));
  // kWantSlotDelta (shmring.h): the generation each slot was last published
  // with by THIS producer (0: never, or not to be relied on) -- kept here, not
  // read back from the slot word, which a lease reclaim bumps
  std::vector<uint32_t> slot_gen(seg ? size_t(a.shm_slots) : 0, 0u);
  // kWantSlotBlocks (shmring.h): a frame's report is the blocks its render
  // stored into (Renderer::render's `written`, and the stamp's)
  const int band_rows = blocks::band_rows_for(H), nbands = blocks::bands(H, band_rows);
  int band_log2 = 0;
  while ((1 << band_log2) < band_rows) ++band_log2;
  const bool blocks_ok = seg && !tiled && incremental && blocks::geometry_ok(H, W, band_rows);
  const size_t npix = size_t(W) * H;
  const auto t_start = std::chrono::steady_clock::now();
  auto next_due = t_start;
  long long published = 0;
  int frame = a.frame_start;
  double render_ms = 0;

  // Render workers.  A frame has three parts: a front half on the main thread
  // (slot acquire, pose -- the RNG, in frame order -- and the metadata part of
  // the message), the render, and a retire step on the main thread (the
  // descriptor, publish, faults, send), strictly in dispatch order.  With T
  // workers up to T + 1 frames are between front half and retire, each in a
  // slot of its own, so what a consumer receives does not depend on T (only
  // the slot indices may).  slot_dirty, slot_layout and slot_gen
  // are touched for a slot only between its acquire and its retire, by the
  // one frame that holds it.  T = 1 renders on the main thread: the loop of a
  // single-threaded producer.  tile16 frames build on one another: T = 1.
  // A worker count taken by rule (no --render-threads) is used only while a
  // consumer of the ring has set kWantSlotDelta: a loader that reads slots in
  // place with a mirror can outrun one render thread, whereas behind a copy
  // path or a training step the second thread would only take CPU from the
  // consumer -- such a producer draws on its main thread, frame by frame.
  const bool by_rule = a.render_threads <= 0;
  int T = a.render_threads;
  if (T <= 0) {
    int cpus = 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = std::max(1, CPU_COUNT(&set));
    T = seg && !tiled && a.codec == "none" ? std::min(2, cpus) : 1;
  }
  if (tiled) T = 1;
  T = std::min(T, 16);

  struct Job {
    long long seq = 0;        // dispatch index: the value of `published` when the frame retires
    int frame = 0;
    int slot = -1;
    bool planar = false;
    sim::Scene scene;         // T > 1: the pose to draw (the main thread's scene has moved on)
    std::optional<codec::Writer> w;
    size_t img_off = 0;
    uint8_t* pixels = nullptr;
    bool delta_known = false;   // ring slot of known content, published by this producer with a known generation
    sim::StoredRect changed;
    bool has_mask = false;
    uint16_t mask[blocks::kMaxBands] = {};
    double ms = 0;
    bool done = false;        // guarded by `mu`
  };
  struct RenderSet {          // one Renderer per stored layout, built when first used
    std::unique_ptr<sim::Renderer> hwc, rgb;
  };

  // ---- front half ----
  long long dispatched = 0;
  const bool garbage_fault = a.fault == "garbage" && a.fault_after >= 0;
  auto front = [&](Job& j, int slot) {
    pose(frame);
    j.seq = dispatched++;
    j.frame = frame;
    j.slot = slot;
    j.delta_known = false, j.has_mask = false, j.changed = sim::StoredRect(), j.ms = 0, j.done = false;
    if (T > 1) {
      if (j.scene.boxes.empty()) j.scene = scene;   // camera, light and plane never change
      else j.scene.boxes = scene.boxes;
    }
    // this frame's layout: rgb_a when the ring's consumers all read RGB in
    // place (the hint is re-read every frame: consumers come and go)
    j.planar = false;
    if (seg && !tiled && planar_ok && a.shm_layout != "interleaved")
      j.planar = a.shm_layout == "planar" || (seg->hint() & 3u) == shm::kWantPlanarAlpha;
    j.w.emplace(4, g_pool.take());
    codec::Writer& w = *j.w;
    w.begin_dict();
    w.key("btid");
    w.integer(a.btid);
    j.img_off = 0;
    if (!seg) {
      w.key("image");
      j.img_off = w.ndarray("u1", {H, W, C}, nullptr, 64);   // 64-byte aligned payload: zero-copy GPU reads
    }
    w.key("xy");
    std::vector<double> xy;
    for (auto& b : scene.boxes)
      for (auto& c : b.corners()) {
        double px = 0, py = 0;
        scene.cam.project(c, &px, &py);
        xy.push_back(px);
        xy.push_back(py);
      }
    w.ndarray("f8", {int64_t(xy.size() / 2), 2}, xy.data());
    w.key("frameid");
    w.integer(frame);
    if (a.stamp) {
      w.key("seq");
      w.integer(j.seq);
    }
    if (lower_left) {
      w.key("origin");
      w.str("lower-left");
    }
    // A ring frame is drawn BEFORE its descriptor is written (the descriptor
    // reports what the render changed), an inline frame after: its pixels
    // live in the message itself.
    if (seg) {
      j.pixels = seg->slot(uint32_t(slot));
    } else {
      w.end_dict();
      j.pixels = w.finish().data() + j.img_off;
    }
    // (a frame that goes out as garbage does not advance the scene frame)
    if (!(garbage_fault && j.seq == a.fault_after)) frame = frame >= a.frame_end ? a.frame_start : frame + 1;
  };

  // ---- render: `s` is the pose, `rs` the calling thread's renderers ----
  auto draw = [&](Job& j, const sim::Scene& s, RenderSet& rs) {
    const auto r0 = std::chrono::steady_clock::now();
    const int slot = j.slot;
    const bool planar = j.planar;
    uint8_t* pixels = j.pixels;
    sim::DirtyRect before;       // ring slot of known content: the rectangle its last frame left
    sim::DirtyRect* dirty = tiled ? &tiled_dirty : (seg && incremental ? &slot_dirty[size_t(slot)] : nullptr);
    uint8_t* const slot_bytes = pixels;
    if (tiled) pixels = tiled_frame.data();
    if (seg && !tiled) {
      uint8_t& held = slot_layout[size_t(slot)];
      const uint8_t now = planar ? kPlanar : kInterleaved;
      if (held != now) {
        slot_dirty[size_t(slot)] = sim::DirtyRect();   // unknown content: full background copy
        if (planar) fill_alpha_plane(pixels, npix);
        held = now;
      }
      // what the slot's known content is about to lose (render() restores
      // it) -- together with what this frame leaves, all that changes
      if (dirty && dirty->known) {
        before.x0 = dirty->x0, before.y0 = dirty->y0, before.x1 = dirty->x1, before.y1 = dirty->y1;
        j.delta_known = slot_gen[size_t(slot)] != 0;
      }
    }
    std::unique_ptr<sim::Renderer>& r = planar ? rs.rgb : rs.hwc;
    if (!r) r.reset(new sim::Renderer(s, planar ? 3 : C, lower_left));
    const bool masked = blocks_ok && dirty;
    if (masked) std::memset(j.mask, 0, sizeof(j.mask));
    r->render(s, pixels, dirty, masked ? j.mask : nullptr, band_log2);
    if (a.stamp) {
      // bytes 0..15 of the stored image (first stored row): 'B','T', btid (u16 LE),
      // 4 zero bytes, seq (u64 LE) -- lets tests match every decoded image to its metadata
      uint8_t st[16] = {'B', 'T', uint8_t(a.btid & 0xff), uint8_t((a.btid >> 8) & 0xff), 0, 0, 0, 0};
      const uint64_t q = uint64_t(j.seq);
      std::memcpy(st + 8, &q, 8);
      if (planar) {
        // the same 16 logical HWC bytes: pixels 0..3, their alpha (bytes 3, 7,
        // 11, 15) in the alpha plane -- rewritten every frame, never restored
        for (int p = 0; p < 4; ++p) {
          std::memcpy(pixels + 3 * p, st + 4 * p, 3);
          pixels[npix * 3 + size_t(p)] = st[4 * p + 3];
          const int row = p / W, col = p % W;   // stored row / column of pixel p
          if (dirty) dirty->foreign(lower_left ? H - 1 - row : row, col, col);
          if (masked) j.mask[row >> band_log2] |= blocks::column_bits(col, col);
        }
      } else {
        std::memcpy(pixels, st, sizeof(st));
        if (dirty) dirty->foreign(lower_left ? H - 1 : 0, 0, (int(sizeof(st)) + C - 1) / C - 1);
        if (masked) j.mask[0] |= blocks::column_bits(0, (int(sizeof(st)) + C - 1) / C - 1);
      }
    }
    if (tiled) {
      // everything outside this frame's dirty rectangle is background
      if (tiled_dirty.empty())
        tiledelta::encode(pixels, key_seg->slot(0), H, W, C, 0, -1, 0, -1, slot_bytes);
      else if (lower_left)   // DirtyRect rows are image rows (0 = top); stored rows are flipped
        tiledelta::encode(pixels, key_seg->slot(0), H, W, C, H - 1 - tiled_dirty.y1, H - 1 - tiled_dirty.y0,
                          tiled_dirty.x0, tiled_dirty.x1, slot_bytes);
      else
        tiledelta::encode(pixels, key_seg->slot(0), H, W, C, tiled_dirty.y0, tiled_dirty.y1, tiled_dirty.x0,
                          tiled_dirty.x1, slot_bytes);
    }
    if (j.delta_known) j.changed = sim::changed_rect(before, *dirty, H, lower_left);
    // the mask holds every block this frame's render or stamp stored into:
    // all else is what the slot held one generation earlier
    j.has_mask = masked && j.delta_known;
    j.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r0).count();
  };

  // ---- retire: false ends the stream ----
  auto retire = [&](Job& j) -> bool {
    const auto r0 = std::chrono::steady_clock::now();
    const int slot = j.slot;
    codec::Writer& w = *j.w;
    if (seg) {
      // descriptor: (segment, slot, byte offset, H, W, C, image key, generation)
      const uint32_t gen = ((seg->state(uint32_t(slot)) >> 2) + 1) & 0x3fffffffu;   // publish() will bump to this
      w.key("_btshm");
      w.begin_tuple();
      w.str(seg->name());
      w.integer(slot);
      w.integer(int64_t(seg->slot_offset(uint32_t(slot))));
      w.integer(H);
      w.integer(W);
      w.integer(C);
      w.str("image");
      w.integer(gen);
      if (tiled) {   // 9th element: (codec, key segment, key generation)
        w.begin_tuple();
        w.str(tiledelta::kName);
        w.str(key_seg->name());
        w.integer(int64_t(key_seg->state(0) >> 2));
        w.end_tuple();
      } else if (j.planar) {   // 9th element: (layout,)
        w.begin_tuple();
        w.str(planar::kName);
        w.end_tuple();
      }
      // 10th element (base_gen, y0, y1, x0, x1) for a consumer that keeps slot
      // copies (shmring.h: kWantSlotDelta); never for tile16 frames, a full
      // render or a slot whose content or layout is not the one last published
      const uint32_t hint = seg->hint();
      if (!tiled && j.delta_known && (hint & shm::kWantSlotDelta)) {
        if (!j.planar) w.none();   // interleaved frames have no 9th element: a non-tuple means "no codec"
        const sim::StoredRect& changed = j.changed;
        w.begin_tuple();
        w.integer(slot_gen[size_t(slot)]);
        w.integer(changed.empty() ? 0 : changed.y0);
        w.integer(changed.empty() ? -1 : changed.y1);
        w.integer(changed.empty() ? 0 : changed.x0);
        w.integer(changed.empty() ? -1 : changed.x1);
        w.end_tuple();
        // 11th element (band_rows, mask) where the consumer asked for it
        // (shmring.h: kWantSlotBlocks) and the frame's size allows a mask
        if (j.has_mask && (hint & shm::kWantSlotBlocks)) {
          uint8_t le[2 * blocks::kMaxBands];
          for (int k = 0; k < nbands; ++k) le[2 * k] = uint8_t(j.mask[k] & 0xff), le[2 * k + 1] = uint8_t(j.mask[k] >> 8);
          w.begin_tuple();
          w.integer(band_rows);
          w.bytes(le, size_t(2 * nbands));
          w.end_tuple();
        }
      }
      w.end_tuple();
      w.end_dict();
      w.finish();
      seg->publish(uint32_t(slot));   // == gen
      slot_gen[size_t(slot)] = gen;
    }
    auto& buf = w.buffer();
    render_ms += j.ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - r0).count();

    if (a.fault != "none" && a.fault_after >= 0 && published == a.fault_after) {
      if (a.fault == "exit") std::_Exit(3);
      if (a.fault == "stall") {
        while (!g_stop) std::this_thread::sleep_for(std::chrono::milliseconds(50));
        return false;
      }
      if (a.fault == "garbage") {
        zmtp::Message m;
        m.push_back(zmtp::Frame::copy_of("\x80\x04garbage", 9));
        try {
          sock->send(std::move(m), 0, intr);
        } catch (const zmtp::Error&) {
          return false;
        }
        if (seg) {
          seg->release(uint32_t(slot), seg->publish(uint32_t(slot)));
          slot_gen[size_t(slot)] = 0;   // published twice: no consumer saw a generation to refer to
        }
        ++published;
        return true;
      }
    }

    zmtp::Message msg;
    msg.push_back(frame_from_vector(std::move(buf)));
    try {
      sock->send(std::move(msg), 0, intr);   // blocks at SNDHWM: backpressure
    } catch (const zmtp::Error& e) {
      if (e.code == zmtp::E_INTR) return false;
      std::fprintf(stderr, "cubesim[%d]: send failed: %s\n", a.btid, e.what());
      return false;
    }
    ++published;
    if (a.fps > 0) {
      // a stall (no consumer connected yet, a full ring or pipe) is not made
      // up for by a burst afterwards: the pace resumes from now.  Otherwise
      // the wait for the first consumer alone left a paced producer a few
      // hundred frames "behind", i.e. unpaced for as long
      next_due += std::chrono::microseconds(int64_t(1e6 / a.fps));
      const auto now = std::chrono::steady_clock::now();
      if (next_due < now) next_due = now;
      else std::this_thread::sleep_until(next_due);
    }
    return true;
  };

  // ---- workers (T > 1): any idle worker takes the oldest queued frame ----
  std::mutex mu;
  std::condition_variable cv_work, cv_done;
  std::deque<Job*> queue;
  bool quit = false;
  std::vector<std::thread> workers;
  for (int t = 0; T > 1 && t < T; ++t)
    workers.emplace_back([&] {
      RenderSet rs;
      for (;;) {
        Job* j = nullptr;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv_work.wait(lk, [&] { return quit || !queue.empty(); });
          if (quit) return;
          j = queue.front();
          queue.pop_front();
        }
        draw(*j, j->scene, rs);
        {
          std::lock_guard<std::mutex> lk(mu);
          j->done = true;
        }
        cv_done.notify_all();
      }
    });
  RenderSet main_set;
  main_set.hwc = std::move(renderer_hwc), main_set.rgb = std::move(renderer_rgb);

  const size_t depth = T > 1 ? size_t(T) + 1 : 1;
  std::vector<Job> jobs(depth);
  size_t head = 0, inflight = 0;
  bool ended = false;
  for (;;) {
    // (the hint is sticky and re-read every round: consumers come after the first frames)
    const bool piped = T > 1 && (!by_rule || (seg && (seg->hint() & shm::kWantSlotDelta) != 0));
    while (!ended && !g_stop && inflight < (piped ? depth : 1) && (a.frames < 0 || dispatched < a.frames)) {
      int slot = -1;
      if (seg) {
        // blocks while every slot is with a consumer -- but never while a
        // drawn frame waits for its retire: the consumer may need that frame
        // before it hands a slot back
        slot = seg->acquire(inflight ? 0 : -1, &g_stop, a.lease_ms);
        if (slot < 0) {
          ended = inflight == 0;
          break;
        }
      }
      Job& j = jobs[(head + inflight) % depth];
      front(j, slot);
      ++inflight;
      if (piped) {
        {
          std::lock_guard<std::mutex> lk(mu);
          queue.push_back(&j);
        }
        cv_work.notify_one();
      } else {
        draw(j, scene, main_set);
        j.done = true;
      }
    }
    if (inflight == 0) break;
    Job& j = jobs[head];
    if (T > 1) {
      std::unique_lock<std::mutex> lk(mu);
      cv_done.wait(lk, [&] { return j.done; });
    }
    head = (head + 1) % depth, --inflight;
    if (!retire(j)) break;
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    quit = true;
  }
  cv_work.notify_all();
  for (auto& t : workers) t.join();   // no render is left writing into the ring when it is unmapped
  double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  if (a.verbose)
    std::fprintf(stderr, "cubesim[%d]: %lld frames in %.2fs (%.1f fps, render %.3f ms/frame)\n", a.btid,
                 published, secs, published / std::max(secs, 1e-9), render_ms / std::max<long long>(published, 1));
  sock->close(g_stop ? 0 : -2);
  return 0;
}
