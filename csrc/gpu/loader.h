// StreamLoader: producer frames -> decoded batch in HBM.
//
// Replaces the reference's receive path (pkg_pytorch/blendtorch/btt/
// dataset.py:64-117 PULL socket per DataLoader worker + pickle.loads +
// default_collate + worker->main shared-memory copy) with one native
// pipeline per GPU rank:
//
//   producers --PUSH/ZMTP--> K PULL sockets (K IO threads, fair-queued)
//     -> the image is either in the producer's shared-memory ring (the
//        message carries a `_btshm` descriptor; the ring is hipHostRegister'ed
//        and mapped once) or inline, read by the IO thread straight into
//        hipHostMalloc'd slots (PinnedPool is the socket allocator)
//     -> worker thread: zero-copy pickle scan locates the image payload,
//        copies only the small non-image bytes (metadata) out
//     -> B items + the next consumer-posted output buffer form a batch;
//        direct path (default, every frame device-visible and 16-byte
//        aligned): the fused decode kernel reads the host frames over PCIe
//        itself, and batches that wait while `launch_depth` launches are
//        queued go out together in one launch; copy path: hipMemcpyAsync of
//        every image into a device staging ring first, then the kernel
//     -> the kernel (flip/gamma/unpack/normalize/CHW|NHWC) writes the
//        consumer's tensor on a private non-blocking HIP stream; an event
//        after the last host read lets the worker hand slots back (no host
//        callback in the stream); the same event (direct path, host-ordered)
//        or a per-batch event marks the batch ready
//     -> consumer (Python) takes batch j; its torch stream waits on the event.
//
// Backpressure is preserved end to end: when the consumer stops posting
// output buffers the worker stops receiving, each pipe fills to RCVHWM, the
// TCP window closes and the producers block at SNDHWM -- exactly the
// behaviour the reference's PUSH/PULL + HWM gives (btb/publisher.py:21-28).
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "../codec/pickle_codec.h"
#include "../common/buffer.h"
#include "../common/crop_draw.h"
#include "../transport/shmring.h"
#include "../transport/zmtp.h"
#include "kernels.h"
#include "launch_policy.h"
#include "slot_mirror.h"

namespace btn {
namespace gpu {

// Fixed-size pinned host slots handed to the transport as its frame
// allocator.  A slot returns to the pool when the last reference to its
// Buffer drops (after the H2D copy that reads it has completed).
class PinnedPool : public Allocator, public std::enable_shared_from_this<PinnedPool> {
 public:
  PinnedPool(size_t slot_bytes, int nslots);
  ~PinnedPool() override;
  // Blocks up to `wait_ms` for a free slot (backpressure on the IO thread),
  // then returns nullptr (heap fallback) if the pool is still dry.
  BufPtr alloc(size_t n) override;
  // A free slot now or nullptr: no wait, not counted as a fallback (the
  // worker stages a heap-received frame into it, StreamLoader::launch)
  BufPtr try_alloc(size_t n);
  void set_wait_ms(int ms) { wait_ms_ = ms; }
  size_t slot_bytes() const { return slot_bytes_; }
  int nslots() const { return nslots_; }
  int free_slots();
  uint64_t fallbacks() const { return fallbacks_.load(); }
  // Device-visible address of a host byte inside the pool (kernels may read
  // the slots directly over PCIe), or nullptr if `host` is not in the pool.
  const uint8_t* device_ptr(const uint8_t* host) const {
    if (!dev_base_ || host < base_ || host >= base_ + slot_bytes_ * size_t(nslots_)) return nullptr;
    return dev_base_ + (host - base_);
  }

 private:
  static void release(void* owner, Buffer* b);
  size_t slot_bytes_;
  int nslots_;
  uint8_t* base_ = nullptr;
  uint8_t* dev_base_ = nullptr;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<int> free_;
  std::atomic<uint64_t> fallbacks_{0};
  int wait_ms_ = 50;
};

struct LoaderConfig {
  std::vector<std::string> addresses;
  int batch_size = 8;
  std::string image_key = "image";
  int rcvhwm = 10;
  int io_threads = 1;
  int device = 0;
  int64_t max_batches = -1;          // -1: stream forever
  size_t max_frame_bytes = 0;        // 0: infer from first frame (x1.05 + 4 KiB)
  int pool_slots = 0;                // 0: auto
  int staging_depth = 3;
  bool skip_bad = false;             // drop malformed messages instead of failing
  // true: when every frame of a batch sits in device-visible pinned host
  // memory (pool slot or registered shm ring) with 16-byte alignment, the
  // decode kernel reads the frames itself over PCIe (zero-copy fused read,
  // ~45 GB/s vs ~35 GB/s for per-frame DMA copies + decode on MI355X);
  // false: always DMA into the device staging ring first.
  bool direct = true;
  // Copy path: a batch's frames are spread over this many HIP streams so
  // several DMA engines pull from host memory concurrently (1: all on the
  // loader stream).  Bounded by the runtime's hardware queues.
  int copy_streams = 2;
  // Direct-path launches queued on the loader stream before new batches wait
  // and coalesce into one launch (0: always hold until 64 images or stream
  // end).  Out of posted buffers the waiting batches still hold while
  // max(1, launch_depth) launches are queued (launch_policy.h).
  int launch_depth = 2;
  // Direct-path plain-decode launch groups rotate over this many non-blocking
  // HIP streams (1..4; 1: everything on the loader stream).  With 2, launch
  // N+1 sits on another hardware queue than launch N and no completion marker
  // of N stands in front of its kernel.  Back-to-back decodes without
  // producers gain 3-6 % that way, but in the streaming pipeline the two
  // launches that `launch_depth` = 2 allows then run side by side, share the
  // link, end together and leave it idle until the host has queued the next
  // pair: 8 % slower than one stream (profiles/r8/decode_overlap.md), hence
  // the default.  `launch_depth` counts the launches in flight over all
  // streams.  Copy-path, pass-through, tile16 and colour-kernel launches
  // always use the loader stream.
  int decode_streams = 1;
  // Order the loader's work against the consumer on the HOST: a posted
  // buffer is written only once the host has seen its post event complete,
  // and a batch is handed out only once the host has seen all its device
  // work (copies / kernel) complete -- no cross-stream hipStreamWaitEvent in
  // either direction.  Each such wait costs 28-430 us of host time on ROCm
  // 7 (profiles/r2/hip_api_cost.json), and issuing them per batch from the
  // loader thread held up the consumer's graph launches (~0.2 ms per step of
  // the disc consumer).  false: the GPU-side waits of round 1.
  bool host_sync = true;
  // Ring hint (shmring.h): true = a loader that reads RGB only, in place
  // (direct path, no alpha in the channel map, no colour kernel) asks its
  // producers for rgb_a frames and leaves the alpha plane in host memory;
  // false = always ask for interleaved frames.
  bool planar_alpha = true;
  // Slot mirror (slot_mirror.h, kernels.h: decode_delta): keep a byte copy of
  // every ring slot in HBM and read only the region its producer reports as
  // rewritten (ring hint kWantSlotDelta) over the link; the rest of the frame
  // comes from the copy.  Only for direct-path plain decodes on one decode
  // stream (not the copy path, pass-through, tile16, the colour kernel, crop
  // or decode_streams > 1), and only for frames the vector kernel takes.  A
  // slot's first read, and any read whose report does not refer to the
  // generation the copy holds, is a whole-frame read as without the mirror.
  // One buffer of nslots x H x W x (3 for rgb_a slots read in place, else C)
  // bytes per ring, made when its producer first reports and freed with the loader; a ring that
  // would take the total past slot_mirror_max_bytes gets none, nor do frames
  // below slot_mirror_min_frame_bytes (0: no lower bound).
  bool slot_mirror = true;
  size_t slot_mirror_max_bytes = size_t(1) << 30;
  size_t slot_mirror_min_frame_bytes = 0;
  // decode parameters (src/dst/B/H/W/Cin filled per batch)
  int cout = 3;
  int cmap[4] = {0, 1, 2, 3};
  int flip_all = 0;
  int out_dtype = OUT_F32;
  int layout = NCHW;
  std::vector<float> lut;            // 4*256 floats (host)
  bool color_matrix = false;         // use the MFMA colour-transform kernel
  std::vector<float> matrix, bias;   // 16 + 4 floats
  // per-image transforms on the same kernel (photometric augmentation):
  // matrices: batch_size x (16 + 4) floats, the transform of each batch position;
  // jitter: every image draws (brightness, contrast, saturation, hue) uniformly from
  // [1 - r, 1 + r] (hue: [-r, r] turns) with a seeded splitmix64 stream in arrival
  // order, and the batch reports the factors it was decoded with
  std::vector<float> matrices;
  bool jitter = false;
  float jitter_range[4] = {0.f, 0.f, 0.f, 0.f};
  float pivot = 0.5f;
  uint64_t jitter_seed = 0;
  // crop + mirror (kernels.h: decode_crop): every image is decoded through a
  // crop_h x crop_w window drawn in arrival order (common/crop_draw.h: random
  // origin and mirror bit from a seeded splitmix64 stream, or the centre, or
  // the fixed origin); the kernel reads only the window's bytes and the batch
  // reports the windows it was decoded with.  Not with the colour kernel and
  // not for tile16 frames.
  bool crop = false;
  int crop_h = 0, crop_w = 0;
  int crop_mode = 0;                 // crop::Mode
  int crop_y0 = 0, crop_x0 = 0;      // the fixed origin
  double mirror = 0.0;
  int x_align = 1;
  uint64_t crop_seed = 0;
  // resized crop (kernels.h: decode_resize): every image is decoded through a
  // window drawn where the crop window is drawn, in arrival order
  // (common/crop_draw.h: resized), and resized to resize_spec.oh x .ow; the
  // batch reports the windows.  As with a crop: at most 64 images per launch,
  // no slot mirror, no tile16 frames, no colour kernel, no pass-through; not
  // together with a crop.
  bool resize = false;
  resized::Spec resize_spec;
  uint64_t resize_seed = 0;
};

// One delivered batch: metadata of each item (non-image bytes of the frame,
// re-based) and the event that completes its device work.
struct BatchMeta {
  std::vector<uint8_t> bytes;        // frame with the image payload cut out
  codec::VPtr tree;                  // parse tree over `bytes` (image entry removed)
  // A shared-memory descriptor the worker only scanned (codec::scan_descriptor)
  // has no tree yet: it is built here, by whoever reads the metadata (the
  // consumer's thread), without the `_btshm` entry.  Throws what the worker
  // would have reported for a message parse() rejects.
  // A change of behaviour for such a message: the scan does not look into the
  // values it skips (an ndarray's dtype, say), so a descriptor message whose
  // other entries parse() rejects used to be counted `bad` on the worker and
  // dropped under skip_bad; now its frame is decoded and counted, and the
  // error surfaces here, from next(), where skip_bad cannot drop one image
  // out of a decoded batch.  cubesim and the Python publisher write no such
  // message.
  bool lazy = false;
  const codec::VPtr& get_tree() {
    if (lazy && !tree) {
      try {
        tree = codec::parse(bytes.data(), bytes.size());
      } catch (const std::exception& e) {
        throw std::runtime_error(std::string("StreamLoader: bad message: unparseable pickle (") + e.what() + ")");
      }
      if (tree && tree->kind == codec::Value::DICT)
        for (size_t i = 0; i + 1 < tree->items.size(); i += 2)
          if (tree->items[i]->kind == codec::Value::STR && tree->items[i]->s == "_btshm") {
            tree->items.erase(tree->items.begin() + long(i), tree->items.begin() + long(i) + 2);
            break;
          }
      lazy = false;
    }
    return tree;
  }
};

// Free list of events of one flag set.  A launch used to create, record and
// destroy its events; a recorded event that nobody waits for any more is
// simply recorded again.  take() and give() may come from any thread (the
// last owner of an EventSet can be the consumer's).
class EventPool {
 public:
  explicit EventPool(unsigned flags) : flags_(flags) {}
  EventPool(const EventPool&) = delete;
  EventPool& operator=(const EventPool&) = delete;
  ~EventPool() {
    for (auto e : free_) (void)hipEventDestroy(e);
  }
  hipError_t take(hipEvent_t* ev) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (!free_.empty()) {
        *ev = free_.back();
        free_.pop_back();
        return hipSuccess;
      }
    }
    created_++;
    return hipEventCreateWithFlags(ev, flags_);
  }
  void give(hipEvent_t ev) {
    std::lock_guard<std::mutex> lk(mu_);
    if (free_.size() < kKeep) free_.push_back(ev);
    else (void)hipEventDestroy(ev);
  }
  uint64_t created() const { return created_.load(); }
  static constexpr size_t kKeep = 32;   // more than are ever in flight (launch depth, posted buffers)

 private:
  const unsigned flags_;
  std::mutex mu_;
  std::vector<hipEvent_t> free_;
  std::atomic<uint64_t> created_{0};
};

// Events owned jointly by an in-flight launch (slot release) and the batches
// waiting for completion (host_sync); they go back to their pool (or are
// destroyed) with the last owner.
struct EventSet {
  std::vector<hipEvent_t> ev;
  std::shared_ptr<EventPool> pool;   // where the events go back to (null: destroyed)
  EventSet() = default;
  EventSet(const EventSet&) = delete;
  EventSet& operator=(const EventSet&) = delete;
  ~EventSet() {
    for (auto e : ev) {
      if (pool) pool->give(e);
      else (void)hipEventDestroy(e);
    }
  }
  // all complete? (errors count as complete: the stream reports them later)
  bool done() const {
    for (auto e : ev)
      if (hipEventQuery(e) == hipErrorNotReady) return false;
    return true;
  }
  void wait() const {
    for (auto e : ev) (void)hipEventSynchronize(e);
  }
};

struct ReadyBatch {
  int64_t index = -1;
  std::vector<BatchMeta> items;
  hipEvent_t done = nullptr;         // GPU-side completion (host_sync = false)
  std::shared_ptr<EventSet> pending; // host-side completion (host_sync): ready once done()
  double recv_ms = 0;                // wall time spent assembling the batch
  struct SlotRef {
    shm::Segment* seg;
    uint32_t slot, gen;
  };
  std::vector<SlotRef> slots;        // host_sync: shm slots re-validated before hand-out
  int64_t launch_no = 0;             // host_sync: the launch that read them
  std::vector<float> jitter;         // colour jitter: 4 factors per image (LoaderConfig::jitter)
  std::vector<int32_t> crop;         // crop: (y0, x0, mirrored) per image (LoaderConfig::crop)
  std::vector<int32_t> window;       // resize: (y0, x0, h, w, mirrored) per image (LoaderConfig::resize)
};

struct LoaderStats {
  uint64_t frames = 0, batches = 0, bytes = 0, bad = 0, pool_fallbacks = 0;
  uint64_t shm_frames = 0, shm_torn = 0;   // via shared memory / slot reclaimed during the copy
  uint64_t shm_stale = 0;                  // descriptors dropped: slot already reclaimed on arrival
  uint64_t direct_batches = 0;             // decoded straight from host memory (no staging copy)
  uint64_t launches = 0;                   // decode kernel launches (< batches when coalesced)
  uint64_t image_bytes = 0;                // image bytes that crossed host -> device
  uint64_t tiled_frames = 0;               // key-frame delta frames (tiledelta.h)
  uint64_t planar_frames = 0;              // shm frames that arrived as rgb_a (planar_alpha.h)
  uint64_t delta_frames = 0;               // frames of which only the reported region was read from the host
  uint64_t block_frames = 0;               // ... of which only the reported blocks were (subset of delta_frames)
  uint64_t mirror_bytes = 0;               // HBM held by slot mirrors
  double h2d_issue_ms = 0;
  // GPU time of one launch per kTimedEveryImages images (timing events around
  // its H2D copies + decode kernel): per-image device cost without timing
  // every launch
  uint64_t timed_launches = 0, timed_images = 0;
  double timed_gpu_ms = 0;
  uint64_t keys_evicted = 0;               // replaced tile16 key frames freed from HBM
  // producer rings at the time of stats(): slots, frames published and not
  // yet claimed (waiting in queues), frames claimed by this loader
  uint64_t ring_slots = 0, ring_published = 0, ring_held = 0;
  uint64_t passthrough_batches = 0;        // copy path, identity decode: DMA only, no kernel
  uint64_t staged_frames = 0;              // heap-received frames copied into a pinned slot (batch kept direct)
  std::map<int64_t, uint64_t> frames_per_btid;   // provenance: frames per producer id
  // worker-thread CPU (thread clock, ms) per stage of its loop -- where the
  // consumer process's CPU per delivered frame goes: socket poll, receive +
  // descriptor parse + batch assembly, decode launches (a subset of the
  // previous), completion checks (reap + promote)
  double cpu_poll_ms = 0, cpu_recv_ms = 0, cpu_launch_ms = 0, cpu_reap_ms = 0;
  int64_t worker_tid = 0;
};

class StreamLoader {
 public:
  explicit StreamLoader(const LoaderConfig& cfg);
  ~StreamLoader();

  void start();
  // Blocks until the first frame fixed H, W, Cin (or timeout -> false).
  bool wait_shape(long timeout_ms, int* H, int* W, int* C);
  // Queue an output buffer for the next batch.  An event recorded on
  // `consumer` now is waited on by the loader stream before it writes, so
  // the caching allocator's reuse of `dst` is safe.
  void post(void* dst, hipStream_t consumer);
  // Next completed batch (in order).  Makes `consumer` wait on its event.
  // Returns false on timeout; throws std::runtime_error on a loader error
  // or when the stream is exhausted (max_batches reached -> index == -1).
  bool next(ReadyBatch* out, hipStream_t consumer, long timeout_ms);
  void stop();
  LoaderStats stats();

 private:
  struct KeyFrame;
  struct MappedSegment;
  struct Item {
    zmtp::Frame frame;
    const uint8_t* src = nullptr;      // image bytes: in the frame or in a shm slot
    const uint8_t* dsrc = nullptr;     // device-visible alias of `src` (pinned + mapped), or null
    shm::Segment* seg = nullptr;       // shared-memory slot to hand back, if any
    uint32_t slot = 0, gen = 0;
    MappedSegment* ms = nullptr;       // the ring `seg` belongs to (slot mirror)
    bool has_delta = false;            // descriptor element 10 (shmring.h: kWantSlotDelta)
    mirror::Delta delta;
    bool has_blocks = false;           // ... and a valid element 11 (shmring.h: kWantSlotBlocks)
    mirror::BlockMask blocks;
    bool flip = false;
    // key-frame delta (csrc/codec/tiledelta.h): `src`/`dsrc` point at the
    // encoded frame (ntiles payload tiles); the key frame is at key_host (shm)
    bool tiled = false;
    int ntiles = 0;
    KeyFrame* key = nullptr;
    const uint8_t* key_host = nullptr;
    // rgb_a slot (csrc/common/planar_alpha.h): `src`/`dsrc` point at H*W*3
    // bytes of packed RGB, the alpha plane follows; read in place with Cin = 3
    bool planar = false;
    std::vector<uint8_t> expanded;     // copy path: the frame rebuilt on the host
    BufPtr staged;                     // pinned slot a heap-received image was copied into (direct path)
    float jit[4] = {1.f, 1.f, 1.f, 0.f};   // colour-jitter factors (LoaderConfig::jitter)
    crop::Window win;                      // crop window (LoaderConfig::crop)
    resized::Window rwin;                  // resize window (LoaderConfig::resize)
    BatchMeta meta;
  };
  // rebuild on the host what the batch cannot read in place: a key-frame
  // delta, and (unless keep_planar) an rgb_a frame back to interleaved RGBA
  void materialize(Item& it, bool keep_planar = false);
  bool reads_rgb_only() const;        // this loader's decode never needs a frame's alpha or interleaving
  struct Posted {
    void* dst;
    hipEvent_t ready;
  };
  void run();
  bool process(zmtp::Message&& msg);
  struct Pending {                    // assembled batch waiting for launch
    std::vector<Item> items;
    void* dst = nullptr;
    hipEvent_t ready = nullptr;
    double t0 = 0;
    bool direct = false;
    bool tiled = false;               // every image a key-frame delta: fill + tile scatter
  };
  void launch();
  void flush_pending(bool ending, bool out_of_buffers = false);   // asks launch_policy.h
  void launch_group(std::vector<Pending>& group);
  hipStream_t next_decode_stream();
  void reap(bool wait_all = false);   // release pinned slots of completed H2D copies
  void evict_keys();
  void drain_sockets();               // stop(): hand back ring slots of still-queued descriptors
  void release_descriptor(const zmtp::Message& m);   // an unprocessed descriptor: slot back to its producer

  LoaderConfig cfg_;
  std::vector<std::unique_ptr<zmtp::Context>> ctxs_;
  std::vector<std::shared_ptr<zmtp::Socket>> socks_;
  std::shared_ptr<PinnedPool> pool_;
  std::thread worker_;
  std::atomic<bool> stop_{false};
  // LoaderStats::cpu_*_ms, in ns (written by the worker, read by stats())
  enum CpuStage { kCpuPoll, kCpuRecv, kCpuLaunch, kCpuReap, kCpuStages };
  std::atomic<uint64_t> cpu_ns_[kCpuStages] = {};
  std::atomic<int64_t> worker_tid_{0};

  std::mutex mu_;
  std::condition_variable cv_;
  bool have_shape_ = false;
  int H_ = 0, W_ = 0, C_ = 0;
  size_t img_bytes_ = 0;
  std::deque<Posted> posted_;
  std::deque<ReadyBatch> ready_;
  std::string error_;
  bool exhausted_ = false;

  // worker-thread state
  hipStream_t stream_ = nullptr;
  std::vector<uint8_t*> staging_;
  float* d_lut_ = nullptr;
  float* d_mat_ = nullptr;   // 16 matrix + 4 bias (or batch_size x 20: LoaderConfig::matrices)
  uint64_t jit_state_ = 0;   // splitmix64 state of the colour-jitter draws
  uint64_t crop_state_ = 0;  // splitmix64 state of the crop-window draws
  uint64_t resize_state_ = 0;  // splitmix64 state of the resize-window draws
  crop::Spec crop_spec() const;
  std::vector<Item> cur_;
  std::deque<Pending> pending_;
  int pending_images_ = 0;
  static constexpr int kMaxDecodeStreams = 4;
  // a launch is timed once this many images went out since the last timed one
  // (sampling by images: with one batch per launch a per-launch rule fires
  // several times as often as with coalesced launches)
  static constexpr int kTimedEveryImages = 96;
  static constexpr int kTimedSkip = 8;         // cold launches never sampled
  int64_t untimed_images_ = 0;
  // reused events: completion markers, the consumer's post events, timing pairs
  std::shared_ptr<EventPool> done_events_, post_events_, time_events_;
  // Waiting on the critical path (a posted buffer's event, the oldest launch,
  // a buffer to launch into) first polls for a bounded time and only then
  // sleeps: a sleep of 10-20 us returns after ~60 us under the default timer
  // slack, most of a decode kernel's run time.  BT_LOADER_SPIN_US (default
  // 150, 0: sleep at once) bounds each such wait's polling.  Loaders
  // configured for the copy path (direct = false) do not poll.
  static constexpr int64_t kKeyIdleLaunches = 64;
  int64_t launch_no_ = 0, retired_launch_ = 0;
  double last_reap_ms_ = 0;
  std::vector<hipStream_t> copy_streams_;      // copy path fan-out (cfg_.copy_streams > 1)
  std::vector<hipEvent_t> copy_done_;          // one per copy stream, reused
  // direct-path plain decodes rotate over these (cfg_.decode_streams); [0] is
  // stream_, the others are owned here and made on first use.  Each launch keeps all its stream-side
  // work (post-event waits, timing and completion events, kernels) on one of them
  std::vector<hipStream_t> decode_streams_;
  size_t decode_rr_ = 0;
  std::vector<hipEvent_t> stage_free_;         // per staging buffer: last kernel reading it
  std::vector<shm::Segment*> seg_list_;        // mapped rings, for stats() (guarded by mu_)
  // the configured decode is the identity on the frame bytes (u8, NHWC, all
  // channels in order, identity table, no flip): copy-path batches are then
  // DMA'd straight into the consumer's tensor and no kernel runs at all
  bool passthrough_ = false;
  void promote_ready();                 // host_sync: completed batches -> ready_
  void host_wait(hipEvent_t ev);        // host_sync: poll an event, promoting meanwhile
  std::deque<ReadyBatch> unready_;      // host_sync: launched, device work not yet seen complete
  struct Inflight {
    int64_t launch_no = 0;
    std::shared_ptr<EventSet> copied;
    hipEvent_t t0 = nullptr, t1 = nullptr;   // sampled launch timing (or null)
    int images = 0;
    std::vector<zmtp::Frame> frames;
    struct Slot {
      shm::Segment* seg;
      uint32_t slot, gen;
    };
    std::vector<Slot> slots;
    std::vector<std::vector<uint8_t>> expanded;   // pageable copy sources, alive until `copied`
    std::vector<BufPtr> staged;                   // pinned slots of staged heap frames, alive until `copied`
  };
  struct MappedSegment {
    std::unique_ptr<shm::Segment> seg;
    uint8_t* dev_base = nullptr;   // device-visible alias of seg->base()
    // slot mirror: nslots x H x W x mirror_cin bytes in HBM (null: none) and
    // the generation it holds per slot
    uint8_t* mirror_dev = nullptr;
    int mirror_cin = 0;
    bool mirror_failed = false;    // no buffer for this ring (budget, frame size, allocation): not tried again
    mirror::Ring ring;
  };
  bool mirror_wanted() const;                           // this loader's configuration can use slot mirrors
  bool slot_blocks_ = true;                             // block masks (decode_delta_blocks) unless BT_SLOT_BLOCKS=0
  uint8_t* slot_mirror(MappedSegment& ms, int cin, bool reported);   // the ring's mirror for such frames, or null
  void invalidate_mirror(shm::Segment* seg, uint32_t slot);
  std::map<const shm::Segment*, MappedSegment*> by_seg_;
  mirror::Budget mirror_budget_;
  MappedSegment& segment(std::string_view name);
  std::map<std::string, MappedSegment, std::less<>> segments_;   // mapped + hipHostRegister'ed
  struct KeyFrame {
    std::unique_ptr<shm::Segment> seg;
    uint8_t* dev = nullptr;          // HBM copy, made on first use
    void* decoded[2] = {nullptr, nullptr};   // decoded for this loader (upper-left, flipped)
    int refs = 0;                    // items holding it that have not launched yet
    int64_t last_launch = 0;         // last launch that read it
  };
  KeyFrame& key_frame(const std::string& name, size_t bytes);
  const void* decoded_key(KeyFrame& kf, bool flip, size_t out_img_bytes);
  std::map<std::string, KeyFrame> keys_;
  std::deque<Inflight> inflight_;   // H2D copies not yet known complete
  int64_t batch_index_ = 0;
  double batch_t0_ = 0;
  double last_progress_ms_ = 0;     // run(): last frame received or batch handed over
  bool first_taken_ = false;        // next() has handed out a batch (guarded by mu_)
  LoaderStats stats_;
  // per-frame counters of process(), folded into stats_ once per launch
  // (lock order: mu_, then tally_mu_)
  struct Tally {
    uint64_t frames = 0, bytes = 0, image_bytes = 0, tiled_frames = 0, planar_frames = 0, shm_frames = 0;
    std::vector<std::pair<int64_t, uint64_t>> btid;
    void add_to(LoaderStats& s) const {
      s.frames += frames, s.bytes += bytes, s.image_bytes += image_bytes;
      s.tiled_frames += tiled_frames, s.planar_frames += planar_frames, s.shm_frames += shm_frames;
      for (const auto& kv : btid) s.frames_per_btid[kv.first] += kv.second;
    }
    void clear() {
      frames = bytes = image_bytes = tiled_frames = planar_frames = shm_frames = 0;
      btid.clear();
    }
  };
  Tally tally_;
  std::mutex tally_mu_;
};

}  // namespace gpu
}  // namespace btn
