// StreamLoader implementation (see loader.h).
#include "loader.h"

#include <pthread.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include "../codec/tiledelta.h"
#include "../common/planar_alpha.h"
#include "../common/trace.h"

#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <stdexcept>

namespace btn {
namespace gpu {

namespace {

void check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Remove the image entry from the dict and shift every payload offset that
// lies behind the cut so the tree indexes the compacted metadata bytes.
void shift_offsets(codec::Value& v, size_t cut, size_t len) {
  if ((v.kind == codec::Value::BYTES || v.kind == codec::Value::NDARRAY || v.np_scalar) && !v.owned) {
    if (v.off >= cut + len) v.off -= len;
  }
  for (auto& c : v.items)
    if (c) shift_offsets(*c, cut, len);
}

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace

// ---------------------------------------------------------------------------
// PinnedPool
// ---------------------------------------------------------------------------
PinnedPool::PinnedPool(size_t slot_bytes, int nslots) : slot_bytes_(slot_bytes), nslots_(nslots) {
  check(hipHostMalloc(reinterpret_cast<void**>(&base_), slot_bytes_ * size_t(nslots_), hipHostMallocDefault),
        "hipHostMalloc(pinned pool)");
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&dev_base_), base_, 0) != hipSuccess) dev_base_ = nullptr;
  free_.reserve(size_t(nslots_));
  for (int i = nslots_ - 1; i >= 0; --i) free_.push_back(i);
}

PinnedPool::~PinnedPool() {
  if (base_) (void)hipHostFree(base_);
}

int PinnedPool::free_slots() {
  std::lock_guard<std::mutex> lk(mu_);
  return int(free_.size());
}

BufPtr PinnedPool::alloc(size_t n) {
  if (n > slot_bytes_) {
    fallbacks_++;
    return nullptr;
  }
  int id;
  {
    std::unique_lock<std::mutex> lk(mu_);
    if (free_.empty() && wait_ms_ > 0)
      cv_.wait_for(lk, std::chrono::milliseconds(wait_ms_), [&] { return !free_.empty(); });
    if (free_.empty()) {
      fallbacks_++;
      return nullptr;
    }
    id = free_.back();
    free_.pop_back();
  }
  auto b = std::make_shared<Buffer>();
  b->data = base_ + size_t(id) * slot_bytes_;
  b->capacity = slot_bytes_;
  b->owner = this;
  b->tag = id;
  b->pinned = true;
  b->release = &PinnedPool::release;
  return b;
}

BufPtr PinnedPool::try_alloc(size_t n) {
  if (n > slot_bytes_) return nullptr;
  int id;
  {
    std::lock_guard<std::mutex> lk(mu_);
    if (free_.empty()) return nullptr;
    id = free_.back();
    free_.pop_back();
  }
  auto b = std::make_shared<Buffer>();
  b->data = base_ + size_t(id) * slot_bytes_;
  b->capacity = slot_bytes_;
  b->owner = this;
  b->tag = id;
  b->pinned = true;
  b->release = &PinnedPool::release;
  return b;
}

void PinnedPool::release(void* owner, Buffer* b) {
  auto* self = static_cast<PinnedPool*>(owner);
  {
    std::lock_guard<std::mutex> lk(self->mu_);
    self->free_.push_back(int(b->tag));
  }
  self->cv_.notify_one();
}

// ---------------------------------------------------------------------------
// StreamLoader
// ---------------------------------------------------------------------------
StreamLoader::StreamLoader(const LoaderConfig& cfg) : cfg_(cfg) {
  // BT_SLOT_BLOCKS=0 keeps the rectangle path (decode_delta) for A/B runs: no
  // block hint to the producers, no block-mask launches
  if (const char* e = std::getenv("BT_SLOT_BLOCKS")) slot_blocks_ = std::strcmp(e, "0") != 0;
  if (cfg_.addresses.empty()) throw std::invalid_argument("StreamLoader: no addresses");
  if (cfg_.batch_size < 1) throw std::invalid_argument("StreamLoader: batch_size < 1");
  // the value table (kernels.h): a bare [4][256] fp32 table is padded with a
  // zero header (mode 0: table lookups)
  if (cfg_.lut.size() == 4 * 256) cfg_.lut.resize(kTableFloats, 0.f);
  if (cfg_.lut.size() != size_t(kTableFloats))
    throw std::invalid_argument("StreamLoader: lut must hold 4*256 or kTableFloats floats");
  if (cfg_.cout < 1 || cfg_.cout > 4) throw std::invalid_argument("StreamLoader: cout must be 1..4");
  if (cfg_.decode_streams < 1 || cfg_.decode_streams > kMaxDecodeStreams)
    throw std::invalid_argument("StreamLoader: decode_streams must be 1..4");
  if (cfg_.color_matrix && !cfg_.jitter && cfg_.matrices.empty() && (cfg_.matrix.size() != 16 || cfg_.bias.size() != 4))
    throw std::invalid_argument("StreamLoader: colour matrix needs 16 + 4 floats");
  if (!cfg_.matrices.empty() && cfg_.matrices.size() != size_t(cfg_.batch_size) * 20)
    throw std::invalid_argument("StreamLoader: per-position colour matrices need batch_size x (16 + 4) floats");
  if ((cfg_.jitter || !cfg_.matrices.empty()) && cfg_.batch_size > kMaxSrcs)
    throw std::invalid_argument("StreamLoader: per-image colour transforms need batch_size <= 64");
  jit_state_ = cfg_.jitter_seed * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
  if (cfg_.crop) {
    if (cfg_.color_matrix) throw std::invalid_argument("StreamLoader: a crop does not combine with the colour kernel");
    if (cfg_.batch_size > kMaxSrcs) throw std::invalid_argument("StreamLoader: a crop needs batch_size <= 64");
    if (cfg_.crop_h < 1 || cfg_.crop_w < 1 || cfg_.crop_h > INT16_MAX || cfg_.crop_w > INT16_MAX ||
        cfg_.crop_mode < crop::kRandom || cfg_.crop_mode > crop::kFixed || cfg_.crop_y0 < 0 || cfg_.crop_x0 < 0 ||
        !(cfg_.mirror >= 0.0 && cfg_.mirror <= 1.0) || (cfg_.x_align != 1 && cfg_.x_align != 4 && cfg_.x_align != 16))
      throw std::invalid_argument("StreamLoader: bad crop (size >= 1, mirror in [0, 1], x_align 1, 4 or 16)");
  }
  crop_state_ = crop::seed_state(cfg_.crop_seed);
  if (cfg_.resize) {
    if (cfg_.crop) throw std::invalid_argument("StreamLoader: a resize does not combine with a crop");
    if (cfg_.color_matrix) throw std::invalid_argument("StreamLoader: a resize does not combine with the colour kernel");
    if (cfg_.batch_size > kMaxSrcs) throw std::invalid_argument("StreamLoader: a resize needs batch_size <= 64");
    if (!resized::valid(cfg_.resize_spec))
      throw std::invalid_argument(
          "StreamLoader: bad resize (size 1..32767, 0 < smin <= smax <= 1, rmin <= 1 <= rmax, mirror in [0, 1])");
  }
  resize_state_ = resized::seed_state(cfg_.resize_seed);
  mirror_budget_ = mirror::Budget(cfg_.slot_mirror_max_bytes);
  int k = std::max(1, std::min<int>(cfg_.io_threads, int(cfg_.addresses.size())));
  for (int i = 0; i < k; ++i) {
    ctxs_.emplace_back(new zmtp::Context());
    auto s = ctxs_.back()->socket(zmtp::PULL);
    s->setsockopt(zmtp::RCVHWM, cfg_.rcvhwm);
    s->setsockopt(zmtp::LINGER, 0);
    socks_.push_back(s);
  }
  for (size_t i = 0; i < cfg_.addresses.size(); ++i) socks_[i % socks_.size()]->connect(cfg_.addresses[i]);
}

namespace {
uint64_t thread_cpu_ns() {
  timespec ts;
  clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
  return uint64_t(ts.tv_sec) * 1000000000ull + uint64_t(ts.tv_nsec);
}
// Host-ordered hand-off (host_sync): with BT_LOADER_BLOCKING=1 the events
// that mark a batch's device work are blocking-sync events, and a worker that
// cannot go on until the oldest launched batch completes (every posted
// buffer in use) sleeps in hipEventSynchronize instead of polling it every
// few microseconds.
bool blocking_waits() {
  static const bool on = [] {
    const char* e = std::getenv("BT_LOADER_BLOCKING");
    return e && e[0] == '1';
  }();
  return on;
}
unsigned completion_event_flags() {
  return hipEventDisableTiming | (blocking_waits() ? hipEventBlockingSync : 0u);
}
// BT_LOADER_CPU=1: the worker accounts its thread CPU per loop stage (the
// thread clock is a system call, ~0.3 us, a few per loop turn: off by default)
bool cpu_accounting() {
  static const bool on = [] {
    const char* e = std::getenv("BT_LOADER_CPU");
    return e && e[0] == '1';
  }();
  return on;
}
// adds the calling thread's CPU time over its scope to one counter
struct CpuScope {
  std::atomic<uint64_t>& acc;
  const bool on = cpu_accounting();
  const uint64_t t0 = on ? thread_cpu_ns() : 0;
  explicit CpuScope(std::atomic<uint64_t>& a) : acc(a) {}
  ~CpuScope() {
    if (on) acc.fetch_add(thread_cpu_ns() - t0, std::memory_order_relaxed);
  }
};
// Completion polling grain of the worker thread while launched batches are in
// flight (BT_LOADER_POLL_US, default 10): finer hands batches over sooner,
// coarser costs less CPU per delivered frame.
std::chrono::microseconds poll_grain() {
  static const long us = [] {
    const char* e = std::getenv("BT_LOADER_POLL_US");
    const long v = e ? std::atol(e) : 10;
    return v > 0 ? v : 10;
  }();
  return std::chrono::microseconds(us);
}
// How long a wait on the critical path polls before it sleeps (loader.h).
// Only a loader configured for the direct path polls: there a launch is a
// ~76 us kernel and a 60 us sleep is most of it.  A copy-path loader
// (direct = false) is bound by its DMA copies, ~270 us per batch; polling
// bought it no throughput and cost 15 CPU-us per frame, so it sleeps at
// once as before (profiles/r11/feed.md).
double spin_ms(const LoaderConfig& cfg) {
  static const double ms = [] {
    const char* e = std::getenv("BT_LOADER_SPIN_US");
    const long v = e ? std::atol(e) : 150;
    return double(std::max(0L, std::min(v, 10000L))) * 1e-3;
  }();
  return cfg.direct ? ms : 0.0;
}
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}
}  // namespace

StreamLoader::~StreamLoader() { stop(); }

void StreamLoader::start() {
  if (worker_.joinable()) return;
  done_events_ = std::make_shared<EventPool>(completion_event_flags());
  post_events_ = std::make_shared<EventPool>(unsigned(hipEventDisableTiming));
  time_events_ = std::make_shared<EventPool>(unsigned(hipEventDefault));
  worker_ = std::thread([this] {
    pthread_setname_np(pthread_self(), "bt-loader");
    worker_tid_ = int64_t(syscall(SYS_gettid));
    try {
      run();
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> lk(mu_);
      error_ = e.what();
    }
    cv_.notify_all();
  });
}

bool StreamLoader::wait_shape(long timeout_ms, int* H, int* W, int* C) {
  std::unique_lock<std::mutex> lk(mu_);
  cv_.wait_for(lk, std::chrono::milliseconds(timeout_ms), [&] { return have_shape_ || !error_.empty(); });
  if (!error_.empty()) throw std::runtime_error(error_);
  if (!have_shape_) return false;
  *H = H_;
  *W = W_;
  *C = C_;
  return true;
}

void StreamLoader::post(void* dst, hipStream_t consumer) {
  DeviceGuard g(cfg_.device);
  hipEvent_t ev;
  check(post_events_ ? post_events_->take(&ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
  check(hipEventRecord(ev, consumer), "hipEventRecord(post)");
  {
    std::lock_guard<std::mutex> lk(mu_);
    posted_.push_back({dst, ev});
  }
  cv_.notify_all();
}

bool StreamLoader::next(ReadyBatch* out, hipStream_t consumer, long timeout_ms) {
  trace::Range tr("btn.loader.next");
  std::unique_lock<std::mutex> lk(mu_);
  cv_.wait_for(lk, std::chrono::milliseconds(timeout_ms),
               [&] { return !ready_.empty() || !error_.empty() || exhausted_; });
  if (ready_.empty()) {
    if (!error_.empty()) throw std::runtime_error(error_);
    if (exhausted_) {
      out->index = -1;
      return true;
    }
    return false;
  }
  *out = std::move(ready_.front());
  ready_.pop_front();
  first_taken_ = true;
  lk.unlock();
  if (out->done) {   // host_sync = false: the consumer stream waits on the device
    DeviceGuard g(cfg_.device);
    check(hipStreamWaitEvent(consumer, out->done, 0), "hipStreamWaitEvent");
    (void)hipEventDestroy(out->done);
    out->done = nullptr;
  }
  out->pending.reset();
  return true;
}

// host_sync: hand out, in order, the launched batches whose device work the
// host has seen complete (worker thread).  Their shm slots are re-validated
// first: a HELD slot a dead-consumer lease took back while the DMA read it
// fails the stream BEFORE the batch reaches the consumer (reap() counts it).
// Without host_sync the batch is handed out at launch and the same check in
// reap() raises on the consumer's next next() call.
void StreamLoader::promote_ready() {
  bool any = false;
  while (!unready_.empty() && unready_.front().pending->done()) {
    ReadyBatch& rb = unready_.front();
    // a launch reap() has retired was validated there (before its slots were
    // handed back: they may already belong to new frames); otherwise the
    // slots are still held by this loader and are checked here
    bool torn = false;
    if (rb.launch_no > retired_launch_)
      for (const ReadyBatch::SlotRef& s : rb.slots)
        if (!s.seg->valid(s.slot, s.gen)) {
          torn = true;
          invalidate_mirror(s.seg, s.slot);   // its mirror copy may hold the next frame's bytes
        }
    std::lock_guard<std::mutex> lk(mu_);
    if ((torn || !error_.empty()) && !cfg_.skip_bad) {   // reap() may have failed the stream already
      if (error_.empty())
        error_ = "StreamLoader: shared-memory slot(s) were reclaimed by their producer while a batch read them";
      stop_ = true;
      any = true;
      break;
    }
    rb.slots.clear();
    ready_.push_back(std::move(rb));
    unready_.pop_front();
    any = true;
  }
  if (any) last_progress_ms_ = now_ms();
  if (any) cv_.notify_all();
}

void StreamLoader::host_wait(hipEvent_t ev) {
  if (hipEventQuery(ev) != hipErrorNotReady) return;
  const double spin_end = now_ms() + spin_ms(cfg_);
  while (!stop_) {
    promote_ready();
    if (hipEventQuery(ev) != hipErrorNotReady) return;
    if (now_ms() < spin_end) cpu_relax();
    else std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

void StreamLoader::stop() {
  stop_ = true;
  cv_.notify_all();
  if (worker_.joinable()) worker_.join();
  drain_sockets();
  for (auto& s : socks_) s->close(0);
  socks_.clear();
  ctxs_.clear();   // joins IO threads; queued frames are released
  DeviceGuard g(cfg_.device);
  for (auto cs : copy_streams_) {
    (void)hipStreamSynchronize(cs);
    (void)hipStreamDestroy(cs);
  }
  copy_streams_.clear();
  for (auto ev : copy_done_) (void)hipEventDestroy(ev);
  copy_done_.clear();
  // launches may be in flight on every decode stream: all of them drain (and
  // the extra ones go) before reap(true) hands their slots back
  for (size_t k = 1; k < decode_streams_.size(); ++k) {
    (void)hipStreamSynchronize(decode_streams_[k]);
    (void)hipStreamDestroy(decode_streams_[k]);
  }
  decode_streams_.clear();
  if (stream_) {
    (void)hipStreamSynchronize(stream_);
    reap(true);                            // drop pinned refs of finished copies
    (void)hipStreamDestroy(stream_);
    stream_ = nullptr;
  }
  for (auto ev : stage_free_)
    if (ev) (void)hipEventDestroy(ev);
  stage_free_.clear();
  for (auto& it : cur_)
    if (it.seg) it.seg->release(it.slot, it.gen);
  cur_.clear();
  for (auto& b : pending_) {
    for (auto& it : b.items)
      if (it.seg) it.seg->release(it.slot, it.gen);
    if (b.ready) (void)hipEventDestroy(b.ready);
  }
  pending_.clear();
  pending_images_ = 0;
  for (auto& kv : segments_) {
    (void)hipHostUnregister(kv.second.seg->base());
    if (kv.second.mirror_dev) (void)hipFree(kv.second.mirror_dev);
  }
  by_seg_.clear();
  segments_.clear();
  for (auto& kv : keys_) {
    if (kv.second.dev) (void)hipFree(kv.second.dev);
    for (void* d : kv.second.decoded)
      if (d) (void)hipFree(d);
  }
  keys_.clear();
  {
    std::lock_guard<std::mutex> lk(mu_);
    seg_list_.clear();
    for (auto& p : posted_) (void)hipEventDestroy(p.ready);
    posted_.clear();
    for (auto& r : ready_)
      if (r.done) (void)hipEventDestroy(r.done);
    ready_.clear();
  }
  unready_.clear();
  for (auto* p : staging_) (void)hipFree(p);
  staging_.clear();
  if (d_lut_) (void)hipFree(d_lut_);
  if (d_mat_) (void)hipFree(d_mat_);
  d_lut_ = d_mat_ = nullptr;
  pool_.reset();
}

// Descriptors still queued in the sockets when the loader stops would pin
// their producers' ring slots until the lease reclaims them: hand them back
// (the reference's PULL socket simply drops queued messages on close).
void StreamLoader::drain_sockets() {
  for (auto& s : socks_) {
    for (int n = 0; n < 4096; ++n) {
      zmtp::Message m;
      try {
        if (!s->try_recv(m)) break;
      } catch (const zmtp::Error&) {
        break;
      }
      release_descriptor(m);
    }
  }
}

// A received but unprocessed shm descriptor: hand its (still PUBLISHED) slot
// back to the producer.  Anything else needs nothing.
void StreamLoader::release_descriptor(const zmtp::Message& m) {
  if (m.size() != 1) return;
  try {
    codec::DescriptorScan sc;
    if (codec::scan_descriptor(m[0].data(), m[0].size, cfg_.image_key.c_str(), &sc)) {
      auto it = segments_.find(std::string_view(sc.segment.p, sc.segment.n));
      if (it != segments_.end()) {
        it->second.seg->release(uint32_t(sc.slot), uint32_t(sc.gen));
      } else {
        std::unique_ptr<shm::Segment> seg(shm::Segment::open(sc.segment.str()));
        seg->release(uint32_t(sc.slot), uint32_t(sc.gen));
      }
      return;
    }
    codec::VPtr root = codec::parse(m[0].data(), m[0].size);
    if (!root || root->kind != codec::Value::DICT) return;
    const codec::Value* d = root->get("_btshm");
    if (!d || d->kind != codec::Value::TUPLE || d->items.size() < 8 || d->items[0]->kind != codec::Value::STR) return;
    const uint32_t slot = uint32_t(d->items[1]->i), gen = uint32_t(d->items[7]->i);
    auto it = segments_.find(d->items[0]->s);
    if (it != segments_.end()) {
      it->second.seg->release(slot, gen);
    } else {
      std::unique_ptr<shm::Segment> seg(shm::Segment::open(d->items[0]->s));
      seg->release(slot, gen);
    }
  } catch (const std::exception&) {
    // producer gone / not a descriptor: nothing to hand back
  }
}

LoaderStats StreamLoader::stats() {
  std::lock_guard<std::mutex> lk(mu_);
  LoaderStats s = stats_;
  {
    std::lock_guard<std::mutex> tk(tally_mu_);   // frames received since the last launch
    tally_.add_to(s);
  }
  s.cpu_poll_ms = double(cpu_ns_[kCpuPoll].load()) * 1e-6;
  s.cpu_recv_ms = double(cpu_ns_[kCpuRecv].load()) * 1e-6;
  s.cpu_launch_ms = double(cpu_ns_[kCpuLaunch].load()) * 1e-6;
  s.cpu_reap_ms = double(cpu_ns_[kCpuReap].load()) * 1e-6;
  s.worker_tid = worker_tid_.load();
  s.pool_fallbacks = pool_ ? pool_->fallbacks() : 0;
  s.ring_slots = s.ring_published = s.ring_held = 0;
  for (const shm::Segment* g : seg_list_) {
    s.ring_slots += g->nslots();
    s.ring_published += g->count(shm::PUBLISHED);
    s.ring_held += g->count(shm::HELD);
  }
  return s;
}

void StreamLoader::run() {
  check(hipSetDevice(cfg_.device), "hipSetDevice");
  check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
  for (int k = 0; cfg_.copy_streams > 1 && k < std::min(cfg_.copy_streams, 4); ++k) {
    hipStream_t cs;
    hipEvent_t ev;
    check(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking), "hipStreamCreate(copy)");
    check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate(copy)");
    copy_streams_.push_back(cs);
    copy_done_.push_back(ev);
  }
  std::vector<std::pair<zmtp::Socket*, int>> items;
  for (auto& s : socks_) items.emplace_back(s.get(), zmtp::POLLIN);
  std::vector<zmtp::Socket*> ready;
  std::vector<zmtp::Message> round;
  const auto intr = [this] { return stop_.load(); };
  const int64_t max_frames = cfg_.max_batches < 0 ? -1 : cfg_.max_batches * cfg_.batch_size;
  int64_t taken = 0;
  while (!stop_) {
    {
      CpuScope cs(cpu_ns_[kCpuReap]);
      promote_ready();
      reap();
    }
    if (max_frames >= 0 && taken >= max_frames) break;
    std::vector<int> ev;
    try {
      CpuScope cs(cpu_ns_[kCpuPoll]);
      // with copies in flight, wake up often enough to recycle their slots
      // promptly (producers / IO threads may be waiting for them)
      trace::Range tp("btn.loader.poll");
      // batches held behind queued launches (launch_policy.h) leave when one
      // retires: like a completion, that is polled for, never slept through
      const bool held = !pending_.empty() && !inflight_.empty();
      const bool watch = held || !unready_.empty();
      ev = zmtp::Socket::poll(items, inflight_.empty() && pending_.empty() && unready_.empty() ? 100 : (watch ? 0 : 1),
                              intr);
      if (watch && std::none_of(ev.begin(), ev.end(), [](int e) { return e != 0; })) {
        // nothing to receive: poll completions -- back to back for a while
        // after the last frame or hand-off, then at the sleep grain
        if (now_ms() - last_progress_ms_ < spin_ms(cfg_)) cpu_relax();
        else std::this_thread::sleep_for(poll_grain());
      }
    } catch (const zmtp::Error& e) {
      if (e.code == zmtp::E_INTR) break;
      throw;
    }
    CpuScope cs(cpu_ns_[kCpuRecv]);
    flush_pending(max_frames >= 0 && taken >= max_frames);
    ready.clear();
    for (size_t i = 0; i < ev.size(); ++i)
      if (ev[i] & zmtp::POLLIN) ready.push_back(socks_[i].get());
    // Fair fan-in (the reference's PULL contract, examples/datagen/Readme.md:
    // 168-177): every round takes at most ONE message per producer pipe,
    // across all IO sockets, whatever the producer -> socket spread (5
    // producers on 4 sockets put 2 on one).  Draining a socket at a time let
    // a lone producer's socket deliver twice its share.  Rounds repeat until
    // one comes back empty or ~64 frames were taken (amortises the poll).
    size_t woke = 0;
    while (!stop_ && !ready.empty() && woke < 64) {
      const size_t room = max_frames >= 0 ? size_t(std::max<int64_t>(0, max_frames - taken)) : size_t(-1);
      if (room == 0) break;
      round.clear();
      if (zmtp::Socket::recv_round(ready, round, room) == 0) break;
      woke += round.size();
      last_progress_ms_ = now_ms();
      // a launch that finished meanwhile goes to the consumer now, not after
      // the up to 64 frames of this wake-up
      if (!unready_.empty()) promote_ready();
      for (auto& m : round) {
        if (stop_) {
          release_descriptor(m);   // the stream failed / stopped mid-round: hand its shm slot back
          continue;
        }
        if (process(std::move(m))) ++taken;
      }
    }
  }
  if (!stop_) flush_pending(true);   // stream complete: nothing more will join the pending batches
  while (!stop_ && !unready_.empty()) {
    unready_.front().pending->wait();
    promote_ready();
  }
  std::lock_guard<std::mutex> lk(mu_);
  exhausted_ = true;
}

bool StreamLoader::process(zmtp::Message&& msg) {
  trace::Range tr("btn.loader.process");
  auto bad = [&](const std::string& why) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stats_.bad++;
      if (!cfg_.skip_bad && error_.empty()) error_ = "StreamLoader: bad message: " + why;
    }
    cv_.notify_all();
    if (!cfg_.skip_bad) stop_ = true;
    return false;
  };
  if (msg.size() != 1) return bad("expected a single-frame message");
  Item it;
  // a claimed shm slot (and the key-frame reference of a tile16 frame) goes
  // back on every exit that does not hand the item to cur_ -- the bad()
  // returns and the throws alike: a rejected descriptor must not pin a ring
  // slot for the HELD lease (minutes) nor keep a replaced key frame alive
  struct ClaimGuard {
    Item& it;
    bool armed = false;
    ~ClaimGuard() {
      if (!armed) return;
      it.seg->release(it.slot, it.gen);
      if (it.key) it.key->refs--;
      it.key = nullptr;
    }
  } guard{it};
  it.frame = std::move(msg[0]);
  const uint8_t* data = it.frame.data();
  const size_t n = it.frame.size;
  codec::VPtr root;
  // A raw or rgb_a shared-memory descriptor -- every frame of the flagship
  // stream -- is scanned for the three entries the worker reads; its tree is
  // built later by the thread that reads the metadata (BatchMeta::get_tree).
  // Everything else (inline images, tile16 frames, protocol-2 pickles, any
  // shape the scan does not model) is parsed here as before.
  codec::DescriptorScan sc;
  const bool scanned = codec::scan_descriptor(data, n, cfg_.image_key.c_str(), &sc) && sc.tag_elems <= 1;
  if (!scanned) {
    try {
      root = codec::parse(data, n);
    } catch (const std::exception& e) {
      return bad(std::string("unparseable pickle (") + e.what() + ")");
    }
    if (!root || root->kind != codec::Value::DICT) return bad("payload is not a dict");
  }
  size_t img_idx = size_t(-1), shm_idx = size_t(-1);
  for (size_t i = 0; root && i + 1 < root->items.size(); i += 2) {
    if (root->items[i]->kind != codec::Value::STR) continue;
    if (root->items[i]->s == cfg_.image_key) img_idx = i;
    else if (root->items[i]->s == "_btshm") shm_idx = i;
  }
  int h, w, c;
  size_t cut = 0, len = 0;
  if (scanned) {
    // the same checks, in the same order, as the parsed descriptor below
    uint8_t* dev_base = nullptr;
    try {
      MappedSegment& ms = segment(std::string_view(sc.segment.p, sc.segment.n));
      it.seg = ms.seg.get();
      it.ms = &ms;
      dev_base = ms.dev_base;
    } catch (const std::exception& e) {
      return bad(e.what());
    }
    it.slot = uint32_t(sc.slot);
    it.gen = uint32_t(sc.gen);
    const int64_t off = sc.offset;
    h = int(sc.h), w = int(sc.w), c = int(sc.c);
    const bool has_codec = sc.tag_elems == 1;
    if (it.slot >= it.seg->nslots() || off < 0 || (!has_codec && size_t(off) + size_t(h) * w * c > it.seg->size()))
      return bad("_btshm descriptor out of range");
    if (!it.seg->claim(it.slot, it.gen)) {
      std::lock_guard<std::mutex> lk(mu_);
      stats_.shm_stale++;
      return false;
    }
    guard.armed = true;
    it.src = it.seg->base() + off;
    if (dev_base) it.dsrc = dev_base + off;
    if (sc.has_delta) {
      const int64_t lim = int64_t(1) << 20;
      bool ok = true;
      for (size_t k = 1; ok && k < 5; ++k) ok = sc.delta[k] >= -lim && sc.delta[k] <= lim;
      if (ok) {
        it.delta.base_gen = uint32_t(sc.delta[0]);
        it.delta.rect.y0 = int(sc.delta[1]), it.delta.rect.y1 = int(sc.delta[2]);
        it.delta.rect.x0 = int(sc.delta[3]), it.delta.rect.x1 = int(sc.delta[4]);
        ok = mirror::delta_valid(it.delta, h, w);
      }
      if (!ok) return bad("malformed _btshm delta");
      it.has_delta = true;
      // element 11: a mask that does not fit the frame means "no mask"
      if (sc.band_rows > 0) {
        mirror::BlockReport br;
        br.band_rows = sc.band_rows, br.mask = sc.mask, br.bytes = sc.mask_bytes;
        it.has_blocks = mirror::blocks_from_report(br, h, w, &it.blocks);
      }
    }
    if (has_codec && sc.tag0.is(planar::kName)) {
      const size_t slot_lo = it.seg->slot_offset(it.slot);
      if (c != 4 || size_t(off) < slot_lo || !planar::rgb_a_valid(h, w, off, slot_lo + it.seg->slot_bytes()))
        return bad("_btshm rgb_a frame out of range");
      it.planar = true;
    } else if (has_codec) {
      return bad("unknown _btshm codec");
    }
  } else if (shm_idx != size_t(-1)) {
    // descriptor (segment, slot, byte offset, H, W, C, key): image in shared memory
    const codec::Value& d = *root->items[shm_idx + 1];
    if (d.kind != codec::Value::TUPLE || d.items.size() < 8 || d.items[0]->kind != codec::Value::STR)
      return bad("malformed _btshm descriptor");
    uint8_t* dev_base = nullptr;
    try {
      MappedSegment& ms = segment(d.items[0]->s);
      it.seg = ms.seg.get();
      it.ms = &ms;
      dev_base = ms.dev_base;
    } catch (const std::exception& e) {
      return bad(e.what());
    }
    it.slot = uint32_t(d.items[1]->i);
    it.gen = uint32_t(d.items[7]->i);
    const int64_t off = d.items[2]->i;
    h = int(d.items[3]->i), w = int(d.items[4]->i), c = int(d.items[5]->i);
    const bool has_codec = d.items.size() >= 9 && d.items[8]->kind == codec::Value::TUPLE;
    if (it.slot >= it.seg->nslots() || off < 0 || (!has_codec && size_t(off) + size_t(h) * w * c > it.seg->size()))
      return bad("_btshm descriptor out of range");
    if (!it.seg->claim(it.slot, it.gen)) {
      // the producer reclaimed the slot (lease expired while this descriptor
      // sat in a queue): its bytes are another frame's now -- drop it.  Once
      // claimed (HELD) the slot is ours until reap() hands it back.
      std::lock_guard<std::mutex> lk(mu_);
      stats_.shm_stale++;
      return false;
    }
    guard.armed = true;   // claimed: every exit but the hand-over to cur_ gives it back
    it.src = it.seg->base() + off;
    if (dev_base) it.dsrc = dev_base + off;
    if (d.items.size() >= 10 && d.items[9]->kind == codec::Value::TUPLE) {
      // 10th element (base_gen, y0, y1, x0, x1): all of the frame outside the
      // rectangle is what this slot held at generation base_gen (shmring.h)
      const codec::Value& dv = *d.items[9];
      bool ok = dv.items.size() == 5;
      for (size_t k = 0; ok && k < 5; ++k) ok = dv.items[k]->kind == codec::Value::INT;
      const int64_t lim = int64_t(1) << 20;
      for (size_t k = 1; ok && k < 5; ++k) ok = dv.items[k]->i >= -lim && dv.items[k]->i <= lim;
      if (ok) {
        it.delta.base_gen = uint32_t(dv.items[0]->i);
        it.delta.rect.y0 = int(dv.items[1]->i), it.delta.rect.y1 = int(dv.items[2]->i);
        it.delta.rect.x0 = int(dv.items[3]->i), it.delta.rect.x1 = int(dv.items[4]->i);
        ok = mirror::delta_valid(it.delta, h, w);
      }
      if (!ok) return bad("malformed _btshm delta");
      it.has_delta = !has_codec || (d.items[8]->items.size() == 1);   // raw and rgb_a frames only
      if (it.has_delta && d.items.size() >= 11 && d.items[10]->kind == codec::Value::TUPLE &&
          d.items[10]->items.size() == 2 && d.items[10]->items[0]->kind == codec::Value::INT &&
          d.items[10]->items[1]->kind == codec::Value::BYTES) {
        // 11th element (band_rows, mask): which blocks of the rectangle (shmring.h); malformed = no mask
        const codec::Value& bv = *d.items[10];
        mirror::BlockReport br;
        br.band_rows = bv.items[0]->i >= 1 && bv.items[0]->i <= (int64_t(1) << 15) ? int(bv.items[0]->i) : 0;
        br.mask = bv.items[1]->ptr(data), br.bytes = bv.items[1]->len;
        it.has_blocks = mirror::blocks_from_report(br, h, w, &it.blocks);
      }
    }
    const codec::Value* tag = has_codec ? d.items[8].get() : nullptr;
    if (tag && tag->items.size() == 1 && tag->items[0]->kind == codec::Value::STR && tag->items[0]->s == planar::kName) {
      // 9th element ('rgb_a',): packed RGB, then the alpha plane.  The whole
      // H*W*4 frame must lie inside this slot: the kernel reads the RGB part
      // in place and materialize() the alpha plane behind it
      const size_t slot_lo = it.seg->slot_offset(it.slot);
      if (c != 4 || size_t(off) < slot_lo || !planar::rgb_a_valid(h, w, off, slot_lo + it.seg->slot_bytes()))
        return bad("_btshm rgb_a frame out of range");
      it.planar = true;
    } else if (tag) {
      // 9th element (codec, key segment, key generation): key-frame delta
      const codec::Value& cd = *tag;
      if (cd.items.size() < 3 || cd.items[0]->kind != codec::Value::STR || cd.items[0]->s != tiledelta::kName ||
          cd.items[1]->kind != codec::Value::STR)
        return bad("unknown _btshm codec");
      if (!tiledelta::supported(h, w, c)) return bad("tile16 frame size must be a multiple of 16");
      // the tile count and every position must stay inside this slot and
      // frame: the scatter kernel trusts them when it reads host memory
      const size_t slot_end = it.seg->slot_offset(it.slot) + it.seg->slot_bytes();
      if (size_t(off) < it.seg->slot_offset(it.slot) || size_t(off) + 4 > slot_end)
        return bad("_btshm tile16 frame out of range");
      const long ntiles = tiledelta::check(it.src, h, w, c, slot_end - size_t(off));
      if (ntiles < 0) return bad("malformed tile16 frame");
      it.ntiles = int(ntiles);
      try {
        KeyFrame& kf = key_frame(cd.items[1]->s, size_t(h) * w * c);
        kf.refs++;
        it.key = &kf;
        it.key_host = kf.seg->slot(0);
      } catch (const std::exception& e) {
        return bad(e.what());
      }
      it.tiled = true;
    }
    root->items.erase(root->items.begin() + long(shm_idx), root->items.begin() + long(shm_idx) + 2);
  } else {
    if (img_idx == size_t(-1)) return bad("no '" + cfg_.image_key + "' entry");
    const codec::Value& img = *root->items[img_idx + 1];
    if (img.kind != codec::Value::NDARRAY || img.dtype != "|u1" || img.fortran)
      return bad("image must be a C-contiguous uint8 ndarray");
    if (img.shape.size() == 3) {
      h = int(img.shape[0]), w = int(img.shape[1]), c = int(img.shape[2]);
    } else if (img.shape.size() == 2) {
      h = int(img.shape[0]), w = int(img.shape[1]), c = 1;
    } else {
      return bad("image must be HxW or HxWxC");
    }
    if (img.owned) {
      // protocol-2 frame: the pixels were decoded out of latin-1 text, they
      // are not a byte range of the frame -- take them by the copy path
      it.expanded.assign(img.owned->begin() + long(img.off), img.owned->begin() + long(img.off + img.len));
      it.src = it.expanded.data();
    } else {
      it.src = data + img.off;
      if (pool_ && it.frame.buf && it.frame.buf->pinned && it.frame.buf->owner == pool_.get())
        it.dsrc = pool_->device_ptr(it.src);
      cut = img.off, len = img.len;
    }
  }
  if (c < 1 || c > 4) return bad("image channels must be 1..4");
  if (scanned)
    it.flip = sc.has_origin && sc.origin.is("lower-left");
  else if (const codec::Value* o = root->get("origin"))
    it.flip = o->kind == codec::Value::STR && o->s == "lower-left";

  if (!have_shape_) {
    for (int k = 0; k < cfg_.cout; ++k)
      if (cfg_.cmap[k] >= c) throw std::runtime_error("StreamLoader: channel map exceeds image channels");
    if (cfg_.color_matrix && (c != 4 || (int64_t(h) * w) % 256 != 0 || w % 4 != 0))
      throw std::runtime_error("StreamLoader: colour matrix needs RGBA input with H*W % 256 == 0, W % 4 == 0");
    if (cfg_.crop && (!crop::fits(crop_spec(), h, w) || h > INT16_MAX || w > INT16_MAX)) {
      const std::string at = cfg_.crop_mode == crop::kFixed
                                 ? " at (" + std::to_string(cfg_.crop_y0) + ", " + std::to_string(cfg_.crop_x0) + ")"
                                 : std::string();
      return bad("a " + std::to_string(cfg_.crop_h) + "x" + std::to_string(cfg_.crop_w) + " crop window" + at +
                 " does not fit the stream's " + std::to_string(h) + "x" + std::to_string(w) + " frames");
    }
    if (cfg_.resize && (!resized::fits(cfg_.resize_spec, h, w) || h > INT16_MAX || w > INT16_MAX)) {
      const resized::Spec& rs = cfg_.resize_spec;
      const std::string what = rs.mode == resized::kFixed
                                   ? "a " + std::to_string(rs.wh) + "x" + std::to_string(rs.ww) + " resize window at (" +
                                         std::to_string(rs.wy0) + ", " + std::to_string(rs.wx0) + ")"
                                   : std::string("a resize window");
      return bad(what + " does not fit the stream's " + std::to_string(h) + "x" + std::to_string(w) + " frames");
    }
    img_bytes_ = size_t(h) * w * c;
    // (an identity decode with a crop or a resize is no pass-through: it takes the kernel)
    passthrough_ = cfg_.out_dtype == OUT_U8 && cfg_.layout == NHWC && cfg_.cout == c && !cfg_.flip_all &&
                   !cfg_.color_matrix && !cfg_.crop && !cfg_.resize;
    for (int k = 0; passthrough_ && k < c; ++k) {
      passthrough_ = cfg_.cmap[k] == k;
      for (int v = 0; passthrough_ && v < 256; ++v) passthrough_ = cfg_.lut[size_t(k) * 256 + size_t(v)] == float(v);
    }
    // sized for an inline frame of this image even when the first message is a
    // shared-memory descriptor (a few hundred bytes): in a mixed fleet the
    // inline producers' frames must fit the slots, or they land on the heap
    // and their batches fall off the direct path
    const size_t inline_bytes = std::max(n, size_t(h) * w * c + n + 1024);
    size_t slot = cfg_.max_frame_bytes ? cfg_.max_frame_bytes : size_t(double(inline_bytes) * 1.05) + 4096;
    slot = (slot + 4095) & ~size_t(4095);
    int nslots = cfg_.pool_slots;
    if (nslots <= 0) {
      // every pipe may hold RCVHWM queued + 1 partial frame; the worker holds
      // the batch being assembled plus the batches whose copies are in flight
      nslots = int(cfg_.addresses.size()) * (cfg_.rcvhwm + 2) + (cfg_.staging_depth + 12) * cfg_.batch_size;
      nslots = std::max(64, nslots + nslots / 2);
      const size_t cap = size_t(4) << 30;   // <= 4 GiB pinned
      if (size_t(nslots) * slot > cap) nslots = int(std::max<size_t>(16, cap / slot));
    }
    pool_ = std::make_shared<PinnedPool>(slot, nslots);
    // every image-bearing frame goes to a pinned slot (small images too: a
    // frame below 64 KB used to be heap-received and took its batch to the
    // copy path); descriptor-only messages stay on the heap
    for (auto& s : socks_) s->set_allocator(pool_, std::min<size_t>(64 * 1024, size_t(h) * w * c));
    for (int k = 0; k < std::max(2, cfg_.staging_depth); ++k) {
      uint8_t* p = nullptr;
      check(hipMalloc(reinterpret_cast<void**>(&p), img_bytes_ * size_t(cfg_.batch_size)), "hipMalloc(staging)");
      staging_.push_back(p);
    }
    check(hipMalloc(reinterpret_cast<void**>(&d_lut_), kTableFloats * sizeof(float)), "hipMalloc(lut)");
    check(hipMemcpy(d_lut_, cfg_.lut.data(), kTableFloats * sizeof(float), hipMemcpyHostToDevice), "upload lut");
    if (cfg_.color_matrix && !cfg_.jitter) {
      std::vector<float> mb(cfg_.matrices);
      if (mb.empty()) {
        mb = cfg_.matrix;
        mb.insert(mb.end(), cfg_.bias.begin(), cfg_.bias.end());
      }
      check(hipMalloc(reinterpret_cast<void**>(&d_mat_), mb.size() * sizeof(float)), "hipMalloc(matrix)");
      check(hipMemcpy(d_mat_, mb.data(), mb.size() * sizeof(float), hipMemcpyHostToDevice), "upload matrix");
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      H_ = h, W_ = w, C_ = c;
      have_shape_ = true;
    }
    cv_.notify_all();
  } else if (h != H_ || w != W_ || c != C_) {
    return bad("image shape changed within the stream");
  }
  // metadata: the frame minus the image payload, tree re-based onto it
  it.meta.bytes.reserve(n - len);
  it.meta.bytes.insert(it.meta.bytes.end(), data, data + cut);
  it.meta.bytes.insert(it.meta.bytes.end(), data + cut + len, data + n);
  if (len) {
    for (size_t i = 0; i + 1 < root->items.size(); i += 2)
      if (root->items[i]->kind == codec::Value::STR && root->items[i]->s == cfg_.image_key) {
        root->items.erase(root->items.begin() + long(i), root->items.begin() + long(i) + 2);
        break;
      }
    shift_offsets(*root, cut, len);
  }
  it.meta.tree = root;
  it.meta.lazy = scanned;

  if (cfg_.jitter) {
    // splitmix64: brightness, contrast, saturation in [max(0, 1 - r), 1 + r], hue in [-r, r] turns
    for (int k = 0; k < 4; ++k) {
      uint64_t z = (jit_state_ += 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      const float u = float(z >> 40) * (1.f / 16777216.f);   // [0, 1)
      const float r = cfg_.jitter_range[k];
      const float lo = k < 3 ? std::max(0.f, 1.f - r) : -r, hi = k < 3 ? 1.f + r : r;
      it.jit[k] = lo + (hi - lo) * u;
    }
  }
  if (cfg_.crop) {
    if (it.tiled) return bad("tile16 frames cannot be cropped (a crop reads raw or rgb_a frames)");
    it.win = crop::draw(crop_state_, crop_spec(), h, w);
  }
  if (cfg_.resize) {
    if (it.tiled) return bad("tile16 frames cannot be resized (a resize reads raw or rgb_a frames)");
    it.rwin = resized::draw(resize_state_, cfg_.resize_spec, h, w);
  }
  if (cur_.empty()) batch_t0_ = now_ms();
  {
    // per-frame counts go to the worker's tally (its own lock: next() and
    // post() never wait behind a frame); launch_group() folds it into stats_
    // once per launch, and stats() adds what is not folded yet
    std::lock_guard<std::mutex> lk(tally_mu_);
    tally_.frames++;
    tally_.bytes += n;
    if (it.tiled) {
      tally_.image_bytes += 4 * (size_t(it.ntiles) + 1) + size_t(it.ntiles) * tiledelta::tile_bytes(c);
      tally_.tiled_frames++;
    } else if (it.planar) {
      // only the RGB part crosses the link when the frame is read in place;
      // materialize() adds the alpha plane's bytes if it has to rebuild it
      tally_.image_bytes += size_t(h) * w * 3;
      tally_.planar_frames++;
    } else {
      tally_.image_bytes += img_bytes_;
    }
    if (it.seg) tally_.shm_frames++;
    bool has_btid = scanned && sc.has_btid;
    int64_t btid = sc.btid;
    if (!scanned)
      if (const codec::Value* b = root->get("btid"))
        if (b->kind == codec::Value::INT) has_btid = true, btid = b->i;
    if (has_btid) {
      auto e = std::find_if(tally_.btid.begin(), tally_.btid.end(), [&](const auto& kv) { return kv.first == btid; });
      if (e == tally_.btid.end()) tally_.btid.emplace_back(btid, 1);
      else e->second++;
    }
  }
  guard.armed = false;
  cur_.push_back(std::move(it));
  if (int(cur_.size()) == cfg_.batch_size) launch();
  return true;
}

StreamLoader::KeyFrame& StreamLoader::key_frame(const std::string& name, size_t bytes) {
  auto it = keys_.find(name);
  if (it != keys_.end()) return it->second;
  KeyFrame kf;
  kf.seg.reset(shm::Segment::open(name));
  if (kf.seg->nslots() < 1 || kf.seg->slot_bytes() < bytes || kf.seg->state(0) % 4 != shm::PUBLISHED)
    throw std::runtime_error("tile16 key segment " + name + " is not a published key frame");
  // once per producer: the key frame stays in HBM for the stream's lifetime
  check(hipMalloc(reinterpret_cast<void**>(&kf.dev), bytes), "hipMalloc(key frame)");
  check(hipMemcpy(kf.dev, kf.seg->slot(0), bytes, hipMemcpyHostToDevice), "upload key frame");
  return keys_[name] = std::move(kf);
}

const void* StreamLoader::decoded_key(KeyFrame& kf, bool flip, size_t out_img_bytes) {
  void*& d = kf.decoded[flip ? 1 : 0];
  if (d) return d;
  // the key frame through this loader's own decode (table, channels, dtype,
  // layout, flip): every tiled image of this producer starts as a copy of it
  check(hipMalloc(&d, out_img_bytes), "hipMalloc(decoded key)");
  DecodeParams dp;
  dp.src = kf.dev;
  dp.dst = d;
  dp.lut = d_lut_;
  dp.B = 1, dp.H = H_, dp.W = W_, dp.Cin = C_, dp.Cout = cfg_.cout;
  std::memcpy(dp.cmap, cfg_.cmap, sizeof(dp.cmap));
  dp.flip_all = cfg_.flip_all || flip;
  dp.out_dtype = cfg_.out_dtype;
  dp.layout = cfg_.layout;
  check(decode(dp, stream_), "decode(key frame)");
  return d;
}

crop::Spec StreamLoader::crop_spec() const {
  crop::Spec s;
  s.h = cfg_.crop_h, s.w = cfg_.crop_w, s.mode = cfg_.crop_mode;
  s.oy = cfg_.crop_y0, s.ox = cfg_.crop_x0, s.mirror = cfg_.mirror, s.x_align = cfg_.x_align;
  return s;
}

bool StreamLoader::reads_rgb_only() const {
  if (!cfg_.planar_alpha || !cfg_.direct || cfg_.color_matrix || passthrough_) return false;
  for (int k = 0; k < cfg_.cout; ++k)
    if (cfg_.cmap[k] == 3) return false;
  return true;
}

void StreamLoader::materialize(Item& it, bool keep_planar) {
  if (it.planar && !keep_planar) {
    // the batch cannot read packed RGB in place (copy path, alpha needed,
    // colour kernel): back to interleaved RGBA, as tiled frames are rebuilt
    const size_t npix = size_t(H_) * W_;
    it.expanded.resize(img_bytes_);
    planar::interleave_rgb_a(it.expanded.data(), it.src, it.src + npix * 3, npix);
    it.src = it.expanded.data();
    it.dsrc = nullptr;
    it.planar = false;
    std::lock_guard<std::mutex> lk(mu_);
    stats_.image_bytes += npix;
    return;
  }
  if (!it.tiled) return;
  it.expanded.resize(img_bytes_);
  tiledelta::expand(it.src, it.key_host, H_, W_, C_, it.expanded.data());
  it.src = it.expanded.data();
  it.dsrc = nullptr;
  it.tiled = false;
  if (it.key) it.key->refs--;   // rebuilt on the host: the HBM key is not read for it
  it.key = nullptr;
}

StreamLoader::MappedSegment& StreamLoader::segment(std::string_view name_view) {
  auto it = segments_.find(name_view);
  if (it != segments_.end()) return it->second;
  const std::string name(name_view);
  MappedSegment ms;
  ms.seg.reset(shm::Segment::open(name));
  // pin + map the producer's ring: the DMA engine (copy path) or the decode
  // kernel itself (direct path) reads the slots in place
  check(hipHostRegister(ms.seg->base(), ms.seg->size(), hipHostRegisterMapped), "hipHostRegister(shm)");
  if (hipHostGetDevicePointer(reinterpret_cast<void**>(&ms.dev_base), ms.seg->base(), 0) != hipSuccess)
    ms.dev_base = nullptr;
  // tell the producer how this loader reads its frames (sticky, shmring.h):
  // RGB only and in place -> it may keep alpha out of the bytes the kernel
  // pulls over the link; anything else needs interleaved pixels
  ms.seg->add_hint(reads_rgb_only() && ms.dev_base ? shm::kWantPlanarAlpha : shm::kNeedInterleaved);
  // ... and that it keeps slot copies: the producer may report what it rewrote
  // (and, unless BT_SLOT_BLOCKS=0, which blocks of the rectangle: shmring.h kWantSlotBlocks)
  if (mirror_wanted() && ms.dev_base) ms.seg->add_hint(shm::kWantSlotDelta | (slot_blocks_ ? shm::kWantSlotBlocks : 0u));
  ms.ring = mirror::Ring(ms.seg->nslots());
  {
    std::lock_guard<std::mutex> lk(mu_);
    seg_list_.push_back(ms.seg.get());   // ring occupancy in stats()
  }
  MappedSegment& kept = segments_[name] = std::move(ms);
  by_seg_[kept.seg.get()] = &kept;
  return kept;
}

bool StreamLoader::mirror_wanted() const {
  return cfg_.slot_mirror && cfg_.direct && !cfg_.color_matrix && !cfg_.crop && !cfg_.resize && cfg_.decode_streams == 1;
}

// The ring's slot mirror for frames of `cin` stored channels (3: rgb_a slots
// read in place), or null.  It is made when the first frame arrives whose
// producer reports (`reported`): by then the producer has seen this loader's
// hints, so the frame has the layout the ring settles on -- the frames
// published before the hints are read whole, as they would be anyway.  One
// buffer for all the ring's slots.  None when the budget is spent, the frames
// are below the configured size or the allocation fails.  A ring that changes
// its layout later (hints are sticky: a few times in its life at most) gets a
// new buffer; hipFree waits for the launches that read the old one.
uint8_t* StreamLoader::slot_mirror(MappedSegment& ms, int cin, bool reported) {
  if (ms.mirror_dev && ms.mirror_cin == cin) return ms.mirror_dev;
  if (!reported || ms.mirror_failed) return nullptr;
  const size_t frame = size_t(H_) * W_ * size_t(cin);
  const size_t bytes = frame * ms.seg->nslots();
  if (ms.mirror_dev) {
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(ms.mirror_dev);
    const size_t old = size_t(H_) * W_ * size_t(ms.mirror_cin) * ms.seg->nslots();
    ms.mirror_dev = nullptr;
    ms.ring = mirror::Ring(ms.seg->nslots());
    mirror_budget_.release(old);
    std::lock_guard<std::mutex> lk(mu_);
    stats_.mirror_bytes -= old;
  }
  ms.mirror_cin = cin;
  ms.mirror_failed = true;
  if (frame < cfg_.slot_mirror_min_frame_bytes || frame % 16 != 0 || !mirror_budget_.reserve(bytes)) return nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&ms.mirror_dev), bytes) != hipSuccess) {
    (void)hipGetLastError();
    ms.mirror_dev = nullptr;
    mirror_budget_.release(bytes);
    return nullptr;
  }
  ms.mirror_failed = false;
  std::lock_guard<std::mutex> lk(mu_);
  stats_.mirror_bytes += bytes;
  return ms.mirror_dev;
}

void StreamLoader::invalidate_mirror(shm::Segment* seg, uint32_t slot) {
  auto it = by_seg_.find(seg);
  if (it != by_seg_.end()) it->second->ring.invalidate(slot);
}

void StreamLoader::reap(bool wait_all) {
  // drop the frames of batches whose H2D copies completed: their pinned
  // slots return to the pool (and unblock an IO thread waiting for one)
  // (diagnostic BT_LOADER_REAP_US: at most one completion query per interval)
  static const long reap_us = [] {
    const char* e = std::getenv("BT_LOADER_REAP_US");
    return e ? std::atol(e) : 0L;
  }();
  if (reap_us > 0 && !wait_all && !inflight_.empty()) {
    const double t = now_ms();
    if (t - last_reap_ms_ < reap_us * 1e-3) return;
    last_reap_ms_ = t;
  }
  while (!inflight_.empty()) {
    Inflight& f = inflight_.front();
    if (wait_all) f.copied->wait();
    else if (!f.copied->done()) break;
    f.copied.reset();
    if (f.t0) {
      float ms = 0;
      // t1 is recorded behind `copied` (direct path: right behind it; copy
      // path: behind the kernel that follows the copies), so a worker that
      // polls `copied` can be here before t1 completes: wait for it instead
      // of losing the sample
      hipError_t te = hipEventElapsedTime(&ms, f.t0, f.t1);
      if (te == hipErrorNotReady) {
        (void)hipEventSynchronize(f.t1);
        te = hipEventElapsedTime(&ms, f.t0, f.t1);
      }
      if (te == hipSuccess) {
        std::lock_guard<std::mutex> lk(mu_);
        stats_.timed_launches++;
        stats_.timed_images += uint64_t(f.images);
        stats_.timed_gpu_ms += ms;
      }
      time_events_->give(f.t0);
      time_events_->give(f.t1);
    }
    uint64_t torn = 0;
    for (auto& s : f.slots) {
      if (!s.seg->valid(s.slot, s.gen)) {   // a HELD slot taken back (dead-consumer lease)
        torn++;
        invalidate_mirror(s.seg, s.slot);
      }
      s.seg->release(s.slot, s.gen);
    }
    if (torn) {
      // the batch went out with another frame's pixels under its metadata:
      // never deliver that silently (skip_bad only counts it)
      {
        std::lock_guard<std::mutex> lk(mu_);
        stats_.shm_torn += torn;
        if (!cfg_.skip_bad && error_.empty())
          error_ = "StreamLoader: " + std::to_string(torn) +
                   " shared-memory slot(s) were reclaimed by their producer while a batch read them";
      }
      cv_.notify_all();
      if (!cfg_.skip_bad) stop_ = true;
    }
    retired_launch_ = f.launch_no;
    inflight_.pop_front();
  }
  evict_keys();
}

// Key frames a producer replaced (set_key_frame) are never referenced again:
// free their HBM copies once no queued batch and no in-flight launch uses them.
void StreamLoader::evict_keys() {
  for (auto it = keys_.begin(); it != keys_.end();) {
    KeyFrame& kf = it->second;
    if (kf.refs == 0 && kf.last_launch <= retired_launch_ && launch_no_ - kf.last_launch > kKeyIdleLaunches) {
      if (kf.dev) (void)hipFree(kf.dev);
      for (void* d : kf.decoded)
        if (d) (void)hipFree(d);
      {
        std::lock_guard<std::mutex> lk(mu_);
        stats_.keys_evicted++;
      }
      it = keys_.erase(it);
    } else {
      ++it;
    }
  }
}

// One batch of B frames is complete: bind it to the next consumer-posted
// output buffer and queue it for launch.
void StreamLoader::launch() {
  trace::Range tr("btn.loader.assemble");
  Posted p{nullptr, nullptr};
  {
    std::unique_lock<std::mutex> lk(mu_);
    const double t_enter = posted_.empty() ? now_ms() : 0.0;
    const double spin_end = t_enter + spin_ms(cfg_);
    // Start of the stream only: until the consumer has taken its first batch
    // it may still be handing over its first buffers (one device allocation
    // each), which is not being out of them.  The worker assembles a batch in
    // a few tens of microseconds now, less than such a post takes, so batches
    // held for coalescing wait up to this long for the next post (asleep on
    // the condition variable post() signals) before they are flushed; with
    // launch_depth = 0 the first 64 images otherwise went out in two launches
    // about one time in four (tests/test_gpu_loader.py: coalesced_launch).
    // After the first hand-out an empty posted_ flushes at once, as before.
    constexpr double kPostGraceMs = 0.3;
    while (posted_.empty() && !stop_) {
      if (!first_taken_ && !pending_.empty() && now_ms() - t_enter < kPostGraceMs) {
        cv_.wait_for(lk, std::chrono::microseconds(50));
        continue;
      }
      lk.unlock();
      // out of output buffers: the consumer is waiting for batches.  With
      // nothing queued on the GPU, holding assembled ones back would only
      // stall it; behind queued launches they could not start any sooner, so
      // they stay until one retires and then leave together
      // (launch_policy.h).  Every turn reaps and asks again, so a held group
      // goes the moment room opens.
      flush_pending(false, true);
      promote_ready();
      lk.lock();
      if (!posted_.empty() || stop_) break;
      if (now_ms() < spin_end) {
        // the buffer is usually a hand-off away (the consumer posts one for
        // every batch it takes): look again at once before sleeping
        lk.unlock();
        cpu_relax();
        lk.lock();
        continue;
      }
      if (!unready_.empty()) {
        // the consumer is most likely waiting for one of these: keep
        // promoting at a fine grain instead of sleeping through a post
        // (blocking: sleep until the oldest completes, then promote it)
        lk.unlock();
        if (blocking_waits()) unready_.front().pending->wait();
        else std::this_thread::sleep_for(poll_grain());
        lk.lock();
        continue;
      }
      if (!pending_.empty() && !inflight_.empty()) {
        // (no host_sync: nothing is unready) batches held behind queued
        // launches leave when one retires, not when the next buffer is posted
        lk.unlock();
        if (blocking_waits()) inflight_.front().copied->wait();
        else std::this_thread::sleep_for(poll_grain());
        lk.lock();
        continue;
      }
      cv_.wait_for(lk, std::chrono::milliseconds(2));
    }
    if (stop_) return;
    p = posted_.front();
    posted_.pop_front();
  }
  Pending pb;
  pb.dst = p.dst;
  pb.ready = p.ready;
  pb.t0 = batch_t0_;
  auto aligned = [](const Item& it) { return it.dsrc && (reinterpret_cast<uintptr_t>(it.dsrc) % 16) == 0; };
  const bool direct = cfg_.direct && int(cur_.size()) <= kMaxSrcs;
  // a batch of key-frame deltas only decodes as such (fill + tile scatter);
  // in any other batch (copy path, MFMA colour kernel, mixed producers) they
  // are rebuilt on the host
  pb.tiled = direct && !cfg_.color_matrix &&
             std::all_of(cur_.begin(), cur_.end(), [&](const Item& it) { return it.tiled && aligned(it); });
  // rgb_a frames are read in place (Cin = 3) by an RGB-only direct decode;
  // anywhere else they are re-interleaved on the host
  const bool planar_in_place = direct && reads_rgb_only();
  if (!pb.tiled)
    for (auto& it : cur_) materialize(it, planar_in_place && aligned(it));
  // mixed batches stay on the direct path: a frame the kernel cannot read in
  // place (heap-received: dry pool, rebuilt on the host, unaligned) is copied
  // into a free pinned slot here, and the rest are still read where they lie
  if (direct && !pb.tiled && pool_)
    for (auto& it : cur_) {
      if (aligned(it)) continue;
      BufPtr b = pool_->try_alloc(img_bytes_);
      if (!b) break;   // no slot free now: this batch takes the copy path
      std::memcpy(b->data, it.src, img_bytes_);
      it.src = b->data;
      it.dsrc = pool_->device_ptr(b->data);
      it.staged = std::move(b);
      std::lock_guard<std::mutex> lk(mu_);
      stats_.staged_frames++;
    }
  pb.direct = direct && std::all_of(cur_.begin(), cur_.end(), aligned);
  if (!pb.direct)
    for (auto& it : cur_) materialize(it);   // the copy path moves whole interleaved frames
  pb.items = std::move(cur_);
  cur_.clear();
  pending_images_ += int(pb.items.size());
  pending_.push_back(std::move(pb));
  flush_pending(false);
}

// The stream of the next direct-path plain decode.  The extra streams are made
// on first use (a loader that never decodes in place -- copy path, tile16,
// colour kernel -- keeps its single stream).  The decode table was uploaded
// with blocking copies long before, and whatever else the loader stream holds
// at that moment is waited for once, so every stream sees complete tables.
hipStream_t StreamLoader::next_decode_stream() {
  if (decode_streams_.empty()) {
    decode_streams_.push_back(stream_);
    if (cfg_.decode_streams > 1) check(hipStreamSynchronize(stream_), "hipStreamSynchronize(loader stream)");
    for (int k = 1; k < cfg_.decode_streams; ++k) {
      hipStream_t s;
      check(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreate(decode)");
      decode_streams_.push_back(s);
    }
  }
  return decode_streams_[decode_rr_++ % decode_streams_.size()];
}

// Launch coalescing: a direct-path batch launches at once while fewer than
// kMaxInflight launches are queued on the loader stream; otherwise it waits,
// and when a launch retires every waiting batch goes out in ONE kernel
// (per-image source/destination pointers); "queued" counts the launches in
// flight over all decode streams.  When the GPU side is the
// bottleneck the launches therefore grow -- fewer ramp-up/tail phases per
// image -- and when the producers are, every batch still launches at once.
// The decision itself is launch_policy.h's; `ending`: nothing more will join
// the pending batches, `out_of_buffers`: the worker waits for a posted buffer.
void StreamLoader::flush_pending(bool ending, bool out_of_buffers) {
  if (pending_.empty()) return;
  reap();
  policy::State ps;
  ps.pending_batches = int(pending_.size());
  ps.pending_images = pending_images_;
  ps.copy_waiting = std::any_of(pending_.begin(), pending_.end(), [](const Pending& b) { return !b.direct; });
  ps.inflight = int(inflight_.size());
  ps.launch_depth = cfg_.launch_depth;
  ps.batch_size = cfg_.batch_size;
  ps.max_images = kMaxSrcs;
  ps.out_of_buffers = out_of_buffers;
  ps.ending = ending;   // (a stopping loader launches nothing more: stop() hands its pending batches back)
  if (!policy::flush_now(ps)) return;
  // maximal runs of direct batches go out together; copy-path batches one by one
  std::vector<Pending> group;
  auto emit = [&] {
    if (!group.empty()) launch_group(group);
    group.clear();
  };
  while (!pending_.empty()) {
    Pending b = std::move(pending_.front());
    pending_.pop_front();
    if (!b.direct) {
      emit();
      group.push_back(std::move(b));
      emit();
    } else {
      if (!group.empty() && group.front().tiled != b.tiled) emit();   // one kernel family per launch
      group.push_back(std::move(b));
    }
  }
  emit();
  pending_images_ = 0;
}

// Images [lo, lo + n) of a launch over per-image sources as a launch of their own.
static DecodeParams slice_params(const DecodeParams& sp, size_t lo, size_t n, size_t out_img_bytes) {
  DecodeParams part = sp;
  if (lo == 0 && n == size_t(sp.B)) return part;
  std::memset(part.flip_bits, 0, sizeof(part.flip_bits));
  for (size_t i = 0; i < n; ++i) {
    part.srcs[i] = sp.srcs[lo + i];
    if (sp.ndsts) part.dsts[i] = sp.dsts[lo + i];
    if ((sp.flip_bits[(lo + i) >> 6] >> ((lo + i) & 63)) & 1) part.flip_bits[i >> 6] |= uint64_t(1) << (i & 63);
  }
  part.B = part.nsrcs = int(n);
  if (sp.ndsts) part.ndsts = int(n);
  else part.dst = static_cast<uint8_t*>(sp.dst) + lo * out_img_bytes;   // one dense batch: this part's images
  return part;
}

void StreamLoader::launch_group(std::vector<Pending>& group) {
  trace::Range tr("btn.loader.launch");
  CpuScope cpu(cpu_ns_[kCpuLaunch]);
  const double t_issue = now_ms();
  const bool direct = group.front().direct;
  int total = 0;
  // a plain decode of host-resident frames (one kernel, or one per source
  // layout) takes the next decode stream in turn; all the launch's stream-side
  // work below -- post-event waits, timing and completion events, kernels --
  // goes to that one stream.  Everything else stays on the loader stream
  const bool plain = direct && !cfg_.color_matrix && !group.front().tiled;
  const hipStream_t st = plain ? next_decode_stream() : stream_;
  for (auto& b : group) {
    if (cfg_.host_sync) {
      host_wait(b.ready);   // the consumer is done with the buffer
      if (!stop_) post_events_->give(b.ready);   // seen complete: nothing waits on it any more
      else (void)hipEventDestroy(b.ready);
    } else {
      check(hipStreamWaitEvent(st, b.ready, 0), "hipStreamWaitEvent(post)");
      (void)hipEventDestroy(b.ready);
    }
    b.ready = nullptr;
    total += int(b.items.size());
  }
  const size_t elem = cfg_.color_matrix ? 4 : (cfg_.out_dtype == OUT_F32 ? 4 : (cfg_.out_dtype == OUT_U8 ? 1 : 2));
  const int cout = cfg_.cout;   // (colour kernel: 4, or 3 for RGB jitter)
  // (with a crop the output image is the window, with a resize its output size)
  const size_t out_img_bytes = cfg_.resize ? size_t(cfg_.resize_spec.oh) * cfg_.resize_spec.ow * cout * elem
                               : cfg_.crop ? size_t(cfg_.crop_h) * cfg_.crop_w * cout * elem
                                           : size_t(H_) * W_ * cout * elem;
  uint64_t flips[4] = {0, 0, 0, 0};
  std::vector<const Item*> all;
  all.reserve(size_t(total));
  for (auto& b : group)
    for (auto& it : b.items) all.push_back(&it);
  for (int i = 0; i < total; ++i)
    if (all[size_t(i)]->flip) {
      if (i >= 256) throw std::runtime_error("StreamLoader: per-image flip supports batch <= 256");
      flips[i >> 6] |= uint64_t(1) << (i & 63);
    }
  // sampled GPU timing: events bracket this launch's copies + kernel (the
  // stream has already passed the consumers' post events here)
  hipEvent_t t0 = nullptr, t1 = nullptr;
  const int64_t launch_no = ++launch_no_;
  // skip the cold first launches (allocation, code-object load, page faults)
  if (launch_no > kTimedSkip) untimed_images_ += total;
  if (untimed_images_ >= kTimedEveryImages && time_events_->take(&t0) == hipSuccess) {
    untimed_images_ = 0;
    if (time_events_->take(&t1) != hipSuccess || hipEventRecord(t0, st) != hipSuccess) {
      time_events_->give(t0);
      if (t1) time_events_->give(t1);
      t0 = t1 = nullptr;
    }
  }
  uint8_t* stage = nullptr;
  const size_t stage_idx = size_t(batch_index_) % staging_.size();
  const bool passthrough = !direct && passthrough_ &&
                           std::none_of(all.begin(), all.end(), [](const Item* it) { return it->flip; });
  auto copied = std::make_shared<EventSet>();
  copied->pool = done_events_;
  auto add_event = [&](hipStream_t st) {
    hipEvent_t ev;
    check(done_events_->take(&ev), "hipEventCreate(copied)");
    check(hipEventRecord(ev, st), "hipEventRecord(copied)");
    copied->ev.push_back(ev);
  };
  if (passthrough && cfg_.host_sync) {
    // identity decode, host-ordered: the buffer is free (post event seen
    // complete), so the frames go by DMA straight into the consumer's tensor
    // over the copy streams with no stream waits at all; one event per
    // stream marks both the slots' release and the batch's readiness
    const size_t K = std::max<size_t>(1, copy_streams_.size());
    int i = 0;
    for (auto& b : group)
      for (size_t k = 0; k < b.items.size(); ++k, ++i) {
        hipStream_t cs = copy_streams_.empty() ? stream_ : copy_streams_[size_t(i) % K];
        check(hipMemcpyAsync(static_cast<uint8_t*>(b.dst) + k * img_bytes_, all[size_t(i)]->src, img_bytes_,
                             hipMemcpyHostToDevice, cs),
              "hipMemcpyAsync(H2D passthrough)");
      }
    for (size_t k = 0; k < K && k < size_t(total); ++k) add_event(copy_streams_.empty() ? stream_ : copy_streams_[k]);
  } else if (passthrough) {
    // identity decode: the frames go by DMA straight into the consumer's
    // tensor (its post event already gates stream_; the copy streams wait on
    // stream_'s progress through it), and no kernel is launched
    hipEvent_t gate;
    check(hipEventCreateWithFlags(&gate, hipEventDisableTiming), "hipEventCreate(gate)");
    check(hipEventRecord(gate, stream_), "hipEventRecord(gate)");
    const size_t K = std::max<size_t>(1, copy_streams_.size());
    int i = 0;
    for (auto& b : group)
      for (size_t k = 0; k < b.items.size(); ++k, ++i) {
        hipStream_t cs = copy_streams_.empty() ? stream_ : copy_streams_[size_t(i) % K];
        if (cs != stream_ && size_t(i) < K) check(hipStreamWaitEvent(cs, gate, 0), "hipStreamWaitEvent(gate)");
        check(hipMemcpyAsync(static_cast<uint8_t*>(b.dst) + k * img_bytes_, all[size_t(i)]->src, img_bytes_,
                             hipMemcpyHostToDevice, cs),
              "hipMemcpyAsync(H2D passthrough)");
      }
    for (size_t k = 0; k < copy_streams_.size() && k < size_t(total); ++k) {
      check(hipEventRecord(copy_done_[k], copy_streams_[k]), "hipEventRecord(copy)");
      check(hipStreamWaitEvent(stream_, copy_done_[k], 0), "hipStreamWaitEvent(copy)");
    }
    (void)hipEventDestroy(gate);
  } else if (!direct) {   // copy path: exactly one batch per launch
    stage = staging_[stage_idx];
    if (copy_streams_.empty()) {
      for (int i = 0; i < total; ++i)
        check(hipMemcpyAsync(stage + size_t(i) * img_bytes_, all[size_t(i)]->src, img_bytes_, hipMemcpyHostToDevice,
                             stream_),
              "hipMemcpyAsync(H2D)");
    } else {
      // frames round-robin over the copy streams (separate hardware queues,
      // so several DMA engines read host memory at once); each copy stream
      // first waits until the kernel that last read this staging buffer is done
      const size_t K = copy_streams_.size();
      hipEvent_t freed = stage_idx < stage_free_.size() ? stage_free_[stage_idx] : nullptr;
      for (size_t k = 0; k < K && k < size_t(total); ++k) {
        if (freed) check(hipStreamWaitEvent(copy_streams_[k], freed, 0), "hipStreamWaitEvent(stage)");
        for (int i = int(k); i < total; i += int(K))
          check(hipMemcpyAsync(stage + size_t(i) * img_bytes_, all[size_t(i)]->src, img_bytes_,
                               hipMemcpyHostToDevice, copy_streams_[k]),
                "hipMemcpyAsync(H2D)");
        check(hipEventRecord(copy_done_[k], copy_streams_[k]), "hipEventRecord(copy)");
        check(hipStreamWaitEvent(stream_, copy_done_[k], 0), "hipStreamWaitEvent(copy)");
      }
    }
  }
  // `copied` marks the last device read of the host slots: after the copies,
  // or (direct) after the kernel that reads them
  const bool host_passthrough = passthrough && cfg_.host_sync;
  if (!direct && !host_passthrough) add_event(stream_);
  const bool per_image_dst = group.size() > 1;
  hipError_t e = hipSuccess;
  if (passthrough) {
    // nothing to launch: the DMA wrote the output
  } else if (cfg_.color_matrix) {
    Color4x4Params cp;
    cp.src = stage;
    cp.dst = static_cast<float*>(group.front().dst);
    if (direct) {
      cp.nsrcs = total;
      for (int i = 0; i < total; ++i) cp.srcs[i] = all[size_t(i)]->dsrc;
    }
    if (per_image_dst) {
      cp.ndsts = total;
      int i = 0;
      for (auto& b : group)
        for (size_t k = 0; k < b.items.size(); ++k)
          cp.dsts[i++] = reinterpret_cast<float*>(static_cast<uint8_t*>(b.dst) + k * out_img_bytes);
    }
    cp.lut = d_lut_;
    if (cfg_.jitter) {
      cp.mat_mode = kColorJitter;
      cp.pivot = cfg_.pivot;
      for (int i = 0; i < total; ++i) std::memcpy(cp.jit[i], all[size_t(i)]->jit, sizeof(cp.jit[i]));
    } else if (!cfg_.matrices.empty()) {
      cp.mat_mode = kColorPos;
      cp.Ms = d_mat_;
      int i = 0;
      for (auto& b : group)
        for (size_t k = 0; k < b.items.size(); ++k) cp.mat_pos[i++] = uint8_t(k);
    } else {
      cp.M = d_mat_;
      cp.bias = d_mat_ + 16;
    }
    cp.B = total, cp.H = H_, cp.W = W_, cp.Cout = cfg_.cout;
    cp.flip_all = cfg_.flip_all;
    std::memcpy(cp.flip_bits, flips, sizeof(flips));
    e = color4x4(cp, stream_);
  } else {
    // rgb_a frames (direct path only: launch() re-interleaved the others) are
    // read in place as packed RGB, Cin = 3
    int nplanar = 0;
    for (const Item* it : all) nplanar += it->planar ? 1 : 0;
    DecodeParams dp;
    dp.src = stage;
    dp.dst = group.front().dst;
    if (direct) {
      dp.nsrcs = total;
      for (int i = 0; i < total; ++i) dp.srcs[i] = all[size_t(i)]->dsrc;
    }
    if (per_image_dst) {
      dp.ndsts = total;
      int i = 0;
      for (auto& b : group)
        for (size_t k = 0; k < b.items.size(); ++k) dp.dsts[i++] = static_cast<uint8_t*>(b.dst) + k * out_img_bytes;
    }
    dp.lut = d_lut_;
    dp.B = total, dp.H = H_, dp.W = W_, dp.Cin = nplanar == total ? 3 : C_, dp.Cout = cfg_.cout;
    std::memcpy(dp.cmap, cfg_.cmap, sizeof(dp.cmap));
    dp.flip_all = cfg_.flip_all;
    std::memcpy(dp.flip_bits, flips, sizeof(flips));
    dp.out_dtype = cfg_.out_dtype;
    dp.layout = cfg_.layout;
    // crop: the same launches through decode_crop, which reads only each
    // image's window -- of the host frames (direct) or of the staging buffer
    // (copy path: just a dense source)
    CropParams crop;
    crop.h = cfg_.crop_h, crop.w = cfg_.crop_w;
    auto set_window = [](CropParams& c, int n, const Item& it) {
      c.y0[n] = int16_t(it.win.y0), c.x0[n] = int16_t(it.win.x0);
      if (it.win.m) c.mirror_bits |= uint64_t(1) << n;
    };
    if (cfg_.crop) {
      if (total > kMaxSrcs) throw std::runtime_error("StreamLoader: a crop launch holds at most 64 images");
      for (int i = 0; i < total; ++i) set_window(crop, i, *all[size_t(i)]);
      if (direct) {
        // only the windows cross the link: take back what process() counted for whole frames
        uint64_t whole = 0, window = 0;
        for (const Item* it : all) {
          whole += it->planar ? uint64_t(H_) * W_ * 3 : uint64_t(img_bytes_);
          window += uint64_t(cfg_.crop_h) * cfg_.crop_w * (it->planar ? 3 : C_);
        }
        std::lock_guard<std::mutex> lk(mu_);
        stats_.image_bytes -= whole - window;
      }
    }
    // resize: likewise through decode_resize, which stages only the rows of
    // each image's window that its taps touch
    ResizeParams rsz;
    rsz.oh = cfg_.resize_spec.oh, rsz.ow = cfg_.resize_spec.ow;
    auto set_rwindow = [](ResizeParams& r, int n, const Item& it) {
      const resized::Window& v = it.rwin;
      r.y0[n] = int16_t(v.y0), r.x0[n] = int16_t(v.x0), r.h[n] = int16_t(v.h), r.w[n] = int16_t(v.w);
      r.sy[n] = float(v.h) / float(r.oh), r.sx[n] = float(v.w) / float(r.ow);
      if (v.m) r.mirror_bits |= uint64_t(1) << n;
    };
    if (cfg_.resize) {
      if (total > kMaxSrcs) throw std::runtime_error("StreamLoader: a resize launch holds at most 64 images");
      for (int i = 0; i < total; ++i) set_rwindow(rsz, i, *all[size_t(i)]);
      if (direct) {
        // at most the windows cross the link (an upper bound: once the vertical
        // scale exceeds 2 the rows between taps are not read either): take back
        // what process() counted for whole frames
        uint64_t whole = 0, window = 0;
        for (const Item* it : all) {
          whole += it->planar ? uint64_t(H_) * W_ * 3 : uint64_t(img_bytes_);
          window += uint64_t(it->rwin.h) * it->rwin.w * (it->planar ? 3 : C_);
        }
        std::lock_guard<std::mutex> lk(mu_);
        stats_.image_bytes -= whole - window;
      }
    }
    // Slot mirror (slot_mirror.h): a plain decode of ring frames reads, per
    // image, only the region its producer reported as rewritten from the host
    // and the rest from the ring's HBM copy, which the same kernel brings up
    // to date.  Host order is stream order on the one decode stream, so the
    // bookkeeping moves to the frame's generation here, when the launch is
    // queued.  Images without a mirror (pool slots, staged or rebuilt frames,
    // a ring over the budget) ride in the same launch with a null mirror.
    //
    // A launch queued behind one that turns out torn (its slot was taken back
    // by the producer while the kernel read it) is still correct: the producer
    // can only have written inside the rectangle of the frame it was drawing,
    // the next frame of that slot, because the two frames agree everywhere
    // else.  Torn bytes in the copy therefore lie inside the next frame's own
    // reported rectangle and are read again from the host by its launch; what
    // that launch takes from the copy was written by earlier, whole reads.
    // reap() / promote_ready() invalidate the slot's entry all the same, so
    // nothing later relies on a copy a torn read produced.
    // With block masks the same holds block by block, by the rule a producer's
    // mask obeys: every byte the render of a frame stores lies in a set block
    // of that frame's mask, stores that a later one of the same render
    // overwrites included, and every byte outside the set blocks is what the
    // slot held one generation earlier (the render reports the blocks it
    // stored into, sim::Renderer::render's `written`; it leaves alone, and
    // does not report, shadow pixels the slot's last frame left as shadow).
    // A producer that takes a slot back writes nothing before that render,
    // so torn bytes lie inside the next frame's set blocks and are read
    // again from the host; a block clear in that mask was not stored into
    // while this launch read it.
    //
    // Frames that admit a block grid (W % 64 == 0, W <= 1024) take
    // decode_delta_blocks whether their producer sent a mask or only a
    // rectangle (the mask is then built from the widened rectangle), at most
    // kMaxBlockImgs images per launch (the masks travel in the kernel
    // arguments); other sizes, and BT_SLOT_BLOCKS=0, keep decode_delta.
    const bool mirror_on = plain && !cfg_.crop && !cfg_.resize && mirror_wanted();
    // the kernel reads this image in its ring slot?  (not a frame staged or rebuilt elsewhere)
    auto in_slot = [](const Item& it) { return it.ms && !it.staged && it.expanded.empty(); };
    // The mirror of the slot such an image lies in; null when the kernel does
    // not read the image there, or when the slot is not mirrored (now): then
    // whatever the copy held for this slot is no base for a later report.
    auto ring_mirror = [&](const Item& it, int cin, bool ok) -> uint8_t* {
      if (!in_slot(it)) return nullptr;
      uint8_t* m = ok ? slot_mirror(*it.ms, cin, it.has_delta) : nullptr;
      if (!m) it.ms->ring.invalidate(it.slot);
      return m ? m + size_t(it.slot) * size_t(H_) * W_ * size_t(cin) : nullptr;
    };
    auto run_mirror = [&](const DecodeParams& sp, const std::vector<const Item*>& imgs, bool ok, bool by_blocks) {
      uint64_t saved = 0, deltas = 0, fine = 0;
      hipError_t err = hipSuccess;
      const size_t step = by_blocks ? size_t(kMaxBlockImgs) : imgs.size();
      for (size_t lo = 0; lo < imgs.size() && err == hipSuccess; lo += step) {
        const size_t n_here = std::min(imgs.size() - lo, step);
        const DecodeParams part = slice_params(sp, lo, n_here, out_img_bytes);
        DeltaParams dl;
        BlockParams bp;
        bp.band_rows = blocks::band_rows_for(H_);   // one grid per frame size (slot_mirror.h: decide_blocks)
        bool any = false;
        for (size_t n = 0; n < n_here; ++n) {
          const Item& it = *imgs[lo + n];
          uint8_t* m = ring_mirror(it, sp.Cin, ok);
          if (!m) continue;
          const mirror::Delta* report = it.has_delta ? &it.delta : nullptr;
          bool used = false, masked = false;
          int64_t host_pixels;
          if (by_blocks) {
            const mirror::BlockMask bm = it.ms->ring.decide_blocks(it.slot, it.gen, report, it.has_blocks ? &it.blocks : nullptr,
                                                                   H_, W_, &used, &masked);
            bp.mirror[n] = m;
            std::memcpy(bp.mask[n], bm.w, sizeof(bp.mask[n]));
            host_pixels = bm.pixels(H_);
          } else {
            const mirror::Region r = it.ms->ring.decide(it.slot, it.gen, report, H_, W_, &used);
            dl.mirror[n] = m;
            dl.y0[n] = int16_t(r.y0), dl.y1[n] = int16_t(r.y1), dl.x0[n] = int16_t(r.x0), dl.x1[n] = int16_t(r.x1);
            host_pixels = r.pixels();
          }
          any = true;
          if (used) {
            deltas++;
            fine += masked;
            saved += uint64_t(int64_t(H_) * W_ - host_pixels) * uint64_t(sp.Cin);
          }
        }
        err = !any ? decode(part, st) : by_blocks ? decode_delta_blocks(part, bp, st) : decode_delta(part, dl, st);
      }
      // only the regions or set blocks cross the link: take back what process() counted for whole frames
      std::lock_guard<std::mutex> lk(mu_);
      stats_.delta_frames += deltas;
      stats_.block_frames += fine;
      stats_.image_bytes -= saved;
      return err;
    };
    auto run_plain = [&](const DecodeParams& sp, const std::vector<const Item*>& imgs) -> hipError_t {
      bool any_ring = false;
      for (const Item* it : imgs) any_ring = any_ring || in_slot(*it);
      if (!mirror_on || !any_ring) return decode(sp, st);
      // (RGBA -> RGBA u8 NHWC keeps decode()'s 4-pixel host-read shape, kernels.hip launch_out: not mirrored)
      const bool raw_rgba = sp.out_dtype == OUT_U8 && sp.layout == NHWC && sp.Cin == 4 && sp.Cout == 4;
      const bool ok = !raw_rgba && decode_delta_supported(sp);
      return run_mirror(sp, imgs, ok, ok && slot_blocks_ && blocks::width_ok(W_));
    };
    if (nplanar > 0 && nplanar < total) {
      // both source layouts in one group (a mixed fleet with inline
      // producers, or the first frames before a producer saw the hint): one
      // launch per layout, each with its own images, outputs and flip bits
      for (int pl = 0; pl < 2 && e == hipSuccess; ++pl) {
        DecodeParams sp = dp;
        std::memset(sp.flip_bits, 0, sizeof(sp.flip_bits));
        CropParams sc;
        sc.h = crop.h, sc.w = crop.w;
        ResizeParams sr;
        sr.oh = rsz.oh, sr.ow = rsz.ow;
        int n = 0, i = 0;
        std::vector<const Item*> sub;
        for (auto& b : group)
          for (size_t k = 0; k < b.items.size(); ++k, ++i) {
            const Item& it = *all[size_t(i)];
            if (it.planar != (pl == 1)) continue;
            sub.push_back(&it);
            sp.srcs[n] = it.dsrc;
            sp.dsts[n] = static_cast<uint8_t*>(b.dst) + k * out_img_bytes;
            if (it.flip) sp.flip_bits[n >> 6] |= uint64_t(1) << (n & 63);
            if (cfg_.crop) set_window(sc, n, it);
            if (cfg_.resize) set_rwindow(sr, n, it);
            ++n;
          }
        sp.B = sp.nsrcs = sp.ndsts = n;
        sp.Cin = pl == 1 ? 3 : C_;
        e = cfg_.resize ? decode_resize(sp, sr, st) : cfg_.crop ? decode_crop(sp, sc, st) : run_plain(sp, sub);
      }
      // (stats_.launches counts launch groups: this one stays one coalesced
      // launch for the batches in it, run as two kernels)
    } else if (group.front().tiled) {
      TileParams tp;
      tp.out_img_bytes = int64_t(out_img_bytes);
      tp.payload_off = int64_t(tiledelta::payload_offset(H_, W_));
      for (int i = 0; i < total; ++i) {
        const Item& it = *all[size_t(i)];
        it.key->refs--;
        it.key->last_launch = launch_no;
        tp.fills[i] = decoded_key(*it.key, cfg_.flip_all || it.flip, out_img_bytes);
        tp.tile_start[i + 1] = tp.tile_start[i] + it.ntiles;
      }
      e = decode_tiles(dp, tp, stream_);
    } else {
      e = cfg_.resize ? decode_resize(dp, rsz, st) : cfg_.crop ? decode_crop(dp, crop, st) : run_plain(dp, all);
    }
  }
  check(e, "decode kernel launch");
  if (direct) add_event(st);
  if (!direct && !passthrough && !copy_streams_.empty()) {
    if (stage_free_.size() < staging_.size()) stage_free_.resize(staging_.size(), nullptr);
    if (!stage_free_[stage_idx])
      check(hipEventCreateWithFlags(&stage_free_[stage_idx], hipEventDisableTiming), "hipEventCreate(stage)");
    check(hipEventRecord(stage_free_[stage_idx], stream_), "hipEventRecord(stage)");
  }
  if (t0 && host_passthrough) {   // the copies ran on other streams: nothing on stream_ to time
    time_events_->give(t0);
    time_events_->give(t1);
    t0 = t1 = nullptr;
  }
  if (t0) check(hipEventRecord(t1, st), "hipEventRecord(t1)");
  Inflight fl;
  fl.launch_no = launch_no;
  fl.t0 = t0, fl.t1 = t1, fl.images = total;
  fl.frames.reserve(size_t(total));
  std::vector<ReadyBatch> done;
  for (auto& b : group) {
    ReadyBatch rb;
    rb.index = batch_index_++;
    rb.launch_no = launch_no;
    rb.items.reserve(b.items.size());
    for (auto& it : b.items) {
      fl.frames.push_back(std::move(it.frame));
      if (it.seg) {
        fl.slots.push_back({it.seg, it.slot, it.gen});
        if (cfg_.host_sync) rb.slots.push_back({it.seg, it.slot, it.gen});
      }
      if (!it.expanded.empty()) fl.expanded.push_back(std::move(it.expanded));
      if (cfg_.jitter) rb.jitter.insert(rb.jitter.end(), it.jit, it.jit + 4);
      if (cfg_.crop) rb.crop.insert(rb.crop.end(), {it.win.y0, it.win.x0, it.win.m});
      if (cfg_.resize) rb.window.insert(rb.window.end(), {it.rwin.y0, it.rwin.x0, it.rwin.h, it.rwin.w, it.rwin.m});
      if (it.staged) fl.staged.push_back(std::move(it.staged));
      rb.items.push_back(std::move(it.meta));
    }
    if (host_passthrough) {
      rb.pending = copied;        // the DMA is all the batch's device work
    } else if (direct && cfg_.host_sync) {
      // every batch of the group completes where the group's `copied` event
      // sits (right behind the kernel): one marker per launch, owned jointly
      rb.pending = copied;
    } else if (cfg_.host_sync) {
      auto fin = std::make_shared<EventSet>();
      fin->pool = done_events_;
      hipEvent_t ev;
      check(done_events_->take(&ev), "hipEventCreate(done)");
      check(hipEventRecord(ev, st), "hipEventRecord(done)");
      fin->ev.push_back(ev);
      rb.pending = fin;
    } else {
      check(hipEventCreateWithFlags(&rb.done, hipEventDisableTiming), "hipEventCreate(done)");
      check(hipEventRecord(rb.done, st), "hipEventRecord(done)");
    }
    rb.recv_ms = t_issue - b.t0;
    done.push_back(std::move(rb));
  }
  fl.copied = copied;
  inflight_.push_back(std::move(fl));
  {
    std::lock_guard<std::mutex> lk(mu_);
    {
      std::lock_guard<std::mutex> tk(tally_mu_);
      tally_.add_to(stats_);
      tally_.clear();
    }
    stats_.batches += group.size();
    stats_.launches++;
    if (direct) stats_.direct_batches += group.size();
    if (passthrough) stats_.passthrough_batches += group.size();
    stats_.h2d_issue_ms += now_ms() - t_issue;
    if (!cfg_.host_sync)
      for (auto& rb : done) ready_.push_back(std::move(rb));
  }
  if (cfg_.host_sync) {
    for (auto& rb : done) unready_.push_back(std::move(rb));
    promote_ready();
  }
  cv_.notify_all();
}

}  // namespace gpu
}  // namespace btn
