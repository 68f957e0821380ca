// Launch policy of the stream loader (csrc/gpu/launch_policy.h) inside a
// discrete-event model of the loader's worker, the GPU queue and the consumer.
// Stand-alone host program, built with -fsanitize=address,undefined by
// tests/test_launch_policy.py.
//
// The model:
//   * batches become available at given times (all at once: GPU-bound; far
//     apart: producer-bound; or at random intervals);
//   * the worker is as fast as it likes: at every event it takes an available
//     batch, binds it to a posted buffer if there is one, and asks the policy
//     -- with out_of_buffers set while it holds a batch and has no buffer --
//     exactly where loader.cpp asks it (top of run(), the wait loop and the
//     end of launch());
//   * a flush sends maximal runs of direct batches as one launch and every
//     copy-path batch alone (loader.cpp: flush_pending);
//   * the GPU runs launches one after another, each a fixed part plus a part
//     per image; when one retires its batches reach the consumer, in order;
//   * the consumer takes a batch, works on it for a while and posts its
//     buffer again.
//
// Checked in every run: every batch is launched once and delivered in order
// (the run never reaches a state without a next event while work is left:
// a pending batch, nothing in flight and no flush), no launch exceeds the
// image cap, copy-path batches launch alone and at once, and with
// launch_depth >= 2 the GPU queue is never empty while a batch is held.
// Producer-bound runs with launch_depth >= 1 launch every batch alone;
// GPU-bound runs with 8 buffers launch fewer times than they have batches.
// The same sweep with the policy's out-of-buffers floor taken away
// (decide(s, 0)) must get stuck: that is the launch_depth = 0 hang the floor
// is there for.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <functional>
#include <queue>
#include <vector>

#include "../gpu/launch_policy.h"

namespace policy = btn::gpu::policy;

namespace {

constexpr double kFixedUs = 17.0;     // ramp, tail and gap of one launch
constexpr double kPerImageUs = 6.3;
constexpr int kMaxImages = 64;

struct Params {
  int launch_depth = 2;
  int prefetch = 8;
  int batches = 8;
  int batch_size = 8;
  int copy_every = 0;               // every n-th batch takes the copy path (0: none)
  std::vector<double> arrive;       // when batch i is complete in the worker's hands
  double consume_us = 1.0;          // consumer's work per batch before it posts the buffer again
  int force_floor = 1;              // 0: the mutant
};

struct Result {
  int launches = 0, delivered = 0;
  bool stuck = false;               // work left and no event to come
  bool out_of_order = false;
  bool over_cap = false;
  bool copy_shared = false;         // a copy-path batch shared a launch or waited
  bool idle_while_held = false;     // GPU queue empty with a batch pending (after the worker acted)
  bool launched_twice = false;
  int held_at_end = 0;              // batches pending when the last one was bound
  int max_group = 0;                // most batches in one launch
};

struct Launch {
  double end;
  std::vector<int> batches;
};

Result simulate(const Params& p) {
  Result r;
  const int N = p.batches;
  double t = 0, gpu_free = 0, consumer_free = 0;
  int next = 0;                     // next batch to bind
  bool have_cur = false;            // batch `next` is complete, waiting for a buffer
  int posted = p.prefetch;
  std::priority_queue<double, std::vector<double>, std::greater<double>> posts;
  std::deque<Launch> inflight;
  std::vector<int> pending;
  std::vector<double> pended_at(size_t(N), -1.0);
  std::vector<int> launched(size_t(N), 0);
  int expect = 0;                   // next batch the consumer should see
  auto is_copy = [&](int b) { return p.copy_every > 0 && b % p.copy_every == p.copy_every - 1; };

  auto launch = [&](const std::vector<int>& group) {
    const int images = int(group.size()) * p.batch_size;
    if (images > kMaxImages) r.over_cap = true;
    for (int b : group) {
      if (launched[size_t(b)]++) r.launched_twice = true;
      if (is_copy(b) && (group.size() != 1 || pended_at[size_t(b)] != t)) r.copy_shared = true;
    }
    const double start = std::max(t, gpu_free);
    gpu_free = start + kFixedUs + kPerImageUs * images;
    inflight.push_back({gpu_free, group});
    r.launches++;
    r.max_group = std::max(r.max_group, int(group.size()));
  };
  auto flush = [&] {
    std::vector<int> group;
    for (int b : pending) {
      if (is_copy(b)) {
        if (!group.empty()) launch(group);
        group.assign(1, b);
        launch(group);
        group.clear();
      } else {
        group.push_back(b);
      }
    }
    if (!group.empty()) launch(group);
    pending.clear();
  };
  auto ask = [&](bool out_of_buffers) {
    policy::State s;
    s.pending_batches = int(pending.size());
    s.pending_images = int(pending.size()) * p.batch_size;
    s.copy_waiting = std::any_of(pending.begin(), pending.end(), is_copy);
    s.inflight = int(inflight.size());
    s.launch_depth = p.launch_depth;
    s.batch_size = p.batch_size;
    s.max_images = kMaxImages;
    s.out_of_buffers = out_of_buffers;
    s.ending = next >= N;
    if (!policy::decide(s, p.force_floor)) return false;
    flush();
    return true;
  };

  for (int guard = 0; guard < 100000; ++guard) {
    // events due now: retirements (batches reach the consumer, which posts
    // each buffer again after its work), then posts
    while (!inflight.empty() && inflight.front().end <= t) {
      for (int b : inflight.front().batches) {
        if (b != expect++) r.out_of_order = true;
        r.delivered++;
        consumer_free = std::max(consumer_free, inflight.front().end) + p.consume_us;
        posts.push(consumer_free);
      }
      inflight.pop_front();
    }
    while (!posts.empty() && posts.top() <= t) {
      posts.pop();
      posted++;
    }
    // the worker acts until it can do no more at this time
    for (bool progress = true; progress;) {
      progress = false;
      if (!have_cur && next < N && p.arrive[size_t(next)] <= t) have_cur = true;
      if (have_cur && posted > 0) {
        posted--;
        pended_at[size_t(next)] = t;
        pending.push_back(next++);
        have_cur = false;
        if (next >= N) r.held_at_end = int(pending.size()) - 1;
        ask(false);                 // end of launch()
        progress = true;
      } else if (have_cur) {
        progress = ask(true);       // the wait loop in launch()
      } else {
        progress = ask(false);      // top of run()
      }
    }
    if (p.launch_depth >= 2 && !pending.empty() && inflight.empty()) r.idle_while_held = true;
    if (next >= N && pending.empty() && inflight.empty()) break;   // all launched and retired
    // the next event
    double nt = -1;
    auto consider = [&](double x) {
      if (x > t && (nt < 0 || x < nt)) nt = x;
    };
    if (!have_cur && next < N) consider(p.arrive[size_t(next)]);
    if (!inflight.empty()) consider(inflight.front().end);
    if (!posts.empty()) consider(posts.top());
    if (nt < 0) {
      r.stuck = true;
      break;
    }
    t = nt;
  }
  if (r.delivered != N) r.stuck = true;
  for (int n : launched)
    if (n != 1) r.stuck = true;
  return r;
}

enum Rate { kGpuBound, kProducerBound, kRandom };

std::vector<double> arrivals(Rate rate, int n, int batch_size, uint32_t seed) {
  std::vector<double> a(size_t(n), 0.0);
  const double kernel = kFixedUs + kPerImageUs * batch_size;
  double t = 0;
  for (int i = 0; i < n; ++i) {
    if (rate == kProducerBound) {
      t += 4 * kernel + 8;          // launch, retirement, consumer and re-post all fit between two batches
    } else if (rate == kRandom) {
      seed = seed * 1664525u + 1013904223u;
      t += 2 * kernel * double(seed >> 8) / double(1u << 24) * ((seed >> 5) & 1);   // bursts and gaps
    }
    a[size_t(i)] = rate == kGpuBound ? 0.0 : t;
  }
  return a;
}

struct Tally {
  int runs = 0, failed = 0, stuck = 0, coalesced = 0, ended_held = 0, max_group = 0;
};

Tally sweep(int force_floor, bool verbose) {
  Tally ty;
  const int depths[] = {0, 1, 2, 3}, prefetches[] = {1, 2, 4, 8}, sizes[] = {8, 3};
  for (int depth : depths)
    for (int prefetch : prefetches)
      for (int n = 1; n <= 40; ++n)
        for (int bs : sizes)
          for (int rate = 0; rate < 3; ++rate)
            for (int copy_every : {0, 3}) {
              Params p;
              p.launch_depth = depth, p.prefetch = prefetch, p.batches = n, p.batch_size = bs;
              p.copy_every = copy_every, p.force_floor = force_floor;
              p.arrive = arrivals(Rate(rate), n, bs, uint32_t(n * 977 + depth * 31 + prefetch));
              if (rate == kRandom) p.consume_us = 40.0;   // a consumer that is sometimes the slower side
              const Result r = simulate(p);
              bool bad = r.stuck || r.out_of_order || r.over_cap || r.copy_shared || r.idle_while_held ||
                         r.launched_twice || r.launches < 1 || r.launches > n;
              if (rate == kProducerBound && depth >= 1 && r.launches != n) bad = true;
              if (rate == kGpuBound && prefetch == 8 && copy_every == 0 && n >= depth + 2 && r.launches >= n) bad = true;
              ty.runs++;
              ty.stuck += r.stuck;
              ty.failed += bad;
              ty.coalesced += r.launches < n;
              ty.ended_held += r.held_at_end > 0 && !r.stuck;
              ty.max_group = std::max(ty.max_group, r.max_group);
              if (bad && verbose)
                std::printf("FAIL depth=%d prefetch=%d batches=%d size=%d rate=%d copy_every=%d: launches=%d delivered=%d "
                            "stuck=%d order=%d cap=%d copy=%d idle=%d twice=%d\n",
                            depth, prefetch, n, bs, rate, copy_every, r.launches, r.delivered, r.stuck, r.out_of_order,
                            r.over_cap, r.copy_shared, r.idle_while_held, r.launched_twice);
            }
  return ty;
}

}  // namespace

int main() {
  const Tally ok = sweep(1, true);
  std::printf("policy: runs=%d failed=%d stuck=%d coalesced=%d ended_held=%d max_group=%d\n", ok.runs, ok.failed, ok.stuck,
              ok.coalesced, ok.ended_held, ok.max_group);
  // the steady state the policy is for: GPU-bound, 8 buffers, launch_depth 2
  Params p;
  p.batches = 40;
  p.arrive = arrivals(kGpuBound, p.batches, p.batch_size, 1);
  const Result h = simulate(p);
  std::printf("headline model: batches=%d launches=%d max_group=%d stuck=%d\n", p.batches, h.launches, h.max_group, h.stuck);
  const Tally mut = sweep(0, false);
  std::printf("mutant (no floor): runs=%d stuck=%d\n", mut.runs, mut.stuck);
  const bool pass = ok.failed == 0 && ok.stuck == 0 && ok.coalesced > 0 && ok.ended_held > 0 && !h.stuck &&
                    h.launches < p.batches && mut.stuck > 0;
  std::printf("%s\n", pass ? "PASS" : "FAILED");
  return pass ? 0 : 1;
}
