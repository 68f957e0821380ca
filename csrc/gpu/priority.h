// Prioritized replay on the device: a 64-ary sum tree of integer masses in
// HBM, a stratified draw by tree descent, the TD-error write-back and the
// eligibility refresh behind an append (csrc/gpu/priority.hip).
//
// Mass: a transition anchored at ring slot s carries a uint32 mass.  0 = the
// anchor may not be drawn (one of the newest `stride` frames, its successor is
// a `first` frame, or the slot is not stored).  An eligible anchor carries
// clamp(rint(priority^alpha * 65536), 1, 2^32 - 1).  *max_mass (device uint32,
// 65536 = priority 1 at the start) is what a freshly appended transition gets;
// only priority_update raises it (atomic max).
//
// Tree: level[0] holds the uint32 masses, level[l >= 1] the uint64 sums of 64
// children each.  count[l] is the number of ALLOCATED nodes of level l:
//     count[0] = capacity rounded up to a multiple of 64
//     count[l] = count[l - 1] / 64, rounded up to a multiple of 64 while it
//                exceeds 64 (a level above it exists); the top level has at
//                most 64 nodes and is not padded
// Padding nodes are 0 and stay 0.  Every number is an integer: sums are exact
// and order-independent, so updates propagate as atomic adds of signed deltas
// and a draw is reproducible on the CPU bit for bit (ops.reference_priority_*).
//
// All three launches run on the caller's stream, allocate nothing, never sync
// and can be captured into a HIP graph.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace btn::gpu {

constexpr int kMaxPriorityLevels = 6;       // capacity <= 2^31
constexpr int kMaxPriorityB = 1024;         // = kMaxReplayB
constexpr uint32_t kPriorityOne = 65536u;   // the mass of priority 1

struct PriorityTree {
  void* level[kMaxPriorityLevels] = {};     // [0]: uint32 (4-byte aligned); [l >= 1]: uint64 (8-byte aligned)
  int64_t count[kMaxPriorityLevels] = {};   // allocated nodes per level (see above)
  int nlevels = 0;
  int64_t capacity = 0;
  uint32_t* max_mass = nullptr;             // [1]
};

// priority_draw: one wave per batch item b < B <= kMaxPriorityB.  With T the
// total mass (the sum of the top level) and C the Philox counter (ctr_value,
// or *counter when counter != nullptr):
//     lo = floor(b T / B), hi = floor((b + 1) T / B)              (stratified)
//     r64 = (o[0] << 32) | o[1] of the Philox4x32-10 block with key seed and
//           counter words (b, C, C >> 32, 6)
//     u = lo + mulhi64(r64, hi - lo)
// and the descent finds the slot whose mass interval holds u: per level, lane
// i loads child i of the node, the wave forms the inclusive uint64 prefix
// sum, the first lane whose prefix exceeds u is the child, and u drops by
// that lane's exclusive prefix.  Outputs, all [B]:
//     index (int64)   the slot (< capacity: padding has mass 0)
//     mass (uint32)   its leaf mass
//     prob (float32)  float(mass) / float(T), one division
//     weight (float32) (min mass of the batch / mass)^beta, computed as
//                     expf(beta * (logf(float(min)) - logf(float(mass)))) by
//                     the last wave to finish (ticket); beta = *beta
// T == 0: index 0, mass 0, prob 0, weight 0.  advance != 0 and a device
// counter: the last wave also adds B to *counter (every wave read it before
// it took its ticket) -- for callers whose next launch does not.
// *ticket (device uint32, 0 between launches) is left 0.
struct PriorityDrawParams {
  int B = 0;
  uint64_t seed = 0;
  uint64_t* counter = nullptr;
  uint64_t ctr_value = 0;
  int advance = 0;
  const float* beta = nullptr;
  uint32_t* ticket = nullptr;
  int64_t* index_out = nullptr;
  uint32_t* mass_out = nullptr;
  float* prob_out = nullptr;
  float* weight_out = nullptr;
};
hipError_t priority_draw(const PriorityTree& t, const PriorityDrawParams& d, hipStream_t stream);

// priority_update: slot index[b] takes the mass of priority[b] (float32;
// negative and NaN count as 0 -> mass 1, +inf -> 2^32 - 1; alpha == 1 skips
// powf, so the mass is exact).  Of duplicates the highest batch position wins
// (all-pairs compare in LDS).  A slot whose mass is 0 (ineligible) stays 0; an
// index outside [0, capacity) is ignored.  The new mass is exchanged into the
// leaf, new - old goes up the tree as 64-bit atomic adds, and *max_mass takes
// an atomic max.
hipError_t priority_update(const PriorityTree& t, const int64_t* index, const float* priority, int B, float alpha,
                           hipStream_t stream);

// priority_extend: the eligibility refresh behind an append of n frames at
// slots start .. start + n - 1 (mod capacity).  head / size: the ring state
// AFTER the append.  Every slot x of that range and every x - stride takes
//     *max_mass  if x is stored, age(x) >= stride and first[(x + stride) % capacity] == 0
//     0          otherwise
// (age(x) = (head - 1 - x) mod capacity) by exchange; the difference goes up
// the tree.  A slot reached twice computes the same mass both times.
hipError_t priority_extend(const PriorityTree& t, int64_t start, int64_t n, int64_t head, int64_t size,
                           int64_t stride, const uint8_t* first, hipStream_t stream);

}  // namespace btn::gpu
