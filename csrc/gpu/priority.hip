// Prioritized replay: the 64-ary integer sum tree of priority.h -- stratified
// draw by tree descent (one wave per batch item), TD-error write-back and the
// eligibility refresh behind an append.  Contracts: priority.h; the numpy
// references: ops.reference_priority_draw / _mass / _extend.
#include <hip/hip_runtime.h>

#include "priority.h"

namespace btn::gpu {

namespace {

constexpr int kWave = 64;

// Philox4x32-10 (Salmon et al., SC'11) with counter words (b, ctr, ctr >> 32,
// c3): the block the replay kernels draw from (kernels.hip philox_block);
// their draws take c3 = 0 .. 5, the prioritized draw takes 6.
__device__ __forceinline__ void philox_block(uint64_t key, uint64_t ctr, uint32_t b, uint32_t c3, uint32_t (&o)[4]) {
  uint32_t c0 = b, c1 = uint32_t(ctr), c2 = uint32_t(ctr >> 32);
  uint32_t k0 = uint32_t(key), k1 = uint32_t(key >> 32);
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0, o[1] = c1, o[2] = c2, o[3] = c3;
}
constexpr uint32_t kPriorityBlock = 6;

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
  const uint32_t lo = __shfl_up(uint32_t(v), d), hi = __shfl_up(uint32_t(v >> 32), d);
  return (uint64_t(hi) << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane) {
  const uint32_t lo = __shfl(uint32_t(v), lane), hi = __shfl(uint32_t(v >> 32), lane);
  return (uint64_t(hi) << 32) | lo;
}

// inclusive prefix sum over the wave's 64 lanes: six shift-and-add steps
__device__ __forceinline__ uint64_t wave_scan(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint64_t o = shfl_up64(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// One wave per batch item.  The descent is nlevels dependent rounds of (one
// coalesced 256- or 512-byte load, a 6-step scan, a ballot): the load's
// latency bounds it, there is nothing to overlap within an item.
__global__ __launch_bounds__(kWave) void priority_draw_kernel(PriorityTree t, PriorityDrawParams d) {
  const int lane = threadIdx.x;
  const uint32_t b = blockIdx.x;
  const uint64_t ctr = d.counter ? d.counter[0] : d.ctr_value;
  uint64_t T = 0, u = 0;
  int64_t node = 0;      // the children of the current node are node * 64 + lane
  uint32_t mass = 0;
#pragma unroll
  for (int l = kMaxPriorityLevels - 1; l >= 0; --l) {
    if (l >= t.nlevels) continue;
    const int64_t i = node * kWave + lane;
    uint64_t v = 0;
    if (i < t.count[l])
      v = l ? static_cast<const uint64_t*>(t.level[l])[i] : uint64_t(static_cast<const uint32_t*>(t.level[0])[i]);
    const uint64_t pre = wave_scan(v, lane);
    if (l == t.nlevels - 1) {
      T = shfl64(pre, kWave - 1);
      if (T == 0) break;
      // floor(b T / B) without a 128-bit product: T = q B + r
      const uint64_t B = uint64_t(d.B), q = T / B, r = T % B;
      const uint64_t lo = b * q + (b * r) / B, hi = (b + 1) * q + ((b + 1) * r) / B;
      uint32_t o[4];
      philox_block(d.seed, ctr, b, kPriorityBlock, o);
      u = lo + __umul64hi((uint64_t(o[0]) << 32) | o[1], hi - lo);
    }
    const unsigned long long over = __ballot(pre > u);
    int pick;
    if (over) {
      pick = __ffsll(over) - 1;
      u -= shfl64(pre - v, pick);
    } else {   // not with a consistent tree (u < the node's sum); stay on a child with mass
      const unsigned long long nz = __ballot(v != 0);
      pick = nz ? 63 - __clzll(nz) : 0;
      u = 0;
    }
    node = node * kWave + pick;
    if (l == 0) mass = __shfl(uint32_t(v), pick);
  }
  if (T == 0) node = 0, mass = 0;
  if (node >= t.capacity) node = t.capacity - 1, mass = 0;   // padding has mass 0: never drawn
  uint32_t last = 0;
  if (lane == 0) {
    d.index_out[b] = node;
    d.prob_out[b] = T ? float(mass) / float(T) : 0.f;
    // the mass goes out write-through, then the ticket: the wave that takes the last one sees every mass
    __hip_atomic_store(d.mass_out + b, mass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    const uint32_t tk = __hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = tk == gridDim.x - 1;
    if (last) {
      __hip_atomic_store(d.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (d.counter && d.advance) d.counter[0] = ctr + uint64_t(d.B);   // every wave read it before its ticket
    }
  }
  if (!__shfl(last, 0)) return;
  __threadfence();
  // importance weights (N prob)^-beta / max = (min mass / mass)^beta
  // all of this lane's masses are loaded before the first is used: one round trip, not one per 64 items
  constexpr int kPerLane = kMaxPriorityB / kWave;
  uint32_t m[kPerLane];
  uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int j = lane + k * kWave;
    m[k] = j < d.B ? __hip_atomic_load(d.mass_out + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xFFFFFFFFu;
  }
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) mn = m[k] < mn ? m[k] : mn;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = __shfl_xor(mn, o);
    mn = other < mn ? other : mn;
  }
  const float beta = d.beta[0];
  const float lmin = mn ? logf(float(mn)) : 0.f;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    const int j = lane + k * kWave;
    if (j < d.B) d.weight_out[j] = mn ? expf(beta * (lmin - logf(float(m[k])))) : 0.f;
  }
}

__device__ __forceinline__ uint32_t mass_of(float p, float alpha) {
  if (!(p > 0.f)) p = 0.f;                         // negative, NaN
  const float x = (alpha == 1.f ? p : powf(p, alpha)) * float(kPriorityOne);
  if (!(x < 4294967296.f)) return 0xFFFFFFFFu;     // +inf and everything past the top mass
  const uint32_t m = uint32_t(rintf(x));
  return m < 1u ? 1u : m;
}

// the leaf takes `mass` by exchange and the difference goes up the tree
__device__ __forceinline__ void leaf_exchange(const PriorityTree& t, int64_t slot, uint32_t mass) {
  const uint32_t old = atomicExch(static_cast<uint32_t*>(t.level[0]) + slot, mass);
  if (old == mass) return;
  const unsigned long long delta = (unsigned long long)(int64_t(mass) - int64_t(old));   // two's complement
  int64_t node = slot;
#pragma unroll
  for (int l = 1; l < kMaxPriorityLevels; ++l) {
    if (l >= t.nlevels) break;
    node >>= 6;
    atomicAdd(static_cast<unsigned long long*>(t.level[l]) + node, delta);
  }
}

// ONE block of B threads (rounded up to whole waves)
__global__ __launch_bounds__(kMaxPriorityB) void priority_update_kernel(PriorityTree t, const int64_t* index,
                                                                        const float* priority, int B, float alpha) {
  // capacity <= 2^31: 0xffffffff marks an index outside the store, and the entries from B to the block's end
  __shared__ __attribute__((aligned(16))) uint32_t slots[kMaxPriorityB];
  const int b = threadIdx.x;
  uint32_t s = 0xFFFFFFFFu;
  if (b < B) {
    const int64_t i = index[b];
    if (i >= 0 && i < t.capacity) s = uint32_t(i);
  }
  slots[b] = s;
  __syncthreads();
  if (s == 0xFFFFFFFFu) return;
  // does a later entry write this slot?  Four entries per LDS read, every lane of a wave at the same address
  // (a broadcast), from the wave's first entry on, and no exit on the way: the reads pipeline
  const uint4* quad = reinterpret_cast<const uint4*>(slots);
  const int nquads = int(blockDim.x) / 4;
  bool later = false;
#pragma unroll 4
  for (int q = (b & ~(kWave - 1)) / 4; q < nquads; ++q) {
    const uint4 w = quad[q];
    const int j = 4 * q;
    later |= (w.x == s && j > b) | (w.y == s && j + 1 > b) | (w.z == s && j + 2 > b) | (w.w == s && j + 3 > b);
  }
  if (later) return;
  uint32_t* leaf = static_cast<uint32_t*>(t.level[0]) + s;
  if (__hip_atomic_load(leaf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;   // ineligible stays 0
  const uint32_t mass = mass_of(priority[b], alpha);
  leaf_exchange(t, int64_t(s), mass);
  atomicMax(t.max_mass, mass);
}

constexpr int kExtendBlock = 256;

__global__ __launch_bounds__(kExtendBlock) void priority_extend_kernel(PriorityTree t, int64_t start, int64_t n,
                                                                       int64_t head, int64_t size, int64_t stride,
                                                                       const uint8_t* first) {
  const int64_t i = int64_t(blockIdx.x) * kExtendBlock + threadIdx.x;
  if (i >= 2 * n) return;
  const int64_t cap = t.capacity;
  // i < n: the appended slot; i >= n: the slot one step before it
  int64_t x = i < n ? start + i : start + (i - n) - stride;
  x %= cap;
  if (x < 0) x += cap;
  int64_t age = (head - 1 - x) % cap;
  if (age < 0) age += cap;
  uint32_t mass = 0;
  if (age < size && age >= stride && first[(x + stride) % cap] == 0) mass = t.max_mass[0];
  leaf_exchange(t, x, mass);
}

bool tree_ok(const PriorityTree& t) {
  if (t.nlevels < 1 || t.nlevels > kMaxPriorityLevels || t.capacity < 1 || t.capacity > (int64_t(1) << 31)) return false;
  if (!t.max_mass || reinterpret_cast<uintptr_t>(t.max_mass) % 4) return false;
  int64_t count = (t.capacity + 63) / 64 * 64;
  for (int l = 0; l < t.nlevels; ++l) {
    if (!t.level[l] || reinterpret_cast<uintptr_t>(t.level[l]) % (l ? 8 : 4)) return false;
    if (l) {
      count /= 64;
      if (count > 64) count = (count + 63) / 64 * 64;
    }
    if (t.count[l] != count) return false;
  }
  return count <= 64;   // the top level is one node's children
}

}  // namespace

hipError_t priority_draw(const PriorityTree& t, const PriorityDrawParams& d, hipStream_t stream) {
  if (!tree_ok(t) || d.B < 0 || d.B > kMaxPriorityB) return hipErrorInvalidValue;
  if (!d.beta || !d.ticket || !d.index_out || !d.mass_out || !d.prob_out || !d.weight_out) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(d.counter) | reinterpret_cast<uintptr_t>(d.index_out)) % 8) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(d.beta) | reinterpret_cast<uintptr_t>(d.ticket) | reinterpret_cast<uintptr_t>(d.mass_out) |
       reinterpret_cast<uintptr_t>(d.prob_out) | reinterpret_cast<uintptr_t>(d.weight_out)) % 4)
    return hipErrorInvalidValue;
  if (d.B == 0) return hipSuccess;
  priority_draw_kernel<<<d.B, kWave, 0, stream>>>(t, d);
  return hipGetLastError();
}

hipError_t priority_update(const PriorityTree& t, const int64_t* index, const float* priority, int B, float alpha,
                           hipStream_t stream) {
  if (!tree_ok(t) || B < 0 || B > kMaxPriorityB || !index || !priority || !(alpha >= 0.f) || !(alpha <= 16.f))
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(index) % 8 || reinterpret_cast<uintptr_t>(priority) % 4) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  priority_update_kernel<<<1, (B + kWave - 1) / kWave * kWave, 0, stream>>>(t, index, priority, B, alpha);
  return hipGetLastError();
}

hipError_t priority_extend(const PriorityTree& t, int64_t start, int64_t n, int64_t head, int64_t size,
                           int64_t stride, const uint8_t* first, hipStream_t stream) {
  if (!tree_ok(t) || !first) return hipErrorInvalidValue;
  const int64_t cap = t.capacity;
  if (n < 0 || n > cap || start < 0 || start >= cap || head < 0 || head >= cap || size < 0 || size > cap ||
      stride < 1 || stride >= cap)
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const int64_t blocks = (2 * n + kExtendBlock - 1) / kExtendBlock;
  priority_extend_kernel<<<dim3(uint32_t(blocks)), kExtendBlock, 0, stream>>>(t, start, n, head, size, stride, first);
  return hipGetLastError();
}

}  // namespace btn::gpu
