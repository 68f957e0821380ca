// gfx950 kernels for the blendtorch image path (see kernels.h).
//
// decode: pure streaming op (~1.2 MB read, 3.7 MB fp32 written per 640x480
// RGBA image), so it is shaped for HBM, not ALU:
//   * every lane handles PPT consecutive pixels of ONE row, so the HWC->CHW
//     de-interleave happens in registers: one 16-byte load per lane for RGBA
//     (12/24 bytes for RGB) and one 16-byte store per output plane -- the
//     "transpose" needs no LDS round trip because each output plane is a
//     contiguous run of the same pixels;
//   * PPT is picked per output dtype so every plane store is exactly 16 B
//     (f32: 4 px, bf16/f16: 8 px, u8: 16 px);
//   * gamma + scale + per-channel mean/std: the host verifies an arithmetic
//     form of the fp32 reference table (fma, or mul/sub[/div] rounded like
//     numpy) per channel, so the kernel computes the value; only the u8 gamma
//     table is looked up, from a lane-private LDS copy (every lane of a
//     ds_read group owns a bank: no conflicts, whatever the pixel values).
//     Bit-exact with the fp32 reference (kernels.h: lut);
//   * the vertical flip (GL lower-left readback) is a source-row remap.
// color4x4: per-pixel 4x4 affine transform on the matrix cores with
//   v_mfma_f32_4x4x1_16b_f32 (16 independent 4x4 blocks per wave, exact f32):
//   block = 4 pixels x 4 output channels, K = input channel, 16 MFMAs per
//   256 pixels; lane l ends up holding output channel (l & 3) of sixteen
//   consecutive pixels -> four 16-byte stores per lane, plane-contiguous.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "kernels.h"

namespace btn {
namespace gpu {

namespace {

constexpr int kBlock = 256;

// Pixels per lane (every plane store is 16 bytes) and bytes per output element.
constexpr int ppt_for(int out) { return out == OUT_F32 ? 4 : (out == OUT_U8 ? 16 : 8); }
constexpr int elem_for(int out) { return out == OUT_F32 ? 4 : (out == OUT_U8 ? 1 : 2); }

// f(std::integral_constant<int, OUT_...>{}) for the runtime out_dtype.
template <typename F>
hipError_t with_out_dtype(int out_dtype, F&& f) {
  switch (out_dtype) {
    case OUT_F32: return f(std::integral_constant<int, OUT_F32>{});
    case OUT_BF16: return f(std::integral_constant<int, OUT_BF16>{});
    case OUT_F16: return f(std::integral_constant<int, OUT_F16>{});
    case OUT_U8: return f(std::integral_constant<int, OUT_U8>{});
  }
  return hipErrorInvalidValue;
}

__device__ __forceinline__ uint16_t f2bf(float f) {
  // round-to-nearest-even in one v_cvt_pk_bf16_f32 (gfx950)
  return __builtin_bit_cast(uint16_t, static_cast<__bf16>(f));
}

__device__ __forceinline__ uint16_t f2h(float f) {
  _Float16 h = (_Float16)f;
  return *reinterpret_cast<uint16_t*>(&h);
}

// Base of image b's output (elements of type T): per-image pointer when the
// launch coalesces several batches, else the b-th slab of one dense tensor.
template <typename T, typename P>
__device__ __forceinline__ T* image_out(const P& p, int b, int64_t img_elems) {
  return p.ndsts ? reinterpret_cast<T*>(p.dsts[b]) : reinterpret_cast<T*>(p.dst) + int64_t(b) * img_elems;
}

// PPT pixels of CIN u8 channels as 32-bit words; byte j is read by shifts (j a compile-time index
// in every use).  (A byte array written through 16-byte stores and read bytewise was kept on the
// stack in the replay kernels: 64-272 bytes of scratch per lane.)
template <int PPT, int CIN>
struct Pixels {
  static constexpr int NW = (PPT * CIN + 3) / 4;
  uint32_t w[NW];
  __device__ __forceinline__ uint32_t v(int j) const { return (w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }
};

// Load PPT pixels (PPT*CIN bytes) with the widest aligned accesses.
template <int PPT, int CIN>
__device__ __forceinline__ void load_pixels(const uint8_t* p, Pixels<PPT, CIN>& px) {
  constexpr int NB = PPT * CIN;
  if constexpr (NB % 16 == 0) {
#pragma unroll
    for (int i = 0; i < NB / 16; ++i) {
      const uint4 q = reinterpret_cast<const uint4*>(p)[i];
      px.w[4 * i] = q.x, px.w[4 * i + 1] = q.y, px.w[4 * i + 2] = q.z, px.w[4 * i + 3] = q.w;
    }
  } else if constexpr (NB % 8 == 0) {
#pragma unroll
    for (int i = 0; i < NB / 8; ++i) {
      const uint2 q = reinterpret_cast<const uint2*>(p)[i];
      px.w[2 * i] = q.x, px.w[2 * i + 1] = q.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NB / 4; ++i) px.w[i] = reinterpret_cast<const uint32_t*>(p)[i];
  }
}

// ---- value transform (kernels.h: lut) --------------------------------------
// LDS holds either the fp32 table (mode 0, <= 4 KiB) or R copies of the u8
// gamma table: word (v >> 2) * R + (lane % R) packs gamma[v & ~3 .. v | 3],
// so with R = 32 lane l of a 32-lane ds_read group always hits bank l (8 KiB).
constexpr int kTabWords = 2048;

struct Xf {
  int arith;               // 0: fp32 table lookups; 1: arithmetic
  const float* lut;        // LDS fp32 table [c][256] (arith == 0)
  const uint8_t* g;        // this lane's column of the LDS gamma table
  int gshift;              // log2 of a gamma row's bytes (4 * copies)
  int gam[4], op[4];
  float a[4], b[4], d[4], r[4];
};

// Read the header (uniform: scalar loads) and stage the table; caller syncs.
__device__ __forceinline__ Xf stage_xf(const float* T, uint32_t* tab, int nch) {
  Xf x;
  x.arith = T[kXfHeader] != 0.f;
  x.lut = reinterpret_cast<const float*>(tab);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    x.gam[c] = T[kXfHeader + 2 + c] != 0.f;
    x.op[c] = int(T[kXfHeader + 6 + c]);
    x.a[c] = T[kXfHeader + 10 + c];
    x.b[c] = T[kXfHeader + 14 + c];
    x.d[c] = T[kXfHeader + 18 + c];
    x.r[c] = T[kXfHeader + 22 + c];
  }
  // gamma copies R (16 or 32): lane l reads copy l % R.  32 = every lane of a
  // ds_read group owns a bank; 16 = half the fill, lanes l and l+16 share a
  // bank (a 2-way conflict only when their values differ in the same column)
  const int rep = int(T[kXfHeader + 1]);
  x.gshift = rep == 32 ? 7 : 6;                 // bytes per gamma row: 4 * R
  x.g = reinterpret_cast<const uint8_t*>(tab) + (threadIdx.x & (rep - 1)) * 4;
  if (!x.arith) {
    // every load first (4 x 256 threads cover the 4 x 256 table): a
    // load-store loop waited out one round trip per 256 entries
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = int(threadIdx.x) + u * int(blockDim.x);
      v[u] = T[i < nch * 256 ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = int(threadIdx.x) + u * int(blockDim.x);
      if (i < nch * 256) reinterpret_cast<float*>(tab)[i] = v[u];
    }
    for (int i = int(threadIdx.x) + 4 * int(blockDim.x); i < nch * 256; i += blockDim.x)   // (blocks < 256 threads)
      reinterpret_cast<float*>(tab)[i] = T[i];
  } else if (rep > 0) {
    // 16-byte stores: the 4 words of a quad sit in one row (same gamma dword)
    const uint32_t* gw = reinterpret_cast<const uint32_t*>(T + kXfGamma);
    const int qshift = rep == 32 ? 3 : 2;       // quads per row: R / 4
    for (int i = threadIdx.x; i < 16 * rep; i += blockDim.x) {
      const uint32_t w = gw[i >> qshift];
      reinterpret_cast<uint4*>(tab)[i] = make_uint4(w, w, w, w);
    }
  }
  return x;
}

// op 1 / op 2 must round every operation on its own (numpy's float32 order),
// never contract the multiply into an fma
__device__ __forceinline__ float xf_mulsub(float x, float a, float b) {
#pragma clang fp contract(off)
  return x * a - b;
}

// op 3: the quotient by the rounded reciprocal plus one fma correction --
// the host proved it equals the correctly rounded division for every input
__device__ __forceinline__ float xf_recip_div(float t, float d, float r) {
  const float q = t * r;
  return __builtin_fmaf(__builtin_fmaf(-q, d, t), r, q);
}

__device__ __forceinline__ float xf_apply(int op, float x, float a, float b, float d, float r) {
  if (op == 0) return __builtin_fmaf(x, a, b);
  const float t = xf_mulsub(x, a, b);
  if (op == 1) return t;
  return op == 3 ? xf_recip_div(t, d, r) : t / d;   // op 2: correctly rounded fp32 division (HIP default)
}

__device__ __forceinline__ float xf_source(const Xf& xf, int c, uint32_t v) {
  return xf.gam[c] ? float(xf.g[((v >> 2) << xf.gshift) + (v & 3)]) : float(v);
}

// Value of output channel c for input byte v (scalar paths).
__device__ __forceinline__ float xf_value(const Xf& xf, int c, uint32_t v) {
  if (!xf.arith) return xf.lut[c * 256 + v];
  return xf_apply(xf.op[c], xf_source(xf, c, v), xf.a[c], xf.b[c], xf.d[c], xf.r[c]);
}

// Output channel c from input channel IC for the lane's PPT pixels.  The
// channel map is a runtime value, but it is uniform across the wave: `lookup`
// branches on it once (scalar branch) into a fully static body, so every
// byte of `px` is addressed with a compile-time index and `px` stays in
// VGPRs (a dynamically indexed byte array would be spilled to scratch).
template <int PPT, int CIN, int IC, int TBL = 0>
__device__ __forceinline__ void lookup_static(const Pixels<PPT, CIN>& px, const Xf& xf, int c, float (&o)[PPT]) {
  if constexpr (TBL == 2) {   // one table for every output channel, 32 copies: xf.lut is this lane's copy
#pragma unroll
    for (int i = 0; i < PPT; ++i) o[i] = xf.lut[px.v(i * CIN + IC) * 32u];
    return;
  }
  if (TBL || !xf.arith) {   // TBL: the host promised a table-mode value table (no arithmetic code at all)
    const float* l = xf.lut + c * 256;
#pragma unroll
    for (int i = 0; i < PPT; ++i) o[i] = l[px.v(i * CIN + IC)];
    return;
  }
  float x[PPT];
  if (xf.gam[c]) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const uint32_t v = px.v(i * CIN + IC);
      x[i] = float(xf.g[((v >> 2) << xf.gshift) + (v & 3)]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < PPT; ++i) x[i] = float(px.v(i * CIN + IC));
  }
  const float a = xf.a[c], b = xf.b[c], d = xf.d[c], r = xf.r[c];
  if (xf.op[c] == 0) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) o[i] = __builtin_fmaf(x[i], a, b);
  } else if (xf.op[c] == 1) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) o[i] = xf_mulsub(x[i], a, b);
  } else if (xf.op[c] == 3) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) o[i] = xf_recip_div(xf_mulsub(x[i], a, b), d, r);
  } else {
#pragma unroll
    for (int i = 0; i < PPT; ++i) o[i] = xf_mulsub(x[i], a, b) / d;
  }
}

template <int PPT, int CIN, int TBL = 0>
__device__ __forceinline__ void lookup(const Pixels<PPT, CIN>& px, int ic, const Xf& xf, int c, float (&o)[PPT]) {
  switch (ic) {
    case 0: lookup_static<PPT, CIN, 0, TBL>(px, xf, c, o); break;
    case 1: if constexpr (CIN > 1) lookup_static<PPT, CIN, 1, TBL>(px, xf, c, o); break;
    case 2: if constexpr (CIN > 2) lookup_static<PPT, CIN, 2, TBL>(px, xf, c, o); break;
    default: if constexpr (CIN > 3) lookup_static<PPT, CIN, 3, TBL>(px, xf, c, o); break;
  }
}

template <int PPT, int CIN, int OUTT, int COUT, int TBL = 0>
__device__ __forceinline__ void store_nhwc(const DecodeParams& p, const Xf& xf, const int* cm,
                                           const Pixels<PPT, CIN>& px, int b, int64_t q, int64_t HW) {
  constexpr int N = PPT * COUT;
  const int64_t off = q * COUT;   // within image b (NHWC)
  float v[COUT][PPT];
#pragma unroll
  for (int c = 0; c < COUT; ++c) lookup<PPT, CIN, TBL>(px, cm[c], xf, c, v[c]);
  if constexpr (OUTT == OUT_F32) {
    float o[N];
#pragma unroll
    for (int i = 0; i < PPT; ++i)
#pragma unroll
      for (int c = 0; c < COUT; ++c) o[i * COUT + c] = v[c][i];
    float4* d = reinterpret_cast<float4*>(image_out<float>(p, b, HW * COUT) + off);
#pragma unroll
    for (int i = 0; i < N / 4; ++i) d[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
  } else if constexpr (OUTT == OUT_BF16 || OUTT == OUT_F16) {
    uint16_t o[N];
#pragma unroll
    for (int i = 0; i < PPT; ++i)
#pragma unroll
      for (int c = 0; c < COUT; ++c) o[i * COUT + c] = OUTT == OUT_BF16 ? f2bf(v[c][i]) : f2h(v[c][i]);
    uint4* d = reinterpret_cast<uint4*>(image_out<uint16_t>(p, b, HW * COUT) + off);
#pragma unroll
    for (int i = 0; i < N / 8; ++i) d[i] = *reinterpret_cast<const uint4*>(&o[8 * i]);
  } else {
    uint8_t o[N];
#pragma unroll
    for (int i = 0; i < PPT; ++i)
#pragma unroll
      for (int c = 0; c < COUT; ++c) o[i * COUT + c] = uint8_t(v[c][i]);
    uint4* d = reinterpret_cast<uint4*>(image_out<uint8_t>(p, b, HW * COUT) + off);
#pragma unroll
    for (int i = 0; i < N / 16; ++i) d[i] = *reinterpret_cast<const uint4*>(&o[16 * i]);
  }
}

// Where one lane's group of PPT pixels comes from / goes to.
struct Group {
  int b;                 // image
  int64_t q;             // first pixel (row-major) in the image
  const uint8_t* src;    // first source byte (flip applied)
};

// (image, first pixel, row, column) of pixel group g.  32-bit division when
// the launch's group count fits (every real frame batch): a 64-bit divide is a
// ~100-instruction sequence, two per lane and group.
template <int PPT>
__device__ __forceinline__ void split_group(int64_t g, int64_t groups_per_img, int W, bool small, int& b, int64_t& q,
                                            int& y, int& x) {
  if (small) {
    const uint32_t g32 = uint32_t(g), gpi = uint32_t(groups_per_img);
    const uint32_t b32 = g32 / gpi;
    const uint32_t q32 = (g32 - b32 * gpi) * uint32_t(PPT);
    const uint32_t y32 = q32 / uint32_t(W);
    b = int(b32), q = int64_t(q32), y = int(y32), x = int(q32 - y32 * uint32_t(W));
  } else {
    b = int(g / groups_per_img);
    q = (g - int64_t(b) * groups_per_img) * PPT;
    y = int(q / W);
    x = int(q - int64_t(y) * W);
  }
}

template <int PPT, int CIN>
__device__ __forceinline__ Group locate(const DecodeParams& p, int64_t g, int64_t groups_per_img, int64_t HW,
                                        bool small) {
  Group r;
  int y, x;
  split_group<PPT>(g, groups_per_img, p.W, small, r.b, r.q, y, x);
  const int b = r.b;
  const bool flip = p.flip_all || (p.flip && p.flip[b]) || (b < 256 && ((p.flip_bits[b >> 6] >> (b & 63)) & 1));
  const int sy = flip ? p.H - 1 - y : y;
  const uint8_t* img = p.nsrcs ? p.srcs[b] : p.src + (p.src_offsets ? p.src_offsets[b] : int64_t(b) * HW * CIN);
  r.src = img + (int64_t(sy) * p.W + x) * CIN;
  return r;
}

// NT: streaming (non-temporal) stores -- output written once and read by a
// later kernel, kept out of the L2's write-back set (replay sample A/B)
template <int PPT, int CIN, int OUTT, int LAYOUT, int TBL = 0, bool NT = false>
__device__ __forceinline__ void emit(const DecodeParams& p, const Xf& xf, const int* cm, int cout, int64_t HW,
                                     const Group& gr, const Pixels<PPT, CIN>& px) {
  const int b = gr.b;
  const int64_t q = gr.q;
  if constexpr (LAYOUT == NCHW) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= cout) break;
      float v[PPT];
      lookup<PPT, CIN, TBL>(px, cm[c], xf, c, v);
      const int64_t off = int64_t(c) * HW + q;   // within image b (NCHW)
      if constexpr (OUTT == OUT_F32) {
        float* d = image_out<float>(p, b, HW * cout) + off;
        if constexpr (NT) {
          typedef float f4v __attribute__((ext_vector_type(4)));
#pragma unroll
          for (int i = 0; i < PPT / 4; ++i)
            __builtin_nontemporal_store(f4v{v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]},
                                        reinterpret_cast<f4v*>(d) + i);
        } else {
#pragma unroll
          for (int i = 0; i < PPT / 4; ++i) reinterpret_cast<float4*>(d)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        }
      } else if constexpr (OUTT == OUT_BF16 || OUTT == OUT_F16) {
        uint16_t o[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) o[i] = OUTT == OUT_BF16 ? f2bf(v[i]) : f2h(v[i]);
        uint16_t* d = image_out<uint16_t>(p, b, HW * cout) + off;
#pragma unroll
        for (int i = 0; i < PPT / 8; ++i) reinterpret_cast<uint4*>(d)[i] = *reinterpret_cast<const uint4*>(&o[8 * i]);
      } else {
        uint8_t o[PPT];
#pragma unroll
        for (int i = 0; i < PPT; ++i) o[i] = uint8_t(v[i]);
        uint8_t* d = image_out<uint8_t>(p, b, HW * cout) + off;
#pragma unroll
        for (int i = 0; i < PPT / 16; ++i) reinterpret_cast<uint4*>(d)[i] = *reinterpret_cast<const uint4*>(&o[16 * i]);
      }
    }
  } else {
    // NHWC (channels_last): PPT*COUT contiguous elements, assembled in
    // registers and written as 16-byte stores (PPT*sizeof(T) == 16).
    switch (cout) {
      case 1: store_nhwc<PPT, CIN, OUTT, 1, TBL>(p, xf, cm, px, b, q, HW); break;
      case 2: store_nhwc<PPT, CIN, OUTT, 2, TBL>(p, xf, cm, px, b, q, HW); break;
      case 3: store_nhwc<PPT, CIN, OUTT, 3, TBL>(p, xf, cm, px, b, q, HW); break;
      default: store_nhwc<PPT, CIN, OUTT, 4, TBL>(p, xf, cm, px, b, q, HW); break;
    }
  }
}

// Grid-stride over pixel groups; U groups per lane per iteration: all U loads
// are issued before the first table lookup, so each lane keeps U requests in
// flight (memory-level parallelism once the grid is smaller than the work).
template <int PPT, int CIN, int OUTT, int LAYOUT, int U>
__global__ __launch_bounds__(kBlock) void decode_vec_kernel(DecodeParams p) {
  __shared__ uint32_t tab[kTabWords];
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  __syncthreads();

  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t groups_per_img = HW / PPT;
  const int64_t total = groups_per_img * p.B;
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cm[c] = p.cmap[c];
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const bool small = total + U * stride < (int64_t(1) << 31) && HW < (int64_t(1) << 31);

  for (int64_t g0 = int64_t(blockIdx.x) * kBlock + threadIdx.x; g0 < total; g0 += U * stride) {
    const Group gr0 = locate<PPT, CIN>(p, g0, groups_per_img, HW, small);
    Pixels<PPT, CIN> px0;
    load_pixels<PPT, CIN>(gr0.src, px0);
    if constexpr (U == 2) {
      const int64_t g1 = g0 + stride;
      const bool has1 = g1 < total;
      // second group's load goes out before the first group's lookups
      const Group gr1 = locate<PPT, CIN>(p, has1 ? g1 : g0, groups_per_img, HW, small);
      Pixels<PPT, CIN> px1;
      load_pixels<PPT, CIN>(gr1.src, px1);
      emit<PPT, CIN, OUTT, LAYOUT>(p, xf, cm, cout, HW, gr0, px0);
      if (has1) emit<PPT, CIN, OUTT, LAYOUT>(p, xf, cm, cout, HW, gr1, px1);
    } else {
      emit<PPT, CIN, OUTT, LAYOUT>(p, xf, cm, cout, HW, gr0, px0);
    }
  }
}

// Key-frame delta, launch 1: every image starts as its producer's decoded
// key frame (16-byte copies, HBM to HBM).
__global__ __launch_bounds__(kBlock) void tile_fill_kernel(DecodeParams p, TileParams t) {
  const int64_t per = t.out_img_bytes / 16;
  const int64_t total = per * p.B;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < total; i += int64_t(gridDim.x) * kBlock) {
    const int b = int(i / per);
    const int64_t j = i - int64_t(b) * per;
    uint8_t* d = p.ndsts ? static_cast<uint8_t*>(p.dsts[b]) : static_cast<uint8_t*>(p.dst) + int64_t(b) * t.out_img_bytes;
    reinterpret_cast<uint4*>(d)[j] = reinterpret_cast<const uint4*>(t.fills[b])[j];
  }
}

// Key-frame delta, launch 2: decode the payload tiles over the filled images.
// LPT = 256 / PPT lanes per 16x16 tile (64 for f32, 32 bf16/f16, 16 u8); lane
// `idx` of a tile takes PPT pixels of tile row idx / (16 / PPT).
template <int PPT, int CIN, int OUTT, int LAYOUT>
__global__ __launch_bounds__(kBlock) void tile_scatter_kernel(DecodeParams p, TileParams t) {
  __shared__ uint32_t tab[kTabWords];
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  __syncthreads();
  constexpr int T = 16, LPT = T * T / PPT, LPR = T / PPT;
  const int64_t HW = int64_t(p.H) * p.W;
  const int ntx = p.W / T;
  const int64_t total = int64_t(t.tile_start[p.B]) * LPT;
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cm[c] = p.cmap[c];
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += int64_t(gridDim.x) * kBlock) {
    const int gt = int(g / LPT), idx = int(g - int64_t(gt) * LPT);
    int b = 0;
    while (b + 1 < p.B && gt >= t.tile_start[b + 1]) ++b;
    const int k = gt - t.tile_start[b];
    const uint8_t* enc = p.srcs[b];
    // independent loads: the tile's position and its pixels
    const uint32_t pos = reinterpret_cast<const uint32_t*>(enc)[1 + k];
    Pixels<PPT, CIN> px;
    load_pixels<PPT, CIN>(enc + t.payload_off + (int64_t(k) * T * T + int64_t(idx) * PPT) * CIN, px);
    const int r = idx / LPR, col = (idx - r * LPR) * PPT;
    const int sy = int(pos / ntx) * T + r, x = int(pos % ntx) * T + col;
    const bool flip = p.flip_all || (p.flip && p.flip[b]) || (b < 256 && ((p.flip_bits[b >> 6] >> (b & 63)) & 1));
    Group gr;
    gr.b = b;
    gr.q = int64_t(flip ? p.H - 1 - sy : sy) * p.W + x;
    gr.src = nullptr;
    emit<PPT, CIN, OUTT, LAYOUT>(p, xf, cm, cout, HW, gr, px);
  }
}

// Generic fallback: one pixel per thread (any W, any alignment).
template <int OUTT>
__global__ __launch_bounds__(kBlock) void decode_scalar_kernel(DecodeParams p) {
  __shared__ uint32_t tab[kTabWords];
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  __syncthreads();
  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t total = HW * p.B;
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += int64_t(gridDim.x) * kBlock) {
    const int b = int(g / HW);
    const int64_t q = g - int64_t(b) * HW;
    const int y = int(q / p.W), x = int(q - int64_t(y) * p.W);
    const bool flip = p.flip_all || (p.flip && p.flip[b]) || (b < 256 && ((p.flip_bits[b >> 6] >> (b & 63)) & 1));
    const int sy = flip ? p.H - 1 - y : y;
    const uint8_t* img = p.nsrcs ? p.srcs[b] : p.src + (p.src_offsets ? p.src_offsets[b] : int64_t(b) * HW * p.Cin);
    const uint8_t* s = img + (int64_t(sy) * p.W + x) * p.Cin;
    for (int c = 0; c < p.Cout; ++c) {
      const float v = xf_value(xf, c, s[p.cmap[c]]);
      const int64_t off = p.layout == NCHW ? int64_t(c) * HW + q : q * p.Cout + c;   // within image b
      const int64_t ie = HW * p.Cout;
      if constexpr (OUTT == OUT_F32) image_out<float>(p, b, ie)[off] = v;
      else if constexpr (OUTT == OUT_BF16) image_out<uint16_t>(p, b, ie)[off] = f2bf(v);
      else if constexpr (OUTT == OUT_F16) image_out<uint16_t>(p, b, ie)[off] = f2h(v);
      else image_out<uint8_t>(p, b, ie)[off] = uint8_t(v);
    }
  }
}

// ---- crop + mirror (kernels.h: decode_crop) --------------------------------
// The same value path as decode(); only the addressing differs: a lane owns
// PPT consecutive pixels of one WINDOW row, read in place from the source
// frame at window row i -> frame row y0 + i (then the flip), window column j
// -> frame column x0 + j, or x0 + w - 1 - j when the image is mirrored.

// NW dwords from a dword-aligned address, widest loads first
template <int NW>
__device__ __forceinline__ void load_words(const uint8_t* a0, uint32_t (&t)[NW + 1]) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  const uint32_t* s = static_cast<const uint32_t*>(__builtin_assume_aligned(a0, 4));
#pragma unroll
  for (int i = 0; i + 4 <= NW; i += 4) {
    u32x4 q;
    __builtin_memcpy(&q, s + i, 16);
    t[i] = q.x, t[i + 1] = q.y, t[i + 2] = q.z, t[i + 3] = q.w;
  }
  constexpr int R = NW % 4, O = NW - R;
  if constexpr (R >= 2) {
    u32x2 q;
    __builtin_memcpy(&q, s + O, 8);
    t[O] = q.x, t[O + 1] = q.y;
  }
  if constexpr (R == 1 || R == 3) t[NW - 1] = s[NW - 1];
}

// The lane's PPT * CIN bytes from `a`.  CIN == 4: `a` is dword aligned.
// CIN == 3: `a` is only byte aligned (a window may start at any column), so
// the lane reads the dwords its bytes lie in and shifts them into place with
// a byte funnel shift.  Those are the dwords [a0, a0 + 4 NW) with a0 = a & ~3,
// and, when a != a0, the one behind them: a0 holds the lane's first byte, and
// with a != a0 its last byte a + 4 NW - 1 lies in [a0 + 4 NW, a0 + 4 NW + 4).
// So no lane reads a dword without a byte of its own pixels, and as the
// frame's H * W * 3 bytes (W % 4 == 0) end on a dword boundary of its
// 16-byte aligned base, the last window row of the last frame row never
// reads past H * W * CIN.
template <int PPT, int CIN>
__device__ __forceinline__ void load_window_pixels(const uint8_t* a, Pixels<PPT, CIN>& px) {
  constexpr int NW = Pixels<PPT, CIN>::NW;
  uint32_t t[NW + 1];
  if constexpr (CIN == 4) {
    load_words<NW>(a, t);
#pragma unroll
    for (int k = 0; k < NW; ++k) px.w[k] = t[k];
  } else {
    const uint32_t s = uint32_t(reinterpret_cast<uintptr_t>(a)) & 3u;
    const uint8_t* a0 = a - s;
    load_words<NW>(a0, t);
    t[NW] = 0;
    if (s) t[NW] = *reinterpret_cast<const uint32_t*>(a0 + 4 * NW);
#pragma unroll
    for (int k = 0; k < NW; ++k) px.w[k] = __builtin_amdgcn_alignbyte(t[k + 1], t[k], s);
  }
}

// Reverse the order of the lane's PPT pixels (every index a compile-time
// constant once unrolled: shifts and ors on registers, no scratch).
template <int PPT, int CIN>
__device__ __forceinline__ void reverse_pixels(Pixels<PPT, CIN>& px) {
  constexpr int NW = Pixels<PPT, CIN>::NW;
  if constexpr (CIN == 4) {
#pragma unroll
    for (int k = 0; k < NW / 2; ++k) {
      const uint32_t u = px.w[k];
      px.w[k] = px.w[NW - 1 - k];
      px.w[NW - 1 - k] = u;
    }
  } else {
    static_assert(CIN == 3, "packed RGB");
    uint32_t pix[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int k = (3 * i) >> 2, sh = (3 * i) & 3;
      const int k1 = k + 1 < NW ? k + 1 : k;
      const uint32_t lo = px.w[k] >> (8 * sh);
      pix[i] = (sh >= 2 ? lo | (px.w[k1] << (8 * (4 - sh))) : lo) & 0xFFFFFFu;
    }
    uint32_t o[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) o[k] = 0;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int k = (3 * i) >> 2, sh = (3 * i) & 3;
      const uint32_t r = pix[PPT - 1 - i];
      o[k] |= r << (8 * sh);
      if (sh >= 2) o[k + 1 < NW ? k + 1 : k] |= r >> (8 * (4 - sh));
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) px.w[k] = o[k];
  }
}

__device__ __forceinline__ bool image_flipped(const DecodeParams& p, int b) {
  return p.flip_all || (p.flip && p.flip[b]) || (b < 256 && ((p.flip_bits[b >> 6] >> (b & 63)) & 1));
}

template <int PPT, int CIN, int OUTT, int LAYOUT>
__global__ __launch_bounds__(kBlock) void decode_crop_kernel(DecodeParams p, CropParams c) {
  __shared__ uint32_t tab[kTabWords];
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  __syncthreads();

  const int64_t HW = int64_t(p.H) * p.W;       // source frame
  const int64_t hw = int64_t(c.h) * c.w;       // window = output image
  const int64_t groups_per_img = hw / PPT;
  const int64_t total = groups_per_img * p.B;
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cm[k] = p.cmap[k];
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const bool small = total + stride < (int64_t(1) << 31);

  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += stride) {
    Group gr;
    int i, j;   // window row, first window column
    split_group<PPT>(g, groups_per_img, c.w, small, gr.b, gr.q, i, j);
    const int b = gr.b;
    const int y = int(c.y0[b]) + i;
    const int sy = image_flipped(p, b) ? p.H - 1 - y : y;
    // the mirror bit is per image and a wave may straddle two images: the
    // mirrored lanes read the PPT source pixels that end the row's mirror
    // image of their group and reverse them (a branch into a static body)
    const bool mirror = (c.mirror_bits >> b) & 1;
    const int xs = int(c.x0[b]) + (mirror ? c.w - PPT - j : j);
    const uint8_t* img = p.nsrcs ? p.srcs[b] : p.src + (p.src_offsets ? p.src_offsets[b] : int64_t(b) * HW * CIN);
    gr.src = img + (int64_t(sy) * p.W + xs) * CIN;
    Pixels<PPT, CIN> px;
    load_window_pixels<PPT, CIN>(gr.src, px);
    if (mirror) reverse_pixels<PPT, CIN>(px);
    emit<PPT, CIN, OUTT, LAYOUT>(p, xf, cm, cout, hw, gr, px);
  }
}

// Crop-aware fallback: one window pixel per thread (any size, any alignment).
template <int OUTT>
__global__ __launch_bounds__(kBlock) void decode_crop_scalar_kernel(DecodeParams p, CropParams c) {
  __shared__ uint32_t tab[kTabWords];
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  __syncthreads();
  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t hw = int64_t(c.h) * c.w;
  const int64_t total = hw * p.B;
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += int64_t(gridDim.x) * kBlock) {
    const int b = int(g / hw);
    const int64_t q = g - int64_t(b) * hw;
    const int i = int(q / c.w), j = int(q - int64_t(i) * c.w);
    const int y = int(c.y0[b]) + i;
    const int sy = image_flipped(p, b) ? p.H - 1 - y : y;
    const int x = int(c.x0[b]) + (((c.mirror_bits >> b) & 1) ? c.w - 1 - j : j);
    const uint8_t* img = p.nsrcs ? p.srcs[b] : p.src + (p.src_offsets ? p.src_offsets[b] : int64_t(b) * HW * p.Cin);
    const uint8_t* s = img + (int64_t(sy) * p.W + x) * p.Cin;
    for (int k = 0; k < p.Cout; ++k) {
      const float v = xf_value(xf, k, s[p.cmap[k]]);
      const int64_t off = p.layout == NCHW ? int64_t(k) * hw + q : q * p.Cout + k;   // within image b
      const int64_t ie = hw * p.Cout;
      if constexpr (OUTT == OUT_F32) image_out<float>(p, b, ie)[off] = v;
      else if constexpr (OUTT == OUT_BF16) image_out<uint16_t>(p, b, ie)[off] = f2bf(v);
      else if constexpr (OUTT == OUT_F16) image_out<uint16_t>(p, b, ie)[off] = f2h(v);
      else image_out<uint8_t>(p, b, ie)[off] = uint8_t(v);
    }
  }
}

// ---- region read + slot mirror (kernels.h: decode_delta) -------------------
// decode_vec_kernel's groups, table, lookup and stores; only the source of a
// lane's one load differs.  A region starts and ends on multiples of 64
// pixels (or spans full rows) and a group is PPT <= 16 pixels of one row with
// W % PPT == 0, so a group lies inside or outside the region as a whole: the
// base pointer is selected, never branched on, and the load is issued once.

// Store PPT pixels back (the widths load_pixels reads them with).
template <int PPT, int CIN>
__device__ __forceinline__ void store_pixels(uint8_t* p, const Pixels<PPT, CIN>& px) {
  constexpr int NB = PPT * CIN;
  if constexpr (NB % 16 == 0) {
#pragma unroll
    for (int i = 0; i < NB / 16; ++i)
      reinterpret_cast<uint4*>(p)[i] = make_uint4(px.w[4 * i], px.w[4 * i + 1], px.w[4 * i + 2], px.w[4 * i + 3]);
  } else if constexpr (NB % 8 == 0) {
#pragma unroll
    for (int i = 0; i < NB / 8; ++i) reinterpret_cast<uint2*>(p)[i] = make_uint2(px.w[2 * i], px.w[2 * i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < NB / 4; ++i) reinterpret_cast<uint32_t*>(p)[i] = px.w[i];
  }
}

// The inside test is a policy: Args travels beside DecodeParams as a kernel
// argument, stage() fills kLdsWords words of LDS before the block's barrier,
// inside() says whether the group at stored row sy, column x of image b is
// read from the host.

// decode_delta: the rectangle [y0, y1] x [x0, x1] of DeltaParams.
struct RectTest {
  using Args = DeltaParams;
  static constexpr int kLdsWords = 0;
  __device__ __forceinline__ static void stage(const Args&, int, uint32_t*) {}
  __device__ __forceinline__ static bool inside(const Args& d, const uint32_t*, int b, int sy, int x) {
    return sy >= int(d.y0[b]) && sy <= int(d.y1[b]) && x >= int(d.x0[b]) && x <= int(d.x1[b]);
  }
};

// decode_delta_blocks: band sy >> log2(band_rows), column block x >> 6, one
// bit.  Blocks are 64 pixels wide on an absolute grid and W % 64 == 0, so a
// group (PPT <= 16 pixels of one row, W % PPT == 0) never straddles one.  The
// masks arrive in the kernel arguments and are staged to LDS beside the value
// table: row b holds image b's band words.
constexpr int kBlockRowWords = 32;   // uint16 per image: kMaxBlockBands words, padded
struct BlockArgs {
  uint8_t* mirror[kMaxBlockImgs];
  uint16_t rows[kMaxBlockImgs][kBlockRowWords];
  int band_log2;
};
static_assert(kMaxBlockBands <= kBlockRowWords, "a row holds the band words");
static_assert(sizeof(DecodeParams) + sizeof(BlockArgs) <= 4096, "both structs travel as kernel arguments");

struct BlockTest {
  using Args = BlockArgs;
  static constexpr int kLdsWords = kMaxBlockImgs * kBlockRowWords / 2;
  __device__ __forceinline__ static void stage(const Args& d, int B, uint32_t* msk) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&d.rows[0][0]);
    for (int i = threadIdx.x; i < B * (kBlockRowWords / 2); i += kBlock) msk[i] = src[i];
  }
  __device__ __forceinline__ static bool inside(const Args& d, const uint32_t* msk, int b, int sy, int x) {
    const uint16_t* rows = reinterpret_cast<const uint16_t*>(msk);
    const uint32_t word = rows[b * kBlockRowWords + (sy >> d.band_log2)];   // (band < kMaxBlockBands: checked on the host)
    return ((word >> (x >> 6)) & 1u) != 0;
  }
};

template <int PPT, int CIN, int OUTT, int LAYOUT, typename Test>
__global__ __launch_bounds__(kBlock) void decode_mirror_kernel(DecodeParams p, typename Test::Args d) {
  __shared__ uint32_t tab[kTabWords];
  __shared__ uint32_t msk[Test::kLdsWords > 0 ? Test::kLdsWords : 1];
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  Test::stage(d, p.B, msk);
  __syncthreads();

  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t groups_per_img = HW / PPT;
  const int64_t total = groups_per_img * p.B;
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cm[c] = p.cmap[c];
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const bool small = total + stride < (int64_t(1) << 31) && HW < (int64_t(1) << 31);

  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += stride) {
    Group gr;
    int y, x;
    split_group<PPT>(g, groups_per_img, p.W, small, gr.b, gr.q, y, x);
    const int b = gr.b;
    const int sy = image_flipped(p, b) ? p.H - 1 - y : y;
    const int64_t off = (int64_t(sy) * p.W + x) * CIN;
    uint8_t* mir = d.mirror[b];
    const bool inside = mir == nullptr || Test::inside(d, msk, b, sy, x);
    const uint8_t* base = inside ? p.srcs[b] : mir;
    gr.src = base + off;
    Pixels<PPT, CIN> px;
    load_pixels<PPT, CIN>(gr.src, px);
    if (inside && mir != nullptr) store_pixels<PPT, CIN>(mir + off, px);
    emit<PPT, CIN, OUTT, LAYOUT>(p, xf, cm, cout, HW, gr, px);
  }
}

int grid_for(int64_t work, int cap = 0) {
  // Measured on MI355X (profiles/decode_unroll_sweep.txt): up to ~4k blocks
  // of work, one resident wave of 2048 blocks (256 CUs x 8) is best; for
  // large batches a grid of 8192 blocks keeps more stores in flight
  // (64 x 640x480 RGBA -> f32: 74.7 us at 2048 blocks, 63.3 us at 8192).
  int64_t blocks = (work + kBlock - 1) / kBlock;
  if (cap <= 0) cap = blocks > 4096 ? 8192 : 2048;
  return int(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

template <typename T>
bool dsts_ok(T* const* dsts, int n, int B, uintptr_t align) {
  if (n != B) return false;
  for (int b = 0; b < n; ++b)
    if (!dsts[b] || (reinterpret_cast<uintptr_t>(dsts[b]) % align) != 0) return false;
  return true;
}

bool srcs_ok(const uint8_t* const* srcs, int n, int B, uintptr_t align) {
  if (n != B) return false;
  for (int b = 0; b < n; ++b)
    if (!srcs[b] || (reinterpret_cast<uintptr_t>(srcs[b]) % align) != 0) return false;
  return true;
}

template <int PPT, int CIN, int OUTT, int U>
void launch_vec_u(const DecodeParams& p, int grid, hipStream_t s) {
  if (p.layout == NCHW)
    decode_vec_kernel<PPT, CIN, OUTT, NCHW, U><<<grid, kBlock, 0, s>>>(p);
  else
    decode_vec_kernel<PPT, CIN, OUTT, NHWC, U><<<grid, kBlock, 0, s>>>(p);
}

template <int PPT, int CIN, int OUTT>
hipError_t launch_vec(const DecodeParams& p, hipStream_t s) {
  int64_t work = int64_t(p.B) * p.H * p.W / PPT;
  // launch-shape overrides for sweeps (BT_DECODE_MAXGRID / BT_DECODE_UNROLL)
  static const int env_grid = std::getenv("BT_DECODE_MAXGRID") ? std::atoi(std::getenv("BT_DECODE_MAXGRID")) : 0;
  static const int env_unroll = std::getenv("BT_DECODE_UNROLL") ? std::atoi(std::getenv("BT_DECODE_UNROLL")) : 0;
  const int grid = grid_for(work, p.max_grid > 0 ? p.max_grid : env_grid);
  // U=2 (two groups' loads in flight per lane) measured no faster than U=1
  // at 8 or 64 frames once the grid is sized right; kept as an option
  const int req = p.unroll > 0 ? p.unroll : env_unroll;
  const int u = req > 0 ? req : 1;
  if (u >= 2)
    launch_vec_u<PPT, CIN, OUTT, 2>(p, grid, s);
  else
    launch_vec_u<PPT, CIN, OUTT, 1>(p, grid, s);
  return hipGetLastError();
}

template <int OUTT>
hipError_t launch_out(const DecodeParams& p, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  // vector path: a lane's PPT pixels sit in one row and its loads are aligned
  const bool src_aligned = p.nsrcs ? srcs_ok(p.srcs, p.nsrcs, p.B, 16)
                                   : (reinterpret_cast<uintptr_t>(p.src) % 16) == 0 && (p.src_offsets == nullptr || p.src_offsets_aligned);
  const bool dst_aligned = p.ndsts ? dsts_ok(p.dsts, p.ndsts, p.B, 16) : (reinterpret_cast<uintptr_t>(p.dst) % 16) == 0;
  bool aligned = (p.W % PPT) == 0 && (int64_t(p.H) * p.W * p.Cin) % 16 == 0 && dst_aligned && src_aligned;
  if constexpr (OUTT == OUT_U8) {
    // RGBA -> RGBA u8 NHWC read from HOST memory (the scatter root's raw
    // frames): 4 pixels per lane, one 16-byte load and one 16-byte store, so
    // 4x the lanes of the 16-pixel shape keep PCIe read requests in flight
    // (the 16-pixel shape read host frames at ~36 GB/s against ~50)
    if (p.nsrcs && p.layout == NHWC && p.Cin == 4 && p.Cout == 4 && aligned && (p.W % 4) == 0)
      return launch_vec<4, 4, OUTT>(p, s);
  }
  if (aligned && p.Cin == 4) return launch_vec<PPT, 4, OUTT>(p, s);
  if (aligned && p.Cin == 3) return launch_vec<PPT, 3, OUTT>(p, s);
  int64_t work = int64_t(p.B) * p.H * p.W;
  decode_scalar_kernel<OUTT><<<grid_for(work, p.max_grid), kBlock, 0, s>>>(p);
  return hipGetLastError();
}

}  // namespace

template <int PPT, int CIN, int OUTT>
void launch_tiles(const DecodeParams& p, const TileParams& t, int grid, hipStream_t s) {
  if (p.layout == NCHW)
    tile_scatter_kernel<PPT, CIN, OUTT, NCHW><<<grid, kBlock, 0, s>>>(p, t);
  else
    tile_scatter_kernel<PPT, CIN, OUTT, NHWC><<<grid, kBlock, 0, s>>>(p, t);
}

template <int OUTT>
void launch_tiles_out(const DecodeParams& p, const TileParams& t, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  const int64_t work = int64_t(t.tile_start[p.B]) * (256 / PPT);
  if (work <= 0) return;
  const int grid = grid_for(work, p.max_grid);
  if (p.Cin == 4)
    launch_tiles<PPT, 4, OUTT>(p, t, grid, s);
  else
    launch_tiles<PPT, 3, OUTT>(p, t, grid, s);
}

hipError_t decode(const DecodeParams& p, hipStream_t stream) {
  if (p.B <= 0 || p.H <= 0 || p.W <= 0) return hipSuccess;
  if (p.Cout < 1 || p.Cout > 4 || p.Cin < 1 || p.Cin > 4) return hipErrorInvalidValue;
  if (p.nsrcs && (p.nsrcs != p.B || p.nsrcs > kMaxSrcs || !srcs_ok(p.srcs, p.nsrcs, p.B, 1))) return hipErrorInvalidValue;
  if (p.ndsts && (p.ndsts != p.B || p.ndsts > kMaxSrcs || !dsts_ok(p.dsts, p.ndsts, p.B, 1))) return hipErrorInvalidValue;
  for (int c = 0; c < p.Cout; ++c)
    if (p.cmap[c] < 0 || p.cmap[c] >= p.Cin) return hipErrorInvalidValue;
  return with_out_dtype(p.out_dtype, [&](auto o) { return launch_out<o()>(p, stream); });
}

namespace {

template <int PPT, int CIN, int OUTT>
void launch_crop_vec(const DecodeParams& p, const CropParams& c, hipStream_t s) {
  const int grid = grid_for(int64_t(p.B) * c.h * c.w / PPT, p.max_grid);
  if (p.layout == NCHW)
    decode_crop_kernel<PPT, CIN, OUTT, NCHW><<<grid, kBlock, 0, s>>>(p, c);
  else
    decode_crop_kernel<PPT, CIN, OUTT, NHWC><<<grid, kBlock, 0, s>>>(p, c);
}

template <int OUTT>
hipError_t launch_crop_out(const DecodeParams& p, const CropParams& c, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  constexpr int64_t ELEM = elem_for(OUTT);
  // vector path: a lane's PPT pixels sit in one window row, every image's
  // source misalignment is a whole number of bytes below a dword of a
  // 16-byte aligned frame whose rows are dword multiples, and the 16-byte
  // plane / pixel-run stores are aligned
  const bool src_aligned = p.nsrcs ? srcs_ok(p.srcs, p.nsrcs, p.B, 16)
                                   : (reinterpret_cast<uintptr_t>(p.src) % 16) == 0 &&
                                         (p.src_offsets ? p.src_offsets_aligned != 0
                                                        : (int64_t(p.H) * p.W * p.Cin) % 16 == 0);
  const bool dst_aligned = p.ndsts ? dsts_ok(p.dsts, p.ndsts, p.B, 16) : (reinterpret_cast<uintptr_t>(p.dst) % 16) == 0;
  const bool vec = (c.w % PPT) == 0 && (p.W % 4) == 0 && src_aligned && dst_aligned &&
                   (int64_t(c.h) * c.w * p.Cout * ELEM) % 16 == 0;
  if (vec && p.Cin == 4) {
    launch_crop_vec<PPT, 4, OUTT>(p, c, s);
  } else if (vec && p.Cin == 3) {
    launch_crop_vec<PPT, 3, OUTT>(p, c, s);
  } else {
    const int64_t work = int64_t(p.B) * c.h * c.w;
    decode_crop_scalar_kernel<OUTT><<<grid_for(work, p.max_grid), kBlock, 0, s>>>(p, c);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t decode_crop(const DecodeParams& p, const CropParams& c, hipStream_t stream) {
  // every condition is checked here, before anything is launched
  if (p.B < 0 || p.B > kMaxSrcs || p.H <= 0 || p.W <= 0 || c.h <= 0 || c.w <= 0 || c.h > p.H || c.w > p.W)
    return hipErrorInvalidValue;
  for (int b = 0; b < p.B; ++b)
    if (c.y0[b] < 0 || c.x0[b] < 0 || int(c.y0[b]) + c.h > p.H || int(c.x0[b]) + c.w > p.W) return hipErrorInvalidValue;
  if (p.Cout < 1 || p.Cout > 4 || p.Cin < 1 || p.Cin > 4) return hipErrorInvalidValue;
  if (p.nsrcs && (p.nsrcs != p.B || !srcs_ok(p.srcs, p.nsrcs, p.B, 1))) return hipErrorInvalidValue;
  if (p.ndsts && (p.ndsts != p.B || !dsts_ok(p.dsts, p.ndsts, p.B, 1))) return hipErrorInvalidValue;
  for (int k = 0; k < p.Cout; ++k)
    if (p.cmap[k] < 0 || p.cmap[k] >= p.Cin) return hipErrorInvalidValue;
  if (p.B == 0) return hipSuccess;
  return with_out_dtype(p.out_dtype, [&](auto o) { return launch_crop_out<o()>(p, c, stream); });
}

// ---- resized crop (kernels.h: decode_resize) -------------------------------
// The value path of decode() per tap, then a bilinear blend in which every
// fp32 operation is rounded on its own.  A block owns a band of R output rows
// of one image: it stages the window span of the source rows the band's taps
// touch as raw bytes into LDS (the table is applied per tap: raw rows are
// Cin bytes a pixel, so a 4096-pixel RGBA row fits twice; decoded fp32 rows of
// Cout floats a pixel would not), and after one barrier every lane produces
// PPT consecutive output pixels of one output row from LDS only.
namespace {

constexpr int kResizeRows = 56 * 1024;   // bytes of staged rows beside the 8-KiB value table: 64 KiB a block
constexpr int kResizeBand = 8;           // output rows per band (lowered for wide windows)

struct Axis {
  int i0, i1;
  float l0, l1;
};

// source taps and weights of output index d (kernels.h: decode_resize)
__device__ __forceinline__ Axis resize_axis(int d, float scale, int n_in) {
#pragma clang fp contract(off)
  float s = (float(d) + 0.5f) * scale - 0.5f;
  s = fmaxf(s, 0.0f);
  Axis a;
  a.i0 = min(int(s), n_in - 1);   // s >= 0: the conversion's truncation is floor
  a.i1 = min(a.i0 + 1, n_in - 1);
  a.l1 = s - float(a.i0);
  a.l0 = 1.0f - a.l1;
  return a;
}

__device__ __forceinline__ float resize_blend(float a, float b, float l0, float l1) {
#pragma clang fp contract(off)
  const float x = a * l0, y = b * l1;
  return x + y;
}

// values of output channel c for N input bytes: lookup_static's value path
template <int N>
__device__ __forceinline__ void resize_values(const Xf& xf, int c, const uint32_t (&v)[N], float (&o)[N]) {
  if (!xf.arith) {
    const float* l = xf.lut + c * 256;
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = l[v[i]];
    return;
  }
  float x[N];
  if (xf.gam[c]) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = float(xf.g[((v[i] >> 2) << xf.gshift) + (v[i] & 3)]);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = float(v[i]);
  }
  const float a = xf.a[c], b = xf.b[c], d = xf.d[c], r = xf.r[c];
  if (xf.op[c] == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = __builtin_fmaf(x[i], a, b);
  } else if (xf.op[c] == 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = xf_mulsub(x[i], a, b);
  } else if (xf.op[c] == 3) {
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = xf_recip_div(xf_mulsub(x[i], a, b), d, r);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = xf_mulsub(x[i], a, b) / d;
  }
}

template <int OUTT>
__device__ __forceinline__ auto resize_cvt(float v) {
  if constexpr (OUTT == OUT_F32) return v;
  else if constexpr (OUTT == OUT_BF16) return f2bf(v);
  else if constexpr (OUTT == OUT_F16) return f2h(v);
  else return uint8_t(fminf(fmaxf(__builtin_rintf(v), 0.0f), 255.0f));   // v_rndne: ties to even
}

// N values to N contiguous elements at the 16-byte aligned d (N * sizeof(element) a multiple of 16)
template <int OUTT, int N>
__device__ __forceinline__ void resize_store_run(void* d, const float (&v)[N]) {
  if constexpr (OUTT == OUT_F32) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      reinterpret_cast<float4*>(d)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else if constexpr (OUTT == OUT_U8) {
    uint32_t o[N / 4];   // packed in registers
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      o[i] = uint32_t(resize_cvt<OUTT>(v[4 * i])) | uint32_t(resize_cvt<OUTT>(v[4 * i + 1])) << 8 |
             uint32_t(resize_cvt<OUTT>(v[4 * i + 2])) << 16 | uint32_t(resize_cvt<OUTT>(v[4 * i + 3])) << 24;
#pragma unroll
    for (int i = 0; i < N / 16; ++i)
      reinterpret_cast<uint4*>(d)[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
  } else {
    uint32_t o[N / 2];
#pragma unroll
    for (int i = 0; i < N / 2; ++i)
      o[i] = uint32_t(resize_cvt<OUTT>(v[2 * i])) | uint32_t(resize_cvt<OUTT>(v[2 * i + 1])) << 16;
#pragma unroll
    for (int i = 0; i < N / 8; ++i)
      reinterpret_cast<uint4*>(d)[i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
  }
}

// emit's stores for values already computed: v[c][u] of PPT pixels from pixel q of image b
template <int PPT, int OUTT, int COUT>
__device__ __forceinline__ void resize_store_nhwc(const DecodeParams& p, int b, int64_t hw, int64_t q,
                                                  const float (&v)[4][PPT]) {
  constexpr int64_t ELEM = OUTT == OUT_F32 ? 4 : (OUTT == OUT_U8 ? 1 : 2);
  float o[PPT * COUT];
#pragma unroll
  for (int u = 0; u < PPT; ++u)
#pragma unroll
    for (int c = 0; c < COUT; ++c) o[u * COUT + c] = v[c][u];
  resize_store_run<OUTT, PPT * COUT>(image_out<uint8_t>(p, b, hw * COUT * ELEM) + q * COUT * ELEM, o);
}

template <int PPT, int OUTT, int LAYOUT>
__device__ __forceinline__ void resize_store(const DecodeParams& p, int b, int64_t hw, int cout, int64_t q,
                                             const float (&v)[4][PPT]) {
  constexpr int64_t ELEM = OUTT == OUT_F32 ? 4 : (OUTT == OUT_U8 ? 1 : 2);
  if constexpr (LAYOUT == NCHW) {
    uint8_t* img = image_out<uint8_t>(p, b, hw * cout * ELEM);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= cout) break;
      resize_store_run<OUTT, PPT>(img + (int64_t(c) * hw + q) * ELEM, v[c]);
    }
  } else {
    switch (cout) {
      case 1: resize_store_nhwc<PPT, OUTT, 1>(p, b, hw, q, v); break;
      case 2: resize_store_nhwc<PPT, OUTT, 2>(p, b, hw, q, v); break;
      case 3: resize_store_nhwc<PPT, OUTT, 3>(p, b, hw, q, v); break;
      default: resize_store_nhwc<PPT, OUTT, 4>(p, b, hw, q, v); break;
    }
  }
}

// Bytes of one staged row: LDS byte o of a row is the byte at (row address &
// ~15) + o, so 16-byte loads stay aligned on both sides; the span starts at
// most 15 bytes in and its last dword ends at most 3 bytes behind it.
inline int resize_row_stride(int wmax, int cin) { return (wmax * cin + 15 + 3 + 15) / 16 * 16; }

template <int PPT, int CIN, int OUTT, int LAYOUT>
__global__ __launch_bounds__(kBlock) void decode_resize_kernel(DecodeParams p, ResizeParams r, int R, int stride) {
  __shared__ uint32_t tab[kTabWords];
  extern __shared__ uint4 resize_rows[];   // 2R rows of `stride` bytes
  const Xf xf = stage_xf(p.lut, tab, p.Cout);   // (the staging barrier below covers the table as well)
  uint8_t* rows = reinterpret_cast<uint8_t*>(resize_rows);

  const int64_t HW = int64_t(p.H) * p.W;       // source frame
  const int64_t ohw = int64_t(r.oh) * r.ow;    // output image
  const int bands = (r.oh + R - 1) / R;
  const int total = bands * p.B;
  const int gpr = r.ow / PPT;                  // lane groups per output row
  const int upr = stride >> 4;                 // 16-byte units per staged row
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cm[k] = p.cmap[k];

  for (int item = blockIdx.x; item < total; item += gridDim.x) {
    const int b = item / bands;
    const int i_lo = (item - b * bands) * R;
    const int nb = min(R, r.oh - i_lo);
    const int y0 = r.y0[b], x0 = r.x0[b], h = r.h[b], w = r.w[b];
    const float sy = r.sy[b], sx = r.sx[b];
    const bool flip = image_flipped(p, b);
    const bool mirror = (r.mirror_bits >> b) & 1;
    const uint8_t* img = p.nsrcs ? p.srcs[b] : p.src + (p.src_offsets ? p.src_offsets[b] : int64_t(b) * HW * CIN);
    // first byte of window row ry's span (flip applied)
    auto row_addr = [&](int ry) {
      const int y = y0 + ry;
      return img + (int64_t(flip ? p.H - 1 - y : y) * p.W + x0) * CIN;
    };
    // The window rows the band's taps touch lie in [ymin, ymax].  Up to 2R of
    // them: staged as that run, row ry in slot ry - ymin (adjacent output
    // rows share taps).  More (the vertical scale exceeds 2, so no two output
    // rows share a tap): output row i_lo + n stages just its two taps, in
    // slots 2n and 2n + 1, and the rows between are never read.
    const int ymin = resize_axis(i_lo, sy, h).i0;
    const int run = resize_axis(i_lo + nb - 1, sy, h).i1 - ymin + 1;
    const bool contig = run <= 2 * R;
    const int nrows = contig ? run : 2 * nb;

    // Stage: unit e is 16-byte unit q of slot k.  Of a row only the dwords
    // that hold a byte of its span are read -- CIN == 4: the span itself;
    // CIN == 3: the span is only byte aligned, and the argument of
    // load_window_pixels holds: the dword of the first byte and the dword of
    // the last byte each hold a byte of the span, and as the frame's
    // H * W * 3 bytes (W % 4 == 0) start on a 16-byte boundary and end on a
    // dword boundary, neither reaches outside [frame, frame + H * W * CIN).
    // Four units' loads are issued before the first LDS store.
    const int units = nrows * upr;
    // unit e: a 16-byte unit inside the span's dwords is loaded into v (its LDS
    // byte offset returned), one on the span's edge copied dword by dword
    auto stage_unit = [&](int e, uint4& v) -> int {
      if (e >= units) return -1;
      const int k = e / upr, qb = (e - k * upr) * 16;
      int ry = ymin + k;
      if (!contig) {
        const Axis a = resize_axis(i_lo + (k >> 1), sy, h);
        ry = (k & 1) ? a.i1 : a.i0;
      }
      const uint8_t* ra = row_addr(ry);
      const int ph = int(reinterpret_cast<uintptr_t>(ra) & 15u);
      const uint8_t* base = ra - ph;
      const int lo = ph & ~3, hi = (ph + w * CIN + 3) & ~3;
      if (qb >= lo && qb + 16 <= hi) {
        v = *reinterpret_cast<const uint4*>(base + qb);
        return k * stride + qb;
      }
#pragma unroll
      for (int d = 0; d < 16; d += 4)
        if (qb + d >= lo && qb + d < hi)
          *reinterpret_cast<uint32_t*>(rows + k * stride + qb + d) = *reinterpret_cast<const uint32_t*>(base + qb + d);
      return -1;
    };
    for (int e0 = threadIdx.x; e0 < units; e0 += 4 * kBlock) {
      uint4 v0, v1, v2, v3;
      const int a0 = stage_unit(e0, v0), a1 = stage_unit(e0 + kBlock, v1);
      const int a2 = stage_unit(e0 + 2 * kBlock, v2), a3 = stage_unit(e0 + 3 * kBlock, v3);
      if (a0 >= 0) *reinterpret_cast<uint4*>(rows + a0) = v0;
      if (a1 >= 0) *reinterpret_cast<uint4*>(rows + a1) = v1;
      if (a2 >= 0) *reinterpret_cast<uint4*>(rows + a2) = v2;
      if (a3 >= 0) *reinterpret_cast<uint4*>(rows + a3) = v3;
    }
    __syncthreads();

    const int groups = nb * gpr;
    for (int g = threadIdx.x; g < groups; g += kBlock) {
      const int li = g / gpr, j = (g - li * gpr) * PPT;
      const int i = i_lo + li;
      const Axis ay = resize_axis(i, sy, h);
      const int k0 = contig ? ay.i0 - ymin : 2 * li, k1 = contig ? ay.i1 - ymin : 2 * li + 1;
      const uint8_t* t0 = rows + k0 * stride + (reinterpret_cast<uintptr_t>(row_addr(ay.i0)) & 15u);
      const uint8_t* t1 = rows + k1 * stride + (reinterpret_cast<uintptr_t>(row_addr(ay.i1)) & 15u);
      int o0[PPT], o1[PPT];
      float lx0[PPT], lx1[PPT];
#pragma unroll
      for (int u = 0; u < PPT; ++u) {
        const Axis ax = resize_axis(mirror ? r.ow - 1 - (j + u) : j + u, sx, w);
        o0[u] = ax.i0 * CIN, o1[u] = ax.i1 * CIN, lx0[u] = ax.l0, lx1[u] = ax.l1;
      }
      float v[4][PPT];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < cout) {
          // the pixels' four taps of this channel: bytes, then values (the
          // table's branches are taken once per channel, as in lookup_static)
          const int ic = cm[c];
          uint32_t tb[4 * PPT];
#pragma unroll
          for (int u = 0; u < PPT; ++u)
            tb[4 * u] = t0[o0[u] + ic], tb[4 * u + 1] = t0[o1[u] + ic], tb[4 * u + 2] = t1[o0[u] + ic],
                   tb[4 * u + 3] = t1[o1[u] + ic];
          float tv[4 * PPT];
          resize_values<4 * PPT>(xf, c, tb, tv);
#pragma unroll
          for (int u = 0; u < PPT; ++u)
            v[c][u] = resize_blend(resize_blend(tv[4 * u], tv[4 * u + 1], lx0[u], lx1[u]),
                                   resize_blend(tv[4 * u + 2], tv[4 * u + 3], lx0[u], lx1[u]), ay.l0, ay.l1);
        } else {
#pragma unroll
          for (int u = 0; u < PPT; ++u) v[c][u] = 0.f;
        }
      }
      resize_store<PPT, OUTT, LAYOUT>(p, b, ohw, cout, int64_t(i) * r.ow + j, v);
    }
    __syncthreads();   // the next band of this block restages the rows
  }
}

// Fallback: one output pixel per thread, its four taps read from the frame
// (any size, any alignment, any Cin).
template <int OUTT>
__global__ __launch_bounds__(kBlock) void decode_resize_scalar_kernel(DecodeParams p, ResizeParams r) {
  __shared__ uint32_t tab[kTabWords];
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  __syncthreads();
  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t ohw = int64_t(r.oh) * r.ow;
  const int64_t total = ohw * p.B;
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total; g += int64_t(gridDim.x) * kBlock) {
    const int b = int(g / ohw);
    const int64_t q = g - int64_t(b) * ohw;
    const int i = int(q / r.ow), j = int(q - int64_t(i) * r.ow);
    const Axis ay = resize_axis(i, r.sy[b], r.h[b]);
    const Axis ax = resize_axis(((r.mirror_bits >> b) & 1) ? r.ow - 1 - j : j, r.sx[b], r.w[b]);
    const bool flip = image_flipped(p, b);
    const int ya = int(r.y0[b]) + ay.i0, yb = int(r.y0[b]) + ay.i1;
    const uint8_t* img = p.nsrcs ? p.srcs[b] : p.src + (p.src_offsets ? p.src_offsets[b] : int64_t(b) * HW * p.Cin);
    const uint8_t* t0 = img + (int64_t(flip ? p.H - 1 - ya : ya) * p.W + r.x0[b]) * p.Cin;
    const uint8_t* t1 = img + (int64_t(flip ? p.H - 1 - yb : yb) * p.W + r.x0[b]) * p.Cin;
    const int o0 = ax.i0 * p.Cin, o1 = ax.i1 * p.Cin;
    for (int k = 0; k < p.Cout; ++k) {
      const int ic = p.cmap[k];
      const float top = resize_blend(xf_value(xf, k, t0[o0 + ic]), xf_value(xf, k, t0[o1 + ic]), ax.l0, ax.l1);
      const float bot = resize_blend(xf_value(xf, k, t1[o0 + ic]), xf_value(xf, k, t1[o1 + ic]), ax.l0, ax.l1);
      const float v = resize_blend(top, bot, ay.l0, ay.l1);
      const int64_t off = p.layout == NCHW ? int64_t(k) * ohw + q : q * p.Cout + k;   // within image b
      const int64_t ie = ohw * p.Cout;
      if constexpr (OUTT == OUT_F32) image_out<float>(p, b, ie)[off] = v;
      else if constexpr (OUTT == OUT_U8) image_out<uint8_t>(p, b, ie)[off] = resize_cvt<OUTT>(v);
      else image_out<uint16_t>(p, b, ie)[off] = resize_cvt<OUTT>(v);
    }
  }
}

template <int PPT, int CIN, int OUTT>
void launch_resize_vec(const DecodeParams& p, const ResizeParams& r, int R, int stride, hipStream_t s) {
  const int items = p.B * ((r.oh + R - 1) / R);
  const int cap = p.max_grid > 0 ? p.max_grid : 2048;
  const int grid = items < cap ? items : cap;
  const size_t lds = size_t(2) * R * stride;
  if (p.layout == NCHW)
    decode_resize_kernel<PPT, CIN, OUTT, NCHW><<<grid, kBlock, lds, s>>>(p, r, R, stride);
  else
    decode_resize_kernel<PPT, CIN, OUTT, NHWC><<<grid, kBlock, lds, s>>>(p, r, R, stride);
}

template <int OUTT>
hipError_t launch_resize_out(const DecodeParams& p, const ResizeParams& r, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  constexpr int64_t ELEM = elem_for(OUTT);
  // staged path: decode_crop's conditions on the sources (16-byte aligned
  // frames; packed RGB rows a whole number of dwords) and on the stores
  const bool src_aligned = p.nsrcs ? srcs_ok(p.srcs, p.nsrcs, p.B, 16)
                                   : (reinterpret_cast<uintptr_t>(p.src) % 16) == 0 &&
                                         (p.src_offsets ? p.src_offsets_aligned != 0
                                                        : (int64_t(p.H) * p.W * p.Cin) % 16 == 0);
  const bool dst_aligned = p.ndsts ? dsts_ok(p.dsts, p.ndsts, p.B, 16) : (reinterpret_cast<uintptr_t>(p.dst) % 16) == 0;
  const bool vec = (r.ow % PPT) == 0 && src_aligned && dst_aligned && (int64_t(r.oh) * r.ow * p.Cout * ELEM) % 16 == 0 &&
                   (p.Cin == 4 || (p.Cin == 3 && (p.W % 4) == 0));
  if (!vec) {
    const int64_t work = int64_t(p.B) * r.oh * r.ow;
    decode_resize_scalar_kernel<OUTT><<<grid_for(work, p.max_grid), kBlock, 0, s>>>(p, r);
    return hipGetLastError();
  }
  int wmax = 1;
  for (int b = 0; b < p.B; ++b) wmax = r.w[b] > wmax ? r.w[b] : wmax;
  const int stride = resize_row_stride(wmax, p.Cin);
  int R = kResizeBand;
  while (R > 1 && 2 * R * stride > kResizeRows) R >>= 1;
  if (2 * R * stride > kResizeRows) return hipErrorInvalidValue;   // a window row too wide to stage twice
  if (p.Cin == 4)
    launch_resize_vec<PPT, 4, OUTT>(p, r, R, stride, s);
  else
    launch_resize_vec<PPT, 3, OUTT>(p, r, R, stride, s);
  return hipGetLastError();
}

}  // namespace

hipError_t decode_resize(const DecodeParams& p, const ResizeParams& r, hipStream_t stream) {
  // every condition is checked here and in launch_resize_out, before anything is launched
  if (p.B < 0 || p.B > kMaxSrcs || p.H <= 0 || p.W <= 0 || r.oh < 1 || r.ow < 1 || r.oh > INT16_MAX || r.ow > INT16_MAX)
    return hipErrorInvalidValue;
  for (int b = 0; b < p.B; ++b)
    if (r.y0[b] < 0 || r.x0[b] < 0 || r.h[b] < 1 || r.w[b] < 1 || int(r.y0[b]) + r.h[b] > p.H ||
        int(r.x0[b]) + r.w[b] > p.W)
      return hipErrorInvalidValue;
  if (p.Cout < 1 || p.Cout > 4 || p.Cin < 1 || p.Cin > 4) return hipErrorInvalidValue;
  if (p.nsrcs && (p.nsrcs != p.B || !srcs_ok(p.srcs, p.nsrcs, p.B, 1))) return hipErrorInvalidValue;
  if (p.ndsts && (p.ndsts != p.B || !dsts_ok(p.dsts, p.ndsts, p.B, 1))) return hipErrorInvalidValue;
  for (int k = 0; k < p.Cout; ++k)
    if (p.cmap[k] < 0 || p.cmap[k] >= p.Cin) return hipErrorInvalidValue;
  if (p.B == 0) return hipSuccess;
  return with_out_dtype(p.out_dtype, [&](auto o) { return launch_resize_out<o()>(p, r, stream); });
}

namespace {

template <int OUTT, typename Test>
hipError_t launch_mirror_out(const DecodeParams& p, const typename Test::Args& d, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  const int grid = grid_for(int64_t(p.B) * p.H * p.W / PPT, p.max_grid);
  if (p.Cin == 4) {
    if (p.layout == NCHW) decode_mirror_kernel<PPT, 4, OUTT, NCHW, Test><<<grid, kBlock, 0, s>>>(p, d);
    else decode_mirror_kernel<PPT, 4, OUTT, NHWC, Test><<<grid, kBlock, 0, s>>>(p, d);
  } else {
    if (p.layout == NCHW) decode_mirror_kernel<PPT, 3, OUTT, NCHW, Test><<<grid, kBlock, 0, s>>>(p, d);
    else decode_mirror_kernel<PPT, 3, OUTT, NHWC, Test><<<grid, kBlock, 0, s>>>(p, d);
  }
  return hipGetLastError();
}

template <typename Test>
hipError_t launch_mirror(const DecodeParams& p, const typename Test::Args& d, hipStream_t s) {
  return with_out_dtype(p.out_dtype, [&](auto o) { return launch_mirror_out<o(), Test>(p, d, s); });
}

// what both mirror reads ask beyond decode_delta_supported(): a dense output
// whose images are 16-byte multiples, and 16-byte aligned mirrors
bool mirror_buffers_ok(const DecodeParams& p, uint8_t* const* mirror) {
  if (!p.ndsts && (size_t(p.H) * p.W * p.Cout * size_t(elem_for(p.out_dtype))) % 16 != 0) return false;
  for (int b = 0; b < p.B; ++b)
    if ((reinterpret_cast<uintptr_t>(mirror[b]) % 16) != 0) return false;
  return true;
}

}  // namespace

bool decode_delta_supported(const DecodeParams& p) {
  if (p.B < 1 || p.B > kMaxSrcs || p.nsrcs != p.B || p.H <= 0 || p.W <= 0 || p.H > INT16_MAX || p.W > INT16_MAX)
    return false;
  if ((p.Cin != 3 && p.Cin != 4) || p.Cout < 1 || p.Cout > 4) return false;
  if (p.out_dtype < OUT_F32 || p.out_dtype > OUT_U8 || (p.layout != NCHW && p.layout != NHWC)) return false;
  for (int c = 0; c < p.Cout; ++c)
    if (p.cmap[c] < 0 || p.cmap[c] >= p.Cin) return false;
  if (p.W % ppt_for(p.out_dtype) != 0 || (int64_t(p.H) * p.W * p.Cin) % 16 != 0) return false;
  if (!srcs_ok(p.srcs, p.nsrcs, p.B, 16)) return false;
  return p.ndsts ? dsts_ok(p.dsts, p.ndsts, p.B, 16) : p.dst != nullptr && (reinterpret_cast<uintptr_t>(p.dst) % 16) == 0;
}

hipError_t decode_delta(const DecodeParams& p, const DeltaParams& d, hipStream_t stream) {
  // every condition is checked here, before anything is launched
  if (p.B == 0) return hipSuccess;
  if (!decode_delta_supported(p) || !mirror_buffers_ok(p, d.mirror)) return hipErrorInvalidValue;
  for (int b = 0; b < p.B; ++b) {
    if (!d.mirror[b]) continue;
    const int y0 = d.y0[b], y1 = d.y1[b], x0 = d.x0[b], x1 = d.x1[b];
    if (y1 < y0) continue;   // nothing from the host
    if (y0 < 0 || y1 >= p.H || x0 < 0 || x1 < x0 || x1 >= p.W) return hipErrorInvalidValue;
    const bool full_rows = x0 == 0 && x1 == p.W - 1;
    const bool blocks = x0 % 64 == 0 && ((x1 + 1) % 64 == 0 || x1 == p.W - 1) && p.W % 64 == 0;
    if (!full_rows && !blocks) return hipErrorInvalidValue;
  }
  return launch_mirror<RectTest>(p, d, stream);
}

bool decode_delta_blocks_supported(const DecodeParams& p) {
  return p.B <= kMaxBlockImgs && p.W % 64 == 0 && p.W <= 1024 && decode_delta_supported(p);
}

hipError_t decode_delta_blocks(const DecodeParams& p, const BlockParams& d, hipStream_t stream) {
  // every condition is checked here, before anything is launched
  if (p.B == 0) return hipSuccess;
  if (!decode_delta_blocks_supported(p) || !mirror_buffers_ok(p, d.mirror)) return hipErrorInvalidValue;
  BlockArgs a = {};
  const unsigned cols = (2u << unsigned((p.W - 1) / 64)) - 1u;
  const int br = d.band_rows;
  if (br <= 0 || (br & (br - 1)) != 0) return hipErrorInvalidValue;
  const int nb = (p.H + br - 1) / br;
  if (nb > kMaxBlockBands) return hipErrorInvalidValue;   // (so every row's band index stays inside a mask row)
  while ((1 << a.band_log2) < br) ++a.band_log2;
  for (int b = 0; b < p.B; ++b) {
    a.mirror[b] = d.mirror[b];
    if (!d.mirror[b]) continue;
    for (int k = 0; k < kMaxBlockBands; ++k) {
      const unsigned w = d.mask[b][k];
      if (k >= nb ? w != 0 : (w & ~cols) != 0) return hipErrorInvalidValue;   // a bit outside the frame
      a.rows[b][k] = uint16_t(w);
    }
  }
  return launch_mirror<BlockTest>(p, a, stream);
}

hipError_t decode_tiles(const DecodeParams& p, const TileParams& t, hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  const int ppt = ppt_for(p.out_dtype);
  const size_t elem = elem_for(p.out_dtype);
  if (p.B > kMaxSrcs || p.nsrcs != p.B || p.H % 16 != 0 || p.W % 16 != 0 || (p.Cin != 3 && p.Cin != 4) ||
      p.Cout < 1 || p.Cout > 4 || p.W % ppt != 0 || t.payload_off % 16 != 0 || t.out_img_bytes % 16 != 0 ||
      t.out_img_bytes != int64_t(p.H) * p.W * p.Cout * int64_t(elem) || !srcs_ok(p.srcs, p.nsrcs, p.B, 16) ||
      (p.ndsts ? !dsts_ok(p.dsts, p.ndsts, p.B, 16) : (reinterpret_cast<uintptr_t>(p.dst) % 16) != 0) ||
      t.tile_start[0] != 0)
    return hipErrorInvalidValue;
  const int64_t ntiles = int64_t(p.H / 16) * (p.W / 16);
  for (int b = 0; b < p.B; ++b)
    if (!t.fills[b] || (reinterpret_cast<uintptr_t>(t.fills[b]) % 16) != 0 || t.tile_start[b + 1] < t.tile_start[b] ||
        t.tile_start[b + 1] - t.tile_start[b] > ntiles)
      return hipErrorInvalidValue;
  for (int c = 0; c < p.Cout; ++c)
    if (p.cmap[c] < 0 || p.cmap[c] >= p.Cin) return hipErrorInvalidValue;
  const int64_t chunks = t.out_img_bytes / 16 * p.B;
  tile_fill_kernel<<<grid_for(chunks, 0), kBlock, 0, stream>>>(p, t);
  return with_out_dtype(p.out_dtype, [&](auto o) {
    launch_tiles_out<o()>(p, t, stream);
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------------------
// fused replay sample: Philox index draw + gather + decode + metadata gather
// ---------------------------------------------------------------------------
namespace {

// Philox4x32-10 (Salmon et al., SC'11), first output word.
__device__ __forceinline__ uint32_t philox_word(uint64_t seed, uint64_t ctr, uint32_t b) {
  uint32_t c0 = b, c1 = uint32_t(ctr), c2 = uint32_t(ctr >> 32), c3 = 0;
  uint32_t k0 = uint32_t(seed), k1 = uint32_t(seed >> 32);
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
  return c0;
}

// Block prologue shared by both replay kernels: the table, this launch's B
// frame indices (drawn or given) in LDS, and the counter hand-over.
template <int TW>
struct ReplaySharedT {
  uint32_t tab[TW];
  uint32_t idx[kMaxReplayB];   // frame indices (< 2^32: replay_sample checks the count)
  uint64_t ctr;
};
using ReplayShared = ReplaySharedT<kTabWords>;

__device__ Xf replay_prologue(const DecodeParams& p, const ReplayParams& r, ReplayShared& sh) {
  const Xf xf = stage_xf(p.lut, sh.tab, p.Cout);
  if (threadIdx.x == 0) sh.ctr = r.index_in ? 0 : (r.counter ? r.counter[0] : r.ctr_value);
  __syncthreads();
  for (int b = threadIdx.x; b < p.B; b += kBlock) {
    const int64_t i = r.index_in ? r.index_in[b]
                                 : int64_t((uint64_t(philox_word(r.seed, sh.ctr, uint32_t(b))) * uint64_t(r.count)) >> 32);
    sh.idx[b] = i;
    if (blockIdx.x == 0 && r.index_out) r.index_out[b] = i;
  }
  __syncthreads();
  return xf;
}

// The counter moves on in a one-lane kernel queued right behind the sample:
// every block of the sample reads it, so no block may advance it in-kernel
// without a grid-wide handshake -- and a per-block atomic (or fence) on one
// address serialises thousands of blocks (measured 68 -> 517 us).
__global__ void replay_advance_kernel(uint64_t* counter, int B) { counter[0] += uint64_t(B); }

// metadata unit m of the launch: 4-byte words of 4-byte-multiple columns,
// single bytes otherwise
template <class Shared>
__device__ __forceinline__ void replay_meta(const ReplayParams& r, const Shared& sh, int B, int64_t m) {
  for (int k = 0; k < r.nmeta; ++k) {
    const int nb = r.meta_bytes[k];
    const int w = (nb % 4 == 0) ? 4 : 1;
    const int64_t per = nb / w, units = per * B;
    if (m < units) {
      const int b = int(m / per);
      const int64_t j = (m - int64_t(b) * per) * w;
      const uint8_t* s = r.meta_src[k] + int64_t(sh.idx[b]) * nb + j;
      uint8_t* d = r.meta_dst[k] + int64_t(b) * nb + j;
      if (w == 4) *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
      else *d = *s;
      return;
    }
    m -= units;
  }
}

// TBL: the value table is in table mode (p.xf_table_only): the lookups are
// plain LDS reads and the kernel carries none of the arithmetic-form code
// (whose registers cut the general kernel to 4 waves per SIMD).  TBL 2: every
// output channel has the same table (xf_table_only 2) -- staged as 32 copies
// interleaved by word, [value][copy], and lane l reads copy l % 32: the 32
// lanes of a ds_read group always hit 32 distinct banks (one 1 KiB table read
// at random bytes ran ~3.4-way conflicted)
constexpr int kUniWords = 256 * 32;
constexpr int kUniU = 4;   // groups in flight per lane (TBL 2)
template <int PPT, int CIN, int OUTT, int LAYOUT, int TBL, bool NT = false>
__global__ __launch_bounds__(kBlock) void replay_vec_kernel(DecodeParams p, ReplayParams r, int64_t meta_units) {
  __shared__ ReplaySharedT<TBL == 2 ? kUniWords : kTabWords> sh;
  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t groups_per_img = HW / PPT;
  const int64_t groups = groups_per_img * p.B;
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) cm[c] = p.cmap[c];
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const bool small = groups + meta_units + stride < (int64_t(1) << 31);
  // Every lane draws the frame index of its own first group (the same Philox
  // word the block's table holds) and issues that group's pixel loads before
  // the LUT staging and the block barrier: the HBM latency of the first
  // loads overlaps the prologue instead of following it (one launch round
  // for a batch of 8).
  const uint64_t ctr = r.index_in ? 0 : (r.counter ? r.counter[0] : r.ctr_value);
  auto frame_of = [&](int b) -> int64_t {
    return r.index_in ? r.index_in[b]
                      : int64_t((uint64_t(philox_word(r.seed, ctr, uint32_t(b))) * uint64_t(r.count)) >> 32);
  };
  const int64_t g0 = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  Group gr0;
  Pixels<PPT, CIN> px0;
  // TBL 2 runs a grid of few blocks (the table staging is per block): each
  // lane keeps kUniU groups' loads in flight per pass
  Group gru[kUniU];
  Pixels<PPT, CIN> pxu[kUniU];
#define BT_UNI_ISSUE(GB, FIRST)                                                                   \
  _Pragma("unroll") for (int u = 0; u < kUniU; ++u) {                                             \
    const int64_t g_ = (GB) + u * stride;                                                         \
    int y_ = 0, x_ = 0;                                                                           \
    split_group<PPT>(g_ < groups ? g_ : 0, groups_per_img, p.W, small, gru[u].b, gru[u].q, y_, x_); \
    const int sy_ = p.flip_all ? p.H - 1 - y_ : y_;                                               \
    const int64_t fi_ = (FIRST) ? frame_of(gru[u].b) : int64_t(sh.idx[gru[u].b]);                \
    gru[u].src = p.src + fi_ * r.frame_bytes + (int64_t(sy_) * p.W + x_) * CIN;                   \
    load_pixels<PPT, CIN>(gru[u].src, pxu[u]);                                                    \
  }
  // (a group past the end re-reads group 0 and is not emitted: no branch around the loads)
  if constexpr (TBL == 2) {
    BT_UNI_ISSUE(g0, true)
  } else if (g0 < groups) {
    int y, x;
    split_group<PPT>(g0, groups_per_img, p.W, small, gr0.b, gr0.q, y, x);
    const int sy = p.flip_all ? p.H - 1 - y : y;
    gr0.src = p.src + frame_of(gr0.b) * r.frame_bytes + (int64_t(sy) * p.W + x) * CIN;
    load_pixels<PPT, CIN>(gr0.src, px0);
  }
  Xf xf;
  if constexpr (TBL == 2) {
    // header scalars as stage_xf reads them; the table expanded into its 32
    // copies (word w = 32 value + copy: consecutive lanes, consecutive words)
    xf.arith = 0;
    float v[kUniWords / kBlock];
#pragma unroll
    for (int i = 0; i < kUniWords / kBlock; ++i) v[i] = p.lut[(int(threadIdx.x) + kBlock * i) >> 5];
#pragma unroll
    for (int i = 0; i < kUniWords / kBlock; ++i) sh.tab[int(threadIdx.x) + kBlock * i] = __float_as_uint(v[i]);
    xf.lut = reinterpret_cast<const float*>(sh.tab) + (threadIdx.x & 31);
  } else {
    xf = stage_xf(p.lut, sh.tab, p.Cout);
  }
  for (int b = threadIdx.x; b < p.B; b += kBlock) {
    const int64_t i = frame_of(b);
    sh.idx[b] = i;
    if (blockIdx.x == 0 && r.index_out) r.index_out[b] = i;
  }
  __syncthreads();
  if constexpr (TBL == 2) {
    for (int64_t gb = g0; gb < groups; gb += kUniU * stride) {
      if (gb != g0) {
        BT_UNI_ISSUE(gb, false)
      }
#pragma unroll
      for (int u = 0; u < kUniU; ++u)
        if (gb + u * stride < groups) emit<PPT, CIN, OUTT, LAYOUT, TBL, NT>(p, xf, cm, cout, HW, gru[u], pxu[u]);
    }
    for (int64_t g = g0; g < groups + meta_units; g += stride)
      if (g >= groups) replay_meta(r, sh, p.B, g - groups);
    return;
  }
#undef BT_UNI_ISSUE
  for (int64_t g = g0; g < groups + meta_units; g += stride) {
    if (g >= groups) {
      replay_meta(r, sh, p.B, g - groups);
      continue;
    }
    if (g == g0) {
      emit<PPT, CIN, OUTT, LAYOUT, TBL, NT>(p, xf, cm, cout, HW, gr0, px0);
      continue;
    }
    Group gr;
    int y, x;
    split_group<PPT>(g, groups_per_img, p.W, small, gr.b, gr.q, y, x);
    const int sy = p.flip_all ? p.H - 1 - y : y;
    gr.src = p.src + int64_t(sh.idx[gr.b]) * r.frame_bytes + (int64_t(sy) * p.W + x) * CIN;
    Pixels<PPT, CIN> px;
    load_pixels<PPT, CIN>(gr.src, px);
    emit<PPT, CIN, OUTT, LAYOUT, TBL, NT>(p, xf, cm, cout, HW, gr, px);
  }
}

// any shape / alignment: one pixel per lane
template <int OUTT>
__global__ __launch_bounds__(kBlock) void replay_scalar_kernel(DecodeParams p, ReplayParams r, int64_t meta_units) {
  __shared__ ReplayShared sh;
  const Xf xf = replay_prologue(p, r, sh);
  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t total = HW * p.B;
  const int64_t ie = HW * p.Cout;
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total + meta_units; g += int64_t(gridDim.x) * kBlock) {
    if (g >= total) {
      replay_meta(r, sh, p.B, g - total);
      continue;
    }
    const int b = int(g / HW);
    const int64_t q = g - int64_t(b) * HW;
    const int y = int(q / p.W), x = int(q - int64_t(y) * p.W);
    const int sy = p.flip_all ? p.H - 1 - y : y;
    const uint8_t* s = p.src + int64_t(sh.idx[b]) * r.frame_bytes + (int64_t(sy) * p.W + x) * p.Cin;
    for (int c = 0; c < p.Cout; ++c) {
      const float v = xf_value(xf, c, s[p.cmap[c]]);
      const int64_t off = p.layout == NCHW ? int64_t(c) * HW + q : q * p.Cout + c;
      if constexpr (OUTT == OUT_F32) reinterpret_cast<float*>(p.dst)[int64_t(b) * ie + off] = v;
      else if constexpr (OUTT == OUT_BF16) reinterpret_cast<uint16_t*>(p.dst)[int64_t(b) * ie + off] = f2bf(v);
      else if constexpr (OUTT == OUT_F16) reinterpret_cast<uint16_t*>(p.dst)[int64_t(b) * ie + off] = f2h(v);
      else reinterpret_cast<uint8_t*>(p.dst)[int64_t(b) * ie + off] = uint8_t(v);
    }
  }
}

template <int OUTT>
hipError_t launch_replay(const DecodeParams& p, const ReplayParams& r, int64_t meta_units, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  const bool vec = (p.W % PPT) == 0 && r.frame_bytes % 16 == 0 && (p.Cin == 3 || p.Cin == 4) &&
                   (reinterpret_cast<uintptr_t>(p.src) % 16) == 0 && (reinterpret_cast<uintptr_t>(p.dst) % 16) == 0 &&
                   (int64_t(p.H) * p.W * p.Cin) % 16 == 0;
  if (vec) {
    int grid = grid_for(int64_t(p.B) * p.H * p.W / PPT + meta_units, p.max_grid);
    // fp32 NCHW table-mode output through non-temporal stores: batch 64 of
    // 640x480 58.5 us against 62.8 (profiles/r5/b6; BT_REPLAY_NT=0: plain stores)
    static const bool nt_env = !(std::getenv("BT_REPLAY_NT") && std::getenv("BT_REPLAY_NT")[0] == '0');
    const bool nt = nt_env && OUTT == OUT_F32 && p.layout == NCHW && p.xf_table_only;
    // one table for all channels (xf_table_only 2): the 32-copy conflict-free
    // form with BT_REPLAY_UNI=1 -- 0 % bank conflicts (PMC) but 83.4 us against
    // 58.4 per batch of 64 (profiles/r5/b8): its 32 KiB table per block halves
    // the resident waves and every one of the 8192 blocks stages it
    static const bool uni_env = std::getenv("BT_REPLAY_UNI") && std::getenv("BT_REPLAY_UNI")[0] == '1';
    const bool uni = uni_env && p.xf_table_only == 2;
    if (uni && p.max_grid <= 0) {   // 4 blocks per CU, the table staged once per block (BT_REPLAY_UNI_GRID)
      static const int ug = std::getenv("BT_REPLAY_UNI_GRID") ? std::atoi(std::getenv("BT_REPLAY_UNI_GRID")) : 1024;
      grid = std::min(grid, ug > 0 ? ug : 1024);
    }
#define BT_REPLAY(CIN, LAY)                                                                  \
  do {                                                                                       \
    if (uni && nt) replay_vec_kernel<PPT, CIN, OUTT, LAY, 2, true><<<grid, kBlock, 0, s>>>(p, r, meta_units); \
    else if (uni) replay_vec_kernel<PPT, CIN, OUTT, LAY, 2><<<grid, kBlock, 0, s>>>(p, r, meta_units); \
    else if (nt) replay_vec_kernel<PPT, CIN, OUTT, LAY, 1, true><<<grid, kBlock, 0, s>>>(p, r, meta_units); \
    else if (p.xf_table_only) replay_vec_kernel<PPT, CIN, OUTT, LAY, 1><<<grid, kBlock, 0, s>>>(p, r, meta_units); \
    else replay_vec_kernel<PPT, CIN, OUTT, LAY, 0><<<grid, kBlock, 0, s>>>(p, r, meta_units);               \
  } while (0)
    if (p.Cin == 4) {
      if (p.layout == NCHW) BT_REPLAY(4, NCHW);
      else BT_REPLAY(4, NHWC);
    } else {
      if (p.layout == NCHW) BT_REPLAY(3, NCHW);
      else BT_REPLAY(3, NHWC);
    }
#undef BT_REPLAY
  } else {
    replay_scalar_kernel<OUTT><<<grid_for(int64_t(p.B) * p.H * p.W + meta_units, p.max_grid), kBlock, 0, s>>>(
        p, r, meta_units);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t replay_sample(const DecodeParams& p, const ReplayParams& r, hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  if (p.B > kMaxReplayB || p.H <= 0 || p.W <= 0 || p.Cin < 1 || p.Cin > 4 || p.Cout < 1 || p.Cout > 4 || !p.src ||
      !p.dst || !p.lut || r.frame_bytes != int64_t(p.H) * p.W * p.Cin || r.nmeta < 0 || r.nmeta > kMaxMeta)
    return hipErrorInvalidValue;
  if (!r.index_in && (r.count < 1 || r.count > (int64_t(1) << 32))) return hipErrorInvalidValue;
  for (int c = 0; c < p.Cout; ++c)
    if (p.cmap[c] < 0 || p.cmap[c] >= p.Cin) return hipErrorInvalidValue;
  int64_t meta_units = 0;
  for (int k = 0; k < r.nmeta; ++k) {
    const int nb = r.meta_bytes[k];
    if (nb <= 0 || !r.meta_src[k] || !r.meta_dst[k]) return hipErrorInvalidValue;
    if (nb % 4 == 0 && ((reinterpret_cast<uintptr_t>(r.meta_src[k]) | reinterpret_cast<uintptr_t>(r.meta_dst[k])) % 4))
      return hipErrorInvalidValue;
    meta_units += int64_t(p.B) * (nb % 4 == 0 ? nb / 4 : nb);
  }
  const hipError_t e = with_out_dtype(p.out_dtype, [&](auto o) { return launch_replay<o()>(p, r, meta_units, stream); });
  if (e != hipSuccess || r.index_in || !r.counter) return e;
  replay_advance_kernel<<<1, 1, 0, stream>>>(r.counter, p.B);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// fused replay sample through crop windows (kernels.h: replay_sample_crop)
// ---------------------------------------------------------------------------
// replay_vec_kernel's prologue, value path, stores and metadata units with
// decode_crop_kernel's addressing: a lane owns PPT consecutive pixels of one
// WINDOW row.  The windows are drawn (or read) in the block prologue next to
// the frame indices and sit packed in LDS.  With a pad the window may leave
// the frame: the row is clamped (whole groups), and a group whose PPT source
// columns do not all lie in [0, W) reads its pixels one by one at the clamped
// columns -- only bytes of its own pixels, no over-read; every other group
// takes load_window_pixels and keeps its proof.
namespace {

// Philox4x32-10 with counter word 3 = c3: the four output words in the order
// philox_word leaves its state (philox_word is word 0 of the block c3 = 0)
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

// frame index and window per image: 8 KiB for kMaxReplayB images.  A window
// is packed as y0 + pad (15 bits), x0 + pad (15 bits), mirror (bit 31): both
// origins lie in [0, 32767] by the launch's limits.
struct ReplayCropShared {
  uint32_t tab[kTabWords];
  uint32_t idx[kMaxReplayB];
  uint32_t win[kMaxReplayB];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int64_t replay_frame(const ReplayParams& r, uint64_t ctr, int b) {
  return r.index_in ? r.index_in[b]
                    : int64_t((uint64_t(philox_word(r.seed, ctr, uint32_t(b))) * uint64_t(r.count)) >> 32);
}

// image b's window, packed.  Given windows are clamped into the legal range
// (the caller validated them; the clamp keeps every read inside the frame
// whatever the tensor holds).
// c3: the Philox block drawn from (1; the transitions' next stack takes 5).
__device__ __forceinline__ uint32_t replay_window(const DecodeParams& p, const ReplayCropParams& c, uint64_t ctr,
                                                  int b, uint32_t c3 = 1u) {
  int y0, x0, m = 0;
  if (c.windows_in) {
    y0 = clampi(c.windows_in[3 * b], -c.pad, p.H + c.pad - c.h);
    x0 = clampi(c.windows_in[3 * b + 1], -c.pad, p.W + c.pad - c.w);
    m = c.windows_in[3 * b + 2] != 0;
  } else if (c.mode == kCropFixed) {
    y0 = c.y0, x0 = c.x0;
  } else {
    uint32_t o[4];
    philox_block(c.window_key, ctr, uint32_t(b), c3, o);
    y0 = int(__umulhi(o[0], c.ny)) - c.pad;
    x0 = int(__umulhi(o[1], c.nx)) * c.x_align - c.pad;
    m = (o[2] >> 8) < c.mirror_threshold;
  }
  return uint32_t(y0 + c.pad) | (uint32_t(x0 + c.pad) << 15) | (uint32_t(m) << 31);
}

// fills sh.idx / sh.win (block 0 also index_out / crop_out); the caller syncs
__device__ __forceinline__ void replay_crop_table(const DecodeParams& p, const ReplayParams& r,
                                                  const ReplayCropParams& c, uint64_t ctr, ReplayCropShared& sh) {
  for (int b = threadIdx.x; b < p.B; b += kBlock) {
    const int64_t i = replay_frame(r, ctr, b);
    const uint32_t win = replay_window(p, c, ctr, b);
    sh.idx[b] = uint32_t(i);
    sh.win[b] = win;
    if (blockIdx.x == 0) {
      if (r.index_out) r.index_out[b] = i;
      if (c.crop_out) {
        c.crop_out[3 * b] = int(win & 0x7FFFu) - c.pad;
        c.crop_out[3 * b + 1] = int((win >> 15) & 0x7FFFu) - c.pad;
        c.crop_out[3 * b + 2] = int(win >> 31);
      }
    }
  }
}

// PPT pixels of one frame row at columns clamp(xs + k, 0, W - 1): one pixel at
// a time (a dword per RGBA pixel -- rows of a 16-byte aligned frame are dword
// multiples --, three bytes per RGB pixel), every index static once unrolled
template <int PPT, int CIN>
__device__ __forceinline__ void load_clamped_pixels(const uint8_t* row, int xs, int W, Pixels<PPT, CIN>& px) {
  constexpr int NW = Pixels<PPT, CIN>::NW;
  if constexpr (CIN == 4) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) px.w[k] = reinterpret_cast<const uint32_t*>(row)[clampi(xs + k, 0, W - 1)];
  } else {
    static_assert(CIN == 3, "packed RGB");
    uint32_t o[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) o[k] = 0;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const uint8_t* s = row + clampi(xs + i, 0, W - 1) * 3;
      const uint32_t v = uint32_t(s[0]) | (uint32_t(s[1]) << 8) | (uint32_t(s[2]) << 16);
      const int k = (3 * i) >> 2, sh = (3 * i) & 3;
      o[k] |= v << (8 * sh);
      if (sh >= 2) o[k + 1 < NW ? k + 1 : k] |= v >> (8 * (4 - sh));
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) px.w[k] = o[k];
  }
}

// The lane's PPT source pixels of window row i, window columns [j, j + PPT),
// in SOURCE order (the caller reverses them when the window is mirrored).
template <int PPT, int CIN>
__device__ __forceinline__ bool load_crop_group(const DecodeParams& p, const ReplayParams& r,
                                                const ReplayCropParams& c, int64_t frame, uint32_t win, int i, int j,
                                                Pixels<PPT, CIN>& px) {
  const int y0 = int(win & 0x7FFFu) - c.pad, x0 = int((win >> 15) & 0x7FFFu) - c.pad;
  const bool mirror = (win >> 31) != 0;
  const int y = clampi(y0 + i, 0, p.H - 1);
  const int sy = p.flip_all ? p.H - 1 - y : y;
  const int xs = x0 + (mirror ? c.w - PPT - j : j);
  const uint8_t* row = p.src + frame * r.frame_bytes + int64_t(sy) * p.W * CIN;
  if (xs >= 0 && xs + PPT <= p.W)
    load_window_pixels<PPT, CIN>(row + xs * CIN, px);
  else   // pad only: the group straddles (or lies beyond) a frame edge
    load_clamped_pixels<PPT, CIN>(row, xs, p.W, px);
  return mirror;
}

// The two choices replay_vec_kernel settled by measurement, measured again
// here (profiles/r12/replay_crop.md, 640x480 RGBA -> fp32 NCHW):
//   * no first-group load ahead of the table staging and the barrier: every
//     lane would run both Philox blocks of its first image itself, and the
//     variant was 1-7 % slower from a graph (batch 8, 448x448: 16.0 against
//     15.3 us; batch 64: 50.3 against 48.0 us) and 4 % slower eagerly at
//     batch 64 (43.3 against 41.7 us);
//   * NT: non-temporal stores for fp32 NCHW table-mode output, as in the
//     uncropped kernel: batch 64 of 448x448 41.7 us against 48.1 with plain
//     stores (eager), batch 8 from a graph 15.3 against 16.3; from a graph at
//     batch 64 plain stores were 2 % ahead (46.8 against 48.0).
template <int PPT, int CIN, int OUTT, int LAYOUT, int TBL, bool NT = false>
__global__ __launch_bounds__(kBlock) void replay_crop_vec_kernel(DecodeParams p, ReplayParams r, ReplayCropParams c,
                                                                 int64_t meta_units) {
  __shared__ ReplayCropShared sh;
  const int64_t hw = int64_t(c.h) * c.w;       // window = output image
  const int64_t groups_per_img = hw / PPT;
  const int64_t groups = groups_per_img * p.B;
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) cm[k] = p.cmap[k];
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const bool small = groups + meta_units + stride < (int64_t(1) << 31);
  // the windows need the counter even when the indices are given
  const uint64_t ctr = r.counter ? r.counter[0] : r.ctr_value;
  const Xf xf = stage_xf(p.lut, sh.tab, p.Cout);
  replay_crop_table(p, r, c, ctr, sh);
  __syncthreads();
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < groups + meta_units; g += stride) {
    if (g >= groups) {
      replay_meta(r, sh, p.B, g - groups);
      continue;
    }
    Group gr;
    int i, j;
    split_group<PPT>(g, groups_per_img, c.w, small, gr.b, gr.q, i, j);
    Pixels<PPT, CIN> px;
    // the mirror bit is per image and a wave may straddle two images: a
    // branch into a static body, as in decode_crop_kernel
    if (load_crop_group<PPT, CIN>(p, r, c, int64_t(sh.idx[gr.b]), sh.win[gr.b], i, j, px)) reverse_pixels<PPT, CIN>(px);
    emit<PPT, CIN, OUTT, LAYOUT, TBL, NT>(p, xf, cm, cout, hw, gr, px);
  }
}

// any window size / alignment / channel count: one window pixel per lane
template <int OUTT>
__global__ __launch_bounds__(kBlock) void replay_crop_scalar_kernel(DecodeParams p, ReplayParams r, ReplayCropParams c,
                                                                    int64_t meta_units) {
  __shared__ ReplayCropShared sh;
  const uint64_t ctr = r.counter ? r.counter[0] : r.ctr_value;
  const Xf xf = stage_xf(p.lut, sh.tab, p.Cout);
  replay_crop_table(p, r, c, ctr, sh);
  __syncthreads();
  const int64_t hw = int64_t(c.h) * c.w;
  const int64_t total = hw * p.B;
  const int64_t ie = hw * p.Cout;
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total + meta_units; g += int64_t(gridDim.x) * kBlock) {
    if (g >= total) {
      replay_meta(r, sh, p.B, g - total);
      continue;
    }
    const int b = int(g / hw);
    const int64_t q = g - int64_t(b) * hw;
    const int i = int(q / c.w), j = int(q - int64_t(i) * c.w);
    const uint32_t win = sh.win[b];
    const int y0 = int(win & 0x7FFFu) - c.pad, x0 = int((win >> 15) & 0x7FFFu) - c.pad;
    const int y = clampi(y0 + i, 0, p.H - 1);
    const int sy = p.flip_all ? p.H - 1 - y : y;
    const int x = clampi(x0 + ((win >> 31) ? c.w - 1 - j : j), 0, p.W - 1);
    const uint8_t* s = p.src + int64_t(sh.idx[b]) * r.frame_bytes + (int64_t(sy) * p.W + x) * p.Cin;
    for (int k = 0; k < p.Cout; ++k) {
      const float v = xf_value(xf, k, s[p.cmap[k]]);
      const int64_t off = int64_t(b) * ie + (p.layout == NCHW ? int64_t(k) * hw + q : q * p.Cout + k);
      if constexpr (OUTT == OUT_F32) reinterpret_cast<float*>(p.dst)[off] = v;
      else if constexpr (OUTT == OUT_BF16) reinterpret_cast<uint16_t*>(p.dst)[off] = f2bf(v);
      else if constexpr (OUTT == OUT_F16) reinterpret_cast<uint16_t*>(p.dst)[off] = f2h(v);
      else reinterpret_cast<uint8_t*>(p.dst)[off] = uint8_t(v);
    }
  }
}

template <int PPT, int CIN, int OUTT, int LAYOUT>
void launch_replay_crop_vec(const DecodeParams& p, const ReplayParams& r, const ReplayCropParams& c,
                            int64_t meta_units, int grid, hipStream_t s) {
  if constexpr (OUTT == OUT_F32 && LAYOUT == NCHW) {
    if (p.xf_table_only) {
      // non-temporal stores where they were measured (the kernel's comment);
      // BT_REPLAY_CROP_NT=0: plain stores
      static const bool nt = !(std::getenv("BT_REPLAY_CROP_NT") && std::getenv("BT_REPLAY_CROP_NT")[0] == '0');
      if (nt) replay_crop_vec_kernel<PPT, CIN, OUTT, LAYOUT, 1, true><<<grid, kBlock, 0, s>>>(p, r, c, meta_units);
      else replay_crop_vec_kernel<PPT, CIN, OUTT, LAYOUT, 1><<<grid, kBlock, 0, s>>>(p, r, c, meta_units);
      return;
    }
  }
  if (p.xf_table_only) replay_crop_vec_kernel<PPT, CIN, OUTT, LAYOUT, 1><<<grid, kBlock, 0, s>>>(p, r, c, meta_units);
  else replay_crop_vec_kernel<PPT, CIN, OUTT, LAYOUT, 0><<<grid, kBlock, 0, s>>>(p, r, c, meta_units);
}

template <int OUTT>
hipError_t launch_replay_crop(const DecodeParams& p, const ReplayParams& r, const ReplayCropParams& c,
                              int64_t meta_units, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  constexpr int64_t ELEM = elem_for(OUTT);
  // decode_crop's vector conditions on replay's dense store and output
  const bool vec = (c.w % PPT) == 0 && (p.W % 4) == 0 && r.frame_bytes % 16 == 0 && (p.Cin == 3 || p.Cin == 4) &&
                   (reinterpret_cast<uintptr_t>(p.src) % 16) == 0 && (reinterpret_cast<uintptr_t>(p.dst) % 16) == 0 &&
                   (int64_t(c.h) * c.w * p.Cout * ELEM) % 16 == 0;
  if (vec) {
    const int grid = grid_for(int64_t(p.B) * c.h * c.w / PPT + meta_units, p.max_grid);
    if (p.Cin == 4) {
      if (p.layout == NCHW) launch_replay_crop_vec<PPT, 4, OUTT, NCHW>(p, r, c, meta_units, grid, s);
      else launch_replay_crop_vec<PPT, 4, OUTT, NHWC>(p, r, c, meta_units, grid, s);
    } else {
      if (p.layout == NCHW) launch_replay_crop_vec<PPT, 3, OUTT, NCHW>(p, r, c, meta_units, grid, s);
      else launch_replay_crop_vec<PPT, 3, OUTT, NHWC>(p, r, c, meta_units, grid, s);
    }
  } else {
    replay_crop_scalar_kernel<OUTT><<<grid_for(int64_t(p.B) * c.h * c.w + meta_units, p.max_grid), kBlock, 0, s>>>(
        p, r, c, meta_units);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t replay_sample_crop(const DecodeParams& p, const ReplayParams& r, const ReplayCropParams& c0,
                              hipStream_t stream) {
  // every condition is checked here, before anything is launched
  if (p.B < 0 || p.B > kMaxReplayB || p.H <= 0 || p.W <= 0 || p.Cin < 1 || p.Cin > 4 || p.Cout < 1 || p.Cout > 4 ||
      !p.src || !p.dst || !p.lut || p.nsrcs || p.ndsts || p.src_offsets || p.flip || r.nmeta < 0 ||
      r.nmeta > kMaxMeta || r.frame_bytes != int64_t(p.H) * p.W * p.Cin)
    return hipErrorInvalidValue;
  if (p.layout != NCHW && p.layout != NHWC) return hipErrorInvalidValue;
  ReplayCropParams c = c0;
  if (c.h <= 0 || c.w <= 0 || c.pad < 0 || c.pad > 16383 || p.H + 2 * c.pad > 32767 || p.W + 2 * c.pad > 32767 ||
      c.h > p.H + 2 * c.pad || c.w > p.W + 2 * c.pad)
    return hipErrorInvalidValue;
  if (c.x_align != 1 && c.x_align != 4 && c.x_align != 16) return hipErrorInvalidValue;
  if (c.mode != kCropRandom && c.mode != kCropFixed) return hipErrorInvalidValue;
  if (c.mirror_threshold > (1u << 24)) return hipErrorInvalidValue;
  if (c.pad != 0 && (c.x_align != 1 || (c.mode != kCropRandom && !c.windows_in))) return hipErrorInvalidValue;
  if (c.mode == kCropFixed && !c.windows_in &&
      (c.y0 < 0 || c.x0 < 0 || c.y0 + c.h > p.H || c.x0 + c.w > p.W))
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(c.windows_in) | reinterpret_cast<uintptr_t>(c.crop_out)) % 4) return hipErrorInvalidValue;
  if (!r.index_in && (r.count < 1 || r.count > (int64_t(1) << 32))) return hipErrorInvalidValue;
  for (int k = 0; k < p.Cout; ++k)
    if (p.cmap[k] < 0 || p.cmap[k] >= p.Cin) return hipErrorInvalidValue;
  int64_t meta_units = 0;
  for (int k = 0; k < r.nmeta; ++k) {
    const int nb = r.meta_bytes[k];
    if (nb <= 0 || !r.meta_src[k] || !r.meta_dst[k]) return hipErrorInvalidValue;
    if (nb % 4 == 0 && ((reinterpret_cast<uintptr_t>(r.meta_src[k]) | reinterpret_cast<uintptr_t>(r.meta_dst[k])) % 4))
      return hipErrorInvalidValue;
    meta_units += int64_t(p.B) * (nb % 4 == 0 ? nb / 4 : nb);
  }
  if (p.B == 0) return hipSuccess;
  c.ny = uint32_t(p.H + 2 * c.pad - c.h + 1);
  c.nx = uint32_t((p.W + 2 * c.pad - c.w) / c.x_align + 1);
  const hipError_t e =
      with_out_dtype(p.out_dtype, [&](auto o) { return launch_replay_crop<o()>(p, r, c, meta_units, stream); });
  // a device counter moves on when this launch drew from it: indices, or windows
  const bool drew = !r.index_in || (c.mode == kCropRandom && !c.windows_in);
  if (e != hipSuccess || !r.counter || !drew) return e;
  replay_advance_kernel<<<1, 1, 0, stream>>>(r.counter, p.B);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// frame-stacked transitions (kernels.h: replay_sample_stack)
// ---------------------------------------------------------------------------
// replay_crop_vec_kernel's body over 2 * B * k VIRTUAL images of Cout planes:
// virtual image v = (d * B + b) * k + f is frame e[b][f + d] through window
// win[d * B + b], and lands at v * Cout * h * w of the dense output -- which is
// [2, B, k * Cout, h, w].  The block prologue builds the frame table and the
// windows in dynamic LDS: 4 * (B * (k + 1) + 2 B) bytes; with n-step returns
// (t.nstep = n) the table rows widen to k + n and a step offset per image joins
// them: 4 * (B * (k + n) + 3 B) bytes.
// Measured against the plain cropped sample of the same 2 B k images
// (profiles/r14/replay_stack.md; 640x480 RGBA, pad 4, k = 3, fp32): batch 64
// 340 against 334 us, batch 8 58.3 against 48.9 us -- the prologue's two
// dependent flag loads (candidates, then the walk back) are paid by each of
// the 8192 blocks, which at batch 8 have little else to do.  A one-block
// table kernel in front would take them out of the blocks; it is not built.
namespace {

// s in [-cap, 2 cap) -> [0, cap)
__device__ __forceinline__ int64_t ring_wrap(int64_t s, int64_t cap) { return s < 0 ? s + cap : (s >= cap ? s - cap : s); }

// One fp32 product / sum, rounded to nearest on its own.  HIP's __fmul_rn and
// __fadd_rn are the plain operators, which the compiler contracts into one FMA
// (one rounding) under the default -ffp-contract=fast: the n-step return has to
// give the bits of a float32 loop on the host, so these two opt out.
__device__ __forceinline__ float fmul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float fadd_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// Fills tbl [B][k + max(n, 1)], win [2][B] and, with n-step returns, stepo [B]
// (block 0 also the outputs); the caller syncs.  The `first` flags are loaded
// in groups whose addresses do not depend on each other: the four candidates
// of a Philox block, then the slots the walk back may stop at; only the stop
// position follows them.  The n-step walk forward reads first[c_2 .. c_n] and
// done[c_0 .. c_{n-1}], slots that depend on the anchor alone like the walk
// back's: its first four steps are issued ahead of the walk back's loads and
// read after them, so n <= 4 adds no load round at all.
// NS: n-step returns.  The 1-step launch is its own instantiation: with the
// walk behind a run-time branch it measured 2 % (batch 64) and 6 % (batch 8)
// slower than before the walk existed (profiles/r16/replay_nstep.md).
template <bool NS>
__device__ __forceinline__ void stack_table(const DecodeParams& p, const ReplayParams& r, const ReplayCropParams& c,
                                            const ReplayStackParams& t, uint64_t ctr, uint32_t* tbl, uint32_t* win,
                                            uint32_t* stepo) {
  const int k = t.stack, S = t.stride, B = p.B, n = NS ? t.nstep : 0;
  const int k1 = k + (n > 1 ? n : 1);
  const int64_t cap = t.capacity;
  // a device state was not seen by the host: reduced into the ring
  int64_t head = t.state ? t.state[0] : t.head, size = t.state ? t.state[1] : t.size;
  head = head < 0 ? 0 : (head >= cap ? cap - 1 : head);
  size = size < 0 ? 0 : (size > cap ? cap : size);
  const bool filled = size > S;
  const uint32_t range = filled ? uint32_t(size - S) : 0u;
  for (int b = threadIdx.x; b < B; b += kBlock) {
    int64_t anchor = 0, succ = 0;
    bool valid = false;
    if (r.index_in) {
      anchor = r.index_in[b] % cap;
      if (anchor < 0) anchor += cap;
      succ = ring_wrap(anchor + S, cap);
      const int64_t age = ring_wrap(head - 1 - anchor, cap);
      valid = filled && age >= S && age < size && t.first[succ] == 0;
    } else {
      for (int blk = 0; blk < 4 && !valid; ++blk) {
        uint32_t o[4];
        philox_block(r.seed, ctr, uint32_t(b), blk ? uint32_t(blk + 1) : 0u, o);
        int64_t s[4], nx[4];
        uint8_t f[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          s[u] = ring_wrap(head - 1 - (int64_t(S) + __umulhi(o[u], range)), cap);
          nx[u] = ring_wrap(s[u] + S, cap);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) f[u] = t.first[nx[u]];
        anchor = s[3];   // none valid: the block's last candidate
#pragma unroll
        for (int u = 3; u >= 0; --u)
          if (f[u] == 0) anchor = s[u], succ = nx[u], valid = true;
      }
      valid = valid && filled;
    }
    if (!valid) succ = anchor;
    uint32_t* e = tbl + b * k1;
    e[k - 1] = uint32_t(anchor);
    if constexpr (!NS) e[k] = uint32_t(succ);
    // n-step: bit j of dmask: done[c_j] != 0 (j < n); bit j of fmask:
    // first[c_j] != 0 (2 <= j <= n).  Step j of a group reads done[c_j] and
    // first[c_{j + 2}]; steps past n - 1 repeat it (their bits are dropped).
    uint32_t dmask = 0, fmask = 0;
    uint8_t gd[4] = {0, 0, 0, 0}, gf[4] = {0, 0, 0, 0};
    int64_t fwd = anchor;   // c_j of the next forward step
    if constexpr (NS) {
      int64_t a[4], a2[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u > 0 && u < n) fwd = ring_wrap(fwd + S, cap);
        a[u] = fwd;
        a2[u] = ring_wrap(ring_wrap(fwd + S, cap) + S, cap);
      }
      if (t.done) {
#pragma unroll
        for (int u = 0; u < 4; ++u) gd[u] = t.done[a[u]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) gf[u] = t.first[a2[u]];
    }
    // walk back: slot c_m = anchor - m S, m < k - 1, stops the walk when it is
    // a first frame or the oldest stored one; stopping is final, so the flags
    // of all c_m are read at once (indices past k - 2 repeat the last)
    uint32_t stop = 0;
    int64_t s = anchor;
    for (int m0 = 0; m0 < k - 1; m0 += 4) {
      int64_t a[4];
      uint8_t f[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = s;
        if (m0 + u < k - 2) s = ring_wrap(s - S, cap);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) f[u] = t.first[a[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (f[u] != 0) stop |= 1u << (m0 + u < k - 2 ? m0 + u : k - 2);
    }
    const int64_t age0 = ring_wrap(head - 1 - anchor, cap);
    int mstop = k - 1;
    for (int m = k - 2; m >= 0; --m)
      if (((stop >> m) & 1u) || age0 + int64_t(m + 1) * S >= size) mstop = m;
    s = anchor;
    for (int m = 1; m <= k - 1; ++m) {
      if (m <= mstop) s = ring_wrap(s - S, cap);
      e[k - 1 - m] = uint32_t(s);
    }
    int steps = 0;
    bool terminated = false;
    if constexpr (NS) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < n && gd[u] != 0) dmask |= 1u << u;
        if (u + 2 <= n && gf[u] != 0) fmask |= 1u << (u + 2);
      }
      for (int j0 = 4; j0 < n; j0 += 4) {   // n > 4: further groups, still anchor-only addresses
        int64_t a[4], a2[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (j0 + u < n) fwd = ring_wrap(fwd + S, cap);
          a[u] = fwd;
          a2[u] = ring_wrap(ring_wrap(fwd + S, cap) + S, cap);
        }
        if (t.done) {
#pragma unroll
          for (int u = 0; u < 4; ++u) gd[u] = t.done[a[u]];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) gf[u] = t.first[a2[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (j0 + u < n && gd[u] != 0) dmask |= 1u << (j0 + u);
          if (j0 + u + 2 <= n && gf[u] != 0) fmask |= 1u << (j0 + u + 2);
        }
      }
      if (valid) {
        steps = 1;
        while (steps < n && ((dmask >> (steps - 1)) & 1u) == 0 && age0 - int64_t(steps) * S >= S &&
               ((fmask >> (steps + 1)) & 1u) == 0)
          ++steps;
        terminated = ((dmask >> (steps - 1)) & 1u) != 0;
      }
      // e[k - 1 + j] = c_min(j, m); succ becomes c_m
      succ = anchor;
      for (int j = 1; j <= n; ++j) {
        if (j <= steps) succ = ring_wrap(succ + S, cap);
        e[k - 1 + j] = uint32_t(succ);
      }
      stepo[b] = uint32_t(steps > 1 ? steps : 1);
    }
    const uint32_t w0 = replay_window(p, c, ctr, b, 1u);
    const uint32_t w1 = t.shared_window ? w0 : replay_window(p, c, ctr, b, 5u);
    win[b] = w0, win[B + b] = w1;
    if (blockIdx.x == 0) {
      if (r.index_out) r.index_out[b] = anchor;
      if (t.next_index_out) t.next_index_out[b] = succ;
      if (t.valid_out) t.valid_out[b] = valid;
      if (c.crop_out) {
        c.crop_out[3 * b] = int(w0 & 0x7FFFu) - c.pad;
        c.crop_out[3 * b + 1] = int((w0 >> 15) & 0x7FFFu) - c.pad;
        c.crop_out[3 * b + 2] = int(w0 >> 31);
      }
      if (t.next_crop_out) {
        t.next_crop_out[3 * b] = int(w1 & 0x7FFFu) - c.pad;
        t.next_crop_out[3 * b + 1] = int((w1 >> 15) & 0x7FFFu) - c.pad;
        t.next_crop_out[3 * b + 2] = int(w1 >> 31);
      }
      if constexpr (NS) {
        // the rewards of c_0 .. c_{m-1}: independent loads, four at a time;
        // every product and sum rounded on its own (no FMA)
        float g = 1.f, R = 0.f;
        int64_t q = anchor;
        for (int j0 = 0; j0 < steps; j0 += 4) {
          float rw[4];
          int64_t a[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (j0 + u > 0 && j0 + u < steps) q = ring_wrap(q + S, cap);
            a[u] = q;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) rw[u] = t.reward[a[u]];
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (j0 + u < steps) {
              R = fadd_rn(R, fmul_rn(g, rw[u]));
              g = fmul_rn(g, t.gamma);
            }
        }
        if (t.return_out) t.return_out[b] = R;
        if (t.discount_out) t.discount_out[b] = (terminated || !valid) ? 0.f : g;
        if (t.steps_out) t.steps_out[b] = steps;
      }
    }
  }
}

// metadata unit m of n columns gathered at table column `col` (replay_meta's units)
__device__ __forceinline__ void stack_meta_cols(int n, const uint8_t* const* src, uint8_t* const* dst, const int* bytes,
                                                const uint32_t* tbl, int k1, int col, int B, int64_t m) {
  for (int q = 0; q < n; ++q) {
    const int nb = bytes[q];
    const int w = (nb % 4 == 0) ? 4 : 1;
    const int64_t per = nb / w, units = per * B;
    if (m < units) {
      const int b = int(m / per);
      const int64_t j = (m - int64_t(b) * per) * w;
      const uint8_t* s = src[q] + int64_t(tbl[b * k1 + col]) * nb + j;
      uint8_t* d = dst[q] + int64_t(b) * nb + j;
      if (w == 4) *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
      else *d = *s;
      return;
    }
    m -= units;
  }
}

// anchor columns (r.meta_*, from e[k - 1]) first, then the next columns (from the
// row's last entry: e[k], with n-step returns e[k - 1 + n] = c_m)
template <bool NS>
__device__ __forceinline__ void stack_meta(const ReplayParams& r, const ReplayStackParams& t, const uint32_t* tbl, int B,
                                           int64_t anchor_units, int64_t m) {
  const int k1 = t.stack + (NS && t.nstep > 1 ? t.nstep : 1);
  if (m < anchor_units) stack_meta_cols(r.nmeta, r.meta_src, r.meta_dst, r.meta_bytes, tbl, k1, t.stack - 1, B, m);
  else stack_meta_cols(t.nnext, t.next_src, t.next_dst, t.next_bytes, tbl, k1, k1 - 1, B, m - anchor_units);
}

// virtual image v -> its frame slot and packed window.  stepo: the per-image
// offset of the next stack in its table row (n-step returns; else it is 1)
template <bool NS>
__device__ __forceinline__ void stack_resolve(const uint32_t* tbl, const uint32_t* win, const uint32_t* stepo, int B,
                                              int k, int k1, uint32_t v, uint32_t& slot, uint32_t& w) {
  const uint32_t Bk = uint32_t(B) * uint32_t(k);
  const uint32_t d = v >= Bk ? 1u : 0u;
  const uint32_t rem = v - d * Bk;
  const uint32_t b = rem / uint32_t(k), f = rem - b * uint32_t(k);
  uint32_t off = d;
  if constexpr (NS) off = d ? stepo[b] : 0u;
  slot = tbl[b * uint32_t(k1) + f + off];
  w = win[d * uint32_t(B) + b];
}

// TBL / NT: replay_crop_vec_kernel's choices, inherited
template <int PPT, int CIN, int OUTT, int TBL, bool NT = false, bool NS = false>
__global__ __launch_bounds__(kBlock) void replay_stack_vec_kernel(DecodeParams p, ReplayParams r, ReplayCropParams c,
                                                                  ReplayStackParams t, int64_t meta_units,
                                                                  int64_t anchor_units) {
  __shared__ uint32_t tab[kTabWords];
  extern __shared__ uint32_t stack_lds[];
  const int k1 = t.stack + (NS && t.nstep > 1 ? t.nstep : 1);
  uint32_t* tbl = stack_lds;
  uint32_t* win = stack_lds + p.B * k1;
  uint32_t* stepo = win + 2 * p.B;   // NS only
  const int64_t hw = int64_t(c.h) * c.w;
  const int64_t groups_per_img = hw / PPT;
  const int64_t groups = groups_per_img * 2 * p.B * t.stack;
  const int cout = p.Cout;
  int cm[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) cm[q] = p.cmap[q];
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  const bool small = groups + meta_units + stride < (int64_t(1) << 31);
  const uint64_t ctr = r.counter ? r.counter[0] : r.ctr_value;
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  stack_table<NS>(p, r, c, t, ctr, tbl, win, stepo);
  __syncthreads();
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < groups + meta_units; g += stride) {
    if (g >= groups) {
      stack_meta<NS>(r, t, tbl, p.B, anchor_units, g - groups);
      continue;
    }
    Group gr;
    int i, j;
    split_group<PPT>(g, groups_per_img, c.w, small, gr.b, gr.q, i, j);
    uint32_t slot, w;
    stack_resolve<NS>(tbl, win, stepo, p.B, t.stack, k1, uint32_t(gr.b), slot, w);
    Pixels<PPT, CIN> px;
    if (load_crop_group<PPT, CIN>(p, r, c, int64_t(slot), w, i, j, px)) reverse_pixels<PPT, CIN>(px);
    emit<PPT, CIN, OUTT, NCHW, TBL, NT>(p, xf, cm, cout, hw, gr, px);
  }
}

// any window size / alignment / channel count: one window pixel per lane
template <int OUTT, bool NS = false>
__global__ __launch_bounds__(kBlock) void replay_stack_scalar_kernel(DecodeParams p, ReplayParams r, ReplayCropParams c,
                                                                     ReplayStackParams t, int64_t meta_units,
                                                                     int64_t anchor_units) {
  __shared__ uint32_t tab[kTabWords];
  extern __shared__ uint32_t stack_lds[];
  const int k1 = t.stack + (NS && t.nstep > 1 ? t.nstep : 1);
  uint32_t* tbl = stack_lds;
  uint32_t* wins = stack_lds + p.B * k1;
  uint32_t* stepo = wins + 2 * p.B;   // NS only
  const uint64_t ctr = r.counter ? r.counter[0] : r.ctr_value;
  const Xf xf = stage_xf(p.lut, tab, p.Cout);
  stack_table<NS>(p, r, c, t, ctr, tbl, wins, stepo);
  __syncthreads();
  const int64_t hw = int64_t(c.h) * c.w;
  const int64_t total = hw * 2 * p.B * t.stack;
  const int64_t ie = hw * p.Cout;
  for (int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x; g < total + meta_units; g += int64_t(gridDim.x) * kBlock) {
    if (g >= total) {
      stack_meta<NS>(r, t, tbl, p.B, anchor_units, g - total);
      continue;
    }
    const int64_t v = g / hw;
    const int64_t q = g - v * hw;
    const int i = int(q / c.w), j = int(q - int64_t(i) * c.w);
    uint32_t slot, win;
    stack_resolve<NS>(tbl, wins, stepo, p.B, t.stack, k1, uint32_t(v), slot, win);
    const int y0 = int(win & 0x7FFFu) - c.pad, x0 = int((win >> 15) & 0x7FFFu) - c.pad;
    const int y = clampi(y0 + i, 0, p.H - 1);
    const int sy = p.flip_all ? p.H - 1 - y : y;
    const int x = clampi(x0 + ((win >> 31) ? c.w - 1 - j : j), 0, p.W - 1);
    const uint8_t* s = p.src + int64_t(slot) * r.frame_bytes + (int64_t(sy) * p.W + x) * p.Cin;
    for (int ch = 0; ch < p.Cout; ++ch) {
      const float val = xf_value(xf, ch, s[p.cmap[ch]]);
      const int64_t off = v * ie + int64_t(ch) * hw + q;
      if constexpr (OUTT == OUT_F32) reinterpret_cast<float*>(p.dst)[off] = val;
      else if constexpr (OUTT == OUT_BF16) reinterpret_cast<uint16_t*>(p.dst)[off] = f2bf(val);
      else if constexpr (OUTT == OUT_F16) reinterpret_cast<uint16_t*>(p.dst)[off] = f2h(val);
      else reinterpret_cast<uint8_t*>(p.dst)[off] = uint8_t(val);
    }
  }
}

template <int PPT, int CIN, int OUTT, bool NS>
void launch_replay_stack_vec(const DecodeParams& p, const ReplayParams& r, const ReplayCropParams& c,
                             const ReplayStackParams& t, int64_t meta_units, int64_t anchor_units, int grid, size_t lds,
                             hipStream_t s) {
  if constexpr (OUTT == OUT_F32) {
    if (p.xf_table_only) {
      // non-temporal stores as in launch_replay_crop_vec (BT_REPLAY_CROP_NT=0: plain stores)
      static const bool nt = !(std::getenv("BT_REPLAY_CROP_NT") && std::getenv("BT_REPLAY_CROP_NT")[0] == '0');
      if (nt) replay_stack_vec_kernel<PPT, CIN, OUTT, 1, true, NS><<<grid, kBlock, lds, s>>>(p, r, c, t, meta_units, anchor_units);
      else replay_stack_vec_kernel<PPT, CIN, OUTT, 1, false, NS><<<grid, kBlock, lds, s>>>(p, r, c, t, meta_units, anchor_units);
      return;
    }
  }
  if (p.xf_table_only) replay_stack_vec_kernel<PPT, CIN, OUTT, 1, false, NS><<<grid, kBlock, lds, s>>>(p, r, c, t, meta_units, anchor_units);
  else replay_stack_vec_kernel<PPT, CIN, OUTT, 0, false, NS><<<grid, kBlock, lds, s>>>(p, r, c, t, meta_units, anchor_units);
}

template <int OUTT, bool NS>
hipError_t launch_replay_stack(const DecodeParams& p, const ReplayParams& r, const ReplayCropParams& c,
                               const ReplayStackParams& t, int64_t meta_units, int64_t anchor_units, hipStream_t s) {
  constexpr int PPT = ppt_for(OUTT);
  constexpr int64_t ELEM = elem_for(OUTT);
  // frame table [B][k + max(n, 1)], windows [2][B], with n-step returns the step offsets [B]
  const size_t lds = sizeof(uint32_t) * (size_t(p.B) * size_t(t.stack + (t.nstep > 1 ? t.nstep : 1)) +
                                         (t.nstep ? 3 : 2) * size_t(p.B));
  const int64_t pixels = int64_t(2) * p.B * t.stack * c.h * c.w;
  // launch_replay_crop's vector conditions
  const bool vec = (c.w % PPT) == 0 && (p.W % 4) == 0 && r.frame_bytes % 16 == 0 && (p.Cin == 3 || p.Cin == 4) &&
                   (reinterpret_cast<uintptr_t>(p.src) % 16) == 0 && (reinterpret_cast<uintptr_t>(p.dst) % 16) == 0 &&
                   (int64_t(c.h) * c.w * p.Cout * ELEM) % 16 == 0;
  if (vec) {
    const int grid = grid_for(pixels / PPT + meta_units, p.max_grid);
    if (p.Cin == 4) launch_replay_stack_vec<PPT, 4, OUTT, NS>(p, r, c, t, meta_units, anchor_units, grid, lds, s);
    else launch_replay_stack_vec<PPT, 3, OUTT, NS>(p, r, c, t, meta_units, anchor_units, grid, lds, s);
  } else {
    replay_stack_scalar_kernel<OUTT, NS><<<grid_for(pixels + meta_units, p.max_grid), kBlock, lds, s>>>(p, r, c, t, meta_units,
                                                                                                   anchor_units);
  }
  return hipGetLastError();
}

// units of n metadata columns for B images; false: a column is malformed
bool meta_cols_units(int n, const uint8_t* const* src, uint8_t* const* dst, const int* bytes, int B, int64_t& units) {
  units = 0;
  if (n < 0 || n > kMaxMeta) return false;
  for (int q = 0; q < n; ++q) {
    const int nb = bytes[q];
    if (nb <= 0 || !src[q] || !dst[q]) return false;
    if (nb % 4 == 0 && ((reinterpret_cast<uintptr_t>(src[q]) | reinterpret_cast<uintptr_t>(dst[q])) % 4)) return false;
    units += int64_t(B) * (nb % 4 == 0 ? nb / 4 : nb);
  }
  return true;
}

}  // namespace

hipError_t replay_sample_stack(const DecodeParams& p, const ReplayParams& r, const ReplayCropParams& c0,
                               const ReplayStackParams& t, hipStream_t stream) {
  // every condition is checked here, before anything is launched
  if (p.B < 0 || p.B > kMaxReplayB || p.H <= 0 || p.W <= 0 || p.Cin < 1 || p.Cin > 4 || p.Cout < 1 || p.Cout > 4 ||
      !p.src || !p.dst || !p.lut || p.nsrcs || p.ndsts || p.src_offsets || p.flip ||
      r.frame_bytes != int64_t(p.H) * p.W * p.Cin || p.layout != NCHW)
    return hipErrorInvalidValue;
  if (t.stack < 1 || t.stack > 16 || int64_t(p.B) * (t.stack + 1) > 8192) return hipErrorInvalidValue;
  if (t.capacity < 2 || t.capacity > (int64_t(1) << 31) || t.stride < 1 || t.stride >= t.capacity || !t.first)
    return hipErrorInvalidValue;
  if (!t.state && (t.size <= t.stride || t.size > t.capacity || t.head < 0 || t.head >= t.capacity))
    return hipErrorInvalidValue;
  if (t.nstep != 0) {   // n-step returns: LDS stays 4 * (B (k + n) + 3 B) <= 44 KiB next to the value table
    if (t.nstep < 1 || t.nstep > 16 || int64_t(p.B) * (t.stack + t.nstep) > 8192 || !t.reward) return hipErrorInvalidValue;
    if (!(t.gamma >= 0.f && t.gamma <= 1.f)) return hipErrorInvalidValue;   // NaN fails both
    if ((reinterpret_cast<uintptr_t>(t.reward) | reinterpret_cast<uintptr_t>(t.return_out) |
         reinterpret_cast<uintptr_t>(t.discount_out) | reinterpret_cast<uintptr_t>(t.steps_out)) % 4)
      return hipErrorInvalidValue;
  }
  ReplayCropParams c = c0;
  if (c.h == 0 && c.w == 0) {   // no crop: the whole frame at (0, 0)
    c = ReplayCropParams();
    c.h = p.H, c.w = p.W, c.mode = kCropFixed;
    if (p.H > 32767 || p.W > 32767) return hipErrorInvalidValue;
  }
  if (c.windows_in) return hipErrorInvalidValue;
  if (c.h <= 0 || c.w <= 0 || c.pad < 0 || c.pad > 16383 || p.H + 2 * c.pad > 32767 || p.W + 2 * c.pad > 32767 ||
      c.h > p.H + 2 * c.pad || c.w > p.W + 2 * c.pad)
    return hipErrorInvalidValue;
  if (c.x_align != 1 && c.x_align != 4 && c.x_align != 16) return hipErrorInvalidValue;
  if (c.mode != kCropRandom && c.mode != kCropFixed) return hipErrorInvalidValue;
  if (c.mirror_threshold > (1u << 24)) return hipErrorInvalidValue;
  if (c.pad != 0 && (c.x_align != 1 || c.mode != kCropRandom)) return hipErrorInvalidValue;
  if (c.mode == kCropFixed && (c.y0 < 0 || c.x0 < 0 || c.y0 + c.h > p.H || c.x0 + c.w > p.W)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(c.crop_out) | reinterpret_cast<uintptr_t>(t.next_crop_out)) % 4) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(r.index_in) | reinterpret_cast<uintptr_t>(r.index_out) |
       reinterpret_cast<uintptr_t>(t.next_index_out) | reinterpret_cast<uintptr_t>(t.state)) % 8)
    return hipErrorInvalidValue;
  for (int q = 0; q < p.Cout; ++q)
    if (p.cmap[q] < 0 || p.cmap[q] >= p.Cin) return hipErrorInvalidValue;
  int64_t anchor_units = 0, next_units = 0;
  if (!meta_cols_units(r.nmeta, r.meta_src, r.meta_dst, r.meta_bytes, p.B, anchor_units) ||
      !meta_cols_units(t.nnext, t.next_src, t.next_dst, t.next_bytes, p.B, next_units))
    return hipErrorInvalidValue;
  if (p.B == 0) return hipSuccess;
  c.ny = uint32_t(p.H + 2 * c.pad - c.h + 1);
  c.nx = uint32_t((p.W + 2 * c.pad - c.w) / c.x_align + 1);
  const int64_t meta_units = anchor_units + next_units;
  const hipError_t e = with_out_dtype(p.out_dtype, [&](auto o) {
    return t.nstep ? launch_replay_stack<o(), true>(p, r, c, t, meta_units, anchor_units, stream)
                   : launch_replay_stack<o(), false>(p, r, c, t, meta_units, anchor_units, stream);
  });
  // a device counter moves on when this launch drew from it: anchors, or windows
  const bool drew = !r.index_in || c.mode == kCropRandom;
  if (e != hipSuccess || !r.counter || !drew) return e;
  replay_advance_kernel<<<1, 1, 0, stream>>>(r.counter, p.B);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// color4x4 on MFMA (v_mfma_f32_4x4x1_16b_f32)
// ---------------------------------------------------------------------------
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Each wave owns 256 consecutive pixels of one image per iteration.
// Operand map of the 16-block 4x4x1 MFMA (lane l = 4*blk + i):
//   A[row i][0] of block blk, B[0][col i] of block blk, D[reg r][col i].
// Row i of block blk at sub-step s (0..3) is pixel 64*i + 4*blk + s, so each
// lane's A operands over the four sub-steps are 4 consecutive pixels -> ONE
// 16-byte load.  K (input channel) accumulates over 4 MFMAs, B = M[i][k].
// Lane (blk, i) receives in reg r the output channel i of pixel
// 64*r + 4*blk + s; over s that is 4 consecutive pixels -> one float4 per
// reg, and for a fixed reg the 16 lanes of one channel cover 64 contiguous
// pixels: every store instruction writes four 256-byte plane runs.
// Row j (output channel) of image b's affine transform, by p.mat_mode.
__device__ __forceinline__ void color_row(const Color4x4Params& p, int b, int j, float bm[4], float& bj) {
  if (p.mat_mode == kColorJitter) {
    const float br = p.jit[b][0], c = p.jit[b][1], s = p.jit[b][2];
    float sn, cs;
    __sincosf(6.283185307179586f * p.jit[b][3], &sn, &cs);
    // row j of the hue rotation about the grey axis (rows sum to 1)
    float h0, h1, h2;
    if (j == 0) h0 = 0.213f + cs * 0.787f - sn * 0.213f, h1 = 0.715f - cs * 0.715f - sn * 0.715f,
                h2 = 0.072f - cs * 0.072f + sn * 0.928f;
    else if (j == 1) h0 = 0.213f - cs * 0.213f + sn * 0.143f, h1 = 0.715f + cs * 0.285f + sn * 0.140f,
                     h2 = 0.072f - cs * 0.072f - sn * 0.283f;
    else h0 = 0.213f - cs * 0.213f - sn * 0.787f, h1 = 0.715f - cs * 0.715f + sn * 0.715f,
         h2 = 0.072f + cs * 0.928f + sn * 0.072f;
    // (Hue . Sat)[j][k] = s * Hue[j][k] + (1 - s) * w[k]  (Hue's rows sum to 1)
    const float bc = br * c, t = 1.f - s;
    if (j < 3) {
      bm[0] = bc * (s * h0 + t * 0.213f), bm[1] = bc * (s * h1 + t * 0.715f), bm[2] = bc * (s * h2 + t * 0.072f);
      bm[3] = 0.f;
      bj = (1.f - c) * p.pivot;
    } else {
      bm[0] = bm[1] = bm[2] = 0.f, bm[3] = 1.f, bj = 0.f;
    }
    return;
  }
  const float* M = p.mat_mode == kColorPos ? p.Ms + 20 * int(p.mat_pos[b])
                   : p.mat_mode == kColorEach ? p.Ms + 20 * int64_t(b) : p.M;
  const float* bias = p.mat_mode == kColorOne ? p.bias : M + 16;
#pragma unroll
  for (int k = 0; k < 4; ++k) bm[k] = M[j * 4 + k];
  bj = bias[j];
}

__global__ __launch_bounds__(kBlock) void color4x4_kernel(Color4x4Params p) {
  __shared__ uint32_t tab[kTabWords];
  const Xf xf = stage_xf(p.lut, tab, 4);   // indexed by INPUT channel here
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 3;
  float bm[4];
  float bj = 0.f;
  int mat_b = -1;   // the image whose matrix row bm / bj hold
  const int64_t HW = int64_t(p.H) * p.W;
  const int64_t segs_per_img = HW / 256;   // host guarantees HW % 256 == 0
  const int64_t total = segs_per_img * p.B;
  const int64_t stride = int64_t(gridDim.x) * (kBlock / 64);
  for (int64_t g = int64_t(blockIdx.x) * (kBlock / 64) + wave; g < total; g += stride) {
    const int b = int(g / segs_per_img);
    const int64_t q0 = (g - int64_t(b) * segs_per_img) * 256;
    if (b != mat_b) {   // wave-uniform: a new image's row j of its transform
      mat_b = b;
      color_row(p, b, j, bm, bj);
    }
    // lane's 4 pixels share a row (W % 4 == 0); the segment may span rows
    const int blk = lane >> 2;
    const int64_t pl = q0 + 64 * j + 4 * blk;
    const int y = int(pl / p.W), x = int(pl - int64_t(y) * p.W);
    const bool flip = p.flip_all || (p.flip && p.flip[b]) || (b < 256 && ((p.flip_bits[b >> 6] >> (b & 63)) & 1));
    const int sy = flip ? p.H - 1 - y : y;
    const uint8_t* img = p.nsrcs ? p.srcs[b] : p.src + (p.src_offsets ? p.src_offsets[b] : int64_t(b) * HW * 4);
    const uint4 v4 = *reinterpret_cast<const uint4*>(img + (int64_t(sy) * p.W + x) * 4);
    const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
    f32x4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const uint32_t px = w[s];
      const float a0 = xf_value(xf, 0, px & 0xff), a1 = xf_value(xf, 1, (px >> 8) & 0xff);
      const float a2 = xf_value(xf, 2, (px >> 16) & 0xff), a3 = xf_value(xf, 3, px >> 24);
      f32x4 c = {bj, bj, bj, bj};
      c = __builtin_amdgcn_mfma_f32_4x4x1f32(a0, bm[0], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_4x4x1f32(a1, bm[1], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_4x4x1f32(a2, bm[2], c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_4x4x1f32(a3, bm[3], c, 0, 0, 0);
      acc[s] = c;
    }
    if (j < p.Cout) {
      // pixel 64*r + 4*blk + s  <-  acc[s][r]
      float* d = image_out<float>(p, b, HW * p.Cout) + int64_t(j) * HW + q0 + 4 * blk;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4*>(d + 64 * r) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
    }
  }
}

__global__ void project_kernel(const float* pts, int64_t N, const float* PV, const float* V, int W, int H,
                               int upper_left, float* out_px, float* out_depth) {
  __shared__ float m[32];
  if (threadIdx.x < 16) m[threadIdx.x] = PV[threadIdx.x];
  else if (threadIdx.x < 32) m[threadIdx.x] = V[threadIdx.x - 16];
  __syncthreads();
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < N; i += int64_t(gridDim.x) * blockDim.x) {
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    float c[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) c[r] = m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3];
    const float nx = c[0] / c[3], ny = c[1] / c[3];
    float px = (nx + 1.f) * 0.5f, py = (ny + 1.f) * 0.5f;
    if (upper_left) py = 1.f - py;
    out_px[2 * i] = px * W;
    out_px[2 * i + 1] = py * H;
    if (out_depth) out_depth[i] = -(m[16 + 8] * x + m[16 + 9] * y + m[16 + 10] * z + m[16 + 11]);
  }
}

}  // namespace

hipError_t color4x4(const Color4x4Params& p, hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  if ((p.mat_mode == kColorPos || p.mat_mode == kColorJitter) && p.B > kMaxSrcs) return hipErrorInvalidValue;
  if ((p.mat_mode == kColorPos || p.mat_mode == kColorEach) && !p.Ms) return hipErrorInvalidValue;
  if ((int64_t(p.H) * p.W) % 256 != 0 || p.W % 4 != 0 || p.Cout < 1 || p.Cout > 4 ||
      (p.ndsts ? !dsts_ok(p.dsts, p.ndsts, p.B, 16) : (reinterpret_cast<uintptr_t>(p.dst) % 16) != 0) ||
      (p.nsrcs ? !srcs_ok(p.srcs, p.nsrcs, p.B, 16) : (reinterpret_cast<uintptr_t>(p.src) % 16) != 0))
    return hipErrorInvalidValue;
  int64_t waves = int64_t(p.B) * p.H * p.W / 256;
  int64_t blocks = (waves + 3) / 4;
  int grid = int(blocks < 4096 ? blocks : 4096);
  color4x4_kernel<<<grid, kBlock, 0, stream>>>(p);
  return hipGetLastError();
}

hipError_t project(const float* pts, int64_t N, const float* PV, const float* V, int W, int H, int upper_left,
                   float* out_px, float* out_depth, hipStream_t stream) {
  if (N <= 0) return hipSuccess;
  int64_t blocks = (N + kBlock - 1) / kBlock;
  int grid = int(blocks < 1024 ? blocks : 1024);
  project_kernel<<<grid, kBlock, 0, stream>>>(pts, N, PV, V, W, H, upper_left, out_px, out_depth);
  return hipGetLastError();
}

}  // namespace gpu
}  // namespace btn
