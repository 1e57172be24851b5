// Shared device helpers for the gfx950 (MI355X, CDNA4) kernels. wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// the C ABI: every descriptor struct, every MAGIC_* code and the prototype each extern "C" definition of a unit is checked against
#include "../../include/magic_hip.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
// second 16-bit storage type: IEEE half (11 significand bits against bf16's 8: ~8x less rounding per stored activation / weight; the
// same MFMA rate, v_mfma_f32_16x16x32_f16).  Every 16-bit kernel is written once over Hh in {bf16, f16}.
typedef _Float16 f16;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;

#define DT_F32 0
#define DT_BF16 1
#define DT_F16 2
static inline bool dtype_ok(int dt) { return dt == DT_F32 || dt == DT_BF16 || dt == DT_F16; }
static inline bool dtype_is16(int dt) { return dt == DT_BF16 || dt == DT_F16; }

// Host-side dispatch: the statement(s) after `dtype` are written once over the type name TY and instantiated in the order bf16, f16, float.
// A dtype outside the three takes the LAST branch (float; f16 for DISPATCH_H): an entry point that must refuse it checks dtype_ok /
// dtype_is16 before it dispatches.  DISPATCH_H is for the kernels that have no float instantiation.
#define DISPATCH_T(dtype, ...)                                                        \
  do {                                                                                \
    if ((dtype) == DT_BF16) { typedef bf16 TY; __VA_ARGS__; }                          \
    else if ((dtype) == DT_F16) { typedef f16 TY; __VA_ARGS__; }                       \
    else { typedef float TY; __VA_ARGS__; }                                           \
  } while (0)
#define DISPATCH_H(dtype, ...)                                                        \
  do {                                                                                \
    if ((dtype) == DT_BF16) { typedef bf16 TY; __VA_ARGS__; }                          \
    else { typedef f16 TY; __VA_ARGS__; }                                             \
  } while (0)
// F(type, NIT) over dtype x the row width H in {128, 256, 384, 768} = the S / M / B / L family (run_r2r_kdl_valid.sh:85-94), NIT = H / 128;
// any other H RETURNS MAGIC_ERR_UNSUPPORTED from the calling function
#define DISPATCH_NIT(dtype, H, F)                                                                                       \
  DISPATCH_T(dtype, if ((H) == 128) F(TY, 1); else if ((H) == 256) F(TY, 2); else if ((H) == 384) F(TY, 3);              \
                    else if ((H) == 768) F(TY, 6); else return MAGIC_ERR_UNSUPPORTED)
// second axis, nested inside either: a small run-time integer `v` as the compile-time constant IV, one of the listed values (any other
// value takes the last one)
#define DISPATCH_I2(v, A, B, ...)                                                     \
  do {                                                                                \
    if ((v) == (A)) { constexpr int IV = (A); __VA_ARGS__; }                           \
    else { constexpr int IV = (B); __VA_ARGS__; }                                     \
  } while (0)
#define DISPATCH_I3(v, A, B, C, ...)                                                  \
  do {                                                                                \
    if ((v) == (A)) { constexpr int IV = (A); __VA_ARGS__; }                           \
    else if ((v) == (B)) { constexpr int IV = (B); __VA_ARGS__; }                      \
    else { constexpr int IV = (C); __VA_ARGS__; }                                     \
  } while (0)

#define WAVE 64

__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(bf16 x) { return (float)x; }
__device__ __forceinline__ float to_f(f16 x) { return (float)x; }
template <typename T> __device__ __forceinline__ T from_f(float x);
template <> __device__ __forceinline__ float from_f<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16 from_f<bf16>(float x) { return (bf16)x; }
template <> __device__ __forceinline__ f16 from_f<f16>(float x) { return (f16)x; }

// MFMA operand vectors of a 16-bit type, the 16x16x32 product, and the transposing LDS read (ds_read_b64_tr_b16: each lane of a 16-lane
// group receives element (l & 15) of 4 consecutive rows) -- the only places where bf16 and f16 need different instructions / builtins
template <typename Hh> struct H16;
template <> struct H16<bf16> { typedef bf16x8 v8; typedef bf16x4 v4; };
template <> struct H16<f16> { typedef f16x8 v8; typedef f16x4 v4; };
template <typename Hh> using h16x8 = typename H16<Hh>::v8;
template <typename Hh> using h16x4 = typename H16<Hh>::v4;
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ bf16x4 lds_tr4(const bf16* p) {
  typedef bf16x4 __attribute__((address_space(3))) * lds4;
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)p);
}
__device__ __forceinline__ f16x4 lds_tr4(const f16* p) {
  typedef s16x4 __attribute__((address_space(3))) * lds4;
  return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)p));
}
// two transposed reads `pitch4` elements (= 4 rows) apart, concatenated: the 8 k-values of one lane's MFMA operand
template <typename Hh> __device__ __forceinline__ h16x8<Hh> lds_tr8(const Hh* p, int pitch4) {
  const h16x4<Hh> lo = lds_tr4(p), hi = lds_tr4(p + pitch4);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// One MFMA operand fragment (A and B alike) from an LDS image `s` of row pitch `pitch` (elements): the 16 rows ("outs") starting at row0 over
// the k-slice starting at k0 -- 32 k-values of a 16-bit type (lane l holds X[row0 + (l&15)][k0 + 8*(l>>4) .. +7]), 4 of float (k0 + (l>>4)).
//  frag_kc: k-contiguous image [row][k], one 16-byte read
//  frag_oc: natural image [k][row] (V: keys x head dims; a TN operand), transposed on the way out of LDS: each 16-lane group g takes rows
//           k = 8g..8g+3 (+4) x 16 outs; lane 4q+p of the group addresses row q, outs 4p..4p+3 and receives out (l&15) of the 4 rows
template <typename Hh> __device__ __forceinline__ h16x8<Hh> frag_kc(const Hh* s, int pitch, int row0, int k0, int lane) {
  return *(const h16x8<Hh>*)(s + (row0 + (lane & 15)) * pitch + k0 + 8 * (lane >> 4));
}
template <typename Hh> __device__ __forceinline__ h16x8<Hh> frag_oc(const Hh* s, int pitch, int row0, int k0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  return lds_tr8(s + (k0 + 8 * g + q) * pitch + row0 + 4 * pp, 4 * pitch);
}
__device__ __forceinline__ float frag_kc(const float* s, int pitch, int row0, int k0, int lane) { return s[(row0 + (lane & 15)) * pitch + k0 + (lane >> 4)]; }
__device__ __forceinline__ float frag_oc(const float* s, int pitch, int row0, int k0, int lane) { return s[(k0 + (lane >> 4)) * pitch + row0 + (lane & 15)]; }

// Two-phase staging of global rows into LDS row images: stage_issue REQUESTS a thread's 16-byte chunks of an image into registers, stage_store puts
// them into LDS.  A caller issues every image of its prologue (and whatever else it reads first) before the first store, so the loads are in
// flight together and the workgroup waits for the slowest of them once.  (A loop that loads, stores and loads again waits for one L2 round trip per
// pass -- hipcc puts s_waitcnt vmcnt(0) in front of every LDS store of such a loop: ~2 us per trip in the step.)
// Chunk `id` of an image is row id / cpr, columns (id % cpr) * VE ...; a thread owns ids tid + it * nthr, it in [it0, it0 + NIT).  A chunk of a row
// at or beyond nvalid, or of a column at or beyond cvalid, is zeros and NO load is issued for it (such rows belong to the next sample or lie past
// the buffer; the zeros feed MFMA contractions); an id at or beyond nchunk touches nothing.  A caller bounds what is in flight (~16 chunks per lane)
// by the NIT it chooses and walks the rest of a large image in further batches (it0 += NIT).
template <typename T> struct RowVecT { typedef T type __attribute__((ext_vector_type(16 / sizeof(T)))); };
template <typename T> using rowvec = typename RowVecT<T>::type;
template <typename T> struct RowImg {
  T* s; int pitch;                 // LDS image and its row pitch (elements)
  const T* src; int ld;            // global rows: row r at src + r * ld
  int nvalid, cvalid;              // valid rows / valid columns (cvalid a multiple of the chunk width)
  int cpr, nchunk;                 // chunks per image row; chunks of the whole (padded) image
};
template <int NIT, typename T>
__device__ __forceinline__ void stage_issue(rowvec<T> (&reg)[NIT], const RowImg<T>& im, const int it0, const int tid, const int nthr) {
  constexpr int VE = 16 / sizeof(T);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int id = tid + (it0 + it) * nthr, r = id / im.cpr, c = (id - r * im.cpr) * VE;
#pragma unroll
    for (int e = 0; e < VE; ++e) reg[it][e] = (T)0.0f;
    if (id < im.nchunk && r < im.nvalid && c < im.cvalid) reg[it] = *(const rowvec<T>*)(im.src + c + __mul24(r, im.ld));      // (rows and row pitches are far below 2^23: a 24-bit multiply)
  }
}
template <int NIT, typename T>
__device__ __forceinline__ void stage_store(const rowvec<T> (&reg)[NIT], const RowImg<T>& im, const int it0, const int tid, const int nthr) {
  constexpr int VE = 16 / sizeof(T);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int id = tid + (it0 + it) * nthr, r = id / im.cpr, c = (id - r * im.cpr) * VE;
    if (id < im.nchunk) *(rowvec<T>*)(im.s + r * im.pitch + c) = reg[it];
  }
}

// Cross-lane reductions as DPP moves (VALU data-parallel primitives: quad permutes and row mirrors inside a 16-lane row), not
// __shfl_xor: hipcc lowers every __shfl_xor to ds_bpermute_b32, a round trip through the LDS crossbar (~100 cycles, each step of
// a butterfly waiting on the previous one) -- measured: the LayerNorm epilogue of the whole-encoder kernel spent 9.4 of its 10.3 us
// in 160 such shuffles.  The 16-lane butterfly below is bit-identical to the xor 1,2,4,8 shuffle sequence (after each step all
// lanes of a group hold the same value, and a + b == b + a).
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
#define DPP_QUAD_XOR1 0xB1         /* quad_perm [1,0,3,2] */
#define DPP_QUAD_XOR2 0x4E         /* quad_perm [2,3,0,1] */
#define DPP_ROW_HALF_MIRROR 0x141
#define DPP_ROW_MIRROR 0x140
__device__ __forceinline__ float row16_sum(float v) {      // every lane of a 16-lane row gets the row's sum
  v += dpp_mov<DPP_QUAD_XOR1>(v);
  v += dpp_mov<DPP_QUAD_XOR2>(v);
  v += dpp_mov<DPP_ROW_HALF_MIRROR>(v);
  v += dpp_mov<DPP_ROW_MIRROR>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_mov<DPP_QUAD_XOR1>(v));
  v = fmaxf(v, dpp_mov<DPP_QUAD_XOR2>(v));
  v = fmaxf(v, dpp_mov<DPP_ROW_HALF_MIRROR>(v));
  v = fmaxf(v, dpp_mov<DPP_ROW_MIRROR>(v));
  return v;
}
__device__ __forceinline__ float lane_bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ __forceinline__ float wave_sum(float v) {
  v = row16_sum(v);
  return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
  v = row16_max(v);
  return fmaxf(fmaxf(lane_bcast(v, 0), lane_bcast(v, 16)), fmaxf(lane_bcast(v, 32), lane_bcast(v, 48)));
}
__device__ __forceinline__ int wave_min_i(int v) {         // every lane gets the wave's minimum
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) v = min(v, __shfl_xor(v, d));
  return v;
}
// Ordered inclusive scan over the 64 lanes: lane l gets v_0 + ... + v_l (Hillis-Steele, 6 steps; every partial sum adds a contiguous run of
// lanes to the run right below it, so lower lanes always come first).  T = int or double.  Shuffles, not DPP: the users are one-wave latency-bound
// kernels that scan a 64-bit value a handful of times (csrc/loss.hip nav_act_kernel), and a DPP row shift moves 32 bits inside 16 lanes only.
template <typename T> __device__ __forceinline__ T wave_scan_sum(T v, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const T o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// exact (erf) GELU, as HF "gelu" / torch F.gelu default
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float dgelu_f(float x) {
  float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  float pdf = 0.39894228040143268f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// Counter-based dropout: keep(site, idx) is a pure function of (seed[0], seed[1], site, logical element index), so the
// forward kernel and the backward kernel regenerate the same mask without ever storing it.  `seed` lives in device
// memory (a replayed HIP graph sees whatever the host-side generator wrote there this step); `site` distinguishes the
// dropout modules of the network; idx is the row-major index in the LOGICAL tensor (no padding columns).
// One full-avalanche 32-bit finaliser (murmur3 fmix32) over (idx ^ ka) + kb.  (Round 2 started with a second, differently keyed mixing round behind
// it: the whole-encoder kernels hash ~33 k elements per sample and layer, and the second round cost 11 of the forward kernel's 305 us and ~30 us
// of the step for no measurable change in the mask statistics -- tests/test_dropout_gpu.py::test_mask_statistics_and_determinism.)
using DropDesc = magic_drop_desc;       // seed == nullptr or p <= 0: off
struct DropState { unsigned ka, kb, thr; float scale; bool on; };
__device__ __forceinline__ DropState drop_init(const DropDesc& d) {
  DropState s;
  s.on = d.seed != nullptr && d.p > 0.f;
  s.ka = 0; s.kb = 0; s.thr = 0; s.scale = 1.f;
  if (s.on) {
    s.ka = d.seed[0] ^ (d.site * 0x9E3779B1u);
    s.kb = d.seed[1] + d.site * 0x85EBCA77u;
    s.thr = (unsigned)((double)d.p * 4294967296.0);
    s.scale = 1.0f / (1.0f - d.p);
  }
  return s;
}
__device__ __forceinline__ float drop_mul(const DropState& s, unsigned idx) {   // 0 (dropped) or 1/(1-p) (kept)
  unsigned x = (idx ^ s.ka) + s.kb;            // both keys in front of ONE full-avalanche finaliser (murmur3 fmix32)
  x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
  return x >= s.thr ? s.scale : 0.f;
}
static inline bool drop_args_ok(const void* seed, float p) { return p >= 0.f && p < 1.f && (p == 0.f || seed != nullptr); }

// the device word every gradient-seeding loss kernel multiplies its gradient coefficient by (loss.hip magic_seed_scale; NULL: none)
const float* seed_scale_get();

static inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MAGIC_OK : MAGIC_ERR_LAUNCH;
}

// Panoramas per workgroup of the fusion backward and its grid -- the rows of its partial buffer (magic_pano_fuse_bwd_blocks) -- for both launches that
// run it: magic_pano_fuse_bwd (graphops.hip) and the fusion job of magic_node_in_bwd (rowops.hip)
#define PF_PB 2
static inline int pano_fuse_blocks(int N) { return (N + PF_PB - 1) / PF_PB; }

// dst_j[c] += sum_b part_j[b][c], b < nblk_j, c < H, in block order (reproducible): the finisher of the partial-row LayerNorm gradients of
// magic_rowbwd (csrc/encbwd.hip), as a standalone launch (magic_colsum_add) or as extra workgroups of magic_embed_in_bwd.  One workgroup per
// job; blockDim.x / H row groups take every (blockDim.x / H)-th block, LDS fold.  `red`: blockDim.x floats of LDS.
#define CSJ_MAX 96
struct ColsumJobs { const float* part[CSJ_MAX]; float* dst[CSJ_MAX]; int nblk[CSJ_MAX]; int n; };
__device__ __forceinline__ void colsum_body(const ColsumJobs& js, const int j, const int H, float* red) {
  const int t = threadIdx.x, c = t % H, grp = t / H, ngrp = blockDim.x / H;
  const float* part = js.part[j];
  const int nb = js.nblk[j];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (grp < ngrp) {
    int b = grp;
    for (; b + 3 * ngrp < nb; b += 4 * ngrp) {
      s0 += part[(long long)b * H + c]; s1 += part[(long long)(b + ngrp) * H + c];
      s2 += part[(long long)(b + 2 * ngrp) * H + c]; s3 += part[(long long)(b + 3 * ngrp) * H + c];
    }
    for (; b < nb; b += ngrp) s0 += part[(long long)b * H + c];
  }
  red[t] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (grp == 0) {
    float v = 0.f;
    for (int g2 = 0; g2 < ngrp; ++g2) v += red[g2 * H + c];
    js.dst[j][c] += v;
  }
}
