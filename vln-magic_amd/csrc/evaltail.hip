// The validation pass on the device: per-row losses and hits of the four proxy tasks and their accumulation, so that a
// validation batch ends in no host read (the driver's validate_* loops, pretrain_src/train_r2r_magic.py:441-587, end every batch in 3-7 .item()s).
//
// magic_mlm_eval -- the MLM head's vocabulary projection, cross-entropy and argmax WITHOUT the logits in memory, in two launches:
//   1. one workgroup per vocabulary slab (64 KB of W: 256 rows at H = 128, 128 rows at H = 256), the slab staged in LDS once, so every W
//      element leaves HBM once; the workgroup walks all masked rows in 64-row tiles (v_mfma_f32_16x16x32, fp32 accumulation, ascending k,
//      bias added in fp32) and stores, per (slab, row), one 16-byte partial {max, sum exp(x - max), argmax index, x[label] if it lies here};
//   2. one wave per row folds the row's partials in slab order and writes loss_row = log sum + max - x[label] and hit_row.
// No workgroup waits for another, no atomics; every reduction runs in a fixed order, so two calls give the same bits.
#include "common.hpp"
#include <math.h>

#define MEV_NT 512            // 8 waves: wave w owns rows 16 (w >> 1) .. +15 of the tile and half (w & 1) of the slab's columns
#define MEV_R 64              // rows per tile
#define MEV_SLAB_BYTES 65536  // of W per workgroup

template <int CTRL> __device__ __forceinline__ int dpp_movi(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int row16_min(int v) {          // every lane of a 16-lane row gets the row's minimum
  v = min(v, dpp_movi<DPP_QUAD_XOR1>(v));
  v = min(v, dpp_movi<DPP_QUAD_XOR2>(v));
  v = min(v, dpp_movi<DPP_ROW_HALF_MIRROR>(v));
  v = min(v, dpp_movi<DPP_ROW_MIRROR>(v));
  return v;
}

static inline int mev_slab_rows(int H) { return MEV_SLAB_BYTES / (2 * H); }
static inline int mev_slabs(int V, int H) { return (V + mev_slab_rows(H) - 1) / mev_slab_rows(H); }
template <int H> constexpr size_t mev_lds_bytes() { return (size_t)(MEV_SLAB_BYTES / (2 * H)) * (H + 8) * 2 + (size_t)MEV_R * 2 * sizeof(f32x4); }

template <typename Hh, int H>
__global__ __launch_bounds__(MEV_NT) void mlm_eval_slab_kernel(int nm, int V, const Hh* __restrict__ hm, const Hh* __restrict__ W, int ldw,
                                                               const float* __restrict__ bias, const int* __restrict__ labels, f32x4* __restrict__ ws) {
  constexpr int SR = MEV_SLAB_BYTES / (2 * H);      // slab rows (vocabulary entries)
  constexpr int WP = H + 8;                         // pitch of the W image (elements): rows 4 banks apart
  constexpr int NJ = SR / 32;                       // 16-column blocks per wave
  constexpr int KS = H / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char mev_smem[];
  Hh* const sW = (Hh*)mev_smem;                                           // [SR][WP]
  f32x4* const sP = (f32x4*)(sW + SR * WP);                               // [R][2]: the two column halves' partials of a tile
  typedef h16x8<Hh> v8;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, rg = wid >> 1, half = wid & 1;
  const int slab = blockIdx.x, c0 = slab * SR;
  const int ntiles = (nm + MEV_R - 1) / MEV_R;
  auto zero8 = [] { v8 z; for (int e = 0; e < 8; ++e) z[e] = (Hh)0.0f; return z; };

  // the slab, once per workgroup; vocabulary rows past V are zeros (their logits are masked below)
#pragma unroll
  for (int i = 0; i < SR * (H / 8) / MEV_NT; ++i) {
    const int c = tid + MEV_NT * i, row = c / (H / 8), cv = c % (H / 8);
    *(v8*)(sW + row * WP + cv * 8) = (c0 + row < V) ? *(const v8*)(W + (long long)(c0 + row) * ldw + cv * 8) : zero8();
  }
  float bv[NJ];
  int col[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    col[j] = c0 + half * (SR / 2) + j * 16 + (lane & 15);
    bv[j] = col[j] < V ? bias[col[j]] : 0.f;
  }
  // A fragments straight from memory (lane l: row l & 15, k = 32 ks + 8 (l >> 4) ..); the next tile's are in flight while this one is computed
  v8 a_cur[KS];
  auto fetch = [&](int tile, v8 (&a)[KS]) {
    const int ar = tile * MEV_R + 16 * rg + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a[ks] = (tile < ntiles && ar < nm) ? *(const v8*)(hm + (long long)ar * H + ks * 32 + 8 * (lane >> 4)) : zero8();
  };
  fetch(0, a_cur);
  __syncthreads();                       // W image complete

  for (int tile = 0; tile < ntiles; ++tile) {
    const int r0 = tile * MEV_R;
    v8 a_nx[KS];
    fetch(tile + 1, a_nx);
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const v8 b = *(const v8*)(sW + (half * (SR / 2) + j * 16 + (lane & 15)) * WP + ks * 32 + 8 * (lane >> 4));
        acc[j] = mfma16(a_cur[ks], b, acc[j]);
      }
    }
    // C/D map of the 16x16 product: col = lane & 15, row = 4 (lane >> 4) + reg.  Per row: this lane's NJ columns, then the 16 lanes of its row group
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 16 * rg + 4 * (lane >> 4) + r, row = r0 + lr;
      const int lbl = row < nm ? labels[row] : -1;
      float v[NJ], m = -INFINITY, xl = 0.f;
      int mi = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        v[j] = col[j] < V ? acc[j][r] + bv[j] : -INFINITY;
        if (v[j] > m) { m = v[j]; mi = col[j]; }                 // ascending columns: the lowest index among equals stays
        if (col[j] == lbl) xl = v[j];
      }
      const float M = row16_max(m);
      const int I = row16_min(m == M ? mi : 0x7fffffff);
      const float Ms = M == -INFINITY ? 0.f : M;                 // a half that lies past V altogether (the last slab): S = 0, and the merge drops it
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) s += __expf(v[j] - Ms);       // exp(-inf) = 0: masked columns
      const float S = row16_sum(s);
      const float X = row16_sum(xl);                             // at most one lane holds the label's column: the sum is exact
      if ((lane & 15) == 0) sP[lr * 2 + half] = (f32x4){M, S, __int_as_float(I), X};
    }
    __syncthreads();
    if (tid < MEV_R && r0 + tid < nm) {                          // the two halves in column order
      const f32x4 p0 = sP[tid * 2], p1 = sP[tid * 2 + 1];
      const float M = fmaxf(p0[0], p1[0]);
      f32x4 o;
      o[0] = M;
      o[1] = p0[1] * __expf(p0[0] - M) + p1[1] * __expf(p1[0] - M);
      o[2] = p1[0] > p0[0] ? p1[2] : p0[2];
      o[3] = p0[3] + p1[3];
      ws[(long long)slab * nm + r0 + tid] = o;
    }
    __syncthreads();                     // the next tile's partials overwrite sP
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) a_cur[ks] = a_nx[ks];
  }
}

// one wave per row: lane l folds the contiguous run of slabs [l c, (l + 1) c) in ascending order, then the lanes are folded in ascending order
__global__ __launch_bounds__(256) void mlm_eval_merge_kernel(int nm, int nslab, const f32x4* __restrict__ ws, const int* __restrict__ labels, int ignore_index,
                                                             float* __restrict__ loss_row, int* __restrict__ hit_row) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nm) return;                 // (wave-uniform)
  const int chunk = (nslab + 63) / 64, k0 = lane * chunk, k1 = min(nslab, k0 + chunk);
  float m = -INFINITY;
  int mi = 0x7fffffff;
  for (int k = k0; k < k1; ++k) {
    const f32x4 p = ws[(long long)k * nm + row];
    if (p[0] > m) { m = p[0]; mi = __float_as_int(p[2]); }
  }
  float M = m;
  for (int o = 32; o; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
  int I = m == M ? mi : 0x7fffffff;
  for (int o = 32; o; o >>= 1) I = min(I, __shfl_xor(I, o));
  float s = 0.f, x = 0.f;
  for (int k = k0; k < k1; ++k) {
    const f32x4 p = ws[(long long)k * nm + row];
    s += p[1] * expf(p[0] - M);
    x += p[3];
  }
  float S = 0.f, X = 0.f;
  for (int l = 0; l < 64; ++l) { S += lane_bcast(s, l); X += lane_bcast(x, l); }
  if (lane == 0) {
    const int lbl = labels[row];
    const bool ign = lbl == ignore_index;
    loss_row[row] = ign ? 0.f : logf(S) + M - X;
    hit_row[row] = ign ? -1 : (I == lbl ? 1 : 0);
  }
}

extern "C" int magic_mlm_eval_supported(int dtype, int H) { return (dtype_is16(dtype) && (H == 128 || H == 256)) ? 1 : 0; }

extern "C" int magic_mlm_eval_ws_need(int dtype, int nm, int V, int H) {
  if (!magic_mlm_eval_supported(dtype, H) || nm < 1 || V < 1) return MAGIC_ERR_ARG;
  const long long need = (long long)mev_slabs(V, H) * nm * 16;
  return need > 0x7fffffffLL ? MAGIC_ERR_ARG : (int)need;
}

template <typename Hh, int H>
static void mev_launch(int nm, int V, const void* hm, const void* W, int ldw, const float* bias, const int* labels, void* ws, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)mlm_eval_slab_kernel<Hh, H>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mev_lds_bytes<H>());
    attr = true;
  }
  hipLaunchKernelGGL((mlm_eval_slab_kernel<Hh, H>), dim3(mev_slabs(V, H)), dim3(MEV_NT), mev_lds_bytes<H>(), st, nm, V, (const Hh*)hm, (const Hh*)W, ldw,
                     bias, labels, (f32x4*)ws);
}

extern "C" int magic_mlm_eval(int dtype, int nm, int V, int H, const void* hm, const void* W, int ldw, const float* bias,
                              const int* labels, int ignore_index, void* ws, float* loss_row, int* hit_row, void* stream) {
  if (!magic_mlm_eval_supported(dtype, H) || nm < 1 || V < 1 || ldw < H || (ldw & 7)) return MAGIC_ERR_ARG;
  if (!hm || !W || !bias || !labels || !ws || !loss_row || !hit_row) return MAGIC_ERR_ARG;
  if (((uintptr_t)hm | (uintptr_t)W | (uintptr_t)ws) & 15) return MAGIC_ERR_ARG;
  if (magic_mlm_eval_ws_need(dtype, nm, V, H) < 0) return MAGIC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_H(dtype, DISPATCH_I2(H, 128, 256, (mev_launch<TY, IV>(nm, V, hm, W, ldw, bias, labels, ws, st))));
  if (launch_status() != MAGIC_OK) return MAGIC_ERR_LAUNCH;
  hipLaunchKernelGGL(mlm_eval_merge_kernel, dim3((nm + 3) / 4), dim3(256), 0, st, nm, mev_slabs(V, H), (const f32x4*)ws, labels, ignore_index, loss_row, hit_row);
  return launch_status();
}

// ---- row metrics of logits that are in memory (validate_sap :513-518, validate_mrc :484-486; the MLM fallback) ----------------------------------
// a workgroup's (value, lowest index) maximum and sums, folded in a fixed order: lanes by butterfly, waves in ascending order
struct ArgMax { float v; int i; };
__device__ __forceinline__ ArgMax argmax_join(ArgMax a, ArgMax b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ ArgMax block_argmax(ArgMax a, ArgMax* red) {
  for (int o = 32; o; o >>= 1) { ArgMax b; b.v = __shfl_xor(a.v, o); b.i = __shfl_xor(a.i, o); a = argmax_join(a, b); }
  __syncthreads();                       // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  ArgMax r = red[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = argmax_join(r, red[w]);
  return r;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) r += red[w];
  return r;
}

template <typename T>
__global__ __launch_bounds__(256) void eval_rows_kernel(int N, const T* __restrict__ logits, int ld, const int* __restrict__ labels, int ignore_index,
                                                        const float* __restrict__ targets, int ldt, float* __restrict__ loss_row, int* __restrict__ hit_row) {
  __shared__ ArgMax red_a[4];
  __shared__ float red_f[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* x = logits + (long long)row * ld;
  ArgMax a = {-INFINITY, 0x7fffffff};
  for (int j = tid; j < N; j += 256) { const float v = to_f(x[j]); if (v > a.v) { a.v = v; a.i = j; } }
  a = block_argmax(a, red_a);
  float s = 0.f;
  for (int j = tid; j < N; j += 256) s += expf(to_f(x[j]) - a.v);
  const float lse = logf(block_sum(s, red_f)) + a.v;
  if (labels) {
    const int lbl = labels[row];
    if (tid == 0) {
      const bool ign = lbl == ignore_index || lbl < 0 || lbl >= N;
      loss_row[row] = ign ? 0.f : lse - to_f(x[ign ? 0 : lbl]);
      hit_row[row] = lbl == ignore_index ? -1 : (a.i == lbl ? 1 : 0);
    }
    return;
  }
  // soft targets: sum_j t_j (log t_j - log p_j) over t_j > 0 = sum t (log t - x) + lse sum t
  const float* t = targets + (long long)row * ldt;
  ArgMax ta = {-INFINITY, 0x7fffffff};
  float st = 0.f, sl = 0.f;
  for (int j = tid; j < N; j += 256) {
    const float tv = t[j];
    if (tv > ta.v) { ta.v = tv; ta.i = j; }
    if (tv > 0.f) { st += tv; sl += tv * (logf(tv) - to_f(x[j])); }
  }
  ta = block_argmax(ta, red_a);
  st = block_sum(st, red_f);
  sl = block_sum(sl, red_f);
  if (tid == 0) {
    const bool empty = !(st > 0.f);      // a bucket-padded row: no target mass
    loss_row[row] = empty ? 0.f : sl + lse * st;
    hit_row[row] = empty ? -1 : (a.i == ta.i ? 1 : 0);
  }
}

extern "C" int magic_eval_rows(int dtype, int M, int N, const void* logits, int ld, const int* labels, int ignore_index,
                               const float* targets, int ldt, float* loss_row, int* hit_row, void* stream) {
  if (!dtype_ok(dtype) || M <= 0 || N <= 0 || ld < N || !logits || !loss_row || !hit_row) return MAGIC_ERR_ARG;
  if ((labels == nullptr) == (targets == nullptr) || (targets && ldt < N)) return MAGIC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(eval_rows_kernel<TY>, dim3(M), dim3(256), 0, st, N, (const TY*)logits, ld, labels, ignore_index, targets, ldt, loss_row, hit_row));
  return launch_status();
}

// ---- one contrastive term of validate_cfp (:548-568): sim = a txt^T / temperature in fp32, one workgroup ----------------------------------------
#define CFE_B 64
template <typename T>
__global__ __launch_bounds__(256) void cfp_eval_kernel(int B, int H, const T* __restrict__ a, const T* __restrict__ txt, float inv_t,
                                                       float* __restrict__ loss_row, int* __restrict__ hit_row) {
  __shared__ float sim[CFE_B * (CFE_B + 1)];
  __shared__ float ce[2 * CFE_B];
  __shared__ int am[CFE_B];
  const int tid = threadIdx.x;
  for (int p = tid; p < B * B; p += 256) {
    const int r = p / B, j = p % B;
    float d = 0.f;
    for (int k = 0; k < H; ++k) d = fmaf(to_f(a[r * H + k]), to_f(txt[j * H + k]), d);
    sim[r * (CFE_B + 1) + j] = d * inv_t;
  }
  __syncthreads();
  if (tid < 2 * B) {                     // threads [0, B): row r against its columns; [B, 2B): column r against its rows
    const int r = tid % B, sr = tid < B ? 1 : CFE_B + 1, base = tid < B ? r * (CFE_B + 1) : r;
    float m = -INFINITY, s = 0.f;
    int mi = 0;
    for (int j = 0; j < B; ++j) { const float v = sim[base + j * sr]; if (v > m) { m = v; mi = j; } }
    for (int j = 0; j < B; ++j) s += expf(sim[base + j * sr] - m);
    ce[tid < B ? r : CFE_B + r] = logf(s) + m - sim[r * (CFE_B + 1) + r];
    if (tid < B) am[r] = mi;
  }
  __syncthreads();
  if (tid < B) {
    loss_row[tid] = 0.5f * (ce[tid] + ce[CFE_B + tid]);
    hit_row[tid] = am[tid] == tid ? 1 : 0;
  }
}

extern "C" int magic_cfp_eval(int dtype, int B, int H, const void* a, const void* txt, float temperature, float* loss_row, int* hit_row, void* stream) {
  if (!dtype_ok(dtype) || B <= 0 || B > CFE_B || H <= 0 || H > 256 || (H & 7) || !a || !txt || !loss_row || !hit_row || temperature <= 0.f) return MAGIC_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(cfp_eval_kernel<TY>, dim3(1), dim3(256), 0, st, B, H, (const TY*)a, (const TY*)txt, 1.f / temperature, loss_row, hit_row));
  return launch_status();
}

// ---- the accumulator block: double loss[4]; long long hits[4]; long long rows[4] (96 bytes, zeroed by the host) -----------------------------------
// one workgroup; thread t takes rows t, t + 256, ... in ascending order, the 256 threads are folded in ascending order by thread 0
__global__ __launch_bounds__(256) void eval_accum_kernel(int M, const float* __restrict__ loss_row, const int* __restrict__ hit_row, double* acc, int slot) {
  __shared__ double sl[256];
  __shared__ int sh[256], sr[256];
  const int tid = threadIdx.x;
  double l = 0.0;
  int h = 0, r = 0;
  for (int i = tid; i < M; i += 256) {
    const int hv = hit_row[i];
    if (hv >= 0) { l += (double)loss_row[i]; r += 1; h += hv == 1; }
  }
  sl[tid] = l; sh[tid] = h; sr[tid] = r;
  __syncthreads();
  if (tid == 0) {
    double L = 0.0;
    long long Hh = 0, R = 0;
    for (int t = 0; t < 256; ++t) { L += sl[t]; Hh += sh[t]; R += sr[t]; }
    long long* cnt = (long long*)(acc + 4);
    acc[slot] += L;
    cnt[slot] += Hh;
    cnt[4 + slot] += R;
  }
}

extern "C" int magic_eval_accum(int M, const float* loss_row, const int* hit_row, void* acc, int slot, void* stream) {
  if (M <= 0 || !loss_row || !hit_row || !acc || slot < 0 || slot > 3 || ((uintptr_t)acc & 7)) return MAGIC_ERR_ARG;
  hipLaunchKernelGGL(eval_accum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, M, loss_row, hit_row, (double*)acc, slot);
  return launch_status();
}
