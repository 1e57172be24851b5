// The embedding-distillation terms of a step in ONE launch (magic_kd_emb): for each of n <= 8 problems
//   sp = round_T(s W^T + b)          [M, Hs] x [Ht, Hs]^T, fp32 accumulation, bias added in fp32 (magic_gemm's rounding point)
//   d  = float(sp) - float(t)        0 outside the device-side extents
//   loss += norm * sum w d^2         one atomic per workgroup
//   ds = round_T(2 coef norm w d)    stored for the deferred weight gradient
//   d_acc = round_T(float(d_acc) + ds W)   over the ROUNDED ds, fp32 accumulation, one rounding (magic_gemm's residual epilogue)
// which the three launches grouped magic_gemm -> magic_mse_multi -> grouped magic_gemm compute with sp and ds making a round trip through
// memory each.  A workgroup owns whole rows: it holds its problem's W [Ht = 256][Hs = 128] in LDS once -- the k-contiguous
// B operand of the first product and, read back with ds_read_b64_tr_b16, the natural [k][out] B operand of the second -- and walks its
// problem's 32-row tiles under it.  sp / ds of a tile live in one LDS image; no workgroup waits for another.  Both products run
// v_mfma_f32_16x16x32 with ascending k in one accumulator, as gemm_block does.
#include "common.hpp"

#define KDE_MAX 8
#define KDE_NT 512            // 8 waves: wave w owns rows 16 (w >> 2) .. +15 of the tile and a quarter of the columns
#define KDE_R 32              // rows per tile
#define KDE_HS 128
#define KDE_HT 256
#define KDE_WP (KDE_HS + 8)   // pitch of the W image (elements): 272 bytes, rows 4 banks apart
#define KDE_DP (KDE_HT + 8)   // pitch of the sp / ds image
#define KDE_OP (KDE_HS + 4)   // pitch of the fp32 image of the second product
#define KDE_BLOCKS 256        // about one workgroup per CU (the reason above MSE_BLOCKS in loss.hip; and one W image per workgroup)

struct KdEmbProb {
  const void* s; const void* t; const void* W; const float* b; const float* w; const float* coef_dev; float* loss; void* ds; void* dacc;
  const int* valid_dev; const float* norm_dev;
  int M, rpb, rpw; long long outer, inner; float norm, coef;
};
struct KdEmb { KdEmbProb p[KDE_MAX]; int start[KDE_MAX + 1]; int n; const float* ss; };

static constexpr size_t kde_lds_bytes() {
  return (size_t)KDE_HT * KDE_WP * 2 + (size_t)KDE_R * KDE_DP * 2 + (size_t)KDE_R * KDE_OP * 4 + (KDE_NT / 64) * 4;
}

template <typename Hh>
__global__ __launch_bounds__(KDE_NT) void kd_emb_kernel(KdEmb kk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kde_smem[];
  Hh* const sW = (Hh*)kde_smem;                                         // [Ht][WP]
  Hh* const sD = sW + KDE_HT * KDE_WP;                                  // [R][DP]: sp, then ds in place
  float* const sO = (float*)(sD + KDE_R * KDE_DP);                      // [R][OP]
  float* const red = sO + KDE_R * KDE_OP;
  typedef h16x8<Hh> v8;

  int pi = 0;
  while (pi + 1 < kk.n && (int)blockIdx.x >= kk.start[pi + 1]) ++pi;
  const KdEmbProb& p = kk.p[pi];
  const int bid = blockIdx.x - kk.start[pi], nblk = kk.start[pi + 1] - kk.start[pi];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, rh = wid >> 2, cq = wid & 3;
  const int M = p.M, ntiles = (M + KDE_R - 1) / KDE_R;
  const Hh* __restrict__ S = (const Hh*)p.s;
  const Hh* __restrict__ Tt = (const Hh*)p.t;
  Hh* __restrict__ DS = (Hh*)p.ds;
  Hh* __restrict__ DA = (Hh*)p.dacc;

  // the weight, once per workgroup
  {
    const Hh* __restrict__ W = (const Hh*)p.W;
#pragma unroll
    for (int i = 0; i < KDE_HT * (KDE_HS / 8) / KDE_NT; ++i) {
      const int c = tid + KDE_NT * i, row = c >> 4, cv = c & 15;
      *(v8*)(sW + row * KDE_WP + cv * 8) = *(const v8*)(W + row * KDE_HS + cv * 8);
    }
  }
  float coef = p.coef;
  if (p.coef_dev) coef *= p.coef_dev[0];
  if (kk.ss) coef *= kk.ss[0];
  const long long vo = p.valid_dev ? p.valid_dev[0] : p.outer, vi = p.valid_dev ? p.valid_dev[1] : p.inner;
  const float nrm = p.norm * (p.norm_dev ? p.norm_dev[0] : 1.f);
  const float c2 = 2.f * coef * nrm;
  float bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bv[j] = p.b ? p.b[cq * 64 + j * 16 + (lane & 15)] : 0.f;

  // registers of a tile's global operands: the A fragments of the first product (lane l: row l & 15, k = 32 ks + 8 (l >> 4) ..), two 8-element
  // chunks of t and one of d_acc per thread; the next tile's are in flight while this one is computed
  v8 a_cur[4], t_cur[2], r_cur;
  auto zero8 = [] { v8 z; for (int e = 0; e < 8; ++e) z[e] = (Hh)0.0f; return z; };
  auto fetch = [&](int tile, v8 (&a)[4], v8 (&tv)[2], v8& rv) {
    const int r0 = tile * KDE_R;
    const int ar = r0 + 16 * rh + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a[ks] = (tile < ntiles && ar < M) ? *(const v8*)(S + (long long)ar * KDE_HS + ks * 32 + 8 * (lane >> 4)) : zero8();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = tid + KDE_NT * u, row = r0 + (c >> 5);
      tv[u] = (tile < ntiles && row < M) ? *(const v8*)(Tt + (long long)row * KDE_HT + (c & 31) * 8) : zero8();
    }
    const int row = r0 + (tid >> 4);
    rv = (DA && tile < ntiles && row < M) ? *(const v8*)(DA + (long long)row * KDE_HS + (tid & 15) * 8) : zero8();
  };
  fetch(bid, a_cur, t_cur, r_cur);
  float lacc = 0.f;
  __syncthreads();                       // W image complete

  for (int tile = bid; tile < ntiles; tile += nblk) {
    const int r0 = tile * KDE_R;
    v8 a_nx[4], t_nx[2], r_nx;
    fetch(tile + nblk, a_nx, t_nx, r_nx);
    // ---- sp = round(s W^T + b): wave = 16 rows x 64 columns
    {
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        v8 b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *(const v8*)(sW + (cq * 64 + j * 16 + (lane & 15)) * KDE_WP + ks * 32 + 8 * (lane >> 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = mfma16(a_cur[ks], b[j], acc[j]);
      }
      // C/D map of the 16x16 product: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sD[(16 * rh + 4 * (lane >> 4) + r) * KDE_DP + cq * 64 + j * 16 + (lane & 15)] = from_f<Hh>(acc[j][r] * 1.f + bv[j]);
    }
    __syncthreads();
    // ---- d, the loss, ds (to memory and, in place of sp, to LDS): thread = two 8-element chunks
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = tid + KDE_NT * u, lr = c >> 5, col = (c & 31) * 8, row = r0 + lr;
      Hh* q = sD + lr * KDE_DP + col;
      v8 g = zero8();
      if (row < M) {
        const v8 sv = *(const v8*)q;
        const long long o = row / p.rpb;
        const long long rr = (long long)(row - o * p.rpb) * KDE_HT + col;
        const float wv = p.w ? p.w[o / p.rpw] : 1.f;
        float d[8], a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { d[e] = (o < vo && rr + e < vi) ? (float)sv[e] - (float)t_cur[u][e] : 0.f; a += d[e] * d[e]; }
        lacc += wv * a;
        const float cw = c2 * wv;
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = (Hh)(cw * d[e]);
        if (DS) *(v8*)(DS + (long long)row * KDE_HT + col) = g;
      }
      *(v8*)q = g;
    }
    if (DA) {                       // (block-uniform)
      __syncthreads();
      // ---- ds W: wave = 16 rows x 32 columns, contraction over the teacher width; B = the W image read along its rows' index
      {
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
        const int g4 = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;
#pragma unroll
        for (int ks = 0; ks < KDE_HT / 32; ++ks) {
          const v8 a = *(const v8*)(sD + (16 * rh + (lane & 15)) * KDE_DP + ks * 32 + 8 * g4);
          v8 b[2];
#pragma unroll
          for (int j = 0; j < 2; ++j) b[j] = lds_tr8(sW + (ks * 32 + 8 * g4 + q4) * KDE_WP + cq * 32 + j * 16 + 4 * pp, 4 * KDE_WP);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[j] = mfma16(a, b[j], acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) sO[(16 * rh + 4 * g4 + r) * KDE_OP + cq * 32 + j * 16 + (lane & 15)] = acc[j][r];
      }
      __syncthreads();
      // ---- d_acc = round(float(d_acc) + ds W): thread = one 8-element chunk
      {
        const int lr = tid >> 4, col = (tid & 15) * 8, row = r0 + lr;
        if (row < M) {
          const f32x4 o0 = *(const f32x4*)(sO + lr * KDE_OP + col), o1 = *(const f32x4*)(sO + lr * KDE_OP + col + 4);
          v8 out;
#pragma unroll
          for (int e = 0; e < 4; ++e) { out[e] = (Hh)(o0[e] + (float)r_cur[e]); out[4 + e] = (Hh)(o1[e] + (float)r_cur[4 + e]); }
          *(v8*)(DA + (long long)row * KDE_HS + col) = out;
        }
      }
    } else {
      __syncthreads();              // the next tile's sp overwrites the image this tile's chunks were read from
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) a_cur[ks] = a_nx[ks];
    t_cur[0] = t_nx[0]; t_cur[1] = t_nx[1]; r_cur = r_nx;
  }
  lacc = wave_sum(lacc);
  if (lane == 0) red[wid] = lacc;
  __syncthreads();
  if (tid == 0 && p.loss) {
    float v = 0.f;
    for (int w = 0; w < KDE_NT / 64; ++w) v += red[w];
    atomicAdd(p.loss, v * nrm);
  }
}

extern "C" int magic_kd_emb_supported(int dtype, int Hs, int Ht) { return (dtype_is16(dtype) && Hs == KDE_HS && Ht == KDE_HT) ? 1 : 0; }

extern "C" int magic_kd_emb(int dtype, int n, const magic_mse_desc* d, int Hs, int Ht, const int* M, const void* const* W, const float* const* b,
                            void* const* d_acc, void* stream) {
  if (n < 1 || n > KDE_MAX || !d || !M || !W || !b) return MAGIC_ERR_ARG;
  if (!magic_kd_emb_supported(dtype, Hs, Ht)) return MAGIC_ERR_ARG;
  KdEmb kk;
  kk.n = n;
  kk.ss = seed_scale_get();
  long long all = 0;
  for (int i = 0; i < n; ++i) {
    const magic_mse_desc& q = d[i];
    void* da = d_acc ? d_acc[i] : nullptr;
    if (M[i] <= 0 || q.outer <= 0 || q.inner <= 0 || q.inner % Ht || !q.s || !q.t || !W[i] || !b[i]) return MAGIC_ERR_ARG;
    const long long rpb = q.inner / Ht;
    if (q.outer * rpb != M[i] || q.t_stride != q.inner || q.s_stride != rpb * Hs || (q.w && q.rows_per_w <= 0)) return MAGIC_ERR_ARG;
    if (q.g_f32 || q.accumulate || q.valid_mod || (q.ds && q.g_stride != q.inner)) return MAGIC_ERR_ARG;
    if ((q.ds == nullptr) != (da == nullptr)) return MAGIC_ERR_ARG;          // the training form writes both, the loss-only form neither
    if (((uintptr_t)q.s | (uintptr_t)q.t | (uintptr_t)W[i] | (uintptr_t)q.ds | (uintptr_t)da) & 15) return MAGIC_ERR_ARG;
    KdEmbProb& p = kk.p[i];
    p.s = q.s; p.t = q.t; p.W = W[i]; p.b = b[i]; p.w = q.w; p.coef_dev = q.coef_dev; p.loss = q.loss; p.ds = q.ds; p.dacc = da;
    p.valid_dev = q.valid_dev; p.norm_dev = q.norm_dev;
    p.M = M[i]; p.rpb = (int)rpb; p.rpw = q.w ? (int)q.rows_per_w : 1; p.outer = q.outer; p.inner = q.inner; p.norm = q.norm; p.coef = q.coef;
    all += M[i];
  }
  // workgroups shared out among the problems by rows, at least one and at most one per tile each
  int total = 0;
  for (int i = 0; i < n; ++i) {
    const long long tiles = (M[i] + KDE_R - 1) / KDE_R;
    long long blocks = ((long long)M[i] * KDE_BLOCKS + all - 1) / all;
    if (blocks > tiles) blocks = tiles;
    if (blocks < 1) blocks = 1;
    blocks = (tiles + (tiles + blocks - 1) / blocks - 1) / ((tiles + blocks - 1) / blocks);      // the fewest workgroups with that many tiles each
    kk.start[i] = total;
    total += (int)blocks;
  }
  for (int i = n; i <= KDE_MAX; ++i) kk.start[i] = total;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)kd_emb_kernel<bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kde_lds_bytes());
    (void)hipFuncSetAttribute((const void*)kd_emb_kernel<f16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kde_lds_bytes());
    attr = true;
  }
  dim3 grid(total), block(KDE_NT);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_H(dtype, hipLaunchKernelGGL(kd_emb_kernel<TY>, grid, block, kde_lds_bytes(), st, kk));
  return launch_status();
}
