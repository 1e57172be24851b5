// The navigator's optimizers on the flat buffers: torch.optim.SGD / RMSprop / Adam / AdamW as `--optim sgd | rms | adam | adamW` builds them
// (map_nav_src/r2r/parser.py:74-77, agent_base.py:124-139: optimizer(self.vln_bert.parameters(), lr=args.lr)), the clip at 40 in front of every
// step (agent_base.py:273-279) and the cosine schedule of --use_lr_sch (agent_base.py:24-32, :144-149, :282-289), as TWO launches per step over
// the whole model: the gradient norm (which also advances the schedule on the device) and one update launch.  optim.hip's kernels are not
// touched: magic_adamw / magic_sumsq / magic_sched_step keep their arithmetic bit for bit.
//
// Device words of one optimizer (the host allocates them once; no host scalar depends on a step count, so a step can be captured and replayed):
//   step[3]  int    [0] = k, the lr step: advances on every step, skipped or not; [1] = t, the state step (Adam's bias correction, torch's
//                   state['step']): taken back by the update launch when it skips; [2] = which of the two norm words this step accumulates into
//   words[4] float  [0] = lr_k, [1] = lr_k / (1 - b1^t), [2] = sqrt(1 - b2^t) (the last two for Adam / AdamW only), [3] = step[2] as this step saw it
//   ss[2]    float  the sum of squares of the gradient, alternating: the update launch of a step zeroes the word the NEXT step accumulates into.
//                   It cannot zero the word it reads: its other blocks may not have read it yet, and a block that starts late would see a norm
//                   of 0 -- so the word a step reads is zeroed one step later, by a launch in which nobody reads it.  For the same reason the two
//                   launches take `which word` from different places: the norm launch from step[2], which only the update launch writes, the
//                   update launch from words[3], which only the norm launch writes.
#include "common.hpp"

enum { RULE_SGD = 0, RULE_RMSPROP = 1, RULE_ADAM = 2, RULE_ADAMW = 3 };
enum { SCHED_CONST = 0, SCHED_COSINE = 1 };

struct FlatSched { int* step; int kind; float lr0, eta_min; int warmup, t_max, rule; float b1, b2; float* words; };

// constant: lr_k = lr0.  cosine(T, eta_min, W): k < W: lr0 (k + 1) / W (the reference's WarmUpLR.get_lr, agent_base.py:24-32); otherwise
// eta_min + (lr0 - eta_min) (1 + cos(pi (k - W) / T)) / 2, CosineAnnealingLR's closed form (agent_base.py:144-149).  In double, as sched_advance.
__device__ __forceinline__ void flat_sched_advance(const FlatSched& a, int slot) {
  const int k = a.step[0];
  a.step[0] = k + 1;
  const int t = a.step[1] + 1;
  a.step[1] = t;
  double lr = (double)a.lr0;
  if (a.kind == SCHED_COSINE) {
    if (k < a.warmup) lr = (double)a.lr0 * (double)(k + 1) / (double)a.warmup;
    else lr = (double)a.eta_min + ((double)a.lr0 - (double)a.eta_min) * (1.0 + cos(3.14159265358979323846 * (double)(k - a.warmup) / (double)a.t_max)) * 0.5;
  }
  a.words[0] = (float)lr;
  if (a.rule == RULE_ADAM || a.rule == RULE_ADAMW) {
    a.words[1] = (float)(lr / (1.0 - pow((double)a.b1, (double)t)));
    a.words[2] = (float)sqrt(1.0 - pow((double)a.b2, (double)t));
  }
  a.words[3] = (float)slot;
}

// sumsq_kernel's loads and block reduction (optim.hip), one atomic per block onto ss[step[2]], a word an earlier update launch (or the constructor)
// zeroed; ss == nullptr: one block that only advances the schedule.  vec == 0: g is not 16-byte aligned, every element goes through the scalar loop.
__global__ __launch_bounds__(1024) void flat_sumsq_sched_kernel(long long n, const float* __restrict__ g, float* ss, FlatSched sa, int vec) {
  __shared__ float red[16];
  const int slot = sa.step[2] & 1;          // (written by update launches only: the same value in every block of this launch)
  if (blockIdx.x == 0 && threadIdx.x == 0) flat_sched_advance(sa, slot);
  if (!ss) return;
  float s = 0.f;
  const long long n4 = vec ? n >> 2 : 0, stride = (long long)gridDim.x * 1024;
  for (long long i = (long long)blockIdx.x * 1024 + threadIdx.x; i < n4; i += 4 * stride) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (i + u * stride < n4) ? ((const float4*)g)[i + u * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 4; ++u) s += v[u].x * v[u].x + v[u].y * v[u].y + v[u].z * v[u].z + v[u].w * v[u].w;
  }
  for (long long i = (n4 << 2) + (long long)blockIdx.x * 1024 + threadIdx.x; i < n; i += stride) { const float v = g[i]; s += v * v; }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < 16; ++w) t += red[w];
    atomicAdd(ss + slot, t);
  }
}

struct FlatUpd {
  long long n, n_decay;
  float *p, *g, *m, *v;
  void* shadow;
  float a1, b2, eps, wd, mu;              // a1: RMSprop's alpha | Adam's beta1
  float* ss;                              // the two norm words, or nullptr
  float max_norm, gscale;
  const float* words;
  int zero_g;
  unsigned* overflow;
  int* step;
};
struct FlatScal { float c, lr, lr_bc1, sq_bc2, a1, b2, eps, wd, mu; };

// one element, fp32, torch.optim's order of operations for the rule (torch/optim/{sgd,rmsprop,adam}.py, the single-tensor forms)
template <int RULE>
__device__ __forceinline__ void flat_update1(float& p, float g, float& m, float& v, bool dec, const FlatScal& s) {
  g *= s.c;
  if (RULE != RULE_ADAMW && dec) g += s.wd * p;                 // the coupled L2 term of SGD / RMSprop / Adam
  if (RULE == RULE_SGD) {
    if (s.mu > 0.f) { m = s.mu * m + g; g = m; }                // (a zero-initialised buffer is torch's first-step rule with dampening 0)
    p -= s.lr * g;
  } else if (RULE == RULE_RMSPROP) {
    v = s.a1 * v + (1.f - s.a1) * g * g;
    float u = g / (sqrtf(v) + s.eps);
    if (s.mu > 0.f) { m = s.mu * m + u; u = m; }
    p -= s.lr * u;
  } else {
    if (RULE == RULE_ADAMW && dec) p -= s.lr * s.wd * p;        // decoupled: p *= 1 - lr wd first, magic_adamw(decay_first = 1)'s arithmetic
    m = s.a1 * m + (1.f - s.a1) * g;
    v = s.b2 * v + (1.f - s.b2) * g * g;
    p -= s.lr_bc1 * m / (sqrtf(v) / s.sq_bc2 + s.eps);
  }
}

// One launch over the whole flat range.  VEC: p, g, m, v are 16-byte aligned (and the shadow 8-byte): 16-byte loads and stores, an 8-byte store of
// four shadow elements, the n & 3 tail through the scalar loop; otherwise the scalar loop takes every element.  n_decay may fall inside a vector.
template <typename Hh, int RULE, bool VEC>
__global__ __launch_bounds__(256) void flat_update_kernel(FlatUpd a) {
  constexpr bool HAS_V = RULE != RULE_SGD;
  const bool has_m = RULE == RULE_ADAM || RULE == RULE_ADAMW || a.mu > 0.f;
  const long long n = a.n, stride = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n4 = VEC ? n >> 2 : 0;
  float ssv = 0.f;
  if (a.ss) {
    const int slot = a.words[3] != 0.f;
    ssv = a.ss[slot];
    // the word the next step accumulates into, and the switch to it: nobody in this launch reads either
    if (first == 0) { a.ss[1 - slot] = 0.f; a.step[2] = 1 - slot; }
  }
  if (a.ss && !isfinite(ssv)) {
    // a non-finite norm skips the update as adamw_kernel does (optim.hip, the comment there gives the reasons): p, the state buffers and the shadow
    // untouched, the gradient consumed, the skip counted, the state step taken back (the lr step stays advanced)
    if (first == 0) { if (a.step) a.step[1] -= 1; if (a.overflow) a.overflow[0] += 1u; }
    if (a.zero_g) {
      for (long long i = first; i < n4; i += stride) ((float4*)a.g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (long long i = (n4 << 2) + first; i < n; i += stride) a.g[i] = 0.f;
    }
    return;
  }
  FlatScal s;
  s.c = a.gscale;
  if (a.ss && a.max_norm > 0.f) s.c = a.gscale * fminf(1.f, a.max_norm / (sqrtf(ssv) * a.gscale + 1e-6f));      // clip_grad_norm_'s factor
  s.lr = a.words[0];
  s.lr_bc1 = (RULE == RULE_ADAM || RULE == RULE_ADAMW) ? a.words[1] : 0.f;
  s.sq_bc2 = (RULE == RULE_ADAM || RULE == RULE_ADAMW) ? a.words[2] : 1.f;
  s.a1 = a.a1; s.b2 = a.b2; s.eps = a.eps; s.wd = a.wd; s.mu = a.mu;
  const long long nd = a.wd > 0.f ? a.n_decay : 0;
  Hh* shadow = (Hh*)a.shadow;
  // every stream is touched once per step and the model is far larger than the caches: nontemporal loads and stores (measured on the MAGIC-L store,
  // 155 M elements: AdamW 1.06-1.09 -> 0.93 ms; unrolling by two and folding sqrt(bc2) into eps to save a division changed nothing)
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (long long i = first; i < n4; i += stride) {
    f32x4 p = __builtin_nontemporal_load((const f32x4*)a.p + i);
    const f32x4 g = __builtin_nontemporal_load((const f32x4*)a.g + i);
    f32x4 m = has_m ? __builtin_nontemporal_load((const f32x4*)a.m + i) : zero4;
    f32x4 v = HAS_V ? __builtin_nontemporal_load((const f32x4*)a.v + i) : zero4;
    const long long e = i << 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = p[j], mj = m[j], vj = v[j];
      flat_update1<RULE>(pj, g[j], mj, vj, e + j < nd, s);
      p[j] = pj; m[j] = mj; v[j] = vj;
    }
    __builtin_nontemporal_store(p, (f32x4*)a.p + i);
    if (has_m) __builtin_nontemporal_store(m, (f32x4*)a.m + i);
    if (HAS_V) __builtin_nontemporal_store(v, (f32x4*)a.v + i);
    if (shadow) {
      h16x4<Hh> o; o[0] = (Hh)p[0]; o[1] = (Hh)p[1]; o[2] = (Hh)p[2]; o[3] = (Hh)p[3];
      __builtin_nontemporal_store(o, (h16x4<Hh>*)shadow + i);
    }
    if (a.zero_g) __builtin_nontemporal_store(zero4, (f32x4*)a.g + i);
  }
  for (long long i = (n4 << 2) + first; i < n; i += stride) {
    float p = a.p[i], m = has_m ? a.m[i] : 0.f, v = HAS_V ? a.v[i] : 0.f;
    flat_update1<RULE>(p, a.g[i], m, v, i < nd, s);
    a.p[i] = p;
    if (has_m) a.m[i] = m;
    if (HAS_V) a.v[i] = v;
    if (shadow) shadow[i] = (Hh)p;
    if (a.zero_g) a.g[i] = 0.f;
  }
}

static inline int flat_nblocks(long long n, int per) {      // optim.hip's nblocks: at most 2048 blocks, the rest by grid stride
  long long b = (n + per - 1) / per;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}
static inline bool rule_ok(int rule) { return rule >= RULE_SGD && rule <= RULE_ADAMW; }

extern "C" int magic_flat_rule_supported(int rule, int has_momentum, int centered, int nesterov, int amsgrad) {
  if (!rule_ok(rule) || centered || nesterov || amsgrad) return 0;
  if (has_momentum && rule != RULE_SGD && rule != RULE_RMSPROP) return 0;
  return 1;
}

extern "C" int magic_flat_sumsq_sched(long long n, const float* g, float* sumsq2_or_null, int* step3, int sched_kind, float lr0, float eta_min,
                                      int warmup, int t_max, int rule, float b1, float b2, float* words, void* stream) {
  if (n <= 0 || !step3 || !words || !rule_ok(rule) || (sched_kind != SCHED_CONST && sched_kind != SCHED_COSINE)) return MAGIC_ERR_ARG;
  if (sched_kind == SCHED_COSINE && (t_max <= 0 || warmup < 0)) return MAGIC_ERR_ARG;
  if (sumsq2_or_null && (!g || ((uintptr_t)g & 3))) return MAGIC_ERR_ARG;
  const int vec = ((uintptr_t)g & 15) == 0;
  int nb = 1;
  if (sumsq2_or_null) { nb = flat_nblocks(n, 4096); nb = nb > 256 ? 256 : nb; }
  hipLaunchKernelGGL(flat_sumsq_sched_kernel, dim3(nb), dim3(sumsq2_or_null ? 1024 : 64), 0, (hipStream_t)stream, n, g, sumsq2_or_null,
                     FlatSched{step3, sched_kind, lr0, eta_min, warmup, t_max, rule, b1, b2, words}, vec);
  return launch_status();
}

template <typename Hh, int RULE>
static void flat_update_launch(const FlatUpd& a, bool vec, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((flat_update_kernel<Hh, RULE, true>), dim3(flat_nblocks((a.n + 3) >> 2, 256)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((flat_update_kernel<Hh, RULE, false>), dim3(flat_nblocks(a.n, 256)), dim3(256), 0, st, a);
}

extern "C" int magic_flat_update(int rule, long long n, float* p, float* g, float* m, float* v, void* shadow, int shadow_dtype,
                                 float alpha_or_b1, float b2, float eps, float wd, float momentum, float* sumsq2_or_null,
                                 float max_norm, float gscale, const float* words, long long n_decay, int zero_grad,
                                 unsigned* overflow, int* step3, void* stream) {
  if (n <= 0 || !rule_ok(rule) || !p || !g || !words || (shadow && !dtype_is16(shadow_dtype))) return MAGIC_ERR_ARG;
  const bool adam = rule == RULE_ADAM || rule == RULE_ADAMW;
  const bool need_m = adam || momentum > 0.f, need_v = rule != RULE_SGD;
  if ((need_m && !m) || (need_v && !v)) return MAGIC_ERR_ARG;
  if (adam && momentum != 0.f) return MAGIC_ERR_ARG;
  if (max_norm > 0.f && !sumsq2_or_null) return MAGIC_ERR_ARG;
  if (sumsq2_or_null && !step3) return MAGIC_ERR_ARG;               // the switch between the two norm words lives in step3[2]
  if (!need_m) m = nullptr;
  if (!need_v) v = nullptr;
  const uintptr_t all = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
  if ((all & 3) || ((uintptr_t)shadow & 1)) return MAGIC_ERR_ARG;
  const bool vec = !(all & 15) && !((uintptr_t)shadow & 7);          // otherwise the scalar path: not an error
  if (n_decay < 0 || n_decay > n) n_decay = n;                      // the whole range is one group
  const FlatUpd a{n, n_decay, p, g, m, v, shadow, alpha_or_b1, b2, eps, wd, momentum, sumsq2_or_null, max_norm, gscale, words,
                  zero_grad, overflow, step3};
  const hipStream_t st = (hipStream_t)stream;
  DISPATCH_H(shadow ? shadow_dtype : DT_BF16,
             switch (rule) {
               case RULE_SGD: flat_update_launch<TY, RULE_SGD>(a, vec, st); break;
               case RULE_RMSPROP: flat_update_launch<TY, RULE_RMSPROP>(a, vec, st); break;
               case RULE_ADAM: flat_update_launch<TY, RULE_ADAM>(a, vec, st); break;
               default: flat_update_launch<TY, RULE_ADAMW>(a, vec, st); break;
             });
  return launch_status();
}
