// Shared pieces of the row kernels (layernorm.hip: the LayerNorm family, the router and the decode entrance; small_linear.hip:
// the skinny and tiny linears; moe_routing.hip: gate and plan): row-chunk loads and stores, wave sums, the LayerNorm row
// statistics, the gate and plan bodies the fused small-batch kernels reuse, the fixed-order fold of partial rows and the host
// dispatch macros.  Everything lives in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int MAXE = 64;  // experts
constexpr int MAXK = 8;   // experts per token

// ------------------------------------------------------------------------------------------
// gate: softmax -> top-K (ties: lowest expert index) -> renormalised weights
// ------------------------------------------------------------------------------------------
template <int EC>  // EC > 0: compile-time expert count; EC == 0: runtime E <= MAXE
__device__ __forceinline__ void gate_topk_row(const float *__restrict__ row, float *__restrict__ gates_row, int32_t *idx_row,
                                              float *w_row, int E_rt, int K) {
  constexpr int CAP = EC > 0 ? EC : MAXE;
  const int E = EC > 0 ? EC : E_rt;
  float v[CAP];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) { v[i] = row[i]; m = fmaxf(m, v[i]); }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) { v[i] = expf(v[i] - m); sum += v[i]; }
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) { v[i] = v[i] / sum; gates_row[i] = v[i]; }
  uint64_t chosen = 0;
  float p[MAXK];
  float psum = 0.f;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    if (k < K) {
      float best = -1.f;
      int bi = 0;
#pragma unroll
      for (int i = 0; i < CAP; ++i)
        if (i < E && !((chosen >> i) & 1) && v[i] > best) { best = v[i]; bi = i; }
      chosen |= 1ull << bi;
      idx_row[k] = bi;
      p[k] = best;
      psum += best;
    }
  }
  const float den = psum + 1e-6f;  // core.py:529
#pragma unroll
  for (int k = 0; k < MAXK; ++k)
    if (k < K) w_row[k] = p[k] / den;
}

// The whole plan in ONE launch for a handful of tokens (S <= 64, E * K <= 16: the single-token decode step, reference
// core.py:1578-1603 - the five launches of apertis_moe_plan were a fifth of a captured token step).  One wave per (expert, k) slot,
// lane = token.  Same semantics: candidates idx[s, k] == e; per expert the capacity is consumed k-major; an overflowing
// slot keeps its `keep` largest gate weights (compared as bits, as plan_select_keys_k does), ties at the threshold in token
// order; the kept rows of a slot sit in token order, the slots expert-major then k.
__device__ __forceinline__ void
plan_small_body(const int32_t *idx, const float *wk, const uint8_t *__restrict__ active, int64_t capacity,
                int32_t *__restrict__ offsets, int32_t *__restrict__ row_token, int32_t *__restrict__ row_k,
                int32_t *__restrict__ slot_of, int S, int E, int K, int32_t *s_off, int32_t *s_rtok) {
  // (s_off [E + 1] / s_rtok [S * K]: optional LDS copies of offsets / row_token for a caller that carries on in the same launch)
  __shared__ int32_t s_tot[16], s_keep[16], s_start[16];
  const int P = E * K, p = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int e = p / K, k = p - e * K;
  int es = -1;
  uint32_t bits = 0;
  if (p < P && lane < S) {
    es = idx[lane * K + k];
    bits = __float_as_uint(wk[lane * K + k]);
  }
  const bool cand = p < P && es == e;
  const unsigned long long cm = __ballot(cand);
  if (p < P && lane == 0) s_tot[p] = __popcll(cm);
  __syncthreads();
  if ((int)threadIdx.x < E) {
    const int ee = threadIdx.x;
    const bool on = active ? active[ee] != 0 : true;
    int64_t load = 0;
    for (int kk = 0; kk < K; ++kk) {
      const int tot = s_tot[ee * K + kk];
      int64_t keep = tot;
      if (!on) keep = 0;
      else if (capacity > 0) {
        const int64_t rem = capacity - load;
        keep = rem <= 0 ? 0 : (tot < rem ? tot : rem);
      }
      s_keep[ee * K + kk] = (int)keep;
      load += keep;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int ee = 0; ee < E; ++ee) {
      offsets[ee] = run;
      if (s_off) s_off[ee] = run;
      for (int kk = 0; kk < K; ++kk) { s_start[ee * K + kk] = run; run += s_keep[ee * K + kk]; }
    }
    offsets[E] = run;
    if (s_off) s_off[E] = run;
  }
  __syncthreads();
  if (p >= P) return;
  const int keep = s_keep[p], tot = s_tot[p];
  bool kept = cand && keep > 0;
  if (keep > 0 && keep < tot) {      // overflow: rank among the slot's candidates by (weight descending, token ascending)
    int pos = 0;
    for (int j = 0; j < S; ++j) {
      const uint32_t bj = (uint32_t)__shfl((int)bits, j);
      if ((cm >> j) & 1ull) pos += (bj > bits) || (bj == bits && j < lane);
    }
    kept = cand && pos < keep;
  }
  const unsigned long long km = __ballot(kept);
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  if (lane < S) {
    if (cand) {
      int slot = -1;
      if (kept) {
        slot = s_start[p] + __popcll(km & lt);
        row_token[slot] = lane;
        row_k[slot] = k;
        if (s_rtok) s_rtok[slot] = lane;
      }
      slot_of[lane * K + k] = slot;
    } else if (e == 0 && (es < 0 || es >= E)) {
      slot_of[lane * K + k] = -1;     // an index outside [0, E): no expert's wave claims the pair
    }
  }
}

// ------------------------------------------------------------------------------------------
// row helpers: a wave owns one row of H elements, lane handles 4-element chunks lane+64*i
// ------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float4 load4(const T *p);
template <> __device__ __forceinline__ float4 load4<float>(const float *p) {
  return *reinterpret_cast<const float4 *>(p);
}
template <> __device__ __forceinline__ float4 load4<bf16_t>(const bf16_t *p) {
  uint2 u = *reinterpret_cast<const uint2 *>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                     __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
// Streaming row data, read once and written once: NON-TEMPORAL both ways.  Every tensor these kernels read or write is 0.2 - 0.5
// GB, larger than what the caches can hand from producer to consumer; moved through them it displaces what the next kernels
// read.  Measured on the whole step (A/B inside one gpurun call, sums of kernel times): `nt` stores in the row kernels alone
// -7 ms per step, most of it in the expert GEMMs that FOLLOW them (they run 1.5 - 2.5 % faster); with the GEMM epilogues',
// the scan outputs' and AdamW's accesses non-temporal as well 479.6 -> 468.9 ms.  Which kernel gains depends on its
// neighbours (the LayerNorm backward is 2 % slower with nt stores, the combine backward behind it 15 % faster), so the
// choice was made on the step, not per kernel.  The affine vectors (gamma, beta, W) stay on plain loads: they are re-read.
template <typename T> __device__ __forceinline__ float4 load4s(const T *p);
template <> __device__ __forceinline__ float4 load4s<float>(const float *p) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  const f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(p));
  return make_float4(t.x, t.y, t.z, t.w);
}
template <> __device__ __forceinline__ float4 load4s<bf16_t>(const bf16_t *p) {
  typedef __attribute__((ext_vector_type(2))) unsigned u2;
  const u2 u = __builtin_nontemporal_load(reinterpret_cast<const u2 *>(p));
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                     __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}
template <typename T> __device__ __forceinline__ void store4(T *p, float4 v);
// (what the write-heavy kernels spend on their stores - round 5, a probe build with the data stores compiled out:
//  profiles/r5_probe_row_kernels_nostore.log; the switch left this file in round 6, round 5's tree has it - tools/probes/README.md)
template <> __device__ __forceinline__ void store4<float>(float *p, float4 v) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  f4 o = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(o, reinterpret_cast<f4 *>(p));
}
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t *p, float4 v) {
  typedef __attribute__((ext_vector_type(4))) bf16_t bf4;
  typedef __attribute__((ext_vector_type(2))) unsigned u2;
  bf4 o = {(bf16_t)v.x, (bf16_t)v.y, (bf16_t)v.z, (bf16_t)v.w};
  __builtin_nontemporal_store(__builtin_bit_cast(u2, o), reinterpret_cast<u2 *>(p));
}

// a row chunk kept in its storage form (the persistent row kernels hold the NEXT row this way: half the registers for bf16)
template <typename TX> struct raw4;
template <> struct raw4<float> { typedef float4 type; };
template <> struct raw4<bf16_t> { typedef uint2 type; };
// a row chunk in its storage form, streamed (non-temporal, see load4s)
__device__ __forceinline__ float4 raw_load(const float *p) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  const f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(p));
  return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ uint2 raw_load(const bf16_t *p) {
  typedef __attribute__((ext_vector_type(2))) unsigned u2;
  const u2 t = __builtin_nontemporal_load(reinterpret_cast<const u2 *>(p));
  return make_uint2(t.x, t.y);
}
__device__ __forceinline__ float4 raw_to_f4(const float4 &v) { return v; }
__device__ __forceinline__ float4 raw_to_f4(const uint2 &u) {
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}

// Sum over the 64 lanes, the same value in every lane.  DPP adds inside the rows of 16 (quad swaps, half-row and row
// mirrors), row broadcasts across them, one v_readlane of lane 63: seven VALU instructions.  As six __shfl_xor steps
// (ds_bpermute_b32 + s_waitcnt lgkmcnt + add each, ~60 cycles of dependent latency per step) the ten reductions per row of
// the router forward were most of that kernel.  Fixed order: deterministic.
// 1 / H once per kernel (the compiler hoists it): the statistics of a row are sums TIMES this instead of sums divided by H -
// an IEEE division is ~10 instructions, and the row kernels did two to four of them per row
__device__ __forceinline__ float inv_h(int H) { return 1.f / (float)H; }

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_f<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
  v += dpp_f<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
  v += dpp_f<0x141, 0xf>(v);   // row_half_mirror
  v += dpp_f<0x140, 0xf>(v);   // row_mirror: every lane holds its row's sum
  v += dpp_f<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v += dpp_f<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3: lane 63 holds the total
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Mean of a wave's row held as IT float4 chunks per lane (chunk i of lane l: columns (l + 64 i) * 4 .. + 3, ignored past H):
// sum / H, and for a row whose elements are all equal that value itself.  sum / H misses it by an ulp (260 copies of 0.3),
// and then x - mean is that ulp in every column: at the default eps (1e-12) rstd = 1e6 turned it into an error of up to 0.67
// in the normalised row, where the stock LayerNorm is exact.  Every other row keeps the sum's bits.
template <int IT>
__device__ __forceinline__ float row_mean(const float4 (&v)[IT], int lane, int H) {
  const float x0 = __shfl(v[0].x, 0);
  float s = 0.f;
  bool same = true;
#pragma unroll
  for (int i = 0; i < IT; ++i)
    if ((lane + 64 * i) * 4 < H) {
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
      same = same && v[i].x == x0 && v[i].y == x0 && v[i].z == x0 && v[i].w == x0;
    }
  const float m = wave_sum(s) * inv_h(H);
  return __builtin_amdgcn_ballot_w64(!same) == 0 ? x0 : m;
}

__device__ __forceinline__ int expert_of_row(const int32_t *offsets, int E, int r) {
  int e = 0;
  while (e + 1 < E && offsets[e + 1] <= r) ++e;
  return e;
}

// The LayerNorm statistics of a wave's row (row_mean's layout): its mean, and rstd = 1 / sqrt(centred sum of squares / H + eps)
template <int IT>
__device__ __forceinline__ void row_stats(const float4 (&v)[IT], int lane, int H, float eps, float &mean, float &rstd) {
  mean = row_mean<IT>(v, lane, H);
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
      const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
      sq += (a * a + b * b) + (cc * cc + d * d);
    }
  }
  rstd = rsqrtf(wave_sum(sq) * inv_h(H) + eps);
}

// rows per wave of the LayerNorm backward (layernorm_bwd_k)
#ifndef APERTIS_LN_RPW
#define APERTIS_LN_RPW 8
#endif
constexpr int LN_RPW = APERTIS_LN_RPW;

// waves per SIMD the COMB form is compiled for at H = 513..768 (IT = 3): 3 = the plain form's occupancy (168 registers, a few
// spilled: 482-500 us at the bench shape, alone), 1 = what the compiler takes by itself (two waves per SIMD, both rows' expert
// rows in flight with the rows: 461-465 us)
#ifndef APERTIS_LN_COMB_WAVES
#define APERTIS_LN_COMB_WAVES 1
#endif
constexpr int LN_COMB_WAVES = APERTIS_LN_COMB_WAVES;

constexpr int SK_MAXN = 16;   // most outputs of the skinny linear and the router

// out[c] = sum_r part[r][c] for c < cols (fixed order)
__global__ void __launch_bounds__(1024)
fold_rows_k(const float *__restrict__ part, float *__restrict__ out, int64_t nrows, int64_t cols) {
  colsum_block(part, 0, nrows, cols, [&](int64_t c, float t) { out[c] = t; });
}

int check_H(int64_t H) { return (H > 0 && H % 4 == 0 && H <= 256 * 16) ? APERTIS_OK : APERTIS_ERR_UNSUPPORTED; }

}  // namespace

// dispatch a kernel template on IT = ceil(H/256) in {1,2,3,4,6,8,12,16}
#define DISPATCH_IT(H, ...)                                    \
  do {                                                         \
    int it_ = (int)ceil_div64((H), 256);                       \
    if (it_ <= 1) { constexpr int IT = 1; __VA_ARGS__; }              \
    else if (it_ <= 2) { constexpr int IT = 2; __VA_ARGS__; }         \
    else if (it_ <= 3) { constexpr int IT = 3; __VA_ARGS__; }         \
    else if (it_ <= 4) { constexpr int IT = 4; __VA_ARGS__; }         \
    else if (it_ <= 6) { constexpr int IT = 6; __VA_ARGS__; }         \
    else if (it_ <= 8) { constexpr int IT = 8; __VA_ARGS__; }         \
    else if (it_ <= 12) { constexpr int IT = 12; __VA_ARGS__; }       \
    else { constexpr int IT = 16; __VA_ARGS__; }                      \
  } while (0)

#define DISPATCH_2T(da, db, ...)                                                           \
  do {                                                                                     \
    if ((da) == APERTIS_F32 && (db) == APERTIS_F32) { typedef float TA; typedef float TB; __VA_ARGS__; }        \
    else if ((da) == APERTIS_F32 && (db) == APERTIS_BF16) { typedef float TA; typedef bf16_t TB; __VA_ARGS__; } \
    else if ((da) == APERTIS_BF16 && (db) == APERTIS_F32) { typedef bf16_t TA; typedef float TB; __VA_ARGS__; } \
    else if ((da) == APERTIS_BF16 && (db) == APERTIS_BF16) { typedef bf16_t TA; typedef bf16_t TB; __VA_ARGS__; } \
    else return APERTIS_ERR_ARG;                                                           \
  } while (0)

// dispatch on (N, IT): N in {2,4,8,16} compile-time; other N <= 16 are padded by the caller
#define SKINNY_N(N_, ...)                                              \
  do {                                                                 \
    if ((N_) == 2) { constexpr int NN = 2; __VA_ARGS__; }              \
    else if ((N_) == 4) { constexpr int NN = 4; __VA_ARGS__; }         \
    else if ((N_) == 8) { constexpr int NN = 8; __VA_ARGS__; }         \
    else if ((N_) == 16) { constexpr int NN = 16; __VA_ARGS__; }       \
    else return APERTIS_ERR_UNSUPPORTED;                               \
  } while (0)
#define SKINNY_IT(K_, ...)                                             \
  do {                                                                 \
    int it_ = (int)ceil_div64((K_), 256);                              \
    if (it_ <= 1) { constexpr int IT = 1; __VA_ARGS__; }               \
    else if (it_ <= 2) { constexpr int IT = 2; __VA_ARGS__; }          \
    else if (it_ <= 3) { constexpr int IT = 3; __VA_ARGS__; }          \
    else if (it_ <= 4) { constexpr int IT = 4; __VA_ARGS__; }          \
    else return APERTIS_ERR_UNSUPPORTED;                               \
  } while (0)
