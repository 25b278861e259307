// MoE routing for gfx950: gate softmax/top-k (plain, with the auxiliary losses, noisy) and the dispatch plan (histogram +
// capacity + overflow thresholds + stable ranks).  The gather-LayerNorm and the weighted combine are in layernorm.hip.
//
// Reference: AdaptiveExpertSystem.forward, /root/reference/src/model/core.py:470-607.
// The reference walks a K x E Python loop with host syncs (nonzero / .any() / topk); here the
// whole plan is built on the device with no host round-trip.  Canonical row order is
// expert-major, then k, then ascending token - equivalent to the reference's k-major loop
// because capacity is consumed per expert.
//
// Integer atomics only (deterministic).
#include "row_common.h"

namespace {

// gate: a thread per token (gate_topk_row, row_common.h)
template <int EC>
__global__ void gate_topk_fwd_k(const float *__restrict__ logits, float *__restrict__ gates,
                                int32_t *__restrict__ idx, float *__restrict__ w, int64_t S, int E_rt,
                                int K) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const int E = EC > 0 ? EC : E_rt;
  gate_topk_row<EC>(logits + s * E, gates + s * E, idx + s * K, w + s * K, E_rt, K);
}

// dlogits from dw (through renorm + top-k gather) and dgates (aux losses), softmax backward
template <int EC>
__global__ void gate_topk_bwd_k(const float *__restrict__ gates, const int32_t *__restrict__ idx,
                                const float *__restrict__ dw, const float *__restrict__ dgates,
                                float *__restrict__ dlogits, int64_t S, int E_rt, int K) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  constexpr int CAP = EC > 0 ? EC : MAXE;
  const int E = EC > 0 ? EC : E_rt;
  float g[CAP], dg[CAP];
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) { g[i] = gates[s * E + i]; dg[i] = dgates ? dgates[s * E + i] : 0.f; }
  if (dw) {
    float psum = 0.f, dot = 0.f;
    for (int k = 0; k < K; ++k) {
      int e = idx[s * K + k];
      float pe = 0.f;
#pragma unroll
      for (int i = 0; i < CAP; ++i)
        if (i == e) pe = g[i];
      psum += pe;
      dot += dw[s * K + k] * pe;
    }
    const float den = psum + 1e-6f;
    const float corr = dot / (den * den);
    for (int k = 0; k < K; ++k) {
      int e = idx[s * K + k];
      float dp = dw[s * K + k] / den - corr;
#pragma unroll
      for (int i = 0; i < CAP; ++i)
        if (i == e) dg[i] += dp;
    }
  }
  float inner = 0.f;
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) inner += dg[i] * g[i];
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) dlogits[s * E + i] = g[i] * (dg[i] - inner);
}

// ------------------------------------------------------------------------------------------
// dispatch plan
// ------------------------------------------------------------------------------------------
constexpr int PLAN_HIST_BLOCKS = 512;   // most work-groups of the candidate histogram (each leaves one row of counts)
struct PlanWs {
  int32_t *total, *keep, *mode, *quota, *seg_start, *bpart;   // bpart [PLAN_HIST_BLOCKS][P]: the histogram launch's rows
  uint32_t *thr;           // [P] overflowing slot: the keep-th largest key (quota: how many of the ties at it are kept)
  int32_t *cstart;         // [P] overflowing slot: where its candidates start in cand
  int32_t *cbase;          // [PLAN_HIST_BLOCKS][P] exclusive prefix of bpart's columns: where a work-group's candidates start in the slot's run
  uint32_t *cand;          // [S*K] the overflowing slots' candidate keys, slot after slot
  int32_t *cnt_g, *cnt_t;  // [P][NCH]
  int P, NCH;
};

PlanWs carve_ws(void *ws, int64_t S, int64_t E, int64_t K) {
  PlanWs w;
  w.P = (int)(E * K);
  w.NCH = (int)ceil_div64(S, 64);
  int32_t *p = (int32_t *)ws;
  w.total = p; p += w.P;
  w.keep = p; p += w.P;
  w.mode = p; p += w.P;
  w.quota = p; p += w.P;
  w.seg_start = p; p += w.P;
  w.thr = (uint32_t *)p; p += w.P;
  w.cstart = p; p += w.P;
  w.cnt_g = p; p += (int64_t)w.P * w.NCH;
  w.cnt_t = p; p += (int64_t)w.P * w.NCH;
  w.bpart = p; p += (int64_t)PLAN_HIST_BLOCKS * w.P;
  w.cbase = p; p += (int64_t)PLAN_HIST_BLOCKS * w.P;
  w.cand = (uint32_t *)p;   // [S*K]
  return w;
}

// Candidates per (expert, k) slot.  Every work-group leaves ONE row of P counts in `bpart` (no global atomics: with the first
// form's atomicAdd per block and slot, 512-1024 work-groups queued up on the same 16 addresses - 41 us for 1 MB of indices on
// the H = 256 configuration); inside a work-group a wave counts each slot it holds with one ballot (a 64-lane LDS atomic on
// <= 16 addresses serialises).  plan_capacity_k sums the rows in block order.
__global__ void __launch_bounds__(256)
plan_hist_k(const int32_t *__restrict__ idx, int32_t *__restrict__ bpart, int64_t SK, int E, int K) {
  __shared__ int32_t h[MAXE * MAXK];
  const int P = E * K, lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < P; i += blockDim.x) h[i] = 0;
  __syncthreads();
  for (int64_t a0 = (int64_t)blockIdx.x * blockDim.x; a0 < SK; a0 += (int64_t)gridDim.x * blockDim.x) {   // (uniform trip count)
    const int64_t a = a0 + threadIdx.x;
    int slot = -1;
    if (a < SK) {
      const int e = idx[a];
      if (e >= 0 && e < E) slot = e * K + (int)(a % K);
    }
    unsigned long long todo = __ballot(slot >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int s0 = __shfl(slot, leader);
      const unsigned long long m = __ballot(slot == s0);
      if (lane == leader) atomicAdd(&h[s0], __popcll(m));
      todo &= ~m;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < P; i += blockDim.x) bpart[(int64_t)blockIdx.x * P + i] = h[i];
}

// per expert: consume capacity k-major (core.py:547-576); then lay the segments out expert-major.  Also where every
// work-group's candidates of a slot go in the compacted candidate array (plan_compact_k): cbase, cstart.
__global__ void plan_capacity_k(PlanWs w, const uint8_t *__restrict__ active, int64_t capacity,
                                int32_t *__restrict__ offsets, int E, int K, int nhist) {
  // totals: the histogram launch's per-work-group rows (integers: any order gives the same sums).  256 threads, 256 / P of them
  // per slot when the slots are few, each with a run of consecutive rows: the sums of the runs before a thread's own are
  // where its rows' exclusive prefixes (cbase) start
  __shared__ int32_t s_sum[256];
  {
    const int P = E * K;
    const int g = P < 256 ? 256 / P : 1;                 // threads per slot
    const int per = (nhist + g - 1) / g;                 // rows per thread
    const int pc = 256 / g;                              // slots per trip; neighbouring threads hold neighbouring slots of one row
    for (int p0 = 0; p0 < P; p0 += pc) {
      const int p = p0 + (int)threadIdx.x % pc, sub = (int)threadIdx.x / pc;
      const bool on = p < P && sub < g;
      const int b0 = min(sub * per, nhist), b1 = min(b0 + per, nhist);
      int t = 0;
      if (on)
        for (int b = b0; b < b1; ++b) t += w.bpart[(int64_t)b * P + p];
      s_sum[threadIdx.x] = t;
      __syncthreads();
      if (on) {
        int run = 0, tt = 0;
        for (int q = 0; q < g; ++q) {
          const int v = s_sum[q * pc + (int)threadIdx.x % pc];
          if (q < sub) run += v;
          tt += v;
        }
        if (sub == 0) w.total[p] = tt;
        for (int b = b0; b < b1; b += 8) {   // (eight loads in flight: a load behind every store is a memory latency per row)
          int v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = b + u < b1 ? w.bpart[(int64_t)(b + u) * P + p] : 0;
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (b + u < b1) { w.cbase[(int64_t)(b + u) * P + p] = run; run += v[u]; }
        }
      }
      __syncthreads();
    }
  }
  const int e = threadIdx.x;
  if (e < E) {
    int64_t load = 0;
    const bool on = active ? active[e] != 0 : true;
    for (int k = 0; k < K; ++k) {
      const int p = e * K + k;
      const int tot = w.total[p];
      int64_t keep = tot;
      if (!on) keep = 0;
      else if (capacity > 0) {
        int64_t rem = capacity - load;
        keep = rem <= 0 ? 0 : (tot < rem ? tot : rem);
      }
      w.keep[p] = (int)keep;
      w.mode[p] = keep == 0 ? 0 : (keep == tot ? 1 : 2);
      w.quota[p] = (int)keep;   // (an overflowing slot: plan_select_keys_k sets the ties to keep, and thr)
      load += keep;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0, crun = 0;
    for (int ee = 0; ee < E; ++ee) {
      offsets[ee] = run;
      for (int k = 0; k < K; ++k) {
        const int p = ee * K + k;
        w.seg_start[p] = run;
        run += w.keep[p];
        w.cstart[p] = crun;
        if (w.mode[p] == 2) crun += w.total[p];
      }
    }
    offsets[E] = run;
  }
}

// The gate weights of every overflowing (mode 2) slot's candidates, gathered into one flat array: same grid and same
// element-to-work-group mapping as plan_hist_k, so work-group b holds exactly bpart[b][p] candidates of slot p and writes
// them from cstart[p] + cbase[b][p] on.  The rank inside the work-group comes from an LDS counter per slot that a wave
// advances once per slot it holds (one ballot, as in plan_hist_k); the order inside a slot's run is free - the select
// needs the multiset of keys only.  No global atomics: every word of cand has one writer.
__global__ void __launch_bounds__(256)
plan_compact_k(PlanWs w, const int32_t *__restrict__ idx, const float *__restrict__ wk, int64_t SK, int E, int K) {
  __shared__ int32_t s_pos[MAXE * MAXK];   // next free word of cand for this work-group's candidates of the slot
  __shared__ int32_t s_m2[MAXE * MAXK];    // slot overflows
  const int P = E * K, lane = threadIdx.x & 63;
  int any = 0;
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    const int m2 = w.mode[i] == 2;
    s_m2[i] = m2;
    s_pos[i] = m2 ? w.cstart[i] + w.cbase[(int64_t)blockIdx.x * P + i] : 0;
    any |= m2;
  }
  if (!__syncthreads_or(any)) return;   // nothing overflows
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int64_t a0 = (int64_t)blockIdx.x * blockDim.x; a0 < SK; a0 += (int64_t)gridDim.x * blockDim.x) {   // (uniform trip count)
    const int64_t a = a0 + threadIdx.x;
    int slot = -1;
    uint32_t bits = 0;
    if (a < SK) {
      const int e = idx[a];
      bits = __float_as_uint(wk[a]);
      if (e >= 0 && e < E) {
        const int p = e * K + (int)(a % K);
        if (s_m2[p]) slot = p;
      }
    }
    unsigned long long todo = __ballot(slot >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int s0 = __shfl(slot, leader);
      const unsigned long long m = __ballot(slot == s0);
      int base = 0;
      if (lane == leader) base = atomicAdd(&s_pos[s0], __popcll(m));
      base = __shfl(base, leader);
      if (slot == s0) w.cand[base + __popcll(m & lt)] = bits;
      todo &= ~m;
    }
  }
}

// Overflowing (e,k) slot, one work-group each: T = the keep-th largest key of the slot's candidates (keys are the raw bits of
// gate weights >= 0, so unsigned order == float order) and how many of the ties at T to keep.  T is built from the top bit
// down, two bits per round: the work-group counts the keys >= T | j << b for j = 1..3 and takes the largest j that still
// leaves `keep` of them.  A count is a compare and an add-with-carry per key in the thread's own counters (as a ballot and a
// scalar popcount per key the 16 waves queued up at the CU's one scalar unit: 47 us per slot of 22 500), summed over the wave
// by DPP once per round; the 16 waves combine through 16 LDS rows (two sets, taken in turn: one barrier per round), which
// each wave reads once, a row per lane, and sums by DPP again.  No histogram and no atomics.
// On-chip budget: the first SEL_REG * 1024 = 32768 candidates stay in registers for all 17 rounds; a slot with more streams
// the rest from cand (L2) every round.  Keys >= 1 are all that is ever counted, so the zero padding never counts.
constexpr int SEL_THREADS = 1024, SEL_REG = 32, SEL_WAVES = SEL_THREADS / 64;
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false); }
__device__ __forceinline__ int wave_sum_i(int v) {   // (wave_sum, row_common.h, on integers)
  v += dpp_i<0xB1, 0xf>(v);
  v += dpp_i<0x4E, 0xf>(v);
  v += dpp_i<0x141, 0xf>(v);
  v += dpp_i<0x140, 0xf>(v);
  v += dpp_i<0x142, 0xa>(v);
  v += dpp_i<0x143, 0xc>(v);
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int row16_sum_i(int v) {   // sum over the lane's row of 16, in every lane
  v += dpp_i<0xB1, 0xf>(v);
  v += dpp_i<0x4E, 0xf>(v);
  v += dpp_i<0x141, 0xf>(v);
  v += dpp_i<0x140, 0xf>(v);
  return v;
}
__global__ void __launch_bounds__(SEL_THREADS)
plan_select_keys_k(PlanWs w) {
  const int p = blockIdx.x;
  if (w.mode[p] != 2) return;
  const int n = w.total[p], keep = w.keep[p];
  const uint32_t *__restrict__ c = w.cand + w.cstart[p];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ int4 s_c[2][SEL_WAVES];
  uint32_t key[SEL_REG];
#pragma unroll
  for (int i = 0; i < SEL_REG; ++i) {
    const int j = i * SEL_THREADS + tid;
    key[i] = j < n ? c[j] : 0u;
  }
  const int nreg = min((n + SEL_THREADS - 1) / SEL_THREADS, SEL_REG);   // register rows that hold a key at all
  int round = 0;
  // keys >= t1, >= t2, >= t3 in the whole slot (t1, t2, t3 >= 1); every thread gets the three sums
  auto count3 = [&](uint32_t t1, uint32_t t2, uint32_t t3, int &n1, int &n2, int &n3) {
    int c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
    for (int i0 = 0; i0 < SEL_REG; i0 += 8)
      if (i0 < nreg) {   // (eight rows per branch; a row of padding counts nothing)
#pragma unroll
        for (int i = i0; i < i0 + 8; ++i) {
          c1 += key[i] >= t1;
          c2 += key[i] >= t2;
          c3 += key[i] >= t3;
        }
      }
    for (int j0 = SEL_REG * SEL_THREADS; j0 < n; j0 += SEL_THREADS) {   // past the budget (uniform trip count)
      const int j = j0 + tid;
      const uint32_t kk = j < n ? c[j] : 0u;
      c1 += kk >= t1;
      c2 += kk >= t2;
      c3 += kk >= t3;
    }
    c1 = wave_sum_i(c1); c2 = wave_sum_i(c2); c3 = wave_sum_i(c3);
    int4 *row = s_c[round & 1];
    ++round;
    if (lane == 0) row[wave] = make_int4(c1, c2, c3, 0);
    __syncthreads();
    // lane l takes wave l & 15's row: ONE LDS read per wave, then the sum over a DPP row of 16 lanes (every thread reading
    // all 16 rows was 256 broadcast reads per round through the CU's LDS: 42 us per slot instead of 36)
    const int4 r = row[lane & (SEL_WAVES - 1)];
    n1 = row16_sum_i(r.x); n2 = row16_sum_i(r.y); n3 = row16_sum_i(r.z);
  };
  uint32_t T = 0;
  for (int b = 30; b >= 0; b -= 2) {
    int n1, n2, n3;
    count3(T | (1u << b), T | (2u << b), T | (3u << b), n1, n2, n3);
    const uint32_t j = n3 >= keep ? 3u : (n2 >= keep ? 2u : (n1 >= keep ? 1u : 0u));
    T |= j << b;
  }
  int gt = 0, u2, u3;
  if (T != 0xffffffffu) count3(T + 1u, 0xffffffffu, 0xffffffffu, gt, u2, u3);
  if (tid == 0) { w.thr[p] = T; w.quota[p] = keep - gt; }
}

__device__ __forceinline__ void plan_flags(const PlanWs &w, const int32_t *idx, const float *wk, int64_t s,
                                           int64_t S, int k, int E, int K, int &e, bool &fg, bool &ft) {
  e = -1; fg = false; ft = false;
  if (s < S) {
    e = idx[s * K + k];
    if (e >= 0 && e < E) {
      const int p = e * K + k;
      const int m = w.mode[p];
      if (m == 1) fg = true;
      else if (m == 2) {
        uint32_t bits = __float_as_uint(wk[s * K + k]);
        uint32_t t = w.thr[p];
        fg = bits > t;
        ft = bits == t;
      }
    } else e = -1;
  }
}

// per 64-token chunk and (e,k): number of kept-for-sure rows and of threshold ties
__global__ void plan_count_k(PlanWs w, const int32_t *__restrict__ idx, const float *__restrict__ wk,
                             int64_t S, int E, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (chunk >= w.NCH) return;
  const int64_t s = chunk * 64 + lane;
  for (int k = 0; k < K; ++k) {
    int e; bool fg, ft;
    plan_flags(w, idx, wk, s, S, k, E, K, e, fg, ft);
    for (int ee = 0; ee < E; ++ee) {
      unsigned long long bg = __ballot(e == ee && fg);
      unsigned long long bt = __ballot(e == ee && ft);
      if (lane == 0) {
        w.cnt_g[(int64_t)(ee * K + k) * w.NCH + chunk] = __popcll(bg);
        w.cnt_t[(int64_t)(ee * K + k) * w.NCH + chunk] = __popcll(bt);
      }
    }
  }
}

// in-place exclusive scan of 2P arrays of NCH ints (blockIdx.x picks the array)
__global__ void __launch_bounds__(256) plan_scan_k(PlanWs w) {
  int32_t *arr = (blockIdx.x < (unsigned)w.P ? w.cnt_g + (int64_t)blockIdx.x * w.NCH
                                              : w.cnt_t + (int64_t)(blockIdx.x - w.P) * w.NCH);
  __shared__ int32_t part[256];
  const int per = (w.NCH + 255) / 256;
  const int b0 = threadIdx.x * per, b1 = min(b0 + per, w.NCH);
  int sum = 0;
  for (int i = b0; i < b1; ++i) sum += arr[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { int t = part[i]; part[i] = run; run += t; }
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int i = b0; i < b1; ++i) { int t = arr[i]; arr[i] = run; run += t; }
}

__global__ void plan_assign_k(PlanWs w, const int32_t *__restrict__ idx, const float *__restrict__ wk,
                              int32_t *__restrict__ row_token, int32_t *__restrict__ row_k,
                              int32_t *__restrict__ slot_of, int64_t S, int E, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t chunk = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (chunk >= w.NCH) return;
  const int64_t s = chunk * 64 + lane;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int k = 0; k < K; ++k) {
    int e; bool fg, ft;
    plan_flags(w, idx, wk, s, S, k, E, K, e, fg, ft);
    int pre_g = 0, pre_t = 0;
    for (int ee = 0; ee < E; ++ee) {
      unsigned long long bg = __ballot(e == ee && fg);
      unsigned long long bt = __ballot(e == ee && ft);
      if (e == ee) { pre_g = __popcll(bg & lt); pre_t = __popcll(bt & lt); }
    }
    if (s < S) {
      int slot = -1;
      if (e >= 0 && (fg || ft)) {
        const int p = e * K + k;
        const int gb = w.cnt_g[(int64_t)p * w.NCH + chunk] + pre_g;
        const int tb = w.cnt_t[(int64_t)p * w.NCH + chunk] + pre_t;
        const int q = w.quota[p];
        if (fg || tb < q) {
          slot = w.seg_start[p] + gb + (tb < q ? tb : q);
          row_token[slot] = (int32_t)s;
          row_k[slot] = k;
        }
      }
      slot_of[s * K + k] = slot;
    }
  }
}

// the plan of a handful of tokens in one launch (plan_small_body, row_common.h)
__global__ void __launch_bounds__(1024)
plan_small_k(const int32_t *__restrict__ idx, const float *__restrict__ wk, const uint8_t *__restrict__ active, int64_t capacity,
             int32_t *__restrict__ offsets, int32_t *__restrict__ row_token, int32_t *__restrict__ row_k,
             int32_t *__restrict__ slot_of, int S, int E, int K) {
  plan_small_body(idx, wk, active, capacity, offsets, row_token, row_k, slot_of, S, E, K, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------
// gate + auxiliary losses in one pass (training): besides gates / top-K / weights, the per-row
// log-sum-exp and the three reductions the two router losses need - column sums of the gates,
// assignment counts per expert, sum of lse^2 - as per-block partials, folded in block order by
// gate_aux_fold_k, which also evaluates (reference core.py:499-505, 524-526)
//   lb = lb_coef * E * sum_e (count_e / S) * (colsum_e / S),   rz = rz_coef * sum_s lse_s^2 / S.
// As stock tensor ops the two losses are ~35 launches forward and ~25 backward per layer, 4-5 us each
// on [S, 8] tensors, plus a 47 us index_add.  stats out: [lb, rz, frac_0..frac_{E-1}].
// ------------------------------------------------------------------------------------------
// Noisy top-k routing (reference core.py:485-488): logits += randn * softplus(w_noise) * alpha.  The standard normals come
// from a counter hash of (seed, token, expert pair) through Box-Muller, so the backward regenerates them instead of keeping
// a [S, E] tensor, and the whole noise path is part of the gate kernels (as tensor ops it was ten launches per layer).
__device__ __forceinline__ void gauss_pair(uint64_t seed, uint64_t pair, float &n0, float &n1) {
  const uint32_t h0 = drop_hash_pair(seed, 2 * pair), h1 = drop_hash_pair(seed ^ 0x9E3779B97F4A7C15ull, 2 * pair + 1);
  const float u1 = ((float)(h0 >> 8) + 1.0f) * (1.0f / 16777216.0f);      // (0, 1]
  const float u2 = (float)(h1 >> 8) * (1.0f / 16777216.0f);               // [0, 1)
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);
  n0 = r * cs;
  n1 = r * sn;
}
__device__ __forceinline__ float softplus_gate(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // F.softplus (beta 1, threshold 20)
// the row's E standard normals (pairs share one Box-Muller draw; an odd last expert uses the first of its pair)
template <int CAP>
__device__ __forceinline__ void row_noise(uint64_t seed, int64_t s, int E, float (&nz)[CAP]) {
  const int64_t ppr = (E + 1) / 2;
#pragma unroll
  for (int i = 0; i < CAP; i += 2) {
    if (i < E) {
      float a, b;
      gauss_pair(seed, (uint64_t)(s * ppr + (i >> 1)), a, b);
      nz[i] = a;
      if (i + 1 < CAP) nz[i + 1] = b;
    }
  }
}

template <int EC>
__global__ void __launch_bounds__(256)
gate_topk_aux_fwd_k(const float *__restrict__ logits, const float *__restrict__ w_noise, float alpha, uint64_t seed,
                    float *__restrict__ gates, int32_t *__restrict__ idx,
                    float *__restrict__ w, float *__restrict__ lse, float *__restrict__ part, int64_t S, int E_rt, int K) {
  constexpr int CAP = EC > 0 ? EC : MAXE;
  const int E = EC > 0 ? EC : E_rt;
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = s < S;
  float v[CAP];
  float cnt[CAP];
  float l2 = 0.f;
#pragma unroll
  for (int i = 0; i < CAP; ++i) { v[i] = 0.f; cnt[i] = 0.f; }
  if (live) {
    const float *row = logits + s * E;
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < E) v[i] = row[i];
    if (w_noise) {
      float nz[CAP];
      row_noise<CAP>(seed, s, E, nz);
#pragma unroll
      for (int i = 0; i < CAP; ++i)
        if (i < E) v[i] += nz[i] * (softplus_gate(w_noise[i]) * alpha);
    }
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < E) m = fmaxf(m, v[i]);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < E) { v[i] = expf(v[i] - m); sum += v[i]; }
    const float l = m + logf(sum);
    lse[s] = l;
    l2 = l * l;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < E) { v[i] = v[i] / sum; gates[s * E + i] = v[i]; }
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
        idx[s * K + k] = bi;
        p[k] = best;
        psum += best;
      }
    }
    const float den = psum + 1e-6f;  // core.py:529
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k < K) w[s * K + k] = p[k] / den;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < E) cnt[i] = (float)((chosen >> i) & 1);
  }
  // block partials: [colsum(gates) E | counts E | sum lse^2]
  __shared__ float red[4][2 * MAXE + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < CAP; ++i) {
    if (i < E) {
      const float a = wave_sum(v[i]), b = wave_sum(cnt[i]);
      if (lane == 0) { red[wv][i] = a; red[wv][E + i] = b; }
    }
  }
  l2 = wave_sum(l2);
  if (lane == 0) red[wv][2 * E] = l2;
  __syncthreads();
  if (threadIdx.x < 2 * E + 1)
    part[(int64_t)blockIdx.x * (2 * E + 1) + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ void __launch_bounds__(1024)
gate_aux_fold_k(const float *__restrict__ part, float *__restrict__ stats, int64_t nblk, int64_t S, int E, float lb_coef,
                float rz_coef) {
  __shared__ float tot[2 * MAXE + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int cols = 2 * E + 1;
  for (int cc = wv; cc < cols; cc += 16) {     // a wave per column: lane-strided partial sums, then the wave (fixed order)
    float a = 0.f;
    for (int64_t b = lane; b < nblk; b += 64) a += part[b * cols + cc];
    a = wave_sum(a);
    if (lane == 0) tot[cc] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float lb = 0.f;
    for (int e = 0; e < E; ++e) lb += (tot[E + e] / (float)S) * (tot[e] / (float)S);
    stats[0] = lb_coef * (float)E * lb;
    stats[1] = rz_coef * tot[2 * E] / (float)S;
  }
  if (threadIdx.x < E) stats[2 + threadIdx.x] = tot[E + threadIdx.x] / (float)S;
}

// backward of gate + losses: dgates[s,e] = dlb * lb_coef * E * frac_e / S (the load-balancing loss through the
// gate means), dlogits += drz * rz_coef * 2 lse_s / S * gates[s,e] (d lse / d logits = softmax)
template <int EC>
__global__ void __launch_bounds__(256)
gate_topk_aux_bwd_k(const float *__restrict__ gates, const int32_t *__restrict__ idx,
                    const float *__restrict__ dw, const float *__restrict__ lse,
                    const float *__restrict__ stats, const float *__restrict__ dlb,
                    const float *__restrict__ drz, float lb_coef, float rz_coef,
                    float *__restrict__ dlogits, float *__restrict__ npart, uint64_t seed, int64_t S, int E_rt, int K) {
  // npart != NULL (noisy routing): [gridDim.x][E] block sums of dlogits * n, the gradient of the per-expert noise scale
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int CAP = EC > 0 ? EC : MAXE;
  const int E = EC > 0 ? EC : E_rt;
  float dsc[CAP];
#pragma unroll
  for (int i = 0; i < CAP; ++i) dsc[i] = 0.f;
  if (s < S) {
  const float glb = dlb ? dlb[0] * lb_coef * (float)E / (float)S : 0.f;
  const float grz = drz ? drz[0] * rz_coef * 2.f * lse[s] / (float)S : 0.f;
  float g[CAP], dg[CAP];
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) { g[i] = gates[s * E + i]; dg[i] = glb * stats[2 + i]; }
  if (dw) {
    float psum = 0.f, dot = 0.f;
    for (int k = 0; k < K; ++k) {
      int e = idx[s * K + k];
      float pe = 0.f;
#pragma unroll
      for (int i = 0; i < CAP; ++i)
        if (i == e) pe = g[i];
      psum += pe;
      dot += dw[s * K + k] * pe;
    }
    const float den = psum + 1e-6f;
    const float corr = dot / (den * den);
    for (int k = 0; k < K; ++k) {
      int e = idx[s * K + k];
      float dp = dw[s * K + k] / den - corr;
#pragma unroll
      for (int i = 0; i < CAP; ++i)
        if (i == e) dg[i] += dp;
    }
  }
  float inner = 0.f;
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) inner += dg[i] * g[i];
  float nz[CAP];
  if (npart) row_noise<CAP>(seed, s, E, nz);
#pragma unroll
  for (int i = 0; i < CAP; ++i)
    if (i < E) {
      const float dl = g[i] * (dg[i] - inner) + grz * g[i];
      dlogits[s * E + i] = dl;
      if (npart) dsc[i] = dl * nz[i];
    }
  }
  if (npart) {
    __shared__ float red[4][MAXE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
      if (i < E) {
        const float a = wave_sum(dsc[i]);
        if (lane == 0) red[wv][i] = a;
      }
    __syncthreads();
    if (threadIdx.x < E)
      npart[(int64_t)blockIdx.x * E + threadIdx.x] =
          (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

// d w_noise[e] = (sum over blocks of npart[., e]) * alpha * sigmoid(w_noise[e])  (softplus' = sigmoid), fixed order
__global__ void __launch_bounds__(1024)
gate_noise_fold_k(const float *__restrict__ npart, const float *__restrict__ w_noise, float alpha, float *__restrict__ dw_noise,
                  int64_t nblk, int E) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int e = wv; e < E; e += 16) {
    float a = 0.f;
    for (int64_t b = lane; b < nblk; b += 64) a += npart[b * E + e];
    a = wave_sum(a);
    if (lane == 0) {
      const float x = w_noise[e];
      dw_noise[e] = a * alpha * (x > 20.f ? 1.f : 1.f / (1.f + expf(-x)));
    }
  }
}

}  // namespace

extern "C" int apertis_moe_gate_topk_fwd(const float *logits, float *gates, int32_t *idx, float *w,
                                         int64_t S, int64_t E, int64_t K, void *stream) {
  if (!logits || !gates || !idx || !w || S < 0) return APERTIS_ERR_ARG;
  if (E < 1 || E > MAXE || K < 1 || K > MAXK || K > E) return APERTIS_ERR_UNSUPPORTED;
  if (S == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)ceil_div64(S, 256)), block(256);
#define GO(EC) hipLaunchKernelGGL(gate_topk_fwd_k<EC>, grid, block, 0, st, logits, gates, idx, w, S, (int)E, (int)K)
  if (E == 4) GO(4); else if (E == 8) GO(8); else if (E == 16) GO(16); else GO(0);
#undef GO
  return apertis_check_launch();
}

extern "C" int apertis_moe_gate_topk_bwd(const float *gates, const int32_t *idx, const float *dw,
                                         const float *dgates, float *dlogits, int64_t S, int64_t E,
                                         int64_t K, void *stream) {
  if (!gates || !idx || !dlogits || S < 0) return APERTIS_ERR_ARG;
  if (E < 1 || E > MAXE || K < 1 || K > MAXK || K > E) return APERTIS_ERR_UNSUPPORTED;
  if (S == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)ceil_div64(S, 256)), block(256);
#define GO(EC) hipLaunchKernelGGL(gate_topk_bwd_k<EC>, grid, block, 0, st, gates, idx, dw, dgates, dlogits, S, (int)E, (int)K)
  if (E == 4) GO(4); else if (E == 8) GO(8); else if (E == 16) GO(16); else GO(0);
#undef GO
  return apertis_check_launch();
}

extern "C" int64_t apertis_moe_plan_workspace_bytes(int64_t S, int64_t E, int64_t K) {
  int64_t P = E * K, NCH = ceil_div64(S > 0 ? S : 1, 64);
  return (7 * P + 2 * P * NCH + 2 * PLAN_HIST_BLOCKS * P + (S > 0 ? S : 1) * K) * 4 + 64;
}

extern "C" int apertis_moe_plan(const int32_t *idx, const float *w, const uint8_t *active,
                                int64_t capacity, int32_t *expert_offsets, int32_t *row_token,
                                int32_t *row_k, int32_t *slot_of, void *ws, int64_t S, int64_t E,
                                int64_t K, void *stream) {
  if (!idx || !w || !expert_offsets || !row_token || !row_k || !slot_of || !ws || S < 0) return APERTIS_ERR_ARG;
  if (E < 1 || E > MAXE || K < 1 || K > MAXK) return APERTIS_ERR_UNSUPPORTED;
  if (S * K > 0x7fffffffLL) return APERTIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (S > 0 && S <= 64 && E * K <= 16) {   // a handful of tokens: the whole plan in one launch
    hipLaunchKernelGGL(plan_small_k, dim3(1), dim3(64 * (unsigned)(E * K)), 0, st, idx, w, active, capacity, expert_offsets,
                       row_token, row_k, slot_of, (int)S, (int)E, (int)K);
    return apertis_check_launch();
  }
  PlanWs pw = carve_ws(ws, S > 0 ? S : 1, E, K);
  int nhist = 0;
  if (S > 0) {
    nhist = (int)std::min<int64_t>(ceil_div64(S * K, 1024), PLAN_HIST_BLOCKS);   // four elements per thread where there are enough
    hipLaunchKernelGGL(plan_hist_k, dim3((unsigned)nhist), dim3(256), 0, st, idx, pw.bpart, S * K, (int)E, (int)K);
  }
  hipLaunchKernelGGL(plan_capacity_k, dim3(1), dim3(256), 0, st, pw, active, capacity, expert_offsets, (int)E, (int)K, nhist);
  if (S > 0) {
    if (capacity > 0) {
      // overflow thresholds (whether any slot overflows is known on the device only)
      hipLaunchKernelGGL(plan_compact_k, dim3((unsigned)nhist), dim3(256), 0, st, pw, idx, w, S * K, (int)E, (int)K);
      hipLaunchKernelGGL(plan_select_keys_k, dim3((unsigned)pw.P), dim3(SEL_THREADS), 0, st, pw);
    }
    dim3 cgrid((unsigned)ceil_div64(pw.NCH, 4)), cblock(256);
    hipLaunchKernelGGL(plan_count_k, cgrid, cblock, 0, st, pw, idx, w, S, (int)E, (int)K);
    hipLaunchKernelGGL(plan_scan_k, dim3(2 * pw.P), dim3(256), 0, st, pw);
    hipLaunchKernelGGL(plan_assign_k, cgrid, cblock, 0, st, pw, idx, w, row_token, row_k, slot_of, S, (int)E, (int)K);
  }
  return apertis_check_launch();
}

extern "C" int64_t apertis_moe_gate_aux_blocks(int64_t S) { return ceil_div64(S > 0 ? S : 1, 256); }

extern "C" int apertis_moe_gate_topk_noisy_aux_fwd(const float *logits, const float *w_noise, float alpha, uint64_t seed,
                                                   float *gates, int32_t *idx, float *w, float *lse, float *part, float *stats,
                                                   int64_t S, int64_t E, int64_t K, float lb_coef, float rz_coef, void *stream) {
  // part: workspace [apertis_moe_gate_aux_blocks(S)][2E+1]; stats: out [2 + E] = [lb, rz, frac_e]; w_noise NULL: no noise
  if (!logits || !gates || !idx || !w || !lse || !part || !stats || S <= 0) return APERTIS_ERR_ARG;
  if (E < 1 || E > MAXE || K < 1 || K > MAXK || K > E) return APERTIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = apertis_moe_gate_aux_blocks(S);
  dim3 grid((unsigned)nblk), block(256);
#define GO(EC) hipLaunchKernelGGL(gate_topk_aux_fwd_k<EC>, grid, block, 0, st, logits, w_noise, alpha, seed, gates, idx, w, lse, part, S, (int)E, (int)K)
  if (E == 4) GO(4); else if (E == 8) GO(8); else if (E == 16) GO(16); else GO(0);
#undef GO
  hipLaunchKernelGGL(gate_aux_fold_k, dim3(1), dim3(1024), 0, st, part, stats, nblk, S, (int)E, lb_coef, rz_coef);
  return apertis_check_launch();
}

extern "C" int apertis_moe_gate_topk_aux_fwd(const float *logits, float *gates, int32_t *idx, float *w, float *lse,
                                             float *part, float *stats, int64_t S, int64_t E, int64_t K, float lb_coef,
                                             float rz_coef, void *stream) {
  return apertis_moe_gate_topk_noisy_aux_fwd(logits, nullptr, 0.f, 0, gates, idx, w, lse, part, stats, S, E, K, lb_coef, rz_coef,
                                             stream);
}

extern "C" int apertis_moe_gate_topk_noisy_aux_bwd(const float *gates, const int32_t *idx, const float *dw, const float *lse,
                                                   const float *stats, const float *dlb, const float *drz, float lb_coef,
                                                   float rz_coef, const float *w_noise, float alpha, uint64_t seed,
                                                   float *dlogits, float *npart, float *dw_noise, int64_t S, int64_t E,
                                                   int64_t K, void *stream) {
  // w_noise != NULL: npart = workspace [apertis_moe_gate_aux_blocks(S)][E], dw_noise = out [E]
  if (!gates || !idx || !lse || !stats || !dlogits || S < 0 || (w_noise && (!npart || !dw_noise))) return APERTIS_ERR_ARG;
  if (!w_noise) npart = nullptr;
  if (E < 1 || E > MAXE || K < 1 || K > MAXK || K > E) return APERTIS_ERR_UNSUPPORTED;
  if (S == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)ceil_div64(S, 256)), block(256);
#define GO(EC) hipLaunchKernelGGL(gate_topk_aux_bwd_k<EC>, grid, block, 0, st, gates, idx, dw, lse, stats, dlb, drz, lb_coef, rz_coef, dlogits, npart, seed, S, (int)E, (int)K)
  if (E == 4) GO(4); else if (E == 8) GO(8); else if (E == 16) GO(16); else GO(0);
#undef GO
  if (npart) hipLaunchKernelGGL(gate_noise_fold_k, dim3(1), dim3(1024), 0, st, npart, w_noise, alpha, dw_noise, (int64_t)grid.x, (int)E);
  return apertis_check_launch();
}

extern "C" int apertis_moe_gate_topk_aux_bwd(const float *gates, const int32_t *idx, const float *dw, const float *lse,
                                             const float *stats, const float *dlb, const float *drz, float lb_coef,
                                             float rz_coef, float *dlogits, int64_t S, int64_t E, int64_t K, void *stream) {
  return apertis_moe_gate_topk_noisy_aux_bwd(gates, idx, dw, lse, stats, dlb, drz, lb_coef, rz_coef, nullptr, 0.f, 0, dlogits,
                                             nullptr, nullptr, S, E, K, stream);
}
