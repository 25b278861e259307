// Next-token selection of generate(): one launch per token step, one 1024-thread work-group per row.
//
// Reference: ApertisForCausalLM.generate, core.py:1605-1633.  Between the LM head's last-position logits and the next token
// the reference runs, per step: the repetition-penalty loop (one in-place division per occurrence of a token in the row's
// history, a host loop), temperature, torch.topk + masked_fill, torch.sort + softmax + cumsum + scatter (top-p), softmax and
// torch.multinomial (or torch.argmax), then the pad / eos bookkeeping.  sample_next_k does all of it for a row:
//   1. penalty      x[v] / p, c times in sequence (c = counts[b, v]): fp32 true divisions, the reference's loop bit for bit
//   2. temperature  x / t (sampling only)
//   3. top-k        threshold = the k-th largest value, duplicates counted: a radix select (8-bit digits, LDS histograms of
//                   counts) over order-preserving 32-bit keys; every x >= threshold stays (ties at the threshold stay)
//   4. top-p        the same walk weighted by exp(x - max): the sorted position whose inclusive cumulative mass first exceeds
//                   top_p, found without a sort; inside the boundary's tie group the lowest vocabulary index comes first
//   5. the token    sampling: the first index, in vocabulary order, whose inclusive prefix of kept weights exceeds u * Z (the
//                   walk once more, keyed by index); greedy: the argmax, lowest index among equal maxima
//   6. bookkeeping  next = alive ? token : pad, alive cleared on an eos id, counts[b, next] += 1
// Determinism: the weights are fixed-point integers (exp(x - max) * 2^44, rounded; a row sums to < 2^63), so every mass -
// histogram bins, totals, prefixes - is an exact integer sum that no order of atomics can change: the same inputs give the
// same token, bit for bit.  Only integer LDS atomics; no work-group talks to another.
#include "common.h"

namespace {

constexpr int SNT = 1024;                        // threads per row
constexpr int SNW = SNT / APERTIS_WAVE;
constexpr double WSCALE = 17592186044416.0;      // 2^44

// order-preserving key of a float (-0 folded onto +0: torch compares them equal)
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f == 0.f ? 0.f : f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float keyf(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ uint64_t wfix(float x, float mx) { return (uint64_t)((double)expf(x - mx) * WSCALE + 0.5); }

// 32 random bits of (seed, row, step): two rounds of the library's avalanche
__device__ __forceinline__ uint32_t sample_bits(uint64_t seed, int64_t row, uint64_t step) {
  uint32_t h = hash_avalanche32((uint32_t)seed ^ ((uint32_t)row * 0x9E3779B9u));
  return hash_avalanche32(h ^ (uint32_t)(seed >> 32) ^ ((uint32_t)step * 0x85ebca6bu) ^ (uint32_t)(step >> 32));
}

struct SampleArgs {
  const void *logits;
  int64_t logits_rs;
  int32_t *counts;
  float penalty, temp, top_p;
  int do_sample;
  int64_t top_k;
  uint64_t seed;
  const int64_t *step;
  int64_t step_off;
  const int64_t *alive_in;
  int64_t *alive_out;
  const int64_t *eos;
  int64_t n_eos, pad;
  int64_t *next;
  const double *uniforms;
  int64_t u_rs, u_cols;
  float *probs_out;
  float *x_out;
  double *u_out;
  int32_t *err;
  int V, ishift;
};

// The processed row of one work-group: R values per thread in registers (entry j * SNT + tid), or R = 0: recomputed from the
// logits and the counts at every pass (the row sits in L2).  Either way a value is computed by the same operations.
template <typename T, int R>
struct Row {
  const T *x;
  const int32_t *cnt;       // NULL: no penalty
  float pen, temp;          // temp = 1: none
  int V;
  float v[R > 0 ? R : 1];

  __device__ __forceinline__ float value(int i) const {
    float f = to_f32(x[i]);
    if (cnt)
      for (int c = cnt[i]; c > 0; --c) f = f / pen;
    if (temp != 1.f) f = f / temp;
    return f;
  }
  __device__ __forceinline__ void load() {
    if constexpr (R > 0) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int i = j * SNT + (int)threadIdx.x;
        v[j] = i < V ? value(i) : 0.f;
      }
    }
  }
  template <class F> __device__ __forceinline__ void each(F f) const {
    if constexpr (R > 0) {
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int i = j * SNT + (int)threadIdx.x;
        if (i < V) f(i, v[j]);
      }
    } else {
      for (int i = threadIdx.x; i < V; i += SNT) f(i, value(i));
    }
  }
};

template <typename U, typename Op>
__device__ __forceinline__ U block_reduce(U v, Op op, U *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  U r = red[0];
#pragma unroll
  for (int w = 1; w < SNW; ++w) r = op(r, red[w]);
  __syncthreads();
  return r;
}

struct SelRes {
  uint32_t found, digit;
  unsigned long long above;
};

// Walk the keys of the participating entries from the top, 8 bits at a time: `key` = the key at which the inclusive running
// weight first exceeds `target`, `above` = the weight of the participants with a larger key.  false when the total weight is
// <= target.  kw(i, x, key, weight) says whether entry i takes part, with which key and weight.  Every thread returns the same.
template <typename Acc, typename RowT, typename KW>
__device__ bool select_desc(const RowT &row, KW kw, int shift0, Acc target, uint32_t &key, Acc &above, Acc *hist, SelRes *res) {
  uint32_t prefix = 0;
  Acc abv = 0;
  for (int shift = shift0; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += SNT) hist[i] = 0;
    __syncthreads();
    const uint32_t hi = shift >= 24 ? 0u : (0xffffffffu << (shift + 8));
    row.each([&](int i, float x) {
      uint32_t k;
      Acc w;
      if (kw(i, x, k, w) && w != 0 && (k & hi) == prefix) atomicAdd(&hist[(k >> shift) & 255u], w);
    });
    __syncthreads();
    if (threadIdx.x < 64) {
      const int l = threadIdx.x;
      Acc h[4];
#pragma unroll
      for (int d = 0; d < 4; ++d) h[d] = hist[4 * l + d];
      const Acc s = (h[0] + h[1]) + (h[2] + h[3]);
      Acc suf = s;                                         // inclusive suffix over lanes >= l (bins from 4l up)
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const Acc t = __shfl_down(suf, o);
        if (l + o < 64) suf += t;
      }
      if (l == 0) res->found = (abv + suf > target) ? 1u : 0u;
      Acc run = abv + (suf - s);
#pragma unroll
      for (int d = 3; d >= 0; --d) {
        const Acc nrun = run + h[d];
        if (run <= target && nrun > target) {
          res->digit = (uint32_t)(4 * l + d);
          res->above = (unsigned long long)run;
        }
        run = nrun;
      }
    }
    __syncthreads();
    if (!res->found) return false;
    prefix |= res->digit << shift;
    abv = (Acc)res->above;
  }
  key = prefix;
  above = abv;
  return true;
}

template <typename T, int R>
__global__ void __launch_bounds__(SNT) sample_next_k(SampleArgs a) {
  __shared__ unsigned long long hist[256];
  __shared__ unsigned long long red64[SNW];
  __shared__ float redf[SNW];
  __shared__ SelRes res;
  const int b = blockIdx.x, V = a.V;
  const uint64_t step = (uint64_t)((a.step ? a.step[0] : 0) + a.step_off);

  double u;
  bool u_bad = false;
  if (a.uniforms) {
    const int64_t s = (int64_t)step;
    u_bad = s < 0 || s >= a.u_cols;
    u = u_bad ? 0.0 : a.uniforms[(int64_t)b * a.u_rs + s];
    if (!(u >= 0.0)) u = 0.0;
    if (u >= 1.0) u = 0x1.fffffffffffffp-1;
  } else {
    u = (double)sample_bits(a.seed, b, step) * 0x1p-32;
  }
  if (threadIdx.x == 0 && a.u_out) a.u_out[b] = u;

  const int64_t alive = a.alive_in[b];
  float *probs = a.probs_out ? a.probs_out + (int64_t)b * V : nullptr;
  if (alive == 0) {                                          // a finished row: pad, nothing else (core.py:1622)
    if (probs)
      for (int i = threadIdx.x; i < V; i += SNT) probs[i] = 0.f;
    if (threadIdx.x == 0) {
      a.next[b] = a.pad;
      a.alive_out[b] = 0;
    }
    return;
  }

  Row<T, R> row;
  row.x = (const T *)a.logits + (int64_t)b * a.logits_rs;
  row.cnt = (a.counts && a.penalty != 1.f) ? a.counts + (int64_t)b * V : nullptr;
  row.pen = a.penalty;
  row.temp = a.do_sample ? a.temp : 1.f;
  row.V = V;
  row.load();
  if (a.x_out) {                                             // (test output: the row after penalty and temperature)
    float *xo = a.x_out + (int64_t)b * V;
    row.each([&](int i, float x) { xo[i] = x; });
  }

  int pick = 0;
  bool failed = false;
  if (!a.do_sample) {
    // torch.argmax: the largest value, NaN above everything, the lowest index among equals
    unsigned long long best = 0;
    row.each([&](int i, float x) {
      const unsigned long long c = ((unsigned long long)(isnan(x) ? 0xffffffffu : fkey(x)) << 32) | (uint32_t)(V - 1 - i);
      best = c > best ? c : best;
    });
    best = block_reduce(best, [](unsigned long long p, unsigned long long q) { return p > q ? p : q; }, red64);
    pick = V - 1 - (int)(uint32_t)best;
  } else {
    float mx = -INFINITY;
    unsigned long long nan_any = 0;
    row.each([&](int i, float x) {
      if (isnan(x)) nan_any = 1;
      else mx = fmaxf(mx, x);
    });
    mx = block_reduce(mx, [](float p, float q) { return fmaxf(p, q); }, redf);
    nan_any = block_reduce(nan_any, [](unsigned long long p, unsigned long long q) { return p | q; }, red64);
    failed = nan_any != 0 || isinf(mx);                      // multinomial raises: inf / nan or no positive weight
    if (!failed) {
      // 3. top-k
      uint32_t Kk = 0;
      if (a.top_k > 0 && a.top_k < V) {
        uint32_t above;
        select_desc<uint32_t>(row, [&](int, float x, uint32_t &k, uint32_t &w) { k = fkey(x); w = 1u; return true; }, 24,
                              (uint32_t)(a.top_k - 1), Kk, above, (uint32_t *)hist, &res);
      }
      // 4. top-p on what top-k left
      bool cut = false;
      uint32_t Kp = 0;
      int vb = V;
      if (a.top_p < 1.f) {
        unsigned long long z1 = 0;
        row.each([&](int, float x) {
          if (fkey(x) >= Kk) z1 += wfix(x, mx);
        });
        z1 = block_reduce(z1, [](unsigned long long p, unsigned long long q) { return p + q; }, red64);
        const double P = (double)a.top_p * (double)z1;
        const unsigned long long target = P <= 0.0 ? 0ull : (unsigned long long)P;   // cum > P <=> cum > floor(P)
        unsigned long long Ap;
        if (target < z1 &&
            select_desc<unsigned long long>(row, [&](int, float x, uint32_t &k, unsigned long long &w) {
              k = fkey(x);
              if (k < Kk) return false;
              w = wfix(x, mx);
              return true;
            }, 24, target, Kp, Ap, hist, &res)) {
          cut = true;
          // the tie group of the boundary key shares one weight: its r-th member (lowest index first) is the boundary
          const unsigned long long wt = wfix(keyf(Kp), mx);
          const uint32_t r = (uint32_t)((target - Ap) / wt);
          uint32_t kidx, above;
          select_desc<uint32_t>(row, [&](int i, float x, uint32_t &k, uint32_t &w) {
            if (fkey(x) != Kp) return false;
            k = (uint32_t)(V - 1 - i);
            w = 1u;
            return true;
          }, a.ishift, r, kidx, above, (uint32_t *)hist, &res);
          vb = V - 1 - (int)kidx;
        }
      }
      auto kept = [&](int i, float x) {
        const uint32_t k = fkey(x);
        return k >= Kk && (!cut || k > Kp || (k == Kp && i <= vb));
      };
      // 5. the draw: inverse CDF in vocabulary order over the kept weights
      unsigned long long z = 0;
      row.each([&](int i, float x) {
        if (kept(i, x)) z += wfix(x, mx);
      });
      z = block_reduce(z, [](unsigned long long p, unsigned long long q) { return p + q; }, red64);
      unsigned long long t = (unsigned long long)(u * (double)z);
      if (t >= z) t = z - 1;                                 // (z >= 2^44: the maximum is always kept)
      uint32_t kd;
      unsigned long long ad;
      select_desc<unsigned long long>(row, [&](int i, float x, uint32_t &k, unsigned long long &w) {
        if (!kept(i, x)) return false;
        k = (uint32_t)(V - 1 - i);
        w = wfix(x, mx);
        return true;
      }, a.ishift, t, kd, ad, hist, &res);                  // (always found: t < z, integer sums are exact)
      pick = V - 1 - (int)kd;
      if (probs) {
        const float zf = (float)((double)z / WSCALE);
        row.each([&](int i, float x) { probs[i] = kept(i, x) ? expf(x - mx) / zf : 0.f; });
      }
    } else if (probs) {
      for (int i = threadIdx.x; i < V; i += SNT) probs[i] = 0.f;
    }
  }
  __syncthreads();                                           // (every thread is done with counts[b, :] and alive_in[b])
  if (threadIdx.x == 0) {
    if (failed || u_bad) atomicOr(a.err, (failed ? 1 : 0) | (u_bad ? 2 : 0));
    bool hit = false;
    for (int64_t e = 0; e < a.n_eos; ++e) hit |= a.eos[e] == (int64_t)pick;
    a.next[b] = pick;
    a.alive_out[b] = hit ? 0 : alive;
    if (a.counts) a.counts[(int64_t)b * V + pick] += 1;
  }
}

__global__ void __launch_bounds__(256)
token_counts_k(const int64_t *__restrict__ tok, int64_t rs, int64_t L, int64_t V, int32_t *__restrict__ counts, int32_t *err) {
  const int64_t b = blockIdx.y, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= L) return;
  int64_t t = tok[b * rs + i];
  if (t >= V) return;                                        // skipped, as the reference skips them (core.py:1608)
  if (t < 0) {                                               // Python indexing: -V..-1 wrap, anything below raises
    if (t < -V) {
      atomicOr(err, 4);
      return;
    }
    t += V;
  }
  atomicAdd(&counts[b * V + t], 1);
}

template <typename T, int R>
void launch_sample(const SampleArgs &a, int64_t B, hipStream_t st) {
  hipLaunchKernelGGL((sample_next_k<T, R>), dim3((unsigned)B), dim3(SNT), 0, st, a);
}

template <typename T>
void dispatch_sample(const SampleArgs &a, int64_t B, hipStream_t st) {
  if (a.V <= SNT) launch_sample<T, 1>(a, B, st);
  else if (a.V <= 4 * SNT) launch_sample<T, 4>(a, B, st);
  else if (a.V <= 8 * SNT) launch_sample<T, 8>(a, B, st);
  else launch_sample<T, 0>(a, B, st);
}

}  // namespace

extern "C" int apertis_token_counts(const int64_t *tokens, int64_t tok_rs, int64_t B, int64_t L, int64_t V, int32_t *counts,
                                    int32_t *err, void *stream) {
  if (!tokens || !counts || !err || B < 1 || L < 0 || V < 1 || (B > 1 && tok_rs < L)) return APERTIS_ERR_ARG;
  if (V > APERTIS_SAMPLE_MAX_VOCAB || B > APERTIS_SAMPLE_MAX_ROWS) return APERTIS_ERR_UNSUPPORTED;
  if (L == 0) return APERTIS_OK;
  hipLaunchKernelGGL(token_counts_k, dim3((unsigned)ceil_div64(L, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, tokens,
                     tok_rs, L, V, counts, err);
  return apertis_check_launch();
}

extern "C" int apertis_sample_next(const void *logits, int64_t logits_rs, int dtype, int64_t B, int64_t V, int32_t *counts,
                                   float penalty, int do_sample, float temperature, int64_t top_k, float top_p, uint64_t seed,
                                   const int64_t *step, int64_t step_off, const int64_t *alive_in, int64_t *alive_out,
                                   const int64_t *eos, int64_t n_eos, int64_t pad, int64_t *next, const double *uniforms,
                                   int64_t u_rs, int64_t u_cols, float *probs_out, float *x_out, double *u_out, int32_t *err,
                                   void *stream) {
  if (!logits || !alive_in || !alive_out || !next || !err || B < 1 || V < 1 || (B > 1 && logits_rs < V)) return APERTIS_ERR_ARG;
  if (n_eos < 0 || (n_eos > 0 && !eos) || top_k < 0 || top_k > V || (do_sample && !(temperature > 0.f))) return APERTIS_ERR_ARG;
  if (uniforms && (u_cols < 1 || u_rs < 0 || (B > 1 && u_rs < u_cols))) return APERTIS_ERR_ARG;
  if (dtype != APERTIS_F32 && dtype != APERTIS_BF16) return APERTIS_ERR_UNSUPPORTED;
  if (V > APERTIS_SAMPLE_MAX_VOCAB || B > 0x7fffffff) return APERTIS_ERR_UNSUPPORTED;
  SampleArgs a;
  a.logits = logits;
  a.logits_rs = logits_rs;
  a.counts = counts;
  a.penalty = penalty;
  a.temp = temperature;
  a.top_p = top_p;
  a.do_sample = do_sample;
  a.top_k = top_k;
  a.seed = seed;
  a.step = step;
  a.step_off = step_off;
  a.alive_in = alive_in;
  a.alive_out = alive_out;
  a.eos = eos;
  a.n_eos = n_eos;
  a.pad = pad;
  a.next = next;
  a.uniforms = uniforms;
  a.u_rs = u_rs;
  a.u_cols = u_cols;
  a.probs_out = probs_out;
  a.x_out = x_out;
  a.u_out = u_out;
  a.err = err;
  a.V = (int)V;
  int nb = 0;                                                // the index walk: 8-bit digits over the bits of V - 1
  while (nb < 32 && ((uint64_t)(V - 1) >> nb)) ++nb;
  a.ishift = nb <= 8 ? 0 : 8 * ((nb + 7) / 8 - 1);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == APERTIS_F32) dispatch_sample<float>(a, B, st);
  else dispatch_sample<bf16_t>(a, B, st);
  return apertis_check_launch();
}
