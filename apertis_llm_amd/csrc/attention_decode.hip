// standard_mha single-token decode on gfx950: the KV-cache append (with the RoPE rotation of q and k, rope_common.h) and
// softmax attention of ONE query row per (sequence, head) over the cached keys (reference core.py:639-700 with a past).
//
// Layout: q, out [B, H*D] rows; k_cache, v_cache [B, cap, H*D] token-major with a row and a batch stride, head h in columns
// [h*D, (h+1)*D) - what the prefill's (k, v) already are: no head transposes.
//
// attn_decode_k: the byte-bound part (K and V are read once).  A head row of D elements is 16-byte pieces over LPR = D*es/16
// lanes (8 for bf16 D 64 ... 32 for fp32 D 128), so a wave reads 64/LPR keys per load instruction, straight from global
// memory into VGPRs, 4 keys in flight per lane.  Each group of LPR lanes runs its own online softmax (m, l, o[16/es]) in fp32
// on the VALU: the dot product is a cross-lane sum inside the group, P is never rounded.  The groups of a wave are merged by
// shuffles, the 4 waves of a work-group through 2 KiB of LDS.  The key range is split over work-groups (grid splits x H x B);
// with splits > 1 every work-group leaves (m, l, o[D]) in a workspace and attn_decode_merge_k folds them in split order.  No
// atomics, no waiting between work-groups: the same inputs and split count give the same bits.
//
// The *_at forms (a captured graph replays them): the step's state is one int64 in device memory, `len` = rows the cache holds.
// The append writes row *len at rotary position *len + pos_offset and refuses, with an error word, a row or a position out of
// range; the attention reads Lk = min(*len + 1, cap) itself and cuts it into a split count fixed by the caller, so grid and
// workspace depend on nothing read from the device.  Same kernels as the by-value forms, same bits for the same row, Lk and
// split count.
//
// Multi-token steps (a chunk of Lq > 1 positions: a chat turn, a piece of a long prompt) - rope_kv_append_chunk_k appends Lq rows
// per sequence and attn_chunk_k attends them causally over cache rows [0, n + Lq).  attn_chunk_k is the forward's algorithm
// with the forward's own per-tile step (attn_tile.h: 16 query rows per wave, 32-key tiles from key 0, online softmax in fp32, no
// LDS), so at one split a query gets the bits attn_fwd_k gives it in the whole sequence.  A short chunk against a long past is
// few work-groups walking many keys: with splits > 1 each wave cuts ITS key tiles into `splits` runs (grid.z), leaves fp32
// (m, l, o[D]) per (row, head, run) in the workspace, and attn_decode_merge_k - unchanged, over B * Lq rows - folds them in order.
//
// Sliding window (entry points of apertis_hip_ext.h): attn_decode_k<.., WIN> cuts keys [max(Lk - window, 0), Lk) of the length it
// read into the fixed pieces, attn_chunk_k<.., WIN> is the forward's window form (first tile, one unsigned compare).  The plain
// instantiations are the code they were: the window is a template flag, its scalar the last field of the argument structs.
#include "attn_tile.h"
#include "rope_common.h"
#include "../../include/apertis_hip_ext.h"

namespace {

constexpr int DEC_WAVES = 4;          // waves per work-group
constexpr int DEC_UNROLL = 4;         // keys in flight per lane group
constexpr int DEC_MIN_KEYS = 128;     // the heuristic gives a split at least this many keys
constexpr int DEC_TARGET_WGS = 256;   // ... and stops splitting at one work-group per CU (measured: DESIGN.md section 3)

template <typename T> __device__ __forceinline__ void unpack16(const uint4 &r, float (&f)[16 / sizeof(T)]) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(w[i]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
}

// (m1, l1) <- merge with (m2, l2); returns the two rescale factors.  m in log2 units; m = -inf with l = 0 is "nothing yet".
__device__ __forceinline__ void softmax_merge(float &m, float m2, float &a1, float &a2) {
  const float mn = fmaxf(m, m2);
  const float mu = mn == -INFINITY ? 0.f : mn;
  a1 = exp2f(m - mu);
  a2 = exp2f(m2 - mu);
  m = mn;
}

struct DecArgs {
  const void *q, *k, *v;
  const int64_t *key_valid;
  void *out;
  float *ws_ml, *ws_o;
  int64_t q_rs, k_rs, k_bs, v_rs, v_bs, kv_rs, out_rs, Lk;
  const int64_t *len;                 // the *_at form: Lk = min(*len + 1, cap) is read here, a.Lk holds cap (null: a.Lk is Lk)
  int H, splits;
  float sl2;                          // scale * log2(e)
  int64_t window;                     // attn_decode_k<.., WIN = true> only: the keys that count, the newest included (>= 1)
};

// WIN (apertis_attention_decode_window_at): only keys [begin, Lk), begin = max(Lk - window, 0), are cut into the pieces, each
// wave's walk starts at its piece's j0 as ever - the by-value call on pointers offset by `begin` rows, with the same bits.
template <typename T, int D, bool WIN = false>
__global__ __launch_bounds__(256) void attn_decode_k(DecArgs a) {
  constexpr int E = 16 / (int)sizeof(T), LPR = D / E, KPW = APERTIS_WAVE / LPR, STEP = DEC_WAVES * KPW;
  __shared__ float sm_m[DEC_WAVES], sm_l[DEC_WAVES], sm_o[DEC_WAVES][D];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane / LPR, c = (lane % LPR) * E;
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  int64_t Lk = a.Lk;
  if (a.len) {                        // (uniform: one scalar load; a piece with j0 == j1 reads nothing and leaves (-inf, 0, 0))
    const int64_t n = *a.len + 1;
    Lk = n < 0 ? 0 : n < a.Lk ? n : a.Lk;
  }
  int64_t j0 = (int64_t)s * Lk / a.splits, j1 = (int64_t)(s + 1) * Lk / a.splits;
  if constexpr (WIN) {                // (Lk >= 0 and window >= 1: no wrap; rows, V rows and mask columns before `begin` are never read)
    const int64_t begin = Lk > a.window ? Lk - a.window : 0, n = Lk - begin;
    j0 = begin + (int64_t)s * n / a.splits;
    j1 = begin + (int64_t)(s + 1) * n / a.splits;
  }
  float qf[E];
  unpack16<T>(*reinterpret_cast<const uint4 *>(static_cast<const T *>(a.q) + (int64_t)b * a.q_rs + h * D + c), qf);
  const T *kp = static_cast<const T *>(a.k) + (int64_t)b * a.k_bs + h * D + c;
  const T *vp = static_cast<const T *>(a.v) + (int64_t)b * a.v_bs + h * D + c;
  const int64_t *kv = a.key_valid ? a.key_valid + (int64_t)b * a.kv_rs : nullptr;
  float m = -INFINITY, l = 0.f, o[E];
#pragma unroll
  for (int e = 0; e < E; ++e) o[e] = 0.f;
  for (int64_t base = j0 + w * KPW; base < j1; base += STEP * DEC_UNROLL) {       // (wave-uniform trip count)
    uint4 kr[DEC_UNROLL], vr[DEC_UNROLL];
    bool ok[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      const int64_t j = base + g + u * STEP;
      ok[u] = j < j1;
      if (kv && ok[u]) ok[u] = kv[j] != 0;
      kr[u] = vr[u] = make_uint4(0u, 0u, 0u, 0u);
      if (ok[u]) {                                  // (a masked or out-of-range key row is never read)
        kr[u] = *reinterpret_cast<const uint4 *>(kp + j * a.k_rs);
        vr[u] = *reinterpret_cast<const uint4 *>(vp + j * a.v_rs);
      }
    }
    float sc[DEC_UNROLL], tmax = -INFINITY;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      float kf[E], d = 0.f;
      unpack16<T>(kr[u], kf);
#pragma unroll
      for (int e = 0; e < E; ++e) d += qf[e] * kf[e];
#pragma unroll
      for (int off = LPR / 2; off >= 1; off >>= 1) d += __shfl_xor(d, off);
      sc[u] = ok[u] ? d * a.sl2 : -INFINITY;
      tmax = fmaxf(tmax, sc[u]);
    }
    float alpha, unused;
    softmax_merge(m, tmax, alpha, unused);
    const float mu = m == -INFINITY ? 0.f : m;
    l *= alpha;
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] *= alpha;
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      const float p = exp2f(sc[u] - mu);            // (exp2(-inf) = 0 for a key that does not count)
      float vf[E];
      unpack16<T>(vr[u], vf);
      l += p;
#pragma unroll
      for (int e = 0; e < E; ++e) o[e] += p * vf[e];
    }
  }
  // the lane groups of the wave: a butterfly, after which every group holds the wave's result
#pragma unroll
  for (int off = LPR; off < APERTIS_WAVE; off <<= 1) {
    float a1, a2;
    softmax_merge(m, __shfl_xor(m, off), a1, a2);
    l = l * a1 + __shfl_xor(l, off) * a2;
#pragma unroll
    for (int e = 0; e < E; ++e) o[e] = o[e] * a1 + __shfl_xor(o[e], off) * a2;
  }
  if (g == 0) {
#pragma unroll
    for (int e = 0; e < E; ++e) sm_o[w][c + e] = o[e];
    if (lane == 0) {
      sm_m[w] = m;
      sm_l[w] = l;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= D) return;
  float M = sm_m[0], L = sm_l[0], O = sm_o[0][t];
#pragma unroll
  for (int i = 1; i < DEC_WAVES; ++i) {             // wave order: fixed
    float a1, a2;
    softmax_merge(M, sm_m[i], a1, a2);
    L = L * a1 + sm_l[i] * a2;
    O = O * a1 + sm_o[i][t] * a2;
  }
  if (a.splits == 1) {
    static_cast<T *>(a.out)[(int64_t)b * a.out_rs + h * D + t] = from_f32<T>(L > 0.f ? O / L : 0.f);
  } else {
    const int64_t idx = ((int64_t)b * a.H + h) * a.splits + s;
    a.ws_o[idx * D + t] = O;
    if (t == 0) {
      a.ws_ml[2 * idx] = M;
      a.ws_ml[2 * idx + 1] = L;
    }
  }
}

// out[b, h*D + t] from the splits' partials, in split order; D threads per (b, h)
template <typename T, int D>
__global__ __launch_bounds__(D) void attn_decode_merge_k(DecArgs a) {
  const int t = threadIdx.x, h = blockIdx.x, b = blockIdx.y;
  const int64_t idx0 = ((int64_t)b * a.H + h) * a.splits;
  float M = a.ws_ml[2 * idx0], L = a.ws_ml[2 * idx0 + 1], O = a.ws_o[idx0 * D + t];
  for (int s = 1; s < a.splits; ++s) {
    float a1, a2;
    softmax_merge(M, a.ws_ml[2 * (idx0 + s)], a1, a2);
    L = L * a1 + a.ws_ml[2 * (idx0 + s) + 1] * a2;
    O = O * a1 + a.ws_o[(idx0 + s) * D + t] * a2;
  }
  static_cast<T *>(a.out)[(int64_t)b * a.out_rs + h * D + t] = from_f32<T>(L > 0.f ? O / L : 0.f);
}

template <typename T, int D> int launch_decode(const DecArgs &a, int64_t B, hipStream_t st) {
  const dim3 grid((unsigned)a.splits, (unsigned)a.H, (unsigned)B);
  if (a.window > 0) hipLaunchKernelGGL((attn_decode_k<T, D, true>), grid, dim3(64 * DEC_WAVES), 0, st, a);
  else hipLaunchKernelGGL((attn_decode_k<T, D>), grid, dim3(64 * DEC_WAVES), 0, st, a);
  if (a.splits > 1) hipLaunchKernelGGL((attn_decode_merge_k<T, D>), dim3((unsigned)a.H, (unsigned)B), dim3(D), 0, st, a);
  return apertis_check_launch();
}

int64_t decode_splits(int64_t B, int64_t H, int64_t Lk) {
  const int64_t want = DEC_TARGET_WGS / (B * H), by_len = Lk / DEC_MIN_KEYS;
  int64_t s = want < by_len ? want : by_len;
  if (s > APERTIS_ATTN_DECODE_MAX_SPLITS) s = APERTIS_ATTN_DECODE_MAX_SPLITS;
  return s < 1 ? 1 : s;
}

// the *_at form of the append: row and position come from *len; a row outside the cache or a position outside the rotary table
// is not written through - the kernel writes nothing and thread 0 sets *err (the host cannot check a replayed step)
struct AppendAt {
  const int64_t *len;
  int64_t pos_offset, cap;
  int32_t *err;
};

// one thread per (sequence, pair j): rotated q pair to q_out, rotated k pair and the v pair into cache row t_cache
template <typename T>
__global__ __launch_bounds__(256) void rope_kv_append_k(const T *q, int64_t q_rs, const T *k, int64_t k_rs, const T *v,
                                                        int64_t v_rs, const float *cs, const float *sn, int64_t max_pos, int64_t t,
                                                        T *qo, int64_t qo_rs, T *kc, int64_t kc_rs, int64_t kc_bs, T *vc,
                                                        int64_t vc_rs, int64_t vc_bs, int64_t t_cache, int64_t half, int64_t total,
                                                        AppendAt at) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (at.len) {
    t_cache = *at.len;
    t = t_cache + at.pos_offset;      // (no overflow: t_cache in [0, cap) is checked first, |pos_offset| on the host)
    if (t_cache < 0 || t_cache >= at.cap || (cs && (t < -max_pos || t >= max_pos))) {
      if (i == 0) *at.err = 1;
      return;
    }
  }
  if (i >= total) return;
  const int64_t b = i / half, j = i - b * half;
  const T *qs = q + b * q_rs + 2 * j, *ks = k + b * k_rs + 2 * j, *vs = v + b * v_rs + 2 * j;
  T *qd = qo + b * qo_rs + 2 * j, *kd = kc + b * kc_bs + t_cache * kc_rs + 2 * j, *vd = vc + b * vc_bs + t_cache * vc_rs + 2 * j;
  if (cs) {
    float c, s, y0, y1;
    rope_cos_sin(cs, sn, t, max_pos, half, j, c, s);
    rope_rotate_pair<false>(to_f32(qs[0]), to_f32(qs[1]), c, s, y0, y1);
    qd[0] = from_f32<T>(y0);
    qd[1] = from_f32<T>(y1);
    rope_rotate_pair<false>(to_f32(ks[0]), to_f32(ks[1]), c, s, y0, y1);
    kd[0] = from_f32<T>(y0);
    kd[1] = from_f32<T>(y1);
  } else {
    qd[0] = qs[0];
    qd[1] = qs[1];
    kd[0] = ks[0];
    kd[1] = ks[1];
  }
  vd[0] = vs[0];
  vd[1] = vs[1];
}

// -------------------------------------------------------------------------------------------------- multi-token steps
// one thread per (sequence, chunk row l, pair j): rotated q pair to q_out [B, Lq, W], rotated k pair and the v pair into cache
// row t_cache0 + l; the rotary position is t0 + l
template <typename T>
__global__ __launch_bounds__(256) void rope_kv_append_chunk_k(const T *q, int64_t q_rs, int64_t q_bs, const T *k, int64_t k_rs,
                                                              int64_t k_bs, const T *v, int64_t v_rs, int64_t v_bs,
                                                              const float *cs, const float *sn, int64_t max_pos, int64_t t0,
                                                              T *qo, T *kc, int64_t kc_rs, int64_t kc_bs, T *vc, int64_t vc_rs,
                                                              int64_t vc_bs, int64_t t_cache0, int64_t Lq, int64_t half,
                                                              int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t tok = i / half, j = i - tok * half;
  const int64_t b = tok / Lq, l = tok - b * Lq;
  const T *qs = q + b * q_bs + l * q_rs + 2 * j, *ks = k + b * k_bs + l * k_rs + 2 * j, *vs = v + b * v_bs + l * v_rs + 2 * j;
  T *qd = qo + tok * 2 * half + 2 * j, *kd = kc + b * kc_bs + (t_cache0 + l) * kc_rs + 2 * j;
  T *vd = vc + b * vc_bs + (t_cache0 + l) * vc_rs + 2 * j;
  if (cs) {
    float c, s, y0, y1;
    rope_cos_sin(cs, sn, t0 + l, max_pos, half, j, c, s);
    rope_rotate_pair<false>(to_f32(qs[0]), to_f32(qs[1]), c, s, y0, y1);
    qd[0] = from_f32<T>(y0);
    qd[1] = from_f32<T>(y1);
    rope_rotate_pair<false>(to_f32(ks[0]), to_f32(ks[1]), c, s, y0, y1);
    kd[0] = from_f32<T>(y0);
    kd[1] = from_f32<T>(y1);
  } else {
    qd[0] = qs[0];
    qd[1] = qs[1];
    kd[0] = ks[0];
    kd[1] = ks[1];
  }
  vd[0] = vs[0];
  vd[1] = vs[1];
}

struct ChunkArgs {
  const void *q, *k, *v;
  const int64_t *key_valid;
  void *out;
  float *ws_ml, *ws_o;
  int64_t q_rs, k_rs, k_bs, v_rs, v_bs, kv_rs, out_rs, Lq, n;
  int H, splits;
  float scale;
  int64_t window;                     // attn_chunk_k<.., WIN = true> only: the keys a row sees, its own included (>= 1)
};

// Query row i of the chunk sits at key position n + i and attends keys j <= n + i with key_valid[b, j] != 0.  Grid: 64-row
// blocks of the chunk (the last, longest-walking block first, as attn_fwd_k) x (B * H) x splits.  A key row at or past n + Lq,
// the row of a masked key and a mask column at or past n + Lq are never read: such a row enters the tile as zeros, and its score
// is replaced by -inf before anything reads it.
// WIN (apertis_attention_chunk_window): the forward's MASK_WINDOW form.  Row i attends keys j with n + i - window < j <= n + i: the
// diagonal and the window are ONE unsigned compare of the distance against the scalar, the wave starts at the tile that holds the
// first key its first row sees (window_first_tile; tiles in front of it are never touched) and the `splits` runs cut [first, ntile).
// Inside that first tile the rows in front of the wave's first key enter as zeros like any row that may not be read: none of the
// wave's rows counts them, so no bit moves.  No loads for the mask, no address that depends on the window.
template <typename T, int D, bool WIN = false>
__global__ __launch_bounds__(256) void attn_chunk_k(ChunkArgs a) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t Lq = a.Lq, Lk = a.n + a.Lq;
  const int bh = blockIdx.y, H = a.H, b = bh / H, h = bh - b * H, sp = blockIdx.z;
  const int64_t nblk = (Lq + WG_ROWS - 1) / WG_ROWS;
  const int64_t q0 = (nblk - 1 - blockIdx.x) * WG_ROWS + (threadIdx.x >> 6) * ROWS;
  if (q0 >= Lq) return;
  const T *qp = static_cast<const T *>(a.q) + (int64_t)b * Lq * a.q_rs + h * D;
  const T *kp = static_cast<const T *>(a.k) + (int64_t)b * a.k_bs + h * D;
  const T *vp = static_cast<const T *>(a.v) + (int64_t)b * a.v_bs + h * D;
  const int64_t *kv = a.key_valid ? a.key_valid + (int64_t)b * a.kv_rs : nullptr;
  const int64_t qi = q0 + c, pi = a.n + qi;                // this lane's chunk row and its position among the keys
  Quarter<T, D> qf;
  load_quarter(qf, qp + qi * a.q_rs + g * (D / 4), qi < Lq);
  const float sl2 = a.scale * LOG2E_F;
  float m = -INFINITY, lsum = 0.f;
  f32x4 acc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the wave's tiles: up to the one that holds its last row's own key; run `sp` of `splits` (wave-uniform, possibly empty)
  const int64_t ntile = (a.n + min(q0 + ROWS - 1, Lq - 1)) / TILE + 1;
  int64_t t0 = sp * ntile / a.splits, t1 = (sp + 1) * ntile / a.splits;
  int64_t wb = 0;                                          // WIN: the first key any row of the wave sees
  if constexpr (WIN) {                                     // (n + q0 >= 0 and window >= 1: the differences cannot wrap)
    const int64_t first = window_first_tile(a.n + q0, a.window) / TILE, nt = ntile - first;
    t0 = first + sp * nt / a.splits;
    t1 = first + (sp + 1) * nt / a.splits;
    wb = max(a.n + q0 - a.window + 1, (int64_t)0);
  }
  for (int64_t kb = t0 * TILE; kb < t1 * TILE; kb += TILE) {
    bool valid[8];                                         // k-slot t of this lane group: may the row be read at all
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int64_t key = kb + tile_row(g, t);
      valid[t] = key < Lk;
      if constexpr (WIN) valid[t] = valid[t] && key >= wb;
      if (kv && valid[t]) valid[t] = kv[key] != 0;
    }
    attn_fwd_tile<T, D>(
        qf, kp, a.k_rs, vp, a.v_rs, kb, sl2, m, lsum, acc, lane,
        [=](int64_t kr) {
          bool ok = kr < Lk;
          if constexpr (WIN) ok = ok && kr >= wb;
          if (kv && ok) ok = kv[kr] != 0;
          return ok;
        },
        [&](int t) {
          if constexpr (WIN) return valid[t] && (uint64_t)(pi - (kb + tile_row(g, t))) < (uint64_t)a.window;
          else return valid[t] && kb + tile_row(g, t) <= pi;
        },
        [&](int t) { return valid[t]; }, [](float p, int) { return p; });
  }
  const float l = xor_sum(lsum);
  if (qi >= Lq) return;
  const int64_t row = (int64_t)b * Lq + qi;
  if (a.splits == 1) {
    store_cols<T, D>(static_cast<T *>(a.out) + row * a.out_rs + h * D, acc, l > 0.f ? 1.f / l : 0.f, lane);
  } else {
    const int64_t idx = (row * H + h) * a.splits + sp;     // (attn_decode_merge_k's layout with B * Lq rows)
    store_cols<float, D>(a.ws_o + idx * D, acc, 1.f, lane);
    if (g == 0) {
      a.ws_ml[2 * idx] = m;
      a.ws_ml[2 * idx + 1] = l;
    }
  }
}

constexpr int64_t MERGE_MAX_ROWS = 65535;                  // grid.y of attn_decode_merge_k

template <typename T, int D> int launch_chunk(const ChunkArgs &a, int64_t B, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div64(a.Lq, WG_ROWS), (unsigned)(B * a.H), (unsigned)a.splits);
  if (a.window > 0) hipLaunchKernelGGL((attn_chunk_k<T, D, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((attn_chunk_k<T, D>), grid, dim3(256), 0, st, a);
  if (a.splits > 1) {
    const int64_t rows = B * a.Lq;
    for (int64_t r0 = 0; r0 < rows; r0 += MERGE_MAX_ROWS) {
      const int64_t nr = rows - r0 < MERGE_MAX_ROWS ? rows - r0 : MERGE_MAX_ROWS;
      DecArgs d{};
      d.out = static_cast<T *>(a.out) + r0 * a.out_rs;
      d.ws_ml = a.ws_ml + 2 * r0 * a.H * a.splits;
      d.ws_o = a.ws_o + r0 * a.H * a.splits * D;
      d.out_rs = a.out_rs;
      d.H = a.H;
      d.splits = a.splits;
      hipLaunchKernelGGL((attn_decode_merge_k<T, D>), dim3((unsigned)a.H, (unsigned)nr), dim3(D), 0, st, d);
    }
  }
  return apertis_check_launch();
}

// The decode rule's form, placed by a sweep of forced counts: the time follows the number of WAVES in
// flight (a 16-row chunk costs what a 64-row one costs at the same count), it stops falling at about 2 048 of them - two per
// SIMD - and a run wants at least two 32-key tiles.
constexpr int CHUNK_TARGET_WAVES = 2048;
constexpr int CHUNK_MIN_KEYS = 2 * TILE;

int64_t chunk_splits(int64_t B, int64_t H, int64_t Lq, int64_t Lk) {
  const int64_t want = CHUNK_TARGET_WAVES / (B * H * ceil_div64(Lq, ROWS)), by_len = Lk / CHUNK_MIN_KEYS;
  int64_t s = want < by_len ? want : by_len;
  if (s > APERTIS_ATTN_DECODE_MAX_SPLITS) s = APERTIS_ATTN_DECODE_MAX_SPLITS;
  return s < 1 ? 1 : s;
}

}  // namespace

// both appends: t and t_cache by value (at.len null), or the device-held length
static int rope_kv_append_impl(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs, const float *cos_cached,
                               const float *sin_cached, int64_t max_pos, int64_t t, void *q_out, int64_t q_out_rs, void *k_cache,
                        int64_t kc_rs, int64_t kc_bs, void *v_cache, int64_t vc_rs, int64_t vc_bs, int64_t cap, int64_t t_cache,
                        int64_t B, int64_t W, int dtype, void *stream, const AppendAt &at) {
  if (!q || !k || !v || !q_out || !k_cache || !v_cache || (cos_cached == nullptr) != (sin_cached == nullptr)) return APERTIS_ERR_ARG;
  if (B < 0 || W <= 0 || (W & 1) || cap < 1 || (dtype != APERTIS_F32 && dtype != APERTIS_BF16)) return APERTIS_ERR_ARG;
  if (q_rs < W || k_rs < W || v_rs < W || q_out_rs < W || kc_rs < W || vc_rs < W || kc_bs < cap * kc_rs || vc_bs < cap * vc_rs)
    return APERTIS_ERR_ARG;
  if (cos_cached && max_pos <= 0) return APERTIS_ERR_ARG;
  if (at.len) {
    // (an offset with which no row of the cache can land in the table is an argument error, and the kernel's sum cannot overflow)
    if (!at.err || (cos_cached && (at.pos_offset <= -max_pos - cap || at.pos_offset >= max_pos))) return APERTIS_ERR_ARG;
  } else {
    if (t_cache < 0 || t_cache >= cap) return APERTIS_ERR_ARG;
    if (cos_cached && (t < -max_pos || t >= max_pos)) return APERTIS_ERR_ARG;
  }
  const int64_t half = W / 2, total = B * half;
  if (total == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  if (dtype == APERTIS_F32)
    hipLaunchKernelGGL((rope_kv_append_k<float>), grid, dim3(256), 0, st, (const float *)q, q_rs, (const float *)k, k_rs,
                       (const float *)v, v_rs, cos_cached, sin_cached, max_pos, t, (float *)q_out, q_out_rs, (float *)k_cache, kc_rs,
                       kc_bs, (float *)v_cache, vc_rs, vc_bs, t_cache, half, total, at);
  else
    hipLaunchKernelGGL((rope_kv_append_k<bf16_t>), grid, dim3(256), 0, st, (const bf16_t *)q, q_rs, (const bf16_t *)k, k_rs,
                       (const bf16_t *)v, v_rs, cos_cached, sin_cached, max_pos, t, (bf16_t *)q_out, q_out_rs, (bf16_t *)k_cache,
                       kc_rs, kc_bs, (bf16_t *)v_cache, vc_rs, vc_bs, t_cache, half, total, at);
  return apertis_check_launch();
}

extern "C" int apertis_rope_kv_append(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                      const float *cos_cached, const float *sin_cached, int64_t max_pos, int64_t t, void *q_out,
                                      int64_t q_out_rs, void *k_cache, int64_t kc_rs, int64_t kc_bs, void *v_cache, int64_t vc_rs,
                                      int64_t vc_bs, int64_t cap, int64_t t_cache, int64_t B, int64_t W, int dtype, void *stream) {
  return rope_kv_append_impl(q, q_rs, k, k_rs, v, v_rs, cos_cached, sin_cached, max_pos, t, q_out, q_out_rs, k_cache, kc_rs, kc_bs,
                             v_cache, vc_rs, vc_bs, cap, t_cache, B, W, dtype, stream, AppendAt{nullptr, 0, 0, nullptr});
}

extern "C" int apertis_rope_kv_append_at(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                         const float *cos_cached, const float *sin_cached, int64_t max_pos, const int64_t *len,
                                         int64_t pos_offset, int32_t *err, void *q_out, int64_t q_out_rs, void *k_cache,
                                         int64_t kc_rs, int64_t kc_bs, void *v_cache, int64_t vc_rs, int64_t vc_bs, int64_t cap,
                                         int64_t B, int64_t W, int dtype, void *stream) {
  if (!len) return APERTIS_ERR_ARG;
  return rope_kv_append_impl(q, q_rs, k, k_rs, v, v_rs, cos_cached, sin_cached, max_pos, 0, q_out, q_out_rs, k_cache, kc_rs, kc_bs,
                             v_cache, vc_rs, vc_bs, cap, 0, B, W, dtype, stream, AppendAt{len, pos_offset, cap, err});
}

extern "C" int64_t apertis_attention_decode_splits(int64_t B, int64_t H, int64_t Lk, int64_t D) {
  if (B < 1 || H < 1 || Lk < 1 || D < 1) return -1;
  return decode_splits(B, H, Lk);
}

extern "C" int64_t apertis_attention_decode_workspace_bytes(int64_t B, int64_t H, int64_t D, int64_t splits) {
  if (B < 0 || H < 1 || D < 1 || splits < 1 || splits > APERTIS_ATTN_DECODE_MAX_SPLITS) return -1;
  return splits == 1 ? 0 : B * H * splits * (D + 2) * (int64_t)sizeof(float);
}

// both attentions: Lk by value (len null), or min(*len + 1, cap) read by the kernel with a split count the caller fixes
static int attention_decode_impl(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs, const void *v_cache,
                          int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *len, const int64_t *key_valid, int64_t kv_rs,
                          void *out, int64_t out_rs, float *workspace, int64_t B, int64_t Lk, int64_t H, int64_t D, int64_t splits,
                          int dtype, void *stream, int64_t window = 0) {
  if (!q || !k_cache || !v_cache || !out) return APERTIS_ERR_ARG;
  if (B < 0 || H <= 0 || D <= 0 || cap < 1 || Lk < 1 || Lk > cap || (dtype != APERTIS_F32 && dtype != APERTIS_BF16))
    return APERTIS_ERR_ARG;
  if ((D != 64 && D != 128) || B > 65535 || H > 65535) return APERTIS_ERR_UNSUPPORTED;
  const int64_t W = H * D, es = dtype == APERTIS_F32 ? 4 : 2;
  if (q_rs < W || out_rs < W || k_rs < W || v_rs < W || k_bs < cap * k_rs || v_bs < cap * v_rs) return APERTIS_ERR_ARG;
  if (key_valid && kv_rs < Lk) return APERTIS_ERR_ARG;
  if (splits < (len ? 1 : 0) || (!len && splits > Lk) || splits > APERTIS_ATTN_DECODE_MAX_SPLITS) return APERTIS_ERR_ARG;
  // 16-byte pieces of a head row: every row start on a 16-byte boundary
  const uint64_t bits = (uint64_t)(uintptr_t)q | (uint64_t)(uintptr_t)k_cache | (uint64_t)(uintptr_t)v_cache |
                        (uint64_t)(q_rs * es) | (uint64_t)(k_rs * es) | (uint64_t)(k_bs * es) | (uint64_t)(v_rs * es) |
                        (uint64_t)(v_bs * es);
  if (bits & 15u) return APERTIS_ERR_UNSUPPORTED;
  if (B == 0) return APERTIS_OK;
  if (splits == 0) splits = decode_splits(B, H, Lk);
  if (splits > 1 && !workspace) return APERTIS_ERR_ARG;
  DecArgs a{};
  a.q = q; a.k = k_cache; a.v = v_cache; a.key_valid = key_valid; a.out = out;
  a.ws_ml = workspace;
  a.ws_o = workspace ? workspace + 2 * B * H * splits : nullptr;
  a.q_rs = q_rs; a.k_rs = k_rs; a.k_bs = k_bs; a.v_rs = v_rs; a.v_bs = v_bs; a.kv_rs = kv_rs; a.out_rs = out_rs; a.Lk = Lk;
  a.len = len;
  a.window = window;                  // (0: the three entry points of the 4.12 table, attn_decode_k<.., false>)
  a.H = (int)H;
  a.splits = (int)splits;
  a.sl2 = (1.f / sqrtf((float)D)) * LOG2E_F;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == APERTIS_F32) return D == 64 ? launch_decode<float, 64>(a, B, st) : launch_decode<float, 128>(a, B, st);
  return D == 64 ? launch_decode<bf16_t, 64>(a, B, st) : launch_decode<bf16_t, 128>(a, B, st);
}

extern "C" int apertis_attention_decode(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs,
                                        const void *v_cache, int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *key_valid,
                                        int64_t kv_rs, void *out, int64_t out_rs, float *workspace, int64_t B, int64_t Lk, int64_t H,
                                        int64_t D, int64_t splits, int dtype, void *stream) {
  return attention_decode_impl(q, q_rs, k_cache, k_rs, k_bs, v_cache, v_rs, v_bs, cap, nullptr, key_valid, kv_rs, out, out_rs,
                               workspace, B, Lk, H, D, splits, dtype, stream);
}

extern "C" int apertis_attention_decode_at(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs,
                                           const void *v_cache, int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *len,
                                           const int64_t *key_valid, int64_t kv_rs, void *out, int64_t out_rs, float *workspace,
                                           int64_t B, int64_t H, int64_t D, int64_t splits, int dtype, void *stream) {
  if (!len) return APERTIS_ERR_ARG;
  // (Lk = cap for the shared checks: key_valid must cover every column the kernel can reach, and the kernel clamps to it)
  return attention_decode_impl(q, q_rs, k_cache, k_rs, k_bs, v_cache, v_rs, v_bs, cap, len, key_valid, kv_rs, out, out_rs, workspace,
                               B, cap, H, D, splits, dtype, stream);
}

// apertis_attention_decode_at under a sliding window (apertis_hip_ext.h): the kernel reads Lk as there and attends keys
// [max(Lk - window, 0), Lk) only, cut into the caller's fixed `splits`
extern "C" int apertis_attention_decode_window_at(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs,
                                                  const void *v_cache, int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *len,
                                                  int64_t window, const int64_t *key_valid, int64_t kv_rs, void *out, int64_t out_rs,
                                                  float *workspace, int64_t B, int64_t H, int64_t D, int64_t splits, int dtype,
                                                  void *stream) {
  if (!len || window < 1) return APERTIS_ERR_ARG;
  return attention_decode_impl(q, q_rs, k_cache, k_rs, k_bs, v_cache, v_rs, v_bs, cap, len, key_valid, kv_rs, out, out_rs, workspace,
                               B, cap, H, D, splits, dtype, stream, window);
}

extern "C" int apertis_rope_kv_append_chunk(const void *q, int64_t q_rs, int64_t q_bs, const void *k, int64_t k_rs, int64_t k_bs,
                                            const void *v, int64_t v_rs, int64_t v_bs, const float *cos_cached,
                                            const float *sin_cached, int64_t max_pos, int64_t t0, void *q_out, void *k_cache,
                                            int64_t kc_rs, int64_t kc_bs, void *v_cache, int64_t vc_rs, int64_t vc_bs, int64_t cap,
                                            int64_t t_cache0, int64_t B, int64_t Lq, int64_t W, int dtype, void *stream) {
  if (!q || !k || !v || !q_out || !k_cache || !v_cache || (cos_cached == nullptr) != (sin_cached == nullptr)) return APERTIS_ERR_ARG;
  if (B < 0 || Lq < 0 || W <= 0 || (W & 1) || cap < 1 || (dtype != APERTIS_F32 && dtype != APERTIS_BF16)) return APERTIS_ERR_ARG;
  if (q_rs < W || k_rs < W || v_rs < W || kc_rs < W || vc_rs < W || kc_bs < cap * kc_rs || vc_bs < cap * vc_rs) return APERTIS_ERR_ARG;
  if (Lq > 0 && (q_bs < Lq * q_rs || k_bs < Lq * k_rs || v_bs < Lq * v_rs)) return APERTIS_ERR_ARG;
  if (cos_cached && max_pos <= 0) return APERTIS_ERR_ARG;
  if (t_cache0 < 0 || t_cache0 > cap || Lq > cap - t_cache0) return APERTIS_ERR_ARG;
  if (cos_cached && Lq > 0 && (t0 < -max_pos || t0 >= max_pos || Lq > max_pos - t0)) return APERTIS_ERR_ARG;
  const int64_t half = W / 2, total = B * Lq * half;
  if (total == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  if (dtype == APERTIS_F32)
    hipLaunchKernelGGL((rope_kv_append_chunk_k<float>), grid, dim3(256), 0, st, (const float *)q, q_rs, q_bs, (const float *)k, k_rs,
                       k_bs, (const float *)v, v_rs, v_bs, cos_cached, sin_cached, max_pos, t0, (float *)q_out, (float *)k_cache,
                       kc_rs, kc_bs, (float *)v_cache, vc_rs, vc_bs, t_cache0, Lq, half, total);
  else
    hipLaunchKernelGGL((rope_kv_append_chunk_k<bf16_t>), grid, dim3(256), 0, st, (const bf16_t *)q, q_rs, q_bs, (const bf16_t *)k,
                       k_rs, k_bs, (const bf16_t *)v, v_rs, v_bs, cos_cached, sin_cached, max_pos, t0, (bf16_t *)q_out,
                       (bf16_t *)k_cache, kc_rs, kc_bs, (bf16_t *)v_cache, vc_rs, vc_bs, t_cache0, Lq, half, total);
  return apertis_check_launch();
}

extern "C" int64_t apertis_attention_chunk_splits(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t D) {
  if (B < 1 || H < 1 || Lq < 1 || Lk < Lq || D < 1) return -1;
  return chunk_splits(B, H, Lq, Lk);
}

extern "C" int64_t apertis_attention_chunk_workspace_bytes(int64_t B, int64_t H, int64_t Lq, int64_t D, int64_t splits) {
  if (B < 0 || H < 1 || Lq < 0 || D < 1 || splits < 1 || splits > APERTIS_ATTN_DECODE_MAX_SPLITS) return -1;
  return splits == 1 ? 0 : B * Lq * H * splits * (D + 2) * (int64_t)sizeof(float);
}

// both chunk attentions: window 0 is the plain causal form (attn_chunk_k<.., false>), else the keys a row sees
static int attention_chunk_impl(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs, const void *v_cache,
                                int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *key_valid, int64_t kv_rs, void *out,
                                int64_t out_rs, float *workspace, int64_t B, int64_t Lq, int64_t n, int64_t H, int64_t D,
                                int64_t splits, int dtype, void *stream, int64_t window) {
  if (!q || !k_cache || !v_cache || !out) return APERTIS_ERR_ARG;
  if (B < 0 || H <= 0 || D <= 0 || cap < 1 || Lq < 1 || n < 0 || n > cap || Lq > cap - n ||
      (dtype != APERTIS_F32 && dtype != APERTIS_BF16))
    return APERTIS_ERR_ARG;
  if ((D != 64 && D != 128) || B * H > 65535) return APERTIS_ERR_UNSUPPORTED;
  const int64_t W = H * D, es = dtype == APERTIS_F32 ? 4 : 2;
  if (q_rs < W || out_rs < W || k_rs < W || v_rs < W || k_bs < cap * k_rs || v_bs < cap * v_rs) return APERTIS_ERR_ARG;
  if (key_valid && kv_rs < n + Lq) return APERTIS_ERR_ARG;
  if (splits < 0 || splits > APERTIS_ATTN_DECODE_MAX_SPLITS) return APERTIS_ERR_ARG;
  // 16-byte row quarters and 16-byte stores of the output: every row start on a 16-byte boundary
  const uint64_t bits = (uint64_t)(uintptr_t)q | (uint64_t)(uintptr_t)k_cache | (uint64_t)(uintptr_t)v_cache |
                        (uint64_t)(uintptr_t)out | (uint64_t)(q_rs * es) | (uint64_t)(out_rs * es) | (uint64_t)(k_rs * es) |
                        (uint64_t)(k_bs * es) | (uint64_t)(v_rs * es) | (uint64_t)(v_bs * es);
  if (bits & 15u) return APERTIS_ERR_UNSUPPORTED;
  if (B == 0) return APERTIS_OK;
  // (under a window no wave walks more than window + Lq keys: the rule is asked at that length; no sizing point is measured for it)
  if (splits == 0) splits = chunk_splits(B, H, Lq, window > 0 && window < n ? window + Lq : n + Lq);
  if (splits > 1 && (!workspace || ((uintptr_t)workspace & 15u))) return APERTIS_ERR_ARG;
  ChunkArgs a{};
  a.q = q; a.k = k_cache; a.v = v_cache; a.key_valid = key_valid; a.out = out;
  a.ws_ml = workspace;
  a.ws_o = workspace ? workspace + 2 * B * Lq * H * splits : nullptr;
  a.q_rs = q_rs; a.k_rs = k_rs; a.k_bs = k_bs; a.v_rs = v_rs; a.v_bs = v_bs; a.kv_rs = kv_rs; a.out_rs = out_rs;
  a.Lq = Lq; a.n = n;
  a.window = window;
  a.H = (int)H;
  a.splits = (int)splits;
  a.scale = 1.f / sqrtf((float)D);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == APERTIS_F32) return D == 64 ? launch_chunk<float, 64>(a, B, st) : launch_chunk<float, 128>(a, B, st);
  return D == 64 ? launch_chunk<bf16_t, 64>(a, B, st) : launch_chunk<bf16_t, 128>(a, B, st);
}

extern "C" int apertis_attention_chunk(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs,
                                       const void *v_cache, int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *key_valid,
                                       int64_t kv_rs, void *out, int64_t out_rs, float *workspace, int64_t B, int64_t Lq, int64_t n,
                                       int64_t H, int64_t D, int64_t splits, int dtype, void *stream) {
  return attention_chunk_impl(q, q_rs, k_cache, k_rs, k_bs, v_cache, v_rs, v_bs, cap, key_valid, kv_rs, out, out_rs, workspace, B, Lq,
                              n, H, D, splits, dtype, stream, 0);
}

// apertis_attention_chunk under a sliding window (apertis_hip_ext.h): row i attends keys j with n + i - window < j <= n + i
extern "C" int apertis_attention_chunk_window(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs,
                                              const void *v_cache, int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *key_valid,
                                              int64_t kv_rs, void *out, int64_t out_rs, float *workspace, int64_t B, int64_t Lq,
                                              int64_t n, int64_t window, int64_t H, int64_t D, int64_t splits, int dtype,
                                              void *stream) {
  if (window < 1) return APERTIS_ERR_ARG;
  return attention_chunk_impl(q, q_rs, k_cache, k_rs, k_bs, v_cache, v_rs, v_bs, cap, key_valid, kv_rs, out, out_rs, workspace, B, Lq,
                              n, H, D, splits, dtype, stream, window);
}
