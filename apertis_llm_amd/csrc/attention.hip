// standard_mha on gfx950: interleaved-pair RoPE over the full projection width (reference core.py:258-293) and causal
// softmax attention (core.py:639-700, F.scaled_dot_product_attention with the causal / padding mask) as a flash-style
// kernel pair: forward with an online softmax that keeps LSE, backward that recomputes P from Q, K and LSE.
//
// Layout: Q, K, V, O and their gradients are token-major [B, L, H*D] with head h in columns [h*D, (h+1)*D) and a row
// stride per tensor (batch stride L * row stride): the projections' outputs are read and out_proj's input written as they
// are, no head transposes.  LSE is fp32 [B, H, L].
//
// One wave owns 16 rows (queries in the forward and the dQ kernel, keys in the dK/dV kernel) and walks the other side in
// tiles of 32; a work-group is 4 independent waves (64 rows).  Key tiles wholly above the diagonal are never touched.
// Two MFMA forms, the same for fp32 (v_mfma_f32_16x16x4_f32, exact fp32) and bf16 (v_mfma_f32_16x16x32_bf16):
//   rows form   C[i][j] = sum_d X[i][d] Y[j][d]   X, Y row tiles [16][D]; lane l reads the quarter row
//               X[l&15][g*D/4 ...] (g = l>>4) - any bijection of d works when both operands use the same one;
//               C lands as C[4g + r][l&15] (r = accumulator register).
//   column form C[d][j] += sum_k Z[k][d] R[k][j]  R a 32-row register tile made of two rows-form results (lane holds
//               R[16s + 4g + r][l&15]); k-slot t of lane group g is row 16(t>>2) + 4g + (t&3), Z is read at that row.
// Every product is oriented so that the later product sums over the row index of the earlier one (S^T = K Q^T then
// O^T += V^T P^T), so no accumulator ever changes lanes.  bf16: P and dS are rounded to bf16 for their products.
// The tiles and the forward's per-tile step live in attn_tile.h: the chunk kernel of attention_decode.hip runs the same step.
//
// CAUSAL = false is the bidirectional form (apertis_attention_full_fwd / _bwd: the vision tower): every wave walks every tile
// of the other side and the diagonal leaves the predicates; everything else - tiles, MFMA forms, dropout hash, one writer per
// output row - is shared.  A sequence with no valid key at all gets O = 0, LSE = +inf and zero gradients, which is what the
// causal form gives a row without a valid key.
//
// MASK_DOC (with CAUSAL) is the document-masked form of packed rows (apertis_attention_doc_fwd / _bwd): query i sees key j iff
// doc_start[b, i] <= j <= i, which for a key reads j <= i < doc_end[b, j] (documents are contiguous runs; start inclusive, end
// exclusive).  A wave's loop begins at the tile of the smallest start among its 16 queries (forward, dQ) and ends at the largest
// end among its 16 keys (dK/dV): both bounds are reduced over the 16 rows and broadcast, so they are wave-uniform.  A skipped
// tile is one in which no key counts for any query of the wave: attn_fwd_tile leaves (m, lsum, acc) as they were on such a tile
// while m = -inf, and the backward adds exact zeros, so skipping is bit-identical to walking.  The bounds are clamped to what the
// causal loops walk, so whatever the two arrays hold only masks: no address depends on them.
//
// MASK_WINDOW (with CAUSAL) is the sliding-window form (apertis_attention_window_fwd / _bwd): the same mask with bounds that are
// a function of the index and ONE scalar W - query i sees key j iff i - W < j <= i, which for a key reads j <= i < j + W.  Nothing
// is loaded and nothing reduced: a wave's first key tile is that of max(0, q0 - W + 1) (q0 its first query: the smallest start),
// its last query tile the one holding min(L, k0 + 15 + W) - 1.  The skip-equals-walk argument and the clamp are the document
// form's, so the bits are those of the document form fed start = max(0, i - W + 1), end = min(L, j + W).  Compared in 64 bits.
#include "attn_tile.h"
#include "rope_common.h"

namespace {

struct AttnArgs {
  const void *q, *k, *v, *o, *dout;
  int64_t q_rs, k_rs, v_rs, o_rs, do_rs, d_rs;
  const int64_t *key_valid;
  float *lse, *dsum;
  void *out, *dq, *dk, *dv;
  int64_t L;
  int H;
  float scale, inv_keep;
  uint64_t seed;
  uint32_t thresh16;
};
// what the MASK_DOC kernels take: AttnArgs and, per token, the first key / one past the last query of its document ([B, L])
struct DocArgs : AttnArgs {
  const int32_t *doc_start, *doc_end;
};
// the window kernels: AttnArgs and the number of keys a query sees, its own included (>= 1)
struct WindowArgs : AttnArgs {
  int64_t window;
};
// the mask on top of CAUSAL: none, the two arrays of packed rows, or the one scalar of a sliding window
enum Mask { MASK_NONE, MASK_DOC, MASK_WINDOW };
template <Mask M> using Args = std::conditional_t<M == MASK_DOC, DocArgs, std::conditional_t<M == MASK_WINDOW, WindowArgs, AttnArgs>>;

// smallest / largest value among the wave's 16 rows (lane & 15; the four lane groups hold copies), as a wave-uniform scalar
__device__ __forceinline__ int rows16_min(int v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = min(v, __shfl_xor(v, o));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int rows16_max(int v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = max(v, __shfl_xor(v, o));
  return __builtin_amdgcn_readfirstlane(v);
}

// ---------------------------------------------------------------------------------------------------------- forward
template <typename T, int D, bool DROP, bool CAUSAL, Mask M>
__global__ __launch_bounds__(256) void attn_fwd_k(Args<M> a) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t L = a.L;
  const int bh = blockIdx.y, H = a.H, b = bh / H, h = bh - b * H;
  const int64_t nblk = (L + WG_ROWS - 1) / WG_ROWS;
  // causal: heaviest blocks first; bidirectional: every block walks all of L, plain order
  const int64_t q0 = (CAUSAL ? nblk - 1 - blockIdx.x : (int64_t)blockIdx.x) * WG_ROWS + (threadIdx.x >> 6) * ROWS;
  if (q0 >= L) return;
  const T *qp = static_cast<const T *>(a.q) + (int64_t)b * L * a.q_rs + h * D;
  const T *kp = static_cast<const T *>(a.k) + (int64_t)b * L * a.k_rs + h * D;
  const T *vp = static_cast<const T *>(a.v) + (int64_t)b * L * a.v_rs + h * D;
  const int64_t *kv = a.key_valid ? a.key_valid + (int64_t)b * L : nullptr;
  const int64_t qi = q0 + c;                               // this lane's query
  Quarter<T, D> qf;
  load_quarter(qf, qp + qi * a.q_rs + g * (D / 4), qi < L);
  const float sl2 = a.scale * LOG2E_F;
  float m = -INFINITY, lsum = 0.f;                         // m in log2 units of the scaled score
  f32x4 acc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t last = CAUSAL ? min(q0 + ROWS - 1, L - 1) : L - 1;
  const uint64_t drow = (uint64_t)bh * (uint64_t)L + (uint64_t)qi;
  int64_t qs = 0, kb0 = 0;                                 // DOC: this query's first key; the wave's first tile
  if constexpr (M == MASK_DOC) {
    qs = qi < L ? a.doc_start[(int64_t)b * L + qi] : INT32_MAX;
    kb0 = min((int64_t)max(rows16_min((int)qs), 0), q0) & ~(int64_t)(TILE - 1);
  }
  // WINDOW: q0 >= 0 and W >= 1, so the difference cannot wrap; the per-lane predicate needs no bound of its own - the
  // diagonal and the window are ONE unsigned compare of the distance qi - key against the scalar W
  if constexpr (M == MASK_WINDOW) kb0 = window_first_tile(q0, a.window);
  for (int64_t kb = kb0; kb <= last; kb += TILE) {
    const int64_t nrows = L - kb;
    attn_fwd_tile<T, D>(
        qf, kp, a.k_rs, vp, a.v_rs, kb, sl2, m, lsum, acc, lane, [=](int64_t kr) { return kr < L; },
        [=](int t) {
          const int64_t key = kb + tile_row(g, t);
          bool ok;
          if constexpr (M == MASK_WINDOW) ok = (uint64_t)(qi - key) < (uint64_t)a.window && key < L;
          else if constexpr (CAUSAL) ok = key <= qi && key < L;
          else ok = key < L;
          if constexpr (M == MASK_DOC) ok = ok && key >= qs;
          if (kv && ok) ok = kv[key] != 0;
          return ok;
        },
        RowsBelow{g, nrows < TILE ? (int)nrows : TILE},
        [=](float p, int t) {
          if constexpr (DROP) return drop_keep(a.seed, (int64_t)drow, kb + tile_row(g, t), L, a.thresh16) ? p * a.inv_keep : 0.f;
          else return p;
        });
  }
  const float l = xor_sum(lsum);
  if (qi >= L) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  store_cols<T, D>(static_cast<T *>(a.out) + (int64_t)b * L * a.o_rs + qi * a.o_rs + h * D, acc, inv, lane);
  if (g == 0) a.lse[(int64_t)bh * L + qi] = l > 0.f ? m / LOG2E_F + logf(l) : INFINITY;
}

// ---------------------------------------------------------------------------------------------------------- backward
// dsum[b, h, i] = sum_d dO[i][d] * O[i][d]  (fp32); one thread per (b, i, h)
template <typename T, int D>
__global__ __launch_bounds__(256) void attn_dsum_k(AttnArgs a, int64_t rows) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * a.H) return;
  const int64_t bi = t / a.H;
  const int h = (int)(t - bi * a.H);
  const int64_t b = bi / a.L, i = bi - b * a.L;
  const T *o = static_cast<const T *>(a.o) + bi * a.o_rs + h * D;
  const T *d = static_cast<const T *>(a.dout) + bi * a.do_rs + h * D;
  float s = 0.f;
#pragma unroll 8
  for (int e = 0; e < D; ++e) s += to_f32(o[e]) * to_f32(d[e]);
  a.dsum[(b * a.H + h) * a.L + i] = s;
}

// dK, dV for the 16 keys of a wave: loop over the query tiles at or below the diagonal (bidirectional: over all of them)
template <typename T, int D, bool DROP, bool CAUSAL, Mask M>
__global__ __launch_bounds__(256) void attn_bwd_dkv_k(Args<M> a) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t L = a.L;
  const int bh = blockIdx.y, H = a.H, b = bh / H, h = bh - b * H;
  const int64_t k0 = (int64_t)blockIdx.x * WG_ROWS + (threadIdx.x >> 6) * ROWS;   // block 0 (the longest walk) first
  if (k0 >= L) return;
  const int64_t bo = (int64_t)b * L;
  const T *qp = static_cast<const T *>(a.q) + bo * a.q_rs + h * D;
  const T *kp = static_cast<const T *>(a.k) + bo * a.k_rs + h * D;
  const T *vp = static_cast<const T *>(a.v) + bo * a.v_rs + h * D;
  const T *dop = static_cast<const T *>(a.dout) + bo * a.do_rs + h * D;
  const float *lse = a.lse + (int64_t)bh * L, *dsum = a.dsum + (int64_t)bh * L;
  const int64_t kj = k0 + c;                               // this lane's key
  bool kok = kj < L;
  if (a.key_valid && kok) kok = a.key_valid[bo + kj] != 0;
  Quarter<T, D> kf, vf;
  load_quarter(kf, kp + kj * a.k_rs + g * (D / 4), kj < L);
  load_quarter(vf, vp + kj * a.v_rs + g * (D / 4), kj < L);
  const float sl2 = a.scale * LOG2E_F;
  f32x4 dk[D / 16], dv[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) dk[dt] = dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  int64_t ke = L, qend = L;                                // DOC: one past this key's last query; the wave's last query + 1
  if constexpr (M == MASK_DOC) {
    ke = kj < L ? a.doc_end[bo + kj] : 0;
    qend = min((int64_t)rows16_max((int)ke), L);
  }
  // WINDOW: W >= L is every query at or below the diagonal; else the sum is < 2 L + 15 and cannot wrap
  if constexpr (M == MASK_WINDOW) qend = a.window >= L ? L : min(k0 + ROWS - 1 + a.window, L);
  for (int64_t qb = CAUSAL ? k0 & ~(int64_t)(TILE - 1) : 0; qb < qend; qb += TILE) {
    f32x4 pd[2], ds[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Quarter<T, D> qf, df;
      const int64_t qr = qb + 16 * s + c;
      load_quarter(qf, qp + qr * a.q_rs + g * (D / 4), qr < L);
      load_quarter(df, dop + qr * a.do_rs + g * (D / 4), qr < L);
      f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
      dot_rows<D>(sv, qf, kf);                             // S[query 16s+4g+r][key c]
      dot_rows<D>(dp, df, vf);                             // dP (of the dropped P)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t qi = qb + 16 * s + 4 * g + r;
        bool ok;
        if constexpr (M == MASK_WINDOW) ok = kok && qi < L && (uint64_t)(qi - kj) < (uint64_t)a.window;
        else if constexpr (CAUSAL) ok = kok && qi < L && kj <= qi;
        else ok = kok && qi < L;
        if constexpr (M == MASK_DOC) ok = ok && qi < ke;
        const float p = ok ? exp2f(sv[r] * sl2 - lse[qi] * LOG2E_F) : 0.f;
        float dpr = dp[r], pdr = p;
        if constexpr (DROP) {
          const bool keep = drop_keep(a.seed, (int64_t)((uint64_t)bh * (uint64_t)L + (uint64_t)qi), kj, L, a.thresh16);
          pdr = keep ? p * a.inv_keep : 0.f;
          dpr = keep ? dpr * a.inv_keep : 0.f;
        }
        pd[s][r] = pdr;
        ds[s][r] = ok ? p * (dpr - dsum[qi]) : 0.f;
      }
    }
    const int64_t nrows = L - qb;
    const RowsBelow rows{g, nrows < TILE ? (int)nrows : TILE};
    acc_cols<D>(dv, dop + qb * a.do_rs, a.do_rs, rows, pd, lane);
    acc_cols<D>(dk, qp + qb * a.q_rs, a.q_rs, rows, ds, lane);
  }
  if (kj >= L) return;
  store_cols<T, D>(static_cast<T *>(a.dk) + (bo + kj) * a.d_rs + h * D, dk, a.scale, lane);
  store_cols<T, D>(static_cast<T *>(a.dv) + (bo + kj) * a.d_rs + h * D, dv, 1.f, lane);
}

// dQ for the 16 queries of a wave: loop over the key tiles at or below the diagonal (bidirectional: over all of them)
template <typename T, int D, bool DROP, bool CAUSAL, Mask M>
__global__ __launch_bounds__(256) void attn_bwd_dq_k(Args<M> a) {
  const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
  const int64_t L = a.L;
  const int bh = blockIdx.y, H = a.H, b = bh / H, h = bh - b * H;
  const int64_t nblk = (L + WG_ROWS - 1) / WG_ROWS;
  const int64_t q0 = (CAUSAL ? nblk - 1 - blockIdx.x : (int64_t)blockIdx.x) * WG_ROWS + (threadIdx.x >> 6) * ROWS;
  if (q0 >= L) return;
  const int64_t bo = (int64_t)b * L;
  const T *qp = static_cast<const T *>(a.q) + bo * a.q_rs + h * D;
  const T *kp = static_cast<const T *>(a.k) + bo * a.k_rs + h * D;
  const T *vp = static_cast<const T *>(a.v) + bo * a.v_rs + h * D;
  const T *dop = static_cast<const T *>(a.dout) + bo * a.do_rs + h * D;
  const int64_t *kv = a.key_valid ? a.key_valid + bo : nullptr;
  const int64_t qi = q0 + c;
  const bool qok = qi < L;
  Quarter<T, D> qf, df;
  load_quarter(qf, qp + qi * a.q_rs + g * (D / 4), qok);
  load_quarter(df, dop + qi * a.do_rs + g * (D / 4), qok);
  const float lse2 = qok ? a.lse[(int64_t)bh * L + qi] * LOG2E_F : INFINITY;
  const float dsq = qok ? a.dsum[(int64_t)bh * L + qi] : 0.f;
  const float sl2 = a.scale * LOG2E_F;
  const uint64_t drow = (uint64_t)bh * (uint64_t)L + (uint64_t)qi;
  f32x4 dq[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int64_t last = CAUSAL ? min(q0 + ROWS - 1, L - 1) : L - 1;
  int64_t qs = 0, kb0 = 0;                                 // DOC: as in the forward
  if constexpr (M == MASK_DOC) {
    qs = qok ? a.doc_start[bo + qi] : INT32_MAX;
    kb0 = min((int64_t)max(rows16_min((int)qs), 0), q0) & ~(int64_t)(TILE - 1);
  }
  if constexpr (M == MASK_WINDOW) kb0 = window_first_tile(q0, a.window);
  for (int64_t kb = kb0; kb <= last; kb += TILE) {
    f32x4 ds[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Quarter<T, D> kf, vf;
      const int64_t kr = kb + 16 * s + c;
      load_quarter(kf, kp + kr * a.k_rs + g * (D / 4), kr < L);
      load_quarter(vf, vp + kr * a.v_rs + g * (D / 4), kr < L);
      f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
      dot_rows<D>(sv, kf, qf);                             // S^T[key 16s+4g+r][query c]
      dot_rows<D>(dp, vf, df);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t key = kb + 16 * s + 4 * g + r;
        bool ok;
        if constexpr (M == MASK_WINDOW) ok = qok && (uint64_t)(qi - key) < (uint64_t)a.window;
        else if constexpr (CAUSAL) ok = qok && key <= qi;
        else ok = qok && key < L;
        if constexpr (M == MASK_DOC) ok = ok && key >= qs;
        if (kv && ok) ok = kv[key] != 0;
        const float p = ok ? exp2f(sv[r] * sl2 - lse2) : 0.f;
        float dpr = dp[r];
        if constexpr (DROP) dpr = drop_keep(a.seed, (int64_t)drow, key, L, a.thresh16) ? dpr * a.inv_keep : 0.f;
        ds[s][r] = ok ? p * (dpr - dsq) : 0.f;
      }
    }
    const int64_t nrows = L - kb;
    acc_cols<D>(dq, kp + kb * a.k_rs, a.k_rs, RowsBelow{g, nrows < TILE ? (int)nrows : TILE}, ds, lane);
  }
  if (!qok) return;
  store_cols<T, D>(static_cast<T *>(a.dq) + (bo + qi) * a.d_rs + h * D, dq, a.scale, lane);
}

template <typename T, int D, bool DROP, bool CAUSAL, Mask M> int launch_fwd(const Args<M> &a, int64_t B, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div64(a.L, WG_ROWS), (unsigned)(B * a.H));
  hipLaunchKernelGGL((attn_fwd_k<T, D, DROP, CAUSAL, M>), grid, dim3(256), 0, st, a);
  return apertis_check_launch();
}
template <typename T, int D, bool DROP, bool CAUSAL, Mask M> int launch_bwd(const Args<M> &a, int64_t B, hipStream_t st) {
  const int64_t rows = B * a.L;
  hipLaunchKernelGGL((attn_dsum_k<T, D>), dim3((unsigned)ceil_div64(rows * a.H, 256)), dim3(256), 0, st, (const AttnArgs &)a, rows);
  const dim3 grid((unsigned)ceil_div64(a.L, WG_ROWS), (unsigned)(B * a.H));
  hipLaunchKernelGGL((attn_bwd_dkv_k<T, D, DROP, CAUSAL, M>), grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL((attn_bwd_dq_k<T, D, DROP, CAUSAL, M>), grid, dim3(256), 0, st, a);
  return apertis_check_launch();
}

template <bool BWD, bool CAUSAL, Mask M> int dispatch(const Args<M> &a, int64_t B, int64_t D, int dtype, bool drop, hipStream_t st) {
#define APERTIS_ATTN_CASE(T, DD)                                                                                                \
  if (D == DD) {                                                                                                                \
    if constexpr (BWD) return drop ? launch_bwd<T, DD, true, CAUSAL, M>(a, B, st) : launch_bwd<T, DD, false, CAUSAL, M>(a, B, st); \
    else return drop ? launch_fwd<T, DD, true, CAUSAL, M>(a, B, st) : launch_fwd<T, DD, false, CAUSAL, M>(a, B, st);      \
  }
  if (dtype == APERTIS_F32) {
    APERTIS_ATTN_CASE(float, 64)
    APERTIS_ATTN_CASE(float, 128)
  } else {
    APERTIS_ATTN_CASE(bf16_t, 64)
    APERTIS_ATTN_CASE(bf16_t, 128)
  }
#undef APERTIS_ATTN_CASE
  return APERTIS_ERR_UNSUPPORTED;
}

// shape / pointer checks shared by both directions; 0, or the error code
int attn_check(std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> strides, int64_t B, int64_t L, int64_t H,
               int64_t D, float p, int dtype) {
  for (const void *q : ptrs)
    if (!q) return APERTIS_ERR_ARG;
  if (B < 0 || L < 0 || H <= 0 || D <= 0 || !(p >= 0.f && p < 1.f) || (dtype != APERTIS_F32 && dtype != APERTIS_BF16))
    return APERTIS_ERR_ARG;
  if ((D != 64 && D != 128) || B * H > 65535) return APERTIS_ERR_UNSUPPORTED;
  const int64_t es = dtype == APERTIS_F32 ? 4 : 2;
  for (int64_t rs : strides)
    if (rs < H * D) return APERTIS_ERR_ARG;
  // 16-byte row quarters: every row start and head offset on a 16-byte boundary
  uint64_t bits = 0;
  for (const void *q : ptrs) bits |= (uint64_t)(uintptr_t)q;
  for (int64_t rs : strides) bits |= (uint64_t)(rs * es);
  if (bits & 15u) return APERTIS_ERR_UNSUPPORTED;
  return APERTIS_OK;
}

AttnArgs make_args(int64_t L, int64_t H, int64_t D, float p, uint64_t seed) {
  AttnArgs a{};
  a.L = L;
  a.H = (int)H;
  a.scale = 1.f / sqrtf((float)D);
  a.inv_keep = 1.f / (1.f - p);
  a.seed = seed;
  a.thresh16 = (uint32_t)(p * 65536.f);
  return a;
}

// ---------------------------------------------------------------------------------------------------------- RoPE
// one thread per (token, pair j) rotates pair j of q and of k; BWD applies the transpose of the rotation
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void rope_qk_k(const T *q, int64_t q_rs, const T *k, int64_t k_rs, const int64_t *pos,
                                                 int64_t pos_bs, const float *cs, const float *sn, int64_t max_pos, T *qo,
                                                 T *ko, int64_t L, int64_t half, int64_t total) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t tok = t / half, j = t - tok * half;
  const int64_t b = tok / L, l = tok - b * L;
  float c, s;                                                // (table lookup and pair arithmetic: rope_common.h)
  rope_cos_sin(cs, sn, pos ? pos[b * pos_bs + l] : l, max_pos, half, j, c, s);
  const T *src[2] = {q + tok * q_rs, k + tok * k_rs};
  T *dst[2] = {qo + tok * 2 * half, ko + tok * 2 * half};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    float y0, y1;
    rope_rotate_pair<BWD>(to_f32(src[u][2 * j]), to_f32(src[u][2 * j + 1]), c, s, y0, y1);
    dst[u][2 * j] = from_f32<T>(y0);
    dst[u][2 * j + 1] = from_f32<T>(y1);
  }
}

template <bool BWD>
int rope_entry(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const int64_t *pos, int64_t pos_bs, const float *cs,
               const float *sn, int64_t max_pos, void *qo, void *ko, int64_t B, int64_t L, int64_t W, int dtype, void *stream) {
  if (!q || !k || !cs || !sn || !qo || !ko) return APERTIS_ERR_ARG;
  if (B < 0 || L < 0 || W <= 0 || (W & 1) || q_rs < W || k_rs < W || pos_bs < 0 || max_pos <= 0) return APERTIS_ERR_ARG;
  if (dtype != APERTIS_F32 && dtype != APERTIS_BF16) return APERTIS_ERR_ARG;
  if (!pos && L > max_pos) return APERTIS_ERR_ARG;
  const int64_t half = W / 2, total = B * L * half;
  if (total == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  if (dtype == APERTIS_F32)
    hipLaunchKernelGGL((rope_qk_k<float, BWD>), grid, dim3(256), 0, st, (const float *)q, q_rs, (const float *)k, k_rs, pos,
                       pos_bs, cs, sn, max_pos, (float *)qo, (float *)ko, L, half, total);
  else
    hipLaunchKernelGGL((rope_qk_k<bf16_t, BWD>), grid, dim3(256), 0, st, (const bf16_t *)q, q_rs, (const bf16_t *)k, k_rs, pos,
                       pos_bs, cs, sn, max_pos, (bf16_t *)qo, (bf16_t *)ko, L, half, total);
  return apertis_check_launch();
}

// MASK_DOC: doc_start / doc_end are checked with the other pointers (null: APERTIS_ERR_ARG); else they are not looked at.
// MASK_WINDOW: window < 1 is APERTIS_ERR_ARG, and so is L > INT32_MAX as for MASK_DOC; else it is not looked at
template <bool CAUSAL, Mask M = MASK_NONE>
int attention_fwd_entry(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs, const int64_t *key_valid,
                        void *out, int64_t out_rs, float *lse, int64_t B, int64_t L, int64_t H, int64_t D, float dropout_p,
                        uint64_t seed, int dtype, void *stream, const int32_t *doc_start = nullptr,
                        const int32_t *doc_end = nullptr, int64_t window = 0) {
  if (M == MASK_DOC && (!doc_start || !doc_end || L > INT32_MAX)) return APERTIS_ERR_ARG;
  if (M == MASK_WINDOW && (window < 1 || L > INT32_MAX)) return APERTIS_ERR_ARG;
  const int rc = attn_check({q, k, v, out, lse}, {q_rs, k_rs, v_rs, out_rs}, B, L, H, D, dropout_p, dtype);
  if (rc) return rc;
  if (B == 0 || L == 0) return APERTIS_OK;
  Args<M> a{};
  static_cast<AttnArgs &>(a) = make_args(L, H, D, dropout_p, seed);
  a.q = q; a.k = k; a.v = v; a.out = out; a.lse = lse; a.key_valid = key_valid;
  a.q_rs = q_rs; a.k_rs = k_rs; a.v_rs = v_rs; a.o_rs = out_rs;
  if constexpr (M == MASK_DOC) { a.doc_start = doc_start; a.doc_end = doc_end; }
  if constexpr (M == MASK_WINDOW) a.window = window;
  return dispatch<false, CAUSAL, M>(a, B, D, dtype, dropout_p > 0.f, (hipStream_t)stream);
}

template <bool CAUSAL, Mask M = MASK_NONE>
int attention_bwd_entry(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs, const void *out,
                        int64_t out_rs, const void *dout, int64_t dout_rs, const float *lse, const int64_t *key_valid,
                        float *workspace, void *dq, void *dk, void *dv, int64_t d_rs, int64_t B, int64_t L, int64_t H, int64_t D,
                        float dropout_p, uint64_t seed, int dtype, void *stream, const int32_t *doc_start = nullptr,
                        const int32_t *doc_end = nullptr, int64_t window = 0) {
  if (M == MASK_DOC && (!doc_start || !doc_end || L > INT32_MAX)) return APERTIS_ERR_ARG;
  if (M == MASK_WINDOW && (window < 1 || L > INT32_MAX)) return APERTIS_ERR_ARG;
  const int rc = attn_check({q, k, v, out, dout, lse, workspace, dq, dk, dv}, {q_rs, k_rs, v_rs, out_rs, dout_rs, d_rs}, B, L,
                            H, D, dropout_p, dtype);
  if (rc) return rc;
  if (B == 0 || L == 0) return APERTIS_OK;
  Args<M> a{};
  static_cast<AttnArgs &>(a) = make_args(L, H, D, dropout_p, seed);
  a.q = q; a.k = k; a.v = v; a.o = out; a.dout = dout; a.lse = (float *)lse; a.key_valid = key_valid; a.dsum = workspace;
  a.dq = dq; a.dk = dk; a.dv = dv;
  a.q_rs = q_rs; a.k_rs = k_rs; a.v_rs = v_rs; a.o_rs = out_rs; a.do_rs = dout_rs; a.d_rs = d_rs;
  if constexpr (M == MASK_DOC) { a.doc_start = doc_start; a.doc_end = doc_end; }
  if constexpr (M == MASK_WINDOW) a.window = window;
  return dispatch<true, CAUSAL, M>(a, B, D, dtype, dropout_p > 0.f, (hipStream_t)stream);
}

}  // namespace

extern "C" int apertis_rope_qk_fwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const int64_t *position_ids,
                                   int64_t pos_batch_stride, const float *cos_cached, const float *sin_cached, int64_t max_pos,
                                   void *q_out, void *k_out, int64_t B, int64_t L, int64_t W, int dtype, void *stream) {
  return rope_entry<false>(q, q_rs, k, k_rs, position_ids, pos_batch_stride, cos_cached, sin_cached, max_pos, q_out, k_out, B,
                           L, W, dtype, stream);
}

extern "C" int apertis_rope_qk_bwd(const void *dq_out, int64_t dq_rs, const void *dk_out, int64_t dk_rs,
                                   const int64_t *position_ids, int64_t pos_batch_stride, const float *cos_cached,
                                   const float *sin_cached, int64_t max_pos, void *dq, void *dk, int64_t B, int64_t L, int64_t W,
                                   int dtype, void *stream) {
  return rope_entry<true>(dq_out, dq_rs, dk_out, dk_rs, position_ids, pos_batch_stride, cos_cached, sin_cached, max_pos, dq, dk,
                          B, L, W, dtype, stream);
}

extern "C" int apertis_attention_fwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                     const int64_t *key_valid, void *out, int64_t out_rs, float *lse, int64_t B, int64_t L,
                                     int64_t H, int64_t D, float dropout_p, uint64_t seed, int dtype, void *stream) {
  return attention_fwd_entry<true>(q, q_rs, k, k_rs, v, v_rs, key_valid, out, out_rs, lse, B, L, H, D, dropout_p, seed, dtype, stream);
}

extern "C" int64_t apertis_attention_bwd_workspace_bytes(int64_t B, int64_t L, int64_t H) {
  if (B < 0 || L < 0 || H <= 0) return -1;
  return B * H * L * (int64_t)sizeof(float);
}

extern "C" int apertis_attention_bwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                     const void *out, int64_t out_rs, const void *dout, int64_t dout_rs, const float *lse,
                                     const int64_t *key_valid, float *workspace, void *dq, void *dk, void *dv, int64_t d_rs,
                                     int64_t B, int64_t L, int64_t H, int64_t D, float dropout_p, uint64_t seed, int dtype,
                                     void *stream) {
  return attention_bwd_entry<true>(q, q_rs, k, k_rs, v, v_rs, out, out_rs, dout, dout_rs, lse, key_valid, workspace, dq, dk, dv, d_rs,
                                   B, L, H, D, dropout_p, seed, dtype, stream);
}

// the bidirectional pair (the vision tower): the same checks, the CAUSAL = false kernels
extern "C" int apertis_attention_full_fwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                          const int64_t *key_valid, void *out, int64_t out_rs, float *lse, int64_t B, int64_t L,
                                          int64_t H, int64_t D, float dropout_p, uint64_t seed, int dtype, void *stream) {
  return attention_fwd_entry<false>(q, q_rs, k, k_rs, v, v_rs, key_valid, out, out_rs, lse, B, L, H, D, dropout_p, seed, dtype, stream);
}

extern "C" int apertis_attention_full_bwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                          const void *out, int64_t out_rs, const void *dout, int64_t dout_rs, const float *lse,
                                          const int64_t *key_valid, float *workspace, void *dq, void *dk, void *dv, int64_t d_rs,
                                          int64_t B, int64_t L, int64_t H, int64_t D, float dropout_p, uint64_t seed, int dtype,
                                          void *stream) {
  return attention_bwd_entry<false>(q, q_rs, k, k_rs, v, v_rs, out, out_rs, dout, dout_rs, lse, key_valid, workspace, dq, dk, dv, d_rs,
                                    B, L, H, D, dropout_p, seed, dtype, stream);
}

// the document-masked causal pair (packed rows): the same checks, null doc_start / doc_end refused, the MASK_DOC kernels
extern "C" int apertis_attention_doc_fwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                         const int64_t *key_valid, const int32_t *doc_start, const int32_t *doc_end, void *out,
                                         int64_t out_rs, float *lse, int64_t B, int64_t L, int64_t H, int64_t D, float dropout_p,
                                         uint64_t seed, int dtype, void *stream) {
  return attention_fwd_entry<true, MASK_DOC>(q, q_rs, k, k_rs, v, v_rs, key_valid, out, out_rs, lse, B, L, H, D, dropout_p, seed, dtype,
                                         stream, doc_start, doc_end);
}

extern "C" int apertis_attention_doc_bwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                         const void *out, int64_t out_rs, const void *dout, int64_t dout_rs, const float *lse,
                                         const int64_t *key_valid, const int32_t *doc_start, const int32_t *doc_end,
                                         float *workspace, void *dq, void *dk, void *dv, int64_t d_rs, int64_t B, int64_t L,
                                         int64_t H, int64_t D, float dropout_p, uint64_t seed, int dtype, void *stream) {
  return attention_bwd_entry<true, MASK_DOC>(q, q_rs, k, k_rs, v, v_rs, out, out_rs, dout, dout_rs, lse, key_valid, workspace, dq, dk, dv,
                                         d_rs, B, L, H, D, dropout_p, seed, dtype, stream, doc_start, doc_end);
}

// the sliding-window causal pair: the same checks, window < 1 refused, the MASK_WINDOW kernels
extern "C" int apertis_attention_window_fwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                            const int64_t *key_valid, int64_t window, void *out, int64_t out_rs, float *lse,
                                            int64_t B, int64_t L, int64_t H, int64_t D, float dropout_p, uint64_t seed, int dtype,
                                            void *stream) {
  return attention_fwd_entry<true, MASK_WINDOW>(q, q_rs, k, k_rs, v, v_rs, key_valid, out, out_rs, lse, B, L, H, D, dropout_p, seed,
                                                dtype, stream, nullptr, nullptr, window);
}

extern "C" int apertis_attention_window_bwd(const void *q, int64_t q_rs, const void *k, int64_t k_rs, const void *v, int64_t v_rs,
                                            const void *out, int64_t out_rs, const void *dout, int64_t dout_rs, const float *lse,
                                            const int64_t *key_valid, int64_t window, float *workspace, void *dq, void *dk, void *dv,
                                            int64_t d_rs, int64_t B, int64_t L, int64_t H, int64_t D, float dropout_p, uint64_t seed,
                                            int dtype, void *stream) {
  return attention_bwd_entry<true, MASK_WINDOW>(q, q_rs, k, k_rs, v, v_rs, out, out_rs, dout, dout_rs, lse, key_valid, workspace, dq,
                                                dk, dv, d_rs, B, L, H, D, dropout_p, seed, dtype, stream, nullptr, nullptr, window);
}
