// The register tiles of the attention kernels (attention.hip: forward and backward; attention_decode.hip: the chunk kernel
// against the KV cache) and ONE statement of the forward's per-tile step, so that attn_fwd_k and attn_chunk_k give a query the
// same bits.  The MFMA forms and their lane layouts are described at the top of attention.hip.  Anonymous namespace: a copy per
// translation unit.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) bf16_t bf16x8;

constexpr int ROWS = 16;       // rows per wave
constexpr int TILE = 32;       // columns per step of a wave's loop
constexpr int WAVES = 4;       // waves per work-group
constexpr int WG_ROWS = ROWS * WAVES;

// the lane's quarter of one head row: D/4 contiguous elements starting at column (lane>>4)*D/4
template <typename T, int D> struct Quarter {
  static constexpr int N = D / 4;
  static constexpr int V = N * (int)sizeof(T) / 16;     // 16-byte loads
  uint4 raw[V];
};

template <typename T, int D>
__device__ __forceinline__ void load_quarter(Quarter<T, D> &f, const T *row, bool ok) {
  if (ok) {
    const uint4 *p = reinterpret_cast<const uint4 *>(row);
#pragma unroll
    for (int i = 0; i < Quarter<T, D>::V; ++i) f.raw[i] = p[i];
  } else {
#pragma unroll
    for (int i = 0; i < Quarter<T, D>::V; ++i) f.raw[i] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// rows form
template <int D>
__device__ __forceinline__ void dot_rows(f32x4 &acc, const Quarter<bf16_t, D> &a, const Quarter<bf16_t, D> &b) {
#pragma unroll
  for (int i = 0; i < Quarter<bf16_t, D>::V; ++i)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a.raw[i]), __builtin_bit_cast(bf16x8, b.raw[i]),
                                                  acc, 0, 0, 0);
}
template <int D>
__device__ __forceinline__ void dot_rows(f32x4 &acc, const Quarter<float, D> &a, const Quarter<float, D> &b) {
#pragma unroll
  for (int i = 0; i < Quarter<float, D>::V; ++i) {
    const f32x4 av = __builtin_bit_cast(f32x4, a.raw[i]), bv = __builtin_bit_cast(f32x4, b.raw[i]);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc, 0, 0, 0);
  }
}

__device__ __forceinline__ int tile_row(int g, int t) { return 16 * (t >> 2) + 4 * g + (t & 3); }

// column form: acc[dt] holds C[d = 16dt + 4g + r][l&15]; z points at row 0 / column 0 of this tile's head slice,
// the row of k-slot t reads as zero (never dereferenced) unless row_ok(t)
template <int D, typename RowOk>
__device__ __forceinline__ void acc_cols(f32x4 (&acc)[D / 16], const bf16_t *z, int64_t z_rs, RowOk row_ok, const f32x4 (&R)[2],
                                         int lane) {
  const int g = lane >> 4, c = lane & 15;
  bf16x8 b;
#pragma unroll
  for (int t = 0; t < 8; ++t) b[t] = (bf16_t)R[t >> 2][t & 3];
  int64_t off[8];
  bool ok[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int kr = tile_row(g, t);
    ok[t] = row_ok(t);
    off[t] = (int64_t)kr * z_rs + c;
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    bf16x8 a;
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = ok[t] ? z[off[t] + 16 * dt] : (bf16_t)0.f;
    acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[dt], 0, 0, 0);
  }
}
template <int D, typename RowOk>
__device__ __forceinline__ void acc_cols(f32x4 (&acc)[D / 16], const float *z, int64_t z_rs, RowOk row_ok, const f32x4 (&R)[2],
                                         int lane) {
  const int g = lane >> 4, c = lane & 15;
  int64_t off[8];
  bool ok[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int kr = tile_row(g, t);
    ok[t] = row_ok(t);
    off[t] = (int64_t)kr * z_rs + c;
  }
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float a = ok[t] ? z[off[t] + 16 * dt] : 0.f;
      acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, R[t >> 2][t & 3], acc[dt], 0, 0, 0);
    }
  }
}

// row d = 16dt + 4g + r of a column-form accumulator, stored as 4 consecutive elements of output row `row`
template <typename T, int D>
__device__ __forceinline__ void store_cols(T *row, const f32x4 (&acc)[D / 16], float s, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    T *p = row + 16 * dt + 4 * g;
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<f32x4 *>(p) = acc[dt] * s;
    } else {
      typedef __attribute__((ext_vector_type(4))) bf16_t bf16x4;
      bf16x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (bf16_t)(acc[dt][r] * s);
      *reinterpret_cast<bf16x4 *>(p) = v;
    }
  }
}

__device__ __forceinline__ float xor_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float xor_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// rows below `nr` of a tile (the forward and the backward: a tile that runs past the sequence end)
struct RowsBelow {
  int g, nr;
  __device__ __forceinline__ bool operator()(int t) const { return tile_row(g, t) < nr; }
};

// Sliding window (the forward, the dQ kernel, attn_chunk_k): the first key of the wave's first tile for a wave whose first row
// sits at key position q0, max(0, q0 - W + 1) rounded down to a tile (q0 >= 0 and W >= 1: the difference cannot wrap).  q0 comes
// from threadIdx.x >> 6, which the compiler cannot see is wave-uniform; read through lane 0 the loop counter and the tile
// addresses built from it stay scalar.  (Read as a TILE INDEX in 32 bits: the window pair refuses L > INT32_MAX as the document
// pair does, and a KV cache of 2^36 rows does not exist.)
__device__ __forceinline__ int64_t window_first_tile(int64_t q0, int64_t window) {
  const int64_t first = max(q0 - window + 1, (int64_t)0) / TILE;
  return (int64_t)__builtin_amdgcn_readfirstlane((int)first) * TILE;
}

// One 32-key tile (keys kb .. kb + 31) of the forward for the 16 queries of a wave, query c = lane & 15 in qf:
// S^T = K Q^T, mask, the online softmax's running (m, lsum) in log2 units, O^T += V^T P^T.  kp / vp: row 0 of this head.
//   k_row_ok(j): whether key row j may be read for the scores (else it enters as zeros; j = kb + 16s + c)
//   key_ok(t)  : whether the key of k-slot t (row kb + tile_row(g, t)) counts for this lane's query
//   v_row_ok(t): whether the V row of k-slot t may be read (else zeros)
//   drop(p, t) : P as it enters P.V (attention dropout; the identity elsewhere)
// A query's numbers depend on its own column of the tile only, and a tile in which none of its keys counts leaves them as
// they were (alpha = exp2(0), every p = 0): which other queries share the wave, and how far the wave's loop runs past a
// query's last key, does not change a bit of its result.
template <typename T, int D, typename KRowOk, typename KeyOk, typename VRowOk, typename Drop>
__device__ __forceinline__ void attn_fwd_tile(const Quarter<T, D> &qf, const T *kp, int64_t k_rs, const T *vp, int64_t v_rs,
                                              int64_t kb, float sl2, float &m, float &lsum, f32x4 (&acc)[D / 16], int lane,
                                              KRowOk k_row_ok, KeyOk key_ok, VRowOk v_row_ok, Drop drop) {
  const int g = lane >> 4, c = lane & 15;
  f32x4 st[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    Quarter<T, D> kf;
    const int64_t kr = kb + 16 * s + c;
    load_quarter(kf, kp + kr * k_rs + g * (D / 4), k_row_ok(kr));
    st[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    dot_rows<D>(st[s], kf, qf);                          // S^T[key 16s+4g+r][query c]
  }
  float tmax = -INFINITY;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      st[s][r] = key_ok(4 * s + r) ? st[s][r] * sl2 : -INFINITY;
      tmax = fmaxf(tmax, st[s][r]);
    }
  tmax = xor_max(tmax);
  const float mn = fmaxf(m, tmax);
  const float mu = mn == -INFINITY ? 0.f : mn;          // (a row with nothing valid yet: p = 0, no -inf - -inf)
  const float alpha = exp2f(m - mu);
  m = mn;
  float ps = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = exp2f(st[s][r] - mu);
      ps += p;
      st[s][r] = drop(p, 4 * s + r);
    }
  lsum = lsum * alpha + ps;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) acc[dt] *= alpha;
  acc_cols<D>(acc, vp + kb * v_rs, v_rs, v_row_ok, st, lane);
}

}  // namespace
