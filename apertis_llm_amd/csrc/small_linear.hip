// The small linears for gfx950: the skinny projection y = x W^T + b with N <= 16 outputs (the MoE router's Linear without its
// LayerNorm) and the tiny one with K <= 64 inputs (the SSM's dt_proj_head), forward and backward; the weight gradients leave
// as per-block partial rows folded in a fixed order (fold_rows_k).
#include "row_common.h"

namespace {

// ------------------------------------------------------------------------------------------
// Skinny linear: y[T,N] = x[T,K] W[N,K]^T + b, N <= 16 (reference core.py:430,482: H -> num_experts).
// A GEMM library spends ~115 us on this 0.4 GFLOP product (N=8); it is a bandwidth problem: one
// wave per row, the weight matrix lives in registers, N dot products are finished with wave
// reductions.  Backward: dx = dy W (row kernel), dW/db = per-wave register sums over 8 rows ->
// block partials -> fixed-order fold.
// ------------------------------------------------------------------------------------------

template <typename TX, int IT, int NN>
__global__ void __launch_bounds__(256)
skinny_fwd_k(const TX *__restrict__ x, const float *__restrict__ W, const float *__restrict__ b, float *__restrict__ y,
             int64_t T, int K) {
  if constexpr (IT <= 4) __builtin_assume(K > 256 * (IT - 1));   // IT = ceil(K / 256): only the last chunk needs its bounds test
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  float4 w[NN][IT];
#pragma unroll
  for (int n = 0; n < NN; ++n)
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      int c = (lane + 64 * i) * 4;
      w[n][i] = c < K ? load4<float>(W + (int64_t)n * K + c) : make_float4(0, 0, 0, 0);
    }
  for (int64_t r = wave; r < T; r += nw) {
    float4 xv[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      int c = (lane + 64 * i) * 4;
      xv[i] = c < K ? load4s<TX>(x + r * K + c) : make_float4(0, 0, 0, 0);
    }
    float acc[NN];
#pragma unroll
    for (int n = 0; n < NN; ++n) {
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < IT; ++i) a += (xv[i].x * w[n][i].x + xv[i].y * w[n][i].y) + (xv[i].z * w[n][i].z + xv[i].w * w[n][i].w);
      acc[n] = wave_sum(a);
    }
    if (lane < NN) {
      float v = 0.f;
#pragma unroll
      for (int n = 0; n < NN; ++n) if (lane == n) v = acc[n];
      y[r * NN + lane] = v + (b ? b[lane] : 0.f);
    }
  }
}

template <typename TX, int IT, int NN>
__global__ void __launch_bounds__(256)
skinny_bwd_k(const TX *__restrict__ x, const float *__restrict__ W, const float *__restrict__ dy, TX *__restrict__ dx,
             float *__restrict__ part, int64_t T, int K) {
  if constexpr (IT <= 4) __builtin_assume(K > 256 * (IT - 1));   // IT = ceil(K / 256): only the last chunk needs its bounds test
  // part: [gridDim.x][NN*K + NN] per-block partial sums of dW (row-major [NN][K]) then db
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4 *red = reinterpret_cast<float4 *>(smem);   // [3 waves][NN][K/4]
  __shared__ float redb[4][SK_MAXN];
  constexpr int RPW = 8;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * RPW, r1 = min(r0 + RPW, T);
  float4 w[NN][IT], aw[NN][IT];
  float abias[NN];
#pragma unroll
  for (int n = 0; n < NN; ++n) {
    abias[n] = 0.f;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      int c = (lane + 64 * i) * 4;
      w[n][i] = c < K ? load4<float>(W + (int64_t)n * K + c) : make_float4(0, 0, 0, 0);
      aw[n][i] = make_float4(0, 0, 0, 0);
    }
  }
  for (int64_t r = r0; r < r1; ++r) {
    float g[NN];
#pragma unroll
    for (int n = 0; n < NN; ++n) g[n] = dy[r * NN + n];   // same address in every lane: one broadcast load
    float4 xv[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      int c = (lane + 64 * i) * 4;
      xv[i] = c < K ? load4s<TX>(x + r * K + c) : make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      int c = (lane + 64 * i) * 4;
      float4 d = make_float4(0, 0, 0, 0);
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        d.x += g[n] * w[n][i].x; d.y += g[n] * w[n][i].y; d.z += g[n] * w[n][i].z; d.w += g[n] * w[n][i].w;
        aw[n][i].x += g[n] * xv[i].x; aw[n][i].y += g[n] * xv[i].y; aw[n][i].z += g[n] * xv[i].z; aw[n][i].w += g[n] * xv[i].w;
      }
      if (c < K) store4<TX>(dx + r * K + c, d);
    }
#pragma unroll
    for (int n = 0; n < NN; ++n) abias[n] += g[n];
  }
  const int Q = K / 4;
  if (wv > 0) {
#pragma unroll
    for (int n = 0; n < NN; ++n)
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        int cq = lane + 64 * i;
        if (cq < Q) red[((wv - 1) * NN + n) * Q + cq] = aw[n][i];
      }
  }
  if (lane == 0)
#pragma unroll
    for (int n = 0; n < NN; ++n) redb[wv][n] = abias[n];
  __syncthreads();
  float *dst = part + (int64_t)blockIdx.x * (NN * K + NN);
  if (wv == 0) {
#pragma unroll
    for (int n = 0; n < NN; ++n)
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        int cq = lane + 64 * i;
        if (cq < Q) {
          float4 a = aw[n][i];
          for (int w_ = 0; w_ < 3; ++w_) {
            float4 u = red[(w_ * NN + n) * Q + cq];
            a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
          }
          *reinterpret_cast<float4 *>(dst + (int64_t)n * K + cq * 4) = a;
        }
      }
    if (lane < NN) dst[NN * K + lane] = (redb[0][lane] + redb[1][lane]) + (redb[2][lane] + redb[3][lane]);
  }
}

// ------------------------------------------------------------------------------------------
// Tiny linear: y[T,N] = x[T,:K] W[N,K]^T + b with K <= 64, N <= 16 - the SSM's dt_proj_head
// (Linear(dt_rank -> heads), reference core.py:361,382), whose input is a column slice of the
// x_param_proj output (row stride ldx).  A GEMM library pays ~20 us forward and ~270 us backward
// (a [11 x 98304] x [98304 x 22] weight gradient on 16x16 macro tiles plus a separate bias
// reduction) for 4 MB of traffic.  One row per thread; W and b sit in LDS (broadcast reads).
// Backward: dx per row, and dW/db as per-block partial sums over a row tile staged in LDS
// (entry q < N*K is dW[q], the next N are db; thread p owns q = p, p + 128, ...), folded in a fixed order.
// ------------------------------------------------------------------------------------------
constexpr int TL_MAXK = 64, TL_MAXN = 16, TL_ROWS = 128;

// a thread's K-element row slice -> floats.  VEC: 16-byte loads (row start 16-byte aligned, the slice rounded
// up to whole chunks stays inside the row); lanes hold different rows ~ld apart, so every load instruction
// touches 64 cache lines whatever its width - six 16-byte loads instead of 44 two-byte ones
template <typename TX, bool VEC>
__device__ __forceinline__ void tl_load_row(const TX *row, int K, float (&xr)[TL_MAXK]) {
  constexpr int EPC = 16 / (int)sizeof(TX);
  if constexpr (VEC) {
#pragma unroll
    for (int ch = 0; ch < TL_MAXK / EPC; ++ch) {
      if (ch * EPC < K) {
        float4 lo, hi = make_float4(0, 0, 0, 0);
        if constexpr (sizeof(TX) == 2) {
          const uint4 u = *reinterpret_cast<const uint4 *>(row + ch * EPC);
          lo = raw_to_f4(make_uint2(u.x, u.y));
          hi = raw_to_f4(make_uint2(u.z, u.w));
          const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
          for (int u8 = 0; u8 < 8; ++u8) xr[ch * 8 + u8] = ch * 8 + u8 < K ? v[u8] : 0.f;
        } else {
          lo = *reinterpret_cast<const float4 *>(row + ch * EPC);
          const float v[4] = {lo.x, lo.y, lo.z, lo.w};
#pragma unroll
          for (int u4 = 0; u4 < 4; ++u4) xr[ch * 4 + u4] = ch * 4 + u4 < K ? v[u4] : 0.f;
        }
      } else {
#pragma unroll
        for (int u = 0; u < EPC; ++u) xr[ch * EPC + u] = 0.f;
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < TL_MAXK; ++r) xr[r] = r < K ? to_f32(row[r]) : 0.f;
  }
}

// W (and b) in LDS as a zero-padded [TL_MAXN][TL_MAXK] table read four weights at a time (ds_read_b128, all lanes the
// same address): one LDS instruction per four FMAs instead of one per FMA - the kernels were LDS-issue-bound
__device__ __forceinline__ void tl_stage_w(float *sW, const float *__restrict__ W, int K, int N) {
  for (int i = threadIdx.x; i < TL_MAXN * TL_MAXK; i += TL_ROWS) {
    const int j = i / TL_MAXK, r = i - j * TL_MAXK;
    sW[i] = (j < N && r < K) ? W[j * K + r] : 0.f;
  }
}

template <typename TX, bool VEC>
__global__ void __launch_bounds__(TL_ROWS)
tiny_linear_fwd_k(const TX *__restrict__ x, int64_t ldx, const float *__restrict__ W, const float *__restrict__ b,
                  float *__restrict__ y, int64_t T, int K, int N) {
  __shared__ __attribute__((aligned(16))) float sW[TL_MAXN * TL_MAXK + TL_MAXN];
  tl_stage_w(sW, W, K, N);
  for (int i = threadIdx.x; i < N; i += TL_ROWS) sW[TL_MAXN * TL_MAXK + i] = b ? b[i] : 0.f;
  __syncthreads();
  const float4 *sW4 = reinterpret_cast<const float4 *>(sW);
  for (int64_t t = (int64_t)blockIdx.x * TL_ROWS + threadIdx.x; t < T; t += (int64_t)gridDim.x * TL_ROWS) {
    float xr[TL_MAXK];
    tl_load_row<TX, VEC>(x + t * ldx, K, xr);
    for (int j = 0; j < N; ++j) {
      float a = sW[TL_MAXN * TL_MAXK + j];
#pragma unroll
      for (int r4 = 0; r4 < TL_MAXK / 4; ++r4)
        if (r4 * 4 < K) {    // the pad entries of the last chunk are zeros on both sides
          const float4 w = sW4[j * (TL_MAXK / 4) + r4];
          a = fmaf(xr[4 * r4], w.x, a); a = fmaf(xr[4 * r4 + 1], w.y, a);
          a = fmaf(xr[4 * r4 + 2], w.z, a); a = fmaf(xr[4 * r4 + 3], w.w, a);
        }
      y[t * N + j] = a;
    }
  }
}

// The same for a handful of rows (the decode step: T <= 64): a thread per (row, output) with W straight from global memory -
// the kernel above stages a 16 x 64 table in LDS and then has ONE thread walk all N outputs of a row (13 us for one token).
// Same accumulation chain per output (bias first, then r = 0, 1, ...): the same bits.
template <typename TX>
__global__ void __launch_bounds__(256)
tiny_linear_fwd_small_k(const TX *__restrict__ x, int64_t ldx, const float *__restrict__ W, const float *__restrict__ b,
                        float *__restrict__ y, int64_t T, int K, int N) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T * N) return;
  const int64_t t = i / N;
  const int j = (int)(i - t * N);
  const TX *row = x + t * ldx;
  const float *w = W + (int64_t)j * K;
  float a = b ? b[j] : 0.f;
  for (int r = 0; r < K; ++r) a = fmaf(to_f32(row[r]), w[r], a);
  y[i] = a;
}

// The dt logits of PACKED rows (ops.ssm.SSM_PACKED; rows are the tokens of [B, L], start = ops.document_layout's int32
// [B, L]): tiny_linear_fwd_k, except that the row of a document's first token at t >= 1 (start[b, t] == t) receives `reset`
// in every column instead of the projection - the scan then forms a = exp2(softplus(reset) * A2) = 0 there, which is the
// state reset.  Such a row is not loaded.  Every other row: the chain above, the same bits.
template <typename TX, bool VEC>
__global__ void __launch_bounds__(TL_ROWS)
tiny_linear_doc_fwd_k(const TX *__restrict__ x, int64_t ldx, const float *__restrict__ W, const float *__restrict__ b,
                      const int32_t *__restrict__ start, float reset, float *__restrict__ y, int64_t T, int64_t L, int K, int N) {
  __shared__ __attribute__((aligned(16))) float sW[TL_MAXN * TL_MAXK + TL_MAXN];
  tl_stage_w(sW, W, K, N);
  for (int i = threadIdx.x; i < N; i += TL_ROWS) sW[TL_MAXN * TL_MAXK + i] = b ? b[i] : 0.f;
  __syncthreads();
  const float4 *sW4 = reinterpret_cast<const float4 *>(sW);
  for (int64_t t = (int64_t)blockIdx.x * TL_ROWS + threadIdx.x; t < T; t += (int64_t)gridDim.x * TL_ROWS) {
    const int64_t tl = t % L;
    if (tl > 0 && (int64_t)start[t] == tl) {
      for (int j = 0; j < N; ++j) y[t * N + j] = reset;
      continue;
    }
    float xr[TL_MAXK];
    tl_load_row<TX, VEC>(x + t * ldx, K, xr);
    for (int j = 0; j < N; ++j) {
      float a = sW[TL_MAXN * TL_MAXK + j];
#pragma unroll
      for (int r4 = 0; r4 < TL_MAXK / 4; ++r4)
        if (r4 * 4 < K) {    // the pad entries of the last chunk are zeros on both sides
          const float4 w = sW4[j * (TL_MAXK / 4) + r4];
          a = fmaf(xr[4 * r4], w.x, a); a = fmaf(xr[4 * r4 + 1], w.y, a);
          a = fmaf(xr[4 * r4 + 2], w.z, a); a = fmaf(xr[4 * r4 + 3], w.w, a);
        }
      y[t * N + j] = a;
    }
  }
}

// ... and for logits that something else has formed (a dt projection the kernel above does not take): only the overwrite
__global__ void __launch_bounds__(256)
doc_reset_rows_k(const int32_t *__restrict__ start, float reset, float *__restrict__ y, int64_t T, int64_t L, int N) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T * N; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / N, tl = t % L;
    if (tl > 0 && (int64_t)start[t] == tl) y[i] = reset;
  }
}

// Backward.  dx per row (W four at a time from LDS, as above).  dW/db as per-block partial sums over the row tile
// staged in LDS: thread p owns the 2 x 4 block dW[2*(p/16) + {0,1}][4*(p%16) + {0..3}] (and db of its two rows when
// p%16 == 0) and reads one 8-byte dy pair and one 16-byte x chunk per row for eight FMAs; rows are walked in order and
// the per-block partials folded in a fixed order.
template <typename TX, bool VEC>
__global__ void __launch_bounds__(TL_ROWS)
tiny_linear_bwd_k(const TX *__restrict__ x, int64_t ldx, const float *__restrict__ W, const float *__restrict__ dy,
                  TX *__restrict__ dx, int64_t lddx, float *__restrict__ part, int64_t T, int K, int N, int zero_to) {
  static_assert(TL_ROWS == (TL_MAXN / 2) * (TL_MAXK / 4), "one 2 x 4 block of dW per thread");
  __shared__ __attribute__((aligned(16))) float sW[TL_MAXN * TL_MAXK];
  __shared__ __attribute__((aligned(16))) float sx[TL_ROWS][TL_MAXK + 4];
  __shared__ __attribute__((aligned(16))) float sdy[TL_ROWS][TL_MAXN + 2];
  tl_stage_w(sW, W, K, N);
  const float4 *sW4 = reinterpret_cast<const float4 *>(sW);
  const int nq = N * K + N;
  const int jb = threadIdx.x >> 4, rb = threadIdx.x & 15;
  float acc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, accb[2] = {0.f, 0.f};
  for (int64_t t0 = (int64_t)blockIdx.x * TL_ROWS; t0 < T; t0 += (int64_t)gridDim.x * TL_ROWS) {
    const int64_t t = t0 + threadIdx.x;
    const bool live = t < T;
    __syncthreads();   // sW loaded / the previous tile is no longer read
    {
      float xr[TL_MAXK];
      if (live) tl_load_row<TX, VEC>(x + t * ldx, K, xr);
#pragma unroll
      for (int r4 = 0; r4 < TL_MAXK / 4; ++r4)
        *reinterpret_cast<float4 *>(&sx[threadIdx.x][4 * r4]) =
            live ? make_float4(xr[4 * r4], xr[4 * r4 + 1], xr[4 * r4 + 2], xr[4 * r4 + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float dyr[TL_MAXN];
#pragma unroll
    for (int j = 0; j < TL_MAXN; ++j) {
      dyr[j] = (live && j < N) ? dy[t * N + j] : 0.f;
      sdy[threadIdx.x][j] = dyr[j];
    }
    if (live) {
      constexpr int EPC = 16 / (int)sizeof(TX);
      TX *drow = dx + t * lddx;
      for (int r0 = 0; r0 < K; r0 += EPC) {
        float a[EPC];
#pragma unroll
        for (int u = 0; u < EPC; ++u) a[u] = 0.f;
#pragma unroll
        for (int j = 0; j < TL_MAXN; ++j)
          if (j < N) {
#pragma unroll
            for (int u4 = 0; u4 < EPC / 4; ++u4) {
              const float4 w = sW4[j * (TL_MAXK / 4) + (r0 >> 2) + u4];   // zeros past K
              a[4 * u4] = fmaf(dyr[j], w.x, a[4 * u4]); a[4 * u4 + 1] = fmaf(dyr[j], w.y, a[4 * u4 + 1]);
              a[4 * u4 + 2] = fmaf(dyr[j], w.z, a[4 * u4 + 2]); a[4 * u4 + 3] = fmaf(dyr[j], w.w, a[4 * u4 + 3]);
            }
          }
        if (VEC && r0 + EPC <= K) {      // whole 16-byte chunk (the output rows are 16-byte aligned when VEC)
          if constexpr (sizeof(TX) == 2) {
            uint32_t wq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
              wq[u] = (uint32_t)__builtin_bit_cast(uint16_t, from_f32<TX>(a[2 * u])) |
                      ((uint32_t)__builtin_bit_cast(uint16_t, from_f32<TX>(a[2 * u + 1])) << 16);
            *reinterpret_cast<uint4 *>(drow + r0) = make_uint4(wq[0], wq[1], wq[2], wq[3]);
          } else {
            *reinterpret_cast<float4 *>(drow + r0) = make_float4(a[0], a[1], a[2], a[3]);
          }
        } else {
#pragma unroll
          for (int u = 0; u < EPC; ++u)
            if (r0 + u < K) drow[r0 + u] = from_f32<TX>(a[u]);
        }
      }
      // the columns [K, zero_to) behind the row receive zeros: the pad of the projection output's gradient (the caller's
      // split_cols slot next to the dt columns - one strided torch fill per layer otherwise)
      if (zero_to > K) {
        int c = K;
        if (VEC && (K & 3) == 0)
          for (; c + 4 <= zero_to; c += 4) {
            if constexpr (sizeof(TX) == 2) *reinterpret_cast<uint2 *>(drow + c) = make_uint2(0u, 0u);
            else *reinterpret_cast<float4 *>(drow + c) = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        for (; c < zero_to; ++c) drow[c] = from_f32<TX>(0.f);
      }
    }
    __syncthreads();
    if (2 * jb < N && 4 * rb < K) {
      for (int row = 0; row < TL_ROWS; ++row) {
        const float2 d = *reinterpret_cast<const float2 *>(&sdy[row][2 * jb]);
        const float4 xv = *reinterpret_cast<const float4 *>(&sx[row][4 * rb]);
        acc[0][0] = fmaf(d.x, xv.x, acc[0][0]); acc[0][1] = fmaf(d.x, xv.y, acc[0][1]);
        acc[0][2] = fmaf(d.x, xv.z, acc[0][2]); acc[0][3] = fmaf(d.x, xv.w, acc[0][3]);
        acc[1][0] = fmaf(d.y, xv.x, acc[1][0]); acc[1][1] = fmaf(d.y, xv.y, acc[1][1]);
        acc[1][2] = fmaf(d.y, xv.z, acc[1][2]); acc[1][3] = fmaf(d.y, xv.w, acc[1][3]);
        if (rb == 0) { accb[0] += d.x; accb[1] += d.y; }
      }
    }
  }
  float *dst = part + (int64_t)blockIdx.x * nq;
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int j = 2 * jb + jj;
    if (j < N) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (4 * rb + u < K) dst[j * K + 4 * rb + u] = acc[jj][u];
      if (rb == 0) dst[N * K + j] = accb[jj];
    }
  }
}

}  // namespace

extern "C" int64_t apertis_skinny_linear_bwd_blocks(int64_t T) { return ceil_div64(T > 0 ? T : 1, 32); }

extern "C" int apertis_skinny_linear_fwd(const void *x, const float *W, const float *b, float *y, int64_t T, int64_t K,
                                         int64_t N, int dtype_x, void *stream) {
  if (!x || !W || !y || T < 0) return APERTIS_ERR_ARG;
  if (K <= 0 || K % 4 || K > 1024 || N < 1 || N > SK_MAXN) return APERTIS_ERR_UNSUPPORTED;
  if (N > 8 && K > 256) return APERTIS_ERR_UNSUPPORTED;   // register budget: N*K/64 weight words per lane
  if (T == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)std::min<int64_t>(ceil_div64(T, 8), 4096)), block(256);
  if (dtype_x == APERTIS_BF16) {
    SKINNY_N(N, SKINNY_IT(K, hipLaunchKernelGGL((skinny_fwd_k<bf16_t, IT, NN>), grid, block, 0, st, (const bf16_t *)x, W, b, y, T, (int)K)));
  } else if (dtype_x == APERTIS_F32) {
    SKINNY_N(N, SKINNY_IT(K, hipLaunchKernelGGL((skinny_fwd_k<float, IT, NN>), grid, block, 0, st, (const float *)x, W, b, y, T, (int)K)));
  } else return APERTIS_ERR_ARG;
  return apertis_check_launch();
}

extern "C" int apertis_skinny_linear_bwd(const void *x, const float *W, const float *dy, void *dx, float *part,
                                         float *dW_db, int64_t T, int64_t K, int64_t N, int dtype_x, void *stream) {
  // part: workspace [apertis_skinny_linear_bwd_blocks(T)][N*K + N]; dW_db: out [N*K + N] (dW then db)
  if (!x || !W || !dy || !dx || !part || !dW_db || T < 0) return APERTIS_ERR_ARG;
  if (K <= 0 || K % 4 || K > 1024 || N < 1 || N > SK_MAXN) return APERTIS_ERR_UNSUPPORTED;
  if (N > 8 && K > 256) return APERTIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = apertis_skinny_linear_bwd_blocks(T);
  dim3 grid((unsigned)nblk), block(256);
  const size_t lds = 3 * (size_t)N * K * sizeof(float);
  if (dtype_x == APERTIS_BF16) {
    SKINNY_N(N, SKINNY_IT(K, launch_lds(skinny_bwd_k<bf16_t, IT, NN>, grid, block, lds, st, (const bf16_t *)x, W, dy, (bf16_t *)dx, part, T, (int)K)));
  } else if (dtype_x == APERTIS_F32) {
    SKINNY_N(N, SKINNY_IT(K, launch_lds(skinny_bwd_k<float, IT, NN>, grid, block, lds, st, (const float *)x, W, dy, (float *)dx, part, T, (int)K)));
  } else return APERTIS_ERR_ARG;
  const int64_t cols = N * K + N;
  hipLaunchKernelGGL(fold_rows_k, dim3((unsigned)ceil_div64(cols, 64)), dim3(1024), 0, st, part, dW_db, nblk, cols);
  return apertis_check_launch();
}

extern "C" int64_t apertis_tiny_linear_bwd_blocks(int64_t T) {
  return std::min<int64_t>(ceil_div64(T > 0 ? T : 1, TL_ROWS), 1024);
}

extern "C" int apertis_tiny_linear_fwd(const void *x, int64_t ldx, const float *W, const float *b, float *y, int64_t T,
                                       int64_t K, int64_t N, int dtype_x, void *stream) {
  if (!x || !W || !y || T < 0 || ldx < K) return APERTIS_ERR_ARG;
  if (K < 1 || K > TL_MAXK || N < 1 || N > TL_MAXN) return APERTIS_ERR_UNSUPPORTED;
  if (T == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)std::min<int64_t>(ceil_div64(T, TL_ROWS), 4096)), block(TL_ROWS);
  if (dtype_x != APERTIS_BF16 && dtype_x != APERTIS_F32) return APERTIS_ERR_ARG;
  if (T <= 64) {   // the decode step
    const dim3 gs((unsigned)ceil_div64(T * N, 256)), bs(256);
    if (dtype_x == APERTIS_BF16) hipLaunchKernelGGL(tiny_linear_fwd_small_k<bf16_t>, gs, bs, 0, st, (const bf16_t *)x, ldx, W, b, y, T, (int)K, (int)N);
    else hipLaunchKernelGGL(tiny_linear_fwd_small_k<float>, gs, bs, 0, st, (const float *)x, ldx, W, b, y, T, (int)K, (int)N);
    return apertis_check_launch();
  }
  const int64_t esz = dtype_x == APERTIS_BF16 ? 2 : 4, epc = 16 / esz;
  const bool vec = (((uintptr_t)x) & 15) == 0 && (ldx * esz) % 16 == 0 && ceil_div64(K, epc) * epc <= ldx;
#define GO(TX, V) hipLaunchKernelGGL((tiny_linear_fwd_k<TX, V>), grid, block, 0, st, (const TX *)x, ldx, W, b, y, T, (int)K, (int)N)
  if (dtype_x == APERTIS_BF16) { if (vec) GO(bf16_t, true); else GO(bf16_t, false); }
  else { if (vec) GO(float, true); else GO(float, false); }
#undef GO
  return apertis_check_launch();
}

extern "C" int apertis_tiny_linear_doc_fwd(const void *x, int64_t ldx, const float *W, const float *b, const int32_t *start,
                                           float reset, float *y, int64_t T, int64_t L, int64_t K, int64_t N, int dtype_x,
                                           void *stream) {
  if (!start || !y || T < 0 || L < 1 || T % L || !(reset == reset) || N < 1) return APERTIS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (!x) {    // y holds the logits already: overwrite the rows of the document starts, nothing else
    if (T == 0) return APERTIS_OK;
    hipLaunchKernelGGL(doc_reset_rows_k, dim3((unsigned)std::min<int64_t>(ceil_div64(T * N, 256), 4096)), dim3(256), 0, st, start,
                       reset, y, T, L, (int)std::min<int64_t>(N, 0x7fffffff));
    return apertis_check_launch();
  }
  if (!W || ldx < K) return APERTIS_ERR_ARG;
  if (K < 1 || K > TL_MAXK || N > TL_MAXN) return APERTIS_ERR_UNSUPPORTED;
  if (dtype_x != APERTIS_BF16 && dtype_x != APERTIS_F32) return APERTIS_ERR_ARG;
  if (T == 0) return APERTIS_OK;
  dim3 grid((unsigned)std::min<int64_t>(ceil_div64(T, TL_ROWS), 4096)), block(TL_ROWS);
  const int64_t esz = dtype_x == APERTIS_BF16 ? 2 : 4, epc = 16 / esz;
  const bool vec = (((uintptr_t)x) & 15) == 0 && (ldx * esz) % 16 == 0 && ceil_div64(K, epc) * epc <= ldx;
#define GO(TX, V) hipLaunchKernelGGL((tiny_linear_doc_fwd_k<TX, V>), grid, block, 0, st, (const TX *)x, ldx, W, b, start, reset, y, T, L, (int)K, (int)N)
  if (dtype_x == APERTIS_BF16) { if (vec) GO(bf16_t, true); else GO(bf16_t, false); }
  else { if (vec) GO(float, true); else GO(float, false); }
#undef GO
  return apertis_check_launch();
}

extern "C" int apertis_tiny_linear_bwd_pad(const void *x, int64_t ldx, const float *W, const float *dy, void *dx, int64_t lddx,
                                           float *part, float *dW_db, int64_t T, int64_t K, int64_t N, int64_t zero_to, int dtype_x,
                                           void *stream) {
  // part: workspace [apertis_tiny_linear_bwd_blocks(T)][N*K + N]; dW_db: out [N*K + N] (dW then db)
  if (!x || !W || !dy || !dx || !part || !dW_db || T < 0 || ldx < K || lddx < K || zero_to > lddx) return APERTIS_ERR_ARG;
  if (zero_to < K) zero_to = K;
  if (K < 1 || K > TL_MAXK || N < 1 || N > TL_MAXN) return APERTIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = apertis_tiny_linear_bwd_blocks(T);
  dim3 grid((unsigned)nblk), block(TL_ROWS);
  if (dtype_x != APERTIS_BF16 && dtype_x != APERTIS_F32) return APERTIS_ERR_ARG;
  const int64_t esz = dtype_x == APERTIS_BF16 ? 2 : 4, epc = 16 / esz;
  const bool vec = (((uintptr_t)x) & 15) == 0 && (ldx * esz) % 16 == 0 && ceil_div64(K, epc) * epc <= ldx &&
                   (((uintptr_t)dx) & 15) == 0 && (lddx * esz) % 16 == 0;
#define GO(TX, V) hipLaunchKernelGGL((tiny_linear_bwd_k<TX, V>), grid, block, 0, st, (const TX *)x, ldx, W, dy, (TX *)dx, lddx, part, T, (int)K, (int)N, (int)zero_to)
  if (dtype_x == APERTIS_BF16) { if (vec) GO(bf16_t, true); else GO(bf16_t, false); }
  else { if (vec) GO(float, true); else GO(float, false); }
#undef GO
  const int64_t cols = N * K + N;
  hipLaunchKernelGGL(fold_rows_k, dim3((unsigned)ceil_div64(cols, 64)), dim3(1024), 0, st, part, dW_db, nblk, cols);
  return apertis_check_launch();
}
extern "C" int apertis_tiny_linear_bwd(const void *x, int64_t ldx, const float *W, const float *dy, void *dx, int64_t lddx,
                                       float *part, float *dW_db, int64_t T, int64_t K, int64_t N, int dtype_x,
                                       void *stream) {
  return apertis_tiny_linear_bwd_pad(x, ldx, W, dy, dx, lddx, part, dW_db, T, K, N, K, dtype_x, stream);
}
