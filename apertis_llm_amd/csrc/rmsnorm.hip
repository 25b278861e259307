// The RMSNorm row kernels for gfx950 (reference core.py:30-59, the `use_rmsnorm` configuration's pre-norms and final norm):
// plain forward / backward and the block boundary y = res + dropout(blk), xn = RMSNorm(y), dense or with the MoE combine
// formed on the fly.  Per row of width H:  r = sqrt(sum x^2 / H),  s = r + eps (eps OUTSIDE the root),  y = scale * x / s.
//
// The shape of layernorm.hip's kernels with simpler statistics: one wave per row, 8/16-byte non-temporal row accesses, fp32
// statistics, plain loads of `scale`; the parameter gradient leaves as one partial row per block and is folded in a fixed
// order.  No float atomics: the same inputs give the same bits on every run.
#include "row_common.h"

namespace {

// r = sqrt(sum x^2 / H) of a wave's row held as IT float4 chunks per lane (row_mean's layout; chunks past H are zero)
template <int IT>
__device__ __forceinline__ float row_rms(const float4 (&v)[IT], int H) {
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < IT; ++i) sq += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
  return sqrtf(wave_sum(sq) * inv_h(H));
}

// one row's output chunks: xn = x * (1 / s) * scale
template <typename TO, int IT>
__device__ __forceinline__ void rms_store_row(const float4 (&v)[IT], float inv, const float *__restrict__ scale, TO *dst, int lane,
                                              int H) {
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
      const float4 g4 = load4<float>(scale + c);
      store4<TO>(dst + c, make_float4(v[i].x * inv * g4.x, v[i].y * inv * g4.y, v[i].z * inv * g4.z, v[i].w * inv * g4.w));
    }
  }
}

// y[r,:] = scale * x[r,:] / (rms[r] + eps)   (IT chunks of 4 per lane)
template <typename TX, typename TO, int IT>
__global__ void __launch_bounds__(256)
rmsnorm_fwd_k(const TX *__restrict__ x, const float *__restrict__ scale, float eps, TO *__restrict__ y, float *__restrict__ rms_o,
              int64_t T, int H) {
  // the dispatch picks IT = ceil(H / 256) for IT <= 4: every chunk below the last lies inside the row, no bounds test needed
  if constexpr (IT <= 4) __builtin_assume(H > 256 * (IT - 1));
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= T) return;
  float4 v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    v[i] = c < H ? load4s<TX>(x + r * H + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float rms = row_rms<IT>(v, H);
  rms_store_row<TO, IT>(v, 1.f / (rms + eps), scale, y + r * H, lane, H);
  if (lane == 0) rms_o[r] = rms;
}

// Block boundary of the pre-norm stack, forward: y = res + dropout(blk) and xn = RMSNorm(y) in one pass - dropadd_ln_fwd_k
// (layernorm.hip) with the RMS statistics: the same dense / combine forms of blk, the same mask (drop_keep4 on r * H + c), the
// norm on y as stored.
template <typename TX, typename TO, int IT>
__global__ void __launch_bounds__(256)
dropadd_rms_fwd_k(const TO *__restrict__ blk, const int32_t *__restrict__ slot_of, const float *__restrict__ wk, int K,
                  const TX *__restrict__ res, const float *__restrict__ scale, float eps, TX *__restrict__ y, TO *__restrict__ xn,
                  float *__restrict__ rms_o, int64_t T, int H, float drop_p, uint64_t seed) {
  if constexpr (IT <= 4) __builtin_assume(H > 256 * (IT - 1));
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= T) return;
  const float ks = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const uint32_t th = (uint32_t)(drop_p * 65536.f);
  float4 v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (c < H) {
      float4 a;
      if (slot_of) {
        // blk is the expert output [rows,H]: the token's row is the MoE combine (apertis_moe_combine_fwd: k ascending, multiply
        // then add, rounded to the block dtype)
        float4 acc = make_float4(0, 0, 0, 0);
        for (int k = 0; k < K; ++k) {
          const int slot = slot_of[r * K + k];
          if (slot < 0) continue;
          const float wv = wk[r * K + k];
          const float4 u = load4s<TO>(blk + (int64_t)slot * H + c);
          acc.x += u.x * wv; acc.y += u.y * wv; acc.z += u.z * wv; acc.w += u.w * wv;
        }
        a = make_float4(to_f32(from_f32<TO>(acc.x)), to_f32(from_f32<TO>(acc.y)), to_f32(from_f32<TO>(acc.z)), to_f32(from_f32<TO>(acc.w)));
      } else {
        a = load4s<TO>(blk + r * H + c);
      }
      const float4 rr = load4s<TX>(res + r * H + c);
      float e[4] = {a.x, a.y, a.z, a.w};
      if (drop_p > 0.f) {
        bool keep[4];
        drop_keep4(seed, (uint64_t)r * (uint64_t)H + (uint64_t)c, th, keep);
#pragma unroll
        for (int j = 0; j < 4; ++j) e[j] = keep[j] ? e[j] * ks : 0.f;
      }
      v[i] = make_float4(rr.x + e[0], rr.y + e[1], rr.z + e[2], rr.w + e[3]);
      store4<TX>(y + r * H + c, v[i]);
      // the norm sees y as stored (a no-op for the fp32 stream)
      v[i] = make_float4(to_f32(from_f32<TX>(v[i].x)), to_f32(from_f32<TX>(v[i].y)), to_f32(from_f32<TX>(v[i].z)), to_f32(from_f32<TX>(v[i].w)));
    } else {
      v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const float rms = row_rms<IT>(v, H);
  rms_store_row<TO, IT>(v, 1.f / (rms + eps), scale, xn + r * H, lane, H);
  if (lane == 0) rms_o[r] = rms;
}

// rows per wave of the backward (4 waves per block, one partial row per block): layernorm_bwd_k's shape
constexpr int RMS_RPW = 8;

// RMSNorm backward.  Block = 4 waves x RMS_RPW rows each, two rows in flight per wave (the row loop is latency-bound otherwise).
// With g = scale * dy and c = sum_j g_j x_j:   dx = g / s - x * c / (H r s^2)  (+ dres), the second term 0 for a row with r == 0
// (what torch's norm backward yields there);   dscale = sum over rows of dy * x / s.  dx is written in x's dtype; dblk
// (optional) is its masked, 1/(1-p)-scaled copy in the gradient dtype, the mask regenerated from (seed, p) as layernorm_bwd_k
// does.  dscale is reduced over the block's waves in LDS and leaves as ONE partial row per block (rms_fold_k adds them).
template <typename TX, typename TG, int IT>
__global__ void __launch_bounds__(256)
rmsnorm_bwd_k(const TX *__restrict__ x, const float *__restrict__ scale, const float *__restrict__ rms_i, float eps,
              const TG *__restrict__ dy, const TX *__restrict__ dres, TX *__restrict__ dx, TG *__restrict__ dblk, float drop_p,
              uint64_t seed, float *__restrict__ part, int64_t T, int H) {
  if constexpr (IT <= 4) __builtin_assume(H > 256 * (IT - 1));
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4 *red = reinterpret_cast<float4 *>(smem);  // [3 waves][H/4]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * RMS_RPW, r1 = min(r0 + RMS_RPW, T);
  float4 ag[IT], g4[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    ag[i] = make_float4(0, 0, 0, 0);
    const int c = (lane + 64 * i) * 4;
    g4[i] = c < H ? load4<float>(scale + c) : make_float4(0, 0, 0, 0);
  }
  for (int64_t r = r0; r < r1; r += 2) {
    const bool two = r + 1 < r1;
    float4 xv[2][IT], dv[2][IT];
    float rms[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t rr = (q == 0 || two) ? r + q : r;
      rms[q] = rms_i[rr];
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < H) { xv[q][i] = load4s<TX>(x + rr * H + c); dv[q][i] = load4s<TG>(dy + rr * H + c); }
        else { xv[q][i] = make_float4(0, 0, 0, 0); dv[q][i] = make_float4(0, 0, 0, 0); }
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (q == 1 && !two) break;
      const float inv = 1.f / (rms[q] + eps);
      float s2 = 0.f;
      float4 gd[IT];
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        // (chunks past H hold zeros in xv, dv and g4: they add nothing)
        const float4 xq = xv[q][i], dq = dv[q][i];
        gd[i] = make_float4(dq.x * g4[i].x, dq.y * g4[i].y, dq.z * g4[i].z, dq.w * g4[i].w);
        ag[i].x += dq.x * xq.x * inv; ag[i].y += dq.y * xq.y * inv; ag[i].z += dq.z * xq.z * inv; ag[i].w += dq.w * xq.w * inv;
        s2 += (gd[i].x * xq.x + gd[i].y * xq.y) + (gd[i].z * xq.z + gd[i].w * xq.w);
      }
      // c / (H r s^2): the factors of 1/s one at a time (r s^2 itself underflows for a tiny row)
      const float cs = wave_sum(s2) * inv_h(H);
      const float kx = rms[q] > 0.f ? cs * inv * inv / rms[q] : 0.f;
      TX *dst = dx + (r + q) * H;
#pragma unroll
      for (int i = 0; i < IT; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < H) {
          // dres: the gradient arriving on the residual branch that bypasses this norm: added here instead of in a separate pass
          const float4 rr = dres ? load4s<TX>(dres + (r + q) * H + c) : make_float4(0, 0, 0, 0);
          const float4 xq = xv[q][i];
          const float4 dt = make_float4(gd[i].x * inv - xq.x * kx + rr.x, gd[i].y * inv - xq.y * kx + rr.y,
                                        gd[i].z * inv - xq.z * kx + rr.z, gd[i].w * inv - xq.w * kx + rr.w);
          store4<TX>(dst + c, dt);
          if (dblk) {
            // block boundary, backward: x was res + dropout(blk), so the block output's gradient is the masked copy of this
            // row's total gradient as stored
            float e[4] = {dt.x, dt.y, dt.z, dt.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = to_f32(from_f32<TX>(e[j]));
            if (drop_p > 0.f) {
              bool keep[4];
              drop_keep4(seed, (uint64_t)(r + q) * (uint64_t)H + (uint64_t)c, (uint32_t)(drop_p * 65536.f), keep);
              const float ks = 1.f / (1.f - drop_p);
#pragma unroll
              for (int j = 0; j < 4; ++j) e[j] = keep[j] ? e[j] * ks : 0.f;
            }
            store4<TG>(dblk + (r + q) * H + c, make_float4(e[0], e[1], e[2], e[3]));
          }
        }
      }
    }
  }
  // block reduction: waves 1..3 park their sums in LDS, wave 0 adds them in order and writes the block's partial row
  const int Q = H / 4;
  if (wv > 0) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int cq = lane + 64 * i;
      if (cq < Q) red[(wv - 1) * Q + cq] = ag[i];
    }
  }
  __syncthreads();
  if (wv == 0) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int cq = lane + 64 * i;
      if (cq < Q) {
        float4 a = ag[i];
        for (int w = 0; w < 3; ++w) {
          const float4 u = red[w * Q + cq];
          a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
        }
        *reinterpret_cast<float4 *>(part + (int64_t)blockIdx.x * H + cq * 4) = a;
      }
    }
  }
}

// dscale[c] = sum_r part[r][c] (fixed order).  With `fold_out` the launch is the FIRST of two levels: block (x, y) sums the
// rows [y*rpg, (y+1)*rpg) into fold_out[y][c]  (ln_fold_k's pattern over H columns)
__global__ void __launch_bounds__(1024)
rms_fold_k(const float *__restrict__ part, float *__restrict__ dscale, int64_t nrows, int H, float *__restrict__ fold_out,
           int64_t rpg) {
  const int64_t r0 = fold_out ? (int64_t)blockIdx.y * rpg : 0, r1 = fold_out ? min(r0 + rpg, nrows) : nrows;
  colsum_block(part, r0, r1, H, [&](int64_t c, float t) {
    if (fold_out) fold_out[(int64_t)blockIdx.y * H + c] = t;
    else dscale[c] = t;
  });
}

// rows of the backward's workspace: one partial row per block, and behind them the row groups of the two-level fold
constexpr int RMS_FOLD_GROUPS = 32;
int64_t rms_part_rows(int64_t T) { return ceil_div64(T > 0 ? T : 1, 4 * RMS_RPW); }
bool rms_two_level(int64_t nblk) { return nblk >= 8 * RMS_FOLD_GROUPS; }
bool rms_dtype_ok(int d) { return d == APERTIS_F32 || d == APERTIS_BF16; }

}  // namespace

extern "C" int64_t apertis_rmsnorm_bwd_blocks(int64_t T, int64_t H) {
  (void)H;
  const int64_t nblk = rms_part_rows(T);
  return nblk + (rms_two_level(nblk) ? RMS_FOLD_GROUPS : 0);
}

extern "C" int apertis_rmsnorm_fwd(const void *x, const float *scale, float eps, void *y, float *rms, int64_t T, int64_t H,
                                   int dtype_x, int dtype_y, void *stream) {
  if (!x || !scale || !y || !rms || T < 0) return APERTIS_ERR_ARG;
  if (!rms_dtype_ok(dtype_x) || !rms_dtype_ok(dtype_y)) return APERTIS_ERR_ARG;
  if (check_H(H)) return APERTIS_ERR_UNSUPPORTED;
  if (T == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)ceil_div64(T, 4)), block(256);
  DISPATCH_2T(dtype_x, dtype_y, DISPATCH_IT(H, hipLaunchKernelGGL((rmsnorm_fwd_k<TA, TB, IT>), grid, block, 0, st,
      (const TA *)x, scale, eps, (TB *)y, rms, T, (int)H)));
  return apertis_check_launch();
}

extern "C" int apertis_rmsnorm_bwd(const void *x, const float *scale, const float *rms, float eps, const void *dy,
                                   const void *dres, void *dx, void *dblk, float drop_p, uint64_t seed, float *part,
                                   float *dscale, int64_t T, int64_t H, int dtype_x, int dtype_g, void *stream) {
  if (!x || !scale || !rms || !dy || !dx || !part || !dscale || T < 0) return APERTIS_ERR_ARG;
  if (!rms_dtype_ok(dtype_x) || !rms_dtype_ok(dtype_g)) return APERTIS_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return APERTIS_ERR_ARG;
  if (check_H(H)) return APERTIS_ERR_UNSUPPORTED;
  if (T == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nblk = rms_part_rows(T);
  dim3 grid((unsigned)nblk), block(256);
  const size_t lds = 3 * (size_t)H * sizeof(float);
  DISPATCH_2T(dtype_x, dtype_g, DISPATCH_IT(H, launch_lds(rmsnorm_bwd_k<TA, TB, IT>, grid, block, lds, st,
      (const TA *)x, scale, rms, eps, (const TB *)dy, (const TA *)dres, (TA *)dx, (TB *)dblk, drop_p, seed, part, T, (int)H)));
  fold_levels(part, part + nblk * H, nblk, H, rms_two_level(nblk) ? RMS_FOLD_GROUPS : 0,
              [&](dim3 fgrid, const float *in, int64_t rows, int64_t rpg, float *fold) {
                hipLaunchKernelGGL(rms_fold_k, fgrid, dim3(1024), 0, st, in, dscale, rows, (int)H, fold, rpg);
              });
  return apertis_check_launch();
}

extern "C" int apertis_dropout_add_rmsnorm_fwd(const void *blk, const int32_t *slot_of, const float *wk, int64_t K,
                                               const void *res, const float *scale, float eps, void *y, void *xn, float *rms,
                                               int64_t T, int64_t H, float drop_p, uint64_t seed, int dtype_x, int dtype_y,
                                               void *stream) {
  if (!blk || !res || !scale || !y || !xn || !rms || T < 0) return APERTIS_ERR_ARG;
  if (!rms_dtype_ok(dtype_x) || !rms_dtype_ok(dtype_y)) return APERTIS_ERR_ARG;
  if (!(drop_p >= 0.f && drop_p < 1.f)) return APERTIS_ERR_ARG;
  if (slot_of && (!wk || K < 1 || K > MAXK)) return APERTIS_ERR_ARG;
  if (check_H(H)) return APERTIS_ERR_UNSUPPORTED;
  if (T == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)ceil_div64(T, 4)), block(256);
  DISPATCH_2T(dtype_x, dtype_y, DISPATCH_IT(H, hipLaunchKernelGGL((dropadd_rms_fwd_k<TA, TB, IT>), grid, block, 0, st,
      (const TB *)blk, slot_of, wk, (int)K, (const TA *)res, scale, eps, (TA *)y, (TB *)xn, rms, T, (int)H, drop_p, seed)));
  return apertis_check_launch();
}
