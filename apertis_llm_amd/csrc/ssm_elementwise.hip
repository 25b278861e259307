// Memory-bound companions of the scan on token-major [T, Dn] data (gfx950):
//   - depthwise causal conv1d + SiLU   (reference core.py:368-375)
//   - post-scan skip + gate            (reference core.py:395-396)
//   - fp32 -> {fp32,bf16} cast with an optional transposed copy (compute copies of the expert
//     weights: [E,R,C] and [E,C,R], so forward and dgrad both read K-contiguous operands)
// Geometry shared by the first two: a thread owns ONE 4-channel chunk (16 B fp32 / 8 B bf16) and
// walks tokens, so per-channel reductions (dD, dw, dbias) stay in registers; a block covers
// RP = 256/CPR rows at a time (CPR = Dn/4 chunks per row) and leaves [nblk, ...] partials that a
// deterministic column-sum kernel folds.
#include <type_traits>

#include "common.h"

namespace {

template <typename T> __device__ __forceinline__ float4 ld4(const T *p);
template <> __device__ __forceinline__ float4 ld4<float>(const float *p) { return *reinterpret_cast<const float4 *>(p); }
template <> __device__ __forceinline__ float4 ld4<bf16_t>(const bf16_t *p) {
  uint2 u = *reinterpret_cast<const uint2 *>(p);
  return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                     __uint_as_float(u.y & 0xffff0000u));
}
template <typename T> __device__ __forceinline__ void st4(T *p, float4 v);
template <> __device__ __forceinline__ void st4<float>(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
template <> __device__ __forceinline__ void st4<bf16_t>(bf16_t *p, float4 v) {
  typedef __attribute__((ext_vector_type(4))) bf16_t bf4;
  bf4 o = {(bf16_t)v.x, (bf16_t)v.y, (bf16_t)v.z, (bf16_t)v.w};
  *reinterpret_cast<bf4 *>(p) = o;
}

// sigmoid on the hardware exp2 / rcp (1 ulp each, ~3e-7 relative: far inside the 1e-4 parity bar), as scan_gate.hip's;
// expf + an IEEE division were ~30 VALU instructions per value
__device__ __forceinline__ float sigmoidf_(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-x * 1.4426950408889634f)); }
__device__ __forceinline__ float siluf_(float x) { return x * sigmoidf_(x); }
__device__ __forceinline__ float silu_grad(float x) { float s = sigmoidf_(x); return s * (1.f + x * (1.f - s)); }

struct Geo { int CPR, RP; };
__host__ __device__ inline Geo make_geo(int64_t Dn) {
  Geo g; g.CPR = (int)(Dn / 4); g.RP = g.CPR >= 256 ? 1 : 256 / g.CPR; return g;
}

// ---------------------------------------------------------------- gate
template <typename TY, typename TIO>
__global__ void __launch_bounds__(256)
ssm_gate_fwd_k(const TY *__restrict__ y, int64_t y_rs, const TIO *__restrict__ xc, int64_t xc_rs,
               const TIO *__restrict__ z, int64_t z_rs, const float *__restrict__ D, TIO *__restrict__ out,
               int64_t out_rs, int64_t T, int Dn) {
  const Geo g = make_geo(Dn);
  const int rr = threadIdx.x / g.CPR;
  if (rr >= g.RP) return;
  for (int c = threadIdx.x - rr * g.CPR; c < g.CPR; c += 256) {
    const float4 d4 = ld4<float>(D + c * 4);
    for (int64_t t = (int64_t)blockIdx.x * g.RP + rr; t < T; t += (int64_t)gridDim.x * g.RP) {
      float4 yv = ld4<TY>(y + t * y_rs + c * 4), xv = ld4<TIO>(xc + t * xc_rs + c * 4), zv = ld4<TIO>(z + t * z_rs + c * 4);
      float4 o = make_float4((yv.x + d4.x * xv.x) * siluf_(zv.x), (yv.y + d4.y * xv.y) * siluf_(zv.y),
                             (yv.z + d4.z * xv.z) * siluf_(zv.z), (yv.w + d4.w * xv.w) * siluf_(zv.w));
      st4<TIO>(out + t * out_rs + c * 4, o);
    }
  }
}

template <typename TY, typename TIO>
__global__ void __launch_bounds__(256)
ssm_gate_bwd_k(const TIO *__restrict__ dout, int64_t dout_rs, const TY *__restrict__ y, int64_t y_rs,
               const TIO *__restrict__ xc, int64_t xc_rs, const TIO *__restrict__ z, int64_t z_rs,
               const float *__restrict__ D, TY *__restrict__ dy, int64_t dy_rs, TIO *__restrict__ dxc, int64_t dxc_rs,
               TIO *__restrict__ dz, int64_t dz_rs, float *__restrict__ dD_part, int64_t T, int Dn) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4 *red = reinterpret_cast<float4 *>(smem);  // [RP][CPR]
  const Geo g = make_geo(Dn);
  const int rr = threadIdx.x / g.CPR;
  const bool on = rr < g.RP;
  for (int c0 = 0; c0 < g.CPR; c0 += 256) {
    const int c = c0 + (on ? threadIdx.x - rr * g.CPR : 0);
    float4 acc = make_float4(0, 0, 0, 0);
    if (on && c < g.CPR) {
      const float4 d4 = ld4<float>(D + c * 4);
      for (int64_t t = (int64_t)blockIdx.x * g.RP + rr; t < T; t += (int64_t)gridDim.x * g.RP) {
        float4 go = ld4<TIO>(dout + t * dout_rs + c * 4), yv = ld4<TY>(y + t * y_rs + c * 4);
        float4 xv = ld4<TIO>(xc + t * xc_rs + c * 4), zv = ld4<TIO>(z + t * z_rs + c * 4);
        float gy[4], gx[4], gz[4];
        const float go_[4] = {go.x, go.y, go.z, go.w}, y_[4] = {yv.x, yv.y, yv.z, yv.w};
        const float x_[4] = {xv.x, xv.y, xv.z, xv.w}, z_[4] = {zv.x, zv.y, zv.z, zv.w}, d_[4] = {d4.x, d4.y, d4.z, d4.w};
        float a_[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float sz = siluf_(z_[j]);
          gy[j] = go_[j] * sz;
          gx[j] = gy[j] * d_[j];
          gz[j] = go_[j] * (y_[j] + d_[j] * x_[j]) * silu_grad(z_[j]);
          a_[j] += gy[j] * x_[j];
        }
        acc = make_float4(a_[0], a_[1], a_[2], a_[3]);
        st4<TY>(dy + t * dy_rs + c * 4, make_float4(gy[0], gy[1], gy[2], gy[3]));
        st4<TIO>(dxc + t * dxc_rs + c * 4, make_float4(gx[0], gx[1], gx[2], gx[3]));
        st4<TIO>(dz + t * dz_rs + c * 4, make_float4(gz[0], gz[1], gz[2], gz[3]));
      }
    }
    __syncthreads();
    if (on && c < g.CPR) red[rr * min(g.CPR, 256) + (c - c0)] = acc;
    __syncthreads();
    if (on && rr == 0 && c < g.CPR) {
      float4 s = red[c - c0];
      for (int r = 1; r < g.RP; ++r) {
        float4 v = red[r * min(g.CPR, 256) + (c - c0)];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      *reinterpret_cast<float4 *>(dD_part + (int64_t)blockIdx.x * Dn + c * 4) = s;
    }
  }
}

// ---------------------------------------------------------------- depthwise causal conv + SiLU
constexpr int CONV_TT = 16;  // tokens per thread run

// ---- run per thread: a thread owns four channels of a 16-token run, with the taps and the x window (in the backward also the
// dpre history) in KM-long register arrays.  The tap count is the template's KW (2..4, KM == KW: the model's widths) or, with
// KW == 0, the runtime k <= KM (5..16, an ssm_conv_kernel off the default path).  The arrays are right-aligned - tap q sits in
// slot off + q, off = KM - k - so every index is a constant once the loops unroll, and the wave-uniform tests `m >= off` skip
// the unused slots (no 0 * x terms: a non-finite value outside the window stays outside); with KW > 0, off is 0 and the tests
// fold away.  Every sum runs q ascending from the bias, whatever the mode: bias + sum_q w[q] * x[t - (k-1) + q].
constexpr int CONV_KMAX = 16;

template <typename T, int KM, int KW>
__global__ void __launch_bounds__(256)
dwconv_silu_fwd_k(const T *__restrict__ x, int64_t x_rs, const float *__restrict__ w, const float *__restrict__ bias,
                  T *__restrict__ out, int64_t out_rs, int64_t B, int64_t L, int Dn, int k_rt) {
  static_assert(KW == 0 || KW == KM, "a compile-time tap count fills the arrays");
  const int k = KW > 0 ? KW : k_rt, off = KM - k;
  const Geo g = make_geo(Dn);
  const int rr = threadIdx.x / g.CPR;
  if (rr >= g.RP) return;
  const int64_t runs_per_seq = ceil_div64(L, CONV_TT);
  for (int c = threadIdx.x - rr * g.CPR; c < g.CPR; c += 256) {
    float wv[4][KM], bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bv[j] = bias[c * 4 + j];
#pragma unroll
      for (int m = 0; m < KM; ++m) wv[j][m] = m >= off ? w[(c * 4 + j) * k + (m - off)] : 0.f;
    }
    for (int64_t run = (int64_t)blockIdx.x * g.RP + rr; run < B * runs_per_seq; run += (int64_t)gridDim.x * g.RP) {
      const int64_t b = run / runs_per_seq, t0 = (run - b * runs_per_seq) * CONV_TT;
      const T *xb = x + b * L * x_rs + c * 4;
      T *ob = out + b * L * out_rs + c * 4;
      float win[KM][4];  // win[m] = x[t-(KM-1)+m]
#pragma unroll
      for (int m = 0; m < KM - 1; ++m) {
        const int64_t tt = t0 - (KM - 1) + m;
        float4 v = (m >= off && tt >= 0) ? ld4<T>(xb + tt * x_rs) : make_float4(0, 0, 0, 0);
        win[m + 1][0] = v.x; win[m + 1][1] = v.y; win[m + 1][2] = v.z; win[m + 1][3] = v.w;
      }
      const int64_t t1 = min(t0 + CONV_TT, L);
      for (int64_t t = t0; t < t1; ++t) {
#pragma unroll
        for (int m = 0; m < KM - 1; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j) win[m][j] = win[m + 1][j];
        float4 v = ld4<T>(xb + t * x_rs);
        win[KM - 1][0] = v.x; win[KM - 1][1] = v.y; win[KM - 1][2] = v.z; win[KM - 1][3] = v.w;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float s = bv[j];
#pragma unroll
          for (int m = 0; m < KM; ++m)
            if (m >= off) s += wv[j][m] * win[m][j];
          s = to_f32(from_f32<T>(s));  // conv output is stored in the activation dtype before SiLU
          o[j] = siluf_(s);
        }
        st4<T>(ob + t * out_rs, make_float4(o[0], o[1], o[2], o[3]));
      }
    }
  }
}

// ---- tile form of the forward (round 2).  The run-per-thread kernel above keeps ONE 8-byte load in flight per thread and
// touches a row as 44 separate pieces: 2.3 TB/s.  Here a work-group takes (batch, 64 tokens): the 64 + KW - 1 input rows
// arrive as 16-byte pieces, several per thread in flight, into an LDS tile laid out like the rows; then thread (rg, p)
// owns piece p of rows rg, rg + RG, ... - its EPC channels' taps stay in registers, the KW input pieces of an output come
// from LDS (consecutive lanes = consecutive 16-byte pieces: conflict-free ds_read_b128), and a wave's stores cover whole
// consecutive rows.  silu through the hardware exp2 / rcp (1 ulp each), as in scan_gate.hip.
constexpr int CONV_TILE_T = 64;
template <typename T> struct Pc16;
template <> struct Pc16<float> {
  static constexpr int EPC = 4;
  __device__ static __forceinline__ void unpack(const uint4 &v, float (&f)[4]) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
  }
  __device__ static __forceinline__ uint4 pack(const float (&f)[4]) {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  }
};
template <> struct Pc16<bf16_t> {
  static constexpr int EPC = 8;
  __device__ static __forceinline__ void unpack(const uint4 &v, float (&f)[8]) {
    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[2 * k] = __uint_as_float(u[k] << 16); f[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u); }
  }
  __device__ static __forceinline__ uint4 pack(const float (&f)[8]) {
    bf16_t e[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = (bf16_t)f[k];
    uint4 v;
    __builtin_memcpy(&v, e, 16);
    return v;
  }
};

// global -> LDS: `total` 16-byte pieces of `nrow` rows (row r of the tile = token t_first + r; rows outside [0, L) are zeros)
__device__ __forceinline__ void conv_tile_in(char *lds, const char *g, int64_t rs_bytes, int64_t t_first, int64_t L, int nrow,
                                             int PCS, int tid) {
  const int total = nrow * PCS;
  for (int i0 = tid; i0 < total; i0 += 1024) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 256;
      const int r = i / PCS, pc = i - r * PCS;
      const int64_t t = t_first + r;
      v[u] = (i < total && t >= 0 && t < L) ? *reinterpret_cast<const uint4 *>(g + t * rs_bytes + pc * 16) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * 256;
      if (i < total) *reinterpret_cast<uint4 *>(lds + (size_t)i * 16) = v[u];
    }
  }
}

template <typename T, int KW>
__global__ void __launch_bounds__(256)
dwconv_silu_fwd_tile_k(const T *__restrict__ x, int64_t x_rs, const float *__restrict__ w, const float *__restrict__ bias,
                       T *__restrict__ out, int64_t out_rs, int64_t L, int PCS, int RG, int nchunks) {
  typedef Pc16<T> PC;
  constexpr int EPC = PC::EPC, TT = CONV_TILE_T;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [TT + KW - 1][PCS * 16 B]
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / nchunks;
  const int64_t t0 = (int64_t)(blockIdx.x - b * nchunks) * TT;
  const int rows = (int)min((int64_t)TT, L - t0);
  const int rg = tid / PCS, p = tid - rg * PCS;
  const bool on = rg < RG;
  float wv[EPC][KW], bv[EPC];
  if (on) {
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      bv[j] = bias[p * EPC + j];
#pragma unroll
      for (int q = 0; q < KW; ++q) wv[j][q] = w[(p * EPC + j) * KW + q];
    }
  }
  conv_tile_in(smem, reinterpret_cast<const char *>(x + b * L * x_rs), x_rs * (int64_t)sizeof(T), t0 - (KW - 1), L, rows + KW - 1,
               PCS, tid);
  __syncthreads();
  if (!on) return;
  const int rowb = PCS * 16;
  char *ob = reinterpret_cast<char *>(out + (b * L + t0) * out_rs) + p * 16;
  for (int r = rg; r < rows; r += RG) {
    float acc[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) acc[j] = bv[j];
#pragma unroll
    for (int q = 0; q < KW; ++q) {
      float f[EPC];
      PC::unpack(*reinterpret_cast<const uint4 *>(smem + (r + q) * rowb + p * 16), f);
#pragma unroll
      for (int j = 0; j < EPC; ++j) acc[j] += wv[j][q] * f[j];
    }
    float o[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) {
      const float s = to_f32(from_f32<T>(acc[j]));  // conv output is stored in the activation dtype before SiLU
      o[j] = s * sigmoidf_(s);
    }
    *reinterpret_cast<uint4 *>(ob + (int64_t)r * out_rs * (int64_t)sizeof(T)) = PC::pack(o);
  }
}

// ---- BOUNDED rows: a token's sequence begins somewhere inside its batch row, and a tap in front of that boundary reads as
// zero - what t - j < 0 is to the kernels above.  Two layouts:
//   PACKED rows (training under ops.ssm.SSM_PACKED): a batch row holds several documents, contiguous runs of tokens, and token
//   t of row b belongs to the document [start[b, t], end[b, t]) (int32 [B, L], ops.document_layout).  The conv stops at a
//   document's first token, so every document gets what it gets in a row of its own.
//   LEFT-PADDED rows (generate()'s prefill under ops.ssm.SSM_LEFT_PAD, forward only): batch row b's sequence begins at token
//   start[b] (int32 [B], clamped to [0, L]).  The output rows before it are exact zeros, so that x_param_proj (no bias) hands
//   the scan Bt = C = dt_in = 0 there and the state stays at 0 up to the first real token.
// Forward, one kernel for both (ROW: the boundary is one start per batch row, else one per token), every width 2..16 and every
// Dn % 4 == 0: a work-group takes (batch, 64 tokens, CB <= 64 four-channel chunks), thread (rg, p) owns chunk p of rows rg,
// rg + RG, ..., and the taps sit in LDS transposed to [k][CB], so that one 16-byte read brings tap q of a thread's four
// channels.  One int per tile row says how many of its leading taps lie before the boundary, and the row masks them with a
// select in front of the multiply: whatever the tile holds there (a left-padded row's pad inputs are loaded like any other)
// never reaches a product, and the product with the zero is still added, as the kernels above add the zeros they load in
// front of a sequence: bias + sum_q w[q] * x[t - (k-1) + q], q ascending, rounded to the io dtype before SiLU, term for term -
// a document's, or a left-padded row's, outputs carry the bits the plain forward gives it alone.  A row whose count reaches k
// lies before the boundary itself: a pad row, which stores its zeros and computes nothing (a token of a document never gets
// there: it is in its own document).  The tile holds the rows as stored (8 bytes per chunk in bf16, not 16): the packed form
// runs in every layer of every training step, and at Dn = 176, k = 4 an fp32 tile's 47 KiB would leave three work-groups per
// CU where the stored form's 24 KiB leaves six.
template <typename T> struct Raw4;
template <> struct Raw4<float> {
  typedef float4 R;
  __device__ static __forceinline__ R zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ static __forceinline__ R load(const float *p) { return *reinterpret_cast<const float4 *>(p); }
  __device__ static __forceinline__ float4 f4(R v) { return v; }
};
template <> struct Raw4<bf16_t> {
  typedef uint2 R;
  __device__ static __forceinline__ R zero() { return make_uint2(0u, 0u); }
  __device__ static __forceinline__ R load(const bf16_t *p) { return *reinterpret_cast<const uint2 *>(p); }
  __device__ static __forceinline__ float4 f4(R u) {
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
};

template <typename T, bool ROW>
__global__ void __launch_bounds__(256)
dwconv_silu_bound_fwd_k(const T *__restrict__ x, int64_t x_rs, const float *__restrict__ w, const float *__restrict__ bias,
                        const int32_t *__restrict__ start, T *__restrict__ out, int64_t out_rs, int64_t L, int CPR, int k, int CB,
                        int nchunks, int ncb) {
  constexpr int TT = CONV_TILE_T;
  typedef Raw4<T> RW;
  typedef typename RW::R R;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4 *taps = reinterpret_cast<float4 *>(smem);              // [k][CB]
  R *tile = reinterpret_cast<R *>(taps + k * CB);               // [TT + k - 1][CB]; tile row j = token t0 - (k - 1) + j
  int32_t *st = reinterpret_cast<int32_t *>(tile + (TT + k - 1) * CB);   // [TT]: taps of tile row r + q with q < st[r] are masked
  const int tid = threadIdx.x;
  const int cb = (int)(blockIdx.x % ncb);
  const int64_t bt = blockIdx.x / ncb, b = bt / nchunks;
  const int64_t t0 = (bt - b * nchunks) * TT;
  const int rows = (int)min((int64_t)TT, L - t0);
  const int c_lo = cb * CB, nc = min(CB, CPR - c_lo);
  const T *xb = x + b * L * x_rs + c_lo * 4;
  T *ob = out + (b * L + t0) * out_rs + c_lo * 4;
  const int nrow = rows + k - 1;
  for (int i = tid; i < nrow * nc; i += 256) {
    const int r = i / nc, c = i - r * nc;
    const int64_t t = t0 - (k - 1) + r;
    tile[r * CB + c] = t >= 0 ? RW::load(xb + t * x_rs + c * 4) : RW::zero();
  }
  for (int i = tid; i < k * nc; i += 256) {
    const int q = i / nc, c = i - q * nc;
    const float *wc = w + (int64_t)(c_lo + c) * 4 * k + q;
    taps[q * CB + c] = make_float4(wc[0], wc[k], wc[2 * k], wc[3 * k]);
  }
  // token t - (k-1) + q lies before the boundary s of token t iff q < s - t + (k-1)   (<= k-1 for a token of a document)
  if (tid < rows) {
    int64_t n;
    if constexpr (ROW) {
      // a row may be longer than 2^31 tokens: the count is clamped from below as well before it narrows to an int (a token far
      // behind start[b] has a very negative one, which masks what 0 masks: nothing)
      const int64_t s = min(max((int64_t)start[b], (int64_t)0), L);
      n = max(s - (t0 + tid) + (k - 1), (int64_t)0);
    } else {
      n = (int64_t)start[b * L + t0 + tid] - (t0 + tid) + (k - 1);   // (L < 2^31 here: this fits an int)
    }
    st[tid] = (int32_t)min(n, (int64_t)k);
  }
  __syncthreads();
  const int rg = tid / CB, p = tid - rg * CB, RG = 256 / CB;
  if (rg >= RG || p >= nc) return;
  const float *bp = bias + (c_lo + p) * 4;
  const float4 bv = make_float4(bp[0], bp[1], bp[2], bp[3]);
  for (int r = rg; r < rows; r += RG) {
    const int lim = st[r];
    if constexpr (ROW) {
      if (lim == k) {
        st4<T>(ob + (int64_t)r * out_rs + p * 4, make_float4(0.f, 0.f, 0.f, 0.f));
        continue;
      }
    }
    float acc[4] = {bv.x, bv.y, bv.z, bv.w};
    for (int q = 0; q < k; ++q) {
      float4 f = RW::f4(tile[(r + q) * CB + p]);
      const float4 wq = taps[q * CB + p];
      if (q < lim) f = make_float4(0.f, 0.f, 0.f, 0.f);
      acc[0] += wq.x * f.x; acc[1] += wq.y * f.y; acc[2] += wq.z * f.z; acc[3] += wq.w * f.w;
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float sj = to_f32(from_f32<T>(acc[j]));  // conv output is stored in the activation dtype before SiLU
      o[j] = siluf_(sj);
    }
    st4<T>(ob + (int64_t)r * out_rs + p * 4, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// ---- backward, run per thread as the forward at the top (KM, KW: the same two modes; a thread owns four channels of a 16-token
// run): dpre[t] = dout[t] * silu'(pre[t]), dx[t] = sum_q w[q] * dpre[t + (k-1) - q], and per-block dw, db partials that
// colsum_rows_k folds in a fixed order - no atomics.  The walk runs KM - 1 tokens past the run: dx is emitted KM - 1 tokens
// behind it, dx[t - (KM-1)] = sum_q w[q] * dp[k-1-q] with w[q] = wv[off + q], i.e. slot KM-1-m of the taps meets slot m of the
// history; dpre of the next run's first k - 1 tokens feeds our dx but not our parameter gradients.
// DOC, packed rows (start, end as in the forward above; KW == 0, KM = 4 for the widths 2..4 and 16 for 5..16): pre is recomputed
// under the forward's predicate - where the walk reaches a document's first token (start[b, t] == t) the window in front of it
// is zeroed (the tokens of one document share their start, so the zeros hold until they leave the window), and the window a run
// begins with is masked by the start of its first token.  Hence dw[c, q] sums pairs of one document only.  dx takes a dpre at
// t' >= end[b, t] as zero, the select in front of the multiply as in the forward.  With one document per row every select
// passes exactly where the plain form reads a value it loaded, so dx carries its bits.  db is summed in fp64 there: it is one
// chain over every token of the batch, the longest sum of the kernel (see the fold at the end).
// (A tile form of the backward - x and dout rows in LDS, a thread walking six consecutive rows of one 16-byte piece with the x
// window and the last KW dpre values in registers - was built and measured: 111 us against 102 us for the run-per-thread
// kernel below at B=40, L=4096, Dn=176; 180 VGPRs leave two waves per SIMD for a walk that is all dependent LDS-read -> FMA
// chains.  Removed; the backward stays as it was.)
template <typename T, int KM, int KW, bool DOC>
__global__ void __launch_bounds__(256, DOC && KM == 4 ? 3 : 1)   // (DOC, KM = 4: the plain k = 4 form's three waves per SIMD - 168 VGPRs)
dwconv_silu_bwd_k(const T *__restrict__ x, int64_t x_rs, const float *__restrict__ w, const float *__restrict__ bias,
                  const T *__restrict__ dout, int64_t dout_rs, const T *__restrict__ dout2, int64_t dout2_rs,
                  const int32_t *__restrict__ start, const int32_t *__restrict__ end, T *__restrict__ dx, int64_t dx_rs,
                  float *__restrict__ dw_part, float *__restrict__ db_part, int64_t B, int64_t L, int Dn, int k_rt) {
  static_assert(KW == 0 || (KW == KM && !DOC), "a compile-time tap count fills the arrays; the packed form takes it at run time");
  typedef typename std::conditional<DOC, double, float>::type BSum;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [RP][CPR][4*KS]: per channel k tap sums, then the bias sum (DOC: as (hi, lo))
  float *red = reinterpret_cast<float *>(smem);
  const int k = KW > 0 ? KW : k_rt, off = KM - k, KS = k + (DOC ? 2 : 1), NA = 4 * KS;
  const Geo g = make_geo(Dn);
  const int rr = threadIdx.x / g.CPR;
  const bool on = rr < g.RP;
  const int64_t runs_per_seq = ceil_div64(L, CONV_TT);
  for (int c0 = 0; c0 < g.CPR; c0 += 256) {
    const int c = c0 + (on ? threadIdx.x - rr * g.CPR : 0);
    float accw[4][KM];
    BSum accb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { accb[j] = 0;
#pragma unroll
      for (int m = 0; m < KM; ++m) accw[j][m] = 0.f; }
    if (on && c < g.CPR) {
      float wv[4][KM], bv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bv[j] = bias[c * 4 + j];
#pragma unroll
        for (int m = 0; m < KM; ++m) wv[j][m] = m >= off ? w[(c * 4 + j) * k + (m - off)] : 0.f;
      }
      for (int64_t run = (int64_t)blockIdx.x * g.RP + rr; run < B * runs_per_seq; run += (int64_t)gridDim.x * g.RP) {
        const int64_t b = run / runs_per_seq, t0 = (run - b * runs_per_seq) * CONV_TT;
        const T *xb = x + b * L * x_rs + c * 4;
        const T *gb = dout + b * L * dout_rs + c * 4;
        // dout2: a second gradient of the same output (its other consumer's), added here as autograd's add kernel would have
        // added it - the sum rounded to T - instead of in a pass of its own
        const T *gb2 = dout2 ? dout2 + b * L * dout2_rs + c * 4 : nullptr;
        const int32_t *sb = DOC ? start + b * L : nullptr, *eb = DOC ? end + b * L : nullptr;
        T *dxb = dx + b * L * dx_rs + c * 4;
        // win[m] = x[t-(KM-1)+m] (zero in front of t's document), dp[m] = dpre[t-(KM-1)+m]; dpre is formed on [t0, te) and taken
        // as zero outside it (KW > 0: the loop bound already stops at t1 + KW - 1)
        const int64_t t1 = min(t0 + CONV_TT, L), te = KW > 0 ? L : min(t1 + (k - 1), L);
        float win[KM][4], dp[KM][4];
#pragma unroll
        for (int m = 0; m < KM; ++m)
#pragma unroll
          for (int j = 0; j < 4; ++j) { win[m][j] = 0.f; dp[m][j] = 0.f; }
        const int64_t s0 = DOC ? max((int64_t)sb[t0], (int64_t)0) : 0;   // the run's first token's document begins here
#pragma unroll
        for (int m = 0; m < KM - 1; ++m) {
          const int64_t tt = t0 - (KM - 1) + m;
          if (m >= off && tt >= s0) { float4 v = ld4<T>(xb + tt * x_rs); win[m + 1][0] = v.x; win[m + 1][1] = v.y; win[m + 1][2] = v.z; win[m + 1][3] = v.w; }
        }
        for (int64_t t = t0; t < t1 + (KM - 1); ++t) {
#pragma unroll
          for (int m = 0; m < KM - 1; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j) { win[m][j] = win[m + 1][j]; dp[m][j] = dp[m + 1][j]; }
          if (t < te) {
            float4 v = ld4<T>(xb + t * x_rs), gv = ld4<T>(gb + t * dout_rs);
            const bool first = DOC && (int64_t)sb[t] == t;   // a document begins here: nothing in front of it is its own
            if (gb2) {
              const float4 g2 = ld4<T>(gb2 + t * dout2_rs);
              gv = make_float4(to_f32(from_f32<T>(gv.x + g2.x)), to_f32(from_f32<T>(gv.y + g2.y)), to_f32(from_f32<T>(gv.z + g2.z)),
                               to_f32(from_f32<T>(gv.w + g2.w)));
            }
            if constexpr (DOC) {
#pragma unroll
              for (int m = 0; m < KM - 1; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) win[m][j] = first ? 0.f : win[m][j];
            }
            win[KM - 1][0] = v.x; win[KM - 1][1] = v.y; win[KM - 1][2] = v.z; win[KM - 1][3] = v.w;
            const float g_[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float s = bv[j];
#pragma unroll
              for (int m = 0; m < KM; ++m)
                if (m >= off) s += wv[j][m] * win[m][j];
              s = to_f32(from_f32<T>(s));
              float d = g_[j] * silu_grad(s);
              dp[KM - 1][j] = d;
              if (t < t1) {  // own tokens only: parameter gradients are not double counted
                accb[j] += (BSum)d;
#pragma unroll
                for (int m = 0; m < KM; ++m)
                  if (m >= off) accw[j][m] += d * win[m][j];
              }
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { win[KM - 1][j] = 0.f; dp[KM - 1][j] = 0.f; }
          }
          const int64_t tp = t - (KM - 1);
          if (tp >= t0) {  // (tp < t1 by the loop bound)
            const int64_t lim = DOC ? (int64_t)eb[tp] - tp : KM;   // dp[m] is dpre[tp + m]: inside tp's document iff m < lim
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float s = 0.f;
#pragma unroll
              for (int m = KM - 1; m >= 0; --m)  // q = k-1-m ascending
                if (m < k) s += wv[j][KM - 1 - m] * (m < lim ? dp[m][j] : 0.f);
              o[j] = s;
            }
            st4<T>(dxb + tp * dx_rs, make_float4(o[0], o[1], o[2], o[3]));
          }
        }
      }
    }
    const int cw = min(g.CPR, 256);
    __syncthreads();
    if (on && c < g.CPR) {
      float *r = red + ((int64_t)rr * cw + (c - c0)) * NA;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float hi = (float)accb[j];
        r[j * KS + k] = hi;
        if constexpr (DOC) r[j * KS + k + 1] = (float)(accb[j] - (double)hi);
#pragma unroll
        for (int m = 0; m < KM; ++m)
          if (m >= off) r[j * KS + (m - off)] = accw[j][m];
      }
    }
    __syncthreads();
    if (on && rr == 0 && c < g.CPR) {
      for (int j = 0; j < 4; ++j) {
        for (int q = 0; q <= k; ++q) {
          // (DOC: the rows' partials meet in fp64, off the token walk, and db - whose chains were fp64 already - comes over as a
          //  (hi, lo) pair: a packed row's dw then carries the rounding of the threads' own 16-token chains and one more, its
          //  db one rounding, as the short documents' do when each is run alone and summed outside.  Measured against the
          //  fp64 restatement at Dn = 4, L = 64, fp32: all-fp32 sums left db at 3.0e-6, the alone runs at 7.4e-7)
          BSum s = 0;
          for (int r = 0; r < g.RP; ++r) {
            const float *e = red + ((int64_t)r * cw + (c - c0)) * NA + j * KS;
            if constexpr (DOC) s += q < k ? (double)e[q] : (double)e[k] + (double)e[k + 1];
            else s += e[q];
          }
          if (q < k) dw_part[((int64_t)blockIdx.x * Dn + c * 4 + j) * k + q] = (float)s;
          else db_part[(int64_t)blockIdx.x * Dn + c * 4 + j] = (float)s;
        }
      }
    }
    __syncthreads();
  }
}

// out[c] = sum_r in[r][c], fixed order (16 row groups, four independent loads in flight)
__global__ void __launch_bounds__(1024)
colsum_rows_k(const float *__restrict__ in, float *__restrict__ out, int64_t rows, int64_t cols) {
  colsum_block(in, 0, rows, cols, [&](int64_t c, float t) { out[c] = t; });
}

// ---------------------------------------------------------------- residual + dropout
// y = res + keep/(1-p) * x  (the `output_dropout(block_out) + residual` of every sub-block,
// reference core.py:836-837,918-919) in one pass; the mask is the counter hash of (seed, index),
// regenerated by the backward.
template <typename TX, typename TR>
__global__ void __launch_bounds__(256)
dropout_add_fwd_k(const TX *__restrict__ x, const TR *__restrict__ res, TR *__restrict__ y, int64_t n4, float drop_p,
                  uint64_t seed) {
  const float ks = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const uint32_t th = (uint32_t)(drop_p * 65536.f);
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n4; v += (int64_t)gridDim.x * blockDim.x) {
    float4 a = ld4<TX>(x + v * 4), r = ld4<TR>(res + v * 4);
    float e[4] = {a.x, a.y, a.z, a.w};
    if (drop_p > 0.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = drop_keep(seed, 0, v * 4 + j, 0, th) ? e[j] * ks : 0.f;
    }
    st4<TR>(y + v * 4, make_float4(r.x + e[0], r.y + e[1], r.z + e[2], r.w + e[3]));
  }
}

template <typename TG, typename TX>
__global__ void __launch_bounds__(256)
dropout_bwd_k(const TG *__restrict__ g, TX *__restrict__ dx, int64_t n4, float drop_p, uint64_t seed) {
  const float ks = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  const uint32_t th = (uint32_t)(drop_p * 65536.f);
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n4; v += (int64_t)gridDim.x * blockDim.x) {
    float4 a = ld4<TG>(g + v * 4);
    float e[4] = {a.x, a.y, a.z, a.w};
    if (drop_p > 0.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = drop_keep(seed, 0, v * 4 + j, 0, th) ? e[j] * ks : 0.f;
    }
    st4<TX>(dx + v * 4, make_float4(e[0], e[1], e[2], e[3]));
  }
}

// ---------------------------------------------------------------- cast (+ transposed copy)
template <typename TO>
__global__ void __launch_bounds__(256)
cast_transpose_k(const float *__restrict__ src, TO *__restrict__ dst, TO *__restrict__ dstT, int R, int C, int ld_dst,
                 int ld_dstT) {
  __shared__ float tile[64][65];
  const int64_t e = blockIdx.z;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const float *s = src + e * (int64_t)R * C;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int i = ty; i < 64; i += 4) {
    int r = r0 + i, c = c0 + tx;
    float v = (r < R && c < C) ? s[(int64_t)r * C + c] : 0.f;
    tile[i][tx] = v;
    if (dst && r < R && c < ld_dst) dst[e * (int64_t)R * ld_dst + (int64_t)r * ld_dst + c] = from_f32<TO>(v);   // pad columns: 0
  }
  __syncthreads();
  if (dstT)
    for (int i = ty; i < 64; i += 4) {
      int c = c0 + i, r = r0 + tx;
      if (r < ld_dstT && c < C) dstT[e * (int64_t)C * ld_dstT + (int64_t)c * ld_dstT + r] = from_f32<TO>(tile[tx][i]);
    }
}

// The same with four columns per thread (round 3): 16-byte loads, 8-byte (bf16) / 16-byte (fp32) stores of both copies - the
// scalar form above moved its bytes at 2.6 TB/s (2-byte stores, 128 bytes per wave instruction).  Needs C, ld_dst and ld_dstT
// multiples of 4 and 16-byte aligned bases (the launcher checks).
template <typename TO> struct out4;
template <> struct out4<bf16_t> {
  __device__ static __forceinline__ void store(bf16_t *p, float a, float b, float c, float d) {
    typedef __attribute__((ext_vector_type(4))) bf16_t bf4;
    const bf4 v = {(bf16_t)a, (bf16_t)b, (bf16_t)c, (bf16_t)d};
    *reinterpret_cast<bf4 *>(p) = v;
  }
};
template <> struct out4<float> {
  __device__ static __forceinline__ void store(float *p, float a, float b, float c, float d) {
    *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d);
  }
};
template <typename TO>
__global__ void __launch_bounds__(256)
cast_transpose4_k(const float *__restrict__ src, TO *__restrict__ dst, TO *__restrict__ dstT, int R, int C, int ld_dst,
                  int ld_dstT) {
  __shared__ float tile[64][65];
  const int64_t e = blockIdx.z;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const float *s = src + e * (int64_t)R * C;
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;        // column quad, row (resp. column) within a pass of 16
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rl = g + 16 * i, r = r0 + rl, c = c0 + q * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < R && c < C) v = *reinterpret_cast<const float4 *>(s + (int64_t)r * C + c);
    tile[rl][q * 4 + 0] = v.x; tile[rl][q * 4 + 1] = v.y; tile[rl][q * 4 + 2] = v.z; tile[rl][q * 4 + 3] = v.w;
    if (dst && r < R && c < ld_dst) out4<TO>::store(dst + e * (int64_t)R * ld_dst + (int64_t)r * ld_dst + c, v.x, v.y, v.z, v.w);   // pad columns: 0
  }
  __syncthreads();
  if (dstT) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cl = g + 16 * i, c = c0 + cl, r = r0 + q * 4;
      if (r < ld_dstT && c < C)
        out4<TO>::store(dstT + e * (int64_t)C * ld_dstT + (int64_t)c * ld_dstT + r, tile[q * 4 + 0][cl], tile[q * 4 + 1][cl],
                        tile[q * 4 + 2][cl], tile[q * 4 + 3][cl]);
    }
  }
}

// The same for MANY weights in one launch (round 4; the training step's compute copies, prepared once per step): a table of
// matrices [R, C] fp32 -> bf16 copy (rows at `rowmap[r]` if given, pitch ld_plain) and bf16 transposed copy (pitch ld_tr), a
// work-group per 64 x 64 tile found by bisection over the entries' first-tile indices.  Pad rows / columns of the
// destinations are never written (the caller zero-fills them once).  The conversion is apertis_cast_transpose's (RNE).
struct WPEntry {
  const float *src; bf16_t *plain; bf16_t *tr; const int32_t *rowmap;
  int32_t R, C, ld_plain, ld_tr, tiles_c, tile0, pad0, pad1;
};
__global__ void __launch_bounds__(256)
weight_prep_k(const WPEntry *__restrict__ tab, int n_entries) {
  __shared__ float tile[64][65];
  const int t = (int)blockIdx.x;
  int lo = 0, hi = n_entries - 1;
  while (lo < hi) {                       // the last entry whose first tile is <= t
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].tile0 <= t) lo = mid; else hi = mid - 1;
  }
  const WPEntry en = tab[lo];
  const int lt = t - en.tile0, tr_ = lt / en.tiles_c, r0 = tr_ * 64, c0 = (lt - tr_ * en.tiles_c) * 64;
  const int R = en.R, C = en.C;
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rl = g + 16 * i, r = r0 + rl, c = c0 + q * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < R && c < C) {
      v = *reinterpret_cast<const float4 *>(en.src + (int64_t)r * C + c);
      if (en.plain) out4<bf16_t>::store(en.plain + (int64_t)(en.rowmap ? en.rowmap[r] : r) * en.ld_plain + c, v.x, v.y, v.z, v.w);
    }
    tile[rl][q * 4 + 0] = v.x; tile[rl][q * 4 + 1] = v.y; tile[rl][q * 4 + 2] = v.z; tile[rl][q * 4 + 3] = v.w;
  }
  __syncthreads();
  if (en.tr) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cl = g + 16 * i, c = c0 + cl, r = r0 + q * 4;
      if (c >= C || r >= R) continue;
      bf16_t *row = en.tr + (int64_t)c * en.ld_tr;
      if (!en.rowmap && r + 3 < R) {
        out4<bf16_t>::store(row + r, tile[q * 4 + 0][cl], tile[q * 4 + 1][cl], tile[q * 4 + 2][cl], tile[q * 4 + 3][cl]);
      } else {
        for (int k = 0; k < 4; ++k)
          if (r + k < R) row[en.rowmap ? en.rowmap[r + k] : r + k] = (bf16_t)tile[q * 4 + k][cl];
      }
    }
  }
}

int gate_blocks(int64_t T, int64_t Dn) {
  Geo g = make_geo(Dn);
  int64_t nb = ceil_div64(T, (int64_t)g.RP * 8);
  return (int)std::max<int64_t>(1, std::min<int64_t>(nb, 2048));
}
int conv_blocks(int64_t B, int64_t L, int64_t Dn) {
  Geo g = make_geo(Dn);
  int64_t runs = B * ceil_div64(L, CONV_TT);
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(runs, g.RP), 4096));
}
// the tile form's LDS: TT + k - 1 rows of PCS = Dn / EPC 16-byte pieces; one work-group may hold at most the CU's 160 KiB
constexpr int64_t CONV_TILE_LDS_MAX = 160 * 1024;
int64_t conv_tile_lds(int64_t Dn, int64_t k, int dtype_io) {
  return (CONV_TILE_T + k - 1) * (Dn / (dtype_io == APERTIS_BF16 ? 8 : 4)) * 16;
}
bool conv_tile_ok(int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io, std::initializer_list<const void *> ptrs,
                  std::initializer_list<int64_t> strides) {
  const int64_t es = dtype_io == APERTIS_BF16 ? 2 : 4, epc = 16 / es;
  if (Dn % epc != 0 || Dn / epc > 256 || B * ceil_div64(L, CONV_TILE_T) >= 0x7fffffffLL || k < 2 || k > 4) return false;
  if (conv_tile_lds(Dn, k, dtype_io) > CONV_TILE_LDS_MAX) return false;
  for (const void *q : ptrs) if (((uintptr_t)q) % 16) return false;
  for (int64_t r : strides) if ((r * es) % 16) return false;
  return true;
}
bool rows_ok(int64_t Dn) { return Dn > 0 && Dn % 4 == 0 && Dn <= 4 * 4096; }

}  // namespace

extern "C" int64_t apertis_ssm_gate_bwd_blocks(int64_t T, int64_t Dn) { return gate_blocks(T, Dn); }
extern "C" int64_t apertis_dwconv_bwd_blocks(int64_t B, int64_t L, int64_t Dn) { return conv_blocks(B, L, Dn); }

#define GATE_TYPES(dy_, dio_, ...)                                                                    \
  do {                                                                                                \
    if ((dy_) == APERTIS_F32 && (dio_) == APERTIS_F32) { typedef float TY; typedef float TIO; __VA_ARGS__; }        \
    else if ((dy_) == APERTIS_F32 && (dio_) == APERTIS_BF16) { typedef float TY; typedef bf16_t TIO; __VA_ARGS__; } \
    else if ((dy_) == APERTIS_BF16 && (dio_) == APERTIS_BF16) { typedef bf16_t TY; typedef bf16_t TIO; __VA_ARGS__; } \
    else return APERTIS_ERR_UNSUPPORTED;                                                              \
  } while (0)

extern "C" int apertis_ssm_gate_fwd(const void *y, int64_t y_rs, const void *xc, int64_t xc_rs, const void *z,
                                    int64_t z_rs, const float *D, void *out, int64_t out_rs, int64_t T, int64_t Dn,
                                    int dtype_y, int dtype_io, void *stream) {
  if (!y || !xc || !z || !D || !out || T < 0) return APERTIS_ERR_ARG;
  if (!rows_ok(Dn) || (y_rs | xc_rs | z_rs | out_rs) % 4) return APERTIS_ERR_UNSUPPORTED;
  if (T == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(gate_blocks(T, Dn)), block(256);
  GATE_TYPES(dtype_y, dtype_io, hipLaunchKernelGGL((ssm_gate_fwd_k<TY, TIO>), grid, block, 0, st, (const TY *)y, y_rs,
                                                   (const TIO *)xc, xc_rs, (const TIO *)z, z_rs, D, (TIO *)out, out_rs, T,
                                                   (int)Dn));
  return apertis_check_launch();
}

extern "C" int apertis_ssm_gate_bwd(const void *dout, int64_t dout_rs, const void *y, int64_t y_rs, const void *xc,
                                    int64_t xc_rs, const void *z, int64_t z_rs, const float *D, void *dy, int64_t dy_rs,
                                    void *dxc, int64_t dxc_rs, void *dz, int64_t dz_rs, float *dD_part, float *dD,
                                    int64_t T, int64_t Dn, int dtype_y, int dtype_io, void *stream) {
  if (!dout || !y || !xc || !z || !D || !dy || !dxc || !dz || !dD_part || !dD || T < 0) return APERTIS_ERR_ARG;
  if (!rows_ok(Dn) || (dout_rs | y_rs | xc_rs | z_rs | dy_rs | dxc_rs | dz_rs) % 4) return APERTIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = gate_blocks(T, Dn);
  Geo g = make_geo(Dn);
  size_t lds = (size_t)g.RP * std::min(g.CPR, 256) * sizeof(float4);
  dim3 grid(nblk), block(256);
  GATE_TYPES(dtype_y, dtype_io, launch_lds(ssm_gate_bwd_k<TY, TIO>, grid, block, lds, st, (const TIO *)dout,
                                                   dout_rs, (const TY *)y, y_rs, (const TIO *)xc, xc_rs, (const TIO *)z,
                                                   z_rs, D, (TY *)dy, dy_rs, (TIO *)dxc, dxc_rs, (TIO *)dz, dz_rs, dD_part,
                                                   T, (int)Dn));
  hipLaunchKernelGGL(colsum_rows_k, dim3((unsigned)ceil_div64(Dn, 64)), dim3(1024), 0, st, dD_part, dD, (int64_t)nblk, Dn);
  return apertis_check_launch();
}

#define CONV_DISPATCH(k_, dt_, ...)                                                             \
  do {                                                                                          \
    if ((dt_) == APERTIS_F32) { typedef float T;                                                \
      if ((k_) == 2) { constexpr int KW = 2; __VA_ARGS__; } else if ((k_) == 3) { constexpr int KW = 3; __VA_ARGS__; } \
      else if ((k_) == 4) { constexpr int KW = 4; __VA_ARGS__; } else return APERTIS_ERR_UNSUPPORTED; }  \
    else if ((dt_) == APERTIS_BF16) { typedef bf16_t T;                                         \
      if ((k_) == 2) { constexpr int KW = 2; __VA_ARGS__; } else if ((k_) == 3) { constexpr int KW = 3; __VA_ARGS__; } \
      else if ((k_) == 4) { constexpr int KW = 4; __VA_ARGS__; } else return APERTIS_ERR_UNSUPPORTED; }  \
    else return APERTIS_ERR_ARG;                                                                \
  } while (0)

#define CONV_TYPES(dt_, ...)                                                                    \
  do {                                                                                          \
    if ((dt_) == APERTIS_F32) { typedef float T; __VA_ARGS__; }                                 \
    else if ((dt_) == APERTIS_BF16) { typedef bf16_t T; __VA_ARGS__; }                          \
    else return APERTIS_ERR_ARG;                                                                \
  } while (0)

extern "C" int apertis_dwconv_silu_fwd(const void *x, int64_t x_rs, const float *w, const float *bias, void *out,
                                       int64_t out_rs, int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io,
                                       void *stream) {
  if (!x || !w || !bias || !out || B < 0 || L < 0) return APERTIS_ERR_ARG;
  if (!rows_ok(Dn) || (x_rs | out_rs) % 4) return APERTIS_ERR_UNSUPPORTED;
  if (B == 0 || L == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  // tile form when every row is whole 16-byte pieces at 16-byte-aligned addresses (the model's shapes) and the tile fits the
  // LDS, else run per thread (widths 5..16: the runtime-width kernel)
  if (conv_tile_ok(B, L, Dn, k, dtype_io, {x, out}, {x_rs, out_rs})) {
    const int64_t epc = dtype_io == APERTIS_BF16 ? 8 : 4;
    const int PCS = (int)(Dn / epc), RG = 256 / PCS, nchunks = (int)ceil_div64(L, CONV_TILE_T);
    const size_t lds = (size_t)conv_tile_lds(Dn, k, dtype_io);
    CONV_DISPATCH(k, dtype_io, launch_lds(dwconv_silu_fwd_tile_k<T, KW>, dim3((unsigned)(B * nchunks)), dim3(256), lds, st,
                                          (const T *)x, x_rs, w, bias, (T *)out, out_rs, L, PCS, RG, nchunks));
    return apertis_check_launch();
  }
  dim3 grid(conv_blocks(B, L, Dn)), block(256);
  if (k > 4 && k <= CONV_KMAX) {
    CONV_TYPES(dtype_io, hipLaunchKernelGGL((dwconv_silu_fwd_k<T, CONV_KMAX, 0>), grid, block, 0, st, (const T *)x, x_rs, w, bias,
                                            (T *)out, out_rs, B, L, (int)Dn, (int)k));
    return apertis_check_launch();
  }
  CONV_DISPATCH(k, dtype_io, hipLaunchKernelGGL((dwconv_silu_fwd_k<T, KW, KW>), grid, block, 0, st, (const T *)x, x_rs, w, bias,
                                                (T *)out, out_rs, B, L, (int)Dn, (int)k));
  return apertis_check_launch();
}

// the bounded forward of both layouts: `row` - start is [B], one boundary per batch row (left-padded), else [B, L] (packed)
static int conv_bound_fwd(bool row, const void *x, int64_t x_rs, const float *w, const float *bias, const int32_t *start, void *out,
                          int64_t out_rs, int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io, void *stream) {
  if (!x || !w || !bias || !start || !out || B < 0 || L < 0) return APERTIS_ERR_ARG;
  if (dtype_io != APERTIS_F32 && dtype_io != APERTIS_BF16) return APERTIS_ERR_ARG;
  // (a packed row's int32 starts cannot name a token past 2^31, and its kernel narrows start - t to an int.  The left-padded
  // form needs no such refusal: it keeps start[b] and the token index in 64 bits and clamps the count to [0, k] before it
  // narrows, so a row of any length that the grid holds goes through)
  if (!rows_ok(Dn) || (x_rs | out_rs) % 4 || x_rs < Dn || out_rs < Dn || k < 2 || k > CONV_KMAX || (!row && L >= 0x7fffffffLL))
    return APERTIS_ERR_UNSUPPORTED;
  const uintptr_t piece = dtype_io == APERTIS_BF16 ? 8 : 16;        // a thread moves four channels at a time
  if ((uintptr_t)x % piece || (uintptr_t)out % piece) return APERTIS_ERR_UNSUPPORTED;
  if (B == 0 || L == 0) return APERTIS_OK;
  const int CPR = (int)(Dn / 4), CB = std::min(CPR, 64);
  const int64_t nchunks = ceil_div64(L, CONV_TILE_T), ncb = ceil_div64(CPR, CB);
  if (nchunks >= 0x7fffffffLL || B * nchunks * ncb >= 0x7fffffffLL) return APERTIS_ERR_UNSUPPORTED;
  // taps + tile as stored + the tile's counts: at most 16 + 79 KiB at k = 16, fp32; 27 KiB at k = 4, Dn = 176, bf16
  const size_t lds = (size_t)k * CB * sizeof(float4) + (size_t)(CONV_TILE_T + k - 1) * CB * piece + CONV_TILE_T * sizeof(int32_t);
  const dim3 grid((unsigned)(B * nchunks * ncb)), block(256);
#define BOUND_FWD(ROW_)                                                                                                          \
  CONV_TYPES(dtype_io, launch_lds(dwconv_silu_bound_fwd_k<T, ROW_>, grid, block, lds, (hipStream_t)stream, (const T *)x, x_rs, w, \
                                  bias, start, (T *)out, out_rs, L, CPR, (int)k, CB, (int)nchunks, (int)ncb))
  if (row) BOUND_FWD(true); else BOUND_FWD(false);
#undef BOUND_FWD
  return apertis_check_launch();
}

extern "C" int apertis_dwconv_silu_start_fwd(const void *x, int64_t x_rs, const float *w, const float *bias, const int32_t *start,
                                             void *out, int64_t out_rs, int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io,
                                             void *stream) {
  return conv_bound_fwd(true, x, x_rs, w, bias, start, out, out_rs, B, L, Dn, k, dtype_io, stream);
}

extern "C" int apertis_dwconv_silu_doc_fwd(const void *x, int64_t x_rs, const float *w, const float *bias, const int32_t *start,
                                           void *out, int64_t out_rs, int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io,
                                           void *stream) {
  return conv_bound_fwd(false, x, x_rs, w, bias, start, out, out_rs, B, L, Dn, k, dtype_io, stream);
}

// the backward of the plain rows (`doc` false; start, end unused) and of packed rows
static int conv_bwd(bool doc, const void *x, int64_t x_rs, const float *w, const float *bias, const void *dout, int64_t dout_rs,
                    const void *dout2, int64_t dout2_rs, const int32_t *start, const int32_t *end, void *dx, int64_t dx_rs,
                    float *dw_part, float *db_part, float *dw, float *db, int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io,
                    void *stream) {
  if (!x || !w || !bias || !dout || !dx || !dw_part || !db_part || !dw || !db || B < 0 || L < 0) return APERTIS_ERR_ARG;
  // (the packed form refuses an unknown dtype here, the plain form after the shapes, where its dispatch meets it)
  if (doc && (!start || !end || (dtype_io != APERTIS_F32 && dtype_io != APERTIS_BF16))) return APERTIS_ERR_ARG;
  if (!dout2) dout2_rs = 0;
  if (!rows_ok(Dn) || (x_rs | dout_rs | dout2_rs | dx_rs) % 4 || k < 2 || k > CONV_KMAX || (doc && L >= 0x7fffffffLL))
    return APERTIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int nblk = conv_blocks(B, L, Dn);
  const Geo g = make_geo(Dn);
  // per chunk and channel k tap sums and the bias sum (packed: in two floats); up to 68 KiB at k = 16, 72 KiB packed
  const size_t lds = (size_t)g.RP * std::min(g.CPR, 256) * 4 * (k + (doc ? 2 : 1)) * sizeof(float);
  const dim3 grid(nblk), block(256);
#define CONV_BWD(KM_, KW_, DOC_)                                                                                                   \
  CONV_TYPES(dtype_io, launch_lds(dwconv_silu_bwd_k<T, KM_, KW_, DOC_>, grid, block, lds, st, (const T *)x, x_rs, w, bias,         \
                                  (const T *)dout, dout_rs, (const T *)dout2, dout2_rs, start, end, (T *)dx, dx_rs, dw_part, db_part, \
                                  B, L, (int)Dn, (int)k))
  if (doc) { if (k > 4) CONV_BWD(CONV_KMAX, 0, true); else CONV_BWD(4, 0, true); }
  else if (k > 4) CONV_BWD(CONV_KMAX, 0, false);
  else if (k == 4) CONV_BWD(4, 4, false);
  else if (k == 3) CONV_BWD(3, 3, false);
  else CONV_BWD(2, 2, false);
#undef CONV_BWD
  hipLaunchKernelGGL(colsum_rows_k, dim3((unsigned)ceil_div64(Dn * k, 64)), dim3(1024), 0, st, dw_part, dw, (int64_t)nblk,
                     Dn * k);
  hipLaunchKernelGGL(colsum_rows_k, dim3((unsigned)ceil_div64(Dn, 64)), dim3(1024), 0, st, db_part, db, (int64_t)nblk, Dn);
  return apertis_check_launch();
}

extern "C" int apertis_dwconv_silu_bwd2(const void *x, int64_t x_rs, const float *w, const float *bias, const void *dout,
                                        int64_t dout_rs, const void *dout2, int64_t dout2_rs, void *dx, int64_t dx_rs,
                                        float *dw_part, float *db_part, float *dw, float *db, int64_t B, int64_t L, int64_t Dn,
                                        int64_t k, int dtype_io, void *stream) {
  return conv_bwd(false, x, x_rs, w, bias, dout, dout_rs, dout2, dout2_rs, nullptr, nullptr, dx, dx_rs, dw_part, db_part, dw, db, B,
                  L, Dn, k, dtype_io, stream);
}

extern "C" int apertis_dwconv_silu_bwd(const void *x, int64_t x_rs, const float *w, const float *bias, const void *dout,
                                       int64_t dout_rs, void *dx, int64_t dx_rs, float *dw_part, float *db_part,
                                       float *dw, float *db, int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io,
                                       void *stream) {
  return apertis_dwconv_silu_bwd2(x, x_rs, w, bias, dout, dout_rs, nullptr, 0, dx, dx_rs, dw_part, db_part, dw, db, B, L, Dn, k,
                                  dtype_io, stream);
}

extern "C" int apertis_dwconv_silu_doc_bwd(const void *x, int64_t x_rs, const float *w, const float *bias, const void *dout,
                                           int64_t dout_rs, const void *dout2, int64_t dout2_rs, const int32_t *start,
                                           const int32_t *end, void *dx, int64_t dx_rs, float *dw_part, float *db_part, float *dw,
                                           float *db, int64_t B, int64_t L, int64_t Dn, int64_t k, int dtype_io, void *stream) {
  return conv_bwd(true, x, x_rs, w, bias, dout, dout_rs, dout2, dout2_rs, start, end, dx, dx_rs, dw_part, db_part, dw, db, B, L, Dn,
                  k, dtype_io, stream);
}

extern "C" int apertis_cast_transpose(const float *src, void *dst, void *dstT, int64_t E, int64_t R, int64_t C,
                                      int64_t ld_dst, int64_t ld_dstT, int dtype_out, void *stream) {
  if (!src || (!dst && !dstT) || E <= 0 || R <= 0 || C <= 0) return APERTIS_ERR_ARG;
  if (ld_dst == 0) ld_dst = C;
  if (ld_dstT == 0) ld_dstT = R;
  // the pad columns are written by the 64-wide tile that holds the last real column
  if (ld_dst < C || ld_dst > ceil_div64(C, 64) * 64 || ld_dstT < R || ld_dstT > ceil_div64(R, 64) * 64) return APERTIS_ERR_ARG;
  if (R > 0x3fffffff || C > 0x3fffffff || E > 65535 || ceil_div64(R, 64) > 65535) return APERTIS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)ceil_div64(C, 64), (unsigned)ceil_div64(R, 64), (unsigned)E), block(256);
  const bool vec4 = C % 4 == 0 && ld_dst % 4 == 0 && ld_dstT % 4 == 0 && (R * C) % 4 == 0 && ((uintptr_t)src) % 16 == 0 &&
                    ((uintptr_t)dst) % 16 == 0 && ((uintptr_t)dstT) % 16 == 0;
#define CT_GO(KERN, TO) hipLaunchKernelGGL(KERN<TO>, grid, block, 0, st, src, (TO *)dst, (TO *)dstT, (int)R, (int)C, (int)ld_dst, (int)ld_dstT)
  if (dtype_out == APERTIS_BF16) {
    if (vec4) CT_GO(cast_transpose4_k, bf16_t); else CT_GO(cast_transpose_k, bf16_t);
  } else if (dtype_out == APERTIS_F32) {
    if (vec4) CT_GO(cast_transpose4_k, float); else CT_GO(cast_transpose_k, float);
  } else {
    return APERTIS_ERR_ARG;
  }
#undef CT_GO
  return apertis_check_launch();
}

extern "C" int64_t apertis_weight_prep_entry_bytes(void) { return (int64_t)sizeof(WPEntry); }
extern "C" int apertis_weight_prep(const void *table, int64_t n_entries, int64_t total_tiles, void *stream) {
  if (!table || n_entries <= 0 || total_tiles <= 0 || n_entries > 0x7fffffff || total_tiles > 0x7fffffff) return APERTIS_ERR_ARG;
  hipLaunchKernelGGL(weight_prep_k, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, (const WPEntry *)table,
                     (int)n_entries);
  return apertis_check_launch();
}

extern "C" int apertis_colsum_f32(const float *in, float *out, int64_t rows, int64_t cols, void *stream) {
  if (!in || !out || rows < 0 || cols <= 0) return APERTIS_ERR_ARG;
  hipLaunchKernelGGL(colsum_rows_k, dim3((unsigned)ceil_div64(cols, 64)), dim3(1024), 0, (hipStream_t)stream, in, out, rows,
                     cols);
  return apertis_check_launch();
}

extern "C" int apertis_dropout_add_fwd(const void *x, const void *res, void *y, int64_t n, float drop_p, uint64_t seed,
                                       int dtype_x, int dtype_res, void *stream) {
  if (!x || !res || !y || n < 0 || drop_p < 0.f || drop_p >= 1.f) return APERTIS_ERR_ARG;
  if (n % 4) return APERTIS_ERR_UNSUPPORTED;
  if (n == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = std::min<int64_t>(ceil_div64(n / 4, 256), 8192);
  dim3 grid((unsigned)nb), block(256);
  if (dtype_x == APERTIS_BF16 && dtype_res == APERTIS_F32)
    hipLaunchKernelGGL((dropout_add_fwd_k<bf16_t, float>), grid, block, 0, st, (const bf16_t *)x, (const float *)res, (float *)y, n / 4, drop_p, seed);
  else if (dtype_x == APERTIS_F32 && dtype_res == APERTIS_F32)
    hipLaunchKernelGGL((dropout_add_fwd_k<float, float>), grid, block, 0, st, (const float *)x, (const float *)res, (float *)y, n / 4, drop_p, seed);
  else if (dtype_x == APERTIS_BF16 && dtype_res == APERTIS_BF16)
    hipLaunchKernelGGL((dropout_add_fwd_k<bf16_t, bf16_t>), grid, block, 0, st, (const bf16_t *)x, (const bf16_t *)res, (bf16_t *)y, n / 4, drop_p, seed);
  else
    return APERTIS_ERR_UNSUPPORTED;
  return apertis_check_launch();
}

extern "C" int apertis_dropout_bwd(const void *g, void *dx, int64_t n, float drop_p, uint64_t seed, int dtype_g,
                                   int dtype_x, void *stream) {
  if (!g || !dx || n < 0 || drop_p < 0.f || drop_p >= 1.f) return APERTIS_ERR_ARG;
  if (n % 4) return APERTIS_ERR_UNSUPPORTED;
  if (n == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = std::min<int64_t>(ceil_div64(n / 4, 256), 8192);
  dim3 grid((unsigned)nb), block(256);
  if (dtype_g == APERTIS_F32 && dtype_x == APERTIS_BF16)
    hipLaunchKernelGGL((dropout_bwd_k<float, bf16_t>), grid, block, 0, st, (const float *)g, (bf16_t *)dx, n / 4, drop_p, seed);
  else if (dtype_g == APERTIS_F32 && dtype_x == APERTIS_F32)
    hipLaunchKernelGGL((dropout_bwd_k<float, float>), grid, block, 0, st, (const float *)g, (float *)dx, n / 4, drop_p, seed);
  else if (dtype_g == APERTIS_BF16 && dtype_x == APERTIS_BF16)
    hipLaunchKernelGGL((dropout_bwd_k<bf16_t, bf16_t>), grid, block, 0, st, (const bf16_t *)g, (bf16_t *)dx, n / 4, drop_p, seed);
  else
    return APERTIS_ERR_UNSUPPORTED;
  return apertis_check_launch();
}
