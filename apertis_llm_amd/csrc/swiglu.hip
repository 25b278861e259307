// The SwiGLU gate of the `use_swiglu` feed-forward (reference core.py:925-993) for gfx950, forward and backward, on the output
// of ONE GEMM against the row-stacked weight [w_gate; w_up]:  gu [rows, 2F], columns [0, F) the gate pre-activation g, columns
// [F, 2F) u.  With s = sigmoid(g):
//   forward    h = g s u
//   backward   dg = dh u s (1 + g (1 - s)),   du = dh g s,   and (optionally) h again, so that the forward need not keep it.
//
// Bandwidth-bound and nothing else: a lane moves 16 bytes per access (8 bf16 / 4 fp32) of g, of u (F elements further) and of
// each output, the grid is capped and strides over the vectors of all rows, every offset is 64-bit (gu of a 1.5B-class step is
// past 4 GiB), the outputs leave on non-temporal stores (out_store16 in grouped_gemm.hip says why; the inputs are read once
// and stream the same way).  fp32 arithmetic in both dtypes: the IEEE expf / division for fp32 data, the hardware exp2 / rcp
// the GEMM epilogues use for bf16, one rounding per output.
#include "common.h"

namespace {

// blocks of a launch: 256 CUs x 8 blocks of 256 lanes; the rest of the vectors is reached by the stride
constexpr int SWIGLU_MAX_BLOCKS = 2048;
constexpr int SWIGLU_BLOCK = 256;

template <typename T> struct vec16;
template <> struct vec16<float> { static constexpr int N = 4; };
template <> struct vec16<bf16_t> { static constexpr int N = 8; };

typedef __attribute__((ext_vector_type(4))) unsigned swg_u4;

// 16 bytes, streamed, in their storage form; and as N floats
template <typename T> __device__ __forceinline__ swg_u4 load16(const T *p) {
  return __builtin_nontemporal_load(reinterpret_cast<const swg_u4 *>(p));
}
__device__ __forceinline__ void unpack16(const swg_u4 &t, float (&v)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = __uint_as_float(t[i]);
}
__device__ __forceinline__ void unpack16(const swg_u4 &t, float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(t[i] << 16);
    v[2 * i + 1] = __uint_as_float(t[i] & 0xffff0000u);
  }
}
template <typename T> __device__ __forceinline__ void store16(T *p, const float (&v)[vec16<T>::N]);
template <> __device__ __forceinline__ void store16<float>(float *p, const float (&v)[4]) {
  swg_u4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = __float_as_uint(v[i]);
  __builtin_nontemporal_store(o, reinterpret_cast<swg_u4 *>(p));
}
template <> __device__ __forceinline__ void store16<bf16_t>(bf16_t *p, const float (&v)[8]) {
  typedef __attribute__((ext_vector_type(8))) bf16_t bf8;
  bf8 o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (bf16_t)v[i];
  __builtin_nontemporal_store(__builtin_bit_cast(swg_u4, o), reinterpret_cast<swg_u4 *>(p));
}

// sigmoid(g).  exp(-g) overflows to +inf for g < -88.7: the quotient is then 0 and every product below stays finite
template <typename T> __device__ __forceinline__ float sigmoid_of(float g);
template <> __device__ __forceinline__ float sigmoid_of<float>(float g) { return 1.f / (1.f + expf(-g)); }
template <> __device__ __forceinline__ float sigmoid_of<bf16_t>(float g) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(g * -LOG2E_F));
}

// The walk both kernels share: vector i of the launch is (row i / Fv, vector i % Fv of the row); a lane starts at its global
// index and advances by the launch's lane count, carried as (rows, vectors) so that no 64-bit division runs in the loop.
struct Walk {
  int64_t r;
  int cv, dr, dc;
  __device__ __forceinline__ Walk(int Fv) {
    const uint32_t i0 = blockIdx.x * SWIGLU_BLOCK + threadIdx.x, stride = gridDim.x * SWIGLU_BLOCK;   // < 2^19 each
    r = i0 / (uint32_t)Fv, cv = (int)(i0 % (uint32_t)Fv);
    dr = (int)(stride / (uint32_t)Fv), dc = (int)(stride % (uint32_t)Fv);
  }
  __device__ __forceinline__ void next(int Fv) {
    r += dr, cv += dc;
    if (cv >= Fv) cv -= Fv, ++r;
  }
};

// Both kernels keep the NEXT vector's loads in flight while they work on the current one (16 bytes per operand in its storage
// form: 4 registers): with one vector per lane and pass the loads a CU has outstanding do not cover the HBM latency.
template <typename T>
__global__ void __launch_bounds__(SWIGLU_BLOCK)
swiglu_fwd_k(const T *__restrict__ gu, T *__restrict__ h, int64_t rows, int64_t F) {
  constexpr int N = vec16<T>::N;
  const int Fv = (int)(F / N);
  Walk w(Fv);
  if (w.r >= rows) return;
  const T *src = gu + w.r * (2 * F) + (int64_t)w.cv * N;
  swg_u4 gn = load16<T>(src), un = load16<T>(src + F);
  for (;;) {
    const swg_u4 gr = gn, ur = un;
    T *dst = h + w.r * F + (int64_t)w.cv * N;
    w.next(Fv);
    const bool more = w.r < rows;
    if (more) {
      src = gu + w.r * (2 * F) + (int64_t)w.cv * N;
      gn = load16<T>(src), un = load16<T>(src + F);
    }
    float g[N], u[N], o[N];
    unpack16(gr, g);
    unpack16(ur, u);
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = g[i] * sigmoid_of<T>(g[i]) * u[i];
    store16<T>(dst, o);
    if (!more) break;
  }
}

template <typename T, bool WITH_H>
__global__ void __launch_bounds__(SWIGLU_BLOCK)
swiglu_bwd_k(const T *__restrict__ dh, const T *__restrict__ gu, T *__restrict__ dgu, T *__restrict__ h_out, int64_t rows,
             int64_t F) {
  constexpr int N = vec16<T>::N;
  const int Fv = (int)(F / N);
  Walk w(Fv);
  if (w.r >= rows) return;
  int64_t ro = w.r * F + (int64_t)w.cv * N, rg = w.r * (2 * F) + (int64_t)w.cv * N;
  swg_u4 gn = load16<T>(gu + rg), un = load16<T>(gu + rg + F), dn = load16<T>(dh + ro);
  for (;;) {
    const swg_u4 gr = gn, ur = un, dr = dn;
    const int64_t co = ro, cg = rg;
    w.next(Fv);
    const bool more = w.r < rows;
    if (more) {
      ro = w.r * F + (int64_t)w.cv * N, rg = w.r * (2 * F) + (int64_t)w.cv * N;
      gn = load16<T>(gu + rg), un = load16<T>(gu + rg + F), dn = load16<T>(dh + ro);
    }
    float g[N], u[N], d[N], dg[N], du[N], o[N];
    unpack16(gr, g);
    unpack16(ur, u);
    unpack16(dr, d);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float s = sigmoid_of<T>(g[i]), gs = g[i] * s;
      dg[i] = d[i] * u[i] * s * (1.f + g[i] * (1.f - s));
      du[i] = d[i] * gs;
      o[i] = gs * u[i];      // (the forward's expression, operation for operation: the same bits)
    }
    store16<T>(dgu + cg, dg);
    store16<T>(dgu + cg + F, du);
    if constexpr (WITH_H) store16<T>(h_out + co, o);
    if (!more) break;
  }
}

bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// argument checks both entry points share: 0 to go on, else the code to return
int swiglu_check(int64_t rows, int64_t F, int dtype) {
  if (rows < 0 || F <= 0 || (dtype != APERTIS_F32 && dtype != APERTIS_BF16)) return APERTIS_ERR_ARG;
  if (F % (dtype == APERTIS_BF16 ? 8 : 4) || F > 0x3fffffffLL) return APERTIS_ERR_UNSUPPORTED;
  return APERTIS_OK;
}

unsigned swiglu_grid(int64_t rows, int64_t F, int dtype) {
  if (rows >= (int64_t)SWIGLU_MAX_BLOCKS * SWIGLU_BLOCK) return SWIGLU_MAX_BLOCKS;     // (and rows * vectors cannot overflow below)
  const int64_t vecs = rows * (F / (dtype == APERTIS_BF16 ? 8 : 4));
  const int64_t blocks = ceil_div64(vecs, SWIGLU_BLOCK);
  return (unsigned)(blocks < SWIGLU_MAX_BLOCKS ? blocks : SWIGLU_MAX_BLOCKS);
}

}  // namespace

extern "C" int apertis_swiglu_fwd(const void *gu, void *h, int64_t rows, int64_t F, int dtype, void *stream) {
  if (!gu || !h) return APERTIS_ERR_ARG;
  if (const int rc = swiglu_check(rows, F, dtype)) return rc;
  if (!al16(gu) || !al16(h)) return APERTIS_ERR_UNSUPPORTED;
  if (rows == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(swiglu_grid(rows, F, dtype)), block(SWIGLU_BLOCK);
  if (dtype == APERTIS_BF16)
    hipLaunchKernelGGL(swiglu_fwd_k<bf16_t>, grid, block, 0, st, (const bf16_t *)gu, (bf16_t *)h, rows, F);
  else
    hipLaunchKernelGGL(swiglu_fwd_k<float>, grid, block, 0, st, (const float *)gu, (float *)h, rows, F);
  return apertis_check_launch();
}

extern "C" int apertis_swiglu_bwd(const void *dh, const void *gu, void *dgu, void *h_out, int64_t rows, int64_t F, int dtype,
                                  void *stream) {
  if (!dh || !gu || !dgu) return APERTIS_ERR_ARG;
  if (const int rc = swiglu_check(rows, F, dtype)) return rc;
  if (!al16(dh) || !al16(gu) || !al16(dgu) || !al16(h_out)) return APERTIS_ERR_UNSUPPORTED;
  if (rows == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(swiglu_grid(rows, F, dtype)), block(SWIGLU_BLOCK);
#define SWIGLU_BWD(T, WITH_H)                                                                                          \
  hipLaunchKernelGGL((swiglu_bwd_k<T, WITH_H>), grid, block, 0, st, (const T *)dh, (const T *)gu, (T *)dgu, (T *)h_out, rows, F)
  if (dtype == APERTIS_BF16) {
    if (h_out) SWIGLU_BWD(bf16_t, true); else SWIGLU_BWD(bf16_t, false);
  } else {
    if (h_out) SWIGLU_BWD(float, true); else SWIGLU_BWD(float, false);
  }
#undef SWIGLU_BWD
  return apertis_check_launch();
}
