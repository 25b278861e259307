// Dead query rows of a causal attention with a key-padding mask (left padding): a row with no valid key at or before its own
// position.  The reference adds finfo.min (not -inf) for both masks, so every score of such a row saturates to one value and
// its softmax is uniform over ALL Lk keys, later and padded ones included: the row's output is the column mean of V[b, 0:Lk],
// the same vector for every head.  attn_fwd_k / attn_chunk_k write zeros there (l = 0); this kernel runs after them and
// overwrites exactly those rows.  It knows neither heads nor head dim: it works on the W = H * D columns.
#include "common.h"

namespace {

constexpr int DR_LANES = 16;                      // lanes across a column block: 16 x 16 bytes = 256 bytes of every row
constexpr int DR_GROUPS = 16;                     // row groups: a wave holds four of them, so one load covers four rows
constexpr int DR_THREADS = DR_LANES * DR_GROUPS;  // 256 threads, four waves

template <typename T> struct DrVec;               // 16 bytes of a row as fp32 values
template <> struct DrVec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float *p, float (&f)[4]) {
    const float4 x = *reinterpret_cast<const float4 *>(p);
    f[0] = x.x; f[1] = x.y; f[2] = x.z; f[3] = x.w;
  }
  static __device__ __forceinline__ void store(float *p, const float (&f)[4]) {
    *reinterpret_cast<float4 *>(p) = make_float4(f[0], f[1], f[2], f[3]);
  }
};
template <> struct DrVec<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16_t *p, float (&f)[8]) {
    const uint4 x = *reinterpret_cast<const uint4 *>(p);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ void store(bf16_t *p, const float (&f)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t lo = __builtin_bit_cast(unsigned short, from_f32<bf16_t>(f[2 * i]));
      const uint32_t hi = __builtin_bit_cast(unsigned short, from_f32<bf16_t>(f[2 * i + 1]));
      w[i] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

// grid (column blocks, B), 256 threads.  Thread (g, c) = (tid / 16, tid % 16) owns the 16 bytes at column (16 x + c) * N of
// the rows g, g + 16, ...: fp32 partial sums per thread, folded over the 16 row groups through LDS in group order.
template <typename T>
__global__ __launch_bounds__(DR_THREADS) void attn_dead_rows_k(const T *__restrict__ v, int64_t v_rs, int64_t v_bs,
                                                               const int64_t *__restrict__ key_valid, int64_t kv_rs,
                                                               T *__restrict__ out, int64_t out_rs, int64_t out_bs, int64_t Lq,
                                                               int64_t n, int64_t W) {
  constexpr int N = DrVec<T>::N;
  __shared__ long long s_first[DR_THREADS / APERTIS_WAVE];
  __shared__ float part[DR_GROUPS][DR_LANES * N];
  __shared__ __attribute__((aligned(16))) float mean[DR_LANES * N];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.y, Lk = n + Lq;

  // 1. first_valid[b]: the first nonzero column of the mask row, Lk if there is none (each thread stops at its first hit)
  const int64_t *kv = key_valid + b * kv_rs;
  long long first = Lk;
  for (int64_t j = tid; j < Lk; j += DR_THREADS)
    if (kv[j] != 0) { first = j; break; }
#pragma unroll
  for (int o = APERTIS_WAVE / 2; o > 0; o >>= 1) {
    const long long other = __shfl_xor(first, o, APERTIS_WAVE);
    first = other < first ? other : first;
  }
  if ((tid & (APERTIS_WAVE - 1)) == 0) s_first[tid / APERTIS_WAVE] = first;
  __syncthreads();
  first = s_first[0];
#pragma unroll
  for (int i = 1; i < DR_THREADS / APERTIS_WAVE; ++i) first = s_first[i] < first ? s_first[i] : first;

  // 2. rows 0 .. nd - 1 of the chunk are dead (row i sits at key position n + i); none: nothing of V is read (block-uniform)
  int64_t nd = first - n;
  nd = nd < 0 ? 0 : (nd > Lq ? Lq : nd);
  if (nd == 0) return;

  // 3. column sums of V[b, 0:Lk]
  const int c = tid % DR_LANES, g = tid / DR_LANES;
  const int64_t col = ((int64_t)blockIdx.x * DR_LANES + c) * N;       // (W % N == 0: a vector is inside the row or outside)
  float s[N];
#pragma unroll
  for (int e = 0; e < N; ++e) s[e] = 0.f;
  if (col < W) {
    const T *vb = v + b * v_bs + col;
    int64_t j = g;
    for (; j + 3 * DR_GROUPS < Lk; j += 4 * DR_GROUPS) {
      float a0[N], a1[N], a2[N], a3[N];
      DrVec<T>::load(vb + j * v_rs, a0);
      DrVec<T>::load(vb + (j + DR_GROUPS) * v_rs, a1);
      DrVec<T>::load(vb + (j + 2 * DR_GROUPS) * v_rs, a2);
      DrVec<T>::load(vb + (j + 3 * DR_GROUPS) * v_rs, a3);
#pragma unroll
      for (int e = 0; e < N; ++e) s[e] += (a0[e] + a1[e]) + (a2[e] + a3[e]);
    }
    for (; j < Lk; j += DR_GROUPS) {
      float a0[N];
      DrVec<T>::load(vb + j * v_rs, a0);
#pragma unroll
      for (int e = 0; e < N; ++e) s[e] += a0[e];
    }
  }
#pragma unroll
  for (int e = 0; e < N; ++e) part[g][c * N + e] = s[e];
  __syncthreads();
  if (tid < DR_LANES * N) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < DR_GROUPS; ++i) t += part[i][tid];
    mean[tid] = t / (float)Lk;
  }
  __syncthreads();

  // 4. the nd dead rows take the mean, rounded once to T
  if (col < W) {
    float m[N];
#pragma unroll
    for (int e = 0; e < N; ++e) m[e] = mean[c * N + e];
    T *ob = out + b * out_bs + col;
    for (int64_t i = g; i < nd; i += DR_GROUPS) DrVec<T>::store(ob + i * out_rs, m);
  }
}

}  // namespace

extern "C" int apertis_attention_dead_rows(const void *v, int64_t v_rs, int64_t v_bs, const int64_t *key_valid, int64_t kv_rs,
                                           void *out, int64_t out_rs, int64_t out_bs, int64_t B, int64_t Lq, int64_t n, int64_t W,
                                           int dtype, void *stream) {
  if (!v || !key_valid || !out) return APERTIS_ERR_ARG;
  if (B < 0 || Lq < 1 || n < 0 || W <= 0 || (dtype != APERTIS_F32 && dtype != APERTIS_BF16)) return APERTIS_ERR_ARG;
  const int64_t Lk = n + Lq, es = dtype == APERTIS_F32 ? 4 : 2, vec = 16 / es;
  if (v_rs < W || out_rs < W || kv_rs < Lk) return APERTIS_ERR_ARG;
  if (B > 1 && (v_bs < Lk * v_rs || out_bs < Lq * out_rs)) return APERTIS_ERR_ARG;
  if (B > 65535 || W % vec) return APERTIS_ERR_UNSUPPORTED;
  // 16-byte loads of V and 16-byte stores of the output: every row start on a 16-byte boundary
  const uint64_t bits = (uint64_t)(uintptr_t)v | (uint64_t)(uintptr_t)out | (uint64_t)(v_rs * es) | (uint64_t)(out_rs * es) |
                        (B > 1 ? (uint64_t)(v_bs * es) | (uint64_t)(out_bs * es) : 0u);
  if (bits & 15u) return APERTIS_ERR_UNSUPPORTED;
  if (B == 0) return APERTIS_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div64(W, DR_LANES * vec), (unsigned)B);
  if (dtype == APERTIS_F32)
    hipLaunchKernelGGL((attn_dead_rows_k<float>), grid, dim3(DR_THREADS), 0, st, (const float *)v, v_rs, v_bs, key_valid, kv_rs,
                       (float *)out, out_rs, out_bs, Lq, n, W);
  else
    hipLaunchKernelGGL((attn_dead_rows_k<bf16_t>), grid, dim3(DR_THREADS), 0, st, (const bf16_t *)v, v_rs, v_bs, key_valid, kv_rs,
                       (bf16_t *)out, out_rs, out_bs, Lq, n, W);
  return apertis_check_launch();
}
