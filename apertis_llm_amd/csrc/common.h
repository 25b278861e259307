// Shared device/host helpers for the gfx950 kernels.  gfx950 only: wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/apertis_hip.h"

#define APERTIS_WAVE 64

typedef __bf16 bf16_t;

template <typename T> struct dtype_of;
template <> struct dtype_of<float> { static constexpr int value = APERTIS_F32; };
template <> struct dtype_of<bf16_t> { static constexpr int value = APERTIS_BF16; };

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
// plain cast: hipcc emits v_cvt_pk_bf16_f32 (RNE, NaN-preserving) on gfx950
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float v) { return (bf16_t)v; }

static inline int apertis_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? APERTIS_OK : APERTIS_ERR_LAUNCH;
}

__host__ __device__ static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// hipLaunchKernelGGL with `lds` bytes of dynamic LDS: a request above the default 48 KiB raises the kernel's limit first
template <typename... P, typename... A>
static inline void launch_lds(void (*kf)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
  if (lds > 48 * 1024) hipFuncSetAttribute((const void *)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kf, grid, block, lds, st, args...);
}

// The fixed-order column fold of per-block partial rows, in[*][cols] fp32: the 1024-thread block x sums rows [r0, r1) of the
// columns c = 64 x + lane - 16 waves take every 16th row with four loads in flight, then wave 0 adds their 16 sums in order
// and hands each column's total to store(c, t) (c < cols).  The body of colsum_kernel, colsum_rows_k, fold_rows_k, ln_fold_k.
template <typename Store>
__device__ __forceinline__ void colsum_block(const float *__restrict__ in, int64_t r0, int64_t r1, int64_t cols, Store store) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  float s = 0.f;
  if (c < cols) {
    int64_t r = r0 + seg;
    for (; r + 48 < r1; r += 64) {
      float a0 = in[r * cols + c], a1 = in[(r + 16) * cols + c], a2 = in[(r + 32) * cols + c], a3 = in[(r + 48) * cols + c];
      s += (a0 + a1) + (a2 + a3);
    }
    for (; r < r1; r += 16) s += in[r * cols + c];
  }
  part[seg][lane] = s;
  __syncthreads();
  if (seg == 0 && c < cols) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i][lane];
    store(c, t);
  }
}

// The launches of that fold over rows [0, rows): one level, or for groups > 0 two - rows [g*rpg, (g+1)*rpg) into tmp[g][:]
// (rpg = ceil(rows / groups)), then those ng rows.  The level count changes the rounding: it stays each caller's choice.
// level(grid, in, rows, rpg, tmp) launches one level of the caller's fold kernel, into tmp if that is not NULL.
template <typename Level>
static inline void fold_levels(const float *in, float *tmp, int64_t rows, int64_t cols, int64_t groups, Level level) {
  const unsigned gx = (unsigned)ceil_div64(cols, 64);
  if (groups > 0) {
    const int64_t rpg = ceil_div64(rows, groups), ng = ceil_div64(rows, rpg);
    level(dim3(gx, (unsigned)ng), in, rows, rpg, tmp);
    level(dim3(gx), (const float *)tmp, ng, ng, (float *)nullptr);
  } else {
    level(dim3(gx), in, rows, rows, (float *)nullptr);
  }
}

// largest power-of-two byte width (<=16) that divides every value in the list
static inline int common_align(std::initializer_list<uint64_t> vals) {
  uint64_t o = 0;
  for (uint64_t v : vals) o |= v;
  int a = 16;
  while (a > 1 && (o & (uint64_t)(a - 1))) a >>= 1;
  return a;
}

// the 32-bit avalanche (murmur3 finaliser) behind every counter hash of the library: dropout masks, the sampling draw
__host__ __device__ __forceinline__ uint32_t hash_avalanche32(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// counter-based keep mask: 16 random bits per element from a 32-bit avalanche of
// (element pair index, seed); the backward regenerates it from the same (seed,row,col)
__device__ __forceinline__ bool drop_keep(uint64_t seed, int64_t row, int64_t col, int64_t ncols, uint32_t thresh16) {
  uint64_t lin = (uint64_t)row * (uint64_t)ncols + (uint64_t)col;
  uint32_t h = (uint32_t)(lin >> 1) ^ (uint32_t)seed;
  h += (uint32_t)(lin >> 33) * 0x9E3779B9u + (uint32_t)(seed >> 32);
  h = hash_avalanche32(h);
  uint32_t r16 = (lin & 1) ? (h >> 16) : (h & 0xffffu);
  return r16 >= thresh16;
}

// the same mask for 4 consecutive elements starting at a linear index that is a multiple of 4:
// two hashes instead of four
__device__ __forceinline__ uint32_t drop_hash_pair(uint64_t seed, uint64_t pair) {
  uint32_t h = (uint32_t)pair ^ (uint32_t)seed;
  h += (uint32_t)(seed >> 32);
  // the high word is zero below 2^33 elements: a wave-uniform branch (hipcc if-converts a per-lane one and keeps
  // the quarter-rate multiply) skips its term
  uint32_t hi = (uint32_t)(pair >> 32);
  if (__builtin_amdgcn_ballot_w64(hi != 0u)) {
    asm volatile("" : "+v"(hi));
    h += hi * 0x9E3779B9u;
  }
  return hash_avalanche32(h);
}
__device__ __forceinline__ void drop_keep4(uint64_t seed, uint64_t lin0, uint32_t thresh16, bool (&keep)[4]) {
  const uint32_t h0 = drop_hash_pair(seed, lin0 >> 1), h1 = drop_hash_pair(seed, (lin0 >> 1) + 1);
  keep[0] = (h0 & 0xffffu) >= thresh16; keep[1] = (h0 >> 16) >= thresh16;
  keep[2] = (h1 & 0xffffu) >= thresh16; keep[3] = (h1 >> 16) >= thresh16;
}

#define LOG2E_F 1.4426950408889634f
