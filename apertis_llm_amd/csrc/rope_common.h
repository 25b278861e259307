// The interleaved-pair rotation of standard_mha's RoPE (reference core.py:258-293), shared by attention.hip (rope_qk_k, whole
// sequences, forward and backward) and attention_decode.hip (rope_kv_append_k, one token into the KV cache): one statement of
// the table lookup and of the pair arithmetic, so both give the same bits.  Anonymous namespace: a copy per translation unit.
#pragma once
#include "common.h"

namespace {

// cos / sin of pair j at position ps of the fp32 tables [max_pos, half].  A negative position reads row ps + max_pos (torch
// indexing wraps it); the host checked the range, and a position outside it is never read: its pair comes out NaN.
__device__ __forceinline__ void rope_cos_sin(const float *cs, const float *sn, int64_t ps, int64_t max_pos, int64_t half,
                                             int64_t j, float &c, float &s) {
  if (ps < 0) ps += max_pos;
  c = NAN;
  s = NAN;
  if (ps >= 0 && ps < max_pos) {
    c = cs[ps * half + j];
    s = sn[ps * half + j];
  }
}

// stock order: (a*cos) - (b*sin), (a*sin) + (b*cos), each product rounded (-ffp-contract=off); BWD: the transposed rotation
template <bool BWD>
__device__ __forceinline__ void rope_rotate_pair(float x0, float x1, float c, float s, float &y0, float &y1) {
  const float p0 = x0 * c, p1 = x1 * s, p2 = x0 * s, p3 = x1 * c;
  if constexpr (!BWD) {
    y0 = p0 - p1;
    y1 = p2 + p3;
  } else {
    y0 = p0 + p1;
    y1 = p3 - p2;
  }
}

}  // namespace
