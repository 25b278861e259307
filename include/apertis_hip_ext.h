/* libapertis_hip.so: entry points added after the 4.12 table.
 *
 * Why a second header: apertis_hip.h is the 4.12 ABI (the Python binding reads its table from it), and it is frozen - 123 entry
 * points, checked name by name against the library, with APERTIS_ABI_VERSION saying which table a build carries.  An entry point
 * that arrives without an ABI bump goes HERE: the same library exports it, every rule of apertis_hip.h holds for it (return
 * codes, dtype codes, `stream`, validation before any launch, no hidden synchronisation), and APERTIS_ABI_VERSION stays 4.12.
 * A caller that needs one of these names looks it up (dlsym, or the Python binding's EXT_SIGNATURES) and treats its absence as
 * "library older than this header".  The next ABI bump folds this file into apertis_hip.h.
 */
#ifndef APERTIS_HIP_EXT_H
#define APERTIS_HIP_EXT_H

#include "apertis_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * standard_mha under a SLIDING WINDOW, against the KV cache: the window forms of the device-length decode step and of the
 * multi-token chunk step.  `window` is the number of keys a query sees, its own included, a host integer by value; window < 1
 * is APERTIS_ERR_ARG whatever else is asked.  The cache keeps every row: the window bounds what is READ.
 *
 * apertis_attention_decode_window_at: the argument list of apertis_attention_decode_at with `window` after `len`.  The kernel
 * reads Lk = min(*len + 1, cap) (0 for *len < 0) as there, and begin = max(Lk - window, 0); the query attends keys [begin, Lk)
 * with key_valid[b, j] != 0.  Piece s of the caller's fixed `splits` is keys [begin + s*(Lk-begin)/splits, begin +
 * (s+1)*(Lk-begin)/splits); an empty piece reads nothing and leaves (m = -inf, l = 0, o = 0).  Grid and workspace depend on
 * nothing read from the device.  K rows, V rows and key_valid columns before `begin` (and at or past Lk) are never read.
 * For the same Lk, window and split count the output has the bits of apertis_attention_decode on k_cache, v_cache and key_valid
 * offset by `begin` rows / columns with Lk' = Lk - begin: the same kernel body, the same partition, each wave's walk relative
 * to its piece.  Every other argument, check and error code as apertis_attention_decode_at.
 *
 * apertis_attention_chunk_window: the argument list of apertis_attention_chunk with `window` after `n`.  Chunk row i sits at key
 * position p = n + i and attends keys j with p - window < j <= p and key_valid[b, j] != 0.  The forward's window form: one
 * unsigned compare of p - j against `window`, every wave (16 rows) starts at the 32-key tile that holds the first key its first
 * row sees, tiles in front of it are never touched, and the `splits` runs cut the wave's tiles [first, last], not [0, last].
 * K and V rows before the first key a wave's first row sees are never read.  With splits = 1 row i has the bits
 * apertis_attention_window_fwd gives row n + i of the whole sequence of n + Lq positions (tiles are aligned at multiples of 32
 * from key 0 in both, and a tile in which no key counts for a row leaves the row's numbers as they were); with window >= n + Lq
 * the bits of apertis_attention_chunk at the same split count.
 *   splits        : 0 takes apertis_attention_chunk_splits(B, H, Lq, Lk = min(n + Lq, window + Lq), D) - no wave walks more
 *                   keys than that; forced: 1..APERTIS_ATTN_DECODE_MAX_SPLITS as there
 *   workspace     : apertis_attention_chunk_workspace_bytes, as there
 *   Every other argument, check and error code as apertis_attention_chunk. */
int apertis_attention_decode_window_at(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs,
                                       const void *v_cache, int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *len,
                                       int64_t window, const int64_t *key_valid, int64_t kv_rs, void *out, int64_t out_rs,
                                       float *workspace, int64_t B, int64_t H, int64_t D, int64_t splits, int dtype, void *stream);
int apertis_attention_chunk_window(const void *q, int64_t q_rs, const void *k_cache, int64_t k_rs, int64_t k_bs,
                                   const void *v_cache, int64_t v_rs, int64_t v_bs, int64_t cap, const int64_t *key_valid,
                                   int64_t kv_rs, void *out, int64_t out_rs, float *workspace, int64_t B, int64_t Lq, int64_t n,
                                   int64_t window, int64_t H, int64_t D, int64_t splits, int dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* APERTIS_HIP_EXT_H */
