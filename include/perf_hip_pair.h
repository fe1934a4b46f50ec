/* The pair table of libperf_hip: a fourth header of the same library, for two fields whose hash grids have the SAME geometry and are
 * evaluated at the same positions (the density and the colour field of a training step).  A pair table interleaves the two fields'
 * 16-bit tables entry by entry -- entry e is one 8-byte word {field A's packed 2 x 16-bit features, field B's} -- so that ONE gather per
 * corner serves both fields.  The entry points are exported from libperf_hip.so, use the descriptors, error codes and conventions of
 * perf_hip.h (perf_last_error() carries the reason of a refusal), and are versioned on their own: PERF_PAIR_ABI_VERSION /
 * perf_pair_version(), recorded in include/perf_hip_pair.abi.json (`python tools/abi_digest.py --pair [--write]`). */
#ifndef PERF_HIP_PAIR_H
#define PERF_HIP_PAIR_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_PAIR_ABI_VERSION 1

int perf_pair_version(void);            /* == PERF_PAIR_ABI_VERSION of the header the library was built from */

/* perf_pair_fill: pair[2 e + field] = the 32-bit word e of table16 (one entry's two 16-bit features), e < n_entries; the other field's
 * words are not touched.  pair: 8-byte aligned, 8 * n_entries bytes; field: 0 or 1; table16: 4-byte aligned.  One launch, no launch when
 * n_entries == 0. */
int perf_pair_fill(void* pair, int field, const void* table16, int64_t n_entries, void* stream);

/* perf_hashgrid_fwd_pair: the forward encode of perf_hashgrid_fwd for both fields of a pair table in ONE launch.
 *   pair:    the pair table: 8-byte entries at the level offsets (in entries) of the descriptor, 8-byte aligned
 *   feat16_a, feat16_b: [L, n, 2] 16-bit, level-major, each bit-identical to what perf_hashgrid_fwd writes from that field's own table
 *   n, n_dev: as in perf_hashgrid_fwd (n = capacity = level stride; only the first min(n, *n_dev) samples are encoded when n_dev != NULL)
 * Built: tcnn table layout, 1..16 levels, both interpolations, both 16-bit types.  Everything else is refused with PERF_E_INVALID before
 * anything is launched.  n == 0 launches nothing. */
int perf_hashgrid_fwd_pair(const perf_grid_desc* grid, const float* x01, const void* pair, void* feat16_a, void* feat16_b, int64_t n,
                           const int64_t* n_dev, int dtype, void* stream);

/* perf_adam_step_dev_pair: perf_adam_step_dev on the flat parameters [network (n_net) | table] of ONE field which, while it refreshes the
 * plain 16-bit working copy w16 as perf_adam_step_dev does, also stores every table entry's packed word into pair[2 e + field] -- the pair
 * table stays current without a pass of its own.  p, m, v, g, w16, the scalars and clear_flag: exactly perf_adam_step_dev's (same
 * arithmetic, element for element); a gated-off step (*gate_dev <= 0) leaves w16 AND the pair table untouched.
 *   w16, pair: required;  field: 0 or 1;  n_net: even, as is n - n_net;  n > 0. */
int perf_adam_step_dev_pair(float* p, float* m, float* v, float* g, void* w16, int64_t n, int dtype, const int32_t* step_dev,
                            const float* lr_dev, const int64_t* gate_dev, float beta1, float beta2, float eps, int zero_grad,
                            int32_t* clear_flag, void* pair, int field, int64_t n_net, void* stream);

/* perf_mlp_fwd_rows: perf_mlp_fwd whose sample i reads its features from row feat_index[i] of feat16 = [L, feat_stride, 2] (rows of a
 * larger feature array -- the kept samples of a batch among its marched samples -- instead of a compacted copy; perf_mlp_bwd's
 * feat_index / feat_stride).  Rows must lie in [0, feat_stride); rows at and beyond the live count are not read.  out, sel, n, n_dev, dtype:
 * perf_mlp_fwd's; results are bit-identical to perf_mlp_fwd on the materialised rows. */
int perf_mlp_fwd_rows(const perf_mlp_desc* mlp, const void* w16, const void* feat16, const int32_t* feat_index, int64_t feat_stride,
                      const uint8_t* sel, float* out, int64_t n, const int64_t* n_dev, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_PAIR_H */
