/* Extension of the libperf_hip C ABI: entry points added after include/perf_hip.h was frozen at PERF_ABI_VERSION 16.  They are
 * exported from the same libperf_hip.so, use the descriptors, error codes and conventions of perf_hip.h (perf_last_error() carries
 * the reason of a refusal), and are versioned on their own: PERF_EXT_ABI_VERSION / perf_ext_version(), recorded in
 * include/perf_hip_ext.abi.json (`python tools/abi_digest.py --ext [--write]`). */
#ifndef PERF_HIP_EXT_H
#define PERF_HIP_EXT_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_EXT_ABI_VERSION 1

int perf_ext_version(void);             /* == PERF_EXT_ABI_VERSION of the header the library was built from */

/* ---- backward of perf_field_grad_x with respect to the density field's parameters (training on surface normals) ----
 * perf_field_grad_x computes, per sample, sigma = a(y) sel and g = a'(y) (J^T p) / (hi - lo) sel.  Given the upstream gradients
 * dsigma [n] and dgrad [n, 3] (world units, as perf_field_grad_x writes g), this call forms d(sum dsigma sigma + dgrad . g) / d(params)
 * in ONE kernel: the forward is recomputed in registers, the network part is accumulated per wave on MFMA and reduced in a fixed
 * order (deterministic, independent of the live count's capacity), the table part is scattered with fp32 global atomics (its last
 * bits depend on the order the atomics retire in).  ReLU has no second derivative; positions get no gradient.
 *   grad: fp32 [n_net | 2 * table entries] (the flat layout of perf_field_bwd), OVERWRITTEN in full whatever the live count;
 *         all zeros when n == 0 or *n_dev == 0.
 *   x01, sel, table16, w16, inv_extent, n, n_dev, dtype: as perf_field_grad_x.
 *   dsigma, dgrad: either may be NULL (taken as zeros), not both.
 *   workspace: perf_field_grad_x_bwd_workspace_bytes(grid, mlp, n) bytes, 16-byte aligned.
 * The launch sequence is fixed (memset of the table part, kernel, reduction) and can be captured.
 * Built: tcnn table layout, Linear interpolation, one hidden layer, 1..16 levels, bf16 / fp16.  Everything else is refused with
 * PERF_E_INVALID before anything is launched. */
int64_t perf_field_grad_x_bwd_workspace_bytes(const perf_grid_desc* grid, const perf_mlp_desc* mlp, int64_t n);
int perf_field_grad_x_bwd(const perf_grid_desc* grid, const perf_mlp_desc* mlp, const float* x01, const uint8_t* sel,
                          const void* table16, const void* w16, const float* inv_extent, const float* dsigma, const float* dgrad,
                          float* grad, void* workspace, int64_t workspace_bytes, int64_t n, const int64_t* n_dev, int dtype,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_EXT_H */
