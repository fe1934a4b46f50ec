/* The sphere distance field of libperf_hip: a third header of the same library, for the consumer of the tinycudann boundary that is
 * not a NeRF field -- SphereDistanceField (a Smoothstep hash grid over the unit sphere's directions, a 35 -> 64 -> 64 -> 1 fp32 MLP with
 * Softplus(beta = 100), and the gradient of its output with respect to the direction).  The entry points are exported from
 * libperf_hip.so, use the descriptors, error codes and conventions of perf_hip.h (perf_last_error() carries the reason of a refusal),
 * and are versioned on their own: PERF_SPHERE_ABI_VERSION / perf_sphere_version(), recorded in include/perf_hip_sphere.abi.json
 * (`python tools/abi_digest.py --sphere [--write]`). */
#ifndef PERF_HIP_SPHERE_H
#define PERF_HIP_SPHERE_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_SPHERE_ABI_VERSION 1

int perf_sphere_version(void);          /* == PERF_SPHERE_ABI_VERSION of the header the library was built from */

/* ---- the field.  All arithmetic is fp32; nothing is rounded to a 16-bit type anywhere.  Per direction u (a unit vector, data only):
 *     x  = 0.49 u + 0.49                     (no selector is applied)
 *     f  = enc(x)        2 L features: L levels x 2, Smoothstep s(t) = t^2 (3 - 2 t), fp32 table in tcnn's layout
 *     J  = df / dx       from s'(t) = 6 t (1 - t)
 *     z1 = W1 [u; f] + b1,  h1 = sp(z1);     z2 = W2 h1 + b2,  h2 = sp(z2);     raw = -(w3 . h2 + b3)
 *     g  = d raw / du = -(A^T d1 + 0.49 J^T B^T d1),   W1 = [A | B],  d2 = sp'(z2) . w3,  d1 = sp'(z1) . (W2^T d2)
 * sp is Softplus(beta = 100, threshold = 20): where 100 z > 20 it is z (sp' = 1, sp'' = 0), elsewhere log1p(exp(100 z)) / 100
 * (sp' = sigmoid(100 z) = s, sp'' = 100 s (1 - s)).
 *
 *   net_f32: ONE flat fp32 buffer, n_net = 64 (3 + 2 L) + 64 + 64 * 64 + 64 + 64 + 1 values, matrices row-major [out][in]:
 *              [ W1: 64 x (3 + 2 L), input = [u (3); f (2 L, level-major: level l at 3 + 2 l, 3 + 2 l + 1)]
 *              | b1: 64 | W2: 64 x 64 | b2: 64 | w3: 64 | b3: 1 ]
 *   table_f32: fp32 [table entries][2] (the grid descriptor's offsets and sizes);   dirs: fp32 [n, 3].
 *
 * Built: tcnn table layout, Smoothstep interpolation, fp32 table, 1..16 levels, width 64, two hidden layers.  Everything else is
 * refused with PERF_E_INVALID before anything is launched; the message names the reason.  The library allocates nothing.
 *
 * perf_sphere_field_fwd: ONE launch.  raw: fp32 [n]; grad: fp32 [n, 3] or NULL (no gradient is formed then: the cheaper branch; the raw
 * values are bit-identical either way).  n == 0 launches nothing. */
int perf_sphere_field_fwd(const perf_grid_desc* grid, const float* table_f32, const float* net_f32, const float* dirs, float* raw,
                          float* grad_or_null, int64_t n, void* stream);

/* perf_sphere_field_bwd: given the upstream gradients draw = dL/d raw [n] and dgrad = dL/d g [n, 3], forms dL / d(net, table) in ONE
 * kernel.  dgrad . g is the directional derivative of raw along dgrad, so one tangent per sample is carried beside the recomputed
 * forward (registers only: nothing per sample goes through memory except the inputs), and the adjoints of (raw, tangent) = (draw, 1)
 * are pulled back together; Softplus contributes its second derivative.  Directions get no gradient.
 *   grad_out: fp32 [n_net | 2 * table entries], OVERWRITTEN in full; all zeros when n == 0.
 *     - the network part is accumulated per wave on the fp32 MFMA, summed per workgroup and then over a FIXED number of workgroup
 *       partials in a fixed order: deterministic, and unchanged when samples with zero upstream are appended;
 *     - the table part is scattered with fp32 global atomics into the zero-filled buffer: its last bits depend on the order the
 *       atomics retire in.
 *   draw, dgrad: either may be NULL (taken as zeros), not both.
 *   workspace: perf_sphere_field_bwd_workspace_bytes(grid, n) bytes (-1: the descriptor is refused), 16-byte aligned, caller-owned.
 * The launch sequence is fixed (memset of the table part, kernel, reduction) and can be captured. */
int64_t perf_sphere_field_bwd_workspace_bytes(const perf_grid_desc* grid, int64_t n);
int perf_sphere_field_bwd(const perf_grid_desc* grid, const float* table_f32, const float* net_f32, const float* dirs,
                          const float* draw_or_null, const float* dgrad_or_null, float* grad_out, void* workspace,
                          int64_t workspace_bytes, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_SPHERE_H */
