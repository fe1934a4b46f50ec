/* The alignment step of PeRF's joint geometry predictor (modules/geo_predictors/pano_joint_predictor.py:204-297) around the sphere
 * distance field of perf_hip_sphere.h: a fifth header of libperf_hip.so, versioned on its own -- PERF_JOINT_ABI_VERSION /
 * perf_joint_version(), recorded in include/perf_hip_joint.abi.json (`python tools/abi_digest.py --joint [--write]`).  Error codes
 * and conventions are those of perf_hip.h: raw device pointers, counts and a stream; an integer return code, the reason of a refusal in
 * perf_last_error(); caller-owned workspaces sized by a *_workspace_bytes call; nothing is allocated; everything that is refused is
 * refused before anything is launched.
 *
 * One iteration aligns P perspective views (B samples each, N = P B) on one field.  Storage is fp32 everywhere; the arithmetic of a
 * sample is carried in double between the fp32 loads and the fp32 stores (15,360 threads are bound by latency, not by the vector rate).
 * Bilinear sampling is torch's grid_sample(mode='bilinear', padding_mode='border', align_corners=False): for a coordinate c in [-1, 1]
 * on an axis of S texels the position is clamp(((c + 1) S - 1) / 2, 0, S - 1), the corners are floor and floor + 1, and a corner
 * outside the map (floor + 1 == S, its weight is 0) is neither read nor written. */
#ifndef PERF_HIP_JOINT_H
#define PERF_HIP_JOINT_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_JOINT_ABI_VERSION 1
#define PERF_JOINT_RECORD 12 /* floats of a sample's record: [sd | db | sn (3) | nb (3) | pr | pm | 0 | 0] */
#define PERF_JOINT_LOSSES 8  /* floats of the loss block:   [L_d | L_n | L_reg | L_ref | TV_d | TV_n | total | 0] */

int perf_joint_version(void);           /* == PERF_JOINT_ABI_VERSION of the header the library was built from */

/* perf_joint_sample: ONE launch, one thread per sample.
 *   sup: [P, 7, R, R] (direction 3, predicted distance 1, predicted normal 3);  bias_d: [P, 1, R, R];  bias_n: [P, 3, Rn, Rn];
 *   ref: [2, H, W] (panorama distance, mask);  coords: [P, B, 2] in [-1, 1], (x, y) as grid_sample takes them.
 *   u_given_or_null: NULL: u = the sampled direction channels, normalised, is formed here and written to u [N, 3].  Not NULL: fp32
 *        [N, 3], the directions the caller formed from the same maps and coordinates; they are taken as they are (the look-up below
 *        and the record use them) and u is not written (it may be NULL).  The field downstream is steep in u (its finest levels have
 *        resolution 2048): a caller that compares or alternates this path with a torch formulation hands both the same bits.
 *   rec: [N, PERF_JOINT_RECORD]: sd = the sampled distance channel, db = the sampled distance bias, sn = the sampled normal channels,
 *        nb = the sampled normal bias, (pr, pm) = ref sampled at u:  beta = asin(u_z), alpha = atan2(u_y, u_x) (the reference divides
 *        both arguments by cos beta > 0, which changes nothing off the poles; at a pole the reference gives NaN), image coordinate
 *        (row, col) = (-beta / pi + 1/2, -alpha / 2 pi + 1/2), sample coordinate (col, row) * 2 - 1, border padding and NO wrap at
 *        the seam, as the reference.
 * P, B, R, Rn >= 1, H, W >= 1, P * B <= 2^30, B <= 2^20 (a view's part of d/dscale is summed by one thread in its order).  P * B == 0 is
 * refused (an alignment step has samples). */
int perf_joint_sample(const float* sup, const float* bias_d, const float* bias_n, const float* ref, const float* coords,
                      const float* u_given_or_null, int32_t P, int64_t B, int32_t R, int32_t Rn, int32_t H, int32_t W, float* u, float* rec,
                      void* stream);

/* perf_joint_loss: the losses of the step and every gradient the head owns.  TWO launches: one thread per sample, then one workgroup
 * that sums the workgroups' partials.
 *   rec, coords, u: as above;  scale: [P];  d: [N] and g: [N, 3]: the field's distance and its gradient at u;  o: [N, 3] the draws of
 *   the tangent frame (b = unit(u x o), a = unit(b x u)).
 *   rd = sd softplus(scale_p) + db,  rn = unit(sn + nb),  v_t = unit((g . t) u + t) for t in (a, b),  h_beta = smooth-L1:
 *     L_d   = mean h_0.5(rd - d)                 L_n   = mean over 2 N of h_0.5(v_t . rn)
 *     L_reg = (mean_p softplus(scale_p) - 1)^2   L_ref = mean over N of h_0.01(pr - d) [pm < 1/2]
 *     total = w_ref L_ref + L_d + w_reg L_reg + w_n L_n + TV_d + w_ntv TV_n   (tv_or_null: two device floats (TV_d, TV_n) as
 *             perf_joint_tv leaves them; NULL: both zero, the 'global' phase)
 *   losses: [PERF_JOINT_LOSSES];  dd: [N] = d total / d d;  dg: [N, 3] = d total / d g -- the upstreams of perf_sphere_field_bwd's
 *   caller;  dscale: [P] = d total / d scale, the L_reg term included.  These are DETERMINISTIC: per-sample values, per-workgroup
 *   partials in double summed in a fixed order; two runs give identical bits.
 *   gbias_d: [P, 1, R, R] and gbias_n: [P, 3, Rn, Rn], both or neither: d total / d db and d total / d nb are scattered ON TOP of what
 *   the buffers hold (perf_joint_tv has written the TV part) with the bilinear weights, by fp32 global atomics: the last bits of
 *   the two maps depend on the order the atomics retire in.  NULL (the 'global' phase): no scatter, the maps are not touched.
 *   workspace: perf_joint_loss_workspace_bytes(P, B) bytes (-1: refused), 16-byte aligned, caller-owned. */
int64_t perf_joint_loss_workspace_bytes(int32_t P, int64_t B);
int perf_joint_loss(const float* rec, const float* coords, const float* scale, const float* u, const float* d, const float* g,
                    const float* o, int32_t P, int64_t B, int32_t R, int32_t Rn, float w_ref, float w_reg, float w_n, float w_ntv,
                    const float* tv_or_null, float* losses, float* dd, float* dg, float* dscale, float* gbias_d_or_null,
                    float* gbias_n_or_null, void* workspace, int64_t workspace_bytes, void* stream);

/* perf_joint_tv: the total variation of a map [n, C, H, W] with smooth-L1(beta = 0.01),
 *     TV = mean h(m[:, :, 1:, :] - m[:, :, :-1, :]) + mean h(m[:, :, :, 1:] - m[:, :, :, :-1]),
 * and weight * d TV / d m, WRITTEN to grad_out [n, C, H, W] in full in gather form (an entry's gradient is a function of its four
 * neighbours): no atomics, no zero-fill, deterministic.  value_out: one float, the unweighted TV, summed over a fixed number of
 * partials in a fixed order.  One streaming pass over the map and one over its gradient; a second, one-workgroup launch sums the
 * partials.  H, W >= 2 (a mean over no differences is refused), n, C >= 1.
 *   workspace: perf_joint_tv_workspace_bytes(n, C, H, W) bytes (-1: refused), 16-byte aligned, caller-owned. */
int64_t perf_joint_tv_workspace_bytes(int64_t n, int32_t C, int32_t H, int32_t W);
int perf_joint_tv(const float* map, int64_t n, int32_t C, int32_t H, int32_t W, float weight, float* grad_out, float* value_out,
                  void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_JOINT_H */
