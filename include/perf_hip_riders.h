/* Step riders of libperf_hip: the front end of the NEXT training batch -- batch draw, lattice tables, the two marching passes -- as
 * workgroups that ride in launches of the CURRENT step's backward, which exist anyway and leave most of the chip idle.  None of that
 * work depends on the parameters being trained: it reads rays, the generator's counter and the occupancy bits.
 *
 * Three stages, each a launch boundary of the stream (no workgroup of a stage waits for another workgroup):
 *   A (perf_rider_draw)   perf_draw_train_batch + perf_occ_lattice_runs, one lane per ray; rides in the grid backward's tile-code launch
 *   B (perf_rider_count)  perf_occ_march_count, one wave per ray;                          rides in the grid backward's replica reduction
 *   C (perf_rider_write)  perf_exclusive_scan_i32 + perf_occ_march_write_points;           rides in the optimizer's launch
 * A rider runs the device function the stand-alone kernel runs: every output is bit-identical to the stand-alone entry points called
 * with the same arguments in the order A, B, C.  Rider workgroups come FIRST in their host launch: the lowest workgroup indices of the
 * one-dimensional hosts (A, C); in the two-dimensional replica reduction (one row of workgroups per level) the first columns of every row,
 * so that riders and the host's own workgroups alternate row by row in dispatch order (the last row's spare rider columns leave at once).
 * A host launch without riders (NULL job) is exactly the launch of the entry point it extends.  A host launch that does not take place (no tile-code
 * pre-pass, no replica reduction: grids that need neither) is replaced by a launch of the rider's own, at the same place of the stream.
 *
 * The entry points are exported from libperf_hip.so, use the descriptors, error codes and conventions of perf_hip.h (perf_last_error()
 * carries the reason of a refusal), and are versioned on their own: PERF_RIDERS_ABI_VERSION / perf_riders_version(), recorded in
 * include/perf_hip_riders.abi.json (`python tools/abi_digest.py --riders [--write]`). */
#ifndef PERF_HIP_RIDERS_H
#define PERF_HIP_RIDERS_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_RIDERS_ABI_VERSION 1

#define PERF_RIDER_THREADS 256            /* threads of a rider workgroup = of a workgroup of every host launch */
#define PERF_RIDER_DRAW_RAYS 256          /* rays per workgroup of stage A (a lane each) */
#define PERF_RIDER_MARCH_RAYS 4           /* rays per workgroup of stages B and C (a wave each) */
#define PERF_RIDER_MAX_RAYS 65536         /* stage C sums the counts before a workgroup's rays itself: quadratic beyond a training batch */

int perf_riders_version(void);            /* == PERF_RIDERS_ABI_VERSION of the header the library was built from */

/* Stage A.  Fields up to `bg`: the arguments of perf_draw_train_batch (same meaning, same NULL rules); t0_scale .. runs: those of
 * perf_occ_lattice_runs with t0 = `jitter` (required) and n_rays = n_local.  marched_live / marched_keep (both or neither): before
 * anything else *marched_keep = *marched_live -- the marched count of the batch being consumed, which stage C of the same step replaces. */
typedef struct perf_rider_draw {
    uint64_t seed;
    int64_t* counter_dev;
    int32_t* ticket;
    int64_t pool_lo, pool_hi, n_local, first_global;
    const float *o_all, *d_all, *color_all, *dist_all, *normal_all;
    float *o, *d, *color, *dist, *normal;
    int64_t* indices_out;
    float *jitter, *noise, *bg;
    float t0_scale, t0_base, step;
    int32_t max_steps;
    int32_t* runs;
    const int64_t* marched_live;
    int64_t* marched_keep;
} perf_rider_draw;

/* Stage B: the arguments of perf_occ_march_count for per-ray origins on the repeated lattice (t0 and runs required: `runs` is the
 * lattice_table argument, the rows perf_occ_lattice_runs wrote). */
typedef struct perf_rider_count {
    const float *rays_o, *rays_d, *t0;
    float t0_scale, t0_base;
    int64_t n_rays;
    const uint32_t *occ_bits, *occ_coarse;
    int32_t res;
    float aabb[6];
    float far_plane, step;
    int32_t max_steps;
    const int32_t* runs;
    uint64_t* masks;
    int32_t* counts;
} perf_rider_count;

/* Stage C: perf_exclusive_scan_i32(counts -> offsets, total) followed by perf_occ_march_write_points(..., rank_lo = 0) for per-ray origins
 * on the repeated lattice.  n_rays <= PERF_RIDER_MAX_RAYS.  offsets [n_rays] and total [1] are written as the scan writes them. */
typedef struct perf_rider_write {
    const float* t0;
    float t0_scale, t0_base;
    int64_t n_rays;
    float step;
    int32_t max_steps;
    const int32_t* runs;
    const uint64_t* masks;
    const int32_t* counts;
    int32_t* offsets;
    int64_t* total;
    int64_t capacity;
    int64_t* ray_indices;
    float *t_starts, *t_ends;
    int32_t* packed_info;
    const float *rays_o, *rays_d;
    float points_aabb[6];
    float* x01;
    uint8_t* sel;
} perf_rider_write;

int64_t perf_sizeof_rider_draw(void);
int64_t perf_sizeof_rider_count(void);
int64_t perf_sizeof_rider_write(void);

/* perf_field_bwd (book == NULL: fixed / redo as given) or perf_field_bwd_book (book != NULL: fixed = redo = 1 implied) whose grid backward
 * carries stage A in its tile-code launch and stage B in its replica reduction.  draw, count: either may be NULL.  tcnn table layout only.
 * Every other argument, every result of the backward and every launch but the two hosts: exactly the entry point's without riders. */
int perf_field_bwd_riders(const perf_grid_desc* grid, const perf_mlp_desc* mlp, const float* x01, const void* w16_net,
                          const void* feat16, const int32_t* feat_index, int64_t feat_stride, const uint8_t* sel, const float* dout,
                          float* grad, int32_t fixed, int32_t redo, int32_t* overflow_flag, int32_t* headroom_state,
                          void* workspace, int64_t workspace_bytes, int64_t n, const int64_t* n_dev, int dtype, const perf_step_book* book,
                          const perf_rider_draw* draw, const perf_rider_count* count, void* stream);

/* perf_adam_step_dev (pair == NULL) or perf_adam_step_dev_pair (pair != NULL) whose launch carries stage C.  Needs the four-elements-per-
 * thread launch (16-byte aligned arrays, n >= 1024); write may be NULL.  The riders run whether or not the step is gated off. */
int perf_adam_step_dev_riders(float* p, float* m, float* v, float* g, void* w16, int64_t n, int dtype, const int32_t* step_dev,
                              const float* lr_dev, const int64_t* gate_dev, float beta1, float beta2, float eps, int zero_grad,
                              int32_t* clear_flag, void* pair, int field, int64_t n_net, const perf_rider_write* write, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_RIDERS_H */
