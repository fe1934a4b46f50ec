"""The next training batch's front end -- batch draw, lattice tables, counting pass, offsets, write pass -- produced while the current
step's backward runs: as workgroups that ride in launches the backward makes anyway (include/perf_hip_riders.h; stage A in the grid
backward's tile-code launch, B in its replica reduction, C in the optimizer's launch).  None of that work reads the parameters being
trained.

A MarchSet is ONE set of the front end's arrays.  The step that consumes it hands its riders the same arrays: every stage overwrites
an array only after the step's last reader of it -- the draw's rows after the loss head, masks and counts after the write pass that
expanded them, the marched samples after the backward -- so that a captured step (fixed addresses) consumes on replay i what replay i - 1
left.  The first batch of a set comes from the stand-alone kernels (`fill`); both ways write the same bits (tests/test_gpu_step_riders.py)."""
import math

import torch

from . import _lib, ops


class MarchSet:
    def __init__(self, key, pool_args, seed, counter, n_rays, estimator, sampling, capacity, points_aabb, stage_c=True):
        """pool_args: (pool_lo, pool_hi, first_global, o_all, d_all, color_all, dist_all, normal_all, want_bg) of ops.draw_train_batch;
        sampling: (near, far, step, max_steps, lattice).  stage_c False: only stages A and B ride; the offsets and the write pass of
        the batch they produced are stand-alone launches at the head of the step that consumes it (marched())."""
        self.key = key
        self.pool_args, self.seed, self.counter, self.n_rays = pool_args, seed, counter, n_rays
        self.estimator, self.sampling, self.capacity, self.points_aabb = estimator, sampling, capacity, points_aabb
        self.structs = None
        self.stage_c, self.stale = stage_c, False
        self.keep = torch.zeros(1, dtype=torch.int64, device=counter.device)      # the CONSUMED batch's marched count (stage A saves it)

    def fill(self):
        """The set's first batch, by the stand-alone kernels (advances the draw counter like every draw)."""
        lo, hi, first, o_all, d_all, c_all, t_all, n_all, want_bg = self.pool_args
        near, far, step, max_steps, lattice = self.sampling
        est = self.estimator
        self.draw = ops.draw_train_batch(self.seed, self.counter, lo, hi, self.n_rays, first, o_all, d_all, c_all, t_all, n_all, want_bg=want_bg)
        u = self.draw['jitter']
        self.runs = ops.lattice_runs((u, step, near), step, max_steps)
        self.t0 = (u, step, near, self.runs)
        o, d = self.draw['o'], self.draw['d']
        self.bits, self.coarse = est.occ_bits(), est.occ_coarse()
        self.masks, self.counts = ops.occ_march_count(o, d, self.t0, self.bits, est._res, est._aabb_host, far, step, max_steps, self.coarse, lattice=lattice)
        self._write()
        self.structs, self.stale = None, False
        return self

    def _write(self):
        near, far, step, max_steps, lattice = self.sampling
        self.offsets, self.total = ops.exclusive_scan_i32(self.counts)
        self.samples = ops.occ_march_write(self.t0, self.masks, self.counts, self.offsets, self.capacity, step, max_steps, self.draw['o'], self.draw['d'],
                                           self.points_aabb, lattice=lattice)

    def marched(self, force=False):
        """What ops.occ_march(..., capacity, points_aabb) returns for the set's rays.  Without stage C: scan and write pass run here when
        the riders left only masks and counts (force: always -- a captured step must hold them whatever the set's state at capture)."""
        if not self.stage_c and (self.stale or force):
            self._write()
        self.stale = False
        ri, ts, te, packed, x01, sel = self.samples
        return (ri, ts, te, packed, self.total, x01, sel)

    def riders(self):
        """-> (draw, count, write): the argument blocks of the three stages that refill this set in place (built once: the addresses stay)."""
        if self.structs is None:
            lo, hi, first, o_all, d_all, c_all, t_all, n_all, _ = self.pool_args
            near, far, step, max_steps, lattice = self.sampling
            est = self.estimator
            o, d = self.draw['o'], self.draw['d']
            ri, ts, te, packed, x01, sel = self.samples
            self.structs = (
                ops.rider_draw(self.seed, self.counter, lo, hi, self.n_rays, first, o_all, d_all, c_all, t_all, n_all, self.draw, step, near, step, max_steps,
                               self.runs, marched_live=self.total if self.stage_c else None, marched_keep=self.keep if self.stage_c else None),
                ops.rider_count(o, d, self.t0, self.bits, est._res, est._aabb_host, far, step, max_steps, self.coarse, self.masks, self.counts),
                ops.rider_write(self.t0, self.masks, self.counts, self.offsets, self.total, self.capacity, step, max_steps, o, d, self.points_aabb,
                                ri, ts, te, packed, x01, sel) if self.stage_c else None)
        return self.structs


def max_steps_of(renderer, estimator):
    """The lattice intervals per ray OccGridEstimator.sampling_ex marches with this renderer's constants."""
    if renderer.max_steps is not None:
        return int(renderer.max_steps)
    span = min(float(renderer.far_plane) - float(renderer.near_plane), estimator._diag)
    return int(math.ceil(span / renderer.render_step_size)) + 1


def supported(renderer, estimator, n_rays):
    """The sampler configurations the riders are built for: sync-free, one phase, a visibility pass, per-ray origins on the repeated
    lattice inside the box (no anchored origins)."""
    return (renderer.sample_capacity is not None and renderer.head_samples is None and renderer.early_stop_eps > 0
            and (renderer.lattice or _lib.DEFAULT_LATTICE) == 'repeated'
            and float(renderer.far_plane) - float(renderer.near_plane) <= estimator._diag
            and 0 < n_rays <= _lib.RIDER_MAX_RAYS)
