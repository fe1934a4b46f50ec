/* Surface nets on the occupied BRICKS of a lattice, on the device: a seventh header of libperf_hip.so, versioned on its own --
 * PERF_BRICKMESH_ABI_VERSION / perf_brickmesh_version(), recorded in include/perf_hip_brickmesh.abi.json
 * (`python tools/abi_digest.py --brickmesh [--write]`).  Error codes and conventions are those of perf_hip.h: raw device pointers, counts
 * and a stream; an integer return code, the reason of a refusal in perf_last_error(); a caller-owned workspace sized by
 * perf_brickmesh_workspace_bytes; nothing is allocated; everything that is refused is refused before anything is launched.  No case
 * tables and no atomics: the order of vertices and faces comes from a scan, so two runs give identical bits.
 *
 * The statement.
 *   Lattice.  A virtual lattice of (nx, ny, nz) cells, each a multiple of PERF_BRICKMESH_EDGE and at most PERF_BRICKMESH_MAX_DIM;
 *     B = (Bx, By, Bz) = (nx, ny, nz) / 8 bricks.  Brick (bx, by, bz), linear index (bx By + by) Bz + bz, stores the 8 x 8 x 8 corners
 *     8b .. 8b+7 per axis, z fastest: values fp32 [n_bricks, 8, 8, 8].  No corner is stored twice (no apron); a corner whose index
 *     equals n on some axis is never stored.
 *   Brick set.  ids: int32 [n_bricks], strictly ascending linear brick indices; a brick's SLOT is its position in ids.  table: int32
 *     [Bx, By, Bz], each brick's slot or -1.  At most PERF_BRICKMESH_MAX_BRICKS bricks (2^30 cells: vertex indices are int32).
 *   Virtual field.  fp32 [nx+1, ny+1, nz+1]: `fill` everywhere except at the stored corners; fill is finite and < thr.
 *   Mesh.  The mesh of the virtual field exactly as include/perf_hip_mesh.h states it -- the inside rule (value >= thr, a NaN outside),
 *     the crossings (NaN t -> 1/2), the vertex formula carried in double and rounded once, the quad rule, orientation and split --
 *     in another order: a vertex's index is the rank of its cell in (slot, local cell index (i 8 + j) 8 + k) order; faces are
 *     ordered by ((slot of the brick that holds corner p) 512 + local corner index of p) 3 + axis, an edge's two triangles adjacent.
 *   Closure.  The dense statement makes every cell around an inside corner active, so the bricks of all eight cells around a stored
 *     corner >= thr must be in the set.  A quad of the virtual field that needs the vertex of a cell of a missing brick is a VIOLATION:
 *     the count pass counts them, both passes skip them (and the cells of missing bricks have no vertex).  No kernel indexes with a
 *     slot of -1: neighbours are looked up through the table, addresses are clamped to valid ones.  With no violation the result is
 *     the dense unit's mesh of the virtual field up to the order, vertices to the bit.
 *
 * Which bricks are live (perf_brickmesh_select).  x(i, n) = fl32(fl32(i) * fl32(1 / n)): the position of lattice corner i in [0, 1] as
 *   a device tensor divided by the host scalar n evaluates (a multiplication by the scalar's fp32 reciprocal; the correctly rounded
 *   i / n where n is a power of two, and never another occupancy cell at a brick's ends for the lattices tested).  c(i, n) =
 *   int(clip(x(i, n), 0.0005, 0.9995) * R) in fp32, R the occupancy resolution: the occupancy cell of the corner, by the rule the
 *   occupancy grid was built with.  Brick b is live iff any cell of `binaries` in the box [c(8bx, nx), c(min(8bx+8, nx), nx)] x (the
 *   same in y) x (the same in z) is set.  That is a superset of the bricks with a corner in a set cell and closes the set for any
 *   field that is below thr in every unset cell.
 *
 * Corners (perf_brickmesh_corners).  For the stored corner (i, j, k): x01 = x(i, nx), x(j, ny), x(k, nz);
 *   interior = 0 < x01 < 1 on all axes; sel = interior and binaries[c(i, nx), c(j, ny), c(k, nz)].
 *
 * Protocol: select -> the caller reads the live count and allocates -> list -> (corners, the field's values) -> count -> the caller
 * reads the three totals (the one host synchronisation of a meshing) and allocates -> write.
 *
 * Workspace, in 8-byte words.  L(n) = n_1 + n_2 + ... with n_1 = ceil(n / 256), n_{k+1} = ceil(n_k / 256), down to the level of one
 * word.  select: S = G + L(G) with G = ceil(Bx By Bz / 256) (the groups' live counts and their scan).  count / write: with
 * W = 8 n_bricks slabs (one x-layer of a brick: 8 x 8 cells, one 64-bit mask), C = 3 W + 2 L(W) + 4 for n_bricks > 0 (the slabs'
 * active masks, their packed ranks -- quads before << 32 | vertices before --, their violation counts, the two scans' levels) and
 * 4 otherwise (the totals, padded).  perf_brickmesh_workspace_bytes = 8 * (max(S, C) rounded up to an even number): 0.375 bytes per
 * cell of a live brick; the values take 4 bytes per stored corner. */
#ifndef PERF_HIP_BRICKMESH_H
#define PERF_HIP_BRICKMESH_H

#include "perf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PERF_BRICKMESH_ABI_VERSION 1
#define PERF_BRICKMESH_EDGE 8
#define PERF_BRICKMESH_MAX_DIM 4096
#define PERF_BRICKMESH_MAX_BRICKS 2097152 /* 2^21 */

int perf_brickmesh_version(void);       /* == PERF_BRICKMESH_ABI_VERSION of the header the library was built from */

/* Bytes of the one workspace that serves select (n_bricks is ignored by it: pass 0) and count / write of n_bricks live bricks (a
 * multiple of 16); -1 with a reason: a dimension below 8, above PERF_BRICKMESH_MAX_DIM or no multiple of 8, n_bricks outside
 * 0 .. min(Bx By Bz, PERF_BRICKMESH_MAX_BRICKS). */
int64_t perf_brickmesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int32_t n_bricks);

/* perf_brickmesh_select: binaries uint8 [R, R, R] (nonzero = set), R = occ_res in 1 .. 4096 -> table int32 [Bx, By, Bz] (slot or -1,
 * slots ascending with the linear brick index) and n_live_dev [1] int64 ON THE DEVICE.  The count may exceed
 * PERF_BRICKMESH_MAX_BRICKS: the later calls refuse such an n_bricks.  workspace: 16-byte aligned, >= workspace_bytes(nx, ny, nz, 0). */
int perf_brickmesh_select(const uint8_t* binaries, int32_t occ_res, int32_t nx, int32_t ny, int32_t nz, int32_t* table, int64_t* n_live_dev,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* perf_brickmesh_list: ids [n_bricks] from the table: ids[table[b]] = b for every table[b] in 0 .. n_bricks-1 (plain stores, each slot
 * written once; slots the table does not hold are left as they were).  ids may be NULL when n_bricks is 0. */
int perf_brickmesh_list(const int32_t* table, int32_t nx, int32_t ny, int32_t nz, int32_t* ids, int32_t n_bricks, void* stream);

/* perf_brickmesh_corners: for the slots first .. first + m - 1 of ids [n_bricks]: x01 fp32 [m * 512, 3], sel uint8 [m * 512] and, unless
 * NULL, interior uint8 [m * 512], by the rules above; binaries, occ_res as in select.  m == 0 is a no-op. */
int perf_brickmesh_corners(const int32_t* ids, int32_t n_bricks, int32_t first, int32_t m, int32_t nx, int32_t ny, int32_t nz,
                           const uint8_t* binaries, int32_t occ_res, float* x01, uint8_t* sel, uint8_t* interior, void* stream);

/* perf_brickmesh_count: classifies the cells of the live bricks, leaves the slabs' masks and ranks in the workspace and
 * counts_dev [3] int64 = (vertices, triangles, violations) on the device.  values, ids may be NULL when n_bricks is 0.  thr and fill
 * finite, fill < thr.  workspace: 16-byte aligned, >= workspace_bytes(nx, ny, nz, n_bricks). */
int perf_brickmesh_count(const float* values, const int32_t* ids, const int32_t* table, int32_t n_bricks, int32_t nx, int32_t ny, int32_t nz,
                         float thr, float fill, void* workspace, int64_t workspace_bytes, int64_t* counts_dev, void* stream);

/* perf_brickmesh_write: vertices [V, 3] fp32, faces [F, 3] int32 and, unless NULL, cells [V] int64 -- the linear cell (i ny + j) nz + k of
 * each vertex in the virtual lattice -- of the SAME values, set, thr, fill and workspace perf_brickmesh_count was given (the stream's
 * order puts it after the count).  lo, hi: HOST pointers to the box's three lower and upper bounds, finite, hi > lo on every axis.
 * vertex_capacity / face_capacity: rows the arrays hold (cells: vertex_capacity); capacities below the counted totals are refused: the
 * call reads the totals back from the workspace after the stream has drained, so it is not for stream capture.  vertices / faces may be
 * NULL when their capacity is 0. */
int perf_brickmesh_write(const float* values, const int32_t* ids, const int32_t* table, int32_t n_bricks, int32_t nx, int32_t ny, int32_t nz,
                         float thr, float fill, const float* lo, const float* hi, const void* workspace, int64_t workspace_bytes,
                         float* vertices, int64_t vertex_capacity, int32_t* faces, int64_t face_capacity, int64_t* cells, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERF_HIP_BRICKMESH_H */
