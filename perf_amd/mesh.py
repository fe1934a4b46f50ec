"""A triangle mesh of the trained density: the field is evaluated on a dense lattice over the scene's aabb and meshed on the device by
naive surface nets (include/perf_hip_mesh.h: no case tables, no atomics, bit-identical from run to run).  Not the reference's: PeRF
writes a point cloud of its input panorama (modules/dataset/dataset.py:110-114) and leaves a trimesh export commented out
(pano_geo_refiner.py:155-157).

    mesh = scene.extract_mesh(resolution=256, colors=True, normals=True)
    write_ply('room.ply', mesh)
"""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, ops


class Mesh(NamedTuple):
    vertices: torch.Tensor                       # [V, 3] fp32, world units
    faces: torch.Tensor                          # [F, 3] int32; normals point from high density to low
    colors: Optional[torch.Tensor] = None        # [V, 3] fp32 in [0, 1]
    normals: Optional[torch.Tensor] = None       # [V, 3] fp32, unit or zero


def surface_nets(field, thr, lo, hi) -> Mesh:
    """field: CUDA fp32 [nx+1, ny+1, nz+1] corner values (z fastest); a corner is inside iff field >= thr; lo, hi: the box the lattice
    spans, three values each.  Two kernels around ONE host read of the two counts (count -> allocate -> write)."""
    field = field.contiguous()
    counts, ws = ops.mesh_count(field, thr)
    n_vertices, n_faces = (int(v) for v in counts.tolist())          # the one host synchronisation of an extraction
    vertices, faces = ops.mesh_write(field, thr, lo, hi, ws, n_vertices, n_faces)
    return Mesh(vertices, faces)


@torch.no_grad()
def density_lattice(scene, resolution, use_occupancy=True, chunk=1 << 22):
    """sigma at the (resolution + 1)^3 corners of the scene's aabb -> fp32 [res+1, res+1, res+1].  Corner i sits at x01 = i / res; the
    border corners fail the field's strict 0 < x01 < 1 selector and are exactly 0, which closes every surface at the box.
    use_occupancy: sigma is zeroed where the estimator's `binaries` cell of the point is empty (the cell of a point by the rule the
    grid was built with, sup_info.py:318: int(clip(x01, 0.0005, 0.9995) * res_occ) per axis) -- the field is untrained outside the
    shell the occupancy marks.  chunk: corners per density_at call."""
    res = int(resolution)
    if res < 1 or res ** 3 > _lib.MESH_MAX_CELLS:
        raise _lib.PerfError(f'density_lattice: resolution {resolution} is outside 1 .. 1024')
    nerf, est = scene.nerf, scene.estimator
    dev = nerf.aabb.device
    n1 = res + 1
    total = n1 ** 3
    out = torch.empty(total, dtype=torch.float32, device=dev)
    occ = est.binaries.reshape(-1) if use_occupancy else None
    occ_res = int(est._res)
    for start in range(0, total, int(chunk)):
        idx = torch.arange(start, min(start + int(chunk), total), dtype=torch.int64, device=dev)
        ijk = torch.stack([idx // (n1 * n1), (idx // n1) % n1, idx % n1], dim=1)
        x01 = (ijk.float() / float(res)).contiguous()
        sel = ((x01 > 0) & (x01 < 1)).all(dim=1).to(torch.uint8)
        sigma = nerf.density_at(x01, sel).float()
        if occ is not None:
            cell = (x01.clamp(0.0005, 0.9995) * occ_res).long()
            sigma = torch.where(occ[(cell[:, 0] * occ_res + cell[:, 1]) * occ_res + cell[:, 2]], sigma, torch.zeros_like(sigma))
        out[start:start + idx.numel()] = sigma
    return out.view(n1, n1, n1)


@torch.no_grad()
def vertex_colors(scene, vertices, chunk=1 << 22):
    """query_rgb at world positions [V, 3] -> fp32 [V, 3]."""
    if not len(vertices):
        return vertices.new_zeros(0, 3)
    return torch.cat([scene.nerf.query_rgb(v).float() for v in vertices.split(chunk)])


@torch.no_grad()
def vertex_normals(scene, vertices, chunk=1 << 22):
    """query_normal at world positions [V, 3] -> fp32 [V, 3], unit or zero."""
    if not len(vertices):
        return vertices.new_zeros(0, 3)
    return torch.cat([scene.nerf.query_normal(v)[1].float() for v in vertices.split(chunk)])


@torch.no_grad()
def extract_mesh(scene, resolution=256, threshold=None, use_occupancy=True, colors=False, normals=False) -> Mesh:
    """The iso-surface sigma = threshold of the scene's density over its aabb.  threshold None: ln 2 / renderer.render_step_size, the
    density at which one render step is half opaque.  colors: query_rgb at the vertices; normals: query_normal at the vertices
    (-grad sigma, unit or zero: the side the density falls towards, as the faces' orientation)."""
    if threshold is None:
        threshold = math.log(2.0) / float(scene.renderer.render_step_size)
    aabb = scene.nerf._aabb_host
    field = density_lattice(scene, resolution, use_occupancy)
    vertices, faces, _, _ = surface_nets(field, threshold, aabb[:3], aabb[3:])
    rgb = nrm = None
    if colors:
        rgb = vertex_colors(scene, vertices)
    if normals:
        nrm = vertex_normals(scene, vertices)
    return Mesh(vertices, faces, rgb, nrm)


# ---- only the occupied bricks of the lattice (include/perf_hip_brickmesh.h) ---------------------------------------------------------------
def _brick_shape(n):
    shape = (int(n),) * 3 if isinstance(n, (int, np.integer)) else tuple(int(v) for v in n)
    if len(shape) != 3 or any(v < _lib.BRICKMESH_EDGE or v % _lib.BRICKMESH_EDGE or v > _lib.BRICKMESH_MAX_DIM for v in shape):
        raise _lib.PerfError(f'a brick lattice has three dimensions, each a multiple of {_lib.BRICKMESH_EDGE} in {_lib.BRICKMESH_EDGE} .. {_lib.BRICKMESH_MAX_DIM}: got {n!r}')
    return shape


def select_bricks(binaries, n):
    """The 8 x 8 x 8-corner bricks of a lattice of n (or (nx, ny, nz)) cells that touch a set cell of the occupancy grid `binaries`
    (bool [R, R, R]) by the box rule of include/perf_hip_brickmesh.h -> (ids int32 [M] ascending linear brick indices, table int32
    [Bx, By, Bz]: each brick's position in ids, or -1).  One host read: the live count, to allocate ids."""
    shape = _brick_shape(n)
    table, n_live = ops.brickmesh_select(binaries, shape)
    m = int(n_live.item())
    if m > _lib.BRICKMESH_MAX_BRICKS:
        raise _lib.PerfError(f'select_bricks: {m} live bricks of a lattice of {shape} cells are more than 2^21: lower the resolution')
    return ops.brickmesh_list(table, m), table


@torch.no_grad()
def density_bricks(scene, n, chunk_bricks=8192):
    """sigma at the stored corners of the live bricks of the scene's lattice of n^3 cells -> (ids, table, values fp32 [M, 8, 8, 8]): at
    every stored corner the value density_lattice(scene, n) has there, to the bit; every corner that is not stored is 0 there.  The
    coordinates of a chunk of bricks are generated on the device.  The occupancy stays a select of its own behind the field (as in
    density_lattice): the field multiplies by its selector, which would turn an overflowed sigma into a NaN instead of 0."""
    shape = _brick_shape(n)
    nerf, est = scene.nerf, scene.estimator
    ids, table = select_bricks(est.binaries, shape)
    m = int(ids.numel())
    values = torch.empty(m, 8, 8, 8, dtype=torch.float32, device=ids.device)
    flat = values.view(m, 512)
    step = max(int(chunk_bricks), 1)
    for first in range(0, m, step):
        count = min(step, m - first)
        x01, sel, interior = ops.brickmesh_corners(ids, first, count, shape, est.binaries)
        sigma = nerf.density_at(x01, interior).float()
        flat[first:first + count] = torch.where(sel.bool(), sigma, torch.zeros_like(sigma)).view(count, 512)
    return ids, table, values


def surface_nets_bricks(values, ids, table, shape, thr, fill, lo, hi):
    """The mesh of the virtual field that is `fill` (< thr) everywhere but at the stored corners `values` [M, 8, 8, 8] of the bricks
    (ids, table) of a lattice of `shape` cells -> (Mesh, cells int64 [V]: each vertex's linear cell (i ny + j) nz + k).  Vertices are
    ordered by (brick slot, cell within the brick).  Raises when the set is not closed: a stored corner >= thr whose eight cells are not
    all in live bricks."""
    shape = _brick_shape(shape)
    values = values.contiguous()
    counts, ws = ops.brickmesh_count(values, ids, table, shape, thr, fill)
    n_vertices, n_faces, violations = (int(v) for v in counts.tolist())          # the one host synchronisation of a meshing
    if violations:
        raise _lib.PerfError(f'surface_nets_bricks: {violations} quads need the vertex of a cell in a brick that is not in the set: the bricks of all eight cells around a '
                             'stored corner >= thr must be live')
    vertices, faces, cells = ops.brickmesh_write(values, ids, table, shape, thr, fill, lo, hi, ws, n_vertices, n_faces)
    return Mesh(vertices, faces), cells


@torch.no_grad()
def extract_mesh_sparse(scene, resolution=1024, threshold=None, colors=False, normals=False) -> Mesh:
    """extract_mesh with the occupancy, evaluated and meshed only on the 8^3 bricks of the lattice that touch the occupancy shell: the
    same vertices (to the bit) and faces in another order, at resolutions up to 4096 (a multiple of 8) as long as at most 2^21 bricks
    are live.  threshold None: ln 2 / renderer.render_step_size; it must be positive (the lattice outside the bricks is 0)."""
    if threshold is None:
        threshold = math.log(2.0) / float(scene.renderer.render_step_size)
    aabb = scene.nerf._aabb_host
    shape = _brick_shape(resolution)
    ids, table, values = density_bricks(scene, shape)
    mesh, _ = surface_nets_bricks(values, ids, table, shape, threshold, 0.0, aabb[:3], aabb[3:])
    rgb = nrm = None
    if colors:
        rgb = vertex_colors(scene, mesh.vertices)
    if normals:
        nrm = vertex_normals(scene, mesh.vertices)
    return Mesh(mesh.vertices, mesh.faces, rgb, nrm)


# ---- the pieces of a mesh: connected components, selection, compaction (include/perf_hip_meshcc.h) ---------------------------------------
class Components(NamedTuple):
    vertex_component: torch.Tensor               # [V] int32: the id of each vertex's component, ids ordered by smallest vertex index
    faces: torch.Tensor                          # [C] int64: faces per component
    vertices: torch.Tensor                       # [C] int32: vertices per component
    signed_volume: Optional[torch.Tensor] = None     # [C] float64: > 0 for a closed surface with outward normals; None without positions


def connected_components(mesh_or_faces, n_vertices=None, vertices=None) -> Components:
    """The pieces of a mesh that share no vertex index, labelled on the device.  mesh_or_faces: a Mesh, or faces int32 [F, 3] with
    n_vertices (and vertices fp32 [V, 3] for the signed volumes).  One host read: the component count with the flag of a face index
    outside [0, V), which is refused."""
    if isinstance(mesh_or_faces, Mesh):
        faces, vertices = mesh_or_faces.faces, mesh_or_faces.vertices
        n_vertices = int(vertices.shape[0])
    else:
        faces = mesh_or_faces
        if n_vertices is None:
            if vertices is None:
                raise _lib.PerfError('connected_components: faces alone do not say how many vertices there are: pass n_vertices or vertices')
            n_vertices = int(vertices.shape[0])
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise _lib.PerfError('connected_components: faces must be a CUDA tensor (there is no CPU path)')
    faces = faces.contiguous()
    if vertices is not None:
        vertices = vertices.contiguous()
    vertex_component, counts, _ = ops.meshcc_label(faces, n_vertices)
    n_components, bad = (int(v) for v in counts.tolist())          # the one host synchronisation of a labelling
    if bad >= 0:
        raise _lib.PerfError(f'connected_components: face {bad} = {faces[bad].tolist()} has an index outside [0, {int(n_vertices)})')
    per_faces, per_vertices, volume = ops.meshcc_stats(faces, vertex_component, n_components, vertices)
    return Components(vertex_component, per_faces, per_vertices, volume)


def select_components(components, min_faces=0, keep_largest=None, orientation=None) -> torch.Tensor:
    """bool [C]: component c is kept iff faces[c] >= min_faces, and keep_largest is None or the rank of c by (more faces first, then
    lower id) is below keep_largest, and orientation is None, or 'inward' and signed_volume[c] < 0, or 'outward' and > 0."""
    if not components.faces.is_cuda:
        raise _lib.PerfError('select_components: the components must be CUDA tensors (there is no CPU path)')
    if orientation not in (None, 'inward', 'outward'):
        raise _lib.PerfError(f"select_components: orientation is None, 'inward' or 'outward', got {orientation!r}")
    faces = components.faces
    keep = faces >= int(min_faces)
    if keep_largest is not None:
        if int(keep_largest) < 0:
            raise _lib.PerfError(f'select_components: keep_largest {keep_largest} is negative')
        order = torch.sort(faces, descending=True, stable=True).indices          # (stable: ties stay in ascending id)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), dtype=order.dtype, device=order.device)
        keep &= rank < int(keep_largest)
    if orientation is not None:
        if components.signed_volume is None:
            raise _lib.PerfError('select_components: an orientation needs signed volumes: label the components with the vertices')
        keep &= (components.signed_volume < 0) if orientation == 'inward' else (components.signed_volume > 0)
    return keep


def filter_mesh(mesh, components, keep):
    """The mesh of the components keep [C] selects -> (Mesh, kept_vertex_index int32 [V']): kept vertices and faces in their old
    relative order, faces re-indexed, colors and normals gathered.  One host read: the two kept counts."""
    if not mesh.faces.is_cuda or not mesh.vertices.is_cuda:
        raise _lib.PerfError('filter_mesh: the mesh must hold CUDA tensors (there is no CPU path)')
    if keep.numel() != components.faces.numel():
        raise _lib.PerfError(f'filter_mesh: keep holds {keep.numel()} entries, there are {components.faces.numel()} components')
    faces, vertices = mesh.faces.contiguous(), mesh.vertices.contiguous()
    counts, ws = ops.meshcc_filter_count(faces, components.vertex_component, keep)
    n_vertices, n_faces = (int(v) for v in counts.tolist())          # the one host synchronisation of a filtering
    new_vertices, new_faces, index = ops.meshcc_filter_write(faces, components.vertex_component, keep, ws, n_vertices, n_faces, vertices)
    gather = index.long()
    colors = mesh.colors[gather] if mesh.colors is not None else None
    normals = mesh.normals[gather] if mesh.normals is not None else None
    return Mesh(new_vertices, new_faces, colors, normals), index


def clean_mesh(mesh, min_faces=0, keep_largest=None, orientation=None) -> Mesh:
    """mesh without its floaters / without one of its two skins: the components select_components keeps.  A thresholded density is a
    thin shell, so its iso-surface is the skin the cameras saw (orientation='inward' for a room seen from inside: normals point into
    the volume the surface encloses, the signed volume is negative) AND the shell's back."""
    components = connected_components(mesh)
    keep = select_components(components, min_faces=min_faces, keep_largest=keep_largest, orientation=orientation)
    return filter_mesh(mesh, components, keep)[0]


# ---- the faces no registered panorama saw (include/perf_hip_meshvis.h) -----------------------------------------------------------------
class Visibility(NamedTuple):
    visible: torch.Tensor                        # [V] int64: bit k set iff view k saw the vertex (dist < stored + tol)
    free: torch.Tensor                           # [V] int64: bit k set iff the vertex lies in view k's observed free space (dist < stored - free_tol)
    n_views: int


class _Views(NamedTuple):
    table: torch.Tensor                          # [K, 16] int32: the device array of perf_meshvis_view
    centres: torch.Tensor                        # [K, 3] fp32
    sizes: list                                  # K (height, width)
    maps: list                                   # the masked distance maps the table points into


def _views(who, views) -> _Views:
    """views: a SupInfoPool, or a list of dicts with 'pose' [4, 4] or [3, 4], 'distance_map' [H, W, 1] or [H, W] and optionally 'mask' of
    the map's shape (what SupInfoPool.sup_infos holds).  The map a view is tested against is distance_map * mask, as the reprojection
    tests of perf_amd/visibility.py form it."""
    if isinstance(views, _Views):
        return views
    infos = views.sup_infos if hasattr(views, 'sup_infos') else views
    poses, maps = [], []
    for info in infos:
        dmap = info['distance_map']
        if not torch.is_tensor(dmap) or not dmap.is_cuda:
            raise _lib.PerfError(f'{who}: a view\'s distance_map must be a CUDA tensor (there is no CPU path)')
        if info.get('mask') is not None:
            dmap = dmap * info['mask'].reshape(dmap.shape).float()
        if dmap.dim() == 3 and dmap.shape[2] == 1:
            dmap = dmap[..., 0]
        if dmap.dim() != 2:
            raise _lib.PerfError(f'{who}: a view\'s distance_map is [H, W, 1] or [H, W], got {tuple(info["distance_map"].shape)}')
        maps.append(dmap.float().contiguous())
        poses.append(info['pose'])
    return _Views(*ops.meshvis_views(poses, maps))


def _tolerances(tol, free_tol):
    tol = float(tol)
    return tol, tol if free_tol is None else float(free_tol)


def vertex_visibility(vertices, views, tol=1 / 256, free_tol=None) -> Visibility:
    """Which registered panoramas saw each vertex, all of them in ONE launch: bit k of `visible` is the depth test of
    NeRFScene.get_pano_visibility_mask against view k (the distance of the vertex from the view's centre < the distance the view stored
    along that direction + tol), bit k of `free` the stricter dist < stored - free_tol (free_tol None: tol): the vertex floats in front
    of what the view stored.  vertices: CUDA fp32 [V, 3]; at most 64 views."""
    if not torch.is_tensor(vertices) or not vertices.is_cuda:
        raise _lib.PerfError('vertex_visibility: vertices must be a CUDA tensor (there is no CPU path)')
    tol, free_tol = _tolerances(tol, free_tol)
    v = _views('vertex_visibility', views)
    visible, free = ops.meshvis_vertex_bits(vertices.contiguous(), v.table, v.sizes, tol, free_tol)
    return Visibility(visible, free, len(v.sizes))


def _check_mesh(who, mesh):
    if not torch.is_tensor(mesh.faces) or not torch.is_tensor(mesh.vertices) or not mesh.faces.is_cuda or not mesh.vertices.is_cuda:
        raise _lib.PerfError(f'{who}: the mesh must hold CUDA tensors (there is no CPU path)')


def _raise_bad_face(who, faces, bad, n_vertices):
    raise _lib.PerfError(f'{who}: face {bad} = {faces[bad].tolist()} has an index outside [0, {int(n_vertices)})')


def _face_keep(who, mesh, visibility, v, facing, min_views, carve, flag=None):
    if int(min_views) < 1:
        raise _lib.PerfError(f'{who}: min_views {min_views} is below 1')
    if visibility.n_views != len(v.sizes):
        raise _lib.PerfError(f'{who}: the visibility holds bits of {visibility.n_views} views, {len(v.sizes)} views are given')
    return ops.meshvis_face_keep(mesh.faces.contiguous(), mesh.vertices.contiguous(), visibility.visible, visibility.free, v.centres, facing, min_views, carve, flag)


def visible_faces(mesh, visibility, views, facing=True, min_views=1, carve=False) -> torch.Tensor:
    """uint8 [F]: a face is kept iff at least min_views views saw all three of its vertices and (facing) the face points at the view --
    surface-nets normals point from the dense side to the empty side, so the skin a camera saw points at it and the back of the density
    shell does not -- and (carve) none of its vertices lies in a view's observed free space.  One host read: the flag of a face index
    outside [0, V), which is refused."""
    _check_mesh('visible_faces', mesh)
    keep, flag = _face_keep('visible_faces', mesh, visibility, _views('visible_faces', views), facing, min_views, carve)
    bad = int(flag.item())
    if bad >= 0:
        _raise_bad_face('visible_faces', mesh.faces, bad, mesh.vertices.shape[0])
    return keep


def _filter_faces(mesh, face_keep, counts, who):
    faces, vertices = mesh.faces.contiguous(), mesh.vertices.contiguous()
    _, ws = ops.meshvis_filter_count(faces, vertices.shape[0], face_keep, counts=counts[:2])
    n_vertices, n_faces, bad = (int(c) for c in counts.tolist())          # the one host synchronisation
    if bad >= 0:
        _raise_bad_face(who, faces, bad, vertices.shape[0])
    new_vertices, new_faces, index = ops.meshvis_filter_write(faces, vertices.shape[0], face_keep, ws, n_vertices, n_faces, vertices)
    gather = index.long()
    colors = mesh.colors[gather] if mesh.colors is not None else None
    normals = mesh.normals[gather] if mesh.normals is not None else None
    return Mesh(new_vertices, new_faces, colors, normals), index


def filter_faces(mesh, face_keep):
    """The mesh of the faces face_keep (bool or uint8 [F]) selects -> (Mesh, kept_vertex_index int32 [V']): a vertex is kept iff a kept face
    names it; kept vertices and faces keep their relative order, faces are re-indexed, colors and normals gathered.  A face with an index
    outside [0, V) is dropped.  One host read: the two kept counts."""
    _check_mesh('filter_faces', mesh)
    if not torch.is_tensor(face_keep) or not face_keep.is_cuda:
        raise _lib.PerfError('filter_faces: face_keep must be a CUDA tensor (there is no CPU path)')
    counts = torch.full((3,), -1, dtype=torch.int64, device=mesh.faces.device)
    return _filter_faces(mesh, face_keep, counts, 'filter_faces')


def cull_unseen(mesh, views, tol=1 / 256, free_tol=None, facing=True, min_views=1, carve=False) -> Mesh:
    """mesh without the faces no registered panorama saw: vertex_visibility -> visible_faces -> filter_faces with ONE host
    synchronisation.  It separates the skin the cameras saw from the back of the density shell where the two are ONE connected component
    (clean_mesh(orientation='inward') keeps nothing of it).  There is no occlusion test against the mesh itself, no colours are taken from
    the panoramas (color_from_panoramas does that, on what the cull leaves), and more than 64 views are refused."""
    _check_mesh('cull_unseen', mesh)
    v = _views('cull_unseen', views)
    visibility = vertex_visibility(mesh.vertices, v, tol, free_tol)
    counts = torch.empty(3, dtype=torch.int64, device=mesh.faces.device)
    keep, _ = _face_keep('cull_unseen', mesh, visibility, v, facing, min_views, carve, counts[2:])
    return _filter_faces(mesh, keep, counts, 'cull_unseen')[0]


# ---- a mesh of a size the caller chooses: vertex clustering (include/perf_hip_meshsimp.h) -------------------------------------------------
class Clusters(NamedTuple):
    vertex_cluster: torch.Tensor                 # [V] int32: the id of each vertex's cluster, ids ordered by smallest member index
    n_clusters: int
    vertices: torch.Tensor                       # [C, 3] fp32: the clusters' vertices under the placement
    representative: torch.Tensor                 # [C] int32: the member nearest the cluster's mean; it carries per-vertex attributes


def _cluster_grid(who, vertices, cell, box):
    """(lo [3], h, n [3]) of include/perf_hip_meshsimp.h: lo and h as the fp32 values the library takes, n = max(1, ceil((hi - lo) / h))
    per axis in double.  box None: the bounds of the finite coordinates, read back from the device."""
    h = float(np.float32(cell))
    if not math.isfinite(h) or h <= 0:
        raise _lib.PerfError(f'{who}: the cell edge {cell!r} is not positive or not finite')
    if box is None:
        bounds = ops.meshsimp_bounds(vertices).tolist()          # the host read-back of the six bounds
        if not all(math.isfinite(b) for b in bounds):            # (no finite coordinate along an axis: the clustering names the vertex)
            bounds = [0.0] * 6
        lo, hi = bounds[:3], bounds[3:]
    else:
        lo, hi = ([float(v) for v in side] for side in box)
        if len(lo) != 3 or len(hi) != 3 or not all(math.isfinite(v) for v in lo + hi) or any(b < a for a, b in zip(lo, hi)):
            raise _lib.PerfError(f'{who}: box is (lo, hi), three finite values each with lo <= hi, got {box!r}')
    lo = [float(np.float32(v)) for v in lo]
    n = [max(1, math.ceil((b - a) / h)) for a, b in zip(lo, hi)]
    if max(n) > _lib.MESHSIMP_MAX_CELLS:
        raise _lib.PerfError(f'{who}: a cell of {h} makes {n} cells per axis of the box, more than 2^21: choose a larger cell')
    return lo, h, n


def _check_placement(who, placement, dedupe='oriented'):
    if placement != 'quadric' and placement not in _lib.MESHSIMP_PLACEMENT:          # ('quadric' is a second pass over the faces, not a placement of the clustering unit)
        raise _lib.PerfError(f"{who}: placement is 'mean', 'member' or 'quadric', got {placement!r}")
    if dedupe not in _lib.MESHSIMP_DEDUPE:
        raise _lib.PerfError(f"{who}: dedupe is 'oriented', 'unoriented' or None, got {dedupe!r}")


def _raise_bad_vertex(who, vertices, bad):
    raise _lib.PerfError(f'{who}: vertex {bad} = {vertices[bad].tolist()} has a coordinate that is not finite')


def cluster_vertices(vertices, cell, box=None, placement='mean') -> Clusters:
    """The vertices fp32 [V, 3] that share a cell of edge `cell` of the grid over box = (lo, hi) (None: the vertices' own bounds, one more
    host read) become one cluster: its vertex is the mean of its members (exact integer sums of 2^-32 fixed-point fractions) or, under
    placement='member', the member nearest that mean, bit for bit.  One host read: the cluster count with the flag of a vertex that is
    not finite, which is refused.  placement='quadric' reads the faces, which this call does not have: quadric_placement takes the
    clusters and the mesh."""
    if placement == 'quadric':
        raise _lib.PerfError("cluster_vertices: placement 'quadric' needs the faces: cluster with 'mean', then call quadric_placement(mesh, clusters, cell, box)")
    if not torch.is_tensor(vertices) or not vertices.is_cuda:
        raise _lib.PerfError('cluster_vertices: vertices must be a CUDA tensor (there is no CPU path)')
    _check_placement('cluster_vertices', placement)
    vertices = vertices.contiguous()
    lo, h, n = _cluster_grid('cluster_vertices', vertices, cell, box)
    vertex_cluster, counts, _ = ops.meshsimp_cluster(vertices, lo, h, n)
    n_clusters, bad = (int(v) for v in counts.tolist())          # the one host synchronisation of a clustering
    if bad >= 0:
        _raise_bad_vertex('cluster_vertices', vertices, bad)
    placed, representative = ops.meshsimp_place(vertices, lo, h, n, vertex_cluster, n_clusters, placement)
    return Clusters(vertex_cluster, n_clusters, placed, representative)


def cluster_faces(faces, clusters, dedupe='oriented'):
    """faces int32 [F, 3] through the clusters -> (faces int32 [F, 3] of cluster ids, keep uint8 [F]): a face is dropped when two of its
    cluster ids are equal, and, of the faces whose triples are equal up to rotation (dedupe='oriented') or as sets ('unoriented': a double
    skin thinner than a cell becomes one), all but the one with the smallest index; None keeps every face that is not degenerate.  One
    host read: the flag of a face index outside [0, V), which is refused."""
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise _lib.PerfError('cluster_faces: faces must be a CUDA tensor (there is no CPU path)')
    _check_placement('cluster_faces', 'mean', dedupe)
    faces = faces.contiguous()
    remapped, keep, flag = ops.meshsimp_faces(faces, clusters.vertex_cluster, dedupe)
    bad = int(flag.item())          # the one host synchronisation
    if bad >= 0:
        _raise_bad_face('cluster_faces', faces, bad, clusters.vertex_cluster.numel())
    return remapped, keep


def simplify_mesh(mesh, cell, box=None, placement='mean', dedupe='oriented'):
    """mesh with one vertex per occupied cell of edge `cell` -> (Mesh, kept_vertex_index int32 [V']): cluster_vertices -> cluster_faces ->
    the compaction of filter_faces, with ONE host read of (clusters, the two flags, kept vertices, kept faces) beside the compaction's own.
    Clusters no kept face names are dropped; kept_vertex_index holds the surviving clusters' representatives, through which colors and
    normals are gathered.  Clustering can pinch a surface: there is no manifold repair.
    placement: 'mean' (the members' mean), 'member' (the member nearest the mean) or 'quadric' (include/perf_hip_meshquadric.h: the
    point of the cell that minimises the summed squared distances to the planes of the members' faces, regularised towards the mean, so
    edges and corners of the surface stay where they are; int64 fixed-point sums, bit-identical from run to run).  'quadric' runs the
    'mean' simplification, then two more launches on the same stream: faces, kept_vertex_index, colors and normals are those of 'mean',
    and there is no further host read (the flag of the faces the 2^60 rule skipped stays on the device: quadric_placement returns it)."""
    _check_mesh('simplify_mesh', mesh)
    _check_placement('simplify_mesh', placement, dedupe)
    vertices, faces = mesh.vertices.contiguous(), mesh.faces.contiguous()
    n_vertices, n_faces = int(vertices.shape[0]), int(faces.shape[0])
    lo, h, n = _cluster_grid('simplify_mesh', vertices, cell, box)
    counts = torch.empty(5, dtype=torch.int64, device=faces.device)
    vertex_cluster, _, ws = ops.meshsimp_cluster(vertices, lo, h, n, n_faces=n_faces, counts=counts[:2])
    remapped, keep, _ = ops.meshsimp_faces(faces, vertex_cluster, dedupe, ws=ws, flag=counts[2:3])
    _, filter_ws = ops.meshvis_filter_count(remapped, n_vertices, keep, counts=counts[3:])
    n_clusters, bad_vertex, bad_face, kept_vertices, kept_faces = (int(c) for c in counts.tolist())          # the one host synchronisation
    if bad_vertex >= 0:
        _raise_bad_vertex('simplify_mesh', vertices, bad_vertex)
    if bad_face >= 0:
        _raise_bad_face('simplify_mesh', faces, bad_face, n_vertices)
    placed, representative = ops.meshsimp_place(vertices, lo, h, n, vertex_cluster, n_clusters, 'mean' if placement == 'quadric' else placement)
    if placement == 'quadric':
        acc, _ = ops.meshquadric_sums(vertices, faces, lo, h, n, vertex_cluster, n_clusters)
        placed = ops.meshquadric_place(vertices, lo, h, n, placed, representative, acc)
    _, new_faces, kept_cluster = ops.meshvis_filter_write(remapped, n_vertices, keep, filter_ws, kept_vertices, kept_faces)
    kept_cluster = kept_cluster.long()
    index = representative[kept_cluster]
    gather = index.long()
    colors = mesh.colors[gather] if mesh.colors is not None else None
    normals = mesh.normals[gather] if mesh.normals is not None else None
    return Mesh(placed[kept_cluster], new_faces, colors, normals), index


class QuadricPlacement(NamedTuple):
    vertices: torch.Tensor                       # [C, 3] fp32: the clusters' vertices by quadric error
    skipped: torch.Tensor                        # [1] int64 ON THE DEVICE: the smallest index of a face the 2^60 rule skipped, or -1


def quadric_placement(mesh, clusters, cell, box=None) -> QuadricPlacement:
    """The vertices of `clusters` (cluster_vertices of mesh.vertices with the SAME cell and box, under either placement) by quadric
    error (include/perf_hip_meshquadric.h), for callers that cluster apart: the 'mean' placement as the anchor, the fixed-point sums
    over mesh.faces, the solve.  No host read: `skipped` stays on the device, and a face with an index outside [0, V) is not followed
    (cluster_faces is what refuses it)."""
    _check_mesh('quadric_placement', mesh)
    vertices, faces = mesh.vertices.contiguous(), mesh.faces.contiguous()
    if not isinstance(clusters, Clusters) or clusters.vertex_cluster.numel() != vertices.shape[0]:
        raise _lib.PerfError('quadric_placement: clusters must be the Clusters cluster_vertices made of mesh.vertices')
    lo, h, n = _cluster_grid('quadric_placement', vertices, cell, box)
    anchor, representative = ops.meshsimp_place(vertices, lo, h, n, clusters.vertex_cluster, clusters.n_clusters, 'mean')
    acc, flags = ops.meshquadric_sums(vertices, faces, lo, h, n, clusters.vertex_cluster, clusters.n_clusters)
    return QuadricPlacement(ops.meshquadric_place(vertices, lo, h, n, anchor, representative, acc), flags[1:])


# ---- the panoramas' colours on the mesh; vertex normals from the faces (include/perf_hip_meshcolor.h) ------------------------------------
class PanoramaColors(NamedTuple):
    colors: torch.Tensor                         # [V, 3] fp32: the blended (or the best view's) colour; the fallback where no view passed
    weight: torch.Tensor                         # [V] fp32: the sum of the passing views' weights (best: the best view's), 0 where none passed
    used: torch.Tensor                           # [V] int64: bit k set iff view k's colour went into the vertex
    best_view: torch.Tensor                      # [V] int8: select='best': the view the colour is from; -1 where none passed and under 'blend'


class _ColorViews(NamedTuple):
    views: _Views                                # the geometric side, as the cull takes it
    pointers: torch.Tensor                       # [K] int64: the device array of the colour maps' pointers
    maps: list                                   # the colour maps it points into


def _color_views(who, views) -> _ColorViews:
    """views: what _views takes, each with a 'color_map' [H, W, 3] of its distance map's height and width (what SupInfoPool.sup_infos
    holds)."""
    if isinstance(views, _ColorViews):
        return views
    if isinstance(views, _Views):
        raise _lib.PerfError(f'{who}: the views carry no colour maps: pass the pool or the list of views itself')
    infos = list(views.sup_infos if hasattr(views, 'sup_infos') else views)
    v = _views(who, infos)
    maps = []
    for k, info in enumerate(infos):
        if info.get('color_map') is None:
            raise _lib.PerfError(f'{who}: view {k} has no color_map')
        maps.append(info['color_map'])
    return _ColorViews(v, *ops.meshcolor_maps(maps, v.sizes))          # (which checks them)


def _normal_scale(box):
    """scale_log2 of include/perf_hip_meshcolor.h for a box (lo, hi): 40 - ceil(log2(D^2)), D^2 the squared diagonal; 0 for no extent."""
    d2 = sum((float(b) - float(a)) ** 2 for a, b in zip(*box))
    if not math.isfinite(d2) or d2 <= 0.0:
        return 0
    return max(-200, min(200, 40 - math.ceil(math.log2(d2))))


def face_normals(mesh, box=None) -> torch.Tensor:
    """Geometric vertex normals fp32 [V, 3]: the faces' area-weighted normals summed at their vertices in fixed point (int64 atomics: no
    floating-point atomics, so the result does not depend on the faces' order and is bit-identical from run to run), then normalised;
    exactly 0 at a vertex no face names or whose faces cancel.  They point where the faces do: from the dense side to the empty side.
    box = (lo, hi) bounds the vertices and sets the fixed point's scale (None: the vertices' own bounds, one more host read).  One host
    read: the flag of a face index outside [0, V), which is refused."""
    _check_mesh('face_normals', mesh)
    vertices, faces = mesh.vertices.contiguous(), mesh.faces.contiguous()
    if box is None:
        bounds = ops.meshsimp_bounds(vertices).tolist()          # the host read-back of the six bounds
        box = (bounds[:3], bounds[3:])
    elif len(box) != 2 or len(box[0]) != 3 or len(box[1]) != 3:
        raise _lib.PerfError(f'face_normals: box is (lo, hi), three values each, got {box!r}')
    acc, flag = ops.meshcolor_normal_sums(vertices, faces, _normal_scale(box))
    bad = int(flag.item())          # the one host synchronisation
    if bad >= 0:
        _raise_bad_face('face_normals', faces, bad, vertices.shape[0])
    return ops.meshcolor_normals(acc)


def panorama_colors(vertices, views, normals=None, tol=1 / 256, facing=True, power=2, select='blend', fallback=None, fill=(0.5, 0.5, 0.5)) -> PanoramaColors:
    """The registered panoramas' colours at vertices fp32 [V, 3], all views in ONE launch.  View k's colour map is sampled where the
    cull's look-up reads its distance map (the same bilinear taps), and counts iff the view saw the vertex (the depth test of
    vertex_visibility: dist < stored + tol) and, with facing, the normal points at the view's centre.  It is weighted by
    cos^power / dist^2 (facing) or 1 / dist^2: a panorama pixel's footprint on the surface grows as dist^2 / cos.  select='blend': the
    weighted mean; 'best': the colour of the view with the largest weight.  Where no view passes: the fallback row [V, 3] if given, else
    fill.  No occlusion test against the mesh itself, no texture atlas here (colours are per vertex: bake_panorama_texture bakes one), no exposure matching between views, no
    wrap at the seam; more than 64 views are refused.  No host read."""
    if not torch.is_tensor(vertices) or not vertices.is_cuda:
        raise _lib.PerfError('panorama_colors: vertices must be a CUDA tensor (there is no CPU path)')
    if select not in _lib.MESHCOLOR_SELECT:
        raise _lib.PerfError(f"panorama_colors: select is 'blend' or 'best', got {select!r}")
    if facing and normals is None:
        raise _lib.PerfError('panorama_colors: facing weights the views by the normals: pass normals, or facing=False')
    if facing and not 1 <= int(power) <= _lib.MESHCOLOR_MAX_POWER:
        raise _lib.PerfError(f'panorama_colors: power {power} is outside 1 .. {_lib.MESHCOLOR_MAX_POWER}')
    cv = _color_views('panorama_colors', views)
    return PanoramaColors(*ops.meshcolor_blend(vertices.contiguous(), normals.contiguous() if facing else None, cv.views.table, cv.views.sizes, cv.pointers, float(tol),
                                               facing, power, select, fallback.contiguous() if fallback is not None else None, fill))


def color_from_panoramas(mesh, views, normals='faces', **kw) -> Mesh:
    """mesh with the panoramas' colours at its vertices (panorama_colors' keywords, and box for face_normals).  normals='faces': the
    views are weighted by the geometric normals of face_normals; 'mesh': by mesh.normals, which must be there; with facing=False neither
    is needed.  mesh.colors, when present, is the fallback of the vertices no view passed for.  The result keeps mesh.normals."""
    _check_mesh('color_from_panoramas', mesh)
    if normals not in ('faces', 'mesh'):
        raise _lib.PerfError(f"color_from_panoramas: normals is 'faces' or 'mesh', got {normals!r}")
    box = kw.pop('box', None)
    weigh_by = None
    if kw.get('facing', True):
        if normals == 'mesh':
            if mesh.normals is None:
                raise _lib.PerfError("color_from_panoramas: normals='mesh' needs mesh.normals: extract them, or use normals='faces'")
            weigh_by = mesh.normals
        else:
            weigh_by = face_normals(mesh, box)
    kw.setdefault('fallback', mesh.colors)
    return Mesh(mesh.vertices, mesh.faces, panorama_colors(mesh.vertices, views, weigh_by, **kw).colors, mesh.normals)


# ---- a texture atlas: as many colour samples as the panoramas hold on a mesh of any size (include/perf_hip_meshtex.h) -------------------
class Atlas(NamedTuple):
    size: int                                    # S: the atlas is S x S texels
    tile: int                                    # T: a tile of T x T texels holds two faces
    uv: torch.Tensor                             # [F, 3, 2] fp32: (u, v) of each face's corners a, b, c; v grows with the row index
    image: torch.Tensor                          # [S, S, 3] fp32: texel (column i, row j) at image[j, i]
    coverage: torch.Tensor                       # [S, S] uint8: 0 no face, 1 inside its face's triangle, 2 gutter
    weight: torch.Tensor                         # [S, S] fp32: the blend's weight, 0 where no view passed
    used: torch.Tensor                           # [S, S] int64: bit k set iff view k's colour went into the texel


def _atlas_capacity(size, tile):
    return 2 * (size // tile) ** 2


def atlas_layout(n_faces, size=None, tile=None):
    """(size, tile) of an atlas that holds n_faces faces, two per tile (capacity 2 (size // tile)^2).  Given size: the largest tile that
    fits; given tile (neither: 8): the smallest power-of-two size in 64 .. 16384; given both: checked.  What does not fit is refused."""
    f = int(n_faces)
    if f < 0:
        raise _lib.PerfError(f'atlas_layout: a negative number of faces ({f})')
    lo, hi, least = _lib.MESHTEX_MIN_SIZE, _lib.MESHTEX_MAX_SIZE, _lib.MESHTEX_MIN_TILE
    if size is not None:
        size = int(size)
        if not lo <= size <= hi:
            raise _lib.PerfError(f'atlas_layout: an atlas size of {size} is outside {lo} .. {hi}')
    if tile is not None:
        tile = int(tile)
        if tile < least or tile > (hi if size is None else size):
            raise _lib.PerfError(f'atlas_layout: a tile of {tile} texels is outside {least} .. {hi if size is None else size}')
    if size is not None and tile is None:
        per_row = max(1, math.isqrt((f + 1) // 2))          # the smallest n with 2 n^2 >= f
        per_row += 2 * per_row * per_row < f
        tile = size // per_row
        if tile < least:
            raise _lib.PerfError(f'atlas_layout: {f} faces do not fit an atlas of {size}: it holds {_atlas_capacity(size, least)} at tiles of {least} texels')
    elif size is None:
        tile = 8 if tile is None else tile
        size = lo
        while size < hi and (size < tile or _atlas_capacity(size, tile) < f):
            size *= 2
    if size < tile or _atlas_capacity(size, tile) < f:
        raise _lib.PerfError(f'atlas_layout: {f} faces are more than the {_atlas_capacity(size, tile) if size >= tile else 0} an atlas of {size} with tiles of {tile} holds')
    return size, tile


def atlas_uv(n_faces, size, tile, device='cuda') -> torch.Tensor:
    """The corner UVs fp32 [F, 3, 2] of the layout: each face's corners sit on texel centres, (i + 0.5) / size."""
    return ops.meshtex_uv(n_faces, size, tile, device)


def _atlas_normals(who, mesh, normals, box=None):
    if normals not in ('flat', 'faces', 'mesh'):
        raise _lib.PerfError(f"{who}: normals is 'flat', 'faces' or 'mesh', got {normals!r}")
    if normals == 'mesh':
        if mesh.normals is None:
            raise _lib.PerfError(f"{who}: normals='mesh' needs mesh.normals: extract them, or use normals='flat' or 'faces'")
        return mesh.normals.contiguous()
    return face_normals(mesh, box) if normals == 'faces' else None


def atlas_points(mesh, size, tile, normals='flat'):
    """The texel -> point map of the atlas, materialised -> (points fp32 [S * S, 3], point_normals fp32 [S * S, 3], face_of int32 [S * S],
    coverage uint8 [S * S]); texel (column i, row j) at element j S + i.  A texel's point is (a + beta (b - a)) + gamma (c - a) of its
    face, extrapolated (not clamped) in the gutter.  normals='flat': the face's own unit normal; 'faces': face_normals' vertex normals
    interpolated (not normalised); 'mesh': mesh.normals interpolated.  One host read: the flag of a face index outside [0, V), refused."""
    _check_mesh('atlas_points', mesh)
    vertices, faces = mesh.vertices.contiguous(), mesh.faces.contiguous()
    points, point_normals, face_of, coverage, flag = ops.meshtex_points(vertices, faces, size, tile, _atlas_normals('atlas_points', mesh, normals))
    bad = int(flag.item())          # the one host synchronisation
    if bad >= 0:
        _raise_bad_face('atlas_points', faces, bad, vertices.shape[0])
    return points, point_normals, face_of, coverage


def bake_panorama_texture(mesh, views, size=None, tile=None, normals='flat', **kw) -> Atlas:
    """A texture atlas of the mesh baked from the registered panoramas in ONE launch: every texel's point goes through the blend of
    panorama_colors (its keywords: tol, facing, power, select, fill; box for normals='faces'), so a mesh of any size carries as many colour
    samples as the atlas has texels.  The layout is atlas_layout's.  mesh.colors, when present, is the fallback of the texels no view
    passed for, interpolated over the face.  Every face gets the same texel budget (no area-proportional charts, no chart merging), no
    mip-safe padding between tiles, no exposure matching, at most 64 views.  One host read: the flag of a face index outside [0, V)."""
    _check_mesh('bake_panorama_texture', mesh)
    vertices, faces = mesh.vertices.contiguous(), mesh.faces.contiguous()
    size, tile = atlas_layout(faces.shape[0], size, tile)
    box = kw.pop('box', None)
    tol, facing, power, select = kw.pop('tol', 1 / 256), kw.pop('facing', True), kw.pop('power', 2), kw.pop('select', 'blend')
    fallback, fill = kw.pop('fallback', mesh.colors), kw.pop('fill', (0.5, 0.5, 0.5))
    if kw:
        raise _lib.PerfError(f'bake_panorama_texture: unknown keywords {sorted(kw)}')
    if select not in _lib.MESHCOLOR_SELECT:
        raise _lib.PerfError(f"bake_panorama_texture: select is 'blend' or 'best', got {select!r}")
    if facing and not 1 <= int(power) <= _lib.MESHTEX_MAX_POWER:
        raise _lib.PerfError(f'bake_panorama_texture: power {power} is outside 1 .. {_lib.MESHTEX_MAX_POWER}')
    if normals not in ('flat', 'faces', 'mesh'):
        raise _lib.PerfError(f"bake_panorama_texture: normals is 'flat', 'faces' or 'mesh', got {normals!r}")
    weigh_by = _atlas_normals('bake_panorama_texture', mesh, normals, box) if facing else None          # (the normals are read only with facing)
    cv = _color_views('bake_panorama_texture', views)
    image, weight, used, coverage, flag = ops.meshtex_bake(vertices, faces, size, tile, cv.views.table, cv.views.sizes, cv.pointers, float(tol), weigh_by, facing, power,
                                                           select, fallback.contiguous() if fallback is not None else None, fill)
    uv = ops.meshtex_uv(faces.shape[0], size, tile, faces.device)
    bad = int(flag.item())          # the one host synchronisation
    if bad >= 0:
        _raise_bad_face('bake_panorama_texture', faces, bad, vertices.shape[0])
    return Atlas(size, tile, uv, image, coverage, weight, used)


def bake_field_texture(scene, mesh, size=None, tile=None, fill=(0.5, 0.5, 0.5)) -> Atlas:
    """A texture atlas of the mesh from the field's own colours: vertex_colors at the covered texels' points (atlas_points); texels of no
    face take fill.  weight is 1 at the covered texels, used is 0."""
    _check_mesh('bake_field_texture', mesh)
    size, tile = atlas_layout(mesh.faces.shape[0], size, tile)
    points, _, _, coverage = atlas_points(mesh, size, tile)
    covered = coverage != 0
    image = torch.tensor([float(v) for v in fill], dtype=torch.float32, device=points.device).repeat(size * size, 1)
    image[covered] = vertex_colors(scene, points[covered].contiguous())
    uv = ops.meshtex_uv(mesh.faces.shape[0], size, tile, points.device)
    return Atlas(size, tile, uv, image.view(size, size, 3), coverage.view(size, size), covered.float().view(size, size),
                 torch.zeros(size, size, dtype=torch.int64, device=points.device))


def sample_atlas(atlas, face_ids, bary) -> torch.Tensor:
    """The atlas' colour at points of the mesh's faces, bilinear, in torch (float64) -> [N, 3] float64.  face_ids [N] integers; bary
    [N, 3]: the weights (alpha, beta, gamma) of the face's corners a, b, c.  The texture coordinate is the corners' uv weighted by bary;
    the texel centre (i, j) sits at (u, v) S - 0.5; taps are clamped to the image."""
    s = int(atlas.size)
    corner = atlas.uv.double()[face_ids.long()] * s - 0.5                                   # [N, 3, 2]: the corners in texel units
    xy = (bary.double().to(corner.device)[:, :, None] * corner).sum(dim=1)
    x, y = xy[:, 0], xy[:, 1]
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    image = atlas.image.double()
    at = lambda yy, xx: image[yy.long().clamp(0, s - 1), xx.long().clamp(0, s - 1)]
    top = at(y0, x0) * (1 - fx)[:, None] + at(y0, x0 + 1) * fx[:, None]
    bottom = at(y0 + 1, x0) * (1 - fx)[:, None] + at(y0 + 1, x0 + 1) * fx[:, None]
    return top * (1 - fy)[:, None] + bottom * fy[:, None]


def atlas_image_u8(atlas) -> np.ndarray:
    """The atlas' image as a file holds it: uint8 [S, S, 3], clipped to [0, 1], ROW S - 1 FIRST (OBJ's v points up)."""
    image = np.nan_to_num(atlas.image.detach().cpu().numpy().astype(np.float64), nan=0.0)
    return np.ascontiguousarray(np.rint(np.clip(image, 0.0, 1.0) * 255.0).astype(np.uint8)[::-1])


def write_obj(path, mesh, atlas):
    """Wavefront OBJ + MTL + the atlas' image beside it -> the image's path.  Three `vt` per face and `f a/ta b/tb c/tc`; the image is
    8-bit, clipped, row S - 1 first; PNG through PIL when it imports, binary PPM otherwise."""
    import os
    v = mesh.vertices.detach().cpu().numpy().astype(np.float64)
    f = mesh.faces.detach().cpu().numpy().astype(np.int64)
    uv = atlas.uv.detach().cpu().numpy().astype(np.float64).reshape(-1, 2)
    if len(uv) != 3 * len(f):
        raise _lib.PerfError(f'write_obj: the atlas holds the corners of {len(uv) // 3} faces, the mesh has {len(f)}')
    stem = os.path.splitext(path)[0]
    pixels = atlas_image_u8(atlas)
    try:
        from PIL import Image
        image_path = stem + '.png'
        Image.fromarray(pixels, 'RGB').save(image_path)
    except ImportError:
        image_path = stem + '.ppm'
        with open(image_path, 'wb') as out:
            out.write(f'P6\n{pixels.shape[1]} {pixels.shape[0]}\n255\n'.encode('ascii'))
            out.write(pixels.tobytes())
    with open(stem + '.mtl', 'w') as out:
        out.write(f'newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {os.path.basename(image_path)}\n')
    lines = [f'mtllib {os.path.basename(stem)}.mtl', 'usemtl atlas']
    lines += ['v %.9g %.9g %.9g' % tuple(row) for row in v]
    lines += ['vt %.9g %.9g' % tuple(row) for row in uv]
    lines += ['f %d/%d %d/%d %d/%d' % (a + 1, 3 * i + 1, b + 1, 3 * i + 2, c + 1, 3 * i + 3) for i, (a, b, c) in enumerate(f)]
    with open(path, 'w') as out:
        out.write('\n'.join(lines) + '\n')
    return image_path


# ---- rays against the mesh itself: closest hit, any hit, occlusion-aware cull (include/perf_hip_meshray.h) ------------------------------
class RayGrid(NamedTuple):
    origin: tuple                                # 3 floats: the fp32 corner of the box
    cell: float                                  # the fp32 cell edge; the margin of the lists is cell / 8
    dims: tuple                                  # (nx, ny, nz)
    offsets: torch.Tensor                        # [nx * ny * nz] int32: where each cell's faces begin in refs, cell (i, j, k) at (i ny + j) nz + k
    refs: torch.Tensor                           # [R] int32: face indices, cell by cell, in no particular order inside a cell
    n_vertices: int                              # of the mesh the grid was built of
    n_faces: int
    bad_face: int                                # the smallest index of a face that can never be hit (an index outside [0, V), a vertex that is not finite), or -1


class RayHits(NamedTuple):
    t: torch.Tensor                              # [N] fp32: the ray parameter of the closest hit, +inf where nothing is hit
    face: torch.Tensor                           # [N] int32: the face hit, -1 where none
    u: torch.Tensor                              # [N] fp32: the hit point is (1 - u - v) a + u b + v c; 0 where nothing is hit
    v: torch.Tensor                              # [N] fp32


def _default_cells(n_faces):
    """Cells along the longest axis of the box: round(cbrt(2 F)) in 1 .. 255 -- about two cells per face over a cubic box, a cell about
    two lattice spacings wide for a surface-nets room (F ~ 12 n^2 at resolution n), and (255 + 1)^3 = 2^24 cells at the most."""
    return min(255, max(1, round((2.0 * max(int(n_faces), 1)) ** (1.0 / 3.0))))


def build_ray_grid(mesh, cell=None) -> RayGrid:
    """The uniform grid the ray queries walk: the box is the bounds of the mesh's finite vertices widened by the margin cell / 8, so every
    finite vertex lies inside and the walked results equal brute force over all faces unconditionally (the grid only skips faces that
    cannot hit).  cell None: the longest edge of the bounds over round(cbrt(2 F)) (at most 255).  Memory: 4 bytes per cell of counts
    (freed on return), 4 per cell of offsets and 4 per reference, under the cap of 2^24 cells (64 MiB each); a surface-nets room lists a face
    3.7 times at 256^3 and 2.7 times at 1024^3 at the default cell.  Count -> scan -> write with two host reads: the six bounds, then the reference count with the
    flag of a face that can never be hit (kept in RayGrid.bad_face, not refused: such a face is listed nowhere)."""
    _check_mesh('build_ray_grid', mesh)
    vertices, faces = mesh.vertices.contiguous(), mesh.faces.contiguous()
    bounds = ops.meshsimp_bounds(vertices).tolist()          # the host read-back of the six bounds
    if not all(math.isfinite(b) for b in bounds):            # (no finite coordinate along an axis: nothing can be hit)
        bounds = [0.0] * 6
    lo, hi = bounds[:3], bounds[3:]
    if cell is None:
        longest = max(b - a for a, b in zip(lo, hi))
        cell = longest / _default_cells(faces.shape[0]) if longest > 0 else 1.0
    h = float(np.float32(cell))
    if not math.isfinite(h) or h <= 0:
        raise _lib.PerfError(f'build_ray_grid: the cell edge {cell!r} is not positive or not finite')
    m = h / 8.0
    origin = []
    for a in lo:
        o = np.float32(a - m)
        while float(o) > a - m:                             # (the fp32 corner never lies above lo - m)
            o = np.nextafter(o, np.float32(-np.inf))
        origin.append(float(o))
    dims = [int(math.floor((b + m - o) / h)) + 1 for o, b in zip(origin, hi)]
    if dims[0] * dims[1] * dims[2] > _lib.MESHRAY_MAX_CELLS:
        raise _lib.PerfError(f'build_ray_grid: a cell of {h} makes {dims} cells over the mesh\'s bounds, more than 2^24: choose a larger cell')
    counts, flag = ops.meshray_grid_count(vertices, faces, origin, h, dims)
    offsets, total = ops.exclusive_scan_i32(counts)
    n_refs, bad = (int(v) for v in torch.cat([total, flag]).tolist())          # the host read of the reference count, with the flag
    if n_refs >= 1 << 31:
        raise _lib.PerfError(f'build_ray_grid: {n_refs} references are 2^31 or more: choose a larger cell')
    refs = ops.meshray_grid_write(vertices, faces, origin, h, dims, counts, offsets, n_refs)
    return RayGrid(tuple(origin), h, tuple(dims), offsets, refs, int(vertices.shape[0]), int(faces.shape[0]), bad)


def _check_grid(who, mesh, grid):
    _check_mesh(who, mesh)
    if not isinstance(grid, RayGrid):
        raise _lib.PerfError(f'{who}: grid is the RayGrid of build_ray_grid, got {type(grid).__name__}')
    if grid.n_vertices != int(mesh.vertices.shape[0]) or grid.n_faces != int(mesh.faces.shape[0]):
        raise _lib.PerfError(f'{who}: the grid was built of a mesh of {grid.n_vertices} vertices and {grid.n_faces} faces, this one has {int(mesh.vertices.shape[0])} and '
                             f'{int(mesh.faces.shape[0])}')
    return mesh.vertices.contiguous(), mesh.faces.contiguous()


def cast_rays(mesh, grid, origins, directions, t_min=0.0, t_max=float('inf'), any_hit=False):
    """Rays origins + t directions (CUDA fp32 [N, 3] each; directions need not be unit) against the mesh: the closest hit by the rule of
    include/perf_hip_meshray.h -- double Moeller-Trumbore per face, two-sided, t_min <= t <= t_max, the lexicographic minimum of (t, face
    index) over ALL faces -> RayHits; any_hit: uint8 [N], 1 iff some face is hit.  The grid only skips faces that cannot hit: the result does
    not depend on its cell, and is bit-identical from run to run.  Not watertight along shared edges.  No host read."""
    vertices, faces = _check_grid('cast_rays', mesh, grid)
    for name, t in (('origins', origins), ('directions', directions)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.PerfError(f'cast_rays: {name} must be a CUDA tensor (there is no CPU path)')
    if math.isnan(float(t_min)) or math.isnan(float(t_max)):
        raise _lib.PerfError(f'cast_rays: t_min ({t_min}) or t_max ({t_max}) is NaN')
    out = ops.meshray_cast(vertices, faces, grid.origin, grid.cell, grid.dims, grid.offsets, grid.refs, origins.contiguous(), directions.contiguous(), t_min, t_max, any_hit)
    return out if any_hit else RayHits(*out)


def vertex_occlusion(mesh, grid, views, visibility) -> torch.Tensor:
    """int64 [V]: bit k is set iff bit k of visibility.visible is set and the mesh itself cuts the segment from the vertex to view k's centre
    (a strict 0 < t < 1; the faces that name the vertex are not tested).  views: what vertex_visibility takes; at most 64.  No host read."""
    vertices, faces = _check_grid('vertex_occlusion', mesh, grid)
    v = _views('vertex_occlusion', views)
    if visibility.n_views != len(v.sizes):
        raise _lib.PerfError(f'vertex_occlusion: the visibility holds bits of {visibility.n_views} views, {len(v.sizes)} views are given')
    return ops.meshray_occluded(vertices, faces, grid.origin, grid.cell, grid.dims, grid.offsets, grid.refs, v.centres, visibility.visible)


def cull_occluded(mesh, views, tol=1 / 256, free_tol=None, facing=True, min_views=1, carve=False, cell=None) -> Mesh:
    """cull_unseen with an occlusion test against the mesh itself: vertex_visibility -> vertex_occlusion on those bits -> the faces rule of
    visible_faces on visible & ~occluded -> filter_faces.  A camera inside a room does not see the back of the density shell through the
    front skin, whatever the faces' winding (facing=False suffices).  cell: of build_ray_grid."""
    _check_mesh('cull_occluded', mesh)
    v = _views('cull_occluded', views)
    visibility = vertex_visibility(mesh.vertices, v, tol, free_tol)
    occluded = vertex_occlusion(mesh, build_ray_grid(mesh, cell), v, visibility)
    visibility = Visibility(visibility.visible & ~occluded, visibility.free, visibility.n_views)
    counts = torch.empty(3, dtype=torch.int64, device=mesh.faces.device)
    keep, _ = _face_keep('cull_occluded', mesh, visibility, v, facing, min_views, carve, counts[2:])
    return _filter_faces(mesh, keep, counts, 'cull_occluded')[0]


def mesh_distance(mesh, grid, rays_o, rays_d) -> torch.Tensor:
    """fp32 [N]: the closest t >= 0 along rays_o + t rays_d (the distance for unit directions), +inf where the mesh is not hit."""
    vertices, faces = _check_grid('mesh_distance', mesh, grid)
    for name, t in (('rays_o', rays_o), ('rays_d', rays_d)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.PerfError(f'mesh_distance: {name} must be a CUDA tensor (there is no CPU path)')
    return ops.meshray_cast(vertices, faces, grid.origin, grid.cell, grid.dims, grid.offsets, grid.refs, rays_o.contiguous(), rays_d.contiguous(), uv=False)[0]


# ---- mesh-to-mesh deviation: the closest point of a mesh, on the rays' grid (include/staged/perf_hip_meshnear.h) -----------------------------
class NearestHits(NamedTuple):
    dist2: torch.Tensor                          # [N] float64: the squared distance to the closest point, +inf where there is no answer
    distance: torch.Tensor                       # [N] fp32: dist2.sqrt().float()
    face: torch.Tensor                           # [N] int32: the face of the closest point (the smallest index among equals), -1 where none
    u: torch.Tensor                              # [N] fp32: the closest point is (1 - u - v) a + u b + v c; 0 where there is no answer
    v: torch.Tensor                              # [N] fp32


class Deviation(NamedTuple):
    max: float                                   # the largest distance of a sample of a to b; +inf when a sample has no answer within max_distance
    mean: float                                  # over the samples that have an answer, as rms and p90
    rms: float
    p90: float                                   # nearest rank: the ceil(0.9 n)-th smallest distance
    argmax_point: tuple                          # the sample of max (the first of equals), three floats; None without samples
    argmax_face_of_b: int                        # the face of b closest to it; -1 when it has no answer
    n_samples: int
    n_beyond: int = 0                            # samples with no answer within max_distance (or not finite): counted, and they make max +inf
    a_to_b: Optional['Deviation'] = None         # symmetric: the two directions; the fields above are those of the direction with the larger
    b_to_a: Optional['Deviation'] = None         # max (the sampled Hausdorff distance), a_to_b's when they are equal


def closest_point(mesh, grid, points, max_distance=float('inf')) -> NearestHits:
    """The closest point of the mesh to every point (CUDA fp32 [N, 3]) by the rule of include/staged/perf_hip_meshnear.h -- the double
    seven-region closest point of a triangle, the lexicographic minimum of (dist2, face index) over ALL faces -> NearestHits.  grid: the
    RayGrid of build_ray_grid; it only skips faces that cannot be the answer, so the result does not depend on its cell and is
    bit-identical from run to run.  A point that is not finite, a mesh without a valid face and an answer beyond max_distance give +inf,
    -1, 0, 0.  The search visits the O((d / cell)^3) cells within the answer's distance d: bound it with max_distance for points far from
    the mesh.  No host read."""
    vertices, faces = _check_grid('closest_point', mesh, grid)
    if not torch.is_tensor(points) or not points.is_cuda:
        raise _lib.PerfError('closest_point: points must be a CUDA tensor (there is no CPU path)')
    if not float(max_distance) >= 0.0:
        raise _lib.PerfError(f'closest_point: max_distance ({max_distance}) is NaN or negative')
    dist2, face, u, v = ops.meshnear_query(vertices, faces, grid.origin, grid.cell, grid.dims, grid.offsets, grid.refs, points.contiguous(), max_distance)
    return NearestHits(dist2, dist2.sqrt().float(), face, u, v)


def _lattice(order):
    """The barycentric lattice points (i, j, k) with i + j + k = order that are not corners, j ascending, then k ascending."""
    return [(order - j - k, j, k) for j in range(order + 1) for k in range(order + 1 - j) if order not in (order - j - k, j, k)]


def surface_samples(mesh, order=2):
    """Points on the mesh -> (points fp32 [M, 3], face int32 [M]): the vertices first, with face -1; then per face, in face order, the
    barycentric lattice points (i, j, k) / order that are not corners (j ascending, then k; order 2: the three edge midpoints), each
    formed in float64 as ((i a + j b) + k c) / order and rounded once to fp32.  order 1: the vertices alone.  M = V + F ((order + 1)
    (order + 2) / 2 - 3).  The samples of a face with an index outside [0, V) are NaN.  Plain torch; no host read."""
    _check_mesh('surface_samples', mesh)
    order = int(order)
    if order < 1:
        raise _lib.PerfError(f'surface_samples: order {order} is below 1')
    vertices, faces = mesh.vertices.float(), mesh.faces
    n_vertices, n_faces = int(vertices.shape[0]), int(faces.shape[0])
    lattice = _lattice(order)
    face_of = torch.full((n_vertices,), -1, dtype=torch.int32, device=vertices.device)
    if not lattice or n_faces == 0 or n_vertices == 0:
        return vertices.contiguous(), face_of
    valid = ((faces >= 0) & (faces < n_vertices)).all(dim=1)
    corners = vertices.double()[faces.clamp(0, n_vertices - 1).long()]                        # [F, 3, 3]
    a, b, c = corners[:, 0], corners[:, 1], corners[:, 2]
    inner = torch.stack([((i * a + j * b) + k * c) / order for i, j, k in lattice], dim=1)          # [F, L, 3]
    inner = torch.where(valid[:, None, None], inner, torch.full_like(inner, float('nan'))).float().reshape(-1, 3)
    ids = torch.arange(n_faces, dtype=torch.int32, device=vertices.device).repeat_interleave(len(lattice))
    return torch.cat([vertices, inner]).contiguous(), torch.cat([face_of, ids])


_DEVIATION_WORDS = 10          # of one direction's statistics on the device


def _direction_stats(points, hits):
    """float64 [10] on the device: max dist2, mean, rms, p90 dist2, the index of max, its face, the samples with an answer, its point."""
    n = int(points.shape[0])
    if n == 0:
        return torch.zeros(_DEVIATION_WORDS, dtype=torch.float64, device=points.device)
    dist2 = hits.dist2
    within = hits.face >= 0
    n_within = within.sum()
    count = n_within.clamp(min=1).double()
    zero = torch.zeros_like(dist2)
    mean = torch.where(within, dist2.sqrt(), zero).sum() / count
    rms = (torch.where(within, dist2, zero).sum() / count).sqrt()
    rank = ((9 * n_within + 9) // 10 - 1).clamp(min=0)                                        # ceil(0.9 n) - 1; the samples beyond sort last (+inf)
    p90 = dist2.sort().values[rank]
    top = dist2.argmax()                                                                     # (the first of equal maxima)
    return torch.cat([torch.stack([dist2[top], mean, rms, p90, top.double(), hits.face[top].double(), n_within.double()]), points[top].double()])


def _deviation_of(words, n):
    if n == 0:
        return Deviation(0.0, 0.0, 0.0, 0.0, None, -1, 0)
    max2, mean, rms, p90, _, face, n_within = words[:7]
    return Deviation(math.sqrt(max2), mean, rms, math.sqrt(p90) if n_within else 0.0, tuple(words[7:10]), int(face), n, n - int(n_within))


def _deviations(directions):
    """[(samples, mesh, grid, max_distance)] -> [Deviation], with ONE host read for all of them."""
    stats = [_direction_stats(points, closest_point(mesh, grid, points, max_distance)) for points, mesh, grid, max_distance in directions]
    words = torch.cat(stats).tolist()                                                        # the one host read
    return [_deviation_of(words[_DEVIATION_WORDS * i:_DEVIATION_WORDS * (i + 1)], int(d[0].shape[0])) for i, d in enumerate(directions)]


def _symmetric(forward, backward):
    return (forward if forward.max >= backward.max else backward)._replace(a_to_b=forward, b_to_a=backward)


def mesh_deviation(a, b, order=2, symmetric=True, cell=None, max_distance=float('inf')) -> Deviation:
    """How far mesh a lies from mesh b: the distances from surface_samples(a, order) to their closest points on b (closest_point), and with
    symmetric also those from b's samples to a; the fields are then those of the direction with the larger max -- the SAMPLED Hausdorff
    distance: a lower bound of the true one, which is attained somewhere between the samples -- with both directions in a_to_b and b_to_a.
    The statistics are torch reductions of the float64 dist2 on the device, read back ONCE at the end (beside the grids' own reads).
    Samples without an answer within max_distance are counted in n_beyond and make max +inf: they are not dropped from it.  cell: of
    build_ray_grid."""
    _check_mesh('mesh_deviation', a)
    _check_mesh('mesh_deviation', b)
    directions = [(surface_samples(a, order)[0], b, build_ray_grid(b, cell), max_distance)]
    if symmetric:
        directions.append((surface_samples(b, order)[0], a, build_ray_grid(a, cell), max_distance))
    out = _deviations(directions)
    return _symmetric(*out) if symmetric else out[0]


def median_edge_length(mesh) -> float:
    """The median length of the 3 F face edges, computed on the device in float64 (one host read); 0 for a mesh without faces."""
    _check_mesh('median_edge_length', mesh)
    n_vertices, n_faces = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    if n_faces == 0 or n_vertices == 0:
        return 0.0
    corners = mesh.vertices.double()[mesh.faces.clamp(0, n_vertices - 1).long()]
    edges = (corners - corners.roll(-1, dims=1)).norm(dim=2).reshape(-1)
    return float(edges.nan_to_num(nan=0.0, posinf=0.0).median())


def tolerance_ladder(mesh, steps=10):
    """The default cells of simplify_to_tolerance: 16 times the mesh's median edge length, then each 1 / sqrt(2) of the one before."""
    first = 16.0 * median_edge_length(mesh)
    return [first * 0.5 ** (0.5 * k) for k in range(steps)] if first > 0 else []


def simplify_to_tolerance(mesh, tol, cells=None, placement='quadric', order=2, **kw):
    """The coarsest simplification of the mesh that stays within tol of it -> (Mesh, cell, Deviation).  cells: the cell edges to try,
    scanned in the order given, coarse to fine; default tolerance_ladder(mesh): at most ten, from 16 times the median edge length, each
    1 / sqrt(2) of the one before.  The first cell whose symmetric sampled deviation (mesh_deviation, order) has max <= tol is returned.
    No monotonicity is assumed: every cell is measured against the original.  If none passes, the finest (last) is returned with its
    deviation and a RuntimeWarning says so.  kw: simplify_mesh's (box, dedupe), and max_distance for the deviation's searches (a limit
    at or above tol leaves the decision as it is: a sample beyond it makes max +inf)."""
    _check_mesh('simplify_to_tolerance', mesh)
    tol = float(tol)
    if not tol >= 0.0:
        raise _lib.PerfError(f'simplify_to_tolerance: the tolerance {tol} is NaN or negative')
    max_distance = kw.pop('max_distance', float('inf'))
    cells = tolerance_ladder(mesh) if cells is None else [float(c) for c in cells]
    if not cells:
        raise _lib.PerfError('simplify_to_tolerance: no cell to try (a mesh without faces has no edge length to start from)')
    samples, grid = surface_samples(mesh, order)[0], build_ray_grid(mesh)
    for cell in cells:
        small = simplify_mesh(mesh, cell, placement=placement, **kw)[0]
        deviation = _symmetric(*_deviations([(surface_samples(small, order)[0], mesh, grid, max_distance), (samples, small, build_ray_grid(small), max_distance)]))
        if deviation.max <= tol:
            return small, cell, deviation
    import warnings
    warnings.warn(f'simplify_to_tolerance: no cell of {cells} stays within {tol}: the finest is returned with a deviation of {deviation.max}', RuntimeWarning)
    return small, cell, deviation


def transfer_vertex_values(src_mesh, values, hits) -> torch.Tensor:
    """The values [V, C] of src_mesh's vertices at the closest points of hits (closest_point against src_mesh) -> [N, C] of values' dtype:
    ((1 - u - v) val[a] + u val[b]) + v val[c] in float64, rounded once; NaN where a point has no answer.  The original's colours at a
    simplified mesh's vertices, for one.  Plain torch; no host read."""
    _check_mesh('transfer_vertex_values', src_mesh)
    n_vertices = int(src_mesh.vertices.shape[0])
    if not torch.is_tensor(values) or values.dim() != 2 or int(values.shape[0]) != n_vertices or values.device != src_mesh.vertices.device:
        raise _lib.PerfError(f'transfer_vertex_values: values must be a [{n_vertices}, C] tensor on the mesh\'s device')
    n = int(hits.face.shape[0])
    if int(src_mesh.faces.shape[0]) == 0 or n_vertices == 0:
        return torch.full((n, int(values.shape[1])), float('nan'), dtype=values.dtype, device=values.device)
    corners = src_mesh.faces[hits.face.clamp(min=0).long()].clamp(0, n_vertices - 1).long()          # [N, 3]
    val = values.double()
    u, v = hits.u.double()[:, None], hits.v.double()[:, None]
    out = (((1.0 - u) - v) * val[corners[:, 0]] + u * val[corners[:, 1]]) + v * val[corners[:, 2]]
    return torch.where((hits.face >= 0)[:, None], out, torch.full_like(out, float('nan'))).to(values.dtype)


def write_ply(path, mesh):
    """Binary little-endian PLY: x y z [nx ny nz] [red green blue as uchar] per vertex, a uchar-counted int list per face."""
    v = mesh.vertices.detach().cpu().numpy().astype('<f4')
    f = mesh.faces.detach().cpu().numpy().astype('<i4')
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if mesh.normals is not None:
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
    if mesh.colors is not None:
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    rows = np.empty(len(v), dtype=fields)
    rows['x'], rows['y'], rows['z'] = v[:, 0], v[:, 1], v[:, 2]
    if mesh.normals is not None:
        n = mesh.normals.detach().cpu().numpy().astype('<f4')
        rows['nx'], rows['ny'], rows['nz'] = n[:, 0], n[:, 1], n[:, 2]
    if mesh.colors is not None:
        c = np.rint(np.clip(mesh.colors.detach().cpu().numpy(), 0.0, 1.0) * 255.0).astype('u1')
        rows['red'], rows['green'], rows['blue'] = c[:, 0], c[:, 1], c[:, 2]
    tris = np.empty(len(f), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    tris['n'] = 3
    tris['i'] = f
    names = {'<f4': 'float', 'u1': 'uchar'}
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}']
    header += [f'property {names[t]} {k}' for k, t in fields]
    header += [f'element face {len(f)}', 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as out:
        out.write(('\n'.join(header) + '\n').encode('ascii'))
        out.write(rows.tobytes())
        out.write(tris.tobytes())
