"""What the mesh units' bindings in perf_amd/ops.py accept and refuse, as one table over the smallest inputs that reach every check: a
tetrahedron (V = 4, F = 4), K = 2 views with 4 x 8 maps, an atlas of 64 with tiles of 4, a 2 x 2 x 2 ray grid, an 8 x 8 x 8 brick lattice
under a 4^3 occupancy grid, a [3, 3, 3] dense field, C = 2 components or clusters and N = 3 rays.

Refusals.  Every tensor argument of every one of the 33 bindings is sent in six wrong forms (KINDS): another dtype, a trailing dimension
more, a length more, a strided view of the same shape, a CPU copy, a list.  A refusal is a PerfError that names the argument, raised before
perf_amd._lib.call is entered (a recorder stands in its place; workspace-size queries do not go through it).  The table was run against
the bindings as they stood before they were rewritten on shared helpers, and records where they did something else:
  NOT_REFUSED         the form was accepted: the case asserts the entry point the recorder saw and the outputs' dtypes and shapes.  The
                      recorder does not call through for these, since several hand the library memory of another size than it is told.
  NOT_A_PERFERROR     not a PerfError at the parent: the form (a list) died there with an AttributeError.  The case asserts a PerfError
                      that names the argument, which is what the shared tensor check gives; against the earlier bindings these 77
                      cases, and no other of the file, fail, each with that AttributeError.
  UNNAMED             the form was refused with a message that names no argument (the pointer helper's) or another one: the case
                      asserts a PerfError before any call, whatever it names.
The workspaces (ws) are in the table like any other tensor.  The bindings judge them by their bytes and their device alone: a count
replaces one that does not serve, a write hands it on.

Accepted calls (PLAIN, QUIRKS, EMPTY) go through to the library: one plain call per binding, the forms the bindings are documented to
take (a strided mask is copied, K = 0 views need no CUDA centres, normals are read only with facing, the bake takes no normals) and
the empty mesh, component list and ray set, with an empty tensor of another dtype where the library gets NULL for it.  Each of these
calls is compared, argument by argument, with the call the earlier bindings made (tests/golden/mesh_binding_calls.json, see
described_call): which pointers are NULL, which tensor every other pointer is, every count and scalar.  The values are the other GPU
tests' business."""
import ctypes
import functools
import json
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, F64, I8, I32, I64, U8, BOOL = torch.float32, torch.float64, torch.int8, torch.int32, torch.int64, torch.uint8, torch.bool
SIZE, TILE = 64, 4
LO, HI, H, N3 = (-0.5, -0.5, -0.5), (1.5, 1.5, 1.5), 1.0, (2, 2, 2)          # the clustering grid, and the ray grid with H as its cell
SHAPE, THR, FILL = (8, 8, 8), 0.5, 0.0
TOL = 1 / 256
WS = 'ws'          # an output that is a workspace: int64, one dimension, any length
KINDS = ('dtype', 'trailing', 'length', 'strided', 'cpu', 'list')
OTHER = {F32: F64, F64: F32, I32: I64, I64: I32, U8: I32, BOOL: I32}


@functools.lru_cache(maxsize=None)
def base():
    """The valid inputs, made once through the bindings themselves and left unchanged."""
    from perf_amd import ops
    dev = 'cuda'
    b = SimpleNamespace()
    b.vertices = torch.tensor([[0, 0, 0], [0.2, 0, 0], [0, 0.2, 0], [1, 0, 0.3]], dtype=F32, device=dev)          # three in one cell of the grid, one in the next
    b.faces = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=I32, device=dev)
    b.normals = torch.nn.functional.normalize(b.vertices - b.vertices.mean(0), dim=1).contiguous()
    b.fallback = torch.full((4, 3), 0.25, dtype=F32, device=dev)
    # the dense lattice
    b.field = torch.zeros(3, 3, 3, dtype=F32, device=dev)
    b.field[1, 1, 1] = 1.0
    counts, b.mesh_ws = ops.mesh_count(b.field, THR)
    b.mesh_nv, b.mesh_nf = counts.tolist()
    # the brick lattice
    b.binaries = torch.ones(4, 4, 4, dtype=BOOL, device=dev)
    b.table, n_live = ops.brickmesh_select(b.binaries, SHAPE)
    assert n_live.item() == 1
    b.ids = ops.brickmesh_list(b.table, 1)
    b.values = torch.zeros(512, dtype=F32, device=dev)
    b.values[3 * 64 + 3 * 8 + 3] = 1.0
    counts, b.brick_ws = ops.brickmesh_count(b.values, b.ids, b.table, SHAPE, THR, FILL)
    b.brick_nv, b.brick_nf, _ = counts.tolist()
    # components
    b.component = torch.zeros(4, dtype=I32, device=dev)
    b.keep = torch.tensor([True, False], device=dev)
    counts, b.cc_ws = ops.meshcc_filter_count(b.faces, b.component, b.keep)
    b.cc_nv, b.cc_nf = counts.tolist()
    # views
    b.poses = [torch.eye(4), torch.tensor([[1, 0, 0, 0.5], [0, 1, 0, 0.25], [0, 0, 1, 0.0], [0, 0, 0, 1]])]
    b.distance_maps = [torch.full((4, 8), 2.0, dtype=F32, device=dev) for _ in range(2)]
    b.color_maps = [torch.full((4, 8, 3), 0.5, dtype=F32, device=dev) for _ in range(2)]
    b.views, b.centres, b.sizes, b.kept_maps = ops.meshvis_views(b.poses, b.distance_maps)
    b.pointers, b.kept_colors = ops.meshcolor_maps(b.color_maps, b.sizes)
    b.visible, b.free = ops.meshvis_vertex_bits(b.vertices, b.views, b.sizes, TOL, 4 * TOL)
    b.face_keep = torch.tensor([1, 0, 1, 1], dtype=U8, device=dev)
    counts, b.vis_ws = ops.meshvis_filter_count(b.faces, 4, b.face_keep)
    b.vis_nv, b.vis_nf = counts.tolist()
    # clusters
    b.cluster, counts, b.simp_ws = ops.meshsimp_cluster(b.vertices, LO, H, N3, n_faces=4)
    assert counts.tolist() == [2, -1]
    b.anchor, b.representative = ops.meshsimp_place(b.vertices, LO, H, N3, b.cluster, 2)
    b.quadrics, _ = ops.meshquadric_sums(b.vertices, b.faces, LO, H, N3, b.cluster, 2)
    b.normal_sums, _ = ops.meshcolor_normal_sums(b.vertices, b.faces, 36)
    # rays
    b.cell_counts, _ = ops.meshray_grid_count(b.vertices, b.faces, LO, H, N3)
    full = b.cell_counts.clone()
    b.offsets, total = ops.exclusive_scan_i32(b.cell_counts)
    b.n_refs = int(total.item())
    b.refs = ops.meshray_grid_write(b.vertices, b.faces, LO, H, N3, b.cell_counts, b.offsets, b.n_refs)
    b.cell_counts = full          # (the write counts them down to 0: every call below gets a copy)
    b.rays_o = torch.tensor([[0.1, 0.1, -0.4], [0.3, 0.1, 0.9], [1.2, 1.2, 1.2]], dtype=F32, device=dev)
    b.rays_d = torch.tensor([[0, 0, 1], [0, 0, -1], [0, 1, 0]], dtype=F32, device=dev)
    # the empty mesh and its companions
    b.v0, b.f0 = torch.zeros(0, 3, dtype=F32, device=dev), torch.zeros(0, 3, dtype=I32, device=dev)
    b.i0, b.l0, b.u0 = torch.zeros(0, dtype=I32, device=dev), torch.zeros(0, dtype=I64, device=dev), torch.zeros(0, dtype=U8, device=dev)
    b.views0, b.pointers0 = torch.zeros(0, 16, dtype=I32), torch.zeros(0, dtype=I64)          # K = 0: on the host
    b.d0 = torch.zeros(0, dtype=F64, device=dev)
    b.no_bricks = torch.full_like(b.table, -1)
    _, b.cc_ws0 = ops.meshcc_filter_count(b.f0, b.i0, b.u0)
    _, b.vis_ws0 = ops.meshvis_filter_count(b.f0, 0, b.u0)
    _, b.brick_ws0 = ops.brickmesh_count(b.d0.float(), b.i0, b.no_bricks, SHAPE, THR, FILL)
    return b


def n_of(t):
    return int(t.shape[0])


# binding -> (entry point, the plain call's arguments, {tensor argument: (dimensions, the word its refusal names)}, the outputs' (dtype, shape))
SPECS = {
    'mesh_count': ('perf_mesh_count', lambda b: dict(ws=b.mesh_ws, field=b.field, thr=THR), {'field': 3},
                   lambda k: [(I64, (2,)), WS]),
    'mesh_write': ('perf_mesh_write', lambda b: dict(field=b.field, thr=THR, lo=LO, hi=HI, ws=b.mesh_ws, n_vertices=b.mesh_nv, n_faces=b.mesh_nf), {'field': 3},
                   lambda k: [(F32, (k['n_vertices'], 3)), (I32, (k['n_faces'], 3))]),
    'brickmesh_select': ('perf_brickmesh_select', lambda b: dict(ws=b.brick_ws, binaries=b.binaries, shape=SHAPE), {'binaries': 3},
                         lambda k: [(I32, (1, 1, 1)), (I64, (1,))]),
    'brickmesh_list': ('perf_brickmesh_list', lambda b: dict(table=b.table, n_bricks=1), {'table': 3},
                       lambda k: [(I32, (k['n_bricks'],))]),
    'brickmesh_corners': ('perf_brickmesh_corners', lambda b: dict(ids=b.ids, first=0, m=1, shape=SHAPE, binaries=b.binaries), {'ids': 1, 'binaries': 3},
                          lambda k: [(F32, (512 * k['m'], 3)), (U8, (512 * k['m'],)), (U8, (512 * k['m'],))]),
    'brickmesh_count': ('perf_brickmesh_count', lambda b: dict(ws=b.brick_ws, values=b.values, ids=b.ids, table=b.table, shape=SHAPE, thr=THR, fill=FILL),
                        {'values': 1, 'ids': 1, 'table': 3}, lambda k: [(I64, (3,)), WS]),
    'brickmesh_write': ('perf_brickmesh_write', lambda b: dict(values=b.values, ids=b.ids, table=b.table, shape=SHAPE, thr=THR, fill=FILL, lo=LO, hi=HI, ws=b.brick_ws,
                                                               n_vertices=b.brick_nv, n_faces=b.brick_nf), {'values': 1, 'ids': 1, 'table': 3},
                        lambda k: [(F32, (k['n_vertices'], 3)), (I32, (k['n_faces'], 3)), (I64, (k['n_vertices'],))]),
    'meshcc_label': ('perf_meshcc_label', lambda b: dict(ws=b.cc_ws, faces=b.faces, n_vertices=4), {'faces': 2},
                     lambda k: [(I32, (k['n_vertices'],)), (I64, (2,)), WS]),
    'meshcc_stats': ('perf_meshcc_stats', lambda b: dict(faces=b.faces, vertex_component=b.component, n_components=2, vertices=b.vertices),
                     {'faces': 2, 'vertex_component': 1, 'vertices': 2},
                     lambda k: [(I64, (k['n_components'],)), (I32, (k['n_components'],)), (F64, (k['n_components'],)) if k['vertices'] is not None else None]),
    'meshcc_filter_count': ('perf_meshcc_filter_count', lambda b: dict(ws=b.cc_ws, faces=b.faces, vertex_component=b.component, keep=b.keep),
                            {'faces': 2, 'vertex_component': 1, 'keep': 1}, lambda k: [(I64, (2,)), WS]),
    'meshcc_filter_write': ('perf_meshcc_filter_write', lambda b: dict(faces=b.faces, vertex_component=b.component, keep=b.keep, ws=b.cc_ws, n_vertices_kept=b.cc_nv,
                                                                       n_faces_kept=b.cc_nf, vertices=b.vertices),
                            {'faces': 2, 'vertex_component': 1, 'keep': 1, 'vertices': 2},
                            lambda k: [(F32, (k['n_vertices_kept'], 3)) if k['vertices'] is not None else None, (I32, (k['n_faces_kept'], 3)), (I32, (k['n_vertices_kept'],))]),
    'meshvis_views': ('', lambda b: dict(poses=b.poses, maps=b.distance_maps), {'poses[1]': (2, 'pose'), 'maps[1]': (2, 'map')},
                      lambda k: [(I32, (len(k['maps']), 16)), (F32, (len(k['maps']), 3)), list, list]),
    'meshvis_vertex_bits': ('perf_meshvis_vertex_bits', lambda b: dict(vertices=b.vertices, views=b.views, sizes=b.sizes, tol=TOL, free_tol=4 * TOL),
                            {'vertices': 2, 'views': 2}, lambda k: [(I64, (n_of(k['vertices']),))] * 2),
    'meshvis_face_keep': ('perf_meshvis_face_keep', lambda b: dict(faces=b.faces, vertices=b.vertices, visible_bits=b.visible, free_bits=b.free, centres=b.centres,
                                                                   flag=torch.empty(1, dtype=I64, device='cuda')),
                          {'faces': 2, 'vertices': 2, 'visible_bits': 1, 'free_bits': 1, 'centres': 2, 'flag': 1},
                          lambda k: [(U8, (n_of(k['faces']),)), (k['flag'].dtype, tuple(k['flag'].shape)) if k['flag'] is not None else (I64, (1,))]),
    'meshvis_filter_count': ('perf_meshvis_filter_count', lambda b: dict(ws=b.vis_ws, faces=b.faces, n_vertices=4, face_keep=b.face_keep, counts=torch.empty(2, dtype=I64, device='cuda')),
                             {'faces': 2, 'face_keep': 1, 'counts': 1},
                             lambda k: [(k['counts'].dtype, tuple(k['counts'].shape)) if k['counts'] is not None else (I64, (2,)), WS]),
    'meshvis_filter_write': ('perf_meshvis_filter_write', lambda b: dict(faces=b.faces, n_vertices=4, face_keep=b.face_keep, ws=b.vis_ws, n_vertices_kept=b.vis_nv,
                                                                         n_faces_kept=b.vis_nf, vertices=b.vertices), {'faces': 2, 'face_keep': 1, 'vertices': 2},
                             lambda k: [(F32, (k['n_vertices_kept'], 3)) if k['vertices'] is not None else None, (I32, (k['n_faces_kept'], 3)), (I32, (k['n_vertices_kept'],))]),
    'meshsimp_bounds': ('perf_meshsimp_bounds', lambda b: dict(vertices=b.vertices), {'vertices': 2}, lambda k: [(F32, (6,))]),
    'meshsimp_cluster': ('perf_meshsimp_cluster', lambda b: dict(ws=b.simp_ws, vertices=b.vertices, lo=LO, h=H, n=N3, n_faces=4, counts=torch.empty(2, dtype=I64, device='cuda')),
                         {'vertices': 2, 'counts': 1},
                         lambda k: [(I32, (n_of(k['vertices']),)), (k['counts'].dtype, tuple(k['counts'].shape)) if k['counts'] is not None else (I64, (2,)), WS]),
    'meshsimp_place': ('perf_meshsimp_place', lambda b: dict(vertices=b.vertices, lo=LO, h=H, n=N3, vertex_cluster=b.cluster, n_clusters=2),
                       {'vertices': 2, 'vertex_cluster': 1}, lambda k: [(F32, (k['n_clusters'], 3)), (I32, (k['n_clusters'],))]),
    'meshsimp_faces': ('perf_meshsimp_faces', lambda b: dict(ws=b.simp_ws, faces=b.faces, vertex_cluster=b.cluster, flag=torch.empty(1, dtype=I64, device='cuda')),
                       {'faces': 2, 'vertex_cluster': 1, 'flag': 1},
                       lambda k: [(I32, (n_of(k['faces']), 3)), (U8, (n_of(k['faces']),)), (k['flag'].dtype, tuple(k['flag'].shape)) if k['flag'] is not None else (I64, (1,))]),
    'meshquadric_sums': ('perf_meshquadric_sums', lambda b: dict(vertices=b.vertices, faces=b.faces, lo=LO, h=H, n=N3, vertex_cluster=b.cluster, n_clusters=2,
                                                                 flags=torch.empty(2, dtype=I64, device='cuda')),
                         {'vertices': 2, 'faces': 2, 'vertex_cluster': 1, 'flags': 1}, lambda k: [(I64, (k['n_clusters'], 9)), (I64, (2,))]),
    'meshquadric_place': ('perf_meshquadric_place', lambda b: dict(vertices=b.vertices, lo=LO, h=H, n=N3, anchor=b.anchor, representative=b.representative, acc=b.quadrics),
                          {'vertices': 2, 'anchor': 2, 'representative': 1, 'acc': 2}, lambda k: [(F32, (n_of(k['acc']), 3))]),
    'meshcolor_normal_sums': ('perf_meshcolor_normal_sums', lambda b: dict(vertices=b.vertices, faces=b.faces, scale_log2=36, flag=torch.empty(1, dtype=I64, device='cuda')),
                              {'vertices': 2, 'faces': 2, 'flag': 1},
                              lambda k: [(I64, (n_of(k['vertices']), 3)), (k['flag'].dtype, tuple(k['flag'].shape)) if k['flag'] is not None else (I64, (1,))]),
    'meshcolor_normals': ('perf_meshcolor_normals', lambda b: dict(acc=b.normal_sums), {'acc': 2}, lambda k: [(F32, (n_of(k['acc']), 3))]),
    'meshcolor_maps': ('', lambda b: dict(color_maps=b.color_maps, sizes=b.sizes), {'color_maps[1]': (3, 'color_map')}, lambda k: [(I64, (len(k['color_maps']),)), list]),
    'meshcolor_blend': ('perf_meshcolor_blend', lambda b: dict(vertices=b.vertices, normals=b.normals, views=b.views, sizes=b.sizes, map_pointers=b.pointers, tol=TOL,
                                                               fallback=b.fallback),
                        {'vertices': 2, 'normals': 2, 'views': 2, 'map_pointers': 1, 'fallback': 2},
                        lambda k: [(F32, (n_of(k['vertices']), 3)), (F32, (n_of(k['vertices']),)), (I64, (n_of(k['vertices']),)), (I8, (n_of(k['vertices']),))]),
    'meshtex_uv': ('perf_meshtex_uv', lambda b: dict(n_faces=4, size=SIZE, tile=TILE), {}, lambda k: [(F32, (k['n_faces'], 3, 2))]),
    'meshtex_points': ('perf_meshtex_points', lambda b: dict(vertices=b.vertices, faces=b.faces, size=SIZE, tile=TILE, normals=b.normals,
                                                             flag=torch.empty(1, dtype=I64, device='cuda')),
                       {'vertices': 2, 'faces': 2, 'normals': 2, 'flag': 1},
                       lambda k: [(F32, (SIZE * SIZE, 3)), (F32, (SIZE * SIZE, 3)), (I32, (SIZE * SIZE,)), (U8, (SIZE * SIZE,)),
                                  (k['flag'].dtype, tuple(k['flag'].shape)) if k['flag'] is not None else (I64, (1,))]),
    'meshtex_bake': ('perf_meshtex_bake', lambda b: dict(vertices=b.vertices, faces=b.faces, size=SIZE, tile=TILE, views=b.views, sizes=b.sizes, map_pointers=b.pointers, tol=TOL,
                                                         normals=b.normals, fallback=b.fallback, flag=torch.empty(1, dtype=I64, device='cuda')),
                     {'vertices': 2, 'faces': 2, 'views': 2, 'map_pointers': 1, 'normals': 2, 'fallback': 2, 'flag': 1},
                     lambda k: [(F32, (SIZE, SIZE, 3)), (F32, (SIZE, SIZE)), (I64, (SIZE, SIZE)), (U8, (SIZE, SIZE)),
                                (k['flag'].dtype, tuple(k['flag'].shape)) if k['flag'] is not None else (I64, (1,))]),
    'meshray_grid_count': ('perf_meshray_grid_count', lambda b: dict(vertices=b.vertices, faces=b.faces, origin=LO, cell=H, dims=N3, flag=torch.empty(1, dtype=I64, device='cuda')),
                           {'vertices': 2, 'faces': 2, 'flag': 1},
                           lambda k: [(I32, (8,)), (k['flag'].dtype, tuple(k['flag'].shape)) if k['flag'] is not None else (I64, (1,))]),
    'meshray_grid_write': ('perf_meshray_grid_write', lambda b: dict(vertices=b.vertices, faces=b.faces, origin=LO, cell=H, dims=N3, counts=b.cell_counts.clone(),
                                                                     offsets=b.offsets, n_refs=b.n_refs),
                           {'vertices': 2, 'faces': 2, 'counts': 1, 'offsets': 1}, lambda k: [(I32, (k['n_refs'],))]),
    'meshray_cast': ('perf_meshray_cast', lambda b: dict(vertices=b.vertices, faces=b.faces, origin=LO, cell=H, dims=N3, offsets=b.offsets, refs=b.refs, rays_o=b.rays_o,
                                                         rays_d=b.rays_d),
                     {'vertices': 2, 'faces': 2, 'offsets': 1, 'refs': 1, 'rays_o': 2, 'rays_d': 2},
                     lambda k: [(F32, (n_of(k['rays_o']),)), (I32, (n_of(k['rays_o']),)), (F32, (n_of(k['rays_o']),)), (F32, (n_of(k['rays_o']),))]),
    'meshray_occluded': ('perf_meshray_occluded', lambda b: dict(vertices=b.vertices, faces=b.faces, origin=LO, cell=H, dims=N3, offsets=b.offsets, refs=b.refs,
                                                                 centres=b.centres, mask_bits=b.visible),
                         {'vertices': 2, 'faces': 2, 'offsets': 1, 'refs': 1, 'centres': 2, 'mask_bits': 1}, lambda k: [(I64, (n_of(k['vertices']),))]),
}
assert len(SPECS) == 33
for _fn in ('mesh_count', 'mesh_write', 'brickmesh_select', 'brickmesh_count', 'brickmesh_write', 'meshcc_label', 'meshcc_filter_count', 'meshcc_filter_write',
            'meshvis_filter_count', 'meshvis_filter_write', 'meshsimp_cluster', 'meshsimp_faces'):
    SPECS[_fn][2]['ws'] = 1          # the workspace: of the count that made it, and passed back into a count to be used again


def wrong(t, kind):
    """Tensor t in the wrong form `kind`."""
    if kind == 'dtype':
        return t.to(OTHER[t.dtype])
    if kind == 'trailing':
        return torch.cat([t, t[..., :1]], dim=-1).contiguous()
    if kind == 'length':
        return torch.cat([t, t[:1]], dim=0).contiguous()
    if kind == 'strided':
        return torch.stack([t, t], dim=-1)[..., 0]
    if kind == 'cpu':
        return t.cpu()
    return t.tolist()


def tensor_cases():
    for fn, (_, _, tensors, _) in SPECS.items():
        for arg, dims in tensors.items():
            dims = dims[0] if isinstance(dims, tuple) else dims
            for kind in KINDS:
                if kind != 'trailing' or dims > 1:          # (in one dimension the trailing one is the length)
                    yield f'{fn}-{arg}-{kind}'


def case_call(case):
    """(binding, keyword arguments, the word the refusal must hold) of a tensor case."""
    fn, arg, kind = case.split('-')
    _, plain, tensors, _ = SPECS[fn]
    kwargs = plain(base())
    word = tensors[arg][1] if isinstance(tensors[arg], tuple) else arg
    if arg.endswith(']'):          # an element of a list of tensors
        arg, i = arg[:-1].split('[')
        kwargs[arg] = list(kwargs[arg])
        kwargs[arg][int(i)] = wrong(kwargs[arg][int(i)], kind)
    else:
        kwargs[arg] = wrong(kwargs[arg], kind)
    return fn, kwargs, word


# ---- what the bindings did with these forms before they were rewritten on shared helpers (see the docstring) -----------------------------
def cases(*lines):
    """'binding: argument kind kind; argument kind' -> the set of case names."""
    out = set()
    for line in lines:
        fn, rest = line.split(': ')
        for part in rest.split('; '):
            arg, *kinds = part.split(' ')
            out.update(f'{fn}-{arg}-{kind}' for kind in kinds)
    return out


# accepted
NOT_REFUSED = cases(
    'mesh_count: field trailing length; ws dtype length cpu',
    'mesh_write: field trailing length; ws dtype length',
    'brickmesh_select: binaries strided; ws dtype length cpu',
    'brickmesh_list: table trailing length strided',
    'brickmesh_corners: ids length strided; binaries strided',
    'brickmesh_count: ids strided; table strided; ws dtype length cpu',
    'brickmesh_write: ids strided; table strided; ws dtype length',
    'meshcc_label: faces length; ws dtype length cpu',
    'meshcc_stats: faces length',
    'meshcc_filter_count: faces length; vertex_component length; keep length strided; ws dtype length cpu',
    'meshcc_filter_write: faces length; keep length strided; ws dtype length',
    'meshvis_views: poses[1] dtype trailing length strided cpu list; maps[1] trailing length strided',
    'meshvis_vertex_bits: vertices length',
    'meshvis_face_keep: faces length; centres length; flag dtype length strided',
    'meshvis_filter_count: face_keep strided; counts dtype length; ws dtype length cpu',
    'meshvis_filter_write: face_keep strided; ws dtype length',
    'meshsimp_bounds: vertices length',
    'meshsimp_cluster: vertices length; counts dtype length; ws dtype length cpu',
    'meshsimp_faces: faces length; vertex_cluster length; flag dtype length strided; ws dtype length cpu',
    'meshquadric_sums: faces length',
    'meshquadric_place: vertices length',
    'meshcolor_normal_sums: vertices length; faces length; flag dtype length strided',
    'meshcolor_normals: acc length',
    'meshcolor_maps: color_maps[1] dtype strided',
    'meshtex_points: faces length; flag dtype length strided',
    'meshtex_bake: faces length; flag dtype length strided',
    'meshray_grid_count: vertices length; faces length; flag dtype length strided',
    'meshray_grid_write: vertices length; faces length',
    'meshray_cast: vertices length; faces length; refs length',
    'meshray_occluded: faces length; refs length; centres length',
)

# died with AttributeError: 'list' object has no attribute ...
NOT_A_PERFERROR = cases(
    'mesh_count: field list; ws list',
    'mesh_write: field list; ws list',
    'brickmesh_select: binaries list; ws list',
    'brickmesh_list: table list',
    'brickmesh_corners: ids list; binaries list',
    'brickmesh_count: values list; ids list; table list; ws list',
    'brickmesh_write: values list; ids list; table list; ws list',
    'meshcc_label: faces list; ws list',
    'meshcc_stats: faces list; vertex_component list; vertices list',
    'meshcc_filter_count: faces list; vertex_component list; keep list; ws list',
    'meshcc_filter_write: faces list; vertex_component list; keep list; vertices list; ws list',
    'meshvis_vertex_bits: vertices list; views list',
    'meshvis_face_keep: faces list; vertices list; visible_bits list; free_bits list; centres list; flag list',
    'meshvis_filter_count: faces list; face_keep list; counts list; ws list',
    'meshvis_filter_write: faces list; face_keep list; vertices list; ws list',
    'meshsimp_cluster: counts list; ws list',
    'meshsimp_place: vertex_cluster list',
    'meshsimp_faces: faces list; vertex_cluster list; flag list; ws list',
    'meshquadric_sums: faces list; vertex_cluster list',
    'meshcolor_normal_sums: faces list; flag list',
    'meshcolor_blend: normals list; views list; map_pointers list; fallback list',
    'meshtex_points: faces list; normals list; flag list',
    'meshtex_bake: faces list; views list; map_pointers list; normals list; fallback list; flag list',
    'meshray_grid_count: faces list; flag list',
    'meshray_grid_write: faces list',
    'meshray_cast: faces list',
    'meshray_occluded: faces list; mask_bits list',
)

# refused, but the message names no argument, or another one (its companion of the other length; vertex_cluster as vertex_component; normals and fallback as vertices)
UNNAMED = cases(
    'mesh_count: field strided cpu; ws strided',
    'mesh_write: field strided cpu; ws strided cpu',
    'brickmesh_select: ws strided',
    'brickmesh_count: values strided; ws strided',
    'brickmesh_write: values strided; ws strided cpu',
    'meshcc_label: ws strided',
    'meshcc_stats: vertex_component length',
    'meshcc_filter_count: ws strided',
    'meshcc_filter_write: vertex_component length; ws strided cpu',
    'meshvis_face_keep: vertices length; flag cpu',
    'meshvis_filter_count: faces length; counts strided cpu; ws strided',
    'meshvis_filter_write: faces length; ws strided cpu',
    'meshsimp_cluster: counts strided cpu; ws strided',
    'meshsimp_place: vertices length; vertex_cluster dtype length strided cpu',
    'meshsimp_faces: vertex_cluster dtype strided cpu; flag cpu; ws strided',
    'meshquadric_sums: vertices length; vertex_cluster dtype length strided cpu',
    'meshquadric_place: acc length',
    'meshcolor_normal_sums: flag cpu',
    'meshcolor_blend: normals dtype trailing length strided cpu; map_pointers strided; fallback dtype trailing length strided cpu',
    'meshtex_points: normals dtype trailing length strided cpu; flag cpu',
    'meshtex_bake: map_pointers strided; normals dtype trailing length strided cpu; fallback dtype trailing length strided cpu; flag cpu',
    'meshray_grid_count: flag cpu',
    'meshray_cast: rays_o length',
    'meshray_occluded: vertices length',
)
assert (NOT_REFUSED | NOT_A_PERFERROR | UNNAMED) <= set(tensor_cases()) and not NOT_REFUSED & NOT_A_PERFERROR and not UNNAMED & (NOT_REFUSED | NOT_A_PERFERROR)


# ---- refusals that are not about a tensor's form: (binding, changed arguments, a word of the message) ---------------------------------------
def _many_views(b):
    return dict(poses=[torch.eye(4)] * 65, maps=[b.distance_maps[0]] * 65)


OTHER_REFUSALS = {
    'mesh_count-one_cell_short': ('mesh_count', lambda b: dict(field=b.field[:, :1].contiguous()), 'field'),
    'mesh_write-lo2': ('mesh_write', lambda b: dict(lo=LO[:2]), 'lo'),
    'mesh_write-hi2': ('mesh_write', lambda b: dict(hi=HI[:2]), 'hi'),
    'brickmesh_write-lo2': ('brickmesh_write', lambda b: dict(lo=LO[:2]), 'lo'),
    'brickmesh_select-shape2': ('brickmesh_select', lambda b: dict(shape=SHAPE[:2]), 'three dimensions'),
    'brickmesh_count-other_lattice': ('brickmesh_count', lambda b: dict(shape=(16, 8, 8)), 'table'),
    'meshcc_label-negative_vertices': ('meshcc_label', lambda b: dict(n_vertices=-1), 'vertices'),
    'meshcc_label-too_many_vertices': ('meshcc_label', lambda b: dict(n_vertices=(1 << 30) + 1), 'vertices'),
    'meshvis_views-65': ('meshvis_views', _many_views, '65 views are more than 64'),
    'meshvis_views-one_pose_short': ('meshvis_views', lambda b: dict(poses=b.poses[:1]), 'poses'),
    'meshvis_views-empty_map': ('meshvis_views', lambda b: dict(maps=[b.distance_maps[0], b.distance_maps[1][:0]]), 'map'),
    'meshvis_vertex_bits-one_size_short': ('meshvis_vertex_bits', lambda b: dict(sizes=b.sizes[:1]), 'views'),
    'meshsimp_cluster-lo2': ('meshsimp_cluster', lambda b: dict(lo=LO[:2]), 'lo'),
    'meshsimp_cluster-n2': ('meshsimp_cluster', lambda b: dict(n=N3[:2]), 'n hold three'),
    'meshsimp_cluster-no_cell': ('meshsimp_cluster', lambda b: dict(n=(2, 0, 2)), 'cells per axis are outside 1 .. 2^21'),
    'meshsimp_cluster-too_many_cells': ('meshsimp_cluster', lambda b: dict(n=(1, 1, (1 << 21) + 1)), 'cells per axis are outside 1 .. 2^21'),
    'meshsimp_place-n2': ('meshsimp_place', lambda b: dict(n=N3[:2]), 'n hold three'),
    'meshsimp_place-too_many_cells': ('meshsimp_place', lambda b: dict(n=((1 << 21) + 1, 1, 1)), 'cells per axis'),
    'meshsimp_place-placement': ('meshsimp_place', lambda b: dict(placement='median'), 'placement'),
    'meshsimp_faces-dedupe': ('meshsimp_faces', lambda b: dict(dedupe='sorted'), 'dedupe'),
    'meshquadric_sums-n2': ('meshquadric_sums', lambda b: dict(n=N3[:2]), 'n hold three'),
    'meshquadric_sums-no_cell': ('meshquadric_sums', lambda b: dict(n=(0, 2, 2)), 'cells per axis'),
    'meshquadric_sums-more_clusters_than_vertices': ('meshquadric_sums', lambda b: dict(n_clusters=5), 'clusters'),
    'meshquadric_sums-negative_clusters': ('meshquadric_sums', lambda b: dict(n_clusters=-1), 'clusters'),
    'meshquadric_place-lo2': ('meshquadric_place', lambda b: dict(lo=LO[:2]), 'lo'),
    'meshquadric_place-too_many_cells': ('meshquadric_place', lambda b: dict(n=(2, 2, 1 << 22)), 'cells per axis'),
    'meshquadric_place-more_clusters_than_vertices': ('meshquadric_place', lambda b: dict(acc=b.quadrics.new_zeros(5, 9), anchor=b.anchor.new_zeros(5, 3),
                                                                                           representative=b.representative.new_zeros(5)), 'acc'),
    'meshcolor_maps-one_map_short': ('meshcolor_maps', lambda b: dict(color_maps=b.color_maps[:1]), 'colour maps'),
    'meshcolor_maps-other_size': ('meshcolor_maps', lambda b: dict(color_maps=[b.color_maps[0], b.color_maps[1][:3].contiguous()]), 'color_map'),
    'meshcolor_blend-select': ('meshcolor_blend', lambda b: dict(select='mean'), 'select'),
    'meshcolor_blend-fill2': ('meshcolor_blend', lambda b: dict(fill=(0.5, 0.5)), 'fill'),
    'meshcolor_blend-facing_without_normals': ('meshcolor_blend', lambda b: dict(normals=None), 'facing needs normals'),
    'meshcolor_blend-one_size_short': ('meshcolor_blend', lambda b: dict(sizes=b.sizes[:1]), 'views'),
    'meshtex_uv-over_capacity': ('meshtex_uv', lambda b: dict(n_faces=513), 'faces'),
    'meshtex_uv-small_atlas': ('meshtex_uv', lambda b: dict(size=32), 'size'),
    'meshtex_uv-large_atlas': ('meshtex_uv', lambda b: dict(size=16385), 'size'),
    'meshtex_uv-small_tile': ('meshtex_uv', lambda b: dict(tile=3), 'tile'),
    'meshtex_uv-negative_faces': ('meshtex_uv', lambda b: dict(n_faces=-1), 'faces'),
    'meshtex_uv-cpu': ('meshtex_uv', lambda b: dict(device='cpu'), 'device'),
    'meshtex_points-over_capacity': ('meshtex_points', lambda b: dict(tile=64), 'faces'),
    'meshtex_points-tile_over_size': ('meshtex_points', lambda b: dict(tile=65), 'tile'),
    'meshtex_bake-over_capacity': ('meshtex_bake', lambda b: dict(tile=64), 'faces'),
    'meshtex_bake-small_atlas': ('meshtex_bake', lambda b: dict(size=63), 'size'),
    'meshtex_bake-select': ('meshtex_bake', lambda b: dict(select='mean'), 'select'),
    'meshtex_bake-fill2': ('meshtex_bake', lambda b: dict(fill=(0.5, 0.5)), 'fill'),
    'meshtex_bake-one_size_short': ('meshtex_bake', lambda b: dict(sizes=b.sizes[:1]), 'views'),
    'meshray_grid_count-dims2': ('meshray_grid_count', lambda b: dict(dims=N3[:2]), 'dims'),
    'meshray_grid_count-origin2': ('meshray_grid_count', lambda b: dict(origin=LO[:2]), 'origin'),
    'meshray_grid_count-no_cell': ('meshray_grid_count', lambda b: dict(dims=(2, 0, 2)), 'cells'),
    'meshray_grid_count-too_many_cells': ('meshray_grid_count', lambda b: dict(dims=(512, 512, 65)), 'more than 2^24 cells'),
    'meshray_grid_write-dims2': ('meshray_grid_write', lambda b: dict(dims=N3[:2]), 'dims'),
    'meshray_grid_write-too_many_cells': ('meshray_grid_write', lambda b: dict(dims=(1 << 24, 2, 1)), 'more than 2^24 cells'),
    'meshray_grid_write-other_grid': ('meshray_grid_write', lambda b: dict(dims=(2, 2, 3)), 'counts'),
    'meshray_cast-dims2': ('meshray_cast', lambda b: dict(dims=N3[:2]), 'dims'),
    'meshray_cast-no_cell': ('meshray_cast', lambda b: dict(dims=(0, 2, 2)), 'cells'),
    'meshray_cast-other_grid': ('meshray_cast', lambda b: dict(dims=(2, 2, 1)), 'offsets'),
    'meshray_cast-one_direction_short': ('meshray_cast', lambda b: dict(rays_d=b.rays_d[:2].contiguous()), 'rays_d'),
    'meshray_occluded-dims2': ('meshray_occluded', lambda b: dict(dims=N3[:2]), 'dims'),
    'meshray_occluded-too_many_cells': ('meshray_occluded', lambda b: dict(dims=(256, 256, 257)), 'more than 2^24 cells'),
    'meshray_occluded-65': ('meshray_occluded', lambda b: dict(centres=torch.zeros(65, 3, device='cuda')), '65 views are more than 64'),
}


# ---- accepted calls beside the plain ones: (binding, changed arguments, the outputs when they are not the plain rule's) ---------------------
def _strided(t):
    return torch.stack([t, t], dim=-1)[..., 0]


QUIRKS = {
    'meshcc_filter_count-strided_bool_keep': ('meshcc_filter_count', lambda b: dict(keep=_strided(b.keep))),
    'meshcc_filter_write-strided_uint8_keep': ('meshcc_filter_write', lambda b: dict(keep=_strided(b.keep.to(U8)))),
    'meshvis_filter_count-strided_uint8_keep': ('meshvis_filter_count', lambda b: dict(face_keep=_strided(b.face_keep), counts=None)),
    'meshvis_filter_write-strided_bool_keep': ('meshvis_filter_write', lambda b: dict(face_keep=_strided(b.face_keep.bool()))),
    'meshcc_stats-no_vertices': ('meshcc_stats', lambda b: dict(vertices=None)),
    'meshcc_filter_write-no_vertices': ('meshcc_filter_write', lambda b: dict(vertices=None)),
    'meshvis_filter_write-no_vertices': ('meshvis_filter_write', lambda b: dict(vertices=None)),
    'meshvis_vertex_bits-no_views_on_the_host': ('meshvis_vertex_bits', lambda b: dict(views=b.views0, sizes=[])),
    'meshvis_face_keep-no_views_on_the_host': ('meshvis_face_keep', lambda b: dict(centres=torch.zeros(0, 3), flag=None)),
    'meshray_occluded-no_views_on_the_host': ('meshray_occluded', lambda b: dict(centres=torch.zeros(0, 3))),
    'meshcolor_blend-no_views_on_the_host': ('meshcolor_blend', lambda b: dict(views=b.views0, sizes=[], map_pointers=b.pointers0)),
    'meshtex_bake-no_views_on_the_host': ('meshtex_bake', lambda b: dict(views=b.views0, sizes=[], map_pointers=b.pointers0)),
    'meshcolor_blend-not_facing_no_normals': ('meshcolor_blend', lambda b: dict(normals=None, facing=False)),
    'meshcolor_blend-not_facing_normals_unread': ('meshcolor_blend', lambda b: dict(normals=torch.zeros(7), facing=False)),
    'meshcolor_blend-best_no_fallback': ('meshcolor_blend', lambda b: dict(select='best', fallback=None)),
    'meshtex_bake-no_normals': ('meshtex_bake', lambda b: dict(normals=None, fallback=None, flag=None)),
    'meshtex_points-no_normals': ('meshtex_points', lambda b: dict(normals=None, flag=None)),
    'meshsimp_place-member': ('meshsimp_place', lambda b: dict(placement='member')),
    'meshsimp_faces-no_dedupe': ('meshsimp_faces', lambda b: dict(dedupe=None, flag=None)),
    'meshsimp_cluster-own_counts': ('meshsimp_cluster', lambda b: dict(counts=None)),
    'meshquadric_sums-own_flags': ('meshquadric_sums', lambda b: dict(flags=None)),
    'meshcolor_normal_sums-own_flag': ('meshcolor_normal_sums', lambda b: dict(flag=None)),
    'meshray_grid_count-own_flag': ('meshray_grid_count', lambda b: dict(flag=None)),
    'meshray_cast-any_hit': ('meshray_cast', lambda b: dict(any_hit=True), lambda k: [(U8, (3,))]),
    'meshray_cast-no_uv': ('meshray_cast', lambda b: dict(uv=False), lambda k: [(F32, (3,)), (I32, (3,)), None, None]),
    'meshcolor_maps-converted': ('meshcolor_maps', lambda b: dict(color_maps=[b.color_maps[0].double(), _strided(b.color_maps[1])])),
}
EMPTY = {
    'brickmesh_list': ('brickmesh_list', lambda b: dict(table=b.no_bricks, n_bricks=0)),
    'brickmesh_corners': ('brickmesh_corners', lambda b: dict(ids=b.i0, m=0)),
    'brickmesh_count': ('brickmesh_count', lambda b: dict(values=b.d0.float(), ids=b.i0, table=b.no_bricks)),
    'meshcc_label': ('meshcc_label', lambda b: dict(faces=b.f0, n_vertices=0)),
    'meshcc_stats': ('meshcc_stats', lambda b: dict(faces=b.f0, vertex_component=b.i0, n_components=0, vertices=b.v0)),
    'meshcc_filter_count': ('meshcc_filter_count', lambda b: dict(faces=b.f0, vertex_component=b.i0, keep=b.u0)),
    'meshvis_views': ('meshvis_views', lambda b: dict(poses=[], maps=[])),
    'meshvis_vertex_bits': ('meshvis_vertex_bits', lambda b: dict(vertices=b.v0)),
    'meshvis_face_keep': ('meshvis_face_keep', lambda b: dict(faces=b.f0, vertices=b.v0, visible_bits=b.l0, free_bits=b.l0)),
    'meshvis_filter_count': ('meshvis_filter_count', lambda b: dict(faces=b.f0, n_vertices=0, face_keep=b.u0)),
    'meshsimp_bounds': ('meshsimp_bounds', lambda b: dict(vertices=b.v0)),
    'meshsimp_cluster': ('meshsimp_cluster', lambda b: dict(vertices=b.v0, n_faces=0)),
    'meshsimp_place': ('meshsimp_place', lambda b: dict(vertices=b.v0, vertex_cluster=b.i0, n_clusters=0)),
    'meshsimp_faces': ('meshsimp_faces', lambda b: dict(faces=b.f0, vertex_cluster=b.i0)),
    'meshquadric_sums': ('meshquadric_sums', lambda b: dict(vertices=b.v0, faces=b.f0, vertex_cluster=b.i0, n_clusters=0)),
    'meshquadric_place': ('meshquadric_place', lambda b: dict(anchor=b.v0, representative=b.i0, acc=b.quadrics[:0].contiguous())),
    'meshcolor_normal_sums': ('meshcolor_normal_sums', lambda b: dict(vertices=b.v0, faces=b.f0)),
    'meshcolor_normals': ('meshcolor_normals', lambda b: dict(acc=b.normal_sums[:0].contiguous())),
    'meshcolor_maps': ('meshcolor_maps', lambda b: dict(color_maps=[], sizes=[])),
    'meshcolor_blend': ('meshcolor_blend', lambda b: dict(vertices=b.v0, normals=b.v0, fallback=b.v0)),
    'meshtex_uv': ('meshtex_uv', lambda b: dict(n_faces=0)),
    'meshtex_points': ('meshtex_points', lambda b: dict(vertices=b.v0, faces=b.f0, normals=b.v0)),
    'meshtex_bake': ('meshtex_bake', lambda b: dict(vertices=b.v0, faces=b.f0, normals=b.v0, fallback=b.v0)),
    'meshray_grid_count': ('meshray_grid_count', lambda b: dict(vertices=b.v0, faces=b.f0)),
    'meshray_grid_write': ('meshray_grid_write', lambda b: dict(vertices=b.v0, faces=b.f0, counts=torch.zeros_like(b.cell_counts), offsets=torch.zeros_like(b.offsets), n_refs=0)),
    'meshray_cast': ('meshray_cast', lambda b: dict(rays_o=b.v0, rays_d=b.v0)),
    'meshray_cast_of_no_mesh': ('meshray_cast', lambda b: dict(vertices=b.v0, faces=b.f0, offsets=torch.zeros_like(b.offsets), refs=b.i0)),
    'meshray_occluded': ('meshray_occluded', lambda b: dict(vertices=b.v0, faces=b.f0, offsets=torch.zeros_like(b.offsets), refs=b.i0, mask_bits=b.l0)),
    'brickmesh_write': ('brickmesh_write', lambda b: dict(values=b.d0.float(), ids=b.i0, table=b.no_bricks, ws=b.brick_ws0, n_vertices=0, n_faces=0)),
    'meshcc_filter_write': ('meshcc_filter_write', lambda b: dict(faces=b.f0, vertex_component=b.i0, keep=b.u0, ws=b.cc_ws0, n_vertices_kept=0, n_faces_kept=0, vertices=b.v0)),
    'meshcc_filter_write_without_vertices': ('meshcc_filter_write', lambda b: dict(faces=b.f0, vertex_component=b.i0, keep=b.u0, ws=b.cc_ws0, n_vertices_kept=0, n_faces_kept=0,
                                                                                   vertices=None)),
    'meshvis_filter_write': ('meshvis_filter_write', lambda b: dict(faces=b.f0, n_vertices=0, face_keep=b.u0, ws=b.vis_ws0, n_vertices_kept=0, n_faces_kept=0, vertices=b.v0)),
    'meshvis_filter_write_without_vertices': ('meshvis_filter_write', lambda b: dict(faces=b.f0, n_vertices=0, face_keep=b.u0, ws=b.vis_ws0, n_vertices_kept=0, n_faces_kept=0,
                                                                                     vertices=None)),
    # an empty tensor of another dtype, where the library gets NULL for it and the dtype was never looked at
    'brickmesh_corners_ids_of_another_dtype': ('brickmesh_corners', lambda b: dict(ids=b.l0, m=0)),
    'brickmesh_count_of_another_dtype': ('brickmesh_count', lambda b: dict(values=b.d0, ids=b.l0, table=b.no_bricks)),
    'brickmesh_write_of_another_dtype': ('brickmesh_write', lambda b: dict(values=b.d0, ids=b.l0, table=b.no_bricks, ws=b.brick_ws0, n_vertices=0, n_faces=0)),
    'meshvis_vertex_bits_of_another_dtype': ('meshvis_vertex_bits', lambda b: dict(vertices=b.v0.double())),
}


CALLS = []
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mesh_binding_calls.json')


def described_call(kwargs, out):
    """The calls of CALLS in words that do not change from run to run: a pointer is None when it is NULL, else the name of the argument
    or the place of the output whose memory it is, else '<new>' (a buffer of the binding's own, or a converted copy); the byte count
    after a workspace's pointer is '<its bytes>'; arrays are lists; counts and scalars are themselves."""
    tensors = {f'out{i}': t for i, t in enumerate(out) if torch.is_tensor(t)}
    tensors.update({k: t for k, t in kwargs.items() if torch.is_tensor(t)})          # (a flag passed in and handed back is the argument)
    owner = {t.data_ptr(): (k, t) for k, t in tensors.items() if t.numel()}
    calls = []
    for name, args in CALLS:
        words, last = [], None
        for a in args:
            if isinstance(a, ctypes.c_void_p):
                last = owner.get(a.value) if a.value else None
                words.append(None if not a.value else f'<{last[0]}>' if last else '<new>')
                continue
            if last is not None and last[1].dtype == I64 and last[1].dim() == 1 and a == last[1].numel() * 8 and not isinstance(a, bool):
                words.append('<its bytes>')
            else:
                words.append(list(a) if isinstance(a, ctypes.Array) else a if a is None or isinstance(a, (int, float)) else type(a).__name__)
            last = None
        calls.append([name, words])
    return calls


# ---- the checks -------------------------------------------------------------------------------------------------------------------------------
def run(monkeypatch, fn, kwargs, through):
    """Call the binding with a recorder in perf_amd._lib.call's place -> (outputs, the entry points it saw); the calls with their
    arguments are left in CALLS."""
    from perf_amd import _lib, ops
    seen, real = [], _lib.call
    del CALLS[:]

    def recorder(name, *args):
        seen.append(name)
        CALLS.append((name, args))
        if through:
            real(name, *args)
    monkeypatch.setattr(_lib, 'call', recorder)
    try:
        out = getattr(ops, fn)(**kwargs)
    finally:
        monkeypatch.setattr(_lib, 'call', real)
    return (out if isinstance(out, tuple) else (out,)), seen


def outcome(monkeypatch, fn, kwargs, word):
    """What a wrong form met: 'refused', 'unnamed' (a PerfError without the word), the name of another exception, or 'accepted'; with the
    entry points seen."""
    from perf_amd._lib import PerfError
    seen = []
    try:
        _, seen = run(monkeypatch, fn, kwargs, through=False)
    except PerfError as e:
        return ('refused' if word in str(e) else 'unnamed'), seen, str(e)
    except Exception as e:          # noqa: BLE001 (the table records which)
        return type(e).__name__, seen, str(e)
    return 'accepted', seen, ''


def check_outputs(fn, kwargs, out, want=None):
    full = SPECS[fn][1](base())
    full.update(kwargs)
    want = (want or SPECS[fn][3])(full)
    assert len(out) == len(want), (fn, len(out), len(want))
    for got, w in zip(out, want):
        if w is None:
            assert got is None, fn
        elif w is list:
            assert isinstance(got, list), fn
        elif w == WS:          # (the one passed in when it serves, whatever it is; else a new one)
            assert got is full.get('ws') or (got.is_cuda and got.dtype == I64 and got.dim() == 1), fn
        else:
            assert torch.is_tensor(got) and got.is_cuda and (got.dtype, tuple(got.shape)) == w, (fn, got.dtype, tuple(got.shape), w)


def accept(monkeypatch, fn, kwargs, through, want=None, key=None):
    full = SPECS[fn][1](base())
    full.update(kwargs)
    out, seen = run(monkeypatch, fn, full, through)
    assert seen == ([SPECS[fn][0]] if SPECS[fn][0] else []), (fn, seen)
    check_outputs(fn, kwargs, out, want)
    calls = described_call(full, out)
    if key is not None:          # the call the earlier bindings made of the same arguments
        assert calls == json.load(open(GOLDEN))[key], (key, calls)
    return calls


@pytest.mark.parametrize('case', list(tensor_cases()))
def test_a_tensor_in_a_wrong_form(case, monkeypatch):
    fn, kwargs, word = case_call(case)
    if case in NOT_REFUSED:
        out, seen = run(monkeypatch, fn, kwargs, through=False)
        assert seen == ([SPECS[fn][0]] if SPECS[fn][0] else []), (case, seen)
        check_outputs(fn, kwargs, out)
        return
    what, seen, message = outcome(monkeypatch, fn, kwargs, word)
    assert not seen, (case, seen)
    if case in UNNAMED:
        assert what in ('refused', 'unnamed'), (case, what, message)
    else:          # (NOT_A_PERFERROR: what the case met before; a PerfError that names the argument now)
        assert what == 'refused', (case, what, message)


@pytest.mark.parametrize('case', list(OTHER_REFUSALS))
def test_an_argument_outside_its_range(case, monkeypatch):
    fn, changed, word = OTHER_REFUSALS[case]
    kwargs = SPECS[fn][1](base())
    kwargs.update(changed(base()))
    what, seen, message = outcome(monkeypatch, fn, kwargs, word)
    assert what == 'refused' and not seen, (case, what, seen, message)


@pytest.mark.parametrize('fn', list(SPECS))
def test_a_plain_call(fn, monkeypatch):
    accept(monkeypatch, fn, {}, through=True, key='plain ' + fn)


@pytest.mark.parametrize('case', list(QUIRKS))
def test_a_documented_form(case, monkeypatch):
    fn, changed, *want = QUIRKS[case]
    accept(monkeypatch, fn, changed(base()), through=True, want=want[0] if want else None, key='form ' + case)


@pytest.mark.parametrize('case', list(EMPTY))
def test_an_empty_input(case, monkeypatch):
    fn, changed = EMPTY[case]
    accept(monkeypatch, fn, changed(base()), through=True, key='empty ' + case)
