"""Write the trained density as a triangle mesh (binary PLY; with --texture, OBJ + MTL + the atlas image): trains the synthetic room, or loads a checkpoint of NeRFScene.state_dict().

  python tools/extract_mesh.py --out room.ply [--resolution 256] [--threshold T] [--no-occupancy] [--no-colors] [--no-normals] [--sparse]
                               [--seen-by-panoramas [--occlusion] [--visibility-tol T] [--carve] [--sup-pool pool.pt]]
                               [--min-component-faces N] [--keep-largest K] [--orientation inward|outward]
                               [--simplify-cell H | --simplify-tolerance E] [--simplify-placement mean|member|quadric]
                               [--simplify-dedupe oriented|unoriented|none] [--report-deviation]
                               [--colors-from-panoramas [--color-select blend|best] [--color-power N] [--sup-pool pool.pt]]
                               [--texture SIZE [--texture-source panoramas|field] [--texture-tile T]]
                               [--checkpoint scene.pt | --geo 3000 --app 1500] [--dtype fp16]

Prints one JSON line: the counts, the threshold and the seconds of training and extraction."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from perf_amd import synthetic
from perf_amd.mesh import write_obj, write_ply
from perf_amd.scene import NeRFScene, SupInfoPool, gen_pano_rays

ap = argparse.ArgumentParser()
ap.add_argument('--out', required=True)
ap.add_argument('--resolution', type=int, default=256)
ap.add_argument('--threshold', type=float, default=None, help='default: ln 2 / render_step_size')
ap.add_argument('--no-occupancy', action='store_true', help='keep the density where the occupancy grid is empty (the field is untrained there)')
ap.add_argument('--sparse', action='store_true', help='evaluate and mesh only the lattice bricks that touch the occupancy shell (resolutions up to 4096, a multiple of 8)')
ap.add_argument('--no-colors', action='store_true')
ap.add_argument('--no-normals', action='store_true')
ap.add_argument('--min-component-faces', type=int, default=0, help='drop the connected components with fewer faces (floaters)')
ap.add_argument('--keep-largest', type=int, default=None, help='keep only this many components, the ones with the most faces')
ap.add_argument('--orientation', choices=['inward', 'outward'], default=None,
                help='keep the closed components whose normals point into (inward: a room seen from inside) or out of the volume they enclose')
ap.add_argument('--seen-by-panoramas', action='store_true',
                help='drop the faces no registered panorama saw (depth test per vertex, facing test per face), before the component cleaning')
ap.add_argument('--visibility-tol', type=float, default=1 / 256, help='the band of the depth test of --seen-by-panoramas, in scene units')
ap.add_argument('--carve', action='store_true', help='with --seen-by-panoramas: also drop the faces with a vertex in observed free space, in front of a stored surface by more than '
                                                       '--visibility-tol (a skin that sits further inside the room than that is carved with the floaters: widen the band)')
ap.add_argument('--occlusion', action='store_true', help='with --seen-by-panoramas: also test each vertex against the mesh itself (a view does not see through the front skin)')
ap.add_argument('--sup-pool', default=None, help='with --checkpoint and --seen-by-panoramas: a torch.save of SupInfoPool.state_dict()')
ap.add_argument('--simplify-cell', type=float, default=None,
                help='after the cleaning: one vertex per occupied cell of this edge (scene units) of the grid over the scene box (vertex clustering)')
ap.add_argument('--simplify-placement', choices=['mean', 'member', 'quadric'], default='mean',
                help='the vertex of a cell: the mean of its vertices, the one of them nearest the mean (no shrinkage), or the point of the cell nearest the planes of '
                     'their faces (quadric error: edges and corners stay sharp)')
ap.add_argument('--simplify-dedupe', choices=['oriented', 'unoriented', 'none'], default='oriented',
                help='of the faces that become equal up to rotation (oriented) or as sets (unoriented: a double skin thinner than a cell) one stays')
ap.add_argument('--colors-from-panoramas', action='store_true',
                help='after the cull and the cleaning, before the simplification: the vertex colours are the registered panoramas\' own, weighted by '
                     'cos^N / dist^2 over the views that saw a vertex (the field\'s colours stay where none did)')
ap.add_argument('--color-select', choices=['blend', 'best'], default='blend', help='with --colors-from-panoramas: the weighted mean of the views, or the best view alone')
ap.add_argument('--color-power', type=int, default=2, help='with --colors-from-panoramas: the power N of the incidence cosine, 1 .. 8')
ap.add_argument('--texture', type=int, default=None, metavar='SIZE',
                help='after the simplification: bake a SIZE x SIZE texture atlas (two faces per tile) and write --out as OBJ + MTL + image, not PLY')
ap.add_argument('--texture-source', choices=['panoramas', 'field'], default='panoramas',
                help='with --texture: the registered panoramas blended as --colors-from-panoramas blends them at every texel, or the field\'s own colours')
ap.add_argument('--texture-tile', type=int, default=None, help='with --texture: the tile edge in texels (default: the largest that holds the faces)')
ap.add_argument('--simplify-tolerance', type=float, default=None, metavar='E',
                help='instead of --simplify-cell: the coarsest cell of a ladder (from 16 median edge lengths down, each 1/sqrt(2) of the one before) whose sampled '
                     'deviation from the cleaned mesh stays within E scene units')
ap.add_argument('--report-deviation', action='store_true',
                help='print the sampled deviation (max, mean, rms, p90 of the closest-point distances, both directions) of every stage\'s output from the stage '
                     'before it: cull, cleaning, simplification')
ap.add_argument('--checkpoint', default=None, help='a torch.save of NeRFScene.state_dict()')
ap.add_argument('--geo', type=int, default=3000)
ap.add_argument('--app', type=int, default=1500)
ap.add_argument('--batch', type=int, default=4096)
ap.add_argument('--dtype', default='fp16')
args = ap.parse_args()
if args.simplify_cell is not None and args.simplify_tolerance is not None:
    ap.error('--simplify-cell and --simplify-tolerance are exclusive: the cell is given, or found for the tolerance')

torch.manual_seed(0); np.random.seed(0)
scene = NeRFScene(dtype=args.dtype)
t0 = time.perf_counter()
views = None          # --seen-by-panoramas: the registered panoramas the mesh is tested against
with_views = args.seen_by_panoramas or args.colors_from_panoramas or (args.texture is not None and args.texture_source == 'panoramas')
if with_views and args.checkpoint and not args.sup_pool:
    ap.error('--seen-by-panoramas and --colors-from-panoramas with --checkpoint need the panoramas: --sup-pool FILE, a torch.save of SupInfoPool.state_dict()')
if args.checkpoint:
    scene.load_state_dict(torch.load(args.checkpoint, map_location='cuda'))
    if with_views:
        views = SupInfoPool(); views.load_state_dict(torch.load(args.sup_pool, map_location='cuda'))
else:
    rays = gen_pano_rays(torch.eye(4), 256, 512)
    dist, rgb = synthetic.room(rays.d)
    pool = SupInfoPool(); pool.register_rays(rays.o, rays.d, rgb, dist)
    if with_views:          # (register_rays leaves no sup_infos: the view is the pose, the distance map the scene trains on and its colours)
        views = [{'pose': torch.eye(4), 'distance_map': dist.reshape(256, 512).float().to('cuda'), 'color_map': rgb.reshape(256, 512, 3).float().to('cuda')}]
    scene.train_conf.pixel_loss_batch_size = args.batch
    scene.train_one_episode(pool, args.geo, args.app)
scene.set_eval()
torch.cuda.synchronize(); t1 = time.perf_counter()
if args.sparse:
    if args.no_occupancy:
        ap.error('--sparse meshes the occupancy shell: it cannot go with --no-occupancy')
    mesh = scene.extract_mesh_sparse(resolution=args.resolution, threshold=args.threshold, colors=not args.no_colors, normals=not args.no_normals)
else:
    mesh = scene.extract_mesh(resolution=args.resolution, threshold=args.threshold, use_occupancy=not args.no_occupancy, colors=not args.no_colors,
                              normals=not args.no_normals)
torch.cuda.synchronize(); t2 = time.perf_counter()
extracted = (len(mesh.vertices), len(mesh.faces))
deviations = {}          # --report-deviation: stage -> the deviation of its output from its input


def report(stage, before, after, known=None):
    if args.report_deviation and len(before.faces) and len(after.faces):
        d = known if known is not None else scene.mesh_deviation(after, before)
        deviations[stage] = {k: getattr(d, k) for k in ('max', 'mean', 'rms', 'p90', 'argmax_point', 'n_samples', 'n_beyond')}
    return after


if args.seen_by_panoramas:          # first the faces no panorama saw, then the components of what is left
    if args.occlusion:          # (the depth test against the panoramas and the segment test against the mesh itself)
        mesh = report('cull', mesh, scene.cull_occluded_mesh(mesh, views, tol=args.visibility_tol, carve=args.carve))
    else:
        mesh = report('cull', mesh, scene.cull_unseen_mesh(mesh, views, tol=args.visibility_tol, carve=args.carve))
seen = {'seen_vertices': len(mesh.vertices), 'seen_faces': len(mesh.faces)} if args.seen_by_panoramas else {}
if args.min_component_faces > 0 or args.keep_largest is not None or args.orientation is not None:          # after either extraction path
    mesh = report('clean', mesh, scene.clean_mesh(mesh, min_faces=args.min_component_faces, keep_largest=args.keep_largest, orientation=args.orientation))
if args.colors_from_panoramas:          # on the fine vertices, which lie on the surface the depth test was made for; the simplification carries the colours
    mesh = scene.color_mesh_from_panoramas(mesh, views, tol=args.visibility_tol, select=args.color_select, power=args.color_power)
cleaned = {'cleaned_vertices': len(mesh.vertices), 'cleaned_faces': len(mesh.faces)} if args.simplify_cell is not None or args.simplify_tolerance is not None else {}
if args.simplify_cell is not None:          # last: the cull and the cleaning have seen the mesh as it was extracted
    mesh = report('simplify', mesh, scene.simplify_mesh(mesh, args.simplify_cell, placement=args.simplify_placement,
                                                        dedupe=None if args.simplify_dedupe == 'none' else args.simplify_dedupe))
elif args.simplify_tolerance is not None:          # the cell is found: the coarsest of the ladder within the tolerance
    small, found_cell, deviation = scene.simplify_mesh_to_tolerance(mesh, args.simplify_tolerance, placement=args.simplify_placement,
                                                                    dedupe=None if args.simplify_dedupe == 'none' else args.simplify_dedupe)
    cleaned['simplify_cell'] = found_cell
    mesh = report('simplify', mesh, small, deviation)
textured = {}
if args.texture is not None:          # after the simplification: the small mesh carries as many colour samples as the atlas has texels
    if args.texture_source == 'panoramas':
        atlas = scene.bake_mesh_texture(mesh, views, size=args.texture, tile=args.texture_tile, tol=args.visibility_tol, select=args.color_select, power=args.color_power)
    else:
        atlas = scene.bake_mesh_texture(mesh, None, size=args.texture, tile=args.texture_tile)
    textured = {'texture': atlas.size, 'texture_tile': atlas.tile, 'texture_source': args.texture_source}
torch.cuda.synchronize(); t3 = time.perf_counter()
if args.texture is not None:
    args.out = os.path.splitext(args.out)[0] + '.obj'
    textured['texture_image'] = write_obj(args.out, mesh, atlas)
else:
    write_ply(args.out, mesh)
print(json.dumps({'out': args.out, 'vertices': len(mesh.vertices), 'faces': len(mesh.faces), 'resolution': args.resolution, 'sparse': args.sparse,
                  'threshold': args.threshold, 'extracted_vertices': extracted[0], 'extracted_faces': extracted[1], **seen, **cleaned, **textured, **({'deviation': deviations} if args.report_deviation else {}), 'prepare_s': t1 - t0, 'extract_s': t2 - t1, 'clean_s': t3 - t2, 'bytes': os.path.getsize(args.out)}))
