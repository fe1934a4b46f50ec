"""ctypes binding of libperf_hip.so (the C ABI declared in include/perf_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a call fails, this
module raises.  Build the library with `python -m perf_amd.build` (or __graft_entry__.build()).
"""
import ctypes
import os
from collections import namedtuple
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libperf_hip.so')

ABI_VERSION = 16         # PERF_ABI_VERSION of include/perf_hip.h this binding was written against
EXT_ABI_VERSION = 1      # PERF_EXT_ABI_VERSION of include/perf_hip_ext.h (entry points added after perf_hip.h was frozen)
SPHERE_ABI_VERSION = 1   # PERF_SPHERE_ABI_VERSION of include/perf_hip_sphere.h (the sphere distance field)
PAIR_ABI_VERSION = 1     # PERF_PAIR_ABI_VERSION of include/perf_hip_pair.h (the pair table of two fields with one grid geometry)
JOINT_ABI_VERSION = 1    # PERF_JOINT_ABI_VERSION of include/perf_hip_joint.h (the joint predictor's alignment step)
MESH_ABI_VERSION = 1     # PERF_MESH_ABI_VERSION of include/perf_hip_mesh.h (surface nets on a dense lattice)
BRICKMESH_ABI_VERSION = 1    # PERF_BRICKMESH_ABI_VERSION of include/perf_hip_brickmesh.h (surface nets on the live bricks of a lattice)
MESHCC_ABI_VERSION = 1       # PERF_MESHCC_ABI_VERSION of include/perf_hip_meshcc.h (connected components of a triangle mesh)
MESHVIS_ABI_VERSION = 1      # PERF_MESHVIS_ABI_VERSION of include/perf_hip_meshvis.h (cull the mesh faces no registered panorama saw)
MESHSIMP_ABI_VERSION = 1     # PERF_MESHSIMP_ABI_VERSION of include/perf_hip_meshsimp.h (simplify a mesh by vertex clustering)
MESHCOLOR_ABI_VERSION = 1    # PERF_MESHCOLOR_ABI_VERSION of include/perf_hip_meshcolor.h (colour a mesh from the registered panoramas; normals from faces)
MESHRAY_ABI_VERSION = 1      # PERF_MESHRAY_ABI_VERSION of include/perf_hip_meshray.h (rays against a mesh on a uniform grid: closest hit, any hit, occlusion)
MESHTEX_ABI_VERSION = 1      # PERF_MESHTEX_ABI_VERSION of include/perf_hip_meshtex.h (a texture atlas for a mesh, baked from the registered panoramas)
MESHQUADRIC_ABI_VERSION = 1  # PERF_MESHQUADRIC_ABI_VERSION of include/perf_hip_meshquadric.h (quadric error placement of a simplified mesh's vertices, sums in fixed point)
MESHNEAR_ABI_VERSION = 1     # PERF_MESHNEAR_ABI_VERSION of include/staged/perf_hip_meshnear.h (the closest point of a mesh to each query point; a staged unit)
RIDERS_ABI_VERSION = 1       # PERF_RIDERS_ABI_VERSION of include/perf_hip_riders.h (the next batch's front end riding in the backward's launches)
MAX_LEVELS = 24
DTYPE_BF16, DTYPE_FP16 = 0, 1
ACT_NONE, ACT_SIGMOID, ACT_EXP = 0, 1, 2
INTERP_LINEAR, INTERP_SMOOTHSTEP = 0, 1
LAYOUT_TCNN, LAYOUT_LINE_LOCAL, LAYOUT_LINE_OVERLAP = 0, 1, 2
LATTICE = {'single': 0, 'repeated': 1, None: 1}          # PERF_LATTICE_*; None = the default
DEFAULT_LATTICE = 'repeated'                 # t_{k+1} = fl(t_k + step): how nerfacc's traverse_grids is understood to march (include/perf_hip.h)


class GridDesc(Structure):
    _fields_ = [('n_levels', c_int32), ('interpolation', c_int32),
                ('scale', c_float * MAX_LEVELS), ('res', c_uint32 * MAX_LEVELS), ('size', c_uint32 * MAX_LEVELS),
                ('offset', c_uint64 * MAX_LEVELS), ('hashed', c_uint32 * MAX_LEVELS),
                ('layout', c_int32), ('sb_shift', c_uint32 * 3), ('local', c_uint32 * MAX_LEVELS), ('nsx', c_uint32 * MAX_LEVELS),
                ('nsxy', c_uint32 * MAX_LEVELS)]


class MlpDesc(Structure):
    _fields_ = [('n_levels', c_int32), ('n_hidden_layers', c_int32), ('n_out', c_int32), ('out_act', c_int32),
                ('exp_shift', c_float)]


class StepBook(Structure):       # perf_step_book: the arguments of perf_step_bookkeeping as a POD block (perf_field_bwd_book)
    _fields_ = [('step_dev', c_void_p), ('gate_dev', c_void_p), ('counters', c_void_p), ('n_marched_dev', c_void_p), ('n_kept_dev', c_void_p),
                ('capacity', c_int64), ('overflow_flag', c_void_p), ('remote_flags', c_void_p), ('eff_gate_out', c_void_p),
                ('schedule', c_void_p), ('iter_dev', c_void_p), ('lr_out', c_void_p), ('ratio_out', c_void_p), ('n_schedule', c_int32),
                ('overflow_redone', c_int32)]


# include/perf_hip_riders.h: the argument blocks of the three rider stages (field for field)
class RiderDraw(Structure):      # perf_rider_draw
    _fields_ = [('seed', c_uint64), ('counter_dev', c_void_p), ('ticket', c_void_p), ('pool_lo', c_int64), ('pool_hi', c_int64), ('n_local', c_int64),
                ('first_global', c_int64), ('o_all', c_void_p), ('d_all', c_void_p), ('color_all', c_void_p), ('dist_all', c_void_p), ('normal_all', c_void_p),
                ('o', c_void_p), ('d', c_void_p), ('color', c_void_p), ('dist', c_void_p), ('normal', c_void_p), ('indices_out', c_void_p),
                ('jitter', c_void_p), ('noise', c_void_p), ('bg', c_void_p), ('t0_scale', c_float), ('t0_base', c_float), ('step', c_float),
                ('max_steps', c_int32), ('runs', c_void_p), ('marched_live', c_void_p), ('marched_keep', c_void_p)]


class RiderCount(Structure):     # perf_rider_count
    _fields_ = [('rays_o', c_void_p), ('rays_d', c_void_p), ('t0', c_void_p), ('t0_scale', c_float), ('t0_base', c_float), ('n_rays', c_int64),
                ('occ_bits', c_void_p), ('occ_coarse', c_void_p), ('res', c_int32), ('aabb', c_float * 6), ('far_plane', c_float), ('step', c_float),
                ('max_steps', c_int32), ('runs', c_void_p), ('masks', c_void_p), ('counts', c_void_p)]


class RiderWrite(Structure):     # perf_rider_write
    _fields_ = [('t0', c_void_p), ('t0_scale', c_float), ('t0_base', c_float), ('n_rays', c_int64), ('step', c_float), ('max_steps', c_int32),
                ('runs', c_void_p), ('masks', c_void_p), ('counts', c_void_p), ('offsets', c_void_p), ('total', c_void_p), ('capacity', c_int64),
                ('ray_indices', c_void_p), ('t_starts', c_void_p), ('t_ends', c_void_p), ('packed_info', c_void_p), ('rays_o', c_void_p),
                ('rays_d', c_void_p), ('points_aabb', c_float * 6), ('x01', c_void_p), ('sel', c_void_p)]


class PerfError(RuntimeError):
    pass


P = c_void_p
LOSS_SCALARS = 256       # PERF_LOSS_SCALARS
STEP_COUNTERS = 8        # PERF_STEP_COUNTERS
HEADROOM_STATE_WORDS = 2 * MAX_LEVELS + 8    # PERF_HEADROOM_STATE_WORDS
DP_STATS = 64            # PERF_DP_STATS
DP_SLOT = 80             # PERF_DP_SLOT
_SIGS = {
    'perf_version': (c_int, []),
    'perf_last_error': (c_char_p, []),
    'perf_sizeof_grid_desc': (c_int64, []),
    'perf_sizeof_mlp_desc': (c_int64, []),
    'perf_sizeof_step_book': (c_int64, []),
    'perf_cast_params': (c_int, [P, P, c_int64, c_int, P]),
    'perf_adam_step': (c_int, [P, P, P, P, P, c_int64, c_int, c_int32, c_float, c_float, c_float, c_float, c_int, P]),
    'perf_adam_step_dev': (c_int, [P, P, P, P, P, c_int64, c_int, P, P, P, c_float, c_float, c_float, c_int, P, P]),
    'perf_step_bookkeeping': (c_int, [P, P, P, P, P, c_int64, P, P, c_int32, P, P, c_int32, P, P, P, P]),
    'perf_points_from_rays': (c_int, [P, P, P, P, P, POINTER(c_float), P, P, c_int64, P, P]),
    'perf_points_normalize': (c_int, [P, POINTER(c_float), P, P, c_int64, P]),
    'perf_hashgrid_fwd': (c_int, [POINTER(GridDesc), P, P, P, c_int64, P, c_int, P]),
    'perf_hashgrid_fwd2': (c_int, [POINTER(GridDesc), P, P, P, P, P, c_int64, c_int, P]),
    'perf_hashgrid_fwd_f32': (c_int, [POINTER(GridDesc), P, P, P, c_int64, P]),
    'perf_hashgrid_bwd_workspace_bytes': (c_int64, [POINTER(GridDesc), c_int64]),
    'perf_hashgrid_bwd': (c_int, [POINTER(GridDesc), P, P, P, c_int64, P, c_int, P, P, P, P, c_int, P, P, c_int64, P]),
    'perf_hashgrid_bwd_lines_workspace_bytes': (c_int64, [POINTER(GridDesc), c_int64]),
    'perf_hashgrid_bwd_lines': (c_int, [POINTER(GridDesc), P, P, P, c_int64, P, c_int, P, P, P, P, c_int, P, P, c_int64, P]),
    'perf_dp_stats_pack': (c_int, [P, P, P, c_int64, P, P]),
    'perf_dp_units': (c_int, [POINTER(GridDesc), P, c_int32, P, P, P, c_int32, P]),
    'perf_dp_slot_pack': (c_int, [P, P, P, c_int64, P, P, c_int64, c_int32, c_int32, P, P]),
    'perf_dp_slot_unpack': (c_int, [P, c_int32, P, P, P, P]),
    'perf_fixed_unfix': (c_int, [POINTER(GridDesc), P, c_int64, c_int64, P, P, P, P]),
    'perf_hashgrid_corners': (c_int, [POINTER(GridDesc), P, P, c_int64, P]),
    'perf_hashgrid_bwd_input': (c_int, [POINTER(GridDesc), P, P, P, P, c_int64, P]),
    'perf_hashgrid_bwd_bwd_input': (c_int, [POINTER(GridDesc), P, P, P, P, P, P, c_int64, P]),
    'perf_hashgrid_bwd_bwd_param': (c_int, [POINTER(GridDesc), P, P, P, P, c_int64, P]),
    'perf_mlp_fwd': (c_int, [POINTER(MlpDesc), P, P, P, P, c_int64, P, c_int, P]),
    'perf_field_infer_scratch_bytes': (c_int64, [POINTER(GridDesc), c_int64]),
    'perf_field_infer': (c_int, [POINTER(GridDesc), POINTER(MlpDesc), P, P, P, P, P, c_int64, P, P, c_int64, P, c_int, P]),
    'perf_field_bwd_workspace_bytes': (c_int64, [POINTER(GridDesc), POINTER(MlpDesc), c_int64, P, P, P]),
    'perf_field_bwd': (c_int, [POINTER(GridDesc), POINTER(MlpDesc), P, P, P, P, c_int64, P, P, P, c_int32, c_int32, P, P, P, c_int64, c_int64, P, c_int, P]),
    'perf_field_bwd_book': (c_int, [POINTER(GridDesc), POINTER(MlpDesc), P, P, P, P, c_int64, P, P, P, P, P, P, c_int64, c_int64, P, c_int, POINTER(StepBook), P]),
    'perf_mlp_bwd_workspace_bytes': (c_int64, [POINTER(MlpDesc), c_int64]),
    'perf_mlp_bwd': (c_int, [POINTER(MlpDesc), P, P, P, c_int64, P, P, P, P, P, P, c_int64, c_int64, P, c_int, P]),
    'perf_pano_raygen': (c_int, [POINTER(c_float), c_int32, c_int32, c_int32, c_int32, P, P, P]),
    'perf_pano_raygen_dev': (c_int, [P, c_int32, c_int32, c_int32, c_int32, P, P, P]),
    'perf_pers_raygen': (c_int, [POINTER(c_float), c_int32, c_int32, c_double, c_int32, c_int32, P, P, P]),
    'perf_pers_raygen_dev': (c_int, [P, c_int32, c_int32, c_double, c_int32, c_int32, P, P, P]),
    'perf_occ_pack_bits': (c_int, [P, P, c_int64, P]),
    'perf_occ_jitter_points': (c_int, [c_uint64, c_uint64, c_int64, c_int64, c_int32, POINTER(c_float), P, P]),
    'perf_occ_ema_update': (c_int, [P, P, c_int64, c_float, P, P]),
    'perf_occ_threshold': (c_int, [P, c_int64, P, c_float, P, P]),
    'perf_occ_mask_words': (c_int64, [c_int32]),
    'perf_occ_lattice_table_len': (c_int64, [c_int32]),
    'perf_occ_lattice_table': (c_int, [c_float, c_float, c_int32, c_int32, P, P]),
    'perf_occ_lattice_runs_len': (c_int64, [c_int64]),
    'perf_occ_lattice_runs': (c_int, [P, c_float, c_float, c_int64, c_float, c_int32, P, P]),
    'perf_occ_march_count': (c_int, [P, P, P, c_float, c_float, c_int64, P, P, c_int32, POINTER(c_float), c_float, c_float, c_int32, c_int32, P, P, P, P]),
    'perf_occ_march_count_head': (c_int, [P, P, P, c_float, c_float, c_int64, P, P, c_int32, POINTER(c_float), c_float, c_float, c_int32, c_int32, P, P, P,
                                  c_int32, P, P, P, P, POINTER(c_float), P, P, P]),
    'perf_occ_coarse_words': (c_int64, [c_int32]),
    'perf_occ_build_coarse': (c_int, [P, c_int32, P, P]),
    'perf_scan_workspace_bytes': (c_int64, [c_int64]),
    'perf_exclusive_scan_i32': (c_int, [P, P, P, c_int64, c_int64, P, P, c_int64, P]),
    'perf_occ_march_write': (c_int, [P, c_float, c_float, c_int64, c_float, c_int32, c_int32, P, P, P, P, c_int64, P, P, P, P, P]),
    'perf_occ_march_write_points': (c_int, [P, c_float, c_float, c_int64, c_float, c_int32, c_int32, P, P, P, P, c_int64, P, P, P, P, P, P, POINTER(c_float), P, P, c_int32, P]),
    'perf_head_tail_counts': (c_int, [P, c_int64, c_int32, P, P, P]),
    'perf_visibility_count2': (c_int, [P, P, P, P, P, P, P, P, c_int64, c_float, P, P]),
    'perf_compact_prefix2': (c_int, [P] * 14 + [c_int64, c_int64] + [P] * 7 + [P, c_int64, P, c_int64, P, c_int64, c_int32, P]),
    'perf_visibility_count': (c_int, [P, P, P, P, c_int64, c_float, P, P, P, c_int32, P, P]),
    'perf_compact_prefix': (c_int, [P, P, P, c_int64, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, P, c_int64, c_int32, P, P]),
    'perf_composite_fwd': (c_int, [P, P, P, P, P, c_int64, P, P, P, P, P, P, P]),
    'perf_composite_bwd': (c_int, [P, P, P, P, c_int64, P, P, P, P, P, P, P, P, P, P, P]),
    'perf_render_finish_eval': (c_int, [P, P, P, c_int64, P, P]),
    'perf_accumulate_fwd': (c_int, [P, P, P, c_int64, c_int32, P, P]),
    'perf_field_grad_x': (c_int, [POINTER(GridDesc), POINTER(MlpDesc), P, P, P, P, POINTER(c_float), P, P, c_int64, P, c_int, P]),
    'perf_normal_composite': (c_int, [P, P, P, c_int64, P, P]),
    'perf_pack_info': (c_int, [P, c_int64, c_int64, P, P]),
    'perf_distloss_fwd': (c_int, [P, P, P, P, c_int64, P, P]),
    'perf_distloss_bwd': (c_int, [P, P, P, P, c_int64, c_float, P, P, P]),
    'perf_geo_loss': (c_int, [P, P, P, P, P, P, c_int64, c_int64, c_float, c_float, P, c_float, P, P, P, P, P]),
    'perf_app_loss': (c_int, [P, P, P, P, c_int64, c_int64, c_float, c_float, P, P, P]),
    'perf_train_head_geo': (c_int, [P, P, P, P, P, c_int64, c_int64, P, P, c_int64, c_float, c_float, P, c_float, P, P, P, P, P, P, P, P, P, P]),
    'perf_train_head_app': (c_int, [P, P, P, P, P, c_int64, c_int64, P, P, c_int64, c_float, c_float, P, P, P, P, P, P, P, P]),
    'perf_composite_distloss_fwd': (c_int, [P, P, P, P, P, c_int64, P, P, P, P, P, P, P]),
    'perf_composite_distloss_bwd': (c_int, [P, P, P, P, c_int64, P, P, P, P, P, P, c_float, P, P, P]),
    'perf_gather_supervision': (c_int, [P, c_int64, P, P, P, P, P, P, P, P, P, P, P]),
    'perf_draw_train_batch': (c_int, [c_uint64, P, P, c_int64, c_int64, c_int64, c_int64] + [P] * 14 + [P]),
    'perf_pdf_resample': (c_int, [P, P, P, c_int64, c_int32, c_int32, P, P]),
    'perf_pano_reproject': (c_int, [P, c_int64, POINTER(c_float), P, c_int32, c_int32, c_int32, c_float, P, P]),
    'perf_morph_binary': (c_int, [P, P, c_int32, c_int32, POINTER(c_uint32), c_int32, c_int32, c_int32, P]),
    'perf_occ_splat': (c_int, [P, P, P, c_int64, c_int32, P, P]),
}

# include/perf_hip_ext.h: exported from the same library, versioned on its own (perf_ext_version)
_SIGS_EXT = {
    'perf_ext_version': (c_int, []),
    'perf_field_grad_x_bwd_workspace_bytes': (c_int64, [POINTER(GridDesc), POINTER(MlpDesc), c_int64]),
    'perf_field_grad_x_bwd': (c_int, [POINTER(GridDesc), POINTER(MlpDesc), P, P, P, P, POINTER(c_float), P, P, P, P, c_int64, c_int64, P, c_int, P]),
}

# include/perf_hip_sphere.h: the sphere distance field, exported from the same library, versioned on its own (perf_sphere_version)
_SIGS_SPHERE = {
    'perf_sphere_version': (c_int, []),
    'perf_sphere_field_fwd': (c_int, [POINTER(GridDesc), P, P, P, P, P, c_int64, P]),
    'perf_sphere_field_bwd_workspace_bytes': (c_int64, [POINTER(GridDesc), c_int64]),
    'perf_sphere_field_bwd': (c_int, [POINTER(GridDesc), P, P, P, P, P, P, P, c_int64, c_int64, P]),
}

# include/perf_hip_pair.h: the pair table, exported from the same library, versioned on its own (perf_pair_version)
_SIGS_PAIR = {
    'perf_pair_version': (c_int, []),
    'perf_pair_fill': (c_int, [P, c_int, P, c_int64, P]),
    'perf_hashgrid_fwd_pair': (c_int, [POINTER(GridDesc), P, P, P, P, c_int64, P, c_int, P]),
    'perf_adam_step_dev_pair': (c_int, [P, P, P, P, P, c_int64, c_int, P, P, P, c_float, c_float, c_float, c_int, P, P, c_int, c_int64, P]),
    'perf_mlp_fwd_rows': (c_int, [POINTER(MlpDesc), P, P, P, c_int64, P, P, c_int64, P, c_int, P]),
}

# include/perf_hip_joint.h: the joint predictor's alignment step, exported from the same library, versioned on its own (perf_joint_version)
JOINT_RECORD = 12        # PERF_JOINT_RECORD
JOINT_LOSSES = 8         # PERF_JOINT_LOSSES
_SIGS_JOINT = {
    'perf_joint_version': (c_int, []),
    'perf_joint_sample': (c_int, [P, P, P, P, P, P, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, P, P, P]),
    'perf_joint_loss_workspace_bytes': (c_int64, [c_int32, c_int64]),
    'perf_joint_loss': (c_int, [P, P, P, P, P, P, P, c_int32, c_int64, c_int32, c_int32, c_float, c_float, c_float, c_float, P, P, P, P, P, P, P, P,
                                c_int64, P]),
    'perf_joint_tv_workspace_bytes': (c_int64, [c_int64, c_int32, c_int32, c_int32]),
    'perf_joint_tv': (c_int, [P, c_int64, c_int32, c_int32, c_int32, c_float, P, P, P, c_int64, P]),
}

# include/perf_hip_mesh.h: surface nets on a dense lattice, exported from the same library, versioned on its own (perf_mesh_version)
MESH_MAX_CELLS = 1 << 30     # PERF_MESH_MAX_CELLS
_SIGS_MESH = {
    'perf_mesh_version': (c_int, []),
    'perf_mesh_workspace_bytes': (c_int64, [c_int32, c_int32, c_int32]),
    'perf_mesh_count': (c_int, [P, c_int32, c_int32, c_int32, c_float, P, c_int64, P, P]),
    'perf_mesh_write': (c_int, [P, c_int32, c_int32, c_int32, c_float, POINTER(c_float), POINTER(c_float), P, c_int64, P, c_int64, P, c_int64, P]),
}

# include/perf_hip_brickmesh.h: surface nets on the live 8^3 bricks of a lattice, versioned on its own (perf_brickmesh_version)
BRICKMESH_EDGE = 8                   # PERF_BRICKMESH_EDGE
BRICKMESH_MAX_DIM = 4096             # PERF_BRICKMESH_MAX_DIM
BRICKMESH_MAX_BRICKS = 1 << 21       # PERF_BRICKMESH_MAX_BRICKS
_SIGS_BRICKMESH = {
    'perf_brickmesh_version': (c_int, []),
    'perf_brickmesh_workspace_bytes': (c_int64, [c_int32, c_int32, c_int32, c_int32]),
    'perf_brickmesh_select': (c_int, [P, c_int32, c_int32, c_int32, c_int32, P, P, P, c_int64, P]),
    'perf_brickmesh_list': (c_int, [P, c_int32, c_int32, c_int32, P, c_int32, P]),
    'perf_brickmesh_corners': (c_int, [P, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, P, c_int32, P, P, P, P]),
    'perf_brickmesh_count': (c_int, [P, P, P, c_int32, c_int32, c_int32, c_int32, c_float, c_float, P, c_int64, P, P]),
    'perf_brickmesh_write': (c_int, [P, P, P, c_int32, c_int32, c_int32, c_int32, c_float, c_float, POINTER(c_float), POINTER(c_float), P, c_int64, P, c_int64,
                                     P, c_int64, P, P]),
}

# include/perf_hip_meshcc.h: connected components of a triangle mesh, versioned on its own (perf_meshcc_version)
MESHCC_MAX_VERTICES = 1 << 30        # PERF_MESHCC_MAX_VERTICES
MESHCC_MAX_FACES = 1 << 38           # PERF_MESHCC_MAX_FACES
_SIGS_MESHCC = {
    'perf_meshcc_version': (c_int, []),
    'perf_meshcc_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'perf_meshcc_label': (c_int, [P, c_int64, c_int64, P, P, P, c_int64, P]),
    'perf_meshcc_stats': (c_int, [P, c_int64, P, c_int64, P, c_int64, P, P, P, P]),
    'perf_meshcc_filter_count': (c_int, [P, c_int64, P, c_int64, P, c_int64, P, c_int64, P, P]),
    'perf_meshcc_filter_write': (c_int, [P, c_int64, P, c_int64, P, c_int64, P, P, c_int64, P, P, c_int64, P, c_int64, P]),
}

# include/perf_hip_meshvis.h: cull the faces of a mesh no registered panorama saw, versioned on its own (perf_meshvis_version)
MESHVIS_MAX_VIEWS = 64               # PERF_MESHVIS_MAX_VIEWS
MESHVIS_MAX_VERTICES = 1 << 30       # PERF_MESHVIS_MAX_VERTICES
MESHVIS_MAX_FACES = 1 << 38          # PERF_MESHVIS_MAX_FACES
MESHVIS_VIEW_BYTES = 64              # sizeof(perf_meshvis_view): rt [9], t [3] fp32, height, width int32, the map's device pointer
_SIGS_MESHVIS = {
    'perf_meshvis_version': (c_int, []),
    'perf_meshvis_sizeof_view': (c_int64, []),
    'perf_meshvis_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'perf_meshvis_vertex_bits': (c_int, [P, c_int64, P, POINTER(c_int32), c_int32, c_float, c_float, P, P, P]),
    'perf_meshvis_face_keep': (c_int, [P, c_int64, P, c_int64, P, P, P, c_int32, c_int32, c_int32, c_int32, P, P, P]),
    'perf_meshvis_filter_count': (c_int, [P, c_int64, c_int64, P, P, c_int64, P, P]),
    'perf_meshvis_filter_write': (c_int, [P, c_int64, c_int64, P, P, P, c_int64, P, P, c_int64, P, c_int64, P]),
}

# include/perf_hip_meshsimp.h: simplify a mesh by vertex clustering, versioned on its own (perf_meshsimp_version)
MESHSIMP_MAX_VERTICES = 1 << 30      # PERF_MESHSIMP_MAX_VERTICES
MESHSIMP_MAX_FACES = (1 << 31) - 1   # PERF_MESHSIMP_MAX_FACES
MESHSIMP_MAX_CELLS = 1 << 21         # PERF_MESHSIMP_MAX_CELLS, per axis
MESHSIMP_PLACEMENT = {'mean': 0, 'member': 1}                       # PERF_MESHSIMP_PLACE_*
MESHSIMP_DEDUPE = {None: 0, 'oriented': 1, 'unoriented': 2}         # PERF_MESHSIMP_DEDUPE_*
MESHSIMP_SCRATCH_BYTES = 48          # of perf_meshsimp_place's scratch, per cluster
_SIGS_MESHSIMP = {
    'perf_meshsimp_version': (c_int, []),
    'perf_meshsimp_table_slots': (c_int64, [c_int64]),
    'perf_meshsimp_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'perf_meshsimp_bounds': (c_int, [P, c_int64, P, P]),
    'perf_meshsimp_cluster': (c_int, [P, c_int64, c_int64, POINTER(c_float), c_float, c_int32, c_int32, c_int32, P, P, P, c_int64, P]),
    'perf_meshsimp_place': (c_int, [P, c_int64, POINTER(c_float), c_float, c_int32, c_int32, c_int32, P, c_int64, c_int32, P, P, P, c_int64, P]),
    'perf_meshsimp_faces': (c_int, [P, c_int64, P, c_int64, c_int32, P, P, P, P, c_int64, P]),
}

# include/perf_hip_meshcolor.h: colour a mesh's vertices from the registered panoramas, vertex normals from faces (perf_meshcolor_version)
MESHCOLOR_MAX_VIEWS = 64             # PERF_MESHCOLOR_MAX_VIEWS
MESHCOLOR_MAX_VERTICES = 1 << 30     # PERF_MESHCOLOR_MAX_VERTICES
MESHCOLOR_MAX_FACES = (1 << 31) - 1  # PERF_MESHCOLOR_MAX_FACES
MESHCOLOR_MAX_POWER = 8              # PERF_MESHCOLOR_MAX_POWER
MESHCOLOR_SELECT = {'blend': 0, 'best': 1}                          # PERF_MESHCOLOR_SELECT_*
_SIGS_MESHCOLOR = {
    'perf_meshcolor_version': (c_int, []),
    'perf_meshcolor_normal_sums': (c_int, [P, c_int64, P, c_int64, c_int32, P, P, P]),
    'perf_meshcolor_normals': (c_int, [P, c_int64, P, P]),
    'perf_meshcolor_blend': (c_int, [P, P, c_int64, P, P, POINTER(c_int32), c_int32, c_float, c_int32, c_int32, c_int32, P, POINTER(c_float), P, P, P, P, P]),
}

# include/perf_hip_meshray.h: rays against a triangle mesh on a uniform grid: closest hit, any hit, segment occlusion (perf_meshray_version)
MESHRAY_MAX_CELLS = 1 << 24          # PERF_MESHRAY_MAX_CELLS
MESHRAY_MAX_VIEWS = 64               # PERF_MESHRAY_MAX_VIEWS
MESHRAY_MAX_VERTICES = 1 << 30       # PERF_MESHRAY_MAX_VERTICES
MESHRAY_MAX_FACES = (1 << 31) - 1    # PERF_MESHRAY_MAX_FACES
_RAY_MESH = [P, c_int64, P, c_int64]                                  # vertices, n_vertices, faces, n_faces
_RAY_BOX = [POINTER(c_float), c_float, POINTER(c_int32)]              # origin, cell, dims
_SIGS_MESHRAY = {
    'perf_meshray_version': (c_int, []),
    'perf_meshray_grid_count': (c_int, _RAY_MESH + _RAY_BOX + [P, P, P]),
    'perf_meshray_grid_write': (c_int, _RAY_MESH + _RAY_BOX + [P, P, c_int64, P, c_int64, P]),
    'perf_meshray_cast': (c_int, _RAY_MESH + _RAY_BOX + [P, P, c_int64, P, P, c_int64, c_float, c_float, c_int32, P, P, P, P, P, P]),
    'perf_meshray_occluded': (c_int, _RAY_MESH + _RAY_BOX + [P, P, c_int64, P, c_int32, P, P, P]),
}

# include/perf_hip_meshtex.h: a texture atlas for a mesh: corner UVs, the texel -> point map, the fused bake (perf_meshtex_version)
MESHTEX_MIN_SIZE = 64                # PERF_MESHTEX_MIN_SIZE
MESHTEX_MAX_SIZE = 16384             # PERF_MESHTEX_MAX_SIZE
MESHTEX_MIN_TILE = 4                 # PERF_MESHTEX_MIN_TILE
MESHTEX_MAX_VIEWS = 64               # PERF_MESHTEX_MAX_VIEWS
MESHTEX_MAX_VERTICES = 1 << 30       # PERF_MESHTEX_MAX_VERTICES
MESHTEX_MAX_POWER = 8                # PERF_MESHTEX_MAX_POWER
MESHTEX_COVER = {'none': 0, 'inside': 1, 'gutter': 2}               # PERF_MESHTEX_COVER_*
_TEX_MESH = [P, c_int64, P, P, c_int64, c_int32, c_int32]             # vertices, n_vertices, normals, faces, n_faces, size, tile
_SIGS_MESHTEX = {
    'perf_meshtex_version': (c_int, []),
    'perf_meshtex_uv': (c_int, [c_int64, c_int32, c_int32, P, P]),
    'perf_meshtex_points': (c_int, _TEX_MESH + [P, P, P, P, P, P]),
    'perf_meshtex_bake': (c_int, _TEX_MESH + [P, P, POINTER(c_int32), c_int32, c_float, c_int32, c_int32, c_int32, P, POINTER(c_float), P, P, P, P, P, P]),
}

# include/perf_hip_meshquadric.h: quadric error placement of the clusters' vertices: int64 fixed-point sums, a 3 x 3 solve (perf_meshquadric_version)
MESHQUADRIC_MAX_VERTICES = 1 << 30       # PERF_MESHQUADRIC_MAX_VERTICES
MESHQUADRIC_MAX_FACES = (1 << 31) - 1    # PERF_MESHQUADRIC_MAX_FACES
MESHQUADRIC_MAX_CELLS = 1 << 21          # PERF_MESHQUADRIC_MAX_CELLS, per axis
MESHQUADRIC_TERMS = 9                    # PERF_MESHQUADRIC_TERMS: qA xx, xy, xz, yy, yz, zz, then qb x, y, z
MESHQUADRIC_FRACTION_BITS = 40           # PERF_MESHQUADRIC_FRACTION_BITS
MESHQUADRIC_SKIP_BITS = 60               # PERF_MESHQUADRIC_SKIP_BITS
MESHQUADRIC_REGULARISER_BITS = 10        # PERF_MESHQUADRIC_REGULARISER_BITS
_QUADRIC_GRID = [POINTER(c_float), c_float, c_int32, c_int32, c_int32]          # lo, h, nx, ny, nz
_SIGS_MESHQUADRIC = {
    'perf_meshquadric_version': (c_int, []),
    'perf_meshquadric_sums': (c_int, [P, c_int64, P, c_int64] + _QUADRIC_GRID + [P, c_int64, P, P, P, P]),
    'perf_meshquadric_place': (c_int, [P, c_int64] + _QUADRIC_GRID + [P, P, P, c_int64, P, P]),
}

# include/perf_hip_riders.h: the step riders, exported from the same library, versioned on their own (perf_riders_version)
RIDER_THREADS = 256          # PERF_RIDER_THREADS
RIDER_DRAW_RAYS = 256        # PERF_RIDER_DRAW_RAYS
RIDER_MARCH_RAYS = 4         # PERF_RIDER_MARCH_RAYS
RIDER_MAX_RAYS = 65536       # PERF_RIDER_MAX_RAYS
_SIGS_RIDERS = {
    'perf_riders_version': (c_int, []),
    'perf_sizeof_rider_draw': (c_int64, []),
    'perf_sizeof_rider_count': (c_int64, []),
    'perf_sizeof_rider_write': (c_int64, []),
    'perf_field_bwd_riders': (c_int, [POINTER(GridDesc), POINTER(MlpDesc), P, P, P, P, c_int64, P, P, P, c_int32, c_int32, P, P, P, c_int64, c_int64, P, c_int,
                                      POINTER(StepBook), POINTER(RiderDraw), POINTER(RiderCount), P]),
    'perf_adam_step_dev_riders': (c_int, [P, P, P, P, P, c_int64, c_int, P, P, P, c_float, c_float, c_float, c_int, P, P, c_int, c_int64, POINTER(RiderWrite), P]),
}

# include/staged/perf_hip_meshnear.h: the closest point of a triangle mesh to each query point, on the grid of perf_hip_meshray.h
# (perf_meshnear_version)
MESHNEAR_MAX_CELLS = 1 << 24         # PERF_MESHNEAR_MAX_CELLS
MESHNEAR_MAX_VERTICES = 1 << 30      # PERF_MESHNEAR_MAX_VERTICES
MESHNEAR_MAX_FACES = (1 << 31) - 1   # PERF_MESHNEAR_MAX_FACES
_SIGS_MESHNEAR = {
    'perf_meshnear_version': (c_int, []),
    'perf_meshnear_query': (c_int, _RAY_MESH + _RAY_BOX + [P, P, c_int64, P, c_int64, c_float, P, P, P, P, P]),
}


def _expects(label):
    return label + ' version {has}, this binding expects {want}'


Unit = namedtuple('Unit', 'name version sigs mismatch sizes header record macro version_fn')


def _unit(name, version, sigs, mismatch, sizes=(), folder=''):
    """One separately versioned C ABI of the library: its name, the version this binding was written against, its signatures, what a
    mismatch is reported as after "<library> has ", ((size function, the bytes this binding expects), ...).  The header and its recorded
    digest (both in include/, below folder when one is given), the version macro and the version function follow from the name; the
    core, perf_hip.h, is the one exception."""
    stem, part = ('perf_hip', '') if name == 'core' else (folder + 'perf_hip_' + name, name + '_')
    return Unit(name, version, sigs, mismatch, sizes, stem + '.h', stem + '.abi.json', f'PERF_{part.upper()}ABI_VERSION', f'perf_{part}version')


# The units of the library.  tools/abi_digest.py, perf_amd/build.py and tests/test_abi_units.py read this table: a new unit adds one row.
_UNITS = (
    _unit('core', ABI_VERSION, _SIGS, _expects('ABI')),
    _unit('ext', EXT_ABI_VERSION, _SIGS_EXT, _expects('extension ABI')),
    _unit('sphere', SPHERE_ABI_VERSION, _SIGS_SPHERE, _expects('sphere-field ABI')),
    _unit('pair', PAIR_ABI_VERSION, _SIGS_PAIR, _expects('pair-table ABI')),
    _unit('joint', JOINT_ABI_VERSION, _SIGS_JOINT, _expects('joint-alignment ABI')),
    _unit('mesh', MESH_ABI_VERSION, _SIGS_MESH, _expects('mesh ABI')),
    _unit('brickmesh', BRICKMESH_ABI_VERSION, _SIGS_BRICKMESH, _expects('brick-mesh ABI')),
    _unit('meshcc', MESHCC_ABI_VERSION, _SIGS_MESHCC, _expects('mesh-component ABI')),
    _unit('meshvis', MESHVIS_ABI_VERSION, _SIGS_MESHVIS,
          'visibility-cull ABI version {has} and a view of {has_sizes[0]} bytes, this binding expects {want} and {want_sizes[0]}',
          (('perf_meshvis_sizeof_view', MESHVIS_VIEW_BYTES),)),
    _unit('meshsimp', MESHSIMP_ABI_VERSION, _SIGS_MESHSIMP, _expects('mesh-simplification ABI')),
    _unit('meshcolor', MESHCOLOR_ABI_VERSION, _SIGS_MESHCOLOR, _expects('mesh-colouring ABI')),
    _unit('meshray', MESHRAY_ABI_VERSION, _SIGS_MESHRAY, _expects('mesh ray-casting ABI')),
    _unit('meshtex', MESHTEX_ABI_VERSION, _SIGS_MESHTEX, _expects('texture-atlas ABI')),
    _unit('meshquadric', MESHQUADRIC_ABI_VERSION, _SIGS_MESHQUADRIC, _expects('quadric-placement ABI')),
    _unit('riders', RIDERS_ABI_VERSION, _SIGS_RIDERS, 'step-rider ABI version {has} or other argument blocks than this binding ({want})',
          (('perf_sizeof_rider_draw', ctypes.sizeof(RiderDraw)), ('perf_sizeof_rider_count', ctypes.sizeof(RiderCount)),
           ('perf_sizeof_rider_write', ctypes.sizeof(RiderWrite)))),
)

# The staged units: bound, version-checked, digested and built exactly like the rows above, with header and record in include/staged/.
# A unit waits here until the pinned table of tests/test_abi_units.py is next open, and then moves up with one pin.
_STAGED_UNITS = (
    _unit('meshnear', MESHNEAR_ABI_VERSION, _SIGS_MESHNEAR, _expects('closest-point ABI'), folder='staged/'),
)

_lib = None


def load():
    """Load the shared library (once).  Raises PerfError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must be imported first: it carries its own libamdhip64, and the HIP runtime that owns the device
    # context has to be the one this library's kernels register with (one runtime per process).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise PerfError(f'{LIB_PATH} not found: build it with `python -m perf_amd.build` '
                        '(there is no CPU fallback for the HIP path)')
    lib = ctypes.CDLL(LIB_PATH)
    for unit in _UNITS + _STAGED_UNITS:
        for name, (res, args) in unit.sigs.items():
            fn = getattr(lib, name, None)
            if fn is None:
                raise PerfError(f'{LIB_PATH} does not export {name}: rebuild with `python -m perf_amd.build --force`')
            fn.restype = res
            fn.argtypes = args
    # the binding and the library must agree on every unit's ABI version and on the layout of the POD descriptors
    for unit in _UNITS + _STAGED_UNITS:
        has, want = getattr(lib, unit.version_fn)(), unit.version
        has_sizes, want_sizes = [getattr(lib, fn)() for fn, _ in unit.sizes], [n for _, n in unit.sizes]
        if has != want or has_sizes != want_sizes:
            raise PerfError(f'{LIB_PATH} has ' + unit.mismatch.format(has=has, want=want, has_sizes=has_sizes, want_sizes=want_sizes)
                            + ': rebuild with `python -m perf_amd.build --force`')
    if (lib.perf_sizeof_grid_desc() != ctypes.sizeof(GridDesc) or lib.perf_sizeof_mlp_desc() != ctypes.sizeof(MlpDesc)
            or lib.perf_sizeof_step_book() != ctypes.sizeof(StepBook)):
        raise PerfError('descriptor layout mismatch between perf_amd/_lib.py and include/perf_hip.h')
    _lib = lib
    return lib


def exported_symbols():
    return sorted(_SIGS)


def check(rc, what=''):
    if rc != 0:
        msg = load().perf_last_error()
        raise PerfError(f'{what} failed (code {rc}): {msg.decode() if msg else ""}')


def call(name, *args):
    lib = load()
    rc = getattr(lib, name)(*args)
    check(rc, name)
