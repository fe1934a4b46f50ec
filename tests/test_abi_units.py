"""Every separately versioned C ABI of the library, checked from the one table of perf_amd/_lib.py without a GPU: the header's macro, the
binding, the recorded digest and the library agree on the pinned version; the header's prototypes are the binding's table, name for name
and parameter count for parameter count; the units' names are disjoint; every header on disk is one unit's and the build depends on it.
A new unit adds one pin here; what is particular to it (constants, parameter types, refusals) is its own test file's."""
import glob
import json
import os
import re

import pytest

from tests import abi_units

ROOT = abi_units.ROOT
# unit -> (the pinned version, the sorted names its header declares)
PINS = {
    'core': (16, [
        'perf_accumulate_fwd', 'perf_adam_step', 'perf_adam_step_dev', 'perf_app_loss', 'perf_cast_params', 'perf_compact_prefix',
        'perf_compact_prefix2', 'perf_composite_bwd', 'perf_composite_distloss_bwd', 'perf_composite_distloss_fwd', 'perf_composite_fwd',
        'perf_distloss_bwd', 'perf_distloss_fwd', 'perf_dp_slot_pack', 'perf_dp_slot_unpack', 'perf_dp_stats_pack', 'perf_dp_units',
        'perf_draw_train_batch', 'perf_exclusive_scan_i32', 'perf_field_bwd', 'perf_field_bwd_book', 'perf_field_bwd_workspace_bytes',
        'perf_field_grad_x', 'perf_field_infer', 'perf_field_infer_scratch_bytes', 'perf_fixed_unfix', 'perf_gather_supervision',
        'perf_geo_loss', 'perf_hashgrid_bwd', 'perf_hashgrid_bwd_bwd_input', 'perf_hashgrid_bwd_bwd_param', 'perf_hashgrid_bwd_input',
        'perf_hashgrid_bwd_lines', 'perf_hashgrid_bwd_lines_workspace_bytes', 'perf_hashgrid_bwd_workspace_bytes', 'perf_hashgrid_corners',
        'perf_hashgrid_fwd', 'perf_hashgrid_fwd2', 'perf_hashgrid_fwd_f32', 'perf_head_tail_counts', 'perf_last_error', 'perf_mlp_bwd',
        'perf_mlp_bwd_workspace_bytes', 'perf_mlp_fwd', 'perf_morph_binary', 'perf_normal_composite', 'perf_occ_build_coarse',
        'perf_occ_coarse_words', 'perf_occ_ema_update', 'perf_occ_jitter_points', 'perf_occ_lattice_runs', 'perf_occ_lattice_runs_len',
        'perf_occ_lattice_table', 'perf_occ_lattice_table_len', 'perf_occ_march_count', 'perf_occ_march_count_head', 'perf_occ_march_write',
        'perf_occ_march_write_points', 'perf_occ_mask_words', 'perf_occ_pack_bits', 'perf_occ_splat', 'perf_occ_threshold', 'perf_pack_info',
        'perf_pano_raygen', 'perf_pano_raygen_dev', 'perf_pano_reproject', 'perf_pdf_resample', 'perf_pers_raygen', 'perf_pers_raygen_dev',
        'perf_points_from_rays', 'perf_points_normalize', 'perf_render_finish_eval', 'perf_scan_workspace_bytes', 'perf_sizeof_grid_desc',
        'perf_sizeof_mlp_desc', 'perf_sizeof_step_book', 'perf_step_bookkeeping', 'perf_train_head_app', 'perf_train_head_geo', 'perf_version',
        'perf_visibility_count', 'perf_visibility_count2']),
    'ext': (1, ['perf_ext_version', 'perf_field_grad_x_bwd', 'perf_field_grad_x_bwd_workspace_bytes']),
    'sphere': (1, ['perf_sphere_field_bwd', 'perf_sphere_field_bwd_workspace_bytes', 'perf_sphere_field_fwd', 'perf_sphere_version']),
    'pair': (1, ['perf_adam_step_dev_pair', 'perf_hashgrid_fwd_pair', 'perf_mlp_fwd_rows', 'perf_pair_fill', 'perf_pair_version']),
    'joint': (1, ['perf_joint_loss', 'perf_joint_loss_workspace_bytes', 'perf_joint_sample', 'perf_joint_tv', 'perf_joint_tv_workspace_bytes', 'perf_joint_version']),
    'mesh': (1, ['perf_mesh_count', 'perf_mesh_version', 'perf_mesh_workspace_bytes', 'perf_mesh_write']),
    'brickmesh': (1, ['perf_brickmesh_corners', 'perf_brickmesh_count', 'perf_brickmesh_list', 'perf_brickmesh_select', 'perf_brickmesh_version',
                      'perf_brickmesh_workspace_bytes', 'perf_brickmesh_write']),
    'meshcc': (1, ['perf_meshcc_filter_count', 'perf_meshcc_filter_write', 'perf_meshcc_label', 'perf_meshcc_stats', 'perf_meshcc_version', 'perf_meshcc_workspace_bytes']),
    'meshvis': (1, ['perf_meshvis_face_keep', 'perf_meshvis_filter_count', 'perf_meshvis_filter_write', 'perf_meshvis_sizeof_view', 'perf_meshvis_version',
                    'perf_meshvis_vertex_bits', 'perf_meshvis_workspace_bytes']),
    'meshsimp': (1, ['perf_meshsimp_bounds', 'perf_meshsimp_cluster', 'perf_meshsimp_faces', 'perf_meshsimp_place', 'perf_meshsimp_table_slots', 'perf_meshsimp_version',
                     'perf_meshsimp_workspace_bytes']),
    'meshcolor': (1, ['perf_meshcolor_blend', 'perf_meshcolor_normal_sums', 'perf_meshcolor_normals', 'perf_meshcolor_version']),
    'meshray': (1, ['perf_meshray_cast', 'perf_meshray_grid_count', 'perf_meshray_grid_write', 'perf_meshray_occluded', 'perf_meshray_version']),
    'meshtex': (1, ['perf_meshtex_bake', 'perf_meshtex_points', 'perf_meshtex_uv', 'perf_meshtex_version']),
    'meshquadric': (1, ['perf_meshquadric_place', 'perf_meshquadric_sums', 'perf_meshquadric_version']),
    'riders': (1, ['perf_adam_step_dev_riders', 'perf_field_bwd_riders', 'perf_riders_version', 'perf_sizeof_rider_count', 'perf_sizeof_rider_draw',
                   'perf_sizeof_rider_write']),
}


def _units():
    from perf_amd import _lib
    return {u.name: u for u in _lib._UNITS}


@pytest.mark.parametrize('name', list(PINS))
def test_header_binding_record_and_library_agree(name):
    from perf_amd import _lib
    abi_digest = abi_units.abi_digest()
    unit, (pinned, names) = _units()[name], PINS[name]
    text, plain = abi_units.header(name)
    record = json.load(open(abi_digest.record_path(name)))
    lib = _lib.load()
    bound = _lib.ABI_VERSION if name == 'core' else getattr(_lib, name.upper() + '_ABI_VERSION')
    assert abi_units.const(text, unit.macro) == bound == unit.version == record['version'] == getattr(lib, unit.version_fn)() == pinned
    flag = '' if name == 'core' else f'--{name} '
    now = abi_digest.digest(os.path.join(ROOT, 'include', unit.header), unit.macro)
    assert now == record == abi_digest.digest_unit(name), f'include/{unit.header} changed: bump {unit.macro}, then `python tools/abi_digest.py {flag}--write`'
    # declarations == binding table == the pinned names, name for name and parameter count for parameter count
    declared = sorted(set(re.findall(r'\b(perf_[a-z0-9_]+)\s*\(', plain)))
    assert declared == sorted(unit.sigs) == names
    for fn, (_, args) in unit.sigs.items():
        params = abi_units.params(plain, fn).strip()
        assert (0 if params in ('', 'void') else len(params.split(','))) == len(args), fn
        assert hasattr(lib, fn) and len(getattr(lib, fn).argtypes or []) == len(args), fn
    assert next(iter(unit.sigs)) == unit.version_fn


def test_the_units_names_are_disjoint():
    sets = [set(u.sigs) for u in _units().values()]
    assert all(not (a & b) for i, a in enumerate(sets) for b in sets[i + 1:])
    assert sum(len(s) for s in sets) == len(set().union(*sets)) == sum(len(names) for _, names in PINS.values())


def test_every_unit_of_the_binding_is_pinned():
    from perf_amd import _lib
    assert [u.name for u in _lib._UNITS] == list(PINS) and len(PINS) == 15
    assert _lib.exported_symbols() == PINS['core'][1]


def test_every_header_on_disk_is_one_units_and_has_its_record():
    units = _units().values()
    on_disk = lambda pattern: sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, 'include', pattern)))
    assert on_disk('perf_hip*.h') == sorted(u.header for u in units) and len({u.header for u in units}) == len(units)
    assert on_disk('*.abi.json') == sorted(u.record for u in units)


@pytest.mark.parametrize('name', list(PINS))
def test_the_build_depends_on_the_units_header(name):
    assert os.path.join(ROOT, 'include', _units()[name].header) in abi_units.build_deps()
