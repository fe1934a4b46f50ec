"""Generate tests/golden/joint_align.npz by IMPORTING the reference's utils/camera_utils.py and utils/geo_utils.py in the build container.

Run only where the reference tree exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_joint_fixture.py REFERENCE_ROOT

The reference's Python never travels; only the small .npz written next to this script does.  sys.modules stubs satisfy the *import
statements* of packages that are not installed here (trimesh, kornia, icecream); no reference logic is replaced.  Tensor.cuda is the
identity, so that _verts_to_dirs runs on the CPU.  Recorded:
  dirs, img_coord           direction_to_img_coord on 256 seeded unit directions; the last 32 are hand-made: next to the seam (alpha
                            within 1e-3 .. 1e-6 of +-pi, either side) and near, not at, the poles (|u_z| up to 1 - 1e-6)
  tri/<k>                   three hand-made triangles, one per branch of _verts_to_dirs' vertex ordering (the lone vertex given
                            first, second, third), and for gen_res 4 and ratios 1.1 and 1.7 its five outputs under
                            verts/<k>/<ratio>/{dirs, ratios, to_vec, down_vec, right_vec}
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20240917


def _directions():
    g = torch.Generator().manual_seed(SEED)
    d = torch.nn.functional.normalize(torch.randn(224, 3, generator=g), dim=-1)
    hand = []
    for k, eps in enumerate((1e-3, 1e-4, 1e-5, 1e-6)):
        for sign in (1.0, -1.0):
            alpha = sign * (np.pi - eps)
            for beta in (0.0, 0.7, -1.1):
                hand.append([np.cos(alpha) * np.cos(beta), np.sin(alpha) * np.cos(beta), np.sin(beta)])
    for z in (1 - 1e-3, 1 - 1e-5, 1 - 1e-6, -(1 - 1e-6)):
        for phi in (0.3, 2.9):
            r = np.sqrt(1 - z * z)
            hand.append([r * np.cos(phi), r * np.sin(phi), z])
    hand = torch.tensor(hand, dtype=torch.float64).float()
    assert hand.shape == (32, 3)
    return torch.cat([d, hand], 0)


TRIANGLES = [          # two vertices at one height, the lone one first / second / third; the third triangle has its lone vertex BELOW
    ([0.1, 0.2, 0.9], [0.5, -0.3, 0.4], [-0.2, 0.6, 0.4]),
    ([0.7, 0.1, -0.2], [0.3, 0.5, 0.6], [-0.1, 0.8, -0.2]),
    ([0.6, 0.2, 0.3], [-0.4, 0.5, 0.3], [0.2, 0.3, -0.7]),
]


def main(ref):
    sys.dont_write_bytecode = True
    for name in ('trimesh', 'kornia', 'kornia.filters', 'kornia.morphology', 'icecream'):
        sys.modules.setdefault(name, types.ModuleType(name))
    creation = types.ModuleType('trimesh.creation')
    creation.icosphere = None
    sys.modules.setdefault('trimesh.creation', creation)
    sys.modules['kornia.filters'].laplacian = None
    sys.modules['kornia.morphology'].erosion = sys.modules['kornia.morphology'].dilation = None
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, ref)
    from utils.camera_utils import direction_to_img_coord
    from utils.geo_utils import _verts_to_dirs
    out = {}
    dirs = _directions()
    out['dirs'] = dirs.numpy()
    out['img_coord'] = direction_to_img_coord(dirs).numpy()
    for k, tri in enumerate(TRIANGLES):
        out[f'tri/{k}'] = np.array(tri, dtype=np.float32)
        for ratio in (1.1, 1.7):
            pts = [np.array(p, dtype=np.float32) for p in tri]
            got = _verts_to_dirs(*pts, gen_res=4, ratio=ratio)
            for name, v in zip(('dirs', 'ratios', 'to_vec', 'down_vec', 'right_vec'), got):
                out[f'verts/{k}/{ratio}/{name}'] = v.numpy()
    np.savez_compressed(os.path.join(HERE, 'joint_align.npz'), **out)
    print('wrote joint_align.npz:', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
