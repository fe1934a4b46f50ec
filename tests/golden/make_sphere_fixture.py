"""Generate tests/golden/sphere_mlp.npz by IMPORTING the reference's VanillaMLP (modules/fields/networks.py) in the build container.

Run only where the reference tree exists (never on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sphere_fixture.py REFERENCE_ROOT

The reference's Python never travels; only the small .npz written next to this script does.  sys.modules stubs satisfy the *import
statements* of packages that are not installed here; no reference logic is replaced.  Recorded, for VanillaMLP(35, 1, 64, 2,
sphere_init=True) with and without weight norm, one seed: the state_dict, 64 inputs, the outputs and the input gradients.  The feature
columns of the first layer (zero at initialisation, where the features would not matter) are redrawn at std 0.05 before recording.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20240611


def main(ref):
    sys.dont_write_bytecode = True
    for name in ('tinycudann', 'nerfacc', 'icecream', 'trimesh', 'cv2', 'kornia'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, ref)
    from modules.fields.networks import VanillaMLP
    out = {}
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(64, 35, generator=g)
    x[:, :3] = torch.nn.functional.normalize(x[:, :3], dim=-1)
    x[:, 3:] *= 0.1
    out['x'] = x.numpy()
    for tag, wn in (('plain', False), ('wn', True)):
        torch.manual_seed(SEED)
        mlp = VanillaMLP(35, 1, 64, 2, sphere_init=True, weight_norm=wn)
        with torch.no_grad():
            first = mlp.layers[0]
            w = first.weight_v if wn else first.weight
            w[:, 3:] = torch.randn(64, 32, generator=g) * 0.05
            if wn:
                first.weight_g.copy_(first.weight_v.norm(2, dim=1, keepdim=True) * 1.25)       # g != |v|: the norm must matter
        xi = x.clone().requires_grad_(True)
        y = mlp(xi)
        gx, = torch.autograd.grad(y.sum(), xi)
        out[f'{tag}/keys'] = np.array(list(mlp.state_dict().keys()))
        for k, v in mlp.state_dict().items():
            out[f'{tag}/sd/{k}'] = v.detach().numpy()
        out[f'{tag}/y'] = y.detach().numpy()
        out[f'{tag}/gx'] = gx.numpy()
    np.savez_compressed(os.path.join(HERE, 'sphere_mlp.npz'), **out)
    print('wrote sphere_mlp.npz:', {k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
