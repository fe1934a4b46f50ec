"""Every weight element reaches its place in the MLP kernels' fragments (stage_fragments: the block's coalesced copy of the weight
vector in LDS, rows one bank apart, and the gather from it).  Weights and features are small integers, chosen so that every sum is an
integer no 16-bit format rounds (|h1| <= 2 * n_levels <= 48, |h2| <= 2 * 48 with two non-zeros per row of the second layer, both
below 2^8) and the fp32 outputs are exact (|out| <= 64 * 96): the forward must EQUAL integer arithmetic, and a misplaced element of a
random integer matrix does not."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(n_levels, nh, dt, n, seed):
    from perf_amd.grid import MlpConfig
    mlp = MlpConfig(n_levels=n_levels, n_hidden_layers=nh, n_output_dims=16, output_activation='None')
    g = torch.Generator().manual_seed(seed)
    pad = mlp.n_in_pad
    w1 = torch.randint(-1, 2, (64, pad), generator=g).float()
    w2 = torch.zeros(64, 64)
    cols = torch.randint(0, 64, (64, 2), generator=g)
    w2.scatter_(1, cols, torch.randint(-1, 2, (64, 2), generator=g).float())       # (a repeated column keeps one of the two values)
    wo = torch.randint(-1, 2, (16, 64), generator=g).float()
    feat = torch.randint(-1, 2, (n_levels, n, 2), generator=g).float()
    x = feat.permute(1, 0, 2).reshape(n, 2 * n_levels)
    h = torch.relu(x @ w1[:, :2 * n_levels].T)
    if nh == 2:
        h = torch.relu(h @ w2.T)
    ref = h @ wo.T
    flat = torch.cat([w1.reshape(-1)] + ([w2.reshape(-1)] if nh == 2 else []) + [wo.reshape(-1)])
    assert flat.numel() == mlp.n_params
    return mlp, flat.to(dt).cuda(), feat.to(dt).cuda().contiguous(), ref


@pytest.mark.parametrize('n', [33, 4100])
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
@pytest.mark.parametrize('nh', [1, 2])
@pytest.mark.parametrize('n_levels', [8, 12, 16, 24])          # one, two (general and fast addressing) and three k-steps
def test_forward_equals_integer_arithmetic(n_levels, nh, dt, n):
    from perf_amd import ops
    mlp, w, feat, ref = _case(n_levels, nh, dt, n, 100 * n_levels + nh)
    out = ops.mlp_fwd(mlp, w, feat)
    assert torch.equal(out.cpu(), ref)
    index = torch.randperm(n, generator=torch.Generator().manual_seed(5))[: n // 2 + 1].int()
    rows = ops.mlp_fwd(mlp, w, ops.IndexedFeat(feat, index.cuda()))
    assert torch.equal(rows.cpu(), ref[index.long()])
