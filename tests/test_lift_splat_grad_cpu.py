"""CPU: the float64 restatement of the lift-splat adjoint (tests/lift_splat_ref.py) against torch autograd, the argument
validation of ``sgv3d_lift_splat_backward`` / ``sgv3d_lift_splat_backward_workspace_bytes`` (every rejection happens before
any HIP call: no GPU here), and the operator's refusal of CPU tensors."""
import numpy as np
import pytest
import torch

import lift_splat_ref as R


def _case(seed, B, D, P, C, X, Y, Z):
    g = np.random.default_rng(seed)
    geom = np.stack([g.integers(-2, X + 2, (B, D * P)), g.integers(-2, Y + 2, (B, D * P)),
                     g.integers(-1, Z + 1, (B, D * P))], -1).astype(np.int32)
    return geom, g.random((B, D, P)), g.standard_normal((B, P, C)), g.standard_normal((B, Y, X, C))


@pytest.mark.parametrize("shape", [(2, 5, 7, 8, 6, 5, 1), (1, 9, 4, 12, 3, 4, 2)])
def test_restatement_equals_float64_autograd(shape):
    """lifted = prob[..., None] * context[:, None] -> index_add_ into the map, differentiated by torch in float64."""
    B, D, P, C, X, Y, Z = shape
    geom, prob, ctx, G = _case(3, *shape)
    tp = torch.from_numpy(prob).requires_grad_(True)
    tc = torch.from_numpy(ctx).requires_grad_(True)
    lifted = (tp[..., None] * tc[:, None]).reshape(B, D * P, C)
    keep = torch.from_numpy(R.kept_mask(geom, (X, Y, Z)))
    out = torch.zeros(B, Y * X, C, dtype=torch.float64)
    tg = torch.from_numpy(geom).long()
    for b in range(B):
        out[b].index_add_(0, (tg[b, :, 1] * X + tg[b, :, 0])[keep[b]], lifted[b][keep[b]])
    out = out.reshape(B, Y, X, C)
    out.backward(torch.from_numpy(G))
    ref = R.backward(geom, prob, ctx, G, (X, Y, Z))
    for got, want in ((R.forward(geom, prob, ctx, (X, Y, Z)), out.detach().numpy()), (ref['grad_prob'], tp.grad.numpy()),
                      (ref['grad_context'], tc.grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert (np.abs(ref['grad_prob']) <= ref['A_prob'] * (1 + 1e-12)).all() and (np.abs(ref['grad_context']) <= ref['A_ctx'] * (1 + 1e-12)).all()
    assert (ref['grad_prob'][~R.kept_mask(geom, (X, Y, Z)).reshape(B, D, P)] == 0).all()


# sizes (B, D, P, C, X, Y, Z), then geom, prob, context, grad_output, (sb, sy, sx), grad_prob, grad_context, workspace, bytes.
# The pointers are never dereferenced: every case below is refused before a launch.
_GOOD = dict(sizes=(1, 64, 100, 80, 8, 8, 1), geom=0x1000, prob=0x2000, context=0x3000, gout=0x4000,
             strides=(8 * 8 * 80, 8 * 80, 80), gprob=0x5000, gctx=0x6000, ws=0x7000, ws_bytes=1 << 30)


def _call(lib, **over):
    a = dict(_GOOD, **over)
    return lib.sgv3d_lift_splat_backward(*a['sizes'], a['geom'], a['prob'], a['context'], a['gout'], *a['strides'], a['gprob'],
                                         a['gctx'], a['ws'], a['ws_bytes'], None)


def _sizes(**kw):
    names = ('B', 'D', 'P', 'C', 'X', 'Y', 'Z')
    return tuple(kw.get(n, v) for n, v in zip(names, _GOOD['sizes']))


def test_argument_validation_without_gpu():
    from sgv3d_amd import _lib
    lib = _lib.load()
    need = lib.sgv3d_lift_splat_backward_workspace_bytes(*_GOOD['sizes'][:4])
    assert need >= 16
    bad = [dict(sizes=_sizes(**{n: v})) for n in ('B', 'D', 'P', 'C', 'X', 'Y', 'Z') for v in (0, -1)]
    bad += [dict(sizes=_sizes(C=6)), dict(sizes=_sizes(C=82)), dict(sizes=_sizes(C=260))]
    bad += [dict(geom=None), dict(prob=None), dict(context=None), dict(gout=None)]
    bad += [dict(gout=0x4004), dict(gout=0x4008), dict(context=0x3004), dict(gctx=0x6008)]
    bad += [dict(strides=(5121, 640, 80)), dict(strides=(5120, 642, 80)), dict(strides=(5120, 640, 81))]
    bad += [dict(ws_bytes=need - 1), dict(ws=None), dict(ws_bytes=0)]
    for over in bad:
        rc = _call(lib, **over)
        msg = lib.sgv3d_last_error()
        assert rc != 0 and b"lift_splat_backward:" in msg, (over, rc, msg)
    for sizes in ((0, 1, 1, 4), (1, 0, 1, 4), (1, 1, 0, 4), (1, 1, 1, 0), (1, 1, 1, 6), (1, 1, 1, 260), (-1, 1, 1, 4)):
        assert lib.sgv3d_lift_splat_backward_workspace_bytes(*sizes) == 0
        assert b"lift_splat_backward_workspace_bytes" in lib.sgv3d_last_error(), sizes
    for sizes in ((1, 1, 1, 4), (2, 90, 5184, 80), (2, 180, 20736, 88), (1, 1, 5, 256)):
        assert lib.sgv3d_lift_splat_backward_workspace_bytes(*sizes) >= 16


def test_lift_splat_refuses_cpu_tensors():
    from sgv3d_amd.ops.voxel_pooling import lift_splat, lift_splat_covers
    geom = torch.zeros(1, 6, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must be a CUDAtensor"):
        lift_splat(geom, torch.zeros(1, 2, 3), torch.zeros(1, 3, 8), (4, 4, 1))
    assert lift_splat_covers(80, 1) and lift_splat_covers(88) and lift_splat_covers(4) and lift_splat_covers(256)
    assert not lift_splat_covers(87) and not lift_splat_covers(260) and not lift_splat_covers(80, 2)
