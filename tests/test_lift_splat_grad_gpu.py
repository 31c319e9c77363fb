"""The differentiable fused lift-splat on the MI355X: ``sgv3d_amd.ops.voxel_pooling.lift_splat`` (forward: the planned gather
forming prob * context rows, backward: ``sgv3d_lift_splat_backward``) against the float64 restatement of
tests/lift_splat_ref.py and against the materialised composition (torch ``mul`` + the ``voxel_pooling`` operator), and the
training forward of the small models with the fusion on and off.

Error bounds of the random cases are a priori: an f32 sum of n rounded products, in any order, is within
(n + 2) * 2^-24 * sum |terms| of the exact value -- n = C for grad_prob, n = D for grad_context."""
import contextlib
import zlib

import numpy as np
import pytest
import torch

import lift_splat_ref as R
from sgv3d_amd import hip_ops
from sgv3d_amd.ops.voxel_pooling import lift_splat, voxel_pooling

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _geom(g, B, D, P, X, Y, Z, zs=(0,)):
    z = g.choice(np.asarray(zs), (B, D * P))
    return np.stack([g.integers(-2, X + 2, (B, D * P)), g.integers(-2, Y + 2, (B, D * P)), z], -1).astype(np.int32)


_CASES = {}


def _case(shape, kind="random", zs=(0,), long_run=False, geom_mode="draw"):
    """Inputs and the float64 reference of one case, computed once and shared (never modified)."""
    key = (shape, kind, zs, long_run, geom_mode)
    if key not in _CASES:
        B, D, P, C, X, Y, Z = shape
        g = np.random.default_rng(zlib.crc32(repr(key).encode()))
        geom = _geom(g, B, D, P, X, Y, Z, zs)
        if long_run:
            geom[0, :D * P // 3, :2] = 3                                   # one long run in one voxel
        if geom_mode == "outside":
            geom[..., 0] = np.where(g.integers(0, 2, (B, D * P)) > 0, X + 1, -1)
        elif geom_mode == "one_voxel":
            geom[..., 0], geom[..., 1], geom[..., 2] = X - 1, Y - 2, 0
        if kind == "integer":
            prob = g.integers(0, 4, (B, D, P)).astype(np.float32)
            ctx = g.integers(-4, 5, (B, P, C)).astype(np.float32)
            G = g.integers(-4, 5, (B, Y, X, C)).astype(np.float32)
        else:
            prob = g.random((B, D, P), dtype=np.float32)
            ctx = g.standard_normal((B, P, C), dtype=np.float32)
            G = g.standard_normal((B, Y, X, C), dtype=np.float32)
        ref = R.backward(geom, prob, ctx, G, (X, Y, Z))
        ref['out'] = R.forward(geom, prob, ctx, (X, Y, Z))
        _CASES[key] = dict(shape=shape, geom=geom, prob=prob, ctx=ctx, G=G, ref=ref)
    return _CASES[key]


def _dev(case):
    t = lambda a: torch.from_numpy(a).cuda()
    return t(case['geom']), t(case['prob']), t(case['ctx']), t(case['G'])


def _fused(case, need=(True, True), nchw_grad=False):
    """-> (out [B, Y, X, C], grad_prob or None, grad_context or None) of the fused operator."""
    B, D, P, C, X, Y, Z = case['shape']
    geom, prob, ctx, G = _dev(case)
    prob.requires_grad_(need[0])
    ctx.requires_grad_(need[1])
    out = lift_splat(geom, prob, ctx, (X, Y, Z))
    assert out.shape == (B, C, Y, X) and out.permute(0, 2, 3, 1).is_contiguous()     # a permuted view of an NHWC buffer
    if any(need):
        g = G.permute(0, 3, 1, 2)
        out.backward(g.contiguous() if nchw_grad else g)
    else:
        assert not out.requires_grad and out.grad_fn is None
    return out.detach().permute(0, 2, 3, 1), prob.grad, ctx.grad


def _materialised(case):
    B, D, P, C, X, Y, Z = case['shape']
    geom, prob, ctx, G = _dev(case)
    prob.requires_grad_(True)
    ctx.requires_grad_(True)
    lifted = prob[..., None] * ctx[:, None]                                        # [B, D, P, C]
    out = voxel_pooling(geom, lifted.reshape(B, D * P, C).contiguous(), (X, Y, Z))
    out.backward(G.permute(0, 3, 1, 2))
    return out.detach().permute(0, 2, 3, 1), prob.grad, ctx.grad


def _check_bounds(case, gp, gc):
    B, D, P, C, X, Y, Z = case['shape']
    ref = case['ref']
    ep = np.abs(gp.cpu().numpy().astype(np.float64) - ref['grad_prob'])
    ec = np.abs(gc.cpu().numpy().astype(np.float64) - ref['grad_context'])
    bp, bc = (C + 2) * U * ref['A_prob'], (D + 2) * U * ref['A_ctx']
    with np.errstate(divide='ignore', invalid='ignore'):
        print(f"{case['shape']}: grad_prob worst error / bound {np.nanmax(np.where(bp > 0, ep / bp, 0)):.3f}, "
              f"grad_context {np.nanmax(np.where(bc > 0, ec / bc, 0)):.3f}")
    assert (ep <= bp).all(), float((ep - bp).max())
    assert (ec <= bc).all(), float((ec - bc).max())


def _check_forward(case, out):
    """(the forward is the existing gather: |out - ref| within the a-priori bound of its longest sum)"""
    ref = case['ref']['out']
    n = case['shape'][1] * case['shape'][2]
    a = R.forward(case['geom'], np.abs(case['prob']), np.abs(case['ctx']), case['shape'][4:])
    assert (np.abs(out.cpu().numpy().astype(np.float64) - ref) <= (n + 2) * U * a).all()


# ------------------------------------------------------------------------------------------------ 1. exact on integers
def test_exact_on_integers():
    case = _case((2, 6, 35, 80, 8, 7, 1), kind="integer")
    out, gp, gc = _fused(case)
    ref = case['ref']
    assert torch.equal(out.cpu().double(), torch.from_numpy(ref['out']))
    assert torch.equal(gp.cpu().double(), torch.from_numpy(ref['grad_prob']))
    assert torch.equal(gc.cpu().double(), torch.from_numpy(ref['grad_context']))
    mout, mgp, mgc = _materialised(case)
    assert torch.equal(out, mout) and torch.equal(gp, mgp) and torch.equal(gc, mgc)


# ------------------------------------------------------------------------------------------------ 2. random data, a-priori bound
RANDOM = [((2, 9, 77, 24, 10, 9, 1), (0,), True), ((2, 9, 77, 80, 10, 9, 1), (0,), True), ((2, 9, 77, 88, 10, 9, 1), (0,), True),
          ((1, 180, 35, 88, 10, 9, 1), (0,), False), ((1, 1, 5, 256, 4, 4, 1), (0,), False),
          ((2, 7, 35, 24, 8, 7, 2), (-1, 0, 1, 2), False), ((2, 6, 35, 4, 8, 7, 1), (0,), False)]


@pytest.mark.parametrize("shape,zs,long_run", RANDOM, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_random_within_a_priori_bound(shape, zs, long_run):
    case = _case(shape, zs=zs, long_run=long_run)
    out, gp, gc = _fused(case)
    _check_bounds(case, gp, gc)
    _check_forward(case, out)
    keep = R.kept_mask(case['geom'], shape[4:]).reshape(shape[:3])
    assert (gp.cpu().numpy()[~keep] == 0).all()                                  # exact zeros where no point is kept
    mout, _, _ = _materialised(case)
    assert torch.equal(out, mout)                                               # forward: bitwise the two-step form


# every (lanes per pixel, columns per lane) shape of the kernel that the cases above do not reach, with D below one round of
# points and over several rounds with a ragged last one
@pytest.mark.parametrize("C", [8, 12, 16, 40, 128, 132, 160])
@pytest.mark.parametrize("D", [5, 70])
def test_every_kernel_shape(C, D):
    case = _case((2, D, 13, C, 6, 5, 1))
    out, gp, gc = _fused(case)
    _check_bounds(case, gp, gc)
    _check_forward(case, out)


# ------------------------------------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("shape,mode", [((2, 9, 35, 24, 8, 7, 1), "outside"), ((2, 9, 35, 24, 8, 7, 1), "one_voxel"),
                                        ((2, 9, 1, 24, 8, 7, 1), "draw")], ids=["all_outside", "one_voxel", "P1"])
def test_edges(shape, mode):
    case = _case(shape, geom_mode=mode)
    out, gp, gc = _fused(case)
    _check_bounds(case, gp, gc)
    _check_forward(case, out)
    if mode == "outside":
        assert not out.any() and not gp.any() and not gc.any()
    if mode == "one_voxel":
        assert int((out.abs().sum(-1) > 0).sum()) == shape[0]


# ------------------------------------------------------------------------------------------------ 4. gradient layouts
def test_gradient_layouts_bitwise_equal():
    case = _case((2, 9, 77, 80, 10, 9, 1), long_run=True)
    _, gp0, gc0 = _fused(case)
    _, gp1, gc1 = _fused(case, nchw_grad=True)
    assert torch.equal(gp0, gp1) and torch.equal(gc0, gc1)


# ------------------------------------------------------------------------------------------------ 5. autograd contract
def test_autograd_contract():
    case = _case((2, 9, 77, 80, 10, 9, 1), long_run=True)
    out, gp, gc = _fused(case)
    out_p, gp_p, gc_p = _fused(case, need=(True, False))
    out_c, gp_c, gc_c = _fused(case, need=(False, True))
    out_n, gp_n, gc_n = _fused(case, need=(False, False))
    assert gc_p is None and gp_c is None and gp_n is None and gc_n is None
    assert torch.equal(gp_p, gp) and torch.equal(gc_c, gc)
    assert torch.equal(out, out_p) and torch.equal(out, out_c) and torch.equal(out, out_n)
    B, D, P, C, X, Y, Z = case['shape']
    geom, prob, ctx, _ = _dev(case)
    o = lift_splat(geom, prob.requires_grad_(True), ctx, (X, Y, Z))
    assert o.grad_fn is not None and not geom.requires_grad
    with pytest.raises(RuntimeError):
        lift_splat(geom.cpu(), prob, ctx, (X, Y, Z))
    with pytest.raises(RuntimeError):
        lift_splat(geom, prob, ctx[..., :78].contiguous(), (X, Y, Z))              # C % 4 != 0: an error, no fallback


# ------------------------------------------------------------------------------------------------ 6. repeatability
@pytest.mark.parametrize("shape", [(2, 9, 77, 80, 10, 9, 1), (1, 180, 35, 88, 10, 9, 1)], ids=["D9", "D180"])
def test_backward_bitwise_repeatable(shape):
    case = _case(shape, long_run=shape[0] == 2)
    _, gp0, gc0 = _fused(case)
    _, gp1, gc1 = _fused(case)
    assert torch.equal(gp0, gp1) and torch.equal(gc0, gc1)


# ------------------------------------------------------------------------------------------------ 7. no tensor of the lifted size
def test_no_tensor_of_the_lifted_size():
    shape = (1, 64, 768, 80, 32, 32, 1)
    B, D, P, C, X, Y, Z = shape
    L = 4 * B * D * P * C
    g = np.random.default_rng(5)
    geom = torch.from_numpy(_geom(g, B, D, P, X, Y, Z)).cuda()
    prob0, ctx0 = torch.rand(B, D, P, device='cuda'), torch.randn(B, P, C, device='cuda')
    G = torch.randn(B, Y, X, C, device='cuda').permute(0, 3, 1, 2)

    def peak(fn):
        prob, ctx = prob0.clone().requires_grad_(True), ctx0.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        fn(prob, ctx).backward(G)
        torch.cuda.synchronize()
        assert prob.grad is not None and ctx.grad is not None
        return torch.cuda.max_memory_allocated() - start

    fused = peak(lambda p, c: lift_splat(geom, p, c, (X, Y, Z)))
    mat = peak(lambda p, c: voxel_pooling(geom, (p[..., None] * c[:, None]).reshape(B, D * P, C).contiguous(), (X, Y, Z)))
    print(f"peak allocation over forward + backward: fused {fused / 1e6:.2f} MB, materialised {mat / 1e6:.2f} MB, lifted tensor {L / 1e6:.2f} MB")
    assert fused < L / 2, (fused, L)
    assert mat > 2 * L, (mat, L)


# ------------------------------------------------------------------------------------------------ 8. model level
@contextlib.contextmanager
def _deterministic_profiled():
    saved = hip_ops.DETERMINISTIC, hip_ops.PROFILE
    hip_ops.DETERMINISTIC, hip_ops.PROFILE = True, []
    try:
        yield
    finally:
        hip_ops.DETERMINISTIC, hip_ops.PROFILE = saved


@contextlib.contextmanager
def _fusion_default(on):
    """The value new backbones take for ``fuse_lift_splat`` (what SGV3D_FUSE_LIFT_SPLAT sets at import)."""
    from sgv3d_amd.layers.backbones import bsm_lss_fpn, lss_fpn
    saved = lss_fpn.FUSE_LIFT_SPLAT, bsm_lss_fpn.FUSE_LIFT_SPLAT
    lss_fpn.FUSE_LIFT_SPLAT = bsm_lss_fpn.FUSE_LIFT_SPLAT = on
    try:
        yield
    finally:
        lss_fpn.FUSE_LIFT_SPLAT, bsm_lss_fpn.FUSE_LIFT_SPLAT = saved


def _kernels():
    return {r[0].split('|')[0] for r in hip_ops.PROFILE}


def _train_once(bsm, fuse):
    """One training forward / backward of the small model (batch 2, Dropout 0) from the seed's state."""
    from sgv3d_amd import synthetic
    from sgv3d_amd.losses import SemanticSupervision
    from sgv3d_amd.models.bev_height import BEVHeight
    from test_train_forward_gpu import _gt
    torch.manual_seed(0)
    bconf, hconf = synthetic.small_bsm_conf(depth=18) if bsm else synthetic.small_conf()
    if bsm:
        bconf = dict(bconf, is_train_height=True)
    model = BEVHeight(bconf, hconf, is_train_height=True) if bsm else BEVHeight(bconf, hconf)
    synthetic.randomize_norm_stats_(model, seed=0)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model = model.cuda().train()
    model.backbone.fuse_lift_splat = fuse
    model.head.train_cfg = dict(model.head.train_cfg, grid_size=[256, 256, 1], point_cloud_range=[0, -12.8, -5, 25.6, 12.8, 3])
    imgs = synthetic.make_images(2, final=bconf['final_dim'], device='cuda', seed=3)
    mats = synthetic.make_mats(2, device='cuda', scale=bconf['final_dim'][0] / 864)
    boxes, labels = _gt(2)
    with _deterministic_profiled():
        out = model(imgs, mats)
        preds = out[0] if bsm else out
        loss = model.loss(model.get_targets([b.cuda() for b in boxes], [l.cuda() for l in labels]), preds)
        if bsm:
            gt_sem = torch.randint(0, 7, (2, 1) + tuple(bconf['final_dim']), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
            loss = loss + SemanticSupervision(8)(out[1], gt_sem.cuda()) * 500
        loss.backward()
        kernels = _kernels()
    maps = [v.detach().clone() for t in preds for v in t[0].values()]
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return kernels, maps, loss.detach().clone(), grads


@pytest.mark.parametrize("bsm", [False, True], ids=["lss", "bsm"])
def test_model_fusion_on_and_off(bsm):
    k1, maps1, loss1, g1 = _train_once(bsm, True)
    k0, maps0, loss0, g0 = _train_once(bsm, False)
    assert "lift_splat_backward" in k1 and "lift_splat_planned" in k1 and "voxel_pooling_planned" not in k1, sorted(k1)
    assert "voxel_pooling_planned" in k0 and "lift_splat_backward" not in k0 and "lift_splat_planned" not in k0, sorted(k0)
    assert len(maps1) == len(maps0) and all(torch.equal(a, b) for a, b in zip(maps1, maps0))
    assert torch.equal(loss1, loss0)
    assert g1.keys() == g0.keys()
    head = [n for n in g1 if n.startswith("head.")]
    assert len(head) > 20 and all(torch.equal(g1[n], g0[n]) for n in head)
    # upstream of the BEV map the two backwards differ in summation order only -- and do reach the image branch
    up = [n for n in g1 if n.startswith("backbone.img_backbone") and float(g0[n].norm()) > 0]
    assert len(up) > 10
    rel = sorted(float((g1[n] - g0[n]).norm() / g0[n].norm()) for n in up)
    print(f"{'bsm' if bsm else 'lss'}: image-backbone gradients, fused against two-step: median relative L2 difference {rel[len(rel) // 2]:.1e}, worst {rel[-1]:.1e}")


def test_fused_training_gradients_match_oracle_lss():
    """The bars of test_training_forward_backward_matches_oracle with the fused path on (checked in the profile)."""
    from test_train_forward_gpu import _compare_with_oracle
    yard = []
    with _fusion_default(True), _deterministic_profiled():
        pred_err, loss_err, worst = _compare_with_oracle(yardstick=yard)
        kernels = _kernels()
    assert "lift_splat_backward" in kernels and "voxel_pooling_planned" not in kernels, sorted(kernels)
    assert pred_err <= 2e-3 and loss_err <= 1e-3, (pred_err, loss_err)
    live = [w for w in worst if w[2] > 1e-7]
    ylive = [w for w in yard if w[2] > 1e-7]
    stat = lambda rows: (sorted(r[0] for r in rows)[len(rows) // 2], sorted(r[0] for r in rows)[int(len(rows) * 0.9)], max(r[0] for r in rows))
    (m, p90, mx), (ym, yp90, ymx) = stat(live), stat(ylive)
    print(f'fused lift-splat, gradient tensors against float64: median {m:.1e} / p90 {p90:.1e} / worst {mx:.1e}; '
          f'torch float32 {ym:.1e} / {yp90:.1e} / {ymx:.1e}')
    assert m <= ym and p90 <= yp90 and mx <= ymx, ((m, p90, mx), (ym, yp90, ymx))
    assert m <= 2e-2 and p90 <= 4.5e-2 and mx <= 1.2e-1
    assert len(live) > 150


def test_fused_training_gradients_match_oracle_bsm():
    """The oracle test of tests/test_bsm_train_gpu.py, bars and all, with the fused path on (checked in the profile)."""
    import test_bsm_train_gpu
    with _fusion_default(True), _deterministic_profiled():
        test_bsm_train_gpu.test_bsm_training_forward_backward_matches_oracle()
        kernels = _kernels()
    assert "lift_splat_backward" in kernels and "voxel_pooling_planned" not in kernels, sorted(kernels)
