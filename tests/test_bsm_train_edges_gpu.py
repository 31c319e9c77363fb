"""The four kernels of csrc/bsm_train.hip on the MI355X at their edges: the focal loss across the grid, at block boundaries,
at every storage geometry, with labels that are no class, with nothing kept, at saturated logits and through the parameters
only the C ABI reaches; the label downsample at every byte lane of its fast path, at every factor and from a misaligned
mask; the upsample adjoint probed tap by tap; the gate adjoint at saturating arguments.

oracle/focal_ref.py in float64 (and autograd through it) is the reference of every focal value and gradient; the inputs
come from tests/bsm_train_edges.py, and tests/test_bsm_train_edges_cpu.py shows that they are fair: the same oracle in
float32 stays within a quarter of every bound applied here."""
import math

import pytest
import torch

import bsm_train_edges as E
from oracle import focal_ref as R
from sgv3d_amd import _lib, bsm_grad
from sgv3d_amd._lib import SGV3DError
from sgv3d_amd.losses import FocalLoss, downsample_gt_semantic
from sgv3d_amd.losses.focal import focal_loss_with_logits

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _st():
    return _lib.stream_handle(torch.device(DEV))


# =============================================================================================== focal loss
def _run(case, layout=None):
    """(loss, gradient in logical order on the CPU) of a case through the wrapper its mode names."""
    x, y = E.focal_inputs(case['name'])
    xd = E.to_layout(x.to(DEV), layout or case['layout']).requires_grad_(True)
    yd = y.to(DEV)
    kw = case['kw']
    if case['mode'] == 'functional':
        loss = focal_loss_with_logits(xd, yd, kw['gamma'], kw['alpha'], kw['reduction'])
    else:
        loss = FocalLoss(case['mode'], **kw)(xd, yd)
    loss.backward()
    return loss.detach().cpu(), xd.grad.cpu()


def _check(case, got, got_g):
    want, want_g = E.focal_reference(case['name'])
    tol, rtol, atol = E.focal_tolerances(want, want_g)
    err = float(((got_g.double() - want_g).abs() / (atol + rtol * want_g.abs())).max())
    print(f"{case['name']}: loss {float(got)!r} want {float(want)!r} (bound {tol:.1e}); gradient at {err:.3f} of its bound")
    assert abs(float(got) - float(want)) <= tol, (float(got), float(want))
    torch.testing.assert_close(got_g.double(), want_g, rtol=rtol, atol=atol)


def _run_and_check(name):
    case = E.FOCAL_CASES[name]
    got, got_g = _run(case)
    _check(case, got, got_g)
    return got, got_g


@pytest.fixture(scope="module")
def grid_runs():
    """name -> (loss, gradient) of the grid-crossing cases, run once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _run(E.FOCAL_CASES[name])
        return cache[name]
    return get


@pytest.mark.parametrize("name", E.names('grid'))
def test_focal_across_the_grid(grid_runs, name):
    """132098 pixels: 1026 of them in the second trip of the grid-stride loop, all 512 float64 partials in use."""
    got, got_g = grid_runs(name)
    _check(E.FOCAL_CASES[name], got, got_g)
    again, again_g = _run(E.FOCAL_CASES[name])
    assert torch.equal(again, got) and torch.equal(again_g, got_g)             # fixed-order sums: bitwise repeatable


@pytest.mark.parametrize("layout", ['nchw', 'nhwc_view'])
@pytest.mark.parametrize("red", ['mean', 'sum'])
def test_focal_across_the_grid_label_types_agree_bitwise(grid_runs, layout, red):
    a, a_g = grid_runs(f'grid-uint8-{layout}-{red}')
    b, b_g = grid_runs(f'grid-int64-{layout}-{red}')
    assert torch.equal(a, b) and torch.equal(a_g, b_g)


@pytest.mark.parametrize("name", E.names('block'))
def test_focal_block_boundaries(name):
    _run_and_check(name)


@pytest.mark.parametrize("name", E.names('classes'))
def test_focal_class_counts_and_strides(name):
    _run_and_check(name)


def _abi(x, target, kind, N, C, P, strides, *, alpha=0.25, gamma=2.0, ignore=None, mean=True, grad_scale=1.0, grad=None,
         ws_short=0, out=None):
    """sgv3d_focal_loss_with_logits as the C ABI has it; returns (return code, loss tensor [1])."""
    lib = _lib.load()
    nws = lib.sgv3d_focal_loss_workspace_bytes()
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    out = torch.full((1,), E.GUARD, device=DEV) if out is None else out
    rc = lib.sgv3d_focal_loss_with_logits(
        N, C, P, _lib.ptr(x), strides[0], strides[1], strides[2], _lib.ptr(target), kind, -1.0 if alpha is None else alpha,
        gamma, 0 if ignore is None else ignore, 0 if ignore is None else 1, 1 if mean else 0, grad_scale, _lib.ptr(grad),
        out.data_ptr(), ws.data_ptr(), nws - ws_short, _st())
    return rc, out


def test_focal_channel_slice_gradient_keeps_the_geometry():
    """7 of 8 channels of a channel-last buffer at the C ABI: the gradient lands at the logits' addresses, the eighth channel of the
    gradient buffer keeps its guard value."""
    case = E.FOCAL_CASES['slice7of8']
    x, y = E.focal_inputs(case['name'])
    xd = E.to_layout(x.to(DEV), 'slice8')
    N, C, H, W = x.shape
    assert xd.stride() == (H * W * 8, 1, W * 8, 8)
    gbuf = torch.full((N, H, W, 8), E.GUARD, device=DEV)
    rc, out = _abi(xd, y.to(DEV), 0, N, C, H * W, (H * W * 8, 1, 8), grad=gbuf)
    _lib.check(rc, "sgv3d_focal_loss_with_logits")
    gbuf = gbuf.cpu()
    assert bool((gbuf[..., 7] == E.GUARD).all())
    _check(case, out.cpu()[0], gbuf[..., :7].permute(0, 3, 1, 2))


@pytest.mark.parametrize("name", E.names('labels'))
def test_focal_labels_outside_the_classes_and_ignored(name):
    case = E.FOCAL_CASES[name]
    _, got_g = _run_and_check(name)
    ig = case['kw']['ignore_index']
    if ig is not None:
        _, y = E.focal_inputs(name)
        ignored = (y == ig).unsqueeze(1).expand_as(got_g)
        assert bool((got_g[ignored] == 0.0).all())                            # exactly 0.0, not a small number
        assert bool((got_g[~ignored] != 0.0).any())


@pytest.mark.parametrize("case", E.NOTHING_KEPT, ids=[c['name'] for c in E.NOTHING_KEPT])
def test_focal_nothing_kept(case):
    """Every label is ignore_index.  The oracle (pinned in the CPU file): loss NaN for 'mean' (the mean of nothing), 0 for 'sum',
    and an all-zero gradient, since boolean indexing scatters nothing back."""
    got, got_g = _run(case)
    if case['kw']['reduction'] == 'mean':
        assert math.isnan(float(got))
    else:
        assert float(got) == 0.0
    assert bool((got_g == 0.0).all()), got_g.flatten()[:8]


@pytest.mark.parametrize("name", E.names('saturation'))
def test_focal_saturated_logits(name):
    """+-30, +-88, +-1e4, 0.0 and -0.0 among 6 * randn logits, each against targets of 1 and of 0: expf, log1pf and 1 - pt at
    both ends of their range."""
    case = E.FOCAL_CASES[name]
    got, got_g = _run_and_check(name)
    assert math.isfinite(float(got)) and bool(torch.isfinite(got_g).all())
    want, want_g = E.focal_reference(name)
    _, rtol, atol = E.focal_tolerances(want, want_g)
    right, wrong, t = E.planted_masks(case)
    assert float(got_g[right].abs().max()) <= atol                            # a saturated correct prediction: nothing to learn
    kw = case['kw']
    div = float(got_g[:, 0].numel()) if kw['reduction'] == 'mean' else 1.0
    w = torch.ones_like(want_g) if kw['alpha'] is None else torch.where(t, kw['alpha'], 1 - kw['alpha']).double()
    torch.testing.assert_close(got_g.double()[wrong], (torch.where(t, -w, w) / div)[wrong], rtol=rtol, atol=atol)


def test_focal_all_predictions_saturated_and_correct():
    """+88 at the labelled class, -88 elsewhere: the loss is 0 to the last bit or a denormal, for every gamma."""
    y = torch.arange(24).reshape(2, 3, 4) % 3
    x = (torch.nn.functional.one_hot(y, 3).permute(0, 3, 1, 2).float() * 2 - 1) * 88
    for gamma in (0.0, 1.0, 1.5, 2.0, 3.0):
        xd = x.to(DEV).requires_grad_(True)
        loss = FocalLoss('multiclass', alpha=0.25, gamma=gamma, reduction='sum')(xd, y.to(DEV))
        loss.backward()
        want = float(R.focal_loss(x.double(), y, 'multiclass', 0.25, gamma, None, 'sum'))
        assert 0.0 <= float(loss) <= 1e-30 and want <= 1e-30, (gamma, float(loss), want)
        assert float(xd.grad.abs().max()) <= 1e-30


@pytest.mark.parametrize("name", E.names('small_gamma'))
def test_focal_gamma_below_one(name):
    """The generic powf branch with a negative exponent in the derivative.  The logits are capped at |x| <= 8: where 1 - pt
    underflows to 0 (the planted +-30 and +-88 of the saturation cases) the oracle's own gradient, gamma * 0^(gamma - 1) times 0,
    is not finite, while the kernel returns 0 there by design -- the reference defines nothing to compare with.  The CPU file
    asserts that the float64 gradient of every case here is finite."""
    got, got_g = _run_and_check(name)
    assert bool(torch.isfinite(got_g).all())


@pytest.mark.parametrize("name", E.names('float_targets'))
def test_focal_float_targets(name):
    """target_kind 2 through FocalLoss('binary'), FocalLoss('multilabel') and focal_loss_with_logits; the divisor of 'mean' is the
    element count (after the wrapper's ignore mask)."""
    _run_and_check(name)


# ----------------------------------------------------------------------------------------------- ABI-only parameters
def _abi_case(name='classes-7-nhwc_view'):
    case = E.FOCAL_CASES[name]
    x, y = E.focal_inputs(name)
    N, C, H, W = x.shape
    xd = x.to(DEV).permute(0, 2, 3, 1).contiguous()                           # NHWC storage
    return case, xd, y.to(DEV), (N, C, H * W), (H * W * C, 1, C)


@pytest.mark.parametrize("mean", [True, False])
def test_focal_grad_scale_and_null_grad(mean):
    """grad_scale multiplies the gradient and leaves the value alone; a null gradient pointer leaves the value alone."""
    case, xd, yd, dims, strides = _abi_case()
    runs = {}
    for gs in (1.0, 0.5, 500.0):
        grad = torch.full_like(xd, E.GUARD)
        rc, out = _abi(xd, yd, 1, *dims, strides, mean=mean, grad_scale=gs, grad=grad)
        _lib.check(rc, "sgv3d_focal_loss_with_logits")
        runs[gs] = (out.cpu(), grad.cpu())
    rc, out = _abi(xd, yd, 1, *dims, strides, mean=mean, grad_scale=500.0, grad=None)
    _lib.check(rc, "sgv3d_focal_loss_with_logits")
    base, base_g = runs[1.0]
    assert torch.equal(out.cpu(), base)
    assert torch.equal(runs[0.5][0], base) and torch.equal(runs[500.0][0], base)
    assert torch.equal(runs[0.5][1], base_g * 0.5)                             # a power of two: exact
    if not mean:
        assert torch.equal(runs[500.0][1], base_g * 500.0)                     # g * 500 on both sides
    # 'mean': g * fl(500 / n) against fl(g * fl(1 / n)) * 500 -- five roundings of 2^-24 between them
    torch.testing.assert_close(runs[500.0][1], base_g * 500.0, rtol=5 * 2.0 ** -24, atol=1e-37)
    # and against the oracle: d (500 * loss) / d logits
    x, y = E.focal_inputs(case['name'])
    xr = x.double().requires_grad_(True)
    (500.0 * R.focal_loss(xr, y, 'multiclass', 0.25, 2.0, None, 'mean' if mean else 'sum')).backward()
    want_g = xr.grad.permute(0, 2, 3, 1)
    torch.testing.assert_close(runs[500.0][1].double(), want_g, rtol=2e-5, atol=2e-6 * float(want_g.abs().max()))


def test_focal_abi_rejections_before_launch():
    """Each bad call returns the error code and launches nothing: loss, gradient keep their fill."""
    _, xd, yd, dims, strides = _abi_case()
    N, C, P = dims
    grad = torch.full_like(xd, E.GUARD)
    out = torch.full((1,), E.GUARD, device=DEV)
    tf = torch.rand_like(xd)
    common = dict(grad=grad, out=out)
    bad = [
        lambda: _abi(xd, yd, 1, N, C, P, strides, gamma=-0.5, **common),
        lambda: _abi(xd, yd, 3, N, C, P, strides, **common),
        lambda: _abi(xd, yd, -1, N, C, P, strides, **common),
        lambda: _abi(xd, tf, 2, N, C, P, strides, ignore=255, **common),
        lambda: _abi(xd, yd, 1, N, C, P, strides, ws_short=1, **common),
        lambda: _abi(xd, yd, 1, 0, C, P, strides, **common),
        lambda: _abi(xd, yd, 1, N, 0, P, strides, **common),
        lambda: _abi(xd, yd, 1, N, C, 0, strides, **common),
        lambda: _abi(None, yd, 1, N, C, P, strides, **common),
        lambda: _abi(xd, None, 1, N, C, P, strides, **common),
    ]
    for call in bad:
        with pytest.raises(SGV3DError):
            _lib.check(call()[0], "rejected call")
    torch.cuda.synchronize()
    assert bool((grad == E.GUARD).all()) and bool((out == E.GUARD).all())


# =============================================================================================== label downsample
@pytest.mark.parametrize("value", E.ONE_HOT_IDS)
def test_labels_one_hot_blocks(value):
    """One non-zero id per 8x8 block, at cell k in block k: a dropped byte lane or row of the fast path loses one output."""
    img = E.one_hot_blocks(value)
    got = downsample_gt_semantic(img.to(DEV), 8).cpu()
    assert got.dtype == torch.uint8 and got.shape == (1, 8, 8)
    assert torch.equal(got, torch.full((1, 8, 8), value, dtype=torch.uint8)), got


def test_labels_ramps_and_constant_blocks():
    for name, img in E.ramp_blocks().items():
        got = downsample_gt_semantic(img.to(DEV), 8).cpu()
        assert torch.equal(got.long(), R.downsample_gt_semantic(img, 8)), name


@pytest.mark.parametrize("shape", E.LABEL_SHAPES, ids=['x'.join(map(str, s)) for s in E.LABEL_SHAPES])
def test_labels_factors_and_shapes(shape):
    B, N, H, W, f = shape
    gt = E.random_mask((B, N, H, W), seed=H + W + f)
    got = downsample_gt_semantic(gt.to(DEV), f).cpu()
    assert got.shape == (B * N, H // f, W // f)
    assert torch.equal(got.long(), R.downsample_gt_semantic(gt, f))


def _labels_abi(ptr, B, H, W, f, out):
    return _lib.load().sgv3d_semantic_labels_downsample(B, H, W, f, ptr, _lib.ptr(out), _st())


@pytest.mark.parametrize("offset", [1, 4])
def test_labels_misaligned_mask(offset):
    """A mask that starts 1 or 4 bytes past an 8-byte boundary: the 8-byte loads of the fast path need that boundary, so the
    kernel takes its byte loop; the labels are those of the aligned copy."""
    B, H, W = 2, 24, 40
    gt = E.random_mask((B, 1, H, W), seed=offset)
    buf = torch.zeros(B * H * W + 8, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 8 == 0
    view = buf[offset:offset + B * H * W]
    view.copy_(gt.to(DEV).view(-1))
    assert view.data_ptr() % 8 == offset
    out = torch.zeros(B, H // 8, W // 8, dtype=torch.uint8, device=DEV)
    _lib.check(_labels_abi(view.data_ptr(), B, H, W, 8, out), "sgv3d_semantic_labels_downsample")
    aligned = downsample_gt_semantic(gt.to(DEV), 8)
    assert torch.equal(out, aligned)
    assert torch.equal(out.cpu().long(), R.downsample_gt_semantic(gt, 8))


def test_labels_abi_rejections_before_launch():
    gt = E.random_mask((1, 1, 16, 24)).to(DEV)
    out = torch.full((6,), 9, dtype=torch.uint8, device=DEV)
    bad = [
        lambda: _labels_abi(gt.data_ptr(), 1, 15, 24, 8, out),
        lambda: _labels_abi(gt.data_ptr(), 1, 16, 20, 8, out),
        lambda: _labels_abi(gt.data_ptr(), 1, 16, 24, 0, out),
        lambda: _labels_abi(gt.data_ptr(), 0, 16, 24, 8, out),
        lambda: _labels_abi(None, 1, 16, 24, 8, out),
        lambda: _labels_abi(gt.data_ptr(), 1, 16, 24, 8, None),
    ]
    for call in bad:
        with pytest.raises(SGV3DError):
            _lib.check(call(), "rejected call")
    torch.cuda.synchronize()
    assert bool((out == 9).all())


# =============================================================================================== upsample adjoint
def _up_device(x, dy):
    xd = x.to(DEV).requires_grad_(True)
    yd = bsm_grad.upsample_bilinear2x(xd)
    yd.backward(dy.to(DEV))
    return yd.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("hw", E.PROBE_SHAPES)
def test_upsample_adjoint_one_hot_probes(hw):
    """dy one-hot at every position of the 2H x 2W map (one sample each): every tap weight is a product of two of {1, 3/4, 1/4},
    so dx equals the float64 autograd result to the last bit -- the 1 at the first and last row and column, and no tap where
    there is no neighbour."""
    H, W = hw
    dy = E.probes(H, W)
    x = torch.zeros(4 * H * W, H, W, 1)
    _, want = E.upsample_reference(x.double(), dy.double())
    _, got = _up_device(x, dy)
    assert torch.equal(got, want.float()), (got - want.float()).abs().max()


@pytest.mark.parametrize("shape", E.ADJOINT_SHAPES)
def test_upsample_adjoint_identity(shape):
    """<up(x), dy> == <x, upT(dy)> with both maps from the device, the inner products in float64 on the host."""
    x, dy = E.adjoint_inputs(shape, positive=True)
    y, dx = _up_device(x, dy)
    err = E.adjoint_error(x, y, dy, dx)
    print(f'{shape}: adjoint identity error {err:.2e}')
    assert err <= 1e-6


@pytest.mark.parametrize("shape", E.ADJOINT_SHAPES)
def test_upsample_adjoint_against_autograd(shape):
    x, dy = E.adjoint_inputs(shape)
    want_y, want_dx = E.upsample_reference(x.double(), dy.double())
    y, dx = _up_device(x, dy)
    torch.testing.assert_close(y.double(), want_y, rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(dx.double(), want_dx, rtol=1e-6, atol=1e-6)


# =============================================================================================== add_mul_sigmoid adjoint
@pytest.mark.parametrize("n", E.GATE_COUNTS)
def test_gate_adjoint_at_saturating_arguments(n):
    """c = 3 * randn with +-20, +-88, +-104 and 0 planted: expf(-c) saturates and overflows.  All three gradients are finite and
    match float64 autograd; dc is exactly 0 where the float32 sigmoid is exactly 0 or 1."""
    a, b, c, dy = E.gate_inputs(n)
    dev = [t.to(DEV).requires_grad_(True) for t in (a, b, c)]
    bsm_grad.add_mul_sigmoid(*dev).backward(dy.to(DEV))
    got = [d.grad.cpu() for d in dev]
    for g, w in zip(got, E.gate_reference(n)):
        assert bool(torch.isfinite(g).all())
        torch.testing.assert_close(g.double(), w, rtol=1e-5, atol=1e-6)
    assert torch.equal(got[0], dy)                                            # da is dy passed through
    saturated = torch.isin(c, torch.tensor(E.GATE_SATURATED))
    assert int(saturated.sum()) >= 2 and bool((got[2][saturated] == 0.0).all())


@pytest.mark.parametrize("n", [0, 3, 1022, -4])
def test_gate_adjoint_rejects_counts_that_are_no_multiple_of_four(n):
    t = [torch.full((1024,), E.GUARD, device=DEV) for _ in range(5)]
    with pytest.raises(SGV3DError):
        _lib.check(_lib.load().sgv3d_add_mul_sigmoid_backward(n, *(v.data_ptr() for v in t), _st()), "rejected call")
    torch.cuda.synchronize()
    assert all(bool((v == E.GUARD).all()) for v in t)
