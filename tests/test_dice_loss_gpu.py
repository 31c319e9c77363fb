"""losses.DiceLoss on the MI355X (csrc/dice_loss.hip): the reference's own float64 values and gradients
(tests/golden/dice_loss.npz) in every layout and label type, known answers bit for bit at every chunk edge of the kernels,
the C ABI's robustness, the autograd contract, a hipGraph of forward + backward, and the dice term of SemanticSupervision.

Bars (tests/dice_ref.py): |loss - ref64| <= max(4 |ref32 - ref64|, 2^-22 max(1, |ref64|)); max |grad - ref64| <=
max(4 max |ref32 - ref64|, 2^-21 max |ref64|), ref32 being the reference's float32 run on the CPU.  Measured on the MI355X:
error / bar at worst 0.29 (median 0.06) for the losses and 0.13 (median 0.05) for the gradients of the 66 fixture runs; the
SemanticSupervision case 0.12 for the loss and 0.29 / 0.33 for the two maps' gradients."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dice_ref
from conftest import GOLDEN
from oracle import focal_ref as R
from sgv3d_amd import _lib, hip_ops
from sgv3d_amd.losses import DiceLoss, FocalLoss, SemanticSupervision, downsample_gt_semantic

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(GOLDEN, "dice_loss.npz"))
CASES = sorted(k[:-5] for k in GOLD.files if k.endswith("_loss"))
LAYOUTS = ("nchw", "nhwc_view", "batch_slice")


def _kw(name):
    return ast.literal_eval(str(GOLD[name + "_kw"]))


def _place(x, layout):
    """``x`` [N, C, *spatial] on the device as a leaf-less view of the given layout (values unchanged)."""
    x = x.to(DEV)
    if layout == "nchw" or x.dim() < 3:
        return x.contiguous()
    last = tuple(range(2, x.dim())) + (1,)
    back = (0, x.dim() - 1) + tuple(range(1, x.dim() - 1))
    if layout == "nhwc_view":                                       # what the training forward hands out
        return x.permute(0, *last).contiguous().permute(*back)
    big = torch.full((x.shape[0] + 3,) + tuple(x.permute(0, *last).shape[1:]), float("nan"), device=DEV)
    big[2:2 + x.shape[0]] = x.permute(0, *last)
    return big[2:2 + x.shape[0]].permute(*back)                      # samples 2.. of a larger channel-last buffer


def _run(loss_fn, x, y):
    x = x.detach().requires_grad_(True)
    loss = loss_fn(x, y)
    loss.backward()
    return loss.detach().cpu(), x.grad.cpu()


# =============================================================================================== fixture cases
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", CASES)
def test_fixture_case(name, layout):
    kw = _kw(name)
    x = _place(torch.from_numpy(GOLD[name + "_x"]), layout)
    y = torch.from_numpy(GOLD[name + "_y"])
    want, want_g = float(GOLD[name + "_loss"]), GOLD[name + "_grad"]
    lbar = dice_ref.loss_bar(want, GOLD[name + "_loss32"])
    gbar = dice_ref.grad_bar(want_g, GOLD[name + "_grad32"])
    kinds = [y] if y.dtype.is_floating_point else [y, y.to(torch.uint8)]
    runs = [_run(DiceLoss(**kw), x, t.to(DEV)) for t in kinds]
    for loss, grad in runs:
        assert loss.dtype == torch.float32 and grad.dtype == torch.float32 and grad.shape == want_g.shape
        lerr = abs(float(loss) - want)
        gerr = float(np.abs(grad.double().numpy() - want_g).max())
        print(f"DICE_RATIO {name} {layout} loss {lerr:.3e} / {lbar:.3e} = {lerr / lbar:.3f}  "
              f"grad {gerr:.3e} / {max(gbar, 1e-300):.3e} = {gerr / gbar if gbar else 0.0:.3f}")
        assert lerr <= lbar, (float(loss), want, lbar)
        assert gerr <= gbar, (gerr, gbar)
        assert torch.isfinite(grad).all()
    if len(runs) == 2:                                              # int64 and uint8 labels: the same bits
        assert runs[0][0].view(torch.int32).item() == runs[1][0].view(torch.int32).item()
        assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    if name == "mc_all_ignored":
        assert float(runs[0][0]) == 0 and not runs[0][1].any()


# =============================================================================================== C ABI helper
def _abi(x, target, kind, act, weight, ignore_index=None, smooth=0.0, eps=1e-7, log_loss=False, ws=None, nws=None, out=None):
    """sgv3d_dice_loss_forward on a view ``x`` [N, C, P]; returns (rc, loss [1], saved [C, 4], call) -- ``call(grad_view,
    upstream)`` runs sgv3d_dice_loss_backward with the same description."""
    lib = _lib.load()
    N, C, P = x.shape
    sb, sc, sp = x.stride()
    need = lib.sgv3d_dice_loss_workspace_bytes(C)
    if ws is None:
        ws = torch.full((max(need, 8) // 8,), float("nan"), dtype=torch.float64, device=DEV)     # a workspace full of NaN
    out = torch.full((1,), -7.0, device=DEV) if out is None else out
    saved = torch.full((C, 4), float("nan"), dtype=torch.float64, device=DEV)
    ign = (0, 0) if ignore_index is None else (int(ignore_index), 1)
    head = (N, C, P, x.data_ptr(), sb, sc, sp, target.data_ptr(), kind, act, ign[0], ign[1], float(smooth), float(eps))
    rc = lib.sgv3d_dice_loss_forward(*head, 1 if log_loss else 0, weight.data_ptr(), out.data_ptr(), saved.data_ptr(),
                                     ws.data_ptr(), need if nws is None else nws, _lib.stream_handle())

    def backward(grad_view, upstream=None):
        assert grad_view.stride() == x.stride()
        return lib.sgv3d_dice_loss_backward(*head, saved.data_ptr(), _lib.ptr(upstream), grad_view.data_ptr(), _lib.stream_handle())
    return rc, out, saved, backward


def _uniform_weight(C):
    return torch.full((C,), 1.0 / C, dtype=torch.float32, device=DEV)


# =============================================================================================== known answers
PIXELS = (1, 3, 4, 5, 255, 256, 257, 1025, 4097)


def _ids(batch, pixels, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, C, (batch, pixels), generator=g)


@pytest.mark.parametrize("C", [2, 7, 8, 19, 32])
def test_known_answers_bit_for_bit(C):
    """pred in {0, 1}: the sums are integers, exact in float64.  pred == onehot gives exactly 0; pred == 1 - onehot with
    smooth = 1 gives sum over the present classes of f32(1/C) * (1 - 1 / (B P + 1)), rounded once to float32."""
    w = float(np.float32(1.0 / C))
    for batch in (1, 3):
        for pixels in PIXELS:
            y = _ids(batch, pixels, C, seed=C * 10007 + pixels * 7 + batch)
            onehot = F.one_hot(y, C).permute(0, 2, 1).float()                      # [B, C, P]
            present = int((onehot.sum(dim=(0, 2)) > 0).sum())
            for labels in (y, y.to(torch.uint8)):
                got = DiceLoss('multiclass', from_logits=False)(onehot.to(DEV), labels.to(DEV))
                assert float(got) == 0.0, (batch, pixels)
                got = DiceLoss('multiclass', from_logits=False, smooth=1.0)((1 - onehot).to(DEV), labels.to(DEV))
                want = np.float32(sum(w * (1.0 - 1.0 / (batch * pixels + 1.0)) for _ in range(present)))
                assert np.float32(float(got)) == want, (batch, pixels, float(got), float(want))


@pytest.mark.parametrize("C", [2, 7, 8, 19, 32])
def test_softmax_kernel_counts_every_pixel_once(C):
    """Logits of +-300 make softmax exactly one-hot, so the three saved sums of a class are exact pixel counts: I where the
    prediction and the label agree, P predictions, T labels -- at every chunk edge, for both label types and both layouts."""
    for batch in (1, 3):
        for pixels in PIXELS:
            y = _ids(batch, pixels, C, seed=C * 31 + pixels + batch)
            pred = _ids(batch, pixels, C, seed=C * 77 + pixels * 3 + batch)
            x = (F.one_hot(pred, C).float() * 600 - 300).to(DEV)                    # [B, P, C] channel-last
            want = torch.zeros(C, 3, dtype=torch.float64)
            for c in range(C):
                want[c, 0] = ((pred == c) & (y == c)).sum()
                want[c, 1] = (pred == c).sum()
                want[c, 2] = (y == c).sum()
            for view in (x.permute(0, 2, 1), x.permute(0, 2, 1).contiguous()):
                for kind, labels in ((1, y.to(DEV)), (0, y.to(torch.uint8).to(DEV))):
                    rc, loss, saved, _ = _abi(view, labels, kind, 2, _uniform_weight(C))
                    _lib.check(rc, "sgv3d_dice_loss_forward")
                    assert torch.equal(saved[:, :3].cpu(), want), (batch, pixels, kind)
                    score = 2 * want[:, 0] / (want[:, 1] + want[:, 2]).clamp_min(1e-7)
                    closed = (float(np.float32(1.0 / C)) * (1 - score) * (want[:, 2] > 0)).sum()
                    assert abs(float(loss) - float(closed)) <= 2.0 ** -23


def test_second_grid_trip_counts_every_pixel_once():
    """More pixels than one trip of the fixed grid covers (256 workgroups x 256 threads): exact counts from the softmax kernel,
    exact known answers from the per-element kernel, and a gradient in every element."""
    C, batch, pixels = 7, 1, 256 * 256 + 257
    y = _ids(batch, pixels, C, seed=1)
    pred = _ids(batch, pixels, C, seed=2)
    x = (F.one_hot(pred, C).float() * 600 - 300).to(DEV)
    rc, loss, saved, backward = _abi(x.permute(0, 2, 1), y.to(torch.uint8).to(DEV), 0, 2, _uniform_weight(C))
    _lib.check(rc, "sgv3d_dice_loss_forward")
    want = torch.stack([torch.stack([((pred == c) & (y == c)).sum(), (pred == c).sum(), (y == c).sum()]) for c in range(C)]).double()
    assert torch.equal(saved[:, :3].cpu(), want)
    grad = torch.full_like(x, float("nan"))
    _lib.check(backward(grad.permute(0, 2, 1)), "sgv3d_dice_loss_backward")
    assert torch.isfinite(grad).all()
    onehot = F.one_hot(y, C).permute(0, 2, 1).float().to(DEV).requires_grad_(True)
    got = DiceLoss('multiclass', from_logits=False)(onehot, y.to(DEV))
    got.backward()
    assert float(got.detach()) == 0.0 and torch.isfinite(onehot.grad).all() and float(onehot.grad.abs().max()) > 0


def test_clamped_denominator_known_answer():
    """multilabel, pred = 0 against a soft target of 1e-9: P + T stays below eps, the loss is exactly 1 and the gradient is
    -2 t / eps (the clamp passes nothing back)."""
    t = torch.full((2, 1, 5, 4), 1e-9)
    x = torch.zeros(2, 1, 5, 4, device=DEV, requires_grad=True)
    loss = DiceLoss('multilabel', from_logits=False)(x, t.to(DEV))
    loss.backward()
    assert float(loss.detach()) == 1.0
    want = np.float32(-2.0 / 1e-7 * float(np.float32(1e-9)))
    assert torch.equal(x.grad.cpu(), torch.full((2, 1, 5, 4), float(want)))


# =============================================================================================== robustness
def test_guard_bands_gaps_nan_buffers_and_repeat():
    """7 of 8 channels of a channel-last buffer, samples 1..2 of 4: the eighth channel, the other samples and the bands around
    the gradient buffer keep their bits; a workspace and a gradient buffer full of NaN give the values of the Python path."""
    name = "mc_log_smooth_ignore"
    kw = _kw(name)
    x = torch.from_numpy(GOLD[name + "_x"])
    y = torch.from_numpy(GOLD[name + "_y"]).to(DEV)
    N, C, H, W = x.shape
    want, want_g = _run(DiceLoss(**kw), x.to(DEV), y)
    store = torch.full((N + 2, H * W, C + 1), 123.0, device=DEV)
    store[1:1 + N, :, :C] = x.permute(0, 2, 3, 1).reshape(N, H * W, C).to(DEV)
    view = store[1:1 + N, :, :C].permute(0, 2, 1)                                     # [N, C, P], strides (P*(C+1), 1, C+1)
    band = 64
    gstore = torch.full((band + store.numel() + band,), float("nan"), device=DEV)
    gbuf = gstore[band:band + store.numel()].view(store.shape)
    gview = gbuf[1:1 + N, :, :C].permute(0, 2, 1)
    results = []
    for _ in range(2):
        gstore.fill_(float("nan"))
        rc, loss, saved, backward = _abi(view, y.reshape(N, -1).contiguous(), 1, 2, _uniform_weight(C), kw['ignore_index'],
                                         kw['smooth'], 1e-7, kw['log_loss'])
        _lib.check(rc, "sgv3d_dice_loss_forward")
        _lib.check(backward(gview), "sgv3d_dice_loss_backward")
        results.append((loss.cpu().clone(), gstore.cpu().clone(), saved.cpu().clone()))
    loss, g, saved = results[0]
    assert loss.view(torch.int32).item() == want.view(torch.int32).item() and torch.isfinite(saved).all()
    gb = g[band:band + store.numel()].view(store.shape)
    assert torch.equal(gb[1:1 + N, :, :C].permute(0, 2, 1).reshape(N, C, H, W).view(torch.int32), want_g.view(torch.int32))
    assert torch.isnan(g[:band]).all() and torch.isnan(g[-band:]).all()               # the guard bands
    assert torch.isnan(gb[0]).all() and torch.isnan(gb[1 + N:]).all() and torch.isnan(gb[1:1 + N, :, C]).all()   # the gaps
    assert bool((store[0] == 123.0).all()) and bool((store[1:1 + N, :, C] == 123.0).all())
    for a, b in zip(results[0], results[1]):                                          # a repeat launch: the same bits
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_short_workspace_and_33_classes_are_refused_before_any_launch():
    lib = _lib.load()
    x = torch.zeros(1, 33, 16, device=DEV)
    y = torch.zeros(1, 16, dtype=torch.uint8, device=DEV)
    rc, out, saved, backward = _abi(x, y, 0, 2, _uniform_weight(33))
    assert rc == -1 and b"2..32" in lib.sgv3d_last_error()
    g = torch.full_like(x, 5.0)
    assert backward(g) == -1 and b"2..32" in lib.sgv3d_last_error()
    rc7, out7, saved7, _ = _abi(x[:, :7], y, 0, 2, _uniform_weight(7), nws=lib.sgv3d_dice_loss_workspace_bytes(7) - 8)
    assert rc7 == -3 and b"workspace too small" in lib.sgv3d_last_error()
    torch.cuda.synchronize()
    assert float(out) == -7.0 and float(out7) == -7.0 and torch.isnan(saved).all() and torch.isnan(saved7).all()
    assert bool((g == 5.0).all())
    with pytest.raises(_lib.SGV3DError, match="not covered"):
        DiceLoss('multiclass')(torch.zeros(1, 33, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError, match="float32"):
        DiceLoss('multiclass')(torch.zeros(1, 7, 4, 4, device=DEV, dtype=torch.bfloat16),
                               torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV))


# =============================================================================================== autograd contract
def _bsm_inputs(seed=0, shape=(2, 7, 9, 12)):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * 3).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    y = torch.randint(0, shape[1], (shape[0],) + shape[2:], generator=g, dtype=torch.uint8)
    return x.to(DEV), y.to(DEV)


def test_no_backward_launch_without_grad_and_upstream_factor(monkeypatch):
    lib = _lib.load()
    real, calls = lib.sgv3d_dice_loss_backward, []

    def spy(*args):
        calls.append(args)
        return real(*args)
    monkeypatch.setattr(lib, "sgv3d_dice_loss_backward", spy)
    x, y = _bsm_inputs(1)
    dice = DiceLoss('multiclass')
    loss = dice(x, y)
    assert not loss.requires_grad and loss.dim() == 0
    w = torch.ones(1, device=DEV, requires_grad=True)
    (dice(x, y) * w).sum().backward()                                # a backward pass that does not reach y_pred
    assert calls == [] and float(w.grad) == float(loss)
    xg = x.clone().requires_grad_(True)
    dice(xg, y).backward()
    assert len(calls) == 1
    x3 = x.clone().requires_grad_(True)
    (3 * dice(x3, y)).backward()
    assert len(calls) == 2 and calls[1][15] is not None             # the upstream scalar went in as a device pointer
    assert torch.equal((3 * xg.grad).view(torch.int32), x3.grad.view(torch.int32))
    assert xg.grad.stride() == xg.stride()


def test_no_device_to_host_copy_in_forward_or_backward():
    x, y = _bsm_inputs(2)
    dice = DiceLoss('multiclass', log_loss=True, smooth=1.0, ignore_index=3, classes=[0, 1, 1, 6])
    soft = DiceLoss('multilabel')
    t = torch.rand(x.shape, device=DEV)
    for fn, tgt in ((dice, y), (soft, t)):                           # the first call builds the class weights (a host copy)
        fn(x.clone().requires_grad_(True), tgt).backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn, tgt in ((dice, y), (soft, t)):
            xg = x.clone().requires_grad_(True)
            (fn(xg, tgt) * 2).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(xg.grad).all()


def test_forward_and_backward_in_one_graph():
    dice = DiceLoss('multiclass', smooth=1.0, ignore_index=255)
    x0, y0 = _bsm_inputs(3)
    sx = x0.clone().requires_grad_(True)
    sy = y0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dice(sx, sy).backward()
    torch.cuda.current_stream().wait_stream(side)
    sx.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sloss = dice(sx, sy)
        sloss.backward()
    for seed in (4, 5):
        x, y = _bsm_inputs(seed)
        y[0, :2] = 255
        with torch.no_grad():
            sx.copy_(x)
            sy.copy_(y)
        graph.replay()
        want, want_g = _run(dice, x, y)
        assert sloss.detach().cpu().view(torch.int32).item() == want.view(torch.int32).item()
        assert torch.equal(sx.grad.cpu().view(torch.int32), want_g.view(torch.int32))


# =============================================================================================== SemanticSupervision
def _semantic_inputs():
    g = torch.Generator().manual_seed(9)
    s0 = torch.randn(2, 8, 12, 7, generator=g) * 2                     # channel-last storage, as the training forward keeps it
    s1 = torch.randn(2, 16, 24, 7, generator=g) * 2
    # the mask is constant over each 8 x 8 block, so that the block-max labels carry every class (independent pixels would
    # leave almost nothing but the largest id)
    cells = torch.randint(0, 7, (2, 1, 16, 24), generator=g, dtype=torch.uint8)
    gt = cells.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)
    assert gt.shape == (2, 1, 128, 192)
    return s0, s1, gt


def _profiled(fn):
    hip_ops.PROFILE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [rec[0] for rec in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = None
    return out, names


def test_semantic_supervision_without_dice_is_unchanged():
    from sgv3d_amd.bsm_grad import upsample_bilinear2x
    s0, s1, gt = _semantic_inputs()
    d0, d1, gtd = s0.to(DEV), s1.to(DEV), gt.to(DEV)
    preds = (d0.permute(0, 3, 1, 2), d1.permute(0, 3, 1, 2))

    def parent():                                                    # SemanticSupervision(8).forward before the dice term existed
        focal = FocalLoss(mode='multiclass', alpha=0.25, gamma=2.0, reduction="mean")
        up = upsample_bilinear2x(preds[0].permute(0, 2, 3, 1))
        labels = downsample_gt_semantic(gtd, 8)
        return (focal(up.permute(0, 3, 1, 2), labels) + focal(preds[1], labels)) / 2
    want, want_names = _profiled(parent)
    for module in (SemanticSupervision(8), SemanticSupervision(8, dice_weight=0.0, dice_kwargs=dict(smooth=1.0))):
        got, names = _profiled(lambda: module(preds, gtd))
        assert names == want_names and names.count("focal_loss") == 2 and not any("dice" in n for n in names)
        assert got.cpu().view(torch.int32).item() == want.cpu().view(torch.int32).item()
    _, names = _profiled(lambda: SemanticSupervision(8, dice_weight=0.5)(preds, gtd))
    assert sorted(names) == sorted(want_names + ["dice_loss", "dice_loss"])


def _semantic_reference(s0, s1, gt, dtype, dice_weight, kw):
    r0 = s0.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    r1 = s1.to(dtype).permute(0, 3, 1, 2).requires_grad_(True)
    up = F.interpolate(r0, scale_factor=2, mode='bilinear')
    labels = R.downsample_gt_semantic(gt, 8)
    loss = R.semantic_loss((r0, r1), gt, 8)
    loss = loss + dice_weight * (dice_ref.dice_loss(up, labels, 'multiclass', **kw) + dice_ref.dice_loss(r1, labels, 'multiclass', **kw)) / 2
    loss.backward()
    return loss.detach(), r0.grad.permute(0, 2, 3, 1), r1.grad.permute(0, 2, 3, 1)


def test_semantic_supervision_with_dice_matches_float64():
    s0, s1, gt = _semantic_inputs()
    kw = dict(smooth=1.0)
    w64, g0_64, g1_64 = _semantic_reference(s0, s1, gt, torch.float64, 0.5, kw)
    w32, g0_32, g1_32 = _semantic_reference(s0, s1, gt, torch.float32, 0.5, kw)
    d0 = s0.to(DEV).requires_grad_(True)
    d1 = s1.to(DEV).requires_grad_(True)
    got = SemanticSupervision(8, dice_weight=0.5, dice_kwargs=kw)((d0.permute(0, 3, 1, 2), d1.permute(0, 3, 1, 2)), gt.to(DEV))
    got.backward()
    lerr, lbar = abs(float(got.detach()) - float(w64)), dice_ref.loss_bar(w64, w32)
    print(f"DICE_SEMANTIC loss {lerr:.3e} / {lbar:.3e} = {lerr / lbar:.3f}")
    rows = []
    for d, g64, g32 in ((d0, g0_64, g0_32), (d1, g1_64, g1_32)):
        assert d.grad is not None and float(d.grad.abs().max()) > 0                  # gradients reach both maps
        gerr = float((d.grad.cpu().double() - g64).abs().max())
        gbar = dice_ref.grad_bar(g64.numpy(), g32.numpy())
        print(f"DICE_SEMANTIC grad {gerr:.3e} / {gbar:.3e} = {gerr / gbar:.3f}")
        rows.append((gerr, gbar))
    assert lerr <= lbar, (float(got.detach()), float(w64), lbar)
    for gerr, gbar in rows:
        assert gerr <= gbar, (gerr, gbar)
    # the dice term is really in: the focal loss alone is far away
    assert abs(float(R.semantic_loss((s0.double().permute(0, 3, 1, 2), s1.double().permute(0, 3, 1, 2)), gt, 8)) - float(got.detach())) > 0.1


def test_bsm_training_step_with_the_dice_term():
    from test_bsm_train_gpu import _model
    from test_train_forward_gpu import _gt
    from sgv3d_amd import synthetic
    B = 2
    model, bconf, hconf = _model(synthetic.small_bsm_conf(depth=18), True, seed=3)
    model = model.cuda().train()
    imgs = synthetic.make_images(B, final=bconf['final_dim'], device='cuda', seed=11)
    mats = synthetic.make_mats(B, device='cuda', scale=128 / 864)
    g = torch.Generator().manual_seed(2)
    gt_sem = torch.randint(0, 7, (B, 1) + tuple(bconf['final_dim']), generator=g, dtype=torch.uint8)
    preds, img_preds = model(imgs, mats)
    semantic = SemanticSupervision(8, dice_weight=0.5)
    (sem_loss, focal_only), names = _profiled(lambda: (semantic(img_preds, gt_sem.cuda()), SemanticSupervision(8)(img_preds, gt_sem.cuda())))
    assert names.count("dice_loss") == 2 and float(sem_loss) > float(focal_only)
    model.head.train_cfg = dict(model.head.train_cfg, grid_size=[256, 256, 1], point_cloud_range=[0, -12.8, -5, 25.6, 12.8, 3])
    boxes, labels = _gt(B)
    targets = model.get_targets([b.cuda() for b in boxes], [l.cuda() for l in labels])
    (model.loss(targets, preds) + sem_loss * 500).backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(gr).all()) for gr in grads)
    assert model.backbone.img_backbone.conv1.weight.grad is None
    assert float(model.backbone.img_backbone.layer1[0].conv1.weight.grad.abs().max()) > 0
