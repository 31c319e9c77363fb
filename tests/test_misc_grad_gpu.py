"""The training adjoints of ``misc_grad`` on the MI355X against plain float64 torch autograd: the stem's max pooling
(csrc/train_misc.hip forward with arg-max bytes + gather adjoint), the trainable stem it sits in, the ASPP image-pooling
branch (``pooled_linear``: dense forward + ``sgv3d_dense_backward_weight``) and the deformable bilinear im2col of the DCN
with its adjoint.

Two kinds of check per section:

* exact inputs (small integers, offsets that are multiples of 1/8, pixel counts that are powers of two): every product and
  partial sum is exact in f32, so the result equals float64 bitwise whatever the order of the float atomics;
* random inputs against the worst-case bound of an f32 evaluation, per element ``|got - want| <= (n + 2) 2^-24 S`` with
  ``S`` the float64 sum of the absolute terms and ``n`` the number of roundings on the longest path from a term to the
  result (accumulation chain plus the roundings inside a term).  One wrong term -- wrong corner, weight, group or window --
  is the size of a term, far above this bound.

Random offsets are multiples of 2^-16 of magnitude <= 3 so that the kernels' f32 sample positions ``(h - 1 + ky) + oy``
(< 2^7 here) are exact: the bound then covers the sampling as well.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_model as TM
from sgv3d_amd import _lib, hip_ops, misc_grad, train_forward
from sgv3d_amd._lib import SGV3DError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _within(got, want, S, n):
    """per element |got - want| <= (n + 2) 2^-24 S (n may be a tensor of per-element chain lengths)."""
    err = (got.double() - want).abs()
    bar = (n + 2) * U * S
    bad = err > bar
    assert not bool(bad.any()), (int(bad.sum()), float(err.max()), float((err - bar).max()))


def _st():
    return _lib.stream_handle(torch.device(DEV))


# ------------------------------------------------------------------------------------------------------ A. max pooling
def _maxpool_train(x):
    """Raw ABI: y and the arg-max tap bytes of the training forward."""
    B, H, W, C = (int(v) for v in x.shape)
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, oh, ow, C, device=DEV)
    idx = torch.empty(B, oh, ow, C, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().sgv3d_maxpool3x3s2_train_forward(B, H, W, C, x.data_ptr(), y.data_ptr(), idx.data_ptr(), _st()),
               "maxpool3x3s2_train_forward")
    return y, idx


def _maxpool_ref(x, dy, dev="cpu"):
    """float64 autograd of F.max_pool2d(3, 2, 1) on NHWC x: (y, window tap of the selected element, dx, dx of |dy|)."""
    B, H, W, C = x.shape
    xr = nchw(x).to(dev, torch.float64).requires_grad_(True)
    y, ind = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    y.backward(nchw(dy).to(dev, torch.float64))
    dx = xr.grad.clone()
    xr.grad = None
    F.max_pool2d(xr, 3, 2, 1).backward(nchw(dy).to(dev, torch.float64).abs())
    oh, ow = y.shape[2], y.shape[3]
    ty = ind // W - (torch.arange(oh, device=dev) * 2 - 1)[:, None]
    tx = ind % W - (torch.arange(ow, device=dev) * 2 - 1)[None, :]
    return nhwc(y.detach()), nhwc(ty * 3 + tx), nhwc(dx), nhwc(xr.grad)


def _maxpool_inputs(B, H, W, C, g):
    ints = torch.randint(0, 3, (B, H, W, C), generator=g).float()               # ties everywhere
    relu = F.relu(torch.randn(B, H, W, C, generator=g))                          # ties at zero
    const = torch.full((B, H, W, C), 1.5)
    special = torch.randn(B, H, W, C, generator=g)
    special[:, :2, :2, 0] = -math.inf                                            # window (0, 0) is all -inf
    special[:, min(1, H - 1), min(1, W - 1), 1] = math.nan                       # one NaN in window (0, 0)
    special[:, 0, 0, 2] = math.nan                                               # two NaNs in window (0, 0)
    special[:, H - 1, W - 1, 2] = math.nan
    special[:, H - 1, W - 1, 3] = -math.inf                                      # -inf beside finite values
    return dict(ints=ints, relu=relu, const=const, randn=torch.randn(B, H, W, C, generator=g), special=special)


def _check_maxpool(x, g, dev="cpu"):
    B, H, W, C = x.shape
    xd = x.to(DEV)
    y, idx = _maxpool_train(xd)
    dy_int = torch.randint(-4, 5, tuple(y.shape), generator=g).float()
    dy_rnd = torch.randn(tuple(y.shape), generator=g)
    y_ref, tap_ref, dx_int_ref, _ = _maxpool_ref(x, dy_int, dev)
    _, _, dx_rnd_ref, S = _maxpool_ref(x, dy_rnd, dev)
    y = y.to(dev)
    assert torch.equal(y.isnan(), y_ref.isnan())
    assert torch.equal(torch.nan_to_num(y.double(), nan=0.0), torch.nan_to_num(y_ref, nan=0.0))
    assert torch.equal(idx.to(dev).long(), tap_ref)
    # the autograd function: y of its forward and dx of its adjoint (at most four windows per element, exact terms)
    xg = xd.clone().requires_grad_(True)
    yf = misc_grad.maxpool3x3s2(xg)
    assert torch.equal(yf.detach().isnan(), y.isnan().to(DEV))
    yf.backward(dy_int.to(DEV))
    assert torch.equal(xg.grad.to(dev).double(), dx_int_ref)
    xg.grad = None
    yf = misc_grad.maxpool3x3s2(xg)
    yf.backward(dy_rnd.to(DEV))
    first = xg.grad.clone()
    _within(first.to(dev), dx_rnd_ref, S, 4)
    xg.grad = None
    misc_grad.maxpool3x3s2(xg).backward(dy_rnd.to(DEV))
    assert torch.equal(xg.grad, first)                                           # gather form: bitwise repeatable
    # eval mode and train mode of the layer agree, NaN included
    inf = hip_ops.maxpool3x3s2(xd)
    assert torch.equal(inf.isnan(), yf.detach().isnan())
    assert torch.equal(torch.nan_to_num(inf, nan=0.0), torch.nan_to_num(yf.detach(), nan=0.0))
    if not bool(x.isnan().any()):
        assert torch.equal(inf, yf.detach())


@pytest.mark.parametrize("hw", [(1, 2), (2, 1), (1, 1), (2, 3), (3, 4), (4, 5), (5, 8), (8, 3), (8, 8)])
def test_maxpool_training_pair(hw):
    """y == F.max_pool2d (NaN masks too), the arg-max byte == torch's index as a window tap (first maximum in row-major
    window order, last NaN), dx == float64 autograd bitwise on integer dy and within the gather's bound on random dy,
    dx bitwise repeatable, train forward == inference kernel."""
    H, W = hw
    g = torch.Generator().manual_seed(H * 16 + W)
    for B, C in ((1, 4), (3, 8), (1, 64), (3, 68)):
        for x in _maxpool_inputs(B, H, W, C, g).values():
            _check_maxpool(x, g)


def test_maxpool_training_pair_stem_size():
    """The cfg-2 stem map 2 x 432 x 768 x 64 (reference on the device, float64)."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 432, 768, 64, generator=g)
    x[:, 100:140, 200:260] = F.relu(x[:, 100:140, 200:260])                      # a patch of ties at zero
    _check_maxpool(x, g, dev=DEV)


# ------------------------------------------------------------------------------------------------------ B. trainable stem
def test_trainable_stem_gradients():
    """frozen_stages=-1 (mmdet's default): conv1 + bn1 (batch statistics) + ReLU + max pooling of ``train_forward.resnet``
    through the HIP adjoints, against float64 F.conv2d -> F.batch_norm(training) -> relu -> F.max_pool2d.  Bars of
    test_norm_grad_gpu; the image is small so that f32 near-ties inside a window are improbable."""
    from sgv3d_amd.layers.blocks import ResNet
    torch.manual_seed(3)
    r = ResNet(depth=18, frozen_stages=-1, norm_eval=False).cuda().train()
    assert not r.frozen_stem()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        r.bn1.weight.copy_(1 + 0.3 * torch.randn(64, generator=g))
        r.bn1.bias.copy_(0.2 * torch.randn(64, generator=g))
    img = torch.randn(2, 3, 40, 56, generator=g)
    x = F.pad(nhwc(img), (0, 1)).to(DEV)                                         # 3 channels padded to 4, as resnet() gets them
    y = misc_grad.maxpool3x3s2(train_forward.bn(r.bn1, train_forward.conv(r.conv1, x), relu=True))
    dy = torch.randn(tuple(y.shape), generator=g)
    y.backward(dy.to(DEV))

    w = r.conv1.weight.detach().cpu().double().requires_grad_(True)
    gw = r.bn1.weight.detach().cpu().double().requires_grad_(True)
    gb = r.bn1.bias.detach().cpu().double().requires_grad_(True)
    h = F.conv2d(img.double(), w, None, 2, 3)
    h = F.batch_norm(h, torch.zeros(64, dtype=torch.float64), torch.ones(64, dtype=torch.float64), gw, gb, True, 0.1, r.bn1.eps)
    ref = F.max_pool2d(F.relu(h), 3, 2, 1)
    ref.backward(nchw(dy).double())
    assert float((nchw(y.detach().cpu()).double() - ref.detach()).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))
    for name, got, want in (("conv1.weight", r.conv1.weight.grad, w.grad), ("bn1.weight", r.bn1.weight.grad, gw.grad),
                            ("bn1.bias", r.bn1.bias.grad, gb.grad)):
        err = float((got.cpu().double() - want).abs().max())
        assert err <= 1e-4 * max(1.0, float(want.abs().max())), (name, err)


# ------------------------------------------------------------------------------------------------------ C. pooled linear
def _pool_chain(P):
    """roundings on the longest path of global_avgpool: lane loop over ceil(P / 32) / 4 pixels, two pair sums, 32 chunk
    partials, the division by P."""
    return math.ceil(math.ceil(P / 32) / 4) + 2 + 32 + 1


def _pooled_linear_case(B, H, W, C, N, exact, g):
    if exact:
        x = torch.randint(-3, 4, (B, H, W, C), generator=g).float()
        w = torch.randint(-3, 4, (N, C, 1, 1), generator=g).float()
        dy = torch.randint(-3, 4, (B, N), generator=g).float()
    else:
        x = torch.randn(B, H, W, C, generator=g)
        w = torch.randn(N, C, 1, 1, generator=g) / C ** 0.5
        dy = torch.randn(B, N, generator=g)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y = misc_grad.pooled_linear(xg, wg)
    y.backward(dy.to(DEV))

    def ref(x, w, dy):
        xr = nchw(x).to(DEV, torch.float64).requires_grad_(True)
        wr = w.to(DEV, torch.float64).requires_grad_(True)
        yr = F.conv2d(F.adaptive_avg_pool2d(xr, 1), wr).reshape(B, N)
        yr.backward(dy.to(DEV, torch.float64))
        return yr.detach(), nhwc(xr.grad), wr.grad.reshape(N, C)

    y_ref, dx_ref, dw_ref = ref(x, w, dy)
    dw = wg.grad.reshape(N, C)
    if exact:
        assert torch.equal(y.detach().double(), y_ref)
        assert torch.equal(xg.grad.double(), dx_ref)
        assert torch.equal(dw.double(), dw_ref)
        return
    # S: the same computation on absolute values (float64)
    ya, dxa, dwa = ref(x.abs(), w.abs(), dy.abs())
    P = H * W
    _within(y.detach(), y_ref, ya, _pool_chain(P) + math.ceil(C / 64) + 6)     # + dense: lane loop + butterfly
    _within(xg.grad, dx_ref, dxa, math.ceil(N / 64) + 6 + 2)                     # dense, f32(1 / P), the product
    _within(dw, dw_ref, dwa, _pool_chain(P) + B)                                 # pooled error + the batch chain


@pytest.mark.parametrize("shape", [
    (1, 54, 96, 512, 512), (2, 54, 96, 512, 512), (8, 54, 96, 512, 512),       # the ASPP image-pooling branch
    (1, 54, 96, 256, 256), (2, 54, 96, 256, 256), (8, 54, 96, 256, 256),
    (3, 1, 1, 100, 36),                                                          # H = W = 1; N, K, N*K off 64 / 256
    (2, 5, 7, 68, 20),
    (5, 3, 9, 132, 70),
])
def test_pooled_linear(shape):
    """forward, dx and dw of the ASPP image pooling (global average + bias-free 1x1 conv) against float64
    F.conv2d(F.adaptive_avg_pool2d(x, 1), w) within the derived bound; bitwise on small integers over 2^k pixels."""
    g = torch.Generator().manual_seed(sum(shape))
    _pooled_linear_case(*shape, exact=False, g=g)


@pytest.mark.parametrize("shape", [(2, 8, 16, 512, 512), (3, 1, 1, 100, 36), (8, 4, 4, 68, 20)])
def test_pooled_linear_exact_on_integers(shape):
    g = torch.Generator().manual_seed(sum(shape))
    _pooled_linear_case(*shape, exact=True, g=g)


def test_dense_backward_weight_raw():
    """sgv3d_dense_backward_weight alone: dW[n][k] = sum_b dY[b][n] X[b][k], bound with the batch chain; N*K not a multiple of
    the 256-thread block; bitwise on integers."""
    g = torch.Generator().manual_seed(8)
    lib = _lib.load()
    for B, K, N in ((1, 7, 3), (8, 512, 512), (5, 100, 37), (16, 33, 65)):
        for exact in (True, False):
            x = torch.randint(-4, 5, (B, K), generator=g).float() if exact else torch.randn(B, K, generator=g)
            dy = torch.randint(-4, 5, (B, N), generator=g).float() if exact else torch.randn(B, N, generator=g)
            xd, dyd = x.to(DEV), dy.to(DEV)
            dw = torch.full((N * K + 64,), 7.0, device=DEV)
            _lib.check(lib.sgv3d_dense_backward_weight(B, K, N, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), _st()),
                       "dense_backward_weight")
            assert bool((dw[N * K:] == 7.0).all())
            want = dy.double().t() @ x.double()
            got = dw[:N * K].reshape(N, K).cpu()
            if exact:
                assert torch.equal(got.double(), want)
            else:
                _within(got, want, dy.double().abs().t() @ x.double().abs(), B)


# ------------------------------------------------------------------------------------------------------ D. deformable im2col
def _col_to_ref(col, B, H, W, C, groups):
    """kernel layout [B, H, W, groups, 9, C / groups] -> the oracle's [B, C, 9, H, W]"""
    return col.reshape(B, H, W, groups, 9, C // groups).permute(0, 3, 5, 4, 1, 2).reshape(B, C, 9, H, W)


def _ref_to_col(col, B, H, W, C, groups):
    return col.reshape(B, groups, C // groups, 9, H, W).permute(0, 4, 5, 1, 3, 2).reshape(B, H, W, 9 * C)


def _contributions(off, H, W):
    """[B, H, W]: how many (pixel, tap, corner) scatters of the adjoint land on each input pixel (a corner outside the image
    does not scatter; a zero-weight corner inside does)."""
    B = off.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    n = torch.zeros(B, H * W, dtype=torch.float64)
    for t in range(9):
        hf = ys - 1 + t // 3 + off[..., 2 * t].double()
        wf = xs - 1 + t % 3 + off[..., 2 * t + 1].double()
        inside = (hf > -1) & (wf > -1) & (hf < H) & (wf < W)
        for dh in (0, 1):
            for dw in (0, 1):
                hh, ww = torch.floor(hf).long() + dh, torch.floor(wf).long() + dw
                ok = inside & (hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= W - 1)
                n.scatter_add_(1, (hh.clamp(0, H - 1) * W + ww.clamp(0, W - 1)).reshape(B, -1), ok.double().reshape(B, -1))
    return n.reshape(B, H, W, 1)


def _dcn_ref(x, off, dcol_k, groups, dev):
    """float64 autograd of the oracle's deform_im2col3x3: (col, dx, doff) in the kernel layouts."""
    B, H, W, C = x.shape
    xr = nchw(x).to(dev, torch.float64).requires_grad_(True)
    orr = nchw(off[..., :18]).to(dev, torch.float64).requires_grad_(True)
    col = TM.deform_im2col3x3(xr, orr)
    col.backward(_col_to_ref(dcol_k.to(dev, torch.float64), B, H, W, C, groups))
    return _ref_to_col(col.detach(), B, H, W, C, groups), nhwc(xr.grad), nhwc(orr.grad)


def _doff_scale(x, off, dcol_k, groups, dev):
    """S of d off[2t] and d off[2t+1]: sum_c |dcol| (hw |v3 - v1| + lw |v4 - v2|) <= sum_c |dcol| (hw (|v1| + |v3|) + ...),
    i.e. |dcol| against the samples of |x| taken on the two grid rows (columns) that bracket the sample -- the oracle's
    im2col at offsets moved to floor(hf) - base and floor(hf) + 1 - base."""
    B, H, W, C = x.shape
    xa = nchw(x).to(dev, torch.float64).abs()
    o = nchw(off[..., :18]).to(dev, torch.float64)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                            indexing="ij")
    da = _col_to_ref(dcol_k.to(dev, torch.float64), B, H, W, C, groups).abs()
    S = []
    for axis in (0, 1):                                                          # 0: d/dy (rows), 1: d/dx (columns)
        tot = 0
        for up in (0, 1):
            moved = o.clone()
            for t in range(9):
                base = (ys if axis == 0 else xs) - 1 + (t // 3 if axis == 0 else t % 3)
                moved[:, 2 * t + axis] = torch.floor(base + o[:, 2 * t + axis]) + up - base
            tot = tot + (da * TM.deform_im2col3x3(xa, moved)).sum(1)             # [B, 9, H, W]
        S.append(tot)
    return torch.stack(S, 2).permute(0, 3, 4, 1, 2).reshape(B, H, W, 18)         # [B, H, W, (tap, axis)]


def _edge_offsets(B, H, W, g):
    """offsets that put every sample on -1, 0, H-1, H (rows) / -1, 0, W-1, W (columns) or 2^-10 either side of one"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    rows = torch.tensor([-1.0, 0.0, H - 1.0, float(H)])
    cols = torch.tensor([-1.0, 0.0, W - 1.0, float(W)])
    nudge = torch.tensor([-2.0 ** -10, 0.0, 2.0 ** -10])
    off = torch.empty(B, H, W, 18)
    for t in range(9):
        th = rows[torch.randint(0, 4, (B, H, W), generator=g)] + nudge[torch.randint(0, 3, (B, H, W), generator=g)]
        tw = cols[torch.randint(0, 4, (B, H, W), generator=g)] + nudge[torch.randint(0, 3, (B, H, W), generator=g)]
        off[..., 2 * t] = th - (ys - 1 + t // 3)
        off[..., 2 * t + 1] = tw - (xs - 1 + t % 3)
    return off


def _offsets(kind, B, H, W, g):
    if kind == "zero":
        return torch.zeros(B, H, W, 18)
    if kind == "int":
        return torch.randint(-2, 3, (B, H, W, 18), generator=g).float()
    if kind == "eighths":
        return torch.randint(-24, 25, (B, H, W, 18), generator=g).float() / 8
    if kind == "edge":
        return _edge_offsets(B, H, W, g)
    if kind == "uniform":
        return torch.round((torch.rand(B, H, W, 18, generator=g) * 6 - 3) * 2 ** 16) / 2 ** 16
    if kind == "far":
        return torch.where(torch.rand(B, H, W, 18, generator=g) < 0.5, -40.0, 40.0) + torch.rand(B, H, W, 18, generator=g)
    raise ValueError(kind)


def _dcn_run(x, off, dcol, groups):
    xg = x.to(DEV).requires_grad_(True)
    og = off.to(DEV).requires_grad_(True)
    col = misc_grad.deform_im2col3x3(xg, og, groups)
    col.backward(dcol.to(DEV))
    return col.detach(), xg.grad, og.grad


def _check_dcn(B, H, W, C, groups, kind, g, dev="cpu"):
    off = _offsets(kind, B, H, W, g)
    exact = kind in ("zero", "int", "eighths", "far")                           # every product and sum exact in f32
    if exact:
        x = torch.randint(-4, 5, (B, H, W, C), generator=g).float()
        dcol = torch.randint(-4, 5, (B, H, W, 9 * C), generator=g).float()
    else:
        x = torch.randn(B, H, W, C, generator=g)
        dcol = torch.randn(B, H, W, 9 * C, generator=g)
    col, dx, doff = _dcn_run(x, off, dcol, groups)
    col_ref, dx_ref, doff_ref = _dcn_ref(x, off, dcol, groups, dev)
    col, dx, doff = col.to(dev), dx.to(dev), doff.to(dev)
    if kind == "far":
        assert not bool(col.any()) and not bool(dx.any()) and not bool(doff.any())
    if exact:
        assert torch.equal(col.double(), col_ref)
        assert torch.equal(dx.double(), dx_ref)
        assert torch.equal(doff.double(), doff_ref)
    else:
        Sc = _ref_to_col(TM.deform_im2col3x3(nchw(x).to(dev, torch.float64).abs(), nchw(off).to(dev, torch.float64)),
                         B, H, W, C, groups)
        _within(col, col_ref, Sc, 5)                                             # weight product, 4 products / sums
        _, Sdx, _ = _dcn_ref(x, off, dcol.abs(), groups, dev)                   # corner weights >= 0: exact S
        _within(dx, dx_ref, Sdx, _contributions(off, H, W).to(dev) + 2)         # atomics + weight product + w * d
        _within(doff, doff_ref, _doff_scale(x, off, dcol, groups, dev), math.ceil(C / 64) + 6 + 4)
    # the offset gradient is a fixed-order reduction: bitwise repeatable (dx uses atomics: checked against the reference only)
    _, _, again = _dcn_run(x, off, dcol, groups)
    assert torch.equal(again.to(dev), doff)


DCN_SHAPES = [
    # (B, H, W, C, groups)
    (2, 5, 7, 4, 1), (1, 6, 5, 8, 2), (2, 4, 6, 16, 4),                         # C = 4 groups
    (2, 7, 9, 64, 1), (1, 6, 7, 64, 4),
    (2, 5, 6, 68, 1), (1, 6, 5, 196, 1),                                         # partial last pass of the lane loop
    (1, 5, 4, 512, 4),
    (2, 1, 7, 64, 4), (1, 6, 1, 68, 1), (2, 2, 2, 16, 4), (1, 1, 1, 8, 2),      # H or W = 1 or 2
]


@pytest.mark.parametrize("shape", DCN_SHAPES)
@pytest.mark.parametrize("kind", ["zero", "int", "eighths", "edge", "uniform", "far"])
def test_deform_im2col_adjoint(shape, kind):
    """col, dx, doff of the deformable im2col against float64 autograd of the oracle's deform_im2col3x3: bitwise on
    integer / eighth offsets with integer data (and the far-out regime: all zero), within the derived bound otherwise;
    doff bitwise repeatable."""
    B, H, W, C, groups = shape
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + C + groups + len(kind))
    _check_dcn(B, H, W, C, groups, kind, g)


@pytest.mark.parametrize("kind", ["zero", "uniform"])
def test_deform_im2col_adjoint_cfg2_layer(kind):
    """the cfg-2 DCN at 2 x 54 x 96 x 512, groups 4 (reference on the device, float64)"""
    g = torch.Generator().manual_seed(54 + len(kind))
    _check_dcn(2, 54, 96, 512, 4, kind, g, dev=DEV)


def test_deform_im2col_backward_raw_abi_strides():
    """off_ld = 27 and grad_off_ld = 24 through the C ABI: the offsets are read from the first 18 columns of a wider row, the
    gradient columns 18 and up keep what they held, and dx is fully written (zeroed first)."""
    g = torch.Generator().manual_seed(27)
    B, H, W, C, groups = 2, 5, 6, 64, 4
    x = torch.randint(-4, 5, (B, H, W, C), generator=g).float()
    off = _offsets("eighths", B, H, W, g)
    dcol = torch.randint(-4, 5, (B, H, W, 9 * C), generator=g).float()
    wide = torch.cat([off, torch.full((B, H, W, 9), 1e6)], -1).to(DEV)           # junk beyond column 18 must not be read
    doff = torch.full((B, H, W, 24), -3.25, device=DEV)
    dx = torch.full((B, H, W, C), 5.5, device=DEV)
    xd, dd = x.to(DEV), dcol.to(DEV)
    _lib.check(_lib.load().sgv3d_deform_im2col3x3_backward(B, H, W, C, groups, xd.data_ptr(), wide.data_ptr(), 27, dd.data_ptr(),
                                                          dx.data_ptr(), doff.data_ptr(), 24, _st()),
               "deform_im2col3x3_backward")
    _, dx_ref, doff_ref = _dcn_ref(x, off, dcol, groups, "cpu")
    assert torch.equal(dx.cpu().double(), dx_ref)
    assert torch.equal(doff[..., :18].cpu().double(), doff_ref)
    assert bool((doff[..., 18:] == -3.25).all())


def test_abi_rejections_before_launch():
    """bad shapes, short leading dimensions and null pointers raise SGV3DError and launch nothing (outputs keep their fill)."""
    lib, st = _lib.load(), _st()
    B, H, W = 1, 4, 4
    x = torch.randn(B, H, W, 16, device=DEV)
    off = torch.zeros(B, H, W, 18, device=DEV)
    dcol = torch.randn(B, H, W, 9 * 16, device=DEV)
    dx = torch.full((B, H, W, 16), 9.0, device=DEV)
    doff = torch.full((B, H, W, 18), 9.0, device=DEV)
    P = lambda t: t.data_ptr()
    bad = [
        lambda: lib.sgv3d_deform_im2col3x3_backward(B, H, W, 8, 4, P(x), P(off), 18, P(dcol), P(dx), P(doff), 18, st),   # 8 % 16
        lambda: lib.sgv3d_deform_im2col3x3_backward(B, H, W, 12, 2, P(x), P(off), 18, P(dcol), P(dx), P(doff), 18, st),  # 12 % 8
        lambda: lib.sgv3d_deform_im2col3x3_backward(B, H, W, 16, 4, P(x), P(off), 17, P(dcol), P(dx), P(doff), 18, st),
        lambda: lib.sgv3d_deform_im2col3x3_backward(B, H, W, 16, 4, P(x), P(off), 18, P(dcol), P(dx), P(doff), 17, st),
        lambda: lib.sgv3d_deform_im2col3x3_backward(B, H, W, 16, 4, None, P(off), 18, P(dcol), P(dx), P(doff), 18, st),
        lambda: lib.sgv3d_deform_im2col3x3_backward(B, H, W, 16, 4, P(x), P(off), 18, P(dcol), P(dx), None, 18, st),
        lambda: lib.sgv3d_maxpool3x3s2_train_forward(B, H, W, 6, P(x), P(dx), P(doff), st),                         # C % 4
        lambda: lib.sgv3d_maxpool3x3s2_train_forward(B, H, W, 16, P(x), P(dx), None, st),
        lambda: lib.sgv3d_maxpool3x3s2_backward(B, H, W, 6, P(doff), P(x), P(dx), st),
        lambda: lib.sgv3d_maxpool3x3s2_backward(B, 0, W, 16, P(doff), P(x), P(dx), st),
        lambda: lib.sgv3d_maxpool3x3s2_backward(B, H, W, 16, None, P(x), P(dx), st),
        lambda: lib.sgv3d_dense_backward_weight(0, 16, 16, P(x), P(x), P(dx), st),
        lambda: lib.sgv3d_dense_backward_weight(1, 16, 16, P(x), None, P(dx), st),
    ]
    for call in bad:
        with pytest.raises(SGV3DError):
            _lib.check(call(), "rejected call")
    torch.cuda.synchronize()
    assert bool((dx == 9.0).all()) and bool((doff == 9.0).all())


@pytest.mark.parametrize("init", ["zero", "perturbed"])
def test_deform_conv_layer_gradients(init):
    """``train_forward.deform_conv`` (offset conv + deformable im2col + per-group GEMMs) forward and backward against float64
    autograd of the oracle's deform_conv3x3 with the offsets from a float64 F.conv2d: gradients of x, the DCN weight and
    conv_offset's weight and bias to 2e-5 x max|ref| (the bars of test_conv_grad_gpu).  ``zero`` is the from-scratch state
    (conv_offset zero-initialised: every sample on an integer pixel, floor's one-sided derivative); ``perturbed`` moves
    the samples off the grid."""
    from sgv3d_amd.layers.backbones.lss_fpn import DCN
    torch.manual_seed(7)
    B, H, W, C, groups = 2, 9, 11, 64, 4
    dcn = DCN(C, C, 3, padding=1, groups=groups)
    g = torch.Generator().manual_seed(70 + len(init))
    if init == "perturbed":
        with torch.no_grad():
            dcn.conv_offset.weight.copy_(0.05 * torch.randn(tuple(dcn.conv_offset.weight.shape), generator=g))
            dcn.conv_offset.bias.copy_(0.5 * torch.randn(18, generator=g))
    dcn = dcn.cuda().train()
    x = torch.randn(B, H, W, C, generator=g)
    dy = torch.randn(B, H, W, C, generator=g)
    xg = x.to(DEV).requires_grad_(True)
    y = train_forward.deform_conv(dcn, xg)
    y.backward(dy.to(DEV))

    p64 = lambda t: t.detach().cpu().double().requires_grad_(True)
    xr, wr, owr, obr = p64(nchw(x)), p64(dcn.weight), p64(dcn.conv_offset.weight), p64(dcn.conv_offset.bias)
    offset = F.conv2d(xr, owr, obr, 1, 1)
    ref = TM.deform_conv3x3(xr, offset, wr, groups)
    ref.backward(nchw(dy).double())
    assert float((nchw(y.detach().cpu()).double() - ref.detach()).abs().max()) <= 1e-5 * float(ref.abs().max())
    for name, got, want in (("x", nchw(xg.grad.cpu()), xr.grad), ("weight", dcn.weight.grad, wr.grad),
                            ("conv_offset.weight", dcn.conv_offset.weight.grad, owr.grad),
                            ("conv_offset.bias", dcn.conv_offset.bias.grad, obr.grad)):
        err = float((got.cpu().double() - want).abs().max())
        assert err <= 2e-5 * float(want.abs().max()), (name, err, float(want.abs().max()))
