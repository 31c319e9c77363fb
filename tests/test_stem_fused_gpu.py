"""GPU: the image stem in one launch (csrc/stem_pool_x3.hip, sgv3d_stem_pool_x3_forward, hip_ops.stem_fused): NCHW image -> 7x7 /
stride 2 convolution + folded BN + ReLU -> 3x3 / stride 2 max-pool -> NHWC map.

The bar is bit equality with the three launches it replaces when the convolution runs on the f32x3 tap-major kernel: the
``nchw_to_nhwc(c_pad=4)`` copy, sgv3d_conv2d_x3_forward (MODE 2 of csrc/conv_pw_x3.hip) on a fixed tile without split-K, and
``maxpool3x3s2``.  The fused kernel's tile is TP_H x TP_W = 4 x 16 pooled pixels."""
import copy
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = (0,)                                # sgv3d_stem_pool_x3_forward's variant codes
TILE_X3 = 64
GUARD = 256                                    # floats of poison before and after the output buffer
POISON = -7.0
PACK_BYTES = 4 * 7 * 3 * 512 * 2


def _ptr(t):
    return None if t is None else t.data_ptr()


def _pack(lib, w):
    """The w_pw_x3 pack of a [64, 3, 7, 7] weight: k order 0 (k = tap * 4 + ci), K = 196 padded to 224."""
    wd = w.to(DEV).contiguous()
    u = torch.empty(4, 7, 3, 512, dtype=torch.bfloat16, device=DEV)
    assert lib.sgv3d_conv_pack_weight_x3(wd.data_ptr(), 64, 3, 7, 7, 4, 64, u.data_ptr(), None) == 0, lib.sgv3d_last_error()
    torch.cuda.synchronize()                   # (the packer reads ``wd`` asynchronously)
    return u


def _out_hw(h, w):
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return hc, wc, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1


def unfused(lib, x, u, scale, shift, x3_variant=5):
    """The three launches: NHWC copy padded to 4 channels, the x3 tap-major convolution (tile variant ``x3_variant``, no split-K,
    ReLU), the max-pool."""
    from sgv3d_amd import hip_ops
    from sgv3d_amd._lib import ConvDesc, CONV_NORMAL
    B, _, H, W = x.shape
    hc, wc, _, _ = _out_hw(H, W)
    x4 = hip_ops.nchw_to_nhwc(x, c_pad=4)
    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin, d.out_h, d.out_w, d.cout = B, H, W, 4, hc, wc, 64
    d.kh, d.kw, d.stride, d.pad, d.dil = 7, 7, 2, 3, 1
    d.x_ld, d.x_coff, d.y_ld, d.y_coff, d.res_ld, d.relu = 4, 0, 64, 0, 0, 1
    d.mode, d.deconv_ks, d.split_k, d.tile, d.k_pad, d.cout_pad, d.k_order = CONV_NORMAL, 0, 1, TILE_X3 | x3_variant, 224, 64, 0
    y = torch.empty(B, hc, wc, 64, device=DEV)
    assert lib.sgv3d_conv2d_x3_forward(ctypes.byref(d), x4.data_ptr(), u.data_ptr(), _ptr(scale), _ptr(shift), None, y.data_ptr(), None, 0,
                                       None) == 0, lib.sgv3d_last_error()
    return hip_ops.maxpool3x3s2(y)


def fused(lib, x, u, scale, shift, variant=0, y_ld=64):
    """The fused launch into a map of ``y_ld`` channels with poisoned guard bands around it: (whole buffer, map view)."""
    B, _, H, W = x.shape
    _, _, hp, wp = _out_hw(H, W)
    numel = B * hp * wp * y_ld
    buf = torch.full((GUARD + numel + GUARD,), POISON, device=DEV)
    y = buf[GUARD:GUARD + numel].view(B, hp, wp, y_ld)
    assert lib.sgv3d_stem_pool_x3_forward(B, H, W, x.data_ptr(), u.data_ptr(), PACK_BYTES, _ptr(scale), _ptr(shift), y.data_ptr(), y_ld,
                                          variant, None) == 0, lib.sgv3d_last_error()
    return buf, y


def _guards_untouched(buf, y):
    assert bool((buf[:GUARD] == POISON).all()) and bool((buf[-GUARD:] == POISON).all())
    if y.shape[-1] > 64:
        assert float(y[..., 64:].max()) == POISON == float(y[..., 64:].min())


@pytest.fixture(scope="module")
def stem(hip):
    """One weight set: Kaiming weights, BN scale / shift with both signs; its pack."""
    lib = hip.load()
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 3, 7, 7, generator=g) * (2.0 / (64 * 49)) ** 0.5
    scale = torch.rand(64, generator=g) + 0.5
    scale[::5] *= -1.0
    shift = torch.randn(64, generator=g) * 0.3
    return dict(lib=lib, w=w, scale=scale, shift=shift, u=_pack(lib, w), scale_d=scale.to(DEV), shift_d=shift.to(DEV))


def _image(B, H, W, seed):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))


# pooled heights {1, 3, 4, 5, 9} x pooled widths {1, 15, 16, 17, 33} (1, TP - 1, TP, TP + 1, 2 TP + 1 of the 4 x 16 tile), every
# residue mod 4 in both dimensions, both parities of the conv map's sizes
EDGE_H = (3, 10, 16, 17, 33)
EDGE_W = (1, 58, 64, 67, 130)
FLOOR = ((1, 1), (7, 9), (8, 8), (9, 10), (37, 53))


@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_launch_is_bit_equal_to_the_three_launches_on_every_edge_geometry(stem, variant):
    lib, u = stem["lib"], stem["u"]
    shapes = list(itertools.product(EDGE_H, EDGE_W)) + list(FLOOR)
    assert {_out_hw(h, 1)[2] for h in EDGE_H} == {1, 3, 4, 5, 9} and {_out_hw(1, w)[3] for w in EDGE_W} == {1, 15, 16, 17, 33}
    assert {h % 4 for h in EDGE_H} == {0, 1, 2, 3} == {w % 4 for w in EDGE_W}
    for i, (H, W) in enumerate(shapes):
        B = 1 + i % 3
        x = _image(B, H, W, 100 + i).to(DEV)
        for affine in (True, False):
            sc, sh = (stem["scale_d"], stem["shift_d"]) if affine else (None, None)
            want = unfused(lib, x, u, sc, sh, x3_variant=(5, 0, 6)[i % 3])
            buf, y = fused(lib, x, u, sc, sh, variant, y_ld=64 if i % 2 else 80)
            assert tuple(y.shape[:3]) == tuple(want.shape[:3])
            assert torch.equal(y[..., :64], want), (H, W, B, affine, float((y[..., :64] - want).abs().max()))
            _guards_untouched(buf, y)


@pytest.mark.parametrize("variant", VARIANTS)
def test_an_image_of_several_tiles_in_both_dimensions(stem, variant):
    """150 x 298 at batch 3: 10 x 5 tiles per image, partial ones on the bottom and right edges."""
    lib, u = stem["lib"], stem["u"]
    x = _image(3, 150, 298, 7).to(DEV)
    want = unfused(lib, x, u, stem["scale_d"], stem["shift_d"])
    buf, y = fused(lib, x, u, stem["scale_d"], stem["shift_d"], variant, y_ld=72)
    assert tuple(want.shape) == (3, 38, 75, 64)
    assert torch.equal(y[..., :64], want)
    _guards_untouched(buf, y)


@pytest.mark.parametrize("variant", VARIANTS)
def test_negative_images_and_a_stem_that_is_negative_everywhere(stem, variant):
    lib, u = stem["lib"], stem["u"]
    x = (-_image(2, 37, 53, 8).abs() - 0.1).to(DEV)                      # an all-negative image
    want = unfused(lib, x, u, stem["scale_d"], stem["shift_d"])
    buf, y = fused(lib, x, u, stem["scale_d"], stem["shift_d"], variant, y_ld=80)
    assert torch.equal(y[..., :64], want) and float(want.max()) > 0.0
    _guards_untouched(buf, y)
    # positive weights on a positive image under a negative scale and shift: every conv value is below zero, ReLU makes it 0 and the
    # pooled map is exactly 0 -- were the pool's padding (or a pixel outside the conv map) read as a value, it would not be
    g = torch.Generator().manual_seed(9)
    w = torch.rand(64, 3, 7, 7, generator=g) + 0.01
    u_pos = _pack(lib, w)
    scale, shift = torch.full((64,), -1.0, device=DEV), torch.full((64,), -0.5, device=DEV)
    for H, W in ((37, 53), (9, 10), (16, 130)):
        x = (_image(2, H, W, 10).abs() + 0.1).to(DEV)
        buf, y = fused(lib, x, u_pos, scale, shift, variant, y_ld=80)
        assert bool((y[..., :64] == 0.0).all())
        assert torch.equal(y[..., :64], unfused(lib, x, u_pos, scale, shift))
        _guards_untouched(buf, y)


@pytest.mark.parametrize("variant", VARIANTS)
def test_non_finite_pixels(stem, variant):
    """One NaN pixel and one Inf pixel: the non-finite outputs are those of the three launches, everything else is bit-equal."""
    lib, u = stem["lib"], stem["u"]
    x = _image(2, 37, 53, 12)
    x[0, 1, 20, 30] = float("nan")
    x[1, 2, 5, 44] = float("inf")
    x = x.to(DEV)
    for sc, sh in ((stem["scale_d"], stem["shift_d"]), (None, None)):
        want = unfused(lib, x, u, sc, sh)
        _, y = fused(lib, x, u, sc, sh, variant)
        bad_want, bad_got = ~torch.isfinite(want), ~torch.isfinite(y)
        assert torch.equal(bad_want, bad_got)
        assert torch.equal(y[~bad_got], want[~bad_want])


@pytest.fixture(scope="module")
def resnet():
    """ResNet-18 with Kaiming weights and the BatchNorm statistics of synthetic.randomize_norm_stats_."""
    from sgv3d_amd import synthetic
    from sgv3d_amd.layers.blocks import ResNet
    torch.manual_seed(3)
    net = ResNet(depth=18).eval()
    net.init_weights()
    synthetic.randomize_norm_stats_(net, 4, residual_gamma=0.3)
    return net


@pytest.mark.parametrize("variant", VARIANTS)
def test_fused_launch_is_as_close_to_float64_as_torch_cpu_float32(hip, resnet, variant):
    """Against conv2d + BN + ReLU + max_pool2d in float64 on the CPU: the largest error is at most twice that of the same chain in
    torch CPU float32 on the same input (e_hip <= 2 e_cpu)."""
    from sgv3d_amd.layers.blocks import fold_bn
    lib = hip.load()
    x = _image(2, 37, 53, 13)

    def chain(dt):
        with torch.no_grad():
            c, bn = resnet.conv1, resnet.bn1
            y = F.conv2d(x.to(dt), c.weight.to(dt), None, 2, 3)
            y = F.batch_norm(y, bn.running_mean.to(dt), bn.running_var.to(dt), bn.weight.to(dt), bn.bias.to(dt), False, 0.0, bn.eps)
            return F.max_pool2d(torch.relu(y), 3, 2, 1).permute(0, 2, 3, 1)
    want = chain(torch.float64)
    e_cpu = float((chain(torch.float32).double() - want).abs().max())
    scale, shift = fold_bn(resnet.bn1, None)
    u = _pack(lib, resnet.conv1.weight.detach())
    _, y = fused(lib, x.to(DEV), u, scale.float().to(DEV).contiguous(), shift.float().to(DEV).contiguous(), variant)
    e_hip = float((y.cpu().double() - want).abs().max())
    print(f"stem 2x3x37x53: fused x3 {e_hip:.3e}, torch CPU float32 {e_cpu:.3e}")
    assert e_hip <= 2.0 * e_cpu, (e_hip, e_cpu)


def test_refused_cases_return_the_error_and_launch_nothing(stem):
    lib, u = stem["lib"], stem["u"]
    x = _image(1, 9, 10, 14).to(DEV)
    y = torch.full((1, 3, 3, 64), POISON, device=DEV)
    sc, sh = stem["scale_d"].data_ptr(), stem["shift_d"].data_ptr()
    good = dict(batch=1, h=9, w=10, x=x.data_ptr(), u=u.data_ptr(), nb=PACK_BYTES, sc=sc, sh=sh, y=y.data_ptr(), y_ld=64, variant=0)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.sgv3d_stem_pool_x3_forward(a["batch"], a["h"], a["w"], a["x"], a["u"], a["nb"], a["sc"], a["sh"], a["y"], a["y_ld"],
                                            a["variant"], None)
        return rc, lib.sgv3d_last_error()
    for kw, text in ((dict(x=None), b"null pointer"), (dict(u=None), b"null pointer"), (dict(y=None), b"null pointer"),
                     (dict(y_ld=60), b"y_ld"), (dict(y_ld=66), b"y_ld"), (dict(batch=0), b"bad shape"), (dict(h=0), b"bad shape"),
                     (dict(w=-3), b"bad shape"), (dict(variant=1), b"unknown variant"), (dict(variant=-1), b"unknown variant"),
                     (dict(nb=PACK_BYTES - 1024), b"weight pack"), (dict(sh=None), b"scale and shift"),
                     (dict(y=y.data_ptr() + 4), b"aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    assert call()[0] == 0                                        # ... and the same arguments, unharmed, run
    torch.cuda.synchronize()
    assert not bool((y == POISON).any())


def test_resnet_through_both_routes(resnet, monkeypatch):
    """``ResNet.hip_forward_image`` under the fixed rule takes the fused launch; with hip_ops.STEM_FUSED off it runs the three
    launches.  With the stem convolution pinned to an f32x3 tile without split-K every stage output is equal bit for bit."""
    from sgv3d_amd import hip_ops
    net = copy.deepcopy(resnet).to(DEV)
    x = _image(2, 37, 53, 15).to(DEV)
    for k, v in dict(AUTOTUNE=False, MFMA_BF16=False, MFMA_F32X3=False, PW_X3=True, STEM_FUSED=True, SPLIT_K=False).items():
        monkeypatch.setattr(hip_ops, k, v)
    launches = []
    real = hip_ops.stem_fused
    monkeypatch.setattr(hip_ops, "stem_fused", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    monkeypatch.setattr(net.hip_state(x.device)["stem"], "tile", 65)     # 64 pixels x 64 channels of conv_pw_x3_kernel
    with torch.no_grad():
        on = net.hip_forward_image(x, split_tag="stage1")
        torch.cuda.synchronize()
        assert len(launches) == 1
        monkeypatch.setattr(hip_ops, "STEM_FUSED", False)
        off = net.hip_forward_image(x, split_tag="stage1")
        plain = net.hip_forward(hip_ops.nchw_to_nhwc(x, c_pad=4))
        torch.cuda.synchronize()
    assert len(launches) == 1 and len(on) == len(off) == len(plain) == 4
    for a, b, c in zip(on, off, plain):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_a_captured_graph_replays_the_fused_launch(stem):
    from sgv3d_amd import hip_ops
    conv = hip_ops.PackedConv(stem["w"], stride=2, pad=3, scale=stem["scale"], shift=stem["shift"], relu=True, cin_pad=4, device=DEV)
    x = _image(2, 37, 53, 16).to(DEV)
    eager = hip_ops.stem_fused(conv, x)
    assert torch.equal(eager, unfused(stem["lib"], x, stem["u"], stem["scale_d"], stem["shift_d"]))
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip_ops.stem_fused(conv, x, out=out)
    side.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # one kernel node: a linear graph
        hip_ops.stem_fused(conv, x, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(_image(2, 37, 53, 17))                               # ... and reads the image of the moment
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, unfused(stem["lib"], x, stem["u"], stem["scale_d"], stem["shift_d"]))
