"""GPU: a bottleneck's conv3 and its stage's shortcut projection in ONE launch of the f32x3 implicit-GEMM kernel
(csrc/conv_pw_x3.hip MODE 3, sgv3d_conv2d_x3_shortcut_forward, hip_ops.conv_shortcut_x3).

The fused launch keeps the k-step order of either source and the two epilogue expressions of the separate launches, so the bar is
bit equality with sgv3d_conv2d_x3_forward called twice with split_k = 1 (the shortcut, then conv3 with that map as its residual)."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = (0, 1, 2, 4, 5, 6, 8, 9, 10)        # desc.tile & 15: m-tile {32, 64, 128} pixels x {128, 64, 256} channels
TILE_X3 = 64
# (stride, input map of the shortcut): stride 1 at 5x7 and 9x16; stride 2 from an odd and an even input, both giving 5x7
GEOMETRIES = ((1, 5, 7), (1, 9, 16), (2, 9, 13), (2, 10, 14))
up32 = lambda v: (v + 31) // 32 * 32


def _desc(B, h, w, cin, oh, ow, cout, stride, x_ld, x_coff, y_ld, y_coff, res_ld, relu, tile):
    from sgv3d_amd._lib import ConvDesc, CONV_NORMAL
    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin, d.out_h, d.out_w, d.cout = B, h, w, cin, oh, ow, cout
    d.kh, d.kw, d.stride, d.pad, d.dil = 1, 1, stride, 0, 1
    d.x_ld, d.x_coff, d.y_ld, d.y_coff, d.res_ld, d.relu = x_ld, x_coff, y_ld, y_coff, res_ld, relu
    d.mode, d.split_k, d.tile, d.k_pad, d.cout_pad, d.k_order = CONV_NORMAL, 1, tile, cin, up32(cout), 1
    return d


def _pack(lib, w):
    """w [cout, cin] f32 on the device -> the fragment-ordered x3 pack."""
    cout, cin = (int(v) for v in w.shape)
    u = torch.empty(up32(cout) // 16, cin // 32, 3, 512, dtype=torch.bfloat16, device=DEV)
    assert lib.sgv3d_conv_pack_weight_x3(w.data_ptr(), cout, cin, 1, 1, cin, up32(cout), u.data_ptr(), None) == 0
    return u


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Case:
    """One (K_a, K_b, cout, geometry, batch): random operands on the device, both sources read through a channel window
    (x_ld > cin, x_coff != 0), the output written into a window of a wider buffer."""

    def __init__(self, lib, ka, kb, cout, geom, B, seed, integer=False):
        stride, H, W = geom
        self.oh, self.ow = (H - 1) // stride + 1, (W - 1) // stride + 1
        self.ka, self.kb, self.cout, self.stride, self.H, self.W, self.B = ka, kb, cout, stride, H, W, B
        g = torch.Generator().manual_seed(seed)
        self.a_ld, self.a_off, self.b_ld, self.b_off, self.y_ld, self.y_off = ka + 12, 8, kb + 8, 4, cout + 20, 12
        if integer:
            rnd = lambda *s: torch.randint(-8, 9, s, generator=g).float()
            self.wa, self.wb = rnd(cout, ka), rnd(cout, kb)
            self.sa, self.sb = torch.randint(1, 4, (cout,), generator=g).float(), torch.randint(1, 4, (cout,), generator=g).float()
        else:
            rnd = lambda *s: torch.randn(*s, generator=g)
            self.wa, self.wb = rnd(cout, ka) / ka ** 0.5, rnd(cout, kb) / kb ** 0.5
            self.sa, self.sb = torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) + 0.5
        self.mid, self.x = rnd(B, self.oh, self.ow, self.a_ld), rnd(B, H, W, self.b_ld)
        self.ha, self.hb = rnd(cout), rnd(cout)
        for k in ("wa", "wb", "sa", "sb", "ha", "hb", "mid", "x"):
            setattr(self, k + "_d", getattr(self, k).to(DEV))
        self.ua, self.ub = _pack(lib, self.wa_d), _pack(lib, self.wb_d)

    def descs(self, variant, relu):
        tile = TILE_X3 | variant
        da = _desc(self.B, self.oh, self.ow, self.ka, self.oh, self.ow, self.cout, 1, self.a_ld, self.a_off, self.y_ld, self.y_off,
                   self.cout, relu, tile)
        db = _desc(self.B, self.H, self.W, self.kb, self.oh, self.ow, self.cout, self.stride, self.b_ld, self.b_off, self.cout, 0, 0, 0,
                   tile)
        return da, db

    def two_launches(self, lib, variant, relu, affine):
        """The shortcut (no ReLU) into a map of its own, then conv3 with that map as the residual: sgv3d_conv2d_x3_forward twice."""
        da, db = self.descs(variant, relu)
        sa, ha, sb, hb = (self.sa_d, self.ha_d, self.sb_d, self.hb_d) if affine else (None,) * 4
        short = torch.empty(self.B, self.oh, self.ow, self.cout, device=DEV)
        y = torch.full((self.B, self.oh, self.ow, self.y_ld), -7.0, device=DEV)
        assert lib.sgv3d_conv2d_x3_forward(ctypes.byref(db), self.x_d.data_ptr(), self.ub.data_ptr(), _ptr(sb), _ptr(hb), None,
                                           short.data_ptr(), None, 0, None) == 0, lib.sgv3d_last_error()
        assert lib.sgv3d_conv2d_x3_forward(ctypes.byref(da), self.mid_d.data_ptr(), self.ua.data_ptr(), _ptr(sa), _ptr(ha),
                                           short.data_ptr(), y.data_ptr(), None, 0, None) == 0, lib.sgv3d_last_error()
        return y

    def fused(self, lib, variant, relu, affine):
        da, db = self.descs(variant, relu)
        sa, ha, sb, hb = (self.sa_d, self.ha_d, self.sb_d, self.hb_d) if affine else (None,) * 4
        y = torch.full((self.B, self.oh, self.ow, self.y_ld), -7.0, device=DEV)
        assert lib.sgv3d_conv2d_x3_shortcut_forward(ctypes.byref(da), self.mid_d.data_ptr(), self.ua.data_ptr(), _ptr(sa), _ptr(ha),
                                                    ctypes.byref(db), self.x_d.data_ptr(), self.ub.data_ptr(), _ptr(sb), _ptr(hb),
                                                    y.data_ptr(), None) == 0, lib.sgv3d_last_error()
        return y

    def float64(self, relu, affine):
        """[B, oh, ow, cout] in float64 from the host copies."""
        a = self.mid[..., self.a_off:self.a_off + self.ka].double() @ self.wa.double().t()
        xs = self.x[:, ::self.stride, ::self.stride, self.b_off:self.b_off + self.kb].double()
        b = xs @ self.wb.double().t()
        if affine:
            a, b = a * self.sa.double() + self.ha.double(), b * self.sb.double() + self.hb.double()
        return torch.relu(a + b) if relu else a + b


_CASES = {}


def _case(lib, ka, kb, cout, geom, B):
    key = (ka, kb, cout, geom, B)
    if key not in _CASES:
        _CASES[key] = _Case(lib, ka, kb, cout, geom, B, seed=hash(key) % 10007)
    return _CASES[key]


SWEEP = list(itertools.product((32, 64), (32, 96), (36, 128, 260), GEOMETRIES, (1, 2)))


@pytest.mark.parametrize("variant", VARIANTS)
def test_two_source_launch_is_bit_equal_to_the_two_launches(hip, variant):
    """Every tile variant x K_a {32, 64} x K_b {32, 96} x cout {36: one ragged column tile, 128: exactly one, 260: several, the last
    ragged} x stride 1 (5x7, 9x16) / stride 2 (9x13 and 10x14 -> 5x7) x batch {1, 2} x ReLU x (scale, shift) null / given; M = 35
    rows is less than any m-tile, 288 (batch 2 of 9x16) leaves a ragged last tile at 128.  The whole output buffer is compared, the
    untouched channels beside the window included."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    for ka, kb, cout, geom, B in SWEEP:
        c = _case(lib, ka, kb, cout, geom, B)
        for relu, affine in itertools.product((1, 0), (True, False)):
            want = c.two_launches(lib, variant, relu, affine)
            got = c.fused(lib, variant, relu, affine)
            assert torch.equal(got, want), (variant, ka, kb, cout, geom, B, relu, affine,
                                            float((got - want).abs().max()))
    assert float(got[..., :c.y_off].max()) == -7.0 and float(got[..., c.y_off + c.cout:].min()) == -7.0


@pytest.mark.parametrize("geom", [(1, 9, 16), (2, 10, 14)])
@pytest.mark.parametrize("cout", [36, 128, 260])
def test_two_source_launch_is_as_close_to_float64_as_the_f32_kernel(hip, geom, cout):
    """Against a float64 convolution: at most twice the error of the f32-MFMA implicit GEMM on the same data (two PackedConv launches
    with tile 4), the bar tests/test_conv_gpu.py applies to the x3 kernels (and < 3e-6 of the output scale)."""
    from sgv3d_amd import _lib
    from sgv3d_amd.hip_ops import PackedConv
    lib = _lib.load()
    for ka, kb in itertools.product((32, 64), (32, 96)):
        c = _case(lib, ka, kb, cout, geom, 2)
        want = c.float64(1, True)
        s = float(want.abs().max())
        got = c.fused(lib, 1, 1, True)[..., c.y_off:c.y_off + cout]
        ds = PackedConv(c.wb_d.reshape(cout, kb, 1, 1), stride=c.stride, scale=c.sb_d, shift=c.hb_d)
        c3 = PackedConv(c.wa_d.reshape(cout, ka, 1, 1), scale=c.sa_d, shift=c.ha_d, relu=True)
        native = c3(c.mid_d, x_coff=c.a_off, residual=ds(c.x_d, x_coff=c.b_off, tile=4, split_k=1), tile=4, split_k=1)
        err = float((got.cpu().double() - want).abs().max()) / s
        e_native = float((native.cpu().double() - want).abs().max()) / s
        print(f"K {ka}+{kb} cout {cout} stride {c.stride}: x3 two-source {err:.3e}, f32 MFMA {e_native:.3e}")
        assert err <= max(2.0 * e_native, 3e-7) and err < 3e-6, (ka, kb, err, e_native)


@pytest.mark.parametrize("variant", [0, 6, 9])
def test_two_source_launch_is_exact_on_small_integers(hip, variant):
    """Integer operands (every product and sum below 2^24): the result is the float64 one exactly -- a dropped partial product, a
    swapped plane or a row gathered from the wrong pixel shows up as a whole number."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    for i, (ka, kb, cout, geom, B) in enumerate(SWEEP[variant % 3::3]):
        c = _Case(lib, ka, kb, cout, geom, B, seed=i, integer=True)
        for relu, affine in ((1, True), (0, False)):
            got = c.fused(lib, variant, relu, affine)[..., c.y_off:c.y_off + cout]
            assert torch.equal(got.cpu().double(), c.float64(relu, affine)), (variant, ka, kb, cout, geom, B, relu, affine)


# ------------------------------------------------------------------------------------------------ block level
def _randomize(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (m.in_channels * m.kernel_size[0] ** 2) ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
    return mod.eval()


def _stage(inplanes, planes, stride, blocks):
    from sgv3d_amd.layers.blocks import Bottleneck
    down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(planes * 4))
    return torch.nn.Sequential(Bottleneck(inplanes, planes, stride, down), *[Bottleneck(planes * 4, planes) for _ in range(blocks - 1)])


def _float64_stage(stage, x):
    for blk in stage:
        o = F.relu(blk.bn1(blk.conv1(x)))
        o = F.relu(blk.bn2(blk.conv2(o)))
        o = blk.bn3(blk.conv3(o))
        x = F.relu(o + (blk.downsample(x) if blk.downsample is not None else x))
    return x


@pytest.mark.parametrize("planes,stride,blocks", [(32, 1, 1), (32, 2, 1), (32, 2, 2), (64, 1, 2)])
def test_bottleneck_through_the_fused_launch_is_bit_equal_to_the_unfused_path(hip, monkeypatch, planes, stride, blocks):
    """``Bottleneck`` alone and a two-block stage at 8x12: the fixed rule (autotune off) takes the two-source launch; with it switched
    off (hip_ops.SHORTCUT_X3) the same blocks run ds and conv3 as two launches of the x3 kernel (tile 60, split-K 1).  Same bits.
    (planes 32: the per-layer dispatch offers the x3 kernel from 64 input channels on, the kernel itself covers 32 -- the unfused
    reference lifts that threshold of PackedConv.pw_x3_ok for itself.)"""
    from sgv3d_amd import hip_ops
    from sgv3d_amd.hip_ops import PackedConv
    stage = _randomize(_stage(64, planes, stride, blocks), 100 + planes + stride).to(DEV)
    x = torch.randn(2, 8, 12, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    monkeypatch.setattr(hip_ops, "AUTOTUNE", False)
    launches = []
    real = hip_ops.conv_shortcut_x3
    monkeypatch.setattr(hip_ops, "conv_shortcut_x3", lambda *a, **k: (launches.append(1), real(*a, **k))[1])

    def forward():
        y = x
        for blk in stage:
            y = blk.hip_forward(y)
        torch.cuda.synchronize()
        return y
    fused = forward()
    assert len(launches) == 1                                  # the stage's first block, once
    monkeypatch.setattr(hip_ops, "SHORTCUT_X3", False)
    ok = PackedConv.pw_x3_ok

    def covers(self, d=None, gate=None, io=0):
        return ok(self, d, gate, io) or (self.kh == 1 and self.kw == 1 and self.cin == 32 and not self.transposed and gate is None and io == 0)
    monkeypatch.setattr(PackedConv, "pw_x3_ok", covers)
    first = stage[0].hip_state(x.device)
    first['c3'].tile = first['ds'].tile = 60
    plain = forward()
    assert len(launches) == 1
    assert torch.equal(fused, plain), float((fused - plain).abs().max())
    # ... and both are the block: against the float64 module
    with torch.no_grad():
        want = _float64_stage(stage.double().cpu(), x.cpu().double().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert float((fused.cpu().double() - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max()))
