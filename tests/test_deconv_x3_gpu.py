"""GPU: kernel == stride transposed convolutions (SECONDFPN's upsampling levels) on the f32x3 pointwise kernel
(csrc/conv_pw_x3.hip MODE 4, sgv3d_conv2d_x3_forward with mode SGV3D_CONV_DECONV, hip_ops.deconv_x3).

The DECONV launch runs the MODE 0 k-loop over ks * ks * cout columns (column = tap * cout + co) and scatters in the epilogue, so the bar
is bit equality with the NORMAL launch of the same pack (scale and shift tiled ks * ks times) followed by torch's pixel shuffle."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = (0, 1, 2, 4, 5, 6, 8, 9, 10)        # desc.tile & 15: m-tile {32, 64, 128} pixels x {128, 64, 256} channels
TILE_X3 = 64
GUARD = 256                                    # floats of poison before and after the output buffer
POISON = -7.0
up32 = lambda v: (v + 31) // 32 * 32


def _desc(B, h, w, cin, cout, ks, y_ld, y_coff, relu, tile, split_k, deconv):
    from sgv3d_amd._lib import ConvDesc, CONV_DECONV, CONV_NORMAL
    d = ConvDesc()
    n = ks * ks * cout
    d.batch, d.in_h, d.in_w, d.cin = B, h, w, cin
    d.kh, d.kw, d.stride, d.pad, d.dil = 1, 1, 1, 0, 1
    d.x_ld, d.x_coff, d.res_ld, d.relu = cin, 0, 0, relu
    d.split_k, d.tile, d.k_pad, d.cout_pad, d.k_order = split_k, tile, cin, up32(n), 1
    if deconv:
        d.mode, d.deconv_ks, d.out_h, d.out_w, d.cout, d.y_ld, d.y_coff = CONV_DECONV, ks, h * ks, w * ks, cout, y_ld, y_coff
    else:
        d.mode, d.deconv_ks, d.out_h, d.out_w, d.cout, d.y_ld, d.y_coff = CONV_NORMAL, 0, h, w, n, n, 0
    return d


def _ptr(t):
    return None if t is None else t.data_ptr()


def _shuffle(t, ks):
    """[B, H, W, ks * ks * cout] with column = (dy * ks + dx) * cout + co -> [B, H ks, W ks, cout], through torch's pixel shuffle
    (NCHW, channel = (co * ks + dy) * ks + dx)."""
    B, H, W, n = t.shape
    cout = n // (ks * ks)
    nchw = t.view(B, H, W, ks * ks, cout).permute(0, 4, 3, 1, 2).reshape(B, cout * ks * ks, H, W)
    return F.pixel_shuffle(nchw, ks).permute(0, 2, 3, 1).contiguous()


class _Case:
    """One (cin, cout, ks, map, batch): the transposed convolution's weight [cin, cout, ks, ks], its x3 pack of the
    [ks * ks * cout][cin] view (row = tap * cout + co), the input, scale and shift; host copies for the references."""

    def __init__(self, lib, cin, cout, ks, hw, B, seed, integer=False):
        self.cin, self.cout, self.ks, (self.H, self.W), self.B = cin, cout, ks, hw, B
        g = torch.Generator().manual_seed(seed)
        if integer:
            rnd = lambda *s: torch.randint(-8, 9, s, generator=g).float()
            self.w, self.scale = rnd(cin, cout, ks, ks), torch.randint(1, 4, (cout,), generator=g).float()
        else:
            rnd = lambda *s: torch.randn(*s, generator=g)
            self.w, self.scale = rnd(cin, cout, ks, ks) / cin ** 0.5, torch.rand(cout, generator=g) + 0.5
            self.scale[::3] *= -1.0                                      # (negative BN scales too)
        self.x, self.shift = rnd(B, self.H, self.W, cin), rnd(cout)
        self.n = ks * ks * cout
        self.y_ld, self.y_off = cout + 20, 12
        rows = self.w.permute(2, 3, 1, 0).reshape(self.n, cin).contiguous()
        self.rows_d, self.x_d, self.scale_d, self.shift_d = (t.to(DEV) for t in (rows, self.x, self.scale, self.shift))
        self.scale_t, self.shift_t = self.scale_d.repeat(ks * ks).contiguous(), self.shift_d.repeat(ks * ks).contiguous()
        self.u = torch.empty(up32(self.n) // 16, cin // 32, 3, 512, dtype=torch.bfloat16, device=DEV)
        assert lib.sgv3d_conv_pack_weight_x3(self.rows_d.data_ptr(), self.n, cin, 1, 1, cin, up32(self.n), self.u.data_ptr(), None) == 0

    def _ws(self, split_k):
        if split_k <= 1:
            return None, 0
        ws = torch.empty(split_k * self.B * self.H * self.W * self.n, device=DEV)
        return ws, ws.numel() * 4

    def normal(self, lib, variant, relu, affine, split_k):
        """The NORMAL launch of the same pack: [B, H, W, ks * ks * cout]."""
        d = _desc(self.B, self.H, self.W, self.cin, self.cout, self.ks, 0, 0, relu, TILE_X3 | variant, split_k, False)
        y = torch.empty(self.B, self.H, self.W, self.n, device=DEV)
        sc, sh = (self.scale_t, self.shift_t) if affine else (None, None)
        ws, nws = self._ws(split_k)
        assert lib.sgv3d_conv2d_x3_forward(ctypes.byref(d), self.x_d.data_ptr(), self.u.data_ptr(), _ptr(sc), _ptr(sh), None,
                                           y.data_ptr(), _ptr(ws), nws, None) == 0, lib.sgv3d_last_error()
        return y

    def deconv(self, lib, variant, relu, affine, split_k):
        """The DECONV launch into a channel window of a wider map with poisoned guard bands around it: (whole buffer, map view)."""
        d = _desc(self.B, self.H, self.W, self.cin, self.cout, self.ks, self.y_ld, self.y_off, relu, TILE_X3 | variant, split_k, True)
        numel = self.B * self.H * self.ks * self.W * self.ks * self.y_ld
        buf = torch.full((GUARD + numel + GUARD,), POISON, device=DEV)
        y = buf[GUARD:GUARD + numel].view(self.B, self.H * self.ks, self.W * self.ks, self.y_ld)
        sc, sh = (self.scale_d, self.shift_d) if affine else (None, None)
        ws, nws = self._ws(split_k)
        assert lib.sgv3d_conv2d_x3_forward(ctypes.byref(d), self.x_d.data_ptr(), self.u.data_ptr(), _ptr(sc), _ptr(sh), None,
                                           y.data_ptr(), _ptr(ws), nws, None) == 0, lib.sgv3d_last_error()
        return buf, y

    def reference(self, dtype, relu, affine):
        """conv_transpose2d (+ scale, shift, ReLU) on the host in ``dtype``: [B, H ks, W ks, cout]."""
        y = F.conv_transpose2d(self.x.to(dtype).permute(0, 3, 1, 2), self.w.to(dtype), stride=self.ks).permute(0, 2, 3, 1)
        if affine:
            y = y * self.scale.to(dtype) + self.shift.to(dtype)
        return torch.relu(y) if relu else y


_CASES = {}


def _case(lib, *key):
    if key not in _CASES:
        _CASES[key] = _Case(lib, *key, seed=hash(key) % 10007)
    return _CASES[key]


SWEEP = list(itertools.product((32, 96), (4, 36, 64), (1, 2, 4, 8), ((5, 7), (9, 16)), (1, 2)))


@pytest.mark.parametrize("variant", VARIANTS)
def test_deconv_launch_is_bit_equal_to_the_normal_launch_and_a_pixel_shuffle(hip, variant):
    """Every tile variant x cin {32, 96} x cout {4, 36: a tap boundary inside a wave's 32 columns and a ragged last tile, 64} x ks
    {1, 2, 4, 8} x maps 5x7 / 9x16 (M not a multiple of 16) x batch {1, 2} x ReLU x (scale, shift) null / given x split-K {1, 3}
    (3 needs three k-steps: cin 96; at cin 32 the entry refuses it), written at a channel offset into a wider map.  The channels
    beside the window and the guard bands around the buffer come back untouched."""
    lib = hip.load()
    for cin, cout, ks, hw, B in SWEEP:
        c = _case(lib, cin, cout, ks, hw, B)
        for relu, affine, split_k in itertools.product((1, 0), (True, False), (1, 3)):
            if split_k > cin // 32:
                d = _desc(B, hw[0], hw[1], cin, cout, ks, c.y_ld, c.y_off, relu, TILE_X3 | variant, split_k, True)
                assert lib.sgv3d_conv2d_x3_forward(ctypes.byref(d), c.x_d.data_ptr(), c.u.data_ptr(), None, None, None, c.x_d.data_ptr(),
                                                   c.x_d.data_ptr(), 1 << 30, None) == -1 and b"split_k" in lib.sgv3d_last_error()
                continue
            want = _shuffle(c.normal(lib, variant, relu, affine, split_k), ks)
            buf, y = c.deconv(lib, variant, relu, affine, split_k)
            got = y[..., c.y_off:c.y_off + cout]
            assert torch.equal(got, want), (variant, cin, cout, ks, hw, B, relu, affine, split_k, float((got - want).abs().max()))
            assert float(y[..., :c.y_off].max()) == POISON == float(y[..., :c.y_off].min())
            assert float(y[..., c.y_off + cout:].max()) == POISON == float(y[..., c.y_off + cout:].min())
            assert bool((buf[:GUARD] == POISON).all()) and bool((buf[-GUARD:] == POISON).all())


@pytest.mark.parametrize("ks", [1, 2, 4, 8])
@pytest.mark.parametrize("cout", [36, 64])
def test_deconv_launch_is_as_close_to_float64_as_torch_cpu_float32(hip, ks, cout):
    """Against float64 ``conv_transpose2d`` (+ scale, shift, ReLU): the largest error is at most twice that of torch's CPU float32
    on the same data (e_hip <= 2 e_cpu), split-K 1 and 3."""
    lib = hip.load()
    for cin, hw in itertools.product((32, 96), ((5, 7), (9, 16))):
        c = _case(lib, cin, cout, ks, hw, 2)
        want = c.reference(torch.float64, 1, True)
        e_cpu = float((c.reference(torch.float32, 1, True).double() - want).abs().max())
        for split_k in (1, 3) if cin >= 96 else (1,):
            _, y = c.deconv(lib, 1, 1, True, split_k)
            e_hip = float((y[..., c.y_off:c.y_off + cout].cpu().double() - want).abs().max())
            print(f"cin {cin} cout {cout} ks {ks} map {hw} split-K {split_k}: x3 deconv {e_hip:.3e}, torch CPU float32 {e_cpu:.3e}")
            assert e_hip <= 2.0 * e_cpu, (cin, hw, split_k, e_hip, e_cpu)


@pytest.mark.parametrize("variant", [0, 6, 9])
def test_deconv_launch_is_exact_on_small_integers(hip, variant):
    """Integer operands (every product and sum below 2^24): the result is the float64 one exactly -- a dropped partial product, a
    swapped plane or a value scattered to the wrong pixel shows up as a whole number."""
    lib = hip.load()
    for i, (cin, cout, ks, hw, B) in enumerate(SWEEP[variant % 3::3]):
        c = _Case(lib, cin, cout, ks, hw, B, seed=i, integer=True)
        for relu, affine, split_k in ((1, True, 1), (0, False, 1)) + (((1, True, 3),) if cin >= 96 else ()):
            _, y = c.deconv(lib, variant, relu, affine, split_k)
            got = y[..., c.y_off:c.y_off + cout].cpu().double()
            assert torch.equal(got, c.reference(torch.float64, relu, affine)), (variant, cin, cout, ks, hw, B, relu, affine, split_k)


def test_refused_cases_return_the_error_and_launch_nothing(hip):
    """A residual, cout % 4, cin % 32, an output that is not input * ks: -1 with the reason, and the poisoned output is untouched."""
    lib = hip.load()
    c = _case(lib, 32, 36, 2, (5, 7), 1)
    y = torch.full((1, 10, 14, c.y_ld), POISON, device=DEV)
    good = lambda: _desc(1, 5, 7, 32, 36, 2, c.y_ld, c.y_off, 1, TILE_X3 | 1, 1, True)

    def call(d, residual=None):
        rc = lib.sgv3d_conv2d_x3_forward(ctypes.byref(d), c.x_d.data_ptr(), c.u.data_ptr(), c.scale_d.data_ptr(), c.shift_d.data_ptr(),
                                         _ptr(residual), y.data_ptr(), None, 0, None)
        return rc, lib.sgv3d_last_error()
    rc, msg = call(good(), residual=y)
    assert rc == -1 and b"no residual" in msg
    d = good()
    d.cout = 38
    rc, msg = call(d)
    assert rc == -1 and b"cout % 4" in msg
    d = good()
    d.cin = d.x_ld = 48
    rc, msg = call(d)
    assert rc == -1 and b"cin % 32" in msg
    for oh, ow in ((10, 15), (11, 14), (5, 7)):
        d = good()
        d.out_h, d.out_w = oh, ow
        rc, msg = call(d)
        assert rc == -1 and b"input * deconv_ks" in msg
    d = good()
    d.deconv_ks = 0
    assert call(d)[0] == -1
    d = good()
    d.kh = d.kw = 3
    assert call(d)[0] == -1
    torch.cuda.synchronize()
    assert bool((y == POISON).all())
    assert call(good())[0] == 0                                  # ... and the same descriptor, unharmed, runs
    torch.cuda.synchronize()
    assert not bool((y[..., c.y_off:c.y_off + 36] == POISON).any())


# ------------------------------------------------------------------------------------------------ SECONDFPN
def _neck(seed):
    from sgv3d_amd.layers.blocks import SECONDFPN
    neck = SECONDFPN(in_channels=(32, 64, 96), out_channels=(32, 36, 64), upsample_strides=(1, 2, 4))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, (torch.nn.ConvTranspose2d, torch.nn.Conv2d)):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[0] ** 0.5)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
    return neck.eval()


def test_secondfpn_through_the_x3_deconv_and_with_it_switched_off(hip, monkeypatch):
    """SECONDFPN (levels 32 -> 32 at stride 1, 64 -> 36 at stride 2, 96 -> 64 at stride 4; 12x20 output, batch 2) under the fixed
    rule: the two transposed levels take ``hip_ops.deconv_x3``; with hip_ops.DECONV_X3 off nothing does.  The stride-1 level (a plain
    1x1 layer either way) is equal bit for bit; on the transposed levels both paths meet the float64 rule (e <= 2 e_cpu)."""
    from sgv3d_amd import hip_ops
    neck = _neck(5)
    g = torch.Generator().manual_seed(6)
    feats = [torch.randn(2, 12 // s, 20 // s, c, generator=g) for s, c in ((1, 32), (2, 64), (4, 96))]
    with torch.no_grad():
        run = lambda dt: torch.cat([blk(f.to(dt).permute(0, 3, 1, 2)) for blk, f in zip(neck.to(dt).deblocks, feats)], 1).permute(0, 2, 3, 1)
        want = run(torch.float64)
        cpu32 = run(torch.float32)
    neck = neck.float().to(DEV)
    dfeats = [f.to(DEV) for f in feats]
    monkeypatch.setattr(hip_ops, "AUTOTUNE", False)
    for k, v in dict(MFMA_BF16=False, MFMA_F32X3=False, PW_X3=True, DECONV_X3=True).items():
        monkeypatch.setattr(hip_ops, k, v)
    launches = []
    real = hip_ops.deconv_x3
    monkeypatch.setattr(hip_ops, "deconv_x3", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    with torch.no_grad():
        on = neck.hip_forward(dfeats)
        torch.cuda.synchronize()
        assert len(launches) == 2
        monkeypatch.setattr(hip_ops, "DECONV_X3", False)
        off = neck.hip_forward(dfeats)
        torch.cuda.synchronize()
    assert len(launches) == 2
    assert tuple(on.shape) == (2, 12, 20, 132)
    assert torch.equal(on[..., :32], off[..., :32])
    for lo, hi in ((32, 68), (68, 132)):
        e_cpu = float((cpu32[..., lo:hi].double() - want[..., lo:hi]).abs().max())
        e_on = float((on[..., lo:hi].cpu().double() - want[..., lo:hi]).abs().max())
        e_off = float((off[..., lo:hi].cpu().double() - want[..., lo:hi]).abs().max())
        print(f"channels [{lo}, {hi}): x3 deconv {e_on:.3e}, f32 MFMA {e_off:.3e}, torch CPU float32 {e_cpu:.3e}")
        assert e_on <= 2.0 * e_cpu, (lo, e_on, e_off, e_cpu)
