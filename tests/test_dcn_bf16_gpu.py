"""One-launch deformable 3x3 convolution on the bf16 matrix cores (csrc/dcn_fused_bf16.hip, hip_ops.deform_conv3x3_bf16) on the
MI355X: the bf16-mode twin of sgv3d_deform_conv3x3_forward.

Yardsticks.  (1) Data on which every f32 summation order gives the same bits (small integers, offsets that are multiples of
1/4): the launch, the im2col + GEMM form in bf16 mode and the float64 DCNv1 must be EQUAL.  (2) Random data: the float64 product
of the ROUNDED operands -- the column tensor hip_ops.deform_im2col3x3 itself writes (bf16 x), or its result rounded to bf16
(f32 x), and the weights rounded to bf16 -- which leaves the summation order only: 2e-5 of the output scale, the bar
tests/test_conv_bf16_gpu.py holds every bf16 convolution to; the im2col + GEMM form is held to the same bar beside it.  Against
the unrounded float64 DCNv1: 2e-2 of the output scale (operand rounding).  (3) The bf16 output is the f32 one rounded once."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from sgv3d_amd import hip_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, C, H, W, groups, cout): the shapes of tests/test_conv_gpu.py::test_deform_conv_fused; all satisfy cpg % 32 == 0, opg % 4 == 0
SMALL = [(2, 128, 9, 11, 4, 128), (1, 256, 13, 7, 2, 96), (3, 64, 5, 5, 2, 264)]
FULL = (1, 512, 54, 96, 4, 512)


@pytest.fixture
def bf16_mode():
    old = hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.DCN_FUSED, hip_ops.DCN_FUSED_BF16
    hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.DCN_FUSED, hip_ops.DCN_FUSED_BF16 = True, False, True, True
    yield
    hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.DCN_FUSED, hip_ops.DCN_FUSED_BF16 = old


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def group_matrices(weight, groups):
    """[cout, cpg, 3, 3] -> per group [opg, 9 * cpg] with k = tap * cpg + ci (the column tensor's order)."""
    cout, cpg = int(weight.shape[0]), int(weight.shape[1])
    opg = cout // groups
    return [weight[g * opg:(g + 1) * opg].permute(0, 2, 3, 1).reshape(opg, 9 * cpg) for g in range(groups)]


def im2col_form(xd, od, weight, groups, out_dtype=torch.float32):
    """The form the launch replaces: deformable im2col + one 1x1 GEMM per group, in bf16 mode."""
    B, H, W, C = xd.shape
    cout, cpg = int(weight.shape[0]), C // groups
    opg = cout // groups
    col = hip_ops.deform_im2col3x3(xd, od, groups)
    out = torch.empty(B, H, W, cout, dtype=out_dtype, device=xd.device)
    for gi, wg in enumerate(group_matrices(weight, groups)):
        hip_ops.PackedConv(wg.reshape(opg, 9 * cpg, 1, 1).contiguous().to(xd.device))(col, out, x_coff=gi * 9 * cpg, y_coff=gi * opg)
    return out, col


def rounded_operand_reference(col, weight, groups):
    """float64 product of the rounded operands: col [B,H,W,groups*9*cpg] as the im2col kernel wrote it, rounded to bf16 (a no-op
    for a bf16 column tensor), times the weights rounded to bf16.  -> NHWC float64 on the CPU."""
    B, H, W, K = col.shape
    c = col.bfloat16().cpu().double().reshape(B * H * W, groups, K // groups)
    outs = [c[:, g] @ wg.bfloat16().double().t() for g, wg in enumerate(group_matrices(weight.cpu(), groups))]
    return torch.cat(outs, 1).reshape(B, H, W, -1)


def far_offsets(offs, H, W):
    offs[:, :, 0, 0] += 40.0                                     # far outside the image: zeros
    offs[:, :, H - 1, W - 1] -= 40.0
    return offs


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SMALL)
def test_exact_on_integer_data(bf16_mode, shape, x_dtype):
    """x integers in [-4, 4], weights integers in [-3, 3], offsets multiples of 1/4 in [-2.5, 2.5] (+40 / -40 at two corner
    pixels): the bilinear weights are multiples of 1/16, every sample is a multiple of 1/16 of magnitude <= 4 (exact in bf16) and
    any partial sum of <= 1152 products stays below 2^24 / 16, so every f32 summation order gives the same bits: zero tolerance."""
    from oracle import torch_model as TM
    B, C, H, W, groups, cout = shape
    g = torch.Generator().manual_seed(7 + C)
    x = torch.randint(-4, 5, (B, C, H, W), generator=g).float()
    weight = torch.randint(-3, 4, (cout, C // groups, 3, 3), generator=g).float()
    quarter = far_offsets(torch.randint(-10, 11, (B, 18, H, W), generator=g).float() / 4, H, W)
    xd = nhwc(x).to(DEV).to(x_dtype)
    assert hip_ops.deform_conv3x3_bf16_eligible(xd, groups, cout)
    packed = hip_ops.PackedDeformBf16(weight.to(DEV), groups)
    for offs in (torch.zeros(B, 18, H, W), quarter):
        od = nhwc(offs).to(DEV)
        got = hip_ops.deform_conv3x3_bf16(xd, od, packed, out_dtype=torch.float32)
        assert got.dtype == torch.float32
        want = TM.deform_conv3x3(x.double(), offs.double(), weight.double(), groups)
        assert torch.equal(nchw(got.cpu()).double(), want)
        old, col = im2col_form(xd, od, weight, groups)
        assert torch.equal(col.float(), col.bfloat16().float())                       # the column tensor is bf16-exact
        assert torch.equal(old, got)
        got16 = hip_ops.deform_conv3x3_bf16(xd, od, packed, out_dtype=torch.bfloat16)
        assert got16.dtype == torch.bfloat16 and torch.equal(got16, got.bfloat16())
        if offs.abs().sum() == 0:
            assert torch.equal(want, F.conv2d(x.double(), weight.double(), None, 1, 1, 1, groups))


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SMALL + [FULL])
def test_random_data_against_rounded_operands(bf16_mode, shape, x_dtype):
    """Bars 2 and 3 of the module docstring, with the output written at channel offset 8 of a buffer 12 channels wider that is
    pre-filled with 7.0 (neighbours untouched), a repeat that must give the same bits, and pixel counts (198, 91, 75, 5184) of
    which only the last is a multiple of the 64-pixel tile."""
    from oracle import torch_model as TM
    B, C, H, W, groups, cout = shape
    g = torch.Generator().manual_seed(50 + C)
    x = torch.randn(B, C, H, W, generator=g)
    weight = torch.randn(cout, C // groups, 3, 3, generator=g) / (9 * C // groups) ** 0.5
    offs = far_offsets(torch.randn(B, 18, H, W, generator=g) * 2.5, H, W)
    xd = nhwc(x).to(DEV).to(x_dtype)
    od = nhwc(offs).to(DEV)
    packed = hip_ops.PackedDeformBf16(weight.to(DEV), groups)

    out = torch.full((B, H, W, cout + 12), 7.0, device=DEV)
    hip_ops.deform_conv3x3_bf16(xd, od, packed, out=out, y_coff=8)
    assert float(out[..., :8].min()) == 7.0 == float(out[..., :8].max())
    assert float(out[..., cout + 8:].min()) == 7.0 == float(out[..., cout + 8:].max())
    got = out[..., 8:cout + 8].contiguous()
    again = torch.full_like(out, 7.0)
    hip_ops.deform_conv3x3_bf16(xd, od, packed, out=again, y_coff=8)
    assert torch.equal(out, again)                                                       # a fixed summation order

    old, col = im2col_form(xd, od, weight, groups)
    assert col.dtype == x_dtype
    want = rounded_operand_reference(col, weight, groups)
    scale = max(1.0, float(want.abs().max()))
    err_new = float((got.cpu().double() - want).abs().max())
    err_old = float((old.cpu().double() - want).abs().max())
    print(f"\n{shape} x {x_dtype}: |new - want| {err_new:.3e}  |im2col form - want| {err_old:.3e}  bar {2e-5 * scale:.3e}")
    assert err_old <= 2e-5 * scale                                                       # the bar is one the existing path meets
    assert err_new <= 2e-5 * scale
    x_seen = xd.float().cpu().permute(0, 3, 1, 2).double()                              # what the kernel was given
    full = nhwc(TM.deform_conv3x3(x_seen, offs.double(), weight.double(), groups))
    assert float((got.cpu().double() - full).abs().max()) <= 2e-2 * max(1.0, float(full.abs().max()))

    out16 = torch.full((B, H, W, cout + 12), 7.0, device=DEV, dtype=torch.bfloat16)
    hip_ops.deform_conv3x3_bf16(xd, od, packed, out=out16, y_coff=8)
    assert float(out16[..., :8].float().min()) == 7.0 == float(out16[..., :8].float().max())
    assert float(out16[..., cout + 8:].float().min()) == 7.0 == float(out16[..., cout + 8:].float().max())
    got16 = out16[..., 8:cout + 8]
    assert torch.equal(got16, got.bfloat16())                                            # the f32 accumulator rounded once
    assert bool(((got16.cpu().double() - want).abs() <= 2.0 ** -8 * want.abs() + 2e-5 * scale).all())


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_samples_are_the_im2col_kernels_bits(bf16_mode, x_dtype):
    """One-hot weights (one group, 32 channels, output k = tap * 32 + ci picks sample k) make the f32 output the A operand itself:
    it must EQUAL the column tensor the im2col kernel writes (rounded to bf16 for f32 tensors) on random data -- this pins the
    sampling arithmetic of csrc/dcn_fused_bf16.hip to that of the two im2col kernels, contraction included."""
    B, C, H, W = 2, 32, 23, 17
    g = torch.Generator().manual_seed(77)
    xd = nhwc(torch.randn(B, C, H, W, generator=g)).to(DEV).to(x_dtype)
    od = nhwc(far_offsets(torch.randn(B, 18, H, W, generator=g) * 2.5, H, W)).to(DEV)
    weight = torch.zeros(9 * C, C, 3, 3)
    for tap in range(9):
        for ci in range(C):
            weight[tap * C + ci, ci, tap // 3, tap % 3] = 1.0
    got = hip_ops.deform_conv3x3_bf16(xd, od, hip_ops.PackedDeformBf16(weight.to(DEV), 1), out_dtype=torch.float32)
    col = hip_ops.deform_im2col3x3(xd, od, 1)
    assert col.dtype == x_dtype and float(col.float().abs().max()) > 1.0
    assert torch.equal(got, col.bfloat16().float())


def test_capturable_and_ineligible_shapes(bf16_mode):
    B, C, H, W, groups, cout = SMALL[0]
    g = torch.Generator().manual_seed(3)
    xd = nhwc(torch.randn(B, C, H, W, generator=g)).to(DEV).bfloat16()
    od = nhwc(torch.randn(B, 18, H, W, generator=g) * 2.5).to(DEV)
    packed = hip_ops.PackedDeformBf16((torch.randn(cout, C // groups, 3, 3, generator=g) / 17).to(DEV), groups)
    eager = hip_ops.deform_conv3x3_bf16(xd, od, packed)
    assert eager.dtype == torch.bfloat16
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip_ops.deform_conv3x3_bf16(xd, od, packed, out=out)
    side.synchronize()
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                # one kernel node: a linear graph
        hip_ops.deform_conv3x3_bf16(xd, od, packed, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)

    # 16 channels per group: not covered -- the switch says so and the raw entry refuses without a launch
    x16 = torch.zeros(1, 4, 4, 64, device=DEV, dtype=torch.bfloat16)
    assert not hip_ops.deform_conv3x3_bf16_eligible(x16, 4, 64)
    assert hip_ops.deform_conv3x3_bf16_eligible(xd, groups, cout)
    assert not hip_ops.deform_conv3x3_bf16_eligible(xd, groups, cout + 2)             # outputs per group % 4
    hip_ops.DCN_FUSED = False
    assert not hip_ops.deform_conv3x3_bf16_eligible(xd, groups, cout)
    hip_ops.DCN_FUSED = True
    hip_ops.MFMA_BF16 = False
    assert not hip_ops.deform_conv3x3_bf16_eligible(xd, groups, cout)
    hip_ops.MFMA_BF16 = True
    hip_ops.DCN_FUSED_BF16 = False
    assert not hip_ops.deform_conv3x3_bf16_eligible(xd, groups, cout)
    hip_ops.DCN_FUSED_BF16 = True
    from sgv3d_amd import _lib
    lib = _lib.load()
    y = torch.full((1, 4, 4, 64), 7.0, device=DEV)
    o16 = torch.zeros(1, 4, 4, 18, device=DEV)
    rc = lib.sgv3d_deform_conv3x3_forward_bf16(1, 4, 4, 64, 4, 16, x16.data_ptr(), 1, o16.data_ptr(), 18, packed.w.data_ptr(),
                                               y.data_ptr(), 0, 64, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and b"channels per group" in lib.sgv3d_last_error()
    assert float(y.min()) == 7.0 == float(y.max())
    with pytest.raises(_lib.SGV3DError):
        hip_ops.PackedDeformBf16(torch.zeros(64, 16, 3, 3, device=DEV), 4)


@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
def test_dcn_module_takes_the_one_launch_path(bf16_mode, monkeypatch, x_dtype):
    """DCN.hip_forward of a small_conf() model in bf16 mode (bf16 tensors, and f32 tensors with BF16_ACTIVATIONS off): the new
    launch is the one taken, its result meets bar 2 (f32) / bar 3 (bf16) against the rounded-operand yardstick built from the
    offsets the layer itself computed; hip_ops.DCN_FUSED = False brings the im2col form back; a weight change followed by
    hip_invalidate() rebuilds the packed bf16 weights."""
    from sgv3d_amd import synthetic as S
    from sgv3d_amd.layers.backbones.lss_fpn import DCN
    from sgv3d_amd.models.bev_height import BEVHeight
    if x_dtype == torch.float32:
        monkeypatch.setattr(hip_ops, "BF16_ACTIVATIONS", False)
    torch.manual_seed(0)
    bc, hc = S.small_conf()
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 0)
    m = m.to(DEV)
    dcn = [mod for mod in m.modules() if isinstance(mod, DCN)]
    assert len(dcn) == 1
    dcn = dcn[0]
    groups = dcn.groups
    g = torch.Generator().manual_seed(11)
    xd = torch.randn(2, 8, 12, dcn.in_channels, generator=g).to(DEV).to(x_dtype)

    calls = {"im2col": 0, "fused": 0, "offset": None}
    real_im2col, real_fused = hip_ops.deform_im2col3x3, hip_ops.deform_conv3x3_bf16

    def counting_im2col(*a, **k):
        calls["im2col"] += 1
        return real_im2col(*a, **k)

    def counting_fused(x, offset, *a, **k):
        calls["fused"] += 1
        calls["offset"] = offset
        return real_fused(x, offset, *a, **k)

    monkeypatch.setattr(hip_ops, "deform_im2col3x3", counting_im2col)
    monkeypatch.setattr(hip_ops, "deform_conv3x3_bf16", counting_fused)

    def check(y, weight):
        assert y.dtype == x_dtype
        offset = calls["offset"]
        assert float(offset.abs().max()) > 0.1                    # randomize_norm_stats_ gave the offset conv real weights
        want = rounded_operand_reference(real_im2col(xd, offset, groups), weight, groups)
        scale = max(1.0, float(want.abs().max()))
        err = (y.cpu().double() - want).abs()
        if x_dtype == torch.float32:
            assert float(err.max()) <= 2e-5 * scale
        else:
            assert bool((err <= 2.0 ** -8 * want.abs() + 2e-5 * scale).all())
        return want

    with torch.no_grad():
        y = dcn.hip_forward(xd)
        assert calls["fused"] == 1 and calls["im2col"] == 0
        want = check(y, dcn.weight.detach())

        hip_ops.DCN_FUSED = False
        y_old = dcn.hip_forward(xd)
        assert calls["fused"] == 1 and calls["im2col"] == 1
        hip_ops.DCN_FUSED = True
        assert y_old.dtype == x_dtype
        scale = max(1.0, float(want.abs().max()))
        assert bool(((y_old.cpu().double() - want).abs() <= (2.0 ** -8 * want.abs() if x_dtype == torch.bfloat16 else 0) + 2e-5 * scale).all())

        w_old = dcn.weight.detach().clone()
        dcn.weight.mul_(-0.5)
        check(dcn.hip_forward(xd), w_old)                         # the packed state still holds the old weights
        dcn.hip_invalidate()
        y_new = dcn.hip_forward(xd)
        assert calls["fused"] == 3 and calls["im2col"] == 1
        want_new = check(y_new, dcn.weight.detach())
        assert float((want_new + 0.5 * want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))    # bf16(-w / 2) = -bf16(w) / 2
