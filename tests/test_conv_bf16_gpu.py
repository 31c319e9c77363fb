"""bf16-MFMA variant of the implicit-GEMM convolution (the compute dtype BASELINE configs[2] / [4] name) on the MI355X.

The kernel rounds both operands to bf16 (nearest even) and accumulates in float32, so against a float64 convolution of
the SAME bf16-rounded operands only the summation order differs (bar 2e-5); against the unrounded float32 convolution
the difference is the operand rounding (2^-9 per operand, bar 2e-2 of the output scale).  Model level: predictions of
the bf16 forward against the float32 oracle, voxel indices untouched (geometry never goes through MFMA)."""
import pytest
import torch
import torch.nn.functional as F

from sgv3d_amd import hip_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [
    # (B, cin, H, W, cout, k, stride, pad, dil)
    (1, 64, 20, 24, 64, 1, 1, 0, 1),
    (2, 64, 17, 19, 128, 3, 1, 1, 1),      # ragged M
    (1, 128, 16, 16, 256, 3, 2, 1, 1),     # stride 2
    (1, 256, 14, 18, 96, 3, 1, 6, 6),      # dilated, cout not a tile multiple
    (1, 80, 32, 32, 160, 7, 2, 3, 1),      # tap-major K (cin % 32 != 0)
    (1, 4, 40, 56, 64, 7, 2, 3, 1),        # image stem, cin padded 3 -> 4
    (1, 512, 9, 11, 18, 3, 1, 1, 1),       # tiny cout
    (1, 2560, 6, 8, 512, 1, 1, 0, 1),      # long K
]


@pytest.fixture
def bf16_mode():
    old = hip_ops.MFMA_BF16
    hip_ops.MFMA_BF16 = True
    yield
    hip_ops.MFMA_BF16 = old


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tile,split", [(0, 0), (1, 1), (2, 2), (3, 1), (4, 3)])
def test_bf16_conv_matches_rounded_operands(bf16_mode, case, tile, split):
    B, cin, H, W, cout, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g)
    conv = hip_ops.PackedConv(w.to(DEV), stride=stride, pad=pad, dil=dil, scale=scale.to(DEV), shift=shift.to(DEV), relu=True)
    nkt = conv.k_pad // 32
    if split > nkt:
        split = 1
    y = conv(x.permute(0, 2, 3, 1).contiguous().to(DEV), tile=tile or None, split_k=split or None)
    got = y.cpu().double().permute(0, 3, 1, 2)
    rx, rw = x.bfloat16().double(), w.bfloat16().double()
    want = F.relu(F.conv2d(rx, rw, None, stride, pad, dil) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None])
    assert float((got - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))
    full = F.relu(F.conv2d(x.double(), w.double(), None, stride, pad, dil) * scale.double()[None, :, None, None] + shift.double()[None, :, None, None])
    assert float((got - full).abs().max()) <= 2e-2 * max(1.0, float(full.abs().max()))


def test_bf16_conv_exact_on_small_integers(bf16_mode):
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-4, 5, (1, 96, 13, 15), generator=g).float()            # bf16-representable operands, exact f32 sums
    w = torch.randint(-3, 4, (80, 96, 3, 3), generator=g).float()
    want = F.conv2d(x, w, None, 1, 1)
    for tile in (1, 2, 3, 4):
        y = hip_ops.PackedConv(w.to(DEV), stride=1, pad=1)(x.permute(0, 2, 3, 1).contiguous().to(DEV), tile=tile)
        assert torch.equal(y.cpu().permute(0, 3, 1, 2), want), tile


def test_bf16_transposed_conv_and_residual(bf16_mode):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 64, 9, 11, generator=g)
    w = torch.randn(64, 32, 2, 2, generator=g) / 8
    y = hip_ops.PackedConv(w.to(DEV), stride=2, transposed=True)(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    want = F.conv_transpose2d(x.bfloat16().double(), w.bfloat16().double(), None, 2)
    assert float((y.cpu().double().permute(0, 3, 1, 2) - want).abs().max()) <= 2e-5
    w2 = torch.randn(64, 64, 1, 1, generator=g) / 8
    res = torch.randn(1, 9, 11, 64, generator=g)
    y2 = hip_ops.PackedConv(w2.to(DEV), relu=True)(x.permute(0, 2, 3, 1).contiguous().to(DEV), residual=res.to(DEV))
    want2 = F.relu(F.conv2d(x.bfloat16().double(), w2.bfloat16().double()) + res.double().permute(0, 3, 1, 2))
    assert float((y2.cpu().double().permute(0, 3, 1, 2) - want2).abs().max()) <= 2e-5


def test_bf16_model_forward_close_to_fp32_oracle(bf16_mode):
    from oracle import torch_model as TM
    from sgv3d_amd import synthetic as S
    from sgv3d_amd.models.bev_height import BEVHeight
    torch.manual_seed(0)
    bc, hc = S.small_conf()
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 0)
    imgs = S.make_images(2, bc['final_dim'], seed=5)
    mats = S.make_mats(2, scale=128 / 864)
    keep = {}
    ref = TM.bevheight_forward(m.state_dict(), bc, hc, imgs, mats, keep)
    m = m.to(DEV)
    with torch.no_grad():
        preds = m(imgs.to(DEV), {k: v.to(DEV) for k, v in mats.items()})
    worst = 0.0
    for t in range(6):
        for k, v in preds[t][0].items():
            want = ref[t][0][k]
            err = float((v.cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))
            worst = max(worst, err)
    assert 1e-5 < worst < 5e-2, worst                                        # rounded operands: not the fp32 path, yet close


# ---------------------------------------------------------------------------------------------- f32x3 (three bf16 terms)
@pytest.fixture
def f32x3_mode():
    old = hip_ops.MFMA_F32X3
    hip_ops.MFMA_F32X3 = True
    yield
    hip_ops.MFMA_F32X3 = old


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
def test_f32x3_conv_is_float32_accurate(case, tile):
    """Error against float64 of the split-operand kernel beside that of the f32-MFMA kernel on the same data: the same
    order of magnitude (both are bounded by float32 rounding of products and sums), and within 2e-6 of the output scale."""
    B, cin, H, W, cout, k, stride, pad, dil = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    x = torch.randn(B, cin, H, W, generator=g) * torch.exp(torch.randn(B, cin, 1, 1, generator=g))     # mixed magnitudes
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    want = F.conv2d(x.double(), w.double(), None, stride, pad, dil)
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    errs = {}
    for mode in (False, True):
        hip_ops.MFMA_F32X3 = mode
        try:
            y = hip_ops.PackedConv(w.to(DEV), stride=stride, pad=pad, dil=dil)(xd, tile=tile, split_k=1)
        finally:
            hip_ops.MFMA_F32X3 = False
        errs[mode] = float((y.cpu().double().permute(0, 3, 1, 2) - want).abs().max()) / float(want.abs().max())
    assert errs[True] <= 2e-6, errs
    assert errs[True] <= 4 * errs[False] + 1e-7, errs


def test_f32x3_exact_on_small_integers(f32x3_mode):
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, (1, 96, 13, 15), generator=g).float()
    w = torch.randint(-3, 4, (80, 96, 3, 3), generator=g).float()
    want = F.conv2d(x, w, None, 1, 1)
    for tile in (1, 2, 3, 4):
        y = hip_ops.PackedConv(w.to(DEV), stride=1, pad=1)(x.permute(0, 2, 3, 1).contiguous().to(DEV), tile=tile)
        assert torch.equal(y.cpu().permute(0, 3, 1, 2), want), tile


def test_f32x3_model_forward_meets_the_fp32_bar(f32x3_mode):
    from oracle import torch_model as TM
    from sgv3d_amd import synthetic as S
    from sgv3d_amd.models.bev_height import BEVHeight
    torch.manual_seed(0)
    bc, hc = S.small_conf()
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 0)
    imgs = S.make_images(2, bc['final_dim'], seed=5)
    mats = S.make_mats(2, scale=128 / 864)
    ref = TM.bevheight_forward(m.state_dict(), bc, hc, imgs, mats)
    m = m.to(DEV)
    with torch.no_grad():
        preds = m(imgs.to(DEV), {k: v.to(DEV) for k, v in mats.items()})
    for t in range(6):
        for k, v in preds[t][0].items():
            torch.testing.assert_close(v.cpu(), ref[t][0][k], rtol=1e-3, atol=1e-3)      # the north-star bar of the f32 path


def test_f32x3_auto_mode_model_meets_the_fp32_bar():
    """'auto': f32x3 tiles (host-side ids 11..14) compete with the f32-MFMA tiles and Winograd per layer; whatever mix the
    measurement picks, the model stays inside the 1e-3 bar and at least one layer took an f32x3 tile."""
    from oracle import torch_model as TM
    from sgv3d_amd import synthetic as S
    from sgv3d_amd.models.bev_height import BEVHeight
    torch.manual_seed(0)
    bc, hc = S.small_conf()
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 0)
    imgs = S.make_images(2, bc['final_dim'], seed=5)
    mats = S.make_mats(2, scale=128 / 864)
    ref = TM.bevheight_forward(m.state_dict(), bc, hc, imgs, mats)
    m = m.to(DEV)
    old, old_db = hip_ops.MFMA_F32X3, dict(hip_ops.TUNE_DB)
    hip_ops.MFMA_F32X3 = "auto"
    try:
        with torch.no_grad():
            preds = m(imgs.to(DEV), {k: v.to(DEV) for k, v in mats.items()})
        picked = [v for k, v in hip_ops.TUNE_DB.items() if "|x3auto" in k]
    finally:
        hip_ops.MFMA_F32X3 = old
        hip_ops.TUNE_DB.clear()
        hip_ops.TUNE_DB.update(old_db)
    assert picked and all(t in (1, 2, 3, 4, 5, 6, 8, 11, 12, 13, 14, 21, 22, 23, 24) for t, _ in picked)     # 8: half-position Winograd, 21..24: m-tile first
    for t in range(6):
        for k, v in preds[t][0].items():
            torch.testing.assert_close(v.cpu(), ref[t][0][k], rtol=1e-3, atol=1e-3)


# ---------------------------------------------------------------------------------------------- fused bf16 CenterHead
def _head_case(B, H, W, counts, seed):
    g = torch.Generator().manual_seed(seed)
    nb, total = len(counts), sum(counts)
    x = torch.randn(B, H, W, 64, generator=g)
    w1 = torch.randn(nb * 64, 64, 3, 3, generator=g) / 24.0
    sc, sh = torch.rand(nb * 64, generator=g) + 0.5, torch.randn(nb * 64, generator=g) * 0.2
    w2 = torch.randn(total, 64, 3, 3, generator=g) / 24.0
    b2 = torch.randn(total, generator=g)
    return x, w1, sc, sh, w2, b2


def _head_reference(x, w1, sc, sh, w2, b2, counts, dev):
    """float64 evaluation of what the bf16 kernel computes: bf16-rounded x / w1 / w2, exact products and sums, BN + ReLU in
    high precision, the hidden map rounded to bf16 before the second convolution."""
    r = lambda t: t.to(dev).bfloat16().double()
    hid = F.conv2d(r(x).permute(0, 3, 1, 2), r(w1), padding=1) * sc.to(dev).double()[None, :, None, None] + sh.to(dev).double()[None, :, None, None]
    hid = hid.clamp_min(0).float().bfloat16().double()
    outs, off = [], 0
    for k, c in enumerate(counts):
        outs.append(F.conv2d(hid[:, k * 64:(k + 1) * 64], r(w2[off:off + c]), b2[off:off + c].to(dev).double(), padding=1))
        off += c
    return torch.cat(outs, 1)


@pytest.mark.parametrize("B,H,W,counts", [(1, 16, 16, (2,)), (2, 20, 37, (1, 3)), (1, 50, 33, (2, 1, 3, 2, 2, 1, 1, 3)),
                                          (1, 64, 48, (4, 1))])
def test_fused_centerhead_bf16(B, H, W, counts):
    """sgv3d_centerhead_branches_forward_bf16 == [3x3 64->64 + BN + ReLU] -> bf16 -> [3x3 64->c + bias] per branch, tiles
    that cross the image border in both directions, up to 4 output channels per branch."""
    x, w1, sc, sh, w2, b2 = _head_case(B, H, W, counts, seed=31)
    nb = len(counts)
    ob = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).to(DEV)
    packed = hip_ops.pack_centerhead_bf16(w1.to(DEV), w2.permute(0, 2, 3, 1).contiguous().to(DEV), ob)
    out = hip_ops.centerhead_branches_bf16(x.to(DEV), packed, sc.to(DEV), sh.to(DEV), b2.to(DEV), ob, nb)
    ref = _head_reference(x, w1, sc, sh, w2, b2, counts, DEV)
    assert out.shape == ref.shape
    scale = max(1.0, float(ref.abs().max()))
    err = float((out.double() - ref).abs().max())
    # fp32 accumulation flips the bf16 rounding of a hidden value now and then (one flip moves an output by ~2e-4)
    assert err < 2e-3 * scale, (err, scale)
    again = hip_ops.centerhead_branches_bf16(x.to(DEV), packed, sc.to(DEV), sh.to(DEV), b2.to(DEV), ob, nb)
    assert torch.equal(out, again)
    from sgv3d_amd import _lib
    for variant in (1, 3):              # 1: the single-role kernel, 3: the ping-pong one (default 0: warp-specialised): same arithmetic, same order
        _lib.load().sgv3d_centerhead_bf16_select_plain(variant)
        try:
            other = hip_ops.centerhead_branches_bf16(x.to(DEV), packed, sc.to(DEV), sh.to(DEV), b2.to(DEV), ob, nb)
        finally:
            _lib.load().sgv3d_centerhead_bf16_select_plain(0)
        assert torch.equal(out, other), variant
    # input channels taken as a slice of a wider buffer
    wide = torch.randn(B, H, W, 96).to(DEV)
    wide[..., 16:80] = x.to(DEV)
    sl = hip_ops.centerhead_branches_bf16(wide, packed, sc.to(DEV), sh.to(DEV), b2.to(DEV), ob, nb, x_coff=16)
    assert torch.equal(out, sl)


def test_fused_centerhead_bf16_exact_on_small_integers():
    """bf16-exact operands and hidden values: every product and sum is exact, the result equals the integer convolution."""
    g = torch.Generator().manual_seed(5)
    counts = (2, 1, 3)
    nb, total = len(counts), sum(counts)
    x = torch.randint(-2, 3, (1, 23, 19, 64), generator=g).float()
    w1 = torch.randint(-1, 2, (nb * 64, 64, 3, 3), generator=g).float()
    w1 = w1 * (torch.rand(w1.shape, generator=g) < 0.05)                    # sparse: hidden values stay below 256 (bf16-exact)
    sc, sh = torch.ones(nb * 64), torch.zeros(nb * 64)
    w2 = torch.randint(-1, 2, (total, 64, 3, 3), generator=g).float()
    b2 = torch.randint(-3, 4, (total,), generator=g).float()
    ob = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).to(DEV)
    out = hip_ops.centerhead_branches_bf16(x.to(DEV), hip_ops.pack_centerhead_bf16(w1.to(DEV), w2.permute(0, 2, 3, 1).contiguous().to(DEV), ob),
                                           sc.to(DEV), sh.to(DEV), b2.to(DEV), ob, nb)
    hid = F.conv2d(x.permute(0, 3, 1, 2).double(), w1.double(), padding=1).clamp_min(0)
    assert float(hid.max()) < 256
    ref, off = [], 0
    for k, c in enumerate(counts):
        ref.append(F.conv2d(hid[:, k * 64:(k + 1) * 64], w2[off:off + c].double(), b2[off:off + c].double(), padding=1))
        off += c
    assert torch.equal(out.cpu().double(), torch.cat(ref, 1))


def test_fused_centerhead_bf16_36_branches_256x256_and_speed():
    """The cfg-2 head shape; also prints the kernel time next to the fp32 fused head's."""
    counts = []
    for nc in (1, 2, 2, 1, 2, 2):
        counts += [2, 1, 3, 2, 2, nc]
    x, w1, sc, sh, w2, b2 = _head_case(1, 256, 256, counts, seed=36)
    nb = len(counts)
    ob = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).to(DEV)
    args = (x.to(DEV), hip_ops.pack_centerhead_bf16(w1.to(DEV), w2.permute(0, 2, 3, 1).contiguous().to(DEV), ob), sc.to(DEV), sh.to(DEV),
            b2.to(DEV), ob, nb)
    out = hip_ops.centerhead_branches_bf16(*args)
    ref = _head_reference(x, w1, sc, sh, w2, b2, counts, DEV)
    err = float((out.double() - ref).abs().max())
    assert err < 2e-3 * max(1.0, float(ref.abs().max())), err
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    evs[0].record()
    for i in range(5):
        hip_ops.centerhead_branches_bf16(*args)
        evs[i + 1].record()
    torch.cuda.synchronize()
    us = min(evs[i].elapsed_time(evs[i + 1]) for i in range(5)) * 1e3
    flops = 2.0 * 256 * 256 * (nb * 64 * 576 + sum(counts) * 576)
    print(f"bf16 fused head 36 x 256x256: {us:.0f} us = {flops / us / 1e6:.0f} TFLOP/s algorithmic")
    from sgv3d_amd import _lib
    for variant, name in ((1, "single-role"), (3, "ping-pong")):
        _lib.load().sgv3d_centerhead_bf16_select_plain(variant)
        try:
            o2 = hip_ops.centerhead_branches_bf16(*args)
            evs[0].record()
            for i in range(5):
                hip_ops.centerhead_branches_bf16(*args)
                evs[i + 1].record()
            torch.cuda.synchronize()
        finally:
            _lib.load().sgv3d_centerhead_bf16_select_plain(0)
        assert torch.equal(out, o2)
        print(f"  {name} kernel: {min(evs[i].elapsed_time(evs[i + 1]) for i in range(5)) * 1e3:.0f} us")


# ---------------------------------------------------------------------------------------------- bf16 activations in HBM
@pytest.mark.parametrize("shape", [
    # B, cin, H, W, cout, k, stride, pad, dil, residual
    (2, 64, 20, 28, 256, 1, 1, 0, 1, True),        # expanding 1x1 with residual (ResNet conv3)
    (1, 256, 19, 23, 64, 1, 1, 0, 1, False),       # reducing 1x1, ragged M
    (1, 64, 17, 21, 64, 3, 1, 1, 1, False),        # 3x3
    (2, 128, 18, 22, 128, 3, 2, 1, 1, False),      # strided 3x3
    (1, 256, 16, 16, 512, 1, 2, 0, 1, False),      # strided 1x1 (downsample)
    (1, 512, 9, 11, 136, 3, 1, 2, 2, True),        # dilated, cout not a multiple of 32
    (1, 4, 40, 56, 64, 7, 2, 3, 1, False),         # stem (tap-major K), f32 image in -> bf16 out
])
@pytest.mark.parametrize("tile", [1, 2, 3, 4])
def test_bf16_io_conv(bf16_mode, shape, tile):
    """sgv3d_conv2d_forward_bf16io: bf16 tensors in (io bit 0), out + residual (bit 1), both; every tile shape, split-K.
    Reference: float64 convolution of the bf16-rounded operands, epilogue in high precision, one rounding to bf16."""
    B, cin, H, W, cout, k, stride, pad, dil, with_res = shape
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    conv = hip_ops.PackedConv(w.to(DEV), stride=stride, pad=pad, dil=dil, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    oh, ow = conv.out_hw(H, W)
    res = torch.randn(B, cout, oh, ow, generator=g) if with_res else None
    x_bf16_ok = cin % 8 == 0
    xq = x.bfloat16() if x_bf16_ok else x
    ref = F.conv2d(xq.double() if x_bf16_ok else x.bfloat16().double(), w.bfloat16().double(), None, stride, pad, dil)
    ref = ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    if res is not None:
        ref = ref + res.bfloat16().double()
    ref = ref.clamp_min(0)
    scale = max(1.0, float(ref.abs().max()))
    xin = xq.permute(0, 2, 3, 1).contiguous().to(DEV)                       # bf16 NHWC when the channel count allows it
    rin = res.bfloat16().permute(0, 2, 3, 1).contiguous().to(DEV) if res is not None else None
    for sk in (1, 2):
        y = conv(xin, residual=rin, tile=tile, split_k=sk, out_dtype=torch.bfloat16)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, oh, ow, cout)
        err = float((y.float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max())
        assert err <= 2.0 ** -8 * scale, (sk, err, scale)                  # half an ulp of bf16 at the output scale (+ f32 noise)
    if x_bf16_ok and res is None:                                           # bf16 in -> f32 out (the necks)
        y32 = conv(xin, tile=tile, split_k=1)
        assert y32.dtype == torch.float32
        assert float((y32.permute(0, 3, 1, 2).cpu().double() - ref).abs().max()) <= 2e-5 * scale
    # channel-slice output (concat) in bf16
    wide = torch.zeros(B, oh, ow, cout + 16, dtype=torch.bfloat16, device=DEV)
    conv(xin, wide, y_coff=8, residual=rin, tile=tile, split_k=1)
    assert torch.equal(wide[..., 8:8 + cout], conv(xin, residual=rin, tile=tile, split_k=1, out_dtype=torch.bfloat16))
    assert float(wide[..., :8].abs().max()) == 0 and float(wide[..., 8 + cout:].abs().max()) == 0


@pytest.mark.parametrize("shape", [
    # B, cin, H, W, cout, stride, residual
    (2, 64, 20, 28, 256, 1, True),         # expanding 1x1 with residual (ResNet conv3)
    (1, 256, 19, 23, 64, 1, False),        # reducing 1x1, ragged M
    (1, 256, 16, 16, 512, 2, False),       # strided 1x1 (downsample)
    (1, 32, 9, 13, 72, 1, True),           # K = 32: half a chunk; cout not a multiple of 64
    (1, 96, 11, 10, 136, 1, False),        # K % 64 == 32 with two chunks; waves beyond N
    (3, 2560, 6, 8, 512, 1, True),         # long K (40 chunks)
    (1, 1024, 17, 30, 256, 1, False),      # ResNet layer-3 reducing layer
    (1, 128, 31, 33, 320, 2, True),        # odd strided map, cout = 5 n-chunks of 64
])
@pytest.mark.parametrize("tile", [31, 32, 33, 34, 35, 36, 37, 38, 39])
def test_bf16_direct_weight_conv_1x1(bf16_mode, shape, tile):
    """sgv3d_conv_dw_bf16_forward (host tile ids 31-35 = SGV3D_TILE_DW_*) on 1x1 layers: bf16 tensors in and out.
    Reference: float64 convolution of the bf16-rounded operands, epilogue in high precision, one rounding to bf16 -- and the
    implicit-GEMM bf16io kernel, which multiplies the same bf16 values in the same k order: bitwise equal outputs."""
    B, cin, H, W, cout, stride, with_res = shape
    g = torch.Generator().manual_seed(cin * 5 + cout + stride)
    x = torch.randn(B, cin, H, W, generator=g).bfloat16()
    w = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    conv = hip_ops.PackedConv(w.to(DEV), stride=stride, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    oh, ow = conv.out_hw(H, W)
    res = torch.randn(B, cout, oh, ow, generator=g).bfloat16() if with_res else None
    ref = F.conv2d(x.double(), w.bfloat16().double(), None, stride)
    ref = ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    if res is not None:
        ref = ref + res.double()
    ref = ref.clamp_min(0)
    scale = max(1.0, float(ref.abs().max()))
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rin = res.permute(0, 2, 3, 1).contiguous().to(DEV) if res is not None else None
    y = conv(xin, residual=rin, tile=tile, split_k=1, out_dtype=torch.bfloat16)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (B, oh, ow, cout)
    err = float((y.float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max())
    assert err <= 2.0 ** -8 * scale, (err, scale)
    assert torch.equal(y, conv(xin, residual=rin, tile=4, split_k=1, out_dtype=torch.bfloat16))
    # channel slices on both sides (concat input / output), guard channels untouched
    xw = torch.randn(B, H, W, cin + 24, generator=g).bfloat16().to(DEV)
    xw[..., 16:16 + cin] = xin
    wide = torch.full((B, oh, ow, cout + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    conv(xw, wide, x_coff=16, y_coff=8, residual=rin, tile=tile, split_k=1)
    assert torch.equal(wide[..., 8:8 + cout], y)
    assert float((wide[..., :8] - 7).abs().max()) == 0 and float((wide[..., 8 + cout:] - 7).abs().max()) == 0


@pytest.mark.parametrize("shape", [
    # B, cin, H, W, cout, k, stride, pad, dil, residual
    (1, 64, 17, 21, 64, 3, 1, 1, 1, False),        # 3x3
    (2, 128, 18, 22, 128, 3, 2, 1, 1, False),      # strided 3x3
    (1, 256, 17, 30, 256, 3, 1, 1, 1, True),       # ResNet layer-3 3x3 with a residual
    (1, 512, 20, 24, 136, 3, 1, 6, 6, False),      # dilated (ASPP), cout not a multiple of 64
    (1, 512, 9, 11, 72, 3, 1, 18, 18, True),       # dilation larger than the map: most taps outside
    (1, 96, 40, 56, 160, 7, 2, 3, 1, False),       # 7x7 stride-2 BEV stem, cin % 64 == 32 (tap chunks half dead)
    (2, 160, 13, 13, 320, 3, 2, 1, 1, False),      # cin = 2.5 chunks per tap
    (1, 32, 12, 9, 64, 5, 1, 2, 1, True),          # 5x5, cin = half a chunk
])
@pytest.mark.parametrize("tile", [31, 32, 33, 34, 35, 36, 37, 38, 39])
def test_bf16_direct_weight_conv_kxk(bf16_mode, shape, tile):
    """The same kernel as an implicit GEMM over taps: padding, stride, dilation, 7x7; against float64 on the bf16-rounded
    operands (half an ulp of bf16 at the output scale) and against the bf16io implicit-GEMM kernel (other k order: 1 bf16 ulp)."""
    B, cin, H, W, cout, k, stride, pad, dil, with_res = shape
    g = torch.Generator().manual_seed(cin * 3 + cout + k)
    x = torch.randn(B, cin, H, W, generator=g).bfloat16()
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    conv = hip_ops.PackedConv(w.to(DEV), stride=stride, pad=pad, dil=dil, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    oh, ow = conv.out_hw(H, W)
    res = torch.randn(B, cout, oh, ow, generator=g).bfloat16() if with_res else None
    ref = F.conv2d(x.double(), w.bfloat16().double(), None, stride, pad, dil)
    ref = ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    if res is not None:
        ref = ref + res.double()
    ref = ref.clamp_min(0)
    scale = max(1.0, float(ref.abs().max()))
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rin = res.permute(0, 2, 3, 1).contiguous().to(DEV) if res is not None else None
    y = conv(xin, residual=rin, tile=tile, split_k=1, out_dtype=torch.bfloat16)
    err = float((y.float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max())
    assert err <= 2.0 ** -8 * scale, (err, scale)
    y_ig = conv(xin, residual=rin, tile=4, split_k=1, out_dtype=torch.bfloat16)
    assert float((y.float() - y_ig.float()).abs().max()) <= 2.0 ** -7 * scale
    xw = torch.randn(B, H, W, cin + 24, generator=g).bfloat16().to(DEV)
    xw[..., 16:16 + cin] = xin
    wide = torch.full((B, oh, ow, cout + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    conv(xw, wide, x_coff=16, y_coff=8, residual=rin, tile=tile, split_k=1)
    assert torch.equal(wide[..., 8:8 + cout], y)
    assert float((wide[..., :8] - 7).abs().max()) == 0 and float((wide[..., 8 + cout:] - 7).abs().max()) == 0


@pytest.mark.parametrize("shape", [
    # B, cin, H, W, k, stride, pad, dil, cout2, residual
    (1, 256, 17, 30, 3, 1, 1, 1, 1024, True),       # ResNet layer-3 bottleneck: conv2 + conv3
    (2, 256, 9, 13, 3, 1, 1, 1, 1024, True),        # ragged M (234 pixels), two images
    (1, 256, 20, 22, 3, 2, 1, 1, 1024, True),       # the strided first block of the layer
    (1, 96, 11, 10, 1, 1, 0, 1, 256, False),        # 1x1 first layer (plain gather), K % 64 == 32, a single output chunk
    (1, 128, 12, 16, 3, 1, 2, 2, 512, False),       # dilated first layer, no residual
])
def test_bf16_direct_weight_conv_pair(bf16_mode, shape):
    """sgv3d_conv_dw_bf16_pair_forward: conv A (k x k -> 256, BN, ReLU) + conv B (1x1 -> cout2, BN, residual, ReLU) in one launch
    with the 256-channel map in LDS: bitwise the two direct-weight launches, and close to float64 on the bf16-rounded operands
    (the middle map rounded to bf16 as both paths do)."""
    B, cin, H, W, k, stride, pad, dil, cout2, with_res = shape
    g = torch.Generator().manual_seed(cin + cout2 + k + stride)
    x = torch.randn(B, cin, H, W, generator=g).bfloat16()
    wa = torch.randn(256, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    wb = torch.randn(cout2, 256, 1, 1, generator=g) / 16.0
    sa, ha = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.3
    sb, hb = torch.rand(cout2, generator=g) + 0.5, torch.randn(cout2, generator=g) * 0.3
    ca = hip_ops.PackedConv(wa.to(DEV), stride=stride, pad=pad, dil=dil, scale=sa.to(DEV), shift=ha.to(DEV), relu=True)
    cb = hip_ops.PackedConv(wb.to(DEV), scale=sb.to(DEV), shift=hb.to(DEV), relu=True)
    oh, ow = ca.out_hw(H, W)
    res = torch.randn(B, cout2, oh, ow, generator=g).bfloat16() if with_res else None
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rin = res.permute(0, 2, 3, 1).contiguous().to(DEV) if res is not None else None
    assert hip_ops.conv_pair_eligible(ca, cb, xin, rin)
    y = hip_ops.conv_pair_bf16(ca, cb, xin, rin)
    mid = ca(xin, tile=31, split_k=1, out_dtype=torch.bfloat16)
    want = cb(mid, residual=rin, tile=31, split_k=1, out_dtype=torch.bfloat16)
    assert torch.equal(y, want)
    m64 = F.conv2d(x.double(), wa.bfloat16().double(), None, stride, pad, dil)
    m64 = (m64 * sa.double()[None, :, None, None] + ha.double()[None, :, None, None]).clamp_min(0).bfloat16().double()
    ref = F.conv2d(m64, wb.bfloat16().double()) * sb.double()[None, :, None, None] + hb.double()[None, :, None, None]
    if res is not None:
        ref = ref + res.double()
    ref = ref.clamp_min(0)
    scale = max(1.0, float(ref.abs().max()))
    assert float((y.float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max()) <= 2.0 ** -6 * scale   # (+ rounding flips of the middle map)


@pytest.mark.parametrize("shape", [
    # B, cin, H, W, cout, k, stride, pad, dil, residual, split
    (1, 256, 17, 30, 256, 3, 1, 1, 1, True, 2),       # 36 chunks, two halves
    (1, 512, 20, 24, 136, 3, 1, 6, 6, False, 5),      # dilated, cout not a multiple of 64, uneven chunk ranges (72 / 5)
    (1, 96, 40, 56, 160, 7, 2, 3, 1, False, 8),       # 147 blocks -> 74 chunks (the last half dead); ranges start inside a tap
    (2, 160, 13, 13, 320, 3, 2, 1, 1, False, 3),      # 2.5 chunks per tap: split boundaries in the middle of a tap
    (1, 2048, 9, 11, 512, 1, 1, 0, 1, True, 8),       # 1x1 (the plain gather), 32 chunks
    (1, 64, 12, 9, 64, 3, 1, 1, 1, True, 9),          # one chunk per workgroup (split == chunks)
])
@pytest.mark.parametrize("tile", [31, 32, 33, 34, 35, 38])
def test_bf16_direct_weight_conv_split_k(bf16_mode, shape, tile):
    """sgv3d_conv_dw_bf16_forward_splitk: the k loop over `split` workgroups per tile, partial tiles summed in split order by the
    reduce kernel which also runs the epilogue.  Against float64 on the bf16-rounded operands, within one bf16 ulp of the unsplit
    kernel (the f32 partial sums associate differently), bitwise repeatable, strided in / out tensors."""
    B, cin, H, W, cout, k, stride, pad, dil, with_res, split = shape
    g = torch.Generator().manual_seed(cin * 5 + cout + k + split)
    x = torch.randn(B, cin, H, W, generator=g).bfloat16()
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    conv = hip_ops.PackedConv(w.to(DEV), stride=stride, pad=pad, dil=dil, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    oh, ow = conv.out_hw(H, W)
    res = torch.randn(B, cout, oh, ow, generator=g).bfloat16() if with_res else None
    ref = F.conv2d(x.double(), w.bfloat16().double(), None, stride, pad, dil)
    ref = ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    if res is not None:
        ref = ref + res.double()
    ref = ref.clamp_min(0)
    scale = max(1.0, float(ref.abs().max()))
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rin = res.permute(0, 2, 3, 1).contiguous().to(DEV) if res is not None else None
    y = conv(xin, residual=rin, tile=tile, split_k=split, out_dtype=torch.bfloat16)
    err = float((y.float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max())
    assert err <= 2.0 ** -8 * scale, (err, scale)
    y1 = conv(xin, residual=rin, tile=tile, split_k=1, out_dtype=torch.bfloat16)
    assert float((y.float() - y1.float()).abs().max()) <= 2.0 ** -7 * scale
    assert torch.equal(y, conv(xin, residual=rin, tile=tile, split_k=split, out_dtype=torch.bfloat16))
    xw = torch.randn(B, H, W, cin + 24, generator=g).bfloat16().to(DEV)
    xw[..., 16:16 + cin] = xin
    wide = torch.full((B, oh, ow, cout + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    conv(xw, wide, x_coff=16, y_coff=8, residual=rin, tile=tile, split_k=split)
    assert torch.equal(wide[..., 8:8 + cout], y)
    assert float((wide[..., :8] - 7).abs().max()) == 0 and float((wide[..., 8 + cout:] - 7).abs().max()) == 0


@pytest.mark.parametrize("shape", [
    # B, cin, H, W, cout, k, stride, pad, dil, residual
    (1, 1024, 27, 48, 256, 1, 1, 0, 1, False),     # 16 chunks, even count
    (1, 96, 13, 17, 256, 1, 1, 0, 1, True),        # 1.5 chunks -> two, the second half dead
    (1, 32, 9, 9, 72, 1, 1, 0, 1, False),          # a single (half) chunk: nothing to prefetch
    (1, 64, 11, 13, 136, 3, 1, 1, 1, True),        # 9 chunks (odd count), taps outside the image
    (2, 160, 13, 13, 320, 3, 2, 1, 1, False),      # 2.5 chunks per tap, strided
    (1, 128, 10, 12, 128, 3, 1, 2, 2, True),       # dilated, 18 chunks
])
def test_bf16_direct_weight_conv_deep_prefetch_is_bitwise_the_plain_tile(bf16_mode, shape):
    """SGV3D_TILE_DW_64x256_DEEP / 128x128_DEEP request rows and fragments two k-chunks ahead (two register sets, loop unrolled by
    two, the last chunk on either set): the same products in the same order as tiles 31 / 32 -- bitwise, for even and odd chunk
    counts, one and two chunks, dead half chunks."""
    B, cin, H, W, cout, k, stride, pad, dil, with_res = shape
    g = torch.Generator().manual_seed(cin + cout + k)
    x = torch.randn(B, H, W, cin, generator=g).bfloat16().to(DEV)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    conv = hip_ops.PackedConv(w.to(DEV), stride=stride, pad=pad, dil=dil, scale=(torch.rand(cout, generator=g) + 0.5).to(DEV),
                              shift=torch.randn(cout, generator=g).to(DEV), relu=True)
    oh, ow = conv.out_hw(H, W)
    res = torch.randn(B, oh, ow, cout, generator=g).bfloat16().to(DEV) if with_res else None
    for plain, deep in ((31, 36), (32, 37), (38, 39)):
        want = conv(x, residual=res, tile=plain, split_k=1, out_dtype=torch.bfloat16)
        got = conv(x, residual=res, tile=deep, split_k=1, out_dtype=torch.bfloat16)
        assert torch.equal(got, want), (plain, deep)


def test_bf16_direct_weight_conv_exact_on_small_integers(bf16_mode):
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-3, 4, (2, 192, 12, 21), generator=g).float()
    for k, pad in ((1, 0), (3, 1)):
        w = torch.randint(-2, 3, (200, 192, k, k), generator=g).float()
        conv = hip_ops.PackedConv(w.to(DEV), pad=pad)
        ref = F.conv2d(x, w, None, 1, pad)                                  # integer sums below 2^24: exact in the f32 accumulators
        xin = x.bfloat16().permute(0, 2, 3, 1).contiguous().to(DEV)
        for tile in (31, 32, 33, 34, 35, 36, 37, 38, 39):
            for split in ((1,) if tile in (36, 37, 39) else (1, 3)):                   # (exact partial sums: any association gives the same bits)
                y = conv(xin, tile=tile, split_k=split, out_dtype=torch.bfloat16)
                assert torch.equal(y.float().permute(0, 3, 1, 2).cpu(), ref.bfloat16().float())


def test_bf16_direct_weight_conv_rejects_what_it_does_not_cover(bf16_mode):
    from sgv3d_amd import _lib
    conv = hip_ops.PackedConv(torch.randn(64, 64, 3, 3, device=DEV), pad=1)
    x = torch.randn(1, 8, 8, 64, device=DEV)
    with pytest.raises(_lib.SGV3DError):
        conv(x, tile=31, split_k=1)                                         # f32 tensors
    with pytest.raises(_lib.SGV3DError):
        conv(x.bfloat16(), tile=31, split_k=10, out_dtype=torch.bfloat16)   # more splits than the 9 k-chunks of the layer
    up = hip_ops.PackedConv(torch.randn(64, 32, 2, 2, device=DEV), stride=2, transposed=True)
    with pytest.raises(_lib.SGV3DError):
        up(x.bfloat16(), tile=31, split_k=2, out_dtype=torch.bfloat16)      # split-K of a transposed convolution


def test_bf16_maxpool(bf16_mode):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 21, 30, generator=g).bfloat16()
    y = hip_ops.maxpool3x3s2(x.permute(0, 2, 3, 1).contiguous().to(DEV))
    want = F.max_pool2d(x.float(), 3, 2, 1)
    assert y.dtype == torch.bfloat16 and torch.equal(y.float().permute(0, 3, 1, 2).cpu(), want)
    # NaN propagates as in F.max_pool2d: one NaN, a window of NaNs only, an all -inf window
    x[:, 0, 3, 5] = float("nan")
    x[:, 1, :2, :2] = float("nan")
    x[:, 2, :2, :2] = float("-inf")
    x[:, 4, 7, 8:10] = float("nan")
    y = hip_ops.maxpool3x3s2(x.permute(0, 2, 3, 1).contiguous().to(DEV)).float().permute(0, 3, 1, 2).cpu()
    want = F.max_pool2d(x.float(), 3, 2, 1)
    assert bool(want.isnan().any()) and bool(want.isneginf().any())
    assert torch.equal(y.isnan(), want.isnan()) and torch.equal(torch.nan_to_num(y, nan=0.0), torch.nan_to_num(want, nan=0.0))


@pytest.mark.parametrize("cin,cout,ks,H,W,x_bf16", [(64, 32, 2, 9, 11, True), (160, 64, 4, 6, 7, True), (80, 64, 1, 10, 12, False),
                                                    (640, 64, 8, 4, 5, True), (1024, 128, 1, 17, 15, True), (256, 128, 4, 19, 13, True)])
def test_bf16_io_transposed_conv(bf16_mode, cin, cout, ks, H, W, x_bf16):
    """SECONDFPN deblocks (ConvTranspose2d, kernel == stride) writing a channel slice of a bf16 concat buffer."""
    g = torch.Generator().manual_seed(cin + ks)
    B = 2
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cin, cout, ks, ks, generator=g) / cin ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    conv = hip_ops.PackedConv(w.to(DEV), stride=ks, transposed=True, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    ref = F.conv_transpose2d(x.bfloat16().double(), w.bfloat16().double(), None, stride=ks)
    ref = (ref * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]).clamp_min(0)
    xin = (x.bfloat16() if x_bf16 else x).permute(0, 2, 3, 1).contiguous().to(DEV)
    out = torch.zeros(B, H * ks, W * ks, cout + 24, dtype=torch.bfloat16, device=DEV)
    for tile in (1, 2, 3, 4):
        out.zero_()
        conv(xin, out, y_coff=16, tile=tile, split_k=1)
        got = out[..., 16:16 + cout].float().permute(0, 3, 1, 2).cpu().double()
        assert float((got - ref).abs().max()) <= 2.0 ** -8 * max(1.0, float(ref.abs().max())), tile
        assert float(out[..., :16].abs().max()) == 0 and float(out[..., 16 + cout:].abs().max()) == 0
    conv(xin, out, y_coff=16, tile=4, split_k=2)
    assert float((out[..., 16:16 + cout].float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max()) <= 2.0 ** -8 * max(1.0, float(ref.abs().max()))
    if x_bf16 and cin % 32 == 0:           # the direct-weight kernel in DECONV mode: bitwise the implicit-GEMM result
        conv(xin, out, y_coff=16, tile=4, split_k=1)
        want = out.clone()
        for tile in (31, 32, 33, 34, 35):
            out.zero_()
            conv(xin, out, y_coff=16, tile=tile, split_k=1)
            assert torch.equal(out, want), tile


# ---------------------------------------------------------------------------------------------- LDS-resident-patch 3x3 kernel
@pytest.mark.parametrize("shape", [
    # B, cin, H, W, cout, residual
    (1, 32, 16, 32, 64, False),        # exactly one tile, one chunk
    (2, 64, 17, 35, 64, True),         # ragged tile edges, two chunks
    (1, 160, 33, 20, 160, True),       # BEV trunk widths (cout = 2.5 tiles of 64)
    (1, 512, 9, 11, 40, False),        # long K, cout % 64 = 40
    (3, 96, 40, 70, 264, True),        # several tiles in x / y / channel, batch
])
@pytest.mark.parametrize("io", [0, 1, 2, 3])
def test_bf16_patch_conv(bf16_mode, shape, io):
    """sgv3d_conv3x3_patch_bf16_forward (tile id 7) against a float64 convolution of the bf16-rounded operands, for the four
    combinations of f32 / bf16 input and output; bitwise equal is not expected against the implicit-GEMM kernel (other k order)."""
    B, cin, H, W, cout, with_res = shape
    g = torch.Generator().manual_seed(cin * 13 + cout + io)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.3
    conv = hip_ops.PackedConv(w.to(DEV), stride=1, pad=1, scale=sc.to(DEV), shift=sh.to(DEV), relu=True)
    xb, yb = bool(io & 1), bool(io & 2)
    res = torch.randn(B, cout, H, W, generator=g) if with_res else None
    xq = x.bfloat16()
    ref = F.conv2d(xq.double(), w.bfloat16().double(), None, 1, 1) * sc.double()[None, :, None, None] + sh.double()[None, :, None, None]
    if res is not None:
        ref = ref + (res.bfloat16() if yb else res).double()
    ref = ref.clamp_min(0)
    scale = max(1.0, float(ref.abs().max()))
    xin = (xq if xb else x).permute(0, 2, 3, 1).contiguous().to(DEV)
    rin = None if res is None else (res.bfloat16() if yb else res).permute(0, 2, 3, 1).contiguous().to(DEV)
    odt = torch.bfloat16 if yb else torch.float32
    y = conv(xin, residual=rin, tile=hip_ops.TILE_PATCH, out_dtype=odt)
    assert y.dtype == odt and tuple(y.shape) == (B, H, W, cout)
    err = float((y.float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max())
    assert err <= (2.0 ** -8 if yb else 2e-5) * scale, (err, scale)
    # against the implicit-GEMM kernel: same operands, different summation order
    y2 = conv(xin, residual=rin, tile=4, split_k=1, out_dtype=odt)
    assert float((y.float() - y2.float()).abs().max()) <= (2.0 ** -7 if yb else 2e-5) * scale
    # split over the 32-channel stages of cin (small maps): partial sums + the shared reduce kernel
    for sk in (2, 3):
        if cin // 32 >= sk:
            y3 = conv(xin, residual=rin, tile=hip_ops.TILE_PATCH, split_k=sk, out_dtype=odt)
            err3 = float((y3.float().permute(0, 3, 1, 2).cpu().double() - ref).abs().max())
            assert err3 <= (2.0 ** -8 if yb else 2e-5) * scale, (sk, err3, scale)
    # channel-slice input and output
    wide_in = torch.zeros(B, H, W, cin + 16, dtype=xin.dtype, device=DEV)
    wide_in[..., 8:8 + cin] = xin
    wide = torch.zeros(B, H, W, cout + 16, dtype=odt, device=DEV)
    conv(wide_in, wide, x_coff=8, y_coff=8, residual=rin, tile=hip_ops.TILE_PATCH)
    assert torch.equal(wide[..., 8:8 + cout], y)
    assert float(wide[..., :8].abs().max()) == 0 and float(wide[..., 8 + cout:].abs().max()) == 0


def test_bf16_patch_conv_exact_on_small_integers(bf16_mode):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (2, 64, 20, 37), generator=g).float()
    w = torch.randint(-2, 3, (72, 64, 3, 3), generator=g).float()
    conv = hip_ops.PackedConv(w.to(DEV), stride=1, pad=1)
    y = conv(x.permute(0, 2, 3, 1).contiguous().to(DEV), tile=hip_ops.TILE_PATCH)
    assert torch.equal(y.permute(0, 3, 1, 2).cpu(), F.conv2d(x, w, None, 1, 1))


# ---------------------------------------------------------------------------------------------- bf16 twins of the small layers
def _bf(t):
    return t.bfloat16().to(DEV)


def test_bf16_small_layers_match_f32_twins():
    """act_bf16.hip: each kernel == its float32 twin evaluated on the same (bf16-representable) inputs, rounded once to bf16."""
    g = torch.Generator().manual_seed(11)
    B, H, W, C = 2, 9, 13, 64
    x = torch.randn(B, H, W, C, generator=g).bfloat16()
    xf = x.float().to(DEV)
    gate = torch.rand(B, C, generator=g).to(DEV)
    # SELayer gate
    assert torch.equal(hip_ops.scale_channels(x.to(DEV), gate), hip_ops.scale_channels(xf, gate).bfloat16())
    # global average pooling: f32 result, same two-stage summation order
    assert torch.equal(hip_ops.global_avgpool(x.to(DEV)), hip_ops.global_avgpool(xf))
    # broadcast into a channel slice
    v = torch.randn(B, 32, generator=g).to(DEV)
    wide = torch.zeros(B, H, W, 96, dtype=torch.bfloat16, device=DEV)
    hip_ops.broadcast_channels(v, wide, y_coff=48)
    ref = torch.zeros(B, H, W, 96, device=DEV)
    hip_ops.broadcast_channels(v, ref, y_coff=48)
    assert torch.equal(wide, ref.bfloat16())
    # bilinear x2
    assert torch.equal(hip_ops.upsample_bilinear2x(x.to(DEV)), hip_ops.upsample_bilinear2x(xf).bfloat16())
    # a + b * sigmoid(c)
    a, b, c = (torch.randn(B, H, W, C, generator=g).bfloat16() for _ in range(3))
    assert torch.equal(hip_ops.add_mul_sigmoid(a.to(DEV), b.to(DEV), c.to(DEV)),
                       hip_ops.add_mul_sigmoid(a.float().to(DEV), b.float().to(DEV), c.float().to(DEV)).bfloat16())
    # deformable sampling (offsets stay f32), 4 groups
    off = (torch.randn(B, H, W, 18, generator=g) * 1.5).to(DEV)
    assert torch.equal(hip_ops.deform_im2col3x3(x.to(DEV), off, 4), hip_ops.deform_im2col3x3(xf, off, 4).bfloat16())


def test_bf16_small_layers_reject_odd_channels():
    from sgv3d_amd._lib import SGV3DError
    x = torch.zeros(1, 4, 4, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(SGV3DError):
        hip_ops.scale_channels(x, torch.ones(1, 12, device=DEV))
    with pytest.raises(SGV3DError):
        hip_ops.upsample_bilinear2x(x)


def test_bf16_lift_and_pooling_match_f32_twins(bf16_mode):
    """sgv3d_lift_bf16 == the f32 lift rounded once; sgv3d_voxel_pooling_forward_planned_bf16 == the f32 gather on the same
    (bf16-representable) feature rows, bit for bit (sums are f32 in the same order)."""
    from sgv3d_amd.ops.voxel_pooling import VoxelPlan
    g = torch.Generator().manual_seed(3)
    B, fH, fW, D, C = 2, 9, 14, 12, 40
    hc = torch.randn(B, fH, fW, D + C, generator=g).to(DEV)
    _, lifted32 = hip_ops.lift(hc, D, C)
    prob, lifted16 = hip_ops.lift(hc, D, C, want_prob=True, lifted_dtype=torch.bfloat16)
    assert lifted16.dtype == torch.bfloat16 and torch.equal(lifted16, lifted32.bfloat16())
    assert torch.equal(prob, hip_ops.lift(hc, D, C, want_prob=True, want_lifted=False)[0])
    N = D * fH * fW
    geom = torch.stack([torch.randint(-2, 18, (B, N), generator=g), torch.randint(-2, 22, (B, N), generator=g),
                        torch.randint(-1, 2, (B, N), generator=g)], -1).int().to(DEV)
    plan = VoxelPlan(geom, (16, 20, 1))
    out16 = plan.pool(lifted16.view(B, N, C))
    out32 = plan.pool(lifted16.float().view(B, N, C))
    assert out16.dtype == torch.float32 and torch.equal(out16, out32)


def test_bf16_pooling_padded_bf16_output(bf16_mode):
    """out_bf16_ld: the pooled map as bf16 rows padded with zero channels == the f32 result rounded once."""
    from sgv3d_amd.ops.voxel_pooling import VoxelPlan
    g = torch.Generator().manual_seed(4)
    B, N, C = 2, 5000, 88
    feats = torch.randn(B, N, C, generator=g).bfloat16().to(DEV)
    geom = torch.stack([torch.randint(-2, 34, (B, N), generator=g), torch.randint(-2, 30, (B, N), generator=g),
                        torch.randint(-1, 2, (B, N), generator=g)], -1).int().to(DEV)
    plan = VoxelPlan(geom, (32, 28, 1))
    ref = plan.pool(feats)                                   # f32 [B, 28, 32, 88]
    out = plan.pool(feats, out_bf16_ld=96)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (B, 28, 32, 96)
    assert torch.equal(out[..., :C], ref.bfloat16()) and float(out[..., C:].abs().max()) == 0
