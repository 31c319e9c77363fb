"""tests/small_layers_ref.py checked on the CPU: each float64 restatement equals torch.nn.functional in float64 on the inputs
tests/test_small_layers_gpu.py uses, and every claim that file leans on -- "exact for integer inputs", "the reference is a
bf16 value", "no pixel sits at the threshold", "the hand-placed offsets hit every boundary value" -- holds for the reference
alone."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_layers_ref as R

F64 = torch.float64
MAXPOOL_HW = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 8), (8, 3), (7, 10), (4, 6)]
UPSAMPLE_HW = [(1, 1), (1, 3), (4, 1), (2, 2), (5, 7)]
DEFORM_HW = [(1, 1), (1, 5), (3, 4)]
HEAD_WIDTHS = [[2, 1, 3, 2, 2, 1], [4, 1], [2, 0, 3]]


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def _equal_nan(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


# ------------------------------------------------------------------------------------------------------------- rounding
def test_round_bf16_rounds_once_to_nearest_even():
    g = R.gen(1)
    x = torch.randn(4096, generator=g)
    assert torch.equal(R.round_bf16(x.double()), x.bfloat16().double())         # f32 -> bf16 is one rounding in torch too
    # 1 + 2^-8 is a tie (even neighbour 1); a hair above it rounds up.  Through float32 the hair is lost first.
    tie = torch.tensor([1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8 - 2.0 ** -40], dtype=F64)
    assert R.round_bf16(tie).tolist() == [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6, -1 - 2.0 ** -7]
    assert tie[1].float().bfloat16().item() == 1.0                               # the double rounding round_bf16 avoids
    special = torch.tensor([0.0, -0.0, math.inf, -math.inf, 3.0, -1024.0], dtype=F64)
    assert torch.equal(R.round_bf16(special), special) and bool(R.round_bf16(torch.tensor([math.nan], dtype=F64)).isnan())
    assert R.is_bf16(torch.tensor([0.75, -3.0, 2.0625])) and not R.is_bf16(torch.tensor([1 + 2.0 ** -8]))


# ------------------------------------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("hw", MAXPOOL_HW)
def test_maxpool_is_torch(hw):
    H, W = hw
    for C in (4, 8, 72):
        x = R.randn_bf16((2, H, W, C), R.gen(H, W, C))
        assert R.is_bf16(x)
        variants = [x]
        if (H, W) == (7, 10):
            variants.append(R.nan_windows(x.clone()))
        if H % 2 == 0 and W % 2 == 0:
            variants.append(R.nan_clipped_corner(x.clone()))
        for v in variants:
            want = F.max_pool2d(nchw(v).double(), 3, 2, 1)
            assert _equal_nan(nchw(R.maxpool3x3s2(v)), want)
            if v is not x:
                assert bool(want.isnan().any()) and bool(want.isneginf().any())
                assert bool(want[..., -1, -1].isnan().any())                      # the clipped last window / the two-NaN window


# -------------------------------------------------------------------------------------------------- mean, dense, sigmoid
@pytest.mark.parametrize("P", [1, 31, 32, 33, 129])
def test_global_mean_is_torch_and_exact_on_integers(P):
    for C in (1, 64, 65, 100):
        for ld in (C, C + 12):
            g = R.gen(P, C, ld)
            xi, xr = R.ints((2, P, ld), g), R.randn_bf16((2, P, ld), g)
            assert R.is_bf16(xi) and R.is_bf16(xr)
            for x in (xi, xr):
                want = F.adaptive_avg_pool2d(x[..., :C].double().permute(0, 2, 1)[..., None], 1).reshape(2, C)
                assert float((R.global_mean(x, C) - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max()))
                assert bool((R.global_mean(x, C, magnitude=True) >= R.global_mean(x, C).abs()).all())
            if P & (P - 1) == 0:
                # every partial sum is an integer of magnitude <= 3 P < 2^24 and P divides exactly: exact in f32, any order
                assert 3 * P < 2 ** 24 and R.is_f32(R.global_mean(xi, C))


@pytest.mark.parametrize("K", [1, 27, 63, 64, 65, 200])
def test_dense_is_torch(K):
    for N in (1, 3, 100):
        for B in (1, 3):
            g = R.gen(K, N, B)
            x, w = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
            scale, bias = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
            for s in (None, scale):
                for b in (None, bias):
                    v = F.linear(x.double(), w.double())
                    v = v * s.double() if s is not None else v
                    v = v + b.double() if b is not None else v
                    for act, want in ((R.ACT_NONE, v), (R.ACT_RELU, F.relu(v)), (R.ACT_SIGMOID, torch.sigmoid(v))):
                        got = R.dense(x, w, s, b, act)
                        assert float((got - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))
                        S = R.dense(x, w, s, b, act, magnitude=True)
                        assert bool((S >= got.abs()).all())
                        if act == R.ACT_SIGMOID:                                  # S = S_linear / 4 + sigmoid
                            assert torch.allclose(S, R.dense(x, w, s, b, R.ACT_NONE, magnitude=True) / 4 + want, rtol=1e-14, atol=0)


def test_sigmoid_caps():
    """sigmoid's slope is at most 1/4 (the factor of the argument's error) and the relative error of 1 / (1 + e) from a
    relative error d of e is e / (1 + e) d <= d: what R.dense's sigmoid S and R.SIGMOID_ROUNDINGS rest on."""
    v = torch.linspace(-30, 30, 20001, dtype=F64)
    s = torch.sigmoid(v)
    assert float((s * (1 - s)).max()) <= 0.25
    e, d = torch.exp(-v), 1e-6
    assert bool(((1 / (1 + e * (1 + d)) - s).abs() <= d * s).all())
    assert R.SIGMOID_ROUNDINGS == R.EXPF_ROUNDINGS + 2 and R.EXPF_ROUNDINGS == 4   # 2 ulp = 4 * 2^-24 (assumed)
    # expf overflows in f32 where sigmoid is already below the smallest normal: the absolute term of the GPU test
    assert float(torch.sigmoid(torch.tensor(-math.log(float(np.finfo(np.float32).max)), dtype=F64))) < R.F32_TINY


@pytest.mark.parametrize("n", [4, 8, 1016, 1020, 1024 + 8])
def test_add_mul_sigmoid_is_torch(n):
    g = R.gen(n)
    a, b = R.randn_bf16((n,), g), R.randn_bf16((n,), g)
    c = (torch.rand(n, generator=g) * 200 - 100).bfloat16().float()
    c[:4] = torch.tensor([math.inf, -math.inf, 0.0, -100.0])
    want = a.double() + b.double() * torch.sigmoid(c.double())
    got = R.add_mul_sigmoid(a, b, c)
    assert float((got - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max()))
    assert got[0] == a[0].double() + b[0].double() and got[1] == a[1].double() and got[2] == a[2].double() + 0.5 * b[2].double()
    assert bool((R.add_mul_sigmoid(a, b, c, magnitude=True) >= got.abs()).all())


# ------------------------------------------------------------------------------------------------------------ bilinear
@pytest.mark.parametrize("hw", UPSAMPLE_HW)
def test_bilinear2x_is_torch_and_exact_on_integers(hw):
    H, W = hw
    for C in (4, 7, 8, 72):
        g = R.gen(H, W, C)
        xi, xr = R.ints((2, H, W, C), g), R.randn_bf16((2, H, W, C), g)
        for x in (xi, xr):
            want = F.interpolate(nchw(x).double(), scale_factor=2, mode="bilinear", align_corners=False)
            assert float((nchw(R.bilinear2x(x)) - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max()))
        yi = R.bilinear2x(xi)
        # weights are products of {0, 1/4, 3/4, 1}: multiples of 1/16; |y| <= 3: 6 bits -- a bf16 (and f32) value, and so is
        # every intermediate of the kernel's expression (each a multiple of 1/16 of magnitude <= 3)
        assert torch.equal(yi * 16, (yi * 16).round()) and float(yi.abs().max()) <= 3 and R.is_bf16(yi) and R.is_f32(yi)


# ----------------------------------------------------------------------------------------------------------------- BSM
@pytest.mark.parametrize("case", R.BSM_CASES, ids=lambda c: "sem%d_ld%d_pad%d_ctx%d_px%d" % c)
def test_bsm_compose_is_torch_and_no_pixel_sits_at_the_threshold(case):
    buf, logits, D, ctx, sem, thr = R.bsm_case(*case)
    assert R.is_f32(logits[..., :sem] * 1024) and float(logits[..., :sem].abs().max()) < 16   # logit - max exact in f32
    got, p0 = R.bsm_compose(buf, logits, D, ctx, sem, thr)
    p = F.softmax(logits[..., :sem].double(), -1)
    keep = (~(p[..., :1] > float(np.float32(thr)))).double()
    assert float((p0 - p[..., 0]).abs().max()) <= 1e-15
    assert torch.equal(got[..., :D], buf[..., :D].double())
    assert torch.equal(got[..., D:D + ctx], buf[..., D:D + ctx].double() * keep)
    assert float((got[..., D + ctx:D + ctx + sem] - p * keep).abs().max()) <= 1e-15
    assert bool((got[..., D + ctx + sem:] == 0).all()) and not bool(got.isnan().any())
    near = (p0 - float(np.float32(thr))).abs() < R.BSM_EXCLUDE
    assert float(near.double().mean()) <= 0.01


def test_bsm_cases_zero_and_keep_pixels_and_tie_is_exact():
    kept = total = 0
    for case in R.BSM_CASES:
        buf, logits, D, ctx, sem, thr = R.bsm_case(*case)
        _, p0 = R.bsm_compose(buf, logits, D, ctx, sem, thr)
        kept += int((p0 <= thr).sum())
        total += p0.numel()
    assert 0.2 * total < kept < 0.8 * total                                      # both decisions are exercised
    logits = torch.tensor([[[-2.0, -2.0]], [[3.0, 3.0]]])
    buf = torch.ones(2, 1, 3 + 5 + 2 + 1)
    for thr, keep in ((0.5, 1.0), (float(np.nextafter(np.float32(0.5), np.float32(0))), 0.0)):
        got, p0 = R.bsm_compose(buf, logits, 3, 5, 2, thr)
        assert bool((p0 == 0.5).all()) and bool((got[..., 3:8] == keep).all()) and bool((got[..., 8:10] == 0.5 * keep).all())


# ------------------------------------------------------------------------------------------------- deformable sampling
def _offset_sets(B, H, W, off_ld, g):
    return dict(edge=R.edge_offsets(B, H, W, off_ld), quarter=R.quarter_offsets(B, H, W, off_ld, g),
                integer=R.quarter_offsets(B, H, W, off_ld, g, integer=True))


@pytest.mark.parametrize("hw", DEFORM_HW)
def test_offset_generators_do_what_they_say(hw):
    H, W = hw
    B = 2
    for off_ld in (18, 27):
        sets = _offset_sets(B, H, W, off_ld, R.gen(H, W, off_ld))
        for name, off in sets.items():
            o = off[..., :18]
            assert float(o.abs().max()) <= 3 and torch.equal(o * 4, (o * 4).round()), name
            assert bool((off[..., 18:] == 1000.0).all())
        assert torch.equal(sets["integer"][..., :18], sets["integer"][..., :18].round())
        hf, wf = R.sample_positions(sets["edge"], H, W)
        for pos, size, axis in ((hf, H, 0), (wf, W, 1)):
            targets = set(R.edge_targets(size))
            assert set(pos.unique().tolist()) <= targets                         # every hand-placed position is a target
            for cls in range(3):
                sel = torch.tensor([[R.pixel_class(h, w, H, W) == cls for w in range(W)] for h in range(H)])
                if not bool(sel.any()):
                    continue                                                     # (a 1 x 1 map has a corner pixel only)
                hit = set(pos[:, sel].unique().tolist())
                bases = {(h if axis == 0 else w) - 1 + k for h in range(H) for w in range(W) if sel[h, w] for k in range(3)}
                reachable = {t for t in targets if any(abs(t - b) <= 3 for b in bases)}
                assert hit == reachable, (cls, axis, sorted(reachable - hit))
                assert reachable == targets                                      # offsets of [-3, 3] reach all eight
        # an outside row meets inside columns and the reverse: the boundary of each axis decides alone somewhere
        row_out, col_out = (hf <= -1) | (hf >= H), (wf <= -1) | (wf >= W)
        assert bool((row_out & ~col_out).any()) and bool((col_out & ~row_out).any()) and bool((~row_out & ~col_out).any())


def _grid_sample_cols(x, off, groups):
    """the same samples through F.grid_sample (bilinear, zero padding, align_corners=True: pixel-centre coordinates)"""
    B, H, W, C = x.shape
    hf, wf = R.sample_positions(off, H, W)                                       # [B, H, W, 9]
    grid = torch.stack([2 * wf / (W - 1) - 1, 2 * hf / (H - 1) - 1], -1).reshape(B, H, W * 9, 2)
    s = F.grid_sample(nchw(x).double(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    s = s.reshape(B, groups, C // groups, H, W, 9)
    return s.permute(0, 3, 4, 1, 5, 2)


@pytest.mark.parametrize("hw", DEFORM_HW)
def test_deform_cols_is_torch_and_exact_on_the_quarter_grid(hw):
    H, W = hw
    B = 2
    for cpg in (4, 8, 32, 40):
        for groups in (1, 4):
            C = cpg * groups
            g = R.gen(H, W, cpg, groups)
            x = R.ints((B, H, W, C), g)
            weight = R.ints((2 * groups, cpg, 3, 3), g, -2, 2)
            # zero offsets: the plain grouped convolution
            zero = torch.zeros(B, H, W, 18)
            want = F.conv2d(nchw(x).double(), weight.double(), None, 1, 1, 1, groups)
            assert torch.equal(nchw(R.deform_conv(x, zero, weight, groups)), want)
            for off_ld in (18, 27):
                for name, off in _offset_sets(B, H, W, off_ld, g).items():
                    col = R.deform_cols(x, off, groups)
                    assert tuple(col.shape) == (B, H, W, groups, 9, cpg)
                    if H > 1 and W > 1:
                        # grid_sample normalises the coordinates (a rounding): equal to 1e-12, not bitwise; positions
                        # exactly on -1 or on the size are zero in both
                        assert float((col - _grid_sample_cols(x, off, groups)).abs().max()) <= 1e-12, name
                    # weights are multiples of 1/16, x integers of magnitude <= 3: each sample a 6-bit value, exact in f32, bf16
                    assert torch.equal(col * 16, (col * 16).round()) and float(col.abs().max()) <= 3 and R.is_bf16(col)
                    hf, wf = R.sample_positions(off, H, W)
                    outside = ~((hf > -1) & (wf > -1) & (hf < H) & (wf < W))[:, :, :, None, :, None].expand_as(col)
                    assert bool((col[outside] == 0).all()) and not bool(torch.signbit(col[outside]).any())
                    # the fused forward: integers of 1/16 below 2^24 / 16 in magnitude: exact in f32 in any order
                    S = R.deform_conv(x, off, weight, groups, magnitude=True)
                    assert float(S.max()) * 16 < 2 ** 24 and R.is_f32(R.deform_conv(x, off, weight, groups))
                    assert bool((S >= R.deform_conv(x, off, weight, groups).abs()).all())


# ------------------------------------------------------------------------------------------------------ head final conv
@pytest.mark.parametrize("hw", [(1, 1), (15, 31), (17, 33)])
def test_head_final_conv_is_torch_and_exact_on_integers(hw):
    H, W = hw
    for hc in (16, 64):
        for widths in HEAD_WIDTHS:
            g = R.gen(H, W, hc, len(widths), 2)
            for exact in (True, False):
                hidden, ws, bs = R.head_case(H, W, hc, widths, 2, exact, g)
                want = torch.cat([F.conv2d(nchw(hidden[i]).double(), ws[i].double(), bs[i].double(), 1, 1)
                                  for i in range(len(widths)) if widths[i]], 1)
                got = R.head_final_conv(hidden, ws, bs)
                assert tuple(got.shape) == (2, sum(widths), H, W)
                S = R.head_final_conv(hidden, ws, bs, magnitude=True)
                assert bool((S >= got.abs()).all())
                if exact:
                    assert torch.equal(got, want) and float(S.max()) < 2 ** 24    # integers below 2^24: exact in f32, any order
                else:
                    assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


def test_head_branch_map_helper_refuses_a_fifth_output():
    from sgv3d_amd import hip_ops
    for widths in HEAD_WIDTHS:
        m = hip_ops.head_branch_of_out(widths).tolist()
        assert m == sorted(m) and [m.count(i) for i in range(len(widths))] == widths
    with pytest.raises(ValueError):
        hip_ops.head_branch_of_out([2, 5, 1])
