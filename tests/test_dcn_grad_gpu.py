"""Differentiable one-launch deformable 3x3 convolution of the mixed-precision training step on the MI355X:
``misc_grad.deform_conv3x3`` (forward csrc/dcn_fused_bf16.hip, weight gradient with the samples recomputed csrc/dcn_grad.hip,
sampling adjoint in gather form in every mode) against the float64 restatement of tests/dcn_grad_ref.py, the column tensor
``hip_ops.deform_im2col3x3`` writes, and the column form of ``train_forward.deform_conv`` it replaces.

Yardsticks for dW.  (1) Data on which every f32 summation order gives the same bits: equality with float64.  (2) Random data: the
float64 product of the ROUNDED operands (column tensor as the im2col kernel writes it, rounded to bf16; dy rounded to bf16), which
leaves the additions only: the products are exact in f32, n - 1 correctly rounded additions in any order err by at most
(n - 1) 2^-24 sum|terms|, a factor 2 covers an adder inside the matrix core that truncates (its rounding is not documented), and the
sum has P terms plus one addition per pixel range: |got - ref| <= (P + split) 2^-23 sum_p |dy_p s_p| per element.  (3) One term per
output: the sample's bits themselves."""
import contextlib

import pytest
import torch

import dcn_grad_ref as R
from sgv3d_amd import _lib, conv_grad, grad_slots, hip_ops, misc_grad

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, C, H, W, groups, cout): pixel counts 198, 91, 75 (none a multiple of the 32-pixel step; the last has opg = 132 > 128 and
# cpg = 32 < 128) and 1440 (several steps per range)
SMALL = [(2, 128, 9, 11, 4, 128), (1, 256, 13, 7, 2, 96), (3, 64, 5, 5, 2, 264)]
MID = (2, 128, 24, 30, 4, 128)
FULL = (1, 512, 54, 96, 4, 512)
SHAPES = SMALL + [MID]
ids = lambda s: "x".join(str(v) for v in s)


@pytest.fixture
def bf16_mode():
    """The mode of tools/train_bench.py --dtype bf16: f32 tensors, bf16 operands."""
    names = ("MFMA_BF16", "MFMA_F32X3", "BF16_ACTIVATIONS", "DCN_FUSED", "DCN_FUSED_BF16", "TRAIN_BF16_WGRAD", "DETERMINISTIC")
    old = [getattr(hip_ops, n) for n in names]
    hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3, hip_ops.BF16_ACTIVATIONS = True, False, False
    hip_ops.DCN_FUSED = hip_ops.DCN_FUSED_BF16 = hip_ops.TRAIN_BF16_WGRAD = True
    hip_ops.DETERMINISTIC = False
    yield
    for n, v in zip(names, old):
        setattr(hip_ops, n, v)


@contextlib.contextmanager
def deterministic(on=True):
    saved = hip_ops.DETERMINISTIC
    hip_ops.DETERMINISTIC = on
    try:
        yield
    finally:
        hip_ops.DETERMINISTIC = saved


@contextlib.contextmanager
def profiled():
    saved = hip_ops.PROFILE
    hip_ops.PROFILE = rec = []
    try:
        yield rec
    finally:
        hip_ops.PROFILE = saved


def labels(rec):
    return {r[0].split('|')[0] for r in rec}


def far_offsets(off):
    off[0, 0, 0] += 40.0                                         # far outside the image: zeros
    off[-1, -1, -1] -= 40.0
    return off


def integer_case(shape, seed=11):
    B, C, H, W, g, cout = shape
    gen = torch.Generator().manual_seed(seed + C)
    x = torch.randint(-4, 5, (B, H, W, C), generator=gen).float()
    dy = torch.randint(-3, 4, (B, H, W, cout), generator=gen).float()
    off = far_offsets((2 * torch.randint(-5, 5, (B, H, W, 18), generator=gen).float() + 1) / 4)     # odd multiples of 1/4 in [-2.25, 2.25]
    return x.to(DEV), off.to(DEV), dy.to(DEV)


_RANDOM = {}


def random_case(shape):
    """(x, offset, dy, weight) on the device and the column tensor the im2col kernel writes; made once per shape, never modified."""
    if shape not in _RANDOM:
        B, C, H, W, g, cout = shape
        gen = torch.Generator().manual_seed(50 + C + H)
        x = torch.randn(B, H, W, C, generator=gen).to(DEV)
        off = far_offsets(torch.randn(B, H, W, 18, generator=gen) * 2.5).to(DEV)
        dy = torch.randn(B, H, W, cout, generator=gen).to(DEV)
        w = (torch.randn(cout, C // g, 3, 3, generator=gen) / (9 * C // g) ** 0.5).to(DEV)
        col = hip_ops.deform_im2col3x3(x, off, g)
        _RANDOM[shape] = (x, off, dy, w, col)
    return _RANDOM[shape]


def effective_split(shape, split):
    B, C, H, W, g, cout = shape
    n = int(_lib.load().sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes(B, H, W, C, g, cout // g, split))
    assert n > 0 and n % (9 * cout * (C // g) * 4) == 0
    return n // (9 * cout * (C // g) * 4)


def column_form_dw(col, dy, groups):
    """The weight gradient the column form computes: conv2d_backward_weight_bf16 of the four 1x1 convolutions over the column tensor."""
    B, H, W, K = col.shape
    cout = int(dy.shape[-1])
    k9, opg = K // groups, cout // groups
    outs = []
    for gi in range(groups):
        cg = col[..., gi * k9:(gi + 1) * k9].contiguous()
        dg = dy[..., gi * opg:(gi + 1) * opg].contiguous()
        d = conv_grad.conv2d_backward_weight_bf16(cg, dg, 1)                           # [opg, 9 cpg, 1, 1], k = tap * cpg + ci
        outs.append(d.reshape(opg, 9, k9 // 9).permute(0, 2, 1))
    return torch.cat(outs, 0).reshape(cout, k9 // 9, 3, 3)


# ------------------------------------------------------------------------------------------------ 1. exact on integers
@pytest.mark.parametrize("split", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_weight_gradient_exact_on_integer_data(bf16_mode, shape, split):
    """x integers in [-4, 4], dy integers in [-3, 3], offsets odd multiples of 1/4 (+40 / -40 at two corner pixels): every sample
    is a multiple of 1/16 of magnitude <= 4 (exact in bf16) and any partial sum over <= 1440 pixels stays below 2^24 / 16, so every
    summation order and every split gives the float64 result: zero tolerance."""
    B, C, H, W, g, cout = shape
    x, off, dy = integer_case(shape)
    col = R.column_tensor(x, off, g)
    assert torch.equal(col, R.bf16_round(col)) and float(col.abs().max()) <= 4
    want, _ = R.dw_from_col(col, dy, g)
    got = misc_grad.deform_conv3x3_backward_weight(x, off, dy, g, split=split)
    assert got.shape == (cout, C // g, 3, 3) and got.dtype == torch.float32
    assert float(want.abs().max()) > 0 and torch.equal(got.double(), want)


# ------------------------------------------------------------------------------------------------ 2. random data, a-priori bound
@pytest.mark.parametrize("shape", SHAPES + [FULL], ids=ids)
def test_weight_gradient_random_data_within_the_summation_bound(bf16_mode, shape):
    B, C, H, W, g, cout = shape
    P = B * H * W
    if shape == FULL:
        gen = torch.Generator().manual_seed(3)
        x = torch.randn(B, H, W, C, generator=gen).to(DEV)
        off = far_offsets(torch.randn(B, H, W, 18, generator=gen) * 2.5).to(DEV)
        dy = torch.randn(B, H, W, cout, generator=gen).to(DEV)
        col = hip_ops.deform_im2col3x3(x, off, g)
    else:
        x, off, dy, _, col = random_case(shape)
    ref, mag = R.dw_from_col(col, dy, g, rounded=True)                                   # float64 on the device
    split = effective_split(shape, 0)
    bound = (P + split) * 2.0 ** -23 * mag
    got = misc_grad.deform_conv3x3_backward_weight(x, off, dy, g)
    with deterministic():                                                                # (no first-call timing of the old kernel)
        old = column_form_dw(col, dy, g)
    tiny = torch.finfo(torch.float64).tiny
    r_new = float(((got.double() - ref).abs() / (bound + tiny)).max())
    r_old = float(((old.double() - ref).abs() / (bound + tiny)).max())
    print(f"{ids(shape)}: P {P}, split {split}: worst |dW - float64 of the rounded operands| / bound: recomputing kernel {r_new:.2e}, "
          f"column form {r_old:.2e}; bound at most {float(bound.max()):.2e} of |dW| max {float(ref.abs().max()):.2e}")
    assert r_new <= 1.0 and r_old <= 1.0, (r_new, r_old)


# ------------------------------------------------------------------------------------------------ 3. one term per output
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_one_term_per_output_gives_the_sample_bits(bf16_mode, shape, split):
    """dy = 1 at (pixel p_i, channel co_i) for distinct channels of ONE group and 0 elsewhere: dW[co_i] is bf16(col[p_i]) bit for
    bit, every other row (other groups included) exactly 0 -- the sample bits, the pixel indexing and the range edges."""
    B, C, H, W, g, cout = shape
    P, cpg, opg = B * H * W, C // g, cout // g
    x, off, _, _, col = random_case(shape)
    grp = g - 1
    pix = sorted({0, 63, 64, 65, P - 1, 31, 32, 33, P // 3, P // 2, P - 2, min(P - 1, 96), min(P - 1, 127)})[:opg]
    cos = [(7 * i + 3) % opg for i in range(len(pix))]
    assert len(set(cos)) == len(cos)
    dy = torch.zeros(P, cout, device=DEV)
    for p, co in zip(pix, cos):
        dy[p, grp * opg + co] = 1.0
    got = misc_grad.deform_conv3x3_backward_weight(x, off, dy.reshape(B, H, W, cout), g, split=split)
    want = torch.zeros(cout, cpg, 3, 3, device=DEV)
    c = col.reshape(P, g, 9, cpg).bfloat16().float()
    for p, co in zip(pix, cos):
        want[grp * opg + co] = c[p, grp].t().reshape(cpg, 3, 3)
    assert float(want.abs().max()) > 0
    want = want + 0.0                                                                    # (a sample that is -0 sums to +0)
    live = torch.zeros(cout, dtype=torch.bool, device=DEV)
    live[[grp * opg + co for co in cos]] = True
    assert torch.equal(got[live].view(torch.int32), want[live].view(torch.int32))        # bitwise
    assert (got[~live] == 0).all()


# ------------------------------------------------------------------------------------------------ 4. overwrite, guard band, repeatability
def test_overwrite_guard_band_repeat_and_short_workspace(bf16_mode):
    shape = SMALL[2]
    B, C, H, W, g, cout = shape
    x, off, dy, _, _ = random_case(shape)
    lib = _lib.load()
    n = cout * (C // g) * 9
    nws = int(lib.sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes(B, H, W, C, g, cout // g, 0))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    st = _lib.stream_handle(torch.device(DEV))

    def run(buf, nbytes=nws):
        return lib.sgv3d_deform_conv3x3_backward_weight_bf16(B, H, W, C, g, cout // g, x.data_ptr(), off.data_ptr(), 18, dy.data_ptr(),
                                                             buf.data_ptr(), 0, ws.data_ptr(), nbytes, st)
    a = torch.full((n + 64,), 7.0, device=DEV)
    assert run(a) == 0
    b = torch.full((n + 64,), -3.0, device=DEV)
    assert run(b) == 0
    torch.cuda.synchronize()
    assert (a[n:] == 7.0).all() and (b[n:] == -3.0).all()                                # guard untouched
    assert torch.equal(a[:n].view(torch.int32), b[:n].view(torch.int32))                 # overwritten, not accumulated; same bits
    ref, _ = R.dw_from_col(hip_ops.deform_im2col3x3(x, off, g), dy, g, rounded=True)
    assert float((a[:n].double() - ref.reshape(-1)).abs().max()) <= 1e-4 * float(ref.abs().max())
    c = torch.full((n + 64,), 7.0, device=DEV)
    assert run(c, nws - 1) == -3 and b"workspace too small" in lib.sgv3d_last_error()     # SGV3D_ENOSPACE
    torch.cuda.synchronize()
    assert (c == 7.0).all()


# ------------------------------------------------------------------------------------------------ 5. the op against the column form
def column_form(x, offset, weight, g):
    """The lines of train_forward.deform_conv the new operator replaces."""
    cout, cpg = int(weight.shape[0]), int(weight.shape[1])
    opg = cout // g
    col = misc_grad.deform_im2col3x3(x, offset, g)
    outs = []
    for gi in range(g):
        wg = weight[gi * opg:(gi + 1) * opg].permute(0, 2, 3, 1).reshape(opg, 9 * cpg, 1, 1)
        outs.append(conv_grad.conv2d(col[..., gi * 9 * cpg:(gi + 1) * 9 * cpg].contiguous(), wg))
    return torch.cat(outs, -1)


def grads(fn, x, off, w, dy, need=(True, True, True)):
    leaves = [t.detach().clone().requires_grad_(n) for t, n in zip((x, off, w), need)]
    y = fn(*leaves)
    y.backward(dy)
    torch.cuda.synchronize()
    return (y.detach(),) + tuple(t.grad for t in leaves)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_operator_against_the_column_form(bf16_mode, shape):
    B, C, H, W, g, cout = shape
    P = B * H * W
    x, off, dy, w, col = random_case(shape)
    with deterministic():                         # the column form's gather adjoint; fixed tile rules for both forms
        y0, dx0, do0, dw0 = grads(lambda a, b, c: column_form(a, b, c, g), x, off, w, dy)
        y1, dx1, do1, dw1 = grads(lambda a, b, c: misc_grad.deform_conv3x3(a, b, c, g), x, off, w, dy)
    assert torch.equal(y1, hip_ops.deform_conv3x3_bf16(x, off, hip_ops.PackedDeformBf16(w, g), out_dtype=torch.float32))
    assert float((y1 - y0).abs().max()) <= 4e-5 * float(y0.abs().max())                  # the two forwards: summation order only
    assert torch.equal(dx1, dx0) and torch.equal(do1, do0)                               # the same kernels on the same inputs
    ref, mag = R.dw_from_col(col, dy, g, rounded=True)
    bound = (P + effective_split(shape, 0)) * 2.0 ** -23 * mag
    assert ((dw1.double() - ref).abs() <= bound).all()
    assert float((dw1 - dw0).abs().max()) <= 2 * float(bound.max())
    # mode off: no float atomics anywhere in the new operator
    a = grads(lambda a, b, c: misc_grad.deform_conv3x3(a, b, c, g), x, off, w, dy)
    b = grads(lambda a, b, c: misc_grad.deform_conv3x3(a, b, c, g), x, off, w, dy)
    assert not hip_ops.deterministic() and all(torch.equal(p, q) for p, q in zip(a, b))
    # against float64 of the unrounded operands: bf16 operand rounding, 2e-2 of the gradient's scale
    f64, _ = R.dw_from_col(R.column_tensor(x, off, g), dy, g)
    assert float((dw1.double() - f64).abs().max()) <= 2e-2 * float(f64.abs().max())


# ------------------------------------------------------------------------------------------------ 6. autograd contract
def test_autograd_contract(bf16_mode):
    shape = SMALL[0]
    B, C, H, W, g, cout = shape
    x, off, dy, w, _ = random_case(shape)
    op = lambda a, b, c: misc_grad.deform_conv3x3(a, b, c, g)
    y, dx, do, dw = grads(op, x, off, w, dy)
    # the weight gradient lands in the claimed slot when one is armed
    wp = w.detach().clone().requires_grad_(True)
    flat = torch.full((wp.numel() + 16,), 5.0, device=DEV)
    grad_slots.register(wp.data_ptr(), flat, 8, wp.numel(), wp.shape)
    try:
        assert grad_slots.claim(wp) is None                                              # not armed yet (and now known as capable)
        grad_slots.arm(wp.data_ptr())
        misc_grad.deform_conv3x3(x, off, wp, g).backward(dy)
        torch.cuda.synchronize()
        assert wp.grad.data_ptr() == flat.data_ptr() + 32
        assert torch.equal(flat[8:8 + wp.numel()].view(wp.shape), dw) and (flat[:8] == 5.0).all() and (flat[8 + wp.numel():] == 5.0).all()
    finally:
        grad_slots.unregister(wp.data_ptr())
    # needs_input_grad: only the work asked for
    for need, absent in (((True, False, False), "dcn_wgrad_bf16"), ((False, True, False), "dcn_wgrad_bf16"),
                         ((False, False, True), "deform_im2col3x3_backward_det")):
        with profiled() as rec:
            out = grads(op, x, off, w, dy, need)
        seen = labels(rec)
        assert absent not in seen and "conv_dcn_fused_bf16" in seen and "deform_im2col3x3" not in seen, (need, sorted(seen))
        assert ("dcn_wgrad_bf16" in seen) == need[2] and ("deform_im2col3x3_backward_det" in seen) == (need[0] or need[1])
        for got, want, n in zip(out[1:], (dx, do, dw), need):
            assert (got is None) if not n else torch.equal(got, want)
    # non-contiguous inputs and gradient
    xn = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    wide = torch.zeros(B, H, W, 20, device=DEV)
    wide[..., :18] = off
    dyn = dy.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not xn.is_contiguous() and not dyn.is_contiguous() and not wide[..., :18].is_contiguous()
    yn, dxn, don, dwn = grads(op, xn, wide[..., :18], w, dyn)
    assert torch.equal(yn, y) and torch.equal(dxn, dx) and torch.equal(don, do) and torch.equal(dwn, dw)
    # an uncovered shape: an error, no fallback
    assert misc_grad.deform_conv3x3_covers(C, g, cout) and not misc_grad.deform_conv3x3_covers(64, 4, 64)
    with pytest.raises(_lib.SGV3DError):
        misc_grad.deform_conv3x3(torch.zeros(1, 5, 5, 64, device=DEV), torch.zeros(1, 5, 5, 18, device=DEV), torch.zeros(64, 16, 3, 3, device=DEV), 4)
    with pytest.raises(_lib.SGV3DError):
        misc_grad.deform_conv3x3(x, off[..., :16], w, g)


# ------------------------------------------------------------------------------------------------ 7. no tensor of the column size
def test_no_tensor_of_the_column_size(bf16_mode):
    B, C, H, W, g, cout = MID
    L = 4 * B * H * W * 9 * C                                                            # 6.6 MB
    x, off, dy, w, _ = random_case(MID)

    def retained(fn):
        xs, os_, ws = (t.detach().clone().requires_grad_(True) for t in (x, off, w))
        torch.cuda.synchronize()
        start = torch.cuda.memory_allocated()
        y = fn(xs, os_, ws)
        torch.cuda.synchronize()
        kept = torch.cuda.memory_allocated() - start - y.numel() * 4
        y.backward(dy)
        torch.cuda.synchronize()
        assert xs.grad is not None and os_.grad is not None and ws.grad is not None
        return kept

    new = retained(lambda a, b, c: misc_grad.deform_conv3x3(a, b, c, g))
    old = retained(lambda a, b, c: column_form(a, b, c, g))
    print(f"kept between forward and backward beyond the output: new operator {new / 1e6:.2f} MB, column form {old / 1e6:.2f} MB, "
          f"column tensor {L / 1e6:.2f} MB")
    assert new < L / 4, (new, L)
    assert old > L, (old, L)


# ------------------------------------------------------------------------------------------------ 8. model level
@contextlib.contextmanager
def fused_train(on):
    saved = hip_ops.DCN_FUSED_TRAIN
    hip_ops.DCN_FUSED_TRAIN = on
    try:
        yield
    finally:
        hip_ops.DCN_FUSED_TRAIN = saved


def test_model_switch_on_and_off(bf16_mode):
    """Small LSS model, batch 2, Dropout 0, bf16 mode, deterministic mode in both runs: the profile shows which form ran; predictions,
    loss and every parameter gradient agree to the bars test_centerhead_branches_as_one_wide_map_match_the_per_branch_form uses for
    'float32 summation order'.

    Both runs take the library's fixed tile / split-K rules (hip_ops.AUTOTUNE off): the deterministic mode applies a choice that an
    EARLIER test of the same process measured and left in hip_ops.TUNE_DB, so without the pin the result depends on what ran before.
    Measured on the MI355X: under the rules the two forms agree bit for bit (loss 146.589310 both ways, every map and every gradient
    tensor equal: at the small model's 192 pixels the two forwards and the two weight gradients sum in the same order).  Behind the
    other GPU tests of the training side, with recorded split-K choices in the column form's GEMMs only, the same two runs gave loss
    146.700500 / 146.710129 (6.6e-5 relative), prediction maps within 9.1e-3, gradient tensors median 5.4e-2, worst 4.0e-1
    (head.trunk.layer3.0.downsample.0.weight): the batch-statistics BatchNorms of this small model amplify a change of f32
    summation order that far -- ONE form moves by 8e-4 in the loss between the two states (146.5893 / 146.7101)."""
    from test_lift_splat_grad_gpu import _train_once
    saved = hip_ops.AUTOTUNE
    hip_ops.AUTOTUNE = False
    try:
        with fused_train(True):
            k1, maps1, loss1, g1 = _train_once(False, True)
        with fused_train(False):
            k0, maps0, loss0, g0 = _train_once(False, True)
    finally:
        hip_ops.AUTOTUNE = saved
    assert {"conv_dcn_fused_bf16", "dcn_wgrad_bf16", "deform_im2col3x3_backward_det"} <= k1 and "deform_im2col3x3" not in k1, sorted(k1)
    assert {"deform_im2col3x3", "deform_im2col3x3_backward_det"} <= k0 and "dcn_wgrad_bf16" not in k0 and "conv_dcn_fused_bf16" not in k0, sorted(k0)
    la, lb = float(loss1), float(loss0)
    pred = max(float((a - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(maps1, maps0))
    assert g1.keys() == g0.keys()
    gscale = max(float(v.abs().max()) for v in g0.values())
    rel = sorted((float((g1[n] - g0[n]).abs().max()) / max(float(g0[n].abs().max()), 1e-3 * gscale), n) for n in g0)
    print(f"fused DCN against the column form, small model: loss {la:.6f} / {lb:.6f} (relative {abs(la - lb) / abs(lb):.1e}); prediction maps "
          f"{pred:.1e}; gradient tensors median {rel[len(rel) // 2][0]:.1e}, worst {rel[-1][0]:.1e} ({rel[-1][1]})")
    assert len(maps1) == len(maps0) and pred <= 1e-4
    assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    assert rel[-1][0] <= 3e-2, rel[-1]


# ------------------------------------------------------------------------------------------------ 9. graph
def test_graphed_step_with_the_fused_dcn_replays_bitwise(bf16_mode):
    from sgv3d_amd import synthetic
    from sgv3d_amd.models.bev_height import BEVHeight
    from sgv3d_amd.train_step import DataParallelAdamW, GraphedTrainStep
    dev = torch.device(DEV)
    bconf, hconf = synthetic.small_conf()
    torch.manual_seed(0)
    model = BEVHeight(bconf, hconf).to(dev).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.head.train_cfg = dict(model.head.train_cfg, grid_size=[256, 256, 1], point_cloud_range=[0, -12.8, -5, 25.6, 12.8, 3])
    imgs = synthetic.make_images(2, final=bconf['final_dim'], device=dev, seed=0)
    mats = synthetic.make_mats(2, device=dev, scale=bconf['final_dim'][0] / 864)
    boxes, lab = synthetic.make_gt(2, seed=0, n_range=(10, 40), stress=False)
    boxes, lab = [b.to(dev) for b in boxes], [l.to(dev) for l in lab]
    opt = DataParallelAdamW(model.parameters(), lr=2e-4, max_grad_norm=5.0)

    def forward_backward():
        loss = model.loss(model.get_targets(boxes, lab), model(imgs, mats))
        loss.backward()
        return loss

    def snapshot():
        return [p.clone() for p, _, _ in opt.flat.buckets], [(m.clone(), v.clone()) for m, v in opt.state], opt.steps

    def restore(snap):
        for (p, _, _), q in zip(opt.flat.buckets, snap[0]):
            p.copy_(q)
        for (m, v), (m0, v0) in zip(opt.state, snap[1]):
            m.copy_(m0); v.copy_(v0)
        opt.steps = snap[2]

    with fused_train(True), profiled() as rec:
        for _ in range(2):
            opt.zero_grad()
            forward_backward()
            opt.step()
        assert {"conv_dcn_fused_bf16", "dcn_wgrad_bf16"} <= labels(rec) and "deform_im2col3x3" not in labels(rec)
    with fused_train(True):
        snap = snapshot()
        graphed = GraphedTrainStep(forward_backward, opt, warmup=0, strict=True)
        assert graphed.graph is not None
        outs = []
        for _ in range(2):
            restore(snap)
            loss = float(graphed().detach())
            torch.cuda.synchronize()
            outs.append((loss, torch.cat([p for p, _, _ in opt.flat.buckets]).clone()))
    assert outs[0][0] == outs[1][0] and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][1], torch.cat(snap[0]))
