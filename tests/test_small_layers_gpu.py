"""The small inference layers of csrc/misc_layers.hip and their bf16 twins of csrc/act_bf16.hip on the MI355X against the
float64 restatements of tests/small_layers_ref.py, at ragged shapes: one-pixel maps, one row, one column, channel counts off
the vector width and off 64, more than one workgroup, slices of wider buffers.

Every comparison is either exact equality (max, copies, one-rounding products, and integer / quarter-pixel inputs for which
every intermediate is an f32 and a bf16 value -- tests/test_small_layers_cpu.py proves that of the reference) or the
worst-case bound of an f32 evaluation

    |got - want| <= (n + 2) 2^-24 S        (_within, the form of tests/test_misc_grad_gpu.py)

with S the same computation on absolute values in float64 and n the roundings on the kernel's longest path, derived next
to each use.  A bf16 twin computes in f32 and rounds once on the store, so its result is the reference rounded once to bf16
unless the f32 bar straddles a rounding boundary: round(want - E) <= got <= round(want + E) with E the f32 bar
(_within_bf16; for exact inputs plain equality with the rounded reference).

Inputs sit in front of a NaN tail and outputs in front of a sentinel tail: a read or write past the tensor shows.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_layers_ref as R
from sgv3d_amd import _lib, hip_ops
from sgv3d_amd._lib import SGV3DError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SENT = -1024.0                         # a bf16 value no case produces
TAIL = 4096
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
SGV3D_ENOSPACE = -3


@pytest.fixture
def bf16_mode():
    """The compute-mode switch of the other bf16 files.  The kernels here are chosen by the tensors' dtype; the fused DCN
    forward of section 9 is the f32-mode launch and runs with the switch as the process has it."""
    old = hip_ops.MFMA_BF16
    hip_ops.MFMA_BF16 = True
    yield
    hip_ops.MFMA_BF16 = old


@pytest.fixture(autouse=True)
def _twin_mode(request):
    """a bf16 twin is tested in the mode it runs in"""
    spec = getattr(request.node, "callspec", None)
    if spec is not None and spec.params.get("dtype") == BF16:
        request.getfixturevalue("bf16_mode")
    yield


def _st():
    return _lib.stream_handle(torch.device(DEV))


def _bar(S, n, eta=0.0):
    return (n + 2) * U * S + eta


def _within(got, want, S, n, eta=0.0):
    """per element |got - want| <= (n + 2) 2^-24 S (+ eta, an absolute term where f32 underflows)"""
    err = (got.double().cpu() - want).abs()
    bar = _bar(S, n, eta)
    bad = ~(err <= bar)
    assert not bool(bad.any()), (int(bad.sum()), float(err[bad].max()), float((err - bar)[bad].max()))


def _within_bf16(got, want, S, n, eta=0.0):
    """the f32 value lies within the bar of ``want`` and is rounded once: round(want - E) <= got <= round(want + E)"""
    g = got.double().cpu()
    E = _bar(S, n, eta)
    bad = ~((g >= R.round_bf16(want - E)) & (g <= R.round_bf16(want + E)))
    assert not bool(bad.any()), (int(bad.sum()), float((g - want).abs()[bad].max()))


def _close(got, want, S, n, dtype, eta=0.0):
    (_within_bf16 if dtype == BF16 else _within)(got, want, S, n, eta)


def _rounded(want, dtype):
    """the float64 reference rounded once to the kernel's output type"""
    return R.round_bf16(want) if dtype == BF16 else want.float().double()


def _equal_nan(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def _dev(t, dtype=F32):
    """``t`` on the device in front of a NaN tail"""
    n = t.numel()
    big = torch.full((n + TAIL,), math.nan, dtype=dtype, device=DEV)
    big[:n] = t.reshape(-1).to(DEV, dtype)
    return big[:n].view(t.shape)


class _Out:
    """a sentinel-filled output of ``shape`` in front of a sentinel tail"""

    def __init__(self, shape, dtype=F32):
        n = math.prod(shape)
        self.big = torch.full((n + TAIL,), SENT, dtype=dtype, device=DEV)
        self.t = self.big[:n].view(shape)
        self.n = n

    def tail_intact(self):
        return bool((self.big[self.n:] == SENT).all())


# ------------------------------------------------------------------------------------------------------ 1. max pooling
MAXPOOL_HW = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 8), (8, 3), (7, 10), (4, 6)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", MAXPOOL_HW)
def test_maxpool(hip, hw, dtype):
    """== F.max_pool2d(x, 3, 2, 1) bit for bit, NaN windows included, two images with different data; the (4, 6) map is there
    for the NaN in the clipped last window of an even-sized map (as is (2, 2))."""
    H, W = hw
    for C in ((4, 8, 72) if dtype == F32 else (8, 72)):
        variants = [R.randn_bf16((2, H, W, C), R.gen(H, W, C))]
        if (H, W) == (7, 10):
            variants.append(R.nan_windows(variants[0].clone()))
        if H % 2 == 0 and W % 2 == 0:
            variants.append(R.nan_clipped_corner(variants[0].clone()))
        for x in variants:
            out = _Out((2, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype)
            hip_ops.maxpool3x3s2(_dev(x, dtype), out=out.t)
            got = out.t.double().cpu()
            assert _equal_nan(got, R.maxpool3x3s2(x))
            assert _equal_nan(got.permute(0, 3, 1, 2), F.max_pool2d(x.permute(0, 3, 1, 2).double(), 3, 2, 1))
            assert out.tail_intact()


# ------------------------------------------------------------------------------------------------------------ 2. layouts
@pytest.mark.parametrize("hw", [(1, 1), (15, 17), (1, 257)])           # HW = 1, 255, 257: below / above one 256-thread block
def test_nchw_to_nhwc(hip, hw):
    H, W = hw
    for C, c_pad in ((3, 4), (5, 8), (8, 8)):
        x = torch.randn(2, C, H, W, generator=R.gen(H, W, C))
        out = _Out((2, H, W, c_pad))
        hip_ops.nchw_to_nhwc(_dev(x), c_pad=c_pad, out=out.t)
        y = out.t.cpu()
        assert torch.equal(y[..., :C], x.permute(0, 2, 3, 1)) and bool((y[..., C:] == 0).all()) and out.tail_intact()


@pytest.mark.parametrize("hw", [(1, 1), (1, 31), (3, 11)])             # HW = 1, 31, 33: around the 32-pixel transpose tile
def test_nhwc_to_nchw(hip, hw):
    H, W = hw
    for C in (1, 32, 33, 87):
        coff, ld = 3, 3 + C + 5
        x = torch.randn(2, H, W, ld, generator=R.gen(H, W, C))
        out = _Out((2, C, H, W))
        hip_ops.nhwc_to_nchw(_dev(x), channels=C, coff=coff, out=out.t)
        assert torch.equal(out.t.cpu(), x[..., coff:coff + C].permute(0, 3, 1, 2)) and out.tail_intact()


@pytest.mark.parametrize("pixels", [1, 257])
def test_copy_channels(hip, pixels):
    for C in (1, 7, 80):
        for coff in (0, 5):
            ld = coff + C + 3
            x = torch.randn(2, 1, pixels, ld, generator=R.gen(pixels, C, coff))
            out = _Out((2, 1, pixels, C))
            hip_ops.copy_channels(_dev(x), out.t, coff=coff)
            assert torch.equal(out.t.cpu(), x[..., coff:coff + C]) and out.tail_intact()


# ------------------------------------------------------------------------------------------------- 3. global average pool
def _pool_chain(P):
    """roundings on the longest path of global_avgpool (the derivation of tests/test_misc_grad_gpu.py): a workgroup sums
    per = ceil(P / 32) pixels, each of its 4 lane groups every fourth of them (ceil(per / 4) adds), two levels of pair sums,
    the 32 chunk partials added in order, the division by P."""
    return math.ceil(math.ceil(P / 32) / 4) + 2 + 32 + 1


def _avgpool_raw(lib, x, B, P, C, ld, ws=None, nbytes=None):
    fn = lib.sgv3d_global_avgpool_bf16 if x.dtype == BF16 else lib.sgv3d_global_avgpool
    need = lib.sgv3d_global_avgpool_workspace_bytes(B, C)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV) if ws is None else ws
    out = _Out((B, C))
    rc = fn(B, P, C, ld, x.data_ptr(), out.t.data_ptr(), ws.data_ptr(), need if nbytes is None else nbytes, _st())
    return rc, out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 31, 32, 33, 129])
def test_global_avgpool(hip, P, dtype):
    """The C entry with x_ld >= C (a channel slice of a wider map): mean within the bound of _pool_chain, exact on integers
    over a power-of-two pixel count, bitwise repeatable, and a workspace one byte short is refused."""
    lib, B = hip.load(), 2
    for C in (1, 64, 65, 100):
        for ld in (C, C + 12):
            g = R.gen(P, C, ld)
            for exact in (True, False):
                x = R.ints((B, P, ld), g) if exact else R.randn_bf16((B, P, ld), g)
                xd = _dev(x, dtype)
                rc, out = _avgpool_raw(lib, xd, B, P, C, ld)
                _lib.check(rc, "global_avgpool")
                want = R.global_mean(x, C)
                if exact and P & (P - 1) == 0:
                    assert torch.equal(out.t.double().cpu(), want)
                else:
                    _within(out.t, want, R.global_mean(x, C, magnitude=True), _pool_chain(P))
                assert out.tail_intact()
                rc, again = _avgpool_raw(lib, xd, B, P, C, ld)
                assert rc == 0 and torch.equal(again.t, out.t)
    need = lib.sgv3d_global_avgpool_workspace_bytes(B, C)
    rc, out = _avgpool_raw(lib, xd, B, P, C, ld, nbytes=need - 1)
    assert rc == SGV3D_ENOSPACE and bool((out.t == SENT).all())


# ------------------------------------------------------------------------------------------------------------- 4. dense
def _dense_chain(K, act):
    """dense_kernel: a lane adds ceil(K / 64) products, the butterfly adds 6 times, then scale and bias: the issue's
    n = ceil(K / 64) + 6 + 2 (the products' own roundings, if the compiler does not contract them, sit in _within's + 2).
    sigmoid: + expf, add, divide = R.SIGMOID_ROUNDINGS, with expf taken as 2 ulp (an assumption, see small_layers_ref)."""
    return math.ceil(K / 64) + 6 + 2 + (R.SIGMOID_ROUNDINGS if act == R.ACT_SIGMOID else 0)


@pytest.mark.parametrize("K", [1, 27, 63, 64, 65, 200])
def test_dense(hip, K):
    """K below, at and above one wave, B * N off a multiple of the 4 waves of a workgroup, every combination of scale, bias
    and activation; the gated entry with run = 0 leaves a sentinel-filled output alone and with run = 1 gives the same bits."""
    zero, one = torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    for N in (1, 3, 100):
        for B in (1, 3):
            g = R.gen(K, N, B)
            x, w = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
            scale, bias = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
            xd, wd, sd, bd = _dev(x), _dev(w), _dev(scale), _dev(bias)
            for s, sdev in ((None, None), (scale, sd)):
                for b, bdev in ((None, None), (bias, bd)):
                    for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_SIGMOID):
                        out = _Out((B, N))
                        hip_ops.dense(xd, wd, sdev, bdev, act, out=out.t)
                        _within(out.t, R.dense(x, w, s, b, act), R.dense(x, w, s, b, act, magnitude=True), _dense_chain(K, act))
                        assert out.tail_intact()
                        skipped = _Out((B, N))
                        hip_ops.dense(xd, wd, sdev, bdev, act, out=skipped.t, run=zero)
                        assert bool((skipped.big == SENT).all())
                        hip_ops.dense(xd, wd, sdev, bdev, act, out=skipped.t, run=one)
                        assert torch.equal(skipped.big, out.big)


# ------------------------------------------------------------------------------------------ 5. broadcast / channel gates
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(1, 1), (3, 11)])                        # P = 1, 33
def test_broadcast_and_scale_channels(hip, hw, dtype):
    """One rounding each, so exact: broadcast == the value (rounded to the map's type), into a channel slice whose
    neighbours stay as they were; scale == the float64 product rounded once.  Three images with gates of their own."""
    H, W = hw
    B = 3
    for C in ((4, 8, 72) if dtype == F32 else (8, 72)):
        g = R.gen(H, W, C)
        v = torch.randn(B, C, generator=g)
        coff, ld = 8, 8 + C + 8
        out = _Out((B, H, W, ld), dtype)
        hip_ops.broadcast_channels(_dev(v), out.t, y_coff=coff)
        y = out.t.double().cpu()
        assert torch.equal(y[..., coff:coff + C], _rounded(v.double(), dtype)[:, None, None, :].expand(B, H, W, C))
        assert bool((y[..., :coff] == SENT).all()) and bool((y[..., coff + C:] == SENT).all()) and out.tail_intact()
        # bf16 twin: gates that are bf16 values, so that the f32 product is exact and the store is the only rounding
        x = R.randn_bf16((B, H, W, C), g)
        gate = torch.rand(B, C, generator=g)
        gate = gate.bfloat16().float() if dtype == BF16 else gate
        out = _Out((B, H, W, C), dtype)
        hip_ops.scale_channels(_dev(x, dtype), _dev(gate), out=out.t)
        assert torch.equal(out.t.double().cpu(), _rounded(x.double() * gate.double()[:, None, None, :], dtype))
        assert out.tail_intact()


# ------------------------------------------------------------------------------------------------------- 6. bilinear x2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (4, 1), (2, 2), (5, 7)])
def test_upsample_bilinear2x(hip, hw, dtype):
    """f32 vector kernel (C = 4, 72), f32 scalar kernel (C = 7), bf16 twin (C = 8, 72).  Integer inputs: every weight is a
    multiple of 1/16 and the result is exact in either type.  Random inputs, n = 7: per output two inner sums of two products
    (2 roundings each on the longest path), the two outer products and the last add; the weights are exact."""
    H, W = hw
    for C in ((4, 72, 7) if dtype == F32 else (8, 72)):
        g = R.gen(H, W, C)
        for exact in (True, False):
            x = R.ints((2, H, W, C), g) if exact else R.randn_bf16((2, H, W, C), g)
            out = _Out((2, 2 * H, 2 * W, C), dtype)
            hip_ops.upsample_bilinear2x(_dev(x, dtype), out=out.t)
            want = R.bilinear2x(x)
            if exact:
                assert torch.equal(out.t.double().cpu(), want)
            else:
                _close(out.t, want, R.bilinear2x(x, magnitude=True), 7, dtype)
            assert out.tail_intact()


# --------------------------------------------------------------------------------------------------- 7. a + b sigmoid(c)
@pytest.mark.parametrize("dtype,n", [(F32, 4), (F32, 8), (F32, 1020), (F32, 1024 + 8), (BF16, 8), (BF16, 1016), (BF16, 1024 + 8)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_add_mul_sigmoid(hip, n, dtype):
    """The bf16 twin takes multiples of 8 (1016 in place of 1020).  c over [-100, 100] with +-inf, 0 and +-100 placed by hand.  n = R.SIGMOID_ROUNDINGS (expf as 2 ulp -- assumed --, add,
    divide) + the product + the sum, on S = |a| + |b| sigmoid(c); below the smallest normal f32 (expf overflows from
    c < -88.7 on, where sigmoid < 2^-126) the relative bound says nothing: + |b| 2^-126.  sigmoid(+-inf) is exactly 1 / 0."""
    if dtype == BF16 and n == 1016:
        z = torch.zeros(1020, dtype=BF16, device=DEV)
        with pytest.raises(SGV3DError):
            hip_ops.add_mul_sigmoid(z, z, z)
    g = R.gen(n)
    a, b = R.randn_bf16((n,), g), R.randn_bf16((n,), g)
    c = ((torch.rand(n, generator=g) * 200 - 100)).bfloat16().float()
    c[:4] = torch.tensor([math.inf, -math.inf, 0.0, -100.0])
    if n >= 8:
        c[4:8] = torch.tensor([100.0, -89.0, 88.0, -0.0])
    out = _Out((n,), dtype)
    hip_ops.add_mul_sigmoid(_dev(a, dtype), _dev(b, dtype), _dev(c, dtype), out=out.t)
    want = R.add_mul_sigmoid(a, b, c)
    _close(out.t, want, R.add_mul_sigmoid(a, b, c, magnitude=True), R.SIGMOID_ROUNDINGS + 2, dtype, eta=b.double().abs() * R.F32_TINY)
    got = out.t.double().cpu()
    assert torch.equal(got[:2], _rounded(torch.stack([a[0].double() + b[0].double(), a[1].double()]), dtype))
    assert out.tail_intact()


# ---------------------------------------------------------------------------------------------------------- 8. BSM compose
def _bsm_chain(sem):
    """bsm_compose_kernel, a semantic column: expf of the numerator (R.EXPF_ROUNDINGS; logit - max is exact for the cases'
    2^-10 grid), the denominator's expf terms (R.EXPF_ROUNDINGS) and its sem - 1 adds, the divide; * keep is exact."""
    return 2 * R.EXPF_ROUNDINGS + (sem - 1) + 1


def _bsm_run(buf, logits, D, ctx, sem, thr):
    B, P, ld = buf.shape
    bd = _dev(buf).view(B, 1, P, ld)
    hip_ops.bsm_compose(bd, _dev(logits).view(B, 1, P, -1), D, ctx, sem, thr)
    return bd.view(B, P, ld).cpu()


@pytest.mark.parametrize("case", R.BSM_CASES, ids=lambda c: "sem%d_ld%d_pad%d_ctx%d_px%d" % c)
def test_bsm_compose(hip, case):
    """Logit rows wider than sem (NaN behind the logits), 0 / 1 / 9 pad columns pre-filled with NaN, a last workgroup that
    is partly empty.  Depth columns bitwise untouched, pad columns exactly 0, context == x * keep exactly (a product with
    0 or 1), softmax within the bound; pixels whose float64 p0 is within 1e-6 of the threshold are not judged
    (tests/test_small_layers_cpu.py: there are none at these seeds)."""
    buf, logits, D, ctx, sem, thr = R.bsm_case(*case)
    got = _bsm_run(buf, logits, D, ctx, sem, thr)
    want, p0 = R.bsm_compose(buf, logits, D, ctx, sem, thr)
    S, _ = R.bsm_compose(buf, logits, D, ctx, sem, thr, magnitude=True)
    judged = (p0 - float(np.float32(thr))).abs() >= R.BSM_EXCLUDE
    assert float(judged.double().mean()) >= 0.99
    assert torch.equal(got[..., :D], buf[..., :D])
    assert bool((got[..., D + ctx + sem:] == 0).all())
    a, b = D, D + ctx
    assert torch.equal(got[..., a:b][judged].double(), want[..., a:b][judged])
    _within(got[..., b:b + sem][judged], want[..., b:b + sem][judged], S[..., b:b + sem][judged], _bsm_chain(sem))


@pytest.mark.parametrize("sem_ld", [2, 7])
def test_bsm_compose_exact_tie(hip, sem_ld):
    """Two equal logits: p0 == 0.5 exactly.  The mask is ``p0 > thr``: at thr = 0.5 everything is kept, at the next f32
    below 0.5 everything is zeroed."""
    D, ctx, sem, P = 3, 5, 2, 9
    g = R.gen(sem_ld, 5)
    buf = torch.randn(2, P, D + ctx + sem + 1, generator=g)
    logits = torch.full((2, P, sem_ld), math.nan)
    logits[..., :2] = R.ints((2, P, 1), g)
    kept = _bsm_run(buf, logits, D, ctx, sem, 0.5)
    assert torch.equal(kept[..., D:D + ctx], buf[..., D:D + ctx]) and bool((kept[..., D + ctx:D + ctx + 2] == 0.5).all())
    gone = _bsm_run(buf, logits, D, ctx, sem, float(np.nextafter(np.float32(0.5), np.float32(0))))
    assert bool((gone[..., D:] == 0).all()) and torch.equal(gone[..., :D], buf[..., :D])


# ------------------------------------------------------------------------------------------------- 9. deformable sampling
def _offset_sets(B, H, W, off_ld, g):
    return dict(edge=R.edge_offsets(B, H, W, off_ld), quarter=R.quarter_offsets(B, H, W, off_ld, g),
                integer=R.quarter_offsets(B, H, W, off_ld, g, integer=True))


def _outside(off, H, W):
    hf, wf = R.sample_positions(off, H, W)
    return ~((hf > -1) & (wf > -1) & (hf < H) & (wf < W))                        # [B, H, W, 9]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off_ld", [18, 27])
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (3, 4)])
def test_deform_im2col(hip, hw, off_ld, dtype):
    """Integer x and offsets on the quarter-pixel grid: every weight is a multiple of 1/16, every sample exact in f32 and in
    bf16, so the column tensor equals the float64 DCNv1 sampling bit for bit -- at sample positions placed by hand on
    -1, -0.75, -0.25, 0, size - 1, size - 0.75, size - 0.25 and size (where ``inside``, floorf and the corner predicates
    decide), on random quarter-pixel and on all-integer offsets.  A sample outside the image is +0, never -0 * x."""
    H, W = hw
    B = 2
    for cpg in ((4, 8, 40) if dtype == F32 else (8, 40)):
        for groups in (1, 4):
            C = cpg * groups
            g = R.gen(H, W, cpg, groups)
            x = R.ints((B, H, W, C), g)
            xd = _dev(x, dtype)
            for name, off in _offset_sets(B, H, W, off_ld, g).items():
                out = _Out((B, H, W, 9 * C), dtype)
                hip_ops.deform_im2col3x3(xd, _dev(off), groups, out=out.t)
                got = out.t.double().cpu().view(B, H, W, groups, 9, cpg)
                assert torch.equal(got, R.deform_cols(x, off, groups)), (name, cpg, groups)
                outside = _outside(off, H, W)[:, :, :, None, :, None].expand_as(got)
                assert not bool(torch.signbit(got[outside]).any()), (name, cpg, groups)
                assert out.tail_intact()


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (3, 4)])
def test_deform_conv_fused_exact(hip, hw):
    """sgv3d_deform_conv3x3_forward on the same offsets: it covers channels per group that are multiples of 32, so
    cpg = 32 here, groups 1 and 4.  Integer x in [-3, 3], integer weights in [-2, 2], quarter-pixel offsets: every product
    and partial sum is an integer multiple of 1/16 below 2^24 / 16 -- exact equality with the float64 DCNv1 result."""
    from sgv3d_amd.hip_ops import PackedConv, deform_conv3x3, deform_conv3x3_eligible
    H, W = hw
    B, cpg, opg = 2, 32, 8
    for groups in (1, 4):
        C, cout = cpg * groups, opg * groups
        g = R.gen(H, W, groups, 9)
        x = R.ints((B, H, W, C), g)
        weight = R.ints((cout, cpg, 3, 3), g, -2, 2)
        convs = [PackedConv(weight[i * opg:(i + 1) * opg].permute(0, 2, 3, 1).reshape(opg, 9 * cpg, 1, 1).contiguous().to(DEV))
                 for i in range(groups)]
        xd = _dev(x)
        assert deform_conv3x3_eligible(xd, convs)
        for off_ld in (18, 27):
            for name, off in _offset_sets(B, H, W, off_ld, g).items():
                out = _Out((B, H, W, cout))
                deform_conv3x3(xd, _dev(off), convs, out=out.t)
                assert torch.equal(out.t.double().cpu(), R.deform_conv(x, off, weight, groups)), (name, groups, off_ld)
                assert out.tail_intact()


# ------------------------------------------------------------------------------------------------- 10. head final conv
HEAD_WIDTHS = [[2, 1, 3, 2, 2, 1], [4, 1], [2, 0, 3]]


def _head_run(hidden, ws, bs, widths):
    nb, B, H, W, hc = hidden.shape
    wcat = torch.cat([w.permute(0, 2, 3, 1) for w in ws], 0).contiguous()
    out = _Out((B, sum(widths), H, W))
    args = (_dev(hidden), _dev(wcat), _dev(torch.cat(bs)), hip_ops.head_branch_of_out(widths, DEV), nb, hc)
    hip_ops.head_final_conv(*args, out=out.t)
    again = _Out((B, sum(widths), H, W))
    hip_ops.head_final_conv(*args, out=again.t)
    assert torch.equal(out.big, again.big)                                       # bitwise repeatable, tail included
    assert out.tail_intact()
    return out.t


@pytest.mark.parametrize("hw", [(1, 1), (15, 31), (16, 32), (17, 33), (33, 65)])
def test_head_final_conv(hip, hw):
    """One pixel, one short of / exactly / one past the 16 x 32 tile, and three tiles each way; 16 and 64 hidden channels;
    the head's own widths, a 4-wide branch (the kernel's most) and a branch without outputs in the middle.  Integer inputs
    and weights: exact.  Random: n = 9 * hc + 1, a chain of 9 * hc multiply-adds in one accumulator and the bias.  The output
    is pre-filled with a sentinel: every plane is written and nothing behind the tensor is."""
    H, W = hw
    for hc in (16, 64):
        for widths in HEAD_WIDTHS:
            for B in (1, 2):
                g = R.gen(H, W, hc, len(widths), B)
                for exact in (True, False):
                    hidden, ws, bs = R.head_case(H, W, hc, widths, B, exact, g)
                    got = _head_run(hidden, ws, bs, widths)
                    want = R.head_final_conv(hidden, ws, bs)
                    if exact:
                        assert torch.equal(got.double().cpu(), want), (hc, widths, B)
                    else:
                        _within(got, want, R.head_final_conv(hidden, ws, bs, magnitude=True), 9 * hc + 1)


def test_head_branch_wider_than_four_is_refused():
    """The kernel writes at most 4 outputs per branch and reports nothing for a fifth.  The widths are host data where the
    map is built (BEVHeightHead.hip_compile), so that is where a wider branch is refused -- no device-to-host sync on the
    frame path; the map the helper builds is ascending with contiguous branches."""
    with pytest.raises(ValueError):
        hip_ops.head_branch_of_out([2, 5, 1])
    with pytest.raises(ValueError):
        hip_ops.head_branch_of_out([0, 0])
    assert hip_ops.head_branch_of_out([2, 0, 4, 1]).tolist() == [0, 0, 2, 2, 2, 2, 3]


# ------------------------------------------------------------------------------------------ the wrappers' host-side checks
def _wrapper_calls():
    """name -> (call, good arguments); each test swaps one tensor for a permuted view / another dtype"""
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=DEV)
    return {
        "maxpool3x3s2": (lambda x: hip_ops.maxpool3x3s2(x), [z(1, 4, 4, 8)]),
        "global_avgpool": (lambda x: hip_ops.global_avgpool(x), [z(1, 4, 4, 8)]),
        "nhwc_to_nchw": (lambda x: hip_ops.nhwc_to_nchw(x), [z(1, 4, 4, 8)]),
        "copy_channels": (lambda x, o: hip_ops.copy_channels(x, o, coff=0), [z(1, 4, 4, 8), z(1, 4, 4, 8)]),
        "bsm_compose": (lambda b, l: hip_ops.bsm_compose(b, l, 2, 4, 2, 0.5), [z(1, 4, 4, 8), z(1, 4, 4, 8)]),
        "broadcast_channels": (lambda v, o: hip_ops.broadcast_channels(v, o), [z(4, 4), z(4, 2, 2, 4)]),
        "head_final_conv": (lambda h, w, b, m: hip_ops.head_final_conv(h, w, b, m, 2, 16),
                            [z(2, 1, 4, 4, 16), z(4, 3, 3, 16), z(4), z(4, dt=torch.int32)]),
    }


def _permuted(t):
    """a view of the same shape and other strides (None where the shape has no two equal dimensions > 1)"""
    dims = [i for i, s in enumerate(t.shape) if s > 1]
    for i in dims:
        for j in dims:
            if i < j and t.shape[i] == t.shape[j]:
                return t.transpose(i, j)
    return None


@pytest.mark.parametrize("name", ["maxpool3x3s2", "global_avgpool", "nhwc_to_nchw", "copy_channels", "bsm_compose",
                                  "broadcast_channels", "head_final_conv"])
def test_wrappers_refuse_views_and_other_dtypes(hip, name):
    """These wrappers hand raw pointers to the library: a permuted view or a tensor of another type must raise instead of
    giving a silently wrong frame.  Only broadcast_channels' map, max pooling and the average pool take bf16 (their twins)."""
    call, good = _wrapper_calls()[name]
    call(*good)                                                                  # the good arguments pass
    takes_bf16 = {"maxpool3x3s2": (0,), "global_avgpool": (0,), "broadcast_channels": (1,)}.get(name, ())
    for i, t in enumerate(good):
        view = _permuted(t)
        if view is not None:
            with pytest.raises(AssertionError):
                call(*[view if j == i else a for j, a in enumerate(good)])
        elif t.dim() > 1:
            raise AssertionError("no permuted view for argument %d of %s" % (i, name))
        wrong = torch.float16 if t.dtype != torch.float16 else F32
        others = [wrong] + ([] if i in takes_bf16 or t.dtype != F32 else [BF16]) + ([torch.int64] if t.dtype == torch.int32 else [])
        for dt in others:
            with pytest.raises(AssertionError):
                call(*[a.to(dt) if j == i else a for j, a in enumerate(good)])
