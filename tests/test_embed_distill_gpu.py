"""The embedding distillation on the MI355X (csrc/embed_distill.hip): the warp kernel bit for bit against the library's host twin
(which tests/test_embed_distill_cpu.py pins to the reference), loss and gradient against the float64 restatement
(tests/embed_distill_ref.py), known answers, the autograd contract, the SAM teacher call and one training step of the small
LSSFPN model with the distillation term.

Bars for loss and gradient: 4 x the reference's own float32 error (the float32 CPU run recorded in the fixture, or the
restatement in float32 on the CPU), floored at 2^-22 of the loss and 2^-21 of the largest gradient: the kernels take d = s - t
and d * d in float32 like ``F.mse_loss`` and add in float64, so each term is off by at most two float32 roundings of random sign,
and the result is rounded to float32 once (2^-24)."""
import os

import numpy as np
import pytest
import torch

import embed_distill_ref as ER
from conftest import GOLDEN
from sgv3d_amd import _lib, distill, hip_ops
from sgv3d_amd.losses import EmbedDistillation

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLD = np.load(os.path.join(GOLDEN, "embed_distill.npz"))
CASES = sorted(k[:-6] for k in GOLD.files if k.endswith("_embed"))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _host_warp(teacher, minv, warped):
    lib = _lib.load()
    teacher = np.ascontiguousarray(teacher, np.float32)
    b, h, w, c = teacher.shape
    minv = np.ascontiguousarray(minv, np.float64).reshape(b, 9)
    warped = np.ascontiguousarray(warped, np.uint8)
    out = np.full(teacher.shape, np.nan, np.float32)
    dead = np.full((b, h, w), 7, np.uint8)
    rc = lib.sgv3d_embed_warp_host(b, h, w, c, teacher.ctypes.data, minv.ctypes.data, warped.ctypes.data, out.ctypes.data,
                                   dead.ctypes.data)
    assert rc == 0, lib.sgv3d_last_error()
    return torch.from_numpy(out), torch.from_numpy(dead)


def _matrices(rng, batch, h, w, strength=1.0):
    """inv(M) of plausible rectifications of an h x w map: zoom 0.8 .. 1.3, a few degrees of roll, a shift, a little perspective."""
    out = []
    for _ in range(batch):
        zoom = rng.uniform(0.8, 1.3)
        a = np.deg2rad(rng.uniform(-4, 4)) * strength
        cx, cy = 0.5 * (w - 1), 0.5 * (h - 1)
        lin = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]) / zoom
        t = np.array([cx, cy]) - lin @ np.array([cx, cy]) + rng.uniform(-0.7, 0.7, 2) * strength
        m = np.eye(3)
        m[:2, :2], m[:2, 2] = lin, t
        m[2, :2] = rng.uniform(-2e-4, 2e-4, 2) * strength
        out.append(m)
    return np.stack(out)


def _teacher(rng, b, h, w, c):
    return rng.standard_normal((b, h, w, c)).astype(np.float32)


# =============================================================================================== the warp kernel
@pytest.mark.parametrize("name", CASES)
def test_warp_kernel_matches_the_host_twin_on_the_fixture(name):
    teacher, minv = GOLD[name + "_embed"][None], GOLD[name + "_minv"][None]
    got, dead = distill.warp_embed(torch.from_numpy(teacher).to(DEV), minv, [1], return_dead=True)
    want, want_dead = _host_warp(teacher, minv, [1])
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(dead.cpu(), want_dead)
    assert torch.equal(_bits(got[0]), _bits(torch.from_numpy(GOLD[name + "_out"])))       # and so the reference's own output


SHAPES = [(1, 2, 2, 4), (3, 2, 2, 8), (1, 5, 7, 36), (3, 5, 7, 256), (1, 17, 241, 4), (3, 17, 241, 8), (1, 17, 241, 256),
          (3, 5, 7, 4), (1, 5, 7, 8), (3, 2, 2, 36), (1, 2, 2, 256), (3, 17, 241, 36),
          (3, 210, 210, 4)]          # more runs of pixels than the largest grid has waves: the second trip of every kernel


@pytest.mark.parametrize("shape", SHAPES)
def test_warp_kernel_matches_the_host_twin(shape):
    b, h, w, c = shape
    rng = np.random.default_rng(b * 1000 + h * 10 + c)
    teacher = _teacher(rng, b, h, w, c)
    minv = _matrices(rng, b, h, w)
    if h == 2:                      # a 2 x 2 map has one live position, (0, 0) read at exactly (0, 0): the identity; a shift kills it
        minv = np.tile(np.eye(3), (b, 1, 1))
        minv[1:, :2, 2] = rng.uniform(0.1, 0.3, (b - 1, 2))
    warped = [1] if b == 1 else [1, 0, 1]
    got, dead = distill.warp_embed(torch.from_numpy(teacher).to(DEV), minv, warped, return_dead=True)
    want, want_dead = _host_warp(teacher, minv, warped)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(dead.cpu(), want_dead)
    share = float(want_dead[0].float().mean())
    assert 0 < share < 1, share                                             # dead and live pixels in the warped frame
    if b == 3:
        assert torch.equal(_bits(got[1]), _bits(torch.from_numpy(teacher[1]))) and not dead[1].any()
    # against the torch restatement as well (positions, dead test and blends written a second time)
    ref, ref_dead = ER.warp_batch(torch.from_numpy(teacher), minv, warped)
    assert torch.equal(_bits(got), _bits(ref)) and torch.equal(dead.cpu().bool(), ref_dead)


def test_warp_guard_bands_dead_mask_nan_prefill_and_repeat():
    lib = _lib.load()
    b, h, w, c = 3, 9, 13, 8
    rng = np.random.default_rng(5)
    teacher = _teacher(rng, b, h, w, c)
    minv = _matrices(rng, b, h, w)
    warped = np.array([1, 0, 1], np.uint8)
    n, band = teacher.size, 64
    buf = torch.full((n + 2 * band,), float("nan"), device=DEV)
    dbuf = torch.full((b * h * w + 2 * band,), 9, dtype=torch.uint8, device=DEV)
    t = torch.from_numpy(teacher).to(DEV)
    m, wd = torch.from_numpy(minv).to(DEV), torch.from_numpy(warped).to(DEV)
    out, dead = buf[band:band + n], dbuf[band:band + b * h * w]
    want, want_dead = _host_warp(teacher, minv, warped)
    for _ in range(2):                                                     # the repeat launch writes the same bits
        rc = lib.sgv3d_embed_warp(b, h, w, c, t.data_ptr(), m.data_ptr(), wd.data_ptr(), out.data_ptr(), dead.data_ptr(),
                                  _lib.stream_handle(DEV))
        assert rc == 0, lib.sgv3d_last_error()
        assert torch.equal(_bits(out.view(b, h, w, c)), _bits(want)) and torch.equal(dead.cpu().view(b, h, w), want_dead)
    assert torch.isnan(buf[:band]).all() and torch.isnan(buf[band + n:]).all() and not torch.isnan(out).any()
    assert (dbuf[:band] == 9).all() and (dbuf[band + b * h * w:] == 9).all()
    # without a dead map, and a teacher holding NaN where no live pixel reads: dead outputs are zeros, not 0 * NaN
    poisoned = teacher.copy()
    _, d0 = ER.warp(torch.from_numpy(teacher[0]), minv[0])
    lonely = torch.ones(h, w, dtype=torch.bool)
    u, v = ER.positions(minv[0], h, w)
    for y in range(h):
        for x in range(w):
            if not d0[y, x]:
                r0, c0 = int(np.floor(float(v[y, x]))), int(np.floor(float(u[y, x])))
                lonely[r0:r0 + 2, c0:c0 + 2] = False
    assert lonely.any()
    poisoned[0][lonely.numpy()] = np.nan
    got = distill.warp_embed(torch.from_numpy(poisoned).to(DEV), minv, warped)
    assert torch.equal(_bits(got[0]), _bits(want[0]))


# =============================================================================================== loss and gradient
def _place(student, layout):
    """student [B, C, h, w] float32 on the CPU -> a device tensor of that shape and values in the named memory layout."""
    if layout == "nchw":
        return student.to(DEV).contiguous()
    if layout == "nhwc_view":           # what train_forward hands out: the NCHW view of an NHWC buffer
        return student.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
    if layout == "batch_slice":         # every other sample of a larger NHWC buffer, starting at the second
        b = student.shape[0]
        big = torch.full((2 * b + 1,) + tuple(student.permute(0, 2, 3, 1).shape[1:]), float("nan"), device=DEV)
        big[1::2] = student.permute(0, 2, 3, 1).to(DEV)
        return big[1::2].permute(0, 3, 1, 2)
    raise ValueError(layout)


def _bars(l64, l32, g64, g32):
    lbar = max(4 * abs(l32 - l64), 2.0 ** -22 * abs(l64))
    gbar = max(4 * float(np.abs(g32.astype(np.float64) - g64).max()), 2.0 ** -21 * float(np.abs(g64).max()))
    return lbar, gbar


def _reference(student, target, dead, weight, mask_dead):
    res = []
    for dt in (torch.float64, torch.float32):
        s = student.detach().clone().to(dt).requires_grad_(True)
        loss = ER.distill_loss(s, target, dead, weight, mask_dead)
        loss.backward()
        res += [float(loss.detach()), s.grad.numpy()]
    return res


BATCH = {}


def _batch_case():
    """Three frames of the 17 x 23 x 36 map: the fixture's strong warp, an unwarped frame, a shrinking warp; computed once."""
    if not BATCH:
        rng = np.random.default_rng(77)
        teacher = np.stack([GOLD["l_strong_embed"], GOLD["l_mild_embed"][::-1].copy(), GOLD["l_mild_embed"]])
        minv = np.stack([GOLD["l_strong_minv"], np.eye(3), GOLD["l_mild_minv"]])
        warped = np.array([1, 0, 1], np.uint8)
        student = torch.from_numpy((0.5 * rng.standard_normal((3, 36, 17, 23))).astype(np.float32))
        target, dead = ER.warp_batch(torch.from_numpy(teacher), minv, warped)
        assert torch.equal(_bits(target[0]), _bits(torch.from_numpy(GOLD["l_strong_out"])))
        BATCH.update(teacher=teacher, minv=minv, warped=warped, student=student, target=target, dead=dead)
        for mask in (False, True):
            BATCH[mask] = _reference(student, target, dead, 1000.0, mask)
    return BATCH


@pytest.mark.parametrize("mask_dead", [False, True])
@pytest.mark.parametrize("layout", ["nchw", "nhwc_view", "batch_slice"])
def test_loss_and_gradient_match_float64(layout, mask_dead):
    c = _batch_case()
    l64, g64, l32, g32 = c[mask_dead]
    s = _place(c["student"], layout).requires_grad_(True)
    loss = EmbedDistillation(1000.0, mask_dead)(s, torch.from_numpy(c["teacher"]).to(DEV), c["minv"], c["warped"])
    loss.backward()
    lbar, gbar = _bars(l64, l32, g64, g32)
    lerr = abs(float(loss.detach()) - l64)
    gerr = float(np.abs(s.grad.cpu().double().numpy() - g64).max())
    print(f"EMBED_DISTILL {layout} mask_dead={mask_dead}: loss {lerr:.3e} / {lbar:.3e} = {lerr / lbar:.3f}, "
          f"grad {gerr:.3e} / {gbar:.3e} = {gerr / gbar:.3f}")
    assert loss.dim() == 0 and loss.dtype == torch.float32
    # (autograd stores the gradient of a leaf that is not dense, the batch slice, as a contiguous tensor)
    assert s.grad.stride() == s.stride() or layout == "batch_slice"
    assert lerr <= lbar, (float(loss.detach()), l64, lbar)
    assert gerr <= gbar, (gerr, gbar)
    if mask_dead:
        assert not s.grad.cpu()[c["dead"][:, None].expand(-1, 36, -1, -1)].any() and abs(l64 - c[False][0]) > 1.0


@pytest.mark.parametrize("name", CASES)
def test_fixture_loss_and_gradient(name):
    """The reference's own numbers: F.mse_loss(gt_embeds, assist) * 1000 on the reference's warped embedding, float64, with its
    float32 CPU run as the yardstick."""
    s = torch.from_numpy(GOLD[name + "_student"])[None].to(DEV).requires_grad_(True)
    loss = EmbedDistillation()(s, torch.from_numpy(GOLD[name + "_embed"])[None].to(DEV), GOLD[name + "_minv"][None], [1])
    loss.backward()
    l64, g64 = float(GOLD[name + "_loss"]), GOLD[name + "_grad"]
    lbar, gbar = _bars(l64, float(GOLD[name + "_loss32"]), g64, GOLD[name + "_grad32"])
    lerr = abs(float(loss.detach()) - l64)
    gerr = float(np.abs(s.grad[0].cpu().double().numpy() - g64).max())
    print(f"EMBED_DISTILL fixture {name}: loss {lerr:.3e} / {lbar:.3e} = {lerr / lbar:.3f}, grad {gerr:.3e} / {gbar:.3e} = {gerr / gbar:.3f}")
    assert lerr <= lbar and gerr <= gbar, (lerr, lbar, gerr, gbar)


def test_plain_mse_without_matrices_and_large_map_second_trip():
    """No matrices: weight * mse.  130 x 260 pixels are more runs than the partial pass has waves (its second grid trip); the
    4-channel map also puts sixteen pixels into every wave pass."""
    rng = np.random.default_rng(3)
    b, c, h, w = 1, 4, 130, 260
    teacher = torch.from_numpy(_teacher(rng, b, h, w, c))
    student = torch.from_numpy(rng.standard_normal((b, c, h, w)).astype(np.float32))
    l64, g64, l32, g32 = _reference(student, teacher, None, 10.0, False)
    for layout in ("nchw", "nhwc_view"):
        s = _place(student, layout).requires_grad_(True)
        loss = EmbedDistillation(10.0)(s, teacher.to(DEV))
        loss.backward()
        lbar, gbar = _bars(l64, l32, g64, g32)
        assert abs(float(loss.detach()) - l64) <= lbar
        assert float(np.abs(s.grad.cpu().double().numpy() - g64).max()) <= gbar


# =============================================================================================== known answers
def test_student_equal_to_the_warped_teacher_gives_exact_zero():
    c = _batch_case()
    t = torch.from_numpy(c["teacher"]).to(DEV)
    target = distill.warp_embed(t, c["minv"], c["warped"])
    for layout_view in (target.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2).contiguous()):
        s = layout_view.clone(memory_format=torch.preserve_format).requires_grad_(True)
        loss = EmbedDistillation()(s, t, c["minv"], c["warped"])
        loss.backward()
        assert _bits(loss).item() == 0 and not _bits(s.grad).any()


def test_unit_difference_known_answer_bit_for_bit():
    b, c, h, w = 2, 8, 4, 8                       # N = 512
    rng = np.random.default_rng(1)
    teacher = torch.from_numpy(rng.integers(-8, 9, (b, h, w, c)).astype(np.float32)).to(DEV)
    sign = torch.from_numpy(rng.choice([-1.0, 1.0], (b, h, w, c)).astype(np.float32)).to(DEV)
    s = (teacher + sign).permute(0, 3, 1, 2).requires_grad_(True)
    minv = np.tile(np.eye(3), (b, 1, 1))
    for weight in (1000.0, 0.3):
        s.grad = None
        loss = EmbedDistillation(weight)(s, teacher, minv, [0, 0])        # unwarped frames: copied, the identity is not applied
        loss.backward()
        assert _bits(loss).item() == _bits(torch.tensor(np.float32(weight))).item()
        want = sign.permute(0, 3, 1, 2) * np.float32(2 * weight / 512)
        assert torch.equal(_bits(s.grad), _bits(want))


def test_mask_dead_all_dead_frame_and_no_live_pixel():
    b, c, h, w = 2, 4, 6, 10
    rng = np.random.default_rng(2)
    teacher = torch.from_numpy(_teacher(rng, b, h, w, c)).to(DEV)
    far = np.eye(3)
    far[0, 2] = 1e6                                # every position of frame 1 lies outside
    minv = np.stack([_matrices(rng, 1, h, w)[0], far])
    target, dead = ER.warp_batch(teacher.cpu(), minv, [1, 1])
    live = int((~dead).sum())
    assert dead[1].all() and 0 < live < h * w
    s = torch.from_numpy(rng.standard_normal((b, c, h, w)).astype(np.float32)).to(DEV).requires_grad_(True)
    loss = EmbedDistillation(64.0, mask_dead=True)(s, teacher, minv, [1, 1])
    loss.backward()
    assert not _bits(s.grad[1]).any()
    d = (s.detach().cpu() - target.permute(0, 3, 1, 2))[0][:, ~dead[0]]
    assert float(d.abs().min()) > 0
    # N is the live count: every live gradient is float32(2 * 64 / N * d), bit for bit
    want = (2 * 64.0 / (live * c) * d.double()).float()
    assert torch.equal(_bits(s.grad[0].cpu()[:, ~dead[0]]), _bits(want))
    assert abs(float(loss.detach()) - 64.0 * float((d.double() ** 2).mean())) <= 2.0 ** -22 * float(loss.detach())
    # no live pixel at all: loss and gradient are 0, not NaN
    s2 = s.detach().clone().requires_grad_(True)
    loss2 = EmbedDistillation(64.0, mask_dead=True)(s2, teacher, np.stack([far, far]), [1, 1])
    loss2.backward()
    assert _bits(loss2).item() == 0 and not _bits(s2.grad).any()
    # the reference's composition on the same input: the dead frame counts with target 0
    s3 = s.detach().clone().requires_grad_(True)
    EmbedDistillation(64.0)(s3, teacher, minv, [1, 1]).backward()
    want3 = (2 * 64.0 / (b * c * h * w) * s.detach()[1].cpu().double()).float()
    assert torch.equal(_bits(s3.grad[1]), _bits(want3))


def test_fused_call_equals_the_loss_on_the_materialised_warp():
    c = _batch_case()
    t = torch.from_numpy(c["teacher"]).to(DEV)
    target = distill.warp_embed(t, c["minv"], c["warped"])
    for layout in ("nchw", "nhwc_view"):
        for mask in (False,):
            s1 = _place(c["student"], layout).requires_grad_(True)
            s2 = _place(c["student"], layout).requires_grad_(True)
            fused = EmbedDistillation(1000.0, mask)(s1, t, c["minv"], c["warped"])
            plain = EmbedDistillation(1000.0, mask)(s2, target)
            fused.backward()
            plain.backward()
            assert _bits(fused).item() == _bits(plain).item() and torch.equal(_bits(s1.grad), _bits(s2.grad))


# =============================================================================================== autograd contract
def _inputs(seed=0):
    c = _batch_case()
    rng = np.random.default_rng(seed)
    s = torch.from_numpy(rng.standard_normal((3, 36, 17, 23)).astype(np.float32))
    return _place(s, "nhwc_view"), torch.from_numpy(c["teacher"]).to(DEV), torch.from_numpy(c["minv"]).to(DEV), \
        torch.from_numpy(c["warped"]).to(DEV)


def test_backward_entry_spy_and_upstream_factor(monkeypatch):
    lib = _lib.load()
    real, calls = lib.sgv3d_embed_distill_backward, []

    def spy(*args):
        calls.append(args)
        return real(*args)
    monkeypatch.setattr(lib, "sgv3d_embed_distill_backward", spy)
    x, t, m, wd = _inputs(1)
    fn = EmbedDistillation()
    loss = fn(x, t, m, wd)
    assert not loss.requires_grad and loss.dim() == 0
    k = torch.ones(1, device=DEV, requires_grad=True)
    (fn(x, t, m, wd) * k).sum().backward()                              # a backward pass that does not reach the student
    assert calls == [] and float(k.grad) == float(loss)
    xg = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    tg = t.clone().requires_grad_(True)
    fn(xg, tg, m, wd).backward()
    assert len(calls) == 1 and tg.grad is None                          # the teacher never gets a gradient
    x3 = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
    (3 * fn(x3, t, m, wd)).backward()
    assert len(calls) == 2 and calls[1][13] is not None                 # the upstream scalar went in as a device pointer
    assert torch.equal(_bits(3 * xg.grad), _bits(x3.grad))
    assert xg.grad.stride() == xg.stride()


def test_no_device_to_host_copy_in_forward_or_backward():
    x, t, m, wd = _inputs(2)
    fn = EmbedDistillation(mask_dead=True)
    fn(x.clone(memory_format=torch.preserve_format).requires_grad_(True), t, m, wd).backward()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        xg = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        (fn(xg, t, m, wd) * 2).backward()
        distill.warp_embed(t, m, wd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(xg.grad).all()


def test_forward_and_backward_in_one_graph():
    fn = EmbedDistillation()
    x0, t0, m0, w0 = _inputs(3)
    sx = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
    st, sm, sw = t0.clone(), m0.clone(), w0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(sx, st, sm, sw).backward()
    torch.cuda.current_stream().wait_stream(side)
    sx.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sloss = fn(sx, st, sm, sw)
        sloss.backward()
    rng = np.random.default_rng(8)
    for seed, flags in ((4, [0, 1, 1]), (5, [1, 1, 0])):
        x, t, _, _ = _inputs(seed)
        t = t.flip(0).contiguous()
        m = torch.from_numpy(_matrices(rng, 3, 17, 23)).to(DEV)
        wd = torch.tensor(flags, dtype=torch.uint8, device=DEV)
        with torch.no_grad():
            sx.copy_(x), st.copy_(t), sm.copy_(m), sw.copy_(wd)
        graph.replay()
        xe = x.clone(memory_format=torch.preserve_format).requires_grad_(True)
        want = fn(xe, t, m, wd)
        want.backward()
        assert _bits(sloss).item() == _bits(want).item() and torch.equal(_bits(sx.grad), _bits(xe.grad))


def test_python_layer_refuses_bad_inputs_before_any_launch():
    x, t, m, wd = _inputs(6)
    fn = EmbedDistillation()
    with pytest.raises(TypeError, match="float32"):
        fn(x.double(), t, m, wd)
    with pytest.raises(TypeError, match="float32"):
        fn(x, t.half(), m, wd)
    with pytest.raises(ValueError, match="needs a teacher"):
        fn(x, t.permute(0, 3, 1, 2), m, wd)
    with pytest.raises(ValueError, match="go together"):
        fn(x, t, m)
    with pytest.raises(ValueError, match="minv"):
        fn(x, t, m[:2], wd)
    with pytest.raises(_lib.SGV3DError, match="not covered"):
        fn(x[:, :3], t[..., :3].contiguous(), m, wd)
    with pytest.raises(_lib.SGV3DError, match="not covered"):
        distill.warp_embed(t[:, :1], m, wd)
    with pytest.raises(RuntimeError, match="MI355X only"):
        fn(x, t.cpu(), m, wd)


def test_workspace_one_byte_short_is_refused():
    lib = _lib.load()
    x, t, m, wd = _inputs(7)
    need = lib.sgv3d_embed_distill_workspace_bytes()
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    out = torch.full((1,), -5.0, device=DEV)
    saved = torch.full((2,), -5.0, dtype=torch.float64, device=DEV)
    st = x.stride()
    args = lambda n: (3, 36, 17, 23, x.data_ptr(), st[0], st[1], st[3], t.data_ptr(), m.data_ptr(), wd.data_ptr(), 1000.0, 0,
                      out.data_ptr(), saved.data_ptr(), ws.data_ptr(), n, _lib.stream_handle(DEV))
    assert lib.sgv3d_embed_distill_forward(*args(need - 1)) == -3 and b"workspace too small" in lib.sgv3d_last_error()
    torch.cuda.synchronize()
    assert float(out) == -5.0 and not ws.any()                              # nothing was launched
    assert lib.sgv3d_embed_distill_forward(*args(need)) == 0
    assert float(out) > 0 and float(saved[0]) == 3 * 36 * 17 * 23


# =============================================================================================== the teacher
def test_sam_teacher_is_the_predictors_resize_and_the_encoder(monkeypatch):
    from functools import partial
    from sgv3d_amd.layers.backbones.sam_encoder import ImageEncoderViT
    from sgv3d_amd.segment_anything import ops as sam_ops
    torch.manual_seed(4)
    enc = ImageEncoderViT(depth=2, embed_dim=64, img_size=1024, mlp_ratio=4, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6),
                          num_heads=2, patch_size=16, qkv_bias=True, use_rel_pos=True, global_attn_indexes=(1,), window_size=14,
                          out_chans=8, final_dim=(864, 1536), downsample_factor=16).to(DEV).eval()
    teacher = distill.SamTeacher(enc, dict(final_dim=(864, 1536)))
    assert abs(teacher.scale - 0.05) < 1e-15
    frames = torch.randint(0, 256, (1, 1080, 1920, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(DEV)
    calls = []
    real_forward, real_resize = enc.forward, sam_ops.resize_bilinear_u8
    monkeypatch.setattr(enc, "forward", lambda x: (calls.append(("forward", tuple(x.shape))), real_forward(x))[1])
    monkeypatch.setattr(sam_ops, "resize_bilinear_u8", lambda f, size, **k: (calls.append(("resize", tuple(size))), real_resize(f, size, **k))[1])
    got = teacher(frames)
    assert calls == [("resize", (576, 1024)), ("forward", (1, 3, 576, 1024))]
    assert tuple(got.shape) == (1, 54, 96, 8) and got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad
    want = real_forward(real_resize(frames, (576, 1024)))                   # what the predictor's resize and the encoder give
    assert torch.equal(_bits(got), _bits(want.permute(0, 2, 3, 1))) and float(got.abs().max()) > 0
    with pytest.raises(ValueError, match="uint8"):
        teacher(frames[:, :1000])


# =============================================================================================== one training step
def _profiled(fn):
    hip_ops.PROFILE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [rec[0].split('|')[0] for rec in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = None
    return out, names


def test_training_step_with_the_distillation_term():
    from oracle import torch_model as O
    from test_train_forward_gpu import _gt, _model, _oracle_loss
    from sgv3d_amd import synthetic
    from sgv3d_amd.models.bev_height import BEVHeight
    B = 2
    _, bconf, hconf = _model()
    bconf = dict(bconf, is_train_height=True)
    torch.manual_seed(0)
    model = BEVHeight(bconf, hconf, is_train_height=True)
    synthetic.randomize_norm_stats_(model, seed=0)
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model = model.cuda().train()
    head_cfg = dict(model.head.train_cfg, grid_size=[256, 256, 1], point_cloud_range=[0, -12.8, -5, 25.6, 12.8, 3])
    model.head.train_cfg = head_cfg
    imgs = synthetic.make_images(B, final=bconf['final_dim'], device='cuda', seed=3)
    mats = synthetic.make_mats(B, device='cuda', scale=bconf['final_dim'][0] / 864)
    boxes, labels = _gt(B)
    h, w = bconf['final_dim'][0] // 16, bconf['final_dim'][1] // 16
    rng = np.random.default_rng(9)
    teacher = _teacher(rng, B, h, w, 256) * 0.5
    minv, warped = _matrices(rng, B, h, w), np.array([1, 0], np.uint8)
    names = [n for n, p in model.named_parameters() if p.requires_grad]

    def run(weight):
        model.zero_grad(set_to_none=True)
        preds, (assist, assist2) = model(imgs, mats)
        assert assist is assist2 and tuple(assist.shape) == (B, 256, h, w)
        targets = model.get_targets([b.cuda() for b in boxes], [l.cuda() for l in labels])
        loss = model.loss(targets, preds)
        if weight:
            loss = loss + EmbedDistillation(weight)(assist, torch.from_numpy(teacher).to(DEV), minv, warped)
        loss.backward()
        return loss.detach(), targets, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}

    (loss0, targets, g0), names0 = _profiled(lambda: run(0.0))
    (loss1, _, g1), names1 = _profiled(lambda: run(1000.0))
    assert not any("embed" in n for n in names0) and names1.count("embed_distill") == 1 and names1.count("embed_distill_backward") == 1
    # without the term the assist layer gets nothing (the statement of tests/test_train_forward_gpu.py:98) and the step is today's:
    # the same launches as a model that returns no aux output, the same bits
    for n in ("backbone.assist_layer.weight", "backbone.assist_layer.bias"):
        assert g0[n] is None or not g0[n].any()
    model.is_train_height = False
    model.backbone.is_train_height = False
    try:
        model.zero_grad(set_to_none=True)
        preds = model(imgs, mats)
        today = model.loss(model.get_targets([b.cuda() for b in boxes], [l.cuda() for l in labels]), preds)
        today.backward()
        assert _bits(today).item() == _bits(loss0).item()
    finally:
        model.is_train_height = True
        model.backbone.is_train_height = True
    assert float(loss1) > float(loss0)

    # float64 oracle: the detector's training forward with is_train_height plus the restatement of the distillation
    sd = {k: (v.detach().cpu().double() if v.dtype.is_floating_point else v.detach().cpu()) for k, v in model.state_dict().items()}
    for n in names:
        sd[n].requires_grad_(True)
    rpreds, (rassist, _) = O.bevheight_train_forward(sd, bconf, hconf, imgs.cpu(), {k: v.cpu() for k, v in mats.items()},
                                                     is_train_height=True)
    tc = tuple([x.cpu().double() if x.dtype == torch.float32 else x.cpu() for x in part] for part in targets)
    target, dead = ER.warp_batch(torch.from_numpy(teacher), minv, warped)
    rloss = _oracle_loss(rpreds, tc, head_cfg['code_weights']) + ER.distill_loss(rassist, target, dead, 1000.0)
    rloss.backward()
    assert abs(float(loss1) - float(rloss.detach())) <= 1e-3 * abs(float(rloss.detach()))
    for n in ("backbone.assist_layer.weight", "backbone.assist_layer.bias"):
        got, want = g1[n].cpu().double(), sd[n].grad
        assert float(got.abs().max()) > 0
        rel = float((got - want).norm() / (want.norm() + 1e-12))
        print(f"EMBED_DISTILL step {n}: relative L2 error {rel:.3e} (bar 2e-2)")
        assert rel <= 2e-2, (n, rel)                  # the median bar of test_training_forward_backward_matches_oracle
    moved = [n for n in names if 'img_backbone' in n and g0[n] is not None
             and float((g1[n] - g0[n]).norm()) > 1e-3 * float(g0[n].norm())]
    assert len(moved) > 20, len(moved)               # the distillation reaches the image backbone
