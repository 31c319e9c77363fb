"""The fused bf16 CenterHead (csrc/head_bf16.hip) against its contract, bit for bit: all three kernels (warp-specialised, single-role,
ping-pong) through both entries (f32 input, bf16 input -- the one bf16 mode runs) at every remainder of the 16 x 16 tile and of the
4-pixel store group (tests/head_bf16_edges.py: GEOMS), on data whose bf16 roundings of x, w1 and the hidden map change values,
exact ties among them, while every partial sum stays a float32 number: the float64 evaluation of the contract is the expected
output and every comparison is torch.equal (tests/test_head_bf16_edges_cpu.py: why that holds, and that a truncating or
tie-away rounding, a rounding left out or an unzeroed hidden pixel outside the image cannot pass).  Every input is a channel
window of a wider NaN-filled map inside a NaN-filled allocation, every output lies between sentinels, every launch runs twice.
Then the branch counts at which the pipelined kernels fill and drain, the 48-branch limit, what the entries and the packer
refuse, and that BEVHeightHead hands the kernel what the sweep covers."""
import pytest
import torch

import head_bf16_edges as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
RAN = {"combinations": 0}          # (map, entry, kernel, window) combinations compared so far in this process


class _Head:
    """The device-side arguments of one branch structure: packed weights, folded BN, biases, out_begin."""

    def __init__(self, p):
        from sgv3d_amd import hip_ops
        self.p, self.counts, self.nb, self.total = p, p["counts"], len(p["counts"]), sum(p["counts"])
        ob = [0]
        for c in self.counts:
            ob.append(ob[-1] + c)
        self.ob = torch.tensor(ob, dtype=torch.int32, device=DEV)
        self.packed = hip_ops.pack_centerhead_bf16(p["w1"].to(DEV), p["w2"].permute(0, 2, 3, 1).contiguous().to(DEV), self.ob)
        self.sc, self.sh, self.b2 = p["sc"].to(DEV), p["sh"].to(DEV), p["b2"].to(DEV)

    def __call__(self, x, out, x_coff=0):
        from sgv3d_amd import hip_ops
        return hip_ops.centerhead_branches_bf16(x, self.packed, self.sc, self.sh, self.b2, self.ob, self.nb, out=out, x_coff=x_coff)


@pytest.fixture(scope="module")
def heads():
    cache = {}

    def get(counts=E.COUNTS, p=None):
        if counts not in cache:
            cache[counts] = _Head(p or E.params(counts))
        return cache[counts]
    return get


@pytest.fixture
def select():
    """sgv3d_centerhead_bf16_select_plain, put back to the default kernel whatever happens."""
    from sgv3d_amd import _lib
    lib = _lib.load()
    try:
        yield lib.sgv3d_centerhead_bf16_select_plain
    finally:
        lib.sgv3d_centerhead_bf16_select_plain(0)


def _inputs(x):
    """[(entry, (ld, coff), guarded device tensor)]: the f32 tensor and its bf16 rounding, each in both channel windows."""
    xb = E.round_bf16(x).float()
    return [("f32", w, E.guarded_input(x, w[0], w[1], DEV)) for w in E.F32_WINDOWS] + \
           [("bf16", w, E.guarded_input_bf16(xb, w[0], w[1], DEV)) for w in E.BF16_WINDOWS]


def _exact(head, select, geom, x, ref, what):
    """Every (entry, window, kernel) on one map: no NaN, sentinels intact, bit equality with ref, the same bits a second time."""
    B, H, W = geom
    for entry, (ld, coff), xg in _inputs(x):
        assert xg.dtype == (torch.float32 if entry == "f32" else torch.bfloat16)
        for kernel in E.KERNELS:
            tag = (what, E.gid(geom), entry, ld, coff, kernel)
            select(kernel)
            outs = []
            for _ in range(2):
                out = E.GuardedOutput((B, head.total, H, W), W + 1, DEV)
                head(xg, out.view, x_coff=coff)
                outs.append(out)
            got, intact = outs[0].result()
            assert not bool(torch.isnan(got).any()), ("a read outside the map or the channel window reached an output", tag)
            assert intact, ("a store outside the output", tag)
            assert tuple(got.shape) == tuple(ref.shape)
            assert torch.equal(got, ref), (tag, float((got - ref).abs().max()), int((got != ref).sum()))
            assert torch.equal(outs[0].flat, outs[1].flat), ("two launches differ", tag)
            RAN["combinations"] += 1
    select(0)


@pytest.mark.parametrize("geom", E.GEOMS, ids=E.gid)
def test_head_bf16_exact_at_every_remainder(heads, select, geom):
    """{f32 entry, bf16x entry} x {kernels 0, 1, 3} x two channel windows on every map of GEOMS, branch widths (1, 4, 2, 3):
    12 combinations per map, 456 in all, each torch.equal to the exact reference.  (With the branch-count and zero-width tests
    below: 600 combinations; the whole file takes 3.4 s on the MI355X.)"""
    x, ref = E.head_case(geom)
    _exact(heads(), select, geom, x, ref, "sweep")
    print(f"bf16 head sweep: {RAN['combinations']} (map, entry, kernel, window) combinations so far")


@pytest.mark.parametrize("geom", E.BRANCH_GEOMS, ids=E.gid)
@pytest.mark.parametrize("nb", E.BRANCH_COUNTS)
def test_head_bf16_branch_counts(heads, select, geom, nb):
    """1, 2 and 3 branches -- where the warp-specialised kernel's two roles and the ping-pong kernel's two groups fill and drain
    (one group idle at nb = 1, an odd count at 3) -- and kMaxBranches = 48 (the single-role kernel's folded-BN table in LDS is
    full), widths cycling 1..4, on the smallest maps that cross a tile seam: exact in all three kernels, both entries."""
    counts = E.cycling_counts(nb)
    x, ref = E.head_case(geom, counts)
    _exact(heads(counts), select, geom, x, ref, f"nb {nb}")


@pytest.mark.parametrize("geom", E.BRANCH_GEOMS, ids=E.gid)
def test_head_bf16_zero_width_branch(heads, select, geom):
    """Widths (2, 0, 4, 1): the branch in the middle has first-layer weights and no outputs.  The planes are those of the head
    without it -- bit for bit, and both are the exact reference."""
    p = E.params((2, 0, 4, 1))
    x = E.head_x(geom)
    ref = E.head_ref(x, p)
    assert torch.equal(ref, E.head_ref(x, E.without_branch(p, 1)))
    _exact(heads((2, 0, 4, 1)), select, geom, x, ref, "zero-width")
    _exact(heads((2, 4, 1), E.without_branch(p, 1)), select, geom, x, ref, "without it")


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(call, exc):
    """``call(out view)`` raises ``exc`` and nothing was launched: the output and its guard bands still hold the sentinel."""
    out = E.GuardedOutput((1, sum(E.COUNTS), 5, 6), 7, DEV)
    with pytest.raises(exc):
        call(out.view)
    torch.cuda.synchronize()
    assert bool((out.flat == E.SENTINEL).all())


def test_head_bf16_entries_refuse_what_they_cannot_run(heads):
    """Each raises SGV3DError before any launch: 49 branches; cin != 64; an f32 x_coff of 2; a bf16 x_coff of 4; a bf16 x_ld of
    68; an x that is not 16-byte aligned (either dtype)."""
    from sgv3d_amd import _lib
    from sgv3d_amd._lib import SGV3DError
    lib = _lib.load()
    head = heads()
    geom = (1, 5, 6)
    x = E.head_x(geom)
    xb = E.round_bf16(x).float()
    good = E.GuardedOutput((1, head.total, 5, 6), 7, DEV)
    head(E.guarded_input(x, 96, 16, DEV), good.view, x_coff=16)                  # the arguments below are one step from this call
    assert torch.equal(good.result()[0], E.head_ref(x, head.p))

    # 49 branches: buffers of the right size for 49, so that the refusal is the only thing between the call and a launch
    nb = E.MAX_BRANCHES + 1
    counts = E.cycling_counts(nb)
    big = _Head.__new__(_Head)
    big.nb, big.total = nb, sum(counts)
    big.ob = torch.tensor([sum(counts[:i]) for i in range(nb + 1)], dtype=torch.int32, device=DEV)
    big.packed = (torch.zeros(lib.sgv3d_centerhead_bf16_weight_bytes(nb), dtype=torch.uint8, device=DEV),
                  torch.zeros(lib.sgv3d_centerhead_bf16_weight2_bytes(nb), dtype=torch.uint8, device=DEV))
    big.sc, big.sh, big.b2 = torch.ones(nb * 64, device=DEV), torch.zeros(nb * 64, device=DEV), torch.zeros(big.total, device=DEV)
    x49 = E.guarded_input(x, 64, 0, DEV)
    out49 = E.GuardedOutput((1, big.total, 5, 6), 7, DEV)
    with pytest.raises(SGV3DError, match="at most 48 branches"):
        big(x49, out49.view)
    torch.cuda.synchronize()
    assert bool((out49.flat == E.SENTINEL).all())

    def raw_cin(cin, xg, fn):
        def call(out):
            rc = fn(1, 5, 6, cin, int(xg.shape[-1]), 0, xg.data_ptr(), head.nb, head.packed[0].data_ptr(), head.sc.data_ptr(),
                    head.sh.data_ptr(), head.total, head.packed[1].data_ptr(), head.b2.data_ptr(), head.ob.data_ptr(), out.data_ptr(),
                    _lib.stream_handle(xg.device))
            _lib.check(rc, "sgv3d_centerhead_branches_forward_bf16")
        return call
    _refused(raw_cin(32, E.guarded_input(x, 64, 0, DEV), lib.sgv3d_centerhead_branches_forward_bf16), SGV3DError)
    _refused(raw_cin(128, E.guarded_input_bf16(torch.cat([xb, xb], -1), 128, 0, DEV), lib.sgv3d_centerhead_branches_forward_bf16x), SGV3DError)

    x96 = E.guarded_input(x, 96, 16, DEV)
    _refused(lambda out: head(x96, out, x_coff=2), SGV3DError)                   # f32: x_coff a multiple of 4
    xb96 = E.guarded_input_bf16(xb, 96, 24, DEV)
    _refused(lambda out: head(xb96, out, x_coff=4), SGV3DError)                  # bf16: x_coff a multiple of 8
    xb68 = torch.zeros(1, 5, 6, 68, dtype=torch.bfloat16, device=DEV)
    _refused(lambda out: head(xb68, out), SGV3DError)                            # bf16: x_ld a multiple of 8 (68 passes the f32 rule)
    n = 5 * 6 * 64
    flat = torch.zeros(n + 8, device=DEV)
    off4 = flat[1:1 + n].view(1, 5, 6, 64)
    flatb = torch.zeros(n + 8, dtype=torch.bfloat16, device=DEV)
    off8 = flatb[4:4 + n].view(1, 5, 6, 64)
    assert off4.data_ptr() % 16 == 4 and off8.data_ptr() % 16 == 8 and off4.is_contiguous() and off8.is_contiguous()
    _refused(lambda out: head(off4, out), SGV3DError)
    _refused(lambda out: head(off8, out), SGV3DError)


@pytest.mark.parametrize("name,ob,rows,nb", [("a branch of 5", [0, 2, 7, 8], 8, 3), ("decreasing", [0, 3, 2, 6], 6, 3),
                                            ("wrong total", [0, 2, 4, 5], 6, 3), ("does not start at 0", [1, 2, 4, 6], 6, 3),
                                            ("49 branches", list(range(50)), 49, 49)], ids=lambda v: v.replace(" ", "-") if isinstance(v, str) else None)
def test_pack_centerhead_bf16_refuses_what_the_kernel_cannot_compute(name, ob, rows, nb):
    """Widths (2, 5, 1) used to pack columns 0..3 of the wide branch and the kernel stored a copy of column 0 into its fifth
    plane, silently.  pack_centerhead_bf16 reads the table back once per weight load and raises ValueError, like
    head_branch_of_out, before any launch; what it accepts is what the sweep above runs."""
    from sgv3d_amd import hip_ops
    w1 = torch.zeros(nb * 64, 64, 3, 3, device=DEV)
    w2 = torch.zeros(rows, 3, 3, 64, device=DEV)
    with pytest.raises(ValueError, match="bf16 fused head"):
        hip_ops.pack_centerhead_bf16(w1, w2, torch.tensor(ob, dtype=torch.int32, device=DEV))
    assert hip_ops.HEAD_BF16_MAX_OUT == 4 and hip_ops.HEAD_BF16_MAX_BRANCHES == E.MAX_BRANCHES


# -------------------------------------------------------------------------------------------------------------------- routing
@pytest.mark.parametrize("bf16_activations", [True, False], ids=["bf16-activations", "f32-activations"])
def test_head_module_hands_the_kernel_what_the_sweep_covers(monkeypatch, bf16_activations):
    """BEVHeightHead.forward (hip_forward behind it) of the small_conf() model in bf16 mode calls hip_ops.centerhead_branches_bf16 once: with a bf16
    shared map when BF16_ACTIVATIONS is on (the production default: the bf16x entry), with an f32 one when it is off; channels
    [0, 64) of a 64-channel map, no out=, branches of at most 4 outputs.  The head's predictions are views of that call's
    result, and a direct call on the recorded arguments gives the same bits."""
    from sgv3d_amd import hip_ops
    from sgv3d_amd import synthetic as S
    from sgv3d_amd.models.bev_height import BEVHeight
    monkeypatch.setattr(hip_ops, "MFMA_BF16", True)
    monkeypatch.setattr(hip_ops, "MFMA_F32X3", False)
    monkeypatch.setattr(hip_ops, "BF16_ACTIVATIONS", bf16_activations)
    monkeypatch.setattr(hip_ops, "AUTOTUNE", False)
    assert hip_ops.FUSED_HEAD
    torch.manual_seed(0)
    bc, hc = S.small_conf()
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 0)
    head = m.head.to(DEV)
    bev = torch.randn(2, hc["bev_backbone_conf"]["in_channels"], 24, 40, generator=torch.Generator().manual_seed(3)).to(DEV)
    real, calls = hip_ops.centerhead_branches_bf16, []

    def recorder(*a, **k):
        out = real(*a, **k)
        calls.append((a, k, out))
        return out

    monkeypatch.setattr(hip_ops, "centerhead_branches_bf16", recorder)
    with torch.no_grad():
        preds = head(bev)                                   # NCHW in, as the reference: forward pads the channels and calls hip_forward
    assert len(calls) == 1
    a, k, out = calls[0]
    x = a[0]
    assert x.dtype == (torch.bfloat16 if bf16_activations else torch.float32)
    assert tuple(x.shape) == (2, 24, 40, 64) and x.is_contiguous() and not k
    s = head.hip_state(bev.device)
    widths = [c for _, _, _, c in s["slices"]]
    assert a[6] == len(widths) == 36 and max(widths) <= hip_ops.HEAD_BF16_MAX_OUT and a[5].tolist()[-1] == sum(widths) == out.shape[1]
    assert float(out.abs().max()) > 0 and bool(torch.isfinite(out).all())
    direct = real(*a)
    assert direct.data_ptr() != out.data_ptr() and torch.equal(direct, out)
    for t, name, off, c in s["slices"]:
        v = preds[t][0][name]
        assert v.data_ptr() == out[:, off:off + c].data_ptr() and torch.equal(v, direct[:, off:off + c])
