"""Sibling F(4x4) layers on one input through sgv3d_conv2d_winograd4_forward_multi (one input-transform launch, the grouped GEMMs,
one output-transform launch; csrc/conv_wino4.hip) against the same layers called one by one: bit for bit, in the guard-banded
buffers of tests/wino_edges.py; ASPP through either route; and the global average pool's one-channel-per-thread form."""
import pytest
import torch

import wino_edges as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = 128


def _convs(dils, seed):
    from sgv3d_amd.hip_ops import PackedConv
    g = E._gen(81, seed)
    out = []
    for k, dil in enumerate(dils):
        w = torch.randn(C, C, 3, 3, generator=g) / (C * 9) ** 0.5
        sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
        kw = dict(scale=sc.to(DEV), shift=sh.to(DEV)) if k != 1 else {}               # the second layer: no folded BN (null scale / bias)
        out.append((PackedConv(w.to(DEV), pad=dil, dil=dil, relu=(k != 2), **kw), w, sc if k != 1 else None, sh if k != 1 else None))
    return out


@pytest.mark.parametrize("geom,dils,variants", [((2, 13, 22), (6, 12, 18), (0, 3, 7)), ((1, 7, 19), (1, 2, 3), (9, 1, 4)),
                                                ((1, 35, 49), (18, 6), (2, 5)), ((1, 5, 9), (1, 6, 12, 18), (6, 8, 0, 1))],
                         ids=lambda v: E.gid(v) if isinstance(v, tuple) else str(v))
def test_multi_equals_the_single_calls_bit_for_bit(geom, dils, variants):
    """2, 3 and 4 descriptors with different dilations, tile variants, ReLU, folded BN or none and output slices: the multi entry
    point writes exactly what the single calls write, nothing outside the slices, and is within the F(4x4) bar of float64."""
    from sgv3d_amd import hip_ops
    x3 = list(hip_ops.WINO4_X3_TILES)
    B, H, W = geom
    n = len(dils)
    layers = _convs(dils, n)
    convs = [l[0] for l in layers]
    tiles = [x3[v] for v in variants]
    x = torch.randn(B, H, W, C, generator=E._gen(82, B, H, W))
    xg = E.guarded_input(x, C + 16, 0, DEV)                                          # channels [0, C) of a wider map, the rest NaN
    ld = n * (C + 4) + 8
    offs = [4 + k * (C + 4) for k in range(n)]                                       # slices with sentinel channels between them

    def single():
        out = E.GuardedOutput((B, H, W, ld), (W + 1) * ld, DEV)
        for c, o, t in zip(convs, offs, tiles):
            c(xg, out.view, y_coff=o, tile=t, split_k=1)
        return out

    def multi():
        out = E.GuardedOutput((B, H, W, ld), (W + 1) * ld, DEV)
        hip_ops.wino4_multi(convs, xg, out.view, offs, tiles)
        return out
    a, b = single(), multi()
    assert torch.equal(a.flat, b.flat), "the multi launch differs from the single calls"
    assert torch.equal(b.flat, multi().flat)
    for (c, w, sc, sh), o in zip(layers, offs):
        got, _ = b.result((o, C))
        assert not bool(torch.isnan(got).any())
        ref = E.epilogue64(E.conv64(x, w, pad=c.dil, dil=c.dil), sc, sh, relu=bool(c.relu))
        assert float((got - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))
    body = b.flat[b.slack:b.flat.numel() - b.slack].view(B, H, W, ld).cpu()
    keep = torch.ones(ld, dtype=torch.bool)
    for o in offs:
        keep[o:o + C] = False
    assert bool((body[..., keep] == E.SENTINEL).all()) and bool((b.flat[:b.slack] == E.SENTINEL).all()) and bool((b.flat[-b.slack:] == E.SENTINEL).all())


def test_wrapper_refuses_what_it_does_not_cover():
    from sgv3d_amd import hip_ops
    from sgv3d_amd._lib import SGV3DError
    convs = [l[0] for l in _convs((6, 12, 18), 3)]
    x3 = list(hip_ops.WINO4_X3_TILES)
    x = torch.zeros(1, 7, 19, C, device=DEV)
    out = torch.zeros(1, 7, 19, 3 * C, device=DEV)
    with pytest.raises(SGV3DError):
        hip_ops.wino4_multi(convs, x, out, [0, C, 2 * C], [x3[0], 9, x3[1]])          # an f32 F(4x4) tile
    with pytest.raises(SGV3DError):
        hip_ops.wino4_multi(convs, x, out, [0, C, 2 * C + 4], [x3[0]] * 3)            # past the buffer
    with pytest.raises(SGV3DError):
        hip_ops.wino4_multi(convs[:1], x, out, [0], [x3[0]])


def test_aspp_through_either_route(monkeypatch):
    """ASPP.hip_forward with the three dilated branches through the multi entry point and through the per-layer calls: the same
    bits, and the multi route is the one taken when the layers' choices are f32x3 tiles and the record says so."""
    from sgv3d_amd import hip_ops
    from sgv3d_amd.layers.backbones.lss_fpn import ASPP
    torch.manual_seed(5)
    m = ASPP(C, C).eval().to(DEV)
    x = torch.randn(1, 13, 22, C, device=DEV)
    x3 = list(hip_ops.WINO4_X3_TILES)
    monkeypatch.setattr(hip_ops, "TUNE_DB", dict(hip_ops.TUNE_DB))
    convs = [b.hip_state(x.device) for b in (m.aspp2, m.aspp3, m.aspp4)]
    for c, t in zip(convs, (x3[0], x3[1], x3[5])):
        c._tile_cache[(1, 13, 22, 0, 0, False, False, hip_ops.CONV_NORMAL, False, False, 0)] = (t, 1)
    hip_ops.TUNE_DB[hip_ops.wino4_multi_signature(convs, x)] = [1, 0]
    calls = []
    real = hip_ops.wino4_multi
    monkeypatch.setattr(hip_ops, "wino4_multi", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        fused = m.hip_forward(x).clone()
        assert calls == [1]
        monkeypatch.setattr(hip_ops, "WINO4_MULTI", False)
        plain = m.hip_forward(x).clone()
        assert calls == [1]
    assert torch.equal(fused, plain)


@pytest.mark.parametrize("Cn,ld", [(30, 30), (30, 44), (64, 65), (5, 7)])
def test_global_avgpool_one_channel_per_thread(Cn, ld):
    """C or the leading dimension no multiple of 4: sgv3d_global_avgpool runs its scalar first stage.  Same sums per channel as the
    16-byte form (compared on the shared channels of an aligned copy), within P eps mean |x| of the float64 mean."""
    from sgv3d_amd import _lib
    lib, B, P, eps = _lib.load(), 2, 777, 2.0 ** -24
    x = torch.randn(B, P, ld, generator=E._gen(83, Cn, ld))
    xd = x.to(DEV)

    def run(t, c, l):
        nbytes = lib.sgv3d_global_avgpool_workspace_bytes(B, c)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = E.GuardedOutput((B, c), 64, DEV)
        _lib.check(lib.sgv3d_global_avgpool(B, P, c, l, t.data_ptr(), out.view.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_handle()), "avgpool")
        got, intact = out.result()
        assert intact
        return got
    got = run(xd, Cn, ld)
    want = x[..., :Cn].double().mean(1)
    bound = P * eps * x[..., :Cn].double().abs().mean(1)
    assert bool(((got - want).abs() <= bound).all())
    c4 = Cn // 4 * 4                                                                  # the 16-byte form on an aligned copy of the first channels
    aligned = x[..., :c4].contiguous().to(DEV)
    assert torch.equal(run(aligned, c4, c4), got[:, :c4])
