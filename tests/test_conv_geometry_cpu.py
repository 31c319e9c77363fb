"""The index arithmetic of the stride-2 data gradient (conv_grad._dgrad_stride2: ``_phase_1d``, ``need``, ``pp``, the interleave
offsets) with the four sub-convolutions computed by F.conv2d and the interleave done by slicing, against float64 autograd on small
integers -- bit for bit, under the cover condition the interleave launcher enforces.  What the kernels do on those layers is
test_conv_geometry_gpu.py's business."""
import pytest
import torch

import conv_geometry as G


def _geometries():
    for k in range(1, 8):
        for pad in range(0, 5):
            if (k, pad) in ((1, 0), (2, 0)):          # 1x1 / pad 0 convolves at the coarse resolution, 2x2 / pad 0 is the patchify layer
                continue
            for H in range(1, 10):
                for W in range(1, 10):
                    oh, ow = G.out_hw(H, W, k, k, 2, pad, 1)
                    if oh > 0 and ow > 0:
                        yield k, pad, H, W


def test_sweep_is_the_documented_one():
    assert sum(1 for _ in _geometries()) == 2204


@pytest.mark.parametrize("k", range(1, 8))
def test_stride2_decomposition_equals_autograd(k):
    g = torch.Generator().manual_seed(k)
    B, cin, cout = 2, 3, 2
    n = 0
    for kk, pad, H, W in _geometries():
        if kk != k:
            continue
        oh, ow = G.out_hw(H, W, k, k, 2, pad, 1)
        x = torch.zeros(B, H, W, cin)
        w = torch.randint(-3, 4, (cout, cin, k, k), generator=g).float()
        dy = torch.randint(-4, 5, (B, oh, ow, cout), generator=g).float()
        _, dx_ref, _ = G.autograd_reference(x, w, dy, 2, pad, 1)
        dx = G.dgrad_stride2_reference(dy, w, (H, W), pad)
        assert torch.equal(dx, dx_ref), (k, pad, H, W)
        n += 1
    assert n > 0


def test_dgrad_forms_restates_the_decomposition():
    # 3x3 / stride 2 / pad 1: taps 2x2, 2x1, 1x2, 1x1; 7x7 / pad 3: 4x4, 4x3, 3x4, 3x3 -- all at stride 1 on dY, one padding for both axes
    taps = lambda k, pad, H, W: sorted((f.kh, f.kw) for f in G.dgrad_forms(k, 2, pad, 1, H, W, 8, 12))
    assert taps(3, 1, 9, 9) == [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert taps(7, 3, 12, 13) == [(3, 3), (3, 4), (4, 3), (4, 4)]
    for f in G.dgrad_forms(3, 2, 1, 1, 9, 9, 8, 10):
        assert (f.cin, f.cout, f.stride, f.dil, f.kind) == (12, 8, 1, 1, "phase") and f.pad >= 0
    # an axis with a single tap carries the other axis' padding: whole output rows / columns lie in it
    got = {(f.kh, f.kw, f.pad) for f in G.dgrad_forms(3, 2, 0, 1, 10, 13, 8, 12)}
    assert got == {(2, 2, 1), (2, 1, 1), (1, 2, 1), (1, 1, 1)}
    (f,) = G.dgrad_forms(3, 1, 0, 6, 20, 20, 8, 12)
    assert (f.kh, f.kw, f.pad, f.dil, f.H, f.W, f.kind) == (3, 3, 12, 6, 8, 8, "rot")
    (f,) = G.dgrad_forms(3, 3, 1, 1, 9, 8, 8, 12)
    assert (f.pad, f.H, f.W) == (1, 9, 8)                     # zero-inserted map: H + 2 pad - (k - 1)
    (f,) = G.dgrad_forms(2, 2, 0, 1, 6, 7, 8, 12)
    assert f.kind == "patchify"


@pytest.mark.parametrize("stride", (1, 3))
def test_data_gradient_refuses_padding_beyond_the_kernel(stride):
    """pad > dil (k - 1): the rotated layer would need a negative padding.  Refused by name before anything is packed or launched
    (CPU tensors: a launch would fail differently)."""
    from sgv3d_amd import _lib, conv_grad
    k, pad, H = 3, 3, 4
    oh = (H + 2 * pad - (k - 1) - 1) // stride + 1
    dy, w = torch.zeros(1, oh, oh, 8), torch.zeros(8, 4, k, k)
    with pytest.raises(_lib.SGV3DError, match=rf"8x4 k3x3 s{stride} p3 d1 layer pads by more than its kernel reaches"):
        conv_grad.conv2d_backward_data(dy, w, (H, H), stride, pad, 1)
