"""CPU: the inputs of tests/test_bsm_train_edges_gpu.py are fair to the kernels of csrc/bsm_train.hip.

For every generated focal case the oracle (oracle/focal_ref.py) evaluated in float32 stays within a quarter of the bound
the GPU test applies to the kernel against the float64 oracle, and the float64 gradient is finite -- so a GPU failure
cannot be blamed on the inputs.  The nothing-kept cases are the exception: the oracle's behaviour there (loss NaN for
'mean', gradient all zero) is pinned here by hand.  The label, upsample and gate generators are checked for the
properties their GPU tests rely on."""
import math

import pytest
import torch

import bsm_train_edges as E
from oracle import focal_ref as R


# ----------------------------------------------------------------------------------------------- focal loss
@pytest.mark.parametrize("name", list(E.FOCAL_CASES))
def test_float32_oracle_within_a_quarter_of_the_bound(name):
    case = E.FOCAL_CASES[name]
    want, want_g = E.focal_reference(name)
    assert math.isfinite(float(want)) and bool(torch.isfinite(want_g).all())
    got, got_g = E.oracle(case, torch.float32)
    tol, rtol, atol = E.focal_tolerances(want, want_g)
    assert atol > 0
    loss_err = abs(float(got) - float(want)) / tol
    grad_err = float(((got_g.double() - want_g).abs() / (atol + rtol * want_g.abs())).max())
    print(f'{name}: float32 oracle at {loss_err:.3f} of the loss bound, {grad_err:.3f} of the gradient bound')
    assert loss_err <= 0.25 and grad_err <= 0.25


def test_case_table_covers_what_it_claims():
    shapes = {n: c['shape'] for n, c in E.FOCAL_CASES.items()}
    pixels = lambda s: s[0] * math.prod(s[2:])
    grid = [shapes[n] for n in E.names('grid')]
    assert all(pixels(s) == 132098 for s in grid) and 132098 > E.GRID and 132098 % E.BLOCK
    assert len(grid) == 8
    assert sorted(pixels(shapes[n]) for n in E.names('block')) == [255, 255, 256, 257, 64 * 511 + 1]
    assert {shapes[n][1] for n in E.names('classes')} == {1, 2, 7, 19}
    # the grid case is the largest input anywhere
    assert max(math.prod(s) for s in shapes.values()) == 132098 * 3
    counts = sorted({math.prod(shapes[n]) for n in E.names('float_targets') if 'functional' in n})
    assert counts == [1, 255, 257, 2 * E.GRID + 3]
    sat = [E.FOCAL_CASES[n]['kw'] for n in E.names('saturation')]
    assert {(k['gamma'], k['alpha'], k['reduction']) for k in sat} == {
        (g, a, r) for g in (0.0, 1.0, 1.5, 2.0, 3.0) for a in (None, 0.25, 0.9) for r in ('mean', 'sum')}
    assert {E.FOCAL_CASES[n]['kw']['gamma'] for n in E.names('small_gamma')} == {0.25, 0.5}
    for n in E.names('small_gamma'):
        assert float(E.focal_inputs(n)[0].abs().max()) <= 8.0


@pytest.mark.parametrize("name", E.names('labels'))
def test_label_cases_hold_the_labels_they_name(name):
    case = E.FOCAL_CASES[name]
    _, y = E.focal_inputs(name)
    C, ig, kind = case['shape'][1], case['kw']['ignore_index'], case['labels']
    assert y.dtype == getattr(torch, case['label_dtype'])
    if kind == 'some255':
        assert ig is None and int((y == 255).sum()) > 20 and int((y < C).sum()) > 20
    elif kind == 'neg_and_C':
        assert ig is None and int((y == -1).sum()) > 10 and int((y == C).sum()) > 10
    elif kind == 'half':
        frac = float((y == ig).float().mean())
        assert 0.4 <= frac <= 0.65, frac
        assert ig == 3 or not bool(((y >= 0) & (y < C) & (y == ig)).any())       # 255 and -100 are no class
    else:
        assert kind == 'all_but_one' and int((y != ig).sum()) == 1


def test_planted_values_meet_both_targets():
    for name in E.names('saturation'):
        case = E.FOCAL_CASES[name]
        x, _ = E.focal_inputs(name)
        right, wrong, t = E.planted_masks(case)
        for v in E.PLANTED:
            here = (x == v) & (torch.signbit(x) == (math.copysign(1.0, v) < 0))      # 0.0 and -0.0 apart
            assert int((here & t).sum()) >= 3 and int((here & ~t).sum()) >= 3, (name, v)
        assert int(right.sum()) > 20 and int(wrong.sum()) > 20
        # what "saturated" means to the oracle: no loss and no gradient where the prediction is right, +-w / divisor where wrong
        want, want_g = E.focal_reference(name)
        _, _, atol = E.focal_tolerances(want, want_g)
        kw = case['kw']
        div = float(x[:, 0].numel()) if kw['reduction'] == 'mean' else 1.0
        a = kw['alpha']
        w = torch.ones_like(want_g) if a is None else torch.where(t, a, 1 - a).double()
        assert float(want_g[right].abs().max()) <= atol
        torch.testing.assert_close(want_g[wrong], (torch.where(t, -w, w) / div)[wrong], rtol=2e-5, atol=atol)


@pytest.mark.parametrize("case", E.NOTHING_KEPT, ids=[c['name'] for c in E.NOTHING_KEPT])
def test_oracle_with_nothing_kept(case):
    """Written out by hand: boolean indexing keeps no element, the mean of nothing is NaN and no gradient is scattered back."""
    _, y = E.focal_inputs(case['name'])
    assert bool((y == case['kw']['ignore_index']).all())
    loss, grad = E.oracle(case, torch.float64)
    assert math.isnan(float(loss)) if case['kw']['reduction'] == 'mean' else float(loss) == 0.0
    assert bool((grad == 0).all())


def test_layouts_are_what_their_names_say():
    x = torch.arange(2 * 7 * 3 * 5, dtype=torch.float32).reshape(2, 7, 3, 5)
    for layout in ('nchw', 'nhwc_view', 'slice8', 'padded_rows'):
        assert torch.equal(E.to_layout(x, layout), x)
    assert E.to_layout(x, 'nhwc_view').stride() == (105, 1, 35, 7)
    s = E.to_layout(x, 'slice8')
    assert s.stride() == (120, 1, 40, 8) and s.stride(0) != 7 * 15 * s.stride(3)
    p = E.to_layout(x, 'padded_rows')
    assert p.stride(2) != p.stride(3) * p.shape[3]                 # the wrapper has to copy this one
    x5 = torch.zeros(2, 7, 3, 5, 7)
    st = E.to_layout(x5, 'nhwc_view').stride()
    assert st[1] == 1 and all(st[i] == st[i + 1] * x5.shape[i + 1] for i in range(2, 4))


# ----------------------------------------------------------------------------------------------- label downsample
@pytest.mark.parametrize("value", E.ONE_HOT_IDS)
def test_one_hot_blocks_reach_every_cell(value):
    img = E.one_hot_blocks(value)
    blocks = img[0, 0].reshape(8, 8, 8, 8).permute(0, 2, 1, 3).reshape(64, 64)       # [block, cell]
    assert torch.equal(blocks, torch.eye(64, dtype=torch.uint8) * value)
    assert bool((R.downsample_gt_semantic(img, 8) == value).all())


def test_ramp_blocks():
    imgs = E.ramp_blocks()
    first = lambda img: img[0, 0].reshape(2, 8, 4, 8)[:, 0, :, 0]
    last = lambda img: img[0, 0].reshape(2, 8, 4, 8)[:, 7, :, 7]
    assert torch.equal(first(imgs['descending']).long(), R.downsample_gt_semantic(imgs['descending'], 8)[0])
    assert torch.equal(last(imgs['ascending']).long(), R.downsample_gt_semantic(imgs['ascending'], 8)[0])
    for name in ('descending', 'ascending'):
        want = R.downsample_gt_semantic(imgs[name], 8)[0]
        assert sorted(set(want.flatten().tolist())) == [191, 255]
        assert int((imgs[name] == 255).sum()) == 4 and int((imgs[name] == 191).sum()) == 4    # unique inside a block
    assert bool((R.downsample_gt_semantic(imgs['equal'], 8) == 201).all()) and not bool(imgs['zero'].any())


def test_label_shapes_cover_the_factors_and_counts():
    cells = lambda s: s[0] * s[1] * (s[2] // s[4]) * (s[3] // s[4])
    assert {s[4] for s in E.LABEL_SHAPES} == {1, 2, 3, 4, 8, 16}
    assert {s[0] * s[1] for s in E.LABEL_SHAPES} >= {1, 3, 6}
    assert {255, 256, 257} <= {cells(s) for s in E.LABEL_SHAPES if s[4] == 8}
    assert any(s[3] == 8 and s[2] > 8 for s in E.LABEL_SHAPES) and any(s[2] == 8 and s[3] > 8 for s in E.LABEL_SHAPES)
    assert all(s[2] % s[4] == 0 and s[3] % s[4] == 0 for s in E.LABEL_SHAPES)
    m = E.random_mask((1, 1, 128, 128))
    assert int(m.max()) == 255 and int(m.min()) == 0


# ----------------------------------------------------------------------------------------------- upsample adjoint
@pytest.mark.parametrize("hw", E.PROBE_SHAPES)
def test_probe_adjoint_weights_are_exact_in_float32(hw):
    """Every tap weight is a product of two of {1, 3/4, 1/4}: the float64 adjoint of a one-hot map survives the cast."""
    H, W = hw
    dy = E.probes(H, W)
    _, dx = E.upsample_reference(torch.zeros(4 * H * W, H, W, 1, dtype=torch.float64), dy.double())
    assert torch.equal(dx.float().double(), dx)
    allowed = {a * b for a in (1.0, 0.75, 0.25) for b in (1.0, 0.75, 0.25)} | {0.0}
    assert set(dx.flatten().tolist()) <= allowed
    assert torch.equal(dx.sum(dim=(1, 2, 3)), torch.ones(4 * H * W, dtype=torch.float64))   # each row of up() sums to 1
    if H == 1 and W == 1:
        assert bool((dx == 1.0).all())
    _, dx32 = E.upsample_reference(torch.zeros(4 * H * W, H, W, 1), dy)
    assert torch.equal(dx32.double(), dx)


@pytest.mark.parametrize("shape", E.ADJOINT_SHAPES)
def test_adjoint_inputs_are_well_conditioned(shape):
    """float32 torch on the CPU meets a quarter of the GPU test's bounds on these inputs."""
    x, dy = E.adjoint_inputs(shape, positive=True)
    assert float(x.min()) >= 0.5 and float(dy.min()) >= 0.5
    y, dx = E.upsample_reference(x, dy)
    y64, dx64 = E.upsample_reference(x.double(), dy.double())
    assert E.adjoint_error(x, y64, dy, dx64) <= 1e-12
    err = E.adjoint_error(x, y, dy, dx)
    print(f'{shape}: float32 adjoint identity error {err:.2e}')
    assert err <= 0.25e-6
    x, dy = E.adjoint_inputs(shape)
    y, dx = E.upsample_reference(x, dy)
    y64, dx64 = E.upsample_reference(x.double(), dy.double())
    assert float(((dx.double() - dx64).abs() / (1e-6 + 1e-6 * dx64.abs())).max()) <= 0.25


def test_adjoint_shapes():
    sizes = [b * h * w * c for b, h, w, c in E.ADJOINT_SHAPES]
    assert 385 in sizes and 385 % E.BLOCK and any(c > E.BLOCK for *_, c in E.ADJOINT_SHAPES)
    assert (1, 1) in {(h, w) for _, h, w, _ in E.ADJOINT_SHAPES}


# ----------------------------------------------------------------------------------------------- add_mul_sigmoid adjoint
@pytest.mark.parametrize("n", E.GATE_COUNTS)
def test_gate_inputs(n):
    a, b, c, dy = E.gate_inputs(n)
    assert n % 4 == 0 and float((dy * b).abs().max()) <= 2.0
    if n >= 1020:
        assert all(int((c == v).sum()) == 3 for v in E.GATE_PLANTED)
    else:
        assert set(c.tolist()) == set(E.GATE_PLANTED[:4])
    s32 = torch.sigmoid(c)
    for v in E.GATE_SATURATED:
        assert bool(((s32[c == v] == 0) | (s32[c == v] == 1)).all())
    assert bool((((s32 == 0) | (s32 == 1)) == torch.isin(c, torch.tensor(E.GATE_SATURATED))).all())
    want = E.gate_reference(n)
    got = E.gate_reference(n, torch.float32)
    for g, w in zip(got, want):
        assert bool(torch.isfinite(w).all())
        assert float(((g.double() - w).abs() / (1e-6 + 1e-5 * w.abs())).max()) <= 0.25
    assert bool((got[2][torch.isin(c, torch.tensor(E.GATE_SATURATED))] == 0).all())
