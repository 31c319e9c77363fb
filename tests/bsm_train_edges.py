"""Input generators and case tables for the edge-shape tests of csrc/bsm_train.hip (test helper, shared by
tests/test_bsm_train_edges_cpu.py and tests/test_bsm_train_edges_gpu.py): the one-pass focal loss, the block-max label
downsample, the adjoint of the x2 bilinear upsample and the adjoint of ``a + b * sigmoid(c)``.

Everything here runs on the CPU (torch generators with fixed seeds); the float64 references come from oracle/focal_ref.py
and from autograd, are computed once per case and are never modified.  The launch constants of the kernels are restated
(``BLOCK``, ``FOCAL_BLOCKS``) so that a case can say which boundary it sits on."""
import functools
import itertools

import torch
import torch.nn.functional as F

from oracle import focal_ref as R

BLOCK = 256                      # threads per block of every kernel in bsm_train.hip
FOCAL_BLOCKS = 512               # blocks of focal_kernel / focal_count_kernel: one grid trip covers 131072 pixels
GRID = BLOCK * FOCAL_BLOCKS
GUARD = 7.5                      # fill of storage a kernel must not write


# =============================================================================================== focal loss
def focal_tolerances(want_loss, want_grad):
    """(loss bound, gradient rtol, gradient atol) of tests/test_bsm_train_gpu.py::test_focal_loss_matches_reference_golden."""
    return 1e-5 * max(1.0, abs(float(want_loss))), 2e-5, 2e-6 * float(want_grad.abs().max())


PLANTED = (30.0, -30.0, 88.0, -88.0, 1e4, -1e4, 0.0, -0.0)


def _case(name, shape, mode='multiclass', logits='wide', labels='uniform', label_dtype='int64', layout='nchw',
          alpha=0.25, gamma=2.0, ignore_index=None, reduction='mean', seed=0):
    return dict(name=name, shape=tuple(shape), mode=mode, logits=logits, labels=labels, label_dtype=label_dtype,
                layout=layout, seed=seed, kw=dict(alpha=alpha, gamma=gamma, ignore_index=ignore_index, reduction=reduction))


def _grid_cases():
    """1. 2 x 257 x 257 = 132098 pixels: one more trip of the grid-stride loop for 1026 of them, a ragged last block."""
    return [_case(f'grid-{dt}-{lay}-{red}', (2, 3, 257, 257), label_dtype=dt, layout=lay, reduction=red, seed=1)
            for dt in ('uint8', 'int64') for lay in ('nchw', 'nhwc_view') for red in ('mean', 'sum')]


def _block_cases():
    """2. pixel counts on both sides of one block, 64 * 511 + 1 pixels in one row, and 3 x 85 where the sample index changes
    inside a wave."""
    out = [_case(f'block-{p}', (1, 7, 1, p), label_dtype='uint8', layout='nhwc_view', seed=2) for p in (255, 256, 257, 64 * 511 + 1)]
    out.append(_case('block-3x85', (3, 7, 5, 17), label_dtype='uint8', layout='nhwc_view', seed=3))
    return out


def _class_cases():
    """3. class counts and storage geometries."""
    out = [_case(f'classes-{c}-{lay}', (2, c, 9, 13), layout=lay, seed=4 + c) for c in (1, 2, 7, 19) for lay in ('nchw', 'nhwc_view')]
    out.append(_case('slice7of8', (2, 7, 9, 13), layout='slice8', label_dtype='uint8', seed=30))
    out.append(_case('two-dim', (37, 7), seed=31))
    out.append(_case('five-dim-joint', (2, 7, 3, 5, 7), layout='nhwc_view', seed=32))
    out.append(_case('five-dim-split', (2, 7, 3, 5, 7), layout='padded_rows', seed=33))
    return out


def _label_cases():
    """4. labels outside [0, classes), the three ignore_index values, half and all but one pixel ignored."""
    out = [_case('uint8-255-no-ignore', (2, 7, 9, 13), labels='some255', label_dtype='uint8', seed=40),
           _case('int64-neg-and-C-no-ignore', (2, 7, 9, 13), labels='neg_and_C', seed=41)]
    for red in ('mean', 'sum'):
        for frac in ('half', 'all_but_one'):
            out.append(_case(f'ignore255-{frac}-{red}', (2, 7, 9, 13), labels=frac, label_dtype='uint8', ignore_index=255,
                             reduction=red, layout='nhwc_view', seed=42))
            out.append(_case(f'ignore-100-{frac}-{red}', (2, 7, 9, 13), labels=frac, ignore_index=-100, reduction=red, seed=43))
            out.append(_case(f'ignore3-{frac}-{red}', (2, 7, 9, 13), labels=frac, ignore_index=3, reduction=red,
                             layout='nhwc_view', seed=44))
    return out


def _saturation_cases():
    """6. 22 copies of every planted value among 528 logits; over 3 uniformly drawn classes each value meets targets of 1 and
    of 0 (the CPU file checks that it does)."""
    return [_case(f'sat-g{g}-a{a}-{red}', (2, 3, 8, 11), logits='planted', gamma=g, alpha=a, reduction=red, label_dtype='uint8',
                  layout='nhwc_view', seed=50)
            for g in (0.0, 1.0, 1.5, 2.0, 3.0) for a in (None, 0.25, 0.9) for red in ('mean', 'sum')]


def _small_gamma_cases():
    """7. gamma below 1 at |logit| <= 8 (see test_focal_gamma_below_one of the GPU file for why)."""
    return [_case(f'gamma{g}-a{a}-{red}', (2, 7, 9, 13), logits='capped8', gamma=g, alpha=a, reduction=red, seed=60)
            for g in (0.25, 0.5) for a in (None, 0.25) for red in ('mean', 'sum')]


def _float_target_cases():
    """8. target_kind 2 through the three wrappers; element counts on both sides of a block and past two grid trips."""
    out = []
    for n in (1, 255, 257, 2 * GRID + 3):
        # a lone element is its own max|gradient|, which makes the bound a relative one: it gets a randn-sized logit, where
        # 1 - pt does not cancel
        wide = 'unit' if n == 1 else 'wide'
        out.append(_case(f'functional-soft-{n}', (n,), mode='functional', logits=wide, labels='soft', reduction='mean', seed=70))
        out.append(_case(f'binary-hard-{n}', (1, 1, 1, n), mode='binary', logits=wide, labels='hard',
                         reduction='sum' if n == 257 else 'mean', seed=71))
    out.append(_case('multilabel-soft', (2, 5, 3, 17), mode='multilabel', labels='soft', gamma=1.5, alpha=None, seed=72))
    out.append(_case('multilabel-hard-sum', (2, 5, 3, 17), mode='multilabel', labels='hard', reduction='sum', layout='nhwc_view', seed=73))
    out.append(_case('binary-ignore255', (3, 1, 5, 17), mode='binary', labels='hard_ignore', ignore_index=255, seed=74))
    out.append(_case('multilabel-ignore-1', (2, 5, 3, 17), mode='multilabel', labels='hard_ignore', ignore_index=-1, reduction='sum', seed=75))
    return out


FOCAL_GROUPS = {
    'grid': _grid_cases(), 'block': _block_cases(), 'classes': _class_cases(), 'labels': _label_cases(),
    'saturation': _saturation_cases(), 'small_gamma': _small_gamma_cases(), 'float_targets': _float_target_cases(),
}
FOCAL_CASES = {c['name']: c for group in FOCAL_GROUPS.values() for c in group}
assert len(FOCAL_CASES) == sum(len(g) for g in FOCAL_GROUPS.values())

# 5. nothing kept: the expected values are written out by hand (loss NaN for 'mean', 0 for 'sum'; gradient all zero)
NOTHING_KEPT = [_case(f'nothing-kept-{dt}-{red}', (2, 7, 9, 13), labels='all', label_dtype=dt, ignore_index=ig, reduction=red,
                      layout='nhwc_view', seed=80)
                for dt, ig in (('uint8', 255), ('int64', -100)) for red in ('mean', 'sum')]


def names(group):
    return [c['name'] for c in FOCAL_GROUPS[group]]


def _logits(case, g):
    shape, kind = case['shape'], case['logits']
    x = 6.0 * torch.randn(shape, generator=g)
    if kind == 'unit':
        x = x / 6.0
    elif kind == 'capped8':
        x = x.clamp(-8.0, 8.0)
    elif kind == 'planted':
        n = x.numel()
        reps = n // (3 * len(PLANTED))                     # a third of the logits are planted values
        where = torch.randperm(n, generator=g)[:reps * len(PLANTED)]
        x.view(-1)[where] = torch.tensor(PLANTED).repeat(reps)
    else:
        assert kind == 'wide'
    return x


def _labels(case, g):
    shape, kind, kw = case['shape'], case['labels'], case['kw']
    ig = kw['ignore_index']
    if case['mode'] != 'multiclass':
        if kind == 'soft':
            return torch.rand(shape, generator=g).clamp(0.01, 0.99)
        y = torch.randint(0, 2, shape, generator=g)
        if kind == 'hard_ignore':
            y[torch.rand(shape, generator=g) < 0.4] = ig
            y = y.reshape((shape[0],) + shape[2:]) if case['mode'] == 'binary' else y
            return y                                        # integer targets: the wrapper masks, then casts
        assert kind == 'hard'
        return y.float()
    C = shape[1]
    sp = (shape[0],) + shape[2:]
    y = torch.randint(0, C, sp, generator=g)
    u = torch.rand(sp, generator=g)
    if kind == 'some255':
        y[u < 0.3] = 255
    elif kind == 'neg_and_C':
        y[u < 0.2] = -1
        y[u > 0.8] = C
    elif kind == 'half':
        y[u < 0.45] = ig
    elif kind == 'all_but_one':
        keep = int(torch.randint(0, y.numel(), (1,), generator=g))
        val = int(y.view(-1)[keep]) if int(y.view(-1)[keep]) != ig else 0
        y.fill_(ig)
        y.view(-1)[keep] = val
    elif kind == 'all':
        y.fill_(ig)
    else:
        assert kind == 'uniform'
    return y.to(getattr(torch, case['label_dtype']))


@functools.lru_cache(maxsize=None)
def focal_inputs(name):
    """(logits float32 in logical [N, C, *spatial] order, targets) of a case; shared, never modified."""
    case = FOCAL_CASES.get(name) or {c['name']: c for c in NOTHING_KEPT}[name]
    g = torch.Generator().manual_seed(1000 + case['seed'])
    return _logits(case, g), _labels(case, g)


def oracle(case, dtype):
    """(loss, gradient) of oracle/focal_ref.py evaluated in ``dtype``."""
    x, y = focal_inputs(case['name'])
    x = x.detach().clone().to(dtype).requires_grad_(True)
    y = y.to(dtype) if y.dtype.is_floating_point else y.long()
    kw = case['kw']
    if case['mode'] == 'functional':
        loss = R.focal_loss_with_logits(x, y, kw['gamma'], kw['alpha'], kw['reduction'])
    else:
        loss = R.focal_loss(x, y, case['mode'], kw['alpha'], kw['gamma'], kw['ignore_index'], kw['reduction'])
    loss.backward()
    return loss.detach(), x.grad


@functools.lru_cache(maxsize=None)
def focal_reference(name):
    """float64 (loss, gradient) of a case of FOCAL_CASES; shared, never modified."""
    return oracle(FOCAL_CASES[name], torch.float64)


def to_layout(x, layout):
    """The logical tensor ``x`` [N, C, *spatial] in one of the storage geometries the training forward (or a caller) hands out."""
    if layout == 'nchw' or x.dim() < 3:
        return x.contiguous()
    if layout == 'nhwc_view':                               # channel-last storage, NCHW view
        return x.movedim(1, -1).contiguous().movedim(-1, 1)
    if layout == 'slice8':                                  # 7 of the 8 channels of a channel-last buffer: sb != C * P * sp
        assert x.shape[1] == 7
        buf = x.new_full((x.shape[0],) + tuple(x.shape[2:]) + (8,), GUARD)
        buf[..., :7] = x.movedim(1, -1)
        return buf[..., :7].movedim(-1, 1)
    if layout == 'padded_rows':                             # rows one element longer than W: spatial dims not jointly contiguous
        buf = x.new_full(tuple(x.shape[:-1]) + (x.shape[-1] + 1,), GUARD)
        buf[..., :-1] = x
        return buf[..., :-1]
    raise ValueError(layout)


def planted_masks(case):
    """(saturated and correct, saturated and wrong, target) over the logits of a multiclass 'planted' case: |x| >= 30 with the
    sign of the logit agreeing / disagreeing with the one-hot target of a kept pixel."""
    x, y = focal_inputs(case['name'])
    t = F.one_hot(y.long(), x.shape[1]).movedim(-1, 1).bool()
    big = x.abs() >= 30
    return big & ((x > 0) == t), big & ((x > 0) != t), t


# =============================================================================================== label downsample
ONE_HOT_IDS = (1, 127, 128, 255)


def one_hot_blocks(value):
    """[1, 1, 64, 64] uint8, all zero but one cell per 8x8 block: block k (row-major over the 8 x 8 blocks) holds ``value`` at
    its cell k (row k // 8, column k % 8), so every byte lane of every row of the fast path decides one output."""
    img = torch.zeros(1, 1, 64, 64, dtype=torch.uint8)
    for k in range(64):
        img[0, 0, 8 * (k // 8) + k // 8, 8 * (k % 8) + k % 8] = value
    return img


def ramp_blocks():
    """{name: [1, 1, 16, 32] uint8}: per 8x8 block a descending ramp (maximum first), an ascending one (maximum last), one value
    throughout and zeros.  The ramps run 192..255 and, in every other block, 128..191: the maximum of a block is unique, above
    127 and differs from its neighbours'."""
    asc = (192 + torch.arange(64)).reshape(8, 8).to(torch.uint8)
    blocks = {'descending': asc.flip(0, 1), 'ascending': asc, 'equal': torch.full((8, 8), 201, dtype=torch.uint8),
              'zero': torch.zeros(8, 8, dtype=torch.uint8)}
    imgs = {}
    for name, blk in blocks.items():
        img = torch.zeros(1, 1, 16, 32, dtype=torch.uint8)
        for by, bx in itertools.product(range(2), range(4)):
            low = (by + bx) % 2 == 1 and name in ('descending', 'ascending')
            img[0, 0, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = blk - 64 if low else blk
        imgs[name] = img
    return imgs


# (B, N, H, W, factor): the generic path at every other factor, sample counts, output cell counts on both sides of a block
# (15 x 17 = 255, 16 x 16, 1 x 257; 3 x 5 x 17 = 255 across samples), one block wide and one block high
LABEL_SHAPES = (
    (1, 1, 9, 14, 1), (2, 1, 10, 18, 2), (1, 2, 24, 36, 4), (1, 1, 32, 80, 16), (1, 3, 15, 21, 3), (1, 1, 48, 3 * 259, 3),
    (1, 1, 120, 136, 8), (1, 1, 128, 128, 8), (1, 1, 8, 2056, 8), (3, 1, 40, 136, 8), (2, 3, 16, 24, 8), (1, 6, 4 * 43, 4 * 6, 4),
    (1, 1, 72, 8, 8), (1, 1, 8, 72, 8), (1, 1, 8, 8, 8),
)


def random_mask(shape, seed=0):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(2000 + seed), dtype=torch.uint8)


# =============================================================================================== upsample adjoint
PROBE_SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 4))
# (B, H, W, C): one pixel, one row, one column, 385 elements (two blocks, ragged tail), 12480 elements with C > one block
ADJOINT_SHAPES = ((1, 1, 1, 7), (2, 1, 5, 8), (2, 6, 1, 3), (1, 5, 11, 7), (3, 4, 4, 260))


def probes(H, W):
    """[4HW, 2H, 2W, 1] float32: sample k is 1 at position k of the output map and 0 elsewhere."""
    n = 4 * H * W
    return torch.eye(n).reshape(n, 2 * H, 2 * W, 1)


def upsample_reference(x, dy):
    """(up(x), upT(dy)) of NHWC float tensors through F.interpolate and autograd in the tensors' own dtype."""
    xr = x.permute(0, 3, 1, 2).detach().clone().requires_grad_(True)
    y = F.interpolate(xr, scale_factor=2, mode='bilinear')
    y.backward(dy.permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1)


def adjoint_inputs(shape, positive=False):
    """(x, dy) for a shape of ADJOINT_SHAPES.  ``positive``: 0.5 + |randn|, for the adjoint identity -- every tap weight is
    positive, so neither inner product cancels and its relative error measures the kernels, not the draw."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(3000 + B * H * W * C)
    x, dy = torch.randn(B, H, W, C, generator=g), torch.randn(B, 2 * H, 2 * W, C, generator=g)
    return (x.abs() + 0.5, dy.abs() + 0.5) if positive else (x, dy)


def adjoint_error(x, y, dy, dx):
    """| <up(x), dy> - <x, upT(dy)> | relative to the larger of the two, accumulated in float64."""
    lhs = float((y.double() * dy.double()).sum())
    rhs = float((x.double() * dx.double()).sum())
    return abs(lhs - rhs) / max(abs(lhs), abs(rhs))


# =============================================================================================== add_mul_sigmoid adjoint
GATE_COUNTS = (4, 1020, 1024, 1028, 4 * 257 * 3)          # one float4; around one block of float4; three blocks and a tail
GATE_PLANTED = (20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 0.0)
# float32 sigmoid is exactly 1 from c = 17.4 up (exp(-c) < 2^-25) and exactly 0 where exp(-c) overflows (c < -88.73)
GATE_SATURATED = (20.0, 88.0, 104.0, -104.0)


def gate_inputs(n):
    """(a, b, c, dy) float32 [n]; c = 3 * randn with the planted values at fixed random places (all of them from n = 1020 up).
    b and dy are randn clamped to [-2, 2] and halved for dy, so |dy * b| <= 2: float32 resolves s * (1 - s) to about one ulp of
    1 (1.2e-7) near s = 1, which dc = dy * b * s * (1 - s) scales by |dy * b|, and the absolute bound of the test is 1e-6."""
    g = torch.Generator().manual_seed(4000 + n)
    a, b, dy = (torch.randn(n, generator=g).clamp(-2.0, 2.0) for _ in range(3))
    dy = 0.5 * dy
    c = 3.0 * torch.randn(n, generator=g)
    k = min(n, len(GATE_PLANTED) * (3 if n > 16 else 1))
    where = torch.randperm(n, generator=g)[:k]
    c[where] = torch.tensor(GATE_PLANTED).repeat(3)[:k]
    return a, b, c, dy


def gate_reference(n, dtype=torch.float64):
    a, b, c, dy = gate_inputs(n)
    ref = [t.to(dtype).requires_grad_(True) for t in (a, b, c)]
    (ref[0] + ref[1] * torch.sigmoid(ref[2])).backward(dy.to(dtype))
    return [r.grad for r in ref]
