"""The kernel-test shapes of the ViT training adjoints, shared by tests/test_vit_grad_cpu.py and tests/test_vit_grad_gpu.py, with their
seeded inputs and the float64 / float32 CPU runs of tests/vit_grad_ref.py (computed once per case and kept).

Seven map / window geometries, each with and without relative position and with and without padding tokens; head_dim, heads and
batch go round so that 32 / 64 / 80, 1..3 heads and batch 1 / 2 all occur with every geometry class:
  12 x 12, window 5     padding in both axes                      9 x 11, window 14   the window larger than the map
  12 x 12 global        144 keys: three 64-key steps, ragged      8 x 8 global        64 keys: the tile edge
  8 x 9 global          72 keys: one past the tile edge            1 x 1               one token
  3 x 4, window 1       twelve windows of one slot
"""
import functools

import torch

import vit_grad_ref as VG

GEOMETRIES = (
    ((12, 12), (5, 5)),
    ((9, 11), (14, 14)),
    ((12, 12), (12, 12)),
    ((8, 8), (8, 8)),
    ((8, 9), (8, 9)),
    ((1, 1), (1, 1)),
    ((3, 4), (1, 1)),
)
HEAD_DIMS = (32, 64, 80)


def _cases():
    out = []
    n = 0
    for gi, (hw, win) in enumerate(GEOMETRIES):
        for rel in (True, False):
            for pad in (True, False):
                out.append(dict(hw=hw, window=win, rel=rel, pad=pad, head_dim=HEAD_DIMS[n % 3], heads=1 + (n // 3 + gi) % 3, batch=1 + (n + gi) % 2))
                n += 1
    return tuple(out)


CASES = _cases()
IDS = tuple(f"{c['hw'][0]}x{c['hw'][1]}-w{c['window'][0]}x{c['window'][1]}-hd{c['head_dim']}x{c['heads']}-b{c['batch']}-"
            f"{'rel' if c['rel'] else 'norel'}-{'pad' if c['pad'] else 'nopad'}" for c in CASES)


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Float32 CPU tensors of case i: qkv, pad_qkv, rel_pos_h, rel_pos_w (None where the case has none), dout."""
    c = CASES[i]
    g = torch.Generator().manual_seed(1000 + i)
    ch = c['heads'] * c['head_dim']
    r = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s
    qkv = r(c['batch'], *c['hw'], 3 * ch)
    pad = r(3 * ch, s=0.5) if c['pad'] else None
    rh = r(2 * c['window'][0] - 1, c['head_dim'], s=0.2) if c['rel'] else None
    rw = r(2 * c['window'][1] - 1, c['head_dim'], s=0.2) if c['rel'] else None
    dout = r(c['batch'], *c['hw'], ch)
    return qkv, pad, rh, rw, dout


def _run(i, dtype):
    c = CASES[i]
    qkv, pad, rh, rw, dout = (None if t is None else t.to(dtype) for t in inputs(i))
    out, lse = VG.attention_forward(qkv, c['heads'], c['window'], pad, rh, rw)
    dqkv, dpad, drh, drw = VG.attention_backward(qkv, c['heads'], c['window'], pad, rh, rw, dout)
    return dict(out=out, lse=lse, dqkv=dqkv, dpad=dpad, drh=drh, drw=drw)


@functools.lru_cache(maxsize=None)
def reference(i):
    """Float64 run of the restatement: out, lse, dqkv, dpad, drh, drw."""
    return _run(i, torch.float64)


@functools.lru_cache(maxsize=None)
def bars(i):
    """Per tensor: 4 x the error of the restatement's own float32 CPU run, floored at 2^-21 max |value| (the summation orders of a
    kernel and of the CPU run differ: the margin of 4)."""
    want, f32 = reference(i), _run(i, torch.float32)
    return {k: bar(f32[k], v) for k, v in want.items() if v is not None}


def bar(f32_run, want):
    return max(4.0 * float((f32_run.double() - want).abs().max()), 2.0 ** -21 * float(want.abs().max()))
