"""Exact data, float64 references, guard-banded bf16 inputs and a CPU restatement of the tile decomposition for the fused bf16
CenterHead of csrc/head_bf16.hip (head_bf16_ws_kernel, head_bf16_kernel, head_bf16_pp_kernel; the f32-input and the bf16-input
entry).  Test helper, shared by tests/test_head_bf16_edges_cpu.py and tests/test_head_bf16_edges_gpu.py; imports without a GPU.

The kernel's contract: x, w1 and w2 are rounded to bf16 (nearest, ties to even); [3x3 64 -> 64] in fp32, folded BN and ReLU in
fp32; hidden pixels outside the image are zero; the hidden map is rounded to bf16 (ties to even); [3x3 64 -> c <= 4] in fp32
plus the bias.  The data below sits on dyadic grids chosen so that every partial sum of both layers, in any order, is a float32
number: the float64 evaluation of the contract IS the expected fp32 output, and the GPU tests compare with torch.equal.  The same
data has x values, w1 taps and hidden values that the roundings change, exact ties among them, so that a truncating or
tie-away rounding, or a rounding left out, changes outputs (test_head_bf16_edges_cpu.py shows each)."""
import functools

import torch
import torch.nn.functional as F

from wino_edges import BIG, GEOMS, NAMED, NAN, SENTINEL, GuardedOutput, _gen, _slack, gid, guarded_input  # noqa: F401  (re-exported)

COUNTS = (1, 4, 2, 3)          # every width a branch may have; total_out = 10, and with an odd H * W the planes of a batch's second
                               # image start at the other 16-byte alignment
TILE = 16                      # kTP of head_bf16.hip: output tile; the hidden tile is 18 x 18, the input patch 20 x 20
STORE = 4                      # pixels of one 16-byte store group
MAX_BRANCHES = 48              # kMaxBranches
X_UNIT = 1.0 / 16.0            # x = k / 16, |k| <= X_KMAX
X_KMAX = 520
HID_UNIT = 1.0 / 32.0          # X_UNIT x the smallest scale: the grid of the hidden map, rounded or not
TIE_TAP = 1.0 + 2.0 ** -8      # halfway between the bf16 neighbours 1 and 1 + 2^-7: ties-to-even gives 1
F32_WINDOWS = ((64, 0), (96, 16))      # (ld, coff) of the f32 input's channel window
BF16_WINDOWS = ((64, 0), (96, 24))     # bf16 input: ld and coff multiples of 8
KERNELS = (0, 1, 3)            # sgv3d_centerhead_bf16_select_plain: warp-specialised (default), single-role, ping-pong
BRANCH_GEOMS = [(1, 17, 17), (1, 1, 33)]          # the smallest maps that cross a tile seam, one each way
BRANCH_COUNTS = (1, 2, 3, MAX_BRANCHES)
TILE_GEOMS = [(1, 1, 1), (1, 16, 16), (1, 17, 17), (1, 13, 22), BIG]     # where the CPU tests run the restatement


def cycling_counts(nb):
    """Branch widths 1, 2, 3, 4, 1, ... for a head of nb branches."""
    return tuple(i % 4 + 1 for i in range(nb))


# ------------------------------------------------------------------------------------------------------------- bf16 roundings
def round_bf16(t, mode="rne"):
    """t (float32 numbers, any float dtype) rounded to bf16 by bit arithmetic, as float64.  'rne': nearest, ties to even (the
    contract; equals torch's .bfloat16(), which the CPU tests assert); 'away': nearest, ties away from zero; 'trunc': the low
    16 bits dropped; 'none': unchanged."""
    if mode == "none":
        return t.double()
    f = t.float().contiguous()
    assert bool((f.double() == t.double()).all()), "round_bf16 takes float32 numbers"
    bits = f.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if mode == "rne":
        bits = bits + 0x7FFF + ((bits >> 16) & 1)
    elif mode == "away":
        bits = bits + 0x8000
    else:
        assert mode == "trunc", mode
    bits = bits & 0xFFFF0000
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.view(torch.float32).double()


def changed_and_ties(t):
    """(share of the values of t that 'rne' changes, share that are exact ties: halfway between two bf16 numbers)."""
    lo, hi = round_bf16(t, "trunc"), round_bf16(t, "away")
    r = round_bf16(t, "rne")
    d = t.double()
    tie = (d != r) & ((d - lo).abs() * 2 == (hi - lo).abs()) & (hi != lo)
    return float((d != r).double().mean()), float(tie.double().mean())


# ------------------------------------------------------------------------------------------------------------------ the data
@functools.lru_cache(maxsize=None)
def params(counts=COUNTS):
    """w1 taps in {0, +-1, +-(1 + 2^-8)} at 5 % density, scales from {0.5, 1, 2}, shifts in quarters, w2 in {-1, 0, 1}, integer
    biases.  A zero-width branch has first-layer weights and no outputs."""
    nb, total = len(counts), sum(counts)
    g = _gen(61, nb, total)
    w1 = torch.randint(-1, 2, (nb * 64, 64, 3, 3), generator=g).double()
    w1 = w1 * (torch.rand(w1.shape, generator=g) < 0.075)                # 2 / 3 of them nonzero: 5 % of the taps
    w1 = torch.where(torch.rand(w1.shape, generator=g) < 0.5, w1, w1 * TIE_TAP).float()
    sc = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (nb * 64,), generator=g)]
    sh = torch.randint(-8, 9, (nb * 64,), generator=g).float() / 4.0
    w2 = torch.randint(-1, 2, (total, 64, 3, 3), generator=g).float()
    b2 = torch.randint(-3, 4, (total,), generator=g).float()
    return dict(counts=tuple(counts), w1=w1, sc=sc, sh=sh, w2=w2, b2=b2)


def without_branch(p, k):
    """The head of ``p`` without its zero-width branch k: the same weights for the others."""
    assert p["counts"][k] == 0
    keep = torch.cat([torch.arange(0, k * 64), torch.arange((k + 1) * 64, len(p["counts"]) * 64)])
    return dict(p, counts=p["counts"][:k] + p["counts"][k + 1:], w1=p["w1"][keep], sc=p["sc"][keep], sh=p["sh"][keep])


@functools.lru_cache(maxsize=None)
def head_x(geom):
    """x = k / 16, |k| <= 520, NHWC f32 [B, H, W, 64]: the input of the f32 entry; the bf16 entry gets it already rounded."""
    B, H, W = geom
    return torch.randint(-X_KMAX, X_KMAX + 1, (B, H, W, 64), generator=_gen(62, B, H, W)).float() * X_UNIT


def hidden_pre(x, p, x_round="rne", w1_round="rne"):
    """ReLU(BN(conv(x, w1))) on rounded operands, float64 NCHW [B, nb * 64, H, W]: the hidden map before its rounding."""
    y = F.conv2d(round_bf16(x, x_round).permute(0, 3, 1, 2), round_bf16(p["w1"], w1_round), padding=1)
    return (y * p["sc"].double()[None, :, None, None] + p["sh"].double()[None, :, None, None]).clamp_min(0)


def _layer2(hid, p, padding):
    out, off = [], 0
    w2 = round_bf16(p["w2"])
    for k, c in enumerate(p["counts"]):
        if c:
            out.append(F.conv2d(hid[:, k * 64:(k + 1) * 64], w2[off:off + c], p["b2"][off:off + c].double(), padding=padding))
        off += c
    return torch.cat(out, 1)


def head_ref(x, p, x_round="rne", w1_round="rne", hid_round="rne"):
    """The contract, on the whole map, float64: NCHW [B, sum(counts), H, W]."""
    return _layer2(round_bf16(hidden_pre(x, p, x_round, w1_round), hid_round), p, 1)


@functools.lru_cache(maxsize=None)
def head_case(geom, counts=COUNTS):
    """(x, the exact reference), computed once per process and left unchanged."""
    x = head_x(geom)
    return x, head_ref(x, params(counts))


def exactness(x, p):
    """The figures the exactness argument needs, for one input: every partial sum of layer 1 is a multiple of X_UNIT bounded by
    conv(|x|, |w1|), the pre-activation a multiple of HID_UNIT, every partial sum of layer 2 a multiple of HID_UNIT bounded by
    576 * max hidden * max |w2| (and by conv(hidden, |w2|), the sum with no cancellation)."""
    xr, w1r = round_bf16(x).permute(0, 3, 1, 2), round_bf16(p["w1"])
    pre = hidden_pre(x, p)
    hid = round_bf16(pre)
    pw = dict(p, w2=p["w2"].abs(), b2=torch.zeros_like(p["b2"]))
    return dict(
        x_on_grid=bool((xr / X_UNIT == (xr / X_UNIT).round()).all()),
        w1_rounded_is_ternary=bool(((w1r == 0) | (w1r.abs() == 1)).all()),
        l1_bound=float(F.conv2d(xr.abs(), w1r.abs(), padding=1).max()) / X_UNIT,
        bn_bound=float((F.conv2d(xr, w1r, padding=1).abs() * p["sc"].double()[None, :, None, None]
                        + p["sh"].double().abs()[None, :, None, None]).max()) / HID_UNIT,
        hid_on_grid=bool((pre / HID_UNIT == (pre / HID_UNIT).round()).all() and (hid / HID_UNIT == (hid / HID_UNIT).round()).all()),
        hid_max=float(hid.max()),
        l2_worst=576.0 * float(hid.max()) * float(p["w2"].abs().max()) / HID_UNIT,
        l2_bound=float(_layer2(hid, pw, 1).max()) / HID_UNIT,
        out_bound=(float(_layer2(hid, pw, 1).max()) + float(p["b2"].abs().max())) / HID_UNIT,
        hid_positive=float((pre > 0).double().mean()),
        hid_changed=changed_and_ties(pre[pre > 0]),
        x_changed=changed_and_ties(x),
        w1_changed=changed_and_ties(p["w1"][p["w1"] != 0]),
    )


def exact_in_f32(t):
    return bool((t.float().double() == t).all()) and float(t.abs().max()) < 2.0 ** 24


# ------------------------------------------------------------------------------------------------------------ guard bands
def guarded_input_bf16(x, ld, coff, device):
    """guarded_input's bf16 twin: x [B, H, W, C] (CPU, bf16 numbers) as channels [coff, coff + C) of a contiguous bf16 NHWC view
    [B, H, W, ld] inside one larger flat allocation, NaN in the slack before and after it and in every channel outside the
    window.  ld and coff are multiples of 8 (16 bytes), as the bf16 entry requires."""
    B, H, W, C = x.shape
    assert ld % 8 == 0 and coff % 8 == 0 and coff + C <= ld
    xb = x.bfloat16()
    assert bool((xb.double() == x.double()).all()), "the bf16 entry takes bf16 numbers"
    body = torch.full((B, H, W, ld), NAN, dtype=torch.bfloat16)
    body[..., coff:coff + C] = xb
    s = _slack(W, ld)
    flat = torch.full((body.numel() + 2 * s,), NAN, dtype=torch.bfloat16)
    flat[s:s + body.numel()] = body.reshape(-1)
    flat = flat.to(device)
    view = flat[s:s + body.numel()].view(B, H, W, ld)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


# ----------------------------------------------------------------------------------- the kernel's decomposition, restated (CPU)
# A workgroup owns a 16 x 16 tile at (y0, x0): it loads the 20 x 20 input patch around it (ZERO outside the image), computes the
# 18 x 18 hidden pixels (the tile and the one-pixel ring layer 2 reads) from it without padding, sets those OUTSIDE THE IMAGE TO
# ZERO -- layer 2 pads the hidden map with zeros, and a hidden pixel computed from an all-zero patch is ReLU(shift), not zero --,
# rounds them to bf16 and runs a valid 3x3 on them.  Every tile recomputes its ring, so the zeroing acts at every image border,
# that of a 16 x 16 map included.
def head_by_tiles(x, p, zero_outside=True, hid_round="rne", x_round="rne", w1_round="rne"):
    B, H, W, _ = x.shape
    xr = round_bf16(x, x_round).permute(0, 3, 1, 2)
    w1r = round_bf16(p["w1"], w1_round)
    sc, sh = p["sc"].double()[None, :, None, None], p["sh"].double()[None, :, None, None]
    ty, tx = -(-H // TILE), -(-W // TILE)
    xp = F.pad(xr, (2, tx * TILE - W + 2, 2, ty * TILE - H + 2))          # patch pixel (iy, ix) of tile (y0, x0): xp[y0 + iy, x0 + ix]
    out = torch.zeros(B, sum(p["counts"]), ty * TILE, tx * TILE, dtype=torch.float64)
    for y0 in range(0, ty * TILE, TILE):
        for x0 in range(0, tx * TILE, TILE):
            patch = xp[:, :, y0:y0 + TILE + 4, x0:x0 + TILE + 4]
            hid = (F.conv2d(patch, w1r) * sc + sh).clamp_min(0)           # 18 x 18: hidden pixel (hy, hx) is image pixel (y0 - 1 + hy, ..)
            if zero_outside:
                gy = torch.arange(y0 - 1, y0 + TILE + 1)
                gx = torch.arange(x0 - 1, x0 + TILE + 1)
                inside = ((gy >= 0) & (gy < H))[:, None] & ((gx >= 0) & (gx < W))[None, :]
                hid = hid * inside
            out[:, :, y0:y0 + TILE, x0:x0 + TILE] = _layer2(round_bf16(hid, hid_round), p, 0)
    return out[:, :, :H, :W]
