"""Edge geometries, guard-banded buffers, exact data and float64 references for the Winograd kernels (test helper, shared by
tests/test_wino_edges_cpu.py and tests/test_wino_edges_gpu.py): csrc/head_wino4.hip (head_wino4_kernel, conv_f4res_kernel),
csrc/conv_wino4.hip (the three-launch F(4x4)), csrc/conv_wino.hip (the F(2x2) kernels, conv_wino_head_kernel and
head_ring_fixup_kernel).  The last part restates the fused heads' decomposition into 16x16 blocks and the ring fix-up's index
map on the CPU, so that the CPU tests can say which geometry reaches which line of it."""
import functools

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------------------- geometries
# (batch, H, W).  The sweep: every size 1..33 once as height and once as width (7 and 33 are coprime: a permutation), so every
# remainder mod 4 (tiles) and mod 16 (blocks) occurs in both dimensions on single-block maps (1..16) and on two- and
# three-block maps (17..33); sizes 1, 2, 3 are smaller than one tile.
SWEEP = [(1, i, ((i - 1) * 7 + 3) % 33 + 1) for i in range(1, 34)]
NAMED = [(1, 1, 1), (1, 1, 33), (1, 33, 1), (1, 16, 16), (1, 17, 17)]
BIG = (2, 35, 49)          # batch 2, 3 x 4 blocks: an interior block with eight neighbours, ragged on both edges
GEOMS = list(dict.fromkeys(SWEEP + NAMED + [BIG]))         # (1, 17, 17) is the sweep's i = 17 as well: listed once
SMALL3 = [(1, 1, 1), (1, 7, 19), BIG]                      # the maps every F(4x4) tile id runs on
DILATED = [(1, 7, 19), (1, 19, 7)]                         # pad = dil = 2: sub-grids of 4 / 3 rows and 10 / 9 columns, and swapped
COUNTS = (3, 5)                                            # outputs of the two head branches: one wider than four


def gid(g):
    return "x".join(str(v) for v in g)


# ------------------------------------------------------------------------------------------------------------ guard bands
NAN = float("nan")
SENTINEL = -777.0


def _slack(w, ld):
    """One full map row plus one pixel, in floats; a multiple of 4 (16 bytes) when ld is."""
    return (w + 1) * ld


def guarded_input(x, ld, coff, device, finite=None):
    """x [B, H, W, C] (CPU f32) as channels [coff, coff + C) of a contiguous NHWC view [B, H, W, ld] inside one larger flat
    allocation: NaN in the slack before and after it and in every channel outside the window.  ``finite``: (first channel,
    value) -- the window's channels from there on hold ``value`` (padded channels the kernel reads against zero weights)."""
    B, H, W, C = x.shape
    assert ld % 4 == 0 and coff % 4 == 0 and coff + C <= ld
    body = torch.full((B, H, W, ld), NAN)
    body[..., coff:coff + C] = x
    if finite is not None:
        body[..., coff + finite[0]:coff + C] = finite[1]
    s = _slack(W, ld)
    flat = torch.full((body.numel() + 2 * s,), NAN)
    flat[s:s + body.numel()] = body.reshape(-1)
    flat = flat.to(device)
    view = flat[s:s + body.numel()].view(B, H, W, ld)
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return view


class GuardedOutput:
    """A contiguous tensor of ``shape`` inside a larger flat allocation filled with SENTINEL.  ``row``: floats of one map row
    plus one pixel (the slack on either side, rounded up to 16 bytes)."""

    def __init__(self, shape, row, device):
        n = 1
        for v in shape:
            n *= int(v)
        self.slack = (row + 3) // 4 * 4
        self.flat = torch.full((n + 2 * self.slack,), SENTINEL, device=device)
        self.view = self.flat[self.slack:self.slack + n].view(*shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0

    def result(self, window=None):
        """(the written part on the CPU as float64, whether everything else still holds the sentinel).  ``window``: the
        channel slice (start, count) of the last dimension the kernel was to write; None: the whole view."""
        flat = self.flat.cpu()
        body = flat[self.slack:flat.numel() - self.slack].view(*self.view.shape)
        intact = bool((flat[:self.slack] == SENTINEL).all()) and bool((flat[flat.numel() - self.slack:] == SENTINEL).all())
        if window is None:
            return body.double(), intact
        c0, n = window
        intact = intact and bool((body[..., :c0] == SENTINEL).all()) and bool((body[..., c0 + n:] == SENTINEL).all())
        return body[..., c0:c0 + n].double(), intact


# ------------------------------------------------------------------------------------------- exact data and float64 references
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1009 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def conv64(x, w, pad=1, dil=1):
    """x NHWC, w OIHW -> NHWC, float64 on the CPU."""
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), padding=pad, dilation=dil).permute(0, 2, 3, 1)


def epilogue64(y, scale=None, shift=None, residual=None, relu=False):
    if scale is not None:
        y = y * scale.double() + shift.double()
    if residual is not None:
        y = y + residual.double()
    return y.clamp_min(0) if relu else y


def head_ref(x, p):
    """[3x3 cin -> 64 + BN + ReLU] then [3x3 64 -> c + bias] per branch, float64: NCHW [B, sum(counts), H, W]."""
    hid = hidden64(x, p)
    out, off = [], 0
    for k, c in enumerate(p["counts"]):
        out.append(F.conv2d(hid[:, k * 64:(k + 1) * 64], p["w2"][off:off + c].double(), p["b2"][off:off + c].double(), padding=1))
        off += c
    return torch.cat(out, 1)


def hidden64(x, p):
    y = F.conv2d(x.permute(0, 3, 1, 2).double(), p["w1"].double(), padding=1)
    return (y * p["sc"].double()[None, :, None, None] + p["sh"].double()[None, :, None, None]).clamp_min(0)


def sparse576(g, cout, cin, density=0.08):
    """Taps in {-1, 0, 1} x 576 = 24^2 (G's entries are k / 24: G g G^T is then integer), whole (cout, cin) kernels kept with
    probability ``density`` so that every sum of the F(4x4) path stays far below 2^24."""
    w = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float() * 576.0
    return w * (torch.rand(cout, cin, 1, 1, generator=g) < density)


@functools.lru_cache(maxsize=None)
def head_f4_params(counts=COUNTS):
    """The data of test_fused_centerhead_f4_exact_on_small_integers: w1 in {-1, 0, 1} x 576 at 8 % density, scale 1 / 64 (the
    hidden map is 9 k + shift, exactly), integer shifts, w2 and b2."""
    g = _gen(41, 0)
    nb, total = len(counts), sum(counts)
    return dict(counts=counts, w1=sparse576(g, nb * 64, 64), sc=torch.full((nb * 64,), 1.0 / 64.0),
                sh=torch.randint(-2, 3, (nb * 64,), generator=g).float(),
                w2=torch.randint(-2, 3, (total, 64, 3, 3), generator=g).float(),
                b2=torch.randint(-3, 4, (total,), generator=g).float())


@functools.lru_cache(maxsize=None)
def head_f2_params(counts=COUNTS):
    """Integer w1, w2, b2 and shifts, scale 1 / 4: the F(2x2) transforms have halves and quarters only, so every intermediate
    of conv_wino_head_kernel is a multiple of 1 / 4 below 2^24."""
    g = _gen(42, 0)
    nb, total = len(counts), sum(counts)
    return dict(counts=counts, w1=torch.randint(-2, 3, (nb * 64, 64, 3, 3), generator=g).float(),
                sc=torch.full((nb * 64,), 0.25), sh=torch.randint(-2, 3, (nb * 64,), generator=g).float(),
                w2=torch.randint(-2, 3, (total, 64, 3, 3), generator=g).float(),
                b2=torch.randint(-3, 4, (total,), generator=g).float())


def head_input(geom, lo, hi, tag):
    B, H, W = geom
    return torch.randint(lo, hi + 1, (B, H, W, 64), generator=_gen(tag, B, H, W)).float()


@functools.lru_cache(maxsize=None)
def head_f4_case(geom):
    x = head_input(geom, -2, 2, 43)
    return x, head_ref(x, head_f4_params())


@functools.lru_cache(maxsize=None)
def head_f2_case(geom):
    x = head_input(geom, -3, 3, 44)
    return x, head_ref(x, head_f2_params())


F4RES_LAYERS = {"64to64": (64, 64, 64), "64to128": (64, 64, 128), "128to64": (128, 120, 64)}     # (cin padded, cin real, cout)


@functools.lru_cache(maxsize=None)
def f4res_params(name):
    """The head's exact construction (the packer is the same h4_pack_kernel) with BN, for conv_f4res_kernel."""
    cin, cin_real, cout = F4RES_LAYERS[name]
    g = _gen(45, cin, cout)
    return dict(cin=cin, cin_real=cin_real, cout=cout, w=sparse576(g, cout, cin_real), sc=torch.full((cout,), 1.0 / 64.0),
                sh=torch.randint(-2, 3, (cout,), generator=g).float())


@functools.lru_cache(maxsize=None)
def f4res_case(name, geom):
    """(x [B, H, W, cin real], integer residual, float64 reference of conv + BN + residual + ReLU)."""
    p = f4res_params(name)
    B, H, W = geom
    g = _gen(46, B, H, W, p["cin"])
    x = torch.randint(-2, 3, (B, H, W, p["cin_real"]), generator=g).float()
    res = torch.randint(-3, 4, (B, H, W, p["cout"]), generator=g).float()
    return x, res, epilogue64(conv64(x, p["w"]), p["sc"], p["sh"], res, relu=True)


@functools.lru_cache(maxsize=None)
def wino4_params():
    """The data of test_winograd_f4x4_x3_keeps_every_partial_product, 128 -> 128, with a folded BN."""
    g = _gen(47, 0)
    return dict(w=torch.randint(-1, 2, (128, 128, 3, 3), generator=g).float() * 576.0,
                sc=torch.rand(128, generator=g) * 0.5 + 0.5, sh=torch.randn(128, generator=g) * 2304.0)


@functools.lru_cache(maxsize=None)
def wino4_case(geom, dil=1):
    """(x in {-1, 0, 1}, float64 reference of conv + BN + ReLU, S = max conv(|x|, |w|): the scale of the products with no
    cancellation, which a one-pixel map has as well)."""
    p = wino4_params()
    B, H, W = geom
    x = torch.randint(-1, 2, (B, H, W, 128), generator=_gen(48, B, H, W, dil)).float()
    ref = epilogue64(conv64(x, p["w"], pad=dil, dil=dil), p["sc"], p["sh"], relu=True)
    return x, ref, float(conv64(x.abs(), p["w"].abs(), pad=dil, dil=dil).max())


@functools.lru_cache(maxsize=None)
def wino2_weight():
    """The integer data of test_conv_wino_gpu._mk(..., integer=True), 32 -> 72."""
    return torch.randint(-2, 3, (72, 32, 3, 3), generator=_gen(49, 0)).float()


@functools.lru_cache(maxsize=None)
def wino2_case(geom):
    B, H, W = geom
    x = torch.randint(-3, 4, (B, H, W, 32), generator=_gen(50, B, H, W)).float()
    return x, conv64(x, wino2_weight())


def exact_in_f32(t):
    """Every value is a float32 number and below 2^24 in magnitude: bit equality with a float32 result then means something."""
    return bool((t.float().double() == t).all()) and float(t.abs().max()) < 2.0 ** 24


# ---------------------------------------------------------------------------- F(4x4, 3x3) restated: how large the intermediates get
_BT = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
_G = torch.tensor([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=torch.float64)     # 24 G
_AT = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)


def f4_intermediates(x, w):
    """F(4x4, 3x3) of x NHWC with w OIHW in float64, tile by tile as the kernels compute it: (the convolution NHWC, whether U is
    integer, a bound on every partial sum of the position GEMMs, a bound on every partial sum of A^T M A)."""
    B, H, W, C = x.shape
    ty, tx = -(-H // 4), -(-W // 4)
    xp = F.pad(x.permute(0, 3, 1, 2).double(), (1, 4 * tx - W + 1, 1, 4 * ty - H + 1))
    d = F.unfold(xp, 6, stride=4).view(B, C, 6, 6, ty * tx)                      # [B, C, 6, 6, tiles]
    V = torch.einsum("ij,bcjkt,lk->bcilt", _BT, d, _BT)
    U = torch.einsum("ij,ocjk,lk->ocil", _G, w.double(), _G) / 576.0
    M = torch.einsum("bcilt,ocil->boilt", V, U)
    acc_bound = float(torch.einsum("bcilt,ocil->boilt", V.abs(), U.abs()).max())
    y = torch.einsum("ui,boilt,vl->bouvt", _AT, M, _AT)
    y_bound = float(torch.einsum("ui,boilt,vl->bouvt", _AT.abs(), M.abs(), _AT.abs()).max())
    y = F.fold(y.reshape(B, -1, ty * tx), (4 * ty, 4 * tx), 4, stride=4)[:, :, :H, :W]
    return y.permute(0, 2, 3, 1), bool((U == U.round()).all()), acc_bound, y_bound


# --------------------------------------------------------------- the fused heads by blocks, restated (CPU, float64, exact data)
# Both fused heads (head_wino4_kernel, conv_wino_head_kernel) work per 16x16 block: the block's hidden pixels -- ZERO where they
# lie outside the image -- are convolved into the block's own 16x16 outputs and into the 68 pixels of the one-pixel ring
# around it (slots 0..17 the row above, x = -1..16; 18..35 the row below; 36..51 the column to the left, y = 0..15; 52..67 the
# column to the right); head_ring_fixup_kernel then adds to every border pixel what the neighbouring blocks owe it.
def ring_sources(py, px):
    """head_ring_fixup_kernel's index map: [(block dy, block dx, ring slot)] a block's local pixel (py, px) reads."""
    src = []
    if py == 0:
        src.append((-1, 0, 18 + px + 1))
    if py == 15:
        src.append((1, 0, px + 1))
    if px == 0:
        src.append((0, -1, 52 + py))
    if px == 15:
        src.append((0, 1, 36 + py))
    if py == 0 and px == 0:
        src.append((-1, -1, 35))
    if py == 0 and px == 15:
        src.append((-1, 1, 18))
    if py == 15 and px == 0:
        src.append((1, -1, 17))
    if py == 15 and px == 15:
        src.append((1, 1, 0))
    return src


def head_by_blocks(x, p, zero_outside=True, sources=ring_sources):
    """The heads' result through the block decomposition.  ``zero_outside=False`` leaves the hidden pixels outside the image as
    the first layer computes them from the zero-padded input (what the kernels' masks are there to prevent); ``sources`` is
    the fix-up's index map."""
    B, H, W, _ = x.shape
    nby, nbx = -(-H // 16), -(-W // 16)
    xe = F.pad(x, (0, 0, 0, nbx * 16 - W, 0, nby * 16 - H))            # the map extended with zeros to whole blocks
    hid = hidden64(xe, p)
    if zero_outside:
        hid[:, :, H:, :] = 0
        hid[:, :, :, W:] = 0
    total = sum(p["counts"])
    out = torch.zeros(B, total, nby * 16, nbx * 16, dtype=torch.float64)
    ring = torch.zeros(B, nby, nbx, total, 68, dtype=torch.float64)
    for by in range(nby):
        for bx in range(nbx):
            hb = hid[:, :, by * 16:by * 16 + 16, bx * 16:bx * 16 + 16]
            off, parts = 0, []
            for k, c in enumerate(p["counts"]):       # padding 2: the 18x18 outputs the block's hidden pixels reach
                parts.append(F.conv2d(hb[:, k * 64:(k + 1) * 64], p["w2"][off:off + c].double(), padding=2))
                off += c
            P = torch.cat(parts, 1)                   # P[.., oy + 1, ox + 1], (oy, ox) in [-1, 16]^2
            out[:, :, by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = P[:, :, 1:17, 1:17] + p["b2"].double()[None, :, None, None]
            ring[:, by, bx, :, 0:18] = P[:, :, 0, :]
            ring[:, by, bx, :, 18:36] = P[:, :, 17, :]
            ring[:, by, bx, :, 36:52] = P[:, :, 1:17, 0]
            ring[:, by, bx, :, 52:68] = P[:, :, 1:17, 17]
    border = [(py, px) for py in range(16) for px in range(16) if py in (0, 15) or px in (0, 15)]
    for by in range(nby):
        for bx in range(nbx):
            for py, px in border:
                y, xx = by * 16 + py, bx * 16 + px
                if y >= H or xx >= W:
                    continue
                for dy, dx, slot in sources(py, px):
                    if 0 <= by + dy < nby and 0 <= bx + dx < nbx:
                        out[:, :, y, xx] += ring[:, by + dy, bx + dx, :, slot]
    return out[:, :, :H, :W]
