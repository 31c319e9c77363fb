"""TEST INFRASTRUCTURE ONLY.  Inputs, known answers and the raw C-ABI call that the CPU and the GPU tests of the circle-NMS
box decode share (csrc/decode.hip, ``nms_type='circle'``).  The reference is ``oracle.decode_ref`` (parity with mmdet3d
unpinned, see there); nothing here restates the decode.

Three kinds of input:

* the *dyadic coder*: 0.5 m cells whose origin and size are powers of two, ``reg`` in {-0.5, 0, 0.5}.  Every centre and every
  squared centre distance is exact in float32, so a decision is the same with one rounding per operation or with fused
  multiply-adds: these cases test logic, not rounding;
* *quantised heat*: logits from LEVELS.  Neighbouring levels in [-8, 8] are more than 3600 float32 ulp apart after the
  sigmoid, 20 and +inf give exactly 1.0, -100 and -inf exactly 0.0, 0 exactly 0.5: the device's exp may differ from numpy's by
  an ulp without changing which scores are equal or how they are ordered.  (No logit in about (-104, -87): its sigmoid is
  subnormal.)  Heat is never NaN;
* regression maps whose bits identify their cell: ``height`` a multiple of 1/4, ``dim`` a multiple of 1/8, ``rot`` and ``vel``
  distinct floats.  ``height`` and ``vel`` are copied through, so their bitwise equality pins the cell a row was gathered from.
"""
import ctypes

import numpy as np

from oracle import decode_ref

LEVELS = np.array([-np.inf, -100, -20, -6, -4, -2, -1, 0, 0.5, 1, 2, 4, 8, 20, np.inf], np.float32)
CELL = 0.5                                                   # metres per heat-map cell of the dyadic coder
X0, Y0 = 0.0, -8.0


def dyadic_coder(max_num, score_threshold=0.1, post_center_range=None):
    c = dict(type='CenterPointBBoxCoder', max_num=max_num, out_size_factor=4, voxel_size=[0.125, 0.125, 8],
             pc_range=[X0, Y0, -5, 256.0, 248.0, 3], code_size=9)
    if score_threshold is not None:
        c['score_threshold'] = score_threshold
    if post_center_range is not None:
        c['post_center_range'] = post_center_range
    return c


# ------------------------------------------------------------------------------------------------ buffers
def make_layout(ncls, has_vel=True):
    """One [B, C, H, W] buffer holds every map of every task (the decode wants one batch stride): name -> (offset, channels)."""
    names = [('reg', 2), ('height', 1), ('dim', 3), ('rot', 2)] + ([('vel', 2)] if has_vel else [])
    layout, off = [], 0
    for nc in ncls:
        d = {}
        for n, c in names + [('heatmap', nc)]:
            d[n] = (off, c)
            off += c
        layout.append(d)
    return layout, off


def preds_of(buf, layout):
    """The head's output structure over views of ``buf`` (numpy or torch)."""
    return tuple([{k: buf[:, o:o + c] for k, (o, c) in d.items()}] for d in layout)


def fill_regression(g, buf, layout, reg_zero=False):
    B, _, H, W = buf.shape
    for d in layout:
        view = lambda n: buf[:, d[n][0]:d[n][0] + d[n][1]]
        view('reg')[:] = 0.0 if reg_zero else g.choice(np.array([-0.5, 0.0, 0.5], np.float32), size=(B, 2, H, W))
        view('height')[:] = g.integers(-12, 13, size=(B, 1, H, W)).astype(np.float32) / 4
        view('dim')[:] = g.integers(-8, 9, size=(B, 3, H, W)).astype(np.float32) / 8
        for n in ('rot', 'vel'):
            if n in d:                                       # distinct floats: a permutation of exact multiples of 2^-10
                m = B * 2 * H * W
                view(n)[:] = ((g.permutation(m).astype(np.float32) - m // 2) / 1024).reshape(B, 2, H, W)
                if n == 'rot':
                    view(n)[:] += np.float32(1.0 / 4096)     # (never atan2(0, 0))


def quantised_heat(g, shape, K, top):
    """Logits drawn from LEVELS.  ``top``: the three highest score values (1.0, sigmoid(8), sigmoid(4)) get about ``top * K``
    cells each per class -- with 0.4 the K-th largest score of a class falls inside the third group of equal scores; None:
    all levels are equally likely."""
    hw = shape[-2] * shape[-1]
    p = np.full(len(LEVELS), 1.0 / len(LEVELS))
    if top is not None:
        q = top * K / hw
        assert 3 * q < 0.9
        p[:] = (1.0 - 3 * q) / (len(LEVELS) - 4)
        p[-1] = p[-2] = q / 2                                # +inf and 20: both exactly 1.0
        p[-3] = p[-4] = q                                    # 8 and 4
    return g.choice(LEVELS, size=shape, p=p)


# (H, W, K, classes per task, B, top (see quantised_heat), score_threshold): the tie cases of tests/test_decode_gpu.py.  The threshold is
# 0.9999 where the merged K best scores are all >= sigmoid(4) (it rejects sigmoid(8) = 0.99966 and keeps 1.0), else 0.1.
TIE_CASES = [
    (37, 53, 500, [1, 2, 3], 2, 0.4, 0.9999),       # odd H*W: scalar loads, idle threads; K <= 512: the one-wave NMS kernel
    (24, 25, 600, [2, 1], 2, None, 0.1),          # H*W == K; K > 512: the serial NMS kernel
    (64, 64, 512, [1, 2, 3], 2, 0.4, 0.9999),
    (257, 256, 512, [2], 1, 0.4, 0.9999),           # H*W > 65536: the top-k form without cached keys
    (32, 32, 1024, [8], 1, 0.05, 0.9999),           # the largest sort the argument checks accept
    (5, 7, 1, [2, 1], 1, None, 0.1),
    (16, 16, 2, [3], 3, None, 0.1),
]
TIE_CAP = 60
TIE_RADII = [0.0, 1.0, 64.0]                       # per task: radius 0 keeps nearly everything (the cap cuts), 8 m keeps few


def tie_case(case, seed=None):
    """-> (buf [B, C, H, W], layout, bbox_coder, test_cfg, classes per task) of one of TIE_CASES."""
    H, W, K, ncls, B, top, thr = case
    g = np.random.default_rng(H * 1000 + W if seed is None else seed)
    layout, C = make_layout(ncls)
    buf = np.zeros((B, C, H, W), np.float32)
    fill_regression(g, buf, layout)
    for d in layout:
        o, c = d['heatmap']
        buf[:, o:o + c] = quantised_heat(g, (B, c, H, W), K, top)
    # the range cuts a margin off every side and the lowest and highest heights (the two tiny cases would lose every row)
    rng = [1.0, Y0 + 1.0, -2.0, X0 + CELL * W * 0.75, Y0 + CELL * H * 0.75, 2.0] if K >= 8 else None
    coder = dyadic_coder(K, thr, rng)
    radii = TIE_RADII[:len(ncls)] if len(ncls) > 1 else [1.0]
    return buf, layout, coder, dict(min_radius=radii, post_max_size=TIE_CAP, nms_type='circle'), ncls


def tie_counts(heat_logits, K):
    """(n_gt, n_eq) of one class's [H, W] logits: cells above and cells equal to the K-th largest score."""
    with np.errstate(over='ignore'):
        s = decode_ref._sigmoid(heat_logits.reshape(-1))
    kth = np.sort(s)[::-1][K - 1]
    return int((s > kth).sum()), int((s == kth).sum())


# ------------------------------------------------------------------------------------------------ hand-built edge cases
EDGE_H, EDGE_W = 24, 25
EDGE_KS = (8, 520)                                 # the one-wave and the serial NMS kernel


def _edge_field(peaks, K, **coder_kw):
    """One task, one class, one sample, background logit -20.  peaks: (row, col, logit[, dict(reg_x, reg_y, height)])."""
    layout, C = make_layout([1])
    buf = np.zeros((1, C, EDGE_H, EDGE_W), np.float32)
    fill_regression(np.random.default_rng(5), buf, layout, reg_zero=True)
    d = layout[0]
    buf[:, d['height'][0]] = 0.0
    buf[:, d['heatmap'][0]] = -20.0
    for p in peaks:
        r, c, logit = p[:3]
        extra = p[3] if len(p) > 3 else {}
        buf[0, d['heatmap'][0], r, c] = logit
        buf[0, d['reg'][0], r, c] = extra.get('reg_x', 0.0)
        buf[0, d['reg'][0] + 1, r, c] = extra.get('reg_y', 0.0)
        buf[0, d['height'][0], r, c] = extra.get('height', 0.0)
    return buf, layout, dyadic_coder(K, **coder_kw)


def xy(row, col):
    return (X0 + CELL * col, Y0 + CELL * row)


def edge_cases(K):
    """name -> (buf, layout, coder, test_cfg, expected [(x, y), ...] of the reported boxes in order).  The answers are
    worked out by hand from the rules (DESIGN.md "Box decode: nms_type='circle'")."""
    out = {}
    far = dict(min_radius=[0.0625], post_max_size=83)
    # score > threshold, strictly: sigmoid(0) == 0.5 exactly
    out['score_threshold'] = _edge_field([(3, 4, 0.0), (10, 12, 0.5)], K, score_threshold=0.5) + (far, [xy(10, 12)])
    # centre range, bounds inclusive; NaN compares false
    zmin = np.float32(-2.0)
    below = np.nextafter(zmin, np.float32(-np.inf))
    peaks = [(2, 1, 6.0), (5, 2, 5.5), (8, 20, 5.0), (11, 21, 4.5),                 # x = 0.5, 1.0, 10.0, 10.5
             (14, 10, 4.0, dict(height=zmin)), (17, 10, 3.5, dict(height=below)),
             (20, 10, 3.0, dict(reg_x=np.nan))]
    out['range'] = _edge_field(peaks, K, score_threshold=0.1, post_center_range=[1.0, -100.0, float(zmin), 10.0, 100.0, 5.0]) + \
        (far, [xy(5, 2), xy(8, 20), xy(14, 10)])
    # dist <= radius^2, inclusive: 3 cells = 1.5 m, squared 2.25
    two = [(6, 5, 3.0), (6, 8, 2.0)]
    out['distance_on'] = _edge_field(two, K) + (dict(min_radius=[2.25], post_max_size=83), [xy(6, 5)])
    under = float(np.nextafter(np.float32(2.25), np.float32(0)))
    out['distance_under'] = _edge_field(two, K) + (dict(min_radius=[under], post_max_size=83), [xy(6, 5), xy(6, 8)])
    # chain: A suppresses B, so B may not suppress C
    out['chain'] = _edge_field([(9, 3, 4.0), (9, 5, 2.0), (9, 7, 1.0)], K) + \
        (dict(min_radius=[1.0], post_max_size=83), [xy(9, 3), xy(9, 7)])
    # only kept boxes count towards post_max_size
    pairs = [(2, 2, 6.0), (2, 3, 5.0), (10, 12, 4.0), (11, 12, 3.0), (20, 20, 2.0), (20, 21, 1.0)]
    for cap in (2, 3):
        out['cap_%d' % cap] = _edge_field(pairs, K) + (dict(min_radius=[0.25], post_max_size=cap),
                                                        [xy(2, 2), xy(10, 12), xy(20, 20)][:cap])
    return out


def empty_case():
    """Two samples, the first without any cell above the threshold.  -> (buf, layout, coder, test_cfg, expected per sample)."""
    buf, layout, coder = _edge_field([], 8)
    buf = np.concatenate([buf, buf.copy()])
    buf[1, layout[0]['heatmap'][0], 7, 9] = 2.0
    buf[1, layout[0]['heatmap'][0], 15, 3] = 1.0
    return buf, layout, coder, dict(min_radius=[0.25], post_max_size=83), [[], [xy(7, 9), xy(15, 3)]]


# ------------------------------------------------------------------------------------------------ dense NMS, no masks
DENSE_RADII = [0.0, 0.25, 1.0, 2.25]
DENSE_SHAPES = [(64, 64, 512), (40, 41, 600), (32, 32, 1024)]


def dense_case(H, W, K, cap, ncls=(2, 2, 2, 2), reg_zero=False, radii=DENSE_RADII, has_vel=True, B=2):
    """Quantised heat on the dyadic coder with neither a score threshold nor a centre range: all K rows are valid."""
    g = np.random.default_rng(H + W + K)
    layout, C = make_layout(list(ncls), has_vel)
    buf = np.zeros((B, C, H, W), np.float32)
    fill_regression(g, buf, layout, reg_zero)
    for d in layout:
        o, c = d['heatmap']
        buf[:, o:o + c] = quantised_heat(g, (B, c, H, W), K, None)
    return buf, layout, dyadic_coder(K, None, None), dict(min_radius=list(radii), post_max_size=cap), list(ncls)


# ------------------------------------------------------------------------------------------------ the rounding probe
def rounding_pairs(coder, radius, rows=256, gap=5):
    """Rows r such that two centres in one column, ``gap`` rows apart (r and r + gap), ``reg = 0``, get a different
    ``dist <= radius`` decision when ``t * voxel + pc`` is one fused multiply-add than when it is two float32 roundings.
    Pure numpy; the fused form is emulated in float64, where the product of two float32 and its sum with a third of similar
    magnitude are exact, then rounded to float32 once.  -> (list of (r, survives_per_operation, survives_fused), pairs tried,
    rows whose fused y differs)."""
    f32 = np.float32
    t = (np.arange(rows, dtype=f32) + f32(0)) * f32(coder['out_size_factor'])
    vy, pcy = f32(coder['voxel_size'][1]), f32(coder['pc_range'][1])
    y_op = (t * vy + pcy).astype(f32)
    y_fma = (t.astype(np.float64) * np.float64(vy) + np.float64(pcy)).astype(f32)
    out = []
    for r in range(rows - gap):
        dec = []
        for y in (y_op, y_fma):
            dy = f32(y[r] - y[r + gap])
            dec.append(bool(f32(dy * dy) > f32(radius)))        # True: the weaker one survives
        if dec[0] != dec[1]:
            out.append((r, dec[0], dec[1]))
    return out, rows - gap, int((y_op != y_fma).sum())


def rounding_field(coder, pair_rows, K=500, H=256, W=256, col0=10, col_step=20):
    """One task, one class, one sample: for every row r of ``pair_rows`` two peaks in one column at rows r and r + 5, the
    columns ``col_step`` cells apart (8 m: no pair sees another under a 2 m radius).  Distinct logits, the upper row stronger."""
    layout, C = make_layout([1])
    buf = np.zeros((1, C, H, W), np.float32)
    fill_regression(np.random.default_rng(6), buf, layout, reg_zero=True)
    hm = layout[0]['heatmap'][0]
    buf[:, layout[0]['height'][0]] = 0.0
    buf[:, hm] = -20.0
    cells = []
    for n, r in enumerate(pair_rows):
        c = col0 + col_step * n
        assert c < W
        buf[0, hm, r, c] = 6.0 - 0.25 * n
        buf[0, hm, r + 5, c] = 6.0 - 0.25 * n - 0.125
        cells.append((r, c))
    return buf, layout, dict(coder, max_num=K), cells


# ------------------------------------------------------------------------------------------------ the oracle, all K rows
def oracle_raw(buf, layout, coder, test_cfg, norm_bbox=True):
    """``raw_decode``'s arrays from the oracle: boxes [T, B, K, 9] (columns 7, 8 zero without ``vel``; z not lowered),
    scores, labels, valid, keep [T, B, K]."""
    preds = preds_of(buf, layout)
    T, B, K = len(layout), buf.shape[0], coder['max_num']
    out = dict(boxes=np.zeros((T, B, K, 9), np.float32), scores=np.zeros((T, B, K), np.float32),
               labels=np.zeros((T, B, K), np.int32), valid=np.zeros((T, B, K), np.uint8), keep=np.zeros((T, B, K), np.uint8))
    with np.errstate(over='ignore'):
        for t in range(T):
            for b, c in enumerate(decode_ref.decode_candidates(preds[t][0], coder, norm_bbox)):
                out['boxes'][t, b, :, :c['boxes'].shape[1]] = c['boxes']
                out['scores'][t, b], out['labels'][t, b], out['valid'][t, b] = c['scores'], c['clses'], c['mask']
                rows = np.nonzero(c['mask'])[0]
                dets = np.concatenate([c['boxes'][rows, :2], c['scores'][rows, None]], 1)
                kept = decode_ref.circle_nms(dets, test_cfg['min_radius'][t], test_cfg['post_max_size'])
                out['keep'][t, b, rows[kept]] = 1
    return out


def oracle_merged(buf, layout, coder, test_cfg, ncls, norm_bbox=True):
    with np.errstate(over='ignore'):
        res = decode_ref.get_bboxes(preds_of(buf, layout), coder, test_cfg, ncls, norm_bbox)
    for r in res:
        if r[0].shape[1] == 7:                                # no vel: the device reports zeros in columns 7 and 8
            r[0] = np.concatenate([r[0], np.zeros((len(r[0]), 2), np.float32)], 1)
    return res


# ------------------------------------------------------------------------------------------------ the C ABI, raw
POISON = 0x5A


def raw_decode(dbuf, layout, coder, test_cfg, norm_bbox=True, ncls=None, ws_delta=0):
    """``sgv3d_centerpoint_decode_tasks`` through ctypes on a device buffer ``dbuf`` [B, C, H, W] (torch).  -> (return code,
    dict of numpy arrays boxes [T, B, K, 9], scores, labels, valid, keep [T, B, K]).  The outputs are pre-filled with the
    byte POISON, so a caller can tell that a rejected call wrote nothing.  ``ncls`` overrides the class counts handed to the
    library and ``ws_delta`` is added to the workspace size it is told (the argument-check tests)."""
    import torch
    from sgv3d_amd import _lib
    lib = _lib.load()
    dev = dbuf.device
    T, B, H, W, K = len(layout), int(dbuf.shape[0]), int(dbuf.shape[2]), int(dbuf.shape[3]), int(coder['max_num'])
    preds = preds_of(dbuf, layout)
    has_vel = all('vel' in d for d in layout)
    ptrs = {k: (ctypes.c_void_p * T)(*[preds[t][0][k].data_ptr() for t in range(T)])
            for k in ('heatmap', 'reg', 'height', 'dim', 'rot') + (('vel',) if has_vel else ())}
    cats = [d['heatmap'][1] for d in layout] if ncls is None else list(ncls)
    nws = lib.sgv3d_centerpoint_decode_tasks_workspace_bytes(B, T, max(max(cats), 1), K)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)
    n = T * B * K
    o = dict(boxes=torch.full((n * 36,), POISON, dtype=torch.uint8, device=dev))
    for name, width in (('scores', 4), ('labels', 4), ('valid', 1), ('keep', 1)):
        o[name] = torch.full((n * width,), POISON, dtype=torch.uint8, device=dev)
    rng, thr = coder.get('post_center_range'), coder.get('score_threshold')
    rng_c = (ctypes.c_float * 6)(*[float(v) for v in rng]) if rng is not None else None
    with torch.cuda.device(dev):
        rc = lib.sgv3d_centerpoint_decode_tasks(
            B, T, (ctypes.c_int32 * T)(*cats), H, W, K, ptrs['heatmap'], ptrs['reg'], ptrs['height'], ptrs['dim'], ptrs['rot'],
            ptrs.get('vel'), int(dbuf.stride(0)), float(coder['out_size_factor']), float(coder['voxel_size'][0]),
            float(coder['voxel_size'][1]), float(coder['pc_range'][0]), float(coder['pc_range'][1]),
            float(thr) if thr is not None else float('-inf'), rng_c, 1 if norm_bbox else 0,
            (ctypes.c_float * T)(*[float(test_cfg['min_radius'][t]) for t in range(T)]), int(test_cfg['post_max_size']),
            ws.data_ptr(), nws + ws_delta, o['boxes'].data_ptr(), o['scores'].data_ptr(), o['labels'].data_ptr(),
            o['valid'].data_ptr(), o['keep'].data_ptr(), _lib.stream_handle(dev))
    torch.cuda.synchronize(dev)
    host = {k: v.cpu().numpy() for k, v in o.items()}
    return rc, dict(boxes=host['boxes'].view(np.float32).reshape(T, B, K, 9), scores=host['scores'].view(np.float32).reshape(T, B, K),
                    labels=host['labels'].view(np.int32).reshape(T, B, K), valid=host['valid'].reshape(T, B, K),
                    keep=host['keep'].reshape(T, B, K))
