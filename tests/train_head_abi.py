"""ctypes callers of the three training-head entry points (``sgv3d_centerhead_targets``, ``sgv3d_centerhead_loss_stats``,
``sgv3d_centerhead_loss``) on numpy arrays, and the seeded inputs of the edge-shape tests.

Every output is carved out of one device buffer that is filled with 0xFF bytes first; ``GUARD`` bytes before and after each
output, and the gaps that the batch strides of the loss leave between samples, must still hold 0xFF after the call."""
import ctypes

import numpy as np

from oracle import train_head_ref as R

GUARD = 512
LN9999 = float(np.log(9999.0))
BRANCHES = (('reg', 2), ('height', 1), ('dim', 3), ('rot', 2), ('vel', 2))
CODE_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 0.5)
BOX_SPLIT = 8            # kBoxSplit of csrc/head_loss.hip


class Arena:
    """One 0xFF-filled device buffer; ``add`` reserves a region that starts ``shift`` bytes after a 256-byte boundary."""

    def __init__(self):
        self.regions, self.size, self.buf, self.host = {}, GUARD, None, None

    def add(self, name, nbytes, shift=0):
        start = (self.size + 255) // 256 * 256 + shift
        self.regions[name] = (start, int(nbytes))
        self.size = start + int(nbytes) + GUARD

    def alloc(self):
        import torch
        self.buf = torch.full((self.size,), 0xFF, dtype=torch.uint8, device='cuda')
        assert self.buf.data_ptr() % 256 == 0
        return self

    def ptr(self, name):
        return self.buf.data_ptr() + self.regions[name][0]

    def put(self, name, array):
        import torch
        raw = np.frombuffer(np.ascontiguousarray(array).tobytes(), np.uint8)
        start, n = self.regions[name]
        assert raw.size == n
        self.buf[start:start + n] = torch.from_numpy(raw.copy()).cuda()

    def fetch(self):
        import torch
        torch.cuda.synchronize()
        self.host = self.buf.cpu().numpy()
        return self.host

    def get(self, name, dtype, shape=None):
        start, n = self.regions[name]
        a = np.frombuffer(self.host[start:start + n].tobytes(), dtype)
        return a.reshape(shape) if shape is not None else a

    def assert_guards(self, partly=None):
        """Every byte outside the regions is 0xFF; ``partly`` maps a region to the byte mask of what may be written in it."""
        free = np.ones(self.host.size, bool)
        for name, (start, n) in self.regions.items():
            free[start:start + n] = False if not partly or name not in partly else ~partly[name]
        assert (self.host[free] == 0xFF).all(), "bytes outside the outputs were written"

    def untouched(self):
        return bool((self.host == 0xFF).all())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lib():
    import torch
    from sgv3d_amd import _lib as L
    return L.load(), L.stream_handle(torch.device('cuda'))


# ------------------------------------------------------------------------------------------------------------- targets
def targets(boxes, labels, classes_per_task, max_objs, h, w, pc=(0.0, 0.0), voxel=(0.1, 0.1), osf=4.0, overlap=0.1, min_radius=2,
            norm_bbox=1, shifts=None, launches=1, null=(), batch=None, n_max=None):
    """``boxes`` f32 [B, n_max, 9], ``labels`` i32 [B, n_max] (or None with ``batch`` / ``n_max`` given).  ``shifts``: byte
    offsets of (heatmap, anno_box, ind, mask) from a 256-byte boundary; ``null``: names of pointers passed as NULL.
    -> dict(rc, heatmap [B, C, h, w], anno [T, B, max_objs, 10], ind, mask, runs = raw bytes after every launch, untouched)."""
    lib, stream = _lib()
    B = int(batch if batch is not None else boxes.shape[0])
    n_max = int(n_max if n_max is not None else boxes.shape[1])
    T, C = len(classes_per_task), max(int(sum(classes_per_task)), 1)
    shifts = shifts or (0, 0, 0, 0)
    slots = T * B * max_objs
    ar = Arena()
    for name, n, s in zip(('heatmap', 'anno', 'ind', 'mask'), (B * C * h * w * 4, slots * 40, slots * 8, slots), shifts):
        ar.add(name, n, s)
    ar.alloc()
    d_boxes = _dev(np.asarray(boxes, np.float32)) if boxes is not None and boxes.size else None
    d_labels = _dev(np.asarray(labels, np.int32)) if labels is not None and labels.size else None
    P = lambda name: None if name in null else ar.ptr(name)
    cpt = (ctypes.c_int32 * T)(*[int(c) for c in classes_per_task])
    runs = []
    for _ in range(launches):
        rc = lib.sgv3d_centerhead_targets(
            B, n_max, None if (d_boxes is None or 'boxes' in null) else d_boxes.data_ptr(),
            None if (d_labels is None or 'labels' in null) else d_labels.data_ptr(), T, cpt, max_objs, h, w, float(pc[0]),
            float(pc[1]), float(voxel[0]), float(voxel[1]), float(osf), float(overlap), int(min_radius), int(norm_bbox),
            P('heatmap'), P('anno'), P('ind'), P('mask'), stream)
        ar.fetch()
        ar.assert_guards()
        runs.append(tuple(ar.get(k, np.uint8).copy() for k in ('heatmap', 'anno', 'ind', 'mask')))
    return dict(rc=rc, heatmap=ar.get('heatmap', np.float32, (B, C, h, w)), anno=ar.get('anno', np.float32, (T, B, max_objs, 10)),
                ind=ar.get('ind', np.int64, (T, B, max_objs)), mask=ar.get('mask', np.uint8, (T, B, max_objs)), runs=runs,
                untouched=ar.untouched())


def train_cfg(max_objs, h, w, pc=(0.0, 0.0), voxel=(0.1, 0.1), osf=4, overlap=0.1, min_radius=2):
    return dict(point_cloud_range=[pc[0], pc[1], -5, pc[0] + w * osf * voxel[0], pc[1] + h * osf * voxel[1], 3],
                grid_size=[w * int(osf), h * int(osf), 1], voxel_size=[voxel[0], voxel[1], 8], out_size_factor=int(osf), dense_reg=1,
                gaussian_overlap=overlap, max_objs=max_objs, min_radius=min_radius, code_weights=list(CODE_WEIGHTS))


def class_names(classes_per_task):
    return [[f"t{t}c{c}" for c in range(n)] for t, n in enumerate(classes_per_task)]


def oracle_targets(boxes, labels, classes_per_task, max_objs, h, w, pc=(0.0, 0.0), voxel=(0.1, 0.1), osf=4.0, overlap=0.1,
                   min_radius=2, **unused):
    """The oracle on the same padded arrays (labels outside 0..total-1 belong to no class there either), in the layout of
    ``targets``: heatmap [B, C, h, w], anno / ind / mask [T, B, ...]."""
    cfg = train_cfg(max_objs, h, w, pc, voxel, osf, overlap, min_radius)
    hm, an, ind, mk = R.get_targets(list(boxes), list(labels), class_names(classes_per_task), cfg)
    return dict(heatmap=np.concatenate(hm, 1), anno=np.stack(an), ind=np.stack(ind), mask=np.stack(mk))


def random_boxes(rng, n, h, w, pc, cell=0.4, margin=1.0, size=(0.4, 3.0, 0.4, 8.0)):
    bx = np.zeros((n, 9), np.float32)
    bx[:, 0] = rng.uniform(pc[0] - margin, pc[0] + w * cell + margin, n)
    bx[:, 1] = rng.uniform(pc[1] - margin, pc[1] + h * cell + margin, n)
    bx[:, 2] = rng.uniform(-3, 1, n)
    bx[:, 3] = rng.uniform(size[0], size[1], n)
    bx[:, 4] = rng.uniform(size[2], size[3], n)
    bx[:, 5] = rng.uniform(0.5, 4.0, n)
    bx[:, 6] = rng.uniform(-np.pi, np.pi, n)
    bx[:, 7:9] = rng.normal(0, 2, (n, 2))
    return bx


def case_nonsquare(h, w):
    """150 boxes in sample 0, none in sample 1 (all padding), labels -1..4 over tasks of 1 and 3 classes (4 = no class)."""
    rng = np.random.default_rng(1000 + h)
    pc = (0.0, -0.2 * h)
    boxes = np.zeros((2, 150, 9), np.float32)
    labels = np.full((2, 150), -1, np.int32)
    boxes[0] = random_boxes(rng, 150, h, w, pc)
    labels[0] = rng.integers(-1, 5, 150)
    return dict(boxes=boxes, labels=labels, classes_per_task=[1, 3], max_objs=500, h=h, w=w, pc=pc)


def case_many(n_max):
    """One task of 3 classes, classes interleaved; -1 and 3 (= total_classes) in the middle of the list; sample 0 and sample 2
    are shorter than sample 1, so they end in padding rows."""
    rng = np.random.default_rng(2000 + n_max)
    h = w = 16
    boxes = np.zeros((3, n_max, 9), np.float32)
    labels = np.full((3, n_max), -1, np.int32)
    for b, n in enumerate((n_max - 9, n_max, n_max // 2)):
        boxes[b, :n] = random_boxes(rng, n, h, w, (0.0, 0.0), margin=0.3, size=(0.4, 2.0, 0.4, 3.0))
        lab = (np.arange(n) + b + 1) % 3          # row 64 of sample 1 is of class 0: boxes in the first rows rank behind it
        lab[10], lab[11], lab[20] = -1, 3, 3
        labels[b, :n] = lab
    return dict(boxes=boxes, labels=labels, classes_per_task=[3], max_objs=500, h=h, w=w)


def case_cut(max_objs):
    rng = np.random.default_rng(3000)
    boxes = random_boxes(rng, 150, 16, 16, (0.0, 0.0), margin=0.0, size=(0.4, 2.0, 0.4, 3.0))[None]
    labels = (np.arange(150, dtype=np.int32) % 2)[None]
    return dict(boxes=boxes, labels=labels, classes_per_task=[2, 1], max_objs=max_objs, h=16, w=16)


def case_edges(h, w):
    """One box per sample, centred in every corner cell and in the middle; min_radius 6 makes the window 13 x 13."""
    cells = sorted({(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)})
    boxes = np.zeros((len(cells), 1, 9), np.float32)
    for i, (cy, cx) in enumerate(cells):
        boxes[i, 0] = [0.4 * cx + 0.13, 0.4 * cy + 0.29, -1.0, 1.6, 3.9, 1.5, 0.3 * i, 1.0, -2.0]
    return dict(boxes=boxes, labels=np.zeros((len(cells), 1), np.int32), classes_per_task=[1], max_objs=3, h=h, w=w, min_radius=6)


def window_cuts(case):
    """Per sample of a one-box case: (left, right, top, bottom) cut of the oracle's window by the map."""
    cfg = train_cfg(**{k: case[k] for k in ('max_objs', 'h', 'w')}, min_radius=case.get('min_radius', 2))
    out = []
    for box in case['boxes'][:, 0]:
        cx, cy = int(np.float32(box[0]) / np.float32(0.1) / 4), int(np.float32(box[1]) / np.float32(0.1) / 4)
        wd, ln = np.float32(box[3] / np.float32(0.1)) / np.float32(4), np.float32(box[4] / np.float32(0.1)) / np.float32(4)
        r = max(cfg['min_radius'], int(R.gaussian_radius((ln, wd), 0.1)))
        out.append((cx - r < 0, cx + r >= case['w'], cy - r < 0, cy + r >= case['h']))
    return out


KNOWN_PC, KNOWN_H, KNOWN_W = (8.0, -4.0), 4, 6


def case_known():
    """Cells of exactly 1.0 (voxel 0.25, out_size_factor 4): the expected arrays of ``known_answers`` are written by hand."""
    px, py = KNOWN_PC
    rows = [
        (px + 2.0, py + 1.0, 0),            # slot 0: cell (1, 2), residual 0
        (px + 6.0, py + 1.0, 0),            # slot 1: x = pc + w -> skipped
        (px - 0.5, py + 3.0, 0),            # slot 2: x cell -0.5 truncates to 0, residual -0.5
        (px - 1.0, py + 3.0, 0),            # slot 3: x cell -1 -> skipped
        (px + 5.0, py - 0.5, 0),            # slot 4: y cell -0.5 truncates to 0
        (px + 5.0, py + 4.0, 0),            # slot 5: y = pc + h -> skipped
        (px + 3.0, py + 2.0, 0),            # slot 6: width 0 -> skipped
        (px + 3.0, py + 2.0, 0),            # slot 7: width < 0 -> skipped
        (px + 5.0, py + 3.0, 0),            # slot 8: the far corner cell (3, 5)
    ]
    boxes = np.zeros((1, len(rows), 9), np.float32)
    for i, (x, y, _) in enumerate(rows):
        boxes[0, i] = [x, y, 0.5, 1.0, 2.0, 4.0, 0.0, 3.0, -7.0]
    boxes[0, 6, 3], boxes[0, 7, 3] = 0.0, -1.0
    return dict(boxes=boxes, labels=np.zeros((1, len(rows)), np.int32), classes_per_task=[1], max_objs=12, h=KNOWN_H, w=KNOWN_W,
                pc=KNOWN_PC, voxel=(0.25, 0.25), min_radius=0, overlap=0.1)


def known_answers():
    """ind / mask / residuals of ``case_known``, by hand."""
    mask = np.zeros(12, np.uint8)
    ind = np.zeros(12, np.int64)
    res = np.zeros((12, 2), np.float32)
    mask[[0, 2, 4, 8]] = 1
    ind[0], ind[2], ind[4], ind[8] = 1 * 6 + 2, 3 * 6 + 0, 0 * 6 + 5, 3 * 6 + 5
    res[2], res[4] = (-0.5, 0.0), (0.0, -0.5)
    rest = np.array([0.5, 0.0, np.log(np.float32(2.0)), np.log(np.float32(4.0)), 0.0, 1.0, 3.0, -7.0], np.float32)
    return dict(mask=mask, ind=ind, res=res, rest=rest, peaks=[(1, 2), (3, 0), (0, 5), (3, 5)])


def case_radius_sweep():
    """1024 samples of one box on a 32 x 32 map: width and length each take 32 values from 0.05 to 12."""
    v = np.linspace(0.05, 12.0, 32).astype(np.float32)
    wd, ln = np.meshgrid(v, v, indexing='ij')
    boxes = np.zeros((1024, 1, 9), np.float32)
    boxes[:, 0] = [6.4 + 0.13, 6.4 + 0.21, -1.0, 1.0, 1.0, 1.5, 0.7, 0.0, 0.0]
    boxes[:, 0, 3], boxes[:, 0, 4] = wd.ravel(), ln.ravel()
    return dict(boxes=boxes, labels=np.zeros((1024, 1), np.int32), classes_per_task=[1], max_objs=1, h=32, w=32)


def case_max_merge():
    """Sample 0: two boxes of one class three cells apart (each peak lies under the other's slope).  Sample 1: two boxes of
    different classes on one cell."""
    boxes = np.zeros((2, 2, 9), np.float32)
    boxes[0, 0] = [0.4 * 5 + 0.1, 0.4 * 6 + 0.1, 0, 4.0, 9.0, 1.5, 0.0, 0, 0]
    boxes[0, 1] = [0.4 * 8 + 0.1, 0.4 * 6 + 0.1, 0, 1.0, 1.0, 1.5, 0.0, 0, 0]
    boxes[1, 0] = [0.4 * 4 + 0.2, 0.4 * 4 + 0.2, 0, 4.0, 9.0, 1.5, 0.0, 0, 0]
    boxes[1, 1] = [0.4 * 4 + 0.3, 0.4 * 4 + 0.1, 0, 1.0, 1.0, 1.5, 0.0, 0, 0]
    labels = np.array([[1, 1], [0, 1]], np.int32)
    return dict(boxes=boxes, labels=labels, classes_per_task=[2], max_objs=4, h=12, w=14)


def cells(case):
    """(cy, cx, on the map) of every row of a case, by the float32 cell arithmetic of the definition (truncation toward zero)."""
    F = np.float32
    pc, voxel, osf = case.get('pc', (0.0, 0.0)), case.get('voxel', (0.1, 0.1)), F(case.get('osf', 4.0))
    fx = (case['boxes'][..., 0] - F(pc[0])) / F(voxel[0]) / osf
    fy = (case['boxes'][..., 1] - F(pc[1])) / F(voxel[1]) / osf
    cx, cy = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)
    return cy, cx, (cx >= 0) & (cx < case['w']) & (cy >= 0) & (cy < case['h'])


TARGET_CASES = {
    'nonsquare_24x40': lambda: case_nonsquare(24, 40), 'nonsquare_40x24': lambda: case_nonsquare(40, 24),
    **{f'many_{n}': (lambda n=n: case_many(n)) for n in (64, 65, 128, 130, 200)},
    **{f'cut_{m}': (lambda m=m: case_cut(m)) for m in (1, 64, 65)},
    'edges_5x7': lambda: case_edges(5, 7), 'edges_1x9': lambda: case_edges(1, 9), 'edges_1x1': lambda: case_edges(1, 1),
    'known': case_known, 'radius_sweep': case_radius_sweep, 'max_merge': case_max_merge,
}


def expected_slots(labels, classes_per_task):
    """Slot of every box by the definition (class after class, input order inside a class), -1 for boxes of no class."""
    total = sum(classes_per_task)
    task_of = np.repeat(np.arange(len(classes_per_task)), classes_per_task)
    slots = np.full(labels.shape, -1, np.int64)
    for b in range(labels.shape[0]):
        for t in range(len(classes_per_task)):
            k = 0
            for c in np.where(task_of == t)[0]:
                for i in np.where(labels[b] == c)[0]:
                    slots[b, i] = k
                    k += 1
    assert ((slots >= 0) == ((labels >= 0) & (labels < total))).all()
    return slots


# ---------------------------------------------------------------------------------------------------------------- loss
def loss_workspace_bytes(batch):
    return int(_lib()[0].sgv3d_centerhead_loss_workspace_bytes(batch))


def loss(inp, grad_scale=1.0, stats=None, p_gap=0, t_planes=(0, 0), g_gap=0, grads=True, code_weights=CODE_WEIGHTS, box_weight=0.25,
         ws_short=0, max_objs_arg=None, t_stride_arg=None, p_stride_arg=None, g_stride_arg=None, null=(), launches=1):
    """``inp``: dict(heat [B, cat, h, w], reg, height, dim, rot, vel, target [B, cat, h, w], anno [B, mo, 10], ind i64 [B, mo],
    mask u8 [B, mo]).  The six prediction maps are channel slices of one buffer whose samples are ``p_gap`` floats apart (NaN in
    the gaps); the target planes sit behind ``t_planes[0]`` and before ``t_planes[1]`` foreign planes (filled with 1.0) of a wider
    heatmap buffer; the gradients are channel slices of one buffer with ``g_gap`` floats between the samples.  ``stats`` None:
    computed by ``sgv3d_centerhead_loss_stats``; else the two floats to inject.  ``grads``: True, False or six booleans.
    -> dict(rc, stats_rc, loss f32[2], stats f32[2], g_heat, g_reg, ... (None without gradients), untouched)."""
    lib, stream = _lib()
    heat = np.asarray(inp['heat'], np.float32)
    B, cat, h, w = heat.shape
    hw = h * w
    mo = int(inp['mask'].shape[1])
    names = ('heat',) + tuple(k for k, _ in BRANCHES)
    chans = (cat,) + tuple(c for _, c in BRANCHES)
    ctot = sum(chans)
    p_stride, g_stride = ctot * hw + p_gap, ctot * hw + g_gap
    pbuf = np.full((B, p_stride), np.nan, np.float32)
    offs, c0 = {}, 0
    for k, c in zip(names, chans):
        pbuf[:, c0 * hw:(c0 + c) * hw] = np.asarray(inp[k], np.float32).reshape(B, c * hw)
        offs[k] = c0 * hw
        c0 += c
    t_total = t_planes[0] + cat + t_planes[1]
    tbuf = np.ones((B, t_total, hw), np.float32)
    tbuf[:, t_planes[0]:t_planes[0] + cat] = np.asarray(inp['target'], np.float32).reshape(B, cat, hw)
    t_stride = t_total * hw
    d_p, d_t = _dev(pbuf), _dev(tbuf)
    d_anno, d_ind = _dev(np.asarray(inp['anno'], np.float32)), _dev(np.asarray(inp['ind'], np.int64))
    d_mask = _dev(np.asarray(inp['mask'], np.uint8))
    nws = loss_workspace_bytes(B)
    flags = (grads,) * 6 if isinstance(grads, bool) else tuple(grads)
    ar = Arena()
    ar.add('stats', 8)
    ar.add('loss', 8)
    ar.add('ws', nws - ws_short)
    ar.add('grad', B * g_stride * 4)
    ar.alloc()
    ws_bytes = nws - ws_short
    t_ptr = d_t.data_ptr() + t_planes[0] * hw * 4
    stats_rc = 0
    if stats is None:
        stats_rc = lib.sgv3d_centerhead_loss_stats(B, cat, h, w, mo, t_ptr, t_stride if t_stride_arg is None else t_stride_arg,
                                                   d_mask.data_ptr(), ar.ptr('stats'), ar.ptr('ws'), ws_bytes, stream)
    else:
        ar.put('stats', np.asarray(stats, np.float32))
    P = lambda k: None if k in null else d_p.data_ptr() + offs[k] * 4
    G = lambda i, k: ar.ptr('grad') + offs[k] * 4 if flags[i] else None
    cw = (ctypes.c_float * 10)(*[float(v) for v in code_weights])
    for _ in range(launches):
        rc = lib.sgv3d_centerhead_loss(
            B, cat, h, w, mo if max_objs_arg is None else max_objs_arg, *[P(k) for k in names],
            p_stride if p_stride_arg is None else p_stride_arg, t_ptr,
            t_stride if t_stride_arg is None else t_stride_arg, d_anno.data_ptr(), d_ind.data_ptr(), d_mask.data_ptr(),
            ar.ptr('stats'), cw, float(box_weight), float(grad_scale), *[G(i, k) for i, k in enumerate(names)],
            g_stride if g_stride_arg is None else g_stride_arg,
            ar.ptr('loss'), ar.ptr('ws'), ws_bytes, stream)
    ar.fetch()
    inside = np.zeros((B, g_stride * 4), bool)
    if all(flags) and rc == 0:
        inside[:, :ctot * hw * 4] = True
    ar.assert_guards({'grad': inside.ravel()})
    s0 = ar.regions['stats'][0]
    out = dict(rc=rc, stats_rc=stats_rc, loss=ar.get('loss', np.float32), stats=ar.get('stats', np.float32),
               untouched=bool((np.delete(ar.host, np.arange(s0, s0 + 8)) == 0xFF).all()))   # all but the stats
    g = ar.get('grad', np.float32, (B, g_stride))
    for k, c in zip(names, chans):
        out['g_' + k] = g[:, offs[k]:offs[k] + c * hw].reshape(B, c, h, w).copy() if all(flags) and rc == 0 else None
    return out


def smooth_logits(rng, shape, scale=2.0):
    """Logits of which none lies within 1e-3 of +-ln 9999, where the clamp of the sigmoid switches the gradient."""
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    x[np.abs(np.abs(x) - LN9999) < 2e-3] = 0.5
    return x


def loss_inputs(seed, batch, cat, h, w, max_objs, live=0.7):
    """Seeded inputs of the loss: smooth logits, targets in [0, 1) with a few cells of exactly 1, random slots on random cells."""
    rng = np.random.default_rng(seed)
    hw = h * w
    inp = dict(heat=smooth_logits(rng, (batch, cat, h, w)))
    for k, c in BRANCHES:
        inp[k] = rng.standard_normal((batch, c, h, w)).astype(np.float32)
    tgt = (rng.uniform(0, 0.95, (batch, cat, h, w)) ** 3).astype(np.float32)
    tgt[rng.uniform(size=tgt.shape) < 0.08] = 1.0
    tgt[rng.uniform(size=tgt.shape) < 0.3] = 0.0
    inp['target'] = tgt
    inp['anno'] = rng.standard_normal((batch, max_objs, 10)).astype(np.float32)
    inp['ind'] = rng.integers(0, hw, (batch, max_objs)).astype(np.int64)
    inp['mask'] = (rng.uniform(size=(batch, max_objs)) < live).astype(np.uint8)
    return inp


def split_parts(max_objs):
    """Part of every slot under the box kernel's split of a sample's slots over BOX_SPLIT workgroups."""
    per = (max_objs + BOX_SPLIT - 1) // BOX_SPLIT
    return np.arange(max_objs) // per


def shared_one_cell(max_objs, batch=2, h=5, w=9, seed=50):
    """All slots of a sample on one cell (another cell per sample)."""
    inp = loss_inputs(seed, batch, 2, h, w, max_objs, live=1.1)
    for b in range(batch):
        inp['ind'][b] = (7 * b + 3) % (h * w)
    return inp


def shared_straddle(max_objs, phase=0, h=5, w=9, seed=51):
    """Pairs of slots on one cell on both sides of the boundaries between two parts of the split; all other slots masked.
    Parts of one slot (max_objs <= 8) cannot pair over every boundary at once: ``phase`` 0 pairs (0, 1), (2, 3), ... and
    ``phase`` 1 pairs (1, 2), (3, 4), ...; with longer parts phase 0 covers every boundary."""
    inp = loss_inputs(seed, 1, 1, h, w, max_objs, live=1.1)
    part = split_parts(max_objs)
    inp['mask'][:] = 0
    cell, used = 0, {-1} if phase == 0 else {0}
    for k in range(1, max_objs):
        if part[k] != part[k - 1] and k - 1 not in used:
            inp['ind'][0, k - 1] = inp['ind'][0, k] = cell
            inp['mask'][0, k - 1] = inp['mask'][0, k] = 1
            used.update((k - 1, k))
            cell += 1
    return inp


def shared_far_trio(max_objs=2100, h=5, w=9, seed=52):
    """Three slots on one cell, more than 256 apart inside one part and across parts, among random other slots elsewhere."""
    inp = loss_inputs(seed, 1, 2, h, w, max_objs, live=0.5)
    cell = 17
    inp['ind'][inp['ind'] == cell] = cell + 1
    trio = (3, 3 + 257, 3 + 257 + 600)
    for k in trio:
        inp['ind'][0, k], inp['mask'][0, k] = cell, 1
    return inp, trio, cell


CLAMP_LOGITS = (9.0, -9.0, 9.5, -9.5, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 0.0)


def clamp_inputs():
    """Every logit of CLAMP_LOGITS on a positive cell (plane 0 row 0), on a cell of target 0 (row 1) and on one of 0.5 (row 2)."""
    inp = loss_inputs(60, 1, 2, 5, len(CLAMP_LOGITS), 4)
    for row, t in enumerate((1.0, 0.0, 0.5)):
        inp['heat'][0, 0, row] = CLAMP_LOGITS
        inp['target'][0, 0, row] = t
    return inp
