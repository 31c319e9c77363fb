"""Shared by the frame-recombination tests and the fixture's maker: synthetic roadside scenes, the fixture's scenes as
frames, and the host entry of csrc/recombine.hip (``sgv3d_recombine_host``) as a function of frames."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "recombine.npz")
CLASS_ID = {"car": 6, "van": 5, "bus": 4, "truck": 3, "pedestrian": 2, "cyclist": 1, "bicycle": 1, "tricyclist": 1, "motorcycle": 1,
            "motorcyclist": 1}


# ---------------------------------------------------------------------------------------------------------------- scenes
def camera(h, w, tilt=0.2, roll=0.0, pan=0.0, focal=1.1, height=6.2, side=-0.1, back=0.4):
    """A roadside camera scaled to an h x w frame -> (Tr_ego2cam f64 [4, 4], P2 f32 [3, 4]); ego x points down the road."""
    f = focal * w
    P2 = np.zeros((3, 4), np.float32)
    P2[:3, :3] = [[f, 0, 0.497 * w + 0.31], [0, f * 1.002, 0.503 * h - 0.27], [0, 0, 1]]
    base = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64)
    ct, st, cr, sr, cp, sp = np.cos(tilt), np.sin(tilt), np.cos(roll), np.sin(roll), np.cos(pan), np.sin(pan)
    R = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]]) @ \
        np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ base
    Tr = np.eye(4)
    Tr[:3, :3] = R
    Tr[:3, 3] = R @ -np.array([back, side, height])
    Tr = Tr.astype(np.float32).astype(np.float64)          # what a calib file's float32 row holds
    Tr[3] = [0, 0, 0, 1]
    return np.linalg.inv(np.linalg.inv(Tr)), P2            # process_sample inverts twice


def ego_box(x, y, yaw, dim):
    """Ego-frame corners [3, 8] of a box of (h, w, l) standing on the ground at (x, y)."""
    h, w, l = dim
    cx = np.array([l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2])
    cy = np.array([w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2])
    cz = np.array([0, 0, 0, 0, h, h, h, h], np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([c * cx - s * cy + x, s * cx + c * cy + y, cz])


SIZES = {"car": (1.5, 1.8, 4.4), "van": (2.0, 1.9, 4.9), "truck": (3.2, 2.5, 8.0), "bus": (3.1, 2.6, 10.5), "pedestrian": (1.7, 0.6, 0.6),
         "cyclist": (1.6, 0.7, 1.8), "motorcyclist": (1.5, 0.8, 1.9), "tricyclist": (1.6, 1.2, 2.4)}


def make_objects(rng, n, names=None, x_range=(14.0, 70.0), pseudo=False):
    names = names or [str(rng.choice(["Car", "car", "Van", "Truck", "Bus", "Pedestrian", "Cyclist", "Motorcyclist", "Tricyclist"]))
                      for _ in range(n)]
    corners, dim = [], []
    for name in names:
        x = rng.uniform(*x_range)
        d = np.array(SIZES[name.lower()]) * rng.uniform(0.9, 1.1, 3)
        corners.append(ego_box(x, rng.uniform(-0.3, 0.3) * x, rng.uniform(-np.pi, np.pi), d))
        dim.append(d)
    return dict(corners=np.array(corners).reshape(n, 3, 8), dim=np.array(dim).reshape(n, 3),
                truncated=rng.integers(0, 3, n).astype(np.float64), occluded=rng.integers(0, 3, n).astype(np.float64),
                score=np.round(rng.uniform(0.7, 1.0, n), 3) if pseudo else np.ones(n), names=list(names))


def make_image(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(xx[..., None] / (5.0 + np.arange(3)) + yy[..., None] / 7.0 + rng.uniform(0, 6))
    return np.clip(base + rng.integers(-25, 26, (h, w, 3)), 0, 255).astype(np.uint8)


def make_mask(frame, h, w, rng):
    """A stored class-id mask: every object's own projected box filled with its class id (first writer wins), plus a few
    stray ids, one of them above 6."""
    import recombine_ref as R
    mask = np.zeros((h, w), np.uint8)
    o = frame['objects']
    for i, name in enumerate(o['names']):
        box = R.float_box(o['corners'][i], None, frame['Tr_ego2cam'], frame['P2'])
        if box is None:
            continue
        x0, y0, x1, y1 = (int(np.clip(v, -1, 10 * w)) for v in box)
        region = mask[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)]
        region[region == 0] = CLASS_ID[name.lower()]
    for _ in range(3):
        y, x = rng.integers(0, h - 3), rng.integers(0, w - 3)
        mask[y:y + 3, x:x + 3] = rng.integers(1, 7)
    mask[h // 2, w // 3] = 7
    return mask


def make_frame(rng, h, w, n_obj, pseudo=False, **cam):
    Tr, P2 = camera(h, w, **cam)
    fr = dict(Tr_ego2cam=Tr, P2=P2, objects=make_objects(rng, n_obj, pseudo=pseudo))
    fr['image'] = make_image(rng, h, w)
    fr['mask'] = make_mask(fr, h, w, rng)
    return fr


def make_scene(seed, h, w, n_src=3, n_dest_obj=3, n_src_obj=7):
    """A destination and ``n_src`` sources whose cameras differ a little in tilt, roll, pan, focal length and height."""
    rng = np.random.default_rng(seed)
    dest = make_frame(rng, h, w, n_dest_obj)
    sources = [make_frame(rng, h, w, n_src_obj, pseudo=bool(s % 2), tilt=0.2 + rng.uniform(-0.03, 0.03), roll=rng.uniform(-0.04, 0.04),
                          pan=rng.uniform(-0.05, 0.05), focal=1.1 * rng.uniform(0.93, 1.07), height=6.2 + rng.uniform(-0.6, 0.6))
               for s in range(n_src)]
    return dest, sources


# --------------------------------------------------------------------------------------------------------------- fixture
def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def _objects_from(G, key):
    return dict(corners=G[f'{key}_corners'], dim=G[f'{key}_dim'], truncated=G[f'{key}_truncated'], occluded=G[f'{key}_occluded'],
                score=G[f'{key}_score'], names=[str(s) for s in G[f'{key}_names']])


def golden_scene(G, name):
    """-> (dest, sources) of fixture scene ``name``; the sources' objects are in the order the reference's draw walked them."""
    def frame(key):
        return dict(image=G[f'{key}_image'], mask=G[f'{key}_mask'], Tr_ego2cam=G[f'{key}_Tr'], P2=G[f'{key}_P2'],
                    objects=_objects_from(G, key))
    return frame(f'{name}_dest'), [frame(f'{name}_src{s}') for s in range(int(G[f'{name}_n_src']))]


def save_frame(out, key, fr, order=None):
    o = fr['objects']
    idx = np.arange(len(o['names'])) if order is None else np.asarray(order, np.int64)
    out[f'{key}_image'], out[f'{key}_mask'] = fr['image'], fr['mask']
    out[f'{key}_Tr'], out[f'{key}_P2'] = np.asarray(fr['Tr_ego2cam'], np.float64), np.asarray(fr['P2'], np.float32)
    out[f'{key}_corners'], out[f'{key}_dim'] = o['corners'][idx], o['dim'][idx]
    for k in ('truncated', 'occluded', 'score'):
        out[f'{key}_{k}'] = np.asarray(o[k], np.float64)[idx]
    out[f'{key}_names'] = np.array([o['names'][i] for i in idx], dtype='U16')


# ------------------------------------------------------------------------------------------------------------ host entry
def host_entry(jobs, max_obj=64, want_warped=True, order=None):
    """``jobs``: list of (dest, sources) -> the outputs of ``sgv3d_recombine_host`` as a dict of arrays plus per-frame label
    text.  All frames of all jobs form the pool."""
    from sgv3d_amd import _lib, recombine as RC
    lib = _lib.load()
    frames, slot = [], {}

    def index_of(fr):
        if id(fr) not in slot:
            slot[id(fr)] = len(frames)
            frames.append(fr)
        return slot[id(fr)]
    desc, objects, classes, names = RC.frame_descriptors([j[0] for j in jobs], [j[1] for j in jobs], index_of, order)
    images = np.ascontiguousarray(np.stack([f['image'] for f in frames]))
    masks = np.ascontiguousarray(np.stack([f['mask'] for f in frames]))
    B, (N, H, W) = len(jobs), masks.shape
    if len(classes) == 0:
        objects, classes = np.zeros((1, 30)), np.zeros(1, np.int32)
    out = dict(images=np.full((B, H, W, 3), 0xA5, np.uint8), masks=np.full((B, H, W), 0xA5, np.uint8), beta=np.full((B, 3), np.nan),
               boxes=np.full((B, max_obj, 4), np.nan), kept=np.full((B, max_obj), -7, np.int32), n_rows=np.full(B, -7, np.int32),
               rows=np.full((B, max_obj, 15), np.nan), info=np.full((B, max_obj, 2), -7, np.int32))
    warped = np.full((B, 3, H, W, 3), np.nan, np.float32) if want_warped else None
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = lib.sgv3d_recombine_host(B, N, H, W, max_obj, int(desc['n_obj'].sum()), P(desc), P(images), P(masks), P(objects), P(classes),
                                  P(out['images']), P(out['masks']), P(out['beta']), P(out['boxes']), P(out['kept']), P(out['n_rows']),
                                  P(out['rows']), P(out['info']), P(warped) if want_warped else None)
    _lib.check(rc, "sgv3d_recombine_host")
    out['warped'], out['names'], out['desc'] = warped, names, desc
    out['lines'] = [RC.label_lines(names[b], out['rows'][b, :out['n_rows'][b]], out['info'][b, :out['n_rows'][b]]) for b in range(B)]
    return out


# ------------------------------------------------------------------------------------------------------ hand-made frames
FLAT_TR = np.eye(4)
FLAT_P2 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def flat_objects(boxes, names=None):
    """Objects whose projected float box through the flat camera (Tr = I, P2 = [I | 0], every corner at depth 1) is exactly
    ``boxes[i]`` = (xmin, ymin, xmax, ymax)."""
    n = len(boxes)
    corners = np.zeros((n, 3, 8))
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        corners[i, 0] = [x1, x1, x0, x0, x1, x1, x0, x0]
        corners[i, 1] = [y1, y0, y0, y1, y1, y0, y0, y1]
        corners[i, 2] = 1.0
    return dict(corners=corners, dim=np.full((n, 3), 2.0), truncated=np.zeros(n), occluded=np.zeros(n), score=np.ones(n),
                names=list(names) if names is not None else ["Car"] * n)


def flat_frame(boxes, h, w, names=None, image=None, mask=None, fill=0):
    """A frame seen by the flat camera: identical cameras give the identity homography and a zero shift."""
    return dict(Tr_ego2cam=FLAT_TR.copy(), P2=FLAT_P2.copy(), objects=flat_objects(boxes, names),
                image=np.full((h, w, 3), fill, np.uint8) if image is None else image,
                mask=np.zeros((h, w), np.uint8) if mask is None else mask)
