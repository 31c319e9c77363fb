"""Golden data of the renderer (tests/test_render_cpu.py) -> render.npz.

* Pillow's ``ImageDraw.line(width=1)`` pixels of some hundreds of integer segments on 17 x 23, 9 x 31 and 40 x 40 canvases.  The
  renderer has its own line rule (DESIGN.md "Rendering detections"); Pillow bounds it from both sides: every Pillow pixel is
  covered by the rule at t = 1 (endpoints up to 10 pixels outside included), and for segments whose endpoints lie inside the
  canvas the rule's pixels lie inside Pillow's line dilated by 3 x 3.  The maker asserts both and REPORTS a violation instead of
  dropping the case.
* The reference's own ``get_lidar_3d_8points``, ``read_label_bboxes`` and ``PointCloudFilter.pcl2xy_plane`` outputs
  (evaluators/result2kitti.py, evaluators/utils.py) for a dozen boxes and one label file.  Needs the reference checkout, as
  make_golden_aux.py does; run from the repository root:  python tests/golden/make_golden_render.py"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_aux as AUX  # noqa: E402
import render_ref as R  # noqa: E402

CANVASES = [(17, 23), (9, 31), (40, 40)]                # (height, width)


def pillow_line(h, w, a, b):
    img = Image.new('L', (w, h), 0)
    ImageDraw.Draw(img).line([tuple(int(v) for v in a), tuple(int(v) for v in b)], fill=255, width=1)
    return np.asarray(img) > 0


def dilate3(m):
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def make_lines(out):
    rng = np.random.default_rng(20241021)
    segs, shapes, pix = [], [], []
    violations = []
    for h, w in CANVASES:
        cases = [((0, 0), (w - 1, h - 1)), ((0, h - 1), (w - 1, 0)), ((3, 4), (3, 4)), ((0, 2), (w - 1, 2)), ((5, 0), (5, h - 1)),
                 ((1, 1), (2, h - 2)), ((w - 2, 1), (1, 2)), ((-7, 3), (w + 6, h - 4)), ((4, -10), (6, h + 9))]
        for _ in range(110):
            inside = rng.random() < 0.6
            lo, hi_x, hi_y = (0, w, h) if inside else (-10, w + 10, h + 10)
            cases.append(((int(rng.integers(lo, hi_x)), int(rng.integers(lo, hi_y))), (int(rng.integers(lo, hi_x)), int(rng.integers(lo, hi_y)))))
        for a, b in cases:
            pil = pillow_line(h, w, a, b)
            rule = R.covered(h, w, a, b, 1)
            if (pil & ~rule).any():
                violations.append(("pillow pixel not covered at t = 1", h, w, a, b))
            inside = 0 <= a[0] < w and 0 <= b[0] < w and 0 <= a[1] < h and 0 <= b[1] < h
            if inside and (rule & ~dilate3(pil)).any():
                violations.append(("rule pixel outside Pillow's line dilated 3 x 3", h, w, a, b))
            segs.append([*a, *b])
            shapes.append([h, w])
            pix.append(np.packbits(pil.reshape(-1)))
    for v in violations:
        print("VIOLATION:", v)
    out['line_segments'] = np.array(segs, np.int32)
    out['line_shapes'] = np.array(shapes, np.int32)
    out['line_offsets'] = np.cumsum([0] + [len(p) for p in pix]).astype(np.int64)
    out['line_pixels'] = np.concatenate(pix)                 # np.packbits of each canvas, row major
    print(f"lines: {len(segs)} segments, {len(violations)} violations")
    return violations


LABEL_TEXT = """Car 0 0 1.61 700.1 400.2 800.3 480.4 1.52 1.83 4.31 -3.21 2.4 31.7 1.49
Pedestrian 0 1 -0.3 100.0 300.0 130.0 380.0 1.71 0.62 0.55 6.02 2.9 18.44 -0.41
Cyclist 0 0 3.9 900.5 500.5 950.5 560.5 1.6 0.7 1.8 2.5 3.1 25.25 0.9
Car 0 2 0.2 0 0 0 0 0 0 0 1.0 2.0 10.0 0.3
Truck 1 0 -2.8 1200.0 350.0 1500.0 600.0 3.4 2.6 9.87 -8.13 1.7 44.9 -7.1
"""


def make_reference(out):
    AUX._numba_stub()
    for name in ('cv2', 'mmcv', 'skimage', 'skimage.io'):
        sys.modules.setdefault(name, types.ModuleType(name))
    pq = types.ModuleType('pyquaternion')
    pq.Quaternion = object
    sys.modules.setdefault('pyquaternion', pq)
    sys.path.insert(0, AUX.REF)
    r2k = importlib.import_module('evaluators.result2kitti')
    utils = importlib.import_module('evaluators.utils')
    rng = np.random.default_rng(77)
    # get_lidar_3d_8points([w, l, h], yaw, centre): the box demo=True draws; rows (size3, yaw, centre3)
    rows = np.concatenate([rng.uniform(0.4, 9.0, (12, 3)), rng.uniform(-3.3, 3.3, (12, 1)), rng.uniform(-40, 90, (12, 2)),
                           rng.uniform(-2, 3, (12, 1))], 1)
    rows[0, 3] = 0.0
    rows[1, :3] = 0.0                                       # zero extents
    out['corner_inputs'] = rows
    out['corner_outputs'] = np.stack([np.asarray(r2k.get_lidar_3d_8points(list(r[:3]), float(r[3]), list(r[4:7]))) for r in rows])
    # pcl2xy_plane of those corners on pcd_vis's canvas and on a small one
    for tag, (side, fwd, res) in (('default', ((-60, 60), (0, 100), 0.1)), ('small', ((-6, 6), (0, 20), 0.25))):
        pf = utils.PointCloudFilter(side_range=side, fwd_range=fwd, res=res)
        xy = [pf.pcl2xy_plane(np.asarray(c)[:, 0], np.asarray(c)[:, 1]) for c in out['corner_outputs']]
        out[f'bev_{tag}_x'] = np.stack([np.asarray(x).reshape(-1) for x, _ in xy]).astype(np.int64)
        out[f'bev_{tag}_y'] = np.stack([np.asarray(y).reshape(-1) for _, y in xy]).astype(np.int64)
        out[f'bev_{tag}_shape'] = np.array(pf.get_meshgrid().shape, np.int64)
        out[f'bev_{tag}_cfg'] = np.array([side[0], side[1], fwd[0], fwd[1], res], np.float64)
    # read_label_bboxes on one label file
    pitch = np.deg2rad(11.0)
    Tr = np.eye(4)
    Tr[:3, :3] = np.array([[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]]) @ \
        np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    Tr[:3, 3] = [0.05, 6.1, 0.3]
    cam2lidar = np.linalg.inv(Tr)
    with tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False) as f:
        f.write(LABEL_TEXT)
    boxes = r2k.read_label_bboxes(f.name, cam2lidar)
    os.unlink(f.name)
    out['label_text'] = np.array(LABEL_TEXT)
    out['label_cam2lidar'] = cam2lidar
    out['label_corners'] = np.stack([np.asarray(b) for b in boxes])
    print("reference: corners", out['corner_outputs'].shape, "label boxes", out['label_corners'].shape)


if __name__ == "__main__":
    out = {}
    make_lines(out)
    make_reference(out)
    np.savez_compressed(os.path.join(AUX.OUT, "render.npz"), **out)
    print("render.npz:", os.path.getsize(os.path.join(AUX.OUT, "render.npz")), "bytes")
