"""Writes tests/golden/train_augment.npz: what the reference dataset's training-time camera augmentation makes of seeded
inputs.  The reference's dataset/nusc_mv_det_dataset.py is imported with empty ``sys.modules`` stubs for the libraries the
captured functions never call (cv2, mmcv, skimage, nuscenes, pyquaternion, mmdet3d, imageio, torchvision through
dataset.transforms); its own ``img_intrin_extrin_transform`` (Pillow LANCZOS resize, paste / crop, BICUBIC rotate) and
``NuscMVDetDataset.sample_intrin_extrin_augmentation`` (through a stand-in ``self`` carrying the three ranges and the
class's ``degree2rad`` / ``get_M``) are then called as they are.  Pillow 10+ dropped ``Image.ANTIALIAS``; it is set to
``Image.LANCZOS``, the filter it named.

Image cases ``<name>``: ``<name>_src`` u8 [H, W, 3], ``<name>_out`` u8 [H, W, 3], ``<name>_args`` f64 [ratio, roll,
transform_pitch] and ``<name>_intrin`` f32 [4, 4] (the rectified intrinsics the transform reads its centre from).

Draws (``draw_*``, one row per frame of ``random.seed(SEED); np.random.seed(SEED)``, in the order dataset/...:550 and
:618-619 consume them): ``draw_ie`` / ``draw_bright`` bool, ``draw_ratio`` / ``draw_roll`` / ``draw_u`` f64 (NaN where not
drawn), ``draw_tp`` i64 transform_pitch, ``draw_intrin`` / ``draw_e2s`` f32 [n, 4, 4] the returned rectified matrices, and
``cam_intrin`` / ``cam_e2s`` f32 [4, 4] the camera they start from.

    python tests/golden/make_golden_train_augment.py /path/to/reference
"""
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261016


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Dummy:
    def __init__(self, *a, **k):
        raise RuntimeError("third-party stub called")


def import_reference(root):
    for name in ('cv2', 'mmcv', 'imageio', 'skimage', 'nuscenes', 'nuscenes.utils', 'pyquaternion', 'mmdet3d',
                 'mmdet3d.core', 'mmdet3d.core.bbox', 'mmdet3d.core.bbox.structures'):
        _stub(name)
    _stub('skimage.transform', rotate=_Dummy, warp=_Dummy, resize=_Dummy)
    _stub('mmdet3d.core.bbox.structures.lidar_box3d', LiDARInstance3DBoxes=_Dummy)
    _stub('nuscenes.utils.data_classes', Box=_Dummy)
    sys.modules['pyquaternion'].Quaternion = _Dummy
    _stub('dataset')
    _stub('dataset.transforms', ResizeLongestSide=_Dummy)
    import importlib.util
    spec = importlib.util.spec_from_file_location('nusc_mv_det_dataset',
                                                  os.path.join(root, 'dataset', 'nusc_mv_det_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def camera(h, w):
    """Roadside-like camera scaled to an h x w frame: pinhole K and an ego -> sensor pose looking down at the road."""
    f = 1.1 * w
    K = np.eye(4, dtype=np.float32)
    K[:3, :3] = [[f, 0, 0.497 * w + 0.31], [0, f * 1.002, 0.503 * h - 0.27], [0, 0, 1]]
    c, s = np.cos(0.2), np.sin(0.2)
    rot = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64)         # ego x forward -> camera z
    tilt = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    e2s = np.eye(4, dtype=np.float32)
    e2s[:3, :3] = tilt @ rot
    e2s[:3, 3] = (tilt @ rot) @ -np.array([0.4, -0.1, 6.2])
    return K, e2s


# name: (H, W), ratio, roll (deg), transform_pitch, kind
CASES = {
    'down': ((90, 160), 0.83, 1.3, 2, 'rgb'),                  # ratio < 1: paste into a black canvas
    'up': ((90, 160), 1.21, -2.4, -3, 'rgb'),                  # ratio > 1: crop of the enlarged frame
    'one_axis': ((90, 160), 1.0065, 0.7, 0, 'rgb'),            # width changes (160 -> 161), height stays 90
    'large_kernel': ((135, 240), 0.3, -0.9, 1, 'rgb'),         # Lanczos support 10: ksize 21
    'unit': ((108, 192), 1.0, 3.1, -1, 'rgb'),                 # no resize, rotation only
    'pitch_off': ((90, 160), 0.97, -1.7, 61, 'rgb'),           # translate pushes most of the frame off
    'mask': ((90, 160), 0.88, 2.2, -4, 'mask'),                # 3-channel label mask
}
N_DRAWS = 20


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('SGV3D_REFERENCE', '')
    ref = import_reference(root)
    Image.ANTIALIAS = Image.LANCZOS
    rng = np.random.default_rng(SEED)
    out = {}
    for name, ((h, w), ratio, roll, tp, kind) in CASES.items():
        if kind == 'mask':
            src = np.repeat(np.repeat(rng.integers(0, 7, (h // 6 + 1, w // 8 + 1, 3)) * 40 + 10, 6, 0), 8, 1)[:h, :w]
            src = src.astype(np.uint8)
        else:   # smooth content plus noise: exercises the filters' negative lobes and the clamps
            yy, xx = np.mgrid[0:h, 0:w]
            base = 128 + 100 * np.sin(xx[..., None] / (5.0 + np.arange(3)) + yy[..., None] / 7.0)
            src = np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
        K, _ = camera(h, w)
        res = np.array(ref.img_intrin_extrin_transform(Image.fromarray(src), ratio, roll, tp, K))
        out[f'{name}_src'] = src
        out[f'{name}_out'] = res
        out[f'{name}_args'] = np.array([ratio, roll, tp], np.float64)
        out[f'{name}_intrin'] = K

    K, e2s = camera(1080, 1920)
    this = types.SimpleNamespace(ratio_range=[1.0, 0.20], roll_range=[0.0, 2.00], pitch_range=[0.0, 0.67])
    this.degree2rad = types.MethodType(ref.NuscMVDetDataset.degree2rad, this)
    this.get_M = types.MethodType(ref.NuscMVDetDataset.get_M, this)
    random.seed(SEED)
    np.random.seed(SEED)
    d = {k: [] for k in ('ie', 'bright', 'ratio', 'roll', 'u', 'tp', 'intrin', 'e2s')}
    for _ in range(N_DRAWS):
        ie = random.random() < 0.5
        if ie:
            Ki, Ei, ratio, roll, tp = ref.NuscMVDetDataset.sample_intrin_extrin_augmentation(
                this, torch.from_numpy(K), torch.from_numpy(e2s))
            Ki, Ei = Ki.numpy(), Ei.numpy()
        else:
            Ki, Ei, ratio, roll, tp = K, e2s, np.nan, np.nan, 0
        bright = random.random() < 0.3
        u = random.random() if bright else np.nan
        for k, v in (('ie', ie), ('bright', bright), ('ratio', ratio), ('roll', roll), ('u', u), ('tp', tp),
                     ('intrin', Ki), ('e2s', Ei)):
            d[k].append(v)
    for k, dt in (('ie', bool), ('bright', bool), ('ratio', np.float64), ('roll', np.float64), ('u', np.float64),
                  ('tp', np.int64), ('intrin', np.float32), ('e2s', np.float32)):
        out[f'draw_{k}'] = np.asarray(d[k], dt)
    out['cam_intrin'] = K
    out['cam_e2s'] = e2s
    out['draw_seed'] = np.array(SEED, np.int64)
    np.savez_compressed(os.path.join(HERE, 'train_augment.npz'), **out)


if __name__ == '__main__':
    main()
