"""Writes tests/golden/sam_masks.npz:

  ``resize_src_<HxW>_<hxw>`` u8 [H, W, 3], ``resize_out_<HxW>_<hxw>`` u8 [h, w, 3]
        Pillow's ``Image.resize((w, h), Image.BILINEAR)`` of small seeded frames: 135x240 -> 54x96, 27x48 -> 54x96, 40x63 -> 61x96 and
        one odd pair per axis (37x96 -> 23x96, 54x61 -> 54x35)
  ``paint_rects`` i32 [n, 4] (x0, y0, x1, y1, inclusive), ``paint_labels`` i32 [n], ``paint_out`` u8 [1080, 1920]
        the reference's own ``get_sam_mask`` (scripts/data_preprocess/recombine_utils.py, imported with the ``sys.modules`` stubs of
        make_golden_recombine.py) with its ``mask_inference`` replaced by a function that returns prepared boolean masks [n, 1, 1080,
        1920], one filled rectangle per box: overlapping boxes, a label above 6, a label 0 under a later box
  ``empty_out_sum``   the sum of its output for the ``[[0, 0, 0, 0]]`` / label 0 call with an all-true prepared mask, and
  ``noboxes_out_sum`` for a [0, 4] prompt tensor: both 0

PATCHED (``patched`` in the fixture says so): ``mask_inference``.  No program text is stored.

    python tests/golden/make_golden_sam_masks.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_recombine import import_reference        # noqa: E402

RESIZES = [((135, 240), (54, 96)), ((27, 48), (54, 96)), ((40, 63), (61, 96)), ((37, 96), (23, 96)), ((54, 61), (54, 35))]
RECTS = np.array([[100, 80, 700, 500], [400, 300, 1200, 900], [1000, 100, 1500, 400], [1100, 200, 1919, 1079], [50, 600, 300, 900]], np.int32)
LABELS = np.array([9, 2, 0, 5, 3], np.int32)


def smooth_frame(rng, h, w):
    """Low-frequency colour plus noise: neighbouring pixels differ, so every coefficient matters."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 100 * np.sin(xx / (3.0 + c) + c) * np.cos(yy / (4.0 + c)) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('SGV3D_REFERENCE', '')
    ref = import_reference(root)
    out = {'patched': np.array("mask_inference: prepared boolean masks")}
    rng = np.random.default_rng(20261020)
    for (h, w), (oh, ow) in RESIZES:
        src = smooth_frame(rng, h, w)
        tag = f"{h}x{w}_{oh}x{ow}"
        out["resize_src_" + tag] = src
        out["resize_out_" + tag] = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))

    def prepared(rects):
        m = torch.zeros(len(rects), 1, 1080, 1920, dtype=torch.bool)
        for i, (x0, y0, x1, y1) in enumerate(rects):
            m[i, 0, y0:y1 + 1, x0:x1 + 1] = True
        return m

    ref.mask_inference = lambda predictor, bboxes, image: prepared(RECTS)
    got = ref.get_sam_mask(None, torch.tensor(RECTS), LABELS.tolist(), None)
    assert got.shape == (1080, 1920, 1) and got.dtype == np.uint8
    out['paint_rects'], out['paint_labels'], out['paint_out'] = RECTS, LABELS, got[..., 0]
    ref.mask_inference = lambda predictor, bboxes, image: torch.ones(1, 1, 1080, 1920, dtype=torch.bool)
    out['empty_out_sum'] = np.array(int(ref.get_sam_mask(None, torch.tensor([[0, 0, 0, 0]]), [0], None).sum()))
    out['noboxes_out_sum'] = np.array(int(ref.get_sam_mask(None, torch.zeros(0, 4), [], None).sum()))
    np.savez_compressed(os.path.join(HERE, 'sam_masks.npz'), **out)


if __name__ == '__main__':
    main()
