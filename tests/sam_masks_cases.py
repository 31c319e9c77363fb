"""The cases the SAM mask tests share (tests/test_sam_masks_cpu.py, tests/test_sam_masks_gpu.py): attention shapes, seeded decoder
models with their inputs, compose inputs.  A case's float64 and float32 restatement runs are computed once per process."""
import functools
import os
from collections import namedtuple

import numpy as np
import torch

import sam_ref

HERE = os.path.dirname(os.path.abspath(__file__))

# (Nq, Nk, head_dim, batch): the few-queries kernel at one split with and without a ragged last wave, at the 64-key wave edges, at
# sixteen splits; the few-keys kernel with one and many workgroups; both head dimensions; a single query on a single key
ATTENTION_SHAPES = [(7, 36, 16, 1), (7, 81, 16, 1), (7, 63, 16, 1), (7, 64, 16, 1), (7, 65, 16, 1), (7, 4096, 16, 2), (7, 7, 32, 1),
                    (1, 1, 32, 1), (36, 7, 16, 1), (4096, 7, 16, 1)]

DecoderCase = namedtuple("DecoderCase", "name grid boxes frames original multimask seed")
# transformer_dim 256, 8 heads, depth 2, mlp_dim 2048.  The seeds are chosen so that the float64 restatement alone keeps the share
# of pixels whose logit lies within the bar of zero under 0.5 % (tests/test_sam_masks_cpu.py asserts it).
DECODER_CASES = [
    DecoderCase("grid6_1box", 6, 1, 1, (54, 96), False, 11),
    DecoderCase("grid6_3boxes_2frames", 6, 3, 2, (54, 96), True, 12),
    DecoderCase("grid9_1box", 9, 1, 1, (81, 131), False, 13),
    DecoderCase("grid9_3boxes_2frames", 9, 3, 2, (81, 131), False, 14),
    DecoderCase("grid64_2boxes", 64, 2, 1, (135, 240), False, 15),
]
WHOLE_SEED = 21
COMPOSE_SIZES = [(54, 96), (27, 48), (135, 240)]


@functools.lru_cache(maxsize=None)
def decoder_case(case):
    """(float64 restatement without an encoder, embedding f64 [F, g, g, 256], boxes f64 [B, 4] in the input frame, frame of each box)."""
    model = sam_ref.randomize_(sam_ref.build(img_size=16 * case.grid, with_encoder=False), case.seed).double()
    g = torch.Generator().manual_seed(case.seed + 1000)
    emb = torch.randn(case.frames, case.grid, case.grid, 256, generator=g, dtype=torch.float64)
    pre = sam_ref.get_preprocess_shape(case.original[0], case.original[1], 16 * case.grid)
    lo = torch.rand(case.boxes, 2, generator=g, dtype=torch.float64) * 0.5
    hi = lo + 0.2 + torch.rand(case.boxes, 2, generator=g, dtype=torch.float64) * 0.3
    scale = torch.tensor([pre[1] - 1, pre[0] - 1], dtype=torch.float64)
    boxes = torch.cat([lo * scale, hi * scale], 1).float().double()       # float32 values: what the device is given
    frames = [i % case.frames for i in range(case.boxes)]
    return model, emb, boxes, frames


_RUNS = {}


def run_ref(model64, emb, boxes, frames, dtype, multimask):
    """(low-res logits, iou) of the restatement in ``dtype`` on the CPU, kept per (model, inputs, dtype)."""
    key = (id(model64), id(emb), id(boxes), tuple(frames), dtype, multimask)
    if key not in _RUNS:
        import copy
        m = model64 if dtype == torch.float64 else copy.deepcopy(model64).float()
        with torch.no_grad():
            _RUNS[key] = (m, emb, boxes) + tuple(m.low_res(emb.to(dtype), boxes.to(dtype), frames, multimask))
    return _RUNS[key][3:]


def compose_case(hw, low):
    """Three frames: frame 0 has overlapping boxes (a label above 6 first, then 2, then a label 0 that paints nothing over a 5), frame 1
    none, frame 2 a box on the last row and column.  Smooth random logits plus rectangles."""
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    def blob(y0, y1, x0, x1):
        a = rng.normal(0, 0.3, (low, low)).astype(np.float32) - 1.0
        a[y0:y1, x0:x1] += 2.5
        return a
    pre_h = int(hw[0] * (4.0 * low / max(hw)) + 0.5) // 4            # rows of the low-res map the frame covers
    logits = np.stack([blob(2, 8, 3, 12), blob(5, 11, 8, 20), blob(1, 6, 1, 6), blob(1, 6, 1, 6), blob(max(pre_h - 4, 0), low, low - 6, low)])
    labels = [9, 2, 0, 5, 3]
    frames = [0, 0, 0, 0, 2]
    return logits, labels, frames, 3


def golden():
    return np.load(os.path.join(HERE, "golden", "sam_masks.npz"))


def whole_frame():
    """The 135 x 240 frame of the resize fixture (its preprocess shape at img_size 96 is 54 x 96) and three pixel boxes."""
    return golden()["resize_src_135x240_54x96"], [[20, 15, 150, 100], [100, 40, 239, 134], [0, 0, 60, 60]]


def preprocessed(frames_u8, size):
    """uint8 [F, H, W, 3] -> f64 [F, 3, h, w] at the preprocess shape, through the coefficient tables the Pillow fixture pins."""
    from sgv3d_amd.segment_anything import ops
    pre = sam_ref.get_preprocess_shape(frames_u8.shape[1], frames_u8.shape[2], size)
    out = np.stack([ops.resize_bilinear_u8_host(f, pre) for f in frames_u8])
    return torch.from_numpy(out).permute(0, 3, 1, 2).double()


@functools.lru_cache(maxsize=None)
def _whole(model_id):
    return {}


def whole_reference(ref64, frame, boxes):
    """(low64, iou64, low32, iou32, float64 full-size logits [B, 1, H, W]) of the whole path on ``frame``."""
    import copy
    cache = _whole(id(ref64))
    if not cache:
        hw = frame.shape[:2]
        tb = sam_ref.apply_boxes(torch.tensor(boxes), hw, 96)
        x = torch.from_numpy(golden()["resize_out_135x240_54x96"]).permute(2, 0, 1).unsqueeze(0).double()
        with torch.no_grad():
            low64, iou64 = ref64.low_res(ref64.image_encoder(x), tb.double(), [0] * len(boxes))
            m32 = copy.deepcopy(ref64).float()
            low32, iou32 = m32.low_res(m32.image_encoder(x.float()), tb, [0] * len(boxes))
            out64 = sam_ref.postprocess_masks(low64, 96, x.shape[-2:], hw)
        cache["v"] = (low64, iou64, low32, iou32, out64)
    return cache["v"]
