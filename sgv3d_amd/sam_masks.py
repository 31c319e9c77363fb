"""The reference's mask stage (scripts/data_preprocess/recombine_utils.py: update_mask_info, get_sam_mask, mask_inference) on the
device: boxes of a pseudo-labelled frame -> SAM -> the class-id ``mask_image`` that ``FrameRecombiner.combine`` and
``recombine.write`` take, without leaving the GPU.

    predictor = SamPredictor(build_sam(checkpoint).cuda())
    boxes, labels = prompts_from_annos(annos, frame.shape[:2])
    mask = get_sam_mask(predictor, boxes, labels, frame)            # uint8 [H, W], values 0..6

The chain is the reference's: ``set_image``, ``transform.apply_boxes_torch``, ``predict_torch(boxes=..., multimask_output=False)``,
then the paint loop ``mask_image += mask * label * (mask_image == 0)`` and ``np.clip(., 0, 6)`` -- the last two inside
sgv3d_sam_mask_compose, which never writes the per-box masks.  Frames are RGB (the reference converts its BGR frame first).
"""
import numpy as np
import torch

from . import _lib

__all__ = ["class2id", "prompts_from_annos", "get_sam_mask", "mask_images"]

class2id = {"car": 6, "van": 5, "bus": 4, "truck": 3, "pedestrian": 2, "cyclist": 1, "bicycle": 1, "tricyclist": 1, "motorcycle": 1,
            "motorcyclist": 1}


def prompts_from_annos(annos, hw):
    """update_mask_info's box clamping: every annotation's ``bbox`` cast to int32, dropped when xmax <= 0 or ymax <= 0, clamped to
    [0, w - 1] x [0, h - 1]; labels by ``class2id`` of the lower-cased ``name``.  Returns (int64 tensor [n, 4], list of n labels)."""
    h, w = int(hw[0]), int(hw[1])
    boxes, labels = [], []
    for anno in annos:
        xmin, ymin, xmax, ymax = (int(v) for v in np.array(anno["bbox"]).astype(np.int32)[:4])
        if xmax <= 0 or ymax <= 0:
            continue
        boxes.append([max(0, xmin), max(0, ymin), min(xmax, w - 1), min(ymax, h - 1)])
        labels.append(class2id[anno["name"].lower()])
    return torch.tensor(np.array(boxes, np.int64).reshape(-1, 4)), labels


def _device_frames(predictor, frames, what):
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise _lib.SGV3DError(f"{what}: the frame must be a uint8 tensor on the GPU (there is no CPU fallback)")
    if frames.dtype != torch.uint8:
        raise _lib.SGV3DError(f"{what}: uint8 frames expected, got {frames.dtype}")
    return frames


def get_sam_mask(predictor, bbox_prompts, bbox_labels, frame, image_format="RGB"):
    """The reference's function of that name for one uint8 [H, W, 3] device frame: uint8 [H, W] on the device.  Boxes are painted in
    order and the first that covers a pixel owns it; a label above 6 is clipped to 6; label 0 paints nothing; no boxes: zeros."""
    frame = _device_frames(predictor, frame, "get_sam_mask")
    if frame.dim() != 3:
        raise _lib.SGV3DError(f"get_sam_mask: [H, W, 3] expected, got {tuple(frame.shape)}")
    return mask_images(predictor, frame.unsqueeze(0), [bbox_prompts], [bbox_labels], image_format)[0]


def mask_images(predictor, frames, boxes_per_frame, labels_per_frame, image_format="RGB"):
    """``get_sam_mask`` for a batch: frames uint8 [F, H, W, 3] on the device, per frame a [n, 4] box tensor / array (pixel
    coordinates of the frame) and n labels -> uint8 [F, H, W].  One encoder pass, one decoder pass over all boxes (each reads its
    frame's embedding by index), one compose launch."""
    frames = _device_frames(predictor, frames, "mask_images")
    if frames.dim() != 4 or len(boxes_per_frame) != frames.shape[0] or len(labels_per_frame) != frames.shape[0]:
        raise _lib.SGV3DError(f"mask_images: frames {tuple(frames.shape)}, {len(boxes_per_frame)} box lists, {len(labels_per_frame)} label lists")
    hw = (int(frames.shape[1]), int(frames.shape[2]))
    boxes, labels, index = [], [], []
    for f, (bx, lb) in enumerate(zip(boxes_per_frame, labels_per_frame)):
        bx = torch.as_tensor(np.asarray(bx.cpu() if isinstance(bx, torch.Tensor) else bx)).reshape(-1, 4)
        if bx.shape[0] != len(lb):
            raise _lib.SGV3DError(f"mask_images: frame {f} has {bx.shape[0]} boxes and {len(lb)} labels")
        boxes.append(bx.to(torch.float64))
        labels += [int(v) for v in lb]
        index += [f] * len(lb)
    if not labels:
        return torch.zeros(frames.shape[:3], dtype=torch.uint8, device=frames.device)
    predictor.set_images(frames, image_format)
    transformed = predictor.transform.apply_boxes_torch(torch.cat(boxes), hw).to(frames.device)
    return predictor.class_masks(transformed, labels, index)
