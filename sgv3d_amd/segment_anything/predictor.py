"""``SamPredictor`` of the segment_anything package for box prompts, plus ``set_images``: a batch of frames whose boxes carry a
frame index, so that the decoder reads each box's image embedding by index."""
import numpy as np
import torch

from .. import _lib
from . import ops
from .modeling import Sam
from .transforms import ResizeLongestSide


class SamPredictor:
    def __init__(self, sam_model: Sam) -> None:
        self.model = sam_model
        self.transform = ResizeLongestSide(sam_model.image_encoder.img_size)
        self.reset_image()

    @property
    def device(self):
        return self.model.device

    def reset_image(self) -> None:
        self.is_image_set = False
        self._features = None
        self.original_size = self.input_size = None
        self._frame0 = None

    @property
    def features(self):
        """[F, C, h, w], a permuted view of the NHWC embedding."""
        return None if self._features is None else self._features.permute(0, 3, 1, 2)

    def _frames(self, image, what):
        if isinstance(image, np.ndarray):
            image = torch.from_numpy(np.ascontiguousarray(image)).to(self.device)
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise _lib.SGV3DError(f"{what}: the image must be a numpy array or a tensor on the GPU (there is no CPU fallback)")
        if image.dtype != torch.uint8 or image.shape[-1] != 3:
            raise _lib.SGV3DError(f"{what}: uint8 [..., H, W, 3] expected, got {image.dtype} {tuple(image.shape)}")
        return image.contiguous()

    def set_image(self, image, image_format: str = "RGB") -> None:
        """uint8 [H, W, 3] (device tensor or numpy array): Pillow's BILINEAR resize to the preprocess shape, then normalise, zero-pad
        and encode."""
        image = self._frames(image, "SamPredictor.set_image")
        if image.dim() != 3:
            raise _lib.SGV3DError(f"SamPredictor.set_image: [H, W, 3] expected, got {tuple(image.shape)}")
        self.set_images(image.unsqueeze(0), image_format)

    def set_images(self, frames, image_format: str = "RGB") -> None:
        """uint8 [F, H, W, 3]: every frame is resized and encoded; ``predict_torch(..., frame_index=)`` names each box's frame."""
        assert image_format in ("RGB", "BGR"), f"image_format must be in ['RGB', 'BGR'], is {image_format}."
        frames = self._frames(frames, "SamPredictor.set_images")
        if frames.dim() != 4:
            raise _lib.SGV3DError(f"SamPredictor.set_images: [F, H, W, 3] expected, got {tuple(frames.shape)}")
        hw = (int(frames.shape[1]), int(frames.shape[2]))
        size = self.transform.get_preprocess_shape(hw[0], hw[1], self.transform.target_length)
        x = ops.resize_bilinear_u8(frames, size, swap_rb=image_format != self.model.image_format)
        self.set_torch_image(x, hw)

    def set_torch_image(self, transformed_image: torch.Tensor, original_image_size) -> None:
        """[F, 3, h, w] float (0..255, already resized so that the long side is the encoder's image size)."""
        ops.require_f32(transformed_image, "SamPredictor.set_torch_image")
        assert (
            len(transformed_image.shape) == 4
            and transformed_image.shape[1] == 3
            and max(*transformed_image.shape[2:]) == self.model.image_encoder.img_size
        ), f"set_torch_image input must be BCHW with long side {self.model.image_encoder.img_size}."
        self.reset_image()
        self.original_size = (int(original_image_size[0]), int(original_image_size[1]))
        self.input_size = tuple(int(s) for s in transformed_image.shape[-2:])
        self._features = self.model.image_encoder.embed(transformed_image)
        self.is_image_set = True

    def get_image_embedding(self) -> torch.Tensor:
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) to generate an embedding.")
        return self.features

    def _frame_index(self, frame_index, boxes):
        """int32 device tensor [B].  A list / array / CPU tensor is checked here; a device tensor is taken as it is (the kernels clamp
        it to the frames that are set), which keeps the call free of host synchronisation."""
        n, f = int(boxes.shape[0]), int(self._features.shape[0])
        if frame_index is None:
            if f != 1:
                raise _lib.SGV3DError(f"SamPredictor: {f} frames are set, frame_index must say which frame each box is in")
            if self._frame0 is None or self._frame0.numel() != n:
                self._frame0 = torch.zeros(n, dtype=torch.int32, device=boxes.device)
            return self._frame0
        if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:
            if frame_index.dtype != torch.int32 or frame_index.numel() != n or not frame_index.is_contiguous():
                raise _lib.SGV3DError("SamPredictor: a device frame_index must be a contiguous int32 tensor with one entry per box")
            return frame_index
        idx = np.asarray(frame_index.cpu() if isinstance(frame_index, torch.Tensor) else frame_index).astype(np.int64).reshape(-1)
        if idx.size != n or (n and (idx.min() < 0 or idx.max() >= f)):
            raise _lib.SGV3DError(f"SamPredictor: frame_index must hold one index in [0, {f}) per box ({n} boxes)")
        return torch.from_numpy(idx.astype(np.int32)).to(boxes.device)

    def _low_res(self, boxes, frame_index, multimask_output):
        if not self.is_image_set:
            raise RuntimeError("An image must be set with .set_image(...) before mask prediction.")
        ops.require_f32(boxes, "SamPredictor.predict_torch")
        if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] == 0:
            raise _lib.SGV3DError(f"SamPredictor.predict_torch: boxes [B, 4] with B > 0 expected, got {tuple(boxes.shape)}")
        m = self.model
        fob = self._frame_index(frame_index, boxes)
        tokens = m.prompt_encoder.box_tokens(boxes, m.mask_decoder.iou_token.weight, m.mask_decoder.mask_tokens.weight)
        return m.mask_decoder(self._features, fob, m.prompt_encoder.get_dense_pe_nhwc(), tokens,
                              m.prompt_encoder.no_mask_embed.weight, multimask_output), fob

    def predict_torch(self, point_coords, point_labels, boxes=None, mask_input=None, multimask_output: bool = True,
                      return_logits: bool = False, frame_index=None):
        """boxes [B, 4] float32 on the device, in the resized frame (``transform.apply_boxes_torch``).  Returns
        (masks [B, n, H, W] bool, or float with ``return_logits``; iou_predictions [B, n]; low_res_masks [B, n, 4h, 4w])."""
        if point_coords is not None or point_labels is not None:
            raise NotImplementedError("SamPredictor.predict_torch: point_coords (point prompts) are not built; the reference only passes boxes")
        if mask_input is not None:
            raise NotImplementedError("SamPredictor.predict_torch: mask_input (mask prompts) is not built; the reference only passes boxes")
        if boxes is None:
            raise NotImplementedError("SamPredictor.predict_torch: a boxes prompt is required")
        (low, iou), _ = self._low_res(boxes, frame_index, multimask_output)
        b, n, s, _ = (int(v) for v in low.shape)
        mode = ops.COMPOSE_LOGIT if return_logits else ops.COMPOSE_BOOL
        masks = ops.mask_compose(mode, low.view(b * n, s, s), self.model.image_encoder.img_size, self.input_size, self.original_size)
        return masks.view(b, n, *self.original_size), iou, low

    def class_masks(self, boxes, labels, frame_index=None):
        """The paint loop of the reference's get_sam_mask over the set frames: boxes [B, 4] as for ``predict_torch``, labels (list or
        int32 device tensor [B]) -> uint8 [F, H, W]; in each frame the first box, in order, that covers a pixel with a non-zero
        label owns it, the value clipped to 0..6.  One compose launch, no per-box mask is written."""
        (low, _), fob = self._low_res(boxes, frame_index, False)
        b, _, s, _ = (int(v) for v in low.shape)
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda):
            labels = torch.tensor([int(v) for v in labels], dtype=torch.int32, device=boxes.device)
        return ops.mask_compose(ops.COMPOSE_CLASS, low.view(b, s, s), self.model.image_encoder.img_size, self.input_size, self.original_size,
                                labels=labels.contiguous(), frame_of_box=fob, frames=int(self._features.shape[0]))
