"""``ResizeLongestSide`` of segment_anything.utils.transforms: the preprocess shape, box coordinates in the resized frame, and the
image resize itself -- Pillow's BILINEAR, which is what upstream's ``resize(to_pil_image(image), target_size)`` runs."""
import numpy as np
import torch

from . import ops


class ResizeLongestSide:
    def __init__(self, target_length: int) -> None:
        self.target_length = target_length

    @staticmethod
    def get_preprocess_shape(oldh: int, oldw: int, long_side_length: int):
        scale = long_side_length * 1.0 / max(oldh, oldw)
        newh, neww = oldh * scale, oldw * scale
        return (int(newh + 0.5), int(neww + 0.5))

    def apply_image(self, image):
        """uint8 [H, W, 3] -> uint8 [h, w, 3] at the preprocess shape.  A device tensor comes back as a device tensor; a numpy array
        is resized on the device and comes back as a numpy array (there is no CPU path)."""
        if isinstance(image, np.ndarray):
            return self.apply_image(torch.from_numpy(np.ascontiguousarray(image)).cuda()).cpu().numpy()
        size = self.get_preprocess_shape(int(image.shape[0]), int(image.shape[1]), self.target_length)
        chw = ops.resize_bilinear_u8(image.unsqueeze(0).contiguous(), size)[0]
        return chw.permute(1, 2, 0).to(torch.uint8).contiguous()

    def apply_coords_torch(self, coords: torch.Tensor, original_size) -> torch.Tensor:
        old_h, old_w = original_size
        new_h, new_w = self.get_preprocess_shape(int(old_h), int(old_w), self.target_length)
        coords = coords.detach().clone().to(torch.float)
        coords[..., 0] = coords[..., 0] * (new_w / old_w)
        coords[..., 1] = coords[..., 1] * (new_h / old_h)
        return coords

    def apply_boxes_torch(self, boxes: torch.Tensor, original_size) -> torch.Tensor:
        """(x0, y0, x1, y1) boxes of the original frame -> float32 boxes of the resized frame: x * new_w / old_w, y * new_h / old_h."""
        return self.apply_coords_torch(boxes.reshape(-1, 2, 2), original_size).reshape(-1, 4)
