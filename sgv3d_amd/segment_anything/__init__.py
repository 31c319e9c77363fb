"""A ``segment_anything``-shaped package on this project's kernels: the names the reference's scripts/data_preprocess import
(``from segment_anything import build_sam, SamPredictor``) with SAM's module tree, so that SAM checkpoints load strictly by name.
Box prompts, float32 decoder, inference only; point and mask prompts, SAM-HQ and training are not built.

``install()`` registers the package under the name ``segment_anything`` for code that imports it by that name."""
import sys

from .build_sam import build_sam, build_sam_hq, build_sam_vit_b, build_sam_vit_h, build_sam_vit_l, sam_model_registry
from .modeling import MaskDecoder, PromptEncoder, Sam, TwoWayTransformer
from .predictor import SamPredictor
from .transforms import ResizeLongestSide

__all__ = ["build_sam", "build_sam_hq", "build_sam_vit_h", "build_sam_vit_l", "build_sam_vit_b", "sam_model_registry", "SamPredictor",
           "Sam", "PromptEncoder", "MaskDecoder", "TwoWayTransformer", "ResizeLongestSide", "install"]


def install():
    """Make ``import segment_anything`` resolve to this package (unless another one is already imported)."""
    return sys.modules.setdefault("segment_anything", sys.modules[__name__])
