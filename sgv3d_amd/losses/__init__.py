"""Mirror of the reference's ``losses`` package for the pieces the SGV3D configs use (losses/__init__.py:1-4):
``FocalLoss`` (csrc/bsm_train.hip) and ``DiceLoss`` (csrc/dice_loss.hip) on the MI355X plus the semantic supervision of the BSM
experiment and the embedding distillation of the reference's assist branch (``EmbedDistillation``, csrc/embed_distill.hip)."""
from .focal import BINARY_MODE, MULTICLASS_MODE, MULTILABEL_MODE, FocalLoss, focal_loss_with_logits
from .dice import DiceLoss
from .distill import EmbedDistillation
from .semantic import SemanticSupervision, downsample_gt_semantic

__all__ = ['BINARY_MODE', 'MULTICLASS_MODE', 'MULTILABEL_MODE', 'FocalLoss', 'DiceLoss', 'EmbedDistillation', 'focal_loss_with_logits',
           'SemanticSupervision', 'downsample_gt_semantic']
