"""Checkpoints of the native training path in the layout the reference harness reads (pytorch-lightning 1.5.10, the
reference's requirements.txt): ``ModelCheckpoint`` files that ``trainer.test(model, ckpt_path=...)`` (``-e --ckpt_path``)
evaluates, and that a native run -- ``DataParallelAdamW`` + ``GraphedTrainStep`` -- resumes bit for bit.

File contents (``torch.save`` of a dict, CPU tensors):

* ``epoch``, ``global_step``, ``pytorch-lightning_version``;
* ``state_dict``: the model's ``state_dict()`` with ``model.`` in front of every key (the harness's ``self.model``);
* ``optimizer_states``: ``[DataParallelAdamW.state_dict()]`` -- ``torch.optim.AdamW``'s layout, so a harness run restores it
  into its own AdamW and a native run loads a harness checkpoint's AdamW state;
* ``lr_schedulers``: ``[MultiStepLR.state_dict()]`` as the reference's scheduler has it after ``epoch`` epochs;
* ``sgv3d``: format version, the run's per-layer kernel choices (``hip_ops.TUNE_DB``), torch CPU / GPU, Python and numpy random
  states, the deterministic flag and the caller's ``extra`` dict (data order).

The file is written to a temporary name and renamed, so a reader never sees half a checkpoint."""
import os
import random

import numpy as np
import torch

from . import hip_ops
from .train_step import multistep_lr

FORMAT_VERSION = 1
LIGHTNING_VERSION = "1.5.10"
PREFIX = "model."

__all__ = ['save_checkpoint', 'load_checkpoint', 'FORMAT_VERSION']


def _cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_cpu(v) for v in obj)
    return obj


def _multistep_state(base_lr, epoch, milestones, gamma):
    """``torch.optim.lr_scheduler.MultiStepLR(opt, milestones, gamma).state_dict()`` after ``epoch`` calls of ``step()``."""
    dummy = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=base_lr)
    sd = torch.optim.lr_scheduler.MultiStepLR(dummy, list(milestones), gamma).state_dict()
    sd.update(last_epoch=int(epoch), _step_count=int(epoch) + 1, _last_lr=[multistep_lr(base_lr, epoch, milestones, gamma)])
    return sd


def save_checkpoint(path, model, opt=None, *, epoch, global_step, base_lr=None, milestones=(19, 23), gamma=0.1, extra=None):
    """Write ``path`` (see the module docstring).  ``base_lr``: the scheduler's base learning rate (default ``opt.lr``)."""
    ckpt = {
        'epoch': int(epoch),
        'global_step': int(global_step),
        'pytorch-lightning_version': LIGHTNING_VERSION,
        'state_dict': {PREFIX + k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
        'optimizer_states': [] if opt is None else [_cpu(opt.state_dict())],
        'lr_schedulers': [] if opt is None else [_multistep_state(opt.lr if base_lr is None else base_lr, epoch, milestones, gamma)],
        'callbacks': {},
        'sgv3d': {
            'format_version': FORMAT_VERSION,
            'tune_db': {k: list(v) for k, v in hip_ops.TUNE_DB.items()},
            'rng': {'torch': torch.get_rng_state(),
                    'cuda': [s.cpu() for s in torch.cuda.get_rng_state_all()] if torch.cuda.is_available() else [],
                    'python': random.getstate(), 'numpy': np.random.get_state()},
            'deterministic': bool(hip_ops.deterministic()),
            'extra': dict(extra or {}),
        },
    }
    tmp = f"{path}.tmp{os.getpid()}"
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, model, opt=None, *, strict=True, restore_rng=True):
    """Load ``path`` into ``model`` (and ``opt``, a ``DataParallelAdamW`` over ``model.parameters()``) and return the meta dict
    ``{'epoch', 'global_step', 'extra', 'deterministic', 'lr_scheduler', 'optimizer_state'}``.

    The weights are copied into the existing parameters: an optimiser built before the load sees them in its buckets, one built
    after takes them up at construction (then pass ``meta['optimizer_state']`` to its ``load_state_dict``).  The checkpoint's
    per-layer kernel choices take precedence over the ones this process has, and no packed or folded weight form made from
    the weights before the load is used afterwards.  The deterministic flag is returned, not applied."""
    ckpt = torch.load(path, map_location='cpu', weights_only=False)
    sd = ckpt['state_dict']
    stripped = {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
    if strict and len(stripped) != len(sd):
        raise KeyError(f"{path}: state_dict keys without the '{PREFIX}' prefix: {sorted(set(sd) - {PREFIX + k for k in stripped})[:5]}")
    if opt is not None and opt.packs is not None:
        opt.packs.close()
    model.load_state_dict(stripped, strict=strict)
    if hasattr(model, 'refresh'):
        model.refresh()                             # packed inference weights and captured graphs of the old weights
    extra = ckpt.get('sgv3d', {})
    tune = extra.get('tune_db', {})
    if tune:
        from . import conv_grad
        for k, v in tune.items():
            hip_ops.tune_record(k, tuple(v))                # (the run's own choices: no longer arch-bound)
        conv_grad._WGRAD_DB.clear()                 # (per-shape copies of TUNE_DB entries)
    opt_states = ckpt.get('optimizer_states') or []
    if opt is not None:
        names = [n for n, _ in model.named_parameters()]
        if len(names) == len(opt.flat.all_params):
            opt.param_names = names
        if opt_states:
            opt.load_state_dict(opt_states[0])
    rng = extra.get('rng')
    if restore_rng and rng:
        torch.set_rng_state(rng['torch'])
        if rng['cuda'] and torch.cuda.is_available() and len(rng['cuda']) == torch.cuda.device_count():
            torch.cuda.set_rng_state_all(rng['cuda'])
        random.setstate(rng['python'])
        np.random.set_state(rng['numpy'])
    return {'epoch': ckpt['epoch'], 'global_step': ckpt['global_step'], 'extra': extra.get('extra', {}),
            'deterministic': extra.get('deterministic'), 'lr_scheduler': (ckpt.get('lr_schedulers') or [None])[0],
            'optimizer_state': opt_states[0] if opt_states else None}
