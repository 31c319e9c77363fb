"""``BEVHeight`` — the detector facade, drop-in for the reference's models/bev_height.py:11-126.

Same constructor (``backbone_conf``, ``head_conf``, ``is_train_height``, ``checkpoint``), same
``forward(x, mats_dict, timestamps=None)`` return structure, same attribute paths
(``.backbone.img_backbone`` ..., ``.head``) and parameter names, so the reference's Lightning
module can do ``self.model = BEVHeight(self.backbone_conf, self.head_conf)`` unchanged
(exps/bevheight/dair-v2x/bev_height_lss_r50_864_1536_256x256.py:209) and load its checkpoints.

The forward is one stream of hand-written gfx950 kernels; between backbone and head the BEV map
stays in the NHWC buffer voxel pooling produced (the reference permutes it to NCHW and makes it
contiguous, layers/backbones/lss_fpn.py:495, only for cuDNN's benefit).
"""
import os
import weakref

import torch
from torch import nn

from .. import hip_ops
from .. import host_ext as _host_ext
from ..calibration import tensor_version
from ..layers.backbones.bsm_lss_fpn import BSMLSSFPN
from ..layers.backbones.lss_fpn import LSSFPN
from ..layers.blocks import HipModule
from ..layers.heads.bev_height_head import BEVHeightHead

__all__ = ['BEVHeight']

# Bumped whenever a module that belongs to a LIVE BEVHeight tree registers a parameter, a buffer or a sub-module (torch's global
# registration hooks; they also fire for attribute assignment and for load_state_dict(assign=True)): BEVHeight._stamp redoes its walk.
# The hooks are process-wide by torch's design, so they are installed with the first BEVHeight instance, removed with the last, and
# ignore every module that is not in such a tree (`_TRACKED`: ids of the modules of the live instances' last walks; a module that
# is attached to a tree later announces itself through the registration on its -- tracked -- parent).
_REGISTRATIONS = [0]
_TRACKED = set()
_LIVE = weakref.WeakSet()
_HOOKS = []


def _count_registration(module, name, value):
    if id(module) in _TRACKED:
        _REGISTRATIONS[0] += 1


def _install_hooks():
    if not _HOOKS:
        _HOOKS.extend([nn.modules.module.register_module_parameter_registration_hook(_count_registration),
                       nn.modules.module.register_module_buffer_registration_hook(_count_registration),
                       nn.modules.module.register_module_module_registration_hook(_count_registration)])


def _instance_gone():
    """A BEVHeight instance was collected: with no instance left the hooks go; otherwise the tracked set is rebuilt by the
    survivors' next walks."""
    _TRACKED.clear()
    alive = list(_LIVE)                   # (iteration skips the dying instance: its weak references are cleared already)
    if not alive:
        for h in _HOOKS:
            h.remove()
        _HOOKS.clear()
    else:
        for m in alive:
            m._flat_dirty = True


class BEVHeight(nn.Module):
    """Detector = camera backbone (``LSSFPN`` or, with ``backbone_conf['is_bsm']``, ``BSMLSSFPN``) + BEV head.

    ``backbone_conf`` / ``head_conf`` are the experiment files' dicts, taken verbatim; ``is_train_height``
    makes the training-mode forward return ``(preds, height_pred)`` as models/bev_height.py:72-77 does;
    ``checkpoint`` optionally names a Lightning checkpoint whose ``model.backbone.*`` entries initialise the
    backbone."""

    def __init__(self, backbone_conf, head_conf, is_train_height=False, checkpoint=None):
        super(BEVHeight, self).__init__()
        if backbone_conf['is_bsm']:
            self.backbone = BSMLSSFPN(**backbone_conf)
        else:
            self.backbone = LSSFPN(**backbone_conf)
        self.head = BEVHeightHead(**head_conf)
        self.is_train_height = is_train_height
        self._param_stamp = None
        # True: replay from the second call of a signature; False: always eager; "auto" (default): build the graph at the
        # second call, time it against the eager forward on that very input (three synchronous calls each) and keep the faster
        self.graph_forward = {"0": False, "1": True}.get(os.environ.get("SGV3D_GRAPH_FORWARD", "auto"), "auto")
        self.graph_cache_size = 2
        self._graphs = {}               # signature -> [calls seen, GraphedForward | None | False (capture failed)]
        self._graph_suspended = 0
        self._flat, self._flat_age, self._flat_gen, self._flat_reg, self._flat_dirty = None, 0, 0, -1, True    # cached walk over the module tree (_stamp)
        self._graph_digest = None       # head.decode_digest() of the last _graphed_forward lookup
        self._decoded = None            # (decode buffer, weak refs to the maps it was computed from, their version, the decode digest): see get_bboxes
        if checkpoint is not None:
            with open(checkpoint, "rb") as f:
                state_dict = torch.load(f, map_location='cpu')
            self.backbone.load_state_dict(self.get_backbone(state_dict))
        _LIVE.add(self)
        _install_hooks()
        weakref.finalize(self, _instance_gone)

    @staticmethod
    def get_backbone(state_dict):
        """Backbone sub-dict of a Lightning checkpoint ('model.backbone.' prefix stripped).  The
        reference's version (models/bev_height.py:35-40) lacks ``self`` and keeps a leading '.'."""
        state_dict = state_dict.get('state_dict', state_dict)
        prefix = 'model.backbone.'
        return {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}

    # ------------------------------------------------------------------------------------------
    def _stamp(self):
        """Identity of the weights the packed HIP tensors (and captured graphs) were made from.

        The exact form -- (address, version) of every parameter and buffer from a walk over the module tree -- costs 1-3 ms of
        pure host time for the ~860 tensors of the cfg-2 model: with one frame in flight (the reference harness's eval_step
        waits for every frame's boxes) the GPU idles through it.  So the walk only collects the ``_parameters`` / ``_buffers``
        dicts of the sub-modules; every forward sums the version counters and the addresses of what those dicts hold NOW
        (~0.3 ms in Python, ~0.03 ms through the compiled helper of sgv3d_amd/host_ext): an in-place write (optimiser step, ``load_state_dict``, ``copy_``) moves the first, a ``p.data = ...`` swap
        or a tensor object replaced inside a dict (a sub-module's own ``.to()`` / ``.half()``, ``_buffers[...] = ...``) the
        second.  Objects registered through ``nn.Module``'s own entry points -- ``m.weight = nn.Parameter(...)``,
        ``register_parameter`` / ``register_buffer``, a sub-module assigned, any ``load_state_dict(assign=True)`` from here, a
        sub-module or a parent (Lightning) -- on a module of this tree bump a registration counter (torch's global registration
        hooks, installed while a BEVHeight instance lives and deaf to every other module; ``_REGISTRATIONS``) and the walk is redone
        on the NEXT forward: no window of stale weights.  ``_apply`` / ``load_state_dict``
        / ``train()`` of this module drop the walk themselves.  What no hook sees -- a sub-module swapped by writing into a
        ``_modules`` dict directly -- is caught by the full walk every ``_RESTAMP_EVERY`` forwards."""
        walk = self._flat
        if walk is None or self._flat_dirty or self._flat_age >= self._RESTAMP_EVERY or self._flat_reg != _REGISTRATIONS[0]:
            mods = list(self.modules())
            dicts = [d for m in mods for d in (m._parameters, m._buffers) if d]     # (an empty one is filled through a hook)
            if walk is None or len(mods) != len(walk[0]) or any(a is not b for a, b in zip(mods, walk[0])):
                self._flat_gen += 1                 # another module tree: never equal to an earlier stamp
            self._flat = walk = (mods, dicts)
            _TRACKED.update(id(m) for m in mods)          # (the registration hooks listen to these modules only)
            self._flat_age, self._flat_dirty = 0, False
            self._flat_reg = _REGISTRATIONS[0]
        self._flat_age += 1
        fast = _host_ext.stamp()
        if fast is not None:                         # the same three sums in C++ (sgv3d_amd/host_ext/stamp_ext.cpp): ~0.03 ms
            n, ver, ptr = fast(walk[1])
            return (self._flat_gen, n, ver, ptr)
        n = ver = ptr = 0
        for d in walk[1]:
            for t in d.values():
                if t is not None:
                    n += 1
                    ver += t._version
                    ptr += t.data_ptr() + (id(t) >> 4)
        return (self._flat_gen, n, ver, ptr)

    _RESTAMP_EVERY = 256

    def _apply(self, fn, *args, **kwargs):
        self._flat_dirty = True                     # buffers (and, with some flags, parameters) become new objects
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._flat_dirty = True                     # (assign=True replaces the Parameter objects)
        return super().load_state_dict(*args, **kwargs)

    def refresh(self):
        """Drop the packed HIP weights (they are rebuilt on the next forward).  Called automatically
        when a parameter or buffer changed in place or was replaced (load_state_dict, .to(), optimiser)."""
        for m in self.modules():
            if isinstance(m, HipModule):
                m._hip = None
        self._param_stamp = None
        self._graphs = {}               # captured graphs read the packed weights that were just dropped

    def train(self, mode=True):
        """Switching between training and inference drops the packed inference weights and the cached module walk: the fused
        optimiser step (train_step.DataParallelAdamW) writes parameters through raw pointers, which no version counter records."""
        super().train(mode)
        self._flat_dirty = True
        self.refresh()
        return self

    def forward(self, x, mats_dict, timestamps=None):
        """Images -> per-task prediction maps, as models/bev_height.py:42-80 does.

        ``x``: float32 [B, num_sweeps, num_cams, 3, H, W] on the GPU.  ``mats_dict``: the seven calibration
        tensors of the reference's collate function -- 'sensor2ego_mats', 'intrin_mats', 'ida_mats',
        'sensor2sensor_mats', 'sensor2virtual_mats' as [B, num_sweeps, num_cams, 4, 4], 'reference_heights' as
        [B, num_sweeps, num_cams], 'bda_mat' as [B, 4, 4].  ``timestamps`` is ignored here as it is there.
        Result: one single-element list per task holding a dict of NCHW maps (reg, height, dim, rot, vel,
        heatmap) -- the nesting mmdet3d's CenterHead produces."""
        if self.training:
            from ..train_forward import bevheight_train_forward
            return bevheight_train_forward(self, x, mats_dict)          # differentiable
        stamp = self._stamp()
        if stamp != self._param_stamp:
            self.refresh()
            self._param_stamp = stamp
        graphed = self._graphed_forward(x, mats_dict)
        if graphed is not None:
            preds, decoded = graphed(self, x, mats_dict)
            # the graph decoded these maps already: remembered for a get_bboxes call on exactly these tensors, unmodified
            self._decoded = (decoded, [weakref.ref(v) for task in preds for v in task[0].values()], tensor_version(preds[0][0]['heatmap']),
                             self._graph_digest)
            return preds
        self._decoded = None
        bev = self.backbone(x, mats_dict, timestamps, nhwc_out=True)   # NHWC buffer [B, Y, X, C]
        return self.head(bev, nhwc=True)

    # ------------------------------------------------------------------------------------------ hipGraph behind forward()
    def _graphed_forward(self, x, mats_dict):
        """The captured hipGraph of this call's signature, or None when the call has to launch eagerly.

        The reference harness calls ``self.model(sweep_imgs, mats)`` once per frame and nothing else
        (exps/bevheight/dair-v2x/bev_height_lss_r50_864_1536_256x256.py:248): a batch-1 forward is ~130 dependent launches,
        so the eager call is bound by the host's launch cadence.  From the SECOND call with the same signature (shapes,
        dtypes, stream, compute mode, weights) the forward is therefore one graph replay on static buffers
        (``pipeline.GraphedForward``; the first call runs eagerly and does the per-layer measurements).  Eager always:
        gradients enabled, inside someone else's stream capture, under ``pipeline.eager_forward`` (``FramePipeline``, the
        instrumented passes), ``self.graph_forward = False`` / ``SGV3D_GRAPH_FORWARD=0``.  ``graph_forward = "auto"`` (the
        default) keeps the replay only where it measures faster than the eager call (``_replay_pays``).  At most ``graph_cache_size``
        signatures keep a graph (each owns its activation buffers, ~1 GB at cfg-2); the least recently used one is dropped."""
        if (not self.graph_forward or self._graph_suspended or torch.is_grad_enabled() or not x.is_cuda
                or hip_ops.PROFILE is not None or torch.cuda.is_current_stream_capturing()):
            return None
        key = (tuple(x.shape), x.dtype, str(x.device), torch.cuda.current_stream(x.device).cuda_stream,
               tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(mats_dict.items())),
               hip_ops.switch_state(), bool(getattr(self.backbone, 'fuse_lift_splat', False)),
               self.head.decode_digest())             # (the recorded decode bakes test_cfg / bbox_coder into kernel arguments)
        self._graph_digest = key[-1]
        entry = self._graphs.get(key)
        if entry is None:
            self._graphs[key] = entry = [0, None]
            while len(self._graphs) > self.graph_cache_size:
                self._graphs.pop(next(iter(self._graphs)))
        else:
            self._graphs[key] = self._graphs.pop(key)            # most recently used last
        entry[0] += 1
        if entry[0] < 2:
            return None                                          # first sight of this signature: eager (packs, measures)
        if entry[1] is None:
            from ..pipeline import GraphedForward, CAPTURE_ERRORS
            try:
                entry[1] = GraphedForward(self, x, mats_dict)
            except CAPTURE_ERRORS as e:
                import warnings
                torch.cuda.synchronize(x.device)
                entry[1] = False
                warnings.warn(f"BEVHeight.forward: hipGraph capture failed ({type(e).__name__}: {e}); this signature keeps "
                              f"launching eagerly", RuntimeWarning, stacklevel=3)
            if entry[1] and self.graph_forward == "auto":
                entry.append(self._replay_pays(entry[1], x, mats_dict))
                if not entry[2]["replay_chosen"]:
                    entry[1] = False                             # (drops the graph and its activation pool)
        return entry[1] or None

    def _replay_pays(self, graphed, x, mats_dict, reps=3):
        """One frame at a time -- the pattern this graph exists for -- through the replay (input copies, the graphs, output
        copies, decode inside) and through the eager forward + decode, ``reps`` synchronous calls each on the caller's input.
        Whether ~170 launches from Python or one long graph submission reaches the GPU sooner depends on the host: on the
        development boxes the two are within 2 % of each other, on a slower host the replay wins by the launch overhead."""
        import time
        from ..pipeline import eager_forward
        dev = x.device

        def timed(fn):
            fn()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
                torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) / reps

        def eager():
            with eager_forward(self):
                bev = self.backbone(x, mats_dict, None, nhwc_out=True)
                self.head.decode_device(self.head(bev, nhwc=True))
        t_graph = timed(lambda: graphed(self, x, mats_dict))
        t_eager = timed(eager)
        return {"replay_ms": t_graph * 1e3, "eager_ms": t_eager * 1e3, "replay_chosen": bool(t_graph < 0.98 * t_eager)}

    def get_targets(self, gt_boxes, gt_labels):
        return self.head.get_targets(gt_boxes, gt_labels)

    def loss(self, targets, preds_dicts):
        return self.head.loss(targets, preds_dicts)

    def get_bboxes(self, preds_dicts, img_metas=None, img=None, rescale=False):
        return self.head.get_bboxes(preds_dicts, img_metas, img, rescale, decoded=self._decoded_for(preds_dicts))

    def _decoded_for(self, preds_dicts):
        """The decode the forward's hipGraph already ran, if ``preds_dicts`` is the very output of the last forward: the same
        tensor objects in the same order, never written since (the 36 maps are views of one buffer and share its version
        counter).  Anything else -- another structure, clones, edited maps, the eager path -- decodes now."""
        spec, self._decoded = self._decoded, None
        if spec is None:
            return None
        decoded, refs, version, digest = spec
        try:
            tensors = [v for task in preds_dicts for v in task[0].values()]
        except (TypeError, AttributeError, IndexError, KeyError):
            return None
        # (maps made under torch.inference_mode() have no version counter: in-place edits cannot be seen, so no reuse)
        if (len(tensors) != len(refs) or any(r() is not t for r, t in zip(refs, tensors)) or version is None
                or tensor_version(tensors[0]) != version or digest != self.head.decode_digest()):
            return None                 # (the last: test_cfg / bbox_coder edited between the forward and get_bboxes, e.g. nms_type)
        return decoded
