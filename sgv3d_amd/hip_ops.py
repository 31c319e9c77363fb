"""Thin host-side wrappers over the C ABI for the convolution family and the small layers.

Tensors here are torch CUDA tensors used purely as device buffers: activations are NHWC float32
``[B, H, W, C]`` (channel-last, the layout the gfx950 kernels want), every call enqueues on torch's
current stream.  No arithmetic happens in PyTorch on this path.
"""
import ctypes
from collections import namedtuple
from functools import partialmethod

import torch

from . import _lib, conv_tiles, pack_cache
from ._lib import ConvDesc, CONV_NORMAL, CONV_DECONV, CONV_NCHW_OUT, CONV_GROUP_PLANES  # noqa: F401
from .conv_tiles import (TILE_WINO, TILE_WINO_RES, TILE_PATCH, TILE_WINO_HALF, TILE_WINO4, TILE_WINO4_WIDE, TILE_WINO4_NARROW,  # noqa: F401
                         TILE_WINO4_OCC, TILE_WINO4_G48, TILE_F4RES)


def _st(t):
    return _lib.stream_handle(t.device)


# When a list, every wrapper appends (kernel name, algorithmic flops, start event, end event) recorded
# on the launch stream (bench.py's roofline pass).  None = no instrumentation.
PROFILE = None
# Pick algorithm / tile / split-K per (layer, input shape) by timing the candidates once, outside graph capture.
# False (SGV3D_NO_AUTOTUNE=1): a fixed rule instead -- the same choices on every run and every rank, hence
# bitwise reproducible results (measured choices can differ between runs with timing noise, which moves the
# results by fp32 rounding since the algorithms sum in different orders); ~10 % slower.
AUTOTUNE = not __import__("os").environ.get("SGV3D_NO_AUTOTUNE")
# True (SGV3D_DETERMINISTIC=1), or torch.use_deterministic_algorithms(True) -- what Lightning's Trainer(deterministic=True)
# sets --: training runs bitwise repeatable.  Read at every launch (a capture bakes in the value it saw): see deterministic().
DETERMINISTIC = __import__("os").environ.get("SGV3D_DETERMINISTIC", "0") not in ("", "0")


def deterministic():
    """True in deterministic mode: the DCN input gradient is the gather-form kernel (no float atomics,
    ``sgv3d_deform_im2col3x3_backward_det``) and no per-layer choice is made by timing -- a layer signature that is in
    TUNE_DB takes its recorded choice, one that is not takes the fixed rule that SGV3D_NO_AUTOTUNE and a graph capture use.
    Scope: bitwise repeatable on the same GPU model, software stack, world size and bucket size."""
    return DETERMINISTIC or torch.are_deterministic_algorithms_enabled()
# True: conv records carry the layer shape in their name (tools/layer_report.py)
PROFILE_DETAIL = False
# False: the autotuner never proposes split-K (experiments; SGV3D_NO_SPLITK=1)
import os as _os
# Number of concurrent copies of a candidate the autotuner times (SGV3D_TUNE_STREAMS, default 1 = an isolated launch).
# With several frames in flight (pipeline.FramePipeline) a layer shares the chip with other frames' kernels: the
# throughput-optimal tile / split differs from the latency-optimal one an isolated launch finds (a split-K or small-tile
# choice that fills idle CUs in isolation only adds work when the CUs are busy anyway).  N > 1 launches the candidate on
# N streams at once and compares the time for all of them to finish.
TUNE_STREAMS = max(1, int(_os.environ.get("SGV3D_TUNE_STREAMS", "1")))
TUNE_VERBOSE = bool(_os.environ.get("SGV3D_TUNE_VERBOSE"))      # print every candidate's time as the first-call measurement goes
# launches per stream and repetitions of a candidate's timing under load (SGV3D_TUNE_ROUNDS / SGV3D_TUNE_REPEATS; the committed
# tune DBs are measured with 8 x 4 -- tools/make_tune_db.sh -- so that near-ties are not decided by noise)
TUNE_ROUNDS = max(1, int(_os.environ.get("SGV3D_TUNE_ROUNDS", "3")))
TUNE_REPEATS = max(1, int(_os.environ.get("SGV3D_TUNE_REPEATS", "2")))
SPLIT_K = not _os.environ.get("SGV3D_NO_SPLITK")
# False: 3x3 / stride-1 layers never use the Winograd F(2x2,3x3) kernel (SGV3D_NO_WINOGRAD=1)
WINOGRAD = not _os.environ.get("SGV3D_NO_WINOGRAD")
# False: CenterHead branches run as two kernels with the hidden maps in HBM (SGV3D_NO_FUSED_HEAD=1)
FUSED_HEAD = not _os.environ.get("SGV3D_NO_FUSED_HEAD")
# fp32 CenterHead branches (SGV3D_HEAD_PATH): 2 (default) = the fused F(4x4) kernel (csrc/head_wino4.hip: 532 us at the cfg-2
# launch); 0 = the fused F(2x2) kernel (conv_wino.hip: 976 us); 1 = first layers as one convolution (its algorithm measured per
# load: F(4x4) in channel chunks) + the final-conv kernel (executes as few MFMAs as path 2 but moves 3.9 GB of M / hidden maps per
# frame: 1264 vs 1089 us per call against path 0 with three in flight); "auto" (None here): all three timed under load at the
# first call.
HEAD_PATH = {"0": 0, "1": 1, "2": 2, "auto": None}.get(_os.environ.get("SGV3D_HEAD_PATH", ""), 2)
# True (SGV3D_BF16=1 or set before the first forward): every convolution multiplies through the bf16 MFMA variant of the
# implicit-GEMM kernel (operands rounded to bf16 on their way into LDS, fp32 accumulation and epilogue, fp32 tensors in
# HBM) -- the compute dtype BASELINE cfg-3 / cfg-5 name.  Winograd and the fused head kernel are fp32-only and are not
# used in this mode (a bf16 direct convolution runs at 16x the fp32 MFMA rate, so the 2.25x saving no longer matters).
MFMA_BF16 = bool(_os.environ.get("SGV3D_BF16"))
# bf16 mode only: the convolution chains of the ResNets (image backbone, BEV trunk) keep their activations as bf16
# tensors in HBM -- the 1x1 / strided layers at the large resolutions are HBM-bound, so halving the bytes is worth more
# than any MFMA tuning there (a 256 -> 1024 1x1 with residual at 68x120x4: 99 -> 55 us).  The stem conv writes bf16, the
# blocks read and write bf16 (epilogue in fp32, one rounding), the necks read bf16 and write fp32.
# SGV3D_NO_BF16_ACTIVATIONS=1 keeps fp32 tensors everywhere (round 1 behaviour).
BF16_ACTIVATIONS = not _os.environ.get("SGV3D_NO_BF16_ACTIVATIONS")
# bf16 compute mode in TRAINING (MFMA_BF16 with BF16_ACTIVATIONS off: f32 tensors, bf16 products): also the weight gradients
# run on the bf16 matrix cores (conv_wgrad_bf16_kernel); 0: they stay on the f32 MFMA kernel
TRAIN_BF16_WGRAD = _os.environ.get("SGV3D_TRAIN_BF16_WGRAD", "1") != "0"
# ... and 3x3 / stride-1 layers may use the all-taps form (conv_wgrad3x3_bf16.hip: a workgroup owns a 64 x 64 tile for all nine taps;
# the batched CenterHead launch always, single layers where the first-call measurement / the tune DB says so); 0: per-tap kernel only
WGRAD_BF16_ALLTAPS = _os.environ.get("SGV3D_WGRAD_BF16_ALLTAPS", "1") != "0"
# Mixed-precision TRAINING with bf16 activation STORAGE in the image backbone (SGV3D_TRAIN_BF16_STORAGE=1, default off): the stages of
# backbone.img_backbone keep their activations and activation gradients as bf16 tensors in HBM -- what autocast keeps between layers
# in the reference (--amp_backend native) -- through the bf16 BatchNorm (csrc/bn_train.hip), the bf16-tensor weight gradients
# (csrc/conv_wgrad*.hip) and the io bits of PackedConv.  Takes effect only where train_bf16_storage_covers() says so; off, or not
# covered: the f32 tensors of the MFMA_BF16 step, bit for bit.
TRAIN_BF16_STORAGE = _os.environ.get("SGV3D_TRAIN_BF16_STORAGE", "0") not in ("", "0")
# SAM ViT encoder in bf16 mode (SGV3D_VIT_BF16=1, default off): between the two residual adds of a Block every tensor is bf16 in HBM and
# attention runs on the bf16 matrix cores (csrc/vit_bf16.hip); the residual stream, the patch embedding and the neck keep f32 tensors.
# Takes effect only where vit_bf16_active() says so; off, or not covered: the f32-tensor path of the compute mode, bit for bit.
VIT_BF16 = _os.environ.get("SGV3D_VIT_BF16", "0") not in ("", "0")
# TRAINING the SAM ViT encoder in bf16 mode (SGV3D_VIT_TRAIN_BF16=1, default off): sgv3d_amd/vit_train.py runs the launches of the bf16
# inference mode above (bf16 tensors between the two residual adds of a Block, saved as they are) and their adjoints: attention on the
# bf16 matrix cores (csrc/vit_grad_bf16.hip), bf16-tensor data and weight gradients of the linear layers.  Takes effect only where
# vit_train_bf16_active() says so; off, or not covered: the f32-tensor training path, bit for bit.
VIT_TRAIN_BF16 = _os.environ.get("SGV3D_VIT_TRAIN_BF16", "0") not in ("", "0")
# 1x1 layers with unpadded channel counts read the OIHW weight tensor itself as their packed weights (diagnostic: 0 packs a copy)
ALIAS_1X1_WEIGHTS = _os.environ.get("SGV3D_ALIAS_1X1_WEIGHTS", "1") != "0"
# True (SGV3D_F32X3=1): the implicit-GEMM layers compute float32-accurate products on the bf16 matrix cores -- every
# operand is split exactly into three bf16 terms and six partial products are accumulated in f32 (csrc/conv_igemm.hip,
# SPLIT3): the error of a product is one f32 rounding, the MFMA time 192 instead of 512 cycles per 16 k.  Winograd
# layers keep competing in the first-call measurement.  Opt-in: the default path multiplies on the f32 MFMA.
# SGV3D_F32X3=auto ("auto" here): the f32x3 tiles compete with the f32-MFMA tiles and Winograd in the first-call
# measurement of every layer (host-side tile ids 11..14 = f32x3 of tiles 1..4); long-K layers pick it, small-K ones do not.
MFMA_F32X3 = {"": False, "0": False, "auto": "auto"}.get(_os.environ.get("SGV3D_F32X3", ""), True)
# (tile, split-K) decisions by layer signature.  SGV3D_TUNE_CACHE=<file> loads them at import and
# save_tune_db() writes them back, so that a profiled run replays the choices of an earlier run
# instead of timing candidates again (keeps rocprofv3 per-kernel averages free of tuning launches).
TUNE_DB = {}
TUNE_STATS = {"measured": 0, "from_db": 0}     # per process: layer signatures timed here / answered from a tune DB
_COMMITTED_SIGS = set()      # signatures that came from tune/gfx950_*.json: honoured on gfx950 devices only
_TUNE_SIDE_STREAMS = []


def _tune_db_path():
    import os
    return os.environ.get("SGV3D_TUNE_CACHE")


def load_tune_db(path=None):
    import json
    import os
    path = path or _tune_db_path()
    if path and os.path.exists(path):
        with open(path) as f:
            loaded = {k: tuple(v) for k, v in json.load(f).items()}
        TUNE_DB.update(loaded)
        _COMMITTED_SIGS.difference_update(loaded)       # (a local measurement overrides a committed one: no longer arch-bound)
    return len(TUNE_DB)


def save_tune_db(path=None):
    import json
    path = path or _tune_db_path()
    if path:
        with open(path, "w") as f:
            json.dump({k: list(v) for k, v in TUNE_DB.items()}, f, indent=0, sort_keys=True)


def load_default_tune_dbs():
    """tune/gfx950_*.json at the repository root: the (algorithm, tile, split-K) choices measured on an MI355X for the
    BASELINE configurations, committed so that a run neither spends its first forward on candidate timing nor moves by
    near-tie picks from run to run.  A layer signature that is not in there is measured as before (autotune is the
    fallback).  SGV3D_NO_TUNE_DB=1 ignores the committed files, SGV3D_TUNE_SKIP=<name>[,<name>] only the named ones;
    SGV3D_TUNE_CACHE=<file> is loaded on top and is the file save_tune_db() writes."""
    import glob
    import os
    if os.environ.get("SGV3D_NO_TUNE_DB"):
        return 0
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tune")
    skip = {x for x in os.environ.get("SGV3D_TUNE_SKIP", "").split(",") if x}      # file names to leave out (re-measuring one DB)
    n = 0
    for f in sorted(glob.glob(os.path.join(root, "gfx950_*.json"))):
        if os.path.basename(f) in skip:
            continue
        with open(f) as fh:
            sigs = list(__import__("json").load(fh))
        n += load_tune_db(f) and 1
        _COMMITTED_SIGS.update(sigs)
    return n


_ARCH_IS_GFX950 = {}


def _is_gfx950(device):
    idx = torch.device(device).index or 0
    if idx not in _ARCH_IS_GFX950:
        _ARCH_IS_GFX950[idx] = "gfx950" in str(getattr(torch.cuda.get_device_properties(idx), "gcnArchName", ""))
    return _ARCH_IS_GFX950[idx]


# How every kernel that competes with another way of doing the same work is chosen, in this order: the fixed rule under
# SGV3D_NO_AUTOTUNE; else the tune DB's entry (``tune_lookup``); else the fixed rule where nothing may be timed (``tune_may_measure``);
# else the candidates are timed (``tune_best_of``, or the site's own loop) and the winner is written back (``tune_record``).  The sites:
# PackedConv._call, conv_pair_choice, conv_shortcut_choice, deconv_x3_choice, stem_fused_choice, BEVHeightHead._branch_path and
# conv_grad._wgrad_choice.
def tune_lookup(sig, device):
    """The tune DB's entry of ``sig`` as stored, or None: under SGV3D_NO_AUTOTUNE (the documented fixed rule consults no record), without
    an entry, and for a committed ``tune/gfx950_*`` entry on a device that is not gfx950."""
    if not AUTOTUNE or sig not in TUNE_DB or (sig in _COMMITTED_SIGS and not _is_gfx950(device)):
        return None
    return TUNE_DB[sig]


def tune_may_measure():
    """Candidates may be timed now: not under SGV3D_NO_AUTOTUNE, not inside a graph capture, not in deterministic mode."""
    return AUTOTUNE and not deterministic() and not torch.cuda.is_current_stream_capturing()


def tune_record(sig, entry):
    """Keep ``entry`` as the choice of ``sig``: measured on THIS device (or restored from a run's own record), no longer arch-bound."""
    TUNE_DB[sig] = entry
    _COMMITTED_SIGS.discard(sig)


def tune_best_of(sig, device, baseline, candidates):
    """Time ``baseline`` and then each of ``candidates`` ((key, thunk) pairs, in their order) with ``time_callable``, each after one warming
    call (a layer inside measures its own candidates there).  Returns (the baseline's time, the key of the fastest candidate -- the first
    of equal ones --, its time); a candidate beats the baseline only when strictly faster, which the caller decides."""
    baseline()
    t0 = time_callable(baseline, device)
    best, t1 = None, None
    for key, fn in candidates:
        fn()
        dt = time_callable(fn, device)
        if TUNE_VERBOSE:
            print(f"[tune] {sig}: {key}: {dt * 1e3 / TUNE_ROUNDS:.1f} us (baseline {t0 * 1e3 / TUNE_ROUNDS:.1f} us)", flush=True)
        if t1 is None or dt < t1:
            best, t1 = key, dt
    return t0, best, t1


load_default_tune_dbs()
load_tune_db()
# Host tile ids: what every id means -- family, ABI code, workgroup footprint, weight form, split-K policy, profile symbol -- is ONE
# table, sgv3d_amd/conv_tiles.py; the names below are read from it
TILES = conv_tiles.TILES
TILE_NAMES = {t: T.label for t, T in TILES.items()}
MFIRST = _os.environ.get("SGV3D_MFIRST", "1") != "0"
# F(4x4) with the f32x3 position GEMM (csrc/gemm_x3_grouped.hip), by tile shape
WINO4_X3_TILES = conv_tiles.family("wino4_x3")
X3_TILE_ROWS = {t: TILES[t].bm for t in WINO4_X3_TILES}
X3_TILE_COLS = {t: TILES[t].bn for t in WINO4_X3_TILES}
WINO4_TILES = conv_tiles.family("wino4", "wino4_x3")


def wino4_axis_tiles(n, dil):
    """F(4x4) tiles along one axis of ``n`` pixels at dilation ``dil`` (csrc/conv_wino4.hip: wino4_axis): every phase its own tiles,
    or the phases stacked on one line with a zero element between neighbours -- whichever is fewer."""
    dil = max(1, int(dil))
    return min(dil * -(-(-(-n // dil)) // 4), -(-(n + dil - 1) // 4))


def wino4_tiles(batch, oh, ow, dil):
    """Rows per position of the three-launch F(4x4) path before padding to the GEMM's m-tile."""
    return batch * wino4_axis_tiles(oh, dil) * wino4_axis_tiles(ow, dil)


def _wino4_tiles_per_phase(batch, oh, ow, dil):
    """The tile count with every sub-grid phase on tiles of its own (what a dilated layer ran before the lattice; dil 1: the same
    number).  The candidate list of the f32x3 position GEMM and the profile's executed flops are part of the recorded dispatch
    (tests/golden/conv_dispatch.json.gz) and keep counting this way: for the three dilated ASPP layers the list is the one their
    committed choices were measured against, and the profile reports up to a quarter more MFMA work than the launch executes."""
    dil = max(1, int(dil))
    return batch * dil * dil * -(-(-(-oh // dil)) // 4) * -(-(-(-ow // dil)) // 4)


WINO4_G48 = _os.environ.get("SGV3D_WINO4_G48", "1") != "0"     # 0: never a candidate
# 0: the f32x3 position GEMM is never a candidate -- every product of the f32 path on the f32 MFMA (bench.py's native_f32_value)
WINO4_X3 = _os.environ.get("SGV3D_WINO4_X3", "1") != "0"
# Implicit-GEMM layers (1x1, strided 3x3 / 1x1, patchify: at most 32 taps, cin % 32 == 0) with f32-accurate products on the bf16 matrix
# cores (csrc/conv_pw_x3.hip).  0: never a candidate.
PW_X3 = _os.environ.get("SGV3D_PW_X3", "1") != "0"
PW_X3_TILES = conv_tiles.family("pw_x3")
PW_X3_DIMS = {t: (TILES[t].bm, TILES[t].bn) for t in PW_X3_TILES}


def _pw_x3_tiles(gemm_m, gemm_n, nkt=None, mfirst=True, skip=()):
    """The pw_x3 tiles worth timing for a gemm_m x gemm_n GEMM, shapes that leave the chip neither empty nor padded: at least ~96
    workgroups (or, where the launch can split K -- ``nkt``, its k-steps of 32, is given --, nkt >= 16), 64-channel tiles only for small
    grids, 256-channel ones only where the GEMM has 256 columns, m-tile first only with several channel tiles (``mfirst`` False: never),
    none of the (bm, bn) shapes in ``skip``."""
    out = ()
    for t in PW_X3_TILES:
        bm, bn = PW_X3_DIMS[t]
        wgs = -(-gemm_m // bm) * -(-gemm_n // bn)
        if (bm, bn) in skip or (bn == 256 and gemm_n < 256) or (TILES[t].mfirst and not (mfirst and MFIRST and gemm_n > bn)):
            continue
        if (wgs >= 96 or (SPLIT_K and nkt is not None and nkt >= 16)) and (bn >= 128 or gemm_n <= 64 or wgs < 1024):
            out += (t,)
    return out


def _split_factors(policy, nk, wgs):
    """The split-K factors above 1 that a launch of ``wgs`` workgroups and ``nk`` k-steps may take under conv_tiles.SPLIT_POLICY[policy]
    (none under SGV3D_NO_SPLITK)."""
    if not SPLIT_K:
        return ()
    pol = conv_tiles.SPLIT_POLICY[policy]
    return tuple(s for s in conv_tiles.SPLITS if nk // s >= pol["min_k"] and wgs < pol["max_wgs"] and wgs * s <= pol["max_total"])


# F(4x4,3x3) in ONE launch (TILE_F4RES): 3x3 / stride 1 / pad 1 layers with 64 input channels (ResNet layer 1) or 64 output channels
# (the CenterHead's shared layer), f32
F4RES = _os.environ.get("SGV3D_F4RES", "1") != "0"     # 0: never a candidate
# f32 implicit GEMM, 64x64 tile with five workgroups per CU (32 KB of swizzled LDS, one register stage; csrc/conv_igemm.hip:
# OCC): for the small-K layers
OCC5_TILES = conv_tiles.select("igemm", occ5=True) + conv_tiles.select("igemm", occ5=True, mfirst=True)
OCC5 = _os.environ.get("SGV3D_OCC5", "1") != "0"       # 0: never candidates
WINO4 = _os.environ.get("SGV3D_WINO4", "1") != "0"     # 0: F(4x4) is never a candidate
WINO4_MIN_CHANNELS = 128                              # candidates only where cin and cout are at least this
WINO_HALF = _os.environ.get("SGV3D_WINO_HALF", "1") != "0"
PATCH_BF16 = _os.environ.get("SGV3D_PATCH_BF16", "1") != "0"
# bf16 mode, bf16 tensors in and out: the direct-weight implicit GEMM (sgv3d_conv_dw_bf16_forward)
DW_TILES = conv_tiles.family("dw_bf16")
DW_DEEP_TILES = conv_tiles.select("dw_bf16", deep=True)
DW_DEEP = _os.environ.get("SGV3D_DW_DEEP", "1") != "0"   # 0: the *_DEEP tiles are never candidates
DW_NARROW = _os.environ.get("SGV3D_DW_NARROW", "1") != "0"   # 0: the 64x128 tile is never a candidate
DW_DEEP_MAX_WGS = int(_os.environ.get("SGV3D_DW_DEEP_MAX_WGS", "768"))   # the *_DEEP tiles are candidates for grids up to this many workgroups
DW_BF16 = _os.environ.get("SGV3D_DW_BF16", "1") != "0"   # 0: never a candidate
DW_SPLIT_K = _os.environ.get("SGV3D_DW_SPLITK", "1") != "0"   # 0: the direct-weight kernel is never split along k


class prof:
    """``with prof("kernel", flops, nbytes):`` brackets a launch with HIP events when PROFILE is active.  ``flops`` /
    ``nbytes``: the launch's ALGORITHMIC work -- 2 x MACs of the direct convolution; every tensor the layer's
    definition touches read or written exactly once.  PROFILE records are ``(name, flops, start, stop, nbytes, extra)``; ``extra``: None or
    ``{'symbol': the MFMA kernel's exact symbol, 'mfma_flops': the flops that kernel EXECUTES in this launch}``."""
    __slots__ = ("name", "flops", "nbytes", "extra", "e0")

    def __init__(self, name, flops=0.0, nbytes=0.0, extra=None):
        self.name, self.flops, self.nbytes, self.extra, self.e0 = name, flops, nbytes, extra, None

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            PROFILE.append((self.name, self.flops, self.e0, e1, self.nbytes, self.extra))
            self.e0 = None
        return False


def heuristic_tile(M, N):
    """Same cost model as pick_tile() in csrc/conv_igemm.hip."""
    best, best_cost = 1, None
    for t, pen in zip(conv_tiles.select("igemm"), (1.0, 1.06, 1.06, 1.18)):
        bm, bn = TILES[t].bm, TILES[t].bn
        tiles = -(-M // bm) * -(-N // bn)
        cost = -(-tiles // 256) * bm * bn * pen
        if best_cost is None or cost < best_cost:
            best, best_cost = t, cost
    return best


def pack_geometry(k, n):
    kp, np_ = ctypes.c_int(), ctypes.c_int()
    _lib.load().sgv3d_conv_pack_geometry(int(k), int(n), ctypes.byref(kp), ctypes.byref(np_))
    return kp.value, np_.value


def fold_bn(bn, conv_bias=None):
    """Eval-mode BatchNorm folded to per-channel (scale, shift):  y = scale * conv + shift."""
    with torch.no_grad():
        inv = torch.rsqrt(bn.running_var.float() + bn.eps)
        gamma = bn.weight.float() if bn.weight is not None else torch.ones_like(inv)
        beta = bn.bias.float() if bn.bias is not None else torch.zeros_like(inv)
        scale = gamma * inv
        shift = beta - bn.running_mean.float() * scale
        if conv_bias is not None:
            shift = shift + conv_bias.float() * scale
    return scale.contiguous(), shift.contiguous()


def train_bf16_storage_covers(channel_counts):
    """Whether the training forward keeps the maps of a ResNet whose stages have these channel counts as bf16 tensors
    (TRAIN_BF16_STORAGE): the mixed-precision step with bf16 weight gradients (MFMA_BF16, not the f32x3 split, TRAIN_BF16_WGRAD) and
    16-byte bf16 pixel rows everywhere (every count a multiple of 8, and at least 16: the bf16 weight-gradient kernels take no narrower
    layer).  Otherwise the f32-tensor path runs, silently, like the other coverage rules."""
    if not (TRAIN_BF16_STORAGE and MFMA_BF16 and TRAIN_BF16_WGRAD) or MFMA_F32X3:
        return False
    counts = [int(c) for c in channel_counts]
    return bool(counts) and all(c >= 16 and c % 8 == 0 for c in counts)


def vit_bf16_covers(dim, num_heads, mlp_dim=None):
    """Whether the bf16 kernels of the SAM ViT encoder take a Block of this shape: head_dim 32, 64 or 80 (sgv3d_vit_attention_bf16)
    and 16-byte bf16 rows everywhere (dim and mlp_dim multiples of 8)."""
    dim, num_heads = int(dim), int(num_heads)
    if dim <= 0 or num_heads <= 0 or dim % num_heads or dim % 8:
        return False
    return dim // num_heads in (32, 64, 80) and (mlp_dim is None or (int(mlp_dim) > 0 and int(mlp_dim) % 8 == 0))


def vit_bf16_active(dim, num_heads, mlp_dim=None):
    """VIT_BF16 in bf16 compute mode (MFMA_BF16, not the f32x3 split) on a covered Block; otherwise the f32-tensor path runs,
    silently, like the other coverage rules."""
    return bool(VIT_BF16 and MFMA_BF16 and not MFMA_F32X3 and vit_bf16_covers(dim, num_heads, mlp_dim))


def vit_train_covers(dim, num_heads):
    """Whether the training forward of the SAM ViT encoder (sgv3d_amd/vit_train.py) takes a Block of this shape: head_dim 32, 64 or
    80 (sgv3d_vit_attention_backward) and 16-byte f32 rows (dim a multiple of 4).  An uncovered shape raises before any launch."""
    dim, num_heads = int(dim), int(num_heads)
    if dim <= 0 or num_heads <= 0 or dim % num_heads or dim % 4:
        return False
    return dim // num_heads in (32, 64, 80)


def vit_train_bf16_active(dim, num_heads, mlp_dim=None):
    """VIT_TRAIN_BF16 in bf16 compute mode (MFMA_BF16, not the f32x3 split) with bf16 weight gradients (TRAIN_BF16_WGRAD) on a Block
    that both the bf16 kernels (vit_bf16_covers) and the training forward (vit_train_covers) take; otherwise the f32-tensor training
    path runs, silently, like the other coverage rules."""
    return bool(VIT_TRAIN_BF16 and MFMA_BF16 and not MFMA_F32X3 and TRAIN_BF16_WGRAD and vit_bf16_covers(dim, num_heads, mlp_dim)
                and vit_train_covers(dim, num_heads))


def dice_covers(mode, num_classes):
    """Whether losses.DiceLoss takes this mode and class count: 'multiclass' keeps one pixel's classes in a thread's registers
    (csrc/dice_loss.hip), which covers 2..32 classes (SGV3D has 7); 'binary' and 'multilabel' walk the classes and take any
    count.  An uncovered combination raises before any launch."""
    c = int(num_classes)
    if mode == "multiclass":
        return 2 <= c <= 32
    return mode in ("binary", "multilabel") and c >= 1


def embed_distill_covers(channels, h, w):
    """Whether the embedding warp and distillation loss (csrc/embed_distill.hip) take this map: a lane owns a quad of channels
    (16-byte accesses), and the bilinear warp needs two rows and two columns.  An uncovered shape raises before any launch."""
    return int(channels) >= 4 and int(channels) % 4 == 0 and int(h) >= 2 and int(w) >= 2


def sam_decoder_covers(transformer_dim, num_heads, downsample_rate=2):
    """Whether the SAM mask decoder's kernels take a two-way transformer of this shape: sgv3d_sam_attention has head dimensions 16
    and 32, so transformer_dim / num_heads (self-attention) and transformer_dim / downsample_rate / num_heads (the cross
    attentions) must each be one of them; transformer_dim % 32 == 0 keeps the upscaled map's transformer_dim / 8 channels in
    16-byte rows.  SAM's 256 / 8 / 2 is covered.  An uncovered decoder raises before any launch."""
    d, h, r = int(transformer_dim), int(num_heads), int(downsample_rate)
    if d <= 0 or h <= 0 or r <= 0 or d % 32 or d % r or d % h or (d // r) % h:
        return False
    return d // h in (16, 32) and d // r // h in (16, 32)


def activation_dtype(*channel_counts):
    """torch.bfloat16 when bf16 mode keeps activations as bf16 tensors in HBM (MFMA_BF16 and BF16_ACTIVATIONS, not the f32x3
    split) and every given channel count allows 16-byte bf16 rows (multiple of 8); else None (= float32 tensors)."""
    if not (MFMA_BF16 and BF16_ACTIVATIONS) or MFMA_F32X3:
        return None
    return torch.bfloat16 if all(int(c) % 8 == 0 for c in channel_counts) else None


def channel_align():
    """Granularity the layers that own their activation buffers pad channel counts to: 4 (16-byte f32 rows); 32 in
    bf16-activation mode, where a multiple of 32 input channels opens the chunk-major k order, bf16 tensors in HBM and the
    patch kernel (SGV3D's 87 / 174 / 348 / 696-channel BEV trunk -> 96 / 192 / 352 / 704; the extra channels are exact zeros)."""
    return 32 if activation_dtype() is not None else 4


def pad_channels(c, align=None):
    align = int(align or channel_align())
    return (int(c) + align - 1) // align * align


# The packed forms of a layer's weights: attribute, packer (called as packer(source, *before, form, *after, stream)), whether the form
# is a permutation of the parameter with padding / rounding (what the pack cache can refresh by a gather), and the plan: (source tensor,
# form buffer, before, after, {what the launch needs to know about the form}), or None for a layer that has no such form.
_Form = namedtuple("_Form", "attr packer permutation plan")
_F32, _BF16, _U8 = torch.float32, torch.bfloat16, torch.uint8
_up32 = lambda v: (v + 31) // 32 * 32


def _plan_w(pc, lib):
    src = pc._keep
    odim = 1 if pc.transposed else 0
    cout, cin = int(src.shape[odim]), int(src.shape[1 - odim])
    if (ALIAS_1X1_WEIGHTS and not pc.transposed and pc.kh == 1 and pc.kw == 1 and cout == pc.cout_pad and cin == pc.k_pad
            and pc.cin == cin and src.is_contiguous() and src.data_ptr() % 16 == 0):
        # a 1x1 layer whose channel counts need no padding: OIHW [cout, cin, 1, 1] IS the packed layout [cout_pad, k_pad] (one tap:
        # both k orders are the identity) -- no pack launch (a training step repacks every layer's weights, forward and data
        # gradient, at ~5 us per launch)
        return src, src.view(pc.cout_pad, pc.k_pad), None, None, {}
    return (src, torch.empty(pc.cout_pad, pc.k_pad, dtype=_F32, device=src.device),
            (cout, cin, int(src.shape[2]), int(src.shape[3]), pc.cin, 1 if pc.transposed else 0, pc.k_order), (pc.k_pad, pc.cout_pad), {})


def _plan_w_wino4(pc, lib):
    # U[p] = (G g G^T)[i][j] for the 36 positions of F(4x4,3x3), each a packed 1x1 weight block of the implicit-GEMM kernel
    k_pad, cout_pad = pack_geometry(pc.cin, pc.cout)
    return (pc._keep, torch.empty(36, cout_pad, k_pad, dtype=_F32, device=pc._keep.device),
            (pc.cout, int(pc._keep.shape[1]), k_pad, cout_pad), (), {"wino4_geom": (k_pad, cout_pad)})


def _plan_w_pw_x3(pc, lib):
    # three bf16 planes per element in fragment order: [cout_pad / 16][kh kw cin / 32][3][512], cout_pad = cout rounded up to 32
    cout_pad = _up32(pc.cout)
    return (pc._keep, torch.empty(cout_pad // 16, _up32(pc.kh * pc.kw * pc.cin) // 32, 3, 512, dtype=_BF16, device=pc._keep.device),
            (pc.cout, int(pc._keep.shape[1]), pc.kh, pc.kw, pc.cin, cout_pad), (), {"pw_x3_cout_pad": cout_pad})


def _plan_w_pw_x3_deconv(pc, lib):
    # transposed convolution (kernel == stride) on the f32x3 pointwise kernel: the x3 pack of the [ks * ks * cout][cin][1][1] view of
    # the weight, row = tap * cout + co (the column order conv_epilogue_store's DECONV scatter decodes)
    if not pc.transposed:
        return None
    n = pc.ks * pc.ks * pc.cout
    w = pc._keep.permute(2, 3, 1, 0).reshape(n, int(pc._keep.shape[0]), 1, 1).contiguous()
    cout_pad = _up32(n)
    return (w, torch.empty(cout_pad // 16, pc.cin // 32, 3, 512, dtype=_BF16, device=w.device),
            (n, int(w.shape[1]), 1, 1, pc.cin, cout_pad), (), {"pw_x3_deconv_cout_pad": cout_pad, "_keep_x3_deconv": w})


def _plan_w_wino4_x3(pc, lib):
    # U[p] of F(4x4,3x3) as three bf16 planes per element: [36][cout_pad][cin / 32][3][32], cout_pad = cout rounded up to 32
    cout_pad = _up32(pc.cout)
    return (pc._keep, torch.empty(36, cout_pad, pc.cin // 32, 3, 32, dtype=_BF16, device=pc._keep.device),
            (pc.cout, int(pc._keep.shape[1]), pc.cin, cout_pad), (), {"wino4_x3_cout_pad": cout_pad})


def _plan_w_dw(pc, lib):
    # transposed convolution (kernel == stride): a 1x1 layer with ks * ks * cout outputs ordered (dy, dx, co)
    w, n = pc._keep, pc.cout                  # [cout, cin_real, kh, kw] f32 on the device ([cin_real, cout, ks, ks] transposed)
    if pc.transposed:
        n = pc.ks * pc.ks * pc.cout
        w = w.permute(2, 3, 1, 0).reshape(n, int(w.shape[0]), 1, 1).contiguous()
    return (w, torch.empty(lib.sgv3d_conv_dw_bf16_weight_bytes(n, pc.cin, pc.kh, pc.kw), dtype=_U8, device=w.device),
            (n, int(w.shape[1]), pc.cin, pc.kh, pc.kw), (), {"_keep_dw": w})      # (the packer reads ``w`` asynchronously)


_FORMS = {
    # implicit GEMM: [cout_pad, k_pad] f32
    "w": _Form("_w", "sgv3d_conv_pack_weight", True, _plan_w),
    # ... its bf16 copy (bf16-activation launches)
    "w_bf16": _Form("w_bf16", "sgv3d_conv_weight_to_bf16", True, lambda pc, lib: (
        pc.w, torch.empty(pc.cout_pad, pc.k_pad, dtype=_BF16, device=pc._keep.device), (pc.k_pad, pc.cout_pad), (), {})),
    # Winograd F(2x2,3x3)
    "w_wino": _Form("_w_wino", "sgv3d_conv_winograd_pack_weight", False, lambda pc, lib: pc.wino_ok and (
        pc._keep, torch.empty(lib.sgv3d_conv_winograd_weight_floats(pc.cout, pc.cin), dtype=_F32, device=pc._keep.device),
        (pc.cout, int(pc._keep.shape[1]), pc.cin), (), {})),
    # U = G g G^T in the fragment order conv_f4res_kernel streams
    "w_f4res": _Form("w_f4res", "sgv3d_conv3x3_f4res_pack_weight", False, lambda pc, lib: (
        pc._keep, torch.empty(int(lib.sgv3d_conv3x3_f4res_weight_floats(pc.cout, pc.cin)), dtype=_F32, device=pc._keep.device),
        (pc.cout, int(pc._keep.shape[1]), pc.cin), (), {})),
    "w_wino4": _Form("w_wino4", "sgv3d_conv_winograd4_pack_weight", False, _plan_w_wino4),
    "w_pw_x3": _Form("w_pw_x3", "sgv3d_conv_pack_weight_x3", False, _plan_w_pw_x3),
    "w_wino4_x3": _Form("w_wino4_x3", "sgv3d_conv_winograd4_pack_weight_x3", False, _plan_w_wino4_x3),
    "w_pw_x3_deconv": _Form("w_pw_x3_deconv", "sgv3d_conv_pack_weight_x3", False, _plan_w_pw_x3_deconv),
    # fragment-ordered bf16 weights of the direct-weight kernel / of the patch kernel
    "w_dw": _Form("w_dw", "sgv3d_conv_dw_bf16_pack_weight", True, _plan_w_dw),
    "w_patch": _Form("w_patch", "sgv3d_conv3x3_patch_bf16_pack_weight", True, lambda pc, lib: (
        pc._keep, torch.empty(lib.sgv3d_conv3x3_patch_bf16_weight_bytes(pc.cout, pc.cin), dtype=_U8, device=pc._keep.device),
        (pc.cout, pc.cin), (), {})),
}


class PackedConv:
    """One convolution (or kernel==stride transposed convolution) with its weights repacked for the
    MFMA implicit-GEMM kernel and BN / bias folded into a per-channel scale & shift."""

    def __init__(self, weight, *, stride=1, pad=0, dil=1, scale=None, shift=None, relu=False,
                 transposed=False, cin_pad=None, device=None, tile=0, pad_out=False):
        w = weight.detach()
        device = device or w.device
        w = w.to(device=device, dtype=torch.float32).contiguous()
        # Channel counts that are not multiples of 4 (SGV3D's 87 / 174-channel BEV trunk) are padded:
        # inputs with zero weight columns (always), outputs with zero rows when the caller owns the
        # activation buffer (pad_out): the extra output channels come out exactly 0 and feed zero
        # weights downstream, so every pixel row stays 16-byte aligned for the kernels.
        odim = 1 if transposed else 0
        self.cout_real = int(w.shape[odim])
        out_align = 4 if pad_out is True else int(pad_out or 0)       # pad_out: True = 4, or the alignment itself
        if out_align and self.cout_real % out_align:
            extra = out_align - self.cout_real % out_align
            shape = list(w.shape)
            shape[odim] = extra
            w = torch.cat([w, w.new_zeros(shape)], odim).contiguous()
            if scale is not None:
                scale = torch.cat([scale.detach().float().to(device), torch.ones(extra, device=device)])
            if shift is not None:
                shift = torch.cat([shift.detach().float().to(device), torch.zeros(extra, device=device)])
        self.cin_real = int(w.shape[0] if transposed else w.shape[1])    # what the algorithmic flop count prices
        if cin_pad is None:
            cin_pad = (self.cin_real + 3) // 4 * 4
        if transposed:
            cin, cout, kh, kw = (int(s) for s in w.shape)
            assert kh == kw == stride, "only kernel == stride transposed convs (SECONDFPN deblocks)"
            self.ks = kh
            self.kh = self.kw = 1
            self.stride, self.pad, self.dil = 1, 0, 1
            gemm_n = cout * kh * kw
        else:
            cout, cin, kh, kw = (int(s) for s in w.shape)
            self.ks = 0
            self.kh, self.kw = kh, kw
            self.stride, self.pad, self.dil = int(stride), int(pad), int(dil)
            gemm_n = cout
        self.transposed = bool(transposed)
        self.cin = int(cin_pad) if cin_pad else cin
        assert self.cin >= cin and self.cin % 4 == 0, f"cin={cin} must be padded to a multiple of 4"
        self.cout = cout
        self.relu = bool(relu)
        self.tile = int(tile)
        k = self.cin if transposed else kh * kw * self.cin
        self.k_pad, self.cout_pad = pack_geometry(k, gemm_n)
        self.k_order = 1 if self.cin % 32 == 0 else 0      # channel-chunk-major k when possible
        self.scale = None if scale is None else scale.detach().to(device=device, dtype=torch.float32).contiguous()
        self.shift = None if shift is None else shift.detach().to(device=device, dtype=torch.float32).contiguous()
        # Every packed form of the weights (implicit GEMM, F(2x2) / F(4x4) Winograd, bf16 patch / direct-weight) is made on
        # first use: a training step packs the current weights of every layer twice (forward, data gradient) and only
        # needs the form its kernel choice reads.
        # (the attributes of _FORMS, and what their packers note down for the launch)
        self._w = self._w_wino = self.w_bf16 = self.w_f4res = self.w_wino4 = self.w_pw_x3 = self.w_wino4_x3 = self.w_dw = self.w_patch = None
        self.wino4_geom = self.pw_x3_cout_pad = self.wino4_x3_cout_pad = self._keep_dw = None
        self.w_pw_x3_deconv = self.pw_x3_deconv_cout_pad = self._keep_x3_deconv = None
        self._entry = None          # pack_cache._Entry when this object is kept across training steps (sgv3d_amd/pack_cache.py)
        self.device = device
        # Winograd F(2x2,3x3) covers the layer
        self.wino_ok = bool(WINOGRAD and not transposed and kh == 3 and kw == 3 and self.stride == 1 and self.dil == 1
                            and self.pad == 1 and self.cin % 8 == 0)
        self._keep = w  # the pack kernels read it asynchronously
        self._tile_cache = {}
        self.patch_ok = (not transposed and kh == 3 and kw == 3 and self.stride == 1 and self.dil == 1
                         and self.pad == 1 and self.cin % 32 == 0 and self.cout % 8 == 0 and self.cin == cin)

    def _form(self, name):
        """The packed weight form ``name`` of _FORMS, made on first use by its packer.  Bound to a pack-cache entry, a form that is a
        permutation of the parameter registers with it (refreshed in place from then on); one that is not makes the layer leave the
        cache (pack_cache._Entry.call)."""
        f = _FORMS[name]
        if self._entry is not None and not f.permutation:
            raise pack_cache.NotAPermutation(name)     # a transformed form: this layer packs per call
        buf = getattr(self, f.attr)
        if buf is not None:
            return buf
        lib = _lib.load()
        plan = f.plan(self, lib)
        if not plan:
            return None
        src, buf, before, after, notes = plan
        if before is not None:                  # (None: ``buf`` is a view of ``src``, nothing to launch)
            with torch.cuda.device(src.device):
                rc = getattr(lib, f.packer)(src.data_ptr(), *before, buf.data_ptr(), *after, _st(src))
            _lib.check(rc, f.packer)
        setattr(self, f.attr, buf)
        for k, v in notes.items():
            setattr(self, k, v)
        # kept across steps: refreshed in place from the parameter -- unless it is a view of the parameter itself
        if self._entry is not None and (before is not None or src.data_ptr() != self._entry.param.data_ptr()):
            self._entry.register(name, buf, lambda pc: pc._form(name))
        return buf

    w = property(lambda self: self._form('w'), doc="weights packed for the implicit-GEMM kernels, [cout_pad, k_pad] f32")
    w_wino = property(lambda self: self._form('w_wino'), doc="Winograd F(2x2,3x3) weights, None when the layer is not covered")

    _bf16_weights = partialmethod(_form, 'w_bf16')
    _dw_weights = partialmethod(_form, 'w_dw')
    _patch_weights = partialmethod(_form, 'w_patch')

    def wino4_ok(self, d=None, gate=None):
        """F(4x4,3x3) covers this layer (and launch): 3x3 / stride 1 / pad 1, f32, NHWC output, no gate, many channels."""
        is3x3 = (not self.transposed and self.kh == 3 and self.kw == 3 and self.stride == 1 and self.pad == self.dil)   # dilated too
        # enough channels for the transforms to be worth it -- or very many output channels on few input ones (the 64 -> 36 x 64
        # first layers of the CenterHead branches: the input transform is shared by all of them)
        wide = min(self.cin, self.cout) >= WINO4_MIN_CHANNELS or (self.cin >= 64 and self.cout >= 1024)
        ok = (WINO4 and WINOGRAD and is3x3 and not MFMA_BF16 and self.cin % 32 == 0 and self.cout % 4 == 0 and wide and gate is None)
        if ok and d is not None:
            ok = ((d.mode == CONV_NORMAL and d.y_ld % 4 == 0 and d.y_coff % 4 == 0) or
                  (d.mode == CONV_GROUP_PLANES and d.deconv_ks % 4 == 0)) and d.x_ld % 4 == 0 and d.x_coff % 4 == 0 and d.res_ld % 4 == 0
        return ok

    def f4res_ok(self, d=None, gate=None, io=0):
        """The resident F(4x4) kernel covers this layer (and launch): f32, 3x3 / stride 1 / pad 1 / dilation 1, NHWC in and
        out, no gate, and 64 input channels with 64 n output channels or 64 n input channels with 64 output channels."""
        ok = (F4RES and WINO4 and WINOGRAD and not MFMA_BF16 and not MFMA_F32X3 and not self.transposed and self.kh == 3
              and self.kw == 3 and self.stride == 1 and self.pad == 1 and self.dil == 1 and gate is None and io == 0
              and self.cin % 64 == 0 and self.cout % 64 == 0 and (self.cin == 64 or self.cout == 64))
        if ok and d is not None:
            ok = (d.mode == CONV_NORMAL and d.x_ld % 4 == 0 and d.x_coff % 4 == 0 and d.y_ld % 4 == 0 and d.y_coff % 4 == 0
                  and d.res_ld % 4 == 0)
        return ok

    def pw_x3_ok(self, d=None, gate=None, io=0):
        """The implicit-GEMM f32x3 kernel (csrc/conv_pw_x3.hip) covers this layer (and launch): a convolution with at most 32 taps and
        cin % 32 == 0 -- the 1x1 layers, the strided 3x3 / 1x1 layers between the stages, the patchify layers of the necks -- or, with
        tap-major weights, at most 64 taps and cin % 4 == 0 (the 7x7 stems); f32 tensors, NHWC output, no gate."""
        taps = self.kh * self.kw
        shape_ok = ((self.k_order == 1 and self.cin % 32 == 0 and self.cin >= 64 and taps <= 32) or        # channel-chunk-major k
                    (self.k_order == 0 and self.cin % 4 == 0 and taps <= 64 and taps * self.cin >= 128))   # tap-major k: the 7x7 stems
        ok = (PW_X3 and not MFMA_BF16 and not MFMA_F32X3 and not self.transposed and gate is None and io == 0 and shape_ok
              and self.cout % 4 == 0)
        if ok and d is not None:
            ok = (d.mode == CONV_NORMAL and d.x_ld % 4 == 0 and d.x_coff % 4 == 0 and d.y_ld % 4 == 0 and d.y_coff % 4 == 0
                  and d.res_ld % 4 == 0)
        return ok

    def _dw_eligible(self, d, gate=None, io=0):
        return (MFMA_BF16 and not MFMA_F32X3 and DW_BF16 and io == 3 and d.mode in (CONV_NORMAL, CONV_DECONV)
                and gate is None and self.cin % 32 == 0 and self.cout % 8 == 0 and d.x_ld % 8 == 0 and d.x_coff % 8 == 0
                and d.y_ld % 8 == 0 and d.y_coff % 8 == 0 and d.res_ld % 8 == 0)

    def out_hw(self, h, w):
        if self.transposed:
            return h * self.ks, w * self.ks
        oh = (h + 2 * self.pad - self.dil * (self.kh - 1) - 1) // self.stride + 1
        ow = (w + 2 * self.pad - self.dil * (self.kw - 1) - 1) // self.stride + 1
        return oh, ow

    def __call__(self, x, out=None, *, shift=None, **kw):
        """``shift``: a per-call replacement of the layer's per-channel shift (f32 [cout] on the device) -- for a layer whose
        bias depends on the input of THIS call (ASPP's pooled branch folded into the 1x1 convolution behind the concat)."""
        if shift is None:
            return self._call(x, out, **kw)
        assert shift.dtype == torch.float32 and shift.numel() == self.cout and shift.is_contiguous() and shift.device == x.device
        saved, self.shift = self.shift, shift
        try:
            return self._call(x, out, **kw)
        finally:
            self.shift = saved

    def _call(self, x, out=None, *, x_coff=0, y_coff=0, residual=None, gate=None, nchw_out=False, tile=None,
              group_planes=0, split_k=None, out_dtype=None):
        """x NHWC [B,H,W,x_ld]; reads channels [x_coff, x_coff+cin).  out NHWC [B,OH,OW,y_ld] written
        at channels [y_coff, y_coff+cout) (allocated [B,OH,OW,cout] if None).
        bf16 mode: ``x`` may be a bf16 tensor, and ``out_dtype=torch.bfloat16`` (or a bf16 ``out``) makes the layer write
        bf16 (then ``residual`` is bf16 too) -- NORMAL layout only."""
        B, H, W, x_ld = (int(s) for s in x.shape)
        assert x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)
        if out is not None:
            out_dtype = out.dtype
        out_dtype = out_dtype or torch.float32
        io = (1 if x.dtype == torch.bfloat16 else 0) | (2 if out_dtype == torch.bfloat16 else 0)
        if io:
            if not MFMA_BF16 or MFMA_F32X3:
                raise _lib.SGV3DError("bf16 tensors are only handled in bf16 mode (hip_ops.MFMA_BF16)")
            if io & 2:
                assert not (nchw_out or group_planes or gate is not None), "bf16 output: NORMAL / transposed-conv layouts only"
                assert residual is None or residual.dtype == torch.bfloat16
            else:
                assert residual is None or residual.dtype == torch.float32
        oh, ow = self.out_hw(H, W)
        if group_planes:
            # [cout/g, B, OH, OW, g]: one NHWC map per group of g output channels
            assert self.cout % group_planes == 0 and not self.transposed and residual is None
            if out is None:
                out = torch.empty(self.cout // group_planes, B, oh, ow, group_planes, dtype=torch.float32, device=x.device)
            assert out.is_contiguous() and out.numel() == B * oh * ow * self.cout
        elif out is None:
            shape = (B, self.cout, oh, ow) if nchw_out else (B, oh, ow, self.cout)
            out = torch.empty(shape, dtype=out_dtype, device=x.device)
        else:
            want = (B, None, oh, ow) if nchw_out else (B, oh, ow, None)
            got = tuple(int(v) for v in out.shape)
            if len(got) != 4 or any(w is not None and w != g for w, g in zip(want, got)) or not out.is_contiguous():
                raise _lib.SGV3DError(f"conv output buffer {got} does not match {want}")
        y_ld = int(out.shape[1] if nchw_out else out.shape[-1])
        if group_planes:
            y_ld, y_coff = self.cout, 0
        d = ConvDesc()
        d.batch, d.in_h, d.in_w, d.cin = B, H, W, self.cin
        d.out_h, d.out_w, d.cout = oh, ow, self.cout
        d.kh, d.kw, d.stride, d.pad, d.dil = self.kh, self.kw, self.stride, self.pad, self.dil
        d.x_ld, d.x_coff, d.y_ld, d.y_coff = x_ld, int(x_coff), y_ld, int(y_coff)
        d.res_ld = int(residual.shape[-1]) if residual is not None else 0
        d.relu = 1 if self.relu else 0
        d.mode = CONV_DECONV if self.transposed else (CONV_NCHW_OUT if nchw_out else CONV_NORMAL)
        d.deconv_ks = self.ks
        if group_planes:
            d.mode, d.deconv_ks = CONV_GROUP_PLANES, int(group_planes)
        d.k_pad, d.cout_pad = self.k_pad, self.cout_pad
        d.x_nchw = 0
        d.k_order = self.k_order
        lib = _lib.load()
        gemm_m = B * (H * W if self.transposed else oh * ow)
        gemm_n = self.cout * (self.ks * self.ks if self.transposed else 1)
        nkt = self.k_pad // 32
        t = int(self.tile if tile is None else tile)
        sk = int(split_k) if split_k else 0
        if t == 0 or sk == 0:
            key = (B, H, W, t, sk, MFMA_BF16, MFMA_F32X3, d.mode, residual is not None, gate is not None, io)
            choice = self._tile_cache.get(key)
            if choice is None:
                sig = (f"{self.cout}x{self.cin}k{self.kh}x{self.kw}s{self.stride}p{self.pad}d{self.dil}"
                       f"ks{self.ks}|{B}x{H}x{W}|m{d.mode}r{int(residual is not None)}g{int(gate is not None)}|{t}.{sk}"
                       + ("|bf16" if MFMA_BF16 else "|f32x3" if MFMA_F32X3 is True else "|x3auto" if MFMA_F32X3 else "")
                       + (f"|io{io}" if io else "") + f"|ts{TUNE_STREAMS}")    # choices are per frames-in-flight load
                choice = self._db_choice(sig, d, x, gate, gemm_m, gemm_n, nkt, t, sk, io)
                if choice is not None:
                    self._tile_cache[key] = choice
                    TUNE_STATS["from_db"] += 1
                elif tune_may_measure():
                    TUNE_STATS["measured"] += 1
                    choice = self._autotune(lib, d, x, residual, gate, out, gemm_m, gemm_n, nkt, t, sk, io)
                    self._tile_cache[key] = choice
                    tune_record(sig, choice)
                else:
                    choice = self._rule(t, sk, d, gemm_m, gemm_n, gate)
            t, sk = choice
        d.tile, d.split_k = t, sk
        name, flops, nbytes, extra = self._profile_record(TILES[t], sk, x, out, residual, gemm_m, io)
        with torch.cuda.device(x.device), prof(name, flops, nbytes, extra):
            rc = self._launch(lib, d, x, residual, gate, out, io)
        _lib.check(rc, "sgv3d_conv2d_forward")
        return out

    def _profile_record(self, T, sk, x, out, residual, gemm_m, io):
        """(label, algorithmic flops, algorithmic bytes, extra) of the launch with tile ``T`` for ``prof``.  The label names the
        INSTANTIATION launch_t (csrc/conv_igemm.hip) picks and ``extra['symbol']`` is the MFMA kernel's exact symbol, so that a
        per-symbol rocprof / PMC summary can be attached to exactly this kernel (bench.py load_traffic)."""
        B, H, W, _ = (int(s) for s in x.shape)
        ks2 = self.ks * self.ks if self.transposed else 1
        # ALGORITHMIC flops: real channel counts, not the zero-padded ones the kernel multiplies
        real_n = self.cout_real * ks2
        flops = 2.0 * gemm_m * real_n * (self.cin_real * self.kh * self.kw)
        plain = T.family == "igemm"
        x3 = plain and (T.x3 or (MFMA_F32X3 is True and not (T.mfirst or T.occ5)))
        name = (("conv_igemm_bf16_" if MFMA_BF16 else "conv_igemm_f32x3_" if x3 else "conv_igemm_") if plain else "conv_") + T.label
        pw1 = self.kh == 1 and self.kw == 1 and self.stride == 1 and self.pad == 0
        if plain and self.k_order == 0:
            name += "_tapmajor"        # the <.., false> instantiation (cin % 32 != 0: stems), a different kernel symbol
        elif plain and not MFMA_BF16 and not x3:
            # pointwise and five-per-CU forms
            if pw1 and not self.transposed and (T.occ5 or self.cin >= 128) and (T.occ5 or T.bm == 64):
                name += "_pw"
            if T.occ5:
                name += "_occ5"
        # algorithmic bytes: input map (the channels this layer reads), weights, output (+ residual), each once
        # (element sizes as the tensors are stored: bf16 activations in HBM count 2 bytes)
        nbytes = (float(x.element_size()) * B * H * W * self.cin_real
                  + (2.0 if MFMA_BF16 else 4.0) * self.cout_real * self.cin_real * self.kh * self.kw * ks2
                  + float(out.element_size()) * gemm_m * real_n
                  + (float(residual.element_size()) * gemm_m * real_n if residual is not None else 0.0))
        if PROFILE_DETAIL:
            name += (f"|{B}x{H}x{W}x{self.cin}->{self.cout} k{self.kh if not self.transposed else -self.ks} "
                     f"s{self.stride} d{self.dil} splitk{sk}" + (" mfirst" if plain and T.mfirst else "") + (" occ5" if T.occ5 else ""))
        if io:
            name = name.replace("conv_igemm_bf16_", "conv_igemm_bf16io_")
        extra = None
        if PROFILE is not None and not MFMA_BF16 and not x3 and T.symbol:
            b = lambda v: "true" if v else "false"
            # ({pw}: as the label ENDS here -- with PROFILE_DETAIL the shape suffix follows and the flag reads false)
            symbol = T.symbol.format(chunk=b(self.k_order != 0), pw=b(name.endswith(("_pw", "_pw_occ5"))),
                                     kmode=2 if self.k_order == 0 else 0 if pw1 else 1)
            if T.flops == "wino4":
                # the grouped GEMM of the three-launch F(4x4) path: 36 positions x rows (tiles padded to the GEMM's m-tile)
                oh, ow = self.out_hw(H, W)
                tiles = _wino4_tiles_per_phase(B, oh, ow, self.dil)
                mfma = 2.0 * 36 * (-(-tiles // T.bm) * T.bm) * self.cin * self.cout
            elif T.flops == "direct_k32":
                mfma = 2.0 * gemm_m * self.cout * _up32(self.cin * self.kh * self.kw)
            else:
                mfma = 2.0 * gemm_m * self.cout * self.cin * self.kh * self.kw * ks2
            extra = {"symbol": symbol, "mfma_flops": mfma}
            if T.x3:
                # six bf16 partial products per f32 product: the kernel's roofline is the bf16 MFMA peak over these flops
                extra["bf16_mfma_flops"] = 6 * mfma
        return name, flops, nbytes, extra

    def _rule(self, t, sk, d, gemm_m, gemm_n, gate=None):
        """Deterministic choice without measurement: Winograd for the layers it covers once the map has
        enough tiles to occupy the chip (split over channel steps to reach ~2 workgroups per CU), else the
        implicit-GEMM tile of the cost model; explicit tile / split arguments win."""
        if t == 0 and self.wino_ok and WINOGRAD and not MFMA_BF16 and d.out_h * d.out_w * d.batch >= 1024:
            wgs = d.batch * -(-d.out_h // 16) * -(-d.out_w // 16) * -(-gemm_n // 64)
            split = 1
            if not sk and SPLIT_K:
                for cand in (2, 3, 4, 6, 8):
                    if wgs * cand <= 512 and self.cin // 8 // cand >= 4:
                        split = cand
            return TILE_WINO, sk or split
        if t == 0 and self._patch_eligible(d, gate) and d.out_h * d.out_w * d.batch >= 4096:
            wgs = d.batch * -(-d.out_h // 16) * -(-d.out_w // 32) * -(-gemm_n // 64)
            split = 1
            if not sk and SPLIT_K:
                for cand in (2, 3, 4, 6, 8):
                    if wgs * cand <= 512 and self.cin // 32 // cand >= 2:
                        split = cand
            return TILE_PATCH, sk or split
        return (t or heuristic_tile(gemm_m, gemm_n)), (sk or 1)

    def _patch_eligible(self, d, gate=None):
        return (MFMA_BF16 and not MFMA_F32X3 and PATCH_BF16 and self.patch_ok and d.mode == CONV_NORMAL and gate is None
                and d.x_ld % 8 == 0 and d.x_coff % 8 == 0 and d.y_ld % 8 == 0 and d.y_coff % 8 == 0
                and (d.res_ld % 8 == 0))

    def _launch(self, lib, d, x, residual, gate, out, io=0):
        """Launch the kernel that host tile ``d.tile`` names (conv_tiles.TILES): its family's launcher, which checks that the kernel
        covers this layer and launch and hands the entry point a copy of ``d`` in the ABI's terms (``_abi``)."""
        T = TILES[d.tile]
        ws, nws = None, 0
        if d.split_k > 1 and T.family != "dw_bf16":
            nws = lib.sgv3d_conv2d_workspace_bytes(ctypes.byref(d))
            ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
        tail = (_lib.ptr(self.scale), _lib.ptr(self.shift), _lib.ptr(residual))
        return getattr(self, "_launch_" + T.entry)(lib, T, d, x, tail, gate, out, io, ws, nws)

    @staticmethod
    def _abi(d, T, k_pad=None, cout_pad=None):
        """``byref`` of a copy of the descriptor with ``tile`` as the entry point reads it (and the geometry of the weight form the
        kernel reads, where that is not the implicit-GEMM one).  ``d`` itself keeps the host id."""
        a = ConvDesc.from_buffer_copy(d)
        if T.abi is not None:
            a.tile = T.abi
        if k_pad is not None:
            a.k_pad, a.cout_pad = k_pad, cout_pad
        return ctypes.byref(a)

    def _launch_conv2d(self, lib, T, d, x, tail, gate, out, io, ws, nws):
        x3 = T.x3 or (MFMA_F32X3 is True)
        if T.occ5 and (MFMA_BF16 or x3 or io or self.k_order != 1):
            raise _lib.SGV3DError("the five-per-CU 64x64 tile is f32 only and needs channel-chunk-major weights (cin % 32 == 0)")
        if io:
            return lib.sgv3d_conv2d_forward_bf16io(self._abi(d, T), x.data_ptr(), self._bf16_weights().data_ptr(), *tail, _lib.ptr(gate),
                                                   out.data_ptr(), _lib.ptr(ws), nws, _st(x), int(io))
        fwd = (lib.sgv3d_conv2d_forward_bf16 if MFMA_BF16 else
               lib.sgv3d_conv2d_forward_f32x3 if x3 else lib.sgv3d_conv2d_forward)
        return fwd(self._abi(d, T), x.data_ptr(), self.w.data_ptr(), *tail, _lib.ptr(gate), out.data_ptr(), _lib.ptr(ws), nws, _st(x))

    def _launch_winograd(self, lib, T, d, x, tail, gate, out, io, ws, nws):
        if not self.wino_ok:
            raise _lib.SGV3DError("this layer has no Winograd weights (needs 3x3 / stride 1 / pad 1 / cin % 8 == 0)")
        return lib.sgv3d_conv2d_winograd_forward(self._abi(d, T), x.data_ptr(), self.w_wino.data_ptr(), *tail, _lib.ptr(gate),
                                                 out.data_ptr(), _lib.ptr(ws), nws, _st(x))

    def _launch_winograd4(self, lib, T, d, x, tail, gate, out, io, ws, nws):
        if not self.wino4_ok(d, gate) or d.split_k > 1:
            raise _lib.SGV3DError("F(4x4) Winograd covers f32 3x3 / stride 1 / pad 1 layers with cin % 32 == 0, cout % 4 == 0, "
                                  "NHWC output, no gate, no split-K")
        u = self._form(T.form)
        a = self._abi(d, T, self.cin, self.wino4_x3_cout_pad) if T.x3 else self._abi(d, T, *self.wino4_geom)
        nws4 = lib.sgv3d_conv2d_winograd4_workspace_bytes(a)
        ws4 = torch.empty(nws4, dtype=torch.uint8, device=x.device)
        return lib.sgv3d_conv2d_winograd4_forward(a, x.data_ptr(), u.data_ptr(), *tail, out.data_ptr(), ws4.data_ptr(), nws4, _st(x))

    def _launch_f4res(self, lib, T, d, x, tail, gate, out, io, ws, nws):
        if not self.f4res_ok(d, gate, io) or d.split_k > 1 or x.dtype != torch.float32:
            raise _lib.SGV3DError("the resident F(4x4) kernel covers f32 3x3 / stride 1 / pad 1 layers with 64 input channels "
                                  "(cout % 64 == 0) or 64 output channels (cin % 64 == 0), NHWC output, no gate, no split-K")
        return lib.sgv3d_conv3x3_f4res_forward(self._abi(d, T), x.data_ptr(), self._form(T.form).data_ptr(), *tail, out.data_ptr(), _st(x))

    def _launch_x3(self, lib, T, d, x, tail, gate, out, io, ws, nws):
        if not self.pw_x3_ok(d, gate, io) or x.dtype != torch.float32:
            raise _lib.SGV3DError("the implicit-GEMM f32x3 kernel covers f32 layers with at most 32 taps, cin % 32 == 0 (>= 64), cout % 4 == 0, "
                                  "NHWC output, no gate")
        u = self._form(T.form)
        return lib.sgv3d_conv2d_x3_forward(self._abi(d, T, d.k_pad, self.pw_x3_cout_pad), x.data_ptr(), u.data_ptr(), *tail, out.data_ptr(),
                                           _lib.ptr(ws), nws, _st(x))

    def _launch_patch_bf16(self, lib, T, d, x, tail, gate, out, io, ws, nws):
        if not self._patch_eligible(d, gate):
            raise _lib.SGV3DError("the bf16 patch kernel covers 3x3 / stride 1 / pad 1 layers with cin % 32 == 0 in bf16 mode")
        return lib.sgv3d_conv3x3_patch_bf16_forward(d.batch, d.in_h, d.in_w, self.cin, self.cout, d.x_ld, d.x_coff, d.y_ld,
                                                    d.y_coff, d.res_ld, d.relu, x.data_ptr(), self._patch_weights().data_ptr(),
                                                    *tail, out.data_ptr(), int(io), int(d.split_k), _lib.ptr(ws), nws, _st(x))

    def _launch_dw_bf16(self, lib, T, d, x, tail, gate, out, io, ws, nws):
        if not self._dw_eligible(d, gate, io) or (d.split_k > 1 and d.mode != CONV_NORMAL):
            raise _lib.SGV3DError("the bf16 direct-weight kernel covers layers with cin % 32 == 0, cout % 8 == 0 and bf16 tensors in "
                                  "and out (NHWC), no gate; split-K in NORMAL mode only")
        if d.split_k > 1:
            nws = lib.sgv3d_conv_dw_bf16_workspace_bytes(ctypes.byref(d))
            ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
            return lib.sgv3d_conv_dw_bf16_forward_splitk(self._abi(d, T), x.data_ptr(), self._dw_weights().data_ptr(), *tail,
                                                         out.data_ptr(), ws.data_ptr(), nws, _st(x))
        return lib.sgv3d_conv_dw_bf16_forward(self._abi(d, T), x.data_ptr(), self._dw_weights().data_ptr(), *tail, out.data_ptr(), _st(x))

    def _time_under_load(self, lib, d, x, residual, gate, out, rounds=None, io=0):
        """Time for TUNE_STREAMS concurrent copies of the launch, ``rounds`` back to back on every stream (all copies
        write the same values to ``out``; split-K workspaces are per launch)."""
        global _TUNE_SIDE_STREAMS
        cur = torch.cuda.current_stream(x.device)
        if len(_TUNE_SIDE_STREAMS) < TUNE_STREAMS:
            _TUNE_SIDE_STREAMS = [torch.cuda.Stream(device=x.device) for _ in range(TUNE_STREAMS)]
        best = None
        rounds = rounds or TUNE_ROUNDS
        for _ in range(TUNE_REPEATS):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            for s in _TUNE_SIDE_STREAMS[:TUNE_STREAMS]:
                s.wait_event(e0)
                with torch.cuda.stream(s):
                    for _r in range(rounds):
                        self._launch(lib, d, x, residual, gate, out, io)
                cur.wait_stream(s)
            e1.record(cur)
            e1.synchronize()
            dt = e0.elapsed_time(e1)
            best = dt if best is None else min(best, dt)
        return best

    def _candidates(self, d, gate, gemm_m, gemm_n, nkt, fixed_tile, fixed_split, io=0):
        """The (tile, (split-K, ...)) pairs this layer may run with on this input / output layout under the module's current
        switches (WINOGRAD, WINO4, WINO_HALF, PATCH_BF16, DW_*, SPLIT_K, MFIRST, MFMA_*): what the first-call measurement times,
        and what a tune-DB entry is checked against before it is trusted (``_db_choice``)."""
        sel = conv_tiles.select
        # an m-tile-first walk needs more than one channel tile
        mfirst = lambda t: MFIRST and d.mode in (CONV_NORMAL, CONV_NCHW_OUT) and gemm_n > TILES[t].bn
        tiles = sel("igemm") + tuple(t for t in sel("igemm", mfirst=True) if mfirst(t))
        if OCC5 and self.k_order == 1 and not MFMA_BF16 and not MFMA_F32X3 and io == 0:
            tiles += sel("igemm", occ5=True) + tuple(t for t in sel("igemm", occ5=True, mfirst=True) if mfirst(t))
        if MFMA_F32X3 == "auto" and not MFMA_BF16:
            tiles += sel("igemm", x3=True)
        if self.wino_ok and WINOGRAD and not MFMA_BF16:
            tiles += (TILE_WINO,)
            if WINO_HALF:
                tiles += (TILE_WINO_HALF,)
            if self.cin <= 96 and self.cout >= 128:
                tiles += (TILE_WINO_RES,)

        if self.wino4_ok(d, gate):            # (also the dilated 3x3 layers, which the F(2x2) kernels do not cover)
            tiles += ((TILE_WINO4, TILE_WINO4_WIDE) + ((TILE_WINO4_NARROW,) if self.cin >= 128 else ()) + ((TILE_WINO4_OCC,) if OCC5 else ())
                      + ((TILE_WINO4_G48,) if WINO4_G48 and self.k_order == 1 else ()))
            if WINO4_X3 and not MFMA_F32X3:
                tiles += self._x3_tiles(d)
        if self.f4res_ok(d, gate, io):
            tiles += (TILE_F4RES,)
        if self.pw_x3_ok(d, gate, io):
            tiles += _pw_x3_tiles(gemm_m, gemm_n, nkt)
        if self._patch_eligible(d, gate):
            tiles += (TILE_PATCH,)
        if self._dw_eligible(d, gate, io):
            dw = lambda bm, bn, deep=False: (conv_tiles.by_shape("dw_bf16", bm, bn, deep),)
            deep = self.kh * self.kw * self.cin >= 512              # enough k for the 128-pixel wave tiles to pay
            tiles += (dw(64, 256) + (dw(128, 256) if deep else ()) if gemm_n > 128 else
                      dw(128, 128) + (dw(256, 128) if deep else ()) if gemm_n > 64 else dw(128, 128) + dw(256, 64))
            if DW_DEEP and self.kh * self.kw * self.cin >= 256:     # few workgroups per CU: the two-chunks-ahead form of the 64-pixel tiles
                if gemm_n > 128 and -(-gemm_m // 64) * -(-gemm_n // 256) <= DW_DEEP_MAX_WGS:
                    tiles += dw(64, 256, True)
                    if DW_NARROW and -(-gemm_m // 64) * -(-gemm_n // 256) <= 384:
                        tiles += dw(64, 128) + dw(64, 128, True)
                elif 64 < gemm_n <= 128 and -(-gemm_m // 128) * -(-gemm_n // 128) <= DW_DEEP_MAX_WGS:
                    tiles += dw(128, 128, True)
        if fixed_tile:
            tiles = (fixed_tile,)
        cands = []
        for t in tiles:
            T = TILES[t]
            wgs = -(-gemm_m // T.bm) * -(-gemm_n // T.bn)
            nk = nkt
            if T.spatial:
                th, tw, kc = T.spatial
                nk = self.cin // kc     # F(2x2): k-steps of 8 channels, nk // s >= 8 keeps >= 4 steps per split; patch: stages of 32, >= 2 per split
                wgs = d.batch * -(-d.out_h // th) * -(-d.out_w // tw) * -(-gemm_n // T.bn)
            if T.family == "dw_bf16":
                nk = -(-(self.kh * self.kw * (self.cin // 32)) // 2)      # chunks of 64 k; >= 4 per split
            if T.split is None or (T.family == "dw_bf16" and (d.mode != CONV_NORMAL or not DW_SPLIT_K)):
                splits = (1,)
            elif fixed_split:
                splits = (fixed_split,)
            else:
                splits = (1,) + _split_factors(T.split, nk, wgs)
            cands.append((t, splits))
        return cands

    def _x3_tiles(self, d):
        """The shapes of the f32x3 position GEMM worth timing for this layer: m-tiles that waste at most 10 % of the rows as padding
        (the smallest waste always), 160 columns only where they cover cout with fewer idle columns than 128 do."""
        tiles = _wino4_tiles_per_phase(d.batch, d.out_h, d.out_w, d.dil)
        waste = {r: (-(-tiles // r) * r - tiles) / tiles for r in sorted(set(X3_TILE_ROWS.values()))}
        best = min(waste.values())
        ms = [r for r in waste if waste[r] <= max(best, 0.10) and (r <= 64 or tiles >= r)]
        idle = lambda c: -(-self.cout // c) * c - self.cout
        cols = [128] + ([160] if idle(160) < idle(128) else [])
        return tuple(conv_tiles.by_shape("wino4_x3", r, c) for c in cols for r in ms)

    def _db_choice(self, sig, d, x, gate, gemm_m, gemm_n, nkt, fixed_tile, fixed_split, io=0):
        """The tune-DB entry of ``sig`` if it is one of the candidates this layer would be measured with right now, else None
        (and the stale entry is dropped, so the caller measures or applies the rule).  A DB is a record of measurements, not
        an override: the kill switches (SGV3D_NO_WINOGRAD, SGV3D_WINO4=0, SGV3D_DW_BF16=0, SGV3D_NO_SPLITK, ...), an
        input / output layout the recorded kernel does not cover (channel offsets / strides are not part of the
        signature) and SGV3D_NO_AUTOTUNE (the documented fixed rule) all win over it, and the committed ``tune/gfx950_*``
        entries only apply on a gfx950 device."""
        choice = tune_lookup(sig, x.device)
        if choice is None:
            return None
        t, sk = int(choice[0]), int(choice[1])
        for ct, splits in self._candidates(d, gate, gemm_m, gemm_n, nkt, fixed_tile, fixed_split, io):
            if ct == t and sk in splits:
                return (t, sk)
        del TUNE_DB[sig]
        _COMMITTED_SIGS.discard(sig)
        return None

    def _autotune(self, lib, d, x, residual, gate, out, gemm_m, gemm_n, nkt, fixed_tile, fixed_split, io=0):
        """Time the candidate (tile, split-K) pairs on the real buffers and keep the fastest.  Results do
        not depend on the tile shape (every output element sums k in the same order); split-K changes
        the association of the k sum (partials added in fixed order), still deterministic."""
        cands = self._candidates(d, gate, gemm_m, gemm_n, nkt, fixed_tile, fixed_split, io)
        best, best_t = (cands[0][0], fixed_split or 1), None
        with torch.cuda.device(x.device):
            for t, splits in cands:
                for sk in splits:
                    d.tile, d.split_k = t, sk
                    _lib.check(self._launch(lib, d, x, residual, gate, out, io), "sgv3d_conv2d_forward")   # warm
                    if TUNE_STREAMS > 1:
                        dt = self._time_under_load(lib, d, x, residual, gate, out, io=io)
                    else:
                        nrep = max(4, TUNE_ROUNDS * TUNE_REPEATS // 2)
                        evs = [torch.cuda.Event(enable_timing=True) for _ in range(nrep + 1)]
                        evs[0].record()
                        for r in range(nrep):
                            self._launch(lib, d, x, residual, gate, out, io)
                            evs[r + 1].record()
                        evs[-1].synchronize()
                        dt = min(evs[r].elapsed_time(evs[r + 1]) for r in range(nrep))
                    if TUNE_VERBOSE:
                        print(f"[tune] {self.cout}x{self.cin}k{self.kh} {d.batch}x{d.in_h}x{d.in_w}: tile {t} split {sk}: {dt * 1e3:.1f} us", flush=True)
                    if best_t is None or dt < best_t:
                        best, best_t = (t, sk), dt
        return best


PAIR_BF16 = _os.environ.get("SGV3D_PAIR_BF16", "1") != "0"   # 0: conv2 + conv3 of a bottleneck are always two launches


# Independent pieces of ONE forward as parallel branches of the captured hipGraph -- BUILT, MEASURED, OFF BY DEFAULT
# (SGV3D_PARALLEL_BRANCHES=1 turns it on).  A batch-1 frame is a chain of ~130 launches, and the narrow ones -- the strided
# shortcut of a residual stage, the four SECONDFPN levels, the 27-feature gate MLPs, the pooled ASPP branch -- leave most CUs
# idle while the next launch waits for them although it does not need their result.  Inside a stream capture ``run_parallel``
# puts every piece on a forked stream and joins them, so the graph gets parallel branches; outside a capture the pieces run in
# order on the current stream.  Every piece writes its own buffer or channel slice: results are bitwise the sequential ones.
# Measured on cfg-2 (round 4, one call, same box): the ~30 fork / join pairs per frame cost more than the overlap returns --
# one frame in flight 169.3 -> 160.7 frames/s, three in flight 209.0 -> 163.3, the harness step 153.3 -> 147.8: every
# cross-stream edge of a hipGraph is a barrier packet plus a semaphore between hardware queues, tens of microseconds each,
# where the kernels it lets overlap are 10-60 us long.
PARALLEL_BRANCHES = _os.environ.get("SGV3D_PARALLEL_BRANCHES", "0") == "1"
_BRANCH_POOL = {}
_BRANCH_TOP = {}


_OWNED_STREAMS = {}       # device index -> cuda_stream handles handed out by distinct_stream() and still meant to be distinct


def distinct_stream(device, avoid=()):
    """A ``torch.cuda.Stream`` whose underlying HIP stream is none of ``avoid`` (streams), not the current stream and none that
    this function handed out before on the device.  ``torch.cuda.Stream()`` draws round-robin from a pool of 32 per device: the
    33rd object IS the first one's stream again, and a fork of a stream capture onto the capturing stream itself (or onto another
    branch of the same capture) is not the graph the code meant -- after enough pipelines / graphed forwards in one process that
    happened (a crash inside hipStreamEndCapture in the GPU suite, round 6)."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    taken = _OWNED_STREAMS.setdefault(key, set())
    banned = {st.cuda_stream for st in avoid if st is not None} | {torch.cuda.current_stream(dev).cuda_stream} | taken
    for _ in range(64):
        st = torch.cuda.Stream(device=dev)
        if st.cuda_stream not in banned:
            if len(taken) < 24:                     # (beyond that the pool cannot keep everything distinct: best effort)
                taken.add(st.cuda_stream)
            return st
    return torch.cuda.Stream(device=dev)


def release_stream(st):
    """Give a stream of ``distinct_stream`` back (its owner is gone)."""
    for taken in _OWNED_STREAMS.values():
        taken.discard(st.cuda_stream)


def run_parallel(device, thunks):
    """``[t() for t in thunks]``; inside a stream capture the thunks are forked branches of the graph (the first one stays on
    the capturing stream).  A call from inside a forked branch runs its thunks in sequence."""
    thunks = list(thunks)
    if len(thunks) <= 1 or not PARALLEL_BRANCHES or not torch.cuda.is_current_stream_capturing():
        return [t() for t in thunks]
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    pool = _BRANCH_POOL.setdefault(key, [])
    top = _BRANCH_TOP.get(key, 0)
    if top > 0:
        # already inside a forked branch: in sequence (forks nested three deep -- MSCThead's scales -> ASPP -> pooled branch --
        # crashed hipStreamEndCapture on ROCm 7.2)
        return [t() for t in thunks]
    need = top + len(thunks) - 1
    while len(pool) < need:
        pool.append(distinct_stream(dev, pool))
    mine = pool[top:need]
    _BRANCH_TOP[key] = need
    cur = torch.cuda.current_stream(dev)
    results = [None] * len(thunks)
    try:
        for st, (i, t) in zip(mine, list(enumerate(thunks))[1:]):
            st.wait_stream(cur)                                   # fork
            with torch.cuda.stream(st):
                results[i] = t()
        results[0] = thunks[0]()
    finally:
        for st in mine:
            cur.wait_stream(st)                                   # join (every forked stream must rejoin the capture)
        _BRANCH_TOP[key] = top
    return results


# A capture that wants to be cut into several hipGraphs (pipeline.GraphedForward) installs a callback here; the forward calls
# graph_split_point() where a cut is useful (after the image backbone's first stage).  None: the call does nothing.
_GRAPH_SPLIT_HOOK = None


def graph_split_point(tag):
    if _GRAPH_SPLIT_HOOK is not None:
        _GRAPH_SPLIT_HOOK(tag)


def switch_state():
    """Every module-level switch that decides WHICH kernels a forward launches, as one hashable value: part of the key of
    anything that records launches for replay (BEVHeight's per-signature hipGraph)."""
    g = globals()
    return tuple(g.get(k) for k in ("AUTOTUNE", "SPLIT_K", "WINOGRAD", "FUSED_HEAD", "HEAD_PATH", "MFMA_BF16", "BF16_ACTIVATIONS",
                                    "MFMA_F32X3", "MFIRST", "WINO4", "WINO_HALF", "PATCH_BF16", "DW_BF16", "DW_DEEP", "DW_NARROW",
                                    "DW_SPLIT_K", "DW_DEEP_MAX_WGS", "PAIR_BF16", "TUNE_STREAMS", "PARALLEL_BRANCHES", "F4RES", "OCC5", "WINO4_G48", "DCN_FUSED", "WINO4_X3", "WINO4_MULTI", "PW_X3",
                                    "DCN_FUSED_BF16", "DCN_FUSED_TRAIN", "TRAIN_BF16_STORAGE", "SHORTCUT_X3", "DECONV_X3", "VIT_BF16", "STEM_FUSED"))


def conv_pair_eligible(a, b, x, residual=None):
    """conv ``a`` (k x k, 256 outputs, ReLU) followed by the 1x1 conv ``b`` (cout % 256 == 0) between bf16 NHWC tensors: the pair
    the fused direct-weight kernel (sgv3d_conv_dw_bf16_pair_forward) covers."""
    return (MFMA_BF16 and not MFMA_F32X3 and DW_BF16 and PAIR_BF16 and x.dtype == torch.bfloat16 and not a.transposed and not b.transposed
            and a.cout == 256 and a.cin % 32 == 0 and int(x.shape[-1]) % 8 == 0 and b.cin == 256 and b.kh == 1 and b.kw == 1
            and b.stride == 1 and b.pad == 0 and b.cout % 256 == 0 and (residual is None or residual.dtype == torch.bfloat16))


def conv_pair_bf16(a, b, x, residual=None, out=None):
    """``b(a(x), residual=residual)`` for two PackedConvs in one launch (bf16 tensors); the map between them stays in LDS."""
    B, H, W, x_ld = (int(v) for v in x.shape)
    oh, ow = a.out_hw(H, W)
    if out is None:
        out = torch.empty(B, oh, ow, b.cout, dtype=torch.bfloat16, device=x.device)
    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin = B, H, W, a.cin
    d.out_h, d.out_w, d.cout = oh, ow, a.cout
    d.kh, d.kw, d.stride, d.pad, d.dil = a.kh, a.kw, a.stride, a.pad, a.dil
    d.x_ld, d.x_coff, d.y_ld, d.y_coff = x_ld, 0, a.cout, 0
    d.relu, d.mode, d.split_k = (1 if a.relu else 0), CONV_NORMAL, 1
    flops = 2.0 * B * oh * ow * (a.cout_real * a.cin_real * a.kh * a.kw + b.cout_real * b.cin_real)
    name = "conv_dw_bf16_pair"
    if PROFILE_DETAIL:
        name += f"|{B}x{H}x{W}x{a.cin}->{a.cout} k{a.kh} s{a.stride} d{a.dil} ->{b.cout} k1"
    with torch.cuda.device(x.device), prof(name, flops):
        rc = _lib.load().sgv3d_conv_dw_bf16_pair_forward(
            ctypes.byref(d), x.data_ptr(), a._dw_weights().data_ptr(), _lib.ptr(a.scale), _lib.ptr(a.shift), b.cout,
            b._dw_weights().data_ptr(), _lib.ptr(b.scale), _lib.ptr(b.shift), _lib.ptr(residual),
            int(residual.shape[-1]) if residual is not None else 0, out.data_ptr(), int(out.shape[-1]), 0, 1 if b.relu else 0, _st(x))
    _lib.check(rc, "sgv3d_conv_dw_bf16_pair_forward")
    return out


def conv_pair_choice(a, b, x, residual=None):
    """True when the fused launch is faster than ``b(a(x))`` with the per-layer choices: measured once per pair and input shape
    under the load the pipeline runs (like the per-layer choices) and kept in the tune DB under a ``pair|`` signature."""
    if not conv_pair_eligible(a, b, x, residual):
        return False
    B, H, W, _ = (int(v) for v in x.shape)
    sig = (f"pair|{a.cout}x{a.cin}k{a.kh}x{a.kw}s{a.stride}p{a.pad}d{a.dil}->{b.cout}|{B}x{H}x{W}|r{int(residual is not None)}|bf16|ts{TUNE_STREAMS}")
    hit = tune_lookup(sig, x.device)
    if hit is not None:
        return bool(hit[0])
    if not tune_may_measure():                               # the fixed rule: fused
        return True
    act = torch.bfloat16
    two = lambda: b(a(x, out_dtype=act), residual=residual, out_dtype=act)
    one = lambda: conv_pair_bf16(a, b, x, residual)
    two(); one()                                             # (both sides warm before either is timed: not tune_best_of's order)
    t2 = time_callable(two, x.device)
    t1 = time_callable(one, x.device)
    tune_record(sig, [1 if t1 < t2 else 0, 0])
    return t1 < t2


# fp32 path: a bottleneck's conv3 and the shortcut projection of its stage's first block as ONE launch of the f32x3 implicit-GEMM kernel
# (csrc/conv_pw_x3.hip MODE 3, sgv3d_conv2d_x3_shortcut_forward): the shortcut map is never written or read back.  0
# (SGV3D_SHORTCUT_X3=0): always two launches.
SHORTCUT_X3 = _os.environ.get("SGV3D_SHORTCUT_X3", "1") != "0"


def conv_shortcut_eligible(c3, ds, mid, x):
    """``c3`` (1x1 / stride 1, the bottleneck's last layer, applied to ``mid``) and ``ds`` (1x1 / stride 1 or 2, no ReLU, the shortcut
    projection, applied to the block's input ``x``) with the same output shape, f32 NHWC tensors, cin % 32 == 0 on both, in the fp32
    mode with the f32x3 pointwise kernel enabled: the pair the two-source launch (``conv_shortcut_x3``) covers."""
    if not (SHORTCUT_X3 and PW_X3 and not MFMA_BF16 and not MFMA_F32X3):
        return False
    if c3.transposed or ds.transposed or mid.dtype != torch.float32 or x.dtype != torch.float32:
        return False
    one = lambda c: c.kh == 1 and c.kw == 1 and c.pad == 0 and c.cin % 32 == 0
    if not (one(c3) and one(ds) and c3.stride == 1 and ds.stride in (1, 2) and not ds.relu and c3.cout == ds.cout and c3.cout % 4 == 0):
        return False
    B, H, W, x_ld = (int(v) for v in x.shape)
    return (tuple(int(v) for v in mid.shape[:3]) == (B,) + ds.out_hw(H, W) and int(mid.shape[-1]) % 4 == 0 and x_ld % 4 == 0
            and int(mid.shape[-1]) >= c3.cin and x_ld >= ds.cin)


def _shortcut_rule_tile(gemm_m, gemm_n):
    """The fixed rule's tile of the two-source launch: 128 channels per workgroup, the largest m-tile of 128 / 64 / 32 pixels that
    still gives two workgroups to each of the 256 CUs (the smallest otherwise)."""
    plain = {PW_X3_DIMS[t]: t for t in PW_X3_TILES if not TILES[t].mfirst}
    for bm in (128, 64):
        if -(-gemm_m // bm) * -(-gemm_n // 128) >= 512:
            return plain[bm, 128]
    return plain[32, 128]


def _shortcut_tiles(gemm_m, gemm_n):
    """The tiles of the two-source launch worth timing: the per-layer candidate list's (``_pw_x3_tiles``) for a launch that cannot split
    K -- without 128 x 64, the one instantiation of the two-source form that spills registers."""
    return _pw_x3_tiles(gemm_m, gemm_n, skip=((128, 64),)) or (_shortcut_rule_tile(gemm_m, gemm_n),)


def conv_shortcut_x3(c3, ds, mid, x, out=None, tile=None):
    """``c3(mid, residual=ds(x))`` in one launch, bit for bit what the two f32x3 launches (split-K 1) give.  ``tile``: a host id of
    the pw_x3 family (default: the fixed rule's)."""
    B, H, W, x_ld = (int(v) for v in x.shape)
    oh, ow = ds.out_hw(H, W)
    assert mid.is_contiguous() and x.is_contiguous() and tuple(int(v) for v in mid.shape[:3]) == (B, oh, ow)
    if out is None:
        out = torch.empty(B, oh, ow, c3.cout, dtype=torch.float32, device=x.device)
    gemm_m = B * oh * ow
    T = TILES[int(tile or _shortcut_rule_tile(gemm_m, c3.cout))]
    if T.family != "pw_x3":
        raise _lib.SGV3DError(f"conv_shortcut_x3: tile {T.id} is not a tile of the f32x3 pointwise kernel")
    da, db = ConvDesc(), ConvDesc()
    for d, c, (h, w), ld in ((da, c3, (oh, ow), int(mid.shape[-1])), (db, ds, (H, W), x_ld)):
        d.batch, d.in_h, d.in_w, d.cin = B, h, w, c.cin
        d.out_h, d.out_w, d.cout = oh, ow, c.cout
        d.kh, d.kw, d.stride, d.pad, d.dil = 1, 1, c.stride, 0, 1
        d.x_ld, d.x_coff, d.y_ld, d.y_coff, d.res_ld = ld, 0, int(out.shape[-1]), 0, 0
        d.relu, d.mode, d.split_k, d.tile = (1 if c.relu else 0), CONV_NORMAL, 1, T.abi
        d.k_pad, d.k_order = c.k_pad, c.k_order
    ua, ub = c3._form(T.form), ds._form(T.form)
    da.cout_pad, db.cout_pad = c3.pw_x3_cout_pad, ds.pw_x3_cout_pad
    flops = 2.0 * gemm_m * (c3.cout_real * c3.cin_real + ds.cout_real * ds.cin_real)
    nbytes = 4.0 * (gemm_m * c3.cin_real + B * H * W * ds.cin_real + c3.cout_real * c3.cin_real + ds.cout_real * ds.cin_real
                    + gemm_m * c3.cout_real)
    name, extra = "conv_pw_x3_shortcut", None
    if PROFILE_DETAIL:
        name += f"|{B}x{oh}x{ow}x{c3.cin}->{c3.cout} k1 s1 + {B}x{H}x{W}x{ds.cin}->{ds.cout} k1 s{ds.stride}"
    if PROFILE is not None:
        mfma = 2.0 * gemm_m * c3.cout * (c3.cin + ds.cin)
        extra = {"symbol": f"conv_pw_x3_kernel<{T.bm // 16}, {T.bn // 32}, 3>", "mfma_flops": mfma, "bf16_mfma_flops": 6 * mfma}
    with torch.cuda.device(x.device), prof(name, flops, nbytes, extra):
        rc = _lib.load().sgv3d_conv2d_x3_shortcut_forward(
            ctypes.byref(da), mid.data_ptr(), ua.data_ptr(), _lib.ptr(c3.scale), _lib.ptr(c3.shift),
            ctypes.byref(db), x.data_ptr(), ub.data_ptr(), _lib.ptr(ds.scale), _lib.ptr(ds.shift), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_conv2d_x3_shortcut_forward")
    return out


def conv_shortcut_signature(c3, ds, x):
    B, H, W, _ = (int(v) for v in x.shape)
    return f"pair|shortcut|{c3.cout}x{c3.cin}+{ds.cin}s{ds.stride}|{B}x{H}x{W}|r{int(c3.relu)}|ts{TUNE_STREAMS}"


def conv_shortcut_choice(c3, ds, mid, x):
    """The host tile id to run ``conv_shortcut_x3`` with, or 0 when ``c3(mid, residual=ds(x))`` with the per-layer choices is the
    faster way (or the pair is not covered).  Measured once per pair and input shape under the load the pipeline runs -- the fused
    launch with each of its tiles against the two launches -- and kept in the tune DB under a ``pair|shortcut|`` signature as
    [fused or not, the fused launch's tile].  The fixed rule (SGV3D_NO_AUTOTUNE, deterministic mode, a capture that meets a new
    signature): fused, with ``_shortcut_rule_tile``."""
    if not conv_shortcut_eligible(c3, ds, mid, x):
        return 0
    gemm_m, gemm_n = int(mid.shape[0]) * int(mid.shape[1]) * int(mid.shape[2]), c3.cout
    rule = _shortcut_rule_tile(gemm_m, gemm_n)
    sig = conv_shortcut_signature(c3, ds, x)
    hit = tune_lookup(sig, x.device)
    if hit is not None:
        on, t = (int(v) for v in hit)
        if not on:
            return 0
        return t if t in PW_X3_TILES else rule
    if not tune_may_measure():
        return rule
    TUNE_STATS["measured"] += 1
    out = torch.empty(tuple(mid.shape[:3]) + (c3.cout,), dtype=torch.float32, device=x.device)
    t2, best, t1 = tune_best_of(sig, x.device, lambda: c3(mid, out, residual=ds(x)),
                                [(t, lambda t=t: conv_shortcut_x3(c3, ds, mid, x, out, tile=t)) for t in _shortcut_tiles(gemm_m, gemm_n)])
    on = t1 < t2
    tune_record(sig, [1, best] if on else [0, 0])
    return best if on else 0

# fp32 path: sibling F(4x4) layers on ONE input (ASPP's three dilated branches) with one launch of the input transform and one of
# the output transform for all of them (csrc/conv_wino4.hip: sgv3d_conv2d_winograd4_forward_multi) instead of one each; the
# grouped GEMMs run as they do per layer, and the result is bit-equal.  0 (SGV3D_WINO4_MULTI=0): always the per-layer calls.
WINO4_MULTI = _os.environ.get("SGV3D_WINO4_MULTI", "1") != "0"
WINO4_MULTI_MAX = 4


def _wino4_sibling_choice(conv, x):
    """(tile, split-K) ``conv(x)`` runs with, as far as it is known without a launch: the layer's own fixed tile, else what its
    first call on this input shape looked up or measured (``_tile_cache``); (0, 0) before that call and where the fixed rule
    decides per call."""
    B, H, W, _ = (int(v) for v in x.shape)
    t = int(conv.tile)
    if t in WINO4_X3_TILES:
        return t, 1
    return conv._tile_cache.get((B, H, W, t, 0, MFMA_BF16, MFMA_F32X3, CONV_NORMAL, False, False, 0), (0, 0))


def wino4_multi_eligible(convs, x, out=None, y_coffs=None, training=False):
    """``convs`` are 2..4 F(4x4) layers (3x3 / stride 1 / pad == dilation, f32, the same cin) applied to the same f32 NHWC ``x`` in
    the fp32 mode, outside training and SGV3D_PARALLEL_BRANCHES, writing channel slices of an f32 NHWC ``out``."""
    if not (WINO4_MULTI and WINO4_X3 and WINO4 and WINOGRAD and not MFMA_BF16 and not MFMA_F32X3 and not PARALLEL_BRANCHES and not training):
        return False
    if not 2 <= len(convs) <= WINO4_MULTI_MAX or x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        return False
    if int(x.shape[0]) < 1 or int(x.shape[-1]) % 4:
        return False
    if any((not c.wino4_ok()) or c.cin != convs[0].cin or c.cin > int(x.shape[-1]) for c in convs):
        return False
    if out is not None:
        ld = int(out.shape[-1])
        if (out.dtype != torch.float32 or out.dim() != 4 or not out.is_contiguous() or tuple(out.shape[:3]) != tuple(x.shape[:3]) or ld % 4
                or y_coffs is None or len(y_coffs) != len(convs)
                or any(int(o) % 4 or int(o) < 0 or int(o) + c.cout > ld for o, c in zip(y_coffs, convs))):
            return False
    return True


def wino4_multi_signature(convs, x):
    B, H, W, _ = (int(v) for v in x.shape)
    return (f"pair|wino4multi|{'+'.join(f'{c.cout}x{c.cin}d{c.dil}' for c in convs)}|{B}x{H}x{W}|ts{TUNE_STREAMS}")


def wino4_multi(convs, x, out, y_coffs, tiles):
    """``convs[l](x, out, y_coff=y_coffs[l], tile=tiles[l], split_k=1)`` for all l through the multi entry point: one input-transform
    launch, the grouped GEMMs, one output-transform launch."""
    n = len(convs)
    if not wino4_multi_eligible(convs, x, out, y_coffs) or len(tiles) != n or any(int(t) not in WINO4_X3_TILES for t in tiles):
        raise _lib.SGV3DError("wino4_multi covers 2..4 F(4x4) layers with f32x3 tiles on one f32 NHWC input in the fp32 mode")
    B, H, W, x_ld = (int(v) for v in x.shape)
    lib = _lib.load()
    descs = (ConvDesc * n)()
    us, flops, nbytes = [], 0.0, 4.0 * B * H * W * convs[0].cin_real
    for l, (c, t) in enumerate(zip(convs, tiles)):
        d = descs[l]
        d.batch, d.in_h, d.in_w, d.cin = B, H, W, c.cin
        d.out_h, d.out_w, d.cout = H, W, c.cout
        d.kh, d.kw, d.stride, d.pad, d.dil = 3, 3, 1, c.pad, c.dil
        d.x_ld, d.x_coff, d.y_ld, d.y_coff = x_ld, 0, int(out.shape[-1]), int(y_coffs[l])
        d.res_ld, d.relu, d.mode, d.deconv_ks = 0, 1 if c.relu else 0, CONV_NORMAL, c.ks
        T = TILES[int(t)]
        us.append(c._form(T.form))
        d.k_pad, d.cout_pad, d.tile, d.x_nchw, d.k_order, d.split_k = c.cin, c.wino4_x3_cout_pad, T.abi, 0, c.k_order, 1
        flops += 2.0 * B * H * W * c.cout_real * c.cin_real * 9
        nbytes += 4.0 * c.cout_real * c.cin_real * 9 + 4.0 * B * H * W * c.cout_real
    arr = lambda ps: (ctypes.c_void_p * n)(*[p or None for p in ps])
    pu, psc, psh, py = (arr([u.data_ptr() for u in us]), arr([_lib.ptr(c.scale) for c in convs]), arr([_lib.ptr(c.shift) for c in convs]),
                        arr([out.data_ptr()] * n))          # (host arrays: alive until the call returns)
    nws = lib.sgv3d_conv2d_winograd4_multi_workspace_bytes(n, ctypes.addressof(descs))
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device), prof("conv_wino4_x3_multi", flops, nbytes):
        rc = lib.sgv3d_conv2d_winograd4_forward_multi(n, ctypes.addressof(descs), x.data_ptr(), ctypes.addressof(pu), ctypes.addressof(psc),
                                                      ctypes.addressof(psh), ctypes.addressof(py), ws.data_ptr(), nws, _st(x))
    _lib.check(rc, "sgv3d_conv2d_winograd4_forward_multi")
    return out


def wino4_multi_choice(convs, x, out, y_coffs, training=False):
    """The f32x3 tiles to run ``wino4_multi`` with, or None when the per-layer calls are the way (the group is not covered, a layer's
    choice for this input is not an f32x3 F(4x4) tile without split-K -- or not known yet: the first frame runs per layer -- or the
    measurement said so).  Measured once per group and input shape against the per-layer calls and kept in the tune DB under a
    ``pair|wino4multi|`` signature as [multi or not, 0].  The fixed rule (SGV3D_NO_AUTOTUNE, deterministic mode, a capture that meets
    a new signature): the multi launch wherever it is covered."""
    if not wino4_multi_eligible(convs, x, out, y_coffs, training):
        return None
    picks = [_wino4_sibling_choice(c, x) for c in convs]
    if any(t not in WINO4_X3_TILES or sk != 1 for t, sk in picks):
        return None
    tiles = tuple(t for t, _ in picks)
    sig = wino4_multi_signature(convs, x)
    hit = tune_lookup(sig, x.device)
    if hit is not None:
        return tiles if int(hit[0]) else None
    if not tune_may_measure():
        return tiles
    TUNE_STATS["measured"] += 1

    def separate():
        for c, o, t in zip(convs, y_coffs, tiles):
            c(x, out, y_coff=o, tile=t, split_k=1)
    t0, _, t1 = tune_best_of(sig, x.device, separate, [(1, lambda: wino4_multi(convs, x, out, y_coffs, tiles))])
    on = t1 < t0
    tune_record(sig, [1 if on else 0, 0])
    return tiles if on else None


# fp32 path: the kernel == stride transposed convolutions of the SECONDFPN necks on the f32x3 pointwise kernel (csrc/conv_pw_x3.hip
# MODE 4: a 1x1 GEMM with ks * ks * cout columns and the transposed-conv scatter in its epilogue) instead of the f32 MFMA
# implicit-GEMM kernel.  0 (SGV3D_DECONV_X3=0): always the layer's per-layer choice.
DECONV_X3 = _os.environ.get("SGV3D_DECONV_X3", "1") != "0"


def deconv_x3_eligible(conv, x, out=None, y_coff=0):
    """``conv`` is a kernel == stride transposed convolution with cin % 32 == 0 and cout % 4 == 0 between f32 NHWC tensors, in the
    fp32 mode with the f32x3 pointwise kernel enabled: the layers ``deconv_x3`` covers."""
    if not (DECONV_X3 and PW_X3 and not MFMA_BF16 and not MFMA_F32X3):
        return False
    if not conv.transposed or conv.ks < 1 or conv.cin % 32 or conv.cout % 4 or x.dtype != torch.float32 or x.dim() != 4:
        return False
    x_ld = int(x.shape[-1])
    if x_ld % 4 or x_ld < conv.cin or int(y_coff) % 4 or int(y_coff) < 0:
        return False
    if out is not None:
        B, H, W, _ = (int(v) for v in x.shape)
        return (out.dtype == torch.float32 and out.dim() == 4 and tuple(int(v) for v in out.shape[:3]) == (B,) + conv.out_hw(H, W)
                and int(out.shape[-1]) % 4 == 0 and int(out.shape[-1]) >= int(y_coff) + conv.cout)
    return True


def _deconv_x3_rule(gemm_m, gemm_n):
    """The fixed rule of ``deconv_x3``: (tile, split-K) = 128 channels per workgroup, the largest m-tile that still gives every CU two
    workgroups, and no split-K -- what the per-layer fixed rule gives a NORMAL 1x1 layer of this GEMM size."""
    return _shortcut_rule_tile(gemm_m, gemm_n), 1


def _deconv_x3_candidates(gemm_m, gemm_n, nkt):
    """The (tile, splits) pairs of ``deconv_x3`` worth timing: the per-layer candidate list's tiles (``_pw_x3_tiles``) and split-K factors
    (``_split_factors``) for a NORMAL 1x1 layer of this GEMM size (m-tile first does not apply to the scatter)."""
    wgs = lambda t: -(-gemm_m // TILES[t].bm) * -(-gemm_n // TILES[t].bn)
    out = tuple((t, (1,) + _split_factors("igemm", nkt, wgs(t))) for t in _pw_x3_tiles(gemm_m, gemm_n, nkt, mfirst=False))
    return out or ((_shortcut_rule_tile(gemm_m, gemm_n), (1,)),)


def deconv_x3(conv, x, out=None, y_coff=0, tile=None, split_k=None):
    """The transposed convolution ``conv`` (kernel == stride, folded BN, ReLU) of ``x`` written to channels
    [y_coff, y_coff + cout) of ``out``, on the f32x3 pointwise kernel.  ``tile``: a host id of the pw_x3 family, ``split_k``: the
    split-K factor (default: the fixed rule's)."""
    B, H, W, x_ld = (int(v) for v in x.shape)
    oh, ow = conv.out_hw(H, W)
    assert x.is_contiguous() and conv.transposed
    if out is None:
        out = torch.empty(B, oh, ow, conv.cout, dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(int(v) for v in out.shape[:3]) == (B, oh, ow)
    gemm_m, gemm_n = B * H * W, conv.ks * conv.ks * conv.cout
    rule_t, rule_s = _deconv_x3_rule(gemm_m, gemm_n)
    T = TILES[int(tile or rule_t)]
    sk = int(split_k or rule_s)
    if T.family != "pw_x3":
        raise _lib.SGV3DError(f"deconv_x3: tile {T.id} is not a tile of the f32x3 pointwise kernel")
    u = conv._form("w_pw_x3_deconv")
    d = ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin = B, H, W, conv.cin
    d.out_h, d.out_w, d.cout = oh, ow, conv.cout
    d.kh, d.kw, d.stride, d.pad, d.dil = 1, 1, 1, 0, 1
    d.x_ld, d.x_coff, d.y_ld, d.y_coff, d.res_ld = x_ld, 0, int(out.shape[-1]), int(y_coff), 0
    d.relu, d.mode, d.deconv_ks, d.split_k, d.tile = (1 if conv.relu else 0), CONV_DECONV, conv.ks, sk, T.abi
    d.k_pad, d.cout_pad, d.k_order = conv.cin, conv.pw_x3_deconv_cout_pad, 1
    ws, nws = None, 0
    if sk > 1:
        nws = 4 * sk * gemm_m * gemm_n
        ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    real_n = conv.cout_real * conv.ks * conv.ks
    flops = 2.0 * gemm_m * real_n * conv.cin_real
    nbytes = 4.0 * (gemm_m * conv.cin_real + real_n * conv.cin_real + gemm_m * real_n)
    name, extra = "conv_pw_x3_deconv", None
    if PROFILE_DETAIL:
        name += f"|{B}x{H}x{W}x{conv.cin}->{conv.cout} k{-conv.ks} s1 d1 splitk{sk}"
    if PROFILE is not None:
        mfma = 2.0 * gemm_m * gemm_n * conv.cin
        extra = {"symbol": f"conv_pw_x3_kernel<{T.bm // 16}, {T.bn // 32}, 4>", "mfma_flops": mfma, "bf16_mfma_flops": 6 * mfma}
    with torch.cuda.device(x.device), prof(name, flops, nbytes, extra):
        rc = _lib.load().sgv3d_conv2d_x3_forward(ctypes.byref(d), x.data_ptr(), u.data_ptr(), _lib.ptr(conv.scale), _lib.ptr(conv.shift),
                                                 None, out.data_ptr(), _lib.ptr(ws), nws, _st(x))
    _lib.check(rc, "sgv3d_conv2d_x3_forward")
    return out


def deconv_x3_signature(conv, x):
    B, H, W, _ = (int(v) for v in x.shape)
    return f"pair|deconv|{conv.cout}x{conv.cin}ks{conv.ks}|{B}x{H}x{W}|r{int(conv.relu)}|ts{TUNE_STREAMS}"


def deconv_x3_choice(conv, x, out=None, y_coff=0):
    """(host tile id, split-K) to run ``deconv_x3`` with, or None when the layer's per-layer f32 choice is the faster way (or the
    layer is not covered).  Measured once per layer and input shape under the load the pipeline runs -- the x3 launch with each of
    its tiles and split-K factors against ``conv(x)`` -- and kept in the tune DB under a ``pair|deconv|`` signature as
    [x3 or not, 100 * split-K + the x3 launch's tile] ([0, 0]: not).  The fixed rule (SGV3D_NO_AUTOTUNE, deterministic mode, a
    capture that meets a new signature): x3, with ``_deconv_x3_rule``."""
    if not deconv_x3_eligible(conv, x, out, y_coff):
        return None
    B, H, W, _ = (int(v) for v in x.shape)
    gemm_m, gemm_n, nkt = B * H * W, conv.ks * conv.ks * conv.cout, conv.cin // 32
    rule = _deconv_x3_rule(gemm_m, gemm_n)
    sig = deconv_x3_signature(conv, x)
    hit = tune_lookup(sig, x.device)
    if hit is not None:
        on, code = (int(v) for v in hit)
        if not on:
            return None
        sk, t = divmod(code, 100)
        ok = t in PW_X3_TILES and not TILES[t].mfirst and 1 <= sk <= max(1, nkt) and (sk == 1 or SPLIT_K)
        return (t, sk) if ok else rule
    if not tune_may_measure():
        return rule
    TUNE_STATS["measured"] += 1
    if out is None:
        out = torch.empty((B,) + conv.out_hw(H, W) + (conv.cout,), dtype=torch.float32, device=x.device)
    t2, best, t1 = tune_best_of(sig, x.device, lambda: conv(x, out, y_coff=y_coff),
                                [((t, sk), lambda t=t, sk=sk: deconv_x3(conv, x, out, y_coff, tile=t, split_k=sk))
                                 for t, splits in _deconv_x3_candidates(gemm_m, gemm_n, nkt) for sk in splits])
    on = t1 < t2
    tune_record(sig, [1, 100 * best[1] + best[0]] if on else [0, 0])
    return best if on else None


# fp32 path: the image stem -- NCHW ingest, 7x7 / stride 2 convolution with folded BN and ReLU, 3x3 / stride 2 max-pool -- as ONE launch
# (csrc/stem_pool_x3.hip, sgv3d_stem_pool_x3_forward: f32x3 products, bit for bit the x3 tap-major convolution between the two small
# kernels) instead of three; neither the 4-channel NHWC copy of the image nor the un-pooled map reaches memory.  0
# (SGV3D_STEM_FUSED=0): always the three launches.
STEM_FUSED = _os.environ.get("SGV3D_STEM_FUSED", "1") != "0"
# variant code of sgv3d_stem_pool_x3_forward -> (pooled rows, pooled columns) per workgroup
STEM_FUSED_VARIANTS = {0: (4, 16)}


def stem_fused_eligible(conv, imgs, act_dtype=None, maxpool=True):
    """``conv`` is a 7x7 / stride 2 / pad 3 layer from 3 image channels to 64 with folded BN and ReLU, followed by the 3x3 / stride 2 /
    pad 1 max-pool (``maxpool``), applied to the contiguous f32 NCHW tensor ``imgs``, in the fp32 mode (``act_dtype``: the network's
    activation dtype, None = f32 tensors) with the f32x3 pointwise kernel enabled: the stem ``stem_fused`` covers."""
    if not (STEM_FUSED and PW_X3 and not MFMA_BF16 and not MFMA_F32X3) or act_dtype is not None or not maxpool:
        return False
    if conv.transposed or conv._entry is not None or not conv.relu or conv.scale is None or conv.shift is None:
        return False
    if (conv.kh, conv.kw, conv.stride, conv.pad, conv.dil) != (7, 7, 2, 3, 1) or (conv.cin_real, conv.cin, conv.cout_real, conv.cout) != (3, 4, 64, 64):
        return False
    return (torch.is_tensor(imgs) and imgs.dim() == 4 and int(imgs.shape[1]) == 3 and imgs.dtype == torch.float32 and imgs.is_contiguous()
            and imgs.numel() > 0)


def stem_fused_out_hw(h, w):
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (hc - 1) // 2 + 1, (wc - 1) // 2 + 1


def stem_fused(conv, imgs, out=None, variant=None):
    """``maxpool3x3s2(conv(nchw_to_nhwc(imgs, c_pad=4)))`` in one launch, bit for bit what the three launches give with ``conv`` on the
    f32x3 tap-major kernel (split-K 1).  ``variant``: a key of STEM_FUSED_VARIANTS (default 0)."""
    B, C, H, W = (int(v) for v in imgs.shape)
    assert C == 3 and imgs.is_contiguous() and imgs.dtype == torch.float32
    variant = int(variant or 0)
    if variant not in STEM_FUSED_VARIANTS:
        raise _lib.SGV3DError(f"stem_fused: unknown variant {variant}")
    hc, wc = conv.out_hw(H, W)
    hp, wp = stem_fused_out_hw(H, W)
    if out is None:
        out = torch.empty(B, hp, wp, conv.cout, dtype=torch.float32, device=imgs.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(int(v) for v in out.shape[:3]) == (B, hp, wp)
    u = conv._form("w_pw_x3")
    flops = 2.0 * B * hc * wc * 64 * 147
    nbytes = 4.0 * (B * 3 * H * W + 64 * 147 + B * hp * wp * 64)
    name, extra = "conv_stem_fused", None
    if PROFILE_DETAIL:
        name += f"|{B}x{H}x{W}x3->64 k7 s2 + maxpool v{variant}"
    if PROFILE is not None:
        tph, tpw = STEM_FUSED_VARIANTS[variant]
        # executed: per workgroup the (2 tph + 1) x (2 tpw + 1) conv pixels of its tile in groups of 16, two groups at a time on each
        # half of the waves, x 64 channels x K = 224 (196 padded)
        ng = -(-(2 * tph + 1) * (2 * tpw + 1) // 16)
        groups = 2 * (-(-ng // 4) + -(-(ng - 1) // 4))
        mfma = 2.0 * B * -(-hp // tph) * -(-wp // tpw) * groups * 16 * 64 * 224
        extra = {"symbol": f"stem_pool_x3_kernel<{tph}, {tpw}>", "mfma_flops": mfma, "bf16_mfma_flops": 6 * mfma}
    with torch.cuda.device(imgs.device), prof(name, flops, nbytes, extra):
        rc = _lib.load().sgv3d_stem_pool_x3_forward(B, H, W, imgs.data_ptr(), u.data_ptr(), u.numel() * u.element_size(),
                                                    _lib.ptr(conv.scale), _lib.ptr(conv.shift), out.data_ptr(), int(out.shape[-1]), variant,
                                                    _st(imgs))
    _lib.check(rc, "sgv3d_stem_pool_x3_forward")
    return out


def stem_fused_signature(conv, imgs):
    B, _, H, W = (int(v) for v in imgs.shape)
    return f"pair|stem|{conv.cout}x{conv.cin_real}k{conv.kh}|{B}x{H}x{W}|ts{TUNE_STREAMS}"


def stem_fused_choice(conv, imgs, act_dtype=None, maxpool=True):
    """The variant to run ``stem_fused`` with, or None when the three launches (``nchw_to_nhwc``, ``conv`` with its per-layer choice,
    ``maxpool3x3s2``) are the faster way (or the stem is not covered).  Measured once per image shape under the load the pipeline runs
    -- the fused launch with each of its variants against the three launches -- and kept in the tune DB under a ``pair|stem|``
    signature as [fused or not, the fused launch's variant].  The fixed rule (SGV3D_NO_AUTOTUNE, deterministic mode, a capture that
    meets a new signature): fused, variant 0."""
    if not stem_fused_eligible(conv, imgs, act_dtype, maxpool):
        return None
    sig = stem_fused_signature(conv, imgs)
    hit = tune_lookup(sig, imgs.device)
    if hit is not None:
        on, v = (int(x) for x in hit)
        if not on:
            return None
        return v if v in STEM_FUSED_VARIANTS else 0
    if not tune_may_measure():
        return 0
    TUNE_STATS["measured"] += 1
    t3, best, t1 = tune_best_of(sig, imgs.device, lambda: maxpool3x3s2(conv(nchw_to_nhwc(imgs, c_pad=conv.cin))),
                                [(v, lambda v=v: stem_fused(conv, imgs, variant=v)) for v in STEM_FUSED_VARIANTS])
    on = t1 < t3
    tune_record(sig, [1, best] if on else [0, 0])
    return best if on else None


def time_callable(fn, device, rounds=None):
    """Milliseconds for TUNE_STREAMS concurrent copies of ``fn`` (``rounds`` calls back to back on every stream; one stream =
    isolated timing), best of TUNE_REPEATS -- how the per-layer candidates are timed, for whole sub-graphs (the CenterHead
    branch paths).  ``fn`` launches on torch's current stream."""
    global _TUNE_SIDE_STREAMS
    rounds = rounds or TUNE_ROUNDS
    cur = torch.cuda.current_stream(device)
    n = max(1, TUNE_STREAMS)
    if len(_TUNE_SIDE_STREAMS) < n:
        _TUNE_SIDE_STREAMS = [torch.cuda.Stream(device=device) for _ in range(n)]
    best = None
    for _ in range(TUNE_REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        for s_ in _TUNE_SIDE_STREAMS[:n]:
            s_.wait_event(e0)
            with torch.cuda.stream(s_):
                for _r in range(rounds):
                    fn()
            cur.wait_stream(s_)
        e1.record(cur)
        e1.synchronize()
        dt = e0.elapsed_time(e1)
        best = dt if best is None else min(best, dt)
    return best


def _dense_layout(t, *dtypes):
    """The small-layer entry points take raw pointers: a view with other strides or another dtype would be read as if it were
    the contiguous tensor of the expected type and give a silently wrong frame."""
    return t.is_contiguous() and t.dtype in (dtypes or (torch.float32,))


_F32_OR_BF16 = (torch.float32, torch.bfloat16)


def maxpool3x3s2(x, out=None):
    B, H, W, C = (int(s) for s in x.shape)
    assert _dense_layout(x, *_F32_OR_BF16)
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty(B, oh, ow, C, dtype=x.dtype, device=x.device)
    assert _dense_layout(out, x.dtype) and tuple(out.shape) == (B, oh, ow, C)
    with torch.cuda.device(x.device), prof("maxpool3x3s2"):
        if x.dtype == torch.bfloat16:
            rc = _lib.load().sgv3d_maxpool3x3s2_bf16(B, H, W, C, x.data_ptr(), out.data_ptr(), _st(x))
        else:
            rc = _lib.load().sgv3d_maxpool3x3s2(B, H, W, C, x.data_ptr(), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_maxpool3x3s2")
    return out


def nchw_to_nhwc(x, c_pad=None, out=None):
    B, C, H, W = (int(s) for s in x.shape)
    assert x.is_contiguous() and x.dtype == torch.float32
    c_pad = int(c_pad or C)
    if out is None:
        out = torch.empty(B, H, W, c_pad, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), prof("nchw_to_nhwc"):
        rc = _lib.load().sgv3d_nchw_to_nhwc(B, C, H, W, c_pad, x.data_ptr(), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_nchw_to_nhwc")
    return out


def nhwc_to_nchw(x, channels=None, coff=0, out=None):
    B, H, W, ld = (int(s) for s in x.shape)
    C = int(channels or ld)
    assert _dense_layout(x)
    if out is None:
        out = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    assert _dense_layout(out) and out.numel() == B * C * H * W
    with torch.cuda.device(x.device), prof("nhwc_to_nchw"):
        rc = _lib.load().sgv3d_nhwc_to_nchw(B, C, H, W, ld, int(coff), x.data_ptr(), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_nhwc_to_nchw")
    return out


def global_avgpool(x, out=None):
    B, H, W, C = (int(s) for s in x.shape)
    assert _dense_layout(x, *_F32_OR_BF16)
    if out is None:
        out = torch.empty(B, C, dtype=torch.float32, device=x.device)
    assert _dense_layout(out) and out.numel() == B * C
    lib = _lib.load()
    nbytes = lib.sgv3d_global_avgpool_workspace_bytes(B, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    fn = lib.sgv3d_global_avgpool_bf16 if x.dtype == torch.bfloat16 else lib.sgv3d_global_avgpool
    with torch.cuda.device(x.device), prof("global_avgpool"):
        rc = fn(B, H * W, C, C, x.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, _st(x))
    _lib.check(rc, "sgv3d_global_avgpool")
    return out


ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def dense(x, w, scale=None, bias=None, act=ACT_NONE, out=None, run=None):
    """x [B,K], w [N,K] -> act(scale*(x @ w.T) + bias) [B,N].  ``run``: int32 device flag; 0 skips the launch's work and leaves
    ``out`` (then required) as it is (sgv3d_dense_gated)."""
    B, K = (int(s) for s in x.shape)
    N = int(w.shape[0])
    assert int(w.shape[1]) == K and x.is_contiguous() and w.is_contiguous()
    assert run is None or out is not None
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == (B, N) and out.dtype == torch.float32 and out.is_contiguous()
    with torch.cuda.device(x.device), prof("dense"):
        if run is not None:
            rc = _lib.load().sgv3d_dense_gated(B, K, N, x.data_ptr(), w.data_ptr(), _lib.ptr(scale), _lib.ptr(bias),
                                              int(act), out.data_ptr(), run.data_ptr(), _st(x))
        else:
            rc = _lib.load().sgv3d_dense(B, K, N, x.data_ptr(), w.data_ptr(), _lib.ptr(scale), _lib.ptr(bias),
                                        int(act), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_dense")
    return out


def broadcast_channels(v, out, y_coff=0):
    """v [B,C] written to out[b, :, :, y_coff:y_coff+C] for every pixel (out NHWC)."""
    B, H, W, ld = (int(s) for s in out.shape)
    C = int(v.shape[1])
    assert _dense_layout(v) and int(v.shape[0]) == B and _dense_layout(out, *_F32_OR_BF16)
    lib = _lib.load()
    fn = lib.sgv3d_broadcast_channels_bf16 if out.dtype == torch.bfloat16 else lib.sgv3d_broadcast_channels
    with torch.cuda.device(out.device), prof("broadcast_channels"):
        rc = fn(B, H * W, C, ld, int(y_coff), v.data_ptr(), out.data_ptr(), _st(out))
    _lib.check(rc, "sgv3d_broadcast_channels")
    return out


def scale_channels(x, gate, out=None):
    """x NHWC [B,H,W,C] * gate [B,C] (SELayer gating)."""
    B, H, W, C = (int(s) for s in x.shape)
    assert tuple(gate.shape) == (B, C) and x.is_contiguous() and gate.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    lib = _lib.load()
    fn = lib.sgv3d_scale_channels_bf16 if x.dtype == torch.bfloat16 else lib.sgv3d_scale_channels
    with torch.cuda.device(x.device), prof("scale_channels"):
        rc = fn(B, H * W, C, x.data_ptr(), gate.data_ptr(), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_scale_channels")
    return out


def copy_channels(x, out, coff=0):
    """out[B,H,W,C] (contiguous) = x[B,H,W,coff:coff+C]."""
    B, H, W, ld = (int(s) for s in x.shape)
    C = int(out.shape[-1])
    assert _dense_layout(x) and _dense_layout(out) and out.numel() == B * H * W * C
    with torch.cuda.device(x.device), prof("copy_channels"):
        rc = _lib.load().sgv3d_copy_channels(B, H * W, C, ld, int(coff), x.data_ptr(), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_copy_channels")
    return out


def upsample_bilinear2x(x, out=None):
    B, H, W, C = (int(s) for s in x.shape)
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(B, 2 * H, 2 * W, C, dtype=x.dtype, device=x.device)
    lib = _lib.load()
    fn = lib.sgv3d_upsample_bilinear2x_bf16 if x.dtype == torch.bfloat16 else lib.sgv3d_upsample_bilinear2x
    with torch.cuda.device(x.device), prof("upsample_bilinear2x"):
        rc = fn(B, H, W, C, x.data_ptr(), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_upsample_bilinear2x")
    return out


def add_mul_sigmoid(a, b, c, out=None):
    """a + b * sigmoid(c), same-shape contiguous tensors."""
    assert a.shape == b.shape == c.shape and a.is_contiguous() and b.is_contiguous() and c.is_contiguous()
    assert a.dtype == b.dtype == c.dtype
    if out is None:
        out = torch.empty_like(a)
    lib = _lib.load()
    fn = lib.sgv3d_add_mul_sigmoid_bf16 if a.dtype == torch.bfloat16 else lib.sgv3d_add_mul_sigmoid
    with torch.cuda.device(a.device), prof("add_mul_sigmoid"):
        rc = fn(a.numel(), a.data_ptr(), b.data_ptr(), c.data_ptr(), out.data_ptr(), _st(a))
    _lib.check(rc, "sgv3d_add_mul_sigmoid")
    return out


def bsm_compose(height_context, semantic_logits, D, ctx, sem, thr):
    """In place on height_context [B,H,W,ld]; semantic_logits [B,H,W,>=sem]."""
    B, H, W, ld = (int(s) for s in height_context.shape)
    assert _dense_layout(height_context) and _dense_layout(semantic_logits)
    assert tuple(semantic_logits.shape[:3]) == (B, H, W) and int(semantic_logits.shape[-1]) >= int(sem)
    with torch.cuda.device(height_context.device), prof("bsm_compose"):
        rc = _lib.load().sgv3d_bsm_compose(B, H * W, int(D), int(ctx), int(sem), ld, semantic_logits.data_ptr(),
                                          int(semantic_logits.shape[-1]), float(thr), height_context.data_ptr(),
                                          _st(height_context))
    _lib.check(rc, "sgv3d_bsm_compose")
    return height_context


DCN_FUSED = _os.environ.get("SGV3D_DCN_FUSED", "1") != "0"     # 0: deformable im2col + one GEMM per group (rounds 1-4)
# bf16 compute mode: the one-launch form of csrc/dcn_fused_bf16.hip.  On: 2.6 - 3.7 x faster than the im2col form in all four cases
# of tools/dcn_probe.py bf16 (profiles/dcn_bf16_bench.json).  SGV3D_DCN_FUSED_BF16=0 keeps the im2col form in bf16
# mode only; SGV3D_DCN_FUSED=0 switches it off together with the f32 launch.
DCN_FUSED_BF16 = _os.environ.get("SGV3D_DCN_FUSED_BF16", "1") != "0"
# mixed-precision TRAINING step (MFMA_BF16 with TRAIN_BF16_WGRAD, f32 tensors): the DCN is misc_grad.deform_conv3x3 -- the one-launch
# forward above, the weight gradient with the samples recomputed (csrc/dcn_grad.hip) and the gather-form sampling adjoint in every
# mode; no column tensor is kept.  0 (SGV3D_DCN_FUSED_TRAIN=0): im2col + one 1x1 convolution per group.  On: the graphed cfg-2 batch-2
# step is 29.94 ms against 30.94 ms, ten times the run-to-run spread (profiles/dcn_train_step_ab.json).
DCN_FUSED_TRAIN = _os.environ.get("SGV3D_DCN_FUSED_TRAIN", "1") != "0"


def deform_conv3x3_eligible(x, convs):
    """f32 NHWC input, packed group weights that share one geometry, channels per group a multiple of 32: what
    sgv3d_deform_conv3x3_forward covers (the bf16 compute mode has a launch of its own: deform_conv3x3_bf16_eligible)."""
    cpg9 = convs[0].cin
    return (DCN_FUSED and not MFMA_BF16 and not MFMA_F32X3 and x.dtype == torch.float32 and len(convs) <= 8 and cpg9 % 9 == 0
            and (cpg9 // 9) % 32 == 0 and convs[0].cout % 4 == 0 and convs[0].k_order == 1
            and all(c.cin == cpg9 and c.cout == convs[0].cout and c.k_pad == convs[0].k_pad and c.cout_pad == convs[0].cout_pad
                    and c.scale is None and c.shift is None and not c.relu for c in convs))


def deform_conv3x3(x, offset, convs, out=None, y_coff=0):
    """DCNv1 forward (lss_fpn.py:190-198) in one launch: x f32 NHWC [B,H,W,C], offset f32 [B,H,W,>=18], ``convs`` the per-group
    PackedConvs of the [opg, 9 * cpg] matrices (k = tap * cpg + ci).  Writes out[..., y_coff : y_coff + groups * opg]."""
    import ctypes
    B, H, W, C = (int(v) for v in x.shape)
    g, opg = len(convs), convs[0].cout
    assert x.is_contiguous() and offset.is_contiguous() and offset.dtype == torch.float32 and int(offset.shape[-1]) >= 18
    if out is None:
        out = torch.empty(B, H, W, g * opg, dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape[:3]) == (B, H, W)
    ptrs = (ctypes.c_void_p * g)(*[c.w.data_ptr() for c in convs])
    flops = 2.0 * B * H * W * g * opg * (convs[0].cin_real)
    nbytes = 4.0 * (B * H * W * (C + 18 + g * opg) + g * opg * convs[0].cin_real)
    with torch.cuda.device(x.device), prof("conv_dcn_fused", flops, nbytes,
                                           {"symbol": "dcn3x3_fused_kernel", "mfma_flops": 2.0 * B * H * W * g * convs[0].cout * convs[0].cin}
                                           if PROFILE is not None else None):
        rc = _lib.load().sgv3d_deform_conv3x3_forward(B, H, W, C, g, opg, x.data_ptr(), offset.data_ptr(), int(offset.shape[-1]), ptrs,
                                                     convs[0].k_pad, convs[0].cout_pad, out.data_ptr(), int(out.shape[-1]), int(y_coff),
                                                     _st(x))
    _lib.check(rc, "sgv3d_deform_conv3x3_forward")
    return out


class PackedDeformBf16:
    """The weights of a DCNv1 3x3 layer ([cout, cin / groups, 3, 3] f32) rounded once to bf16 and packed in the MFMA-fragment order
    of csrc/dcn_fused_bf16.hip (sgv3d_deform_conv3x3_bf16_pack_weight), made once per compiled state."""

    def __init__(self, weight, groups, device=None):
        w = weight.detach()
        device = device or w.device
        w = w.to(device=device, dtype=torch.float32).contiguous()
        cout, cpg, kh, kw = (int(v) for v in w.shape)
        assert kh == 3 and kw == 3 and cout % int(groups) == 0
        self.groups, self.channels, self.opg = int(groups), cpg * int(groups), cout // int(groups)
        lib = _lib.load()
        nbytes = int(lib.sgv3d_deform_conv3x3_bf16_weight_bytes(self.channels, self.groups, self.opg))
        if nbytes == 0:
            raise _lib.SGV3DError(f"deform_conv3x3_bf16: shape not covered (channels={self.channels} groups={self.groups} "
                                  f"outputs per group={self.opg})")
        self.w = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=device)
        with torch.cuda.device(device):
            rc = lib.sgv3d_deform_conv3x3_bf16_pack_weight(w.data_ptr(), self.channels, self.groups, self.opg, self.w.data_ptr(), _st(w))
        _lib.check(rc, "sgv3d_deform_conv3x3_bf16_pack_weight")
        self._keep = w   # the pack kernel reads it asynchronously


def deform_conv3x3_bf16_covers(channels, groups, out_channels):
    """The shapes sgv3d_deform_conv3x3_forward_bf16 covers: at most 8 groups, channels per group a multiple of 32, outputs per
    group a multiple of 4 (whatever the compute mode: DCN.hip_compile packs the bf16 weights of every covered layer)."""
    C, g, cout = int(channels), int(groups), int(out_channels)
    return 0 < g <= 8 and C % g == 0 and (C // g) % 32 == 0 and cout % g == 0 and (cout // g) % 4 == 0


def deform_conv3x3_bf16_eligible(x, groups, out_channels):
    """bf16 compute mode with the one-launch form switched on (DCN_FUSED_BF16), NHWC input in bf16 or f32 and a covered shape
    (deform_conv3x3_bf16_covers).  SGV3D_DCN_FUSED=0 turns the launch off like the f32 one."""
    if not (DCN_FUSED and DCN_FUSED_BF16 and MFMA_BF16 and not MFMA_F32X3) or x.dim() != 4 or x.dtype not in (torch.bfloat16, torch.float32):
        return False
    return deform_conv3x3_bf16_covers(x.shape[-1], groups, out_channels)


def deform_conv3x3_bf16(x, offset, packed, out=None, y_coff=0, out_dtype=None):
    """DCNv1 forward (lss_fpn.py:190-198) in one launch on the bf16 matrix cores: x NHWC [B,H,W,C] bf16 or f32, offset f32
    [B,H,W,>=18], ``packed`` a PackedDeformBf16.  Writes out[..., y_coff : y_coff + groups * opg] (f32 or bf16; default: the dtype
    of x); the bf16 output is the f32 one rounded once."""
    B, H, W, C = (int(v) for v in x.shape)
    g, opg = packed.groups, packed.opg
    assert C == packed.channels and x.dtype in (torch.bfloat16, torch.float32)
    assert x.is_contiguous() and offset.is_contiguous() and offset.dtype == torch.float32 and int(offset.shape[-1]) >= 18
    assert tuple(offset.shape[:3]) == (B, H, W)
    if out is None:
        out = torch.empty(B, H, W, g * opg, dtype=out_dtype or x.dtype, device=x.device)
    assert out.is_contiguous() and out.dtype in (torch.bfloat16, torch.float32) and tuple(out.shape[:3]) == (B, H, W)
    assert out_dtype is None or out.dtype == out_dtype
    flops = 2.0 * B * H * W * g * opg * 9 * (C // g)
    nbytes = (float(B * H * W) * (C * x.element_size() + 18 * 4 + g * opg * out.element_size()) + 2.0 * g * opg * 9 * (C // g))
    # (no ``symbol`` extra: none of the bf16-mode launches records one, and bench.py then lets the dominant LABEL stand for its
    #  kernel -- a single symbol here would make this launch the "dominant kernel" of every --dtype bf16 roofline pass.  The label
    #  is one instantiation family, dcn3x3_fused_bf16_kernel, priced with these flops against the bf16 peak.)
    with torch.cuda.device(x.device), prof("conv_dcn_fused_bf16", flops, nbytes):
        rc = _lib.load().sgv3d_deform_conv3x3_forward_bf16(B, H, W, C, g, opg, x.data_ptr(), int(x.dtype == torch.bfloat16),
                                                          offset.data_ptr(), int(offset.shape[-1]), packed.w.data_ptr(),
                                                          out.data_ptr(), int(out.dtype == torch.bfloat16), int(out.shape[-1]),
                                                          int(y_coff), _st(x))
    _lib.check(rc, "sgv3d_deform_conv3x3_forward_bf16")
    return out


def deform_im2col3x3(x, offset, groups, out=None):
    """x NHWC [B,H,W,C], offset NHWC [B,H,W,>=18] -> col [B,H,W,groups*9*(C/groups)]."""
    B, H, W, C = (int(s) for s in x.shape)
    if out is None:
        out = torch.empty(B, H, W, 9 * C, dtype=x.dtype, device=x.device)
    assert offset.dtype == torch.float32 and out.dtype == x.dtype
    lib = _lib.load()
    fn = lib.sgv3d_deform_im2col3x3_bf16 if x.dtype == torch.bfloat16 else lib.sgv3d_deform_im2col3x3
    with torch.cuda.device(x.device), prof("deform_im2col3x3"):
        rc = fn(B, H, W, C, int(groups), x.data_ptr(), offset.data_ptr(), int(offset.shape[-1]), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_deform_im2col3x3")
    return out


HEAD_FINAL_MAX_OUT = 4          # kHfMaxOut of csrc/misc_layers.hip: the outputs one branch of head_final_conv may have


def head_branch_of_out(widths, device=None):
    """The ``branch_of_out`` map of head_final_conv, int32 [sum(widths)], from the host list of outputs per branch.  Built
    here it is ascending with each branch's outputs contiguous, which the kernel assumes; a branch wider than
    HEAD_FINAL_MAX_OUT, whose extra planes the kernel would leave unwritten, is refused here, on the host, where the
    widths are known (the kernel's own copy of the map lives on the device and is not read back on the frame path)."""
    widths = [int(c) for c in widths]
    if any(c < 0 or c > HEAD_FINAL_MAX_OUT for c in widths) or sum(widths) == 0:
        raise ValueError(f"head_final_conv: a branch has 0..{HEAD_FINAL_MAX_OUT} outputs and the head at least one, got {widths}")
    return torch.tensor([i for i, c in enumerate(widths) for _ in range(c)], dtype=torch.int32, device=device)


def head_final_conv(hidden, weight, bias, branch_of_out, num_branches, hidden_ch, out=None):
    """hidden [nb, B, H, W, hc] (one NHWC map per branch); weight [sum_c,3,3,hc]; -> NCHW [B,sum_c,H,W].
    ``branch_of_out`` int32 [sum_c] on the device: build it with head_branch_of_out.  The kernel writes the first
    HEAD_FINAL_MAX_OUT outputs of a branch and takes them to be contiguous from the branch's first one; the map is not
    read back here (no device-to-host sync on the frame path), so a map from elsewhere is the caller's to get right."""
    nb, B, H, W, hc = (int(s) for s in hidden.shape)
    assert nb == num_branches and hc == hidden_ch and _dense_layout(hidden)
    total = int(weight.shape[0])
    assert _dense_layout(weight) and tuple(weight.shape) == (total, 3, 3, hc)
    assert _dense_layout(bias) and bias.numel() == total
    assert _dense_layout(branch_of_out, torch.int32) and branch_of_out.numel() == total
    if out is None:
        out = torch.empty(B, total, H, W, dtype=torch.float32, device=hidden.device)
    assert _dense_layout(out) and out.numel() == B * total * H * W
    with torch.cuda.device(hidden.device), prof("head_final_conv", 2.0 * B * H * W * total * 9 * hidden_ch):
        rc = _lib.load().sgv3d_head_final_conv(B, H, W, int(num_branches), int(hidden_ch), total,
                                              hidden.data_ptr(), weight.data_ptr(), bias.data_ptr(),
                                              branch_of_out.data_ptr(), out.data_ptr(), _st(hidden))
    _lib.check(rc, "sgv3d_head_final_conv")
    return out


def centerhead_branches(x, first, w2, b2, out_begin, num_branches, out=None):
    """Both layers of all CenterHead branches in one kernel (hidden maps never leave the chip).
    x NHWC [B,H,W,ld]; first: PackedConv of the concatenated first layers (needs Winograd weights, hidden 64);
    w2 [sum_c,3,3,64]; b2 [sum_c]; out_begin int32 [nb+1] (device).  -> NCHW [B,sum_c,H,W]."""
    B, H, W, ld = (int(s) for s in x.shape)
    assert x.is_contiguous() and first.wino_ok and first.cout == num_branches * 64
    total = int(w2.shape[0])
    if out is None:
        out = torch.empty(B, total, H, W, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    nws = lib.sgv3d_centerhead_branches_workspace_bytes(B, H, W, total)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    flops = 2.0 * B * H * W * (first.cout * first.cin * 9 + total * 9 * 64)
    with torch.cuda.device(x.device), prof("conv_wino_head", flops):
        rc = lib.sgv3d_centerhead_branches_forward(B, H, W, first.cin, ld, 0, x.data_ptr(), int(num_branches),
                                                   first.w_wino.data_ptr(), _lib.ptr(first.scale), _lib.ptr(first.shift),
                                                   total, w2.data_ptr(), b2.data_ptr(), out_begin.data_ptr(), out.data_ptr(),
                                                   ws.data_ptr(), nws, _st(x))
    _lib.check(rc, "sgv3d_centerhead_branches_forward")
    return out


def pack_centerhead_f4(w1):
    """First layers of the CenterHead branches concatenated, f32 OIHW [nb*64, 64, 3, 3] (device) -> the F(4x4) fragment
    stream of sgv3d_centerhead_branches_forward_f4 (csrc/head_wino4.hip)."""
    assert w1.is_cuda and w1.dtype == torch.float32 and tuple(w1.shape[1:]) == (64, 3, 3) and int(w1.shape[0]) % 64 == 0
    nb = int(w1.shape[0]) // 64
    lib = _lib.load()
    w1 = w1.contiguous()
    u = torch.empty(int(lib.sgv3d_centerhead_f4_weight_floats(nb)), dtype=torch.float32, device=w1.device)
    with torch.cuda.device(w1.device):
        _lib.check(lib.sgv3d_centerhead_f4_pack_weight(w1.data_ptr(), nb, u.data_ptr(), _st(w1)), "sgv3d_centerhead_f4_pack_weight")
    return u


def centerhead_branches_f4(x, u, scale1, shift1, w2, b2, out_begin, num_branches, out=None):
    """``centerhead_branches`` with the first layers in Winograd F(4x4) form: x NHWC f32 [B,H,W,ld] (channels [0, 64)),
    ``u`` from ``pack_centerhead_f4``, scale1 / shift1 the folded BN of the first layers [nb*64].  -> NCHW [B,sum_c,H,W]."""
    B, H, W, ld = (int(s) for s in x.shape)
    assert x.is_contiguous() and x.dtype == torch.float32
    total = int(w2.shape[0])
    if out is None:
        out = torch.empty(B, total, H, W, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    nws = lib.sgv3d_centerhead_branches_workspace_bytes(B, H, W, total)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    flops = 2.0 * B * H * W * (num_branches * 64 * 64 * 9 + total * 9 * 64)
    with torch.cuda.device(x.device), prof("conv_head_wino4", flops):
        rc = lib.sgv3d_centerhead_branches_forward_f4(B, H, W, 64, ld, 0, x.data_ptr(), int(num_branches), u.data_ptr(),
                                                      _lib.ptr(scale1), _lib.ptr(shift1), total, w2.data_ptr(), b2.data_ptr(),
                                                      out_begin.data_ptr(), out.data_ptr(), ws.data_ptr(), nws, _st(x))
    _lib.check(rc, "sgv3d_centerhead_branches_forward_f4")
    return out


HEAD_BF16_MAX_OUT = 4           # columns head_bf16_pack_w2_kernel keeps per branch (csrc/head_bf16.hip)
HEAD_BF16_MAX_BRANCHES = 48     # kMaxBranches of csrc/head_bf16.hip


def pack_centerhead_bf16(w1, w2, out_begin):
    """First layers of the CenterHead branches concatenated, f32 [nb*64, 64, 3, 3], and final layers f32 [sum_c, 3, 3, 64]
    with ``out_begin`` int32 [nb+1] -> the two bf16 buffers sgv3d_centerhead_branches_forward_bf16 streams
    (fragment-ordered first layers; [branch][tap][4][64] final layers).
    The kernel computes at most HEAD_BF16_MAX_OUT = 4 outputs per branch and at most HEAD_BF16_MAX_BRANCHES = 48 branches.  The
    packer keeps columns 0..3 of a branch only and the kernel would store a copy of them into the planes of a wider one, and the
    C entry cannot see the table (device memory), so the table is read back and checked HERE, once per weight load:
    ``out_begin`` starts at 0, does not decrease, ends at sum_c, and no branch is wider than 4; else ValueError, before any
    launch.  (A zero-width branch is fine: it has first-layer weights and no outputs.)"""
    w1 = w1.detach().float().contiguous()
    w2 = w2.detach().float().contiguous()
    nb = int(w1.shape[0]) // 64
    assert int(w1.shape[0]) == nb * 64 and tuple(w1.shape[1:]) == (64, 3, 3), "bf16 fused head: 64 -> 64 3x3 first layers"
    assert tuple(w2.shape[1:]) == (3, 3, 64) and int(out_begin.numel()) == nb + 1 and out_begin.dtype == torch.int32
    ob = [int(v) for v in out_begin.tolist()]
    widths = [b - a for a, b in zip(ob, ob[1:])]
    if nb < 1 or nb > HEAD_BF16_MAX_BRANCHES:
        raise ValueError(f"bf16 fused head: 1..{HEAD_BF16_MAX_BRANCHES} branches, got {nb}")
    if ob[0] != 0 or ob[-1] != int(w2.shape[0]) or any(c < 0 for c in widths):
        raise ValueError(f"bf16 fused head: out_begin must start at 0, not decrease and end at {int(w2.shape[0])} (the rows of w2), got {ob}")
    if any(c > HEAD_BF16_MAX_OUT for c in widths):
        raise ValueError(f"bf16 fused head: a branch has at most {HEAD_BF16_MAX_OUT} outputs, got widths {widths}")
    lib = _lib.load()
    p1 = torch.empty(lib.sgv3d_centerhead_bf16_weight_bytes(nb), dtype=torch.uint8, device=w1.device)
    p2 = torch.empty(lib.sgv3d_centerhead_bf16_weight2_bytes(nb), dtype=torch.uint8, device=w1.device)
    with torch.cuda.device(w1.device):
        _lib.check(lib.sgv3d_centerhead_bf16_pack_weight(w1.data_ptr(), nb, 64, p1.data_ptr(), _st(w1)),
                   "sgv3d_centerhead_bf16_pack_weight")
        _lib.check(lib.sgv3d_centerhead_bf16_pack_weight2(w2.data_ptr(), out_begin.data_ptr(), nb, p2.data_ptr(), _st(w1)),
                   "sgv3d_centerhead_bf16_pack_weight2")
    p1._keep = (w1, w2)             # the pack kernels read them asynchronously
    return p1, p2


def centerhead_branches_bf16(x, packed, scale1, shift1, b2, out_begin, num_branches, out=None, x_coff=0):
    """bf16-MFMA version of ``centerhead_branches``: x NHWC f32 or bf16 [B,H,W,ld] (channels [x_coff, x_coff+64); ld and x_coff
    multiples of 4, of 8 for a bf16 x), ``packed`` from ``pack_centerhead_bf16``, scale1 / shift1 [nb*64] folded BN, b2 [sum_c]
    -> NCHW f32 [B,sum_c,H,W].  At most HEAD_BF16_MAX_BRANCHES = 48 branches (refused by the C entry) of at most
    HEAD_BF16_MAX_OUT = 4 outputs each: ``out_begin`` is the table ``pack_centerhead_bf16`` checked -- it is not read back here
    (no device-to-host sync on the frame path), so pass the same one."""
    B, H, W, ld = (int(s) for s in x.shape)
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)
    total = int(b2.shape[0])
    if out is None:
        out = torch.empty(B, total, H, W, dtype=torch.float32, device=x.device)
    flops = 2.0 * B * H * W * (num_branches * 64 * 64 * 9 + total * 9 * 64)
    lib = _lib.load()
    fwd = lib.sgv3d_centerhead_branches_forward_bf16x if x.dtype == torch.bfloat16 else lib.sgv3d_centerhead_branches_forward_bf16
    with torch.cuda.device(x.device), prof("conv_head_bf16", flops):
        rc = fwd(
            B, H, W, 64, ld, int(x_coff), x.data_ptr(), int(num_branches), packed[0].data_ptr(), scale1.data_ptr(),
            shift1.data_ptr(), total, packed[1].data_ptr(), b2.data_ptr(), out_begin.data_ptr(), out.data_ptr(), _st(x))
    _lib.check(rc, "sgv3d_centerhead_branches_forward_bf16")
    return out


def lift(height_context, D, C, want_prob=False, want_lifted=True, lifted_dtype=None):
    """height_context NHWC [B,fH,fW,D+C] -> (prob [B,D,P] | None, lifted [B,D,P,C] | None).
    ``lifted_dtype=torch.bfloat16`` (bf16 compute mode, C % 4 == 0): the lifted tensor is written as bf16."""
    B, fH, fW, ld = (int(s) for s in height_context.shape)
    assert ld == D + C
    P = fH * fW
    lifted_dtype = lifted_dtype or torch.float32
    prob = torch.empty(B, D, P, dtype=torch.float32, device=height_context.device) if want_prob else None
    lifted = torch.empty(B, D, P, C, dtype=lifted_dtype, device=height_context.device) if want_lifted else None
    lib = _lib.load()
    fn = lib.sgv3d_lift_bf16 if (want_lifted and lifted_dtype == torch.bfloat16) else lib.sgv3d_lift
    with torch.cuda.device(height_context.device), prof("lift"):
        rc = fn(B, P, D, C, height_context.data_ptr(), _lib.ptr(prob), _lib.ptr(lifted), _st(height_context))
    _lib.check(rc, "sgv3d_lift")
    return prob, lifted
