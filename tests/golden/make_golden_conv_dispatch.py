"""Recorder of the convolution dispatch (``sgv3d_amd.hip_ops.PackedConv``): which kernels a layer may run with, which one the
fixed rule picks, what a launch with a given (tile, split-K) hands to the C ABI and what it reports to the profiler.  No GPU: the
layers live on ``device='cpu'`` and ``_lib.load()`` is replaced by a stand-in that forwards only ``sgv3d_conv_pack_geometry`` (host
arithmetic) to the real library and otherwise writes down the call -- its name, every integer argument, "p" or "-" for a pointer
argument (given or null), and ``tile`` / ``split_k`` / ``k_pad`` / ``cout_pad`` of the descriptor as passed.  Candidate lists are
written in their order as "tile tile ..:split,split,..;" with neighbours of equal splits on one entry.

    python tests/golden/make_golden_conv_dispatch.py        # rewrites tests/golden/conv_dispatch.json.gz

``tests/test_conv_dispatch_cpu.py`` runs ``record()`` again and wants the same, entry by entry.  Cases:
  * every convolution signature of ``tune/gfx950_*.json`` under the switches it names, launched with the committed choice;
  * a sweep that launches every host tile id on a layer its family covers, in the layouts / modes the committed files do not
    have (NCHW output, group planes, gate, f32x3, channel offsets), under kill switches, and bound to a pack-cache entry;
  * per family a layer it does not cover: the exception and its message.
"""
import contextlib
import ctypes
import glob
import gzip
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json.gz")

# every switch of hip_ops the dispatch reads, at its documented default: the record does not depend on the SGV3D_* environment
DEFAULTS = dict(MFMA_BF16=False, MFMA_F32X3=False, WINOGRAD=True, WINO4=True, WINO4_G48=True, WINO4_X3=True, WINO_HALF=True, PW_X3=True,
                F4RES=True, OCC5=True, PATCH_BF16=True, DW_BF16=True, DW_DEEP=True, DW_NARROW=True, DW_DEEP_MAX_WGS=768, DW_SPLIT_K=True,
                SPLIT_K=True, MFIRST=True, ALIAS_1X1_WEIGHTS=True, PROFILE=None, PROFILE_DETAIL=False, BF16_ACTIVATIONS=True)
DESC_FIELDS = ("tile", "split_k", "k_pad", "cout_pad")
SIG = re.compile(r"^(\d+)x(\d+)k(\d+)x(\d+)s(\d+)p(\d+)d(\d+)ks(\d+)\|(\d+)x(\d+)x(\d+)\|m(\d)r(\d)g(\d)\|(\d+)\.(\d+)((?:\|\w+)*)\|ts\d+$")


class _StandIn:
    """What ``_lib.load()`` returns while recording."""

    def __init__(self, lib_mod, real):
        self._protos, self._real, self.calls = lib_mod._PROTOS, real, []

    def __getattr__(self, name):
        if name == "sgv3d_conv_pack_geometry":
            return getattr(self._real, name)
        if name not in self._protos:
            raise AttributeError(name)
        restype, argtypes = self._protos[name]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            rec = [name]
            for a, ty in zip(args, argtypes):
                obj = getattr(a, "_obj", None)
                if obj is not None and hasattr(obj, "cout_pad"):          # byref(ConvDesc)
                    rec.append({f: int(getattr(obj, f)) for f in DESC_FIELDS})
                elif ty in (ctypes.c_int, ctypes.c_size_t, ctypes.c_longlong):
                    rec.append(int(a))
                else:
                    rec.append("-" if a is None else "p")
            self.calls.append(rec)
            return 256 if restype is ctypes.c_size_t else 0 if restype is ctypes.c_int else None
        return call


class _NoEvent:
    def __init__(self, **kw):
        pass

    def record(self, *a):
        pass


class _FakeEntry:
    """A pack-cache entry (``PackedConv._entry``): writes down which forms register with it."""

    def __init__(self, param):
        self.param, self.registered = param, []

    def register(self, name, packed, getter):
        self.registered.append([name, list(packed.shape), str(packed.dtype)])


@contextlib.contextmanager
def _cpu_stage():
    """hip_ops on a host without a GPU: the library stand-in, no device contexts, streams or events; switches at their defaults.
    Everything is put back on exit."""
    import torch
    from sgv3d_amd import _lib, hip_ops
    real = _lib.load()
    stand_in = _StandIn(_lib, real)
    saved_lib = (_lib.load, _lib.stream_handle)
    saved_cuda = (torch.cuda.device, torch.cuda.Event)
    saved_sw = {k: getattr(hip_ops, k) for k in DEFAULTS}
    _lib.load, _lib.stream_handle = (lambda: stand_in), (lambda device=None: 0)
    torch.cuda.device, torch.cuda.Event = (lambda dev: contextlib.nullcontext()), _NoEvent
    try:
        yield hip_ops, stand_in
    finally:
        _lib.load, _lib.stream_handle = saved_lib
        torch.cuda.device, torch.cuda.Event = saved_cuda
        for k, v in saved_sw.items():
            setattr(hip_ops, k, v)


def _layer(cout, cin, k=1, stride=1, pad=0, dil=1, ks=0, B=1, H=32, W=32, **kw):
    """A case: the layer, the input size and (``kw``) how it is launched.  Keys of ``kw``: mode (0 NORMAL / 2 NCHW out / 3 group
    planes), res, gate, fixed (tile, split given to the constructor / the signature), bf16, f32x3, io, tile, split, sw (switch
    overrides), x_off / y_off (channel offsets into wider buffers), entry (bind to a pack-cache entry), detail (PROFILE_DETAIL)."""
    kh, kw_ = (k, k) if isinstance(k, int) else k
    return dict(dict(cout=cout, cin=cin, kh=kh, kw=kw_, stride=stride, pad=pad, dil=dil, ks=ks, B=B, H=H, W=W, mode=1 if ks else 0, res=0,
                     gate=0, fixed=(0, 0), bf16=False, f32x3=False, io=0, tile=1, split=1, sw={}, x_off=0, y_off=0, entry=False,
                     detail=False), **kw)


def _from_signature(sig, choice):
    m = SIG.match(sig)
    assert m, sig
    cout, cin, kh, kw, stride, pad, dil, ks, B, H, W, mode, res, gate, ft, fs = (int(v) for v in m.groups()[:16])
    tags = [t for t in m.group(17).split("|") if t]
    io = [int(t[2:]) for t in tags if t.startswith("io")]
    return _layer(cout, cin, (kh, kw), stride, pad, dil, ks, B, H, W, mode=mode, res=res, gate=gate, fixed=(ft, fs), bf16="bf16" in tags,
                  f32x3=True if "f32x3" in tags else "auto" if "x3auto" in tags else False, io=io[0] if io else 0,
                  tile=int(choice[0]), split=int(choice[1]))


def _cands_text(cands):
    groups = []
    for t, splits in cands:
        splits = ",".join(str(int(v)) for v in splits)
        if groups and groups[-1][1] == splits:
            groups[-1][0].append(int(t))
        else:
            groups.append(([int(t)], splits))
    return ";".join(" ".join(str(t) for t in ts) + ":" + splits for ts, splits in groups)


def run_case(hip_ops, stand_in, c):
    """One case -> {'cands', 'rule', 'calls', 'prof' | 'error'} (plain JSON values)."""
    import torch
    from sgv3d_amd import _lib
    for k, v in DEFAULTS.items():
        setattr(hip_ops, k, v)
    hip_ops.MFMA_BF16, hip_ops.MFMA_F32X3 = c["bf16"], c["f32x3"]
    for k, v in c["sw"].items():
        setattr(hip_ops, k, v)
    transposed = c["ks"] > 0
    shape = (c["cin"], c["cout"], c["ks"], c["ks"]) if transposed else (c["cout"], c["cin"], c["kh"], c["kw"])
    weight = torch.empty(shape, dtype=torch.float32)
    stand_in.calls.clear()
    conv = hip_ops.PackedConv(weight, stride=c["ks"] if transposed else c["stride"], pad=c["pad"], dil=c["dil"],
                              scale=torch.empty(c["cout"]), shift=torch.empty(c["cout"]), relu=True, transposed=transposed,
                              cin_pad=c["cin"], device="cpu", tile=c["fixed"][0])
    entry = None
    if c["entry"]:
        entry = conv._entry = _FakeEntry(weight)
    B, H, W, io, mode = c["B"], c["H"], c["W"], c["io"], c["mode"]
    oh, ow = conv.out_hw(H, W)
    x_ld, y_ld = c["cin"] + c["x_off"], c["cout"] + c["y_off"]
    act = lambda bf16, *s: torch.empty(s, dtype=torch.bfloat16 if bf16 else torch.float32)
    x = act(io & 1, B, H, W, x_ld)
    residual = act(io & 2, B, oh, ow, c["cout"]) if c["res"] else None
    gate = torch.empty(B, c["cin"]) if c["gate"] else None
    groups = 0
    if mode == 3:
        groups = 64 if c["cout"] % 64 == 0 else 4
    out = act(io & 2, B, oh, ow, y_ld) if c["y_off"] else None
    # the descriptor of this launch, for _candidates / _rule (what PackedConv builds before it chooses)
    d = _lib.ConvDesc()
    d.batch, d.in_h, d.in_w, d.cin, d.out_h, d.out_w, d.cout = B, H, W, conv.cin, oh, ow, conv.cout
    d.kh, d.kw, d.stride, d.pad, d.dil = conv.kh, conv.kw, conv.stride, conv.pad, conv.dil
    d.x_ld, d.x_coff, d.y_ld, d.y_coff = x_ld, c["x_off"], (conv.cout if groups else y_ld), (0 if groups else c["y_off"])
    d.res_ld, d.relu, d.mode, d.deconv_ks = (c["cout"] if c["res"] else 0), 1, mode, (groups if groups else conv.ks)
    d.k_pad, d.cout_pad, d.x_nchw, d.k_order = conv.k_pad, conv.cout_pad, 0, conv.k_order
    gemm_m = B * (H * W if transposed else oh * ow)
    gemm_n = conv.cout * (conv.ks * conv.ks if transposed else 1)
    ft, fs = c["fixed"]
    rec = {"cands": _cands_text(conv._candidates(d, gate, gemm_m, gemm_n, conv.k_pad // 32, ft, fs, io)),
           "rule": list(conv._rule(ft, fs, d, gemm_m, gemm_n, gate))}
    hip_ops.PROFILE, hip_ops.PROFILE_DETAIL = [], bool(c["detail"])
    try:
        conv(x, out, x_coff=c["x_off"], y_coff=c["y_off"], residual=residual, gate=gate, nchw_out=(mode == 2), group_planes=groups,
             tile=c["tile"], split_k=c["split"], out_dtype=torch.bfloat16 if io & 2 else None)
        rec["prof"] = [[p[0], p[1], p[4], p[5]] for p in hip_ops.PROFILE]
    except Exception as e:      # noqa: BLE001 -- the type and the message are the record
        rec["error"] = [type(e).__name__, str(e)]
    finally:
        hip_ops.PROFILE = None
    rec["calls"] = [list(r) for r in stand_in.calls]
    if entry is not None:
        rec["registered"] = entry.registered
    return rec


def committed_cases():
    cases = {}
    for f in sorted(glob.glob(os.path.join(ROOT, "tune", "gfx950_*.json"))):
        with open(f) as fh:
            db = json.load(fh)
        for sig, choice in sorted(db.items()):
            if sig.startswith(("centerhead_branches", "wgrad|", "pair|")):
                continue
            cases[os.path.basename(f)[len("gfx950_"):-len(".json")] + ":" + sig] = _from_signature(sig, choice)
    return cases


def sweep_cases():
    L = _layer
    cases = {}

    def add(name, case):
        assert name not in cases, name
        cases[name] = case
    c3 = dict(k=3, pad=1, B=2)                                     # a 3x3 / stride 1 / pad 1 layer
    # --- every host tile id on a layer its family covers
    for t in (1, 2, 3, 4, 21, 22, 23, 24, 44, 45, 5, 6, 8, 9, 10, 15, 46, 47) + tuple(range(50, 60)):
        add(f"f32 3x3 128->128 tile {t}", L(128, 128, **c3, tile=t, res=t % 2, detail=t in (21, 45)))
    for t in (11, 12, 13, 14):
        add(f"x3auto 3x3 128->128 tile {t}", L(128, 128, **c3, tile=t, f32x3="auto"))
        add(f"f32 1x1 256->64 tile {t}", L(64, 256, tile=t))
    for t in (1, 4):
        add(f"f32x3 3x3 128->128 tile {t}", L(128, 128, **c3, tile=t, f32x3=True, split=2))
    add("f32 3x3 64->128 tile 40", L(128, 64, **c3, tile=40))
    add("f32 3x3 128->64 tile 40", L(64, 128, **c3, tile=40, res=1))
    for t in (60, 61, 62, 64, 65, 66, 70, 71, 72, 74, 75, 76, 80, 81, 82, 90, 91, 92):
        add(f"f32 1x1 256->256 tile {t}", L(256, 256, B=2, tile=t, split=1 + t % 3))
    add("f32 3x3s2 128->256 tile 61", L(256, 128, k=3, stride=2, pad=1, tile=61))
    add("f32 7x7s2 4->64 tile 62", L(64, 4, k=7, stride=2, pad=3, H=64, W=64, tile=62))
    for t in (1, 2, 3, 4, 44):
        add(f"f32 1x1 256->256 tile {t}", L(256, 256, B=2, tile=t, detail=t == 44))
    add("f32 1x1 64->256 tile 3", L(256, 64, tile=3))              # pointwise, cin < 128
    add("f32 7x7s2 4->64 tile 2", L(64, 4, k=7, stride=2, pad=3, H=64, W=64, tile=2))       # tap-major
    add("f32 3x3 dil2 128->128 tile 9", L(128, 128, k=3, pad=2, dil=2, tile=9))
    add("f32 3x3 dil2 128->128 tile 52", L(128, 128, k=3, pad=2, dil=2, tile=52))
    add("f32 deconv2 128->64 tile 1", L(64, 128, ks=2, tile=1, split=2))
    add("bf16 3x3 64->64 tile 7", L(64, 64, **c3, bf16=True, tile=7, split=2))
    add("bf16 io3 3x3 64->64 tile 7", L(64, 64, **c3, bf16=True, io=3, tile=7, res=1))
    for t in (31, 32, 33, 34, 35, 36, 37, 38, 39):
        add(f"bf16 io3 1x1 256->256 tile {t}", L(256, 256, B=2, bf16=True, io=3, tile=t, res=t % 2))
    add("bf16 io3 3x3 256->256 tile 31 split 2", L(256, 256, **c3, bf16=True, io=3, tile=31, split=2))
    add("bf16 io3 deconv2 128->64 tile 32", L(64, 128, ks=2, bf16=True, io=3, tile=32))
    for io in (0, 1, 2, 3):
        add(f"bf16 io{io} 1x1 256->256 tile 1", L(256, 256, bf16=True, io=io, tile=1, split=2))
        add(f"bf16 io{io} 3x3 64->64 tile 24", L(64, 128, **c3, bf16=True, io=io, tile=24, detail=True))
    # --- layouts the committed files do not have
    add("f32 nchw 1x1 256->256 tile 21", L(256, 256, mode=2, tile=21))
    add("f32 nchw 3x3 128->128 tile 5", L(128, 128, **c3, mode=2, tile=5, split=2))
    add("f32 planes 3x3 64->2304 tile 9", L(2304, 64, **c3, mode=3, tile=9))
    add("f32 planes 3x3 64->2304 tile 1", L(2304, 64, **c3, mode=3, tile=1))
    add("f32 gate 3x3 128->128 tile 5", L(128, 128, **c3, gate=1, tile=5))
    add("f32 gate 1x1 256->256 tile 4", L(256, 256, gate=1, tile=4))
    add("f32 offsets 3x3 128->128 tile 9", L(128, 128, **c3, x_off=8, y_off=16, tile=9))
    add("f32 offsets 3x3 128->128 tile 4", L(128, 128, **c3, x_off=6, y_off=2, tile=4))     # F(4x4) not a candidate
    add("bf16 io3 offsets 1x1 256->256 tile 31", L(256, 256, bf16=True, io=3, x_off=8, y_off=8, tile=31))
    add("bf16 io3 offsets 1x1 256->256 tile 1", L(256, 256, bf16=True, io=3, x_off=4, y_off=4, tile=1))     # direct-weight not a candidate
    add("f32 fixed tile 3x3 128->128", L(128, 128, **c3, fixed=(5, 0), tile=5, split=1))
    add("f32 fixed split 3x3 128->128", L(128, 128, **c3, fixed=(0, 2), tile=1, split=2))
    add("bf16 io3 fixed split 3x3 256->256", L(256, 256, **c3, bf16=True, io=3, fixed=(0, 3), tile=31, split=3))
    add("bf16 fixed split 3x3 64->64", L(64, 64, **c3, bf16=True, fixed=(0, 3), tile=7, split=3))
    # --- the candidate lists and the rule at model sizes, and under the kill switches
    big = dict(k=3, pad=1, B=4, H=128, W=128)
    add("f32 3x3 256->256 128x128", L(256, 256, **big, tile=9))
    add("f32 3x3 64->256 128x128", L(256, 64, **big, tile=6))
    add("f32 3x3 96->96 16x16", L(96, 96, k=3, pad=1, H=16, W=16, tile=8, split=3))
    add("bf16 io3 3x3 256->256 128x128", L(256, 256, **big, bf16=True, io=3, tile=34))
    add("bf16 io3 3x3 512->512 16x16", L(512, 512, k=3, pad=1, H=16, W=16, bf16=True, io=3, tile=38, split=4))
    add("bf16 io3 3x3 128->128 16x16", L(128, 128, k=3, pad=1, H=16, W=16, bf16=True, io=3, tile=37))
    for sw in ("WINOGRAD", "WINO4", "WINO4_G48", "WINO4_X3", "WINO_HALF", "OCC5", "MFIRST", "SPLIT_K", "F4RES"):
        add(f"f32 3x3 256->256 128x128 {sw}=0", L(256, 256, **big, tile=1, sw={sw: False}))
    for sw in ("PW_X3", "OCC5", "MFIRST", "SPLIT_K", "ALIAS_1X1_WEIGHTS"):
        add(f"f32 1x1 256->256 {sw}=0", L(256, 256, B=2, tile=2, sw={sw: False}))
    for sw in ("PATCH_BF16", "DW_BF16", "DW_DEEP", "DW_NARROW", "DW_SPLIT_K", "SPLIT_K", "MFIRST"):
        add(f"bf16 io3 3x3 512->512 16x16 {sw}=0", L(512, 512, k=3, pad=1, H=16, W=16, bf16=True, io=3, tile=1, sw={sw: False}))
    add("bf16 io3 3x3 512->512 16x16 DW_DEEP_MAX_WGS=1", L(512, 512, k=3, pad=1, H=16, W=16, bf16=True, io=3, tile=1, sw={"DW_DEEP_MAX_WGS": 1}))
    add("x3auto 3x3 256->256 128x128", L(256, 256, **big, f32x3="auto", tile=11))
    add("f32x3 3x3 256->256 128x128", L(256, 256, **big, f32x3=True, tile=9))
    # --- bound to a pack-cache entry: permutations register, transformed forms refuse
    add("entry f32 3x3 128->128 tile 1", L(128, 128, **c3, tile=1, entry=True))
    add("entry f32 1x1 256->256 tile 1 (alias)", L(256, 256, tile=1, entry=True))
    add("entry f32 1x1 252->256 tile 1", L(256, 252, tile=1, entry=True))
    add("entry bf16 io3 1x1 256->256 tile 1", L(256, 256, bf16=True, io=3, tile=1, entry=True))
    add("entry bf16 io3 1x1 256->256 tile 31", L(256, 256, bf16=True, io=3, tile=31, entry=True))
    add("entry bf16 io3 deconv2 128->64 tile 32", L(64, 128, ks=2, bf16=True, io=3, tile=32, entry=True))
    add("entry bf16 3x3 64->64 tile 7", L(64, 64, **c3, bf16=True, tile=7, entry=True))
    add("entry f32 3x3 128->128 tile 5", L(128, 128, **c3, tile=5, entry=True))
    add("entry f32 3x3 128->128 tile 9", L(128, 128, **c3, tile=9, entry=True))
    add("entry f32 3x3 128->128 tile 50", L(128, 128, **c3, tile=50, entry=True))
    add("entry f32 3x3 64->128 tile 40", L(128, 64, **c3, tile=40, entry=True))
    add("entry f32 1x1 256->256 tile 60", L(256, 256, tile=60, entry=True))
    # --- per family, a layer (or launch) it does not cover
    add("refused igemm: bf16 tensors in f32 mode", L(256, 256, io=3, tile=1))
    add("refused igemm: tile 44 tap-major", L(64, 4, k=7, stride=2, pad=3, H=64, W=64, tile=44))
    add("refused igemm: tile 45 bf16 mode", L(256, 256, bf16=True, tile=45))
    add("refused igemm: unknown tile", L(256, 256, tile=99))
    add("refused wino: 1x1", L(256, 256, tile=5))
    add("refused wino: stride 2 tile 8", L(128, 128, k=3, stride=2, pad=1, tile=8))
    add("refused wino4: 1x1", L(256, 256, tile=9))
    add("refused wino4: split-K", L(128, 128, **c3, tile=10, split=2))
    add("refused wino4: bf16 mode tile 47", L(128, 128, **c3, bf16=True, tile=47))
    add("refused wino4_x3: 64 channels", L(64, 64, **c3, tile=50))
    add("refused wino4_x3: gate", L(128, 128, **c3, gate=1, tile=55))
    add("refused f4res: 128->128", L(128, 128, **c3, tile=40))
    add("refused f4res: split-K", L(128, 64, **c3, tile=40, split=2))
    add("refused pw_x3: 32 channels", L(64, 32, tile=60))
    add("refused pw_x3: deconv", L(64, 128, ks=2, tile=71))
    add("refused pw_x3: f32x3 mode", L(256, 256, f32x3=True, tile=82))
    add("refused patch_bf16: f32 mode", L(64, 64, **c3, tile=7))
    add("refused patch_bf16: 1x1", L(256, 256, bf16=True, io=3, tile=7))
    add("refused dw_bf16: f32 tensors", L(256, 256, bf16=True, tile=31))
    add("refused dw_bf16: deconv split-K", L(64, 128, ks=2, bf16=True, io=3, tile=32, split=2))
    add("refused dw_bf16: 20 channels", L(256, 20, bf16=True, io=3, tile=36))
    return cases


def record():
    """{case name: record}: the committed signatures, then the sweep."""
    out = {}
    with _cpu_stage() as (hip_ops, stand_in):
        for group in (committed_cases(), sweep_cases()):
            for name, case in group.items():
                out[name] = run_case(hip_ops, stand_in, case)
    return out


def dumps(rec):
    """The record as the golden file holds it: gzip (no timestamp) of JSON with one case per line."""
    lines = [json.dumps(name) + ":" + json.dumps(r, separators=(",", ":"), sort_keys=True) for name, r in rec.items()]
    return gzip.compress(("{\n" + ",\n".join(lines) + "\n}\n").encode(), 9, mtime=0)


def loads(data):
    return json.loads(gzip.decompress(data))


if __name__ == "__main__":
    got = record()
    with open(OUT, "wb") as f:
        f.write(dumps(got))
    print(f"{len(got)} cases, {sum('error' in r for r in got.values())} refused, {os.path.getsize(OUT)} bytes -> {OUT}")
