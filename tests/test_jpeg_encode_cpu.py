"""CPU: the JPEG encoder's C ABI, its header and its host entry (csrc/jpeg_encode.hip) and the numpy restatement
(tests/jpeg_encode_ref.py) against the files Pillow wrote for tests/golden/jpeg_encode.npz, byte for byte.  No GPU and no
Pillow: the fixture holds the inputs and the files."""
import ctypes
import os
import re

import numpy as np
import pytest

import jpeg_encode_ref as E
import jpeg_ref as R
from sgv3d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sgv3d_jpeg_encode_header", "sgv3d_jpeg_encode_workspace_bytes", "sgv3d_jpeg_encode", "sgv3d_jpeg_encode_host")


@pytest.fixture(scope="module")
def fx():
    return E.load_fixture()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def host_entry(lib, frames, quality, subsampling, restart, max_bytes=None, expect=0):
    """sgv3d_jpeg_encode_host on uint8 [n, h, w, 3] -> ([bytes or None], lengths, status); guard bytes around the files."""
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    hs, vs = E.SUBSAMPLING[subsampling]
    mb = h * w * 6 + 4096 if max_bytes is None else max_bytes
    slot = (mb + 15) // 16 * 16
    files, ln, st = np.full(n * slot, 0xA5, np.uint8), np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    rc = lib.sgv3d_jpeg_encode_host(n, h, w, quality, hs, vs, restart, mb, frames.ctypes.data, files.ctypes.data, files.size,
                                    ln.ctypes.data, st.ctypes.data)
    assert rc == expect, (rc, lib.sgv3d_last_error())
    out, o, written = [], 0, np.zeros(n * slot, bool)
    for i in range(n):
        out.append(files[o:o + ln[i]].tobytes() if ln[i] else None)
        written[o:o + ln[i]] = True
        o += (int(ln[i]) + 15) // 16 * 16
    assert (files[~written] == 0xA5).all(), "bytes outside the files were written"
    return out, ln, st


def test_header_declares_the_entries_with_the_ctypes_arity():
    text = open(os.path.join(ROOT, "include", "sgv3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == len(_lib._PROTOS[name][1]), name
    assert "#define SGV3D_JPEG_ENC_EOVERFLOW 1" in text and "#define SGV3D_JPEG_ENC_HEADER_MAX 640" in text


def test_every_rejection_without_a_gpu(lib):
    hdr, n = (ctypes.c_uint8 * 640)(), ctypes.c_int()
    H = lambda *a: lib.sgv3d_jpeg_encode_header(*a, ctypes.addressof(hdr), ctypes.byref(n), None)
    ok = (24, 40, 95, 2, 2, 0)
    assert H(*ok) == 0 and n.value == 623
    bad = {'quality 0': (24, 40, 0, 2, 2, 0), 'quality 101': (24, 40, 101, 2, 2, 0), 'sampling 1x2': (24, 40, 95, 1, 2, 0),
           'sampling 4x1': (24, 40, 95, 4, 1, 0), 'restart interval 65536': (24, 40, 95, 2, 2, 65536),
           'restart interval -1': (24, 40, 95, 2, 2, -1), 'size 0 x 40': (0, 40, 95, 2, 2, 0), 'size 24 x 65536': (24, 65536, 95, 2, 2, 0)}
    for word, args in bad.items():
        assert H(*args) == -1 and word.encode() in lib.sgv3d_last_error(), (word, lib.sgv3d_last_error())
        h, w, q, hs, vs, r = args
        if not word.startswith('quality'):
            assert lib.sgv3d_jpeg_encode_workspace_bytes(1, h, w, hs, vs, r, 4096) == 0, word
    assert lib.sgv3d_jpeg_encode_header(*ok, None, ctypes.byref(n), None) == -1 and b'null' in lib.sgv3d_last_error()
    assert lib.sgv3d_jpeg_encode_header(*ok, ctypes.addressof(hdr), None, None) == -1
    nws = lib.sgv3d_jpeg_encode_workspace_bytes(2, 24, 40, 2, 2, 0, 4096)
    assert nws > 2 * (12 * 128 + 4096) and nws % 16 == 0
    for frames, mb in ((0, 4096), (4097, 4096), (1, 0), (1, (1 << 26) + 1)):
        assert lib.sgv3d_jpeg_encode_workspace_bytes(frames, 24, 40, 2, 2, 0, mb) == 0
    # the device entry refuses everything before any launch: no GPU is touched here.  16 is a stand-in, never dereferenced
    src = np.zeros((2, 24, 40, 3), np.uint8)
    p = src.ctypes.data
    D = lambda *a, work=16, wb=nws, files=16, fb=2 * 4096, ln=16, st=16, s=p: lib.sgv3d_jpeg_encode(
        *a, s, work, wb, files, fb, ln, st, None)
    good = (2, 24, 40, 95, 2, 2, 0, 4096)
    for word, args in bad.items():
        h, w, q, hs, vs, r = args
        assert D(2, h, w, q, hs, vs, r, 4096) == -1 and word.encode() in lib.sgv3d_last_error(), word
    assert D(2, 24, 40, 95, 2, 2, 0, 0) == -1 and b'max_bytes' in lib.sgv3d_last_error()
    assert D(0, 24, 40, 95, 2, 2, 0, 4096) == -1 and b'frames' in lib.sgv3d_last_error()
    for kw in (dict(s=None), dict(files=None), dict(ln=None), dict(st=None), dict(work=None)):
        assert D(*good, **kw) == -1, kw
    assert D(*good, work=24) == -1 and b'aligned' in lib.sgv3d_last_error()
    assert D(*good, fb=2 * 4096 - 1) == -1 and b'files holds' in lib.sgv3d_last_error()
    assert D(*good, wb=nws - 1) == -3 and b'workspace' in lib.sgv3d_last_error()
    # the host entry checks the same
    ln, st, files = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2 * 4096, np.uint8)
    Hh = lambda *a, s=p, f=files.ctypes.data, fb=files.size, l=ln.ctypes.data, t=st.ctypes.data: lib.sgv3d_jpeg_encode_host(*a, s, f, fb, l, t)
    assert Hh(*good) == 0
    for word, args in bad.items():
        h, w, q, hs, vs, r = args
        assert Hh(2, h, w, q, hs, vs, r, 4096) == -1, word
    for kw in (dict(s=None), dict(f=None), dict(l=None), dict(t=None), dict(fb=100)):
        assert Hh(*good, **kw) == -1, kw
    assert Hh(2, 24, 40, 95, 2, 2, 0, 0) == -1


def test_python_layer_rejects_settings_before_anything_else():
    from sgv3d_amd.jpeg_encode import JpegEncodeError, JpegEncoder
    for kw in (dict(quality=0), dict(quality=101), dict(quality=74.5), dict(subsampling='4:1:1'), dict(subsampling=(2, 2)),
               dict(restart=65536), dict(restart=-1), dict(src_hw=(0, 8)), dict(src_hw=(8, 65536)), dict(max_bytes=0),
               dict(max_bytes=(1 << 26) + 1)):
        with pytest.raises(JpegEncodeError):
            JpegEncoder(**dict(dict(src_hw=(24, 40), device='cpu'), **kw))


def test_header_is_the_head_of_pillows_file_for_every_setting(fx):
    from sgv3d_amd.jpeg_encode import header
    for c in E.cases(fx):
        want = E.case_file(fx, c)
        hdr, quant = header(c['h'], c['w'], c['quality'], c['subsampling'], c['restart'])
        assert len(hdr) == (629 if c['restart'] else 623) and want[:len(hdr)] == hdr, c['name']
        hs, vs = E.SUBSAMPLING[c['subsampling']]
        assert E.header(c['h'], c['w'], c['quality'], hs, vs, c['restart']) == hdr, c['name']
        info = R.parse(want)
        assert np.array_equal(quant[0], info['qt'][0]) and np.array_equal(quant[1], info['qt'][1])
    for q in (1, 30, 50, 75, 95, 100):                            # the scaling rule at the qualities it was checked for
        _, quant = header(8, 8, q)
        assert np.array_equal(quant, np.stack(E.quant_tables(q)))
    assert header(8, 8, 1)[1].max() == 255 and header(8, 8, 100)[1].max() == 1


def test_restatement_and_host_entry_equal_pillow_on_every_case(fx, lib):
    bad = []
    for c in E.cases(fx):
        want, a = E.case_file(fx, c), E.case_input(fx, c)
        files, ln, st = host_entry(lib, a[None], c['quality'], c['subsampling'], c['restart'])
        if files[0] != want or ln[0] != len(want) or st[0] != 0:
            bad.append(('host', c['name']))
        if E.encode(a, c['quality'], c['subsampling'], c['restart']) != want:
            bad.append(('restatement', c['name']))
    assert not bad, bad


def test_restatements_coefficients_are_the_files(fx):
    """The quantised coefficients of the restatement, block by block, against the entropy decode of Pillow's file."""
    for name in ('24x40_noise_420_q75_r0', '24x48_smooth_420_q75_r0', '40x24_checker_420_q75_r0', '37x61_noise_422_q100_r0',
                 '9x7_noise_444_q75_r0', '17x33_smooth_420_q95_r1'):
        c = next(c for c in E.cases(fx) if c['name'] == name)
        hs, vs = E.SUBSAMPLING[c['subsampling']]
        want = R.coefficients(R.parse(E.case_file(fx, c)))
        got = E.coefficients(E.case_input(fx, c), c['quality'], hs, vs)
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_host_entry_batches_and_decodes_like_pillows_file(fx, lib):
    names = ['37x61_noise_420_q75_r0', '37x61_smooth_420_q75_r0', '37x61_checker_420_q75_r0', '37x61_zeros_420_q75_r0']
    cs = [next(c for c in E.cases(fx) if c['name'] == n) for n in names]
    want = [E.case_file(fx, c) for c in cs]
    files, ln, st = host_entry(lib, np.stack([E.case_input(fx, c) for c in cs]), 75, '4:2:0', 0)
    assert files == want and st.tolist() == [0] * 4 and len(set(ln.tolist())) == 4
    for name in ('41x65_noise_420_q75_r1', '37x61_noise_444_q100_r0', '24x40_smooth_422_q75_r0'):
        c = next(c for c in E.cases(fx) if c['name'] == name)
        got, _, _ = host_entry(lib, E.case_input(fx, c)[None], c['quality'], c['subsampling'], c['restart'])
        assert np.array_equal(R.decode(got[0]), R.decode(E.case_file(fx, c))), name


def test_overflow_is_flagged_one_byte_short_of_the_file(fx, lib):
    names = ['37x61_noise_420_q75_r0', '37x61_smooth_420_q75_r0', '37x61_checker_420_q75_r0']
    cs = [next(c for c in E.cases(fx) if c['name'] == n) for n in names]
    want = [E.case_file(fx, c) for c in cs]
    frames = np.stack([E.case_input(fx, c) for c in cs])
    files, ln, st = host_entry(lib, frames, 75, '4:2:0', 0, max_bytes=len(want[0]))
    assert files == want and st.tolist() == [0, 0, 0]
    files, ln, st = host_entry(lib, frames, 75, '4:2:0', 0, max_bytes=len(want[0]) - 1)
    assert st.tolist() == [1, 0, 0] and ln.tolist() == [0, len(want[1]), len(want[2])] and files == [None] + want[1:]
    # a file with stuffed bytes, one byte short: the unstuffed stream alone would still fit
    c = next(c for c in E.cases(fx) if c['name'] == '37x61_checker_444_q100_r0')
    w = E.case_file(fx, c)
    assert R.parse(w)['scan'].count(b'\xff\x00') > 0
    for mb, flag in ((len(w), 0), (len(w) - 1, 1)):
        files, ln, st = host_entry(lib, E.case_input(fx, c)[None], 100, '4:4:4', 0, max_bytes=mb)
        assert st.tolist() == [flag] and files == [None if flag else w]


def test_write_puts_the_encoded_bytes_on_disk_and_keeps_the_default_path(tmp_path, fx):
    from sgv3d_amd import recombine as RC
    c = next(c for c in E.cases(fx) if c['name'] == '24x40_noise_420_q75_r0')
    image, data = E.case_input(fx, c), E.case_file(fx, c)
    mask = np.zeros((24, 40), np.uint8)
    dest = dict(Tr_ego2cam=np.eye(4), P2=np.eye(3, 4))
    RC.write(str(tmp_path / 'a'), "000001", None, mask, dest, ["x"], encoded=data)
    assert (tmp_path / 'a' / 'training' / 'image_2' / '000001.jpg').read_bytes() == data
    assert (tmp_path / 'a' / 'training' / 'label_2' / '000001.txt').read_text() == "x\n"
    with pytest.raises(ValueError, match='JPEG'):
        RC.write(str(tmp_path / 'a'), "000002", None, mask, dest, [], encoded=b'not a file')
    # the default path is Pillow's default save, as before (quality 75, 4:2:0)
    RC.write(str(tmp_path / 'b'), "000001", image, mask, dest, ["x"])
    assert (tmp_path / 'b' / 'training' / 'image_2' / '000001.jpg').read_bytes() == data
    for sub in ('calib', 'denorm', 'label_2', 'mask_image'):
        fa, fb = sorted((tmp_path / 'a' / 'training' / sub).iterdir())[0], sorted((tmp_path / 'b' / 'training' / sub).iterdir())[0]
        assert fa.read_bytes() == fb.read_bytes(), sub
