"""CPU: the host JPEG parser (sgv3d_jpeg_parse) against what Pillow reports, the files it must reject, the numpy
restatement of the decode (tests/jpeg_ref.py) against Pillow's output, a model of the kernels' subsequence-and-resolve
entropy decode against the sequential one, and argument checks that need no GPU."""
import io
import os
import random
import sys

import numpy as np
import pytest

from conftest import GOLDEN
import jpeg_ref as R

sys.path.insert(0, GOLDEN)
from make_golden_jpeg import SMALL, encode, pil_decode, scene  # noqa: E402

PIL = pytest.importorskip("PIL.Image")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "jpeg.npz"))


def _bytes(d, name):
    return d[f'{name}_jpg'].tobytes()


@pytest.mark.parametrize("name", sorted(SMALL) + ['full_plain', 'full_rst'])
def test_parser_fields_match_pillow(fixture, name):
    from sgv3d_amd.jpeg import parse
    data = _bytes(fixture, name)
    rec, _ = parse(data)
    im = PIL.open(io.BytesIO(data))
    assert (int(rec['width']), int(rec['height'])) == im.size
    (_, h0, v0, q0), (_, h1, v1, q1), (_, h2, v2, q2) = im.layer
    assert (int(rec['hs']), int(rec['vs'])) == (h0, v0) and (h1, v1, h2, v2) == (1, 1, 1, 1)
    assert int(rec['mcux']) == -(-im.size[0] // (8 * h0)) and int(rec['mcuy']) == -(-im.size[1] // (8 * v0))
    assert int(rec['blocks_per_mcu']) == h0 * v0 + 2
    for c, q in enumerate((q0, q1, q2)):
        assert list(rec['quant'][c]) == list(im.quantization[q])
    # the segment ends in front of EOI, and starts after the SOS header
    assert data[int(rec['scan_off']) + int(rec['scan_len']):] == b'\xff\xd9'
    assert data[int(rec['scan_off']) - 14:int(rec['scan_off']) - 12] == b'\xff\xda'
    info = R.parse(data)
    assert int(rec['restart']) == info['restart']
    assert (int(rec['restart']) > 0) == (name in ('rst1', 'rst7', 'full_rst'))


def test_parser_huffman_tables_decode_like_the_restatement(fixture):
    """The derived tables: every code of the file's tables is found by the 9-bit lookup or by maxcode / valoff."""
    from sgv3d_amd.jpeg import parse
    for name in ('s420_61x83', 'optimize', 'q100'):
        data = _bytes(fixture, name)
        rec, _ = parse(data)
        info = R.parse(data)
        for c, (td, ta) in enumerate(info['tables']):
            for cls, tid in ((0, td), (1, ta)):
                t = rec['huff'][c][cls]
                for (ln, code), sym in R._codes(*info['dht'][(cls, tid)]).items():
                    if ln <= 9:
                        for low in range(1 << (9 - ln)):
                            assert int(t['look'][(code << (9 - ln)) | low]) == (ln << 8) | sym
                    else:
                        assert int(t['look'][code >> (ln - 9)]) == 0
                        assert code <= int(t['maxcode'][ln]) and int(t['huffval'][code + int(t['valoff'][ln])]) == sym


def _patched(data, find, offset, value):
    b = bytearray(data)
    b[b.index(find) + offset] = value
    return bytes(b)


REJECTS = {
    'progressive': 'progressive',
    'grayscale': '1 components',
    'cmyk': '4 components',
    'truncated': 'missing EOI',
    'arithmetic': 'arithmetic coding',
    '12bit': '12-bit samples',
}


@pytest.mark.parametrize("what", sorted(REJECTS))
def test_rejected_fixture_files(fixture, what):
    from sgv3d_amd.jpeg import JpegError, parse
    with pytest.raises(JpegError, match=REJECTS[what]):
        parse(fixture[f'bad_{what}'].tobytes())


def test_rejected_patched_headers(fixture):
    from sgv3d_amd.jpeg import JpegError, parse
    base = _bytes(fixture, 's420_61x83')
    sof = base.index(b'\xff\xc0')
    cases = {
        'RGB component ids': bytes(bytearray(base[:sof + 10]) + b'R' + base[sof + 11:sof + 13] + b'G'
                                   + base[sof + 14:sof + 16] + b'B' + base[sof + 17:]),
        'sampling factors': _patched(base, b'\xff\xc0', 11, 0x12),
        'more than one scan': _patched(base, b'\xff\xda', 4, 1),
        'missing SOS': base[:base.index(b'\xff\xda')],
        'lossless': _patched(base, b'\xff\xc0', 1, 0xC3),
        'hierarchical': _patched(base, b'\xff\xc0', 1, 0xC5),
        'not a JPEG': b'\x89PNG\r\n\x1a\n' + base[8:],
    }
    for msg, data in cases.items():
        with pytest.raises(JpegError, match=msg):
            parse(data)
    # an Adobe marker with transform 0 (RGB) in front of the frame header
    adobe = b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00'
    with pytest.raises(JpegError, match='Adobe transform 0'):
        parse(base[:2] + adobe + base[2:])
    parse(base[:2] + adobe[:-1] + b'\x01' + base[2:])   # transform 1 (YCbCr) is accepted


@pytest.mark.parametrize("name", sorted(SMALL))
def test_restatement_reproduces_fixture(fixture, name):
    got = R.decode(_bytes(fixture, name))
    want = fixture[f'{name}_rgb']
    assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {(got != want).sum()} bytes differ"


def test_restatement_matches_pillow_on_random_files():
    """Sizes 1..40 (narrow widths take libjpeg-turbo's plain replication), every sampling, qualities, restarts."""
    rng = random.Random(7)
    for t in range(40):
        h, w = rng.randint(1, 40), (1, 2, 3, 4, 5, 6)[t] if t < 6 else rng.randint(1, 40)
        kw = dict(quality=rng.choice([5, 30, 75, 95, 100]), subsampling=rng.choice([0, 1, 2]))
        if rng.random() < 0.3:
            kw['restart_marker_blocks'] = rng.randint(1, 5)
        if rng.random() < 0.3:
            kw['optimize'] = True
        data = encode(scene(h, w, 100 + t), **kw)
        assert np.array_equal(R.decode(data), pil_decode(data)), (h, w, kw)


@pytest.mark.parametrize("name", ['s420_61x83', 'rst1', 'rst7', 'optimize', 'q5', 's420_1x1', 's444_8x8'])
def test_subsequence_model_equals_sequential_decode(fixture, name):
    """The kernels' scheme (speculative decode from guessed states, continuation until synchronised, anchors, exclusive
    scan, final decode, DC prefix sums) gives the sequential decoder's coefficients at tiny subsequence lengths."""
    info = R.parse(_bytes(fixture, name))
    seq = R.coefficients(info)
    for sb in (8, 9, 13, 32, 1 << 20):
        par, anchors = R.coefficients_parallel(info, sb)
        assert anchors[0] == 0 and np.array_equal(par, seq), (name, sb)


def test_decoder_argument_errors(fixture):
    """Checked on the host before any launch (no GPU needed)."""
    from sgv3d_amd import _lib
    from sgv3d_amd.jpeg import JpegDecoder, JpegError
    with pytest.raises(ValueError, match='seq_bytes'):
        JpegDecoder((61, 83), device='cuda:0', seq_bytes=4)
    with pytest.raises(ValueError, match='max_bytes'):
        JpegDecoder((61, 83), max_bytes=0, device='cuda:0')
    with pytest.raises(ValueError, match='src_hw'):
        JpegDecoder((0, 83), device='cuda:0')
    dec = JpegDecoder((61, 83), max_bytes=1 << 16, device='cuda:0')
    a, b = _bytes(fixture, 's420_61x83'), _bytes(fixture, 's422_61x83')
    with pytest.raises(JpegError, match='differ in size'):
        dec.plan([a, _bytes(fixture, 's420_17x9')])
    with pytest.raises(JpegError, match='differ in sampling'):
        dec.plan([a, b])
    with pytest.raises(JpegError, match='capacity'):
        JpegDecoder((61, 83), max_bytes=256, device='cuda:0').plan([a])
    with pytest.raises(JpegError, match='frame 1: .*progressive'):
        JpegDecoder((32, 48), device='cuda:0').plan([encode(scene(32, 48, 1)), fixture['bad_progressive'].tobytes()])
    with pytest.raises(ValueError, match='lead'):
        dec.plan([a, a], lead=(1, 1, 3))
    with pytest.raises(ValueError, match='empty'):
        dec.plan([])
    with pytest.raises(TypeError):
        dec.plan(a)
    recs, _, lead = dec.plan([a, a], lead=(1, 2, 1))
    assert lead == (1, 2, 1) and len(recs) == 2
    lib = _lib.load()
    assert lib.sgv3d_jpeg_workspace_bytes(1, 61, 83, 1 << 16, 64) > 0
    for bad in ((0, 61, 83, 1 << 16, 64), (1, 0, 83, 1 << 16, 64), (1, 61, 83, 0, 64), (1, 61, 83, 1 << 16, 7)):
        assert lib.sgv3d_jpeg_workspace_bytes(*bad) == 0
