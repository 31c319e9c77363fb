"""CPU: the host JPEG parser (sgv3d_jpeg_parse) against what Pillow reports, the files it must reject, the numpy
restatement of the decode (tests/jpeg_ref.py) against Pillow's output, a model of the kernels' subsequence-and-resolve
entropy decode against the sequential one, and argument checks that need no GPU.  The stress fixture
(tests/golden/jpeg_stress.npz): that it is as hostile as it is meant to be, the restatement and the parser on it, the
re-coder (tests/jpeg_recode.py) round trip, and the corrupt scans of the GPU containment test on the restatement's
machine first."""
import functools
import io
import os
import random
import re
import sys
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
import jpeg_recode as C
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


# ---------------------------------------------------------------------------------------------- the stress fixture
STRESS = np.load(os.path.join(GOLDEN, "jpeg_stress.npz"))
STRESS_NAMES = C.case_names(STRESS)
SMALL_ENTROPY = [n for n in STRESS_NAMES if n.startswith(('cc', 'rc_'))]   # 64x96 / 61x83 content and re-coded files
RECODED = [n for n in STRESS_NAMES if n.startswith('rc_') and not n.endswith('_src')]
CORRUPT_SOURCES = ('cc420_noise_q100_r1', 'rc_scene420_fill1')


@functools.lru_cache(maxsize=None)
def _decoded(name):
    """-> (info, coefficients, trace) of a stress file by the restatement's sequential decode"""
    info, trace = R.parse(STRESS[f'{name}_jpg'].tobytes()), []
    return info, R.coefficients(info, trace), trace


def test_stress_fixture_size_and_cases():
    assert os.path.getsize(os.path.join(GOLDEN, "jpeg_stress.npz")) <= 893272
    for samp in ('444', '422', '420'):
        for v in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49):
            assert f'sw{samp}_17x{v}' in STRESS_NAMES and f'sw{samp}_{v}x33' in STRESS_NAMES
    info = R.parse(STRESS['cc420_noise_q100_r0_jpg'].tobytes())
    assert all((q == 1).all() for q in info['qt'].values())          # quality 100 is the all-ones table


def test_stress_fixture_is_hostile():
    """The properties the stress files are there for, counted in what Pillow and the re-coder wrote with ``re`` on the
    scan bytes and with the restatement's sequential decode (never with the decoder under test)."""
    stuffed, before_marker, filled, odd_interval = [], [], [], []
    for n in STRESS_NAMES:
        info = R.parse(STRESS[f'{n}_jpg'].tobytes())
        scan = info['scan']
        if info['h'] <= 256 and info['w'] <= 256 and len(re.findall(b'\xff\x00', scan)) >= 100:
            stuffed.append(n)
        if len(re.findall(b'\xff\x00\xff+[\xd0-\xd7]', scan)) >= 3:   # (several per file: at different bit phases)
            before_marker.append(n)
        if re.search(b'\xff\xff[\xd0-\xd7]', scan):
            filled.append(n)
        if len(re.findall(b'\xff[\xd0-\xd7]', scan)) > 8 and info['mcux'] % info['restart']:
            odd_interval.append(n)
    assert len(stuffed) >= 3, stuffed
    assert len(before_marker) >= 3, before_marker
    assert len(filled) >= 2, filled
    assert odd_interval, "no file with more than 8 restart markers at an interval that does not divide the MCU row"
    _, coef, trace = _decoded('cc444_noise_q100_r3')
    assert (coef[:, 63] != 0).any(), "no block whose coefficient 63 is non-zero"
    assert any(cls == 1 and sym == 0xF0 for cls, _, sym in _decoded('cc420_zrl_r0')[2]), "no ZRL symbol"
    trace = _decoded('rc_scene420_long')[2]
    assert 2 * sum(ln > 9 for _, ln, _ in trace) > len(trace), "codes longer than 9 bits are not the common case"
    # a constant image: many DC codes in one 8-byte subsequence (the restatement's machine walks the true path)
    M = R._Machine(_decoded('cc420_const_r0')[0])
    st, per_sub = (0, 0, 0), {}
    while st[0] < M.bits:
        nxt, dc, _ = M.step(st)
        per_sub[st[0] >> 6] = per_sub.get(st[0] >> 6, 0) + int(dc)
        st = nxt
    assert max(per_sub.values()) >= 8, max(per_sub.values())
    info = _decoded('rc_noise_split')[0]
    (_, _, _, q1), (_, _, _, q2) = info['comps'][1:]
    assert info['tables'][1] != info['tables'][2] and q1 != q2 and not np.array_equal(info['qt'][q1], info['qt'][q2])
    for cls in (0, 1):
        assert info['dht'][(cls, info['tables'][1][cls])] != info['dht'][(cls, info['tables'][2][cls])]


@pytest.mark.parametrize("name", STRESS_NAMES)
def test_restatement_reproduces_stress_fixture(name):
    """Pillow's decode is the ground: the restatement equals it on every stress file."""
    kind, want = C.expected(STRESS, name)
    got = R.decode(STRESS[f'{name}_jpg'].tobytes())
    if kind == 'rgb':
        assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {(got != want).sum()} bytes differ"
    else:
        bad = np.nonzero(np.array([zlib.crc32(r.tobytes()) for r in got], np.uint32) != want)[0]
        assert got.shape[0] == want.shape[0] and bad.size == 0, f"{name}: rows {bad[:10].tolist()} differ"


@pytest.mark.parametrize("name", SMALL_ENTROPY)
def test_subsequence_model_on_stress_files(name):
    info, seq, _ = _decoded(name)
    for sb in (8, 9, 13):
        par, anchors = R.coefficients_parallel(info, sb)
        assert anchors[0] == 0 and np.array_equal(par, seq), (name, sb)


@pytest.mark.parametrize("name", RECODED)
def test_parser_on_recoded_files(name):
    """Table ids, restart interval, the scan and the derived tables agree with the restatement's parse."""
    from sgv3d_amd.jpeg import parse
    data = STRESS[f'{name}_jpg'].tobytes()
    rec, _ = parse(data)
    info = R.parse(data)
    assert (int(rec['height']), int(rec['width']), int(rec['hs']), int(rec['vs'])) == (info['h'], info['w'], info['hs'],
                                                                                      info['vs'])
    assert int(rec['restart']) == info['restart']
    off, ln = int(rec['scan_off']), int(rec['scan_len'])
    assert data[off:off + ln] == info['scan'] and data[off + ln:].lstrip(b'\xff') == b'\xd9'
    if name.endswith('_split'):
        assert info['tables'] == [(0, 0), (1, 1), (2, 2)]
    for c, (td, ta) in enumerate(info['tables']):
        assert list(rec['quant'][c]) == list(info['qt'][info['comps'][c][3]])
        for cls, tid in ((0, td), (1, ta)):
            t = rec['huff'][c][cls]
            look = np.zeros(512, np.int64)
            for (ln_, code), sym in R._codes(*info['dht'][(cls, tid)]).items():
                if ln_ <= 9:
                    look[code << (9 - ln_):(code + 1) << (9 - ln_)] = (ln_ << 8) | sym
                else:
                    assert code <= int(t['maxcode'][ln_]) and int(t['huffval'][code + int(t['valoff'][ln_])]) == sym
            assert np.array_equal(t['look'].astype(np.int64), look)
            bits = info['dht'][(cls, tid)][0]
            assert [int(v) for v in t['maxcode'][1:17]] == [
                max((code for (l, code) in R._codes(*info['dht'][(cls, tid)]) if l == ln_), default=-1)
                for ln_ in range(1, 17)], bits


def test_parser_rejects_undefined_and_all_ones_tables():
    from sgv3d_amd.jpeg import JpegError, parse
    data = STRESS['rc_scene420_each_jpg'].tobytes()
    rec, _ = parse(data)
    sos = int(rec['scan_off']) - 14
    assert data[sos:sos + 2] == b'\xff\xda'
    undefined = data[:sos + 8] + b'\x13' + data[sos + 9:]             # Cb: DC table 1, AC table 3 (never defined)
    with pytest.raises(JpegError, match='undefined Huffman table'):
        parse(undefined)
    ones = b'\xff\xc4' + (19 + 2).to_bytes(2, 'big') + b'\x00' + bytes([2] + [0] * 15) + b'\x00\x01'   # codes 0 and 1
    with pytest.raises(JpegError, match='bad Huffman table .code overflow at length 1'):
        parse(data[:sos] + ones + data[sos:])
    with pytest.raises(AssertionError, match='code overflow'):
        C.check_table([2] + [0] * 15, [0, 1])


@pytest.mark.parametrize("src", ['rc_noise_src', 'rc_const_src', 'rc_scene420_src', 'rc_scene444_src',
                                 'cc422_noise_q3_r3', 'sw420_17x9'])
def test_recoder_round_trip(src):
    """recode(tables='same') at the source's own restart interval decodes (restatement) to the source's pixels, and
    leaves the coefficients and the quantisation tables alone whatever the knobs."""
    data = STRESS[f'{src}_jpg'].tobytes()
    again = C.recode(data)
    assert np.array_equal(R.decode(again), C.expected(STRESS, src)[1])
    a, b = R.parse(data), R.parse(C.recode(data, tables='split', restart=5, fill=2, segments='extra each'))
    assert np.array_equal(R.coefficients(a), R.coefficients(b)) and b['restart'] == 5
    assert [c[3] for c in a['comps']] == [c[3] for c in b['comps']]
    assert all(np.array_equal(a['qt'][k], b['qt'][k]) for k in a['qt'])


@pytest.mark.parametrize("src", CORRUPT_SOURCES)
def test_corrupt_scans_are_contained_by_the_model(src):
    """The corrupt scans the GPU containment test uses, on the restatement's machine first: the headers still parse,
    every walk terminates and every coefficient index stays in range; the valid file itself reports no error."""
    from sgv3d_amd.jpeg import parse
    data = STRESS[f'{src}_jpg'].tobytes()
    assert C.model_status(data) == 0
    for what, bad in C.corruptions(data).items():
        rec, _ = parse(bad)
        assert int(rec['scan_len']) == len(R.parse(data)['scan']), what
        for sb in (8, 64):
            assert C.model_status(bad, sb) >= 0, what
