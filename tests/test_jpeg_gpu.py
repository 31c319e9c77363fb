"""GPU: the JPEG decode (csrc/jpeg.hip) byte for byte against Pillow's decode (tests/golden/jpeg.npz: small files whole,
1080x1920 files by row CRC32) at several subsequence lengths, mixed batches, repeatability, the decode fed into
ImagePreprocessor, graph capture with restaging, FramePipeline(decode=), a corrupt frame contained by its status word,
and argument errors raised before any launch.  The stress fixture (tests/golden/jpeg_stress.npz: edge sizes, noise,
constant and high-frequency content, re-coded Huffman tables, fill bytes, odd restart intervals, frames that cross the
kernels' chunk sizes): every file byte-exact at several subsequence lengths, mixed batches, reused buffers, and
structured corruptions contained by the status word."""
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import jpeg_recode as C
import preprocess_ref as P
from sgv3d_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMG_CONF = dict(img_mean=[123.675, 116.28, 103.53], img_std=[58.395, 57.12, 57.375], to_rgb=True)
SMALL = ('s420_61x83', 's422_61x83', 's444_61x83', 's420_17x9', 's422_17x9', 's444_8x8', 's420_1x1', 'rst1', 'rst7',
         'optimize', 'q100', 'q5')
SAME_420 = ('s420_61x83', 'rst1', 'optimize', 'q5')   # 61x83 4:2:0 files with different tables, qualities, restarts


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "jpeg.npz"))


def _dec(hw, **kw):
    from sgv3d_amd.jpeg import JpegDecoder
    return JpegDecoder(hw, device=DEV, **kw)


def _jpg(d, name):
    return d[f'{name}_jpg'].tobytes()


def _row_crc(rgb):
    return np.array([zlib.crc32(r.tobytes()) for r in rgb], np.uint32)


@pytest.mark.parametrize("name", SMALL)
def test_small_files_byte_exact(fixture, name):
    want = fixture[f'{name}_rgb']
    dec = _dec(want.shape[:2], max_bytes=1 << 16)
    got = dec([_jpg(fixture, name)])
    assert tuple(got.shape) == (1,) + want.shape
    assert np.array_equal(got[0].cpu().numpy(), want), f"{name}: {(got[0].cpu().numpy() != want).sum()} bytes differ"
    assert dec.status().tolist() == [0]


@pytest.mark.parametrize("seq_bytes", [8, 64, 1024])
def test_full_size_by_row_crc(fixture, seq_bytes):
    """Both 1080x1920 files in one batch, at the smallest subsequence length and two larger ones."""
    dec = _dec((1080, 1920))
    got = dec([_jpg(fixture, 'full_plain'), _jpg(fixture, 'full_rst')], seq_bytes=seq_bytes).cpu().numpy()
    for i, name in enumerate(('full_plain', 'full_rst')):
        bad = np.nonzero(_row_crc(got[i]) != fixture[f'{name}_crc'])[0]
        assert bad.size == 0, f"{name} seq_bytes={seq_bytes}: rows {bad[:10].tolist()} differ"
    assert dec.status().tolist() == [0, 0]


def test_subsequence_lengths_agree(fixture):
    files = [_jpg(fixture, n) for n in SAME_420]
    dec = _dec((61, 83), max_bytes=1 << 16)
    outs = [dec(files, seq_bytes=s).cpu() for s in (8, 9, 13, 64, 4096)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    for i, n in enumerate(SAME_420):
        assert np.array_equal(outs[0][i].numpy(), fixture[f'{n}_rgb'])


def test_mixed_batch_equals_single_and_repeats(fixture):
    files = [_jpg(fixture, n) for n in SAME_420]
    dec = _dec((61, 83), max_bytes=1 << 16)
    batch = dec(files, lead=(2, 1, 2)).cpu()
    assert tuple(batch.shape) == (2, 1, 2, 61, 83, 3)
    flat = batch.view(4, 61, 83, 3)
    for i, f in enumerate(files):
        assert torch.equal(flat[i], dec([f])[0].cpu())
    assert torch.equal(dec(files, lead=(2, 1, 2)).cpu(), batch)       # two runs: bitwise identical


def test_decode_then_preprocess(fixture):
    """Decode -> ImagePreprocessor equals preprocess_ref on the fixture's expected frame."""
    from sgv3d_amd.preprocess import ImagePreprocessor
    want_rgb = fixture['s420_61x83_rgb']
    pre = ImagePreprocessor({'final_dim': (40, 64), 'bot_pct_lim': (0.0, 0.0)}, IMG_CONF, src_hw=(61, 83), device=DEV)
    frames = _dec((61, 83), max_bytes=1 << 16)([_jpg(fixture, 's420_61x83')])
    imgs, _ = pre(frames)
    want = P.normalize(P.transform(want_rgb, pre.resize_dims, pre.crop, False), IMG_CONF['img_mean'], IMG_CONF['img_std'],
                       True)
    assert np.array_equal(imgs[0, 0, 0].cpu().numpy(), want)


def test_graph_capture_replays_newly_staged_files(fixture):
    from sgv3d_amd.jpeg import JpegStaging
    dec = _dec((61, 83), max_bytes=1 << 16)
    st = JpegStaging(dec, (2,))
    st.stage([_jpg(fixture, SAME_420[0]), _jpg(fixture, SAME_420[1])])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st.launch()                                    # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = st.launch()
    for pair in ((SAME_420[2], SAME_420[3]), (SAME_420[1], SAME_420[0])):
        st.stage([_jpg(fixture, n) for n in pair])     # (nothing queued reads the pinned buffer: synchronised below)
        g.replay()
        torch.cuda.synchronize()
        for i, n in enumerate(pair):
            assert np.array_equal(out[i].cpu().numpy(), fixture[f'{n}_rgb']), n
        assert st.status().tolist() == [0, 0]


def test_frame_pipeline_with_decode(fixture):
    """FramePipeline(decode=, preprocess=) fed encoded files == FramePipeline(preprocess=) fed their decoded frames."""
    from sgv3d_amd.models.bev_height import BEVHeight
    from sgv3d_amd.pipeline import FramePipeline
    from sgv3d_amd.preprocess import ImagePreprocessor
    bc, hc = S.small_conf(depth=18)
    torch.manual_seed(0)
    m = BEVHeight(bc, hc).eval()
    S.randomize_norm_stats_(m, 1)
    m = m.to(DEV)
    pre = ImagePreprocessor({'final_dim': bc['final_dim'], 'bot_pct_lim': (0.0, 0.0)}, IMG_CONF, src_hw=(61, 83),
                            device=DEV)
    mats = {k: v.to(DEV) for k, v in S.make_mats(1, scale=128 / 864).items()}
    names = (SAME_420[0], SAME_420[2], SAME_420[3])
    frames = [torch.from_numpy(fixture[f'{n}_rgb']).to(DEV).view(1, 1, 1, 61, 83, 3) for n in names]
    plain = FramePipeline(m, frames[0], mats, slots=2, preprocess=pre)
    want = [{k: v.clone() for k, v in plain.result(plain.submit(f, mats))[3][0].items()} for f in frames]
    del plain
    pipe = FramePipeline(m, [_jpg(fixture, names[0])], mats, slots=2, preprocess=pre,
                         decode=_dec((61, 83), max_bytes=1 << 16))
    assert pipe.use_graph
    got = [{k: v.clone() for k, v in pipe.result(pipe.submit([_jpg(fixture, n)], mats))[3][0].items()} for n in names]
    for g, w in zip(got, want):
        for k in w:
            assert torch.equal(g[k], w[k]), k


def test_corrupt_scan_is_reported_and_contained(fixture):
    """One frame with a valid header and random scan bytes: the batch completes, that frame's status is non-zero and
    the other frames are byte-exact."""
    from sgv3d_amd.jpeg import parse
    good = _jpg(fixture, 's420_61x83')
    rec, _ = parse(good)
    off, ln = int(rec['scan_off']), int(rec['scan_len'])
    rnd = np.random.default_rng(3).integers(0, 255, ln, dtype=np.uint8).tobytes()   # (no 0xFF: no markers)
    bad = good[:off] + rnd + good[off + ln:]
    for seq in (8, 64):
        dec = _dec((61, 83), max_bytes=1 << 16)
        out = dec([good, bad, _jpg(fixture, 'q5')], seq_bytes=seq).cpu().numpy()
        st = dec.status()
        assert st[0] == 0 and st[2] == 0 and st[1] != 0, st
        assert np.array_equal(out[0], fixture['s420_61x83_rgb']) and np.array_equal(out[2], fixture['q5_rgb'])


def test_errors_before_any_launch(fixture):
    from sgv3d_amd.jpeg import JpegError
    dec = _dec((61, 83), max_bytes=256)
    with pytest.raises(JpegError, match='capacity'):
        dec([_jpg(fixture, 's420_61x83')])
    dec = _dec((61, 83), max_bytes=1 << 16)
    with pytest.raises(JpegError, match='differ in size'):
        dec([_jpg(fixture, 's420_61x83'), _jpg(fixture, 's420_17x9')])
    with pytest.raises(JpegError, match='differ in sampling'):
        dec([_jpg(fixture, 's420_61x83'), _jpg(fixture, 's422_61x83')])
    with pytest.raises(JpegError, match='progressive'):
        _dec((32, 48))([fixture['bad_progressive'].tobytes()])
    with pytest.raises(ValueError, match='out must be'):
        dec([_jpg(fixture, 's420_61x83')], out=torch.empty(1, 61, 83, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match='seq_bytes'):
        dec([_jpg(fixture, 's420_61x83')], seq_bytes=4)
    with pytest.raises(RuntimeError, match='nothing decoded'):
        dec.status()


# ---------------------------------------------------------------------------------------------- the stress fixture
STRESS = np.load(os.path.join(GOLDEN, "jpeg_stress.npz"))
STRESS_NAMES = C.case_names(STRESS)
STRESS_SMALL = [n for n in STRESS_NAMES if not n.startswith('big_')]
STRESS_ENTROPY = [n for n in STRESS_NAMES if n.startswith(('cc', 'cx', 'rc_'))]   # content classes and re-coded files
MIXED_420 = ('cc420_noise_q100_r1', 'rc_noise_long', 'cc420_const_r3', 'rc_noise_split', 'rc_const_long',
             'cc420_zrl_r6', 'rc_noise_src', 'cc420_bw8_r0', 'rc_const_split', 'rc_noise_fill3', 'rc_noise_combo',
             'cc420_noise_q100_r0')
CORRUPT_SOURCES = ('cc420_noise_q100_r1', 'rc_scene420_fill1')


def _sjpg(name):
    return STRESS[f'{name}_jpg'].tobytes()


def _hw(name):
    kind, want = C.expected(STRESS, name)
    if kind == 'rgb':
        return want.shape[:2]
    from sgv3d_amd.jpeg import parse
    rec, _ = parse(_sjpg(name))
    return int(rec['height']), int(rec['width'])


def _assert_frame(got, name, what=''):
    """got: uint8 [h, w, 3] numpy == Pillow's decode of the case (whole, or by row CRC32)"""
    kind, want = C.expected(STRESS, name)
    if kind == 'crc':
        bad = np.nonzero(_row_crc(got) != want)[0]
        assert got.shape[0] == want.shape[0] and bad.size == 0, (f"{name} {what}: {bad.size} rows differ, first "
                                                                 f"{bad[:10].tolist()}")
        return
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = np.argwhere(got != want)
    assert diff.shape[0] == 0, (f"{name} {what}: {diff.shape[0]} bytes differ, first at (row, column, channel) "
                                f"{tuple(diff[0].tolist())}: {got[tuple(diff[0])]} != {want[tuple(diff[0])]}")


@pytest.mark.parametrize("name", STRESS_SMALL)
def test_stress_small_files_byte_exact(name):
    dec = _dec(_hw(name), max_bytes=1 << 17)
    got = dec([_sjpg(name)])
    _assert_frame(got[0].cpu().numpy(), name)
    assert dec.status().tolist() == [0]


@pytest.mark.parametrize("name", STRESS_ENTROPY)
def test_stress_subsequence_lengths_agree(name):
    """8, 9 and 13 bytes, the default, a long one, and one subsequence for the whole scan."""
    dec = _dec(_hw(name), max_bytes=1 << 17)
    outs = []
    for s in (8, 9, 13, 64, 1024, 1 << 17):
        outs.append(dec([_sjpg(name)], seq_bytes=s)[0].cpu())
        assert dec.status().tolist() == [0], (name, s)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    _assert_frame(outs[0].numpy(), name)


@pytest.mark.parametrize("order", [tuple(range(12)), (11, 3, 7, 0, 9, 1, 5, 10, 2, 8, 4, 6)])
def test_stress_mixed_batches(order):
    """64x96 4:2:0 files with different restart intervals, table sets (same, long, split), fill bytes and content in
    one batch: every frame equals its single-file decode and the fixture; a second run is bitwise equal."""
    names = [MIXED_420[i] for i in order]
    files = [_sjpg(n) for n in names]
    dec = _dec((64, 96), max_bytes=1 << 15)
    batch = dec(files, lead=(2, 3, 2)).cpu()
    assert dec.status().tolist() == [0] * 12
    flat = batch.view(12, 64, 96, 3)
    for i, n in enumerate(names):
        assert torch.equal(flat[i], dec([files[i]])[0].cpu()), n
        _assert_frame(flat[i].numpy(), n, 'in a mixed batch')
    assert torch.equal(dec(files, lead=(2, 3, 2)).cpu(), batch)


@pytest.mark.parametrize("seq_bytes", [8, 64])
def test_stress_chunk_crossers_by_row_crc(seq_bytes):
    """1024x1040 4:2:0: 16640 luma blocks (more than one chunk of the DC scan), 65 MCUs per row at restart interval 7
    (more than eight intervals, none ends a row), with the file's tables and with long codes."""
    names = ('big_1024x1040_r7', 'big_1024x1040_r7_long')
    dec = _dec((1024, 1040), max_bytes=1 << 17)
    got = dec([_sjpg(n) for n in names], seq_bytes=seq_bytes).cpu().numpy()
    for i, n in enumerate(names):
        _assert_frame(got[i], n, f'seq_bytes={seq_bytes}')
    assert dec.status().tolist() == [0, 0]


def test_stress_large_frame_by_row_crc():
    dec = _dec((2176, 3840))
    got = dec([_sjpg('big_2176x3840')]).cpu().numpy()
    _assert_frame(got[0], 'big_2176x3840')
    assert dec.status().tolist() == [0]


def test_stress_reused_buffers_do_not_leak():
    """A long noise scan, then a constant-colour scan of a few hundred bytes, then noise again through one decoder
    and one set of persistent buffers: stale exits / sync / base entries of the longer scan must not reach the
    short one."""
    from sgv3d_amd.jpeg import JpegStaging
    names = ('cc420_noise_q100_r0', 'cc420_const_r0', 'cc420_noise_q100_r1', 'rc_const_long', 'rc_noise_edge9')
    dec = _dec((64, 96), max_bytes=1 << 15, seq_bytes=8)
    st = JpegStaging(dec, (1,))
    for n in names:
        _assert_frame(dec([_sjpg(n)])[0].cpu().numpy(), n, 'through a reused decoder')
        assert dec.status().tolist() == [0]
        st.stage([_sjpg(n)])
        out = st.launch()
        torch.cuda.synchronize()
        _assert_frame(out[0].cpu().numpy(), n, 'through reused buffers')
        assert st.status().tolist() == [0]


@pytest.mark.parametrize("src", CORRUPT_SOURCES)
def test_stress_corruptions_are_reported_and_contained(src):
    """One flipped bit, a zeroed last quarter and an overwritten restart marker (each first run on the restatement's
    machine by tests/test_jpeg_cpu.py): the batch completes, the good frames around the corrupt one are byte-exact and
    the corrupt frame's status is non-zero wherever the model reports an error."""
    good = _sjpg(src)
    other = 'cc420_zrl_r1' if src.startswith('cc') else 'rc_scene420_split'
    hw = _hw(src)
    for what, bad in C.corruptions(good).items():
        for seq in (8, 64):
            model = C.model_status(bad, seq)
            dec = _dec(hw, max_bytes=1 << 15)
            out = dec([good, bad, _sjpg(other)], seq_bytes=seq).cpu().numpy()
            st = dec.status()
            assert st[0] == 0 and st[2] == 0, (what, seq, st)
            assert model == 0 or st[1] != 0, (what, seq, st, model)
            _assert_frame(out[0], src, f'next to {what}')
            _assert_frame(out[2], other, f'next to {what}')
