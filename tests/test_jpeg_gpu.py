"""GPU: the JPEG decode (csrc/jpeg.hip) byte for byte against Pillow's decode (tests/golden/jpeg.npz: small files whole,
1080x1920 files by row CRC32) at several subsequence lengths, mixed batches, repeatability, the decode fed into
ImagePreprocessor, graph capture with restaging, FramePipeline(decode=), a corrupt frame contained by its status word,
and argument errors raised before any launch."""
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN
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
