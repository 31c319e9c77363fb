"""GPU: on-device JPEG encoding (csrc/jpeg_encode.hip, sgv3d_amd/jpeg_encode.py) against the files Pillow wrote for
tests/golden/jpeg_encode.npz, byte for byte, against the host entry that runs the kernels' functions, and against the
call's contract: guard bands, a dirty workspace, overflow, a short workspace, launch and copy counts, graph capture.
Fixtures only: Pillow is not imported here."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_encode_ref as E
import jpeg_ref as R
from sgv3d_amd import _lib, hip_ops
from sgv3d_amd.jpeg_encode import EOVERFLOW, SUBSAMPLING, JpegEncodeError, JpegEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256                                          # bytes of 0xA5 around every region the call writes


@pytest.fixture(scope="module")
def fx():
    return E.load_fixture()


def _enc(c, **kw):
    kw.setdefault('max_bytes', c['h'] * c['w'] * 6 + 4096)
    return JpegEncoder(src_hw=(c['h'], c['w']), quality=c['quality'], subsampling=c['subsampling'], restart=c['restart'],
                       device=DEV, **kw)


def _case(fx, name):
    return next(c for c in E.cases(fx) if c['name'] == name)


def host_entry(frames, quality, subsampling, restart, max_bytes):
    """sgv3d_jpeg_encode_host on a uint8 [n, h, w, 3] array -> ([bytes or None], status)"""
    lib = _lib.load()
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    hs, vs = SUBSAMPLING[subsampling]
    slot = (max_bytes + 15) // 16 * 16
    files, ln, st = np.zeros(n * slot, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = lib.sgv3d_jpeg_encode_host(n, h, w, quality, hs, vs, restart, max_bytes, frames.ctypes.data, files.ctypes.data, files.size,
                                    ln.ctypes.data, st.ctypes.data)
    assert rc == 0, lib.sgv3d_last_error()
    out, o = [], 0
    for i in range(n):
        out.append(files[o:o + ln[i]].tobytes() if ln[i] else None)
        o += (int(ln[i]) + 15) // 16 * 16
    return out, st


def test_every_fixture_case_byte_for_byte(fx):
    """One encoder per case (107 small calls); the results are fetched after all of them were enqueued."""
    pending = []
    for c in E.cases(fx):
        frame = torch.from_numpy(E.case_input(fx, c)).to(DEV)
        pending.append((c, _enc(c)(frame[None])))
    bad = []
    for c, res in pending:
        got = res.files()[0]
        want = E.case_file(fx, c)
        assert res.status().tolist() == [0] and res.lengths().tolist() == [len(want)], c['name']
        if got != want:
            bad.append(c['name'])
    assert not bad, bad


def _guarded_call(enc, frames, fill_work=None, short=0, max_bytes=None):
    """sgv3d_jpeg_encode with guard bands around files, lengths, status and the workspace -> (rc, files region, lengths,
    status); asserts that the guard bands and the unused tail of the files region are untouched."""
    lib = _lib.load()
    n = frames.shape[0]
    H, W = enc.src_hw
    mb = enc.max_bytes if max_bytes is None else max_bytes
    nws = int(lib.sgv3d_jpeg_encode_workspace_bytes(n, H, W, enc.hs, enc.vs, enc.restart, mb))
    assert nws > 0 and nws % 16 == 0
    slot = (mb + 15) // 16 * 16
    sizes = [n * slot, 4 * n, 4 * n, nws]
    offs, total = [], GUARD
    for s in sizes:
        offs.append(total)
        total += (s + 15) // 16 * 16 + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    if fill_work is not None:
        buf[offs[3]:offs[3] + nws] = fill_work
    p = buf.data_ptr()
    assert p % 16 == 0
    rc = lib.sgv3d_jpeg_encode(n, H, W, enc.quality, enc.hs, enc.vs, enc.restart, mb, frames.data_ptr(), p + offs[3], nws - short,
                               p + offs[0], n * slot, p + offs[1], p + offs[2], _lib.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    used = np.zeros(total, bool)
    for o, s in zip(offs, sizes):
        used[o:o + s] = True
    assert (raw[~used] == 0xA5).all(), "a guard band was written"
    if rc != 0:
        assert (raw == 0xA5).all(), "a refused call wrote something"
        return rc, None, None, None
    ln = raw[offs[1]:offs[1] + 4 * n].view(np.int32).copy()
    st = raw[offs[2]:offs[2] + 4 * n].view(np.int32).copy()
    region = raw[offs[0]:offs[0] + n * slot]
    written = np.zeros(n * slot, bool)
    files, o = [], 0
    for i in range(n):
        files.append(region[o:o + ln[i]].tobytes() if ln[i] else None)
        written[o:o + ln[i]] = True
        o += (int(ln[i]) + 15) // 16 * 16
    assert (region[~written] == 0xA5).all(), "bytes outside the files were written"
    return rc, files, ln, st


BATCH = ['37x61_noise_420_q75_r0', '37x61_smooth_420_q75_r0', '37x61_checker_420_q75_r0', '37x61_zeros_420_q75_r0']


def test_batch_of_four_contents_guard_bands_and_dirty_workspace(fx):
    cs = [_case(fx, n) for n in BATCH]
    want = [E.case_file(fx, c) for c in cs]
    assert len(set(len(w) for w in want)) == 4                    # the lengths differ inside one call
    frames = torch.from_numpy(np.stack([E.case_input(fx, c) for c in cs])).to(DEV)
    enc = _enc(cs[0])
    rc, files, ln, st = _guarded_call(enc, frames)
    assert rc == 0 and files == want and ln.tolist() == [len(w) for w in want] and st.tolist() == [0] * 4
    # a workspace full of 0xFF: the call clears what it ORs into
    rc, again, ln2, st2 = _guarded_call(enc, frames, fill_work=0xFF)
    assert rc == 0 and again == want and ln2.tolist() == ln.tolist() and st2.tolist() == [0] * 4
    # the Python layer: the same files, any lead shape
    res = enc(frames.reshape(2, 2, 37, 61, 3))
    assert res.files() == want and res.lead == (2, 2)


def test_multi_chunk_stream_with_restart_markers_in_a_dirty_workspace(fx):
    c = _case(fx, '130x260_noise_422_q75_r17')
    frames = torch.from_numpy(E.case_input(fx, c)[None]).to(DEV)
    rc, files, _, st = _guarded_call(_enc(c), frames, fill_work=0xFF)
    assert rc == 0 and st.tolist() == [0] and files == [E.case_file(fx, c)]


def test_overflow_flags_one_frame_and_leaves_its_neighbours(fx):
    cs = [_case(fx, n) for n in BATCH]
    want = [E.case_file(fx, c) for c in cs]
    frames = torch.from_numpy(np.stack([E.case_input(fx, c) for c in cs])).to(DEV)
    enc = _enc(cs[0])
    # one byte short of the noise frame's file (found by the scan's capacity test or by the layout's, after stuffing)
    rc, files, ln, st = _guarded_call(enc, frames, max_bytes=len(want[0]) - 1)
    assert rc == 0 and st.tolist() == [EOVERFLOW, 0, 0, 0] and ln.tolist() == [0] + [len(w) for w in want[1:]]
    assert files == [None] + want[1:]
    # exactly enough: nothing overflows
    rc, files, ln, st = _guarded_call(enc, frames, max_bytes=len(want[0]))
    assert rc == 0 and st.tolist() == [0] * 4 and files == want
    # through the Python layer
    big = _enc(cs[0], max_bytes=len(want[2]) - 1)
    res = big(frames[2:3])
    assert res.status().tolist() == [EOVERFLOW] and res.files(strict=False) == [None]
    with pytest.raises(JpegEncodeError, match='max_bytes'):
        res.files()


def test_short_workspace_and_bad_frames_are_refused_before_any_launch(fx):
    c = _case(fx, BATCH[0])
    frames = torch.from_numpy(E.case_input(fx, c)[None]).to(DEV)
    enc = _enc(c)
    rc, _, _, _ = _guarded_call(enc, frames, short=16)
    assert rc == -3 and b"workspace" in _lib.load().sgv3d_last_error()        # SGV3D_ENOSPACE
    saved, hip_ops.PROFILE = hip_ops.PROFILE, []
    try:
        for bad in (frames.cpu(), frames[..., 0], frames.float(), frames[:, :, :-1], frames.permute(0, 2, 1, 3)):
            with pytest.raises(JpegEncodeError):
                enc(bad)
        assert hip_ops.PROFILE == []
    finally:
        hip_ops.PROFILE = saved


@pytest.mark.parametrize("name", ['37x61_noise_420_q75_r0', '37x61_noise_420_q30_r5', '41x65_checker_444_q95_r1',
                                  '130x260_noise_422_q75_r17'])
def test_encode_then_decode_is_the_restatements_decode_of_the_fixture(fx, name):
    from sgv3d_amd.jpeg import JpegDecoder
    c = _case(fx, name)
    frames = torch.from_numpy(E.case_input(fx, c)[None]).to(DEV)
    files = _enc(c)(frames).files()
    dec = JpegDecoder(src_hw=(c['h'], c['w']), max_bytes=1 << 18, device=DEV)
    got = dec(files)
    assert dec.status().tolist() == [0]
    assert np.array_equal(got[0].cpu().numpy(), R.decode(E.case_file(fx, c)))


def test_recombine_encode_write_equals_the_host_entry(tmp_path):
    import recombine_util as U
    from sgv3d_amd import recombine as RC
    h, w = 40, 64
    dest, sources = U.make_scene(31, h, w, n_dest_obj=2, n_src_obj=3)
    on = lambda f: dict(f, image=torch.from_numpy(f['image']).to(DEV), mask=torch.from_numpy(f['mask']).to(DEV))
    rec = RC.FrameRecombiner(src_hw=(h, w), max_obj=32)
    res = rec.combine([on(dest)], [[on(s) for s in sources]])
    enc = JpegEncoder(src_hw=(h, w), device=DEV)
    data = enc(res.frames).files()[0]
    RC.write(str(tmp_path), "000007", res.frames[0], res.masks[0], dest, res.labels()[0]['lines'], encoded=data)
    on_disk = (tmp_path / "training" / "image_2" / "000007.jpg").read_bytes()
    want, st = host_entry(res.frames.cpu().numpy(), 95, '4:2:0', 0, enc.max_bytes)
    assert st.tolist() == [0] and on_disk == want[0] and on_disk[:2] == b'\xff\xd8' and on_disk[-2:] == b'\xff\xd9'
    assert R.parse(on_disk)['h'] == h and R.parse(on_disk)['w'] == w


def _labels_kernels_copies(fn):
    """The project's profiler labels of what ``fn`` enqueues, and the kernels and device -> host copies torch's profiler sees."""
    from torch.profiler import ProfilerActivity, profile
    saved = hip_ops.PROFILE
    hip_ops.PROFILE = []
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        labels = [r[0] for r in hip_ops.PROFILE]
    finally:
        hip_ops.PROFILE = saved
    names = [e.name for e in prof.events()]
    kernels = [n for n in names if any(k in n for k in ('k_transform', 'k_size', 'k_scan', 'k_pack', 'k_ffcount', 'k_layout', 'k_stuff'))
               and 'hipLaunch' not in n]
    copies = [n for n in names if 'memcpy' in n.lower()]
    print("kernels:", kernels, "copies:", sorted(set(copies)))
    return labels, kernels, [c for c in copies if 'dtoh' in c.lower().replace(' ', '')]


@pytest.mark.parametrize("batch", [1, 4])
def test_seven_launches_and_two_copies_whatever_the_batch(fx, batch):
    cs = [_case(fx, n) for n in BATCH[:batch]]
    frames = torch.from_numpy(np.stack([E.case_input(fx, c) for c in cs])).to(DEV)
    enc = _enc(cs[0])
    want = [E.case_file(fx, c) for c in cs]
    assert enc(frames).files() == want                            # (warm)
    got = []
    labels, kernels, d2h = _labels_kernels_copies(lambda: got.append(enc(frames).files()))
    assert got[0] == want
    assert labels == ["jpeg_encode", "jpeg_lengths_to_host", "jpeg_files_to_host"], labels
    assert len(kernels) == 7, kernels
    assert len(d2h) == 2, d2h


def test_graph_capture_replays_on_new_frames(fx):
    cs = [_case(fx, n) for n in BATCH]
    enc = _enc(cs[0])
    n = 2
    frames = torch.zeros(n, 37, 61, 3, dtype=torch.uint8, device=DEV)
    work = torch.empty(enc.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    files = torch.zeros(n * enc.slot_bytes, dtype=torch.uint8, device=DEV)
    words = torch.zeros(2 * n, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(frames, work=work, files=files, words=words)          # (warm, outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = enc(frames, work=work, files=files, words=words)
    for pair in ((0, 1), (2, 3), (3, 0)):
        frames.copy_(torch.from_numpy(np.stack([E.case_input(fx, cs[i]) for i in pair])).to(DEV))
        g.replay()
        torch.cuda.synchronize()
        res._words = res._files = None                            # the same buffers hold the replay's results
        assert res.files() == [E.case_file(fx, cs[i]) for i in pair]


def test_a_stream_of_more_than_256_chunks_equals_the_host_entry():
    """Noise at quality 100, 4:4:4, 520x760: a file of about 1.9 MB, more than the 256 chunks of 4096 bytes one pass of the
    layout kernel sums, and 18525 blocks, 19 per lane of the scan.  No fixture can hold it: the yardstick is the host entry,
    which the CPU tests pin to Pillow."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (1, 520, 760, 3), dtype=np.uint8)
    enc = JpegEncoder(src_hw=(520, 760), quality=100, subsampling='4:4:4', restart=95, max_bytes=3 << 20, device=DEV)
    got = enc(torch.from_numpy(a).to(DEV)).files()
    want, st = host_entry(a, 100, '4:4:4', 95, 3 << 20)
    assert st.tolist() == [0] and len(want[0]) > 256 * 4096 + 629
    assert got == want
