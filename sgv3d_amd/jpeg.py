"""On-device JPEG decoding: camera files -> the uint8 RGB frames ``np.asarray(Image.open(f))`` gives, byte for byte.

Replaces the last CPU stage of the reference dataset's image path (dataset/nusc_mv_det_dataset.py:510 ``Image.open``,
:617 ``np.array(img)``).  The host parses each file's headers (``sgv3d_jpeg_parse``) and packs the descriptors and the
entropy-coded segments into one pinned buffer; one non-blocking upload and eight launches (csrc/jpeg.hip) do the rest.
The output feeds ``ImagePreprocessor``, ``TrainAugmenter`` and ``FramePipeline`` as it is.

    dec = JpegDecoder(src_hw=(1080, 1920))
    frames = dec([open(p, 'rb').read() for p in paths])          # uint8 cuda [B, H, W, 3]
    imgs, ida_mats = pre(frames)

Supported: Huffman-coded sequential 8-bit JPEG (SOF0 / SOF1), three YCbCr components in one interleaved scan, 4:4:4,
4:2:2 or 4:2:0, any size, with or without restart markers, 8- or 16-bit quantisation tables, standard or optimised
Huffman tables.  Anything else raises ``JpegError`` before any launch; there is no CPU fallback.  Nothing here
synchronises the host except ``status()``.  ``JpegStaging`` splits a call into staging (host only) and launching (the
upload + kernels), so that the launch half can be captured into a graph and replayed after new files are staged.
"""
import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ['JpegDecoder', 'JpegStaging', 'JpegError', 'parse', 'FRAME_DTYPE', 'STATUS_BITS']

HUFF_DTYPE = np.dtype([('look', '<u2', (512,)), ('maxcode', '<i4', (18,)), ('valoff', '<i4', (18,)),
                       ('huffval', 'u1', (256,))])
FRAME_DTYPE = np.dtype([('width', '<i4'), ('height', '<i4'), ('hs', '<i4'), ('vs', '<i4'), ('mcux', '<i4'),
                        ('mcuy', '<i4'), ('blocks_per_mcu', '<i4'), ('restart', '<i4'), ('scan_off', '<i8'),
                        ('scan_len', '<i4'), ('pad', '<i4'), ('quant', '<u2', (3, 64)), ('huff', HUFF_DTYPE, (3, 2))])
assert HUFF_DTYPE.itemsize == 1424 and FRAME_DTYPE.itemsize == 8976   # include/sgv3d_hip.h

# sgv3d_jpeg_decode's per-frame status bits (include/sgv3d_hip.h SGV3D_JPEG_E*)
STATUS_BITS = {1: 'bad Huffman code', 2: 'coefficient index past 63', 4: 'scan ended before the last MCU',
               8: 'marker where no restart interval ends', 16: 'more blocks than the frame has'}

DEFAULT_SEQ_BYTES = 64     # subsequence length of the parallel entropy decode (a launch argument: any 8 .. 2^20)
MIN_SEQ_BYTES = 8


class JpegError(ValueError):
    """A file the decoder does not take (the message names the feature), or a batch it cannot decode together."""


def parse(data):
    """Host parse of one file -> its descriptor (a ``FRAME_DTYPE`` record; ``scan_off`` relative to the file)."""
    lib = _lib.load()
    mv = memoryview(data).cast('B')
    buf = (ctypes.c_uint8 * len(mv)).from_buffer_copy(mv) if mv.readonly else (ctypes.c_uint8 * len(mv)).from_buffer(mv)
    rec = np.zeros(1, FRAME_DTYPE)
    h, w = ctypes.c_int(), ctypes.c_int()
    rc = lib.sgv3d_jpeg_parse(ctypes.addressof(buf), len(mv), rec.ctypes.data, ctypes.byref(h), ctypes.byref(w))
    if rc != 0:
        msg = lib.sgv3d_last_error()
        raise JpegError(msg.decode() if msg else f"jpeg_parse failed (code {rc})")
    return rec[0], buf


def _up16(n):
    return (int(n) + 15) // 16 * 16


class JpegDecoder:
    """Batches of JPEG files of one size (``src_hw``) -> uint8 cuda frames.  ``max_bytes``: the largest entropy-coded
    segment a frame may have (grids and buffers are sized from it, never from the actual lengths); ``seq_bytes``: the
    subsequence length of the parallel entropy decode."""

    def __init__(self, src_hw=(1080, 1920), max_bytes=1 << 20, device=None, seq_bytes=DEFAULT_SEQ_BYTES):
        dev = torch.device(device if device is not None else 'cuda')
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.max_bytes = int(max_bytes)
        self.seq_bytes = int(seq_bytes)
        if not (1 <= self.src_hw[0] <= 65535 and 1 <= self.src_hw[1] <= 65535):
            raise ValueError(f"JpegDecoder: src_hw {self.src_hw} outside 1..65535")
        if not 1 <= self.max_bytes <= 1 << 26:
            raise ValueError(f"JpegDecoder: max_bytes {self.max_bytes} outside 1..2^26")
        if not MIN_SEQ_BYTES <= self.seq_bytes <= 1 << 20:
            raise ValueError(f"JpegDecoder: seq_bytes {self.seq_bytes} outside {MIN_SEQ_BYTES}..2^20")
        self.slot_bytes = _up16(self.max_bytes)
        self._status = None

    # ---- host half
    def plan(self, jpegs, lead=None):
        """Parse every file and check the batch -> (descriptors FRAME_DTYPE [n], [(scan bytes view)], lead)."""
        if isinstance(jpegs, (bytes, bytearray, memoryview)) or not hasattr(jpegs, '__len__'):
            raise TypeError("JpegDecoder: jpegs must be a list of bytes-like objects")
        n = len(jpegs)
        if n == 0:
            raise ValueError("JpegDecoder: empty batch")
        if lead is None:
            lead = (n,)
        lead = tuple(int(v) for v in lead)
        if int(np.prod(lead)) != n:
            raise ValueError(f"JpegDecoder: lead {lead} does not hold {n} frames")
        recs = np.zeros(n, FRAME_DTYPE)
        scans = []
        H, W = self.src_hw
        for i, data in enumerate(jpegs):
            try:
                rec, buf = parse(data)
            except JpegError as e:
                raise JpegError(f"frame {i}: {e}") from None
            if (int(rec['height']), int(rec['width'])) != (H, W):
                raise JpegError(f"frame {i}: {int(rec['height'])}x{int(rec['width'])}, the decoder is built for {H}x{W} "
                                f"(frames must not differ in size)")
            if i and (int(rec['hs']), int(rec['vs'])) != (int(recs[0]['hs']), int(recs[0]['vs'])):
                raise JpegError(f"frame {i}: sampling {int(rec['hs'])}x{int(rec['vs'])}, frame 0 "
                                f"{int(recs[0]['hs'])}x{int(recs[0]['vs'])} (frames must not differ in sampling)")
            if int(rec['scan_len']) > self.max_bytes:
                raise JpegError(f"frame {i}: scan of {int(rec['scan_len'])} bytes exceeds the decoder's capacity of "
                                f"{self.max_bytes} bytes (max_bytes)")
            off, ln = int(rec['scan_off']), int(rec['scan_len'])
            scans.append((buf, off, ln))
            recs[i] = rec
        return recs, scans, lead

    @staticmethod
    def packed_bytes(scans):
        """Bytes ``pack`` writes: the descriptors, then every scan rounded up to 16 bytes."""
        return len(scans) * FRAME_DTYPE.itemsize + sum(_up16(ln) for _, _, ln in scans)

    def pack(self, recs, scans, host):
        """Descriptors, then the scans one after the other at 16-byte aligned offsets of the data region, into the uint8
        array ``host`` (at least ``packed_bytes(scans)`` long)."""
        n = len(recs)
        dbytes = n * FRAME_DTYPE.itemsize
        o = 0
        for i, (buf, off, ln) in enumerate(scans):
            ctypes.memmove(host.ctypes.data + dbytes + o, ctypes.addressof(buf) + off, ln)
            recs[i]['scan_off'] = o
            o += _up16(ln)
        host[:dbytes] = recs.view(np.uint8)
        return recs

    def staging_bytes(self, n):
        """Capacity of a staging buffer for n frames (``JpegStaging``)."""
        return n * FRAME_DTYPE.itemsize + n * self.slot_bytes

    def workspace_bytes(self, n, seq_bytes=None):
        H, W = self.src_hw
        seq = self.seq_bytes if seq_bytes is None else int(seq_bytes)
        return int(_lib.load().sgv3d_jpeg_workspace_bytes(n, H, W, self.max_bytes, seq))

    # ---- device half
    def launch(self, recs, dev_staging, work, status, out, seq_bytes=None):
        """Enqueue the kernels on the current stream: ``dev_staging`` holds what ``pack`` wrote, ``recs`` its host copy."""
        n = len(recs)
        H, W = self.src_hw
        dbytes = n * FRAME_DTYPE.itemsize
        seq = self.seq_bytes if seq_bytes is None else int(seq_bytes)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().sgv3d_jpeg_decode(
                n, H, W, self.max_bytes, seq, recs.ctypes.data, dev_staging.data_ptr(), dev_staging.data_ptr() + dbytes,
                int(dev_staging.numel() - dbytes), status.data_ptr(), work.data_ptr(), int(work.numel()),
                out.data_ptr(), _lib.stream_handle(self.device)), "jpeg_decode")

    def _out(self, lead, out):
        shape = lead + self.src_hw + (3,)
        if out is None:
            return torch.empty(shape, dtype=torch.uint8, device=self.device)
        if tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"JpegDecoder: out must be a contiguous uint8 {shape} tensor on {self.device}")
        return out

    def __call__(self, jpegs, out=None, lead=None, seq_bytes=None):
        """jpegs: a list of bytes-like files -> uint8 cuda [B, H, W, 3], or lead + (H, W, 3) with ``lead=(B, S, N)``.
        Everything is checked before the first launch; the call returns without waiting for the device."""
        if seq_bytes is not None and not MIN_SEQ_BYTES <= int(seq_bytes) <= 1 << 20:
            raise ValueError(f"JpegDecoder: seq_bytes {seq_bytes} outside {MIN_SEQ_BYTES}..2^20")
        recs, scans, lead = self.plan(jpegs, lead)
        out = self._out(lead, out)
        n = len(recs)
        # a fresh pinned block per call: the caching host allocator keeps it until the copy below has run
        host = torch.empty(self.packed_bytes(scans), dtype=torch.uint8, pin_memory=True)
        self.pack(recs, scans, host.numpy())
        with torch.cuda.device(self.device):
            dev = host.to(self.device, non_blocking=True)
            work = torch.empty(self.workspace_bytes(n, seq_bytes), dtype=torch.uint8, device=self.device)
            status = torch.empty(n, dtype=torch.int32, device=self.device)
            self.launch(recs, dev, work, status, out, seq_bytes)
        self._status = status
        return out

    def status(self):
        """Per-frame status words of the last call (0: decoded cleanly; bits: ``STATUS_BITS``).  Waits for that call."""
        if self._status is None:
            raise RuntimeError("JpegDecoder: nothing decoded yet")
        return self._status.cpu().numpy()


class JpegStaging:
    """Persistent buffers for batches of ``n = prod(lead)`` files: a pinned staging buffer, its device copy, the
    workspace, the status words and the output frames ``out`` (uint8 lead + (H, W, 3)).

    ``stage(jpegs)`` parses and packs on the host only; ``launch()`` enqueues the upload and the kernels on the current
    stream, and can be captured into a graph: a replay decodes whatever was staged last.  The caller must not stage
    while a queued upload still reads the pinned buffer (wait for the event of the previous launch)."""

    def __init__(self, dec, lead, out=None):
        self.dec = dec
        self.lead = tuple(int(v) for v in lead)
        self.n = int(np.prod(self.lead))
        self.host = torch.empty(dec.staging_bytes(self.n), dtype=torch.uint8, pin_memory=True)
        self.dev = torch.zeros(dec.staging_bytes(self.n), dtype=torch.uint8, device=dec.device)
        self.work = torch.empty(dec.workspace_bytes(self.n), dtype=torch.uint8, device=dec.device)
        self.status_words = torch.zeros(self.n, dtype=torch.int32, device=dec.device)
        self.out = dec._out(self.lead, out)
        self.recs = None

    def stage(self, jpegs):
        recs, scans, _ = self.dec.plan(jpegs, self.lead)
        self.recs = self.dec.pack(recs, scans, self.host.numpy())

    def launch(self):
        if self.recs is None:
            raise RuntimeError("JpegStaging: nothing staged")
        with torch.cuda.device(self.dec.device):
            self.dev.copy_(self.host, non_blocking=True)
            self.dec.launch(self.recs, self.dev, self.work, self.status_words, self.out)
        return self.out

    def status(self):
        return self.status_words.cpu().numpy()
