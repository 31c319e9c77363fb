"""On-device JPEG encoding: uint8 RGB frames -> the files ``Image.fromarray(frame).save(f, format='JPEG', quality=q,
subsampling=s, restart_marker_blocks=r)`` writes, byte for byte (Pillow over libjpeg-turbo, ``optimize`` and
``progressive`` off).

Closes the image path of the offline SSDG generation (the reference's ``save_kitti_format``,
scripts/data_preprocess/recombine_utils.py:802): decode -> recombine -> encode stay on the device and only the compressed
files cross to the host.  Seven launches (csrc/jpeg_encode.hip) whatever the batch, then two copies: the length and status
words, and the files themselves, which lie compacted one after the other at 16-byte aligned offsets.

    enc = JpegEncoder(src_hw=(1080, 1920), quality=95, subsampling='4:2:0')
    res = enc(frames)                       # uint8 cuda [B, H, W, 3] (or any lead shape); returns without waiting
    for path, data in zip(paths, res.files()):
        open(path, 'wb').write(data)

Supported: baseline sequential JPEG (SOF0), 8-bit, three YCbCr components in one interleaved scan, the Annex-K Huffman
tables; quality 1..100, 4:4:4 / 4:2:2 / 4:2:0, restart intervals 0..65535 MCUs.  The default (quality 95, 4:2:0, no restart
markers) is what OpenCV documents for ``imwrite``; that it gives OpenCV's bytes is not pinned by any test.  Anything else
(grayscale, optimised tables, progressive) raises before any launch; there is no CPU fallback.  A frame whose file would
exceed ``max_bytes`` gets status ``EOVERFLOW`` and length 0; ``files()`` raises for it, ``files(strict=False)`` gives None.
"""
import ctypes

import numpy as np
import torch

from . import _lib, hip_ops

__all__ = ['JpegEncoder', 'EncodedFrames', 'JpegEncodeError', 'SUBSAMPLING', 'EOVERFLOW', 'header']

SUBSAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}
EOVERFLOW = 1            # include/sgv3d_hip.h SGV3D_JPEG_ENC_EOVERFLOW
HEADER_MAX = 640         # SGV3D_JPEG_ENC_HEADER_MAX


class JpegEncodeError(ValueError):
    """Settings or frames the encoder does not take, or a frame whose file did not fit ``max_bytes``."""


def _up16(n):
    return (int(n) + 15) // 16 * 16


def _sampling(subsampling):
    if isinstance(subsampling, str) and subsampling in SUBSAMPLING:
        return SUBSAMPLING[subsampling]
    raise JpegEncodeError(f"JpegEncoder: subsampling {subsampling!r} is none of {sorted(SUBSAMPLING)}")


def header(h, w, quality=95, subsampling='4:2:0', restart=0):
    """-> (the bytes from SOI to the end of SOS, the quantisation tables u16 [2, 64] in natural order)."""
    hs, vs = _sampling(subsampling)
    lib = _lib.load()
    buf = (ctypes.c_uint8 * HEADER_MAX)()
    n = ctypes.c_int()
    quant = np.zeros((2, 64), np.uint16)
    rc = lib.sgv3d_jpeg_encode_header(int(h), int(w), int(quality), hs, vs, int(restart), ctypes.addressof(buf), ctypes.byref(n),
                                      quant.ctypes.data)
    if rc != 0:
        msg = lib.sgv3d_last_error()
        raise JpegEncodeError(msg.decode() if msg else f"jpeg_encode_header failed (code {rc})")
    return bytes(buf[:n.value]), quant


class EncodedFrames:
    """What ``JpegEncoder.__call__`` returns: the device buffers of one call and the event that follows its launches."""

    def __init__(self, files, words, event, n, lead):
        self.device_files, self.device_words, self.event, self.n, self.lead = files, words, event, n, lead
        self._words = None
        self._files = None

    def _host_words(self):
        if self._words is None:
            with hip_ops.prof("jpeg_lengths_to_host"):
                self._words = self.device_words.cpu().numpy()      # copy 1: lengths | status (waits for the call)
        return self._words

    def lengths(self):
        """int32 [n]: the file lengths in bytes (0 for a frame that overflowed).  Waits for the call."""
        return self._host_words()[:self.n].copy()

    def status(self):
        """int32 [n]: 0, or ``EOVERFLOW``.  Waits for the call."""
        return self._host_words()[self.n:].copy()

    def offsets(self):
        """int64 [n + 1]: where each file starts in the compacted buffer; [n] is the number of bytes to copy."""
        return np.concatenate([[0], np.cumsum((self.lengths().astype(np.int64) + 15) // 16 * 16)])

    def files(self, strict=True):
        """-> a list of ``bytes``, one file per frame.  Waits for the call."""
        if self._files is None:
            off = self.offsets()
            with hip_ops.prof("jpeg_files_to_host"):                # copy 2: the files, each rounded up to 16 bytes
                raw = self.device_files[:int(off[-1])].cpu().numpy() if off[-1] else np.zeros(0, np.uint8)
            ln = self.lengths()
            self._files = [raw[off[i]:off[i] + ln[i]].tobytes() if ln[i] else None for i in range(self.n)]
        if strict:
            bad = [i for i, f in enumerate(self._files) if f is None]
            if bad:
                raise JpegEncodeError(f"frames {bad}: the file exceeds the encoder's max_bytes (status EOVERFLOW)")
        return list(self._files)


class JpegEncoder:
    """Frames of one size (``src_hw``) -> JPEG files.  ``max_bytes``: the largest file a frame may give (buffers and grids
    follow it, never the actual lengths); the default, H W + 4096, is a third of the raw frame."""

    def __init__(self, src_hw=(1080, 1920), quality=95, subsampling='4:2:0', restart=0, max_bytes=None, device=None):
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        H, W = self.src_hw
        if not (1 <= H <= 65535 and 1 <= W <= 65535):
            raise JpegEncodeError(f"JpegEncoder: src_hw {self.src_hw} outside 1..65535")
        self.hs, self.vs = _sampling(subsampling)
        self.subsampling = subsampling
        if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
            raise JpegEncodeError(f"JpegEncoder: quality {quality!r} outside 1..100")
        if isinstance(restart, bool) or int(restart) != restart or not 0 <= int(restart) <= 65535:
            raise JpegEncodeError(f"JpegEncoder: restart interval {restart!r} outside 0..65535")
        self.quality, self.restart = int(quality), int(restart)
        self.max_bytes = H * W + 4096 if max_bytes is None else int(max_bytes)
        if not 1 <= self.max_bytes <= 1 << 26:
            raise JpegEncodeError(f"JpegEncoder: max_bytes {self.max_bytes} outside 1..2^26")
        self.slot_bytes = _up16(self.max_bytes)
        self.header, self.quant = header(H, W, self.quality, subsampling, self.restart)     # built once
        dev = torch.device(device if device is not None else 'cuda')
        if dev.type == 'cuda' and dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.device = dev

    def workspace_bytes(self, n):
        H, W = self.src_hw
        nws = int(_lib.load().sgv3d_jpeg_encode_workspace_bytes(int(n), H, W, self.hs, self.vs, self.restart, self.max_bytes))
        if nws == 0:
            msg = _lib.load().sgv3d_last_error()
            raise JpegEncodeError(msg.decode() if msg else "sgv3d_jpeg_encode_workspace_bytes refused the sizes")
        return nws

    def check(self, frames):
        """-> (n, lead) of a uint8 cuda [..., H, W, 3] tensor, or raises."""
        H, W = self.src_hw
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise JpegEncodeError("JpegEncoder: frames must be a uint8 tensor on the GPU (there is no CPU path)")
        if frames.device != self.device:
            raise JpegEncodeError(f"JpegEncoder: frames are on {frames.device}, the encoder on {self.device}")
        if frames.dtype != torch.uint8 or frames.dim() < 3 or tuple(frames.shape[-3:]) != (H, W, 3):
            raise JpegEncodeError(f"JpegEncoder: frames {tuple(frames.shape)} {frames.dtype} are not uint8 [..., {H}, {W}, 3] "
                                  f"(grayscale and other layouts are not encoded)")
        if not frames.is_contiguous():
            raise JpegEncodeError("JpegEncoder: frames must be contiguous")
        lead = tuple(frames.shape[:-3])
        n = int(np.prod(lead)) if lead else 1
        if not 1 <= n <= 4096:
            raise JpegEncodeError(f"JpegEncoder: {n} frames outside 1..4096")
        return n, lead

    def launch(self, frames, n, work, files, words):
        """Enqueue the seven launches on the current stream.  files u8 [>= n * slot_bytes], words i32 [2 n] (lengths | status),
        work u8 [workspace_bytes(n)]: device tensors the caller keeps alive."""
        H, W = self.src_hw
        with torch.cuda.device(self.device), hip_ops.prof("jpeg_encode"):
            _lib.check(_lib.load().sgv3d_jpeg_encode(
                n, H, W, self.quality, self.hs, self.vs, self.restart, self.max_bytes, frames.data_ptr(), work.data_ptr(),
                int(work.numel()), files.data_ptr(), int(files.numel()), words.data_ptr(), words.data_ptr() + 4 * n,
                _lib.stream_handle(self.device)), "jpeg_encode")

    def __call__(self, frames, work=None, files=None, words=None):
        """frames: uint8 cuda [B, H, W, 3] or lead + (H, W, 3).  Everything is checked before the first launch; the call
        returns an ``EncodedFrames`` without waiting for the device."""
        n, lead = self.check(frames)
        nws = self.workspace_bytes(n)
        with torch.cuda.device(self.device):
            if work is None:
                work = torch.empty(nws, dtype=torch.uint8, device=self.device)
            if files is None:
                files = torch.empty(n * self.slot_bytes, dtype=torch.uint8, device=self.device)
            if words is None:
                words = torch.empty(2 * n, dtype=torch.int32, device=self.device)
            self.launch(frames, n, work, files, words)
            ev = torch.cuda.Event()
            ev.record()
        return EncodedFrames(files, words, ev, n, lead)
