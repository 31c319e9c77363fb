"""numpy restatement of the encode csrc/jpeg_encode.hip does (test infrastructure, not product code): libjpeg's baseline
encoder as Pillow drives it (``save(format='JPEG', quality=q, subsampling=s, restart_marker_blocks=r)``), rule by rule as
DESIGN.md "JPEG encoding" states them.

* ``quant_tables``: the Annex-K tables scaled by the quality.
* ``planes``: jccolor's fixed-point RGB -> YCbCr, the edge replication and jcsample's h2v1 / h2v2 downsampling.
* ``fdct_islow``: jfdctint.c.  ``coefficients``: quantised blocks in scan order, dummy blocks included, natural order.
* ``header``: SOI .. SOS in Pillow's order.  ``encode``: the whole file.
* ``load_fixture`` / ``case_input`` / ``case_file``: tests/golden/jpeg_encode.npz.
"""
import os

import numpy as np

import jpeg_ref as R

SUBSAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}

K_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                   72, 92, 95, 98, 112, 100, 103, 99])
K_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99]
                    + [99] * 36)
# Annex K.3 - K.6: (BITS, HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
            0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
            0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
            0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
            0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
            0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
            0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
              0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
              0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
              0xf9, 0xfa])


def quant_tables(quality):
    """-> (luma, chroma) int64 [64] in natural order: jpeg_set_quality with force_baseline."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (K_LUMA, K_CHROMA))


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad_right(p, width):
    return np.concatenate([p, np.repeat(p[:, -1:], width - p.shape[1], axis=1)], axis=1) if width > p.shape[1] else p


def _pad_down(p, height):
    return np.concatenate([p, np.repeat(p[-1:], height - p.shape[0], axis=0)], axis=0) if height > p.shape[0] else p


def planes(rgb, hs, vs):
    """-> [Y, Cb, Cr] planes padded to whole MCUs the way libjpeg's pre-processing controller pads them."""
    H, W = rgb.shape[:2]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    out = []
    for c, p in enumerate(ycc(rgb)):
        h, v = (1, 1) if c == 0 else (hs, vs)                    # downsampling factors of the component
        wblocks = -(-(-(-W // h)) // 8)                          # width_in_blocks
        p = _pad_right(p, wblocks * 8 * h)                       # replicated before downsampling
        p = _pad_down(p, -(-H // vs) * vs)                       # only up to a multiple of the MCU's sample rows
        if h == 2 and v == 1:
            bias = np.arange(p.shape[1] // 2) & 1
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif h == 2 and v == 2:
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        rows = mcuy * 8 * (vs if c == 0 else 1)
        out.append(_pad_right(_pad_down(p, rows), mcux * 8 * (hs if c == 0 else 1)))   # the last downsampled row, replicated
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    d = [d[..., i] for i in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (tmp10 + tmp11) << 2 if first else _descale(tmp10 + tmp11, 2)
    o[4] = (tmp10 - tmp11) << 2 if first else _descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * 4433
    o[2] = _descale(z1 + tmp13 * 6270, n)
    o[6] = _descale(z1 - tmp12 * 15137, n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5] = _descale(tmp4 + z1 + z3, n), _descale(tmp5 + z2 + z4, n)
    o[3], o[1] = _descale(tmp6 + z2 + z3, n), _descale(tmp7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_islow(blocks):
    """int64 [..., 8, 8] samples (not yet level shifted) -> jfdctint's output (scaled by 8)."""
    x = _fdct_1d(blocks.astype(np.int64) - 128, True)                       # the rows
    return np.swapaxes(_fdct_1d(np.swapaxes(x, -1, -2), False), -1, -2)     # the columns


def quantise(c, q):
    d = q.reshape(8, 8) * 8
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(rgb, quality, hs, vs):
    """-> int64 [blocks, 64], natural order, in scan order (luma blocks of the MCU row by row, Cb, Cr), dummy blocks included."""
    H, W = rgb.shape[:2]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    wb, hb = -(-W // 8), -(-H // 8)
    ql, qc = quant_tables(quality)
    pl = planes(rgb, hs, vs)

    def blocks(p, q):
        b = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).swapaxes(1, 2)
        return quantise(fdct_islow(b), q).reshape(b.shape[0], b.shape[1], 64)
    y, cb, cr = blocks(pl[0], ql), blocks(pl[1], qc), blocks(pl[2], qc)
    out = []
    for my in range(mcuy):
        for mx in range(mcux):
            mcu = []
            for r in range(vs):
                for c in range(hs):
                    by, bx = my * vs + r, mx * hs + c
                    if by < hb and bx < wb:
                        mcu.append(y[by, bx])
                    else:                                        # a dummy block: the DC of the block before it, or of the last
                        blk = np.zeros(64, np.int64)             # block of the MCU's previous block row
                        blk[0] = mcu[-1][0] if by < hb else mcu[r * hs - 1][0]
                        mcu.append(blk)
            out.extend(mcu + [cb[my, mx], cr[my, mx]])
    return np.stack(out)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)


def header(H, W, quality, hs, vs, restart):
    out = b'\xff\xd8' + _seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t, q in enumerate(quant_tables(quality)):
        out += _seg(0xDB, bytes([t]) + bytes(int(v) for v in q[R.ZIGZAG]))
    out += _seg(0xC0, bytes([8]) + H.to_bytes(2, 'big') + W.to_bytes(2, 'big')
                + bytes([3, 1, hs * 16 + vs, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tid, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _seg(0xC4, bytes([tid]) + bytes(bits) + bytes(vals))
    if restart:
        out += _seg(0xDD, restart.to_bytes(2, 'big'))
    return out + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def scan(coef, hs, vs, restart):
    enc = [{sym: (code, ln) for (ln, code), sym in R._codes(*t).items()} for t in (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)]
    lum, bpm = hs * vs, hs * vs + 2
    out, acc, nbits, pred = bytearray(), 0, 0, [0, 0, 0]

    def flush():
        nonlocal acc, nbits
        pad = -nbits % 8
        acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
        out.extend(acc.to_bytes(nbits // 8, 'big').replace(b'\xff', b'\xff\x00'))
        acc = nbits = 0

    def put(code, ln):
        nonlocal acc, nbits
        acc, nbits = (acc << ln) | code, nbits + ln

    for i, blk in enumerate(coef):
        m, b = divmod(i, bpm)
        comp = 0 if b < lum else b - lum + 1
        if b == 0 and restart and m and m % restart == 0:
            flush()
            out.extend([0xFF, 0xD0 + (m // restart - 1) % 8])
            pred = [0, 0, 0]
        dc, ac = enc[2 * (comp > 0)], enc[2 * (comp > 0) + 1]
        zz = blk[R.ZIGZAG]
        d, pred[comp] = int(zz[0]) - pred[comp], int(zz[0])
        s = abs(d).bit_length()
        put(*dc[s])
        put(d if d >= 0 else d + (1 << s) - 1, s)
        last = 0
        for k in np.nonzero(zz[1:])[0] + 1:
            run, v = int(k) - last - 1, int(zz[k])
            while run > 15:
                put(*ac[0xF0])
                run -= 16
            s = abs(v).bit_length()
            put(*ac[(run << 4) | s])
            put(v if v >= 0 else v + (1 << s) - 1, s)
            last = int(k)
        if last < 63:
            put(*ac[0])
        if nbits >= 4096:
            keep = nbits % 8
            out.extend((acc >> keep).to_bytes(nbits // 8, 'big').replace(b'\xff', b'\xff\x00'))
            acc, nbits = acc & ((1 << keep) - 1), keep
    flush()
    return bytes(out)


def encode(rgb, quality=95, subsampling='4:2:0', restart=0):
    """uint8 [H, W, 3] -> the bytes of the file."""
    hs, vs = SUBSAMPLING[subsampling]
    H, W = rgb.shape[:2]
    return header(H, W, quality, hs, vs, restart) + scan(coefficients(rgb, quality, hs, vs), hs, vs, restart) + b'\xff\xd9'


# ---------------------------------------------------------------- tests/golden/jpeg_encode.npz
def load_fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_encode.npz'))


def cases(fx):
    """-> [dict(name, h, w, content, subsampling, quality, restart)] in the fixture's order"""
    out = []
    for line in fx['cases'].tolist():
        name, h, w, content, sub, q, r = line.split('|')
        out.append(dict(name=name, h=int(h), w=int(w), content=content, subsampling=sub, quality=int(q), restart=int(r)))
    return out


def case_input(fx, c):
    return fx[f"in_{c['h']}x{c['w']}_{c['content']}"]


def case_file(fx, c):
    return fx[f"f_{c['name']}"].tobytes()
