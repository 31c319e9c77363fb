"""An entropy re-coder for baseline JPEG files (test infrastructure, like jpeg_ref.py; numpy and bytes only, no Pillow).

``recode(data, ...)`` reads the coefficients of a valid file with ``jpeg_ref.coefficients`` and writes a new file with
the same frame header, quantisation tables and coefficient values, and a scan encoded again with

* ``tables``: 'same' (the file's own tables), or tables made from the file's symbol counts: 'long' (code lengths in
  reverse frequency order: the commonest symbols get the 10..16-bit codes), 'edge9' (the commonest symbols get lengths
  9 and 10), 'split' (Y keeps the file's tables as ids 0; Cb gets 'edge9' tables as ids 1, Cr 'long' tables as ids 2);
* ``restart``: the restart interval in MCUs (None: the file's own, 0: none);
* ``fill``: extra FF fill bytes in front of every restart marker and of EOI;
* ``segments``: words out of 'extra' (COM / APPn segments in front of SOF and between the tables and SOS, holding
  bytes that look like markers) and 'each' (one DQT / DHT segment per table instead of one segment for all).

No coefficient and no quantisation value changes.  Every table made here passes libjpeg's checks (asserted).
"""
import re
from collections import Counter

import numpy as np

import jpeg_ref as R


def segments_of(data):
    """The marker segments in front of the scan: [(marker, body bytes)], SOS last."""
    data, p, out = bytes(data), 2, []
    while True:
        while data[p + 1] == 0xFF:
            p += 1
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], 'big')
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out


def check_table(bits, vals):
    """libjpeg's jpeg_make_d_derived_tbl checks: <= 256 symbols, lengths <= 16, no code overflow (no all-ones code)."""
    assert len(bits) == 16 and sum(bits) == len(vals) and 1 <= len(vals) <= 256 and len(set(vals)) == len(vals)
    code = 0
    for ln in range(1, 17):
        code += bits[ln - 1]
        assert code < (1 << ln), f"code overflow at length {ln}"
        code <<= 1
    return bits, vals


def _table(pairs):
    """[(symbol, length)] -> (bits, vals) of the canonical table."""
    pairs = sorted(pairs, key=lambda sl: sl[1])
    bits = [sum(1 for _, l in pairs if l == ln) for ln in range(1, 17)]
    return check_table(bits, [s for s, _ in pairs])


def _fits(lengths):
    return sum(1 << (16 - l) for l in lengths) <= (1 << 16) - 1   # Kraft, with the all-ones code left free


def long_table(freq):
    """Lengths in reverse frequency order: the rarest symbols take the few short codes, the commonest 10..16 bits."""
    syms = sorted(freq, key=lambda s: (freq[s], s))               # rarest first
    n = len(syms)
    for shorts in range(min(8, n // 3), -1, -1):
        for mids in range(min(6, n - shorts), -1, -1):
            lengths = list(range(1, shorts + 1)) + list(range(10, 10 + mids)) + [16] * (n - shorts - mids)
            if _fits(lengths):
                return _table(list(zip(syms, lengths)))
    raise AssertionError("no long table fits")


def edge9_table(freq):
    """The commonest symbols get lengths 9, 10, 9, 10; the others 2..7, then 11, 12 and 16 bits."""
    syms = sorted(freq, key=lambda s: (-freq[s], s))              # commonest first
    lengths = ([9, 10, 9, 10] + [2, 3, 4, 5, 6, 7] + [11] * 20 + [12] * 40 + [16] * 256)[:len(syms)]
    assert _fits(lengths)
    return _table(list(zip(syms, lengths)))


def _symbols(coef, info, restart):
    """Per block in scan order: (component, [(class, symbol, extra bits, number of extra bits)])."""
    lum, bpm = info['hs'] * info['vs'], info['bpm']
    pred, out = [0, 0, 0], []
    for i, blk in enumerate(coef):
        m, b = divmod(i, bpm)
        comp = 0 if b < lum else b - lum + 1
        if b == 0 and restart and m % restart == 0:
            pred = [0, 0, 0]
        zz = blk[R.ZIGZAG]
        d = int(zz[0]) - pred[comp]
        pred[comp] = int(zz[0])
        s = abs(d).bit_length()
        syms = [(0, s, d if d >= 0 else d + (1 << s) - 1, s)]
        last = 0
        for k in np.nonzero(zz[1:])[0] + 1:
            run = int(k) - last - 1
            while run > 15:
                syms.append((1, 0xF0, 0, 0))
                run -= 16
            v = int(zz[k])
            s = abs(v).bit_length()
            syms.append((1, (run << 4) | s, v if v >= 0 else v + (1 << s) - 1, s))
            last = int(k)
        if last < 63:
            syms.append((1, 0x00, 0, 0))
        out.append((comp, syms))
    return out


def _encoders(tabs):
    return {key: {sym: (code, ln) for (ln, code), sym in R._codes(*bv).items()} for key, bv in tabs.items()}


def recode(data, tables='same', restart=None, fill=0, segments=''):
    """-> the bytes of the re-coded file (see the module's docstring for the knobs)"""
    data = bytes(data)
    info = R.parse(data)
    coef = R.coefficients(info)
    restart = info['restart'] if restart is None else int(restart)
    blocks = _symbols(coef, info, restart)
    # the Huffman tables {(class, id): (bits, vals)} and each component's (DC id, AC id)
    if tables == 'same':
        ids = list(info['tables'])
        used = {(c, t[c]) for t in ids for c in (0, 1)}
        tabs = {k: check_table(*info['dht'][k]) for k in sorted(used)}
    else:
        freq = {(c, comp): Counter() for c in (0, 1) for comp in range(3)}
        for comp, syms in blocks:
            for c, sym, _, _ in syms:
                freq[(c, comp)][sym] += 1
        if tables == 'split':
            ids = [(0, 0), (1, 1), (2, 2)]
            tabs = {(c, 0): check_table(*info['dht'][(c, info['tables'][0][c])]) for c in (0, 1)}
            tabs.update({(c, 1): edge9_table(freq[(c, 1)]) for c in (0, 1)})
            tabs.update({(c, 2): long_table(freq[(c, 2)]) for c in (0, 1)})
        else:
            make = {'long': long_table, 'edge9': edge9_table}[tables]
            ids = [(0, 0), (1, 1), (1, 1)]
            tabs = {(c, 0): make(freq[(c, 0)]) for c in (0, 1)}
            tabs.update({(c, 1): make(freq[(c, 1)] + freq[(c, 2)]) for c in (0, 1)})
    enc = _encoders(tabs)
    # the scan
    bpm, scan, acc, nbits, chunk = info['bpm'], bytearray(), 0, 0, bytearray()
    nmcu = len(blocks) // bpm

    def flush():
        nonlocal acc, nbits
        pad = -nbits % 8
        acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
        chunk.extend(acc.to_bytes(nbits // 8, 'big'))
        acc = nbits = 0
        scan.extend(bytes(chunk).replace(b'\xff', b'\xff\x00'))
        chunk.clear()

    for m in range(nmcu):
        if restart and m and m % restart == 0:
            flush()
            scan.extend(b'\xff' * fill + bytes([0xFF, 0xD0 + (m // restart - 1) % 8]))
        for comp, syms in blocks[m * bpm:(m + 1) * bpm]:
            for c, sym, extra, ne in syms:
                code, ln = enc[(c, ids[comp][c])][sym]
                acc, nbits = (((acc << ln) | code) << ne) | extra, nbits + ln + ne
            if nbits >= 4096:
                keep = nbits % 8
                chunk.extend((acc >> keep).to_bytes(nbits // 8, 'big'))
                acc, nbits = acc & ((1 << keep) - 1), keep
    flush()
    # the headers
    def seg(m, body):
        return bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)

    src = segments_of(data)
    extra, each = 'extra' in segments, 'each' in segments
    out = bytearray(b'\xff\xd8')
    for m, body in src:
        if 0xE0 <= m <= 0xEF:
            out += seg(m, body)
    if extra:
        out += seg(0xFE, b'a comment with marker bytes \xff\xda\x00\x0c\x03 \xff\xc4 \xff\xd9 \xff\xdd\x00\x04\x00\x01')
        out += seg(0xE5, b'\xff\xc0\x00\x11\x08' + bytes(range(40)))
    dqt = b''.join(b for m, b in src if m == 0xDB)
    one = [dqt[i:i + 65] for i in range(0, len(dqt), 65)]
    assert all(t[0] < 4 for t in one), "16-bit quantisation tables are not re-written"
    for body in (one if each else [dqt]):
        out += seg(0xDB, body)
    out += seg(*next((m, b) for m, b in src if m in (0xC0, 0xC1)))
    dht = [bytes([(c << 4) | t]) + bytes(bits) + bytes(vals) for (c, t), (bits, vals) in sorted(tabs.items())]
    for body in (dht if each else [b''.join(dht)]):
        out += seg(0xC4, body)
    if restart:
        out += seg(0xDD, restart.to_bytes(2, 'big'))
    if extra:
        out += seg(0xFE, b'\xff\xd8\xff\xda between the tables and the scan')
    sos = next(b for m, b in src if m == 0xDA)
    out += seg(0xDA, bytes([3]) + b''.join(bytes([sos[1 + 2 * i], (ids[i][0] << 4) | ids[i][1]]) for i in range(3))
               + b'\x00\x3f\x00')
    return bytes(out + scan + b'\xff' * fill + b'\xff\xd9')


# ---------------------------------------------------------------- helpers of the tests on tests/golden/jpeg_stress.npz
def case_names(fx):
    return sorted(k[:-4] for k in fx.files if k.endswith('_jpg'))


def expected(fx, name):
    """-> ('rgb', uint8 [h, w, 3]) or ('crc', uint32 [h]): Pillow's decode of the case's file."""
    alias = dict(e.split('=') for e in fx['same'].tolist())
    name = alias.get(name, name)
    return ('rgb', fx[f'{name}_rgb']) if f'{name}_rgb' in fx.files else ('crc', fx[f'{name}_crc'])


def corruptions(data):
    """Three structured corruptions of a valid file with restart markers, headers untouched and no new marker made:
    one flipped bit in the middle of the scan, the last quarter of the scan zeroed, a restart marker overwritten."""
    data = bytes(data)
    info = R.parse(data)
    s0 = data.index(info['scan'])
    n = len(info['scan'])
    out = {}
    p = s0 + n // 2
    while 0xFF in data[p - 1:p + 2] or data[p] == 0xFE or data[p - 1:p + 1] == b'\xff\x00':
        p += 1
    out['bitflip'] = data[:p] + bytes([data[p] ^ 1]) + data[p + 1:]
    out['zero_tail'] = data[:s0 + n - n // 4] + bytes(n // 4) + data[s0 + n:]
    m = [m for m in re.finditer(b'\xff+[\xd0-\xd7]', info['scan'])]
    m = m[len(m) // 2]                                                # (with its fill bytes)
    out['rst_overwritten'] = data[:s0 + m.start()] + b'\x12' * len(m.group()) + data[s0 + m.end():]
    return out


def model_status(data, seq_bytes=8):
    """The restatement's machine on a possibly corrupt scan: the true path from the first bit, and every speculative
    start of the subsequence scheme, must terminate (every step moves forward) with every coefficient index in 0..63.
    -> the status bits the kernels would report for the true path (jpeg_ref._Machine.err, 4 / 16: too few / too many
    blocks, 8 also for a restart marker that is not at the end of an interval)."""
    info = R.parse(data)
    M = R._Machine(info)
    nb = info['mcux'] * info['mcuy'] * info['bpm']

    def walk(st, end):
        blocks = 0
        while st[0] < end and st[0] < M.bits:
            nxt, dc, co = M.step(st)
            assert nxt[0] > st[0] and 0 <= nxt[1] < M.bpm and 0 <= nxt[2] < 64, (st, nxt)
            assert co is None or 0 <= co[0] <= 63, co
            if M.rst:
                ri = info['restart'] * info['bpm']
                if not ri or blocks % ri:
                    M.err |= 8
            blocks += dc
            st = nxt
        return blocks
    for j in range(-(-M.n // seq_bytes)):
        start = j * seq_bytes
        start += 1 if j and M.s[start] == 0 and M.s[start - 1] == 0xFF else 0
        walk((start * 8, 0, 0), min((j + 1) * seq_bytes, M.n) * 8)
    M.err = 0
    blocks = walk((0, 0, 0), M.bits)
    return M.err | (4 if blocks < nb else 0) | (16 if blocks > nb else 0)
