"""numpy restatement of the decode csrc/jpeg.hip does (test infrastructure, not product code).

* ``parse``: markers -> sizes, sampling, quantisation tables (natural order), Huffman tables, restart interval, scan.
* ``coefficients``: a sequential Huffman decoder as libjpeg's decode_mcu runs it (MCU by MCU, restart markers read where
  an interval ends, DC predictors reset there) -> int [blocks, 64] in natural order, DC predicted.
* ``coefficients_parallel``: a model of the kernels' subsequence-and-resolve scheme (speculative decode from guessed
  states, continuation until synchronised, anchors, exclusive scan, final decode, DC prefix sums) on the same scan.
* ``idct_islow``: jidctint.c in int64 with its range-limit table; ``upsample``: jdsample.c's fancy upsampling;
  ``ycc_to_rgb``: jdcolor.c's fixed-point conversion; ``decode``: the whole path -> uint8 [H, W, 3].
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def parse(data):
    data = bytes(data)
    assert data[:2] == b'\xff\xd8', "no SOI"
    p, out = 2, dict(restart=0, qt={}, dht={})
    while True:
        while data[p] == 0xFF and data[p + 1] == 0xFF:
            p += 1
        assert data[p] == 0xFF
        m = data[p + 1]
        p += 2
        if 0xD0 <= m <= 0xD7 or m in (0x01, 0xD8):
            continue
        seg = int.from_bytes(data[p:p + 2], 'big')
        body, p = data[p + 2:p + seg], p + seg
        if m in (0xC0, 0xC1):
            assert body[0] == 8
            out['h'], out['w'] = int.from_bytes(body[1:3], 'big'), int.from_bytes(body[3:5], 'big')
            out['comps'] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i])
                            for i in range(body[5])]
        elif m == 0xC4:
            q = 0
            while q < len(body):
                tc, th = body[q] >> 4, body[q] & 15
                bits = list(body[q + 1:q + 17])
                n = sum(bits)
                out['dht'][(tc, th)] = (bits, list(body[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                w = 2 if pq else 1
                vals = [int.from_bytes(body[q + 1 + w * k:q + 1 + w * (k + 1)], 'big') for k in range(64)]
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = vals
                out['qt'][tq] = nat
                q += 1 + 64 * w
        elif m == 0xDD:
            out['restart'] = int.from_bytes(body[:2], 'big')
        elif m == 0xDA:
            ns = body[0]
            out['tables'] = [(body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            s0 = p
            q = s0
            while True:
                q = data.index(b'\xff', q)
                r = q + 1
                while data[r] == 0xFF:
                    r += 1
                if data[r] == 0 or 0xD0 <= data[r] <= 0xD7:
                    q = r + 1
                    continue
                break
            out['scan'] = data[s0:q]
            hs, vs = out['comps'][0][1], out['comps'][0][2]
            out['hs'], out['vs'] = hs, vs
            out['mcux'] = -(-out['w'] // (8 * hs))
            out['mcuy'] = -(-out['h'] // (8 * vs))
            out['bpm'] = hs * vs + 2
            return out


def _codes(bits, vals):
    """canonical Huffman codes -> {(length, code): symbol}"""
    table, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            table[(ln, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _destuff(seg):
    return seg.replace(b'\xff\x00', b'\xff')


def _block_tables(info):
    """per block of an MCU: (component, DC table, AC table)"""
    lum = info['hs'] * info['vs']
    tabs = [(_codes(*info['dht'][(0, td)]), _codes(*info['dht'][(1, ta)])) for td, ta in info['tables']]
    return [(0 if b < lum else b - lum + 1,) + tabs[0 if b < lum else b - lum + 1] for b in range(info['bpm'])]


class _Bits:
    def __init__(self, seg):
        self.bits = np.unpackbits(np.frombuffer(_destuff(seg), np.uint8))
        self.p = 0

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | (int(self.bits[self.p]) if self.p < len(self.bits) else 0)
            self.p += 1
        return v


def coefficients(info, trace=None):
    """libjpeg's sequential decode -> int64 [blocks, 64] natural order, DC predicted.  ``trace``: a list that receives
    (class, code length, symbol) of every Huffman code in decode order."""
    scan = info['scan']
    ri = info['restart']
    # the intervals: split at RSTn markers
    segs, q, start = [], 0, 0
    while True:
        q = scan.find(b'\xff', q)
        if q < 0:
            break
        r = q + 1
        while r < len(scan) and scan[r] == 0xFF:
            r += 1
        if r < len(scan) and 0xD0 <= scan[r] <= 0xD7:
            segs.append(scan[start:q])
            start = q = r + 1
        else:
            q = r + 1
    segs.append(scan[start:])
    bt = _block_tables(info)
    nmcu = info['mcux'] * info['mcuy']
    coef = np.zeros((nmcu * info['bpm'], 64), np.int64)
    si, rd, pred = 0, _Bits(segs[0]), [0, 0, 0]
    for m in range(nmcu):
        if ri and m and m % ri == 0:
            si += 1
            rd, pred = _Bits(segs[si]), [0, 0, 0]
        for b, (comp, dct, act) in enumerate(bt):
            blk = coef[m * info['bpm'] + b]
            s = _huff(rd, dct, trace, 0)
            pred[comp] += _extend(rd.get(s), s)
            blk[0] = pred[comp]
            k = 1
            while k < 64:
                rs = _huff(rd, act, trace, 1)
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    blk[ZIGZAG[k]] = _extend(rd.get(s), s)
                elif r != 15:
                    break
                else:
                    k += 15
                k += 1
    return coef


def _huff(rd, table, trace=None, cls=0):
    code = 0
    for ln in range(1, 17):
        code = (code << 1) | rd.get(1)
        if (ln, code) in table:
            if trace is not None:
                trace.append((cls, ln, table[(ln, code)]))
            return table[(ln, code)]
    raise ValueError("bad Huffman code")


# ---------------------------------------------------------------- the kernels' scheme, restated
class _Machine:
    """The state machine of csrc/jpeg.hip's step(): state (raw bit offset, block in MCU, coefficient index)."""

    def __init__(self, info):
        self.s = info['scan']
        self.n = len(self.s)
        self.bits = 8 * self.n
        self.bpm = info['bpm']
        bt = _block_tables(info)
        self.tab = [(d, a) for _, d, a in bt]
        self.err = 0   # the kernel's status bits met so far: 1 bad code, 2 coefficient past 63, 4 short, 8 marker

    def _byte(self, i):
        return self.s[i] if i < self.n else None

    def _marker(self, m):
        while m + 1 < self.n and self.s[m + 1] == 0xFF:
            m += 1
        if m + 1 < self.n and 0xD0 <= self.s[m + 1] <= 0xD7:
            return (m + 2) * 8
        return self.bits

    def step(self, st):
        """-> (new state, DC code?, coefficient (zigzag index, value) or None)"""
        pos, b, k = st
        byte0, sh = pos >> 3, pos & 7
        self.rst = False   # (True after a step that took a restart marker)
        # destuffed bytes from byte0 (raw offset of each), up to the first marker / the end
        dbytes, raws, r = [], [], 0
        while len(dbytes) < 5:
            v = self._byte(byte0 + r)
            if v is None:
                break
            if v != 0xFF:
                dbytes.append(v)
                raws.append(r)
                r += 1
            elif self._byte(byte0 + r + 1) == 0:
                dbytes.append(0xFF)
                raws.append(r)
                r += 2
            else:
                break
        mk = len(dbytes) if len(dbytes) < 5 else 5
        mraw = r   # raw offset of the marker when mk < 5
        q = 1 if sh else 0
        ones = (1 << (8 - sh)) - 1
        if mk == q and (sh == 0 or (dbytes[0] & ones) == ones):
            if b or k:
                self.err |= 8
            after = self._marker(byte0 + (raws[1] if q and len(raws) > 1 else (mraw if q else 0)))
            self.rst = after < self.bits
            return (after, 0, 0), False, None
        acc = 0
        for i in range(5):
            acc = (acc << 8) | (dbytes[i] if i < mk else 0)
        peek = ((acc << (24 + sh)) >> 32) & 0xFFFFFFFF
        comp = self.tab[b][1 if k else 0]
        ln = sym = None
        for l in range(1, 17):
            if (l, peek >> (32 - l)) in comp:
                ln, sym = l, comp[(l, peek >> (32 - l))]
                break
        if ln is None:
            ln, sym = 16, 0
            self.err |= 1
        ns = sym & 15
        nb = ln + ns
        if sh + nb > 8 * mk:
            self.err |= 4
            return (self._marker(byte0 + mraw), 0, 0), False, None
        val = _extend(((peek << ln) & 0xFFFFFFFF) >> (32 - ns), ns) if ns else 0
        o2 = sh + nb
        j = o2 >> 3
        rj = raws[j] if j < len(raws) else mraw
        pos = (byte0 + rj) * 8 + (o2 & 7)
        dc, co = False, None
        if k == 0:
            dc, co, k = True, (0, val), 1
        else:
            run = sym >> 4
            if ns == 0:
                k = k + 16 if run == 15 else 64
                if k > 64:
                    self.err |= 2
                k = min(k, 64)
            else:
                k += run
                if k > 63:
                    self.err |= 2
                    k = 64
                else:
                    co, k = (k, val), k + 1
        if k == 64:
            k, b = 0, (b + 1) % self.bpm
        return (pos, b, k), dc, co

    def run(self, st, end, sink=None):
        n = 0
        while st[0] < end and st[0] < self.bits:
            st, dc, co = self.step(st)
            n += dc
            if sink is not None:
                sink(dc, co)
        return st, n


def coefficients_parallel(info, seq_bytes):
    """The kernels' scheme with subsequences of ``seq_bytes`` -> (coefficients as ``coefficients``, the anchors)."""
    M = _Machine(info)
    L = M.n
    nsub = -(-L // seq_bytes)
    end = lambda j: min((j + 1) * seq_bytes, L) * 8
    exits, cnt = [], []
    for j in range(nsub):   # A: speculative
        start = j * seq_bytes
        if j and M.s[start] == 0 and M.s[start - 1] == 0xFF:
            start += 1
        st, n = M.run((start * 8, 0, 0), end(j))
        exits.append(st)
        cnt.append(n)
    sync, rcnt = [], []
    for j in range(nsub):   # B: continuation until synchronised
        st, n, m = exits[j], cnt[0] if j == 0 else 0, j + 1
        while m < nsub:
            st, c = M.run(st, end(m))
            n += c
            if st == exits[m]:
                break
            m += 1
        sync.append(m)
        rcnt.append(n)
    anchors, a = [], 0   # C: the anchor chain and the exclusive scan
    while a < nsub:
        anchors.append(a)
        a = sync[a]
    base, tot = {}, 0
    for a in anchors:
        base[a] = tot
        tot += rcnt[a]
    nb = info['mcux'] * info['mcuy'] * info['bpm']
    assert tot == nb, (tot, nb)
    coef = np.zeros((nb, 64), np.int64)
    for a in anchors:   # D: final decode
        st = (0, 0, 0) if a == 0 else exits[a]
        idx = [base[a] - 1]

        def sink(dc, co, idx=idx):
            idx[0] += dc
            if co is not None:
                coef[idx[0], ZIGZAG[co[0]]] = co[1]
        M.run(st, M.bits if sync[a] >= nsub else end(sync[a]), sink)
    # E: DC prediction per component, reset at every restart interval
    lum, bpm, ri = info['hs'] * info['vs'], info['bpm'], info['restart']
    for comp, (off, per) in enumerate([(0, lum), (lum, 1), (lum + 1, 1)]):
        run = 0
        for m in range(info['mcux'] * info['mcuy']):
            if m == 0 or (ri and m % ri == 0):
                run = 0
            for i in range(per):
                run += coef[m * bpm + off + i, 0]
                coef[m * bpm + off + i, 0] = run
    return coef, anchors


# ---------------------------------------------------------------- IDCT, upsampling, colour
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(v):
    """v: int64 [..., 8] -> the eight sums of jidctint.c before descaling"""
    i0, i1, i2, i3, i4, i5, i6, i7 = [v[..., i] for i in range(8)]
    z1 = (i2 + i6) * 4433
    tmp2 = z1 + i6 * -15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i7, i5, i3, i1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    return np.stack([t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3], -1)


def idct_islow(coef, q):
    """coef int [n, 64] natural order, q [64] -> uint8 [n, 8, 8] (jidctint.c + its range-limit table)"""
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(-1, 8, 8)
    ws = _descale(_idct_1d(x.transpose(0, 2, 1)), 11).astype(np.int32).astype(np.int64)   # columns -> int workspace
    ws = ws.transpose(0, 2, 1)                                   # [n, row, col]
    out = _descale(_idct_1d(ws), 18)
    w = ((out + 512) & 1023) - 512 + 128
    return np.clip(w, 0, 255).astype(np.uint8)


def planes(info, coef):
    """The padded component planes (uint8) the IDCT fills."""
    hs, vs, mx, my, bpm = info['hs'], info['vs'], info['mcux'], info['mcuy'], info['bpm']
    lum = hs * vs
    qs = [info['qt'][c[3]] for c in info['comps']]
    out = []
    for comp in range(3):
        if comp == 0:
            idx = [(u % hs, u // hs, u) for u in range(lum)]
            H, W = my * vs * 8, mx * hs * 8
        else:
            idx = [(0, 0, lum + comp - 1)]
            H, W = my * 8, mx * 8
        pl = np.zeros((H, W), np.uint8)
        blocks = idct_islow(coef, qs[comp]).reshape(my, mx, bpm, 8, 8)
        for ox, oy, u in idx:
            h1 = hs if comp == 0 else 1
            v1 = vs if comp == 0 else 1
            b = blocks[:, :, u]                                  # [my, mx, 8, 8]
            view = pl.reshape(my, v1, 8, mx, h1, 8)
            view[:, oy, :, :, ox, :] = b.transpose(0, 2, 1, 3)
        out.append(pl)
    return out


def upsample(c, hs, vs, H, W):
    """jdsample.c: fancy h2v1 / h2v2 (box when the downsampled width is 1 or 2) -> int [H, W]"""
    c = c.astype(np.int64)
    if hs == 1:
        return c[:H, :W]
    dw, dh = -(-W // hs), -(-H // vs)
    x = np.arange(W)
    cx = x >> 1
    if dw <= 2:
        rows = (np.arange(H) >> 1) if vs == 2 else np.arange(H)
        return c[rows][:, cx]
    xn = np.where(x & 1, np.minimum(cx + 1, dw - 1), np.maximum(cx - 1, 0))
    if vs == 1:
        row = c[:H]
        return np.where(x & 1, (3 * row[:, cx] + row[:, xn] + 2) >> 2, (3 * row[:, cx] + row[:, xn] + 1) >> 2)
    y = np.arange(H)
    cy = y >> 1
    yn = np.where(y & 1, np.minimum(cy + 1, dh - 1), np.maximum(cy - 1, 0))
    cs = 3 * c[cy] + c[yn]                                       # [H, cw]
    return np.where(x & 1, (3 * cs[:, cx] + cs[:, xn] + 7) >> 4, (3 * cs[:, cx] + cs[:, xn] + 8) >> 4)


def ycc_to_rgb(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-46802 * cr + (-22554 * cb + 32768)) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data, seq_bytes=None):
    """The whole decode -> uint8 [H, W, 3] (sequential entropy decode, or the subsequence scheme with seq_bytes)."""
    info = parse(data)
    coef = coefficients(info) if seq_bytes is None else coefficients_parallel(info, seq_bytes)[0]
    Y, Cb, Cr = planes(info, coef)
    H, W = info['h'], info['w']
    return ycc_to_rgb(Y[:H, :W].astype(np.int64), upsample(Cb, info['hs'], info['vs'], H, W),
                      upsample(Cr, info['hs'], info['vs'], H, W))
