// JPEG decoding on the device: the camera files of the reference dataset (dataset/nusc_mv_det_dataset.py:510 Image.open,
// :617 np.array(img)) -> uint8 RGB frames, byte for byte libjpeg-turbo's default decode as Pillow runs it.
//
// Host: sgv3d_jpeg_parse walks the markers and fills one fixed-size descriptor per frame (sampling, MCU grid, restart
// interval, quantisation tables in natural order, Huffman tables in libjpeg's derived form, the entropy-coded segment).
//
// Device, eight launches per batch whatever its size and content (grids follow the byte capacity and the frame size):
//   Z  zero     the coefficient blocks of every frame (the entropy decode writes only the coefficients it meets).
//   A  spec     every scan is cut into subsequences of seq_bytes bytes; subsequence j is decoded from a guessed state
//               g_j = (its first bit, block 0 of an MCU, coefficient 0) to its exit: the first codeword boundary at or
//               past its end.  A state is (raw bit offset, block index within the MCU, coefficient index); the bit
//               offset alone is not enough, luma blocks share tables.  g_0 is the true start.
//   B  sync     thread j continues from exit_j through j+1, j+2, ... until its state at the end of subsequence m equals
//               exit_m: from there on path(g_j) and path(g_m) are one path.  sync(j) = m, and the DC codes met on the
//               way are counted.  Bounded by the scan: the worst case is one continuation over the rest of it.
//   C  resolve  one workgroup per frame: the anchors 0, sync(0), sync(sync(0)), ... (pointer doubling, 1024
//               subsequences at a time).  The true path equals path(g_a) from the end of anchor a to the end of
//               sync(a), so the anchors' ranges tile the scan; an exclusive scan of their counts gives each range's
//               first block.  The total must equal the frame's blocks.
//   D  final    each anchor decodes its range again from its resolved state and writes int16 coefficients (DC as the
//               difference) into the blocks from its first block on.
//   E  dc       one workgroup per (frame, component): a segmented prefix sum of the DC differences in decode order,
//               reset at every restart interval.
//   F  idct     dequantise + jidctint.c (JDCT_ISLOW) with its range-limit table, one thread per block -> padded
//               component planes.
//   G  color    jdsample.c's fancy upsampling (h2v1 / h2v2 triangle filters, replicated edges; plain replication for
//               a downsampled width of 1 or 2, as libjpeg-turbo chooses) + jdcolor.c's fixed-point YCbCr -> RGB,
//               written straight into [frames, h, w, 3].
// Errors inside a scan (a bad code, a run past coefficient 63, a marker where no restart is due, a scan that ends
// early) set bits of the frame's status word; every read stays inside the frame's (16-byte padded) scan and every
// write inside its blocks, planes and output, whatever the bytes hold.
#include <string.h>

#include <vector>

#include "common.hpp"

using namespace sgv3d;

static_assert(sizeof(sgv3d_jpeg_huff) == 1424 && sizeof(sgv3d_jpeg_frame) == 8976, "descriptor layout (sgv3d_amd/jpeg.py)");

namespace {

constexpr int kNatural[64 + 16] = {   // zigzag -> natural order (jpeg_natural_order); the tail guards a run past 63
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63, 63, 63,
    63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63, 63};
__constant__ uint8_t dNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------------------------------------------------------ host parser

struct Cursor {
    const uint8_t *d;
    size_t n, p;
    bool has(size_t k) const { return p + k <= n; }
    int u8() { return d[p++]; }
    int u16() {
        const int v = (d[p] << 8) | d[p + 1];
        p += 2;
        return v;
    }
};

// libjpeg's jpeg_make_d_derived_tbl, plus its check that every code fits its length
int derive_huff(const uint8_t bits[17], const uint8_t *vals, int nvals, bool dc, sgv3d_jpeg_huff *t) {
    memset(t, 0, sizeof(*t));
    int size[257], code[257], p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < bits[l]; ++i) size[p++] = l;
    size[p] = 0;
    if (p != nvals || p > 256) return fail(SGV3D_EINVAL, "jpeg_parse: bad Huffman table (%d symbols)", p);
    int c = 0, si = size[0];
    p = 0;
    while (size[p]) {
        while (size[p] == si) code[p++] = c++;
        if (c >= (1 << si)) return fail(SGV3D_EINVAL, "jpeg_parse: bad Huffman table (code overflow at length %d)", si);
        c <<= 1;
        ++si;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (bits[l]) {
            t->valoff[l] = p - code[p];
            p += bits[l];
            t->maxcode[l] = code[p - 1];
        } else {
            t->maxcode[l] = -1;
        }
    }
    t->maxcode[0] = -1;
    t->maxcode[17] = 0xFFFFF;
    for (int i = 0; i < nvals; ++i) {
        t->huffval[i] = vals[i];
        if (dc && vals[i] > 15) return fail(SGV3D_EINVAL, "jpeg_parse: bad Huffman table (DC symbol %d > 15)", vals[i]);
    }
    p = 0;
    for (int l = 1; l <= 9; ++l)
        for (int i = 0; i < bits[l]; ++i, ++p) {
            int lb = code[p] << (9 - l);
            for (int k = 0; k < (1 << (9 - l)); ++k) t->look[lb++] = (uint16_t)((l << 8) | vals[p]);
        }
    return SGV3D_OK;
}

int parse(const uint8_t *data, size_t len, sgv3d_jpeg_frame *f) {
    memset(f, 0, sizeof(*f));
    Cursor c{data, len, 0};
    if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return fail(SGV3D_EINVAL, "jpeg_parse: not a JPEG file (no SOI)");
    c.p = 2;
    sgv3d_jpeg_huff dht[2][4];
    bool have_dht[2][4] = {}, have_dqt[4] = {};
    uint16_t dqt[4][64];
    int comp_id[3] = {}, comp_tq[3] = {}, comp_h[3] = {}, comp_v[3] = {};
    bool have_sof = false, adobe = false, jfif = false;
    int adobe_transform = -1;
    for (;;) {
        // next marker: FF (fill FFs) code
        if (!c.has(2)) return fail(SGV3D_EINVAL, "jpeg_parse: missing SOS (file ends before the scan)");
        if (c.d[c.p] != 0xFF) return fail(SGV3D_EINVAL, "jpeg_parse: bad marker at byte %zu", c.p);
        while (c.has(1) && c.d[c.p] == 0xFF) ++c.p;
        if (!c.has(1)) return fail(SGV3D_EINVAL, "jpeg_parse: missing SOS (file ends before the scan)");
        const int m = c.u8();
        if (m == 0xD9) return fail(SGV3D_EINVAL, "jpeg_parse: missing SOS (EOI before any scan)");
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;   // stray SOI / RSTn / TEM: no length
        if (!c.has(2)) return fail(SGV3D_EINVAL, "jpeg_parse: truncated marker segment");
        const size_t seg = (size_t)c.u16();
        if (seg < 2 || !c.has(seg - 2)) return fail(SGV3D_EINVAL, "jpeg_parse: truncated marker segment 0x%02X", m);
        const size_t end = c.p + seg - 2;
        if (m == 0xC2 || m == 0xC6 || m == 0xCA || m == 0xCE)
            return fail(SGV3D_EINVAL, "jpeg_parse: progressive JPEG is not supported (SOF%d)", m - 0xC0);
        if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF)
            return fail(SGV3D_EINVAL, "jpeg_parse: lossless JPEG is not supported (SOF%d)", m - 0xC0);
        if (m == 0xC5) return fail(SGV3D_EINVAL, "jpeg_parse: hierarchical JPEG is not supported (SOF5)");
        if (m == 0xC9) return fail(SGV3D_EINVAL, "jpeg_parse: arithmetic coding is not supported (SOF9)");
        if (m == 0xCC) return fail(SGV3D_EINVAL, "jpeg_parse: arithmetic coding is not supported (DAC)");
        if (m == 0xC8) return fail(SGV3D_EINVAL, "jpeg_parse: reserved SOF marker JPG");
        if (m == 0xDC) return fail(SGV3D_EINVAL, "jpeg_parse: DNL is not supported");
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof) return fail(SGV3D_EINVAL, "jpeg_parse: more than one frame header");
            if (seg < 8) return fail(SGV3D_EINVAL, "jpeg_parse: truncated SOF");
            const int prec = c.u8();
            if (prec != 8) return fail(SGV3D_EINVAL, "jpeg_parse: %d-bit samples are not supported (8-bit only)", prec);
            f->height = c.u16();
            f->width = c.u16();
            const int nf = c.u8();
            if (f->height == 0 || f->width == 0) return fail(SGV3D_EINVAL, "jpeg_parse: zero image size (DNL) is not supported");
            if (nf != 3) return fail(SGV3D_EINVAL, "jpeg_parse: %d components are not supported (3, YCbCr only)", nf);
            if (seg != 8 + 3 * 3) return fail(SGV3D_EINVAL, "jpeg_parse: bad SOF length");
            for (int i = 0; i < 3; ++i) {
                comp_id[i] = c.u8();
                const int hv = c.u8();
                comp_h[i] = hv >> 4, comp_v[i] = hv & 15;
                comp_tq[i] = c.u8();
                if (comp_tq[i] > 3) return fail(SGV3D_EINVAL, "jpeg_parse: bad quantisation table index");
            }
            const bool s444 = comp_h[0] == 1 && comp_v[0] == 1, s422 = comp_h[0] == 2 && comp_v[0] == 1,
                       s420 = comp_h[0] == 2 && comp_v[0] == 2;
            if (!(s444 || s422 || s420) || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1)
                return fail(SGV3D_EINVAL, "jpeg_parse: sampling factors %dx%d,%dx%d,%dx%d are not supported (4:4:4, "
                            "4:2:2, 4:2:0 only)", comp_h[0], comp_v[0], comp_h[1], comp_v[1], comp_h[2], comp_v[2]);
            if (comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
                return fail(SGV3D_EINVAL, "jpeg_parse: RGB component ids are not supported (YCbCr only)");
            f->hs = comp_h[0], f->vs = comp_v[0];
            have_sof = true;
        } else if (m == 0xC4) {
            while (c.p < end) {
                if (!c.has(17) || c.p + 17 > end) return fail(SGV3D_EINVAL, "jpeg_parse: truncated DHT");
                const int tcth = c.u8(), tc = tcth >> 4, th = tcth & 15;
                if (tc > 1 || th > 3) return fail(SGV3D_EINVAL, "jpeg_parse: bad DHT class / index");
                uint8_t bits[17] = {};
                int nv = 0;
                for (int l = 1; l <= 16; ++l) nv += bits[l] = (uint8_t)c.u8();
                if (nv > 256 || c.p + nv > end) return fail(SGV3D_EINVAL, "jpeg_parse: bad Huffman table (%d symbols)", nv);
                const int rc = derive_huff(bits, c.d + c.p, nv, tc == 0, &dht[tc][th]);
                if (rc) return rc;
                c.p += nv;
                have_dht[tc][th] = true;
            }
        } else if (m == 0xDB) {
            while (c.p < end) {
                const int pqtq = c.u8(), pq = pqtq >> 4, tq = pqtq & 15;
                if (pq > 1 || tq > 3) return fail(SGV3D_EINVAL, "jpeg_parse: bad DQT precision / index");
                if (c.p + 64 * (pq + 1) > end) return fail(SGV3D_EINVAL, "jpeg_parse: truncated DQT");
                for (int k = 0; k < 64; ++k) dqt[tq][kNatural[k]] = (uint16_t)(pq ? c.u16() : c.u8());
                have_dqt[tq] = true;
            }
        } else if (m == 0xDD) {
            if (seg != 4) return fail(SGV3D_EINVAL, "jpeg_parse: bad DRI length");
            f->restart = c.u16();
        } else if (m == 0xE0) {
            jfif = seg >= 7 && memcmp(c.d + c.p, "JFIF\0", 5) == 0;
        } else if (m == 0xEE) {
            if (seg >= 14 && memcmp(c.d + c.p, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = c.d[c.p + 11];
            }
        } else if (m == 0xDA) {
            if (!have_sof) return fail(SGV3D_EINVAL, "jpeg_parse: SOS before the frame header");
            if (adobe && adobe_transform != 1)
                return fail(SGV3D_EINVAL, "jpeg_parse: Adobe transform %d is not supported (YCbCr, transform 1, only)",
                            adobe_transform);
            (void)jfif;
            const int ns = c.u8();
            if (ns != 3) return fail(SGV3D_EINVAL, "jpeg_parse: a scan of %d components: more than one scan is not "
                                     "supported (one interleaved scan only)", ns);
            if (seg != 6 + 2 * 3) return fail(SGV3D_EINVAL, "jpeg_parse: bad SOS length");
            for (int i = 0; i < 3; ++i) {
                const int id = c.u8(), tt = c.u8(), td = tt >> 4, ta = tt & 15;
                if (id != comp_id[i]) return fail(SGV3D_EINVAL, "jpeg_parse: scan components out of frame order");
                if (td > 3 || ta > 3 || !have_dht[0][td] || !have_dht[1][ta])
                    return fail(SGV3D_EINVAL, "jpeg_parse: scan uses an undefined Huffman table");
                if (!have_dqt[comp_tq[i]]) return fail(SGV3D_EINVAL, "jpeg_parse: undefined quantisation table");
                f->huff[i][0] = dht[0][td];
                f->huff[i][1] = dht[1][ta];
                memcpy(f->quant[i], dqt[comp_tq[i]], sizeof(f->quant[i]));
            }
            const int ss = c.u8(), se = c.u8(), ahal = c.u8();
            if (ss != 0 || se != 63 || ahal != 0)
                return fail(SGV3D_EINVAL, "jpeg_parse: spectral selection / approximation (progressive) is not supported");
            // the entropy-coded segment runs to the first marker that is not RSTn (FF 00 is a stuffed FF)
            const size_t s0 = c.p;
            size_t q = s0;
            for (;;) {
                const void *ff = memchr(c.d + q, 0xFF, len - q);
                if (!ff) return fail(SGV3D_EINVAL, "jpeg_parse: missing EOI (file ends inside the scan)");
                q = (size_t)(static_cast<const uint8_t *>(ff) - c.d);
                size_t r = q + 1;
                while (r < len && c.d[r] == 0xFF) ++r;   // fill bytes
                if (r >= len) return fail(SGV3D_EINVAL, "jpeg_parse: missing EOI (file ends inside the scan)");
                const int code = c.d[r];
                if (code == 0x00 || (code >= 0xD0 && code <= 0xD7)) {
                    q = r + 1;
                    continue;
                }
                if (code == 0xD9) break;
                if (code == 0xC4 || code == 0xDA || code == 0xDB || code == 0xDD)
                    return fail(SGV3D_EINVAL, "jpeg_parse: more than one scan is not supported (marker 0x%02X after "
                                "the first)", code);
                return fail(SGV3D_EINVAL, "jpeg_parse: missing EOI (marker 0x%02X ends the scan)", code);
            }
            if (q - s0 > 0x7FFFFFF0u / 8) return fail(SGV3D_EINVAL, "jpeg_parse: scan of %zu bytes too large", q - s0);
            f->scan_off = (int64_t)s0;
            f->scan_len = (int32_t)(q - s0);
            if (f->scan_len == 0) return fail(SGV3D_EINVAL, "jpeg_parse: empty scan");
            f->mcux = (f->width + 8 * f->hs - 1) / (8 * f->hs);
            f->mcuy = (f->height + 8 * f->vs - 1) / (8 * f->vs);
            f->blocks_per_mcu = f->hs * f->vs + 2;
            return SGV3D_OK;
        }
        // APPn, COM and every other segment with a length: skipped
        c.p = end;
    }
}

// ------------------------------------------------------------------------------------------------ device decode

constexpr int kBlk = 256;         // threads of the subsequence kernels
constexpr int kResolve = 1024;    // threads of the resolve / dc kernels (one workgroup per frame / component)
constexpr int kLevels = 10;       // pointer doubling levels: 2^10 = kResolve hops
constexpr int kDcRun = 16;        // DC differences per thread and chunk

struct Layout {
    int nsub_cap, blk_cap;
    size_t ycap, ccap;
    size_t exits, ints, coef, planes, total;   // byte offsets of each region
};

int max_blocks(int h, int w) {
    const int a = ((h + 7) / 8) * ((w + 7) / 8) * 3;          // 4:4:4
    const int b = ((h + 7) / 8) * ((w + 15) / 16) * 4;        // 4:2:2
    const int c = ((h + 15) / 16) * ((w + 15) / 16) * 6;      // 4:2:0
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

Layout layout(int frames, int h, int w, int max_bytes, int seq_bytes) {
    Layout L{};
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    L.nsub_cap = (int)(((long long)max_bytes + seq_bytes - 1) / seq_bytes);
    L.blk_cap = max_blocks(h, w);
    L.ycap = (size_t)((h + 15) / 16 * 16) * ((w + 15) / 16 * 16);
    L.ccap = (size_t)((h + 7) / 8 * 8) * ((w + 7) / 8 * 8);
    L.exits = 0;
    L.ints = up((size_t)frames * L.nsub_cap * 8);
    L.coef = L.ints + up((size_t)frames * L.nsub_cap * 4 * 4);
    L.planes = L.coef + up((size_t)frames * L.blk_cap * 128);
    L.total = L.planes + up((size_t)frames * (L.ycap + 2 * L.ccap));
    return L;
}

struct Args {
    const sgv3d_jpeg_frame *fr;
    const uint8_t *data;
    int32_t *status;
    unsigned long long *exits;   // [frames][nsub_cap] exit state of each subsequence's speculative decode
    int32_t *cnt;                // [frames][nsub_cap] DC codes of the speculative decode
    int32_t *sync;               // [frames][nsub_cap]
    int32_t *rcnt;               // [frames][nsub_cap] DC codes of the continuation range
    int32_t *base;               // [frames][nsub_cap] first block of an anchor's range, -1: not an anchor
    int16_t *coef;               // [frames][blk_cap][64]
    uint8_t *planes;             // [frames][ycap + 2 ccap]
    uint8_t *dst;                // [frames][h][w][3]
    int nsub_cap, seq_bytes, blk_cap, h, w;
    size_t ycap, ccap;
};

// a decoder state: raw bit offset in the scan, block index within the MCU, coefficient index (0: DC next)
__device__ inline unsigned long long pack(int pos, int b, int k) {
    return ((unsigned long long)(unsigned)pos << 32) | (unsigned)(b << 8 | k);
}

struct Dec {
    const uint8_t *d;             // the frame's scan
    int len, bits;                // bytes; bits = 8 len = the END position
    int lumab, bpm, restart;      // luma blocks per MCU, blocks per MCU, restart interval
    const sgv3d_jpeg_huff *h;     // LDS copy of the frame's six tables
    int pos, b, k;
    int err;
    int cb;                            // the scan bytes [cb, cb + 32) held in q0..q3 (cb a multiple of 8)
    unsigned long long q0, q1, q2, q3;
};

__device__ inline unsigned long long dword_at(const Dec &s, int byte) {   // aligned 8 bytes of the scan, 0 past its end
    return byte < s.len ? *reinterpret_cast<const unsigned long long *>(s.d + byte) : 0ull;
}

// the 16 scan bytes from byte0 (little-endian in lo, hi).  A step's position depends on the previous step, so a load
// per step would put one memory round trip on every codeword of the serial chain: the window is reloaded only when
// byte0 .. byte0 + 12 leave it (every 12 to 20 bytes).
__device__ __forceinline__ void window(Dec &s, int byte0, unsigned long long &lo, unsigned long long &hi) {
    if (byte0 < s.cb || byte0 + 13 > s.cb + 32) {
        s.cb = byte0 & ~7;
        s.q0 = dword_at(s, s.cb);
        s.q1 = dword_at(s, s.cb + 8);
        s.q2 = dword_at(s, s.cb + 16);
        s.q3 = dword_at(s, s.cb + 24);
    }
    const int off = byte0 - s.cb, wi = off >> 3, sub = (off & 7) * 8;
    const unsigned long long q0 = s.q0, q1 = s.q1, q2 = s.q2, q3 = s.q3;   // (selects on values, not on members)
    const unsigned long long a = wi == 0 ? q0 : (wi == 1 ? q1 : q2);
    const unsigned long long b = wi == 0 ? q1 : (wi == 1 ? q2 : q3);
    const unsigned long long c = wi == 0 ? q2 : q3;
    lo = sub ? (a >> sub) | (b << (64 - sub)) : a;
    hi = sub ? (b >> sub) | (c << (64 - sub)) : b;
}

// the byte after `m` (a marker's FF at raw byte m, or m >= len): after fill bytes, RSTn -> the state after it; anything
// else, or the end of the scan -> END
__device__ __forceinline__ void take_marker(Dec &s, int m) {
    while (m + 1 < s.len && s.d[m + 1] == 0xFF) ++m;
    if (m < s.len && m + 1 < s.len && (s.d[m + 1] & 0xF8) == 0xD0) {
        s.pos = (m + 2) * 8;
    } else {
        s.pos = s.bits;
    }
    s.b = 0;
    s.k = 0;
}

// One transition: a restart marker (with its 1-bit padding) or the end, else one Huffman code with its extra bits.
// Returns kDC when a DC code was decoded, kRST when a restart marker was taken; the coefficient met (zig-zag index,
// value) goes to *kz / *v (*kz = -1: none).
constexpr int kDC = 1, kRST = 2;
__device__ __forceinline__ int step(Dec &s, int *kz, int *v) {
    *kz = -1;
    const int byte0 = s.pos >> 3, sh = s.pos & 7;
    const int o = 0;
    unsigned long long lo, hi;
    window(s, byte0, lo, hi);
    auto wbyte = [&](int i) -> unsigned {   // byte i (0..15) of the 16-byte window
        return (unsigned)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFF);
    };
    // up to five destuffed bytes from byte0; mk = index of the first that is a marker or past the scan
    unsigned long long acc = 0;
    int r = 0, mk = 5;
    unsigned skip = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        unsigned val = 0;
        if (mk == 5) {
            if (byte0 + r >= s.len) {
                mk = t;
            } else {
                const unsigned bv = wbyte(o + r);
                if (bv != 0xFF) {
                    val = bv;
                    r += 1;
                } else if (byte0 + r + 1 < s.len && wbyte(o + r + 1) == 0) {
                    val = 0xFF;
                    r += 2;
                    skip |= 1u << t;
                } else {
                    mk = t;
                }
            }
        }
        acc = (acc << 8) | val;
    }
    // a marker right here, or after 1-bits to the byte boundary: restart (or end)
    const int q = sh ? 1 : 0;
    const unsigned ones = (1u << (8 - sh)) - 1;
    if (mk == q && (sh == 0 || ((unsigned)(acc >> 32) & ones) == ones)) {
        if (s.b != 0 || s.k != 0) s.err |= SGV3D_JPEG_EMARKER;
        take_marker(s, byte0 + (q ? 1 + (int)(skip & 1) : 0));
        return s.pos < s.bits ? kRST : 0;
    }
    const unsigned peek = (unsigned)((acc << (24 + sh)) >> 32);
    const int comp = s.b < s.lumab ? 0 : s.b - s.lumab + 1;
    const sgv3d_jpeg_huff &t = s.h[comp * 2 + (s.k ? 1 : 0)];
    const unsigned lk = t.look[peek >> 23];
    int len, sym;
    if (lk) {
        len = (int)(lk >> 8);
        sym = (int)(lk & 255);
    } else {
        len = 0;
        sym = 0;
        for (int l = 10; l <= 16; ++l) {
            const int code = (int)(peek >> (32 - l));
            if (code <= t.maxcode[l]) {
                len = l;
                sym = t.huffval[(code + t.valoff[l]) & 255];
                break;
            }
        }
        if (!len) {
            s.err |= SGV3D_JPEG_EBADCODE;
            len = 16;
        }
    }
    const int ns = sym & 15;   // (DC categories above 15 are rejected by the parser)
    const int n = len + ns;
    if (sh + n > 8 * mk) {   // the code runs into a marker or past the scan
        s.err |= SGV3D_JPEG_ESHORT;
        take_marker(s, byte0 + mk + __popc(skip & ((1u << mk) - 1)));
        return 0;
    }
    int val = 0;
    if (ns) {
        val = (int)((peek << len) >> (32 - ns));
        if (val < (1 << (ns - 1))) val += 1 - (1 << ns);
    }
    const int o2 = sh + n, j = o2 >> 3;
    s.pos = (byte0 + j + __popc(skip & ((1u << j) - 1))) * 8 + (o2 & 7);
    int dc = 0;
    if (s.k == 0) {
        *kz = 0;
        *v = val;
        s.k = 1;
        dc = kDC;
    } else {
        const int run = sym >> 4;
        if (ns == 0) {
            if (run == 15) {
                s.k += 16;
            } else {
                s.k = 64;
            }
            if (s.k > 64) {
                s.err |= SGV3D_JPEG_ECOEF;
                s.k = 64;
            }
        } else {
            s.k += run;
            if (s.k > 63) {
                s.err |= SGV3D_JPEG_ECOEF;
                s.k = 64;
            } else {
                *kz = s.k;
                *v = val;
                s.k += 1;
            }
        }
    }
    if (s.k == 64) {
        s.k = 0;
        if (++s.b == s.bpm) s.b = 0;
    }
    return dc;
}

// decode from the current state while pos < end (and not at END); returns the DC codes met
__device__ __forceinline__ int run_to(Dec &s, int end) {
    int n = 0, kz, v;
    while (s.pos < end && s.pos < s.bits) n += step(s, &kz, &v) & kDC;
    return n;
}

__device__ inline void load_tables(const sgv3d_jpeg_frame &f, sgv3d_jpeg_huff *lds) {
    const unsigned *src = reinterpret_cast<const unsigned *>(&f.huff[0][0]);
    unsigned *dst = reinterpret_cast<unsigned *>(lds);
    for (int i = threadIdx.x; i < (int)(sizeof(f.huff) / 4); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

__device__ inline Dec make_dec(const Args &a, const sgv3d_jpeg_frame &f, const sgv3d_jpeg_huff *tabs) {
    Dec s;
    s.d = a.data + f.scan_off;
    s.len = f.scan_len;
    s.bits = f.scan_len * 8;
    s.lumab = f.hs * f.vs;
    s.bpm = f.blocks_per_mcu;
    s.restart = f.restart;
    s.h = tabs;
    s.pos = 0, s.b = 0, s.k = 0, s.err = 0;
    s.cb = -64;
    s.q0 = s.q1 = s.q2 = s.q3 = 0;
    return s;
}

__device__ inline void set_state(Dec &s, unsigned long long st) {
    s.pos = (int)(st >> 32);
    s.b = (int)((st >> 8) & 0xFF);
    s.k = (int)(st & 0xFF);
}

// Z: zero the frame's coefficient blocks (16 bytes per thread); also clears the status word
__global__ __launch_bounds__(kBlk) void jpeg_zero_kernel(Args a) {
    const int f = blockIdx.y;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    const long long nb = (long long)fr.mcux * fr.mcuy * fr.blocks_per_mcu;
    const long long i = (long long)blockIdx.x * kBlk + threadIdx.x;
    if (i == 0) a.status[f] = 0;
    if (i >= nb * 8) return;
    reinterpret_cast<int4 *>(a.coef + (size_t)f * a.blk_cap * 64)[i] = make_int4(0, 0, 0, 0);
}

// A: speculative decode of every subsequence from its guessed state
__global__ __launch_bounds__(kBlk) void jpeg_spec_kernel(Args a) {
    __shared__ sgv3d_jpeg_huff tabs[6];
    const int f = blockIdx.y;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    load_tables(fr, tabs);
    const int j = blockIdx.x * kBlk + threadIdx.x;
    const int nsub = (fr.scan_len + a.seq_bytes - 1) / a.seq_bytes;
    if (j >= nsub) return;
    Dec s = make_dec(a, fr, tabs);
    int start = j * a.seq_bytes;
    if (j > 0 && s.d[start] == 0 && s.d[start - 1] == 0xFF) ++start;   // (a guess never starts on a stuffed zero)
    s.pos = start * 8;
    const int end = (int)min((long long)(j + 1) * a.seq_bytes, (long long)fr.scan_len) * 8;
    const int n = run_to(s, end);
    const size_t o = (size_t)f * a.nsub_cap + j;
    a.exits[o] = pack(s.pos, s.b, s.k);
    a.cnt[o] = n;
}

// B: continuation of path(g_j) until it meets the speculative path of a later subsequence
__global__ __launch_bounds__(kBlk) void jpeg_sync_kernel(Args a) {
    __shared__ sgv3d_jpeg_huff tabs[6];
    const int f = blockIdx.y;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    load_tables(fr, tabs);
    const int j = blockIdx.x * kBlk + threadIdx.x;
    const int nsub = (fr.scan_len + a.seq_bytes - 1) / a.seq_bytes;
    if (j >= nsub) return;
    const size_t o = (size_t)f * a.nsub_cap;
    Dec s = make_dec(a, fr, tabs);
    set_state(s, a.exits[o + j]);
    int n = j == 0 ? a.cnt[o] : 0;
    int m = j + 1;
    for (; m < nsub; ++m) {
        const int end = (int)min((long long)(m + 1) * a.seq_bytes, (long long)fr.scan_len) * 8;
        n += run_to(s, end);
        if (pack(s.pos, s.b, s.k) == a.exits[o + m]) break;
    }
    a.sync[o + j] = m;   // nsub: the range runs to the end of the scan
    a.rcnt[o + j] = n;
}

// C: the anchors 0 -> sync(0) -> ..., and the first block of each anchor's range
__global__ __launch_bounds__(kResolve) void jpeg_resolve_kernel(Args a) {
    __shared__ short jmp[kLevels][kResolve];
    __shared__ unsigned char on[kResolve];
    __shared__ int part[kResolve / kWave];
    __shared__ int sh_last;
    const int f = blockIdx.x, tid = threadIdx.x;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    const int nsub = (fr.scan_len + a.seq_bytes - 1) / a.seq_bytes;
    const size_t o = (size_t)f * a.nsub_cap;
    int p = 0;                 // the first anchor at or after this chunk
    long long carry = 0;       // blocks of the ranges before this chunk
    for (int c0 = 0; c0 < nsub; c0 += kResolve) {
        const int j = c0 + tid;
        const int nx = j < nsub ? a.sync[o + j] : 0x7FFFFFFF;
        jmp[0][tid] = (short)(nx - c0 < kResolve ? nx - c0 : -1);
        on[tid] = (j == p);
        if (tid == 0) sh_last = -1;
        __syncthreads();
        for (int r = 1; r < kLevels; ++r) {
            const int t = jmp[r - 1][tid];
            jmp[r][tid] = t < 0 ? (short)-1 : jmp[r - 1][t];
            __syncthreads();
        }
        for (int r = kLevels - 1; r >= 0; --r) {
            const int t = jmp[r][tid];
            const bool mark = on[tid] && t >= 0;
            __syncthreads();
            if (mark) on[t] = 1;
            __syncthreads();
        }
        const bool anchor = on[tid] && j < nsub;
        if (anchor) atomicMax(&sh_last, tid);
        // exclusive scan of the anchors' counts
        int v = anchor ? a.rcnt[o + j] : 0;
        const int lane = tid & (kWave - 1), wv = tid / kWave;
        int incl = v;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int u = __shfl_up(incl, d, kWave);
            if (lane >= d) incl += u;
        }
        if (lane == kWave - 1) part[wv] = incl;
        __syncthreads();
        int before = 0;
        for (int i = 0; i < wv; ++i) before += part[i];
        if (j < nsub) a.base[o + j] = anchor ? (int)(carry + before + incl - v) : -1;
        int tot = 0;
        for (int i = 0; i < kResolve / kWave; ++i) tot += part[i];
        carry += tot;
        const int last = sh_last;
        if (last >= 0) p = a.sync[o + c0 + last];
        __syncthreads();
    }
    if (tid == 0) {
        const long long nb = (long long)fr.mcux * fr.mcuy * fr.blocks_per_mcu;
        if (carry < nb) atomicOr(a.status + f, SGV3D_JPEG_ESHORT);
        if (carry > nb) atomicOr(a.status + f, SGV3D_JPEG_ELONG);
    }
}

// D: each anchor decodes its range from its resolved state and writes the coefficients
__global__ __launch_bounds__(kBlk) void jpeg_final_kernel(Args a) {
    __shared__ sgv3d_jpeg_huff tabs[6];
    const int f = blockIdx.y;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    load_tables(fr, tabs);
    const int j = blockIdx.x * kBlk + threadIdx.x;
    const int nsub = (fr.scan_len + a.seq_bytes - 1) / a.seq_bytes;
    if (j >= nsub) return;
    const size_t o = (size_t)f * a.nsub_cap;
    const int base = a.base[o + j];
    if (base < 0) return;
    Dec s = make_dec(a, fr, tabs);
    if (j > 0) set_state(s, a.exits[o + j]);
    const int last = a.sync[o + j];
    const int end = last >= nsub ? s.bits : (int)min((long long)(last + 1) * a.seq_bytes, (long long)fr.scan_len) * 8;
    const long long nb = (long long)fr.mcux * fr.mcuy * fr.blocks_per_mcu;
    const long long interval = (long long)fr.restart * fr.blocks_per_mcu;
    int16_t *coef = a.coef + (size_t)f * a.blk_cap * 64;
    long long idx = (long long)base - 1;   // the block being filled (a range may start inside one)
    while (s.pos < end && s.pos < s.bits) {
        int kz, v = 0;
        const int fl = step(s, &kz, &v);
        idx += fl & kDC;
        if ((fl & kRST) && (interval == 0 || (idx + 1) % interval != 0)) s.err |= SGV3D_JPEG_EMARKER;   // (not at an interval end)
        if (kz >= 0) {
            if (idx >= 0 && idx < nb) {
                coef[(size_t)idx * 64 + dNatural[kz]] = (int16_t)v;
            } else {
                s.err |= SGV3D_JPEG_ELONG;
            }
        }
    }
    if (s.err) atomicOr(a.status + f, s.err);
}

// E: DC prediction: segmented prefix sum per (frame, component) in decode order, reset at each restart interval
__global__ __launch_bounds__(kResolve) void jpeg_dc_kernel(Args a) {
    __shared__ int pf[kResolve], pv[kResolve];
    const int comp = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    const int per = comp == 0 ? fr.hs * fr.vs : 1;
    const int off = comp == 0 ? 0 : fr.hs * fr.vs + comp - 1;
    const long long mcus = (long long)fr.mcux * fr.mcuy;
    const long long n = mcus * per;
    int16_t *coef = a.coef + (size_t)f * a.blk_cap * 64;
    auto blk = [&](long long e) { return (e / per) * fr.blocks_per_mcu + off + e % per; };
    auto starts = [&](long long e) {   // a new DC predictor: the first block of the component in a restart interval
        return e == 0 || (fr.restart > 0 && e % per == 0 && (e / per) % fr.restart == 0);
    };
    int carry = 0;
    for (long long c0 = 0; c0 < n; c0 += (long long)kResolve * kDcRun) {
        const long long e0 = c0 + (long long)tid * kDcRun;
        int fl = 0, sum = 0;
        for (int i = 0; i < kDcRun && e0 + i < n; ++i) {
            if (starts(e0 + i)) {
                fl = 1;
                sum = 0;
            }
            sum += coef[(size_t)blk(e0 + i) * 64];
        }
        // inclusive segmented scan of (flag, sum) over the workgroup
        pf[tid] = fl;
        pv[tid] = sum;
        __syncthreads();
        for (int d = 1; d < kResolve; d <<= 1) {
            int f2 = 0, v2 = 0;
            const bool has = tid >= d;
            if (has) f2 = pf[tid - d], v2 = pv[tid - d];
            __syncthreads();
            if (has) {
                if (!pf[tid]) pv[tid] += v2;
                pf[tid] |= f2;
            }
            __syncthreads();
        }
        int run = carry;   // the predictor entering this thread's run
        if (tid > 0) run = pf[tid - 1] ? pv[tid - 1] : carry + pv[tid - 1];
        for (int i = 0; i < kDcRun && e0 + i < n; ++i) {
            if (starts(e0 + i)) run = 0;
            int16_t *p = coef + (size_t)blk(e0 + i) * 64;
            run += *p;
            *p = (int16_t)run;
        }
        const int lf = pf[kResolve - 1], lv = pv[kResolve - 1];
        carry = lf ? lv : carry + lv;
        __syncthreads();
    }
}

// F: dequantise + jidctint.c, one thread per block
constexpr int kCB = 13, kP1 = 2;
__device__ inline long long descale(long long x, int n) { return (x + (1ll << (n - 1))) >> n; }
__device__ inline unsigned char range_limit(long long x) {   // range_limit[x & RANGE_MASK] of the post-IDCT table
    const int w = (int)(((x + 512) & 1023) - 512) + 128;
    return (unsigned char)(w < 0 ? 0 : (w > 255 ? 255 : w));
}

// one 1-D pass of jidctint.c on eight values (JLONG arithmetic); results not yet descaled
__device__ inline void idct_1d(long long i0, long long i1, long long i2, long long i3, long long i4, long long i5,
                               long long i6, long long i7, long long r[8]) {
    long long z1 = (i2 + i6) * 4433;   // FIX_0_541196100
    long long tmp2 = z1 + i6 * -15137; // FIX_1_847759065
    long long tmp3 = z1 + i2 * 6270;   // FIX_0_765366865
    long long tmp0 = (i0 + i4) << kCB;
    long long tmp1 = (i0 - i4) << kCB;
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = i7;
    tmp1 = i5;
    tmp2 = i3;
    tmp3 = i1;
    z1 = tmp0 + tmp3;
    long long z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * 9633;   // FIX_1_175875602
    tmp0 *= 2446;                            // FIX_0_298631336
    tmp1 *= 16819;                           // FIX_2_053119869
    tmp2 *= 25172;                           // FIX_3_072711026
    tmp3 *= 12299;                           // FIX_1_501321110
    z1 *= -7373;                             // FIX_0_899976223
    z2 *= -20995;                            // FIX_2_562915447
    z3 *= -16069;                            // FIX_1_961570560
    z4 *= -3196;                             // FIX_0_390180644
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    r[0] = tmp10 + tmp3, r[7] = tmp10 - tmp3;
    r[1] = tmp11 + tmp2, r[6] = tmp11 - tmp2;
    r[2] = tmp12 + tmp1, r[5] = tmp12 - tmp1;
    r[3] = tmp13 + tmp0, r[4] = tmp13 - tmp0;
}

__global__ __launch_bounds__(kBlk) void jpeg_idct_kernel(Args a) {
    __shared__ unsigned short q[3][64];
    const int f = blockIdx.y;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    for (int i = threadIdx.x; i < 3 * 64; i += kBlk) q[i / 64][i % 64] = fr.quant[i / 64][i % 64];
    __syncthreads();
    const long long nb = (long long)fr.mcux * fr.mcuy * fr.blocks_per_mcu;
    const long long bi = (long long)blockIdx.x * kBlk + threadIdx.x;
    if (bi >= nb) return;
    const int bpm = fr.blocks_per_mcu, lumab = fr.hs * fr.vs;
    const int mcu = (int)(bi / bpm), u = (int)(bi % bpm);
    const int mx = mcu % fr.mcux, my = mcu / fr.mcux;
    int comp, bx, by, pitch;
    size_t plane;
    if (u < lumab) {
        comp = 0;
        bx = mx * fr.hs + u % fr.hs;
        by = my * fr.vs + u / fr.hs;
        pitch = fr.mcux * 8 * fr.hs;
        plane = 0;
    } else {
        comp = u - lumab + 1;
        bx = mx;
        by = my;
        pitch = fr.mcux * 8;
        plane = a.ycap + (comp - 1) * a.ccap;
    }
    int in[64];   // DEQUANTIZE: coefficient x quantisation value (ISLOW_MULT_TYPE, int)
    const int4 *c4 = reinterpret_cast<const int4 *>(a.coef + ((size_t)f * a.blk_cap + bi) * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int4 v = c4[i];
        const int w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            in[i * 8 + 2 * t] = (int)(int16_t)(w4[t] & 0xFFFF) * (int)q[comp][i * 8 + 2 * t];
            in[i * 8 + 2 * t + 1] = (int)(int16_t)((unsigned)w4[t] >> 16) * (int)q[comp][i * 8 + 2 * t + 1];
        }
    }
    int ws[64];   // jidctint.c's int workspace
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        long long r[8];
        idct_1d(in[c], in[8 + c], in[16 + c], in[24 + c], in[32 + c], in[40 + c], in[48 + c], in[56 + c], r);
#pragma unroll
        for (int i = 0; i < 8; ++i) ws[i * 8 + c] = (int)descale(r[i], kCB - kP1);
    }
    uint8_t *dst = a.planes + (size_t)f * (a.ycap + 2 * a.ccap) + plane + (size_t)by * 8 * pitch + bx * 8;
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        const int *w = ws + row * 8;
        long long r[8];
        idct_1d(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], r);
        unsigned long long w8 = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) w8 |= (unsigned long long)range_limit(descale(r[i], kCB + kP1 + 3)) << (8 * i);
        *reinterpret_cast<unsigned long long *>(dst + (size_t)row * pitch) = w8;
    }
}

// G: fancy upsampling + YCbCr -> RGB, one thread per output pixel
constexpr int kCX = 64, kCY = 4;

__device__ inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ inline int chroma(const uint8_t *p, int pitch, int x, int y, int hs, int vs, int dw, int dh) {
    if (hs == 1) return p[(size_t)y * pitch + x];
    const int cx = x >> 1;
    if (dw <= 2) {   // libjpeg-turbo upsamples by replication when the downsampled width is 1 or 2
        return p[(size_t)(vs == 2 ? y >> 1 : y) * pitch + cx];
    }
    const int xn = (x & 1) ? min(cx + 1, dw - 1) : max(cx - 1, 0);
    if (vs == 1) {
        const uint8_t *row = p + (size_t)y * pitch;
        return (x & 1) ? (3 * row[cx] + row[xn] + 2) >> 2 : (3 * row[cx] + row[xn] + 1) >> 2;
    }
    const int cy = y >> 1;
    const int yn = (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);
    const uint8_t *r0 = p + (size_t)cy * pitch, *r1 = p + (size_t)yn * pitch;
    const int s0 = 3 * r0[cx] + r1[cx], s1 = 3 * r0[xn] + r1[xn];
    return (x & 1) ? (3 * s0 + s1 + 7) >> 4 : (3 * s0 + s1 + 8) >> 4;
}

__global__ __launch_bounds__(kCX *kCY) void jpeg_color_kernel(Args a) {
    const int f = blockIdx.z;
    const sgv3d_jpeg_frame &fr = a.fr[f];
    const int x = blockIdx.x * kCX + threadIdx.x, y = blockIdx.y * kCY + threadIdx.y;
    if (x >= a.w || y >= a.h) return;
    const uint8_t *pl = a.planes + (size_t)f * (a.ycap + 2 * a.ccap);
    const int ypitch = fr.mcux * 8 * fr.hs, cpitch = fr.mcux * 8;
    const int dw = (a.w + fr.hs - 1) / fr.hs, dh = (a.h + fr.vs - 1) / fr.vs;
    const int Y = pl[(size_t)y * ypitch + x];
    const int cb = chroma(pl + a.ycap, cpitch, x, y, fr.hs, fr.vs, dw, dh) - 128;
    const int cr = chroma(pl + a.ycap + a.ccap, cpitch, x, y, fr.hs, fr.vs, dw, dh) - 128;
    // jdcolor.c build_ycc_rgb_table: SCALEBITS 16, FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802,
    // FIX(0.34414) = 22554
    const int rr = (91881 * cr + 32768) >> 16;
    const int bb = (116130 * cb + 32768) >> 16;
    const int gg = (-46802 * cr + (-22554 * cb + 32768)) >> 16;
    uint8_t *o = a.dst + (((size_t)f * a.h + y) * a.w + x) * 3;
    o[0] = (uint8_t)clamp255(Y + rr);
    o[1] = (uint8_t)clamp255(Y + gg);
    o[2] = (uint8_t)clamp255(Y + bb);
}

bool args_ok(int frames, int h, int w, int max_bytes, int seq_bytes) {
    return frames > 0 && frames <= 65535 && h > 0 && h <= 65535 && w > 0 && w <= 65535 && max_bytes > 0 &&
           max_bytes <= (1 << 26) && seq_bytes >= 8 && seq_bytes <= (1 << 20);
}

}  // namespace

extern "C" int sgv3d_jpeg_parse(const uint8_t *data, size_t len, sgv3d_jpeg_frame *desc, int *h, int *w) {
    SGV3D_REQUIRE(data && desc, "jpeg_parse: null pointer");
    const int rc = parse(data, len, desc);
    if (rc) return rc;
    if (h) *h = desc->height;
    if (w) *w = desc->width;
    return SGV3D_OK;
}

extern "C" size_t sgv3d_jpeg_workspace_bytes(int frames, int h, int w, int max_bytes, int seq_bytes) {
    if (!args_ok(frames, h, w, max_bytes, seq_bytes)) return 0;
    return layout(frames, h, w, max_bytes, seq_bytes).total;
}

extern "C" int sgv3d_jpeg_decode(int frames, int h, int w, int max_bytes, int seq_bytes,
                                 const sgv3d_jpeg_frame *frames_host, const sgv3d_jpeg_frame *frames_dev,
                                 const uint8_t *data, long long data_len, int32_t *status, void *work,
                                 size_t work_bytes, uint8_t *dst, void *stream) {
    const char *what = "jpeg_decode";
    SGV3D_REQUIRE(args_ok(frames, h, w, max_bytes, seq_bytes),
                  "%s: bad sizes (frames %d, %dx%d, max_bytes %d (1..2^26), seq_bytes %d (8..2^20))", what, frames, h,
                  w, max_bytes, seq_bytes);
    SGV3D_REQUIRE(frames_host && frames_dev && data && status && dst && work, "%s: null pointer", what);
    SGV3D_REQUIRE((reinterpret_cast<uintptr_t>(data) & 15) == 0 && (reinterpret_cast<uintptr_t>(work) & 15) == 0,
                  "%s: data and work must be 16-byte aligned", what);
    const sgv3d_jpeg_frame &f0 = frames_host[0];
    for (int i = 0; i < frames; ++i) {
        const sgv3d_jpeg_frame &r = frames_host[i];
        SGV3D_REQUIRE(r.width == w && r.height == h, "%s: frame %d is %dx%d, the batch is %dx%d (frames must not differ "
                      "in size)", what, i, r.height, r.width, h, w);
        SGV3D_REQUIRE(r.hs == f0.hs && r.vs == f0.vs, "%s: frame %d has sampling %dx%d, frame 0 %dx%d (frames must not "
                      "differ in sampling)", what, i, r.hs, r.vs, f0.hs, f0.vs);
        SGV3D_REQUIRE((r.hs == 1 && r.vs == 1) || (r.hs == 2 && r.vs == 1) || (r.hs == 2 && r.vs == 2),
                      "%s: frame %d: unsupported sampling %dx%d", what, i, r.hs, r.vs);
        SGV3D_REQUIRE(r.mcux == (w + 8 * r.hs - 1) / (8 * r.hs) && r.mcuy == (h + 8 * r.vs - 1) / (8 * r.vs) &&
                          r.blocks_per_mcu == r.hs * r.vs + 2 && r.restart >= 0,
                      "%s: frame %d: inconsistent MCU grid", what, i);
        SGV3D_REQUIRE(r.scan_len > 0 && r.scan_len <= max_bytes, "%s: frame %d: scan of %d bytes exceeds the decoder's "
                      "capacity of %d bytes", what, i, r.scan_len, max_bytes);
        SGV3D_REQUIRE(r.scan_off >= 0 && (r.scan_off & 15) == 0 &&
                          r.scan_off + ((long long)r.scan_len + 15) / 16 * 16 <= data_len,
                      "%s: frame %d: scan [%lld, +%d) not 16-byte aligned or outside the %lld data bytes", what, i,
                      (long long)r.scan_off, r.scan_len, data_len);
        for (int c = 0; c < 3; ++c)
            for (int t = 0; t < 2; ++t) {
                const sgv3d_jpeg_huff &hf = r.huff[c][t];
                for (int l = 1; l <= 16; ++l)
                    SGV3D_REQUIRE(hf.maxcode[l] < (1 << l) && hf.maxcode[l] >= -1,
                                  "%s: frame %d: malformed Huffman table", what, i);
                for (int e = 0; e < 512; ++e)
                    SGV3D_REQUIRE(hf.look[e] == 0 || ((hf.look[e] >> 8) >= 1 && (hf.look[e] >> 8) <= 9),
                                  "%s: frame %d: malformed Huffman lookup", what, i);
            }
    }
    const Layout L = layout(frames, h, w, max_bytes, seq_bytes);
    if (work_bytes < L.total) return fail(SGV3D_ENOSPACE, "%s: workspace of %zu bytes, need %zu", what, work_bytes, L.total);
    Args a{};
    uint8_t *wk = static_cast<uint8_t *>(work);
    const size_t per = (size_t)frames * L.nsub_cap;
    a.fr = frames_dev;
    a.data = data;
    a.status = status;
    a.exits = reinterpret_cast<unsigned long long *>(wk + L.exits);
    a.cnt = reinterpret_cast<int32_t *>(wk + L.ints);
    a.sync = a.cnt + per;
    a.rcnt = a.sync + per;
    a.base = a.rcnt + per;
    a.coef = reinterpret_cast<int16_t *>(wk + L.coef);
    a.planes = wk + L.planes;
    a.dst = dst;
    a.nsub_cap = L.nsub_cap, a.seq_bytes = seq_bytes, a.blk_cap = L.blk_cap, a.h = h, a.w = w;
    a.ycap = L.ycap, a.ccap = L.ccap;
    hipStream_t st = as_stream(stream);
    const dim3 sub_grid(cdiv(L.nsub_cap, kBlk), frames);
    hipLaunchKernelGGL(jpeg_zero_kernel, dim3(cdiv((long long)L.blk_cap * 8, kBlk), frames), dim3(kBlk), 0, st, a);
    hipLaunchKernelGGL(jpeg_spec_kernel, sub_grid, dim3(kBlk), 0, st, a);
    hipLaunchKernelGGL(jpeg_sync_kernel, sub_grid, dim3(kBlk), 0, st, a);
    hipLaunchKernelGGL(jpeg_resolve_kernel, dim3(frames), dim3(kResolve), 0, st, a);
    hipLaunchKernelGGL(jpeg_final_kernel, sub_grid, dim3(kBlk), 0, st, a);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3, frames), dim3(kResolve), 0, st, a);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv(L.blk_cap, kBlk), frames), dim3(kBlk), 0, st, a);
    hipLaunchKernelGGL(jpeg_color_kernel, dim3(cdiv(w, kCX), cdiv(h, kCY), frames), dim3(kCX, kCY), 0, st, a);
    return check_launch(what);
}
