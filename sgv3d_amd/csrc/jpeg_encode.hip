// JPEG encoding on the device: uint8 RGB frames -> the files Pillow's save(format='JPEG', quality, subsampling,
// restart_marker_blocks) writes (libjpeg-turbo: baseline SOF0, three YCbCr components in one interleaved scan, the
// Annex-K Huffman tables), byte for byte.  DESIGN.md "JPEG encoding" states every rule.
//
// Seven launches on one stream, whatever the batch and the data, no host wait, integer atomics only:
//   transform  colour conversion, edge replication, downsampling, jfdctint, quantisation -> int16 coefficients in
//              zigzag order, one 128-byte row per block in scan order, dummy blocks included (8 lanes per block)
//   size       per block (one wave, one lane per coefficient): DC difference and bit count; clears the bit stream
//   scan       per frame: exclusive sums of the bit counts, every restart interval starting on a byte; capacity test
//   pack       per block: every lane ORs its codes into the unstuffed stream at its bit offset
//   ffcount    FF bytes per 4096-byte chunk of the unstuffed stream
//   layout     per frame: sums of the FF counts, the file length, the capacity test, the file's offset
//   stuff      header, scan with FF 00 stuffing and RSTn markers, EOI
// Every stage is a __host__ __device__ function of one work item; sgv3d_jpeg_encode_host runs the same functions in loops.
#include <string.h>

#include <vector>

#include "common.hpp"
#include "jpeg_std_tables.hpp"

namespace {

using namespace sgv3d;

#define HD __host__ __device__ __forceinline__

constexpr int kChunk = 4096;        // bytes of the unstuffed stream per workgroup of ffcount / stuff (16 per lane)
constexpr int kScanThreads = 1024;  // one workgroup per frame in scan
constexpr int kMaxFrames = 4096;
constexpr int kMaxBytes = 1 << 26;

struct Geo {
    int h, w, hs, vs;
    int mcux, mcuy, bpm, nlum;  // MCU grid, blocks per MCU, luma blocks per MCU
    int wb, hb;                 // real luma block columns / rows: ceil(w / 8), ceil(h / 8)
    int ch;                     // chroma rows that are downsampled from the image: ceil(h / vs)
    int restart, nint;          // restart interval in MCUs (0: none), number of intervals
    int nblk;                   // blocks per frame in scan order
    int hdr;                    // header bytes
    int max_bytes, ucap, chunks;
};

struct QTab {
    uint16_t q[2][64];  // luma, chroma in natural order
};

struct Header {
    uint8_t b[SGV3D_JPEG_ENC_HEADER_MAX];
};

// ------------------------------------------------------------------------------------------------ tables
#define ZIGZAG_POS                                                                                                         \
    {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53, \
     10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63}
const uint8_t h_zigpos[64] = ZIGZAG_POS;  // natural index -> position in zigzag order
__device__ const uint8_t d_zigpos[64] = ZIGZAG_POS;
[[maybe_unused]] const uint32_t h_enc_dc[2][12] = {SGV3D_JPEG_K_ENC_DC_LUMA, SGV3D_JPEG_K_ENC_DC_CHROMA};
[[maybe_unused]] __device__ const uint32_t d_enc_dc[2][12] = {SGV3D_JPEG_K_ENC_DC_LUMA, SGV3D_JPEG_K_ENC_DC_CHROMA};
[[maybe_unused]] const uint32_t h_enc_ac[2][256] = {SGV3D_JPEG_K_ENC_AC_LUMA, SGV3D_JPEG_K_ENC_AC_CHROMA};
[[maybe_unused]] __device__ const uint32_t d_enc_ac[2][256] = {SGV3D_JPEG_K_ENC_AC_LUMA, SGV3D_JPEG_K_ENC_AC_CHROMA};

#ifdef __HIP_DEVICE_COMPILE__
#define TABLE(name) d_##name
#else
#define TABLE(name) h_##name
#endif

// ------------------------------------------------------------------------------------------------ geometry
HD int first_of_interval(const Geo &g, int blk) {
    if (blk % g.bpm) return 0;
    const int mcu = blk / g.bpm;
    return g.restart ? mcu % g.restart == 0 : mcu == 0;
}

// Block `blk` of the scan -> its component, the block of the component's plane it is transformed from, and whether it is
// a dummy block (AC zero, DC of the block libjpeg copies it from: the block before it in a real block row, the last block
// of the MCU's previous block row below the image; either is a real block of the MCU's first column / row).
HD void resolve(const Geo &g, int blk, int &comp, int &bx, int &by, bool &dummy) {
    const int mcu = blk / g.bpm, b = blk % g.bpm, mx = mcu % g.mcux, my = mcu / g.mcux;
    dummy = false;
    if (b >= g.nlum) {
        comp = b - g.nlum + 1;
        bx = mx;
        by = my;
        return;
    }
    comp = 0;
    bx = mx * g.hs + b % g.hs;
    by = my * g.vs + b / g.hs;
    if (by >= g.hb) {
        dummy = true;
        by = my * g.vs;
        bx = mx * g.hs + g.hs - 1;
    }
    if (bx >= g.wb) {
        dummy = true;
        bx = mx * g.hs;
    }
}

// The block whose DC is the predictor of blk's, -1 where the predictor is 0 (start of the scan or of a restart interval).
HD int dc_predecessor(const Geo &g, int blk) {
    const int mcu = blk / g.bpm, b = blk % g.bpm;
    if (b > 0 && b < g.nlum) return blk - 1;
    if (g.restart ? mcu % g.restart == 0 : mcu == 0) return -1;
    return b == 0 ? blk - g.bpm + g.nlum - 1 : blk - g.bpm;
}

// ------------------------------------------------------------------------------------------------ transform
HD int ycc(int comp, const uint8_t *p) {
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Row r of block (bx, by) of a component's plane, level shifted: jccolor, the edge rules and jcsample in one.
HD void load_row(const uint8_t *img, const Geo &g, int comp, int bx, int by, int r, int v[8]) {
    const int W = g.w, H = g.h;
    if (comp == 0) {
        const int y = min(by * 8 + r, H - 1);
        const uint8_t *row = img + (size_t)y * W * 3;
        for (int j = 0; j < 8; ++j) v[j] = ycc(0, row + (size_t)min(bx * 8 + j, W - 1) * 3) - 128;
        return;
    }
    const int cy = min(by * 8 + r, g.ch - 1);   // below the image: the last downsampled row again
    const int y0 = min(cy * g.vs, H - 1), y1 = min(cy * g.vs + g.vs - 1, H - 1);
    const uint8_t *r0 = img + (size_t)y0 * W * 3, *r1 = img + (size_t)y1 * W * 3;
    for (int j = 0; j < 8; ++j) {
        const int cx = bx * 8 + j;
        if (g.hs == 1) {
            v[j] = ycc(comp, r0 + (size_t)min(cx, W - 1) * 3) - 128;
            continue;
        }
        const size_t x0 = (size_t)min(2 * cx, W - 1) * 3, x1 = (size_t)min(2 * cx + 1, W - 1) * 3;
        const int a = ycc(comp, r0 + x0), b = ycc(comp, r0 + x1);
        if (g.vs == 1)
            v[j] = ((a + b + (cx & 1)) >> 1) - 128;
        else
            v[j] = ((a + b + ycc(comp, r1 + x0) + ycc(comp, r1 + x1) + 1 + (cx & 1)) >> 2) - 128;
    }
}

HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c (CONST_BITS 13, PASS1_BITS 2) on eight values: PASS 1 the rows, PASS 2 the columns.
template <int PASS>
HD void fdct8(int d[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int n = PASS == 1 ? 11 : 15;
    if (PASS == 1) {
        d[0] = (tmp10 + tmp11) * 4;
        d[4] = (tmp10 - tmp11) * 4;
    } else {
        d[0] = descale(tmp10 + tmp11, 2);
        d[4] = descale(tmp10 - tmp11, 2);
    }
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = descale(z1 + tmp13 * 6270, n);
    d[6] = descale(z1 + tmp12 * -15137, n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(t4 + z1 + z3, n);
    d[5] = descale(t5 + z2 + z4, n);
    d[3] = descale(t6 + z2 + z3, n);
    d[1] = descale(t7 + z1 + z4, n);
}

HD int quantise(int c, int q) {
    const int d = q * 8;
    int a = c < 0 ? -c : c;
    a = (a + (d >> 1)) / d;
    return c < 0 ? -a : a;
}

// ------------------------------------------------------------------------------------------------ entropy coding
struct Code {
    unsigned long long bits;  // right aligned
    int len;                  // 0..64
};

HD int bit_length(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// What lane k of a block writes: k = 0 the DC difference v; k > 0 with v != 0 the ZRLs of its run, its code and its value
// bits; k = 63 with v = 0 the EOB.  nz: bit j set where coefficient j (1..63, zigzag order) is not zero.
HD Code lane_code(int k, int v, unsigned long long nz, int chroma) {
    Code c = {0, 0};
    if (k == 0) {
        const int s = bit_length(v);
        const uint32_t e = TABLE(enc_dc)[chroma][s];
        c.bits = ((unsigned long long)(e >> 8) << s) | (unsigned)(v < 0 ? v + (1 << s) - 1 : v);
        c.len = (int)(e & 255) + s;
    } else if (v != 0) {
        const unsigned long long below = nz & ((1ull << k) - 1);
        int run = k - (below ? 63 - __builtin_clzll(below) : 0) - 1;
        const uint32_t zrl = TABLE(enc_ac)[chroma][0xF0];
        for (; run > 15; run -= 16) {
            c.bits = (c.bits << (zrl & 255)) | (zrl >> 8);
            c.len += (int)(zrl & 255);
        }
        const int s = bit_length(v);
        const uint32_t e = TABLE(enc_ac)[chroma][(run << 4) | s];
        c.bits = (((c.bits << (e & 255)) | (e >> 8)) << s) | (unsigned)(v < 0 ? v + (1 << s) - 1 : v);
        c.len += (int)(e & 255) + s;
    } else if (k == 63) {
        const uint32_t e = TABLE(enc_ac)[chroma][0];
        c.bits = e >> 8;
        c.len = (int)(e & 255);
    }
    return c;
}

HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24); }

HD void or_word(uint32_t *p, uint32_t v) {
    if (!v) return;
#ifdef __HIP_DEVICE_COMPILE__
    atomicOr(p, bswap32(v));
#else
    *p |= bswap32(v);
#endif
}

// ORs the `len` low bits of `code` into the big-endian bit stream at bit position `pos` (words cleared beforehand).
HD void put_bits(uint32_t *words, long long pos, unsigned long long code, int len) {
    if (len == 0) return;
    const int s = (int)(pos & 31), sh = 96 - s - len;   // code * 2^sh in a 96-bit field
    const unsigned long long lo = sh < 64 ? code << sh : 0;
    const uint32_t hi = sh == 0 ? 0u : (sh < 64 ? (uint32_t)(code >> (64 - sh)) : (uint32_t)(code << (sh - 64)));
    uint32_t *w = words + (pos >> 5);
    or_word(w, hi);
    or_word(w + 1, (uint32_t)(lo >> 32));
    or_word(w + 2, (uint32_t)lo);
}

// ------------------------------------------------------------------------------------------------ scan of the bit counts
// A run of blocks as a function of the bit position p it starts at: hb ? roundup8(p + a) + b : p + a.
struct Seg {
    long long a, b;
    int hb;
};
HD long long up8(long long p) { return (p + 7) & ~7ll; }
HD Seg seg_of(int first, uint32_t bits) { return first ? Seg{0, (long long)bits, 1} : Seg{(long long)bits, 0, 0}; }
HD Seg compose(const Seg &f, const Seg &s) {   // f, then s
    if (!s.hb) return f.hb ? Seg{f.a, f.b + s.a, 1} : Seg{f.a + s.a, 0, 0};
    return f.hb ? Seg{f.a, up8(f.b + s.a) + s.b, 1} : Seg{f.a + s.a, s.b, 1};
}
HD long long apply(const Seg &f, long long p) { return f.hb ? up8(p + f.a) + f.b : p + f.a; }

HD Seg scan_summary(const Geo &g, const uint32_t *bits, int i0, int i1) {
    Seg f = {0, 0, 0};
    for (int i = i0; i < i1; ++i) f = compose(f, seg_of(first_of_interval(g, i), bits[i]));
    return f;
}
// bits[i0..i1) -> exclusive bit offsets (modulo 2^32: only read where the frame fits), interval starts in bytes
HD void scan_write(const Geo &g, uint32_t *bits, int32_t *istart, int i0, int i1, long long p) {
    for (int i = i0; i < i1; ++i) {
        if (first_of_interval(g, i)) {
            p = up8(p);
            istart[g.restart ? i / g.bpm / g.restart : 0] = (int32_t)min(p >> 3, (long long)INT32_MAX);
        }
        const uint32_t n = bits[i];
        bits[i] = (uint32_t)p;
        p += n;
    }
}
HD void scan_finish(const Geo &g, long long end_bits, int32_t *ubytes, int32_t *status) {
    const long long U = up8(end_bits) >> 3;
    const bool over = (long long)g.hdr + U + 2ll * (g.nint - 1) + 2 > g.max_bytes;
    *ubytes = over ? 0 : (int32_t)U;
    *status = over ? SGV3D_JPEG_ENC_EOVERFLOW : 0;
}

// ------------------------------------------------------------------------------------------------ stuffing
HD int ff_count16(const uint8_t *stream, long long u0, int U) {
    int n = 0;
    for (int j = 0; j < 16; ++j) n += (u0 + j < U && stream[u0 + j] == 0xFF);
    return n;
}

// The 16 bytes of the unstuffed stream at u0 -> their places in the file: `ff` FF bytes lie before u0 in the frame.
HD void stuff16(const Geo &g, const uint8_t *stream, const int32_t *istart, long long u0, int U, int ff, uint8_t *file) {
    if (u0 >= U) return;
    int lo = 0, hi = g.nint;   // k: the interval of byte u0 = (number of starts <= u0) - 1
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (istart[mid] <= u0) lo = mid; else hi = mid;
    }
    int k = lo;
    uint8_t *o = file + g.hdr + u0 + ff + 2ll * k - (k > 0 && istart[k] == u0 ? 2 : 0);
    if (k > 0 && istart[k] == u0) --k;   // the marker in front of byte u0 is this lane's
    for (int j = 0; j < 16 && u0 + j < U; ++j) {
        if (k + 1 < g.nint && istart[k + 1] == u0 + j) {
            *o++ = 0xFF;
            *o++ = (uint8_t)(0xD0 + (k & 7));
            ++k;
        }
        const uint8_t v = stream[u0 + j];
        *o++ = v;
        if (v == 0xFF) *o++ = 0;
    }
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void k_transform(const uint8_t *__restrict__ frames, int16_t *__restrict__ coef, Geo g, QTab qt) {
    __shared__ int tile[32][8][9];
    __shared__ __attribute__((aligned(16))) int16_t zz[32][64];
    const int lb = threadIdx.x >> 3, t = threadIdx.x & 7, blk = blockIdx.x * 32 + lb;
    const bool valid = blk < g.nblk;
    const uint8_t *img = frames + (size_t)blockIdx.y * g.h * g.w * 3;
    int comp = 0, bx = 0, by = 0, v[8];
    bool dummy = false;
    if (valid) {
        resolve(g, blk, comp, bx, by, dummy);
        load_row(img, g, comp, bx, by, t, v);
        fdct8<1>(v);
        for (int j = 0; j < 8; ++j) tile[lb][t][j] = v[j];
    }
    __syncthreads();
    if (valid) {
        for (int r = 0; r < 8; ++r) v[r] = tile[lb][r][t];
        fdct8<2>(v);
        for (int r = 0; r < 8; ++r) {
            const int n = r * 8 + t;
            const int q = quantise(v[r], qt.q[comp > 0][n]);
            zz[lb][d_zigpos[n]] = (int16_t)(dummy && n ? 0 : q);
        }
    }
    __syncthreads();
    if (valid)
        reinterpret_cast<uint4 *>(coef + ((size_t)blockIdx.y * g.nblk + blk) * 64)[t] = reinterpret_cast<const uint4 *>(zz[lb])[t];
}

// lane's coefficient of block blk (the DC difference in lane 0) and the mask of the non-zero AC coefficients
__device__ __forceinline__ int lane_value(const int16_t *coef, const Geo &g, int blk, int lane, unsigned long long &nz) {
    int v = coef[(size_t)blk * 64 + lane];
    if (lane == 0) {
        const int p = dc_predecessor(g, blk);
        if (p >= 0) v -= coef[(size_t)p * 64];
    }
    nz = __ballot(lane > 0 && v != 0);
    return v;
}

__global__ __launch_bounds__(256) void k_size(const int16_t *__restrict__ coef, uint32_t *__restrict__ bits, uint4 *__restrict__ stream, Geo g) {
    const size_t f = blockIdx.y;
    // clear the frame's unstuffed stream (pack ORs into it)
    uint4 *s = stream + f * (g.ucap / 16);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < g.ucap / 16; i += gridDim.x * 256) s[i] = make_uint4(0, 0, 0, 0);
    const int lane = threadIdx.x & 63, blk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= g.nblk) return;
    unsigned long long nz;
    const int v = lane_value(coef + f * g.nblk * 64, g, blk, lane, nz);
    int n = lane_code(lane, v, nz, blk % g.bpm >= g.nlum).len;
    for (int d = 32; d; d >>= 1) n += __shfl_xor(n, d);
    if (lane == 0) bits[f * g.nblk + blk] = (uint32_t)n;
}

__global__ __launch_bounds__(kScanThreads) void k_scan(uint32_t *__restrict__ bits, int32_t *__restrict__ istart, int32_t *__restrict__ ubytes,
                                                        int32_t *__restrict__ status, Geo g) {
    __shared__ Seg seg[2][kScanThreads];
    const size_t f = blockIdx.x;
    uint32_t *b = bits + f * g.nblk;
    const int t = threadIdx.x, per = (g.nblk + kScanThreads - 1) / kScanThreads;
    const int i0 = (int)min((long long)t * per, (long long)g.nblk), i1 = (int)min((long long)(t + 1) * per, (long long)g.nblk);
    seg[0][t] = scan_summary(g, b, i0, i1);
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kScanThreads; d <<= 1) {   // inclusive scan under composition
        seg[cur ^ 1][t] = t >= d ? compose(seg[cur][t - d], seg[cur][t]) : seg[cur][t];
        cur ^= 1;
        __syncthreads();
    }
    scan_write(g, b, istart + f * g.nint, i0, i1, t ? apply(seg[cur][t - 1], 0) : 0);
    if (t == 0) scan_finish(g, apply(seg[cur][kScanThreads - 1], 0), ubytes + f, status + f);
}

__global__ __launch_bounds__(256) void k_pack(const int16_t *__restrict__ coef, const uint32_t *__restrict__ bits, const int32_t *__restrict__ status,
                                               uint32_t *__restrict__ stream, Geo g) {
    const size_t f = blockIdx.y;
    const int lane = threadIdx.x & 63, blk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blk >= g.nblk || status[f]) return;
    unsigned long long nz;
    const int v = lane_value(coef + f * g.nblk * 64, g, blk, lane, nz);
    const Code c = lane_code(lane, v, nz, blk % g.bpm >= g.nlum);
    int incl = c.len;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    uint32_t *w = stream + f * (g.ucap / 4);
    const long long p = bits[f * g.nblk + blk];
    put_bits(w, p + incl - c.len, c.bits, c.len);
    if (lane == 63 && (blk == g.nblk - 1 || first_of_interval(g, blk + 1))) {   // pad the interval with 1-bits
        const int pad = (int)(-(p + incl) & 7);
        put_bits(w, p + incl, (1u << pad) - 1, pad);
    }
}

__device__ __forceinline__ int block_sum_256(int v, int *lds) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// exclusive sums over the 256 lanes of the workgroup; lds: 256 ints
__device__ __forceinline__ int block_exclusive_256(int v, int *lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    return lds[t] - v;
}

__global__ __launch_bounds__(256) void k_ffcount(const uint8_t *__restrict__ stream, const int32_t *__restrict__ ubytes, int32_t *__restrict__ cnt,
                                                  Geo g) {
    __shared__ int lds[4];
    const size_t f = blockIdx.y;
    const int n = ff_count16(stream + f * g.ucap, (long long)blockIdx.x * kChunk + threadIdx.x * 16, ubytes[f]);
    const int total = block_sum_256(n, lds);
    if (threadIdx.x == 0) cnt[f * g.chunks + blockIdx.x] = total;
}

// One workgroup walks the frames: exclusive sums of each frame's chunk counts, its length, its capacity test, its offset.
__global__ __launch_bounds__(256) void k_layout(int32_t *__restrict__ cnt, const int32_t *__restrict__ ubytes, int32_t *__restrict__ status,
                                                 int32_t *__restrict__ lengths, long long *__restrict__ fileoff, int frames, Geo g) {
    __shared__ int lds[256];
    long long out = 0;
    for (int f = 0; f < frames; ++f) {
        int carry = 0;
        for (int base = 0; base < g.chunks; base += 256) {
            const int i = base + threadIdx.x;
            const int v = i < g.chunks ? cnt[(size_t)f * g.chunks + i] : 0;
            const int ex = block_exclusive_256(v, lds);
            if (i < g.chunks) cnt[(size_t)f * g.chunks + i] = carry + ex;
            carry += lds[255];
            __syncthreads();
        }
        long long len = (long long)g.hdr + ubytes[f] + carry + 2ll * (g.nint - 1) + 2;
        const bool over = status[f] != 0 || len > g.max_bytes;
        if (over) len = 0;
        if (threadIdx.x == 0) {
            status[f] = over ? SGV3D_JPEG_ENC_EOVERFLOW : 0;
            lengths[f] = (int32_t)len;
            fileoff[f] = out;
        }
        out += (len + 15) & ~15ll;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_stuff(const uint8_t *__restrict__ stream, const int32_t *__restrict__ istart, const int32_t *__restrict__ ubytes,
                                                const int32_t *__restrict__ cnt, const int32_t *__restrict__ status,
                                                const int32_t *__restrict__ lengths, const long long *__restrict__ fileoff,
                                                uint8_t *__restrict__ files, Geo g, Header hdr) {
    __shared__ int lds[256];
    const size_t f = blockIdx.y;
    if (status[f]) return;
    const int U = ubytes[f];
    if ((long long)blockIdx.x * kChunk >= U) return;
    uint8_t *file = files + fileoff[f];
    const uint8_t *s = stream + f * g.ucap;
    const long long u0 = (long long)blockIdx.x * kChunk + threadIdx.x * 16;
    const int n = ff_count16(s, u0, U);
    const int ff = cnt[f * g.chunks + blockIdx.x] + block_exclusive_256(n, lds);
    stuff16(g, s, istart + f * g.nint, u0, U, ff, file);
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < g.hdr; i += 256) file[i] = hdr.b[i];
        if (threadIdx.x == 0) {
            file[lengths[f] - 2] = 0xFF;
            file[lengths[f] - 1] = 0xD9;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
int quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }

void quant_tables(int quality, QTab &qt) {
    static const uint8_t base[2][64] = {SGV3D_JPEG_K_QUANT_LUMA, SGV3D_JPEG_K_QUANT_CHROMA};
    const int s = quality_scale(quality);
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (base[t][i] * s + 50) / 100;
            qt.q[t][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

int check_settings(const char *who, int h, int w, int quality, int hs, int vs, int restart) {
    SGV3D_REQUIRE(h >= 1 && h <= 65535 && w >= 1 && w <= 65535, "%s: size %d x %d outside 1..65535", who, h, w);
    SGV3D_REQUIRE(quality >= 1 && quality <= 100, "%s: quality %d outside 1..100", who, quality);
    SGV3D_REQUIRE((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2),
                  "%s: sampling %dx%d is none of 1x1 (4:4:4), 2x1 (4:2:2), 2x2 (4:2:0)", who, hs, vs);
    SGV3D_REQUIRE(restart >= 0 && restart <= 65535, "%s: restart interval %d outside 0..65535", who, restart);
    return SGV3D_OK;
}

uint8_t *segment(uint8_t *p, int marker, int body) {
    *p++ = 0xFF;
    *p++ = (uint8_t)marker;
    *p++ = (uint8_t)((body + 2) >> 8);
    *p++ = (uint8_t)((body + 2) & 255);
    return p;
}

int build_header(int h, int w, int hs, int vs, int restart, const QTab &qt, uint8_t *out) {
    static const uint8_t zig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    static const uint8_t bits[4][16] = {SGV3D_JPEG_K_BITS_DC_LUMA, SGV3D_JPEG_K_BITS_AC_LUMA, SGV3D_JPEG_K_BITS_DC_CHROMA,
                                        SGV3D_JPEG_K_BITS_AC_CHROMA};
    static const uint8_t v0[] = SGV3D_JPEG_K_VALS_DC_LUMA, v1[] = SGV3D_JPEG_K_VALS_AC_LUMA, v2[] = SGV3D_JPEG_K_VALS_DC_CHROMA,
                         v3[] = SGV3D_JPEG_K_VALS_AC_CHROMA;
    static const uint8_t *const vals[4] = {v0, v1, v2, v3};
    static const int nvals[4] = {sizeof(v0), sizeof(v1), sizeof(v2), sizeof(v3)};
    static const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    uint8_t *p = out;
    *p++ = 0xFF;
    *p++ = 0xD8;
    p = segment(p, 0xE0, 14);
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(p, jfif, 14);
    p += 14;
    for (int t = 0; t < 2; ++t) {
        p = segment(p, 0xDB, 65);
        *p++ = (uint8_t)t;
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)qt.q[t][zig[k]];
    }
    p = segment(p, 0xC0, 15);
    *p++ = 8;
    *p++ = (uint8_t)(h >> 8);
    *p++ = (uint8_t)(h & 255);
    *p++ = (uint8_t)(w >> 8);
    *p++ = (uint8_t)(w & 255);
    *p++ = 3;
    for (int c = 0; c < 3; ++c) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c ? 0x11 : hs * 16 + vs);
        *p++ = (uint8_t)(c ? 1 : 0);
    }
    for (int t = 0; t < 4; ++t) {
        p = segment(p, 0xC4, 17 + nvals[t]);
        *p++ = ids[t];
        memcpy(p, bits[t], 16);
        p += 16;
        memcpy(p, vals[t], nvals[t]);
        p += nvals[t];
    }
    if (restart) {
        p = segment(p, 0xDD, 2);
        *p++ = (uint8_t)(restart >> 8);
        *p++ = (uint8_t)(restart & 255);
    }
    p = segment(p, 0xDA, 10);
    *p++ = 3;
    for (int c = 0; c < 3; ++c) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (uint8_t)(c ? 0x11 : 0x00);
    }
    *p++ = 0;
    *p++ = 63;
    *p++ = 0;
    return (int)(p - out);
}

Geo geometry(int h, int w, int hs, int vs, int restart, int max_bytes) {
    Geo g;
    g.h = h, g.w = w, g.hs = hs, g.vs = vs;
    g.mcux = (w + 8 * hs - 1) / (8 * hs), g.mcuy = (h + 8 * vs - 1) / (8 * vs);
    g.nlum = hs * vs, g.bpm = g.nlum + 2;
    g.wb = (w + 7) / 8, g.hb = (h + 7) / 8, g.ch = (h + vs - 1) / vs;
    g.restart = restart;
    const long long nmcu = (long long)g.mcux * g.mcuy;
    g.nint = restart ? (int)((nmcu + restart - 1) / restart) : 1;
    g.nblk = (int)(nmcu * g.bpm);   // at most 8192 * 8192 * 3
    g.hdr = 623 + (restart ? 6 : 0);
    g.max_bytes = max_bytes;
    g.ucap = (max_bytes + kChunk - 1) / kChunk * kChunk;
    g.chunks = g.ucap / kChunk;
    return g;
}

size_t up16(size_t n) { return (n + 15) / 16 * 16; }

struct Layout {
    size_t coef, bits, istart, stream, cnt, ubytes, fileoff, total;
};
Layout layout(int frames, const Geo &g) {
    Layout l;
    size_t o = 0;
    l.coef = o, o += up16((size_t)frames * g.nblk * 128);
    l.bits = o, o += up16((size_t)frames * g.nblk * 4);
    l.istart = o, o += up16((size_t)frames * g.nint * 4);
    l.stream = o, o += (size_t)frames * g.ucap;
    l.cnt = o, o += up16((size_t)frames * g.chunks * 4);
    l.ubytes = o, o += up16((size_t)frames * 4);
    l.fileoff = o, o += up16((size_t)frames * 8);
    l.total = o;
    return l;
}

int check_call(const char *who, int frames, int h, int w, int quality, int hs, int vs, int restart, int max_bytes, const void *src,
               const void *files, long long files_bytes, const void *lengths, const void *status) {
    if (int rc = check_settings(who, h, w, quality, hs, vs, restart)) return rc;
    SGV3D_REQUIRE(frames >= 1 && frames <= kMaxFrames, "%s: %d frames outside 1..%d", who, frames, kMaxFrames);
    SGV3D_REQUIRE(max_bytes >= 1 && max_bytes <= kMaxBytes, "%s: max_bytes %d outside 1..2^26", who, max_bytes);
    SGV3D_REQUIRE(src && files && lengths && status, "%s: null pointer", who);
    SGV3D_REQUIRE(files_bytes >= (long long)frames * (long long)up16(max_bytes), "%s: files holds %lld bytes, %d frames of up to %d need %lld", who,
                  files_bytes, frames, max_bytes, (long long)frames * (long long)up16(max_bytes));
    return SGV3D_OK;
}

}  // namespace

extern "C" int sgv3d_jpeg_encode_header(int h, int w, int quality, int hs, int vs, int restart, uint8_t *header, int *header_len,
                                        uint16_t *quant) {
    if (int rc = check_settings("sgv3d_jpeg_encode_header", h, w, quality, hs, vs, restart)) return rc;
    SGV3D_REQUIRE(header && header_len, "sgv3d_jpeg_encode_header: null pointer");
    QTab qt;
    quant_tables(quality, qt);
    *header_len = build_header(h, w, hs, vs, restart, qt, header);
    if (quant) memcpy(quant, qt.q, sizeof(qt.q));
    return SGV3D_OK;
}

extern "C" size_t sgv3d_jpeg_encode_workspace_bytes(int frames, int h, int w, int hs, int vs, int restart, int max_bytes) {
    if (check_settings("sgv3d_jpeg_encode_workspace_bytes", h, w, 50, hs, vs, restart) != SGV3D_OK) return 0;
    if (frames < 1 || frames > kMaxFrames || max_bytes < 1 || max_bytes > kMaxBytes) {
        fail(SGV3D_EINVAL, "sgv3d_jpeg_encode_workspace_bytes: %d frames / max_bytes %d out of range", frames, max_bytes);
        return 0;
    }
    return layout(frames, geometry(h, w, hs, vs, restart, max_bytes)).total;
}

extern "C" int sgv3d_jpeg_encode(int frames, int h, int w, int quality, int hs, int vs, int restart, int max_bytes, const uint8_t *src,
                                 void *work, size_t work_bytes, uint8_t *files, long long files_bytes, int32_t *lengths, int32_t *status,
                                 void *stream) {
    const char *who = "sgv3d_jpeg_encode";
    if (int rc = check_call(who, frames, h, w, quality, hs, vs, restart, max_bytes, src, files, files_bytes, lengths, status)) return rc;
    SGV3D_REQUIRE(work && ((uintptr_t)work & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    const Geo g = geometry(h, w, hs, vs, restart, max_bytes);
    const Layout l = layout(frames, g);
    if (work_bytes < l.total) return fail(SGV3D_ENOSPACE, "%s: the workspace holds %zu bytes, %zu are needed", who, work_bytes, l.total);
    QTab qt;
    quant_tables(quality, qt);
    Header hdr;
    memset(hdr.b, 0, sizeof(hdr.b));
    build_header(h, w, hs, vs, restart, qt, hdr.b);
    char *ws = (char *)work;
    int16_t *coef = (int16_t *)(ws + l.coef);
    uint32_t *bits = (uint32_t *)(ws + l.bits);
    int32_t *istart = (int32_t *)(ws + l.istart), *cnt = (int32_t *)(ws + l.cnt), *ubytes = (int32_t *)(ws + l.ubytes);
    uint8_t *ustream = (uint8_t *)(ws + l.stream);
    long long *fileoff = (long long *)(ws + l.fileoff);
    hipStream_t st = as_stream(stream);
    k_transform<<<dim3(cdiv(g.nblk, 32), frames), 256, 0, st>>>(src, coef, g, qt);
    if (int rc = check_launch("jpeg_encode transform")) return rc;
    k_size<<<dim3(cdiv(g.nblk, 4), frames), 256, 0, st>>>(coef, bits, (uint4 *)ustream, g);
    if (int rc = check_launch("jpeg_encode size")) return rc;
    k_scan<<<frames, kScanThreads, 0, st>>>(bits, istart, ubytes, status, g);
    if (int rc = check_launch("jpeg_encode scan")) return rc;
    k_pack<<<dim3(cdiv(g.nblk, 4), frames), 256, 0, st>>>(coef, bits, status, (uint32_t *)ustream, g);
    if (int rc = check_launch("jpeg_encode pack")) return rc;
    k_ffcount<<<dim3(g.chunks, frames), 256, 0, st>>>(ustream, ubytes, cnt, g);
    if (int rc = check_launch("jpeg_encode ffcount")) return rc;
    k_layout<<<1, 256, 0, st>>>(cnt, ubytes, status, lengths, fileoff, frames, g);
    if (int rc = check_launch("jpeg_encode layout")) return rc;
    k_stuff<<<dim3(g.chunks, frames), 256, 0, st>>>(ustream, istart, ubytes, cnt, status, lengths, fileoff, files, g, hdr);
    return check_launch("jpeg_encode stuff");
}

extern "C" int sgv3d_jpeg_encode_host(int frames, int h, int w, int quality, int hs, int vs, int restart, int max_bytes, const uint8_t *src,
                                      uint8_t *files, long long files_bytes, int32_t *lengths, int32_t *status) {
    const char *who = "sgv3d_jpeg_encode_host";
    if (int rc = check_call(who, frames, h, w, quality, hs, vs, restart, max_bytes, src, files, files_bytes, lengths, status)) return rc;
    const Geo g = geometry(h, w, hs, vs, restart, max_bytes);
    QTab qt;
    quant_tables(quality, qt);
    Header hdr;
    build_header(h, w, hs, vs, restart, qt, hdr.b);
    std::vector<int16_t> coef((size_t)g.nblk * 64);
    std::vector<uint32_t> bits(g.nblk), words(g.ucap / 4);
    std::vector<int32_t> istart(g.nint), cnt(g.chunks);
    long long out = 0;
    for (int f = 0; f < frames; ++f) {
        const uint8_t *img = src + (size_t)f * h * w * 3;
        // transform
        for (int blk = 0; blk < g.nblk; ++blk) {
            int comp, bx, by, tile[8][8], v[8];
            bool dummy;
            resolve(g, blk, comp, bx, by, dummy);
            for (int r = 0; r < 8; ++r) {
                load_row(img, g, comp, bx, by, r, v);
                fdct8<1>(v);
                for (int j = 0; j < 8; ++j) tile[r][j] = v[j];
            }
            for (int c = 0; c < 8; ++c) {
                for (int r = 0; r < 8; ++r) v[r] = tile[r][c];
                fdct8<2>(v);
                for (int r = 0; r < 8; ++r) {
                    const int n = r * 8 + c;
                    coef[(size_t)blk * 64 + h_zigpos[n]] = (int16_t)(dummy && n ? 0 : quantise(v[r], qt.q[comp > 0][n]));
                }
            }
        }
        // size
        auto lane_values = [&](int blk, int v[64]) {
            unsigned long long nz = 0;
            for (int k = 0; k < 64; ++k) {
                v[k] = coef[(size_t)blk * 64 + k];
                if (k && v[k]) nz |= 1ull << k;
            }
            const int p = dc_predecessor(g, blk);
            if (p >= 0) v[0] -= coef[(size_t)p * 64];
            return nz;
        };
        for (int blk = 0; blk < g.nblk; ++blk) {
            int v[64], n = 0;
            const unsigned long long nz = lane_values(blk, v);
            for (int k = 0; k < 64; ++k) n += lane_code(k, v[k], nz, blk % g.bpm >= g.nlum).len;
            bits[blk] = (uint32_t)n;
        }
        // scan: the kernel's chunks and its composition, in order
        int32_t U = 0;
        {
            const int per = (g.nblk + kScanThreads - 1) / kScanThreads;
            Seg run = {0, 0, 0};
            for (int t = 0; t < kScanThreads; ++t) {
                const int i0 = (int)std::min((long long)t * per, (long long)g.nblk), i1 = (int)std::min((long long)(t + 1) * per, (long long)g.nblk);
                const Seg s = scan_summary(g, bits.data(), i0, i1);
                scan_write(g, bits.data(), istart.data(), i0, i1, apply(run, 0));
                run = compose(run, s);
            }
            scan_finish(g, apply(run, 0), &U, status + f);
        }
        lengths[f] = 0;
        if (status[f]) continue;
        // pack
        std::fill(words.begin(), words.end(), 0u);
        for (int blk = 0; blk < g.nblk; ++blk) {
            int v[64];
            const unsigned long long nz = lane_values(blk, v);
            long long p = bits[blk];
            for (int k = 0; k < 64; ++k) {
                const Code c = lane_code(k, v[k], nz, blk % g.bpm >= g.nlum);
                put_bits(words.data(), p, c.bits, c.len);
                p += c.len;
            }
            if (blk == g.nblk - 1 || first_of_interval(g, blk + 1)) {
                const int pad = (int)(-p & 7);
                put_bits(words.data(), p, (1u << pad) - 1, pad);
            }
        }
        // ffcount, layout
        const uint8_t *s = (const uint8_t *)words.data();
        int ff_total = 0;
        for (int c = 0; c < g.chunks; ++c) {
            cnt[c] = ff_total;
            for (int t = 0; t < 256; ++t) ff_total += ff_count16(s, (long long)c * kChunk + t * 16, U);
        }
        const long long len = (long long)g.hdr + U + ff_total + 2ll * (g.nint - 1) + 2;
        if (len > g.max_bytes) {
            status[f] = SGV3D_JPEG_ENC_EOVERFLOW;
            continue;
        }
        lengths[f] = (int32_t)len;
        // stuff
        uint8_t *file = files + out;
        for (int c = 0; c < g.chunks; ++c) {
            int ff = cnt[c];
            for (int t = 0; t < 256; ++t) {
                const long long u0 = (long long)c * kChunk + t * 16;
                stuff16(g, s, istart.data(), u0, U, ff, file);
                ff += ff_count16(s, u0, U);
            }
        }
        memcpy(file, hdr.b, g.hdr);
        file[len - 2] = 0xFF;
        file[len - 1] = 0xD9;
        out += (len + 15) & ~15ll;
    }
    return SGV3D_OK;
}
