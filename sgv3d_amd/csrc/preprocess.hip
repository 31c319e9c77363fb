// Camera-frame preprocessing on the device: uint8 HWC frames -> the float32 planar tensor BEVHeight.forward takes, and
// the SGV3D semantic mask -> uint8 labels.  Replaces the per-image CPU path of the reference's dataset
// (dataset/nusc_mv_det_dataset.py:133-161 img_transform: PIL resize (bicubic) + crop + flip; :594-625 mmcv.imnormalize +
// HWC->CHW; :603-614 the mask through the same img_transform, then (mask / 40).astype(uint8)[..., 0]).
//
// The resize is Pillow's 8-bit separable resampler restated exactly (Pillow's src/libImaging/Resample.c): integer
// coefficients with 22 fractional bits, a horizontal pass into uint8, then a vertical pass, each accumulator started at
// 1 << 21 and clipped to 0..255 after >> 22.  Pillow skips a pass whose dimension does not change; at scale 1 the
// coefficients are the identity (one weight of 1 << 22), so running both passes always gives the same bytes.
// The coefficient tables are computed on the host (sgv3d_resample_coeffs) and uploaded once by the caller.
//
// Built with -ffp-contract=off: the normalise is two float32 roundings, (x - mean) then * (1 / std), as mmcv's
// imnormalize_ does with cv2.subtract / cv2.multiply.
#include <math.h>

#include "common.hpp"

using namespace sgv3d;

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64;       // output columns per workgroup
constexpr int kTileH = 16;       // output rows per workgroup
constexpr int kPrecision = 22;   // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)
constexpr int kMaxKsize = 17;    // 2 * ceil(2 * 4) + 1: a 4x downscale

// Pillow's bicubic filter, a = -0.5 (Resample.c bicubic_filter)
double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

int ksize_of(int in_size, int out_size) {
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(2.0 * fs) * 2 + 1;
}

// Largest source span (in pixels) that `tile` consecutive output positions read: the window of output o covers
// [int(c_o - s + 0.5), int(c_o + s + 0.5)) with c_o = (o + 0.5) * scale, so `tile` outputs span at most
// (tile - 1) * scale + 2 s + 1 pixels.
int span_cap(int in_size, int out_size, int tile) {
    const double scale = (double)in_size / out_size;
    const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil((tile - 1) * scale + 2.0 * support) + 2;
}

struct PrepArgs {
    const uint8_t *src;
    void *dst;
    const int2 *xb;  // [rs_w] (first source column, taps)
    const int *xk;   // [rs_w][kx]
    const int2 *yb;  // [rs_h]
    const int *yk;   // [rs_h][ky]
    int in_h, in_w, chans;      // source frame [in_h, in_w, chans] uint8
    int rs_h, rs_w;             // resized size
    int crop_x, crop_y;         // crop box origin in the resized image
    int out_h, out_w;           // crop box size = output size
    int kx, ky;                 // coefficient row lengths
    int flip, swap_rb;
    int rows_cap, pitch;        // staged source rows / LDS row pitch in bytes
    float mean[3], mul[3];
};

__device__ inline int clip8(int acc) {
    const int v = acc >> kPrecision;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// One workgroup = kTileH x kTileW outputs of one frame.  LDS: the source rows and columns the tile reads (16-byte
// aligned chunks of each row), the horizontal pass's uint8 result for the tile's columns, and the tile's coefficients.
// NCH = channels resampled: 3 (images) or 1 (masks: channel 0 of a chans-channel frame).  KT >= both ksizes: the tap loops
// are unrolled to KT (guarded by the window's tap count), so a thread's LDS reads of all taps are in flight together.
template <int NCH, int KT>
__global__ __launch_bounds__(kBlock) void preprocess_kernel(PrepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int TP = kTileW * NCH;  // horizontal-pass row pitch (bytes)
    const int tid = threadIdx.x;
    const int f = blockIdx.z;
    const int ox0 = blockIdx.x * kTileW, oy0 = blockIdx.y * kTileH;
    const int jn = min(kTileW, a.out_w - ox0), in_ = min(kTileH, a.out_h - oy0);
    const int C = a.chans;

    // resized columns of the tile (contiguous; reversed when flipped), clipped to the resized image
    const int cx_lo = a.flip ? a.out_w - ox0 - jn : ox0;
    const int rx_lo = max(cx_lo + a.crop_x, 0), rx_hi = min(cx_lo + jn + a.crop_x, a.rs_w);
    const int ry_lo = max(oy0 + a.crop_y, 0), ry_hi = min(oy0 + in_ + a.crop_y, a.rs_h);
    const bool any = rx_lo < rx_hi && ry_lo < ry_hi;

    int sx0 = 0, sy0 = 0, ncols = 0, nrows = 0;
    if (any) {
        const int2 bx0 = a.xb[rx_lo], bx1 = a.xb[rx_hi - 1], by0 = a.yb[ry_lo], by1 = a.yb[ry_hi - 1];
        sx0 = max(bx0.x, 0);
        sy0 = max(by0.x, 0);
        ncols = min(bx1.x + bx1.y, a.in_w) - sx0;
        nrows = min(by1.x + by1.y, a.in_h) - sy0;
        ncols = max(0, min(ncols, (a.pitch - 32) / C));   // (span_cap bounds both; the clamps keep LDS in range regardless)
        nrows = max(0, min(nrows, a.rows_cap));
    }

    unsigned char *stage = smem;                                        // [rows_cap][pitch]
    unsigned char *hrow = smem + (size_t)a.rows_cap * a.pitch;          // [rows_cap][TP]
    int *kxs = reinterpret_cast<int *>(hrow + (size_t)a.rows_cap * TP);  // [kTileW][kx]
    int *kys = kxs + kTileW * a.kx;                                     // [kTileH][ky]

    const uint8_t *frame = a.src + (size_t)f * a.in_h * a.in_w * C;
    const size_t row_bytes = (size_t)a.in_w * C;
    const int span = ncols * C;

    // 1. stage source rows [sy0, sy0 + nrows), bytes [sx0 C, (sx0 + ncols) C), as 16-byte loads.  Each chunk is a
    //    16-byte aligned block that holds at least one byte of the range, so it never leaves the pages of the frame.
    const int nch = (span + 30) / 16 + 1;
    for (int idx = tid; idx < nrows * nch; idx += kBlock) {
        const int r = idx / nch, q = idx - r * nch;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(frame + (size_t)(sy0 + r) * row_bytes + (size_t)sx0 * C);
        const uintptr_t c = (b0 & ~(uintptr_t)15) + 16 * (uintptr_t)q;
        if (c < b0 + span)
            *reinterpret_cast<uint4 *>(stage + r * a.pitch + 16 * q) = *reinterpret_cast<const uint4 *>(c);
    }
    // the tile's coefficients (columns in output order, so the flip is absorbed here)
    for (int idx = tid; idx < kTileW * a.kx; idx += kBlock) {
        const int j = idx / a.kx, k = idx - j * a.kx;
        const int cx = a.flip ? a.out_w - 1 - (ox0 + j) : ox0 + j;
        const int rx = cx + a.crop_x;
        kxs[idx] = (j < jn && rx >= 0 && rx < a.rs_w) ? a.xk[(size_t)rx * a.kx + k] : 0;
    }
    for (int idx = tid; idx < kTileH * a.ky; idx += kBlock) {
        const int i = idx / a.ky, k = idx - i * a.ky;
        const int ry = oy0 + i + a.crop_y;
        kys[idx] = (i < in_ && ry >= 0 && ry < a.rs_h) ? a.yk[(size_t)ry * a.ky + k] : 0;
    }
    __syncthreads();

    // 2. horizontal pass: staged row r, tile column j -> hrow[r][j][c]
    {
        const int j = tid & (kTileW - 1);
        const int cx = a.flip ? a.out_w - 1 - (ox0 + j) : ox0 + j;
        const int rx = cx + a.crop_x;
        if (any && j < jn && rx >= 0 && rx < a.rs_w) {
            const int2 b = a.xb[rx];
            const int x0 = max(b.x, sx0) - sx0;
            const int n = min(b.y, ncols - x0);
            const int *w = kxs + j * a.kx;
            for (int r = tid / kTileW; r < nrows; r += kBlock / kTileW) {
                const uintptr_t b0 = reinterpret_cast<uintptr_t>(frame + (size_t)(sy0 + r) * row_bytes + (size_t)sx0 * C);
                const unsigned char *p = stage + r * a.pitch + (int)(b0 & 15) + x0 * C;
                int acc[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] = 1 << (kPrecision - 1);
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    if (k < n) {
                        const int wk = w[k];
#pragma unroll
                        for (int c = 0; c < NCH; ++c) acc[c] += (int)p[k * C + c] * wk;
                    }
                }
#pragma unroll
                for (int c = 0; c < NCH; ++c) hrow[r * TP + j * NCH + c] = (unsigned char)clip8(acc[c]);
            }
        }
    }
    __syncthreads();

    // 3. vertical pass + crop fill + output: thread = one output row x 4 consecutive columns
    const int i = tid / (kTileW / 4), j0 = (tid % (kTileW / 4)) * 4;
    if (i >= in_ || j0 >= jn) return;
    const int oy = oy0 + i, ry = oy + a.crop_y;
    int v[4][NCH];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[q][c] = 0;
    if (any && ry >= 0 && ry < a.rs_h) {
        const int2 b = a.yb[ry];
        const int y0 = max(b.x, sy0) - sy0;
        const int n = min(b.y, nrows - y0);
        const int *w = kys + i * a.ky;
        int acc[4][NCH];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < NCH; ++c) acc[q][c] = 1 << (kPrecision - 1);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            const bool tap = k < n;
            const int wk = tap ? w[k] : 0;
            // 4 * NCH consecutive bytes at a 4-byte aligned offset (TP and j0 * NCH are multiples of 4)
            const unsigned *h = reinterpret_cast<const unsigned *>(hrow + (y0 + k) * TP + j0 * NCH);
            unsigned words[NCH];
#pragma unroll
            for (int t = 0; t < NCH; ++t) words[t] = tap ? h[t] : 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const int e = q * NCH + c;
                    acc[q][c] += (int)((words[e >> 2] >> (8 * (e & 3))) & 0xff) * wk;
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cx = a.flip ? a.out_w - 1 - (ox0 + j0 + q) : ox0 + j0 + q;
            const int rx = cx + a.crop_x;
            if (rx >= 0 && rx < a.rs_w)
#pragma unroll
                for (int c = 0; c < NCH; ++c) v[q][c] = clip8(acc[q][c]);
        }
    }
    const int nq = min(4, jn - j0);
    const size_t plane = (size_t)a.out_h * a.out_w;
    const size_t o = (size_t)oy * a.out_w + ox0 + j0;
    if (NCH == 3) {
        float *dst = static_cast<float *>(a.dst) + (size_t)f * 3 * plane + o;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sc = a.swap_rb ? 2 - c : c;
            float y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = ((float)v[q][sc] - a.mean[c]) * a.mul[c];
            float *p = dst + c * plane;
            if (nq == 4 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                *reinterpret_cast<float4 *>(p) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
                for (int q = 0; q < nq; ++q) p[q] = y[q];
            }
        }
    } else {
        uint8_t *p = static_cast<uint8_t *>(a.dst) + (size_t)f * plane + o;
        uint8_t m[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) m[q] = (uint8_t)(v[q][0] / 40);
        if (nq == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            *reinterpret_cast<uchar4 *>(p) = make_uchar4(m[0], m[1], m[2], m[3]);
        } else {
            for (int q = 0; q < nq; ++q) p[q] = m[q];
        }
    }
}

PerDeviceSize g_lds_images, g_lds_mask;

template <int NCH, int KT>
int launch_kt(const PrepArgs &a, size_t lds, PerDeviceSize &state, const char *what, int frames, void *stream) {
    auto kernel = preprocess_kernel<NCH, KT>;
    if (lds > 64 * 1024 && !ensure_dynamic_lds(reinterpret_cast<const void *>(kernel), lds, state))
        return fail(SGV3D_ELAUNCH, "%s: cannot raise the LDS limit to %zu bytes", what, lds);
    hipLaunchKernelGGL(kernel, dim3(cdiv(a.out_w, kTileW), cdiv(a.out_h, kTileH), frames), dim3(kBlock), lds,
                       as_stream(stream), a);
    return check_launch(what);
}

template <int NCH>
int launch(const char *what, int frames, int in_h, int in_w, int chans, int rs_h, int rs_w, int crop_x, int crop_y,
           int out_h, int out_w, int flip, int swap_rb, const int32_t *xbounds, const int32_t *xcoeffs, int xksize,
           const int32_t *ybounds, const int32_t *ycoeffs, int yksize, const float *mean, const float *std,
           const uint8_t *src, void *dst, void *stream) {
    SGV3D_REQUIRE(frames > 0 && frames <= 65535 && in_h > 0 && in_w > 0 && rs_h > 0 && rs_w > 0 && out_h > 0 &&
                      out_w > 0 && chans > 0 && chans <= 16,
                  "%s: non-positive or unsupported size", what);
    SGV3D_REQUIRE(in_h <= 4 * rs_h && in_w <= 4 * rs_w, "%s: downscale above 4x (%dx%d -> %dx%d)", what, in_h, in_w,
                  rs_h, rs_w);
    SGV3D_REQUIRE(xksize == ksize_of(in_w, rs_w) && yksize == ksize_of(in_h, rs_h),
                  "%s: coefficient tables do not match the sizes (ksize %d, %d)", what, xksize, yksize);
    SGV3D_REQUIRE(flip == 0 || flip == 1, "%s: flip must be 0 or 1", what);
    SGV3D_REQUIRE(src && dst && xbounds && xcoeffs && ybounds && ycoeffs, "%s: null pointer", what);
    SGV3D_REQUIRE((reinterpret_cast<uintptr_t>(xbounds) & 7) == 0 && (reinterpret_cast<uintptr_t>(ybounds) & 7) == 0,
                  "%s: bounds tables must be 8-byte aligned", what);
    PrepArgs a{};
    a.src = src;
    a.dst = dst;
    a.xb = reinterpret_cast<const int2 *>(xbounds);
    a.xk = xcoeffs;
    a.yb = reinterpret_cast<const int2 *>(ybounds);
    a.yk = ycoeffs;
    a.in_h = in_h, a.in_w = in_w, a.chans = chans;
    a.rs_h = rs_h, a.rs_w = rs_w;
    a.crop_x = crop_x, a.crop_y = crop_y;
    a.out_h = out_h, a.out_w = out_w;
    a.kx = xksize, a.ky = yksize;
    a.flip = flip, a.swap_rb = swap_rb ? 1 : 0;
    a.rows_cap = span_cap(in_h, rs_h, kTileH);
    a.pitch = ((span_cap(in_w, rs_w, kTileW) * chans + 32) + 15) / 16 * 16;
    if (NCH == 3) {
        SGV3D_REQUIRE(mean && std, "%s: null mean / std", what);
        for (int c = 0; c < 3; ++c) {
            SGV3D_REQUIRE(std[c] != 0.0f, "%s: zero std", what);
            a.mean[c] = mean[c];
            a.mul[c] = (float)(1.0 / (double)std[c]);
        }
    }
    const size_t lds = (size_t)a.rows_cap * (a.pitch + kTileW * NCH) + 4 * (size_t)(kTileW * xksize + kTileH * yksize);
    SGV3D_REQUIRE(lds <= 160 * 1024, "%s: tile needs %zu bytes of LDS", what, lds);
    PerDeviceSize &state = NCH == 3 ? g_lds_images : g_lds_mask;
    const int kt = xksize > yksize ? xksize : yksize;   // 5: upscale / scale 1, 7: up to 1.5x down (the DAIR 0.8 resize)
    if (kt <= 5) return launch_kt<NCH, 5>(a, lds, state, what, frames, stream);
    if (kt <= 7) return launch_kt<NCH, 7>(a, lds, state, what, frames, stream);
    if (kt <= 9) return launch_kt<NCH, 9>(a, lds, state, what, frames, stream);
    return launch_kt<NCH, kMaxKsize>(a, lds, state, what, frames, stream);
}

}  // namespace

extern "C" int sgv3d_resample_coeffs(int in_size, int out_size, int32_t *bounds, int32_t *coeffs, int *ksize) {
    SGV3D_REQUIRE(in_size > 0 && out_size > 0, "resample_coeffs: non-positive size (%d -> %d)", in_size, out_size);
    const int ks = ksize_of(in_size, out_size);
    SGV3D_REQUIRE(ks <= kMaxKsize, "resample_coeffs: downscale above 4x (%d -> %d)", in_size, out_size);
    if (ksize) *ksize = ks;
    if (!bounds || !coeffs) return SGV3D_OK;
    // Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c), box = the whole input
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    double w[kMaxKsize];
    for (int o = 0; o < out_size; ++o) {
        const double center = (o + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = bicubic((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        for (int x = 0; x < ks; ++x) {
            double v = x < xmax ? w[x] : 0.0;
            if (x < xmax && ww != 0.0) v /= ww;
            coeffs[(size_t)o * ks + x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecision)) : (int)(0.5 + v * (1 << kPrecision));
        }
        bounds[2 * o] = xmin;
        bounds[2 * o + 1] = xmax;
    }
    return SGV3D_OK;
}

extern "C" int sgv3d_preprocess_images(int frames, int in_h, int in_w, int rs_h, int rs_w, int crop_x, int crop_y,
                                       int out_h, int out_w, int flip, int swap_rb, const int32_t *xbounds,
                                       const int32_t *xcoeffs, int xksize, const int32_t *ybounds, const int32_t *ycoeffs,
                                       int yksize, const float *mean, const float *std, const uint8_t *src, float *dst,
                                       void *stream) {
    return launch<3>("preprocess_images", frames, in_h, in_w, 3, rs_h, rs_w, crop_x, crop_y, out_h, out_w, flip, swap_rb,
                     xbounds, xcoeffs, xksize, ybounds, ycoeffs, yksize, mean, std, src, dst, stream);
}

extern "C" int sgv3d_preprocess_mask(int frames, int in_h, int in_w, int channels, int rs_h, int rs_w, int crop_x,
                                     int crop_y, int out_h, int out_w, int flip, const int32_t *xbounds,
                                     const int32_t *xcoeffs, int xksize, const int32_t *ybounds, const int32_t *ycoeffs,
                                     int yksize, const uint8_t *src, uint8_t *dst, void *stream) {
    return launch<1>("preprocess_mask", frames, in_h, in_w, channels, rs_h, rs_w, crop_x, crop_y, out_h, out_w, flip, 0,
                     xbounds, xcoeffs, xksize, ybounds, ycoeffs, yksize, nullptr, nullptr, src, dst, stream);
}
