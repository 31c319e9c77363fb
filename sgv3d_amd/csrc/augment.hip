// Training-time camera augmentation on the device (dataset/nusc_mv_det_dataset.py get_image with is_train): uint8 HWC
// frames -> the float32 planar tensor BEVHeight.forward takes, and the SGV3D semantic mask -> uint8 labels.
//
// Six launches per batch, whatever its size (A and B are not launched when no frame is rectified):
//   A_h, A_v  intrinsic rectification (:94-110 img_intrin_extrin_transform): Pillow's 8-bit two-pass resampler with the
//             LANCZOS filter to int(W ratio) x int(H ratio), then pasted into / cropped to a black source-sized canvas.
//             Per-frame coefficient tables (the ratio differs per frame), computed on the host
//             (sgv3d_resample_coeffs_filter).  A_v writes the canvas directly: canvas (y, x) = resized (y + off_y,
//             x + off_x), 0 outside.
//   B         Image.rotate(-roll, center, translate=(0, transform_pitch), BICUBIC): Pillow's ImagingGenericTransform with
//             the affine map (double arithmetic, position a0 (x + .5) + a1 (y + .5) + a2, fill where the position is
//             outside the source before the -0.5 shift, border-clamped 4x4 neighbourhood, a = -1 cubic, clamp then
//             truncate to uint8).  The six coefficients come from the host.
//   C_h, C_v  the eval-time bicubic resize + crop of img_transform (:133-161), the same resampler as preprocess.hip;
//             C_v writes uint8 HWC and, for jittered frames, the exact integer sum of cv2's 8-bit BGR2GRAY values.
//   D         brightness (:618-623: beta from the mean gray and the frame's draw u, cv2.convertScaleAbs(img, 1, beta))
//             + mmcv.imnormalize + HWC->CHW.
// Frames that are not rectified skip A and B (C reads the source frame); frames without jitter skip the sum and shift.
// The mask path is A -> B -> C on channel 0, then // 40 (:553-554, :603-614).
//
// Built with -ffp-contract=off: the warp's positions and cubic weights are Pillow's double expressions operation by
// operation, the brightness shift is one float32 add, and the normalise is two float32 roundings.
#include <math.h>

#include <vector>

#include "common.hpp"

using namespace sgv3d;

namespace {

constexpr int kBX = 64, kBY = 4;      // 256 threads: 64 columns x 4 rows of outputs
constexpr int kPrecision = 22;        // Pillow's PRECISION_BITS for 8-bit images

double bicubic_filter(double x) {     // Resample.c bicubic_filter, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

double sinc_filter(double x) {        // Resample.c sinc_filter
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

double lanczos_filter(double x) {     // Resample.c lanczos_filter: truncated sinc, support 3
    if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
    return 0.0;
}

double bilinear_filter(double x) {    // Resample.c bilinear_filter: the triangle, support 1
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

double filter_support(int filter) { return filter == SGV3D_FILTER_LANCZOS ? 3.0 : filter == SGV3D_FILTER_BILINEAR ? 1.0 : 2.0; }

int ksize_of(int filter, int in_size, int out_size) {
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(filter_support(filter) * fs) * 2 + 1;
}

__device__ inline int clip8(int acc) {
    const int v = acc >> kPrecision;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct AugArgs {
    const sgv3d_aug_frame *fr;   // device copy of the per-frame descriptors
    const int32_t *tab;          // per-frame Lanczos tables
    const uint8_t *src;          // [n, H, W, cs]
    uint8_t *w1;                 // [n_rectified, H, W, NCH]: A_h result, then the warped frame
    uint8_t *w2;                 // [n, H, max(W, out_w), NCH]: the canvas, then C_h's result
    uint8_t *u8;                 // images: [n, out_h, out_w, 3] C_v's result
    unsigned long long *sums;    // images: [n] gray sums
    void *dst;                   // images f32 [n, 3, out_h, out_w]; masks u8 [n, out_h, out_w]
    const int32_t *cxb, *cxk, *cyb, *cyk;   // C: bicubic tables (bounds [rs][2], coeffs [rs][k])
    int H, W, cs;
    int rs_h, rs_w, crop_x, crop_y, out_h, out_w, ckx, cky;
    int swap_rb;
    float mean[3], mul[3];
};

__device__ inline size_t frame_px(const AugArgs &a) { return (size_t)a.H * a.W; }
__device__ inline size_t w2_px(const AugArgs &a) { return (size_t)a.H * (a.W > a.out_w ? a.W : a.out_w); }

// A_h: rectified frames' Lanczos horizontal pass over the resized columns the canvas shows,
// [max(off_x, 0), min(W + off_x, rs_w)) -> w1[slot][y][j] (row pitch W).
template <int NCH>
__global__ __launch_bounds__(kBX *kBY) void lanczos_h_kernel(AugArgs a) {
    const sgv3d_aug_frame fr = a.fr[blockIdx.z];
    if (!fr.ie) return;
    const int j = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    const int vx0 = max(fr.off_x, 0), vx1 = min(a.W + fr.off_x, fr.rs_w);
    if (y >= a.H || j >= vx1 - vx0) return;
    const int rx = j + vx0;
    const int32_t *b = a.tab + fr.xtab + 2 * (size_t)rx;
    const int32_t *k = a.tab + fr.xtab + 2 * (size_t)fr.rs_w + (size_t)rx * fr.kx;
    const int x0 = b[0], n = min(b[1], fr.kx);
    const uint8_t *row = a.src + ((size_t)blockIdx.z * frame_px(a) + (size_t)y * a.W) * a.cs;
    int acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = 1 << (kPrecision - 1);
    for (int t = 0; t < n; ++t) {
        const int x = min(max(x0 + t, 0), a.W - 1);
        const int wk = k[t];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] += (int)row[(size_t)x * a.cs + c] * wk;
    }
    uint8_t *o = a.w1 + ((size_t)fr.slot * frame_px(a) + (size_t)y * a.W + j) * NCH;
#pragma unroll
    for (int c = 0; c < NCH; ++c) o[c] = (uint8_t)clip8(acc[c]);
}

// A_v: the vertical pass written straight into the source-sized canvas w2[f] (paste / crop, black outside).
template <int NCH>
__global__ __launch_bounds__(kBX *kBY) void lanczos_v_kernel(AugArgs a) {
    const sgv3d_aug_frame fr = a.fr[blockIdx.z];
    if (!fr.ie) return;
    const int x = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const int rx = x + fr.off_x, ry = y + fr.off_y;
    int v[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) v[c] = 0;
    if (rx >= 0 && rx < fr.rs_w && ry >= 0 && ry < fr.rs_h) {
        const int j = rx - max(fr.off_x, 0);
        const int32_t *b = a.tab + fr.ytab + 2 * (size_t)ry;
        const int32_t *k = a.tab + fr.ytab + 2 * (size_t)fr.rs_h + (size_t)ry * fr.ky;
        const int y0 = b[0], n = min(b[1], fr.ky);
        const uint8_t *col = a.w1 + ((size_t)fr.slot * frame_px(a) + j) * NCH;
        int acc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = 1 << (kPrecision - 1);
        for (int t = 0; t < n; ++t) {
            const int yy = min(max(y0 + t, 0), a.H - 1);
            const int wk = k[t];
            const uint8_t *p = col + (size_t)yy * a.W * NCH;
#pragma unroll
            for (int c = 0; c < NCH; ++c) acc[c] += (int)p[c] * wk;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = clip8(acc[c]);
    }
    uint8_t *o = a.w2 + ((size_t)blockIdx.z * w2_px(a) + (size_t)y * a.W + x) * NCH;
#pragma unroll
    for (int c = 0; c < NCH; ++c) o[c] = (uint8_t)v[c];
}

// Geometry.c BICUBIC: p1 + d (p2 + d (p3 + d p4)), a = -1
__device__ inline double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2;
    const double p2 = -v1 + v3;
    const double p3 = 2 * (v1 - v2) + v3 - v4;
    const double p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

// B: Image.rotate of the canvas w2[f] -> w1[slot]
template <int NCH>
__global__ __launch_bounds__(kBX *kBY) void warp_kernel(AugArgs a) {
    const sgv3d_aug_frame fr = a.fr[blockIdx.z];
    if (!fr.ie) return;
    const int x = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const double xo = x + 0.5, yo = y + 0.5;
    double xin = fr.affine[0] * xo + fr.affine[1] * yo + fr.affine[2];
    double yin = fr.affine[3] * xo + fr.affine[4] * yo + fr.affine[5];
    uint8_t *o = a.w1 + ((size_t)fr.slot * frame_px(a) + (size_t)y * a.W + x) * NCH;
    if (!(xin >= 0.0 && xin < a.W && yin >= 0.0 && yin < a.H)) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) o[c] = 0;
        return;
    }
    xin -= 0.5;
    yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const double dx = xin - fx, dy = yin - fy;
    const int ix = (int)fx - 1, iy = (int)fy - 1;
    int cols[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cols[i] = min(max(ix + i, 0), a.W - 1);
    const uint8_t *img = a.w2 + (size_t)blockIdx.z * w2_px(a) * NCH;
    double r[4][NCH];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint8_t *row = img + (size_t)min(max(iy + j, 0), a.H - 1) * a.W * NCH;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            r[j][c] = cubic(row[cols[0] * NCH + c], row[cols[1] * NCH + c], row[cols[2] * NCH + c],
                            row[cols[3] * NCH + c], dx);
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const double v = cubic(r[0][c], r[1][c], r[2][c], r[3][c], dy);
        o[c] = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (uint8_t)v);
    }
}

// C_h: bicubic horizontal pass over the crop's columns [max(crop_x, 0), min(crop_x + out_w, rs_w)) of the eval resize,
// reading the warped frame (rectified) or the source frame -> w2[f][y][j] (row pitch out_w).  Also zeroes the gray sums.
template <int NCH>
__global__ __launch_bounds__(kBX *kBY) void bicubic_h_kernel(AugArgs a) {
    const sgv3d_aug_frame fr = a.fr[blockIdx.z];
    const int j = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    if (a.sums && j == 0 && y == 0) a.sums[blockIdx.z] = 0ull;
    const int vx0 = max(a.crop_x, 0), vx1 = min(a.crop_x + a.out_w, a.rs_w);
    if (y >= a.H || j >= vx1 - vx0) return;
    const int rx = j + vx0;
    const int x0 = a.cxb[2 * rx], n = min(a.cxb[2 * rx + 1], a.ckx);
    const int32_t *k = a.cxk + (size_t)rx * a.ckx;
    const uint8_t *row;
    int stride;
    if (fr.ie) {
        row = a.w1 + ((size_t)fr.slot * frame_px(a) + (size_t)y * a.W) * NCH;
        stride = NCH;
    } else {
        row = a.src + ((size_t)blockIdx.z * frame_px(a) + (size_t)y * a.W) * a.cs;
        stride = a.cs;
    }
    int acc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc[c] = 1 << (kPrecision - 1);
    for (int t = 0; t < n; ++t) {
        const int x = min(max(x0 + t, 0), a.W - 1);
        const int wk = k[t];
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] += (int)row[(size_t)x * stride + c] * wk;
    }
    uint8_t *o = a.w2 + ((size_t)blockIdx.z * w2_px(a) + (size_t)y * a.out_w + j) * NCH;
#pragma unroll
    for (int c = 0; c < NCH; ++c) o[c] = (uint8_t)clip8(acc[c]);
}

// C_v: vertical pass + crop -> images: u8[f] HWC and the gray sum of jittered frames; masks: labels // 40
template <int NCH>
__global__ __launch_bounds__(kBX *kBY) void bicubic_v_kernel(AugArgs a) {
    __shared__ unsigned long long part[kBX * kBY / kWave];
    const sgv3d_aug_frame fr = a.fr[blockIdx.z];
    const int x = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    unsigned gray = 0;
    if (x < a.out_w && y < a.out_h) {
        const int rx = x + a.crop_x, ry = y + a.crop_y;
        int v[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) v[c] = 0;
        if (rx >= 0 && rx < a.rs_w && ry >= 0 && ry < a.rs_h) {
            const int j = rx - max(a.crop_x, 0);
            const int y0 = a.cyb[2 * ry], n = min(a.cyb[2 * ry + 1], a.cky);
            const int32_t *k = a.cyk + (size_t)ry * a.cky;
            const uint8_t *col = a.w2 + ((size_t)blockIdx.z * w2_px(a) + j) * NCH;
            int acc[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) acc[c] = 1 << (kPrecision - 1);
            for (int t = 0; t < n; ++t) {
                const int yy = min(max(y0 + t, 0), a.H - 1);
                const int wk = k[t];
                const uint8_t *p = col + (size_t)yy * a.out_w * NCH;
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] += (int)p[c] * wk;
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) v[c] = clip8(acc[c]);
        }
        const size_t o = (size_t)blockIdx.z * a.out_h * a.out_w + (size_t)y * a.out_w + x;
        if (NCH == 3) {
            uint8_t *p = a.u8 + o * 3;
#pragma unroll
            for (int c = 0; c < NCH; ++c) p[c] = (uint8_t)v[c];
            // cv2 COLOR_BGR2GRAY, 8-bit fixed point, on RGB-ordered data: channel 0 takes the B weight
            gray = (unsigned)((v[0] * 1868 + v[1 % NCH] * 9617 + v[2 % NCH] * 4899 + 8192) >> 14);
        } else {
            static_cast<uint8_t *>(a.dst)[o] = (uint8_t)(v[0] / 40);
        }
    }
    if (NCH != 3 || !fr.bright) return;
    unsigned long long s = gray;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) s += __shfl_down(s, off, kWave);
    const int tid = threadIdx.y * kBX + threadIdx.x;
    if ((tid & (kWave - 1)) == 0) part[tid / kWave] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int i = 0; i < kBX * kBY / kWave; ++i) t += part[i];
        atomicAdd(a.sums + blockIdx.z, t);
    }
}

// D: brightness + normalise + HWC -> CHW; thread = 4 consecutive pixels of one row
__global__ __launch_bounds__(kBX *kBY) void normalize_kernel(AugArgs a) {
    const sgv3d_aug_frame fr = a.fr[blockIdx.z];
    const int x0 = (blockIdx.x * kBX + threadIdx.x) * 4, y = blockIdx.y * kBY + threadIdx.y;
    if (x0 >= a.out_w || y >= a.out_h) return;
    float shift = 0.0f;
    if (fr.bright) {
        const double npix = (double)a.out_h * (double)a.out_w;
        const double mean = (double)a.sums[blockIdx.z] / npix;
        double beta = fr.u * (100 - mean);
        const double mag = fabs(beta) < 50.0 ? fabs(beta) : 50.0;
        beta = beta > 0 ? mag : -mag;
        shift = (float)beta;
    }
    const size_t plane = (size_t)a.out_h * a.out_w;
    const size_t o = (size_t)y * a.out_w + x0;
    const uint8_t *p = a.u8 + ((size_t)blockIdx.z * plane + o) * 3;
    const int nq = min(4, a.out_w - x0);
    float *dst = static_cast<float *>(a.dst) + (size_t)blockIdx.z * 3 * plane + o;
    float v[4][3];
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float x = q < nq ? (float)p[q * 3 + c] : 0.0f;
            if (fr.bright) {   // cv2.convertScaleAbs: saturate_cast<uchar>(|x * 1 + beta|), rounding to nearest even
                x = rintf(fabsf(x * 1.0f + shift));
                x = x > 255.0f ? 255.0f : x;
            }
            v[q][c] = x;
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sc = a.swap_rb ? 2 - c : c;
        float yv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) yv[q] = (v[q][sc] - a.mean[c]) * a.mul[c];
        float *d = dst + c * plane;
        if (nq == 4 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
            *reinterpret_cast<float4 *>(d) = make_float4(yv[0], yv[1], yv[2], yv[3]);
        } else {
            for (int q = 0; q < nq; ++q) d[q] = yv[q];
        }
    }
}

struct Sizes {
    size_t sums, u8, w2, w1, total;
};

Sizes workspace_sizes(int frames, int rectified, int in_h, int in_w, int out_h, int out_w, int nch) {
    Sizes s{};
    const size_t align = 256;
    auto up = [&](size_t v) { return (v + align - 1) / align * align; };
    s.sums = nch == 3 ? up(8 * (size_t)frames) : 0;
    s.u8 = nch == 3 ? up((size_t)frames * out_h * out_w * 3) : 0;
    s.w2 = up((size_t)frames * in_h * (size_t)(in_w > out_w ? in_w : out_w) * nch);
    s.w1 = up((size_t)rectified * in_h * in_w * nch);
    s.total = s.sums + s.u8 + s.w2 + s.w1;
    return s;
}

template <int NCH>
int launch(const char *what, int frames, int in_h, int in_w, int chans, const sgv3d_aug_frame *fh,
           const sgv3d_aug_frame *fd, const int32_t *tables, long long tables_len, int rs_h, int rs_w, int crop_x,
           int crop_y, int out_h, int out_w, int swap_rb, const int32_t *xbounds, const int32_t *xcoeffs, int xksize,
           const int32_t *ybounds, const int32_t *ycoeffs, int yksize, const float *mean, const float *std,
           const uint8_t *src, void *work, size_t work_bytes, void *dst, void *stream) {
    SGV3D_REQUIRE(frames > 0 && frames <= 65535 && in_h > 0 && in_w > 0 && rs_h > 0 && rs_w > 0 && out_h > 0 &&
                      out_w > 0 && chans >= NCH && chans <= 16,
                  "%s: non-positive or unsupported size", what);
    SGV3D_REQUIRE(xksize == ksize_of(SGV3D_FILTER_BICUBIC, in_w, rs_w) &&
                      yksize == ksize_of(SGV3D_FILTER_BICUBIC, in_h, rs_h),
                  "%s: resize coefficient tables do not match the sizes (ksize %d, %d)", what, xksize, yksize);
    SGV3D_REQUIRE(fh && fd && src && dst && xbounds && xcoeffs && ybounds && ycoeffs && tables_len >= 0,
                  "%s: null pointer", what);
    int rectified = 0;
    for (int f = 0; f < frames; ++f) {
        const sgv3d_aug_frame &r = fh[f];
        SGV3D_REQUIRE((r.ie == 0 || r.ie == 1) && (r.bright == 0 || r.bright == 1), "%s: frame %d: ie / bright must be 0 "
                      "or 1", what, f);
        SGV3D_REQUIRE(NCH == 3 || !r.bright, "%s: frame %d: masks take no brightness jitter", what, f);
        if (r.bright) SGV3D_REQUIRE(isfinite(r.u), "%s: frame %d: non-finite u", what, f);
        if (!r.ie) continue;
        SGV3D_REQUIRE(r.rs_w > 0 && r.rs_h > 0, "%s: frame %d: resized size %dx%d below one pixel", what, f, r.rs_h,
                      r.rs_w);
        SGV3D_REQUIRE(r.kx == ksize_of(SGV3D_FILTER_LANCZOS, in_w, r.rs_w) &&
                          r.ky == ksize_of(SGV3D_FILTER_LANCZOS, in_h, r.rs_h),
                      "%s: frame %d: Lanczos tables do not match the sizes", what, f);
        SGV3D_REQUIRE(r.xtab >= 0 && r.xtab + (long long)r.rs_w * (2 + r.kx) <= tables_len && r.ytab >= 0 &&
                          r.ytab + (long long)r.rs_h * (2 + r.ky) <= tables_len,
                      "%s: frame %d: Lanczos tables out of range", what, f);
        SGV3D_REQUIRE(r.slot == rectified, "%s: frame %d: slot %d, expected %d (rectified frames in order)", what, f,
                      r.slot, rectified);
        for (int i = 0; i < 6; ++i) SGV3D_REQUIRE(isfinite(r.affine[i]), "%s: frame %d: non-finite affine", what, f);
        ++rectified;
    }
    SGV3D_REQUIRE(rectified == 0 || tables, "%s: null tables", what);
    const Sizes s = workspace_sizes(frames, rectified, in_h, in_w, out_h, out_w, NCH);
    SGV3D_REQUIRE(work, "%s: null workspace", what);
    if (work_bytes < s.total) return fail(SGV3D_ENOSPACE, "%s: workspace of %zu bytes, need %zu", what, work_bytes, s.total);
    SGV3D_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7) == 0, "%s: workspace must be 8-byte aligned", what);
    AugArgs a{};
    a.fr = fd;
    a.tab = tables;
    a.src = src;
    uint8_t *w = static_cast<uint8_t *>(work);
    a.sums = NCH == 3 ? reinterpret_cast<unsigned long long *>(w) : nullptr;
    a.u8 = NCH == 3 ? w + s.sums : nullptr;
    a.w2 = w + s.sums + s.u8;
    a.w1 = w + s.sums + s.u8 + s.w2;
    a.dst = dst;
    a.cxb = xbounds, a.cxk = xcoeffs, a.cyb = ybounds, a.cyk = ycoeffs;
    a.H = in_h, a.W = in_w, a.cs = chans;
    a.rs_h = rs_h, a.rs_w = rs_w, a.crop_x = crop_x, a.crop_y = crop_y, a.out_h = out_h, a.out_w = out_w;
    a.ckx = xksize, a.cky = yksize;
    a.swap_rb = swap_rb ? 1 : 0;
    if (NCH == 3) {
        SGV3D_REQUIRE(mean && std, "%s: null mean / std", what);
        for (int c = 0; c < 3; ++c) {
            SGV3D_REQUIRE(std[c] != 0.0f, "%s: zero std", what);
            a.mean[c] = mean[c];
            a.mul[c] = (float)(1.0 / (double)std[c]);
        }
    }
    hipStream_t st = as_stream(stream);
    const dim3 blk(kBX, kBY);
    const dim3 src_grid(cdiv(in_w, kBX), cdiv(in_h, kBY), frames);
    if (rectified) {
        hipLaunchKernelGGL(lanczos_h_kernel<NCH>, src_grid, blk, 0, st, a);
        hipLaunchKernelGGL(lanczos_v_kernel<NCH>, src_grid, blk, 0, st, a);
        hipLaunchKernelGGL(warp_kernel<NCH>, src_grid, blk, 0, st, a);
    }
    hipLaunchKernelGGL(bicubic_h_kernel<NCH>, dim3(cdiv(out_w, kBX), cdiv(in_h, kBY), frames), blk, 0, st, a);
    hipLaunchKernelGGL(bicubic_v_kernel<NCH>, dim3(cdiv(out_w, kBX), cdiv(out_h, kBY), frames), blk, 0, st, a);
    if (NCH == 3)
        hipLaunchKernelGGL(normalize_kernel, dim3(cdiv(out_w, 4 * kBX), cdiv(out_h, kBY), frames), blk, 0, st, a);
    return check_launch(what);
}

}  // namespace

extern "C" int sgv3d_resample_coeffs_filter(int filter, int in_size, int out_size, int32_t *bounds, int32_t *coeffs,
                                            int *ksize) {
    SGV3D_REQUIRE(filter == SGV3D_FILTER_BICUBIC || filter == SGV3D_FILTER_LANCZOS || filter == SGV3D_FILTER_BILINEAR,
                  "resample_coeffs_filter: unknown filter %d", filter);
    SGV3D_REQUIRE(in_size > 0 && out_size > 0, "resample_coeffs_filter: non-positive size (%d -> %d)", in_size,
                  out_size);
    const int ks = ksize_of(filter, in_size, out_size);
    if (ksize) *ksize = ks;
    if (!bounds || !coeffs) return SGV3D_OK;
    // Pillow's precompute_coeffs + normalize_coeffs_8bpc (Resample.c), box = the whole input
    double (*fn)(double) = filter == SGV3D_FILTER_LANCZOS ? lanczos_filter : filter == SGV3D_FILTER_BILINEAR ? bilinear_filter : bicubic_filter;
    const double scale = (double)in_size / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(filter) * fs, ss = 1.0 / fs;
    std::vector<double> w(ks);
    for (int o = 0; o < out_size; ++o) {
        const double center = (o + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = fn((x + xmin - center + 0.5) * ss);
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

extern "C" size_t sgv3d_augment_workspace_bytes(int frames, int rectified, int in_h, int in_w, int out_h, int out_w,
                                                int mask) {
    if (frames <= 0 || rectified < 0 || rectified > frames || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0)
        return 0;
    return workspace_sizes(frames, rectified, in_h, in_w, out_h, out_w, mask ? 1 : 3).total;
}

extern "C" int sgv3d_augment_images(int frames, int in_h, int in_w, const sgv3d_aug_frame *frames_host,
                                    const sgv3d_aug_frame *frames_dev, const int32_t *tables, long long tables_len,
                                    int rs_h, int rs_w, int crop_x, int crop_y, int out_h, int out_w, int swap_rb,
                                    const int32_t *xbounds, const int32_t *xcoeffs, int xksize, const int32_t *ybounds,
                                    const int32_t *ycoeffs, int yksize, const float *mean, const float *std,
                                    const uint8_t *src, void *work, size_t work_bytes, float *dst, void *stream) {
    return launch<3>("augment_images", frames, in_h, in_w, 3, frames_host, frames_dev, tables, tables_len, rs_h, rs_w,
                     crop_x, crop_y, out_h, out_w, swap_rb, xbounds, xcoeffs, xksize, ybounds, ycoeffs, yksize, mean,
                     std, src, work, work_bytes, dst, stream);
}

extern "C" int sgv3d_augment_mask(int frames, int in_h, int in_w, int channels, const sgv3d_aug_frame *frames_host,
                                  const sgv3d_aug_frame *frames_dev, const int32_t *tables, long long tables_len,
                                  int rs_h, int rs_w, int crop_x, int crop_y, int out_h, int out_w,
                                  const int32_t *xbounds, const int32_t *xcoeffs, int xksize, const int32_t *ybounds,
                                  const int32_t *ycoeffs, int yksize, const uint8_t *src, void *work, size_t work_bytes,
                                  uint8_t *dst, void *stream) {
    return launch<1>("augment_mask", frames, in_h, in_w, channels, frames_host, frames_dev, tables, tables_len, rs_h,
                     rs_w, crop_x, crop_y, out_h, out_w, 0, xbounds, xcoeffs, xksize, ybounds, ycoeffs, yksize,
                     nullptr, nullptr, src, work, work_bytes, dst, stream);
}
