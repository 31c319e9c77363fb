// Frame recombination on the device: the data generation step of SGV3D's semi-supervised pipeline
// (scripts/data_preprocess/recombine_utils.py: get_M, transform_with_M_bilinear, unify_extrinsic_params_tools,
// update_bbox_info, iou, objects_combine_tools, label_generation).  Up to three labeled or pseudo-labeled source frames
// are warped into the camera of a destination frame, matched to its brightness, their objects gated by 2-D IoU against
// the boxes accepted so far, the accepted objects' pixels and class ids pasted over the destination, and the labels of
// the generated frame written in the destination camera.
//
// Four launches per batch of generated frames, whatever the number of sources:
//   1  gray partials: every source warped in full (float64 bilinear, rounded to float32 once), its float32 gray summed
//      in float64 per workgroup in a fixed order; the destination's 8-bit gray summed in integers (grid z = source).
//   2  one wave per generated frame: the partials reduced in index order, beta per source, every object's 2-D box, and
//      the serial gate walk; each object's maximum IoU is taken wave-parallel over the accepted list.
//   3  per destination pixel, the sources in order: inside an accepted box of the source -> warp position -> the
//      source's class-id mask, nearest neighbour -> if non-zero, the warped, brightness-shifted pixel and the id
//      overwrite what is there.  Pixels outside every accepted box never compute a warp.
//   4  labels of the destination's own objects and of the accepted ones, rounded as the label text rounds them.
// No atomics anywhere: a launch is repeatable bit for bit.
//
// The class-id masks stand in for SAM: the reference prompts SAM with the accepted boxes; here the caller supplies each
// frame's stored class-id mask (mask_image // 40, the product of the reference's first stage), which is warped with the
// frame and kept inside the union of the source's accepted boxes.
//
// Every arithmetic step is a __host__ __device__ function shared with sgv3d_recombine_host, which also walks the
// partial sums in the kernels' order.  Built with -ffp-contract=off: float64 expressions round once per operation, as
// numpy's do; the one fused operation is the explicit fma of the decimal rounding (round_decimals.hpp).
#include <math.h>

#include <vector>

#include "common.hpp"
#include "round_decimals.hpp"

namespace {

using sgv3d::as_stream;
using sgv3d::cdiv;
using sgv3d::check_launch;
using sgv3d::kWave;
using sgv3d::round4;

constexpr int kBX = 64, kBY = 4;               // launch 1: 64 x 4 pixels, one per thread; a wave is one row of the tile
constexpr int kPX = 4;                         // launch 3: four consecutive pixels per thread
constexpr int kSrc = SGV3D_RECOMBINE_MAX_SOURCES;
constexpr int kObjCols = 30;                   // corners [3][8] | dim h, w, l | truncated | occluded | score
constexpr int kRowCols = 15;                   // truncated, occluded, alpha, x1, y1, x2, y2, h, w, l, x, y, z, rotation_y, score
constexpr int kFocus = 6;                      // classes 0..5: car, van, truck, bus, pedestrian, cyclist (cls_focus)

#define HD __host__ __device__ inline

// ---------------------------------------------------------------------------------------------------------------- warp
// transform_with_M_bilinear's position of destination pixel (u, v) in the source: p = Minv . (10u, 10v, 10), q = p.xy /
// p.z, the dead flag on the unclipped q, then q clipped to [0, W-2] x [0, H-2].  A non-finite q (the reference would
// fail on its index) is dead.
HD bool warp_position(const double *mi, int u, int v, int W, int H, double *qx, double *qy) {
    const double x = (double)u * 10.0, y = (double)v * 10.0, z = 10.0;
    const double px = (mi[0] * x + mi[1] * y) + mi[2] * z;
    const double py = (mi[3] * x + mi[4] * y) + mi[5] * z;
    const double pz = (mi[6] * x + mi[7] * y) + mi[8] * z;
    double cx = px / pz, cy = py / pz;
    const double mx = (double)(W - 2), my = (double)(H - 2);
    if (!(isfinite(cx) && isfinite(cy))) {
        *qx = 0.0;
        *qy = 0.0;
        return true;
    }
    const bool dead = cx < 0.0 || cx > mx || cy < 0.0 || cy > my;
    cx = cx < 0.0 ? 0.0 : (cx > mx ? mx : cx);
    cy = cy < 0.0 ? 0.0 : (cy > my ? my : cy);
    *qx = cx;
    *qy = cy;
    return dead;
}

// The bilinear blend of one channel: the two rows along the column fraction first (fr1, fr2), then the rows along the
// row fraction (image_new); rounded to float32 once.  c0 <= W-2 and r0 <= H-2, so the +1 neighbours exist.
HD float bilinear(const uint8_t *img, int W, int ch, double qx, double qy) {
    const double fc = floor(qx), fr = floor(qy);
    const int c0 = (int)fc, r0 = (int)fr;
    const uint8_t *p = img + ((size_t)r0 * W + c0) * 3 + ch;
    const double wl = (double)(c0 + 1) - qx, wr = qx - (double)c0;
    const double fr1 = wl * (double)p[0] + wr * (double)p[3];
    const double fr2 = wl * (double)p[(size_t)W * 3] + wr * (double)p[(size_t)W * 3 + 3];
    return (float)(((double)(r0 + 1) - qy) * fr1 + (qy - (double)r0) * fr2);
}

// cv2.cvtColor(float32, COLOR_BGR2GRAY) on RGB-ordered data: channel 2 is B
HD float gray_f32(float r, float g, float b) { return (0.114f * b + 0.587f * g) + 0.299f * r; }
// cv2.cvtColor(uint8, COLOR_BGR2GRAY): 14-bit fixed point, as augment.hip restates it
HD unsigned gray_u8(unsigned r, unsigned g, unsigned b) { return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14; }
// cv2.convertScaleAbs(x, alpha=1, beta): saturate_cast<uchar>(|x + beta|), ties to even; NaN -> 0
HD uint8_t shift_u8(float x, float beta) {
    const float v = rintf(fabsf(x + beta));
    return !(v > 0.0f) ? 0 : (v > 255.0f ? 255 : (uint8_t)v);
}

// beta = 100 (b_d - b_s) / b_s, magnitude capped at 60 with Python's min (a NaN stays), sign kept
HD double beta_of(double bd, double bs) {
    const double beta = 100.0 * (bd - bs) / bs;
    const double a = fabs(beta);
    const double mag = 60.0 < a ? 60.0 : a;
    return beta > 0.0 ? mag : -mag;
}

// --------------------------------------------------------------------------------------------------------------- boxes
HD double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
HD double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// Corner k of object `o` (corners stored [3][8]) plus delta, through Tr (3x4, homogeneous 1) -> camera frame
HD void camera_corner(const double *o, int k, const double *delta, const double *tr, double *c) {
    double x = o[k], y = o[8 + k], z = o[16 + k];
    if (delta) {
        x = x + delta[0];
        y = y + delta[1];
        z = z + delta[2];
    }
    c[0] = ((tr[0] * x + tr[1] * y) + tr[2] * z) + tr[3];
    c[1] = ((tr[4] * x + tr[5] * y) + tr[6] * z) + tr[7];
    c[2] = ((tr[8] * x + tr[9] * y) + tr[10] * z) + tr[11];
}

// update_bbox_info: the eight corners projected with P2, min and max (a NaN stays, as in numpy), dropped when xmax <= 0
// or ymax <= 0, minima clamped with Python's max(0, v).  box = xmin, ymin, xmax, ymax; returns false when dropped.
// *clamped: bit 0 / 1 set when xmin / ymin became the integer 0 (the label text then reads "0").
HD bool float_box(const double *o, const double *delta, const double *tr, const double *p2, double *box, int *clamped) {
    double x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    for (int k = 0; k < 8; ++k) {
        double c[3];
        camera_corner(o, k, delta, tr, c);
        const double hx = ((p2[0] * c[0] + p2[1] * c[1]) + p2[2] * c[2]) + p2[3];
        const double hy = ((p2[4] * c[0] + p2[5] * c[1]) + p2[6] * c[2]) + p2[7];
        const double hz = ((p2[8] * c[0] + p2[9] * c[1]) + p2[10] * c[2]) + p2[11];
        const double u = hx / hz, v = hy / hz;
        if (k == 0) {
            x0 = x1 = u;
            y0 = y1 = v;
        } else {
            x0 = np_min(x0, u);
            x1 = np_max(x1, u);
            y0 = np_min(y0, v);
            y1 = np_max(y1, v);
        }
    }
    *clamped = (!(x0 > 0.0) ? 1 : 0) | (!(y0 > 0.0) ? 2 : 0);
    box[0] = x0 > 0.0 ? x0 : 0.0;
    box[1] = y0 > 0.0 ? y0 : 0.0;
    box[2] = x1;
    box[3] = y1;
    return !(x1 <= 0.0 || y1 <= 0.0);
}

// astype(np.int32): truncation; what does not fit (NaN included) gives INT32_MIN, as the x86 conversion does
HD int trunc_i32(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (int)0x80000000; }

// The integer box the gate tests and the mask is kept inside; false for degenerate boxes
HD bool int_box(const double *box, int W, int H, int *ib) {
    int xmin = trunc_i32(box[0]), ymin = trunc_i32(box[1]), xmax = trunc_i32(box[2]), ymax = trunc_i32(box[3]);
    if (xmax <= 0 || ymax <= 0) return false;
    xmin = xmin > 0 ? xmin : 0;
    ymin = ymin > 0 ? ymin : 0;
    xmax = xmax < W - 1 ? xmax : W - 1;
    ymax = ymax < H - 1 ? ymax : H - 1;
    if (xmax <= xmin || ymax <= ymin || xmax - xmin <= 1 || ymax - ymin <= 1) return false;
    ib[0] = xmin, ib[1] = ymin, ib[2] = xmax, ib[3] = ymax;
    return true;
}

// iou(a[None], b[None]): intersection over (area_a + area_b - intersection + 10e-9)
HD double box_iou(const double *a, const double *b) {
    const double zero = 0.0;
    const double ih = np_max(zero, np_min(a[2], b[2]) - np_max(a[0], b[0]));
    const double iw = np_max(zero, np_min(a[3], b[3]) - np_max(a[1], b[1]));
    const double inter = ih * iw;
    const double aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / (((aa + ab) - inter) + 10e-9);
}

// label_generation: one row of kRowCols values, rounded
HD void label_row(const double *o, const double *delta, const double *tr, const double *fbox, double *out) {
    double c[8][3];
    for (int k = 0; k < 8; ++k) camera_corner(o, k, delta, tr, c[k]);
    double loc[3];
    for (int a = 0; a < 3; ++a) {                               // np.mean over the eight corners: numpy's pairwise tree
        const double s = ((c[0][a] + c[1][a]) + (c[2][a] + c[3][a])) + ((c[4][a] + c[5][a]) + (c[6][a] + c[7][a]));
        loc[a] = s / 8.0;
    }
    const double h = o[24], w = o[25], l = o[26];
    loc[1] = loc[1] + h / 2.0;
    const double dx = c[0][0] - c[3][0], dz = c[0][2] - c[3][2];
    const double rotation = atan2(-dz, dx);
    const double pi = 3.141592653589793;
    double alpha = rotation - atan2(loc[0], loc[2]);
    if (alpha > pi) alpha = alpha - 2.0 * pi;
    if (alpha <= -1.0 * pi) alpha = alpha + 2.0 * pi;
    const double at = atan(tan(alpha));                         // normalize_angle
    alpha = cos(alpha) < 0.0 ? at + pi : at;
    out[0] = o[27];
    out[1] = o[28];
    out[2] = round4(alpha);
    for (int k = 0; k < 4; ++k) out[3 + k] = round4(fbox[k]);
    out[7] = round4(h);
    out[8] = round4(w);
    out[9] = round4(l);
    for (int k = 0; k < 3; ++k) out[10 + k] = round4(loc[k]);
    out[13] = round4(rotation);
    out[14] = round4(o[29]);
}

// ------------------------------------------------------------------------------------------------------------ workspace
struct Layout {
    size_t gray, dgray, acc, ibox, cbox, cstart, row_of, flags, total;
    int tiles;
};

Layout layout_of(int batch, int h, int w, int max_obj) {
    Layout L{};
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    L.tiles = cdiv(w, kBX) * cdiv(h, kBY);
    size_t o = 0;
    L.gray = o, o += up((size_t)batch * kSrc * L.tiles * sizeof(double));          // float64 gray partial of every tile
    L.dgray = o, o += up((size_t)batch * L.tiles * sizeof(unsigned long long));    // integer gray partials of the destination
    L.acc = o, o += up((size_t)batch * (max_obj + 1) * 4 * sizeof(double));        // the accepted list (init_bboxes)
    L.ibox = o, o += up((size_t)batch * max_obj * 4 * sizeof(int32_t));            // integer box per object
    L.cbox = o, o += up((size_t)batch * max_obj * 4 * sizeof(int32_t));            // accepted integer boxes, compact, by source
    L.cstart = o, o += up((size_t)batch * (kSrc + 1) * sizeof(int32_t));           // their range per source
    L.row_of = o, o += up((size_t)batch * max_obj * sizeof(int32_t));              // label row of every object, -1: none
    L.flags = o, o += up((size_t)batch * max_obj * sizeof(int32_t));               // candidate bit 4 | clamped bits 0, 1
    L.total = o;
    return L;
}

struct Args {
    const sgv3d_recombine_frame *fr;
    const uint8_t *images, *masks;
    const double *objects;
    const int32_t *classes;
    double *gray;
    unsigned long long *dgray;
    double *acc;
    int32_t *ibox, *cbox, *cstart, *row_of, *flags;
    uint8_t *out_images, *out_masks;
    double *beta, *boxes, *rows;
    int32_t *kept, *n_rows, *row_info;
    int H, W, max_obj, tiles;
};

// ------------------------------------------------------------------------------------------------------------- launch 1
__global__ __launch_bounds__(kBX *kBY) void gray_partials_kernel(Args a, int batch) {
    __shared__ double part[kBY];
    __shared__ unsigned long long ipart[kBY];
    const int z = blockIdx.z;
    const bool is_dest = z >= batch * kSrc;
    const int b = is_dest ? z - batch * kSrc : z / kSrc, s = is_dest ? 0 : z % kSrc;
    const sgv3d_recombine_frame &fr = a.fr[b];
    if (!is_dest && s >= fr.n_src) return;                      // block-uniform: nothing of this slice is ever read
    const int x = blockIdx.x * kBX + threadIdx.x, y = blockIdx.y * kBY + threadIdx.y;
    const bool inside = x < a.W && y < a.H;
    const size_t px = (size_t)a.H * a.W;
    const int tile = blockIdx.y * gridDim.x + blockIdx.x;
    if (is_dest) {
        unsigned long long g = 0;
        if (inside) {
            const uint8_t *p = a.images + ((size_t)fr.dest * px + (size_t)y * a.W + x) * 3;
            g = gray_u8(p[0], p[1], p[2]);
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) g += __shfl_down(g, off, kWave);
        if (threadIdx.x == 0) ipart[threadIdx.y] = g;
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0) {
            unsigned long long t = 0;
            for (int i = 0; i < kBY; ++i) t += ipart[i];
            a.dgray[(size_t)b * a.tiles + tile] = t;
        }
        return;
    }
    double g = 0.0;
    if (inside) {
        double qx, qy;
        if (!warp_position(fr.minv[s], x, y, a.W, a.H, &qx, &qy)) {
            const uint8_t *img = a.images + (size_t)fr.src[s] * px * 3;
            g = (double)gray_f32(bilinear(img, a.W, 0, qx, qy), bilinear(img, a.W, 1, qx, qy), bilinear(img, a.W, 2, qx, qy));
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) g = g + __shfl_down(g, off, kWave);   // lane 0: the fixed tree of 64
    if (threadIdx.x == 0) part[threadIdx.y] = g;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        double t = 0.0;
        for (int i = 0; i < kBY; ++i) t = t + part[i];
        a.gray[((size_t)b * kSrc + s) * a.tiles + tile] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------- launch 2
// The reduce both sides run: lane i sums elements i, i + 64, i + 128, ... in order (coalesced, and the loads of one lane do
// not depend on each other), then the 64 lane sums are added in lane order.
template <typename T>
HD T lane_sum_of(const T *p, int n, int lane) {
    T t = 0;
#pragma unroll 8
    for (int i = lane; i < n; i += kWave) t = t + p[i];
    return t;
}

__global__ __launch_bounds__(kWave) void gate_kernel(Args a) {
    __shared__ double lane_sum[kWave];
    __shared__ unsigned long long lane_isum[kWave];
    const int b = blockIdx.x, lane = threadIdx.x;
    const sgv3d_recombine_frame &fr = a.fr[b];
    const double npix = (double)a.H * (double)a.W;

    // brightness: the destination's mean gray, then beta of every source
    lane_isum[lane] = lane_sum_of(a.dgray + (size_t)b * a.tiles, a.tiles, lane);
    __syncthreads();
    unsigned long long dsum = 0;
    for (int i = 0; i < kWave; ++i) dsum += lane_isum[i];
    const double bd = (double)dsum / npix;
    for (int s = 0; s < kSrc; ++s) {
        double beta = 0.0;
        if (s < fr.n_src) {
            __syncthreads();
            lane_sum[lane] = lane_sum_of(a.gray + ((size_t)b * kSrc + s) * a.tiles, a.tiles, lane);
            __syncthreads();
            double t = 0.0;
            for (int i = 0; i < kWave; ++i) t = t + lane_sum[i];
            beta = beta_of(bd, t / npix);
        }
        if (lane == 0) a.beta[b * kSrc + s] = beta;
    }

    // every object's float box, integer box and candidate flag, in parallel
    const int n_dest = fr.n_obj[0];
    int n_all = n_dest;
    for (int s = 0; s < fr.n_src; ++s) n_all += fr.n_obj[1 + s];
    const size_t ob = (size_t)b * a.max_obj;
    for (int j = lane; j < n_all; j += kWave) {
        int s = -1, first = n_dest;                             // source of object j; -1: the destination's own
        if (j >= n_dest)
            for (s = 0; s < fr.n_src - 1 && j >= first + fr.n_obj[1 + s]; ++s) first += fr.n_obj[1 + s];
        const double *o = a.objects + (size_t)(fr.obj0 + j) * kObjCols;
        double box[4];
        int ib[4] = {0, 0, 0, 0}, clamped = 0;
        bool ok = float_box(o, s < 0 ? nullptr : fr.delta[s], fr.tr, fr.p2, box, &clamped);
        if (s >= 0) {
            const int c = a.classes[fr.obj0 + j];
            ok = ok && c >= 0 && c < kFocus && int_box(box, a.W, a.H, ib);
        }
        for (int k = 0; k < 4; ++k) {
            a.boxes[(ob + j) * 4 + k] = box[k];
            a.ibox[(ob + j) * 4 + k] = ib[k];
        }
        a.flags[ob + j] = (ok ? 4 : 0) | clamped;
    }
    __syncthreads();

    // the destination's own objects open the accepted list, in order
    double *acc = a.acc + (size_t)b * (a.max_obj + 1) * 4;
    int n_acc = 0, rows = 0;
    for (int base = 0; base < n_dest; base += kWave) {
        const int j = base + lane;
        const bool keep = j < n_dest && (a.flags[ob + j] & 4);
        const unsigned long long m = __ballot(keep);
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (keep)
            for (int k = 0; k < 4; ++k) acc[(size_t)(n_acc + rank) * 4 + k] = a.boxes[(ob + j) * 4 + k];
        if (j < n_dest) {
            a.row_of[ob + j] = keep ? rows + rank : -1;
            a.kept[ob + j] = keep ? 1 : 0;
        }
        n_acc += __popcll(m);
        rows = n_acc;
    }
    if (n_acc == 0) {                                           // init_bboxes = [[0, 0, 0, 0]]
        if (lane < 4) acc[lane] = 0.0;
        n_acc = 1;
    }
    __syncthreads();

    // the walk: serial over the sources' objects, each object's maximum IoU wave-parallel over the accepted list
    int32_t *cbox = a.cbox + ob * 4;
    int n_c = 0, j = n_dest;
    for (int s = 0; s < kSrc; ++s) {
        if (lane == 0) a.cstart[b * (kSrc + 1) + s] = n_c;
        const int n_s = s < fr.n_src ? fr.n_obj[1 + s] : 0;
        for (int i = 0; i < n_s; ++i, ++j) {
            bool accept = false;
            if (a.flags[ob + j] & 4) {                          // wave-uniform
                double nb[4];
                for (int k = 0; k < 4; ++k) nb[k] = (double)a.ibox[(ob + j) * 4 + k];
                double best = -1.0;
                int nan = 0;
                for (int t = lane; t < n_acc; t += kWave) {
                    const double v = box_iou(acc + (size_t)t * 4, nb);
                    nan |= v != v;
                    best = v > best ? v : best;
                }
#pragma unroll
                for (int off = kWave / 2; off > 0; off >>= 1) {
                    const double other = __shfl_xor(best, off, kWave);
                    best = other > best ? other : best;
                    nan |= __shfl_xor(nan, off, kWave);
                }
                accept = !nan && best < 0.15;                   // np.max(ious) < 0.15: a NaN rejects
                if (accept) {
                    if (lane < 4) {
                        acc[(size_t)n_acc * 4 + lane] = nb[lane];
                        cbox[n_c * 4 + lane] = a.ibox[(ob + j) * 4 + lane];
                    }
                    ++n_acc;
                    ++n_c;
                }
                __syncthreads();                                // the appended box is visible to the next object's lanes
            }
            if (lane == 0) {
                a.kept[ob + j] = accept ? 1 : 0;
                a.row_of[ob + j] = accept ? rows : -1;
            }
            rows += accept ? 1 : 0;
        }
    }
    if (lane == 0) {
        a.cstart[b * (kSrc + 1) + kSrc] = n_c;
        a.n_rows[b] = rows;
    }
}

// ------------------------------------------------------------------------------------------------------------- launch 3
// The composite of one destination pixel: the sources in order, each overwriting where its kept mask is non-zero.
HD void composite_pixel(const sgv3d_recombine_frame &fr, const uint8_t *images, const uint8_t *masks, int H, int W, const int32_t *cbox,
                        const int32_t *cstart, const double *beta, unsigned hit, int x, int y, uint8_t *rgb, uint8_t *id) {
    const size_t px = (size_t)H * W;
    for (int s = 0; s < fr.n_src; ++s) {
        if (!(hit >> s & 1)) continue;
        bool in_box = false;
        for (int t = cstart[s]; t < cstart[s + 1] && !in_box; ++t) {
            const int32_t *q = cbox + (size_t)t * 4;
            in_box = x >= q[0] && x <= q[2] && y >= q[1] && y <= q[3];
        }
        if (!in_box) continue;
        double qx, qy;
        if (warp_position(fr.minv[s], x, y, W, H, &qx, &qy)) continue;
        const int mx = (int)floor(qx + 0.5), my = (int)floor(qy + 0.5);      // <= W-1, H-1: q is clipped to W-2, H-2
        unsigned m = masks[(size_t)fr.src[s] * px + (size_t)my * W + mx];
        m = m > 6u ? 6u : m;
        if (m == 0) continue;
        const uint8_t *img = images + (size_t)fr.src[s] * px * 3;
        const float sh = (float)beta[s];
        for (int c = 0; c < 3; ++c) rgb[c] = shift_u8(bilinear(img, W, c, qx, qy), sh);
        *id = (uint8_t)m;
    }
}

__global__ __launch_bounds__(kBX *kBY) void composite_kernel(Args a) {
    const int b = blockIdx.z;
    const sgv3d_recombine_frame &fr = a.fr[b];
    const int tx0 = blockIdx.x * kBX * kPX, ty0 = blockIdx.y * kBY;
    const int tx1 = min(tx0 + kBX * kPX, a.W) - 1, ty1 = min(ty0 + kBY, a.H) - 1;
    const int32_t *cbox = a.cbox + (size_t)b * a.max_obj * 4, *cstart = a.cstart + b * (kSrc + 1);
    const int tid = threadIdx.y * kBX + threadIdx.x;
    unsigned hit = 0;                                           // bit s: an accepted box of source s touches this tile
    for (int s = 0; s < fr.n_src; ++s) {
        int any = 0;
        for (int t = cstart[s] + tid; t < cstart[s + 1]; t += kBX * kBY) {
            const int32_t *q = cbox + (size_t)t * 4;
            any |= q[0] <= tx1 && q[2] >= tx0 && q[1] <= ty1 && q[3] >= ty0;
        }
        if (__syncthreads_or(any)) hit |= 1u << s;
    }
    const int x0 = tx0 + threadIdx.x * kPX, y = ty0 + threadIdx.y;
    if (x0 >= a.W || y >= a.H) return;
    const size_t px = (size_t)a.H * a.W;
    const size_t o = (size_t)y * a.W + x0;
    const uint8_t *dimg = a.images + ((size_t)fr.dest * px + o) * 3, *dmask = a.masks + (size_t)fr.dest * px + o;
    uint8_t *oimg = a.out_images + ((size_t)b * px + o) * 3, *omask = a.out_masks + (size_t)b * px + o;
    const int nq = min(kPX, a.W - x0);
    uint8_t rgb[kPX * 3], id[kPX];
    for (int q = 0; q < kPX; ++q) {
        id[q] = 0;
        for (int c = 0; c < 3; ++c) rgb[q * 3 + c] = 0;
        if (q >= nq) continue;
        for (int c = 0; c < 3; ++c) rgb[q * 3 + c] = dimg[q * 3 + c];
        id[q] = dmask[q] > 6 ? 6 : dmask[q];
        if (hit) composite_pixel(fr, a.images, a.masks, a.H, a.W, cbox, cstart, a.beta + b * kSrc, hit, x0 + q, y, rgb + q * 3, id + q);
    }
    if (nq == kPX && (reinterpret_cast<uintptr_t>(oimg) & 3) == 0 && (reinterpret_cast<uintptr_t>(omask) & 3) == 0) {
        uint32_t w[4];
        __builtin_memcpy(w, rgb, 12);
        __builtin_memcpy(w + 3, id, 4);
        uint32_t *d = reinterpret_cast<uint32_t *>(oimg);
        d[0] = w[0], d[1] = w[1], d[2] = w[2];
        *reinterpret_cast<uint32_t *>(omask) = w[3];
    } else {
        for (int q = 0; q < nq; ++q) {
            for (int c = 0; c < 3; ++c) oimg[q * 3 + c] = rgb[q * 3 + c];
            omask[q] = id[q];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- launch 4
HD void label_of(const sgv3d_recombine_frame &fr, const double *objects, const double *boxes, const int32_t *flags, int j, double *row,
                 int32_t *info) {
    int s = -1, first = fr.n_obj[0];
    if (j >= first)
        for (s = 0; s < fr.n_src - 1 && j >= first + fr.n_obj[1 + s]; ++s) first += fr.n_obj[1 + s];
    label_row(objects + (size_t)(fr.obj0 + j) * kObjCols, s < 0 ? nullptr : fr.delta[s], fr.tr, boxes + (size_t)j * 4, row);
    info[0] = j;
    info[1] = flags[j] & 3;
}

__global__ __launch_bounds__(256) void labels_kernel(Args a) {
    const int b = blockIdx.x;
    const sgv3d_recombine_frame &fr = a.fr[b];
    int n_all = fr.n_obj[0];
    for (int s = 0; s < fr.n_src; ++s) n_all += fr.n_obj[1 + s];
    const size_t ob = (size_t)b * a.max_obj;
    for (int j = threadIdx.x; j < n_all; j += blockDim.x) {
        const int r = a.row_of[ob + j];
        if (r < 0) continue;                                    // r < rows <= n_all <= max_obj
        label_of(fr, a.objects, a.boxes + ob * 4, a.flags + ob, j, a.rows + (ob + r) * kRowCols, a.row_info + (ob + r) * 2);
    }
}

// ----------------------------------------------------------------------------------------------------------- validation
int validate(const char *who, int batch, int pool, int h, int w, int max_obj, int total_obj, const sgv3d_recombine_frame *fh,
             const void *images, const void *masks, const void *objects, const void *classes, const void *out_images,
             const void *out_masks, const void *beta, const void *boxes, const void *kept, const void *n_rows, const void *rows,
             const void *row_info) {
    SGV3D_REQUIRE(fh && images && masks && objects && classes && out_images && out_masks && beta && boxes && kept && n_rows && rows &&
                      row_info,
                  "%s: null pointer", who);
    SGV3D_REQUIRE(batch >= 1 && batch <= 8192 && pool >= 1 && max_obj >= 1 && total_obj >= 0, "%s: non-positive or unsupported size "
                  "(batch %d, pool %d, max_obj %d, total_obj %d)", who, batch, pool, max_obj, total_obj);
    SGV3D_REQUIRE(h >= 2 && w >= 2 && h <= 16384 && w <= 16384, "%s: frame of %d x %d: both sides must be in [2, 16384]", who, h, w);
    SGV3D_REQUIRE((long long)batch * max_obj <= 0x3fffffffLL && (long long)total_obj <= 0x3fffffffLL / kObjCols, "%s: too many objects", who);
    for (int b = 0; b < batch; ++b) {
        const sgv3d_recombine_frame &f = fh[b];
        SGV3D_REQUIRE(f.n_src >= 0 && f.n_src <= kSrc, "%s: frame %d: %d sources, at most %d", who, b, f.n_src, kSrc);
        SGV3D_REQUIRE(f.dest >= 0 && f.dest < pool, "%s: frame %d: destination %d outside the pool of %d", who, b, f.dest, pool);
        long long n = f.n_obj[0];
        SGV3D_REQUIRE(f.n_obj[0] >= 0, "%s: frame %d: negative object count", who, b);
        for (int s = 0; s < kSrc; ++s) {
            if (s >= f.n_src) {
                SGV3D_REQUIRE(f.n_obj[1 + s] == 0, "%s: frame %d: objects of source %d, which is not there", who, b, s);
                continue;
            }
            SGV3D_REQUIRE(f.src[s] >= 0 && f.src[s] < pool, "%s: frame %d: source %d outside the pool of %d", who, b, f.src[s], pool);
            SGV3D_REQUIRE(f.n_obj[1 + s] >= 0, "%s: frame %d: negative object count", who, b);
            n += f.n_obj[1 + s];
            for (int k = 0; k < 9; ++k) SGV3D_REQUIRE(isfinite(f.minv[s][k]), "%s: frame %d: non-finite homography", who, b);
        }
        SGV3D_REQUIRE(n <= max_obj, "%s: frame %d: %lld objects, max_obj is %d", who, b, n, max_obj);
        SGV3D_REQUIRE(f.obj0 >= 0 && f.obj0 + n <= total_obj, "%s: frame %d: objects [%d, %lld) outside the %d given", who, b, f.obj0,
                      f.obj0 + n, total_obj);
    }
    return SGV3D_OK;
}

}  // namespace

extern "C" size_t sgv3d_recombine_workspace_bytes(int batch, int h, int w, int max_obj) {
    if (batch < 1 || batch > 8192 || h < 2 || w < 2 || h > 16384 || w > 16384 || max_obj < 1 || (long long)batch * max_obj > 0x3fffffffLL)
        return 0;
    return layout_of(batch, h, w, max_obj).total;
}

extern "C" int sgv3d_recombine_frames(int batch, int pool, int h, int w, int max_obj, int total_obj, const sgv3d_recombine_frame *frames_host,
                                      const sgv3d_recombine_frame *frames_dev, const uint8_t *images, const uint8_t *masks,
                                      const double *objects, const int32_t *classes, void *work, size_t work_bytes, uint8_t *out_images,
                                      uint8_t *out_masks, double *beta, double *boxes, int32_t *kept, int32_t *n_rows, double *rows,
                                      int32_t *row_info, void *stream) {
    const int rc = validate("recombine_frames", batch, pool, h, w, max_obj, total_obj, frames_host, images, masks, objects, classes,
                            out_images, out_masks, beta, boxes, kept, n_rows, rows, row_info);
    if (rc != SGV3D_OK) return rc;
    SGV3D_REQUIRE(frames_dev && work, "recombine_frames: null pointer");
    SGV3D_REQUIRE(((uintptr_t)work & 7) == 0 && ((uintptr_t)frames_dev & 7) == 0 && ((uintptr_t)objects & 7) == 0 &&
                      ((uintptr_t)beta & 7) == 0 && ((uintptr_t)boxes & 7) == 0 && ((uintptr_t)rows & 7) == 0,
                  "recombine_frames: misaligned buffer");
    const Layout L = layout_of(batch, h, w, max_obj);
    if (work_bytes < L.total)
        return sgv3d::fail(SGV3D_ENOSPACE, "recombine_frames: workspace of %zu bytes, %zu needed", work_bytes, L.total);
    uint8_t *wk = static_cast<uint8_t *>(work);
    Args a{};
    a.fr = frames_dev;
    a.images = images, a.masks = masks, a.objects = objects, a.classes = classes;
    a.gray = reinterpret_cast<double *>(wk + L.gray);
    a.dgray = reinterpret_cast<unsigned long long *>(wk + L.dgray);
    a.acc = reinterpret_cast<double *>(wk + L.acc);
    a.ibox = reinterpret_cast<int32_t *>(wk + L.ibox);
    a.cbox = reinterpret_cast<int32_t *>(wk + L.cbox);
    a.cstart = reinterpret_cast<int32_t *>(wk + L.cstart);
    a.row_of = reinterpret_cast<int32_t *>(wk + L.row_of);
    a.flags = reinterpret_cast<int32_t *>(wk + L.flags);
    a.out_images = out_images, a.out_masks = out_masks;
    a.beta = beta, a.boxes = boxes, a.rows = rows, a.kept = kept, a.n_rows = n_rows, a.row_info = row_info;
    a.H = h, a.W = w, a.max_obj = max_obj, a.tiles = L.tiles;
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(gray_partials_kernel, dim3(cdiv(w, kBX), cdiv(h, kBY), batch * (kSrc + 1)), dim3(kBX, kBY), 0, st, a, batch);
    hipLaunchKernelGGL(gate_kernel, dim3(batch), dim3(kWave), 0, st, a);
    hipLaunchKernelGGL(composite_kernel, dim3(cdiv(w, kBX * kPX), cdiv(h, kBY), batch), dim3(kBX, kBY), 0, st, a);
    hipLaunchKernelGGL(labels_kernel, dim3(batch), dim3(256), 0, st, a);
    return check_launch("recombine_frames");
}

// The same arithmetic over host pointers; the sums follow the kernels' order (tile -> row tree of 64 -> four rows ->
// 64 strided lane sums in lane order), so beta agrees bit for bit.  warped: optional float32 [batch, 3, h, w, 3], every source warped
// in full (dead pixels 0), what launch 1 takes the gray of.
extern "C" int sgv3d_recombine_host(int batch, int pool, int h, int w, int max_obj, int total_obj, const sgv3d_recombine_frame *frames,
                                    const uint8_t *images, const uint8_t *masks, const double *objects, const int32_t *classes,
                                    uint8_t *out_images, uint8_t *out_masks, double *beta, double *boxes, int32_t *kept, int32_t *n_rows,
                                    double *rows, int32_t *row_info, float *warped) {
    const int rc = validate("recombine_host", batch, pool, h, w, max_obj, total_obj, frames, images, masks, objects, classes, out_images,
                            out_masks, beta, boxes, kept, n_rows, rows, row_info);
    if (rc != SGV3D_OK) return rc;
    const Layout L = layout_of(batch, h, w, max_obj);
    const int tiles_x = cdiv(w, kBX), tiles_y = cdiv(h, kBY);
    const size_t px = (size_t)h * w;
    std::vector<double> part(L.tiles), acc((size_t)(max_obj + 1) * 4);
    std::vector<unsigned long long> ipart(L.tiles);
    std::vector<int32_t> cbox((size_t)max_obj * 4), row_of(max_obj), flags(max_obj);
    for (int b = 0; b < batch; ++b) {
        const sgv3d_recombine_frame &fr = frames[b];
        const double npix = (double)h * (double)w;
        // launch 1 + the reduce of launch 2
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                unsigned long long t = 0;
                for (int y = ty * kBY; y < ty * kBY + kBY && y < h; ++y)
                    for (int x = tx * kBX; x < tx * kBX + kBX && x < w; ++x) {
                        const uint8_t *p = images + ((size_t)fr.dest * px + (size_t)y * w + x) * 3;
                        t += gray_u8(p[0], p[1], p[2]);
                    }
                ipart[ty * tiles_x + tx] = t;
            }
        unsigned long long dsum = 0;
        for (int lane = 0; lane < kWave; ++lane) dsum += lane_sum_of(ipart.data(), L.tiles, lane);
        const double bd = (double)dsum / npix;
        for (int s = 0; s < kSrc; ++s) {
            beta[b * kSrc + s] = 0.0;
            if (s >= fr.n_src) {
                if (warped) std::fill(warped + ((size_t)b * kSrc + s) * px * 3, warped + ((size_t)b * kSrc + s + 1) * px * 3, 0.0f);
                continue;
            }
            const uint8_t *img = images + (size_t)fr.src[s] * px * 3;
            for (int ty = 0; ty < tiles_y; ++ty)
                for (int tx = 0; tx < tiles_x; ++tx) {
                    double t = 0.0;
                    for (int r = 0; r < kBY; ++r) {
                        double lane_v[kWave];
                        const int y = ty * kBY + r;
                        for (int i = 0; i < kWave; ++i) {
                            const int x = tx * kBX + i;
                            double g = 0.0;
                            if (x < w && y < h) {
                                double qx, qy;
                                float v[3] = {0.0f, 0.0f, 0.0f};
                                if (!warp_position(fr.minv[s], x, y, w, h, &qx, &qy)) {
                                    for (int c = 0; c < 3; ++c) v[c] = bilinear(img, w, c, qx, qy);
                                    g = (double)gray_f32(v[0], v[1], v[2]);
                                }
                                if (warped)
                                    for (int c = 0; c < 3; ++c) warped[(((size_t)b * kSrc + s) * px + (size_t)y * w + x) * 3 + c] = v[c];
                            }
                            lane_v[i] = g;
                        }
                        for (int off = kWave / 2; off > 0; off >>= 1)
                            for (int i = 0; i < off; ++i) lane_v[i] = lane_v[i] + lane_v[i + off];
                        t = t + lane_v[0];
                    }
                    part[ty * tiles_x + tx] = t;
                }
            double t = 0.0;
            for (int lane = 0; lane < kWave; ++lane) t = t + lane_sum_of(part.data(), L.tiles, lane);
            beta[b * kSrc + s] = beta_of(bd, t / npix);
        }
        // launch 2: boxes and gate
        const size_t ob = (size_t)b * max_obj;
        int j = 0, n_acc = 0, n_rows_b = 0, n_c = 0, cstart[kSrc + 1];
        for (int s = -1; s < fr.n_src; ++s) {
            if (s >= 0) cstart[s] = n_c;
            if (s == 0 && n_acc == 0) {
                for (int k = 0; k < 4; ++k) acc[k] = 0.0;
                n_acc = 1;
            }
            for (int i = 0; i < fr.n_obj[1 + s]; ++i, ++j) {
                const double *o = objects + (size_t)(fr.obj0 + j) * kObjCols;
                double box[4];
                int ib[4] = {0, 0, 0, 0}, clamped = 0;
                bool ok = float_box(o, s < 0 ? nullptr : fr.delta[s], fr.tr, fr.p2, box, &clamped);
                if (s >= 0) {
                    const int c = classes[fr.obj0 + j];
                    ok = ok && c >= 0 && c < kFocus && int_box(box, w, h, ib);
                }
                for (int k = 0; k < 4; ++k) boxes[(ob + j) * 4 + k] = box[k];
                flags[j] = (ok ? 4 : 0) | clamped;
                bool accept = ok;
                if (ok && s >= 0) {
                    double nb[4], best = -1.0;
                    bool nan = false;
                    for (int k = 0; k < 4; ++k) nb[k] = (double)ib[k];
                    for (int t = 0; t < n_acc; ++t) {
                        const double v = box_iou(&acc[(size_t)t * 4], nb);
                        nan = nan || v != v;
                        best = v > best ? v : best;
                    }
                    accept = !nan && best < 0.15;
                    if (accept)
                        for (int k = 0; k < 4; ++k) {
                            acc[(size_t)n_acc * 4 + k] = nb[k];
                            cbox[(size_t)n_c * 4 + k] = ib[k];
                        }
                    n_c += accept ? 1 : 0;
                } else if (ok) {
                    for (int k = 0; k < 4; ++k) acc[(size_t)n_acc * 4 + k] = box[k];
                }
                n_acc += accept ? 1 : 0;
                kept[ob + j] = accept ? 1 : 0;
                row_of[j] = accept ? n_rows_b++ : -1;
            }
        }
        for (int s = fr.n_src < 0 ? 0 : fr.n_src; s <= kSrc; ++s) cstart[s] = n_c;
        n_rows[b] = n_rows_b;
        // launch 3
        unsigned all = 0;
        for (int s = 0; s < fr.n_src; ++s) all |= 1u << s;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t o = (size_t)y * w + x;
                uint8_t rgb[3], id = masks[(size_t)fr.dest * px + o];
                id = id > 6 ? 6 : id;
                for (int c = 0; c < 3; ++c) rgb[c] = images[((size_t)fr.dest * px + o) * 3 + c];
                composite_pixel(fr, images, masks, h, w, cbox.data(), cstart, beta + b * kSrc, all, x, y, rgb, &id);
                for (int c = 0; c < 3; ++c) out_images[((size_t)b * px + o) * 3 + c] = rgb[c];
                out_masks[(size_t)b * px + o] = id;
            }
        // launch 4
        for (int k = 0; k < j; ++k)
            if (row_of[k] >= 0)
                label_of(fr, objects, boxes + ob * 4, flags.data(), k, rows + (ob + row_of[k]) * kRowCols, row_info + (ob + row_of[k]) * 2);
    }
    return SGV3D_OK;
}
