// Detections drawn where they are: 3-D box wireframes on the camera frame (visual_utils.draw_box_3d), the boxes' footprints on a
// BEV canvas (result2kitti.pcd_vis) and the class mask laid over the frame, from decode_device's packed buffer to the u8 frames
// JpegEncoder reads.  The contract is DESIGN.md "Rendering detections"; OpenCV's own pixels are not reproduced, the line rule
// below is this project's and is stated in integers.
//
// Three launches per call, whatever the batch:
//   render_setup_kernel  one workgroup per sample: the keep rule and compaction of detections_to_kitti_kernel, then per kept box
//                        (and per label box) one thread runs box_prims: corners, near-plane cut, projection, Liang-Barsky clip
//                        and truncation in float64.  Primitive p of a sample is edge p % E of box p / E (E = 14 on the camera
//                        frame, 4 on the canvas), predictions first, then labels; a dropped segment keeps its number and has
//                        thickness 0.
//   render_bin_kernel    one thread per (32-bit word of primitive numbers, 32 x 32 tile): bit i of word w is set when primitive
//                        32 w + i's bounding box, grown by ceil(t / 2), touches the tile.  Layout [word][tile]; no atomics.
//   render_paint_kernel  one workgroup per tile of either target, a thread owns four pixels of a row.  The tile's words go
//                        through LDS once; each wave walks the set bits from the highest down (wave-uniform) and lanes with
//                        unpainted pixels run the integer coverage test, until every lane is painted or the bits run out.
//
// box_prims, clip_segment and covers are __host__ __device__ and shared with sgv3d_render_detections_host.  This file is
// compiled with -ffp-contract=off: every float64 expression rounds once per operation on host and device alike.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "kitti_geom.hpp"

namespace {

using sgv3d::as_stream;
using sgv3d::check_launch;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / sgv3d::kWave;
constexpr int kCalib = 33;
constexpr int kTile = 32;
constexpr int kCamEdges = SGV3D_RENDER_CAM_EDGES, kBevEdges = SGV3D_RENDER_BEV_EDGES;
constexpr int kPrimInts = 5;                                    // x0, y0, x1, y1, colour | thickness << 24
constexpr int kMaxWords = 2 * SGV3D_RENDER_MAX_BOXES * kCamEdges / 32;
constexpr double kGuard = SGV3D_RENDER_GUARD;

// Where everything lies in the workspace, in int32 units from a sample's base.
struct Layout {
    int cam_tx, cam_ty, bev_tx, bev_ty, cam_words, bev_words;
    long long list, cam_prims, bev_prims, meta, cam_bits, bev_bits, per_sample;
};

__host__ __device__ inline Layout make_layout(const sgv3d_render_desc &D) {
    Layout L;
    L.cam_tx = (D.width + kTile - 1) / kTile;
    L.cam_ty = (D.height + kTile - 1) / kTile;
    L.bev_tx = (D.bev_w + kTile - 1) / kTile;
    L.bev_ty = (D.bev_h + kTile - 1) / kTile;
    L.cam_words = (2 * D.max_boxes * kCamEdges + 31) / 32;
    L.bev_words = D.bev_h ? (2 * D.max_boxes * kBevEdges + 31) / 32 : 0;
    long long o = 0;
    L.list = o, o += D.n;
    L.cam_prims = o, o += (long long)2 * D.max_boxes * kCamEdges * kPrimInts;
    L.bev_prims = o, o += D.bev_h ? (long long)2 * D.max_boxes * kBevEdges * kPrimInts : 0;
    L.meta = o, o += 4;                                         // primitives on the camera frame, on the canvas
    L.cam_bits = o, o += (long long)L.cam_words * L.cam_tx * L.cam_ty;
    L.bev_bits = o, o += (long long)L.bev_words * L.bev_tx * L.bev_ty;
    L.per_sample = o;
    return L;
}

// ------------------------------------------------------------------------------------------------ geometry (float64)
__host__ __device__ inline bool is_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

__host__ __device__ inline void put_prim(int32_t *q, int x0, int y0, int x1, int y1, uint32_t ct) {
    q[0] = x0, q[1] = y0, q[2] = x1, q[3] = y1, q[4] = (int32_t)ct;
}

// Liang-Barsky against [-64, w + 64] x [-64, h + 64], then truncation toward zero.  The four borders are taken in the order
// left, right, top, bottom (a d that is not finite drops the segment); r = q / p; an entering border (p < 0) raises t0, a leaving one lowers t1; the new endpoints are
// a + t * d with the ORIGINAL a and d, and an endpoint whose t was not moved is kept as it is.
__host__ __device__ inline bool clip_segment(double ax, double ay, double bx, double by, double w, double h, int32_t *q, uint32_t ct) {
    if (!(is_finite(ax) && is_finite(ay) && is_finite(bx) && is_finite(by))) return false;
    const double dx = bx - ax, dy = by - ay;
    if (!(is_finite(dx) && is_finite(dy))) return false;         // the difference of two huge coordinates can overflow
    const double p[4] = {-dx, dx, -dy, dy};
    const double qq[4] = {ax - (-kGuard), (w + kGuard) - ax, ay - (-kGuard), (h + kGuard) - ay};
    double t0 = 0.0, t1 = 1.0;
    for (int k = 0; k < 4; ++k) {
        if (p[k] == 0.0) {
            if (qq[k] < 0.0) return false;
            continue;
        }
        const double r = qq[k] / p[k];
        if (p[k] < 0.0) {
            if (r > t1) return false;
            if (r > t0) t0 = r;
        } else {
            if (r < t0) return false;
            if (r < t1) t1 = r;
        }
    }
    const double x0 = t0 > 0.0 ? ax + t0 * dx : ax, y0 = t0 > 0.0 ? ay + t0 * dy : ay;
    const double x1 = t1 < 1.0 ? ax + t1 * dx : bx, y1 = t1 < 1.0 ? ay + t1 * dy : by;
    put_prim(q, (int)x0, (int)y0, (int)x1, (int)y1, ct);
    return true;
}

// u, v of a point of the camera frame through K, as kitti_row projects the corners
__host__ __device__ inline void project(const double *K, const double *h, double *u, double *v) {
    const double d = dot3(K + 6, h[0], h[1], h[2]);
    *u = dot3(K, h[0], h[1], h[2]) / d;
    *v = dot3(K + 3, h[0], h[1], h[2]) / d;
}

// The primitives of one box from its eight corners in the lidar frame: 14 on the camera frame (cam), 4 on the canvas (bev, may
// be null).  A dropped segment is written as zeros (thickness 0).
__host__ __device__ inline void box_prims(const double (*P)[3], const double *cal, const sgv3d_render_desc &D, uint32_t cam_rgb,
                                          uint32_t bev_rgb, int32_t *cam, int32_t *bev) {
    constexpr unsigned char ea[kCamEdges] = {0, 1, 5, 4, 1, 2, 6, 2, 3, 7, 3, 4, 0, 1};
    constexpr unsigned char eb[kCamEdges] = {1, 5, 4, 0, 2, 6, 5, 3, 7, 6, 0, 7, 5, 4};
    const double *Tr = cal, *K = cal + 12;
    double H[8][3];
    for (int k = 0; k < 8; ++k) {
        H[k][0] = dot3(Tr, P[k][0], P[k][1], P[k][2]) + Tr[3];
        H[k][1] = dot3(Tr + 4, P[k][0], P[k][1], P[k][2]) + Tr[7];
        H[k][2] = dot3(Tr + 8, P[k][0], P[k][1], P[k][2]) + Tr[11];
    }
    const double zn = D.z_near;
    for (int e = 0; e < kCamEdges; ++e) {
        int32_t *q = cam + e * kPrimInts;
        put_prim(q, 0, 0, 0, 0, 0);
        double a[3] = {H[ea[e]][0], H[ea[e]][1], H[ea[e]][2]}, b[3] = {H[eb[e]][0], H[eb[e]][1], H[eb[e]][2]};
        const bool a_behind = a[2] < zn, b_behind = b[2] < zn;
        if (a_behind && b_behind) continue;
        if (a_behind) {                                         // the endpoint behind the plane moves onto it
            const double s = (zn - a[2]) / (b[2] - a[2]);
            for (int i = 0; i < 3; ++i) a[i] = a[i] + s * (b[i] - a[i]);
        } else if (b_behind) {
            const double s = (zn - b[2]) / (a[2] - b[2]);
            for (int i = 0; i < 3; ++i) b[i] = b[i] + s * (a[i] - b[i]);
        }
        double ua, va, ub, vb;
        project(K, a, &ua, &va);
        project(K, b, &ub, &vb);
        const uint32_t t = e < 12 ? (uint32_t)D.thickness : 1u;
        clip_segment(ua, va, ub, vb, (double)D.width, (double)D.height, q, cam_rgb | (t << 24));
    }
    if (!bev) return;
    constexpr unsigned char fa[kBevEdges] = {0, 0, 1, 2}, fb[kBevEdges] = {1, 3, 2, 3};
    double X[4], Y[4];
    bool ok[4];
    for (int k = 0; k < 4; ++k) {                               // pcl2xy_plane: int32 truncation, then the integer offsets
        const double vx = -P[k][1] / D.bev_res, vy = -P[k][0] / D.bev_res;
        ok[k] = fabs(vx) < 2147483648.0 && fabs(vy) < 2147483648.0;
        X[k] = ok[k] ? (double)((long long)(int)vx - D.bev_x_off) : 0.0;
        Y[k] = ok[k] ? (double)((long long)(int)vy + D.bev_y_off) : 0.0;
    }
    for (int e = 0; e < kBevEdges; ++e) {
        int32_t *q = bev + e * kPrimInts;
        put_prim(q, 0, 0, 0, 0, 0);
        if (!(ok[fa[e]] && ok[fb[e]])) continue;
        clip_segment(X[fa[e]], Y[fa[e]], X[fb[e]], Y[fb[e]], (double)D.bev_w, (double)D.bev_h, q, bev_rgb | (2u << 24));
    }
}

__host__ __device__ inline uint32_t rgb_of(const uint8_t *c) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

// Detection row -> corners: the eight corners kitti_row projects for the 2-D box.
template <typename T>
__host__ __device__ inline void pred_prims(const T *box, int label, const double *cal, const sgv3d_render_desc &D, int32_t *cam,
                                           int32_t *bev) {
    const double *Rm = cal + 21, *tr = cal + 30;
    const double bx = box[0], by = box[1], bz = box[2];
    const double x = dot3(Rm, bx, by, bz) + tr[0];
    const double y = dot3(Rm + 3, bx, by, bz) + tr[1];
    const double z = dot3(Rm + 6, bx, by, bz) + tr[2];
    const double w = box[4], l = box[3], h = box[5], yaw = box[6];
    const double c = cos(yaw), s = sin(yaw);
    const double zb = (z + h / 2) - h / 2;
    double P[8][3];
    for (int k = 0; k < 8; ++k) box_corner(k, w, l, h, c, s, x, y, zb, P[k]);
    box_prims(P, cal, D, rgb_of(D.class_colors + 3 * label), rgb_of(D.bev_pred_color), cam, bev);
}

__host__ __device__ inline void label_prims(const double *row, const double *cal, const sgv3d_render_desc &D, int32_t *cam,
                                            int32_t *bev) {
    const double c = cos(row[6]), s = sin(row[6]);
    double P[8][3];
    for (int k = 0; k < 8; ++k) box_corner(k, row[3], row[4], row[5], c, s, row[0], row[1], row[2], P[k]);
    box_prims(P, cal, D, rgb_of(D.label_color), rgb_of(D.bev_label_color), cam, bev);
}

// ------------------------------------------------------------------------------------------------ coverage (int64)
// Pixel (px, py) against the segment a -> b at thickness t.  Sides are at most 8192 + 2 * 64, so 4 * cr^2 < 2^62.
__host__ __device__ inline bool covers(int px, int py, int ax, int ay, int bx, int by, int t) {
    const long long dx = bx - ax, dy = by - ay, qx = px - ax, qy = py - ay;
    const long long L2 = dx * dx + dy * dy, s = qx * dx + qy * dy, t2 = (long long)t * t;
    if (L2 == 0 || s <= 0) return 4 * (qx * qx + qy * qy) <= t2;
    if (s >= L2) {
        const long long rx = px - bx, ry = py - by;
        return 4 * (rx * rx + ry * ry) <= t2;
    }
    const long long cr = qx * dy - qy * dx;
    return 4 * cr * cr <= t2 * L2;
}

// the mask overlay of one pixel: every channel becomes (f * (256 - alpha) + palette[id] * alpha + 128) >> 8
__host__ __device__ inline uint32_t blend(uint32_t px, const uint8_t *pal, int alpha) {
    uint32_t out = 0;
    for (int c = 0; c < 3; ++c) {
        const uint32_t f = (px >> (8 * c)) & 0xff;
        out |= ((f * (uint32_t)(256 - alpha) + (uint32_t)pal[c] * (uint32_t)alpha + 128u) >> 8) << (8 * c);
    }
    return out;
}

__host__ __device__ inline bool prim_touches(const int32_t *q, int x_lo, int y_lo, int x_hi, int y_hi) {
    const int t = (int)((uint32_t)q[4] >> 24);
    if (t == 0) return false;
    const int g = (t + 1) / 2;
    const int lo_x = (q[0] < q[2] ? q[0] : q[2]) - g, hi_x = (q[0] < q[2] ? q[2] : q[0]) + g;
    const int lo_y = (q[1] < q[3] ? q[1] : q[3]) - g, hi_y = (q[1] < q[3] ? q[3] : q[1]) + g;
    return lo_x <= x_hi && hi_x >= x_lo && lo_y <= y_hi && hi_y >= y_lo;
}

// ------------------------------------------------------------------------------------------------ kernels
struct RenderArgs {
    sgv3d_render_desc D;
    Layout L;
    const int32_t *labels, *counts, *label_counts;
    const double *calib, *label_boxes;
    const uint8_t *frames, *masks;
    uint8_t *out, *bev;
    int32_t *status, *work;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void render_setup_kernel(const T *__restrict__ boxes, const T *__restrict__ scores,
                                                                KittiParams P, RenderArgs A) {
    __shared__ int wave_cnt[kWaves];
    const sgv3d_render_desc &D = A.D;
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / sgv3d::kWave;
    const size_t row0 = (size_t)b * D.n;
    int32_t *ws = A.work + (size_t)b * A.L.per_sample;
    int32_t *list = ws + A.L.list;
    int n = A.counts[b];
    n = n < 0 ? 0 : (n > D.n ? D.n : n);                        // rows at or beyond counts[b] are never read
    int running = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int r = base + tid;
        int c = -1;
        const bool keep = r < n && kitti_keep((double)scores[row0 + r], A.labels[row0 + r], P, &c);
        const unsigned long long mask = __ballot(keep);
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if ((tid & (sgv3d::kWave - 1)) == 0) wave_cnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kWaves; ++k) {
            before += k < wave ? wave_cnt[k] : 0;
            total += wave_cnt[k];
        }
        if (keep) list[running + before + rank] = r;            // running + before + rank < n <= D.n
        running += total;
        __syncthreads();
    }
    int nlab = 0;
    if (A.label_boxes) {
        nlab = A.label_counts[b];
        nlab = nlab < 0 ? 0 : (nlab > D.m ? D.m : nlab);
    }
    const bool overflow = running > D.max_boxes || nlab > D.max_boxes;
    const int boxes_drawn = overflow ? 0 : running + nlab;     // <= 2 * max_boxes
    if (tid == 0) {
        ws[A.L.meta + 0] = boxes_drawn * kCamEdges;
        ws[A.L.meta + 1] = D.bev_h ? boxes_drawn * kBevEdges : 0;
        ws[A.L.meta + 2] = running;
        ws[A.L.meta + 3] = nlab;
        A.status[b] = overflow ? SGV3D_RENDER_EOVERFLOW : 0;
    }
    __syncthreads();                                            // the list is visible to the whole workgroup
    const double *cal = A.calib + (size_t)b * kCalib;
    for (int j = tid; j < boxes_drawn; j += kThreads) {
        int32_t *cam = ws + A.L.cam_prims + (size_t)j * kCamEdges * kPrimInts;
        int32_t *bev = D.bev_h ? ws + A.L.bev_prims + (size_t)j * kBevEdges * kPrimInts : nullptr;
        if (j < running) {
            const int r = list[j];
            pred_prims(boxes + (row0 + r) * 9, A.labels[row0 + r], cal, D, cam, bev);
        } else {
            label_prims(A.label_boxes + ((size_t)b * D.m + (j - running)) * 7, cal, D, cam, bev);
        }
    }
}

__global__ __launch_bounds__(kThreads) void render_bin_kernel(RenderArgs A) {
    const Layout &L = A.L;
    const int b = blockIdx.y;
    int32_t *ws = A.work + (size_t)b * L.per_sample;
    const long long cam_tiles = (long long)L.cam_tx * L.cam_ty, bev_tiles = (long long)L.bev_tx * L.bev_ty;
    const long long cam_items = cam_tiles * L.cam_words, items = cam_items + bev_tiles * L.bev_words;
    long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= items) return;
    const bool on_bev = idx >= cam_items;
    idx -= on_bev ? cam_items : 0;
    const long long tiles = on_bev ? bev_tiles : cam_tiles;
    const int tiles_x = on_bev ? L.bev_tx : L.cam_tx;
    const int w = (int)(idx / tiles), tile = (int)(idx % tiles);        // the tile runs fastest: a wave shares its primitives
    const int nprims = ws[L.meta + (on_bev ? 1 : 0)];
    if (w * 32 >= nprims) return;                               // words beyond the primitives are never read either
    const int32_t *prims = ws + (on_bev ? L.bev_prims : L.cam_prims);
    const int x_lo = (tile % tiles_x) * kTile, y_lo = (tile / tiles_x) * kTile;
    uint32_t word = 0;
    for (int i = 0; i < 32 && w * 32 + i < nprims; ++i)
        if (prim_touches(prims + (size_t)(w * 32 + i) * kPrimInts, x_lo, y_lo, x_lo + kTile - 1, y_lo + kTile - 1)) word |= 1u << i;
    ws[(on_bev ? L.bev_bits : L.cam_bits) + idx] = (int32_t)word;       // idx = w * tiles + tile
}

__global__ __launch_bounds__(kThreads) void render_paint_kernel(RenderArgs A) {
    __shared__ uint32_t sw[kMaxWords];
    const sgv3d_render_desc &D = A.D;
    const Layout &L = A.L;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int32_t *ws = A.work + (size_t)b * L.per_sample;
    const int cam_tiles = L.cam_tx * L.cam_ty;
    const bool on_bev = (int)blockIdx.x >= cam_tiles;
    const int tile = on_bev ? (int)blockIdx.x - cam_tiles : (int)blockIdx.x;
    const int tiles = on_bev ? L.bev_tx * L.bev_ty : cam_tiles, tiles_x = on_bev ? L.bev_tx : L.cam_tx;
    const int W = on_bev ? D.bev_w : D.width, Hh = on_bev ? D.bev_h : D.height;
    const int nprims = ws[L.meta + (on_bev ? 1 : 0)];
    const int nwords = (nprims + 31) / 32;
    const int32_t *bits = ws + (on_bev ? L.bev_bits : L.cam_bits);
    const int32_t *prims = ws + (on_bev ? L.bev_prims : L.cam_prims);

    uint32_t mine = 0;
    for (int w = tid; w < nwords; w += kThreads) {
        sw[w] = (uint32_t)bits[(size_t)w * tiles + tile];
        mine |= sw[w];
    }
    const bool has = __syncthreads_or(mine != 0);
    const bool in_place = !on_bev && A.out == A.frames;
    const bool masked = !on_bev && A.masks && A.status[b] == 0;
    if (in_place && !has && !masked) return;                    // block-uniform

    const int x = (tile % tiles_x) * kTile + (tid & 7) * 4, y = (tile / tiles_x) * kTile + (tid >> 3);
    const int nvalid = y < Hh ? (W - x < 0 ? 0 : (W - x > 4 ? 4 : W - x)) : 0;
    if (nvalid == 0) return;
    const size_t pix = ((size_t)b * Hh + y) * W + x;
    uint8_t *dst = (on_bev ? A.bev : A.out) + pix * 3;
    uint32_t px[4] = {0, 0, 0, 0};                              // R | G << 8 | B << 16
    bool changed = false;
    if (!on_bev) {
        const uint8_t *src = A.frames + pix * 3;
        if (nvalid == 4 && ((uintptr_t)src & 3) == 0) {
            const uint32_t d0 = ((const uint32_t *)src)[0], d1 = ((const uint32_t *)src)[1], d2 = ((const uint32_t *)src)[2];
            px[0] = d0 & 0xffffffu;
            px[1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
            px[2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
            px[3] = d2 >> 8;
        } else {
            for (int i = 0; i < nvalid; ++i) px[i] = rgb_of(src + 3 * i);
        }
        if (masked) {
            const uint8_t *mp = A.masks + pix;
            uint32_t mv = 0;
            if (nvalid == 4 && ((uintptr_t)mp & 3) == 0) {
                mv = *(const uint32_t *)mp;
            } else {
                for (int i = 0; i < nvalid; ++i) mv |= (uint32_t)mp[i] << (8 * i);
            }
            for (int i = 0; i < nvalid; ++i) {
                const int id = (int)((mv >> (8 * i)) & 0xff) / 40;
                if (id >= 1 && id <= 6) {
                    px[i] = blend(px[i], D.palette + 3 * id, D.mask_alpha);
                    changed = true;
                }
            }
        }
    }
    if (has) {
        uint32_t todo = (1u << nvalid) - 1;                     // pixels no primitive has painted yet
        bool walking = true;                                    // wave-uniform
        for (int w = nwords - 1; w >= 0 && walking; --w) {
            uint32_t word = __builtin_amdgcn_readfirstlane(sw[w]);
            while (word) {
                const int bit = 31 - __clz(word);
                word &= ~(1u << bit);
                const int32_t *q = prims + (size_t)(w * 32 + bit) * kPrimInts;
                const int ax = q[0], ay = q[1], bx = q[2], by = q[3];
                const uint32_t ct = (uint32_t)q[4];
                for (int i = 0; i < 4; ++i)
                    if (((todo >> i) & 1) && covers(x + i, y, ax, ay, bx, by, (int)(ct >> 24))) {
                        px[i] = ct & 0xffffffu;
                        todo &= ~(1u << i);
                        changed = true;
                    }
                if (__ballot(todo != 0) == 0) {                 // every lane of the wave is painted: the walk ends
                    walking = false;
                    break;
                }
            }
        }
    }
    if (in_place && !changed) return;
    if (nvalid == 4 && ((uintptr_t)dst & 3) == 0) {
        ((uint32_t *)dst)[0] = px[0] | (px[1] << 24);
        ((uint32_t *)dst)[1] = (px[1] >> 8) | (px[2] << 16);
        ((uint32_t *)dst)[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int i = 0; i < nvalid; ++i) {
            dst[3 * i + 0] = (uint8_t)px[i];
            dst[3 * i + 1] = (uint8_t)(px[i] >> 8);
            dst[3 * i + 2] = (uint8_t)(px[i] >> 16);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

int check_desc(const char *who, const sgv3d_render_desc *d) {
    SGV3D_REQUIRE(d, "%s: null descriptor", who);
    SGV3D_REQUIRE(d->batch >= 1 && d->batch <= 65535 && d->n >= 1 && d->m >= 0, "%s: bad size (batch %d, n %d, m %d)", who, d->batch,
                  d->n, d->m);
    SGV3D_REQUIRE((long long)d->batch * d->n <= 0x7fffffffLL && (long long)d->batch * d->m <= 0x7fffffffLL, "%s: batch too large", who);
    SGV3D_REQUIRE(d->height >= 1 && d->height <= SGV3D_RENDER_MAX_SIDE && d->width >= 1 && d->width <= SGV3D_RENDER_MAX_SIDE,
                  "%s: frame %d x %d outside [1, %d]", who, d->height, d->width, SGV3D_RENDER_MAX_SIDE);
    SGV3D_REQUIRE((d->bev_h == 0 && d->bev_w == 0) || (d->bev_h >= 1 && d->bev_h <= SGV3D_RENDER_MAX_SIDE && d->bev_w >= 1 &&
                                                        d->bev_w <= SGV3D_RENDER_MAX_SIDE),
                  "%s: canvas %d x %d is neither 0 x 0 nor inside [1, %d]", who, d->bev_h, d->bev_w, SGV3D_RENDER_MAX_SIDE);
    SGV3D_REQUIRE(d->max_boxes >= 1 && d->max_boxes <= SGV3D_RENDER_MAX_BOXES, "%s: max_boxes %d outside [1, %d]", who, d->max_boxes,
                  SGV3D_RENDER_MAX_BOXES);
    SGV3D_REQUIRE(d->thickness >= 1 && d->thickness <= 15, "%s: thickness %d outside [1, 15]", who, d->thickness);
    SGV3D_REQUIRE(d->f64_inputs == 0 || d->f64_inputs == 1, "%s: f64_inputs is 0 (float32 boxes and scores) or 1 (float64), not %d", who,
                  d->f64_inputs);
    SGV3D_REQUIRE(d->num_classes >= 1 && d->num_classes <= kMaxClasses, "%s: num_classes %d outside [1, %d]", who, d->num_classes,
                  kMaxClasses);
    SGV3D_REQUIRE(d->mask_alpha >= 0 && d->mask_alpha <= 256, "%s: mask_alpha %d outside [0, 256]", who, d->mask_alpha);
    SGV3D_REQUIRE(d->score_thr == d->score_thr, "%s: score_thr is NaN", who);
    SGV3D_REQUIRE(is_finite(d->z_near) && d->z_near > 0.0, "%s: z_near must be positive and finite", who);
    SGV3D_REQUIRE(d->bev_h == 0 || (is_finite(d->bev_res) && d->bev_res > 0.0), "%s: bev_res must be positive and finite", who);
    for (int k = 0; k < d->num_classes; ++k)
        SGV3D_REQUIRE(d->class_table[k] >= -1 && d->class_table[k] <= 2, "%s: class_table[%d] = %d is not -1, 0, 1 or 2", who, k,
                      d->class_table[k]);
    return SGV3D_OK;
}

int check_args(const char *who, const sgv3d_render_desc *d, const void *boxes, const void *scores, const void *labels,
               const void *counts, const double *calib, const double *label_boxes, const int32_t *label_counts, const uint8_t *frames,
               const uint8_t *masks, uint8_t *out, uint8_t *bev, int32_t *status, KittiParams *P) {
    const int rc = check_desc(who, d);
    if (rc != SGV3D_OK) return rc;
    SGV3D_REQUIRE(boxes && scores && labels && counts && calib && frames && out && status, "%s: null pointer", who);
    SGV3D_REQUIRE((d->m == 0) == (label_boxes == nullptr) && (label_boxes == nullptr) == (label_counts == nullptr),
                  "%s: label_boxes and label_counts go with m >= 1, null pointers with m = 0", who);
    SGV3D_REQUIRE((d->bev_h == 0) == (bev == nullptr), "%s: the bev pointer goes with a canvas size, a null pointer with 0 x 0", who);
    const uintptr_t in_mask = d->f64_inputs ? 7 : 3;
    SGV3D_REQUIRE(((uintptr_t)boxes & in_mask) == 0 && ((uintptr_t)scores & in_mask) == 0 && ((uintptr_t)calib & 7) == 0 &&
                      ((uintptr_t)label_boxes & 7) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)counts & 3) == 0 &&
                      ((uintptr_t)label_counts & 3) == 0 && ((uintptr_t)status & 3) == 0,
                  "%s: misaligned buffer", who);
    const size_t fbytes = (size_t)d->batch * d->height * d->width * 3, bbytes = (size_t)d->batch * d->bev_h * d->bev_w * 3;
    SGV3D_REQUIRE(out == frames || !overlap(out, fbytes, frames, fbytes), "%s: out partly overlaps frames", who);
    SGV3D_REQUIRE(!masks || !overlap(out, fbytes, masks, fbytes / 3), "%s: out overlaps masks", who);
    SGV3D_REQUIRE(!bev || (!overlap(bev, bbytes, frames, fbytes) && !overlap(bev, bbytes, out, fbytes) &&
                           (!masks || !overlap(bev, bbytes, masks, fbytes / 3))),
                  "%s: bev overlaps frames, masks or out", who);
    memset(P, 0, sizeof(*P));
    P->n = d->n;
    P->num_classes = d->num_classes;
    P->thr = d->score_thr;
    for (int k = 0; k < kMaxClasses; ++k) P->cls[k] = k < d->num_classes ? d->class_table[k] : -1;
    return SGV3D_OK;
}

}  // namespace

extern "C" size_t sgv3d_render_workspace_bytes(const sgv3d_render_desc *d) {
    if (check_desc("render_workspace_bytes", d) != SGV3D_OK) return 0;
    return (size_t)make_layout(*d).per_sample * d->batch * sizeof(int32_t);
}

extern "C" int sgv3d_render_detections(const sgv3d_render_desc *d, const void *boxes, const void *scores, const int32_t *labels,
                                       const int32_t *counts, const double *calib, const double *label_boxes,
                                       const int32_t *label_counts, const uint8_t *frames, const uint8_t *masks, uint8_t *out,
                                       uint8_t *bev, int32_t *status, void *workspace, size_t workspace_bytes, void *stream) {
    KittiParams P;
    const int rc = check_args("render_detections", d, boxes, scores, labels, counts, calib, label_boxes, label_counts, frames, masks, out,
                              bev, status, &P);
    if (rc != SGV3D_OK) return rc;
    SGV3D_REQUIRE(workspace, "render_detections: null pointer");
    SGV3D_REQUIRE(((uintptr_t)workspace & 3) == 0, "render_detections: misaligned buffer");
    const size_t need = sgv3d_render_workspace_bytes(d);
    if (workspace_bytes < need)
        return sgv3d::fail(SGV3D_ENOSPACE, "render_detections: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    RenderArgs A;
    A.D = *d;
    A.L = make_layout(*d);
    A.labels = labels, A.counts = counts, A.label_counts = label_counts, A.calib = calib, A.label_boxes = label_boxes;
    A.frames = frames, A.masks = masks, A.out = out, A.bev = bev, A.status = status, A.work = (int32_t *)workspace;
    hipStream_t st = as_stream(stream);
    if (d->f64_inputs)
        hipLaunchKernelGGL(render_setup_kernel<double>, dim3(d->batch), dim3(kThreads), 0, st, (const double *)boxes,
                           (const double *)scores, P, A);
    else
        hipLaunchKernelGGL(render_setup_kernel<float>, dim3(d->batch), dim3(kThreads), 0, st, (const float *)boxes,
                           (const float *)scores, P, A);
    int lrc = check_launch("render_detections (setup)");
    if (lrc != SGV3D_OK) return lrc;
    const long long cam_tiles = (long long)A.L.cam_tx * A.L.cam_ty, bev_tiles = (long long)A.L.bev_tx * A.L.bev_ty;
    const long long items = cam_tiles * A.L.cam_words + bev_tiles * A.L.bev_words;
    hipLaunchKernelGGL(render_bin_kernel, dim3(sgv3d::cdiv(items, kThreads), d->batch), dim3(kThreads), 0, st, A);
    lrc = check_launch("render_detections (bin)");
    if (lrc != SGV3D_OK) return lrc;
    hipLaunchKernelGGL(render_paint_kernel, dim3((unsigned)(cam_tiles + bev_tiles), d->batch), dim3(kThreads), 0, st, A);
    return check_launch("render_detections (paint)");
}

namespace {

// One target painted primitive by primitive in ascending order: the last writer of a pixel is its highest-numbered primitive.
void paint_host(const std::vector<int32_t> &prims, int W, int H, uint8_t *img) {
    for (size_t p = 0; p * kPrimInts < prims.size(); ++p) {
        const int32_t *q = prims.data() + p * kPrimInts;
        const uint32_t ct = (uint32_t)q[4];
        const int t = (int)(ct >> 24);
        if (t == 0) continue;
        const int g = (t + 1) / 2;
        const int x_lo = std::max(0, std::min(q[0], q[2]) - g), x_hi = std::min(W - 1, std::max(q[0], q[2]) + g);
        const int y_lo = std::max(0, std::min(q[1], q[3]) - g), y_hi = std::min(H - 1, std::max(q[1], q[3]) + g);
        for (int y = y_lo; y <= y_hi; ++y)
            for (int x = x_lo; x <= x_hi; ++x)
                if (covers(x, y, q[0], q[1], q[2], q[3], t)) {
                    uint8_t *o = img + ((size_t)y * W + x) * 3;
                    o[0] = (uint8_t)ct, o[1] = (uint8_t)(ct >> 8), o[2] = (uint8_t)(ct >> 16);
                }
    }
}

template <typename T>
void render_host(const sgv3d_render_desc &D, const KittiParams &P, const T *boxes, const T *scores, const int32_t *labels,
                 const int32_t *counts, const double *calib, const double *label_boxes, const int32_t *label_counts,
                 const uint8_t *frames, const uint8_t *masks, uint8_t *out, uint8_t *bev, int32_t *status) {
    const size_t fpix = (size_t)D.height * D.width, bpix = (size_t)D.bev_h * D.bev_w;
    for (int b = 0; b < D.batch; ++b) {
        const size_t row0 = (size_t)b * D.n;
        const int cnt = counts[b] < 0 ? 0 : (counts[b] > D.n ? D.n : counts[b]);
        std::vector<int> kept;
        for (int r = 0; r < cnt; ++r) {
            int c = -1;
            if (kitti_keep((double)scores[row0 + r], labels[row0 + r], P, &c)) kept.push_back(r);
        }
        int nlab = label_boxes ? label_counts[b] : 0;
        nlab = nlab < 0 ? 0 : (nlab > D.m ? D.m : nlab);
        const bool overflow = (int)kept.size() > D.max_boxes || nlab > D.max_boxes;
        status[b] = overflow ? SGV3D_RENDER_EOVERFLOW : 0;
        uint8_t *o = out + (size_t)b * fpix * 3;
        const uint8_t *f = frames + (size_t)b * fpix * 3;
        if (o != f) memcpy(o, f, fpix * 3);
        if (bev) memset(bev + (size_t)b * bpix * 3, 0, bpix * 3);
        if (overflow) continue;
        const int nboxes = (int)kept.size() + nlab;
        std::vector<int32_t> cam((size_t)nboxes * kCamEdges * kPrimInts), bv(bev ? (size_t)nboxes * kBevEdges * kPrimInts : 0);
        const double *cal = calib + (size_t)b * kCalib;
        for (int j = 0; j < nboxes; ++j) {
            int32_t *cq = cam.data() + (size_t)j * kCamEdges * kPrimInts;
            int32_t *bq = bev ? bv.data() + (size_t)j * kBevEdges * kPrimInts : nullptr;
            if (j < (int)kept.size())
                pred_prims(boxes + (row0 + kept[j]) * 9, labels[row0 + kept[j]], cal, D, cq, bq);
            else
                label_prims(label_boxes + ((size_t)b * D.m + (j - kept.size())) * 7, cal, D, cq, bq);
        }
        if (masks)
            for (size_t i = 0; i < fpix; ++i) {
                const int id = masks[(size_t)b * fpix + i] / 40;
                if (id < 1 || id > 6) continue;
                const uint32_t v = blend(rgb_of(o + 3 * i), D.palette + 3 * id, D.mask_alpha);
                o[3 * i] = (uint8_t)v, o[3 * i + 1] = (uint8_t)(v >> 8), o[3 * i + 2] = (uint8_t)(v >> 16);
            }
        paint_host(cam, D.width, D.height, o);
        if (bev) paint_host(bv, D.bev_w, D.bev_h, bev + (size_t)b * bpix * 3);
    }
}

}  // namespace

extern "C" int sgv3d_render_detections_host(const sgv3d_render_desc *d, const void *boxes, const void *scores, const int32_t *labels,
                                            const int32_t *counts, const double *calib, const double *label_boxes,
                                            const int32_t *label_counts, const uint8_t *frames, const uint8_t *masks, uint8_t *out,
                                            uint8_t *bev, int32_t *status) {
    KittiParams P;
    const int rc = check_args("render_detections_host", d, boxes, scores, labels, counts, calib, label_boxes, label_counts, frames, masks,
                              out, bev, status, &P);
    if (rc != SGV3D_OK) return rc;
    if (d->f64_inputs)
        render_host(*d, P, (const double *)boxes, (const double *)scores, labels, counts, calib, label_boxes, label_counts, frames, masks,
                    out, bev, status);
    else
        render_host(*d, P, (const float *)boxes, (const float *)scores, labels, counts, calib, label_boxes, label_counts, frames, masks, out,
                    bev, status);
    return SGV3D_OK;
}
