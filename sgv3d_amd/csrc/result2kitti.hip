// Detections -> KITTI annotation rows on the device: RoadSideEvaluator._format_bbox followed by result2kitti._convert
// (evaluators/det_evaluators.py, evaluators/result2kitti.py) without the JSON file, the label files and their parser.
//
// Per sample one workgroup reads rows [:counts[b]] of decode_device's buffer in place.  Pass 1 decides which rows are
// kept (score above the threshold, class in the category map) and compacts their row indices IN INPUT ORDER into the
// workspace: a wave ballot gives every kept lane its rank inside the wave (mbcnt), the four waves' counts go through
// LDS, a running offset carries over the chunks.  Pass 2 walks that dense list, so the float64 arithmetic (two boxes
// of corners, five libm calls, thirteen roundings) runs for kept detections only and on full waves.  No atomics: a
// launch is repeatable bit for bit.
//
// The arithmetic is ONE __host__ __device__ function (kitti_row) shared by the kernel and by
// sgv3d_detections_to_kitti_host.  This file is compiled with -ffp-contract=off: sums run left to right with one
// rounding per operation, as numpy's and Python's float64 expressions do; the only fused operation is the explicit
// fma of the rounding recipe, which needs the exact residual of a product.
#include <math.h>

#include "common.hpp"
#include "kitti_geom.hpp"
#include "round_decimals.hpp"

namespace {

using sgv3d::as_stream;
using sgv3d::check_launch;
using sgv3d::round4;

constexpr int kThreads = 256;                  // four waves per sample
constexpr int kWaves = kThreads / sgv3d::kWave;
constexpr int kFields = 13;
constexpr int kCalib = 33;                     // Tr_velo_to_cam 3x4 | camera matrix 3x3 | ego2global rotation 3x3 | translation 3

// One detection -> the 13 unrounded columns alpha, x1, y1, x2, y2, h, l, w, x, y, z, rotation_y, score.
template <typename T>
__host__ __device__ inline void kitti_row(const T *box, T score_f, const double *cal, double img_w, double img_h, double *out) {
    const double *Tr = cal, *K = cal + 12, *Rm = cal + 21, *tr = cal + 30;
    const double bx = box[0], by = box[1], bz = box[2];
    // _format_bbox: the centre goes through ego2global, the yaw ("box_yaw") does not; size = box[[4, 3, 5]] = (w, l, h)
    const double x = dot3(Rm, bx, by, bz) + tr[0];
    const double y = dot3(Rm + 3, bx, by, bz) + tr[1];
    const double z = dot3(Rm + 6, bx, by, bz) + tr[2];
    const double w = box[4], l = box[3], h = box[5], yaw = box[6];
    const double c = cos(yaw), s = sin(yaw);
    const double pi = 3.141592653589793;

    // alpha: the edge corner 3 -> corner 0 of the (l, w, h) box in the camera's x-z plane, minus the viewing angle
    double p0[3], p3[3];
    box_corner(0, l, w, h, c, s, x, y, z, p0);
    box_corner(3, l, w, h, c, s, x, y, z, p3);
    const double c0x = dot3(Tr, p0[0], p0[1], p0[2]) + Tr[3], c0z = dot3(Tr + 8, p0[0], p0[1], p0[2]) + Tr[11];
    const double c3x = dot3(Tr, p3[0], p3[1], p3[2]) + Tr[3], c3z = dot3(Tr + 8, p3[0], p3[1], p3[2]) + Tr[11];
    const double ccx = dot3(Tr, x, y, z) + Tr[3], ccz = dot3(Tr + 8, x, y, z) + Tr[11];
    double alpha = atan2(-(c0z - c3z), c0x - c3x) - atan2(ccx, ccz);
    if (alpha > pi) alpha -= 2.0 * pi;
    if (alpha <= -pi) alpha += 2.0 * pi;
    const double a = atan(tan(alpha));                          // normalize_angle
    out[0] = cos(alpha) < 0 ? a + pi : a;

    // 2-D box: the eight corners of the box built with (w, l, h) as extents, projected; no test for depth <= 0
    const double zb = (z + h / 2) - h / 2;
    double umin = 0, umax = 0, vmin = 0, vmax = 0;
    for (int k = 0; k < 8; ++k) {
        double p[3];
        box_corner(k, w, l, h, c, s, x, y, zb, p);
        const double h0 = dot3(Tr, p[0], p[1], p[2]) + Tr[3];
        const double h1 = dot3(Tr + 4, p[0], p[1], p[2]) + Tr[7];
        const double h2 = dot3(Tr + 8, p[0], p[1], p[2]) + Tr[11];
        const double d = dot3(K + 6, h0, h1, h2);
        const double u = dot3(K, h0, h1, h2) / d, v = dot3(K + 3, h0, h1, h2) / d;
        if (k == 0) {
            umin = umax = u;
            vmin = vmax = v;
        } else {                                                // numpy's min / max: a NaN stays
            umin = (u < umin || u != u) ? u : umin;
            umax = (u > umax || u != u) ? u : umax;
            vmin = (v < vmin || v != v) ? v : vmin;
            vmax = (v > vmax || v != v) ? v : vmax;
        }
    }
    out[1] = 0.0 > umin ? 0.0 : umin;                           // Python's max(a, 0.0) / min(a, W): a unless the bound bites
    out[2] = 0.0 > vmin ? 0.0 : vmin;
    out[3] = img_w < umax ? img_w : umax;
    out[4] = img_h < vmax ? img_h : vmax;
    out[5] = h;
    out[6] = l;
    out[7] = w;
    out[8] = (dot3(Tr, x, y, z)) + Tr[3] * 1.0;                 // location = Tr . [x, y, z, 1]
    out[9] = (dot3(Tr + 4, x, y, z)) + Tr[7] * 1.0;
    out[10] = (dot3(Tr + 8, x, y, z)) + Tr[11] * 1.0;
    out[11] = 0.5 * pi - yaw;
    out[12] = (double)score_f;
}

template <typename T>
__host__ __device__ inline void kitti_store(const T *box, T score, int cls_id, const double *cal, const KittiParams &P,
                                            double *fields, int32_t *cls) {
    double out[kFields];
    kitti_row(box, score, cal, P.img_w, P.img_h, out);
    for (int k = 0; k < kFields; ++k) fields[k] = P.digits == 4 ? round4(out[k]) : out[k];
    *cls = cls_id;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void detections_to_kitti_kernel(const T *__restrict__ boxes, const T *__restrict__ scores,
                                                                       const int32_t *__restrict__ labels,
                                                                       const int32_t *__restrict__ counts,
                                                                       const double *__restrict__ calib, KittiParams P,
                                                                       int32_t *__restrict__ list, double *__restrict__ fields,
                                                                       int32_t *__restrict__ cls, int32_t *__restrict__ kept) {
    __shared__ int wave_cnt[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / sgv3d::kWave;
    const size_t row0 = (size_t)b * P.n;
    int n = counts[b];
    n = n < 0 ? 0 : (n > P.n ? P.n : n);                        // rows at or beyond counts[b] are never read
    list += row0;
    int running = 0;                                            // kept rows before this chunk (block-uniform)
    for (int base = 0; base < n; base += kThreads) {
        const int r = base + tid;
        int c = -1;
        const bool keep = r < n && kitti_keep((double)scores[row0 + r], labels[row0 + r], P, &c);
        const unsigned long long mask = __ballot(keep);
        const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        if ((tid & (sgv3d::kWave - 1)) == 0) wave_cnt[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int k = 0; k < kWaves; ++k) {
            before += k < wave ? wave_cnt[k] : 0;
            total += wave_cnt[k];
        }
        if (keep) list[running + before + rank] = r;            // running + before + rank < n <= N
        running += total;
        __syncthreads();
    }
    if (tid == 0) kept[b] = running;                            // the true count, beyond max_det too
    __syncthreads();                                            // the list is visible to the whole workgroup
    const int m = running < P.max_det ? running : P.max_det;
    const double *cal = calib + (size_t)b * kCalib;
    for (int j = tid; j < m; j += kThreads) {
        const int r = list[j];
        int c = -1;
        const T score = scores[row0 + r];
        kitti_keep((double)score, labels[row0 + r], P, &c);
        const size_t o = (size_t)b * P.max_det + j;
        kitti_store(boxes + (row0 + r) * 9, score, c, cal, P, fields + o * kFields, cls + o);
    }
}

int fill_params(const char *who, int batch, int n, const void *boxes, const void *scores, const void *labels, const void *counts,
                const void *calib, const int8_t *class_table, int num_classes, double score_thr, int img_w, int img_h, int max_det,
                int digits, int f64_inputs, const void *fields, const void *cls, const void *kept, KittiParams *P) {
    SGV3D_REQUIRE(batch >= 1 && n >= 1 && max_det >= 1, "%s: non-positive size (batch %d, n %d, max_det %d)", who, batch, n, max_det);
    SGV3D_REQUIRE(boxes && scores && labels && counts && calib && class_table && fields && cls && kept, "%s: null pointer", who);
    SGV3D_REQUIRE(num_classes >= 1 && num_classes <= kMaxClasses, "%s: num_classes %d outside [1, %d]", who, num_classes, kMaxClasses);
    SGV3D_REQUIRE(f64_inputs == 0 || f64_inputs == 1, "%s: f64_inputs is 0 (float32 boxes and scores) or 1 (float64), not %d", who, f64_inputs);
    SGV3D_REQUIRE(digits == 4 || digits == -1, "%s: digits is 4 or -1 (unrounded), not %d", who, digits);
    SGV3D_REQUIRE(img_w >= 1 && img_h >= 1, "%s: non-positive image size %d x %d", who, img_w, img_h);
    SGV3D_REQUIRE((long long)batch * n <= 0x7fffffffLL && (long long)batch * max_det <= 0x7fffffffLL, "%s: batch too large", who);
    P->n = n;
    P->max_det = max_det;
    P->digits = digits;
    P->num_classes = num_classes;
    P->thr = score_thr;
    P->img_w = (double)img_w;
    P->img_h = (double)img_h;
    for (int k = 0; k < kMaxClasses; ++k) {
        const int v = k < num_classes ? class_table[k] : -1;
        SGV3D_REQUIRE(v >= -1 && v <= 2, "%s: class_table[%d] = %d is not -1, 0 (Car), 1 (Pedestrian) or 2 (Cyclist)", who, k, v);
        P->cls[k] = (signed char)v;
    }
    return SGV3D_OK;
}

}  // namespace

extern "C" double sgv3d_round_decimals_host(double v, int digits) {
    if (digits == -1) return v;
    if (digits != 4) {
        sgv3d::fail(SGV3D_EINVAL, "round_decimals_host: digits is 4 or -1 (unrounded), not %d", digits);
        return NAN;
    }
    return round4(v);
}

extern "C" size_t sgv3d_detections_to_kitti_workspace_bytes(int batch, int n) {
    if (batch < 1 || n < 1 || (long long)batch * n > 0x7fffffffLL) return 0;
    return (size_t)batch * n * sizeof(int32_t);                 // the kept rows' indices of every sample, in input order
}

extern "C" int sgv3d_detections_to_kitti(int batch, int n, const void *boxes, const void *scores, int f64_inputs, const int32_t *labels,
                                         const int32_t *counts, const double *calib, const int8_t *class_table, int num_classes,
                                         double score_thr, int img_w, int img_h, int max_det, int digits, void *workspace,
                                         size_t workspace_bytes, double *fields, int32_t *cls, int32_t *kept, void *stream) {
    KittiParams P;
    const int rc = fill_params("detections_to_kitti", batch, n, boxes, scores, labels, counts, calib, class_table, num_classes,
                               score_thr, img_w, img_h, max_det, digits, f64_inputs, fields, cls, kept, &P);
    if (rc != SGV3D_OK) return rc;
    SGV3D_REQUIRE(workspace, "detections_to_kitti: null pointer");
    const uintptr_t in_mask = f64_inputs ? 7 : 3;
    SGV3D_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)fields & 7) == 0 && ((uintptr_t)calib & 7) == 0 &&
                      ((uintptr_t)boxes & in_mask) == 0 && ((uintptr_t)scores & in_mask) == 0,
                  "detections_to_kitti: misaligned buffer");
    if (workspace_bytes < sgv3d_detections_to_kitti_workspace_bytes(batch, n))
        return sgv3d::fail(SGV3D_ENOSPACE, "detections_to_kitti: workspace of %zu bytes, %zu needed", workspace_bytes,
                           sgv3d_detections_to_kitti_workspace_bytes(batch, n));
    if (f64_inputs)
        hipLaunchKernelGGL(detections_to_kitti_kernel<double>, dim3(batch), dim3(kThreads), 0, as_stream(stream), (const double *)boxes,
                           (const double *)scores, labels, counts, calib, P, (int32_t *)workspace, fields, cls, kept);
    else
        hipLaunchKernelGGL(detections_to_kitti_kernel<float>, dim3(batch), dim3(kThreads), 0, as_stream(stream), (const float *)boxes,
                           (const float *)scores, labels, counts, calib, P, (int32_t *)workspace, fields, cls, kept);
    return check_launch("detections_to_kitti");
}

namespace {

template <typename T>
void detections_to_kitti_host(int batch, int n, const T *boxes, const T *scores, const int32_t *labels, const int32_t *counts,
                              const double *calib, const KittiParams &P, double *fields, int32_t *cls, int32_t *kept) {
    for (int b = 0; b < batch; ++b) {
        const size_t row0 = (size_t)b * n;
        const int cnt = counts[b] < 0 ? 0 : (counts[b] > n ? n : counts[b]);
        int m = 0;
        for (int r = 0; r < cnt; ++r) {
            int c = -1;
            if (!kitti_keep((double)scores[row0 + r], labels[row0 + r], P, &c)) continue;
            if (m < P.max_det) {
                const size_t o = (size_t)b * P.max_det + m;
                kitti_store(boxes + (row0 + r) * 9, scores[row0 + r], c, calib + (size_t)b * kCalib, P, fields + o * kFields, cls + o);
            }
            ++m;
        }
        kept[b] = m;
    }
}

}  // namespace

extern "C" int sgv3d_detections_to_kitti_host(int batch, int n, const void *boxes, const void *scores, int f64_inputs,
                                              const int32_t *labels, const int32_t *counts, const double *calib,
                                              const int8_t *class_table, int num_classes, double score_thr, int img_w, int img_h,
                                              int max_det, int digits, double *fields, int32_t *cls, int32_t *kept) {
    KittiParams P;
    const int rc = fill_params("detections_to_kitti_host", batch, n, boxes, scores, labels, counts, calib, class_table, num_classes,
                               score_thr, img_w, img_h, max_det, digits, f64_inputs, fields, cls, kept, &P);
    if (rc != SGV3D_OK) return rc;
    if (f64_inputs)
        detections_to_kitti_host(batch, n, (const double *)boxes, (const double *)scores, labels, counts, calib, P, fields, cls, kept);
    else
        detections_to_kitti_host(batch, n, (const float *)boxes, (const float *)scores, labels, counts, calib, P, fields, cls, kept);
    return SGV3D_OK;
}
