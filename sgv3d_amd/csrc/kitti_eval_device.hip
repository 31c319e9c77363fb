// The KITTI AP tables on the device: everything between the annotation arrays and the [metric, class, difficulty,
// strict | loose, 41] precision / recall / orientation curves (kitti_utils/eval.py eval_class + clean_data, the host twin
// of which is csrc/kitti_eval.cpp).  One call evaluates every cell = (metric 2-D | BEV | 3-D) x class x difficulty x
// minimum-overlap row; DESIGN.md §18.
//
// Launches, all on the caller's stream, no host wait in between, no float atomics (integer counters only):
//   1 kitti_prep_kernel        zeroes the counters and the status word; BEV (5) and 3-D (7) boxes of both sides
//   2,3 sgv3d_rotate_iou_pairs box_dim 5 and 7 (csrc/rotate_iou.hip, unchanged); float32, read in place, widened exactly
//   4 kitti_overlap2d_kernel   image_box_overlap in float64, one rounding per operation (-ffp-contract=off)
//   5 kitti_match_kernel<0>    the match at threshold 0 without false positives: every ground-truth row g of a cell gets
//                              slot[cell][g] = score of its true positive, or -inf; num_valid_gt per cell
//   6 kitti_sort_kernel        per cell: bitonic sort (descending) of the power-of-two padded slots in global memory, the
//                              true-positive count, then recall_thresholds walked serially by one thread
//   7 kitti_match_kernel<1>    the match with false positives for every (cell, image, threshold): integer tp / fp / fn
//                              added per (cell, threshold), the float64 similarity of an image stored per (cell, image,
//                              threshold)
//   8 kitti_finish_kernel      per cell: the similarity summed in image order, the three divisions (0 / 0 = NaN), the
//                              NaN-propagating running maximum from the right
//
// clean_data runs inside the match: the ignore flags of a ground-truth row come from its name id, occlusion, truncation
// and box height (gt_flag), those of a detection from its class id and box height (dt_flag), DontCare boxes are the rows
// whose name id carries kDontCareBit.  Nothing is built per (class, difficulty) on the host.
//
// THE MATCH.  One wave handles one image of one cell.  Detection j lives in lane j % 64, bit j / 64 of that lane's 64-bit
// masks (at most 4096 detections per image; more sets status bit 1 and the image counts as having none).  Ground-truth
// rows go in order; per row the serial scan over the detections of match_frame (csrc/kitti_eval.cpp) is restated as an
// order-independent reduction over (tier, key, index), larger tier first, then larger key, then LOWER index:
//   candidates      ignored_det != -1, not assigned, score >= threshold (compute_fp only), overlap > min_overlap
//   compute_fp off  candidates with score > -1e7 (the scan's start value); tier 0, key = score.  The scan replaces its choice
//                   on `score > valid` only, so the highest score wins and of equal scores the first.
//   compute_fp on   ignored_det == 0: tier 1, key = overlap.  The scan's max_overlap starts at 0 and min_overlap >= 0 is
//                   required, so the first such candidate is always taken, and a later one only on `overlap > max_overlap`:
//                   the largest overlap wins, of equal overlaps the first.  ignored_det == 1: tier 0, key = 0.  The scan
//                   takes one only while nothing has been chosen (`valid == kNone`), and any later ignored_det == 0
//                   candidate replaces it (`assigned_ignored`): it wins only when no tier-1 candidate exists, and then the
//                   first one does.
// The outcome per row (miss / assigned only / true positive) is match_frame's.  The DontCare discount of the 2-D metric is
// a property of one detection (some DontCare box covers it by more than min_overlap), so it is a mask computed once per
// (cell, image).  An image's orientation similarity is summed in ground-truth order.
//
// Every function the kernels run is __host__ __device__ and is run again by sgv3d_kitti_eval_device_host with the lanes as
// a loop, so the restatement is tested without a GPU.
#include <math.h>

#include <vector>

#include "common.hpp"

namespace {

using sgv3d::as_stream;
using sgv3d::check_launch;

#define KE_HD __host__ __device__ inline

constexpr int kPts = 41;
constexpr int kGtFields = 14;          // x1 y1 x2 y2 | alpha | location 3 | dimensions 3 | rotation_y | truncated | occluded
constexpr int kDtFields = 13;          // alpha | x1 y1 x2 y2 | h l w | x y z | rotation_y | score   (KittiDetections' row)
constexpr int kLanes = 64;
constexpr int kMaxGt = 1 << 28;        // ground-truth rows of a set: the slots of a cell are padded to a power of two
constexpr int kMaxDet = kLanes * 64;   // one bit per detection in a lane's 64-bit masks
constexpr int kWavesPerBlock = 4;
constexpr int kSortThreads = 1024;
constexpr int kDontCareBit = 8;        // name id: kind (0 car 1 pedestrian 2 cyclist 3 bus 4 van 5 person_sitting 6 other) | bit
constexpr double kNone = -10000000.0;  // match_frame's "nothing chosen" score
constexpr int kStatusThresholds = 1, kStatusImage = 2;

struct Params {
    int M, TG, TD, NC, aos, ncell, pad;         // pad: slots per cell, a power of two >= max(TG, 1)
    long long pairs;
    int cls[4];
    double mo[2][3][4];                         // [strict | loose][metric][class index]
};

struct View {
    // the packed input
    const long long *ov_off;                    // [M + 1]
    const int32_t *gt_off, *dt_off, *tile_off;  // [M + 1]
    const double *gt, *dt;                      // [TG, 14], [TD, 13]
    const int32_t *gt_name, *dt_cls;            // [TG], [TD]
    // the workspace
    double *gbox7, *gbox5, *dbox7, *dbox5;
    const float *ov_bev, *ov_3d;                // [pairs], detection-major per image
    double *ov2d;                               // [pairs]
    double *slots;                              // [ncell, pad]
    double *thr;                                // [ncell, 41]
    double *sim;                                // [6 * NC, M, 41]: cells of the 2-D metric only
    unsigned long long *counts;                 // [ncell, 41, 3] tp fp fn
    int32_t *nvalid;                            // [ncell]
    // outputs
    int32_t *nthr;                              // [ncell]
    int32_t *status;                            // [1]
};

size_t up8(size_t n) { return (n + 7) / 8 * 8; }

int pad_of(int total_gt) {
    int p = 1;
    while (p < total_gt) p <<= 1;
    return p;
}

// byte offsets of the packed input's sections; returns the total
size_t packed_layout(int M, int TG, int TD, size_t off[8]) {
    size_t o = 0;
    off[0] = o; o += (size_t)(M + 1) * 8;
    for (int k = 1; k <= 3; ++k) { off[k] = o; o += up8((size_t)(M + 1) * 4); }
    off[4] = o; o += (size_t)TG * kGtFields * 8;
    off[5] = o; o += (size_t)TD * kDtFields * 8;
    off[6] = o; o += up8((size_t)TG * 4);
    off[7] = o; o += up8((size_t)TD * 4);
    return o;
}

enum { W_GBOX7, W_GBOX5, W_DBOX7, W_DBOX5, W_BEV, W_3D, W_OV2D, W_SLOTS, W_THR, W_SIM, W_COUNTS, W_NVALID, W_N };

size_t workspace_layout(int M, int TG, int TD, long long pairs, int NC, size_t off[W_N]) {
    const size_t ncell = (size_t)18 * NC;
    size_t o = 0;
    off[W_GBOX7] = o; o += (size_t)TG * 7 * 8;
    off[W_GBOX5] = o; o += (size_t)TG * 5 * 8;
    off[W_DBOX7] = o; o += (size_t)TD * 7 * 8;
    off[W_DBOX5] = o; o += (size_t)TD * 5 * 8;
    off[W_BEV] = o; o += up8((size_t)pairs * 4);
    off[W_3D] = o; o += up8((size_t)pairs * 4);
    off[W_OV2D] = o; o += (size_t)pairs * 8;
    off[W_SLOTS] = o; o += ncell * (size_t)pad_of(TG) * 8;
    off[W_THR] = o; o += ncell * kPts * 8;
    off[W_SIM] = o; o += (size_t)6 * NC * (size_t)M * kPts * 8;
    off[W_COUNTS] = o; o += ncell * kPts * 3 * 8;
    off[W_NVALID] = o; o += up8(ncell * 4);
    return o;
}

void carve(const Params &P, const void *packed, void *ws, const float *ov_bev, const float *ov_3d, int32_t *nthr, int32_t *status,
           View *v) {
    size_t po[8], wo[W_N];
    packed_layout(P.M, P.TG, P.TD, po);
    workspace_layout(P.M, P.TG, P.TD, P.pairs, P.NC, wo);
    const char *p = (const char *)packed;
    char *w = (char *)ws;
    v->ov_off = (const long long *)(p + po[0]);
    v->gt_off = (const int32_t *)(p + po[1]);
    v->dt_off = (const int32_t *)(p + po[2]);
    v->tile_off = (const int32_t *)(p + po[3]);
    v->gt = (const double *)(p + po[4]);
    v->dt = (const double *)(p + po[5]);
    v->gt_name = (const int32_t *)(p + po[6]);
    v->dt_cls = (const int32_t *)(p + po[7]);
    v->gbox7 = (double *)(w + wo[W_GBOX7]);
    v->gbox5 = (double *)(w + wo[W_GBOX5]);
    v->dbox7 = (double *)(w + wo[W_DBOX7]);
    v->dbox5 = (double *)(w + wo[W_DBOX5]);
    v->ov_bev = ov_bev ? ov_bev : (const float *)(w + wo[W_BEV]);
    v->ov_3d = ov_3d ? ov_3d : (const float *)(w + wo[W_3D]);
    v->ov2d = (double *)(w + wo[W_OV2D]);
    v->slots = (double *)(w + wo[W_SLOTS]);
    v->thr = (double *)(w + wo[W_THR]);
    v->sim = (double *)(w + wo[W_SIM]);
    v->counts = (unsigned long long *)(w + wo[W_COUNTS]);
    v->nvalid = (int32_t *)(w + wo[W_NVALID]);
    v->nthr = nthr;
    v->status = status;
}

// ---------------------------------------------------------------------------------------------- clean_data, per row

KE_HD double min_height(int d) { return d == 0 ? 40.0 : 25.0; }                      // _MIN_HEIGHT
KE_HD double max_occlusion(int d) { return (double)d; }                              // _MAX_OCCLUSION
KE_HD double max_truncation(int d) { return d == 0 ? 0.15 : (d == 1 ? 0.3 : 0.5); }  // _MAX_TRUNCATION

// ignored_gt of clean_data: 0 evaluate, 1 ignore (neighbouring class, or beyond the difficulty's limits), -1 other class
KE_HD int gt_flag(int name_id, int cls, const double *row, int d) {
    const int kind = name_id & 7;
    const bool same = kind == cls;
    const bool near = (cls == 0 && kind == 4) || (cls == 1 && kind == 5);             // _NEIGHBOUR
    const bool hard = row[13] > max_occlusion(d) || row[12] > max_truncation(d) || (row[3] - row[1]) <= min_height(d);
    if (near || (same && hard)) return 1;
    return same ? 0 : -1;
}

// ignored_dt: the height test overrides the class test, as the assignment order of clean_data does
KE_HD int dt_flag(int kind, int cls, const double *row, int d) {
    if (fabs(row[4] - row[2]) < min_height(d)) return 1;
    return kind == cls ? 0 : -1;
}

// numpy's minimum / maximum: a NaN stays
KE_HD double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
KE_HD double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// image_box_overlap, criterion -1; b: the detection's box, q: the ground truth's
KE_HD double overlap2d(const double *b, const double *q) {
    const double iw = np_min(b[2], q[2]) - np_max(b[0], q[0]);
    const double ih = np_min(b[3], q[3]) - np_max(b[1], q[1]);
    const double ab = (b[2] - b[0]) * (b[3] - b[1]);
    const double aq = (q[2] - q[0]) * (q[3] - q[1]);
    const double inter = iw * ih;
    const double ua = ab + aq - inter;
    return (iw > 0 && ih > 0) ? inter / ua : 0.0;
}

// match_frame's DontCare overlap (intersection over the detection's area), with std::min / std::max's choice of operand
KE_HD double overlap_dontcare(const double *b, const double *q) {
    const double iw = (q[2] < b[2] ? q[2] : b[2]) - (b[0] < q[0] ? q[0] : b[0]);
    if (!(iw > 0)) return 0.0;
    const double ih = (q[3] < b[3] ? q[3] : b[3]) - (b[1] < q[1] ? q[1] : b[1]);
    if (!(ih > 0)) return 0.0;
    return iw * ih / ((b[2] - b[0]) * (b[3] - b[1]));
}

// ---------------------------------------------------------------------------------------------- one image of one cell

struct Image {
    int cell, metric, cls, diff, G, D, g0, d0, chunks;
    long long o0;
    double mo;
    bool aos;
};

KE_HD Image image_of(const Params &P, const View &v, int cell, int img, bool *bad) {
    Image im;
    im.cell = cell;
    const int k = cell & 1, d = (cell >> 1) % 3, mc = (cell >> 1) / 3;
    const int c = mc % P.NC;
    im.metric = mc / P.NC;
    im.cls = P.cls[c];
    im.diff = d;
    im.mo = P.mo[k][im.metric][c];
    im.aos = P.aos != 0 && im.metric == 0;
    const long long g0 = v.gt_off[img], g1 = v.gt_off[img + 1], d0 = v.dt_off[img], d1 = v.dt_off[img + 1], o0 = v.ov_off[img];
    // inconsistent offsets: nothing of the image is touched; too many detections: the image counts as having none
    const bool broken = g0 < 0 || g1 < g0 || g1 > P.TG || d0 < 0 || d1 < d0 || d1 > P.TD || o0 < 0 || o0 + (g1 - g0) * (d1 - d0) > P.pairs;
    const bool crowded = !broken && d1 - d0 > kMaxDet;
    *bad = broken || crowded;
    im.g0 = broken ? 0 : (int)g0;
    im.G = broken ? 0 : (int)(g1 - g0);
    im.d0 = *bad ? 0 : (int)d0;
    im.D = *bad ? 0 : (int)(d1 - d0);
    im.o0 = *bad ? 0 : o0;
    im.chunks = (im.D + kLanes - 1) / kLanes;
    return im;
}

KE_HD double overlap_at(const View &v, const Image &im, int j, int i) {
    const long long o = im.o0 + (long long)j * im.G + i;
    return im.metric == 0 ? v.ov2d[o] : (double)(im.metric == 1 ? v.ov_bev[o] : v.ov_3d[o]);
}

struct LaneMasks {
    unsigned long long base, ign1, dontcare;    // ignored_det != -1 | ignored_det == 1 | covered by a DontCare box
};

KE_HD LaneMasks lane_masks(const View &v, const Image &im, int lane) {
    LaneMasks m{0, 0, 0};
    for (int c = 0; c < im.chunks; ++c) {
        const int j = c * kLanes + lane;
        if (j >= im.D) break;
        const double *row = v.dt + (size_t)(im.d0 + j) * kDtFields;
        const int f = dt_flag(v.dt_cls[im.d0 + j], im.cls, row, im.diff);
        if (f != -1) m.base |= 1ull << c;
        if (f == 1) m.ign1 |= 1ull << c;
        if (im.metric == 0 && f == 0) {
            for (int g = 0; g < im.G; ++g) {
                if (!(v.gt_name[im.g0 + g] & kDontCareBit)) continue;
                if (overlap_dontcare(row + 1, v.gt + (size_t)(im.g0 + g) * kGtFields) > im.mo) {
                    m.dontcare |= 1ull << c;
                    break;
                }
            }
        }
    }
    return m;
}

KE_HD unsigned long long lane_below(const View &v, const Image &im, int lane, double thresh) {
    unsigned long long m = 0;
    for (int c = 0; c < im.chunks; ++c) {
        const int j = c * kLanes + lane;
        if (j >= im.D) break;
        if (v.dt[(size_t)(im.d0 + j) * kDtFields + 12] < thresh) m |= 1ull << c;
    }
    return m;
}

struct Best {
    int tier, idx;
    double key;
};

KE_HD Best no_best() { return Best{-1, 0x7fffffff, 0.0}; }

KE_HD bool beats(const Best &a, const Best &b) {
    if (a.tier != b.tier) return a.tier > b.tier;
    if (a.key != b.key) return a.key > b.key;
    return a.idx < b.idx;
}

// a lane's best candidate for ground-truth row i among its eligible detections (bits of `elig`)
template <bool FP>
KE_HD Best lane_best(const View &v, const Image &im, int lane, int i, unsigned long long elig, unsigned long long ign1) {
    Best best = no_best();
    for (int c = 0; c < im.chunks; ++c) {
        if (!((elig >> c) & 1)) continue;
        const int j = c * kLanes + lane;
        const double ov = overlap_at(v, im, j, i);
        if (!(ov > im.mo)) continue;
        Best cand;
        cand.idx = j;
        if (FP) {
            const bool ig = (ign1 >> c) & 1;
            cand.tier = ig ? 0 : 1;
            cand.key = ig ? 0.0 : ov;
        } else {
            cand.tier = 0;
            cand.key = v.dt[(size_t)(im.d0 + j) * kDtFields + 12];
            if (!(cand.key > kNone)) continue;
        }
        if (beats(cand, best)) best = cand;
    }
    return best;
}

struct Counts {
    long long tp, fp, fn;
    double similarity;
};

// What the wave does with the winner of ground-truth row i; `flag` is the row's ignored_gt (not -1).  Returns whether the
// winner becomes assigned.
KE_HD bool settle(const View &v, const Image &im, int i, int flag, const Best &w, bool winner_ign1, Counts *c, double *tp_score) {
    *tp_score = -INFINITY;
    if (w.tier < 0) {
        if (flag == 0) ++c->fn;
        return false;
    }
    if (flag == 1 || winner_ign1) return true;
    ++c->tp;
    const double *drow = v.dt + (size_t)(im.d0 + w.idx) * kDtFields;
    *tp_score = drow[12];
    if (im.aos) c->similarity += (1.0 + cos(v.gt[(size_t)(im.g0 + i) * kGtFields + 4] - drow[0])) / 2.0;
    return true;
}

// get_thresholds / recall_thresholds over the descending scores[0 .. n): returns how many thresholds the walk produces and
// stores the first 41 of them
KE_HD int threshold_walk(const double *scores, long long n, long long num_gt, double *out) {
    double current = 0;
    int count = 0;
    for (long long i = 0; i < n; ++i) {
        const double l = (double)(i + 1) / (double)num_gt;
        const double r = i + 1 < n ? (double)(i + 2) / (double)num_gt : l;
        if ((r - current) < (current - l) && i + 1 < n) continue;
        if (count < kPts) out[count] = scores[i];
        ++count;
        current += 1.0 / (kPts - 1.0);
    }
    return count;
}

KE_HD double nan_max(const double *v, int n) {   // np.max: a NaN anywhere gives NaN
    double m = v[0];
    for (int i = 0; i < n; ++i) {
        if (v[i] != v[i]) return NAN;
        m = m < v[i] ? v[i] : m;
    }
    return m;
}

// the compare-exchange of the bitonic network for element idx at stage (k, j), done by the lower partner of the pair
KE_HD void bitonic_step(double *s, int idx, int k, int j) {
    const int l = idx ^ j;
    if (l <= idx) return;
    const double a = s[idx], b = s[l];
    const bool descending = (idx & k) == 0;
    if (descending ? a < b : a > b) {
        s[idx] = b;
        s[l] = a;
    }
}

KE_HD void box_rows(const double *gt_row, double *b7, double *b5, bool detection) {
    // ground truth: location 5..7, dimensions 8..10, rotation_y 11; detection: h l w 5..7 (dimensions = w h l as the label
    // reader orders them), location 8..10, rotation_y 11
    const double *r = gt_row;
    const double loc[3] = {detection ? r[8] : r[5], detection ? r[9] : r[6], detection ? r[10] : r[7]};
    const double dim[3] = {detection ? r[7] : r[8], detection ? r[5] : r[9], detection ? r[6] : r[10]};
    const double ry = r[11];
    b7[0] = loc[0]; b7[1] = loc[1]; b7[2] = loc[2]; b7[3] = dim[0]; b7[4] = dim[1]; b7[5] = dim[2]; b7[6] = ry;
    b5[0] = loc[0]; b5[1] = loc[2]; b5[2] = dim[0]; b5[3] = dim[2]; b5[4] = ry;
}

// ---------------------------------------------------------------------------------------------- kernels

__global__ __launch_bounds__(256) void kitti_prep_kernel(Params P, View v) {
    const long long n_zero = (long long)P.ncell * kPts * 3;
    const long long total = max(max((long long)P.TG, (long long)P.TD), n_zero);
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        if (t < P.TG) box_rows(v.gt + t * kGtFields, v.gbox7 + t * 7, v.gbox5 + t * 5, false);
        if (t < P.TD) box_rows(v.dt + t * kDtFields, v.dbox7 + t * 7, v.dbox5 + t * 5, true);
        if (t < n_zero) v.counts[t] = 0ull;
        if (t < P.ncell) v.nvalid[t] = 0;
        if (t == 0) *v.status = 0;
    }
}

__global__ __launch_bounds__(256) void kitti_overlap2d_kernel(Params P, View v) {
    bool bad;
    const Image im = image_of(P, v, 0, blockIdx.x, &bad);
    const long long n = (long long)im.G * im.D;
    for (long long p = threadIdx.x; p < n; p += blockDim.x) {
        const int j = (int)(p / im.G), i = (int)(p % im.G);
        v.ov2d[im.o0 + p] = overlap2d(v.dt + (size_t)(im.d0 + j) * kDtFields + 1, v.gt + (size_t)(im.g0 + i) * kGtFields);
    }
}

__device__ __forceinline__ Best wave_best(Best b) {
    for (int s = 1; s < kLanes; s <<= 1) {
        Best o;
        o.tier = __shfl_xor(b.tier, s);
        o.idx = __shfl_xor(b.idx, s);
        o.key = __shfl_xor(b.key, s);
        if (beats(o, b)) b = o;
    }
    return b;
}

__device__ __forceinline__ int wave_sum(int x) {
    for (int s = 1; s < kLanes; s <<= 1) x += __shfl_xor(x, s);
    return x;
}

template <bool FP>
__global__ __launch_bounds__(kWavesPerBlock *kLanes) void kitti_match_kernel(Params P, View v) {
    const int lane = threadIdx.x & (kLanes - 1);
    const long long item = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (item >= (long long)P.ncell * P.M) return;
    const int cell = (int)(item / P.M), img = (int)(item % P.M);
    bool bad;
    const Image im = image_of(P, v, cell, img, &bad);
    if (bad && lane == 0) atomicOr(v.status, kStatusImage);
    const LaneMasks lm = lane_masks(v, im, lane);
    int nthr = 1;
    if (FP) {
        nthr = v.nthr[cell];
        nthr = nthr > kPts ? kPts : nthr;
    }
    for (int t = 0; t < nthr; ++t) {
        unsigned long long assigned = 0, below = 0;
        if (FP) below = lane_below(v, im, lane, v.thr[(size_t)cell * kPts + t]);
        Counts c{0, 0, 0, 0.0};
        int valid = 0;
        for (int i = 0; i < im.G; ++i) {
            const int flag = gt_flag(v.gt_name[im.g0 + i], im.cls, v.gt + (size_t)(im.g0 + i) * kGtFields, im.diff);
            double tp_score = -INFINITY;
            if (flag != -1) {
                valid += flag == 0;
                const Best w = wave_best(lane_best<FP>(v, im, lane, i, lm.base & ~assigned & ~below, lm.ign1));
                const int owner = w.tier < 0 ? 0 : (w.idx & (kLanes - 1));
                const int bit = w.tier < 0 ? 0 : (w.idx >> 6);
                const bool w_ign1 = __shfl((int)((lm.ign1 >> bit) & 1), owner) != 0;
                if (settle(v, im, i, flag, w, w_ign1, &c, &tp_score) && lane == owner) assigned |= 1ull << bit;
            }
            if (!FP && lane == 0) v.slots[(size_t)cell * P.pad + im.g0 + i] = tp_score;
        }
        if (!FP) {
            if (lane == 0 && valid) atomicAdd(v.nvalid + cell, valid);
        } else {
            const int fp = wave_sum(__popcll(lm.base & ~lm.ign1 & ~assigned & ~below & ~lm.dontcare));
            if (lane == 0) {
                unsigned long long *cnt = v.counts + ((size_t)cell * kPts + t) * 3;
                if (c.tp) atomicAdd(cnt, (unsigned long long)c.tp);
                if (fp) atomicAdd(cnt + 1, (unsigned long long)fp);
                if (c.fn) atomicAdd(cnt + 2, (unsigned long long)c.fn);
                if (im.aos) v.sim[((size_t)cell * P.M + img) * kPts + t] = c.similarity;
            }
        }
    }
}

__global__ __launch_bounds__(kSortThreads) void kitti_sort_kernel(Params P, View v) {
    __shared__ int s_n;
    const int cell = blockIdx.x;
    double *s = v.slots + (size_t)cell * P.pad;
    for (int idx = P.TG + threadIdx.x; idx < P.pad; idx += kSortThreads) s[idx] = -INFINITY;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (int k = 2; k <= P.pad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = threadIdx.x; idx < P.pad; idx += kSortThreads) bitonic_step(s, idx, k, j);
            __syncthreads();
        }
    // the number of true positives: the last finite slot of the descending list (at most one thread finds it)
    for (int idx = threadIdx.x; idx < P.pad; idx += kSortThreads)
        if (s[idx] > -INFINITY && (idx + 1 == P.pad || !(s[idx + 1] > -INFINITY))) s_n = idx + 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int count = threshold_walk(s, s_n, v.nvalid[cell], v.thr + (size_t)cell * kPts);
        v.nthr[cell] = count > kPts ? kPts : count;
        if (count > kPts) atomicOr(v.status, kStatusThresholds);
    }
}

KE_HD void finish_raw(const Params &P, const View &v, int cell, int t, int nthr, double *p, double *r, double *o) {
    *p = *r = *o = 0.0;
    if (t >= nthr) return;
    const unsigned long long *cnt = v.counts + ((size_t)cell * kPts + t) * 3;
    const double tp = (double)(long long)cnt[0], fp = (double)(long long)cnt[1], fn = (double)(long long)cnt[2];
    *r = tp / (tp + fn);
    *p = tp / (tp + fp);
    if (P.aos && cell < 6 * P.NC) {
        double sim = 0.0;
        for (int m = 0; m < P.M; ++m) sim += v.sim[((size_t)cell * P.M + m) * kPts + t];
        *o = sim / (tp + fp);
    }
}

__global__ __launch_bounds__(kLanes) void kitti_finish_kernel(Params P, View v, double *precision, double *recall, double *orientation) {
    __shared__ double s_p[kPts], s_r[kPts], s_o[kPts];
    const int cell = blockIdx.x, t = threadIdx.x;
    int nthr = v.nthr[cell];
    nthr = nthr > kPts ? kPts : nthr;
    if (t < kPts) finish_raw(P, v, cell, t, nthr, s_p + t, s_r + t, s_o + t);
    __syncthreads();
    if (t >= kPts) return;
    const size_t o = (size_t)cell * kPts + t;
    const bool live = t < nthr;
    precision[o] = live ? nan_max(s_p + t, kPts - t) : 0.0;
    recall[o] = live ? nan_max(s_r + t, kPts - t) : 0.0;
    orientation[o] = live && P.aos && cell < 6 * P.NC ? nan_max(s_o + t, kPts - t) : 0.0;
}

// ---------------------------------------------------------------------------------------------- argument checks

int fill_params(const char *who, int num_images, int total_gt, int total_dt, long long total_pairs, const void *packed,
                size_t packed_bytes, int num_classes, const int32_t *classes, const double *min_overlaps, int compute_aos,
                const void *precision, const void *recall, const void *orientation, const void *num_thresholds, const void *status,
                Params *P) {
    SGV3D_REQUIRE(num_images >= 0 && total_gt >= 0 && total_dt >= 0 && total_pairs >= 0,
                  "%s: negative count (images %d, ground truth %d, detections %d, pairs %lld)", who, num_images, total_gt, total_dt,
                  total_pairs);
    SGV3D_REQUIRE(num_classes >= 1 && num_classes <= 4, "%s: num_classes %d outside [1, 4]", who, num_classes);
    SGV3D_REQUIRE(packed && classes && min_overlaps && precision && recall && orientation && num_thresholds && status,
                  "%s: null pointer", who);
    SGV3D_REQUIRE(compute_aos == 0 || compute_aos == 1, "%s: compute_aos is 0 or 1, not %d", who, compute_aos);
    // (kMaxGt keeps the sort's stage counter k <= 2 * pad inside an int)
    SGV3D_REQUIRE(total_gt <= kMaxGt && total_pairs <= (long long)total_gt * total_dt, "%s: sizes out of range", who);
    SGV3D_REQUIRE(num_images > 0 || (total_gt == 0 && total_dt == 0), "%s: %d ground-truth and %d detection rows in no image", who, total_gt,
                  total_dt);
    SGV3D_REQUIRE((long long)18 * num_classes * num_images <= 0x7fffffffLL, "%s: too many images", who);
    size_t off[8];
    SGV3D_REQUIRE(packed_bytes == packed_layout(num_images, total_gt, total_dt, off),
                  "%s: the packed input has %zu bytes, its layout for these counts %zu", who, packed_bytes,
                  packed_layout(num_images, total_gt, total_dt, off));
    SGV3D_REQUIRE(((uintptr_t)packed & 7) == 0 && ((uintptr_t)precision & 7) == 0 && ((uintptr_t)recall & 7) == 0 &&
                      ((uintptr_t)orientation & 7) == 0 && ((uintptr_t)num_thresholds & 3) == 0 && ((uintptr_t)status & 3) == 0,
                  "%s: misaligned buffer", who);
    P->M = num_images; P->TG = total_gt; P->TD = total_dt; P->NC = num_classes; P->aos = compute_aos;
    P->ncell = 18 * num_classes;
    P->pad = pad_of(total_gt);
    P->pairs = total_pairs;
    for (int c = 0; c < 4; ++c) {
        P->cls[c] = c < num_classes ? classes[c] : 0;
        SGV3D_REQUIRE(P->cls[c] >= 0 && P->cls[c] <= 3, "%s: class id %d is not 0 (car), 1 (pedestrian), 2 (cyclist) or 3 (bus)", who,
                      P->cls[c]);
    }
    for (int k = 0; k < 2; ++k)
        for (int m = 0; m < 3; ++m)
            for (int c = 0; c < 4; ++c) {
                const double mo = c < num_classes ? min_overlaps[(k * 3 + m) * num_classes + c] : 0.0;
                // the restated selection needs the scan's max_overlap = 0 start to lie at or below every candidate's overlap
                SGV3D_REQUIRE(mo >= 0.0, "%s: minimum overlap %g is negative or NaN", who, mo);
                P->mo[k][m][c] = mo;
            }
    return SGV3D_OK;
}

// ---------------------------------------------------------------------------------------------- the host twin

Best fold_lanes(const Best *lanes) {
    Best b = lanes[0];
    for (int l = 1; l < kLanes; ++l)
        if (beats(lanes[l], b)) b = lanes[l];
    return b;
}

template <bool FP>
void match_host(const Params &P, const View &v) {
    for (int cell = 0; cell < P.ncell; ++cell)
        for (int img = 0; img < P.M; ++img) {
            bool bad;
            const Image im = image_of(P, v, cell, img, &bad);
            if (bad) *v.status |= kStatusImage;
            LaneMasks lm[kLanes];
            for (int l = 0; l < kLanes; ++l) lm[l] = lane_masks(v, im, l);
            int nthr = 1;
            if (FP) nthr = v.nthr[cell] > kPts ? kPts : v.nthr[cell];
            for (int t = 0; t < nthr; ++t) {
                unsigned long long assigned[kLanes] = {}, below[kLanes] = {};
                if (FP)
                    for (int l = 0; l < kLanes; ++l) below[l] = lane_below(v, im, l, v.thr[(size_t)cell * kPts + t]);
                Counts c{0, 0, 0, 0.0};
                int valid = 0;
                for (int i = 0; i < im.G; ++i) {
                    const int flag = gt_flag(v.gt_name[im.g0 + i], im.cls, v.gt + (size_t)(im.g0 + i) * kGtFields, im.diff);
                    double tp_score = -INFINITY;
                    if (flag != -1) {
                        valid += flag == 0;
                        Best lanes[kLanes];
                        for (int l = 0; l < kLanes; ++l)
                            lanes[l] = lane_best<FP>(v, im, l, i, lm[l].base & ~assigned[l] & ~below[l], lm[l].ign1);
                        const Best w = fold_lanes(lanes);
                        const int owner = w.tier < 0 ? 0 : (w.idx & (kLanes - 1)), bit = w.tier < 0 ? 0 : (w.idx >> 6);
                        const bool w_ign1 = (lm[owner].ign1 >> bit) & 1;
                        if (settle(v, im, i, flag, w, w_ign1, &c, &tp_score)) assigned[owner] |= 1ull << bit;
                    }
                    if (!FP) v.slots[(size_t)cell * P.pad + im.g0 + i] = tp_score;
                }
                if (!FP) {
                    v.nvalid[cell] += valid;
                } else {
                    long long fp = 0;
                    for (int l = 0; l < kLanes; ++l)
                        fp += __builtin_popcountll(lm[l].base & ~lm[l].ign1 & ~assigned[l] & ~below[l] & ~lm[l].dontcare);
                    unsigned long long *cnt = v.counts + ((size_t)cell * kPts + t) * 3;
                    cnt[0] += (unsigned long long)c.tp;
                    cnt[1] += (unsigned long long)fp;
                    cnt[2] += (unsigned long long)c.fn;
                    if (im.aos) v.sim[((size_t)cell * P.M + img) * kPts + t] = c.similarity;
                }
            }
        }
}

}  // namespace

extern "C" size_t sgv3d_kitti_eval_device_workspace_bytes(int num_images, int total_gt, int total_dt, long long total_pairs,
                                                          int num_classes) {
    if (num_images < 0 || total_gt < 0 || total_dt < 0 || total_pairs < 0 || num_classes < 1 || num_classes > 4 ||
        total_gt > kMaxGt || total_pairs > (long long)total_gt * total_dt ||
        (num_images == 0 && (total_gt || total_dt)))
        return 0;
    size_t off[W_N];
    return workspace_layout(num_images, total_gt, total_dt, total_pairs, num_classes, off);
}

extern "C" int sgv3d_kitti_eval_device(int num_images, int total_gt, int total_dt, long long total_pairs, int num_tiles,
                                       const void *packed, size_t packed_bytes, int num_classes, const int32_t *classes,
                                       const double *min_overlaps, int compute_aos, void *workspace, size_t workspace_bytes,
                                       double *precision, double *recall, double *orientation, int32_t *num_thresholds,
                                       int32_t *status, void *stream) {
    Params P;
    const int rc = fill_params("kitti_eval_device", num_images, total_gt, total_dt, total_pairs, packed, packed_bytes, num_classes, classes,
                               min_overlaps, compute_aos, precision, recall, orientation, num_thresholds, status, &P);
    if (rc != SGV3D_OK) return rc;
    SGV3D_REQUIRE(num_tiles >= 0, "kitti_eval_device: negative tile count %d", num_tiles);
    SGV3D_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "kitti_eval_device: null or misaligned workspace");
    const size_t need = sgv3d_kitti_eval_device_workspace_bytes(num_images, total_gt, total_dt, total_pairs, num_classes);
    if (workspace_bytes < need)
        return sgv3d::fail(SGV3D_ENOSPACE, "kitti_eval_device: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    View v;
    carve(P, packed, workspace, nullptr, nullptr, num_thresholds, status, &v);
    hipStream_t s = as_stream(stream);
    const long long prep = std::max<long long>(std::max(total_gt, total_dt), (long long)P.ncell * kPts * 3);
    hipLaunchKernelGGL(kitti_prep_kernel, dim3(std::min<long long>(sgv3d::cdiv(prep, 256), 4096)), dim3(256), 0, s, P, v);
    int lrc = check_launch("kitti_prep_kernel");
    if (lrc != SGV3D_OK) return lrc;
    if (num_images > 0 && num_tiles > 0) {
        for (int dim = 5; dim <= 7; dim += 2) {
            lrc = sgv3d_rotate_iou_pairs(num_images, num_tiles, v.dt_off, v.gt_off, v.tile_off, v.ov_off, dim == 5 ? v.dbox5 : v.dbox7,
                                         dim == 5 ? v.gbox5 : v.gbox7, dim, -1, const_cast<float *>(dim == 5 ? v.ov_bev : v.ov_3d), stream);
            if (lrc != SGV3D_OK) return lrc;
        }
    }
    const long long waves = (long long)P.ncell * num_images;
    if (num_images > 0) {
        hipLaunchKernelGGL(kitti_overlap2d_kernel, dim3(num_images), dim3(256), 0, s, P, v);
        if ((lrc = check_launch("kitti_overlap2d_kernel")) != SGV3D_OK) return lrc;
        hipLaunchKernelGGL(kitti_match_kernel<false>, dim3(sgv3d::cdiv(waves, kWavesPerBlock)), dim3(kWavesPerBlock * kLanes), 0, s, P, v);
        if ((lrc = check_launch("kitti_match_kernel<0>")) != SGV3D_OK) return lrc;
    }
    hipLaunchKernelGGL(kitti_sort_kernel, dim3(P.ncell), dim3(kSortThreads), 0, s, P, v);
    if ((lrc = check_launch("kitti_sort_kernel")) != SGV3D_OK) return lrc;
    if (num_images > 0) {
        hipLaunchKernelGGL(kitti_match_kernel<true>, dim3(sgv3d::cdiv(waves, kWavesPerBlock)), dim3(kWavesPerBlock * kLanes), 0, s, P, v);
        if ((lrc = check_launch("kitti_match_kernel<1>")) != SGV3D_OK) return lrc;
    }
    hipLaunchKernelGGL(kitti_finish_kernel, dim3(P.ncell), dim3(kLanes), 0, s, P, v, precision, recall, orientation);
    return check_launch("kitti_finish_kernel");
}

extern "C" int sgv3d_kitti_eval_device_host(int num_images, int total_gt, int total_dt, long long total_pairs, const void *packed,
                                            size_t packed_bytes, const float *overlaps_bev, const float *overlaps_3d, int num_classes,
                                            const int32_t *classes, const double *min_overlaps, int compute_aos, double *precision,
                                            double *recall, double *orientation, int32_t *num_thresholds, int32_t *status,
                                            double *thresholds) {
    Params P;
    const int rc = fill_params("kitti_eval_device_host", num_images, total_gt, total_dt, total_pairs, packed, packed_bytes, num_classes,
                               classes, min_overlaps, compute_aos, precision, recall, orientation, num_thresholds, status, &P);
    if (rc != SGV3D_OK) return rc;
    SGV3D_REQUIRE(total_pairs == 0 || (overlaps_bev && overlaps_3d), "kitti_eval_device_host: null overlaps");
    // the offsets are host memory here: check them before anything is indexed with them
    size_t po[8];
    packed_layout(num_images, total_gt, total_dt, po);
    {
        const char *p = (const char *)packed;
        const long long *oo = (const long long *)(p + po[0]);
        const int32_t *go = (const int32_t *)(p + po[1]), *dof = (const int32_t *)(p + po[2]);
        SGV3D_REQUIRE(oo[0] == 0 && go[0] == 0 && dof[0] == 0, "kitti_eval_device_host: offsets do not start at 0");
        for (int m = 0; m < num_images; ++m) {
            const long long g = (long long)go[m + 1] - go[m], d = (long long)dof[m + 1] - dof[m];
            SGV3D_REQUIRE(g >= 0 && d >= 0, "kitti_eval_device_host: negative count in image %d", m);
            SGV3D_REQUIRE(d <= kMaxDet, "kitti_eval_device_host: image %d has %lld detections, at most %d are matched", m, d, kMaxDet);
            SGV3D_REQUIRE(oo[m + 1] - oo[m] == g * d, "kitti_eval_device_host: overlap offsets of image %d do not match its counts", m);
        }
        SGV3D_REQUIRE(go[num_images] == total_gt && dof[num_images] == total_dt && oo[num_images] == total_pairs,
                      "kitti_eval_device_host: offsets do not end at the totals");
    }
    size_t wo[W_N];
    std::vector<double> ws(workspace_layout(num_images, total_gt, total_dt, total_pairs, num_classes, wo) / 8 + 1);
    View v;
    static const float none = 0.f;
    carve(P, packed, ws.data(), overlaps_bev ? overlaps_bev : &none, overlaps_3d ? overlaps_3d : &none, num_thresholds, status, &v);
    *status = 0;
    for (size_t t = 0; t < (size_t)P.ncell * kPts * 3; ++t) v.counts[t] = 0;
    for (int c = 0; c < P.ncell; ++c) v.nvalid[c] = 0;
    for (int m = 0; m < num_images; ++m) {                                   // kitti_overlap2d_kernel
        bool bad;
        const Image im = image_of(P, v, 0, m, &bad);
        for (long long p = 0; p < (long long)im.G * im.D; ++p)
            v.ov2d[im.o0 + p] = overlap2d(v.dt + (size_t)(im.d0 + p / im.G) * kDtFields + 1, v.gt + (size_t)(im.g0 + p % im.G) * kGtFields);
    }
    match_host<false>(P, v);
    for (int cell = 0; cell < P.ncell; ++cell) {                             // kitti_sort_kernel
        double *s = v.slots + (size_t)cell * P.pad;
        for (int idx = P.TG; idx < P.pad; ++idx) s[idx] = -INFINITY;
        for (int k = 2; k <= P.pad; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1)
                for (int idx = 0; idx < P.pad; ++idx) bitonic_step(s, idx, k, j);
        int n = 0;
        for (int idx = 0; idx < P.pad; ++idx)
            if (s[idx] > -INFINITY && (idx + 1 == P.pad || !(s[idx + 1] > -INFINITY))) n = idx + 1;
        const int count = threshold_walk(s, n, v.nvalid[cell], v.thr + (size_t)cell * kPts);
        v.nthr[cell] = count > kPts ? kPts : count;
        if (count > kPts) *status |= kStatusThresholds;
    }
    if (thresholds)
        for (int cell = 0; cell < P.ncell; ++cell)
            for (int t = 0; t < kPts; ++t) thresholds[cell * kPts + t] = t < v.nthr[cell] ? v.thr[(size_t)cell * kPts + t] : 0.0;
    match_host<true>(P, v);
    for (int cell = 0; cell < P.ncell; ++cell) {                             // kitti_finish_kernel
        double p[kPts], r[kPts], o[kPts];
        const int nthr = v.nthr[cell];
        for (int t = 0; t < kPts; ++t) finish_raw(P, v, cell, t, nthr, p + t, r + t, o + t);
        for (int t = 0; t < kPts; ++t) {
            const size_t at = (size_t)cell * kPts + t;
            const bool live = t < nthr;
            precision[at] = live ? nan_max(p + t, kPts - t) : 0.0;
            recall[at] = live ? nan_max(r + t, kPts - t) : 0.0;
            orientation[at] = live && P.aos && cell < 6 * P.NC ? nan_max(o + t, kPts - t) : 0.0;
        }
    }
    return SGV3D_OK;
}
