// Rotated-IoU BEV NMS of the CenterPoint box decode on the device: the `nms_type='rotate'` branch of mmdet3d 0.18.1
// CenterHead.get_bboxes (get_task_detections + the rotated-box BEV NMS).  mmdet3d is neither vendored in the reference nor
// installed: PARITY UNPINNED, the definition is the one restated in DESIGN.md "Box decode", and tests/decode_rotate_ref.py
// is its float64 restatement.
//
// Input: the candidate stage of decode.hip as it is (K candidates per (task, sample) in descending score order, boxes
// (x, y, z, d0, d1, d2, yaw, vx, vy), the coder's mask `valid`).  One launch, grid (batch, tasks), 512 threads:
//   1. ordered compaction by ballots of the candidates that pass the test score threshold (score >= thr, when thr > 0),
//      cut to the first pre_max_size of them; corner offsets, area and circumscribed radius of each ONCE into LDS
//   2. pairwise phase over all threads: a wave takes a row i, its lanes the candidates j > i of one 64-bit word; the ballot
//      of "circumscribed circles meet" is the word of the suppression bit matrix.  Then every surviving bit is resolved by
//      clipping rectangle j against rectangle i (float32, both translated so that i's centre is the origin): the bit stays
//      when IoU > nms_thr.  A thread resolves word w of row (tid + 67 w) mod CAP, so that the long rows of a cluster of
//      boxes are spread over the threads.
//   3. ONE wave walks the candidates in order: lane t holds word t of the removed set, "is i alive" is a wave-uniform
//      read, a kept i ORs its row in.  keep[:post_max_size], then the post_center_limit_range test on the survivors (a box
//      outside the range has suppressed its neighbours and has used a post_max_size slot by then).
// K <= 512: the bit matrix lives in LDS (512 x 8 x 8 B).  K <= 1024: the plain form, the same code with the matrix in the
// caller's workspace.  No atomics, nothing allocated, no host synchronisation.
//
// This file is compiled with -ffp-contract=off: the host build of the geometry (sgv3d_rotated_bev_iou_host) and the
// device build round every operation once, in the same order.
#include <math.h>

#include "common.hpp"

using namespace sgv3d;

namespace {

constexpr int kThreads = 512;
constexpr int kMaxTasks = 16;

__host__ __device__ inline bool finite_f(float v) { return fabsf(v) <= 3.4028235e38f; }      // false for NaN and +-inf

// THE rectangle convention (mmdet3d 0.18.1, before the v1.0 coordinate refactor; the clockwise one of the KITTI
// evaluator's corners_of in rotate_iou.hip): a corner offset (ox, oy) from the centre, (+-d0/2, +-d1/2), maps to
// (ox cos + oy sin, -ox sin + oy cos).  Offsets only: the centre is added per pair, relative to the other box.
// Order (-,-) (-,+) (+,+) (+,-): clockwise with x to the right and y up, which clip_against() relies on.
__host__ __device__ inline void corner_offsets(float d0, float d1, float yaw, float *off) {
    const float c = cosf(yaw), s = sinf(yaw);
    const float hx = d0 * 0.5f, hy = d1 * 0.5f;
    const float ox[4] = {-hx, -hx, hx, hx};
    const float oy[4] = {-hy, hy, hy, -hy};
    for (int k = 0; k < 4; ++k) {
        off[2 * k] = ox[k] * c + oy[k] * s;
        off[2 * k + 1] = -ox[k] * s + oy[k] * c;
    }
}

struct RBox {
    float x, y;         // centre
    float off[8];       // corner offsets from the centre
    float area, rad;    // d0 * d1, radius of the circumscribed circle
    int ok;             // 0: degenerate (non-finite centre / yaw, extent not finite and positive): IoU 0 with everything
};

__host__ __device__ inline RBox make_rbox(float x, float y, float d0, float d1, float yaw) {
    RBox r;
    r.x = x; r.y = y;
    r.ok = finite_f(x) && finite_f(y) && finite_f(yaw) && finite_f(d0) && finite_f(d1) && d0 > 0.f && d1 > 0.f;
    if (r.ok) {
        corner_offsets(d0, d1, yaw, r.off);
        r.area = d0 * d1;
        r.rad = 0.5f * sqrtf(d0 * d0 + d1 * d1);
    } else {
        for (int k = 0; k < 8; ++k) r.off[k] = 0.f;
        r.area = 0.f; r.rad = 0.f;
    }
    return r;
}

// the circumscribed circles are apart: the rectangles cannot meet (a hair of slack, so that float32 rounding of the
// radii never rejects a pair with a real overlap)
__host__ __device__ inline bool circles_apart(float dx, float dy, float ra, float rb) {
    const float s = ra + rb;
    return dx * dx + dy * dy > s * s * 1.0001f;
}

// Sutherland-Hodgman: the convex polygon p (n points, x/y interleaved) cut by the half plane to the right of a -> b
// (the inside of a clockwise polygon), into q.  Returns the new count (at most n + 1).
__host__ __device__ inline int clip_against(const float *p, int n, float ax, float ay, float bx, float by, float *q) {
    if (n == 0) return 0;
    const float ex = bx - ax, ey = by - ay;
    int m = 0;
    float px = p[2 * (n - 1)], py = p[2 * (n - 1) + 1];
    float sp = ex * (py - ay) - ey * (px - ax);                 // <= 0: inside
    for (int k = 0; k < n; ++k) {
        const float cx = p[2 * k], cy = p[2 * k + 1];
        const float sc = ex * (cy - ay) - ey * (cx - ax);
        if ((sp <= 0.f) != (sc <= 0.f)) {                       // the edge p -> c crosses the line
            const float t = sp / (sp - sc);
            q[2 * m] = px + t * (cx - px);
            q[2 * m + 1] = py + t * (cy - py);
            ++m;
        }
        if (sc <= 0.f) { q[2 * m] = cx; q[2 * m + 1] = cy; ++m; }
        px = cx; py = cy; sp = sc;
    }
    return m;
}

// IoU of two non-degenerate rectangles whose circles meet: b is translated by (dx, dy) = centre(b) - centre(a), a sits at
// the origin.  inter / max(area_a + area_b - inter, 1e-8).
__host__ __device__ inline float clipped_iou(const float *offa, float area_a, const float *offb, float area_b, float dx, float dy) {
    float p[18], q[18];
    for (int k = 0; k < 4; ++k) { p[2 * k] = dx + offb[2 * k]; p[2 * k + 1] = dy + offb[2 * k + 1]; }
    int n = 4;                                                  // (four cuts, p -> q -> p -> q -> p)
    n = clip_against(p, n, offa[0], offa[1], offa[2], offa[3], q);
    n = clip_against(q, n, offa[2], offa[3], offa[4], offa[5], p);
    n = clip_against(p, n, offa[4], offa[5], offa[6], offa[7], q);
    n = clip_against(q, n, offa[6], offa[7], offa[0], offa[1], p);
    float twice = 0.f;
    for (int k = 1; k + 1 < n; ++k)                             // fan of triangles from point 0
        twice += (p[2 * k] - p[0]) * (p[2 * k + 3] - p[1]) - (p[2 * k + 1] - p[1]) * (p[2 * k + 2] - p[0]);
    const float inter = 0.5f * fabsf(twice);
    return inter / fmaxf(area_a + area_b - inter, 1e-8f);
}

__host__ __device__ inline float rotated_bev_iou(const RBox &a, const RBox &b) {
    if (!a.ok || !b.ok) return 0.f;
    const float dx = b.x - a.x, dy = b.y - a.y;
    if (circles_apart(dx, dy, a.rad, b.rad)) return 0.f;
    return clipped_iou(a.off, a.area, b.off, b.area, dx, dy);
}

struct RotateCfg {
    float nms_thr[kMaxTasks];
    float score_thr;            // <= 0: no test-time score filter
    float range[6];
    int has_range, pre_max, post_max;      // the caps: INT_MAX when absent
};

// CAP: candidates a workgroup can hold (a multiple of 64).  LDS_MAT: the bit matrix [CAP][CAP / 64] lives in LDS, else its
// first K rows at `gmat` + (task, sample) * K * CAP / 64.
template <int CAP, bool LDS_MAT>
__global__ __launch_bounds__(kThreads) void rotate_nms_kernel(int K, const float *__restrict__ boxes, const float *__restrict__ scores,
                                                              const unsigned char *__restrict__ valid, const RotateCfg cfg,
                                                              unsigned long long *__restrict__ gmat, unsigned char *__restrict__ keep) {
    constexpr int W = CAP / 64;                       // words of a row
    constexpr int R = CAP / kThreads;                 // candidates per thread in the compaction
    static_assert(W <= 64 && CAP % kThreads == 0, "one lane per word in the walk");
    __shared__ float s_x[CAP], s_y[CAP], s_area[CAP], s_rad[CAP];
    __shared__ float s_off[CAP][8];
    __shared__ short s_cid[CAP];
    __shared__ unsigned char s_flag[CAP];             // bit 0: not degenerate, bit 1: inside post_center_limit_range
    __shared__ int wave_cnt[kThreads / 64];
    __shared__ unsigned long long s_mat[LDS_MAT ? CAP * W : 1];
    const long long cell = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const long long row0 = cell * K;                  // this (task, sample)'s K candidates
    unsigned long long *mat = LDS_MAT ? s_mat : gmat + cell * K * W;
    const float thr = cfg.nms_thr[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // (1) ordered compaction of valid_r, cut at pre_max_size
    int n = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int c = r * kThreads + tid;
        bool v = false;
        if (c < K) {
            keep[row0 + c] = 0;
            v = valid[row0 + c] != 0;
            if (cfg.score_thr > 0.f) v = v && scores[row0 + c] >= cfg.score_thr;
        }
        const unsigned long long m = __ballot(v);
        if (lane == 0) wave_cnt[wid] = __popcll(m);
        __syncthreads();
        int pos = n + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wid) pos += wave_cnt[w];
            n += wave_cnt[w];
        }
        if (v && pos < cfg.pre_max) {
            const float *bx = boxes + (row0 + c) * 9;
            const float x = bx[0], y = bx[1], z = bx[2];
            const RBox rb = make_rbox(x, y, bx[3], bx[4], bx[6]);
            s_cid[pos] = (short)c;
            s_x[pos] = x; s_y[pos] = y; s_area[pos] = rb.area; s_rad[pos] = rb.rad;
#pragma unroll
            for (int k = 0; k < 8; ++k) s_off[pos][k] = rb.off[k];
            bool in = true;
            if (cfg.has_range)
                in = x >= cfg.range[0] && y >= cfg.range[1] && z >= cfg.range[2] && x <= cfg.range[3] && y <= cfg.range[4] &&
                     z <= cfg.range[5];
            s_flag[pos] = (unsigned char)((rb.ok ? 1 : 0) | (in ? 2 : 0));
        }
        __syncthreads();
    }
    n = min(n, cfg.pre_max);
    // (2a) circle test: word w of row i by one ballot (rows i < n, words from the one that holds i + 1 on; the rest zero)
    for (int i = wid; i < n; i += kThreads / 64) {
        const float xi = s_x[i], yi = s_y[i], ri = s_rad[i];
        const bool oki = s_flag[i] & 1;
        for (int w = 0; w < W; ++w) {
            const int j = 64 * w + lane;
            bool near = false;
            if (j > i && j < n && oki && (s_flag[j] & 1)) near = !circles_apart(s_x[j] - xi, s_y[j] - yi, ri, s_rad[j]);
            const unsigned long long m = __ballot(near);
            if (lane == 0) mat[i * W + w] = m;
        }
    }
    __syncthreads();
    // (2b) resolve every set bit by clipping
    for (int rr = 0; rr < R; ++rr) {
        for (int w = 0; w < W; ++w) {
            const int i = (rr * kThreads + tid + 67 * w) & (CAP - 1);
            if (i >= n) continue;
            unsigned long long word = mat[i * W + w], left = word;
            if (left == 0ull) continue;
            float offi[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) offi[k] = s_off[i][k];
            const float xi = s_x[i], yi = s_y[i], ai = s_area[i];
            while (left) {
                const int l = __ffsll((long long)left) - 1;
                left &= left - 1ull;
                const int j = 64 * w + l;
                const float iou = clipped_iou(offi, ai, s_off[j], s_area[j], s_x[j] - xi, s_y[j] - yi);
                if (!(iou > thr)) word &= ~(1ull << l);
            }
            mat[i * W + w] = word;                        // (this thread alone owns the word)
        }
    }
    __syncthreads();
    if (wid != 0) return;
    // (3) the walk: lane t < W holds word t of the removed set
    unsigned long long removed = 0ull;
    int kept = 0;
    for (int i = 0; i < n; ++i) {                         // wave-uniform
        const unsigned lo = __builtin_amdgcn_readlane((unsigned)removed, i >> 6);
        const unsigned hi = __builtin_amdgcn_readlane((unsigned)(removed >> 32), i >> 6);
        if (((((unsigned long long)hi << 32) | lo) >> (i & 63)) & 1ull) continue;
        if (kept >= cfg.post_max) break;                  // keep[:post_max_size]
        ++kept;
        if (lane == 0 && (s_flag[i] & 2)) keep[row0 + s_cid[i]] = 1;
        if (lane < W) removed |= mat[i * W + lane];
    }
}

constexpr int kLdsCap = 512, kPlainCap = 1024;

}  // namespace

extern "C" int sgv3d_rotated_bev_iou_host(int n, const float *a5, const float *b5, float *iou) {
    SGV3D_REQUIRE(n >= 0, "rotated_bev_iou_host: negative count");
    if (n == 0) return SGV3D_OK;
    SGV3D_REQUIRE(a5 && b5 && iou, "rotated_bev_iou_host: null pointer");
    for (int k = 0; k < n; ++k) {
        const float *a = a5 + 5 * (size_t)k, *b = b5 + 5 * (size_t)k;
        iou[k] = rotated_bev_iou(make_rbox(a[0], a[1], a[2], a[3], a[4]), make_rbox(b[0], b[1], b[2], b[3], b[4]));
    }
    return SGV3D_OK;
}

extern "C" size_t sgv3d_rotate_nms_workspace_bytes(int batch, int num_tasks, int max_num) {
    if (batch <= 0 || num_tasks <= 0 || max_num <= 0 || max_num > kPlainCap) return 0;
    // the plain form's bit matrix, max_num rows per (task, sample); the K <= 512 form keeps its matrix in LDS
    const size_t rows = max_num <= kLdsCap ? 0 : (size_t)batch * num_tasks * max_num;
    return rows * (kPlainCap / 64) * sizeof(unsigned long long) + 256;
}

extern "C" int sgv3d_rotate_nms(int batch, int num_tasks, int max_num, const float *boxes, const float *scores,
                                const unsigned char *valid, float score_threshold, const float *nms_thr, int pre_max_size,
                                int post_max_size, const float *limit_range, void *workspace, size_t workspace_bytes,
                                unsigned char *keep, void *stream) {
    SGV3D_REQUIRE(batch > 0 && num_tasks > 0 && num_tasks <= kMaxTasks && max_num > 0,
                  "rotate_nms: non-positive size (or more than %d tasks)", kMaxTasks);
    SGV3D_REQUIRE(max_num <= kPlainCap, "rotate_nms: max_num=%d exceeds %d", max_num, kPlainCap);
    SGV3D_REQUIRE(boxes && scores && valid && nms_thr && keep && workspace, "rotate_nms: null pointer");
    // (an IoU is never negative: with nms_thr >= 0 a pair whose circumscribed circles are apart, IoU 0, never suppresses)
    for (int t = 0; t < num_tasks; ++t) SGV3D_REQUIRE(nms_thr[t] >= 0.f, "rotate_nms: nms_thr[%d] is negative or NaN", t);
    const size_t need = sgv3d_rotate_nms_workspace_bytes(batch, num_tasks, max_num);
    SGV3D_REQUIRE(workspace_bytes >= need, "rotate_nms: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    SGV3D_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "rotate_nms: workspace is not 8-byte aligned");
    RotateCfg cfg;
    for (int t = 0; t < kMaxTasks; ++t) cfg.nms_thr[t] = t < num_tasks ? nms_thr[t] : 0.f;
    cfg.score_thr = score_threshold;
    cfg.has_range = limit_range != nullptr;
    for (int i = 0; i < 6; ++i) cfg.range[i] = limit_range ? limit_range[i] : 0.f;
    cfg.pre_max = pre_max_size > 0 ? pre_max_size : 0x7fffffff;
    cfg.post_max = post_max_size > 0 ? post_max_size : 0x7fffffff;
    const dim3 grid(batch, num_tasks);
    unsigned long long *gmat = static_cast<unsigned long long *>(workspace);
    if (max_num <= kLdsCap)
        hipLaunchKernelGGL((rotate_nms_kernel<kLdsCap, true>), grid, dim3(kThreads), 0, as_stream(stream), max_num, boxes, scores,
                           valid, cfg, gmat, keep);
    else
        hipLaunchKernelGGL((rotate_nms_kernel<kPlainCap, false>), grid, dim3(kThreads), 0, as_stream(stream), max_num, boxes, scores,
                           valid, cfg, gmat, keep);
    return check_launch("rotate_nms");
}
