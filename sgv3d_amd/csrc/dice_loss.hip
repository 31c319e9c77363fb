// DiceLoss of the reference's losses package (losses/dice.py:57-130 over soft_dice_score, losses/_functional.py:172-187) for
// the semantic maps of the SGV3D BSM branch: value and input gradient without leaving the device.
//
//   sgv3d_dice_loss_forward    two launches.  dice_partial_*: per class c the sums I = sum p*t, P = sum p, T = sum t over the
//                              kept elements; pixels dealt over a fixed grid, per-thread sums in float64 (the float32 products
//                              widened), wave reduce, one partial per (workgroup, class, sum).  dice_finish_kernel (one
//                              workgroup): the partials added in workgroup order, score / loss / d loss / d score in float64.
//   sgv3d_dice_loss_backward   one launch: recomputes the activation and writes every element of the gradient view once.
//
// No float atomics and a fixed summation order: a value and a gradient repeat bit for bit.  Nothing waits on the host between
// the launches, and the upstream factor of backward is read from device memory, so forward + backward capture into a hipGraph.
//
// The maps are small (cfg-5 at batch 2: 2*7*108*192 floats = 1.16 MB): every launch is bounded by its launch latency and one
// dependent trip to HBM / L2, not by bandwidth or by the float64 rate (the backward pass evaluates softmax in float64, ~41 k
// pixels x 7 exponentials).
#include <algorithm>

#include "common.hpp"

using namespace sgv3d;

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / kWave;
constexpr int kDiceBlocks = 256;      // workgroups of the partial pass (one per CU); fewer when the map has fewer pixels
constexpr int kMaxSoftmaxClasses = 32;

struct DiceArgs {
    const float *pred;           // element (b, c, p) at b*sb + c*sc + p*sp
    float *grad;                 // same addressing (backward)
    const void *target;          // kind 0: uint8 [B][P]; 1: int64 [B][P]; 2: float32 addressed like pred
    const float *weight;         // [C] multiplicity of the class in `classes` / len(classes)
    const float *upstream;       // [1] or null (= 1)
    long long sb, sc, sp;
    int batch, classes, pixels, kind, act;
    int use_ignore, log_loss, blocks;
    long long ignore_index;
    double smooth, eps;
    double *partial;             // [blocks][C][3]
    double *saved;               // [C][4]: I, P, T, d loss / d score
    float *out;                  // [1]
};

template <typename R>
__device__ __forceinline__ R exp_of(R x);
template <>
__device__ __forceinline__ float exp_of<float>(float x) { return expf(x); }
template <>
__device__ __forceinline__ double exp_of<double>(double x) { return exp(x); }

template <typename R>
__device__ __forceinline__ R sigmoid_of(R x) {          // exp(logsigmoid(x)), dice.py:68
    const R e = exp_of<R>(x < R(0) ? x : -x);
    return (x >= R(0) ? R(1) : e) / (R(1) + e);
}

__device__ __forceinline__ long long label_at(const DiceArgs &a, long long e) {
    return a.kind == 0 ? (long long)static_cast<const unsigned char *>(a.target)[e] : static_cast<const long long *>(a.target)[e];
}

// (sample, pixel) of element e: a 32-bit division where the element count allows it (the 64-bit one costs as much as the
// rest of a pixel's work)
__device__ __forceinline__ void split_index(long long e, int pixels, bool narrow, long long &b, long long &p) {
    if (narrow) {
        const unsigned q = (unsigned)e / (unsigned)pixels;
        b = q;
        p = (unsigned)e - q * (unsigned)pixels;
    } else {
        b = e / pixels;
        p = e - b * pixels;
    }
}

// NV per-thread sums laid out [3][CMAX] (I, P, T per class), kT threads: wave reduce of the live classes' sums, then the
// waves' values added in wave order; dst[i] valid for every live i after the call.
template <int NV, int CMAX>
__device__ __forceinline__ void block_reduce_store(double (&v)[NV], int classes, double *lds /*[kWaves][NV]*/, double *dst) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i % CMAX < classes) {
            double x = v[i];
            for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
            if ((threadIdx.x & 63) == 0) lds[wave * NV + i] = x;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NV; i += kT) {
        if (i % CMAX < classes) {
            double r = 0;
            for (int w = 0; w < kWaves; ++w) r += lds[w * NV + i];
            dst[i] = r;
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------- partial sums, softmax
// One thread per (sample, pixel): the pixel's classes are kept in registers (CMAX of them), the label is read once.
template <int CMAX>
__global__ void __launch_bounds__(kT) dice_partial_softmax_kernel(DiceArgs a) {
    __shared__ double lds[kWaves * 3 * CMAX];
    double acc[3 * CMAX];                      // [c] I, [CMAX + c] P, [2 CMAX + c] T
#pragma unroll
    for (int i = 0; i < 3 * CMAX; ++i) acc[i] = 0;
    const int C = a.classes;
    const long long total = (long long)a.batch * a.pixels;
    const bool narrow = total <= 0xffffffffLL;
    for (long long e = blockIdx.x * (long long)kT + threadIdx.x; e < total; e += (long long)gridDim.x * kT) {
        const long long lab = label_at(a, e);
        if (a.use_ignore && lab == a.ignore_index) continue;           // m = 0: p*m and t*m add nothing
        long long b, p;
        split_index(e, a.pixels, narrow, b, p);
        const float *x = a.pred + b * a.sb + p * a.sp;
        float v[CMAX];
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) { v[c] = x[c * a.sc]; mx = fmaxf(mx, v[c]); }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) { v[c] = expf(v[c] - mx); sum += v[c]; }
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
                const float pr = v[c] / sum;
                acc[CMAX + c] += (double)pr;
                if (lab == c) { acc[c] += (double)pr; acc[2 * CMAX + c] += 1.0; }
            }
    }
    // partial[block][c][j] <- acc[j * CMAX + c]
    __shared__ double out[3 * CMAX];
    block_reduce_store<3 * CMAX, CMAX>(acc, C, lds, out);
    for (int i = threadIdx.x; i < 3 * C; i += kT) {
        const int c = i / 3, j = i - 3 * c;
        a.partial[((long long)blockIdx.x * C + c) * 3 + j] = out[j * CMAX + c];
    }
}

// ---------------------------------------------------------------------------------------------- partial sums, per element
// binary / multilabel: same-shape float targets, sigmoid or no activation, any number of classes.  The workgroup walks the
// classes; for a class its threads stride over (sample, pixel).
__global__ void __launch_bounds__(kT) dice_partial_elementwise_kernel(DiceArgs a) {
    __shared__ double lds[kWaves * 3];
    const long long total = (long long)a.batch * a.pixels;
    const bool narrow = total <= 0xffffffffLL;
    const float *tg = static_cast<const float *>(a.target);
    const float ign = (float)a.ignore_index;
    for (int c = 0; c < a.classes; ++c) {
        double acc[3] = {0, 0, 0};
        for (long long e = blockIdx.x * (long long)kT + threadIdx.x; e < total; e += (long long)gridDim.x * kT) {
            long long b, p;
            split_index(e, a.pixels, narrow, b, p);
            const long long off = b * a.sb + c * a.sc + p * a.sp;
            const float t = tg[off];
            if (a.use_ignore && t == ign) continue;
            const float x = a.pred[off];
            const float pr = a.act == 1 ? sigmoid_of<float>(x) : x;
            acc[0] += (double)(pr * t);
            acc[1] += (double)pr;
            acc[2] += (double)t;
        }
        block_reduce_store<3, 1>(acc, 1, lds, a.partial + ((long long)blockIdx.x * a.classes + c) * 3);
    }
}

// ---------------------------------------------------------------------------------------------- finish
__device__ __forceinline__ double block_sum_f64(double v, double *lds) {   // kT threads; result valid in thread 0
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kWaves; ++i) r += lds[i];
    __syncthreads();
    return r;
}

// The partials of kFinishGroup classes at a time are staged in LDS by all threads (one trip to memory), then one thread per
// (class, sum) adds its column in workgroup order: a serial walk over global memory would pay a memory latency per partial.
constexpr int kFinishGroup = 8;

__global__ void __launch_bounds__(kT) dice_finish_kernel(DiceArgs a) {
    __shared__ double stage[kDiceBlocks * 3 * kFinishGroup];           // 48 KB
    __shared__ double sums[3 * kFinishGroup];
    __shared__ double lds[kWaves];
    const int C = a.classes;
    double mine = 0;
    for (int c0 = 0; c0 < C; c0 += kFinishGroup) {
        const int g = min(kFinishGroup, C - c0), n = 3 * g;
        for (int idx = threadIdx.x; idx < a.blocks * n; idx += kT) {
            const int blk = idx / n, i = idx - blk * n;
            stage[idx] = a.partial[((long long)blk * C + c0) * 3 + i];
        }
        __syncthreads();
        if ((int)threadIdx.x < n) {
            double s = 0;
#pragma unroll 8
            for (int blk = 0; blk < a.blocks; ++blk) s += stage[blk * n + threadIdx.x];   // index order
            sums[threadIdx.x] = s;
        }
        __syncthreads();
        if ((int)threadIdx.x < g) {
            const int c = c0 + threadIdx.x;
            const double I = sums[3 * threadIdx.x], P = sums[3 * threadIdx.x + 1], T = sums[3 * threadIdx.x + 2];
            const double den = fmax(P + T + a.smooth, a.eps);           // clamp_min(eps), _functional.py:186
            const double score = (2.0 * I + a.smooth) / den;
            double loss, dscore;
            if (a.log_loss) {                                           // dice.py:108-111
                loss = -log(fmax(score, a.eps));
                dscore = score >= a.eps ? -1.0 / score : 0.0;
            } else {
                loss = 1.0 - score;
                dscore = -1.0;
            }
            const double w = T > 0 ? (double)a.weight[c] : 0.0;        // classes without a true pixel count nothing (:118-119)
            a.saved[4 * c + 0] = I;
            a.saved[4 * c + 1] = P;
            a.saved[4 * c + 2] = T;
            a.saved[4 * c + 3] = w * dscore;
            mine += w * loss;
        }
        __syncthreads();
    }
    const double tot = block_sum_f64(mine, lds);
    if (threadIdx.x == 0) a.out[0] = (float)tot;
}

// ---------------------------------------------------------------------------------------------- backward
// d loss / d p[b, c, .] = ca * t + cb with the two per-class constants below (score = (2 I + smooth) / max(den, eps); the clamp
// passes the gradient where den >= eps, as torch's clamp_min does).
__device__ __forceinline__ void class_coefficients(const DiceArgs &a, int c, double &ca, double &cb) {
    const double I = a.saved[4 * c + 0], P = a.saved[4 * c + 1], T = a.saved[4 * c + 2], ds = a.saved[4 * c + 3];
    const double raw = P + T + a.smooth;
    const double den = fmax(raw, a.eps);
    ca = ds * 2.0 / den;
    cb = raw >= a.eps ? -ds * (2.0 * I + a.smooth) / (den * den) : 0.0;
    if (ds == 0.0) { ca = 0.0; cb = 0.0; }
}

template <int CMAX>
__global__ void __launch_bounds__(kT) dice_backward_softmax_kernel(DiceArgs a) {
    __shared__ double s_ca[CMAX], s_cb[CMAX];
    const int C = a.classes;
    if ((int)threadIdx.x < C) {
        double ca, cb;
        class_coefficients(a, threadIdx.x, ca, cb);
        s_ca[threadIdx.x] = ca;
        s_cb[threadIdx.x] = cb;
    }
    __syncthreads();
    const float up = a.upstream ? a.upstream[0] : 1.f;
    const long long total = (long long)a.batch * a.pixels;
    const bool narrow = total <= 0xffffffffLL;
    for (long long e = blockIdx.x * (long long)kT + threadIdx.x; e < total; e += (long long)gridDim.x * kT) {
        long long b, p;
        split_index(e, a.pixels, narrow, b, p);
        const long long base = b * a.sb + p * a.sp;
        const long long lab = label_at(a, e);
        if (a.use_ignore && lab == a.ignore_index) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) a.grad[base + c * a.sc] = 0.f;
            continue;
        }
        double v[CMAX];
        double mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) { v[c] = (double)a.pred[base + c * a.sc]; mx = fmax(mx, v[c]); }
        double sum = 0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) { v[c] = exp(v[c] - mx); sum += v[c]; }
        double dot = 0;                                                  // sum_c g_c p_c
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
                v[c] /= sum;
                dot += ((lab == c ? s_ca[c] : 0.0) + s_cb[c]) * v[c];
            }
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
                const double g = (lab == c ? s_ca[c] : 0.0) + s_cb[c];
                a.grad[base + c * a.sc] = (float)(v[c] * (g - dot)) * up;
            }
    }
}

__global__ void __launch_bounds__(kT) dice_backward_elementwise_kernel(DiceArgs a) {
    const long long total = (long long)a.batch * a.pixels;
    const bool narrow = total <= 0xffffffffLL;
    const float *tg = static_cast<const float *>(a.target);
    const float ign = (float)a.ignore_index;
    const float up = a.upstream ? a.upstream[0] : 1.f;
    for (int c = 0; c < a.classes; ++c) {
        double ca, cb;
        class_coefficients(a, c, ca, cb);
        for (long long e = blockIdx.x * (long long)kT + threadIdx.x; e < total; e += (long long)gridDim.x * kT) {
            long long b, p;
            split_index(e, a.pixels, narrow, b, p);
            const long long off = b * a.sb + c * a.sc + p * a.sp;
            const float t = tg[off];
            double d = 0;
            if (!(a.use_ignore && t == ign)) {
                d = ca * (double)t + cb;
                if (a.act == 1) {
                    const double pr = sigmoid_of<double>((double)a.pred[off]);
                    d *= pr * (1.0 - pr);
                }
            }
            a.grad[off] = (float)d * up;
        }
    }
}

int fill_args(DiceArgs &a, const char *who, int batch, int num_classes, int pixels, const float *pred, long long batch_stride,
              long long class_stride, long long pixel_stride, const void *target, int target_kind, int activation,
              long long ignore_index, int use_ignore_index, double smooth, double eps) {
    SGV3D_REQUIRE(batch > 0 && num_classes > 0 && pixels > 0, "%s: bad sizes", who);
    SGV3D_REQUIRE(pred && target, "%s: null pointer", who);
    SGV3D_REQUIRE(target_kind >= 0 && target_kind <= 2, "%s: target_kind must be 0 (uint8 labels), 1 (int64 labels) or 2 (float targets)", who);
    SGV3D_REQUIRE(activation >= 0 && activation <= 2, "%s: activation must be 0 (none), 1 (sigmoid) or 2 (softmax)", who);
    SGV3D_REQUIRE(activation != 2 || (num_classes >= 2 && num_classes <= kMaxSoftmaxClasses),
                  "%s: softmax covers 2..32 classes", who);
    SGV3D_REQUIRE(activation != 2 || target_kind != 2, "%s: softmax needs integer labels", who);
    SGV3D_REQUIRE(target_kind == 2 || activation == 2, "%s: integer labels need softmax (activation 2)", who);
    a.pred = pred; a.target = target;
    a.sb = batch_stride; a.sc = class_stride; a.sp = pixel_stride;
    a.batch = batch; a.classes = num_classes; a.pixels = pixels; a.kind = target_kind; a.act = activation;
    a.use_ignore = use_ignore_index ? 1 : 0; a.ignore_index = ignore_index; a.smooth = smooth; a.eps = eps;
    return SGV3D_OK;
}

int grid_for(const DiceArgs &a, int cap) { return (int)std::min<long long>(cap, ((long long)a.batch * a.pixels + kT - 1) / kT); }

}  // namespace

extern "C" size_t sgv3d_dice_loss_workspace_bytes(int num_classes) {
    return num_classes > 0 ? (size_t)kDiceBlocks * num_classes * 3 * sizeof(double) : 0;
}

extern "C" int sgv3d_dice_loss_forward(int batch, int num_classes, int pixels, const float *pred, long long batch_stride,
                                       long long class_stride, long long pixel_stride, const void *target, int target_kind,
                                       int activation, long long ignore_index, int use_ignore_index, double smooth, double eps,
                                       int log_loss, const float *class_weight, float *loss_out, double *saved,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    DiceArgs a{};
    if (int rc = fill_args(a, "dice_loss_forward", batch, num_classes, pixels, pred, batch_stride, class_stride, pixel_stride,
                           target, target_kind, activation, ignore_index, use_ignore_index, smooth, eps))
        return rc;
    SGV3D_REQUIRE(class_weight && loss_out && saved && workspace, "dice_loss_forward: null pointer");
    if (workspace_bytes < sgv3d_dice_loss_workspace_bytes(num_classes))
        return fail(SGV3D_ENOSPACE, "dice_loss_forward: workspace too small (%zu bytes, %zu needed)", workspace_bytes,
                    sgv3d_dice_loss_workspace_bytes(num_classes));
    a.weight = class_weight; a.out = loss_out; a.saved = saved; a.log_loss = log_loss ? 1 : 0;
    a.partial = static_cast<double *>(workspace);
    a.blocks = grid_for(a, kDiceBlocks);
    hipStream_t s = as_stream(stream);
    if (activation == 2) {
        if (num_classes <= 8) dice_partial_softmax_kernel<8><<<a.blocks, kT, 0, s>>>(a);
        else if (num_classes <= 16) dice_partial_softmax_kernel<16><<<a.blocks, kT, 0, s>>>(a);
        else dice_partial_softmax_kernel<32><<<a.blocks, kT, 0, s>>>(a);
        if (int rc = check_launch("dice_partial_softmax_kernel")) return rc;
    } else {
        dice_partial_elementwise_kernel<<<a.blocks, kT, 0, s>>>(a);
        if (int rc = check_launch("dice_partial_elementwise_kernel")) return rc;
    }
    dice_finish_kernel<<<1, kT, 0, s>>>(a);
    return check_launch("dice_finish_kernel");
}

extern "C" int sgv3d_dice_loss_backward(int batch, int num_classes, int pixels, const float *pred, long long batch_stride,
                                        long long class_stride, long long pixel_stride, const void *target, int target_kind,
                                        int activation, long long ignore_index, int use_ignore_index, double smooth, double eps,
                                        const double *saved, const float *upstream, float *grad, void *stream) {
    DiceArgs a{};
    if (int rc = fill_args(a, "dice_loss_backward", batch, num_classes, pixels, pred, batch_stride, class_stride, pixel_stride,
                           target, target_kind, activation, ignore_index, use_ignore_index, smooth, eps))
        return rc;
    SGV3D_REQUIRE(saved && grad, "dice_loss_backward: null pointer");
    a.saved = const_cast<double *>(saved); a.upstream = upstream; a.grad = grad;
    hipStream_t s = as_stream(stream);
    const int grid = grid_for(a, 4 * kDiceBlocks);
    if (activation == 2) {
        if (num_classes <= 8) dice_backward_softmax_kernel<8><<<grid, kT, 0, s>>>(a);
        else if (num_classes <= 16) dice_backward_softmax_kernel<16><<<grid, kT, 0, s>>>(a);
        else dice_backward_softmax_kernel<32><<<grid, kT, 0, s>>>(a);
        return check_launch("dice_backward_softmax_kernel");
    }
    dice_backward_elementwise_kernel<<<grid, kT, 0, s>>>(a);
    return check_launch("dice_backward_elementwise_kernel");
}
