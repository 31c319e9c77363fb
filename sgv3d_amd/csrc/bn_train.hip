// Training-mode BatchNorm2d fused with the residual add and the ReLU around it, NHWC fp32.
// Reference: every `norm(conv(x))` / `relu(out + identity)` of the mmdet ResNet blocks, SECONDFPN, HeightNet and the
// head (layers/backbones/lss_fpn.py, layers/heads/bev_height_head.py) in training mode, i.e. ATen / MIOpen batch_norm
// with batch statistics + separate add and ReLU kernels.  All four kernels are HBM-bound streams:
//
//   forward   bn_stats_kernel    per-channel sum and sum of squares over the B*H*W pixels (float64 accumulators: no
//                                cancellation in E[x^2] - mean^2), per-block partials
//             bn_finalize_kernel mean, biased variance, 1/sqrt(var + eps), folded scale / shift, running statistics
//                                (momentum, unbiased variance) -- what nn.BatchNorm2d updates in training mode
//             bn_apply_kernel    y = relu(x * scale + shift + residual)              (reads x [+ residual], writes y)
//   backward  bn_bwd_reduce_kernel   dz = dy * (y > 0);  dbeta = sum dz;  dgamma = sum dz * xhat   (float64 partials)
//             bn_bwd_finalize_kernel sums the partials
//             bn_bwd_apply_kernel    dx = gamma * invstd * (dz - dbeta / M - xhat * dgamma / M);  d_residual = dz
//
// Thread layout: 16 lanes x float4 cover 64 channels of a pixel (256 contiguous bytes), 16 pixel rows per block pass;
// a block owns a (64-channel, pixel-range) slab, blockIdx.x = channel group, blockIdx.y = pixel range.
#include "common.hpp"

using namespace sgv3d;

namespace {

constexpr int kMaxBlocks = 1024;  // partial blocks (channel groups x pixel ranges) the workspace is sized for

struct BnArgs {
    const float *x, *res, *y_in, *dy;     // forward: x, res;  backward: x, y_in (forward output, ReLU mask), dy
    float *y, *dx, *dres;
    const float *gamma, *beta;
    float *running_mean, *running_var, *mean, *invstd, *scale, *shift, *dgamma, *dbeta;
    double *partial;                       // [ranges][C][2]
    long long pixels;
    int channels, ranges, pix_per_range, relu;   // relu 2 (backward): the mask is bn(x) > 0 recomputed from x (no residual in the forward)
    float momentum, eps;
};

__global__ __launch_bounds__(256) void bn_stats_kernel(const BnArgs a) {
    __shared__ double lds[16][64][2];
    const int cg = blockIdx.x * 64, c4 = (threadIdx.x & 15) * 4, prow = threadIdx.x >> 4;
    const long long p0 = (long long)blockIdx.y * a.pix_per_range;
    const long long p1 = p0 + a.pix_per_range < a.pixels ? p0 + a.pix_per_range : a.pixels;
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (cg + c4 < a.channels) {
        const float *base = a.x + cg + c4;
        long long p = p0 + prow;
        for (; p + 48 < p1; p += 64) {           // four loads in flight per thread
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(base + (p + 16 * u) * a.channels);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s[0] += v[u].x; s[1] += v[u].y; s[2] += v[u].z; s[3] += v[u].w;
                q[0] += (double)v[u].x * v[u].x; q[1] += (double)v[u].y * v[u].y;
                q[2] += (double)v[u].z * v[u].z; q[3] += (double)v[u].w * v[u].w;
            }
        }
        for (; p < p1; p += 16) {
            const float4 v = *reinterpret_cast<const float4 *>(base + p * a.channels);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
            q[0] += (double)v.x * v.x; q[1] += (double)v.y * v.y; q[2] += (double)v.z * v.z; q[3] += (double)v.w * v.w;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { lds[prow][c4 + i][0] = s[i]; lds[prow][c4 + i][1] = q[i]; }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int c = threadIdx.x >> 1, k = threadIdx.x & 1;
        double t = 0;
        for (int r = 0; r < 16; ++r) t += lds[r][c][k];
        if (cg + c < a.channels) a.partial[((size_t)blockIdx.y * a.channels + cg + c) * 2 + k] = t;
    }
}

// Sum of the per-range partials of channel c: kFinCh channels per block, 256 / kFinCh threads per channel over the range axis (a
// 1024-range layer: 16 independent loads per thread, issued together), the slice sums added in slice order (fixed order);
// s0 / s1 valid in the threads with slice 0.
constexpr int kFinCh = 4, kFinSlices = 256 / kFinCh;

__device__ __forceinline__ void sum_partials(const BnArgs &a, int c, int slice, double (*lds)[kFinCh][2], double &s0, double &s1) {
    double s = 0, q = 0;
    if (c < a.channels) {
        int r = slice;
        for (; r + 3 * kFinSlices < a.ranges; r += 4 * kFinSlices) {
            double2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const double2 *>(a.partial + ((size_t)(r + u * kFinSlices) * a.channels + c) * 2);
#pragma unroll
            for (int u = 0; u < 4; ++u) { s += v[u].x; q += v[u].y; }
        }
        for (; r < a.ranges; r += kFinSlices) {
            const double2 v = *reinterpret_cast<const double2 *>(a.partial + ((size_t)r * a.channels + c) * 2);
            s += v.x;
            q += v.y;
        }
    }
    const int cl = threadIdx.x % kFinCh;
    lds[slice][cl][0] = s;
    lds[slice][cl][1] = q;
    __syncthreads();
    s0 = s1 = 0;
    if (slice == 0)
        for (int i = 0; i < kFinSlices; ++i) { s0 += lds[i][cl][0]; s1 += lds[i][cl][1]; }
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const BnArgs a) {
    __shared__ double lds[kFinSlices][kFinCh][2];
    const int c = blockIdx.x * kFinCh + threadIdx.x % kFinCh, slice = threadIdx.x / kFinCh;
    double s, q;
    sum_partials(a, c, slice, lds, s, q);
    if (slice != 0 || c >= a.channels) return;
    const double m = (double)a.pixels;
    const double mean = s / m;
    double var = q / m - mean * mean;
    var = var > 0 ? var : 0;
    const float invstd = (float)(1.0 / sqrt(var + (double)a.eps));
    a.mean[c] = (float)mean;
    a.invstd[c] = invstd;
    const float g = a.gamma ? a.gamma[c] : 1.f, b = a.beta ? a.beta[c] : 0.f;
    // (explicit roundings: the backward recomputes exactly these two numbers when it derives the ReLU mask from x)
    const float scale = __fmul_rn(g, invstd);
    a.scale[c] = scale;
    a.shift[c] = __fmaf_rn(-(float)mean, scale, b);
    if (a.running_mean) a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * (float)mean;
    if (a.running_var) {
        const double unbiased = m > 1 ? var * m / (m - 1) : var;
        a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * (float)unbiased;
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const BnArgs a) {
    const int c4n = a.channels / 4;
    const long long total = a.pixels * c4n;
    const float4 *x4 = reinterpret_cast<const float4 *>(a.x), *r4 = reinterpret_cast<const float4 *>(a.res);
    const float4 *sc4 = reinterpret_cast<const float4 *>(a.scale), *sh4 = reinterpret_cast<const float4 *>(a.shift);
    float4 *y4 = reinterpret_cast<float4 *>(a.y);
    const float floor_ = a.relu ? 0.f : -__builtin_inff();
    // the grid is sized so that its thread count is a multiple of channels / 4: a thread keeps its channels
    const int c = (int)((blockIdx.x * 256u + threadIdx.x) % (unsigned)c4n);
    const float4 sc = sc4[c], sh = sh4[c];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
        const float4 v = x4[i];
        float4 o = make_float4(__fmaf_rn(v.x, sc.x, sh.x), __fmaf_rn(v.y, sc.y, sh.y), __fmaf_rn(v.z, sc.z, sh.z), __fmaf_rn(v.w, sc.w, sh.w));
        if (r4) {
            const float4 r = r4[i];
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        o.x = fmaxf(o.x, floor_); o.y = fmaxf(o.y, floor_); o.z = fmaxf(o.z, floor_); o.w = fmaxf(o.w, floor_);
        y4[i] = o;
    }
}

// scale / shift of channels c .. c + 3 exactly as bn_finalize_kernel folded them (same roundings)
__device__ __forceinline__ void fold_affine(const BnArgs &a, int c, const float4 mean, const float4 istd, float4 &sc, float4 &sh) {
    float4 g = make_float4(1.f, 1.f, 1.f, 1.f), b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.gamma) g = *reinterpret_cast<const float4 *>(a.gamma + c);
    if (a.beta) b = *reinterpret_cast<const float4 *>(a.beta + c);
    sc = make_float4(__fmul_rn(g.x, istd.x), __fmul_rn(g.y, istd.y), __fmul_rn(g.z, istd.z), __fmul_rn(g.w, istd.w));
    sh = make_float4(__fmaf_rn(-mean.x, sc.x, b.x), __fmaf_rn(-mean.y, sc.y, b.y), __fmaf_rn(-mean.z, sc.z, b.z), __fmaf_rn(-mean.w, sc.w, b.w));
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const BnArgs a) {
    __shared__ double lds[16][64][2];
    const int cg = blockIdx.x * 64, c4 = (threadIdx.x & 15) * 4, prow = threadIdx.x >> 4;
    const long long p0 = (long long)blockIdx.y * a.pix_per_range;
    const long long p1 = p0 + a.pix_per_range < a.pixels ? p0 + a.pix_per_range : a.pixels;
    double sb[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0};
    if (cg + c4 < a.channels) {
        const float4 mean = *reinterpret_cast<const float4 *>(a.mean + cg + c4);
        const float4 istd = *reinterpret_cast<const float4 *>(a.invstd + cg + c4);
        float4 fsc, fsh;
        const bool from_x = a.relu == 2;
        if (from_x) fold_affine(a, cg + c4, mean, istd, fsc, fsh);
        auto one = [&](float4 d, const float4 v, float4 y) {
            if (from_x) y = make_float4(__fmaf_rn(v.x, fsc.x, fsh.x), __fmaf_rn(v.y, fsc.y, fsh.y), __fmaf_rn(v.z, fsc.z, fsh.z), __fmaf_rn(v.w, fsc.w, fsh.w));
            if (a.relu) {
                d.x = y.x > 0.f ? d.x : 0.f; d.y = y.y > 0.f ? d.y : 0.f; d.z = y.z > 0.f ? d.z : 0.f; d.w = y.w > 0.f ? d.w : 0.f;
            }
            sb[0] += d.x; sb[1] += d.y; sb[2] += d.z; sb[3] += d.w;
            sg[0] += (double)d.x * ((v.x - mean.x) * istd.x); sg[1] += (double)d.y * ((v.y - mean.y) * istd.y);
            sg[2] += (double)d.z * ((v.z - mean.z) * istd.z); sg[3] += (double)d.w * ((v.w - mean.w) * istd.w);
        };
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        long long p = p0 + prow;
        for (; p + 16 < p1; p += 32) {           // six loads in flight per thread
            const size_t o0 = p * a.channels + cg + c4, o1 = (p + 16) * a.channels + cg + c4;
            const float4 d0 = *reinterpret_cast<const float4 *>(a.dy + o0), d1 = *reinterpret_cast<const float4 *>(a.dy + o1);
            const float4 v0 = *reinterpret_cast<const float4 *>(a.x + o0), v1 = *reinterpret_cast<const float4 *>(a.x + o1);
            const float4 y0 = a.relu == 1 ? *reinterpret_cast<const float4 *>(a.y_in + o0) : zero;
            const float4 y1 = a.relu == 1 ? *reinterpret_cast<const float4 *>(a.y_in + o1) : zero;
            one(d0, v0, y0);
            one(d1, v1, y1);
        }
        for (; p < p1; p += 16) {
            const size_t o = p * a.channels + cg + c4;
            one(*reinterpret_cast<const float4 *>(a.dy + o), *reinterpret_cast<const float4 *>(a.x + o),
                a.relu == 1 ? *reinterpret_cast<const float4 *>(a.y_in + o) : zero);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { lds[prow][c4 + i][0] = sb[i]; lds[prow][c4 + i][1] = sg[i]; }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int c = threadIdx.x >> 1, k = threadIdx.x & 1;
        double t = 0;
        for (int r = 0; r < 16; ++r) t += lds[r][c][k];
        if (cg + c < a.channels) a.partial[((size_t)blockIdx.y * a.channels + cg + c) * 2 + k] = t;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const BnArgs a) {
    __shared__ double lds[kFinSlices][kFinCh][2];
    const int c = blockIdx.x * kFinCh + threadIdx.x % kFinCh, slice = threadIdx.x / kFinCh;
    double sb, sg;
    sum_partials(a, c, slice, lds, sb, sg);
    if (slice != 0 || c >= a.channels) return;
    a.dbeta[c] = (float)sb;
    a.dgamma[c] = (float)sg;
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnArgs a) {
    const int c4n = a.channels / 4;
    const long long total = a.pixels * c4n;
    const float inv_m = (float)(1.0 / (double)a.pixels);
    const float4 *x4 = reinterpret_cast<const float4 *>(a.x), *y4 = reinterpret_cast<const float4 *>(a.y_in);
    const float4 *d4 = reinterpret_cast<const float4 *>(a.dy);
    float4 *dx4 = reinterpret_cast<float4 *>(a.dx), *dr4 = reinterpret_cast<float4 *>(a.dres);
    const int c = (int)((blockIdx.x * 256u + threadIdx.x) % (unsigned)c4n) * 4;   // constant per thread (grid sizing)
    const float4 mean = *reinterpret_cast<const float4 *>(a.mean + c), istd = *reinterpret_cast<const float4 *>(a.invstd + c);
    float4 db = *reinterpret_cast<const float4 *>(a.dbeta + c), dg = *reinterpret_cast<const float4 *>(a.dgamma + c);
    float4 g = make_float4(1.f, 1.f, 1.f, 1.f);
    if (a.gamma) g = *reinterpret_cast<const float4 *>(a.gamma + c);
    // dx = k1 * (dz - kb - (x - mean) * kg) with k1 = gamma * invstd, kb = dbeta / M, kg = invstd * dgamma / M
    const float4 k1 = make_float4(g.x * istd.x, g.y * istd.y, g.z * istd.z, g.w * istd.w);
    db.x *= inv_m; db.y *= inv_m; db.z *= inv_m; db.w *= inv_m;
    dg.x *= istd.x * inv_m; dg.y *= istd.y * inv_m; dg.z *= istd.z * inv_m; dg.w *= istd.w * inv_m;
    float4 fsc, fsh;
    const bool from_x = a.relu == 2;
    if (from_x) fold_affine(a, c, mean, istd, fsc, fsh);
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
        float4 d = d4[i];
        const float4 v = x4[i];
        if (a.relu) {
            const float4 y = from_x ? make_float4(__fmaf_rn(v.x, fsc.x, fsh.x), __fmaf_rn(v.y, fsc.y, fsh.y), __fmaf_rn(v.z, fsc.z, fsh.z),
                                                  __fmaf_rn(v.w, fsc.w, fsh.w))
                                    : y4[i];
            d.x = y.x > 0.f ? d.x : 0.f; d.y = y.y > 0.f ? d.y : 0.f; d.z = y.z > 0.f ? d.z : 0.f; d.w = y.w > 0.f ? d.w : 0.f;
        }
        if (dr4) dr4[i] = d;
        float4 o;
        o.x = k1.x * (d.x - db.x - (v.x - mean.x) * dg.x);
        o.y = k1.y * (d.y - db.y - (v.y - mean.y) * dg.y);
        o.z = k1.z * (d.z - db.z - (v.z - mean.z) * dg.z);
        o.w = k1.w * (d.w - db.w - (v.w - mean.w) * dg.w);
        dx4[i] = o;
    }
}

int plan(long long pixels, int channels, BnArgs &a) {
    SGV3D_REQUIRE(pixels > 0 && channels > 0 && channels % 4 == 0, "batchnorm: pixels > 0 and channels %% 4 == 0 required");
    a.pixels = pixels; a.channels = channels;
    SGV3D_REQUIRE(cdiv(channels, 64) <= kMaxBlocks, "batchnorm: too many channels");
    // ~1024 blocks of 4 waves with 4 - 6 loads in flight per thread, at least 128 pixels per range
    int ranges = kMaxBlocks / cdiv(channels, 64);
    ranges = ranges < 1 ? 1 : ranges;
    const long long cap = pixels / 128 > 0 ? pixels / 128 : 1;
    ranges = ranges > cap ? (int)cap : ranges;
    a.pix_per_range = (int)((pixels + ranges - 1) / ranges);
    a.ranges = (int)((pixels + a.pix_per_range - 1) / a.pix_per_range);
    return SGV3D_OK;
}

// Blocks of the elementwise passes: about `total / 256` capped at 8192, rounded up to a multiple of c4n / gcd(c4n, 256) so
// that the thread count is a multiple of c4n (= channels / 4) and every thread keeps its channel chunk.
int stream_blocks(long long total, int c4n) {
    long long b = (total + 255) / 256;
    b = b < 8192 ? b : 8192;
    int g = c4n, h = 256;
    while (h) { const int t = g % h; g = h; h = t; }
    const int step = c4n / g;
    return (int)((b + step - 1) / step * step);
}

size_t partial_bytes(int) { return (size_t)kMaxBlocks * 64 * 2 * sizeof(double); }

}  // namespace

extern "C" size_t sgv3d_batchnorm_workspace_bytes(int channels) {
    return channels > 0 ? partial_bytes(channels) + 2 * (size_t)channels * sizeof(float) : 0;
}

extern "C" int sgv3d_batchnorm_train_forward(long long pixels, int channels, const float *x, const float *residual,
                                             const float *gamma, const float *beta, float *running_mean,
                                             float *running_var, float momentum, float eps, int relu, float *y,
                                             float *save_mean, float *save_invstd, void *workspace,
                                             size_t workspace_bytes, void *stream) {
    BnArgs a{};
    if (int rc = plan(pixels, channels, a)) return rc;
    SGV3D_REQUIRE(x && y && save_mean && save_invstd && workspace, "batchnorm_train_forward: null pointer");
    SGV3D_REQUIRE(workspace_bytes >= sgv3d_batchnorm_workspace_bytes(channels), "batchnorm_train_forward: workspace too small");
    SGV3D_REQUIRE(aligned16(x) && aligned16(y) && (!residual || aligned16(residual)) && aligned16(workspace),
                  "batchnorm_train_forward: buffers must be 16-byte aligned");
    a.x = x; a.res = residual; a.y = y; a.gamma = gamma; a.beta = beta; a.running_mean = running_mean;
    a.running_var = running_var; a.mean = save_mean; a.invstd = save_invstd; a.momentum = momentum; a.eps = eps; a.relu = relu;
    a.partial = static_cast<double *>(workspace);
    a.scale = reinterpret_cast<float *>(static_cast<char *>(workspace) + partial_bytes(channels));
    a.shift = a.scale + channels;
    hipStream_t s = as_stream(stream);
    bn_stats_kernel<<<dim3(cdiv(channels, 64), a.ranges), 256, 0, s>>>(a);
    if (int rc = check_launch("bn_stats_kernel")) return rc;
    bn_finalize_kernel<<<cdiv(channels, kFinCh), 256, 0, s>>>(a);
    if (int rc = check_launch("bn_finalize_kernel")) return rc;
    bn_apply_kernel<<<stream_blocks(pixels * (channels / 4), channels / 4), 256, 0, s>>>(a);
    return check_launch("bn_apply_kernel");
}

namespace {
int bn_backward(long long pixels, int channels, const float *x, const float *y, const float *dy, const float *gamma, const float *beta,
                const float *save_mean, const float *save_invstd, int relu, float *dx, float *dresidual, float *dgamma, float *dbeta,
                void *workspace, size_t workspace_bytes, void *stream);
}

extern "C" int sgv3d_batchnorm_train_backward(long long pixels, int channels, const float *x, const float *y,
                                              const float *dy, const float *gamma, const float *save_mean,
                                              const float *save_invstd, int relu, float *dx, float *dresidual,
                                              float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                              void *stream) {
    SGV3D_REQUIRE(!relu || y, "batchnorm_train_backward: the forward output is needed for the ReLU mask");
    return bn_backward(pixels, channels, x, y, dy, gamma, nullptr, save_mean, save_invstd, relu ? 1 : 0, dx, dresidual, dgamma, dbeta,
                       workspace, workspace_bytes, stream);
}

extern "C" int sgv3d_batchnorm_relu_train_backward_from_x(long long pixels, int channels, const float *x, const float *dy,
                                                          const float *gamma, const float *beta, const float *save_mean,
                                                          const float *save_invstd, float *dx, float *dgamma, float *dbeta,
                                                          void *workspace, size_t workspace_bytes, void *stream) {
    SGV3D_REQUIRE((!gamma || aligned16(gamma)) && (!beta || aligned16(beta)), "batchnorm_relu_train_backward_from_x: gamma / beta must be 16-byte aligned");
    return bn_backward(pixels, channels, x, nullptr, dy, gamma, beta, save_mean, save_invstd, 2, dx, nullptr, dgamma, dbeta, workspace,
                       workspace_bytes, stream);
}

namespace {
int bn_backward(long long pixels, int channels, const float *x, const float *y, const float *dy, const float *gamma, const float *beta,
                const float *save_mean, const float *save_invstd, int relu, float *dx, float *dresidual, float *dgamma, float *dbeta,
                void *workspace, size_t workspace_bytes, void *stream) {
    BnArgs a{};
    if (int rc = plan(pixels, channels, a)) return rc;
    SGV3D_REQUIRE(x && dy && save_mean && save_invstd && dx && dgamma && dbeta && workspace, "batchnorm_train_backward: null pointer");
    a.beta = beta;
    SGV3D_REQUIRE(workspace_bytes >= sgv3d_batchnorm_workspace_bytes(channels), "batchnorm_train_backward: workspace too small");
    SGV3D_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dx) && (!y || aligned16(y)) && (!dresidual || aligned16(dresidual)) &&
                  aligned16(save_mean) && aligned16(save_invstd) && aligned16(dgamma) && aligned16(dbeta) && (!gamma || aligned16(gamma)),
                  "batchnorm_train_backward: buffers must be 16-byte aligned");
    a.x = x; a.y_in = y; a.dy = dy; a.gamma = gamma; a.mean = const_cast<float *>(save_mean);
    a.invstd = const_cast<float *>(save_invstd); a.relu = relu; a.dx = dx; a.dres = dresidual; a.dgamma = dgamma; a.dbeta = dbeta;
    a.partial = static_cast<double *>(workspace);
    hipStream_t s = as_stream(stream);
    bn_bwd_reduce_kernel<<<dim3(cdiv(channels, 64), a.ranges), 256, 0, s>>>(a);
    if (int rc = check_launch("bn_bwd_reduce_kernel")) return rc;
    bn_bwd_finalize_kernel<<<cdiv(channels, kFinCh), 256, 0, s>>>(a);
    if (int rc = check_launch("bn_bwd_finalize_kernel")) return rc;
    bn_bwd_apply_kernel<<<stream_blocks(pixels * (channels / 4), channels / 4), 256, 0, s>>>(a);
    return check_launch("bn_bwd_apply_kernel");
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// The same three entries on bf16 NHWC tensors (mixed-precision training with bf16 activation storage, hip_ops.TRAIN_BF16_STORAGE):
// x, residual, y, dy, dx, d_residual are bf16, everything per channel stays f32 and the per-range partials float64.  The arithmetic
// is the f32 kernels' on the upcast values (an upcast is exact), followed by ONE round-to-nearest-even where a map is written; the
// workspace, the plan, the finalize kernels and their roundings are the ones above.  The passes move half the bytes, which is all
// that can make an HBM-bound stream faster.
//
// Thread layout: one 16-byte load is 8 channels; 8 lanes cover 64 channels of a pixel (128 contiguous bytes), 32 pixel rows per
// block pass; a block owns the same (64-channel, pixel-range) slab as above, so the partial layout is unchanged.  channels % 8 == 0.
namespace {

typedef __bf16 bn_bf16x8 __attribute__((ext_vector_type(8)));
typedef float bn_f32x8 __attribute__((ext_vector_type(8)));

struct BnMaps16 {                          // the bf16 maps of a call (BnArgs carries the f32 / f64 side)
    const unsigned short *x, *res, *y_in, *dy;
    unsigned short *y, *dx, *dres;
};

__device__ __forceinline__ bn_f32x8 up8(const uint4 w) {
    bn_f32x8 v;
    v[0] = __uint_as_float(w.x << 16); v[1] = __uint_as_float(w.x & 0xffff0000u);
    v[2] = __uint_as_float(w.y << 16); v[3] = __uint_as_float(w.y & 0xffff0000u);
    v[4] = __uint_as_float(w.z << 16); v[5] = __uint_as_float(w.z & 0xffff0000u);
    v[6] = __uint_as_float(w.w << 16); v[7] = __uint_as_float(w.w & 0xffff0000u);
    return v;
}

__device__ __forceinline__ uint4 down8(const bn_f32x8 v) {      // round to nearest even
    return __builtin_bit_cast(uint4, __builtin_convertvector(v, bn_bf16x8));
}

__device__ __forceinline__ bn_f32x8 ld8f(const float *p) {
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    bn_f32x8 v = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return v;
}

// scale / shift of channels c .. c + 7 exactly as bn_finalize_kernel folded them (fold_affine on both halves)
__device__ __forceinline__ void fold_affine8(const BnArgs &a, int c, const bn_f32x8 mean, const bn_f32x8 istd, bn_f32x8 &sc, bn_f32x8 &sh) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float4 s4, h4;
        fold_affine(a, c + 4 * h, make_float4(mean[4 * h], mean[4 * h + 1], mean[4 * h + 2], mean[4 * h + 3]),
                    make_float4(istd[4 * h], istd[4 * h + 1], istd[4 * h + 2], istd[4 * h + 3]), s4, h4);
        sc[4 * h] = s4.x; sc[4 * h + 1] = s4.y; sc[4 * h + 2] = s4.z; sc[4 * h + 3] = s4.w;
        sh[4 * h] = h4.x; sh[4 * h + 1] = h4.y; sh[4 * h + 2] = h4.z; sh[4 * h + 3] = h4.w;
    }
}

// the 32 row sums of a block's 64 channels, added in row order, to the partials of this pixel range
__device__ __forceinline__ void block_partials16(const BnArgs &a, double (*lds)[64][2], int cg, int c8, int prow, const double *s, const double *q) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { lds[prow][c8 + i][0] = s[i]; lds[prow][c8 + i][1] = q[i]; }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int c = threadIdx.x >> 1, k = threadIdx.x & 1;
        double t = 0;
        for (int r = 0; r < 32; ++r) t += lds[r][c][k];
        if (cg + c < a.channels) a.partial[((size_t)blockIdx.y * a.channels + cg + c) * 2 + k] = t;
    }
}

__global__ __launch_bounds__(256) void bn_stats_bf16_kernel(const BnArgs a, const BnMaps16 t) {
    __shared__ double lds[32][64][2];
    const int cg = blockIdx.x * 64, c8 = (threadIdx.x & 7) * 8, prow = threadIdx.x >> 3;
    const long long p0 = (long long)blockIdx.y * a.pix_per_range;
    const long long p1 = p0 + a.pix_per_range < a.pixels ? p0 + a.pix_per_range : a.pixels;
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (cg + c8 < a.channels) {
        const unsigned short *base = t.x + cg + c8;
        long long p = p0 + prow;
        for (; p + 96 < p1; p += 128) {          // four loads in flight per thread
            uint4 w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const uint4 *>(base + (p + 32 * u) * a.channels);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bn_f32x8 v = up8(w[u]);
#pragma unroll
                for (int i = 0; i < 8; ++i) { s[i] += v[i]; q[i] += (double)v[i] * v[i]; }
            }
        }
        for (; p < p1; p += 32) {
            const bn_f32x8 v = up8(*reinterpret_cast<const uint4 *>(base + p * a.channels));
#pragma unroll
            for (int i = 0; i < 8; ++i) { s[i] += v[i]; q[i] += (double)v[i] * v[i]; }
        }
    }
    block_partials16(a, lds, cg, c8, prow, s, q);
}

__global__ __launch_bounds__(256) void bn_apply_bf16_kernel(const BnArgs a, const BnMaps16 t) {
    const int c8n = a.channels / 8;
    const long long total = a.pixels * c8n;
    const uint4 *x8 = reinterpret_cast<const uint4 *>(t.x), *r8 = reinterpret_cast<const uint4 *>(t.res);
    uint4 *y8 = reinterpret_cast<uint4 *>(t.y);
    const float floor_ = a.relu ? 0.f : -__builtin_inff();
    // the grid is sized so that its thread count is a multiple of channels / 8: a thread keeps its channels
    const int c = (int)((blockIdx.x * 256u + threadIdx.x) % (unsigned)c8n) * 8;
    const bn_f32x8 sc = ld8f(a.scale + c), sh = ld8f(a.shift + c);
    auto one = [&](const uint4 xw, const uint4 rw) {
        const bn_f32x8 v = up8(xw), r = up8(rw);
        bn_f32x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float e = __fmaf_rn(v[i], sc[i], sh[i]);
            if (r8) e += r[i];
            o[i] = fmaxf(e, floor_);
        }
        return down8(o);
    };
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);
    const long long stride = gridDim.x * 256ll;
    long long i = blockIdx.x * 256ll + threadIdx.x;
    for (; i + stride < total; i += 2 * stride) {      // two (four with a residual) loads in flight per thread
        const uint4 x0 = x8[i], x1 = x8[i + stride];
        const uint4 r0 = r8 ? r8[i] : none, r1 = r8 ? r8[i + stride] : none;
        y8[i] = one(x0, r0);
        y8[i + stride] = one(x1, r1);
    }
    if (i < total) y8[i] = one(x8[i], r8 ? r8[i] : none);
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_bf16_kernel(const BnArgs a, const BnMaps16 t) {
    __shared__ double lds[32][64][2];
    const int cg = blockIdx.x * 64, c8 = (threadIdx.x & 7) * 8, prow = threadIdx.x >> 3;
    const long long p0 = (long long)blockIdx.y * a.pix_per_range;
    const long long p1 = p0 + a.pix_per_range < a.pixels ? p0 + a.pix_per_range : a.pixels;
    double sb[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (cg + c8 < a.channels) {
        const bn_f32x8 mean = ld8f(a.mean + cg + c8), istd = ld8f(a.invstd + cg + c8);
        bn_f32x8 fsc = {}, fsh = {};
        const bool from_x = a.relu == 2;
        if (from_x) fold_affine8(a, cg + c8, mean, istd, fsc, fsh);
        auto one = [&](const uint4 dw, const uint4 xw, const uint4 yw) {
            bn_f32x8 d = up8(dw);
            const bn_f32x8 v = up8(xw);
            bn_f32x8 y = up8(yw);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (from_x) y[i] = __fmaf_rn(v[i], fsc[i], fsh[i]);
                if (a.relu) d[i] = y[i] > 0.f ? d[i] : 0.f;
                sb[i] += d[i];
                sg[i] += (double)d[i] * ((v[i] - mean[i]) * istd[i]);
            }
        };
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        long long p = p0 + prow;
        for (; p + 32 < p1; p += 64) {           // six loads in flight per thread
            const size_t o0 = p * a.channels + cg + c8, o1 = (p + 32) * a.channels + cg + c8;
            const uint4 d0 = *reinterpret_cast<const uint4 *>(t.dy + o0), d1 = *reinterpret_cast<const uint4 *>(t.dy + o1);
            const uint4 v0 = *reinterpret_cast<const uint4 *>(t.x + o0), v1 = *reinterpret_cast<const uint4 *>(t.x + o1);
            const uint4 y0 = a.relu == 1 ? *reinterpret_cast<const uint4 *>(t.y_in + o0) : zero;
            const uint4 y1 = a.relu == 1 ? *reinterpret_cast<const uint4 *>(t.y_in + o1) : zero;
            one(d0, v0, y0);
            one(d1, v1, y1);
        }
        for (; p < p1; p += 32) {
            const size_t o = p * a.channels + cg + c8;
            one(*reinterpret_cast<const uint4 *>(t.dy + o), *reinterpret_cast<const uint4 *>(t.x + o),
                a.relu == 1 ? *reinterpret_cast<const uint4 *>(t.y_in + o) : zero);
        }
    }
    block_partials16(a, lds, cg, c8, prow, sb, sg);
}

__global__ __launch_bounds__(256) void bn_bwd_apply_bf16_kernel(const BnArgs a, const BnMaps16 t) {
    const int c8n = a.channels / 8;
    const long long total = a.pixels * c8n;
    const float inv_m = (float)(1.0 / (double)a.pixels);
    const uint4 *x8 = reinterpret_cast<const uint4 *>(t.x), *y8 = reinterpret_cast<const uint4 *>(t.y_in);
    const uint4 *d8 = reinterpret_cast<const uint4 *>(t.dy);
    uint4 *dx8 = reinterpret_cast<uint4 *>(t.dx), *dr8 = reinterpret_cast<uint4 *>(t.dres);
    const int c = (int)((blockIdx.x * 256u + threadIdx.x) % (unsigned)c8n) * 8;   // constant per thread (grid sizing)
    const bn_f32x8 mean = ld8f(a.mean + c), istd = ld8f(a.invstd + c);
    bn_f32x8 db = ld8f(a.dbeta + c), dg = ld8f(a.dgamma + c), k1;
    // dx = k1 * (dz - kb - (x - mean) * kg) with k1 = gamma * invstd, kb = dbeta / M, kg = invstd * dgamma / M
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        k1[i] = (a.gamma ? a.gamma[c + i] : 1.f) * istd[i];
        db[i] *= inv_m;
        dg[i] *= istd[i] * inv_m;
    }
    bn_f32x8 fsc = {}, fsh = {};
    const bool from_x = a.relu == 2, with_y = a.relu == 1;
    if (from_x) fold_affine8(a, c, mean, istd, fsc, fsh);
    auto one = [&](long long i, const uint4 dw, const uint4 xw, const uint4 yw) {
        bn_f32x8 d = up8(dw), o;
        const bn_f32x8 v = up8(xw), ys = up8(yw);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (a.relu) {
                const float y = from_x ? __fmaf_rn(v[k], fsc[k], fsh[k]) : ys[k];
                d[k] = y > 0.f ? d[k] : 0.f;
            }
            o[k] = k1[k] * (d[k] - db[k] - (v[k] - mean[k]) * dg[k]);
        }
        if (dr8) dr8[i] = down8(d);            // (a masked copy of dy: exact)
        dx8[i] = down8(o);
    };
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const long long stride = gridDim.x * 256ll;
    long long i = blockIdx.x * 256ll + threadIdx.x;
    for (; i + stride < total; i += 2 * stride) {      // four to six loads in flight per thread
        const uint4 d0 = d8[i], d1 = d8[i + stride], v0 = x8[i], v1 = x8[i + stride];
        const uint4 y0 = with_y ? y8[i] : zero, y1 = with_y ? y8[i + stride] : zero;
        one(i, d0, v0, y0);
        one(i + stride, d1, v1, y1);
    }
    if (i < total) one(i, d8[i], x8[i], with_y ? y8[i] : zero);
}

int plan16(long long pixels, int channels, BnArgs &a) {
    SGV3D_REQUIRE(channels > 0 && channels % 8 == 0, "batchnorm (bf16 tensors): channels %% 8 == 0 required");
    return plan(pixels, channels, a);
}

int bn_backward16(long long pixels, int channels, const void *x, const void *y, const void *dy, const float *gamma, const float *beta,
                  const float *save_mean, const float *save_invstd, int relu, void *dx, void *dresidual, float *dgamma, float *dbeta,
                  void *workspace, size_t workspace_bytes, void *stream) {
    BnArgs a{};
    if (int rc = plan16(pixels, channels, a)) return rc;
    SGV3D_REQUIRE(x && dy && save_mean && save_invstd && dx && dgamma && dbeta && workspace, "batchnorm_train_backward_bf16: null pointer");
    SGV3D_REQUIRE(workspace_bytes >= sgv3d_batchnorm_workspace_bytes(channels), "batchnorm_train_backward_bf16: workspace too small");
    SGV3D_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dx) && (!y || aligned16(y)) && (!dresidual || aligned16(dresidual)) &&
                  aligned16(save_mean) && aligned16(save_invstd) && aligned16(dgamma) && aligned16(dbeta) && (!gamma || aligned16(gamma)) &&
                  (!beta || aligned16(beta)) && aligned16(workspace),
                  "batchnorm_train_backward_bf16: buffers must be 16-byte aligned");
    a.gamma = gamma; a.beta = beta; a.mean = const_cast<float *>(save_mean); a.invstd = const_cast<float *>(save_invstd);
    a.relu = relu; a.dgamma = dgamma; a.dbeta = dbeta;
    a.partial = static_cast<double *>(workspace);
    BnMaps16 t{};
    t.x = static_cast<const unsigned short *>(x); t.y_in = static_cast<const unsigned short *>(y);
    t.dy = static_cast<const unsigned short *>(dy); t.dx = static_cast<unsigned short *>(dx);
    t.dres = static_cast<unsigned short *>(dresidual);
    hipStream_t s = as_stream(stream);
    bn_bwd_reduce_bf16_kernel<<<dim3(cdiv(channels, 64), a.ranges), 256, 0, s>>>(a, t);
    if (int rc = check_launch("bn_bwd_reduce_bf16_kernel")) return rc;
    bn_bwd_finalize_kernel<<<cdiv(channels, kFinCh), 256, 0, s>>>(a);
    if (int rc = check_launch("bn_bwd_finalize_kernel")) return rc;
    bn_bwd_apply_bf16_kernel<<<stream_blocks(pixels * (channels / 8), channels / 8), 256, 0, s>>>(a, t);
    return check_launch("bn_bwd_apply_bf16_kernel");
}

}  // namespace

extern "C" int sgv3d_batchnorm_train_forward_bf16(long long pixels, int channels, const void *x, const void *residual,
                                                  const float *gamma, const float *beta, float *running_mean,
                                                  float *running_var, float momentum, float eps, int relu, void *y,
                                                  float *save_mean, float *save_invstd, void *workspace,
                                                  size_t workspace_bytes, void *stream) {
    BnArgs a{};
    if (int rc = plan16(pixels, channels, a)) return rc;
    SGV3D_REQUIRE(x && y && save_mean && save_invstd && workspace, "batchnorm_train_forward_bf16: null pointer");
    SGV3D_REQUIRE(workspace_bytes >= sgv3d_batchnorm_workspace_bytes(channels), "batchnorm_train_forward_bf16: workspace too small");
    SGV3D_REQUIRE(aligned16(x) && aligned16(y) && (!residual || aligned16(residual)) && aligned16(workspace),
                  "batchnorm_train_forward_bf16: buffers must be 16-byte aligned");
    a.gamma = gamma; a.beta = beta; a.running_mean = running_mean; a.running_var = running_var; a.mean = save_mean;
    a.invstd = save_invstd; a.momentum = momentum; a.eps = eps; a.relu = relu;
    a.partial = static_cast<double *>(workspace);
    a.scale = reinterpret_cast<float *>(static_cast<char *>(workspace) + partial_bytes(channels));
    a.shift = a.scale + channels;
    BnMaps16 t{};
    t.x = static_cast<const unsigned short *>(x); t.res = static_cast<const unsigned short *>(residual);
    t.y = static_cast<unsigned short *>(y);
    hipStream_t s = as_stream(stream);
    bn_stats_bf16_kernel<<<dim3(cdiv(channels, 64), a.ranges), 256, 0, s>>>(a, t);
    if (int rc = check_launch("bn_stats_bf16_kernel")) return rc;
    bn_finalize_kernel<<<cdiv(channels, kFinCh), 256, 0, s>>>(a);
    if (int rc = check_launch("bn_finalize_kernel")) return rc;
    bn_apply_bf16_kernel<<<stream_blocks(pixels * (channels / 8), channels / 8), 256, 0, s>>>(a, t);
    return check_launch("bn_apply_bf16_kernel");
}

extern "C" int sgv3d_batchnorm_train_backward_bf16(long long pixels, int channels, const void *x, const void *y, const void *dy,
                                                   const float *gamma, const float *save_mean, const float *save_invstd, int relu,
                                                   void *dx, void *dresidual, float *dgamma, float *dbeta, void *workspace,
                                                   size_t workspace_bytes, void *stream) {
    SGV3D_REQUIRE(!relu || y, "batchnorm_train_backward_bf16: the forward output is needed for the ReLU mask");
    return bn_backward16(pixels, channels, x, y, dy, gamma, nullptr, save_mean, save_invstd, relu ? 1 : 0, dx, dresidual, dgamma, dbeta,
                         workspace, workspace_bytes, stream);
}

extern "C" int sgv3d_batchnorm_relu_train_backward_from_x_bf16(long long pixels, int channels, const void *x, const void *dy,
                                                               const float *gamma, const float *beta, const float *save_mean,
                                                               const float *save_invstd, void *dx, float *dgamma, float *dbeta,
                                                               void *workspace, size_t workspace_bytes, void *stream) {
    return bn_backward16(pixels, channels, x, nullptr, dy, gamma, beta, save_mean, save_invstd, 2, dx, nullptr, dgamma, dbeta, workspace,
                         workspace_bytes, stream);
}
