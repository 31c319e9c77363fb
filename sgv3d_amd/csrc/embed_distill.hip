// Distillation of SAM's image embedding into the camera backbone's 1/16 feature map: the embedding warp of the reference's
// dataset (transform_with_M_bilinear, dataset/nusc_mv_det_dataset.py:351-385) and `F.mse_loss(gt_embeds, assist) * weight`
// (exps/bevheight/dair-v2x/bev_height_lss_r50_864_1536_128x128.py:247-256) with its gradient, without leaving the device.
//
//   sgv3d_embed_warp              one launch: the warped teacher, materialised (users who store warped targets, the tests).
//   sgv3d_embed_warp_host         the same arithmetic over host pointers, through the same per-pixel functions.
//   sgv3d_embed_distill_forward   two launches.  The warped teacher is formed per pixel and never written; d = s - t and d * d
//                                 in float32, widened to float64 for the sum; one partial per workgroup over a fixed grid, then a
//                                 one-workgroup finish that adds the partials in a fixed order.
//   sgv3d_embed_distill_backward  one launch: recomputes the warp and writes every element of the gradient view once.
//
// Work is dealt in runs of kPix consecutive pixels per wave.  The position arithmetic (two float64 divisions, the dead test,
// the four blend weights) is per pixel, not per channel: lane i of the wave does it for pixel i of the run, and the lanes that
// own the pixel's channel quads fetch it with a lane shuffle.  At C = 256 a wave's 64 lanes are the 64 quads of one pixel.
// Teacher, NHWC student and gradient move as 16-byte accesses; a student that is not channel-contiguous (plain NCHW) is read
// and written four scalars per lane through its strides.
//
// No float atomics, a fixed summation order, nothing waits on the host, the upstream factor is read on the device: value and
// gradient repeat bit for bit and forward + backward capture into a hipGraph.  Built with -ffp-contract=off: the warp restates
// numpy float64 expressions one rounding at a time, on host and device alike.
#include <algorithm>
#include <cmath>

#include "common.hpp"

using namespace sgv3d;

#define HD __host__ __device__ inline

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / kWave;
constexpr int kPix = 8;               // pixels per wave run
constexpr int kMaxBlocks = 1024;      // workgroups of the partial pass (four per CU)

enum { kCopy = 0, kLive = 1, kDead = 2 };

// Where output pixel (x, y) of a warped frame reads: rows r0, r0 + 1 and columns c0, c0 + 1 with the four weights, or dead.
struct Pos {
    int mode, r0, c0;
    double ax0, ax1, ay0, ay1;
};

// transform_with_M_bilinear for one pixel, m = inv(M) row-major.  The reference clips u, v to [0, w - 2] x [0, h - 2] and zeroes
// the pixels whose unclipped position lies outside: a pixel that survives was not moved by the clip, so the clip is not
// restated.  A position that is not a number is dead as well (the reference's integer cast of it is undefined).
HD Pos embed_position(const double *m, int x, int y, int h, int w) {
    const double X = 10.0 * (double)x, Y = 10.0 * (double)y, Z = 10.0;
    const double a = (m[0] * X + m[1] * Y) + m[2] * Z;
    const double b = (m[3] * X + m[4] * Y) + m[5] * Z;
    const double c = (m[6] * X + m[7] * Y) + m[8] * Z;
    const double u = a / c, v = b / c;
    Pos p;
    p.mode = kDead; p.r0 = 0; p.c0 = 0; p.ax0 = p.ax1 = p.ay0 = p.ay1 = 0.0;
    if (!(u >= 0.0 && u <= (double)(w - 2) && v >= 0.0 && v <= (double)(h - 2))) return p;
    const double fc = floor(u), fr = floor(v);
    p.mode = kLive;
    p.c0 = (int)fc;
    p.r0 = (int)fr;
    p.ax0 = (fc + 1.0) - u;
    p.ax1 = u - fc;
    p.ay0 = (fr + 1.0) - v;
    p.ay1 = v - fr;
    return p;
}

HD float embed_blend(double ax0, double ax1, double ay0, double ay1, float i00, float i01, float i10, float i11) {
    const double f1 = ax0 * (double)i00 + ax1 * (double)i01;
    const double f2 = ax0 * (double)i10 + ax1 * (double)i11;
    return (float)(ay0 * f1 + ay1 * f2);
}

struct EmbedArgs {
    const float *teacher;        // [B, h, w, C]
    const double *minv;          // [B][9] or null (no frame is warped)
    const unsigned char *warped; // [B] or null
    const float *student;        // element (b, c, p) at b*sb + c*sc + p*sp
    float *grad;                 // same addressing (backward)
    float *out;                  // [B, h, w, C] (warp)
    unsigned char *dead;         // [B, h, w] or null (warp)
    const float *upstream;       // [1] or null (= 1)
    long long sb, sc, sp;
    int batch, h, w, channels, mask_dead, blocks;
    double weight;
    double *partial;             // [kMaxBlocks] sums, then [kMaxBlocks] counts (unsigned long long)
    double *saved;               // [2]: N, 2 weight / N
    float *loss;                 // [1]
};

// The run of kPix pixels starting at pixel `first`: lane i < kPix holds pixel first + i.
struct Run {
    int mode;
    long long toff;              // teacher element offset of the pixel (copy) or of I00 (live)
    long long soff;              // student element offset of the pixel's channel 0
    double ax0, ax1, ay0, ay1;
};

__device__ __forceinline__ Run run_position(const EmbedArgs &a, long long first, long long total_px, int lane) {
    Run r;
    r.mode = kDead; r.toff = 0; r.soff = 0; r.ax0 = r.ax1 = r.ay0 = r.ay1 = 0.0;
    const long long g = first + lane;
    if (lane < kPix && g < total_px) {
        const int hw = a.h * a.w;
        const long long b = g / hw;
        const int p = (int)(g - b * hw);
        const int y = p / a.w, x = p - y * a.w;
        r.soff = b * a.sb + (long long)p * a.sp;
        const bool warp = a.minv && a.warped && a.warped[b] != 0;
        if (!warp) {
            r.mode = kCopy;
            r.toff = g * a.channels;
        } else {
            const Pos q = embed_position(a.minv + b * 9, x, y, a.h, a.w);
            r.mode = q.mode;
            r.toff = ((b * a.h + q.r0) * a.w + q.c0) * a.channels;
            r.ax0 = q.ax0; r.ax1 = q.ax1; r.ay0 = q.ay0; r.ay1 = q.ay1;
        }
    }
    return r;
}

// The run's pixel j as seen by the lane that owns one of its channel quads.  Every lane of the wave must call this.
__device__ __forceinline__ Run run_fetch(const Run &r, int j) {
    Run o;
    o.mode = __shfl(r.mode, j, kWave);
    o.toff = __shfl(r.toff, j, kWave);
    o.soff = __shfl(r.soff, j, kWave);
    o.ax0 = __shfl(r.ax0, j, kWave);
    o.ax1 = __shfl(r.ax1, j, kWave);
    o.ay0 = __shfl(r.ay0, j, kWave);
    o.ay1 = __shfl(r.ay1, j, kWave);
    return o;
}

// The warped teacher's channel quad q of the fetched pixel.
__device__ __forceinline__ float4 teacher_quad(const EmbedArgs &a, const Run &r, int q) {
    if (r.mode == kDead) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float *t = a.teacher + r.toff + 4 * q;
    const float4 i00 = *reinterpret_cast<const float4 *>(t);
    if (r.mode == kCopy) return i00;
    const long long row = (long long)a.w * a.channels;
    const float4 i01 = *reinterpret_cast<const float4 *>(t + a.channels);
    const float4 i10 = *reinterpret_cast<const float4 *>(t + row);
    const float4 i11 = *reinterpret_cast<const float4 *>(t + row + a.channels);
    return make_float4(embed_blend(r.ax0, r.ax1, r.ay0, r.ay1, i00.x, i01.x, i10.x, i11.x),
                       embed_blend(r.ax0, r.ax1, r.ay0, r.ay1, i00.y, i01.y, i10.y, i11.y),
                       embed_blend(r.ax0, r.ax1, r.ay0, r.ay1, i00.z, i01.z, i10.z, i11.z),
                       embed_blend(r.ax0, r.ax1, r.ay0, r.ay1, i00.w, i01.w, i10.w, i11.w));
}

template <bool VEC>
__device__ __forceinline__ float4 student_quad(const EmbedArgs &a, const Run &r, int q) {
    if (VEC) return *reinterpret_cast<const float4 *>(a.student + r.soff + 4 * q);
    const float *s = a.student + r.soff + (long long)(4 * q) * a.sc;
    return make_float4(s[0], s[a.sc], s[2 * a.sc], s[3 * a.sc]);
}

// ---------------------------------------------------------------------------------------------- the materialising warp
__global__ void __launch_bounds__(kT) embed_warp_kernel(EmbedArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int Q = a.channels >> 2;
    const long long total_px = (long long)a.batch * a.h * a.w;
    const long long runs = (total_px + kPix - 1) / kPix;
    const long long n_waves = (long long)gridDim.x * kWaves;
    for (long long wb = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); wb < runs; wb += n_waves) {
        const long long first = wb * kPix;
        const Run mine = run_position(a, first, total_px, lane);
        if (a.dead && lane < kPix && first + lane < total_px) a.dead[first + lane] = mine.mode == kDead ? 1 : 0;
        const int items = (total_px - first < kPix ? (int)(total_px - first) : kPix) * Q;
        for (int base = 0; base < items; base += kWave) {
            const int it = base + lane;
            const bool on = it < items;
            const int j = on ? it / Q : 0, q = it - j * Q;
            const Run r = run_fetch(mine, j);
            if (on) *reinterpret_cast<float4 *>(a.out + (first + j) * a.channels + 4 * q) = teacher_quad(a, r, q);
        }
    }
}

// ---------------------------------------------------------------------------------------------- loss: partial sums
template <bool VEC>
__global__ void __launch_bounds__(kT) embed_distill_partial_kernel(EmbedArgs a) {
    __shared__ double lds_s[kWaves];
    __shared__ unsigned long long lds_n[kWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int Q = a.channels >> 2;
    const long long total_px = (long long)a.batch * a.h * a.w;
    const long long runs = (total_px + kPix - 1) / kPix;
    const long long n_waves = (long long)gridDim.x * kWaves;
    double acc = 0.0;
    unsigned long long cnt = 0;          // channel quads that count
    for (long long wb = (long long)blockIdx.x * kWaves + wave; wb < runs; wb += n_waves) {
        const long long first = wb * kPix;
        const Run mine = run_position(a, first, total_px, lane);
        const int items = (total_px - first < kPix ? (int)(total_px - first) : kPix) * Q;
        for (int base = 0; base < items; base += kWave) {
            const int it = base + lane;
            const bool on = it < items;
            const int j = on ? it / Q : 0, q = it - j * Q;
            const Run r = run_fetch(mine, j);
            if (on && !(a.mask_dead && r.mode == kDead)) {
                const float4 t = teacher_quad(a, r, q);
                const float4 s = student_quad<VEC>(a, r, q);
                const float d0 = s.x - t.x, d1 = s.y - t.y, d2 = s.z - t.z, d3 = s.w - t.w;
                acc += (double)(d0 * d0);
                acc += (double)(d1 * d1);
                acc += (double)(d2 * d2);
                acc += (double)(d3 * d3);
                cnt += 1;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, kWave);
        cnt += __shfl_xor(cnt, o, kWave);
    }
    if (lane == 0) { lds_s[wave] = acc; lds_n[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        unsigned long long n = 0;
        for (int i = 0; i < kWaves; ++i) { s += lds_s[i]; n += lds_n[i]; }
        a.partial[blockIdx.x] = s;
        reinterpret_cast<unsigned long long *>(a.partial + kMaxBlocks)[blockIdx.x] = n;
    }
}

// One workgroup: thread i adds partials 4 i .. 4 i + 3 in index order, the wave adds its threads' values in a butterfly, thread 0
// adds the waves in wave order.  The order depends on nothing but the number of partials.
__global__ void __launch_bounds__(kT) embed_distill_finish_kernel(EmbedArgs a) {
    __shared__ double lds_s[kWaves];
    __shared__ unsigned long long lds_n[kWaves];
    static_assert(kMaxBlocks == 4 * kT, "one thread per four partials");
    const unsigned long long *counts = reinterpret_cast<const unsigned long long *>(a.partial + kMaxBlocks);
    double s = 0.0;
    unsigned long long n = 0;
    for (int k = 0; k < 4; ++k) {
        const int i = 4 * (int)threadIdx.x + k;
        if (i < a.blocks) { s += a.partial[i]; n += counts[i]; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, kWave);
        n += __shfl_xor(n, o, kWave);
    }
    if ((threadIdx.x & 63) == 0) { lds_s[threadIdx.x >> 6] = s; lds_n[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        unsigned long long quads = 0;
        for (int i = 0; i < kWaves; ++i) { tot += lds_s[i]; quads += lds_n[i]; }
        const double N = 4.0 * (double)quads;
        a.saved[0] = N;
        a.saved[1] = quads ? 2.0 * a.weight / N : 0.0;
        a.loss[0] = quads ? (float)(a.weight * tot / N) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------- gradient
template <bool VEC>
__global__ void __launch_bounds__(kT) embed_distill_backward_kernel(EmbedArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int Q = a.channels >> 2;
    const long long total_px = (long long)a.batch * a.h * a.w;
    const long long runs = (total_px + kPix - 1) / kPix;
    const long long n_waves = (long long)gridDim.x * kWaves;
    const double k = a.saved[1];
    const float up = a.upstream ? a.upstream[0] : 1.f;
    for (long long wb = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); wb < runs; wb += n_waves) {
        const long long first = wb * kPix;
        const Run mine = run_position(a, first, total_px, lane);
        const int items = (total_px - first < kPix ? (int)(total_px - first) : kPix) * Q;
        for (int base = 0; base < items; base += kWave) {
            const int it = base + lane;
            const bool on = it < items;
            const int j = on ? it / Q : 0, q = it - j * Q;
            const Run r = run_fetch(mine, j);
            if (!on) continue;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!(a.mask_dead && r.mode == kDead)) {
                const float4 t = teacher_quad(a, r, q);
                const float4 s = student_quad<VEC>(a, r, q);
                g.x = (float)(k * (double)(s.x - t.x)) * up;
                g.y = (float)(k * (double)(s.y - t.y)) * up;
                g.z = (float)(k * (double)(s.z - t.z)) * up;
                g.w = (float)(k * (double)(s.w - t.w)) * up;
            }
            if (VEC) {
                *reinterpret_cast<float4 *>(a.grad + r.soff + 4 * q) = g;
            } else {
                float *o = a.grad + r.soff + (long long)(4 * q) * a.sc;
                o[0] = g.x; o[a.sc] = g.y; o[2 * a.sc] = g.z; o[3 * a.sc] = g.w;
            }
        }
    }
}

int check_map(const char *who, int batch, int h, int w, int channels, const float *teacher) {
    SGV3D_REQUIRE(batch > 0 && channels > 0, "%s: bad sizes", who);
    SGV3D_REQUIRE(h >= 2 && w >= 2, "%s: the map must be at least 2 x 2", who);
    SGV3D_REQUIRE(channels % 4 == 0, "%s: channels must be a multiple of 4", who);
    SGV3D_REQUIRE(teacher, "%s: null pointer", who);
    return SGV3D_OK;
}

int fill_distill(EmbedArgs &a, const char *who, int batch, int channels, int h, int w, const float *student, long long sb,
                 long long sc, long long sp, const float *teacher, const double *minv, const unsigned char *warped, int mask_dead) {
    if (int rc = check_map(who, batch, h, w, channels, teacher)) return rc;
    SGV3D_REQUIRE(student, "%s: null pointer", who);
    SGV3D_REQUIRE((minv == nullptr) == (warped == nullptr), "%s: minv and warped go together", who);
    SGV3D_REQUIRE(sb >= 0 && sc >= 1 && sp >= 1, "%s: bad strides", who);
    SGV3D_REQUIRE(aligned16(teacher), "%s: teacher must be 16-byte aligned", who);
    a.teacher = teacher; a.minv = minv; a.warped = warped; a.student = student;
    a.sb = sb; a.sc = sc; a.sp = sp;
    a.batch = batch; a.h = h; a.w = w; a.channels = channels; a.mask_dead = mask_dead ? 1 : 0;
    return SGV3D_OK;
}

// 16-byte accesses to a view: channel-contiguous, every pixel's quad aligned
bool view_is_vector(const void *p, long long sb, long long sc, long long sp) {
    return sc == 1 && sp % 4 == 0 && sb % 4 == 0 && aligned16(p);
}

long long runs_of(const EmbedArgs &a) { return ((long long)a.batch * a.h * a.w + kPix - 1) / kPix; }

}  // namespace

extern "C" int sgv3d_embed_warp(int batch, int h, int w, int channels, const float *teacher, const double *minv,
                                const uint8_t *warped, float *out, uint8_t *dead, void *stream) {
    if (int rc = check_map("embed_warp", batch, h, w, channels, teacher)) return rc;
    SGV3D_REQUIRE(minv && warped && out, "embed_warp: null pointer");
    SGV3D_REQUIRE(aligned16(teacher) && aligned16(out), "embed_warp: teacher and out must be 16-byte aligned");
    SGV3D_REQUIRE(out + (long long)batch * h * w * channels <= teacher || teacher + (long long)batch * h * w * channels <= out,
                  "embed_warp: out overlaps teacher");
    EmbedArgs a{};
    a.teacher = teacher; a.minv = minv; a.warped = warped; a.out = out; a.dead = dead;
    a.batch = batch; a.h = h; a.w = w; a.channels = channels;
    const int grid = (int)std::min<long long>(4 * kMaxBlocks, (runs_of(a) + kWaves - 1) / kWaves);
    embed_warp_kernel<<<grid, kT, 0, as_stream(stream)>>>(a);
    return check_launch("embed_warp_kernel");
}

extern "C" int sgv3d_embed_warp_host(int batch, int h, int w, int channels, const float *teacher, const double *minv,
                                     const uint8_t *warped, float *out, uint8_t *dead) {
    if (int rc = check_map("embed_warp_host", batch, h, w, channels, teacher)) return rc;
    SGV3D_REQUIRE(minv && warped && out, "embed_warp_host: null pointer");
    SGV3D_REQUIRE(out + (long long)batch * h * w * channels <= teacher || teacher + (long long)batch * h * w * channels <= out,
                  "embed_warp_host: out overlaps teacher");
    const long long C = channels, row = (long long)w * C;
    for (int b = 0; b < batch; ++b)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const long long px = ((long long)b * h + y) * w + x;
                float *o = out + px * C;
                if (!warped[b]) {
                    for (int c = 0; c < channels; ++c) o[c] = teacher[px * C + c];
                    if (dead) dead[px] = 0;
                    continue;
                }
                const Pos p = embed_position(minv + (long long)b * 9, x, y, h, w);
                if (dead) dead[px] = p.mode == kDead ? 1 : 0;
                if (p.mode == kDead) {
                    for (int c = 0; c < channels; ++c) o[c] = 0.f;
                    continue;
                }
                const float *t = teacher + (((long long)b * h + p.r0) * w + p.c0) * C;
                for (int c = 0; c < channels; ++c)
                    o[c] = embed_blend(p.ax0, p.ax1, p.ay0, p.ay1, t[c], t[C + c], t[row + c], t[row + C + c]);
            }
    return SGV3D_OK;
}

extern "C" size_t sgv3d_embed_distill_workspace_bytes(void) { return (size_t)kMaxBlocks * (sizeof(double) + sizeof(unsigned long long)); }

extern "C" int sgv3d_embed_distill_forward(int batch, int channels, int h, int w, const float *student, long long batch_stride,
                                           long long channel_stride, long long pixel_stride, const float *teacher,
                                           const double *minv, const uint8_t *warped, double weight, int mask_dead,
                                           float *loss_out, double *saved, void *workspace, size_t workspace_bytes, void *stream) {
    EmbedArgs a{};
    if (int rc = fill_distill(a, "embed_distill_forward", batch, channels, h, w, student, batch_stride, channel_stride,
                              pixel_stride, teacher, minv, warped, mask_dead))
        return rc;
    SGV3D_REQUIRE(loss_out && saved && workspace, "embed_distill_forward: null pointer");
    SGV3D_REQUIRE(std::isfinite(weight), "embed_distill_forward: weight must be finite");
    SGV3D_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(saved) & 7) == 0,
                  "embed_distill_forward: workspace and saved must be 8-byte aligned");
    if (workspace_bytes < sgv3d_embed_distill_workspace_bytes())
        return fail(SGV3D_ENOSPACE, "embed_distill_forward: workspace too small (%zu bytes, %zu needed)", workspace_bytes,
                    sgv3d_embed_distill_workspace_bytes());
    a.weight = weight; a.loss = loss_out; a.saved = saved; a.partial = static_cast<double *>(workspace);
    a.blocks = (int)std::min<long long>(kMaxBlocks, (runs_of(a) + kWaves - 1) / kWaves);
    hipStream_t s = as_stream(stream);
    if (view_is_vector(student, batch_stride, channel_stride, pixel_stride))
        embed_distill_partial_kernel<true><<<a.blocks, kT, 0, s>>>(a);
    else
        embed_distill_partial_kernel<false><<<a.blocks, kT, 0, s>>>(a);
    if (int rc = check_launch("embed_distill_partial_kernel")) return rc;
    embed_distill_finish_kernel<<<1, kT, 0, s>>>(a);
    return check_launch("embed_distill_finish_kernel");
}

extern "C" int sgv3d_embed_distill_backward(int batch, int channels, int h, int w, const float *student, long long batch_stride,
                                            long long channel_stride, long long pixel_stride, const float *teacher,
                                            const double *minv, const uint8_t *warped, int mask_dead, const double *saved,
                                            const float *upstream, float *grad, void *stream) {
    EmbedArgs a{};
    if (int rc = fill_distill(a, "embed_distill_backward", batch, channels, h, w, student, batch_stride, channel_stride,
                              pixel_stride, teacher, minv, warped, mask_dead))
        return rc;
    SGV3D_REQUIRE(saved && grad, "embed_distill_backward: null pointer");
    // the gradient view spans [grad, grad + span); the teacher is read while it is written
    const long long span = (long long)(batch - 1) * batch_stride + (long long)(channels - 1) * channel_stride +
                           ((long long)h * w - 1) * pixel_stride + 1;
    const float *t_end = teacher + (long long)batch * h * w * channels;
    SGV3D_REQUIRE(grad + span <= teacher || t_end <= grad, "embed_distill_backward: grad overlaps teacher");
    a.saved = const_cast<double *>(saved); a.upstream = upstream; a.grad = grad;
    const int grid = (int)std::min<long long>(4 * kMaxBlocks, (runs_of(a) + kWaves - 1) / kWaves);
    hipStream_t s = as_stream(stream);
    if (view_is_vector(student, batch_stride, channel_stride, pixel_stride) &&
        view_is_vector(grad, batch_stride, channel_stride, pixel_stride))
        embed_distill_backward_kernel<true><<<grid, kT, 0, s>>>(a);
    else
        embed_distill_backward_kernel<false><<<grid, kT, 0, s>>>(a);
    return check_launch("embed_distill_backward_kernel");
}
