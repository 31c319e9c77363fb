// Weight gradient of the deformable 3x3 convolution (mmcv 1.4.0 DeformConv2dPack / DCNv1 as configured at
// layers/backbones/lss_fpn.py:190-198; forward: dcn_fused_bf16.hip) with the SAMPLES RECOMPUTED, on the bf16 matrix cores
// (mixed-precision training: f32 tensors, bf16 operands, f32 accumulation):
//
//   dW[g opg + co][ci][r][s] = sum over pixels p of  bf16(dY[p][g opg + co]) * bf16(sample(x, p, tap = 3 r + s, g cpg + ci))
//
// The column form of the training step keeps the sampled column tensor [B, H, W, 9 C] (f32) from the forward for this product
// (95 MB per frame at 54 x 96 x 512) and copies it once more per group.  Here nothing of that size exists: the sample is formed
// from x and the offsets on the way into LDS, bit for bit as dcn3x3_fused_bf16_kernel forms it for f32 x (the same fmaf chain,
// this file is built with -ffp-contract=off, one rounding to bf16) -- which is bit for bit the column tensor of
// sgv3d_deform_im2col3x3 rounded to bf16.
//
//   workgroup   256 threads = 4 waves; owns one (group, tap) and a 128 (co) x 128 (ci) accumulator tile -- the whole (group, tap)
//               matrix at the layer's 128 x 128 per group -- and walks a range of pixels, 32 per step.  A wave owns 64 x 64: 2 x 2
//               accumulators of v_mfma_f32_32x32x16_bf16 (64 VGPRs); blocks of 32 rows / columns beyond opg / cpg are skipped.
//   operands    the reduction index is the PIXEL, the slow axis of both operands in memory.  The LDS images stay pixel-major --
//               per 64-channel half [32 pixels][64 channels] bf16, 128 B per pixel, filled with 16-byte stores of 8 rounded
//               channels -- and are read with ds_read_b64_tr_b16 (a 4-pixel x 16-channel block per 16 lanes, delivered
//               channel-major), as conv_wgrad3x3_bf16.hip does; the same half-row swap on bit 1 of the pixel index keeps the four
//               rows of a block on four bank quarters.
//   staging     thread (pixel = tid / 8, 8-channel chunk = tid % 8 of both halves) derives the tap's four corner offsets and
//               bilinear weights ONCE per step (the tap is fixed per workgroup) and uses them for 16 samples: 16 16-byte buffer
//               loads of x, 4 of dY.  Corners outside the image, samples outside it, rows past B H W, channels beyond cpg / opg:
//               an offset past the buffer's range, the load returns zeros.  The loads of step j + 1 (and the offsets of
//               step j + 2) are in flight under the MFMAs of step j; the images are double-buffered, one barrier per step.
//   split       the pixel axis is cut into `split` ranges of whole steps, chosen from the shape alone (at most 512 workgroups, two
//               per CU; at least 128 pixels per range).  Partial tiles go to the workspace [range][group][tap][co][ci];
//               dcn_wgrad_reduce_kernel adds them in range order and writes OIHW.  Every sum has a fixed order: two calls give
//               the same bits.
//
// Bound: 2 * 9 * P * cout * cpg flop is microseconds on the matrix pipe (8 MFMAs per wave and step); the step's cost is the
// gather -- 20 KiB of corner rows through the vector-memory path -- and ~150 vector-ALU instructions per thread of sampling
// arithmetic.  Measured numbers: DESIGN 14.
#include "common.hpp"

using namespace sgv3d;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int kP = 32;                       // pixels per step (two k-steps of 16)
constexpr int kRowB = 128;                   // bytes per pixel row of a half image (64 channels bf16)
constexpr int kHalfB = kP * kRowB;           // 4096
constexpr int kStageB = 4 * kHalfB;          // dY half 0, dY half 1, samples half 0, samples half 1
constexpr int kTile = 128;                   // co and ci per workgroup
constexpr int kMaxGroups = 8;
constexpr int kTargetWgs = 512;              // two resident workgroups per CU
constexpr int kMinRange = 128;               // pixels per range the rule keeps
constexpr unsigned kOutside = 0x80000000u;   // buffer offset past every tensor this entry accepts (< 2 GiB), also after + 16 + a channel offset

struct DgArgs {
    const float *x, *off, *dy;
    float *ws, *dw;
    int H, W, C, cpg, opg, groups, cout;
    int M;                                   // B * H * W
    int off_ld;
    int tiles_co, tiles_ci;
    int split, per;                          // pixel ranges and pixels per range (a multiple of kP)
    unsigned x_bytes, y_bytes;
};

__device__ __forceinline__ unsigned img_off(int row, int bytecol) { return (unsigned)(row * kRowB + (bytecol ^ (((row >> 1) & 1) << 6))); }

__device__ __forceinline__ bf16x8 tr_read8(const unsigned char *lds, unsigned off) {
    // rows (pixels) k .. k + 3 and k + 4 .. k + 7 of this lane's channel: two transposed reads of 4 x 16 blocks
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(lds + off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(lds + off + 4 * kRowB));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

__global__ __launch_bounds__(256, 2) void dcn_wgrad_bf16_kernel(const DgArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kStageB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // blockIdx.x -> (group, tap, co tile, ci tile); blockIdx.y = pixel range
    int it = blockIdx.x;
    const int tci = it % a.tiles_ci; it /= a.tiles_ci;
    const int tco = it % a.tiles_co; it /= a.tiles_co;
    const int tap = it % 9;
    const int grp = it / 9;
    const int co0 = tco * kTile, ci0 = tci * kTile;
    const int p0 = blockIdx.y * a.per;
    const int pend = min(p0 + a.per, a.M);
    const int nsteps = (pend - p0 + kP - 1) / kP;
    const int ky = tap / 3, kx = tap - ky * 3;

    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t y_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.dy, 0, (int)a.y_bytes, 0x00020000);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][n][e] = 0.f;

    // ---- staging: a thread owns pixel sp of the step and the 8-channel chunk sc of both 64-channel halves
    const int sp = tid >> 3, sc = (tid & 7) * 8;
    unsigned dy_c[2][2];                         // byte offset of (half, 4-channel piece) inside a pixel of dY, or kOutside
    unsigned x_c[2];                             // byte offset of this thread's 8 channels of a half inside a pixel of x, or kOutside
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int co = co0 + h * 64 + sc, ci = ci0 + h * 64 + sc;
        dy_c[h][0] = co < a.opg ? (unsigned)(grp * a.opg + co) * 4u : kOutside;
        dy_c[h][1] = co + 4 < a.opg ? (unsigned)(grp * a.opg + co + 4) * 4u : kOutside;
        x_c[h] = ci < a.cpg ? (unsigned)(grp * a.cpg + ci) * 4u : kOutside;
    }
    const unsigned st_off = img_off(sp, sc * 2);

    float noy = 0.f, nox = 0.f;                  // offsets (dy, dx) of this tap at the pixel of the next step to request
    float cw[4];
    f32x4 rdy[2][2], rx[2][4][2];

    auto fetch_off = [&](int j) {
        const int m = p0 + j * kP + sp;
        const bool ok = j < nsteps && m < a.M;
        const float *o = a.off + (size_t)(ok ? m : 0) * a.off_ld + 2 * tap;
        noy = ok ? o[0] : 0.f;
        nox = ok ? o[1] : 0.f;
    };
    // requests dY and the four corners of step j (its offsets are in noy / nox)
    auto issue = [&](int j) {
        const int m = p0 + j * kP + sp;
        const bool pok = m < a.M;
        const unsigned mm = pok ? (unsigned)m : 0u;
        const unsigned t2 = mm / (unsigned)a.W;
        const int pw = (int)(mm - t2 * (unsigned)a.W);
        const unsigned b = t2 / (unsigned)a.H;
        const int ph = (int)(t2 - b * (unsigned)a.H);
        const unsigned ybase = mm * (unsigned)a.cout * 4u;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                rdy[h][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                          y_rsrc, (pok && dy_c[h][i] != kOutside) ? ybase + dy_c[h][i] : kOutside, 0, 0));
        // the sample's position, corners and weights: dcn3x3_fused_bf16_kernel's tap_params, operation by operation
        const float hf = (float)(ph - 1 + ky) + noy;
        const float wf = (float)(pw - 1 + kx) + nox;
        const bool in = pok && hf > -1.f && wf > -1.f && hf < (float)a.H && wf < (float)a.W;
        const int hl = (int)floorf(hf), wl = (int)floorf(wf);
        const int hh = hl + 1, wh = wl + 1;
        const float lh = hf - (float)hl, lw = wf - (float)wl;
        const float uh = 1.f - lh, uw = 1.f - lw;
        const bool k1 = in && hl >= 0 && wl >= 0, k2 = in && hl >= 0 && wh <= a.W - 1;
        const bool k3 = in && hh <= a.H - 1 && wl >= 0, k4 = in && hh <= a.H - 1 && wh <= a.W - 1;
        cw[0] = k1 ? uh * uw : 0.f; cw[1] = k2 ? uh * lw : 0.f;
        cw[2] = k3 ? lh * uw : 0.f; cw[3] = k4 ? lh * lw : 0.f;
        const unsigned cb = (unsigned)a.C * 4u;
        const unsigned pbase = b * (unsigned)(a.H * a.W) * cb;
        unsigned co[4];
        co[0] = k1 ? pbase + (unsigned)(hl * a.W + wl) * cb : kOutside;
        co[1] = k2 ? pbase + (unsigned)(hl * a.W + wh) * cb : kOutside;
        co[2] = k3 ? pbase + (unsigned)(hh * a.W + wl) * cb : kOutside;
        co[3] = k4 ? pbase + (unsigned)(hh * a.W + wh) * cb : kOutside;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned o = (co[k] != kOutside && x_c[h] != kOutside) ? co[k] + x_c[h] : kOutside;
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    rx[h][k][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, o + 16u * i, 0, 0));
            }
    };
    // bilinear combination in f32 (the contracted chain of the im2col kernels, see dcn_fused_bf16.hip), one rounding to bf16;
    // dY rounded once; 16-byte stores into stage `buf`
    auto commit = [&](int buf) {
        unsigned char *const st = lds + buf * kStageB;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x8 d = __builtin_shufflevector(rdy[h][0], rdy[h][1], 0, 1, 2, 3, 4, 5, 6, 7);
            *reinterpret_cast<bf16x8 *>(st + h * kHalfB + st_off) = __builtin_convertvector(d, bf16x8);
            bf16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v1 = rx[h][0][e >> 2][e & 3], v2 = rx[h][1][e >> 2][e & 3];
                const float v3 = rx[h][2][e >> 2][e & 3], v4 = rx[h][3][e >> 2][e & 3];
                float s = cw[1] * v2;
                s = __builtin_fmaf(cw[0], v1, s);
                s = __builtin_fmaf(cw[2], v3, s);
                s = __builtin_fmaf(cw[3], v4, s);
                v[e] = (__bf16)s;
            }
            *reinterpret_cast<bf16x8 *>(st + (2 + h) * kHalfB + st_off) = v;
        }
    };

    // ---- fragment addresses (ds_read_b64_tr_b16: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p + 3 of the block)
    const int fq = (lane & 15) >> 2, fp = lane & 3;
    const int frow = fq + 8 * (lane >> 5);                               // k = 8 (lane / 32) + q (+ 4 for the second read)
    const int fcol = 16 * ((lane >> 4) & 1) + 4 * fp;                    // channel within a block of 32
    unsigned f_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) f_off[i] = img_off(frow, (32 * i + fcol) * 2);
    // blocks of 32 output / input channels of this wave that exist (wave-uniform)
    bool live_a[2], live_b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        live_a[i] = co0 + wm * 64 + 32 * i < a.opg;
        live_b[i] = ci0 + wn * 64 + 32 * i < a.cpg;
    }

    fetch_off(0);
    issue(0);
    fetch_off(1);
    commit(0);
    __syncthreads();
    for (int j = 0; j < nsteps; ++j) {
        const bool have_next = j + 1 < nsteps;
        if (have_next) {
            issue(j + 1);
            fetch_off(j + 2);
        }
        __builtin_amdgcn_sched_barrier(0);
        const unsigned char *const dyi = lds + (j & 1) * kStageB + wm * kHalfB;
        const unsigned char *const xi = lds + (j & 1) * kStageB + (2 + wn) * kHalfB;
#pragma unroll
        for (int ks = 0; ks < kP / 16; ++ks) {
            bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = tr_read8(dyi, f_off[i] + ks * 16 * kRowB);
                fb[i] = tr_read8(xi, f_off[i] + ks * 16 * kRowB);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    if (live_a[i] && live_b[n]) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[n], acc[i][n], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (have_next) commit((j + 1) & 1);
        __syncthreads();
    }

    // partial tile -> workspace [range][group][tap][co][ci]
    float *const ws = a.ws + (((size_t)blockIdx.y * a.groups + grp) * 9 + tap) * (size_t)a.opg * a.cpg;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int ci = ci0 + wn * 64 + 32 * n + (lane & 31);
        if (ci >= a.cpg) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int co = co0 + wm * 64 + 32 * i + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
                if (co < a.opg) ws[(size_t)co * a.cpg + ci] = acc[i][n][e];
            }
    }
}

// dw[g opg + co][ci][tap] = sum over the ranges (in order) of ws[range][g][tap][co][ci]
__global__ __launch_bounds__(256) void dcn_wgrad_reduce_kernel(const DgArgs a) {
    const long long total = 9ll * a.cout * a.cpg;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float *ws = a.ws + i;
    float v = 0.f;
    int p = 0;
    for (; p + 8 <= a.split; p += 8) {                      // eight independent loads in flight, added in order
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = ws[(size_t)(p + k) * total];
#pragma unroll
        for (int k = 0; k < 8; ++k) v += t[k];
    }
    for (; p < a.split; ++p) v += ws[(size_t)p * total];
    const int ci = (int)(i % a.cpg);
    long long r = i / a.cpg;
    const int co = (int)(r % a.opg); r /= a.opg;
    const int tap = (int)(r % 9);
    const int g = (int)(r / 9);
    a.dw[((size_t)(g * a.opg + co) * a.cpg + ci) * 9 + tap] = v;
}

// geometry, limits and the split; nothing here touches the device
int fill(const char *who, int batch, int h, int w, int channels, int groups, int out_per_group, int split, DgArgs &a) {
    SGV3D_REQUIRE(batch > 0 && h > 0 && w > 0 && channels > 0 && groups > 0 && out_per_group > 0 && split >= 0, "%s: bad sizes", who);
    SGV3D_REQUIRE(groups <= kMaxGroups && channels % groups == 0 && (channels / groups) % 32 == 0 && out_per_group % 4 == 0,
                  "%s: groups <= %d, channels %% groups == 0, channels per group %% 32, outputs per group %% 4 (cpg=%d opg=%d groups=%d)",
                  who, kMaxGroups, channels / groups, out_per_group, groups);
    const long long M = (long long)batch * h * w;
    const long long cout = (long long)groups * out_per_group;
    SGV3D_REQUIRE(M < 0x7fffffffLL && M * channels * 4 < 0x7fffff00LL && M * cout * 4 < 0x7fffff00LL,
                  "%s: x and dy must be smaller than 2 GiB (32-bit buffer offsets)", who);
    a = DgArgs{};
    a.H = h; a.W = w; a.C = channels; a.cpg = channels / groups; a.opg = out_per_group; a.groups = groups; a.cout = (int)cout;
    a.M = (int)M;
    a.tiles_co = cdiv(a.opg, kTile); a.tiles_ci = cdiv(a.cpg, kTile);
    const int steps = cdiv(M, kP);
    int s = split;
    if (s <= 0) {
        const int tiles = groups * 9 * a.tiles_co * a.tiles_ci;
        const int by_pixels = (int)(M / kMinRange);
        s = kTargetWgs / tiles;
        s = s > by_pixels ? by_pixels : s;
    }
    s = s < 1 ? 1 : (s > steps ? steps : s);
    a.per = cdiv(steps, s) * kP;
    a.split = cdiv(M, a.per);
    SGV3D_REQUIRE(a.split <= 65535, "%s: too many pixel ranges (%d)", who, a.split);
    a.x_bytes = (unsigned)(M * channels * 4);
    a.y_bytes = (unsigned)(M * cout * 4);
    return SGV3D_OK;
}

size_t ws_bytes(const DgArgs &a) { return (size_t)a.split * 9 * a.cout * a.cpg * sizeof(float); }

}  // namespace

extern "C" size_t sgv3d_deform_conv3x3_backward_weight_bf16_workspace_bytes(int batch, int h, int w, int channels, int groups,
                                                                            int out_per_group, int split) {
    DgArgs a;
    if (fill("deform_conv3x3_backward_weight_bf16_workspace_bytes", batch, h, w, channels, groups, out_per_group, split, a) != SGV3D_OK)
        return 0;
    return ws_bytes(a);
}

extern "C" int sgv3d_deform_conv3x3_backward_weight_bf16(int batch, int h, int w, int channels, int groups, int out_per_group,
                                                         const float *x, const float *offset, int off_ld, const float *dy, float *dw,
                                                         int split, void *workspace, size_t workspace_bytes, void *stream) {
    const char *const who = "deform_conv3x3_backward_weight_bf16";
    DgArgs a;
    if (int rc = fill(who, batch, h, w, channels, groups, out_per_group, split, a)) return rc;
    SGV3D_REQUIRE(off_ld >= 18, "%s: off_ld %d < 18", who, off_ld);
    SGV3D_REQUIRE(x && offset && dy && dw && workspace, "%s: null pointer", who);
    SGV3D_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(offset) | reinterpret_cast<uintptr_t>(dw)) & 3) == 0,
                  "%s: x, dy and the workspace must be 16-byte aligned, offset and dw 4-byte aligned", who);
    if (workspace_bytes < ws_bytes(a))
        return fail(SGV3D_ENOSPACE, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, ws_bytes(a));
    a.x = x; a.off = offset; a.dy = dy; a.dw = dw; a.ws = static_cast<float *>(workspace);
    a.off_ld = off_ld;
    hipStream_t st = as_stream(stream);
    dcn_wgrad_bf16_kernel<<<dim3(groups * 9 * a.tiles_co * a.tiles_ci, a.split), 256, 0, st>>>(a);
    if (int rc = check_launch("dcn_wgrad_bf16_kernel")) return rc;
    dcn_wgrad_reduce_kernel<<<dim3((unsigned)cdiv(9ll * a.cout * a.cpg, 256)), 256, 0, st>>>(a);
    return check_launch("dcn_wgrad_reduce_kernel");
}
