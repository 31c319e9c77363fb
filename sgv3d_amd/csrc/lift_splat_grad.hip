// Adjoint of the fused lift-splat (layers/backbones/lss_fpn.py:462-466,486 + ops/voxel_pooling/voxel_pooling.py:58-69)
// without the [B, D*P, C] lifted tensor or its gradient:
//
//   grad_prob[b, d, p]    = sum_c  context[b, p, c] * G[b, v(b, d, p), c]      (0 where the point is not kept)
//   grad_context[b, p, c] = sum_d  prob[b, d, p]    * G[b, v(b, d, p), c]      (kept d only)
//
// v(b, d, p) is the voxel of point d*P + p, kept iff 0 <= x < X, 0 <= y < Y, 0 <= z < Z (the reference kernel's test; z is
// only bounds-checked).  The adjoint of the scatter is a BALANCED gather: every pixel owns exactly D rows of G, so there is
// no sort, no plan and no atomic.
//
// lsg_kernel<G, K>: a group of G lanes owns one pixel (64 / G pixels per wave, one wave per workgroup so that the ~1 300
// waves of cfg-2 batch 2 spread evenly over the CUs).  Lane j of the group holds the float4 columns j, j + G, ... of the
// context row and of the grad_context accumulator in registers (K columns per lane, K * G >= C / 4), so one load instruction
// of the group reads G * 16 contiguous bytes of a G row.  The D points are walked in rounds of G: lane j reads the geometry
// and the probability of point d0 + j once, the group shares them by lane shuffles, and the rows of U points are in flight
// together.  The G per-point dot products of a round are reduced across the group by a transposing butterfly (G - 1
// shuffles for G sums instead of G * log2 G) that leaves the sum of point d0 + j in lane j, which stores it.
// Both sums have a fixed order: ascending d for grad_context, a fixed tree for grad_prob -- bitwise repeatable.
//
// One launch, no workspace traffic.  Splitting D over 2 or 4 grid slices (partial context rows through the workspace, added in
// slice order by a second kernel) was measured and dropped: 40.3 / 42.4 / 38.4 us at cfg-2 batch 2 (10 368 pixels, 1 296
// waves) and 206 / 212 / 218 us at cfg-5 for 1 / 2 / 4 slices -- a round of 8 points issues 24 row loads per lane (196 VGPRs at C = 80),
// which hides the Infinity-Cache latency without more waves.  The workspace argument is reserved (16 bytes).
#include "common.hpp"

using namespace sgv3d;

namespace {

struct LsgArgs {
    const int32_t *geom;
    const float *prob;
    const float *ctx;
    const float *gout;
    float *gprob;
    float *gctx;
    long long sb, sy, sx;
    long long total;    // B * P
    int D, P, C4, X, Y, Z;
};

template <int G>
__device__ __forceinline__ int group_bcast(int v, int base, int j) {
    if constexpr (G == 1) return v;
    return __shfl(v, base + j, 64);
}
template <int G>
__device__ __forceinline__ float group_bcast(float v, int base, int j) {
    if constexpr (G == 1) return v;
    return __shfl(v, base + j, 64);
}

template <int G, int K, bool WP, bool WC>
__global__ __launch_bounds__(64) void lsg_kernel(const LsgArgs a) {
    constexpr int U = G < 4 ? G : 4;                 // points whose rows are in flight together
    const int lane = threadIdx.x;
    const int j = lane & (G - 1);
    const int base = lane & ~(G - 1);
    const long long gid = (long long)blockIdx.x * (64 / G) + lane / G;
    const bool valid = gid < a.total;
    const int b = valid ? (int)(gid / a.P) : 0;
    const int p = valid ? (int)(gid - (long long)b * a.P) : 0;

    bool in[K];
    float4 ctx[K], acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        in[k] = j + k * G < a.C4;
        ctx[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (WP && valid && in[k]) ctx[k] = reinterpret_cast<const float4 *>(a.ctx)[gid * a.C4 + j + k * G];
    }
    const float4 *grow = reinterpret_cast<const float4 *>(a.gout + (long long)b * a.sb) + j;
    const long long pt0 = (long long)b * a.D * a.P + p;       // point (b, d = 0, p)

    for (int d0 = 0; d0 < a.D; d0 += G) {
        // lane j: voxel (as the float4 offset of its G row inside the sample) and probability of point d0 + j
        const int dj = d0 + j;
        const bool mine = valid && dj < a.D;
        int v = -1;
        float pr = 0.f;
        if (mine) {
            const long long pt = pt0 + (long long)dj * a.P;
            const int32_t *gp = a.geom + pt * 3;
            const int x = gp[0], y = gp[1], z = gp[2];
            if ((unsigned)x < (unsigned)a.X && (unsigned)y < (unsigned)a.Y && (unsigned)z < (unsigned)a.Z) {
                v = (int)((y * a.sy + x * a.sx) >> 2);
                if (WC) pr = a.prob[pt];
            }
        }
        float s[G];
#pragma unroll
        for (int u0 = 0; u0 < G; u0 += U) {
            float4 g[U][K];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int vu = group_bcast<G>(v, base, u0 + u);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    g[u][k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (vu >= 0 && in[k]) g[u][k] = grow[(long long)vu + k * G];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (WC) {
                    const float pu = group_bcast<G>(pr, base, u0 + u);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        acc[k].x = fmaf(pu, g[u][k].x, acc[k].x);
                        acc[k].y = fmaf(pu, g[u][k].y, acc[k].y);
                        acc[k].z = fmaf(pu, g[u][k].z, acc[k].z);
                        acc[k].w = fmaf(pu, g[u][k].w, acc[k].w);
                    }
                }
                if (WP) {
                    float t = 0.f;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        t = fmaf(ctx[k].x, g[u][k].x, t);
                        t = fmaf(ctx[k].y, g[u][k].y, t);
                        t = fmaf(ctx[k].z, g[u][k].z, t);
                        t = fmaf(ctx[k].w, g[u][k].w, t);
                    }
                    s[u0 + u] = t;
                }
            }
        }
        if (WP) {
            // transposing butterfly: after the step of width h a lane keeps the half of the sums its bit h selects
#pragma unroll
            for (int h = G / 2; h >= 1; h >>= 1) {
                const bool upper = (lane & h) != 0;
#pragma unroll
                for (int i = 0; i < h; ++i) {
                    const float send = upper ? s[i] : s[i + h];
                    const float keep = upper ? s[i + h] : s[i];
                    s[i] = keep + __shfl_xor(send, h, 64);
                }
            }
            if (mine) a.gprob[pt0 + (long long)dj * a.P] = v >= 0 ? s[0] : 0.f;
        }
    }
    if (WC && valid) {
        float4 *o = reinterpret_cast<float4 *>(a.gctx) + gid * a.C4 + j;
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (in[k]) o[k * G] = acc[k];
    }
}

// lanes per pixel and float4 columns per lane for C / 4 columns: K <= 4
void lsg_shape(int C4, int &G, int &K) {
    G = C4 <= 1 ? 1 : C4 <= 2 ? 2 : C4 <= 4 ? 4 : C4 <= 32 ? 8 : 16;
    K = (C4 + G - 1) / G;
}

template <int G, int K>
void lsg_launch(const LsgArgs &a, dim3 grid, hipStream_t st) {
    if (a.gprob && a.gctx)
        hipLaunchKernelGGL((lsg_kernel<G, K, true, true>), grid, dim3(64), 0, st, a);
    else if (a.gprob)
        hipLaunchKernelGGL((lsg_kernel<G, K, true, false>), grid, dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((lsg_kernel<G, K, false, true>), grid, dim3(64), 0, st, a);
}

}  // namespace

extern "C" size_t sgv3d_lift_splat_backward_workspace_bytes(int batch_size, int num_depth, int num_pixels, int num_channels) {
    if (batch_size <= 0 || num_depth <= 0 || num_pixels <= 0 || num_channels <= 0 || num_channels % 4 || num_channels > 256) {
        fail(SGV3D_EINVAL, "lift_splat_backward_workspace_bytes: needs positive sizes, C %% 4 == 0, C <= 256 (B=%d D=%d P=%d C=%d)",
             batch_size, num_depth, num_pixels, num_channels);
        return 0;
    }
    return 16;      // reserved: the kernel stages nothing (see the note on splitting D above)
}

extern "C" int sgv3d_lift_splat_backward(int batch_size, int num_depth, int num_pixels, int num_channels, int num_voxel_x,
                                         int num_voxel_y, int num_voxel_z, const int32_t *geom_xyz, const float *prob,
                                         const float *context, const float *grad_output, long long sb, long long sy,
                                         long long sx, float *grad_prob, float *grad_context, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    const int B = batch_size, D = num_depth, P = num_pixels, C = num_channels;
    SGV3D_REQUIRE(B > 0 && D > 0 && P > 0 && C > 0 && num_voxel_x > 0 && num_voxel_y > 0 && num_voxel_z > 0,
                  "lift_splat_backward: non-positive size (B=%d D=%d P=%d C=%d X=%d Y=%d Z=%d)", B, D, P, C, num_voxel_x,
                  num_voxel_y, num_voxel_z);
    SGV3D_REQUIRE(C % 4 == 0 && C <= 256, "lift_splat_backward: needs C %% 4 == 0, 4 <= C <= 256 (got %d)", C);
    SGV3D_REQUIRE((long long)B * P < 0x7fffffffLL, "lift_splat_backward: B*P=%lld pixel groups do not fit one grid dimension",
                  (long long)B * P);
    SGV3D_REQUIRE(geom_xyz && prob && context && grad_output, "lift_splat_backward: null pointer");
    SGV3D_REQUIRE((reinterpret_cast<uintptr_t>(grad_output) & 15) == 0 && sb % 4 == 0 && sy % 4 == 0 && sx % 4 == 0,
                  "lift_splat_backward: grad_output rows must be 16-B aligned (pointer and sb, sy, sx multiples of 4 floats)");
    SGV3D_REQUIRE((reinterpret_cast<uintptr_t>(context) & 15) == 0 && (reinterpret_cast<uintptr_t>(grad_context) & 15) == 0,
                  "lift_splat_backward: context / grad_context rows must be 16-B aligned");
    // a row's float4 offset inside its sample travels as one non-negative int32
    SGV3D_REQUIRE(sy >= 0 && sx >= 0 && ((num_voxel_y - 1) * sy + (num_voxel_x - 1) * sx) / 4 + C / 4 < 0x7fffffffLL,
                  "lift_splat_backward: sy, sx must be non-negative and a sample's map smaller than 2^31 float4");
    const size_t need = sgv3d_lift_splat_backward_workspace_bytes(B, D, P, C);
    SGV3D_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
                  "lift_splat_backward: workspace has %zu bytes, needs %zu (16-B aligned)", workspace ? workspace_bytes : (size_t)0, need);
    if (!grad_prob && !grad_context) return SGV3D_OK;

    LsgArgs a;
    a.geom = geom_xyz; a.prob = prob; a.ctx = context; a.gout = grad_output;
    a.gprob = grad_prob; a.gctx = grad_context;
    a.sb = sb; a.sy = sy; a.sx = sx;
    a.total = (long long)B * P;
    a.D = D; a.P = P; a.C4 = C / 4; a.X = num_voxel_x; a.Y = num_voxel_y; a.Z = num_voxel_z;
    int G, K;
    lsg_shape(a.C4, G, K);
    const dim3 grid((unsigned)((a.total + 64 / G - 1) / (64 / G)));
    const hipStream_t st = as_stream(stream);
    switch (G * 8 + K) {
        case 1 * 8 + 1: lsg_launch<1, 1>(a, grid, st); break;
        case 2 * 8 + 1: lsg_launch<2, 1>(a, grid, st); break;
        case 4 * 8 + 1: lsg_launch<4, 1>(a, grid, st); break;
        case 8 * 8 + 1: lsg_launch<8, 1>(a, grid, st); break;
        case 8 * 8 + 2: lsg_launch<8, 2>(a, grid, st); break;
        case 8 * 8 + 3: lsg_launch<8, 3>(a, grid, st); break;
        case 8 * 8 + 4: lsg_launch<8, 4>(a, grid, st); break;
        case 16 * 8 + 3: lsg_launch<16, 3>(a, grid, st); break;
        case 16 * 8 + 4: lsg_launch<16, 4>(a, grid, st); break;
        default: return fail(SGV3D_EINVAL, "lift_splat_backward: no kernel for C=%d", C);
    }
    return check_launch("lsg_kernel");
}
