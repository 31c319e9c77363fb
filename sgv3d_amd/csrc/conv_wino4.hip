// Winograd F(4x4, 3x3) for gfx950 in three launches -- the form for layers with MANY channels on SMALL maps (HeightNet's ten
// 512 -> 512 convolutions at 54x96, ResNet layer 3 / 4, the 640-channel BEV trunk stage): 3x3 / stride 1 / pad 1 convolutions
// the reference runs through cuDNN (layers/backbones/lss_fpn.py:161-250 and the mmdet ResNet blocks it builds).
//
//   Y = A^T [ sum_ci (G g G^T) (.) (B^T d B) ] A     per 4x4 output tile (6x6 input tile, 36 positions)
//
// executes 36 / 16 / 9 = 1/4 of the direct form's multiplications, against 1/2.25 for the F(2x2) kernels of conv_wino.hip.
// With 36 positions the accumulators of a fused kernel no longer fit a wave (36 x 16 registers), so the three stages are
// separate launches and the middle one -- all of the matrix work -- is the f32 MFMA implicit-GEMM kernel itself, run as a
// GROUPED GEMM over the positions (conv_gemm_grouped, conv_igemm.hip):
//
//   1. wino4_input_kernel    x NHWC -> V[36][tiles_pad][cin]          (B^T d B; one thread per tile and 4 channels)
//   2. conv_gemm_grouped     M[p] = V[p] . U[p]^T, p = 0..35          (U[p][cout][cin] = (G g G^T)[p], packed per position;
//                                                                       SGV3D_TILE_48x64: conv_gemm_grouped16, gemm16_grouped.hip)
//   3. wino4_output_kernel   M[36][tiles_pad][cout] -> y NHWC         (A^T M A, folded BN / bias, residual, ReLU)
//
// V and M (28 MB each for a 512-channel 54x96 layer) are written once and read once; they stay in the 256 MB last-level
// cache between the launches.  The transforms are HBM / L2-bound streaming kernels (bound: HBM, 4 (1 + 2.25) bytes per input
// element and 4 (2.25 + 1 [+ 1]) per output element); the GEMM is bound by the f32 MFMA rate.  Pays where cin and cout are
// large (the transforms cost O(pixels x channels), the GEMM O(pixels x cin x cout)): the first-call measurement of hip_ops
// decides per layer.  fp32 rounding: the transformed operands are up to 100x the inputs (|B^T| row sums 10), so the error of an
// output is ~1e-5 of its scale against ~1e-6 for F(2x2); tests/test_conv_wino_gpu.py bounds it against float64.
#include "conv_common.hpp"
#include "f32x3.hpp"

using namespace sgv3d;

namespace {

struct f4 {
    float x, y, z, w;
};
__device__ __forceinline__ f4 ld4(const float *p) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    return {v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ void st4(float *p, const f4 &v) { *reinterpret_cast<float4 *>(p) = make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ f4 fma4(float s, const f4 &a, const f4 &b) {   // s * a + b
    return {fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z), fmaf(s, a.w, b.w)};
}
__device__ __forceinline__ f4 add4(const f4 &a, const f4 &b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
__device__ __forceinline__ f4 sub4(const f4 &a, const f4 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w}; }

// B^T (6 -> 6), 12 operations:
//   t0 = 4 d0 - 5 d2 + d4          t1 = (d4 - 4 d2) + (d3 - 4 d1)     t2 = (d4 - 4 d2) - (d3 - 4 d1)
//   t3 = (d4 - d2) + 2 (d3 - d1)   t4 = (d4 - d2) - 2 (d3 - d1)       t5 = 4 d1 - 5 d3 + d5
__device__ __forceinline__ void wino4_bt(f4 &d0, f4 &d1, f4 &d2, f4 &d3, f4 &d4, f4 &d5) {
    const f4 a = fma4(-4.f, d2, d4), b = fma4(-4.f, d1, d3);
    const f4 c = sub4(d4, d2), e = sub4(d3, d1);
    const f4 t0 = fma4(4.f, d0, fma4(-5.f, d2, d4));
    const f4 t5 = fma4(4.f, d1, fma4(-5.f, d3, d5));
    d0 = t0;
    d1 = add4(a, b);
    d2 = sub4(a, b);
    d3 = fma4(2.f, e, c);
    d4 = fma4(-2.f, e, c);
    d5 = t5;
}

// A^T (6 -> 4), 10 operations:
//   y0 = m0 + (m1 + m2) + (m3 + m4)        y1 = (m1 - m2) + 2 (m3 - m4)
//   y2 = (m1 + m2) + 4 (m3 + m4)           y3 = (m1 - m2) + 8 (m3 - m4) + m5
__device__ __forceinline__ void wino4_at(const f4 &m0, const f4 &m1, const f4 &m2, const f4 &m3, const f4 &m4, const f4 &m5,
                                         f4 &y0, f4 &y1, f4 &y2, f4 &y3) {
    const f4 p = add4(m1, m2), q = sub4(m1, m2), r = add4(m3, m4), s = sub4(m3, m4);
    y0 = add4(add4(m0, p), r);
    y1 = fma4(2.f, s, q);
    y2 = fma4(4.f, r, p);
    y3 = add4(fma4(8.f, s, q), m5);
}

// Threads per workgroup of the transform kernels (single-wave workgroups -- 672 instead of 168 for a 512-channel 54x96 layer --
// measured the same in round 6: the transforms are bound by the latency of their 36 dependent-free loads and 36-108 stores per
// thread, not by how the waves spread over the CUs).
constexpr int kTB = 256;

// One axis of the tile lattice of a dilated layer.  A 3x3 with pad == dil is dil independent convolutions per axis, on the
// sub-grids p, p + dil, p + 2 dil, ... (phase p = 0 .. dil - 1).  Two ways to cut an axis of n pixels into 4-element tiles:
//   split    every phase has its own tiles: dil * ceil(ceil(n / dil) / 4) of them, the last tile of every phase mostly padding;
//   stacked  the phases stand one after another on ONE line with a single zero element between neighbours and that line is cut:
//            ceil((n + dil - 1) / 4) tiles.  A 3x3 reaches +-1 element, so the separator (or the end of the line) is exactly the
//            zero padding the first / last element of a sub-grid sees, and a tile may hold elements of two or more phases.
// The host takes the form with fewer tiles (split on a tie: dil == 1 is always split, and both forms are then the same map).
struct Wino4Axis {
    int n, dil;
    int tiles;             // tiles of the axis (all phases)
    int per_phase;         // split: tiles of one phase; 0: stacked
};

__host__ __device__ inline Wino4Axis wino4_axis(int n, int dil) {
    const int split = dil * (((n + dil - 1) / dil + 3) / 4), stacked = (n + dil - 1 + 3) / 4;
    Wino4Axis a;
    a.n = n;
    a.dil = dil;
    a.tiles = stacked < split ? stacked : split;
    a.per_phase = stacked < split ? 0 : split / dil;
    return a;
}

// The lattice's index map: pix[k] = the pixel coordinate of element 4 t + k0 + k of tile t's line (k0 = -1, N = 6: the inputs of
// the tile; k0 = 0, N = 4: its outputs), or -1 for a separator and for anything outside the image -- read as zero, never stored.
// Stacked: phases [0, r) have q + 1 elements and the others q (n = q dil + r), each followed by one separator, so the first
// element decodes with one division and the following ones by stepping (a phase with no elements is its separator alone).
template <int N>
__host__ __device__ __forceinline__ void wino4_axis_pixels(const Wino4Axis &ax, int t, int k0, int (&pix)[N]) {
    if (ax.per_phase) {
        const int p = t / ax.per_phase, e0 = 4 * (t - p * ax.per_phase) + k0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int e = e0 + k, c = p + e * ax.dil;
            pix[k] = (e >= 0 && c < ax.n) ? c : -1;
        }
        return;
    }
    const int q = ax.n / ax.dil, r = ax.n - q * ax.dil, head = r * (q + 2);
    const int v = 4 * t + k0;
    int p = -1, i = 0, len = 0;           // v == -1: in front of the line; the step below then enters phase 0
    if (v >= 0) {
        if (v < head) {
            p = v / (q + 2);
            i = v - p * (q + 2);
        } else {
            const int u = (v - head) / (q + 1);
            p = r + u;
            i = v - head - u * (q + 1);
        }
        len = q + (p < r ? 1 : 0);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        pix[k] = ((unsigned)p < (unsigned)ax.dil && i < len) ? p + i * ax.dil : -1;
        if (++i > len) {
            ++p;
            i = 0;
            len = q + (p < r ? 1 : 0);
        }
    }
}

// What the transform kernels decode with.  kDilated false (dil == 1): the plain map, tile t = pixels 4 t + k0 ..., which is what
// wino4_axis_pixels gives at dil 1 -- compiled on its own so that the non-dilated layers (57 of a cfg-2 frame's 60 launches) run
// the code they ran before there was a lattice: the divisions and branches of the general decode sit in front of a latency-bound
// kernel's first load and cost it 0.2 - 0.4 us per launch.
template <bool kDilated, int N>
__device__ __forceinline__ void wino4_pixels(const Wino4Axis &ax, int t, int k0, int (&pix)[N]) {
    if constexpr (kDilated) {
        wino4_axis_pixels(ax, t, k0, pix);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const int c = 4 * t + k0 + k;
            pix[k] = (unsigned)c < (unsigned)ax.n ? c : -1;
        }
    }
}

struct Wino4Args {
    const float *x, *scale, *bias, *res;
    float *v, *m, *y;
    int batch, h, w, cin, cout, x_ld, x_coff, y_ld, y_coff, res_ld, relu;
    Wino4Axis ay, ax;      // the tile lattice of the rows and of the columns: ay.tiles x ax.tiles tiles per image
    int rows;              // rows of V / M per position (tiles of all images, padded to a multiple of the GEMM's m-tile)
    int c0, cn;            // output-channel chunk [c0, c0 + cn) this pass of the GEMM / output transform covers (M holds cn columns)
    int gw;                // 0: NHWC output; > 0 (GROUP_PLANES): y is [cout / gw][pixels][gw], one NHWC map per group of gw channels
};

// tile index -> (image, tile of the row lattice, tile of the column lattice)
__device__ __forceinline__ void wino4_tile(const Wino4Args &a, int t, int &b, int &ty, int &tx) {
    const int per_img = a.ay.tiles * a.ax.tiles;
    b = t / per_img;
    const int r = t - b * per_img;
    ty = r / a.ax.tiles;
    tx = r - ty * a.ax.tiles;
}

// one thread: one tile x 4 input channels.  Consecutive threads = consecutive channel quads: 16-byte accesses, contiguous.
template <bool kDilated>
__global__ __launch_bounds__(kTB) void wino4_input_kernel(const Wino4Args a) {
    const int cq = a.cin >> 2;
    const long long i = (long long)blockIdx.x * kTB + threadIdx.x;
    const long long ntile = (long long)a.batch * a.ay.tiles * a.ax.tiles;
    if (i >= ntile * cq) return;
    const int t = (int)(i / cq), c = (int)(i - (long long)t * cq) * 4;
    int b, ty, tx;
    wino4_tile(a, t, b, ty, tx);
    int yy[6], xx[6];
    wino4_pixels<kDilated>(a.ay, ty, -1, yy);
    wino4_pixels<kDilated>(a.ax, tx, -1, xx);
    const float *xb = a.x + (size_t)b * a.h * a.w * a.x_ld + a.x_coff + c;
    f4 d[6][6];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
#pragma unroll
        for (int cc = 0; cc < 6; ++cc)
            d[rr][cc] = (yy[rr] >= 0 && xx[cc] >= 0) ? ld4(xb + ((size_t)yy[rr] * a.w + xx[cc]) * a.x_ld) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) wino4_bt(d[0][cc], d[1][cc], d[2][cc], d[3][cc], d[4][cc], d[5][cc]);     // B^T d
    float *vb = a.v + (size_t)t * a.cin + c;
    const size_t plane = (size_t)a.rows * a.cin;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
        wino4_bt(d[rr][0], d[rr][1], d[rr][2], d[rr][3], d[rr][4], d[rr][5]);                                 // (B^T d) B
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) st4(vb + (size_t)(rr * 6 + cc) * plane, d[rr][cc]);
    }
}

// one thread: one tile x 4 output channels
template <bool kDilated>
__device__ __forceinline__ void wino4_output_body(const Wino4Args &a, const long long i) {     // i: (tile, channel quad) of the layer
    const int cq = a.cn >> 2;
    const long long ntile = (long long)a.batch * a.ay.tiles * a.ax.tiles;
    if (i >= ntile * cq) return;
    const int t = (int)(i / cq), cl = (int)(i - (long long)t * cq) * 4;     // cl: column inside the chunk
    const int c = a.c0 + cl;                                                // output channel
    int b, ty, tx;
    wino4_tile(a, t, b, ty, tx);
    const float *mb = a.m + (size_t)t * a.cn + cl;
    const size_t plane = (size_t)a.rows * a.cn;
    f4 rr_[4][6];                                           // A^T M: 4 x 6
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) {
        const f4 m0 = ld4(mb + (size_t)(0 * 6 + cc) * plane), m1 = ld4(mb + (size_t)(1 * 6 + cc) * plane),
                 m2 = ld4(mb + (size_t)(2 * 6 + cc) * plane), m3 = ld4(mb + (size_t)(3 * 6 + cc) * plane),
                 m4 = ld4(mb + (size_t)(4 * 6 + cc) * plane), m5 = ld4(mb + (size_t)(5 * 6 + cc) * plane);
        wino4_at(m0, m1, m2, m3, m4, m5, rr_[0][cc], rr_[1][cc], rr_[2][cc], rr_[3][cc]);
    }
    int yy[4], xx[4];                                       // (decoded behind the 36 loads, not in front of them)
    wino4_pixels<kDilated>(a.ay, ty, 0, yy);
    wino4_pixels<kDilated>(a.ax, tx, 0, xx);
    const f4 sc = a.scale ? ld4(a.scale + c) : f4{1.f, 1.f, 1.f, 1.f};
    const f4 sh = a.bias ? ld4(a.bias + c) : f4{0.f, 0.f, 0.f, 0.f};
    const float floor_ = a.relu ? 0.f : -__builtin_inff();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        f4 o[4];
        wino4_at(rr_[u][0], rr_[u][1], rr_[u][2], rr_[u][3], rr_[u][4], rr_[u][5], o[0], o[1], o[2], o[3]);   // (A^T M) A
        if (yy[u] < 0) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (xx[v] < 0) continue;
            const size_t pix = ((size_t)b * a.h + yy[u]) * a.w + xx[v];
            f4 q = {fmaf(o[v].x, sc.x, sh.x), fmaf(o[v].y, sc.y, sh.y), fmaf(o[v].z, sc.z, sh.z), fmaf(o[v].w, sc.w, sh.w)};
            if (a.res) q = add4(q, ld4(a.res + pix * a.res_ld + c));
            q = {fmaxf(q.x, floor_), fmaxf(q.y, floor_), fmaxf(q.z, floor_), fmaxf(q.w, floor_)};
            if (a.gw > 0) {            // plane of the channel's group (gw % 4 == 0: a quad never straddles groups)
                const int grp = c / a.gw;
                st4(a.y + ((size_t)grp * a.batch * a.h * a.w + pix) * a.gw + (c - grp * a.gw), q);
            } else {
                st4(a.y + pix * a.y_ld + a.y_coff + c, q);
            }
        }
    }
}

template <bool kDilated>
__global__ __launch_bounds__(kTB) void wino4_output_kernel(const Wino4Args a) {
    wino4_output_body<kDilated>(a, (long long)blockIdx.x * kTB + threadIdx.x);
}

// Up to four sibling layers on ONE input (ASPP's dilated branches) in one launch of a transform: the workgroups of layer l are
// [first[l], first[l + 1]) -- a workgroup never straddles layers -- and each runs the single-layer body on its layer's arguments,
// element for element the arithmetic of the separate launches.
constexpr int kWino4Multi = 4;
struct Wino4MultiArgs {
    Wino4Args a[kWino4Multi];
    int first[kWino4Multi + 1];
    int n;
};

__device__ __forceinline__ int wino4_multi_layer(const Wino4MultiArgs &m) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < kWino4Multi; ++k) l += (k < m.n && (int)blockIdx.x >= m.first[k]) ? 1 : 0;
    return l;
}

__global__ __launch_bounds__(kTB) void wino4_output_multi_kernel(const Wino4MultiArgs m) {
    const int l = wino4_multi_layer(m);
    wino4_output_body<true>(m.a[l], (long long)((int)blockIdx.x - m.first[l]) * kTB + threadIdx.x);
}

// U[p][co][ci] = (G g G^T)[i][j], p = 6 i + j, written straight into the 36 packed weight blocks [cout_pad][k_pad] of the
// grouped GEMM (k = ci: a 1x1 weight in either k order), zero rows / columns in the padding.  One thread per (co, ci).
//   G = [[1/4, 0, 0], [-1/6, -1/6, -1/6], [-1/6, 1/6, -1/6], [1/24, 1/12, 1/6], [1/24, -1/12, 1/6], [0, 0, 1]]
__global__ __launch_bounds__(256) void wino4_pack_weight_kernel(const float *__restrict__ w, int cout, int cin, int k_pad,
                                                                int cout_pad, float *__restrict__ u) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)cout_pad * k_pad) return;
    const int co = (int)(i / k_pad), ci = (int)(i - (long long)co * k_pad);
    float g[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (co < cout && ci < cin) {
        const float *p = w + ((size_t)co * cin + ci) * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = p[a * 3 + b];
    }
    // G g: 6 x 3 (rows of G applied to the columns of g), then (G g) G^T: 6 x 6
    float t[6][3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float s02 = g[0][b] + g[2][b];
        t[0][b] = 0.25f * g[0][b];
        t[1][b] = (-1.f / 6.f) * (s02 + g[1][b]);
        t[2][b] = (-1.f / 6.f) * (s02 - g[1][b]);
        t[3][b] = (1.f / 24.f) * g[0][b] + (1.f / 12.f) * g[1][b] + (1.f / 6.f) * g[2][b];
        t[4][b] = (1.f / 24.f) * g[0][b] - (1.f / 12.f) * g[1][b] + (1.f / 6.f) * g[2][b];
        t[5][b] = g[2][b];
    }
    const size_t block = (size_t)cout_pad * k_pad;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const float s02 = t[r][0] + t[r][2];
        const float o[6] = {0.25f * t[r][0], (-1.f / 6.f) * (s02 + t[r][1]), (-1.f / 6.f) * (s02 - t[r][1]),
                            (1.f / 24.f) * t[r][0] + (1.f / 12.f) * t[r][1] + (1.f / 6.f) * t[r][2],
                            (1.f / 24.f) * t[r][0] - (1.f / 12.f) * t[r][1] + (1.f / 6.f) * t[r][2], t[r][2]};
#pragma unroll
        for (int c = 0; c < 6; ++c) u[(size_t)(r * 6 + c) * block + i] = o[c];
    }
}

// ---- f32x3 forms (f32x3.hpp): the operands of the position GEMMs as three bf16 planes -------------------------------------
__device__ __forceinline__ void split3(const f4 &x, bf16x4 &hi, bf16x4 &mid, bf16x4 &lo) {
    sgv3d::split3(f32x4{x.x, x.y, x.z, x.w}, hi, mid, lo);
}

// as wino4_input_kernel, writing V3 [36][rows][cin/32][3][32] bf16: one thread = one tile x 4 input channels -> three 8-byte
// stores per position (the 8 threads of a 32-channel record fill its three 64-byte planes)
template <bool kDilated>
__device__ __forceinline__ void wino4_input_x3_body(const Wino4Args &a, const long long i) {
    const int cq = a.cin >> 2;
    const long long ntile = (long long)a.batch * a.ay.tiles * a.ax.tiles;
    if (i >= ntile * cq) return;
    const int t = (int)(i / cq), c = (int)(i - (long long)t * cq) * 4;
    int b, ty, tx;
    wino4_tile(a, t, b, ty, tx);
    int yy[6], xx[6];
    wino4_pixels<kDilated>(a.ay, ty, -1, yy);
    wino4_pixels<kDilated>(a.ax, tx, -1, xx);
    const float *xb = a.x + (size_t)b * a.h * a.w * a.x_ld + a.x_coff + c;
    f4 d[6][6];
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
#pragma unroll
        for (int cc = 0; cc < 6; ++cc)
            d[rr][cc] = (yy[rr] >= 0 && xx[cc] >= 0) ? ld4(xb + ((size_t)yy[rr] * a.w + xx[cc]) * a.x_ld) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) wino4_bt(d[0][cc], d[1][cc], d[2][cc], d[3][cc], d[4][cc], d[5][cc]);     // B^T d
    // record (row t, k-chunk c / 32) of position p: bf16 index ((p * rows + t) * (cin / 32) + c / 32) * 96 + plane * 32 + c % 32
    __bf16 *vb = reinterpret_cast<__bf16 *>(a.v) + ((size_t)t * (a.cin >> 5) + (c >> 5)) * 96 + (c & 31);
    const size_t plane = (size_t)a.rows * (a.cin >> 5) * 96;
#pragma unroll
    for (int rr = 0; rr < 6; ++rr) {
        wino4_bt(d[rr][0], d[rr][1], d[rr][2], d[rr][3], d[rr][4], d[rr][5]);                                 // (B^T d) B
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) {
            bf16x4 hi, mid, lo;
            split3(d[rr][cc], hi, mid, lo);
            __bf16 *o = vb + (size_t)(rr * 6 + cc) * plane;
            *reinterpret_cast<bf16x4 *>(o) = hi;
            *reinterpret_cast<bf16x4 *>(o + 32) = mid;
            *reinterpret_cast<bf16x4 *>(o + 64) = lo;
        }
    }
}

template <bool kDilated>
__global__ __launch_bounds__(kTB) void wino4_input_x3_kernel(const Wino4Args a) {
    wino4_input_x3_body<kDilated>(a, (long long)blockIdx.x * kTB + threadIdx.x);
}

__global__ __launch_bounds__(kTB) void wino4_input_x3_multi_kernel(const Wino4MultiArgs m) {
    const int l = wino4_multi_layer(m);
    wino4_input_x3_body<true>(m.a[l], (long long)((int)blockIdx.x - m.first[l]) * kTB + threadIdx.x);
}

// U3[p][co / 16][ci / 32][plane][fragment order] = the three bf16 terms of (G g G^T)[i][j], p = 6 i + j; zero rows / columns in the padding.
// One thread per (co, ci); the arithmetic of wino4_pack_weight_kernel, then the split.
__global__ __launch_bounds__(256) void wino4_pack_weight_x3_kernel(const float *__restrict__ w, int cout, int cin, int k_pad,
                                                                   int cout_pad, __bf16 *__restrict__ u) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)cout_pad * k_pad) return;
    const int co = (int)(i / k_pad), ci = (int)(i - (long long)co * k_pad);
    float g[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    if (co < cout && ci < cin) {
        const float *p = w + ((size_t)co * cin + ci) * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = p[a * 3 + b];
    }
    float t[6][3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float s02 = g[0][b] + g[2][b];
        t[0][b] = 0.25f * g[0][b];
        t[1][b] = (-1.f / 6.f) * (s02 + g[1][b]);
        t[2][b] = (-1.f / 6.f) * (s02 - g[1][b]);
        t[3][b] = (1.f / 24.f) * g[0][b] + (1.f / 12.f) * g[1][b] + (1.f / 6.f) * g[2][b];
        t[4][b] = (1.f / 24.f) * g[0][b] - (1.f / 12.f) * g[1][b] + (1.f / 6.f) * g[2][b];
        t[5][b] = g[2][b];
    }
    const size_t block = (size_t)cout_pad * k_pad * 3;
    __bf16 *ub = u3_at(u, co, ci, k_pad);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const float s02 = t[r][0] + t[r][2];
        const float o[6] = {0.25f * t[r][0], (-1.f / 6.f) * (s02 + t[r][1]), (-1.f / 6.f) * (s02 - t[r][1]),
                            (1.f / 24.f) * t[r][0] + (1.f / 12.f) * t[r][1] + (1.f / 6.f) * t[r][2],
                            (1.f / 24.f) * t[r][0] - (1.f / 12.f) * t[r][1] + (1.f / 6.f) * t[r][2], t[r][2]};
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            __bf16 hi, mid, lo;
            split3_rounded(o[c], hi, mid, lo);
            u3_store(ub + (size_t)(r * 6 + c) * block, hi, mid, lo);
        }
    }
}

// the tile lattice of both axes, the tiles of all images, and the padded row count per position
void wino4_geom(const sgv3d_conv_desc *d, Wino4Axis &ay, Wino4Axis &ax, long long &tiles, int &rows) {
    ay = wino4_axis(d->out_h, d->dil);
    ax = wino4_axis(d->out_w, d->dil);
    tiles = (long long)d->batch * ay.tiles * ax.tiles;
    const int g = (d->tile & SGV3D_TILE_X3) ? gemm_x3_tile_rows(d->tile & 15)
                  : (d->tile & ~SGV3D_TILE_OCC5) == SGV3D_TILE_32x128 ? 32 : d->tile == SGV3D_TILE_48x64 ? 48 : 64;   // the GEMM's m-tile height
    rows = (int)((tiles + g - 1) / g * g);
}

// Output channels per pass: M of a pass (36 x rows x chunk floats) is kept below ~160 MB so that it is still in the 256 MB
// last-level cache when the output transform reads it back -- the 64 -> 2304 first layers of the CenterHead branches at
// 256x256 would otherwise write and re-read 1.36 GB.  Multiples of 128 (the packed weight blocks' row granularity).
int wino4_chunk(const sgv3d_conv_desc *d, int rows) {
    const long long per_channel = 36LL * rows * 4;
    long long cn = (160LL << 20) / per_channel / 128 * 128;
    if (cn < 128) cn = 128;
    return cn >= d->cout ? d->cout : (int)cn;
}

}  // namespace

// w_src: OIHW [cout, cin, 3, 3] f32 (cin may be smaller than the layer's padded channel count: the rest is zero) -> u_packed:
// 36 x cout_pad x k_pad floats, (cout_pad, k_pad) = sgv3d_conv_pack_geometry(cin_pad, cout)
extern "C" int sgv3d_conv_winograd4_pack_weight(const float *w_src, int cout, int cin, int k_pad, int cout_pad, float *u_packed,
                                                void *stream) {
    SGV3D_REQUIRE(w_src && u_packed && cout > 0 && cin > 0 && k_pad >= cin && k_pad % 32 == 0 && cout_pad >= cout,
                  "conv_winograd4_pack_weight: bad arguments (cout=%d cin=%d k_pad=%d cout_pad=%d)", cout, cin, k_pad, cout_pad);
    const long long total = (long long)cout_pad * k_pad;
    hipLaunchKernelGGL(wino4_pack_weight_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), w_src, cout, cin, k_pad,
                       cout_pad, u_packed);
    return check_launch("wino4_pack_weight_kernel");
}

// ... as three bf16 planes per element for the f32x3 position GEMM (desc.tile = SGV3D_TILE_X3 | variant): u3_packed is
// 36 x cout_pad x cin_pad x 3 bf16 (cin_pad % 32 == 0, cout_pad = cout rounded up to 32), layout [p][co][ci / 32][plane][ci % 32]
extern "C" int sgv3d_conv_winograd4_pack_weight_x3(const float *w_src, int cout, int cin, int cin_pad, int cout_pad, void *u3_packed,
                                                   void *stream) {
    SGV3D_REQUIRE(w_src && u3_packed && cout > 0 && cin > 0 && cin_pad >= cin && cin_pad % 32 == 0 && cout_pad >= cout && cout_pad % 32 == 0,
                  "conv_winograd4_pack_weight_x3: bad arguments (cout=%d cin=%d cin_pad=%d cout_pad=%d)", cout, cin, cin_pad, cout_pad);
    const long long total = (long long)cout_pad * cin_pad;
    hipLaunchKernelGGL(wino4_pack_weight_x3_kernel, dim3(cdiv(total, 256)), dim3(256), 0, as_stream(stream), w_src, cout, cin, cin_pad,
                       cout_pad, static_cast<__bf16 *>(u3_packed));
    return check_launch("wino4_pack_weight_x3_kernel");
}

// The tile lattice of one axis on the host (what wino4_geom and the transform kernels use): the tile count, whether the phases are
// stacked, and -- pixels != nullptr -- the pixel coordinate (or -1) of the `count` (1..6) elements from 4 * tile + k0 on.
extern "C" int sgv3d_wino4_lattice_axis(int n, int dil, int tile, int k0, int count, int *tiles, int *stacked, int *pixels) {
    SGV3D_REQUIRE(n > 0 && dil > 0, "wino4_lattice_axis: bad axis (n=%d dil=%d)", n, dil);
    const Wino4Axis ax = wino4_axis(n, dil);
    if (tiles) *tiles = ax.tiles;
    if (stacked) *stacked = ax.per_phase == 0;
    if (pixels) {
        SGV3D_REQUIRE(tile >= 0 && tile < ax.tiles && (k0 == -1 || k0 == 0) && count >= 1 && count <= 6,
                      "wino4_lattice_axis: bad tile / element range (tile=%d k0=%d count=%d)", tile, k0, count);
        int pix[6];
        wino4_axis_pixels(ax, tile, k0, pix);
        for (int k = 0; k < count; ++k) pixels[k] = pix[k];
    }
    return SGV3D_OK;
}

// bytes of V + M
extern "C" size_t sgv3d_conv2d_winograd4_workspace_bytes(const sgv3d_conv_desc *d) {
    if (!d || d->batch <= 0 || d->out_h <= 0 || d->out_w <= 0 || d->cin <= 0 || d->cout <= 0 || d->dil <= 0) return 0;
    Wino4Axis ay, ax;
    int rows;
    long long tiles;
    wino4_geom(d, ay, ax, tiles, rows);
    if (d->tile & SGV3D_TILE_X3)         // V as three bf16 planes (6 bytes per element), M f32
        return 36 * (size_t)rows * (6 * (size_t)d->cin + sizeof(float) * (size_t)wino4_chunk(d, rows));
    return sizeof(float) * 36 * (size_t)rows * ((size_t)d->cin + (size_t)wino4_chunk(d, rows));
}

// u_packed: 36 blocks [cout_pad][k_pad] (sgv3d_conv_pack_geometry(cin, cout)), block p = i * 6 + j the 1x1 weight
// (G g G^T)[i][j] packed by sgv3d_conv_pack_weight.  desc: as for sgv3d_conv2d_winograd_forward (NORMAL mode, no gate, no
// split-K); desc.k_pad / desc.cout_pad describe ONE block; desc.tile: SGV3D_TILE_64x64 (default) or SGV3D_TILE_64x128 for
// the grouped GEMM.
extern "C" int sgv3d_conv2d_winograd4_forward(const sgv3d_conv_desc *d, const float *x, const float *u_packed,
                                              const float *scale, const float *bias, const float *residual, float *y,
                                              void *workspace, size_t workspace_bytes, void *stream) {
    SGV3D_REQUIRE(d && x && u_packed && y && workspace, "conv2d_winograd4_forward: null pointer");
    SGV3D_REQUIRE(d->kh == 3 && d->kw == 3 && d->stride == 1 && d->dil >= 1 && d->pad == d->dil,
                  "conv2d_winograd4_forward: only 3x3 / stride 1 / pad == dilation");
    SGV3D_REQUIRE(d->batch > 0 && d->in_h > 0 && d->in_w > 0 && d->cin > 0 && d->cout > 0 && d->out_h == d->in_h && d->out_w == d->in_w,
                  "conv2d_winograd4_forward: bad sizes");
    const bool planes = d->mode == SGV3D_CONV_GROUP_PLANES;
    SGV3D_REQUIRE(d->mode == SGV3D_CONV_NORMAL || planes, "conv2d_winograd4_forward: NHWC or GROUP_PLANES output only");
    SGV3D_REQUIRE(!planes || (d->deconv_ks > 0 && d->deconv_ks % 4 == 0 && d->cout % d->deconv_ks == 0 && residual == nullptr),
                  "conv2d_winograd4_forward: GROUP_PLANES needs deconv_ks = group width (a multiple of 4) dividing cout, no residual");
    SGV3D_REQUIRE(d->cin % 4 == 0 && d->cout % 4 == 0 && (d->x_ld & 3) == 0 && (d->x_coff & 3) == 0 &&
                      (planes || ((d->y_ld & 3) == 0 && (d->y_coff & 3) == 0)) && (residual == nullptr || (d->res_ld & 3) == 0),
                  "conv2d_winograd4_forward: channel counts, leading dimensions and offsets must be multiples of 4");
    SGV3D_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(residual) |
                    reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(u_packed) |
                    reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
                  "conv2d_winograd4_forward: pointers must be 16-B aligned");
    SGV3D_REQUIRE(d->x_ld >= d->x_coff + d->cin && (planes || d->y_ld >= d->y_coff + d->cout) && (residual == nullptr || d->res_ld >= d->cout),
                  "conv2d_winograd4_forward: leading dimension too small");
    const size_t need = sgv3d_conv2d_winograd4_workspace_bytes(d);
    if (workspace_bytes < need) return fail(SGV3D_ENOSPACE, "conv2d_winograd4_forward: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    Wino4Args a;
    a.x = x; a.scale = scale; a.bias = bias; a.res = residual; a.y = y;
    a.batch = d->batch; a.h = d->in_h; a.w = d->in_w; a.cin = d->cin; a.cout = d->cout;
    a.x_ld = d->x_ld; a.x_coff = d->x_coff; a.y_ld = d->y_ld; a.y_coff = d->y_coff; a.res_ld = d->res_ld; a.relu = d->relu;
    long long tiles;
    wino4_geom(d, a.ay, a.ax, tiles, a.rows);
    SGV3D_REQUIRE(tiles < 0x7fffffffLL / 64, "conv2d_winograd4_forward: too many tiles");
    const bool x3 = (d->tile & SGV3D_TILE_X3) != 0;
    a.v = static_cast<float *>(workspace);
    a.m = x3 ? reinterpret_cast<float *>(static_cast<unsigned char *>(workspace) + (size_t)36 * a.rows * d->cin * 6)
             : a.v + (size_t)36 * a.rows * d->cin;
    hipStream_t st = as_stream(stream);
    a.gw = planes ? d->deconv_ks : 0;
    a.c0 = 0; a.cn = d->cout;
    if (x3) {
        // f32x3: u_packed is the three-plane bf16 form (sgv3d_conv_winograd4_pack_weight_x3), desc.cout_pad its rows per block
        SGV3D_REQUIRE(d->cin % 32 == 0 && d->cout_pad % 32 == 0 && d->cout_pad >= d->cout,
                      "conv2d_winograd4_forward: SGV3D_TILE_X3 needs cin %% 32 == 0 and cout_pad (a multiple of 32) of the x3 weights");
        SGV3D_REQUIRE((d->tile & 15) < 10, "conv2d_winograd4_forward: unknown SGV3D_TILE_X3 variant %d", d->tile & 15);
        if (d->dil > 1) hipLaunchKernelGGL(wino4_input_x3_kernel<true>, dim3(cdiv(tiles * (d->cin / 4), kTB)), dim3(kTB), 0, st, a);
        else hipLaunchKernelGGL(wino4_input_x3_kernel<false>, dim3(cdiv(tiles * (d->cin / 4), kTB)), dim3(kTB), 0, st, a);
        const int chunk3 = wino4_chunk(d, a.rows);
        for (int c0 = 0; c0 < d->cout; c0 += chunk3) {
            a.c0 = c0;
            a.cn = d->cout - c0 < chunk3 ? d->cout - c0 : chunk3;
            // block p of the chunk's weights: cout_pad rows of cin * 6 bytes after block p - 1, shifted by c0 rows
            if (int rc = conv_gemm_grouped_x3(a.v, static_cast<const unsigned char *>(static_cast<const void *>(u_packed)) + (size_t)c0 * d->cin * 6,
                                              a.m, a.rows, d->cin, a.cn, d->cout_pad - c0, d->tile & 15, st, (size_t)d->cout_pad * d->cin * 6)) return rc;
            if (d->dil > 1) hipLaunchKernelGGL(wino4_output_kernel<true>, dim3(cdiv(tiles * (a.cn / 4), kTB)), dim3(kTB), 0, st, a);
            else hipLaunchKernelGGL(wino4_output_kernel<false>, dim3(cdiv(tiles * (a.cn / 4), kTB)), dim3(kTB), 0, st, a);
        }
        return check_launch("conv2d_winograd4_forward(x3)");
    }
    if (d->dil > 1) hipLaunchKernelGGL(wino4_input_kernel<true>, dim3(cdiv(tiles * (d->cin / 4), kTB)), dim3(kTB), 0, st, a);
    else hipLaunchKernelGGL(wino4_input_kernel<false>, dim3(cdiv(tiles * (d->cin / 4), kTB)), dim3(kTB), 0, st, a);
    int tile = (d->tile == SGV3D_TILE_64x128 || d->tile == SGV3D_TILE_32x128 || d->tile == SGV3D_TILE_48x64) ? d->tile
               : (d->tile & SGV3D_TILE_OCC5) ? (SGV3D_TILE_64x64 | SGV3D_TILE_OCC5) : SGV3D_TILE_64x64;
    if (tile == SGV3D_TILE_32x128 && (d->k_order != 1 || d->cin < 128)) tile = SGV3D_TILE_64x64;    // (what the narrow tile covers)
    SGV3D_REQUIRE(tile != SGV3D_TILE_48x64 || (d->k_order == 1 && d->cin % 32 == 0),
                  "conv2d_winograd4_forward: SGV3D_TILE_48x64 needs channel-chunk-major weights (cin %% 32 == 0)");
    // one pass per chunk of output channels: block p of the chunk's weights is cout_pad x k_pad floats after block p - 1
    // like the full blocks, shifted by c0 rows
    const int chunk = wino4_chunk(d, a.rows);
    for (int c0 = 0; c0 < d->cout; c0 += chunk) {
        a.c0 = c0;
        a.cn = d->cout - c0 < chunk ? d->cout - c0 : chunk;
        if (tile == SGV3D_TILE_48x64) {
            if (int rc = conv_gemm_grouped16(a.v, u_packed + (size_t)c0 * d->k_pad, a.m, a.rows, 36, d->cin, a.cn, d->k_pad,
                                             d->cout_pad, st)) return rc;
        } else if (int rc = conv_gemm_grouped(a.v, u_packed + (size_t)c0 * d->k_pad, a.m, a.rows, 36, d->cin, a.cn, d->k_pad,
                                              d->cout_pad, d->k_order, tile, st)) return rc;
        if (d->dil > 1) hipLaunchKernelGGL(wino4_output_kernel<true>, dim3(cdiv(tiles * (a.cn / 4), kTB)), dim3(kTB), 0, st, a);
        else hipLaunchKernelGGL(wino4_output_kernel<false>, dim3(cdiv(tiles * (a.cn / 4), kTB)), dim3(kTB), 0, st, a);
    }
    return check_launch("conv2d_winograd4_forward");
}

// ---- sibling layers on one input: one input-transform launch, n grouped GEMMs, one output-transform launch ------------------
namespace {

// what sgv3d_conv2d_winograd4_forward checks, for one descriptor of the multi entry point (f32x3, NHWC, one channel pass)
int wino4_multi_check(const sgv3d_conv_desc *d, const sgv3d_conv_desc *d0, const void *u, const float *scale, const float *bias, const float *y) {
    SGV3D_REQUIRE(u && y, "conv2d_winograd4_forward_multi: null pointer");
    SGV3D_REQUIRE(d->kh == 3 && d->kw == 3 && d->stride == 1 && d->dil >= 1 && d->pad == d->dil,
                  "conv2d_winograd4_forward_multi: only 3x3 / stride 1 / pad == dilation");
    SGV3D_REQUIRE(d->batch > 0 && d->in_h > 0 && d->in_w > 0 && d->cin > 0 && d->cout > 0 && d->out_h == d->in_h && d->out_w == d->in_w,
                  "conv2d_winograd4_forward_multi: bad sizes");
    SGV3D_REQUIRE(d->batch == d0->batch && d->in_h == d0->in_h && d->in_w == d0->in_w && d->cin == d0->cin && d->x_ld == d0->x_ld &&
                      d->x_coff == d0->x_coff,
                  "conv2d_winograd4_forward_multi: the layers must read the same input (batch, map, cin, x_ld, x_coff)");
    SGV3D_REQUIRE(d->mode == SGV3D_CONV_NORMAL && d->split_k <= 1, "conv2d_winograd4_forward_multi: NHWC output, no split-K");
    SGV3D_REQUIRE((d->tile & SGV3D_TILE_X3) && (d->tile & 15) < 10, "conv2d_winograd4_forward_multi: SGV3D_TILE_X3 | variant tiles only");
    SGV3D_REQUIRE(d->cin % 32 == 0 && d->cout % 4 == 0 && d->cout_pad % 32 == 0 && d->cout_pad >= d->cout && (d->x_ld & 3) == 0 &&
                      (d->x_coff & 3) == 0 && (d->y_ld & 3) == 0 && (d->y_coff & 3) == 0,
                  "conv2d_winograd4_forward_multi: cin %% 32, cout %% 4, cout_pad %% 32, leading dimensions and offsets %% 4");
    SGV3D_REQUIRE(((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(scale) |
                    reinterpret_cast<uintptr_t>(bias)) & 15) == 0, "conv2d_winograd4_forward_multi: pointers must be 16-B aligned");
    SGV3D_REQUIRE(d->x_ld >= d->x_coff + d->cin && d->y_ld >= d->y_coff + d->cout, "conv2d_winograd4_forward_multi: leading dimension too small");
    return SGV3D_OK;
}

}  // namespace

// the layers' own workspaces (sgv3d_conv2d_winograd4_workspace_bytes), one after another
extern "C" size_t sgv3d_conv2d_winograd4_multi_workspace_bytes(int n, const sgv3d_conv_desc *descs) {
    if (!descs || n < 1 || n > kWino4Multi) return 0;
    size_t total = 0;
    for (int l = 0; l < n; ++l) {
        const size_t b = sgv3d_conv2d_winograd4_workspace_bytes(descs + l);
        if (b == 0) return 0;
        total += (b + 255) / 256 * 256;
    }
    return total;
}

// n <= 4 F(4x4) layers with f32x3 tiles that read the same x (descs[l] may differ in dilation, weights, folded BN, output slice
// and tile variant; no residual): ONE launch of the input transform for all, the n grouped GEMMs as
// sgv3d_conv2d_winograd4_forward launches them, ONE launch of the output transform.  Bit-equal to n single calls.
extern "C" int sgv3d_conv2d_winograd4_forward_multi(int n, const sgv3d_conv_desc *descs, const float *x, const void *const *u_packed,
                                                    const float *const *scale, const float *const *bias, float *const *y,
                                                    void *workspace, size_t workspace_bytes, void *stream) {
    SGV3D_REQUIRE(n >= 1 && n <= kWino4Multi, "conv2d_winograd4_forward_multi: 1 to %d layers, not %d", kWino4Multi, n);
    SGV3D_REQUIRE(descs && x && u_packed && scale && bias && y && workspace, "conv2d_winograd4_forward_multi: null pointer");
    SGV3D_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
                  "conv2d_winograd4_forward_multi: pointers must be 16-B aligned");
    for (int l = 0; l < n; ++l)
        if (int rc = wino4_multi_check(descs + l, descs, u_packed[l], scale[l], bias[l], y[l])) return rc;
    const size_t need = sgv3d_conv2d_winograd4_multi_workspace_bytes(n, descs);
    if (workspace_bytes < need)
        return fail(SGV3D_ENOSPACE, "conv2d_winograd4_forward_multi: workspace has %zu bytes, needs %zu", workspace_bytes, need);
    Wino4MultiArgs in, out;
    in.n = out.n = n;
    in.first[0] = out.first[0] = 0;
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    for (int l = 0; l < n; ++l) {
        const sgv3d_conv_desc *d = descs + l;
        Wino4Args &a = in.a[l];
        a.x = x; a.scale = scale[l]; a.bias = bias[l]; a.res = nullptr; a.y = y[l];
        a.batch = d->batch; a.h = d->in_h; a.w = d->in_w; a.cin = d->cin; a.cout = d->cout;
        a.x_ld = d->x_ld; a.x_coff = d->x_coff; a.y_ld = d->y_ld; a.y_coff = d->y_coff; a.res_ld = 0; a.relu = d->relu;
        long long tiles;
        wino4_geom(d, a.ay, a.ax, tiles, a.rows);
        SGV3D_REQUIRE(tiles < 0x7fffffffLL / 64, "conv2d_winograd4_forward_multi: too many tiles");
        SGV3D_REQUIRE(wino4_chunk(d, a.rows) == d->cout, "conv2d_winograd4_forward_multi: a layer whose M needs more than one channel pass");
        a.v = reinterpret_cast<float *>(ws);
        a.m = reinterpret_cast<float *>(ws + (size_t)36 * a.rows * d->cin * 6);
        ws += (sgv3d_conv2d_winograd4_workspace_bytes(d) + 255) / 256 * 256;
        a.gw = 0; a.c0 = 0; a.cn = d->cout;
        out.a[l] = a;
        in.first[l + 1] = in.first[l] + cdiv(tiles * (d->cin / 4), kTB);
        out.first[l + 1] = out.first[l] + cdiv(tiles * (d->cout / 4), kTB);
    }
    for (int l = n; l < kWino4Multi; ++l) {
        in.a[l] = in.a[0]; out.a[l] = out.a[0];
        in.first[l + 1] = in.first[n]; out.first[l + 1] = out.first[n];
    }
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(wino4_input_x3_multi_kernel, dim3(in.first[n]), dim3(kTB), 0, st, in);
    for (int l = 0; l < n; ++l) {
        const sgv3d_conv_desc *d = descs + l;
        const Wino4Args &a = in.a[l];
        if (int rc = conv_gemm_grouped_x3(a.v, static_cast<const unsigned char *>(u_packed[l]), a.m, a.rows, d->cin, d->cout, d->cout_pad,
                                          d->tile & 15, st, (size_t)d->cout_pad * d->cin * 6)) return rc;
    }
    hipLaunchKernelGGL(wino4_output_multi_kernel, dim3(out.first[n]), dim3(kTB), 0, st, out);
    return check_launch("conv2d_winograd4_forward_multi");
}
