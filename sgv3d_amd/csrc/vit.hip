// SAM's ViT image encoder (layers/backbones/sam_encoder.py of the reference), the parts that are not a convolution:
// windowed / global attention with decomposed relative position (one flash-style launch on the f32 MFMA), LayerNorm over
// the channels of an NHWC map, exact GELU, the input normalise + pad, and the crop + bilinear resize behind the neck.
// gfx950 only.  Vector stores only, no float atomics: every kernel is repeatable bit for bit.
#include <math.h>

#include "common.hpp"

using namespace sgv3d;

namespace sgv3d {
int vit_attention_impl(const sgv3d_vit_attn_desc *desc, const float *qkv, const float *pad_qkv, const float *rel_pos_h,
                       const float *rel_pos_w, float *out, float *lse, void *stream);
}

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;
constexpr int kQT = 64;  // queries per workgroup: 16 per wave
constexpr int kKT = 64;  // keys per LDS tile

static inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------------------------
// attention
// ------------------------------------------------------------------------------------------------
// A workgroup owns 64 consecutive queries of one (image, head, window); wave w owns 16 of them.  All products are
// v_mfma_f32_16x16x4_f32 (A: lane holds [row lane & 15][k lane >> 4], B: [k lane >> 4][col lane & 15], D: col lane & 15,
// row 4 * (lane >> 4) + reg).
//   S^T = K Q^T  (swapped): lane (q = lane & 15, g = lane >> 4) holds the logits of query q for keys 4 g + r, r = 0..3, of each
//                16-key sub-tile, so the row maximum is 16 in-lane fmax and two cross-lane steps.  A dot product may sum the head
//                dimension in any order as long as both operands agree: k-step 4 c + i takes d = 16 c + 4 g + i from lane group
//                g, so a lane's operands of four steps are ONE 16-byte read (q from HBM once, K from LDS per tile).
//   O^T = V^T P^T: k-step r of a sub-tile sums over the keys {4 g + r}: the B operand is accumulator register r of S^T as it
//                stands, no lane movement.  The rows of O^T may stand for any d as well: accumulator 4 c + i holds d = 64 c +
//                4 (lane & 15) + i in row lane & 15, so one 16-byte read of V[key][64 c + 4 (lane & 15)] feeds four MFMAs
//                (a 32- or 16-wide rest of the head dimension takes 8- and 4-byte reads the same way).  O^T has the query on
//                the lane too: the online-softmax rescale is one multiplier per lane, and a lane stores 16 consecutive floats.
// K sits in LDS with rows of head_dim + 8 floats and V with rows of head_dim (40 at head_dim 32): with these strides the
// 16-byte operand reads of both are conflict-free in the lane groups the LDS serves them in.  The next tile is loaded into
// registers after QK^T and written to LDS behind the barrier.  T_h = q rel_pos_h^T and T_w = q rel_pos_w^T are formed once
// per workgroup on the MFMA (table rows as the A operand) and kept in LDS as [query][kh] and [query][kw].
// Workgroups are renumbered so that each of the 8 XCDs, which take consecutive workgroup ids in turn, walks a contiguous
// run of (image, head, window, query tile): the query tiles that share a head's K and V then share an L2.
struct AttnParams {
    int B, H, W, nH, win_h, win_w, nwy, nwx, T, nqt, th_ld, tw_ld;
    float scale, inv_win_w;
    const float *qkv, *pad, *rh, *rw;
    float *out;
    float *lse;      // LSE kernels only: [B, nH, H, W], row maximum + log of the row sum
};

template <int HD>
struct AttnGeom {
    static constexpr int LDK = HD + 8;               // LDS row of K
    static constexpr int LDV = HD == 32 ? 40 : HD;   // LDS row of V
    static constexpr int floats = kKT * (LDK + LDV);
};

template <int HD, bool LSE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(HD <= 64 ? 3 : 2))) void vit_attention_kernel(AttnParams p) {
    constexpr int LDK = AttnGeom<HD>::LDK, LDV = AttnGeom<HD>::LDV;
    constexpr int NC = HD / 16;  // 16-byte operand reads per key row of QK^T (four k-steps each)
    constexpr int NS = HD / 4;   // k-steps of QK^T
    constexpr int NJ = HD / 16;  // accumulators of O^T
    constexpr int N4 = NJ / 4, N2 = (NJ % 4) / 2, N1 = NJ % 2;   // ... fed four, two and one at a time
    constexpr int D2 = 64 * N4, D1 = D2 + 32 * N2;               // where the 8- and 4-byte parts of the head dimension begin
    constexpr int NL = HD / 16;  // float4 per thread, tensor and tile
    constexpr int C4 = HD / 4;   // float4 per key row
    extern __shared__ __align__(16) float lds[];
    float *Ks = lds;
    float *Vs = Ks + kKT * LDK;
    float *Th = Vs + kKT * LDV;
    float *Tw = Th + kQT * p.th_ld;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, g = lane >> 4;
    int bid = blockIdx.x;
    {
        const int per_xcd = gridDim.x / 8;
        if (bid < 8 * per_xcd) bid = (bid & 7) * per_xcd + (bid >> 3);     // (the last gridDim.x % 8 ids stay)
    }
    const int qt = bid % p.nqt;
    bid /= p.nqt;
    const int wx = bid % p.nwx;
    bid /= p.nwx;
    const int wy = bid % p.nwy;
    bid /= p.nwy;
    const int head = bid % p.nH;
    const int b = bid / p.nH;
    const int C = p.nH * HD;
    const int h0 = wy * p.win_h, w0 = wx * p.win_w;
    const bool rel = p.rh != nullptr;

    // q, k, v of window token t (< T): the map's row, or the padding token's (null: zeros)
    auto token = [&](int t) -> const float * {
        const int kh = (int)(((float)t + 0.5f) * p.inv_win_w), kw = t - kh * p.win_w;     // t / win_w, see below
        const int h = h0 + kh, w = w0 + kw;
        if (h < p.H && w < p.W) return p.qkv + ((size_t)((size_t)b * p.H + h) * p.W + w) * (size_t)(3 * C) + head * HD;
        return p.pad ? p.pad + head * HD : nullptr;
    };

    // this lane's query: q[4 c + i] = Q[16 c + 4 g + i]
    const int myq = wave * 16 + lq;
    int tq = qt * kQT + myq;
    const bool q_live = tq < p.T;
    tq = q_live ? tq : p.T - 1;
    const int qh = tq / p.win_w, qw = tq - qh * p.win_w;
    float q[NS], qs[NS];
    {
        const float *src = token(tq);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (src) v = *reinterpret_cast<const f32x4 *>(src + 16 * c + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                q[4 * c + i] = v[i];
                qs[4 * c + i] = v[i] * p.scale;
            }
        }
    }

    if (rel) {
        // T_h[query][kh] = q . rel_pos_h[qh - kh + win_h - 1]: the product with every table row, kept where a key row answers
        for (int axis = 0; axis < 2; ++axis) {
            const float *tab = axis ? p.rw : p.rh;
            const int win = axis ? p.win_w : p.win_h, ld = axis ? p.tw_ld : p.th_ld, qpos = axis ? qw : qh;
            float *dst = (axis ? Tw : Th) + myq * ld;
            const int rows = 2 * win - 1;
            for (int r0 = 0; r0 < rows; r0 += 16) {
                const float *trow = tab + (size_t)min(r0 + lq, rows - 1) * HD + 4 * g;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(trow + 16 * c);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], q[4 * c + i], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = r0 + 4 * g + r;
                    const int kpos = qpos + win - 1 - t;
                    if (t < rows && kpos >= 0 && kpos < win) dst[kpos] = acc[r];
                }
            }
        }
    }

    f32x4 kreg[NL], vreg[NL];
    auto gload = [&](int tile) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int key = i / C4, c4 = i - key * C4;
            const int t = tile * kKT + key;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};   // keys past T: zero V (their P is exactly 0)
            if (t < p.T) {
                const float *src = token(t);
                if (src) {
                    kv = *reinterpret_cast<const f32x4 *>(src + C + 4 * c4);
                    vv = *reinterpret_cast<const f32x4 *>(src + 2 * C + 4 * c4);
                }
            }
            kreg[n] = kv;
            vreg[n] = vv;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int key = i / C4, c4 = i - key * C4;
            *reinterpret_cast<f32x4 *>(Ks + key * LDK + 4 * c4) = kreg[n];
            *reinterpret_cast<f32x4 *>(Vs + key * LDV + 4 * c4) = vreg[n];
        }
    };

    const int ntiles = (p.T + kKT - 1) / kKT;
    float m = -INFINITY, l = 0.f;     // running maximum (the same in the four lanes of a query), this lane's share of the sum
    f32x4 O[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) O[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *th = Th + myq * p.th_ld, *tw = Tw + myq * p.tw_ld;
    const float *kbase = Ks + lq * LDK + 4 * g;      // + sub * 16 * LDK + 16 * c
    const float *vbase = Vs + 4 * g * LDV;           // + (sub * 16 + r) * LDV + the lane's columns

    gload(0);
    for (int tile = 0; tile < ntiles; ++tile) {
        __syncthreads();   // the previous tile has been read (first pass: T_h, T_w are written)
        lstore();
        __syncthreads();

        f32x4 S[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) S[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x4 kf[4];
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) kf[sub] = *reinterpret_cast<const f32x4 *>(kbase + sub * 16 * LDK + 16 * c);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)      // four independent accumulators in turn
                    S[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[sub][i], qs[4 * c + i], S[sub], 0, 0, 0);
        }

        if (tile + 1 < ntiles) gload(tile + 1);

        const bool last = tile == ntiles - 1;     // the only tile with slots past T
        float mx = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = tile * kKT + sub * 16 + 4 * g + r;
                float s = S[sub][r];
                if (rel) {
                    // kh = t / win_w without the integer division: exact for t < 128 * win_w, win_w <= 128 (every case is
                    // enumerated in tests/test_sam_encoder_cpu.py); a slot past T reads a valid entry and is masked below
                    const int tc = last ? min(t, p.T - 1) : t;
                    const int kh = (int)(((float)tc + 0.5f) * p.inv_win_w), kw = tc - kh * p.win_w;
                    s += th[kh] + tw[kw];
                }
                if (last && t >= p.T) s = -INFINITY;     // a key past the window: masked, not a zero logit
                S[sub][r] = s;
                mx = fmaxf(mx, s);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m, mx);      // finite from the first tile on: key 0 is never masked
        const float alpha = __expf(m - m_new);   // first tile: exp(-inf) = 0
        l *= alpha;
#pragma unroll
        for (int j = 0; j < NJ; ++j) O[j] *= alpha;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(S[sub][r] - m_new);     // v_exp_f32 of the difference times log2(e)
                S[sub][r] = e;
                l += e;
            }
        m = m_new;

#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *vrow = vbase + (sub * 16 + r) * LDV;
                const float pk = S[sub][r];
#pragma unroll
                for (int c = 0; c < N4; ++c) {
                    const f32x4 vf = *reinterpret_cast<const f32x4 *>(vrow + 64 * c + 4 * lq);
#pragma unroll
                    for (int i = 0; i < 4; ++i) O[4 * c + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i], pk, O[4 * c + i], 0, 0, 0);
                }
                if (N2) {
                    const f32x2 vf = *reinterpret_cast<const f32x2 *>(vrow + D2 + 2 * lq);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        O[4 * N4 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i], pk, O[4 * N4 + i], 0, 0, 0);
                }
                if (N1) O[NJ - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[D1 + lq], pk, O[NJ - 1], 0, 0, 0);
            }
    }

    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const int oh = h0 + qh, ow = w0 + qw;
    if (q_live && oh < p.H && ow < p.W) {
        if (LSE && g == 0) p.lse[(((size_t)b * p.nH + head) * p.H + oh) * p.W + ow] = m + logf(l);
        // row 4 g + r of accumulator 4 c + i is d = 64 c + 4 (4 g + r) + i: sixteen consecutive floats per lane and c
        float *dst = p.out + ((size_t)((size_t)b * p.H + oh) * p.W + ow) * (size_t)C + head * HD;
#pragma unroll
        for (int c = 0; c < N4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 o = {O[4 * c][r] / l, O[4 * c + 1][r] / l, O[4 * c + 2][r] / l, O[4 * c + 3][r] / l};
                *reinterpret_cast<f32x4 *>(dst + 64 * c + 16 * g + 4 * r) = o;
            }
        if (N2) {      // d = D2 + 2 (4 g + r) + i
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const f32x4 o = {O[4 * N4][r] / l, O[4 * N4 + 1][r] / l, O[4 * N4][r + 1] / l, O[4 * N4 + 1][r + 1] / l};
                *reinterpret_cast<f32x4 *>(dst + D2 + 8 * g + 2 * r) = o;
            }
        }
        if (N1) {      // d = D1 + 4 g + r
            const f32x4 o = {O[NJ - 1][0] / l, O[NJ - 1][1] / l, O[NJ - 1][2] / l, O[NJ - 1][3] / l};
            *reinterpret_cast<f32x4 *>(dst + D1 + 4 * g) = o;
        }
    }
}

template <int HD, bool LSE>
int launch_attention_lse(const AttnParams &p, int blocks, size_t lds_bytes, hipStream_t stream) {
    static PerDeviceSize state;
    if (!ensure_dynamic_lds(reinterpret_cast<const void *>(vit_attention_kernel<HD, LSE>), lds_bytes, state))
        return fail(SGV3D_ELAUNCH, "vit_attention: cannot reserve %zu bytes of LDS", lds_bytes);
    hipLaunchKernelGGL((vit_attention_kernel<HD, LSE>), dim3(blocks), dim3(kBlock), lds_bytes, stream, p);
    return check_launch("vit_attention_kernel");
}

// LSE is a template parameter: the instantiation without it is the kernel as it was, instruction for instruction
template <int HD>
int launch_attention(const AttnParams &p, int blocks, size_t lds_bytes, hipStream_t stream) {
    return p.lse ? launch_attention_lse<HD, true>(p, blocks, lds_bytes, stream) : launch_attention_lse<HD, false>(p, blocks, lds_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// LayerNorm: one wave per row
// ------------------------------------------------------------------------------------------------
__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// Two passes, never E[x^2] - E[x]^2.  The sums are carried in f64: the test's bar is relative to |x_hat| element by element, and
// a mean rounded to f32 is off by up to half an ulp OF THE MEAN -- for a row that sits at 1e4 with unit spread that alone is
// 5e-4 on every x_hat, whatever its size.  With the f64 mean, x - mean is rounded once, relative to itself.
__global__ __launch_bounds__(kBlock) void layernorm_kernel(long long rows, int c4, const f32x4 *x, const f32x4 *__restrict__ weight,
                                                           const f32x4 *__restrict__ bias, float eps, f32x4 *y) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const f32x4 *xr = x + row * c4;
    f32x4 *yr = y + row * c4;
    const double inv_c = 1.0 / (4.0 * (double)c4);
    double s = 0.0;
    for (int i = lane; i < c4; i += 64) {
        const f32x4 v = xr[i];
        s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
    }
    const double mean = wave_sum(s) * inv_c;
    double sq = 0.0;
    for (int i = lane; i < c4; i += 64) {
        const f32x4 v = xr[i];
        const double e0 = (double)v[0] - mean, e1 = (double)v[1] - mean, e2 = (double)v[2] - mean, e3 = (double)v[3] - mean;
        sq += (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
    }
    const float rstd = (float)(1.0 / sqrt(wave_sum(sq) * inv_c + (double)eps));
    for (int i = lane; i < c4; i += 64) {
        const f32x4 v = xr[i], w = weight[i], bb = bias[i];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (float)((double)v[k] - mean) * rstd * w[k] + bb[k];
        yr[i] = o;
    }
}

// ------------------------------------------------------------------------------------------------
// GELU (erf form).  For x < 0, 1 + erf(z) is written erfc(-z): no cancellation in the left tail.
// ------------------------------------------------------------------------------------------------
__device__ inline float gelu1(float x) {
    const float z = x * 0.70710678118654752440f;
    const float t = x < 0.f ? erfcf(-z) : 1.0f + erff(z);
    return 0.5f * x * t;
}

__global__ __launch_bounds__(kBlock) void gelu_kernel(long long n4, int tail, const float *x, float *y) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n4) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = gelu1(v[k]);
        reinterpret_cast<f32x4 *>(y)[i] = o;
    }
    if (i < tail) y[4 * n4 + i] = gelu1(x[4 * n4 + i]);
}

// ------------------------------------------------------------------------------------------------
// normalise + pad to the square, NCHW -> NHWC with four channels
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void vit_preprocess_kernel(int B, int H, int W, int S, const float *__restrict__ img,
                                                                const float *__restrict__ mean, const float *__restrict__ stdv,
                                                                f32x4 *y) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)B * S * S) return;
    const int w = (int)(i % S);
    const int h = (int)((i / S) % S);
    const long long b = i / ((long long)S * S);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (h < H && w < W) {
        const float *src = img + ((b * 3) * H + h) * (long long)W + w;
        const long long plane = (long long)H * W;
        o[0] = (src[0] - mean[0]) / stdv[0];
        o[1] = (src[plane] - mean[1]) / stdv[1];
        o[2] = (src[2 * plane] - mean[2]) / stdv[2];
    }
    y[i] = o;
}

// ------------------------------------------------------------------------------------------------
// crop + bilinear resize (align_corners=False), NHWC
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void resize_bilinear_kernel(int B, int h, int w, int c4, int ch, int cw, int oh, int ow,
                                                                 const f32x4 *__restrict__ x, f32x4 *y) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)B * oh * ow * c4) return;
    const int c = (int)(i % c4);
    const int ox = (int)((i / c4) % ow);
    const int oy = (int)((i / ((long long)c4 * ow)) % oh);
    const long long b = i / ((long long)c4 * ow * oh);
    const double sy = fmax(((double)oy + 0.5) * ((double)ch / (double)oh) - 0.5, 0.0);
    const double sx = fmax(((double)ox + 0.5) * ((double)cw / (double)ow) - 0.5, 0.0);
    const int y0 = min((int)sy, ch - 1), x0 = min((int)sx, cw - 1);
    const int y1 = y0 + (y0 < ch - 1 ? 1 : 0), x1 = x0 + (x0 < cw - 1 ? 1 : 0);
    const double ly = sy - (double)y0, lx = sx - (double)x0;
    const double hy = 1.0 - ly, hx = 1.0 - lx;
    const f32x4 *base = x + b * h * (long long)w * c4 + c;
    const f32x4 v00 = base[((long long)y0 * w + x0) * c4], v01 = base[((long long)y0 * w + x1) * c4];
    const f32x4 v10 = base[((long long)y1 * w + x0) * c4], v11 = base[((long long)y1 * w + x1) * c4];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o[k] = (float)(hy * (hx * (double)v00[k] + lx * (double)v01[k]) + ly * (hx * (double)v10[k] + lx * (double)v11[k]));
    y[i] = o;
}

}  // namespace

// sgv3d_vit_attention, and with `lse` sgv3d_vit_attention_lse (csrc/vit_grad.hip): one body, so `out` has the same bits in both
int sgv3d::vit_attention_impl(const sgv3d_vit_attn_desc *desc, const float *qkv, const float *pad_qkv, const float *rel_pos_h,
                              const float *rel_pos_w, float *out, float *lse, void *stream) {
    SGV3D_REQUIRE(desc, "vit_attention: null descriptor");
    const sgv3d_vit_attn_desc &d = *desc;
    SGV3D_REQUIRE(d.batch > 0 && d.height > 0 && d.width > 0 && d.heads > 0 && d.head_dim > 0 && d.win_h > 0 && d.win_w > 0,
                  "vit_attention: zero or negative dimension (batch %d, map %d x %d, heads %d, head_dim %d, window %d x %d)", d.batch,
                  d.height, d.width, d.heads, d.head_dim, d.win_h, d.win_w);
    SGV3D_REQUIRE((long long)d.heads * d.head_dim % 4 == 0, "vit_attention: heads * head_dim = %lld is not a multiple of 4", (long long)d.heads * d.head_dim);
    SGV3D_REQUIRE(d.head_dim == 32 || d.head_dim == 64 || d.head_dim == 80, "vit_attention: head_dim %d is not one of 32, 64, 80",
                  d.head_dim);
    SGV3D_REQUIRE(d.win_h <= 128 && d.win_w <= 128, "vit_attention: window %d x %d exceeds 128", d.win_h, d.win_w);
    SGV3D_REQUIRE((rel_pos_h == nullptr) == (rel_pos_w == nullptr),
                  "vit_attention: rel_pos_h and rel_pos_w must be given together or not at all");
    SGV3D_REQUIRE(qkv && out, "vit_attention: null qkv or out");
    SGV3D_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(pad_qkv), "vit_attention: qkv, pad_qkv and out must be 16-byte aligned");
    const long long channels = (long long)d.heads * d.head_dim;
    SGV3D_REQUIRE(3 * channels < (1LL << 24), "vit_attention: heads * head_dim too large");
    AttnParams p;
    p.B = d.batch, p.H = d.height, p.W = d.width, p.nH = d.heads, p.win_h = d.win_h, p.win_w = d.win_w;
    p.nwy = cdiv(d.height, d.win_h), p.nwx = cdiv(d.width, d.win_w);
    p.T = d.win_h * d.win_w;
    p.nqt = cdiv(p.T, kQT);
    const bool rel = rel_pos_h != nullptr;
    p.th_ld = rel ? (d.win_h | 1) : 0;      // odd rows: the four lanes of a query and its 15 neighbours spread over the banks
    p.tw_ld = rel ? (d.win_w | 1) : 0;
    p.scale = 1.0f / sqrtf((float)d.head_dim);
    p.inv_win_w = 1.0f / (float)d.win_w;
    p.qkv = qkv, p.pad = pad_qkv, p.rh = rel_pos_h, p.rw = rel_pos_w, p.out = out, p.lse = lse;
    const long long blocks = (long long)d.batch * d.heads * p.nwy * p.nwx * p.nqt;
    SGV3D_REQUIRE(blocks < (1LL << 31), "vit_attention: too many workgroups");
    const int kv_floats = d.head_dim == 32 ? AttnGeom<32>::floats : d.head_dim == 64 ? AttnGeom<64>::floats : AttnGeom<80>::floats;
    const size_t lds_bytes = sizeof(float) * ((size_t)kv_floats + (size_t)kQT * (p.th_ld + p.tw_ld));
    hipStream_t s = as_stream(stream);
    switch (d.head_dim) {
        case 32: return launch_attention<32>(p, (int)blocks, lds_bytes, s);
        case 64: return launch_attention<64>(p, (int)blocks, lds_bytes, s);
        default: return launch_attention<80>(p, (int)blocks, lds_bytes, s);
    }
}

extern "C" int sgv3d_vit_attention(const sgv3d_vit_attn_desc *desc, const float *qkv, const float *pad_qkv,
                                   const float *rel_pos_h, const float *rel_pos_w, float *out, void *stream) {
    return vit_attention_impl(desc, qkv, pad_qkv, rel_pos_h, rel_pos_w, out, nullptr, stream);
}

extern "C" int sgv3d_layernorm(long long rows, int channels, const float *x, const float *weight, const float *bias, float eps,
                               float *y, void *stream) {
    SGV3D_REQUIRE(rows > 0 && channels > 0, "layernorm: non-positive size (rows %lld, channels %d)", rows, channels);
    SGV3D_REQUIRE(channels % 4 == 0, "layernorm: channels %d is not a multiple of 4", channels);
    SGV3D_REQUIRE(x && weight && bias && y, "layernorm: null pointer");
    SGV3D_REQUIRE(eps >= 0.f, "layernorm: negative eps");
    SGV3D_REQUIRE(aligned16(x) && aligned16(weight) && aligned16(bias) && aligned16(y), "layernorm: pointers must be 16-byte aligned");
    const long long blocks = (rows + kBlock / 64 - 1) / (kBlock / 64);
    SGV3D_REQUIRE(blocks < (1LL << 31), "layernorm: too many rows");
    hipLaunchKernelGGL(layernorm_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), rows, channels / 4,
                       reinterpret_cast<const f32x4 *>(x), reinterpret_cast<const f32x4 *>(weight),
                       reinterpret_cast<const f32x4 *>(bias), eps, reinterpret_cast<f32x4 *>(y));
    return check_launch("layernorm_kernel");
}

extern "C" int sgv3d_gelu(long long n, const float *x, float *y, void *stream) {
    SGV3D_REQUIRE(n > 0, "gelu: non-positive count %lld", n);
    SGV3D_REQUIRE(x && y, "gelu: null pointer");
    SGV3D_REQUIRE(aligned16(x) && aligned16(y), "gelu: pointers must be 16-byte aligned");
    const long long n4 = n / 4;
    const long long blocks = (n4 + kBlock) / kBlock;    // at least one: its first threads take the tail
    SGV3D_REQUIRE(blocks < (1LL << 31), "gelu: too many values");
    hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), n4, (int)(n - 4 * n4), x, y);
    return check_launch("gelu_kernel");
}

extern "C" int sgv3d_vit_preprocess(int batch, int height, int width, const float *img, const float *mean, const float *stdv,
                                    int size, float *y, void *stream) {
    SGV3D_REQUIRE(batch > 0 && height > 0 && width > 0 && size > 0, "vit_preprocess: non-positive size");
    SGV3D_REQUIRE((height > width ? height : width) == size, "vit_preprocess: the long side of %d x %d is not %d", height, width, size);
    SGV3D_REQUIRE(img && mean && stdv && y, "vit_preprocess: null pointer");
    SGV3D_REQUIRE(aligned16(y), "vit_preprocess: y must be 16-byte aligned");
    const long long blocks = ((long long)batch * size * size + kBlock - 1) / kBlock;
    SGV3D_REQUIRE(blocks < (1LL << 31), "vit_preprocess: too many pixels");
    hipLaunchKernelGGL(vit_preprocess_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), batch, height, width, size,
                       img, mean, stdv, reinterpret_cast<f32x4 *>(y));
    return check_launch("vit_preprocess_kernel");
}

extern "C" int sgv3d_resize_bilinear(int batch, int h, int w, int channels, int crop_h, int crop_w, int out_h, int out_w,
                                     const float *x, float *y, void *stream) {
    SGV3D_REQUIRE(batch > 0 && h > 0 && w > 0 && channels > 0 && crop_h > 0 && crop_w > 0 && out_h > 0 && out_w > 0,
                  "resize_bilinear: non-positive size");
    SGV3D_REQUIRE(channels % 4 == 0, "resize_bilinear: channels %d is not a multiple of 4", channels);
    SGV3D_REQUIRE(x && y, "resize_bilinear: null pointer");
    SGV3D_REQUIRE(aligned16(x) && aligned16(y), "resize_bilinear: pointers must be 16-byte aligned");
    const int ch = crop_h < h ? crop_h : h, cw = crop_w < w ? crop_w : w;
    const long long blocks = ((long long)batch * out_h * out_w * (channels / 4) + kBlock - 1) / kBlock;
    SGV3D_REQUIRE(blocks < (1LL << 31), "resize_bilinear: too many outputs");
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), batch, h, w, channels / 4,
                       ch, cw, out_h, out_w, reinterpret_cast<const f32x4 *>(x), reinterpret_cast<f32x4 *>(y));
    return check_launch("resize_bilinear_kernel");
}
