// What the four ViT sources (vit.hip, vit_bf16.hip, vit_grad.hip, vit_grad_bf16.hip) must agree on bit for bit, each defined
// once: the descriptor checks and the window geometry of the attention entries, the LayerNorm row statistics, the erf term of
// GELU, and the f32 MFMA operand code for a head dimension split into 64-, 32- and 16-wide parts.  gfx950 only.
#pragma once
#include <math.h>

#include "common.hpp"

namespace sgv3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------
// host: descriptor checks and the window fields of the kernel parameters
// ------------------------------------------------------------------------------------------------
// csrc/vit.hip: sgv3d_vit_attention with an optional lse output (the same kernel body, the same bits of `out`), which
// sgv3d_vit_attention_lse of csrc/vit_grad.hip calls
int vit_attention_impl(const sgv3d_vit_attn_desc *desc, const float *qkv, const float *pad_qkv, const float *rel_pos_h,
                       const float *rel_pos_w, float *out, float *lse, void *stream);

// The checks every attention entry makes of its descriptor, under the entry's name.  `vec`: the multiple of heads * head_dim the
// entry's vector accesses need (0: none beyond head_dim's own).
static inline int check_attn_desc(const char *who, const sgv3d_vit_attn_desc *desc, int vec) {
    if (!desc) return fail(SGV3D_EINVAL, "%s: null descriptor", who);
    const sgv3d_vit_attn_desc &d = *desc;
    if (!(d.batch > 0 && d.height > 0 && d.width > 0 && d.heads > 0 && d.head_dim > 0 && d.win_h > 0 && d.win_w > 0))
        return fail(SGV3D_EINVAL, "%s: zero or negative dimension (batch %d, map %d x %d, heads %d, head_dim %d, window %d x %d)", who,
                    d.batch, d.height, d.width, d.heads, d.head_dim, d.win_h, d.win_w);
    const long long channels = (long long)d.heads * d.head_dim;
    if (vec && channels % vec != 0) return fail(SGV3D_EINVAL, "%s: heads * head_dim = %lld is not a multiple of %d", who, channels, vec);
    if (!(d.head_dim == 32 || d.head_dim == 64 || d.head_dim == 80))
        return fail(SGV3D_EINVAL, "%s: head_dim %d is not one of 32, 64, 80", who, d.head_dim);
    if (!(d.win_h <= 128 && d.win_w <= 128)) return fail(SGV3D_EINVAL, "%s: window %d x %d exceeds 128", who, d.win_h, d.win_w);
    if (!(3 * channels < (1LL << 24))) return fail(SGV3D_EINVAL, "%s: heads * head_dim too large", who);
    return SGV3D_OK;
}

// B, H, W, nH, win_h, win_w, nwy, nwx, T, inv_win_w of AttnParams (both) and BwdParams
template <class P>
static inline void fill_window(P &p, const sgv3d_vit_attn_desc &d) {
    p.B = d.batch, p.H = d.height, p.W = d.width, p.nH = d.heads, p.win_h = d.win_h, p.win_w = d.win_w;
    p.nwy = cdiv(d.height, d.win_h), p.nwx = cdiv(d.width, d.win_w);
    p.T = d.win_h * d.win_w;
    p.inv_win_w = 1.0f / (float)d.win_w;
}

// LDS row of a [query][kh] or [query][kw] table: odd, so the four lanes of a query and its 15 neighbours spread over the banks
static inline int odd_ld(bool rel, int win) { return rel ? (win | 1) : 0; }

static inline float softmax_scale(int head_dim) { return 1.0f / sqrtf((float)head_dim); }

// ------------------------------------------------------------------------------------------------
// device: window geometry
// ------------------------------------------------------------------------------------------------
// t / win_w without the integer division: exact for t < 128 * win_w, win_w <= 128 (every case is enumerated in
// tests/test_sam_encoder_cpu.py)
__device__ __forceinline__ int slot_row(int t, float inv_win_w) { return (int)(((float)t + 0.5f) * inv_win_w); }

// One (image, head, window) and, in the forward kernels, the query tile of it that a workgroup owns.
struct Window {
    int b, head, h0, w0, qt;

    // whether the window's token (kh, kw) lies on the map (false: a padding token), and then its pixel index (b * H + h) * W + w
    template <class P>
    __device__ __forceinline__ bool pixel(const P &p, int kh, int kw, long long &pix) const {
        const int h = h0 + kh, w = w0 + kw;
        if (!(h < p.H && w < p.W)) return false;
        pix = ((long long)b * p.H + h) * p.W + w;
        return true;
    }
};

// g = ((image * nH + head) * nwy + wy) * nwx + wx
template <class P, class I>
__device__ __forceinline__ Window decode_window(const P &p, I g) {
    Window r;
    const int wx = (int)(g % p.nwx);
    g /= p.nwx;
    const int wy = (int)(g % p.nwy);
    g /= p.nwy;
    r.head = (int)(g % p.nH);
    r.b = (int)(g / p.nH);
    r.h0 = wy * p.win_h, r.w0 = wx * p.win_w;
    r.qt = 0;
    return r;
}

// The forward kernels: workgroup id -> (window, query tile), the query tile fastest.  Workgroups are renumbered so that each of
// the 8 XCDs, which take consecutive workgroup ids in turn, walks a contiguous run: the query tiles that share a head's K and V
// then share an L2.
template <class P>
__device__ __forceinline__ Window decode_workgroup(const P &p) {
    int bid = blockIdx.x;
    const int per_xcd = gridDim.x / 8;
    if (bid < 8 * per_xcd) bid = (bid & 7) * per_xcd + (bid >> 3);     // (the last gridDim.x % 8 ids stay)
    const int qt = bid % p.nqt;
    Window r = decode_window(p, bid / p.nqt);
    r.qt = qt;
    return r;
}

// ------------------------------------------------------------------------------------------------
// device: LayerNorm row statistics, one wave per row
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

struct LnStats {
    double mean;
    float rstd;
};

// Two passes, never E[x^2] - E[x]^2.  The sums are carried in f64: the test's bar is relative to |x_hat| element by element, and
// a mean rounded to f32 is off by up to half an ulp OF THE MEAN -- for a row that sits at 1e4 with unit spread that alone is
// 5e-4 on every x_hat, whatever its size.  With the f64 mean, x - mean is rounded once, relative to itself.
__device__ __forceinline__ LnStats ln_row_stats(const f32x4 *xr, int c4, int lane, float eps) {
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
    return LnStats{mean, (float)(1.0 / sqrt(wave_sum(sq) * inv_c + (double)eps))};
}

__device__ __forceinline__ float ln_xhat(float v, const LnStats &st) { return (float)((double)v - st.mean) * st.rstd; }

// ------------------------------------------------------------------------------------------------
// device: GELU (erf form)
// ------------------------------------------------------------------------------------------------
// 1 + erf(x / sqrt 2) = 2 Phi(x).  For x < 0 it is written erfc(-z): no cancellation in the left tail.
__device__ __forceinline__ float gelu_erf_term(float x) {
    const float z = x * 0.70710678118654752440f;
    return x < 0.f ? erfcf(-z) : 1.0f + erff(z);
}

__device__ __forceinline__ float gelu1(float x) { return 0.5f * x * gelu_erf_term(x); }

// ------------------------------------------------------------------------------------------------
// device: f32 MFMA operands over the head dimension (v_mfma_f32_16x16x4_f32, lq = lane & 15, g = lane >> 4)
// ------------------------------------------------------------------------------------------------
// The HD / 16 accumulators of a transposed product acc^T[d][column] are fed four, two and one at a time: accumulator 4 c + i holds
// d = 64 c + 4 lq + i in row lq, so one 16-byte read of a row's [64 c + 4 lq] feeds four MFMAs; a 32- or 16-wide rest of the head
// dimension takes 8- and 4-byte reads the same way.
template <int HD>
struct HeadSplit {
    static constexpr int NJ = HD / 16;                                  // accumulators
    static constexpr int N4 = NJ / 4, N2 = (NJ % 4) / 2, N1 = NJ % 2;   // ... fed four, two and one at a time
    static constexpr int D2 = 64 * N4, D1 = D2 + 32 * N2;               // where the 8- and 4-byte parts of the head dimension begin
};

// acc^T[d][column] += sum over the 64 rows of an LDS tile M (rows of LD floats) of M[row][d] * Wt[row][column], where Wt holds the
// rows 4 g + r of each 16-row sub-tile in register r, as the accumulators of a 16x16 product stand.  mbase = M + 4 g LD: the
// lane group's first row.  (lq by reference, as the loops this replaces had it: by value the compiler forms one address of
// the backward's prologue in two instructions where it took one.)
template <int HD, int LD>
__device__ __forceinline__ void accum_rows(f32x4 (&acc)[HD / 16], const float *mbase, const f32x4 (&Wt)[4], const int &lq) {
    typedef HeadSplit<HD> HS;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float *mrow = mbase + (sub * 16 + r) * LD;
            const float wk = Wt[sub][r];
#pragma unroll
            for (int c = 0; c < HS::N4; ++c) {
                const f32x4 mf = *reinterpret_cast<const f32x4 *>(mrow + 64 * c + 4 * lq);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[4 * c + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(mf[i], wk, acc[4 * c + i], 0, 0, 0);
            }
            if (HS::N2) {
                const f32x2 mf = *reinterpret_cast<const f32x2 *>(mrow + HS::D2 + 2 * lq);
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    acc[4 * HS::N4 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(mf[i], wk, acc[4 * HS::N4 + i], 0, 0, 0);
            }
            if (HS::N1) acc[HS::NJ - 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(mrow[HS::D1 + lq], wk, acc[HS::NJ - 1], 0, 0, 0);
        }
}

// The lane's column of acc^T as a row dst[d] of HD floats, every element through f.  Row 4 g + r of accumulator 4 c + i is
// d = 64 c + 4 (4 g + r) + i: sixteen consecutive floats per lane and c.
template <int HD, class F>
__device__ __forceinline__ void store_rows(float *dst, const f32x4 (&acc)[HD / 16], int g, F f) {
    typedef HeadSplit<HD> HS;
#pragma unroll
    for (int c = 0; c < HS::N4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 v = {f(acc[4 * c][r]), f(acc[4 * c + 1][r]), f(acc[4 * c + 2][r]), f(acc[4 * c + 3][r])};
            *reinterpret_cast<f32x4 *>(dst + 64 * c + 16 * g + 4 * r) = v;
        }
    if (HS::N2) {      // d = D2 + 2 (4 g + r) + i
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
            const f32x4 v = {f(acc[4 * HS::N4][r]), f(acc[4 * HS::N4 + 1][r]), f(acc[4 * HS::N4][r + 1]), f(acc[4 * HS::N4 + 1][r + 1])};
            *reinterpret_cast<f32x4 *>(dst + HS::D2 + 8 * g + 2 * r) = v;
        }
    }
    if (HS::N1) {      // d = D1 + 4 g + r
        const f32x4 v = {f(acc[HS::NJ - 1][0]), f(acc[HS::NJ - 1][1]), f(acc[HS::NJ - 1][2]), f(acc[HS::NJ - 1][3])};
        *reinterpret_cast<f32x4 *>(dst + HS::D1 + 4 * g) = v;
    }
}

}  // namespace sgv3d
