// SAM's prompt encoder and mask decoder (the segment_anything package the reference's scripts/data_preprocess import), the
// parts that are not a linear layer, a transposed convolution, a LayerNorm or a GELU:
//   sgv3d_sam_attention       softmax(q k^T scale) v where one side has at most 16 rows (the decoder's token side)
//   sgv3d_sam_prompt_tokens   [iou_token, mask_tokens, box corner encodings] of every box in one launch
//   sgv3d_sam_dense_pe        PositionEmbeddingRandom over the grid, NHWC
//   sgv3d_sam_gather_add      src[b] = image_embedding[frame of box b] + no_mask_embed (the embedding is read by index)
//   sgv3d_sam_hyper_product   masks[b, i] = sum_c hyper[b, i, c] upscaled[b, :, c]: the "weights" are activations per box
//   sgv3d_sam_mask_compose    low-res logits -> class-id image (or per-box masks): both bilinear resizes of postprocess_masks
//                             composed into 16 taps per output pixel, no [B, S, S] or [B, H, W] float map in between
//   sgv3d_resize_u8_filter    Pillow's two integer passes (any sgv3d_resample_coeffs_filter table) u8 HWC -> f32 CHW
// gfx950 only.  Vector stores only, no atomics: every kernel is repeatable bit for bit.  The compose arithmetic is float64
// and shared, function by function, with sgv3d_sam_mask_compose_host (built with -ffp-contract=off).
#include <math.h>

#include <cmath>
#include <vector>

#include "common.hpp"

using namespace sgv3d;

#define HD_FN __host__ __device__ inline

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;
constexpr int kSmall = 16;     // the small side of sgv3d_sam_attention: at most this many rows
constexpr int kChunk = 256;    // keys per workgroup of the few-queries kernel: one per thread
constexpr int kPrecision = 22; // Pillow's PRECISION_BITS for 8-bit images

// ------------------------------------------------------------------------------------------------
// attention with one small side
// ------------------------------------------------------------------------------------------------
struct SamAttnParams {
    int B, nq, nk, heads, q_ld, k_ld, v_ld, o_ld, splits;
    float scale;
    const float *q, *k, *v;
    float *out, *part;
};

template <int HD>
__device__ inline void load_row(const float *p, float (&r)[HD]) {
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(p)[c];
        r[4 * c] = v.x, r[4 * c + 1] = v.y, r[4 * c + 2] = v.z, r[4 * c + 3] = v.w;
    }
}

// Few queries (nq <= 16) on many keys: workgroup (split, head, image) owns 256 consecutive keys.  Thread t forms the logits of
// key t for every query (its K row in registers, the queries broadcast from LDS); wave w turns the LDS rows of queries w, w + 4,
// .. into exp(s - max) and their sum; then thread (d = t % HD, g = t / HD) sums p v[., d] over the keys g, g + G, .. for every
// query, so each V row is read once, in full 64- or 128-byte rows; the G partial sums meet in LDS in the order g = 0, 1, ...
// One split: the result is written.  More: (sum, max, weight sum) go to the workspace and sam_attn_combine_kernel joins them.
template <int HD>
__global__ __launch_bounds__(kBlock) void sam_attn_fewq_kernel(SamAttnParams p) {
    constexpr int G = kBlock / HD;
    __shared__ float sq[kSmall * HD];
    __shared__ float ss[kSmall][kChunk];
    __shared__ float red[G][kSmall][HD];
    __shared__ float sm[kSmall], sl[kSmall];
    const int split = blockIdx.x, head = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const int k0 = split * kChunk;
    const int nvalid = min(kChunk, p.nk - k0);
    for (int i = t; i < p.nq * HD; i += kBlock)
        sq[i] = p.q[((size_t)b * p.nq + i / HD) * p.q_ld + head * HD + i % HD];
    __syncthreads();
    if (t < nvalid) {
        float kr[HD];
        load_row<HD>(p.k + ((size_t)b * p.nk + k0 + t) * p.k_ld + head * HD, kr);
        for (int qi = 0; qi < p.nq; ++qi) {
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) dot = fmaf(sq[qi * HD + d], kr[d], dot);
            ss[qi][t] = dot * p.scale;
        }
    } else {
        for (int qi = 0; qi < p.nq; ++qi) ss[qi][t] = -INFINITY;
    }
    __syncthreads();
    const int wave = t / kWave, lane = t % kWave;
    for (int qi = wave; qi < kSmall; qi += kBlock / kWave) {
        if (qi >= p.nq) {                      // rows the product below multiplies by: exact zeros
#pragma unroll
            for (int j = 0; j < kChunk / kWave; ++j) ss[qi][lane + kWave * j] = 0.f;
            continue;
        }
        float v[kChunk / kWave];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < kChunk / kWave; ++j) {
            v[j] = ss[qi][lane + kWave * j];
            m = fmaxf(m, v[j]);
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kChunk / kWave; ++j) {
            const float e = expf(v[j] - m);    // the chunk holds a key, so m is finite; a padding slot gives exp(-inf) = 0
            ss[qi][lane + kWave * j] = e;
            sum += e;
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
        if (lane == 0) sm[qi] = m, sl[qi] = sum;
    }
    __syncthreads();
    const int d = t % HD, g = t / HD;
    float acc[kSmall];
#pragma unroll
    for (int qi = 0; qi < kSmall; ++qi) acc[qi] = 0.f;
    const float *vp = p.v + ((size_t)b * p.nk + k0) * p.v_ld + head * HD + d;
    for (int j = g; j < nvalid; j += G) {
        const float vv = vp[(size_t)j * p.v_ld];
#pragma unroll
        for (int qi = 0; qi < kSmall; ++qi) acc[qi] = fmaf(ss[qi][j], vv, acc[qi]);
    }
#pragma unroll
    for (int qi = 0; qi < kSmall; ++qi) red[g][qi][d] = acc[qi];
    __syncthreads();
    for (int o = t; o < p.nq * HD; o += kBlock) {
        const int qi = o / HD, dd = o % HD;
        float s = 0.f;
#pragma unroll
        for (int gg = 0; gg < G; ++gg) s += red[gg][qi][dd];
        if (p.splits == 1) {
            p.out[((size_t)b * p.nq + qi) * p.o_ld + head * HD + dd] = s / sl[qi];
        } else {
            float *w = p.part + ((((size_t)b * p.heads + head) * p.splits + split) * kSmall + qi) * (HD + 2);
            w[dd] = s;
            if (dd == 0) w[HD] = sm[qi], w[HD + 1] = sl[qi];
        }
    }
}

// The online-softmax combine of the splits, in split order: one thread per output value.
template <int HD>
__global__ __launch_bounds__(kBlock) void sam_attn_combine_kernel(SamAttnParams p) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const long long total = (long long)p.B * p.heads * p.nq * HD;
    if (i >= total) return;
    const int d = (int)(i % HD), qi = (int)(i / HD % p.nq), head = (int)(i / HD / p.nq % p.heads), b = (int)(i / HD / p.nq / p.heads);
    const float *w = p.part + ((((size_t)b * p.heads + head) * p.splits) * kSmall + qi) * (HD + 2);
    const size_t step = (size_t)kSmall * (HD + 2);
    float m = -INFINITY;
    for (int s = 0; s < p.splits; ++s) m = fmaxf(m, w[s * step + HD]);
    float num = 0.f, den = 0.f;
    for (int s = 0; s < p.splits; ++s) {
        const float e = expf(w[s * step + HD] - m);
        num = fmaf(w[s * step + d], e, num);
        den = fmaf(w[s * step + HD + 1], e, den);
    }
    p.out[((size_t)b * p.nq + qi) * p.o_ld + head * HD + d] = num / den;
}

// Many queries on few keys (nk <= 16): K and V of one (image, head) sit in LDS, one query per lane, its row, its logits and
// its output in registers; every query row is read once and every output row written once, 16 bytes at a time.
template <int HD>
__global__ __launch_bounds__(kBlock) void sam_attn_fewk_kernel(SamAttnParams p) {
    __shared__ float sk[kSmall * HD], sv[kSmall * HD];
    const int head = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    for (int i = t; i < p.nk * HD; i += kBlock) {
        const size_t row = (size_t)b * p.nk + i / HD;
        sk[i] = p.k[row * p.k_ld + head * HD + i % HD];
        sv[i] = p.v[row * p.v_ld + head * HD + i % HD];
    }
    __syncthreads();
    const long long qi = (long long)blockIdx.x * kBlock + t;
    if (qi >= p.nq) return;
    float qr[HD];
    load_row<HD>(p.q + ((size_t)b * p.nq + qi) * p.q_ld + head * HD, qr);
    float s[kSmall];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < kSmall; ++j) {
        s[j] = -INFINITY;
        if (j < p.nk) {
            float dot = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) dot = fmaf(qr[d], sk[j * HD + d], dot);
            s[j] = dot * p.scale;
            m = fmaxf(m, s[j]);
        }
    }
    float acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < kSmall; ++j) {
        if (j < p.nk) {
            const float e = expf(s[j] - m);
            l += e;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = fmaf(e, sv[j * HD + d], acc[d]);
        }
    }
    f32x4 *o = reinterpret_cast<f32x4 *>(p.out + ((size_t)b * p.nq + qi) * p.o_ld + head * HD);
#pragma unroll
    for (int c = 0; c < HD / 4; ++c) {
        f32x4 v;
        v.x = acc[4 * c] / l, v.y = acc[4 * c + 1] / l, v.z = acc[4 * c + 2] / l, v.w = acc[4 * c + 3] / l;
        o[c] = v;
    }
}

int sam_attn_check(const sgv3d_sam_attn_desc *desc) {
    SGV3D_REQUIRE(desc, "sam_attention: null descriptor");
    const sgv3d_sam_attn_desc &d = *desc;
    SGV3D_REQUIRE(d.batch > 0 && d.nq > 0 && d.nk > 0 && d.heads > 0 && d.head_dim > 0,
                  "sam_attention: zero or negative dimension (batch %d, nq %d, nk %d, heads %d, head_dim %d)", d.batch, d.nq, d.nk,
                  d.heads, d.head_dim);
    SGV3D_REQUIRE(d.head_dim == 16 || d.head_dim == 32, "sam_attention: head_dim %d is not one of 16, 32", d.head_dim);
    SGV3D_REQUIRE(d.nq <= kSmall || d.nk <= kSmall, "sam_attention: neither side is small (nq %d, nk %d, at most %d on one)", d.nq,
                  d.nk, kSmall);
    SGV3D_REQUIRE(d.heads <= 65535 && d.batch <= 65535, "sam_attention: heads %d or batch %d above 65535", d.heads, d.batch);
    const long long c = (long long)d.heads * d.head_dim;
    SGV3D_REQUIRE(d.q_ld >= c && d.k_ld >= c && d.v_ld >= c && d.o_ld >= c,
                  "sam_attention: a row stride (q %d, k %d, v %d, out %d) is below heads * head_dim = %lld", d.q_ld, d.k_ld, d.v_ld,
                  d.o_ld, c);
    SGV3D_REQUIRE(d.q_ld % 4 == 0 && d.k_ld % 4 == 0 && d.v_ld % 4 == 0 && d.o_ld % 4 == 0,
                  "sam_attention: row strides (q %d, k %d, v %d, out %d) must be multiples of 4", d.q_ld, d.k_ld, d.v_ld, d.o_ld);
    SGV3D_REQUIRE(std::isfinite(d.scale), "sam_attention: scale is not finite");
    return SGV3D_OK;
}

size_t sam_attn_workspace(const sgv3d_sam_attn_desc &d) {
    if (d.nk <= kSmall) return 0;
    const int splits = cdiv(d.nk, kChunk);
    return splits == 1 ? 0 : (size_t)d.batch * d.heads * splits * kSmall * (d.head_dim + 2) * sizeof(float);
}

template <int HD>
int sam_attn_launch(const SamAttnParams &p, hipStream_t st) {
    if (p.nk <= kSmall) {
        hipLaunchKernelGGL(sam_attn_fewk_kernel<HD>, dim3(cdiv(p.nq, kBlock), p.heads, p.B), dim3(kBlock), 0, st, p);
        return check_launch("sam_attn_fewk_kernel");
    }
    hipLaunchKernelGGL(sam_attn_fewq_kernel<HD>, dim3(p.splits, p.heads, p.B), dim3(kBlock), 0, st, p);
    if (int rc = check_launch("sam_attn_fewq_kernel")) return rc;
    if (p.splits == 1) return SGV3D_OK;
    const long long total = (long long)p.B * p.heads * p.nq * HD;
    hipLaunchKernelGGL(sam_attn_combine_kernel<HD>, dim3(cdiv(total, kBlock)), dim3(kBlock), 0, st, p);
    return check_launch("sam_attn_combine_kernel");
}

// ------------------------------------------------------------------------------------------------
// prompt encoder
// ------------------------------------------------------------------------------------------------
// PositionEmbeddingRandom._pe_encoding of one point in [0, 1]^2, channel c of dim: z = (2 x - 1) G[0][j] + (2 y - 1) G[1][j],
// j = c mod dim / 2; sin(2 pi z) below dim / 2, cos above.  Evaluated in f64 and rounded once.
__device__ inline float pe_value(double x, double y, const float *gauss, int half, int c) {
    const int j = c < half ? c : c - half;
    const double z = (2.0 * x - 1.0) * (double)gauss[j] + (2.0 * y - 1.0) * (double)gauss[half + j];
    const double a = 2.0 * M_PI * z;
    return (float)(c < half ? sin(a) : cos(a));
}

__global__ __launch_bounds__(kBlock) void sam_prompt_tokens_kernel(int boxes, int dim, const float *box, double in_h, double in_w,
                                                                   const float *gauss, const float *corner0, const float *corner1,
                                                                   const float *iou_token, const float *mask_tokens, float *tokens) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)boxes * 7 * dim) return;
    const int c = (int)(i % dim), r = (int)(i / dim % 7), b = (int)(i / dim / 7);
    float v;
    if (r == 0) {
        v = iou_token[c];
    } else if (r < 5) {
        v = mask_tokens[(r - 1) * dim + c];
    } else {
        const int k = r - 5;
        const double x = ((double)box[4 * b + 2 * k] + 0.5) / in_w, y = ((double)box[4 * b + 2 * k + 1] + 0.5) / in_h;
        v = pe_value(x, y, gauss, dim / 2, c) + (k ? corner1[c] : corner0[c]);
    }
    tokens[i] = v;
}

__global__ __launch_bounds__(kBlock) void sam_dense_pe_kernel(int h, int w, int dim, const float *gauss, float *pe) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)h * w * dim) return;
    const int c = (int)(i % dim), x = (int)(i / dim % w), y = (int)(i / dim / w);
    pe[i] = pe_value((x + 0.5) / w, (y + 0.5) / h, gauss, dim / 2, c);
}

__global__ __launch_bounds__(kBlock) void sam_gather_add_kernel(int boxes, int frames, long long row4, int c4, const f32x4 *emb,
                                                                const int32_t *frame_of_box, const f32x4 *vec, f32x4 *out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= boxes * row4) return;
    const int b = (int)(i / row4);
    const long long r = i % row4;
    const int f = min(max(frame_of_box[b], 0), frames - 1);     // the caller checked the indices; never read outside
    out[i] = emb[f * row4 + r] + vec[r % c4];
}

// out[b, i, p] = sum_c hyper[b, i, c] up[b, p, c]: one thread per pixel, its row of `channels` floats read 16 bytes at a time,
// the at most 4 hypernetwork rows of the box in LDS.
__global__ __launch_bounds__(kBlock) void sam_hyper_product_kernel(long long pixels, int channels, int n, int hyper_ld, const float *hyper,
                                                                   const float *up, float *out) {
    extern __shared__ float sh[];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < n * channels; i += kBlock) sh[i] = hyper[(size_t)b * hyper_ld + i];
    __syncthreads();
    const long long px = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (px >= pixels) return;
    const f32x4 *row = reinterpret_cast<const f32x4 *>(up + ((size_t)b * pixels + px) * channels);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < channels / 4; ++c) {
        const f32x4 v = row[c];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < n) {
                const float *h = sh + i * channels + 4 * c;
                acc[i] = fmaf(v.w, h[3], fmaf(v.z, h[2], fmaf(v.y, h[1], fmaf(v.x, h[0], acc[i]))));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < n) out[((size_t)b * n + i) * pixels + px] = acc[i];
}

// ------------------------------------------------------------------------------------------------
// postprocess_masks composed: lowres [low, low] -> bilinear to [size, size] -> crop [pre] -> bilinear to [out]
// ------------------------------------------------------------------------------------------------
// One axis.  F.interpolate(align_corners=False): source position max(0, scale (o + 0.5) - 0.5) with scale = in / out, the
// upper neighbour clamped.  Output o of the second resize reads a0, a1 of the cropped square map; each of those reads two
// low-res entries: four (index, weight) pairs per axis, 16 taps per pixel.
HD_FN void lerp_axis(int o, int in, int out, int *i0, int *i1, double *l) {
    double s = ((double)in / (double)out) * ((double)o + 0.5) - 0.5;
    if (s < 0.0) s = 0.0;
    int a = (int)s;
    if (a > in - 1) a = in - 1;
    *i0 = a;
    *i1 = a + 1 < in ? a + 1 : in - 1;
    *l = s - (double)a;
}

HD_FN void compose_axis(int o, int out, int pre, int size, int low, int idx[4], double w[4]) {
    int a0, a1;
    double l1;
    lerp_axis(o, pre, out, &a0, &a1, &l1);
    const int a[2] = {a0, a1};
    const double wa[2] = {1.0 - l1, l1};
    for (int k = 0; k < 2; ++k) {
        int b0, b1;
        double l2;
        lerp_axis(a[k], low, size, &b0, &b1, &l2);
        idx[2 * k] = b0, idx[2 * k + 1] = b1;
        w[2 * k] = wa[k] * (1.0 - l2), w[2 * k + 1] = wa[k] * l2;
    }
}

HD_FN double compose_pixel(const float *logit, int low, const int *iy, const double *wy, const int *ix, const double *wx) {
    double v = 0.0;
    for (int i = 0; i < 4; ++i) {
        const float *row = logit + (size_t)iy[i] * low;
        double r = 0.0;
        for (int j = 0; j < 4; ++j) r += wx[j] * (double)row[ix[j]];
        v += wy[i] * r;
    }
    return v;
}

// get_sam_mask's paint loop for one pixel given the boxes' values there: the first box that covers the pixel with a non-zero
// label owns it (mask_image += mask * label * (mask_image == 0)), then np.clip(., 0, 6).
HD_FN bool paint(int label, double v, uint8_t *cls) {
    if (!(v > 0.0) || label == 0) return false;
    *cls = (uint8_t)(label < 0 ? 0 : (label > 6 ? 6 : label));
    return true;
}

struct ComposeParams {
    int mode, boxes, frames, low, size, pre_h, pre_w, out_h, out_w;
    const float *logits;
    const int32_t *labels, *frame_of_box;
    void *out;
    double *wy, *wx;   // [out_h][4], [out_w][4]
    int *iy, *ix;
};

struct ComposeTables {
    size_t wy, wx, iy, ix, total;
};
ComposeTables compose_tables(int out_h, int out_w) {
    ComposeTables t;
    t.wy = 0;
    t.wx = t.wy + (size_t)out_h * 4 * sizeof(double);
    t.iy = t.wx + (size_t)out_w * 4 * sizeof(double);
    t.ix = t.iy + (size_t)out_h * 4 * sizeof(int);
    t.total = (t.ix + (size_t)out_w * 4 * sizeof(int) + 255) / 256 * 256;
    return t;
}

__global__ __launch_bounds__(kBlock) void compose_tables_kernel(ComposeParams p) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int idx[4];
    double w[4];
    if (i < p.out_h) {
        compose_axis(i, p.out_h, p.pre_h, p.size, p.low, idx, w);
        for (int k = 0; k < 4; ++k) p.iy[4 * i + k] = idx[k], p.wy[4 * i + k] = w[k];
    } else if (i < p.out_h + p.out_w) {
        const int x = i - p.out_h;
        compose_axis(x, p.out_w, p.pre_w, p.size, p.low, idx, w);
        for (int k = 0; k < 4; ++k) p.ix[4 * x + k] = idx[k], p.wx[4 * x + k] = w[k];
    }
}

// mode CLASS: one thread per pixel of [frames, out_h, out_w]; it walks the boxes in order, evaluates those of its frame and stops
// at the first that paints.  Modes BOOL / LOGIT: one thread per pixel of [boxes, out_h, out_w].
__global__ __launch_bounds__(kBlock) void compose_kernel(ComposeParams p) {
    const int x = blockIdx.x * 64 + threadIdx.x % 64, y = blockIdx.y * 4 + threadIdx.x / 64, z = blockIdx.z;
    if (x >= p.out_w || y >= p.out_h) return;
    int iy[4], ix[4];
    double wy[4], wx[4];
    for (int k = 0; k < 4; ++k) iy[k] = p.iy[4 * y + k], wy[k] = p.wy[4 * y + k], ix[k] = p.ix[4 * x + k], wx[k] = p.wx[4 * x + k];
    const size_t px = ((size_t)z * p.out_h + y) * p.out_w + x, lowpx = (size_t)p.low * p.low;
    if (p.mode == SGV3D_SAM_COMPOSE_CLASS) {
        uint8_t cls = 0;
        for (int b = 0; b < p.boxes; ++b) {
            if (p.frame_of_box[b] != z) continue;
            if (paint(p.labels[b], compose_pixel(p.logits + b * lowpx, p.low, iy, wy, ix, wx), &cls)) break;
        }
        static_cast<uint8_t *>(p.out)[px] = cls;
    } else {
        const double v = compose_pixel(p.logits + z * lowpx, p.low, iy, wy, ix, wx);
        if (p.mode == SGV3D_SAM_COMPOSE_BOOL)
            static_cast<uint8_t *>(p.out)[px] = v > 0.0 ? 1 : 0;
        else
            static_cast<float *>(p.out)[px] = (float)v;
    }
}

int compose_check(int mode, int boxes, int frames, int low, int size, int pre_h, int pre_w, int out_h, int out_w, const float *logits,
                  const int32_t *labels, const int32_t *frame_of_box, const void *out) {
    SGV3D_REQUIRE(mode == SGV3D_SAM_COMPOSE_CLASS || mode == SGV3D_SAM_COMPOSE_BOOL || mode == SGV3D_SAM_COMPOSE_LOGIT,
                  "sam_mask_compose: unknown mode %d", mode);
    SGV3D_REQUIRE(boxes >= 0 && frames > 0, "sam_mask_compose: negative box count %d or non-positive frame count %d", boxes, frames);
    SGV3D_REQUIRE(mode == SGV3D_SAM_COMPOSE_CLASS || boxes > 0, "sam_mask_compose: the per-box modes need at least one box");
    SGV3D_REQUIRE(low > 0 && size > 0 && pre_h > 0 && pre_w > 0 && out_h > 0 && out_w > 0,
                  "sam_mask_compose: non-positive size (low %d, size %d, preprocess %d x %d, output %d x %d)", low, size, pre_h, pre_w,
                  out_h, out_w);
    SGV3D_REQUIRE(pre_h <= size && pre_w <= size, "sam_mask_compose: the preprocess shape %d x %d exceeds the square %d", pre_h, pre_w, size);
    SGV3D_REQUIRE(low <= 32768 && out_h <= 65535 * 4, "sam_mask_compose: low %d or out_h %d too large", low, out_h);
    SGV3D_REQUIRE(boxes <= 65535 && frames <= 65535, "sam_mask_compose: boxes %d or frames %d above 65535", boxes, frames);
    SGV3D_REQUIRE(out, "sam_mask_compose: null output");
    SGV3D_REQUIRE(boxes == 0 || logits, "sam_mask_compose: null logits");
    SGV3D_REQUIRE(mode != SGV3D_SAM_COMPOSE_CLASS || boxes == 0 || (labels && frame_of_box), "sam_mask_compose: null labels or frame_of_box");
    return SGV3D_OK;
}

// ------------------------------------------------------------------------------------------------
// Pillow's resize with a coefficient table: horizontal pass u8 -> u8, vertical pass u8 -> f32 CHW
// ------------------------------------------------------------------------------------------------
__device__ inline int clip8(int acc) {
    const int v = acc >> kPrecision;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(kBlock) void resize_u8_h_kernel(int in_h, int in_w, int out_w, const int32_t *bounds, const int32_t *coeffs,
                                                             int ksize, const uint8_t *src, uint8_t *tmp) {
    const int x = blockIdx.x * 64 + threadIdx.x % 64, y = blockIdx.y * 4 + threadIdx.x / 64, f = blockIdx.z;
    if (x >= out_w || y >= in_h) return;
    const int x0 = bounds[2 * x], n = min(bounds[2 * x + 1], ksize);
    const int32_t *k = coeffs + (size_t)x * ksize;
    const uint8_t *row = src + ((size_t)f * in_h + y) * in_w * 3;
    int acc[3] = {1 << (kPrecision - 1), 1 << (kPrecision - 1), 1 << (kPrecision - 1)};
    for (int t = 0; t < n; ++t) {
        const int xs = min(max(x0 + t, 0), in_w - 1);
        const int wk = k[t];
        for (int c = 0; c < 3; ++c) acc[c] += (int)row[(size_t)xs * 3 + c] * wk;
    }
    uint8_t *o = tmp + (((size_t)f * in_h + y) * out_w + x) * 3;
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)clip8(acc[c]);
}

__global__ __launch_bounds__(kBlock) void resize_u8_v_kernel(int in_h, int out_h, int out_w, const int32_t *bounds, const int32_t *coeffs,
                                                             int ksize, int swap_rb, const uint8_t *tmp, float *dst) {
    const int x = blockIdx.x * 64 + threadIdx.x % 64, y = blockIdx.y * 4 + threadIdx.x / 64, f = blockIdx.z;
    if (x >= out_w || y >= out_h) return;
    const int y0 = bounds[2 * y], n = min(bounds[2 * y + 1], ksize);
    const int32_t *k = coeffs + (size_t)y * ksize;
    const uint8_t *col = tmp + ((size_t)f * in_h * out_w + x) * 3;
    int acc[3] = {1 << (kPrecision - 1), 1 << (kPrecision - 1), 1 << (kPrecision - 1)};
    for (int t = 0; t < n; ++t) {
        const int ys = min(max(y0 + t, 0), in_h - 1);
        const int wk = k[t];
        for (int c = 0; c < 3; ++c) acc[c] += (int)col[(size_t)ys * out_w * 3 + c] * wk;
    }
    for (int c = 0; c < 3; ++c)
        dst[(((size_t)f * 3 + (swap_rb ? 2 - c : c)) * out_h + y) * out_w + x] = (float)clip8(acc[c]);
}

}  // namespace

extern "C" size_t sgv3d_sam_attention_workspace_bytes(const sgv3d_sam_attn_desc *desc) {
    if (sam_attn_check(desc) != SGV3D_OK) return 0;
    return sam_attn_workspace(*desc);
}

extern "C" int sgv3d_sam_attention(const sgv3d_sam_attn_desc *desc, const float *q, const float *k, const float *v, float *out,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = sam_attn_check(desc)) return rc;
    const sgv3d_sam_attn_desc &d = *desc;
    SGV3D_REQUIRE(q && k && v && out, "sam_attention: null q, k, v or out");
    SGV3D_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out), "sam_attention: q, k, v and out must be 16-byte aligned");
    const size_t need = sam_attn_workspace(d);
    SGV3D_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && aligned16(workspace)),
                  "sam_attention: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
    SamAttnParams p;
    p.B = d.batch, p.nq = d.nq, p.nk = d.nk, p.heads = d.heads;
    p.q_ld = d.q_ld, p.k_ld = d.k_ld, p.v_ld = d.v_ld, p.o_ld = d.o_ld;
    p.splits = d.nk <= kSmall ? 1 : cdiv(d.nk, kChunk);
    SGV3D_REQUIRE(p.splits <= 65535 * 32, "sam_attention: nk %d too large", d.nk);
    p.scale = d.scale;
    p.q = q, p.k = k, p.v = v, p.out = out, p.part = static_cast<float *>(workspace);
    return d.head_dim == 16 ? sam_attn_launch<16>(p, as_stream(stream)) : sam_attn_launch<32>(p, as_stream(stream));
}

extern "C" int sgv3d_sam_prompt_tokens(int boxes, int dim, int in_h, int in_w, const float *box, const float *gauss, const float *corner0,
                                       const float *corner1, const float *iou_token, const float *mask_tokens, float *tokens, void *stream) {
    SGV3D_REQUIRE(boxes > 0 && dim > 0 && in_h > 0 && in_w > 0, "sam_prompt_tokens: non-positive size (boxes %d, dim %d, input %d x %d)", boxes,
                  dim, in_h, in_w);
    SGV3D_REQUIRE(dim % 2 == 0, "sam_prompt_tokens: dim %d is odd", dim);
    SGV3D_REQUIRE(box && gauss && corner0 && corner1 && iou_token && mask_tokens && tokens, "sam_prompt_tokens: null pointer");
    const long long total = (long long)boxes * 7 * dim;
    SGV3D_REQUIRE(total < (1LL << 31), "sam_prompt_tokens: too many values");
    hipLaunchKernelGGL(sam_prompt_tokens_kernel, dim3(cdiv(total, kBlock)), dim3(kBlock), 0, as_stream(stream), boxes, dim, box, (double)in_h,
                       (double)in_w, gauss, corner0, corner1, iou_token, mask_tokens, tokens);
    return check_launch("sam_prompt_tokens_kernel");
}

extern "C" int sgv3d_sam_dense_pe(int h, int w, int dim, const float *gauss, float *pe, void *stream) {
    SGV3D_REQUIRE(h > 0 && w > 0 && dim > 0, "sam_dense_pe: non-positive size (%d x %d x %d)", h, w, dim);
    SGV3D_REQUIRE(dim % 2 == 0, "sam_dense_pe: dim %d is odd", dim);
    SGV3D_REQUIRE(gauss && pe, "sam_dense_pe: null pointer");
    const long long total = (long long)h * w * dim;
    SGV3D_REQUIRE(total < (1LL << 31), "sam_dense_pe: too many values");
    hipLaunchKernelGGL(sam_dense_pe_kernel, dim3(cdiv(total, kBlock)), dim3(kBlock), 0, as_stream(stream), h, w, dim, gauss, pe);
    return check_launch("sam_dense_pe_kernel");
}

extern "C" int sgv3d_sam_gather_add(int boxes, int frames, long long pixels, int channels, const float *emb, const int32_t *frame_of_box,
                                    const float *vec, float *out, void *stream) {
    SGV3D_REQUIRE(boxes > 0 && frames > 0 && pixels > 0 && channels > 0, "sam_gather_add: non-positive size (boxes %d, frames %d, pixels %lld, channels %d)",
                  boxes, frames, pixels, channels);
    SGV3D_REQUIRE(channels % 4 == 0, "sam_gather_add: channels %d is not a multiple of 4", channels);
    SGV3D_REQUIRE(emb && frame_of_box && vec && out, "sam_gather_add: null pointer");
    SGV3D_REQUIRE(aligned16(emb) && aligned16(vec) && aligned16(out), "sam_gather_add: emb, vec and out must be 16-byte aligned");
    const long long row4 = pixels * (channels / 4);
    const long long blocks = (boxes * row4 + kBlock - 1) / kBlock;
    SGV3D_REQUIRE(blocks < (1LL << 31), "sam_gather_add: too many values");
    hipLaunchKernelGGL(sam_gather_add_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), boxes, frames, row4, channels / 4,
                       reinterpret_cast<const f32x4 *>(emb), frame_of_box, reinterpret_cast<const f32x4 *>(vec), reinterpret_cast<f32x4 *>(out));
    return check_launch("sam_gather_add_kernel");
}

extern "C" int sgv3d_sam_hyper_product(int boxes, long long pixels, int channels, int n, int hyper_ld, const float *hyper, const float *up,
                                       float *out, void *stream) {
    SGV3D_REQUIRE(boxes > 0 && pixels > 0 && channels > 0 && n > 0, "sam_hyper_product: non-positive size (boxes %d, pixels %lld, channels %d, n %d)",
                  boxes, pixels, channels, n);
    SGV3D_REQUIRE(n <= 4, "sam_hyper_product: n %d above 4", n);
    SGV3D_REQUIRE(channels % 4 == 0 && channels <= 1024, "sam_hyper_product: channels %d is not a multiple of 4 up to 1024", channels);
    SGV3D_REQUIRE(hyper_ld >= n * channels, "sam_hyper_product: hyper_ld %d below n * channels = %d", hyper_ld, n * channels);
    SGV3D_REQUIRE(boxes <= 65535, "sam_hyper_product: boxes %d above 65535", boxes);
    SGV3D_REQUIRE(hyper && up && out, "sam_hyper_product: null pointer");
    SGV3D_REQUIRE(aligned16(up), "sam_hyper_product: up must be 16-byte aligned");
    const long long bx = (pixels + kBlock - 1) / kBlock;
    SGV3D_REQUIRE(bx < (1LL << 31), "sam_hyper_product: too many pixels");
    hipLaunchKernelGGL(sam_hyper_product_kernel, dim3((unsigned)bx, boxes), dim3(kBlock), (size_t)n * channels * sizeof(float), as_stream(stream),
                       pixels, channels, n, hyper_ld, hyper, up, out);
    return check_launch("sam_hyper_product_kernel");
}

extern "C" size_t sgv3d_sam_mask_compose_workspace_bytes(int out_h, int out_w) {
    if (out_h <= 0 || out_w <= 0) return 0;
    return compose_tables(out_h, out_w).total;
}

extern "C" int sgv3d_sam_mask_compose(int mode, int boxes, int frames, int low, int size, int pre_h, int pre_w, int out_h, int out_w,
                                      const float *logits, const int32_t *labels, const int32_t *frame_of_box, void *out, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    if (int rc = compose_check(mode, boxes, frames, low, size, pre_h, pre_w, out_h, out_w, logits, labels, frame_of_box, out)) return rc;
    const ComposeTables t = compose_tables(out_h, out_w);
    SGV3D_REQUIRE(workspace && workspace_bytes >= t.total && aligned16(workspace), "sam_mask_compose: workspace of %zu bytes needed, %zu given",
                  t.total, workspace ? workspace_bytes : (size_t)0);
    SGV3D_REQUIRE(mode != SGV3D_SAM_COMPOSE_LOGIT || aligned16(out), "sam_mask_compose: out must be 16-byte aligned");
    ComposeParams p;
    p.mode = mode, p.boxes = boxes, p.frames = frames, p.low = low, p.size = size, p.pre_h = pre_h, p.pre_w = pre_w, p.out_h = out_h, p.out_w = out_w;
    p.logits = logits, p.labels = labels, p.frame_of_box = frame_of_box, p.out = out;
    char *ws = static_cast<char *>(workspace);
    p.wy = reinterpret_cast<double *>(ws + t.wy), p.wx = reinterpret_cast<double *>(ws + t.wx);
    p.iy = reinterpret_cast<int *>(ws + t.iy), p.ix = reinterpret_cast<int *>(ws + t.ix);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(compose_tables_kernel, dim3(cdiv(out_h + out_w, kBlock)), dim3(kBlock), 0, st, p);
    if (int rc = check_launch("compose_tables_kernel")) return rc;
    const int planes = mode == SGV3D_SAM_COMPOSE_CLASS ? frames : boxes;
    hipLaunchKernelGGL(compose_kernel, dim3(cdiv(out_w, 64), cdiv(out_h, 4), planes), dim3(kBlock), 0, st, p);
    return check_launch("compose_kernel");
}

extern "C" int sgv3d_sam_mask_compose_host(int mode, int boxes, int frames, int low, int size, int pre_h, int pre_w, int out_h, int out_w,
                                           const float *logits, const int32_t *labels, const int32_t *frame_of_box, void *out) {
    if (int rc = compose_check(mode, boxes, frames, low, size, pre_h, pre_w, out_h, out_w, logits, labels, frame_of_box, out)) return rc;
    std::vector<int> iy((size_t)out_h * 4), ix((size_t)out_w * 4);
    std::vector<double> wy((size_t)out_h * 4), wx((size_t)out_w * 4);
    for (int y = 0; y < out_h; ++y) compose_axis(y, out_h, pre_h, size, low, &iy[4 * (size_t)y], &wy[4 * (size_t)y]);
    for (int x = 0; x < out_w; ++x) compose_axis(x, out_w, pre_w, size, low, &ix[4 * (size_t)x], &wx[4 * (size_t)x]);
    const size_t lowpx = (size_t)low * low;
    const int planes = mode == SGV3D_SAM_COMPOSE_CLASS ? frames : boxes;
    for (int z = 0; z < planes; ++z)
        for (int y = 0; y < out_h; ++y)
            for (int x = 0; x < out_w; ++x) {
                const size_t px = ((size_t)z * out_h + y) * out_w + x;
                const int *py = &iy[4 * (size_t)y], *pxi = &ix[4 * (size_t)x];
                const double *qy = &wy[4 * (size_t)y], *qx = &wx[4 * (size_t)x];
                if (mode == SGV3D_SAM_COMPOSE_CLASS) {
                    uint8_t cls = 0;
                    for (int b = 0; b < boxes; ++b) {
                        if (frame_of_box[b] != z) continue;
                        if (paint(labels[b], compose_pixel(logits + b * lowpx, low, py, qy, pxi, qx), &cls)) break;
                    }
                    static_cast<uint8_t *>(out)[px] = cls;
                } else {
                    const double v = compose_pixel(logits + z * lowpx, low, py, qy, pxi, qx);
                    if (mode == SGV3D_SAM_COMPOSE_BOOL)
                        static_cast<uint8_t *>(out)[px] = v > 0.0 ? 1 : 0;
                    else
                        static_cast<float *>(out)[px] = (float)v;
                }
            }
    return SGV3D_OK;
}

extern "C" int sgv3d_resize_u8_filter(int frames, int in_h, int in_w, int out_h, int out_w, const int32_t *xbounds, const int32_t *xcoeffs,
                                      int xksize, const int32_t *ybounds, const int32_t *ycoeffs, int yksize, int swap_rb, const uint8_t *src,
                                      uint8_t *tmp, float *dst, void *stream) {
    SGV3D_REQUIRE(frames > 0 && in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, "resize_u8_filter: non-positive size (%d frames, %d x %d -> %d x %d)",
                  frames, in_h, in_w, out_h, out_w);
    SGV3D_REQUIRE(xksize > 0 && yksize > 0, "resize_u8_filter: non-positive ksize (%d, %d)", xksize, yksize);
    SGV3D_REQUIRE(xbounds && xcoeffs && ybounds && ycoeffs && src && tmp && dst, "resize_u8_filter: null pointer");
    SGV3D_REQUIRE(frames <= 65535 && in_h <= 65535 * 4 && out_h <= 65535 * 4, "resize_u8_filter: too many frames or rows");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(resize_u8_h_kernel, dim3(cdiv(out_w, 64), cdiv(in_h, 4), frames), dim3(kBlock), 0, st, in_h, in_w, out_w, xbounds, xcoeffs,
                       xksize, src, tmp);
    if (int rc = check_launch("resize_u8_h_kernel")) return rc;
    hipLaunchKernelGGL(resize_u8_v_kernel, dim3(cdiv(out_w, 64), cdiv(out_h, 4), frames), dim3(kBlock), 0, st, in_h, out_h, out_w, ybounds, ycoeffs,
                       yksize, swap_rb, tmp, dst);
    return check_launch("resize_u8_v_kernel");
}
