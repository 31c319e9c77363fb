// SAM's ViT image encoder (layers/backbones/sam_encoder.py of the reference), the parts that are not a convolution:
// windowed / global attention with decomposed relative position (one flash-style launch on the f32 MFMA), LayerNorm over
// the channels of an NHWC map, exact GELU, the input normalise + pad, and the crop + bilinear resize behind the neck.
// What the bf16 forms (csrc/vit_bf16.hip) and the adjoints (csrc/vit_grad.hip) must share with these kernels bit for bit is
// defined once, in csrc/vit_common.hpp.  gfx950 only.  Vector stores only, no float atomics: every kernel is repeatable bit for bit.
#include "vit_common.hpp"

using namespace sgv3d;

namespace {

constexpr int kBlock = 256;
constexpr int kQT = 64;  // queries per workgroup: 16 per wave
constexpr int kKT = 64;  // keys per LDS tile

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
// Workgroups are renumbered over the 8 XCDs (decode_workgroup); the P V loop and the store of O^T are accum_rows and store_rows,
// which the backward uses as well.
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
    constexpr int NL = HD / 16;  // float4 per thread, tensor and tile
    constexpr int C4 = HD / 4;   // float4 per key row
    extern __shared__ __align__(16) float lds[];
    float *Ks = lds;
    float *Vs = Ks + kKT * LDK;
    float *Th = Vs + kKT * LDV;
    float *Tw = Th + kQT * p.th_ld;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, g = lane >> 4;
    const Window wg = decode_workgroup(p);
    const int head = wg.head;
    const int C = p.nH * HD;
    const bool rel = p.rh != nullptr;

    // q, k, v of window token t (< T): the map's row, or the padding token's (null: zeros)
    auto token = [&](int t) -> const float * {
        const int kh = slot_row(t, p.inv_win_w);
        long long pix;
        if (wg.pixel(p, kh, t - kh * p.win_w, pix)) return p.qkv + pix * (3 * C) + head * HD;
        return p.pad ? p.pad + head * HD : nullptr;
    };

    // this lane's query: q[4 c + i] = Q[16 c + 4 g + i]
    const int myq = wave * 16 + lq;
    int tq = wg.qt * kQT + myq;
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
                    // a slot past T reads a valid entry and is masked below
                    const int tc = last ? min(t, p.T - 1) : t;
                    const int kh = slot_row(tc, p.inv_win_w), kw = tc - kh * p.win_w;
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

        accum_rows<HD, LDV>(O, vbase, S, lq);      // O^T += V^T P^T
    }

    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const int oh = wg.h0 + qh, ow = wg.w0 + qw;
    if (q_live && oh < p.H && ow < p.W) {
        if (LSE && g == 0) p.lse[(((size_t)wg.b * p.nH + head) * p.H + oh) * p.W + ow] = m + logf(l);
        float *dst = p.out + ((size_t)((size_t)wg.b * p.H + oh) * p.W + ow) * (size_t)C + head * HD;
        store_rows<HD>(dst, O, g, [l](float o) { return o / l; });
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
// LayerNorm: one wave per row (ln_row_stats, ln_xhat)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void layernorm_kernel(long long rows, int c4, const f32x4 *x, const f32x4 *__restrict__ weight,
                                                           const f32x4 *__restrict__ bias, float eps, f32x4 *y) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const f32x4 *xr = x + row * c4;
    f32x4 *yr = y + row * c4;
    const LnStats st = ln_row_stats(xr, c4, lane, eps);
    for (int i = lane; i < c4; i += 64) {
        const f32x4 v = xr[i], w = weight[i], bb = bias[i];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = ln_xhat(v[k], st) * w[k] + bb[k];
        yr[i] = o;
    }
}

// ------------------------------------------------------------------------------------------------
// GELU (erf form, gelu1)
// ------------------------------------------------------------------------------------------------
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
    const int rc = check_attn_desc("vit_attention", desc, 4);
    if (rc != SGV3D_OK) return rc;
    const sgv3d_vit_attn_desc &d = *desc;
    SGV3D_REQUIRE((rel_pos_h == nullptr) == (rel_pos_w == nullptr),
                  "vit_attention: rel_pos_h and rel_pos_w must be given together or not at all");
    SGV3D_REQUIRE(qkv && out, "vit_attention: null qkv or out");
    SGV3D_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(pad_qkv), "vit_attention: qkv, pad_qkv and out must be 16-byte aligned");
    AttnParams p;
    fill_window(p, d);
    p.nqt = cdiv(p.T, kQT);
    const bool rel = rel_pos_h != nullptr;
    p.th_ld = odd_ld(rel, d.win_h), p.tw_ld = odd_ld(rel, d.win_w);
    p.scale = softmax_scale(d.head_dim);
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
