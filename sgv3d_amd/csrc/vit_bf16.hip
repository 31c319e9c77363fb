// SAM's ViT image encoder in bf16 mode (hip_ops.VIT_BF16): the attention launch on v_mfma_f32_16x16x32_bf16 with bf16 tensors in
// HBM, LayerNorm with a bf16 result and GELU on bf16 tensors.  The f32 forms are csrc/vit.hip; the semantics (windows indexed in
// the un-partitioned map, the qkv bias as the padding tokens, the unscaled q in the relative-position terms) are the same.
// The descriptor checks, the window geometry, the LayerNorm row statistics and the GELU formula are the f32 forms' own, from
// csrc/vit_common.hpp; the attention inner loop has other MFMA operands and is this file's.
// gfx950 only.  Vector stores only, no atomics: every kernel is repeatable bit for bit.
#include "vit_common.hpp"

using namespace sgv3d;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int kBlock = 256;
constexpr int kKT = 64;  // keys per LDS tile: two k-steps of 32 keys for P V, four 16-key sub-tiles for Q K^T

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
    return z;
}

// eight f32 parameters (16-byte aligned), rounded to bf16 (RNE) on the way in
__device__ __forceinline__ bf16x8 cvt8(const float *src) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(src), b = *reinterpret_cast<const f32x4 *>(src + 4);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = (__bf16)a[j];
        o[4 + j] = (__bf16)b[j];
    }
    return o;
}

// ds_read_b64_tr_b16 twice: this lane's column of rows k .. k + 3 (elements 0..3) and of the four rows 16 below (elements 4..7).
// Every lane of a 16-lane group supplies the address of row (lane >> 2) & 3, columns 4 (lane & 3) .. + 3 of the group's block.
__device__ __forceinline__ bf16x8 tr_read8(const unsigned char *lds, int off, int off_hi) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(lds + off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(lds + off_hi));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// ------------------------------------------------------------------------------------------------
// attention
// ------------------------------------------------------------------------------------------------
// A workgroup of four waves owns 64 QW consecutive queries of one (image, head, window); a wave owns QW blocks of 16.  Both
// products are v_mfma_f32_16x16x32_bf16 (A: lane holds [row lane & 15][k 8 (lane >> 4) + j], B: [k 8 (lane >> 4) + j][col
// lane & 15], j = 0..7; D: col lane & 15, row 4 (lane >> 4) + reg).  With lq = lane & 15 and g = lane >> 4:
//   S^T = K Q^T  A = 16 keys of the K image (one 16-byte row read, d = 32 s + 8 g + j in k-step s), B = the query block, read from
//                HBM once.  Lane (lq, g) then holds the logits of query lq for keys 4 g + r of each 16-key sub-tile: the row maximum
//                is in-lane fmax and two cross-lane steps.  head_dim 80 takes a third k-step whose d >= 80 are zero in both operands.
//                The accumulator is scaled by head_dim^-0.5 in f32; T_h and T_w are added in f32.
//   O^T = V^T P^T  one k-step sums 32 keys: slot 8 g + j stands for key 16 (j >> 2) + 4 g + (j & 3) of the 32, so the B operand of
//                lane (lq, g) is registers 0..3 of S^T's sub-tiles 2 kb and 2 kb + 1, rounded to bf16, as they stand.  The A operand
//                follows the same permutation: two transposed reads (ds_read_b64_tr_b16) of the row-major V image give lane (lq, g)
//                column 16 db + lq of rows 4 g .. 4 g + 3 and of the four rows 16 below.  O^T has the query on the lane: the rescale
//                is one multiplier per lane and block, and a lane stores four consecutive bf16 of d = 16 db + 4 g + r.
// P is rounded to bf16 once and the row sum adds the ROUNDED values; O / l is rounded to bf16 once.
// LDS: K rows of 2 head_dim + 16 bytes, V rows of 96 bytes (head_dim 32) or 160 bytes (64, 80: an odd number of 32-byte units, so
// the eight rows a 32-lane half reads transposed fall on eight distinct 32-byte units of the 256-byte bank row: conflict-free).
// Both are double-buffered: the next tile is loaded into registers after Q K^T and written to the other buffer after P V, one
// barrier per tile.  T_h = q rel_pos_h^T and T_w = q rel_pos_w^T (bf16 operands, f32 sums) are formed once per workgroup on the
// MFMA and kept in LDS as f32 [query][kh] and [query][kw].  The last tile of a window skips its second 32-key block when no key
// lives there.  Workgroups are renumbered over the 8 XCDs (decode_workgroup).
struct AttnParams {
    int B, H, W, nH, win_h, win_w, nwy, nwx, T, nqt, th_ld, tw_ld;
    float scale2, inv_win_w;      // scale2 = head_dim^-0.5 log2(e): the logits are kept in units of log2
    const __bf16 *qkv;
    const float *pad, *rh, *rw;
    __bf16 *out;
    float *lse;                   // the lse entry only: [B, nH, H, W], natural-log units
};

template <int HD>
struct AttnGeom {
    static constexpr int KSTR = 2 * HD + 16;            // bytes per key row of the K image
    static constexpr int VSTR = HD == 32 ? 96 : 160;    // ... of the V image
    static constexpr int kv_bytes = 2 * kKT * (KSTR + VSTR);
};

constexpr float kLog2e = 1.44269504088896341f;

// VEC: win_w % 4 == 0, so the four consecutive slots of a lane share kh and are four consecutive kw: one T_h read and one 16-byte
// T_w read per four scores (tw_ld is a multiple of 4 then)
// LSE: also lse = (m + log2 l) ln 2 of every query, l the row sum over the rounded P (sgv3d_vit_attention_bf16_lse); `out` is
// the same instruction stream either way
template <int HD, int QW, bool VEC, bool LSE>
__device__ __forceinline__ void vit_attention_bf16_body(const AttnParams &p) {
    constexpr int QT = 64 * QW;          // queries per workgroup
    constexpr int NK = (HD + 31) / 32;   // k-steps of Q K^T
    constexpr int ND = HD / 16;          // accumulators of O^T per query block
    constexpr int C8 = HD / 8;           // 16-byte chunks per key row
    constexpr int NL = (kKT * C8 + kBlock - 1) / kBlock;
    constexpr int KSTR = AttnGeom<HD>::KSTR, VSTR = AttnGeom<HD>::VSTR;
    constexpr int KBUF = kKT * KSTR, VBUF = kKT * VSTR;
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned char *Kb = lds;
    unsigned char *Vb = lds + 2 * KBUF;
    float *Th = reinterpret_cast<float *>(lds + 2 * KBUF + 2 * VBUF);
    float *Tw = Th + QT * p.th_ld;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, g = lane >> 4;
    const Window wg = decode_workgroup(p);
    const int head = wg.head;
    const int C = p.nH * HD;
    const bool rel = p.rh != nullptr;

    // eight consecutive d of q (which = 0), k (1) or v (2) of window token t (< T): the map's, or the padding token's (null: zeros)
    auto load8 = [&](int t, int which, int d0) -> bf16x8 {
        const int kh = slot_row(t, p.inv_win_w);
        const int col = which * C + head * HD + d0;
        long long pix;
        if (wg.pixel(p, kh, t - kh * p.win_w, pix)) return *reinterpret_cast<const bf16x8 *>(p.qkv + pix * (3 * C) + col);
        if (p.pad) return cvt8(p.pad + col);
        return zero8();
    };

    int qh[QW], qw[QW];
    bool q_live[QW];
    bf16x8 qf[QW][NK];
#pragma unroll
    for (int qb = 0; qb < QW; ++qb) {
        int tq = wg.qt * QT + (wave * QW + qb) * 16 + lq;
        q_live[qb] = tq < p.T;
        tq = q_live[qb] ? tq : p.T - 1;
        qh[qb] = tq / p.win_w;
        qw[qb] = tq - qh[qb] * p.win_w;
#pragma unroll
        for (int s = 0; s < NK; ++s) qf[qb][s] = 32 * s + 8 * g < HD ? load8(tq, 0, 32 * s + 8 * g) : zero8();
    }

    if (rel) {
        // T_h[query][kh] = q . rel_pos_h[qh - kh + win_h - 1]: the product with every table row, kept where a key row answers
        for (int axis = 0; axis < 2; ++axis) {
            const float *tab = axis ? p.rw : p.rh;
            const int win = axis ? p.win_w : p.win_h, ld = axis ? p.tw_ld : p.th_ld;
            float *base = axis ? Tw : Th;
            const int rows = 2 * win - 1;
            for (int r0 = 0; r0 < rows; r0 += 16) {
                const float *trow = tab + (size_t)min(r0 + lq, rows - 1) * HD;
                f32x4 acc[QW];
#pragma unroll
                for (int qb = 0; qb < QW; ++qb) acc[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < NK; ++s) {
                    const bf16x8 a = 32 * s + 8 * g < HD ? cvt8(trow + 32 * s + 8 * g) : zero8();
#pragma unroll
                    for (int qb = 0; qb < QW; ++qb) acc[qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[qb][s], acc[qb], 0, 0, 0);
                }
#pragma unroll
                for (int qb = 0; qb < QW; ++qb) {
                    float *dst = base + ((wave * QW + qb) * 16 + lq) * ld;
                    const int qpos = axis ? qw[qb] : qh[qb];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int t = r0 + 4 * g + r;
                        const int kpos = qpos + win - 1 - t;
                        if (t < rows && kpos >= 0 && kpos < win) dst[kpos] = acc[qb][r] * kLog2e;
                    }
                }
            }
        }
    }

    bf16x8 kreg[NL], vreg[NL];
    auto gload = [&](int tile) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int key = i / C8, c8 = i - key * C8;
            const int t = tile * kKT + key;
            kreg[n] = zero8();      // keys past T: zero K and V (their P is exactly 0)
            vreg[n] = zero8();
            if (i < kKT * C8 && t < p.T) {
                kreg[n] = load8(t, 1, 8 * c8);
                vreg[n] = load8(t, 2, 8 * c8);
            }
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int key = i / C8, c8 = i - key * C8;
            if (i < kKT * C8) {
                *reinterpret_cast<bf16x8 *>(Kb + buf * KBUF + key * KSTR + 16 * c8) = kreg[n];
                *reinterpret_cast<bf16x8 *>(Vb + buf * VBUF + key * VSTR + 16 * c8) = vreg[n];
            }
        }
    };

    const int ntiles = (p.T + kKT - 1) / kKT;
    float m[QW];            // running maximum, in units of log2 (the same in the four lanes of a query)
    f32x4 L[QW];            // the sum of the ROUNDED P: the product of P^T with a matrix of ones, every row the same
    f32x4 O[QW][ND];
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.f;
    const float *th[QW], *tw[QW];
#pragma unroll
    for (int qb = 0; qb < QW; ++qb) {
        m[qb] = -INFINITY;
        L[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < ND; ++j) O[qb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        th[qb] = Th + ((wave * QW + qb) * 16 + lq) * p.th_ld;
        tw[qb] = Tw + ((wave * QW + qb) * 16 + lq) * p.tw_ld;
    }
    const int koff = lq * KSTR + 16 * g;                                 // + sub * 16 * KSTR + 64 * s
    const int voff = (4 * g + (lq >> 2)) * VSTR + 8 * (lq & 3);         // + kb * 32 * VSTR + 32 * db

    gload(0);
    lstore(0);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1;
        __syncthreads();   // this tile is written, the other buffer has been read (first pass: T_h, T_w are written)
        const unsigned char *Kc = Kb + buf * KBUF, *Vc = Vb + buf * VBUF;
        const bool last = tile == ntiles - 1;                    // the only tile with slots past T
        const bool two = !last || p.T - tile * kKT > 32;         // its second 32-key block holds a key

        f32x4 S[QW][4];
#pragma unroll
        for (int qb = 0; qb < QW; ++qb)
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) S[qb][sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb == 0 || two) {
#pragma unroll
                for (int s = 0; s < NK; ++s) {
                    // head_dim 80, third k-step: lane groups 2 and 3 stand for d >= 80; they re-read a valid chunk and use zeros
                    const bool dead = HD == 80 && s == 2 && g >= 2;
                    const int off = koff + 64 * s - (dead ? 32 : 0);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int sub = 2 * kb + h;
                        bf16x8 kf = *reinterpret_cast<const bf16x8 *>(Kc + sub * 16 * KSTR + off);
                        if (dead) kf = zero8();
#pragma unroll
                        for (int qb = 0; qb < QW; ++qb) S[qb][sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qb][s], S[qb][sub], 0, 0, 0);
                    }
                }
            }
        }

        if (!last) gload(tile + 1);

        float mx[QW];
#pragma unroll
        for (int qb = 0; qb < QW; ++qb) mx[qb] = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int t0 = tile * kKT + sub * 16 + 4 * g;
            float bias[QW][4];      // T_h + T_w of the lane's four slots; a slot past T takes a valid entry (it is masked below)
            if (rel) {
                if (VEC) {
                    const int tc = min(t0, p.T - 4);
                    const int kh = slot_row(tc, p.inv_win_w), kw = tc - kh * p.win_w;
#pragma unroll
                    for (int qb = 0; qb < QW; ++qb) {
                        const float a = th[qb][kh];
                        const f32x4 w4 = *reinterpret_cast<const f32x4 *>(tw[qb] + kw);
#pragma unroll
                        for (int r = 0; r < 4; ++r) bias[qb][r] = a + w4[r];
                    }
                } else {
                    // (kh, kw) of four consecutive slots: one division, then steps
                    const int tc = min(t0, p.T - 1);
                    int kh = slot_row(tc, p.inv_win_w), kw = tc - kh * p.win_w;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
#pragma unroll
                        for (int qb = 0; qb < QW; ++qb) bias[qb][r] = th[qb][kh] + tw[qb][kw];
                        if (t0 + r + 1 < p.T) {
                            ++kw;
                            if (kw == p.win_w) kw = 0, ++kh;
                        }
                    }
                }
            }
#pragma unroll
            for (int qb = 0; qb < QW; ++qb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // the scale multiplies the f32 accumulator, never a bf16 operand
                    float s = rel ? fmaf(S[qb][sub][r], p.scale2, bias[qb][r]) : S[qb][sub][r] * p.scale2;
                    if (last && t0 + r >= p.T) s = -INFINITY;     // a key past the window: masked, not a zero logit
                    S[qb][sub][r] = s;
                    mx[qb] = fmaxf(mx[qb], s);
                }
        }

        bf16x8 pf[QW][2];
#pragma unroll
        for (int qb = 0; qb < QW; ++qb) {
            float v = mx[qb];
            v = fmaxf(v, __shfl_xor(v, 16));
            v = fmaxf(v, __shfl_xor(v, 32));
            const float m_new = fmaxf(m[qb], v);       // finite from the first tile on: key 0 is never masked
            const float alpha = __builtin_amdgcn_exp2f(m[qb] - m_new);   // first tile: 2^-inf = 0
            m[qb] = m_new;
            if (__any(alpha != 1.f)) {      // some query of the wave met a new maximum (a factor of 1 changes no bit)
                L[qb] *= alpha;
#pragma unroll
                for (int j = 0; j < ND; ++j) O[qb][j] *= alpha;
            }
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // v_exp_f32 of the difference (log2 e is in scale2 and in the tables), rounded to bf16 once
                    pf[qb][sub >> 1][4 * (sub & 1) + r] = (__bf16)__builtin_amdgcn_exp2f(S[qb][sub][r] - m_new);
                }
        }

#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (kb == 0 || two) {
#pragma unroll
                for (int qb = 0; qb < QW; ++qb) L[qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf[qb][kb], L[qb], 0, 0, 0);
#pragma unroll
                for (int db = 0; db < ND; ++db) {
                    const int off = voff + kb * 32 * VSTR + 32 * db;
                    const bf16x8 vf = tr_read8(Vc, off, off + 16 * VSTR);
#pragma unroll
                    for (int qb = 0; qb < QW; ++qb) O[qb][db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qb][kb], O[qb][db], 0, 0, 0);
                }
            }
        }

        if (!last) lstore(buf ^ 1);
    }

#pragma unroll
    for (int qb = 0; qb < QW; ++qb) {
        const float sum = L[qb][0];
        const int oh = wg.h0 + qh[qb], ow = wg.w0 + qw[qb];
        if (q_live[qb] && oh < p.H && ow < p.W) {
            // row 4 g + r of accumulator db is d = 16 db + 4 g + r: four consecutive bf16 per lane and db
            __bf16 *dst = p.out + ((size_t)((size_t)wg.b * p.H + oh) * p.W + ow) * (size_t)C + head * HD + 4 * g;
#pragma unroll
            for (int db = 0; db < ND; ++db) {
                bf16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (__bf16)(O[qb][db][r] / sum);
                *reinterpret_cast<bf16x4 *>(dst + 16 * db) = o;
            }
            if (LSE && g == 0)
                p.lse[(((size_t)wg.b * p.nH + head) * p.H + oh) * (size_t)p.W + ow] = (m[qb] + log2f(sum)) * 0.69314718055994530942f;
        }
    }
}

template <int HD, int QW, bool VEC>
__global__ __launch_bounds__(kBlock) void vit_attention_bf16_kernel(AttnParams p) {
    vit_attention_bf16_body<HD, QW, VEC, false>(p);
}

template <int HD, int QW, bool VEC>
__global__ __launch_bounds__(kBlock) void vit_attention_bf16_lse_kernel(AttnParams p) {
    vit_attention_bf16_body<HD, QW, VEC, true>(p);
}

template <int HD, int QW, bool VEC>
int launch_attention(const AttnParams &p, int blocks, size_t lds_bytes, hipStream_t stream) {
    if (p.lse) {
        static PerDeviceSize state_lse;
        if (!ensure_dynamic_lds(reinterpret_cast<const void *>(vit_attention_bf16_lse_kernel<HD, QW, VEC>), lds_bytes, state_lse))
            return fail(SGV3D_ELAUNCH, "vit_attention_bf16_lse: cannot reserve %zu bytes of LDS", lds_bytes);
        hipLaunchKernelGGL((vit_attention_bf16_lse_kernel<HD, QW, VEC>), dim3(blocks), dim3(kBlock), lds_bytes, stream, p);
        return check_launch("vit_attention_bf16_lse_kernel");
    }
    static PerDeviceSize state;
    if (!ensure_dynamic_lds(reinterpret_cast<const void *>(vit_attention_bf16_kernel<HD, QW, VEC>), lds_bytes, state))
        return fail(SGV3D_ELAUNCH, "vit_attention_bf16: cannot reserve %zu bytes of LDS", lds_bytes);
    hipLaunchKernelGGL((vit_attention_bf16_kernel<HD, QW, VEC>), dim3(blocks), dim3(kBlock), lds_bytes, stream, p);
    return check_launch("vit_attention_bf16_kernel");
}

template <int HD>
int launch_attention_hd(const AttnParams &p, bool wide, bool vec, int blocks, size_t lds_bytes, hipStream_t stream) {
    if (wide) return vec ? launch_attention<HD, 2, true>(p, blocks, lds_bytes, stream) : launch_attention<HD, 2, false>(p, blocks, lds_bytes, stream);
    return vec ? launch_attention<HD, 1, true>(p, blocks, lds_bytes, stream) : launch_attention<HD, 1, false>(p, blocks, lds_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// LayerNorm with a bf16 result: layernorm_kernel of csrc/vit.hip (ln_row_stats, ln_xhat) and one more rounding
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void layernorm_bf16out_kernel(long long rows, int c4, const f32x4 *x, const f32x4 *__restrict__ weight,
                                                                   const f32x4 *__restrict__ bias, float eps, bf16x4 *y) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const f32x4 *xr = x + row * c4;
    bf16x4 *yr = y + row * c4;
    const LnStats st = ln_row_stats(xr, c4, lane, eps);
    for (int i = lane; i < c4; i += 64) {
        const f32x4 v = xr[i], w = weight[i], bb = bias[i];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = ln_xhat(v[k], st) * w[k] + bb[k];
        bf16x4 ob;
#pragma unroll
        for (int k = 0; k < 4; ++k) ob[k] = (__bf16)o[k];
        yr[i] = ob;
    }
}

// ------------------------------------------------------------------------------------------------
// GELU on bf16 tensors: the f32 formula (gelu1) on the widened value, rounded once
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gelu_bf16_kernel(long long n8, int tail, const __bf16 *x, __bf16 *y) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n8) {
        const bf16x8 v = reinterpret_cast<const bf16x8 *>(x)[i];
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (__bf16)gelu1((float)v[k]);
        reinterpret_cast<bf16x8 *>(y)[i] = o;
    }
    if (i < tail) y[8 * n8 + i] = (__bf16)gelu1((float)x[8 * n8 + i]);
}

}  // namespace

// sgv3d_vit_attention_bf16 (lse null) and sgv3d_vit_attention_bf16_lse: one set of checks, one launch geometry
static int vit_attention_bf16_impl(const char *who, const sgv3d_vit_attn_desc *desc, const void *qkv, const float *pad_qkv,
                                   const float *rel_pos_h, const float *rel_pos_w, void *out, float *lse, void *stream) {
    const int rc = check_attn_desc(who, desc, 8);
    if (rc != SGV3D_OK) return rc;
    const sgv3d_vit_attn_desc &d = *desc;
    SGV3D_REQUIRE((rel_pos_h == nullptr) == (rel_pos_w == nullptr), "%s: rel_pos_h and rel_pos_w must be given together or not at all", who);
    SGV3D_REQUIRE(qkv && out, "%s: null qkv or out", who);
    SGV3D_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(pad_qkv) && aligned16(rel_pos_h) && aligned16(rel_pos_w),
                  "%s: qkv, pad_qkv, rel_pos_h, rel_pos_w and out must be 16-byte aligned", who);
    AttnParams p;
    fill_window(p, d);
    const bool rel = rel_pos_h != nullptr;
    const bool vec = rel && d.win_w % 4 == 0;      // 16-byte T_w reads: rows of win_w + 4 floats
    p.th_ld = odd_ld(rel, d.win_h);
    p.tw_ld = vec ? d.win_w + 4 : odd_ld(rel, d.win_w);
    p.scale2 = softmax_scale(d.head_dim) * kLog2e;
    p.qkv = static_cast<const __bf16 *>(qkv), p.pad = pad_qkv, p.rh = rel_pos_h, p.rw = rel_pos_w, p.out = static_cast<__bf16 *>(out);
    p.lse = lse;
    const size_t kv_bytes = d.head_dim == 32 ? AttnGeom<32>::kv_bytes : d.head_dim == 64 ? AttnGeom<64>::kv_bytes : AttnGeom<80>::kv_bytes;
    const size_t t_bytes = sizeof(float) * (size_t)(p.th_ld + p.tw_ld);      // per query
    // 32 queries per wave (a K / V fragment read feeds two MFMAs) where a window has more than 64 queries and two workgroups
    // still share a CU's 160 KiB of LDS; 16 per wave otherwise
    const bool wide = p.T > 64 && kv_bytes + 128 * t_bytes <= 64 * 1024;
    const int qtile = wide ? 128 : 64;
    p.nqt = cdiv(p.T, qtile);
    const size_t lds_bytes = kv_bytes + (size_t)qtile * t_bytes;
    const long long blocks = (long long)d.batch * d.heads * p.nwy * p.nwx * p.nqt;
    SGV3D_REQUIRE(blocks < (1LL << 31), "%s: too many workgroups", who);
    hipStream_t s = as_stream(stream);
    switch (d.head_dim) {
        case 32: return launch_attention_hd<32>(p, wide, vec, (int)blocks, lds_bytes, s);
        case 64: return launch_attention_hd<64>(p, wide, vec, (int)blocks, lds_bytes, s);
        default: return launch_attention_hd<80>(p, wide, vec, (int)blocks, lds_bytes, s);
    }
}

extern "C" int sgv3d_vit_attention_bf16(const sgv3d_vit_attn_desc *desc, const void *qkv, const float *pad_qkv, const float *rel_pos_h,
                                        const float *rel_pos_w, void *out, void *stream) {
    return vit_attention_bf16_impl("vit_attention_bf16", desc, qkv, pad_qkv, rel_pos_h, rel_pos_w, out, nullptr, stream);
}

extern "C" int sgv3d_vit_attention_bf16_lse(const sgv3d_vit_attn_desc *desc, const void *qkv, const float *pad_qkv, const float *rel_pos_h,
                                            const float *rel_pos_w, void *out, float *lse, void *stream) {
    SGV3D_REQUIRE(lse, "vit_attention_bf16_lse: null lse");
    SGV3D_REQUIRE(aligned16(lse), "vit_attention_bf16_lse: lse must be 16-byte aligned");
    return vit_attention_bf16_impl("vit_attention_bf16_lse", desc, qkv, pad_qkv, rel_pos_h, rel_pos_w, out, lse, stream);
}

extern "C" int sgv3d_layernorm_bf16out(long long rows, int channels, const float *x, const float *weight, const float *bias, float eps,
                                       void *y, void *stream) {
    SGV3D_REQUIRE(rows > 0 && channels > 0, "layernorm_bf16out: non-positive size (rows %lld, channels %d)", rows, channels);
    SGV3D_REQUIRE(channels % 8 == 0, "layernorm_bf16out: channels %d is not a multiple of 8", channels);
    SGV3D_REQUIRE(x && weight && bias && y, "layernorm_bf16out: null pointer");
    SGV3D_REQUIRE(eps >= 0.f, "layernorm_bf16out: negative eps");
    SGV3D_REQUIRE(aligned16(x) && aligned16(weight) && aligned16(bias) && aligned16(y), "layernorm_bf16out: pointers must be 16-byte aligned");
    const long long blocks = (rows + kBlock / 64 - 1) / (kBlock / 64);
    SGV3D_REQUIRE(blocks < (1LL << 31), "layernorm_bf16out: too many rows");
    hipLaunchKernelGGL(layernorm_bf16out_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), rows, channels / 4,
                       reinterpret_cast<const f32x4 *>(x), reinterpret_cast<const f32x4 *>(weight),
                       reinterpret_cast<const f32x4 *>(bias), eps, reinterpret_cast<bf16x4 *>(y));
    return check_launch("layernorm_bf16out_kernel");
}

extern "C" int sgv3d_gelu_bf16(long long n, const void *x, void *y, void *stream) {
    SGV3D_REQUIRE(n > 0, "gelu_bf16: non-positive count %lld", n);
    SGV3D_REQUIRE(x && y, "gelu_bf16: null pointer");
    SGV3D_REQUIRE(aligned16(x) && aligned16(y), "gelu_bf16: pointers must be 16-byte aligned");
    const long long n8 = n / 8;
    const long long blocks = (n8 + kBlock) / kBlock;    // at least one: its first threads take the tail
    SGV3D_REQUIRE(blocks < (1LL << 31), "gelu_bf16: too many values");
    hipLaunchKernelGGL(gelu_bf16_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), n8, (int)(n - 8 * n8),
                       static_cast<const __bf16 *>(x), static_cast<__bf16 *>(y));
    return check_launch("gelu_bf16_kernel");
}
