// The attention adjoint of SAM's ViT image encoder in bf16 training mode (hip_ops.VIT_TRAIN_BF16): the adjoint of the launch of
// csrc/vit_bf16.hip on v_mfma_f32_16x16x32_bf16 with bf16 tensors in HBM.  The semantics are those of the f32 adjoint
// (csrc/vit_grad.hip): windows in the un-partitioned map, padding slots as keys but never as queries, the unscaled q in the
// relative-position terms, dpad_qkv.  gfx950 only.  Vector stores only, no atomics, a fixed summation order: repeatable bit for bit
// and graph-capturable (no host wait, no allocation).
#include "vit_common.hpp"

using namespace sgv3d;

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

constexpr int kBlock = 256;
constexpr int kTile = 64;     // owned slots per workgroup (16 per wave) and streamed slots per LDS tile
constexpr float kLog2e = 1.44269504088896341f;

static inline long long up4(long long v) { return (v + 3) & ~3LL; }
// ranges of `a_bytes` and `b_bytes` bytes
static inline bool overlaps(const void *a, unsigned long long a_bytes, const void *b, unsigned long long b_bytes) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa < pb + b_bytes && pb < pa + a_bytes;
}

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.f;
    return z;
}

// eight f32 parameters (16-byte aligned), rounded to bf16 (RNE) on the way in, as the forward rounds them
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

// ds_read_b64_tr_b16 twice, as csrc/vit_bf16.hip reads V: this lane's column of rows k .. k + 3 and of the four rows 16 below
__device__ __forceinline__ bf16x8 tr_read8(const unsigned char *lds, int off, int off_hi) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(lds + off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(lds + off_hi));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

// Per (image, head, window) "group" with T = win_h * win_w slots (Tp = T rounded up to 64) the workspace holds, in floats, what
// the f32 adjoint's holds:
//   lse_w, delta_w [G][Tp]          lse (in units of log2) of the slot as a query, +inf for a padding slot or a slot past T (its P
//                                   is exactly 0: never a query), and delta = dO . O (0 there)
//   th [G][Tp][win_h], tw [G][Tp][win_w]      log2(e) q_i . R_h[ih - kh + win_h - 1] and ... R_w[...], formed as the forward forms them
//   thT [G][win_h][Tp], twT [G][win_w][Tp]    the same, transposed: what a lane that owns a KEY reads for four queries at once
//   ah [G][Tp][win_h], aw [G][Tp][win_w]      A_h, A_w of the query-owning launch, read by the table-gradient launch
//   padpart [G * ntiles][2][head_dim]         dk, dv summed over the padding slots of one key tile
//   relpart_h [G][2 win_h - 1][head_dim], relpart_w [G][2 win_w - 1][head_dim]
// Launches: prep (th, tw, lse_w, delta_w) -> keys (dk, dv, padpart) -> queries (dq, ah, aw) -> table partials -> finish.
struct BwdLayout {
    long long G, T, Tp, nt;
    long long lse_w, delta_w, th, tw, thT, twT, ah, aw, padpart, relh, relw, total;   // offsets in floats
};

static BwdLayout bwd_layout(const sgv3d_vit_attn_desc &d, bool rel) {
    BwdLayout L;
    const long long nwy = cdiv(d.height, d.win_h), nwx = cdiv(d.width, d.win_w);
    L.G = (long long)d.batch * d.heads * nwy * nwx;
    L.T = (long long)d.win_h * d.win_w;
    L.nt = (L.T + kTile - 1) / kTile;
    L.Tp = L.nt * kTile;
    long long o = 0;
    auto take = [&](long long n) {
        const long long at = o;
        o += up4(n);
        return at;
    };
    L.lse_w = take(L.G * L.Tp);
    L.delta_w = take(L.G * L.Tp);
    const long long nh = rel ? L.G * L.Tp * d.win_h : 0, nw = rel ? L.G * L.Tp * d.win_w : 0;
    L.th = take(nh), L.tw = take(nw), L.thT = take(nh), L.twT = take(nw), L.ah = take(nh), L.aw = take(nw);
    L.padpart = take(L.G * L.nt * 2 * d.head_dim);
    L.relh = take(rel ? L.G * (2LL * d.win_h - 1) * d.head_dim : 0);
    L.relw = take(rel ? L.G * (2LL * d.win_w - 1) * d.head_dim : 0);
    L.total = o;
    return L;
}

struct BwdParams {
    int B, H, W, nH, HD, win_h, win_w, nwy, nwx, T, Tp, nt, ah_ld, aw_ld;
    float scale, scale2, inv_win_w;     // scale2 = scale log2(e): the logits are formed in units of log2, as in the forward
    const __bf16 *qkv, *out, *dout;
    const float *pad, *rh, *rw, *lse;
    __bf16 *dqkv;
    float *dpad, *drh, *drw;
    float *lse_w, *delta_w, *th, *tw, *thT, *twT, *ah, *aw, *padpart, *relh, *relw;
    long long G;
};

// pixel index ((b * H + h) * W + w) of window slot t (< T), or -1 for a padding slot
__device__ inline long long slot_pixel(const BwdParams &p, const Window &gr, int t) {
    const int kh = t / p.win_w;
    long long pix;
    return gr.pixel(p, kh, t - kh * p.win_w, pix) ? pix : -1;
}

// A workgroup takes 64 slots of one group, a wave 16 of them: T_h and T_w of the slot as a query, formed as the forward forms
// them (bf16 q and bf16-rounded table rows on the MFMA, k-steps in order, times log2 e), to th / tw and their transposes; then one
// thread per slot: lse in units of log2 and delta = dO . O in f32 from the stored bf16 values.
template <int HD>
__global__ __launch_bounds__(kBlock) void attn_bwd16_prep_kernel(BwdParams p) {
    constexpr int NK = (HD + 31) / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, g = lane >> 4;
    const long long grp = blockIdx.x / p.nt;
    const int ot = (int)(blockIdx.x - grp * p.nt);
    const Window gr = decode_window(p, grp);
    const int C = p.nH * HD;
    if (p.rh != nullptr) {
        const int o = ot * kTile + wave * 16 + lq;
        const int oc = min(o, p.T - 1);
        const int qh = oc / p.win_w, qw = oc - qh * p.win_w;
        const long long pix = o < p.T ? slot_pixel(p, gr, o) : -1;
        bf16x8 qf[NK];
#pragma unroll
        for (int s = 0; s < NK; ++s)
            qf[s] = (pix >= 0 && 32 * s + 8 * g < HD) ? *reinterpret_cast<const bf16x8 *>(p.qkv + pix * 3 * C + gr.head * HD + 32 * s + 8 * g)
                                                      : zero8();
        for (int axis = 0; axis < 2; ++axis) {
            const float *tab = axis ? p.rw : p.rh;
            const int win = axis ? p.win_w : p.win_h;
            float *row = (axis ? p.tw : p.th) + (grp * p.Tp + o) * win;
            float *col = (axis ? p.twT : p.thT) + grp * win * p.Tp + o;
            const int rows = 2 * win - 1, qpos = axis ? qw : qh;
            for (int r0 = 0; r0 < rows; r0 += 16) {
                const float *trow = tab + (size_t)min(r0 + lq, rows - 1) * HD;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < NK; ++s) {
                    const bf16x8 a = 32 * s + 8 * g < HD ? cvt8(trow + 32 * s + 8 * g) : zero8();
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, qf[s], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = r0 + 4 * g + r;
                    const int kpos = qpos + win - 1 - t;
                    if (t < rows && kpos >= 0 && kpos < win) {
                        const float v = acc[r] * kLog2e;
                        row[kpos] = v;
                        col[(long long)kpos * p.Tp] = v;
                    }
                }
            }
        }
    }
    if (tid < kTile) {
        const int i = ot * kTile + tid;
        const long long pix = i < p.T ? slot_pixel(p, gr, i) : -1;
        float dl = 0.f, ls = INFINITY;
        if (pix >= 0) {
            const __bf16 *o = p.out + pix * C + gr.head * HD, *dO = p.dout + pix * C + gr.head * HD;
            for (int d = 0; d < HD; d += 8) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(o + d), b = *reinterpret_cast<const bf16x8 *>(dO + d);
#pragma unroll
                for (int e = 0; e < 8; ++e) dl = fmaf((float)a[e], (float)b[e], dl);
            }
            const long long hw = pix - (long long)gr.b * p.H * p.W;
            ls = p.lse[((long long)gr.b * p.nH + gr.head) * p.H * p.W + hw] * kLog2e;
        }
        p.lse_w[grp * p.Tp + i] = ls;
        p.delta_w[grp * p.Tp + i] = dl;
    }
}

template <int HD>
struct BwdGeom {
    static constexpr int STR = HD == 32 ? 96 : 160;     // bytes per row of both streamed tiles: the V image of csrc/vit_bf16.hip
    static constexpr int LD = HD + 8;                   // floats per row of the two f32 staging tiles
    static constexpr int bytes = 2 * kTile * STR + 2 * kTile * LD * 4;
};

// All five products are v_mfma_f32_16x16x32_bf16 in the operand layouts of csrc/vit_bf16.hip (lq = lane & 15, g = lane >> 4).  A
// wave OWNS 16 slots, one per lq, as the B operand (d = 32 s + 8 g + j of k-step s in registers) and the workgroup streams 64-row
// tiles of two bf16 tensors X, Y through LDS:
//   KEYS = false  owned: queries (a = q, bb = dO), streamed: X = K, Y = V.    dq^T += K^T dS^T.   A_h, A_w accumulate in LDS (f32).
//   KEYS = true   owned: keys (a = k, bb = v),    streamed: X = Q, Y = dO.   dv^T += dO^T P,  dk^T += Q^T dS.
// S and dP: A = 16 streamed rows (one 16-byte row read per k-step), B = the owned operand; lane (lq, g) then holds streamed rows
// 4 g + r of each 16-row sub-tile for owned slot lq.  With KEYS = false that is the forward's own product (A = K, B = Q, the same
// k-step order); S is scaled in f32 and T_h + T_w (prep) is added in f32, as in the forward.  P = exp2(S - lse) in f32; P and
// dS = P (dP - delta) are rounded to bf16 once, as the B operands of the second products, whose A operands are transposed reads
// (ds_read_b64_tr_b16) of the same row-major tiles: slot 8 g + j of a k-step stands for row 16 (j >> 2) + 4 g + (j & 3) of 32 in
// both operands.  The softmax scale multiplies the f32 accumulators of dq and dk at the end.  Nothing of size tokens x keys exists.
template <int HD, bool KEYS>
__global__ __launch_bounds__(kBlock) void attn_bwd16_kernel(BwdParams p) {
    constexpr int NK = (HD + 31) / 32, ND = HD / 16, C8 = HD / 8, C4 = HD / 4;
    constexpr int NL = (kTile * C8 + kBlock - 1) / kBlock;
    constexpr int STR = BwdGeom<HD>::STR, LD = BwdGeom<HD>::LD, BUF = kTile * STR;
    extern __shared__ __align__(16) unsigned char lds[];
    unsigned char *Xs = lds, *Ys = lds + BUF;
    float *St1 = reinterpret_cast<float *>(lds + 2 * BUF);
    float *St2 = St1 + kTile * LD;
    float *Ahs = St2 + kTile * LD;           // [64][ah_ld]   (KEYS = false with tables only)
    float *Aws = Ahs + kTile * p.ah_ld;      // [64][aw_ld]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lq = lane & 15, g = lane >> 4;
    const long long grp = blockIdx.x / p.nt;
    const int ot = (int)(blockIdx.x - grp * p.nt);
    const Window gr = decode_window(p, grp);
    const int C = p.nH * HD;
    const bool rel = p.rh != nullptr;
    const float *lse_w = p.lse_w + grp * p.Tp, *delta_w = p.delta_w + grp * p.Tp;

    const int myrow = wave * 16 + lq;
    const int o = ot * kTile + myrow;             // owned slot (< Tp)
    const int oc = min(o, p.T - 1);
    const int o_h = oc / p.win_w, o_w = oc - o_h * p.win_w;
    const long long opix = o < p.T ? slot_pixel(p, gr, o) : -1;

    bf16x8 a[NK], bb[NK];
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        const int d0 = 32 * s + 8 * g;
        a[s] = bb[s] = zero8();
        if (d0 < HD) {
            if (KEYS) {
                if (opix >= 0) {
                    const __bf16 *src = p.qkv + opix * 3 * C + C + gr.head * HD + d0;
                    a[s] = *reinterpret_cast<const bf16x8 *>(src), bb[s] = *reinterpret_cast<const bf16x8 *>(src + C);
                } else if (o < p.T && p.pad) {
                    a[s] = cvt8(p.pad + C + gr.head * HD + d0), bb[s] = cvt8(p.pad + 2 * C + gr.head * HD + d0);
                }
            } else if (opix >= 0) {
                a[s] = *reinterpret_cast<const bf16x8 *>(p.qkv + opix * 3 * C + gr.head * HD + d0);
                bb[s] = *reinterpret_cast<const bf16x8 *>(p.dout + opix * C + gr.head * HD + d0);
            }
        }
    }
    const float lse_o = KEYS ? 0.f : lse_w[o], delta_o = KEYS ? 0.f : delta_w[o];

    if (!KEYS && rel)
        for (int i = tid; i < kTile * (p.ah_ld + p.aw_ld); i += kBlock) Ahs[i] = 0.f;

    bf16x8 xreg[NL], yreg[NL];
    auto gload = [&](int tile) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int row = i / C8, c8 = i - row * C8;
            const int t = tile * kTile + row;
            xreg[n] = zero8();      // rows past T, and the padding slots as queries: zero
            yreg[n] = zero8();
            if (i < kTile * C8 && t < p.T) {
                const long long pix = slot_pixel(p, gr, t);
                if (KEYS) {
                    if (pix >= 0) {
                        xreg[n] = *reinterpret_cast<const bf16x8 *>(p.qkv + pix * 3 * C + gr.head * HD + 8 * c8);
                        yreg[n] = *reinterpret_cast<const bf16x8 *>(p.dout + pix * C + gr.head * HD + 8 * c8);
                    }
                } else if (pix >= 0) {
                    const __bf16 *src = p.qkv + pix * 3 * C + C + gr.head * HD + 8 * c8;
                    xreg[n] = *reinterpret_cast<const bf16x8 *>(src), yreg[n] = *reinterpret_cast<const bf16x8 *>(src + C);
                } else if (p.pad) {
                    xreg[n] = cvt8(p.pad + C + gr.head * HD + 8 * c8), yreg[n] = cvt8(p.pad + 2 * C + gr.head * HD + 8 * c8);
                }
            }
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int row = i / C8, c8 = i - row * C8;
            if (i < kTile * C8) {
                *reinterpret_cast<bf16x8 *>(Xs + row * STR + 16 * c8) = xreg[n];
                *reinterpret_cast<bf16x8 *>(Ys + row * STR + 16 * c8) = yreg[n];
            }
        }
    };

    f32x4 acc1[ND], acc2[ND];     // KEYS: dk^T, dv^T; else dq^T (acc2 unused)
#pragma unroll
    for (int j = 0; j < ND; ++j) acc1[j] = acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int roff = lq * STR + 16 * g;                                  // + sub * 16 * STR + 64 * s
    const int toff = (4 * g + (lq >> 2)) * STR + 8 * (lq & 3);          // + kb * 32 * STR + 32 * db

    gload(0);
    for (int tile = 0; tile < p.nt; ++tile) {
        __syncthreads();
        lstore();
        __syncthreads();

        f32x4 S[4], dP[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) S[sub] = dP[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < NK; ++s) {
            // head_dim 80, third k-step: lane groups 2 and 3 stand for d >= 80; they re-read a valid chunk and use zeros
            const bool dead = HD == 80 && s == 2 && g >= 2;
            const int off = roff + 64 * s - (dead ? 32 : 0);
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) {
                bf16x8 xf = *reinterpret_cast<const bf16x8 *>(Xs + sub * 16 * STR + off);
                bf16x8 yf = *reinterpret_cast<const bf16x8 *>(Ys + sub * 16 * STR + off);
                if (dead) xf = yf = zero8();
                S[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, a[s], S[sub], 0, 0, 0);
                dP[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yf, bb[s], dP[sub], 0, 0, 0);
            }
        }

        if (tile + 1 < p.nt) gload(tile + 1);

        // S -> P (kept in S), dP -> dS (kept in dP), both f32
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int t0 = tile * kTile + sub * 16 + 4 * g;
            f32x4 ls, dl, bias = {0.f, 0.f, 0.f, 0.f};
            if (KEYS) {
                ls = *reinterpret_cast<const f32x4 *>(lse_w + t0);
                dl = *reinterpret_cast<const f32x4 *>(delta_w + t0);
                if (rel) {
                    const f32x4 thv = *reinterpret_cast<const f32x4 *>(p.thT + (grp * p.win_h + o_h) * p.Tp + t0);
                    const f32x4 twv = *reinterpret_cast<const f32x4 *>(p.twT + (grp * p.win_w + o_w) * p.Tp + t0);
                    bias = thv + twv;
                }
            } else {
                ls = f32x4{lse_o, lse_o, lse_o, lse_o};
                dl = f32x4{delta_o, delta_o, delta_o, delta_o};
                if (rel) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int tc = min(t0 + r, p.T - 1);
                        const int kh = slot_row(tc, p.inv_win_w), kw = tc - kh * p.win_w;
                        bias[r] = p.th[(grp * p.Tp + o) * p.win_h + kh] + p.tw[(grp * p.Tp + o) * p.win_w + kw];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // the forward's logit: the scale multiplies the f32 accumulator, T_h + T_w is added in f32
                const float s = rel ? fmaf(S[sub][r], p.scale2, bias[r]) : S[sub][r] * p.scale2;
                float pr = __builtin_amdgcn_exp2f(s - ls[r]);      // lse = +inf (not a query): exactly 0
                if (KEYS ? o >= p.T : t0 + r >= p.T) pr = 0.f;      // a key past the window
                S[sub][r] = pr;
                dP[sub][r] = pr * (dP[sub][r] - dl[r]);
            }
        }

        if (!KEYS && rel) {
            // A_h[query][kh] += dS, A_w[query][kw] += dS in f32, in the f32 adjoint's fixed order (csrc/vit_grad.hip): the four lanes
            // of a query hold keys 4 apart; A_w is added by all lanes at once unless the window is so narrow that they meet on a kw,
            // A_h by the four lanes in turn, each lane adding its run of keys of one row as one sum.  The LDS operations of one wave
            // complete in issue order; between two turns stands a wavefront-scope fence and a wave barrier.
            float *ahrow = Ahs + myrow * p.ah_ld, *awrow = Aws + myrow * p.aw_ld;
            const bool aw_meets = 4 % p.win_w == 0 || 8 % p.win_w == 0 || 12 % p.win_w == 0;
            for (int gg = 0; gg < 4; ++gg) {
                if (g == gg) {
                    int cur = -1;
                    float run = 0.f;
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int t = tile * kTile + sub * 16 + 4 * g + r;
                            if (t < p.T) {
                                const int kh = slot_row(t, p.inv_win_w), kw = t - kh * p.win_w;
                                if (kh != cur) {
                                    if (cur >= 0) ahrow[cur] += run;
                                    cur = kh, run = 0.f;
                                }
                                run += dP[sub][r];
                                if (aw_meets) awrow[kw] += dP[sub][r];
                            }
                        }
                    if (cur >= 0) ahrow[cur] += run;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (!aw_meets) {
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int t = tile * kTile + sub * 16 + 4 * g + r;
                        if (t < p.T) {
                            const int kh = slot_row(t, p.inv_win_w);
                            awrow[t - kh * p.win_w] += dP[sub][r];
                        }
                    }
            }
        }

        // P and dS rounded to bf16 once: registers 0..3 of sub-tiles 2 kb and 2 kb + 1 are slots 0..7 of k-step kb, as they stand
        bf16x8 pf[2], df[2];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pf[sub >> 1][4 * (sub & 1) + r] = (__bf16)S[sub][r];
                df[sub >> 1][4 * (sub & 1) + r] = (__bf16)dP[sub][r];
            }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int db = 0; db < ND; ++db) {
                const int off = toff + kb * 32 * STR + 32 * db;
                if (KEYS) acc2[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_read8(Ys, off, off + 16 * STR), pf[kb], acc2[db], 0, 0, 0);
                acc1[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_read8(Xs, off, off + 16 * STR), df[kb], acc1[db], 0, 0, 0);
            }
    }

    // row 4 g + r of accumulator db is d = 16 db + 4 g + r of owned slot lq: staged as f32 rows [owned][d]
#pragma unroll
    for (int db = 0; db < ND; ++db) {
        *reinterpret_cast<f32x4 *>(St1 + myrow * LD + 16 * db + 4 * g) = acc1[db] * p.scale;
        if (KEYS) *reinterpret_cast<f32x4 *>(St2 + myrow * LD + 16 * db + 4 * g) = acc2[db];
    }
    __syncthreads();
    if (KEYS) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int row = i / C8, c8 = i - row * C8;
            const int t = ot * kTile + row;
            if (i < kTile * C8 && t < p.T) {
                const long long pix = slot_pixel(p, gr, t);
                if (pix >= 0) {
                    bf16x8 k8, v8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        k8[e] = (__bf16)St1[row * LD + 8 * c8 + e];
                        v8[e] = (__bf16)St2[row * LD + 8 * c8 + e];
                    }
                    __bf16 *dst = p.dqkv + pix * 3 * C + C + gr.head * HD + 8 * c8;
                    *reinterpret_cast<bf16x8 *>(dst) = k8;
                    *reinterpret_cast<bf16x8 *>(dst + C) = v8;
                }
            }
        }
        if (tid < 2 * C4) {      // the padding slots of this tile, in slot order, in f32
            const int which = tid / C4, c4 = tid - which * C4;
            const float *src = (which ? St2 : St1) + 4 * c4;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int row = 0; row < kTile; ++row) {
                const int t = ot * kTile + row;
                if (t < p.T && slot_pixel(p, gr, t) < 0) s += *reinterpret_cast<const f32x4 *>(src + row * LD);
            }
            *reinterpret_cast<f32x4 *>(p.padpart + ((long long)blockIdx.x * 2 + which) * HD + 4 * c4) = s;
        }
    } else {
        if (rel) {
            for (int i = tid; i < kTile * p.win_h; i += kBlock) {
                const int row = i / p.win_h, k = i - row * p.win_h;
                p.ah[(grp * p.Tp + ot * kTile + row) * p.win_h + k] = Ahs[row * p.ah_ld + k];
            }
            for (int i = tid; i < kTile * p.win_w; i += kBlock) {
                const int row = i / p.win_w, k = i - row * p.win_w;
                p.aw[(grp * p.Tp + ot * kTile + row) * p.win_w + k] = Aws[row * p.aw_ld + k];
            }
        }
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int row = i / C8, c8 = i - row * C8;
            const int t = ot * kTile + row;
            if (i >= kTile * C8 || t >= p.T) continue;
            const long long pix = slot_pixel(p, gr, t);
            if (pix < 0) continue;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = St1[row * LD + 8 * c8 + e];
            if (rel) {
                // the table rows as the forward read them: rounded to bf16
                const int ih = t / p.win_w, iw = t - ih * p.win_w;
                for (int k = 0; k < p.win_h; ++k) {
                    const bf16x8 tr = cvt8(p.rh + (long long)(ih - k + p.win_h - 1) * HD + 8 * c8);
                    const float w = Ahs[row * p.ah_ld + k];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaf(w, (float)tr[e], v[e]);
                }
                for (int k = 0; k < p.win_w; ++k) {
                    const bf16x8 tr = cvt8(p.rw + (long long)(iw - k + p.win_w - 1) * HD + 8 * c8);
                    const float w = Aws[row * p.aw_ld + k];
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaf(w, (float)tr[e], v[e]);
                }
            }
            bf16x8 q8;
#pragma unroll
            for (int e = 0; e < 8; ++e) q8[e] = (__bf16)v[e];
            *reinterpret_cast<bf16x8 *>(p.dqkv + pix * 3 * C + gr.head * HD + 8 * c8) = q8;
        }
    }
}

// dR_h[r] and dR_w[r] of one group, as attn_bwd_table_kernel of csrc/vit_grad.hip: blockIdx = (group, table row of either axis),
// threadIdx.x = 4 channels, threadIdx.y = one of eight slices of the window's columns, each summed in slot order in f32; the
// slices are added in slice order.  q is the stored bf16 value, unscaled.
constexpr int kTabSlices = 8;
__global__ __launch_bounds__(32 * kTabSlices) void attn_bwd16_table_kernel(BwdParams p) {
    __shared__ f32x4 part[kTabSlices][32];
    const int rows_h = 2 * p.win_h - 1, rows_w = 2 * p.win_w - 1;
    const long long grp = blockIdx.x / (rows_h + rows_w);
    int r = (int)(blockIdx.x - grp * (rows_h + rows_w));
    const bool ax = r >= rows_h;
    if (ax) r -= rows_h;
    const int c4 = threadIdx.x, slice = threadIdx.y, HD = p.HD, C = p.nH * HD;
    const bool live = 4 * c4 < HD;
    const Window gr = decode_window(p, grp);
    const int win = ax ? p.win_w : p.win_h;
    const int off = r - (win - 1);         // query position minus key position
    const float *A = (ax ? p.aw : p.ah) + grp * p.Tp * win;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    const int nh = min(p.win_h, p.H - gr.h0), nw = min(p.win_w, p.W - gr.w0);     // the real tokens of the window
    if (live)
        for (int ih = 0; ih < nh; ++ih) {
            if (!ax && (ih - off < 0 || ih - off >= win)) continue;
            for (int iw = slice; iw < nw; iw += kTabSlices) {
                const int k = (ax ? iw : ih) - off;
                if (k < 0 || k >= win) continue;
                const int i = ih * p.win_w + iw;
                const float w = A[(long long)i * win + k];
                const long long pix = ((long long)gr.b * p.H + gr.h0 + ih) * p.W + gr.w0 + iw;
                const bf16x4 q = *reinterpret_cast<const bf16x4 *>(p.qkv + pix * 3 * C + gr.head * HD + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] = fmaf(w, (float)q[e], s[e]);
            }
        }
    part[slice][c4] = s;
    __syncthreads();
    if (slice == 0 && live) {
        for (int k = 1; k < kTabSlices; ++k) s += part[k][c4];
        float *dst = (ax ? p.relw : p.relh) + (grp * (ax ? rows_w : rows_h) + r) * HD + 4 * c4;
        *reinterpret_cast<f32x4 *>(dst) = s;
    }
}

// The partials in workgroup order: dpad_qkv (q part zero), drel_pos_h, drel_pos_w.  One thread per four outputs.
__global__ __launch_bounds__(kBlock) void attn_bwd16_finish_kernel(BwdParams p) {
    const int HD = p.HD, C = p.nH * HD, C4 = HD / 4;
    const long long n_pad = p.dpad ? 3LL * C / 4 : 0;
    const long long n_h = p.drh ? (2LL * p.win_h - 1) * C4 : 0, n_w = p.drw ? (2LL * p.win_w - 1) * C4 : 0;
    long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i < n_pad) {
        const int which = (int)(i / (C / 4));      // 0 q, 1 k, 2 v
        const int ch = 4 * (int)(i - (long long)which * (C / 4));
        const int head = ch / HD, d = ch - head * HD;
        if (which > 0) {
            const long long per_head = (long long)p.nwy * p.nwx * p.nt;      // workgroups of one (image, head)
            for (int b = 0; b < p.B; ++b)
                for (long long k = 0; k < per_head; ++k)
                    s += *reinterpret_cast<const f32x4 *>(p.padpart + ((((long long)b * p.nH + head) * per_head + k) * 2 + (which - 1)) * HD + d);
        }
        *reinterpret_cast<f32x4 *>(p.dpad + 4 * i) = s;
        return;
    }
    i -= n_pad;
    if (i < n_h + n_w) {
        const bool ax = i >= n_h;
        if (ax) i -= n_h;
        const long long rows = 2LL * (ax ? p.win_w : p.win_h) - 1;
        const float *part = ax ? p.relw : p.relh;
        for (long long g = 0; g < p.G; ++g) s += *reinterpret_cast<const f32x4 *>(part + g * rows * HD + 4 * i);
        *reinterpret_cast<f32x4 *>((ax ? p.drw : p.drh) + 4 * i) = s;
    }
}

template <int HD, bool KEYS>
int launch_bwd(const BwdParams &p, long long blocks, size_t lds_bytes, hipStream_t stream) {
    static PerDeviceSize state;
    if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_bwd16_kernel<HD, KEYS>), lds_bytes, state))
        return fail(SGV3D_ELAUNCH, "vit_attention_bf16_backward: cannot reserve %zu bytes of LDS", lds_bytes);
    hipLaunchKernelGGL((attn_bwd16_kernel<HD, KEYS>), dim3((unsigned)blocks), dim3(kBlock), lds_bytes, stream, p);
    return check_launch(KEYS ? "attn_bwd16_kernel<keys>" : "attn_bwd16_kernel<queries>");
}

template <int HD>
int launch_all(const BwdParams &p, const BwdLayout &L, bool rel, hipStream_t s) {
    hipLaunchKernelGGL(attn_bwd16_prep_kernel<HD>, dim3((unsigned)(L.G * L.nt)), dim3(kBlock), 0, s, p);
    int r = check_launch("attn_bwd16_prep_kernel");
    if (r != SGV3D_OK) return r;
    const size_t lds_keys = BwdGeom<HD>::bytes, lds_q = lds_keys + sizeof(float) * (size_t)kTile * (p.ah_ld + p.aw_ld);
    // lds_q is at most 2 * 64 * 160 + 2 * 64 * 88 * 4 + 64 * (129 + 129) * 4 = 131 584 bytes of the 160 KB: the window is at most 128 x 128
    r = launch_bwd<HD, true>(p, L.G * L.nt, lds_keys, s);
    if (r != SGV3D_OK) return r;
    r = launch_bwd<HD, false>(p, L.G * L.nt, lds_q, s);
    if (r != SGV3D_OK) return r;
    if (rel) {
        hipLaunchKernelGGL(attn_bwd16_table_kernel, dim3((unsigned)(L.G * (2LL * p.win_h + 2LL * p.win_w - 2))), dim3(32, kTabSlices), 0, s, p);
        r = check_launch("attn_bwd16_table_kernel");
        if (r != SGV3D_OK) return r;
    }
    const long long n_fin = (p.dpad ? 3LL * p.nH * HD / 4 : 0) + (rel ? (2LL * p.win_h + 2LL * p.win_w - 2) * (HD / 4) : 0);
    if (n_fin > 0) {
        hipLaunchKernelGGL(attn_bwd16_finish_kernel, dim3((unsigned)cdiv(n_fin, kBlock)), dim3(kBlock), 0, s, p);
        r = check_launch("attn_bwd16_finish_kernel");
    }
    return r;
}

}  // namespace

extern "C" size_t sgv3d_vit_attention_bf16_backward_workspace_bytes(const sgv3d_vit_attn_desc *desc) {
    if (check_attn_desc("vit_attention_bf16_backward_workspace_bytes", desc, 8) != SGV3D_OK) return 0;
    return sizeof(float) * (size_t)bwd_layout(*desc, true).total;     // with tables: an upper bound for the call without
}

extern "C" int sgv3d_vit_attention_bf16_backward(const sgv3d_vit_attn_desc *desc, const void *qkv, const float *pad_qkv,
                                                 const float *rel_pos_h, const float *rel_pos_w, const void *out, const float *lse,
                                                 const void *dout, void *dqkv, float *dpad_qkv, float *drel_pos_h, float *drel_pos_w,
                                                 void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = check_attn_desc("vit_attention_bf16_backward", desc, 8);
    if (rc != SGV3D_OK) return rc;
    const sgv3d_vit_attn_desc &d = *desc;
    SGV3D_REQUIRE((rel_pos_h == nullptr) == (rel_pos_w == nullptr),
                  "vit_attention_bf16_backward: rel_pos_h and rel_pos_w must be given together or not at all");
    const bool rel = rel_pos_h != nullptr;
    SGV3D_REQUIRE(qkv && out && lse && dout && dqkv, "vit_attention_bf16_backward: null qkv, out, lse, dout or dqkv");
    SGV3D_REQUIRE(!pad_qkv || dpad_qkv, "vit_attention_bf16_backward: pad_qkv is given, dpad_qkv is null");
    SGV3D_REQUIRE(rel ? (drel_pos_h && drel_pos_w) : (!drel_pos_h && !drel_pos_w),
                  "vit_attention_bf16_backward: drel_pos_h and drel_pos_w must be given exactly when the tables are");
    SGV3D_REQUIRE(aligned16(qkv) && aligned16(pad_qkv) && aligned16(rel_pos_h) && aligned16(rel_pos_w) && aligned16(out) &&
                      aligned16(lse) && aligned16(dout) && aligned16(dqkv) && aligned16(dpad_qkv) && aligned16(drel_pos_h) &&
                      aligned16(drel_pos_w) && aligned16(workspace),
                  "vit_attention_bf16_backward: every pointer must be 16-byte aligned");
    // dqkv is written by the key-owning launch while the query-owning launch still reads qkv, out and dout
    const unsigned long long tokens = (unsigned long long)d.batch * d.height * d.width, cbytes = 2ULL * d.heads * d.head_dim;
    SGV3D_REQUIRE(!overlaps(dqkv, 3 * tokens * cbytes, qkv, 3 * tokens * cbytes) && !overlaps(dqkv, 3 * tokens * cbytes, out, tokens * cbytes) &&
                      !overlaps(dqkv, 3 * tokens * cbytes, dout, tokens * cbytes),
                  "vit_attention_bf16_backward: dqkv must not overlap qkv, out or dout");
    const BwdLayout L = bwd_layout(d, rel);
    SGV3D_REQUIRE(L.G * L.Tp < (1LL << 31) && L.G * (2LL * d.win_h + 2LL * d.win_w) < (1LL << 31),
                  "vit_attention_bf16_backward: too many workgroups");
    if (!workspace || workspace_bytes < sizeof(float) * (size_t)L.total)
        return fail(SGV3D_ENOSPACE, "vit_attention_bf16_backward: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0,
                    sizeof(float) * (size_t)L.total);

    BwdParams p;
    fill_window(p, d);
    p.HD = d.head_dim, p.Tp = (int)L.Tp, p.nt = (int)L.nt, p.ah_ld = odd_ld(rel, d.win_h), p.aw_ld = odd_ld(rel, d.win_w);
    p.scale = softmax_scale(d.head_dim);
    p.scale2 = p.scale * kLog2e;
    p.qkv = static_cast<const __bf16 *>(qkv), p.out = static_cast<const __bf16 *>(out), p.dout = static_cast<const __bf16 *>(dout);
    p.pad = pad_qkv, p.rh = rel_pos_h, p.rw = rel_pos_w, p.lse = lse;
    p.dqkv = static_cast<__bf16 *>(dqkv), p.dpad = dpad_qkv, p.drh = drel_pos_h, p.drw = drel_pos_w;
    float *ws = static_cast<float *>(workspace);
    p.lse_w = ws + L.lse_w, p.delta_w = ws + L.delta_w, p.th = ws + L.th, p.tw = ws + L.tw, p.thT = ws + L.thT, p.twT = ws + L.twT;
    p.ah = ws + L.ah, p.aw = ws + L.aw, p.padpart = ws + L.padpart, p.relh = ws + L.relh, p.relw = ws + L.relw;
    p.G = L.G;
    hipStream_t s = as_stream(stream);
    switch (d.head_dim) {
        case 32: return launch_all<32>(p, L, rel, s);
        case 64: return launch_all<64>(p, L, rel, s);
        default: return launch_all<80>(p, L, rel, s);
    }
}
