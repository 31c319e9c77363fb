// Training adjoints of SAM's ViT image encoder (csrc/vit.hip): the attention launch with windows, padding tokens and the decomposed
// relative position, LayerNorm, the exact GELU and the crop + bilinear resize.  gfx950 only.  Vector stores only, no float atomics,
// a fixed summation order everywhere: every entry is repeatable bit for bit and graph-capturable (no host wait, no allocation).
// What must repeat the forward bit for bit (the window geometry, the LayerNorm row statistics, the erf term of GELU, the f32 MFMA
// operand code) is the forward's own definition, from csrc/vit_common.hpp.
#include "vit_common.hpp"

using namespace sgv3d;

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 64;     // owned rows per workgroup (16 per wave) and streamed rows per LDS tile
constexpr int kLnChunk = 32;  // rows per partial of the LayerNorm weight / bias gradient

static inline long long up4(long long v) { return (v + 3) & ~3LL; }
// two ranges of `bytes` bytes each
static inline bool overlaps(const void *a, const void *b, unsigned long long bytes) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return (pa > pb ? pa - pb : pb - pa) < bytes;
}

// ------------------------------------------------------------------------------------------------
// attention backward
// ------------------------------------------------------------------------------------------------
// Per (image, head, window) "group" with T = win_h * win_w slots (Tp = T rounded up to 64) the workspace holds, in floats:
//   lse_w, delta_w [G][Tp]          lse of the slot as a query (+inf for a padding slot or a slot past T: its P is exactly 0, so it
//                                   is never a query) and delta = dO . O (0 there)
//   th [G][Tp][win_h], tw [G][Tp][win_w]      q_i . R_h[ih - kh + win_h - 1] and q_i . R_w[...] (unscaled q), row per query
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
    float scale, inv_win_w;
    const float *qkv, *pad, *rh, *rw, *out, *lse, *dout;
    float *dqkv, *dpad, *drh, *drw;
    float *lse_w, *delta_w, *th, *tw, *thT, *twT, *ah, *aw, *padpart, *relh, *relw;
    long long G;
};

// pixel index ((b * H + h) * W + w) of window slot t (< T), or -1 for a padding slot
__device__ inline long long slot_pixel(const BwdParams &p, const Window &gr, int t) {
    const int kh = t / p.win_w;
    long long pix;
    return gr.pixel(p, kh, t - kh * p.win_w, pix) ? pix : -1;
}

// One workgroup of 64 threads per (group, slot): the slot's lse and delta and its row of th / tw.
__global__ __launch_bounds__(64) void attn_bwd_prep_kernel(BwdParams p) {
    const long long bid = blockIdx.x;
    const long long g = bid / p.Tp;
    const int i = (int)(bid - g * p.Tp);
    const Window gr = decode_window(p, g);
    const int HD = p.HD, C = p.nH * HD;
    const long long pix = i < p.T ? slot_pixel(p, gr, i) : -1;
    const bool rel = p.rh != nullptr;
    const int ih = i / p.win_w, iw = i - ih * p.win_w;
    const int items = (rel ? p.win_h + p.win_w : 0) + 1;
    for (int it = threadIdx.x; it < items; it += 64) {
        if (it == items - 1) {
            float dl = 0.f, ls = INFINITY;
            if (pix >= 0) {
                const float *o = p.out + pix * C + gr.head * HD, *dO = p.dout + pix * C + gr.head * HD;
                for (int d = 0; d < HD; d += 4) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(o + d), b = *reinterpret_cast<const f32x4 *>(dO + d);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dl = fmaf(a[e], b[e], dl);
                }
                ls = p.lse[(((long long)gr.b * p.nH + gr.head) * p.H + (pix / p.W) % p.H) * p.W + pix % p.W];
            }
            p.lse_w[g * p.Tp + i] = ls;
            p.delta_w[g * p.Tp + i] = dl;
            continue;
        }
        const bool ax = it >= p.win_h;     // 0: height axis, 1: width axis
        const int kpos = ax ? it - p.win_h : it, win = ax ? p.win_w : p.win_h, qpos = ax ? iw : ih;
        float s = 0.f;
        if (pix >= 0) {
            const float *q = p.qkv + pix * 3 * C + gr.head * HD;
            const float *row = (ax ? p.rw : p.rh) + (long long)(qpos - kpos + win - 1) * HD;
            for (int d = 0; d < HD; d += 4) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(q + d), b = *reinterpret_cast<const f32x4 *>(row + d);
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fmaf(a[e], b[e], s);
            }
        }
        (ax ? p.tw : p.th)[(g * p.Tp + i) * win + kpos] = s;
        (ax ? p.twT : p.thT)[(g * win + kpos) * p.Tp + i] = s;
    }
}

template <int HD>
struct BwdGeom {
    static constexpr int LD = HD + 8;   // LDS row of both streamed tiles
    static constexpr int floats = 2 * kTile * LD;
};

// All products are v_mfma_f32_16x16x4_f32 in the operand layouts of the forward (csrc/vit.hip).  A wave OWNS 16 columns (one per
// lane & 15; the four lanes of a column hold a quarter of the head dimension each) and the workgroup streams 64-row tiles of two
// tensors X, Y through LDS:
//   KEYS = false  owned: queries (a = scale q, bb = dO), streamed: X = K, Y = V.   dq^T += K^T dS^T.   A_h, A_w accumulate in LDS.
//   KEYS = true   owned: keys (a = k, bb = v),        streamed: X = scale Q, Y = dO.   dv^T += dO^T P,  dk^T += (scale Q)^T dS.
// S and dP come out as [streamed row 4 g + r of a 16-row sub-tile][owned column], which is the B operand of the second product as
// it stands.  P = exp(S - lse) is recomputed per tile; nothing of size tokens x keys is stored.
template <int HD, bool KEYS>
__global__ __launch_bounds__(kBlock) void attn_bwd_kernel(BwdParams p) {
    constexpr int LD = BwdGeom<HD>::LD;
    constexpr int NC = HD / 16, NS = HD / 4, NJ = HD / 16;
    constexpr int NL = HD / 16, C4 = HD / 4;
    extern __shared__ __align__(16) float lds[];
    float *Xs = lds;
    float *Ys = Xs + kTile * LD;
    float *Ahs = Ys + kTile * LD;            // [64][ah_ld]   (KEYS = false with tables only)
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

    float a[NS], bb[NS];
    {
        const float *sa = nullptr, *sb = nullptr;
        if (KEYS) {
            if (opix >= 0) sa = p.qkv + opix * 3 * C + C + gr.head * HD, sb = sa + C;
            else if (p.pad) sa = p.pad + C + gr.head * HD, sb = sa + C;
        } else if (opix >= 0) {
            sa = p.qkv + opix * 3 * C + gr.head * HD, sb = p.dout + opix * C + gr.head * HD;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
            if (sa) va = *reinterpret_cast<const f32x4 *>(sa + 16 * c + 4 * g), vb = *reinterpret_cast<const f32x4 *>(sb + 16 * c + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[4 * c + i] = KEYS ? va[i] : va[i] * p.scale;
                bb[4 * c + i] = vb[i];
            }
        }
    }
    const float lse_o = KEYS ? 0.f : lse_w[o], delta_o = KEYS ? 0.f : delta_w[o];

    if (!KEYS && rel)
        for (int i = tid; i < kTile * (p.ah_ld + p.aw_ld); i += kBlock) Ahs[i] = 0.f;

    f32x4 xreg[NL], yreg[NL];
    auto gload = [&](int tile) {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int row = i / C4, c4 = i - row * C4;
            const int t = tile * kTile + row;
            f32x4 xv = {0.f, 0.f, 0.f, 0.f}, yv = {0.f, 0.f, 0.f, 0.f};
            if (t < p.T) {
                const long long pix = slot_pixel(p, gr, t);
                if (KEYS) {
                    if (pix >= 0) {
                        xv = *reinterpret_cast<const f32x4 *>(p.qkv + pix * 3 * C + gr.head * HD + 4 * c4) * p.scale;     // the forward's scaled q
                        yv = *reinterpret_cast<const f32x4 *>(p.dout + pix * C + gr.head * HD + 4 * c4);
                    }
                } else {
                    const float *src = pix >= 0 ? p.qkv + pix * 3 * C + C + gr.head * HD : p.pad ? p.pad + C + gr.head * HD : nullptr;
                    if (src) {
                        xv = *reinterpret_cast<const f32x4 *>(src + 4 * c4);
                        yv = *reinterpret_cast<const f32x4 *>(src + C + 4 * c4);
                    }
                }
            }
            xreg[n] = xv;
            yreg[n] = yv;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int row = i / C4, c4 = i - row * C4;
            *reinterpret_cast<f32x4 *>(Xs + row * LD + 4 * c4) = xreg[n];
            *reinterpret_cast<f32x4 *>(Ys + row * LD + 4 * c4) = yreg[n];
        }
    };
    // acc^T[d][owned] += sum over the tile's rows of M[row][d] * Wt[row][owned]
    auto accum = [&](f32x4(&acc)[NJ], const float *M, const f32x4(&Wt)[4]) { accum_rows<HD, LD>(acc, M + 4 * g * LD, Wt, lq); };
    // stage acc^T (times mul) as rows [owned][d] of an LDS tile with row length LD
    auto stage = [&](float *dst_tile, const f32x4(&acc)[NJ], float mul) {
        store_rows<HD>(dst_tile + myrow * LD, acc, g, [mul](float v) { return v * mul; });
    };

    f32x4 acc1[NJ], acc2[NJ];     // KEYS: dk^T, dv^T; else dq^T (acc2 unused)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc1[j] = acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *xbase = Xs + lq * LD + 4 * g, *ybase = Ys + lq * LD + 4 * g;

    gload(0);
    for (int tile = 0; tile < p.nt; ++tile) {
        __syncthreads();
        lstore();
        __syncthreads();

        f32x4 S[4], dP[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) S[sub] = dP[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x4 xf[4], yf[4];
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) {
                xf[sub] = *reinterpret_cast<const f32x4 *>(xbase + sub * 16 * LD + 16 * c);
                yf[sub] = *reinterpret_cast<const f32x4 *>(ybase + sub * 16 * LD + 16 * c);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    S[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(xf[sub][i], a[4 * c + i], S[sub], 0, 0, 0);
                    dP[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(yf[sub][i], bb[4 * c + i], dP[sub], 0, 0, 0);
                }
        }

        if (tile + 1 < p.nt) gload(tile + 1);

        // S -> P (kept in S), dP -> dS (kept in dP)
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int t0 = tile * kTile + sub * 16 + 4 * g;
            f32x4 ls, dl, thv = {0.f, 0.f, 0.f, 0.f}, twv = {0.f, 0.f, 0.f, 0.f};
            if (KEYS) {
                ls = *reinterpret_cast<const f32x4 *>(lse_w + t0);
                dl = *reinterpret_cast<const f32x4 *>(delta_w + t0);
                if (rel) {
                    thv = *reinterpret_cast<const f32x4 *>(p.thT + (grp * p.win_h + o_h) * p.Tp + t0);
                    twv = *reinterpret_cast<const f32x4 *>(p.twT + (grp * p.win_w + o_w) * p.Tp + t0);
                }
            } else {
                ls = f32x4{lse_o, lse_o, lse_o, lse_o};
                dl = f32x4{delta_o, delta_o, delta_o, delta_o};
                if (rel) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int tc = min(t0 + r, p.T - 1);
                        const int kh = slot_row(tc, p.inv_win_w), kw = tc - kh * p.win_w;
                        thv[r] = p.th[(grp * p.Tp + o) * p.win_h + kh];
                        twv[r] = p.tw[(grp * p.Tp + o) * p.win_w + kw];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = S[sub][r] + (thv[r] + twv[r]);      // (scale q) . k in the forward's summation order, both ways
                float pr = __expf(s - ls[r]);                 // lse = +inf (not a query): exactly 0
                if (!KEYS && t0 + r >= p.T) pr = 0.f;         // a key past the window
                S[sub][r] = pr;
                dP[sub][r] = pr * (dP[sub][r] - dl[r]);
            }
        }

        if (KEYS) {
            accum(acc2, Ys, S);      // dv^T += dO^T P
            accum(acc1, Xs, dP);     // dk^T += Q^T dS
        } else {
            accum(acc1, Xs, dP);     // dq^T += K^T dS^T
            if (rel) {
                // A_h[query][kh] += dS, A_w[query][kw] += dS, in a fixed order and with no two lanes on one address at a time.  The four
                // lanes of a query hold keys 4 apart: they meet on a kw only if win_w divides 4, 8 or 12, and on a kh almost always.
                // So A_w is added by all lanes at once unless the window is that narrow, and A_h by the four lanes in turn, each
                // lane adding its run of keys of one row as one sum.  What keeps the turns in order: the LDS operations of one
                // wave complete in the order they are issued (one in-order LDS queue per wave), and between two turns stands a
                // wavefront-scope acquire-release fence, across which the compiler may move no load or store of LDS, with a wave
                // barrier that keeps the scheduler from moving anything else.
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
        }
    }

    __syncthreads();     // the last tile has been read
    if (KEYS) {
        stage(Xs, acc1, 1.0f);      // Q was scaled on the way in
        stage(Ys, acc2, 1.0f);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NL; ++n) {
            const int i = tid + kBlock * n;
            const int row = i / C4, c4 = i - row * C4;
            const int t = ot * kTile + row;
            if (t < p.T) {
                const long long pix = slot_pixel(p, gr, t);
                if (pix >= 0) {
                    float *dst = p.dqkv + pix * 3 * C + C + gr.head * HD + 4 * c4;
                    *reinterpret_cast<f32x4 *>(dst) = *reinterpret_cast<const f32x4 *>(Xs + row * LD + 4 * c4);
                    *reinterpret_cast<f32x4 *>(dst + C) = *reinterpret_cast<const f32x4 *>(Ys + row * LD + 4 * c4);
                }
            }
        }
        if (tid < 2 * C4) {      // the padding slots of this tile, in slot order
            const int which = tid / C4, c4 = tid - which * C4;
            const float *src = (which ? Ys : Xs) + 4 * c4;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            for (int row = 0; row < kTile; ++row) {
                const int t = ot * kTile + row;
                if (t < p.T && slot_pixel(p, gr, t) < 0) s += *reinterpret_cast<const f32x4 *>(src + row * LD);
            }
            *reinterpret_cast<f32x4 *>(p.padpart + ((long long)blockIdx.x * 2 + which) * HD + 4 * c4) = s;
        }
    } else {
        stage(Xs, acc1, p.scale);
        __syncthreads();
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
            const int row = i / C4, c4 = i - row * C4;
            const int t = ot * kTile + row;
            if (t >= p.T) continue;
            const long long pix = slot_pixel(p, gr, t);
            if (pix < 0) continue;
            f32x4 v = *reinterpret_cast<const f32x4 *>(Xs + row * LD + 4 * c4);
            if (rel) {
                const int ih = t / p.win_w, iw = t - ih * p.win_w;
                for (int k = 0; k < p.win_h; ++k) {
                    const f32x4 tr = *reinterpret_cast<const f32x4 *>(p.rh + (long long)(ih - k + p.win_h - 1) * HD + 4 * c4);
                    const float w = Ahs[row * p.ah_ld + k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaf(w, tr[e], v[e]);
                }
                for (int k = 0; k < p.win_w; ++k) {
                    const f32x4 tr = *reinterpret_cast<const f32x4 *>(p.rw + (long long)(iw - k + p.win_w - 1) * HD + 4 * c4);
                    const float w = Aws[row * p.aw_ld + k];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaf(w, tr[e], v[e]);
                }
            }
            *reinterpret_cast<f32x4 *>(p.dqkv + pix * 3 * C + gr.head * HD + 4 * c4) = v;
        }
    }
}

// dR_h[r] and dR_w[r] of one group: blockIdx = (group, table row of either axis), threadIdx.x = 4 channels, threadIdx.y = one of
// eight slices of the window's columns (iw = slice, slice + 8, ...), each summed in slot order; the slices are added in slice order.
constexpr int kTabSlices = 8;
__global__ __launch_bounds__(32 * kTabSlices) void attn_bwd_table_kernel(BwdParams p) {
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
                const f32x4 q = *reinterpret_cast<const f32x4 *>(p.qkv + pix * 3 * C + gr.head * HD + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] = fmaf(w, q[e], s[e]);
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
__global__ __launch_bounds__(kBlock) void attn_bwd_finish_kernel(BwdParams p) {
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
    if (!ensure_dynamic_lds(reinterpret_cast<const void *>(attn_bwd_kernel<HD, KEYS>), lds_bytes, state))
        return fail(SGV3D_ELAUNCH, "vit_attention_backward: cannot reserve %zu bytes of LDS", lds_bytes);
    hipLaunchKernelGGL((attn_bwd_kernel<HD, KEYS>), dim3((unsigned)blocks), dim3(kBlock), lds_bytes, stream, p);
    return check_launch(KEYS ? "attn_bwd_kernel<keys>" : "attn_bwd_kernel<queries>");
}

template <bool KEYS>
int launch_bwd_hd(const BwdParams &p, long long blocks, size_t lds_bytes, hipStream_t stream) {
    switch (p.HD) {
        case 32: return launch_bwd<32, KEYS>(p, blocks, lds_bytes, stream);
        case 64: return launch_bwd<64, KEYS>(p, blocks, lds_bytes, stream);
        default: return launch_bwd<80, KEYS>(p, blocks, lds_bytes, stream);
    }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm backward
// ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// four values of dy as f32: the f32 tensor's own, or the bf16 tensor's widened (exact), so that sgv3d_layernorm_backward_bf16dy
// does the arithmetic of sgv3d_layernorm_backward on dy.float()
__device__ __forceinline__ f32x4 widen4(const f32x4 v) { return v; }
__device__ __forceinline__ f32x4 widen4(const bf16x4 v) { return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}; }

// One wave per row: the forward's mean and rstd (ln_row_stats), the two row sums of the gradient in f64, dx; the row's mean and rstd
// go to the workspace for the weight / bias partials.  DY4: f32x4 or bf16x4.
template <class DY4>
__global__ __launch_bounds__(kBlock) void layernorm_bwd_dx_kernel(long long rows, int c4, const f32x4 *__restrict__ x,
                                                                  const f32x4 *__restrict__ weight, float eps, const DY4 *dy, f32x4 *dx,
                                                                  double *stats) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const f32x4 *xr = x + row * c4;
    const DY4 *gr = dy + row * c4;
    f32x4 *dr = dx + row * c4;
    const double inv_c = 1.0 / (4.0 * (double)c4);
    const LnStats st = ln_row_stats(xr, c4, lane, eps);
    double s1 = 0.0, s2 = 0.0;
    for (int i = lane; i < c4; i += 64) {
        const f32x4 v = xr[i], w = weight[i], d = widen4(gr[i]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double gk = (double)d[k] * (double)w[k];
            const float xh = ln_xhat(v[k], st);
            s1 += gk;
            s2 += gk * (double)xh;
        }
    }
    const double m1 = wave_sum(s1) * inv_c, m2 = wave_sum(s2) * inv_c;
    for (int i = lane; i < c4; i += 64) {
        const f32x4 v = xr[i], w = weight[i], d = widen4(gr[i]);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float xh = ln_xhat(v[k], st);
            o[k] = (float)((double)st.rstd * ((double)d[k] * (double)w[k] - m1 - (double)xh * m2));
        }
        dr[i] = o;
    }
    if (lane == 0) {
        stats[2 * row] = st.mean;
        stats[2 * row + 1] = (double)st.rstd;
    }
}

// partial[chunk][2][C] (f64): a chunk of kLnChunk rows, one thread per channel, rows in order.  DY: float or __bf16.
template <class DY>
__global__ __launch_bounds__(kBlock) void layernorm_bwd_partial_kernel(long long rows, int C, const float *__restrict__ x,
                                                                       const DY *__restrict__ dy, const double *__restrict__ stats,
                                                                       double *partial) {
    const int c = blockIdx.y * kBlock + threadIdx.x;
    if (c >= C) return;
    const long long r0 = (long long)blockIdx.x * kLnChunk, r1 = r0 + kLnChunk < rows ? r0 + kLnChunk : rows;
    double sw = 0.0, sb = 0.0;
    for (long long r = r0; r < r1; ++r) {
        const float xh = ln_xhat(x[r * C + c], LnStats{stats[2 * r], (float)stats[2 * r + 1]});
        const double d = (double)(float)dy[r * C + c];
        sw += d * (double)xh;
        sb += d;
    }
    partial[((long long)blockIdx.x * 2) * C + c] = sw;
    partial[((long long)blockIdx.x * 2 + 1) * C + c] = sb;
}

__global__ __launch_bounds__(kBlock) void layernorm_bwd_finish_kernel(int chunks, int C, const double *__restrict__ partial, float *dweight,
                                                                      float *dbias) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    double sw = 0.0, sb = 0.0;
    for (int k = 0; k < chunks; ++k) {
        sw += partial[((long long)k * 2) * C + c];
        sb += partial[((long long)k * 2 + 1) * C + c];
    }
    dweight[c] = (float)sw;
    dbias[c] = (float)sb;
}

// ------------------------------------------------------------------------------------------------
// GELU backward: dx = dy (Phi(x) + x phi(x)); Phi from the forward's erf term (gelu_erf_term)
// ------------------------------------------------------------------------------------------------
__device__ inline float gelu_grad1(float x, float dy) {
    const float cdf = 0.5f * gelu_erf_term(x);
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    return dy * fmaf(x, pdf, cdf);
}

__global__ __launch_bounds__(kBlock) void gelu_bwd_kernel(long long n4, int tail, const float *x, const float *dy, float *dx) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n4) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i], d = reinterpret_cast<const f32x4 *>(dy)[i];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = gelu_grad1(v[k], d[k]);
        reinterpret_cast<f32x4 *>(dx)[i] = o;
    }
    if (i < tail) dx[4 * n4 + i] = gelu_grad1(x[4 * n4 + i], dy[4 * n4 + i]);
}

// bf16 tensors: gelu_grad1 on the widened values, rounded once (RNE).  Every thread reads its values before it writes: in place is fine.
__global__ __launch_bounds__(kBlock) void gelu_bwd_bf16_kernel(long long n8, int tail, const __bf16 *x, const __bf16 *dy, __bf16 *dx) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < n8) {
        const bf16x8 v = reinterpret_cast<const bf16x8 *>(x)[i], d = reinterpret_cast<const bf16x8 *>(dy)[i];
        bf16x8 o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (__bf16)gelu_grad1((float)v[k], (float)d[k]);
        reinterpret_cast<bf16x8 *>(dx)[i] = o;
    }
    if (i < tail) dx[8 * n8 + i] = (__bf16)gelu_grad1((float)x[8 * n8 + i], (float)dy[8 * n8 + i]);
}

// ------------------------------------------------------------------------------------------------
// crop + bilinear resize backward, gather form
// ------------------------------------------------------------------------------------------------
// the weight with which output position o reads input position i along one axis (0 for most o), as resize_bilinear_kernel forms it
__device__ inline double resize_tap(int o, int i, int in, int out) {
    const double s = fmax(((double)o + 0.5) * ((double)in / (double)out) - 0.5, 0.0);
    const int i0 = min((int)s, in - 1);
    const int i1 = i0 + (i0 < in - 1 ? 1 : 0);
    const double l = s - (double)i0;
    return (i0 == i ? 1.0 - l : 0.0) + (i1 == i ? l : 0.0);
}

// the outputs that can read input position i: source position within (i - 1, i + 1), two positions of slack either side
__device__ inline void resize_range(int i, int in, int out, int &lo, int &hi) {
    const double r = (double)out / (double)in;
    lo = max((int)floor(((double)i - 0.5) * r - 0.5) - 2, 0);
    hi = min((int)ceil(((double)i + 1.5) * r - 0.5) + 2, out - 1);
}

__global__ __launch_bounds__(kBlock) void resize_bilinear_bwd_kernel(int B, int h, int w, int c4, int ch, int cw, int oh, int ow,
                                                                     const f32x4 *__restrict__ dy, f32x4 *dx) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long long)B * h * w * c4) return;
    const int c = (int)(i % c4);
    const int ix = (int)((i / c4) % w);
    const int iy = (int)((i / ((long long)c4 * w)) % h);
    const long long b = i / ((long long)c4 * w * h);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (iy < ch && ix < cw) {
        int ylo, yhi, xlo, xhi;
        resize_range(iy, ch, oh, ylo, yhi);
        resize_range(ix, cw, ow, xlo, xhi);
        for (int oy = ylo; oy <= yhi; ++oy) {
            const double wy = resize_tap(oy, iy, ch, oh);
            if (wy == 0.0) continue;
            double rowacc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int ox = xlo; ox <= xhi; ++ox) {
                const double wx = resize_tap(ox, ix, cw, ow);
                if (wx == 0.0) continue;
                const f32x4 d = dy[((b * oh + oy) * ow + ox) * c4 + c];
#pragma unroll
                for (int k = 0; k < 4; ++k) rowacc[k] += wx * (double)d[k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += wy * rowacc[k];
        }
    }
    dx[i] = f32x4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
}

}  // namespace

extern "C" int sgv3d_vit_attention_lse(const sgv3d_vit_attn_desc *desc, const float *qkv, const float *pad_qkv, const float *rel_pos_h,
                                       const float *rel_pos_w, float *out, float *lse, void *stream) {
    SGV3D_REQUIRE(lse, "vit_attention_lse: null lse");
    SGV3D_REQUIRE(aligned16(lse), "vit_attention_lse: lse must be 16-byte aligned");
    return vit_attention_impl(desc, qkv, pad_qkv, rel_pos_h, rel_pos_w, out, lse, stream);
}

extern "C" size_t sgv3d_vit_attention_backward_workspace_bytes(const sgv3d_vit_attn_desc *desc) {
    if (check_attn_desc("vit_attention_backward_workspace_bytes", desc, 0) != SGV3D_OK) return 0;
    return sizeof(float) * (size_t)bwd_layout(*desc, true).total;     // with tables: an upper bound for the call without
}

extern "C" int sgv3d_vit_attention_backward(const sgv3d_vit_attn_desc *desc, const float *qkv, const float *pad_qkv,
                                            const float *rel_pos_h, const float *rel_pos_w, const float *out, const float *lse,
                                            const float *dout, float *dqkv, float *dpad_qkv, float *drel_pos_h, float *drel_pos_w,
                                            void *workspace, size_t workspace_bytes, void *stream) {
    const int rc = check_attn_desc("vit_attention_backward", desc, 0);
    if (rc != SGV3D_OK) return rc;
    const sgv3d_vit_attn_desc &d = *desc;
    SGV3D_REQUIRE((rel_pos_h == nullptr) == (rel_pos_w == nullptr),
                  "vit_attention_backward: rel_pos_h and rel_pos_w must be given together or not at all");
    const bool rel = rel_pos_h != nullptr;
    SGV3D_REQUIRE(qkv && out && lse && dout && dqkv, "vit_attention_backward: null qkv, out, lse, dout or dqkv");
    SGV3D_REQUIRE(!pad_qkv || dpad_qkv, "vit_attention_backward: pad_qkv is given, dpad_qkv is null");
    SGV3D_REQUIRE(rel ? (drel_pos_h && drel_pos_w) : (!drel_pos_h && !drel_pos_w),
                  "vit_attention_backward: drel_pos_h and drel_pos_w must be given exactly when the tables are");
    SGV3D_REQUIRE(aligned16(qkv) && aligned16(pad_qkv) && aligned16(rel_pos_h) && aligned16(rel_pos_w) && aligned16(out) &&
                      aligned16(lse) && aligned16(dout) && aligned16(dqkv) && aligned16(dpad_qkv) && aligned16(drel_pos_h) &&
                      aligned16(drel_pos_w) && aligned16(workspace),
                  "vit_attention_backward: every pointer must be 16-byte aligned");
    const BwdLayout L = bwd_layout(d, rel);
    SGV3D_REQUIRE(L.G * L.Tp < (1LL << 31) && L.G * (2LL * d.win_h + 2LL * d.win_w) < (1LL << 31),
                  "vit_attention_backward: too many workgroups");
    const int ah_ld = odd_ld(rel, d.win_h), aw_ld = odd_ld(rel, d.win_w);
    const size_t tile_floats = d.head_dim == 32 ? BwdGeom<32>::floats : d.head_dim == 64 ? BwdGeom<64>::floats : BwdGeom<80>::floats;
    const size_t lds_keys = sizeof(float) * tile_floats, lds_q = lds_keys + sizeof(float) * (size_t)kTile * (ah_ld + aw_ld);
    // lds_q is at most 2 * 64 * 88 + 64 * (129 + 129) floats = 111 104 bytes of the 160 KB: the window is at most 128 x 128
    if (!workspace || workspace_bytes < sizeof(float) * (size_t)L.total)
        return fail(SGV3D_ENOSPACE, "vit_attention_backward: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0,
                    sizeof(float) * (size_t)L.total);

    BwdParams p;
    fill_window(p, d);
    p.HD = d.head_dim, p.Tp = (int)L.Tp, p.nt = (int)L.nt, p.ah_ld = ah_ld, p.aw_ld = aw_ld;
    p.scale = softmax_scale(d.head_dim);
    p.qkv = qkv, p.pad = pad_qkv, p.rh = rel_pos_h, p.rw = rel_pos_w, p.out = out, p.lse = lse, p.dout = dout;
    p.dqkv = dqkv, p.dpad = dpad_qkv, p.drh = drel_pos_h, p.drw = drel_pos_w;
    float *ws = static_cast<float *>(workspace);
    p.lse_w = ws + L.lse_w, p.delta_w = ws + L.delta_w, p.th = ws + L.th, p.tw = ws + L.tw, p.thT = ws + L.thT, p.twT = ws + L.twT;
    p.ah = ws + L.ah, p.aw = ws + L.aw, p.padpart = ws + L.padpart, p.relh = ws + L.relh, p.relw = ws + L.relw;
    p.G = L.G;
    hipStream_t s = as_stream(stream);

    hipLaunchKernelGGL(attn_bwd_prep_kernel, dim3((unsigned)(L.G * L.Tp)), dim3(64), 0, s, p);
    int r = check_launch("attn_bwd_prep_kernel");
    if (r != SGV3D_OK) return r;
    r = launch_bwd_hd<true>(p, L.G * L.nt, lds_keys, s);
    if (r != SGV3D_OK) return r;
    r = launch_bwd_hd<false>(p, L.G * L.nt, lds_q, s);
    if (r != SGV3D_OK) return r;
    if (rel) {
        hipLaunchKernelGGL(attn_bwd_table_kernel, dim3((unsigned)(L.G * (2LL * d.win_h + 2LL * d.win_w - 2))), dim3(32, kTabSlices), 0, s, p);
        r = check_launch("attn_bwd_table_kernel");
        if (r != SGV3D_OK) return r;
    }
    const long long n_fin = (dpad_qkv ? 3LL * d.heads * d.head_dim / 4 : 0) + (rel ? (2LL * d.win_h + 2LL * d.win_w - 2) * (d.head_dim / 4) : 0);
    if (n_fin > 0) {
        hipLaunchKernelGGL(attn_bwd_finish_kernel, dim3((unsigned)cdiv(n_fin, kBlock)), dim3(kBlock), 0, s, p);
        r = check_launch("attn_bwd_finish_kernel");
    }
    return r;
}

extern "C" size_t sgv3d_layernorm_backward_workspace_bytes(long long rows, int channels) {
    if (rows <= 0 || channels <= 0) return 0;
    const long long chunks = (rows + kLnChunk - 1) / kLnChunk;
    return sizeof(double) * (size_t)(2 * rows + 2 * chunks * channels);
}

// sgv3d_layernorm_backward (DY = float) and sgv3d_layernorm_backward_bf16dy (DY = __bf16): one set of checks, the same three launches
template <class DY, class DY4>
static int layernorm_backward_impl(const char *who, long long rows, int channels, const float *x, const float *weight, float eps,
                                   const DY *dy, float *dx, float *dweight, float *dbias, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    SGV3D_REQUIRE(rows > 0 && channels > 0, "%s: non-positive size (rows %lld, channels %d)", who, rows, channels);
    SGV3D_REQUIRE(channels % 4 == 0, "%s: channels %d is not a multiple of 4", who, channels);
    SGV3D_REQUIRE(x && weight && dy && dx && dweight && dbias, "%s: null pointer", who);
    SGV3D_REQUIRE(eps >= 0.f, "%s: negative eps", who);
    SGV3D_REQUIRE(aligned16(x) && aligned16(weight) && aligned16(dy) && aligned16(dx) && aligned16(dweight) && aligned16(dbias) &&
                      aligned16(workspace),
                  "%s: pointers must be 16-byte aligned", who);
    // the weight / bias partials read x and dy after dx has been written
    const unsigned long long span = 4ULL * (unsigned long long)rows * (unsigned long long)channels;
    // (dy spans sizeof(DY) bytes per value: for the f32 dy the same test as for x)
    const unsigned long long dy_span = sizeof(DY) * (unsigned long long)rows * (unsigned long long)channels;
    const uintptr_t pdx = reinterpret_cast<uintptr_t>(dx), pdy = reinterpret_cast<uintptr_t>(dy);
    SGV3D_REQUIRE(!overlaps(dx, x, span) && !(pdx < pdy + dy_span && pdy < pdx + span), "%s: dx must not overlap x or dy", who);
    const long long blocks = (rows + kBlock / 64 - 1) / (kBlock / 64);
    const long long chunks = (rows + kLnChunk - 1) / kLnChunk;
    SGV3D_REQUIRE(blocks < (1LL << 31), "%s: too many rows", who);
    const size_t need = sgv3d_layernorm_backward_workspace_bytes(rows, channels);
    if (!workspace || workspace_bytes < need)
        return fail(SGV3D_ENOSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace ? workspace_bytes : (size_t)0, need);
    double *stats = static_cast<double *>(workspace), *partial = stats + 2 * rows;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(layernorm_bwd_dx_kernel<DY4>, dim3((unsigned)blocks), dim3(kBlock), 0, s, rows, channels / 4,
                       reinterpret_cast<const f32x4 *>(x), reinterpret_cast<const f32x4 *>(weight), eps,
                       reinterpret_cast<const DY4 *>(dy), reinterpret_cast<f32x4 *>(dx), stats);
    int r = check_launch("layernorm_bwd_dx_kernel");
    if (r != SGV3D_OK) return r;
    hipLaunchKernelGGL(layernorm_bwd_partial_kernel<DY>, dim3((unsigned)chunks, (unsigned)cdiv(channels, kBlock)), dim3(kBlock), 0, s, rows,
                       channels, x, dy, stats, partial);
    r = check_launch("layernorm_bwd_partial_kernel");
    if (r != SGV3D_OK) return r;
    hipLaunchKernelGGL(layernorm_bwd_finish_kernel, dim3((unsigned)cdiv(channels, kBlock)), dim3(kBlock), 0, s, (int)chunks, channels,
                       partial, dweight, dbias);
    return check_launch("layernorm_bwd_finish_kernel");
}

extern "C" int sgv3d_layernorm_backward(long long rows, int channels, const float *x, const float *weight, float eps, const float *dy,
                                        float *dx, float *dweight, float *dbias, void *workspace, size_t workspace_bytes, void *stream) {
    return layernorm_backward_impl<float, f32x4>("layernorm_backward", rows, channels, x, weight, eps, dy, dx, dweight, dbias, workspace,
                                                 workspace_bytes, stream);
}

extern "C" int sgv3d_layernorm_backward_bf16dy(long long rows, int channels, const float *x, const float *weight, float eps, const void *dy,
                                               float *dx, float *dweight, float *dbias, void *workspace, size_t workspace_bytes,
                                               void *stream) {
    return layernorm_backward_impl<__bf16, bf16x4>("layernorm_backward_bf16dy", rows, channels, x, weight, eps,
                                                   static_cast<const __bf16 *>(dy), dx, dweight, dbias, workspace, workspace_bytes, stream);
}

extern "C" int sgv3d_gelu_backward(long long n, const float *x, const float *dy, float *dx, void *stream) {
    SGV3D_REQUIRE(n > 0, "gelu_backward: non-positive count %lld", n);
    SGV3D_REQUIRE(x && dy && dx, "gelu_backward: null pointer");
    SGV3D_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dx), "gelu_backward: pointers must be 16-byte aligned");
    const long long n4 = n / 4;
    const long long blocks = (n4 + kBlock) / kBlock;
    SGV3D_REQUIRE(blocks < (1LL << 31), "gelu_backward: too many values");
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), n4, (int)(n - 4 * n4), x, dy, dx);
    return check_launch("gelu_bwd_kernel");
}

extern "C" int sgv3d_gelu_backward_bf16(long long n, const void *x, const void *dy, void *dx, void *stream) {
    SGV3D_REQUIRE(n > 0, "gelu_backward_bf16: non-positive count %lld", n);
    SGV3D_REQUIRE(x && dy && dx, "gelu_backward_bf16: null pointer");
    SGV3D_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(dx), "gelu_backward_bf16: pointers must be 16-byte aligned");
    // in place (dx the same tensor as x or dy) is allowed; a shifted overlap is not: a thread would read what another has written
    const unsigned long long span = 2ULL * (unsigned long long)n;
    SGV3D_REQUIRE((dx == x || !overlaps(dx, x, span)) && (dx == dy || !overlaps(dx, dy, span)),
                  "gelu_backward_bf16: dx must be x, dy or a tensor that overlaps neither");
    const long long n8 = n / 8;
    const long long blocks = (n8 + kBlock) / kBlock;    // at least one: its first threads take the tail
    SGV3D_REQUIRE(blocks < (1LL << 31), "gelu_backward_bf16: too many values");
    hipLaunchKernelGGL(gelu_bwd_bf16_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), n8, (int)(n - 8 * n8),
                       static_cast<const __bf16 *>(x), static_cast<const __bf16 *>(dy), static_cast<__bf16 *>(dx));
    return check_launch("gelu_bwd_bf16_kernel");
}

extern "C" int sgv3d_resize_bilinear_backward(int batch, int h, int w, int channels, int crop_h, int crop_w, int out_h, int out_w,
                                              const float *dy, float *dx, void *stream) {
    SGV3D_REQUIRE(batch > 0 && h > 0 && w > 0 && channels > 0 && crop_h > 0 && crop_w > 0 && out_h > 0 && out_w > 0,
                  "resize_bilinear_backward: non-positive size");
    SGV3D_REQUIRE(channels % 4 == 0, "resize_bilinear_backward: channels %d is not a multiple of 4", channels);
    SGV3D_REQUIRE(dy && dx, "resize_bilinear_backward: null pointer");
    SGV3D_REQUIRE(aligned16(dy) && aligned16(dx), "resize_bilinear_backward: pointers must be 16-byte aligned");
    const int ch = crop_h < h ? crop_h : h, cw = crop_w < w ? crop_w : w;
    const long long blocks = ((long long)batch * h * w * (channels / 4) + kBlock - 1) / kBlock;
    SGV3D_REQUIRE(blocks < (1LL << 31), "resize_bilinear_backward: too many pixels");
    hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), batch, h, w, channels / 4,
                       ch, cw, out_h, out_w, reinterpret_cast<const f32x4 *>(dy), reinterpret_cast<f32x4 *>(dx));
    return check_launch("resize_bilinear_bwd_kernel");
}
