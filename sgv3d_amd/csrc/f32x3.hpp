// "f32x3": float32-accurate products on the bf16 matrix cores.  What the kernels of the family (gemm_x3_grouped.hip,
// conv_pw_x3.hip, stem_pool_x3.hip and the F(4x4) producers of conv_wino4.hip) must agree on bit for bit, each defined once: the
// split of an f32 number into three bf16 terms, the order of the six partial products, the fragment-ordered weight pack, the LDS
// image of a row tile and the k-loop around them.  Device code, gfx950 only.  (The SPLIT3 form of conv_igemm_bf16_kernel does the
// same arithmetic on the 32x32x16 instruction with macros of its own.)
//
// Arithmetic.  Every f32 operand x is split EXACTLY into three bf16 terms, hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi -
// mid) (the remainders are exact in f32: 3 x 8 significand bits = f32's 24).  A product x * w is the f32 sum of the six partial
// products of weight >= 2^-16, accumulated in f32 by the MFMA; the three dropped ones are below 2^-24 of the product: one f32
// rounding, as v_mfma_f32_16x16x4_f32 would commit.  Six v_mfma_f32_16x16x32_bf16 (16 cycles each, K = 32) do the work of eight
// v_mfma_f32_16x16x4_f32 (32 cycles each): 96 cycles against 256.
#pragma once
#include "common.hpp"

namespace sgv3d {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// the split
// ------------------------------------------------------------------------------------------------
// v = hi + mid + lo exactly (8 + 8 + 8 significand bits; the remainders v - hi and v - hi - mid are exact in f32)
__device__ __forceinline__ void split3(const f32x4 v, bf16x4 &hi, bf16x4 &mid, bf16x4 &lo) {
    hi = __builtin_convertvector(v, bf16x4);
    const f32x4 r1 = v - __builtin_convertvector(hi, f32x4);
    mid = __builtin_convertvector(r1, bf16x4);
    const f32x4 r2 = r1 - __builtin_convertvector(mid, f32x4);
    lo = __builtin_convertvector(r2, bf16x4);
}

// The three bf16 terms of the f32 number v, contraction off: where v is a product, v - hi would otherwise fuse with the
// multiplication into one multiply-add and mid would carry the product's UNROUNDED tail (576 * (1 / 6) came out as
// 96 + 2.9e-6) -- the f32x3 weights are to be the terms of the rounded f32 weight, integer where that is.
__device__ __forceinline__ void split3_rounded(float v, __bf16 &hi, __bf16 &mid, __bf16 &lo) {
#pragma clang fp contract(off)
    hi = (__bf16)v;
    const float r1 = v - (float)hi;
    mid = (__bf16)r1;
    lo = (__bf16)(r1 - (float)mid);
}

// ------------------------------------------------------------------------------------------------
// the product: w and x are the [hi, mid, lo] fragments of one k-step (v_mfma_f32_16x16x32_bf16, w on the A side)
// ------------------------------------------------------------------------------------------------
// Term t of the six, small terms first -- (w lo, x hi), (w hi, x lo), (mid, mid), (w mid, x hi), (w hi, x mid), (hi, hi) -- so
// that the leading product meets an accumulator that already holds the corrections.  A kernel with several independent
// accumulators may interleave their terms; every accumulator takes its own in this order.
__device__ __forceinline__ void x3_term(int t, const bf16x8 *w, const bf16x8 *x, f32x4 &acc) {
    constexpr int wp[6] = {2, 0, 1, 1, 0, 0}, xp[6] = {0, 2, 1, 0, 1, 0};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[wp[t]], x[xp[t]], acc, 0, 0, 0);
}

__device__ __forceinline__ void x3_product(const bf16x8 *w, const bf16x8 *x, f32x4 &acc) {
#pragma unroll
    for (int t = 0; t < 6; ++t) x3_term(t, w, x, acc);
}

// ------------------------------------------------------------------------------------------------
// U3, the weight pack: [cout_pad / 16][K / 32][3][512] bf16 in FRAGMENT order
// ------------------------------------------------------------------------------------------------
// Block of 16 output channels x k-step x plane = 512 elements = 1024 contiguous bytes, element (channel c, k) at
// ((k / 8) * 16 + c) * 8 + k % 8: the 64 lanes of a wave load one MFMA operand with one buffer_load_dwordx4 each, contiguously,
// lane l at 16 l.  The three planes [hi | mid | lo] of a k-step follow one another: 3072 bytes per k-step of a block.
constexpr int kU3PlaneElems = 512, kU3PlaneBytes = 2 * kU3PlaneElems, kU3StepBytes = 3 * kU3PlaneBytes;

// the packers: where the hi term of (output channel co, k) goes in the pack u of K (a multiple of 32) k per channel; mid and lo
// kU3PlaneElems further each
template <class I>
__device__ __forceinline__ __bf16 *u3_at(__bf16 *u, int co, int k, I K) {
    return u + (((size_t)(co >> 4) * (K >> 5) + (k >> 5)) * 3) * kU3PlaneElems + ((((k & 31) >> 3) * 16 + (co & 15)) * 8 + (k & 7));
}

__device__ __forceinline__ void u3_store(__bf16 *q, __bf16 hi, __bf16 mid, __bf16 lo) {
    q[0] = hi;
    q[kU3PlaneElems] = mid;
    q[2 * kU3PlaneElems] = lo;
}

// the kernels: this lane's byte offset into channel block cb (k-step 0, plane hi)
__device__ __forceinline__ unsigned u3_lane_offset(int cb, int ksteps, int lane) {
    return (unsigned)(((long long)cb * ksteps) * kU3StepBytes + lane * 16);
}

// ... or an offset past every buffer (the load then returns zeros) for a block in the padding beyond cout_pad
__device__ __forceinline__ unsigned u3_lane_offset(int cb, int ksteps, int lane, int cout_pad) {
    return cb * 16 < cout_pad ? u3_lane_offset(cb, ksteps, lane) : 0xffffffffu;
}

// one fragment: plane s of k-step kt
__device__ __forceinline__ bf16x8 u3_load(__amdgpu_buffer_rsrc_t w_rsrc, unsigned lane_offset, int kt, int s) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, lane_offset, kt * kU3StepBytes + s * kU3PlaneBytes, 0));
}

// a wave's six fragments of k-step kt: two channel blocks (lane offsets wgo) x three planes
__device__ __forceinline__ void u3_load_step(__amdgpu_buffer_rsrc_t w_rsrc, const unsigned (&wgo)[2], int kt, bf16x8 (&fw)[2][3]) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int s = 0; s < 3; ++s) fw[nb][s] = u3_load(w_rsrc, wgo[nb], kt, s);
}

// ------------------------------------------------------------------------------------------------
// the row tile in LDS: two buffers of three planes [hi | mid | lo] of BM rows x 32 k
// ------------------------------------------------------------------------------------------------
// Rows of 64 bytes, the 16-byte chunk c of row r stored at c ^ (-(r >> 2) & 3): the four 16-lane groups of a ds_read_b128 (rows
// {0-3, 12-15} at one chunk with rows {4-11} at the next, and so on) each fall on 64 distinct banks; a plane is BM x 64 + 64 bytes
// so that the 8-lane groups of a staging store that straddle two planes or two rows use both halves of the banks.
constexpr int x3_plane_bytes(int bm) { return bm * 64 + 64; }
constexpr int x3_buf_bytes(int bm) { return 3 * x3_plane_bytes(bm); }

// the chunk swizzle key of row r
__device__ __forceinline__ int x3_swizzle(int row) { return (-(row >> 2)) & 3; }

// Lane (l16, g) of a row fragment reads row l16 of a 16-row block, k range [8 g, 8 g + 8): + 16 ma rows, + plane, + buffer.  (A
// macro: as a function of (l16, g) it compiles to the same value with the operands of one instruction exchanged.)
#define X3_FRAG_OFFSET(L16, G) ((unsigned)((L16) * 64) + (unsigned)(((G) ^ sgv3d::x3_swizzle(L16)) << 4))

// ------------------------------------------------------------------------------------------------
// the k-loop: acc[ma][nb] += rows x weights over nkt k-steps, for a wave that owns 16 MA rows x 32 columns (nb = 2 blocks of 16)
// ------------------------------------------------------------------------------------------------
// weights  never touch LDS: a wave's 6 fragments of a k-step (2 column blocks x 3 planes) come from L2 straight into registers,
//          requested one k-step ahead (weight k-step wkt0 + kt for the loop's k-step kt).
// rows     through LDS.  The rows of k-step kt + 1 are in registers while k-step kt computes and are stored into the OTHER buffer
//          behind the MFMAs of row block MA - 2; the rows of k-step kt + 2 are requested right behind that store: ONE barrier per
//          k-step.  sched_barriers keep the request / MFMA / store order.
// The row source is the including kernel's: two statement macros passed in by name, which work on registers of their own,
//   REQUEST(kt)   request the rows of k-step kt (called with kt = 0, 1, 2, ... in turn)
//   STORE(b)      store the held rows, split into the three planes, into LDS buffer b (0 or 1)
// (A macro, not a template over a row-source functor: the functor form compiled to other register assignments and another
// instruction order in every instantiation, and these kernels are held to their measured code.)
// MA: 16-row blocks of the tile; SMEM: the two buffers; WGO[2]: u3_lane_offset of the wave's two channel blocks; X_FRAG:
// X3_FRAG_OFFSET of the lane; FW[2][2][3]: bf16x8 registers for the weights, [stage][nb][plane]; ACC[MA][2].
#define X3_KSTEP_(MA, SMEM, W_RSRC, WGO, WKT0, NKT, X_FRAG, FW, ACC, REQUEST, STORE, KT, B, ST)                       \
    do {                                                                                                              \
        constexpr int plane_ = sgv3d::x3_plane_bytes(16 * (MA)), buf_ = sgv3d::x3_buf_bytes(16 * (MA));               \
        if ((KT) + 1 < (NKT)) sgv3d::u3_load_step(W_RSRC, WGO, (WKT0) + ((KT) + 1), (FW)[(ST) ^ 1]);                  \
        sgv3d::bf16x8 fx_[2][3];                                                                                      \
        _Pragma("unroll") for (int s = 0; s < 3; ++s)                                                                 \
            fx_[0][s] = *reinterpret_cast<const sgv3d::bf16x8 *>((SMEM) + (B) * buf_ + (X_FRAG) + s * plane_);        \
        _Pragma("unroll") for (int ma = 0; ma < (MA); ++ma) {                                                         \
            if (ma + 1 < (MA)) {                                                                                      \
                _Pragma("unroll") for (int s = 0; s < 3; ++s)                                                         \
                    fx_[(ma + 1) & 1][s] =                                                                            \
                        *reinterpret_cast<const sgv3d::bf16x8 *>((SMEM) + (B) * buf_ + (X_FRAG) + (ma + 1) * 16 * 64 + s * plane_); \
            }                                                                                                         \
            if (ma == ((MA) > 2 ? (MA) - 2 : (MA) - 1) && (KT) + 1 < (NKT)) {                                         \
                STORE((B) ^ 1);                                                                                       \
                if ((KT) + 2 < (NKT)) REQUEST((KT) + 2);                                                              \
            }                                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
            _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) sgv3d::x3_product((FW)[ST][nb], fx_[ma & 1], (ACC)[ma][nb]); \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
        }                                                                                                             \
        if ((KT) + 1 < (NKT)) __syncthreads();                                                                        \
    } while (0)

#define X3_KLOOP(MA, SMEM, W_RSRC, WGO, WKT0, NKT, X_FRAG, FW, ACC, REQUEST, STORE)                                   \
    do {                                                                                                              \
        REQUEST(0);                                                                                                   \
        sgv3d::u3_load_step(W_RSRC, WGO, WKT0, (FW)[0]);                                                              \
        STORE(0);                                                                                                     \
        if ((NKT) > 1) REQUEST(1);                                                                                    \
        __syncthreads();                                                                                              \
        int kt_ = 0;                                                                                                  \
        for (; kt_ + 1 < (NKT); kt_ += 2) {                                                                           \
            X3_KSTEP_(MA, SMEM, W_RSRC, WGO, WKT0, NKT, X_FRAG, FW, ACC, REQUEST, STORE, kt_, 0, 0);                  \
            X3_KSTEP_(MA, SMEM, W_RSRC, WGO, WKT0, NKT, X_FRAG, FW, ACC, REQUEST, STORE, kt_ + 1, 1, 1);              \
        }                                                                                                             \
        if (kt_ < (NKT)) X3_KSTEP_(MA, SMEM, W_RSRC, WGO, WKT0, NKT, X_FRAG, FW, ACC, REQUEST, STORE, kt_, 0, 0);     \
    } while (0)

}  // namespace sgv3d
