// The image stem in one launch: NCHW image -> 7x7 / stride 2 / pad 3 convolution (3 -> 64) + folded BN + ReLU -> 3x3 / stride 2 / pad 1
// max-pool -> NHWC map (mmdet ResNet's conv1 / bn1 / relu / maxpool, built at layers/backbones/lss_fpn.py:296-297), with
// float32-accurate products on the bf16 matrix cores ("f32x3", f32x3.hpp).  It replaces three launches -- nchw_to_nhwc_kernel
// (c_pad 4), the tap-major stem convolution and maxpool3x3s2_kernel -- and the two maps between them (the 4-channel NHWC copy of
// the image and the un-pooled 64-channel map, written and read once each) never reach memory.
//
//   y[b][ph][pw][co] = max over the 3x3 window of conv pixels (2 ph - 1 + dy, 2 pw - 1 + dx) inside the conv map of
//                      max(fmaf(sum_k x3(pixel, k) * w3(co, k), scale[co], shift[co]), 0)
//
// Arithmetic: bit for bit conv_pw_x3_kernel<.., 2> (sgv3d_conv2d_x3_forward on the 4-channel copy, no split-K) followed by
// maxpool3x3s2_kernel.  The weights are that launch's pack, unchanged (sgv3d_conv_pack_weight_x3, k order 0: k = tap * 4 + ci, K = 196
// padded to 224 = 7 k-steps of 8 taps x 4 channels, fragment order).  A pixel fragment holds for lane (l16, g) of k-step kt the k range
// [32 kt + 8 g, 32 kt + 8 g + 8) = taps 8 kt + 2 g and 8 kt + 2 g + 1 x 4 channels of conv pixel l16, what that kernel's LDS rows hold;
// channel 3, the taps outside the image and taps >= 49 are zeros, as its masked loads return; the split and the order of a k-step's
// six partial products are f32x3.hpp's, on a zeroed accumulator, the k-steps in order; the epilogue is the same fused multiply-add and
// fmaxf.  An MFMA's result for one (channel, pixel) element depends on that element's operands only, so which 16 pixels share an
// instruction does not matter.  max is exact; the pool uses maxpool3x3s2_kernel's NaN-propagating comparison in its window order.
//
// Kernel.  A tile is TPH x TPW = 4 x 16 pooled pixels of one image: 9 x 33 conv pixels from a 23 x 71 input patch.  One persistent
// workgroup of 4 waves per CU walks the tiles w, w + gridDim.x, ...: its weights stay in registers over all of them, and the patch of
// its next tile is requested (21 dwords per lane) before the MFMAs of the current one, so that a tile costs its MFMAs, the split of
// the patch into LDS, the pool and two barriers, not the memory round trips.
//   patch    read from the three planes with coalesced row reads, split once and kept in LDS as three bf16 planes of 4-channel pixels
//            (8 bytes per pixel and plane; 3 x 23 x 71 x 8 B = 39 KB).  Conv pixel (r, c) of the tile reads patch pixel (2 r + kh, 2 c + kw):
//            consecutive conv pixels are 16 bytes apart, a lane's two taps are two 8-byte reads (ds_read_b64: two groups of 32 lanes
//            on 64 banks; the lane groups g and g + 1 of a 32-lane group read overlapping pixels, which broadcast).
//   weights  a wave owns 32 output channels and keeps all 7 k-steps of their weights in registers (2 x 7 x 3 fragments = 168 VGPRs),
//            loaded once per workgroup from L2 in fragment order: the k-loop issues no weight load at all.  The fragments of k-step
//            kt + 1 are read from LDS before the MFMAs of k-step kt (one wave per SIMD: nothing else hides the LDS latency).
//   pixels   the 297 conv pixels of the tile are numbered row-major and cut into 19 groups of 16; waves {0, 1} take the even groups,
//            {2, 3} the odd ones, two groups at a time (four independent accumulator chains).  Per group and k-step: 6 LDS reads of 8
//            bytes per lane for 12 MFMAs.
//   pool     the conv tile goes through LDS as f32 (297 pixels x 68 floats: 64 channels + 4 of padding so that the 16 lanes of a
//            store hit distinct banks; 79 KB); a thread then pools 4 channels of one output pixel and stores 16 bytes.
// One workgroup per CU (119 KB of LDS; 256 VGPRs + 86 AGPRs, no spills).  No atomics, no split-K: the result is deterministic.
//
// Bound: MFMA bf16 with 6 x 2 x (20 x 16 pixels per tile) x 64 x 224 executed flop; HBM traffic is the image once and the pooled map once.
#include "conv_common.hpp"
#include "f32x3.hpp"

using namespace sgv3d;

namespace {

struct StemPoolArgs {
    const float *x, *scale, *shift;
    const void *w;             // the w_pw_x3 pack of the 64 x 3 x 7 x 7 weight: [4][7][3][512] bf16
    float *y;
    int H, W, Hc, Wc, Hp, Wp, y_ld;
    int tiles_h, tiles_w, ntiles;
    unsigned w_bytes, x_bytes;
};

// as maxpool3x3s2_kernel's (misc_layers.hip): propagates NaN like torch's pooling kernels
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

template <int TPH, int TPW>
__global__ __launch_bounds__(256) void stem_pool_x3_kernel(const StemPoolArgs a) {
    constexpr int CH = 2 * TPH + 1, CW = 2 * TPW + 1, NPIX = CH * CW, NG = (NPIX + 15) / 16;
    constexpr int PH = 4 * TPH + 7, PW = 4 * TPW + 7, NPATCH = PH * PW;
    constexpr int PLANE = NPATCH * 8;                          // bytes of one bf16 plane of the patch
    constexpr int PATCH_BYTES = (3 * PLANE + 15) / 16 * 16;
    constexpr int CT_LD = 68;                                  // floats per conv pixel in LDS
    constexpr int KT = 7;                                      // k-steps: 49 taps x 4 channels = 196, padded to 224
    __shared__ __attribute__((aligned(16))) unsigned char smem[PATCH_BYTES + NPIX * CT_LD * 4];
    float *ct = reinterpret_cast<float *>(smem + PATCH_BYTES);

    const int tid = threadIdx.x;
    const int per_img = a.tiles_h * a.tiles_w;
    const int wave = tid >> 6, lane = tid & 63;
    const int l16 = lane & 15, g = lane >> 4;
    const int half = wave & 1, pq = wave >> 1;                 // channels [32 half, 32 half + 32), pixel groups pq, pq + 2, ...

    // ---- weights: all k-steps of this wave's 32 channels, global -> registers, once per workgroup
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(a.w), 0, (int)a.w_bytes, 0x00020000);
    bf16x8 fw[2][KT][3];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int s = 0; s < 3; ++s)
                fw[nb][kt][s] = u3_load(w_rsrc, u3_lane_offset(2 * half, KT, lane), nb * KT + kt, s);

    // ---- patch: NCHW planes -> registers (requested one tile ahead) -> three bf16 planes of 4-channel pixels in LDS; zeros outside
    // the image (the load's offset is then out of the buffer's range and returns 0) and in channel 3
    constexpr int IT = (NPATCH + 255) / 256;
    const unsigned hw4 = (unsigned)(a.H * a.W) * 4u;
    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, (int)a.x_bytes, 0x00020000);
    float v[IT][3];
    int prow[IT], pcol[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int idx = tid + 256 * i;
        prow[i] = (int)((unsigned)idx / (unsigned)PW);
        pcol[i] = idx - prow[i] * PW;
    }
    // tile t = (image b, tile row th, tile column tw): pooled pixels from (ph0, pw0) = (TPH th, TPW tw); tile pixel (0, 0) is conv pixel
    // (2 ph0 - 1, 2 pw0 - 1), patch pixel (0, 0) is image pixel (4 ph0 - 5, 4 pw0 - 5)
#define STEM_TILE(T, B_, PH0, PW0)                                                                                 \
    const int B_ = (int)((unsigned)(T) / (unsigned)per_img);                                                       \
    const int PH0 = (int)((unsigned)((T) - B_ * per_img) / (unsigned)a.tiles_w) * TPH;                             \
    const int PW0 = ((T) - B_ * per_img - (PH0 / TPH) * a.tiles_w) * TPW;
#define STEM_LOAD_PATCH(T)                                                                                         \
    do {                                                                                                           \
        STEM_TILE(T, lb_, lph0_, lpw0_)                                                                            \
        const unsigned img_ = (unsigned)lb_ * 3u * hw4;                                                            \
        _Pragma("unroll") for (int i = 0; i < IT; ++i) {                                                           \
            const int ih = 4 * lph0_ - 5 + prow[i], iw = 4 * lpw0_ - 5 + pcol[i];                                  \
            const bool in = tid + 256 * i < NPATCH && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W; \
            const unsigned off = img_ + (unsigned)(ih * a.W + iw) * 4u;                                            \
            _Pragma("unroll") for (int c = 0; c < 3; ++c)                                                          \
                v[i][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(x_rsrc, in ? off + c * hw4 : 0xffffffffu, 0, 0)); \
        }                                                                                                          \
    } while (0)

    // this lane's two taps of every k-step as byte offsets into the patch; k-step 6 holds tap 48 (g == 0, first half) and zeros
    unsigned toff[KT][2];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int t = 8 * kt + 2 * g + j;
            const int tt = t < 49 ? t : 0;
            const int kh = tt / 7, kw = tt - kh * 7;
            toff[kt][j] = (unsigned)((kh * PW + kw) * 8);
        }
    const bool tap48 = g == 0;

    f32x4 sc[2], sh[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int col = 32 * half + 16 * nb + 4 * g;
        sc[nb] = a.scale ? *reinterpret_cast<const f32x4 *>(a.scale + col) : f32x4{1.f, 1.f, 1.f, 1.f};
        sh[nb] = a.shift ? *reinterpret_cast<const f32x4 *>(a.shift + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // persistent: workgroup w takes tiles w, w + gridDim.x, ...
    int tile = blockIdx.x;
    if (tile < a.ntiles) STEM_LOAD_PATCH(tile);
    for (; tile < a.ntiles; tile += gridDim.x) {
        STEM_TILE(tile, b, ph0, pw0)
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int idx = tid + 256 * i;
            if (idx >= NPATCH) continue;
            const f32x4 x4 = {v[i][0], v[i][1], v[i][2], 0.f};
            bf16x4 hi, mid, lo;
            split3(x4, hi, mid, lo);
            unsigned char *d = smem + idx * 8;
            *reinterpret_cast<bf16x4 *>(d) = hi;
            *reinterpret_cast<bf16x4 *>(d + PLANE) = mid;
            *reinterpret_cast<bf16x4 *>(d + 2 * PLANE) = lo;
        }
        // (also: every thread has finished pooling the previous tile, whose conv tile this one overwrites)
        __syncthreads();
        // the next tile's patch travels while this one is computed
        if (tile + (int)gridDim.x < a.ntiles) STEM_LOAD_PATCH(tile + (int)gridDim.x);

        // ---- conv: two pixel groups at a time, accumulators [group][channel block]
        for (int g0 = pq; g0 < NG; g0 += 4) {
            int p[2];
            unsigned base[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                p[u] = 16 * (g0 + 2 * u) + l16;
                const int pp = p[u] < NPIX ? p[u] : NPIX - 1;  // (the lanes past the tile read its last pixel and store nothing)
                const int r = (int)((unsigned)pp / (unsigned)CW), c = pp - r * CW;
                base[u] = (unsigned)((2 * r * PW + 2 * c) * 8);
            }
            f32x4 acc[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) acc[u][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
            // the fragments of k-step kt + 1 are requested before the MFMAs of k-step kt (one wave per SIMD: nothing else hides the
            // LDS latency); the scheduling barriers keep that order
            bf16x8 fx[2][2][3];
#define STEM_LOAD_FX(K, D)                                                                                         \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) _Pragma("unroll") for (int s = 0; s < 3; ++s) {                  \
        bf16x4 t0 = *reinterpret_cast<const bf16x4 *>(smem + s * PLANE + base[u] + toff[K][0]);                    \
        bf16x4 t1 = *reinterpret_cast<const bf16x4 *>(smem + s * PLANE + base[u] + toff[K][1]);                    \
        if ((K) == KT - 1) {                                   /* the zero padding of K: taps 49 .. 55 */          \
            t0 = tap48 ? t0 : bf16x4{};                                                                            \
            t1 = bf16x4{};                                                                                         \
        }                                                                                                          \
        fx[D][u][s] = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);                                     \
    }
            STEM_LOAD_FX(0, 0)
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                if (kt + 1 < KT) STEM_LOAD_FX(kt + 1, (kt + 1) & 1)
                __builtin_amdgcn_sched_barrier(0);
                // the four accumulator chains take their six terms in turn
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) x3_term(t, fw[nb][kt], fx[kt & 1][u], acc[u][nb]);
                __builtin_amdgcn_sched_barrier(0);
            }
#undef STEM_LOAD_FX
            // accumulator (u, nb) of this lane = conv pixel p[u], channels 32 half + 16 nb + 4 g + (0..3)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (p[u] >= NPIX) continue;
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = fmaxf(__builtin_fmaf(acc[u][nb][e], sc[nb][e], sh[nb][e]), 0.f);
                    *reinterpret_cast<f32x4 *>(ct + p[u] * CT_LD + 32 * half + 16 * nb + 4 * g) = o;
                }
            }
        }
        __syncthreads();

        // ---- pool: a thread = 4 channels of one pooled pixel; the window's pixels outside the conv map are skipped (padding)
#pragma unroll
        for (int i = 0; i < TPH * TPW * 16 / 256; ++i) {
            const int o = tid + 256 * i;
            const int c4 = o & 15, pix = o >> 4;
            const int phl = pix / TPW, pwl = pix - phl * TPW;
            const int ph = ph0 + phl, pw = pw0 + pwl;
            if (ph >= a.Hp || pw >= a.Wp) continue;
            f32x4 m = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                if ((unsigned)(2 * ph - 1 + dy) >= (unsigned)a.Hc) continue;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    if ((unsigned)(2 * pw - 1 + dx) >= (unsigned)a.Wc) continue;
                    const f32x4 q = *reinterpret_cast<const f32x4 *>(ct + ((2 * phl + dy) * CW + 2 * pwl + dx) * CT_LD + 4 * c4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) m[e] = max_nan(m[e], q[e]);
                }
            }
            *reinterpret_cast<f32x4 *>(a.y + (((size_t)b * a.Hp + ph) * a.Wp + pw) * a.y_ld + 4 * c4) = m;
        }
    }
#undef STEM_LOAD_PATCH
#undef STEM_TILE
}

}  // namespace

extern "C" int sgv3d_stem_pool_x3_forward(int batch, int h, int w, const float *x_nchw, const void *w_x3, size_t w_bytes,
                                          const float *scale, const float *shift, float *y_nhwc, int y_ld, int variant, void *stream) {
    SGV3D_REQUIRE(x_nchw && w_x3 && y_nhwc, "stem_pool_x3_forward: null pointer");
    SGV3D_REQUIRE(batch > 0 && h > 0 && w > 0, "stem_pool_x3_forward: bad shape (batch=%d h=%d w=%d)", batch, h, w);
    SGV3D_REQUIRE(y_ld >= 64 && y_ld % 4 == 0, "stem_pool_x3_forward: y_ld = %d must be a multiple of 4, at least 64", y_ld);
    SGV3D_REQUIRE(variant == 0, "stem_pool_x3_forward: unknown variant %d (0: 4 x 16 pooled pixels per workgroup)", variant);
    SGV3D_REQUIRE((scale == nullptr) == (shift == nullptr), "stem_pool_x3_forward: scale and shift come together");
    // the pack of a 64 x 3 x 7 x 7 weight with cin_pad 4, cout_pad 64: 4 blocks x 7 k-steps x 3 planes x 1 KB
    SGV3D_REQUIRE(w_bytes >= 86016 && w_bytes < 0xf0000000ull, "stem_pool_x3_forward: the weight pack has %zu bytes, needs 86016", w_bytes);
    SGV3D_REQUIRE(((reinterpret_cast<uintptr_t>(w_x3) | reinterpret_cast<uintptr_t>(y_nhwc) | reinterpret_cast<uintptr_t>(scale) |
                    reinterpret_cast<uintptr_t>(shift)) & 15) == 0 && (reinterpret_cast<uintptr_t>(x_nchw) & 3) == 0,
                  "stem_pool_x3_forward: weights, scale, shift and output must be 16-B aligned");
    constexpr int TPH = 4, TPW = 16;
    StemPoolArgs a;
    a.x = x_nchw; a.w = w_x3; a.scale = scale; a.shift = shift; a.y = y_nhwc;
    a.H = h; a.W = w;
    a.Hc = (h - 1) / 2 + 1; a.Wc = (w - 1) / 2 + 1;
    a.Hp = (a.Hc - 1) / 2 + 1; a.Wp = (a.Wc - 1) / 2 + 1;
    a.y_ld = y_ld;
    a.tiles_h = cdiv(a.Hp, TPH); a.tiles_w = cdiv(a.Wp, TPW);
    a.w_bytes = (unsigned)w_bytes;
    const long long tiles = (long long)batch * a.tiles_h * a.tiles_w, xb = (long long)batch * h * w * 12;
    SGV3D_REQUIRE(tiles < 0x7fffffffLL && xb < 0xf0000000LL, "stem_pool_x3_forward: images larger than 3.75 GiB (32-bit buffer offsets)");
    a.ntiles = (int)tiles;
    a.x_bytes = (unsigned)xb;
    // persistent workgroups, one per CU (its LDS holds one): each keeps the weights in registers over all its tiles
    static int cus = 0;
    if (cus == 0) {
        int dev = 0, n = 0;
        cus = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    const unsigned wgs = (unsigned)(tiles < cus ? tiles : cus);
    hipLaunchKernelGGL((stem_pool_x3_kernel<TPH, TPW>), dim3(wgs), dim3(256), 0, as_stream(stream), a);
    return check_launch("stem_pool_x3_kernel");
}
