// Deformable 3x3 convolution (mmcv 1.4.0 DeformConv2dPack / DCNv1 as configured at layers/backbones/lss_fpn.py:190-198: 3x3,
// stride 1, pad 1, dilation 1, groups 4, deform_groups 1, no bias) in ONE launch on the bf16 matrix cores -- the bf16-mode twin
// of dcn_fused.hip:
//
//   out[p][g * opg + co] = sum_tap sum_ci bf16(W[g][co][tap * cpg + ci]) * bf16(bilinear(x[:, :, g * cpg + ci], p + tap + offset[p][tap]))
//
// The bf16 mode used to write the sampled column tensor [B, H, W, 9 C] to HBM (sgv3d_deform_im2col3x3_bf16: 301 MB at
// 4 x 68 x 120 x 512) and read it back with one 1x1 GEMM per group.  Here a sample goes from the input map into the GEMM's LDS
// stage and is formed ONCE: a workgroup owns 64 pixels and (up to) 128 output channels of one group -- all of them for the
// layer's 128 per group.
//
//   workgroup   256 threads = 4 waves; tile 64 pixels x 128 output channels (of one group) x 32 k per step; a wave owns all 64
//               pixels x 32 channels: 2 x 4 accumulators of v_mfma_f32_16x16x32_bf16 (32 VGPRs).  The weights are the A operand
//               (channel on the row), so that a lane ends up with 4 consecutive output channels of one pixel (16-byte / 8-byte
//               stores).
//   samples     k-step kt = (tap, 32-channel chunk of the group).  Thread (pixel r = tid / 4, 8 channels c = tid % 4) derives per
//               tap the four corner offsets (out of range for corners outside the image, for whole samples outside it and for
//               the rows past B H W: the buffer load returns zeros, the reference's zero padding, without a branch) and the four
//               bilinear weights from the (dy, dx) pairs staged in LDS once per workgroup; per k-step it issues four 16-byte
//               loads (bf16 x; eight for f32 x), combines them in f32, rounds once to bf16 and stores 16 bytes into the
//               double-buffered LDS tile [64 pixels][32 k] (64-byte rows, 16-byte slots XOR-swizzled with (pixel >> 2) & 3: the
//               fragment reads of 16 pixels x one slot hit 16 different slots of the 256-byte bank row).  One barrier per k-step.
//   weights     never in LDS: packed once (dcn_bf16_pack_kernel) in fragment order [group][16-channel block][k-step][lane][8] and
//               streamed from L2 one k-step ahead, 1 KiB contiguous per wave and load.
//   epilogue    raw accumulators (the layer has neither bias nor norm) as f32, or rounded once to bf16.
//
// Arithmetic of a sample: bit for bit what sgv3d_deform_im2col3x3_bf16 / sgv3d_deform_im2col3x3 (then rounded to bf16 by the
// GEMM) feed the im2col form's GEMMs.  Those two kernels are built with the compiler's default contraction, which turns their
// w1 v1 + w2 v2 + w3 v3 + w4 v4 into  fma(w4, v4, fma(w3, v3, fma(w1, v1, w2 * v2)))  (the product w2 v2 is the one that is
// rounded); that chain is written out below with explicit fmaf, and this file is built with -ffp-contract=off so that nothing
// else (position, fractions, the weights' products) is contracted either.  tests/test_dcn_bf16_gpu.py compares against the
// column tensor of those kernels themselves.
// Summation: f32 accumulation inside the MFMA, k-steps in ascending (tap, channel) order, no split along k: a fixed order.
//
// Bound (nothing here was analysed beyond this count): per k-step and workgroup 8 MFMAs of 16 cycles per wave beside ~60
// vector-ALU instructions per thread and 24 KiB through the CU's vector-memory path (16 KiB of corner rows, 8 KiB of weight
// fragments) -- the sampling, not the matrix pipe.
//
// Resource usage (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage), f32 and bf16 output alike:
//   bf16 x: 105 VGPRs, 0 AGPRs, 12800 bytes of LDS, 0 bytes of scratch, 4 waves per SIMD
//   f32 x:  121 VGPRs, 0 AGPRs, 12800 bytes of LDS, 0 bytes of scratch, 4 waves per SIMD
#include "conv_common.hpp"

using namespace sgv3d;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;                  // k per step: one MFMA
constexpr int BM = 64;                  // pixels per workgroup
constexpr int BN = 128;                 // output channels per workgroup (8 blocks of 16; a wave owns 2)
constexpr int kThreads = 256;
constexpr int kMaxGroups = 8;
constexpr int kFragB = 64 * 16;         // bytes of one weight fragment (64 lanes x 8 bf16)
constexpr unsigned kOutside = 0x80000000u;   // buffer offset past every tensor this entry accepts (< 2 GiB), also after + 16 + chunk

struct DcnBfArgs {
    const void *x;                  // NHWC [B, H, W, C], bf16 or f32
    const float *off;
    const void *w;                  // packed fragments (dcn_bf16_pack_kernel)
    void *y;                        // [B, H, W, y_ld], f32 or bf16
    int H, W, C, cpg, opg, groups;
    int M;                          // B * H * W
    int off_ld, y_ld, y_coff;
    int nkt;                        // k-steps: 9 * cpg / 32
    int nchunk;                     // 128-channel chunks per group: ceil(opg / 128)
    int tiles_m;
    unsigned x_bytes, w_bytes;
};

// weights OIHW f32 [groups * opg][cpg][3][3] -> [group][16-channel block nb < 8 nchunk][k-step][lane][8] bf16 (one rounding, to
// nearest even): lane l holds channel 16 nb + (l & 15), k = 32 kt + 8 (l >> 4) + j with k = tap * cpg + ci (the A operand layout
// of v_mfma_f32_16x16x32_bf16); zeros beyond opg
__global__ __launch_bounds__(64) void dcn_bf16_pack_kernel(const float *__restrict__ w, int cpg, int opg, int nkt, int nblk,
                                                           __bf16 *__restrict__ out) {
    const int id = blockIdx.x;                      // (g * nblk + nb) * nkt + kt
    const int kt = id % nkt, gnb = id / nkt;
    const int nb = gnb % nblk, g = gnb / nblk;
    const int kpt = cpg / BK;
    const int tap = kt / kpt, cb = kt - tap * kpt;
    const int l = threadIdx.x;
    const int co = nb * 16 + (l & 15);
    __bf16 *dst = out + ((size_t)id * 64 + l) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = cb * BK + 8 * (l >> 4) + j;
        dst[j] = co < opg ? (__bf16)w[((size_t)(g * opg + co) * cpg + ci) * 9 + tap] : (__bf16)0.f;
    }
}

// (by value: __builtin_bit_cast applied directly to an element of an ext-vector reads element 0)
__device__ __forceinline__ float as_f32(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

template <bool XBF, bool YBF>
__global__ __launch_bounds__(kThreads, 2) void dcn3x3_fused_bf16_kernel(const DcnBfArgs a) {
    constexpr int ESZ = XBF ? 2 : 4;                // bytes per element of x
    constexpr int NLD = XBF ? 1 : 2;                // 16-byte loads per corner: 8 channels
    constexpr int kBufB = BM * BK * 2;              // bytes of one sample tile
    __shared__ __attribute__((aligned(16))) char smem[2 * kBufB];
    __shared__ float off_s[BM][18];

    // XCD-aware walk (as dcn3x3_fused_kernel): the workgroups of one XCD take consecutive logical tiles; the pixel tile changes
    // fastest, so that an XCD's L2 holds one group's weights and a band of the input map
    const int per_m = a.groups * a.nchunk;
    const int logical = xcd_tile(blockIdx.x, a.tiles_m * per_m);
    const int tgc = (int)((unsigned)logical / (unsigned)a.tiles_m);      // (group, channel chunk)
    const int tm = logical - tgc * a.tiles_m;
    const int grp = tgc / a.nchunk;
    const int chunk = tgc - grp * a.nchunk;
    const int m0 = tm * BM;

    const int tid = threadIdx.x;
    const int c = tid & 3, r = tid >> 2;            // this thread samples 8 channels (c) of pixel row r

    // ---- offsets of the tile's 64 pixels -> LDS (18 floats each; rows past M: zeros)
    for (int i = tid; i < BM * 18; i += kThreads) {
        const int rr = i / 18, cc = i - rr * 18;
        const int m = m0 + rr;
        off_s[rr][cc] = m < a.M ? a.off[(size_t)m * a.off_ld + cc] : 0.f;
    }

    const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.x, 0, (int)a.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)a.w, 0, (int)a.w_bytes, 0x00020000);

    // pixel coordinates of this thread's row
    const int m_row = m0 + r;
    const bool pok = m_row < a.M;
    int ph, pw;
    unsigned pbase;                // byte offset of (image b, this thread's 8 channels of the group) -- the corner's pixel offset is added
    {
        const int mm = pok ? m_row : 0;
        const unsigned t2 = (unsigned)mm / (unsigned)a.W;
        pw = (int)((unsigned)mm - t2 * a.W);
        const unsigned b = t2 / (unsigned)a.H;
        ph = (int)(t2 - b * a.H);
        pbase = (unsigned)(((size_t)b * a.H * a.W * a.C + (size_t)grp * a.cpg + c * 8) * ESZ);
    }
    char *const st_ptr = smem + r * (BK * 2) + ((c ^ ((r >> 2) & 3)) * 16);

    const int wave = tid >> 6, lane = tid & 63;
    const int l16 = lane & 15, lq = lane >> 4;
    // fragment reads: pixel row 16 mb + l16, logical 16-byte slot lq (k = 8 lq .. 8 lq + 7)
    const int rd_off = l16 * (BK * 2) + ((lq ^ ((l16 >> 2) & 3)) * 16);
    // this wave's two 16-channel blocks; a wave whose 32 channels lie beyond opg only samples (wave-uniform)
    const int col0 = chunk * BN + 32 * wave;                    // first channel of the wave inside the group
    const bool live0 = col0 < a.opg, live1 = col0 + 16 < a.opg;
    const int nblk = 8 * a.nchunk;
    const int nb0 = grp * nblk + chunk * 8 + 2 * wave;
    const unsigned w_off0 = (unsigned)((size_t)nb0 * a.nkt * kFragB + lane * 16);
    const unsigned w_off1 = w_off0 + (unsigned)(a.nkt * kFragB);

    f32x4 acc[2][4];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

    // per-tap sampling state: corner byte offsets (kOutside = absent) and bilinear weights
    unsigned co[4];
    float cw[4];
    u32x4 rx[4][NLD];
    bf16x8 wc[2], wn[2];
    const int kpt = a.cpg / BK;                  // k-steps per tap
    int ld_kt = 0, ld_tap = 0, ld_c = 0;         // next k-step to fetch: its tap and channel chunk inside the group

    __syncthreads();                             // off_s

    auto tap_params = [&]() {
        const int ky = ld_tap / 3, kx = ld_tap - ky * 3;
        const float oy = off_s[r][2 * ld_tap], ox = off_s[r][2 * ld_tap + 1];
        const float hf = (float)(ph - 1 + ky) + oy;
        const float wf = (float)(pw - 1 + kx) + ox;
        const bool in = pok && hf > -1.f && wf > -1.f && hf < (float)a.H && wf < (float)a.W;
        const int hl = (int)floorf(hf), wl = (int)floorf(wf);
        const int hh = hl + 1, wh = wl + 1;
        const float lh = hf - (float)hl, lw = wf - (float)wl;
        const float uh = 1.f - lh, uw = 1.f - lw;
        const bool k1 = in && hl >= 0 && wl >= 0, k2 = in && hl >= 0 && wh <= a.W - 1;
        const bool k3 = in && hh <= a.H - 1 && wl >= 0, k4 = in && hh <= a.H - 1 && wh <= a.W - 1;
        cw[0] = k1 ? uh * uw : 0.f; cw[1] = k2 ? uh * lw : 0.f;
        cw[2] = k3 ? lh * uw : 0.f; cw[3] = k4 ? lh * lw : 0.f;
        const unsigned cb = (unsigned)a.C * (unsigned)ESZ;
        co[0] = k1 ? pbase + (unsigned)(hl * a.W + wl) * cb : kOutside;
        co[1] = k2 ? pbase + (unsigned)(hl * a.W + wh) * cb : kOutside;
        co[2] = k3 ? pbase + (unsigned)(hh * a.W + wl) * cb : kOutside;
        co[3] = k4 ? pbase + (unsigned)(hh * a.W + wh) * cb : kOutside;
    };
    // requests the four corners of channel chunk ld_c of tap ld_tap and the weight fragments of k-step ld_kt
    auto load = [&]() {
        if (ld_c == 0) tap_params();
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int i = 0; i < NLD; ++i)
                rx[k][i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, co[k] + 16 * i, ld_c * (BK * ESZ), 0));
        wn[0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_off0, ld_kt * kFragB, 0));
        wn[1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_off1, ld_kt * kFragB, 0));
        ++ld_kt;
        if (++ld_c == kpt) { ld_c = 0; ++ld_tap; }
    };
    // bilinear combination in f32 (the contracted chain of the im2col kernels, see the head of the file), one rounding to bf16,
    // 16 bytes into sample tile `buf`
    auto combine_store = [&](int buf) {
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v1, v2, v3, v4;
            if constexpr (XBF) {
                const int d = e >> 1;
                v1 = (e & 1) ? bf16_hi(rx[0][0][d]) : bf16_lo(rx[0][0][d]);
                v2 = (e & 1) ? bf16_hi(rx[1][0][d]) : bf16_lo(rx[1][0][d]);
                v3 = (e & 1) ? bf16_hi(rx[2][0][d]) : bf16_lo(rx[2][0][d]);
                v4 = (e & 1) ? bf16_hi(rx[3][0][d]) : bf16_lo(rx[3][0][d]);
            } else {
                v1 = as_f32(rx[0][e >> 2][e & 3]);
                v2 = as_f32(rx[1][e >> 2][e & 3]);
                v3 = as_f32(rx[2][e >> 2][e & 3]);
                v4 = as_f32(rx[3][e >> 2][e & 3]);
            }
            float s = cw[1] * v2;
            s = __builtin_fmaf(cw[0], v1, s);
            s = __builtin_fmaf(cw[2], v3, s);
            s = __builtin_fmaf(cw[3], v4, s);
            v[e] = (__bf16)s;
        }
        *reinterpret_cast<bf16x8 *>(st_ptr + buf * kBufB) = v;
    };

    load();
    combine_store(0);
    wc[0] = wn[0]; wc[1] = wn[1];
    __syncthreads();
    int buf = 0;
    for (int kt = 0; kt < a.nkt; ++kt) {
        const bool have_next = kt + 1 < a.nkt;
        if (have_next) load();
        bf16x8 fx[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) fx[mb] = *reinterpret_cast<const bf16x8 *>(smem + buf * kBufB + mb * 16 * (BK * 2) + rd_off);
        if (live0) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[0][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[0], fx[mb], acc[0][mb], 0, 0, 0);
        }
        if (live1) {
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) acc[1][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[1], fx[mb], acc[1][mb], 0, 0, 0);
        }
        if (have_next) {
            combine_store(buf ^ 1);
            wc[0] = wn[0]; wc[1] = wn[1];
        }
        __syncthreads();
        buf ^= 1;
    }

    // accumulator (nb, mb): pixel m0 + 16 mb + l16, output channels (group grp) col0 + 16 nb + 4 lq + (0..3)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int col = col0 + 16 * nb + 4 * lq;
        if (col >= a.opg) continue;
        const size_t ybase = (size_t)(m0 + l16) * a.y_ld + a.y_coff + grp * a.opg + col;
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            if (m0 + 16 * mb + l16 >= a.M) continue;
            const size_t yo = ybase + (size_t)mb * 16 * a.y_ld;
            if constexpr (YBF) {
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (__bf16)acc[nb][mb][e];
                *reinterpret_cast<bf16x4 *>(static_cast<__bf16 *>(a.y) + yo) = o;
            } else {
                *reinterpret_cast<f32x4 *>(static_cast<float *>(a.y) + yo) = acc[nb][mb];
            }
        }
    }
}

bool dcn_bf16_geometry(int channels, int groups, int out_per_group, int *nkt, int *nblk, long long *bytes) {
    if (channels <= 0 || groups <= 0 || groups > kMaxGroups || channels % groups || out_per_group <= 0) return false;
    const int cpg = channels / groups;
    if (cpg % BK || out_per_group % 4) return false;
    *nkt = 9 * (cpg / BK);
    *nblk = 8 * cdiv(out_per_group, BN);
    *bytes = (long long)groups * *nblk * *nkt * kFragB;
    return *bytes < 0x7fffff00LL;
}

}  // namespace

extern "C" size_t sgv3d_deform_conv3x3_bf16_weight_bytes(int channels, int groups, int out_per_group) {
    int nkt, nblk;
    long long bytes;
    return dcn_bf16_geometry(channels, groups, out_per_group, &nkt, &nblk, &bytes) ? (size_t)bytes : 0;
}

extern "C" int sgv3d_deform_conv3x3_bf16_pack_weight(const float *weight, int channels, int groups, int out_per_group, void *w_packed,
                                                     void *stream) {
    int nkt = 0, nblk = 0;
    long long bytes = 0;
    SGV3D_REQUIRE(dcn_bf16_geometry(channels, groups, out_per_group, &nkt, &nblk, &bytes),
                  "deform_conv3x3_bf16_pack_weight: groups <= 8, channels %% groups == 0, channels per group %% 32, outputs per group %% 4 "
                  "(channels=%d groups=%d opg=%d)", channels, groups, out_per_group);
    SGV3D_REQUIRE(weight && w_packed, "deform_conv3x3_bf16_pack_weight: null pointer");
    hipLaunchKernelGGL(dcn_bf16_pack_kernel, dim3(groups * nblk * nkt), dim3(64), 0, as_stream(stream), weight, channels / groups,
                       out_per_group, nkt, nblk, static_cast<__bf16 *>(w_packed));
    return check_launch("dcn_bf16_pack_kernel");
}

extern "C" int sgv3d_deform_conv3x3_forward_bf16(int batch, int h, int w, int channels, int groups, int out_per_group, const void *x,
                                                 int x_is_bf16, const float *offset, int off_ld, const void *w_packed, void *y,
                                                 int y_is_bf16, int y_ld, int y_coff, void *stream) {
    SGV3D_REQUIRE(batch > 0 && h > 0 && w > 0 && channels > 0 && groups > 0 && groups <= kMaxGroups && channels % groups == 0 &&
                      out_per_group > 0 && off_ld >= 18,
                  "deform_conv3x3_forward_bf16: bad shape");
    int nkt = 0, nblk = 0;
    long long w_bytes = 0;
    SGV3D_REQUIRE(dcn_bf16_geometry(channels, groups, out_per_group, &nkt, &nblk, &w_bytes) && y_coff >= 0 && (y_ld & 3) == 0 &&
                      (y_coff & 3) == 0 && y_ld >= y_coff + groups * out_per_group,
                  "deform_conv3x3_forward_bf16: channels per group %% 32, outputs per group %% 4, output stride / offset %% 4 "
                  "(cpg=%d opg=%d y_ld=%d y_coff=%d)", channels / groups, out_per_group, y_ld, y_coff);
    SGV3D_REQUIRE(x && offset && w_packed && y, "deform_conv3x3_forward_bf16: null pointer");
    const long long M = (long long)batch * h * w;
    const long long x_bytes = M * channels * (x_is_bf16 ? 2 : 4);
    SGV3D_REQUIRE(M < 0x7fffffffLL && x_bytes < 0x7fffff00LL && M * y_ld < 0x7fffffffLL,
                  "deform_conv3x3_forward_bf16: input map larger than 2 GiB (32-bit buffer offsets)");
    SGV3D_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(w_packed)) & 15) == 0,
                  "deform_conv3x3_forward_bf16: pointers must be 16-B aligned");
    DcnBfArgs a;
    a.x = x; a.off = offset; a.w = w_packed; a.y = y;
    a.H = h; a.W = w; a.C = channels; a.cpg = channels / groups; a.opg = out_per_group; a.groups = groups;
    a.M = (int)M; a.off_ld = off_ld; a.y_ld = y_ld; a.y_coff = y_coff;
    a.nkt = nkt; a.nchunk = nblk / 8;
    a.tiles_m = cdiv(M, BM);
    a.x_bytes = (unsigned)x_bytes;
    a.w_bytes = (unsigned)w_bytes;
    const long long grid = (long long)a.tiles_m * groups * a.nchunk;
    SGV3D_REQUIRE(grid < 0x7fffffffLL, "deform_conv3x3_forward_bf16: too many tiles");
    const dim3 g((unsigned)grid), b(kThreads);
    hipStream_t s = as_stream(stream);
    if (x_is_bf16) {
        if (y_is_bf16) hipLaunchKernelGGL((dcn3x3_fused_bf16_kernel<true, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((dcn3x3_fused_bf16_kernel<true, false>), g, b, 0, s, a);
    } else {
        if (y_is_bf16) hipLaunchKernelGGL((dcn3x3_fused_bf16_kernel<false, true>), g, b, 0, s, a);
        else hipLaunchKernelGGL((dcn3x3_fused_bf16_kernel<false, false>), g, b, 0, s, a);
    }
    return check_launch("dcn3x3_fused_bf16_kernel");
}
