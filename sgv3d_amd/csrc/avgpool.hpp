// nn.AdaptiveAvgPool2d((1, 1)) (ASPP.global_avg_pool, layers/backbones/lss_fpn.py:81-86): the two deterministic stages the f32
// kernels (misc_layers.hip) and their bf16 twins (act_bf16.hip) share, so that both give the same bits on the same values.
//
//   1. partial   kAvgChunks workgroups per (image, channel group) sum a pixel range each: pixel lane g = 0..3 of the workgroup
//                adds pixels p0 + g, p0 + g + 4, ... in order, the four lanes combine as (l0 + l1) + (l2 + l3)
//                -> part[image][chunk][channel] in the caller's workspace (sgv3d_global_avgpool_workspace_bytes)
//   2. final     one workgroup per (image, 32 channels): lane k = 0..7 adds the partials of chunks 16 k .. 16 k + 15 in order, the
//                eight lanes combine as a fixed pairwise tree, then the division by the pixel count
//
// A channel's sum never depends on which form of stage 1 ran (16-byte loads of a channel quad, or one channel per thread).
// 128 chunks: a 512-channel 54x96 map is 256 workgroups of ~41 pixels, 11 dependent adds per thread of a 16-byte load each.  The
// 32-chunk form before it also launched 256 workgroups (8 channel groups x 32 chunks), but with 4-byte loads and 41 dependent adds
// per thread: the gain is the wider loads and the four times shorter chain, not the number of workgroups.
#pragma once
#include "common.hpp"

namespace sgv3d {

constexpr int kAvgBlock = 256;
constexpr int kAvgChunks = 128;
constexpr int kAvgFinalLanes = 8;          // kAvgChunks / 8 = 16 partials per lane
static_assert(kAvgChunks % kAvgFinalLanes == 0 && kAvgBlock == 32 * kAvgFinalLanes, "final stage: 32 channels x 8 lanes");

// the pixel range of a chunk
__device__ __forceinline__ void avgpool_chunk(int P, int chunk, int &p0, int &p1) {
    const int per = (P + kAvgChunks - 1) / kAvgChunks;
    p0 = chunk * per;
    p1 = min(P, p0 + per);
}

// stage 1, one channel per thread (any C, any leading dimension): 64 channels x 4 pixel lanes per workgroup.
// grid (ceil(C / 64), kAvgChunks, batch)
template <typename T>
__device__ __forceinline__ void avgpool_partial_scalar(int P, int C, int ld, const T *__restrict__ x, float *__restrict__ part) {
    __shared__ float red[4][64];
    const int b = blockIdx.z, chunk = blockIdx.y;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int g = threadIdx.x >> 6;
    int p0, p1;
    avgpool_chunk(P, chunk, p0, p1);
    float s = 0.f;
    if (c < C)
        for (int p = p0 + g; p < p1; p += 4) s += (float)x[((long long)b * P + p) * ld + c];
    red[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < C)
        part[((long long)b * kAvgChunks + chunk) * C + c] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// stage 2.  grid (ceil(C / 32), batch)
__device__ __forceinline__ void avgpool_final(int P, int C, const float *__restrict__ part, float *__restrict__ y) {
    __shared__ float red[kAvgFinalLanes][32];
    constexpr int kPer = kAvgChunks / kAvgFinalLanes;
    const int b = blockIdx.y, c = blockIdx.x * 32 + (threadIdx.x & 31), k = threadIdx.x >> 5;
    float s = 0.f;
    if (c < C) {
        const float *p = part + ((long long)b * kAvgChunks + k * kPer) * C + c;
#pragma unroll
        for (int j = 0; j < kPer; ++j) s += p[(long long)j * C];
    }
    red[k][threadIdx.x & 31] = s;
    __syncthreads();
    if (k == 0 && c < C) {
        const int t = threadIdx.x;
        const float s01 = red[0][t] + red[1][t], s23 = red[2][t] + red[3][t], s45 = red[4][t] + red[5][t], s67 = red[6][t] + red[7][t];
        y[(long long)b * C + c] = ((s01 + s23) + (s45 + s67)) / (float)P;
    }
}

}  // namespace sgv3d
