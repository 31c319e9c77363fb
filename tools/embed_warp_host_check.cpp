// Stand-alone sanitizer program for the host entry of the embedding warp (sgv3d_embed_warp_host, csrc/embed_distill.hip):
// a batch of four 11 x 19 x 12 embeddings (a strong warp, a shrinking one whose border is dead, an unwarped frame, and a matrix
// that throws every position far outside or onto not-a-number), with every buffer in its own exactly sized heap block, so that
// AddressSanitizer sees any access past a row or a frame.  Then the smallest map (2 x 2 x 4).  CPU only: no kernel is launched.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer tools/embed_warp_host_check.cpp sgv3d_amd/csrc/embed_distill.hip \
//       sgv3d_amd/csrc/common.cpp -o embed_warp_host_check && ASAN_OPTIONS=detect_leaks=0 ./embed_warp_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/sgv3d_hip.h"

namespace {

uint32_t state = 20261020u;
float next() {
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) / 8388608.0f - 1.0f;
}

}  // namespace

int main() {
    const int B = 4, H = 11, W = 19, C = 12;
    const size_t px = (size_t)H * W;
    std::vector<float> teacher(B * px * C), out(B * px * C, -7.f);
    for (auto &v : teacher) v = next();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> minv = {
        0.77, 0.05, 1.9, -0.05, 0.77, 1.1, 1e-4, -2e-4, 1.0,        // strong: zoom in, rotate
        1.25, -0.04, -2.2, 0.04, 1.25, -1.3, 0.0, 0.0, 1.0,         // shrink: the border reads outside
        nan, nan, nan, nan, nan, nan, nan, nan, nan,                // unwarped: never read
        1.0, 0.0, 1e300, 0.0, nan, 0.0, 0.0, 0.0, 1e-300,           // positions at infinity and not-a-number
    };
    std::vector<uint8_t> warped = {1, 1, 0, 1}, dead(B * px, 9);
    int rc = sgv3d_embed_warp_host(B, H, W, C, teacher.data(), minv.data(), warped.data(), out.data(), dead.data());
    if (rc != 0) {
        std::printf("sgv3d_embed_warp_host failed (%d): %s\n", rc, sgv3d_last_error());
        return 1;
    }
    size_t n_dead[4] = {0, 0, 0, 0};
    double sum = 0;
    bool ok = true;
    for (int b = 0; b < B; ++b)
        for (size_t p = 0; p < px; ++p) {
            const uint8_t d = dead[b * px + p];
            ok = ok && d <= 1;
            n_dead[b] += d;
            for (int c = 0; c < C; ++c) {
                const float v = out[(b * px + p) * C + c];
                ok = ok && std::isfinite(v) && std::fabs(v) <= 1.0f && (!d || v == 0.f);
                sum += v;
            }
        }
    for (size_t i = 0; i < px * C; ++i) ok = ok && out[2 * px * C + i] == teacher[2 * px * C + i];
    std::printf("dead %zu %zu %zu %zu of %zu, sum %.9f\n", n_dead[0], n_dead[1], n_dead[2], n_dead[3], px, sum);
    ok = ok && n_dead[0] < px / 4 && n_dead[1] > px / 4 && n_dead[1] < px && n_dead[2] == 0 && n_dead[3] == px;

    // the smallest map, no dead output: only the pixel (0, 0) of an identity warp survives
    std::vector<float> t2(2 * 2 * 4), o2(2 * 2 * 4, -7.f);
    for (auto &v : t2) v = next();
    const std::vector<double> eye = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const uint8_t one = 1;
    rc = sgv3d_embed_warp_host(1, 2, 2, 4, t2.data(), eye.data(), &one, o2.data(), nullptr);
    for (int c = 0; c < 4; ++c) ok = ok && rc == 0 && o2[c] == t2[c] && o2[4 + c] == 0.f && o2[8 + c] == 0.f && o2[12 + c] == 0.f;

    // bad calls are refused before anything is touched
    if (sgv3d_embed_warp_host(B, 1, W, C, teacher.data(), minv.data(), warped.data(), out.data(), nullptr) != -1) return 2;
    if (sgv3d_embed_warp_host(B, H, W, 10, teacher.data(), minv.data(), warped.data(), out.data(), nullptr) != -1) return 2;
    if (sgv3d_embed_warp_host(B, H, W, C, teacher.data(), minv.data(), warped.data(), teacher.data() + C, nullptr) != -1) return 2;
    std::printf(ok ? "OK\n" : "unexpected result\n");
    return ok ? 0 : 3;
}
