// Stand-alone sanitizer program for the host entry of the frame recombination (sgv3d_recombine_host, csrc/recombine.hip):
// a 37 x 61 batch of two generated frames (three sources and one source) with perturbed homographies, boxes that are
// accepted, rejected, clamped and dropped, and every output placed in its own exactly sized heap block, so that
// AddressSanitizer sees any access past a row, a frame or a list.  CPU only: no kernel is launched.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer tools/recombine_host_check.cpp sgv3d_amd/csrc/recombine.hip \
//       sgv3d_amd/csrc/common.cpp -o recombine_host_check && ASAN_OPTIONS=detect_leaks=0 ./recombine_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/sgv3d_hip.h"

namespace {

uint32_t state = 20261018u;
uint32_t next() {
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

// an object of the flat camera (Tr = I, P2 = [I | 0], depth 1): its float box is (x0, y0, x1, y1)
void flat_object(double *o, double x0, double y0, double x1, double y1) {
    const double xs[8] = {x1, x1, x0, x0, x1, x1, x0, x0}, ys[8] = {y1, y0, y0, y1, y1, y0, y0, y1};
    for (int k = 0; k < 8; ++k) o[k] = xs[k], o[8 + k] = ys[k], o[16 + k] = 1.0;
    o[24] = 1.5, o[25] = 1.8, o[26] = 4.4, o[27] = 0.0, o[28] = 1.0, o[29] = 0.875;
}

}  // namespace

int main() {
    const int H = 37, W = 61, pool = 4, batch = 2, max_obj = 9;
    const size_t px = (size_t)H * W;
    std::vector<uint8_t> images(pool * px * 3), masks(pool * px);
    for (auto &v : images) v = (uint8_t)next();
    for (auto &v : masks) v = (uint8_t)(next() % 9);
    const double boxes[9][4] = {{5, 4, 30, 20},                                                        // the destination's
                                {6, 5, 31, 21}, {33, 5, 58, 30}, {-9, 3, 0, 9}, {40, 10, 200, 90},      // source 0
                                {2, 24, 20, 35}, {2.9, 24, 3.9, 35},                                    // source 1
                                {-5, -5, 200, 200},                                                    // source 2
                                {10, 10, 50, 30}};                                                     // frame 1, source 0
    std::vector<double> objects(9 * 30);
    std::vector<int32_t> classes = {9, 0, 3, 0, 4, 5, 1, 2, 1};   // the destination's own may be any known name
    for (int i = 0; i < 9; ++i) flat_object(&objects[i * 30], boxes[i][0], boxes[i][1], boxes[i][2], boxes[i][3]);
    std::vector<sgv3d_recombine_frame> fr(batch);
    std::memset(fr.data(), 0, batch * sizeof(sgv3d_recombine_frame));
    const double flat_tr[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int b = 0; b < batch; ++b) {
        std::memcpy(fr[b].tr, flat_tr, sizeof flat_tr);
        std::memcpy(fr[b].p2, flat_tr, sizeof flat_tr);
        for (int s = 0; s < 3; ++s) {
            const double m[9] = {1.0 + 0.01 * s, 0.003 * (b + 1), 1.7 - s, -0.004, 0.99, 0.6 * s - 0.9, 1e-5 * s, -2e-5, 1.0};
            std::memcpy(fr[b].minv[s], m, sizeof m);
        }
    }
    fr[0].dest = 0, fr[0].n_src = 3, fr[0].src[0] = 1, fr[0].src[1] = 2, fr[0].src[2] = 3, fr[0].obj0 = 0;
    fr[0].n_obj[0] = 1, fr[0].n_obj[1] = 4, fr[0].n_obj[2] = 2, fr[0].n_obj[3] = 1;
    fr[1].dest = 3, fr[1].n_src = 1, fr[1].src[0] = 0, fr[1].obj0 = 8, fr[1].n_obj[1] = 1;
    std::vector<uint8_t> out_images(batch * px * 3), out_masks(batch * px);
    std::vector<double> beta(batch * 3), fbox(batch * max_obj * 4), rows(batch * max_obj * 15);
    std::vector<int32_t> kept(batch * max_obj, -7), n_rows(batch), info(batch * max_obj * 2);
    std::vector<float> warped(batch * 3 * px * 3);
    const int rc = sgv3d_recombine_host(batch, pool, H, W, max_obj, 9, fr.data(), images.data(), masks.data(), objects.data(), classes.data(),
                                        out_images.data(), out_masks.data(), beta.data(), fbox.data(), kept.data(), n_rows.data(),
                                        rows.data(), info.data(), warped.data());
    if (rc != 0) {
        std::printf("sgv3d_recombine_host failed (%d): %s\n", rc, sgv3d_last_error());
        return 1;
    }
    unsigned long long sum = 0;
    for (auto v : out_images) sum = sum * 31 + v;
    for (auto v : out_masks) sum = sum * 31 + v;
    std::printf("rows %d %d, kept", n_rows[0], n_rows[1]);
    for (int i = 0; i < 8; ++i) std::printf(" %d", kept[i]);
    std::printf(" | %d, beta %.6f %.6f %.6f | %.6f, checksum %llu\n", kept[max_obj], beta[0], beta[1], beta[2], beta[3], sum);
    // one bad call: more objects than max_obj must be refused before anything is touched
    if (sgv3d_recombine_host(batch, pool, H, W, 7, 9, fr.data(), images.data(), masks.data(), objects.data(), classes.data(), out_images.data(),
                             out_masks.data(), beta.data(), fbox.data(), kept.data(), n_rows.data(), rows.data(), info.data(), nullptr) != -1)
        return 2;
    const bool ok = n_rows[0] >= 2 && kept[1] == 0 && kept[2] == 1 && kept[3] == 0 && kept[6] == 0 && std::isfinite(beta[0]);
    std::printf(ok ? "OK\n" : "unexpected result\n");
    return ok ? 0 : 3;
}
