// Stand-alone sanitizer program for the host twin of the renderer (sgv3d_render_detections_host, csrc/render.hip): three 37 x 61
// frames with boxes in view, across every frame edge and the near plane, behind the camera, far outside, at NaN and at infinity,
// with labels, a mask and a BEV canvas, every buffer in its own exactly sized heap block, so that AddressSanitizer sees any
// access past a row, a frame or a list.  Then in place, an overflowing sample, and refused calls.  CPU only: no kernel is
// launched.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer tools/render_host_check.cpp sgv3d_amd/csrc/render.hip \
//       sgv3d_amd/csrc/common.cpp -o render_host_check && ASAN_OPTIONS=detect_leaks=0 ./render_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sgv3d_hip.h"

namespace {

uint32_t state = 20261021u;
uint32_t next() {
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

}  // namespace

int main() {
    const int B = 3, N = 15, M = 3, H = 37, W = 61, BH = 81, BW = 49;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    sgv3d_render_desc d;
    std::memset(&d, 0, sizeof(d));
    d.batch = B, d.n = N, d.m = M, d.height = H, d.width = W, d.bev_h = BH, d.bev_w = BW, d.bev_x_off = -24, d.bev_y_off = 80;
    d.max_boxes = 16, d.thickness = 3, d.f64_inputs = 1, d.num_classes = 4, d.mask_alpha = 96;
    d.score_thr = 0.45, d.z_near = 0.5, d.bev_res = 0.25;
    d.class_table[0] = 0, d.class_table[1] = 1, d.class_table[2] = 2, d.class_table[3] = -1;
    for (int k = 0; k < 12; ++k) d.class_colors[k] = (uint8_t)(40 + 17 * k);
    d.label_color[0] = 255, d.bev_pred_color[2] = 255, d.bev_label_color[0] = 255;
    for (int k = 0; k < 21; ++k) d.palette[k] = (uint8_t)(11 * k);
    const double rows[N][8] = {                                  // x, y, z, l, w, h, yaw, score
        {12, 0.3, 0, 4.2, 1.9, 1.6, 0.3, 0.9},  {10, 10.2, 0, 4, 2, 1.5, 0.1, 0.8},   {10, -10.1, 0, 4, 2, 1.5, -0.2, 0.8},
        {8, 1, 6.3, 3, 2, 2.5, 0.7, 0.7},       {6, -1, -2.6, 3, 2, 2, 1.1, 0.7},     {1.2, 0.4, 0.2, 4, 1.8, 1.4, 0.05, 0.95},
        {-10, 0, 0, 4, 2, 1.5, 0, 0.9},         {5, 700, 0, 4, 2, 1.5, 0, 0.9},       {15, 2, 0.5, 0, 0, 0, 0.4, 0.9},
        {nan, 1, 0, 4, 2, 1.5, 0.2, 0.9},       {14, -2, 0, 4, 2, 1.5, 0.2, 0.45},    {13, 3, 0, 1, 1, 1, inf, 0.9},
        {1e300, -1e300, 0, 1e300, 2, 1.5, 0.2, 0.9}, {16, -3, 0, 4.5, 2, 1.7, 0.5, 0.6},
        {0.9, 0, 0, 1e307, 0.2, 1, 0, 0.9}};                     // finite projections near -+1.7e308 whose difference is not
    std::vector<double> boxes((size_t)B * N * 9, 0.0), scores((size_t)B * N), calib((size_t)B * 33, 0.0), labels7((size_t)B * M * 7);
    std::vector<int32_t> cls((size_t)B * N), counts = {N, N - 3, 0}, lcounts = {M, 1, 0}, status(B, -9);
    for (int b = 0; b < B; ++b) {
        for (int r = 0; r < N; ++r) {
            for (int k = 0; k < 7; ++k) boxes[((size_t)b * N + r) * 9 + k] = rows[r][k] + (k == 0 ? 0.37 * b : 0.0);
            scores[(size_t)b * N + r] = rows[r][7];
            cls[(size_t)b * N + r] = r % 4 == 3 ? (r == 11 ? 7 : 3) : r % 3;      // class 7 is out of range, class 3 unmapped
        }
        double *c = calib.data() + (size_t)b * 33;                 // camera along lidar +x, 1.5 m up
        c[1] = -1, c[6] = -1, c[7] = 1.5, c[8] = 1;
        c[12] = W / 2 + 0.37, c[14] = W / 2 - 0.21, c[16] = W / 2 + 0.11, c[17] = H / 2 + 0.4, c[20] = 1;
        c[21] = c[25] = c[29] = 1;
        c[30] = 0.1 * b;
        const double lab[M][7] = {{12.2, 0.2, 0.05, 4, 1.8, 1.5, 0.28}, {16.2, -2.9, 0, 4.4, 2.1, 1.6, 0.52}, {9, 30, 0, 4, 2, 1.5, nan}};
        for (int r = 0; r < M; ++r)
            for (int k = 0; k < 7; ++k) labels7[((size_t)b * M + r) * 7 + k] = lab[r][k];
    }
    std::vector<uint8_t> frames((size_t)B * H * W * 3), masks((size_t)B * H * W), out(frames.size(), 0xA5), bev((size_t)B * BH * BW * 3, 0xA5);
    for (auto &v : frames) v = (uint8_t)next();
    for (auto &v : masks) v = (uint8_t)next();

    int rc = sgv3d_render_detections_host(&d, boxes.data(), scores.data(), cls.data(), counts.data(), calib.data(), labels7.data(),
                                          lcounts.data(), frames.data(), masks.data(), out.data(), bev.data(), status.data());
    if (rc != 0) {
        std::printf("sgv3d_render_detections_host failed (%d): %s\n", rc, sgv3d_last_error());
        return 1;
    }
    size_t drawn = 0, lit = 0;
    for (size_t i = 0; i < out.size(); ++i) drawn += out[i] != frames[i];
    for (auto v : bev) lit += v != 0;
    bool ok = status[0] == 0 && status[1] == 0 && status[2] == 0 && drawn > 1000 && lit > 100;
    std::printf("drawn bytes %zu, canvas bytes %zu, status %d %d %d\n", drawn, lit, status[0], status[1], status[2]);

    // in place, no mask, no canvas, float32 inputs: sample 2 has nothing to draw and keeps its bytes
    std::vector<float> boxes32(boxes.begin(), boxes.end()), scores32(scores.begin(), scores.end());
    std::vector<uint8_t> mine(frames);
    sgv3d_render_desc e = d;
    e.bev_h = e.bev_w = 0, e.f64_inputs = 0, e.m = 0, e.thickness = 1;
    rc = sgv3d_render_detections_host(&e, boxes32.data(), scores32.data(), cls.data(), counts.data(), calib.data(), nullptr, nullptr,
                                      mine.data(), nullptr, mine.data(), nullptr, status.data());
    const size_t frame = (size_t)H * W * 3;
    ok = ok && rc == 0 && std::memcmp(mine.data() + 2 * frame, frames.data() + 2 * frame, frame) == 0 &&
         std::memcmp(mine.data(), frames.data(), frame) != 0;

    // overflow: sample 0 keeps more than max_boxes detections and is copied through, sample 1 has too many labels
    e = d;
    e.max_boxes = 2;
    counts[1] = 1;
    lcounts[0] = 0, lcounts[1] = 3;
    std::fill(out.begin(), out.end(), (uint8_t)0xA5);
    rc = sgv3d_render_detections_host(&e, boxes.data(), scores.data(), cls.data(), counts.data(), calib.data(), labels7.data(),
                                      lcounts.data(), frames.data(), nullptr, out.data(), bev.data(), status.data());
    ok = ok && rc == 0 && status[0] == SGV3D_RENDER_EOVERFLOW && status[1] == SGV3D_RENDER_EOVERFLOW && status[2] == 0 &&
         std::memcmp(out.data(), frames.data(), out.size()) == 0;
    for (auto v : bev) ok = ok && v == 0;

    // bad calls are refused before anything is touched
    e = d;
    e.thickness = 16;
    if (sgv3d_render_detections_host(&e, boxes.data(), scores.data(), cls.data(), counts.data(), calib.data(), labels7.data(), lcounts.data(),
                                     frames.data(), masks.data(), out.data(), bev.data(), status.data()) != -1)
        return 2;
    if (sgv3d_render_detections_host(&d, boxes.data(), scores.data(), cls.data(), counts.data(), calib.data(), labels7.data(), lcounts.data(),
                                     frames.data(), masks.data(), frames.data() + 3, bev.data(), status.data()) != -1)
        return 2;
    if (sgv3d_render_workspace_bytes(&e) != 0 || sgv3d_render_workspace_bytes(&d) == 0) return 2;
    std::printf(ok ? "OK\n" : "unexpected result\n");
    return ok ? 0 : 3;
}
