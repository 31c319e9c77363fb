// Stand-alone sanitizer program for the host entry of the device AP evaluator (sgv3d_kitti_eval_device_host,
// csrc/kitti_eval_device.hip): random frames with 0, 1, 63, 64, 65 and 130 detections against 0, 1, 7 and 65 ground-truth
// boxes, every name kind, tied scores and overlaps; the packed input, both overlap arrays and every output live in their own
// exactly sized heap blocks, so that AddressSanitizer sees any access past a row, an image or a cell.  CPU only: no kernel
// is launched.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer tools/device_eval_host_check.cpp sgv3d_amd/csrc/kitti_eval_device.hip \
//       sgv3d_amd/csrc/rotate_iou.hip sgv3d_amd/csrc/common.cpp -o device_eval_host_check && \
//       ASAN_OPTIONS=detect_leaks=0 ./device_eval_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/sgv3d_hip.h"

namespace {

uint32_t state = 20261019u;
uint32_t next() {
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}
double pick(std::initializer_list<double> v) { return v.begin()[next() % v.size()]; }
size_t up8(size_t n) { return (n + 7) / 8 * 8; }

}  // namespace

int main() {
    const int gt_counts[] = {0, 1, 7, 65, 3, 12, 9, 0}, dt_counts[] = {130, 65, 64, 63, 1, 0, 20, 5};
    const int M = 8, C = 4;
    std::vector<int32_t> gt_off(M + 1, 0), dt_off(M + 1, 0), tile_off(M + 1, 0);
    std::vector<long long> ov_off(M + 1, 0);
    for (int m = 0; m < M; ++m) {
        gt_off[m + 1] = gt_off[m] + gt_counts[m];
        dt_off[m + 1] = dt_off[m] + dt_counts[m];
        tile_off[m + 1] = tile_off[m] + ((dt_counts[m] + 15) / 16) * ((gt_counts[m] + 15) / 16);
        ov_off[m + 1] = ov_off[m] + (long long)gt_counts[m] * dt_counts[m];
    }
    const int TG = gt_off[M], TD = dt_off[M];
    const long long pairs = ov_off[M];
    // the packed input, section after section (include/sgv3d_hip.h)
    const size_t bytes = (size_t)(M + 1) * 8 + 3 * up8((size_t)(M + 1) * 4) + (size_t)TG * 14 * 8 + (size_t)TD * 13 * 8 + up8((size_t)TG * 4) +
                         up8((size_t)TD * 4);
    std::vector<double> block(bytes / 8);          // 8-byte aligned, exactly `bytes` long
    char *p = (char *)block.data();
    std::memcpy(p, ov_off.data(), (M + 1) * 8); p += (M + 1) * 8;
    std::memcpy(p, gt_off.data(), (M + 1) * 4); p += up8((M + 1) * 4);
    std::memcpy(p, dt_off.data(), (M + 1) * 4); p += up8((M + 1) * 4);
    std::memcpy(p, tile_off.data(), (M + 1) * 4); p += up8((M + 1) * 4);
    double *gt = (double *)p; p += (size_t)TG * 14 * 8;
    double *dt = (double *)p; p += (size_t)TD * 13 * 8;
    int32_t *gt_name = (int32_t *)p; p += up8((size_t)TG * 4);
    int32_t *dt_cls = (int32_t *)p;
    auto box = [](double *b) {
        b[0] = pick({0, 50, 100, 400}); b[1] = pick({0, 20});
        b[2] = b[0] + pick({100, 150}); b[3] = b[1] + pick({20, 25, 30, 40, 41, 60, 90, 120});
    };
    for (int g = 0; g < TG; ++g) {
        double *r = gt + (size_t)g * 14;
        box(r);
        r[4] = (double)(next() % 60) / 10 - 3;
        for (int k = 5; k < 12; ++k) r[k] = 1.0 + (next() % 7);
        r[12] = pick({0, 0, 0.1, 0.2, 0.4, 0.6});
        r[13] = pick({0, 0, 1, 2, 3});
        const uint32_t kind = next() % 9;
        gt_name[g] = kind < 7 ? (int32_t)kind : (kind == 7 ? (6 | 8) : 0);        // every kind, DontCare, more cars
    }
    for (int d = 0; d < TD; ++d) {
        double *r = dt + (size_t)d * 13;
        r[0] = (double)(next() % 60) / 10 - 3;
        box(r + 1);
        for (int k = 5; k < 12; ++k) r[k] = 1.0 + (next() % 7);
        r[12] = (double)(next() % 11) / 10;
        dt_cls[d] = (int32_t)(next() % 5);
    }
    std::vector<float> bev(pairs), d3(pairs);
    for (long long i = 0; i < pairs; ++i) {
        bev[i] = next() % 5 < 3 ? (float)(next() % 11) / 10 : 0.f;
        d3[i] = next() % 5 < 3 ? (float)(next() % 11) / 10 : 0.f;
    }
    const int32_t classes[C] = {0, 1, 2, 3};
    std::vector<double> mo(2 * 3 * C);
    for (int k = 0; k < 2; ++k)
        for (int m = 0; m < 3; ++m)
            for (int c = 0; c < C; ++c) mo[(k * 3 + m) * C + c] = (c == 0 || c == 3) ? (k && m ? 0.5 : 0.7) : (k && m ? 0.25 : 0.5);
    const size_t n = (size_t)18 * C * 41;
    std::vector<double> precision(n, -1), recall(n, -1), orientation(n, -1), thresholds(n, -1);
    std::vector<int32_t> nthr(18 * C, -7), status(1, -7);
    const int rc = sgv3d_kitti_eval_device_host(M, TG, TD, pairs, block.data(), bytes, bev.data(), d3.data(), C, classes, mo.data(), 1,
                                                precision.data(), recall.data(), orientation.data(), nthr.data(), status.data(),
                                                thresholds.data());
    if (rc != 0) {
        std::printf("sgv3d_kitti_eval_device_host failed (%d): %s\n", rc, sgv3d_last_error());
        return 1;
    }
    int most = 0, cells = 0;
    double sum = 0;
    for (int c = 0; c < 18 * C; ++c) {
        most = nthr[c] > most ? nthr[c] : most;
        cells += nthr[c] > 0;
        for (int t = 0; t < nthr[c]; ++t) sum += precision[(size_t)c * 41 + t] + recall[(size_t)c * 41 + t] + orientation[(size_t)c * 41 + t];
    }
    std::printf("status %d, %d of %d cells with thresholds, at most %d, checksum %.9f\n", status[0], cells, 18 * C, most, sum);
    // bad calls are refused before anything is touched: a class id outside 0..3, offsets that do not end at the totals
    const int32_t bad_classes[C] = {0, 1, 2, 4};
    if (sgv3d_kitti_eval_device_host(M, TG, TD, pairs, block.data(), bytes, bev.data(), d3.data(), C, bad_classes, mo.data(), 1, precision.data(),
                                     recall.data(), orientation.data(), nthr.data(), status.data(), nullptr) != -1)
        return 2;
    if (sgv3d_kitti_eval_device_host(M, TG, TD, pairs - 1, block.data(), bytes, bev.data(), d3.data(), C, classes, mo.data(), 1, precision.data(),
                                     recall.data(), orientation.data(), nthr.data(), status.data(), nullptr) != -1)
        return 3;
    const bool ok = status[0] == 0 && most >= 3 && cells >= 12 && std::isfinite(sum);
    std::printf(ok ? "OK\n" : "unexpected result\n");
    return ok ? 0 : 4;
}
