// Stand-alone sanitizer program for the host twin of the SAM mask compose (sgv3d_sam_mask_compose_host, csrc/sam_decoder.hip): the
// edge cases of tests/test_sam_masks_gpu.py -- original sizes 54 x 96, 27 x 48, 135 x 240 and 37 x 61 at img_size 96 (24 x 24 low-res
// logits), overlapping boxes, a label above 6, a label 0, an empty frame, a box on the last row and column, no boxes at all -- with
// every input and output in its own exactly sized heap block, so that AddressSanitizer sees any access past a row, a map or a list.
// CPU only: no kernel is launched.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer tools/sam_mask_compose_host_check.cpp sgv3d_amd/csrc/sam_decoder.hip \
//       sgv3d_amd/csrc/common.cpp -o sam_mask_compose_host_check && ASAN_OPTIONS=detect_leaks=0 ./sam_mask_compose_host_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/sgv3d_hip.h"

namespace {

uint32_t state = 20261020u;
float next() {
    state = state * 1664525u + 1013904223u;
    return (float)(state >> 8) / (float)(1 << 24) - 0.5f;
}

int preprocess(int side, int longest, int size) { return (int)(side * ((double)size / longest) + 0.5); }

}  // namespace

int main() {
    const int low = 24, size = 96, boxes = 5, frames = 3;
    const int sizes[4][2] = {{54, 96}, {27, 48}, {135, 240}, {37, 61}};
    const std::vector<int32_t> labels = {9, 2, 0, 5, 3}, frame_of_box = {0, 0, 0, 0, 2};
    unsigned long long sum = 0;
    for (const auto &hw : sizes) {
        const int h = hw[0], w = hw[1], longest = h > w ? h : w;
        const int pre_h = preprocess(h, longest, size), pre_w = preprocess(w, longest, size);
        std::vector<float> logits((size_t)boxes * low * low);
        for (auto &v : logits) v = 0.6f * next() - 1.0f;
        const int rect[5][4] = {{2, 8, 3, 12}, {5, 11, 8, 20}, {1, 6, 1, 6}, {1, 6, 1, 6}, {pre_h / 4 - 4, low, low - 6, low}};
        for (int b = 0; b < boxes; ++b)
            for (int y = rect[b][0] < 0 ? 0 : rect[b][0]; y < rect[b][1]; ++y)
                for (int x = rect[b][2]; x < rect[b][3]; ++x) logits[((size_t)b * low + y) * low + x] += 2.5f;
        std::vector<uint8_t> cls((size_t)frames * h * w, 77), mask((size_t)boxes * h * w, 77);
        std::vector<float> val((size_t)boxes * h * w, -7.f);
        int rc = sgv3d_sam_mask_compose_host(SGV3D_SAM_COMPOSE_CLASS, boxes, frames, low, size, pre_h, pre_w, h, w, logits.data(), labels.data(),
                                             frame_of_box.data(), cls.data());
        rc |= sgv3d_sam_mask_compose_host(SGV3D_SAM_COMPOSE_BOOL, boxes, frames, low, size, pre_h, pre_w, h, w, logits.data(), nullptr, nullptr, mask.data());
        rc |= sgv3d_sam_mask_compose_host(SGV3D_SAM_COMPOSE_LOGIT, boxes, frames, low, size, pre_h, pre_w, h, w, logits.data(), nullptr, nullptr, val.data());
        if (rc != 0) {
            std::printf("sgv3d_sam_mask_compose_host failed (%d): %s\n", rc, sgv3d_last_error());
            return 1;
        }
        const size_t px = (size_t)h * w;
        int top = 0;
        for (size_t i = 0; i < px; ++i) {
            // the paint loop over the per-box masks, by hand
            int want = 0;
            for (int b = 0; b < 4 && !want; ++b)
                if (mask[b * px + i] && labels[b]) want = labels[b] > 6 ? 6 : labels[b];
            if (cls[i] != want || cls[px + i] != 0 || cls[2 * px + i] != (mask[4 * px + i] ? 3 : 0)) return 2;
            for (int b = 0; b < boxes; ++b)
                if ((val[b * px + i] > 0.f) != (mask[b * px + i] != 0) && val[b * px + i] != 0.f) return 3;
            top = cls[i] > top ? cls[i] : top;
        }
        if (top != 6 || cls[3 * px - 1] != 3) return 4;
        for (auto v : cls) sum = sum * 31 + v;
        // no boxes at all: zeros, and no input is read
        std::vector<uint8_t> none((size_t)2 * h * w, 77);
        if (sgv3d_sam_mask_compose_host(SGV3D_SAM_COMPOSE_CLASS, 0, 2, low, size, pre_h, pre_w, h, w, nullptr, nullptr, nullptr, none.data()) != 0) return 5;
        for (auto v : none)
            if (v) return 6;
    }
    // bad calls are refused before anything is touched
    uint8_t one = 0;
    if (sgv3d_sam_mask_compose_host(7, 1, 1, low, size, 54, 96, 1, 1, nullptr, nullptr, nullptr, &one) != -1) return 7;
    if (sgv3d_sam_mask_compose_host(SGV3D_SAM_COMPOSE_BOOL, 1, 1, low, size, 97, 96, 1, 1, nullptr, nullptr, nullptr, &one) != -1) return 8;
    std::printf("checksum %llu\nOK\n", sum);
    return 0;
}
