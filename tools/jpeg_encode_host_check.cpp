// Stand-alone sanitizer program for the host entry of the JPEG encoder (sgv3d_jpeg_encode_host, csrc/jpeg_encode.hip) and
// for sgv3d_jpeg_encode_header: the sizes of tests/golden/jpeg_encode.npz (1x1 .. 168x328) at the three samplings, five
// qualities and restart intervals 0, 1, 3 and one MCU row, on noise, a ramp and a checkerboard, in batches of two.  The
// frames, the files, the lengths, the status words and the header live in their own exactly sized heap blocks, the files
// block as small as the entry takes (frames * roundup16(max_bytes), with max_bytes the length the first pass found), so
// that AddressSanitizer sees any access past a frame, a file or a word.  Every file is checked for its markers; a second
// pass one byte short must flag the longer frame and leave the other.  CPU only: no kernel is launched.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-omit-frame-pointer tools/jpeg_encode_host_check.cpp sgv3d_amd/csrc/jpeg_encode.hip \
//       sgv3d_amd/csrc/common.cpp -o jpeg_encode_host_check && ASAN_OPTIONS=detect_leaks=0 ./jpeg_encode_host_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../include/sgv3d_hip.h"

namespace {

uint32_t state = 20261019u;
uint32_t next() {
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

long long up16(long long n) { return (n + 15) / 16 * 16; }

int fail(const char *what, int h, int w, int q, int hs, int vs, int r) {
    std::printf("%s at %dx%d quality %d sampling %dx%d restart %d: %s\n", what, h, w, q, hs, vs, r, sgv3d_last_error());
    return 1;
}

// SOI, the header, EOI, and no marker inside the scan but RSTn in order
bool well_formed(const uint8_t *f, int len, const uint8_t *hdr, int hdr_len, int restart) {
    if (len < hdr_len + 3 || std::memcmp(f, hdr, hdr_len) != 0 || f[len - 2] != 0xFF || f[len - 1] != 0xD9) return false;
    int rst = 0;
    for (int i = hdr_len; i < len - 2; ++i) {
        if (f[i] != 0xFF) continue;
        const int m = f[++i];
        if (m == 0) continue;
        if (!restart || m != 0xD0 + (rst++ & 7)) return false;
    }
    return true;
}

}  // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {8, 8}, {9, 7}, {16, 16}, {17, 33}, {24, 40}, {24, 48}, {40, 24}, {37, 61}, {41, 65}, {130, 260}, {168, 328}};
    const int samplings[][2] = {{1, 1}, {2, 1}, {2, 2}}, qualities[] = {10, 30, 75, 95, 100};
    int calls = 0;
    long long bytes = 0;
    for (const auto &hw : sizes)
        for (const auto &s : samplings)
            for (int ri = 0; ri < 4; ++ri) {
                const int h = hw[0], w = hw[1], hs = s[0], vs = s[1], n = 2;
                const int mcux = (w + 8 * hs - 1) / (8 * hs);
                const int restart = ri == 0 ? 0 : (ri == 1 ? 1 : (ri == 2 ? 3 : mcux));
                const int q = qualities[(calls + ri) % 5];
                const size_t frame = (size_t)h * w * 3;
                std::unique_ptr<uint8_t[]> src(new uint8_t[n * frame]);
                for (size_t i = 0; i < frame; ++i) src[i] = (uint8_t)next();                       // noise
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x)
                        for (int c = 0; c < 3; ++c)
                            src[frame + ((size_t)y * w + x) * 3 + c] = (calls & 1) ? (uint8_t)(((x + y) & 1) * 255) : (uint8_t)(2 * y + x + 40 * c);
                std::unique_ptr<uint8_t[]> hdr(new uint8_t[SGV3D_JPEG_ENC_HEADER_MAX]);
                std::unique_ptr<uint16_t[]> quant(new uint16_t[128]);
                int hdr_len = 0;
                if (sgv3d_jpeg_encode_header(h, w, q, hs, vs, restart, hdr.get(), &hdr_len, quant.get()) != 0 ||
                    hdr_len != (restart ? 629 : 623))
                    return fail("sgv3d_jpeg_encode_header", h, w, q, hs, vs, restart);
                std::unique_ptr<int32_t[]> len(new int32_t[n]), status(new int32_t[n]);
                // pass 1: room to spare
                int max_bytes = (int)frame * 3 + 4096;
                {
                    std::unique_ptr<uint8_t[]> files(new uint8_t[n * up16(max_bytes)]);
                    if (sgv3d_jpeg_encode_host(n, h, w, q, hs, vs, restart, max_bytes, src.get(), files.get(), n * up16(max_bytes), len.get(),
                                               status.get()) != 0 || status[0] || status[1])
                        return fail("sgv3d_jpeg_encode_host", h, w, q, hs, vs, restart);
                    if (!well_formed(files.get(), len[0], hdr.get(), hdr_len, restart) ||
                        !well_formed(files.get() + up16(len[0]), len[1], hdr.get(), hdr_len, restart))
                        return fail("a malformed file", h, w, q, hs, vs, restart);
                }
                const int l0 = len[0], l1 = len[1], longest = l0 > l1 ? l0 : l1;
                bytes += l0 + l1;
                // pass 2: exactly enough, in a block of exactly the size the entry asks for
                {
                    max_bytes = longest;
                    std::unique_ptr<uint8_t[]> files(new uint8_t[n * up16(max_bytes)]);
                    if (sgv3d_jpeg_encode_host(n, h, w, q, hs, vs, restart, max_bytes, src.get(), files.get(), n * up16(max_bytes), len.get(),
                                               status.get()) != 0 || status[0] || status[1] || len[0] != l0 || len[1] != l1)
                        return fail("the exact fit", h, w, q, hs, vs, restart);
                }
                // pass 3: one byte short of the longer file
                if (l0 != l1) {
                    max_bytes = longest - 1;
                    std::unique_ptr<uint8_t[]> files(new uint8_t[n * up16(max_bytes)]);
                    if (sgv3d_jpeg_encode_host(n, h, w, q, hs, vs, restart, max_bytes, src.get(), files.get(), n * up16(max_bytes), len.get(),
                                               status.get()) != 0)
                        return fail("the short fit", h, w, q, hs, vs, restart);
                    const int big = l0 > l1 ? 0 : 1;
                    if (status[big] != SGV3D_JPEG_ENC_EOVERFLOW || len[big] != 0 || status[1 - big] != 0 || len[1 - big] != (big ? l0 : l1) ||
                        !well_formed(files.get(), len[1 - big], hdr.get(), hdr_len, restart))
                        return fail("the overflow", h, w, q, hs, vs, restart);
                }
                ++calls;
            }
    // bad calls are refused before anything is touched
    uint8_t one[3] = {1, 2, 3}, out[16];
    int32_t l = -7, st = -7;
    if (sgv3d_jpeg_encode_host(1, 1, 1, 0, 2, 2, 0, 16, one, out, 16, &l, &st) != -1) return 2;
    if (sgv3d_jpeg_encode_host(1, 1, 1, 95, 2, 2, 0, 16, one, out, 15, &l, &st) != -1 || l != -7 || st != -7) return 3;
    std::printf("%d settings, %lld bytes of files\nOK\n", calls, bytes);
    return 0;
}
