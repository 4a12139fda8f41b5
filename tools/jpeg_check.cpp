// Stand-alone checker of the host JPEG code (csrc/jpeg_host.cpp), meant to be built with the host
// compiler and -fsanitize=address,undefined (tests/test_jpeg_host.py does):
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -DYXH_JPEG_STANDALONE -Iinclude -Ipixeltable-yolox_amd/csrc
//       tools/jpeg_check.cpp pixeltable-yolox_amd/csrc/jpeg_host.cpp -o jpeg_check
//   jpeg_check file.jpg ...
//
// Every file goes through probe, decode and the host render as it is (one "ok" / "rc" line each on
// stdout), then through a seeded set of truncations and byte flips of it.  Damaged input may be
// refused or decoded; what must hold is that every call returns, that the sanitizers stay silent
// and that the guard bytes around the coefficient buffer, the workspace and the destination
// survive.  Exit status 0 if so.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "yoloxhip.h"

namespace {

constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0xA5;
constexpr long long kMaxPixels = 1 << 22;  // a flipped size byte may ask for a huge image: not rendered

struct Guarded {
    std::vector<uint8_t> mem;
    size_t n;
    explicit Guarded(size_t bytes) : mem(bytes + 2 * kGuard + 16, kGuardByte), n(bytes) {}
    uint8_t* data() {  // 16-aligned payload behind the front guard
        uintptr_t p = (uintptr_t)mem.data() + kGuard;
        return (uint8_t*)((p + 15) & ~(uintptr_t)15);
    }
    bool intact() {
        const uint8_t* lo = data();
        for (const uint8_t* p = mem.data(); p < lo; ++p)
            if (*p != kGuardByte) return false;
        for (const uint8_t* p = lo + n; p < mem.data() + mem.size(); ++p)
            if (*p != kGuardByte) return false;
        return true;
    }
};

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {  // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// -> the decode's status (or the probe's, if that refused), -100 on a broken guard
int run(const uint8_t* bytes, size_t len, long long* checksum) {
    // the input itself in an exact-size heap block: a read past `len` is the sanitizer's to catch
    std::vector<uint8_t> in(bytes, bytes + len);
    yxh_jpeg_info info;
    memset(&info, 0, sizeof(info));
    int rc = yxh_jpeg_probe(in.data(), in.size(), &info);
    if (rc != YXH_OK) return rc;
    if ((long long)info.height * info.width > kMaxPixels) return YXH_EUNSUPPORTED;
    Guarded coef((size_t)info.coef_bytes);
    yxh_jpeg_image im;
    rc = yxh_jpeg_decode(in.data(), in.size(), (int16_t*)coef.data(), coef.n, &im);
    if (!coef.intact()) return -100;
    if (rc != YXH_OK) return rc;
    Guarded ws(yxh_jpeg_workspace_bytes(im.height, im.width, im.sampling));
    Guarded dst((size_t)im.height * im.width * 3);
    rc = yxh_jpeg_render_host((const int16_t*)coef.data(), &im, 1, ws.data(), dst.data());
    if (!coef.intact() || !ws.intact() || !dst.intact()) return -100;
    if (checksum) {
        long long s = 0;
        for (size_t i = 0; i < dst.n; ++i) s += dst.data()[i] * (long long)(i % 251 + 1);
        *checksum = s;
    }
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
        return 2;
    }
    int bad = 0;
    long long calls = 0, decoded = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
        fclose(f);
        long long sum = 0;
        const int rc = run(data.data(), data.size(), &sum);
        if (rc == YXH_OK) printf("ok %s %lld\n", argv[a], sum);
        else printf("rc %d %s (%s)\n", rc, argv[a], yxh_last_error());
        bad += rc == -100;
        // truncations: every prefix of a small file, 256 seeded lengths of a larger one
        const size_t len = data.size();
        const int ntrunc = len <= 2048 ? (int)len : 256;
        for (int t = 0; t < ntrunc; ++t) {
            const size_t cut = len <= 2048 ? (size_t)t : rnd() % len;
            const int r = run(data.data(), cut, nullptr);
            bad += r == -100;
            decoded += r == YXH_OK;
            ++calls;
        }
        // byte flips: one to four bytes replaced, anywhere (headers and scan alike)
        for (int t = 0; t < 400; ++t) {
            std::vector<uint8_t> m(data);
            const int k = 1 + (int)(rnd() % 4);
            for (int j = 0; j < k; ++j) m[rnd() % len] = (uint8_t)rnd();
            const int r = run(m.data(), m.size(), nullptr);
            bad += r == -100;
            decoded += r == YXH_OK;
            ++calls;
        }
    }
    printf("%lld damaged inputs, %lld of them decoded, %d guard failures\n", calls, decoded, bad);
    return bad ? 1 : 0;
}
