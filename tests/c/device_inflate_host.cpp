// device_inflate_host.cpp -- TEST HARNESS.  The per-lane DEFLATE decoder of the device-side BLOW5 reader
// (sigfish_amd/csrc/blow5_kernels.hpp: inflate_zlib_lane, the body of blow5_inflate_kernel) compiled for the HOST, so that it can
// run under AddressSanitizer / UBSan (not available for GPU code on this pool) and against zlib on far more streams than a GPU
// test budget allows.  usage: device_inflate_host [iterations] [seed] [cases.bin]
// cases.bin (written by tests/deflate_craft.py, flat_file(): crafted streams, answers from zlib): u32 count, then per case
//   u32 kind (1: sound, decodes to `plain`; 0: refused; 2: sound for zlib, declined here by design -- bytes behind the stream),
//   u32 plain bytes, u32 stream bytes, plain, stream.
// Every record sits in a heap block of exactly its size plus the padding the device gives its input (random bytes: what lies behind a
// record there is the next record), every output in a heap block of exactly its slot: a byte beside either is a sanitizer report.
#define SFA_HOST_HARNESS
#include "../../sigfish_amd/csrc/blow5_kernels.hpp"

#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {
constexpr size_t kInPad = 128;  // ctx::Blow5::reserve_inflate: the device's input buffer ends 128 bytes behind the last record

// one stream through the lane decoder: input and output in exact-size heap blocks, decoder state as stale as the last record left it
int decode(const uint8_t *stream, size_t n, uint8_t *out, int64_t cap, sfa::InflateLds &S) {
    std::unique_ptr<uint8_t[]> in(new uint8_t[n + kInPad]);
    if (n) memcpy(in.get(), stream, n);
    for (size_t i = n; i < n + kInPad; ++i) in[i] = rand() & 255;
    return sfa::inflate_zlib_lane(in.get(), static_cast<int64_t>(n), out, cap, S);
}

// the crafted cases; returns the number of failures, -1 where the file cannot be read
int crafted(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        printf("cannot open %s\n", path);
        return -1;
    }
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return -1;
    int n_sound = 0, n_refused = 0, n_design = 0, bad = 0;
    sfa::InflateLds S;
    memset(&S, 0xa5, sizeof S);
    for (uint32_t k = 0; k < count; ++k) {
        uint32_t h[3];
        if (fread(h, 4, 3, f) != 3) return -1;
        std::vector<uint8_t> plain(h[1]), stream(h[2]);
        if (h[1] && fread(plain.data(), 1, h[1], f) != h[1]) return -1;
        if (h[2] && fread(stream.data(), 1, h[2], f) != h[2]) return -1;
        bool ok;
        int r;
        if (h[0]) {
            ++n_sound;
            std::unique_ptr<uint8_t[]> out(new uint8_t[h[1] ? h[1] : 1]);  // exactly what it needs: not a byte more may be written
            r = decode(stream.data(), stream.size(), out.get(), h[1], S);
            ok = r == static_cast<int>(h[1]) && (h[1] == 0 || memcmp(out.get(), plain.data(), h[1]) == 0);
            if (h[0] == 2) {  // zlib's bytes or declined
                n_design += r == -1;
                ok = ok || r == -1;
            }
            if (ok && h[1] > 0) {  // a slot one byte short declines
                std::unique_ptr<uint8_t[]> small(new uint8_t[h[1] - 1 ? h[1] - 1 : 1]);
                ok = decode(stream.data(), stream.size(), small.get(), h[1] - 1, S) == -1;
            }
        } else {  // room for anything a crafted text holds: refused for its own reason, not for a full slot
            ++n_refused;
            const int64_t cap = 1 << 17;
            std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
            r = decode(stream.data(), stream.size(), out.get(), cap, S);
            ok = r == -1;
        }
        if (!ok) {
            ++bad;
            printf("FAIL crafted case %u (%s): %u plain, %u stream bytes, got %d\n", k, h[0] ? "sound" : "refused", h[1], h[2], r);
        }
    }
    fclose(f);
    printf("crafted: %d sound, %d refused, %d failures\n", n_sound, n_refused, bad);
    printf("crafted: %d of the sound ones declined by design\n", n_design);
    return bad;
}
}  // namespace

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 4000;
    srand(argc > 2 ? atoi(argv[2]) : 1);
    int bad_crafted = 0;
    if (argc > 3 && (bad_crafted = crafted(argv[3])) < 0) return 2;
    srand(argc > 2 ? atoi(argv[2]) : 1);  // (the random campaign draws what it drew before there were crafted cases)
    int bad = 0;
    for (int it = 0; it < iters; ++it) {
        const int n = rand() % (it % 50 == 0 ? 120000 : 9000);
        std::vector<uint8_t> src(n + 1);
        const int kind = rand() % 5;
        for (int i = 0; i < n; ++i)
            src[i] = kind == 0 ? rand() & 255 : kind == 1 ? (rand() % 6) * (rand() % 40) : kind == 2 ? "the quick brown fox "[i % 20] : kind == 3 ? 0 : (i * 7 + (rand() % 3)) & 255;
        uLongf cl = compressBound(n) + n / 2 + 4096;  // (tiny memLevel / window settings expand beyond compressBound's estimate)
        std::vector<uint8_t> comp(cl + 256, 0);
        const int levels[4] = {0, 1, 6, 9};
        const int level = levels[rand() % 4];
        z_stream zs{};
        const int strategy = rand() % 4 == 0 ? Z_FIXED : Z_DEFAULT_STRATEGY;
        deflateInit2(&zs, level, Z_DEFLATED, 9 + rand() % 7, 1 + rand() % 9, strategy);
        zs.next_in = src.data();
        zs.avail_in = n;
        zs.next_out = comp.data();
        zs.avail_out = cl;
        if (deflate(&zs, Z_FINISH) != Z_STREAM_END) {
            printf("harness: deflate did not finish\n");
            return 2;
        }
        cl = zs.total_out;
        deflateEnd(&zs);
        for (size_t i = cl; i < comp.size(); ++i) comp[i] = rand() & 255;  // what lies behind a record on the device: anything
        std::vector<uint8_t> out(n + 64);
        sfa::InflateLds S;
        int r = sfa::inflate_zlib_lane(comp.data(), cl, out.data(), n + 16, S);
        bool ok = r == n && memcmp(out.data(), src.data(), n) == 0;
        // a slot that is too small must be refused, a corrupted stream must not be accepted as something else
        if (ok && n > 64) ok = sfa::inflate_zlib_lane(comp.data(), cl, out.data(), n - 1 - rand() % 32, S) == -1;
        if (ok && cl > 12) {
            std::vector<uint8_t> c2(comp);
            c2[2 + rand() % (cl - 6)] ^= 1 << (rand() % 8);
            std::vector<uint8_t> o2(n + 64), ref(n + 64);
            const int r2 = sfa::inflate_zlib_lane(c2.data(), cl, o2.data(), n + 16, S);
            uLongf rl = n + 16;
            const int zr = uncompress(ref.data(), &rl, c2.data(), cl);
            if (zr == Z_OK)
                ok = r2 == static_cast<int>(rl) && memcmp(o2.data(), ref.data(), rl) == 0;
            else  // zlib refuses: so must we -- unless the flipped bit sat where only zlib looks and the payload is intact (its
                  // Adler-32 still matches): accepting the original bytes is harmless
                ok = r2 == -1 || (r2 == n && memcmp(o2.data(), src.data(), n) == 0);
        }
        if (!ok) {
            if (++bad < 6) printf("FAIL it=%d n=%d kind=%d level=%d strategy=%d clen=%lu r=%d\n", it, n, kind, level, strategy, static_cast<unsigned long>(cl), r);
        }
    }
    printf("%d iterations, %d failures\n", iters, bad);
    return bad != 0 || bad_crafted != 0;
}
