// zstd_lane_host.cpp -- TEST HARNESS.  The zstd frame decoder of the BLOW5 readers (sigfish_amd/csrc/zstd_lane.hpp: zstd_frame_lane,
// the host reader's decoder and the body of blow5_zstd_kernel) compiled for the HOST with its own main, so that it runs under
// AddressSanitizer / UBSan.  Every input, output and scratch area is a heap block of exactly its size: a byte read or written
// beside one is a report.
//   usage: zstd_lane_host <frames.bin> [iterations] [seed]
// frames.bin (written by tests/test_zstd_cpu.py from tests/golden/zstd/frames.npz): u32 count, then per frame
//   u32 sound (1: decodes to `plain`; 0: malformed), u32 plain bytes, u32 frame bytes, plain, frame.
// Sound frames must decode byte-exact; malformed ones must give -1 or (where no checksum can tell) a length within the slot.
// Where libzstd.so.1 opens, `iterations` random streams of the five kinds of device_inflate_host.cpp follow, each one also
// truncated and with flipped bytes.  Exit status: the number of mismatches (at most 255).
#define SFA_HOST_HARNESS
#include "../../sigfish_amd/csrc/zstd_lane.hpp"

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {
// exact-size heap blocks (a std::vector's capacity may exceed its size, which would hide an overrun from ASan)
struct Block {
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Block(size_t bytes) : p(new uint8_t[bytes ? bytes : 1]), n(bytes) {}
    uint8_t *data() { return p.get(); }
};

int decode(const uint8_t *frame, size_t n, uint8_t *out, int64_t cap) {
    Block in(n), scratch(static_cast<size_t>(sfa::zstd_scratch_bytes(cap)));
    if (n) memcpy(in.data(), frame, n);
    return sfa::zstd_frame_lane(in.data(), static_cast<int64_t>(n), out, cap, scratch.data());
}

typedef size_t (*bound_fn)(size_t);
typedef void *(*create_fn)();
typedef size_t (*free_fn)(void *);
typedef size_t (*setp_fn)(void *, int, int);
typedef size_t (*comp2_fn)(void *, void *, size_t, const void *, size_t);
typedef unsigned (*iserr_fn)(size_t);
typedef size_t (*decomp_fn)(void *, size_t, const void *, size_t);
}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("usage: zstd_lane_host <frames.bin> [iterations] [seed]\n");
        return 255;
    }
    const int iters = argc > 2 ? atoi(argv[2]) : 2000;
    srand(argc > 3 ? atoi(argv[3]) : 1);
    int bad = 0;
    // ---- the fixture frames ----
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f) {
            printf("cannot open %s\n", argv[1]);
            return 255;
        }
        uint32_t count = 0;
        if (fread(&count, 4, 1, f) != 1) return 255;
        int n_sound = 0, n_bad = 0;
        for (uint32_t k = 0; k < count; ++k) {
            uint32_t h[3];
            if (fread(h, 4, 3, f) != 3) return 255;
            std::vector<uint8_t> plain(h[1]), frame(h[2]);
            if (h[1] && fread(plain.data(), 1, h[1], f) != h[1]) return 255;
            if (h[2] && fread(frame.data(), 1, h[2], f) != h[2]) return 255;
            if (h[0]) {
                ++n_sound;
                Block out(h[1]);  // exactly what it needs: not a byte more may be written
                const int r = decode(frame.data(), frame.size(), out.data(), h[1]);
                bool ok = r == static_cast<int>(h[1]) && (h[1] == 0 || memcmp(out.data(), plain.data(), h[1]) == 0);
                if (ok && h[1] > 0) {  // a slot one byte short declines
                    Block small(h[1] - 1);
                    ok = decode(frame.data(), frame.size(), small.data(), h[1] - 1) == -1;
                }
                if (!ok) {
                    ++bad;
                    printf("FAIL fixture %u (sound): %u plain, %u frame bytes, got %d\n", k, h[1], h[2], r);
                }
            } else {
                ++n_bad;
                const int64_t cap = 4 * static_cast<int64_t>(h[2]) + 4096;
                Block out(static_cast<size_t>(cap));
                const int r = decode(frame.data(), frame.size(), out.data(), cap);
                if (!(r == -1 || (r >= 0 && r <= cap))) {
                    ++bad;
                    printf("FAIL fixture %u (malformed): got %d\n", k, r);
                }
                printf("malformed fixture %u: %d\n", k, r);
            }
        }
        fclose(f);
        printf("fixtures: %d sound, %d malformed, %d failures\n", n_sound, n_bad, bad);
    }
    // ---- random campaign against libzstd ----
    void *lib = dlopen("libzstd.so.1", RTLD_NOW);
    if (!lib) {
        printf("libzstd.so.1 does not open: random campaign skipped\n");
        return bad > 255 ? 255 : bad;
    }
    const bound_fn z_bound = reinterpret_cast<bound_fn>(dlsym(lib, "ZSTD_compressBound"));
    const create_fn z_create = reinterpret_cast<create_fn>(dlsym(lib, "ZSTD_createCCtx"));
    const free_fn z_free = reinterpret_cast<free_fn>(dlsym(lib, "ZSTD_freeCCtx"));
    const setp_fn z_set = reinterpret_cast<setp_fn>(dlsym(lib, "ZSTD_CCtx_setParameter"));
    const comp2_fn z_comp = reinterpret_cast<comp2_fn>(dlsym(lib, "ZSTD_compress2"));
    const iserr_fn z_iserr = reinterpret_cast<iserr_fn>(dlsym(lib, "ZSTD_isError"));
    const decomp_fn z_decomp = reinterpret_cast<decomp_fn>(dlsym(lib, "ZSTD_decompress"));
    if (!z_bound || !z_create || !z_free || !z_set || !z_comp || !z_iserr || !z_decomp) {
        printf("libzstd.so.1 lacks a symbol: random campaign skipped\n");
        return bad > 255 ? 255 : bad;
    }
    void *cctx = z_create();
    int lenient = 0;
    for (int it = 0; it < iters; ++it) {
        const int n = rand() % (it % 50 == 0 ? 300001 : 9000);
        std::vector<uint8_t> src(n + 1);
        const int kind = rand() % 5;
        for (int i = 0; i < n; ++i)
            src[i] = kind == 0 ? rand() & 255 : kind == 1 ? (rand() % 6) * (rand() % 40) : kind == 2 ? "the quick brown fox "[i % 20] : kind == 3 ? 0 : (i * 7 + (rand() % 3)) & 255;
        const int levels[4] = {1, 3, 9, 19};
        const int level = levels[rand() % 4], checksum = rand() & 1;
        z_set(cctx, 100 /* ZSTD_c_compressionLevel */, level);
        z_set(cctx, 201 /* ZSTD_c_checksumFlag */, checksum);
        std::vector<uint8_t> comp(z_bound(n));
        const size_t cl = z_comp(cctx, comp.data(), comp.size(), src.data(), n);
        if (z_iserr(cl)) {
            printf("harness: ZSTD_compress2 failed\n");
            return 255;
        }
        Block out(n);
        const int r = decode(comp.data(), cl, out.data(), n);
        bool ok = r == n && (n == 0 || memcmp(out.data(), src.data(), n) == 0);
        if (ok && n > 64) {  // a slot that is too small must be refused
            const int cap = n - 1 - rand() % 32;
            Block small(cap);
            ok = decode(comp.data(), cl, small.data(), cap) == -1;
        }
        // the same stream truncated, and with flipped bytes: declined, or -- where libzstd takes it too -- the same bytes
        for (int variant = 0; ok && variant < 2 && cl > 1; ++variant) {
            std::vector<uint8_t> c2(comp.begin(), comp.begin() + cl);
            if (variant == 0) {
                c2.resize(rand() % cl);
            } else {
                const int flips = 1 + rand() % 3;
                for (int k = 0; k < flips; ++k) c2[rand() % cl] ^= 1 << (rand() % 8);
            }
            const int cap = n + 16;
            Block o2(cap), ref(cap);
            const int r2 = decode(c2.data(), c2.size(), o2.data(), cap);
            const size_t zr = z_decomp(ref.data(), cap, c2.data(), c2.size());
            if (r2 < -1 || r2 > cap)
                ok = false;
            else if (r2 >= 0 && !z_iserr(zr) && c2.size() > 0)
                ok = static_cast<size_t>(r2) == zr && (zr == 0 || memcmp(o2.data(), ref.data(), zr) == 0);
            else if (r2 >= 0 && c2.size() > 0)
                ++lenient;  // (taken here, refused there: counted, looked at by hand; no checksum on such a stream can tell)
            if (!ok) printf("variant %d: ours %d, libzstd %s %zu\n", variant, r2, z_iserr(zr) ? "error" : "ok", zr);
        }
        if (!ok && ++bad < 8) printf("FAIL it=%d n=%d kind=%d level=%d checksum=%d clen=%zu r=%d\n", it, n, kind, level, checksum, cl, r);
    }
    z_free(cctx);
    printf("%d iterations, %d failures, %d corrupted streams taken that libzstd refuses\n", iters, bad, lenient);
    return bad > 255 ? 255 : bad;
}
