// zstd_lane.hpp -- a Zstandard frame decoder written from the format (RFC 8878), ONE TEXT for the host reader (host/blow5.cpp) and
// for the device (blow5_zstd_kernel, sfa_zstd.hip), as blow5_kernels.hpp's inflate_zlib_lane is: plain C++ behind
// __device__ __forceinline__ (ZS_DEV ZS_INL below), a serial decoder per record.  No libzstd anywhere.
//
// What it takes: one or more frames back to back, skippable frames; single-segment headers and window descriptors; a content
// size of 0, 1, 2, 4, 8 bytes (checked against what was produced); the content checksum (XXH64, low 32 bits); a dictionary id
// field that says 0.  Raw, RLE and compressed blocks.  Raw, RLE, Huffman (1 and 4 streams, weights direct or FSE-compressed,
// codes up to 11 bits) and treeless literals.  Sequences with predefined, RLE, FSE-compressed and repeat tables, the three
// repeat offsets carried from block to block, matches that overlap their own output.  What it declines (-1): a dictionary,
// a reserved block type, a block beyond the block maximum, a match that reaches in front of the frame's first byte, any
// table beyond its accuracy limit (LL/ML 9, OF 8, weights 6), any read beyond in_bytes, any write beyond out_cap.
//
// Bounds: every input byte is read through a checked index or through zs_window(), which loads only inside [p, p + n); every
// output byte is written behind a comparison with out_cap; every table index is masked by, or compared with, the size the
// table was built for; the scratch is addressed with the constants below only.
#pragma once

// SFA_HOST_HARNESS: host code (host/blow5.cpp, whichever compiler and language mode builds it, and tests/c/zstd_lane_host.cpp
// under sanitizers); otherwise device code.  The decoder below says ZS_DEV ZS_INL where blow5_kernels.hpp says
// __device__ __forceinline__: a HIP compilation of a host unit has __device__ defined already and must not get it here.
#if defined(SFA_HOST_HARNESS) || !defined(__HIPCC__)
#include <string.h>
#define ZS_DEV
#define ZS_INL inline
#else
#include <hip/hip_runtime.h>
#define ZS_DEV __device__
#define ZS_INL __forceinline__
#endif
#include <stdint.h>

namespace sfa {

constexpr int kZstdBlockMax = 128 * 1024;  // Block_Maximum_Size of the format, and so the most literals a block can hold
constexpr int kZstdHufLog = 11;
// scratch of one decoder: the tables at fixed places, the Huffman-coded literals of the current block behind them
constexpr int kZsHuf = 0;         // uint16_t[1 << 11]  (symbol << 8) | code length, indexed by the next 11 bits
constexpr int kZsLL = 4096;       // ZstdFse[1 << 9]    literal lengths
constexpr int kZsML = 6144;       // ZstdFse[1 << 9]    match lengths
constexpr int kZsOF = 8192;       // ZstdFse[1 << 8]    offset codes
constexpr int kZsWFse = 9216;     // ZstdFse[1 << 6]    the table the Huffman weights are compressed with
constexpr int kZsWeights = 9472;  // uint8_t[256]       Huffman weights
constexpr int kZsNorm = 9728;     // int16_t[64]        normalised counts of the table being built
constexpr int kZsNext = 9856;     // uint16_t[64]       next state of every symbol (table building), rank counts (Huffman)
constexpr int kZstdTableBytes = 9984;
// bytes a caller provides for a record whose output slot holds out_cap bytes: a block's literals are at most the block, and a
// block that holds more than the slot does not fit the slot
constexpr int64_t zstd_scratch_bytes(int64_t out_cap) {
    return kZstdTableBytes + (out_cap < kZstdBlockMax ? (out_cap < 0 ? 0 : out_cap) : kZstdBlockMax);
}

struct ZstdFse {
    uint16_t base;
    uint8_t sym, nbits;
};

ZS_DEV const int8_t kZstdLLDefault[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
ZS_DEV const int8_t kZstdMLDefault[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                              1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
ZS_DEV const int8_t kZstdOFDefault[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
ZS_DEV const uint32_t kZstdLLBase[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,   10,  11,  12,   13,   14,   15,   16,    18,
                                             20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
ZS_DEV const uint8_t kZstdLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
ZS_DEV const uint32_t kZstdMLBase[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18,  19,  20,  21,   22,   23,   24,   25,    26,    27,   28, 29,
                                             30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
ZS_DEV const uint8_t kZstdMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                            0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

ZS_DEV ZS_INL int zs_highbit(uint32_t x) { return 31 - __builtin_clz(x); }  // x != 0

// The 64 bits of a backward bit stream below bit position `pos` (bits [pos - 64, pos) of the bytes at p, bit 0 = lowest bit of
// p[0]), the next bit to read on top; bits in front of the stream read as 0.  Loads only bytes of [p, p + ceil(pos / 8)).
// At least 57 of the 64 bits are meaningful.
ZS_DEV ZS_INL uint64_t zs_window(const uint8_t *p, int64_t pos) {
    if (pos <= 0) return 0;
    const int64_t e = (pos + 7) >> 3;
    uint64_t w;
    if (e >= 8) {
        __builtin_memcpy(&w, p + e - 8, 8);
    } else {
        w = 0;
        for (int64_t i = 0; i < e; ++i) w |= static_cast<uint64_t>(p[i]) << (8 * (8 - e + i));
    }
    return w << (e * 8 - pos);
}

struct ZsBack {  // a backward bit stream: `pos` bits are left; below 0 the stream is exhausted (zeros are read, the caller checks)
    const uint8_t *p;
    int64_t pos;
    // starts behind the padding: the highest set bit of the last byte marks the end
    ZS_DEV ZS_INL bool init(const uint8_t *b, int64_t n) {
        p = b;
        pos = 0;
        if (n < 1 || b[n - 1] == 0) return false;
        pos = (n - 1) * 8 + zs_highbit(b[n - 1]);
        return true;
    }
    ZS_DEV ZS_INL uint32_t read(int k) {  // k <= 32
        if (k == 0) return 0;
        const uint32_t v = static_cast<uint32_t>(zs_window(p, pos) >> (64 - k));
        pos -= k;
        return v;
    }
};

// FSE table description (RFC 8878 4.1.1): the normalised counts of up to max_sym + 1 symbols, read forward from p[0 .. n).
// Returns the bytes it took or -1.
ZS_DEV inline int zs_read_ncount(const uint8_t *p, int64_t n, int max_log, int max_sym, int16_t *norm, int *n_sym, int *log_out) {
    int64_t bit = 0;
    const int64_t nbits_in = n * 8;
    auto get = [&](int k) -> uint32_t {  // k <= 17; bytes behind the input read as 0, the total is checked at the end
        uint32_t v = 0;
        const int64_t b = bit >> 3;
        for (int j = 0; j < 4; ++j)
            if (b + j < n) v |= static_cast<uint32_t>(p[b + j]) << (8 * j);
        v = (v >> (bit & 7)) & ((1u << k) - 1u);
        bit += k;
        return v;
    };
    const int log = static_cast<int>(get(4)) + 5;
    if (log > max_log) return -1;
    int remaining = 1 << log, s = 0;
    while (remaining > 0 && s <= max_sym) {
        if (bit > nbits_in) return -1;
        const int nb = zs_highbit(static_cast<uint32_t>(remaining + 1)) + 1;
        uint32_t val = get(nb);
        const uint32_t lower = (1u << (nb - 1)) - 1u;
        const uint32_t threshold = (1u << nb) - 1u - static_cast<uint32_t>(remaining + 1);
        if ((val & lower) < threshold) {
            bit -= 1;
            val &= lower;
        } else if (val > lower) {
            val -= threshold;
        }
        const int proba = static_cast<int>(val) - 1;
        remaining -= proba < 0 ? 1 : proba;
        norm[s++] = static_cast<int16_t>(proba);
        if (proba == 0) {
            uint32_t rep = get(2);
            for (;;) {
                if (bit > nbits_in) return -1;
                for (uint32_t i = 0; i < rep; ++i) {
                    if (s > max_sym) return -1;
                    norm[s++] = 0;
                }
                if (rep != 3) break;
                rep = get(2);
            }
        }
    }
    if (remaining != 0 || bit > nbits_in) return -1;
    *n_sym = s;
    *log_out = log;
    return static_cast<int>((bit + 7) >> 3);
}

// decoding table from normalised counts (4.1.1): `next` is work space of n_sym entries
ZS_DEV inline bool zs_fse_build(const int16_t *norm, int n_sym, int log, ZstdFse *t, uint16_t *next) {
    const int size = 1 << log;
    int high = size;
    for (int s = 0; s < n_sym; ++s)
        if (norm[s] == -1) {
            if (high == 0) return false;
            t[--high].sym = static_cast<uint8_t>(s);
            next[s] = 1;
        }
    const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    int pos = 0, filled = 0;
    for (int s = 0; s < n_sym; ++s) {
        if (norm[s] <= 0) continue;
        next[s] = static_cast<uint16_t>(norm[s]);
        for (int i = 0; i < norm[s]; ++i) {
            if (filled++ >= high) return false;  // (more cells announced than the table has left; so high > 0 below)
            t[pos].sym = static_cast<uint8_t>(s);
            do pos = (pos + step) & mask;  // (step is odd: every cell comes by, cell 0 < high among them)
            while (pos >= high);
        }
    }
    if (pos != 0 || filled != high) return false;
    for (int i = 0; i < size; ++i) {
        const int s = t[i].sym;
        if (s >= n_sym) return false;
        const uint32_t nx = next[s]++;
        if (nx == 0 || nx >= 2u * static_cast<uint32_t>(size)) return false;
        const int nb = log - zs_highbit(nx);
        if (nb < 0) return false;
        t[i].nbits = static_cast<uint8_t>(nb);
        t[i].base = static_cast<uint16_t>((nx << nb) - static_cast<uint32_t>(size));
    }
    return true;
}

// XXH64 with seed 0 (the content checksum is its low 32 bits)
ZS_DEV ZS_INL uint64_t zs_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
ZS_DEV ZS_INL uint64_t zs_rd64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
ZS_DEV inline uint64_t zs_xxh64(const uint8_t *p, int64_t len) {
    const uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull, P5 = 0x27D4EB2F165667C5ull;
    const uint8_t *const end = p + len;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
        for (; end - p >= 32; p += 32) {
            v1 = zs_rotl(v1 + zs_rd64(p) * P2, 31) * P1;
            v2 = zs_rotl(v2 + zs_rd64(p + 8) * P2, 31) * P1;
            v3 = zs_rotl(v3 + zs_rd64(p + 16) * P2, 31) * P1;
            v4 = zs_rotl(v4 + zs_rd64(p + 24) * P2, 31) * P1;
        }
        h = zs_rotl(v1, 1) + zs_rotl(v2, 7) + zs_rotl(v3, 12) + zs_rotl(v4, 18);
        h = (h ^ (zs_rotl(v1 * P2, 31) * P1)) * P1 + P4;
        h = (h ^ (zs_rotl(v2 * P2, 31) * P1)) * P1 + P4;
        h = (h ^ (zs_rotl(v3 * P2, 31) * P1)) * P1 + P4;
        h = (h ^ (zs_rotl(v4 * P2, 31) * P1)) * P1 + P4;
    } else {
        h = P5;
    }
    h += static_cast<uint64_t>(len);
    for (; end - p >= 8; p += 8) h = zs_rotl(h ^ (zs_rotl(zs_rd64(p) * P2, 31) * P1), 27) * P1 + P4;
    if (end - p >= 4) {
        uint32_t v;
        __builtin_memcpy(&v, p, 4);
        h = zs_rotl(h ^ (v * P1), 23) * P2 + P3;
        p += 4;
    }
    for (; p < end; ++p) h = zs_rotl(h ^ (*p * P5), 11) * P1;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    return h;
}

// what a frame's blocks hand on to each other
struct ZstdState {
    int huf_log;                 // 0: no Huffman table yet (a treeless block has nothing to reuse)
    int ll_log, of_log, ml_log;  // -1: no table yet (repeat mode has nothing to repeat)
    uint32_t rep[3];
};

// Huffman tree description (4.2.1) at p[0 .. n) -> the decoding table; returns the bytes it took or -1
ZS_DEV inline int zs_read_huf(const uint8_t *p, int64_t n, uint8_t *tables, ZstdState &st) {
    uint8_t *weights = tables + kZsWeights;
    uint16_t *huf = reinterpret_cast<uint16_t *>(tables + kZsHuf);
    uint16_t *rank = reinterpret_cast<uint16_t *>(tables + kZsNext);  // [0..16) codes per length, [16..32) next cell per length
    st.huf_log = 0;
    if (n < 1) return -1;
    const int hb = p[0];
    int n_w = 0, took;
    if (hb >= 128) {  // weights given directly, four bits each
        n_w = hb - 127;
        took = 1 + (n_w + 1) / 2;
        if (took > n) return -1;
        for (int i = 0; i < n_w; ++i) weights[i] = (i & 1) ? (p[1 + i / 2] & 15) : (p[1 + i / 2] >> 4);
    } else {  // FSE-compressed, two interleaved states
        took = 1 + hb;
        if (hb < 1 || took > n) return -1;
        int16_t *norm = reinterpret_cast<int16_t *>(tables + kZsNorm);
        ZstdFse *wt = reinterpret_cast<ZstdFse *>(tables + kZsWFse);
        int n_sym, log;
        const int hd = zs_read_ncount(p + 1, hb, 6, 12, norm, &n_sym, &log);
        if (hd < 0 || hd >= hb) return -1;
        if (!zs_fse_build(norm, n_sym, log, wt, rank)) return -1;
        ZsBack br;
        if (!br.init(p + 1 + hd, hb - hd)) return -1;
        const uint32_t mask = (1u << log) - 1u;
        uint32_t s1 = br.read(log) & mask, s2 = br.read(log) & mask;
        if (br.pos < 0) return -1;
        for (;;) {
            if (n_w > 253) return -1;
            weights[n_w++] = wt[s1].sym;
            s1 = (wt[s1].base + br.read(wt[s1].nbits)) & mask;
            if (br.pos < 0) {
                weights[n_w++] = wt[s2].sym;
                break;
            }
            weights[n_w++] = wt[s2].sym;
            s2 = (wt[s2].base + br.read(wt[s2].nbits)) & mask;
            if (br.pos < 0) {
                weights[n_w++] = wt[s1].sym;
                break;
            }
        }
    }
    // the last weight follows from the others: together they fill a power of two
    uint32_t sum = 0;
    for (int i = 0; i < n_w; ++i) {
        if (weights[i] > kZstdHufLog) return -1;
        if (weights[i]) sum += 1u << (weights[i] - 1);
    }
    if (sum == 0) return -1;
    const int log = zs_highbit(sum) + 1;
    if (log > kZstdHufLog) return -1;
    const uint32_t left = (1u << log) - sum;
    if (left & (left - 1)) return -1;  // not a power of two
    weights[n_w++] = static_cast<uint8_t>(zs_highbit(left) + 1);
    for (int l = 0; l < 32; ++l) rank[l] = 0;
    for (int i = 0; i < n_w; ++i) rank[weights[i]]++;  // (by weight: code length = log + 1 - weight)
    // cells: weight 1 (the longest codes) first, from cell 0; a code of weight w covers 1 << (w - 1) cells
    uint32_t at = 0;
    for (int w = 1; w <= log; ++w) {
        rank[16 + w] = static_cast<uint16_t>(at);
        at += static_cast<uint32_t>(rank[w]) << (w - 1);
    }
    if (at != (1u << log)) return -1;
    for (int s = 0; s < n_w; ++s) {
        const int w = weights[s];
        if (!w) continue;
        const uint32_t len = 1u << (w - 1), c = rank[16 + w];
        if (c + len > (1u << log)) return -1;
        const uint16_t e = static_cast<uint16_t>((s << 8) | (log + 1 - w));
        for (uint32_t i = 0; i < len; ++i) huf[c + i] = e;
        rank[16 + w] = static_cast<uint16_t>(c + len);
    }
    st.huf_log = log;
    return took;
}

// one Huffman stream p[0 .. n) -> exactly cnt symbols; the stream must end with the last symbol
ZS_DEV inline bool zs_huf_stream(const uint8_t *p, int64_t n, const uint16_t *huf, int log, uint8_t *dst, int64_t cnt) {
    ZsBack br;
    if (!br.init(p, n)) return false;
    int64_t i = 0;
    while (i < cnt) {
        const uint64_t w = zs_window(p, br.pos);
        int used = 0;
        do {  // up to five symbols from one window (57 meaningful bits, codes of at most 11)
            const uint32_t e = huf[static_cast<uint32_t>((w << used) >> (64 - log))];
            dst[i++] = static_cast<uint8_t>(e >> 8);
            used += e & 15u;
        } while (i < cnt && used <= 57 - kZstdHufLog);
        br.pos -= used;
        if (br.pos < 0) return false;
    }
    return br.pos == 0;
}

// the table of one of LL / OF / ML for this block, by its mode; p advances behind what was read
ZS_DEV inline bool zs_seq_table(int mode, const uint8_t *&p, const uint8_t *end, int max_log, int max_sym, const int8_t *dflt, int dflt_n, int dflt_log,
                                    ZstdFse *t, int *log, uint8_t *tables) {
    int16_t *norm = reinterpret_cast<int16_t *>(tables + kZsNorm);
    uint16_t *next = reinterpret_cast<uint16_t *>(tables + kZsNext);
    if (mode == 0) {  // predefined
        for (int s = 0; s < dflt_n; ++s) norm[s] = dflt[s];
        *log = dflt_log;
        return zs_fse_build(norm, dflt_n, dflt_log, t, next);
    }
    if (mode == 1) {  // RLE: one symbol, no bits
        if (p >= end || *p > max_sym) return false;
        t[0].sym = *p++;
        t[0].nbits = 0;
        t[0].base = 0;
        *log = 0;
        return true;
    }
    if (mode == 2) {
        int n_sym, lg;
        *log = -1;
        const int took = zs_read_ncount(p, end - p, max_log, max_sym, norm, &n_sym, &lg);
        if (took < 0) return false;
        p += took;
        if (!zs_fse_build(norm, n_sym, lg, t, next)) return false;
        *log = lg;
        return true;
    }
    return *log >= 0;  // repeat: the table of the block before
}

// one compressed block b[0 .. n) -> out[op ...); returns the new op or -1.  `first`: where the frame's output starts
ZS_DEV inline int64_t zs_block(const uint8_t *b, int64_t n, uint8_t *out, int64_t op, int64_t first, int64_t cap, uint8_t *tables, uint8_t *lit_buf,
                                   int64_t lit_cap, ZstdState &st) {
    // ---- literals section (3.1.1.3.1) ----
    if (n < 1) return -1;
    const int ltype = b[0] & 3, sf = (b[0] >> 2) & 3;
    const uint8_t *lit;   // the block's literals: in the input (raw), one byte of it (RLE), or decoded into lit_buf
    int64_t n_lit, hdr;
    bool lit_rle = false;
    if (ltype < 2) {
        if (sf == 0 || sf == 2) {
            hdr = 1;
            n_lit = b[0] >> 3;
        } else if (sf == 1) {
            if (n < 2) return -1;
            hdr = 2;
            n_lit = (b[0] >> 4) | (static_cast<int64_t>(b[1]) << 4);
        } else {
            if (n < 3) return -1;
            hdr = 3;
            n_lit = (b[0] >> 4) | (static_cast<int64_t>(b[1]) << 4) | (static_cast<int64_t>(b[2]) << 12);
        }
        if (n_lit > kZstdBlockMax) return -1;
        if (ltype == 0) {
            if (hdr + n_lit > n) return -1;
            lit = b + hdr;
            hdr += n_lit;
        } else {
            if (hdr + 1 > n) return -1;
            lit = b + hdr;
            lit_rle = true;
            hdr += 1;
        }
    } else {
        const int hb = sf < 2 ? 3 : sf + 2, sb = sf < 2 ? 10 : sf == 2 ? 14 : 18;
        if (n < hb) return -1;
        uint64_t h = 0;
        for (int i = 0; i < hb; ++i) h |= static_cast<uint64_t>(b[i]) << (8 * i);
        n_lit = static_cast<int64_t>((h >> 4) & ((1u << sb) - 1u));
        const int64_t n_comp = static_cast<int64_t>((h >> (4 + sb)) & ((1u << sb) - 1u));
        if (n_lit > kZstdBlockMax || n_lit > lit_cap || hb + n_comp > n) return -1;
        const uint8_t *q = b + hb, *const qend = q + n_comp;
        if (ltype == 2) {
            const int took = zs_read_huf(q, n_comp, tables, st);
            if (took < 0) return -1;
            q += took;
        } else if (st.huf_log == 0) {
            return -1;  // treeless, and no tree
        }
        const uint16_t *huf = reinterpret_cast<const uint16_t *>(tables + kZsHuf);
        if (sf == 0) {
            if (!zs_huf_stream(q, qend - q, huf, st.huf_log, lit_buf, n_lit)) return -1;
        } else {
            if (qend - q < 6) return -1;
            const int64_t s1 = q[0] | (q[1] << 8), s2 = q[2] | (q[3] << 8), s3 = q[4] | (q[5] << 8);
            q += 6;
            const int64_t s4 = (qend - q) - s1 - s2 - s3;
            const int64_t each = (n_lit + 3) / 4, last = n_lit - 3 * each;
            if (s4 < 1 || last < 0) return -1;
            if (!zs_huf_stream(q, s1, huf, st.huf_log, lit_buf, each)) return -1;
            if (!zs_huf_stream(q + s1, s2, huf, st.huf_log, lit_buf + each, each)) return -1;
            if (!zs_huf_stream(q + s1 + s2, s3, huf, st.huf_log, lit_buf + 2 * each, each)) return -1;
            if (!zs_huf_stream(q + s1 + s2 + s3, s4, huf, st.huf_log, lit_buf + 3 * each, last)) return -1;
        }
        lit = lit_buf;
        hdr = hb + n_comp;
    }
    int64_t lp = 0;  // literals used
    const int64_t block_first = op;
    auto copy_lit = [&](int64_t k) -> bool {
        if (k > n_lit - lp || k > cap - op) return false;
        if (lit_rle) {
            const uint8_t v = lit[0];
            for (int64_t i = 0; i < k; ++i) out[op + i] = v;
        } else {
            for (int64_t i = 0; i < k; ++i) out[op + i] = lit[lp + i];
        }
        lp += k;
        op += k;
        return true;
    };
    // ---- sequences section (3.1.1.3.2) ----
    const uint8_t *p = b + hdr, *const end = b + n;
    if (p >= end) return -1;
    int64_t n_seq = *p++;
    if (n_seq >= 128) {
        if (n_seq == 255) {
            if (end - p < 2) return -1;
            n_seq = p[0] + (static_cast<int64_t>(p[1]) << 8) + 0x7F00;
            p += 2;
        } else {
            if (end - p < 1) return -1;
            n_seq = ((n_seq - 128) << 8) + p[0];
            p += 1;
        }
    }
    if (n_seq == 0) {
        if (p != end) return -1;
    } else {
        if (p >= end) return -1;
        const int modes = *p++;
        if (modes & 3) return -1;  // reserved
        ZstdFse *ll = reinterpret_cast<ZstdFse *>(tables + kZsLL), *of = reinterpret_cast<ZstdFse *>(tables + kZsOF), *ml = reinterpret_cast<ZstdFse *>(tables + kZsML);
        if (!zs_seq_table(modes >> 6, p, end, 9, 35, kZstdLLDefault, 36, 6, ll, &st.ll_log, tables)) return -1;
        if (!zs_seq_table((modes >> 4) & 3, p, end, 8, 31, kZstdOFDefault, 29, 5, of, &st.of_log, tables)) return -1;
        if (!zs_seq_table((modes >> 2) & 3, p, end, 9, 52, kZstdMLDefault, 53, 6, ml, &st.ml_log, tables)) return -1;
        ZsBack br;
        if (!br.init(p, end - p)) return -1;
        const uint32_t ll_mask = (1u << st.ll_log) - 1u, of_mask = (1u << st.of_log) - 1u, ml_mask = (1u << st.ml_log) - 1u;
        uint32_t s_ll = br.read(st.ll_log) & ll_mask, s_of = br.read(st.of_log) & of_mask, s_ml = br.read(st.ml_log) & ml_mask;
        if (br.pos < 0) return -1;
        for (int64_t i = 0; i < n_seq; ++i) {
            const uint32_t c_of = of[s_of].sym, c_ll = ll[s_ll].sym, c_ml = ml[s_ml].sym;
            if (c_of > 31 || c_ll > 35 || c_ml > 52) return -1;
            const uint64_t ov = (uint64_t(1) << c_of) + br.read(static_cast<int>(c_of));
            const int64_t mlen = static_cast<int64_t>(kZstdMLBase[c_ml]) + br.read(kZstdMLBits[c_ml]);
            const int64_t llen = static_cast<int64_t>(kZstdLLBase[c_ll]) + br.read(kZstdLLBits[c_ll]);
            if (i + 1 < n_seq) {  // the states move in this order; the last sequence leaves them where they are
                s_ll = (ll[s_ll].base + br.read(ll[s_ll].nbits)) & ll_mask;
                s_ml = (ml[s_ml].base + br.read(ml[s_ml].nbits)) & ml_mask;
                s_of = (of[s_of].base + br.read(of[s_of].nbits)) & of_mask;
            }
            if (br.pos < 0) return -1;
            uint64_t offset;
            if (ov > 3) {
                offset = ov - 3;
                st.rep[2] = st.rep[1];
                st.rep[1] = st.rep[0];
                st.rep[0] = static_cast<uint32_t>(offset);
            } else {
                const int idx = static_cast<int>(ov) + (llen == 0 ? 1 : 0);  // 1 .. 4
                if (idx == 1) {
                    offset = st.rep[0];
                } else {
                    offset = idx == 4 ? st.rep[0] - 1u : st.rep[idx - 1];
                    if (offset == 0) return -1;
                    if (idx > 2) st.rep[2] = st.rep[1];
                    st.rep[1] = st.rep[0];
                    st.rep[0] = static_cast<uint32_t>(offset);
                }
            }
            if (!copy_lit(llen)) return -1;
            // a match lies inside this frame's output, and fits the slot; it may overlap what it writes
            if (offset > static_cast<uint64_t>(op - first) || mlen > cap - op) return -1;
            const uint8_t *src = out + op - static_cast<int64_t>(offset);
            for (int64_t k = 0; k < mlen; ++k) out[op + k] = src[k];
            op += mlen;
        }
        if (br.pos != 0) return -1;  // the stream ends with the last sequence
    }
    if (!copy_lit(n_lit - lp)) return -1;
    if (op - block_first > kZstdBlockMax) return -1;
    return op;
}

// in[0 .. in_bytes): zstd frames -> out[0 .. out_cap); returns the bytes produced or -1.  `tables`: kZstdTableBytes, 4-byte
// aligned; `lit`: lit_cap bytes, min(kZstdBlockMax, out_cap) at least (they may lie in another memory than the tables)
ZS_DEV inline int zstd_frame_lane2(const uint8_t *in, int64_t in_bytes, uint8_t *out, int64_t out_cap, uint8_t *tables, uint8_t *lit, int64_t lit_cap) {
    if (in_bytes < 4 || out_cap < 0) return -1;
    if (out_cap > 0x7fffffff) out_cap = 0x7fffffff;
    int64_t ip = 0, op = 0;
    while (ip < in_bytes) {
        if (in_bytes - ip < 4) return -1;
        uint32_t magic;
        __builtin_memcpy(&magic, in + ip, 4);
        ip += 4;
        if ((magic & 0xfffffff0u) == 0x184D2A50u) {  // skippable frame: a size and that many bytes
            if (in_bytes - ip < 4) return -1;
            uint32_t sz;
            __builtin_memcpy(&sz, in + ip, 4);
            ip += 4;
            if (sz > in_bytes - ip) return -1;
            ip += sz;
            continue;
        }
        if (magic != 0xFD2FB528u || in_bytes - ip < 1) return -1;
        const int fhd = in[ip++];
        const int fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, checksum = (fhd >> 2) & 1, did_flag = fhd & 3;
        if (fhd & 8) return -1;  // reserved bit
        uint64_t window = 0;
        if (!single) {
            if (in_bytes - ip < 1) return -1;
            const int wd = in[ip++];
            const uint64_t base = uint64_t(1) << (10 + (wd >> 3));
            window = base + (base >> 3) * (wd & 7);
        }
        const int did_bytes = did_flag == 3 ? 4 : did_flag;
        if (in_bytes - ip < did_bytes) return -1;
        for (int i = 0; i < did_bytes; ++i)
            if (in[ip + i] != 0) return -1;  // a dictionary: none here
        ip += did_bytes;
        const int fcs_bytes = fcs_flag == 0 ? single : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
        if (in_bytes - ip < fcs_bytes) return -1;
        uint64_t fcs = 0;
        for (int i = 0; i < fcs_bytes; ++i) fcs |= static_cast<uint64_t>(in[ip + i]) << (8 * i);
        if (fcs_bytes == 2) fcs += 256;
        ip += fcs_bytes;
        if (single) window = fcs;
        if (fcs_bytes && fcs > static_cast<uint64_t>(out_cap - op)) return -1;
        const int64_t block_max = window < static_cast<uint64_t>(kZstdBlockMax) ? static_cast<int64_t>(window) : kZstdBlockMax;
        const int64_t first = op;
        ZstdState st;
        st.huf_log = 0;
        st.ll_log = st.of_log = st.ml_log = -1;
        st.rep[0] = 1, st.rep[1] = 4, st.rep[2] = 8;
        for (;;) {
            if (in_bytes - ip < 3) return -1;
            const uint32_t bh = in[ip] | (in[ip + 1] << 8) | (static_cast<uint32_t>(in[ip + 2]) << 16);
            ip += 3;
            const int last = bh & 1, type = (bh >> 1) & 3;
            const int64_t bs = bh >> 3;
            if (type == 3 || bs > block_max) return -1;
            if (type == 0) {
                if (bs > in_bytes - ip || bs > out_cap - op) return -1;
                for (int64_t i = 0; i < bs; ++i) out[op + i] = in[ip + i];
                ip += bs;
                op += bs;
            } else if (type == 1) {
                if (in_bytes - ip < 1 || bs > out_cap - op) return -1;
                const uint8_t v = in[ip++];
                for (int64_t i = 0; i < bs; ++i) out[op + i] = v;
                op += bs;
            } else {
                if (bs > in_bytes - ip) return -1;
                op = zs_block(in + ip, bs, out, op, first, out_cap, tables, lit, lit_cap, st);
                if (op < 0) return -1;
                ip += bs;
            }
            if (last) break;
        }
        if (fcs_bytes && static_cast<uint64_t>(op - first) != fcs) return -1;
        if (checksum) {
            if (in_bytes - ip < 4) return -1;
            uint32_t want;
            __builtin_memcpy(&want, in + ip, 4);
            ip += 4;
            if (static_cast<uint32_t>(zs_xxh64(out + first, op - first)) != want) return -1;
        }
    }
    return static_cast<int>(op);
}

// the same with one scratch area of zstd_scratch_bytes(out_cap) bytes, 4-byte aligned: tables, then literals
ZS_DEV inline int zstd_frame_lane(const uint8_t *in, int64_t in_bytes, uint8_t *out, int64_t out_cap, uint8_t *scratch) {
    return zstd_frame_lane2(in, in_bytes, out, out_cap, scratch, scratch + kZstdTableBytes, zstd_scratch_bytes(out_cap) - kZstdTableBytes);
}

// the content size the first frame's header states, or -1 (none stated, or no frame header at in[0]): lets a reader size its buffer
ZS_DEV inline int64_t zstd_stated_size(const uint8_t *in, int64_t in_bytes) {
    if (in_bytes < 5) return -1;
    uint32_t magic;
    __builtin_memcpy(&magic, in, 4);
    if (magic != 0xFD2FB528u) return -1;
    const int fhd = in[4], fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did_flag = fhd & 3;
    const int fcs_bytes = fcs_flag == 0 ? single : fcs_flag == 1 ? 2 : fcs_flag == 2 ? 4 : 8;
    const int64_t at = 5 + (single ? 0 : 1) + (did_flag == 3 ? 4 : did_flag);
    if (!fcs_bytes || in_bytes < at + fcs_bytes) return -1;
    uint64_t fcs = 0;
    for (int i = 0; i < fcs_bytes; ++i) fcs |= static_cast<uint64_t>(in[at + i]) << (8 * i);
    if (fcs_bytes == 2) fcs += 256;
    return fcs > static_cast<uint64_t>(INT64_MAX) ? INT64_MAX : static_cast<int64_t>(fcs);
}

}  // namespace sfa
