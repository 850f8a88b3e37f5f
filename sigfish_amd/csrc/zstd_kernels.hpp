// zstd_kernels.hpp -- zstd-compressed BLOW5 records decompressed ON THE DEVICE: blow5_zstd_kernel fills the payload slots that
// blow5_inflate_kernel fills for zlib records (out / out_off / out_len of blow5_kernels.hpp), so that blow5_fields_kernel,
// blow5_svb_kernel and everything behind them run unchanged.  The decoder is zstd_lane.hpp, the text the host reader compiles:
// serial per record, so the parallelism is over the records of a batch -- ONE LANE PER RECORD, `lanes` records per wave chosen
// by the host from the batch size (see blow5_inflate_kernel on why the records are spread thin).
//
// Where the 9 984 bytes of tables of a decoder live (the literals of a block, up to 128 KB, are in HBM either way):
//   kLds = true   in LDS, at most kZstdLdsLanes decoders per block within the 64 KB a launch may ask for (the shipping placement:
//                 3.27 ms against 3.64 ms for 4 096 records)
//   kLds = false  in the record's scratch area in HBM, planned by the host beside the payload slots
// Both are built; option "zstd_tables" of a context chooses (1 LDS, 0 HBM).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef SFA_DEFINE_ZSTD_KERNELS  // (the decoder's text reaches no other unit's device code)
#include "zstd_lane.hpp"
#endif

namespace sfa {

struct ZstdArgs {
    const uint8_t *in;           // records back to back
    const int64_t *in_off;       // [n+1]
    uint8_t *out;                // payloads, slot i = [out_off[i], out_off[i+1])
    const int64_t *out_off;      // [n+1] capacities
    int32_t *out_len;            // [n] bytes produced, -1: declined (malformed, truncated, or larger than its slot)
    uint8_t *scratch;            // area i = [scratch_off[i], scratch_off[i+1]): zstd_scratch_bytes(slot size), 16-byte aligned
    const int64_t *scratch_off;  // [n+1]
    int32_t n;
};

constexpr int kZstdMaxLanes = 32;  // records per wave, tables in HBM
constexpr int kZstdLdsLanes = 4;   // ... tables in LDS: 4 x 9 984 bytes (6 would fit 64 KB; a power of two keeps the host's choice simple)

// bytes of scratch the host plans for a record whose slot holds slot_bytes (zstd_scratch_bytes, rounded up to 16)
int64_t blow5_zstd_scratch_bytes(int64_t slot_bytes);
// records, offsets and slots are on the device already (stream order); launches only
void launch_blow5_zstd(const ZstdArgs &a, int cu_count, bool lds_tables, hipStream_t stream);

#ifdef SFA_DEFINE_ZSTD_KERNELS  // defined in exactly one translation unit (sfa_zstd.hip)
template <bool kLds>
__global__ void __launch_bounds__(64) blow5_zstd_kernel(const ZstdArgs a, const int lanes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char zstd_lds[];
    if (static_cast<int>(threadIdx.x) >= lanes) return;
    const int i = blockIdx.x * lanes + threadIdx.x;
    if (i >= a.n) return;
    const int64_t b = a.in_off[i], e = a.in_off[i + 1];
    const int64_t ob = a.out_off[i], oe = a.out_off[i + 1];
    const int64_t sb = a.scratch_off[i], se = a.scratch_off[i + 1];
    const int64_t cap = oe - ob;
    // the host plans zstd_scratch_bytes(cap) per record; a plan that gives less gets no decoder
    if (e < b || cap < 0 || se - sb < zstd_scratch_bytes(cap)) {
        a.out_len[i] = -1;
        return;
    }
    uint8_t *const area = a.scratch + sb;
    uint8_t *const tables = kLds ? zstd_lds + static_cast<size_t>(threadIdx.x) * kZstdTableBytes : area;
    a.out_len[i] = zstd_frame_lane2(a.in + b, e - b, a.out + ob, cap, tables, area + kZstdTableBytes, se - sb - kZstdTableBytes);
}
#endif

}  // namespace sfa
