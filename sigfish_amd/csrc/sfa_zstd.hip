// sfa_zstd.hip -- the device-side zstd record decoder (zstd_kernels.hpp): its kernels and their launch, a unit of its own so
// that the units of the other BLOW5 kernels compile exactly as before.
#include <hip/hip_runtime.h>

#define SFA_DEFINE_ZSTD_KERNELS
#include "zstd_kernels.hpp"

namespace sfa {

// records per wave: about one wave per SIMD, as for the device inflate (blow5_inflate_kernel, inflate_lanes)
static int zstd_lanes(int32_t n, int cu_count, int max_lanes) {
    const int64_t simds = static_cast<int64_t>(cu_count) * 4;
    int lanes = 1;
    while (lanes < max_lanes && static_cast<int64_t>(n) > simds * lanes) lanes *= 2;
    return lanes;
}

int64_t blow5_zstd_scratch_bytes(int64_t slot_bytes) { return (zstd_scratch_bytes(slot_bytes) + 15) & ~int64_t(15); }

void launch_blow5_zstd(const ZstdArgs &a, int cu_count, bool lds_tables, hipStream_t stream) {
    if (a.n <= 0) return;
    if (lds_tables) {
        const int lanes = zstd_lanes(a.n, cu_count, kZstdLdsLanes);
        hipLaunchKernelGGL(blow5_zstd_kernel<true>, dim3((a.n + lanes - 1) / lanes), dim3(64), static_cast<size_t>(kZstdTableBytes) * lanes, stream, a, lanes);
    } else {
        const int lanes = zstd_lanes(a.n, cu_count, kZstdMaxLanes);
        hipLaunchKernelGGL(blow5_zstd_kernel<false>, dim3((a.n + lanes - 1) / lanes), dim3(64), 0, stream, a, lanes);
    }
}

}  // namespace sfa
