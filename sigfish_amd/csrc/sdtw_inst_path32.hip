// sdtw_inst_path32.hip -- explicit instantiations of the band fill behind sfa_event_maps (sdtw_path.hpp): 32 rows per lane, and
// the same shape in row strips for queries beyond 2048 events
#include "sdtw_path.hpp"

namespace sfa {
template __global__ void sdtw_path_fill_kernel<32, 64, false>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<32, 32, false>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<32, 16, false>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<32, 64, true>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<32, 32, true>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<32, 16, true>(const PathArgs);
template __global__ void sdtw_path_strip_kernel<false, false>(const PathArgs);
template __global__ void sdtw_path_strip_kernel<false, true>(const PathArgs);
template __global__ void sdtw_path_strip_kernel<true, false>(const PathArgs);
template __global__ void sdtw_path_strip_kernel<true, true>(const PathArgs);
}  // namespace sfa
