// sdtw_inst_path16.hip -- explicit instantiations of the band fill behind sfa_event_maps (sdtw_path.hpp): 16 lanes per row
#include "sdtw_path.hpp"

namespace sfa {
template __global__ void sdtw_path_fill_kernel<16, 16, false>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<8, 16, false>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<4, 16, false>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<16, 16, true>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<8, 16, true>(const PathArgs);
template __global__ void sdtw_path_fill_kernel<4, 16, true>(const PathArgs);
}  // namespace sfa
