// sdtw_inst_strips_pipe_sec.hip -- row strips, pipelined pass 1 with the candidate lists of secondary mappings (sdtw_strips.hpp)
#include "sdtw_strips.hpp"
namespace sfa {
template __global__ void sdtw_strip_sec_pipe_kernel<false>(const StripArgs, int32_t *);
template __global__ void sdtw_strip_sec_pipe_kernel<true>(const StripArgs, int32_t *);
}  // namespace sfa
