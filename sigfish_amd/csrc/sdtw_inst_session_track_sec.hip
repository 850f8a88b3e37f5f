// alignment sessions with candidate lists (sfa_session_candidates_config), start columns carried (sdtw_session.hpp)
#include "sdtw_session.hpp"
namespace sfa {
template __global__ void sdtw_session_kernel<true, true>(const SessionArgs);
}
