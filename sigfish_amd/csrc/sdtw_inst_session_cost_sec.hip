// alignment sessions with candidate lists, costs only: SFA_SESSION_NO_START (sdtw_session.hpp)
#include "sdtw_session.hpp"
namespace sfa {
template __global__ void sdtw_session_kernel<false, true>(const SessionArgs);
}
