// alignment sessions, reach targets: the base mask and the anchor table from the prepared runs, the live mask under a depth cap
// (sdtw_session_reach.hpp)
#define SFA_DEFINE_SESSION_REACH_KERNELS
#include "sdtw_session_reach.hpp"
