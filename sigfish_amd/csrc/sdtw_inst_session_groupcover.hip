// alignment sessions, group caps: the live label table and the depth record of every group (sdtw_session_groupcover.hpp)
#define SFA_DEFINE_SESSION_GROUPCOVER_KERNELS
#include "sdtw_session_groupcover.hpp"
