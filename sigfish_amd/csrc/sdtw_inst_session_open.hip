// alignment sessions, open and closed target groups: the two-class reduction under a bitmap of open groups (sdtw_session_open.hpp)
#define SFA_DEFINE_SESSION_OPEN_KERNELS
#include "sdtw_session_open.hpp"
