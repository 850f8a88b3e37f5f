// alignment sessions, coverage caps: depth tracks on the device and the live mask derived from them (sdtw_session_cover.hpp)
#define SFA_DEFINE_SESSION_COVER_KERNELS
#include "sdtw_session_cover.hpp"
