// alignment sessions, target groups: the labelled reduction over the carried rows and its heads (sdtw_session_group.hpp)
#define SFA_DEFINE_SESSION_GROUP_KERNELS
#include "sdtw_session_group.hpp"
