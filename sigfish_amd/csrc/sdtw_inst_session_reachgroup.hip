// alignment sessions, reach groups: the label table and its anchors from the prepared runs, the live labels under a group cap,
// the depth records over the body columns (sdtw_session_reachgroup.hpp)
#define SFA_DEFINE_SESSION_REACHGROUP_KERNELS
#include "sdtw_session_reachgroup.hpp"
