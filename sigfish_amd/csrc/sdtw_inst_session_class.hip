// alignment sessions, target classes: the masked reduction over the carried rows and its merge (sdtw_session_class.hpp)
#define SFA_DEFINE_SESSION_CLASS_KERNELS
#include "sdtw_session_class.hpp"
