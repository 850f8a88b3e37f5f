// alignment sessions, start columns carried and propagated (sdtw_session.hpp)
#include "sdtw_session.hpp"
namespace sfa {
template __global__ void sdtw_session_kernel<true>(const SessionArgs);
}
