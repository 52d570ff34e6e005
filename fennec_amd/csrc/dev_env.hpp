// Development switches (tile sizes, priorities, thresholds, A/B of two correct kernels) exist in `make DEVELOP=1` builds only:
// dev_env() is getenv there and a constant nullptr in a release build, so the compiler drops the branch (common.hpp: what
// steers the library from outside).  Plain C++: the host-only plans read their switches through it too.
#pragma once
#include <cstdlib>

namespace fnx {

#ifdef FNX_DEVELOP
inline const char *dev_env(const char *name) { return std::getenv(name); }
#else
inline const char *dev_env(const char *) { return nullptr; }
#endif

}  // namespace fnx
