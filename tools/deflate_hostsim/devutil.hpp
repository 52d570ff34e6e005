// Stand-in for csrc/devutil.hpp on the CPU: global-memory dwords are plain dwords.
#pragma once
#include <cstdint>
typedef const uint32_t g_u32;
typedef uint32_t g_u32w;
