// boxDownsample's source range of an output index: one text for the kernels (devutil.hpp) and for the host-only plans, which
// are also built without HIP (blur_plan.cpp).
#pragma once

#ifdef __HIPCC__
#define FNX_HOST_DEVICE __host__ __device__ inline __attribute__((always_inline))   // (__forceinline__, spelt out: no HIP header needed)
#else
#define FNX_HOST_DEVICE inline
#endif

namespace fnx {

// boxDownsample's source range of output index d (ssim.go:262-275)
FNX_HOST_DEVICE void box_edge(int d, double ratio, int srcN, int &s0, int &s1)
{
    s0 = static_cast<int>(static_cast<double>(d) * ratio);
    s1 = static_cast<int>(static_cast<double>(d + 1) * ratio);
    if (s1 > srcN) s1 = srcN;
    if (s0 >= s1) s0 = s1 - 1;
    if (s0 < 0) s0 = 0;
}

}  // namespace fnx
