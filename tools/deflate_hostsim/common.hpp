// Stand-in for csrc/common.hpp when deflate.hip is compiled for the CPU (tools/deflate_hostsim): the HIP words the file uses,
// with a workgroup run as 256 host threads.  __shared__ is static storage (one workgroup runs at a time), __syncthreads a
// barrier over the 256 threads, the atomics are the host's, a launch runs the grid's workgroups one after the other.
#pragma once
#include <pthread.h>

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

#include "fennec_hip.h"

#define __global__
#define __device__
#define __shared__ static
#define __forceinline__ inline
#define __launch_bounds__(n)

namespace fnx_sim {
constexpr int LANES = 256;
struct Idx { unsigned x; };
inline thread_local Idx t_thread, t_block;
inline pthread_barrier_t g_barrier;
inline unsigned long long g_lanes[LANES];                             // __shfl_xor's exchange

inline void run_grid(unsigned nblocks, unsigned lanes, const std::function<void()> &body)
{
    if (lanes != LANES) abort();
    pthread_barrier_init(&g_barrier, nullptr, LANES);
    for (unsigned b = 0; b < nblocks; b++) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < LANES; t++) th.emplace_back([&, t] { t_thread.x = t; t_block.x = b; body(); });
        for (auto &x : th) x.join();
    }
    pthread_barrier_destroy(&g_barrier);
}
}  // namespace fnx_sim

#define threadIdx fnx_sim::t_thread
#define blockIdx fnx_sim::t_block
struct dim3 { unsigned x; explicit dim3(unsigned v) : x(v) {} };
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) fnx_sim::run_grid((grid).x, (block).x, [&] { kernel(__VA_ARGS__); })
inline int hipGetLastError() { return 0; }

inline void __syncthreads() { pthread_barrier_wait(&fnx_sim::g_barrier); }
inline uint32_t atomicAdd(uint32_t *p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline uint32_t atomicOr(uint32_t *p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
inline uint32_t atomicMax(uint32_t *p, uint32_t v)
{
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
inline int __clz(int v) { return v ? __builtin_clz(static_cast<unsigned>(v)) : 32; }
inline uint32_t __brev(uint32_t v)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
// every lane of the workgroup calls it; a lane's partner is in its own wave of 64 for every offset below 64
inline unsigned long long __shfl_xor(unsigned long long v, int off, int width)
{
    (void)width;
    fnx_sim::g_lanes[threadIdx.x] = v;
    __syncthreads();
    const unsigned long long r = fnx_sim::g_lanes[threadIdx.x ^ static_cast<unsigned>(off)];
    __syncthreads();
    return r;
}
// v_alignbyte_b32: bytes sel .. sel + 3 of the eight bytes hi : lo
#define __builtin_amdgcn_alignbyte(hi, lo, sel) \
    static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | static_cast<uint64_t>(lo)) >> (8 * ((sel) & 3)))

// ---- the host side of launch_deflate: a context that only hands out memory
struct fnx_ctx { void *slot[4]; void *stream; int deflate_level; };
namespace fnx {
enum Slot { SLOT_DEFLATE_TOK, SLOT_DEFLATE_SLOTS, SLOT_DEFLATE_OUT, SLOT_DEFLATE_SIZE };
inline int scratch(fnx_ctx *ctx, Slot s, size_t bytes, void **out)
{
    free(ctx->slot[s]);
    *out = ctx->slot[s] = aligned_alloc(16, (bytes + 15) & ~size_t(15));
    return *out ? FNX_OK : FNX_ERR_INVALID;
}
inline void note_route(fnx_ctx *, int, const char *) {}
inline int prof_begin(fnx_ctx *, int = FNX_PROF_MAIN) { return FNX_OK; }
inline int prof_end(fnx_ctx *) { return FNX_OK; }
}  // namespace fnx
#define FNX_TRY(expr) do { const int rc_ = (expr); if (rc_ != FNX_OK) return rc_; } while (0)
#define FNX_HIP(expr) do { if ((expr) != 0) return FNX_ERR_INVALID; } while (0)
