// hip/hip_runtime.h -- a stand-in for HIP's header that lets the kernel files
// of bsdb_amd/csrc compile unchanged as plain C++20 for the host (clang++,
// whose extensions they use) and runs a launch on the CPU, so that a
// stand-alone program can put the kernels under ASan + UBSan
// (tests/piece_host_check.cpp, tests/test_piece_host_cpu.py).  Test code: the
// library never includes it.
//
// The execution model.  hostwave::launch(grid, threads, kernel, args...) runs
// the workgroups of the grid one after another.  A workgroup is `threads`
// lanes; every lane is a fiber (ucontext) with a stack of its own, all on the
// calling thread, created once and kept across launches.  A lane runs until it
// meets a barrier or returns; then the next lane runs, in lane order, so a run
// is deterministic: nothing depends on a scheduler.  __shared__ is `static`,
// which is sound because one workgroup is alive at a time (it starts zeroed and
// keeps what the last workgroup left, where LDS starts with anything).
// threadIdx, blockIdx, gridDim and blockDim are variables the launcher sets
// whenever it resumes a lane.
//
// __syncthreads is a barrier of the workgroup.  __shfl, __shfl_xor, __shfl_up,
// __ballot and __builtin_amdgcn_readlane exchange through a slot per lane of
// the wave (64 lanes) between two barriers of the wave.  A lane that has
// returned from the kernel has left both barriers and counts as inactive: a
// ballot sees 0 from it, a shuffle from it returns the caller's own value.  A
// barrier that can never complete (some live lane of the wave or workgroup
// waits elsewhere, or not at all) is reported and the program aborts: barrier
// placement that is not uniform does not pass silently.  ASan is told of every
// fiber switch (its fiber annotations), so stack checks stay exact.
//
// What this emulation checks: addressing (every load and store, global and
// "LDS", under ASan), arithmetic (UBSan), wave-uniform control flow and barrier
// placement.  What it says nothing about: the memory model, lanes of one wave
// racing through LDS or global memory (lanes here never run at the same time,
// and between two barriers one lane runs to the end before the next starts),
// code generation, and speed.  The GPU suite stays the judge of the real
// kernels.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <ucontext.h>

#include <type_traits>
#include <utility>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define HOSTWAVE_ASAN 1
#endif
#endif
#if defined(HOSTWAVE_ASAN)
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>
#endif

// ---- qualifiers ------------------------------------------------------------
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static

// ---- types -----------------------------------------------------------------
struct dim3 {
    uint32_t x, y, z;
    constexpr dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {}
};
struct alignas(8) uint2 {
    uint32_t x, y;
};
struct alignas(16) uint4 {
    uint32_t x, y, z, w;
};
// (A copy of an aggregate is a memcpy, at which UBSan does not look; these copy through a reference, so a 16-byte
// load from an address that is no multiple of 16 -- fine for x86 and for the GPU alike -- is a report here.)
struct alignas(16) ulonglong2 {
    unsigned long long x, y;
    ulonglong2() = default;
    constexpr ulonglong2(unsigned long long x_, unsigned long long y_) : x(x_), y(y_) {}
    constexpr ulonglong2(const ulonglong2 &o) : x(o.x), y(o.y) {}
    constexpr ulonglong2 &operator=(const ulonglong2 &o) {
        x = o.x, y = o.y;
        return *this;
    }
};
inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
inline ulonglong2 make_ulonglong2(unsigned long long x, unsigned long long y) { return ulonglong2{x, y}; }

inline dim3 threadIdx, blockIdx, gridDim, blockDim;

namespace hostwave {

constexpr uint32_t WAVE = 64;
constexpr uint32_t MAX_THREADS = 1024;
constexpr size_t STACK_BYTES = 256 << 10;

struct Fiber {
    ucontext_t uc;
    uint8_t *stack = nullptr;
    void *fake = nullptr;  // ASan's fake stack of the fiber while it is switched out
    bool live = false;     // inside the kernel of the workgroup that is running
};

struct Group {
    ucontext_t main_uc;
    void *main_fake = nullptr;
    const void *main_bottom = nullptr;
    size_t main_size = 0;
    Fiber lane[MAX_THREADS];
    uint32_t made = 0;     // fibers created so far
    uint32_t threads = 0;  // of the launch under way
    uint32_t cur = 0;      // the lane that runs
    void (*body)(void *) = nullptr;
    void *body_arg = nullptr;
    dim3 block;
    // barriers: arrivals and a generation per wave and for the workgroup
    uint32_t wave_alive[MAX_THREADS / WAVE], wave_arrived[MAX_THREADS / WAVE], wave_gen[MAX_THREADS / WAVE];
    uint32_t group_alive = 0, group_arrived = 0, group_gen = 0;
    uint64_t progress = 0;  // barriers passed and lanes finished: a round without any is a deadlock
    uint64_t slot[MAX_THREADS];
};

inline Group &group() {
    static Group *g = new Group();  // (never freed: the fibers' stacks live as long as the program)
    return *g;
}

inline void switch_context(ucontext_t *from, void **from_fake, ucontext_t *to, const void *to_bottom, size_t to_size) {
#if defined(HOSTWAVE_ASAN)
    __sanitizer_start_switch_fiber(from_fake, to_bottom, to_size);
#else
    (void)from_fake, (void)to_bottom, (void)to_size;
#endif
    swapcontext(from, to);
#if defined(HOSTWAVE_ASAN)
    __sanitizer_finish_switch_fiber(*from_fake, nullptr, nullptr);
#endif
}

// the running lane hands the thread back to the launcher
inline void yield() {
    Group &g = group();
    Fiber &f = g.lane[g.cur];
    switch_context(&f.uc, &f.fake, &g.main_uc, g.main_bottom, g.main_size);
}

inline void lane_leaves(Group &g, uint32_t t) {  // arrive_and_drop at both barriers
    const uint32_t w = t / WAVE;
    g.lane[t].live = false;
    ++g.progress;
    if (--g.wave_alive[w] && g.wave_arrived[w] == g.wave_alive[w]) g.wave_arrived[w] = 0, ++g.wave_gen[w];
    if (--g.group_alive && g.group_arrived == g.group_alive) g.group_arrived = 0, ++g.group_gen;
}

// A fiber's life: run the kernel of every workgroup it is handed, for ever.
inline void fiber_main() {
    Group &g = group();
#if defined(HOSTWAVE_ASAN)
    __sanitizer_finish_switch_fiber(nullptr, &g.main_bottom, &g.main_size);
#endif
    for (;;) {
        const uint32_t t = g.cur;
        g.body(g.body_arg);
        lane_leaves(g, t);
        yield();
    }
}

inline void wave_barrier() {
    Group &g = group();
    const uint32_t w = g.cur / WAVE, gen = g.wave_gen[w];
    if (++g.wave_arrived[w] == g.wave_alive[w]) g.wave_arrived[w] = 0, ++g.wave_gen[w];
    while (g.wave_gen[w] == gen) yield();
    ++g.progress;
}

inline void group_barrier() {
    Group &g = group();
    const uint32_t gen = g.group_gen;
    if (++g.group_arrived == g.group_alive) g.group_arrived = 0, ++g.group_gen;
    while (g.group_gen == gen) yield();
    ++g.progress;
}

inline void run_group(Group &g, dim3 grid, dim3 block_index) {
    for (uint32_t w = 0; w < MAX_THREADS / WAVE; ++w) g.wave_alive[w] = g.wave_arrived[w] = 0;
    for (uint32_t t = 0; t < g.threads; ++t) {
        g.lane[t].live = true;
        ++g.wave_alive[t / WAVE];
    }
    g.group_alive = g.threads, g.group_arrived = 0;
    for (uint32_t left = g.threads; left;) {
        const uint64_t before = g.progress;
        left = 0;
        for (uint32_t t = 0; t < g.threads; ++t) {
            if (!g.lane[t].live) continue;
            g.cur = t;
            threadIdx = dim3(t), blockIdx = block_index, gridDim = grid, blockDim = g.block;
            switch_context(&g.main_uc, &g.main_fake, &g.lane[t].uc, g.lane[t].stack, STACK_BYTES);
            left += g.lane[t].live;
        }
        if (left && g.progress == before) {
            fprintf(stderr, "hostwave: workgroup %u: %u lanes wait at a barrier that cannot complete\n", block_index.x, left);
            abort();
        }
    }
}

template <class... KArgs, class... Args>
inline void launch(dim3 grid, dim3 threads, void (*kernel)(KArgs...), Args &&...args) {
    Group &g = group();
    if (!threads.x || threads.x > MAX_THREADS || threads.y != 1 || threads.z != 1 || grid.y != 1 || grid.z != 1) {
        fprintf(stderr, "hostwave: a launch is grid (x, 1, 1) of 1 .. %u threads\n", MAX_THREADS);
        abort();
    }
    for (; g.made < threads.x; ++g.made) {
        Fiber &f = g.lane[g.made];
        // (a page that cannot be touched below the stack: an overflow is a fault, not a neighbour's bytes)
        void *p = mmap(nullptr, 4096 + STACK_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED || mprotect(p, 4096, PROT_NONE)) abort();
        f.stack = (uint8_t *)p + 4096;
        getcontext(&f.uc);
        f.uc.uc_stack.ss_sp = f.stack;
        f.uc.uc_stack.ss_size = STACK_BYTES;
        f.uc.uc_link = nullptr;
        makecontext(&f.uc, fiber_main, 0);
    }
    auto call = [&]() { kernel(KArgs(args)...); };  // every lane gets its own copy of the arguments, as on the device
    g.body = [](void *c) { (*static_cast<decltype(call) *>(c))(); };
    g.body_arg = &call;
    g.threads = threads.x;
    g.block = threads;
    for (uint32_t b = 0; b < grid.x; ++b) run_group(g, grid, dim3(b));
}

// ---- wave operations ---------------------------------------------------------
template <class T>
inline uint64_t to_slot(T v) {
    static_assert(std::is_trivially_copyable<T>::value && sizeof(T) <= 8, "a shuffle moves up to 8 bytes");
    uint64_t s = 0;
    memcpy(&s, &v, sizeof(T));
    return s;
}
template <class T>
inline T from_slot(uint64_t s) {
    T v;
    memcpy(&v, &s, sizeof(T));
    return v;
}

// lane `src` of the caller's wave holds the value, or -1: the caller's own
template <class T>
inline T exchange(T v, int src) {
    Group &g = group();
    const uint32_t me = g.cur, base = me & ~(WAVE - 1);
    g.slot[me] = to_slot(v);
    wave_barrier();
    T out = v;
    if (src >= 0 && base + (uint32_t)src < g.threads && g.lane[base + (uint32_t)src].live) out = from_slot<T>(g.slot[base + (uint32_t)src]);
    wave_barrier();
    return out;
}

inline uint32_t lane_id() { return group().cur & (WAVE - 1); }

inline uint64_t ballot(bool pred) {
    Group &g = group();
    const uint32_t me = g.cur, base = me & ~(WAVE - 1);
    g.slot[me] = pred;
    wave_barrier();
    uint64_t m = 0;
    for (uint32_t l = 0; l < WAVE && base + l < g.threads; ++l)
        if (g.lane[base + l].live && g.slot[base + l]) m |= 1ull << l;
    wave_barrier();
    return m;
}

inline uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((uint64_t)hi << 32 | lo) >> (sh & 31)); }

}  // namespace hostwave

inline void __syncthreads() { hostwave::group_barrier(); }

template <class T>
inline T __shfl(T v, int src, int width = 64) {
    const int lane = (int)hostwave::lane_id();
    return hostwave::exchange(v, (lane & ~(width - 1)) | (src & (width - 1)));
}
template <class T>
inline T __shfl_xor(T v, int mask, int width = 64) {
    const int lane = (int)hostwave::lane_id(), src = lane ^ mask;
    return hostwave::exchange(v, (src & ~(width - 1)) == (lane & ~(width - 1)) ? src : -1);
}
template <class T>
inline T __shfl_up(T v, unsigned delta, int width = 64) {
    const int lane = (int)hostwave::lane_id(), src = lane - (int)delta;
    return hostwave::exchange(v, src >= (lane & ~(width - 1)) ? src : -1);
}
inline uint64_t __ballot(int pred) { return hostwave::ballot(pred != 0); }

#define __builtin_amdgcn_readlane(v, l) hostwave::exchange((uint32_t)(v), (int)(l))
#define __builtin_amdgcn_alignbit(hi, lo, sh) hostwave::alignbit((hi), (lo), (sh))

// ---- bits and products -------------------------------------------------------
inline int __popc(uint32_t x) { return __builtin_popcount(x); }
inline int __popcll(uint64_t x) { return __builtin_popcountll(x); }
inline int __clzll(long long x) { return x ? __builtin_clzll((unsigned long long)x) : 64; }
inline uint32_t __umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
inline uint64_t __umul64hi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

// ---- atomics (one lane runs at a time; kept atomic all the same) ----------------
template <class T>
inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
template <class T>
inline T atomicOr(T *p, T v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
template <class T>
inline T atomicMax(T *p, T v) {
    T old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
template <class T>
inline T atomicMin(T *p, T v) {
    T old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
