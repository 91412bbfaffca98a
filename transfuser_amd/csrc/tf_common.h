// Host-side helpers shared by every C-ABI translation unit.
#pragma once
#include "tf_prims.h"
#include <stdio.h>
#include <string.h>

namespace tf {

void set_error(const char* fmt, ...);  // api.cpp
bool ablated(const char* kernel);      // api.cpp: TF_ABLATE=substr[,substr...] turns the matching kernels' launches into no-ops (timing diagnosis only)
bool deterministic();                  // api.cpp: tf_set_deterministic - every reduction that would end in fp32 atomics takes its fixed-order form (or refuses); read on the host at launch time
long float_atomic_count(int add);      // api.cpp: launches of kernel forms that combine partial results with float atomics (tf_float_atomic_launches)
long slab_splitk_count(int add);       // api.cpp: launches of the ordered slab k-split of the MFMA engine (tf_slab_splitk_launches)

#ifdef TF_EMU
#define TF_LAUNCH_AS(name, kern, grid, block, stream, ...)               \
    do {                                                                    \
        (void)(stream);                                                     \
        emu::launch((grid), (block), [=]() { kern(__VA_ARGS__); });         \
    } while (0)
inline int launch_status(const char*) { return 0; }
#else
#define TF_LAUNCH_AS(name, kern, grid, block, stream, ...)                                              \
    do {                                                                                                   \
        static const bool tf_ablated_ = tf::ablated(name);                                               \
        if (!tf_ablated_) hipLaunchKernelGGL(kern, (grid), (block), 0, (hipStream_t)(stream), __VA_ARGS__); \
    } while (0)
inline int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}
#endif

// TF_ABLATE matches the kernel's name as the launch site spells it; a launch helper that is a template over functors passes a name that carries them
#define TF_LAUNCH(kern, ...) TF_LAUNCH_AS(#kern, kern, __VA_ARGS__)

#define TF_REQUIRE(cond, ...)            \
    do {                                 \
        if (!(cond)) {                   \
            tf::set_error(__VA_ARGS__);  \
            return -1;                   \
        }                                \
    } while (0)

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace tf
