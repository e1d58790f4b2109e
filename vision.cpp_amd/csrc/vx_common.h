// Shared helpers of the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/visp_hip_kernels.h"

void vx_set_error(const char* fmt, ...);

#define VX_CHECK(expr)                                                                     \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            vx_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return 0;                                                                      \
        }                                                                                  \
    } while (0)

#define VX_REQUIRE(cond, ...)                 \
    do {                                      \
        if (!(cond)) {                        \
            vx_set_error(__VA_ARGS__);        \
            return 0;                         \
        }                                     \
    } while (0)

#define VX_LAUNCH_CHECK() VX_CHECK(hipGetLastError())

typedef _Float16 f16;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute: set it once per (kernel, device), not once per process
hipError_t vx_ensure_dynamic_lds(const void* kernel, int bytes);

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// ---- host launch helpers: grid sizes of the one-thread-per-item kernels
// one block per per_block items, every item gets a thread
inline unsigned blocks_for(long items, int per_block = 256) { return (unsigned)((items + per_block - 1) / per_block); }
// the same for a grid-stride kernel: at least one block, at most cap blocks (the kernel's loop covers the rest)
inline int grid_stride_blocks(long items, int cap, int per_block = 256) {
    const long b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#include "vx_device.h"
