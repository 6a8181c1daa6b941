// pc_image_host.h -- the host plumbing every image-side library has: the last HIP error, HIPCHK, cdiv and the alignment helpers.
// Header only and included by exactly one translation unit per library, so `static` and the unnamed namespace give every library
// its own copy: no library links another, and g_last_hip is per library.  Each library keeps its own *_strerror (the messages
// differ) and its own *_last_hip_error (the exported name differs).
#ifndef PC_IMAGE_HOST_H
#define PC_IMAGE_HOST_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "pcodec.h"

static std::atomic<int> g_last_hip{0};
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { g_last_hip = (int)_e; return PC_ERR_HIP; } } while (0)

namespace {

typedef unsigned long long u64;

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline bool mult4(int64_t v) { return v % 4 == 0; }

// p is aligned to n bytes
inline bool aligned(const void* p, int n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// a float32 pointer and three strides in elements as the wide path needs them: 128-bit accesses
inline bool f32_wide(const void* p, int64_t s0, int64_t s1, int64_t s2) { return aligned(p, 16) && mult4(s0) && mult4(s1) && mult4(s2); }

}  // namespace

#endif  // PC_IMAGE_HOST_H
