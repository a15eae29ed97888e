// cuda_runtime.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/, see build_ref.py).
//
// Lets the reference engine's translation units compile as plain host C++: the CUDA function-space
// qualifiers are empty, the launch types are plain structs, and device memory is host memory. Only API
// names appear here; no reference code.
//
// Floating-point flavours: with REF_FLAVOUR_B defined, the six single-precision
// transcendentals the reference calls are redirected to this project's csrc/iq_fp.h — the same
// redirection IQO_GLIBC_LIBM switches off in oracle/iqpt_oracle.c. Without it they are glibc's (flavour A).
#pragma once

// every standard header that declares the redirected names comes first, so the macros below only touch
// the reference's own calls
#include <cmath>
#include <math.h>
#include <complex>
#include <random>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#define __host__
#define __device__
#define __global__
#define __shared__

struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    constexpr dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

// the reference's headers call these unqualified (a CUDA toolchain puts them in the global namespace)
using std::isinf;
using std::isnan;

enum cudaError { cudaSuccess = 0, cudaErrorMemoryAllocation = 2 };
typedef cudaError cudaError_t;
enum cudaMemcpyKind { cudaMemcpyHostToHost = 0, cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2,
                      cudaMemcpyDeviceToDevice = 3, cudaMemcpyDefault = 4 };

inline cudaError cudaMalloc(void** p, size_t bytes) {
    *p = std::malloc(bytes ? bytes : 1);
    return *p ? cudaSuccess : cudaErrorMemoryAllocation;
}
template <typename T> inline cudaError cudaMalloc(T** p, size_t bytes) { return cudaMalloc((void**)p, bytes); }
template <typename T> inline cudaError cudaMallocManaged(T** p, size_t bytes, unsigned int = 1) {
    return cudaMalloc((void**)p, bytes);
}
inline cudaError cudaMemcpy(void* dst, const void* src, size_t bytes, cudaMemcpyKind) {
    std::memcpy(dst, src, bytes);
    return cudaSuccess;
}
inline cudaError cudaMemset(void* dst, int value, size_t bytes) {
    std::memset(dst, value, bytes);
    return cudaSuccess;
}
inline cudaError cudaFree(void* p) {
    std::free(p);
    return cudaSuccess;
}
inline cudaError cudaDeviceSynchronize() { return cudaSuccess; }
inline cudaError cudaDeviceReset() { return cudaSuccess; }
inline cudaError cudaGetLastError() { return cudaSuccess; }
inline const char* cudaGetErrorName(cudaError e) { return e == cudaSuccess ? "cudaSuccess" : "cudaError"; }
inline const char* cudaGetErrorString(cudaError e) { return e == cudaSuccess ? "no error" : "host allocation failed"; }

#ifdef REF_FLAVOUR_B
#include "iq_fp.h"
#define sinf iq_sinf
#define cosf iq_cosf
#define tanf iq_tanf
#define acosf iq_acosf
#define asinf iq_asinf
#define atan2f iq_atan2f
#endif
