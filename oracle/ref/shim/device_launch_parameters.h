// device_launch_parameters.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/).
// The launch coordinates of the thread a host loop is currently playing; ref_driver.cpp defines them.
#pragma once
#include "cuda_runtime.h"

extern thread_local uint3 threadIdx;
extern thread_local uint3 blockIdx;
extern thread_local dim3 blockDim;
extern thread_local dim3 gridDim;
