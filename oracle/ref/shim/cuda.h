// cuda.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/). Everything lives in cuda_runtime.h.
#pragma once
#include "cuda_runtime.h"
