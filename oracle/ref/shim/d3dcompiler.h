// d3dcompiler.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/). Nothing the host loop uses.
#pragma once
#include "d3d11.h"
