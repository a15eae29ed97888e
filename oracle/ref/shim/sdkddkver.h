// sdkddkver.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/). Intentionally empty.
#pragma once
