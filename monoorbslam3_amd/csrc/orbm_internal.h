// What the matcher's other source files need of the handle that orbm_matcher.hip defines.  Internal: not an exported symbol.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbm.h"

// Start of a device entry point on handle `c` that enqueues on `s`: selects the handle's device and notes a NULL-stream call
// (HandleStream::device_call, orb_host.h), so that the stream rule of include/orbx.h holds for every file of the matcher.
__attribute__((visibility("hidden"))) hipError_t orbm_device_call(orbm_t *c, hipStream_t s);
