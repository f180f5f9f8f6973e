// What the matcher's other source files need of the handle that orbm_matcher.hip defines.  Internal: not an exported symbol.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbm.h"

// Start of a device entry point on handle `c` that enqueues on `s`: selects the handle's device and notes a NULL-stream call
// (HandleStream::device_call, orb_host.h), so that the stream rule of include/orbx.h holds for every file of the matcher.
__attribute__((visibility("hidden"))) hipError_t orbm_device_call(orbm_t *c, hipStream_t s);

// Start of a host-pointer entry point on handle `c` (HandleStream::host_call), which then stages through the handle: `bytes` of
// device memory and as many of pinned host memory (grow-only, the handle's; one host-pointer call runs per handle at a time) and
// the handle's own stream, on which such a call uploads, computes, downloads and waits.
__attribute__((visibility("hidden"))) hipError_t orbm_host_stage(orbm_t *c, size_t bytes, void **dev, void **pinned, hipStream_t *s);
