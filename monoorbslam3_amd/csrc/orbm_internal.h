// What the matcher's other source files need of the handle that orbm_matcher.hip defines.  Internal: not an exported symbol.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbm.h"
#include "orb_host.h"

// Start of a device entry point on handle `c` that enqueues on `s`: selects the handle's device and notes a NULL-stream call
// (HandleStream::device_call, orb_host.h), so that the stream rule of include/orbx.h holds for every file of the matcher.
__attribute__((visibility("hidden"))) hipError_t orbm_device_call(orbm_t *c, hipStream_t s);

// Start of a host-pointer entry point on handle `c` (HandleStream::host_call), which then stages through the handle: `bytes` of
// device memory and as many of pinned host memory (grow-only, the handle's; one host-pointer call runs per handle at a time) and
// the handle's own stream, on which such a call uploads, computes, downloads and waits.
__attribute__((visibility("hidden"))) hipError_t orbm_host_stage(orbm_t *c, size_t bytes, void **dev, void **pinned, hipStream_t *s);

// The scratch of the two-view RANSAC (orbm_two_view.hip): `bytes` of device memory of the handle's own, grow-only, apart from the
// blocks the searches use, so that a search and the RANSAC behind it on one stream share nothing.  One call in flight per handle.
__attribute__((visibility("hidden"))) hipError_t orbm_two_view_scratch(orbm_t *c, size_t bytes, void **dev);
// The same for the pose recovery behind it (orbm_two_view_pose.hip), a block of its own: growing it never frees what the RANSAC ahead of
// it on the stream still reads.
__attribute__((visibility("hidden"))) hipError_t orbm_two_view_pose_scratch(orbm_t *c, size_t bytes, void **dev);

// ---- what the map-side device entry points share (orbm_project / triangulate / refresh / observations) -------------------------
constexpr int ORBM_MAX_POINTS = 1 << 19;   // map points per call: k_project's frustum form and k_cull keep one bit per point in 64 KB of LDS
constexpr int ORBM_MAX_LIST = 1024;        // observations per list (MEDOID_MAX of k_medoid): the refresh leaves longer lists untouched
static inline int orbm_check_points(int n) { return n > ORBM_MAX_POINTS ? orbx_set_error(ORBX_E_UNSUPPORTED, "more than 524288 map points in one call") : ORBX_OK; }
static inline int orbm_check_stride(int n) { return n > ORBM_MEDIAN_MAX_STRIDE ? orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_MEDIAN_MAX_STRIDE (8192) slots per key frame") : ORBX_OK; }
static inline int orbm_check_camera(const orbm_proj_camera *cam) { return cam->model != 0 && cam->model != 1 ? orbx_set_error(ORBX_E_ARG, "camera model must be 0 (Pinhole) or 1 (Fisheye)") : ORBX_OK; }
static inline int orbm_check_kf_rows(const void *kps, const void *desc = nullptr) { return ((((uintptr_t)kps) | ((uintptr_t)desc)) & (sizeof(void *) - 1)) ? orbx_set_error(ORBX_E_ARG, "the key-frame table's pointer arrays must be pointer aligned") : ORBX_OK; }

// Start of a device entry point, behind its argument checks (an argument error is reported before the device is looked for): a
// device, a handle, the point limit (n_points: the projection entries), the handle's device selected; *out = the stream to enqueue on
static inline int orbm_begin_device(orbm_t *h, void *stream, hipStream_t *out, int n_points = 0)
{
    if (int rc = orb_need_device()) return rc;
    if (!h) return orbx_set_error(ORBX_E_ARG, "null handle");
    if (int rc = orbm_check_points(n_points)) return rc;
    hipStream_t s = (hipStream_t)stream; // NULL is stream 0 itself (include/orbx.h, "Streams")
    ORB_TRY(orbm_device_call(h, s));
    *out = s;
    return ORBX_OK;
}
