// Device functions of the camera models that more than one of the matcher's source files evaluates (orbm_project.hip,
// orbm_triangulate.hip).  Float, no fused multiply-add; `/` and sqrtf are the correctly rounded ones.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/orbm.h"

#pragma clang fp contract(off)

namespace {

// camera->project(Pc): Pinhole.cpp:34-38 / Fisheye.cpp:52-66
__device__ __forceinline__ void project(const orbm_proj_camera &c, float X, float Y, float Z, float &u, float &v)
{
    const float a = X / Z, b = Y / Z;
    if (c.model == 0) {
        u = c.fx * a + c.cx;
        v = c.fy * b + c.cy;
    } else {
        const float r = sqrtf(a * a + b * b);
        const float theta = atanf(r);
        const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta2 * theta3, theta7 = theta2 * theta5,
                    theta9 = theta2 * theta7;
        const float theta_d = (((theta + c.k[0] * theta3) + c.k[1] * theta5) + c.k[2] * theta7) + c.k[3] * theta9;
        u = ((c.fx * theta_d) * a) / r + c.cx;
        v = ((c.fy * theta_d) * b) / r + c.cy;
    }
}

} // namespace
