// The camera of the double-precision visual edges: projection and its Jacobian for the Pinhole and the Kannala-Brandt model.  Shared
// by orbba.hip (the edges on a camera-frame VertexSE3) and orbvi.hip (the edges on a body-frame VertexPose), so that both evaluate
// the same expressions in the same order.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

struct BaCam { double fx, fy, cx, cy, delta; int model; double k[4]; };
// camera->project(Pc) (G2oTypes.h:250 through Camera): Pinhole.cpp:28-32, or the Kannala-Brandt model of Fisheye.cpp:35-49
__device__ __forceinline__ void ba_project(const BaCam &cam, double X, double Y, double Z, double *u, double *v)
{
    if (cam.model == 0) {
        *u = cam.fx * (X / Z) + cam.cx;
        *v = cam.fy * (Y / Z) + cam.cy;
        return;
    }
    const double a = X / Z, b = Y / Z;
    const double r = sqrt(a * a + b * b);
    const double theta = atan(r);
    const double theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta2 * theta3, theta7 = theta2 * theta5,
                 theta9 = theta2 * theta7;
    const double theta_d = theta + cam.k[0] * theta3 + cam.k[1] * theta5 + cam.k[2] * theta7 + cam.k[3] * theta9;
    *u = cam.fx * theta_d * a / r + cam.cx; // a point on the optical axis (r = 0) is 0 / 0 here as in the reference
    *v = cam.fy * theta_d * b / r + cam.cy;
}
// camera->getProjJacobian(Pc) (G2oTypes.cpp:42): Pinhole.cpp:49-53 or Fisheye.cpp:83-108; row-major 2 x 3
__device__ __forceinline__ void ba_proj_jacobian(const BaCam &cam, double X, double Y, double Z, double Jp[6])
{
    if (cam.model == 0) {
        Jp[0] = cam.fx / Z; Jp[1] = 0.0; Jp[2] = -cam.fx * X / (Z * Z);
        Jp[3] = 0.0; Jp[4] = cam.fy / Z; Jp[5] = -cam.fy * Y / (Z * Z);
        return;
    }
    const double x2 = X * X, y2 = Y * Y, z2 = Z * Z;
    const double r2 = x2 + y2, r = sqrt(r2), r3 = r2 * r;
    const double theta = atan2(r, Z);
    const double theta2 = theta * theta, theta3 = theta2 * theta, theta4 = theta2 * theta2, theta5 = theta4 * theta,
                 theta6 = theta2 * theta4, theta7 = theta6 * theta, theta8 = theta4 * theta4, theta9 = theta8 * theta;
    const double f = theta + theta3 * cam.k[0] + theta5 * cam.k[1] + theta7 * cam.k[2] + theta9 * cam.k[3];
    const double fd = 1 + 3 * cam.k[0] * theta2 + 5 * cam.k[1] * theta4 + 7 * cam.k[2] * theta6 + 9 * cam.k[3] * theta8;
    Jp[0] = cam.fx * (fd * Z * x2 / (r2 * (r2 + z2)) + f * y2 / r3);
    Jp[3] = cam.fy * (fd * Z * Y * X / (r2 * (r2 + z2)) - f * Y * X / r3);
    Jp[1] = cam.fx * (fd * Z * Y * X / (r2 * (r2 + z2)) - f * Y * X / r3);
    Jp[4] = cam.fy * (fd * Z * y2 / (r2 * (r2 + z2)) + f * x2 / r3);
    Jp[2] = -cam.fx * fd * X / (r2 + z2);
    Jp[5] = -cam.fy * fd * Y / (r2 + z2);
}
