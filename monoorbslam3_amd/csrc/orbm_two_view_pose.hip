// The pose recovery of the two-view initialisation on the device (include/orbm.h, "Two-view initialisation: the pose and the points"):
// what TwoViewReconstruction::Reconstruct does behind the RH decision, and the tail in which the tracker consumes it.
//   orbm_two_view_pose_device   TwoViewReconstruction.cpp:79-83 (dispatch), :346-475 (ReconstructH), :477-556 (ReconstructF), :598-687
//                               (CheckRT), :689-705 (Triangulate), :707-724 (DecomposeE), Tracking.cpp:622-627
//   orbm_two_view_pose          the same with host pointers: one pinned copy each way on the handle's stream
//   orbm_two_view_decide        the decision rules of :353, :440-471, :484, :510-552 on the host, the code the device runs
//
// Three launches on the caller's stream, nothing between them:
//   k_tvp_decompose  ONE lane: E = K^T F K or A = K^-1 H K, the 3 x 3 one-sided Jacobi, the four or eight (R, t), all in DOUBLE on the
//                    float inputs, rounded to float once per hypothesis
//   k_tvp_check      ONE workgroup of 1024 per hypothesis: CheckRT in float, threads striding over the match list; nGood and nInlier by
//                    wave popcounts added in LDS; the cosine of rank min(50, nGood - 1) by a radix select (four 8-bit digits of the
//                    order-preserving integer image of the float, a 256-bin histogram in LDS per digit)
//   k_tvp_decide     ONE workgroup of 1024: the decision, then the winner walked AGAIN for d_points3D / d_triangulated -- the same
//                    arithmetic on the same inputs, bit for bit the same gates, as orbm_triangulate.hip's second walk -- and d_matches12_out
//
// CheckRT's evaluation orders are the header's (float; no fused multiply-add: the build passes -ffp-contract=off and the pragma below
// repeats it; `/` and sqrtf are the correctly rounded ones).  The 4 x 4 solve of Triangulate is orbm_jacobi.h's, the one
// orbm_triangulate.hip runs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_jacobi.h"

#pragma clang fp contract(off)

namespace {

constexpr int TP_T = 1024;            // threads of k_tvp_check and k_tvp_decide
constexpr int TP_WAVES = TP_T / 64;
constexpr int TP_SWEEPS3 = 8;         // the 3 x 3 in double: at its floor after 4 sweeps on the RANSAC's rank-2 step; 8 are run
constexpr int TP_HYP = 8;
constexpr unsigned TP_NO_KEY = 0xffffffffu;   // a match that is not good has no cosine

// head, handle scratch, int32 x 8: [0] 0 go on, 1 the RANSAC refused, 2 H degenerate; [1] family (0 F, 1 H); [2] hypotheses; [3] n_matches
// kept inside 0 .. n1; [4] nInlier (k_tvp_check's workgroup 0)
enum { HEAD_STATUS = 0, HEAD_FAMILY = 1, HEAD_HYP = 2, HEAD_MATCHES = 3, HEAD_INLIERS = 4 };

// d_hyp_code: where a key point of frame 1 left CheckRT (:628-676)
enum { C_NO_MATCH = 0, C_NOT_INLIER = 1, C_NOT_FINITE = 2, C_BEHIND_1 = 3, C_BEHIND_2 = 4, C_ERROR_1 = 5, C_ERROR_2 = 6, C_GOOD = 7, C_GOOD_NO_PARALLAX = 8 };

struct TvpCam { float fx, fy, cx, cy; };

// ---- the decision: :353, :440-471 (H) and :484, :510-552 (F) ------------------------------------------------------------------------
// returns the status (0 accepted, 3 no clear winner or too few good, 4 parallax too low); winner is -1 unless accepted
__host__ __device__ __forceinline__ int tvp_decide(int family, const int (&good)[TP_HYP], const float (&par)[TP_HYP], int n_inlier, float min_parallax,
                                                   int &winner, int &min_good)
{
    winner = -1;
    if (family) {
        const int r = (int)rint(0.6 * (double)n_inlier);   // cvRound: to nearest, ties to even
        min_good = r < 100 ? r : 100;
        int best = 0, second = -1, idx = -1;
        float best_par = -1.f;
#pragma unroll
        for (int k = 0; k < TP_HYP; ++k) {
            if (good[k] > best) second = best, best = good[k], idx = k, best_par = par[k];
            else if (good[k] > second) second = good[k];
        }
        const bool clear = (double)second < 0.75 * (double)best && best > min_good;
        if (clear && best_par >= min_parallax) {
            winner = idx;
            return 0;
        }
        return clear ? 4 : 3;
    }
    const int f = (int)floor(0.6 * (double)n_inlier);      // cvFloor
    min_good = f < 100 ? f : 100;
    int max_good = good[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) max_good = good[k] > max_good ? good[k] : max_good;
    const int good_th = (int)floor(0.7 * (double)max_good);
    int similar = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) similar += good[k] > good_th ? 1 : 0;
    if (max_good < min_good || similar > 1) return 3;
    // the cascade of :524-552: the first hypothesis that reaches the maximum, and no other, is asked for its parallax
    const int idx = max_good == good[0] ? 0 : max_good == good[1] ? 1 : max_good == good[2] ? 2 : 3;
    const float p = idx == 0 ? par[0] : idx == 1 ? par[1] : idx == 2 ? par[2] : par[3];
    if (p > min_parallax) {
        winner = idx;
        return 0;
    }
    return 4;
}

// ---- the decomposition, double --------------------------------------------------------------------------------------------------------
// row-major 3 x 3 products, a row times a column as (p0 + p1) + p2
__device__ __forceinline__ void mul3(const double (&a)[9], const double (&b)[9], double (&o)[9])
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
}
__device__ __forceinline__ double det3(const double (&m)[9])
{
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ __forceinline__ void swap_cols(bool on, double &na, double &nb, double (&a)[3], double (&b)[3], double (&va)[3], double (&vb)[3])
{
    const double t = na;
    na = on ? nb : na, nb = on ? t : nb;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double x = a[r], y = va[r];
        a[r] = on ? b[r] : a[r], b[r] = on ? x : b[r];
        va[r] = on ? vb[r] : va[r], vb[r] = on ? y : vb[r];
    }
}
// m (row-major) = U diag(w) V^T, w descending; U and Vt row-major.  U's last column is B's column over its norm where `full_u` and the
// norm is not 0, u0 x u1 otherwise: the left null vector of a rank-2 E, which a one-sided Jacobi leaves as a zero column
__device__ __forceinline__ void svd3(const double (&m)[9], bool full_u, double (&U)[9], double (&w)[3], double (&Vt)[9])
{
    double B[3][3], V[3][3];   // by column
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) B[c][r] = m[3 * r + c], V[c][r] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < TP_SWEEPS3; ++sweep) {
        rotate3(B[0], B[1], V[0], V[1]);
        rotate3(B[0], B[2], V[0], V[2]);
        rotate3(B[1], B[2], V[1], V[2]);
    }
    double n0 = sqrt(dot3(B[0], B[0])), n1 = sqrt(dot3(B[1], B[1])), n2 = sqrt(dot3(B[2], B[2]));
    swap_cols(n0 < n1, n0, n1, B[0], B[1], V[0], V[1]);
    swap_cols(n1 < n2, n1, n2, B[1], B[2], V[1], V[2]);
    swap_cols(n0 < n1, n0, n1, B[0], B[1], V[0], V[1]);
    w[0] = n0, w[1] = n1, w[2] = n2;
    double u0[3], u1[3], u2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) u0[r] = B[0][r] / n0, u1[r] = B[1][r] / n1;
    const bool own = full_u && n2 > 0.0;
    u2[0] = own ? B[2][0] / n2 : u0[1] * u1[2] - u0[2] * u1[1];
    u2[1] = own ? B[2][1] / n2 : u0[2] * u1[0] - u0[0] * u1[2];
    u2[2] = own ? B[2][2] / n2 : u0[0] * u1[1] - u0[1] * u1[0];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        U[3 * r] = u0[r], U[3 * r + 1] = u1[r], U[3 * r + 2] = u2[r];
        Vt[r] = V[0][r], Vt[3 + r] = V[1][r], Vt[6 + r] = V[2][r];
    }
}
// one hypothesis rounded to float: R, and t over its norm
__device__ __forceinline__ void put_hyp(float *__restrict__ hyp_R, float *__restrict__ hyp_t, int k, const double (&R)[9], double sign, const double (&t)[3])
{
    const double norm = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
    for (int j = 0; j < 9; ++j) hyp_R[9 * k + j] = (float)R[j];
#pragma unroll
    for (int j = 0; j < 3; ++j) hyp_t[3 * k + j] = (float)(sign * (t[j] / norm));
}

__global__ __launch_bounds__(64) void k_tvp_decompose(const TvpCam cam, const float *__restrict__ in_H, const float *__restrict__ in_F,
                                                      const int32_t *__restrict__ ransac_result, int family, int n1, int32_t *__restrict__ head,
                                                      float *__restrict__ hyp_R, float *__restrict__ hyp_t)
{
    if (threadIdx.x != 0) return;
    const int fam = family < 0 ? (ransac_result[4] != 0 ? 1 : 0) : family;
    const int n = min(max(ransac_result[0], 0), n1);   // whatever the caller's d_ransac_result holds, the walks stay inside the arrays
    head[HEAD_FAMILY] = fam, head[HEAD_MATCHES] = n, head[HEAD_INLIERS] = 0;
    if (ransac_result[1] != 0) {                       // the RANSAC refused: only d_result will be written
        head[HEAD_STATUS] = 1, head[HEAD_HYP] = 0;
        return;
    }
    const double fx = (double)cam.fx, fy = (double)cam.fy, cx = (double)cam.cx, cy = (double)cam.cy;
    const double K[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
    double M[9], L[9], T[9], A[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) M[j] = (double)(fam ? in_H[j] : in_F[j]);
    if (fam) {   // invK, closed form (:360)
        L[0] = 1.0 / fx, L[1] = 0.0, L[2] = -cx / fx, L[3] = 0.0, L[4] = 1.0 / fy, L[5] = -cy / fy, L[6] = 0.0, L[7] = 0.0, L[8] = 1.0;
    } else {     // K^T (:490)
        L[0] = fx, L[1] = 0.0, L[2] = 0.0, L[3] = 0.0, L[4] = fy, L[5] = 0.0, L[6] = cx, L[7] = cy, L[8] = 1.0;
    }
    mul3(L, M, T);
    mul3(T, K, A);
    double U[9], w[3], Vt[9];
    svd3(A, fam != 0, U, w, Vt);
    int n_hyp = 0, status = 0;
    if (!fam) {   // DecomposeE (:707-724) and the four pairs of :505-508
        const double W[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0}, Wt[9] = {0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
        const double t[3] = {U[2], U[5], U[8]};
        double X[9], R1[9], R2[9];
        mul3(U, W, X);
        mul3(X, Vt, R1);
        mul3(U, Wt, X);
        mul3(X, Vt, R2);
        const double s1 = det3(R1) < 0.0 ? -1.0 : 1.0, s2 = det3(R2) < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) R1[j] = s1 * R1[j], R2[j] = s2 * R2[j];
        put_hyp(hyp_R, hyp_t, 0, R1, 1.0, t);
        put_hyp(hyp_R, hyp_t, 1, R2, 1.0, t);
        put_hyp(hyp_R, hyp_t, 2, R1, -1.0, t);
        put_hyp(hyp_R, hyp_t, 3, R2, -1.0, t);
        n_hyp = 4;
    } else {      // Faugeras (:368-436), the eight in the order they are computed
        const double s = det3(U) * det3(Vt);
        const double d1 = w[0], d2 = w[1], d3 = w[2];
        if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) {
            status = 2;
        } else {
            const double aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
            const double root = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3));
            const double s_theta = root / ((d1 + d3) * d2), c_theta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
            const double s_phi = root / ((d1 - d3) * d2), c_phi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
                const double sign = (i == 0 || i == 3) ? 1.0 : -1.0;   // s_theta[], s_phi[] = {+, -, -, +}
                double Rp[9], X[9], R[9], tp[3], t[3];
                // d' = d2
                const double st = sign * s_theta;
                Rp[0] = c_theta, Rp[1] = 0.0, Rp[2] = -st, Rp[3] = 0.0, Rp[4] = 1.0, Rp[5] = 0.0, Rp[6] = st, Rp[7] = 0.0, Rp[8] = c_theta;
                mul3(U, Rp, X);
                mul3(X, Vt, R);
#pragma unroll
                for (int j = 0; j < 9; ++j) R[j] = s * R[j];
                tp[0] = x1 * (d1 - d3), tp[1] = 0.0, tp[2] = -x3 * (d1 - d3);
#pragma unroll
                for (int r = 0; r < 3; ++r) t[r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
                put_hyp(hyp_R, hyp_t, i, R, 1.0, t);
                // d' = -d2
                const double sp = sign * s_phi;
                Rp[0] = c_phi, Rp[1] = 0.0, Rp[2] = sp, Rp[3] = 0.0, Rp[4] = -1.0, Rp[5] = 0.0, Rp[6] = sp, Rp[7] = 0.0, Rp[8] = -c_phi;
                mul3(U, Rp, X);
                mul3(X, Vt, R);
#pragma unroll
                for (int j = 0; j < 9; ++j) R[j] = s * R[j];
                tp[0] = x1 * (d1 + d3), tp[1] = 0.0, tp[2] = x3 * (d1 + d3);
#pragma unroll
                for (int r = 0; r < 3; ++r) t[r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
                put_hyp(hyp_R, hyp_t, 4 + i, R, 1.0, t);
            }
            n_hyp = 8;
        }
    }
    for (int k = n_hyp; k < TP_HYP; ++k) {   // the rows no hypothesis fills
        for (int j = 0; j < 9; ++j) hyp_R[9 * k + j] = 0.f;
        for (int j = 0; j < 3; ++j) hyp_t[3 * k + j] = 0.f;
    }
    head[HEAD_STATUS] = status, head[HEAD_HYP] = n_hyp;
}

// ---- CheckRT, float --------------------------------------------------------------------------------------------------------------------
struct TvpPose {
    float R[9], t[3], P2[12], O2[3];
};

// :611-624: P2 = K * [R | t] and O2 = -R^T * t, a row times a column as (p0 + p1) + p2
__device__ __forceinline__ void load_pose(const TvpCam &cam, const float *__restrict__ hyp_R, const float *__restrict__ hyp_t, int k, TvpPose &p)
{
#pragma unroll
    for (int j = 0; j < 9; ++j) p.R[j] = hyp_R[9 * k + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) p.t[j] = hyp_t[3 * k + j];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float a = c < 3 ? p.R[c] : p.t[0], b = c < 3 ? p.R[3 + c] : p.t[1], d = c < 3 ? p.R[6 + c] : p.t[2];
        p.P2[c] = (cam.fx * a + 0.f * b) + cam.cx * d;
        p.P2[4 + c] = (0.f * a + cam.fy * b) + cam.cy * d;
        p.P2[8 + c] = (0.f * a + 0.f * b) + 1.f * d;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) p.O2[c] = ((-p.R[c]) * p.t[0] + (-p.R[3 + c]) * p.t[1]) + (-p.R[6 + c]) * p.t[2];
}

// Eigen's normalize(): v /= sqrt(v . v) where v . v > 0
__device__ __forceinline__ void normalize3(float &x, float &y, float &z)
{
    const float n2 = (x * x + y * y) + z * z;
    if (n2 > 0.f) {
        const float n = sqrtf(n2);
        x = x / n, y = y / n, z = z / n;
    }
}

// :630-676 for one inlier match; returns the code, Pc1 and cosParallax
__device__ __forceinline__ int check_one(const TvpCam &cam, const TvpPose &p, float th2, float x1, float y1, float x2, float y2, float (&pc)[3], float &cos_par)
{
    // Triangulate (:692-696), A by column; P1 = K [I | 0]
    const float P1[12] = {cam.fx, 0.f, cam.cx, 0.f, 0.f, cam.fy, cam.cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    float A[4][4], V[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        A[k][0] = x1 * P1[8 + k] - P1[k];
        A[k][1] = y1 * P1[8 + k] - P1[4 + k];
        A[k][2] = x2 * p.P2[8 + k] - p.P2[k];
        A[k][3] = y2 * p.P2[8 + k] - p.P2[4 + k];
#pragma unroll
        for (int r = 0; r < 4; ++r) V[k][r] = r == k ? 1.f : 0.f;
    }
    for (int sweep = 0; sweep < TR_SWEEPS; ++sweep) {
        rotate(A[0], A[1], V[0], V[1]);
        rotate(A[0], A[2], V[0], V[2]);
        rotate(A[0], A[3], V[0], V[3]);
        rotate(A[1], A[2], V[1], V[2]);
        rotate(A[1], A[3], V[1], V[3]);
        rotate(A[2], A[3], V[2], V[3]);
    }
    float best = dot4(A[0], A[0]);
    float ph[4] = {V[0][0], V[0][1], V[0][2], V[0][3]};
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const float nk = dot4(A[k], A[k]);
        const bool take = nk < best;
        best = take ? nk : best;
#pragma unroll
        for (int r = 0; r < 4; ++r) ph[r] = take ? V[k][r] : ph[r];
    }
    // :703 without :700: Ph(3) == 0 divides, and the gate of :636 drops the match
    const float x = ph[0] / ph[3], y = ph[1] / ph[3], z = ph[2] / ph[3];
    pc[0] = x, pc[1] = y, pc[2] = z;
    cos_par = 0.f;
    if (!isfinite(x) || !isfinite(y) || !isfinite(z)) return C_NOT_FINITE;
    float ax = x - 0.f, ay = y - 0.f, az = z - 0.f;   // Pc1 - O1
    normalize3(ax, ay, az);
    float bx = x - p.O2[0], by = y - p.O2[1], bz = z - p.O2[2];
    normalize3(bx, by, bz);
    cos_par = (ax * bx + ay * by) + az * bz;
    const bool parallax = (double)cos_par < 0.99998;   // float against a double literal
    if (z <= 0.f && parallax) return C_BEHIND_1;
    const float x_2 = ((p.R[0] * x + p.R[1] * y) + p.R[2] * z) + p.t[0], y_2 = ((p.R[3] * x + p.R[4] * y) + p.R[5] * z) + p.t[1];
    const float z_2 = ((p.R[6] * x + p.R[7] * y) + p.R[8] * z) + p.t[2];
    if (z_2 <= 0.f && parallax) return C_BEHIND_2;
    const float inv_z1 = 1.f / z;
    const float u1 = (cam.fx * x) * inv_z1 + cam.cx, v1 = (cam.fy * y) * inv_z1 + cam.cy;
    const float e1 = (x1 - u1) * (x1 - u1) + (y1 - v1) * (y1 - v1);
    if (e1 > th2) return C_ERROR_1;
    const float inv_z2 = 1.f / z_2;
    const float u2 = (cam.fx * x_2) * inv_z2 + cam.cx, v2 = (cam.fy * y_2) * inv_z2 + cam.cy;
    const float e2 = (x2 - u2) * (x2 - u2) + (y2 - v2) * (y2 - v2);
    if (e2 > th2) return C_ERROR_2;
    return parallax ? C_GOOD : C_GOOD_NO_PARALLAX;
}

// the unsigned whose order is the float's
__device__ __forceinline__ unsigned float_key(float v)
{
    const unsigned u = __float_as_uint(v);
    const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return k == TP_NO_KEY ? TP_NO_KEY - 1u : k;
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(TP_T) void k_tvp_check(const TvpCam cam, const orbx_kp *__restrict__ kps1, int n1, const orbx_kp *__restrict__ kps2, int n2,
                                                    const int32_t *__restrict__ pairs, const uint8_t *__restrict__ inl_H,
                                                    const uint8_t *__restrict__ inl_F, float th2, int32_t *head, const float *__restrict__ hyp_R,
                                                    const float *__restrict__ hyp_t, unsigned *__restrict__ keys, int32_t *__restrict__ hyp_good,
                                                    float *__restrict__ hyp_parallax, uint8_t *hyp_code)
{
    __shared__ int s_count[2];
    __shared__ int s_hist[256];
    __shared__ int s_wave[TP_WAVES];
    __shared__ int s_sel[2];
    const int tid = threadIdx.x, h = blockIdx.x;
    if (head[HEAD_STATUS] == 1) return;   // uniform: the RANSAC refused, nothing is written
    const int n_hyp = head[HEAD_HYP], n = head[HEAD_MATCHES];
    const uint8_t *__restrict__ inl = head[HEAD_FAMILY] ? inl_H : inl_F;
    const bool live = h < n_hyp;
    uint8_t *code = hyp_code ? hyp_code + (size_t)h * n1 : nullptr;
    if (code)
        for (int i = tid; i < n1; i += TP_T) code[i] = C_NO_MATCH;
    if (!live && h != 0) {   // a row no hypothesis fills; workgroup 0 still counts the inliers
        if (tid == 0) hyp_good[h] = 0, hyp_parallax[h] = 0.f;
        return;
    }
    if (tid < 2) s_count[tid] = 0;
    __syncthreads();          // the row of codes is zeroed before a match writes its own
    TvpPose pose;
    load_pose(cam, hyp_R, hyp_t, live ? h : 0, pose);
    unsigned *__restrict__ row = keys + (size_t)h * n1;
    int count[2] = {0, 0};    // inliers, good
    for (int k = tid; k < n; k += TP_T) {
        const int i = pairs[2 * k], m = pairs[2 * k + 1];
        const bool in = i >= 0 && i < n1 && m >= 0 && m < n2;
        unsigned key = TP_NO_KEY;
        if (in) {
            int c = C_NOT_INLIER;
            if (inl[k]) {
                count[0] += 1;
                if (live) {
                    float pc[3], cos_par;
                    c = check_one(cam, pose, th2, kps1[i].x, kps1[i].y, kps2[m].x, kps2[m].y, pc, cos_par);
                    if (c >= C_GOOD) count[1] += 1, key = float_key(cos_par);
                }
            }
            if (code && live) code[i] = (uint8_t)c;
        }
        row[k] = key;
    }
    block_add(s_count, {0, 1}, count);
    __syncthreads();
    const int n_good = s_count[1];
    if (h == 0 && tid == 0) head[HEAD_INLIERS] = s_count[0];
    if (!live) {              // uniform: workgroup 0 of a call without hypotheses
        if (tid == 0) hyp_good[h] = 0, hyp_parallax[h] = 0.f;
        return;
    }
    if (tid == 0) hyp_good[h] = n_good;
    if (n_good == 0) {        // :683
        if (tid == 0) hyp_parallax[h] = 0.f;
        return;
    }
    // :680-682: the element of rank min(50, nGood - 1) in ascending order, most significant digit first
    int rank = n_good - 1 < 50 ? n_good - 1 : 50;
    unsigned prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned above = pass ? 0xffffffffu << (shift + 8) : 0u;   // the digits already chosen
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        for (int k = tid; k < n; k += TP_T) {
            const unsigned key = row[k];
            if (key != TP_NO_KEY && (key & above) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        const int v = tid < 256 ? s_hist[tid] : 0;
        int total;
        const int before = block_scan<TP_WAVES>(v, s_wave, total);
        if (tid < 256 && before <= rank && rank < before + v) s_sel[0] = tid, s_sel[1] = rank - before;
        __syncthreads();
        prefix |= (unsigned)s_sel[0] << shift;
        rank = s_sel[1];
    }
    if (tid == 0) hyp_parallax[h] = (acosf(key_float(prefix)) * 180.f) / 3.14159274f;   // acosf(c) * 180 / M_PIf32
}

__global__ __launch_bounds__(TP_T) void k_tvp_decide(const TvpCam cam, const orbx_kp *__restrict__ kps1, int n1, const orbx_kp *__restrict__ kps2, int n2,
                                                     const int32_t *__restrict__ pairs, const uint8_t *__restrict__ inl_H,
                                                     const uint8_t *__restrict__ inl_F, const int32_t *__restrict__ matches12, float th2,
                                                     float min_parallax, const int32_t *__restrict__ head, const float *__restrict__ hyp_R,
                                                     const float *__restrict__ hyp_t, const int32_t *__restrict__ hyp_good,
                                                     const float *__restrict__ hyp_parallax, float *__restrict__ R21, float *__restrict__ t21,
                                                     float *points3D, uint8_t *triangulated, int32_t *__restrict__ matches12_out,
                                                     int32_t *__restrict__ result)
{
    __shared__ int s_count[2];
    const int tid = threadIdx.x;
    const int fam = head[HEAD_FAMILY];
    if (head[HEAD_STATUS] == 1) {   // uniform
        if (tid < 16) result[tid] = tid == 0 ? 1 : tid == 1 ? fam : tid == 3 ? -1 : 0;
        return;
    }
    const int n = head[HEAD_MATCHES], n_inlier = head[HEAD_INLIERS];
    int good[TP_HYP];
    float par[TP_HYP];
#pragma unroll
    for (int k = 0; k < TP_HYP; ++k) good[k] = hyp_good[k], par[k] = hyp_parallax[k];
    int winner, min_good;
    int status = tvp_decide(fam, good, par, n_inlier, min_parallax, winner, min_good);
    if (head[HEAD_STATUS] == 2) status = 2, winner = -1;
    if (tid < 2) s_count[tid] = 0;
    for (int i = tid; i < n1; i += TP_T) {
        points3D[3 * i] = 0.f, points3D[3 * i + 1] = 0.f, points3D[3 * i + 2] = 0.f;
        triangulated[i] = 0;
    }
    if (tid < 12) {
        const float v = winner >= 0 ? (tid < 9 ? hyp_R[9 * winner + tid] : hyp_t[3 * winner + tid - 9]) : 0.f;
        if (tid < 9) R21[tid] = v; else t21[tid - 9] = v;
    }
    __syncthreads();
    int count[2] = {0, 0};   // triangulated, matches left
    if (winner >= 0) {       // uniform: the winner's walk again, the same gates bit for bit
        const uint8_t *__restrict__ inl = fam ? inl_H : inl_F;
        TvpPose pose;
        load_pose(cam, hyp_R, hyp_t, winner, pose);
        for (int k = tid; k < n; k += TP_T) {
            const int i = pairs[2 * k], m = pairs[2 * k + 1];
            if (i < 0 || i >= n1 || m < 0 || m >= n2 || !inl[k]) continue;
            float pc[3], cos_par;
            const int c = check_one(cam, pose, th2, kps1[i].x, kps1[i].y, kps2[m].x, kps2[m].y, pc, cos_par);
            if (c >= C_GOOD) points3D[3 * i] = pc[0], points3D[3 * i + 1] = pc[1], points3D[3 * i + 2] = pc[2];   // :672
            if (c == C_GOOD) triangulated[i] = 1, count[0] += 1;                                                  // :675
        }
    }
    __syncthreads();
    for (int i = tid; i < n1; i += TP_T) {   // Tracking.cpp:622-627
        const int m = matches12[i];
        const int out = winner >= 0 && m >= 0 && !triangulated[i] ? -1 : m;
        matches12_out[i] = out;
        count[1] += out >= 0 && out < n2 ? 1 : 0;
    }
    block_add(s_count, {0, 1}, count);
    __syncthreads();
    if (tid < 16) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < TP_HYP; ++k) v = tid == 8 + k ? good[k] : v;
        v = tid == 0 ? status : tid == 1 ? fam : tid == 2 ? head[HEAD_HYP] : tid == 3 ? winner : tid == 4 ? n_inlier : tid == 5 ? min_good : v;
        v = tid == 6 ? s_count[0] : tid == 7 ? s_count[1] : v;
        result[tid] = v;
    }
}

struct TvpScratch {
    int32_t *head;
    unsigned *keys;
    size_t total;
    void lay(void *block, int n1)
    {
        head = (int32_t *)block;
        keys = (unsigned *)((char *)block + 32);
        total = 32 + (size_t)TP_HYP * n1 * 4;
    }
};

int check(float fx, float fy, const void *kps1, int n1, const void *kps2, int n2, const void *matches12, const void *pairs, const void *H,
          const void *F, const void *inl_H, const void *inl_F, const void *ransac_result, int family, float sigma, const void *R21,
          const void *t21, const void *points3D, const void *triangulated, const void *matches12_out, const void *hyp_R, const void *hyp_t,
          const void *hyp_good, const void *hyp_parallax, const void *result)
{
    if (!kps1 || !kps2 || !matches12 || !pairs || !H || !F || !inl_H || !inl_F || !ransac_result || !R21 || !t21 || !points3D || !triangulated ||
        !matches12_out || !hyp_R || !hyp_t || !hyp_good || !hyp_parallax || !result)
        return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n1 < 1 || n2 < 1) return orbx_set_error(ORBX_E_ARG, "n1 and n2 must be at least 1");
    if (!(sigma > 0.f)) return orbx_set_error(ORBX_E_ARG, "sigma must be positive");
    if (!(fx > 0.f) || !(fy > 0.f) || !isfinite(fx) || !isfinite(fy)) return orbx_set_error(ORBX_E_ARG, "fx and fy must be finite and positive");
    if (family < -1 || family > 1) return orbx_set_error(ORBX_E_ARG, "family must be -1 (the RANSAC's choice), 0 (F) or 1 (H)");
    if (n1 > ORBM_TWO_VIEW_MAX_KEYPOINTS || n2 > ORBM_TWO_VIEW_MAX_KEYPOINTS)
        return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_TWO_VIEW_MAX_KEYPOINTS (65536) key points in a frame");
    return ORBX_OK;
}

// the three launches on `s`; every pointer is device memory
int launch(orbm_t *h, hipStream_t s, const TvpCam &cam, const void *d_kps1, int n1, const void *d_kps2, int n2, const int32_t *d_matches12,
           const int32_t *d_pairs, const float *d_H, const float *d_F, const uint8_t *d_inl_H, const uint8_t *d_inl_F, const int32_t *d_ransac_result,
           int family, float sigma, float min_parallax, float *d_R21, float *d_t21, float *d_points3D, uint8_t *d_triangulated,
           int32_t *d_matches12_out, float *d_hyp_R, float *d_hyp_t, int32_t *d_hyp_good, float *d_hyp_parallax, uint8_t *d_hyp_code,
           int32_t *d_result)
{
    TvpScratch sc;
    sc.lay(nullptr, n1);   // measures
    void *dev = nullptr;
    ORB_TRY(orbm_two_view_pose_scratch(h, sc.total, &dev));
    sc.lay(dev, n1);
    const float th2 = 4.f * sigma * sigma;   // :451, :505
    hipLaunchKernelGGL(k_tvp_decompose, dim3(1), dim3(64), 0, s, cam, d_H, d_F, d_ransac_result, family, n1, sc.head, d_hyp_R, d_hyp_t);
    hipLaunchKernelGGL(k_tvp_check, dim3(TP_HYP), dim3(TP_T), 0, s, cam, (const orbx_kp *)d_kps1, n1, (const orbx_kp *)d_kps2, n2, d_pairs, d_inl_H,
                       d_inl_F, th2, sc.head, d_hyp_R, d_hyp_t, sc.keys, d_hyp_good, d_hyp_parallax, d_hyp_code);
    hipLaunchKernelGGL(k_tvp_decide, dim3(1), dim3(TP_T), 0, s, cam, (const orbx_kp *)d_kps1, n1, (const orbx_kp *)d_kps2, n2, d_pairs, d_inl_H,
                       d_inl_F, d_matches12, th2, min_parallax, sc.head, d_hyp_R, d_hyp_t, d_hyp_good, d_hyp_parallax, d_R21, d_t21, d_points3D,
                       d_triangulated, d_matches12_out, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

} // namespace

extern "C" int orbm_two_view_decide(int family, const int32_t *n_good, const float *parallax, int n_inlier, float min_parallax, int32_t *winner,
                                    int32_t *min_good, int32_t *reason)
{
    if (!n_good || !parallax || !winner || !min_good || !reason) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (family < 0 || family > 1) return orbx_set_error(ORBX_E_ARG, "family must be 0 (F) or 1 (H)");
    if (n_inlier < 0) return orbx_set_error(ORBX_E_ARG, "negative inlier count");
    int good[TP_HYP];
    float par[TP_HYP];
    const int rows = family ? 8 : 4;
    for (int k = 0; k < TP_HYP; ++k) good[k] = k < rows ? n_good[k] : 0, par[k] = k < rows ? parallax[k] : 0.f;
    int w = -1, mg = 0;
    *reason = tvp_decide(family, good, par, n_inlier, min_parallax, w, mg);
    *winner = w, *min_good = mg;
    return ORBX_OK;
}

extern "C" int orbm_two_view_pose_device(orbm_t *h, float fx, float fy, float cx, float cy, const void *d_kps1, int n1, const void *d_kps2, int n2,
                                         const int32_t *d_matches12, const int32_t *d_pairs, const float *d_H, const float *d_F,
                                         const uint8_t *d_inl_H, const uint8_t *d_inl_F, const int32_t *d_ransac_result, int family, float sigma,
                                         float min_parallax, float *d_R21, float *d_t21, float *d_points3D, uint8_t *d_triangulated,
                                         int32_t *d_matches12_out, float *d_hyp_R, float *d_hyp_t, int32_t *d_hyp_good, float *d_hyp_parallax,
                                         uint8_t *d_hyp_code, int32_t *d_result, void *stream)
{
    if (int rc = check(fx, fy, d_kps1, n1, d_kps2, n2, d_matches12, d_pairs, d_H, d_F, d_inl_H, d_inl_F, d_ransac_result, family, sigma, d_R21,
                       d_t21, d_points3D, d_triangulated, d_matches12_out, d_hyp_R, d_hyp_t, d_hyp_good, d_hyp_parallax, d_result))
        return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    const TvpCam cam = {fx, fy, cx, cy};
    return launch(h, s, cam, d_kps1, n1, d_kps2, n2, d_matches12, d_pairs, d_H, d_F, d_inl_H, d_inl_F, d_ransac_result, family, sigma, min_parallax,
                  d_R21, d_t21, d_points3D, d_triangulated, d_matches12_out, d_hyp_R, d_hyp_t, d_hyp_good, d_hyp_parallax, d_hyp_code, d_result);
}

extern "C" int orbm_two_view_pose(orbm_t *h, float fx, float fy, float cx, float cy, const void *kps1, int n1, const void *kps2, int n2,
                                  const int32_t *matches12, const int32_t *pairs, const float *H, const float *F, const uint8_t *inl_H,
                                  const uint8_t *inl_F, const int32_t *ransac_result, int family, float sigma, float min_parallax, float *R21,
                                  float *t21, float *points3D, uint8_t *triangulated, int32_t *matches12_out, float *hyp_R, float *hyp_t,
                                  int32_t *hyp_good, float *hyp_parallax, uint8_t *hyp_code, int32_t *result)
{
    if (int rc = check(fx, fy, kps1, n1, kps2, n2, matches12, pairs, H, F, inl_H, inl_F, ransac_result, family, sigma, R21, t21, points3D,
                       triangulated, matches12_out, hyp_R, hyp_t, hyp_good, hyp_parallax, result))
        return rc;
    if (int rc = orb_need_device()) return rc;
    if (!h) return orbx_set_error(ORBX_E_ARG, "null handle");
    // staging block, the device's and the pinned one alike: [kps1 | kps2 | matches12 | pairs | H | F | inl_H | inl_F | ransac_result] up,
    // [result | R21 .. hyp_code] down
    const size_t N1 = (size_t)n1, N2 = (size_t)n2;
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t at = total; total += (bytes + 15) & ~(size_t)15; return at; };
    const size_t o_kps1 = take(N1 * sizeof(orbx_kp)), o_kps2 = take(N2 * sizeof(orbx_kp)), o_m = take(N1 * 4), o_pairs = take(N1 * 8);
    const size_t o_H = take(36), o_F = take(36), o_iH = take(N1), o_iF = take(N1), o_rr = take(32);
    const size_t in_end = total;
    const size_t o_res = take(64), o_R = take(36), o_t = take(12), o_p3 = take(N1 * 12), o_tri = take(N1), o_mo = take(N1 * 4);
    const size_t o_hR = take(TP_HYP * 36), o_ht = take(TP_HYP * 12), o_hg = take(TP_HYP * 4), o_hp = take(TP_HYP * 4);
    const size_t o_code = take(hyp_code ? TP_HYP * N1 : 0);
    void *dev = nullptr, *pin = nullptr;
    hipStream_t s = nullptr;
    ORB_TRY(orbm_host_stage(h, total, &dev, &pin, &s));
    char *d = (char *)dev, *p = (char *)pin;
    memcpy(p + o_kps1, kps1, N1 * sizeof(orbx_kp)), memcpy(p + o_kps2, kps2, N2 * sizeof(orbx_kp)), memcpy(p + o_m, matches12, N1 * 4);
    memcpy(p + o_pairs, pairs, N1 * 8), memcpy(p + o_H, H, 36), memcpy(p + o_F, F, 36), memcpy(p + o_iH, inl_H, N1), memcpy(p + o_iF, inl_F, N1);
    memcpy(p + o_rr, ransac_result, 32);
    ORB_TRY(hipMemcpyAsync(d, p, in_end, hipMemcpyHostToDevice, s));
    const TvpCam cam = {fx, fy, cx, cy};
    if (int rc = launch(h, s, cam, d + o_kps1, n1, d + o_kps2, n2, (const int32_t *)(d + o_m), (const int32_t *)(d + o_pairs), (const float *)(d + o_H),
                        (const float *)(d + o_F), (const uint8_t *)(d + o_iH), (const uint8_t *)(d + o_iF), (const int32_t *)(d + o_rr), family, sigma,
                        min_parallax, (float *)(d + o_R), (float *)(d + o_t), (float *)(d + o_p3), (uint8_t *)(d + o_tri), (int32_t *)(d + o_mo),
                        (float *)(d + o_hR), (float *)(d + o_ht), (int32_t *)(d + o_hg), (float *)(d + o_hp),
                        hyp_code ? (uint8_t *)(d + o_code) : nullptr, (int32_t *)(d + o_res)))
        return rc;
    ORB_TRY(hipMemcpyAsync(p + in_end, d + in_end, total - in_end, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));
    memcpy(result, p + o_res, 64);
    if (result[0] == 1) return ORBX_OK;   // the RANSAC refused: only `result` is written
    memcpy(R21, p + o_R, 36), memcpy(t21, p + o_t, 12), memcpy(points3D, p + o_p3, N1 * 12), memcpy(triangulated, p + o_tri, N1);
    memcpy(matches12_out, p + o_mo, N1 * 4), memcpy(hyp_R, p + o_hR, TP_HYP * 36), memcpy(hyp_t, p + o_ht, TP_HYP * 12);
    memcpy(hyp_good, p + o_hg, TP_HYP * 4), memcpy(hyp_parallax, p + o_hp, TP_HYP * 4);
    if (hyp_code) memcpy(hyp_code, p + o_code, TP_HYP * N1);
    return ORBX_OK;
}
