// The H / F RANSAC of the two-view initialisation on the device (include/orbm.h, "Two-view initialisation: the H / F RANSAC"): what
// TwoViewReconstruction::Reconstruct does between SearchForInitialization and ReconstructH / ReconstructF.
//   orbm_two_view_ransac_device   TwoViewReconstruction.cpp:20-79 (match list, draw, RH), :86-344 (Find*, Compute*, Check*), :558-596 (Normalize)
//   orbm_two_view_ransac          the same with host pointers: one pinned copy each way on the handle's stream
//   orbm_two_view_sets            the draw of :42-58 on the host
//
// Three launches on the caller's stream, nothing between them:
//   k_tv_prepare     ONE workgroup of 1024: the match list (block scan), Normalize of both frames (tree sums), the draw
//   k_tv_hypotheses  ONE WAVE per hypothesis, 2 * iters waves, four to a workgroup: matrix, singular vector, de-normalisation, score
//   k_tv_pick        ONE workgroup of 1024: first maximum per family, the masks expanded, RH, d_result
//
// Evaluation orders outside the singular-vector solves are the header's (no fused multiply-add: the build passes
// -ffp-contract=off and the pragma below repeats it; `/` and the square roots are the correctly rounded ones).
//
// The solve.  The reference takes the last column of V of a JacobiSVD of the 16 x 9 (H) or 8 x 9 (F) matrix A.  Here a one-sided
// (Hestenes) Jacobi rotates pairs of COLUMNS of A until they are orthogonal, applying the rotations to V = I, as
// orbm_triangulate.hip does for its 4 x 4; the column of least norm belongs to the smallest singular value.  One lane cannot hold
// 144 + 81 values, so lane r of every 16 holds ROW r of A and of V (9 + 9 values, constant indices) and the three column dot
// products of a rotation are 16-wide __shfl_xor butterflies (steps 8, 4, 2, 1: they stay inside the 16 lanes, and a butterfly
// leaves the same bits in all of them, so the four quarters of the wave run the same solve and no lane diverges).  The 36 pairs
// of a sweep are unrolled; TV_SWEEPS sweeps run.
//
// The solve runs in DOUBLE on the float matrix (the sample is normalised and the entries are multiplied in float, as the
// reference does), and so do the rank-2 step and the de-normalisation; the 3 x 3 is rounded to float once.  The reason is a
// numpy trial, not a device measurement: a float restatement of this loop with TEN sweeps (360 rotations; the shipped loop runs
// 9 sweeps, 324 rotations, in double) left 3 .. 12 times the error of LAPACK's float SVD against a float64 one on the test
// scenes, which the test's bar of 4 times does not allow; in double what remains is the rounding of the float inputs, which
// LAPACK's float run has too (0.3 .. 2 times its error in the same restatement; 0.06 .. 3.0 times measured on the device).
// Convergence of the double loop there (8 .. 2000 matches, general and planar, 200 sets each, every sample, conditioned or not):
// the sine of the angle to LAPACK's float64 vector
// is below 1e-8 after 7 sweeps and at its floor (1e-13) after 8; 9 are run.  The 3 x 3 of the rank-2 step (three pairs a sweep, in
// every lane's registers) is at its floor after 4 sweeps; TV_SWEEPS3 = 6 are run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/orbm.h"
#include "../../include/orbx.h"
#include "orb_device.h"
#include "orb_host.h"
#include "orbm_internal.h"
#include "orbm_jacobi.h"

#pragma clang fp contract(off)

namespace {

constexpr int TV_T = 1024;          // threads of k_tv_prepare and k_tv_pick
constexpr int TV_WAVES = TV_T / 64;
constexpr int TV_HYP_WAVES = 4;     // hypotheses per workgroup of k_tv_hypotheses
constexpr int TV_SWEEPS = 9;
constexpr int TV_SWEEPS3 = 6;
constexpr int TV_MAX_ITERS = ORBM_TWO_VIEW_MAX_ITERS;
constexpr unsigned TV_RNG_COEFF = 4164903690u;   // cv::RNG

// head: [0] n_matches, [1] status of k_tv_prepare (0, or 1: fewer than 8 matches -- the later kernels return at once)
// norm: meanX, meanY, sX, sY of frame 1, then of frame 2

__device__ __host__ __forceinline__ unsigned rng_next(unsigned long long &state)
{
    state = (unsigned long long)(unsigned)state * TV_RNG_COEFF + (state >> 32);
    return (unsigned)state;
}

// The raw stream on 64 lanes.  With b = 2^32 the 64-bit state S = c * b + x steps to S' = a * x + c, and S' * b = a * b * x + b * c
// = S (mod m), m = a * b - 1: the generator is S' = S * a (mod m), so the state 128 j steps ahead is S * a^(128 j) (mod m) -- one
// modular product by a constant of the table below.  The congruence names the state only once it lies in [1, m]: any state does
// after three real steps (c <= a after one, S <= a * b after two, S <= m after three, and stays), and 0 is reached from 0 alone,
// which no call starts from.  So every lane takes four real steps to S_4, whose draw is raw[3]; lane j then owns raw[3 + 128 j ..
// 3 + 128 j + 127], and lane 0 writes raw[0 .. 2] too.  m itself (the fixed point x = b - 1, c = a - 1) is the residue 0.
constexpr unsigned long long TV_RNG_MOD = ((unsigned long long)TV_RNG_COEFF << 32) - 1ull;
constexpr int TV_RNG_LANES = 64, TV_RNG_CHUNK = 128;   // 3 + 64 * 128 >= 8 * TV_MAX_ITERS
struct TvJump { unsigned long long a[TV_RNG_LANES]; };  // a^(128 j) mod m; by value in the launch's arguments

__device__ __host__ __forceinline__ unsigned long long rng_addmod(unsigned long long x, unsigned long long y)   // x, y < m
{
    unsigned long long s = x + y;   // may wrap: the true sum is below 2 m < 2^65, and subtracting m modulo 2^64 is right either way
    if (s < x || s >= TV_RNG_MOD) s -= TV_RNG_MOD;
    return s;
}
__device__ __host__ inline unsigned long long rng_mulmod(unsigned long long x, unsigned long long y)           // x, y < m
{
    unsigned long long r = 0;
    for (int bit = 63; bit >= 0; --bit) {
        r = rng_addmod(r, r);
        if ((y >> bit) & 1ull) r = rng_addmod(r, x);
    }
    return r;
}
// lane `lane` of TV_RNG_LANES writes its share of raw[0 .. count)
__device__ __host__ inline void rng_lane(unsigned long long state, const TvJump &jump, int lane, int count, unsigned *raw)
{
    unsigned head[4];
    for (int k = 0; k < 4; ++k) head[k] = rng_next(state);   // S_1 .. S_4
    if (lane == 0)
        for (int k = 0; k < 3; ++k)
            if (k < count) raw[k] = head[k];
    const int first = 3 + TV_RNG_CHUNK * lane;
    if (first >= count) return;
    unsigned long long t = rng_mulmod(state == TV_RNG_MOD ? 0ull : state, jump.a[lane]);
    if (t == 0) t = TV_RNG_MOD;
    for (int k = 0; k < TV_RNG_CHUNK && first + k < count; ++k) {
        raw[first + k] = (unsigned)t;
        rng_next(t);
    }
}
inline TvJump rng_jump_table()
{
    TvJump j;
    unsigned long long step = 1;   // a^128 mod m
    for (int k = 0; k < TV_RNG_CHUNK; ++k) step = rng_mulmod(step, (unsigned long long)TV_RNG_COEFF);
    j.a[0] = 1;
    for (int k = 1; k < TV_RNG_LANES; ++k) j.a[k] = rng_mulmod(j.a[k - 1], step);
    return j;
}

// the eight "take index randi, move the last into its place" steps of one set from its eight raw draws: position p of the
// shrinking availableIndices holds p unless an earlier step moved a last element there -- at most eight overrides
__device__ __host__ __forceinline__ void resolve_set(const unsigned (&raw)[8], int n_matches, int (&out)[8])
{
    int ov_pos[8], ov_val[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int size = n_matches - j;
        const int randi = (int)(raw[j] % (unsigned)size);
        int idx = randi, last = size - 1;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < j) {   // ascending: the latest override of a position wins
                idx = ov_pos[k] == randi ? ov_val[k] : idx;
                last = ov_pos[k] == size - 1 ? ov_val[k] : last;
            }
        out[j] = idx;
        ov_pos[j] = randi;
        ov_val[j] = last;
    }
}

__global__ __launch_bounds__(TV_T) void k_tv_prepare(const orbx_kp *__restrict__ kps1, int n1, const orbx_kp *__restrict__ kps2, int n2,
                                                     const int32_t *__restrict__ matches12, int iters, unsigned long long rng_state, int draw,
                                                     const TvJump jump, int32_t *__restrict__ pairs, int32_t *__restrict__ head, float *__restrict__ norm,
                                                     int32_t *__restrict__ sets, int32_t *__restrict__ result)
{
    __shared__ unsigned s_raw[8 * TV_MAX_ITERS];
    __shared__ float s_part[TV_WAVES][4];
    __shared__ int s_wave[TV_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // match_pairs (:26-30) in ascending i.  The list is walked twice: fewer than 8 matches have to be found BEFORE anything is
    // written, so the first walk only counts and the second, on the same flags, writes the rows
    int n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int at = 0;
        for (int i0 = 0; i0 < n1; i0 += TV_T) {   // uniform trip count
            const int i = i0 + tid;
            const int m = i < n1 ? matches12[i] : -1;
            const int flag = m >= 0 && m < n2;
            int total;
            const int before = block_scan<TV_WAVES>(flag, s_wave, total);
            if (pass && flag) pairs[2 * (at + before)] = i, pairs[2 * (at + before) + 1] = m;
            at += total;
        }
        if (pass) break;
        n = at;
        if (tid == 0) head[0] = n, head[1] = n < 8 ? 1 : 0;
        if (n < 8) {   // uniform: the reference would index an empty vector; only d_result is written
            if (tid < 8) result[tid] = tid == 0 ? n : tid == 1 ? 1 : tid == 2 || tid == 3 ? -1 : 0;
            return;
        }
    }
    for (int i = n + tid; i < n1; i += TV_T) pairs[2 * i] = -1, pairs[2 * i + 1] = -1;   // the rows behind the list
    // the raw 32-bit stream does not depend on n_matches: the last wave produces it, each lane 128 values from a state it jumps to,
    // while the others reduce (its share of a call: profiles/two_view_latency.txt, drawn against given sets)
    if (draw && wave == TV_WAVES - 1) rng_lane(rng_state, jump, lane, 8 * iters, s_raw);
    // Normalize (:558-596) over ALL key points of each frame; the sums as a tree: a thread's stride, the wave's butterfly, the waves in order
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int round = 0; round < 2; ++round) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < n1; i += TV_T) {
            const float x = kps1[i].x, y = kps1[i].y;
            acc[0] += round ? fabsf(x - mean[0]) : x;
            acc[1] += round ? fabsf(y - mean[1]) : y;
        }
        for (int i = tid; i < n2; i += TV_T) {
            const float x = kps2[i].x, y = kps2[i].y;
            acc[2] += round ? fabsf(x - mean[2]) : x;
            acc[3] += round ? fabsf(y - mean[3]) : y;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = wave_sum(acc[k]);
            if (lane == 0) s_part[wave][k] = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = 0.f;
            for (int w = 0; w < TV_WAVES; ++w) t = t + s_part[w][k];
            const float m = t / (float)(k < 2 ? n1 : n2);
            if (round == 0) mean[k] = m; else s[k] = 1.f / m;
        }
        __syncthreads();   // s_part is rewritten by the next round; behind the second round: s_raw is complete
    }
#pragma unroll
    for (int k = 0; k < 8; ++k)   // constant indices: the arrays stay in registers
        if (tid == k) norm[k] = (k & 2) ? s[(k >> 2) * 2 + (k & 1)] : mean[(k >> 2) * 2 + (k & 1)];
    if (draw && tid < iters) {
        unsigned raw[8];
        int out[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[j] = s_raw[8 * tid + j];
        resolve_set(raw, n, out);
#pragma unroll
        for (int j = 0; j < 8; ++j) sets[8 * tid + j] = out[j];
    }
}

// the sum of v over the 16 lanes that hold the rows of one matrix; the same bits in all of them
__device__ __forceinline__ double sum16(double v)
{
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

// jacobi_cs (the rotation angle of one Hestenes step), dot3 and rotate3: orbm_jacobi.h, shared with orbm_two_view_pose.hip

// ComputeF21 :220-223: U diag(w0, w1, 0) V^T of the row-major 3 x 3 `m`, in place
__device__ __forceinline__ void rank2(double (&m)[9])
{
    double B[3][3], V[3][3];   // by column
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) B[c][r] = m[3 * r + c], V[c][r] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < TV_SWEEPS3; ++sweep) {
        rotate3(B[0], B[1], V[0], V[1]);
        rotate3(B[0], B[2], V[0], V[2]);
        rotate3(B[1], B[2], V[1], V[2]);
    }
    const double n0 = dot3(B[0], B[0]), n1 = dot3(B[1], B[1]), n2 = dot3(B[2], B[2]);
    int k = 0;
    double best = n0;
    if (n1 < best) best = n1, k = 1;
    if (n2 < best) k = 2;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t0 = k == 0 ? 0.0 : B[0][r] * V[0][c], t1 = k == 1 ? 0.0 : B[1][r] * V[1][c], t2 = k == 2 ? 0.0 : B[2][r] * V[2][c];
            m[3 * r + c] = (t0 + t1) + t2;
        }
}

__global__ __launch_bounds__(TV_HYP_WAVES * 64) void k_tv_hypotheses(const orbx_kp *__restrict__ kps1, const orbx_kp *__restrict__ kps2,
                                                                     const int32_t *__restrict__ pairs, const int32_t *__restrict__ head,
                                                                     const float *__restrict__ norm, const int32_t *__restrict__ sets, int iters,
                                                                     float inv_sigma2, int words, float *__restrict__ hyp,
                                                                     float *__restrict__ hyp_score, unsigned long long *__restrict__ masks)
{
    const int lane = threadIdx.x & 63;
    const int g = uniform(blockIdx.x * TV_HYP_WAVES + (threadIdx.x >> 6));   // no barrier below: a wave may leave alone
    if (g >= 2 * iters || head[1] != 0) return;
    const int n = head[0];
    const int fam = g >= iters ? 1 : 0, it = g - fam * iters;   // 0: H, 1: F
    const float m1x = norm[0], m1y = norm[1], s1x = norm[2], s1y = norm[3], m2x = norm[4], m2y = norm[5], s2x = norm[6], s2y = norm[7];
    // this lane's row of A and of V
    const int r = lane & 15;
    double a[9], v[9];
    {
        const int k = fam ? (r & 7) : (r >> 1);
        const int idx = min(max(sets[8 * it + k], 0), n - 1);   // a caller's set is kept inside the match list
        const int i1 = pairs[2 * idx], i2 = pairs[2 * idx + 1];
        const float u1 = (kps1[i1].x - m1x) * s1x, v1 = (kps1[i1].y - m1y) * s1y;
        const float u2 = (kps2[i2].x - m2x) * s2x, v2 = (kps2[i2].y - m2y) * s2y;
        if (fam) {          // :207-215
            const bool on = r < 8;
            a[0] = on ? u2 * u1 : 0.f, a[1] = on ? u2 * v1 : 0.f, a[2] = on ? u2 : 0.f;
            a[3] = on ? v2 * u1 : 0.f, a[4] = on ? v2 * v1 : 0.f, a[5] = on ? v2 : 0.f;
            a[6] = on ? u1 : 0.f, a[7] = on ? v1 : 0.f, a[8] = on ? 1.f : 0.f;
        } else if (r & 1) { // :182-190
            a[0] = u1, a[1] = v1, a[2] = 1.f, a[3] = 0.f, a[4] = 0.f, a[5] = 0.f;
            a[6] = -u2 * u1, a[7] = -u2 * v1, a[8] = -u2;
        } else {            // :172-180
            a[0] = 0.f, a[1] = 0.f, a[2] = 0.f, a[3] = -u1, a[4] = -v1, a[5] = -1.f;
            a[6] = v2 * u1, a[7] = v2 * v1, a[8] = v2;
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) v[c] = r == c ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < TV_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = p + 1; q < 9; ++q) {
                const double alpha = sum16(a[p] * a[p]), beta = sum16(a[q] * a[q]), gamma = sum16(a[p] * a[q]);
                double c, s;
                jacobi_cs(alpha, beta, gamma, c, s);
                const double x = a[p], y = a[q];
                a[p] = c * x - s * y;
                a[q] = s * x + c * y;
                const double vx = v[p], vy = v[q];
                v[p] = c * vx - s * vy;
                v[q] = s * vx + c * vy;
            }
    }
    // the column of least norm: strict '<' in ascending order; its column of V, row j from lane j
    double best = sum16(a[0] * a[0]), mine = v[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        const double nk = sum16(a[k] * a[k]);
        const bool take = nk < best;
        best = take ? nk : best;
        mine = take ? v[k] : mine;
    }
    double hn[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) hn[j] = __shfl(mine, j);
    // the de-normalisation, still in double on the float entries of T1 and T2; rounded to float once
    float h[9];
    const double t1x = (double)(-m1x * s1x), t1y = (double)(-m1y * s1y);   // T1(0, 2), T1(1, 2) (:595)
    double m[9];
    if (fam) {
        rank2(hn);
        // T2^T * Fn
        const double t2x = (double)(-m2x * s2x), t2y = (double)(-m2y * s2y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m[c] = (double)s2x * hn[c];
            m[3 + c] = (double)s2y * hn[3 + c];
            m[6 + c] = (t2x * hn[c] + t2y * hn[3 + c]) + hn[6 + c];
        }
    } else {
        // T2^-1 * Hn, T2^-1 = [1 / sX2, 0, meanX2; 0, 1 / sY2, meanY2; 0, 0, 1]
        const double ix = 1.0 / (double)s2x, iy = 1.0 / (double)s2y;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m[c] = ix * hn[c] + (double)m2x * hn[6 + c];
            m[3 + c] = iy * hn[3 + c] + (double)m2y * hn[6 + c];
            m[6 + c] = hn[6 + c];
        }
    }
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {   // (...) * T1
        h[3 * rr] = (float)(m[3 * rr] * (double)s1x);
        h[3 * rr + 1] = (float)(m[3 * rr + 1] * (double)s1y);
        h[3 * rr + 2] = (float)((m[3 * rr] * t1x + m[3 * rr + 1] * t1y) + m[3 * rr + 2]);
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 9; ++j) hyp[(size_t)g * 9 + j] = h[j];
    }
    // the score: all 64 lanes stride over the matches
    float inv[9];
    if (!fam) {   // H12 = H21.inverse(): the cofactors over the determinant in double, rounded to float once
        double d[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) d[j] = (double)h[j];
        const double c0 = d[4] * d[8] - d[5] * d[7], c1 = d[3] * d[8] - d[5] * d[6], c2 = d[3] * d[7] - d[4] * d[6];
        const double id = 1.0 / ((d[0] * c0 - d[1] * c1) + d[2] * c2);
        inv[0] = (float)(c0 * id), inv[1] = (float)((d[2] * d[7] - d[1] * d[8]) * id), inv[2] = (float)((d[1] * d[5] - d[2] * d[4]) * id);
        inv[3] = (float)(-c1 * id), inv[4] = (float)((d[0] * d[8] - d[2] * d[6]) * id), inv[5] = (float)((d[2] * d[3] - d[0] * d[5]) * id);
        inv[6] = (float)(c2 * id), inv[7] = (float)((d[1] * d[6] - d[0] * d[7]) * id), inv[8] = (float)((d[0] * d[4] - d[1] * d[3]) * id);
    }
    float acc = 0.f;
    for (int base = 0; base < n; base += 64) {   // uniform trip count: the ballot sees the whole wave
        const int k = base + lane;
        bool inl = false;
        if (k < n) {
            const int i1 = pairs[2 * k], i2 = pairs[2 * k + 1];
            const float u1 = kps1[i1].x, v1 = kps1[i1].y, u2 = kps2[i2].x, v2 = kps2[i2].y;
            inl = true;
            if (fam) {   // CheckFundamental :316-338
                const float th = 3.841f, th_score = 5.991f;
                const float a2 = (h[0] * u1 + h[1] * v1) + h[2], b2 = (h[3] * u1 + h[4] * v1) + h[5], c2 = (h[6] * u1 + h[7] * v1) + h[8];
                const float num2 = (a2 * u2 + b2 * v2) + c2;
                const float chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_sigma2;
                if (chi1 > th) inl = false; else acc += th_score - chi1;
                const float a1 = (h[0] * u2 + h[3] * v2) + h[6], b1 = (h[1] * u2 + h[4] * v2) + h[7], c1 = (h[2] * u2 + h[5] * v2) + h[8];
                const float num1 = (a1 * u1 + b1 * v1) + c1;
                const float chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_sigma2;
                if (chi2 > th) inl = false; else acc += th_score - chi2;
            } else {     // CheckHomography :262-282
                const float th = 5.991f;
                const float w2 = 1.f / ((inv[6] * u2 + inv[7] * v2) + inv[8]);
                const float x1 = ((inv[0] * u2 + inv[1] * v2) + inv[2]) * w2, y1 = ((inv[3] * u2 + inv[4] * v2) + inv[5]) * w2;
                const float chi1 = ((u1 - x1) * (u1 - x1) + (v1 - y1) * (v1 - y1)) * inv_sigma2;
                if (chi1 > th) inl = false; else acc += th - chi1;
                const float w1 = 1.f / ((h[6] * u1 + h[7] * v1) + h[8]);
                const float x2 = ((h[0] * u1 + h[1] * v1) + h[2]) * w1, y2 = ((h[3] * u1 + h[4] * v1) + h[5]) * w1;
                const float chi2 = ((u2 - x2) * (u2 - x2) + (v2 - y2) * (v2 - y2)) * inv_sigma2;
                if (chi2 > th) inl = false; else acc += th - chi2;
            }
        }
        const unsigned long long mk = __ballot(inl);
        if (lane == 0) masks[(size_t)g * words + (base >> 6)] = mk;   // base / 64 < words: n <= n1 <= 64 * words
    }
    const float score = wave_sum(acc);
    if (lane == 0) hyp_score[g] = score;
}

__global__ __launch_bounds__(TV_T) void k_tv_pick(const int32_t *__restrict__ head, int iters, int n1, int words, const float *__restrict__ hyp,
                                                  const float *__restrict__ hyp_score, const unsigned long long *__restrict__ masks,
                                                  float *__restrict__ out_H, float *__restrict__ out_F, uint8_t *__restrict__ inl_H,
                                                  uint8_t *__restrict__ inl_F, float *__restrict__ out_score, float *__restrict__ out_rh,
                                                  int32_t *__restrict__ result)
{
    __shared__ float s_max[2][TV_WAVES];
    __shared__ int s_idx[2][TV_WAVES];
    __shared__ int s_count[2];
    if (head[1] != 0) return;   // uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = head[0];
    if (tid < 2) s_count[tid] = 0;
    // the first index whose score is the maximum (:116, :155: strict '>'); a score that is not above 0 -- a NaN too -- never wins
#pragma unroll
    for (int fam = 0; fam < 2; ++fam) {
        float s = tid < iters ? hyp_score[fam * iters + tid] : 0.f;
        s = s > 0.f ? s : 0.f;
        const float wm = wave_max(s);
        const unsigned long long at = __ballot(s == wm);
        if (lane == 0) s_max[fam][wave] = wm, s_idx[fam][wave] = wave * 64 + (int)__ffsll((long long)at) - 1;
    }
    __syncthreads();
    int win[2];
    float best[2];
#pragma unroll
    for (int fam = 0; fam < 2; ++fam) {
        win[fam] = -1, best[fam] = 0.f;
        for (int w = 0; w < TV_WAVES; ++w)
            if (s_max[fam][w] > best[fam]) best[fam] = s_max[fam][w], win[fam] = s_idx[fam][w];
    }
    // the two winning mask rows, a byte per match index; entries from n_matches on are 0
    int cnt[2] = {0, 0};
    for (int i = tid; i < n1; i += TV_T) {
#pragma unroll
        for (int fam = 0; fam < 2; ++fam) {
            int bit = 0;
            if (i < n && win[fam] >= 0) bit = (int)(masks[(size_t)(fam * iters + win[fam]) * words + (i >> 6)] >> (i & 63) & 1ull);
            (fam ? inl_F : inl_H)[i] = (uint8_t)bit;
            cnt[fam] += bit;
        }
    }
    block_add(s_count, {0, 1}, cnt);
    if (tid < 18) {
        const int fam = tid >= 9, j = tid - 9 * fam, w = fam ? win[1] : win[0];
        (fam ? out_F : out_H)[j] = w >= 0 ? hyp[(size_t)(fam * iters + w) * 9 + j] : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        const float sum = best[0] + best[1];
        const bool none = sum == 0.f;                       // :73
        const float rh = none ? 0.f : best[0] / sum;        // :74
        out_score[0] = best[0], out_score[1] = best[1];
        out_rh[0] = rh;
        result[0] = n, result[1] = none ? 2 : 0, result[2] = win[0], result[3] = win[1];
        result[4] = rh > 0.5f ? 1 : 0;                      // :79
        result[5] = s_count[0], result[6] = s_count[1], result[7] = 0;
    }
}

// the handle scratch of one call, 16-byte aligned pieces
struct TvScratch {
    int32_t *head;
    float *norm;
    int32_t *sets;
    float *hyp, *hyp_score;
    unsigned long long *masks;
    size_t total;
    void lay(void *block, int iters, int words)
    {
        char *base = (char *)block;
        total = 0;
        auto take = [&](size_t bytes) { char *p = base + total; total += (bytes + 15) & ~(size_t)15; return p; };
        head = (int32_t *)take(16), norm = (float *)take(32), sets = (int32_t *)take((size_t)iters * 32);
        hyp = (float *)take((size_t)iters * 72), hyp_score = (float *)take((size_t)iters * 8);
        masks = (unsigned long long *)take((size_t)2 * iters * words * 8);
    }
};

int check(const void *kps1, int n1, const void *kps2, int n2, const void *matches12, float sigma, int iters, const void *pairs, const void *H,
          const void *F, const void *inl_H, const void *inl_F, const void *score, const void *rh, const void *result)
{
    if (!kps1 || !kps2 || !matches12 || !pairs || !H || !F || !inl_H || !inl_F || !score || !rh || !result)
        return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n1 < 1 || n2 < 1) return orbx_set_error(ORBX_E_ARG, "n1 and n2 must be at least 1");
    if (iters < 1 || iters > TV_MAX_ITERS) return orbx_set_error(ORBX_E_ARG, "iters must be 1 .. 1024");
    if (!(sigma > 0.f)) return orbx_set_error(ORBX_E_ARG, "sigma must be positive");
    // behind the argument errors: 2 * iters mask rows of n1 bits stay within 16 MB of handle scratch, every index within int
    if (n1 > ORBM_TWO_VIEW_MAX_KEYPOINTS || n2 > ORBM_TWO_VIEW_MAX_KEYPOINTS)
        return orbx_set_error(ORBX_E_UNSUPPORTED, "more than ORBM_TWO_VIEW_MAX_KEYPOINTS (65536) key points in a frame");
    return ORBX_OK;
}

// the three launches on `s`; every pointer is device memory
int launch(orbm_t *h, hipStream_t s, const void *d_kps1, int n1, const void *d_kps2, int n2, const int32_t *d_matches12, float sigma, int iters,
           uint64_t rng_state, const int32_t *d_sets, int32_t *d_pairs, float *d_H, float *d_F, uint8_t *d_inl_H, uint8_t *d_inl_F, float *d_score,
           float *d_rh, float *d_hyp, float *d_hyp_score, int32_t *d_result)
{
    const int words = (n1 + 63) / 64;
    TvScratch sc;
    sc.lay(nullptr, iters, words);   // measures
    void *dev = nullptr;
    ORB_TRY(orbm_two_view_scratch(h, sc.total, &dev));
    sc.lay(dev, iters, words);
    float *hyp = d_hyp ? d_hyp : sc.hyp, *hyp_score = d_hyp_score ? d_hyp_score : sc.hyp_score;
    const float inv_sigma2 = 1.f / (sigma * sigma);   // :251, :304
    hipLaunchKernelGGL(k_tv_prepare, dim3(1), dim3(TV_T), 0, s, (const orbx_kp *)d_kps1, n1, (const orbx_kp *)d_kps2, n2, d_matches12, iters,
                       (unsigned long long)(rng_state ? rng_state : ORBM_TWO_VIEW_RNG_DEFAULT), d_sets ? 0 : 1, rng_jump_table(), d_pairs, sc.head, sc.norm, sc.sets,
                       d_result);
    hipLaunchKernelGGL(k_tv_hypotheses, dim3((2 * iters + TV_HYP_WAVES - 1) / TV_HYP_WAVES), dim3(TV_HYP_WAVES * 64), 0, s, (const orbx_kp *)d_kps1,
                       (const orbx_kp *)d_kps2, d_pairs, sc.head, sc.norm, d_sets ? d_sets : sc.sets, iters, inv_sigma2, words, hyp, hyp_score,
                       sc.masks);
    hipLaunchKernelGGL(k_tv_pick, dim3(1), dim3(TV_T), 0, s, sc.head, iters, n1, words, hyp, hyp_score, sc.masks, d_H, d_F, d_inl_H, d_inl_F,
                       d_score, d_rh, d_result);
    ORB_TRY(hipGetLastError());
    return ORBX_OK;
}

} // namespace

extern "C" int orbm_two_view_sets(int n_matches, int iters, uint64_t rng_state, int32_t *sets)
{
    if (!sets) return orbx_set_error(ORBX_E_ARG, "null argument");
    if (n_matches < 8) return orbx_set_error(ORBX_E_ARG, "a set needs eight matches");
    if (iters < 1 || iters > TV_MAX_ITERS) return orbx_set_error(ORBX_E_ARG, "iters must be 1 .. 1024");
    // the raw stream by the code the device runs, lane after lane
    const unsigned long long state = rng_state ? rng_state : ORBM_TWO_VIEW_RNG_DEFAULT;
    const TvJump jump = rng_jump_table();
    std::vector<unsigned> stream((size_t)8 * iters);
    for (int lane = 0; lane < TV_RNG_LANES; ++lane) rng_lane(state, jump, lane, 8 * iters, stream.data());
    for (int it = 0; it < iters; ++it) {
        unsigned raw[8];
        int out[8];
        for (int j = 0; j < 8; ++j) raw[j] = stream[(size_t)8 * it + j];
        resolve_set(raw, n_matches, out);
        for (int j = 0; j < 8; ++j) sets[8 * it + j] = out[j];
    }
    return ORBX_OK;
}

extern "C" int orbm_two_view_ransac_device(orbm_t *h, const void *d_kps1, int n1, const void *d_kps2, int n2, const int32_t *d_matches12,
                                           float sigma, int iters, uint64_t rng_state, const int32_t *d_sets, int32_t *d_pairs, float *d_H,
                                           float *d_F, uint8_t *d_inl_H, uint8_t *d_inl_F, float *d_score, float *d_rh, float *d_hyp,
                                           float *d_hyp_score, int32_t *d_result, void *stream)
{
    if (int rc = check(d_kps1, n1, d_kps2, n2, d_matches12, sigma, iters, d_pairs, d_H, d_F, d_inl_H, d_inl_F, d_score, d_rh, d_result)) return rc;
    hipStream_t s;
    if (int rc = orbm_begin_device(h, stream, &s)) return rc;
    return launch(h, s, d_kps1, n1, d_kps2, n2, d_matches12, sigma, iters, rng_state, d_sets, d_pairs, d_H, d_F, d_inl_H, d_inl_F, d_score, d_rh,
                  d_hyp, d_hyp_score, d_result);
}

extern "C" int orbm_two_view_ransac(orbm_t *h, const void *kps1, int n1, const void *kps2, int n2, const int32_t *matches12, float sigma,
                                    int iters, uint64_t rng_state, const int32_t *sets, int32_t *pairs, float *H, float *F, uint8_t *inl_H,
                                    uint8_t *inl_F, float *score, float *rh, float *hyp, float *hyp_score, int32_t *result)
{
    if (int rc = check(kps1, n1, kps2, n2, matches12, sigma, iters, pairs, H, F, inl_H, inl_F, score, rh, result)) return rc;
    if (int rc = orb_need_device()) return rc;
    if (!h) return orbx_set_error(ORBX_E_ARG, "null handle");
    // staging block, the device's and the pinned one alike: [kps1 | kps2 | matches12 | sets] up, [result | pairs .. hyp_score] down
    const size_t N1 = (size_t)n1, N2 = (size_t)n2, I = (size_t)iters;
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t at = total; total += (bytes + 15) & ~(size_t)15; return at; };
    const size_t o_kps1 = take(N1 * sizeof(orbx_kp)), o_kps2 = take(N2 * sizeof(orbx_kp)), o_m = take(N1 * 4), o_sets = take(sets ? I * 32 : 0);
    const size_t in_end = total;
    const size_t o_res = take(32), o_pairs = take(N1 * 8), o_H = take(36), o_F = take(36), o_iH = take(N1), o_iF = take(N1), o_sc = take(8), o_rh = take(4);
    const size_t o_hyp = take(hyp ? I * 72 : 0), o_hs = take(hyp_score ? I * 8 : 0);
    void *dev = nullptr, *pin = nullptr;
    hipStream_t s = nullptr;
    ORB_TRY(orbm_host_stage(h, total, &dev, &pin, &s));
    char *d = (char *)dev, *p = (char *)pin;
    memcpy(p + o_kps1, kps1, N1 * sizeof(orbx_kp)), memcpy(p + o_kps2, kps2, N2 * sizeof(orbx_kp)), memcpy(p + o_m, matches12, N1 * 4);
    if (sets) memcpy(p + o_sets, sets, I * 32);
    ORB_TRY(hipMemcpyAsync(d, p, in_end, hipMemcpyHostToDevice, s));
    if (int rc = launch(h, s, d + o_kps1, n1, d + o_kps2, n2, (const int32_t *)(d + o_m), sigma, iters, rng_state,
                        sets ? (const int32_t *)(d + o_sets) : nullptr, (int32_t *)(d + o_pairs), (float *)(d + o_H), (float *)(d + o_F),
                        (uint8_t *)(d + o_iH), (uint8_t *)(d + o_iF), (float *)(d + o_sc), (float *)(d + o_rh), hyp ? (float *)(d + o_hyp) : nullptr,
                        hyp_score ? (float *)(d + o_hs) : nullptr, (int32_t *)(d + o_res)))
        return rc;
    ORB_TRY(hipMemcpyAsync(p + in_end, d + in_end, total - in_end, hipMemcpyDeviceToHost, s));
    ORB_TRY(hipStreamSynchronize(s));
    memcpy(result, p + o_res, 32);
    if (result[1] == 1) return ORBX_OK;   // fewer than 8 matches: only `result` is written
    memcpy(pairs, p + o_pairs, N1 * 8), memcpy(H, p + o_H, 36), memcpy(F, p + o_F, 36), memcpy(inl_H, p + o_iH, N1), memcpy(inl_F, p + o_iF, N1);
    memcpy(score, p + o_sc, 8), memcpy(rh, p + o_rh, 4);
    if (hyp) memcpy(hyp, p + o_hyp, I * 72);
    if (hyp_score) memcpy(hyp_score, p + o_hs, I * 8);
    return ORBX_OK;
}
