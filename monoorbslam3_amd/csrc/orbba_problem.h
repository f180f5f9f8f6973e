// What the host-pointer BA entry points (orbba.hip) do to an orbba_problem before a device is looked for: the null and size checks,
// and THE host index builder -- orbba_linearize, orbba_optimize and orbba_local_bundle_adjustment all call it, and
// orbba_local_bundle_adjustment_device builds the same arrays with its k_lmi_* kernels.  Plain C++17 without a HIP include, so
// that tests/cpp/ba_index.cpp compiles it alone with a host compiler (tests/test_ba_abi.py).
#pragma once
#include <stddef.h>

#include <vector>

#include "../../include/orbba.h"
#include "../../include/orbx.h"

namespace {

// an entry point's answer to its arguments: ORBX_OK, or the code and the text of orbx_last_error()
struct BaVerdict {
    int code;
    const char *text;
};

inline bool ba_sizes_ok(const orbba_problem *p, int min_edges) { return p->n_poses >= 1 && p->n_points >= 1 && p->n_edges >= min_edges; }
inline bool ba_arrays_ok(const orbba_problem *p)
{
    return p->pose_R && p->pose_t && p->pose_fixed && p->points &&
           (!p->n_edges || (p->edge_pose && p->edge_point && p->edge_z && p->edge_inv_sigma2));
}
// sizes and arrays of a host-pointer problem; orbba_linearize alone takes a problem without edges (min_edges = 0)
inline BaVerdict ba_check_problem(const orbba_problem *p, int min_edges)
{
    if (!ba_sizes_ok(p, min_edges)) return {ORBX_E_ARG, "bad sizes"};
    if (!ba_arrays_ok(p)) return {ORBX_E_ARG, "null input array"};
    return {ORBX_OK, nullptr};
}

// Index structures of a problem, each a function of pose_fixed, edge_pose and edge_point alone:
//   pose_off [n_poses + 1], pose_edges [n_edges]   the edges of each pose (CSR), in edge order
//   point_off [n_points + 1]                       the contiguous edge range of each point
// and for the LM loop (`lm`):
//   free_pose [n_free], pose_slot [n_poses]        the poses that are not fixed, and each pose's place among them (-1: fixed)
//   edge_of [n_free x n_points]                    the edge of a free pose and a point, -1 where there is none
struct BaIndex {
    std::vector<int> pose_off, pose_edges, point_off, free_pose, pose_slot, edge_of;
};

// Checks the content of a problem that passed ba_check_problem and builds its index.  "every pose is fixed" (lm) comes first; the
// edges are then walked in edge order and the first offending edge decides: index out of range, point below its predecessor's, and
// (lm) a second edge of the same free pose and point.  ORBX_E_UNSUPPORTED, when edge_of would exceed 2^28 cells, comes behind
// every argument error.  On an error *ix is left half built.
inline BaVerdict ba_build_index(const orbba_problem *p, bool lm, BaIndex *ix)
{
    const int NP = p->n_poses, NL = p->n_points, NE = p->n_edges;
    ix->pose_off.assign((size_t)NP + 1, 0);
    ix->point_off.assign((size_t)NL + 1, 0);
    ix->pose_edges.resize((size_t)NE);
    ix->free_pose.clear();
    ix->pose_slot.clear();
    ix->edge_of.clear();
    if (lm) {
        ix->pose_slot.assign((size_t)NP, -1);
        for (int i = 0; i < NP; ++i)
            if (!p->pose_fixed[i]) { ix->pose_slot[i] = (int)ix->free_pose.size(); ix->free_pose.push_back(i); }
        if (ix->free_pose.empty()) return {ORBX_E_ARG, "every pose is fixed: nothing to optimise"};
    }
    // edge_of is filled on the way when it may be that large; the limit itself is reported behind the walk
    const size_t NF = ix->free_pose.size();
    const bool fits = NF * (size_t)NL <= (size_t)1 << 28;
    if (lm && fits) ix->edge_of.assign(NF * (size_t)NL, -1);
    // the edges of a point are contiguous, so a free pose observes a point twice exactly when its previous edge had that point too
    std::vector<int> last_point(lm ? (size_t)NP : 0, -1);
    for (int e = 0; e < NE; ++e) {
        const int ip = p->edge_pose[e], il = p->edge_point[e];
        if (ip < 0 || ip >= NP || il < 0 || il >= NL) return {ORBX_E_ARG, "edge index out of range"};
        if (e && il < p->edge_point[e - 1]) return {ORBX_E_ARG, "edges must be grouped by point"};
        if (lm && ix->pose_slot[ip] >= 0) {
            if (last_point[ip] == il) return {ORBX_E_ARG, "a point is observed twice by the same key frame"};
            last_point[ip] = il;
            if (fits) ix->edge_of[(size_t)ix->pose_slot[ip] * NL + il] = e;
        }
        ix->pose_off[ip + 1]++;
        ix->point_off[il + 1]++;
    }
    if (lm && !fits) return {ORBX_E_UNSUPPORTED, "free poses x points table too large"};
    for (int i = 0; i < NP; ++i) ix->pose_off[i + 1] += ix->pose_off[i];
    for (int i = 0; i < NL; ++i) ix->point_off[i + 1] += ix->point_off[i];
    std::vector<int> fill(ix->pose_off.begin(), ix->pose_off.end() - 1);
    for (int e = 0; e < NE; ++e) ix->pose_edges[fill[p->edge_pose[e]]++] = e;
    return {ORBX_OK, nullptr};
}

} // namespace
