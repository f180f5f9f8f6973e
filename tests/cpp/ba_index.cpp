// The host index builder of the BA entry points (monoorbslam3_amd/csrc/orbba_problem.h) on its own, without HIP or the library:
// reads one problem from stdin and prints the builder's verdict and the six index arrays (tests/test_ba_abi.py).
//   in:  lm n_poses n_points n_edges, then n_poses pose_fixed, n_edges edge_pose, n_edges edge_point (all integers)
//   out: "status <code>", "message <text>", then one line per array: name and its values
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "orbba_problem.h"

static void print(const char *name, const std::vector<int> &v)
{
    printf("%s", name);
    for (int x : v) printf(" %d", x);
    printf("\n");
}

int main()
{
    int lm = 0, NP = 0, NL = 0, NE = 0;
    if (scanf("%d %d %d %d", &lm, &NP, &NL, &NE) != 4 || NP < 0 || NL < 0 || NE < 0) return 2;
    std::vector<uint8_t> fixed((size_t)NP);
    std::vector<int32_t> ep((size_t)NE), el((size_t)NE);
    std::vector<double> reals(9 * (size_t)NP + 3 * (size_t)NL + 2 * (size_t)NE + 1); // never read by the builder: only not NULL
    int v = 0;
    for (int i = 0; i < NP; ++i) { if (scanf("%d", &v) != 1) return 2; fixed[i] = (uint8_t)v; }
    for (int e = 0; e < NE; ++e) if (scanf("%d", &ep[e]) != 1) return 2;
    for (int e = 0; e < NE; ++e) if (scanf("%d", &el[e]) != 1) return 2;
    orbba_problem p = {};
    p.n_poses = NP, p.n_points = NL, p.n_edges = NE;
    p.pose_R = p.pose_t = p.points = p.edge_z = p.edge_inv_sigma2 = reals.data();
    p.pose_fixed = fixed.data(), p.edge_pose = ep.data(), p.edge_point = el.data();
    BaIndex ix;
    BaVerdict verdict = ba_check_problem(&p, lm ? 1 : 0);
    if (!verdict.code) verdict = ba_build_index(&p, lm != 0, &ix);
    printf("status %d\nmessage %s\n", verdict.code, verdict.text ? verdict.text : "");
    if (verdict.code) return 0;
    print("pose_off", ix.pose_off);
    print("pose_edges", ix.pose_edges);
    print("point_off", ix.point_off);
    print("free_pose", ix.free_pose);
    print("pose_slot", ix.pose_slot);
    print("edge_of", ix.edge_of);
    return 0;
}
