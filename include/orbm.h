/*
 * orbm.h -- C ABI of the MI355X ORB matcher cores (liborbx.so).
 *
 * Drop-in boundary for the reference's ORBMatcher
 * (modules/ORB/ORBMatcher.h:12-52, modules/ORB/ORBMatcher.cpp).  The 256-bit
 * Hamming brute force of every Search* routine runs as HIP kernels (the dense best / second-best search on the
 * matrix pipe; the window searches with Frame::grid and getFeaturesInArea on the device as well); the greedy,
 * order-dependent resolution (which mutates Frame/KeyFrame/MapPoint objects in
 * the reference) consumes the device-computed distances on the host so that the
 * results are identical to the reference's sequential loops.
 * The header-only shim monoorbslam3_amd/compat/ORBMatcher.h maps the
 * reference's Frame/KeyFrame types onto these plain-array entry points.
 *
 * Returns 0 or a negative ORBX_E_* code (orbx.h); text in orbx_last_error().
 * All entry points are re-entrant: a handle owns its (non-blocking) stream and scratch, and the
 * reference calls SearchForTriangulation and the fuse from the LocalMapping thread while
 * Tracking calls SearchByBow / SearchByProjection (LocalMapping.cpp:168, 282, 301; Tracking.cpp:262, 289) -- use one
 * handle per thread; handles never wait for each other (orbx.h, "Streams and threads"; tests/cpp/two_threads.cpp).
 */
#ifndef ORBM_H
#define ORBM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBM_TH_LOW 50        /* modules/ORB/ORBMatcher.cpp:13 */
#define ORBM_TH_HIGH 100      /* modules/ORB/ORBMatcher.cpp:14 */
#define ORBM_HISTO_LENGTH 30  /* modules/ORB/ORBMatcher.cpp:15 */

typedef struct orbm_ctx orbm_t;

int orbm_create(int device, orbm_t **out);
void orbm_destroy(orbm_t *h);
/* Kernel-choice switches per handle (parity twins; no reference counterpart).  They replace the ORBM_BEST2 / ORBM_WINDOW
 * environment variables of earlier builds.  Unknown switch / value out of range: ORBX_E_ARG. */
#define ORBM_VAR_BEST2 0   /* dense best / second-best: 0 FP4 matrix path k_best2_fp4 (default), 1 i8 matrix path k_best2_mfma, 2 VALU k_best2 */
#define ORBM_VAR_WINDOW 1  /* window searches of the host entry points: 0 grid and lists on the device (default), 1 host grid */
#define ORBM_VAR_BEST2_RESIDENT 2 /* k_best2_fp4's grid: 0 one workgroup per (problem, 512 queries) (default); 1 or 2: that many
                                   * workgroups per CU walk the blocks, so the kernel holds a fixed share of every CU (half of the
                                   * registers and 37 KB of LDS per workgroup) -- for a caller that runs it beside other kernels */
#define ORBM_VAR_INIT_LANES 3 /* orbm_search_for_initialization_device: lanes that share one query's window list in the resolve kernel:
                              * 0 chosen from the mean list length (default), or 1, 4, 16, 64 (the parity twins) */
#define ORBM_VAR_INIT_MAX_SWEEPS 4 /* orbm_search_for_initialization_device: sweeps of the fixed point before it gives up (d_result[1]
                                    * = 2): 0 = ORBM_INIT_MAX_SWEEPS (default), or 1 .. ORBM_INIT_MAX_SWEEPS */
int orbm_set_variant(orbm_t *h, int which, int value);

/* DBoW2::FeatureVector (thirdParty/DBoW2/DBoW2/FeatureVector.h) flattened to CSR:
 * node ids ascending, indices of a node in insertion (ascending feature) order. */
typedef struct orbm_fv {
    int32_t n_nodes;
    const uint32_t *node_ids;
    const int32_t *offsets; /* n_nodes + 1 */
    const uint32_t *indices;
} orbm_fv;

/* ORBMatcher::DescriptorDistance (modules/ORB/ORBMatcher.cpp:17-31) for all pairs:
 * out[i*nb + j] = popcount(a[i] ^ b[j]), 0..256.  Host pointers. */
int orbm_hamming_matrix(orbm_t *h, const uint8_t *a, int na, const uint8_t *b, int nb, uint16_t *out);
/* same with device pointers, enqueued on `stream` (hipStream_t; NULL: orbx.h, "Streams") */
int orbm_hamming_matrix_device(orbm_t *h, const uint8_t *d_a, int na, const uint8_t *d_b, int nb, uint16_t *d_out,
                               void *stream);

/* Best / second-best of every query row among the candidate rows, the inner loop of
 * SearchByBow (ORBMatcher.cpp:148-162): strict '<' updates in ascending candidate order,
 * both distances start at 256, best index -1 when no candidate.  row_ok / col_ok
 * (may be NULL) are byte masks: skipped queries return (-1,256,256); masked candidates
 * are not considered.  `n_pairs` independent (A,B) problems are processed in one launch:
 * problem p uses a + p*a_stride ... (strides in descriptors/elements).  Device pointers.
 * Which kernel runs: problems without a candidate mask (d_col_ok == NULL) and nb_max <= 8160 take a matrix-pipe
 * kernel (k_best2_fp4, or k_best2_mfma with ORBM_VAR_BEST2 = 1); a candidate mask, more candidates, or ORBM_VAR_BEST2 = 2
 * take the VALU kernel (k_best2).  All three give the same outputs; only the speed differs. */
int orbm_best2_device(orbm_t *h, int n_pairs, const uint8_t *d_a, size_t a_stride, const int32_t *d_na, int na_max,
                      const uint8_t *d_b, size_t b_stride, const int32_t *d_nb, int nb_max,
                      const uint8_t *d_row_ok, const uint8_t *d_col_ok, int32_t *d_best_idx, uint16_t *d_best,
                      uint16_t *d_second, void *stream);
/* host-pointer convenience wrapper for one problem */
int orbm_best2(orbm_t *h, const uint8_t *a, int na, const uint8_t *b, int nb, const uint8_t *row_ok,
               const uint8_t *col_ok, int32_t *best_idx, uint16_t *best, uint16_t *second);

/* Distances for explicit candidate lists (CSR): for query q (descriptor a[q_idx[q]]) and
 * t in [off[q], off[q+1]): out[t] = hamming(a[q_idx[q]], b[c_idx[t]]).  Host pointers.
 * This is the device primitive under every window / BoW-node search. */
int orbm_hamming_csr(orbm_t *h, const uint8_t *a, int na, const uint8_t *b, int nb, const int32_t *q_idx,
                     const int32_t *off, int n_queries, const int32_t *c_idx, uint16_t *out);

/* ORBMatcher::SearchByBow(keyFrame, frame) (modules/ORB/ORBMatcher.cpp:118-201).
 * kf_mp_ok[i] != 0 <=> keyFrame->getMapPoints()[i] is non-null and not bad (:143).
 * frame_mp[j] (in/out): -1 where frame->map_points[j] is null; on return matched
 * entries hold the key-frame feature index whose MapPoint the reference would assign (:165).
 * Returns the match count through n_matches. */
int orbm_search_by_bow(orbm_t *h, float nn_ratio, int check_orientation,
                       const uint8_t *desc1, const float *angle1, const uint8_t *kf_mp_ok, int n1, const orbm_fv *fv1,
                       const uint8_t *desc2, const float *angle2, int32_t *frame_mp, int n2, const orbm_fv *fv2,
                       int *n_matches);

/* ORBMatcher::SearchForTriangulation(kf1, kf2, matches12) (modules/ORB/ORBMatcher.cpp:417-522),
 * including its `bestIdx2 > 0` acceptance rule (:484).  has_mp1/2[i] != 0 <=> hasMapPoint(i). */
int orbm_search_for_triangulation(orbm_t *h, int check_orientation,
                                  const uint8_t *desc1, const float *angle1, const uint8_t *has_mp1, int n1,
                                  const orbm_fv *fv1,
                                  const uint8_t *desc2, const float *angle2, const uint8_t *has_mp2, int n2,
                                  const orbm_fv *fv2, int32_t *matches12, int *n_matches);

/* ORBMatcher::SearchForInitialization(frame1, frame2, vecPreMatched, matches12, windowSize)
 * (modules/ORB/ORBMatcher.cpp:33-116) with Frame::getFeaturesInArea (Frame.cpp:97-127) over
 * plain arrays.  kps are orbx_kp-layout records (28 bytes).  prematched: n1 (x,y) pairs, in/out. */
int orbm_search_for_initialization(orbm_t *h, float nn_ratio, int check_orientation,
                                   const void *kps1, const uint8_t *desc1, int n1,
                                   const void *kps2, const uint8_t *desc2, int n2,
                                   int img_w, int img_h, float *prematched_xy, int32_t *matches12,
                                   int window_size, int *n_matches);

/* ORBMatcher::SearchByProjection(lastFrame, curFrame, th) and (lastKF, curFrame, th)
 * (modules/ORB/ORBMatcher.cpp:203-274 and :276-348 -- the two bodies are the same loop).  The caller (shim)
 * keeps the camera / pose maths: for every feature i of the last frame it passes q_ok[i] = 1 iff the feature has
 * a live MapPoint whose projection is in front of the camera and inside the image (:213-224), the projection
 * q_xy, the radius th * key_points[i].size, the octave (window levels octave-1 .. octave+1, :226-229), the
 * MapPoint descriptor and the key-point angle.  frame_mp (in/out): -1 where curFrame->map_points[j] is null,
 * any other value = occupied; matched entries are set to the query index i (:245).  kps2 = orbx_kp records. */
int orbm_search_by_projection_frame(orbm_t *h, int check_orientation,
                                    const uint8_t *q_desc, const float *q_xy, const float *q_radius,
                                    const int32_t *q_octave, const float *q_angle, const uint8_t *q_ok, int nq,
                                    const void *kps2, const uint8_t *desc2, int n2, int img_w, int img_h,
                                    int32_t *frame_mp, int *n_matches);

/* ORBMatcher::SearchByProjection(frame, mapPoints, th) (modules/ORB/ORBMatcher.cpp:350-415).  q_ok[i] = 1 iff
 * mp->track_in_view && !mp->isBad() (:355); q_xy = (track_proj_x, track_proj_y); q_radius = the radius computed at
 * :362-365; q_level = track_scale_level (window levels level-1 .. level, :367-369).  frame_mp (in/out): -1 where
 * frame->map_points[j] is null OR bad (such slots may be taken, :383), anything else = occupied by a good point;
 * matched entries are set to the query index.  counters[3] = {numOutViewAndBad, fail1, fail2} (:353, :403, :408). */
int orbm_search_by_projection_points(orbm_t *h, float nn_ratio,
                                     const uint8_t *q_desc, const float *q_xy, const float *q_radius,
                                     const int32_t *q_level, const uint8_t *q_ok, int nq,
                                     const void *kps2, const uint8_t *desc2, int n2, int img_w, int img_h,
                                     int32_t *frame_mp, int *n_matches, int32_t *counters);

/* static ORBMatcher::SearchByProjection(keyFrame, mapPoints, Map *pointMap, th) -- the map-point fuse that
 * LocalMapping.cpp:282,301 calls (modules/ORB/ORBMatcher.h:44-45, ORBMatcher.cpp:524-592).  This entry point is the part
 * of the loop body that reads no MapPoint / KeyFrame state: for map point i with q_ok[i] = 1 (the caller evaluated
 * :534-552: projection in front of the camera and in the image, distance invariance, viewing angle) it walks
 * KeyFrame::getFeaturesInArea(p.x, p.y, radius, predictLevel-1, predictLevel) (KeyFrame.cpp:181-211, STRICT window
 * test), drops key points whose squared re-projection error exceeds 5.991 * sigma2[octave] (:566-567, float against
 * double) and returns the closest descriptor with distance < TH_LOW + 1 (:560, :569-574, first on ties):
 * best_idx[i] = key-point index or -1, best_dist[i] = its distance (TH_LOW + 1 when none).  q_radius[i] =
 * th * scale_factor[predictLevel] (:555), sigma2 = ORBExtractor::getSquareSigmas() (n_levels entries).
 * The caller replays :534 (null / bad / already observed, evaluated live) and :577-591 (addObservation / replace)
 * in map-point order on its own objects -- see compat/ORBMatcher.h. */
int orbm_search_fuse(orbm_t *h, const uint8_t *q_desc, const float *q_xy, const float *q_radius,
                     const int32_t *q_level, const uint8_t *q_ok, int nq,
                     const void *kps, const uint8_t *desc, int n, int img_w, int img_h,
                     const float *sigma2, int n_levels, int32_t *best_idx, int32_t *best_dist, int *n_found);

/* Frame / KeyFrame::getFeaturesInArea (modules/BasicObject/Frame.cpp:97-127, KeyFrame.cpp:181-211) plus the descriptor
 * distance of every hit, for nq queries against ONE device-resident frame record: d_kps / d_desc as written by
 * orbx_extract_batch_device (undistorted key points: orbf's d_kp_un), d_cell_start / d_cell_items = the CSR grid of
 * orbf_frame_post_device (grid_cols x grid_rows cells of 40 px, cell id = cx * grid_rows + cy).  Query q: centre
 * d_q_xy[2q..], radius d_q_radius[q], levels d_q_min_level[q] .. d_q_max_level[q] with the reference's beCheckLevel rule
 * (Frame.cpp:107), d_q_ok[q] = 0 switches it off.  strict != 0 = KeyFrame's `< r` test; d_sigma2 != NULL drops hits whose
 * squared distance to the centre exceeds 5.991 * d_sigma2[octave] (the fuse, ORBMatcher.cpp:566-567).
 * d_lists[q * cap + p] = distance << 22 | key-point index for the p-th hit in the reference's list order (cx outer, cy
 * inner, ascending index inside a cell), p < cap; d_counts[q] = the full list length (may exceed cap), -1 for a query
 * that is off.  Every pointer is device memory; enqueued on `stream` (NULL: orbx.h, "Streams").  This is the primitive under
 * the four window searches above, which wrap it with one staging copy each way when called with host pointers. */
int orbm_window_lists_device(orbm_t *h, const void *d_kps, const uint8_t *d_desc, const int32_t *d_cell_start,
                             const int32_t *d_cell_items, int grid_cols, int grid_rows, const uint8_t *d_q_desc,
                             const float *d_q_xy, const float *d_q_radius, const int32_t *d_q_min_level,
                             const int32_t *d_q_max_level, const uint8_t *d_q_ok, int nq, int strict,
                             const float *d_sigma2, int cap, int32_t *d_counts, uint32_t *d_lists, void *stream);

/* SearchByBow (Tracking.cpp:262 -> ORBMatcher.cpp:118-201) and SearchForTriangulation (LocalMapping.cpp:168 -> :417-522) on
 * device-resident records, greedy pass included: descriptors and key-point records (orbx_kp: the angle is read from them) as
 * orbx_extract_batch_device leaves them, the two
 * FeatureVectors as orbv_transform_device leaves them (node ids ascending, CSR offsets, feature indices, the node COUNT in device
 * memory), so the BoW branch of the tracking thread -- extract, computeBow, SearchByBow -- has no host hop either.
 *   d_kf_mp_ok [n1]   key-frame features that have a live map point (:141-146): the queries
 *   d_frame_mp [n2]   in / out as in the host entry point: -1 = free; a match writes the key-frame feature index
 *   d_has_mp1 / d_has_mp2: features that already have a map point (skipped, :452 / :466); d_matches12 [n1] receives the matches
 *     (the flags are the caller's: orbm_triangulate_matches_device sets them for the rows it appends, no other call of the mapper step
 *     touches them, so ahead of a step's first search they are derived from the key frame's slot row: slot >= 0)
 * A feature of side 2 lies in one vocabulary node, so the reference's order-dependent loop only couples queries of the same
 * node: every node is resolved by its own workgroup with the fixed point of the projection searches below, on the 8 closest
 * initially-free candidates per query (a query whose list is used up rescans its node on the device).  Rotation histogram
 * (the reference's 1/30 factor) and ComputeThreeMaxima on the device as well.
 * d_result (int32 x 8, device): [0] matches, [1] = 1 if a shared node holds more than 4096 features on a side -- found before
 * anything is written: NOTHING was changed then (frame_mp as passed, matches12 all -1, no match counted), as the projection
 * searches below guarantee on overflow, so the host entry point can take over on the same arrays --, [2] the most sweeps a
 * node needed, [3] matches before the rotation filter.
 * One call in flight per handle (the scratch is the handle's).  Enqueued on `stream` (NULL: orbx.h, "Streams"); no host wait. */
int orbm_search_by_bow_device(orbm_t *h, float nn_ratio, int check_orientation, const uint8_t *d_desc1, const void *d_kps1,
                              const uint8_t *d_kf_mp_ok, int n1, const uint32_t *d_fv1_nodes, const int32_t *d_fv1_off,
                              const uint32_t *d_fv1_idx, const int32_t *d_n_fv1, const uint8_t *d_desc2, const void *d_kps2,
                              int32_t *d_frame_mp, int n2, const uint32_t *d_fv2_nodes, const int32_t *d_fv2_off,
                              const uint32_t *d_fv2_idx, const int32_t *d_n_fv2, int32_t *d_result, void *stream);
int orbm_search_for_triangulation_device(orbm_t *h, int check_orientation, const uint8_t *d_desc1, const void *d_kps1,
                                         const uint8_t *d_has_mp1, int n1, const uint32_t *d_fv1_nodes, const int32_t *d_fv1_off,
                                         const uint32_t *d_fv1_idx, const int32_t *d_n_fv1, const uint8_t *d_desc2,
                                         const void *d_kps2, const uint8_t *d_has_mp2, int n2, const uint32_t *d_fv2_nodes,
                                         const int32_t *d_fv2_off, const uint32_t *d_fv2_idx, const int32_t *d_n_fv2,
                                         int32_t *d_matches12, int32_t *d_result, void *stream);

/* The two SearchByProjection calls of the tracking thread (Tracking.cpp:289-336) on a device-resident frame record, greedy
 * pass included (modules/ORB/ORBMatcher.cpp:229-246 and :379-407): nothing returns to the host between the extraction,
 * orbf_frame_post_device and the matched map points.  Queries (device arrays, as the host entry points above take them):
 * descriptors, projections, radii, octave / predicted level, angle (frame -> frame only), q_ok.  The frame: d_kps2 / d_desc2 /
 * CSR grid as for orbm_window_lists_device, n2 key points.  d_frame_mp [n2], in/out, the meaning of the host entry points:
 * -1 = free, anything else = occupied; matched entries receive the query index.
 * The greedy order of the reference -- query i takes its closest candidate not taken by a query before it -- is reproduced
 * by a fixed-point iteration on the device (every query re-chooses among the candidates no EARLIER query currently holds,
 * until nothing changes); the rotation histogram and ComputeThreeMaxima (:594-622) run there too.
 * list_cap = the pool of window-list entries is nq * list_cap (48 covers the tracking radii; the reference's lists have
 * no bound).  d_result (int32 x 8, device): [0] matches (the return value), [1] = 1 if the lists did not fit the pool --
 * then nothing was changed and the call is to be repeated with a larger list_cap --, [2] sweeps of the fixed point,
 * [3] window-list entries; map points -> frame: [4] numOutViewAndBad, [5] fail1, [6] fail2 (:353-354).
 * nq + n2 <= 38400.  Enqueued on `stream` (NULL: orbx.h, "Streams"); no host synchronisation -- with two provisos: the packed
 * lists live in the handle's scratch, so ONE call may be in flight per handle (use a handle per thread / per stream), and the
 * first call that needs a larger scratch (nq * list_cap grew) reallocates it, which waits for the device once.  When the lists
 * overflow the pool ([1] = 1) d_frame_mp is left as it was: a chain that goes on to orbba_pose_edges_device then optimises the
 * pose on the matches d_frame_mp already held -- size list_cap so that this cannot happen (48 covers the tracking radii at 2000
 * features; the window of a lost-track search needs more), or read d_result back before trusting the pose. */
int orbm_search_by_projection_frame_device(orbm_t *h, int check_orientation, const uint8_t *d_q_desc, const float *d_q_xy,
                                           const float *d_q_radius, const int32_t *d_q_octave, const float *d_q_angle,
                                           const uint8_t *d_q_ok, int nq, const void *d_kps2, const uint8_t *d_desc2,
                                           const int32_t *d_cell_start, const int32_t *d_cell_items, int grid_cols, int grid_rows,
                                           int n2, int list_cap, int32_t *d_frame_mp, int32_t *d_result, void *stream);
int orbm_search_by_projection_points_device(orbm_t *h, float nn_ratio, const uint8_t *d_q_desc, const float *d_q_xy,
                                            const float *d_q_radius, const int32_t *d_q_level, const uint8_t *d_q_ok, int nq,
                                            const void *d_kps2, const uint8_t *d_desc2, const int32_t *d_cell_start,
                                            const int32_t *d_cell_items, int grid_cols, int grid_rows, int n2, int list_cap,
                                            int32_t *d_frame_mp, int32_t *d_result, void *stream);

/* SearchForInitialization (modules/ORB/ORBMatcher.cpp:33-116) on device-resident records: frame 1's key points / descriptors and
 * frame 2's undistorted record + CSR grid as orbf_frame_post_device leaves it.  d_pre [n1][2] is vecPreMatched, in / out (:112-114);
 * d_matches12 [n1] receives the matches (-1 = none).  The window lists (getFeaturesInArea(pre, windowSize, level1, level1) of the
 * level-0 features), the order-dependent matching with its stealing rule (:63, :75-81), the rotation histogram -- robbed queries
 * stay in it, as in the reference -- and ComputeThreeMaxima all run on the device; the result equals the host entry point's.
 * Limits: n2 + 5 n1 <= 38400 (the claims live in LDS), list_cap entries per query on average (pool of n1 * list_cap).
 * d_result (int32 x 8): [0] matches, [1] = 1 when the lists overflowed the pool (d_matches12 all -1, d_pre untouched: repeat with
 * a larger list_cap or use the host entry point), [1] = 2 when the fixed point had not settled after ORBM_INIT_MAX_SWEEPS sweeps
 * (ORBM_VAR_INIT_MAX_SWEEPS lowers the cap; same guarantee: nothing written; use the host entry point), [2] sweeps of the fixed
 * point (the cap when [1] = 2), [3] list entries.
 * Cost: ONE workgroup resolves the search; a sweep walks every level-0 feature's window list (1, 4 or 16 lanes share a list,
 * chosen from the mean list length: ORBM_VAR_INIT_LANES) and, per entry, the chain of queries that claim that candidate.  Measured
 * device time of the whole call (profiles/r06_match_latency.txt): 0.11 ms on two extracted views (22 entries per list, 3 sweeps; the
 * host entry point 0.17 ms), 1.2 ms on a crowded scene of near-duplicates (900 x 850 features in 260 x 200 px: 390 entries per
 * list, 5 sweeps; host 0.5 ms -- there the host entry point is the faster one), 5 ms with every feature of both frames in ONE window
 * (2000-entry lists; host 10 ms).  The proof bounds the sweeps by n1 + 1; ORBM_INIT_MAX_SWEEPS keeps a pathological scene from
 * holding a CU for longer than that.
 * Enqueued on `stream` (NULL: orbx.h, "Streams"); one call in flight per handle. */
#define ORBM_INIT_MAX_SWEEPS 64
int orbm_search_for_initialization_device(orbm_t *h, float nn_ratio, int check_orientation, const void *d_kps1, const uint8_t *d_desc1,
                                          int n1, const void *d_kps2, const uint8_t *d_desc2, const int32_t *d_cell_start2,
                                          const int32_t *d_cell_items2, int grid_cols, int grid_rows, int n2, float *d_pre,
                                          int window_size, int list_cap, int32_t *d_matches12, int32_t *d_result, void *stream);

/* The per-point search of the static fuse SearchByProjection(keyFrame, mapPoints, Map*, th) (ORBMatcher.cpp:556-575) on a
 * device-resident key-frame record (key points, descriptors, CSR grid): KeyFrame::getFeaturesInArea(p, radius, predictLevel - 1,
 * predictLevel) with its strict window test, the chi-square gate of :566-567 (d_sigma2 = the level table of square sigmas, indexed
 * by the key point's octave) and the closest descriptor below TH_LOW + 1.  d_best_idx [nq] (-1 = none) / d_best_dist [nq]; what
 * the reference does with a hit (:577-589) mutates its objects and stays with the caller (compat/ORBMatcher.h), or with
 * orbm_fuse_apply_device below for a caller that keeps the slot arrays on the device.
 * d_result (int32 x 8): [0] points with a hit, [1] = 1 if a window held more than list_cap hits (that point's answer is then
 * taken from the first list_cap: repeat with a larger list_cap).  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
int orbm_search_fuse_device(orbm_t *h, const uint8_t *d_q_desc, const float *d_q_xy, const float *d_q_radius, const int32_t *d_q_level,
                            const uint8_t *d_q_ok, int nq, const void *d_kps, const uint8_t *d_desc, const int32_t *d_cell_start,
                            const int32_t *d_cell_items, int grid_cols, int grid_rows, const float *d_sigma2, int list_cap,
                            int32_t *d_best_idx, int32_t *d_best_dist, int32_t *d_result, void *stream);

/* ---- Projection-search queries built on the device -------------------------------------------------------------------------
 * The three builders below turn a map-point table and a pose, both in device memory, into the query arrays the three projection
 * searches above take (d_q_xy, d_q_radius, d_q_level / d_q_octave, d_q_angle, d_q_ok, in their layouts), so that a search whose
 * queries depend on a pose the device has just computed -- the second stage of Tracking.cpp:386-427 reads the pose that
 * orbba_pose_optimize_batch_device left -- needs no read-back, host loop and upload.  They are for callers that keep a map-point
 * table on the device; the reference-signature shims (compat/ORBMatcher.h) keep their host loop over MapPoint objects.
 *
 * Camera: a host struct, copied into the launch's arguments.  min_x .. max_y are the bounds isInImage tests with `<` / `>=`
 * (Pinhole.cpp:44-47; Fisheye.cpp:75-78: pass 0, width, 0, height).
 * Pose: d_pose_R (9 doubles, row major) / d_pose_t (3 doubles) as orbba_pose_optimize_batch_device writes them.  The kernel rounds
 * them to float first (the reference's Pose is Matrix3f / Vector3f, Optimize.cpp:528-529); everything after that is float.
 * Map points, structure of arrays with nq entries: d_points [nq][3] getPos(), d_valid [nq] (non-null and not bad), and for the
 * frustum and fuse forms d_normals [nq][3] getAverageDirection(), d_min_dist / d_max_dist [nq] get{Min,Max}DistanceInvariance().
 * Level tables (frustum, fuse): scale_factors (host, n_levels <= 16 floats, ORBExtractor::getScaleFactors()) and
 * log_scale_factor (getLogScaleFactor()), copied into the launch's arguments.
 *
 * Arithmetic (float, -ffp-contract=off: no fused multiply-add), fixed so that it can be checked bit for bit:
 *   Pc_k  = ((R_k0 * x + R_k1 * y) + R_k2 * z) + t_k                          Pose::map (R * Pw + t)
 *   O_w_k = -((R_0k * t_0 + R_1k * t_1) + R_2k * t_2)                         Pose.cpp:12-14
 *   OP = Pw - O_w;  dist = sqrtf((ox * ox + oy * oy) + oz * oz);  OP . Pn = (ox * nx + oy * ny) + oz * nz
 *   Pinhole  u = fx * (X / Z) + cx, v = fy * (Y / Z) + cy                     Pinhole.cpp:34-38
 *   Fisheye  a = X / Z, b = Y / Z, r = sqrtf(a * a + b * b), theta = atanf(r),
 *            theta_d = (((theta + k0 * theta3) + k1 * theta5) + k2 * theta7) + k3 * theta9,
 *            u = ((fx * theta_d) * a) / r + cx                                Fisheye.cpp:52-66 (r = 0 gives NaN, which isInImage lets pass, as there)
 *   level = clamp(ceil(logf(max_dist / dist) / log_scale_factor), 0, n_levels - 1)     MapPoint.cpp:159-170
 * Division and square root are the correctly rounded ones; logf and atanf are the device library's, which are not correctly
 * rounded: a level may differ from another logf's where log(max_dist / dist) / log_scale_factor is within rounding of an integer.
 *
 * Outputs: a query that is switched off has q_ok = 0 and zeros in every other array.  d_result (int32 x 8, device, written --
 * not accumulated -- by the call): [0] queries switched on, then one count per gate that rejected a point, in the reference's
 * order of tests (a point is counted at the first gate that rejects it); unused entries are 0.
 * One launch of one workgroup per call (a few thousand points are latency-bound); the frustum form keeps its "already in the
 * frame" mask in LDS, so no builder uses handle scratch, allocates or waits on the host; a builder followed by its search on the
 * same handle and stream is the intended use.  nq <= 524288 (ORBX_E_UNSUPPORTED above: the mask is one bit per point in 64 KB).
 * Arguments are checked first (ORBX_E_ARG); without a HIP device the call fails with ORBX_E_NO_DEVICE.  nq = 0 is allowed.
 * Enqueued on `stream` (NULL: orbx.h, "Streams"). */
typedef struct orbm_proj_camera {
    int32_t model;                    /* 0 = Pinhole (modules/Sensor/Pinhole.cpp), 1 = Fisheye (Kannala-Brandt, modules/Sensor/Fisheye.cpp) */
    float fx, fy, cx, cy;
    float k[4];                       /* Fisheye dist_coeffs k1..k4; ignored by Pinhole */
    float min_x, max_x, min_y, max_y; /* isInImage: p.x < min_x || p.x >= max_x || p.y < min_y || p.y >= max_y is outside */
} orbm_proj_camera;

/* Frame / key frame -> frame: the per-feature part of SearchByProjection(lastFrame | lastKF, curFrame, th) ahead of the window
 * (modules/ORB/ORBMatcher.cpp:212-229, :276-348; compat/ORBMatcher.h projectionFromFrame).  Point i belongs to feature i of the
 * last frame, whose orbx_kp records are d_kps1: skip if !d_valid[i] (:214-217); Pc = R Pw + t; reject Pc.z < 0 (:221); project;
 * reject outside the image (:224); then q_xy = p, q_radius = th * kps1[i].size, q_octave = kps1[i].octave, q_angle = kps1[i].angle.
 * d_result: [0] on, [1] invalid, [2] negative depth, [3] outside the image. */
int orbm_project_frame_device(orbm_t *h, const orbm_proj_camera *cam, const double *d_pose_R, const double *d_pose_t,
                              const float *d_points, const uint8_t *d_valid, const void *d_kps1, int nq, float th,
                              float *d_q_xy, float *d_q_radius, int32_t *d_q_octave, float *d_q_angle, uint8_t *d_q_ok,
                              int32_t *d_result, void *stream);

/* Local map -> frame: the loop of Tracking.cpp:403-412 with Frame::isInFrustum (modules/BasicObject/Frame.cpp:129-166) and the
 * radius rule of ORBMatcher.cpp:360-365.  d_frame_mp [n2] is the frame's map-point slot per key point in the shared index space
 * orbba_pose_edges_device documents: a point whose index occurs in it is already matched in this frame and is switched off (the
 * `last_frame_seen == current_frame->id` test of Tracking.cpp:404; entries outside [0, nq) are ignored) -- run
 * orbba_pose_drop_outliers_device first, so that the points poseOptimize dropped no longer count as matched.
 * Gates in order: positive depth (Frame.cpp:137), in image (:140), min_dist <= dist <= max_dist (:148),
 * viewCos = OP . Pn / dist >= view_cos_limit (:152-153).  Then level = predictScaleLevel(dist) (:156),
 * q_radius = (th * (viewCos > 0.998 ? 2.5f : 4.f)) * scale_factors[level] (the comparison in double, as ORBMatcher.cpp:363).
 * d_view_cos [nq] (may be NULL) receives track_view_cos.
 * d_result: [0] on (numToMatch, Tracking.cpp:408), [1] invalid, [2] already in the frame, [3] negative depth, [4] outside the image,
 * [5] distance, [6] viewing angle, [7] outView (Tracking.cpp:410) = [3] + [4] + [5] + [6]. */
int orbm_project_frustum_device(orbm_t *h, const orbm_proj_camera *cam, const double *d_pose_R, const double *d_pose_t,
                                const float *d_points, const uint8_t *d_valid, const float *d_normals, const float *d_min_dist,
                                const float *d_max_dist, int nq, const int32_t *d_frame_mp, int n2, const float *scale_factors,
                                int n_levels, float log_scale_factor, float th, float view_cos_limit, float *d_q_xy,
                                float *d_q_radius, int32_t *d_q_level, uint8_t *d_q_ok, float *d_view_cos, int32_t *d_result,
                                void *stream);

/* Map points -> key frame: the tests of the static fuse SearchByProjection(keyFrame, mapPoints, Map*, th) that read no mutable
 * state (ORBMatcher.cpp:536-553).  The three that do (:534: null / bad / already observed by the key frame) stay with the caller
 * through d_valid, as in compat/ORBMatcher.h.  Gates in order: positive depth (:538), in image (:541), distance (:547),
 * OP . Pn < 0.5 * dist rejects (:550).  level = predictScaleLevel(dist), q_radius = th * scale_factors[level] (:552-553).
 * d_result: [0] on, [1] invalid, [2] negative depth, [3] outside the image, [4] distance, [5] viewing angle. */
int orbm_project_fuse_device(orbm_t *h, const orbm_proj_camera *cam, const double *d_pose_R, const double *d_pose_t,
                             const float *d_points, const uint8_t *d_valid, const float *d_normals, const float *d_min_dist,
                             const float *d_max_dist, int nq, const float *scale_factors, int n_levels, float log_scale_factor,
                             float th, float *d_q_xy, float *d_q_radius, int32_t *d_q_level, uint8_t *d_q_ok, int32_t *d_result,
                             void *stream);

/* ---- New map points triangulated on the device -------------------------------------------------------------------------------
 * LocalMapping::createNewMapPoints (modules/Frontend/LocalMapping.cpp:146-259) between SearchForTriangulation and the fuse: for
 * every feature i of key frame 1 (the older one) with d_matches12[i] = m in [0, n2) -- anything else is "no match" --
 * TwoViewReconstruction::Triangulate (TwoViewReconstruction.cpp:689-705), the gates of LocalMapping.cpp:187-241 in their order and,
 * for a match that passes, what the MapPoint constructor and MapPoint::update() leave (MapPoint.cpp:16-30, :43-76), appended to a
 * map-point table in the layout the builders above read.  Key frame 2 is current_kf, the new point's reference key frame.
 * orbm_search_for_triangulation_device -> this call -> orbm_project_fuse_device on one stream needs no host hop; the key frames of
 * one mapper step are coupled through d_has_mp2 (a feature of the current key frame that received a point is skipped by the next
 * search, ORBMatcher.cpp:452, :466), which this call sets.  The baseline / median-depth skip (:163-165) and the Map / KeyFrame
 * bookkeeping (:243-248) stay with the caller.
 *
 * Inputs.  cam, poses (9 + 3 doubles each, rounded to float first), orbx_kp records as for the builders above; key frame 1's pose
 * is (d_pose_R1, d_pose_t1).  d_fisheye_scale: the reference's scale_mat (Fisheye.cpp:21-30), scale_h rows of scale_w floats in
 * device memory, read at [(int) y][(int) x] with the index kept inside the table; NULL (and the sizes ignored) for Pinhole only.
 * d_desc2 [n2][32].  sigma2: host, n_levels <= 16 floats, ORBExtractor::getSquareSigmas(), indexed by the key point's octave
 * (kept inside the table); max_scale_factor = getMaxScaleFactor().  The three thresholds of the reference: cos_parallax = 0.99998
 * and chi2 = 5.991 (double literals there, hence doubles here), ratio_factor = 1.5f * getScaleFactor(1).
 *
 * Arithmetic (float, no fused multiply-add; `/` and sqrtf correctly rounded; project() as documented above):
 *   back-projection  xn = (x - cx) * inv_fx, yn = (y - cy) * inv_fy, inv_fx = 1.f / fx; Fisheye: xn * s, yn * s   Pinhole.cpp:40-42, Fisheye.cpp:68-73
 *   A row 0 / 1 = xn1 * P1.row(2) - P1.row(0) / yn1 * P1.row(2) - P1.row(1), rows 2 / 3 the same of key frame 2, P = [R | t]
 *   Ph = the right singular vector of A's smallest singular value (a one-sided Jacobi in float: not bit-reproducible by another
 *        SVD; see csrc/orbm_triangulate.hip); Ph.w == 0: triangulate fail; Pw = Ph.xyz / Ph.w
 *   O_w as above;  n_v = Pw - O_v, dist_v = sqrtf((x * x + y * y) + z * z), n_v = n_v / dist_v
 *   cosParallax = (n1x * n2x + n1y * n2y) + n1z * n2z, rejected when (double) cosParallax > cos_parallax
 *   Pc = R Pw + t as above, rejected when Pc.z <= 0;  e = (u - x) * (u - x) + (v - y) * (v - y), rejected when
 *        (double) e > (double) sigma2[octave] * chi2
 *   distRatio = dist1 / dist2, levelRatio = sqrtf(sigma2[octave2]) / sqrtf(sigma2[octave1]), rejected when
 *        distRatio * ratio_factor < levelRatio || distRatio > levelRatio * ratio_factor
 *   normal = (n1 + n2) / 2.f;  span = dist2 * kp2.size;  max_dist = 1.2f * span;  min_dist = 0.8f * (span / max_scale_factor)
 *
 * Outputs.  The accepted matches in ascending i -- the reference's creation order -- become the rows *d_n_points, *d_n_points + 1,
 * ... of the table: d_points [cap_points][3], d_valid = 1, d_normals [..][3], d_min_dist / d_max_dist (the ...Invariance values,
 * MapPoint.cpp:83-91), d_desc [..][32] = key frame 2's descriptor row (:28), d_obs [..][2] = (i, m); the row index goes to
 * d_mp1[i] and d_mp2[m] (the key frames' map-point slots, LocalMapping.cpp:245-246; other entries untouched), d_has_mp1[i] =
 * d_has_mp2[m] = 1, and *d_n_points advances.  Rows below the old *d_n_points are not touched.  d_code [n1] (may be NULL)
 * receives the gate code of every feature: -1 no match, 0 accepted, else the index of the counter below.
 * d_result (int32 x 8, written, not accumulated): [0] accepted (numGood), [1] = 1 when the accepted matches do not fit behind
 * *d_n_points in cap_points rows -- found before anything is written: the table, the slots, the flags and the counter are then as
 * passed, [0] is 0, and only d_code and d_result were written --, [2] triangulate fail, [3] illegal (non-finite), [4] small
 * parallax, [5] negative depth (either key frame), [6] re-projection error (either), [7] scale inconsistent.
 * One launch of one workgroup; no handle scratch, allocation or host wait.  d_desc2 and d_desc must be 4-byte aligned.
 * Arguments are checked first (ORBX_E_ARG); without a HIP device the call fails with ORBX_E_NO_DEVICE.  n1 = 0 and a call without
 * any match are allowed.  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
int orbm_triangulate_matches_device(orbm_t *h, const orbm_proj_camera *cam, const float *d_fisheye_scale, int scale_w, int scale_h,
                                    const double *d_pose_R1, const double *d_pose_t1, const double *d_pose_R2, const double *d_pose_t2,
                                    const void *d_kps1, int n1, const void *d_kps2, const uint8_t *d_desc2, int n2,
                                    const int32_t *d_matches12, const float *sigma2, int n_levels, float max_scale_factor,
                                    double cos_parallax, double chi2, float ratio_factor, int32_t *d_n_points, int cap_points,
                                    float *d_points, uint8_t *d_valid, float *d_normals, float *d_min_dist, float *d_max_dist,
                                    uint8_t *d_desc, int32_t *d_obs, int32_t *d_mp1, int32_t *d_mp2, uint8_t *d_has_mp1,
                                    uint8_t *d_has_mp2, int32_t *d_code, int32_t *d_result, void *stream);
/* The same with host pointers throughout (fisheye_scale included), for a caller built on the reference's host objects: synchronous
 * on the handle's stream, one pinned copy each way (the key points' scale entries are gathered on the host, the new rows only
 * come back).  Same bytes as the device entry point. */
int orbm_triangulate_matches(orbm_t *h, const orbm_proj_camera *cam, const float *fisheye_scale, int scale_w, int scale_h,
                             const double *pose_R1, const double *pose_t1, const double *pose_R2, const double *pose_t2,
                             const void *kps1, int n1, const void *kps2, const uint8_t *desc2, int n2, const int32_t *matches12,
                             const float *sigma2, int n_levels, float max_scale_factor, double cos_parallax, double chi2,
                             float ratio_factor, int32_t *n_points, int cap_points, float *points, uint8_t *valid, float *normals,
                             float *min_dist, float *max_dist, uint8_t *desc, int32_t *obs, int32_t *mp1, int32_t *mp2,
                             uint8_t *has_mp1, uint8_t *has_mp2, int32_t *code, int32_t *result);

/* ---- Map points refreshed on the device ----------------------------------------------------------------------------------------
 * The writer of the map-point table the builders and the triangulation above read (d_points, d_valid, d_normals, d_min_dist,
 * d_max_dist, d_desc; cap_points rows, rows at or above cap_points do not exist): what the reference does with
 * `mp->computeDescriptor(); mp->update();` (MapPoint.cpp:103-152, :43-76) for every point of a new key frame (LocalMapping.cpp:93-105),
 * of the current key frame after the fuse (:304-315) and of every bundle adjustment (Optimize.cpp:89, :440, :948, :1305), plus the
 * counting loop of the KeyFrame::updateConnections that follows it (KeyFrame.cpp:233-242) and KeyFrame::computeSceneMedianDepth
 * (KeyFrame.cpp:159-179) for the baseline test ahead of the triangulation (LocalMapping.cpp:163-165).  A caller that keeps the table
 * on the device no longer reads it back after a fuse or a BA.  There is deliberately NO host-pointer twin: the reference-signature
 * shims (compat/) keep their host objects, and orbm_distinctive_descriptors below stays for them.
 *
 * Key frames: a host struct of device pointers, copied into the launch's arguments like orbm_proj_camera.  Poses are rounded to
 * float first, as everywhere in this header.  d_kps[k] / d_desc[k] are key frame k's records as orbx_extract_batch_device /
 * orbf_frame_post_device leave them (descriptor rows 4-byte aligned), d_n[k] their number, d_bad[k] != 0 <=> KeyFrame::isBad().
 *
 * Observations of the table's rows in CSR form: row p's are d_obs_kf / d_obs_kp [d_obs_off[p] .. d_obs_off[p + 1]) (d_obs_off has
 * cap_points + 1 entries, the two arrays n_obs), a (key-frame slot, feature index) pair each; d_ref_kf[p] is the slot of
 * reference_kf.  The reference's std::map<shared_ptr<KeyFrame>, size_t> iterates in heap-address order, which no restatement can
 * reproduce: THE CSR ORDER IS THE ORDER, for the normal's sum and for the descriptor's first-on-ties rule.
 * Nothing of this is trusted.  An observation whose key-frame slot is outside [0, n_kf) or whose feature is outside [0, d_n[kf])
 * is dropped -- it takes part in nothing below -- and counted, never dereferenced; offsets that do not describe a list inside
 * [0, n_obs] (negative, descending, past the end) give an empty list.
 *
 * d_sel [n_sel] lists the rows to refresh: a key frame's slot array as d_mp2 of the triangulation leaves it, or the point list of
 * a BA.  Entries outside [0, cap_points) (the -1s) are skipped, rows with d_valid == 0 are skipped and counted (MapPoint.cpp:50,
 * :108), duplicates are allowed (the row is written twice with the same bytes).  For a selected row with n remaining observations
 * (float, no fused multiply-add; `/` and sqrtf correctly rounded):
 *   O_k      = the camera centre of key frame k, O_w_k = -((R_0k * t_0 + R_1k * t_1) + R_2k * t_2) as above
 *   d_j      : v = Pw - O;  len = sqrtf((vx * vx + vy * vy) + vz * vz);  d_j = len > 0 ? v / len : v            Eigen's normalized()
 *   normal   = s / (float) n,  s = ((0 + d_0) + d_1) + ... per component in CSR order; bad key frames take part   MapPoint.cpp:57-63, :73
 *   dist     = sqrtf(...) of Pw - O_ref;  kp = the feature of the first observation with kf == d_ref_kf[p], or feature 0 of the
 *              reference key frame when there is none (obs[refKeyFrame] through map::operator[]);  span = dist * kp.size;
 *   d_max_dist = 1.2f * span;  d_min_dist = 0.8f * (span / max_scale_factor)        :66-72, :83-91 -- the triangulation's expressions
 *   d_desc[p] = the descriptor row, gathered through kf->d_desc, of the observation of least median Hamming distance to the rows
 *              of all observations whose key frame is not bad: median = sorted[(N - 1) / 2] with the self distance included, strict
 *              `<` from 256, first in CSR order on ties (:103-152, the rule of orbm_distinctive_descriptors); left as it was when
 *              every observer is bad (:122).
 * Left ENTIRELY untouched and counted: a row with n == 0 (the reference would divide by zero), a row with more than 1024
 * observations, and a row whose d_ref_kf is outside [0, n_kf) or names an unobserved key frame without a feature 0.
 *
 * d_covis (may be NULL) [n_kf], written, not accumulated: for every selected valid row -- per entry of d_sel, so a duplicate
 * counts twice, as the reference's loop over a key frame's slots does, and whether or not the row was left untouched -- and each
 * remaining observation with kf != kf_self, d_covis[kf]++.  CONNECT_TH, the sort and the graph edits are
 * orbm_update_connections_device ("The covisibility graph on the device").
 * d_result (int32 x 8, written): [0] rows refreshed, [1] skipped invalid, [2] untouched: no usable observation, [3] untouched: over
 * 1024 observations, [4] observations dropped for an index out of range (of every selected valid row), [5] refreshed rows whose
 * descriptor was left as it was: every observer bad, [6] refreshed rows whose reference key frame was not among their observations,
 * [7] untouched: no reference key frame feature to read.
 * Cost: one wave per selected row, four to a workgroup, 8 KB of LDS per workgroup, so the common list of 2-15 observations does not
 * pay for the longest: a list of more than 64 observations re-gathers its descriptors in tiles of 64 (9 * (n / 64)^2 tile loads).
 * Every path gives the same bytes.  No scratch memory, handle scratch, allocation or host wait.  d_desc must be 4-byte aligned.
 * Arguments are checked first (ORBX_E_ARG); without a HIP device the call fails with ORBX_E_NO_DEVICE.  n_sel = 0 is allowed (d_covis
 * and d_result are zeroed).  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
typedef struct orbm_kf_table {
    int32_t n_kf;
    const double *d_pose_R, *d_pose_t;   /* [n_kf][9] / [n_kf][3] */
    const uint8_t *d_bad;                /* [n_kf] KeyFrame::isBad() */
    const void *const *d_kps;            /* [n_kf] device pointers to orbx_kp records */
    const uint8_t *const *d_desc;        /* [n_kf] device pointers to [n][32] descriptors, 4-byte aligned */
    const int32_t *d_n;                  /* [n_kf] features per key frame */
} orbm_kf_table;
int orbm_refresh_points_device(orbm_t *h, const orbm_kf_table *kf, const int32_t *d_sel, int n_sel, const float *d_points,
                               const uint8_t *d_valid, int cap_points, float *d_normals, float *d_min_dist, float *d_max_dist,
                               uint8_t *d_desc, const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs,
                               const int32_t *d_ref_kf, float max_scale_factor, int kf_self, int32_t *d_covis, int32_t *d_result,
                               void *stream);

/* KeyFrame::computeSceneMedianDepth (KeyFrame.cpp:159-179) for n_kf key frames in one launch, a workgroup each.  Key frame k's
 * map-point slots are d_slots[k * stride ..], min(d_n[k], stride) of them; every slot in [0, cap_points) contributes (the reference
 * tests non-null only, not bad) z = ((R_20 * x + R_21 * y) + R_22 * z) + t_2.  d_count[k] = their number, d_median[k] = the element
 * d_count[k] / 2 of the ascending order -- an exact selection on order-preserving keys, the value a sort returns (-0 orders below
 * +0) -- and NaN when the count is 0 (the reference reads past an empty vector).  With cur >= 0 and d_baseline != NULL also
 * d_baseline[k] = sqrtf(...) of O_cur - O_k (LocalMapping.cpp:163); the test baseline / median < 0.01 stays with the caller, who
 * reads n_kf pairs back once.  stride <= ORBM_MEDIAN_MAX_STRIDE (ORBX_E_UNSUPPORTED above: the keys live in LDS); cur < n_kf.
 * Arguments are checked first; no device: ORBX_E_NO_DEVICE; n_kf = 0 is allowed.  Enqueued on `stream`; no scratch, no host wait. */
#define ORBM_MEDIAN_MAX_STRIDE 8192   /* ORBV_MAX_FEATURES */
int orbm_scene_median_depth_device(orbm_t *h, int n_kf, const double *d_pose_R, const double *d_pose_t, const int32_t *d_slots,
                                   const int32_t *d_n, int stride, const float *d_points, int cap_points, int cur, float *d_median,
                                   int32_t *d_count, float *d_baseline, void *stream);

/* ---- Observations built and key frames culled on the device -------------------------------------------------------------------
 * The one link of the mapper step that the three sections above left on the host: the CSR the refresh reads, rebuilt from the key
 * frames' slot arrays, and LocalMapping::KeyFrameCulling (modules/Frontend/LocalMapping.cpp:318-372) with the cascade of
 * KeyFrame::setBad -> MapPoint::eraseObservation -> MapPoint::setBad (KeyFrame.cpp:402-418, MapPoint.cpp:190-226).  With them and
 * orbm_fuse_apply_device (the next section: the searches alone find the fuse's hits, they do not apply them)
 * triangulate -> build -> fuse -> build -> refresh -> local BA -> cull runs on one stream; the local BA ("Local bundle adjustment on the
 * device-resident map" below) is the one link that waits, for its small read-backs -- nothing else returns to the host.  Both are
 * integer only.  Device pointers only, and deliberately NO host-pointer twin, for the refresh's reason: the reference-signature shims
 * (compat/) keep their host objects.
 *
 * THE SLOT ARRAYS ARE THE TRUTH.  Key frame k's map-point slots are d_slots[k * stride ..], min(d_n[k], stride) of them (the layout
 * of orbm_scene_median_depth_device; d_mp1 / d_mp2 of the triangulation are such rows), and row p's observations are exactly the
 * pairs (k, i) with d_slots[k * stride + i] == p.  The CSR (d_obs_off / d_obs_kf / d_obs_kp, as the refresh takes it) is their
 * inverse, an index that can be rebuilt at any time.  A CSR entry (k, i) of row p is LIVE iff d_slots[k * stride + i] == p and
 * d_bad[k] == 0.  The refresh's "THE CSR ORDER IS THE ORDER" is hereby ascending (k, i): the reference's std::map iterates in
 * heap-address order, which nothing reproduces.
 *
 * orbm_build_observations_device.  Slot i of key frame k holding p:
 *   p outside [0, cap_points) (the -1s included)   no map point; not counted
 *   d_valid[p] == 0                                 skipped, d_result[2]++: a bad point has no observations (MapPoint.cpp:217)
 *   else d_bad[k] != 0                              skipped, d_result[3]++: KeyFrame::setBad erased them (KeyFrame.cpp:410)
 *   else                                            the observation (k, i) of row p
 * (a d_n[k] <= 0 gives key frame k no slot).  d_obs_off receives cap_points + 1 offsets, d_obs_kf / d_obs_kp the n_obs =
 * d_obs_off[cap_points] entries, every row's list in ascending (k, i); entries at and past n_obs are not written.  The bytes are
 * the same on every run: count into d_obs_off, scan, scatter the keys k * ORBM_MEDIAN_MAX_STRIDE + i behind the rows' cursors --
 * the cursor of row p is d_obs_off[p + 1] itself, which the scatter advances from the row's start to its end, the final value --
 * and then SORT every list on its key, one wave per row, four to a workgroup, by rank (the number of smaller keys of the list, read
 * in tiles of 64), so the order the atomics came in never reaches the output.  A sort was chosen over a stable placement because
 * the latter needs a count per (block of slots, row), which is scratch of the order of the table.  NO scratch memory and no handle
 * scratch: d_obs_kp holds the unsorted keys, d_obs_kf receives the sorted ones, and the wave splits them in place.
 * Two slots (k, i), (k, i') of one key frame naming the same row cannot occur in the reference (addObservation refuses the second,
 * MapPoint.cpp:184); here both entries are emitted and the row is counted in d_result[5].
 * Overflow: n_obs > cap_obs is found after the count and before anything is scattered; d_obs_kf / d_obs_kp are then untouched and
 * d_obs_off is ALL ZEROS -- every list is empty, so a refresh enqueued behind it changes nothing -- and d_result[1] = 1.
 * What the calls of a mapper step's opening do behind such a build (tests/mapper_session.py runs a session through one): the refresh
 * counts every selected valid row under "no observation" and leaves d_covis all zero, so orbm_update_connections_device has nothing to
 * do; and orbm_cull_map_points_device sees getNumObs() == 0 for every row, so every listed row of age >= 2 goes bad, its slots left
 * naming it (the next build skips them as invalid).  That destroys a map: a chain that does not read d_result[1] back sizes cap_obs to
 * n_kf * stride, which cannot overflow.
 * d_result (int32 x 8, written, not accumulated): [0] n_obs (the full count, also on overflow), [1] overflow, [2] slots skipped: row
 * invalid, [3] slots skipped: key frame bad, [4] the longest list, [5] rows in which a key frame occurs more than once (0 on
 * overflow: it is found by the sort), [6] rows with more than 1024 observations (the refresh leaves those untouched), [7] 0.
 * Limits (ORBX_E_UNSUPPORTED above): stride <= ORBM_MEDIAN_MAX_STRIDE; n_kf <= 262143 (n_kf * ORBM_MEDIAN_MAX_STRIDE fits in int32);
 * cap_points <= 524288, the builders' limit.  n_kf = 0 is allowed and gives all-zero offsets.
 * Cost: five launches (clear, count, a one-workgroup scan over cap_points + 1 offsets, scatter, sort); a list of n entries costs
 * n * ceil(n / 64) lane reads in the sort, so the common list of 2-15 is one pass of one wave.  Kernels: no scratch memory; static
 * LDS 72 B (the scan) and none elsewhere; at most 32 VGPRs.
 * Arguments are checked first (ORBX_E_ARG); without a HIP device the call fails with ORBX_E_NO_DEVICE.  Enqueued on `stream` (NULL:
 * orbx.h, "Streams"); no allocation, no host wait. */
int orbm_build_observations_device(orbm_t *h, int n_kf, const int32_t *d_n, const uint8_t *d_bad, const int32_t *d_slots, int stride,
                                   const uint8_t *d_valid, int cap_points, int cap_obs, int32_t *d_obs_off, int32_t *d_obs_kf,
                                   int32_t *d_obs_kp, int32_t *d_result, void *stream);

/* LocalMapping::KeyFrameCulling with its cascade.  recent / timestamps: HOST arrays, copied into the launch's arguments as
 * orbm_proj_camera is: the key-frame slots of Map::getRecentKeyFrames(25) in that order and their timestamps, n_recent <= 32
 * (ORBX_E_UNSUPPORTED above); an entry outside [0, kf->n_kf) is an argument error.  first_kf: the slot of the key frame with id 0,
 * or -1.  The reference's constants: th_obs = 3, redundant_ratio = 0.9, max_gap = 1.5 (double literals there, hence doubles here).
 * Of kf the kernel uses d_kps and d_n only; d_bad is in / out and may be the array kf->d_bad points to.  d_slots, d_valid as above,
 * in / out; d_ref_kf [cap_points] (the refresh's) in / out.  The CSR is the one orbm_build_observations_device left from these slots;
 * it is never rewritten and read with the refresh's distrust: offsets that do not describe a list inside [0, n_obs] give an empty
 * list; an entry whose key frame is outside [0, n_kf) or whose feature is outside [0, min(d_n[k], stride)) is dropped, never
 * dereferenced (d_result[6] counts such entries once each, over all of [0, n_obs)).  Liveness is evaluated against d_slots and d_bad
 * as they are NOW, so a stale CSR entry is harmless.  Behind a build that overflowed every list is empty: numMP is still counted from
 * the slots, numRedundant is 0 for every candidate, so every candidate is kept (d_code 0, or 1 / 2) and nothing is written but the
 * outputs; orbm_erase_connections_device then finds no code 3 and leaves the graph.
 *
 * Candidates idx = 1 .. n_recent - 2 strictly in order, last = 0 (n_recent < 3: no candidate -- not the reference's size_t
 * underflow).  For c = recent[idx]:
 *   c == first_kf                                              skipped, d_code 1                                     :329
 *   else timestamps[idx + 1] - timestamps[last] > max_gap      skipped, d_code 2                                     :330
 *   numMP        = slots i of c with p = d_slots[..] in [0, cap_points) and d_valid[p] != 0                          :341
 *   numRedundant = those of them whose row has more than th_obs live entries (getNumObs()) and at least th_obs live entries
 *                  (k2, i2) with k2 != c and octave(k2, i2) <= octave(c, i) + 1, octaves from the orbx_kp records; the `break` of
 *                  :355 only caps the count, so no order enters                                                      :344-359
 *   (double) numRedundant > redundant_ratio * (double) numMP false: kept, d_code 0, last = idx                       :364
 *   else culled, d_code 3, last unchanged: d_bad[c] = 1; then for every row p named by a slot of c with p in range and d_valid[p]
 *        != 0 -- ONCE per row, should two slots of c name it -- the observation (c, .) is erased (MapPoint.cpp:190-208): with
 *        L = the live entries of p of key frames other than c, in CSR order,
 *          d_ref_kf[p] == c and L not empty: d_ref_kf[p] = the key frame of L's first entry (observations.begin(), :198-199);
 *          |L| <= 2: the point goes bad (:202, :210-226): d_valid[p] = 0 and d_slots[k2 * stride + i2] = -1 for every entry of L;
 *        finally every slot of c, whatever it holds, becomes -1 (map_points.clear(), KeyFrame.cpp:418).
 * Each candidate sees what the ones before it wrote.  The covisibility-graph and spanning-tree edits of KeyFrame::setBad are
 * orbm_erase_connections_device, which takes d_code as it is; Map::eraseMapPoint stays with the caller, who reads d_code.
 * d_code [n_recent]: -1 at positions 0 and n_recent - 1, else as above; d_num_mp / d_num_redundant [n_recent]: 0 where not evaluated.
 * d_result (int32 x 8, written): [0] culled, [1] kept, [2] skipped, [3] points set bad, [4] slots cleared in key frames other than
 * the culled one, [5] d_ref_kf entries reassigned, [6] CSR entries dropped for an index out of range, [7] 0.
 * Shape: ONE launch of ONE workgroup of 1024 threads, a thread per slot of the candidate, workgroup barriers between the phases --
 * the candidates are sequential and the work (<= 23 candidates x <= 8192 slots x short lists) is latency, as in k_project /
 * k_triangulate; inside a candidate the slots are independent, because a point's cascade touches only that point's slots.  The
 * once-per-row rule is a claim mask of one bit per table row in dynamic LDS (cap_points / 8 bytes, hence cap_points <= 524288,
 * ORBX_E_UNSUPPORTED above; stride <= ORBM_MEDIAN_MAX_STRIDE likewise).  No scratch memory, handle scratch, allocation or host wait;
 * static LDS 40 B; at most 64 VGPRs.
 * Arguments are checked first (ORBX_E_ARG; th_obs >= 0, first_kf in [-1, n_kf)); without a HIP device the call fails with
 * ORBX_E_NO_DEVICE.  n_recent = 0 is allowed.  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
int orbm_cull_keyframes_device(orbm_t *h, const orbm_kf_table *kf, uint8_t *d_bad, int32_t *d_slots, int stride, uint8_t *d_valid,
                               int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs,
                               int32_t *d_ref_kf, const int32_t *recent, const double *timestamps, int n_recent, int first_kf,
                               int th_obs, double redundant_ratio, double max_gap, int32_t *d_code, int32_t *d_num_mp,
                               int32_t *d_num_redundant, int32_t *d_result, void *stream);

/* ---- The fuse's hits applied on the device --------------------------------------------------------------------------------------
 * What the static fuse SearchByProjection(keyFrame, mapPoints, Map*, th) does with a hit (modules/ORB/ORBMatcher.cpp:574-589):
 * MapPoint::addObservation + KeyFrame::addMapPoint, or MapPoint::replace (MapPoint.cpp:233-264), on the slot arrays of the section
 * above.  With it orbm_project_fuse_device -> orbm_search_fuse_device -> this call runs per target key frame of
 * LocalMapping::searchInNeighbors (LocalMapping.cpp:261-316) without a wait, a read-back, a host loop and an upload, and the chain
 * triangulate -> build -> fuse -> build -> refresh -> local BA -> cull exists as that section states it.  THE SLOT ARRAYS ARE
 * THE TRUTH: an observation is a slot, so addObservation and addMapPoint are ONE store, and replace rewrites the slots that name the
 * loser.  Integer only.  Device pointers only, and deliberately NO host-pointer twin, for the refresh's reason: the reference-signature
 * shims (compat/) keep their host objects.
 * The list of fuseMapPoints itself -- the de-duplicated union of the target key frames' slots (LocalMapping.cpp:287-300) -- is
 * orbm_fuse_targets_device's d_rows ("The covisibility graph on the device").  Out of scope, the caller's: Map::eraseMapPoint
 * (MapPointCulling is orbm_cull_map_points_device, "Key frames inserted and recent map points culled on the device").
 *
 * Entries: d_best_idx [nq] as orbm_search_fuse_device leaves it; entry j is table row d_rows[j], or row j when d_rows is NULL (the
 * builders index the table by query).  kf_target = K, the key frame searched.  d_n, d_bad, d_slots (in / out), stride: the layout of
 * orbm_build_observations_device.  d_valid (in / out), cap_points: the table.  obs(p) = the pairs (k, i) with d_slots[k * stride + i]
 * == p, i < min(d_n[k], stride) and d_bad[k] == 0, in ascending (k, i); getNumObs() is its size.
 *
 * For j = 0 .. nq - 1 IN ORDER, p = the entry's row, s = d_best_idx[j], n_K = min(max(d_n[K], 0), stride); the first rule that
 * applies decides (d_code[j]):
 *   0 none       s < 0
 *   1 dropped    s >= n_K, or p outside [0, cap_points): counted, nothing is read through it
 *   2 gated      d_valid[p] == 0, or p is named by one of the n_K slots of K: isObserveKeyFrame, on the slots as they are when entry j
 *                is reached (:534; orbm_project_fuse_device left these tests to its caller's d_valid)
 *   3 added      o = d_slots[K * stride + s] is outside [0, cap_points): d_slots[K * stride + s] = p (:576-578)
 *   4 bad occupant   d_valid[o] == 0: nothing is written (:579 is false), the entry counts as a match (:587)
 *   5 / 6 replace    otherwise.  The loser L is p when getNumObs(o) > getNumObs(p), strictly (:580; code 5: the list point replaced by
 *                the occupant), else o (code 6; a tie replaces the occupant); the winner W is the other row.  For every (k, i) of
 *                obs(L) in order: d_slots[k * stride + i] = W if W has no observation in key frame k at that moment, else -1
 *                (MapPoint.cpp:249-257; should L hold two slots of one key frame, the first moves and the second is cleared; a slot
 *                of L in a bad key frame is no observation and stays).  Then d_valid[L] = 0.  Then, with d_found / d_visible
 *                [cap_points] (int32; both or neither may be NULL), d_found[W] += d_found[L] + d_visible[L]: the reference calls
 *                increaseFound(numFound) and increaseFound(numVisible) (:259-260), and this is the reference's text, not a
 *                correction; d_visible is only read.  d_ref_kf is not an argument: replace does not touch reference_kf.
 *   7 undone     a replace in which the CSR list of p or of o is longer than ORBM_MAX_LIST (1024) entries: left undone and counted,
 *                as the refresh leaves such rows; the entry counts as a match.
 * d_refresh_sel [nq]: W for codes 5 / 6 (computeDescriptor on the winner, MapPoint.cpp:261), p for code 3, else -1: behind a rebuilt
 * CSR it is orbm_refresh_points_device's d_sel with n_sel = nq (the refresh skips -1 and allows duplicates).
 * d_result (int32 x 8, written, not accumulated): [0] the reference's return value, the entries with a code of 3 or more, [1] the
 * refusal (below), [2] observations added, [3] list points replaced by the occupant, [4] occupants replaced by the list point, [5]
 * slots cleared because the winner already observed the key frame, [6] gated, [7] everything dropped or left undone: entries of code
 * 1 and 7 plus the CSR entries dropped for an index out of range (once each, over all of [0, n_obs), as the culling counts them).
 *
 * The observation index: d_obs_off / d_obs_kf / d_obs_kp / n_obs as orbm_build_observations_device left it from THESE slots with no
 * edit in between.  It only tells where the slots naming a row are; it is never rewritten, and read with the refresh's distrust:
 * offsets that do not describe a list inside [0, n_obs] give an empty list, an entry whose key frame is outside [0, n_kf) or whose
 * feature is outside [0, min(d_n[k], stride)) is dropped and counted, never dereferenced, and an entry counts only if its slot
 * names the row NOW.  A CSR that is not fresh may therefore give a different answer -- observations it does not list are neither
 * counted nor moved -- but never an access out of bounds.
 *
 * Parallelism and the refusal.  Entries that hit different slots of K do not interact if (1) no row occurs in two LIVE entries (an
 * entry that is not none, dropped or gated on the arrays as passed), (2) no hit slot's valid occupant is named by a second slot of K,
 * and (3) no live row is an occupant, which the gate ensures.  Then every row belongs to at most one CHAIN, the live entries of one
 * hit slot in list order, and the gate of an entry is the same on the arrays as passed as when it is reached.  The reference's
 * callers satisfy both: fuseMapPoints is a set, and addObservation refuses a second slot.  (1) and (2) are checked before anything
 * is written: on a violation d_result = {0, 1 (a row twice) or 2 (an occupant in two slots; 1 wins), 0 ...} and d_slots, d_valid,
 * d_found, d_code and d_refresh_sel are EXACTLY as passed (d_work is not).
 * Shape: ONE launch of ONE workgroup of 1024 threads, as the culling; a mask of one bit per table row in dynamic LDS (cap_points / 8
 * bytes, hence cap_points <= 524288) for "named by a slot of K" and then for the two premises, plus one int per slot of K (the first
 * live entry of each hit slot: 4 * stride bytes, stride <= ORBM_MEDIAN_MAX_STRIDE); then a wave per chain, lanes across the lists: the
 * winner's observations are the live entries of the lists of every row merged into it plus the chain's own slot of K.  d_work [nq]
 * (int32) is the caller's work array: the entries' classes and the chains' links.  The bytes are the same on every run: counts are
 * sums, and no stored value depends on the order atomics arrive in.  No scratch memory, handle scratch, allocation or host wait;
 * static LDS 1064 B; at most 64 VGPRs (sixteen waves in one workgroup: 128 is all a thread could have).
 * Arguments are checked first (ORBX_E_ARG; kf_target in [0, n_kf)); limits (ORBX_E_UNSUPPORTED): cap_points <= 524288, stride <=
 * ORBM_MEDIAN_MAX_STRIDE, nq <= 2^30; without a HIP device the call fails with ORBX_E_NO_DEVICE.  nq = 0 is allowed.  Enqueued on
 * `stream` (NULL: orbx.h, "Streams"). */
int orbm_fuse_apply_device(orbm_t *h, const int32_t *d_best_idx, const int32_t *d_rows, int nq, int n_kf, int kf_target,
                           const int32_t *d_n, const uint8_t *d_bad, int32_t *d_slots, int stride, uint8_t *d_valid, int cap_points,
                           const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs, int32_t *d_found,
                           const int32_t *d_visible, int32_t *d_work, int32_t *d_code, int32_t *d_refresh_sel, int32_t *d_result,
                           void *stream);

/* ---- Local bundle adjustment on the device-resident map --------------------------------------------------------------------------
 * Optimize::localBundleAdjustment (modules/Backend/Optimize.cpp:766-951) for a caller whose slot arrays, map-point table and key-frame
 * poses live in device memory, in three calls on one stream:
 *   orbm_local_ba_problem_device                  :766-889  the local map gathered, vertices and edges built: an orbba_problem in device memory
 *   orbba_local_bundle_adjustment_device (orbba.h) :892-922  the two rounds of Levenberg-Marquardt on those arrays
 *   orbm_local_ba_apply_device                    :914-950  outlier observations erased with their cascade, poses and positions written back
 * Between the first and the second the caller reads the first 32 bytes of the assembly's d_result back ONCE (the three sizes are host
 * ints of the LM call) and the LM call waits for one small block per trial; no table, slot array or index returns to the host, and
 * no host loop runs over points or observations.  mp->update() (:948) is orbm_refresh_points_device with d_sel = d_point_row behind a
 * rebuilt CSR; it is not repeated here.  d_local (getConnectedKFs) is orbm_connected_keyframes_device's d_out ("The covisibility graph on
 * the device"), MapPointCulling is orbm_cull_map_points_device; only Map::eraseMapPoint stays with the caller.
 * The two calls below follow this header's rules for the map side: device pointers only and deliberately NO host-pointer twin; no
 * allocation, handle scratch or host wait; results written, not accumulated; the same bytes on every run; every index that comes
 * from device memory is distrusted -- dropped and counted, never dereferenced out of range.  THE SLOT ARRAYS ARE THE TRUTH and the CSR
 * (as orbm_build_observations_device left it from these slots) only tells where the slots naming a row are: offsets that do not
 * describe a list inside [0, n_obs] give an empty list, an entry whose key frame is outside [0, n_kf) or whose feature is outside
 * [0, min(d_n[k], stride)) is dropped (counted once each over all of [0, n_obs)), and an entry is LIVE iff its slot names the row NOW
 * and its key frame is not bad.
 *
 * orbm_local_ba_problem_device.  d_local [n_local] (device): d_local[0] is the current key frame, the rest getConnectedKFs() in the
 * caller's order -- or orbm_connected_keyframes_device's d_out with n_local = its n_out: the -1 fill is dropped below, so no count is
 * read back.  first_kf: the slot of the key frame with id 0, or -1, as in the culling.
 *   Local key frames: the entries of d_local in order.  An entry outside [0, n_kf) is dropped (d_result[6]); a later entry whose key
 *     frame is bad is skipped (:777, d_result[7]); an entry naming a key frame an earlier entry named is dropped (d_result[6]).  Entry 0
 *     is taken whether or not it is bad.
 *   Local points (:783-792): the rows p in [0, cap_points) with d_valid[p] != 0 named by one of the min(max(d_n[k], 0), stride) slots
 *     of a local key frame, each numbered at its FIRST occurrence in (position among the kept local key frames, slot) order -- the
 *     reference's BA_local_for_kf marking.  A row that ends up without an edge is dropped before numbering (d_result[8]).
 *   Edges (:860-889): per local point in that order, its LIVE CSR entries in CSR order.  A key frame that occurs a second time in one
 *     row's list gives no second edge (d_result[9]; the LM refuses a point observed twice by a key frame).  For edge e of point x:
 *     d_edge_point[e] = x (non-decreasing), d_edge_pose[e] = the pose of the key frame, d_edge_z[2e..] = the orbx_kp record's (x, y)
 *     widened to double, d_edge_inv_sigma2[e] = (double)((1.f / size) / size) (:877), d_edge_kf / d_edge_kp[e] = (key-frame slot,
 *     feature); d_edge_off[x] = the point's first edge, d_edge_off[n_points] = n_edges.
 *   Poses: the kept local key frames in list order, then the fixed ones (:795-806) -- every key frame of an edge that is not local --
 *     in ASCENDING SLOT ORDER.  That is a stated canonicalisation: the reference's order comes from std::map's heap addresses, and a
 *     fixed pose has no block in the system, so its position reaches no number.  d_pose_fixed = 1 for those and for a local key frame
 *     equal to first_kf (:830); d_pose_R / d_pose_t = (double)(float) of the table's values (the reference's Pose is float);
 *     d_ba_points [x][3] = (double) of d_points[d_point_row[x]]; d_pose_kf [pose] / d_point_row [x] map back to slots and rows.
 * The output arrays are an orbba_problem (orbba.h) in device memory: d_pose_R [cap_poses][9], d_pose_t [..][3], d_pose_fixed, d_pose_kf
 * [cap_poses]; d_ba_points [cap_local_points][3], d_point_row [cap_local_points], d_edge_off [cap_local_points + 1]; d_edge_pose,
 * d_edge_point, d_edge_inv_sigma2, d_edge_kf, d_edge_kp [cap_edges], d_edge_z [cap_edges][2].  d_work: the caller's work array of
 * cap_points + n_kf int32 (the rows' first occurrences and the key frames' poses; its contents afterwards are unspecified).
 * d_result (int32 x 16, written; the first eight -- 32 bytes -- are what the caller reads back): [0] n_poses, [1] n_points, [2]
 * n_edges, [3] local key frames kept (the poses apply writes), [4] fixed key frames, [5] the refusal, a bit mask: 1 more poses than
 * cap_poses, 2 more points than cap_local_points, 4 more edges than cap_edges, 8 no free pose (no local key frame besides first_kf),
 * 16 no edge; [6] entries of d_local dropped, [7] skipped for a bad key frame; [8] rows dropped for having no edge, [9] second edges
 * of a key frame in one row, [10] CSR entries dropped for an index out of range; the rest 0.  On a refusal the counts are still the
 * FULL counts, no array is written at or past its capacity, and what lies below is unspecified: do not run the LM on it.
 * Behind a build that overflowed (every list empty; tests/mapper_session.py's session csr_overflow_late) the call keeps its local key
 * frames ([0] = [3], no fixed one), drops every valid row they name for having no edge ([8] counts each once, [1] = [2] = 0) and refuses
 * with 16: the caller, who reads [5] back, runs neither the LM nor orbm_local_ba_apply_device, and the step goes on to the culling.
 * Shape: ONE launch of ONE workgroup of 1024 threads with barriers between the phases, as the culling -- 20 key frames x 2000 slots x
 * short lists are latency: first occurrences by atomicMin (the least key wins whatever the order), then the slots in order, a tile of
 * 1024 at a time, with a block scan of (has an edge, edges) numbering points and edges.  A row's list is walked twice (count, write)
 * and a key frame's second entry is found by re-reading the list's start, so a list of n entries costs n^2 / 2 reads by one thread:
 * nothing for the 2-30 of a map, slow for a forged CSR.  No scratch memory; static LDS 4288 B; at most 64 VGPRs.
 * Limits (ORBX_E_UNSUPPORTED above): n_local <= ORBM_LOCAL_BA_MAX_LOCAL, stride <= ORBM_MEDIAN_MAX_STRIDE, cap_points <= 524288.
 * Arguments are checked first (ORBX_E_ARG: n_local and the capacities >= 1, first_kf in [-1, n_kf)); without a HIP device the call fails
 * with ORBX_E_NO_DEVICE.  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
#define ORBM_LOCAL_BA_MAX_LOCAL 1024
int orbm_local_ba_problem_device(orbm_t *h, const orbm_kf_table *kf, const int32_t *d_slots, int stride, const uint8_t *d_valid,
                                 const float *d_points, int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf,
                                 const int32_t *d_obs_kp, int n_obs, const int32_t *d_local, int n_local, int first_kf, int cap_poses,
                                 int cap_local_points, int cap_edges, int32_t *d_work, double *d_pose_R, double *d_pose_t,
                                 uint8_t *d_pose_fixed, double *d_ba_points, int32_t *d_edge_pose, int32_t *d_edge_point,
                                 double *d_edge_z, double *d_edge_inv_sigma2, int32_t *d_edge_kf, int32_t *d_edge_kp, int32_t *d_edge_off,
                                 int32_t *d_point_row, int32_t *d_pose_kf, int32_t *d_result, void *stream);

/* orbm_local_ba_apply_device.  n_local, n_points, n_edges: d_result[3], [1], [2] of the assembly, which the caller read back for the
 * LM; d_pose_kf, d_point_row, d_edge_off, d_edge_kf, d_edge_kp: the assembly's maps; d_est_pose_R / d_est_pose_t / d_est_points /
 * d_outlier: the outputs of orbba_local_bundle_adjustment_device.  In / out: d_slots, d_valid, d_ref_kf [cap_points] (the refresh's),
 * d_points, and d_kf_pose_R / d_kf_pose_t, the key-frame table's pose arrays.  The CSR is the one the assembly read.
 *   Erase (:927-934).  For each local point x, row p = d_point_row[x], its edges e in [d_edge_off[x], d_edge_off[x + 1]) with
 *     d_outlier[e] != 0 in edge order, (k, i) = (d_edge_kf[e], d_edge_kp[e]); nothing more once the point is bad (:931).  If the slot
 *     (k, i) still names p and k is not bad: d_slots[k * stride + i] = -1 (KeyFrame::eraseMapPoint), then MapPoint::eraseObservation
 *     (MapPoint.cpp:190-208) as orbm_cull_keyframes_device states it: with L = the live entries of p of key frames other than k, in CSR
 *     order, d_ref_kf[p] == k and L not empty: d_ref_kf[p] = the key frame of L's first entry; |L| <= 2: the point goes bad, d_valid[p]
 *     = 0 and the slot of every entry of L becomes -1.  (Should a second slot of k name p, which the reference cannot have, it stays.)
 *     Points are independent -- a point's cascade touches only its own slots --, the edges of one point sequential.
 *   Poses (:937-941).  For q < n_local, key frame k = d_pose_kf[q]: d_kf_pose_R / d_kf_pose_t[k] = (double)(float) of the estimate.
 *     The fixed key frames behind them are not written.
 *   Points (:944-950).  Every local row still valid after the erasures: d_points[p] = (float) of the estimate.
 * An entry of d_point_row outside [0, cap_points), offsets of d_edge_off that do not describe a list inside [0, n_edges], an edge
 * whose (k, i) is unusable and an entry of d_pose_kf outside [0, n_kf) are dropped and counted, never dereferenced.
 * d_result (int32 x 8, written): [0] observations erased, [1] points set bad, [2] slots cleared by the cascade, [3] reference key
 * frames moved, [4] rows whose position was written, [5] CSR entries dropped for an index out of range, [6] entries of the assembly's
 * maps dropped, [7] poses written.
 * Shape: ONE launch of ONE workgroup of 1024 threads, a thread per local point, then per local key frame.  No scratch memory, handle
 * scratch, allocation or host wait; static LDS 32 B; at most 64 VGPRs.  Limits and errors as above.  Enqueued on `stream`. */
int orbm_local_ba_apply_device(orbm_t *h, int n_kf, const int32_t *d_n, const uint8_t *d_bad, int32_t *d_slots, int stride,
                               uint8_t *d_valid, int32_t *d_ref_kf, float *d_points, int cap_points, double *d_kf_pose_R,
                               double *d_kf_pose_t, const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs,
                               int n_local, int n_points, int n_edges, const int32_t *d_pose_kf, const int32_t *d_point_row,
                               const int32_t *d_edge_off, const int32_t *d_edge_kf, const int32_t *d_edge_kp, const double *d_est_pose_R,
                               const double *d_est_pose_t, const double *d_est_points, const uint8_t *d_outlier, int32_t *d_result,
                               void *stream);

/* ---- The covisibility graph on the device ------------------------------------------------------------------------------------------
 * What the links of the mapper step exchange: KeyFrame::connected_kf_weights / ordered_connected_kfs and the spanning tree
 * (modules/BasicObject/KeyFrame.cpp:225-362, :402-467; CONNECT_TH = 15, KeyFrame.h:24) in device memory beside the slot arrays, with
 * four entry points: updateConnections behind the refresh's d_covis, the graph part of setBad behind the culling's d_code, the target
 * key frames and the fuseMapPoints list of LocalMapping::searchInNeighbors (LocalMapping.cpp:263-300), and getConnectedKFs /
 * getBestCovisibleKFs as the d_local of orbm_local_ba_problem_device.  With them the only read-back the graph adds per key frame is
 * the target list of at most n_first * (1 + n_second) = 120 ints, which the host needs anyway: kf_target of the fuse calls is a host
 * int.  The map side's rules hold: device pointers only and deliberately NO host-pointer twin; no allocation, handle scratch or host
 * wait; integer only, written not accumulated, the same bytes on every run.
 *
 * The state is the caller's, a host struct of device pointers copied into the launch's arguments as orbm_kf_table is:
 *   - the caller zero-fills d_weight and d_ord_n and fills d_parent with -1 ONCE; a new key frame's row and column are then empty;
 *   - only rows and columns below the call's n_kf (<= cap_kf) are read or written;
 *   - entries of d_ord_kf[k] at and past the d_ord_n[k] a call leaves are never written by that call;
 *   - ordered_connected_weights[i] is d_weight[k][d_ord_kf[k][i]] -- the reference re-sorts the list at every change of a map entry,
 *     so the invariant holds there -- and is therefore not stored;
 *   - the children of k are the j with d_parent[j] == k.  The reference's consumers all test isBad(), for which the set is the same;
 *   - THE ORDER OF A LIST is descending weight and ascending key-frame slot among equal weights.  That is a stated canonicalisation:
 *     the reference sorts pair<int, shared_ptr>, so its ties fall in heap-address order.  Likewise, where the reference takes "the
 *     first strictly greater" over an unordered_map (the fallback maxKF, KeyFrame.cpp:254), the choice here is the LEAST SLOT among the
 *     maxima.  Lists are compared on the full int32 weight; a row entry is an entry iff it is non-zero;
 *   - list entries and lengths read back from device memory are distrusted: a length is kept inside [0, n_kf], an entry outside
 *     [0, n_kf) is dropped and counted, never dereferenced.
 * Every call checks its arguments first (ORBX_E_ARG: a null graph or graph array, n_kf outside [0, cap_kf], a key frame outside
 * [0, n_kf)), then the limits (ORBX_E_UNSUPPORTED: cap_kf > ORBM_GRAPH_MAX_KF, stride > ORBM_MEDIAN_MAX_STRIDE, cap_points > 524288),
 * then fails with ORBX_E_NO_DEVICE without a HIP device.  Enqueued on `stream` (NULL: orbx.h, "Streams").
 *
 * orbm_update_connections_device: KeyFrame::updateConnections of key frame K = kf_self behind orbm_refresh_points_device's d_covis
 * (called with the same kf_self), which is the counting loop of :233-242.
 *   c[j] = d_covis[j] for j != K with d_bad[j] == 0 and d_covis[j] > 0, else 0.  A positive count of a bad key frame is ignored and
 *     counted in d_result[5]; a negative count, or d_covis[K] != 0, is ignored and counted in [6].
 *   No c[j] > 0: d_result[1] = 1 and NOTHING of the graph is written (:244).
 *   S = { j : c[j] >= connect_th }; if S is empty, S = { the least j with c[j] = max } and [2] = 1 (:265-268).
 *   For every j in S (addConnection, :293-304): if d_weight[j][K] != c[j] then d_weight[j][K] = c[j] and list j is rebuilt from ALL
 *     non-zero entries of row j; otherwise list j is left exactly as it is.  This is the reference's asymmetry, kept on purpose: a list
 *     rebuilt by updateBestCovisibles holds the sub-threshold entries that the key frame's own updateConnections put into its map; a
 *     list written by updateConnections does not hold them.
 *   Row K becomes c, every column below n_kf (connected_kf_weights = kfCounter, :281: entries of K that are now zero disappear from
 *     K's row only, the column entries d_weight[j][K] of such j survive).  List K = S in list order, d_ord_n[K] = |S|.
 *   If d_parent[K] < 0 and K != first_kf (the slot of the key frame with id 0, or -1): d_parent[K] = the head of list K, [4] = 1
 *     (be_first_connection, :285-289).
 *   d_work: n_kf int32, the caller's (the marks of the lists to rebuild).  connect_th >= 1 (the reference's is CONNECT_TH = 15).
 *   d_result (int32 x 8): [0] |S|, [1] nothing to do, [2] fallback used, [3] neighbour lists rebuilt, [4] parent assigned, [5], [6] as
 *   above, [7] 0.
 *
 * orbm_erase_connections_device: the graph part of KeyFrame::setBad, chained behind orbm_cull_keyframes_device.  recent is the HOST
 * array the culling took (n_recent <= 32, copied into the arguments; more, or an entry outside [0, n_kf), is an argument error), d_code
 * the culling's device output; with d_code == NULL every entry is processed.  For idx in order with d_code[idx] == 3, c = recent[idx]:
 *   for every j != c with d_weight[c][j] > 0: if d_weight[j][c] > 0 it becomes 0, list j is rebuilt from its whole row, [1]++
 *     (eraseConnection, :403-405, :306-317);
 *   row c becomes all zero and d_ord_n[c] = 0 (:419-420);
 *   with P = d_parent[c]: every j with d_parent[j] == c gets d_parent[j] = P ([2]++).  This IS what :423-460 do: the loop never inserts
 *     the chosen child into parentCandidates, so the candidate set stays { parent } and every child, linked to it or not, bad or not,
 *     ends with changeParent(parent).  The reference's text, not a correction.  With P < 0 the tree is left alone and [3]++ (the
 *     reference would dereference null).  d_parent[c] itself stays.
 * Each candidate sees what the ones before it wrote (a culled child of a culled key frame moves twice).  A list's final bytes depend on
 * its row's final values only, so the lists are rebuilt once, behind the last candidate; [1] counts erases, [4] the lists rebuilt (a
 * key frame erased itself later in the call is among them and ends with an empty list).  d_work: n_kf int32.
 *   d_result (int32 x 8): [0] key frames erased, [1] - [3] as above, [4] lists rebuilt, the rest 0.
 *
 * orbm_fuse_targets_device: LocalMapping.cpp:263-300.  d_n, d_bad, d_slots, stride, d_valid, cap_points: the layout of
 * orbm_build_observations_device.
 *   Targets, sequentially: for a in the first min(n_first, d_ord_n[cur]) entries of list cur: skipped if marked, else appended and
 *     marked; then for b in the first min(n_second, d_ord_n[a]) entries of list a: skipped if marked or b == cur, else marked and
 *     appended (a skipped a's list is not walked).  The reference's values are 20 and 5.  The marks are per call: the reference's
 *     fuse_target_for_kf == current_kf->id stamps are unique per call, and its id-0 coincidence is not restated.  Bad key frames are
 *     NOT filtered, because the reference does not filter them; they are counted in [3] (their slots are -1 after a cull, so they add
 *     no row).
 *   Rows: over the targets in order and their min(max(d_n[k], 0), stride) slots in order, every p in [0, cap_points):
 *     d_valid[p] == 0 is skipped and counted in [4] (:292); a row is listed at its FIRST occurrence (:296-298), later ones are counted
 *     in [6].  Rows that cur already observes stay in the list: the fuse's gate handles them, as in the reference.
 *   d_work: cap_points int32, the caller's (the rows' first occurrences; contents afterwards unspecified).
 *   d_result (int32 x 8): [0] n_targets and [1] n_rows, both FULL counts; [2] the refusal, a bit mask: 1 more targets than
 *   cap_targets, 2 more rows than cap_rows -- nothing is written at or past a capacity, and what lies below d_rows' is unspecified on
 *   a refusal --; [3] bad targets, [4] invalid, [5] list entries dropped for an index out of range, [6] duplicates, [7] 0.
 *   The caller reads d_result and d_targets back once and runs the per-target chain: one direction orbm_project_fuse_device ->
 *   orbm_search_fuse_device -> orbm_fuse_apply_device per target, the other with d_rows = this call's d_rows and nq = n_rows.
 *
 * orbm_connected_keyframes_device: d_out = [kf if include_self] + the first min(max_n, d_ord_n[kf]) entries of list kf, cut to n_out
 * entries, then -1 up to n_out; *d_n_out = the number before the fill.  With include_self = 1 and max_n = n_kf this is d_local of
 * orbm_local_ba_problem_device, which already drops entries outside [0, n_kf): the caller passes n_local = n_out without a read-back.
 *
 * Shape (latency, not throughput).  k_graph_update and k_graph_erase are ONE workgroup of 1024 threads each; they mark the rows whose
 * list changes in d_work, and k_graph_resort, launched behind them with one workgroup per key frame, rebuilds the marked ones -- a
 * workgroup reads its own mark and row and writes its own list, nothing another workgroup writes in that launch.  A list is sorted as
 * 64-bit keys (weight complement above the slot: distinct, so the order is the bytes) by a bitonic network in LDS, 32 KB for 4096
 * keys.  k_graph_fuse_targets is one workgroup: wave 0 walks the lists while the others clear d_work, then the rows' first occurrences
 * by atomicMin (the least key wins whatever the order) and the slots in order, a tile of 1024 at a time, numbered by a block scan.
 * As compiled for gfx950 -- VGPRs / scratch / static LDS: k_graph_update 26 / 0 / 32808 B, k_graph_erase 24 / 0 / 32 B, k_graph_resort
 * 12 / 0 / 32776 B, k_graph_fuse_targets 52 / 0 / 16992 B, k_graph_connected 9 / 0 / 0 B: no scratch memory, at most 64 VGPRs. */
#define ORBM_GRAPH_MAX_KF 4096
typedef struct orbm_covis_graph {
    int32_t cap_kf;        /* row pitch of the two matrices, <= ORBM_GRAPH_MAX_KF */
    int32_t *d_weight;     /* [cap_kf][cap_kf]  connected_kf_weights of key frame k: d_weight[k * cap_kf + j], 0 = no entry */
    int32_t *d_ord_kf;     /* [cap_kf][cap_kf]  ordered_connected_kfs of k: the first d_ord_n[k] entries of row k */
    int32_t *d_ord_n;      /* [cap_kf] */
    int32_t *d_parent;     /* [cap_kf]  spanning-tree parent, -1 = none yet (be_first_connection) */
} orbm_covis_graph;
int orbm_update_connections_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, const uint8_t *d_bad, const int32_t *d_covis,
                                   int kf_self, int first_kf, int connect_th, int32_t *d_work, int32_t *d_result, void *stream);
int orbm_erase_connections_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, const int32_t *recent, int n_recent,
                                  const int32_t *d_code, int32_t *d_work, int32_t *d_result, void *stream);
int orbm_fuse_targets_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, const int32_t *d_n, const uint8_t *d_bad,
                             const int32_t *d_slots, int stride, const uint8_t *d_valid, int cap_points, int cur, int n_first,
                             int n_second, int cap_targets, int cap_rows, int32_t *d_work, int32_t *d_targets, int32_t *d_rows,
                             int32_t *d_result, void *stream);
int orbm_connected_keyframes_device(orbm_t *h, const orbm_covis_graph *graph, int n_kf, int kf, int include_self, int max_n,
                                    int32_t *d_out, int n_out, int32_t *d_n_out, void *stream);

/* ---- The tracker's local map on the device -----------------------------------------------------------------------------------------
 * What Tracking::trackLocalMap (modules/Frontend/Tracking.cpp:345-373) does around its search and its pose optimisation, on the arrays
 * the sections above own: updateLocalKeyFrames + updateLocalMapPoints (:429-537), which decide what the second SearchByProjection of
 * every frame may see; the increaseVisible / increaseFound counters (:388-412, :362-364) that orbm_fuse_apply_device reads as
 * d_visible / d_found; and KeyFrame::getNumTrackedMapPoint of the reference key frame (KeyFrame.cpp:146-152), which needNewKeyFrame
 * tests (:544-545).  With them stage 1 -> orbm_local_map_device -> orbm_project_frustum_device -> orbm_track_counters_device (1 | 2) ->
 * the points search -> orbba_pose_edges_device -> poseOptimize -> orbba_pose_drop_outliers_device -> orbm_track_counters_device (4) ->
 * orbm_num_tracked_points_device runs on one stream without a host hop between the two stages.  The map side's rules hold: device
 * pointers only and deliberately NO host-pointer twin; no allocation, handle scratch or host wait; integer only, written not
 * accumulated (the two counter arrays aside: they are counters), the same bytes on every run; everything read back from device memory
 * is distrusted: clamped, dropped and counted, never dereferenced.  Arguments are checked first (ORBX_E_ARG: a null pointer, a negative
 * count, n_kf outside [0, cap_kf], a bad entry of recent), then the limits (ORBX_E_UNSUPPORTED: cap_kf > ORBM_GRAPH_MAX_KF, stride or n2
 * > ORBM_MEDIAN_MAX_STRIDE, cap_points > 524288), then the call fails with ORBX_E_NO_DEVICE without a HIP device.  Enqueued on `stream`
 * (NULL: orbx.h, "Streams").
 * d_n, d_bad, d_slots, stride, d_valid, cap_points and the CSR (d_obs_off / d_obs_kf / d_obs_kp, n_obs): the layout of
 * orbm_build_observations_device and what it left.  The CSR is read with the culling's distrust: offsets that do not describe a list
 * inside [0, n_obs] give an empty list; an entry (k, i') whose key frame is outside [0, n_kf) or whose feature is outside [0,
 * min(max(d_n[k], 0), stride)) is DROPPED; an entry of row p that is not LIVE (d_slots[k * stride + i'] == p and d_bad[k] == 0) is
 * STALE and skipped.  Both kinds are counted.
 *
 * orbm_local_map_device.  d_frame_mp [n2], in / out: the slots of the frame the reference votes from -- the current frame, or the last
 * frame once the IMU is initialised (:432-460); the caller passes whichever applies.  Values are table rows.
 *   Votes.  For i < n2, p = d_frame_mp[i]: p outside [0, cap_points): nothing happens; d_valid[p] == 0: d_frame_mp[i] = -1, [5]++
 *     (:441-443); otherwise every live CSR entry (k, i') of row p adds one to votes[k] (dropped entries [6]++, stale ones [7]++).  This
 *     is per entry of d_frame_mp: a row named twice votes twice, as the reference's loop does.
 *   The list.  First the entries of recent in order, each marked (:466-470): recent is a HOST array of key-frame slots in
 *     Map::getRecentKeyFrames(10) order (Map.cpp:42-53: oldest first), n_recent <= 32, copied into the launch's arguments as
 *     orbm_erase_connections_device does; more, an entry outside [0, n_kf) or a repeated entry is an argument error.  The reference does
 *     not test them for bad, so neither does this; bad ones are counted in [9].  Then every k with votes[k] > 0 ([8] of them) in
 *     ASCENDING SLOT ORDER, appended and marked unless already marked; maxKF is the LEAST SLOT among the maxima of the votes.  Both are
 *     stated canonicalisations where the reference iterates an unordered_map<shared_ptr<KeyFrame>, int> (:474-487), the same two the
 *     graph section makes.  The kf->isBad() of :476 cannot be met: a live entry has no bad key frame.
 *   Expansion (:490-519), sequential and literal.  Positions 0 .. end0 - 1 of the list, end0 fixed at the length the two steps above
 *     left (iterEnd is taken once).  At each position, kf = the entry there:
 *       1. the list's length > max_kf: stop ([11] = 1);
 *       2. the first min(n_neigh, d_ord_n[kf]) entries of list kf: each that is neither bad nor marked is appended and marked (an
 *          entry outside [0, n_kf) is dropped, [10]++; the length is kept inside [0, n_kf]);
 *       3. the first child not bad and not marked -- the least j < n_kf with d_parent[j] == kf, ascending slot standing in for the
 *          reference's std::set<shared_ptr> order -- is appended and marked; at most one;
 *       4. d_parent[kf] in [0, n_kf) and not marked: appended and marked, and THE WHOLE WALK ENDS ([11] = 2).
 *     Step 4 is the reference's text, not a correction: the `break` of :517 sits in the outer `for`, and the parent is not tested for
 *     bad.  The walk running out of positions gives [11] = 0.  The reference's values are n_neigh = 10 and max_kf = 80.  The marks are
 *     per call: the track_frame_id == current_frame->id stamps are unique per frame, and their id-0 coincidence is not restated.
 *   Points (:525-537).  Over the list in order and each key frame's min(max(d_n[k], 0), stride) slots in order, every p in [0,
 *     cap_points) with d_valid[p] != 0 at its FIRST occurrence; later occurrences are counted in [13], invalid rows in [12].
 *   Outputs.  d_local_kf [cap_local_kf]: the list.  d_rows [cap_rows]: local_map_points in the order above.  d_local_mask [cap_points]
 *     uint8, EVERY entry written: 1 iff the row is in d_rows.  d_ref (device int32, in / out): maxKF when there is one, else untouched
 *     (:522).  Nothing is written at or past a capacity; on a refusal ([2] != 0) the mask is ALL ZERO, d_ref is untouched and what lies
 *     below the capacities is unspecified.  The clearing of d_frame_mp happens regardless: it is idempotent and the reference's first act.
 *   d_work: cap_points + n_kf int32, the caller's, the size of orbm_local_ba_problem_device's (the rows' first occurrences in the first
 *   cap_points; contents afterwards unspecified).
 *   d_result (int32 x 16, written): [0] key frames and [1] rows, both FULL counts; [2] the refusal, a bit mask: 1 more key frames than
 *   cap_local_kf, 2 more rows than cap_rows; [3] maxKF or -1, [4] its votes; [5] - [13] as above; [14], [15] 0.
 *   WHY A MASK.  d_local_mask goes straight into orbm_project_frustum_device as d_valid with nq = the table's row count, so the
 *   queries, and the frame_mp the search fills, stay in the one index space orbba_pose_edges_device documents.  This runs the points
 *   search in ASCENDING ROW ORDER; the reference's order descends from unordered_map iteration, which nothing reproduces.  d_rows is
 *   the reference-shaped list for a caller that gathers instead.
 *
 * orbm_track_counters_device: the counters of one tracked frame.  d_visible, d_found: int32 [cap_points], ACCUMULATED by design.  what,
 * a bit mask (0 .. 7):
 *   1  :388-398.  A slot of d_frame_mp [n2] (in / out) in [0, cap_points) with d_valid == 0 becomes -1 ([3]++); otherwise
 *      d_visible[p]++ ([0]++).
 *   2  :406-408.  d_visible[q]++ for every q < nq with d_q_ok[q] != 0 ([1]++): the frustum builder's q_ok IS that loop's isInFrustum,
 *      and its "already in the frame" gate is :404.  Needs d_q_ok and nq <= cap_points (ORBX_E_ARG); d_q_ok may be NULL without it.
 *   4  :362-364.  d_found[p]++ for every slot in [0, cap_points) ([2]++), with no test for bad, as there; a slot that bit 1 of the same
 *      call cleared is not counted.
 * A caller issues 1 | 2 behind the builder and 4 behind poseOptimize and the drop.  d_result (int32 x 8, written): [0] - [3], the rest 0.
 *
 * orbm_num_tracked_points_device: KeyFrame::getNumTrackedMapPoint(min_obs).  d_kf is a DEVICE int32, the d_ref orbm_local_map_device
 * leaves, so no read-back sits in between; it is distrusted: outside [0, n_kf) gives d_count[0] = 0 and d_count[1] = 1.  d_count[0] =
 * the slots of that key frame holding a p in [0, cap_points) whose live CSR entries number at least min_obs.  No test for bad, as in
 * the reference: a bad row has no live entry, so it fails any min_obs >= 1.  d_count (int32 x 4, written): [0], [1], [2] CSR entries
 * dropped for an index out of range, [3] 0.  The comparison num_inlier < numRefMatch * theRefRatio stays with the caller.
 *
 * Shape (latency, not throughput).  k_local_map is ONE workgroup of 1024 threads: the votes are an LDS array of n_kf ints filled by LDS
 * atomics, a thread per frame slot walking its row's list; the marks are one bit per key frame in LDS; the voted key frames are
 * appended behind a block scan over the slots in order; wave 0 runs the expansion, its lanes across a neighbour list and a ballot for
 * the first child, while the other waves clear d_work; then the rows' first occurrences by atomicMin (the least key wins whatever the
 * order) and the slots in order, a tile of 1024 at a time, numbered by a block scan.  The two small calls clear their result and run a
 * thread per slot / per query.
 * As compiled for gfx950 -- VGPRs / scratch / static LDS: k_local_map 60 / 0 / 33412 B, k_track_counters 14 / 0 / 0 B, k_num_tracked
 * 16 / 0 / 0 B: no scratch memory, at most 64 VGPRs. */
int orbm_local_map_device(orbm_t *h, int32_t *d_frame_mp, int n2, const uint8_t *d_valid, int cap_points, const int32_t *d_obs_off,
                          const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs, int n_kf, const int32_t *d_n, const uint8_t *d_bad,
                          const int32_t *d_slots, int stride, const orbm_covis_graph *graph, const int32_t *recent, int n_recent,
                          int n_neigh, int max_kf, int cap_local_kf, int cap_rows, int32_t *d_work, int32_t *d_local_kf, int32_t *d_rows,
                          uint8_t *d_local_mask, int32_t *d_ref, int32_t *d_result, void *stream);
int orbm_track_counters_device(orbm_t *h, int32_t *d_frame_mp, int n2, const uint8_t *d_valid, int cap_points, const uint8_t *d_q_ok,
                               int nq, int what, int32_t *d_visible, int32_t *d_found, int32_t *d_result, void *stream);
int orbm_num_tracked_points_device(orbm_t *h, const int32_t *d_kf, int min_obs, int n_kf, const int32_t *d_n, const uint8_t *d_bad,
                                   const int32_t *d_slots, int stride, int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf,
                                   const int32_t *d_obs_kp, int n_obs, int32_t *d_count, void *stream);

/* ---- Key frames inserted and recent map points culled on the device ---------------------------------------------------------------
 * The start of every mapper step, which the sections above left on the host: Tracking::createNewKeyFrame with the KeyFrame constructor
 * (modules/Frontend/Tracking.cpp:578-588, modules/BasicObject/KeyFrame.cpp:15-25) and the loop of LocalMapping::processNewKeyFrame
 * (modules/Frontend/LocalMapping.cpp:93-105); the Map / KeyFrame bookkeeping of a triangulated point (:243-248) with the fields of the
 * MapPoint constructor that orbm_triangulate_matches_device does not write (MapPoint.cpp:18, :24-25); and LocalMapping::MapPointCulling
 * (:117-144) with the cascade of MapPoint::setBad (MapPoint.cpp:210-226).  With them the non-inertial body of LocalMapping::Run (:29-62)
 * has a device form for every step, and a tracked frame -- d_frame_mp and the pose orbba_pose_optimize_batch_device left -- becomes a
 * key frame without a read-back.  The map side's rules hold: device pointers only and deliberately NO host-pointer twin; no allocation,
 * handle scratch or host wait; results written, not accumulated; the same bytes on every run (counts are sums, and no stored value
 * depends on the order atomics arrive in); THE SLOT ARRAYS ARE THE TRUTH, the CSR only says where to look and is never rewritten;
 * every index or count read from device memory is distrusted: clamped, or dropped and counted, never dereferenced out of range.
 * Arguments are checked first (ORBX_E_ARG: a null pointer, a negative count, K outside [0, cap_kf), a negative id), then the limits
 * (ORBX_E_UNSUPPORTED: stride > ORBM_MEDIAN_MAX_STRIDE, cap_points > 524288), then the call fails with ORBX_E_NO_DEVICE without a HIP
 * device.  Enqueued on `stream` (NULL: orbx.h, "Streams").
 *
 * orbm_insert_keyframe_device.  K: the new key frame's slot, the caller's choice, in [0, cap_kf).  d_pose_R [cap_kf][9], d_pose_t
 * [cap_kf][3], d_bad, d_kps, d_desc, d_n [cap_kf]: the arrays an orbm_kf_table points to, here as their owner holds them (the two
 * pointer arrays pointer aligned).  d_slots, stride, d_valid, cap_points: the layout of orbm_build_observations_device.  The frame:
 * d_frame_mp [n2], table rows in the convention of orbm_track_counters_device, READ ONLY (the reference erases on the KeyFrame, not
 * on the Frame) and not overlapping d_slots; d_frame_pose_R [9] / d_frame_pose_t [3], device doubles as the pose optimisation leaves
 * them; frame_kps / frame_desc, the HOST VALUES of the device pointers to the frame's orbx_kp records and descriptors.
 *   Row K of the table: the pose copied bit for bit, d_bad[K] = 0, d_n[K] = n2, d_kps[K] = frame_kps, d_desc[K] = frame_desc.
 *   EVERY one of the stride slots of row K is written, so nothing of an earlier use of the row survives.  Slot i < min(n2, stride),
 *   p = d_frame_mp[i]:
 *     p == -1                                the slot becomes -1
 *     else p outside [0, cap_points)         the slot becomes -1, [3]++
 *     else d_valid[p] == 0                   the slot becomes -1, [2]++: eraseMapPoint (:98)
 *     else                                   the slot becomes p, [0]++: the slot IS the observation, so addObservation (:100) is this store
 *   Slots i >= min(n2, stride) become -1.  A row that a lower slot of K already names keeps its second slot -- the reference's
 *   map_points[i] keeps it too, only addObservation refuses (MapPoint.cpp:184) -- and is counted in [4] as (slots holding a point) -
 *   (distinct rows), through a mask of one bit per table row, so the count does not depend on order; orbm_build_observations_device
 *   emits both entries of such a row and counts it.
 *   d_result (int32 x 8, written): [0] slots holding a point, [1] 0, [2] slots cleared because the row is invalid, [3] values outside
 *   [0, cap_points) other than -1, [4] slots naming a row that a lower slot of K already names, [5] max(n2 - stride, 0), [6], [7] 0.
 *   The chain.  `mp->computeDescriptor(); mp->update();` (:101-102) and `current_kf->updateConnections()` (:108) are the calls the
 *   sections above have: this call -> orbm_build_observations_device -> orbm_refresh_points_device with d_sel = d_slots + K * stride,
 *   n_sel = stride and kf_self = K -> orbm_update_connections_device with the same kf_self.
 *
 * orbm_register_new_points_device: what LocalMapping.cpp:243-248 and MapPoint.cpp:18, :24-25 leave for the rows that
 * orbm_triangulate_matches_device appended.  d_n_points: the device int the triangulation advances; d_n_registered: a device int,
 * in / out, rows below it are finished; K: the current key frame's slot; kf_id: its KeyFrame::id, by which the culling ages points --
 * it counts culled key frames too, so a caller that never reuses a slot passes K.  d_ref_kf (the refresh's), d_first_kf, d_found,
 * d_visible (the counters of orbm_track_counters_device): int32 [cap_points].  d_recent [cap_recent] with the device int d_n_recent,
 * in / out: recent_map_points as table rows.
 *   a = clamp(*d_n_registered, 0, cap_points), b = clamp(*d_n_points, 0, cap_points), r = clamp(*d_n_recent, 0, cap_recent).
 *   Refusal 2 when a > b; refusal 1 when r + (b - a) > cap_recent; on a refusal nothing but d_result is written ([4] is then r).
 *   Otherwise for rows a .. b - 1: d_ref_kf = K, d_first_kf = kf_id, d_found = d_visible = 1, d_recent[r + (row - a)] = row -- ascending
 *   row order, the creation order, the reference's push_back order -- then *d_n_recent = r + (b - a) and *d_n_registered = b.
 *   Rows are registered whether or not a fuse has set them bad meanwhile: the reference pushes at creation and the culling removes them.
 *   One call may follow each triangulation or only the last one of a step; the bytes are the same either way.
 *   d_result (int32 x 8, written): [0] rows registered, [1] the refusal, [2] a, [3] b, [4] the new *d_n_recent, [5] - [7] 0.
 *
 * orbm_cull_map_points_device.  d_recent / d_n_recent (in / out), cap_recent: the list above; cur_kf_id: current_kf->id; d_first_kf,
 * d_found, d_visible: read only; d_valid, d_slots: in / out; n_kf, d_n, d_bad, stride, cap_points and the CSR (d_obs_off / d_obs_kf /
 * d_obs_kp, n_obs): the layout of orbm_build_observations_device and what it left from these slots.  n = clamp(*d_n_recent, 0,
 * cap_recent).  For entry j < n, p = d_recent[j]; the first rule that applies decides d_code[j] (d_code [cap_recent], int32; entries at
 * and past n are not written):
 *   -1  p outside [0, cap_points)                                                      dropped from the list, [7]++
 *    1  d_valid[p] == 0                                                         :126   removed from the list, [2]++ (numBad)
 *    2  (float) d_found[p] / (float) d_visible[p] < 0.25f      :129, MapPoint.cpp:278   setBad(p), removed, [3]++ (numFoundRatio)
 *    3  (uint32_t) cur_kf_id - (uint32_t) d_first_kf[p] >= 2 and numObs(p) <= 2  :133   setBad(p), removed, [4]++
 *    4  that difference > 2                                                     :136   removed from the list only, [5]++
 *    0  otherwise                                                                      kept, [0]++
 *   The float division is literal: 0 / 0 is NaN and compares false, x / 0 is +-inf, negative counts divide as they are.  The reference's
 *   difference is unsigned 64-bit (an unsigned int less an unsigned long); for non-negative ids the 32-bit wrap gives the same two
 *   verdicts: a first id above the current one wraps to at least 2^31 + 1 here and to nearly 2^64 there, both beyond 2.
 *   numObs(p) = the LIVE CSR entries of p (the slot names p now and its key frame is not bad): getNumObs() as orbm_fuse_apply_device
 *   defines it.  setBad(p): d_valid[p] = 0 and d_slots[k * stride + i] = -1 for every live entry ([6]++ each); a slot in a bad key frame
 *   is no observation and stays, as in the fuse.  No list-length limit: nothing is staged, a list is walked as it is.  The CSR is read
 *   with the culling's distrust: offsets that do not describe a list inside [0, n_obs] give an empty list; an entry whose key frame is
 *   outside [0, n_kf) or whose feature is outside [0, min(max(d_n[k], 0), stride)) is dropped, never dereferenced, and counted in [7]
 *   once each over all of [0, n_obs).
 *   The kept entries are compacted IN PLACE in list order -- a tile's reads, a barrier, its writes behind a block scan -- and
 *   *d_n_recent becomes their number; the entries of d_recent at and past it are as passed.
 *   Why it is parallel: a setBad touches only slots that name its own row and numObs(q) reads only slots that name q, so entries of
 *   different rows do not interact and a thread per entry gives the sequential loop's result.  The one premise, that no row occurs
 *   twice in the list (the reference's list gets one push_back per constructed point), is checked over all tiles BEFORE anything is
 *   written: on a violation d_result = {0, 1, 0 ...} and d_recent, *d_n_recent, d_valid, d_slots and d_code are exactly as passed.
 *   d_result (int32 x 8, written): [0] kept, [1] the refusal, [2] already bad, [3] found ratio, [4] few observations, [5] aged out, [6]
 *   slots cleared, [7] entries of code -1 plus CSR entries dropped.  Map::eraseMapPoint stays with the caller, who reads d_code; rows
 *   are never reused.
 *
 * Shape (latency, not throughput: hundreds to a few thousand entries).  Each call is ONE launch of ONE workgroup of 1024 threads that
 * walks its input in tiles of 1024 with workgroup barriers between the phases.  k_kf_insert and k_kf_cull_points keep one bit per table
 * row in dynamic LDS (cap_points / 8 bytes, hence cap_points <= 524288): the distinct rows of K, and the premise.  k_kf_register reads
 * its three counters in every thread ahead of a barrier, and one thread rewrites them behind the last tile.
 * As compiled for gfx950 -- VGPRs / scratch / static LDS: k_kf_insert 16 / 0 / 32 B, k_kf_register 32 / 0 / 0 B, k_kf_cull_points
 * 42 / 0 / 352 B: no scratch memory, at most 64 VGPRs. */
int orbm_insert_keyframe_device(orbm_t *h, int K, int cap_kf, double *d_pose_R, double *d_pose_t, uint8_t *d_bad, const void **d_kps,
                                const uint8_t **d_desc, int32_t *d_n, int32_t *d_slots, int stride, const uint8_t *d_valid,
                                int cap_points, const int32_t *d_frame_mp, int n2, const double *d_frame_pose_R,
                                const double *d_frame_pose_t, const void *frame_kps, const uint8_t *frame_desc, int32_t *d_result,
                                void *stream);
int orbm_register_new_points_device(orbm_t *h, const int32_t *d_n_points, int32_t *d_n_registered, int K, int kf_id, int cap_points,
                                    int32_t *d_ref_kf, int32_t *d_first_kf, int32_t *d_found, int32_t *d_visible, int32_t *d_recent,
                                    int cap_recent, int32_t *d_n_recent, int32_t *d_result, void *stream);
int orbm_cull_map_points_device(orbm_t *h, int32_t *d_recent, int32_t *d_n_recent, int cap_recent, int cur_kf_id,
                                const int32_t *d_first_kf, const int32_t *d_found, const int32_t *d_visible, uint8_t *d_valid,
                                int cap_points, int n_kf, const int32_t *d_n, const uint8_t *d_bad, int32_t *d_slots, int stride,
                                const int32_t *d_obs_off, const int32_t *d_obs_kf, const int32_t *d_obs_kp, int n_obs, int32_t *d_code,
                                int32_t *d_result, void *stream);

/* ---- The inertial local BA window on the device-resident map ----------------------------------------------------------------------
 * Optimize::localFullBundleAdjustment (modules/Backend/Optimize.cpp:1064-1310, what every key frame runs once the IMU is initialised)
 * for a caller whose slot arrays, map-point table, key-frame table, state rows, record bank and priors live in device memory.  Every
 * numeric stage of it exists: the inertial edges, priors and bias walks (orbi_factors.h), EdgeMono with the Schur complement, the
 * 480-unknown solve and the back-substitution (the visual-window header).  This section is the piece between the map and those calls:
 *   orbm_inertial_window_problem_device          :1073-1108, :1129-1244  steps 1 and 3: solve states, local points, fixed key frames
 *                                                under the reference's cap, the EdgeMono arrays and the inertial side's job lists
 *   orbm_inertial_window_velocity_prior_device   :1288 (KeyFrame::setVelocity)  velo_priori of the OLDEST key frame, step 7's remainder
 * and the mapper step after IMU initialisation is one chain on one stream:
 *   the assembly -> ONE read-back of d_result's first 32 bytes (the sizes are host ints of the calls below)
 *   orbi_graph_init_device (d_init_jobs) -> orbi_edge_information_device (d_inertial_edges)
 *   the caller's Levenberg-Marquardt loop over orbi_linearize_device (d_inertial_edges, d_prior_jobs) and the visual-window header's
 *     calls (d_ba_points, d_edge_state, d_edge_point, d_edge_z, d_edge_inv_sigma2, d_fixed); its per-trial scalars are the only other
 *     read-backs.  THE LOOP IS NOT HERE: its decisions are the caller's (tests/inertial_loop.py closes it as test code)
 *   the visual-window linearisation in mode 2 -> d_outlier
 *   orbi_graph_recover_device (d_recover_jobs; its d_pose_R / d_pose_t are T_cw of the solve states)
 *   orbm_local_ba_apply_device, UNCHANGED, with n_local = n_solve, d_pose_kf = d_state_kf, those poses, the live point buffer and
 *     d_outlier: the outlier observations erased with their cascade (:1263-1272), T_cw into the key-frame table (:1287), the
 *     positions written back (:1301-1307).  The assembly emits its maps in that call's layout for exactly this
 *   orbi_set_bias_device (d_bias_ids, the recover's d_bias; :1291) -> orbi_prior_information_device (d_prior_info_jobs; :1293-1296)
 *   orbm_inertial_window_velocity_prior_device
 *   orbm_build_observations_device -> orbm_refresh_points_device (d_sel = d_point_row; mp->update(), :1305)
 * (The recover runs ahead of the apply, which reads its poses; the other calls behind the loop are independent of each other.)
 * inertialOptimize / fullInertialOptimize and the loop itself are not here.  localInertialBundleAdjustment, what the mapper runs in front of
 * this function when the tracker is RECENTLY_LOST, is the next section ("The inertial chain on the device-resident map") with orbil.h.
 * The two calls follow this header's rules for the map side, as "Local bundle adjustment on the device-resident map" states them:
 * device pointers only and deliberately NO host-pointer twin; no allocation, handle scratch or host wait; results written, not
 * accumulated; the same bytes on every run; every index that comes from device memory is distrusted -- dropped and counted, never
 * dereferenced out of range.  THE SLOT ARRAYS ARE THE TRUTH, the CSR only tells where the slots naming a row are, and LIVE is as there.
 * This header does not include the headers of the calls above: the job lists are int32 arrays in their documented layouts.
 *
 * orbm_inertial_window_problem_device.  The map as orbm_local_ba_problem_device takes it.  d_window [n_window] (device): the slots of
 * getRecentKeyFrames(numOpt), OLDEST FIRST as Map.cpp:42-53 returns them; the caller computes numOpt = min(n - 2, 10 or 25).  d_kf_imu
 * [n_kf][3] (device) = per key frame (its row of the 15-float state array, its record of the orbi_record bank, its orbi_prior slot), held
 * against the host ints n_src, cap_bank, n_priors.  max_fixed: the reference's maxNumFixed, ORBM_IW_MAX_FIXED_DEFAULT.
 *   Solve states (:1076-1079): state s is d_window[s].  The inertial chain is positional, so NOTHING IS SKIPPED -- where the local BA
 *     drops an entry of d_local that is out of range, bad or repeated and goes on, here such an entry (outside [0, n_kf), a bad key
 *     frame, a key frame an earlier entry named; counted in d_result[6]) REFUSES the whole call, bit 8 of d_result[5]: the call stops
 *     there, d_result[0] = d_result[3] = n_window, every other count is 0 and no output array is written.  A window key frame one of
 *     whose three d_kf_imu indices is out of range refuses the call as well (bit 32, counted in d_result[7]); the counts are then full.
 *     n_solve = n_window.
 *   Local points (:1083-1092): the rows p in [0, cap_points) with d_valid[p] != 0 named by one of the min(max(d_n[k], 0), stride) slots
 *     of a window key frame, each numbered at its FIRST occurrence in (window position, slot) order -- the reference's BA_local_for_kf
 *     marking, orbm_local_ba_problem_device's rule.  A row that ends up without an edge is dropped before numbering (d_result[8]).
 *   Fixed key frames, with the reference's cap (:1095-1108): for every key frame f that is not in the window and not bad, first[f] =
 *     the smallest local-point number with a LIVE CSR entry on f (d_result[13] counts the key frames that have one).  X = the smallest
 *     point number at which #{f : first[f] <= X} >= max_fixed, no bound when the count never gets there; the fixed set is {f :
 *     first[f] <= X}, INCLUSIVE -- the reference pushes every observer of a point and only then breaks.  (The kernel orders rows by
 *     their first-occurrence keys, which order them as their numbers do, so the set needs no numbering and no order of execution.)
 *     Fixed states follow the solve states in ASCENDING SLOT ORDER: a stated canonicalisation, the one of the local BA -- the
 *     reference's order is the order it met them, and a fixed pose has no block in the system, so its position reaches no number.  A
 *     fixed key frame whose state row is outside [0, n_src) refuses the call (bit 32, d_result[7]).
 *   Edges (:1218-1244): per local point in order, its LIVE CSR entries in CSR order whose key frame is a solve or a fixed state.  A key
 *     frame's second entry in one row gives no second edge (d_result[9]; tested first).  An entry on a live key frame that is neither a
 *     solve nor a fixed state is dropped (d_result[11]); that only happens behind the cap and is the second stated canonicalisation:
 *     the reference hands g2o a null vertex there.  A point with more than 256 kept edges is emitted and counted (d_result[12]): the
 *     linearisation drops such a point whole and the caller should know.
 *   Outputs for the visual window, in the layout its calls and orbm_local_ba_apply_device take: d_ba_points [x][3] = (double) of
 *     d_points[d_point_row[x]]; d_point_row [x]; d_edge_off [n_points + 1]; for edge e of point x d_edge_point[e] = x (non-decreasing),
 *     d_edge_state[e] = the state of its key frame, d_edge_z[2e ..] = the orbx_kp record's (x, y) widened, d_edge_inv_sigma2[e] =
 *     (double)((1.f / size) / size) (:1233), d_edge_kf / d_edge_kp[e] = (key-frame slot, feature); d_state_kf [n_states] = the slots.
 *   Outputs for the inertial side, ready job lists:
 *     d_init_jobs [n_states][3]       orbi_graph_init_device: (state, state row, record; record -1 for a fixed state: no bias vertices)
 *     d_fixed [n_states]              0 for a solve state, ORBI_FIX_POSE | _VELO | _GYRO | _ACC (15) for a fixed one
 *     d_inertial_edges [n_solve - 1]  orbi_edge (4 x int32) {s, s + 1, record of key frame s, ORBI_EDGE_WALKS (1)}: :1153-1174 takes the
 *                                     OLDER key frame's pre-integrator, and its C for both walks
 *     d_prior_jobs [1][3]             orbi_prior_job (state 0, prior slot of the oldest key frame, VELO | GYRO | ACC | ACC_GYRO_INFO = 15), :1176-1191
 *     d_recover_jobs [n_solve][3]     orbi_graph_recover_device: (s, state row, ORBI_RECOVER_POSE (1))
 *     d_bias_ids [n_solve]            the records, orbi_set_bias_device's d_ids
 *     d_prior_info_jobs [n_solve - 1][3]  orbi_prior_information_device, for s >= 1: (prior slot of key frame s, record of key frame s - 1,
 *                                     state row of key frame s) -- :1293-1296 with bias_priori = the previous key frame's new bias
 * Capacities: d_state_kf, d_fixed [cap_states], d_init_jobs [cap_states][3]; d_ba_points [cap_local_points][3], d_point_row
 * [cap_local_points], d_edge_off [cap_local_points + 1]; d_edge_state, d_edge_point, d_edge_inv_sigma2, d_edge_kf, d_edge_kp [cap_edges],
 * d_edge_z [cap_edges][2]; d_inertial_edges [n_window - 1][4], d_prior_jobs [3], d_recover_jobs [n_window][3], d_bias_ids [n_window],
 * d_prior_info_jobs [n_window - 1][3] (none may be NULL; with n_window = 1 the two lists of n_window - 1 are not written).  d_work: the
 * caller's work array of cap_points + 2 * n_kf int32 (contents afterwards unspecified).
 * d_result (int32 x 16, written; the first eight -- 32 bytes -- are what the caller reads back): [0] n_states, [1] n_points, [2]
 * n_edges, [3] n_solve, [4] n_fixed, [5] the refusal, a bit mask: 1 more states than cap_states, 2 more points than cap_local_points,
 * 4 more edges than cap_edges, 8 a window entry unusable, 16 no edge, 32 an imu index out of range; [6] window entries unusable, [7]
 * key frames with a d_kf_imu index out of range; [8] rows dropped for having no edge, [9] second edges of a key frame in one row,
 * [10] CSR entries dropped for an index out of range, [11] entries dropped behind the cap, [12] points with more than 256 edges,
 * [13] key frames that could be fixed without a cap; the rest 0.  On a refusal other than bit 8 the counts are the FULL counts, no
 * array is written at or past its capacity, the job lists and measurements are not written and what lies below is unspecified.
 * Shape: ONE launch of ONE workgroup of 1024 threads with barriers between the phases, as orbm_local_ba_problem_device, with which it
 * shares the slot walk, the live-entry walk and the second-entry test (csrc/orbm_map.h) -- 10-25 key frames x 2000 slots x short lists
 * are latency.  The cap costs one more walk of the lists (an integer atomicMin per entry) and a counting binary search of at most 18
 * rounds over the keys.  Integer atomics only.  As compiled for gfx950 -- VGPRs / scratch / static LDS: k_iw_problem 58 / 0 /
 * 320 B, k_iw_velocity_prior 6 / 0 / 0 B: no scratch memory, at most 64 VGPRs.
 * Limits (ORBX_E_UNSUPPORTED above): n_window <= ORBM_IW_MAX_SOLVE (the solve's 480 unknowns), stride <= ORBM_MEDIAN_MAX_STRIDE,
 * cap_points <= 524288.  Arguments are checked first (ORBX_E_ARG: a null pointer, a negative count, n_window, max_fixed and the
 * capacities >= 1); without a HIP device the call fails with ORBX_E_NO_DEVICE.  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
#define ORBM_IW_MAX_SOLVE 32
#define ORBM_IW_MAX_FIXED_DEFAULT 150
struct orbi_prior;
int orbm_inertial_window_problem_device(orbm_t *h, const orbm_kf_table *kf, const int32_t *d_slots, int stride, const uint8_t *d_valid,
                                        const float *d_points, int cap_points, const int32_t *d_obs_off, const int32_t *d_obs_kf,
                                        const int32_t *d_obs_kp, int n_obs, const int32_t *d_window, int n_window, const int32_t *d_kf_imu,
                                        int n_src, int cap_bank, int n_priors, int max_fixed, int cap_states, int cap_local_points,
                                        int cap_edges, int32_t *d_work, double *d_ba_points, int32_t *d_point_row, int32_t *d_edge_off,
                                        int32_t *d_edge_state, int32_t *d_edge_point, double *d_edge_z, double *d_edge_inv_sigma2,
                                        int32_t *d_edge_kf, int32_t *d_edge_kp, int32_t *d_state_kf, int32_t *d_init_jobs, uint8_t *d_fixed,
                                        int32_t *d_inertial_edges, int32_t *d_prior_jobs, int32_t *d_recover_jobs, int32_t *d_bias_ids,
                                        int32_t *d_prior_info_jobs, int32_t *d_result, void *stream);

/* orbm_inertial_window_velocity_prior_device.  KeyFrame::setVelocity (KeyFrame.cpp:65-69) also sets velo_priori, and step 7 calls it
 * for every window key frame; orbi_prior_information_device does that for the key frames s >= 1 (its source state), the OLDEST gets no
 * setPrioriInformation.  This call: with (s, row, flags) = the FIRST entry of d_recover_jobs and (state, slot, mask) = the FIRST entry
 * of d_prior_jobs, d_priors[slot].velo_priori = d_src[15 * row + 12 ..), the three floats orbi_graph_recover_device left; bias_priori and
 * the three information matrices of the slot are not touched.  d_priors: the orbi_prior array (36 floats a slot).  A row outside
 * [0, n_src) or a slot outside [0, n_priors): nothing is written.  d_result (int32 x 8, written): [0] 1 written, [1] 1 dropped.
 * One launch of one wave.  ORBX_E_ARG: a null pointer, a negative count; then ORBX_E_NO_DEVICE.  Enqueued on `stream`. */
int orbm_inertial_window_velocity_prior_device(orbm_t *h, struct orbi_prior *d_priors, int n_priors, const float *d_src, int n_src,
                                               const int32_t *d_recover_jobs, const int32_t *d_prior_jobs, int32_t *d_result, void *stream);

/* ---- The inertial chain on the device-resident map ---------------------------------------------------------------------------------
 * Optimize::localInertialBundleAdjustment (modules/Backend/Optimize.cpp:953-1062), which the mapper runs when the tracker is
 * RECENTLY_LOST (LocalMapping.cpp:47-48), directly in front of localFullBundleAdjustment, for a caller whose key-frame table, state
 * rows, record bank and priors live in device memory.  Its graph is the last min(n, 10 or 20) key frames with every pose a constant; its
 * formulas are orbi_factors.h's and its optimisation is orbil.h's, one launch.  This section is the piece between the map and those calls:
 *   orbm_inertial_chain_problem_device           :965-1029  steps 1 and 3: the states, their fixed flags, the edges and the job lists
 *   orbm_inertial_chain_velocity_priors_device   :1044-1053 (KeyFrame::setVelocity)  velo_priori of EVERY window key frame
 * and the mapper step is one chain on one stream
 *   the assembly -> orbi_graph_init_device (d_init_jobs) -> orbi_edge_information_device (d_inertial_edges)
 *     -> orbil_chain_optimize_device (d_fixed, d_inertial_edges) -> orbi_graph_recover_device (d_recover_jobs)
 *     -> orbi_set_bias_device (d_bias_ids, the recover's d_bias) -> orbm_inertial_chain_velocity_priors_device (d_velo_jobs)
 * in which the host knows every size (n_window states, n_window - 1 edges): THE CHAIN HAS NO READ-BACK AT ALL.  The rules are those of
 * "The inertial local BA window on the device-resident map": device pointers only, no host-pointer twin, no allocation, handle scratch
 * or host wait, results written, the same bytes on every run, every index from device memory distrusted.  This header does not include
 * the headers of the calls above: the job lists are int32 arrays in their documented layouts.
 *
 * orbm_inertial_chain_problem_device.  d_window [n_window] (device): the slots of getRecentKeyFrames(numOpt), OLDEST FIRST; the caller
 * computes numOpt = min(n, 10 or 20) (:959-963).  d_bad [n_kf]: the key-frame table's bad flags.  d_kf_imu [n_kf][3] (device) = per key
 * frame (its row of the 15-float state array, its record of the orbi_record bank, its orbi_prior slot), held against the host ints n_src,
 * cap_bank, n_priors -- the map the window assembly takes.  Outputs, state s = d_window[s]:
 *     d_init_jobs [n_window][3]        orbi_graph_init_device: (s, state row, record)
 *     d_fixed [n_window]               15 for state 0 -- setFixed(i == 0) on its three vertices (:992-1007); it has no pose vertex --,
 *                                      ORBI_FIX_POSE (1) for the rest: the poses are constants of EdgeInertialOnly
 *     d_inertial_edges [n_window - 1]  orbi_edge (4 x int32) {s, s + 1, record of key frame s, ORBI_EDGE_WALKS (1)}: :1012-1029 takes the
 *                                      OLDER key frame's pre-integrator, and its C for both walks
 *     d_recover_jobs [n_window][3]     orbi_graph_recover_device: (s, state row, 0): velocity and biases, no pose
 *     d_bias_ids [n_window]            the records, orbi_set_bias_device's d_ids
 *     d_velo_jobs [n_window][2]        the call below: (state row, prior slot)
 *     d_state_kf [n_window]            the slots
 *   Refusal.  The chain is positional, so NOTHING IS SKIPPED: a window entry outside [0, n_kf), a bad key frame, a key frame an earlier
 *   entry named (bit 8 of d_result[1], counted in [2]) or a window key frame one of whose three d_kf_imu indices is out of range (bit
 *   32, counted in [3]) REFUSES the whole call, AND THE REFUSAL IS HONOURED ON THE DEVICE: every entry of every job list is -1,
 *   d_inertial_edges and d_state_kf included, and d_fixed is all 15, so every call behind it drops every job by its own distrust, the
 *   optimisation finds no free vertex and no edge, and the state rows, the bank's biases and the priors keep their bytes.
 *   d_result (int32 x 8, written): [0] n_window, [1] the refusal, a bit mask (8, 32: the window assembly's bits), [2] window entries
 *   unusable, [3] key frames with a d_kf_imu index out of range; the rest 0.
 *   Shape: ONE launch of ONE workgroup of 64 threads, a thread per position; integer work only.  ORBX_E_ARG: a null pointer, a negative
 *   count, n_window < 2; ORBX_E_UNSUPPORTED: n_window > ORBM_IC_MAX_WINDOW (20, the reference's maxOpt with beLarge and orbil.h's cap);
 *   then ORBX_E_NO_DEVICE.  Enqueued on `stream` (NULL: orbx.h, "Streams").
 *
 * orbm_inertial_chain_velocity_priors_device.  KeyFrame::setVelocity (KeyFrame.cpp:65-69) also sets velo_priori, and :1044-1053 call it
 * for every window key frame.  For each of the n jobs (row, slot) of d_velo_jobs, d_priors[slot].velo_priori = d_src[15 * row + 12 ..),
 * the three floats orbi_graph_recover_device left; nothing else of the slot is touched.  A row outside [0, n_src) or a slot outside
 * [0, n_priors) is dropped.  d_result (int32 x 8, written): [0] written, [1] dropped.  One launch of one wave.  ORBX_E_ARG: a null
 * pointer, a negative count; ORBX_E_UNSUPPORTED: n > ORBM_IC_MAX_WINDOW; then ORBX_E_NO_DEVICE.  Enqueued on `stream`.
 * As compiled for gfx950 -- VGPRs / scratch / static LDS: k_ic_problem 22 / 0 / 192 B, k_ic_velocity_priors 14 / 0 / 32 B. */
#define ORBM_IC_MAX_WINDOW 20
int orbm_inertial_chain_problem_device(orbm_t *h, int n_kf, const uint8_t *d_bad, const int32_t *d_window, int n_window,
                                       const int32_t *d_kf_imu, int n_src, int cap_bank, int n_priors, int32_t *d_init_jobs,
                                       uint8_t *d_fixed, int32_t *d_inertial_edges, int32_t *d_recover_jobs, int32_t *d_bias_ids,
                                       int32_t *d_velo_jobs, int32_t *d_state_kf, int32_t *d_result, void *stream);
int orbm_inertial_chain_velocity_priors_device(orbm_t *h, struct orbi_prior *d_priors, int n_priors, const float *d_src, int n_src,
                                               const int32_t *d_velo_jobs, int n, int32_t *d_result, void *stream);

/* ---- The map rescaled and rotated on the device ------------------------------------------------------------------------------------
 * Map::applyScaleRotation (modules/BasicObject/Map.cpp:96-124), what LocalMapping::initializeIMU does with the gravity direction and
 * the scale its optimisation found (LocalMapping.cpp:435-445), for a caller whose key-frame table, state rows, prior slots and map-point
 * table live in device memory.  The steps ahead of it are orbii.h's; this header does not include it.
 *   d_summary [10] (device, float): Rwy = d_summary[0..9) row-major and s = d_summary[9], as orbii_recover_device leaves them.  THEY ARE
 *     READ ON THE DEVICE, and so is the reference's decision (LocalMapping.cpp:435-439): with be_first != 0 and s < min_scale (0.1f) the
 *     call writes NOTHING but d_result, where [3] = 1 -- the chain needs no host wait to honour it.
 *   Otherwise, float, no fused multiply-add, product-sums as (p0 + p1) + p2, Ryw = Rwy^T, (Ryw * x) * s read left to right:
 *     per key frame k < n_kf with d_bad[k] == 0 (T_cw = d_pose_R / d_pose_t [k], doubles rounded to float first; the results are stored
 *     as doubles holding floats):  R_cw <- R_cw * Rwy;  t_cw <- t_cw * s with be_first, else unchanged  (KeyFrame::setPose, Map.cpp:103-105).
 *     Through d_kf_imu [n_kf][3] = (state row, record, prior slot), the map of orbm_inertial_window_problem_device: the state row's
 *     (Rwb, twb) = T_cw.inverse() * T_cb of the NEW pose (KeyFrame.cpp:33), by the code of orbi_imu_pose_device; its v <- (Ryw * v) * s
 *     (without `* s` when be_first == 0), which also goes to velo_priori of the prior slot (KeyFrame::setVelocity).  A key frame whose
 *     state row or prior slot is outside [0, n_src) / [0, n_priors) ([1]), or names the row or slot of an earlier key frame that is not bad
 *     ([2]), has its pose updated and neither its row nor its slot touched.  The record is not read.
 *     per row p < min(max(*d_n_points, 0), cap_points) with d_valid[p] != 0:  pos <- (Ryw * pos) * s  (Map.cpp:117-119).
 *   mp->update() (Map.cpp:120) is the caller's orbm_build_observations_device + orbm_refresh_points_device over all rows, and
 *   tracker->updateFrameIMU() is orbi_predict_device; both exist.
 * d_result (int32 x 8, written): [0] key frames whose row and slot were written, [1], [2] as above, [3] 1 when refused, [4] points moved.
 * calib: a host struct (orbi.h's orbi_calib), copied into the launch.  Device pointers only, no host-pointer twin, no allocation, no
 * handle scratch, no host wait; integer atomics only, so the same input gives the same bytes.  Three launches: the counters, a wave per
 * key frame (four per workgroup), a thread per point row.  As compiled for gfx950 -- VGPRs / scratch / static LDS: k_rescale_begin
 * 2 / 0 / 0 B, k_rescale_kf 12 / 0 / 768 B, k_rescale_points 10 / 0 / 4 B.
 * Arguments are checked first (ORBX_E_ARG: a null pointer, a negative count; ORBX_E_UNSUPPORTED: cap_points > 524288); without a HIP
 * device the call fails with ORBX_E_NO_DEVICE.  n_kf = 0 and cap_points = 0 are allowed.  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
struct orbi_calib;
int orbm_apply_scale_rotation_device(orbm_t *h, const struct orbi_calib *calib, int n_kf, double *d_pose_R, double *d_pose_t,
                                     const uint8_t *d_bad, const int32_t *d_kf_imu, float *d_state, int n_src, struct orbi_prior *d_priors,
                                     int n_priors, float *d_points, const uint8_t *d_valid, const int32_t *d_n_points, int cap_points,
                                     const float *d_summary, int be_first, float min_scale, int32_t *d_result, void *stream);

/* ---- Two-view initialisation: the H / F RANSAC ---------------------------------------------------------------------------------------
 * The front half of TwoViewReconstruction::Reconstruct (modules/Frontend/TwoViewReconstruction.cpp:14-84, reached from
 * Tracking.cpp:620 through Pinhole.cpp:90 / Fisheye.cpp:138), the consumer of the d_matches12 that
 * orbm_search_for_initialization_device leaves on the device: the match list (:26-30), the draw of the eight-point sets (:42-58),
 * FindHomography and FindFundamental (:86-161) with ComputeH21 / ComputeF21 (:163-224), CheckHomography / CheckFundamental (:226-344)
 * and Normalize (:558-596), and the RH decision (:73-79).  ReconstructH / ReconstructF / CheckRT / DecomposeE: the next section, orbm_two_view_pose_device.
 *
 * Inputs.  d_kps1 [n1], d_kps2 [n2]: orbx_kp records, UNDISTORTED by the caller (Fisheye's cv::fisheye::undistortPoints is not part
 * of this); only x and y are read.  d_matches12 [n1]: m in [0, n2) is a match, anything else none.  sigma: the reference's 1.f
 * (Pinhole.cpp:86); invSigma2 = 1.f / (sigma * sigma).  iters: max_iterations (200 there), 1 .. ORBM_TWO_VIEW_MAX_ITERS.
 * d_sets: NULL -- the sets are drawn on the device from rng_state as orbm_two_view_sets draws them (0: cv::RNG's default state,
 * ORBM_TWO_VIEW_RNG_DEFAULT) -- or [iters][8] int32 indices into the match list, for a caller who wants the draw of their own
 * OpenCV; an index outside the list is kept inside it.
 *
 * Arithmetic (float unless said otherwise, no fused multiply-add; `/` and sqrt correctly rounded; a product-sum of three reads
 * (p0 + p1) + p2):
 *   Normalize over ALL key points of a frame, matched or not: meanX = sum(x) / N, meanDevX = sum(fabsf(x - meanX)) / N, sX = 1.f / meanDevX,
 *     T = [sX, 0, -meanX * sX; 0, sY, -meanY * sY; 0, 0, 1]; a point is ((x - meanX) * sX, (y - meanY) * sY).  The four sums are TREES
 *     (a thread's stride of 1024, the wave's butterfly, the sixteen waves in order), so T1 and T2 differ from the reference's running
 *     float sums in the last bits.
 *   The matrix of :172-190 (16 x 9) / :207-215 (8 x 9) from the normalised sample, its entries multiplied in float.  From here to the
 *     de-normalised 3 x 3 the arithmetic is DOUBLE on those floats and on the float entries of T1 and T2, rounded to float once at the
 *     end: a float Jacobi of 360 rotations would leave several times the error of the float SVD the reference runs.
 *   Hn, Fn = the right singular vector of the matrix's smallest singular value, row-major 3 x 3 (a one-sided Jacobi, a fixed number of
 *     sweeps: not bit-reproducible by another SVD; csrc/orbm_two_view.hip); Fn then loses its smallest singular value (:220-223), by
 *     the same method on the 3 x 3.
 *   H21 = (T2^-1 * Hn) * T1 with T2^-1 = [1 / sX2, 0, meanX2; 0, 1 / sY2, meanY2; 0, 0, 1];  F21 = (T2^T * Fn) * T1; the zeros of
 *     T are not multiplied: M = T2^-1 * Hn has M(0, c) = (1 / sX2) * Hn(0, c) + meanX2 * Hn(2, c), T2^T * Fn has M(2, c) =
 *     (T2(0, 2) * Fn(0, c) + T2(1, 2) * Fn(1, c)) + Fn(2, c), and X = M * T1 has X(r, 0) = M(r, 0) * sX1, X(r, 1) = M(r, 1) * sY1,
 *     X(r, 2) = (M(r, 0) * T1(0, 2) + M(r, 1) * T1(1, 2)) + M(r, 2).  From here on float again, on the rounded H21 and F21.
 *   CheckHomography per match, H12 = the cofactors of the float H21 times 1 / det, det = (h11 * c11 - h12 * c12) + h13 * c13, in double
 *     and rounded to float once (H21 mixes entries of 1e-3 and of 1e2: a float inverse is off by 1e-3 relative in places, LAPACK's less):
 *     w = 1.f / ((h31inv * u2 + h32inv * v2) + h33inv), u2in1 = ((h11inv * u2 + h12inv * v2) + h13inv) * w, v2in1 alike,
 *     chiSquare1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * invSigma2; the second side with H21 and (u1, v1);
 *     th = 5.991f.  CheckFundamental: a2 = (f11 * u1 + f12 * v1) + f13, b2, c2 alike, num2 = (a2 * u2 + b2 * v2) + c2,
 *     chiSquare1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * invSigma2; the second side with the columns of F21 and (u2, v2);
 *     th = 3.841f, thScore = 5.991f.  Per side `if (chi > th) inlier = false; else score += thScore - chi` (a NaN adds itself, as there).
 *   The score of a hypothesis: lane l of the wave adds the sides of the matches l, l + 64, ... in that order, then the 64 sums meet in a
 *     butterfly (steps 32 .. 1): a fixed order, so the same input gives the same bytes, and not the reference's running sum.
 *   The pick per family: the FIRST iteration whose score is the maximum (:116, :155 use a strict `>`); a score that is not above 0
 *     picks nothing.  RH = SH / (SH + SF), one float add and one float divide; H is chosen when RH > 0.5f.
 *
 * Outputs, every one written by a call that succeeds with d_result[1] != 1, none otherwise:
 *   d_pairs [n1][2] int32: match_pairs in ascending i, (i, m); the rows from n_matches on are (-1, -1).
 *   d_H, d_F [9] float row-major: the winning H21 and F21.  d_inl_H, d_inl_F [n1] uint8 per MATCH index (row of d_pairs): the two
 *   inlier masks, 0 from n_matches on.  d_score [2]: SH, SF.  d_rh [1]: RH (0 when SH + SF == 0).
 *   d_hyp [2][iters][9] float (may be NULL): every hypothesis after de-normalisation, H then F.  d_hyp_score [2][iters] float (may be
 *   NULL): every hypothesis's score.  Documented outputs: a caller may want to refine the runners-up.
 * d_result (int32 x 8, written): [0] n_matches; [1] status: 0 ok, 1 fewer than 8 matches (the reference would index an empty vector;
 *   ONLY d_result is written), 2 SH + SF == 0 (:73, the reference returns false); [2], [3] the winning iteration of H and of F, -1
 *   when no hypothesis scored above 0 (the matrix is then zeros and the mask all 0; the reference leaves them unset); [4] 1 when
 *   RH > 0.5f, i.e. H is chosen; [5], [6] the inlier counts of H and of F; [7] 0.
 * The draw's parity with OpenCV is UNPINNED: OpenCV is not available where this library is built and tested, so orbm_two_view_sets
 * restates cv::RNG from its published source (the multiply-with-carry state = (uint32) state * 4164903690 + (state >> 32), the draw
 * (uint32) state % size) and is held to a model that restates the same text; pass d_sets to use the draw of your own OpenCV.
 *
 * Shape (latency, not throughput: 2 * iters waves on 256 CUs).  Three launches on `stream`, no host wait: k_tv_prepare, ONE workgroup of
 * 1024 (the list by a block scan, walked twice so that fewer than 8 matches are found before a row is written; Normalize; the draw:
 * the 8 * iters raw values do not depend on n_matches, and the generator is state' = state * 4164903690 modulo 4164903690 * 2^32 - 1,
 * so one wave makes them, each lane 128 values from a state it jumps to by one modular product, and
 * a lane per iteration resolves its eight "take index randi, move the last into its place" steps on an eight-entry override list);
 * k_tv_hypotheses, ONE WAVE per hypothesis, four to a workgroup (the rows of the matrix on 16 lanes, the column dot products 16-wide
 * __shfl_xor butterflies; then all 64 lanes stride over the matches, the inlier bits one __ballot word per 64 matches in handle
 * scratch); k_tv_pick, ONE workgroup of 1024.  Handle scratch (grow-only, apart from the searches'): the sets, the hypotheses, their
 * scores and 2 * iters mask rows of ceil(n1 / 64) words; one call in flight per handle.  As compiled for gfx950 -- VGPRs / scratch /
 * static LDS: k_tv_prepare 81 / 0 / 33088 B, k_tv_hypotheses 222 / 0 / 0 B, k_tv_pick 40 / 0 / 264 B: no scratch memory; the two
 * one-workgroup kernels within 128 VGPRs (all a thread of sixteen waves can have), k_tv_hypotheses within 256 (its 18 doubles a lane and
 * three butterflies in flight; two waves per SIMD remain, which is what 2 * 1024 waves put on the 1024 SIMDs of the device).
 * Measured device time of one call at iters = 200 (profiles/two_view_latency.txt): 196 us at 300 matches, 211 us at 2000; 8 us less with d_sets given.
 * Refused with ORBX_E_ARG before any launch, every byte left as passed: iters outside 1 .. 1024, n1 or n2 < 1, sigma <= 0, a required
 * pointer NULL.  Behind those, also before any launch: n1 or n2 above ORBM_TWO_VIEW_MAX_KEYPOINTS is ORBX_E_UNSUPPORTED.  Without a HIP
 * device the call fails with ORBX_E_NO_DEVICE.  Enqueued on `stream` (NULL: orbx.h, "Streams"). */
#define ORBM_TWO_VIEW_MAX_ITERS 1024
#define ORBM_TWO_VIEW_MAX_KEYPOINTS 65536 /* n1, n2: the 2 * iters mask rows of n1 bits stay within 16 MB of handle scratch */
#define ORBM_TWO_VIEW_RNG_DEFAULT 0xffffffffull
int orbm_two_view_ransac_device(orbm_t *h, const void *d_kps1, int n1, const void *d_kps2, int n2, const int32_t *d_matches12, float sigma,
                                int iters, uint64_t rng_state, const int32_t *d_sets, int32_t *d_pairs, float *d_H, float *d_F,
                                uint8_t *d_inl_H, uint8_t *d_inl_F, float *d_score, float *d_rh, float *d_hyp, float *d_hyp_score,
                                int32_t *d_result, void *stream);
/* The same with host pointers throughout: synchronous on the handle's stream, one pinned copy each way, the same kernels and the
 * same bytes as the device entry point. */
int orbm_two_view_ransac(orbm_t *h, const void *kps1, int n1, const void *kps2, int n2, const int32_t *matches12, float sigma, int iters,
                         uint64_t rng_state, const int32_t *sets, int32_t *pairs, float *H, float *F, uint8_t *inl_H, uint8_t *inl_F,
                         float *score, float *rh, float *hyp, float *hyp_score, int32_t *result);
/* The draw of :42-58 on the host, no device needed: sets [iters][8] int32, eight distinct indices below n_matches each, the
 * generator running on from set to set (rng_state 0: ORBM_TWO_VIEW_RNG_DEFAULT).  ORBX_E_ARG: n_matches < 8, iters outside
 * 1 .. 1024, sets NULL. */
int orbm_two_view_sets(int n_matches, int iters, uint64_t rng_state, int32_t *sets);

/* ---- Two-view initialisation: the pose and the points ---------------------------------------------------------------------------------
 * The back half of TwoViewReconstruction::Reconstruct (modules/Frontend/TwoViewReconstruction.cpp): the dispatch (:79-83), ReconstructH
 * (:346-475), ReconstructF (:477-556), CheckRT (:598-687), Triangulate (:689-705), DecomposeE (:707-724), and the tail in which the
 * tracker consumes the result (Tracking.cpp:622-627).  It reads exactly what orbm_two_view_ransac_device writes, from device memory,
 * and goes directly behind it on the same stream.
 *
 * Inputs.  fx, fy, cx, cy: K.  d_kps1 [n1], d_kps2 [n2]: orbx_kp records, UNDISTORTED by the caller as for the RANSAC; only x and y are
 * read.  d_matches12 [n1].  d_pairs, d_H, d_F, d_inl_H, d_inl_F and d_ransac_result (int32 x 8): the RANSAC's outputs of those names
 * (its d_result).  family: -1 takes the RANSAC's choice from d_ransac_result[4] ON THE DEVICE (1: H), 0 forces F, 1 forces H -- for a
 * caller who wants the runner-up.  d_ransac_result[1] != 0 (the RANSAC refused) is found on the device too: the call then writes
 * d_result and nothing else.  d_ransac_result[0] is kept inside 0 .. n1, and a row of d_pairs outside [0, n1) x [0, n2) is skipped.
 * sigma: the reference's 1.f; th2 = 4.f * sigma * sigma (:451, :505).  min_parallax: the reference's 1.f (degrees).
 *
 * Two places where the reference cannot be followed literally.
 *   ReconstructH's hypothesis vectors.  It constructs vR(8), vt(8), vn(8) and then push_backs the eight computed hypotheses BEHIND them,
 *     so its loop at :447 checks eight default-constructed, uninitialised matrices.  The library checks the eight computed hypotheses
 *     in the order they are computed: d' = d2 for i = 0..3 (rows 0..3), then d' = -d2 for i = 0..3 (rows 4..7) -- the evident intent, and
 *     upstream ORB-SLAM's.  vn is never read and is not built.
 *   Triangulate returning false.  It returns false on Ph(3) == 0 and leaves Pc1 unset, which CheckRT then reads.  Here the division
 *     produces a non-finite point and the isfinite gate of :636 drops the match.
 *
 * Arithmetic.
 *   The decomposition runs in DOUBLE on the float H21 / F21 and the float K and is rounded to float once per hypothesis (R, and t over
 *     its norm), as the RANSAC's solve does and for its reason (a fixed-sweep float Jacobi leaves several times the float SVD's error):
 *     E = (K^T * F21) * K; A = (K^-1 * H21) * K with K^-1 = [1 / fx, 0, -cx / fx; 0, 1 / fy, -cy / fy; 0, 0, 1]; the 3 x 3 SVD by a
 *     one-sided Jacobi (8 sweeps; the columns of B = A * V over their norms are U, sorted by descending norm).  DecomposeE needs the
 *     column of U of the zero singular value, which B does not hold: U.col(2) = u0 x u1; R1 = U * W * V^T, R2 = U * W^T * V^T, each
 *     negated when its determinant is negative (:720-723); t = U.col(2).  H: s = det(U) * det(V^T), the degeneracy test
 *     d1 / d2 < 1.00001 || d2 / d3 < 1.00001 on the double singular values, and the formulas of :376-436 as written.
 *   The ORDER of the hypotheses is the library's own.  An SVD is unique only up to joint sign flips of (u_i, v_i), and up to independent
 *     signs on the null pair of E; these flips permute {R1, R2} x {t, -t} and the eight of H.  The order here is fixed by this Jacobi
 *     and deterministic -- the same input gives the same bytes -- but another SVD lists the same SET in another order.  The set of
 *     hypotheses and the decision are what the reference determines; compare hypotheses by nearest (R, t), never by index.  F's rows
 *     are (R1, t), (R2, t), (R1, -t), (R2, -t) of this library's R1, R2, t.
 *   CheckRT runs in float, no fused multiply-add, `/` and sqrt correctly rounded, in the reference's statement order; a row times a
 *     column reads ((p0 + p1) + p2) + p3.  P1 = K [I | 0], P2 = K * [R | t] in pixel units, O2 = -R^T * t.  Triangulate's 4 x 4 right
 *     singular vector is orbm_triangulate_matches_device's solve (a one-sided Jacobi, six sweeps, shared source).  n1.normalize() divides
 *     by sqrt(n1 . n1) where that is above 0.  cosParallax is compared with 0.99998 in double; proj_u1 = (fx * Pc1(0)) * invZ1 + cx.
 *   The parallax is (acosf(c) * 180.f) / M_PIf32 with c the element of rank min(50, nGood - 1) of the good cosines in ascending order:
 *     an exact order statistic (a radix select over the order-preserving integer image of the floats), not a sort; acosf is the
 *     device's.
 *   The decision is orbm_two_view_decide's, below.
 *
 * Outputs.  Every one is written by a call that gets as far as the hypotheses (d_result[0] != 1):
 *   d_R21 [9], d_t21 [3] float, row-major: the winning hypothesis; zeros when not accepted.
 *   d_points3D [n1][3] float, per key point of frame 1: Pc1 of the winning hypothesis where CheckRT stored it (:672: every good match,
 *     those with cosParallax >= 0.99998 too), zeros elsewhere and when not accepted.
 *   d_triangulated [n1] uint8: the winner's vbGood; zeros when not accepted.
 *   d_matches12_out [n1] int32 (Tracking.cpp:622-627): d_matches12 with every entry >= 0 that is not triangulated set to -1 when
 *     accepted; d_matches12 unchanged when not.  The next stage reads its input from the device.
 *   d_hyp_R [8][9], d_hyp_t [8][3] float, d_hyp_good [8] int32, d_hyp_parallax [8] float: every hypothesis, its nGood and its parallax
 *     (degrees).  F fills the first four rows and zeros the rest; a degenerate H zeros all eight.
 *   d_hyp_code [8][n1] uint8, may be NULL: where each key point of frame 1 left CheckRT under each hypothesis.  0 no match, 1 matched
 *     but not an inlier of the family used (:628), 2 not finite (:636), 3 behind camera 1 (:649), 4 behind camera 2 (:653), 5 error in
 *     image 1 (:661), 6 error in image 2 (:669), 7 good (nGood and vbGood), 8 good without parallax (nGood and the point, vbGood false).
 *     The rows of hypotheses that do not exist are zeros.
 *   d_result, int32 x 16: [0] status: 0 accepted, 1 the RANSAC refused (ONLY d_result is written; [1] the family, [3] -1, the rest 0),
 *     2 H degenerate (:370), 3 no clear winner or too few good, 4 parallax too low (the other conditions hold); [1] the family used
 *     (0 F, 1 H); [2] the number of hypotheses (4, 8, or 0 when degenerate); [3] the winner's row, -1 unless accepted; [4] nInlier;
 *     [5] minGood; [6] the number triangulated (0 unless accepted); [7] matches left: the entries of d_matches12_out in [0, n2);
 *     [8..15] a copy of d_hyp_good.
 *
 * Shape (latency: at most 8 hypotheses and a few thousand matches, 65536 at the cap).  Three launches on `stream`, no host wait, no
 * allocation in steady state: k_tvp_decompose, one lane (the 3 x 3 Jacobi and the hypotheses in constant-indexed registers);
 * k_tvp_check, ONE workgroup of 1024 per hypothesis, threads striding over the match list, nGood and nInlier by wave popcounts added in
 * LDS, the select four 8-bit digits with a 256-bin histogram in LDS each, the keys in handle scratch; k_tvp_decide, ONE workgroup of
 * 1024: the decision, then the winner walked AGAIN for d_points3D / d_triangulated (the same arithmetic on the same inputs, so the same
 * gates bit for bit, as orbm_triangulate_matches_device's second walk), then d_matches12_out.  Handle scratch (grow-only, a block of its
 * own): 32 bytes and 8 rows of n1 keys; one call in flight per handle.  As compiled for gfx950 -- VGPRs / scratch / static LDS:
 * k_tvp_decompose 168 / 0 / 0 B, k_tvp_check 86 / 0 / 1104 B, k_tvp_decide 90 / 0 / 8 B: no scratch memory; the two workgroups of sixteen
 * waves within the 128 VGPRs a thread of theirs can have, the single wave of k_tvp_decompose within 256.
 * Measured device time of one call (profiles/two_view_latency.txt): 56 us at 250 matches (229 inliers), 133 us at 1647 (1553 inliers);
 * the search, the RANSAC and this call on one stream 271 and 734 us.  The float32 numpy model of this half takes 2 and 12 ms on the host
 * behind a wait and a read-back: an order of magnitude only, numpy is not the reference's C++.
 * Refused with ORBX_E_ARG before any launch, every byte left as passed: a required pointer NULL (all but d_hyp_code), n1 or n2 < 1,
 * sigma <= 0, fx or fy not finite or not positive, family outside -1 .. 1.  Behind those, also before any launch: n1 or n2 above
 * ORBM_TWO_VIEW_MAX_KEYPOINTS is ORBX_E_UNSUPPORTED.  Without a HIP device the call fails with ORBX_E_NO_DEVICE.  Enqueued on `stream`
 * (NULL: orbx.h, "Streams"). */
int orbm_two_view_pose_device(orbm_t *h, float fx, float fy, float cx, float cy, const void *d_kps1, int n1, const void *d_kps2, int n2,
                              const int32_t *d_matches12, const int32_t *d_pairs, const float *d_H, const float *d_F, const uint8_t *d_inl_H,
                              const uint8_t *d_inl_F, const int32_t *d_ransac_result, int family, float sigma, float min_parallax,
                              float *d_R21, float *d_t21, float *d_points3D, uint8_t *d_triangulated, int32_t *d_matches12_out,
                              float *d_hyp_R, float *d_hyp_t, int32_t *d_hyp_good, float *d_hyp_parallax, uint8_t *d_hyp_code,
                              int32_t *d_result, void *stream);
/* The same with host pointers throughout: synchronous on the handle's stream, one pinned copy each way, the same kernels and the
 * same bytes as the device entry point. */
int orbm_two_view_pose(orbm_t *h, float fx, float fy, float cx, float cy, const void *kps1, int n1, const void *kps2, int n2,
                       const int32_t *matches12, const int32_t *pairs, const float *H, const float *F, const uint8_t *inl_H,
                       const uint8_t *inl_F, const int32_t *ransac_result, int family, float sigma, float min_parallax, float *R21,
                       float *t21, float *points3D, uint8_t *triangulated, int32_t *matches12_out, float *hyp_R, float *hyp_t,
                       int32_t *hyp_good, float *hyp_parallax, uint8_t *hyp_code, int32_t *result);
/* The decision of ReconstructF (family 0: n_good and parallax hold four entries) or ReconstructH (family 1: eight) on the host, no
 * device needed: the same code the device runs.  winner: the accepted hypothesis or -1; min_good; reason: 0 accepted, 3 no clear winner
 * or too few good, 4 parallax too low (and the other conditions hold).  The reference's spellings are kept:
 *   H: minGood = min(cvRound(0.6 * nInlier), 100), to nearest with ties to even, in double; bestGood / secondBestGood tracked as the
 *     loop of :447-464 does, the FIRST maximum winning; accepted when secondBestGood < 0.75 * bestGood && bestParallax >= minParallax &&
 *     bestGood > minGood.
 *   F: minGood = min(cvFloor(0.6 * nInlier), 100); goodTh = cvFloor(0.7 * maxGood); maxGood < minGood || nSimilar > 1 rejects; the
 *     cascade of :524-552, so the first hypothesis that reaches the maximum is the one asked; its parallax test is a strict `>`.
 * ORBX_E_ARG: a pointer NULL, family not 0 or 1, n_inlier < 0. */
int orbm_two_view_decide(int family, const int32_t *n_good, const float *parallax, int n_inlier, float min_parallax, int32_t *winner,
                         int32_t *min_good, int32_t *reason);

/* MapPoint::computeDescriptor (modules/BasicObject/MapPoint.cpp:103-152) for n_groups map points at once.
 * Group g = the descriptors desc[off[g] .. off[g+1]) of one point's observations (the caller skips bad key frames,
 * :115-120).  best_idx[g] = index inside the group of the descriptor with the least median Hamming distance to the
 * group (median = sorted row[(N-1)/2], self distance 0 included; first index on ties, :138-146); -1 for an empty
 * group (the reference returns without touching the descriptor, :122).  At most 1024 observations per point. */
int orbm_distinctive_descriptors(orbm_t *h, const uint8_t *desc, const int32_t *off, int n_groups, int32_t *best_idx);
int orbm_distinctive_descriptors_device(orbm_t *h, const uint8_t *d_desc, const int32_t *d_off, int n_groups,
                                        int32_t *d_best_idx, void *stream);

/* ORBMatcher::ComputeThreeMaxima (modules/ORB/ORBMatcher.cpp:594-622) on bin sizes */
void orbm_three_maxima(const int32_t *hist_sizes, int n_bins, int *ind1, int *ind2, int *ind3);

#ifdef __cplusplus
}
#endif
#endif
