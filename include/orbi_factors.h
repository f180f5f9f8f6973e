/*
 * orbi_factors.h -- the declarations of orbi.h's section "Inertial factors linearised on the device".  Include orbi.h, which ends by
 * including this file; the section's text (the graph, the arithmetic, the evaluation orders, the kernels' resources) is there.
 */
#ifndef ORBI_FACTORS_H
#define ORBI_FACTORS_H

#ifndef ORBI_H
#error "include orbi.h, not orbi_factors.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* d_fixed[s]: setFixed per vertex of state s, also "this state has no such vertex" */
#define ORBI_FIX_POSE 1
#define ORBI_FIX_VELO 2
#define ORBI_FIX_GYRO 4
#define ORBI_FIX_ACC 8
/* orbi_edge.flags */
#define ORBI_EDGE_WALKS 1          /* the edge carries the gyro and the acc EdgeBiasWalk between the bias vertices of i and j */
/* orbi_prior_job.mask */
#define ORBI_PRIOR_VELO 1
#define ORBI_PRIOR_GYRO 2
#define ORBI_PRIOR_ACC 4
#define ORBI_PRIOR_ACC_GYRO_INFO 8 /* with ORBI_PRIOR_ACC: the acc prior is weighted with gyro_info (Optimize.cpp:1189) */
/* a job of orbi_graph_recover_device: flags */
#define ORBI_RECOVER_POSE 1
/* d_result of orbi_linearize_device beyond ORBI_R_DONE / _RANGE / _REFUSED, which count edges there */
#define ORBI_R_PRIOR_DONE 4        /* prior jobs applied */
#define ORBI_R_PRIOR_RANGE 5       /* prior jobs dropped: state or prior slot outside its range */
#define ORBI_EDGE_WORK 488         /* doubles of workspace per edge (orbi_linearize_device) */
#define ORBI_JACOBI_SWEEPS 6       /* cyclic Jacobi sweeps of orbi_prior_information_device */

typedef struct orbi_edge {         /* one EdgeInertial / EdgeInertialOnly, with or without its two EdgeBiasWalk */
    int32_t i, j;                  /* first and second state */
    int32_t rec;                   /* the record of the bank: the PreIntegrator between them */
    int32_t flags;
} orbi_edge;

typedef struct orbi_prior {        /* what a KeyFrame keeps for its three EdgePriori3D, floats as it holds them; matrices row-major */
    float velo_priori[3], bias_priori[6];
    float velo_info[9], gyro_info[9], acc_info[9];
} orbi_prior;

typedef struct orbi_prior_job {
    int32_t state, prior, mask;
} orbi_prior_job;

typedef struct orbi_graph {        /* by value: the vertices, all in device memory */
    double *Rwb, *twb, *v, *bg, *ba;   /* [n_states][9], [n_states][3] x 4 */
    uint8_t *fixed;                    /* [n_states] */
    int32_t n_states, pad;
} orbi_graph;

/* KeyFrame::setPrioriInformation (KeyFrame.cpp:86-98) and the priors of the constructor (:23-24) for n jobs d_jobs[3k .. 3k+3) =
 * (prior slot, source record, source state): velo_info, gyro_info, acc_info from the record's C; bias_priori = the record's
 * updated_bias; velo_priori = d_src[15*state + 12 ..) -- a source state of -1 (always, when d_src == NULL) leaves velo_priori as it is.
 * A slot, record or source state outside its range: dropped (ORBI_R_RANGE).  A job naming the slot of an earlier job of the list,
 * dropped or not: dropped (ORBI_R_DUPLICATE).  C[9:12,9:12] or C[12:15,12:15] with determinant 0: refused, the slot stays untouched (ORBI_R_REFUSED). */
int orbi_prior_information_device(orbi_prior *d_priors, int n_priors, const orbi_record *d_bank, int cap, const float *d_src, int n_src,
                                  const int32_t *d_jobs, int n, int32_t *d_result, void *stream);

/* The vertices from device state (Optimize.cpp:557-573, :623-651, :992-1007) for n jobs d_jobs[3k .. 3k+3) = (state, source state,
 * record): Rwb, twb, v = the 15 floats d_src[15*source ..) widened; bg, ba = the record's updated_bias widened, or zero with record -1
 * (a state without bias vertices).  d_fixed is the caller's and is not read.  Out of range: ORBI_R_RANGE; a state an earlier job
 * names, dropped or not: ORBI_R_DUPLICATE. */
int orbi_graph_init_device(orbi_graph graph, const orbi_record *d_bank, int cap, const float *d_src, int n_src, const int32_t *d_jobs, int n,
                           int32_t *d_result, void *stream);

/* Once per optimisation: d_info[81e ..) and d_walk_info[18e ..) (gyro, then acc) of edge e from record d_edges[e].rec.  Only `rec` and
 * `flags` of an edge are read.  rec outside [0, cap): blocks zeroed, ORBI_R_RANGE.  A zero pivot in C[0:9,0:9], or, on an edge with
 * ORBI_EDGE_WALKS, a walk block with determinant 0: all of the edge's blocks zeroed, ORBI_R_REFUSED.  (Without the flag a walk block
 * with determinant 0 is zeroed and nothing is counted.) */
int orbi_edge_information_device(const orbi_record *d_bank, int cap, const orbi_edge *d_edges, int n_edges, double *d_info, double *d_walk_info,
                                 int32_t *d_result, void *stream);

/* computeError, linearizeOplus and constructQuadraticForm of every edge and prior.  gravity: GRAVITY_VALUE.  huber_delta > 0: the
 * Huber kernel on the inertial edges.  mode 0: everything; mode 1: computeError only -- d_H_diag, d_H_off, d_b and d_J are neither
 * read nor written and may be NULL.  d_work: n_edges x ORBI_EDGE_WORK doubles of scratch, the caller's, both modes.  d_J (mode 0) and
 * d_float (both modes; [n_edges][15]: the float dR, dV, dP of the edge's bias vertices) may be NULL.  Outputs of a dropped or skipped
 * edge or prior job are zero.  Two launches. */
int orbi_linearize_device(orbi_graph graph, const orbi_record *d_bank, int cap, float gravity, const orbi_edge *d_edges, int n_edges,
                          const double *d_info, const double *d_walk_info, const orbi_prior *d_priors, int n_priors,
                          const orbi_prior_job *d_prior_jobs, int n_prior_jobs, double huber_delta, int mode, double *d_work, double *d_err,
                          double *d_chi2, double *d_chi2_prior, double *d_total, double *d_H_diag, double *d_H_off, double *d_b, double *d_J,
                          float *d_float, int32_t *d_result, void *stream);

/* oplusImpl of every vertex that is not fixed with d_dx[15s ..).  d_iter[s]: CameraImuPose's update counter, the caller's (zero at
 * the start of an optimisation).  d_result[ORBI_R_DONE]: the states with at least one vertex moved. */
int orbi_graph_oplus_device(orbi_graph graph, const double *d_dx, int32_t *d_iter, int32_t *d_result, void *stream);

/* Step 5 of the optimisers (Optimize.cpp:602-607, :1044-1053) for n jobs d_jobs[3k .. 3k+3) = (state, destination, flags): the
 * state's v rounded to float into d_dst[15*destination + 12 ..); (bg, ba) rounded to float into d_bias[6k ..), the array
 * orbi_set_bias_device takes.  With ORBI_RECOVER_POSE also (Rwb, twb) rounded to float into d_dst[15*destination ..) and, when
 * d_pose_R / d_pose_t (they go together) are given, T_cw = T_cb * T_wb.inverse() of those floats into d_pose_R[9k ..), d_pose_t[3k ..)
 * as doubles holding floats.  Out of range: ORBI_R_RANGE, its d_bias row zeroed; a destination an earlier job names, dropped or not:
 * ORBI_R_DUPLICATE, likewise. */
int orbi_graph_recover_device(orbi_graph graph, orbi_calib calib, const int32_t *d_jobs, int n, float *d_dst, int n_dst, float *d_bias,
                              double *d_pose_R, double *d_pose_t, int32_t *d_result, void *stream);

#ifdef __cplusplus
}
#endif
#endif
