"""Array model of the inertial chain assembled on the device-resident map (include/orbm.h, "The inertial chain on the device-resident
map"): orbm_inertial_chain_problem_device and orbm_inertial_chain_velocity_priors_device restated in numpy, integers and float copies
only, and a chain scene of tests/inertial_chain.py laid out as the map side such a caller holds (by the method of
inertial_window_model.map_from_window_scene).  TEST CODE ONLY."""
import numpy as np

import factors_model as fm

C_STATES, C_REFUSED, C_WINDOW_UNUSABLE, C_IMU_RANGE = 0, 1, 2, 3
REFUSE_WINDOW, REFUSE_IMU = 8, 32
MAX_WINDOW = 20
OUT = ("init_jobs", "fixed", "inertial_edges", "recover_jobs", "bias_ids", "velo_jobs", "state_kf")
WIDTH = dict(init_jobs=3, inertial_edges=4, recover_jobs=3, velo_jobs=2)


def problem(bad, window, kf_imu, n_src, cap_bank, n_priors):
    """-> dict of the seven lists and result i32 [8].  State s is window[s]; an entry out of range, bad or named by an earlier entry, or a
    d_kf_imu index of a usable entry out of range, refuses the call: -1 everywhere, fixed all 15"""
    n, n_kf = len(window), len(bad)
    unusable = imu_range = 0
    rows = []
    for s, k in enumerate(int(x) for x in window):
        usable = 0 <= k < n_kf and bad[k] == 0 and k not in [int(x) for x in window[:s]]
        unusable += not usable
        if usable:
            row, rec, prior = (int(v) for v in kf_imu[k])
            imu_range += row < 0 or row >= n_src or rec < 0 or rec >= cap_bank or prior < 0 or prior >= n_priors
            rows.append((k, row, rec, prior))
    refused = (unusable != 0) * REFUSE_WINDOW | (imu_range != 0) * REFUSE_IMU
    result = np.array([n, refused, unusable, imu_range, 0, 0, 0, 0], np.int32)
    if refused:
        o = dict(init_jobs=np.full((n, 3), -1, np.int32), fixed=np.full(n, 15, np.uint8), inertial_edges=np.full((n - 1, 4), -1, np.int32),
                 recover_jobs=np.full((n, 3), -1, np.int32), bias_ids=np.full(n, -1, np.int32), velo_jobs=np.full((n, 2), -1, np.int32),
                 state_kf=np.full(n, -1, np.int32))
        return dict(o, result=result)
    o = dict(init_jobs=np.array([(s, row, rec) for s, (_, row, rec, _) in enumerate(rows)], np.int32),
             fixed=np.array([15] + [fm.FIX_POSE] * (n - 1), np.uint8),
             inertial_edges=np.array([(s, s + 1, rows[s][2], fm.EDGE_WALKS) for s in range(n - 1)], np.int32).reshape(n - 1, 4),
             recover_jobs=np.array([(s, row, 0) for s, (_, row, _, _) in enumerate(rows)], np.int32),
             bias_ids=np.array([r[2] for r in rows], np.int32), velo_jobs=np.array([(r[1], r[3]) for r in rows], np.int32),
             state_kf=np.array([r[0] for r in rows], np.int32))
    return dict(o, result=result)


def velocity_priors(priors, src, velo_jobs):
    """priors f32 [n_priors, 36] (orbi_prior), src f32 [n_src, 15], velo_jobs i32 [n, 2] -> (priors after, result i32 [8])"""
    out, res = priors.copy(), np.zeros(8, np.int32)
    for row, slot in np.asarray(velo_jobs).reshape(-1, 2):
        ok = 0 <= row < len(src) and 0 <= slot < len(out)
        res[0 if ok else 1] += 1
        if ok:
            out[slot, :3] = src[row, 12:15]
    return out, res


def map_from_chain_scene(sc, seed=3):
    """a chain scene laid out as what the assembly reads: key frames in shuffled slots with two more, one of them bad, state rows and prior
    slots behind d_kf_imu in shuffled order (record s stays the bank's entry s: the bank is the scene's), random priors"""
    rng = np.random.RandomState(seed)
    n = sc["graph"].n
    n_kf, n_src, n_priors = n + 2, n + 1, n + 2
    order = [int(k) for k in rng.permutation(n_kf)]
    window, spare, bad_kf = order[:n], order[n], order[n + 1]
    row_of_state, prior_of_state = rng.permutation(n_src)[:n], rng.permutation(n_priors)[:n]
    src = rng.uniform(-1, 1, (n_src, 15)).astype(np.float32)
    src[row_of_state] = sc["src"]
    kf_imu = np.full((n_kf, 3), -1, np.int32)
    for s in range(n):
        kf_imu[window[s]] = (row_of_state[s], s, prior_of_state[s])
    kf_imu[spare] = kf_imu[bad_kf] = (n_src - 1, 0, n_priors - 1)
    bad = np.zeros(n_kf, np.uint8)
    bad[bad_kf] = 1
    priors = rng.uniform(-1, 1, (n_priors, 36)).astype(np.float32)
    return dict(n_kf=n_kf, bad=bad, window=np.array(window, np.int32), kf_imu=kf_imu, n_src=n_src, cap_bank=len(sc["recs"]), n_priors=n_priors, src=src,
                priors=priors, spare=spare, bad_kf=bad_kf)
