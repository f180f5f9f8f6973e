"""numpy restatement of the front half of TwoViewReconstruction::Reconstruct (reference modules/Frontend/TwoViewReconstruction.cpp):
:14-84 without the Reconstruct calls (the match list, the draw of the eight-point sets, RH), :86-344 (FindHomography, FindFundamental,
ComputeH21, ComputeF21, CheckHomography, CheckFundamental) and :558-596 (Normalize), statement by statement, in the dtype given:
float64 is the yardstick of tests/test_two_view_gpu.py, float32 (LAPACK's SVD where the reference runs Eigen's JacobiSVD) the ruler
its margins are taken from.  Also the seeded two-view scenes of both test files."""
import numpy as np

TH_H = 5.991                   # CheckHomography's th
TH_F, TH_SCORE = 3.841, 5.991  # CheckFundamental's th, thScore
RNG_COEFF = 4164903690         # cv::RNG's multiplier
RNG_DEFAULT = 0xFFFFFFFF       # cv::RNG's default state


# ---- :23-58 ------------------------------------------------------------------------------------------------------------------------
def match_pairs(matches12, n2):
    """:26-30 -- (i, matches12[i]) in ascending i; an entry outside [0, n2) is "no match", as the library reads it"""
    m = np.asarray(matches12)
    i = np.flatnonzero((m >= 0) & (m < n2))
    return np.stack([i, m[i]], axis=1).astype(np.int32).reshape(-1, 2)


def rng_next(state):
    """cv::RNG::next(): multiply with carry; returns (new state, the 32-bit draw)"""
    state = ((state & 0xFFFFFFFF) * RNG_COEFF + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
    return state, state & 0xFFFFFFFF


def draw_sets(n_matches, iters, state=RNG_DEFAULT):
    """:42-58 with the availableIndices vector itself: take index randi, move the last into its place, pop"""
    state = int(state) or RNG_DEFAULT
    sets = np.zeros((iters, 8), np.int32)
    for it in range(iters):
        avail = list(range(n_matches))
        for j in range(8):
            state, r = rng_next(state)
            randi = r % len(avail)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


# ---- :558-596 ----------------------------------------------------------------------------------------------------------------------
def normalize(xy, dt):
    """Normalize over ALL key points of a frame, sums in the sequential order of the reference"""
    xy = np.asarray(xy, dt)
    n = dt(len(xy))
    if dt == np.float32:       # the running float sum, element by element (cumsum adds in order)
        mean = np.array([np.cumsum(xy[:, 0], dtype=dt)[-1], np.cumsum(xy[:, 1], dtype=dt)[-1]], dt) / n
    else:
        mean = xy.sum(axis=0) / n
    p = xy - mean
    if dt == np.float32:
        dev = np.array([np.cumsum(np.abs(p[:, 0]), dtype=dt)[-1], np.cumsum(np.abs(p[:, 1]), dtype=dt)[-1]], dt) / n
    else:
        dev = np.abs(p).sum(axis=0) / n
    s = dt(1) / dev
    T = np.eye(3, dtype=dt)
    T[0, 0], T[1, 1] = s[0], s[1]
    T[0, 2], T[1, 2] = -mean[0] * s[0], -mean[1] * s[1]
    return (p * s).astype(dt), T


# ---- :163-224 ----------------------------------------------------------------------------------------------------------------------
def h_matrix(p1, p2, dt):
    """the 16 x 9 matrix of ComputeH21"""
    A = np.zeros((16, 9), dt)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A[0::2, 3], A[0::2, 4], A[0::2, 5] = -u1, -v1, -1
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = v2 * u1, v2 * v1, v2
    A[1::2, 0], A[1::2, 1], A[1::2, 2] = u1, v1, 1
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = -u2 * u1, -u2 * v1, -u2
    return A


def f_matrix(p1, p2, dt):
    """the 8 x 9 matrix of ComputeF21"""
    A = np.ones((8, 9), dt)
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    A[:, 0], A[:, 1], A[:, 2] = u2 * u1, u2 * v1, u2
    A[:, 3], A[:, 4], A[:, 5] = v2 * u1, v2 * v1, v2
    A[:, 6], A[:, 7] = u1, v1
    return A


def compute_h21(p1, p2, dt):
    A = h_matrix(p1, p2, dt)
    _, w, vt = np.linalg.svd(A, full_matrices=True)
    return vt[8].reshape(3, 3).astype(dt), w


def compute_f21(p1, p2, dt):
    A = f_matrix(p1, p2, dt)
    _, w, vt = np.linalg.svd(A, full_matrices=True)
    pre = vt[8].reshape(3, 3).astype(dt)
    u, w3, vt3 = np.linalg.svd(pre)
    w3 = w3.copy()
    w3[2] = 0
    return ((u * w3) @ vt3).astype(dt), w


# ---- :226-344 ----------------------------------------------------------------------------------------------------------------------
def check_homography(H21, xy1, xy2, sigma, dt):
    """returns (score, inlier flags, chiSquare1, chiSquare2) over the matched points xy1[k] <-> xy2[k]"""
    H21 = np.asarray(H21, dt)
    H12 = np.linalg.inv(H21).astype(dt)
    inv_sigma2 = dt(1) / (dt(sigma) * dt(sigma))
    th = dt(np.float32(TH_H))
    u1, v1, u2, v2 = (np.asarray(a, dt) for a in (xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]))
    with np.errstate(all="ignore"):
        w = dt(1) / (H12[2, 0] * u2 + H12[2, 1] * v2 + H12[2, 2])
        a = (H12[0, 0] * u2 + H12[0, 1] * v2 + H12[0, 2]) * w
        b = (H12[1, 0] * u2 + H12[1, 1] * v2 + H12[1, 2]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_sigma2
        w = dt(1) / (H21[2, 0] * u1 + H21[2, 1] * v1 + H21[2, 2])
        a = (H21[0, 0] * u1 + H21[0, 1] * v1 + H21[0, 2]) * w
        b = (H21[1, 0] * u1 + H21[1, 1] * v1 + H21[1, 2]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_sigma2
    return _score(chi1, chi2, th, th, dt)


def check_fundamental(F21, xy1, xy2, sigma, dt):
    F = np.asarray(F21, dt)
    inv_sigma2 = dt(1) / (dt(sigma) * dt(sigma))
    u1, v1, u2, v2 = (np.asarray(a, dt) for a in (xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]))
    with np.errstate(all="ignore"):
        a2 = F[0, 0] * u1 + F[0, 1] * v1 + F[0, 2]
        b2 = F[1, 0] * u1 + F[1, 1] * v1 + F[1, 2]
        c2 = F[2, 0] * u1 + F[2, 1] * v1 + F[2, 2]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv_sigma2
        a1 = F[0, 0] * u2 + F[1, 0] * v2 + F[2, 0]
        b1 = F[0, 1] * u2 + F[1, 1] * v2 + F[2, 1]
        c1 = F[0, 2] * u2 + F[1, 2] * v2 + F[2, 2]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv_sigma2
    return _score(chi1, chi2, dt(np.float32(TH_F)), dt(np.float32(TH_SCORE)), dt)


def _score(chi1, chi2, th, th_score, dt):
    """`if (chi > th) inlier = false; else score += thScore - chi` per side, the score summed in match order"""
    out1, out2 = chi1 > th, chi2 > th
    terms = np.stack([np.where(out1, dt(0), th_score - chi1), np.where(out2, dt(0), th_score - chi2)], axis=1).reshape(-1)
    score = np.cumsum(terms, dtype=dt)[-1] if dt == np.float32 and len(terms) else terms.sum(dtype=dt)
    return dt(score), ~(out1 | out2), chi1, chi2


# ---- :86-161 and :60-84 ------------------------------------------------------------------------------------------------------------
def run_model(kps1_xy, kps2_xy, matches12, sigma, iters, sets=None, state=RNG_DEFAULT, dt=np.float64):
    """FindHomography + FindFundamental + RH.  Returns a dict: pairs, sets, T1, T2, hyp [2][iters][3][3], hyp_score [2][iters],
    cond [2][iters] (the gates of test (a): (s8 - s9) / s1 of the 16 x 9 matrix, s8 / s1 of the 8 x 9 one), win [2] (-1: no score
    above 0), H, F, inl [2][n_matches], score [2], rh, status."""
    xy1, xy2 = np.asarray(kps1_xy, np.float32), np.asarray(kps2_xy, np.float32)
    pairs = match_pairs(matches12, len(xy2))
    n = len(pairs)
    out = dict(pairs=pairs, n_matches=n, status=0)
    if n < 8:
        out["status"] = 1
        return out
    sets = draw_sets(n, iters, state) if sets is None else np.asarray(sets)
    p1, T1 = normalize(xy1, dt)
    p2, T2 = normalize(xy2, dt)
    m1, m2 = xy1[pairs[:, 0]].astype(dt), xy2[pairs[:, 1]].astype(dt)
    hyp, score, cond = np.zeros((2, iters, 3, 3), dt), np.zeros((2, iters), dt), np.zeros((2, iters))
    best = [dt(0), dt(0)]
    win = [-1, -1]
    inl = np.zeros((2, n), bool)
    mats = np.zeros((2, 3, 3), dt)
    T2inv = np.linalg.inv(T2).astype(dt)
    for it in range(iters):
        s1, s2 = p1[pairs[sets[it], 0]], p2[pairs[sets[it], 1]]
        Hn, w = compute_h21(s1, s2, dt)
        cond[0, it] = (w[7] - w[8]) / w[0]
        Fn, w = compute_f21(s1, s2, dt)
        cond[1, it] = w[7] / w[0]
        hyp[0, it] = T2inv @ Hn @ T1
        hyp[1, it] = T2.T @ Fn @ T1
        for fam, check in ((0, check_homography), (1, check_fundamental)):
            sc, flags, _, _ = check(hyp[fam, it], m1, m2, sigma, dt)
            score[fam, it] = sc
            if sc > best[fam]:                                  # :116, :155 -- strict
                best[fam], win[fam], inl[fam], mats[fam] = sc, it, flags, hyp[fam, it]
    sh, sf = best
    out.update(sets=sets, T1=T1, T2=T2, hyp=hyp, hyp_score=score, cond=cond, win=win, H=mats[0], F=mats[1], inl=inl,
               score=np.array(best, dt))
    if sh + sf == 0:
        out["status"] = 2
        out["rh"] = dt(0)
    else:
        out["rh"] = sh / (sh + sf)
    return out


def unit_sine(a, b):
    """the sine of the angle between two 3 x 3 matrices as 9-vectors, sign free"""
    a, b = np.asarray(a, np.float64).reshape(-1, 9), np.asarray(b, np.float64).reshape(-1, 9)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    c = np.abs((a * b).sum(axis=1))
    # 1 - c^2 loses everything below 1e-8: the sine is the norm of the difference of the aligned unit vectors, to first order
    sgn = np.sign((a * b).sum(axis=1))[:, None]
    d = np.linalg.norm(a - sgn * b, axis=1)
    return d * np.sqrt(np.maximum(1 - d * d / 4, 0))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
W, H, FX, FY, CX, CY = 752, 480, 460.0, 460.0, 376.0, 240.0


def make_scene(n_matches, seed, planar=False, noise=0.5, wrong=0.2, extra1=37, extra2=11):
    """Two views of a seeded cloud through a 752 x 480 pinhole: depths 3..9 ("general") or a tilted plane ("planar"), `noise` px of
    Gaussian noise, `wrong` of the pairings shuffled among themselves, n1 != n2 (unmatched key points in both frames, spread among
    the matched ones) and -1 holes in matches12.  Returns dict(xy1 [n1][2] f32, xy2 [n2][2] f32, matches12 [n1] i32)."""
    r = np.random.RandomState(seed)
    n = n_matches
    u = r.uniform(30, W - 30, n)
    v = r.uniform(30, H - 30, n)
    if planar:
        z = 6.0 + 0.004 * (u - CX) + 0.003 * (v - CY)
    else:
        z = r.uniform(3, 9, n)
    P = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], axis=1)
    ang = np.array([0.02, -0.05, 0.015])
    th = np.linalg.norm(ang)
    k = ang / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    t = np.array([0.45, 0.05, 0.08])
    Q = P @ R.T + t
    a = np.stack([u, v], axis=1) + r.normal(0, noise, (n, 2))
    b = np.stack([Q[:, 0] / Q[:, 2] * FX + CX, Q[:, 1] / Q[:, 2] * FY + CY], axis=1) + r.normal(0, noise, (n, 2))
    n_wrong = int(round(wrong * n))
    if n_wrong > 1:
        idx = r.choice(n, n_wrong, replace=False)
        b[idx] = b[np.roll(idx, 1)]
    # unmatched key points in both frames, then both frames shuffled
    n1, n2 = n + extra1, n + extra2
    xy1 = np.concatenate([a, np.stack([r.uniform(0, W, extra1), r.uniform(0, H, extra1)], axis=1)])
    xy2 = np.concatenate([b, np.stack([r.uniform(0, W, extra2), r.uniform(0, H, extra2)], axis=1)])
    o1, o2 = r.permutation(n1), r.permutation(n2)
    inv2 = np.empty(n2, np.int64)
    inv2[o2] = np.arange(n2)
    m = np.full(n1, -1, np.int32)
    m[:n] = inv2[np.arange(n)]
    return dict(xy1=xy1[o1].astype(np.float32), xy2=xy2[o2].astype(np.float32), matches12=m[o1].astype(np.int32))


# (matches, seed, planar, iters): the scenes of tests/test_two_view_gpu.py, whose conditions tests/test_two_view_cpu.py asserts on the
# model alone.  The match counts straddle the ballot word (64), half of it and the eight of a set; iters 1, 7 and 200.
SCENES = [(8, 1, False, 200), (9, 2, False, 200), (31, 3, False, 7), (32, 4, False, 200), (33, 5, False, 1), (63, 6, False, 200),
          (64, 7, False, 200), (65, 8, False, 200), (300, 9, False, 200), (2000, 10, False, 200),
          (9, 11, True, 7), (33, 12, True, 200), (65, 13, True, 200), (300, 14, True, 200)]
BAND = 1e-3     # a side whose chi-square lies within this, relative, of its threshold may fall either way
GATE = 1e-3     # the conditioning gate of check (a)

_cache = {}


def scene_models(n, seed, planar, iters, sigma=1.0):
    """(scene, float64 model, float32 model) of one entry of SCENES, computed once per process and not to be changed"""
    key = (n, seed, planar, iters, sigma)
    if key not in _cache:
        sc = make_scene(n, seed, planar)
        m64 = run_model(sc["xy1"], sc["xy2"], sc["matches12"], sigma, iters, dt=np.float64)
        m32 = run_model(sc["xy1"], sc["xy2"], sc["matches12"], sigma, iters, dt=np.float32)
        _cache[key] = (sc, m64, m32)
    return _cache[key]


def banded_sides(fam, M, xy1, xy2, sigma):
    """per match, per side: the float64 chi-square of matrix M lies within BAND of its threshold; also (score, flags)"""
    check = check_fundamental if fam else check_homography
    th = np.float64(np.float32(TH_F if fam else TH_H))
    sc, flags, c1, c2 = check(M, xy1, xy2, sigma, np.float64)
    chi = np.stack([c1, c2], axis=1)
    return np.abs(chi - th) <= BAND * th, sc, flags
