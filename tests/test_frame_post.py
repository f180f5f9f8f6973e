"""Frame post-processing (Frame.cpp:24-51): oracle KATs on the CPU, HIP-vs-oracle parity on the GPU."""
import numpy as np
import pytest

from monoorbslam3_amd import synth

KITTI = dict(width=1242, height=375, fx=718.856, fy=718.856, cx=607.1928, cy=185.2157)
EUROC = dict(width=752, height=480, fx=458.654, fy=457.296, cx=367.215, cy=248.375)
EUROC_DIST = (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05)


def _kps(oracle_mod, n, w, h, seed):
    rng = np.random.RandomState(seed)
    k = np.zeros(n, dtype=oracle_mod.KP_DTYPE)
    k["octave"] = rng.randint(0, 8, n)
    s = (1.2 ** k["octave"]).astype(np.float32)
    # level coordinates times the level scale, as operator() emits them (ORBExtractor.cpp:537-542)
    k["x"] = (rng.randint(19, w, n) / s).astype(np.int32).astype(np.float32) * s
    k["y"] = (rng.randint(19, h, n) / s).astype(np.int32).astype(np.float32) * s
    k["size"] = 31 * s
    k["angle"] = rng.uniform(0, 360, n)
    k["response"] = rng.randint(7, 200, n)
    k["class_id"] = -1
    return k


def _distort(cam, dist, x, y):
    """forward RAD_TAN model in float64 (what undistortion must invert)"""
    k = list(dist) + [0.0] * (12 - len(dist))
    xn, yn = (x - cam["cx"]) / cam["fx"], (y - cam["cy"]) / cam["fy"]
    r2 = xn * xn + yn * yn
    cd = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = xn * cd + 2 * k[2] * xn * yn + k[3] * (r2 + 2 * xn * xn)
    yd = yn * cd + k[2] * (r2 + 2 * yn * yn) + 2 * k[3] * xn * yn
    return xd * cam["fx"] + cam["cx"], yd * cam["fy"] + cam["cy"]


def test_oracle_undistort_is_copy_without_k1(oracle_mod):
    k = _kps(oracle_mod, 500, 1242, 375, 1)
    for dist in ((), (0.0, 0.1, 0.01, 0.01)):  # Pinhole.cpp:62 only looks at dist[0]
        raw, un, start, items = oracle_mod.frame_post(**KITTI, dist=dist, kps=k)
        assert raw.tobytes() == k.tobytes() and un.tobytes() == k.tobytes()
        assert start[-1] == len(k) and sorted(items) == list(range(len(k)))


def test_oracle_undistort_inverts_the_forward_model(oracle_mod):
    rng = np.random.RandomState(2)
    xu, yu = rng.uniform(60, 690, 400), rng.uniform(40, 440, 400)
    xd, yd = _distort(EUROC, EUROC_DIST, xu, yu)
    k = _kps(oracle_mod, 400, 752, 480, 3)
    k["x"], k["y"] = xd, yd
    raw, un, _, _ = oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=k)
    # only five fixed-point iterations (cv::undistortPoints' default): tight near the centre, ~0.07 px in the
    # corners of this strongly distorted camera (the forward shift there is 47 px)
    err = np.hypot(un["x"] - xu, un["y"] - yu)
    assert err.max() < 0.1
    centre = np.hypot(xu - EUROC["cx"], yu - EUROC["cy"]) < 150
    assert err[centre].max() < 2e-3
    assert np.array_equal(raw["x"], k["x"]) and np.array_equal(un["angle"], k["angle"])


def test_oracle_grid_is_cell_major_and_ascending(oracle_mod):
    k = _kps(oracle_mod, 2000, 752, 480, 4)
    _, un, start, items = oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=k)
    rows = 480 // 40
    assert len(start) == (752 // 40 + 1) * rows + 1  # Frame.cpp:32-40: 752 is not a multiple of 40
    for c in range(len(start) - 1):
        cell = items[start[c]:start[c + 1]]
        assert np.all(np.diff(cell) > 0)
        assert np.all((np.floor(un["x"][cell]).astype(int) // 40) * rows + np.floor(un["y"][cell]).astype(int) // 40 == c)
    inside = (np.floor(un["x"]) >= 0) & (np.floor(un["x"]) < 752) & (np.floor(un["y"]) >= 0) & (np.floor(un["y"]) < 480)
    assert start[-1] == inside.sum()


# ---------------------------------------------------------------------- edges: shared with test_frame_post_edges_gpu.py
# (width, height, cells): one cell, two, exactly one per thread of the grid kernel's 256, one more (two cells per thread,
# half the threads idle), a common size, and the largest grid orbf_create accepts
GRID_SIZES = [(40, 40, 1), (41, 40, 2), (640, 640, 256), (10280, 40, 257), (1920, 1080, 1296), (43880, 280, 7679)]
EUROC_K12 = EUROC_DIST + (0.01, 0.002, -0.001, 0.0005, 1e-4, -2e-4, 3e-4, 1e-5)
NEG_DIST = (-2.0, 0.3, 0.001, 0.001)  # icdist turns negative over most of the image
# groups of edge_kps()
UNIFORM, ON_BORDER, BELOW_BORDER, BELOW_SIZE, AT_SIZE, MINUS_HALF, MINUS_ZERO, MINUS_TINY, LAST_CELL, CELL_ZERO = range(10)


def grid_dim(v):
    return v // 40 + (v % 40 != 0)


def _below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def edge_kps(oracle_mod, w, h, seed):
    """About 1500 key points for a w x h camera, shuffled: returns (key points, group of each).  Every group puts its edge
    value in x for the first half and in y for the second half, the other coordinate uniform inside the image."""
    rng = np.random.RandomState(seed)
    cols, rows = grid_dim(w), grid_dim(h)

    def inside(n, lo_x=0, hi_x=w, lo_y=0, hi_y=h):
        x = np.minimum(rng.uniform(lo_x, hi_x, n).astype(np.float32), _below(hi_x))
        y = np.minimum(rng.uniform(lo_y, hi_y, n).astype(np.float32), _below(hi_y))
        return x, y

    def edged(n, ex, ey):
        x, y = inside(n)
        x[: n // 2] = ex[: n // 2]
        y[n // 2:] = ey[n // 2:]
        return x, y

    def const(v):
        return np.full(64, v, np.float32)

    bx, by = 40.0 * rng.randint(0, cols, 160), 40.0 * rng.randint(0, rows, 160)
    ux, uy = 40.0 * rng.randint(0, cols + 1, 160), 40.0 * rng.randint(0, rows + 1, 160)  # 0 gives a negative denormal
    parts = [(UNIFORM, inside(300)),
             (ON_BORDER, edged(160, bx.astype(np.float32), by.astype(np.float32))),
             (BELOW_BORDER, edged(160, _below(ux), _below(uy))),
             (BELOW_SIZE, edged(64, const(_below(w)), const(_below(h)))),
             (AT_SIZE, edged(64, const(w), const(h))),
             (MINUS_HALF, edged(64, const(-0.5), const(-0.5))),
             (MINUS_ZERO, edged(64, const(-0.0), const(-0.0))),
             (MINUS_TINY, edged(64, const(-1e-7), const(-1e-7))),
             (LAST_CELL, inside(600, 40 * (cols - 1), w, 40 * (rows - 1), h)),
             (CELL_ZERO, inside(100, 0, min(w, 40), 0, min(h, 40)))]
    group = np.concatenate([np.full(len(p[0]), g) for g, p in parts])
    order = rng.permutation(len(group))
    k = _kps(oracle_mod, len(group), 60, 60, seed + 1)
    k["x"] = np.concatenate([p[0] for _, p in parts])[order]
    k["y"] = np.concatenate([p[1] for _, p in parts])[order]
    return k, group[order]


def uniform_kps(oracle_mod, n, w, h, seed):
    rng = np.random.RandomState(seed)
    k = _kps(oracle_mod, n, w, h, seed + 1)
    k["x"], k["y"] = rng.uniform(0, w, n), rng.uniform(0, h, n)
    return k


def undistort_model(cam, dist, u, v):
    """cv::undistortPoints' five fixed-point iterations restated in float64 numpy, operation for operation.  Returns (x, y as
    float32, exit): exit is the iteration at which icdist < 0 ended the loop for that point, -1 where all five ran."""
    k = np.zeros(12)
    k[: len(dist)] = np.asarray(dist, np.float32)  # the camera holds floats
    fx, fy, cx, cy = (float(np.float32(cam[n])) for n in ("fx", "fy", "cx", "cy"))
    u, v = np.asarray(u, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
    x0, y0 = (u - cx) * (1. / fx), (v - cy) * (1. / fy)
    x, y, live, exit_at = x0.copy(), y0.copy(), np.ones(len(u), bool), np.full(len(u), -1)
    with np.errstate(all="ignore"):  # points that have left the loop keep being computed, and thrown away
        for j in range(5):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            out = live & (icdist < 0)
            exit_at[out] = j
            live &= ~out
            dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = np.where(live, (x0 - dx) * icdist, np.where(out, x0, x))
            y = np.where(live, (y0 - dy) * icdist, np.where(out, y0, y))
        return (fx * x + 0. * y + cx).astype(np.float32), (0. * x + fy * y + cy).astype(np.float32), exit_at


def check_undistort_branches(exit_at):
    """the coverage the NEG_DIST case is there for: every one of the five exits is taken, and the plain path too"""
    counts = [int((exit_at == j).sum()) for j in range(5)]
    assert all(c > 0 for c in counts), counts
    assert (exit_at == -1).sum() >= 1000
    return counts


def fisheye_case(oracle_mod):
    """(size_scale table, key points): fractional coordinates (the lookup truncates), the last pixel, all inside the image."""
    rng = np.random.RandomState(21)
    w, h = EUROC["width"], EUROC["height"]
    table = rng.uniform(0.8, 2.5, (h, w)).astype(np.float32)
    k = _kps(oracle_mod, 1200, w, h, 22)
    k["x"] = (rng.randint(0, w, 1200) + rng.choice([0.0, 0.25, 0.5, 0.99], 1200)).astype(np.float32)
    k["y"] = (rng.randint(0, h, 1200) + rng.choice([0.0, 0.25, 0.5, 0.99], 1200)).astype(np.float32)
    k["x"][:8], k["y"][:8] = 100.99, 200.99
    k["x"][8:16], k["y"][8:16] = w - 1, h - 1
    k["x"][16:24], k["y"][16:24] = w - 1, rng.randint(0, h, 8) + 0.99
    assert k["x"].min() >= 0 and k["x"].max() < w and k["y"].min() >= 0 and k["y"].max() < h  # the table index stays in range
    return table, k


@pytest.mark.parametrize("w,h,cells", GRID_SIZES)
def test_oracle_grid_at_borders_and_sizes(oracle_mod, w, h, cells):
    """PosInGrid restated in three lines of numpy: floor, bounds, cx * rows + cy."""
    k, group = edge_kps(oracle_mod, w, h, 30)
    raw, un, start, items = oracle_mod.frame_post(width=w, height=h, fx=500., fy=500., cx=w / 2, cy=h / 2, dist=(), kps=k)
    assert un.tobytes() == k.tobytes() and raw.tobytes() == k.tobytes()
    rows = grid_dim(h)
    assert len(start) == cells + 1 == grid_dim(w) * rows + 1
    fx, fy = np.floor(k["x"].astype(np.float64)), np.floor(k["y"].astype(np.float64))
    inside = (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    cell = ((fx // 40) * rows + fy // 40).astype(np.int64)
    idx = np.flatnonzero(inside)
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(np.bincount(cell[idx], minlength=cells))]))
    assert np.array_equal(items, idx[np.argsort(cell[idx], kind="stable")])
    # truncation instead of floor would put (-1, 0) into column / row 0; `<=` instead of `<` would keep x == width
    for g in (AT_SIZE, MINUS_HALF, MINUS_TINY):
        assert not np.isin(np.flatnonzero(group == g), items).any(), g
    assert np.isin(np.flatnonzero(group == MINUS_ZERO), items).all()  # floor(-0.0) == 0
    assert np.isin(np.flatnonzero((group == BELOW_SIZE) | (group == LAST_CELL) | (group == CELL_ZERO)), items).all()
    assert start[-1] - start[-2] >= 600 and start[1] >= 100  # the two crowded cells
    negative_denormal = (k["x"] < 0) & (k["x"] > -1e-40) | (k["y"] < 0) & (k["y"] > -1e-40)
    assert negative_denormal.any() and not np.isin(np.flatnonzero(negative_denormal), items).any()


def test_oracle_undistort_takes_every_exit(oracle_mod):
    k = uniform_kps(oracle_mod, 3000, 752, 480, 5)
    x, y, exit_at = undistort_model(EUROC, NEG_DIST, k["x"], k["y"])
    counts = check_undistort_branches(exit_at)
    assert sum(counts) + (exit_at == -1).sum() == 3000
    _, un, _, _ = oracle_mod.frame_post(**EUROC, dist=NEG_DIST, kps=k)
    assert un["x"].tobytes() == x.tobytes() and un["y"].tobytes() == y.tobytes()
    # a point that left through icdist < 0 is back where it started, up to the rounding of (u - cx) / fx * fx + cx
    out = exit_at >= 0
    assert np.abs(un["x"][out] - k["x"][out]).max() < 1e-3 and np.abs(un["y"][out] - k["y"][out]).max() < 1e-3


@pytest.mark.parametrize("n_dist", [1, 2, 5, 8])
def test_oracle_absent_coefficients_are_zeros(oracle_mod, n_dist):
    k = uniform_kps(oracle_mod, 800, 752, 480, 6)
    short = oracle_mod.frame_post(**EUROC, dist=EUROC_K12[:n_dist], kps=k)
    full = oracle_mod.frame_post(**EUROC, dist=EUROC_K12[:n_dist] + (0.0,) * (12 - n_dist), kps=k)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(short, full))
    x, y, _ = undistort_model(EUROC, EUROC_K12[:n_dist], k["x"], k["y"])
    assert short[1]["x"].tobytes() == x.tobytes() and short[1]["y"].tobytes() == y.tobytes()
    assert not np.array_equal(short[1]["x"], k["x"])


@pytest.mark.parametrize("case", ["k1_zero", "k1_minus_zero", "fisheye"])
def test_oracle_undistort_is_copy(oracle_mod, case):
    k = uniform_kps(oracle_mod, 500, 752, 480, 7)
    dist, kw = {"k1_zero": ((0.0, 0.1, 0.01, 0.01), {}), "k1_minus_zero": ((-0.0, 0.1, 0.01, 0.01), {}),
                "fisheye": (EUROC_DIST, dict(undistort=False))}[case]
    raw, un, _, _ = oracle_mod.frame_post(**EUROC, dist=dist, kps=k, **kw)
    assert raw.tobytes() == k.tobytes() and un.tobytes() == k.tobytes()


def test_oracle_size_scale_lookup_truncates(oracle_mod):
    table, k = fisheye_case(oracle_mod)
    raw, un, _, _ = oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=k, undistort=False, size_scale=table)
    assert np.array_equal(raw["size"], k["size"] * table[k["y"].astype(np.int32), k["x"].astype(np.int32)])
    assert np.array_equal(raw["x"], k["x"]) and un.tobytes() == raw.tobytes()
    assert (np.round(k["x"]) != np.trunc(k["x"])).sum() > 100  # rounding would have read another entry


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["kitti_nodist", "euroc", "euroc_k3", "fisheye"])
def test_frame_post_parity(oracle_mod, case):
    from monoorbslam3_amd.frame import FramePost
    if case == "kitti_nodist":
        cam, dist, kw = KITTI, (), {}
    elif case == "euroc":
        cam, dist, kw = EUROC, EUROC_DIST, {}
    elif case == "euroc_k3":
        cam, dist, kw = EUROC, EUROC_DIST + (0.01, 0.002, -0.001, 0.0005, 1e-4, -2e-4, 3e-4, 1e-5), {}
    else:
        rng = np.random.RandomState(8)
        cam, dist = EUROC, EUROC_DIST
        kw = dict(undistort=False, size_scale=rng.uniform(0.8, 2.5, (480, 752)).astype(np.float32))
    k = _kps(oracle_mod, 2500, cam["width"], cam["height"], 11)
    k["x"][:40] = np.linspace(-3, cam["width"] + 3, 40)  # some key points leave the image after undistortion
    want = oracle_mod.frame_post(**cam, dist=dist, kps=k, **kw)
    fp = FramePost(**cam, dist=dist, **kw)
    got = fp(k)
    for g, w, name in zip(got, want, ("raw", "undistorted", "cell_start", "cell_items")):
        assert g.tobytes() == w.tobytes(), name
    assert len(fp(k[:0])[3]) == 0  # empty frame


@pytest.mark.gpu
def test_frame_post_batch_on_extractor_output(oracle_mod):
    """extract_batch_device -> frame_post_device without leaving the GPU; every frame equals the oracle's record."""
    import torch
    from monoorbslam3_amd.extractor import ORBExtractor
    from monoorbslam3_amd.frame import FramePost
    B, W, H = 6, 752, 480
    frames = synth.make_frames(B, W, H, seed=77)
    ex = ORBExtractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    cap = ex.max_keypoints(W, H)
    d_img = torch.from_numpy(frames).cuda()
    kp = torch.zeros((B, cap, 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    ex.extract_batch_device(d_img.data_ptr(), B, W, H, W, W * H, kp.data_ptr(), desc.data_ptr(), cap, n.data_ptr(),
                            s.cuda_stream)
    fp = FramePost(**EUROC, dist=EUROC_DIST)
    un = torch.zeros_like(kp)
    start = torch.zeros((B, fp.n_cells + 1), dtype=torch.int32, device="cuda")
    items = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    fp.post_device(B, kp.data_ptr(), n.data_ptr(), cap, un.data_ptr(), start.data_ptr(), items.data_ptr(), s.cuda_stream)
    s.synchronize()
    n_h = n.cpu().numpy()
    for f in range(B):
        raw_h = kp[f].cpu().numpy().view(oracle_mod.KP_DTYPE).reshape(-1)[: n_h[f]]
        w_raw, w_un, w_start, w_items = oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=raw_h)
        assert un[f].cpu().numpy().view(oracle_mod.KP_DTYPE).reshape(-1)[: n_h[f]].tobytes() == w_un.tobytes()
        assert np.array_equal(start[f].cpu().numpy(), w_start)
        assert np.array_equal(items[f].cpu().numpy()[: w_start[-1]], w_items)
