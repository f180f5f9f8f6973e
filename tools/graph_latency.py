"""Latency of the covisibility-graph step of one new key frame, both ways in one run: 200 key frames whose lists hold about 40
neighbours over CONNECT_TH, 2000 slots per key frame, 60000 table rows.
  device form   orbm_update_connections_device -> orbm_fuse_targets_device -> orbm_connected_keyframes_device on one stream, device
                time between two HIP events; the graph's arrays are restored by device copies outside the timed span.  Twice: as
                enqueued from Python on an idle stream, where the span also holds the gaps in which the device waits for the next
                launch, and behind a stream kept busy by large fills, so that all three launches are queued before the first one
                starts and the kernels run back to back (with the caches the fills left: cold)
  host form     the parent commit's: wait, read d_covis, the slot arrays, d_n and d_valid back, the array model of tests/graph_model.py
                (`update`, `fuse_targets`, `connected`: numpy and Python loops), upload d_local, the targets and the rows.  Host wall
                time up to the wait that ends the uploads.  The loops are NUMPY's and Python's, not the reference's C++: the figure bounds
                what the host hop costs here, it is not a measurement of KeyFrame::updateConnections.
p50 (and p90) of `reps` calls after `warm` warm-up calls, every form.  Writes profiles/graph_latency.txt (or
the path given as the first argument)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def make_scene(n_kf=200, stride=2000, cap=60000, near=40, seed=7):
    import graph_model as gm
    rng = np.random.RandomState(seed)
    g = gm.new_graph(n_kf)
    bad = np.zeros(n_kf, np.uint8)

    def covis_of(k):
        v = np.zeros(n_kf, np.int32)
        others = rng.choice(np.delete(np.arange(n_kf), k), near + 15, replace=False)
        v[others[:near]] = rng.randint(gm.CONNECT_TH, 120, near)
        v[others[near:]] = rng.randint(1, gm.CONNECT_TH, 15)
        return v

    for k in range(n_kf - 1):
        gm.update(g, n_kf, bad, covis_of(k), k, 0)
    cur = n_kf - 1
    slots = rng.randint(0, cap, (n_kf, stride)).astype(np.int32)
    slots[rng.rand(n_kf, stride) < 0.4] = -1
    return dict(g=g, bad=bad, cur=cur, covis=covis_of(cur), slots=slots, n=np.full(n_kf, stride, np.int32),
                valid=(rng.rand(cap) < 0.97).astype(np.uint8), n_kf=n_kf, stride=stride, cap=cap)


def main(out_path):
    import torch
    import graph_model as gm
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.matcher import CovisGraph, ORBMatcher
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    warm, reps = 20, 300
    sc = make_scene()
    n_kf, stride, cap, cur = sc["n_kf"], sc["stride"], sc["cap"], sc["cur"]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    zi = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    begin = {k: up(sc["g"][k]) for k in ("weight", "ord_kf", "ord_n", "parent")}
    now = {k: v.clone() for k, v in begin.items()}
    graph = CovisGraph.make(now["weight"], now["ord_kf"], now["ord_n"], now["parent"])
    cap_targets, cap_rows = 120, cap
    d = dict(bad=up(sc["bad"]), covis=up(sc["covis"]), n=up(sc["n"]), slots=up(sc["slots"]), valid=up(sc["valid"]), work_kf=zi(n_kf), work=zi(cap),
             targets=zi(cap_targets), rows=zi(cap_rows), out=zi(n_kf + 1), n_out=zi(1))
    res = {k: zi(8) for k in ("update", "targets")}
    m = ORBMatcher()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def restore():
        for k, v in begin.items():
            now[k].copy_(v)

    busy = torch.empty(64 << 20, dtype=torch.int32, device=dev)            # 256 MB: eight fills outlast the three launches many times

    def device_form(behind_busy=False):
        if behind_busy:
            for _ in range(8):
                busy.zero_()
        e0.record()
        m.UpdateConnectionsDevice(graph, dict(d, work=d["work_kf"], result=res["update"]), n_kf, cur, first_kf=0)
        m.FuseTargetsDevice(graph, dict(d, result=res["targets"]), n_kf, stride, cap, cur, cap_targets, cap_rows)
        m.ConnectedKeyFramesDevice(graph, d, n_kf, cur)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def host_form():
        t0 = time.perf_counter()
        torch.cuda.synchronize()                                           # the wait the chain has to make
        covis, slots, n, valid = (d[k].cpu().numpy() for k in ("covis", "slots", "n", "valid"))
        g = gm.copy_graph(sc["g"])                                         # the host's own graph
        r_up = gm.update(g, n_kf, sc["bad"], covis, cur, 0)
        targets, rows, r_t = gm.fuse_targets(g, n_kf, n, sc["bad"], slots, stride, valid, cap, cur)
        local, n_local = gm.connected(g, n_kf, cur, True, n_kf, n_kf + 1)
        d["out"].copy_(torch.from_numpy(local))
        d["targets"][:len(targets)].copy_(torch.from_numpy(targets))
        d["rows"][:len(rows)].copy_(torch.from_numpy(rows))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, (g, r_up, targets, rows, r_t, local)

    t = dict(device=[], queued=[], host=[])
    for key, behind_busy in (("device", False), ("queued", True)):
        for i in range(warm + reps):
            restore()
            a = device_form(behind_busy)
            if i >= warm:
                t[key].append(a)
    for i in range(warm + reps):
        us, want = host_form()
        if i >= warm:
            t["host"].append(us)
    restore()
    device_form()
    g, r_up, targets, rows, r_t, local = want
    c = lambda x: x.cpu().numpy()  # noqa: E731
    same = (np.array_equal(c(res["update"]), r_up) and np.array_equal(c(res["targets"]), r_t) and np.array_equal(c(d["targets"])[:len(targets)], targets)
            and np.array_equal(c(d["rows"])[:len(rows)], rows) and np.array_equal(c(d["out"]), local) and np.array_equal(c(now["weight"]), g["weight"])
            and np.array_equal(c(now["ord_n"]), g["ord_n"]) and np.array_equal(c(now["parent"]), g["parent"]))
    pct = lambda v, q: float(np.percentile(v, q))  # noqa: E731
    lines = [
        "the graph step of one new key frame: %d key frames x %d slots, %d table rows; d_result of the update %s, of the fuse targets %s; kernels %s"
        % (n_kf, stride, cap, r_up.tolist(), r_t.tolist(), _lib.kernels_sha16()),
        "device form (orbm_update_connections_device -> orbm_fuse_targets_device -> orbm_connected_keyframes_device, device time by HIP events), "
        "p50 / p90 of %d after %d warm-up calls: %.1f / %.1f us enqueued from Python on an idle stream (the waits for the next launch included), "
        "%.1f / %.1f us with the three launches queued behind a busy stream (back to back, caches cold)"
        % (reps, warm, pct(t["device"], 50), pct(t["device"], 90), pct(t["queued"], 50), pct(t["queued"], 90)),
        "host form (wait, d_covis / slots / d_n / d_valid read-back, the model's PYTHON loops, d_local / targets / rows uploaded), host wall time, "
        "p50 / p90 of %d after %d warm-up calls: %.1f / %.1f us   (numpy's and Python's loops, not the reference's C++)"
        % (reps, warm, pct(t["host"], 50), pct(t["host"], 90)),
        "both forms gave the same bytes: %s" % same,
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "graph_latency.txt"))
