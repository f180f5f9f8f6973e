"""The IMU preintegration and pose prediction on the MI355X (include/orbi.h) against the float32 run of tests/imu_model.py, BIT FOR
BIT: every field of every record, every pool row and d_result, with padded arrays and intact guards.  No tolerances, no exclusions.
Model outputs are computed once per scene and shared."""
import numpy as np
import pytest

import imu_model as im
import projection_model as pm
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _bits, _stream, _up

pytestmark = pytest.mark.gpu

_cache = {}


def _calib(cal):
    from monoorbslam3_amd import imu
    return imu.Calib.make(cal["Rcb"], cal["tcb"], cal["cov_noise"], cal["cov_walk"], cal["gravity"])


def _model(key, make, run):
    """(scene, packed bank and pool as passed, packed bank and pool after, d_result) -- computed once, shared, never changed"""
    if key not in _cache:
        sc = make()
        before = sc["bank"].pack()
        after = sc["bank"].copy()
        res = run(sc, after)
        _cache[key] = (sc, before, after.pack(), res)
    return _cache[key]


class _Device:
    """the bank, the pool and d_result as padded device arrays"""

    def __init__(self, torch, dev, bank, pool):
        self.torch, self.dev = torch, dev
        self.cap, self.cap_meas = len(bank), pool.shape[1]
        self.bank = _padded(torch, dev, np.frombuffer(bank.tobytes(), np.uint8), 0xA5)
        self.pool = _padded(torch, dev, pool, np.float32(-3.5))
        self.result = _padded(torch, dev, np.full(8, 77, np.int32), -6)

    def finish(self):
        self.torch.cuda.synchronize()
        self.torch.cuda.set_stream(self.torch.cuda.default_stream(self.dev))
        assert _guards_intact(self.bank[0], 0xA5) and _guards_intact(self.pool[0], np.float32(-3.5)) and _guards_intact(self.result[0], -6)
        bank = np.frombuffer(self.bank[1].cpu().numpy().tobytes(), im.RECORD)
        return bank, self.pool[1].cpu().numpy().reshape(self.cap, self.cap_meas, 7), self.result[1].cpu().numpy()


def _assert_state(got, want, what):
    """bank, pool, d_result: the same bytes; names the first field that differs"""
    (gb, gp, gr), (wb, wp, wr) = got, want
    print(what, "device d_result", gr.tolist(), "model", wr.tolist())
    assert np.array_equal(gr, wr), what
    for k in im.RECORD.names:
        same = np.array([gb[k][i].tobytes() == wb[k][i].tobytes() for i in range(len(wb))])
        assert same.all(), (what, k, "records", np.nonzero(~same)[0][:8].tolist())
    assert gb.tobytes() == wb.tobytes(), what
    rows = np.array([_bits(gp[i]).tobytes() == _bits(wp[i]).tobytes() for i in range(len(wp))])
    assert rows.all(), (what, "pool rows", np.nonzero(~rows)[0][:8].tolist())


def _integrate(torch, dev, sc, before, stream_kind):
    from monoorbslam3_amd import imu
    d = _Device(torch, dev, *before)
    jobs, samples = _up(torch, dev, sc["jobs"]), _up(torch, dev, sc["samples"])
    st = _stream(torch, dev, stream_kind)
    imu.integrate_device(_calib(sc["cal"]), d.bank[1], d.pool[1], d.cap, d.cap_meas, jobs, len(sc["jobs"]), samples, len(sc["samples"]),
                         d.result[1], stream=st)
    got = d.finish()
    assert jobs.cpu().numpy().tobytes() == sc["jobs"].tobytes() and samples.cpu().numpy().tobytes() == sc["samples"].tobytes()
    return got


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("n_jobs", [1, 4, 5, 257])
def test_integrate_equals_the_model(n_jobs, stream_kind):
    """1, 4, 5 (the edge of a four-wave workgroup: d_result is added up over two workgroups) and 257 jobs of 65, 0, 1, 2 and 3 samples
    (65: three staged chunks, the last of one sample).  The large scene also holds two jobs sharing one sample range, a job with gyro ==
    bias.bg (the d < 1e-6 branch of ExpSO3f / RightJacobianSO3f), a pool row filled exactly, one a sample over (refused: record and
    row as passed, d_result[4] = 71), ids -1 and cap, a repeated id and a sample range past the array.  Every record, every pool row
    and d_result equal the model's bytes; the inputs are as passed."""
    import torch
    dev = torch.device("cuda", 0)
    sc, before, after, res = _model(("integrate", n_jobs), lambda: im.make_integrate_scene(n_jobs),
                                    lambda sc, bank: im.run_integrate(sc["cal"], bank, sc["jobs"], sc["samples"]))
    if sc["special"]:
        assert res.tolist() == [n_jobs - 5, 3, 1, 1, im.CAP_MEAS + 1, 0, 0, 0]
        full = int(sc["jobs"][12]["id"])
        assert after[0]["n_meas"][full] == im.CAP_MEAS
    else:
        assert res.tolist() == [n_jobs, 0, 0, 0, 0, 0, 0, 0]
    _assert_state(_integrate(torch, dev, sc, before, stream_kind), after + (res,), "integrate %d" % n_jobs)


def test_zero_jobs_write_eight_zeros_and_nothing_else():
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    sc, before, _, _ = _model(("integrate", 4), lambda: im.make_integrate_scene(4), lambda sc, bank: im.run_integrate(sc["cal"], bank, sc["jobs"], sc["samples"]))
    cal = _calib(sc["cal"])
    ids = _up(torch, dev, np.zeros(1, np.int32))
    bias = _up(torch, dev, np.zeros(6, np.float32))
    jobs, samples = _up(torch, dev, sc["jobs"]), _up(torch, dev, sc["samples"])
    calls = [lambda d: imu.reset_device(d.bank[1], d.cap, ids, 0, d.result[1]),
             lambda d: imu.integrate_device(cal, d.bank[1], d.pool[1], d.cap, d.cap_meas, jobs, 0, samples, len(sc["samples"]), d.result[1]),
             lambda d: imu.set_bias_device(cal, d.bank[1], d.pool[1], d.cap, d.cap_meas, ids, bias, 0, d.result[1]),
             lambda d: imu.merge_next_device(cal, d.bank[1], d.pool[1], d.cap, d.cap_meas, ids, ids, 0, d.result[1])]
    for k, call in enumerate(calls):
        d = _Device(torch, dev, *before)
        call(d)
        _assert_state(d.finish(), before + (np.zeros(8, np.int32),), "zero jobs, call %d" % k)


def test_set_bias_equals_the_model():
    """bg steps whose float norm lies 3 .. 12 ulps below (two) and above (two) 0.01 -- the scene asserts it --, a step of 0.05 on a FULL
    pool row (70 measurements re-integrated: three staged chunks), small steps, a record without measurements, ids -1 and cap, a
    repeated id: three jobs re-integrate, and bank, pool and d_result equal the model's bytes."""
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    sc, before, after, res = _model("bias", im.make_bias_scene, lambda sc, bank: im.run_set_bias(sc["cal"], bank, sc["ids"], sc["bias"]))
    assert res.tolist() == [9, 2, 1, 0, 0, 3, 0, 0]
    d = _Device(torch, dev, *before)
    imu.set_bias_device(_calib(sc["cal"]), d.bank[1], d.pool[1], d.cap, d.cap_meas, _up(torch, dev, sc["ids"]), _up(torch, dev, sc["bias"]),
                        len(sc["ids"]), d.result[1])
    _assert_state(d.finish(), after + (res,), "set_bias")
    assert after[0]["n_meas"][4] == im.CAP_MEAS and not after[0]["delta_bias"][4].any() and after[0]["delta_bias"][0].any()


def test_merge_next_equals_the_model():
    """delta_bias.bg norms of 5e-6 (the next list only) and 2e-5 (Reset, then both lists), a sum of 71 > cap_meas (refused before the
    reset: record and row as passed), a sum of exactly 70, an empty next, equal ids (counted, nothing written), ids out of range, two
    jobs that conflict with an earlier one and two that share a next with one: bank, pool and d_result equal the model's bytes."""
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    sc, before, after, res = _model("merge", im.make_merge_scene, lambda sc, bank: im.run_merge(sc["cal"], bank, sc["ids"], sc["nxt"]))
    assert res.tolist() == [8, 2, 2, 1, im.CAP_MEAS + 1, 2, 1, 0]
    d = _Device(torch, dev, *before)
    imu.merge_next_device(_calib(sc["cal"]), d.bank[1], d.pool[1], d.cap, d.cap_meas, _up(torch, dev, sc["ids"]), _up(torch, dev, sc["nxt"]),
                          len(sc["ids"]), d.result[1])
    _assert_state(d.finish(), after + (res,), "merge_next")
    assert after[0]["n_meas"][6] == im.CAP_MEAS and after[0]["n_meas"][4] == before[0]["n_meas"][4]


def test_reset_equals_the_model():
    """The three constructors and Reset on records that hold integrations: a given bias, another record's updated_bias (which differs
    from its bias), the record's own updated_bias (ReIntegrate's Reset), the zero bias of a call without d_bias; src < -1 and >= cap,
    id out of range, a repeated id and a src that an earlier job resets are dropped and counted.  n_meas = 0, pool rows untouched."""
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    ids = np.array([2, 3, 0, 4, -1, 12, 5, 6, 2, 7], np.int32)
    src = np.array([-1, 1, 0, 5, 1, -1, -2, 12, -1, 2], np.int32)
    bias = np.random.RandomState(5).normal(0, 0.02, (len(ids), 6)).astype(np.float32)

    def run(sc, bank):
        a, b = bank, bank.copy()
        return (a, im.run_reset(a, ids, src, bias)), (b, im.run_reset(b, ids[:4], None, None))

    key = "reset"
    if key not in _cache:
        sc = im.make_bias_scene()
        im.run_set_bias(sc["cal"], sc["bank"], sc["ids"], sc["bias"])      # updated_bias != bias in most records
        before = sc["bank"].pack()
        (a, res_a), (b, res_b) = run(sc, sc["bank"].copy())
        _cache[key] = (sc, before, a.pack(), res_a, b.pack(), res_b)
    sc, before, after_a, res_a, after_b, res_b = _cache[key]
    assert res_a.tolist() == [4, 4, 2, 0, 0, 0, 0, 0] and res_b.tolist() == [4, 0, 0, 0, 0, 0, 0, 0]
    assert all(before[0]["updated_bias"][i].tobytes() != before[0]["bias"][i].tobytes() for i in (0, 1, 5)) and not after_b[0]["bias"][ids[:4]].any()
    assert after_a[0]["bias"][3].tobytes() == before[0]["updated_bias"][1].tobytes() and after_a[0]["bias"][0].tobytes() == before[0]["updated_bias"][0].tobytes()
    d = _Device(torch, dev, *before)
    imu.reset_device(d.bank[1], d.cap, _up(torch, dev, ids), len(ids), d.result[1], d_src=_up(torch, dev, src), d_bias=_up(torch, dev, bias))
    _assert_state(d.finish(), after_a + (res_a,), "reset")
    d = _Device(torch, dev, *before)
    imu.reset_device(d.bank[1], d.cap, _up(torch, dev, ids), 4, d.result[1])
    _assert_state(d.finish(), after_b + (res_b,), "reset, default constructor")


def _predict_model():
    if "predict" not in _cache:
        sc = im.make_predict_scene()
        _cache["predict"] = (sc, sc["bank"].pack(), [im.predict(sc["cal"], sc["bank"].recs[i], sc["src"][i]) for i in range(3)])
    return _cache["predict"]


def test_predict_and_imu_pose_equal_the_model():
    """Three source states: no bias change, a small one (delta_bias != 0: the Jacobians and ExpSO3f(JRg * dbg) act) and a 300-sample
    integration with one.  orbi_predict_device: the destination's 15 floats and the pose doubles hold the model's float values bit for
    bit, in place (d_dst == d_src) as well and without the pose outputs; orbi_imu_pose_device on those doubles: the model's (Rwb, twb)
    bit for bit, the velocity untouched.  Padded outputs, intact guards."""
    import torch
    from monoorbslam3_amd import imu
    dev = torch.device("cuda", 0)
    sc, (bank, pool), want = _predict_model()
    cal = _calib(sc["cal"])
    d_bank = _up(torch, dev, bank)
    for i in range(3):
        dst, Rcw, tcw = want[i]
        src = _up(torch, dev, sc["src"][i])
        out = dict(dst=_padded(torch, dev, np.full(15, 7.5, np.float32), np.float32(-1.5)), R=_padded(torch, dev, np.full(9, 7.5), -2.5),
                   t=_padded(torch, dev, np.full(3, 7.5), -3.5), back=_padded(torch, dev, np.full(15, 9.25, np.float32), np.float32(-4.5)),
                   inplace=_padded(torch, dev, sc["src"][i], np.float32(-5.5)))
        imu.predict_device(cal, d_bank, 3, i, src, out["dst"][1], out["R"][1], out["t"][1])
        imu.predict_device(cal, d_bank, 3, i, out["inplace"][1], out["inplace"][1])
        imu.imu_pose_device(cal, out["R"][1], out["t"][1], out["back"][1])
        torch.cuda.synchronize()
        for k, fill in (("dst", np.float32(-1.5)), ("R", -2.5), ("t", -3.5), ("back", np.float32(-4.5)), ("inplace", np.float32(-5.5))):
            assert _guards_intact(out[k][0], fill), k
        g = {k: v[1].cpu().numpy() for k, v in out.items()}
        assert np.array_equal(_bits(g["dst"]), _bits(dst)), i
        assert np.array_equal(_bits(g["inplace"]), _bits(dst)), i
        assert g["R"].tobytes() == Rcw.reshape(9).astype(np.float64).tobytes() and g["t"].tobytes() == tcw.astype(np.float64).tobytes(), i
        Rwb, twb = im.imu_pose(sc["cal"], g["R"], g["t"])
        assert np.array_equal(_bits(g["back"][:9]), _bits(Rwb.reshape(9))) and np.array_equal(_bits(g["back"][9:12]), _bits(twb)), i
        assert (g["back"][12:] == np.float32(9.25)).all()
        assert d_bank.cpu().numpy().tobytes() == bank.tobytes() and src.cpu().numpy().tobytes() == sc["src"][i].tobytes()


def _chain_model():
    """the tracker's frame: ten samples into the last frame's and the last key frame's record, the prediction from the last frame, the
    frame form's queries under the predicted pose"""
    if "chain" not in _cache:
        rng = np.random.RandomState(17)
        cal = im.calib()
        bank = im.Bank(2, 64)
        for r in bank.recs:
            r.reset(im.random_bias(rng))
        im.prefill(cal, bank, 1, 40, 41)                                    # the key frame is several frames old
        samples = im.make_stream(10, 42)
        jobs = np.zeros(2, im.JOB)
        for j in range(2):
            jobs[j] = (j, 0, 10, 0, samples["t"][0] - 0.4 / im.RATE - float(bank.recs[j].delta_t), samples["t"][-1] + 0.6 / im.RATE)
        src = np.concatenate([im.rodrigues([0.3, -0.2, 0.5]).reshape(9), [0.4, -1.0, 0.2], [0.5, 0.1, -0.3]]).astype(np.float32)
        before = bank.pack()
        res = im.run_integrate(cal, bank, jobs, samples)
        dst, Rcw, tcw = im.predict(cal, bank.recs[0], src)
        cloud = pm.make_cloud(pm.FRAME, False, 1500, 23)
        # the cloud as the predicted camera sees it where the cloud's own pose saw it: every gate keeps its share
        Pc = cloud["points"].astype(np.float64) @ cloud["R"].T + cloud["t"]
        points = ((Pc - tcw.astype(np.float64)) @ Rcw.astype(np.float64)).astype(np.float32)
        q = pm.evaluate(pm.FRAME, cloud["cam"], cloud["bounds"], Rcw, tcw, points, cloud["valid"], kps1=cloud["kps1"], th=cloud["th"])
        assert q["result"][0] >= 0.3 * cloud["n"] and (q["result"][1:4] >= 0.02 * cloud["n"]).all()
        _cache["chain"] = dict(cal=cal, before=before, after=bank.pack(), res=res, jobs=jobs, samples=samples, src=src, dst=dst, Rcw=Rcw, tcw=tcw,
                               cloud=cloud, points=points, q=q)
    return _cache["chain"]


@pytest.mark.parametrize("stream_kind", ["null", "explicit"])
def test_chain_integrate_predict_project_on_one_stream_with_one_wait(stream_kind):
    """orbi_integrate_device (the last frame and the last key frame, the same ten samples) -> orbi_predict_device ->
    orbm_project_frame_device with a Pinhole camera, enqueued back to back on one stream, ONE wait at the end: the records, the
    predicted state and the queries equal the models' (tests/projection_model.py fed with the model's predicted pose) bit for bit."""
    import torch
    from monoorbslam3_amd import imu
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    c = _chain_model()
    cloud, n = c["cloud"], c["cloud"]["n"]
    cal = _calib(c["cal"])
    d = _Device(torch, dev, *c["before"])
    jobs, samples, src = _up(torch, dev, c["jobs"]), _up(torch, dev, c["samples"]), _up(torch, dev, c["src"])
    dst = torch.full((15,), 7.5, dtype=torch.float32, device=dev)
    q = dict(pose_R=torch.full((9,), 7.5, dtype=torch.float64, device=dev), pose_t=torch.full((3,), 7.5, dtype=torch.float64, device=dev),
             points=_up(torch, dev, c["points"]), valid=_up(torch, dev, cloud["valid"]), kps1=_up(torch, dev, cloud["kps1"]),
             q_xy=torch.full((n, 2), 7.5, dtype=torch.float32, device=dev), q_radius=torch.full((n,), 7.5, dtype=torch.float32, device=dev),
             q_level=torch.full((n,), 77, dtype=torch.int32, device=dev), q_angle=torch.full((n,), 7.5, dtype=torch.float32, device=dev),
             q_ok=torch.full((n,), 7, dtype=torch.uint8, device=dev), result=torch.full((8,), 77, dtype=torch.int32, device=dev))
    m = ORBMatcher()
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    st = _stream(torch, dev, stream_kind)
    imu.integrate_device(cal, d.bank[1], d.pool[1], d.cap, d.cap_meas, jobs, 2, samples, len(c["samples"]), d.result[1], stream=st)
    imu.predict_device(cal, d.bank[1], d.cap, 0, src, dst, q["pose_R"], q["pose_t"], stream=st)
    m.ProjectFrameDevice(cam, q, n, cloud["th"], stream=st)
    _assert_state(d.finish(), c["after"] + (c["res"],), "chain")           # the one wait
    assert np.array_equal(_bits(dst.cpu().numpy()), _bits(c["dst"]))
    assert q["pose_R"].cpu().numpy().tobytes() == c["Rcw"].reshape(9).astype(np.float64).tobytes()
    assert q["pose_t"].cpu().numpy().tobytes() == c["tcw"].astype(np.float64).tobytes()
    want = c["q"]
    assert np.array_equal(q["result"].cpu().numpy(), want["result"]) and np.array_equal(q["q_ok"].cpu().numpy(), want["q_ok"])
    for k in ("q_xy", "q_radius", "q_angle"):
        assert np.array_equal(_bits(q[k].cpu().numpy()), _bits(want[k].astype(np.float32))), k
    assert np.array_equal(q["q_level"].cpu().numpy(), want["q_level"])
