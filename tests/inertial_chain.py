"""The scenes of localInertialBundleAdjustment's optimisation (include/orbil.h) and their model runs: TEST CODE ONLY, shared by
tests/test_inertial_chain_cpu.py and tests/test_inertial_chain_gpu.py.

A scene is factors_model.make_chain with the fixed flags orbm_inertial_chain_problem_device gives (15 for the oldest state: it has no
pose vertex and setFixed(i == 0) fixes its velocity and biases, Optimize.cpp:992-1007; FIX_POSE for the rest) and no priors.  The model
of the loop is inertial_loop.ModelPose(sc, visual=False) under inertial_loop.optimize(be, 10) -- vi_model.solve handles any n --, and the
model of the staged solve is vi_model.solve itself.

What a loop scene needs, and why make_chain's defaults do not give it.  With every pose fixed the problem is linear in the velocities and
nearly so in the biases, so ten iterations of g2o's policy reach the minimum after five or six and decide the rest on rounding -- and
with make_chain's pose noise, which a fixed pose cannot shed, and its records' unrelated biases under the calibration's tight walks the
total stays at 1e4 to 1e5 there, where the float cast of the bias vertices (Imu.cpp:182-192) alone moves it by more than computeScale's
1e-3: such a trial is decided by rounding at |rho| > 1 and inertial_loop.flat_from() does not see it.  So the chain is built with
noise 0 (the states are what the records predict), a calibration whose bias walks are loose (WALKS), and the free vertices disturbed by
DISTURB = sigma of (velocity, gyro bias, acc bias): the gyro bias enters through Log of a rotation, and at 2 rad/s that keeps all ten
iterations gaining (rho 0.3 to 1); at 5 rad/s a Gauss-Newton step overshoots, and the policy rejects and accepts in turn on |rho| > 0.2.
tests/test_inertial_chain_cpu.py holds every scene to the condition of tests/test_inertial_loop_cpu.py.

The shapes are the smallest at which the band walk, the passes of the edges over the eight waves and the cap can go wrong:
  "chain 2"             one edge, one block column with a successor
  "chain 3"             a block column with a predecessor and a successor
  "chain 10"            9 edges, one more than the eight waves of a pass
  "chain 20"            19 edges, ORBIL_MAX_STATES
  "chain 10 rejecting"  rejected trials followed by accepted ones, under the default lambda init
  "chain 4 refused"     the last edge without its walks, so the last state's biases have zero rows, and lambda forced to 0: the first
                        pivot there is 0, every solve is refused, 0 * ni stays 0, all max_trials trials have temp = DBL_MAX and the
                        estimate keeps its starting bytes
A model run is computed once and shared: nobody changes it."""
import numpy as np

import factors_model as fm
import imu_model as im
import inertial_loop as il
import vi_model as vm

ITERATIONS = 10
FULL = (100,) * 5                                     # full records: a closed loop needs their baselines (tests/inertial_loop.py)
WALKS = dict(walk_gyro=0.2, walk_acc=3.0)             # im.calib's: loose bias walks
DISTURB = (0.5, 2.0, 0.3)
# name -> (states, make_chain's seed, the disturbance, optimize's keywords)
SCENES = {
    "chain 2": (2, 21, DISTURB, {}),
    "chain 3": (3, 22, DISTURB, {}),
    "chain 10": (10, 23, DISTURB, {}),
    "chain 20": (20, 24, DISTURB, {}),
    "chain 10 rejecting": (10, 25, (0.5, 5.0, 0.3), {}),
    "chain 4 refused": (4, 26, DISTURB, dict(forced_lambda_init=0.0)),
}
REFUSED, REJECTING = "chain 4 refused", "chain 10 rejecting"
# the mapper chain's scene: the graph as orbi_graph_init_device leaves it, nothing disturbed.  No loop is judged on it (it decides on
# rounding from its sixth iteration on); the chain of calls is held to its own bytes and to the models of the calls around the loop
MAP_SCENE = "chain 3 as initialised"
EXTRA = {MAP_SCENE: (3, 22, (0.0, 0.0, 0.0), {})}
_scenes, _runs = {}, {}


def chain_fixed(n):
    """d_fixed of orbm_inertial_chain_problem_device"""
    return np.array([15] + [fm.FIX_POSE] * (n - 1), np.uint8)


def scene(name):
    if name not in _scenes:
        n, seed, (dv, dbg, dba), _ = dict(SCENES, **EXTRA)[name]
        sc = fm.make_chain(n - 1, seed=seed, noise=0.0, cal=im.calib(**WALKS), sample_counts=FULL)
        g = sc["graph"]
        g.fixed[:] = chain_fixed(n)
        rng = np.random.RandomState(seed + 500)
        g.v[1:] += rng.normal(0, dv, (n - 1, 3))
        g.bg[1:] += rng.normal(0, dbg, (n - 1, 3))
        g.ba[1:] += rng.normal(0, dba, (n - 1, 3))
        if name == REFUSED:
            sc["edges"]["flags"][-1] = 0
        sc["priors"], sc["pjobs"] = np.zeros(1, fm.PRIOR), np.zeros(0, fm.PRIOR_JOB)
        _scenes[name] = sc
    return _scenes[name]


def options(name):
    """(lambda_init as orbil_chain_options takes it, optimize's keywords)"""
    kw = dict(SCENES, **EXTRA)[name][3]
    return (-1.0 if "forced_lambda_init" in kw else kw.get("user_lambda_init", 0.0)), kw


def run(name, be):
    r = il.optimize(be, ITERATIONS, **dict(SCENES, **EXTRA)[name][3])
    return dict(rounds=[r], estimate=be.estimate(), refused=be.refused)


def model_backend(name, noise=None):
    return il.ModelPose(scene(name), visual=False, noise=noise)


def model_run(name):
    if name not in _runs:
        _runs[name] = run(name, model_backend(name))
    return _runs[name]


def start_linearization(name):
    """the linearisation of a scene at its start: what the staged solve is tested on"""
    sc = scene(name)
    return vm.inertial_linearize(sc, sc["graph"])
