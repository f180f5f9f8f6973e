"""g2o's Levenberg-Marquardt trial policy (csrc/orb_lm_policy.h) without a GPU.  tests/cpp/lm_policy.cpp runs the header's four
functions in the loop shape of lm_loop over a script of totals and scales; tests/inertial_loop.py's optimize runs over the same numbers
behind a scripted back-end.  The program is built twice: as it is, where the cube is the host's pow -- Python's ** 3 is the same pow, so
every figure is held to the model as bits --, and with -D__HIP_DEVICE_COMPILE__, where the device loops' x*x*x runs on the CPU: the
decisions, rho, temp and scale are equal as bits and lambda stays within 2 ulp per accepted trial, the one extra rounding of the cube.
A NaN is held to be a NaN: the text between the program and the test does not carry its payload.  Then the "written once" rule of the
policy, by text: the three sources that run it include the header, call it, and have none of its arithmetic themselves -- but for
k_pose_optimize, the one loop that keeps its copy."""
import math
import os
import re
import struct
import subprocess

import pytest

import inertial_loop as il
from resource_checks import ROOT, defines_itself, source

INF, NAN, DBL_MAX = float("inf"), float("nan"), il.DBL_MAX
F = {k: i for i, k in enumerate(il.FIELDS)}


def _script(lam, iterations, its, max_trials=10, lower=il.LOWER, upper=il.UPPER):
    """its: per iteration (current, [(ok, ti, tv, scale_pose, scale_points), ...]).  The program reads them as one stream, so only the LAST
    iteration may offer more trials than the policy reads: there they show that the loop stopped of itself"""
    return dict(lam=lam, iterations=iterations, its=its, max_trials=max_trials, lower=lower, upper=upper)


def _trial(current, rho, scale=50.0):
    """an evaluated trial whose rho is about `rho`: the total at the trial point, on the inertial side, and computeScale, on the pose side"""
    return (1, current - rho * scale, 0.0, scale, 0.0)


# against a current of 100: rho = -1.5; totals nobody reads and, as the step of a refused solve is zero, computeScale = 0
REJECT, REFUSED = (1, 150.0, 25.0, 30.0, 20.0), (0, 1.0, 1.0, 0.0, 0.0)
# current 100, total 54.5, computeScale 50: rho = 0.90998..., alpha = 0.448... is not clamped, and pow(x, 3) and x*x*x differ in the last
# bit (0x1.1a43487382114p-1 and ...115p-1; found on the CPU and fixed here)
BAND = (1, 50.0, 4.5, 30.0, 20.0)
# name -> (script, the decisions of the model's trace, iterations run): every path of the policy
SCRIPTS = {
    "clamped by lower": (_script(1.0, 1, [(100.0, [_trial(100.0, 1.0)])]), "a", 1),
    "clamped by upper": (_script(1.0, 1, [(100.0, [_trial(100.0, 0.1)])]), "a", 1),
    "in the band": (_script(1.0, 2, [(100.0, [BAND]), (54.5, [_trial(54.5, 0.9)])]), "aa", 2),
    "rejected, then accepted": (_script(1.0, 2, [(100.0, [REJECT, REJECT, BAND]), (54.5, [(1, 60.0, 0.0, 50.0, 0.0), _trial(54.5, 0.5)])]), "rrara", 2),
    "a refused solve": (_script(1.0, 1, [(100.0, [REFUSED, BAND])]), "ra", 1),
    "max_trials rejections": (_script(1.0, 3, [(100.0, [REJECT] * 4)], max_trials=3), "rrr", 1),
    "rho is zero": (_script(1.0, 3, [(100.0, [(1, 60.0, 40.0, 50.0, 0.0), BAND])]), "r", 1),
    "a total that is not finite": (_script(1.0, 2, [(100.0, [(1, NAN, 1.0, 50.0, 0.0)]), (100.0, [BAND])]), "ra", 2),
    "an infinite total": (_script(1.0, 1, [(100.0, [(1, INF, 1.0, 50.0, 0.0), BAND])]), "ra", 1),
    "lambda overflows": (_script(1e300, 3, [(100.0, [REJECT] * 10)]), "r" * 7, 1),
    "other bounds": (_script(1.0, 3, [(100.0, [_trial(100.0, 1.0)]), (50.0, [_trial(50.0, 0.868, 20.0)]), (32.0, [_trial(32.0, 0.944, 20.0)])], lower=0.25, upper=0.5), "aaa", 3),
}


class Scripted:
    """a back-end of inertial_loop.optimize that hands out a script's numbers in their order"""

    def __init__(self, sc):
        self.its, self.trials = iter(sc["its"]), None

    def linearize(self):
        current, trials = next(self.its)
        self.trials = iter(trials)
        return current

    def trial(self, lam):
        ok, ti, tv, scale_pose, scale_points = next(self.trials)
        self.t = (ti, tv)
        return bool(ok), scale_pose, scale_points

    def totals(self):
        return self.t

    def accept(self):
        pass

    reject = accept


def _model(sc):
    return il.optimize(Scripted(sc), sc["iterations"], user_lambda_init=sc["lam"], max_trials=sc["max_trials"], lower=sc["lower"], upper=sc["upper"])


def _text(sc):
    words = [sc["lam"].hex(), str(sc["max_trials"]), str(sc["iterations"]), sc["lower"].hex(), sc["upper"].hex()]
    for current, trials in sc["its"]:
        words.append(current.hex())
        for ok, *reals in trials:
            words += [str(ok)] + [float(v).hex() for v in reals]
    return " ".join(words)


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    """flavour -> run(script) -> (the rows, lambda, iterations, trials); "host": the header as the host compiler sees it, "device": its
    device branch on the CPU"""
    out = {}
    for flavour, flags in (("host", []), ("device", ["-D__HIP_DEVICE_COMPILE__"])):
        exe = str(tmp_path_factory.mktemp("lm_policy") / flavour)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "monoorbslam3_amd", "csrc")] + flags +
                              [os.path.join(ROOT, "tests", "cpp", "lm_policy.cpp"), "-o", exe])

        def run(sc, exe=exe):
            lines = subprocess.run([exe], input=_text(sc), text=True, capture_output=True, check=True).stdout.splitlines()
            end = lines[-1].split()
            assert end[0] == "end" and len(end) == 4, lines[-1]
            return [[float.fromhex(w) for w in ln.split()] for ln in lines[:-1]], float.fromhex(end[1]), int(end[2]), int(end[3])
        out[flavour] = run
    return out


def _same(a, b):
    a, b = float(a), float(b)
    return (math.isnan(a) and math.isnan(b)) or struct.pack("<d", a) == struct.pack("<d", b)


def _ulps(a, b):
    return abs(a - b) / math.ulp(b)


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_the_header_is_the_model_loop(policy, name):
    sc, decisions, its = SCRIPTS[name]
    want = _model(sc)
    assert il.decisions([want]) == [decisions] and want["iterations"] == its, (il.decisions([want]), want["iterations"])
    # the host's cube: every figure as bits
    rows, lam, n_its, n_trials = policy["host"](sc)
    assert (n_its, n_trials) == (its, len(decisions)) and len(rows) == n_trials and _same(lam, want["lam"]), (n_its, n_trials, lam.hex(), want["lam"].hex())
    for row, t in zip(rows, want["trace"]):
        assert len(row) == len(il.FIELDS)
        for k, (got, ref) in enumerate(zip(row, t)):
            assert _same(got, ref), (il.FIELDS[k], got, ref)
    # the device's cube: the decisions and what they are taken from as bits; lambda within the cube's extra rounding
    rows, lam, n_its, n_trials = policy["device"](sc)
    assert (n_its, n_trials) == (its, len(decisions)) and len(rows) == n_trials
    accepted = 0
    for row, t in zip(rows, want["trace"]):
        for k, (got, ref) in enumerate(zip(row, t)):
            if k != F["lam"]:
                assert _same(got, ref), (il.FIELDS[k], got, ref)
        print(name, "trial", row[:2], "lambda", row[F["lam"]].hex(), "model", t[F["lam"]].hex(), "accepted before", accepted)
        assert _same(row[F["lam"]], t[F["lam"]]) if accepted == 0 else _ulps(row[F["lam"]], t[F["lam"]]) <= 2 * accepted
        accepted += bool(t[F["accepted"]])
    assert _same(lam, want["lam"]) if accepted == 0 or not math.isfinite(want["lam"]) else _ulps(lam, want["lam"]) <= 2 * accepted


def test_each_script_takes_the_path_it_is_named_for():
    """the model's trace, by its figures"""
    run = {name: _model(sc) for name, (sc, _, _) in SCRIPTS.items()}
    tr = {name: r["trace"] for name, r in run.items()}

    def alpha(t):
        return 1.0 - (2 * t[F["rho"]] - 1) ** 3
    t = tr["clamped by lower"][0]
    assert alpha(t) < il.LOWER and run["clamped by lower"]["lam"] == 1.0 * il.LOWER
    t = tr["clamped by upper"][0]
    assert 0 < t[F["rho"]] < 0.2 and alpha(t) > il.UPPER and run["clamped by upper"]["lam"] == 1.0 * il.UPPER
    a, b = tr["in the band"]
    assert il.LOWER < alpha(a) < il.UPPER and il.LOWER < alpha(b) < il.UPPER and b[F["lam"]] == 1.0 * alpha(a) and b[F["current"]] == a[F["temp"]]
    # nu doubles with every rejection and goes back to 2 with an accepted trial: 1, 2, 8, then alpha, then twice that
    r = tr["rejected, then accepted"]
    assert [t[F["trial"]] for t in r] == [0, 1, 2, 0, 1] and [t[F["iteration"]] for t in r] == [0, 0, 0, 1, 1]
    assert [t[F["lam"]] for t in r[:3]] == [1.0, 2.0, 8.0] and r[3][F["lam"]] == 8.0 * alpha(r[2]) and r[4][F["lam"]] == 2.0 * r[3][F["lam"]]
    t = tr["a refused solve"][0]
    assert not t[F["ok"]] and t[F["temp"]] == DBL_MAX and t[F["rho"]] == -INF and tr["a refused solve"][1][F["lam"]] == 2.0
    assert len(tr["max_trials rejections"]) == 3 and run["max_trials rejections"]["iterations"] == 1 < 3      # Terminate on qmax
    assert run["max_trials rejections"]["lam"] == 1.0 * 2 * 4 * 8
    t, = tr["rho is zero"]
    assert t[F["rho"]] == 0 and t[F["temp"]] == t[F["current"]] and not t[F["accepted"]] and run["rho is zero"]["iterations"] == 1 < 3
    t = tr["a total that is not finite"][0]
    assert math.isnan(t[F["rho"]]) and not t[F["accepted"]] and [x[F["iteration"]] for x in tr["a total that is not finite"]] == [0, 1]
    t = tr["an infinite total"][0]
    assert t[F["temp"]] == INF and t[F["rho"]] == -INF and tr["an infinite total"][1][F["trial"]] == 1
    # 1e300 * 2 * 4 * ... : the seventh rejection leaves the loop on an infinite lambda; it is not counted, and Terminate fires
    r = run["lambda overflows"]
    assert len(r["trace"]) == 7 < 10 and r["lam"] == INF and r["iterations"] == 1 < 3 and r["trace"][-1][F["trial"]] == 6
    assert math.isfinite(r["trace"][-1][F["lam"]])
    a, b, c = tr["other bounds"]
    # each of the three is decided otherwise under g2o's bounds: 1/4 not 1/3, 1/2 where 0.60 would have stood, 0.30 where 1/3 would have
    assert alpha(a) < 0.25 and b[F["lam"]] == 0.25 and 0.5 < alpha(b) < il.UPPER and c[F["lam"]] == 0.125 and 0.25 < alpha(c) < il.LOWER
    assert run["other bounds"]["lam"] == 0.125 * alpha(c)


def test_the_two_cubes_are_different_code(policy):
    """on BAND's rho pow and x*x*x differ in the last bit, alpha is not clamped, and the two builds leave lambdas that differ"""
    sc = SCRIPTS["in the band"][0]
    t = _model(sc)["trace"][0]
    x = 2 * t[F["rho"]] - 1
    assert t[F["rho"]].hex() == "0x1.d1e92271097f6p-1" and (x ** 3).hex() == "0x1.1a43487382114p-1" and (x * x * x).hex() == "0x1.1a43487382115p-1"
    host, device = policy["host"](sc)[0][1][F["lam"]], policy["device"](sc)[0][1][F["lam"]]
    assert host == 1.0 - x ** 3 and device == 1.0 - x * x * x and host != device and _ulps(device, host) <= 2


# ---- written once, by text ---------------------------------------------------------------------------------------------------------------
USERS = ("orbba.hip", "orbvi_loop.hip", "orbwl.hip")
COPY = ("ni *= 2", "2 * rho - 1", "1e-3")


def _body(text, head):
    """(the body of the function whose definition starts with `head`, the source without it): from the "{" at the start of a line
    behind `head` to the first "}" at the start of a line"""
    at = text.index(head)
    a = text.index("\n{\n", at)
    b = text.index("\n}\n", a) + 3
    return text[a:b], text[:a] + text[b:]


def test_the_policy_is_written_once():
    """orbba.hip (lm_loop), orbvi_loop.hip (k_vi_pose_loop) and orbwl.hip (k_vwl_decide) include the header and call its trial, loop test
    and Terminate; none has the damping update, the cube or computeScale's 1e-3 of its own; the trace row is written in one place.
    k_pose_optimize (orbba.hip) is the one loop that keeps a copy -- with the header's calls it kept its registers and its bytes and
    measured 1.5 to 3.5 % slower on an MI355X (profiles/lm_policy_shared.txt) --, so its body is set aside here, and it is
    held to BE that copy: whoever moves it takes this exception out"""
    policy = source("orb_lm_policy.h")
    for src in USERS:
        text = source(src)
        if src == "orbba.hip":
            kernel, text = _body(text, "void k_pose_optimize(")
            kernel = re.sub(r"//[^\n]*", "", kernel)
            assert all(word in kernel for word in COPY) and "lm_policy_" not in kernel
            loop = re.sub(r"//[^\n]*", "", _body(text, "\nint lm_loop(")[0])
            for fn in ("lm_policy_iteration", "lm_policy_trial", "lm_policy_again", "lm_policy_terminate"):
                assert re.search(r"\b%s\(" % fn, loop), fn
            assert "LmPolicy p = {0.0, 2.0, 0.0, 0.0, 0, o.lower, o.upper}" in loop                    # orbba_lm_options' bounds
        code = re.sub(r"//[^\n]*", "", text)
        assert '#include "orb_lm_policy.h"' in text, src
        for fn in ("lm_policy_trial", "lm_policy_again", "lm_policy_terminate"):
            assert re.search(r"\b%s\(" % fn, code) and not defines_itself(text, fn), (src, fn)
        for word in ("ni * 2", "ni *= 2", "2 * rho - 1", "pow("):
            assert word not in code, (src, word)
        assert not [ln for ln in code.splitlines() if "1e-3" in ln and "scale" in ln], src
    assert len(re.findall(r"^__host__ __device__ __forceinline__ void lm_trace_row\(", policy, re.M)) == 1
    for src in ("orbvi_loop.hip", "orbwl.hip"):
        code = re.sub(r"//[^\n]*", "", source(src))
        assert len(re.findall(r"\blm_trace_row\(", code)) == 1 and not defines_itself(code, "lm_trace_row"), src
        assert not re.search(r"r\[12\]", code), src
    assert re.search(r"static_assert\([^;]*LM_TRACE_ROW == ORBVI_LOOP_TRACE", source("orbvi_loop.hip"))
    assert re.search(r"static_assert\([^;]*ORBWL_TRACE == LM_TRACE_ROW", source("orbwl.hip"))
