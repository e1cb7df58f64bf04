"""The stopping rule of one VHEM EM trial as one shared function
(csrc/vhem_em_trial_ctrl.h: every wave of the batched-trials kernel runs it on the
device), checked on the CPU through its host build (tests/vhememcheck) against a
transcription of the decision lines of vhem.hem_h3m_c_trials on hand-made LogL
sequences; and the ``em_engine`` option of vhem.default_hemopt."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_PATH = os.path.join(ROOT, "tests", "vhememcheck", "libvhememcheck.so")

CONTINUE, STOP, FALLBACK = 0, 1, 2


class Ctrl(ctypes.Structure):  # csrc/vhem_em_trial_ctrl.h TrialCtrl
    _fields_ = [("num_iter", ctypes.c_int), ("done", ctypes.c_int), ("fallback", ctypes.c_int),
                ("stop_iter", ctypes.c_int), ("fb_iter", ctypes.c_int), ("pad_", ctypes.c_int),
                ("LogL", ctypes.c_double)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(CHECK_PATH):
        subprocess.run(["make", "-C", ROOT, "vhememcheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(CHECK_PATH)
    cp = ctypes.POINTER(Ctrl)
    lib.vhem_trial_ctrl_size.restype = ctypes.c_int
    lib.vhem_trial_ctrl_init.argtypes = [cp]
    lib.vhem_trial_ctrl_init.restype = None
    lib.vhem_trial_ctrl_slots.argtypes = [ctypes.c_int]
    lib.vhem_trial_ctrl_slots.restype = ctypes.c_int
    for name in ("vhem_trial_ctrl_ends", "vhem_trial_ctrl_decide"):
        fn = getattr(lib, name)
        fn.argtypes = [cp, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double]
        fn.restype = ctypes.c_int
    lib.vhem_trial_ctrl_record.argtypes = [cp, ctypes.c_int, ctypes.c_double, ctypes.c_int]
    lib.vhem_trial_ctrl_record.restype = ctypes.c_int
    assert lib.vhem_trial_ctrl_size() == ctypes.sizeof(Ctrl)
    return lib


def _python_loop(LLs, max_iter, min_iter, termvalue):
    """vhem.hem_h3m_c_trials lines 251-267 for one trial, fed its log-likelihoods."""
    LogL, LogLs, num_iter = -np.inf, [], 0
    for steps, new_LL in enumerate(LLs, 1):
        new_LL = float(new_LL)
        old_LL = LogL
        LogL = new_LL
        LogLs.append(new_LL)
        with np.errstate(invalid="ignore", divide="ignore"):
            change = (np.float64(new_LL) - old_LL) / abs(np.float64(old_LL)) if num_iter > 1 else np.inf
        stop = bool(change < termvalue) or num_iter > max_iter
        if stop and num_iter >= min_iter:
            return dict(num_iter=num_iter, LogL=LogL, LogLs=LogLs, steps=steps)
        num_iter += 1
    raise AssertionError("the sequence ended before the trial stopped")


def _ctrl_loop(lib, LLs, max_iter, min_iter, termvalue):
    c = Ctrl()
    lib.vhem_trial_ctrl_init(ctypes.byref(c))
    assert (c.num_iter, c.done, c.fallback, c.stop_iter, c.fb_iter) == (0, 0, 0, -1, -1)
    assert c.LogL == -np.inf
    slots = lib.vhem_trial_ctrl_slots(max_iter)
    LogLs = np.full(slots, -7.0)
    steps = 0
    for j, L in enumerate(LLs):
        ends = lib.vhem_trial_ctrl_ends(ctypes.byref(c), L, max_iter, min_iter, termvalue)
        before = c.num_iter
        slot = lib.vhem_trial_ctrl_record(ctypes.byref(c), STOP if ends else CONTINUE, L, j)
        assert slot == j == before            # E-step number e has num_iter == e
        assert 0 <= slot < slots
        LogLs[slot] = L
        steps += 1
        if ends:
            # at a stop nothing is accepted: num_iter is the count before the increment
            assert c.done == 1 and c.stop_iter == j and c.num_iter == before and c.fallback == 0
            break
        assert c.done == 0 and c.num_iter == before + 1
    else:
        raise AssertionError("the sequence ended before the trial stopped")
    return dict(num_iter=c.num_iter, LogL=c.LogL, LogLs=list(LogLs[:steps]), steps=steps,
                untouched=LogLs[steps:])


def _same(a, b):
    return (a == b) or (np.isnan(a) and np.isnan(b))


def _check(lib, LLs, max_iter, min_iter=1, termvalue=1e-5):
    want = _python_loop(LLs, max_iter, min_iter, termvalue)
    got = _ctrl_loop(lib, LLs, max_iter, min_iter, termvalue)
    assert got["num_iter"] == want["num_iter"] and got["steps"] == want["steps"]
    assert _same(got["LogL"], want["LogL"])
    assert len(got["LogLs"]) == len(want["LogLs"])
    assert all(_same(x, y) for x, y in zip(got["LogLs"], want["LogLs"]))
    assert np.all(got["untouched"] == -7.0)
    assert got["steps"] <= max_iter + 2
    return got


def test_no_stop_at_num_iter_0_and_1(lib):
    # whatever the values: falling, equal, rising, not finite
    for seq in ([-5.0, -50.0, -500.0], [-5.0, -5.0, -5.0], [-5.0, 1e300, -4.0],
                [np.nan, -3.0, -3.0], [0.5, 0.25, 0.125]):
        got = _check(lib, seq, max_iter=20)
        assert got["num_iter"] == 2 and got["steps"] == 3
    # min_iter 0 changes nothing: change is +inf while num_iter <= 1
    assert _check(lib, [-5.0, -5.0, -5.0], max_iter=20, min_iter=0)["num_iter"] == 2


def test_change_equal_to_termvalue_does_not_stop(lib):
    # old = -64, new = -63: (new - old) / |old| = 1 / 64 exactly
    term = 1.0 / 64.0
    got = _check(lib, [-100.0, -64.0, -63.0, -62.99], max_iter=20, termvalue=term)
    assert got["steps"] == 4                      # the third E-step did not stop (strict <)
    # the change one ulp below the bar stops (the bar moved: 1 / 64 is the change itself)
    got = _check(lib, [-100.0, -64.0, -63.0], max_iter=20, termvalue=np.nextafter(term, 1.0))
    assert got["steps"] == 3
    got = _check(lib, [-100.0, -64.0, -63.0, -62.99], max_iter=20, termvalue=np.nextafter(term, 0.0))
    assert got["steps"] == 4
    # ... and where the change itself can move by one ulp: old = -1, termvalue = 1,
    # new = 0 gives 1 exactly, new = -2^-53 the double below 1
    for new, steps in ((0.0, 4), (-2.0 ** -53, 3)):
        assert (new - -1.0) / 1.0 == (1.0 if steps == 4 else np.nextafter(1.0, 0.0))
        got = _check(lib, [-5.0, -1.0, new, -1.0][:steps], max_iter=20, termvalue=1.0)
        assert got["steps"] == steps


def test_falling_likelihood_stops(lib):
    got = _check(lib, [-100.0, -90.0, -95.0], max_iter=20)
    assert got["num_iter"] == 2 and got["LogL"] == -95.0


def test_nan_from_the_start_runs_to_max_iter_plus_1(lib):
    for max_iter in (0, 1, 3, 7):
        got = _check(lib, [np.nan] * (max_iter + 2), max_iter=max_iter)
        assert got["num_iter"] == max_iter + 1 and got["steps"] == max_iter + 2


def test_minus_inf_then_finite(lib):
    # old_LL = -inf at num_iter 2: change = inf / inf = NaN, no stop; then it converges
    got = _check(lib, [-10.0, -np.inf, -9.0, -9.0], max_iter=20)
    assert got["steps"] == 4
    got = _check(lib, [-np.inf, -10.0, -9.0, -9.0], max_iter=20)
    assert got["steps"] == 4 and got["num_iter"] == 3


def test_minus_inf_twice(lib):
    # (-inf) - (-inf) = NaN: never below termvalue
    got = _check(lib, [-np.inf, -np.inf, -np.inf, -np.inf, -10.0, -10.0], max_iter=20)
    assert got["steps"] == 6
    got = _check(lib, [-np.inf] * 5, max_iter=3)
    assert got["num_iter"] == 4


def test_min_iter_delays_the_stop(lib):
    seq = [-100.0, -90.0, -89.99999999, -89.99999999, -89.99999999, -89.99999999]
    assert _check(lib, seq[:3], max_iter=20, min_iter=1)["num_iter"] == 2
    assert _check(lib, seq[:4], max_iter=20, min_iter=3)["num_iter"] == 3
    assert _check(lib, seq, max_iter=20, min_iter=5)["num_iter"] == 5


def test_max_iter_0(lib):
    got = _check(lib, [-100.0, -50.0], max_iter=0)
    assert got["num_iter"] == 1 and got["steps"] == 2
    assert lib.vhem_trial_ctrl_slots(0) == 2


def test_logls_slot_count(lib):
    # termvalue 0 on a rising sequence: every one of the max_iter + 2 slots is used
    for max_iter in (0, 1, 3, 6):
        assert lib.vhem_trial_ctrl_slots(max_iter) == max_iter + 2
        seq = [-100.0 + 3.0 * q for q in range(max_iter + 2)]
        got = _check(lib, seq, max_iter=max_iter, termvalue=0.0)
        assert got["steps"] == max_iter + 2 and len(got["untouched"]) == 0


def test_random_sequences_follow_the_transcription(lib):
    rng = np.random.default_rng(5)
    for _ in range(200):
        max_iter = int(rng.integers(0, 8))
        min_iter = int(rng.integers(0, max_iter + 2))
        seq = -100.0 + np.cumsum(rng.choice([2.0, 1e-3, 1e-9, 0.0, -1e-3], size=max_iter + 2))
        seq = [float(x) for x in seq]
        if rng.random() < 0.2:
            seq[int(rng.integers(0, len(seq)))] = float(rng.choice([np.nan, -np.inf, np.inf]))
        _check(lib, seq, max_iter=max_iter, min_iter=min_iter, termvalue=float(rng.choice([0.0, 1e-5, 1e-2])))


def test_device_decision_freezes_a_non_finite_likelihood(lib):
    c = Ctrl()
    lib.vhem_trial_ctrl_init(ctypes.byref(c))
    for bad in (np.nan, np.inf, -np.inf):
        assert lib.vhem_trial_ctrl_decide(ctypes.byref(c), bad, 5, 1, 1e-5) == FALLBACK
    assert lib.vhem_trial_ctrl_decide(ctypes.byref(c), -3.0, 5, 1, 1e-5) == CONTINUE
    assert lib.vhem_trial_ctrl_record(ctypes.byref(c), FALLBACK, np.nan, 4) == 0
    assert (c.done, c.fallback, c.fb_iter, c.stop_iter, c.num_iter) == (1, 1, 4, -1, 0)
    # for finite values the decision is the rule
    c = Ctrl()
    lib.vhem_trial_ctrl_init(ctypes.byref(c))
    for j, L in enumerate([-100.0, -90.0, -95.0]):
        ends = lib.vhem_trial_ctrl_ends(ctypes.byref(c), L, 20, 1, 1e-5)
        what = lib.vhem_trial_ctrl_decide(ctypes.byref(c), L, 20, 1, 1e-5)
        assert what == (STOP if ends else CONTINUE)
        lib.vhem_trial_ctrl_record(ctypes.byref(c), what, L, j)
    assert c.done == 1 and c.stop_iter == 2


# ---- options (both fail without the feature: the field is unknown) ----
def test_default_hemopt_em_engine():
    from vbhem_amd import vhem
    assert vhem.default_hemopt(2, 2, seed=1)["em_engine"] == "host"
    assert vhem.default_hemopt(2, 2, seed=1, em_engine="device")["em_engine"] == "device"


def test_default_hemopt_rejects_unknown_em_engine():
    from vbhem_amd import vhem
    with pytest.raises(ValueError, match="'host' or 'device'"):
        vhem.default_hemopt(2, 2, seed=1, em_engine="gpu")
