"""The stopping rule of one EM trial as one shared function (csrc/vbhem_em_trial_ctrl.h:
the batched-trials kernel runs it on the device), checked on the CPU through its host
build (tests/emtrialscheck) against a transcription of the decision lines of
em.vbhem_h3m_c_trials; and the C ABI / Python surface of the device-side trials loop
(vbhem_em_run_trials) as far as it can be checked without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_PATH = os.path.join(ROOT, "tests", "emtrialscheck", "libemtrialscheck.so")


class Ctrl(ctypes.Structure):  # csrc/vbhem_em_trial_ctrl.h TrialCtrl
    _fields_ = [("it", ctypes.c_int), ("done", ctypes.c_int), ("stable", ctypes.c_int),
                ("cur", ctypes.c_int), ("stop_iter", ctypes.c_int), ("pad_", ctypes.c_int),
                ("lastL", ctypes.c_double), ("L_final", ctypes.c_double)]


@pytest.fixture(scope="module")
def ctrl_lib():
    if not os.path.exists(CHECK_PATH):
        subprocess.run(["make", "-C", ROOT, "emtrialscheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(CHECK_PATH)
    lib.trial_ctrl_size.restype = ctypes.c_int
    lib.trial_ctrl_init.argtypes = [ctypes.POINTER(Ctrl)]
    lib.trial_ctrl_init.restype = None
    lib.trial_ctrl_step.argtypes = [ctypes.POINTER(Ctrl), ctypes.c_double, ctypes.c_int, ctypes.c_double]
    lib.trial_ctrl_step.restype = ctypes.c_int
    lib.emtrialscheck_seq_count.restype = ctypes.c_int
    lib.emtrialscheck_seq_max_len.restype = ctypes.c_int
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    lib.emtrialscheck_seq.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, dp, ip, dp, ip, ip]
    lib.emtrialscheck_seq.restype = ctypes.c_int
    assert lib.trial_ctrl_size() == ctypes.sizeof(Ctrl)
    return lib


def _sequences(lib):
    out = []
    for i in range(lib.emtrialscheck_seq_count()):
        name = ctypes.create_string_buffer(64)
        L = (ctypes.c_double * lib.emtrialscheck_seq_max_len())()
        mi, it, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        md = ctypes.c_double()
        n = lib.emtrialscheck_seq(i, name, 64, L, ctypes.byref(mi), ctypes.byref(md), ctypes.byref(it),
                                  ctypes.byref(st))
        assert n >= 1
        out.append(dict(name=name.value.decode(), L=[L[q] for q in range(n)], max_iter=mi.value,
                        minDiff=md.value, iters=it.value, stable=bool(st.value)))
    return out


def _python_loop(Ls, maxIter, minDiff):
    """The decision lines of em.vbhem_h3m_c_trials (em.py) for one trial, fed its bounds."""
    lastL = -np.finfo(float).max
    it, LogLs, stable, L, flips, steps = 0, [], True, -np.inf, 0, 0
    for Lr in Ls:
        Lr = np.float64(Lr)
        steps += 1
        with np.errstate(all="ignore"):
            stop = (it > 1 and abs((Lr - lastL) / lastL) <= minDiff) or it == maxIter
        if np.isnan(Lr):
            L = -np.inf
            stable = False
            stop = True
        else:
            L = Lr
            flips += 1  # post[r] = host.mstep(...)
            it += 1
            LogLs.append(Lr)
            lastL = Lr
        if stop:
            break
    else:
        raise AssertionError("the sequence ended before the trial stopped")
    return dict(iters=it, LogLs=LogLs, stable=stable, LL=L, flips=flips, steps=steps)


def _ctrl_loop(lib, Ls, maxIter, minDiff):
    c = Ctrl()
    lib.trial_ctrl_init(ctypes.byref(c))
    assert (c.it, c.done, c.stable, c.cur, c.stop_iter) == (0, 0, 1, 0, -1)
    assert c.lastL == -np.finfo(float).max and c.L_final == -np.inf
    LogLs = np.full(maxIter + 1, -7.0)
    flips = steps = 0
    for Lr in Ls:
        cur = c.cur
        slot = lib.trial_ctrl_step(ctypes.byref(c), float(Lr), maxIter, minDiff)
        steps += 1
        if slot >= 0:
            assert slot == steps - 1 and slot <= maxIter
            LogLs[slot] = Lr
            assert c.cur == cur ^ 1  # the M-step is accepted
        else:
            assert np.isnan(Lr) and c.cur == cur
        flips += int(c.cur != cur)
        if c.done:
            assert c.stop_iter == steps - 1
            break
    else:
        raise AssertionError("the sequence ended before the trial stopped")
    assert np.all(LogLs[c.it:] == -7.0)  # nothing recorded past the accepted iterations
    return dict(iters=c.it, LogLs=list(LogLs[:c.it]), stable=bool(c.stable), LL=c.L_final, flips=flips,
                steps=steps, cur=c.cur)


def test_ctrl_step_matches_the_python_loop_on_hand_made_sequences(ctrl_lib):
    seqs = _sequences(ctrl_lib)
    names = {s["name"] for s in seqs}
    assert {"converging", "exact_at_2", "max_iter_0", "max_iter_1", "nan_at_0", "nan_at_3", "huge_first",
            "zero_lastL"} <= names
    for s in seqs:
        want = _python_loop(s["L"], s["max_iter"], s["minDiff"])
        got = _ctrl_loop(ctrl_lib, s["L"], s["max_iter"], s["minDiff"])
        assert want["steps"] == len(s["L"]), s["name"]  # the hand-made outcome: stops at its last bound
        assert (want["iters"], want["stable"]) == (s["iters"], s["stable"]), s["name"]
        for k in ("iters", "stable", "flips", "steps"):
            assert got[k] == want[k], (s["name"], k, got[k], want[k])
        np.testing.assert_array_equal(got["LogLs"], want["LogLs"], err_msg=s["name"])
        assert got["LL"] == want["LL"], s["name"]
        assert got["cur"] == got["iters"] % 2, s["name"]


def test_ctrl_step_it_gt_1_rule(ctrl_lib):
    """A change within minDiff at iteration 1 does not stop the trial; the same at 2 does,
    also when it equals minDiff exactly."""
    s = {q["name"]: q for q in _sequences(ctrl_lib)}["exact_at_2"]
    L = s["L"]
    assert L[1] == L[0] and abs((L[2] - L[1]) / L[1]) == s["minDiff"]
    got = _ctrl_loop(ctrl_lib, L, s["max_iter"], s["minDiff"])
    assert got["iters"] == 3 and got["steps"] == 3


def test_ctrl_step_replays_host_engine_trials(vb, ctrl_lib, monkeypatch):
    """em.vbhem_h3m_c_trials on the oracle stand-in engine (the case of
    test_em_trials_host_logic_cpu): every trial's bounds, replayed through the function,
    stop it at the same iteration with the same record."""
    from oracle_engine import OracleEngine
    from test_trials import _trial_posts
    from vbhem_amd import em, host
    N, K, S, Sb, d, cov, T, R = 24, 3, 3, 3, 2, 1, 6, 3
    cs = make_case(N, K, S, Sb, d, cov, seed=5, tau=T)
    posts = _trial_posts(cs, R, 5)
    opt = dict(cs["opt"], max_iter=15, minDiff=1e-5)
    bs = vb.BaseSet.from_numpy(cs["base"])
    seen = []
    real = host.lower_bound

    def spy(*a, **k):
        L = real(*a, **k)
        seen.append(float(L))
        return L

    monkeypatch.setattr(host, "lower_bound", spy)
    tr = em.vbhem_h3m_c_trials(posts, OracleEngine(bs, R * K, S, T, nthreads=1, trials=R), opt)
    monkeypatch.undo()
    # the loop calls lower_bound for the running trials in order, once per iteration
    # (a stable trial: one call per accepted iteration; an unstable one: one more)
    calls = [a.iters + (0 if a.stable else 1) for a in tr.results]
    per = [[] for _ in range(R)]
    q = 0
    for it in range(max(calls)):
        for r in range(R):
            if it < calls[r]:
                per[r].append(seen[q])
                q += 1
    assert q == len(seen) and len({a.iters for a in tr.results}) >= 1
    for r in range(R):
        a = tr.results[r]
        got = _ctrl_loop(ctrl_lib, per[r], opt["max_iter"], opt["minDiff"])
        assert got["iters"] == a.iters and got["stable"] == a.stable and got["steps"] == len(per[r])
        np.testing.assert_array_equal(got["LogLs"], a.LogLs)
        assert got["LL"] == a.LL


def _base(N, Sb, d, cov=1):
    from vbhem_amd import _capi
    p = 1 << 20
    return _capi.BaseT(N, Sb, d, cov, p, p, p, p, p)


def test_trials_workspace_bytes(capi_lib):
    ws = capi_lib.vbhem_em_trials_workspace_bytes
    assert ws(ctypes.byref(_base(10, 3, 2)), 3, 3, 4, 8) > 0
    assert ws(ctypes.byref(_base(10, 3, 2)), 3, 3, 1, 8) > 0
    assert ws(ctypes.byref(_base(10, 3, 2)), 64, 3, 4, 8) > 0     # R K = 256
    assert ws(ctypes.byref(_base(10, 3, 2)), 65, 3, 4, 8) == 0    # R K = 260
    assert ws(ctypes.byref(_base(10, 3, 17)), 3, 3, 4, 8) == 0    # d = 17
    assert ws(ctypes.byref(_base(10, 3, 2)), 3, 17, 4, 8) == 0    # S = 17
    assert ws(ctypes.byref(_base(10, 4, 2)), 3, 3, 4, 8) == 0     # Sb > S
    assert ws(ctypes.byref(_base(10, 3, 2)), 3, 3, 0, 8) == 0     # R = 0
    assert ws(None, 3, 3, 4, 8) == 0
    # more trials need more room
    assert ws(ctypes.byref(_base(10, 3, 2)), 3, 3, 8, 8) > ws(ctypes.byref(_base(10, 3, 2)), 3, 3, 4, 8)


def test_run_trials_refuses_bad_shapes_and_arguments(vb, capi_lib):
    from vbhem_amd import native_em
    K, S, d, R = 65, 3, 2, 4
    cs = make_case(6, K, S, 3, d, 1, seed=3, tau=4)
    pbs = [native_em._PostBuf(cs["P"], 1) for _ in range(R)]
    ob = native_em._OptBuf(dict(cs["opt"], max_iter=3, minDiff=1e-6))
    arr = (type(pbs[0].t) * R)(*[pb.t for pb in pbs])
    v = ctypes.c_void_p(1 << 20)
    args = lambda base, posts: (ctypes.byref(base), v, R, 4, ctypes.byref(ob.t), posts, v, v, v, v, v, v, v,  # noqa: E731
                                v, ctypes.c_size_t(1 << 40), None)
    rc = capi_lib.vbhem_em_run_trials(*args(_base(6, 3, d), arr))
    assert rc == -2 and b"256" in capi_lib.vbhem_last_error()      # VBHEM_ERR_UNSUPPORTED
    rc = capi_lib.vbhem_em_run_trials(*args(_base(6, 3, d + 1), arr))
    assert rc == -1 and b"covmode" in capi_lib.vbhem_last_error()  # VBHEM_ERR_ARG: d differs
    rc = capi_lib.vbhem_em_run_trials(*args(_base(6, 3, d, cov=0), arr))
    assert rc == -1
    rc = capi_lib.vbhem_em_run_trials(*args(_base(6, 3, d), None))
    assert rc == -1


def test_em_engine_keyword(vb):
    from oracle_engine import OracleEngine
    from test_trials import _trial_posts
    from vbhem_amd import cluster, em
    N, K, S, Sb, d, cov, T, R = 8, 2, 2, 2, 2, 1, 4, 2
    cs = make_case(N, K, S, Sb, d, cov, seed=2, tau=T)
    posts = _trial_posts(cs, R, 2)
    bs = vb.BaseSet.from_numpy(cs["base"])
    eng = OracleEngine(bs, R * K, S, T, nthreads=1, trials=R)
    opt = dict(cs["opt"], max_iter=2, minDiff=1e-6)
    with pytest.raises(ValueError, match="em_engine"):
        em.vbhem_h3m_c_trials(posts, eng, opt, em_engine="nope")
    with pytest.raises(ValueError, match="EStepEngine"):
        em.vbhem_h3m_c_trials(posts, eng, opt, em_engine="device")
    with pytest.raises(ValueError, match="allreduce"):
        em.vbhem_h3m_c_trials(posts, eng, opt, em_engine="device", allreduce=lambda t: None)
    with pytest.raises(ValueError, match="em_engine"):
        cluster.vbhem_h3m_c(bs, dict(opt, K=K, S=S, trials=2, seed=1, em_engine="gpu"), device="cpu")
    # the default is the host engine, and naming it changes nothing
    a = em.vbhem_h3m_c_trials(posts, eng, opt)
    b = em.vbhem_h3m_c_trials(posts, eng, opt, em_engine="host")
    np.testing.assert_array_equal(a.LLall, b.LLall)
