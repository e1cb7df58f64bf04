"""The device-side trials loop with per-trial hyperparameters, a mask and the bound's
derivatives on the device (vbhem_em_run_trials_hyp: csrc/vbhem_em_trials.hip,
csrc/vbhem_em_trials_derivs.hip; native_em.run_trials(opts=, active=, calc_deriv=)), the
batched hyperparameter learner on it (hyp.vbhem_h3m_c_hyp_batch with the device evaluator)
and the clustering's hyp_engine="device".

The reference of a trial is the single-trial device loop (native_em.run) from the same
posterior under the trial's own options: the same E-step kernels and the same per-(k, s)
arithmetic, so the bounds differ only through the batched E-step's common shift, and the
derivatives through the device's psi_onediv / DPP sums against the host's psi_recur /
serial sums.  The bars are the project's own: equal iteration counts and stability, bounds
at rtol 1e-10, posterior fields within 1e-9, derivatives at rtol 1e-10 / atol 1e-9
(tests/test_hyp.py::test_native_loop_derivatives_match_python_loop).  A stopping decision
can only differ where a tested change |dL / L| lies at minDiff itself: every case asserts
on the reference runs that none lies within 5 % of it.

Every case prints its worst figures before it asserts; the table is in DESIGN.md 4.20.
"""
import numpy as np
import pytest

from cases import make_case
from conftest import rel_err
from hyp_batch_common import trial_opts, trial_posts

DEV = "cuda:0"
POST_FIELDS = ("alpha", "eta", "epsilon", "lam", "v", "m", "W")


def _assert_margin(results, minDiff):
    """No change the stopping rule tests (iterations > 1) lies within 5 % of minDiff."""
    closest = np.inf
    for r, a in enumerate(results):
        L = np.asarray(a.LogLs, dtype=np.float64)
        if L.size > 2:
            ratio = np.abs((L[2:] - L[1:-1]) / L[1:-1]) / minDiff
            closest = min(closest, float(np.min(np.abs(ratio - 1.0))))
            assert not np.any((ratio > 0.95) & (ratio < 1.05)), (r, ratio)
    return closest


def _deriv_err(got, ref):
    """max over the transformed derivatives of |got - ref| / (1e-9 + 1e-10 |ref|): <= 1 is
    np.allclose(rtol=1e-10, atol=1e-9)."""
    w = 0.0
    for k, v in ref.items():
        if k == "raw":
            continue
        g, v = np.atleast_1d(got[k]).astype(float), np.atleast_1d(v).astype(float)
        w = max(w, float(np.max(np.abs(g - v) / (1e-9 + 1e-10 * np.abs(v)))))
    return w


def _compare(name, got, refs, rows, minDiff):
    closest = _assert_margin([refs[r] for r in rows], minDiff)
    wl = wp = wd = 0.0
    for r in rows:
        a, b = got[r], refs[r]
        n = min(len(a.LogLs), len(b.LogLs))
        if n:
            wl = max(wl, float(np.max(np.abs(np.array(a.LogLs[:n]) - np.array(b.LogLs[:n])) /
                                      np.abs(np.array(b.LogLs[:n])))))
        if a.stable and b.stable:
            wp = max(wp, max(rel_err(getattr(a.post, f), getattr(b.post, f)) for f in POST_FIELDS))
            wd = max(wd, _deriv_err(a.dLL, b.dLL))
    print(f"[em_trials_hyp {name}] trials {list(rows)} iters={[refs[r].iters for r in rows]} worst bound rel {wl:.2e} "
          f"posterior rel {wp:.2e} derivative |err| / (1e-9 + 1e-10 |ref|) {wd:.3g}; "
          f"closest |change / minDiff - 1| {closest:.3g}")
    for r in rows:
        a, b = got[r], refs[r]
        assert a.iters == b.iters and a.stable == b.stable, (name, r, a.iters, b.iters, a.stable, b.stable)
        assert len(a.LogLs) == len(b.LogLs) == b.iters
        assert np.allclose(a.LogLs, b.LogLs, rtol=1e-10, atol=0), (name, r)
        assert set(a.dLL) >= {k for k in b.dLL if k != "raw"}
        if not b.stable:
            assert a.LL == b.LL == -np.inf
            assert all(np.all(np.isnan(v)) for k, v in a.dLL.items() if k != "raw")
            continue
        assert a.LL == a.LogLs[-1]
        for f in POST_FIELDS:
            assert rel_err(getattr(a.post, f), getattr(b.post, f)) < 1e-9, (name, r, f)
        for k, v in b.dLL.items():
            if k != "raw":
                assert np.all(np.isfinite(np.atleast_1d(v))), (name, r, k)
                np.testing.assert_allclose(np.atleast_1d(a.dLL[k]), np.atleast_1d(v), rtol=1e-10, atol=1e-9,
                                           err_msg=f"{name} trial {r} {k}")


def _setup(vb, shape, max_iter, minDiff, seed, **over):
    name, N, K, S, Sb, d, cov, T, ragged, R = shape
    cs = make_case(N, K, S, Sb, d, cov, seed=seed, ragged=ragged, tau=T, **over)
    posts = trial_posts(cs, R, seed)
    opts = trial_opts(dict(cs["opt"], max_iter=max_iter, minDiff=minDiff), R, seed)
    bs = vb.BaseSet.from_numpy(cs["base"])
    return cs, posts, opts, bs


def _references(posts, opts, bs, K, S, T, rows):
    from vbhem_amd import native_em
    from vbhem_amd.estep import EStepEngine
    one = EStepEngine(bs, K, S, T, device=DEV)
    return {r: native_em.run(posts[r], one, opts[r], calc_deriv=True) for r in rows}


# (name, N, K, S, Sb, d, cov, T, ragged, R), max_iter, minDiff, seed, option overrides
CASES = [
    (("A", 60, 3, 3, 3, 2, 1, 8, False, 4), 40, 1e-6, 11, {}),
    (("B", 40, 3, 4, 4, 3, 0, 7, True, 4), 40, 1e-6, 11, dict(W0=[0.4, 0.9, 1.3])),
    (("C_S1", 30, 1, 1, 1, 2, 1, 5, False, 6), 40, 1e-6, 2, {}),
    (("C_S3", 30, 1, 3, 3, 2, 1, 5, False, 6), 40, 1e-6, 2, {}),
    (("E", 50, 2, 16, 12, 16, 1, 6, False, 3), 3, 1e-6, 1, dict(W0=list(np.linspace(0.5, 1.5, 16)))),
    (("F", 100, 4, 2, 2, 2, 1, 6, False, 64), 8, 1e-6, 1, {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0][0] for c in CASES])
def test_per_trial_hyperparameters_match_single_trial_runs(vb, case):
    from vbhem_amd import native_em
    from vbhem_amd.estep import EStepEngine
    shape, max_iter, minDiff, seed, over = case
    name, N, K, S, Sb, d, cov, T, ragged, R = shape
    cs, posts, opts, bs = _setup(vb, shape, max_iter, minDiff, seed, **over)
    refs = _references(posts, opts, bs, K, S, T, range(R))
    tr = native_em.run_trials(posts, EStepEngine(bs, R * K, S, T, device=DEV, trials=R), opts[0], opts=opts,
                              calc_deriv=True)
    _compare(name, tr.results, refs, range(R), minDiff)
    # the trials ran under different hyperparameters: their results differ from each other
    a, b = tr.results[0], tr.results[1]
    # (d_logalpha0 and d_logeta0 are 0 for every trial at K = 1, S = 1)
    assert a.LL != b.LL and not np.array_equal(a.dLL["d_loglambda0"], b.dLL["d_loglambda0"])
    assert not np.array_equal(a.dLL["d_m0"], b.dLL["d_m0"])
    if name in ("E", "F"):
        assert all(x.iters == max_iter + 1 for x in tr.results)
    if name == "A":
        assert len({x.iters for x in tr.results}) >= 2      # trials stop at different iterations


@pytest.mark.gpu
def test_mask_and_fates(vb):
    """Case A with slot 1 inactive: the active trials meet the bars, slot 1 comes back as it
    went in, bit for bit, with NaN derivatives.  Then trial 2 unstable from its first bound
    as well (alpha[0] = NaN): its derivatives are NaN and the others are unaffected."""
    from vbhem_amd import native_em
    from vbhem_amd.estep import EStepEngine
    shape = ("A", 60, 3, 3, 3, 2, 1, 8, False, 4)
    name, N, K, S, Sb, d, cov, T, ragged, R = shape
    cs, posts, opts, bs = _setup(vb, shape, 40, 1e-6, 11)
    refs = _references(posts, opts, bs, K, S, T, (0, 2, 3))
    eng = EStepEngine(bs, R * K, S, T, device=DEV, trials=R)
    active = [1, 0, 1, 1]
    tr = native_em.run_trials(posts, eng, opts[0], opts=opts, active=active, calc_deriv=True)
    _compare("A masked", tr.results, refs, (0, 2, 3), 1e-6)

    def frozen(tr):
        assert tr.results[1] is None and np.isnan(tr.LLall[1])
        raw = tr.raw
        assert raw["iters"][1] == 0 and raw["L_final"][1] == -np.inf and raw["stable"][1] == 0
        assert np.all(raw["LogLs"][1] == 0.0) and np.all(np.isnan(raw["dLL"][1]))
        for f in POST_FIELDS:
            np.testing.assert_array_equal(getattr(raw["posts"][1], f),
                                          np.asarray(getattr(posts[1], f), dtype=np.float64), err_msg=f)

    frozen(tr)
    assert tr.best == (0, 2, 3)[int(np.argmax([refs[r].LL for r in (0, 2, 3)]))]
    bad = [p.copy() for p in posts]
    bad[2].alpha = bad[2].alpha.copy()
    bad[2].alpha[0] = np.nan
    tr2 = native_em.run_trials(bad, eng, opts[0], opts=opts, active=active, calc_deriv=True)
    frozen(tr2)
    u = tr2.results[2]
    assert u.iters == 0 and not u.stable and u.LL == -np.inf and u.LogLs == []
    assert all(np.all(np.isnan(v)) for v in u.dLL.values()) and np.all(np.isnan(tr2.raw["dLL"][2]))
    for f in POST_FIELDS:
        np.testing.assert_array_equal(getattr(u.post, f), np.asarray(getattr(bad[2], f), dtype=np.float64))
    _compare("A masked, trial 2 unstable", tr2.results, refs, (0, 3), 1e-6)


# ---- the batched learner ----
HYP_LENGTH = 6


@pytest.fixture(scope="module")
def learner(vb):
    """The batched learner's run that the two tests below share (computed once, not changed)."""
    from vbhem_amd import hyp
    cs = make_case(40, 3, 3, 2, 2, 1, seed=5, tau=10, W0=1.0, m0=[1.5, 1.5])
    opt = dict(cs["opt"], max_iter=60, minDiff=1e-10, learn_hyps=1)
    starts = trial_posts(cs, 3, 5)
    ev = hyp.device_evaluator(cs["bs"], 3, 3, 10, DEV)
    out = hyp.vbhem_h3m_c_hyp_batch(cs["bs"], opt, starts, ev, length=HYP_LENGTH)
    return cs, opt, starts, out


@pytest.mark.gpu
def test_batched_learner_evaluation_replay(vb, learner):
    """Every point the batched learner evaluated, re-evaluated by the single-trial loop
    (native_em.run with calc_deriv): f at rtol 1e-10, g at rtol 1e-10 / atol 1e-9.  With
    minDiff = 1e-10 and max_iter = 60 the stopping rule never decides (asserted: every
    reference run takes 61 iterations)."""
    from vbhem_amd import hyp, native_em
    from vbhem_amd.estep import EStepEngine
    cs, opt, starts, out = learner
    one = EStepEngine(cs["bs"], 3, 3, 10, device=DEV)
    info = hyp.hypinfo(1, opt)
    wf = wg = 0.0
    checks = []
    for q, h in enumerate(out):
        assert h["evaluations"] == len(h["X_evals"]) >= 2
        for X, f, g in zip(h["X_evals"], h["f_evals"], h["g_evals"]):
            o = hyp.set_opt(X, opt, info)
            o, flags = vb.clip_hyps(o, with_flags=True)
            o["hyp_clipped"] = flags
            ref = native_em.run(starts[q], one, o, calc_deriv=True)
            assert ref.iters == 61 and ref.stable, (q, ref.iters)
            gr = np.concatenate([-np.atleast_1d(ref.dLL[i.derivname]).reshape(-1) for i in info])
            wf = max(wf, abs(f + ref.LL) / abs(ref.LL))
            wg = max(wg, float(np.max(np.abs(g - gr) / (1e-9 + 1e-10 * np.abs(gr)))))
            checks.append((q, f, -ref.LL, g, gr))
    print(f"[hyp batch replay] evaluations {[h['evaluations'] for h in out]} line searches "
          f"{[h['line_searches'] for h in out]}: worst f rel {wf:.2e}, g |err| / (1e-9 + 1e-10 |ref|) {wg:.3g}")
    for q, f, fr, g, gr in checks:
        np.testing.assert_allclose(f, fr, rtol=1e-10, atol=0, err_msg=str(q))
        np.testing.assert_allclose(g, gr, rtol=1e-10, atol=1e-9, err_msg=str(q))
    for q, h in enumerate(out):
        ref = native_em.run(starts[q], one, h["vbopt"])
        print(f"[hyp batch replay] slot {q}: start {-h['fX'][0]:.10g} learnt {h['result'].LL:.10g} "
              f"single-trial {ref.LL:.10g}")
        np.testing.assert_allclose(h["result"].LL, ref.LL, rtol=1e-10, atol=0)
        assert h["result"].stable and h["result"].iters == ref.iters
        assert np.all(np.diff(h["fX"]) <= 0)
        # (the final run repeats the evaluation at the optimum in another batch: 1e-10)
        assert h["result"].LL >= -h["fX"][0] - 1e-10 * abs(h["fX"][0])


@pytest.mark.gpu
def test_batched_learner_follows_the_sequential_learner(vb, learner, monkeypatch):
    """Against hyp.vbhem_h3m_c_hyp(loop='native') per start: the same numbers of
    evaluations and line searches, fX and the final bound at rtol 1e-8 (evaluation-level
    deviations are barred at 1e-10 above; on the CPU, noise of 1e-13 on every f and g left
    the counts equal and moved fX by at most 1.1e-11 -- about 100 x -- and the optimiser's X
    by up to 4e-7, so X is printed, not asserted; the final bound stands for it)."""
    from vbhem_amd import hyp, native_em
    from vbhem_amd.estep import EStepEngine
    cs, opt, starts, out = learner
    one = EStepEngine(cs["bs"], 3, 3, 10, device=DEV)
    seen = []
    real = native_em.run

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(-r.LL)
        return r

    monkeypatch.setattr(native_em, "run", spy)
    seq = []
    for P in starts:
        del seen[:]
        h = hyp.vbhem_h3m_c_hyp(cs["bs"], opt, P, one, length=HYP_LENGTH, loop="native")
        seq.append((h, list(seen[:-1])))                   # the last call is the final EM
    monkeypatch.undo()
    for q, ((b, fs), a) in enumerate(zip(seq, out)):
        n = min(len(fs), len(a["f_evals"]))
        rel = np.abs(np.array(a["f_evals"][:n]) - np.array(fs[:n])) / np.abs(np.array(fs[:n]))
        fork = np.flatnonzero(rel > 1e-8)
        print(f"[hyp batch vs sequential] slot {q}: evaluations {a['evaluations']} / {b['evaluations']}, line "
              f"searches {a['line_searches']} / {b['line_searches']}, worst f rel over the common evaluations "
              f"{float(rel.max()):.2e}, max |X - X_seq| {float(np.max(np.abs(a['opt_transhyp'] - b['opt_transhyp']))):.2e}")
        if fork.size:
            i = int(fork[0])
            print(f"  first differing evaluation {i}: f {a['f_evals'][i]!r} against {fs[i]!r}, X {a['X_evals'][i]}")
    for q, ((b, fs), a) in enumerate(zip(seq, out)):
        assert a["evaluations"] == b["evaluations"] and a["line_searches"] == b["line_searches"], q
        np.testing.assert_allclose(a["fX"], b["fX"], rtol=1e-8, atol=0, err_msg=str(q))
        np.testing.assert_allclose(a["result"].LL, b["result"].LL, rtol=1e-8, atol=0, err_msg=str(q))


@pytest.mark.gpu
def test_cluster_with_the_device_hyp_engine(vb):
    """cluster.vbhem_h3m_c on the planted HMMs (K = S = 2, 4 'baseem' trials, learn_hyps = 1,
    4 line searches): hyp_engine='device' re-optimises the same trials as 'host' (NaN
    elsewhere), picks the same best trial and labels, bounds at rtol 1e-8."""
    from vbhem_amd import cluster, vhem
    hmms, _ = vhem.planted_hmms(20, seed=3)
    base = vhem.hmms_to_h3m(hmms, "full")
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20, Nv=100,
               seed=1001, trials=4, max_iter=30, minDiff=1e-5, learn_hyps=1, hyp_length=4, initmode="baseem")
    o = vb.default_options(2, 2, 2, **opt)
    host = cluster.vbhem_h3m_c(base, o, DEV)
    dev = cluster.vbhem_h3m_c(base, dict(o, hyp_engine="device"), DEV)
    print("re-optimised bounds host", host["LLall"], "device", dev["LLall"])
    assert np.array_equal(np.isnan(host["LLall"]), np.isnan(dev["LLall"])) and np.isfinite(host["LLall"]).any()
    assert dev["best"] == host["best"] and np.array_equal(dev["label"], host["label"])
    ok = np.isfinite(host["LLall"])
    np.testing.assert_allclose(dev["LLall"][ok], host["LLall"][ok], rtol=1e-8, atol=0)
    assert dev["hyp"] is not None and "X_evals" in dev["hyp"] and "X_evals" not in host["hyp"]
    assert dev["hyp"]["evaluations"] == host["hyp"]["evaluations"]
