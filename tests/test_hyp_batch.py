"""The batched hyperparameter learner on the CPU: the lockstep minimisers
(hyp.minimize_lockstep) against hyp.minimize alone, bit for bit; the batched learner
(hyp.vbhem_h3m_c_hyp_batch) with the host evaluator on the oracle stand-in engine against
one hyp.vbhem_h3m_c_hyp per start; per-trial options and the mask of the host trials
engine (em.vbhem_h3m_c_trials) against em.vbhem_h3m_c_step_fc; and the clustering's
``hyp_engine`` option.  The oracle engine computes each trial on its own, so batching
cannot change a bit: every comparison here is exact."""
import numpy as np
import pytest

from cases import make_case
from hyp_batch_common import trial_opts, trial_posts
from oracle_engine import OracleEngine

POST_FIELDS = ("alpha", "eta", "epsilon", "lam", "v", "m", "W")


def _rosen(n):
    def F(x):
        f = np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2)
        g = np.zeros_like(x)
        g[:-1] += -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2 * (1 - x[:-1])
        g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
        return float(f), g
    return F, np.linspace(-1.2, 1.0, n)


def _quad(n, seed):
    rng = np.random.default_rng(seed)
    Q = rng.normal(size=(n, n))
    A = Q @ Q.T + n * np.eye(n)
    b = rng.normal(size=n)
    return (lambda x: (float(0.5 * x @ A @ x - b @ x), A @ x - b)), np.zeros(n)


def _nan_region():
    """A quadratic that is NaN beyond x0 > 3: the extrapolation runs into it and bisects."""
    def F(x):
        if x[0] > 3.0:
            return np.nan, np.full(2, np.nan)
        return float((x[0] - 2.9) ** 2 + 0.5 * (x[1] + 1.0) ** 2), np.array([2 * (x[0] - 2.9), x[1] + 1.0])
    return F, np.array([-10.0, 4.0])


@pytest.mark.parametrize("method", ["LBFGS", "BFGS", "CG"])
def test_minimize_lockstep_matches_minimize(vb, method):
    from vbhem_amd.hyp import minimize, minimize_lockstep
    objs = [_rosen(2), _quad(5, 3), _rosen(4), _nan_region(), _quad(3, 8)]
    # (CG on the NaN-region quadratic reaches a gradient of exactly 0 in its 7th line search,
    # where minimize's Polack-Ribiere ratio divides by it: 6 line searches there)
    length = 6 if method == "CG" else 12
    alone, counts, saw_nan = [], [], []
    for F, X0 in objs:
        n = [0, 0]

        def G(x, F=F, n=n):
            n[0] += 1
            f, g = F(x)
            n[1] += int(not np.isfinite(f))
            return f, g

        alone.append(minimize(X0, G, length=length, method=method))
        counts.append(n[0])
        saw_nan.append(n[1])
    assert saw_nan[3] >= 1                                  # the bisect path
    assert len(set(counts)) >= 3                            # the slots finish at different rounds
    rounds, sizes = [0], []

    def Fbatch(req):
        rounds[0] += 1
        sizes.append(len(req))
        return {q: objs[q][0](x) for q, x in req.items()}

    got = minimize_lockstep([X0 for _, X0 in objs], Fbatch, length=length, method=method)
    print(f"[lockstep {method}] evaluations per slot {counts}, rounds {rounds[0]}, slots per round {sizes}")
    assert rounds[0] == max(counts) and sum(sizes) == sum(counts)
    assert sizes == sorted(sizes, reverse=True)             # finished slots drop out
    for q, ((x, fX, i), (xr, fXr, ir)) in enumerate(zip(got, alone)):
        assert np.array_equal(x, xr, equal_nan=True) and np.array_equal(fX, fXr, equal_nan=True) and i == ir, q


def test_minimize_lockstep_errors(vb):
    """An exception as a slot's answer is raised in that slot's objective alone (the line
    search bisects, minimize_new.m:147-155); an error that ends a slot's minimize is raised
    by minimize_lockstep; a Fbatch that raises reaches every slot of the round."""
    from vbhem_amd.hyp import minimize, minimize_lockstep
    F = lambda x: ((x[0] - 1.9) ** 2, np.array([2 * (x[0] - 1.9)]))  # noqa: E731
    calls = []

    def alone(x):
        calls.append(1)
        if len(calls) == 5:
            raise RuntimeError("status -2")
        return F(x)

    ref = minimize(np.array([-10.0]), alone, length=20)
    n = {0: 0, 1: 0}

    def Fbatch(req):
        out = {}
        for q, x in req.items():
            n[q] += 1
            out[q] = RuntimeError("status -2") if (q == 0 and n[q] == 5) else F(x)
        return out

    a, b = minimize_lockstep([np.array([-10.0]), np.array([-10.0])], Fbatch, length=20)
    plain = minimize(np.array([-10.0]), F, length=20)
    assert np.array_equal(a[0], ref[0]) and np.array_equal(a[1], ref[1]) and a[2] == ref[2]
    assert np.array_equal(b[0], plain[0]) and np.array_equal(b[1], plain[1]) and b[2] == plain[2]
    with pytest.raises(RuntimeError, match="first"):        # the first evaluation is not guarded
        minimize_lockstep([np.array([0.0])], lambda req: {0: RuntimeError("first")}, length=3)

    def broken(req):
        raise RuntimeError("whole batch")

    with pytest.raises(RuntimeError, match="whole batch"):
        minimize_lockstep([np.array([0.0]), np.array([1.0])], broken, length=3)


def _exprmt1(vb, N=12):
    return vb.synth_base_set(N, 2, 2, 2, vb.COV_FULL, seed=1002, exprmt1=True)


OPT = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5],
           tau=20, Nv=100, seed=1001, trials=3, max_iter=30, minDiff=1e-5, learn_hyps=0)


def test_hyp_batch_matches_sequential_learner(vb):
    """Three starts on the exprmt1 base (K = S = 2), length 4, host evaluator on the oracle
    engine, against three vbhem_h3m_c_hyp runs: every figure bit-equal."""
    from vbhem_amd import em, hyp
    base = _exprmt1(vb)
    o = vb.default_options(2, 2, 2, **dict(OPT, max_iter=40, minDiff=1e-8, learn_hyps=1))
    one = OracleEngine(base, 2, 2, o["tau"], nthreads=2)
    starts = []
    for seed in (7, 8, 9):
        rb, rg, om = vb.baseem_draws(base, 2, 2, seed=seed)
        starts.append(em.vbhem_h3m_c_step_fc(vb.baseem_init(base, o, rb, rg, om), one, o).post)
    seq = [hyp.vbhem_h3m_c_hyp(base, o, P, one, length=4) for P in starts]
    calls = []
    ev = hyp.host_evaluator(lambda R: OracleEngine(base, R * 2, 2, o["tau"], nthreads=2, trials=R))

    def spy(posts, opts, active, calc_deriv):
        calls.append((list(active), calc_deriv))
        return ev(posts, opts, active, calc_deriv)

    bat = hyp.vbhem_h3m_c_hyp_batch(base, o, starts, spy, length=4)
    evals = [s["evaluations"] for s in seq]
    print(f"[hyp batch cpu] evaluations {evals}: {len(calls) - 1} rounds instead of {sum(evals)} runs; "
          f"fX ends {[float(s['fX'][-1]) for s in seq]}")
    assert len(bat) == 3 and len(calls) == max(evals) + 1            # + the final EM, one call
    assert calls[-1] == ([True] * 3, False) and all(c[1] for c in calls[:-1])
    assert sum(sum(c[0]) for c in calls[:-1]) == sum(evals)
    for q, (a, b) in enumerate(zip(bat, seq)):
        assert a["evaluations"] == b["evaluations"] and a["line_searches"] == b["line_searches"], q
        assert np.array_equal(a["fX"], b["fX"]) and np.array_equal(a["opt_transhyp"], b["opt_transhyp"]), q
        assert a["result"].LL == b["result"].LL and a["opt_L"] == b["opt_L"], q
        assert a["result"].LogLs == b["result"].LogLs
        for f in POST_FIELDS:
            np.testing.assert_array_equal(getattr(a["result"].post, f), getattr(b["result"].post, f))
        assert len(a["X_evals"]) == len(a["f_evals"]) == len(a["g_evals"]) == a["evaluations"]
        assert a["f_evals"][0] == a["fX"][0] and set(a["fX"]) <= set(a["f_evals"])
        for name in ("alpha0", "eta0", "epsilon0", "lambda0", "v0"):
            assert a["vbopt"][name] == b["vbopt"][name]


def test_host_trials_engine_with_per_trial_options_and_mask(vb):
    """em.vbhem_h3m_c_trials(opts=..., active=...) on the oracle engine: every active trial
    equals vbhem_h3m_c_step_fc with its own options bit for bit, derivatives included; an
    inactive slot is None; the defaults are today's call."""
    from vbhem_amd import em
    N, K, S, Sb, d, cov, T, R = 24, 3, 3, 3, 2, 1, 6, 4
    cs = make_case(N, K, S, Sb, d, cov, seed=5, tau=T)
    posts = trial_posts(cs, R, 5)
    opts = trial_opts(dict(cs["opt"], max_iter=15, minDiff=1e-5, calc_LLderiv=1), R, 5)
    bs = vb.BaseSet.from_numpy(cs["base"])
    active = [True, False, True, True]
    tr = em.vbhem_h3m_c_trials(posts, OracleEngine(bs, R * K, S, T, nthreads=1, trials=R), opts[0],
                               opts=opts, active=active)
    assert tr.results[1] is None and np.isnan(tr.LLall[1])
    one = OracleEngine(bs, K, S, T, nthreads=1)
    lls = []
    for r in (0, 2, 3):
        ref = em.vbhem_h3m_c_step_fc(posts[r], one, opts[r])
        got = tr.results[r]
        lls.append(ref.LL)
        assert got.iters == ref.iters and got.stable == ref.stable and got.LogLs == ref.LogLs and got.LL == ref.LL
        for f in POST_FIELDS:
            np.testing.assert_array_equal(getattr(got.post, f), getattr(ref.post, f), err_msg=f)
        assert set(got.dLL) == set(ref.dLL)
        for k in ref.dLL:
            if k != "raw":
                np.testing.assert_array_equal(got.dLL[k], ref.dLL[k], err_msg=k)
    assert len(set(lls)) == 3 and tr.best == (0, 2, 3)[int(np.argmax(lls))]
    # the defaults: the call as it was
    a = em.vbhem_h3m_c_trials(posts, OracleEngine(bs, R * K, S, T, nthreads=1, trials=R), opts[0])
    b = em.vbhem_h3m_c_trials(posts, OracleEngine(bs, R * K, S, T, nthreads=1, trials=R), opts[0],
                              opts=[opts[0]] * R, active=[1] * R)
    np.testing.assert_array_equal(a.LLall, b.LLall)
    assert a.best == b.best and all(x is not None for x in a.results)
    with pytest.raises(ValueError, match="opts"):
        em.vbhem_h3m_c_trials(posts, OracleEngine(bs, R * K, S, T, nthreads=1, trials=R), opts[0], opts=opts[:2])


def test_cluster_hyp_engine_option(vb):
    """With an engine factory (no device engine) hyp_engine='device' is the host loop; a
    value that is neither raises."""
    from vbhem_amd import cluster
    base = _exprmt1(vb, N=10)
    factory = lambda b, K, S, T, trials=1: OracleEngine(b, K, S, T, nthreads=2, trials=trials)  # noqa: E731
    o = vb.default_options(2, 2, 2, **dict(OPT, trials=3, max_iter=8, learn_hyps=1, hyp_length=2))
    a = cluster.vbhem_h3m_c(base, o, engine_factory=factory)
    b = cluster.vbhem_h3m_c(base, dict(o, hyp_engine="host"), engine_factory=factory)
    c = cluster.vbhem_h3m_c(base, dict(o, hyp_engine="device"), engine_factory=factory)
    for x in (b, c):
        np.testing.assert_array_equal(a["LLall"], x["LLall"])
        assert a["best"] == x["best"] and np.array_equal(a["label"], x["label"])
        np.testing.assert_array_equal(a["hyp"]["fX"], x["hyp"]["fX"])
    assert np.isfinite(a["LLall"]).any()
    with pytest.raises(ValueError, match="hyp_engine"):
        cluster.vbhem_h3m_c(base, dict(o, hyp_engine="gpu"), engine_factory=factory)
