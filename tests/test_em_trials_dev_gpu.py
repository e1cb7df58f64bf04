"""The device-side EM of R batched trials (vbhem_em_run_trials: csrc/vbhem_em_trials.hip,
native_em.run_trials, em_engine="device") against the host engine
(em.vbhem_h3m_c_trials as it stands) on the same initial posteriors.

The two engines run the same E-step kernels; the bound, the M-step and the prelude are
numpy on one side and the device kernels' fp64 on the other (Gauss-Jordan against LU,
Stirling lgamma against libm's), so a trial's bounds differ in the last digits (measured:
at most 4.9e-14 relative, posteriors 2.1e-13, hat_Z 4.6e-12 over all cases) and the
bars are those of tests/test_trials.py::test_em_trials_match_separate_runs: equal
iteration counts and stability, bounds at rtol 1e-10, every posterior field within 1e-9,
hat_Z within 1e-8, the same best trial and the same labels.  A stopping decision can only
differ when a tested change |dL / L| lies at minDiff itself: every case asserts, on the host
engine's own trajectory, that none lies within 5 % of it (the seeds are fixed so).

Every case prints its worst figures before it asserts; the table is in DESIGN.md 4.19.
"""
import numpy as np
import pytest
import torch

from cases import make_case
from conftest import hatz_err, rel_err

DEV = "cuda:0"
POST_FIELDS = ("alpha", "eta", "epsilon", "lam", "v", "m", "W")


def _trial_posts(cs, R, seed):
    """R cluster posteriors over the same base set: the case's posterior and R-1
    re-perturbed copies (the recipe of tests/test_trials.py)."""
    posts = [cs["P"].copy()]
    for r in range(1, R):
        P = cs["P"].copy()
        rng = np.random.default_rng(seed * 100 + r)
        P.epsilon = P.epsilon * rng.uniform(0.3, 1.7, P.epsilon.shape)
        P.eta = P.eta * rng.uniform(0.3, 1.7, P.eta.shape)
        P.m = P.m + rng.normal(0.0, 0.5, P.m.shape)
        P.alpha = P.alpha * rng.uniform(0.5, 1.5, P.alpha.shape)
        posts.append(P)
    return posts


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


def _compare(name, host_tr, dev_tr, minDiff):
    """The bars; every trial is compared.  Prints the worst figures before asserting."""
    R = len(host_tr.results)
    assert len(dev_tr.results) == R
    closest = _assert_margin(host_tr.results, minDiff)
    wl = wp = wz = 0.0
    for a, b in zip(dev_tr.results, host_tr.results):
        n = min(len(a.LogLs), len(b.LogLs))
        if n:
            wl = max(wl, float(np.max(np.abs(np.array(a.LogLs[:n]) - np.array(b.LogLs[:n])) /
                                      np.abs(np.array(b.LogLs[:n])))))
        if a.stable and b.stable:
            wp = max(wp, max(rel_err(getattr(a.post, f), getattr(b.post, f)) for f in POST_FIELDS))
            wz = max(wz, hatz_err(a.hatZ.cpu().numpy(), b.hatZ.cpu().numpy()))
    print(f"[em_trials {name}] R={R} iters={[b.iters for b in host_tr.results]} worst bound rel {wl:.2e} "
          f"posterior rel {wp:.2e} hat_Z {wz:.2e}; closest |change / minDiff - 1| {closest:.3g}")
    for r, (a, b) in enumerate(zip(dev_tr.results, host_tr.results)):
        assert a.iters == b.iters and a.stable == b.stable, (name, r, a.iters, b.iters, a.stable, b.stable)
        assert len(a.LogLs) == len(b.LogLs) == b.iters
        assert np.allclose(a.LogLs, b.LogLs, rtol=1e-10, atol=0), (name, r)
        if not b.stable:
            assert a.LL == b.LL == -np.inf and a.label is None and a.point is None
            continue
        assert a.LL == a.LogLs[-1]
        for f in POST_FIELDS:
            assert rel_err(getattr(a.post, f), getattr(b.post, f)) < 1e-9, (name, r, f)
        assert hatz_err(a.hatZ.cpu().numpy(), b.hatZ.cpu().numpy()) < 1e-8, (name, r)
        assert rel_err(a.L_elbo.cpu().numpy(), b.L_elbo.cpu().numpy()) < 1e-9, (name, r)
        assert rel_err(a.Nj, b.Nj) < 1e-9, (name, r)
        assert torch.equal(a.label.cpu(), b.label.cpu()), (name, r)
    assert dev_tr.best == host_tr.best, (name, dev_tr.LLall, host_tr.LLall)


def _both(vb, shape, max_iter, minDiff, seed, mutate=None):
    from vbhem_amd import em
    from vbhem_amd.estep import EStepEngine
    name, N, K, S, Sb, d, cov, T, ragged, R = shape
    cs = make_case(N, K, S, Sb, d, cov, seed=seed, ragged=ragged, tau=T)
    posts = _trial_posts(cs, R, seed)
    if mutate is not None:
        mutate(posts)
    opt = dict(cs["opt"], max_iter=max_iter, minDiff=minDiff)
    bs = vb.BaseSet.from_numpy(cs["base"])
    eng = EStepEngine(bs, R * K, S, T, device=DEV, trials=R)
    host_tr = em.vbhem_h3m_c_trials(posts, eng, opt)
    dev_tr = em.vbhem_h3m_c_trials(posts, EStepEngine(bs, R * K, S, T, device=DEV, trials=R), opt,
                                   em_engine="device")
    return posts, opt, bs, host_tr, dev_tr


# (name, N, K, S, Sb, d, cov, T, ragged, R), max_iter, minDiff, seed
CASES = [
    # K S = 9: blocks of 4 waves straddle the trials; two stopping iterations
    (("A", 60, 3, 3, 3, 2, 1, 8, False, 4), 40, 1e-6, 11),
    # diagonal covariances, ragged bases
    (("B", 40, 3, 4, 4, 3, 0, 7, True, 4), 40, 1e-6, 11),
    # one wave per trial, the S = 1 branch of the statistics, logOmega of one cluster
    (("C_S1", 30, 1, 1, 1, 2, 1, 5, False, 6), 40, 1e-6, 2),
    (("C_S3", 30, 1, 3, 3, 2, 1, 5, False, 6), 40, 1e-6, 2),
    # 128 partials per trial: two strided rounds in the trial's last wave
    (("D", 200, 16, 8, 8, 8, 1, 10, False, 4), 5, 1e-6, 6),
    # the largest d and S
    (("E", 50, 2, 16, 12, 16, 1, 6, False, 3), 3, 1e-6, 1),
    # R K = 256
    (("F", 100, 4, 2, 2, 2, 1, 6, False, 64), 8, 1e-6, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0][0] for c in CASES])
def test_device_engine_matches_host_engine(vb, case):
    shape, max_iter, minDiff, seed = case
    _, _, _, host_tr, dev_tr = _both(vb, shape, max_iter, minDiff, seed)
    _compare(shape[0], host_tr, dev_tr, minDiff)
    if shape[0] == "A":
        assert len({a.iters for a in dev_tr.results}) >= 2  # trials stop at different iterations
    if shape[0] in ("D", "E", "F"):
        assert all(a.iters == max_iter + 1 for a in dev_tr.results)


@pytest.mark.gpu
def test_mixed_fates(vb):
    """Case A with trial 1 unstable from its first bound (alpha[0] = NaN) and max_iter = 9:
    two trials converge at iteration 8, one runs to max_iter.  The NaN trial keeps its
    input, bit for bit; the others meet the bars although the NaN trial's clusters ride
    along in every E-step; every trial's hat_Z is the E-step of its own stopping iteration."""
    from vbhem_amd import em
    from vbhem_amd.estep import EStepEngine

    def nan_alpha(posts):
        posts[1].alpha = posts[1].alpha.copy()
        posts[1].alpha[0] = np.nan

    shape = ("G", 60, 3, 3, 3, 2, 1, 8, False, 4)
    posts, opt, bs, host_tr, dev_tr = _both(vb, shape, 9, 1e-6, 11, nan_alpha)
    _compare("G", host_tr, dev_tr, 1e-6)
    bad = dev_tr.results[1]
    assert bad.iters == 0 and bad.LL == -np.inf and bad.LogLs == [] and not bad.stable
    for f in POST_FIELDS:
        np.testing.assert_array_equal(getattr(bad.post, f), np.asarray(getattr(posts[1], f), dtype=np.float64))
    iters = [a.iters for a in dev_tr.results]
    assert max(iters) == opt["max_iter"] + 1                        # one stops at max_iter
    early = [r for r in (0, 2, 3) if iters[r] < opt["max_iter"] + 1]
    assert early                                                    # another converged before
    # an early trial's latched hat_Z: the E-step of ITS last iteration, which a single run
    # of that trial alone (the host loop, one trial) ends with
    r = early[0]
    K = shape[2]
    one = em.vbhem_h3m_c_step_fc(posts[r], EStepEngine(bs, K, shape[3], shape[7], device=DEV), opt)
    assert one.iters == iters[r]
    assert hatz_err(dev_tr.results[r].hatZ.cpu().numpy(), one.hatZ.cpu().numpy()) < 1e-8
    assert rel_err(dev_tr.results[r].L_elbo.cpu().numpy(), one.L_elbo.cpu().numpy()) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("cov", [1, 0], ids=["full", "diag"])
def test_one_trial_gives_the_single_trial_loops_bits(vb, cov):
    """R = 1: the trials loop runs the arithmetic of the single-trial device loop
    (native_em.run) -- the same bounds, iteration count and posterior, bit for bit; twice on
    one engine gives the same bits, the workspace is reused, and a run from other
    posteriors in between leaves no trace (records and tickets start afresh)."""
    from vbhem_amd import native_em
    from vbhem_amd.estep import EStepEngine
    N, K, S, Sb, d, T = (60, 3, 3, 3, 2, 8) if cov else (40, 3, 4, 4, 3, 7)
    cs = make_case(N, K, S, Sb, d, cov, seed=11, ragged=not cov, tau=T)
    opt = dict(cs["opt"], max_iter=6, minDiff=1e-6)
    bs = vb.BaseSet.from_numpy(cs["base"])
    P, Q = _trial_posts(cs, 2, 11)
    ref = native_em.run(P, EStepEngine(bs, K, S, T, device=DEV), opt)
    eng = EStepEngine(bs, K, S, T, device=DEV, trials=1)
    a = native_em.run_trials([P], eng, opt)
    ws = eng._em_ws
    other = native_em.run_trials([Q], eng, dict(opt, max_iter=3))
    b = native_em.run_trials([P], eng, opt)
    assert eng._em_ws is ws and ws.data_ptr() == eng._em_ws.data_ptr()
    assert other.results[0].iters == 4 and other.results[0].LogLs != a.results[0].LogLs[:4]
    for got in (a.results[0], b.results[0]):
        assert got.iters == ref.iters == 7 and got.stable and ref.stable
        np.testing.assert_array_equal(np.array(got.LogLs), np.array(ref.LogLs))
        assert got.LL == ref.LL
        for f in POST_FIELDS:
            np.testing.assert_array_equal(getattr(got.post, f), getattr(ref.post, f), err_msg=f)
        assert torch.equal(got.hatZ, ref.hatZ) and torch.equal(got.L_elbo, ref.L_elbo)
    assert a.best == b.best == 0


@pytest.mark.gpu
def test_cluster_with_the_device_engine(vb, monkeypatch):
    """cluster.vbhem_h3m_c on the planted HMMs (K = 2, S = 2, 6 'baseem' trials): the same
    best trial and labels, every trial's bound at rtol 1e-10.  Where the clustering runs
    the trials one after another (S = 17; Sb > S) em_engine='device' is that same path."""
    from vbhem_amd import cluster, em, vhem
    hmms, _ = vhem.planted_hmms(20, seed=3)
    base = vhem.hmms_to_h3m(hmms, "full")
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20, Nv=100,
               seed=1001, trials=6, max_iter=30, minDiff=1e-5, learn_hyps=0, initmode="baseem")
    o = vb.default_options(2, 2, 2, **opt)
    seen = []
    real = em.vbhem_h3m_c_trials

    def spy(*a, **k):
        tr = real(*a, **k)
        seen.append((k.get("em_engine", "host"), tr))
        return tr

    monkeypatch.setattr(em, "vbhem_h3m_c_trials", spy)
    host = cluster.vbhem_h3m_c(base, o, DEV)
    dev = cluster.vbhem_h3m_c(base, dict(o, em_engine="device"), DEV)
    monkeypatch.undo()
    assert [e for e, _ in seen] == ["host", "device"]
    _compare("I", seen[0][1], seen[1][1], opt["minDiff"])
    print("bounds host", host["LLall"], "device", dev["LLall"])
    assert dev["best"] == host["best"] and np.array_equal(dev["label"], host["label"])
    np.testing.assert_allclose(dev["LLall"], host["LLall"], rtol=1e-10, atol=0)
    for S in (17, 1):  # no batched E-step (S > 16; Sb = 2 > S = 1): one trial after another
        oo = vb.default_options(2, S, 2, **dict(opt, trials=2, max_iter=2))
        h = cluster.vbhem_h3m_c(base, oo, DEV)
        g = cluster.vbhem_h3m_c(base, dict(oo, em_engine="device"), DEV)
        assert np.array_equal(h["LLall"], g["LLall"]) and np.array_equal(h["label"], g["label"])
        for f in POST_FIELDS:
            np.testing.assert_array_equal(getattr(h["result"].post, f), getattr(g["result"].post, f))
