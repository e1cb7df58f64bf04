"""VHEM clustering on the CPU: the restatement (tests/vhem_ref.py) pinned by closed
forms, the package's host math (vbhem_amd.vhem) against it, and the EM loop, trials
and vhem_cluster on a CPU stand-in engine over the oracle's per-pair E-step."""
import warnings

import numpy as np
import pytest
import torch

import vhem_ref as ref
from cases import make_case, make_reduced
from vhem_standin import StandInEngine, factory

TOL = 1e-12


@pytest.fixture(scope="module")
def vh(vb):
    from vbhem_amd import vhem
    return vhem


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    assert float(np.abs(a - b).max()) <= tol * scale, float(np.abs(a - b).max())


def red_h3m(K, S, d, cov, seed, omega=None):
    r = make_reduced(K, S, d, cov, seed=seed)
    r["omega"] = np.full(K, 1.0 / K) if omega is None else np.asarray(omega, dtype=float)
    r["LogL"] = -np.inf
    return r


def opts(**over):
    o = dict(tau=5, Nv=100, inf_norm="nt", smooth=1.0, reg_cov=0.001, termvalue=1e-5, max_iter=100,
             min_iter=1)
    o.update(over)
    return o


# -- the restatement, pinned by closed forms ---------------------------------
@pytest.mark.parametrize("norm", ["", "n", "nt", "t"])
def test_ref_one_cluster(vo, norm):
    """K = 1: Z = 1 and LogL = sum_i (log 1 + N_i L_i / inf_norm)."""
    base = make_case(7, 1, 3, 3, 2, 1, seed=3)["base"]
    h = red_h3m(1, 3, 2, 1, 3)
    o = opts(inf_norm=norm)
    es = ref.estep(base, h, o)
    assert np.array_equal(es["Z"], np.ones((7, 1)))
    Kb, T, Nv = 7, o["tau"], o["Nv"]
    inn = {"": 1.0, "n": Nv / Kb, "nt": T * Nv / Kb, "t": float(T)}[norm]
    L = vo.c_vhem_estep_pairs(base, h, T, 1.0)["LL_elbo"][:, 0]
    want = sum(0.0 + (Nv * base["omega"][i] * Kb) * (L[i] / inn) for i in range(Kb))
    assert abs(es["LogL"] - want) <= 1e-12 * abs(want)


def test_ref_identical_clusters(vo):
    """Two identical clusters: Z(i, :) = omega_r."""
    base = make_case(6, 2, 3, 3, 2, 0, seed=4)["base"]
    h = red_h3m(1, 3, 2, 0, 4)
    h2 = {k: (np.concatenate([v, v]) if isinstance(v, np.ndarray) and k != "omega" else v)
          for k, v in h.items()}
    h2["omega"] = np.array([0.3, 0.7])
    es = ref.estep(base, h2, opts())
    close(es["Z"], np.tile([0.3, 0.7], (6, 1)), 1e-14)


@pytest.mark.parametrize("cov", [1, 0])
def test_ref_mstep_moments(vo, cov):
    """One cluster of one state, tau = 1, smooth = 1: the M-step mean and covariance are
    the omega * prior weighted moments of the base Gaussians, plus reg_cov."""
    base = make_case(6, 1, 1, 3, 2, cov, seed=5, ragged=True)["base"]
    base["omega"] = np.random.default_rng(1).dirichlet(np.ones(6))
    h = red_h3m(1, 1, 2, cov, 5)
    o = opts(tau=1, reg_cov=0.01)
    es = ref.estep(base, h, o)
    hm = ref.mstep_finish(ref.mstep_sums(base, es, 0), 1, 0.01, cov)
    w = base["omega"][:, None] * base["prior"]
    w = w / w.sum()
    mu = np.einsum("ib,iba->a", w, base["centres"])
    if cov == 1:
        m2 = np.einsum("ib,ibac->ac", w, base["covars"] + base["centres"][..., :, None] *
                       base["centres"][..., None, :])
        want = m2 - np.outer(mu, mu) + 0.01 * np.eye(2)
    else:
        want = np.einsum("ib,iba->a", w, base["covars"] + base["centres"] ** 2) - mu ** 2 + 0.01
    close(hm["centres"][0], mu, 1e-12)
    close(hm["covars"][0], want, 1e-12)
    close(hm["A"], [[1.0]])
    assert hm["emit_vcounts"].shape == (1,)


def test_ref_gate_excludes_underflowed_pairs(vo):
    """inf_norm = '' and Nv = 100: some Z underflow to exactly 0 (the > 0 gate then
    drops the pair) while other off-winner entries stay positive."""
    base = make_case(40, 3, 3, 3, 2, 1, seed=11)["base"]
    es = ref.estep(base, red_h3m(3, 3, 2, 1, 11), opts(inf_norm="", tau=10))
    off = np.sort(es["Z"], axis=1)[:, :-1]
    assert (off == 0).any() and (off > 0).any()


# -- the package's host math against the restatement --------------------------
@pytest.mark.parametrize("cov,S,tau", [(1, 3, 5), (0, 3, 5), (1, 1, 5), (0, 2, 1)])
def test_hem_mstep(vo, vh, cov, S, tau):
    base = make_case(9, 3, S, 3, 2, cov, seed=6, ragged=True)["base"]
    es = ref.estep(base, red_h3m(3, S, 2, cov, 6, omega=[0.2, 0.5, 0.3]), opts(tau=tau))
    st = ref.packed_stats(base, es, cov)
    got = vh.hem_mstep(st, 9, tau, 0.001, cov)
    for j in range(3):
        want = ref.mstep_finish(ref.mstep_sums(base, es, j), tau, 0.001, cov)
        for k in ("prior", "A", "centres", "covars", "emit_vcounts"):
            close(got[k][j], want[k])
    close(got["omega"], es["Z"].sum(0) / 9)


def test_degenerate_fixes(vh):
    rng = np.random.default_rng(2)
    h = red_h3m(3, 3, 2, 1, 7, omega=[0.0, 0.6, 0.4])
    h["A"][1, 0, 2] = 0.0
    h["emit_vcounts"] = np.array([[1.0, 2.0, 3.0], [4.0, 0.0, 1.0], [1.0, 1.0, 1.0]])
    draws = [rng.random((3,)), rng.random((3, 3)), rng.random((2,))]

    def feeder():
        it = iter(draws)
        return lambda shape: next(it).reshape(shape)

    a, b = vh.copy_h3m(h), vh.copy_h3m(h)
    da, db = feeder(), feeder()
    vh.hem_fix_degenerate_component(a, 0, 3, da)
    ref.fix_degenerate_component(b, 0, 3, db)
    vh.hem_fix_degenerate_hmm(a, 1, 1, da)
    ref.fix_degenerate_hmm(b, 1, 1, db)
    for k in ("omega", "prior", "A", "centres", "covars", "emit_vcounts"):
        close(a[k], b[k])
    assert a["A"][0, 0, 2] == 0.0 and abs(a["omega"].sum() - 1) < 1e-15
    close(a["omega"], [0.3, 0.3, 0.4])


def _hmm_list(base, drop=()):
    out = []
    for i in range(base["prior"].shape[0]):
        if i in drop:
            out.append(None)
            continue
        n = int(base["nstates"][i])
        out.append(dict(prior=base["prior"][i, :n], trans=base["A"][i, :n, :n],
                        pdf=[dict(mean=base["centres"][i, s],
                                  cov=base["covars"][i, s] if base["covmode"] == 1 else
                                  np.diag(base["covars"][i, s])) for s in range(n)]))
    return out


@pytest.mark.parametrize("cov", [1, 0])
def test_hmms_to_h3m(vh, cov):
    base = make_case(6, 2, 3, 3, 2, cov, seed=8, ragged=True)["base"]
    hm = _hmm_list(base, drop=(2,))
    got = vh.hmms_to_h3m(hm, "full" if cov else "diag").numpy()
    want = ref.hmms_to_h3m(hm, cov)
    for k in ("nstates", "prior", "A", "centres", "covars", "omega"):
        close(got[k], want[k])
    assert got["omega"][2] == 0 and got["nstates"][2] == 1


def test_h3m_to_hmms(vh):
    h = red_h3m(3, 2, 2, 0, 9)
    h.update(Z=np.array([[0.1, 0.7, 0.2], [0.5, 0.2, 0.3], [0.2, 0.2, 0.6], [0.0, 0.9, 0.1]]),
             LogL=-3.0, LogLs=[-5.0, -3.0], L_elbo1=np.zeros((4, 3)),
             emit_vcounts=np.arange(6.0).reshape(3, 2))
    g = vh.h3m_to_hmms(h, 0)
    assert g["label"].tolist() == [1, 0, 2, 1]
    assert [x.tolist() for x in g["groups"]] == [[1], [0, 3], [2]]
    assert g["group_size"].tolist() == [1, 2, 1]
    assert g["LogL"] == -3.0 and g["LogLs"] == [-5.0, -3.0] and g["L_elbo1"].shape == (4, 3)
    close(g["hmms"][1]["pdf"][0]["cov"], np.diag(h["covars"][1, 0]))
    close(g["hmms"][2]["stats"]["emit_vcounts"], [4.0, 5.0])
    close(g["hmms"][0]["trans"], h["A"][0])


# -- the EM loop ---------------------------------------------------------------
class ScriptedEngine:
    """fused_vhem returns harmless statistics with LogL from a script."""

    def __init__(self, base, K, S, LLs):
        self.base, self.K, self.S, self.trials = base, K, S, 1
        self.device = torch.device("cpu")
        self.LLs = list(LLs)
        self.n = 0
        self.hatZ = torch.full((base.N, K), 1.0 / K, dtype=torch.float64)
        self.LL = torch.zeros((base.N, K), dtype=torch.float64)

    def set_clusters(self, c):
        pass

    def set_log_omega(self, lo):
        pass

    def fused_vhem(self, Ni, omegaB, inf_norm, smooth=1.0):
        from vbhem_amd import host
        d = self.base.d
        v = np.ones(host.stats_len(self.K, self.S, d, self.base.covmode))
        v[self.K + self.K * self.S + self.K * self.S * self.S] = self.LLs[min(self.n, len(self.LLs) - 1)]
        # second moments large enough for a positive variance
        NU = host.stats_nu(d, self.base.covmode)
        U = v[-self.K * self.S * NU:].reshape(self.K, self.S, NU)
        U[..., 1 + d:] = 0.0
        U[..., 1 + d:1 + 2 * d] = 5.0
        self.n += 1
        return torch.from_numpy(v)


@pytest.mark.parametrize("LLs,kw,iters,warns", [
    # changeLL = inf until num_iter > 1: two M-steps at least; then 1e-6 < 1e-5 stops
    ([-100.0, -90.0, -80.0, -80.0 + 8e-5], {}, 3, False),
    # a negative change stops too, with a warning
    ([-100.0, -90.0, -95.0, -50.0], {}, 2, True),
    # max_iter: stop once num_iter > max_iter
    ([-100.0, -90.0, -80.0, -70.0, -60.0, -50.0, -40.0], dict(max_iter=3), 4, False),
    # min_iter holds a converged run
    ([-100.0, -90.0, -90.0, -90.0, -90.0, -90.0, -90.0], dict(min_iter=5), 5, False),
])
def test_stopping_rule(vb, vh, LLs, kw, iters, warns):
    bs = make_case(4, 2, 2, 2, 2, 0, seed=1)["bs"]
    eng = ScriptedEngine(bs, 2, 2, LLs)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = vh.hem_h3m_c_step(red_h3m(2, 2, 2, 0, 1), eng, opts(**kw))
    assert out["num_iter"] == iters
    assert out["LogLs"] == LLs[:iters + 1]
    assert any("negative" in str(x.message) for x in w) == warns


@pytest.mark.parametrize("cov,smooth,norm", [(1, 1.0, "nt"), (0, 2.5, "n")])
def test_em_loop_matches_restatement(vb, vo, vh, cov, smooth, norm):
    cs = make_case(12, 3, 3, 3, 2, cov, seed=12, ragged=True)
    h0 = red_h3m(3, 3, 2, cov, 12)
    o = opts(smooth=smooth, inf_norm=norm, tau=6)
    want = ref.c_step(h0, cs["base"], o, draw=np.random.default_rng(5).random)
    got = vh.hem_h3m_c_step(h0, StandInEngine(cs["bs"], 3, 3, 6), o, np.random.default_rng(5))
    assert got["num_iter"] == want["num_iter"] and want["num_iter"] >= 2
    close(got["LogLs"], want["LogLs"], 1e-9)
    for k in ("omega", "prior", "A", "centres", "covars", "Z", "L_elbo1"):
        close(got[k], want[k], 1e-7)


def test_trials_equal_single_runs(vb, vh):
    cs = make_case(10, 2, 2, 2, 2, 1, seed=13)
    hs = [red_h3m(2, 2, 2, 1, 20 + r) for r in range(3)]
    o = opts()
    both = vh.hem_h3m_c_trials(hs, StandInEngine(cs["bs"], 6, 2, 5, trials=3), o)
    for r in range(3):
        one = vh.hem_h3m_c_step(hs[r], StandInEngine(cs["bs"], 2, 2, 5), o)
        assert one["num_iter"] == both[r]["num_iter"]
        close(one["LogLs"], both[r]["LogLs"], 1e-13)
        close(one["Z"], both[r]["Z"], 1e-12)


# -- initialisations -------------------------------------------------------------
def _opt(vh, K, S, mode, **kw):
    return vh.default_hemopt(K, S, seed=1, initmode=mode, **kw)


def test_init_baseem(vb, vh):
    bs = make_case(8, 2, 3, 3, 2, 1, seed=14, ragged=True)["bs"]
    om = bs.omega.clone()
    om[[0, 3, 5]] = 0
    bs.omega = om / om.sum()
    bn = bs.numpy()
    h = vh.initialize_hem_h3m_c(bs, _opt(vh, 2, 3, "baseem"), np.random.default_rng(3))
    close(h["omega"], [0.5, 0.5])
    close(h["prior"], np.full((2, 3), 1 / 3))
    close(h["A"], np.full((2, 3, 3), 1 / 3))
    live = [(i, s) for i in range(8) if bn["omega"][i] > 0 for s in range(int(bn["nstates"][i]))]
    for j in range(2):
        for n in range(3):
            assert any(np.array_equal(h["centres"][j, n], bn["centres"][i, s]) and
                       np.array_equal(h["covars"][j, n], bn["covars"][i, s]) for i, s in live)
    h2 = vh.initialize_hem_h3m_c(bs, _opt(vh, 2, 3, "baseem"), np.random.default_rng(3))
    close(h["centres"], h2["centres"], 0.0)


def test_init_base(vb, vh):
    bs = make_case(6, 2, 3, 3, 2, 0, seed=15)["bs"]
    bn = bs.numpy()
    h = vh.initialize_hem_h3m_c(bs, _opt(vh, 2, 3, "base", covar_type="diag"),
                                np.random.default_rng(4))
    idx = np.random.default_rng(4).permutation(6)[:2]
    close(h["A"], bn["A"][idx], 0.0)
    close(h["centres"], bn["centres"][idx], 0.0)
    close(h["omega"], [0.5, 0.5])


@pytest.mark.parametrize("mode,iom", [("gmmNew", "r0"), ("gmmNew2", "u0"), ("gmmNew", "m0")])
def test_init_gmmnew(vb, vh, mode, iom):
    bs = make_case(12, 3, 2, 3, 2, 1, seed=16, ragged=True)["bs"]
    o = _opt(vh, 3, 2, mode, initopt=dict(mode=iom))
    h = vh.initialize_hem_h3m_c(bs, o, np.random.default_rng(6))
    assert h["centres"].shape == (3, 2, 2) and h["covars"].shape == (3, 2, 2, 2)
    assert abs(h["omega"].sum() - 1) < 1e-14 and np.all(h["omega"] > 0)
    assert np.all(np.linalg.eigvalsh(h["covars"]) > 0)
    if mode == "gmmNew":      # the S Gaussians are shared by every cluster
        close(h["centres"][0], h["centres"][1], 0.0)
    else:                      # N * Kr different Gaussians
        assert len({tuple(c) for c in h["centres"].reshape(-1, 2)}) == 6
    if "u" in iom:
        close(h["A"], np.full((3, 2, 2), 0.5))
    if "m" in iom:
        ok = np.isfinite(h["A"]).all(axis=(1, 2))
        close(h["A"][ok].sum(-1), np.ones((int(ok.sum()), 2)), 1e-12)


def test_init_subsample(vb, vh):
    bs = vb.synth_base_set(450, 2, 2, 2, 1, seed=3)
    sub = vh._init_base(bs, np.random.default_rng(0))
    i0 = int(np.random.default_rng(0).integers(0, 50))
    assert sub.N == 400 and abs(float(sub.omega.sum()) - 1) < 1e-12
    assert torch.equal(sub.centres, bs.centres[i0:i0 + 400])


# -- trials, driver ---------------------------------------------------------------
def test_options(vh):
    o = vh.default_hemopt(3, 2, seed=7)
    assert (o["trials"], o["reg_cov"], o["termvalue"], o["max_iter"], o["min_iter"], o["tau"], o["Nv"],
            o["inf_norm"], o["smooth"], o["sortclusters"], o["initmode"]) == \
        (100, 0.001, 1e-5, 100, 1, 10, 100, "nt", 1.0, "f", "auto")
    assert o["initopt"] == dict(iter=30, trials=4, mode="")
    assert vh.default_hemopt(3, 2, seed=7, initmode="gmmNew2")["initopt"]["mode"] == "u0"
    with pytest.raises(ValueError, match="seed"):
        vh.default_hemopt(3, 2)
    for bad in (dict(computeStats=1), dict(M=2), dict(initmode="kmeans"), dict(inf_norm="x"),
                dict(nonsense=1)):
        with pytest.raises(ValueError):
            vh.default_hemopt(3, 2, seed=1, **bad)
    assert [vh.inf_norm_value(m, 10, 100, 40) for m in ("", "n", "nt", "tn", "t")] == \
        [1.0, 2.5, 25.0, 25.0, 10.0]


def test_k_equals_kb(vb, vh):
    hm, _ = vh.planted_hmms(2, seed=1)
    out = vh.vhem_cluster(hm, 4, 2, dict(seed=1, trials=2, sortclusters=""), engine_factory=factory())
    assert out["LogL"] == 0.0 and np.array_equal(out["Z"], np.eye(4))
    assert out["label"].tolist() == [0, 1, 2, 3]
    close(out["hmms"][3]["trans"], hm[3]["trans"])


def test_all_nan_trials_raise(vb, vh):
    bs = make_case(4, 2, 2, 2, 2, 0, seed=1)["bs"]
    o = vh.default_hemopt(2, 2, seed=1, initmode="baseem", trials=2, covar_type="diag")
    make = lambda base, K, S, T, trials=1: ScriptedEngine(base, K, S, [float("nan")])  # noqa: E731
    with pytest.raises(ValueError, match="NaN"):
        vh.hem_h3m_c(bs, dict(o, max_iter=2), engine_factory=make,
                     inits=[red_h3m(2, 2, 2, 0, 1)])


@pytest.fixture(scope="module")
def planted(vb, vh):
    hm, lab = vh.planted_hmms(20, seed=0)
    log = []
    out = vh.vhem_cluster(hm, 2, 2, dict(seed=3, trials=8, initmode="baseem"),
                          engine_factory=factory(log))
    return hm, lab, out, log


def test_vhem_cluster_planted(vb, vh, planted):
    """The exprmt1 recipe on the stand-in: the planted labels are recovered."""
    from vbhem_amd import evaluate
    hm, lab, out, log = planted
    assert evaluate.rand_index(out["label"], lab)[0] == 1
    assert sorted(out["group_size"].tolist()) == [20, 20]
    # (Z = exp(lz - lse) with |lz| ~ 1e2: each entry carries ~ulp(lz) = 1e-14 relative)
    close(out["Z"].sum(1), np.ones(40), 1e-12)
    assert out["LogL"] == np.nanmax(out["trials_LL"]) and len(out["trials_LL"]) == 8
    assert len(log) == 1 and log[0].trials == 8          # one batched launch per iteration
    assert out["LogLs"][-1] == out["LogL"] and out["L_elbo1"].shape == (40, 2)
    for g in out["hmms"]:
        assert g["stats"]["emit_vcounts"].shape == (2,)
        close(g["trans"].sum(1), [1.0, 1.0], 1e-12)
    # sortclusters 'f': the first state is the prior's argmax
    assert all(int(np.argmax(g["prior"])) == 0 for g in out["hmms"])


def test_auto_picks_best(vb, vh):
    hm, lab = vh.planted_hmms(6, seed=2)
    kw = dict(seed=5, trials=2, max_iter=8)
    runs = {m: vh.vhem_cluster(hm, 2, 2, dict(kw, initmode=m), engine_factory=factory())
            for m in ("baseem", "gmmNew", "gmmNew2")}
    auto = vh.vhem_cluster(hm, 2, 2, dict(kw, initmode="auto"), engine_factory=factory())
    best = max(runs, key=lambda m: runs[m]["LogL"])
    assert auto["LogL"] == runs[best]["LogL"] and auto["initmode"] == best


def test_keep_suboptimal(vb, vh):
    hm, _ = vh.planted_hmms(5, seed=4)
    out = vh.vhem_cluster(hm, 2, 2, dict(seed=2, trials=3, initmode="baseem", max_iter=5,
                                         keep_suboptimal_hmms=1), engine_factory=factory())
    assert 1 <= len(out["suboptimal_hmms"]) <= 3 and len(out["trials_LL"]) == 3
