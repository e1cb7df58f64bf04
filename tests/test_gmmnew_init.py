"""The batched 'gmmNew' initialisation on the CPU: the serial walker of
csrc/vbhem_ghem_run.h (tests/ghemcheck) against h3m.gmm_mix_hier_em, gmm_mix_hier_em_batch
and gmmnew_init_batch on a stand-in engine backed by the walker against gmm_mix_hier_em and
gmmnew_init, and vbhem_h3m_c with init_engine='device' on the stand-in.  Inputs, conditions
and tolerances: tests/ghem_ref.py."""
import numpy as np
import pytest

import ghem_ref as G


def test_advance_equals_the_discarded_draw(vb):
    """bit_generator.advance(T n) leaves a PCG64 generator where random((T, n)) does: the
    same next integers() and random()."""
    for seed, T, n in ((1, 3, 25), (2, 8, 1000), (3, 32, 513)):
        a = np.random.Generator(np.random.PCG64(seed))
        b = np.random.Generator(np.random.PCG64(seed))
        a.random((T, n))
        b.bit_generator.advance(T * n)
        assert a.integers(n) == b.integers(n)
        assert [a.random() for _ in range(5)] == [b.random() for _ in range(5)]
        assert np.array_equal(a.random((2, 3)), b.random((2, 3)))
    j0, u = G.draws_of(5, 300, 4)
    X, C = G.points(300, 2, True, 4, 5)
    with np.errstate(all="ignore"):
        a = vb.h3m.gmm_mix_hier_em(X, C, True, 4, 1500.0, 30, np.random.Generator(np.random.PCG64(5)))
        b = vb.h3m.gmm_mix_hier_em(X, C, True, 4, 1500.0, 30, G.Draws(j0, u))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("n,d,T,full", G.SHAPES)
def test_walker_matches_reference(vb, n, d, T, full):
    G.scenario_shape(G.HOST, n, d, T, full)


def test_measured_units_hold(vb):
    """The walker's largest deviation from the reference over the shapes stays near what
    ghem_ref.MEASURED_UNITS records: within twice that (another libm or BLAS moves it),
    where the bound is eight times that."""
    worst = G.measure_units()
    print("units", worst)
    assert G.UNITS == 8.0 * G.MEASURED_UNITS
    assert max(worst.values()) <= 2.0 * G.MEASURED_UNITS, worst


def test_tile_is_a_function_of_n_and_d(vb):
    assert G.tile_points(300, 2) == G.tile_points(25, 16) == G.tile_points(262144, 2) == 256
    assert G.tile_points(G.LARGE[0], 2) == G.tile_points(G.LARGE[0], 16) == 1024
    assert [s[0] for s in G.SHAPES[2:6]] == [255, 256, 257, 513]


def test_walker_matches_reference_with_large_tiles(vb):
    G.scenario_shape(G.HOST, *G.LARGE)


def test_iterations(vb):
    G.scenario_iterations(G.HOST)


def test_init_centres(vb):
    G.scenario_init_centres(G.HOST)


def test_bad_trials_are_contained(vb):
    G.scenario_contained(G.HOST)


def test_walker_batch_is_order_independent(vb):
    G.scenario_batching(G.HOST, 3)


def test_logpost_is_optional(vb):
    G.scenario_optional(G.HOST)


def test_limits(vb):
    X, C = G.points(40, 2, True, 2, 1)
    G.run_fit(G.HOST, np.zeros((40, 17)), np.zeros((40, 17)), False, 2, 100.0, 3, [0], [[0.5]], expect=-2)
    G.run_fit(G.HOST, X, C, True, 33, 100.0, 3, [0], [np.zeros(32)], expect=-2)
    with pytest.raises(ValueError, match="T <= 32"):
        vb.h3m.gmm_mix_hier_em_batch(X, C, True, 33, 100.0, 3, [1], engine=G.CheckEngine())
    with pytest.raises(ValueError, match="d <= 16"):
        vb.h3m.gmm_mix_hier_em_batch(np.zeros((40, 17)), np.ones((40, 17)), False, 2, 100.0, 3, [1],
                                     engine=G.CheckEngine())
    base = vb.synth_base_set(6, 2, 2, 2, vb.COV_FULL, seed=3)
    with pytest.raises(ValueError, match="S <= 32"):
        vb.h3m.gmmnew_init_batch(base, vb.default_options(2, 33, 2, Nv=10), [1], engine=G.CheckEngine())


# ---------------------------------------------------------------------------------------
# the Python layer on the stand-in engine
# ---------------------------------------------------------------------------------------
def _admissible_seeds(X, C, full, T, vs, seeds, iterations=30):
    out = []
    for s in seeds:
        try:
            G.ref_fit(X, C, full, T, vs, iterations, *G.draws_of(s, X.shape[0], T))
        except AssertionError:
            continue
        out.append(s)
    return out


def test_em_batch_equals_gmm_mix_hier_em(vb):
    """Per trial what gmm_mix_hier_em returns, and the generator left where it leaves it."""
    X, C = G.points(300, 3, True, 4, 51)
    vs = G.samples_of(300)
    seeds = _admissible_seeds(X, C, True, 4, vs, range(200, 230))[:5]
    info = {}
    got = vb.h3m.gmm_mix_hier_em_batch(X, C, True, 4, vs, 30, seeds, engine=G.CheckEngine(), want_logpost=True,
                                       info=info)
    assert info["replayed"] == [] and len(got) == len(seeds) == 5
    for r, s in enumerate(seeds):
        g = np.random.Generator(np.random.PCG64(s))
        mx, cen, vr, lp = vb.h3m.gmm_mix_hier_em(X, C, True, 4, vs, 30, g)
        ref = dict(mxwt=mx, centres=cen, covars=vr, logpost=lp, logp=info["logp"][r])
        one = {k: [v] for k, v in zip(("mxwt", "centres", "covars", "logpost"), got[r])}
        one["logp"] = [info["logp"][r]]
        G.assert_close(one, ref, 0, X, C)
        assert g.random() == info["rngs"][r].random()
    plain = vb.h3m.gmm_mix_hier_em_batch(X, C, True, 4, vs, 30, seeds[:2], engine=G.CheckEngine())
    assert plain[0][3] is None and np.array_equal(plain[1][1], got[1][1])
    # given centres: the discarded draw alone is skipped
    init = np.stack([X[[1, 50, 100, 200]] + 0.25, X[[2, 60, 110, 210]] + 0.25])
    info = {}
    got = vb.h3m.gmm_mix_hier_em_batch(X, C, True, 4, vs, 30, [7, 8], engine=G.CheckEngine(), init_centres=init,
                                       info=info)
    for r, s in enumerate((7, 8)):
        g = np.random.Generator(np.random.PCG64(s))
        ref = vb.h3m.gmm_mix_hier_em(X, C, True, 4, vs, 30, g, init[r])
        assert np.abs(got[r][1] - ref[1]).max() <= G.UNITS * 300 * 2.0 ** -53 * np.abs(X).max()
        assert g.random() == info["rngs"][r].random()


def test_one_component_stays_on_the_host(vb):
    """T = 1: the closed form, no engine call, no draw consumed."""
    X, C = G.points(50, 2, False, 2, 52)
    eng, info = G.CheckEngine(), {}
    got = vb.h3m.gmm_mix_hier_em_batch(X, C, False, 1, 100.0, 30, [3, 4], engine=eng, info=info)
    ref = vb.h3m.gmm_mix_hier_em(X, C, False, 1, 100.0, 30, None)
    assert eng.calls == 0
    assert all(np.array_equal(a, b) for a, b in zip(got[1], ref))
    assert info["rngs"][0].random() == np.random.Generator(np.random.PCG64(3)).random()


def test_em_batch_replays_what_is_not_ok(vb):
    """NONFINITE: the replay returns the reference's NaN centre; SINGULAR: it raises numpy's
    LinAlgError; DEGENERATE: the reference's other branch.  Healthy trials are untouched."""
    X, C = G.points(300, 2, True, 3, 53)
    vs = G.samples_of(300)
    seeds = _admissible_seeds(X, C, True, 3, vs, range(300, 320))[:2]
    good = X[[3, 120, 250]] + 0.25
    far = good.copy()
    far[1] = 1e4
    info = {}
    with np.errstate(all="ignore"):
        got = vb.h3m.gmm_mix_hier_em_batch(X, C, True, 3, vs, 30, [1, 2, 3], engine=G.CheckEngine(),
                                           init_centres=[good, far, good], info=info)
        ref = vb.h3m.gmm_mix_hier_em(X, C, True, 3, vs, 30, np.random.Generator(np.random.PCG64(2)), far)
    assert info["replayed"] == [1] and info["status"].tolist() == [G.OK, G.NONFINITE, G.OK]
    assert np.isnan(got[1][1][1]).all() and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[1], ref))
    assert np.array_equal(got[0][1], got[2][1]) and np.isfinite(got[0][1]).all()
    with pytest.raises(np.linalg.LinAlgError):
        vb.h3m.gmm_mix_hier_em_batch(X, np.zeros_like(C), True, 3, vs, 30, seeds, engine=G.CheckEngine())
    Xd = np.repeat(X[:2], 150, axis=0)
    info = {}
    with np.errstate(all="ignore"):
        got = vb.h3m.gmm_mix_hier_em_batch(Xd, C, True, 3, vs, 30, [5], engine=G.CheckEngine(), info=info)
        g = np.random.Generator(np.random.PCG64(5))
        ref = vb.h3m.gmm_mix_hier_em(Xd, C, True, 3, vs, 30, g)
    assert info["status"].tolist() == [G.DEGENERATE] and info["replayed"] == [0]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[0], ref))
    assert g.random() == info["rngs"][0].random()


def _points_of(vb, base):
    bn = base.numpy()
    ns = bn["nstates"]
    return (np.concatenate([bn["centres"][i, :int(ns[i])] for i in range(base.N)]),
            np.concatenate([bn["covars"][i, :int(ns[i])] for i in range(base.N)]))


def _init_seeds(vb, base, o, seeds, count):
    X, C = _points_of(vb, base)
    full = base.covmode == vb.COV_FULL
    return X, C, _admissible_seeds(X, C, full, o["S"], o["Nv"] * base.N, seeds, int(o.get("initopt_iter", 30)))[:count]


def test_init_batch_equals_gmmnew_init(vb):
    """Field by field, full and diagonal covariances (mode 'r0' and 'u0')."""
    for covmode, mode, d in ((vb.COV_FULL, "r0", 2), (vb.COV_DIAG, "u0", 3)):
        base = vb.synth_base_set(30, 3, 3, d, covmode, seed=21)
        o = vb.default_options(3, 3, d, Nv=10, seed=1, covmode=covmode, initopt_mode=mode)
        X, C, seeds = _init_seeds(vb, base, o, range(100, 130), 4)
        assert len(seeds) == 4
        info = {}
        got = vb.h3m.gmmnew_init_batch(base, o, seeds, engine=G.CheckEngine(), info=info)
        assert info["replayed"] == [] and {"points", "fit", "host"} <= set(info)
        for a, s in zip(got, seeds):
            G.posterior_close(a, vb.h3m.gmmnew_init(base, o, s), X.shape[0], X, C, covmode == vb.COV_FULL)
    with pytest.raises(ValueError, match="'m'"):
        vb.h3m.gmmnew_init_batch(base, dict(o, initopt_mode="m"), [1], engine=G.CheckEngine())


def test_cluster_device_engine_runs_gmmnew_batched(vb, monkeypatch):
    """vbhem_h3m_c with initmode 'gmmNew': init_engine='device' goes through the batched
    call (here on the stand-in) and gives the host path's trials."""
    from oracle_engine import OracleEngine
    from vbhem_amd import cluster
    made = []

    def stand_in(device, chunk_trials=None):
        made.append(G.CheckEngine(device, chunk_trials))
        return made[-1]

    monkeypatch.setattr(vb.h3m, "GhemDeviceEngine", stand_in)
    base = vb.synth_base_set(16, 2, 2, 2, vb.COV_FULL, seed=1002, exprmt1=True)
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20, Nv=100,
               seed=1001, trials=3, max_iter=10, minDiff=1e-5, learn_hyps=0, initmode="gmmNew")
    o = vb.default_options(2, 2, 2, **opt)
    factory = lambda b, K, S, T, trials=1: OracleEngine(b, K, S, T, nthreads=2, trials=trials)
    host = cluster.vbhem_h3m_c(base, o, engine_factory=factory)
    assert not made
    dev = cluster.vbhem_h3m_c(base, dict(o, init_engine="device"), engine_factory=factory)
    assert len(made) == 1 and made[0].calls == 1
    assert dev["best"] == host["best"] and np.array_equal(dev["label"], host["label"])
    np.testing.assert_allclose(dev["LLall"], host["LLall"], rtol=1e-8)
