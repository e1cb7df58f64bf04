"""The TILED schedule of the initialisations' k-means on the CPU: the serial tiled walker of
csrc/vbhem_wtk_tiled_run.h (tests/wtktilecheck: the kernels' phases and tile order, one lane)
against h3m.kmeans_pp / h3m.weighted_kmeans and against the block schedule's walker; the
re-seed hand-over; wtkmeans_init_batch and gmmnew_init_batch with schedule="tiled" on
stand-in engines backed by the walker; opt["init_schedule"].  Inputs, conditions and
tolerances: tests/wtk_ref.py, tests/ghem_ref.py (through tests/wtk_tiled_ref.py)."""
import numpy as np
import pytest

import ghem_ref as G
import wtk_ref as W
import wtk_tiled_ref as T


@pytest.mark.parametrize("n,d,K", T.SHAPES)
def test_walker_matches_reference(vb, n, d, K):
    T.scenario_shape(T.HOST, n, d, K)


def test_tile_size_and_rounds(vb):
    assert [T.tile_points(n, 8) for n in (1, 256, 262144, 262145)] == [256, 256, 256, 1024]
    assert T.rounds_of(16, False) == 15 + 100 + 1 + 101 and T.rounds_of(16, True) == 15 + 100


def test_singletons(vb):
    T.scenario_singletons(T.HOST)


def test_weightless_cluster_and_zero_weights(vb):
    T.scenario_weightless(T.HOST)


def test_emptied_cluster_goes_to_the_block_schedule(vb):
    T.scenario_emptied(T.HOST)


def test_bad_and_degenerate_are_contained(vb):
    T.scenario_contained(T.HOST)


def test_walker_batch_is_order_independent(vb):
    T.scenario_batching(T.HOST, 3)


def test_limits(vb):
    X, w = W.blobs(40, 2, 2, 1)
    T.run_cluster(T.HOST, X, w, 33, [0], [np.zeros(32)], expect=-2)
    T.run_cluster(T.HOST, np.zeros((40, 17)), w, 2, [0], [[0.5]], expect=-2)
    T.run_seed(T.HOST, X, 33, [0], [np.zeros(32)], expect=-2)
    T.run_seed(T.HOST, X, 1, [0], [[0.0]], expect=-2)
    base = vb.synth_base_set(6, 2, 2, 2, vb.COV_FULL, seed=3)
    with pytest.raises(ValueError, match="K <= 32"):
        vb.h3m.wtkmeans_init_batch(base, vb.default_options(33, 2, 2, Nv=10), [1], engine=T.WtkEngine(),
                                   schedule="tiled")
    with pytest.raises(ValueError, match="S <= 32"):
        vb.h3m.gmmnew_init_batch(base, vb.default_options(2, 33, 2, Nv=10), [1], engine=T.GhemEngine(),
                                 schedule="tiled")
    for call in (lambda: vb.h3m.wtkmeans_init_batch(base, vb.default_options(2, 2, 2, Nv=10), [1],
                                                    engine=T.WtkEngine(), schedule="grid"),
                 lambda: vb.h3m.gmmnew_init_batch(base, vb.default_options(2, 2, 2, Nv=10), [1],
                                                  engine=T.GhemEngine(), schedule="grid"),
                 lambda: vb.h3m.WtkDeviceEngine("cpu", schedule="grid")):
        with pytest.raises(ValueError, match="schedule"):
            call()


# ---------------------------------------------------------------------------------------
# the initialisations on the stand-in engines
# ---------------------------------------------------------------------------------------
def _wtk_e2e(vb, base, o, seeds):
    pts = vb.h3m.wtkmeans_points(base, o.get("initopt_mode", "r0"))
    want = [vb.h3m.wtkmeans_init(base, o, s, pts) for s in seeds]
    eng = T.WtkEngine()
    got = vb.h3m.wtkmeans_init_batch(base, o, seeds, engine=eng, schedule="tiled")
    assert eng.calls == 1 and len(got) == len(want)
    for a, b in zip(got, want):
        W.posterior_equal(a, b, pts[0].shape[0], np.abs(pts[0]).max())


def test_wtkmeans_init_batch_tiled_equals_wtkmeans_init(vb):
    """Field by field over seeds with clusters of more than S members (a fresh generator
    handed to makeAprior) and of at most S members (padding); then diagonal covariances."""
    base = vb.synth_base_set(9, 3, 2, 2, vb.COV_FULL, seed=21)
    o = vb.default_options(4, 3, 2, Nv=10, seed=1)
    seeds = [s for s in range(100, 160) if W.admissible(vb, base, o, s)][:12]
    assert len(seeds) == 12
    _wtk_e2e(vb, base, o, seeds)
    based = vb.synth_base_set(12, 2, 3, 3, vb.COV_DIAG, seed=22)
    od = vb.default_options(2, 2, 3, Nv=10, covmode=vb.COV_DIAG, initopt_mode="u0")
    _wtk_e2e(vb, based, od, [s for s in range(5, 40) if W.admissible(vb, based, od, s)][:2])


def test_wtkmeans_init_batch_tiled_replays_degenerate_trials(vb):
    """Fewer distinct means than clusters: the tiled seeding ends DEGENERATE and the trial
    goes through wtkmeans_init, as under the block schedule."""
    import torch
    base = vb.synth_base_set(8, 2, 2, 2, vb.COV_FULL, seed=24)
    base.centres[:] = torch.tensor([[0.0, 0.0], [3.0, 1.0]], dtype=torch.float64)[None]
    o = vb.default_options(3, 2, 2, Nv=10)
    info = {}
    got = vb.h3m.wtkmeans_init_batch(base, o, [7, 8], engine=T.WtkEngine(), schedule="tiled", info=info)
    assert info["replayed"] == [0, 1]
    for s, a in zip((7, 8), got):
        b = vb.h3m.wtkmeans_init(base, o, s)
        for k in ("alpha", "eta", "epsilon", "lam", "v", "W", "m"):
            np.testing.assert_allclose(getattr(a, k), getattr(b, k), rtol=1e-12, atol=1e-12)


def _admissible_seeds(X, C, full, T_, vs, seeds, iterations=30):
    out = []
    for s in seeds:
        try:
            G.ref_fit(X, C, full, T_, vs, iterations, *G.draws_of(s, X.shape[0], T_))
        except AssertionError:
            continue
        out.append(s)
    return out


def test_em_batch_tiled_equals_gmm_mix_hier_em(vb):
    """Per trial what gmm_mix_hier_em returns, the seeding's Lloyd passes reported, and the
    generator left where gmm_mix_hier_em leaves it; a DEGENERATE seeding is replayed."""
    X, C = G.points(300, 3, True, 4, 51)
    vs = G.samples_of(300)
    seeds = _admissible_seeds(X, C, True, 4, vs, range(200, 230))[:4]
    assert len(seeds) == 4
    eng, info = T.GhemEngine(), {}
    got = vb.h3m.gmm_mix_hier_em_batch(X, C, True, 4, vs, 30, seeds, engine=eng, want_logpost=True, info=info,
                                       schedule="tiled")
    block_info = {}
    vb.h3m.gmm_mix_hier_em_batch(X, C, True, 4, vs, 30, seeds, engine=G.CheckEngine(), info=block_info)
    assert eng.seeds == 1 and eng.calls == 1 and info["replayed"] == []
    assert np.array_equal(info["iters"], block_info["iters"]) and np.array_equal(info["status"], block_info["status"])
    for r, s in enumerate(seeds):
        g = np.random.Generator(np.random.PCG64(s))
        mx, cen, vr, lp = vb.h3m.gmm_mix_hier_em(X, C, True, 4, vs, 30, g)
        one = {k: [v] for k, v in zip(("mxwt", "centres", "covars", "logpost"), got[r])}
        one["logp"] = [info["logp"][r]]
        G.assert_close(one, dict(mxwt=mx, centres=cen, covars=vr, logpost=lp, logp=info["logp"][r]), 0, X, C)
        assert g.random() == info["rngs"][r].random()
    # given centres: nothing to seed
    eng = T.GhemEngine()
    vb.h3m.gmm_mix_hier_em_batch(X, C, True, 4, vs, 30, [7], engine=eng, schedule="tiled",
                                 init_centres=[X[[1, 50, 100, 200]] + 0.25])
    assert eng.seeds == 0 and eng.calls == 1
    # fewer distinct points than components, between two ordinary trials
    Xd = np.repeat(X[:2], 150, axis=0)
    info = {}
    with np.errstate(all="ignore"):
        got = vb.h3m.gmm_mix_hier_em_batch(Xd, C, True, 3, vs, 30, [5], engine=T.GhemEngine(), info=info,
                                           schedule="tiled")
        g = np.random.Generator(np.random.PCG64(5))
        ref = vb.h3m.gmm_mix_hier_em(Xd, C, True, 3, vs, 30, g)
    assert info["status"].tolist() == [G.DEGENERATE] and info["replayed"] == [0]
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got[0], ref))
    assert g.random() == info["rngs"][0].random()


def test_gmmnew_init_batch_tiled_equals_gmmnew_init(vb):
    for covmode, mode, d in ((vb.COV_FULL, "r0", 2), (vb.COV_DIAG, "u0", 3)):
        base = vb.synth_base_set(30, 3, 3, d, covmode, seed=21)
        o = vb.default_options(3, 3, d, Nv=10, seed=1, covmode=covmode, initopt_mode=mode)
        bn = base.numpy()
        X = np.concatenate([bn["centres"][i, :int(bn["nstates"][i])] for i in range(base.N)])
        C = np.concatenate([bn["covars"][i, :int(bn["nstates"][i])] for i in range(base.N)])
        full = covmode == vb.COV_FULL
        seeds = _admissible_seeds(X, C, full, 3, o["Nv"] * base.N, range(100, 130))[:4]
        assert len(seeds) == 4
        eng, info = T.GhemEngine(), {}
        got = vb.h3m.gmmnew_init_batch(base, o, seeds, engine=eng, info=info, schedule="tiled")
        assert eng.seeds == 1 and info["replayed"] == [] and {"points", "fit", "seed", "host"} <= set(info)
        for a, s in zip(got, seeds):
            G.posterior_close(a, vb.h3m.gmmnew_init(base, o, s), X.shape[0], X, C, full)


# ---------------------------------------------------------------------------------------
# opt["init_schedule"]
# ---------------------------------------------------------------------------------------
def test_init_schedule_option(vb, monkeypatch):
    """A bad value raises; 'tiled' reaches the engines of both initialisations under
    init_engine='device' and gives the host path's trials; under 'host' it is ignored."""
    from oracle_engine import OracleEngine
    from vbhem_amd import cluster
    made = []

    def wtk_stand_in(device, chunk_trials=None, schedule="block"):
        made.append(("wtk", schedule))
        return T.WtkEngine() if schedule == "tiled" else W.CheckEngine()

    def ghem_stand_in(device, chunk_trials=None):
        made.append(T.GhemEngine(device, chunk_trials))
        return made[-1]

    monkeypatch.setattr(vb.h3m, "WtkDeviceEngine", wtk_stand_in)
    monkeypatch.setattr(vb.h3m, "GhemDeviceEngine", ghem_stand_in)
    base = vb.synth_base_set(16, 2, 2, 2, vb.COV_FULL, seed=1002, exprmt1=True)
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20, Nv=100,
               seed=1001, trials=3, max_iter=10, minDiff=1e-5, learn_hyps=0)
    factory = lambda b, K, S, T_, trials=1: OracleEngine(b, K, S, T_, nthreads=2, trials=trials)
    for initmode in ("wtkmeans", "gmmNew"):
        o = vb.default_options(2, 2, 2, **dict(opt, initmode=initmode))
        with pytest.raises(ValueError, match="init_schedule"):
            cluster.vbhem_h3m_c(base, dict(o, init_engine="device", init_schedule="grid"), engine_factory=factory)
        host = cluster.vbhem_h3m_c(base, o, engine_factory=factory)
        ignored = cluster.vbhem_h3m_c(base, dict(o, init_engine="host", init_schedule="tiled"), engine_factory=factory)
        assert not made and np.array_equal(host["LLall"], ignored["LLall"])
        dev = cluster.vbhem_h3m_c(base, dict(o, init_engine="device", init_schedule="tiled"), engine_factory=factory)
        assert len(made) == 1
        if initmode == "wtkmeans":
            assert made == [("wtk", "tiled")]
        else:
            assert made[0].seeds == 1 and made[0].calls == 1
        made.clear()
        block = cluster.vbhem_h3m_c(base, dict(o, init_engine="device"), engine_factory=factory)
        if initmode == "wtkmeans":
            assert made == [("wtk", "block")]
        else:
            assert made[0].seeds == 0 and made[0].calls == 1
        made.clear()
        for run in (dev, block):
            assert run["best"] == host["best"] and np.array_equal(run["label"], host["label"])
            np.testing.assert_allclose(run["LLall"], host["LLall"], rtol=1e-8)
