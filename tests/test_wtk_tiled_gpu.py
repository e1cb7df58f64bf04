"""The TILED schedule of the initialisations' k-means on the GPU (csrc/vbhem_wtk_tiled.hip):
the kernels against h3m.kmeans_pp / h3m.weighted_kmeans, against the block schedule and
against the serial tiled walker; past the tile-size switch; bitwise independence of a trial
from the batch; the re-seed hand-over and the contained trials; the seeding entry and
gmmnew_init_batch(schedule="tiled") against gmmnew_init; the limits; vbhem_h3m_c with
init_schedule="tiled" against the host path.  Inputs, conditions and tolerances:
tests/wtk_ref.py, tests/ghem_ref.py (through tests/wtk_tiled_ref.py)."""
import numpy as np
import pytest

import ghem_ref as G
import wtk_ref as W
import wtk_tiled_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n,d,K", T.SHAPES)
def test_kernels_match_reference_and_walker(vb, n, d, K):
    T.scenario_shape(T.DEVICE, n, d, K)
    X, w, j0, u = W.case(n, d, K, 3)
    T.against_walker(X, w, K, j0, u)
    block = W.run_cluster(W.DEVICE, X, w, K, [j0], [u])          # the block schedule's kernels
    tiled = T.run_cluster(T.DEVICE, X, w, K, [j0], [u])
    assert all(np.array_equal(block[k], tiled[k]) for k in T.KEYS)


def test_large_tiles(vb):
    """n beyond 262,144: tiles of 1,024 points, four 256-point parts each, a last tile of one
    point; one trial."""
    n, d, K = T.LARGE
    assert T.tile_points(n, d) == 1024 and n % 1024 == 1
    T.scenario_shape(T.DEVICE, n, d, K)
    X, w, j0, u = W.case(n, d, K, 3)
    T.against_walker(X, w, K, j0, u)


def test_singletons(vb):
    T.scenario_singletons(T.DEVICE)


def test_weightless_cluster_and_zero_weights(vb):
    T.scenario_weightless(T.DEVICE)


def test_emptied_cluster_goes_to_the_block_schedule(vb):
    T.scenario_emptied(T.DEVICE)


def test_bad_and_degenerate_are_contained(vb):
    """Nothing is provoked beyond a status code: the kernels end such a trial by their own
    tests on the inputs."""
    T.scenario_contained(T.DEVICE)


@pytest.mark.parametrize("R", [1, 3, 20])
def test_batching_bit_for_bit(vb, R):
    """R = 20 leaves a ragged last group of trials (groups of 8)."""
    T.scenario_batching(T.DEVICE, R)


def test_limits(vb):
    X, w = W.blobs(40, 2, 2, 1)
    T.run_cluster(T.DEVICE, X, w, 33, [0], [np.zeros(32)], expect=-2)
    T.run_cluster(T.DEVICE, np.zeros((40, 17)), w, 2, [0], [[0.5]], expect=-2)
    T.run_seed(T.DEVICE, X, 33, [0], [np.zeros(32)], expect=-2)
    T.run_seed(T.DEVICE, np.zeros((40, 17)), 2, [0], [[0.5]], expect=-2)
    base = vb.synth_base_set(6, 2, 2, 2, vb.COV_FULL, seed=3)
    with pytest.raises(ValueError, match="K <= 32"):
        vb.h3m.wtkmeans_init_batch(base, vb.default_options(33, 2, 2, Nv=10), [1], DEV, schedule="tiled")
    with pytest.raises(ValueError, match="S <= 32"):
        vb.h3m.gmmnew_init_batch(base, vb.default_options(2, 33, 2, Nv=10), [1], DEV, schedule="tiled")
    C = np.ones((40, 17))
    with pytest.raises(ValueError, match="d <= 16"):
        vb.h3m.gmm_mix_hier_em_batch(np.zeros((40, 17)), C, False, 2, 100.0, 3, [1], DEV, schedule="tiled")


def test_wtkmeans_init_batch_tiled(vb):
    """wtkmeans_init_batch(schedule='tiled') against wtkmeans_init and against the block
    schedule, whatever the chunking."""
    h3m = vb.h3m
    base = vb.synth_base_set(9, 3, 2, 2, vb.COV_FULL, seed=21)
    o = vb.default_options(4, 3, 2, Nv=10, seed=1)
    pts = h3m.wtkmeans_points(base, "r0")
    seeds = [s for s in range(100, 160) if W.admissible(vb, base, o, s)][:12]
    want = [h3m.wtkmeans_init(base, o, s, pts) for s in seeds]
    got = h3m.wtkmeans_init_batch(base, o, seeds, DEV, schedule="tiled")
    block = h3m.wtkmeans_init_batch(base, o, seeds, DEV)
    for a, b, c in zip(got, want, block):
        W.posterior_equal(a, b, pts[0].shape[0], np.abs(pts[0]).max())
        W.posterior_equal(a, c, pts[0].shape[0], np.abs(pts[0]).max())
    for chunk in (1, 7):
        ch = h3m.wtkmeans_init_batch(base, o, seeds, DEV, chunk_trials=chunk, schedule="tiled")
        for a, b in zip(got, ch):
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("alpha", "eta", "epsilon", "m", "W"))
    big = vb.synth_base_set(300, 4, 4, 8, vb.COV_FULL, seed=31)
    ob = vb.default_options(4, 3, 8, Nv=10, seed=1, v0=10.0)
    sb = [s for s in range(10, 30) if W.admissible(vb, big, ob, s)][:3]
    pb = h3m.wtkmeans_points(big, "r0")
    for a, s in zip(h3m.wtkmeans_init_batch(big, ob, sb, DEV, schedule="tiled"), sb):
        W.posterior_equal(a, h3m.wtkmeans_init(big, ob, s, pb), pb[0].shape[0], np.abs(pb[0]).max())


def _points_of(base):
    bn = base.numpy()
    ns = bn["nstates"]
    return (np.concatenate([bn["centres"][i, :int(ns[i])] for i in range(base.N)]),
            np.concatenate([bn["covars"][i, :int(ns[i])] for i in range(base.N)]))


def test_gmmnew_init_batch_tiled(vb):
    """gmmnew_init_batch(schedule='tiled') against gmmnew_init at d = 2, 3, 8: the seeding by
    vbhem_wtk_seed_tiled_batch, the EM from its centres; the Lloyd passes and E-steps of the
    block schedule's call."""
    h3m = vb.h3m
    for covmode, mode, d, N, Sb in ((vb.COV_FULL, "r0", 2, 30, 3), (vb.COV_DIAG, "u0", 3, 30, 3),
                                    (vb.COV_FULL, "r0", 8, 150, 4)):
        base = vb.synth_base_set(N, 3, Sb, d, covmode, seed=21)
        o = vb.default_options(3, 3, d, Nv=10, seed=1, covmode=covmode, initopt_mode=mode, v0=d + 3.0)
        X, C = _points_of(base)
        full = covmode == vb.COV_FULL
        seeds = []
        for s in range(100, 130):
            try:
                G.ref_fit(X, C, full, 3, o["Nv"] * base.N, 30, *G.draws_of(s, X.shape[0], 3))
            except AssertionError:
                continue
            seeds.append(s)
        seeds = seeds[:4]
        assert len(seeds) == 4
        info, binfo = {}, {}
        got = h3m.gmmnew_init_batch(base, o, seeds, DEV, info=info, schedule="tiled")
        h3m.gmmnew_init_batch(base, o, seeds, DEV, info=binfo)
        assert info["replayed"] == [] and info["esteps"] == binfo["esteps"]
        for a, s in zip(got, seeds):
            G.posterior_close(a, h3m.gmmnew_init(base, o, s), X.shape[0], X, C, full)
        ch = h3m.gmmnew_init_batch(base, o, seeds, DEV, chunk_trials=3, schedule="tiled")
        for a, b in zip(got, ch):
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("alpha", "eta", "epsilon", "m", "W"))


@pytest.mark.parametrize("initmode", ["wtkmeans", "gmmNew"])
def test_cluster_tiled_init_equals_host(vb, initmode):
    """vbhem_h3m_c on the planted HMMs, 5 trials: init_schedule='tiled' under
    init_engine='device' gives the host path's best trial and labels, every trial's bound
    within 1e-8 relative (the bar of test_wtk_init_gpu.py and test_gmmnew_init_gpu.py)."""
    from vbhem_amd import cluster, vhem
    hmms, _ = vhem.planted_hmms(20, seed=3)
    base = vhem.hmms_to_h3m(hmms, "full")
    opt = dict(alpha0=1e6, eta0=1.0, epsilon0=1.0, lambda0=1.0, v0=5.0, W0=1.0, m0=[1.5, 1.5], tau=20, Nv=100,
               seed=1001, trials=5, max_iter=30, minDiff=1e-5, learn_hyps=0, initmode=initmode)
    o = vb.default_options(2, 2, 2, **opt)
    host = cluster.vbhem_h3m_c(base, dict(o, init_engine="host"), DEV)
    dev = cluster.vbhem_h3m_c(base, dict(o, init_engine="device", init_schedule="tiled"), DEV)
    print("bounds host", host["LLall"], "tiled", dev["LLall"])
    assert dev["best"] == host["best"] and np.array_equal(dev["label"], host["label"])
    np.testing.assert_allclose(dev["LLall"], host["LLall"], rtol=1e-8)
    with pytest.raises(ValueError, match="init_schedule"):
        cluster.vbhem_h3m_c(base, dict(o, init_engine="device", init_schedule="grid"), DEV)
    if initmode == "wtkmeans":      # 'auto' hands the schedule to both initialisations
        auto = cluster.vbhem_h3m_cluster(None, 2, 2, dict(opt, initmode="auto", trials=2, init_engine="device",
                                                           init_schedule="tiled"), DEV, base=base)
        assert np.isfinite(auto["init_trials_LL"]).all()
