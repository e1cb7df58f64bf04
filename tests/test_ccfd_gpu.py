"""CCFD clustering on the GPU (vbhem_amd/ccfd.py over the kernels of vbhmm_ccfd.hip):
the fused distance against the restatement (tests/ccfd_ref.py) at RTOL_PAIRS under
conftest.stat_err -- the bound and the metric tests/test_score_gpu.py holds
kld_matrix to --, its packing and tile edges, its memory, the density-peak passes
against the restatement exactly, and the search end to end."""
import ctypes

import numpy as np
import pytest
import torch

import ccfd_ref as cr
import ppk_ref as pr
import score_ref as sr
from conftest import RTOL_PAIRS, stat_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ccfd(vb, capi_lib):
    from vbhem_amd import ccfd as mod
    return mod


@pytest.fixture(scope="module")
def score(vb, capi_lib):
    from vbhem_amd import score as mod
    return mod


# ----------------------------------------------------------------------------
# the distance
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sr.SHAPES, ids=sr.shape_id)
def test_distance_matches_restatement(ccfd, shape):
    K, d, diag = shape
    hmms, data, ref = cr.distance_case(K, d, diag)
    assert min(len(s) for g in data for s in g) == 1 and np.isfinite(ref).all()
    D = ccfd.distance_matrix(hmms, data, device=DEV)
    assert D.dtype == torch.float64 and D.device.type == "cuda" and tuple(D.shape) == (3, 3)
    D = D.cpu().numpy()
    print("distance err", stat_err(D, ref))
    assert stat_err(D, ref) < RTOL_PAIRS
    assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()


SEGMENTS = [3, 130, 1, 128, 127]   # inside a tile, past it, packed, filling it, one short of it


@pytest.fixture(scope="module")
def tile_case():
    """33 two-state HMMs in two dimensions, subject i with SEGMENTS[i % 5] trials of 1 to 3
    observations."""
    rng = np.random.default_rng(5)
    hmms = [sr.make_hmm(rng, 2, 2, False) for _ in range(33)]
    data = [sr.sample_data(rng, [h], [int(v) for v in rng.integers(1, 4, SEGMENTS[i % 5])], 2)
            for i, h in enumerate(hmms)]
    return hmms, data


@pytest.fixture(scope="module")
def tile_results(ccfd, tile_case):
    hmms, data = tile_case
    return {H: ccfd.distance_matrix(hmms[:H], data[:H], device=DEV).cpu().numpy() for H in (2, 5, 33)}


def unfused(score, hmms, data):
    K = score.kld_matrix(hmms, data, device=DEV).cpu().numpy()
    S = 0.5 * (K + K.T)
    np.fill_diagonal(S, 0.0)
    return S


@pytest.mark.parametrize("H", [2, 5, 33])
def test_distance_packing_and_tile_edges(ccfd, score, tile_case, tile_results, H):
    hmms, data = tile_case
    D = tile_results[H]
    assert D.shape == (H, H) and np.array_equal(D, D.T) and (np.diag(D) == 0).all() and np.isfinite(D).all()
    want = unfused(score, hmms[:H], data[:H])
    print("against kld_matrix", stat_err(D, want))
    assert stat_err(D, want) < RTOL_PAIRS
    if H <= 5:
        ref = cr.distance(hmms[:H], data[:H])
        print("against the restatement", stat_err(D, ref))
        assert stat_err(D, ref) < RTOL_PAIRS
    # a segment's sum does not depend on H or on what the segment is packed with
    assert np.array_equal(D[:2, :2], tile_results[2])
    if H == 33:
        assert np.array_equal(D[:5, :5], tile_results[5])
    # two runs are bitwise equal
    again = ccfd.distance_matrix(hmms[:H], data[:H], device=DEV).cpu().numpy()
    assert np.array_equal(D, again)


def test_distance_empty_segment_is_nan(ccfd, score, tile_case):
    hmms, data = tile_case
    pick = [0, 2, 4]
    data3 = [data[0], [], data[4]]
    D = ccfd.distance_matrix([hmms[i] for i in pick], data3, device=DEV).cpu().numpy()
    K = score.kld_matrix([hmms[i] for i in pick], data3, device=DEV).cpu().numpy()
    assert np.isnan(K[1]).all()
    assert np.isnan(D[1, [0, 2]]).all() and np.isnan(D[[0, 2], 1]).all() and (np.diag(D) == 0).all()
    assert np.isfinite(D[0, 2]) and D[0, 2] == D[2, 0]
    assert stat_err(D[0, 2], 0.5 * (K[0, 2] + K[2, 0])) < RTOL_PAIRS
    # an empty trial: NaN as well
    data3 = [data[0], [np.zeros((0, 2))] + list(data[2]), data[4]]
    D = ccfd.distance_matrix([hmms[i] for i in pick], data3, device=DEV).cpu().numpy()
    assert np.isnan(D[1, [0, 2]]).all() and np.isfinite(D[0, 2])


@pytest.mark.parametrize("c", [1, 3])
def test_distance_row_does_not_depend_on_position(ccfd, tile_case, c):
    """Subject X (c trials) first, or after the 127 trials of subject Y: with c = 1 X is
    packed into Y's tile at its last lane, with c = 3 it opens the next tile."""
    hmms, data = tile_case
    X, Y, Z = (hmms[0], data[0][:c]), (hmms[4], data[4]), (hmms[2], data[2])
    assert len(Y[1]) == 127
    A = ccfd.distance_matrix([X[0], Y[0], Z[0]], [X[1], Y[1], Z[1]], device=DEV).cpu().numpy()
    B = ccfd.distance_matrix([Y[0], X[0], Z[0]], [Y[1], X[1], Z[1]], device=DEV).cpu().numpy()
    assert A[0, 1] == B[1, 0] and A[0, 2] == B[1, 2] and A[1, 2] == B[0, 2]


def test_distance_memory(ccfd, score):
    """H = 512 subjects of 8 trials: the peak stays below the [H][N_total] matrix that
    must not be built (16 MB); D itself is 2 MB."""
    H, per, T = 512, 8, 5
    rng = np.random.default_rng(9)
    hmms = [sr.make_hmm(rng, 3, 2, False) for _ in range(H)]
    data = [[rng.uniform(0, 4, (T, 2)) for _ in range(per)] for _ in range(H)]
    hset = score.HmmSet(hmms, DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    D = ccfd.distance_matrix(hset, data, device=DEV)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise", rise, "bound", H * H * per * 8)
    assert rise < H * (H * per) * 8
    assert bool(torch.isfinite(D).all()) and torch.equal(D, D.T)
    # three of its entries against the pairwise restatement
    pairs = ((0, 1), (17, 300), (511, 256))
    ref = [cr.distance([hmms[i], hmms[j]], [data[i], data[j]])[0, 1] for i, j in pairs]
    assert stat_err([float(D[i, j]) for i, j in pairs], ref) < RTOL_PAIRS


def test_distance_c_abi_and_row_extrema(score):
    """The C-ABI through plain host arrays (tests/ccfdcheck): the kernels themselves, and
    the per-row minimum and maximum over j > i."""
    lib = cr.load_ccfdcheck()
    hmms, data, ref = cr.distance_case(9, 3, False)
    rc, D, mn, mx = cr.run_distance_check(lib, score.pack_hmms(hmms), data, 3, device=True)
    assert rc == 0 and stat_err(D, ref) < RTOL_PAIRS
    assert mn[0] == min(D[0, 1], D[0, 2]) and mx[0] == max(D[0, 1], D[0, 2]) and mn[1] == mx[1] == D[1, 2]
    assert mn[2] == np.inf and mx[2] == -np.inf


def test_unsupported_sizes_are_rejected(ccfd, score):
    from vbhem_amd import _capi
    rng = np.random.default_rng(1)
    hset = score.HmmSet([sr.make_hmm(rng, 2, 2, False) for _ in range(2)], DEV)
    with pytest.raises(ValueError, match="one list of sequences per HMM"):
        ccfd.distance_matrix(hset, [[np.zeros((2, 2))]], device=DEV)
    lib = _capi.lib()
    desc = _capi.ScoreHmmsT(2, 17, 2, 1, 0, 0, 0, 0, 0)
    sd = _capi.SeqsT(0, 2, 0, 0, 0)
    assert lib.vbhmm_ccfd_distance(ctypes.byref(desc), 0, ctypes.byref(sd), 0, 0, 0, 0, 0, 0, 0) == -2


# ----------------------------------------------------------------------------
# the passes
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("N", cr.PASS_SIZES)
def test_passes_equal_restatement(ccfd, N):
    D, dcs, cl, rho_b, want = cr.pass_case(N)
    eng = ccfd.DeviceEngine(torch.from_numpy(np.array(D)).to(DEV))
    mn, mx, maxd = eng.stats()
    assert (mn, mx, maxd) == (want["rowmin"].min(), want["rowmax"][:-1].max(), want["maxd"])
    assert np.array_equal(eng._rowmin.cpu().numpy(), want["rowmin"])
    assert np.array_equal(eng._rowmax.cpu().numpy(), want["rowmax"])
    rho = eng.rho(dcs)                                  # three cut-offs, one read of D
    assert np.array_equal(rho, want["rho"])
    assert all(np.array_equal(eng.rho([dc])[0], rho[c]) for c, dc in enumerate(dcs))
    ranks = [ccfd.rank_of(r) for r in rho]
    assert np.array_equal(np.stack(ranks), want["rank"])
    delta, nneigh = eng.delta(ranks, maxd)
    assert delta.tobytes() == want["delta"].tobytes() and np.array_equal(nneigh, want["nneigh"])
    for c in range(3):
        d1, n1 = eng.delta([ranks[c]], maxd)
        assert d1[0].tobytes() == delta[c].tobytes() and np.array_equal(n1[0], nneigh[c])
    if N >= 3:   # row 0 lies at the largest distance from every point: no neighbour below maxd
        assert (nneigh[:, 0] == -1).all() and (delta[:, 0] == np.where(want["rank"][:, 0] == 0, -1, maxd)).all()
    assert np.array_equal(eng.border(dcs[0], cl, rho_b), want["border"])
    assert N < 63 or want["border"].max() > 0
    assert not eng.border(dcs[0], np.zeros(N, dtype=np.int64), rho_b).any()    # one cluster
    # the cut-off that equals an entry: the border test takes it, rho does not
    assert np.array_equal(eng.border(dcs[1], cl, rho_b), cr.passes_restated(D, [dcs[1]], cl, rho_b)["border"])
    assert np.array_equal(ccfd.NumpyEngine(np.array(D)).rho(dcs), rho)


def test_passes_through_the_c_abi():
    lib = cr.load_ccfdcheck()
    D, dcs, cl, rho_b, want = cr.pass_case(65)
    rc, got = cr.run_passes_device(lib, D, dcs, want["rank"], want["maxd"], cl, rho_b)
    assert rc == 0
    for k in ("rowmin", "rowmax", "rho", "nneigh", "border"):
        assert np.array_equal(got[k], want[k]), k
    assert got["delta"].tobytes() == want["delta"].tobytes()


# ----------------------------------------------------------------------------
# the search
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("G,per,seed", cr.PLANTED)
def test_planted_device_engine_equals_restatement(ccfd, G, per, seed):
    D, _ = cr.planted(G, per, seed)
    got = ccfd.myccfd_from_dist(torch.from_numpy(np.array(D)).to(DEV))
    assert got["ccfd_result"]["dist"].device.type == "cuda"
    cr.check_planted(got, G, per, seed)
    assert got["ccfd_result"]["fitness"] == ccfd.myccfd_from_dist(np.array(D))["ccfd_result"]["fitness"]


def test_errors_on_the_device(ccfd):
    bad = np.array(cr.planted(2, 20, 1)[0])
    bad[3, 5] = bad[5, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ccfd.myccfd_from_dist(torch.from_numpy(bad).to(DEV))
    with pytest.raises(ccfd.NoSingularPoints):
        ccfd.myccfd_from_dist(torch.from_numpy(2.5 * (1 - np.eye(70))).to(DEV))
    with pytest.raises(ValueError, match="at least 2"):
        ccfd.CCFD(torch.zeros((1, 1), dtype=torch.float64, device=DEV), 10)


def test_end_to_end(ccfd):
    """Two families of 8 three-state HMMs (ppk_ref.families over score_ref.make_hmm), 10
    sampled trials each: distance and search on the device equal the restatement's
    search on that same matrix; purity is asserted at the value the restatement reaches
    on the restatement's own distance."""
    hmms, fam = pr.families(3, 2, 2, 8, seed=0)
    rng = np.random.default_rng(77)
    data = [sr.sample_data(rng, [h], [int(v) for v in rng.integers(1, 9, 10)], 2) for h in hmms]
    got = ccfd.myccfd(hmms, data, device=DEV)
    g = got["ccfd_result"]
    D = g["dist"].cpu().numpy()
    ref_D = cr.distance(hmms, data)
    print("distance err", stat_err(D, ref_D))
    assert stat_err(D, ref_D) < RTOL_PAIRS and np.array_equal(D, D.T)
    ref = cr.myccfd_from_dist(D)
    r = ref["ccfd_result"]
    for k in ("rho", "icl", "cl", "halo"):
        assert np.array_equal(g[k], r[k]), k
    assert g["delta"].tobytes() == r["delta"].tobytes()
    assert cr.rel_close(g["dc"], r["dc"]) and cr.rel_close(g["fitness"], r["fitness"])
    assert g["percent"] == r["percent"] and g["NCLUST"] == r["NCLUST"]
    assert np.array_equal(got["label"], ref["label"]) and np.array_equal(got["weight"], ref["weight"])
    assert [h is hmms[i] for h, i in zip(got["hmms"], g["icl"])] == [True] * g["NCLUST"]
    own = cr.myccfd_from_dist(ref_D)
    print("purity", cr.purity(got["label"], fam), "the restatement's", cr.purity(own["label"], fam))
    assert cr.purity(got["label"], fam) == cr.purity(own["label"], fam)
