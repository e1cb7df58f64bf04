"""What the tests of the TILED schedule of the initialisations' k-means share
(csrc/vbhem_wtk_tiled.hip, csrc/vbhem_wtk_tiled_run.h): the loader of the check build
(tests/wtktilecheck), the stand-in engines backed by the serial tiled walker, and the
scenarios the CPU tests run on the walker and the GPU tests on the kernels.

Reference, inputs, conditions and tolerances are those of tests/wtk_ref.py and
tests/ghem_ref.py, imported unchanged: h3m.kmeans_pp and h3m.weighted_kmeans run under the
watchers there (assignment gaps and draw margins above 1e-9, no energy step in
[0.5e-6, 2e-6]); labels, counts, statuses and both iteration counts are equal, centres agree
within wtk_ref.tol(n) of the largest |coordinate|.
"""
import ctypes
import os
import subprocess

import numpy as np

import ghem_ref as G
import wtk_ref as W

CHECK_PATH = os.path.join(W.ROOT, "tests", "wtktilecheck", "libwtktilecheck.so")
OK, DEGENERATE, BAD = W.OK, W.DEGENERATE, W.BAD
HOST, DEVICE = W.HOST, W.DEVICE
KEYS = ("labels", "counts", "status", "iters")

# (n, d, K): the demo's size; one tile short of full, full, a last tile of one point, three
# tiles; every dimension bucket; K = 1, the limits of d and K
SHAPES = [(30, 2, 3), (255, 2, 3), (256, 3, 2), (257, 2, 3), (513, 3, 2), (257, 2, 1), (513, 8, 8), (257, 8, 32),
          (513, 16, 32), (256, 16, 3)]
# past the tile-size switch: tiles of 1,024 points, a last tile of one point
LARGE = (262144 + 1025, 2, 2)

_cache = {}


def load_check():
    if "lib" not in _cache:
        if not os.path.exists(CHECK_PATH):
            subprocess.run(["make", "-C", W.ROOT, "wtktilecheck"], check=True, stdout=subprocess.DEVNULL)
        import torch  # noqa: F401  (the library binds to the HIP runtime torch loaded)
        lib = ctypes.CDLL(CHECK_PATH)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.wtktilecheck_tile_points.argtypes = [ci, ci]
        lib.wtktilecheck_rounds.argtypes = [ci, ci]
        lib.wtktilecheck_cluster.argtypes = [ci] * 5 + [vp] * 4 + [ci] + [vp] * 6
        lib.wtktilecheck_seed.argtypes = [ci] * 5 + [vp] * 3 + [ci] + [vp] * 5
        for f in (lib.wtktilecheck_tile_points, lib.wtktilecheck_rounds, lib.wtktilecheck_cluster,
                  lib.wtktilecheck_seed):
            f.restype = ci
        _cache["lib"] = lib
    return _cache["lib"]


def tile_points(n, d):
    return load_check().wtktilecheck_tile_points(n, d)


def rounds_of(K, seed_only):
    return load_check().wtktilecheck_rounds(K, int(seed_only))


def run_cluster(where, X, w, K, j0, u, chunk=0, expect=0):
    """The first stage of R trials by the tiled schedule: labels [R][n], counts [R][K],
    status [R], iters [R][2]; reseed [R], rounds [R] (the walker's; -7 from the device);
    outputs keep -7 where nothing was written."""
    X, w, j0 = W._f(X), W._f(w), W._i(j0)
    n, d = X.shape
    R = j0.size
    u = W._f(u).reshape(R, max(K - 1, 1))
    labels, counts = np.full((R, n), -7, np.int32), np.full((R, K), -7, np.int32)
    status, iters = np.full(R, -7, np.int32), np.full((R, 2), -7, np.int32)
    reseed, rounds = np.full(R, -7, np.int32), np.full(R, -7, np.int32)
    rc = load_check().wtktilecheck_cluster(where, n, d, K, R, W._p(X), W._p(w), W._p(j0), W._p(u), chunk, W._p(labels),
                                           W._p(counts), W._p(status), W._p(iters), W._p(reseed), W._p(rounds))
    assert rc == expect, rc
    return dict(labels=labels, counts=counts, status=status, iters=iters, reseed=reseed, rounds=rounds)


def run_seed(where, X, K, j0, u, chunk=0, expect=0):
    """kmeans_pp alone of R trials by the tiled schedule: centres [R][K][d], status [R],
    iters [R] (Lloyd passes), reseed [R], rounds [R]."""
    X, j0 = W._f(X), W._i(j0)
    n, d = X.shape
    R = j0.size
    u = W._f(u).reshape(R, max(K - 1, 1))
    cen = np.full((R, K, d), -7.0)
    status, iters = np.full(R, -7, np.int32), np.full(R, -7, np.int32)
    reseed, rounds = np.full(R, -7, np.int32), np.full(R, -7, np.int32)
    rc = load_check().wtktilecheck_seed(where, n, d, K, R, W._p(X), W._p(j0), W._p(u), chunk, W._p(cen), W._p(status),
                                        W._p(iters), W._p(reseed), W._p(rounds))
    assert rc == expect, rc
    return dict(centres=cen, status=status, iters=iters, reseed=reseed, rounds=rounds)


class WtkEngine(W.CheckEngine):
    """wtk_ref.CheckEngine with the first stage by the tiled walker: the stand-in for
    h3m.WtkDeviceEngine(schedule='tiled') on a machine without a GPU."""

    def __init__(self, where=HOST, chunk=0):
        super().__init__(where, chunk)
        self.schedule, self.calls = "tiled", 0

    def cluster(self, pts, w, K, j0, u):
        self.calls += 1
        self.X, self.K = pts.cpu().numpy(), K
        r = run_cluster(self.where, self.X, w.cpu().numpy(), K, j0, u, self.chunk)
        return r["labels"], r["counts"], r["status"], r["iters"]


class GhemEngine(G.CheckEngine):
    """ghem_ref.CheckEngine with the tiled seeding (the walker): the stand-in for
    h3m.GhemDeviceEngine under schedule='tiled'."""

    def __init__(self, device=None, chunk_trials=None, where=HOST):
        super().__init__(device, chunk_trials, where)
        self.seeds = 0

    def seed(self, X, T, j0, u):
        self.seeds += 1
        r = run_seed(self.where, X, T, j0, u, self.chunk)
        return r["centres"], r["status"], r["iters"]


# ----------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------
def check_trial(where, X, w, K, j0, u):
    """One first-stage trial by the tiled schedule against kmeans_pp then weighted_kmeans of
    the reference, and against the block schedule's walker."""
    cen, t = W.ref_pp(X, K, j0, u)
    lab, _, en, _ = W.ref_wk(X, w, K, cen)
    got = run_cluster(where, X, w, K, [j0], [u])
    assert got["status"][0] == OK
    assert np.array_equal(got["labels"][0], lab)
    assert np.array_equal(got["counts"][0], np.bincount(lab, minlength=K))
    assert got["iters"][0].tolist() == [t.passes, len(en) - 1]
    block = W.run_cluster(HOST, X, w, K, [j0], [u])
    assert all(np.array_equal(got[k], block[k]) for k in KEYS)
    if where == HOST:
        assert got["reseed"][0] == 0 and 1 <= got["rounds"][0] <= rounds_of(K, False)
        # the rounds used: the seeding's, the Lloyd passes, the first assignment, and one
        # per energy the stopping rule read
        assert got["rounds"][0] == (K - 1) + t.passes + 1 + min(len(en) + 1, 101)
    return got


def check_seed(where, X, K, j0, u):
    """kmeans_pp alone by the tiled schedule against h3m.kmeans_pp and the block walker."""
    ref, t = W.ref_pp(X, K, j0, u)
    got = run_seed(where, X, K, [j0], [u])
    n, big = X.shape[0], np.abs(X).max()
    assert got["status"][0] == OK and got["iters"][0] == t.passes
    assert W.close(got["centres"][0], ref, n, big), np.abs(got["centres"][0] - ref).max()
    block = W.run_pp(HOST, X, K, j0, u)
    assert block["iters"] == got["iters"][0] and W.close(got["centres"][0], block["cen"], n, big)
    return got


def scenario_shape(where, n, d, K):
    X, w, j0, u = W.case(n, d, K, 3)
    tr = check_trial(where, X, w, K, j0, u)
    sd = check_seed(where, X, K, j0, u) if K >= 2 else None
    return tr, sd


def against_walker(X, w, K, j0, u):
    """The kernels against the serial tiled walker: the discrete outputs equal, the seeding's
    centres within the tolerance (the orders of all sums are the same; the margin is for the
    two compilers' arithmetic)."""
    dev, host = (run_cluster(where, X, w, K, [j0], [u]) for where in (DEVICE, HOST))
    assert all(np.array_equal(dev[k], host[k]) for k in KEYS)
    if K >= 2:
        sd, sh = (run_seed(where, X, K, [j0], [u]) for where in (DEVICE, HOST))
        assert np.array_equal(sd["status"], sh["status"]) and np.array_equal(sd["iters"], sh["iters"])
        assert W.close(sd["centres"], sh["centres"], X.shape[0], np.abs(X).max())
        print("seeding centres, kernels - walker:", float(np.abs(sd["centres"] - sh["centres"]).max()))


def singleton_cases():
    """n = K, the run started from every point (wtk_ref.draws_for), so every cluster is a
    singleton when the sweeps begin and a member's own candidate is NaN or Inf: the inputs of
    wtk_ref.scenario_singletons whose reference passes the conditions."""
    if "singletons" not in _cache:
        out = []
        for K, d in ((4, 2), (2, 3), (3, 2)):
            for s in range(300):
                rng = np.random.default_rng(s)
                X = np.ascontiguousarray(rng.uniform(0, 40, (K, d)))
                w = rng.uniform(0.2, 1.0, K)
                w /= w.sum()
                dr = W.draws_for(X, np.arange(K))
                if dr is None:
                    continue
                try:
                    cen, _ = W.ref_pp(X, K, *dr)
                    lab, _, _, _ = W.ref_wk(X, w, K, cen)
                except AssertionError:
                    continue
                assert np.array_equal(cen, X)
                out.append((X, w, K, dr[0], dr[1], lab))
                break
        _cache["singletons"] = out
    return _cache["singletons"]


def scenario_singletons(where):
    cases = singleton_cases()
    assert len(cases) >= 2
    for X, w, K, j0, u, lab in cases:
        assert (lab != np.arange(K)).all()    # every singleton moved
        check_trial(where, X, w, K, j0, u)


def scenario_weightless(where):
    """wtk_ref.scenario_weightless through a whole trial: forty far points that weigh nothing
    become a cluster of the seeding, get the zero centre and cw = 0 in the sweeps and attract
    every weighted point, as in the reference; then zero weights among ordinary points."""
    X, w = W.blobs(200, 2, 2, 77)
    X[:40] += 300.0
    w[:40] = 0.0
    w /= w.sum()
    for s in range(40):
        j0, u = W.draws_of(s, 200, 2)
        try:
            cen, _ = W.ref_pp(X, 2, j0, u)
            lab, fin, _, _ = W.ref_wk(X, w, 2, cen)
        except AssertionError:
            continue
        if (fin == 0.0).all(1).any():
            break
    else:
        raise AssertionError("no admissible draw leaves the weightless cluster")
    a, b = int(lab[40]), int(lab[0])
    assert a != b and (lab[40:] == a).all() and (lab[:40] == b).all() and (fin[b] == 0.0).all()   # it did attract them
    check_trial(where, X, w, 2, j0, u)
    X2, w2 = W.blobs(300, 3, 4, 78)
    w2[::3] = 0.0
    w2 /= w2.sum()
    for s in range(78, 98):
        j0, u = W.draws_of(s, 300, 4)
        try:
            cen, _ = W.ref_pp(X2, 4, j0, u)
            W.ref_wk(X2, w2, 4, cen)
        except AssertionError:
            continue
        break
    check_trial(where, X2, w2, 4, j0, u)


def scenario_emptied(where):
    """wtk_ref.emptied_case(): the Lloyd update empties a cluster, the trial's re-seed flag is
    set (the walker reports it) and the block schedule's result is returned -- between two
    ordinary trials, whose bits stay."""
    for X, k, j0, u, cen in W.emptied_case():
        n = X.shape[0]
        w = np.random.default_rng(n).uniform(0.2, 1.0, n)
        w /= w.sum()
        j1, u1 = W.draws_of(5, n, k)
        block = W.run_cluster(HOST, X, w, k, [j1, j0, j1], [u1, u, u1])
        got = run_cluster(where, X, w, k, [j1, j0, j1], [u1, u, u1])
        assert got["status"][1] == OK and block["status"][1] == OK
        if where == HOST:
            assert got["reseed"][1] == 1
        assert all(np.array_equal(got[key][1], block[key][1]) for key in KEYS)
        assert all(np.array_equal(got[key][0], got[key][2]) for key in KEYS)
        alone = run_cluster(where, X, w, k, [j1], [u1])
        assert all(np.array_equal(got[key][0], alone[key][0]) for key in KEYS)
        sd = run_seed(where, X, k, [j0], [u])
        assert sd["status"][0] == OK and W.close(sd["centres"][0], cen, n, np.abs(X).max())
        bp = W.run_pp(HOST, X, k, j0, u)
        assert sd["iters"][0] == bp["iters"]
        if where == HOST:
            assert sd["reseed"][0] == 1 and np.array_equal(sd["centres"][0], bp["cen"])


def scenario_contained(where):
    """Trials that are not OK write their status alone and leave the others' bits: a draw out
    of range (BAD) between ordinary trials; a NaN coordinate or weight (BAD: the points are
    shared, so every trial); fewer distinct points than centres (DEGENERATE: likewise)."""
    X, w, j0, u = W.case(300, 2, 3, 3, seed=11)
    j1, u1 = W.draws_of(12, 300, 3)
    alone = run_cluster(where, X, w, 3, [j0, j1], [u, u1])
    mixed = run_cluster(where, X, w, 3, [j0, 300, j1, -1], [u, u, u1, u1])
    assert alone["status"].tolist() == [OK, OK] and mixed["status"].tolist() == [OK, BAD, OK, BAD]
    for a, b in ((0, 0), (1, 2)):
        assert all(np.array_equal(alone[k][a], mixed[k][b]) for k in ("labels", "counts", "iters"))
    for r in (1, 3):
        assert (mixed["labels"][r] == -7).all() and (mixed["counts"][r] == -7).all() and (mixed["iters"][r] == -7).all()
    Xn = X.copy()
    Xn[17, 1] = np.nan
    bad = run_cluster(where, Xn, w, 3, [j0, j1], [u, u1])
    assert bad["status"].tolist() == [BAD, BAD] and (bad["labels"] == -7).all() and (bad["counts"] == -7).all()
    wn = w.copy()
    wn[299] = np.inf
    assert run_cluster(where, X, wn, 3, [j0, j1], [u, u1])["status"].tolist() == [BAD, BAD]
    Xd = np.repeat(X[:2], 150, axis=0)
    deg = run_cluster(where, Xd, w, 3, [j0, j1], [u, u1])
    assert deg["status"].tolist() == [DEGENERATE, DEGENERATE] and (deg["labels"] == -7).all()
    # the seeding alone
    sa = run_seed(where, X, 3, [j0, j1], [u, u1])
    sm = run_seed(where, X, 3, [j0, 300, j1, -1], [u, u, u1, u1])
    assert sm["status"].tolist() == [OK, BAD, OK, BAD]
    assert np.array_equal(sa["centres"], sm["centres"][[0, 2]]) and np.array_equal(sa["iters"], sm["iters"][[0, 2]])
    assert (sm["centres"][[1, 3]] == -7.0).all() and (sm["iters"][[1, 3]] == -7).all()
    assert run_seed(where, Xn, 3, [j0], [u])["status"].tolist() == [BAD]
    sdeg = run_seed(where, Xd, 3, [j0], [u])
    assert sdeg["status"].tolist() == [DEGENERATE] and (sdeg["centres"] == -7.0).all()


def scenario_batching(where, R):
    """A trial's outputs bit for bit whatever R, its place, the chunking and the run."""
    X, w, _, _ = W.case(W.BLOCK + 1, 2, 3, 3)
    j0, u = W.trial_draws(range(50, 50 + R), X.shape[0], 3)
    base = run_cluster(where, X, w, 3, j0, u)
    assert (base["status"] == OK).all() and (base["counts"].sum(1) == W.BLOCK + 1).all()
    again = run_cluster(where, X, w, 3, j0, u)
    rev = run_cluster(where, X, w, 3, j0[::-1], u[::-1])
    one = run_cluster(where, X, w, 3, j0[:1], u[:1])
    for k in KEYS:
        assert np.array_equal(base[k], again[k]) and np.array_equal(base[k], rev[k][::-1]), k
        assert np.array_equal(base[k][:1], one[k]), k
    sbase = run_seed(where, X, 3, j0, u)
    srev = run_seed(where, X, 3, j0[::-1], u[::-1])
    assert np.array_equal(sbase["centres"], srev["centres"][::-1]) and np.array_equal(sbase["iters"], srev["iters"][::-1])
    for chunk in (1, 7):
        ch = run_cluster(where, X, w, 3, j0, u, chunk=chunk)
        assert all(np.array_equal(base[k], ch[k]) for k in KEYS), chunk
        assert np.array_equal(sbase["centres"], run_seed(where, X, 3, j0, u, chunk=chunk)["centres"]), chunk
    return base
