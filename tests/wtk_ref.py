"""What the batched 'wtkmeans' initialisation tests share: the inputs, the reference with
its conditions, the loader of the check build (tests/wtkcheck) and the comparisons.

Reference: h3m.kmeans_pp, h3m.weighted_kmeans and h3m.wtkmeans_init, unchanged.  kmeans_pp
gets a generator double (Draws) that returns the injected first index and performs numpy's
choice(n, p = ...) -- cdf = cumsum(p), cdf /= cdf[-1], searchsorted(cdf, u, 'right') -- with
the injected uniform draw; test_wtk_init.py checks the double against a real generator.
While the reference runs, h3m's numpy is watched (traced()): every argmin and every D2 draw
is recorded, so that the conditions under which exact label equality means something are
computed on the reference itself and asserted for every input:
  * at every assignment the two smallest candidates lie more than GAP = 1e-9 apart,
    relative to the second (a column whose second candidate is +Inf has no rival; all
    +Inf picks cluster 0 on both sides);
  * every D2 draw lies more than GAP from its neighbouring cdf values;
  * no |dE| of weighted_kmeans lies in [0.5e-6, 2e-6].
An input that fails one of them is replaced by another one, never excused.

Tolerance: labels, counts, iteration counts and statuses are equal; centres and energies
agree within 100 n 2^-53 of the largest |coordinate| (energies: of the largest of that and
the largest energy), the bound of n-term sums in another order.
"""
import contextlib
import ctypes
import os
import subprocess

import numpy as np

import pkgload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_PATH = os.path.join(ROOT, "tests", "wtkcheck", "libwtkcheck.so")
OK, DEGENERATE, BAD = 0, 1, 2
GAP = 1e-9
HOST, DEVICE = 0, 1
BLOCK = 256      # the kernels' block stride (csrc/vbhem_wtk_run.h kBlock)

_cache = {}


def h3m():
    pkgload.load()
    from vbhem_amd import h3m as mod
    return mod


def tol(n):
    return 100.0 * n * 2.0 ** -53


# ----------------------------------------------------------------------------
# the reference, watched
# ----------------------------------------------------------------------------
class Trace:
    def __init__(self):
        self.gaps, self.draws, self.reseeds, self.passes = [], [], 0, 0


class _Numpy:
    """numpy as h3m sees it while traced: argmin and argmax record what they decide."""

    def __init__(self, trace):
        self._t = trace

    def __getattr__(self, name):
        return getattr(np, name)

    def argmin(self, x, axis=None):
        x = np.asarray(x)
        self._t.passes += 1
        if axis == 0 and x.ndim == 2 and x.shape[0] > 1:
            two = np.partition(x, 1, axis=0)[:2]
            with np.errstate(invalid="ignore"):
                gap = np.where(np.isinf(two[1]), 1.0, (two[1] - two[0]) / np.maximum(np.abs(two[1]), 1e-300))
            self._t.gaps.append(float(gap.min()))
        return np.argmin(x, axis=axis)

    def argmax(self, x, axis=None):
        self._t.reseeds += 1
        return np.argmax(x, axis=axis)


@contextlib.contextmanager
def traced():
    mod, t = h3m(), Trace()
    mod.np = _Numpy(t)
    try:
        yield t
    finally:
        mod.np = np


class Draws:
    """The generator double of kmeans_pp: integers() returns j0, choice(n, p) searches the
    cdf with the next injected uniform draw and records its distance to the cdf values
    around it."""

    def __init__(self, j0, u, trace=None):
        self.j0, self.u, self.i, self.t, self.first = int(j0), list(np.atleast_1d(u)), 0, trace, True

    def integers(self, n):
        assert self.first, "the reference took its degenerate branch"
        self.first = False
        return self.j0

    def choice(self, n, p):
        u = self.u[self.i]
        self.i += 1
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        j = int(np.searchsorted(cdf, u, side="right"))
        if self.t is not None:
            lo = cdf[j - 1] if j > 0 else -1.0
            self.t.draws.append(float(min(u - lo, cdf[j] - u)))
        return j


def draws_of(seed, n, k):
    """What a PCG64(seed) generator gives kmeans_pp on n points for k centres."""
    g = np.random.Generator(np.random.PCG64(seed))
    return int(g.integers(n)), np.array([g.random() for _ in range(k - 1)] + [0.0] * (k == 1))


def ref_pp(X, k, j0, u):
    """h3m.kmeans_pp from the injected draws: (centres, trace), the conditions asserted."""
    with traced() as t:
        cen = h3m().kmeans_pp(X, k, Draws(j0, u, t))
    assert all(g > GAP for g in t.gaps), ("assignment gap", min(t.gaps))
    assert all(g > GAP for g in t.draws), ("draw margin", min(t.draws))
    return cen, t


def ref_wk(X, w, K, cen0, it_max=100):
    """h3m.weighted_kmeans: (labels, centres, energies, the last energy computed)."""
    with traced() as t:
        lab, cen, en = h3m().weighted_kmeans(K, it_max, X, w, cen0)
    assert all(g > GAP for g in t.gaps), ("assignment gap", min(t.gaps))
    last = float((w * ((X - cen[lab]) ** 2).sum(1)).sum())
    steps = np.abs(np.diff(np.append(en, last)))
    assert not ((steps >= 0.5e-6) & (steps <= 2e-6)).any(), ("energy step", steps)
    return lab, cen, en, last


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def blobs(n, d, K, seed, spread=6.0):
    """n points around K random centres in [0, 40]^d with uneven weights."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.0, 40.0, (max(K, 1), d))
    X = mu[rng.integers(0, max(K, 1), n)] + spread * rng.normal(size=(n, d))
    w = rng.uniform(0.2, 1.0, n)
    return np.ascontiguousarray(X), w / w.sum()


# (n, d, K, S): the demo's size, the edges of a block stride, every dimension bucket, the
# limits of K and S, and the two strided cases
SHAPES = [(30, 2, 3, 3), (BLOCK - 1, 2, 3, 3), (BLOCK, 3, 2, 1), (BLOCK + 1, 2, 3, 3), (2 * BLOCK + 1, 3, 2, 3),
          (300, 2, 1, 3), (400, 8, 16, 3), (700, 16, 32, 16), (8000, 2, 8, 3), (4099, 8, 16, 3)]


def case(n, d, K, S, seed=None):
    """Points, weights and a first-stage draw whose reference passes the conditions: the
    first seed from ``seed`` that does."""
    key = ("case", n, d, K, S, seed)
    if key not in _cache:
        base = 7 * n + 3 * d + K if seed is None else seed
        X, w = blobs(n, d, K, base)
        for s in range(base, base + 20):
            j0, u = draws_of(s, n, K)
            try:
                cen, _ = ref_pp(X, K, j0, u)
                ref_wk(X, w, K, cen)
            except AssertionError:
                continue
            _cache[key] = (X, w, j0, u)
            break
        else:
            raise AssertionError(f"no admissible draw for {key}")
    return _cache[key]


def draws_for(X, picks):
    """The draws that make kmeans_pp start from the points ``picks``: the first index and,
    per further centre, the middle of its interval of the cdf (None if a pick has d2 = 0)."""
    d2, u = ((X - X[picks[0]]) ** 2).sum(1), []
    for c in picks[1:]:
        if d2[c] <= 0:
            return None
        cdf = np.cumsum(d2 / d2.sum())
        cdf /= cdf[-1]
        u.append(0.5 * ((cdf[c - 1] if c > 0 else 0.0) + cdf[c]))
        d2 = np.minimum(d2, ((X - X[c]) ** 2).sum(1))
    return int(picks[0]), np.array(u)


def emptied_case():
    """An input on which the reference's kmeans_pp re-seeds an emptied cluster, found by a
    seed search over the reference: small point sets, the draws chosen so that the run
    starts from a random subset of the points (D2 draws of a generator hardly ever lead
    there: none in 20,000 seeds)."""
    if "emptied" not in _cache:
        for s in range(2000):
            rng = np.random.default_rng(s)
            d, n, k = int(rng.integers(1, 3)), int(rng.integers(10, 40)), int(rng.integers(3, 9))
            X = np.ascontiguousarray(rng.normal(size=(n, d)) * rng.uniform(0.2, 3, size=(1, d)))
            dr = draws_for(X, rng.choice(n, k, replace=False))
            if dr is None:
                continue
            try:
                cen, t = ref_pp(X, k, *dr)
            except AssertionError:
                continue
            if t.reseeds:
                _cache.setdefault("emptied", []).append((X, k, dr[0], dr[1], cen))
                if len(_cache["emptied"]) == 3:
                    break
        else:
            raise AssertionError("no input re-seeds")
    return _cache["emptied"]


# ----------------------------------------------------------------------------
# the check library
# ----------------------------------------------------------------------------
def load_check():
    if "lib" not in _cache:
        if not os.path.exists(CHECK_PATH):
            subprocess.run(["make", "-C", ROOT, "wtkcheck"], check=True, stdout=subprocess.DEVNULL)
        import torch  # noqa: F401  (the library binds to the HIP runtime torch loaded)
        lib = ctypes.CDLL(CHECK_PATH)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.wtkcheck_pp.argtypes = [ci, ci, ci, vp, ci, vp, ci, ci, vp, ci, vp, vp, vp, vp]
        lib.wtkcheck_wk.argtypes = [ci, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp]
        lib.wtkcheck_cluster.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp]
        lib.wtkcheck_states.argtypes = [ci, ci, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        for f in (lib.wtkcheck_pp, lib.wtkcheck_wk, lib.wtkcheck_cluster, lib.wtkcheck_states):
            f.restype = ci
        _cache["lib"] = lib
    return _cache["lib"]


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def run_pp(where, X, k, j0, u, idx=None, max_iter=100, expect=0):
    """(a) alone: dict(status, iters, cen, lab); outputs keep -7 where nothing was written."""
    X, u = _f(X), _f(np.atleast_1d(u))
    n, d = X.shape
    idx = None if idx is None else _i(idx)
    ns = n if idx is None else idx.size
    cen, lab = np.full((k, d), -7.0), np.full(ns, -7, np.int32)
    it, st = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    rc = load_check().wtkcheck_pp(where, n, d, _p(X), ns, _p(idx), k, int(j0), _p(u), max_iter, _p(cen), _p(lab),
                                  _p(it), _p(st))
    assert rc == expect, rc
    return dict(status=int(st[0]), iters=int(it[0]), cen=cen, lab=lab)


def run_wk(where, X, w, K, cen0, it_max=100):
    """(b) alone: dict(status, iters, cen, lab, energies [iters + 1], last)."""
    X, w, cen = _f(X), _f(w), _f(cen0).copy()
    n, d = X.shape
    lab, en = np.full(n, -7, np.int32), np.full(it_max + 1, -7.0)
    last, it, st = np.full(1, -7.0), np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    rc = load_check().wtkcheck_wk(where, n, d, _p(X), _p(w), K, it_max, _p(cen), _p(lab), _p(en), _p(last), _p(it),
                                  _p(st))
    assert rc == 0, rc
    k = max(int(it[0]), 0) + 1
    return dict(status=int(st[0]), iters=int(it[0]), cen=cen, lab=lab, energies=en[:k].copy(), last=float(last[0]))


def run_cluster(where, X, w, K, j0, u, chunk=0, expect=0):
    """The first stage of R trials: labels [R][n], counts [R][K], status [R], iters [R][2]."""
    X, w, j0 = _f(X), _f(w), _i(j0)
    n, d = X.shape
    R = j0.size
    u = _f(u).reshape(R, max(K - 1, 1))
    labels, counts = np.full((R, n), -7, np.int32), np.full((R, K), -7, np.int32)
    status, iters = np.full(R, -7, np.int32), np.full((R, 2), -7, np.int32)
    rc = load_check().wtkcheck_cluster(where, n, d, K, R, _p(X), _p(w), _p(j0), _p(u), chunk, _p(labels), _p(counts),
                                       _p(status), _p(iters))
    assert rc == expect, rc
    return dict(labels=labels, counts=counts, status=status, iters=iters)


def run_states(where, X, labels, K, S, trial, cluster, nmem, j0, u):
    """The second stage: centres [R][K][S][d] (-7 where no item wrote), status [I], iters [I]."""
    X, labels = _f(X), _i(labels)
    n, d = X.shape
    R, I = labels.shape[0], len(trial)
    u = _f(u).reshape(I, max(S - 1, 1))
    cen = np.full((R, K, S, d), -7.0)
    status, iters = np.full(I, -7, np.int32), np.full(I, -7, np.int32)
    rc = load_check().wtkcheck_states(where, n, d, K, S, R, _p(X), _p(labels), I, _p(_i(trial)), _p(_i(cluster)),
                                      _p(_i(nmem)), _p(_i(j0)), _p(u), _p(cen), _p(status), _p(iters))
    assert rc == 0, rc
    return dict(centres=cen, status=status, iters=iters)


class CheckEngine:
    """h3m.WtkDeviceEngine's interface over the check library: the walker (where = HOST),
    the stand-in engine of wtkmeans_init_batch on a machine without a GPU."""

    def __init__(self, where=HOST, chunk=0):
        import torch
        self.where, self.chunk, self.dev = where, chunk, torch.device("cpu")

    def cluster(self, pts, w, K, j0, u):
        self.X, self.K = pts.cpu().numpy(), K
        r = run_cluster(self.where, self.X, w.cpu().numpy(), K, j0, u, self.chunk)
        return r["labels"], r["counts"], r["status"], r["iters"]

    def labels_of(self, labels, r):
        return labels[r]

    def states(self, labels, S, trial, cluster, nmem, j0, u):
        r = run_states(self.where, self.X, labels, self.K, S, trial, cluster, nmem, j0, u)
        return r["centres"], r["status"], r["iters"]


# ----------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------
def close(a, b, n, scale):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) <= tol(n) * scale


def check_pp(where, X, k, j0, u, idx=None):
    """(a) through the walker or the kernels against h3m.kmeans_pp on the same subset."""
    sub = X if idx is None else X[np.asarray(idx)]
    ref, t = ref_pp(sub, k, j0, u)
    got = run_pp(where, X, k, j0, u, idx)
    assert got["status"] == OK
    assert close(got["cen"], ref, sub.shape[0], np.abs(sub).max()), np.abs(got["cen"] - ref).max()
    assert got["iters"] == t.passes
    return got, t


def check_wk(where, X, w, K, cen0, it_max=100):
    """(b) through the walker or the kernels against h3m.weighted_kmeans."""
    lab, cen, en, last = ref_wk(X, w, K, cen0, it_max)
    got = run_wk(where, X, w, K, cen0, it_max)
    n, big = X.shape[0], np.abs(X).max()
    assert got["status"] == OK
    assert np.array_equal(got["lab"], lab)
    assert got["iters"] == len(en) - 1
    assert close(got["cen"], cen, n, big), np.abs(got["cen"] - cen).max()
    escale = max(big, float(np.abs(en).max()))
    assert close(got["energies"], en, n, escale) and close(got["last"], last, n, escale)
    return got


def check_trial(where, X, w, K, j0, u):
    """One first-stage trial against kmeans_pp then weighted_kmeans of the reference."""
    cen, t = ref_pp(X, K, j0, u)
    lab, _, en, _ = ref_wk(X, w, K, cen)
    got = run_cluster(where, X, w, K, [j0], [u])
    assert got["status"][0] == OK
    assert np.array_equal(got["labels"][0], lab)
    assert np.array_equal(got["counts"][0], np.bincount(lab, minlength=K))
    assert got["iters"][0].tolist() == [t.passes, len(en) - 1]
    return got


def admissible(vb, base, o, seed):
    """The gap condition on every k-means wtkmeans_init runs for this seed (its D2 draws
    come from the generator itself, so their margins are covered by the equality asked of
    the result: a draw on a cdf edge would change the centres)."""
    try:
        with traced() as t:
            vb.h3m.wtkmeans_init(base, o, seed)
    except AssertionError:
        return False
    return all(g > GAP for g in t.gaps)


def posterior_equal(a, b, n, big):
    """Two Posteriors field by field: m within the tolerance, the rest equal."""
    for k in ("alpha", "eta", "epsilon", "lam", "v", "W"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.W0mode == b.W0mode
    assert close(a.m, b.m, n, big), np.abs(a.m - b.m).max()


# ----------------------------------------------------------------------------
# scenarios run by the CPU tests on the walker and by the GPU tests on the kernels
# ----------------------------------------------------------------------------
def scenario_shape(where, n, d, K, S):
    """(a) and (b) alone, a whole first-stage trial, and (a) on one cluster's members."""
    X, w, j0, u = case(n, d, K, S)
    got, _ = check_pp(where, X, K, j0, u)
    check_wk(where, X, w, K, got["cen"])
    tr = check_trial(where, X, w, K, j0, u)
    lab, cnt = tr["labels"][0], tr["counts"][0]
    c = int(np.argmax(cnt))
    if cnt[c] <= S:
        return
    idx = np.flatnonzero(lab == c)
    for s in range(20):     # a second-stage draw whose reference passes the conditions
        j2, u2 = draws_of(1000 + s, idx.size, S)
        try:
            ref, t = ref_pp(X[idx], S, j2, u2)
        except AssertionError:
            continue
        break
    else:
        raise AssertionError("no admissible second-stage draw")
    check_pp(where, X, S, j2, u2, idx)
    st = run_states(where, X, tr["labels"], K, S, [0], [c], [cnt[c]], [j2], [u2])
    assert st["status"][0] == OK and st["iters"][0] == t.passes
    assert close(st["centres"][0, c], ref, idx.size, np.abs(X).max())
    assert (np.delete(st["centres"][0], c, axis=0) == -7.0).all()


def scenario_singletons(where):
    """n = K: every cluster a singleton, so a member's own candidate is 0 cw / 0 = NaN (or
    x / 0 = Inf) and the minimum must pass over it.  (With an empty cluster left behind,
    every candidate of the next sweep would be an exact zero: such inputs fail the gap
    condition, so the seeds searched here are those whose singletons swap places.)"""
    done = 0
    for K, d in ((4, 2), (2, 3), (3, 2)):
        for s in range(300):
            rng = np.random.default_rng(s)
            X = np.ascontiguousarray(rng.uniform(0, 40, (K, d)))
            w = rng.uniform(0.2, 1.0, K)
            w /= w.sum()
            try:
                ref_wk(X, w, K, X.copy())
            except AssertionError:
                continue
            got = check_wk(where, X, w, K, X.copy())
            assert (got["lab"] != np.arange(K)).all()    # every singleton moved
            done += 1
            break
    assert done >= 2


def scenario_weightless(where):
    """A cluster whose members all weigh nothing (entered through the given centres) gets
    the zero centre and cw = 0, hence a zero adjustment: it attracts every weighted point,
    as in the reference.  Then zero-weight points among ordinary ones."""
    X, w = blobs(200, 2, 2, 77)
    X[:40] += 300.0
    w[:40] = 0.0
    w /= w.sum()
    cen0 = np.stack([X[:40].mean(0), X[40:].mean(0)])
    lab, cen, en, _ = ref_wk(X, w, 2, cen0)
    assert (lab[40:] == 0).all() and (lab[:40] == 1).all() and (cen[1] == 0.0).all()   # it did attract them
    check_wk(where, X, w, 2, cen0)
    X2, w2 = blobs(300, 3, 4, 78)
    w2[::3] = 0.0
    w2 /= w2.sum()
    j0, u = draws_of(78, 300, 4)
    got, _ = check_pp(where, X2, 4, j0, u)
    check_wk(where, X2, w2, 4, got["cen"])


def scenario_emptied(where):
    for X, k, j0, u, cen in emptied_case():
        _, t = check_pp(where, X, k, j0, u)
        assert t.reseeds >= 1


def scenario_contained(where):
    """Trials and items that are not OK write their status alone and leave the others' bits:
    a draw out of range (BAD) between ordinary trials; a NaN coordinate (BAD: the points are
    shared, so every trial); fewer distinct points than centres (DEGENERATE: likewise); and
    in the second stage a cluster of identical points (DEGENERATE) and a wrong member count
    (BAD) between ordinary items."""
    X, w, j0, u = case(300, 2, 3, 3, seed=11)
    j1, u1 = draws_of(12, 300, 3)
    alone = run_cluster(where, X, w, 3, [j0, j1], [u, u1])
    mixed = run_cluster(where, X, w, 3, [j0, 300, j1, -1], [u, u, u1, u1])
    assert mixed["status"].tolist() == [OK, BAD, OK, BAD]
    for a, b in ((0, 0), (1, 2)):
        assert all(np.array_equal(alone[k][a], mixed[k][b]) for k in ("labels", "counts", "iters"))
    for r in (1, 3):
        assert (mixed["labels"][r] == -7).all() and (mixed["counts"][r] == -7).all() and (mixed["iters"][r] == -7).all()
    Xn = X.copy()
    Xn[17, 1] = np.nan
    bad = run_cluster(where, Xn, w, 3, [j0, j1], [u, u1])
    assert bad["status"].tolist() == [BAD, BAD] and (bad["labels"] == -7).all()
    Xd = np.repeat(X[:2], 150, axis=0)
    deg = run_cluster(where, Xd, w, 3, [j0, j1], [u, u1])
    assert deg["status"].tolist() == [DEGENERATE, DEGENERATE] and (deg["labels"] == -7).all()
    # second stage: cluster 2 is eight copies of one point
    Xs = np.concatenate([X, np.repeat([[500.0, 500.0]], 8, axis=0)])
    labels = np.concatenate([alone["labels"][0] % 2, np.full(8, 2)]).astype(np.int32)[None]
    cnt = np.bincount(labels[0], minlength=3)
    j2, u2 = draws_of(13, int(cnt[0]), 3)
    j3, u3 = draws_of(14, int(cnt[1]), 3)
    good = run_states(where, Xs, labels, 3, 3, [0, 0], [0, 1], cnt[:2], [j2, j3], [u2, u3])
    both = run_states(where, Xs, labels, 3, 3, [0, 0, 0, 0], [0, 2, 1, 1], [cnt[0], 8, cnt[1] - 1, cnt[1]],
                      [j2, 3, 0, j3], [u2, u2, u3, u3])
    assert good["status"].tolist() == [OK, OK]
    assert both["status"].tolist() == [OK, DEGENERATE, BAD, OK]
    assert np.array_equal(good["centres"], both["centres"]) and (both["centres"][0, 2] == -7.0).all()
    assert both["iters"][[0, 3]].tolist() == good["iters"].tolist() and both["iters"][1] == -7


def trial_draws(seeds, n, K):
    d = [draws_of(s, n, K) for s in seeds]
    return [j for j, _ in d], np.stack([u for _, u in d])


def scenario_batching(where, R):
    """A trial's outputs bit for bit whatever R, its place, the chunking and the run."""
    X, w, _, _ = case(BLOCK + 1, 2, 3, 3)
    j0, u = trial_draws(range(50, 50 + R), X.shape[0], 3)
    base = run_cluster(where, X, w, 3, j0, u)
    keys = ("labels", "counts", "status", "iters")
    assert (base["status"] == OK).all()
    again = run_cluster(where, X, w, 3, j0, u)
    rev = run_cluster(where, X, w, 3, j0[::-1], u[::-1])
    perm = np.random.default_rng(R).permutation(R)
    shuf = run_cluster(where, X, w, 3, [j0[i] for i in perm], u[perm])
    one = run_cluster(where, X, w, 3, j0[:1], u[:1])
    for k in keys:
        assert np.array_equal(base[k], again[k]) and np.array_equal(base[k], rev[k][::-1]), k
        assert np.array_equal(base[k][perm], shuf[k]) and np.array_equal(base[k][:1], one[k]), k
    for chunk in (1, 7):
        ch = run_cluster(where, X, w, 3, j0, u, chunk=chunk)
        assert all(np.array_equal(base[k], ch[k]) for k in keys), chunk
    return base
