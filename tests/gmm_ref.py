"""What the batched GMM fit tests share: the inputs, the reference (vbhmm_em.py
gmm_fit_randsample itself, called with a generator double that returns the injected
rows), the loader of the host check build (tests/gmmcheck) and the comparison.

Inputs:
  (a) demo subjects 0, 2 and 6, K = 2 and 3, 12 trials each, seed 100, with the rows the
      host driver drew (72 fits; the two draws that fail before their regularised refit
      are kept as fits of their own);
  (b) one dim = 3 and one dim = 8 subject from gaussian_subject, K = 2;
  (c) edge sizes: N = K + 1, N = 63, 64, 65 and 129 (the edges of a round of lanes), K = 8
      at dim = 2, start rows that include observation 0 and observation N - 1;
  (d) the planted ill-conditioned fit: 40 points from N([160, 210], 20^2) and one point at
      [1e4, 1e4], K = 2, rows [40, 3];
  (e) the corners of the kernel's buckets (corner_fits): (K, dim) = (4, 2), (4, 8), (8, 8),
      (6, 4), (7, 5), (8, 3), (2, 1), (8, 1) on subjects drawn from K well-separated states,
      3 fits each.  These are compared with the reference with NO fit left out: the tests
      assert that compare_with_reference returns 0.

Tolerances: the project's own for the batched EM, ll and the lls trajectory at 1e-9
relative, parameters at post_err < 1e-8.  A fit may be left out of the comparison with
the reference only if the reference itself disagrees on it when its observations are
permuted (another iteration count, another status, or parameters apart by more than
1e-9); at most 5 % of a test's fits.  The iteration at which an ill-conditioned fit fails
is not asserted (it moves under reordering); its status is.
"""
import ctypes
import os
import subprocess

import numpy as np

import vbhmm_em_batch_ref as R

ROOT = R.ROOT
CHECK_PATH = os.path.join(ROOT, "tests", "gmmcheck", "libgmmcheck.so")
CONVERGED, MAX_ITER, ILL, BAD = 0, 1, 2, 3
STATUS = ("converged", "max_iter", "ill_conditioned", "bad_fit")
SENTINEL = -7.0     # what the output arrays hold before a call
GPU_SUBJECTS = (0, 2, 6)

_cache = {}
em_mod = R.em_mod


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
class FixedRows:
    """A generator double: choice() returns the injected rows."""

    def __init__(self, rows):
        self.rows = np.asarray(rows, dtype=np.int64)

    def choice(self, N, K, replace=False):
        assert K == self.rows.size and not replace
        return self.rows


class Recorder:
    """A generator that records what choice() gave."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.log = []

    def choice(self, N, K, replace=False):
        r = self.rng.choice(N, K, replace=replace)
        self.log.append(r.copy())
        return r


def ref_fit(X, K, rows, reg=0.0, max_iter=100, tolfun=1e-5):
    """gmm_fit_randsample from the given rows: prior, mean, cov, lls, ll, iters, status."""
    lls = []
    try:
        g = em_mod().gmm_fit_randsample(X, K, FixedRows(rows), tolfun=tolfun, max_iter=max_iter, reg=reg, trace=lls)
    except np.linalg.LinAlgError:
        return dict(status=ILL, iters=len(lls) + 1, lls=np.array(lls))
    last = lls[-2] if len(lls) > 1 else -np.inf
    done = abs(lls[-1] - last) <= tolfun * abs(lls[-1])
    return dict(g, status=CONVERGED if done else MAX_ITER, iters=len(lls), lls=np.array(lls), ll=lls[-1])


def ref_cached(key, X, K, rows, reg, max_iter=100):
    k = ("ref", key, K, tuple(int(r) for r in rows), reg, max_iter)
    if k not in _cache:
        _cache[k] = ref_fit(X, K, rows, reg, max_iter)
    return _cache[k]


def ref_disagrees(X, K, rows, reg, max_iter=100):
    """The reference against itself with the observations permuted."""
    a = ref_fit(X, K, rows, reg, max_iter)
    perm = np.random.default_rng(12345).permutation(X.shape[0])
    inv = np.argsort(perm)
    b = ref_fit(X[perm], K, inv[np.asarray(rows)], reg, max_iter)
    if a["status"] != b["status"] or (a["status"] != ILL and a["iters"] != b["iters"]):
        return True
    if a["status"] == ILL:
        return False
    return any(np.max(np.abs(a[k] - b[k]) / np.maximum(np.abs(a[k]), 1e-300)) > 1e-9 for k in ("prior", "mean", "cov"))


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
class HostSubjects:
    """What random_gmm_batch and the stand-in engine read of a SubjectBatch."""

    def __init__(self, datas, dim):
        self.dim = dim
        self.datas = [[np.asarray(a, dtype=np.float64).reshape(-1, dim) for a in d] for d in datas]
        self.X = [np.concatenate(d, axis=0) for d in self.datas]
        self.S = len(self.datas)


def host_draws(X, K, numtrials, seed):
    """The host driver's trials of one (subject, K): per trial its GMM, the rows and reg of
    the fit that gave it, and the rows of the draw that failed before it (or None)."""
    rng, out = Recorder(seed), []
    for _ in range(numtrials):
        n0 = len(rng.log)
        g = em_mod().random_gmm([X], K, rng)
        d = rng.log[n0:]
        out.append(dict(gmm=g, rows=d[-1], reg=1e-10 if len(d) == 2 else 0.0, failed=d[0] if len(d) == 2 else None))
    return out


def demo_fits(subjects=GPU_SUBJECTS, numtrials=12):
    """(subj, fits, trials): the demo subset's subjects (re-indexed 0..), its fits
    (subject, K, rows, reg) -- every trial's, then the failed draws -- and the host
    driver's trials {(subject, K): host_draws}."""
    key = ("demo", subjects, numtrials)
    if key not in _cache:
        allsub = R.demo_subjects()
        subj = [allsub[i] for i in subjects]
        trials, fits, failed = {}, [], []
        for s, d in enumerate(subj):
            X = np.concatenate(d)
            for K in (2, 3):
                trials[(s, K)] = host_draws(X, K, numtrials, 100)
                for t in trials[(s, K)]:
                    fits.append((s, K, t["rows"], t["reg"]))
                    if t["failed"] is not None:
                        failed.append((s, K, t["failed"], 0.0))
        _cache[key] = (subj, fits + failed, trials)
    return _cache[key]


def dim_fits(dim):
    subj, runs = R.runs_c(dim)
    X = np.concatenate(subj[0])
    rng = np.random.default_rng(70 + dim)
    return subj, [(0, 2, rng.choice(X.shape[0], 2, replace=False), 0.0) for _ in range(3)]


def edge_fits():
    """Subjects of one sequence with N = 3, 63, 64, 65, 129 and 200 observations: K = 2
    from rows that include 0 and N - 1 (N = 3: K + 1), and K = 8 on the 200."""
    sizes = (3, 63, 64, 65, 129, 200)
    subj = [R.gaussian_subject(30 + i, [n]) for i, n in enumerate(sizes)]
    fits = [(s, 2, np.array([n - 1, 0]), 0.0) for s, n in enumerate(sizes)]
    fits += [(s, 2, np.array([0, n // 2]), 0.0) for s, n in enumerate(sizes) if n > 3]
    fits.append((5, 8, np.random.default_rng(8).choice(200, 8, replace=False), 0.0))
    fits.append((5, 8, np.array([199, 0, 17, 33, 64, 65, 128, 63]), 0.0))
    return subj, fits


# (K, dim) at the corners of the kernel's buckets: K = 4 and 8 fill KM, K * dim = 64 leaves
# no spare lane, K * dim * dim = 512 is 8 rounds of the covariance loops
CORNERS = [(4, 2), (4, 8), (8, 8), (6, 4), (7, 5), (8, 3), (2, 1), (8, 1)]


def corner_fits(K, dim):
    """A subject of 40 sequences of 1..12 steps from K states (R.states_subject) and 3 fits
    from seeded start rows.  With these seeds every fit completes (one of K = 8, dim = 1 at
    max_iter) and the reference agrees with itself on every fit when its observations are
    permuted: no fit may be left out."""
    key = ("corner", K, dim)
    if key not in _cache:
        lens = np.random.default_rng(7000).integers(1, 13, 40)
        subj = [R.states_subject(7100 + 10 * K + dim, K, dim, lens)]
        N = int(lens.sum())
        rng = np.random.default_rng(7200)
        _cache[key] = (subj, [(0, K, rng.choice(N, K, replace=False), 0.0) for _ in range(3)])
    return _cache[key]


def planted_subject():
    rng = np.random.default_rng(1)
    X = np.concatenate([rng.normal([160.0, 210.0], 20.0, (40, 2)), [[1e4, 1e4]]])
    return [[X]]


PLANTED_ROWS = np.array([40, 3])


def hyper_vector(opt):
    em = em_mod()
    copt, _ = em.vbhmm_clip_hyps(opt)
    dim = len(copt["mu0"])
    W0 = np.asarray(copt["W0"], dtype=np.float64)
    W0inv = np.linalg.inv(float(W0) * np.eye(dim) if W0.size == 1 else np.diag(W0.reshape(-1)))
    return np.ascontiguousarray(em.em_hyper_vector(copt, W0inv)), copt


# ----------------------------------------------------------------------------
# the check library
# ----------------------------------------------------------------------------
def load_check():
    if "lib" not in _cache:
        if not os.path.exists(CHECK_PATH):
            subprocess.run(["make", "-C", ROOT, "gmmcheck"], check=True, stdout=subprocess.DEVNULL)
        import torch  # noqa: F401  (the library binds to the HIP runtime torch loaded)
        lib = ctypes.CDLL(CHECK_PATH)
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        lib.gmmcheck_host.argtypes = [ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, ci, cd, vp] + [vp] * 8
        lib.gmmcheck_host.restype = ci
        lib.gmmcheck_device.argtypes = [ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, ci, cd, vp, ci] + [vp] * 8
        lib.gmmcheck_device.restype = ci
        _cache["lib"] = lib
    return _cache["lib"]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_fits(subj, fits, dim, where="host", max_iter=100, tolfun=1e-5, hyper=None, chunk_runs=0, KM=None,
             expect=0):
    """Every fit through the host walker (where='host') or the library's kernels on device
    0 ('device').  One dict per fit: status (int), iters, ll, lls, prior, mean, cov (states
    k < K), post_init (the packed row, with hyper) and ``raw``, the whole output rows as
    they came back over SENTINEL-filled arrays (for bitwise comparisons and 'untouched')."""
    lib = load_check()
    off, x, first = R.pack_subjects(subj, dim)
    Ks = np.array([f[1] for f in fits], dtype=np.int32)
    sub = np.array([f[0] for f in fits], dtype=np.int32)
    KM = KM or (4 if Ks.max() <= 4 else 8)
    Rn = len(fits)
    rows = np.zeros((Rn, KM), dtype=np.int32)
    for i, f in enumerate(fits):
        r = np.asarray(f[2]).reshape(-1)[:KM]
        rows[i, :r.size] = r
    reg = np.array([f[3] for f in fits], dtype=np.float64)
    PL = em_mod().em_post_len(KM, dim)
    o_pr, o_me = np.full((Rn, KM), SENTINEL), np.full((Rn, KM, dim), SENTINEL)
    o_co, o_ll = np.full((Rn, KM, dim, dim), SENTINEL), np.full(Rn, SENTINEL)
    o_it, o_ss = np.full(Rn, -7, dtype=np.int32), np.full(Rn, -7, dtype=np.int32)
    o_lls = np.full((Rn, max_iter), SENTINEL)
    o_pi = np.full((Rn, PL), SENTINEL) if hyper is not None else None
    args = [len(subj), dim, _ptr(off), _ptr(x), _ptr(first), Rn, KM, _ptr(sub), _ptr(Ks), _ptr(rows), _ptr(reg),
            int(max_iter), float(tolfun), _ptr(hyper)]
    outs = [_ptr(a) for a in (o_pr, o_me, o_co, o_ll, o_it, o_ss, o_lls, o_pi)]
    if where == "host":
        rc = lib.gmmcheck_host(*args, *outs)
    else:
        rc = lib.gmmcheck_device(*args, int(chunk_runs), *outs)
    assert rc == expect, (where, rc)
    if rc != 0:
        return None
    out = []
    for r in range(Rn):
        K, it = int(Ks[r]), max(int(o_it[r]) - (int(o_ss[r]) == ILL), 0)    # no ll of the failing iteration
        K = min(max(K, 0), KM)
        out.append(dict(status=int(o_ss[r]), iters=int(o_it[r]), ll=float(o_ll[r]), lls=o_lls[r, :it].copy(),
                        prior=o_pr[r, :K].copy(), mean=o_me[r, :K].copy(), cov=o_co[r, :K].copy(),
                        post_init=o_pi[r].copy() if o_pi is not None else None,
                        raw=(o_pr[r].copy(), o_me[r].copy(), o_co[r].copy(), o_lls[r].copy(),
                             o_pi[r].copy() if o_pi is not None else np.zeros(0), float(o_ll[r]), int(o_it[r]),
                             int(o_ss[r]))))
    return out


def same_bits(a, b, KM_differs=False):
    """Two results of run_fits: every output identical, NaN patterns included.  Across KM
    the rows have different lengths: the states' parameters are compared."""
    if KM_differs:
        return (all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("prior", "mean", "cov", "lls"))
                and a["raw"][6:] == b["raw"][6:] and np.array_equal(a["ll"], b["ll"], equal_nan=True))
    return (all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["raw"][:5], b["raw"][:5]))
            and np.array_equal(a["raw"][5], b["raw"][5], equal_nan=True) and a["raw"][6:] == b["raw"][6:])


def untouched(g):
    """A BAD_FIT wrote its status alone."""
    return (g["status"] == BAD and g["iters"] == -7 and g["ll"] == SENTINEL
            and all((x == SENTINEL).all() for x in g["raw"][:5]))


def standin_fit_batch(subjects, fits, tolfun=1e-5, max_iter=100, keep_lls=False, hyper=None, chunk_runs=0,
                      KM=None, where="host"):
    """gmm_fit_batch's signature and results with the walker (or the check library's
    device call) behind it: the stand-in engine of random_gmm_batch."""
    got = run_fits(subjects.datas, fits, subjects.dim, where, max_iter, tolfun, hyper, chunk_runs, KM)
    out = []
    for g in got:
        done = g["status"] < ILL
        out.append(dict(prior=g["prior"] if done else None, mean=g["mean"] if done else None,
                        cov=g["cov"] if done else None, ll=g["ll"], iters=g["iters"], status=STATUS[g["status"]]))
    return (out, np.stack([g["post_init"] for g in got])) if hyper is not None else out


# ----------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------
def compare_with_reference(got, subj, fits, post_err, tag="", max_iter=100):
    """Status always; iters, lls at 1e-9 and parameters at post_err < 1e-8 for fits the
    reference completes.  Returns the number of fits left out (see the module docstring)."""
    excluded = 0
    for i, (g, (s, K, rows, reg)) in enumerate(zip(got, fits)):
        X = np.concatenate(subj[s])
        ref = ref_cached((tag, s, X.shape), X, K, rows, reg, max_iter)
        try:
            assert g["status"] == ref["status"], (tag, i, g["status"], ref["status"])
            if ref["status"] == ILL:
                continue
            assert g["iters"] == ref["iters"], (tag, i, g["iters"], ref["iters"])
            np.testing.assert_allclose(g["lls"], ref["lls"], rtol=1e-9, err_msg=f"{tag} fit {i}")
            np.testing.assert_allclose(g["ll"], ref["ll"], rtol=1e-9, err_msg=f"{tag} fit {i}")
            for k in ("prior", "mean", "cov"):
                assert post_err(g[k], ref[k]) < 1e-8, (tag, i, k, post_err(g[k], ref[k]))
        except AssertionError:
            if not ref_disagrees(X, K, rows, reg, max_iter):
                raise
            excluded += 1
    assert excluded * 20 <= len(got), (tag, excluded, len(got))
    return excluded


def compare_runs(a, b, post_err, tag=""):
    """Kernels against the walker: equal status and iters, lls at 1e-9, parameters and
    post_init at 1e-8."""
    for i, (d, h) in enumerate(zip(a, b)):
        assert d["status"] == h["status"], (tag, i, d["status"], h["status"])
        if h["status"] == BAD:
            assert untouched(d) and untouched(h), (tag, i)
            continue
        if h["status"] == ILL:     # the iteration of the failing pivot is not asserted
            assert all((x == SENTINEL).all() for x in (d["raw"][0], d["raw"][1], d["raw"][2], d["raw"][4])), (tag, i)
            continue
        assert d["iters"] == h["iters"], (tag, i, d["iters"], h["iters"])
        np.testing.assert_allclose(d["lls"], h["lls"], rtol=1e-9, err_msg=f"{tag} fit {i}")
        np.testing.assert_allclose(d["ll"], h["ll"], rtol=1e-9, err_msg=f"{tag} fit {i}")
        for k in ("prior", "mean", "cov"):
            assert post_err(d[k], h[k]) < 1e-8, (tag, i, k)
        if h["post_init"] is not None:
            assert post_err(d["post_init"], h["post_init"]) < 1e-8, (tag, i)


def check_initial_posterior(got, subj, fits, opt, post_err, KM, tag=""):
    """The packed initial posterior of every completed fit against
    pack_posterior(vbhmm_init(...)) of the same GMM, piece by piece at 1e-8, and the
    padding bit for bit."""
    em = em_mod()
    _, copt = hyper_vector(opt)
    dim = len(copt["mu0"])
    n = 0
    for i, (g, (s, K, rows, reg)) in enumerate(zip(got, fits)):
        if g["status"] >= ILL:
            assert (g["post_init"] == SENTINEL).all(), (tag, i)
            continue
        X = np.concatenate(subj[s])
        mix = em.vbhmm_init([X], K, copt, dict(prior=g["prior"], mean=g["mean"], cov=g["cov"]))
        want = em.pack_posterior(mix, K, KM, dim)
        a, b = em.unpack_posterior(g["post_init"], K, KM, dim), em.unpack_posterior(want, K, KM, dim)
        for k in R.POST_KEYS:
            assert post_err(a[k], b[k]) < 1e-8, (tag, i, k, post_err(a[k], b[k]))
        # every entry no state owns is the host's padding
        nan = np.nan
        blank = dict(alpha=np.full(K, nan), epsilon=np.full((K, K), nan), beta=np.full(K, nan), v=np.full(K, nan),
                     m=np.full((K, dim), nan), W=np.full((K, dim, dim), nan))
        pad = ~np.isnan(em.pack_posterior(blank, K, KM, dim))
        assert np.array_equal(g["post_init"][pad], want[pad]), (tag, i)
        n += 1
    assert n > 0
