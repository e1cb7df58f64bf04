"""What the batched 'gmmNew' initialisation tests share: the inputs, the reference with its
conditions, the loader of the check build (tests/ghemcheck) and the comparisons.

Reference: h3m.gmm_mix_hier_em and h3m.gmmnew_init, unchanged.  gmm_mix_hier_em gets the
generator double of wtk_ref (Draws: the injected first index and uniform draws of
kmeans_pp) with a random() that discards, as the reference discards its rand(T, n).  While
the reference runs, h3m's numpy is watched: wtk_ref's record of every argmin and D2 draw,
and every logp (the argument of the loop's isfinite).  The conditions under which equal
statuses and iteration counts mean something are computed on the reference itself and
asserted for every input:
  * the k-means++ conditions of wtk_ref: assignment gaps and draw margins above GAP = 1e-9;
  * every increment logp - last of the run lies more than 1e-9 max(1, |logp|) from the
    stopping threshold 1e-6.
An input that fails one of them is replaced by another one, never excused.

Tolerance.  Statuses, Lloyd passes and E-step counts are equal.  The continuous outputs
agree within UNITS n 2^-53 scale, with scale the largest |coordinate| for the centres, the
largest |covariance entry| plus the largest |coordinate| squared for the covariances,
max(1, |logp|) for logp, and 1 for mxwt and for logpost (compared where the reference's
value is above -30).  UNITS is eight times the largest deviation of the serial walker from
the numpy reference over SHAPES, but at least wtk_ref's 100: see MEASURED_UNITS.  The same
bound serves kernels against walker: they differ by the order of n-term sums and by the
device's exp and log, a perturbation of the same kind as, and no larger than, numpy's
pairwise sums and LAPACK inverse against the walker's serial sums and Cholesky.
"""
import contextlib
import ctypes
import os
import subprocess

import numpy as np

import wtk_ref as W

ROOT = W.ROOT
CHECK_PATH = os.path.join(ROOT, "tests", "ghemcheck", "libghemcheck.so")
OK, DEGENERATE, BAD, NONFINITE, SINGULAR = 0, 1, 2, 3, 4
HOST, DEVICE = W.HOST, W.DEVICE
STOP, STOP_MARGIN = 1e-6, 1e-9

# Measured 2026-10-20 on the CPU by measure_units() below: the serial walker against
# h3m.gmm_mix_hier_em over SHAPES with iterations 30, 1 and 0.  The largest deviation in
# units of n 2^-53 scale: mxwt 0.04, centres 0.24, covars 0.025, logp 0.063, logpost 64.0
# (at n = 3, where a log-posterior near -20 moves by a few of its own ulps).  The largest:
MEASURED_UNITS = 64.0
UNITS = max(100.0, 8.0 * MEASURED_UNITS)

_cache = {}


def h3m():
    return W.h3m()


# ----------------------------------------------------------------------------
# the reference, watched
# ----------------------------------------------------------------------------
class _Numpy(W._Numpy):
    """wtk_ref's watched numpy, which also records every logp the EM loop tests."""

    def isfinite(self, x):
        if np.ndim(x) == 0:
            self._t.logps.append(float(x))
        return np.isfinite(x)


@contextlib.contextmanager
def traced():
    mod, t = h3m(), W.Trace()
    t.logps = []
    mod.np = _Numpy(t)
    try:
        yield t
    finally:
        mod.np = np


class Draws(W.Draws):
    """kmeans_pp's generator double, with the discarded rand(T, n) of gmm_mix_hier_em."""

    def random(self, shape=None):
        assert shape is not None, "only the discarded draw is expected"
        return None


def draws_of(seed, n, T):
    """What a PCG64(seed) generator gives gmm_mix_hier_em on n points for T components."""
    g = np.random.Generator(np.random.PCG64(seed))
    g.random((T, n))
    return int(g.integers(n)), np.array([g.random() for _ in range(T - 1)])


def increments_ok(logps):
    last = -np.finfo(float).max
    for lp in logps:
        if not np.isfinite(lp):
            return True
        if abs((lp - last) - STOP) <= STOP_MARGIN * max(1.0, abs(lp)):
            return False
        if lp - last < STOP:
            return True
        last = lp
    return True


def ref_fit(X, C, full, T, vs, iterations, j0=None, u=None, init=None):
    """h3m.gmm_mix_hier_em from the injected draws (or given centres): dict(mxwt, centres,
    covars, logpost, logp, iters = [Lloyd passes, E-steps]), the conditions asserted."""
    with traced() as t:
        mx, cen, vr, lp = h3m().gmm_mix_hier_em(X, C, full, T, vs, iterations,
                                                Draws(0 if j0 is None else j0, [] if u is None else u, t), init)
    assert all(g > W.GAP for g in t.gaps), ("assignment gap", min(t.gaps))
    assert all(g > W.GAP for g in t.draws), ("draw margin", min(t.draws))
    assert increments_ok(t.logps), ("increment", t.logps)
    return dict(mxwt=mx, centres=cen, covars=vr, logpost=lp, logp=t.logps[-1] if t.logps else 0.0,
                iters=[t.passes, len(t.logps)], logps=t.logps)


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def points(n, d, full, T, seed):
    """n base-state Gaussians around T random centres; covariances as synth_base_set
    makes them: L L' / d + 0.5 I (diagonal: the diagonal of that)."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(0.0, 12.0, (T, d))
    X = mu[rng.integers(0, T, n)] + rng.normal(size=(n, d))
    L = rng.normal(size=(n, d, d))
    C = L @ L.transpose(0, 2, 1) / d + 0.5 * np.eye(d)
    if not full:
        C = np.ascontiguousarray(np.diagonal(C, axis1=1, axis2=2))
    return np.ascontiguousarray(X), np.ascontiguousarray(C)


def samples_of(n):
    """The virtual samples of a test input: 5 per point (gmmnew_init: Nv Kb = Nv n / Sb)."""
    return 5.0 * n


def shapes(P=256):
    """(n, d, T, full): the demo's size, n = T, the edges of the point tile P, more than
    two tiles, every dimension bucket and its edges, the limits of d and T."""
    return [(25, 2, 3, True), (3, 2, 3, True), (P - 1, 1, 2, False), (P, 3, 3, True), (P + 1, 2, 8, False),
            (2 * P + 1, 8, 8, True), (P + 1, 9, 3, True), (2 * P + 1, 16, 32, True), (2 * P + 1, 16, 2, False),
            (P - 1, 9, 32, False), (32, 3, 32, True), (300, 1, 3, True)]


SHAPES = shapes()
# beyond the size at which the tile grows to 1,024 points (four 256-point parts per tile in
# the E-step kernel), with a last tile of one point
LARGE = (262144 + 1025, 2, 2, False)


def case(n, d, T, full, iterations=30, seed=None):
    """Points and a draw whose reference passes the conditions: the first seed from
    ``seed`` that does.  Returns (X, C, j0, u, ref)."""
    key = ("case", n, d, T, full, iterations, seed)
    if key not in _cache:
        base = 11 * n + 5 * d + T + (0 if full else 1) if seed is None else seed
        X, C = points(n, d, full, T, base)
        for s in range(base, base + 20):
            j0, u = draws_of(s, n, T)
            try:
                ref = ref_fit(X, C, full, T, samples_of(n), iterations, j0, u)
            except AssertionError:
                continue
            _cache[key] = (X, C, j0, u, ref)
            break
        else:
            raise AssertionError(f"no admissible draw for {key}")
    return _cache[key]


# ----------------------------------------------------------------------------
# the check library
# ----------------------------------------------------------------------------
def load_check():
    if "lib" not in _cache:
        if not os.path.exists(CHECK_PATH):
            subprocess.run(["make", "-C", ROOT, "ghemcheck"], check=True, stdout=subprocess.DEVNULL)
        import torch  # noqa: F401  (the library binds to the HIP runtime torch loaded)
        lib = ctypes.CDLL(CHECK_PATH)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.ghemcheck_tile_points.argtypes = [ci, ci]
        lib.ghemcheck_fit.argtypes = [ci] * 6 + [vp, vp, ctypes.c_double, ci, vp, vp, vp, ci] + [vp] * 7
        lib.ghemcheck_tile_points.restype = lib.ghemcheck_fit.restype = ci
        _cache["lib"] = lib
    return _cache["lib"]


def tile_points(n, d):
    return load_check().ghemcheck_tile_points(n, d)


def run_fit(where, X, C, full, T, vs, iterations, j0=None, u=None, init=None, chunk=0, logpost=True, expect=0):
    """R trials through the walker or the kernels: dict(mxwt [R][T], centres, covars,
    logpost | None, logp [R], status [R], iters [R][2]); -7 where nothing was written."""
    X, C = W._f(X), W._f(C)
    n, d = X.shape
    if init is not None:
        init = W._f(init).reshape(-1, T, d)
        R, j0, u = init.shape[0], None, None
    else:
        j0 = W._i(np.atleast_1d(j0))
        R = j0.size
        u = W._f(u).reshape(R, max(T - 1, 1))
    cd = (d, d) if full else (d,)
    out = dict(mxwt=np.full((R, T), -7.0), centres=np.full((R, T, d), -7.0), covars=np.full((R, T) + cd, -7.0),
               logpost=np.full((R, T, n), -7.0) if logpost else None, logp=np.full(R, -7.0),
               status=np.full(R, -7, np.int32), iters=np.full((R, 2), -7, np.int32))
    rc = load_check().ghemcheck_fit(where, n, d, int(full), T, R, W._p(X), W._p(C), float(vs), int(iterations),
                                    W._p(j0), W._p(u), W._p(init), chunk, W._p(out["mxwt"]), W._p(out["centres"]),
                                    W._p(out["covars"]), W._p(out["logpost"]), W._p(out["logp"]), W._p(out["status"]),
                                    W._p(out["iters"]))
    assert rc == expect, rc
    return out


class CheckEngine:
    """h3m.GhemDeviceEngine's interface over the check library: the walker (where = HOST),
    the stand-in engine of gmm_mix_hier_em_batch on a machine without a GPU."""

    def __init__(self, device=None, chunk_trials=None, where=HOST):
        import torch
        self.where, self.chunk, self.dev = where, int(chunk_trials or 0), torch.device("cpu")
        self.calls = 0

    def fit(self, X, C, full, T, vs, iterations, j0, u, init, want_logpost):
        self.calls += 1
        return run_fit(self.where, X, C, full, T, vs, iterations, j0, u, init, self.chunk, want_logpost)


# ----------------------------------------------------------------------------
# comparisons
# ----------------------------------------------------------------------------
def deviations(got, ref, r, X, C):
    """Trial r of ``got`` against a reference dict, per output in units of n 2^-53 scale."""
    n = X.shape[0]
    big = float(np.abs(X).max())
    scale = dict(mxwt=1.0, centres=big, covars=float(np.abs(C).max()) + big * big,
                 logp=max(1.0, abs(float(ref["logp"]))), logpost=1.0)
    out = {}
    for k, sc in scale.items():
        if got[k] is None:
            continue
        a, b = np.asarray(got[k][r], dtype=float), np.asarray(ref[k], dtype=float)
        keep = b > -30.0 if k == "logpost" else np.ones(b.shape, bool)
        diff = np.abs(a - b)[keep]
        out[k] = float(diff.max()) / (n * 2.0 ** -53 * sc) if diff.size else 0.0
    return out


def assert_close(got, ref, r, X, C):
    dev = deviations(got, ref, r, X, C)
    assert all(np.isfinite(v) and v <= UNITS for v in dev.values()), dev
    return dev


def check_fit(where, X, C, full, T, iterations, j0=None, u=None, init=None):
    """One trial through the walker or the kernels against h3m.gmm_mix_hier_em."""
    vs = samples_of(X.shape[0])
    ref = ref_fit(X, C, full, T, vs, iterations, j0, u, init)
    got = run_fit(where, X, C, full, T, vs, iterations, j0, None if u is None else [u],
                  None if init is None else [init])
    assert got["status"][0] == OK
    assert got["iters"][0].tolist() == ref["iters"], (got["iters"][0], ref["iters"])
    return got, ref, assert_close(got, ref, 0, X, C)


def measure_units():
    """The walker against the reference over SHAPES, iterations 30, 1 and 0: the largest
    deviation per output, in units."""
    worst = {}
    for n, d, T, full in SHAPES:
        for iterations in (30, 1, 0):
            X, C, j0, u, ref = case(n, d, T, full, iterations)
            got = run_fit(HOST, X, C, full, T, samples_of(n), iterations, j0, [u])
            for k, v in deviations(got, ref, 0, X, C).items():
                worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ----------------------------------------------------------------------------
# scenarios run by the CPU tests on the walker and by the GPU tests on the kernels
# ----------------------------------------------------------------------------
def scenario_shape(where, n, d, T, full):
    X, C, j0, u, _ = case(n, d, T, full)
    return check_fit(where, X, C, full, T, 30, j0, u)


def scenario_iterations(where):
    """iterations 0 (the start values, zero log-posteriors), 1 (one M-step, never prepared)
    and the default."""
    for iterations in (0, 1, 30):
        X, C, j0, u, ref = case(300, 2, 3, True, iterations)
        got, _, _ = check_fit(where, X, C, True, 3, iterations, j0, u)
        assert got["iters"][0, 1] == min(iterations, ref["iters"][1])
        if iterations == 0:
            assert (got["logpost"] == 0.0).all() and (got["mxwt"] == 1.0 / 3).all()


def scenario_init_centres(where):
    """Given centres: no seeding, no draw read, zero Lloyd passes."""
    for full in (True, False):
        X, C = points(300, 3, full, 4, 41)
        init = X[[5, 77, 150, 299]] + 0.25
        got, _, _ = check_fit(where, X, C, full, 4, 30, init=init)
        assert got["iters"][0, 0] == 0


def healthy():
    X, C, j0, u, _ = case(300, 2, 3, True, seed=61)
    j1, u1 = draws_of(62, 300, 3)
    ref_fit(X, C, True, 3, samples_of(300), 30, j1, u1)
    return X, C, [j0, j1], np.stack([u, u1])


def same_trial(a, ra, b, rb):
    return all(np.array_equal(a[k][ra], b[k][rb]) for k in ("mxwt", "centres", "covars", "logpost", "logp", "status",
                                                            "iters") if a[k] is not None)


def untouched(got, r):
    return all((got[k][r] == -7).all() for k in ("mxwt", "centres", "covars", "logpost", "logp", "iters"))


def scenario_contained(where):
    """Trials that are not OK write their status alone and leave the others' bits.  A
    centre at 1e4 takes no point: its weights are 0 / 0 and the next logp is NaN
    (NONFINITE; the reference keeps the NaN centre).  All-zero covariances: a zero pivot
    (SINGULAR; numpy's inverse raises).  Fewer distinct points than T (DEGENERATE) and a
    NaN coordinate (BAD) hold for every trial of a call: the points are shared."""
    X, C, j0, u = healthy()
    vs = samples_of(300)
    alone = run_fit(where, X, C, True, 3, vs, 30, j0, u)
    assert alone["status"].tolist() == [OK, OK]
    # a draw out of range between healthy trials
    mixed = run_fit(where, X, C, True, 3, vs, 30, [j0[0], 300, j0[1], -1], [u[0], u[0], u[1], u[1]])
    assert mixed["status"].tolist() == [OK, BAD, OK, BAD]
    assert same_trial(alone, 0, mixed, 0) and same_trial(alone, 1, mixed, 2)
    assert untouched(mixed, 1) and untouched(mixed, 3)
    # a far centre between healthy ones, all from given centres
    good = X[[3, 120, 250]] + 0.25
    far = good.copy()
    far[1] = 1e4
    base = run_fit(where, X, C, True, 3, vs, 30, init=[good, good + 0.5])
    got = run_fit(where, X, C, True, 3, vs, 30, init=[good, far, good + 0.5])
    assert base["status"].tolist() == [OK, OK] and got["status"].tolist() == [OK, NONFINITE, OK]
    assert same_trial(base, 0, got, 0) and same_trial(base, 1, got, 2) and untouched(got, 1)
    with np.errstate(all="ignore"):
        ref = h3m().gmm_mix_hier_em(X, C, True, 3, vs, 30, Draws(0, []), far)
    assert np.isnan(ref[1][1]).all()
    # all-zero covariances
    zero = run_fit(where, X, np.zeros_like(C), True, 3, vs, 30, j0, u)
    assert zero["status"].tolist() == [SINGULAR, SINGULAR] and untouched(zero, 0) and untouched(zero, 1)
    with np.testing.assert_raises(np.linalg.LinAlgError):
        h3m().gmm_mix_hier_em(X, np.zeros_like(C), True, 3, vs, 30, Draws(j0[0], u[0]))
    # ... with iterations = 0 nothing is inverted, on either side
    assert run_fit(where, X, np.zeros_like(C), True, 3, vs, 0, j0, u)["status"].tolist() == [OK, OK]
    Xd = np.repeat(X[:2], 150, axis=0)
    deg = run_fit(where, Xd, C, True, 3, vs, 30, j0, u)
    assert deg["status"].tolist() == [DEGENERATE, DEGENERATE] and untouched(deg, 0)
    Xn = X.copy()
    Xn[17, 1] = np.nan
    bad = run_fit(where, Xn, C, True, 3, vs, 30, j0, u)
    assert bad["status"].tolist() == [BAD, BAD] and untouched(bad, 1)
    Cn = C.copy()
    Cn[200, 0, 1] = np.inf
    assert run_fit(where, X, Cn, True, 3, vs, 30, j0, u)["status"].tolist() == [BAD, BAD]


def trial_draws(seeds, n, T):
    dr = [draws_of(s, n, T) for s in seeds]
    return [j for j, _ in dr], np.stack([u for _, u in dr])


def scenario_batching(where, R):
    """A trial's outputs bit for bit whatever R, its place, the chunking and the run."""
    n = tile_points(300, 2) + 1
    X, C = points(n, 2, True, 3, 71)
    vs = samples_of(n)
    j0, u = trial_draws(range(80, 80 + R), n, 3)
    fit = lambda j, uu, chunk=0: run_fit(where, X, C, True, 3, vs, 30, j, uu, chunk=chunk)
    base = fit(j0, u)
    assert (base["status"] == OK).all()
    again, rev, one = fit(j0, u), fit(j0[::-1], u[::-1]), fit(j0[:1], u[:1])
    perm = np.random.default_rng(R).permutation(R)
    shuf = fit([j0[i] for i in perm], u[perm])
    for r in range(R):
        assert same_trial(base, r, again, r) and same_trial(base, r, rev, R - 1 - r), r
        assert same_trial(base, int(perm[r]), shuf, r), r
    assert same_trial(base, 0, one, 0)
    for chunk in (1, 7):
        ch = fit(j0, u, chunk)
        assert all(same_trial(base, r, ch, r) for r in range(R)), chunk
    return base


def scenario_optional(where):
    """logpost not wanted changes nothing else."""
    X, C, j0, u = healthy()
    vs = samples_of(300)
    a = run_fit(where, X, C, True, 3, vs, 30, j0, u)
    b = run_fit(where, X, C, True, 3, vs, 30, j0, u, logpost=False)
    assert b["logpost"] is None and same_trial(b, 0, a, 0) and same_trial(b, 1, a, 1)


def posterior_close(a, b, n, X, C, full):
    """Two Posteriors of gmmnew_init field by field: the fields that come from the draws
    are equal; m within the centres' tolerance; W = ((v - d - 1) cov)^-1 within the
    covariances' relative tolerance times the condition of the inverse."""
    for k in ("alpha", "eta", "epsilon", "lam", "v"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.W0mode == b.W0mode
    big = float(np.abs(X).max())
    unit = UNITS * n * 2.0 ** -53
    assert np.abs(a.m - b.m).max() <= unit * big, np.abs(a.m - b.m).max()
    # dW = -W dV W: |dW| <= |W|^2 |dV|, |dV| <= max(v - d - 1) unit scale
    dv = float((b.v - X.shape[1] - 1).max()) * unit * (float(np.abs(C).max()) + big * big)
    wn = float(np.abs(b.W).max())
    d = X.shape[1] if full else 1
    assert np.abs(a.W - b.W).max() <= 2.0 * d * d * wn * wn * dv, (np.abs(a.W - b.W).max(), wn, dv)
