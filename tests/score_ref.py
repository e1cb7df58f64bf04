"""Numpy loop restatements of the reference's sequence-scoring functions -- the
judge of tests/test_score.py and tests/test_score_gpu.py -- written from
src/hmm/vbhmm_ll.m:40-116, vbhmm_map_state.m:28-138 (viterbi_path, normalize),
vbhmm_prob_state.m:27-48 and vbhmm_random_sample.m:76-79 (multirnd), with
MATLAB's mvnpdf formula: cov = R'R (upper Cholesky factor), q = |(x - mean) / R|^2,
rho = exp(-q/2 - sum log diag R - d log(2 pi)/2); a vector cov is diagonal.
State indices are 0-based.  Also the shared test cases and their cached
reference results.
"""
import ctypes
import functools
import os

import numpy as np
from scipy.linalg import solve_triangular

RHO_FLOOR = np.frombuffer(np.uint64(10).tobytes(), dtype=np.float64)[0]  # 4.9407e-323


# ----------------------------------------------------------------------------
# restatements
# ----------------------------------------------------------------------------
def log_mvnpdf(x, mean, cov):
    """log of mvnpdf(x, mean, cov) per row of x [T][d]."""
    mean = np.asarray(mean, dtype=np.float64).reshape(-1)
    d = mean.size
    x0 = np.asarray(x, dtype=np.float64).reshape(-1, d) - mean
    cov = np.asarray(cov, dtype=np.float64)
    if cov.ndim < 2 or (cov.size == d and d > 1):
        R = np.sqrt(cov.reshape(-1))
        xr = x0 / R
        logdet = np.sum(np.log(R))
    else:
        R = np.linalg.cholesky(cov.reshape(d, d)).T          # upper, cov = R'R
        xr = solve_triangular(R.T, x0.T, lower=True).T if len(x0) else x0  # x0 / R
        logdet = np.sum(np.log(np.diag(R)))
    return -0.5 * np.sum(xr ** 2, axis=1) - logdet - d * np.log(2 * np.pi) / 2


def emissions(hmm, x):
    """(rho [T][K], log rho) of the observations x under every state."""
    lr = np.stack([log_mvnpdf(x, p["mean"], p["cov"]) for p in hmm["pdf"]], axis=1)
    with np.errstate(under="ignore"):
        return np.exp(lr), lr


def emissions_each(hmm, data):
    """emissions() of every sequence, evaluated once over the concatenated rows."""
    d = len(np.reshape(hmm["pdf"][0]["mean"], -1))
    rows = [np.asarray(x, dtype=np.float64).reshape(-1, d) for x in data]
    rho, lr = emissions(hmm, np.concatenate(rows) if rows else np.zeros((0, d)))
    cut = np.cumsum([len(r) for r in rows])[:-1]
    return np.split(rho, cut), np.split(lr, cut)


def forward_ll(prior, trans, rho):
    """vbhmm_ll.m:70-102 for one sequence: zero floor, scaled forward pass, sum log c."""
    rho = np.array(rho, dtype=np.float64)
    rho[rho == 0] = RHO_FLOOR
    T, K = rho.shape
    prior = np.asarray(prior, dtype=np.float64).reshape(-1)
    c = np.zeros(T)
    alpha = np.zeros(K)
    with np.errstate(all="ignore"):
        for t in range(T):
            if t == 0:
                a = prior * rho[0]
            else:
                a = (alpha[:, None] * trans).sum(axis=0) * rho[t]   # (alpha * trans) .* rho(t, :)
            c[t] = np.sum(a)
            alpha = a / c[t]
        return float(np.sum(np.log(c)))


def vbhmm_ll(hmm, data, opt="n"):
    """(loglik [N], errors [N])."""
    trans = np.asarray(hmm["trans"], dtype=np.float64)
    ll = np.zeros(len(data))
    for n, rho in enumerate(emissions_each(hmm, data)[0] if len(data) else []):
        ll[n] = forward_ll(hmm["prior"], trans, rho)
    if "n" in opt:
        d = len(np.reshape(hmm["pdf"][0]["mean"], -1))
        rows = np.array([np.asarray(x).reshape(-1, d).shape[0] for x in data], dtype=np.float64)
        with np.errstate(all="ignore"):
            ll = ll / rows
    return ll, np.isinf(ll)


def normalize(a):
    z = np.sum(a)
    return a / (z + (z == 0)), z


def viterbi_path(prior, trans, obslik):
    """viterbi_path (scaled) for obslik [T][K]: (path, loglik, margin); margin = the
    smallest relative gap (best - second) / best over every max of the recursion
    and the final one (inf for one state)."""
    obslik = np.asarray(obslik, dtype=np.float64)
    T, K = obslik.shape
    prior = np.asarray(prior, dtype=np.float64).reshape(-1)
    trans = np.asarray(trans, dtype=np.float64)
    if T == 0:
        return np.zeros(0, dtype=np.int64), 0.0, np.inf
    psi = np.zeros((T, K), dtype=np.int64)
    scale = np.ones(T)
    margin = np.inf

    def gap(v):
        if len(v) < 2:
            return np.inf
        s = np.sort(v)
        return (s[-1] - s[-2]) / s[-1] if s[-1] > 0 else 0.0

    with np.errstate(all="ignore"):
        delta, z = normalize(prior * obslik[0])
        scale[0] = 1.0 / z
        for t in range(1, T):
            new = np.zeros(K)
            for j in range(K):
                cand = delta * trans[:, j]
                psi[t, j] = int(np.argmax(cand))      # first maximum, as MATLAB's max
                margin = min(margin, gap(cand))
                new[j] = cand[psi[t, j]] * obslik[t, j]
            delta, z = normalize(new)
            scale[t] = 1.0 / z
        path = np.zeros(T, dtype=np.int64)
        path[-1] = int(np.argmax(delta))
        margin = min(margin, gap(delta))
        for t in range(T - 2, -1, -1):
            path[t] = psi[t + 1, path[t + 1]]
        return path, float(-np.sum(np.log(scale))), margin


def vbhmm_map_state(hmm, data):
    """(paths, logliks, smallest margin)."""
    out, lls, margin = [], [], np.inf
    for rho in (emissions_each(hmm, data)[0] if len(data) else []):
        p, ll, mg = viterbi_path(hmm["prior"], hmm["trans"], rho)
        out.append(p)
        lls.append(ll)
        margin = min(margin, mg)
    return out, np.array(lls), margin


def vbhmm_prob_state(hmm, seqs):
    prior, trans = np.asarray(hmm["prior"]).reshape(-1), np.asarray(hmm["trans"])
    pr = np.zeros(len(seqs))
    for i, X in enumerate(seqs):
        p = prior[X[0]]
        for t in range(1, len(X)):
            p = p * trans[X[t - 1], X[t]]
        pr[i] = p
    return pr


def multirnd(cumprob, f):
    return int(np.sum(f > np.asarray(cumprob)))


# ----------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------
def make_hmm(rng, K, d, diag, spread=4.0, scale=1.0, centre=0.0):
    """A random K-state HMM: Dirichlet prior / rows, means centre + U[0, spread]^d * scale,
    covariances (L L'/d + 0.5 I) scale^2 or a U[0.5, 1.5] scale^2 vector."""
    prior = rng.dirichlet(np.ones(K) * 2.0)
    trans = rng.dirichlet(np.ones(K) * 2.0, size=K)
    pdf = []
    for _ in range(K):
        mean = centre + rng.uniform(0, spread, d) * scale
        if diag:
            cov = rng.uniform(0.5, 1.5, d) * scale ** 2
        else:
            L = rng.normal(size=(d, d))
            cov = (L @ L.T / d + 0.5 * np.eye(d)) * scale ** 2
        pdf.append(dict(mean=mean, cov=cov))
    return dict(prior=prior, trans=trans, pdf=pdf)


def sample_data(rng, hmms, lens, d, spread=4.0, scale=1.0, centre=0.0):
    """Sequences of the given lengths: points around the means of the HMMs' states."""
    means = np.concatenate([[p["mean"] for p in h["pdf"]] for h in hmms])
    out = []
    for T in lens:
        pick = means[rng.integers(0, len(means), T)]
        out.append(pick + rng.normal(0, 0.8 * scale, (T, d)))
    return out


def floor_case(single):
    """K = 2, d = 2; at step 2 the observation is ~1e3 standard deviations from every
    state (single: from state 1 only), so rho is exactly 0 there."""
    hmm = dict(prior=np.array([0.6, 0.4]), trans=np.array([[0.7, 0.3], [0.45, 0.55]]),
               pdf=[dict(mean=np.array([0.0, 0.0]), cov=np.array([[1.0, 0.2], [0.2, 1.5]])),
                    dict(mean=np.array([3.0, 1.0]), cov=np.array([[0.8, -0.1], [-0.1, 0.6]]))])
    x = np.array([[0.3, -0.2], [2.5, 1.2], [900.0, -700.0], [0.1, 0.4], [2.9, 0.8]])
    if single:
        hmm["pdf"][1]["mean"] = np.array([1000.0, 1000.0])
        x[2] = [0.5, 0.5]
    return hmm, [x, x[:3], x[2:3]]


RAGGED = (0, 1, 2, 17)
STATE_COUNTS = (1, 3, 4, 5, 8, 9, 16)   # both sides of the 4 / 8 / 16 buckets
DIMS = (1, 2, 3, 8)
SHAPES = [(K, d, diag) for K in STATE_COUNTS for d in DIMS for diag in (False, True)]


def shape_id(s):
    return f"K{s[0]}-d{s[1]}-{'diag' if s[2] else 'full'}"


@functools.lru_cache(maxsize=None)
def make_case(K, d, diag, N=6, H=3, seed=0):
    """H HMMs of different state counts (the largest K) and N ragged sequences whose
    first lengths are RAGGED."""
    rng = np.random.default_rng(1000 * K + 10 * d + int(diag) + 7919 * seed + 131 * N + 17 * H)
    counts = [K, max(1, K // 2), max(1, K - 1)]
    counts = (counts * ((H + 2) // 3))[:H]
    hmms = [make_hmm(rng, k, d, diag) for k in counts]
    lens = (list(RAGGED) + [int(v) for v in rng.integers(1, 12, max(0, N - len(RAGGED)))])[:N]
    if N == 1:
        lens = [5]
    return hmms, sample_data(rng, hmms, lens, d)


@functools.lru_cache(maxsize=None)
def reference(K, d, diag, N=6, H=3, seed=0):
    """The restatement's results for make_case(...), computed once: ll [H][N]
    (unnormalised), lln (normalised), paths [H][N], vll [H][N], the smallest Viterbi
    margin and the log-densities' (largest below -700, smallest above -760) zone check."""
    hmms, data = make_case(K, d, diag, N, H, seed)
    ll = np.array([vbhmm_ll(h, data, "")[0] for h in hmms])
    lln = np.array([vbhmm_ll(h, data, "n")[0] for h in hmms])
    paths, vll, margin = [], [], np.inf
    for h in hmms:
        p, v, mg = vbhmm_map_state(h, data)
        paths.append(p)
        vll.append(v)
        margin = min(margin, mg)
    lr = np.concatenate([a.reshape(-1) for h in hmms for a in emissions_each(h, data)[1]])
    return dict(ll=ll, lln=lln, paths=paths, vll=np.array(vll), margin=margin, logrho=lr)


def outside_denormal_zone(logrho):
    """Every log-density is above -700 or below -760: exp is normal or exactly 0 in
    any implementation."""
    lr = np.asarray(logrho)
    return bool(np.all((lr > -700) | (lr < -760)))


# ----------------------------------------------------------------------------
# the host build of the pair routines (tests/scorecheck/libscorecheck.so)
# ----------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORECHECK_PATH = os.path.join(ROOT, "tests", "scorecheck", "libscorecheck.so")


def load_scorecheck():
    if not os.path.exists(SCORECHECK_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "scorecheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(SCORECHECK_PATH)
    vp = ctypes.c_void_p
    args = [ctypes.c_int] * 4 + [vp] * 5 + [ctypes.c_int] + [vp] * 5
    lib.scorecheck_host.argtypes = args
    lib.scorecheck_host.restype = ctypes.c_longlong
    lib.scorecheck_device.argtypes = args
    lib.scorecheck_device.restype = ctypes.c_int
    return lib


def run_scorecheck(lib, packed, data, d, device=False):
    """(status, ll [H][N], vll [H][N], paths [H][N]) of the packed HMMs (score.pack_hmms)
    on the sequences ``data`` through the host loop (or the kernels)."""
    H, KM = packed["prior"].shape
    lens = [int(np.asarray(a).reshape(-1, d).shape[0]) for a in data]
    off = np.zeros(len(data) + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    x = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, d) for a in data])
                             if total else np.zeros((1, d)))
    N = len(data)
    ll, vll = np.full((H, N), 7.0), np.full((H, N), 7.0)
    path = np.full((H, max(total, 1)), -1, dtype=np.int32)
    arrs = [np.ascontiguousarray(packed[k]) for k in ("nstates", "prior", "trans", "mean", "cov")]
    fn = lib.scorecheck_device if device else lib.scorecheck_host
    rc = fn(H, KM, d, int(packed["covmode"]), *[a.ctypes.data for a in arrs], N, off.ctypes.data,
            x.ctypes.data, ll.ctypes.data, vll.ctypes.data, path.ctypes.data)
    pth = path[:, :total]
    paths = [[pth[h, off[n]:off[n + 1]].astype(np.int64) for n in range(N)] for h in range(H)]
    return int(rc), ll, vll, paths
