"""Loop restatement of the reference's CCFD clustering -- the judge of
tests/test_ccfd.py and tests/test_ccfd_gpu.py -- written from the text of
src/compare_mtds/ccfd/CCFD.m and myccfd.m, statement by statement and in their loop
order, separately from vbhem_amd/ccfd.py:

  CCFD(dist, percent, pur, k, dc)   CCFD.m:2-256
  distance(hmms, data)              myccfd.m:14-30 over score_ref.vbhmm_ll
  myccfd_from_dist(dist, ...)       myccfd.m:42-114

Indices, labels and centres are 0-based; a point without a label yet holds -2 (the
reference's -1), a halo point -1 (the reference's 0), no neighbour -1 (the
reference's 0 or an unassigned entry).  Where MATLAB stops on an index error (cl(0),
dc(3) of a shorter vector) or on error('NO SINGULAR POINTS'), NoSingular is raised.
CCFD also returns the margins of its decisions, so a test can show that no last-bit
difference in a mean can flip one.  Also the planted inputs and the loader of the
host check build.
"""
import ctypes
import functools
import os
import sys

import numpy as np

import score_ref as sr

REALMAX = sys.float_info.max


class NoSingular(RuntimeError):
    pass


# ----------------------------------------------------------------------------
# CCFD.m
# ----------------------------------------------------------------------------
def stable_descending(rho):
    """[~, ordrho] = sort(rho, 'descend'): equal values keep their index order."""
    return sorted(range(len(rho)), key=lambda i: -rho[i])


def sweeps(dist, dc):
    """CCFD.m:18-61: (rho, ordrho, delta, nneigh, maxd); delta(ordrho(1)) already max(delta)."""
    ND = dist.shape[0]
    rho = [0.0] * ND
    for i in range(ND - 1):
        for j in range(i + 1, ND):
            if dist[i, j] < dc:
                rho[i] = rho[i] + 1.0
                rho[j] = rho[j] + 1.0
    maxd = float(np.max(dist))
    ordrho = stable_descending(rho)
    delta = [0.0] * ND
    nneigh = [-1] * ND
    delta[ordrho[0]] = -1.0
    for ii in range(1, ND):
        delta[ordrho[ii]] = maxd
        for jj in range(ii):
            if dist[ordrho[ii], ordrho[jj]] < delta[ordrho[ii]]:
                delta[ordrho[ii]] = dist[ordrho[ii], ordrho[jj]]
                nneigh[ordrho[ii]] = ordrho[jj]
    delta[ordrho[0]] = max(delta)
    return rho, ordrho, delta, nneigh, maxd


def border_rho(dist, dc, cl, rho, NCLUST):
    """CCFD.m:191-206."""
    ND = dist.shape[0]
    bord_rho = [0.0] * NCLUST
    for i in range(ND - 1):
        for j in range(i + 1, ND):
            if cl[i] != cl[j] and dist[i, j] <= dc:
                rho_aver = (rho[i] + rho[j]) / 2.0
                if rho_aver > bord_rho[cl[i]]:
                    bord_rho[cl[i]] = rho_aver
                if rho_aver > bord_rho[cl[j]]:
                    bord_rho[cl[j]] = rho_aver
    return bord_rho


def CCFD(dist, percent, pur, k=3, dc=None):
    dist = np.asarray(dist, dtype=np.float64)
    if dc is None:
        sda = np.sort(np.asarray(pur, dtype=np.float64).reshape(-1))
        dc = sda[0] + (sda[-1] - sda[0]) * percent / 100
    ND = dist.shape[0]
    rho, ordrho, delta, nneigh, maxd = sweeps(dist, dc)

    gamma = [rho[i] * delta[i] for i in range(ND)]
    mgamma = sum(gamma) / ND
    threshold = 2 * mgamma
    useid = [0 if gamma[i] > threshold else 1 for i in range(ND)]
    kept = [gamma[i] for i in range(ND) if useid[i] == 1]
    if len(kept) < 1:
        raise NoSingular("NO SINGULAR POINTS")       # mean and cov of nothing: NaN, no point passes
    mgamma = sum(kept) / len(kept)
    covgamma = sum((g - mgamma) ** 2 for g in kept) / (len(kept) - 1) if len(kept) > 1 else 0.0
    nfivesigma = mgamma + 5 * np.sqrt(covgamma)
    pfivesigma = mgamma - 5 * np.sqrt(covgamma)
    singid = [i for i in range(ND) if gamma[i] > nfivesigma] + [i for i in range(ND) if gamma[i] < pfivesigma]
    margins = dict(trim=min(abs(g - threshold) / max(abs(threshold), 1e-300) for g in gamma),
                   sigma=min(min(abs(g - nfivesigma), abs(g - pfivesigma)) / max(abs(nfivesigma), 1e-300)
                             for g in gamma))
    if len(singid) < 1:
        raise NoSingular("NO SINGULAR POINTS")

    with np.errstate(all="ignore"):
        den = np.float64((max(rho) - min(rho)) + min(rho))
        k_star1 = (k * (max(delta) - min(delta)) + min(delta)) / den
        k_star2 = ((1 / k) * (max(delta) - min(delta)) + min(delta)) / den
        NCLUST = 0
        cl = [-2] * ND
        icl = []
        centre = []
        for j in singid:
            a, b = np.float64(rho[j]) / np.float64(delta[j]), np.float64(delta[j]) / np.float64(rho[j])
            centre.append(min(abs(a - 1 / k_star2) / abs(1 / k_star2), abs(b - k_star1) / abs(k_star1)))
            if a < (1 / k_star2) and b < k_star1:
                cl[j] = NCLUST
                icl.append(j)
                NCLUST += 1
    margins["centre"] = min(centre)
    if NCLUST < 1:
        raise NoSingular("NO SINGULAR POINTS")
    for i in range(ND):
        if cl[ordrho[i]] == -2:
            if nneigh[ordrho[i]] < 0:
                raise NoSingular("a point without a label has no neighbour")   # cl(0) in MATLAB
            cl[ordrho[i]] = cl[nneigh[ordrho[i]]]

    halo = list(cl)
    if NCLUST > 1:
        bord_rho = border_rho(dist, dc, cl, rho, NCLUST)
        for i in range(ND):
            if rho[i] < bord_rho[cl[i]]:
                halo[i] = -1

    fit1 = 0.0
    for j in range(NCLUST):
        s = 0.0
        for i in range(ND):
            if cl[i] == j:
                s = s + dist[i, icl[j]]
        fit1 = fit1 + s / ND                         # length(jiterm) = ND, not the cluster's size
    fit1 = fit1 / NCLUST
    if NCLUST > 1:
        tot = 0.0
        tmp = np.zeros((NCLUST, NCLUST))
        for j in range(NCLUST):
            for i in range(j + 1, NCLUST):
                tmp[j, i] = dist[icl[j], icl[i]]
                tmp[i, j] = dist[icl[j], icl[i]]
        for j in range(NCLUST):                      # sum(tmpfit2(:)): column-major
            for i in range(NCLUST):
                tot = tot + tmp[i, j]
        fit2 = tot / NCLUST / (NCLUST - 1)
    else:
        fit2 = 0.0
    with np.errstate(all="ignore"):
        fitness = float(np.float64(fit2) / np.float64(fit1))
    return dict(fitness=fitness, dc=float(dc), icl=np.array(icl, dtype=np.int64), cl=np.array(cl, dtype=np.int64),
                rho=np.array(rho, dtype=np.int64), delta=np.array(delta), nneigh=np.array(nneigh, dtype=np.int64),
                halo=np.array(halo, dtype=np.int64), rank=np.argsort(np.array(ordrho)), margins=margins)


# ----------------------------------------------------------------------------
# myccfd.m
# ----------------------------------------------------------------------------
def distance(hmms, data):
    """myccfd.m:14-30: dist(i, j) = dist(j, i) = 0.5 (kld(i, j, data_i) + kld(j, i, data_j)),
    kld = mean(ll1 - ll2) of the normalised log-likelihoods; the diagonal stays 0."""
    ND = len(hmms)
    with np.errstate(all="ignore"):
        ll = [[sr.vbhmm_ll(hmms[j], list(data[i]), "n")[0] for j in range(ND)] for i in range(ND)]
        dist = np.zeros((ND, ND))
        for i in range(ND):
            for j in range(i + 1, ND):
                kij = np.sum(ll[i][i] - ll[i][j]) / np.float64(len(data[i]))
                kji = np.sum(ll[j][j] - ll[j][i]) / np.float64(len(data[j]))
                dist[i, j] = 0.5 * (kij + kji)
                dist[j, i] = dist[i, j]
    return dist


def upper(dist):
    ND = len(dist)
    return np.array([dist[i, j] for i in range(ND) for j in range(i + 1, ND)])


def myccfd_from_dist(dist, slope=3, ccfd=CCFD, log=None):
    """myccfd.m:42-114 on a finished matrix.  ``ccfd``: the CCFD to call (a test passes a
    scripted one); ``log``: a list that receives (p0, failed) of every search call."""
    dist = np.asarray(dist, dtype=np.float64)
    pur = upper(dist)
    percent, r, cofr = 10.0, 3.0, [-1, 0, 1]
    dc, icl, cl = {}, {}, {}
    fitidx, p0 = 2, percent
    while r > 0:
        fitness = [0.0, 0.0, 0.0]
        for i in range(3):
            p0 = percent + r * cofr[i]
            try:
                res = ccfd(dist, p0, pur, slope)
                fitness[i], dc[i], icl[i], cl[i] = res["fitness"], res["dc"], res["icl"], res["cl"]
                failed = False
            except NoSingular:
                fitness[i] = -REALMAX
                failed = True
            if log is not None:
                log.append((p0, failed))
        if sum(f == max(fitness) for f in fitness) == 3:
            fitidx = 2
        else:
            fitidx = fitness.index(max(fitness))
        percent = percent + r * cofr[fitidx]
        r = r - 0.5
    if fitidx not in dc:
        raise NoSingular("the chosen candidate never succeeded")       # dc(fitidx) past the end
    star = ccfd(dist, p0, pur, slope, dc[fitidx])
    centres, label = icl[fitidx], cl[fitidx]
    NCLUST = len(centres)
    groups = [np.nonzero(label == i)[0] for i in range(NCLUST)]
    size = np.array([len(g) for g in groups], dtype=np.float64)
    result = dict(fitness=star["fitness"], percent=percent, dc=star["dc"], icl=centres, cl=label, rho=star["rho"],
                  delta=star["delta"], NCLUST=NCLUST, halo=star["halo"], dist=dist, k=slope)
    return dict(ccfd_result=result, label=label, groups=groups, weight=size / size.sum())


def purity(label, truth):
    label, truth = np.asarray(label), np.asarray(truth)
    return sum(np.bincount(truth[label == c]).max() for c in set(label.tolist())) / len(label)


# ----------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------
PLANTED = [(G, per, seed) for (G, per) in ((2, 20), (3, 12), (4, 16)) for seed in (1, 2, 3)]


@functools.lru_cache(maxsize=None)
def planted(G, per, seed):
    """(D, truth): G centres normal(size=(G, 2)) * 8, ``per`` points each at unit spread,
    Euclidean distances (bitwise symmetric, zero diagonal).  The groups are interleaved
    (point k belongs to centre k mod G).  The order matters to CCFD, which breaks ties
    between equal densities by index: with the groups stored one after the other the
    restatement merges two groups of (4, 16, seed 3) and mislabels two points of
    (4, 16, seed 1); interleaved, all nine inputs give K = G and purity 1."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(G, 2)) * 8
    truth = np.arange(G * per) % G
    pts = centres[truth] + rng.normal(size=(G * per, 2))
    n = len(pts)
    D = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = np.sqrt(np.sum((pts[i] - pts[j]) ** 2))
    D.setflags(write=False)
    return D, truth


@functools.lru_cache(maxsize=None)
def planted_reference(G, per, seed):
    """(result of myccfd_from_dist, the search log, the smallest decision margin over
    every CCFD call that succeeded)."""
    D, _ = planted(G, per, seed)
    log, margins = [], []

    def watched(*a):
        res = CCFD(*a)
        margins.append(min(res["margins"].values()))
        return res

    res = myccfd_from_dist(D, 3, watched, log)
    return res, log, min(margins)


MARGIN = 1e-9


def rel_close(a, b, rtol=1e-12):
    return abs(a - b) <= rtol * abs(b)


def check_planted(got, G, per, seed):
    """``got`` (vbhem_amd.ccfd's result on planted(G, per, seed)) equals the restatement's:
    rho, icl, cl, halo exactly, delta bit for bit, dc and fitness to 1e-12 relative."""
    res, log, margin = planted_reference(G, per, seed)
    _, truth = planted(G, per, seed)
    ref, g = res["ccfd_result"], got["ccfd_result"]
    # the restatement first: K = G, purity 1, none of the 18 search calls failed, and no
    # decision close enough to its threshold for a last-bit difference to flip it
    assert ref["NCLUST"] == G and purity(res["label"], truth) == 1.0
    assert len(log) == 18 and not any(failed for _, failed in log)
    assert margin > MARGIN
    for k in ("rho", "icl", "cl", "halo"):
        assert np.array_equal(g[k], ref[k]), k
    assert g["delta"].tobytes() == ref["delta"].tobytes()
    assert rel_close(g["dc"], ref["dc"]) and rel_close(g["fitness"], ref["fitness"])
    assert g["percent"] == ref["percent"] and g["NCLUST"] == G and g["k"] == 3
    assert np.array_equal(got["label"], res["label"]) and np.array_equal(got["weight"], res["weight"])
    assert all(np.array_equal(a, b) for a, b in zip(got["groups"], res["groups"]))


def quantised(N, seed=0, step=0.125, top=4.0):
    """A symmetric [N][N] matrix of multiples of ``step`` in (0, top], zero diagonal: ties
    between distances and between densities are the rule."""
    rng = np.random.default_rng(seed + 31 * N)
    A = np.ceil(rng.uniform(0, top, (N, N)) / step) * step
    D = np.triu(A, 1)
    D = D + D.T
    return D


def ranks_of(rho):
    """[C][N] positions in the stable descending sort of every row of rho."""
    return np.stack([np.argsort(np.array(stable_descending(list(r)))) for r in np.atleast_2d(rho)]).astype(np.int32)


# ----------------------------------------------------------------------------
# the host build of the row routines and the distance (tests/ccfdcheck/libccfdcheck.so)
# ----------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCFDCHECK_PATH = os.path.join(ROOT, "tests", "ccfdcheck", "libccfdcheck.so")


def load_ccfdcheck():
    if not os.path.exists(CCFDCHECK_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "ccfdcheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(CCFDCHECK_PATH)
    vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    dist = [ci] * 4 + [vp] * 5 + [ci] + [vp] * 4
    lib.ccfdcheck_distance_host.argtypes = dist
    lib.ccfdcheck_distance_host.restype = ctypes.c_longlong
    lib.ccfdcheck_distance_device.argtypes = dist + [vp, vp]
    lib.ccfdcheck_distance_device.restype = ci
    for name, args in (("rowstats", [vp, ci, vp, vp]), ("rho", [vp, ci, vp, ci, vp]),
                       ("delta", [vp, ci, vp, ci, cd, vp, vp]), ("border", [vp, ci, cd, vp, vp, vp])):
        fn = getattr(lib, f"ccfdcheck_{name}_host")
        fn.argtypes, fn.restype = args, None
    lib.ccfdcheck_passes_device.argtypes = [vp, ci, vp, ci, vp, cd] + [vp] * 8
    lib.ccfdcheck_passes_device.restype = ci
    return lib


def flatten(data, d):
    """(offsets int32 [N+1], x [total][d], seg int32 [H+1]) of per-HMM lists of sequences."""
    seqs = [np.asarray(a, dtype=np.float64).reshape(-1, d) for g in data for a in g]
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(a) for a in seqs])
    x = np.ascontiguousarray(np.concatenate(seqs) if off[-1] > 0 else np.zeros((1, d)))
    seg = np.zeros(len(data) + 1, dtype=np.int32)
    seg[1:] = np.cumsum([len(g) for g in data])
    return off, x, seg


def run_distance_check(lib, packed, data, d, device=False):
    """(status, D[, rowmin, rowmax]) of the packed HMMs (score.pack_hmms) and their data."""
    H, KM = packed["prior"].shape
    off, x, seg = flatten(data, d)
    arrs = [np.ascontiguousarray(packed[k]) for k in ("nstates", "prior", "trans", "mean", "cov")]
    D = np.full((H, H), 7.0)
    args = [H, KM, d, int(packed["covmode"]), *[a.ctypes.data for a in arrs], len(off) - 1, off.ctypes.data,
            x.ctypes.data, seg.ctypes.data, D.ctypes.data]
    if not device:
        return int(lib.ccfdcheck_distance_host(*args)), D
    mn, mx = np.zeros(H), np.zeros(H)
    return int(lib.ccfdcheck_distance_device(*args, mn.ctypes.data, mx.ctypes.data)), D, mn, mx


def run_passes_host(lib, D, dcs, rank, maxd, cl, rho_b):
    """dict(rowmin, rowmax, rho [C][N], delta, nneigh, border) of the host loops (border at dcs[0])."""
    D = np.ascontiguousarray(D, dtype=np.float64)
    N, C = len(D), len(dcs)
    dcs = np.ascontiguousarray(dcs, dtype=np.float64)
    rank, cl, rho_b = (np.ascontiguousarray(a, dtype=np.int32) for a in (rank, cl, rho_b))
    out = dict(rowmin=np.zeros(N), rowmax=np.zeros(N), rho=np.zeros((C, N), dtype=np.int32),
               delta=np.zeros((C, N)), nneigh=np.zeros((C, N), dtype=np.int32), border=np.zeros(N))
    p = lambda a: a.ctypes.data
    lib.ccfdcheck_rowstats_host(p(D), N, p(out["rowmin"]), p(out["rowmax"]))
    lib.ccfdcheck_rho_host(p(D), N, p(dcs), C, p(out["rho"]))
    lib.ccfdcheck_delta_host(p(D), N, p(rank), C, float(maxd), p(out["delta"]), p(out["nneigh"]))
    lib.ccfdcheck_border_host(p(D), N, float(dcs[0]), p(cl), p(rho_b), p(out["border"]))
    return out


def run_passes_device(lib, D, dcs, rank, maxd, cl, rho_b):
    D = np.ascontiguousarray(D, dtype=np.float64)
    N, C = len(D), len(dcs)
    dcs = np.ascontiguousarray(dcs, dtype=np.float64)
    rank, cl, rho_b = (np.ascontiguousarray(a, dtype=np.int32) for a in (rank, cl, rho_b))
    out = dict(rowmin=np.zeros(N), rowmax=np.zeros(N), rho=np.zeros((C, N), dtype=np.int32),
               delta=np.zeros((C, N)), nneigh=np.zeros((C, N), dtype=np.int32), border=np.zeros(N))
    p = lambda a: a.ctypes.data
    rc = lib.ccfdcheck_passes_device(p(D), N, p(dcs), C, p(rank), float(maxd), p(cl), p(rho_b), p(out["rowmin"]),
                                     p(out["rowmax"]), p(out["rho"]), p(out["delta"]), p(out["nneigh"]),
                                     p(out["border"]))
    return int(rc), out


def passes_restated(D, dcs, cl, rho_b):
    """What the four passes must give at the cut-offs ``dcs``, from sweeps() and plain
    loops: rowmin, rowmax, rho [C][N], rank [C][N], delta and nneigh [C][N] (the
    top-ranked row with the placeholder -1), border [N] at dcs[0] for the labels ``cl``
    and densities ``rho_b``, and maxd."""
    D = np.asarray(D, dtype=np.float64)
    N, C = len(D), len(dcs)
    rho, rank = np.zeros((C, N), dtype=np.int64), np.zeros((C, N), dtype=np.int64)
    delta, nneigh = np.zeros((C, N)), np.zeros((C, N), dtype=np.int64)
    for c in range(C):
        r, ordrho, dl, nn, maxd = sweeps(D, dcs[c])
        rho[c], delta[c], nneigh[c] = r, dl, nn
        rank[c] = np.argsort(np.array(ordrho))
        delta[c, ordrho[0]] = -1.0
    border = np.zeros(N)
    for i in range(N):
        for j in range(N):
            if cl[i] != cl[j] and D[i, j] <= dcs[0]:
                border[i] = max(border[i], (rho_b[i] + rho_b[j]) / 2.0)
    up = [D[i, i + 1:] for i in range(N)]
    rowmin = np.array([u.min() if len(u) else np.inf for u in up])
    rowmax = np.array([u.max() if len(u) else -np.inf for u in up])
    return dict(rowmin=rowmin, rowmax=rowmax, rho=rho, rank=rank, delta=delta, nneigh=nneigh, border=border,
                maxd=float(np.max(D)))


PASS_SIZES = (2, 3, 63, 64, 65, 257)   # a wave of 64 lanes, one past it, more than a workgroup of 256


@functools.lru_cache(maxsize=None)
def pass_case(N):
    """(D, dcs, cl, rho_b, expected): a quantised matrix, three cut-offs of which the
    middle one equals an entry, labels of three clusters, and passes_restated of them.
    Row 0 of the matrices with N >= 3 is at the largest distance from every point, so
    it has no neighbour below maxd whatever its rank."""
    D = quantised(N, seed=1)
    if N >= 3:
        D[0, 1:] = D[1:, 0] = 5.0
    dcs = [1.0625, float(D[N - 1, N - 2]), 3.5]
    cl = (np.arange(N) * 7 // 3) % 3
    rho_b = np.asarray(sweeps(D, dcs[0])[0], dtype=np.int64)
    D.setflags(write=False)
    return D, dcs, cl, rho_b, passes_restated(D, dcs, cl, rho_b)


# distance cases: the HMMs of score_ref.make_case, every HMM with its own ragged trials
TRIAL_LENGTHS = ([1, 2, 17, 5], [3, 1], [7, 1, 4, 2, 9])


@functools.lru_cache(maxsize=None)
def distance_case(K, d, diag):
    """(hmms, data_by_hmm, the restatement's distance matrix) of one score_ref shape."""
    hmms = sr.make_case(K, d, diag)[0]
    rng = np.random.default_rng(500 * K + 10 * d + int(diag))
    data = [sr.sample_data(rng, [h], lens, d) for h, lens in zip(hmms, TRIAL_LENGTHS)]
    return hmms, data, distance(hmms, data)
