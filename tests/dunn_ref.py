"""Loop restatement of the reference's Dunn index and PPK criteria -- the judge of
tests/test_dunn.py, tests/test_kld_plan.py, tests/test_kld_jobs_gpu.py and
tests/test_dunn_gpu.py -- written from the text of
Synthetic_experiment/compute_hmms_dist.m, compute_inter_Centhmms_dist.m and
evaluate_vbhem_jounarl.m:27-57, :237-296, over score_ref.vbhmm_ll, separately from
vbhem_amd/evaluate.py.  Indices are 0-based.  Also the shared cases and the loader of the
host check build (tests/kldcheck)."""
import ctypes
import functools
import os

import numpy as np

import score_ref as sr


# ----------------------------------------------------------------------------
# restatements
# ----------------------------------------------------------------------------
def vbhmm_kld(hmm1, hmm2, data1):
    """vbhmm_kld.m with 'n': mean(ll1 - ll2) over data1 (NaN for no data)."""
    data1 = list(data1)
    with np.errstate(all="ignore"):
        ll1, ll2 = sr.vbhmm_ll(hmm1, data1, "n")[0], sr.vbhmm_ll(hmm2, data1, "n")[0]
        return float(np.sum(ll1 - ll2) / np.float64(len(data1)))


def cendata(ind_data, groups, kind, cent_ids=None):
    """compute_hmms_dist.m:18-44: per centre the pooled trials of its members ('vb', 'vh',
    'dic'), or the trials of the centre's own subject ('sc', 'ccfd': cent_ids[j])."""
    out = []
    for j, g in enumerate(groups):
        if kind in ("vb", "vh", "dic"):
            out.append([s for i in g for s in ind_data[i]])
        else:
            out.append(list(ind_data[cent_ids[j]]))
    return out


def compute_hmms_dist(cent, ind_hmms, ind_data, groups, kind, cent_ids=None):
    """compute_hmms_dist.m:47-65: per centre the array over its members."""
    cd = cendata(ind_data, groups, kind, cent_ids)
    dists = []
    for j, c in enumerate(cent):
        m = np.zeros(len(groups[j]))
        for q, i in enumerate(groups[j]):
            m[q] = 0.5 * (vbhmm_kld(c, ind_hmms[i], cd[j]) + vbhmm_kld(ind_hmms[i], c, ind_data[i]))
        dists.append(m)
    return dists


def compute_inter_dist(cent, ind_data, groups, kind, cent_ids=None):
    """compute_inter_Centhmms_dist.m:40-54: (inter_dists_vct, inter_Dists)."""
    cd = cendata(ind_data, groups, kind, cent_ids)
    n = len(cent)
    inter, vct = np.zeros((n, n)), []
    for i in range(n):
        for j in range(i + 1, n):
            inter[i, j] = 0.5 * (vbhmm_kld(cent[i], cent[j], cd[i]) + vbhmm_kld(cent[j], cent[i], cd[j]))
            vct.append(inter[i, j])
    return np.array(vct), inter


def dunn(cent, ind_hmms, ind_data, groups, kind, cent_ids=None):
    """evaluate_vbhem_jounarl.m:324-333: dict(intra, inter, inter_vct, DI)."""
    if len(cent) == 1:
        return dict(intra=[], inter=np.zeros((1, 1)), inter_vct=np.zeros(0), DI=0.0)
    intra = compute_hmms_dist(cent, ind_hmms, ind_data, groups, kind, cent_ids)
    vct, inter = compute_inter_dist(cent, ind_data, groups, kind, cent_ids)
    with np.errstate(all="ignore"):
        DI = float(np.float64(min(vct)) / np.float64(max(max(m) for m in intra)))
    return dict(intra=intra, inter=inter, inter_vct=vct, DI=DI)


def logtrick(lA):
    """logtrick.m over the rows of lA [K][N]: log(sum_k exp(lA))."""
    mv = np.max(lA, axis=0)
    return mv + np.log(np.sum(np.exp(lA - mv), axis=0))


def ppk_loglik(hmms, weight, data_by_subject):
    """evaluate_vbhem_jounarl.m:44-52 for point HMMs without counts."""
    group_data = [s for d in data_by_subject for s in d]
    ll = np.stack([sr.vbhmm_ll(h, group_data, "n")[0] for h in hmms], axis=1)     # [N][K]
    return float(np.sum(logtrick(np.log(np.asarray(weight))[:, None] + ll.T)))


def num_pars(kk, ss, dim):
    return (kk - 1) + kk * ((ss - 1) + ss * (ss - 1) + ss * 2 * dim)


def sc_aic(ppk_ll, K, S, dim, T, div_T=0):
    out = np.zeros((len(K), len(S)))
    for k, kk in enumerate(K):
        for s, ss in enumerate(S):
            out[k, s] = (-2 * ppk_ll[k][s] / T if div_T else -2 * ppk_ll[k][s]) + 2 * num_pars(kk, ss, dim)
    return out


def sc_bic(ppk_ll, K, S, dim, n_bic, T, div_T=0):
    out = np.zeros((len(K), len(S)))
    for k, kk in enumerate(K):
        for s, ss in enumerate(S):
            out[k, s] = (-2 * ppk_ll[k][s] / T if div_T else -2 * ppk_ll[k][s]) + np.log(n_bic) * num_pars(kk, ss, dim)
    return out


def kld_jobs(hmms, seqs, lists, jobs):
    """kl[p] = mean over the list's items of ll_a / T - ll_b / T, the normalised
    log-likelihoods of every HMM on every sequence computed once."""
    with np.errstate(all="ignore"):
        ll = np.array([sr.vbhmm_ll(h, list(seqs), "n")[0] for h in hmms])
        out = np.zeros(len(jobs))
        for p, (a, b, l) in enumerate(jobs):
            it = np.asarray(lists[l], dtype=np.int64)
            out[p] = np.sum(ll[a, it] - ll[b, it]) / np.float64(len(it))
    return out


# ----------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------
SEGMENTS = [3, 130, 1, 128, 127]   # inside a tile, past it, packed, filling it, one short of it
EDGE_LENGTHS = (1, 127, 128, 129, 130, 257)


@functools.lru_cache(maxsize=None)
def tile_case():
    """33 two-state HMMs in two dimensions, subject i with SEGMENTS[i % 5] trials of 1 to 3
    observations (the case of tests/test_ccfd_gpu.py, built the same way)."""
    rng = np.random.default_rng(5)
    hmms = [sr.make_hmm(rng, 2, 2, False) for _ in range(33)]
    data = [sr.sample_data(rng, [h], [int(v) for v in rng.integers(1, 4, SEGMENTS[i % 5])], 2)
            for i, h in enumerate(hmms)]
    return hmms, data


def gathered(c, kind, N):
    """c items out of N sequences: reversed (0), strided (1), repeated (2)."""
    q = np.arange(c)
    return ((N - 1 - q) % N, (7 * q) % N, (q // 2 * 3) % N)[kind].astype(np.int64)


@functools.lru_cache(maxsize=None)
def small_case():
    """6 HMMs (1 to 3 states, d = 2, diagonal) and 300 sequences of 1 to 3 observations."""
    rng = np.random.default_rng(21)
    hmms = [sr.make_hmm(rng, k, 2, True) for k in (3, 2, 3, 1, 3, 2)]
    seqs = sr.sample_data(rng, hmms, [int(v) for v in rng.integers(1, 4, 300)], 2)
    return hmms, seqs


@functools.lru_cache(maxsize=None)
def small_ll():
    """The normalised log-likelihoods [6][300] of small_case, by the restatement."""
    hmms, seqs = small_case()
    ll = np.array([sr.vbhmm_ll(h, seqs, "n")[0] for h in hmms])
    ll.setflags(write=False)
    return ll


def jobs_from_ll(ll, lists, jobs):
    out = np.zeros(len(jobs))
    with np.errstate(all="ignore"):
        for p, (a, b, l) in enumerate(jobs):
            it = np.asarray(lists[l], dtype=np.int64)
            out[p] = np.sum(ll[a, it] - ll[b, it]) / np.float64(len(it))
    return out


@functools.lru_cache(maxsize=None)
def dunn_case():
    """7 two- and three-state subject HMMs in 3 clusters of 1, 2 and 4, 3 to 5 trials of 1 to
    6 observations each, 3 centre HMMs of their own, and centre subjects taken from the
    members."""
    rng = np.random.default_rng(33)
    hmms = [sr.make_hmm(rng, 2 + i % 2, 2, False) for i in range(7)]
    data = [sr.sample_data(rng, [h], [int(v) for v in rng.integers(1, 7, 3 + i % 3)], 2) for i, h in enumerate(hmms)]
    centres = [sr.make_hmm(rng, 3, 2, False) for _ in range(3)]
    groups = [np.array([4]), np.array([6, 1]), np.array([0, 2, 5, 3])]
    centre_subjects = [4, 1, 5]
    return hmms, data, centres, groups, centre_subjects


@functools.lru_cache(maxsize=None)
def dunn_reference(pooled):
    hmms, data, centres, groups, cs = dunn_case()
    if pooled == "members":
        return dunn(centres, hmms, data, groups, "vb")
    return dunn([hmms[i] for i in cs], hmms, data, groups, "ccfd", cs)


# ----------------------------------------------------------------------------
# the host build of the planner and the walk of its tiles (tests/kldcheck/libkldcheck.so)
# ----------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KLDCHECK_PATH = os.path.join(ROOT, "tests", "kldcheck", "libkldcheck.so")
ERR_ARG = -1


def load_kldcheck():
    if not os.path.exists(KLDCHECK_PATH):
        import subprocess
        subprocess.run(["make", "-C", ROOT, "kldcheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(KLDCHECK_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.kldcheck_plan.argtypes = [ci, ci, ci, vp, vp, ci, vp, vp, ctypes.c_char_p, ci]
    lib.kldcheck_plan.restype = ci
    hm = [ci] * 4 + [vp] * 5 + [ci, vp, vp] + [ci, vp, vp, ci, vp]
    lib.kldcheck_jobs_host.argtypes = hm + [vp, vp, vp, ctypes.c_char_p, ci]
    lib.kldcheck_jobs_host.restype = ctypes.c_longlong
    lib.kldcheck_jobs_device.argtypes = hm + [vp]
    lib.kldcheck_jobs_device.restype = ci
    return lib


def flat_lists(lists):
    """(offsets int32 [L + 1], items int32) of a list of int sequences."""
    ls = [np.asarray(l, dtype=np.int32).reshape(-1) for l in lists]
    off = np.zeros(len(ls) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(l) for l in ls])
    items = np.ascontiguousarray(np.concatenate(ls) if ls else np.zeros(0), dtype=np.int32)
    return off, (items if items.size else np.zeros(1, dtype=np.int32))


def run_plan(lib, H, N, lists, jobs, offsets=None):
    """(status, message, counts) of the planner alone; counts: own slots, own tiles, lanes,
    cross tiles, the most passes of a tile, workspace bytes.  ``offsets`` overrides the
    list offsets."""
    off, items = flat_lists(lists)
    if offsets is not None:
        off = np.ascontiguousarray(offsets, dtype=np.int32)
    jb = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 3))
    counts = np.zeros(6, dtype=np.int64)
    msg = ctypes.create_string_buffer(256)
    rc = lib.kldcheck_plan(H, N, len(off) - 1, off.ctypes.data, items.ctypes.data, len(jb), jb.ctypes.data,
                           counts.ctypes.data, msg, 256)
    return int(rc), msg.value.decode(), counts


def _hmm_args(packed, seqs, d):
    H, KM = packed["prior"].shape
    lens = [int(np.asarray(a).reshape(-1, d).shape[0]) for a in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens)
    x = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1, d) for a in seqs])
                             if off[-1] > 0 else np.zeros((1, d)))
    arrs = [np.ascontiguousarray(packed[k]) for k in ("nstates", "prior", "trans", "mean", "cov")]
    keep = arrs + [off, x]
    return [H, KM, d, int(packed["covmode"]), *[a.ctypes.data for a in arrs], len(seqs), off.ctypes.data,
            x.ctypes.data], keep


def run_jobs(lib, packed, seqs, d, lists, jobs, device=False):
    """Host walk: (status, message, kl, own_hits, pair_hits); device: (status, kl) through
    vbhmm_kld_jobs on device 0."""
    args, keep = _hmm_args(packed, seqs, d)
    off, items = flat_lists(lists)
    jb = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 3))
    P = len(jb)
    kl = np.full(max(P, 1), 7.0)
    args += [len(off) - 1, off.ctypes.data, items.ctypes.data, P, jb.ctypes.data]
    if device:
        rc = lib.kldcheck_jobs_device(*args, kl.ctypes.data)
        return int(rc), kl[:P]
    pairs = int(sum(off[l + 1] - off[l] for l in jb[:, 2])) if P else 0
    uniq = {(int(a), int(l)) for a, _, l in jb}
    own = int(sum(off[l + 1] - off[l] for _, l in uniq))
    own_hits, pair_hits = np.zeros(max(own, 1), dtype=np.int32), np.zeros(max(pairs, 1), dtype=np.int32)
    msg = ctypes.create_string_buffer(256)
    rc = lib.kldcheck_jobs_host(*args, kl.ctypes.data, own_hits.ctypes.data, pair_hits.ctypes.data, msg, 256)
    del keep
    return int(rc), msg.value.decode(), kl[:P], own_hits[:own], pair_hits[:pairs]
