"""What the batched VB-HMM EM tests share: the inputs, the oracle's results (computed
once per session), the loader of the host check build (tests/vbhmmemcheck) and the
comparison under the iteration-count condition.

Inputs:
  (a) the demo's 10 subjects, K = 1:3, 4 trials for K > 1 (1 for K = 1), the GMMs from
      random_gmm with default_rng(100) per (subject, K): 90 runs;
  (b) one seeded synthetic subject of 70 sequences (the lane rounds see 64 + 6) with
      lengths uniform in 1..49 including T = 1, two Gaussian states in 2-D,
      K in {1, 2, 3, 5} (5 uses KM = 8), 3 trials each: 12 runs;
  (c) edge subjects: exactly 64 and 65 sequences, a single sequence, dim = 3 and dim = 8
      with K = 2, and one list that interleaves K = 1, 2, 3 runs of different subjects;
  (d) the corners of the kernels' buckets (runs_d): per (K, dim) one subject drawn from K
      well-separated states (states_subject), 3 GMM-initialised runs at K.  Scalar W0 at
      (K, dim) = (4, 2), (4, 8), (8, 2), (8, 8), (6, 4), (7, 5), (5, 8), (2, 1), (8, 1); a
      diagonal, unequal W0 = 0.001 (1 + a) at (8, 8) and (3, 2).  (8, 1) has a fourth run
      whose first state starts empty (Nk ~ 1e-45: the 1e-50 guards);
  (e) shapes of one subject (runs_e), K = 2 and 3: 130 sequences of 1..3 steps, 4 sequences
      of which one has 300 steps (dim = 3), and 14 sequences of which the first, the last
      and two adjacent ones are empty.

Inputs (d) and (e) get NO near-threshold exclusion: their seeds are chosen so that
near_threshold is false for every oracle trajectory, and the tests assert that
compare_with_oracle leaves no run out.  One figure of theirs is close to its tolerance:
the first-iteration t1_S of run 0 of (8, 8) with the diagonal W0 is 9.95e-11 (walker) and
9.5e-11 (device) from the oracle against RTOL_PAIRS = 1e-10.  That run's initial W (from
inv, not symmetrised) is asymmetric by 2e-14; the run routines take log det from its lower
triangle, the oracle from the whole matrix, 3e-12 apart.  The tolerance
stays.
"""
import ctypes
import os
import subprocess

import numpy as np

import vbhmm_em_oracle as vho

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_PATH = os.path.join(ROOT, "tests", "vbhmmemcheck", "libvbhmmemcheck.so")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

# demo/vbdemo_face.m:21-31, as tests/test_vbhmm_em.py
DEMO_VBOPT = dict(alpha0=1.0, mu0=[160.0, 210.0], W0=0.001, beta0=1.0, v0=10.0, epsilon0=1.0, seed=100)

_cache = {}


def em_mod():
    import pkgload
    pkgload.load()
    from vbhem_amd import vbhmm_em
    return vbhmm_em


def options(dim=2, **over):
    o = dict(DEMO_VBOPT)
    if dim != 2:
        o.update(mu0=[150.0 + 10.0 * a for a in range(dim)], v0=float(dim + 8))
    o.update(over)
    return em_mod().vbhmm_default_options(dim, **o)


def demo_subjects():
    fx = np.load(os.path.join(GOLDEN_DIR, "demo_fixations.npz"))
    off, x, subj = fx["offsets"], fx["x"], fx["subject"]
    seqs = [x[off[n]:off[n + 1]] for n in range(off.size - 1)]
    return [[s for s, g in zip(seqs, subj) if g == i] for i in range(len(fx["names"]))]


def gaussian_subject(seed, lens, dim=2):
    """Sequences from two Gaussian states (sticky transitions), ~20 px spread."""
    rng = np.random.default_rng(seed)
    mu = np.stack([150.0 + 10.0 * np.arange(dim), 210.0 - 12.0 * np.arange(dim)])
    out = []
    for T in lens:
        z, seq = int(rng.integers(2)), []
        for _ in range(int(T)):
            seq.append(mu[z] + rng.normal(0.0, 20.0, dim))
            if rng.random() < 0.3:
                z = 1 - z
        out.append(np.array(seq).reshape(-1, dim))
    return out


def synthetic_subject():
    rng = np.random.default_rng(2024)
    lens = rng.integers(1, 50, 70)
    lens[3] = 1          # T = 1 is in whatever the draw gave
    lens[68] = 49
    return gaussian_subject(7, lens)


def gmm_trials(data, K, n, seed=100):
    rng = np.random.default_rng(seed)
    return [em_mod().random_gmm(data, K, rng) for _ in range(n)]


def runs_a():
    """[(subject index, K, gmm)] of input (a) and its subjects."""
    if "a" not in _cache:
        subj = demo_subjects()
        runs = [(s, K, g) for s, d in enumerate(subj) for K in (1, 2, 3)
                for g in gmm_trials(d, K, 1 if K == 1 else 4)]
        _cache["a"] = (subj, runs)
    return _cache["a"]


def runs_b():
    if "b" not in _cache:
        subj = [synthetic_subject()]
        runs = [(0, K, g) for K in (1, 2, 3, 5) for g in gmm_trials(subj[0], K, 3)]
        _cache["b"] = (subj, runs)
    return _cache["b"]


def runs_c(dim):
    """Edge subjects of one dimension.  dim = 2: subjects of 64, 65 and 1 sequences with
    K = 1, 2, 3 runs interleaved across the subjects; dim = 3, 8: one subject, K = 2."""
    key = ("c", dim)
    if key not in _cache:
        if dim == 2:
            rng = np.random.default_rng(5)
            subj = [gaussian_subject(11, rng.integers(1, 6, 64)), gaussian_subject(12, rng.integers(1, 6, 65)),
                    gaussian_subject(13, [9])]
            per = {(s, K): gmm_trials(subj[s], K, 1, seed=40 + s)[0] for s in range(3) for K in (1, 2, 3)}
            order = [(0, 1), (1, 2), (2, 3), (0, 3), (1, 1), (2, 2), (0, 2), (1, 3), (2, 1)]
            runs = [(s, K, per[(s, K)]) for s, K in order]
        else:
            subj = [gaussian_subject(20 + dim, np.random.default_rng(dim).integers(2, 8, 30), dim)]
            runs = [(0, 2, g) for g in gmm_trials(subj[0], 2, 2, seed=60 + dim)]
        _cache[key] = (subj, runs)
    return _cache[key]


def states_subject(seed, C, dim, lens):
    """Sequences from C well-separated Gaussian states in dim dimensions: state c's mean
    is 150 + 60 perm[c] + 10 a + N(0, 15) in coordinate a, the spread 20, and a step leaves
    its state for a uniformly drawn one with probability 0.3.  A length of 0 gives an
    empty [0][dim] sequence."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(C)
    mu = 150.0 + 60.0 * perm[:, None] + 10.0 * np.arange(dim)[None, :] + rng.normal(0.0, 15.0, (C, dim))
    out = []
    for T in lens:
        z, seq = int(rng.integers(C)), np.zeros((int(T), dim))
        for t in range(int(T)):
            seq[t] = mu[z] + rng.normal(0.0, 20.0, dim)
            if rng.random() < 0.3:
                z = int(rng.integers(C))
        out.append(seq)
    return out


# (K, dim, diagonal W0): the corners of the kernels' buckets.  K = 4 and 8 fill KM, K * dim
# = 64 leaves no spare lane, K * dim * dim = 512 is 8 rounds of the covariance loop.
CASES_D = [(4, 2, False), (4, 8, False), (8, 2, False), (8, 8, False), (6, 4, False), (7, 5, False),
           (5, 8, False), (2, 1, False), (8, 1, False), (8, 8, True), (3, 2, True)]
# the seed of each case's subject and GMM draws where it is not 0: the first of 0, 1, .. for
# which no oracle trajectory of the case comes within 1 % of minDiff of the stopping
# threshold (near_threshold asks for 0.01 %)
SEEDS_D = {"d4x8": 1}
NAMES_D = [f"d{K}x{dim}" + ("w" if w else "") for K, dim, w in CASES_D]
NAMES_E = ["e130", "e300", "e0"]
SEEDS_E = {"e130": 1}


def diag_W0(dim):
    return [0.001 * (1 + a) for a in range(dim)]


def runs_d(name):
    """One case of input (d): a subject of 40 sequences of 1..12 steps from K states, 3
    GMM-initialised runs at K.  (subj, runs, opt)."""
    key = ("d", name)
    if key not in _cache:
        K, dim, w = CASES_D[NAMES_D.index(name)]
        seed = SEEDS_D.get(name, 0)
        lens = np.random.default_rng(1000 + seed).integers(1, 13, 40)
        subj = [states_subject(2000 + 100 * seed + 10 * K + dim, K, dim, lens)]
        runs = [(0, K, g) for g in gmm_trials(subj[0], K, 3, seed=3000 + seed)]
        if (K, dim) == (8, 1):
            # a fourth run whose first component is heavy and far from every observation:
            # the state's first-iteration gamma is ~1e-48 and less, Nk and Nk1 are of the
            # size of the 1e-50 they are guarded with, xbar is a quotient of two such numbers
            far = {k: np.array(v, dtype=np.float64, copy=True) for k, v in runs[0][2].items()}
            far["mean"][0] = 5000.0
            far["prior"][:] = [0.93] + [0.01] * 7
            runs.append((0, K, far))
        _cache[key] = (subj, runs, options(dim, W0=diag_W0(dim)) if w else options(dim))
    return _cache[key]


EMPTY_AT = (0, 5, 6, 13)     # first, two adjacent in the middle, last (of 14)


def runs_e(name):
    """One case of input (e).  e130: 130 sequences of 1..3 steps (a third round of lanes),
    dim = 2; e300: 4 sequences, one of 300 steps, dim = 3; e0: 14 sequences of which the
    first, the last and two adjacent ones in the middle are empty, dim = 2.  K = 2 and 3,
    2 runs each.  (subj, runs, opt)."""
    key = ("e", name)
    if key not in _cache:
        seed = SEEDS_E.get(name, 0)
        rng = np.random.default_rng(4000 + seed)
        if name == "e130":
            dim, lens = 2, rng.integers(1, 4, 130)
        elif name == "e300":
            dim, lens = 3, np.array([7, 300, 1, 12])
        else:
            dim, lens = 2, rng.integers(2, 9, 14)
            lens[list(EMPTY_AT)] = 0
        subj = [states_subject(5000 + seed, 3, dim, lens)]
        runs = [(0, K, g) for K in (2, 3) for g in gmm_trials(subj[0], K, 2, seed=6000 + seed)]
        _cache[key] = (subj, runs, options(dim))
    return _cache[key]


def runs_mixed():
    """K = 8 and K = 5 runs at dim = 8 of two subjects of different sizes (input d8x8's 40
    sequences and one of 15), interleaved so that larger and smaller runs alternate."""
    if "mixed" not in _cache:
        big, r8, opt = runs_d("d8x8")
        small = states_subject(2500, 5, 8, np.random.default_rng(2501).integers(4, 13, 15))
        subj = [big[0], small]
        b5 = [(0, 5, g) for g in gmm_trials(subj[0], 5, 2, seed=2502)]
        s5 = [(1, 5, g) for g in gmm_trials(subj[1], 5, 2, seed=2503)]
        _cache["mixed"] = (subj, [r8[0], s5[0], b5[0], r8[1], s5[1], r8[2], b5[1]], opt)
    return _cache["mixed"]


def corner_input(name):
    """(subj, runs, opt) of a case of input (d) or (e) by its name."""
    return runs_d(name) if name in NAMES_D else runs_e(name)


def without_empty(subj):
    return [[a for a in d if a.shape[0] > 0] for d in subj]


def oracle_runs(name, subj, runs, opt):
    """vbhmm_em_oracle.em(..., fb_fn='c') of every run, once per session."""
    key = ("oracle", name)
    if key not in _cache:
        _cache[key] = [vho.em(subj[s], K, opt, g, fb_fn="c") for s, K, g in runs]
    return _cache[key]


# ----------------------------------------------------------------------------
# packing and the check library
# ----------------------------------------------------------------------------
def pack_subjects(subj, dim):
    seqs = [np.asarray(a, dtype=np.float64).reshape(-1, dim) for d in subj for a in d]
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([a.shape[0] for a in seqs])
    first = np.zeros(len(subj) + 1, dtype=np.int32)
    first[1:] = np.cumsum([len(d) for d in subj])
    return off, np.ascontiguousarray(np.concatenate(seqs)), first


def initial_posteriors(subj, runs, opt):
    """vbhmm_init of every run (a gmm, or a dict with alpha .. W used as it is)."""
    em = em_mod()
    out = []
    for s, K, g in runs:
        if "alpha" in g:
            out.append(g)
        else:
            X = np.concatenate([np.asarray(a, dtype=np.float64) for a in subj[s]])
            out.append(em.vbhmm_init([X], K, opt, g))
    return out


def load_check():
    if "lib" not in _cache:
        if not os.path.exists(CHECK_PATH):
            subprocess.run(["make", "-C", ROOT, "vbhmmemcheck"], check=True, stdout=subprocess.DEVNULL)
        import torch  # noqa: F401  (the library binds to the HIP runtime torch loaded)
        lib = ctypes.CDLL(CHECK_PATH)
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        lib.vbhmmemcheck_host.argtypes = [ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, ci, cd] + [vp] * 7
        lib.vbhmmemcheck_host.restype = ci
        lib.vbhmmemcheck_device.argtypes = [ci, ci, vp, vp, vp, ci, ci, vp, vp, vp, vp, ci, cd, ci] + [vp] * 7
        lib.vbhmmemcheck_device.restype = ci
        _cache["lib"] = lib
    return _cache["lib"]


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_check(subj, runs, opt, where="host", max_iter=None, chunk_runs=0, KM=None, expect=0):
    """Every run through the host walker (where='host') or the library's kernels on
    device 0 ('device').  One dict per run: LL, LLs, iters, status, varpar,
    varpar_estep, Nk1, Nk, M, xbar, t1_S, and ``raw`` (the packed output rows, for
    bitwise comparisons)."""
    em = em_mod()
    dim = len(opt["mu0"])
    lib = load_check()
    off, x, first = pack_subjects(subj, dim)
    mixes = initial_posteriors(subj, runs, opt)
    Ks = np.array([r[1] for r in runs], dtype=np.int32)
    sub = np.array([r[0] for r in runs], dtype=np.int32)
    KM = KM or (4 if Ks.max() <= 4 else 8 if Ks.max() <= 8 else 16)
    R = len(runs)
    PL, SL = em.em_post_len(KM, dim), em.em_stats_len(KM, dim)
    post = np.ascontiguousarray(np.stack([em.pack_posterior(m, K, KM, dim) for m, K in zip(mixes, Ks)]))
    W0 = np.asarray(opt["W0"], dtype=np.float64)
    W0inv = np.linalg.inv(float(W0) * np.eye(dim) if W0.size == 1 else np.diag(W0.reshape(-1)))
    hv = np.ascontiguousarray(em.em_hyper_vector(opt, W0inv))
    mi = int(max_iter if max_iter is not None else opt["maxIter"])
    o_post, o_est, o_st = np.zeros((R, PL)), np.zeros((R, PL)), np.zeros((R, SL))
    o_LL, o_it, o_ss = np.zeros(R), np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    o_LLs = np.zeros((R, mi))
    args = [len(subj), dim, _ptr(off), _ptr(x), _ptr(first), R, KM, _ptr(sub), _ptr(Ks), _ptr(post), _ptr(hv),
            mi, float(opt["minDiff"])]
    outs = [_ptr(a) for a in (o_post, o_est, o_st, o_LL, o_it, o_ss, o_LLs)]
    if where == "host":
        rc = lib.vbhmmemcheck_host(*args, *outs)
    else:
        rc = lib.vbhmmemcheck_device(*args, int(chunk_runs), *outs)
    assert rc == expect, (where, rc)
    if rc != 0:
        return None
    out = []
    for r in range(R):
        K = int(Ks[r])
        st = em.unpack_stats(o_st[r], K, KM, dim)
        out.append(dict(LL=float(o_LL[r]), iters=int(o_it[r]), status=int(o_ss[r]),
                        LLs=o_LLs[r, :int(o_it[r])].copy(), varpar=em.unpack_posterior(o_post[r], K, KM, dim),
                        varpar_estep=em.unpack_posterior(o_est[r], K, KM, dim),
                        raw=(o_post[r].copy(), o_est[r].copy(), o_st[r].copy(), o_LLs[r].copy(),
                             float(o_LL[r]), int(o_it[r]), int(o_ss[r])), **st))
    return out


def same_bits(a, b, KM_differs=False):
    """Two results of run_check: every output identical, NaN patterns included.  Across KM
    the packed rows have different lengths: the states' own entries are compared."""
    if KM_differs:
        own = (all(np.array_equal(a[g][k], b[g][k], equal_nan=True)
                   for g in ("varpar", "varpar_estep") for k in POST_KEYS)
               and all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("Nk1", "Nk", "M", "xbar", "t1_S", "LLs")))
        return own and np.array_equal(a["LL"], b["LL"], equal_nan=True) and a["raw"][5:] == b["raw"][5:]
    return (all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a["raw"][:4], b["raw"][:4]))
            and (a["raw"][4] == b["raw"][4] or (np.isnan(a["raw"][4]) and np.isnan(b["raw"][4])))
            and a["raw"][5:] == b["raw"][5:])


# ----------------------------------------------------------------------------
# comparison with the oracle
# ----------------------------------------------------------------------------
POST_KEYS = ("alpha", "epsilon", "beta", "v", "m", "W")


def near_threshold(LLs, min_diff):
    """The oracle's own trajectory passes within 1e-4 minDiff of the stopping threshold
    at some iteration: | |dL / L| - minDiff | < 1e-4 minDiff."""
    LLs = np.asarray(LLs, dtype=np.float64)
    if LLs.size < 2:
        return False
    rel = np.abs((LLs[1:] - LLs[:-1]) / LLs[:-1])
    return bool((np.abs(rel - min_diff) < 1e-4 * min_diff).any())


def compare_with_oracle(got, ref, opt, post_err, tag=""):
    """LLs at rtol 1e-9, both the final posterior with post_err < 1e-8, iters and status
    equal -- except for runs whose oracle trajectory is near the threshold (at most 1
    run in 20), which are compared up to the shorter trajectory.  ``got`` entries give
    LLs, iters, status (0 converged, 1 max_iter, 2 unstable) and varpar."""
    excluded = 0
    for i, (g, r) in enumerate(zip(got, ref)):
        ref_status = 1 if (r["iters"] == opt["maxIter"] and not _converged(r["LLs"], opt["minDiff"])) else 0
        if near_threshold(r["LLs"], opt["minDiff"]) and (g["iters"] != r["iters"] or g["status"] != ref_status):
            excluded += 1
            n = min(len(g["LLs"]), len(r["LLs"]))
            np.testing.assert_allclose(g["LLs"][:n], r["LLs"][:n], rtol=1e-9, err_msg=f"{tag} run {i}")
            continue
        assert g["iters"] == r["iters"], (tag, i, g["iters"], r["iters"])
        assert g["status"] == ref_status, (tag, i, g["status"], ref_status)
        np.testing.assert_allclose(g["LLs"], r["LLs"], rtol=1e-9, err_msg=f"{tag} run {i}")
        for k in POST_KEYS:
            assert post_err(g["varpar"][k], r["varpar"][k]) < 1e-8, (tag, i, k)
    assert excluded * 20 <= len(got), (tag, excluded, len(got))
    return excluded


def _converged(LLs, min_diff):
    return len(LLs) > 1 and abs((LLs[-1] - LLs[-2]) / LLs[-2]) <= min_diff


def oracle_estep_posterior(subj_data, K, opt, gmm, iters):
    """The oracle's posterior AT its last E-step: the EM again, stopped one M-step early
    (maxIter = iters - 1 ends with the M-step that precedes E-step ``iters``)."""
    if iters == 1:
        mix = vho.init_from_gmm(subj_data, K, opt, gmm)
        return dict(alpha=mix["alpha"], epsilon=mix["epsilon"], beta=mix["beta"], v=mix["v"], m=mix["m"].T,
                    W=mix["W"].transpose(2, 0, 1))
    return vho.em(subj_data, K, dict(opt, maxIter=iters - 1, minDiff=0.0), gmm, fb_fn="c")["varpar"]


def oracle_first_iteration(subj_data, K, opt, gmm):
    """Nk1, Nk, M, xbar, t1_S and the bound of the oracle's first iteration: the
    statistics as vbhmm_em_oracle.em takes them, from the C forward-backward at the
    initial posterior."""
    import vbhem_oracle as vo
    dim = len(opt["mu0"])
    data = [np.asarray(a, float).reshape(-1, dim) for a in subj_data]
    mix = vho.init_from_gmm(data, K, opt, gmm)
    vp = dict(v=mix["v"], W=mix["W"].transpose(2, 0, 1), epsilon=mix["epsilon"], alpha=mix["alpha"],
              m=mix["m"].T, beta=mix["beta"])
    f = vo.c_vbhmm_fb(data, vp, vo.vbhmm_prelude(vp))
    gam = f["gamma"].transpose(2, 1, 0)
    t_Nk1 = gam.sum(axis=1)
    Nk1, Nk = t_Nk1[:, 0] + 1e-50, t_Nk1.sum(axis=1) + 1e-50
    M = f["xi_sum"].transpose(1, 2, 0).sum(axis=2)
    xbar, S = np.zeros((K, dim)), np.zeros((K, dim, dim))
    for k in range(K):
        acc = np.zeros(dim)
        for n, a in enumerate(data):
            for t in range(a.shape[0]):
                acc += a[t] * gam[k, n, t]
        xbar[k] = acc / Nk[k]
        acc = np.zeros((dim, dim))
        for n, a in enumerate(data):
            for t in range(a.shape[0]):
                d1 = a[t] - xbar[k]
                acc += gam[k, n, t] * np.outer(d1, d1)
        S[k] = acc / Nk[k]
    L1 = vho.em(data, K, dict(opt, maxIter=1), gmm, fb_fn="c")["LLs"][0]
    return dict(Nk1=Nk1, Nk=Nk, M=M, xbar=xbar, t1_S=S, L=L1)


# ----------------------------------------------------------------------------
# the unstable run (host walker and device)
# ----------------------------------------------------------------------------
def unstable_runs():
    """Three runs of demo subject 0: K = 2, an initial posterior whose W_1 has a negative
    determinant (log det = NaN), K = 3."""
    subj, runs = runs_a()
    opt = options()
    good = [r for r in runs if r[0] == 0 and r[1] in (2, 3)]
    a, b = good[0], [r for r in good if r[1] == 3][0]
    bad = dict(initial_posteriors(subj, [a], opt)[0])
    bad["W"] = np.array(bad["W"], copy=True)
    bad["W"][0] = np.diag([-1e-3, 1e-3])
    return subj, [a, (0, 2, bad), b], opt, bad


def check_unstable(where):
    subj, runs, opt, bad = unstable_runs()
    got = run_check(subj, runs, opt, where)
    u = got[1]
    assert u["status"] == 2 and u["iters"] == 1 and u["LL"] == -np.inf
    assert u["LLs"].tolist() == [-np.inf]
    for k in POST_KEYS:
        assert np.array_equal(u["varpar"][k], np.asarray(bad[k], dtype=np.float64)), k
    for i in (0, 2):
        alone = run_check(subj, [runs[i]], opt, where)[0]
        assert np.isfinite(got[i]["LL"]) and got[i]["status"] == 0
        assert same_bits(got[i], alone), i
