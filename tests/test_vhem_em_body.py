"""The M-step and the next E-step constants of one (cluster, state) of a VHEM EM trial as
one shared function (csrc/vhem_em_iter_body.h: one wavefront of the batched-trials kernel
runs it on the device), checked on the CPU through its host build (tests/vhememcheck: the
one-lane wave, the same elimination entry by entry) against vhem.hem_mstep +
host.vhem_cluster_constants on random packed statistics.

The bars are those of the GPU tests (tests/test_vhem_em_trials_gpu.py): every parameter
and every constant within 1e-9 normwise.  The covariances are built with a condition
number of at most 1e4 (asserted), so an inverse by Gauss-Jordan without pivoting and one
by LAPACK's LU agree to about 1e4 * 2^-52 * d ~ 4e-11 at d = 16, inside the bar."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pkgload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_PATH = os.path.join(ROOT, "tests", "vhememcheck", "libvhememcheck.so")
BAR = 1e-9
PARAMS = ("omega", "prior", "A", "centres", "covars", "emit_vcounts")
CONSTS = ("logA", "logPi", "m", "P", "c")

vb = pkgload.load()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(CHECK_PATH):
        subprocess.run(["make", "-C", ROOT, "vhememcheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(CHECK_PATH)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.vhememcheck_body.argtypes = [ctypes.c_int] * 6 + [ctypes.c_double] + [dp] * 13
    lib.vhememcheck_body.restype = ctypes.c_int
    return lib


def rel_err(a, b):
    """Normwise: max|a - b| / max|b|; -inf must sit at the same places."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    inf = np.isneginf(b)
    assert np.array_equal(np.isneginf(a), inf)
    if inf.all():
        return 0.0
    return float(np.max(np.abs(a[~inf] - b[~inf])) / max(np.max(np.abs(b[~inf])), 1e-300))


def random_stats(K, S, d, cov, seed, cond=1e4):
    """Packed VHEM statistics (Nj | N1 | M | LogL 0 | U = Nr, Y, SC) of K S states with
    weight w, mean mu and covariance C: Y = w mu, SC = w (C + mu mu').  Returns the
    vector and the largest condition number of C + reg_cov I."""
    rng = np.random.default_rng(seed)
    Nj = rng.uniform(0.5, 5.0, K)
    N1 = rng.uniform(0.1, 2.0, (K, S))
    M = rng.uniform(0.1, 2.0, (K, S, S))
    w = rng.uniform(1.0, 9.0, (K, S))
    mu = rng.normal(0.0, 2.0, (K, S, d))
    worst = 1.0
    if cov == 1:
        Q = np.linalg.qr(rng.normal(size=(K, S, d, d)))[0]
        ev = np.exp(rng.uniform(0.0, np.log(cond) * 0.9, (K, S, d))) * 0.01
        C = np.einsum("ksab,ksb,kscb->ksac", Q, ev, Q)
        C = (C + np.swapaxes(C, -1, -2)) / 2
        SC = w[..., None, None] * (C + mu[..., :, None] * mu[..., None, :])
        iu = np.triu_indices(d)
        scp = SC[..., iu[0], iu[1]]
        worst = float(np.max(np.linalg.cond(C + 0.001 * np.eye(d))))
    else:
        C = np.exp(rng.uniform(0.0, np.log(cond) * 0.9, (K, S, d))) * 0.01
        scp = w[..., None] * (C + mu * mu)
        worst = float(np.max((C + 0.001).max(-1) / (C + 0.001).min(-1)))
    U = np.concatenate([w[..., None], w[..., None] * mu, scp], axis=-1)
    vec = np.concatenate([Nj, N1.ravel(), M.ravel(), [-1234.5, 0.0], U.ravel()])
    assert vec.size == vb.host.stats_len(K, S, d, cov)
    return vec, worst


def run_body(lib, K, S, d, cov, Kb, tau, reg, vec, given=None):
    """The body over every (k, s): (flag, parameters, constants).  vec None: the prelude
    of the parameters `given`."""
    dd = (d, d) if cov == 1 else (d,)
    par = dict(omega=np.zeros(K), prior=np.zeros((K, S)), A=np.zeros((K, S, S)),
               centres=np.zeros((K, S, d)), covars=np.zeros((K, S) + dd), emit_vcounts=np.zeros((K, S)))
    if given is not None:
        for k in ("omega", "prior", "A", "centres", "covars"):
            par[k] = np.ascontiguousarray(given[k], dtype=np.float64).copy()
    con = dict(logA=np.zeros((K, S, S)), logPi=np.zeros((K, S)), m=np.zeros((K, S, d)),
               P=np.zeros((K, S) + dd), c=np.zeros((K, S)), logOmega=np.zeros(K))
    dp = ctypes.POINTER(ctypes.c_double)
    p = lambda a: a.ctypes.data_as(dp)                               # noqa: E731
    keep = np.ascontiguousarray(vec) if vec is not None else None
    sv = None if keep is None else p(keep)
    flag = lib.vhememcheck_body(K, S, d, cov, Kb, tau, reg, sv,
                                *(p(par[k]) for k in PARAMS), *(p(con[k]) for k in CONSTS),
                                p(con["logOmega"]))
    return flag, par, con


def reference(vec, K, S, d, cov, Kb, tau, reg):
    from vbhem_amd import vhem
    st = vb.host.unpack_stats(vec, K, S, d, cov)
    new = vhem.hem_mstep(st, Kb, tau, reg, cov)
    con = vb.host.vhem_cluster_constants(new, cov)
    with np.errstate(divide="ignore"):
        con["logOmega"] = np.log(new["omega"])
    return new, con


@pytest.mark.parametrize("cov", [1, 0], ids=["full", "diag"])
@pytest.mark.parametrize("d", [1, 2, 8, 16])
@pytest.mark.parametrize("S", [1, 3, 16])
def test_body_matches_numpy(lib, S, d, cov):
    K, Kb, tau, reg = 3, 11, 6, 0.001
    vec, cond = random_stats(K, S, d, cov, seed=100 * S + 10 * d + cov)
    assert cond <= 1e4
    flag, par, con = run_body(lib, K, S, d, cov, Kb, tau, reg, vec)
    want_p, want_c = reference(vec, K, S, d, cov, Kb, tau, reg)
    worst = max([rel_err(par[k], want_p[k]) for k in PARAMS] +
                [rel_err(con[k], want_c[k]) for k in CONSTS + ("logOmega",)])
    print(f"[vhem body S={S} d={d} cov={cov}] cond {cond:.3g} worst {worst:.2e}")
    assert flag == 0
    for k in PARAMS:
        assert rel_err(par[k], want_p[k]) < BAR, k
    for k in CONSTS + ("logOmega",):
        assert rel_err(con[k], want_c[k]) < BAR, k
    # the prelude of these parameters gives the same constants
    flag2, _, con2 = run_body(lib, K, S, d, cov, Kb, tau, reg, None, given=par)
    assert flag2 == 0
    for k in CONSTS + ("logOmega",):
        assert np.array_equal(con2[k], con[k]), k


@pytest.mark.parametrize("S", [1, 3])
def test_tau_1_substitutes_A(lib, S):
    K, d, cov, Kb, reg = 2, 2, 1, 7, 0.001
    vec, _ = random_stats(K, S, d, cov, seed=9 + S)
    flag, par, con = run_body(lib, K, S, d, cov, Kb, 1, reg, vec)
    want_p, want_c = reference(vec, K, S, d, cov, Kb, 1, reg)
    assert flag == 0
    assert np.array_equal(par["A"], np.repeat(np.eye(S)[None], K, 0))
    for k in PARAMS:
        assert rel_err(par[k], want_p[k]) < BAR, k
    for k in CONSTS:
        assert rel_err(con[k], want_c[k]) < BAR, k
    # 1e-12 + new_prior, as hem_mstep_component.m:138 on the substituted counts
    N1 = vec[K:K + K * S].reshape(K, S)
    assert np.array_equal(par["emit_vcounts"], 1e-12 + N1)


def test_sums_follow_numpy_bit_for_bit(lib):
    """prior, A and emit_vcounts use numpy's summation order (pairwise from 8 terms)."""
    for S in (3, 8, 13, 16):
        K, d, cov = 2, 2, 0
        vec, _ = random_stats(K, S, d, cov, seed=S)
        _, par, _ = run_body(lib, K, S, d, cov, 5, 6, 0.001, vec)
        want_p, _ = reference(vec, K, S, d, cov, 5, 6, 0.001)
        for k in ("omega", "prior", "A", "emit_vcounts", "centres"):
            assert np.array_equal(par[k], want_p[k]), (S, k)


def _flag_of(lib, vec, K=3, S=3, d=2, cov=1):
    return run_body(lib, K, S, d, cov, 11, 6, 0.001, vec)[0]


def test_fallback_flag(lib):
    K, S, d, cov = 3, 3, 2, 1
    NU = vb.host.stats_nu(d, cov)
    vec, _ = random_stats(K, S, d, cov, seed=1)
    assert _flag_of(lib, vec) == 0
    # Nj[k] == 0: omega == 0 (hem_fix_degenerate_component's test)
    v = vec.copy()
    v[1] = 0.0
    assert _flag_of(lib, v) == 1
    from vbhem_amd import vhem
    new = vhem.hem_mstep(vb.host.unpack_stats(v, K, S, d, cov), 11, 6, 0.001, cov)
    assert np.flatnonzero(new["omega"] == 0).tolist() == [1]
    # an unvisited state: its prior and its column of M zero (hem_fix_degenerate_hmm's test);
    # its other statistics stay, so nothing else is out of the ordinary
    v = vec.copy()
    k, s = 2, 1
    v[K + k * S + s] = 0.0
    M = v[K + K * S:K + K * S + K * S * S].reshape(K, S, S)
    M[k, :, s] = 0.0
    assert _flag_of(lib, v) == 1
    new = vhem.hem_mstep(vb.host.unpack_stats(v, K, S, d, cov), 11, 6, 0.001, cov)
    assert np.argwhere(new["emit_vcounts"] == 0).tolist() == [[k, s]]
    # a zero column alone is no flag: log A = -inf is allowed
    v = vec.copy()
    v[K + K * S:K + K * S + K * S * S].reshape(K, S, S)[k, :, s] = 0.0
    assert _flag_of(lib, v) == 0
    # a NaN statistic, wherever it is
    o = K + K * S + K * S * S + 2
    for at in (0, K + 4, K + K * S + 7, o, o + 1, o + 1 + d, o + 4 * NU + NU - 1):
        v = vec.copy()
        v[at] = np.nan
        assert _flag_of(lib, v) == 1, at
    # an indefinite covariance: log det of a negative determinant
    v = vec.copy()
    v[o + 1 + d] = -abs(v[o + 1 + d]) * 10
    assert _flag_of(lib, v) == 1


def test_prelude_lets_a_zero_weight_pass(lib):
    """The constants of GIVEN parameters: omega == 0 gives logOmega = -inf and no flag (the
    E-step takes it: Z = 0 exactly); a NaN centre is flagged."""
    K, S, d, cov = 2, 3, 2, 0
    vec, _ = random_stats(K, S, d, cov, seed=4)
    _, par, _ = run_body(lib, K, S, d, cov, 5, 6, 0.001, vec)
    par["omega"] = np.array([0.0, 1.0])
    par["prior"][0, 2] = 0.0
    flag, _, con = run_body(lib, K, S, d, cov, 5, 6, 0.001, None, given=par)
    assert flag == 0 and np.isneginf(con["logOmega"][0]) and np.isneginf(con["logPi"][0, 2])
    par["centres"][1, 1, 0] = np.nan
    assert run_body(lib, K, S, d, cov, 5, 6, 0.001, None, given=par)[0] == 1


def test_shapes_outside_the_body(lib):
    vec, _ = random_stats(1, 1, 1, 0, seed=0)
    assert run_body(lib, 1, 1, 1, 0, 5, 6, 0.0, vec)[0] == 0
    dp = ctypes.POINTER(ctypes.c_double)
    none = ctypes.cast(None, dp)
    assert lib.vhememcheck_body(1, 17, 2, 1, 5, 6, 0.0, *([none] * 13)) == -1
    assert lib.vhememcheck_body(1, 2, 17, 1, 5, 6, 0.0, *([none] * 13)) == -1
