"""The two device-side EM loops (vbhem_em_run_trials, vhem_em_run_trials) at the dimensions
their in-wave Gauss-Jordan inverse (gauss_jordan, csrc/vbhem_em_iter_body.h) has not seen,
against the host engines, at the bars of tests/test_em_trials_dev_gpu.py and
tests/test_vhem_em_trials_gpu.py unchanged.

gauss_jordan spreads the n = 2 d^2 entries of [Mt | I] over the 64 lanes of a wave, entry
lane + 64 j in round j.  The other tests run d = 2, 3, 8, 16: n = 8 and 18 (one partial round),
128 and 512 (whole rounds only).  Here every d has a last round that only some lanes own;
the host walkers of tests/vhememcheck and tests/emderivcheck restate the elimination on one
lane and cannot see lane ownership.  Per d: n = 2 d^2, whole rounds, lanes owning an entry in the
last round (the VBHEM loop's prelude also eliminates the d x d left half alone for log det W
of the initial posterior: n = d^2).

    d    2 d^2   whole rounds   lanes in the last round
    5      50         0                 50
    6      72         1                  8
    7      98         1                 34
    9     162         2                 34
   10     200         3                  8
   11     242         3                 50
   12     288         4                 32
   13     338         5                 18
   14     392         6                  8
   15     450         7                  2

Every case prints its worst figures before it asserts.
"""
import functools

import numpy as np
import pytest

from cases import make_case
from test_em_trials_dev_gpu import _both, _compare
from test_vhem_em_trials_gpu import NV, assert_margin, compare, run_both, untouched

pytestmark = pytest.mark.gpu

MAX_ITER, MIN_DIFF = 3, 1e-6
# d -> (2 d^2, lanes that own an entry in the last round)
LAST_ROUND = {5: (50, 50), 6: (72, 8), 7: (98, 34), 9: (162, 34), 10: (200, 8), 11: (242, 50), 12: (288, 32),
              13: (338, 18), 14: (392, 8), 15: (450, 2)}
# (d, cov, seed): (N, K, S, Sb, T, R) = (40, 2, 3, 3, 6, 3), ragged
VBHEM_CASES = [(d, 1, 20 + d) for d in sorted(LAST_ROUND)] + [
    # diagonal covariances: no inverse on the host engine; the device loop eliminates the same
    # [Mt | I] (Mt carries the rank-one term mult1 dd'), 162 entries, and takes log det W from
    # the diagonal instead of the eliminated left half
    (9, 0, 29),
]
# (d, seed): full covariances, (N, K, S, Sb, tau, R) = (40, 2, 3, 3, 6, 3); 2 d^2 = 72, 162, 338, 450:
# 8, 34, 18 and 2 lanes own an entry in the last round
VHEM_CASES = [(6, 6), (9, 9), (13, 13), (15, 15)]


def test_last_round_table():
    for d, (n, lanes) in LAST_ROUND.items():
        assert n == 2 * d * d and lanes == (n % 64 or 64) and lanes < 64 and n <= 8 * 64


@pytest.mark.parametrize("d,cov,seed", VBHEM_CASES, ids=["d%d_%s" % (d, "full" if c else "diag")
                                                          for d, c, _ in VBHEM_CASES])
def test_vbhem_device_engine_matches_host_engine(vb, d, cov, seed):
    name = "dim%d%s" % (d, "" if cov else "diag")
    shape = (name, 40, 2, 3, 3, d, cov, 6, True, 3)
    _, _, _, host_tr, dev_tr = _both(vb, shape, MAX_ITER, MIN_DIFF, seed)
    # every trial runs to max_iter on the host engine, stable: every M-step's inverse is compared
    assert all(b.iters == MAX_ITER + 1 and b.stable for b in host_tr.results), \
        [(b.iters, b.stable) for b in host_tr.results]
    _compare(name, host_tr, dev_tr, MIN_DIFF)
    assert all(a.iters == MAX_ITER + 1 for a in dev_tr.results)


@functools.lru_cache(maxsize=None)
def vhem_build(d, seed):
    """test_vhem_em_trials_gpu.build_case's recipe: 'baseem' initialisations on Generators of
    their own; termvalue = 0.0, max_iter = 2 as in its case B (every trial runs 4 E-steps)."""
    from vbhem_amd import vhem
    N, K, S, Sb, tau, R = 40, 2, 3, 3, 6, 3
    cs = make_case(N, K, S, Sb, d, 1, seed=seed, ragged=True, tau=tau)
    iopt = vhem.default_hemopt(K, S, seed=1, initmode="baseem", tau=tau, covar_type="full")
    inits = []
    for r in range(R):
        rng = np.random.Generator(np.random.PCG64(7000 + 100 * seed + r))
        inits.append(vhem.initialize_hem_h3m_c(cs["bs"], iopt, rng))
    opt = dict(tau=tau, Nv=NV, inf_norm="nt", smooth=1.0, reg_cov=0.001, termvalue=0.0, max_iter=2,
               min_iter=1)
    return cs["base"], tuple(inits), opt


@pytest.mark.parametrize("d,seed", VHEM_CASES, ids=["d%d" % d for d, _ in VHEM_CASES])
def test_vhem_device_engine_matches_host_engine(vb, d, seed):
    base, inits, opt = vhem_build(d, seed)
    host, dev, rh, rd = run_both(vb, base, inits, opt)
    R = len(inits)
    assert_margin(host, opt["termvalue"])
    assert untouched(rh) == list(range(R)), "a degenerate fix ran in the host engine"
    assert all(d_["fallback_trials"] == [] for d_ in dev)
    assert untouched(rd) == list(range(R))
    compare("dim%d" % d, host, dev)
    assert all(len(h["LogLs"]) == opt["max_iter"] + 2 for h in host)
    assert all(len(d_["LogLs"]) == opt["max_iter"] + 2 for d_ in dev)
