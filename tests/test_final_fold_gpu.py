"""The folded finish of the fused E-step (S = 8, SB <= 8, T = 10, one base group): when
fb_list4_kernel accumulated the gated sums, stats_final_fold_kernel sums its partials per
(cluster, state) in list4_stats_reduce_kernel's order, shifts them back and stores the packed
statistics, and sums the responsibility kernels' columns over the chunks as stats_final_kernel
does -- one launch instead of two.  VBHEM_NO_FINAL_FOLD=1 restores the two launches.

Every case requires the packed statistics of the two paths to be the same bits
(np.array_equal on the raw vectors; the fold changes no summation order and applies the one
`0.0 +` the second kernel applied), holds the folded result to the oracle at the suite's
stat_err < 1e-9, and checks through vbhem_last_kernel(3) that each path is the one that ran.
The references are tests/test_list4_stats.py's (computed once per case, shared with it).
"""
import numpy as np
import pytest
import torch

from cases import make_case
from conftest import stat_err
from test_list4_stats import DEV, KEYS, S, T, reference

pytestmark = pytest.mark.gpu

FOLD, TWO = "vbhem::stats_final_fold_kernel", "vbhem::stats_final_kernel"
ACC = "vbhem::list4_stats_reduce_kernel"


def run(vb, base, consts, tN, logOmega, calls=1, armed=False, **sw):
    """The packed statistics (raw vector) of the last of `calls` fused calls on a fresh engine
    under the switches sw, the finishing kernel, the statistics family, the fallback count."""
    from vbhem_amd import _capi
    from vbhem_amd.estep import EStepEngine
    K = consts["logPi"].shape[0]
    with _capi.switches(FUSED_DENSE=0, **sw):
        eng = EStepEngine(vb.BaseSet.from_numpy(base), K, S, T, device=DEV)
        eng.set_clusters(consts)
        eng.set_log_omega(logOmega)
        tN_dev = torch.as_tensor(tN, device=DEV)
        for _ in range(calls):
            vec = eng.fused(tN_dev).cpu().numpy().copy()
        names = (_capi.last_kernel(3), _capi.last_kernel(2))
        nfb = eng.fallback_count()
        host = None
        if armed:   # the same call with the completion word, into pinned host memory
            w, hs = eng.done_word(), eng.host_stats_buffer()
            for k in (1, 2):
                eng.fused(tN_dev, out=hs, done=(w, k))
                w.wait(k, timeout_s=30)
                assert w.value == k
                host = hs.numpy().copy()
                assert np.array_equal(host, vec), k
            torch.cuda.synchronize()
            assert eng.fallback_count() == nfb          # the flag head's counters are clean
            assert _capi.last_kernel(3) == names[0]
    return vec, names, nfb, host


def check(vb, base, consts, tN, logOmega, ref, cov, expect_fold=True, armed=False, **sw):
    d = base["centres"].shape[2]
    K = consts["logPi"].shape[0]
    new, names, nfb, _ = run(vb, base, consts, tN, logOmega, armed=armed, **sw)
    again, _, _, _ = run(vb, base, consts, tN, logOmega, calls=2, **sw)
    old, names_old, nfb_old, _ = run(vb, base, consts, tN, logOmega, armed=armed, NO_FINAL_FOLD=1, **sw)
    print("finish", names, "/", names_old, "fallback", nfb, "differing entries", int((new != old).sum()),
          "of", new.size)
    assert names == ((FOLD if expect_fold else TWO), ACC), names
    assert names_old == (TWO, ACC), names_old
    got = vb.host.unpack_stats(new, K, S, d, cov)
    for k in KEYS:
        e = stat_err(got[k], ref[k])
        print(k, "vs oracle %.3g" % e)
        assert e < 1e-9, (k, e)
    assert np.array_equal(new, old)        # bit for bit (no NaN: held to the oracle above)
    assert np.array_equal(new, again)      # and from call to call
    assert nfb == nfb_old
    return got, nfb


def check_key(vo, vb, key, tscale=100.0, **kw):
    base, consts, tN, logOmega, Z, ref = reference(vo, key, tscale)
    got, nfb = check(vb, base, consts, tN, logOmega, ref, key[5], **kw)
    return got, nfb, Z


@pytest.mark.parametrize("d,cov", [(2, 1), (8, 1), (11, 0)], ids=["d2_nup16", "d8_nup48", "d11_nup32"])
def test_feature_tiles(vb, vo, d, cov):
    """NU = 6, 45, 23 moments per state: one, three and two feature tiles of 16 in a partial;
    a row of a block is NU + 1 + S = 15, 54, 32 columns of its 64."""
    check_key(vo, vb, ("plain", 41, 3, 8, d, cov, False))


def test_ragged_base_states(vb, vo):
    """SB = 5 with ragged nstates (padded base states in the accumulating pass)."""
    check_key(vo, vb, ("plain", 41, 3, 5, 3, 1, True))


def test_more_waves_than_items(vb, vo):
    """N = 5: at most two quads per cluster on a grid of thousands of waves -- a cluster's
    partials are one or two slots, 14 or 15 of a block's 16 thread groups sum nothing."""
    got, nfb, Z = check_key(vo, vb, ("plain", 5, 3, 8, 3, 1, False))
    assert 0 < (Z > 1e-8).sum() <= 15


def test_one_empty_list(vb, vo):
    """Cluster 0 loses every base: its slot count is 0, its sections are written as zeros
    (+0.0 in both paths) while the other clusters' are not."""
    cs = make_case(41, 3, S, 8, 3, 1, seed=5, tau=T)
    consts = {k: np.array(v, copy=True) for k, v in cs["consts"].items()}
    consts["c"][0] += 1.0e4
    pairs = vo.c_estep_pairs(cs["base"], consts, T, nthreads=4)
    tN = 100.0 * 41 * cs["base"]["omega"]
    logOmega, hz, Z, Nj = vo.responsibilities(pairs["LL_elbo"], tN, cs["post"]["alpha"])
    assert not (Z[:, 0] > 1e-8).any() and (Z[:, 1:] > 1e-8).any()
    got, _ = check(vb, cs["base"], consts, tN, logOmega, vo.c_statistics(Z, pairs, 1), 1)
    assert not np.any(got["N1"][0]) and not np.any(got["Y"][0]) and np.any(got["N1"][1:])


def test_every_list_empty(vb, vo):
    """tscale = 1e-9: no pair gated, every N1 | M | U entry a zero."""
    got, _, Z = check_key(vo, vb, ("plain", 41, 3, 8, 3, 1, False), tscale=1e-9)
    assert not (Z > 1e-8).any()
    for k in ("N1", "M", "Nr", "Y", "SC"):
        assert not np.any(got[k]), k


def test_flagged_pairs_and_completion_word(vb, vo):
    """test_exact_fallback_mfma_kernels' adversarial input: cluster 0 wins and flags every base
    in both passes, the accumulating pass recomputes them inline.  Run with the completion
    word as well: the ticket arrives after the statistics (host memory equals the unarmed
    call's bits when the word is seen, twice), and the counter the finishing kernel borrows
    for its blocks is left clean (the fallback count repeats)."""
    got, nfb, Z = check_key(vo, vb, ("adv", 41, 2, 8, 3, 1, False), armed=True)
    assert nfb >= 2 * 41 and (Z[:, 0] > 1e-8).all()


def test_two_base_groups_step_aside(vb, vo):
    """VBHEM_GROUP_BASES = 21: two groups, the second adds into slab 0 -- the fold does not
    apply, both runs take the two launches and the result is what it was."""
    check_key(vo, vb, ("plain", 41, 3, 8, 3, 1, False), expect_fold=False, GROUP_BASES=21)


def test_several_chunks(vb, vo):
    """N = 5,000, K = 2: 79 chunks of responsibility partials for the Nj / Lt columns (more
    than the 16 partitions, the four-fold unrolled sum) and hundreds of slots per cluster."""
    check_key(vo, vb, ("plain", 5000, 2, 8, 3, 1, False), tscale=1e-3)
