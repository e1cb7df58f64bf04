"""The gated statistics accumulated inside fb_list4_kernel (S = 8, SB <= 8, T = 10).

Default path: the gate-list pass keeps Z nu_1, Z (A' o H) and (Z sum_t_nu) Us of each
wave's items in LDS, flushes one partial per (wave, cluster run) and
list4_stats_reduce_kernel sums the partials; VBHEM_NO_LIST4_STATS=1 restores the
per-pair stores and stats_list_m_kernel.  Every case compares the fused call's
unpacked statistics under the new path with the oracle's (stat_err < 1e-9, the suite's
bound) and with the old path's (stat_err < 1e-10, the bound of two summation orders of
the same terms, as test_c4_gated_matches_dense), and checks that each path is the one
that ran (last_kernel(2)).

The CPU test checks the slot plan both kernels and the host share
(vbhem_list4_slots.h) through the library's vbhem_list4_stats_slot_plan.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cases import lib_switches, make_case  # noqa: F401  (lib_switches: a fixture)
from conftest import stat_err

DEV = "cuda:0"
KEYS = ("Nj", "N1", "M", "Nr", "Y", "SC")
NEW, OLD = "vbhem::list4_stats_reduce_kernel", "vbhem::stats_list_kernels"
S, T = 8, 10


def adversarial(vb, N, K, d=3):
    """tests.test_gpu_parity.adversarial_case at S = Sb = 8, T = 10: cluster 0's pairs
    underflow the factorised normaliser, the other clusters lose every base."""
    cs = make_case(N, K, S, S, d, 1, seed=99, tau=T)
    c = {k: np.array(v, copy=True) for k, v in cs["consts"].items()}
    lA = np.full((S, S), -600.0)
    for r in range(S):
        lA[r, (r + 1) % S] = 0.0
    c["logA"][0] = lA
    c["c"][0] = 1200.0
    c["c"][0, 0] = 0.0
    c["c"][1:] = 1.0e4
    return cs, c


@functools.lru_cache(maxsize=None)
def oracle(key):
    """(base, consts, alpha, LL pairs) of a named case, computed once."""
    import pkgload
    import vbhem_oracle as vo
    vb = pkgload.load()
    kind, N, K, Sb, d, cov, ragged = key
    if kind == "adv":
        cs, consts = adversarial(vb, N, K, d)
    else:
        cs = make_case(N, K, S, Sb, d, cov, seed=31 + N + d, ragged=ragged, tau=T)
        consts = {k: np.array(v, copy=True) for k, v in cs["consts"].items()}
    base = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in cs["base"].items()}
    if kind == "rowsum":
        base["A"][N // 2, 2] *= 1.5 / base["A"][N // 2, 2].sum()
    pairs = vo.c_estep_pairs(base, consts, T, nthreads=4)
    return base, consts, cs["post"]["alpha"], pairs


def reference(vo, key, tscale):
    base, consts, alpha, pairs = oracle(key)
    N, cov = key[1], key[5]
    tN = tscale * N * base["omega"]
    logOmega, hz, Z, Nj = vo.responsibilities(pairs["LL_elbo"], tN, alpha)
    return base, consts, tN, logOmega, Z, vo.c_statistics(Z, pairs, cov)


def fused(vb, base, consts, tN, logOmega, cov, calls=1):
    """The unpacked statistics, the raw vector, the fallback count and the statistics
    kernel family of a fused call on a fresh engine (the last of `calls` calls)."""
    from vbhem_amd import _capi
    from vbhem_amd.estep import EStepEngine
    K, d = consts["logPi"].shape[0], base["centres"].shape[2]
    eng = EStepEngine(vb.BaseSet.from_numpy(base), K, S, T, device=DEV)
    eng.set_clusters(consts)
    eng.set_log_omega(logOmega)
    for _ in range(calls):
        vec = eng.fused(torch.as_tensor(tN, device=DEV)).cpu().numpy().copy()
    return vb.host.unpack_stats(vec, K, S, d, cov), vec, eng.fallback_count(), _capi.last_kernel(2)


def check(vb, vo, lib_switches, key, tscale=100.0, expect_flags=None, **switches):
    base, consts, tN, logOmega, Z, ref = reference(vo, key, tscale)
    cov = key[5]
    if switches:
        lib_switches(**switches)
    new, vec, nfb, kern = fused(vb, base, consts, tN, logOmega, cov)
    assert kern == NEW, kern
    from vbhem_amd import _capi
    with _capi.switches(NO_LIST4_STATS=1):  # (inside the test's own switches)
        old, _, nfb_old, kern_old = fused(vb, base, consts, tN, logOmega, cov)
    assert kern_old == OLD, kern_old
    for k in KEYS:
        e_ref, e_old = stat_err(new[k], ref[k]), stat_err(new[k], old[k])
        print(key, k, "vs oracle %.3g  vs old path %.3g" % (e_ref, e_old))
        assert e_ref < 1e-9, (k, e_ref)
        assert e_old < 1e-10, (k, e_old)
    assert nfb == nfb_old
    if expect_flags is not None:
        assert expect_flags(nfb, Z), nfb
    return new, vec, Z


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 7, 41])
def test_partial_quads(vb, vo, lib_switches, N):
    """Gate lists of every length mod 4 (inactive pair slots; the lengths are asserted),
    and, at N = 41, fewer items than waves: each wave takes at most one."""
    key = ("plain", N, 3, 8, 3, 1, False)
    _, _, Z = check(vb, vo, lib_switches, key)
    lens = (Z > 1e-8).sum(axis=0)
    assert lens.sum() >= N
    if N == 41:
        assert set(int(x) % 4 for x in lens) - {0}, lens
    # a softer weight: every cluster's list is the whole base set (N mod 4 = 1, 3, 1)
    _, _, Z = check(vb, vo, lib_switches, key, tscale=1e-3)
    assert ((Z > 1e-8).sum(axis=0) == N).all()


@pytest.mark.gpu
def test_empty_lists(vb, vo, lib_switches):
    """tscale = 1e-9: no pair passes the gate, every section is written as zeros (twice:
    stale partials of the first call change nothing); and a case in which one cluster's
    list is empty while the others' are not."""
    key = ("plain", 41, 3, 8, 3, 1, False)
    base, consts, tN, logOmega, Z, ref = reference(vo, key, 1e-9)
    assert not (Z > 1e-8).any()
    _, _, Zs = check(vb, vo, lib_switches, key)  # leaves non-zero partials behind
    new, _, _ = check(vb, vo, lib_switches, key, tscale=1e-9)
    for k in ("N1", "M", "Nr", "Y", "SC"):
        assert not np.any(new[k]), k
    cs = make_case(41, 3, S, 8, 3, 1, seed=5, tau=T)
    consts = {k: np.array(v, copy=True) for k, v in cs["consts"].items()}
    consts["c"][0] += 1.0e4         # cluster 0 loses every base
    pairs = vo.c_estep_pairs(cs["base"], consts, T, nthreads=4)
    tN = 100.0 * 41 * cs["base"]["omega"]
    logOmega, hz, Z, Nj = vo.responsibilities(pairs["LL_elbo"], tN, cs["post"]["alpha"])
    assert not (Z[:, 0] > 1e-8).any() and (Z[:, 1:] > 1e-8).any()
    st = vo.c_statistics(Z, pairs, 1)
    got, _, _, kern = fused(vb, cs["base"], consts, tN, logOmega, 1)
    assert kern == NEW
    for k in KEYS:
        assert stat_err(got[k], st[k]) < 1e-9, k
    assert not np.any(got["N1"][0]) and not np.any(got["Y"][0])


@pytest.mark.gpu
def test_more_items_than_waves(vb, vo, lib_switches):
    """K = 2, N = 5000 at a weight scale at which both clusters gate most bases: more
    items than the grid has waves (asserted on the oracle's Z), so waves hold several
    items and the cluster boundary falls inside a wave's range."""
    key = ("plain", 5000, 2, 8, 3, 1, False)
    nw = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4
    tscale = None
    for ts in (10.0, 8.0, 12.0):  # chosen on the CPU, from the oracle's Z (2048 waves)
        Z = reference(vo, key, ts)[4]
        items = [(int(n) + 3) // 4 for n in (Z > 1e-8).sum(axis=0)]
        if sum(items) > nw and items[0] % -(-sum(items) // nw) != 0:
            tscale = ts
            break
    if tscale is None:
        pytest.skip("no weight scale gives more items than the grid's %d waves" % nw)
    _, _, Z = check(vb, vo, lib_switches, key, tscale=tscale)
    items = [(int(n) + 3) // 4 for n in (Z > 1e-8).sum(axis=0)]
    assert sum(items) > nw and min(items) > 0
    per = -(-sum(items) // nw)
    assert items[0] % per != 0  # the boundary is inside a wave's range


@pytest.mark.gpu
@pytest.mark.parametrize("d,cov", [(3, 1), (8, 1), (8, 0)], ids=["nup16", "nup48", "nup32"])
def test_tile_counts(vb, vo, lib_switches, d, cov):
    """NUP / 16 = 1, 3, 2 feature tiles."""
    check(vb, vo, lib_switches, ("plain", 41, 3, 8, d, cov, False))


@pytest.mark.gpu
def test_ragged_base_states(vb, vo, lib_switches):
    """SB = 5 with ragged nstates: the non-FAST instantiation (padded base states)."""
    check(vb, vo, lib_switches, ("plain", 41, 3, 5, 3, 1, True))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [41, 5000])
def test_flagged_pairs_adversarial(vb, vo, lib_switches, N):
    """The adversarial cluster wins and flags every base in both passes: its pairs are
    counted once, from their exact values (the sums match the oracle), and the fallback
    count equals the old path's."""
    check(vb, vo, lib_switches, ("adv", N, 2, 8, 3, 1, False),
          expect_flags=lambda nfb, Z: nfb >= 2 * N and (Z[:, 0] > 1e-8).all())


@pytest.mark.gpu
def test_flagged_pairs_rowsum(vb, vo, lib_switches):
    """One base row of A sums to 1.5: that base's pairs are flagged in both passes, exactly."""
    key = ("rowsum", 41, 3, 8, 3, 1, False)
    check(vb, vo, lib_switches, key,
          expect_flags=lambda nfb, Z: nfb == 3 + int((Z[41 // 2] > 1e-8).sum()))


@pytest.mark.gpu
def test_base_groups(vb, vo, lib_switches):
    """Several base groups (VBHEM_GROUP_BASES): the first group writes the sections, later
    groups add; with flagged pairs as well."""
    check(vb, vo, lib_switches, ("plain", 41, 3, 8, 3, 1, False), GROUP_BASES=16, NSLAB=5)
    check(vb, vo, lib_switches, ("adv", 41, 2, 8, 3, 1, False), GROUP_BASES=16,
          expect_flags=lambda nfb, Z: nfb >= 2 * 41)


@pytest.mark.gpu
def test_deterministic(vb, vo, lib_switches):
    """Two calls bit-equal, and equal after an intervening call of another shape."""
    key = ("plain", 5000, 2, 8, 3, 1, False)
    base, consts, tN, logOmega, Z, ref = reference(vo, key, 1e-3)
    _, v1, _, kern = fused(vb, base, consts, tN, logOmega, 1)
    assert kern == NEW
    _, v2, _, _ = fused(vb, base, consts, tN, logOmega, 1, calls=2)
    assert np.array_equal(v1, v2)
    b2, c2, tN2, lO2, _, _ = reference(vo, ("adv", 41, 2, 8, 3, 1, False), 100.0)
    fused(vb, b2, c2, tN2, lO2, 1)
    _, v3, _, _ = fused(vb, base, consts, tN, logOmega, 1)
    assert np.array_equal(v1, v3)


# ---- CPU: the slot plan ----
def slot_plan(lib, tot, nw):
    K = len(tot)
    arr = (ctypes.c_int * K)(*tot)
    per = ctypes.c_int(0)
    first, count = (ctypes.c_int * K)(), (ctypes.c_int * K)()
    fn = lib.vbhem_list4_stats_slot_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    nitem = fn(arr, K, nw, ctypes.byref(per), first, count)
    return nitem, per.value, list(first), list(count)


def test_slot_plan(capi_lib):
    """Slots are unique, ordered by item, dense per cluster and at most nw + K, for empty,
    one-entry and uneven lists and K up to kList4MaxK (1024)."""
    rng = np.random.default_rng(5)
    cases = [([0], 8), ([1], 8), ([0, 0, 0], 4), ([1, 0, 1], 4), ([5, 7, 41], 8), ([5, 7, 41], 2048),
             ([4096, 1, 0, 4095, 2], 16), ([100000] * 16, 2048), ([3, 0, 0, 9, 0], 1)]
    cases.append((list(rng.integers(0, 50, 1024)), 2048))
    cases.append((list(rng.integers(0, 3, 1024)), 64))
    cases.append((list(rng.integers(0, 5000, 37)), 2048))
    for tot, nw in cases:
        tot = [int(t) for t in tot]
        K = len(tot)
        nitem, per, first, count = slot_plan(capi_lib, tot, nw)
        items = [(t + 3) // 4 for t in tot]
        assert nitem == sum(items) and per >= 1 and per * nw >= nitem
        # the plan, item by item: wave = item // per, slot = wave + cluster
        seen, last, it = set(), -1, 0
        for j in range(K):
            slots = []
            for _ in range(items[j]):
                s = it // per + j
                if not slots or slots[-1] != s:
                    slots.append(s)
                it += 1
            if not slots:
                assert count[j] == 0
                continue
            assert slots == list(range(first[j], first[j] + count[j])), (tot[:8], nw, j)  # dense
            assert slots[0] > last and not (seen & set(slots))                        # ordered, unique
            seen |= set(slots)
            last = slots[-1]
        assert len(seen) <= nw + K and (not seen or max(seen) < nw + K)
        assert all(it_ // per < nw for it_ in range(0, nitem, max(1, per)))          # every wave exists
