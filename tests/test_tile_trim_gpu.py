"""The S = 8 backward kernel with a quad's work around its step loop trimmed (DESIGN.md 4.4c,
round 9: the tile loop over ping-pong input registers, K3's clamp only where it can act)
against the same library with the trim switched off (VBHEM_NO_BWD4_TRIM=1) and the oracle.

Every case runs one fused E-step twice and compares L_elbo, hat_Z, the packed statistics and
the fallback count bit for bit (the flag list itself is consumed inside the call: a pair
flagged by one kernel only would take its L_elbo from the exact recursion in one run and
from the fast one in the other, and move the count), then the default run against the
oracle at the suite's bars (RTOL_PAIRS for L_elbo, 1e-9 for the statistics, the north star
for hat_Z).

Shapes: SB in {8, 5, 1} (whole and zero-padded base blocks), K in {1, 3, 16}, N in {1, 5, 130}
(a lone pair, a partial last quad, several quads), and the two N at which a wave's tile
count goes just past two and just past three on this device (both parities of the unrolled
loop and its early exit), from the kernel's own launch plan; N = 130 again in three base
groups.  Whole tiles take their loads from uniform bases, the partial last one clamps.  The
must-flag cases take the clamped K3 (a range, row-sum or non-finite lane in the quad; a
cluster with lpi = -inf) or the version with the per-step underflow test (an A' entry below
2^-600).
"""
import ctypes

import numpy as np
import pytest
import torch

from cases import make_case
from conftest import RTOL_NORTH_STAR, RTOL_PAIRS, elem_err, hatz_err, stat_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, T, D = 8, 10, 2
STAT_KEYS = ("Nj", "N1", "M", "Nr", "Y", "SC")


def run(vb, base, consts, logOmega, tN, **switches):
    from vbhem_amd import _capi
    from vbhem_amd.estep import EStepEngine
    K = consts["logPi"].shape[0]
    with _capi.switches(**switches):
        eng = EStepEngine(vb.BaseSet.from_numpy(base), K, S, T, device=DEV)
        eng.set_clusters(consts)
        eng.set_log_omega(logOmega)
        stats = eng.fused(torch.as_tensor(tN, device=DEV)).cpu().numpy().copy()
        return dict(stats=stats, LL=eng.LL.cpu().numpy(), hatZ=eng.hatZ.cpu().numpy(),
                    flagged=eng.fallback_count(), kernel=_capi.last_kernel(0))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check(vb, vo, cs, base=None, consts=None, oracle=True, **switches):
    """Both runs, bit for bit; the default run against the oracle.  Returns the two runs."""
    base = cs["base"] if base is None else base
    consts = cs["consts"] if consts is None else consts
    N, K = base["prior"].shape[0], consts["logPi"].shape[0]
    tN = 100.0 * N * base["omega"]
    pairs = vo.c_estep_pairs(base, consts, T, nthreads=4)
    with np.errstate(all="ignore"):
        logOmega, hz, Z, Nj = vo.responsibilities(pairs["LL_elbo"], tN, cs["post"]["alpha"])
    new = run(vb, base, consts, logOmega, tN, **switches)
    old = run(vb, base, consts, logOmega, tN, NO_BWD4_TRIM=1, **switches)
    assert new["kernel"] == "vbhem::fb_bwd4_kernel<true>"
    assert old["kernel"] == "vbhem::fb_bwd4_kernel<true, false>"
    for k in ("LL", "hatZ", "stats"):
        assert same_bits(new[k], old[k]), k
    assert new["flagged"] == old["flagged"]
    if oracle:
        assert np.isfinite(pairs["LL_elbo"]).all()
        st = vo.c_statistics(Z, pairs, 1)
        got = vb.host.unpack_stats(new["stats"], K, S, D, 1)
        for k in STAT_KEYS:
            assert stat_err(got[k], st[k]) < 1e-9, k
        assert elem_err(new["LL"], pairs["LL_elbo"]) < RTOL_PAIRS
        assert hatz_err(new["hatZ"], hz) < RTOL_NORTH_STAR
    return new, old, Z


@pytest.mark.parametrize("N", [1, 5, 130])
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("SB", [8, 5, 1])
def test_small_shapes(vb, vo, SB, K, N):
    cs = make_case(N, K, S, SB, D, 1, seed=3 + SB + K, ragged=(SB == 5), tau=T)
    new, old, Z = check(vb, vo, cs)
    assert new["flagged"] == 0


def plan(capi_lib, K, N):
    out = (ctypes.c_int * 3)()
    capi_lib.vbhem_bwd4_launch_plan.restype = ctypes.c_int
    capi_lib.vbhem_bwd4_launch_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    assert capi_lib.vbhem_bwd4_launch_plan(K, N, out) == 0
    return tuple(out)


@pytest.mark.parametrize("sweeps", [2, 3])
def test_wave_tile_parities(vb, vo, capi_lib, sweeps):
    """N just past `sweeps` quads for every wave of a cluster: the first waves run sweeps + 1
    tiles, the others sweeps (an odd and an even count side by side, the early exit of the
    unrolled loop and its latch)."""
    K = 16
    quad, waves, blocks = plan(capi_lib, K, 1 << 20)        # the grid of a large call
    N = sweeps * blocks * waves * quad + 3                   # three bases of one more quad
    assert plan(capi_lib, K, N) == (quad, waves, blocks)     # the same grid at this N
    assert -(-(N // quad + 1) // (blocks * waves)) == sweeps + 1
    cs = make_case(N, K, S, 8, D, 1, seed=20 + sweeps, tau=T)
    new, old, Z = check(vb, vo, cs)
    assert new["flagged"] == 0


def test_base_groups(vb, vo):
    """Three base groups (VBHEM_GROUP_BASES): the passes of the later groups start at a base
    other than 0, whole tiles and a partial last one in each."""
    cs = make_case(130, 3, S, 8, D, 1, seed=31, tau=T)
    new, old, Z = check(vb, vo, cs, GROUP_BASES=50)
    assert new["flagged"] == 0


def test_launch_plan_of_a_small_call(capi_lib):
    quad, waves, blocks = plan(capi_lib, 3, 10)
    assert quad == 4 and waves >= 1 and blocks == 1         # 10 bases: one block's tiles


def _emission(base, consts):
    """E[i, j, sigma, beta] of the full-covariance emission term, numpy."""
    mu, Sg = base["centres"], base["covars"]
    m, P, c = consts["m"], consts["P"], consts["c"]
    d = mu.shape[-1]
    diff = mu[:, None, None, :, :] - m[None, :, :, None, :]
    quad = np.einsum("nksbx,ksxy,nksby->nksb", diff, P, diff)
    tr = np.einsum("ksxy,nbyx->nksb", P, Sg)
    return -0.5 * (d * np.log(2 * np.pi) + c[None, :, :, None] + tr + quad)


@pytest.mark.parametrize("case", ["rowsum", "vlim", "nan_mean", "inf_lpi", "tiny_A"])
def test_quads_that_keep_the_clamp(vb, vo, case):
    """One base or cluster that must leave the plain K3: a base row sum of 1 + 2e-6 (flagged:
    its K pairs and its gated ones again); one E column astride vlim = 7e5 / T - 3 (the pairs
    with an element at or past it flagged); one NaN base mean (not flagged: the kernels'
    L_elbo for it is compared between the two runs only, the oracle's is NaN); lpi = -inf
    for one cluster state (the clamp acts); an A' entry of e^-800 (the
    tile loop with the per-step underflow test)."""
    N, K = 41, 3
    cs = make_case(N, K, S, 8, D, 1, seed=9, tau=T)
    base = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in cs["base"].items()}
    consts = {k: np.array(v, copy=True) for k, v in cs["consts"].items()}
    i0, b0 = 17, 3
    vlim = 7.0e5 / T - 3.0
    if case == "rowsum":
        base["A"][i0, 2] *= (1.0 + 2e-6) / base["A"][i0, 2].sum()
    elif case == "vlim":
        E0 = _emission(base, consts)[i0, :, :, b0]
        # the column's |E| spreads with the states' precisions: slide it until the clusters
        # differ (one with an element past vlim, one without) and no element is so close
        # below vlim that Ef = E + amax rowsum(Ab) (|amax| <= log S = 2.08) or the rounding
        # of E decides
        cov0 = base["covars"][i0, b0].copy()
        trP = float(np.mean(np.trace(consts["P"], axis1=-2, axis2=-1)))
        for delta in np.arange(-4.0e4, 4.0e4, 2.5e3):
            lam = 2.0 * (vlim + delta + E0.mean()) / trP
            base["covars"][i0, b0] = cov0 + lam * np.eye(D)
            E1 = -_emission(base, consts)[i0, :, :, b0]
            near = (E1 > vlim - 2.2) & (E1 < vlim + 1e-3)
            past = (E1 >= vlim).any(axis=1)
            if past.any() and not past.all() and not near.any():
                break
        else:
            raise AssertionError("no placement of the column astride vlim")
    elif case == "nan_mean":
        base["centres"][i0, b0, 0] = np.nan
    elif case == "inf_lpi":
        consts["logPi"][1, 5] = -np.inf
    elif case == "tiny_A":
        consts["logA"][1, 2, 4] = -800.0
    new, old, Z = check(vb, vo, cs, base, consts, oracle=(case != "nan_mean"))
    gated = Z > 1e-8
    if case == "rowsum":
        assert new["flagged"] == K + int(gated[i0].sum())
    elif case == "vlim":
        assert new["flagged"] == int(past.sum()) + int((gated[i0] & past).sum()) > 0
