"""The E-step recursion kernels at the state counts no other test reaches: S = 7, 9, 10, 11,
13, 14 and 15 (cases.STATE_COUNT_SHAPES), against the oracle.

fb_split_kernel<S, LPC, MODE> and fb_bwd2_kernel<S> are instantiated for every S = 1..16;
cases.SHAPES and the other GPU tests stop at S in {1..6, 8, 12, 16}.  The S here are the ones
with an irregular lane mapping: padded rows (SH = ceil(S / LPC) does not divide S; at S = 9
the group's last lane owns padded rows only), the clamped branch of load_row, pairs of
S LPC = 14..60 lanes that straddle wavefronts with idle lanes at the block's end, and in
fb_bwd2_kernel a padded second column (S = 7) or 64 % S idle lanes per wave with pairs
across the 16-lane DPP rows (S >= 9).

Per shape:
* the per-pair outputs (vbhem_estep_pairs: fb_split_kernel's dense mode), sum_t_nu included;
* the fused call on the gated schedule (fb_bwd2_kernel, then fb_split_kernel's list mode)
  in three gate regimes -- tscale = 100 (Z nearly one-hot: short lists, some empty),
  1e-9 (no pair passes) and 0.3 (EVERY pair of every cluster passes: at N = 37 / 75 each
  cluster's list is more than two work items of the list kernel);
* the fused call on the dense schedule;
* the gated schedule under VBHEM_NO_BWD2 (fb_split_kernel's backward mode: LPC = 1 at
  S = 7, 2 from 9 -- odd S on two lanes).
Every run asserts the kernel instance that ran (vbhem_last_kernel) and a fallback count of
zero, after checking on the CPU that no normaliser can underflow: a fast path that broke
must not hide behind the exact fallback, nor a dispatch change behind the generic kernel.

Tolerances are those of test_gpu_parity: RTOL_PAIRS for per-pair outputs and L_elbo,
stat_err < 1e-9 for the statistics, test_fused_matches_oracle's Lt1 / Lt7 bounds and
RTOL_NORTH_STAR for hat_Z.  Each test prints its figures before it asserts (DESIGN.md
section 4.14b records them).
"""
import functools

import numpy as np
import pytest
import torch

from cases import SHAPES, STATE_COUNT_SHAPES, lib_switches, make_case  # noqa: F401  (lib_switches: a fixture)
from conftest import RTOL_NORTH_STAR, RTOL_PAIRS, elem_err, hatz_err, rel_err, stat_err
from test_gpu_parity import DEV, PAIR_KEYS, engine, seed_of

pytestmark = pytest.mark.gpu

NAMES = [s[0] for s in STATE_COUNT_SHAPES]
# fb_split_kernel's backward mode at the S of cases.SHAPES that neither a VHEM case nor another
# VBHEM_NO_BWD2 run puts it at: S = 6, 16 (test_backward_mode_at_old_state_counts; the S = 1
# shape of cases.SHAPES has Sb = 3 > S, which is fb_pairs_kernel's)
OLD_BACKWARD = [s for s in SHAPES if s[0] in ("d16diag", "S16")]
BY_NAME = {s[0]: s for s in STATE_COUNT_SHAPES + OLD_BACKWARD}
MISSING_S = {7, 9, 10, 11, 13, 14, 15}
assert {s[3] for s in STATE_COUNT_SHAPES} == MISSING_S and len(NAMES) == len(set(NAMES))
assert [s[3] for s in OLD_BACKWARD] == [16, 6]

GATE = 1e-8
STAT_KEYS = ("Nj", "N1", "M", "Nr", "Y", "SC")
# (id, schedule, tscale, VBHEM_NO_BWD2)
FUSED_MODES = [("gated-Nv100", "gated", 100.0, 0), ("gated-allgated", "gated", 1e-9, 0),
               ("gated-allpass", "gated", 0.3, 0), ("dense-Nv100", "dense", 100.0, 0),
               ("nobwd2-allpass", "gated", 0.3, 1)]
_checked = {m: set() for m in ["pairs"] + [m[0] for m in FUSED_MODES]}


def lpc_fwd(S):   # fb_split_kernel's lanes per column, dense / list mode (split_lpc)
    return 1 if S <= 4 else 2 if S <= 8 else 4


def lpc_bwd(S):   # ... and backward mode (split_lpc_bwd)
    return 1 if S <= 8 else 2


def no_underflow(consts):
    """The kernels' normaliser Z(sigma) = sum_s A'(sigma, s) G(s) has A' = exp(logA - rowmax)
    and G = exp(V - max V), so one G is 1 and Z >= min A'.  The exact fallback takes a pair
    when some Z < 1e-200 (kZMinS; fb_bwd2_kernel: 2^-665): with min A' >= e^-400 none can."""
    la = consts["logA"]
    return float((la - la.max(-1, keepdims=True)).min()) > -400.0 and all(
        np.isfinite(consts[k]).all() for k in ("logA", "logPi", "m", "P", "c"))


@functools.lru_cache(maxsize=None)
def pairs_case(name):
    """(case, the oracle's per-pair outputs) -- computed once, never modified."""
    _, N, K, S, Sb, d, cov, T, ragged = BY_NAME[name]
    cs = make_case(N, K, S, Sb, d, cov, seed=seed_of(name), ragged=ragged, tau=T)
    import vbhem_oracle as vo
    return cs, vo.c_estep_pairs(cs["base"], cs["consts"], T, nthreads=4, want_tnu=True)


@functools.lru_cache(maxsize=None)
def fused_case(name):
    """(case, the oracle's per-pair outputs) of the fused tests (test_gpu_parity's seed + 1)."""
    _, N, K, S, Sb, d, cov, T, ragged = BY_NAME[name]
    cs = make_case(N, K, S, Sb, d, cov, seed=seed_of(name) + 1, ragged=ragged, tau=T)
    import vbhem_oracle as vo
    return cs, vo.c_estep_pairs(cs["base"], cs["consts"], T, nthreads=4)


@functools.lru_cache(maxsize=None)
def fused_reference(name, tscale):
    """The oracle's responsibilities and statistics at tilde N = tscale N omega."""
    import vbhem_oracle as vo
    _, N, K, S, Sb, d, cov, T, ragged = BY_NAME[name]
    cs, pairs = fused_case(name)
    tN = tscale * N * cs["base"]["omega"]
    logOmega, hz, Z, Nj = vo.responsibilities(pairs["LL_elbo"], tN, cs["post"]["alpha"])
    return tN, logOmega, hz, Z, vo.c_statistics(Z, pairs, cov)


@pytest.mark.parametrize("name", NAMES)
def test_pairs_match_oracle(vb, vo, name):
    from vbhem_amd import _capi
    _, N, K, S, Sb, d, cov, T, ragged = BY_NAME[name]
    cs, ref = pairs_case(name)
    assert no_underflow(cs["consts"]) and all(np.isfinite(v).all() for v in ref.values())
    eng = engine(vb, cs["base"], cs["consts"], T)
    got = eng.pairs(want_tnu=True)
    torch.cuda.synchronize()
    kernel, nfb = _capi.last_kernel(0), eng.fallback_count()
    figs = {}
    for k in PAIR_KEYS + ("sum_t_nu",):
        g = got[k].cpu().numpy()
        figs[k] = (rel_err(g, ref[k]), stat_err(g, ref[k]))
    print("FIGS", name, "pairs", kernel, "fallback", nfb,
          {k: "%.2e/%.2e" % v for k, v in figs.items()})
    assert kernel == "vbhem::fb_split_kernel<%d, %d, 0>" % (S, lpc_fwd(S)), kernel
    assert nfb == 0
    for k, (e_norm, e_elem) in figs.items():
        assert e_norm < RTOL_PAIRS, (name, k, e_norm)
        assert e_elem < 1e-8, (name, k, e_elem)
    _checked["pairs"].add(name)


def check_fused(vb, lib_switches, name, mode):
    """One fused call of shape `name` in `mode` (a FUSED_MODES row) against the oracle."""
    from vbhem_amd import _capi
    mode_id, schedule, tscale, no_bwd2 = mode
    _, N, K, S, Sb, d, cov, T, ragged = BY_NAME[name]
    cs, pairs = fused_case(name)
    tN, logOmega, hz, Z, st = fused_reference(name, tscale)
    assert no_underflow(cs["consts"]) and np.isfinite(pairs["LL_elbo"]).all()
    # the gate regime, on the oracle alone (conditions on the inputs, not tolerances)
    gated_pairs = (Z > GATE).sum(0)
    if tscale == 0.3:      # every pair of every cluster is gated ...
        assert (hz >= GATE).all() and (gated_pairs == N).all(), gated_pairs
        if N >= 37:        # ... and a cluster's list is more than two work items of the
            assert N > 2 * (512 // (S * lpc_fwd(S)))   # list kernel (<= 512 threads a block)
    elif tscale == 1e-9:   # no pair is
        assert (gated_pairs == 0).all(), gated_pairs
    lib_switches(FUSED_DENSE=int(schedule == "dense"), NO_BWD2=no_bwd2)
    eng = engine(vb, cs["base"], cs["consts"], T)
    eng.set_log_omega(logOmega)
    vec = eng.fused(torch.as_tensor(tN, device=DEV)).cpu().numpy()
    kernels, nfb = (_capi.last_kernel(0), _capi.last_kernel(1)), eng.fallback_count()
    got = vb.host.unpack_stats(vec, K, S, d, cov)
    figs = {k: stat_err(got[k], st[k]) for k in STAT_KEYS}
    Lt1 = float((Z * pairs["LL_elbo"]).sum())
    Lt7 = float((hz * np.log(hz)).sum())
    figs["Lt1"] = abs(got["Lt1"] - Lt1) / abs(Lt1)
    figs["Lt7"] = abs(got["Lt7"] - Lt7) / (1e-9 * abs(Lt7) + 1e-9)   # in units of its bound
    figs["hatZ"] = hatz_err(eng.hatZ.cpu().numpy(), hz)
    figs["LL"] = elem_err(eng.LL.cpu().numpy(), pairs["LL_elbo"])
    print("FIGS", name, mode_id, kernels, "fallback", nfb, "gated", gated_pairs.tolist(),
          {k: "%.2e" % v for k, v in figs.items()})
    # the instance that ran: never the generic kernel, never another S
    if schedule == "gated":
        want0 = ("vbhem::fb_split_kernel<%d, %d, 1>" % (S, lpc_bwd(S)) if no_bwd2 else
                 "vbhem::fb_bwd2_kernel<%d>" % S)
        assert kernels == (want0, "vbhem::fb_split_kernel<%d, %d, 2>" % (S, lpc_fwd(S))), kernels
    else:
        assert kernels[0] == "vbhem::fb_split_kernel<%d, %d, 0>" % (S, lpc_fwd(S)), kernels
    assert nfb == 0
    assert np.isfinite(vec).all()
    for k in STAT_KEYS:
        assert figs[k] < 1e-9, (name, k, figs[k])
    assert abs(got["Lt1"] - Lt1) <= 1e-10 * abs(Lt1)
    assert abs(got["Lt7"] - Lt7) <= 1e-9 * abs(Lt7) + 1e-9
    assert figs["hatZ"] < RTOL_NORTH_STAR
    assert figs["LL"] < RTOL_PAIRS


@pytest.mark.parametrize("mode", FUSED_MODES, ids=[m[0] for m in FUSED_MODES])
@pytest.mark.parametrize("name", NAMES)
def test_fused_matches_oracle(vb, vo, lib_switches, name, mode):
    check_fused(vb, lib_switches, name, mode)
    _checked[mode[0]].add(name)


@pytest.mark.parametrize("name", [s[0] for s in OLD_BACKWARD])
def test_backward_mode_at_old_state_counts(vb, vo, lib_switches, name):
    """fb_split_kernel<S, LPC, 1> at S = 6 (one lane per column) and 16 (two): the gated
    schedule under VBHEM_NO_BWD2 on shapes of cases.SHAPES, tscale = 100."""
    check_fused(vb, lib_switches, name, ("nobwd2-Nv100", "gated", 100.0, 1))


def test_no_shape_was_left_out():
    """Runs last: every shape went through every mode above and passed it."""
    for mode, names in _checked.items():
        assert len(names) == len(STATE_COUNT_SHAPES) and names == set(NAMES), (mode, sorted(set(NAMES) - names))
    assert {BY_NAME[n][3] for n in _checked["pairs"]} == MISSING_S
