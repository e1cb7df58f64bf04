"""The device-side VHEM EM of R batched trials (vhem_em_run_trials: csrc/vhem_em.hip,
csrc/vhem_em_trials.hip; vhem.hem_h3m_c_trials(..., em_engine="device")) against the host
engine (vhem.hem_h3m_c_trials as it stands) on the same initial mixtures and Generators.

The two engines run the same E-step kernels; the stopping rule is one shared function,
the M-step and the E-step constants are numpy on one side and the device's fp64 on the
other (Gauss-Jordan without pivoting against LAPACK's LU, the device's log against
libm's), so a trial's log-likelihoods differ in the last digits.  The bars are those of
tests/test_em_trials_dev_gpu.py: equal num_iter per trial, the same best trial and the
same labels, LogLs at rtol 1e-10, every parameter within 1e-9 normwise, Z within 1e-8.

A stopping decision can only differ when a tested change lies at termvalue itself, and a
fix changes what a trial computes: every case asserts, on the host engine's own
trajectory, that no tested change lies within 5 % of termvalue and -- unless the case is
about the fallback -- that no degenerate fix ran (a fix draws from the trial's Generator;
its state after the run is compared with an untouched twin).  The seeds are fixed so.

Every case prints its worst figures before it asserts; the table is in DESIGN.md 4.21.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vhem_ref as ref
from cases import make_case, make_reduced
from conftest import hatz_err, rel_err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NV = 100
PARAMS = ("omega", "prior", "A", "centres", "covars", "emit_vcounts")

# name: (N, K, S, Sb, d, cov, ragged, tau, R, max_iter, termvalue, min_iter, seed, first)
CASES = {
    # the em_case shape of tests/test_vhem_gpu.py with four starts: trials stop at
    # different iterations
    "A": (40, 3, 3, 3, 2, 1, True, 6, 4, 100, 1e-5, 1, 17, 1),
    # every trial runs max_iter + 2 E-steps
    "B": (40, 3, 4, 4, 3, 0, True, 7, 4, 3, 0.0, 1, 12, 0),
    # the 1e-12 substitutions: S == 1, and tau == 1
    "C_S1": (30, 1, 1, 1, 2, 1, False, 5, 3, 100, 1e-5, 1, 2, 0),
    "C_tau1": (30, 2, 3, 3, 2, 1, False, 1, 3, 100, 1e-5, 1, 4, 0),
    # the S = 8 matrix-core E-step path and the 8 x 8 inverse
    "D": (200, 16, 8, 8, 8, 1, False, 10, 4, 3, 1e-5, 1, 6, 0),
    # the largest inverse and the Sb < S padding
    "E": (50, 2, 16, 12, 16, 1, False, 6, 3, 2, 1e-5, 1, 1, 0),
    # R K = 256; and K S = 9: blocks of 4 waves straddle the trials
    "F": (100, 4, 2, 2, 2, 1, False, 6, 64, 6, 1e-5, 1, 3, 0),
    "F_KS9": (100, 3, 3, 3, 2, 1, False, 6, 5, 6, 1e-5, 1, 1, 0),
    # A with min_iter 8
    "H": (40, 3, 3, 3, 2, 1, True, 6, 4, 100, 1e-5, 8, 17, 1),
}


@functools.lru_cache(maxsize=None)
def build_case(name):
    """(base dict, the R initial mixtures, hemopt fields) -- built once, never modified.
    The initial mixtures are 'baseem' initialisations (initialize_hem_h3m_c.m:111-139) on
    Generators of their own, numbers `first` .. `first` + R - 1 of the case's seed."""
    from vbhem_amd import vhem
    N, K, S, Sb, d, cov, ragged, tau, R, max_iter, term, min_iter, seed, first = CASES[name]
    cs = make_case(N, K, S, Sb, d, cov, seed=seed, ragged=ragged, tau=tau)
    iopt = vhem.default_hemopt(K, S, seed=1, initmode="baseem", tau=tau,
                               covar_type="full" if cov == 1 else "diag")
    inits = []
    for r in range(first, first + R):
        rng = np.random.Generator(np.random.PCG64(7000 + 100 * seed + r))
        inits.append(vhem.initialize_hem_h3m_c(cs["bs"], iopt, rng))
    opt = dict(tau=tau, Nv=NV, inf_norm="nt", smooth=1.0, reg_cov=0.001, termvalue=term,
               max_iter=max_iter, min_iter=min_iter)
    return cs["base"], tuple(inits), opt


def case_G():
    """A with trial 1's initial omega[0] = 0 and trial 2's cluster 0 without state 2."""
    base, inits, opt = build_case("A")
    inits = [{k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in h.items()} for h in inits]
    inits[1]["omega"] = np.array([0.0, 0.5, 0.5])
    inits[2]["prior"][0, 2] = 0.0
    inits[2]["prior"][0] /= inits[2]["prior"][0].sum()
    inits[2]["A"][0, :, 2] = 0.0
    inits[2]["A"][0] /= inits[2]["A"][0].sum(1, keepdims=True)
    return base, tuple(inits), opt


def rngs_for(R, seed=900):
    return [np.random.Generator(np.random.PCG64(seed + r)) for r in range(R)]


def engine(vb, base, inits, tau):
    from vbhem_amd.estep import EStepEngine
    K, S = inits[0]["prior"].shape
    return EStepEngine(vb.BaseSet.from_numpy(base), len(inits) * K, S, tau, device=DEV,
                       trials=len(inits))


def run_both(vb, base, inits, opt):
    """(host results, device results, host Generators, device Generators)."""
    from vbhem_amd import vhem
    R = len(inits)
    rh, rd = rngs_for(R), rngs_for(R)
    host = vhem.hem_h3m_c_trials(list(inits), engine(vb, base, inits, opt["tau"]), opt, rh)
    dev = vhem.hem_h3m_c_trials(list(inits), engine(vb, base, inits, opt["tau"]), opt, rd,
                                em_engine="device")
    return host, dev, rh, rd


def changes_of(LogLs):
    """The changes the rule tests: E-steps with num_iter > 1."""
    L = np.asarray(LogLs, dtype=np.float64)
    return (L[2:] - L[1:-1]) / np.abs(L[1:-1]) if L.size > 2 else np.zeros(0)


def assert_margin(host, termvalue):
    """No tested change lies within 5 % of termvalue (termvalue 0: none is 0)."""
    closest = np.inf
    for r, h in enumerate(host):
        ch = changes_of(h["LogLs"])
        if ch.size == 0:
            continue
        if termvalue == 0:
            assert not np.any(ch == 0), (r, ch)
            continue
        ratio = ch / termvalue
        closest = min(closest, float(np.min(np.abs(ratio - 1.0))))
        assert not np.any((ratio > 0.95) & (ratio < 1.05)), (r, ratio)
    return closest


def untouched(rngs, which=None):
    """The trials whose Generator drew nothing (no degenerate fix ran)."""
    fresh = rngs_for(len(rngs))
    return [r for r in (range(len(rngs)) if which is None else which)
            if rngs[r].bit_generator.state == fresh[r].bit_generator.state]


def compare(name, host, dev, trials=None):
    """The bars on the trials given (default: all).  Prints the worst figures first."""
    trials = list(range(len(host))) if trials is None else trials
    wl = wp = wz = 0.0
    for r in trials:
        a, b = dev[r], host[r]
        n = min(len(a["LogLs"]), len(b["LogLs"]))
        La, Lb = np.array(a["LogLs"][:n]), np.array(b["LogLs"][:n])
        wl = max(wl, float(np.max(np.abs(La - Lb) / np.abs(Lb))))
        wp = max(wp, max(rel_err(a[f], b[f]) for f in PARAMS))
        wz = max(wz, hatz_err(a["Z"], b["Z"]))
    print(f"[vhem_em_trials {name}] R={len(host)} num_iter={[h['num_iter'] for h in host]} "
          f"worst LogLs rel {wl:.2e} parameters {wp:.2e} Z {wz:.2e}")
    for r in trials:
        a, b = dev[r], host[r]
        assert a["num_iter"] == b["num_iter"], (name, r, a["num_iter"], b["num_iter"])
        assert len(a["LogLs"]) == len(b["LogLs"]) == b["num_iter"] + 1
        assert np.allclose(a["LogLs"], b["LogLs"], rtol=1e-10, atol=0), (name, r)
        assert a["LogL"] == a["LogLs"][-1]
        for f in PARAMS:
            assert a[f].shape == b[f].shape
            assert rel_err(a[f], b[f]) < 1e-9, (name, r, f)
        assert hatz_err(a["Z"], b["Z"]) < 1e-8, (name, r)
        assert rel_err(a["L_elbo1"], b["L_elbo1"]) < 1e-9, (name, r)
        assert np.array_equal(np.argmax(a["Z"], 1), np.argmax(b["Z"], 1)), (name, r)
    LLa = np.array([dev[r]["LogL"] for r in trials])
    LLb = np.array([host[r]["LogL"] for r in trials])
    assert int(np.argmax(LLa)) == int(np.argmax(LLb)), (name, LLa, LLb)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_engine_matches_host_engine(vb, name):
    base, inits, opt = build_case(name)
    host, dev, rh, rd = run_both(vb, base, inits, opt)
    R = len(inits)
    closest = assert_margin(host, opt["termvalue"])
    assert untouched(rh) == list(range(R)), "a degenerate fix ran in the host engine"
    print(f"[vhem_em_trials {name}] closest |change / termvalue - 1| {closest:.3g}")
    assert all(d_["fallback_trials"] == [] for d_ in dev)
    assert untouched(rd) == list(range(R))
    compare(name, host, dev)
    iters = [h["num_iter"] for h in host]
    if name == "A":
        assert len(set(iters)) >= 2, iters         # the latch keeps trials that stop apart
    if name == "B":
        # every trial runs max_iter + 2 E-steps
        assert all(len(h["LogLs"]) == opt["max_iter"] + 2 for h in host), iters
        assert all(len(d_["LogLs"]) == opt["max_iter"] + 2 for d_ in dev)
    if name == "H":
        assert min(iters) >= 8 and min(d_["num_iter"] for d_ in dev) >= 8
        # ... and without min_iter some trial would have stopped before (the case bites)
        assert min(h["num_iter"] for h in run_both(vb, *build_case("A"))[0]) < 8


def test_flagged_trials_take_the_host_engine(vb):
    """G: an initial omega of 0 (fix_degenerate_component) and an unvisited state
    (fix_degenerate_hmm).  The device flags both; their results and their Generators'
    states are the host engine's, bit for bit; the other trials meet the bars."""
    base, inits, opt = case_G()
    # the reference shows the fixes (and none in the other trials)
    for r in range(4):
        want = ref.c_step(inits[r], base, opt, draw=rngs_for(4)[r].random)
        assert (want["fixes"] > 0) == (r in (1, 2)), (r, want["fixes"])
    host, dev, rh, rd = run_both(vb, base, inits, opt)
    assert_margin([host[0], host[3]], opt["termvalue"])
    assert untouched(rh) == [0, 3]
    assert all(d_["fallback_trials"] == [1, 2] for d_ in dev)
    for r in (1, 2):
        assert rd[r].bit_generator.state == rh[r].bit_generator.state
        assert dev[r]["num_iter"] == host[r]["num_iter"]
        assert dev[r]["LogLs"] == host[r]["LogLs"] and dev[r]["LogL"] == host[r]["LogL"]
        for f in PARAMS + ("Z", "L_elbo1"):
            assert np.array_equal(dev[r][f], host[r][f]), (r, f)
    assert untouched(rd) == [0, 3]
    compare("G", host, dev, trials=[0, 3])


def test_runs_repeat_bit_for_bit_on_one_engine(vb):
    """I: A twice on one engine with another run (other options, so other stopping
    iterations) in between: records, tickets and the workspace start afresh."""
    from vbhem_amd import vhem
    base, inits, opt = build_case("A")
    eng = engine(vb, base, inits, opt["tau"])
    first = vhem.hem_h3m_c_trials(list(inits), eng, opt, rngs_for(4), em_engine="device")
    other = vhem.hem_h3m_c_trials(list(inits[::-1]), eng, dict(opt, max_iter=2), rngs_for(4),
                                  em_engine="device")
    assert all(o["num_iter"] <= 3 for o in other)
    again = vhem.hem_h3m_c_trials(list(inits), eng, opt, rngs_for(4), em_engine="device")
    for a, b in zip(first, again):
        assert a["num_iter"] == b["num_iter"] and a["LogLs"] == b["LogLs"] and a["LogL"] == b["LogL"]
        for f in PARAMS + ("Z", "L_elbo1"):
            assert np.array_equal(a[f], b[f]), f
        assert a["fallback_trials"] == b["fallback_trials"] == []


def test_vhem_cluster_with_both_engines(vb):
    """J: the one-line call; equal labels and t_best, trials_LL within the LogLs bar."""
    from vbhem_amd import vhem
    hm, _ = vhem.planted_hmms(20, seed=0)
    outs = {}
    for eng in ("host", "device"):
        base = vhem.hmms_to_h3m(hm, "full")
        opt = vhem.default_hemopt(2, 2, seed=3, trials=8, initmode="baseem", em_engine=eng)
        outs[eng] = (vhem.hem_h3m_c(base, opt, DEV),
                     vhem.vhem_cluster(hm, 2, 2, dict(seed=3, trials=8, initmode="baseem", em_engine=eng),
                                       device=DEV))
    (hh, ho), (dh, do) = outs["host"], outs["device"]
    # the preconditions, on the host engine's trajectory of the same eight trials
    base = vhem.hmms_to_h3m(hm, "full")
    opt = vhem.default_hemopt(2, 2, seed=3, trials=8, initmode="baseem")
    rngs = [np.random.Generator(np.random.PCG64(3 + t)) for t in range(1, 9)]
    inits = [vhem.initialize_hem_h3m_c(base, opt, rngs[t]) for t in range(8)]
    before = [g.bit_generator.state for g in rngs]
    trials = vhem.hem_h3m_c_trials(inits, engine(vb, base.numpy(), inits, opt["tau"]), opt, rngs)
    assert [h["LogL"] for h in trials] == list(hh["trials_LL"])
    assert_margin(trials, opt["termvalue"])
    assert [g.bit_generator.state for g in rngs] == before, "a degenerate fix ran"
    assert dh["t_best"] == hh["t_best"]
    assert np.allclose(dh["trials_LL"], hh["trials_LL"], rtol=1e-10, atol=0)
    assert np.array_equal(do["label"], ho["label"])
    assert np.allclose(do["trials_LL"], ho["trials_LL"], rtol=1e-10, atol=0)
    assert do["hemopt"]["em_engine"] == "device" and ho["hemopt"]["em_engine"] == "host"
    assert "fallback_trials" in dh and "fallback_trials" not in hh


def _c_entry(vb, base, K, S, R, max_iter=3, min_iter=1):
    """vhem_em_run_trials called directly on valid arrays: (status, workspace bytes)."""
    from vbhem_amd import _capi
    from vbhem_amd.estep import EStepEngine
    d, cov = base["centres"].shape[-1], base["covmode"]
    eng = EStepEngine(vb.BaseSet.from_numpy(base), R * K, S, 5, device=DEV, trials=R)
    lib = _capi.lib()
    nb = int(lib.vhem_em_trials_workspace_bytes(ctypes.byref(eng._bt), K, S, R, 5))
    dd = (d, d) if cov == 1 else (d,)
    arr = [np.full((R, K), 1.0 / K), np.full((R, K, S), 1.0 / S), np.full((R, K, S, S), 1.0 / S),
           np.zeros((R, K, S, d)),
           np.ascontiguousarray(np.broadcast_to(np.eye(d) if cov == 1 else np.ones(d), (R, K, S) + dd)),
           np.zeros((R, K, S))]
    mix = _capi.VhemMixTrialsT(K, S, d, cov, *(a.ctypes.data for a in arr))
    copt = _capi.VhemEmOptT(1.0, 1.0, 0.001, 1e-5, 5, max_iter, min_iter)
    SL = vb.host.stats_len(K, S, d, cov)
    LogLs = np.zeros((R, max(max_iter, 0) + 2))
    ni, fb, fi = (np.zeros(R, dtype=np.int32) for _ in range(3))
    LL, stats = np.zeros(R), np.zeros((R, SL))
    ws = torch.empty((max(nb, 256),), dtype=torch.uint8, device=DEV)
    ob = torch.full((base["prior"].shape[0],), 1.0 / base["prior"].shape[0], dtype=torch.float64, device=DEV)
    rc = lib.vhem_em_run_trials(ctypes.byref(eng._bt), _capi.ptr(ob), _capi.ptr(ob), R, 5,
                                ctypes.byref(copt), ctypes.byref(mix), LogLs.ctypes.data, ni.ctypes.data,
                                LL.ctypes.data, fb.ctypes.data, fi.ctypes.data, stats.ctypes.data,
                                _capi.ptr(eng.hatZ), _capi.ptr(eng.LL), _capi.ptr(ws), ws.numel(),
                                eng._stream())
    return rc, nb, lib.vbhem_last_error().decode(errors="replace")


# name: (N, K, S, Sb, d, cov, R)
OUTSIDE = {"S17": (12, 2, 17, 17, 2, 1, 2), "d17": (12, 2, 3, 3, 17, 0, 1)}


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_shapes_outside_the_device_engine(vb, name):
    """K: em_engine='device' takes the host engine (the same path: the same bits), and the
    C entry returns VBHEM_ERR_UNSUPPORTED naming the limit."""
    from vbhem_amd import vhem
    N, K, S, Sb, d, cov, R = OUTSIDE[name]
    cs = make_case(N, K, S, Sb, d, cov, seed=3, tau=5)
    inits = []
    for r in range(R):
        h = make_reduced(K, S, d, cov, seed=40 + r)
        h.update(omega=np.full(K, 1.0 / K), LogL=-np.inf)
        inits.append(h)
    bs = vb.BaseSet.from_numpy(cs["base"])
    outs = []
    for eng in ("host", "device"):
        opt = vhem.default_hemopt(K, S, seed=5, tau=5, max_iter=3, em_engine=eng,
                                  covar_type="full" if cov == 1 else "diag")
        assert not vhem.device_em_supported(bs, K, S, R, opt)
        outs.append(vhem.hem_h3m_c(bs, opt, DEV, inits=inits))
    a, b = outs
    assert a["LogLs"] == b["LogLs"] and a["t_best"] == b["t_best"]
    assert np.array_equal(a["trials_LL"], b["trials_LL"])
    for f in PARAMS + ("Z",):
        assert np.array_equal(a[f], b[f]), f
    assert "fallback_trials" not in b
    rc, nb, msg = _c_entry(vb, cs["base"], K, S, R)
    assert rc == -2 and nb == 0                    # VBHEM_ERR_UNSUPPORTED
    assert ("S > 16" in msg) if name == "S17" else ("d > 16" in msg)


def test_c_entry_limits(vb):
    """max_iter < 0 and a min_iter that needs more than max_iter + 2 E-steps are refused
    by name; max_iter = 0 runs (two E-steps)."""
    cs = make_case(12, 2, 3, 3, 2, 1, seed=3, tau=5)
    rc, nb, msg = _c_entry(vb, cs["base"], 2, 3, 2, max_iter=-1)
    assert rc == -2 and nb > 0 and "max_iter" in msg
    rc, _, msg = _c_entry(vb, cs["base"], 2, 3, 2, max_iter=3, min_iter=5)
    assert rc == -2 and "min_iter" in msg
    rc, _, _ = _c_entry(vb, cs["base"], 2, 3, 2, max_iter=0)
    assert rc == 0
