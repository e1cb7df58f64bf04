"""The gate masks of the fused E-step's gated schedule (K <= 64): the responsibility kernels
store one 64-bit word per base, bit j set when pair (i, j) passes the gate, from the very
comparison that feeds their per-chunk gate counts; gate_list_kernel ranks from those words
instead of reading the K doubles of Z again.  VBHEM_NO_GATE_MASKS=1 restores the second pass
over Z, K > 64 always takes it.

Every case runs the fused call with and without the switch on fresh engines and requires
list_tot, every list entry, hat_Z, L_elbo and the packed statistics to be equal (torch.equal /
array_equal: the same bits).  The lists are also held to what the gate says on the call's own
outputs -- VBHEM: hat_Z * tilde_N > 1e-8, VHEM: Z * omega_b > 0, one IEEE product each, so
numpy's bits are the kernel's -- ascending bases per cluster, and the mask words to the same
table (the region is filled with a sentinel first: with the switch on, or at K > 64, it must
come back untouched, which shows which path ran).

The lists, their totals and the masks are read from the engine's workspace at the offsets
vbhem_fused_workspace_layout gives (tests/test_workspace_layout.py checks those on the CPU).
"""
import ctypes

import numpy as np
import pytest
import torch

from cases import make_case, make_reduced

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATE = 1e-8
SENTINEL = 0xA5


def layout(eng):
    """(bytes, group, list offset, list_tot offset, mask offset or -1) of eng's fused workspace."""
    fn = eng.lib.vbhem_fused_workspace_layout
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_longlong)]
    out = (ctypes.c_longlong * 5)()
    nb = fn(ctypes.addressof(eng._bt), ctypes.addressof(eng._ct), eng.T, eng.trials, out)
    assert nb > 0
    return int(nb), int(out[0]), int(out[1]), int(out[2]), int(out[3])


def prepare_workspace(eng):
    """The engine's fused workspace, allocated here so that the mask region can be marked."""
    from vbhem_amd import _capi
    nb, group, o_list, o_tot, o_mask = layout(eng)
    eng._ws_fused = _capi.workspace(nb, eng.device)
    assert eng._ws_fused.numel() == nb
    if o_mask >= 0:
        eng._ws_fused[o_mask:o_mask + 8 * group] = SENTINEL
    return group, o_list, o_tot, o_mask


def read_workspace(eng, lay):
    group, o_list, o_tot, o_mask = lay
    K, N = eng.K, eng.N
    ws = eng._ws_fused
    assert N <= group   # one base group: the lists hold the whole call
    tot = ws[o_tot:o_tot + 4 * K].view(torch.int32).cpu().numpy().copy()
    lst = ws[o_list:o_list + 4 * K * group].view(torch.int32).reshape(K, group).cpu().numpy()
    lists = [lst[j, :tot[j]].copy() for j in range(K)]
    masks = None
    if o_mask >= 0:
        masks = ws[o_mask:o_mask + 8 * N].view(torch.int64).cpu().numpy().copy().view(np.uint64)
    return tot, lists, masks


def run_vbhem(vb, cs, K, S, tscale, trials=1, consts=None, logOmega=None, zero_base=None, **sw):
    """One fused VBHEM call on a fresh engine under the switches sw."""
    from vbhem_amd import _capi
    from vbhem_amd.estep import EStepEngine
    N = cs["base"]["centres"].shape[0]
    with _capi.switches(FUSED_DENSE=0, **sw):
        eng = EStepEngine(vb.BaseSet.from_numpy(cs["base"]), K, S, cs["T"], device=DEV, trials=trials)
        eng.set_clusters(cs["consts"] if consts is None else consts)
        eng.set_log_omega(np.log(np.full(K, 1.0 / K)) if logOmega is None else logOmega)
        lay = prepare_workspace(eng)
        tN = tscale * N * np.asarray(cs["base"]["omega"], dtype=np.float64)
        if zero_base is not None:
            tN[zero_base] = 0.0
        vec = eng.fused(torch.as_tensor(tN, device=DEV)).clone()
        torch.cuda.synchronize()
        tot, lists, masks = read_workspace(eng, lay)
    weight = eng.hatZ.cpu().numpy() * tN[:, None]      # Z = hat_Z tilde_N, as resp_kernel rounds it
    return dict(vec=vec, hatZ=eng.hatZ.clone(), LL=eng.LL.clone(), tot=tot, lists=lists, masks=masks,
                gated=weight > GATE, nfb=eng.fallback_count())


def compare(K, on, off, expect_masks):
    """The two runs equal; the lists and the masks what the gate says on the outputs."""
    N = on["gated"].shape[0]
    print("K", K, "N", N, "gated pairs", int(on["gated"].sum()), "of", on["gated"].size, "per cluster",
          on["tot"].tolist()[:8], "fallback", on["nfb"])
    assert np.array_equal(on["gated"], off["gated"])
    want = [np.flatnonzero(on["gated"][:, j]).astype(np.int32) for j in range(K)]
    for run in (on, off):
        assert run["tot"].tolist() == [len(w) for w in want]
        for j in range(K):
            assert np.array_equal(run["lists"][j], want[j]), j
    assert torch.equal(on["hatZ"], off["hatZ"])
    assert torch.equal(on["LL"], off["LL"])
    assert torch.equal(on["vec"], off["vec"])
    assert on["nfb"] == off["nfb"]
    if K > 64:
        assert on["masks"] is None and off["masks"] is None
        return
    sentinel = np.full(N, int.from_bytes(bytes([SENTINEL]) * 8, "little"), dtype=np.uint64)
    assert np.array_equal(off["masks"], sentinel)          # the switch: no mask is written
    if expect_masks:
        words = (on["gated"].astype(np.uint64) << np.arange(K, dtype=np.uint64)[None, :]).sum(1).astype(np.uint64)
        assert np.array_equal(on["masks"], words)
    else:
        assert np.array_equal(on["masks"], sentinel)


def both(vb, cs, K, S, tscale, **kw):
    on = run_vbhem(vb, cs, K, S, tscale, **kw)
    off = run_vbhem(vb, cs, K, S, tscale, NO_GATE_MASKS=1, **kw)
    compare(K, on, off, expect_masks=True)
    return on


# ---- cluster counts: every lane layout of the responsibility kernels -----------------------
@pytest.mark.parametrize("K", [1, 4, 8, 16, 17, 33, 64, 65])
@pytest.mark.parametrize("S", [8, 5], ids=["S8_list4", "S5_split"])
def test_cluster_counts(vb, K, S):
    """K = 4, 8, 16, 64: resp_kernel<K> (a lane per cluster, 64 / K bases per wave step, buffer
    stores); 1, 17, 33: resp_kernel<0> with masked lanes; 65: above a word, the pass over Z.
    N = 257: two chunks, the second slice of a chunk partial.  tscale = 100: short lists."""
    cs = make_case(257, K, S, S, 2, 0, seed=300 + K + S, tau=10)
    on = both(vb, cs, K, S, 100.0)
    assert on["gated"].any()
    if K >= 4:
        assert not on["gated"].all()


# ---- base counts: partial slices, one and several chunks ------------------------------------
@pytest.mark.parametrize("N", [1, 3, 255, 256, 257, 1030])
@pytest.mark.parametrize("K,S", [(16, 8), (17, 5)], ids=["K16_S8", "K17_S5"])
def test_base_counts(vb, N, K, S):
    """N = 1, 3: one partial wave step; 255 / 256 / 257: around gate_list_kernel's slice of
    256 bases and over one to five chunks; 1,030: 17 chunks of 61 bases."""
    cs = make_case(N, K, S, S, 2, 0, seed=400 + N + K, tau=10)
    both(vb, cs, K, S, 100.0)


# ---- the gate's corners ---------------------------------------------------------------------
@pytest.mark.parametrize("K,S", [(16, 8), (33, 5), (64, 5)], ids=["K16_S8", "K33_S5", "K64_S5"])
def test_no_pair_gated(vb, K, S):
    cs = make_case(257, K, S, S, 2, 0, seed=500 + K, tau=10)
    on = both(vb, cs, K, S, 1e-9)
    assert not on["gated"].any() and not on["tot"].any()


@pytest.mark.parametrize("K,S", [(16, 8), (33, 5), (64, 5)], ids=["K16_S8", "K33_S5", "K64_S5"])
def test_every_pair_gated(vb, K, S):
    """A small weight scale flattens hat_Z to about 1 / K: every pair passes, every list is
    the whole base set -- except the base whose tilde N is exactly 0, which must stay out of
    every list (Z = 0 is not > 1e-8)."""
    N = 257
    cs = make_case(N, K, S, S, 2, 0, seed=600 + K, tau=10)
    on = both(vb, cs, K, S, 1e-5, zero_base=100)   # Z about 1e-5 / K, far above the gate
    assert not on["gated"][100].any()
    assert np.delete(on["gated"], 100, axis=0).all()
    assert on["tot"].tolist() == [N - 1] * K
    assert on["masks"][100] == 0


def test_trials(vb):
    """resp_trials_kernel: three trials of five clusters as one set of 15."""
    from vbhem_amd.em import _stack_constants
    R, K, S, N = 3, 5, 5, 257
    css = [make_case(N, K, S, S, 2, 0, seed=700 + r, tau=10) for r in range(R)]
    consts = _stack_constants([c["consts"] for c in css])
    kw = dict(trials=R, consts=consts, logOmega=np.log(np.full(R * K, 1.0 / K)))
    on = both(vb, css[0], R * K, S, 100.0, **kw)
    assert on["gated"].any() and not on["gated"].all()


# ---- VHEM: the gate w = Z omega_b > 0 --------------------------------------------------------
def run_vhem(vb, base, h, K, S, T, **sw):
    from vbhem_amd import _capi
    from vbhem_amd.estep import EStepEngine
    N = base["centres"].shape[0]
    with _capi.switches(FUSED_DENSE=0, **sw):
        eng = EStepEngine(vb.BaseSet.from_numpy(base), K, S, T, device=DEV)
        eng.set_clusters(vb.host.vhem_cluster_constants(h, base["covmode"]))
        with np.errstate(divide="ignore"):
            eng.set_log_omega(np.log(h["omega"]))
        lay = prepare_workspace(eng)
        ob = torch.as_tensor(base["omega"], device=DEV)
        Ni = (100.0 * ob) * float(N)
        vec = eng.fused_vhem(Ni, ob, float(T), 1.0).clone()
        torch.cuda.synchronize()
        tot, lists, masks = read_workspace(eng, lay)
    weight = eng.hatZ.cpu().numpy() * np.asarray(base["omega"])[:, None]   # w = Z omega_b
    return dict(vec=vec, hatZ=eng.hatZ.clone(), LL=eng.LL.clone(), tot=tot, lists=lists, masks=masks,
                gated=weight > 0.0, nfb=eng.fallback_count())


@pytest.mark.parametrize("K,S", [(16, 8), (5, 5), (64, 5), (65, 5)], ids=["K16_S8", "K5_S5", "K64_S5", "K65_S5"])
def test_vhem(vb, K, S):
    """vhem_resp_kernel: a wave per base, its lane groups over the clusters.  Base 7 has
    omega_b = 0 (its weights are exactly 0 whatever Z is), the last cluster omega_r = 0 (Z
    exactly 0): neither may enter a list; the far clusters' Z underflow to 0 for some bases."""
    N, T, d, cov = 257, 10, 2, 0
    cs = make_case(N, 2, S, S, d, cov, seed=800 + K, tau=T)
    base = cs["base"]
    om = np.ones(N)
    om[7] = 0.0
    base["omega"] = om / om.sum()
    red = make_reduced(K, S, d, cov, seed=810 + K)
    rng = np.random.default_rng(820 + K)
    # the clusters spread along one direction away from cluster 0, the bases around cluster 0
    step = rng.normal(size=(S, d))
    for j in range(K):
        red["centres"][j] = red["centres"][0] + 0.4 * j * step
    base["centres"] = red["centres"][0][None] + rng.normal(0.0, 0.3, base["centres"].shape)
    omega = rng.dirichlet(np.ones(K) * 5)
    omega[K - 1] = 0.0
    h = dict(red, omega=omega / omega.sum(), LogL=-np.inf)
    on = run_vhem(vb, base, h, K, S, T)
    off = run_vhem(vb, base, h, K, S, T, NO_GATE_MASKS=1)
    compare(K, on, off, expect_masks=True)
    assert not on["gated"][7].any() and not on["gated"][:, K - 1].any()
    assert on["gated"].any()
