"""Seeded test cases: packed base sets + cluster posteriors + E-step constants.

Base HMMs come from the product's synthetic generator (same generator the
bench uses, on the CPU); cluster posteriors from the 'baseem' initialisation,
then perturbed so that every cluster/state has distinct transition, prior,
precision and scale parameters (baseem alone gives uniform epsilon/eta, which
would leave logA constant and hide indexing errors).
"""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

import pkgload
import vbhem_oracle as vo

vb = pkgload.load()


@pytest.fixture
def lib_switches():
    """``lib_switches(NO_BWD4=1)`` enters ``_capi.switches(...)`` for the rest of the
    test (this thread's library switches; names with or without the VBHEM_ prefix).
    Test modules import it from here."""
    from vbhem_amd import _capi
    with contextlib.ExitStack() as stack:
        yield lambda **values: stack.enter_context(_capi.switches(**values))


def post_dict(post) -> dict:
    return {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in post.asdict().items()}


def make_case(N=6, K=3, S=3, Sb=3, d=2, covmode=1, seed=0, ragged=False, perturb=True,
              tau=10, exprmt1=False, face=False, Nv=100, **opt_over):
    """Returns dict(base=numpy base dict, post=posterior dict, consts=E-step constants
    (oracle prelude), opt=options, T=tau, bs=BaseSet, P=Posterior)."""
    bs = vb.synth_base_set(N, K, Sb, d, covmode, seed=1000 + seed, device="cpu",
                           exprmt1=exprmt1, ragged=ragged, face=face)
    v0 = max(5.0, d + 1.0)
    if face:  # demo/vbdemo_face.m:49-61 hyperparameters (m0 defaults to [256, 192])
        opt_over = dict(dict(W0=0.001, v0=10.0), **opt_over)
        v0 = opt_over.pop("v0")
    opt = vb.default_options(K, S, d, tau=tau, Nv=Nv, covmode=covmode, v0=v0, **opt_over)
    rb, rg, om = vb.baseem_draws(bs, K, S, seed=77 + seed)
    P = vb.baseem_init(bs, opt, rb, rg, om)
    if perturb:
        rng = np.random.default_rng(500 + seed)
        P.epsilon = P.epsilon * rng.uniform(0.2, 1.8, P.epsilon.shape)
        P.eta = P.eta * rng.uniform(0.2, 1.8, P.eta.shape)
        P.lam = P.lam * rng.uniform(0.5, 1.5, P.lam.shape)
        P.v = P.v + rng.uniform(0.0, 3.0, P.v.shape)
        sc = rng.uniform(0.7, 1.3, P.v.shape)
        P.W = P.W * (sc[..., None, None] if covmode == 1 else sc[..., None])
        P.m = P.m + rng.normal(0.0, 8.0 if face else 0.3, P.m.shape)
        P.alpha = P.alpha * rng.uniform(0.5, 1.5, P.alpha.shape)
    base = bs.numpy()
    post = post_dict(P)
    consts = vo.prelude(post, covmode)
    return dict(base=base, post=post, consts=consts, opt=opt, T=tau, bs=bs, P=P)


# shapes exercised by the parity tests: (name, N, K, S, Sb, d, covmode, T, ragged)
SHAPES = [
    ("full_small", 5, 3, 3, 3, 2, 1, 6, False),
    ("diag_small", 5, 3, 3, 3, 2, 0, 6, False),
    ("T1", 4, 2, 3, 3, 2, 1, 1, False),
    ("T2", 4, 2, 3, 3, 2, 1, 2, False),
    ("S1", 4, 3, 1, 3, 2, 1, 5, False),
    ("Sb1", 4, 3, 3, 1, 2, 1, 5, False),
    ("ragged_full", 9, 3, 4, 4, 3, 1, 7, True),
    ("ragged_diag", 9, 3, 4, 4, 3, 0, 7, True),
    ("SbgtS", 4, 2, 2, 5, 2, 1, 4, False),
    ("odd", 5, 5, 5, 5, 5, 1, 9, False),
    ("d1", 4, 2, 3, 3, 1, 0, 5, False),
    ("C2like", 6, 4, 3, 2, 2, 1, 50, False),
    ("C3like", 6, 8, 5, 5, 2, 0, 10, False),
    ("C4like", 3, 16, 8, 8, 8, 1, 10, False),
    ("C5like", 1, 32, 12, 12, 16, 1, 10, False),
    ("S16", 2, 3, 16, 16, 4, 1, 6, False),
    ("d16diag", 2, 3, 6, 6, 16, 0, 6, False),
    # S = 8, T = 10: the MFMA kernels (fb_bwd4_kernel, fb_list4_kernel); padded base
    # states (SB < 8, ragged) and gate lists that end inside a 4-pair quad
    ("S8_ragged", 9, 5, 8, 6, 3, 1, 10, True),
    ("S8_quads", 37, 4, 8, 8, 2, 0, 10, False),
    # S = 12: the MFMA backward pass on 3 x 3 blocks (fb_bwd12_kernel); SB < 12 pads
    # whole and partial column blocks, a quad ending past the last base
    ("S12_ragged", 9, 5, 12, 9, 3, 1, 10, True),
    ("S12_quads", 37, 4, 12, 12, 2, 0, 10, False),
    ("S12_sb5", 7, 3, 12, 5, 2, 1, 6, False),
    # outside the column-split kernel's limits (S <= 16, SB <= S, d <= 16): generic kernel
    ("d20", 3, 2, 3, 3, 20, 1, 5, False),
    ("S20", 2, 2, 20, 20, 2, 1, 4, False),
    ("T50_SbgtS", 3, 3, 2, 6, 2, 0, 50, True),
]


# the state counts S <= 16 that SHAPES leaves out: 7, 9, 10, 11, 13, 14, 15 (same tuple layout;
# tests/test_fb_state_counts_gpu.py).  fb_split_kernel holds rows in LPC lanes of SH =
# ceil(S / LPC) rows each (dense / list: LPC = 2 at S = 7, 4 from 9; backward: 1, 2), so
# these S have padded rows (S = 9: lane h = 3 holds none but padded rows) and 14 to 60
# lanes per pair: pairs straddle wavefronts and the block's last lanes idle.
# fb_bwd2_kernel has a padded second column at S = 7 and, from 9, 64 % S idle lanes per
# wave with pairs across its 16-lane DPP rows.  N = 37 (75 at S = 7): with every pair
# gated a cluster's list is more than two of the list kernel's work items (at most
# 512 / (S LPC) pairs) and fb_bwd2_kernel's last tile ends inside a wave
STATE_COUNT_SHAPES = [
    ("S7_ragged", 9, 3, 7, 7, 2, 1, 10, True),    # d = 2 full: K1 inside the kernels
    ("S7_sb4", 6, 4, 7, 4, 3, 1, 6, False),       # emission GEMM path, padded base columns
    ("S7_lists", 75, 2, 7, 7, 2, 0, 10, False),
    ("S9_ragged", 9, 3, 9, 9, 3, 1, 10, True),
    ("S9_sb5", 5, 2, 9, 5, 2, 0, 6, False),
    ("S9_lists", 37, 4, 9, 9, 2, 0, 10, False),
    ("S10_lists", 37, 3, 10, 10, 2, 1, 10, False),
    ("S11_ragged", 37, 3, 11, 8, 4, 0, 7, True),
    ("S13_ragged", 37, 3, 13, 13, 3, 1, 10, True),
    ("S13_sb1", 4, 2, 13, 1, 2, 1, 5, False),
    ("S14_sb9", 37, 2, 14, 9, 2, 0, 6, False),
    ("S15_ragged", 37, 3, 15, 15, 4, 1, 10, True),
]


# the cluster counts K that the single-call shapes above leave out (they stop at K in {1..6, 8,
# 16, 32}; same tuple layout; tests/test_cluster_count_cases.py, test_fused_cluster_counts_gpu.py).
# The fused epilogue picks its path by K: resp_kernel<K> for K = 4, 8, 16, 32, 64 (a lane per
# cluster, 64 / K bases per wave step, two steps pipelined), else resp_kernel<0> with G = the
# power of two >= K lanes per base -- K <= G with the lanes past K masked, or K > 64 with a lane
# holding the clusters gl, gl + 64, ...  A chunk is at least 64 bases: N = 131 gives chunks of
# 44 / 44 / 43, N = 65 and 70 two.  Downstream of K: gate_list_kernel's ballot masks of all K
# clusters (a second round of its j0 loop past K = 256), the (cluster, part) grid of
# stats_list_m_kernel, stats_kernel's row groups (ngroups > 1 from K S > 128), stats_final_kernel
# and nm_kernel
CLUSTER_COUNT_SHAPES = [
    ("K2_chunks", 131, 2, 3, 3, 2, 1, 5, True),      # G = 2: 32 bases per wave step, 3 chunks
    ("K4_chunks", 131, 4, 3, 3, 2, 0, 5, False),     # resp_kernel<4>: chunks shorter than one step pair
    ("K7", 131, 7, 3, 3, 2, 1, 5, True),             # G = 8, one masked lane
    ("K9", 131, 9, 2, 3, 2, 0, 4, False),            # G = 16, 7 masked lanes
    ("K15", 70, 15, 3, 3, 2, 1, 5, True),
    ("K17", 131, 17, 3, 3, 2, 0, 5, True),           # G = 32
    ("K31", 65, 31, 2, 2, 2, 1, 4, False),           # N = 65: a second chunk
    ("K32_chunks", 131, 32, 3, 3, 2, 1, 5, True),    # resp_kernel<32>
    ("K33", 131, 33, 3, 3, 2, 0, 5, True),           # G = 64, one base per step
    ("K63", 65, 63, 2, 2, 2, 1, 4, False),
    ("K64", 131, 64, 3, 3, 2, 1, 5, True),           # resp_kernel<64>
    ("K64_one", 9, 64, 2, 2, 3, 0, 4, False),        # one short chunk: the second pipelined step all past its end
    ("K65", 131, 65, 3, 3, 2, 1, 5, True),           # the K > 64 loop: lane 0 holds two clusters
    ("K100", 70, 100, 2, 2, 2, 0, 4, False),
    ("K129", 65, 129, 2, 2, 2, 1, 4, True),          # lanes hold 3 or 2 clusters
    ("K257", 70, 257, 2, 2, 2, 0, 4, False),         # gate_list_kernel's second j0 round (KC = 1)
    ("K13_S8", 45, 13, 8, 8, 3, 1, 10, True),        # fb_bwd4 / fb_list4 and the MFMA statistics at odd K
    ("K33_S8", 45, 33, 8, 6, 2, 0, 10, True),
    ("K17_S12", 37, 17, 12, 9, 3, 1, 10, True),      # fb_bwd12 / fb_list12
    ("K65_S5", 70, 65, 5, 5, 2, 0, 10, False),       # the C3-like short-K1 path at K > 64
]

# batched trials, R trials of K_trial clusters as one set of R K_trial <= 256 clusters
# (resp_trials_kernel: G lanes per base from the total, a lane holds the clusters gl + s G of
# slots s < 4, a trial's clusters are consecutive and so cross lane 63 and the slots):
# (name, N, K_trial, S, Sb, d, covmode, T, ragged, R)
TRIAL_COUNT_SHAPES = [
    ("t3x5", 131, 5, 3, 3, 2, 1, 5, True, 3),        # 15 clusters: G = 16, 4 bases per step
    ("t9x3", 131, 3, 3, 3, 2, 0, 5, True, 9),        # 27: G = 32
    ("t5x13", 70, 13, 3, 3, 2, 1, 5, True, 5),       # 65: one cluster in slot 1
    ("t22x3", 131, 3, 3, 3, 2, 1, 5, True, 22),      # 66: trial 21 = lane 63 of slot 0 + lanes 0, 1 of slot 1
    ("t10x7", 131, 7, 2, 2, 2, 0, 4, False, 10),     # 70
    ("t2x33", 131, 33, 2, 2, 2, 0, 4, False, 2),     # 66: a trial wider than half a wave
    ("t26x5", 131, 5, 2, 2, 2, 0, 4, False, 26),     # 130: three slots
    ("t3x65", 70, 65, 2, 2, 2, 1, 4, False, 3),      # 195: a trial wider than a wave
    ("t51x5", 70, 5, 2, 2, 2, 1, 4, False, 51),      # 255
    ("t64x4", 131, 4, 2, 2, 2, 0, 4, True, 64),      # 256: the limit
    ("t2x128", 65, 128, 2, 2, 2, 0, 4, False, 2),    # 256 with two trials
    ("t100x1", 70, 1, 3, 3, 2, 1, 5, False, 100),    # K_trial = 1: hat_Z = 1 + 1e-50 everywhere
]


# the observation dimensions d <= 16 that the shapes above leave out (same tuple layout;
# tests/test_dimension_cases.py, test_fused_dimensions_gpu.py).  By d and the
# covariance mode the E-step picks: the emission GEMM's k-steps kq = ceil(KD / 4), KD = d (d + 1)
# / 2 + d (full) or 2 d (diagonal), in register buckets of 4, 12 and 40 k-steps; the feature
# tiles nt = ceil(NU / 16), NU = 1 + KD, of stats_list_m_kernel<NTW, G> (nt <= 4: G = 4 pair
# groups of NTW = nt tiles; 5-6: G = 2, NTW = 3; 7-8: G = 2, NTW = 4; 9-12: G = 1, NTW = 3) and,
# behind the switches, the grouped kernel (NU <= 32), the operand kernel (NU <= 64) and the
# covariance gather.  Small otherwise: N = 37 ragged bases, K = 4, S = Sb = 3, T = 5
DIMENSION_SHAPES = [
    ("d1_full", 37, 4, 3, 3, 1, 1, 5, True),        # kq = 1 of a full covariance (KD = 2), NU = 3
    ("d6_full", 37, 4, 3, 3, 6, 1, 5, True),        # kq = 7, 12-step bucket; NU = 28, (nt, G, NTW) = (2, 4, 2)
    ("d7_full", 37, 4, 3, 3, 7, 1, 5, True),        # kq = 9; NU = 36, (3, 4, 3)
    ("d9_full", 37, 4, 3, 3, 9, 1, 5, True),        # kq = 14: first of the 40-step bucket; NU = 55, (4, 4, 4)
    ("d10_full", 37, 4, 3, 3, 10, 1, 5, True),      # kq = 17; NU = 66, (5, 2, 3): the second tile group half padded
    ("d11_full", 37, 4, 3, 3, 11, 1, 5, True),      # kq = 20; NU = 78, (5, 2, 3)
    ("d12_full", 37, 4, 3, 3, 12, 1, 5, True),      # kq = 23; NU = 91, (6, 2, 3)
    ("d13_full", 37, 4, 3, 3, 13, 1, 5, True),      # kq = 26; NU = 105, (7, 2, 4): the second tile group partial
    ("d14_full", 37, 4, 3, 3, 14, 1, 5, True),      # kq = 30; NU = 120, (8, 2, 4)
    ("d15_full", 37, 4, 3, 3, 15, 1, 5, True),      # kq = 34; NU = 136, (9, 1, 3): the fourth tile group empty
    ("d6_diag", 37, 4, 3, 3, 6, 0, 5, True),        # kq = 3 (the raw kernel's kq = 3 under NO_UGEMM); NU = 13
    ("d7_diag", 37, 4, 3, 3, 7, 0, 5, True),        # kq = 4, NU = 15: last of the 4-step bucket and of one tile
    ("d8_diag", 37, 4, 3, 3, 8, 0, 5, True),        # kq = 4; NU = 17: first of two tiles
    ("d9_diag", 37, 4, 3, 3, 9, 0, 5, True),        # kq = 5: first of the 12-step bucket; NU = 19
    ("d15_diag", 37, 4, 3, 3, 15, 0, 5, True),      # kq = 8; NU = 31
    # K S = 132 > 128 in the 40-step bucket: W' of 256 rows is staged in four chunks of 4 row tiles
    ("d11_rows", 37, 33, 4, 4, 11, 1, 5, True),
    # S = 8, T = 10 (fb_bwd4_kernel / fb_list4_kernel): the list-4 accumulation with two feature
    # tiles of a full covariance; and NU = 55 past the accumulation's 48, where the statistics
    # fall to stats_list_m_kernel<4, 4> behind fb_list4_kernel (padded base states)
    ("d6_S8", 37, 4, 8, 8, 6, 1, 10, False),
    ("d9_S8_ragged", 37, 4, 8, 6, 9, 1, 10, True),
    # S = 12 (fb_bwd12_kernel / fb_list12_kernel) on the 40-step emission GEMM
    ("d10_S12", 37, 4, 12, 9, 10, 1, 10, True),
]


def make_reduced(K=3, S=3, d=2, covmode=1, seed=0, zero_transition=False) -> dict:
    """Point-estimate reduced HMMs for the VHEM sibling (hem_hmm_bwd_fwd_mex.c):
    Dirichlet rows for A and prior, means in [0, 5]^d, SPD covariances
    (L L'/d + 0.5 I) or diagonal U[0.5, 1.5].  zero_transition sets A[0][0][-1]
    (renormalised) and prior[0][-1] to 0, so log(A) and log(prior) hold -inf."""
    rng = np.random.default_rng(4000 + seed)
    A = rng.dirichlet(np.ones(S), size=(K, S))
    prior = rng.dirichlet(np.ones(S), size=K)
    if zero_transition and S > 1:
        A[0, 0, -1] = 0.0
        A[0, 0] /= A[0, 0].sum()
        prior[0, -1] = 0.0
        prior[0] /= prior[0].sum()
    centres = rng.uniform(0.0, 5.0, (K, S, d))
    if covmode == 1:
        L = rng.normal(size=(K, S, d, d))
        covars = np.einsum("ksab,kscb->ksac", L, L) / d + 0.5 * np.eye(d)
    else:
        covars = rng.uniform(0.5, 1.5, (K, S, d))
    return dict(A=A, prior=prior, centres=centres, covars=covars)

