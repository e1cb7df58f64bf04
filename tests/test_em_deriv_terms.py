"""The arithmetic of the bound's hyperparameter derivatives that trials_derivs_kernel runs
on the device (csrc/vbhem_em_deriv_terms.h), checked on the CPU through its host build
(tests/emderivcheck) against host.lower_bound_derivs(...)["raw"]; and the C ABI of the
batched trials loop with per-trial hyperparameters (vbhem_em_run_trials_hyp) as far as
it can be checked without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cases import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_PATH = os.path.join(ROOT, "tests", "emderivcheck", "libemderivcheck.so")


@pytest.fixture(scope="module")
def deriv_lib():
    if not os.path.exists(CHECK_PATH):
        subprocess.run(["make", "-C", ROOT, "emderivcheck"], check=True, stdout=subprocess.DEVNULL)
    lib = ctypes.CDLL(CHECK_PATH)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emderivcheck_table_len.restype = ctypes.c_int
    lib.emderivcheck_table_layout.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.emderivcheck_table_layout.restype = None
    lib.emderivcheck_raw.argtypes = [ctypes.c_int] * 5 + [dp] * 10
    lib.emderivcheck_raw.restype = None
    return lib


def _table(lib, opt, d):
    """A trial's hyperparameter table as vbhem_em_run_trials_hyp fills it (the bound's
    four constants are not read by the derivatives and stay 0)."""
    lay = (ctypes.c_int * 7)()
    lib.emderivcheck_table_layout(d, lay)
    h = np.zeros(lib.emderivcheck_table_len(d))
    assert h.size == 9 + d + d * d
    for i, name in enumerate(("alpha0", "eta0", "epsilon0", "lambda0", "v0")):
        h[lay[i]] = opt[name]
    h[lay[5]:lay[5] + d] = np.asarray(opt["m0"], dtype=float)
    W0 = np.asarray(opt["W0"], dtype=float)
    W0f = W0 * np.eye(d) if W0.size == 1 else np.diag(W0)
    h[lay[6]:lay[6] + d * d] = np.linalg.inv(W0f).reshape(-1)
    return h


@pytest.mark.parametrize("cov,W0", [(1, 0.7), (1, [0.4, 0.9, 1.3]), (0, 0.25), (0, [0.3, 0.5, 2.0])],
                         ids=["full-iid", "full-diagW0", "diag-iid", "diag-diagW0"])
def test_deriv_terms_match_host(vb, deriv_lib, cov, W0):
    """The four cases of tests/test_hyp.py::test_native_derivatives_match_host, at its bar."""
    cs = make_case(6, 4, 3, 3, 3, cov, seed=29, tau=5, W0=W0, m0=[0.2, -0.4, 0.8])
    opt = dict(cs["opt"])
    P, consts = cs["P"], cs["consts"]
    K, S, d = P.m.shape
    logOm = vb.host.log_omega_tilde(P.alpha)
    ref = vb.host.lower_bound_derivs(logOm, P, consts, opt, cov)["raw"]
    nW = int(np.size(opt["W0"]))
    out = np.zeros(5 + nW + d)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (
        P.v, P.lam, P.m, P.W, logOm, consts["logPi"], consts["logA"], consts["logLambdaTilde"],
        _table(deriv_lib, opt, d), out)]
    dp = ctypes.POINTER(ctypes.c_double)
    deriv_lib.emderivcheck_raw(K, S, d, cov, nW, *[a.ctypes.data_as(dp) for a in arrs])
    out = arrs[-1]
    got = {"alpha0": out[0:1], "eta0": out[1:2], "epsilon0": out[2:3], "v0": out[3:4],
           "lambda0": out[4:5], "W0": out[5:5 + nW], "m0": out[5 + nW:]}
    worst = 0.0
    for k, v in ref.items():
        v = np.atleast_1d(v)
        worst = max(worst, float(np.max(np.abs(got[k] - v) / np.maximum(np.abs(v), 1.0))))
    print(f"[deriv terms cov={cov} nW={nW}] worst |got - ref| / max(|ref|, 1) = {worst:.2e}")
    for k, v in ref.items():
        np.testing.assert_allclose(got[k], np.atleast_1d(v), rtol=1e-12, atol=1e-12, err_msg=k)


def _base(N, Sb, d, cov=1):
    from vbhem_amd import _capi
    p = 1 << 20
    return _capi.BaseT(N, Sb, d, cov, p, p, p, p, p)


def test_trials_hyp_workspace_bytes(capi_lib):
    ws = capi_lib.vbhem_em_trials_hyp_workspace_bytes
    b = lambda *a, **k: ctypes.byref(_base(*a, **k))  # noqa: E731
    assert ws(b(10, 3, 2), 3, 3, 4, 8, 1) > 0
    assert ws(b(10, 3, 2), 3, 3, 4, 8, 2) > ws(b(10, 3, 2), 3, 3, 4, 8, 1)   # W0 per dimension
    assert ws(b(10, 3, 2), 64, 3, 4, 8, 1) > 0     # R K = 256
    assert ws(b(10, 3, 2), 65, 3, 4, 8, 1) == 0    # R K = 260
    assert ws(b(10, 3, 17), 3, 3, 4, 8, 1) == 0    # d = 17
    assert ws(b(10, 3, 2), 3, 17, 4, 8, 1) == 0    # S = 17
    assert ws(b(10, 4, 2), 3, 3, 4, 8, 1) == 0     # Sb > S
    assert ws(b(10, 3, 2), 3, 3, 0, 8, 1) == 0     # R = 0
    assert ws(b(10, 3, 3), 3, 3, 4, 8, 2) == 0     # W0_len neither 1 nor d
    assert ws(None, 3, 3, 4, 8, 1) == 0
    # more trials need more room; never more than the plain entry's, whose layout it shares
    assert ws(b(10, 3, 2), 3, 3, 8, 8, 1) > ws(b(10, 3, 2), 3, 3, 4, 8, 1)
    assert ws(b(10, 3, 2), 3, 3, 4, 8, 2) == capi_lib.vbhem_em_trials_workspace_bytes(b(10, 3, 2), 3, 3, 4, 8)


def test_run_trials_hyp_refuses_bad_arguments(vb, capi_lib):
    from vbhem_amd import _capi, native_em
    K, S, d, R = 3, 3, 2, 4
    cs = make_case(6, K, S, 3, d, 1, seed=3, tau=4)
    pbs = [native_em._PostBuf(cs["P"], 1) for _ in range(R)]
    arr = (type(pbs[0].t) * R)(*[pb.t for pb in pbs])
    v = ctypes.c_void_p(1 << 20)

    def run(base, opts, posts=arr):
        obs = [native_em._OptBuf(o) for o in opts] if opts is not None else None
        oa = (_capi.EmOptT * R)(*[ob.t for ob in obs]) if obs is not None else None
        # a workspace too small for any shape: a call that passes the checks ends there
        return capi_lib.vbhem_em_run_trials_hyp(ctypes.byref(base), v, R, 4, oa, None, posts, v, v, v, v, v, v,
                                                v, v, v, ctypes.c_size_t(8), None)

    opt = dict(cs["opt"], max_iter=3, minDiff=1e-6)
    assert run(_base(6, 3, d), [opt] * R) == -3                       # VBHEM_ERR_WORKSPACE: checks passed
    assert run(_base(6, 3, d), None) == -1
    assert run(_base(6, 3, d), [opt] * R, None) == -1
    for bad in (dict(opt, max_iter=4), dict(opt, minDiff=1e-5), dict(opt, Nv=50.0), dict(opt, W0=[1.0, 2.0])):
        rc = run(_base(6, 3, d), [opt, opt, bad, opt])
        assert rc == -1 and b"equal in every trial" in capi_lib.vbhem_last_error(), bad
    rc = run(_base(6, 3, d + 1), [opt] * R)
    assert rc == -1 and b"covmode" in capi_lib.vbhem_last_error()
    rc = run(_base(6, 4, d), [opt] * R)                               # Sb > S
    assert rc == -2 and b"vbhem_em_run_trials_hyp" in capi_lib.vbhem_last_error()
    # differing hyperparameters alone are what the entry is for
    assert run(_base(6, 3, d), [opt, dict(opt, alpha0=2.0, v0=7.5), opt, dict(opt, m0=[0.1, 0.2])]) == -3
