"""The library's run-time switches (csrc/vbhem_switches.h; vbhem_switch_* in
include/vbhem_estep.h; _capi.switch_names / set_switch / switches): one table, defaults
from the environment read once, changes per host thread.

CPU: the table through the C API, the context manager, the per-thread set, the
environment defaults (a fresh child process) and DESIGN.md 5.1.
GPU: the switches that choose the recursion kernels of the gated schedule at S = 8 and
S = 12 each select the kernel they name (vbhem_last_kernel), and that kernel's outputs
agree with the default kernels' (the oracle tests' bounds: RTOL_PAIRS for L_elbo,
stat_err < 1e-9 for the statistics).  Some of them (VBHEM_NO_BWD2 / _BWD12 / _LIST12) are
set by no other test: wired to the wrong field they would change nothing anywhere else.
"""
import glob
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from cases import make_case
from conftest import ROOT, RTOL_PAIRS, elem_err, stat_err


@pytest.fixture
def capi(capi_lib):
    from vbhem_amd import _capi
    yield _capi
    capi_lib.vbhem_switch_reset()


def test_names_round_trip(capi):
    names = capi.switch_names()
    assert names and len(set(names)) == len(names)
    assert capi.lib().vbhem_switch_name(len(names)) is None
    assert capi.lib().vbhem_switch_name(-1) is None
    for name in names:
        assert name.startswith("VBHEM_")
        v = capi.get_switch(name)
        assert capi.get_switch(name[len("VBHEM_"):]) == v     # with or without the prefix
        assert capi.set_switch(name, v) == v
        assert capi.get_switch(name) == v
        # another value (a boolean holds 0 or 1; an integer whatever it is given)
        new = 1 - v if v in (0, 1) else 37
        assert capi.set_switch(name, new) == v
        assert capi.get_switch(name) == new
        assert capi.set_switch(name, v) == new


def test_set_get_reset(capi):
    assert capi.set_switch("NO_BWD4", 1) == 0
    assert capi.set_switch("VBHEM_NO_BWD4", 1) == 1
    assert capi.set_switch("GROUP_BASES", 64) == -1
    assert (capi.get_switch("NO_BWD4"), capi.get_switch("GROUP_BASES")) == (1, 64)
    for bad in ("NO_SUCH_SWITCH", "VBHEM_", "no_bwd4", ""):
        with pytest.raises(capi.VbhemError, match=r"status -1\)") as ex:
            capi.set_switch(bad, 1)
        assert bad in str(ex.value)
        with pytest.raises(capi.VbhemError, match=r"status -1\)"):
            capi.get_switch(bad)
    assert (capi.get_switch("NO_BWD4"), capi.get_switch("GROUP_BASES")) == (1, 64)
    capi.lib().vbhem_switch_reset()
    assert (capi.get_switch("NO_BWD4"), capi.get_switch("GROUP_BASES")) == (0, -1)


def test_context_manager_restores(capi):
    capi.set_switch("NSLAB", 7)
    with capi.switches(NO_LIST4=1, VBHEM_NSLAB="9", EM_SPLIT=0):
        assert [capi.get_switch(n) for n in ("NO_LIST4", "NSLAB", "EM_SPLIT")] == [1, 9, 0]
        with capi.switches(NO_LIST4=0):
            assert capi.get_switch("NO_LIST4") == 0
        assert capi.get_switch("NO_LIST4") == 1
    assert [capi.get_switch(n) for n in ("NO_LIST4", "NSLAB", "EM_SPLIT")] == [0, 7, -1]
    with pytest.raises(KeyError):
        with capi.switches(NO_BWD12=1, SU_BLOCKS=5):
            assert (capi.get_switch("NO_BWD12"), capi.get_switch("SU_BLOCKS")) == (1, 5)
            raise KeyError("inside")
    assert (capi.get_switch("NO_BWD12"), capi.get_switch("SU_BLOCKS")) == (0, -1)
    # an unknown name: the switches set before it are put back
    with pytest.raises(capi.VbhemError):
        with capi.switches(NO_BWD12=1, NO_SUCH_SWITCH=1):
            pass
    assert capi.get_switch("NO_BWD12") == 0


def test_fused_mode_is_the_fused_dense_switch(capi):
    prev = capi.set_fused_mode(capi.FUSED_DENSE)
    assert capi.get_switch("FUSED_DENSE") == 1
    with capi.switches(FUSED_DENSE=0):
        assert capi.set_fused_mode(capi.FUSED_GATED) == capi.FUSED_GATED
    assert capi.set_fused_mode(prev) == capi.FUSED_DENSE


def test_switches_are_per_thread(capi):
    capi.set_switch("NO_BWD4", 1)
    seen = {}

    def worker():
        seen["default"] = capi.get_switch("NO_BWD4")   # this thread's own set
        capi.set_switch("NO_LIST4", 1)
        capi.set_switch("NO_BWD4", 0)
        seen["own"] = (capi.get_switch("NO_BWD4"), capi.get_switch("NO_LIST4"))

    th = threading.Thread(target=worker)
    th.start()
    th.join()
    assert seen == {"default": 0, "own": (0, 1)}
    # the main thread's set is untouched by the worker
    assert (capi.get_switch("NO_BWD4"), capi.get_switch("NO_LIST4")) == (1, 0)


def test_environment_defaults():
    """The process defaults, in a fresh process: a boolean set to 1 and to 0, two integers,
    and a switch that is not set."""
    code = ("import sys; sys.path.insert(0, %r); import pkgload; pkgload.load(); "
            "from vbhem_amd import _capi; "
            "print(*[_capi.get_switch(n) for n in "
            "('NO_BWD4', 'NO_LIST4', 'GROUP_BASES', 'EM_SPLIT', 'NSLAB', 'NO_BWD12')])" % ROOT)
    env = {k: v for k, v in os.environ.items() if not k.startswith("VBHEM_") or k == "VBHEM_LIB_PATH"}
    env.update(VBHEM_NO_BWD4="1", VBHEM_NO_LIST4="0", VBHEM_GROUP_BASES="64", VBHEM_EM_SPLIT="0")
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True, capture_output=True,
                         text=True).stdout
    assert out.split() == ["1", "0", "64", "0", "-1", "0"]


def test_documented(capi):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = re.search(r"^### 5\.1 .*?(?=^## )", text, re.S | re.M).group(0)
    for name in capi.switch_names():
        assert re.search(r"`%s\b" % name, sec), name
    pkg = os.path.dirname(os.path.abspath(capi.__file__))
    srcs = glob.glob(os.path.join(pkg, "csrc", "*"))
    assert srcs
    for path in srcs:
        assert "VBHEM_NO_UPF" not in open(path, errors="replace").read(), path


# ---- GPU: each recursion-kernel switch selects the kernel it names -------------------
DEV = "cuda:0"
N, K, D, COV, T = 37, 3, 2, 1, 10     # nine quads of bases and a partial one; T = 10: list kernels
GATED_SHAPES = {"S8": (8, 8), "S8_sb5": (8, 5), "S12": (12, 12)}
# S: (backward kernel, list kernel, their switches)
MFMA = {8: ("fb_bwd4_kernel", "fb_list4_kernel", "NO_BWD4", "NO_LIST4"),
        12: ("fb_bwd12_kernel", "fb_list12_kernel", "NO_BWD12", "NO_LIST12")}
_default_runs = {}


def _run(vb, shape, **sw):
    from vbhem_amd import _capi
    from vbhem_amd.estep import EStepEngine
    S, Sb = GATED_SHAPES[shape]
    cs = make_case(N, K, S, Sb, D, COV, seed=61 + S + Sb, ragged=True, tau=T)
    with _capi.switches(FUSED_DENSE=0, **sw):
        eng = EStepEngine(vb.BaseSet.from_numpy(cs["base"]), K, S, T, device=DEV)
        eng.set_clusters(cs["consts"])
        eng.set_log_omega(np.log(np.full(K, 1.0 / K)))
        vec = eng.fused(torch.as_tensor(100.0 * N * cs["base"]["omega"], device=DEV)).cpu().numpy()
        torch.cuda.synchronize()
    return dict(LL=eng.LL.cpu().numpy(), stats=vb.host.unpack_stats(vec, K, S, D, COV),
                kernels=(_capi.last_kernel(0), _capi.last_kernel(1)))


def _default(vb, shape):
    if shape not in _default_runs:
        _default_runs[shape] = _run(vb, shape)
    return _default_runs[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(GATED_SHAPES))
def test_default_kernels(vb, shape):
    bwd, lst = MFMA[GATED_SHAPES[shape][0]][:2]
    k0, k1 = _default(vb, shape)["kernels"]
    assert k0.startswith("vbhem::%s<" % bwd) and k1.startswith("vbhem::%s<" % lst), (k0, k1)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["no_mfma_bwd", "no_bwd2", "no_mfma_list"])
@pytest.mark.parametrize("shape", list(GATED_SHAPES))
def test_switch_selects_its_kernel(vb, shape, which):
    S = GATED_SHAPES[shape][0]
    bwd, lst, no_bwd, no_list = MFMA[S]
    ref = _default(vb, shape)
    if which == "no_mfma_bwd":      # VBHEM_NO_BWD4 / _BWD12: fb_bwd2_kernel<S>, the list pass as before
        got = _run(vb, shape, **{no_bwd: 1})
        assert got["kernels"][0] == "vbhem::fb_bwd2_kernel<%d>" % S, got["kernels"]
        assert got["kernels"][1] == ref["kernels"][1]
    elif which == "no_bwd2":        # VBHEM_NO_BWD2: fb_split_kernel's backward mode
        got = _run(vb, shape, NO_BWD2=1)
        assert got["kernels"][0].startswith("vbhem::fb_split_kernel<%d, " % S), got["kernels"]
        assert got["kernels"][0].endswith(", 1>")   # kFbBackward
    else:                           # VBHEM_NO_LIST4 / _LIST12: fb_split_kernel's list mode
        got = _run(vb, shape, **{no_list: 1})
        assert got["kernels"][0] == ref["kernels"][0]
        assert got["kernels"][1].startswith("vbhem::fb_split_kernel<%d, " % S), got["kernels"]
        assert got["kernels"][1].endswith(", 2>")   # kFbList
    assert np.isfinite(ref["LL"]).all()
    err = elem_err(got["LL"], ref["LL"])
    print(shape, which, got["kernels"], "LL", err)
    assert err < RTOL_PAIRS, (shape, which, err)
    for k in ("Nj", "N1", "M", "Nr", "Y", "SC"):
        err = stat_err(got["stats"][k], ref["stats"][k])
        print(shape, which, k, err)
        assert err < 1e-9, (shape, which, k, err)
