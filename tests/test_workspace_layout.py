"""The gate masks' place in the fused call's workspace (csrc/vbhem_estep_sched.hip carve_fused,
gate_masks_supported / gate_mask_words in csrc/vbhem_stats_plan.h), on the CPU through the
library's vbhem_fused_workspace_layout -- the carving itself lives in the library, not in a
header tests/plancheck could rebuild.

One 64-bit word per base of a group while K <= 64, none above; 256-byte aligned; clear of the
gate lists and their totals; directly before the exact fallback's scratch, which stays last (so
the buffers the hot kernels use do not move); the size the *_workspace_bytes entries report;
and independent of the switches that only choose kernels.
"""
import ctypes

import pytest

SHAPES = [  # (N, K, S, SB, d, covmode, T, R)
    (100000, 16, 8, 8, 8, 1, 10, 1),    # C4
    (12500, 16, 8, 8, 8, 1, 10, 1),     # its shard
    (1, 1, 3, 3, 2, 0, 5, 1),
    (257, 64, 5, 5, 2, 0, 10, 1),
    (257, 65, 5, 5, 2, 0, 10, 1),       # above a word: no masks
    (1030, 17, 5, 5, 2, 0, 10, 1),
    (131, 15, 3, 3, 2, 1, 5, 3),        # three trials of five clusters
    (70, 195, 2, 2, 2, 1, 4, 3),        # trials, K > 64
    (3, 33, 12, 9, 3, 1, 10, 1),
]


def align256(x):
    return (x + 255) // 256 * 256


def ask(lib, shape):
    from vbhem_amd import _capi
    N, K, S, SB, d, cov, T, R = shape
    bt = _capi.BaseT(N, SB, d, cov, None, None, None, None, None, None)
    ct = _capi.ClusterT(K, S, None, None, None, None, None)
    fn = lib.vbhem_fused_workspace_layout
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_longlong)]
    out = (ctypes.c_longlong * 5)()
    nb = fn(ctypes.addressof(bt), ctypes.addressof(ct), T, R, out)
    want = lib.vbhem_fused_trials_workspace_bytes(ctypes.byref(bt), ctypes.byref(ct), R, T)
    return int(nb), int(want), [int(v) for v in out]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_K%d_S%d_R%d" % (s[0], s[1], s[2], s[7]))
def test_mask_region(capi_lib, shape):
    N, K, S, SB, d, cov, T, R = shape
    nb, want, (group, o_list, o_tot, o_mask, o_scratch) = ask(capi_lib, shape)
    assert nb == want and nb > 0
    assert 1 <= group and min(N, group) == N      # these shapes are one base group
    assert o_list >= 0 and o_tot >= o_list + 4 * K * group and o_scratch > o_tot
    assert o_list % 256 == 0 and o_tot % 256 == 0 and o_scratch % 256 == 0
    if K > 64:
        assert o_mask == -1
        return
    assert o_mask % 256 == 0
    assert o_mask >= o_tot + 4 * K                              # clear of the lists and totals
    assert o_scratch == o_mask + align256(8 * group)            # a word per base, then the scratch
    assert o_scratch < nb


def test_bad_arguments(capi_lib):
    fn = capi_lib.vbhem_fused_workspace_layout
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_longlong)]
    assert fn(None, None, 10, 1, (ctypes.c_longlong * 5)()) == 0


def test_independent_of_kernel_switches(capi_lib):
    """The size is a function of the shape: VBHEM_NO_GATE_MASKS and VBHEM_NO_FINAL_FOLD choose
    kernels, not buffers (a workspace sized on one thread serves a call on another).  The group
    size (VBHEM_GROUP_BASES, a test switch) does move it: a word per base of the group."""
    from vbhem_amd import _capi
    shape = (1030, 17, 5, 5, 2, 0, 10, 1)
    ref = ask(capi_lib, shape)
    with _capi.switches(NO_GATE_MASKS=1, NO_FINAL_FOLD=1):
        assert ask(capi_lib, shape) == ref
    with _capi.switches(GROUP_BASES=100):
        nb, want, (group, o_list, o_tot, o_mask, o_scratch) = ask(capi_lib, shape)
        assert nb == want and group == 100
        assert o_scratch == o_mask + align256(8 * 100)
