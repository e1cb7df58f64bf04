"""The S = 8 backward kernel's tile trim on the CPU: its switch, and
the sizes it must not move.  The trim lives inside fb_bwd4_kernel -- it adds no prepared
section and no workspace region -- so the prepared operand and the fused workspace are the
sizes the shape alone gives, whatever the switch says, and their regions stay 256-byte
aligned (tests/test_workspace_layout.py holds the layout itself)."""
import ctypes

import pytest

SHAPES = [  # (N, K, S, SB, d, covmode, T)
    (100000, 16, 8, 8, 8, 1, 10),   # C4
    (12500, 16, 8, 8, 8, 1, 10),    # its shard
    (130, 3, 8, 5, 2, 1, 10),
    (1, 1, 8, 1, 2, 1, 10),
]


def sizes(lib, shape):
    from vbhem_amd import _capi
    N, K, S, SB, d, cov, T = shape
    bt = _capi.BaseT(N, SB, d, cov, None, None, None, None, None, None)
    ct = _capi.ClusterT(K, S, None, None, None, None, None)
    fn = lib.vbhem_fused_workspace_layout
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_longlong)]
    out = (ctypes.c_longlong * 5)()
    layout = int(fn(ctypes.addressof(bt), ctypes.addressof(ct), T, 1, out))
    return (int(lib.vbhem_prepare_base_bytes(ctypes.byref(bt))),
            int(lib.vbhem_fused_workspace_bytes(ctypes.byref(bt), ctypes.byref(ct), T)),
            int(lib.vbhem_pairs_workspace_bytes(ctypes.byref(bt), ctypes.byref(ct), T)),
            layout, [int(v) for v in out])


def test_switch_is_in_the_table(capi_lib):
    from vbhem_amd import _capi
    assert "VBHEM_NO_BWD4_TRIM" in _capi.switch_names()
    assert _capi.get_switch("NO_BWD4_TRIM") == 0
    with _capi.switches(NO_BWD4_TRIM=1):
        assert _capi.get_switch("VBHEM_NO_BWD4_TRIM") == 1
    assert _capi.get_switch("NO_BWD4_TRIM") == 0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_K%d_SB%d" % (s[0], s[1], s[3]))
def test_sizes_do_not_depend_on_the_switch(capi_lib, shape):
    from vbhem_amd import _capi
    ref = sizes(capi_lib, shape)
    prepared, fused, pairs, layout, (group, o_list, o_tot, o_mask, o_scratch) = ref
    assert prepared > 0 and prepared % 8 == 0
    assert fused == layout > 0 and pairs > 0
    for off in (o_list, o_tot, o_mask, o_scratch):
        assert off % 256 == 0
    with _capi.switches(NO_BWD4_TRIM=1):
        assert sizes(capi_lib, shape) == ref


def test_launch_plan_rejects_bad_arguments(capi_lib):
    fn = capi_lib.vbhem_bwd4_launch_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 3)()
    assert fn(0, 10, out) == -1
    assert fn(3, 0, out) == -1
    assert fn(3, 10, None) == -1
