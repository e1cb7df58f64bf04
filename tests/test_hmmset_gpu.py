"""The prepare path that scoring and PPK share (csrc/vbhmm_hmmset.h), through the C
ABI on device tensors: a state count outside [1, KM] is an argument error that names
the lowest such HMM, and the flags it raised are consumed, so the same buffers
prepare again."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ERR_ARG = -1  # include/vbhem_estep.h VBHEM_ERR_ARG
H, KM, D = 3, 4, 2


def test_bad_state_count_is_rejected_and_consumed(vb, capi_lib):
    from vbhem_amd import _capi
    from vbhem_amd.h3m import COV_DIAG
    lib, f64 = capi_lib, torch.float64
    nstates = torch.tensor([2, 5, 0], dtype=torch.int32, device=DEV)
    prior = torch.full((H, KM), 1.0 / KM, dtype=f64, device=DEV)
    trans = torch.eye(KM, dtype=f64, device=DEV).repeat(H, 1, 1).contiguous()
    mean = torch.arange(KM, dtype=f64, device=DEV)[None, :, None].expand(H, KM, D).contiguous()
    cov = torch.ones((H, KM, D), dtype=f64, device=DEV)
    desc = _capi.ScoreHmmsT(H, KM, D, COV_DIAG, *(_capi.ptr(t) for t in (nstates, prior, trans, mean, cov)))
    st = _capi.stream(DEV)
    bufs = {}
    for name in ("score", "ppk"):
        nb = int(getattr(lib, f"vbhmm_{name}_prepared_bytes")(ctypes.byref(desc)))
        assert nb > 0
        bufs[name] = torch.empty((nb // 8,), dtype=f64, device=DEV)

    def prepare(name):
        buf = bufs[name]
        extra = (0.5, 0.45) if name == "ppk" else ()
        rc = getattr(lib, f"vbhmm_{name}_prepare")(ctypes.byref(desc), *extra, _capi.ptr(buf), buf.numel() * 8, st)
        return rc, lib.vbhem_last_error().decode()

    for name in ("score", "ppk"):
        rc, msg = prepare(name)
        print(name, rc, msg)
        assert rc == ERR_ARG
        assert "state count of HMM 1 is outside [1, KM]" in msg
    nstates.copy_(torch.tensor([2, 4, 1], dtype=torch.int32))
    for name in ("score", "ppk"):
        rc, msg = prepare(name)
        assert rc == 0, msg

    offsets = torch.tensor([0, 2, 4, 6], dtype=torch.int32, device=DEV)
    x = torch.linspace(-1.0, 2.0, 6 * D, dtype=f64, device=DEV).reshape(6, D).contiguous()
    seqs = _capi.SeqsT(3, D, 2, _capi.ptr(offsets), _capi.ptr(x))
    ll = torch.full((H, 3), float("nan"), dtype=f64, device=DEV)
    rc = lib.vbhmm_score_ll(ctypes.byref(desc), _capi.ptr(bufs["score"]), ctypes.byref(seqs), _capi.ptr(ll), st)
    assert rc == 0, lib.vbhem_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ll).all()), ll
