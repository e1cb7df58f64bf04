"""ctypes binding of libvbhem_estep.so (include/vbhem_estep.h).

The library is built in-tree (``make lib`` / ``__graft_entry__.build()``) into
``<package>/lib/``.  torch is imported first so that the library binds to the
HIP runtime torch already loaded (both carry SONAME libamdhip64.so.7); device
buffers are torch tensors and the stream is torch's current stream.

There is no CPU fallback: if the library is missing, :func:`lib` raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import os

import torch  # noqa: F401  (must precede the CDLL: shared HIP runtime)

HERE = os.path.dirname(os.path.abspath(__file__))
# VBHEM_LIB_PATH: another build of the same library (A/B experiments)
LIB_PATH = os.environ.get("VBHEM_LIB_PATH") or os.path.join(HERE, "lib", "libvbhem_estep.so")

VBHEM_COV_DIAG, VBHEM_COV_FULL = 0, 1
_c_int, _c_size, _vp = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p


class BaseT(ctypes.Structure):
    _fields_ = [("N", _c_int), ("SB", _c_int), ("d", _c_int), ("covmode", _c_int),
                ("nstates", _vp), ("prior", _vp), ("A", _vp), ("centres", _vp), ("covars", _vp),
                ("U", _vp)]


class ClusterT(ctypes.Structure):
    _fields_ = [("K", _c_int), ("S", _c_int), ("logA", _vp), ("logPi", _vp), ("m", _vp),
                ("P", _vp), ("c", _vp)]


class PostT(ctypes.Structure):  # include/vbhem_em.h vbhem_post_t
    _fields_ = [("K", _c_int), ("S", _c_int), ("d", _c_int), ("covmode", _c_int),
                ("alpha", _vp), ("eta", _vp), ("epsilon", _vp), ("lam", _vp), ("v", _vp),
                ("m", _vp), ("W", _vp)]


class EmOptT(ctypes.Structure):  # include/vbhem_em.h vbhem_em_opt_t
    _fields_ = [("alpha0", ctypes.c_double), ("eta0", ctypes.c_double),
                ("epsilon0", ctypes.c_double), ("lambda0", ctypes.c_double),
                ("v0", ctypes.c_double), ("m0", _vp), ("W0", _vp), ("W0_len", _c_int),
                ("Nv", ctypes.c_double), ("max_iter", _c_int), ("minDiff", ctypes.c_double)]


class VhemMixTrialsT(ctypes.Structure):  # include/vhem_em.h vhem_mix_trials_t
    _fields_ = [("K", _c_int), ("S", _c_int), ("d", _c_int), ("covmode", _c_int),
                ("omega", _vp), ("prior", _vp), ("A", _vp), ("centres", _vp), ("covars", _vp),
                ("emit_vcounts", _vp)]


class VhemEmOptT(ctypes.Structure):  # include/vhem_em.h vhem_em_opt_t
    _fields_ = [("inf_norm", ctypes.c_double), ("smooth", ctypes.c_double),
                ("reg_cov", ctypes.c_double), ("termvalue", ctypes.c_double),
                ("tau", _c_int), ("max_iter", _c_int), ("min_iter", _c_int)]


class SeqsT(ctypes.Structure):  # include/vbhmm_fb.h vbhmm_seqs_t
    _fields_ = [("N", _c_int), ("dim", _c_int), ("maxT", _c_int), ("offsets", _vp), ("x", _vp)]


class HmmParamsT(ctypes.Structure):  # include/vbhmm_fb.h vbhmm_params_t
    _fields_ = [("K", _c_int), ("dim", _c_int), ("m", _vp), ("W", _vp), ("v", _vp), ("beta", _vp),
                ("logLambdaTilde", _vp), ("pz1", _vp), ("A", _vp),
                ("const_denominator", ctypes.c_double)]


class EmSubjectsT(ctypes.Structure):  # include/vbhmm_em.h vbhmm_em_subjects_t
    _fields_ = [("seqs", SeqsT), ("S", _c_int), ("seq_first", _vp), ("max_seqs", _c_int),
                ("max_obs", _c_int)]


class EmRunsT(ctypes.Structure):  # include/vbhmm_em.h vbhmm_em_runs_t
    _fields_ = [("R", _c_int), ("KM", _c_int), ("subject", _vp), ("K", _vp), ("post", _vp)]


class EmHyperT(ctypes.Structure):  # include/vbhmm_em.h vbhmm_em_hyper_t
    _fields_ = [("alpha0", ctypes.c_double), ("epsilon0", ctypes.c_double),
                ("beta0", ctypes.c_double), ("v0", ctypes.c_double),
                ("m0", ctypes.c_double * 8), ("W0inv_diag", ctypes.c_double * 8)]


class EmBatchOptT(ctypes.Structure):  # include/vbhmm_em.h vbhmm_em_opt_t
    _fields_ = [("max_iter", _c_int), ("min_diff", ctypes.c_double), ("chunk_runs", _c_int)]


class GmmFitsT(ctypes.Structure):  # include/vbhmm_gmm.h vbhmm_gmm_fits_t
    _fields_ = [("R", _c_int), ("KM", _c_int), ("subject", _vp), ("K", _vp), ("rows", _vp), ("reg", _vp)]


class GmmOptT(ctypes.Structure):  # include/vbhmm_gmm.h vbhmm_gmm_opt_t
    _fields_ = [("max_iter", _c_int), ("tolfun", ctypes.c_double), ("chunk_runs", _c_int)]


class ScoreHmmsT(ctypes.Structure):  # include/vbhmm_score.h vbhmm_score_hmms_t
    _fields_ = [("H", _c_int), ("KM", _c_int), ("dim", _c_int), ("covmode", _c_int),
                ("nstates", _vp), ("prior", _vp), ("trans", _vp), ("mean", _vp), ("cov", _vp)]


class DicModelsT(ctypes.Structure):  # include/vbhmm_dic.h vbhmm_dic_models_t
    _fields_ = [("G", _c_int), ("C", _c_int), ("S", _c_int), ("d", _c_int),
                ("max_model_clusters", _c_int), ("model_off", _vp), ("nstates_r", _vp),
                ("logw", _vp), ("scale", _vp), ("logA", _vp), ("logPi", _vp), ("m", _vp),
                ("P", _vp), ("c", _vp)]


class EmExtT(ctypes.Structure):  # include/vbhem_em.h vbhem_em_ext_t
    _fields_ = [("rccl_comm", _vp), ("iter_seconds", _vp), ("calc_deriv", _c_int), ("dLL", _vp)]


ALLREDUCE_FN = ctypes.CFUNCTYPE(_c_int, _vp, _c_size, _vp, _vp)
RCCL_ID_BYTES = 128  # include/vbhem_dist.h VBHEM_RCCL_ID_BYTES

EXPORTS = {
    "vbhem_prepare_base_bytes": (_c_size, [ctypes.POINTER(BaseT)]),
    "vbhem_prepare_base": (_c_int, [ctypes.POINTER(BaseT), _vp, _c_size, _vp]),
    "vbhem_pairs_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int]),
    "vbhem_estep_pairs": (_c_int, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vbhem_estep_pairs_host": (_c_int, [_c_int, ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int,
                                        _vp, _vp, _vp, _vp, _vp, _vp]),
    "vhem_estep_pairs": (_c_int, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int,
                                  ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _c_size, _vp]),
    "vhem_estep_pairs_host": (_c_int, [_c_int, ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT),
                                       _c_int, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vbhem_stats_nu": (_c_size, [_c_int, _c_int]),
    "vbhem_stats_len": (_c_size, [_c_int, _c_int, _c_int, _c_int]),
    "vbhem_fused_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int]),
    "vbhem_estep_fused": (_c_int, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int,
                                   _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vbhem_fused_trials_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT),
                                                     _c_int, _c_int]),
    "vbhem_estep_fused_trials": (_c_int, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int,
                                          _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vhem_fused_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int]),
    "vhem_fused_trials_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT),
                                                    _c_int, _c_int]),
    "vhem_estep_fused": (_c_int, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int,
                                  ctypes.c_double, _vp, _vp, ctypes.c_double, _vp, _vp, _vp, _vp,
                                  _vp, _c_size, _vp]),
    "vhem_estep_fused_trials": (_c_int, [ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT), _c_int,
                                         _c_int, ctypes.c_double, _vp, _vp, ctypes.c_double, _vp,
                                         _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vbhem_last_fallback_count": (_c_int, [_vp, _vp]),
    "vbhem_host_device_pointer": (_c_int, [_vp, ctypes.POINTER(_vp)]),
    "vbhem_arm_done_word": (_c_int, [_vp, ctypes.c_ulonglong]),
    "vbhem_done_word_alloc": (_c_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "vbhem_done_word_free": (_c_int, [_vp]),
    "vbhem_ctx_create": (_c_int, [_c_int, ctypes.POINTER(BaseT), _c_int, _c_int, _c_int, _c_int,
                                  ctypes.POINTER(_vp)]),
    "vbhem_ctx_fused": (_c_int, [_vp, ctypes.POINTER(ClusterT), _vp, _vp, _vp, _vp, _vp]),
    "vbhem_ctx_destroy": (None, [_vp]),
    "vbhem_estep_fused_host": (_c_int, [_c_int, ctypes.POINTER(BaseT), ctypes.POINTER(ClusterT),
                                        _c_int, _vp, _vp, _vp, _vp, _vp]),
    "vbhem_timing_enable": (_c_int, [_c_int]),
    "vbhem_timing_read": (_c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong),
                                   ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_longlong)]),
    "vbhem_timing_read_emission": (_c_int, [ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_longlong)]),
    "vbhem_timing_read_gated": (_c_int, [ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_longlong)]),
    "vbhem_timing_read_em_math": (_c_int, [ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_longlong)]),
    "vbhem_set_fused_mode": (_c_int, [_c_int]),
    "vbhem_switch_count": (_c_int, []),
    "vbhem_switch_name": (ctypes.c_char_p, [_c_int]),
    "vbhem_switch_get": (_c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]),
    "vbhem_switch_set": (_c_int, [ctypes.c_char_p, ctypes.c_longlong,
                                  ctypes.POINTER(ctypes.c_longlong)]),
    "vbhem_switch_reset": (None, []),
    "vbhem_debug_extra_lds": (_c_size, [_c_size]),
    "vbhem_em_prelude": (_c_int, [ctypes.POINTER(PostT), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vbhem_em_lower_bound": (_c_int, [ctypes.POINTER(PostT), ctypes.POINTER(EmOptT), _vp, _vp,
                                      _vp, _vp, _vp, ctypes.POINTER(ctypes.c_double)]),
    "vbhem_em_mstep": (_c_int, [ctypes.POINTER(EmOptT), _vp, ctypes.POINTER(PostT)]),
    "vbhem_em_host_iteration": (_c_int, [ctypes.POINTER(EmOptT), _vp, ctypes.POINTER(PostT), _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp,
                                         ctypes.POINTER(ctypes.c_double)]),
    "vbhem_em_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), _c_int, _c_int, _c_int]),
    "vbhem_em_run": (_c_int, [ctypes.POINTER(BaseT), _vp, _c_int, ctypes.POINTER(EmOptT),
                              ctypes.POINTER(PostT), _vp, ctypes.POINTER(_c_int),
                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_int), _vp, _vp,
                              _vp, _vp, _c_size, _vp, ALLREDUCE_FN, _vp]),
    "vbhem_em_run_ext": (_c_int, [ctypes.POINTER(BaseT), _vp, _c_int, ctypes.POINTER(EmOptT),
                                  ctypes.POINTER(PostT), _vp, ctypes.POINTER(_c_int),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_int), _vp, _vp,
                                  _vp, _vp, _c_size, _vp, ALLREDUCE_FN, _vp,
                                  ctypes.POINTER(EmExtT)]),
    "vbhem_em_trials_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), _c_int, _c_int, _c_int,
                                                  _c_int]),
    "vbhem_em_run_trials": (_c_int, [ctypes.POINTER(BaseT), _vp, _c_int, _c_int,
                                     ctypes.POINTER(EmOptT), ctypes.POINTER(PostT), _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vbhem_em_trials_hyp_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), _c_int, _c_int,
                                                      _c_int, _c_int, _c_int]),
    "vbhem_em_run_trials_hyp": (_c_int, [ctypes.POINTER(BaseT), _vp, _c_int, _c_int,
                                         ctypes.POINTER(EmOptT), _vp, ctypes.POINTER(PostT), _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vbhem_em_lower_bound_derivs": (_c_int, [ctypes.POINTER(PostT), ctypes.POINTER(EmOptT), _vp,
                                             _vp, _vp, _vp, _vp]),
    "vhem_em_trials_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), _c_int, _c_int, _c_int,
                                                 _c_int]),
    "vhem_em_run_trials": (_c_int, [ctypes.POINTER(BaseT), _vp, _vp, _c_int, _c_int,
                                    ctypes.POINTER(VhemEmOptT), ctypes.POINTER(VhemMixTrialsT),
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vbhem_hmms_to_h3m": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int] + [_vp] * 15),
    "vbhem_rccl_available": (_c_int, []),
    "vbhem_rccl_unique_id": (_c_int, [_vp]),
    "vbhem_rccl_comm_init": (_c_int, [_c_int, _c_int, _vp, _c_int, ctypes.POINTER(_vp)]),
    "vbhem_rccl_comm_destroy": (_c_int, [_vp]),
    "vbhem_rccl_allreduce_sum": (_c_int, [_vp, _vp, _c_size, _vp]),
    "vbhem_rccl_allreduce_to": (_c_int, [_vp, _vp, _c_size, _vp, _vp]),
    "vbhmm_fb_workspace_bytes": (_c_size, [ctypes.POINTER(SeqsT), _c_int]),
    "vbhmm_fb": (_c_int, [ctypes.POINTER(SeqsT), ctypes.POINTER(HmmParamsT), _vp, _vp, _vp, _vp, _vp,
                          _c_size, _vp]),
    "vbhmm_fb_host": (_c_int, [_c_int, ctypes.POINTER(SeqsT), ctypes.POINTER(HmmParamsT), _vp, _vp,
                               _vp, _vp]),
    "vbhmm_score_prepared_bytes": (_c_size, [ctypes.POINTER(ScoreHmmsT)]),
    "vbhmm_score_prepare": (_c_int, [ctypes.POINTER(ScoreHmmsT), _vp, _c_size, _vp]),
    "vbhmm_score_workspace_bytes": (_c_size, [ctypes.POINTER(ScoreHmmsT), ctypes.c_longlong]),
    "vbhmm_score_ll": (_c_int, [ctypes.POINTER(ScoreHmmsT), _vp, ctypes.POINTER(SeqsT), _vp, _vp]),
    "vbhmm_score_viterbi": (_c_int, [ctypes.POINTER(ScoreHmmsT), _vp, ctypes.POINTER(SeqsT),
                                     ctypes.c_longlong, _vp, _vp, _vp, _c_size, _vp]),
    "vbhmm_ppk_prepared_bytes": (_c_size, [ctypes.POINTER(ScoreHmmsT)]),
    "vbhmm_ppk_prepare": (_c_int, [ctypes.POINTER(ScoreHmmsT), ctypes.c_double, ctypes.c_double, _vp,
                                   _c_size, _vp]),
    "vbhmm_ppk_gram": (_c_int, [ctypes.POINTER(ScoreHmmsT), _vp, ctypes.POINTER(ScoreHmmsT), _vp,
                                _c_int, _c_int, _vp, _vp]),
    "vbhmm_ccfd_distance_workspace_bytes": (_c_size, [_c_int, ctypes.c_longlong]),
    "vbhmm_ccfd_distance": (_c_int, [ctypes.POINTER(ScoreHmmsT), _vp, ctypes.POINTER(SeqsT), _vp, _vp,
                                     _c_size, _vp, _vp, _vp, _vp]),
    "vbhmm_ccfd_rowstats": (_c_int, [_vp, _c_int, _vp, _vp, _vp]),
    "vbhmm_ccfd_rho": (_c_int, [_vp, _c_int, ctypes.POINTER(ctypes.c_double), _c_int, _vp, _vp]),
    "vbhmm_ccfd_delta": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, _vp, _vp, _vp]),
    "vbhmm_ccfd_border": (_c_int, [_vp, _c_int, ctypes.c_double, _vp, _vp, _vp, _vp]),
    "vbhmm_kld_jobs_workspace_bytes": (_c_size, [_c_int, _vp, _c_int, _vp]),
    "vbhmm_kld_jobs": (_c_int, [ctypes.POINTER(ScoreHmmsT), _vp, ctypes.POINTER(SeqsT), _c_int, _vp, _vp, _c_int,
                                _vp, _vp, _c_size, _vp, _vp]),
    "vbhmm_dic_workspace_bytes": (_c_size, [ctypes.POINTER(BaseT), ctypes.POINTER(DicModelsT), _c_int]),
    "vbhmm_dic_loglik": (_c_int, [ctypes.POINTER(BaseT), ctypes.POINTER(DicModelsT), _c_int, _vp, _vp,
                                  _vp, _c_size, _vp]),
    "vbhmm_em_post_len": (_c_size, [_c_int, _c_int]),
    "vbhmm_em_stats_len": (_c_size, [_c_int, _c_int]),
    "vbhmm_em_batch_workspace_bytes": (_c_size, [ctypes.POINTER(EmSubjectsT), _c_int, _c_int, _c_int]),
    "vbhmm_em_batch": (_c_int, [ctypes.POINTER(EmSubjectsT), ctypes.POINTER(EmRunsT),
                                ctypes.POINTER(EmHyperT), ctypes.POINTER(EmBatchOptT), _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "vbhmm_em_gamma": (_c_int, [ctypes.POINTER(EmSubjectsT), ctypes.POINTER(EmRunsT), _vp, _vp, _vp,
                                _c_int, _vp, _c_size, _vp]),
    "vbhmm_gmm_fit_workspace_bytes": (_c_size, [ctypes.POINTER(EmSubjectsT), _c_int, _c_int, _c_int]),
    "vbhmm_gmm_fit_batch": (_c_int, [ctypes.POINTER(EmSubjectsT), ctypes.POINTER(GmmFitsT),
                                     ctypes.POINTER(GmmOptT), _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     ctypes.POINTER(EmHyperT), _vp, _vp, _c_size, _vp]),
    "vbhem_wtk_cluster_workspace_bytes": (_c_size, [_c_int] * 5),
    "vbhem_wtk_cluster_batch": (_c_int, [_c_int] * 4 + [_vp] * 4 + [_c_int] + [_vp] * 5 + [_c_size, _vp]),
    "vbhem_wtk_states_workspace_bytes": (_c_size, [ctypes.c_longlong]),
    "vbhem_wtk_states_batch": (_c_int, [_c_int] * 5 + [_vp, _vp, _c_int] + [_vp] * 4 + [ctypes.c_longlong]
                               + [_vp] * 6 + [_c_size, _vp]),
    "vbhem_wtk_cluster_tiled_workspace_bytes": (_c_size, [_c_int] * 5),
    "vbhem_wtk_cluster_tiled_batch": (_c_int, [_c_int] * 4 + [_vp] * 4 + [_c_int] + [_vp] * 5 + [_c_size, _vp]),
    "vbhem_wtk_seed_tiled_workspace_bytes": (_c_size, [_c_int] * 5),
    "vbhem_wtk_seed_tiled_batch": (_c_int, [_c_int] * 4 + [_vp] * 3 + [_c_int] + [_vp] * 4 + [_c_size, _vp]),
    "vbhem_ghem_workspace_bytes": (_c_size, [_c_int] * 6),
    "vbhem_ghem_fit_batch": (_c_int, [_c_int] * 5 + [_vp, _vp, ctypes.c_double, _c_int, _vp, _vp, _vp, _c_int]
                             + [_vp] * 8 + [_c_size, _vp]),
    "vbhem_last_error": (ctypes.c_char_p, []),
    "vbhem_last_kernel": (ctypes.c_char_p, [_c_int]),
    "vbhem_version": (ctypes.c_char_p, []),
}

_LIB = None


class VbhemError(RuntimeError):
    pass


def lib():
    """Load (once) and return the CDLL; raises if the HIP library is absent."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"libvbhem_estep.so not found at {LIB_PATH}; build it with `make lib` "
                "(or __graft_entry__.build()).  There is no CPU fallback.")
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = h
    return _LIB


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().vbhem_last_error().decode(errors="replace")
        raise VbhemError(f"{what} failed (status {rc}): {msg}")


def ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def stream(device) -> ctypes.c_void_p:
    """torch's current stream on ``device``, as the C ABI's ``void *stream``."""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def workspace(nbytes: int, device, align: int = 1) -> torch.Tensor:
    """An uninitialised uint8 buffer on ``device`` for a ``*_workspace_bytes`` answer:
    ``nbytes`` long, and at least ``align`` bytes (the C ABI refuses a null workspace;
    the entries that ask for 16-byte alignment also take 16 bytes as their least size)."""
    return torch.empty((max(int(nbytes), align),), dtype=torch.uint8, device=device)


def timing_enable(on: bool = True, fb_only: bool = False) -> None:
    """Kernel timing on this thread: every timed launch, or (fb_only) the fb
    launches alone (two events per E-step)."""
    lib().vbhem_timing_enable((2 if fb_only else 1) if on else 0)


def timing_read() -> dict:
    """Summed HIP-event times of the fb/stats kernel launches since the last read."""
    fb, st = ctypes.c_double(), ctypes.c_double()
    nf, npairs, ns = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    check(lib().vbhem_timing_read(ctypes.byref(fb), ctypes.byref(nf), ctypes.byref(npairs),
                                  ctypes.byref(st), ctypes.byref(ns)), "vbhem_timing_read")
    em, ne = ctypes.c_double(), ctypes.c_longlong()
    check(lib().vbhem_timing_read_emission(ctypes.byref(em), ctypes.byref(ne)),
          "vbhem_timing_read_emission")
    gf, ng = ctypes.c_double(), ctypes.c_longlong()
    check(lib().vbhem_timing_read_gated(ctypes.byref(gf), ctypes.byref(ng)),
          "vbhem_timing_read_gated")
    mm, nm = ctypes.c_double(), ctypes.c_longlong()
    check(lib().vbhem_timing_read_em_math(ctypes.byref(mm), ctypes.byref(nm)),
          "vbhem_timing_read_em_math")
    return dict(fb_ms=fb.value, fb_launches=nf.value, fb_pairs=npairs.value,
                stats_ms=st.value, stats_launches=ns.value, em_ms=em.value, em_launches=ne.value,
                gated_fwd_ms=gf.value, gated_fwd_launches=ng.value, em_math_ms=mm.value,
                em_math_launches=nm.value)


def last_kernel(pass_: int) -> str:
    """The kernel this thread's last E-step ran for recursion pass 0 (every pair) or
    1 (the gate-list pass), as the kernel trace names it ("" before any)."""
    return lib().vbhem_last_kernel(int(pass_)).decode()


FUSED_GATED, FUSED_DENSE = 0, 1


def set_fused_mode(mode: int) -> int:
    """Fused E-step schedule (FUSED_GATED default, FUSED_DENSE); returns the previous one."""
    return int(lib().vbhem_set_fused_mode(int(mode)))


def switch_names() -> list:
    """The library's run-time switches ("VBHEM_NO_BWD4", ...)."""
    return [lib().vbhem_switch_name(i).decode() for i in range(lib().vbhem_switch_count())]


def get_switch(name: str) -> int:
    v = ctypes.c_longlong()
    check(lib().vbhem_switch_get(name.encode(), ctypes.byref(v)), "vbhem_switch_get")
    return v.value


def set_switch(name: str, value: int) -> int:
    """Set a switch (with or without the VBHEM_ prefix) for this thread; returns the
    previous value."""
    prev = ctypes.c_longlong()
    check(lib().vbhem_switch_set(name.encode(), int(value), ctypes.byref(prev)), "vbhem_switch_set")
    return prev.value


@contextlib.contextmanager
def switches(**values):
    """``with switches(NO_BWD4=1, GROUP_BASES=64): ...`` -- this thread's switches set
    inside the block, the previous values back on exit (also after an exception)."""
    prev = []
    try:
        for name, value in values.items():
            prev.append((name, set_switch(name, value)))
        yield
    finally:
        for name, value in reversed(prev):
            set_switch(name, value)
