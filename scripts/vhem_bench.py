#!/usr/bin/env python
"""Times the fused VHEM E-step (vhem_estep_fused / vhem_estep_fused_trials) on the GPU
under both schedules (gated, dense) with inf_norm = 'nt' and '', at two shapes, T = 10:

    (a) N = 1,000, K = 4, S = 3, d = 2 (full), R = 100 trials batched in one launch
        (gated schedule only: the trials form needs it), R = 64 (the largest batch the
        VBHEM yardstick takes at K = 4) and one trial alone (both schedules)
    (b) the C4 shape: N = 100,000, K = 16, S = 8, d = 8 (full)

and prints one JSON line per (shape, trials, inf_norm): the time per E-step of each
schedule, the share of pairs that pass the w > 0 gate, and, as the yardstick, the
VBHEM fused step (vbhem_estep_fused*) at the same shape in the same process (same
recursions; the responsibilities and the gate differ).  A last line times
vhem_cluster on the planted set (vhem.planted_hmms: 2 x 20 HMMs) with the default
100 trials x 'auto'.

Protocol: untimed calls for --settle-ms, then --windows windows that alternate the
modes; each window warms its mode up once, then times --reps calls between two device
events.  The line reports the median window and the range.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pkgload  # noqa: E402

T, NV = 10, 100


def timed(fn, reps, dev):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def point_clusters(vb, base, K, S, R, seed):
    """R * K point-estimate clusters: baseem initialisations of the base set."""
    from vbhem_amd import vhem
    o = vhem.default_hemopt(K, S, seed=seed, initmode="baseem")
    hs = [vhem.initialize_hem_h3m_c(base, o, np.random.default_rng(seed + r)) for r in range(R)]
    return {k: np.concatenate([h[k] for h in hs]) for k in ("A", "prior", "centres", "covars", "omega")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=10, help="calls per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=500.0)
    ap.add_argument("--scale", type=float, default=1.0, help="scale N (rehearsal)")
    ap.add_argument("--cluster-trials", type=int, default=100)
    ap.add_argument("--skip-cluster", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vhem_bench.py needs a GPU")
    vb = pkgload.load()
    from vbhem_amd import _capi, vhem
    from vbhem_amd.estep import EStepEngine
    dev = torch.device(args.device)
    shapes = [("a", max(8, int(1000 * args.scale)), 4, 3, 3, 2, 1, (100, 64, 1)),
              ("b_C4", max(8, int(100_000 * args.scale)), 16, 8, 8, 8, 1, (1,))]
    for name, N, K, S, Sb, d, cov, Rs in shapes:
        base = vb.synth_base_set(N, K, Sb, d, cov, seed=4242, device="cpu")
        for R in Rs:
            red = point_clusters(vb, base, K, S, R, seed=11)
            eng = EStepEngine(base, R * K, S, T, device=dev, trials=R)
            ob = eng.base.omega
            Ni = (float(NV) * ob) * float(N)
            consts_vhem = vb.host.vhem_cluster_constants(red, cov)
            # the VBHEM yardstick: R baseem posteriors of the same base set
            opt = vb.default_options(K, S, d, tau=T, Nv=NV, covmode=cov, v0=max(5.0, d + 2.0))
            posts = [vb.baseem_init(base, opt, *vb.baseem_draws(base, K, S, seed=50 + r)) for r in range(R)]
            cv = [vb.host.cluster_constants(p, cov) for p in posts]
            consts_vb = {k: np.concatenate([c[k] for c in cv]) for k in ("logA", "logPi", "m", "P", "c")}
            logOm_vb = np.concatenate([vb.host.log_omega_tilde(p.alpha) for p in posts])
            for norm in ("nt", ""):
                inn = vhem.inf_norm_value(norm, T, NV, N)

                def vh_call():
                    eng.fused_vhem(Ni, ob, inn, 1.0)

                def vb_call():
                    eng.fused(Ni)

                modes = [("gated", _capi.FUSED_GATED)] + ([("dense", _capi.FUSED_DENSE)] if R == 1 else [])
                res = {}
                prev = _capi.set_fused_mode(_capi.FUSED_GATED)
                try:
                    for which, consts, lo, call in (("vhem", consts_vhem, np.log(red["omega"]), vh_call),
                                                    ("vbhem", consts_vb, logOm_vb, vb_call)):
                        eng.set_clusters(consts)
                        eng.set_log_omega(lo)
                        if which == "vbhem" and R * K > 256:   # vbhem_estep_fused_trials' limit
                            res["vbhem"] = "unsupported (R * K > 256): see the R = 64 line"
                            continue
                        t0 = time.perf_counter()
                        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
                            call()
                            torch.cuda.synchronize(dev)
                        ts = {m: [] for m, _ in modes}
                        for _ in range(args.windows):
                            for m, code in modes:
                                _capi.set_fused_mode(code)
                                ts[m].append(timed(call, args.reps, dev))
                        for m, _ in modes:
                            res[f"{which}_{m}_ms"] = round(float(np.median(ts[m])), 4)
                            res[f"{which}_{m}_ms_range"] = [round(min(ts[m]), 4), round(max(ts[m]), 4)]
                        if which == "vhem":
                            w = eng.hatZ * ob[:, None]
                            res["gate_pass_share"] = round(float((w > 0).double().mean()), 6)
                            res["vbhem_gate_would_pass"] = round(float((eng.hatZ * Ni[:, None] > 1e-8).double().mean()), 6)
                        else:
                            res["vbhem_gate_pass_share"] = round(float(
                                (eng.hatZ * Ni[:, None] > 1e-8).double().mean()), 6)
                finally:
                    _capi.set_fused_mode(prev)
                print(json.dumps(dict(shape=dict(name=name, N=N, K=K, S=S, Sb=Sb, d=d, T=T), trials=R,
                                      inf_norm=norm, **res,
                                      protocol=dict(settle_ms=args.settle_ms, windows=args.windows,
                                                    reps=args.reps, timer="device events around the calls"))),
                      flush=True)
            del eng
    if not args.skip_cluster:
        hm, lab = vhem.planted_hmms(20, seed=0)
        from vbhem_amd import evaluate
        vhem.vhem_cluster(hm, 2, 2, dict(seed=1, trials=2), device=dev)     # warm-up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = vhem.vhem_cluster(hm, 2, 2, dict(seed=3, trials=args.cluster_trials), device=dev)
        torch.cuda.synchronize(dev)
        print(json.dumps(dict(vhem_cluster=dict(hmms=len(hm), K=2, S=2, trials=args.cluster_trials,
                                                initmode="auto", seconds=round(time.perf_counter() - t0, 3),
                                                best_init=out["initmode"], LogL=out["LogL"],
                                                rand_index=float(evaluate.rand_index(out["label"], lab)[0])))),
              flush=True)


if __name__ == "__main__":
    main()
