#!/usr/bin/env python
"""Times the DIC likelihood of a K x S grid on the GPU: dic.loglik_grid with
engine="fused" (one vbhmm_dic_loglik launch for all models) against engine="pairs" (every
model through EStepEngine.pairs(smooth=1), the log-sum-exp in torch), on the grid
K = 1:6 x S = 1:5 (30 models, 105 clusters, d = 2) at two shapes:

    the exprmt1 shape:  N = 40 subject HMMs,      Sb = 2, tau = 50
    a large set:        N = 100,000 subject HMMs, Sb = 3, tau = 10

Both engines get the same device-resident base set and the same list of models; a call
includes packing the models and uploading their constants.

One JSON line per shape.  Protocol as scripts/ccfd_bench.py: untimed calls for
--settle-ms, then --windows windows that alternate the engines; each window warms its
engine up once and times at least --reps calls, and at least --window-ms of them, by the
host clock around the calls and a final device synchronise.  The line reports the median
window and the range.  Needs a GPU.
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


def timed(fn, reps, dev):
    """Milliseconds per call by the host clock, the last call synchronised (a call packs
    and uploads on the host, so the host clock is what a user waits for)."""
    fn()  # warm-up of this variant
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / reps, out


SHAPES = [dict(N=40, Sb=2, T=50), dict(N=100000, Sb=3, T=10)]
KS, SS, DIM = range(1, 7), range(1, 6), 2


def grid_models(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for K in KS:
        for S in SS:
            out.append(dict(prior=rng.dirichlet(np.ones(S), size=K), A=rng.dirichlet(np.ones(S), size=(K, S)),
                            centres=rng.uniform(0, 5, (K, S, DIM)), covars=rng.uniform(0.5, 1.5, (K, S, DIM)),
                            omega=rng.dirichlet(np.ones(K)), scale=10.0))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=600.0)
    ap.add_argument("--window-ms", type=float, default=300.0, help="least timed work per window")
    ap.add_argument("--scale", type=float, default=1.0, help="scale N (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dic_bench.py needs a GPU")
    vb = pkgload.load()
    from vbhem_amd import dic
    dev = torch.device(args.device)
    models = grid_models()
    pk = dic.pack_models(models)
    for i, s in enumerate(SHAPES):
        N, Sb, T = max(1, int(s["N"] * args.scale)), s["Sb"], s["T"]
        base = vb.synth_base_set(N, 2, Sb, DIM, vb.COV_DIAG, seed=700 + i, device="cpu").to(dev)
        variants = {
            "fused": lambda: dic.loglik_grid(base, models, T, dev, "fused"),
            "pairs": lambda: dic.loglik_grid(base, models, T, dev, "pairs"),
        }
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            variants["fused"]()
            torch.cuda.synchronize(dev)
        reps = {k: max(args.reps, int(np.ceil(args.window_ms / timed(fn, 1, dev)[0]))) for k, fn in variants.items()}
        ms = {k: [] for k in variants}
        outs = {}
        for _ in range(args.windows):
            for k, fn in variants.items():
                t, outs[k] = timed(fn, reps[k], dev)
                ms[k].append(t)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        a, b = outs["fused"].cpu().numpy(), outs["pairs"].cpu().numpy()
        pairs_steps = N * pk["C"] * T
        line = dict(shape=dict(N=N, Sb=Sb, T=T, d=DIM, models=pk["G"], clusters=pk["C"]))
        for k in variants:
            line[k + "_ms"] = round(med[k], 4)
            line[k + "_ms_range"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        line.update(pairs_over_fused=round(med["pairs"] / med["fused"], 3),
                    fused_pair_steps_per_s=round(pairs_steps / (med["fused"] * 1e-3), 1),
                    max_rel_difference=float(np.max(np.abs(a - b) / np.abs(b))),
                    protocol=dict(settle_ms=args.settle_ms, windows=args.windows, reps=reps,
                                  timer="host clock around the calls, synchronised at the end"))
        print(json.dumps(line), flush=True)
        del base


if __name__ == "__main__":
    main()
