#!/usr/bin/env python
"""Times base-HMM learning end to end under engine="fused" (one vbhmm_em_batch call for
every run) against engine="loop" (one vbhmm_fb launch and one synchronous copy per EM
iteration per run), at two shapes:

    (i)  the demo:  10 subjects x K = 1:3 x 50 trials (tests/golden/demo_fixations.npz),
                    vbhmm_learn_batch on both engines, and one evaluation of the
                    learn_hyps_batch objective on both engines;
    (ii) exprmt1's: --subjects seeded synthetic subjects of 25 sequences x T = 50,
                    K = 1:3 x 10 trials; the fused engine over everything, the loop
                    engine on a --loop-subjects subset, reported per run; and the fused
                    call alone at several launch chunk sizes.

The GMMs of the random trials are drawn once on the host (timed on their own: both
engines draw the same ones in the same way) and injected into both engines, so the engine
times hold the EM alone; "fused_with_gmm" adds the two, and gmm_share is the part of it
the host-side GMM fits take.  Host clock around a device synchronise, one warm-up per
engine, engines alternating within a repeat, in one process.  One JSON line per shape.
Needs a GPU.
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

DEMO_VBOPT = dict(alpha0=1.0, mu0=[160.0, 210.0], W0=0.001, beta0=1.0, v0=10.0, epsilon0=1.0, seed=100)
KS = [1, 2, 3]


def demo_subjects():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "demo_fixations.npz"))
    off, x, subj = fx["offsets"], fx["x"], fx["subject"]
    seqs = [x[off[n]:off[n + 1]] for n in range(off.size - 1)]
    return [[s for s, g in zip(seqs, subj) if g == i] for i in range(len(fx["names"]))]


def synthetic_subjects(S, nseq=25, T=50, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(S):
        mu = np.array([[100.0, 150.0], [220.0, 260.0]]) + rng.normal(0, 15.0, (2, 2))
        z = rng.integers(2, size=(nseq, T))
        out.append([mu[z[n]] + rng.normal(0, 20.0, (T, 2)) for n in range(nseq)])
    return out


def clock(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def spread(v):
    v = np.asarray(v, dtype=float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), n=int(v.size))


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def draw_gmms(em, subjects, opt):
    t0 = time.perf_counter()
    g = []
    for i, d in enumerate(subjects):
        g.append({K: em._draw_inits(d, K, opt, None) for K in KS})
        if i % 200 == 199:
            note("gmms drawn for", i + 1, "subjects")
    return time.perf_counter() - t0, g


def shape_demo(em, dev, repeats):
    subjects = demo_subjects()
    opt = em.vbhmm_default_options(2, **dict(DEMO_VBOPT, numtrials=50))
    t_gmm, gmms = draw_gmms(em, subjects, opt)
    runs = sum(len(g[K]) for g in gmms for K in KS)
    t = dict(loop=[], fused=[])
    for eng in ("loop", "fused"):  # warm-up
        em.vbhmm_learn_batch(subjects[:2], KS, opt, device=dev, gmms=gmms[:2], engine=eng)
    for _ in range(repeats):
        for eng in ("loop", "fused"):
            dt, (hm, LL) = clock(lambda: em.vbhmm_learn_batch(subjects, KS, opt, device=dev, gmms=gmms, engine=eng), dev)
            t[eng].append(dt)
    # one evaluation of the learn_hyps_batch objective
    ev = dict(loop=[], fused=[])
    val = {}
    lopt = dict(opt, numtrials=5, learn_hyps_batch=1)
    lg = [{K: g[K][:5] for K in KS} for g in gmms]
    for eng in ("loop", "fused"):
        grad, X0, _, _ = em.hyps_batch_objective(subjects, KS, lopt, device=dev, gmms=lg, engine=eng)
        grad(X0)
        for _ in range(repeats):
            dt, out = clock(lambda: grad(X0), dev)
            ev[eng].append(dt)
        val[eng] = float(out[0])
    fused = spread(t["fused"])
    return dict(shape="demo", subjects=len(subjects), runs=runs, gmm_seconds=t_gmm,
                loop_seconds=spread(t["loop"]), fused_seconds=fused,
                speedup=float(np.median(t["loop"]) / np.median(t["fused"])),
                fused_with_gmm=fused["median"] + t_gmm, gmm_share=t_gmm / (fused["median"] + t_gmm),
                hyps_batch_eval_loop=spread(ev["loop"]), hyps_batch_eval_fused=spread(ev["fused"]),
                hyps_batch_value_loop=val["loop"], hyps_batch_value_fused=val["fused"])


def shape_synthetic(em, vbhmm, dev, S, loop_S, repeats, chunks):
    subjects = synthetic_subjects(S)
    opt = em.vbhmm_default_options(2, **dict(DEMO_VBOPT, mu0=[160.0, 205.0], numtrials=10))
    t_gmm, gmms = draw_gmms(em, subjects, opt)
    runs = sum(len(g[K]) for g in gmms for K in KS)
    em.vbhmm_learn_batch(subjects[:2], KS, opt, device=dev, gmms=gmms[:2], engine="fused")
    tf = [clock(lambda: em.vbhmm_learn_batch(subjects, KS, opt, device=dev, gmms=gmms, engine="fused"), dev)[0]
          for _ in range(repeats)]
    em.vbhmm_learn_batch(subjects[:1], KS, opt, device=dev, gmms=gmms[:1], engine="loop")
    tl, _ = clock(lambda: em.vbhmm_learn_batch(subjects[:loop_S], KS, opt, device=dev, gmms=gmms[:loop_S]), dev)
    loop_runs = sum(len(g[K]) for g in gmms[:loop_S] for K in KS)
    note("engines timed; chunk sizes next")
    # the fused call alone, by launch chunk size: device seconds, and per launch
    sbt = vbhmm.SubjectBatch(subjects, 2, dev)
    rl = [(s, K, g) for s in range(S) for K in KS for g in gmms[s][K]]
    by_chunk = {}
    for c in chunks:
        tm = []
        for _ in range(repeats + 1):
            part = {}
            em.vbhmm_em_batch(sbt, rl, opt, finish=False, chunk_runs=c, timing=part)
            tm.append(part)
            note("chunk", c, part)
        dv = [p["device"] for p in tm[1:]]
        launches = -(-len(rl) // c)
        by_chunk[str(c)] = dict(device_seconds=spread(dv), launches=launches,
                                seconds_per_launch=float(np.median(dv)) / launches,
                                init_seconds=float(np.median([p["init"] for p in tm[1:]])),
                                unpack_seconds=float(np.median([p["unpack"] for p in tm[1:]])))
    fused = spread(tf)
    return dict(shape="synthetic", subjects=S, sequences=25, T=50, runs=runs, gmm_seconds=t_gmm,
                fused_seconds=fused, fused_ms_per_run=1e3 * fused["median"] / runs,
                loop_subjects=loop_S, loop_seconds=tl, loop_ms_per_run=1e3 * tl / loop_runs,
                fused_with_gmm=fused["median"] + t_gmm, gmm_share=t_gmm / (fused["median"] + t_gmm),
                by_chunk=by_chunk)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--subjects", type=int, default=2000)
    ap.add_argument("--loop-subjects", type=int, default=20)
    ap.add_argument("--chunks", type=int, nargs="*", default=[256, 1024, 4096, 16384])
    ap.add_argument("--shapes", nargs="*", default=["demo", "synthetic"])
    a = ap.parse_args()
    pkgload.load()
    from vbhem_amd import vbhmm, vbhmm_em as em
    if "demo" in a.shapes:
        print(json.dumps(shape_demo(em, a.device, a.repeats)), flush=True)
    if "synthetic" in a.shapes:
        print(json.dumps(shape_synthetic(em, vbhmm, a.device, a.subjects, min(a.loop_subjects, a.subjects),
                                         a.repeats, a.chunks)), flush=True)


if __name__ == "__main__":
    main()
