#!/usr/bin/env python
"""Times the Dunn index of a clustering on the GPU: the fused route (one
score.kld_jobs call, evaluate.dunn_index's) against the log-likelihood-matrix route
(score.ll_matrix over the centres and all members, then the same means and the same
reductions), at two shapes:

    demo-sized:  60 subjects x 20 trials of 8 observations, K = 3 centres, 3 states, d = 2
    large:       2,000 subjects x 20 trials of 8 observations, K = 4 centres, 3 states, d = 2

Clusters of equal size, cendata = all members' trials.  Both routes start from the same
prepared HmmSet (centres, then subjects), the same SequenceBatch and the same host lists
and jobs, and both end with DI on the host, so the host's packing of HMMs and trials is
in neither; the fused route's planner, upload and the read-back of the P values are in
it, and so are the matrix route's gathers and score.kld_matrix's padded segment mean
(the gathers' index tensors are built once, outside the timing).

One JSON line per shape.  Protocol as scripts/ccfd_bench.py: untimed calls for
--settle-ms, then --windows windows that alternate the two routes; each window warms its
route up once and times at least --reps calls, and at least --window-ms of them, on the
host clock around calls that end in a device synchronise.  The line reports the median
window, the range of each route, the run-to-run spread (the larger range over its
median), the peak memory rise of one call of each route, and the largest difference
between the two routes' values.  Needs a GPU.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import pkgload  # noqa: E402
from score_bench import synth  # noqa: E402

SHAPES = [dict(name="demo", H=60, per=20, K=3, S=3, d=2, T=8), dict(name="large", H=2000, per=20, K=4, S=3, d=2, T=8)]


def wall(fn, reps, dev):
    fn()  # warm-up of this route
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / reps, out


def peak_rise(fn, dev):
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return int(torch.cuda.max_memory_allocated(dev) - before)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=600.0)
    ap.add_argument("--window-ms", type=float, default=300.0, help="least timed work per window")
    ap.add_argument("--scale", type=float, default=1.0, help="scale H (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dunn_bench.py needs a GPU")
    vb = pkgload.load()
    from vbhem_amd import evaluate, score
    from vbhem_amd.vbhmm import SequenceBatch
    dev = torch.device(args.device)
    for i, s in enumerate(SHAPES):
        K, S, d, T, per = s["K"], s["S"], s["d"], s["T"], s["per"]
        H = max(K, int(s["H"] * args.scale)) // K * K
        N = H * per
        base, data = synth(vb, K + H, N, S, d, T, seed=700 + i)      # HMMs 0 .. K - 1 are the centres
        hset, batch = score.HmmSet(base, dev), SequenceBatch(data, d, dev)
        groups = [np.arange(c, H, K) for c in range(K)]
        first = np.arange(H + 1) * per
        lists, jobs = evaluate.dunn_jobs(groups, first)
        jb = np.asarray(jobs, dtype=np.int64)
        lens = np.array([len(lists[l]) for l in jb[:, 2]])
        # sequence scores of the fused route: one per (job, item), one per item of every unique (a, list)
        own_scores = sum(len(lists[l]) for _, l in {(int(a), int(l)) for a, _, l in jb})
        # the matrix route's gathers: per (job, item) the rows a, b and the column
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        row_a, row_b = t(np.repeat(jb[:, 0], lens)), t(np.repeat(jb[:, 1], lens))
        col = t(np.concatenate([lists[l] for l in jb[:, 2]]))
        counts = [int(c) for c in lens]

        def fused():
            kl = score.kld_jobs(hset, batch, lists, jb).cpu().numpy()
            return evaluate.dunn_reduce(kl, groups)

        def matrix():   # score.kld_matrix's steps: the matrix, the terms, the padded segment mean
            ll = score.ll_matrix(hset, batch, True)
            terms = ll[row_a, col] - ll[row_b, col]
            kl = score._segment_mean(terms[None, :], counts)[0]
            return evaluate.dunn_reduce(kl.cpu().numpy(), groups)

        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            fused()
            torch.cuda.synchronize(dev)
        reps = max(args.reps, int(np.ceil(args.window_ms / wall(fused, 1, dev)[0])))
        reps_m = max(args.reps, int(np.ceil(args.window_ms / wall(matrix, 1, dev)[0])))
        tf, tm, a, b = [], [], None, None
        for _ in range(args.windows):
            ms, a = wall(fused, reps, dev)
            tf.append(ms)
            ms, b = wall(matrix, reps_m, dev)
            tm.append(ms)
        mf, mm = float(np.median(tf)), float(np.median(tm))
        spread = max((max(tf) - min(tf)) / mf, (max(tm) - min(tm)) / mm)
        va = np.concatenate(a["intra"] + [a["inter_vct"]])
        vb_ = np.concatenate(b["intra"] + [b["inter_vct"]])
        line = dict(shape=dict(name=s["name"], H=H, trials=per, K=K, S=S, d=d, T=T),
                    scores=dict(fused=int(lens.sum()) + own_scores, matrix=(K + H) * N),
                    fused_ms=round(mf, 3), fused_ms_range=[round(min(tf), 3), round(max(tf), 3)],
                    matrix_ms=round(mm, 3), matrix_ms_range=[round(min(tm), 3), round(max(tm), 3)],
                    matrix_over_fused=round(mm / mf, 3), spread=round(spread, 4),
                    fused_peak_bytes=peak_rise(fused, dev), matrix_peak_bytes=peak_rise(matrix, dev),
                    DI=a["DI"], max_abs_difference_over_max=float(np.abs(va - vb_).max() / np.abs(vb_).max()),
                    protocol=dict(settle_ms=args.settle_ms, windows=args.windows, reps=[reps, reps_m],
                                  timer="host clock around calls that end in a device synchronise"))
        print(json.dumps(line), flush=True)
        del hset, batch, row_a, row_b, col


if __name__ == "__main__":
    main()
