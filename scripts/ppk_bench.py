#!/usr/bin/env python
"""Times ppk.ppk_matrix (hmm_ppk_gram_kernel) on the GPU at two shapes, T = 10:

    2,000 HMMs, K = 3, d = 2
    1,000 HMMs, K = 16, d = 8

and prints one JSON line per shape: the time of the symmetric Gram matrix (the
pairs i <= j) and HMM pairs per second, the time of the rectangular call of the set
with itself (all H^2 pairs), and the per-pair time of the numpy restatement
(tests/ppk_ref.py) on the CPU over --cpu-pairs sampled pairs, with the ratio.

Protocol: untimed symmetric launches for --settle-ms (the clocks settle), then
--windows windows that alternate the two modes; each window warms its mode up once,
then times --reps calls between two device events (the stream is synchronised on
the second).  The line reports the median window and the range.  Needs a GPU; the
Gram matrix has no CPU path.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pkgload  # noqa: E402

SHAPES = [dict(H=2000, K=3, d=2), dict(H=1000, K=16, d=8)]
T = 10


def synth(H, K, d, seed):
    """H K-state full-covariance HMMs in 8 families 3 apart, as dicts."""
    rng = np.random.default_rng(seed)
    hmms = []
    for h in range(H):
        L = rng.normal(size=(K, d, d))
        cov = L @ L.transpose(0, 2, 1) / d + 0.5 * np.eye(d)
        mean = 3.0 * (h % 8) + rng.uniform(0, 4, (K, d))
        hmms.append(dict(prior=rng.dirichlet(np.ones(K) * 2), trans=rng.dirichlet(np.ones(K) * 2, size=K),
                         pdf=[dict(mean=mean[k], cov=cov[k]) for k in range(K)]))
    return hmms


def timed(fn, reps, dev):
    fn()  # warm-up of this mode
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--reps", type=int, default=20, help="calls per window")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--settle-ms", type=float, default=600.0)
    ap.add_argument("--cpu-pairs", type=int, default=200, help="sampled pairs for the numpy restatement")
    ap.add_argument("--scale", type=float, default=1.0, help="scale H (rehearsal)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ppk_bench.py needs a GPU")
    pkgload.load()
    import ppk_ref
    from vbhem_amd import ppk
    dev = torch.device(args.device)
    for i, s in enumerate(SHAPES):
        H, K, d = max(1, int(s["H"] * args.scale)), s["K"], s["d"]
        hmms = synth(H, K, d, seed=200 + i)
        pset = ppk.PpkSet(hmms, device=dev)

        def sym():
            return ppk.ppk_matrix(pset, None, T)

        def rect():
            return ppk.ppk_matrix(pset, pset, T)

        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
            sym()
            torch.cuda.synchronize(dev)
        ts, tr = [], []
        for _ in range(args.windows):
            ms, a = timed(sym, args.reps, dev)
            ts.append(ms)
            ms, b = timed(rect, args.reps, dev)
            tr.append(ms)
        same = bool(torch.equal(torch.triu(a), torch.triu(b)))
        rng = np.random.default_rng(i)
        pick = rng.integers(0, H, (args.cpu_pairs, 2))
        t0 = time.perf_counter()
        ref = np.array([ppk_ref.elkernel(hmms[p], hmms[q], T) for p, q in pick])
        cpu_ms = (time.perf_counter() - t0) * 1e3 / max(1, len(pick))
        got = a.cpu().numpy()[pick[:, 0], pick[:, 1]]
        err = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-5 * np.abs(ref).max()))) if len(pick) else 0.0
        msym, mrect = float(np.median(ts)), float(np.median(tr))
        pairs = H * (H + 1) // 2
        print(json.dumps(dict(
            shape=dict(H=H, K=K, d=d, T=T), kernel="hmm_ppk_gram_kernel",
            sym_ms=round(msym, 4), sym_ms_range=[round(min(ts), 4), round(max(ts), 4)],
            hmm_pairs_per_s=round(pairs / (msym * 1e-3), 1),
            rect_ms=round(mrect, 4), rect_ms_range=[round(min(tr), 4), round(max(tr), 4)],
            rect_over_sym=round(mrect / msym, 3), upper_triangles_equal=same,
            numpy_ms_per_pair=round(cpu_ms, 4), gpu_us_per_pair=round(msym * 1e3 / pairs, 6),
            numpy_over_gpu=round(cpu_ms / (msym / pairs), 1), sampled_pairs=int(len(pick)),
            sampled_err=err,
            protocol=dict(settle_ms=args.settle_ms, windows=args.windows, reps=args.reps,
                          timer="device events around the calls"))), flush=True)


if __name__ == "__main__":
    main()
