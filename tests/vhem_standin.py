"""A CPU stand-in for EStepEngine's VHEM interface (set_clusters, set_log_omega,
fused_vhem, hatZ, LL, trials, base, device) over the oracle's per-pair E-step
(vbhem_oracle.c_vhem_estep_pairs), so that the EM loop and vhem_cluster of
vbhem_amd.vhem run without a GPU.  The responsibilities, weights and gated sums follow
include/vbhem_estep.h (vhem_estep_fused) with numpy; they are written independently of
tests/vhem_ref.py (vectorised here, MATLAB-shaped loops there)."""
import numpy as np
import torch

import vbhem_oracle as vo


class StandInEngine:
    def __init__(self, base, K, S, T, trials=1):
        self.base = base.to("cpu")
        self.bn = self.base.numpy()
        self.K, self.S, self.T, self.trials = int(K), int(S), int(T), int(trials)
        self.device = torch.device("cpu")
        self.consts = None
        self.logOmega = None
        self.hatZ = torch.zeros((self.base.N, self.K), dtype=torch.float64)
        self.LL = torch.zeros((self.base.N, self.K), dtype=torch.float64)
        self.calls = 0

    def set_clusters(self, consts):
        self.consts = {k: np.array(consts[k], dtype=np.float64) for k in ("logA", "logPi", "m", "P", "c")}

    def set_log_omega(self, lo):
        self.logOmega = np.array(lo, dtype=np.float64)

    def _red(self):
        c = self.consts
        cov = np.linalg.inv(c["P"]) if self.bn["covmode"] == 1 else 1.0 / c["P"]
        return dict(A=np.exp(c["logA"]), prior=np.exp(c["logPi"]), centres=c["m"], covars=cov)

    def fused_vhem(self, Ni, omegaB, inf_norm, smooth=1.0, out=None):
        self.calls += 1
        covmode = self.bn["covmode"]
        pr = vo.c_vhem_estep_pairs(self.bn, self._red(), self.T, smooth)
        Ni = Ni.cpu().numpy()
        ob = omegaB.cpu().numpy()
        LL = pr["LL_elbo"]
        R, KT, S = self.trials, self.K // self.trials, self.S
        d = self.bn["centres"].shape[2]
        Z = np.zeros_like(LL)
        vecs = []
        for r in range(R):
            cs = slice(r * KT, (r + 1) * KT)
            lz = self.logOmega[None, cs] + Ni[:, None] * (LL[:, cs] / inf_norm)
            mx = lz.max(1, keepdims=True)
            lse = mx[:, 0] + np.log(np.exp(lz - mx).sum(1))
            Zr = np.exp(lz - lse[:, None])
            Z[:, cs] = Zr
            w = Zr * ob[:, None]
            g = np.where(w > 0, w, 0.0)                    # [N][KT]
            N1 = np.einsum("ij,ijs->js", g, pr["sum_nu_1"][:, cs])
            M = np.einsum("ij,ijst->jst", g, pr["sum_xi"][:, cs])
            Nr = np.einsum("ij,ijs->js", g, pr["emit_pr"][:, cs])
            Y = np.einsum("ij,ijsa->jsa", g, pr["emit_mu"][:, cs])
            if covmode == 1:
                SC = np.einsum("ij,ijsab->jsab", g, pr["emit_Mu"][:, cs])
                iu = np.triu_indices(d)
                SCp = SC[..., iu[0], iu[1]]
            else:
                SCp = np.einsum("ij,ijsa->jsa", g, pr["emit_Mu"][:, cs])
            U = np.concatenate([Nr[..., None], Y, SCp], axis=-1)
            vecs.append(np.concatenate([Zr.sum(0), N1.ravel(), M.ravel(), [lse.sum(), 0.0], U.ravel()]))
        self.hatZ = torch.from_numpy(Z)
        self.LL = torch.from_numpy(LL.copy())
        return torch.from_numpy(np.concatenate(vecs))


def factory(log=None):
    def make(base, K, S, T, trials=1):
        e = StandInEngine(base, K, S, T, trials)
        if log is not None:
            log.append(e)
        return e
    return make
