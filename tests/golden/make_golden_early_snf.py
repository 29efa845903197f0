"""Generate tests/golden/early_snf_golden.npz from the reference's own fusion code.

TEST INFRASTRUCTURE, run in the build container only (it reads the reference checkout, which does
not exist on the GPU box):

    python tests/golden/make_golden_early_snf.py

The reference's similarity_fusion.py, cross_recurrence.py and alignment_tools.py are imported by
file path with make_golden.py's stubbing (numba.jit becomes the identity). For seeded continuous
point clouds (no ties), three "features" per pair, in float64:

  cross_recurrence.get_ssm / get_csm                         the inputs: SSMA, SSMB, CSM per feature
  similarity_fusion.getWCSMSSM (K, mu = 0.5)                 :76-99   the parent affinity matrices
  similarity_fusion.doSimilarityFusionWs (K, niters, 1)      :146-186 the fused matrix
  F[:M, M:] + F[M:, :M].T                                    the cross block
  cross_recurrence.csm_to_binary(np.exp(-cross), KAPPA)      :137-161 the binary matrix
  alignment_tools.smith_waterman_constrained                 the score

Shapes (12, 12), (9, 20), (20, 9); K in {4, 10}; niters in {0, 1, 5}. Data only: inputs and
recorded results.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, _load, _stub  # noqa: E402

SHAPES = [(12, 12), (9, 20), (20, 9)]
KS = [4, 10]
NITERS = [0, 1, 5]
KAPPA = 0.25
SEED = 20261020


def main():
    _stub("numba", jit=lambda *a, **k: (lambda f: f))
    sf = _load("ref_similarity_fusion", REF + "/algorithms/utils/similarity_fusion.py")
    cr = _load("ref_cross_recurrence", REF + "/algorithms/utils/cross_recurrence.py")
    at = _load("ref_alignment_tools", REF + "/algorithms/utils/alignment_tools.py")
    rng = np.random.Generator(np.random.PCG64(SEED))
    out = {"shapes": np.array(SHAPES), "Ks": np.array(KS), "niters": np.array(NITERS), "kappa": np.array(KAPPA)}
    for s, (M, N) in enumerate(SHAPES):
        dists = []
        for f in range(3):
            # a shared drifting curve plus noise, so the cross block has diagonal structure
            t = np.linspace(0, 3 + f, max(M, N))
            base = np.stack([np.sin((d + 1) * t) + 0.3 * d for d in range(6)], 1)
            X = base[:M] + 0.2 * rng.normal(size=(M, 6))
            Y = base[:N] + 0.2 * rng.normal(size=(N, 6))
            A, B, C = cr.get_ssm(X), cr.get_ssm(Y), cr.get_csm(X, Y)
            dists.append((A, B, C))
            out["s%d_f%d_ssma" % (s, f)], out["s%d_f%d_ssmb" % (s, f)], out["s%d_f%d_csm" % (s, f)] = A, B, C
        for K in KS:
            Ws = [sf.getWCSMSSM(A, B, C, K) for A, B, C in dists]
            out["s%d_K%d_W" % (s, K)] = np.stack(Ws)
            for it in NITERS:
                F = sf.doSimilarityFusionWs([np.array(W) for W in Ws], K, it, 1)
                cross = F[:M, M:] + F[M:, :M].T
                binary = cr.csm_to_binary(np.exp(-cross), KAPPA)
                key = "s%d_K%d_it%d_" % (s, K, it)
                out[key + "F"], out[key + "cross"] = F, cross
                out[key + "binary"] = binary.astype(np.uint8)
                out[key + "score"] = np.array(float(at.smith_waterman_constrained(binary)))
    path = os.path.join(HERE, "early_snf_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
