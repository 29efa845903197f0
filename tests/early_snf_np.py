"""Pure-numpy restatement of the per-pair similarity network fusion of EarlyFusion ("early SNF";
the definition: include/acoss_hip.h, acoss_earlyfusion_snf) -- TEST INFRASTRUCTURE ONLY.

Everything follows the dtype of its inputs, as numpy does in the reference (float32 distances give
float32 affinities held in a float64 parent matrix; float64 distances stay float64). Two steps the
definition leaves to the implementation have a switch each, `Eval`:
  exp     "canon": oracle.canon_expf (float32 inputs only; float64 inputs always take numpy's)
          "numpy": np.exp
  rowsum  "sequential": getP's row sums add the columns one at a time in ascending order
          "pairwise": np.sum
With ("canon", "sequential") every operation is the one the HIP kernels perform, in their order:
the k smallest summed ascending, the K neighbours of both sparse products in ascending column order
from +0 with one rounded multiply and one rounded add per term.
"""
from collections import namedtuple

import numpy as np

Eval = namedtuple("Eval", "exp rowsum")
CANON = Eval("canon", "sequential")
NUMPY = Eval("numpy", "pairwise")


def split(M, N, K):
    """(k1, k2) of getWCSMSSM (similarity_fusion.py:93-94)."""
    k1 = int(K * float(M) / (M + N))
    return k1, K - k1


def pair_ok(M, N, K):
    """False where the reference raises: getW's partition needs 1 <= k <= rows - 2 (k = 0 divides by
    zero), getS's argpartition K < M + N."""
    k1, k2 = split(M, N, K)
    return 1 <= k1 <= M - 2 and 1 <= k2 <= N - 2 and K < M + N


def _exp(x, ev):
    if x.dtype == np.float32 and ev.exp == "canon":
        import oracle
        return oracle.canon_expf(x)
    return np.exp(x)


def _kmean(D, k, axis):
    """Mean of the k smallest along `axis`, added one at a time in ascending order, in D's dtype."""
    s = np.sort(D, axis=axis)
    s = s if axis == 1 else s.T
    acc = np.zeros(s.shape[0], D.dtype)
    for t in range(k):
        acc = acc + s[:, t]
    return acc / np.asarray(k, D.dtype)


def getW(D, k, mu=0.5, ev=CANON):
    """similarity_fusion.py:15-36."""
    DSym = 0.5 * (D + D.T)
    np.fill_diagonal(DSym, 0)
    MeanDist = _kmean(DSym, k + 1, 1) * float(k + 1) / float(k)
    Eps = (MeanDist[:, None] + MeanDist[None, :] + DSym) / 3
    Denom = 2 * (mu * Eps) ** 2
    Denom[Denom == 0] = 1
    return _exp(-DSym ** 2 / Denom, ev)


def getWCSM(C, k1, k2, mu=0.5, ev=CANON):
    """similarity_fusion.py:38-54."""
    Eps = (_kmean(C, k2, 1)[:, None] + _kmean(C, k1, 0)[None, :] + C) / 3
    with np.errstate(invalid="ignore", divide="ignore"):
        return _exp(-C ** 2 / (2 * (mu * Eps) ** 2), ev)


def getWCSMSSM(SSMA, SSMB, CSM, K, mu=0.5, ev=CANON):
    """similarity_fusion.py:56-99: the float64 parent matrix."""
    M, N = SSMA.shape[0], SSMB.shape[0]
    k1, k2 = split(M, N, K)
    W = np.zeros((M + N, M + N))
    W[:M, :M] = getW(SSMA, k1, mu, ev)
    WAB = getWCSM(CSM, k1, k2, mu, ev)
    W[:M, M:] = WAB
    W[M:, :M] = WAB.T
    W[M:, M:] = getW(SSMB, k2, mu, ev)
    return W


def getP(W, ev=CANON):
    if ev.rowsum == "sequential":
        rs = np.zeros(W.shape[0])
        for j in range(W.shape[1]):
            rs = rs + W[:, j]
    else:
        rs = np.sum(W, 1)
    rs[rs == 0] = 1
    return W / rs[:, None]


def getS(W, K):
    """(J, V): the K largest of each row, lowest column among equals, sorted by column, divided by
    their sum in that order."""
    J = np.sort(np.argsort(-W, axis=1, kind="stable")[:, :K], axis=1)
    V = np.take_along_axis(W, J, 1)
    sn = np.zeros(W.shape[0])
    for k in range(K):
        sn = sn + V[:, k]
    sn[sn == 0] = 1
    return J, V / sn[:, None]


def step(A, J, V, reg_diag):
    n, K = J.shape
    B = np.zeros((n, n))
    for k in range(K):
        B = B + V[None, :, k] * A[:, J[:, k]]
    out = np.zeros((n, n))
    for k in range(K):
        out = out + V[:, k, None] * B[J[:, k], :]
    if reg_diag > 0:
        out[np.arange(n), np.arange(n)] += reg_diag
    return out


def fuse(Ws, K, niters, reg_diag=1.0, ev=CANON):
    """doSimilarityFusionWs (similarity_fusion.py:146-186) with its `Pts = nextPts` aliasing."""
    Pts = [getP(W, ev) for W in Ws]
    Ss = [getS(W, K) for W in Ws]
    L = len(Pts)
    for it in range(niters):
        nxt = list(Pts) if it == 0 else Pts
        for i in range(L):
            A = np.zeros(Pts[0].shape)
            for k in range(L):
                if k != i:
                    A = A + Pts[k]
            nxt[i] = step(A / float(L - 1), Ss[i][0], Ss[i][1], reg_diag)
        Pts = nxt
    F = np.zeros(Pts[0].shape)
    for P in Pts:
        F = F + P
    return F / L


def cross_block(F, M):
    return F[:M, M:] + F[M:, :M].T


def nneighbs(kappa, ncols):
    return int(np.round(kappa * ncols)) if kappa < 1 else int(kappa)


def binarize_top(cross, kappa):
    """nn ones per row at the nn largest values, ties to the lowest column (stable argsort)."""
    if kappa == 0:
        return np.ones(cross.shape, np.uint8)
    nn = nneighbs(kappa, cross.shape[1])
    B = np.zeros(cross.shape, np.uint8)
    idx = np.argsort(-cross, axis=1, kind="stable")[:, :nn]
    np.put_along_axis(B, idx, 1, 1)
    return B


def distances(f1, f2):
    """[(SSMA, SSMB, CSM)] float32 per feature (mfccs, ssms, chromas) of two tracks' block features."""
    from oracle import np_oracle as npo
    out = []
    for key in ("mfccs", "ssms"):
        out.append((npo.get_ssm(f1[key]), npo.get_ssm(f2[key]), npo.get_csm(f1[key], f2[key])))
    c1, c2 = f1["chromas"], f2["chromas"]
    out.append((npo.get_csm_cosine(c1, c1), npo.get_csm_cosine(c2, c2),
                npo.get_csm_blocked_oti(c1, c2, f1["chroma_med"], f2["chroma_med"], npo.get_csm_cosine)))
    return [tuple(np.asarray(x, np.float32) for x in t) for t in out]


def early_snf(dists, kappa, K, niters, mu=0.5, reg_diag=1.0, ev=CANON):
    """{"W", "F", "cross", "binary", "score"} of one pair from its three (SSMA, SSMB, CSM); score and
    cross NaN (the rest None) where pair_ok is False."""
    import oracle
    M, N = dists[0][2].shape
    if not pair_ok(M, N, K):
        return {"W": None, "F": None, "cross": np.full((M, N), np.nan), "binary": None, "score": float("nan")}
    Ws = [getWCSMSSM(A, B, C, K, mu, ev) for A, B, C in dists]
    F = fuse(Ws, K, niters, reg_diag, ev)
    cross = cross_block(F, M)
    binary = binarize_top(cross, kappa)
    return {"W": Ws, "F": F, "cross": cross, "binary": binary, "score": oracle.sw_constrained(binary)}
