"""Restatement of the inference for new documents with a learned SCM / MCM model (include/libcluster_hip.h,
lc_tmodel_predict), built from the oracle's vbeY / vbeZ only (scluster.cpp:50-124, mcluster.cpp:49-135).
The model objects are anything that offers Elogweight() (weights) and Eloglike(X) (clusters): the oracle's own
distributions, or stand-ins rebuilt from a learned model's accessors."""
from typing import NamedTuple

import numpy as np

import lc_oracle as o


class DocInference(NamedTuple):
    qY: np.ndarray      # (T,)   qY^R
    label_t: int        # argmax_t, lowest t on ties
    Fyz: float          # sum_t qY^R_t like_t - logZ_y of sweep R
    Fz: float           # -sum_n logZ_n of the last vbeZ
    sweeps: int         # R
    qZ: np.ndarray      # (N, K) of the last vbeZ
    logZ: np.ndarray    # (N,)
    label: np.ndarray   # (N,) argmax_k of c_k + L_nk, lowest k on ties
    margin: np.ndarray  # (N,) gap between the two largest c_k + L_nk (inf for K = 1)
    margin_t: float     # gap between the two largest qY^R_t (inf for T = 1)
    trace: list         # per sweep r: (qY^{r-1}, qY^r, delta_r)


def _vbeY(qZ, weights_j, weights_t, w, clusters_t):
    qY, Fyz = o.vbeY([qZ], weights_j, weights_t, None, w, clusters_t)
    return qY[0], Fyz


def _gap(v):
    v = np.sort(np.asarray(v, dtype=np.float64), axis=-1)
    return v[..., -1] - v[..., -2] if v.shape[-1] > 1 else np.full(v.shape[:-1], np.inf)


def row_terms(X, qY, weights_t, clusters):
    """c_k + L_nk of every row (the argument of vbeZ's softmax), (N, K)."""
    K = len(clusters)
    X = np.asarray(X, dtype=np.float64)
    E = np.zeros(K)
    for t in range(len(weights_t)):
        E = E + qY[t] * weights_t[t].Elogweight()
    if X.shape[0] == 0:
        return np.zeros((0, K))
    return np.stack([E[k] + clusters[k].Eloglike(X) for k in range(K)], axis=1)


def infer_document(X, weights_j, weights_t, clusters, max_sweeps, tol, w=None, clusters_t=None):
    """One document X (N, D) of a group with weights weights_j; w (Dt,) and clusters_t for the MCM."""
    if max_sweeps < 1:
        raise ValueError("max_sweeps must be at least 1")
    X = np.asarray(X, dtype=np.float64)
    K = len(clusters)
    mcm = clusters_t is not None and len(clusters_t) > 0
    wj = np.asarray(w, dtype=np.float64).reshape(1, -1) if mcm else None
    ct = clusters_t if mcm else None
    # qY^0 = softmax(a): vbeY of a document whose counts N_k are all zero
    qY, _ = _vbeY(np.zeros((0, K)), weights_j, weights_t, wj, ct)
    trace, Fyz, R = [], 0.0, 0
    for r in range(1, max_sweeps + 1):
        qZ, _ = o.vbeZ(X, qY, weights_t, clusters)
        new, Fyz = _vbeY(qZ, weights_j, weights_t, wj, ct)
        delta = float(np.max(np.abs(new - qY)))
        trace.append((qY, new, delta))
        qY, R = new, r
        if tol >= 0 and delta <= tol:
            break
    qZ, Fz = o.vbeZ(X, qY, weights_t, clusters)
    terms = row_terms(X, qY, weights_t, clusters)
    logZ = o.logsumexp(terms) if X.shape[0] else np.zeros(0)
    return DocInference(qY, int(np.argmax(qY)), Fyz, Fz, R, qZ, logZ, np.argmax(terms, axis=1).astype(np.int32),
                        _gap(terms), float(_gap(qY)), trace)


def document_bound(X, qY, weights_j, weights_t, clusters, w=None, clusters_t=None):
    """Fyz_i + Fz_i evaluated consistently at qY: vbeZ with qY, then the document's terms of F with THAT qY held (not
    the vbeY update): sum_t qY_t (log qY_t - a_t) + Fz.  Coordinate ascent with the model fixed does not increase it."""
    K = len(clusters)
    mcm = clusters_t is not None and len(clusters_t) > 0
    wj = np.asarray(w, dtype=np.float64).reshape(1, -1) if mcm else None
    a = np.array(weights_j.Elogweight(), dtype=np.float64).copy()
    if mcm:
        a = a + np.array([clusters_t[t].Eloglike(wj)[0] for t in range(len(clusters_t))])
    _, Fz = o.vbeZ(np.asarray(X, dtype=np.float64), qY, weights_t, clusters)
    pos = qY > 0
    return float(np.sum(qY[pos] * (np.log(qY[pos]) - a[pos]))) + Fz


class Weights:
    """Stand-in for a weight distribution: Elogweight() from lc_tmodel_weights."""

    def __init__(self, elog):
        self._e = np.asarray(elog, dtype=np.float64)

    def Elogweight(self):
        return self._e


def gauss_wish(c):
    """Stand-in for a Gauss-Wishart cluster from lc_tmodel_cluster's nu, beta, m, iW, logdW: Eloglike by
    distributions.cpp:356-370 (the formula at lc_estep_posterior)."""
    D = len(c["mean"])
    g = o.GaussWish(1.0, D)
    g.nu, g.beta, g.logdW = float(c["nu"]), float(c["beta"]), float(c["logdW"])
    g.m, g.iW = np.asarray(c["mean"], dtype=np.float64), np.asarray(c["iW"], dtype=np.float64)
    return g


def synthetic_documents(rng, J, I, n, D, K, T, Dt=0, scale=5.0, wscale=4.0):
    """J groups of I documents drawn from T document classes, each a different mixture over K Gaussian segments whose
    means are drawn at `scale` (1.5: overlapping segments, documents need different numbers of sweeps).  Returns
    (X, W, classes): W is None for Dt = 0."""
    mu = rng.normal(0, scale, (K, D))
    mix = rng.dirichlet(np.full(K, 0.4), T)
    mw = rng.normal(0, wscale, (T, max(Dt, 1)))
    X, W, cls = [], [], []
    for _ in range(J):
        Xj, Wj, cj = [], [], []
        for _ in range(I):
            t = int(rng.integers(0, T))
            nn = max(1, n + int(rng.integers(-(n // 3), n // 3 + 1)))
            z = rng.choice(K, size=nn, p=mix[t])
            Xj.append(mu[z] + rng.normal(size=(nn, D)))
            Wj.append(mw[t] + 0.7 * rng.normal(size=max(Dt, 1)))
            cj.append(t)
        X.append(Xj)
        W.append(np.array(Wj))
        cls.append(cj)
    return X, (W if Dt else None), cls


def many_segment_documents(rng, T=12, per_class=4, docs_per_class=2, n=200, D=4, scale=5.0, held_rows=90):
    """One group of T x docs_per_class documents; class t draws its rows from its own per_class unit Gaussian segments
    (means at `scale`), so a learner ends with several classes and some tens of segments: a T x K table larger than
    the inference kernel keeps in LDS, and more segments than a row keeps in registers.  Returns (X, classes, qY0,
    held): qY0 puts 0.9 on the true class, held is one further document of held_rows rows per class."""
    K = T * per_class
    mu = rng.normal(0, scale, (K, D))

    def draw(t, rows):
        z = rng.integers(0, per_class, rows) + t * per_class
        return mu[z] + rng.normal(size=(rows, D))

    X, cls = [], []
    for t in range(T):
        for _ in range(docs_per_class):
            X.append(draw(t, n))
            cls.append(t)
    q = np.full((len(X), T), 0.1 / (T - 1))
    q[np.arange(len(X)), cls] = 0.9
    return [X], cls, [q], [draw(t, held_rows) for t in range(T)]
