"""loo_rows_kernel and loo_worst_kernel (lc_kernels_loo.hip) through the lcx_test_loo_rows hook of the hooks library
(bound here, as tests/test_gpu_stats_lists.py binds its own): synthetic tables, no model fit.  The reference is numpy on the same tables (the raw E-step column included, which the hook takes as an
argument); the bars are the project's own of DESIGN 4.15 / 4.15.1."""
import numpy as np
import pytest
from scipy.special import logsumexp

import aux_hooks as ah
import incomplete_ref as ref
import incomplete_var_ref as vref

pytestmark = pytest.mark.gpu

RG, GUARD = 16, 64
CANARY = -7.25e77  # (no result has this value; pad rows, pad columns and the guards keep it)


_P, _I, _L = ah._P, ah._I, ah._L
LOO_ROWS_ARGS = [_P, _I, _I, _I, _P, _L, _L, _P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _P]


def loo_rows_hook():
    fn = getattr(ah.hooks(), "lcx_test_loo_rows")
    fn.argtypes, fn.restype = LOO_ROWS_ARGS, ah.C.c_int
    return fn


def _dp(D):
    return (D + 15) // 16 * 16 if D <= 128 else (D + 63) // 64 * 64


class Case:
    """Kp random posteriors at width D; blocks: list of (rows, weights [Kp]) -> the padded device arrays and the numpy result"""

    def __init__(self, D, Kp, seed):
        rng = np.random.default_rng(seed)
        self.D, self.Kp, self.DP, self.rng = D, Kp, _dp(D), rng
        self.post = [ref.random_posterior(rng, D) for _ in range(Kp)]
        DP = self.DP
        self.mean, self.P = np.zeros((Kp, DP)), np.zeros((Kp, DP, DP))
        self.hl, self.ip = np.zeros((Kp, DP)), np.zeros((Kp, DP))
        self.s, self.e0, self.e1, self.G0, self.G1, self.gnu = (np.zeros(Kp) for _ in range(6))
        self.chol = []
        for k, (nu, beta, m, iW) in enumerate(self.post):
            P, G, s, e = ref.tables(nu, beta, iW)
            self.mean[k, :D], self.P[k, :D, :D] = m, P
            self.hl[k, :D], self.ip[k, :D] = 0.5 * np.log(np.diag(P)), 1.0 / np.diag(P)
            self.s[k], self.e0[k], self.e1[k], self.G0[k], self.G1[k] = s, e[0], e[1], G[0], G[1]
            self.gnu[k] = vref.g_table(nu, beta, D)[1] * nu
            self.chol.append(np.linalg.cholesky(iW))

    def rows(self, n):
        ks = self.rng.integers(0, self.Kp, n)
        return np.stack([self.post[k][2] + 2.0 * self.rng.normal(size=self.D) for k in ks]) if n else np.zeros((0, self.D))

    def weights(self):
        w = self.rng.random(self.Kp) + 0.05
        return w / w.sum()

    def run(self, blocks, variance=True, worst=True):
        D, DP, Kp = self.D, self.DP, self.Kp
        J = len(blocks)
        npad = [(x.shape[0] + RG - 1) // RG * RG for x, _ in blocks]
        NP = sum(npad)
        X = np.full((NP, DP), 1.5e3)  # (pad rows and pad columns hold finite junk)
        col = np.full((Kp, NP), -3.0e2)
        logp = np.full(NP, 1.0e300)
        rg, valid, grp = [], np.zeros(NP, bool), np.zeros(NP, int)
        at = 0
        for j, (x, _) in enumerate(blocks):
            n = x.shape[0]
            X[at:at + n, :D] = x
            valid[at:at + n], grp[at:at + npad[j]] = True, j
            rg += [ah_pack(j, min(RG, n - g * RG)) for g in range(npad[j] // RG)]
            at += npad[j]
        X[:, D:] = np.where(valid[:, None], 0.0, X[:, D:])  # (the context pads valid rows with zeros)
        tt1 = np.stack([np.log(w) + self.G1 for _, w in blocks])
        tt0 = np.stack([np.log(w) + self.G0 for _, w in blocks])
        Xv = X[valid][:, :D]
        d2 = np.stack([nu * np.sum(np.linalg.solve(L, (Xv - m).T) ** 2, axis=0) for (nu, _, m, _), L in zip(self.post, self.chol)])
        col[:, valid] = -0.5 * d2
        gv = grp[valid]
        logp[valid] = logsumexp(tt0[gv] - self.e0 * np.log1p(self.s * d2.T), axis=1)
        want = self.numpy_route(Xv, d2.T, tt1[gv], logp[valid])
        size = NP * DP + 2 * GUARD
        cond, cmean = np.full(size, CANARY), np.full(size, CANARY)
        var = np.full(size, CANARY) if variance else None
        wst = np.full(NP + 2 * GUARD, -77, dtype=np.int32) if worst else None
        val = np.full(NP + 2 * GUARD, CANARY) if worst else None
        rgi = np.array(rg, dtype=np.int32)
        rc = loo_rows_hook()(
            ah._p(X), DP, D, Kp, ah._p(col), NP, NP // RG, ah._p(rgi) if J > 1 else None, blocks[0][0].shape[0], J, ah._p(tt1),
            ah._p(self.s), ah._p(self.e1), ah._p(self.gnu) if variance else None, ah._p(self.mean), ah._p(self.P), ah._p(self.hl),
            ah._p(self.ip), ah._p(logp), GUARD, ah._p(cond), ah._p(cmean), ah._p(var), ah._p(wst), ah._p(val))
        assert rc == 0, rc
        out = {}
        for name, buf in (("cond", cond), ("mean", cmean), ("var", var)):
            if buf is None:
                continue
            assert np.all(buf[:GUARD] == CANARY) and np.all(buf[-GUARD:] == CANARY), name  # around the buffer
            mid = buf[GUARD:-GUARD].reshape(NP, DP)
            assert np.all(mid[~valid] == CANARY) and np.all(mid[:, D:] == CANARY), name  # pad rows, pad columns
            out[name] = mid[valid][:, :D].copy()
        if worst:
            assert np.all(wst[:GUARD] == -77) and np.all(wst[-GUARD:] == -77) and np.all(wst[GUARD:-GUARD][~valid] == -77)
            assert np.all(val[:GUARD] == CANARY) and np.all(val[-GUARD:] == CANARY) and np.all(val[GUARD:-GUARD][~valid] == CANARY)
            out["worst"], out["value"] = wst[GUARD:-GUARD][valid].copy(), val[GUARD:-GUARD][valid].copy()
        return out, want

    def numpy_route(self, X, d2, tt1, logp):
        """X (N, D), d2 (N, Kp), tt1 (N, Kp) -> dict of cond, mean, var and the scales of their bars"""
        D = self.D
        P, m = self.P[:, :D, :D], self.mean[:, :D]
        pd = np.stack([np.diag(Pk) for Pk in P])  # (Kp, D)
        V = np.einsum("nkc,kcd->nkd", X[:, None, :] - m[None], P)
        d2a = np.maximum(d2[:, :, None] - V ** 2 / pd, 0.0)
        z = self.s[None, :, None] * d2a
        t = tt1[:, :, None] - 0.5 * np.log(pd) - self.e1[None, :, None] * np.log1p(z)
        rest = logsumexp(t, axis=1)
        r = np.exp(t - rest[:, None, :])
        dl = -V / pd
        cov = self.gnu[None, :, None] * (1 + z) / pd
        dm = np.sum(r * dl, axis=1)
        var = np.sum(r * (cov + (dl - dm[:, None, :]) ** 2), axis=1)  # (centred on the mean: the reference's form)
        return {"cond": logp[:, None] - rest, "mean": X + dm, "var": var,
                "cb": np.maximum(np.abs(logp)[:, None], np.abs(rest)), "S": np.abs(X[:, None, :] + dl).max(axis=1),
                "V": (cov + (dl - dm[:, None, :]) ** 2).max(axis=1)}


def ah_pack(group, nvalid):
    return (group << 5) | nvalid  # (lck::rginfo_pack)


def _check(got, want, tag):
    rc = np.max(np.abs(got["cond"] - want["cond"]) / want["cb"])
    rm = np.max(np.abs(got["mean"] - want["mean"]) / want["S"])
    rv = np.max(np.abs(got["var"] - want["var"]) / want["V"]) if "var" in got else 0.0
    print(f"{tag}: max |device - numpy| / scale: cond {rc:.2e} (bar 1e-10), mean {rm:.2e} (1e-9), var {rv:.2e} (1e-9)")
    assert np.all(np.abs(got["cond"] - want["cond"]) <= 1e-10 * want["cb"]), rc
    assert np.all(np.abs(got["mean"] - want["mean"]) <= 1e-9 * want["S"]), rm
    if "var" in got:
        assert np.all(np.abs(got["var"] - want["var"]) <= 1e-9 * want["V"]) and np.all(got["var"] > 0), rv
    if "worst" in got:
        assert np.array_equal(got["worst"], np.argmin(got["cond"], axis=1))
        assert np.array_equal(got["value"], got["cond"].min(axis=1))


SHAPES = [(2, 1, 1), (3, 17, 2), (23, 47, 5), (64, 33, 33), (72, 16, 3), (200, 20, 65)]


@pytest.mark.parametrize("D,N,Kp", SHAPES)
def test_against_numpy(D, N, Kp):
    c = Case(D, Kp, 1700 + D)
    blocks = [(c.rows(N), c.weights())]
    got, want = c.run(blocks)
    _check(got, want, f"D = {D}, N = {N}, Kp = {Kp}")
    again, _ = c.run(blocks)  # the same bits on every run
    assert all(np.array_equal(got[k], again[k]) for k in got)
    plain, _ = c.run(blocks, variance=False)  # the instance without variance: the same cond and mean, no var
    assert "var" not in plain and np.array_equal(plain["cond"], got["cond"]) and np.array_equal(plain["mean"], got["mean"])
    assert np.array_equal(plain["worst"], got["worst"])


def test_two_blocks_with_their_own_weights():
    """5 + 20 rows: the second block starts inside the first wave's pair of row groups, and its last row group is partly
    filled; every block is scored with its own weight table"""
    c = Case(23, 4, 1801)
    blocks = [(c.rows(5), c.weights()), (c.rows(20), c.weights())]
    got, want = c.run(blocks)
    _check(got, want, "two blocks")
    for j, (x, w) in enumerate(blocks):  # ... and equals the block on its own, bit for bit
        alone, _ = c.run([(x, w)])
        lo = 0 if j == 0 else 5
        assert all(np.array_equal(alone[k], got[k][lo:lo + x.shape[0]]) for k in alone), j
    swapped, _ = c.run([(blocks[0][0], blocks[1][1]), (blocks[1][0], blocks[0][1])])
    assert not np.array_equal(swapped["cond"], got["cond"])  # (the weight tables do differ)


@pytest.mark.parametrize("D,Kp", [(5, 3), (64, 4), (72, 3)])
def test_a_row_gives_the_same_bits_wherever_it_sits(D, Kp):
    c = Case(D, Kp, 1900 + D)
    w = c.weights()
    first, other = c.rows(3), c.rows(40)
    moved = other.copy()
    moved[21] = first[0]
    a, _ = c.run([(first, w)])
    b, _ = c.run([(moved, w)])
    for k in ("cond", "mean", "var", "worst", "value"):
        assert np.array_equal(a[k][0], b[k][21]), k


def test_hook_refuses_a_missing_array():
    """nothing is launched when an array the kernel would read is missing"""
    fn = loo_rows_hook()
    z = np.zeros(16 * 16)
    assert fn(None, 16, 5, 2, ah._p(z), 16, 1, None, 4, 1, ah._p(z), ah._p(z), ah._p(z), None, ah._p(z), ah._p(z),
              ah._p(z), ah._p(z), ah._p(z), 0, ah._p(z), ah._p(z), None, None, None) == -1
