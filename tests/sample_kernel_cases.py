"""The inputs of the launcher-level tests of the samplers (tests/test_gpu_sample_kernels.py), built without a device and held
to their conditions by tests/test_sample_exact_refs_host.py: synthetic tables, no model fit.  The exact values are
tests/sample_ref.py's; E_REF below is that reference's own error on exactly these inputs."""
import numpy as np

import sample_ref as sr

RG = 16
SEED = 0xC0FFEE11_5EED0BAD  # (the high word of the key is set)
SHAPES = [0.3, 1.0, 2.5, 250.0]
# (lc_kernels_sample.hip, lc_predict.hpp, lc_philox.hpp: compared with the sources' text by the host test)
CD_BATCH, CD_DRAWS, PC_WAVE_ROWS, PC_THREADS, DRAWS_MAX = 8, 4, 64, 256, 64

# The float64 reference against 40-digit arithmetic on the same Philox words, over every entry of the cases below, scaled by
# the magnitude of the entry's summed terms (tests/test_sample_exact_refs_host.py measures it again and holds every constant
# between 1x and 2x of what it measures).  It carries the conditioning of log, sincos (a normal near a zero of cos or sin),
# exp (its argument times 2^-53) and 1 + c x near 0.
E_REF = {"gw": 4.1e-15, "ng": 6.5e-15, "eg": 2.0e-15, "cond": 2.0e-15, "gamma": 4.2e-15}


def dp_of(D):
    """the context's padding of a row"""
    return (D + 15) // 16 * 16 if D <= 128 else (D + 63) // 64 * 64


class SampleCase:
    """tables of Kp components at width D and a layout: `blocks` = J blocks of sizes (5, 0, 37) with their own cdfs, else one
    block of NP = 40 padded rows of which 37 are valid (NP is no multiple of 16)"""

    def __init__(self, name, mode, D, Kp, blocks, row_offset, DP=None, rows=37):
        self.name, self.mode, self.D, self.Kp, self.row_offset = name, mode, D, Kp, row_offset
        self.DP = DP or dp_of(D)
        rng = np.random.default_rng(77 * mode + 1000 * D + 2 * Kp + int(blocks))
        self.shape = np.array([SHAPES[(k + D) % 4] for k in range(Kp)])
        self.loc = rng.normal(size=(Kp, D)) * 3.0
        if mode == 0:
            self.fac = rng.normal(size=(Kp, D, D)) / np.sqrt(D)  # (the strictly upper part is never read: it stays junk)
            self.fac[:, np.arange(D), np.arange(D)] = 0.5 + rng.random((Kp, D))
            if D > 128:  # wide rows: a band and every 64th column, exact zeros between them (the reference skips those products)
                i, j = np.indices((D, D))
                self.fac[:, (i >= j) & (i - j >= 6) & (j % 64 != 0)] = 0.0
        else:
            self.fac = 0.2 + rng.random((Kp, D))
        if blocks:
            self.sizes = [5, 0, 37]
            w = rng.random((3, Kp)) + 0.05
            if Kp > 2:
                w[2, -2:] = 0.0  # trailing components without weight ...
            w /= w.sum(axis=1, keepdims=True)
            self.cdf = np.cumsum(w, axis=1)
            if Kp > 2:
                self.cdf[2] *= 0.97  # ... and a short sum: rows with u above it take klast
            self.klast = np.array([Kp - 1, Kp - 1, Kp - 3 if Kp > 2 else Kp - 1], dtype=np.int32)
            npad = [(n + RG - 1) // RG * RG for n in self.sizes]
            self.goff = np.concatenate([[0], np.cumsum(npad)]).astype(np.int64)
            self.NP = int(self.goff[-1])
            self.rginfo = np.array([(j << 5) | min(RG, n - g * RG) for j, n in enumerate(self.sizes) for g in range(npad[j] // RG)],
                                   dtype=np.int32)
            self.nrows = 0
        else:
            self.sizes = [rows]
            w = rng.random((1, Kp)) + 0.05
            self.cdf = np.cumsum(w / w.sum(axis=1, keepdims=True), axis=1)
            self.cdf[:, -1] = 1.0
            self.klast = np.array([Kp - 1], dtype=np.int32)
            self.goff, self.rginfo, self.nrows = None, None, rows
            self.NP = 40 if rows == 37 else (rows + RG - 1) // RG * RG
        self.J = len(self.sizes)

    def block_rows(self):
        """(block, padded position of its first row, rows) for every block with rows"""
        at = 0
        for j, n in enumerate(self.sizes):
            if n:
                yield j, at, n
            at += (n + RG - 1) // RG * RG

    def exact(self, xp=sr.F64, first=0, count=None):
        """-> [(padded position of the first row, Exact)] per block with rows (rows [first, first + count) of a single block)"""
        out = []
        for j, at, n in self.block_rows():
            rows = np.arange(n) if count is None else np.arange(first, first + count)
            out.append((at + int(rows[0]), sr.sample_rows(self.mode, SEED, j, rows, self.cdf[j], int(self.klast[j]), self.loc, self.fac,
                                                         self.shape, self.row_offset, xp)))
        return out


OFFSETS = [0, (1 << 32) - 5, (1 << 33) + 7]  # c0 wraps into c1 inside a row group
SAMPLE_CASES = {c.name: c for c in [
    SampleCase("gw_d1", 0, 1, 1, False, OFFSETS[0]), SampleCase("gw_d2", 0, 2, 5, True, OFFSETS[1]),
    SampleCase("gw_d3_dp4", 0, 3, 5, False, OFFSETS[2], DP=4), SampleCase("gw_d23", 0, 23, 5, True, OFFSETS[0]),
    SampleCase("gw_d64", 0, 64, 1, True, OFFSETS[1]), SampleCase("gw_d65", 0, 65, 5, False, OFFSETS[1]),
    SampleCase("gw_d23_k1", 0, 23, 1, False, OFFSETS[2]),
    SampleCase("ng_d1", 1, 1, 5, True, OFFSETS[1]), SampleCase("ng_d4", 1, 4, 1, False, OFFSETS[2]),
    SampleCase("ng_d7", 1, 7, 5, False, OFFSETS[1]), SampleCase("ng_d17", 1, 17, 5, True, OFFSETS[0]),
    SampleCase("eg_d1", 2, 1, 5, False, OFFSETS[1]), SampleCase("eg_d4", 2, 4, 5, True, OFFSETS[2]),
    SampleCase("eg_d7", 2, 7, 1, True, OFFSETS[1]), SampleCase("eg_d17", 2, 17, 5, False, OFFSETS[0]),
]}
WIDE_CASE = SampleCase("gw_d520", 0, 520, 1, False, OFFSETS[1], rows=16)  # more than 64 KB of dynamic LDS
FAMILY = {0: "gw", 1: "ng", 2: "eg"}


# ---- conditional draws ---------------------------------------------------------------------------------------------------------
class CondCase:
    """synthetic tables of a conditional-draws launch and what predict_cond_kernel would have left (t_k, logp): blocks =
    [(padded rows, valid rows per row group)]"""

    def __init__(self, name, Kp, ndraws, Da, Db, fills, planted=False, past_panel=None):
        rng = np.random.default_rng(1000 * Kp + 10 * ndraws + Da + Db)
        self.name, self.Kp, self.ndraws, self.Da, self.Db = name, Kp, ndraws, Da, Db
        self.Dae, self.Dbp, self.DP = (Da + 1 + 3) // 4 * 4, (Db + 3) // 4 * 4, dp_of(Da)
        self.fills = [np.asarray(f, dtype=np.int32) for f in fills]
        self.J = len(fills)
        self.nrg = sum(f.size for f in self.fills)
        NP = self.NP = self.nrg * RG
        self.goff = np.concatenate([[0], np.cumsum([f.size * RG for f in self.fills])]).astype(np.int64)
        self.rginfo = np.concatenate([(j << 5) | f for j, f in enumerate(self.fills)]).astype(np.int32)
        self.valid = (np.arange(NP) % RG) < np.repeat(np.concatenate(self.fills), RG)
        self.block = np.repeat(np.arange(self.J), [f.size * RG for f in self.fills])
        self.X = np.full((NP, self.DP), 7.5e3)  # (pad rows hold finite junk)
        self.X[self.valid] = 0.0
        self.X[self.valid, :Da] = rng.normal(size=(int(self.valid.sum()), Da))
        self.ldq = NP + RG
        self.t = np.full((Kp, self.ldq), -3.0e2)
        self.t[:, :NP][:, self.valid] = rng.normal(size=(Kp, int(self.valid.sum()))) * 2.0
        self.pexp = np.array([[0.7, 1.0, 2.5, 11.5][(k + Da) % 4] for k in range(Kp)])
        self.cq = 0.5 + rng.random(Kp)
        self.ttab = rng.normal(size=(self.J, Kp)) + 1.0
        self.mext = np.zeros((Kp, self.Dae))
        self.mext[:, :Da] = rng.normal(size=(Kp, Da))
        self.T = rng.normal(size=(Kp, self.Dae, self.Dbp)) / np.sqrt(Da + 1)  # (rows past the ones column and pad columns: junk)
        L = np.tril(rng.normal(size=(Kp, Db, Db))) / np.sqrt(Db)
        L[:, np.arange(Db), np.arange(Db)] = 0.5 + rng.random((Kp, Db))
        self.Lt = np.full((Kp, self.Dbp, self.Dbp), 3.25e2)  # (the pads: junk)
        self.Lt[:, :Db, :Db] = np.transpose(L, (0, 2, 1))  # Lt[k][j][c] = L_k[c][j], zero for j > c
        if past_panel is not None:
            # Columns j past a panel of 64 targets add nothing to it, and cond_draws_kernel stops at the panel's end (`jend`):
            # what sits there is not read.  The launcher's contract has ZEROS there, so this pins an implementation detail, on
            # purpose: it is the only way a `jend` that runs too far shows.  A kernel that legitimately reads those zeros fails
            # the case that uses this; it then has to go, not the kernel.
            self.Lt[:, 64:Db, :64] = past_panel
        vpos = np.flatnonzero(self.valid)
        self.planted = {}
        if planted:
            assert Kp >= 5 and vpos.size >= 40
            under, short, hard = vpos[3], vpos[17], vpos[30:34]
            self.t[:, under] = -1.0e4
            self.t[2, under] = 0.25  # all but one r_k underflow to 0
            self.t[Kp - 2:, short] = -1.0e4  # the last components have no weight ...
            for p in hard:
                self.t[:, p] = -9.0e2
                self.t[(p % Kp), p] = 1.5  # every draw of the row chooses the same component
            self.planted = {"under": under, "short": short, "hard": hard}
        m = self.t[:, :NP].max(axis=0)
        self.logp = np.where(self.valid, m + np.log(np.exp(self.t[:, :NP] - m).sum(axis=0)), 1.0e300)
        if planted:
            self.logp[self.planted["short"]] += np.log(1.0e3)  # ... and the running sum stays below (nearly) every u

    def exact(self, xp=sr.F64, ndraws=None):
        """-> [(padded positions of the block's valid rows, Exact)] per block"""
        out = []
        for j in range(self.J):
            lo, hi = int(self.goff[j]), int(self.goff[j + 1])
            pos = lo + np.flatnonzero(self.valid[lo:hi])
            if pos.size == 0:
                continue
            out.append((pos, sr.cond_draws(SEED, j, pos - lo, ndraws or self.ndraws, self.X[pos, : self.Da], self.t[:, pos].T, self.logp[pos],
                                           self.ttab[j], self.pexp, self.mext, self.T, self.Lt, self.cq, self.Db, xp)))
        return out


def _fills(*blocks):
    return [list(b) for b in blocks]


COND_CASES = {c.name: c for c in [
    CondCase("k1_m1_1x1", 1, 1, 1, 1, _fills([11])),                                        # a partial wave
    CondCase("k7_m4_8x3", 7, 4, 8, 3, _fills([16, 16, 16, 16, 6])),                         # NP = 80: two waves
    CondCase("k8_m5_3x65", 8, 5, 3, 65, _fills([13]), past_panel=-4.0e3),                   # the second target panel, jend
    CondCase("k9_m64_64x2", 9, 64, 64, 2, _fills([16])),                                    # Dae = 68: the second c0 trip
    CondCase("k17_m5_8x3_blocks", 17, 5, 8, 3, _fills([16, 5, 16, 16, 0, 16, 9], [16] * 9 + [3]), planted=True),  # NP = 272: two blocks
]}
