"""Kept-quad masks of the E-step (EstepLaunch::qmask): the normalisation sweep writes, next to every
responsibility it stores, one bit per (row, cluster quad) -- "not (q < 2^-300) in any of the quad's clusters", the list
builder's rule -- and the statistics pass that follows takes its probe counts and its row lists from those bits instead of
reading qZ a third time.  Everything below is equality: the masks against the rule in numpy on the qZ of the same launch,
the emitting launch against the launch without masks, the lists and the probe counts from masks against those from qZ, a
context with the setter on against one with it off.  The hooks (lcx_test_estep_masks, lcx_test_list_build,
lcx_test_speck_probe) are bound here."""
from __future__ import annotations

import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import aux_hooks as ah
import hot_refs as hr
import lc_oracle as o
import stats_lists_ref as sl
import test_gpu_stats_lists as tl
import test_gpu_stats_speck_skip as sk

pytestmark = pytest.mark.gpu

TAU = 2.0 ** -300
SENT = -7.25e300
MSENT = 0xABCD
HOOKED = str(ah.HOOKS_LIB)
#          DC  K     three row groups per wave (K = 32, 30); four, log q~ in LDS (K = 13, 20)
SHAPES = [(64, 32), (56, 30), (64, 13), (64, 20)]
NROWS = 3 * 192 + 37  # three full blocks of the three-row-group instances and a ragged one
R = 24.0              # distance of a cluster's mean from the origin: exp(-R^2) is a speck, not zero


def _bind(name, args):
    fn = getattr(ah.hooks(), name)
    fn.argtypes = args
    fn.restype = C.c_int
    return fn


def estep_hook():
    v, i, l = C.c_void_p, C.c_int, C.c_longlong
    return _bind("lcx_test_estep_masks", [v, i, i, l, v, v, i, v, l, i, v, i, l, v, l, v, l, v, l, v])


def build_hook():
    v, i, l = C.c_void_p, C.c_int, C.c_longlong
    return _bind("lcx_test_list_build", [i, v, i, l, i, l, v, l, v, v, l, v, l])


def probe_hook():
    v, i, l = C.c_void_p, C.c_int, C.c_longlong
    return _bind("lcx_test_speck_probe", [i, v, l, i, l, v, v])


def mask_rule(q):
    """[K x NP] responsibilities -> [quads x NP / 16] uint16 words: bit i of word (c, g) = row 16 g + i keeps quad c"""
    kept = sl.kept_rows(q)
    nq, NP = kept.shape
    bits = kept.reshape(nq, NP // 16, 16).astype(np.uint32)
    return (bits << np.arange(16, dtype=np.uint32)).sum(axis=2).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def problem(DC, K, groups):
    """Unit whiteners, means R e_k.  Valid rows 0 ... 95 sit on a cluster (two whole waves of hard rows: s = 1, logZ == mx);
    rows 200 ... 263 at the origin (soft in every quad); of the others, by row index mod 4: on a cluster; on a cluster; half
    way between two clusters of one quad; half way between clusters of two quads.  Row 5 holds a NaN.  groups = 2: 300 + 313
    rows, so four pad rows sit inside; either way a last row group of pad rows alone.  Checked on the CPU before the GPU
    sees it (lc_oracle.logsumexp): rows with logZ == mx and rows without, responsibilities below 2^-300 and not below."""
    D = DC - 3
    rng = np.random.default_rng(1000 * DC + 10 * K + groups)
    counts = [300, NROWS - 300] if groups == 2 else [NROWS]
    valid, grp = ah.valid_rows(counts), ah.group_of_rows(counts)
    rginfo = np.concatenate([ah.rginfo_of(counts), [((groups - 1) << 5) | 0]]).astype(np.int32)
    valid, grp = np.concatenate([valid, np.zeros(16, bool)]), np.concatenate([grp, np.full(16, groups - 1)])
    NP = valid.size
    M = np.zeros((K, D))
    M[np.arange(K), np.arange(K)] = R
    X = np.zeros((NP, 64))
    for i, n in enumerate(np.flatnonzero(valid)):
        a = (7 * i) % K
        if 200 <= i < 264:
            x = np.zeros(D)
        elif i < 96 or i % 4 < 2:
            x = M[a]
        elif i % 4 == 2:
            a -= a % 4
            a -= 4 if a + 1 >= K else 0
            x = 0.5 * (M[a] + M[a + 1])
        else:
            x = 0.5 * (M[a] + M[(a + 4) % (K - K % 4)])
        X[n, :D] = x + 0.01 * rng.normal(size=D)
    nanrow = int(np.flatnonzero(valid)[5])
    X[nanrow, 3] = np.nan
    A = np.broadcast_to(np.eye(D), (K, D, D)).copy()
    ctab = rng.uniform(-0.1, 0.1, size=(groups, K))
    params = hr.pack_params(A, M, 64, DC)
    # ---- the construction holds what it is meant to hold ----
    Au, bneg = hr.unpack_params(params, 64, DC)
    lq = hr.estep_ref(X, Au, bneg, ctab, grp)[0].astype(np.float64)
    rows = valid & ~np.isnan(lq).any(axis=0)
    lz, mx = o.logsumexp(lq[:, rows].T), lq[:, rows].max(axis=0)
    assert (lz == mx).sum() >= 90 and (lz != mx).sum() >= 64, ((lz == mx).sum(), (lz != mx).sum())
    q = np.exp(lq[:, rows] - lz)
    assert ((q > 0) & (q < TAU)).any() and (q >= TAU).any()
    kept = sl.kept_rows(q)
    assert (kept.sum(axis=0) == 1).any() and (kept.sum(axis=0) == 2).any() and kept.all(axis=0).any()
    return dict(DC=DC, K=K, X=X, params=params, ctab=ctab, rginfo=rginfo if groups == 2 else None, nrows=NROWS if groups == 1 else 0,
                valid=valid, nanrow=nanrow, NP=NP)


def run_estep(p, masks, ll):
    """-> status, emits, qZ [K + 1 x NP] (a guard row), F_z partials, LL_k partials or None, mask words [quads x nrg] + guard"""
    K, NP = p["K"], p["NP"]
    nrg, nq = NP // 16, (K + 3) // 4
    plan = ah.estep_plan(64, p["DC"], K, nrg)
    assert plan["ok"] and plan["pstride"] == p["params"].shape[1]
    qZ = np.full((K + 1, NP), SENT)
    fz = np.full(plan["grid"] + 2, SENT)
    llp = np.full(plan["grid"] * K + 3, SENT) if ll else None
    qm = np.full(nq * nrg + 8, MSENT, dtype=np.uint16)
    emits = C.c_int(-1)
    X, pr, ct = (np.ascontiguousarray(p[k], dtype=np.float64) for k in ("X", "params", "ctab"))
    rg = p["rginfo"]
    rc = estep_hook()(X.ctypes.data, 64, p["DC"], nrg, pr.ctypes.data, ct.ctypes.data, ct.shape[0], None if rg is None else rg.ctypes.data,
                      p["nrows"], K, qZ.ctypes.data, K + 1, NP, fz.ctypes.data, fz.size, None if llp is None else llp.ctypes.data,
                      0 if llp is None else llp.size, qm.ctypes.data if masks else None, qm.size if masks else 0, C.addressof(emits))
    return rc, emits.value, qZ, fz, llp, qm


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("DC,K", SHAPES)
def test_masks_are_the_rule(DC, K, groups):
    """The words the sweep wrote equal the rule on the qZ that came back from the same launch.  A row of NaNs is in every
    quad.  Pad rows (inside, at the end, a
    whole row group of them) are in no quad, every other row in at least one, nothing is written behind the last word."""
    p = problem(DC, K, groups)
    for ll in (False, True):
        rc, emits, qZ, fz, llp, qm = run_estep(p, True, ll)
        assert rc == 0 and emits == 1, (rc, emits)
        q = qZ[:K]
        nq, nrg = (K + 3) // 4, p["NP"] // 16
        assert np.all(qZ[K] == SENT) and np.all(qm[nq * nrg:] == MSENT), "a guard was written"
        words = qm[:nq * nrg].reshape(nq, nrg)
        assert np.array_equal(words, mask_rule(q)), np.argwhere(words != mask_rule(q))[:8]
        bit = (words[:, np.arange(p["NP"]) // 16] >> (np.arange(p["NP"]) % 16)) & 1  # [quads x NP]
        # The row whose X holds a NaN: its log q~ are NaN.  Four row groups per wave without ll_part (one exponential per
        # entry, q = e / sum): e = 0 everywhere, 0 * (1 / 0) = NaN is stored, and the row is in every quad.  The other
        # sweeps take exp_nonpos(log q~ - logZ), whose fmax(x, -750) drops a NaN: they have always stored 0.0 there (the test
        # below compares with the launch without masks), and the row is in no quad.  Either way the masks follow what is
        # stored; the two list builders and the two probes below see NaNs on every shape.
        if K <= 21 and not ll:
            assert np.isnan(q[:, p["nanrow"]]).all() and bit[:, p["nanrow"]].all()
        else:
            assert np.all(q[:, p["nanrow"]] == 0.0) and not bit[:, p["nanrow"]].any()
        assert not bit[:, ~p["valid"]].any() and not words[:, -1].any() and np.all(q[:, ~p["valid"]] == 0.0)
        ok = p["valid"].copy()
        # (four row groups per wave: the selector chain that hands a lane its row group's distance multiplies the NaN by
        #  zero for the three rows 16, 32 and 48 further on, which share its lanes -- they are NaN rows too, as ever)
        ok[p["nanrow"]:p["nanrow"] + (64 if K <= 21 else 16):16] = False
        assert (bit[:, ok].sum(axis=0) >= 1).all() and (bit.sum(axis=0) == 1).sum() >= 90


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("DC,K", SHAPES)
def test_the_sweep_stores_the_same_bits_with_and_without_masks(DC, K, groups):
    """qZ and the F_z partials of the emitting launch equal those of the launch with qmask == nullptr bit for bit -- hard
    rows, soft rows, mixed waves --, with ll_part the LL_k partials as well."""
    p = problem(DC, K, groups)
    for ll in (False, True):
        a, b = run_estep(p, True, ll), run_estep(p, False, ll)
        assert a[0] == 0 and b[0] == 0 and np.all(b[5] == MSENT)
        assert sk.same_bits(a[2], b[2]) and sk.same_bits(a[3], b[3])
        if ll:
            assert sk.same_bits(a[4], b[4]) and not np.all(a[4] == SENT)


@pytest.mark.parametrize("DP,DC,K", [(96, 96, 32), (32, 32, 20), (192, 192, 16)])
def test_a_width_without_an_emitting_instance_refuses_the_pointer(DP, DC, K):
    """hipErrorInvalidValue from launch_estep, nothing written"""
    out = np.full(8, -7, dtype=np.int64)
    assert ah.hooks().lc_test_estep_plan(DP, DC, K, 0, 0, 40, out.ctypes.data) == 0 and out[0] == 1
    rng = np.random.default_rng(DP)
    X, params, ctab = np.zeros((640, DP)), np.zeros((K, out[7])), rng.normal(size=(1, K))
    nq = (K + 3) // 4
    qZ, fz, qm = np.full((K, 640), SENT), np.full(int(out[2]) + 2, SENT), np.full(nq * 40, MSENT, dtype=np.uint16)
    emits = C.c_int(-1)
    rc = estep_hook()(X.ctypes.data, DP, DC, 40, params.ctypes.data, ctab.ctypes.data, 1, None, 600, K, qZ.ctypes.data, K, 640,
                      fz.ctypes.data, fz.size, None, 0, qm.ctypes.data, qm.size, C.addressof(emits))
    assert rc == ah.HIP_ERROR_INVALID_VALUE and emits.value == 0
    assert np.all(qZ == SENT) and np.all(fz == SENT) and np.all(qm == MSENT)


def build_lists(which, q, DC, K, masks, chunk_rows=0):
    q = np.ascontiguousarray(q, dtype=np.float64)
    NP = q.shape[1]
    out = np.full(2, -7, dtype=np.int64)
    plan = ah.suffstat_plan(64, DC, NP, K, "dense")
    nch, cr = (plan["nchunks"], plan["chunk_rows"]) if chunk_rows == 0 else (-(-NP // chunk_rows), chunk_rows)
    nq = (K + 3) // 4
    lens = np.full(nch * nq, -7, dtype=np.int32)
    ent = np.full(nch * nq * cr, -7, dtype=np.int32)
    masks = np.ascontiguousarray(masks, dtype=np.uint16)
    rc = build_hook()(which, q.ctypes.data, DC, NP, K, NP, masks.ctypes.data, chunk_rows, out.ctypes.data, lens.ctypes.data, lens.size,
                      ent.ctypes.data, ent.size)
    assert rc == 0 and (out[0], out[1]) == (nch, cr), (rc, out)
    return lens.reshape(nch, nq), ent.reshape(nch, nq, cr)


@pytest.mark.parametrize("chunk_rows", [0, 100])
@pytest.mark.parametrize("DC,K", [s for s in SHAPES if s[1] != 13])  # (K = 13 at D = 64 is the few-cluster kernel's: no list route)
def test_lists_from_masks_are_the_lists_from_qz(DC, K, chunk_rows):
    """launch_suffstat_list_build_masks against launch_suffstat_list_build on the same qZ (hard, mixed and soft rows, a NaN, a
    value of exactly 2^-300 and the next one below): lengths and entries equal, and equal to the numpy rule.  Three chunks or
    more; chunk_rows = 100: chunk boundaries that are no multiple of 16, so a thread's sixteen bits come out of two words."""
    NP = tl.np3(DC, K) if chunk_rows == 0 else 320
    rng = np.random.default_rng(DC + K + NP)
    hard = sk.hard_q(rng, K, NP)
    hard[4, 10], hard[5, 21], hard[6, 33] = TAU, np.nextafter(TAU, 0.0), np.nan
    soft = rng.dirichlet(np.full(K, 0.3), NP).T.copy()
    soft[:, NP - 3:] = 0.0
    for name, q in (("hard", hard), ("mixed", tl.mixed_q(rng, K, NP)), ("soft", soft)):
        words = mask_rule(q)
        la, ea = build_lists(0, q, DC, K, words, chunk_rows)
        lb, eb = build_lists(1, q, DC, K, words, chunk_rows)
        assert la.shape[0] >= 3 and np.array_equal(la, lb) and np.array_equal(ea, eb), name
        rl, rlists = sl.list_rule(q, la.shape[0], ea.shape[2])
        assert np.array_equal(lb, rl)
        for i in range(la.shape[0]):
            for c in range(la.shape[1]):
                assert np.array_equal(eb[i, c, :rl[i, c]], rlists[i][c]) and np.all(eb[i, c, rl[i, c]:] == -7), (name, i, c)


@pytest.mark.parametrize("K", [32, 20, 13])
def test_probe_counts_from_masks_are_those_from_qz(K):
    """N = 8192: launch_speck_probe_masks returns the two counts, the pairs and the rows of launch_speck_probe on the hard,
    mixed, soft, quarter and less constructions of tests/test_gpu_stats_lists.py."""
    N = 8192
    rng = np.random.default_rng(99 + K)
    soft = rng.dirichlet(np.full(K, 0.3), N).T.copy()
    hard = 2.0 ** -rng.uniform(301.0, 1000.0, size=(K, N))
    hard[np.arange(N) % K, np.arange(N)] = 1.0
    quarter = soft.copy()
    quarter[:8] = 0.0
    less = quarter.copy()
    less[0, 0] = 0.5
    seen = set()
    for name, q in (("hard", hard), ("mixed", tl.mixed_q(rng, K, N)), ("soft", soft), ("quarter", quarter), ("less", less)):
        q = np.ascontiguousarray(q)
        words = np.ascontiguousarray(mask_rule(q))
        outs = []
        for which in (0, 1):
            out = np.full(4, -7, dtype=np.int64)
            assert probe_hook()(which, q.ctypes.data, N, K, N, words.ctypes.data, out.ctypes.data) == 0
            outs.append(out)
        assert np.array_equal(outs[0], outs[1]) and outs[0][2] == 2048 * ((K + 3) // 4) and outs[0][3] == N, (name, outs)
        seen.add((int(outs[0][0]), int(outs[0][1])))
    assert len(seen) >= 3  # (the constructions really differ in what the probe sees)


@pytest.mark.parametrize("K", [32, 20])
def test_context_builds_its_lists_from_masks_with_the_same_bits(K):
    """N = 8192, D = 64, bench.py's separated mixture from smoothed labels, three fixed VBEM iterations: with the setter on the
    list passes are built from masks, with it off none is; F trace, cluster posteriors, weights and qZ are equal bit for bit."""
    sys.path.insert(0, str(ah.ROOT))
    import bench
    from libcluster_amd import capi

    N, D = 8192, 64
    assert ah.suffstat_plan(64, 64, N, K, "dense")["route"] == "feat"
    mu, L = bench.mixture(D, K, 1004)
    res = []
    for on in (True, False):
        with capi.Context(0) as ctx:
            ctx.set_estep_masks(on)
            ctx.synth(N, D, K, mu, L, 1004, 0, 0.9)
            F, tr, mdl = ctx.vbem(capi.W_DIRICHLET, fixed_iters=3)
            cl = [mdl.cluster(k) for k in range(K)]
            lists, masks = ctx.speck_list_passes(), ctx.speck_mask_passes()
            print(f"K={K} masks {'on' if on else 'off'}: speck passes {ctx.speck_passes()}, list passes {lists}, built from masks {masks}")
            assert lists >= 1 and masks == (lists if on else 0), (on, lists, masks)
            res.append((np.array([F]), tr, np.concatenate(mdl.weights(0)), ctx.get_qz([N])[0], cl))
            mdl.close()
    a, b = res
    for u, v in zip(a[:4], b[:4]):
        assert u.shape == v.shape and sk.same_bits(u, v)
    for ca, cb in zip(a[4], b[4]):
        for key in ca:
            assert sk.same_bits(np.asarray(ca[key], dtype=np.float64), np.asarray(cb[key], dtype=np.float64)), key


_CHILD = r"""
import sys, json
sys.path.insert(0, {root!r})
import numpy as np
import bench
from libcluster_amd import capi
N, D, K = 8192, 64, 32
what = {what!r}
out = {{}}
def counters(ctx):
    return [ctx.speck_list_passes(), ctx.speck_mask_passes()]
if what.startswith("cluster"):
    # 20 separated clusters: from K = 17 on the statistics are the feature GEMM's and the hard passes take the list route
    mu, L = bench.mixture(D, 20, 1005)
    with capi.Context(0) as ctx:
        ctx.set_estep_masks(what != "cluster_off")
        ctx.synth(N, D, 20, mu, L, 1005, 0, 1.0)
        F, mdl = ctx.cluster(capi.W_DIRICHLET)
        out["cluster"] = counters(ctx) + [mdl.dims()[1], float(F).hex()]
        mdl.close()
else:
    empty = 4 if what == "prune" else 0  # prune: the first four clusters own nothing, prune_clusters moves every other column
    mu, L = bench.mixture(D, K - empty, 1004)
    with capi.Context(0) as ctx:
        ctx.synth(N, D, K - empty, mu, L, 1004, 0, 0.9)
        if empty:
            ctx.set_qz(np.hstack([np.zeros((N, empty)), ctx.get_qz([N])[0]]))
        F, tr, mdl = ctx.vbem(capi.W_DIRICHLET, fixed_iters=3)
        out["vbem"] = counters(ctx)
        q = ctx.get_qz([N])[0]
        if what == "set_qz":
            ctx.set_qz(np.roll(q, 1, axis=1))  # hard rows again, every row with another owner: stale masks would be wrong ones
        elif what == "fill_qz":
            ctx.fill_qz(K, 1.0 / K)
        elif what == "prune":
            out["removed"] = ctx.prune(mdl)
        mdl.close()
        ctx.suffstat()
        out["after"] = counters(ctx)
        out["K"] = ctx.dims()[3]
print("RESULT " + json.dumps(out))
"""


def _child(what, env):
    e = dict(os.environ, LC_LIB_PATH=HOOKED, **env)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=str(ah.ROOT), what=what)], capture_output=True, text=True, timeout=300,
                       env=e, cwd=str(ah.ROOT))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    return r, json.loads(line[-1][7:]) if line else None


STALE = "mask words are not those of qZ"


@pytest.mark.parametrize("what", ["set_qz", "fill_qz", "prune"])
def test_a_foreign_write_withdraws_the_masks(what):
    """Test-hooks library.  Three VBEM iterations leave valid masks of hard rows; then one foreign writer of qZ -- set_qz,
    fill_qz, or prune_clusters taking four empty columns out in front of the others (qz_keep_columns) -- and a statistics pass.  With LC_TEST_VERIFY_QMASK (the masks a pass is about
    to trust are recomputed from qZ by the rule, a difference throws) the run passes and that pass is not built from masks.
    With LC_TEST_QMASK_KEEP_STALE as well the writer "forgets" to withdraw them (and the pass which K they were for): the
    pass must throw."""
    r, out = _child(what, {"LC_TEST_VERIFY_QMASK": "1"})
    assert r.returncode == 0 and out, r.stdout[-2000:] + r.stderr[-2000:]
    print(what, out, r.stderr.count("[masks] verified"))
    lists, masks = out["vbem"]
    assert masks == lists >= 1 and r.stderr.count("[masks] verified") >= 2
    assert out["after"][1] == masks, out  # not mask-built
    if what == "set_qz":
        assert out["after"][0] == lists + 1  # (hard rows: a list pass, built from qZ)
    if what == "prune":
        assert out["removed"] == 4 and out["K"] == 28 and out["after"][0] == lists + 1
    bad, _ = _child(what, {"LC_TEST_VERIFY_QMASK": "1", "LC_TEST_QMASK_KEEP_STALE": "1"})
    assert bad.returncode != 0 and STALE in bad.stderr, bad.stderr[-1500:]


def test_model_selection_keeps_the_masks_honest():
    """cluster() to 20 clusters at N = 8192 with ordinary E-steps (LC_SPLIT_NO_DCACHE: Context::estep, which emits) and
    LC_TEST_VERIFY_QMASK: between the VBEM runs stand qz_clone_to_alt / qz_swap_alt, the sub-problems' gathers, qz_split_from
    and qz_keep_columns.  From K = 17 on the hard passes are list passes built from masks, every one verified; K and F equal
    those of the run with the setter off.  With LC_TEST_QMASK_KEEP_STALE the first pass behind a split throws.  The default
    schedule (E-steps from the distance cache, which never emit: estep_cache withdraws the masks through ensure_qz) passes the
    check too."""
    env = {"LC_TEST_VERIFY_QMASK": "1", "LC_SPLIT_NO_DCACHE": "1"}
    r, out = _child("cluster", env)
    assert r.returncode == 0 and out, r.stdout[-2000:] + r.stderr[-2000:]
    off, out_off = _child("cluster_off", env)
    assert off.returncode == 0 and out_off, off.stderr[-2000:]
    nver = r.stderr.count("[masks] verified")
    print(out, out_off, nver)
    lists, masks, K, F = out["cluster"]
    assert K >= 18 and masks >= 1 and nver >= masks and lists >= masks
    assert out_off["cluster"][1] == 0 and out_off["cluster"][2:] == [K, F] and out_off["cluster"][0] == lists
    bad, _ = _child("cluster", dict(env, LC_TEST_QMASK_KEEP_STALE="1"))
    assert bad.returncode != 0 and STALE in bad.stderr, bad.stderr[-1500:]
    dflt, out_d = _child("cluster", {"LC_TEST_VERIFY_QMASK": "1"})
    assert dflt.returncode == 0 and out_d and out_d["cluster"][2] == K, dflt.stderr[-1500:]
