"""Inference for new documents with a learned SCM / MCM model on the device (lc_tmodel_predict).

Every model is learned on the GPU (return_model=True); the reference is tests/topic_infer_ref.py (the oracle's vbeY / vbeZ)
run on stand-in objects rebuilt from the model's OWN accessors, so what is compared is the inference alone.  The bars
are the project's for the two-level models: assert_q_close(rtol=1e-6) on qY and qZ, 1e-8 relative on Fyz, Fz and the
per-row logZ sums, labels equal wherever the reference's two best candidates differ by more than 1e-9."""
import json

import numpy as np
import pytest

import lc_oracle as o
import libcluster_amd as lc
import topic_infer_ref as tir
from conftest import GOLDEN
from libcluster_amd import capi
from test_gpu_parity import assert_q_close

pytestmark = pytest.mark.gpu

SWEEPS = (1, 3, 8)


def _stand_ins(m):
    d = m.dims()
    wj = [tir.Weights(m.weights(0, j)[0]) for j in range(d["J"])]
    wt = [tir.Weights(m.weights(1, t)[0]) for t in range(d["T"])]
    cl = [tir.gauss_wish(m.cluster(0, k)) for k in range(d["K"])]
    ct = [tir.gauss_wish(m.cluster(1, t)) for t in range(d["T"])] if d["Dt"] > 0 else None
    return wj, wt, cl, ct


def _rel(got, ref, what):
    print(f"    {what}: got {got!r} ref {ref!r}")
    assert abs(got - ref) <= 1e-8 * abs(ref), what


def _check_doc(p, i, r, sweeps=None):
    """document i of TopicPrediction p against the reference DocInference r"""
    print(f"  doc {i}: N = {r.qZ.shape[0]} sweeps {p.sweeps[i]} (ref {r.sweeps}) "
          f"max |dqY| = {np.max(np.abs(p.qY[i] - r.qY)):.3e}")
    if sweeps is not None:
        assert p.sweeps[i] == sweeps == r.sweeps
    assert_q_close(p.qY[i], r.qY, rtol=1e-6)
    if p.qZ is not None:
        print(f"    max |dqZ| = {np.max(np.abs(p.qZ[i] - r.qZ), initial=0.0):.3e}")
        assert_q_close(p.qZ[i], r.qZ, rtol=1e-6)
    _rel(p.Fyz[i], r.Fyz, "Fyz")
    _rel(p.Fz[i], r.Fz, "Fz")
    _rel(float(p.logZ[i].sum()), float(r.logZ.sum()), "sum logZ")
    assert p.label[i].dtype == np.int32 and p.label[i].shape == r.label.shape
    clear = r.margin > 1e-9
    assert np.array_equal(p.label[i][clear], r.label[clear])
    if r.margin_t > 1e-9:
        assert p.label_t[i] == r.label_t


def _parity(m, docs, groups=None, W=None, sweeps=SWEEPS, qz=True):
    wj, wt, cl, ct = _stand_ins(m)
    for ms in sweeps:
        print(f"max_sweeps = {ms}")
        p = m.predict(docs, W=W, groups=groups, max_sweeps=ms, tol=-1.0, qz=qz)
        assert p.qY.shape == (len(docs), len(wt)) and p.label_t.dtype == np.int32 and p.sweeps.dtype == np.int32
        for i, x in enumerate(docs):
            g = 0 if groups is None else int(groups[i])
            r = tir.infer_document(x, wj[g], wt, cl, ms, -1.0, None if W is None else W[i], ct)
            _check_doc(p, i, r, ms)


@pytest.fixture(scope="module")
def golden(xcat):
    top = json.loads((GOLDEN / "topic_traces.json").read_text())
    X = [xcat["X"][:6], xcat["X"][6:]]
    out = {}
    ref = top["learnSCM"]
    res = lc.learnSCM(X, trunc=ref["maxT"], qY0=ref["qY0"], return_model=True)
    out["scm"] = (res[-1], res[1], None)
    ref = top["learnMCM"]
    res = lc.learnMCM(xcat["O"], X, trunc=ref["maxT"], qY0=ref["qY0"], return_model=True)
    out["mcm"] = (res[-1], res[1], np.vstack(xcat["O"]))
    out["docs"] = list(X[0]) + list(X[1])
    out["groups"] = [0] * len(X[0]) + [1] * len(X[1])
    yield out
    out["scm"][0].close()
    out["mcm"][0].close()


def _overlapping(mcm, seed):
    """the overlapping set-up (J = 3, I = 12, n ~ 30, D = 3, K = 4, T = 3, means at scale 1.5): 3 groups to learn
    from, a 4th of held-out documents from the same classes.  The seeds are two for which the oracle's own model
    needs different numbers of sweeps for the held-out documents (SCM: 3 to 33 at tol = 1e-5; MCM, whose document
    observations settle most of qY: 2 to 4)"""
    rng = np.random.default_rng(seed)
    X, W, _ = tir.synthetic_documents(rng, 4, 12, 30, 3, 4, 3, Dt=2 if mcm else 0, scale=1.5)
    qY0 = [o.random_qY(12, 6, rng) for _ in range(3)]
    if mcm:
        res = lc.learnMCM(W[:3], X[:3], trunc=6, qY0=qY0, return_model=True)
    else:
        res = lc.learnSCM(X[:3], trunc=6, qY0=qY0, return_model=True)
    groups = rng.integers(0, 3, len(X[3])).astype(np.int32)
    return res[-1], res[1], X, W, groups, rng


@pytest.fixture(scope="module")
def overlap_scm():
    out = _overlapping(False, 2025)
    yield out
    out[0].close()


@pytest.fixture(scope="module")
def overlap_mcm():
    out = _overlapping(True, 2032)
    yield out
    out[0].close()


@pytest.mark.parametrize("kind", ["scm", "mcm"])
def test_parity_on_the_golden_documents(golden, kind):
    """the documents of test/scluster_test.cpp / mcluster_test.cpp, each with the weights of its own group (0 and 1)"""
    m, _, W = golden[kind]
    _parity(m, golden["docs"], golden["groups"], W)


def test_parity_on_held_out_documents_scm(overlap_scm):
    """D = 3 (not a multiple of 4), groups 0..2, documents that need different numbers of sweeps"""
    m, _, X, _, groups, _ = overlap_scm
    _parity(m, X[3], groups)


def test_parity_on_held_out_documents_mcm(overlap_mcm):
    m, _, X, W, groups, _ = overlap_mcm
    _parity(m, X[3], groups, W[3])


def test_parity_for_one_row_empty_and_very_large_documents(overlap_scm):
    """a one-row document, a document without rows, and one of 300 000 rows, whose L tile does not fit the LDS budget
    (the sweeps re-read its columns from global memory), next to ordinary ones in the same launch"""
    m, _, X, _, _, _ = overlap_scm
    rng = np.random.default_rng(7)
    big = np.vstack([X[3][i % 12] for i in range(40)])
    big = big[rng.integers(0, big.shape[0], 300_000)] + 0.05 * rng.normal(size=(300_000, 3))
    docs = [X[3][0], X[3][1][:1], np.zeros((0, 3)), big, X[3][2], np.vstack(X[3][3:7])]
    groups = np.array([0, 1, 2, 1, 2, 0], dtype=np.int32)
    _parity(m, docs, groups)
    p = m.predict(docs, groups=groups, max_sweeps=50, tol=1e-5)
    wj = _stand_ins(m)[0]
    a = wj[2].Elogweight()
    assert p.sweeps[2] == 1 and p.Fz[2] == 0.0 and p.label[2].shape == (0,)  # no rows: delta_1 = 0
    np.testing.assert_allclose(p.qY[2], np.exp(a - o.logsumexp(a[None, :])[0]), rtol=1e-12)


def test_parity_with_a_class_by_segment_table_beyond_the_lds_budget():
    """T x K larger than the kernel's LDS allowance for the E table (128 doubles, lck::TOPIC_E_LDS), and K above the
    sixteen terms a row keeps in registers"""
    rng = np.random.default_rng(5)
    X, _, qY0, held = tir.many_segment_documents(rng)
    res = lc.learnSCM(X, trunc=qY0[0].shape[1], qY0=qY0, return_model=True)
    m = res[-1]
    try:
        d = m.dims()
        print("learned T, K =", d["T"], d["K"])
        assert d["T"] * d["K"] > 128 and d["K"] > 16
        _parity(m, held[:5] + [np.vstack(held[5:8])])
    finally:
        m.close()


def test_parity_at_a_width_that_takes_the_wide_e_step():
    """D = 130 > 128: the raw E-step in front of the kernel is estep_wide_kernel"""
    rng = np.random.default_rng(11)
    D = 130
    mu = rng.normal(0, 3.0, (2, D))
    docs = [mu[i % 2] + rng.normal(size=(150 + 10 * i, D)) for i in range(6)]
    qY0 = [o.random_qY(6, 2, rng)]
    res = lc.learnSCM([docs], trunc=2, qY0=qY0, return_model=True)
    m = res[-1]
    try:
        held = [mu[i % 2] + rng.normal(size=(40 + 30 * i, D)) for i in range(3)]
        _parity(m, held)
    finally:
        m.close()


def _converged(m, docs, groups, W, tol=1e-5, max_sweeps=50):
    wj, wt, cl, ct = _stand_ins(m)
    p = m.predict(docs, W=W, groups=groups, max_sweeps=max_sweeps, tol=tol, qz=True)
    for i, x in enumerate(docs):
        g = 0 if groups is None else int(groups[i])
        w = None if W is None else W[i]
        assert 1 <= p.sweeps[i] <= max_sweeps
        # one more reference sweep from the returned qY moves it by at most tol (plus the qY parity bar)
        qZ, _ = o.vbeZ(x, p.qY[i], wt, cl)
        new, _ = tir._vbeY(qZ, wj[g], wt, None if w is None else np.asarray(w).reshape(1, -1), ct)
        move = float(np.max(np.abs(new - p.qY[i])))
        r = tir.infer_document(x, wj[g], wt, cl, max_sweeps, tol, w, ct)
        print(f"  doc {i}: sweeps {p.sweeps[i]} (ref {r.sweeps}), next sweep moves qY by {move:.3e}")
        if p.sweeps[i] < max_sweeps:
            assert move <= tol + 1e-6 * max(tol, move) + 1e-11
        if r.sweeps == p.sweeps[i]:  # (the same stopping decision on both sides: the fixed-count bars apply)
            _check_doc(p, i, r)
    return p


def test_converged_mode_stops_every_document_on_its_own(overlap_scm, overlap_mcm):
    for m, _, X, W, groups, _ in (overlap_scm, overlap_mcm):
        p = _converged(m, X[3], groups, None if W is None else W[3])
        print("sweeps:", p.sweeps.tolist())
        assert len(set(p.sweeps.tolist())) > 1  # the documents of this set-up need different numbers of sweeps


@pytest.mark.parametrize("kind", ["scm", "mcm"])
def test_training_documents_keep_their_class(golden, kind, overlap_scm, overlap_mcm):
    """label_t of every training document is the argmax of its training qY"""
    m, qY, W = golden[kind]
    p = m.predict(golden["docs"], W=W, groups=golden["groups"])
    assert p.label_t.tolist() == [int(np.argmax(q)) for q in np.vstack(qY)]
    m, qY, X, W, _, _ = overlap_mcm if kind == "mcm" else overlap_scm
    docs = [x for Xj in X[:3] for x in Xj]
    groups = [j for j in range(3) for _ in X[j]]
    p = m.predict(docs, W=None if W is None else np.vstack(W[:3]), groups=groups)
    assert p.label_t.tolist() == [int(np.argmax(q)) for q in np.vstack(qY)]


def test_two_calls_give_the_same_bits_and_qz_is_optional(overlap_mcm):
    m, _, X, W, groups, _ = overlap_mcm
    docs = X[3] + [np.vstack(X[3])]  # (the last one spreads over several waves)
    Wd = np.vstack([W[3], W[3][:1]])
    g = np.concatenate([groups, groups[:1]])
    a = m.predict(docs, W=Wd, groups=g, max_sweeps=6, tol=-1.0, qz=True)
    b = m.predict(docs, W=Wd, groups=g, max_sweeps=6, tol=-1.0, qz=True)
    c = m.predict(docs, W=Wd, groups=g, max_sweeps=6, tol=-1.0, qz=False)
    assert c.qZ is None
    for other in (b, c):
        for f in ("qY", "label_t", "Fyz", "Fz", "sweeps"):
            assert np.array_equal(getattr(a, f), getattr(other, f)), f
        for i in range(len(docs)):
            assert np.array_equal(a.label[i], other.label[i]) and np.array_equal(a.logZ[i], other.logZ[i])
    for qa, qb in zip(a.qZ, b.qZ):
        assert np.array_equal(qa, qb)
        np.testing.assert_allclose(qa.sum(axis=1), 1.0, rtol=1e-12)


def test_context_plumbing_release_and_errors(xcat):
    from test_gpu_predict import _check, _fit, _oracle

    rng = np.random.default_rng(3)
    X, _, _ = tir.synthetic_documents(rng, 2, 6, 40, 2, 3, 2)
    res = lc.learnSCM(X, trunc=3, qY0=[o.random_qY(6, 3, rng) for _ in range(2)], return_model=True)
    assert len(res) == 8 and isinstance(res[-1], capi.TopicModel)
    assert len(lc.learnSCM(X, trunc=3, qY0=[o.random_qY(6, 3, rng) for _ in range(2)])) == 7  # default tuple unchanged
    m = res[-1]
    T = m.dims()["T"]
    docs = X[1]
    before = m.predict(docs, max_sweeps=4, tol=-1.0)
    m.release_data()
    after = m.predict(docs, max_sweeps=4, tol=-1.0)  # the parameters stay
    assert np.array_equal(before.qY, after.qY) and np.array_equal(before.Fz, after.Fz)
    with pytest.raises(ValueError):
        m.qZ()
    with pytest.raises(ValueError):
        m.qY()
    with capi.Context(0) as ctx:
        ctx.set_data(docs)
        with pytest.raises(ValueError, match="no document prediction"):
            ctx.get_doc_predictions(0, len(docs), T)
        m.predict_context(ctx, max_sweeps=4, tol=-1.0, keep_qz=True)
        qY = ctx.get_doc_predictions(0, len(docs), T)[0]
        assert np.array_equal(qY, before.qY)
        assert np.array_equal(ctx.get_doc_predictions(2, 3, T)[0], before.qY[2:5])
        with pytest.raises(ValueError, match="no log density"):
            ctx.get_predictions(0, 0, docs[0].shape[0], logp=True)
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_doc_predictions(0, len(docs) + 1, T)
        # argument errors
        with pytest.raises(ValueError, match="max_sweeps"):
            m.predict_context(ctx, max_sweeps=0)
        with pytest.raises(ValueError, match="group index out of range"):
            m.predict_context(ctx, groups=[0, 0, 2, 0, 0, 0])
        with pytest.raises(ValueError, match="must be NULL for an SCM"):
            check_w = np.zeros((len(docs), 1))
            capi.check(capi.lib().lc_tmodel_predict(m._h, ctx._h, None, capi.dptr(check_w), 4, -1.0, 0))
        # a flat model on the same context afterwards: lc_model_predict's own parity check on block 0
        fm, fctx = _fit([np.vstack(X[0])], capi.W_STICKBREAK, capi.C_GAUSSWISH, 3)
        try:
            fm.predict_context(ctx, keep_qz=True)
            ws, cls, prior = _oracle(fm)
            n = docs[0].shape[0]
            q = ctx.get_qz([x.shape[0] for x in docs])[0]
            _check(capi.Prediction(*ctx.get_predictions(0, 0, n), q), docs[0], ws[0], cls, prior, False)
            with pytest.raises(ValueError, match="no document prediction"):  # (the flat prediction replaced it)
                ctx.get_doc_predictions(0, 1, T)
        finally:
            fm.close()
            fctx.close()
        m.predict_context(ctx, max_sweeps=4, tol=-1.0)
        ctx.set_data([x[:5] for x in docs])  # new rows: the per-document outputs belong to the old ones
        with pytest.raises(ValueError, match="no document prediction"):
            ctx.get_doc_predictions(0, 1, T)
    with capi.Context(0) as ctx:
        ctx.set_data([np.zeros((4, 3))])
        with pytest.raises(ValueError, match="Mismatched dims"):
            m.predict_context(ctx)
    # MCM: W is required
    Xm, Wm, _ = tir.synthetic_documents(rng, 1, 6, 40, 2, 3, 2, Dt=2)
    mm = lc.learnMCM(Wm, Xm, trunc=3, qY0=[o.random_qY(6, 3, rng)], return_model=True)[-1]
    with capi.Context(0) as ctx:
        ctx.set_data(Xm[0])
        with pytest.raises(ValueError, match="same number of 'docs'"):
            mm.predict_context(ctx)
    mm.close()
    # a freed model
    h = m._h
    m.close()
    with capi.Context(0) as ctx:
        ctx.set_data(docs)
        with pytest.raises(ValueError, match="freed"):
            capi.check(capi.lib().lc_tmodel_predict(h, ctx._h, None, None, 4, -1.0, 0))
    with pytest.raises(ValueError, match="freed"):
        capi.check(capi.lib().lc_tmodel_release_data(h))
