"""Inference for new documents with a learned SCM / MCM model (lc_tmodel_predict): the definition as
tests/topic_infer_ref.py restates it from the oracle's vbeY / vbeZ, checked on the oracle's own models, and the new
symbols of the C ABI.  No GPU needed."""
import json
import re

import numpy as np
import pytest

import lc_oracle as o
import topic_infer_ref as tir
from conftest import GOLDEN
from libcluster_amd import capi

NEW_SYMBOLS = ("lc_tmodel_predict", "lc_ctx_get_doc_predictions", "lc_tmodel_release_data")


def _learn(X, W, maxT, qY0):
    """The oracle's model as (qY, weights_j, weights_t, clusters, clusters_t or None)."""
    if W is None:
        _, qY, _, wj, wt, cl = o.learnSCM(X, maxT=maxT, qY0=qY0)
        return qY, wj, wt, cl, None
    _, qY, _, wj, wt, ct, cl = o.learnMCM(W, X, maxT=maxT, qY0=qY0)
    return qY, wj, wt, cl, ct


@pytest.fixture(scope="module")
def setups(xcat):
    """name -> (X, W, model): the two committed set-ups of tests/golden/topic_traces.json and the overlapping synthetic
    one (J = 3, I = 12, n ~ 30, D = 3, K = 4, T = 3, component means at scale 1.5)."""
    top = json.loads((GOLDEN / "topic_traces.json").read_text())
    Xg = [xcat["X"][:6], xcat["X"][6:]]
    out = {}
    for name, W in (("learnSCM", None), ("learnMCM", xcat["O"])):
        ref = top[name]
        qY0 = [np.array(q) for q in ref["qY0"]]
        out[name] = (Xg, W, _learn(Xg, W, ref["maxT"], qY0))
    rng = np.random.default_rng(2024)
    X, _, _ = tir.synthetic_documents(rng, 3, 12, 30, 3, 4, 3, scale=1.5)
    qY0 = [o.random_qY(12, 6, rng) for _ in range(3)]
    out["synthetic"] = (X, None, _learn(X, None, 6, qY0))
    return out


def _documents(X, W, model):
    qY, wj, wt, cl, ct = model
    for j in range(len(X)):
        for i in range(len(X[j])):
            yield X[j][i], (None if W is None else W[j][i]), wj[j], wt, cl, ct, qY[j][i]


@pytest.mark.parametrize("name", ["learnSCM", "learnMCM", "synthetic"])
def test_training_documents_are_recalled(setups, name):
    """Every training document's label_t equals the argmax of its training qY; no document is left out."""
    X, W, model = setups[name]
    n = 0
    for x, w, wj, wt, cl, ct, qtrain in _documents(X, W, model):
        r = tir.infer_document(x, wj, wt, cl, 50, o.CONVERGE, w, ct)
        assert r.label_t == int(np.argmax(qtrain)), (name, n, r.qY, qtrain)
        assert 1 <= r.sweeps <= 50
        n += 1
    assert n == sum(len(Xj) for Xj in X)


@pytest.mark.parametrize("name", ["learnSCM", "learnMCM", "synthetic"])
def test_sweeps_are_coordinate_ascent(setups, name):
    """With the model fixed the document's bound Fyz_i + Fz_i, evaluated with the same qY in both terms, does not
    increase from sweep to sweep beyond rounding (FENGYDEL, the learners' own slack), and the returned Fyz + Fz is that
    bound at qY^R."""
    X, W, model = setups[name]
    for x, w, wj, wt, cl, ct, _ in _documents(X, W, model):
        r = tir.infer_document(x, wj, wt, cl, 12, -1.0, w, ct)
        F = [tir.document_bound(x, r.trace[0][0], wj, wt, cl, w, ct)]
        F += [tir.document_bound(x, new, wj, wt, cl, w, ct) for _, new, _ in r.trace]
        for a, b in zip(F[:-1], F[1:]):
            assert (b - a) / abs(a) <= o.FENGYDEL, (name, F)
        assert abs((r.Fyz + r.Fz) - F[-1]) <= 1e-9 * abs(F[-1])


def test_sweep_rule_and_empty_document(setups):
    X, W, model = setups["synthetic"]
    _, wj, wt, cl, ct = model
    x = X[1][3]
    for ms in (1, 3, 8):
        r = tir.infer_document(x, wj[1], wt, cl, ms, -1.0)
        assert r.sweeps == ms and len(r.trace) == ms  # tol < 0: exactly max_sweeps
    r = tir.infer_document(x, wj[1], wt, cl, 50, 1e-5)
    assert r.trace[-1][2] <= 1e-5 and all(d > 1e-5 for _, _, d in r.trace[:-1])  # the FIRST sweep with delta <= tol
    # a document without rows: N_k = 0, qY = softmax(a) = the group's weights, one sweep, Fz = 0
    e = tir.infer_document(np.zeros((0, 3)), wj[2], wt, cl, 50, 1e-5)
    a = wj[2].Elogweight()
    sm = np.exp(a - o.logsumexp(a[None, :])[0])
    assert e.sweeps == 1 and e.Fz == 0.0 and e.qZ.shape == (0, len(cl)) and e.label.shape == (0,)
    np.testing.assert_allclose(e.qY, sm, rtol=1e-14)
    assert e.label_t == int(np.argmax(sm))
    with pytest.raises(ValueError):
        tir.infer_document(x, wj[1], wt, cl, 0, 1e-5)


def test_restatement_rows_agree_with_vbeZ(setups):
    """logZ and label per row come from the same c_k + L_nk that vbeZ normalises."""
    X, W, model = setups["learnMCM"]
    for x, w, wj, wt, cl, ct, _ in _documents(X, W, model):
        r = tir.infer_document(x, wj, wt, cl, 4, -1.0, w, ct)
        assert abs(-r.logZ.sum() - r.Fz) <= 1e-12 * abs(r.Fz)
        np.testing.assert_array_equal(r.label, np.argmax(r.qZ, axis=1))


def test_stand_ins_reproduce_the_oracle_objects(setups):
    """The objects the GPU tests rebuild from a model's accessors (nu, beta, m, iW, logdW; Elogweight) give the same
    Eloglike as the distributions they describe."""
    X, _, model = setups["learnSCM"]
    _, wj, wt, cl, _ = model
    for c in cl:
        g = tir.gauss_wish({"nu": c.nu, "beta": c.beta, "mean": c.m, "iW": c.iW, "logdW": c.logdW})
        np.testing.assert_allclose(g.Eloglike(X[0][0]), c.Eloglike(X[0][0]), rtol=1e-14)
    np.testing.assert_array_equal(tir.Weights(wj[0].Elogweight()).Elogweight(), wj[0].Elogweight())


def test_header_declares_and_library_exports_the_new_symbols(lib):
    declared = capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/libcluster_hip.h"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    txt = re.sub(r"\s+", " ", capi.HEADER.read_text())
    assert ("int lc_tmodel_predict(lc_tmodel* m, lc_ctx* ctx, const int* groups, const double* W, int max_sweeps, "
            "double tol, int keep_qz);") in txt
    assert ("int lc_ctx_get_doc_predictions(lc_ctx* ctx, int doc0, int n, double* qY, int32_t* label_t, double* Fyz, "
            "double* Fz, int32_t* sweeps);") in txt
    assert "int lc_tmodel_release_data(lc_tmodel* m);" in txt


def test_python_interface_has_the_new_arguments():
    import inspect

    import libcluster_amd as lc

    for fn in (lc.learnSCM, lc.learnMCM):
        assert inspect.signature(fn).parameters["return_model"].default is False
    sig = inspect.signature(capi.TopicModel.predict)
    assert list(sig.parameters)[1:] == ["X", "W", "groups", "max_sweeps", "tol", "qz", "device"]
    assert sig.parameters["max_sweeps"].default == 50
    assert capi.TopicPrediction._fields == ("qY", "label_t", "Fyz", "Fz", "sweeps", "label", "logZ", "qZ")
    assert hasattr(capi.TopicModel, "predict_context") and hasattr(capi.TopicModel, "release_data")
