"""Device-resident float64 tensors in, row results on the device, through the public interface:
Context.set_data, the flat and grouped learners and Model.predict on CUDA torch tensors against the numpy route on the
same values -- the same image, and from there the same bits everywhere."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def lc(lib):
    import libcluster_amd

    return libcluster_amd


@pytest.fixture(scope="module")
def capi(lib):
    from libcluster_amd import capi

    return capi


@pytest.fixture(scope="module")
def blobs():
    """N = 3000, D = 5, three separated components, rows shuffled; (X, the same rows as three ragged blocks)"""
    rng = np.random.default_rng(42)
    mu = np.array([[0.0, 0, 0, 0, 0], [9.0, 9, 0, -9, 0], [-9.0, 9, 9, 0, 9]])
    X = np.vstack([rng.standard_normal((1000, 5)) + m for m in mu])
    X = np.ascontiguousarray(X[rng.permutation(3000)])
    return X, [X[:700], X[700:1801], X[1801:]]


@pytest.fixture(scope="module")
def model(lc, blobs):
    """a VDP model learned on the host route, shared (read only) by the prediction tests"""
    out = lc.learnVDP(blobs[0], nthreads=2, return_model=True)
    yield out[-1]
    out[-1].close()


def same(a, b):
    if a is None or b is None:
        return a is b
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_result(dev, host, torch, grouped=False):
    """(F, qZ, w, mu, cov) of a learner on tensors against the same on arrays: qZ on the device, everything the same bits"""
    assert dev[0] == host[0]
    qd, qh = (dev[1], host[1]) if grouped else ([dev[1]], [host[1]])
    assert len(qd) == len(qh)
    for a, b in zip(qd, qh):
        assert a.is_cuda and a.dtype == torch.float64 and a.is_contiguous()
        assert torch.equal(a.cpu(), torch.from_numpy(np.ascontiguousarray(b)))
    wd, wh = (dev[2], host[2]) if grouped else ([dev[2]], [host[2]])
    assert len(wd) == len(wh) and all(same(a, b) for a, b in zip(wd, wh))
    assert len(dev[3]) == len(host[3]) and all(same(a, b) for a, b in zip(dev[3], host[3]))
    for a, b in zip(dev[4], host[4]):
        assert (a is None and b is None) or same(a, b)


def test_tensor_and_array_give_the_same_image(capi, torch):
    import ingest_hooks as ih

    rng = np.random.default_rng(3)
    Xs = [rng.standard_normal((n, 23)) for n in (37, 64, 5)]
    Xt = [torch.from_numpy(x).cuda() for x in Xs]
    # a context of the same shape that held nothing but NaN has come and gone: the block cache hands its blocks back, so
    # whatever the pack does not write shows
    with capi.Context(0) as c0:
        c0.set_data([np.full_like(x, np.nan) for x in Xs])
    with capi.Context(0) as ct, capi.Context(0) as ch:
        ct.set_data(Xt)
        ch.set_data(Xs)
        rt, it = ih.ctx_image(ct)
        rh, im = ih.ctx_image(ch)
        assert rt == 0 and rh == 0 and it.shape == im.shape == (48 + 64 + 16, 32)
        assert np.array_equal(it.view(np.uint64), im.view(np.uint64))
        for j, x in enumerate(Xs):
            assert same(ct.get_rows(j, 0, x.shape[0]), x)
        assert ct.data_range() == (min(x.min() for x in Xs), 0) == ch.data_range()
        # the image is a copy: zeroing the tensors changes nothing the context computes
        ct.fill_qz(3, 0.25)
        before = (ct.colsums(), ct.suffstat())
        for x in Xt:
            x.zero_()
        torch.cuda.synchronize()
        after = (ct.colsums(), ct.suffstat())
        assert same(before[0], after[0]) and all(same(a, b) for a, b in zip(before[1], after[1]))
        ch.fill_qz(3, 0.25)
        assert all(same(a, b) for a, b in zip(after[1], ch.suffstat()))
        assert same(ct.get_rows(1, 0, 64), Xs[1])


@pytest.mark.parametrize("name", ("learnVDP", "learnBGMM", "learnDGMM"))
def test_flat_learners_match_the_numpy_route(lc, torch, blobs, name):
    X = blobs[0]
    Xt = torch.from_numpy(X).cuda()
    host = getattr(lc, name)(X, nthreads=2)
    dev = getattr(lc, name)(Xt, nthreads=2)
    assert_same_result(dev, host, torch)
    assert dev[1].device == Xt.device and dev[1].shape == (3000, len(dev[3]))
    if name == "learnVDP":  # column-major input: the transposing pack, the same image and so the same bits again
        Xc = Xt.t().contiguous().t()
        assert Xc.stride() == (1, 3000)
        assert_same_result(lc.learnVDP(Xc, nthreads=2), host, torch)


def test_grouped_learner_matches_the_numpy_route(lc, torch, blobs):
    Xs = blobs[1]
    host = lc.learnGMC(Xs, nthreads=2)
    dev = lc.learnGMC([torch.from_numpy(x).cuda() for x in Xs], nthreads=2)
    assert_same_result(dev, host, torch, grouped=True)
    assert [tuple(q.shape)[0] for q in dev[1]] == [x.shape[0] for x in Xs]


def test_expgamma_domain_comes_from_the_device(lc, torch, blobs):
    X = np.abs(blobs[0]) + 0.01
    bad = X.copy()
    bad[-1, 3] = -1e-3
    with pytest.raises(ValueError, match=r"range \[0, inf\)"):
        lc.learnBEMM(torch.from_numpy(bad).cuda(), nthreads=2)
    assert_same_result(lc.learnBEMM(torch.from_numpy(X).cuda(), nthreads=2), lc.learnBEMM(X, nthreads=2), torch)


def assert_same_prediction(dev, host, torch, qz=True):
    assert dev.label.is_cuda and dev.label.dtype == torch.int32
    assert dev.logZ.is_cuda and dev.logZ.dtype == torch.float64 and dev.logp.is_cuda and dev.logp.dtype == torch.float64
    assert same(dev.label.cpu().numpy(), host.label)
    assert same(dev.logZ.cpu().numpy(), host.logZ) and same(dev.logp.cpu().numpy(), host.logp)
    if qz:
        assert dev.qZ.is_cuda and dev.qZ.dtype == torch.float64 and same(dev.qZ.cpu().numpy(), host.qZ)
    else:
        assert dev.qZ is None and host.qZ is None


def test_predict_matches_the_numpy_route(model, torch, blobs):
    X, Xs = blobs[0][:777] * 1.01, [blobs[0][100:165] + 0.5, blobs[0][2000:2129]]
    assert_same_prediction(model.predict(torch.from_numpy(X).cuda(), qz=True), model.predict(X, qz=True), torch)
    assert_same_prediction(model.predict(torch.from_numpy(X).cuda()), model.predict(X), torch, qz=False)
    dev = model.predict([torch.from_numpy(x).cuda() for x in Xs], groups=[0, 0], qz=True)
    host = model.predict(Xs, groups=[0, 0], qz=True)
    assert len(dev) == len(host) == 2
    for d, h in zip(dev, host):
        assert_same_prediction(d, h, torch)


def test_context_queries_work_on_a_tensor_filled_context(model, capi, torch, blobs):
    X = blobs[0][:300].copy()
    with capi.Context(0) as ct, capi.Context(0) as ch:  # complete rows: every column scored given the others
        ct.set_data(torch.from_numpy(X).cuda())
        ch.set_data(X)
        model.explain_context(ct)
        model.explain_context(ch)
        for a, b in zip(ct.get_leave_one_out(0, 0, 300), ch.get_leave_one_out(0, 0, 300)):
            assert same(a, b)
    X[::7, 2] = np.nan
    X[5, :4] = np.nan
    with capi.Context(0) as ct, capi.Context(0) as ch:  # rows with holes
        ct.set_data(torch.from_numpy(X).cuda())
        ch.set_data(X)
        assert ct.data_range() == (np.nanmin(X), int(np.isnan(X).sum())) == ch.data_range()
        model.predict_incomplete_context(ct)
        model.predict_incomplete_context(ch)
        for a, b in zip(ct.get_completed(0, 0, 300), ch.get_completed(0, 0, 300)):
            assert same(a, b)


def test_predict_follows_the_producer_on_torchs_current_stream(model, torch, blobs):
    """(cannot prove the ordering; catches a wrapper that works on another stream than the one that produced X)"""
    base = torch.from_numpy(blobs[0]).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        Xt = base * 1.5 + 0.25
        dev = model.predict(Xt, qz=True)
    assert_same_prediction(dev, model.predict(blobs[0] * 1.5 + 0.25, qz=True), torch)


def test_refused_before_anything_is_launched(lc, capi, torch, blobs):
    Xt = torch.from_numpy(blobs[0][:64]).cuda()
    with capi.Context(0) as ctx:
        with pytest.raises(TypeError, match="float64"):
            ctx.set_data(Xt.float())
        with pytest.raises(ValueError, match="mixes"):
            ctx.set_data([Xt, blobs[0][:10]])
        with pytest.raises(ValueError, match="2-D"):
            ctx.set_data(Xt[:, 0])
        with pytest.raises(ValueError, match="inconsistent"):
            ctx.set_data([Xt, Xt[:, :3]])
        assert ctx.dims()[0] == 0  # nothing reached the context
    with pytest.raises(TypeError, match="float64"):
        lc.learnVDP(Xt.float())
    with pytest.raises(ValueError, match="device"):
        lc.learnVDP(Xt, device=Xt.device.index + 1)
