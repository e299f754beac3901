"""Leave-one-out conditionals through the public interface (Model.explain, lc_model_predict_leave_one_out): per
row and column log p(x_d | x_-d), E[x_d | x_-d], Var[x_d | x_-d] and the column a row's model likes least.

Models, held-out rows and posteriors are those of tests/test_gpu_incomplete.py (its cached _model).  Two witnesses:
  * tests/leave_one_out_ref.py, loo_direct: numpy / scipy on the posteriors, one NaN per row of an (N D, D) array through the
    references of the rows with holes -- never the device, never the emulation of its route;
  * the existing device route: D calls of Model.predict_incomplete(variance=True), column d unknown in every row.
Bars: |cond - ref| <= 1e-10 max(|logp|, |rest|), |mean - ref| <= 1e-9 S, |var - ref| <= 1e-9 V with
S = max_k |M_k,d| and V = max_k [Cov_k,d + (M_k,d - mean_d)^2] from the reference.  One exception, the model that sits 1e3
away from the origin: max(1e-10, 4 E) (and 1e-9 -> max(1e-9, 4 E)) with E the largest error of the numpy emulation of the
route against the reference in the same units, computed here and printed -- the rule of tests/test_gpu_incomplete.py.
The D = 2 model has StickBreak weights whose prior component has nu = 2: its variance does not exist (the error test below),
so that case is held to cond and mean only."""
import functools

import numpy as np
import pytest

import leave_one_out_ref as loo
import test_gpu_incomplete as inc
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

CASES = ["d2", "d5", "d23", "d64", "d200", "d23_offset"]


def _rows(name):
    Xnew = inc._model(name)[1]
    return Xnew[:60] if name == "d200" else Xnew


@functools.lru_cache(maxsize=None)
def _reference(name):
    """computed once, shared and never changed"""
    m, _, (cls, prior, ws, _) = inc._model(name)
    return loo.loo_direct(_rows(name), cls, prior, *ws[0], variance=name != "d2")


def _ratios(got, want, variance):
    cb, S, V = loo.bars(want)
    rc = float(np.max(np.abs(got.cond_logp - want.cond) / cb))
    rm = float(np.max(np.abs(got.mean - want.mean) / S))
    rv = float(np.max(np.abs(got.var - want.var) / V)) if variance else 0.0
    return rc, rm, rv


@pytest.mark.parametrize("name", CASES)
def test_against_numpy_scipy(name):
    m, _, (cls, prior, ws, _) = inc._model(name)
    X = _rows(name)
    variance = name != "d2"
    want = _reference(name)
    share = float(np.mean(want.rmax < 0.99))
    print(f"{name}: share of (row, column) pairs with max_k r < 0.99 = {share:.2f}")
    assert share >= 0.1, share  # not vacuous, by the reference alone
    fc, fm = 1e-10, 1e-9
    if name == "d23_offset":
        emu = loo.loo_emulate(X, cls, prior, *ws[0])
        cb, S, V = loo.bars(want)
        E = float(max(np.max(np.abs(emu.cond - want.cond) / cb), np.max(np.abs(emu.mean - want.mean) / S),
                      np.max(np.abs(emu.var - want.var) / V)))
        print(f"{name}: largest error of the emulated route in units of the bars' scales E = {E:.3e}")
        fc, fm = max(1e-10, 4 * E), max(1e-9, 4 * E)
    keep = X.copy()
    got = m.explain(keep, variance=variance)
    assert np.array_equal(keep.view(np.int64), X.view(np.int64))  # the input array is unchanged
    assert isinstance(got, capi.LeaveOneOutVar if variance else capi.LeaveOneOut)
    assert got.cond_logp.shape == X.shape and got.mean.shape == X.shape and got.worst.dtype == np.int32
    rc, rm, rv = _ratios(got, want, variance)
    print(f"{name}: max |device - ref| / scale: cond {rc:.3e} (bar {fc:.1e}), mean {rm:.3e} ({fm:.1e}), var {rv:.3e} ({fm:.1e})")
    assert np.array_equal(got.logp, m.predict(X).logp)  # bit for bit
    assert np.array_equal(got.worst, np.argmin(got.cond_logp, axis=1))
    assert np.all(np.isfinite(got.cond_logp)) and np.all(np.isfinite(got.mean))
    assert rc <= fc and rm <= fm and rv <= fm, (rc, rm, rv)
    if variance:
        assert np.all(got.var > 0)
        plain = m.explain(X)  # the call without variance: the same bits
        assert plain.var is None and all(np.array_equal(getattr(plain, f), getattr(got, f)) for f in plain._fields)


@pytest.mark.parametrize("name", ["d5", "d23"])
def test_against_the_existing_device_route(name):
    """D calls of predict_incomplete(variance=True), column d unknown in every row: an independent witness on the device"""
    m, _, _ = inc._model(name)
    X = _rows(name)
    want = _reference(name)
    cb, S, V = loo.bars(want)
    got = m.explain(X, variance=True)
    worst = [0.0, 0.0, 0.0]
    for d in range(X.shape[1]):
        Xh = X.copy()
        Xh[:, d] = np.nan
        old = m.predict_incomplete(Xh, variance=True)
        worst[0] = max(worst[0], float(np.max(np.abs(old.logp - (got.logp - got.cond_logp[:, d])) / cb[:, d])))
        worst[1] = max(worst[1], float(np.max(np.abs(old.rows[:, d] - got.mean[:, d]) / S[:, d])))
        worst[2] = max(worst[2], float(np.max(np.abs(old.var[:, 0] - got.var[:, d]) / V[:, d])))
    print(f"{name}: max |explain - predict_incomplete| / scale: rest {worst[0]:.3e}, mean {worst[1]:.3e}, var {worst[2]:.3e}")
    assert worst[0] <= 1e-10 and worst[1] <= 1e-9 and worst[2] <= 1e-9, worst


def test_blocks_groups_and_reuse():
    m, held, _ = inc._grouped_model()
    blocks, groups = [held[0][:37], held[1][:5]], [2, 0]
    got = m.explain(blocks, groups=groups, variance=True)
    assert len(got) == 2
    for b, (x, g) in enumerate(zip(blocks, groups)):
        alone = m.explain(x, groups=[g], variance=True)
        assert all(np.array_equal(u, v) for u, v in zip(alone, got[b])), b
    other = m.explain(blocks[0], groups=[0])
    assert np.max(np.abs(other.cond_logp - got[0].cond_logp)) > 1e-6  # (the groups' weights differ)
    with capi.Context(0) as ctx:
        ctx.set_data(blocks)
        with pytest.raises(ValueError, match="no leave-one-out prediction"):
            ctx.get_leave_one_out(0, 0, 4)
        m.explain_context(ctx, groups, variance=True)
        part = ctx.get_leave_one_out(0, 5, 7, variance=True)
        assert all(np.array_equal(u, v[5:12]) for u, v in zip(part, got[0]))
        m.predict_incomplete_context(ctx, groups)  # replaces the prediction
        with pytest.raises(ValueError, match="no leave-one-out prediction"):
            ctx.get_leave_one_out(0, 0, 4)
        assert np.array_equal(ctx.get_completed(1, 0, 5).logp, got[1].logp)
        m.explain_context(ctx, groups)  # ... and the reverse
        with pytest.raises(ValueError, match="no completed rows"):
            ctx.get_completed(0, 0, 4)
        assert np.array_equal(ctx.get_leave_one_out(1, 0, 5).cond_logp, got[1].cond_logp)
        with pytest.raises(ValueError):  # (the ranking queries refuse it as they refuse an incomplete prediction)
            ctx.top_rows(3, by="logp")


def test_far_row_stays_finite():
    m, Xnew, (cls, _, _, _) = inc._model("d23")
    X = Xnew[:20].copy()
    sigma = np.sqrt(np.diag(cls[0][3]) / cls[0][0])
    X[11] = cls[0][2] + 1e6 * sigma
    got = m.explain(X, variance=True)
    for f in ("logp", "cond_logp", "mean", "var"):
        assert np.all(np.isfinite(getattr(got, f))), f
    assert np.all(got.var > 0)
    assert np.array_equal(got.worst, np.argmin(got.cond_logp, axis=1))


def test_a_nan_is_refused_with_block_and_row():
    m, held, _ = inc._grouped_model()
    blocks = [held[0][:37].copy(), held[1][:12].copy()]
    blocks[1][7, 2] = np.nan
    blocks[1][9, 0] = np.nan
    keep = [b.copy() for b in blocks]
    with capi.Context(0) as ctx:
        ctx.set_data(blocks)
        assert capi.lib().lc_model_predict_leave_one_out(m._h, ctx._h, None, 0) == capi.LC_EINVAL
        msg = capi.lib().lc_last_error().decode()
        assert "row 7" in msg and "block 1" in msg and "complete rows" in msg and "lc_model_predict_incomplete" in msg, msg
        with pytest.raises(ValueError, match="no leave-one-out prediction"):
            ctx.get_leave_one_out(0, 0, 4)
        for j, k in enumerate(keep):  # the observations keep every bit, NaNs included
            assert np.array_equal(ctx.get_rows(j, 0, k.shape[0]).view(np.int64), k.view(np.int64))
        with pytest.raises(ValueError, match="row 7 of block 1"):
            m.explain_context(ctx, variance=True)
        m.predict_incomplete_context(ctx)  # the call that takes such rows still works on the same context
        assert ctx.get_completed(1, 0, 12).count[7] == 1


def test_variance_needs_nu_above_two():
    m, Xnew, (cls, prior, ws, _) = inc._model("d2")
    Epi, rest = ws[0]
    assert rest > 0 and not prior[0] - 2 > 0  # a positive-weight component (the prior's) has nu <= 2
    with pytest.raises(capi.DomainError, match="prior component"):
        m.explain(Xnew[:30], variance=True)
    got = m.explain(Xnew[:30])
    assert np.all(np.isfinite(got.cond_logp)) and np.all(np.isfinite(got.mean))
    with capi.Context(0) as ctx:
        ctx.set_data([Xnew[:30]])
        m.explain_context(ctx)
        with pytest.raises(capi.DomainError):
            m.explain_context(ctx, variance=True)
        with pytest.raises(ValueError, match="no leave-one-out prediction"):  # a failing call leaves none
            ctx.get_leave_one_out(0, 0, 4)


def test_argument_errors():
    m, Xnew, _ = inc._model("d23")
    rng = np.random.default_rng(5)
    Xd = np.abs(rng.normal(size=(200, 4))) + 0.1
    ng, _ = inc._fit([Xd], capi.W_DIRICHLET, 3, ckind=capi.C_NORMGAMMA)
    with pytest.raises(ValueError, match="Gauss-Wishart"):
        ng.explain(Xd[:10])
    with capi.Context(0) as ctx:
        ctx.set_data([Xnew[:20, :22].copy()])
        with pytest.raises(ValueError, match="Mismatched dims"):
            m.explain_context(ctx)
        ctx.set_data([Xnew[:20]])
        with pytest.raises(ValueError, match="group index"):
            m.explain_context(ctx, groups=[3])
        m.explain_context(ctx)
        with pytest.raises(ValueError, match="no variance"):
            ctx.get_leave_one_out(0, 0, 4, variance=True)
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_leave_one_out(0, 18, 3)
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_leave_one_out(1, 0, 1)
        L = capi.lib()
        buf = np.full((4, 26), -1.0)
        assert L.lc_ctx_get_leave_one_out(ctx._h, 0, 0, 4, None, None, None, None, 0, None) == capi.LC_OK  # any output may be NULL
        assert L.lc_ctx_get_leave_one_out(ctx._h, 0, 0, 4, None, capi.dptr(buf), None, None, 22, None) == capi.LC_EINVAL
        assert L.lc_ctx_get_leave_one_out(ctx._h, 0, 0, 4, None, capi.dptr(buf), None, None, 26, None) == capi.LC_OK
        assert np.array_equal(buf[:, :23], ctx.get_leave_one_out(0, 0, 4).cond_logp) and np.all(buf[:, 23:] == -1.0)
