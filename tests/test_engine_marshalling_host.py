"""Host tests of the marshalling layer of xeofs_amd/engine.py: the private helpers every entry point goes through.  No GPU and
no engine context -- `sketch_matrix` is host-native, the context-state helpers run against a stub that records calls.  What
is pinned here is what each call site passes today (the keywords are quoted next to the case), so that the GPU suite does
not have to see it indirectly.
"""

from types import SimpleNamespace

import numpy as np
import pytest

from xeofs_amd import engine, sharded


# ------------------------------------------------------------------------------------------------ _sketch
class Future:
    """anything with `.result()`: counts how often it is joined"""

    def __init__(self, value):
        self.value, self.joins = value, 0

    def result(self):
        self.joins += 1
        return self.value


# the keywords of the call sites: (identity_when_full, exact_rows)
FIT = dict(identity_when_full=False, exact_rows=False)            # fit, fit_sharded
RSVD = dict(identity_when_full=False, exact_rows=True)            # rsvd, crosscov_rsvd
FULL = dict(identity_when_full=True, exact_rows=True)             # crosscov_rsvd_sharded, the four complex entries, complex_rsvd
PANEL = dict(identity_when_full=True, exact_rows=None, resolve_first=True)      # sharded._resolve_sketch


@pytest.mark.parametrize("kw", [FIT, RSVD, FULL, PANEL])
@pytest.mark.parametrize("seed", [0, 7, 2 ** 32 - 1])
def test_sketch_none_is_the_legacy_draw(kw, seed):
    rows, width = 37, 12
    got = engine._sketch(rows, width, None, seed, **kw)
    ref = np.random.RandomState(seed).normal(size=(rows, width)).astype(np.float32)
    assert got.dtype == np.float32 and got.flags.c_contiguous and got.shape == (rows, width)
    assert np.array_equal(got, ref)
    # a RandomState instance draws from its own stream (and advances it)
    rs = np.random.RandomState(seed)
    assert np.array_equal(engine._sketch(rows, width, None, rs, **kw), ref)
    assert not np.array_equal(engine._sketch(rows, width, None, rs, **kw), ref)


@pytest.mark.parametrize("kw", [FIT, RSVD, FULL, PANEL])
def test_sketch_joins_a_future_once_and_casts(kw):
    om = np.asfortranarray(np.arange(40 * 6, dtype=np.float64).reshape(40, 6))
    fut = Future(om)
    got = engine._sketch(40, 6, fut, None, **kw)
    assert fut.joins == 1
    assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, om.astype(np.float32))
    real = engine.SketchFuture(40, 6, 3)
    assert np.array_equal(engine._sketch(40, 6, real, None, **kw), engine.sketch_matrix(40, 6, 3))
    assert np.array_equal(engine._sketch(30, 6, engine.SketchSlice(real, 30), None, **kw), engine.sketch_matrix(30, 6, 3))
    # a float32 C-contiguous array passes through as it is (no copy of a page-locked staging buffer)
    own = engine.sketch_matrix(40, 6, 5)
    assert engine._sketch(40, 6, own, None, **kw) is own


def test_sketch_full_width_identity():
    # the complex entries: [rank, k + n_oversamples] with the ones on the leading diagonal, wider than the rank or not
    for rows, width in ((8, 8), (8, 13)):
        got = engine._sketch(rows, width, None, 0, **FULL)
        ref = np.zeros((rows, width), np.float32)
        ref[np.arange(rows), np.arange(rows)] = 1.0
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, ref)
    # ... where the caller's matrix is neither joined nor checked
    fut = Future(np.zeros((3, 3)))
    assert np.array_equal(engine._sketch(8, 8, fut, None, **FULL), np.eye(8, dtype=np.float32))
    assert fut.joins == 0
    assert np.array_equal(engine._sketch(8, 8, np.zeros((2, 2)), None, **FULL), np.eye(8, dtype=np.float32))
    # one column short of full width: a draw
    assert np.array_equal(engine._sketch(8, 7, None, 4, **FULL), engine.sketch_matrix(8, 7, 4))
    # the real single-GPU entries leave the identity to the engine: they hand it the draw
    for kw in (FIT, RSVD):
        assert np.array_equal(engine._sketch(8, 8, None, 4, **kw), engine.sketch_matrix(8, 8, 4))
    # the panel-level drivers: the square identity of the rank, after resolving what they were given
    fut = Future(np.zeros((8, 13)))
    om, l = sharded._resolve_sketch(5, 8, 8, fut, None)
    assert l == 8 and fut.joins == 1
    assert om.dtype == np.float32 and om.flags.c_contiguous and np.array_equal(om, np.eye(8, dtype=np.float32))
    rs = np.random.RandomState(1)
    sharded._resolve_sketch(5, 8, 8, None, rs)                          # the discarded draw advances a shared stream
    assert np.array_equal(rs.normal(size=3), np.random.RandomState(1).normal(size=8 * 13 + 3)[-3:])


def test_sketch_shape_rule():
    rows, width = 20, 6
    msg = r"omega must have shape \(20, 6\)"
    ok = np.ones((rows, width), np.float32)
    more_rows = np.ones((rows + 5, width), np.float32)
    for kw in (FIT, RSVD, FULL):
        assert engine._sketch(rows, width, ok, None, **kw) is ok
        for bad in (np.ones((rows - 1, width)), np.ones((rows, width + 1)), np.ones((rows, width - 1)), np.ones(rows),
                    np.ones((rows, width, 1))):
            with pytest.raises(ValueError, match=msg):
                engine._sketch(rows, width, bad, None, **kw)
            with pytest.raises(ValueError, match=msg):
                engine._sketch(rows, width, Future(bad), None, **kw)
    # further rows: the fused fits take them (the engine is told the row count), every other entry wants the exact shape
    assert engine._sketch(rows, width, more_rows, None, **FIT) is more_rows
    for kw in (RSVD, FULL):
        with pytest.raises(ValueError, match=msg):
            engine._sketch(rows, width, more_rows, None, **kw)
    # the panel-level drivers check nothing and cut the columns they use
    om, l = sharded._resolve_sketch(4, rows, 2, more_rows, None)
    assert l == 6 and om.shape == (rows + 5, 6) and om.flags.c_contiguous
    om, l = sharded._resolve_sketch(4, 5, 2, np.arange(30, dtype=np.float64).reshape(5, 6), None)
    assert l == 5 and np.array_equal(om, np.eye(5, dtype=np.float32))
    with pytest.raises(ValueError, match=r"rank of the dataset \(rank = 3\)"):
        sharded._resolve_sketch(4, 3, 2, None, 0)


def test_sketch_propagates_a_failed_draw():
    with pytest.raises(ValueError, match="Seed must be between"):
        engine._sketch(4, 2, engine.SketchFuture(4, 2, -1), None, **RSVD)


# ------------------------------------------------------------------------------------------------ _n_iter_code
def test_n_iter_code():
    for complex_rule in (False, True):
        assert engine._n_iter_code("auto", complex_rule) == -1
        assert engine._n_iter_code(0, complex_rule) == 0
        assert engine._n_iter_code(4, complex_rule) == 4
        assert engine._n_iter_code(np.int64(7), complex_rule) == 7
        assert type(engine._n_iter_code(np.int64(7), complex_rule)) is int
        assert engine._n_iter_code(-1, complex_rule) == -1
    assert engine._n_iter_code(None, True) == -1
    assert engine._n_iter_code("converge", True) == -2
    # the real rule knows neither
    with pytest.raises(TypeError):
        engine._n_iter_code(None)
    with pytest.raises(ValueError):
        engine._n_iter_code("converge")
    with pytest.raises(ValueError):
        engine._n_iter_code("sometimes", True)


# ------------------------------------------------------------------------------------------------ _weights
def test_weights():
    assert engine._weights(None, 5) is None
    w = engine._weights([1, 2, 3], 3)
    assert w.dtype == np.float64 and w.flags.c_contiguous and np.array_equal(w, [1.0, 2.0, 3.0])
    w = engine._weights(np.arange(8, dtype=np.float32)[::2], 4)
    assert w.dtype == np.float64 and w.flags.c_contiguous and np.array_equal(w, [0.0, 2.0, 4.0, 6.0])
    own = np.ones(4)
    assert engine._weights(own, 4) is own
    for bad in (np.ones(3), np.ones(5), np.ones((4, 1)), 1.0):
        with pytest.raises(ValueError, match="^feature_weights must have one entry per stacked feature$"):
            engine._weights(bad, 4)
        with pytest.raises(ValueError, match="^feature_weights must have one entry per stacked feature of the slice$"):
            engine._weights(bad, 4, what="stacked feature of the slice")


# ------------------------------------------------------------------------------------------------ _FitStats
def test_fit_stats_dict():
    st = engine._FitStats(3, 4, True)
    assert len(st.args) == 7
    st.mean[:], st.std[:], st.vf[:], st.vs[:] = 1.5, 2.5, [1, 0, 1, 1], [1, 1, 0]
    st.n.value, st.p.value, st.tv.value = 2, 3, 0.25
    d = st.as_dict()
    assert list(d) == ["mean", "std", "valid_feature", "valid_sample", "n", "p", "total_variance"]
    assert d["mean"].dtype == np.float64 and d["std"].dtype == np.float64
    assert d["valid_feature"].dtype == bool and d["valid_feature"].tolist() == [True, False, True, True]
    assert d["valid_sample"].dtype == bool and d["valid_sample"].tolist() == [True, True, False]
    assert (d["n"], d["p"], d["total_variance"]) == (2, 3, 0.25) and type(d["n"]) is int and type(d["total_variance"]) is float
    d = st.as_dict(fused=True)
    assert list(d)[-1] == "fused" and d["fused"] is True
    # fit_sharded: the keys keep their places when the entry supplies the values
    d = st.as_dict(valid_sample=np.ones(3, bool), n=3, p=9, fused=True)
    assert list(d) == ["mean", "std", "valid_feature", "valid_sample", "n", "p", "total_variance", "fused"]
    assert d["valid_sample"].all() and (d["n"], d["p"]) == (3, 9)
    st = engine._FitStats(3, 4, False)
    assert st.mean is None and st.std is None and st.args[0] is None and st.args[1] is None
    assert st.as_dict()["mean"] is None


# ------------------------------------------------------------------------------------------------ _layout / _collective
class StubLib:
    def __init__(self):
        self.calls = []

    def eofx_ctx_set_layout(self, handle, mode):
        self.calls.append(("layout", handle, mode))

    def eofx_ctx_set_sample_raw(self, handle, flag):
        self.calls.append(("sample_raw", handle, flag))


def stub_ctx():
    return SimpleNamespace(lib=StubLib(), handle="H")


@pytest.mark.parametrize("mode,sample_raw", [(0, False), (1, False), (2, True), (3, False), (3, True)])
def test_layout_sets_and_resets(mode, sample_raw):
    ctx = stub_ctx()
    with engine._layout(ctx, mode, sample_raw=sample_raw):
        assert sorted(ctx.lib.calls) == [("layout", "H", mode), ("sample_raw", "H", int(sample_raw))]
        assert all(type(c[2]) is int for c in ctx.lib.calls)
        ctx.lib.calls.append("body")
    after = ctx.lib.calls[ctx.lib.calls.index("body") + 1:]
    assert sorted(after) == [("layout", "H", 0), ("sample_raw", "H", 0)]


def test_layout_resets_when_the_body_raises():
    ctx = stub_ctx()
    with pytest.raises(KeyError):
        with engine._layout(ctx, 3, sample_raw=True):
            ctx.lib.calls.append("body")
            raise KeyError("boom")
    after = ctx.lib.calls[ctx.lib.calls.index("body") + 1:]
    assert sorted(after) == [("layout", "H", 0), ("sample_raw", "H", 0)]
    # the default leaves the sample-raw flag at 0 throughout
    ctx = stub_ctx()
    with engine._layout(ctx, 2):
        pass
    assert [c for c in ctx.lib.calls if c[0] == "sample_raw"] == [("sample_raw", "H", 0)] * 2


def test_layout_modes_of_the_entries():
    assert engine._layout_mode(False, False, False) == 0 and engine._layout_mode(True, False, False) == 1
    assert engine._layout_mode(False, True, False) == 2 and engine._layout_mode(True, True, False) == 2
    assert engine._layout_mode(False, True, True) == 3 and engine._layout_mode(False, False, True) == 0


def test_collective_stored_exception_wins_over_the_status():
    ctx = stub_ctx()
    ctx._comm_err = RuntimeError("left over from an earlier call")
    with engine._collective(ctx):
        assert ctx._comm_err is None              # cleared on entry
        rc = 0
    assert rc == 0 and ctx._comm_err is None

    boom = KeyError("raised inside the callback communicator")
    reached = []
    with pytest.raises(KeyError) as info:
        with engine._collective(ctx):
            ctx._comm_err = boom                  # what the trampoline of comm_set_callback does, then returns 1
            rc = 7
        reached.append(rc)                        # where the caller would look at the status code
    assert info.value is boom and not reached

    # a context that never had a callback communicator has no slot at all
    bare = SimpleNamespace()
    with engine._collective(bare):
        pass
    assert bare._comm_err is None


def test_collective_outside_layout_resets_the_layout_first():
    """fit_sharded's order: layout back to 0, then the stored exception, and only then the status code"""
    ctx = stub_ctx()
    with pytest.raises(KeyError):
        with engine._collective(ctx), engine._layout(ctx, 3):
            ctx._comm_err = KeyError("boom")
    assert sorted(ctx.lib.calls[-2:]) == [("layout", "H", 0), ("sample_raw", "H", 0)]


def test_trampoline_stores_what_the_callback_raises():
    """comm_set_callback's trampoline is the producer of the slot `_collective` reads"""
    seen = {}

    class Lib:
        def eofx_ctx_comm_set_callback(self, handle, cb, user, world, rank):
            seen["cb"] = cb
            return 0

    ctx = SimpleNamespace(lib=Lib(), handle=None)
    boom = ValueError("rank 1 went away")

    def failing(buf, count, dtype, op, stream):
        raise boom

    engine.comm_set_callback(ctx, failing, 2, 0)
    with pytest.raises(ValueError) as info:
        with engine._collective(ctx):
            rc = seen["cb"](None, None, 4, 0, 0, None)
    assert info.value is boom and rc == 1
    engine.comm_set_callback(ctx, lambda *a: None, 2, 0)
    with engine._collective(ctx):
        assert seen["cb"](None, None, 4, 0, 0, None) == 0
