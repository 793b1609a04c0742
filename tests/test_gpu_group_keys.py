"""The key-column builders against a numpy restatement (``tests/groupkeys_ref.py``): ``rass_index_keys_from_attr``,
``rass_index_keys_from_attr_edges`` and ``rass_index_attr_minmax``.  Every comparison is ``array_equal``."""
import ctypes

import numpy as np
import pytest

import groupkeys_ref as R

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5          # RASS_ERR_INVALID, RASS_ERR_UNSUPPORTED

DIM = 128
I32_MIN1, I32_MAX = R.MISSING + 1, R.INT32_MAX


def column(rng, n):
    """Values over the whole int32 range with both ends, negatives, small values and ~10 % missing."""
    v = rng.integers(-50, 200, size=n).astype(np.int64)
    wide = rng.random(n) < 0.3
    v[wide] = rng.integers(I32_MIN1, I32_MAX, size=int(wide.sum()), endpoint=True)
    v[rng.random(n) < 0.1] = R.MISSING
    for at, val in zip(rng.permutation(n)[:4], (I32_MIN1, I32_MAX, -1, 0)):
        v[at] = val
    return v.astype(np.int32)


@pytest.fixture(scope="module")
def eng(gpu):
    from rassengine_amd.engine import Engine
    e = Engine(0, DIM)
    yield e
    e.close()


def make_index(eng, name, n, values=None, col=2):
    idx = eng.open_index(name)
    idx.add(np.ones((n, DIM), dtype=np.float32), tags=np.zeros(n, dtype=np.int32), normalize=True)
    if values is not None:
        idx.set_attr(col, 0, values)
    return idx


EDGE_SETS = {
    2: np.array([-10, 100]),
    3: np.array([I32_MIN1, 0, I32_MAX]),
    1000: np.concatenate([np.arange(-60, 939), [I32_MAX]]),
    4097: np.concatenate([np.linspace(I32_MIN1, I32_MAX - 5000, 4096).astype(np.int64), [I32_MAX]]),
}


@pytest.mark.parametrize("n", [1, 31, 33, 1000, 100003])
def test_builders_match_numpy(gpu, eng, n):
    rng = np.random.default_rng(n)
    v = column(rng, n)
    idx = make_index(eng, f"keys-{n}", n, v)
    try:
        for missing in (-1, 0, 5):
            # base 0, a base inside the values, and bases that make v - base overflow int32 in both directions
            for base in (0, -50, 7, I32_MIN1, I32_MAX, -(1 << 31)):
                got = idx.group_keys_from_attr(2, base=base, missing=missing).cpu().numpy()
                assert got.dtype == np.int32 and got.shape[0] >= n + idx.KEY_SLACK_ROWS     # n_keys > rows: the tail is -1
                assert np.array_equal(got, R.keys_from_attr(v, base, missing, got.shape[0])), (missing, base)
            for ne, edges in EDGE_SETS.items():
                assert len(edges) == ne and edges[-1] == I32_MAX or ne == 2
                got = idx.group_keys_from_attr(2, missing=missing, edges=edges).cpu().numpy()
                assert np.array_equal(got, R.keys_from_edges(v, edges, missing, got.shape[0])), (missing, ne)
        # a column never set: every row is missing
        for missing in (-1, 3):
            got = idx.group_keys_from_attr(5, missing=missing).cpu().numpy()
            assert np.all(got[:n] == missing) and np.all(got[n:] == -1)
            got = idx.group_keys_from_attr(5, missing=missing, edges=[0, 1]).cpu().numpy()
            assert np.all(got[:n] == missing) and np.all(got[n:] == -1)
    finally:
        eng.drop_index(idx.name)


def test_builder_refusals_leave_the_buffer_alone(gpu, eng):
    import rassengine_amd._native as N
    n = 1000
    idx = make_index(eng, "keys-refuse", n, column(np.random.default_rng(1), n))
    L = idx._L
    buf = gpu.full((n + 10,), 77, dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()
    p = ctypes.c_void_p(buf.data_ptr())
    ok_edges = np.array([0, 5, 9], dtype=np.int32)
    ep = lambda e: e.ctypes.data_as(ctypes.c_void_p)
    try:
        bad = [
            L.rass_index_keys_from_attr(idx._h, 2, 0, -1, p, n - 1),                       # n_keys < rows
            L.rass_index_keys_from_attr(idx._h, 8, 0, -1, p, n), L.rass_index_keys_from_attr(idx._h, -1, 0, -1, p, n),
            L.rass_index_keys_from_attr(idx._h, 2, 0, -2, p, n),                           # missing_key < -1
            L.rass_index_keys_from_attr_edges(idx._h, 2, ep(ok_edges), 3, -1, p, n - 1),
            L.rass_index_keys_from_attr_edges(idx._h, 2, ep(np.array([0, 5, 5], dtype=np.int32)), 3, -1, p, n),   # not ascending
            L.rass_index_keys_from_attr_edges(idx._h, 2, ep(np.array([3, 2], dtype=np.int32)), 2, -1, p, n),
            L.rass_index_keys_from_attr_edges(idx._h, 2, ep(np.arange(4098, dtype=np.int32)), 4098, -1, p, n),   # too many
            L.rass_index_keys_from_attr_edges(idx._h, 2, ep(ok_edges), 1, -1, p, n),
            L.rass_index_keys_from_attr_edges(idx._h, 2, ep(ok_edges), 3, -2, p, n),
        ]
        assert bad == [INVALID] * len(bad)
        idx.engine.synchronize()
        assert np.all(buf.cpu().numpy() == 77)
        assert L.rass_index_keys_from_attr(idx._h, 2, 0, -1, p, n) == N.RASS_OK            # n_keys == rows: entry n untouched
        idx.engine.synchronize()
        got = buf.cpu().numpy()
        assert np.all(got[n:] == 77) and np.array_equal(got[:n], R.keys_from_attr(idx.get_attr(2, 0, n), 0, -1, n))
        for kw in (dict(col=8), dict(col=-1), dict(missing=-2), dict(base=1 << 31), dict(edges=[1]), dict(edges=[2, 2]),
                   dict(edges=np.arange(4098)), dict(edges=[0.5, 1.5]), dict(edges=[0, 1], base=3)):
            with pytest.raises(ValueError):
                idx.group_keys_from_attr(**dict(dict(col=2), **kw))
    finally:
        eng.drop_index(idx.name)


def test_keys_from_tag(gpu, eng):
    rng = np.random.default_rng(4)
    for n in (1, 33, 5000):
        tags = (rng.integers(0, 1 << 24, size=n) | (rng.integers(0, 128, size=n) << 24)).astype(np.int32)
        idx = eng.open_index(f"keys-tag-{n}")
        idx.add(np.ones((n, DIM), dtype=np.float32), tags=tags, normalize=True)
        dead = rng.permutation(n)[:n // 10]
        for r in dead:
            idx.delete(int(r))
        live = tags.astype(np.int64)
        for mask, shift in ((0x00FFFFFF, 0), (0x7F000000, 24), (0x7FFFFFFF, 0), (0x00000F00, 8)):
            got = idx.group_keys_from_tag(mask).cpu().numpy()
            want = np.full(got.shape[0], -1, dtype=np.int32)
            want[:n] = (live & mask) >> shift
            want[dead] = -1
            assert got.shape[0] == n + idx.KEY_SLACK_ROWS and np.array_equal(got, want), (n, hex(mask))
        buf = gpu.full((n,), 77, dtype=gpu.int32, device="cuda")
        gpu.cuda.synchronize()
        p = ctypes.c_void_p(buf.data_ptr())
        assert [idx._L.rass_index_keys_from_tag(idx._h, m, p, k) for m, k in ((0, n), (-1, n), (0xFF, n - 1))] == [INVALID] * 3
        idx.engine.synchronize()
        assert np.all(buf.cpu().numpy() == 77)
        for bad in (0, -1, 1 << 31):
            with pytest.raises(ValueError):
                idx.group_keys_from_tag(bad)
        eng.drop_index(idx.name)


def test_attr_minmax(gpu, eng):
    n = 5000
    rng = np.random.default_rng(3)
    v = column(rng, n)
    tags = np.zeros(n, dtype=np.int32)
    idx = make_index(eng, "keys-minmax", n, v)
    try:
        assert idx.attr_minmax(2) == R.attr_minmax(v, tags) and idx.attr_minmax(2)[:2] == (I32_MIN1, I32_MAX)
        # the extremes die: a tombstone's value does not count
        for r in np.flatnonzero((v == I32_MIN1) | (v == I32_MAX)):
            idx.delete(int(r))
            tags[r] = -1
        want = R.attr_minmax(v, tags)
        assert idx.attr_minmax(2) == want and want[0] > I32_MIN1 and want[1] < I32_MAX
        assert idx.attr_minmax(4) == (None, None, 0)                                       # never set
        idx.set_attr(4, 0, np.full(n, R.MISSING, dtype=np.int64))
        assert idx.attr_minmax(4) == (None, None, 0)                                       # all missing
        idx.set_attr(4, 17, np.array([-3]))
        assert idx.attr_minmax(4) == (-3, -3, 1)
        with pytest.raises(ValueError):
            idx.attr_minmax(8)
    finally:
        eng.drop_index(idx.name)
    empty = eng.open_index("keys-empty")
    assert empty.attr_minmax(0) == (None, None, 0)
    assert empty.group_keys_from_attr(0).cpu().numpy().tolist() == [-1] * empty.KEY_SLACK_ROWS
    eng.drop_index(empty.name)
