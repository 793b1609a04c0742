"""Helpers of tests/test_gpu_nonfinite.py: rows and queries that hold a NaN or an Inf, the twin index that holds a deleted
finite row in the place of each, and the comparisons.  Nothing here computes a score: the references are the fp64 oracle and
the numpy restatements the search forms already have."""
import numpy as np

TOL_F64 = 2e-6
PM = 0x00FFFFFF                       # RASS_TAG_PATIENT_MASK
KINDS = ("nan", "inf", "part")


def poison_vec(rng, kind, dim):
    """(vector, normalize): "nan" / "inf" hold one such value and are normalised on the way in, which makes the stored row
    all-NaN; "part" is a unit row with three NaN entries, stored as it is."""
    v = rng.standard_normal(dim).astype(np.float32)
    if kind == "nan":
        v[int(rng.integers(dim))] = np.nan
        return v, True
    if kind == "inf":
        v[int(rng.integers(dim))] = np.inf
        return v, True
    assert kind == "part"
    v /= np.linalg.norm(v)
    v[[3, dim // 3, dim - 2]] = np.nan
    return v, False


def poison_queries(q, where):
    """A copy of ``q`` with the queries ``where`` poisoned: a NaN in the even ones, a +Inf in the odd ones."""
    q = q.copy()
    for j, i in enumerate(where):
        q[i, (7 * j + 5) % q.shape[1]] = np.inf if j % 2 else np.nan
    return q


def twin_vectors(rng, x, poison):
    """(xa, xb, normalize): ``x`` with the rows of ``poison`` ({row: kind}) replaced by poisoned vectors (A) and by random
    unit rows (B); normalize[r] is how row r is added to both."""
    n, dim = x.shape
    xa, xb, norm = x.copy(), x.copy(), np.ones(n, dtype=bool)
    for r in sorted(poison):
        xa[r], norm[r] = poison_vec(rng, poison[r], dim)
        u = rng.standard_normal(dim).astype(np.float32)
        xb[r] = u / np.linalg.norm(u)
    return xa, xb, norm


def add_runs(ix, v, tags, norm, first=0, last=None):
    """Rows [first, last) of ``v`` in ``add`` calls of consecutive rows that share ``normalize``."""
    last = len(v) if last is None else last
    a = first
    while a < last:
        b = a + 1
        while b < last and norm[b] == norm[a]:
            b += 1
        assert ix.add(v[a:b], tags=None if tags is None else tags[a:b], normalize=bool(norm[a])) == a
        a = b


def open_twin(eng, name, xa, xb, norm, tags, poison, dtype="f32"):
    """(A, B) from ``twin_vectors``' output: the same add calls, then delete(row) on B for every poisoned row."""
    A, B = eng.open_index(name + "-A", dtype=dtype), eng.open_index(name + "-B", dtype=dtype)
    add_runs(A, xa, tags, norm)
    add_runs(B, xb, tags, norm)
    for r in sorted(poison):
        B.delete(r)
    return A, B


def build_twin(eng, name, x, tags, poison, rng, dtype="f32"):
    """(A, B, xb, tags_ref): A holds the poisoned rows; B got the same add calls with a random unit row in the place of each,
    then delete(row).  ``xb`` / ``tags_ref`` (-1 on the poisoned rows) are the cleaned corpus of the oracle."""
    xa, xb, norm = twin_vectors(rng, x, poison)
    A, B = open_twin(eng, name, xa, xb, norm, tags, poison, dtype)
    tags_ref = (np.zeros(len(x), dtype=np.int32) if tags is None else tags.copy())
    tags_ref[sorted(poison)] = -1
    return A, B, xb, tags_ref


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(a, b, what=""):
    """Two answers (tuples of arrays) equal bit for bit."""
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    assert len(a) == len(b), what
    for j, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(bits(u), bits(v)), (what, "output %d" % j, np.argwhere(bits(u) != bits(v))[:4].tolist())


def swaps_are_ties(i_gpu, i_ref, all64):
    for q in range(i_ref.shape[0]):
        for a, b in zip(i_gpu[q], i_ref[q]):
            if a != b and (a < 0 or b < 0 or abs(all64[q, a] - all64[q, b]) > 2 * TOL_F64):
                return False
    return True


def no_near_ties(rs, tol=TOL_F64):
    """No two of each query's reference scores (best first, k + 1 of them, -inf padding) within 2 ``tol``: then the ids are
    decided and the tie allowance of ``swaps_are_ties`` is never used."""
    rs = np.asarray(rs, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        gap = rs[:, :-1] - rs[:, 1:]
    return bool(np.all(~(gap <= 2 * tol)))              # inf - inf = NaN past the end: not a tie


def clear_of(thr, all64, tags_ref):
    """No live row scores within 2 TOL_F64 of a finite threshold: the hit set is decided."""
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), (all64.shape[0],))
    live = tags_ref != -1
    return all(not np.isfinite(t) or np.all(np.abs(all64[q, live] - t) > 2 * TOL_F64) for q, t in enumerate(thr))


def check_topk(got, ref, all64, k):
    """(scores, ids) against the oracle's (scores [nq, k + 1], ids): ids equal (swaps only between fp64 near-ties, which
    ``no_near_ties`` excludes), scores within TOL_F64, the same slots filled."""
    s, i = got
    rs, ri = ref
    assert no_near_ties(rs), "reference near-tie: choose another seed"
    rs, ri = rs[:, :k], ri[:, :k]
    assert swaps_are_ties(i, ri, all64), np.argwhere(i != ri)[:4].tolist()
    assert np.array_equal(i >= 0, ri >= 0)
    ok = ri >= 0
    assert np.all(np.abs(s[ok].astype(np.float64) - rs[ok]) <= TOL_F64)
    assert np.all(np.isneginf(s[~ok]))


def empty_rows(out, rows, fills):
    """The queries ``rows`` of every array of ``out`` hold its empty value ``fills[j]``."""
    for a, f in zip(out, fills):
        a = np.asarray(a)[rows]
        assert np.all(np.isneginf(a)) if (isinstance(f, float) and np.isneginf(f)) else np.all(a == f), (a, f)
