"""Thin object layer over the C ABI: one ``Engine`` per process per GPU, named ``FlatIndex``
objects that live in HBM.  Host arrays are numpy; device-resident entry points take torch
tensors only as (pointer, shape) carriers — torch is plumbing for memory and streams here.
"""
from __future__ import annotations

import ctypes
import threading
from typing import Dict, Optional, Tuple

import numpy as np

from . import _native as N


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def pack_allow(mask: np.ndarray) -> np.ndarray:
    """Boolean row mask(s) -> allow-list bitmap words (``FlatIndex.search_allowed``): ``mask`` is bool [n] or [nb, n]; the
    result is uint32 [ceil(n / 32)] or [nb, ceil(n / 32)] with bit ``r & 31`` of word ``r >> 5`` set where row r is allowed."""
    m = np.asarray(mask, dtype=bool)
    if m.ndim not in (1, 2):
        raise ValueError(f"expected a boolean mask [n] or [nb, n], got shape {m.shape}")
    n = m.shape[-1]
    words = (n + 31) // 32
    padded = np.zeros(m.shape[:-1] + (words * 32,), dtype=bool)
    padded[..., :n] = m
    packed = np.packbits(padded, axis=-1, bitorder="little")
    return np.ascontiguousarray(packed).view("<u4").reshape(m.shape[:-1] + (words,)).astype(np.uint32, copy=False)


def unpack_allow(words: np.ndarray, n: int) -> np.ndarray:
    """The inverse of ``pack_allow``: uint32 words [w] or [nb, w] -> bool [n] or [nb, n] (n <= 32 w)."""
    w = np.ascontiguousarray(np.asarray(words).astype("<u4", copy=False))
    if w.ndim not in (1, 2) or int(n) < 0 or int(n) > w.shape[-1] * 32:
        raise ValueError(f"expected uint32 words [w] or [nb, w] with 32 w >= n, got shape {w.shape} for n = {n}")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (w.shape[-1] * 4,)), axis=-1, bitorder="little")
    return bits[..., :int(n)].astype(bool)


class Engine:
    """Owns one GPU's corpus slabs for the life of the process (SURVEY §8b ownership)."""

    _lock = threading.Lock()
    _singletons: Dict[Tuple[int, int], "Engine"] = {}

    def __init__(self, device: int = 0, dim: int = 1024):
        self._L = N.lib()
        h = ctypes.c_void_p()
        N.check("rass_engine_create", self._L.rass_engine_create(device, dim, ctypes.byref(h)))
        self._h = h
        self.device = device
        self.dim = dim
        self._indices: Dict[str, "FlatIndex"] = {}

    @classmethod
    def get(cls, device: int = 0, dim: int = 1024) -> "Engine":
        """Process-global engine for (device, dim): OpenSearchIndexer is built per request
        (reference app/main.py:2802), so lookups must be O(1)."""
        with cls._lock:
            eng = cls._singletons.get((device, dim))
            if eng is None:
                eng = cls._singletons[(device, dim)] = Engine(device, dim)
            return eng

    def close(self) -> None:
        if self._h:
            with Engine._lock:
                for key, eng in list(Engine._singletons.items()):
                    if eng is self:
                        del Engine._singletons[key]
            self._L.rass_engine_destroy(self._h)
            self._h = None
            self._indices.clear()

    def __del__(self):  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int) -> None:
        """Run engine work on a caller-owned hipStream_t (0 = HIP's null stream, which is
        what ``torch.cuda.current_stream().cuda_stream`` returns for torch's default stream)."""
        N.check("rass_engine_set_stream", self._L.rass_engine_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def reset_stream(self) -> None:
        N.check("rass_engine_reset_stream", self._L.rass_engine_reset_stream(self._h))

    @property
    def stream(self) -> int:
        """The hipStream_t (as int) engine work is enqueued on."""
        return int(self._L.rass_engine_get_stream(self._h) or 0)

    def synchronize(self) -> None:
        N.check("rass_engine_synchronize", self._L.rass_engine_synchronize(self._h))

    def kernel_timing_begin(self, max_launches: int) -> None:
        """Bracket every scan-kernel launch with a hipEvent pair on the engine stream."""
        N.check("rass_engine_kernel_timing_begin", self._L.rass_engine_kernel_timing_begin(self._h, int(max_launches)))

    def kernel_timing_end(self) -> Tuple[float, int]:
        """(summed scan-kernel milliseconds, launches) since ``kernel_timing_begin``."""
        ms = ctypes.c_double(0.0)
        n = ctypes.c_int(0)
        N.check("rass_engine_kernel_timing_end",
                self._L.rass_engine_kernel_timing_end(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def open_index(self, name: str, capacity_rows: int = 0, dtype: str = "f32") -> "FlatIndex":
        """Look up or create the named cosine index (ensure_index_exists, app/main.py:350).  ``dtype``:
        "f32" (the parity path) or "bf16" (a bf16-only corpus: half the HBM, scores within ~1e-3)."""
        idx = self._indices.get(name)
        if idx is not None:
            return idx
        code = {"f32": N.RASS_F32, "bf16": N.RASS_BF16}[dtype]
        h = ctypes.c_void_p()
        N.check("rass_index_open",
                self._L.rass_index_open(self._h, name.encode(), code, int(capacity_rows), ctypes.byref(h)))
        idx = FlatIndex(self, name, h)
        self._indices[name] = idx
        return idx

    def search_multi(self, indices, queries: np.ndarray, k: int, q_filter: Optional[np.ndarray] = None,
                     q_filter_mask: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """CROSS-INDEX batch (``rass_index_search_multi``): query i is answered over ``indices[i]``; queries of
        different per-user indices share scan launches.  Returns (scores f32 [nq,k], ids i64 [nq,k]), ids being
        rows of each query's own index."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim or q.shape[0] != len(indices):
            raise ValueError(f"expected one [{self.dim}] query per index, got {q.shape} for {len(indices)} indices")
        nq = q.shape[0]
        f = None if q_filter is None else np.ascontiguousarray(q_filter, dtype=np.int32)
        m = None if q_filter_mask is None else np.ascontiguousarray(q_filter_mask, dtype=np.int32)
        if (f is not None and f.shape != (nq,)) or (m is not None and (f is None or m.shape != (nq,))):
            raise ValueError("q_filter / q_filter_mask must be one int32 per query (mask needs filter)")
        handles = (ctypes.c_void_p * nq)(*[ix._h for ix in indices])
        out_s = np.empty((nq, int(k)), dtype=np.float32)
        out_i = np.empty((nq, int(k)), dtype=np.int64)
        N.check("rass_index_search_multi",
                self._L.rass_index_search_multi(handles, _np_ptr(q), nq, int(k), _np_ptr(f), _np_ptr(m), _np_ptr(out_s),
                                                _np_ptr(out_i)))
        return out_s, out_i

    def drop_index(self, name: str) -> None:
        N.check("rass_index_drop", self._L.rass_index_drop(self._h, name.encode()))
        self._indices.pop(name, None)

    def load_index(self, name: str, path: str) -> "FlatIndex":
        h = ctypes.c_void_p()
        N.check("rass_index_load", self._L.rass_index_load(self._h, name.encode(), path.encode(), ctypes.byref(h)))
        idx = FlatIndex(self, name, h)
        self._indices[name] = idx
        return idx


class FlatIndex:
    """Row-major fp32 cosine index resident in HBM; row ids are insertion ordinals."""

    def __init__(self, engine: Engine, name: str, handle: ctypes.c_void_p):
        self.engine = engine
        self.name = name
        self._h = handle
        self._L = engine._L

    # ---- bookkeeping
    @property
    def count(self) -> int:
        """Live rows (OpenSearchIndexer.has_any_data's count, app/main.py:1475)."""
        return int(self._L.rass_index_count(self._h))

    @property
    def rows(self) -> int:
        return int(self._L.rass_index_rows(self._h))

    @property
    def dim(self) -> int:
        return int(self._L.rass_index_dim(self._h))

    @property
    def row_stride(self) -> int:
        return int(self._L.rass_index_row_stride(self._h))

    MULTI_MAX_TILES = 65536      # rass_index_search_multi: 32-row tiles per cross-index batch (kMultiMaxItems)

    @property
    def dtype(self) -> str:
        return "bf16" if int(self._L.rass_index_dtype(self._h)) == 1 else "f32"

    @property
    def has_global_ids(self) -> bool:
        return int(self._L.rass_index_has_global_ids(self._h)) != 0

    @property
    def multi_tiles(self) -> int:
        """Tiles this index would take of a cross-index batch's budget; 0 = it cannot join one (bf16 corpus,
        caller-assigned ids, or too large on its own): search it through its own batcher."""
        if self.dtype != "f32" or self.has_global_ids or self.row_stride > 1024:
            return 0
        tiles = max(1, (self.rows + 31) // 32)        # an empty index may join too (it answers with padding)
        return tiles if tiles <= self.MULTI_MAX_TILES // 2 else 0

    @property
    def device_rows_ptr(self) -> int:
        """Device pointer of the tile16 slab (invalidated by growth)."""
        return int(self._L.rass_index_device_rows(self._h) or 0)

    @property
    def device_tags_ptr(self) -> int:
        return int(self._L.rass_index_device_tags(self._h) or 0)

    # ---- write path
    def add(self, vecs: np.ndarray, tags: Optional[np.ndarray] = None, normalize: bool = True,
            first_global_id: int = -1) -> int:
        """Append rows (host fp32 [n, dim]); returns the ORDINAL of the first appended row.
        ``first_global_id`` >= 0: searches report ``first_global_id + i`` for row i of this batch instead
        of its ordinal (a shard of a multi-GPU index, ``rass_index_add_ex``)."""
        v = np.ascontiguousarray(vecs, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"expected [n, {self.dim}] vectors, got {v.shape}")
        t = None
        if tags is not None:
            t = np.ascontiguousarray(tags, dtype=np.int32)
            if t.shape != (v.shape[0],):
                raise ValueError("tags must be one int32 per row")
        first = ctypes.c_int64(-1)
        N.check("rass_index_add_ex", self._L.rass_index_add_ex(self._h, _np_ptr(v), _np_ptr(t), v.shape[0],
                                                              1 if normalize else 0, int(first_global_id), 0,
                                                              ctypes.byref(first)))
        return int(first.value)

    def add_device(self, d_vecs_ptr: int, n: int, d_tags_ptr: int = 0, normalize: bool = True) -> int:
        first = ctypes.c_int64(-1)
        N.check("rass_index_add_device",
                self._L.rass_index_add_device(self._h, ctypes.c_void_p(d_vecs_ptr), ctypes.c_void_p(d_tags_ptr or 0),
                                              int(n), 1 if normalize else 0, ctypes.byref(first)))
        return int(first.value)

    def fill_synthetic(self, n: int, seed: int, row_id_base: int = 0) -> None:
        N.check("rass_index_fill_synthetic",
                self._L.rass_index_fill_synthetic(self._h, int(n), ctypes.c_uint64(seed), int(row_id_base)))

    def delete(self, row: int) -> None:
        N.check("rass_index_delete", self._L.rass_index_delete(self._h, int(row)))

    def compact(self) -> np.ndarray:
        """Remove every tombstoned row on the GPU (``rass_index_compact``): the live rows keep their order and their stored
        bits and take the ordinals 0 .. count-1, and the HBM of the dead ones is returned.  Returns the old -> new ordinal
        map (int64, -1 for a removed row).  Out of place: needs room for the compacted index next to the old one.  Ordinals
        handed out earlier are only valid for the ``layout_epoch`` they were read under."""
        while True:
            new_row = np.empty(self.rows, dtype=np.int64)
            before, after = ctypes.c_int64(-1), ctypes.c_int64(-1)
            rc = self._L.rass_index_compact(self._h, _np_ptr(new_row), new_row.shape[0], ctypes.byref(before), ctypes.byref(after))
            if rc < 0 and before.value > new_row.shape[0]:
                continue            # rows were appended since the map was sized
            N.check("rass_index_compact", rc)
            return new_row[:before.value]

    @property
    def layout_epoch(self) -> int:
        """Compactions that moved rows so far: a row ordinal is only meaningful together with this value."""
        return int(self._L.rass_index_layout_epoch(self._h))

    @property
    def epoch(self) -> Tuple[int, int, int]:
        """(rows, tombstones, layout_epoch): changes whenever a stored answer could (``prefetch.index_epoch``)."""
        rows = self.rows
        return (rows, rows - self.count, self.layout_epoch)

    def get_row(self, row: int) -> np.ndarray:
        out = np.empty(self.dim, dtype=np.float32)
        N.check("rass_index_get_row", self._L.rass_index_get_row(self._h, int(row), _np_ptr(out)))
        return out

    def get_rows(self, first_row: int, n: int) -> np.ndarray:
        """Stored (normalised) rows [first_row, first_row+n) as fp32 [n, dim]."""
        out = np.empty((int(n), self.dim), dtype=np.float32)
        N.check("rass_index_get_rows", self._L.rass_index_get_rows(self._h, int(first_row), int(n), _np_ptr(out)))
        return out

    PREFILTER_MODES = {False: 0, None: 0, 0: 0, "off": 0, True: 1, 1: 1, "bf16": 1, 2: 2, "int8": 2, 3: 3, "int8_exact": 3}

    def set_prefilter(self, enable=True) -> None:
        """Candidate scan over a reduced copy of the slab + exact fp32 re-rank; off by default.
        ``enable``: False / "off", True / "bf16" (half the bytes per pass), "int8" (a quarter) or "int8_exact" (the int8 scan
        with a per-query certificate and an exact fp32 fallback: the flat scan's answers bit for bit, k <= 32)."""
        try:
            mode = self.PREFILTER_MODES[enable]
        except (KeyError, TypeError):
            raise ValueError(f"prefilter mode must be one of off / bf16 / int8 / int8_exact, not {enable!r}") from None
        N.check("rass_index_set_prefilter", self._L.rass_index_set_prefilter(self._h, mode))

    @property
    def prefilter(self) -> bool:
        return bool(self._L.rass_index_get_prefilter(self._h))

    @property
    def prefilter_mode(self) -> str:
        return ("off", "bf16", "int8", "int8_exact")[int(self._L.rass_index_get_prefilter(self._h))]

    def certify_stats(self) -> dict:
        """Mode 3 (int8_exact): queries searched, certified and sent to the fp32 fallback since the mode was set, and the
        certificate's row maxima R and V (synchronises)."""
        q, c, f = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        R, V = ctypes.c_float(0.0), ctypes.c_float(0.0)
        N.check("rass_index_certify_stats",
                self._L.rass_index_certify_stats(self._h, ctypes.byref(q), ctypes.byref(c), ctypes.byref(f),
                                                 ctypes.byref(R), ctypes.byref(V)))
        return {"queries": q.value, "certified": c.value, "fallbacks": f.value, "R": R.value, "V": V.value}

    def candidates_exact_device(self, d_queries, k: int, q_filter=None):
        """Mode 3's parity hook for <= 32 queries on the device (a torch CUDA fp32 tensor [nq, dim]): (candidate scores f32
        [nq, 128], LOCAL rows i64 [nq, 128], tau f32 [nq], certified i32 [nq]) as torch tensors (include/rass_engine.h)."""
        import torch
        nq = int(d_queries.shape[0])
        assert d_queries.is_cuda and d_queries.dtype == torch.float32 and d_queries.is_contiguous() and d_queries.shape[1] == self.dim
        dev = d_queries.device
        s = torch.empty((nq, 128), dtype=torch.float32, device=dev)
        r = torch.empty((nq, 128), dtype=torch.int64, device=dev)
        tau = torch.empty((nq,), dtype=torch.float32, device=dev)
        cert = torch.empty((nq,), dtype=torch.int32, device=dev)
        f = None
        if q_filter is not None:
            f = torch.as_tensor(np.ascontiguousarray(q_filter, dtype=np.int32)).to(dev)
        torch.cuda.current_stream().synchronize()     # the engine works on its own stream
        N.check("rass_index_candidates_exact_device",
                self._L.rass_index_candidates_exact_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), nq, int(k),
                                                           ctypes.c_void_p(f.data_ptr()) if f is not None else None,
                                                           ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(r.data_ptr()),
                                                           ctypes.c_void_p(tau.data_ptr()), ctypes.c_void_p(cert.data_ptr())))
        self.engine.synchronize()
        return s, r, tau, cert

    def sample_floor_device(self, d_queries, k: int, q_filter=None):
        """The sample floor's parity hook for a fused fp32 batch (more than 32 queries on the device, a torch CUDA fp32 tensor
        [nq, dim]): (representative LOCAL rows i32 [nq, 32], their flat-scan scores f32 [nq, 32]) as torch tensors; -1 / -inf
        where a block of the sample has no row the query may rank (include/rass_engine.h)."""
        import torch
        nq = int(d_queries.shape[0])
        assert d_queries.is_cuda and d_queries.dtype == torch.float32 and d_queries.is_contiguous() and d_queries.shape[1] == self.dim
        dev = d_queries.device
        rows = torch.empty((nq, 32), dtype=torch.int32, device=dev)
        scores = torch.empty((nq, 32), dtype=torch.float32, device=dev)
        f = None
        if q_filter is not None:
            f = torch.as_tensor(np.ascontiguousarray(q_filter, dtype=np.int32)).to(dev)
        torch.cuda.current_stream().synchronize()     # the engine works on its own stream
        N.check("rass_index_sample_floor_device",
                self._L.rass_index_sample_floor_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), nq, int(k),
                                                       ctypes.c_void_p(f.data_ptr()) if f is not None else None,
                                                       ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(scores.data_ptr())))
        self.engine.synchronize()
        return rows, scores

    def step_floors_device(self, d_queries, k: int, q_filter=None):
        """Beside sample_floor_device: the one floor per query (f32 [nq], a torch tensor) the batch computes from those 32
        scores for its step-kernel launches (include/rass_engine.h)."""
        import torch
        nq = int(d_queries.shape[0])
        assert d_queries.is_cuda and d_queries.dtype == torch.float32 and d_queries.is_contiguous() and d_queries.shape[1] == self.dim
        dev = d_queries.device
        floors = torch.empty((nq,), dtype=torch.float32, device=dev)
        f = None
        if q_filter is not None:
            f = torch.as_tensor(np.ascontiguousarray(q_filter, dtype=np.int32)).to(dev)
        torch.cuda.current_stream().synchronize()     # the engine works on its own stream
        N.check("rass_index_step_floors_device",
                self._L.rass_index_step_floors_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), nq, int(k),
                                                      ctypes.c_void_p(f.data_ptr()) if f is not None else None,
                                                      ctypes.c_void_p(floors.data_ptr())))
        self.engine.synchronize()
        return floors

    def candidates_device(self, d_queries, q_filter=None):
        """The active prefilter mode's candidate lists BEFORE the exact re-rank, for <= 32 queries on the device (a torch
        CUDA fp32 tensor [nq, dim]): (scores f32 [nq, 32], LOCAL rows i64 [nq, 32]) as torch tensors.  A parity hook: the
        int8 path is integer work and is compared with the oracle bit for bit (tests/test_gpu_prefilter_int8.py)."""
        import torch
        nq = int(d_queries.shape[0])
        assert d_queries.is_cuda and d_queries.dtype == torch.float32 and d_queries.is_contiguous() and d_queries.shape[1] == self.dim
        s = torch.empty((nq, 32), dtype=torch.float32, device=d_queries.device)
        r = torch.empty((nq, 32), dtype=torch.int64, device=d_queries.device)
        f = None
        if q_filter is not None:
            f = torch.as_tensor(np.ascontiguousarray(q_filter, dtype=np.int32)).to(d_queries.device)
        torch.cuda.current_stream().synchronize()     # the engine works on its own stream
        N.check("rass_index_candidates_device",
                self._L.rass_index_candidates_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), nq,
                                                     ctypes.c_void_p(f.data_ptr()) if f is not None else None,
                                                     ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(r.data_ptr())))
        self.engine.synchronize()
        return s, r

    def save(self, path: str) -> None:
        N.check("rass_index_save", self._L.rass_index_save(self._h, path.encode()))

    # ---- read path
    def _queries(self, queries) -> np.ndarray:
        """The queries of a host search as contiguous float32 [nq, dim]."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {q.shape}")
        return q

    @staticmethod
    def _thresholds(min_score, nq: int) -> np.ndarray:
        """``min_score`` (one number, or one per query) as float32 [nq]; NaN refused."""
        thr = np.asarray(min_score)
        if thr.dtype.kind not in "fiu":
            raise ValueError(f"min_score must be real numbers, not {thr.dtype}")
        if thr.ndim == 0:
            thr = np.full(nq, thr)
        thr = np.ascontiguousarray(thr, dtype=np.float32)
        if thr.shape != (nq,):
            raise ValueError("min_score must be one number, or one per query")
        if np.isnan(thr).any():
            raise ValueError("min_score must not be NaN")
        return thr

    @staticmethod
    def _filters(q_filter, q_filter_mask, nq: int) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """``q_filter`` / ``q_filter_mask`` as int32 [nq] each, or None where not given (a mask needs a filter)."""
        f = m = None
        if q_filter is not None:
            f = np.ascontiguousarray(q_filter, dtype=np.int32)
            if f.shape != (nq,):
                raise ValueError("q_filter must be one int32 per query")
        if q_filter_mask is not None:
            if f is None:
                raise ValueError("q_filter_mask needs q_filter")
            m = np.ascontiguousarray(q_filter_mask, dtype=np.int32)
            if m.shape != (nq,):
                raise ValueError("q_filter_mask must be one int32 per query")
        return f, m

    def search(self, queries: np.ndarray, k: int, q_filter: Optional[np.ndarray] = None,
               q_filter_mask: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Exact cosine top-k.  Returns (scores f32 [nq,k], ids i64 [nq,k]); raw cosine, best
        first, ties by id ascending, (-inf, -1) padding.  ``q_filter`` restricts query q to rows whose
        tag equals it (-1 = no filter); with ``q_filter_mask`` to rows with ``(tag & mask) == filter``.
        Any k >= 1: k > 32 is served exactly in passes of 32 (``rass_index_search_ex``).  Thread-safe."""
        q = self._queries(queries)
        f, m = self._filters(q_filter, q_filter_mask, q.shape[0])
        k = int(k)
        out_s = np.empty((q.shape[0], k), dtype=np.float32)
        out_i = np.empty((q.shape[0], k), dtype=np.int64)
        N.check("rass_index_search_ex", self._L.rass_index_search_ex(self._h, _np_ptr(q), q.shape[0], k, _np_ptr(f),
                                                                    _np_ptr(m), _np_ptr(out_s), _np_ptr(out_i)))
        return out_s, out_i

    MAX_HITS = N.RASS_MAX_K_MULTIPASS   # search_range: the longest list one call returns

    def search_range(self, queries: np.ndarray, min_score, max_hits: int = 256, q_filter: Optional[np.ndarray] = None,
                     q_filter_mask: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Score-threshold (radial) search, ``rass_index_search_range``: every live row that passes query q's filter and
        scores ``>= min_score[q]`` (raw cosine; one float32 per query, or one number for all of them; ``-inf`` allowed, NaN
        refused).  Returns (scores f32 [nq, max_hits], ids i64 [nq, max_hits], totals i64 [nq]): the matching rows best
        first, ties by id ascending, (-inf, -1) padding, and the EXACT number of matching rows — where that exceeds
        ``max_hits`` (<= 4096) the list is the best ``max_hits`` of them.  One corpus pass per 32 queries whatever the
        number of hits; always the exact fp32 scan (the prefilter mode is ignored); fp32 indices only.  Thread-safe."""
        q = self._queries(queries)
        nq = q.shape[0]
        thr = self._thresholds(min_score, nq)
        max_hits = int(max_hits)
        if not 1 <= max_hits <= self.MAX_HITS:
            raise ValueError(f"max_hits must be in [1, {self.MAX_HITS}], got {max_hits}")
        f, m = self._filters(q_filter, q_filter_mask, nq)
        out_s = np.empty((nq, max_hits), dtype=np.float32)
        out_i = np.empty((nq, max_hits), dtype=np.int64)
        total = np.empty((nq,), dtype=np.int64)
        N.check("rass_index_search_range",
                self._L.rass_index_search_range(self._h, _np_ptr(q), nq, _np_ptr(thr), max_hits, _np_ptr(f), _np_ptr(m),
                                                _np_ptr(out_s), _np_ptr(out_i), _np_ptr(total)))
        return out_s, out_i, total

    def search_range_device(self, d_queries_ptr: int, nq: int, d_min_score_ptr: int, max_hits: int, d_out_scores_ptr: int,
                            d_out_ids_ptr: int, d_total_ptr: int, id_base: int = 0, d_q_filter_ptr: int = 0,
                            d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_range`` (``rass_index_search_range_device``); nq <= 32.  A query with more
        matches than ``max_hits`` gets the EMPTY list and its exact total; a NaN threshold matches nothing."""
        N.check("rass_index_search_range_device",
                self._L.rass_index_search_range_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq),
                                                       ctypes.c_void_p(d_min_score_ptr), int(max_hits),
                                                       ctypes.c_void_p(d_q_filter_ptr or 0),
                                                       ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                       ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr),
                                                       ctypes.c_void_p(d_total_ptr)))

    MAX_GROUPS = 1 << 20                # search_grouped: the exclusive bound of a group key

    @staticmethod
    def _check_grouped(k, group_mask, n_groups) -> Tuple[int, int, int]:
        k, group_mask, n_groups = int(k), int(group_mask), int(n_groups)
        if not 1 <= k <= N.RASS_MAX_K_MULTIPASS:
            raise ValueError(f"k must be in [1, {N.RASS_MAX_K_MULTIPASS}], got {k}")
        if not 1 <= group_mask <= 0x7FFFFFFF:
            raise ValueError(f"group_mask must be non-zero and within 0x7fffffff, got {group_mask:#x}")
        if not 1 <= n_groups <= FlatIndex.MAX_GROUPS:
            raise ValueError(f"n_groups must be in [1, {FlatIndex.MAX_GROUPS}], got {n_groups}")
        return k, group_mask, n_groups

    def search_grouped(self, queries: np.ndarray, k: int, group_mask: int, n_groups: int, q_filter: Optional[np.ndarray] = None,
                       q_filter_mask: Optional[np.ndarray] = None
                       ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Grouped (collapsed) search, ``rass_index_search_grouped``: the group of a row is
        ``(tag & group_mask) >> ctz(group_mask)`` (``RASS_TAG_PATIENT_MASK``: by patient, ``RASS_TAG_DOCTYPE_MASK``: by doc
        type; group 0 is a group like any other), ``n_groups`` the exclusive bound of that key (<= 1 048 576).  Every group
        with a live row passing query q's filter is represented by its best such row (score desc, row asc).  Returns
        (scores f32 [nq, k], ids i64 [nq, k], groups i32 [nq, k], totals i64 [nq]): the representatives of the k best
        groups, best first, (-inf, -1, -1) padding, and the EXACT number of distinct groups with a matching row.  One corpus
        pass per 32 queries whatever k (<= 4096) is; always the exact fp32 scan (the prefilter mode is ignored); fp32
        indices only.  A matching row whose group key is >= ``n_groups`` makes the call fail.  Thread-safe."""
        q = self._queries(queries)
        nq = q.shape[0]
        k, group_mask, n_groups = self._check_grouped(k, group_mask, n_groups)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        out_s = np.empty((nq, k), dtype=np.float32)
        out_i = np.empty((nq, k), dtype=np.int64)
        out_g = np.empty((nq, k), dtype=np.int32)
        total = np.empty((nq,), dtype=np.int64)
        N.check("rass_index_search_grouped",
                self._L.rass_index_search_grouped(self._h, _np_ptr(q), nq, k, group_mask, n_groups, _np_ptr(f), _np_ptr(m),
                                                  _np_ptr(out_s), _np_ptr(out_i), _np_ptr(out_g), _np_ptr(total)))
        return out_s, out_i, out_g, total

    def search_grouped_device(self, d_queries_ptr: int, nq: int, k: int, group_mask: int, n_groups: int, d_out_scores_ptr: int,
                              d_out_ids_ptr: int, d_out_groups_ptr: int, d_group_total_ptr: int, d_status_ptr: int,
                              id_base: int = 0, d_q_filter_ptr: int = 0, d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_grouped`` (``rass_index_search_grouped_device``); nq <= 32.  ``*d_status`` (one
        int32) ends as 1 when a matching row's group key was >= ``n_groups`` (that row is left out), else 0."""
        k, group_mask, n_groups = self._check_grouped(k, group_mask, n_groups)
        N.check("rass_index_search_grouped_device",
                self._L.rass_index_search_grouped_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), k, group_mask, n_groups,
                                                         ctypes.c_void_p(d_q_filter_ptr or 0),
                                                         ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                         ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr),
                                                         ctypes.c_void_p(d_out_groups_ptr), ctypes.c_void_p(d_group_total_ptr),
                                                         ctypes.c_void_p(d_status_ptr)))

    @staticmethod
    def _check_counts(size, group_mask, n_groups) -> Tuple[int, int, int]:
        size = int(size)
        if not 1 <= size <= N.RASS_MAX_K_MULTIPASS:
            raise ValueError(f"size must be in [1, {N.RASS_MAX_K_MULTIPASS}], got {size}")
        _, group_mask, n_groups = FlatIndex._check_grouped(1, group_mask, n_groups)
        return size, group_mask, n_groups

    def search_counts(self, queries: np.ndarray, min_score, size: int, group_mask: int, n_groups: int,
                      q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None
                      ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Semantic terms aggregation, ``rass_index_aggregate``: the hits of query q are ``search_range``'s (live, filter
        passed, score ``>= min_score[q]``; one float32 per query or one number for all; ``-inf`` allowed, NaN refused), the
        group of a row is ``search_grouped``'s.  Returns (groups i32 [nq, size], counts i64 [nq, size], scores f32
        [nq, size], ids i64 [nq, size], n_buckets i64 [nq], total_hits i64 [nq]): the ``size`` first buckets under (count
        desc, group asc) with the score and id of each bucket's best hit, (-1, 0, -inf, -1) padding, the EXACT number of
        groups with a hit and the EXACT number of hits (``search_range``'s total).  One corpus pass per 32 queries; always
        the exact fp32 scan (the prefilter mode is ignored); fp32 indices only.  A hit whose group key is >= ``n_groups``
        makes the call fail.  Thread-safe."""
        q = self._queries(queries)
        nq = q.shape[0]
        thr = self._thresholds(min_score, nq)
        size, group_mask, n_groups = self._check_counts(size, group_mask, n_groups)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        out_g = np.empty((nq, size), dtype=np.int32)
        out_c = np.empty((nq, size), dtype=np.int64)
        out_s = np.empty((nq, size), dtype=np.float32)
        out_i = np.empty((nq, size), dtype=np.int64)
        n_buckets = np.empty((nq,), dtype=np.int64)
        total = np.empty((nq,), dtype=np.int64)
        N.check("rass_index_aggregate",
                self._L.rass_index_aggregate(self._h, _np_ptr(q), nq, _np_ptr(thr), size, group_mask, n_groups, _np_ptr(f),
                                             _np_ptr(m), _np_ptr(out_g), _np_ptr(out_c), _np_ptr(out_s), _np_ptr(out_i),
                                             _np_ptr(n_buckets), _np_ptr(total)))
        return out_g, out_c, out_s, out_i, n_buckets, total

    def search_counts_device(self, d_queries_ptr: int, nq: int, d_min_score_ptr: int, size: int, group_mask: int, n_groups: int,
                             d_out_groups_ptr: int, d_out_counts_ptr: int, d_out_scores_ptr: int, d_out_ids_ptr: int,
                             d_n_buckets_ptr: int, d_total_hits_ptr: int, d_status_ptr: int, id_base: int = 0,
                             d_q_filter_ptr: int = 0, d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_counts`` (``rass_index_aggregate_device``); nq <= 32.  A NaN threshold matches
        nothing.  ``*d_status`` (one int32) ends as 1 when a hit's group key was >= ``n_groups`` (that hit is left out of
        every figure), else 0."""
        size, group_mask, n_groups = self._check_counts(size, group_mask, n_groups)
        N.check("rass_index_aggregate_device",
                self._L.rass_index_aggregate_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq),
                                                    ctypes.c_void_p(d_min_score_ptr), size, group_mask, n_groups,
                                                    ctypes.c_void_p(d_q_filter_ptr or 0),
                                                    ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                    ctypes.c_void_p(d_out_groups_ptr), ctypes.c_void_p(d_out_counts_ptr),
                                                    ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr),
                                                    ctypes.c_void_p(d_n_buckets_ptr), ctypes.c_void_p(d_total_hits_ptr),
                                                    ctypes.c_void_p(d_status_ptr)))

    # ---- key columns: group and aggregate by any attribute column, optionally within a bitmap
    KEY_NONE = N.RASS_KEY_NONE             # a row in no group
    ERR_INVALID = -1                       # RASS_ERR_INVALID: what a native call answers to a column that is too short
    MAX_KEY_EDGES = N.RASS_MAX_KEY_EDGES   # group_keys_from_attr(edges=...): 4 096 buckets
    KEY_SLACK_ROWS = 2048                  # keys a new column gets beyond ``rows``: rows appended meanwhile still fit

    @staticmethod
    def _check_key_builder(col, base, missing, edges):
        col, base, missing = int(col), int(base), int(missing)
        if not 0 <= col < N.RASS_MAX_ATTRS:
            raise ValueError(f"col must be in [0, {N.RASS_MAX_ATTRS}), got {col}")
        if not -(1 << 31) <= base <= (1 << 31) - 1:
            raise ValueError(f"base must fit int32, got {base}")
        if not -1 <= missing <= (1 << 31) - 1:
            raise ValueError(f"missing must be -1 (no group) or a key >= 0 that fits int32, got {missing}")
        if edges is not None:
            e = np.asarray(edges)
            if e.ndim != 1 or e.dtype.kind not in "iu" or not 2 <= e.shape[0] <= FlatIndex.MAX_KEY_EDGES:
                raise ValueError(f"edges must be 2 .. {FlatIndex.MAX_KEY_EDGES} integers in a 1-d array")
            if int(e.min()) < -(1 << 31) or int(e.max()) > (1 << 31) - 1:
                raise ValueError("edges must fit int32")
            if base != 0:
                raise ValueError("base has no meaning with edges")
            edges = np.ascontiguousarray(e, dtype=np.int32)
            if np.any(edges[1:] <= edges[:-1]):
                raise ValueError("edges must be strictly ascending")
        return col, base, missing, edges

    def group_keys_from_attr(self, col: int, base: int = 0, missing: int = -1, edges=None):
        """A key column from attribute column ``col``: an int32 CUDA tensor of ``rows`` entries plus slack (the surplus reads
        ``KEY_NONE``) that ``search_grouped_by_keys`` / ``search_counts_by_keys`` take.  Without ``edges`` the key of a row
        is ``value - base`` (``rass_index_keys_from_attr``; a result outside [0, 2^31) is ``KEY_NONE``): keyword codes with
        ``base=0``, ints and days with ``base=min``.  With ``edges`` (2 .. 4097 strictly ascending int32) key j means
        ``edges[j] <= value < edges[j + 1]``, a value outside them ``KEY_NONE`` (``rass_index_keys_from_attr_edges``).  A row
        without a value gets ``missing`` (-1: no group).  The column names rows of one ``layout_epoch``; rows appended after
        the call have no group in it."""
        import torch
        col, base, missing, edges = self._check_key_builder(col, base, missing, edges)
        for _ in range(4):
            n = self.rows + self.KEY_SLACK_ROWS
            out = torch.empty((n,), dtype=torch.int32, device=f"cuda:{self.engine.device}")
            torch.cuda.current_stream(out.device).synchronize()     # the engine works on its own stream
            if edges is None:
                fn = "rass_index_keys_from_attr"
                rc = self._L.rass_index_keys_from_attr(self._h, col, base, missing, ctypes.c_void_p(out.data_ptr()), n)
            else:
                fn = "rass_index_keys_from_attr_edges"
                rc = self._L.rass_index_keys_from_attr_edges(self._h, col, _np_ptr(edges), edges.shape[0], missing,
                                                             ctypes.c_void_p(out.data_ptr()), n)
            if rc < 0 and self.rows > n:
                continue            # the index outgrew the slack meanwhile
            N.check(fn, rc)
            self.engine.synchronize()     # the builder ran on the engine's stream: the tensor is complete for torch's too
            return out
        raise RuntimeError(f"{self.name}: the index kept outgrowing the key column under construction")

    def group_keys_from_tag(self, mask: int):
        """The tag-keyed searches' group as a key column (``rass_index_keys_from_tag``): ``(tag & mask) >> ctz(mask)`` per live
        row, ``KEY_NONE`` for a tombstone and in the slack; what ``search_grouped`` / ``search_counts`` group by under that
        mask, for the ``*_by_keys`` calls that also take a bitmap."""
        import torch
        mask = int(mask)
        if not 1 <= mask <= 0x7FFFFFFF:
            raise ValueError(f"mask must be non-zero and within 0x7fffffff, got {mask:#x}")
        for _ in range(4):
            n = self.rows + self.KEY_SLACK_ROWS
            out = torch.empty((n,), dtype=torch.int32, device=f"cuda:{self.engine.device}")
            torch.cuda.current_stream(out.device).synchronize()     # the engine works on its own stream
            rc = self._L.rass_index_keys_from_tag(self._h, mask, ctypes.c_void_p(out.data_ptr()), n)
            if rc == self.ERR_INVALID and self.rows > n:
                continue            # the index outgrew the slack meanwhile
            N.check("rass_index_keys_from_tag", rc)
            self.engine.synchronize()
            return out
        raise RuntimeError(f"{self.name}: the index kept outgrowing the key column under construction")

    def attr_minmax(self, col: int) -> Tuple[Optional[int], Optional[int], int]:
        """(min, max, n_present) of attribute column ``col`` over the live rows that have a value (``rass_index_attr_minmax``:
        one small reduction on the device); (None, None, 0) when no live row has one."""
        col = int(col)
        if not 0 <= col < N.RASS_MAX_ATTRS:
            raise ValueError(f"col must be in [0, {N.RASS_MAX_ATTRS}), got {col}")
        lo, hi, n = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        N.check("rass_index_attr_minmax", self._L.rass_index_attr_minmax(self._h, col, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(n)))
        return (int(lo.value), int(hi.value), int(n.value)) if n.value else (None, None, 0)

    @staticmethod
    def _check_keys(keys, allow, nq: int):
        """The key column and the bitmap of a ``*_by_keys`` call, checked without touching the device."""
        dev_k = not isinstance(keys, np.ndarray) and hasattr(keys, "data_ptr")
        if dev_k:
            if not keys.is_cuda or str(keys.dtype) != "torch.int32" or keys.dim() != 1 or not keys.is_contiguous():
                raise ValueError("a device key column must be a contiguous 1-d int32 CUDA tensor")
        else:
            k = np.asarray(keys)
            if k.ndim != 1 or k.dtype.kind not in "iu":
                raise ValueError(f"keys must be a 1-d integer array or a device key column, got {k.dtype} {k.shape}")
            if k.size and (int(k.min()) < -(1 << 31) or int(k.max()) > (1 << 31) - 1):
                raise ValueError("keys must fit int32")
        if allow is None:
            return
        dev_a = not isinstance(allow, np.ndarray) and hasattr(allow, "data_ptr")
        if dev_a:
            if not allow.is_cuda or str(allow.dtype) != "torch.int32" or not allow.is_contiguous():
                raise ValueError("a device bitmap must be a contiguous int32 CUDA tensor")
        shape = tuple(allow.shape) if dev_a else np.asarray(allow).shape
        if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] not in (1, nq)):
            raise ValueError(f"allow must be [words] (shared) or [nq, words], got {shape} for {nq} queries")

    def _fit_keys(self, keys, allow):
        """``keys`` / ``allow`` on the device and long enough for the index as it is now: a key column shorter than the
        index is padded with ``KEY_NONE`` (rows appended since it was built have no group), a bitmap with zero words."""
        import torch
        dev = torch.device(f"cuda:{self.engine.device}")
        if isinstance(keys, np.ndarray) or not hasattr(keys, "data_ptr"):
            keys = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.int32)).to(dev)
        rows = self.rows
        if keys.shape[0] < rows:
            pad = torch.full((rows + self.KEY_SLACK_ROWS - keys.shape[0],), self.KEY_NONE, dtype=torch.int32, device=dev)
            keys = torch.cat([keys, pad]).contiguous()
        if allow is not None:
            if isinstance(allow, np.ndarray) or not hasattr(allow, "data_ptr"):
                allow = torch.from_numpy(np.ascontiguousarray(allow, dtype=np.uint32).view(np.int32)).to(dev)
            need = (rows + 31) // 32
            if allow.shape[-1] < need:
                pad = need + self.ALLOW_SLACK_WORDS - allow.shape[-1]
                allow = torch.cat([allow, torch.zeros(tuple(allow.shape[:-1]) + (pad,), dtype=torch.int32, device=dev)], dim=-1).contiguous()
        torch.cuda.current_stream(dev).synchronize()     # the engine works on its own stream
        return keys, allow

    @staticmethod
    def _key_call_args(keys, allow):
        n_bitmaps = 0 if allow is None else (1 if allow.dim() == 1 else int(allow.shape[0]))
        return (ctypes.c_void_p(keys.data_ptr()), int(keys.shape[0]),
                ctypes.c_void_p(allow.data_ptr()) if allow is not None else None, n_bitmaps,
                int(allow.shape[-1]) if allow is not None else 0)

    def _by_keys(self, fn: str, keys, allow, call):
        """``call(d_keys, n_keys, d_allow, n_bitmaps, words)`` -> rc with the columns fitted to the index; run again where an
        append outgrew them between the fit and the native call's own check."""
        for _ in range(4):
            k, a = self._fit_keys(keys, allow)
            d_keys, n_keys, d_allow, n_bitmaps, words = self._key_call_args(k, a)
            rc = call(d_keys, n_keys, d_allow, n_bitmaps, words)
            if rc == self.ERR_INVALID and (self.rows > n_keys or (a is not None and self.allow_words > words)):
                continue            # the native check refused columns an append has just outgrown: fit them again
            N.check(fn, rc)
            return
        raise RuntimeError(f"{self.name}: the index kept outgrowing the key column during the search")

    def search_grouped_by_keys(self, queries: np.ndarray, k: int, keys, n_groups: int, allow=None,
                               q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None
                               ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``search_grouped`` with the group of a row taken from a key column (``rass_index_search_grouped_keys``): ``keys`` is
        what ``group_keys_from_attr`` returns, or any int32 per row (numpy is uploaded) — >= 0 the group, negative = the row
        is in no group and is never a match; a key >= ``n_groups`` on a matching row makes the call fail.  ``allow``
        (optional): a bitmap as ``search_allowed`` takes it ([words] shared, [nq, words] one per query; dim <= 1024 only) —
        a row then also needs its bit; the scan still streams the whole index.  Keys or bitmaps shorter than the index are
        padded (no group / not allowed).  Returns what ``search_grouped`` returns; totals count only rows with a group."""
        q = self._queries(queries)
        nq = q.shape[0]
        k, _, n_groups = self._check_grouped(k, 1, n_groups)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        self._check_keys(keys, allow, nq)
        out_s = np.empty((nq, k), dtype=np.float32)
        out_i = np.empty((nq, k), dtype=np.int64)
        out_g = np.empty((nq, k), dtype=np.int32)
        total = np.empty((nq,), dtype=np.int64)
        if nq == 0:
            return out_s, out_i, out_g, total
        fn = "rass_index_search_grouped_keys"
        self._by_keys(fn, keys, allow, lambda d_keys, n_keys, d_allow, n_bitmaps, words: self._L.rass_index_search_grouped_keys(
            self._h, _np_ptr(q), nq, k, d_keys, n_keys, n_groups, d_allow, n_bitmaps, words, _np_ptr(f), _np_ptr(m),
            _np_ptr(out_s), _np_ptr(out_i), _np_ptr(out_g), _np_ptr(total)))
        return out_s, out_i, out_g, total

    def search_grouped_by_keys_device(self, d_queries_ptr: int, nq: int, k: int, d_keys_ptr: int, n_keys: int, n_groups: int,
                                      d_out_scores_ptr: int, d_out_ids_ptr: int, d_out_groups_ptr: int, d_group_total_ptr: int,
                                      d_status_ptr: int, d_allow_ptr: int = 0, n_bitmaps: int = 0, words_per_bitmap: int = 0,
                                      id_base: int = 0, d_q_filter_ptr: int = 0, d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_grouped_by_keys`` (``rass_index_search_grouped_keys_device``); nq <= 32.  Nothing is
        padded: ``n_keys`` below the index's rows is refused.  ``*d_status`` as in ``search_grouped_device``."""
        k, _, n_groups = self._check_grouped(k, 1, n_groups)
        N.check("rass_index_search_grouped_keys_device",
                self._L.rass_index_search_grouped_keys_device(
                    self._h, ctypes.c_void_p(d_queries_ptr), int(nq), k, ctypes.c_void_p(d_keys_ptr), int(n_keys), n_groups,
                    ctypes.c_void_p(d_allow_ptr or 0), int(n_bitmaps), int(words_per_bitmap),
                    ctypes.c_void_p(d_q_filter_ptr or 0), ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                    ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr), ctypes.c_void_p(d_out_groups_ptr),
                    ctypes.c_void_p(d_group_total_ptr), ctypes.c_void_p(d_status_ptr)))

    MAX_GROUP_SIZE = N.RASS_MAX_GROUP_SIZE   # search_group_hits: rows kept per group

    @staticmethod
    def _check_group_hits(k, n_groups, group_size, capped) -> Tuple[int, int, int]:
        k, _, n_groups = FlatIndex._check_grouped(k, 1, n_groups)
        group_size = int(group_size)
        if not 1 <= group_size <= FlatIndex.MAX_GROUP_SIZE:
            raise ValueError(f"group_size must be in [1, {FlatIndex.MAX_GROUP_SIZE}], got {group_size}")
        if n_groups * group_size > FlatIndex.MAX_GROUPS:
            raise ValueError(f"n_groups * group_size must not exceed {FlatIndex.MAX_GROUPS}, got {n_groups} * {group_size}")
        if capped and k * group_size > N.RASS_MAX_K_MULTIPASS:
            raise ValueError(f"the capped list needs k * group_size <= {N.RASS_MAX_K_MULTIPASS}, got {k} * {group_size}")
        return k, n_groups, group_size

    def search_group_hits(self, queries: np.ndarray, k: int, keys, n_groups: int, group_size: int, allow=None,
                          q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None, capped: bool = False):
        """``search_grouped_by_keys`` with inner hits (``rass_index_search_group_hits_keys``): the ``group_size`` best rows of
        each of a query's ``k`` best groups, in one corpus pass.  ``keys`` / ``allow`` / filters as in
        ``search_grouped_by_keys``.  Returns ``(scores [nq, k, group_size], ids, groups [nq, k], totals [nq])``: a group's rows
        best first (score descending, row ascending), ``[q, j, 0]`` being what ``search_grouped_by_keys`` reports at
        ``[q, j]``, ``(-inf, -1)`` past a group's last matching row.  ``capped=True`` appends ``(capped_scores [nq, k],
        capped_ids)``: the exact top-k of all matching rows with at most ``group_size`` rows of any one group (needs
        ``k * group_size <= 4096``).  fp32 indices with dim <= 1024."""
        q = self._queries(queries)
        nq = q.shape[0]
        k, n_groups, group_size = self._check_group_hits(k, n_groups, group_size, capped)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        self._check_keys(keys, allow, nq)
        out_s = np.empty((nq, k, group_size), dtype=np.float32)
        out_i = np.empty((nq, k, group_size), dtype=np.int64)
        out_g = np.empty((nq, k), dtype=np.int32)
        total = np.empty((nq,), dtype=np.int64)
        cap_s = np.empty((nq, k), dtype=np.float32) if capped else None
        cap_i = np.empty((nq, k), dtype=np.int64) if capped else None
        if nq > 0:
            fn = "rass_index_search_group_hits_keys"
            self._by_keys(fn, keys, allow, lambda d_keys, n_keys, d_allow, n_bitmaps, words: self._L.rass_index_search_group_hits_keys(
                self._h, _np_ptr(q), nq, k, d_keys, n_keys, n_groups, group_size, d_allow, n_bitmaps, words, _np_ptr(f), _np_ptr(m),
                _np_ptr(out_s), _np_ptr(out_i), _np_ptr(out_g), _np_ptr(total), _np_ptr(cap_s), _np_ptr(cap_i)))
        return (out_s, out_i, out_g, total, cap_s, cap_i) if capped else (out_s, out_i, out_g, total)

    def search_group_hits_device(self, d_queries_ptr: int, nq: int, k: int, d_keys_ptr: int, n_keys: int, n_groups: int,
                                 group_size: int, d_out_scores_ptr: int, d_out_ids_ptr: int, d_out_groups_ptr: int,
                                 d_group_total_ptr: int, d_status_ptr: int, d_out_capped_scores_ptr: int = 0,
                                 d_out_capped_ids_ptr: int = 0, d_allow_ptr: int = 0, n_bitmaps: int = 0, words_per_bitmap: int = 0,
                                 id_base: int = 0, d_q_filter_ptr: int = 0, d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_group_hits`` (``rass_index_search_group_hits_keys_device``): nq <= 4096 in launch
        groups of 32.  Outputs ``[nq, k, group_size]`` scores / ids, ``[nq, k]`` groups, ``[nq]`` totals and, where both
        capped pointers are given, the ``[nq, k]`` capped list.  Nothing is padded: ``n_keys`` below the index's rows is
        refused.  ``*d_status`` = 1 where a matching row's key was >= ``n_groups``."""
        k, n_groups, group_size = self._check_group_hits(k, n_groups, group_size, bool(d_out_capped_scores_ptr))
        N.check("rass_index_search_group_hits_keys_device",
                self._L.rass_index_search_group_hits_keys_device(
                    self._h, ctypes.c_void_p(d_queries_ptr), int(nq), k, ctypes.c_void_p(d_keys_ptr), int(n_keys), n_groups,
                    group_size, ctypes.c_void_p(d_allow_ptr or 0), int(n_bitmaps), int(words_per_bitmap),
                    ctypes.c_void_p(d_q_filter_ptr or 0), ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                    ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr), ctypes.c_void_p(d_out_groups_ptr),
                    ctypes.c_void_p(d_group_total_ptr), ctypes.c_void_p(d_out_capped_scores_ptr or 0),
                    ctypes.c_void_p(d_out_capped_ids_ptr or 0), ctypes.c_void_p(d_status_ptr)))

    def search_counts_by_keys(self, queries: np.ndarray, min_score, size: int, keys, n_groups: int, allow=None,
                              q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None
                              ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``search_counts`` with the group of a row taken from a key column and, optionally, within a bitmap
        (``rass_index_aggregate_keys``); ``keys`` / ``allow`` as in ``search_grouped_by_keys``.  A row without a group is
        never a hit: it is in no bucket and in neither total.  Returns what ``search_counts`` returns."""
        q = self._queries(queries)
        nq = q.shape[0]
        thr = self._thresholds(min_score, nq)
        size, _, n_groups = self._check_counts(size, 1, n_groups)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        self._check_keys(keys, allow, nq)
        out_g = np.empty((nq, size), dtype=np.int32)
        out_c = np.empty((nq, size), dtype=np.int64)
        out_s = np.empty((nq, size), dtype=np.float32)
        out_i = np.empty((nq, size), dtype=np.int64)
        n_buckets = np.empty((nq,), dtype=np.int64)
        total = np.empty((nq,), dtype=np.int64)
        if nq == 0:
            return out_g, out_c, out_s, out_i, n_buckets, total
        fn = "rass_index_aggregate_keys"
        self._by_keys(fn, keys, allow, lambda d_keys, n_keys, d_allow, n_bitmaps, words: self._L.rass_index_aggregate_keys(
            self._h, _np_ptr(q), nq, _np_ptr(thr), size, d_keys, n_keys, n_groups, d_allow, n_bitmaps, words, _np_ptr(f),
            _np_ptr(m), _np_ptr(out_g), _np_ptr(out_c), _np_ptr(out_s), _np_ptr(out_i), _np_ptr(n_buckets), _np_ptr(total)))
        return out_g, out_c, out_s, out_i, n_buckets, total

    def search_counts_by_keys_device(self, d_queries_ptr: int, nq: int, d_min_score_ptr: int, size: int, d_keys_ptr: int,
                                     n_keys: int, n_groups: int, d_out_groups_ptr: int, d_out_counts_ptr: int,
                                     d_out_scores_ptr: int, d_out_ids_ptr: int, d_n_buckets_ptr: int, d_total_hits_ptr: int,
                                     d_status_ptr: int, d_allow_ptr: int = 0, n_bitmaps: int = 0, words_per_bitmap: int = 0,
                                     id_base: int = 0, d_q_filter_ptr: int = 0, d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_counts_by_keys`` (``rass_index_aggregate_keys_device``); nq <= 32.  Nothing is
        padded.  ``*d_status`` as in ``search_counts_device``."""
        size, _, n_groups = self._check_counts(size, 1, n_groups)
        N.check("rass_index_aggregate_keys_device",
                self._L.rass_index_aggregate_keys_device(
                    self._h, ctypes.c_void_p(d_queries_ptr), int(nq), ctypes.c_void_p(d_min_score_ptr), size,
                    ctypes.c_void_p(d_keys_ptr), int(n_keys), n_groups, ctypes.c_void_p(d_allow_ptr or 0), int(n_bitmaps),
                    int(words_per_bitmap), ctypes.c_void_p(d_q_filter_ptr or 0), ctypes.c_void_p(d_q_filter_mask_ptr or 0),
                    int(id_base), ctypes.c_void_p(d_out_groups_ptr), ctypes.c_void_p(d_out_counts_ptr),
                    ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr), ctypes.c_void_p(d_n_buckets_ptr),
                    ctypes.c_void_p(d_total_hits_ptr), ctypes.c_void_p(d_status_ptr)))

    STATS_ORDERS = {"_count": N.RASS_STATS_BY_COUNT, "value_count": N.RASS_STATS_BY_VALUE_COUNT, "min": N.RASS_STATS_BY_MIN,
                    "max": N.RASS_STATS_BY_MAX}

    @staticmethod
    def _check_stats(value_col, order_by, keys, n_groups) -> Tuple[int, int]:
        value_col = int(value_col)
        if not 0 <= value_col < N.RASS_MAX_ATTRS:
            raise ValueError(f"value_col must be in [0, {N.RASS_MAX_ATTRS}), got {value_col}")
        if order_by not in FlatIndex.STATS_ORDERS:
            raise ValueError(f"order_by must be one of {sorted(FlatIndex.STATS_ORDERS)}, got {order_by!r}")
        if keys is None and int(n_groups) != 1:
            raise ValueError(f"keys=None is the global form: n_groups must be 1, got {n_groups}")
        return value_col, FlatIndex.STATS_ORDERS[order_by]

    def search_stats_by_keys(self, queries: np.ndarray, min_score, size: int, keys, n_groups: int, value_col: int,
                             order_by: str = "_count", descending: bool = True, allow=None,
                             q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None):
        """``search_counts_by_keys`` with a stats sub-aggregation (``rass_index_aggregate_stats_keys``): per listed bucket also
        the count, sum, min and max of attribute column ``value_col`` over the bucket's hits, in the same corpus pass.
        ``keys=None`` with ``n_groups=1`` is the global form (every row in bucket 0).  ``order_by``: ``"_count"``,
        ``"value_count"``, ``"min"`` or ``"max"``, ``descending`` or not; ties by key ascending, buckets without a present
        value last in both directions.  Returns ``(groups, counts, scores, ids, value_counts, sums, mins, maxs, n_buckets,
        total_hits)``: the first four and last two as ``search_counts_by_keys`` (identical to it under ``"_count"``
        descending), the stats ``[nq, size]`` int64 / int64 / int32 / int32 with zeros where a bucket has no present value
        and past the last bucket.  fp32 indices with dim <= 1024."""
        q = self._queries(queries)
        nq = q.shape[0]
        thr = self._thresholds(min_score, nq)
        size, _, n_groups = self._check_counts(size, 1, n_groups)
        value_col, by = self._check_stats(value_col, order_by, keys, n_groups)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        fit = keys if keys is not None else np.zeros(0, dtype=np.int32)
        self._check_keys(fit, allow, nq)
        out_g = np.empty((nq, size), dtype=np.int32)
        out_c = np.empty((nq, size), dtype=np.int64)
        out_s = np.empty((nq, size), dtype=np.float32)
        out_i = np.empty((nq, size), dtype=np.int64)
        out_vc = np.empty((nq, size), dtype=np.int64)
        out_sum = np.empty((nq, size), dtype=np.int64)
        out_min = np.empty((nq, size), dtype=np.int32)
        out_max = np.empty((nq, size), dtype=np.int32)
        n_buckets = np.empty((nq,), dtype=np.int64)
        total = np.empty((nq,), dtype=np.int64)
        if nq > 0:
            fn = "rass_index_aggregate_stats_keys"
            self._by_keys(fn, fit, allow, lambda d_keys, n_keys, d_allow, n_bitmaps, words: self._L.rass_index_aggregate_stats_keys(
                self._h, _np_ptr(q), nq, _np_ptr(thr), size, d_keys if keys is not None else None, n_keys, n_groups, value_col, by,
                1 if descending else 0, d_allow, n_bitmaps, words, _np_ptr(f), _np_ptr(m), _np_ptr(out_g), _np_ptr(out_c),
                _np_ptr(out_s), _np_ptr(out_i), _np_ptr(out_vc), _np_ptr(out_sum), _np_ptr(out_min), _np_ptr(out_max),
                _np_ptr(n_buckets), _np_ptr(total)))
        return out_g, out_c, out_s, out_i, out_vc, out_sum, out_min, out_max, n_buckets, total

    def search_stats_by_keys_device(self, d_queries_ptr: int, nq: int, d_min_score_ptr: int, size: int, d_keys_ptr: int,
                                    n_keys: int, n_groups: int, value_col: int, d_out_groups_ptr: int, d_out_counts_ptr: int,
                                    d_out_scores_ptr: int, d_out_ids_ptr: int, d_out_value_counts_ptr: int, d_out_sums_ptr: int,
                                    d_out_mins_ptr: int, d_out_maxs_ptr: int, d_n_buckets_ptr: int, d_total_hits_ptr: int,
                                    d_status_ptr: int, order_by: str = "_count", descending: bool = True, d_allow_ptr: int = 0,
                                    n_bitmaps: int = 0, words_per_bitmap: int = 0, id_base: int = 0, d_q_filter_ptr: int = 0,
                                    d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_stats_by_keys`` (``rass_index_aggregate_stats_keys_device``); nq <= 32.
        ``d_keys_ptr`` 0 with ``n_groups`` 1 is the global form.  Nothing is padded.  ``*d_status`` as in
        ``search_counts_device``."""
        size, _, n_groups = self._check_counts(size, 1, n_groups)
        value_col, by = self._check_stats(value_col, order_by, d_keys_ptr or None, n_groups)
        N.check("rass_index_aggregate_stats_keys_device",
                self._L.rass_index_aggregate_stats_keys_device(
                    self._h, ctypes.c_void_p(d_queries_ptr), int(nq), ctypes.c_void_p(d_min_score_ptr), size,
                    ctypes.c_void_p(d_keys_ptr or 0), int(n_keys), n_groups, value_col, by, 1 if descending else 0,
                    ctypes.c_void_p(d_allow_ptr or 0), int(n_bitmaps), int(words_per_bitmap),
                    ctypes.c_void_p(d_q_filter_ptr or 0), ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                    ctypes.c_void_p(d_out_groups_ptr), ctypes.c_void_p(d_out_counts_ptr), ctypes.c_void_p(d_out_scores_ptr),
                    ctypes.c_void_p(d_out_ids_ptr), ctypes.c_void_p(d_out_value_counts_ptr), ctypes.c_void_p(d_out_sums_ptr),
                    ctypes.c_void_p(d_out_mins_ptr), ctypes.c_void_p(d_out_maxs_ptr), ctypes.c_void_p(d_n_buckets_ptr),
                    ctypes.c_void_p(d_total_hits_ptr), ctypes.c_void_p(d_status_ptr)))

    AGG_ORDERS = {"_count": N.RASS_AGG_BY_COUNT, "max_score": N.RASS_AGG_BY_SCORE}

    @staticmethod
    def _check_counts_hits(size, n_groups, top_hits, order_by) -> Tuple[int, int, int, int]:
        size, _, n_groups = FlatIndex._check_counts(size, 1, n_groups)
        top_hits = int(top_hits)
        if not 1 <= top_hits <= FlatIndex.MAX_GROUP_SIZE:
            raise ValueError(f"top_hits must be in [1, {FlatIndex.MAX_GROUP_SIZE}], got {top_hits}")
        if n_groups * top_hits > FlatIndex.MAX_GROUPS:
            raise ValueError(f"n_groups * top_hits must not exceed {FlatIndex.MAX_GROUPS}, got {n_groups} * {top_hits}")
        if order_by not in FlatIndex.AGG_ORDERS:
            raise ValueError(f"order_by must be one of {sorted(FlatIndex.AGG_ORDERS)}, got {order_by!r}")
        return size, n_groups, top_hits, FlatIndex.AGG_ORDERS[order_by]

    def search_counts_hits_by_keys(self, queries: np.ndarray, min_score, size: int, keys, n_groups: int, top_hits: int,
                                   order_by: str = "_count", allow=None, q_filter: Optional[np.ndarray] = None,
                                   q_filter_mask: Optional[np.ndarray] = None):
        """``search_counts_by_keys`` with a top_hits sub-aggregation (``rass_index_aggregate_hits_keys``): per listed bucket
        also its ``top_hits`` best hits, in the same corpus pass.  ``order_by``: ``"_count"`` (doc_count descending, then key
        ascending: ``search_counts_by_keys``' order) or ``"max_score"`` (by each bucket's best hit).  ``keys`` / ``allow`` /
        filters as in ``search_counts_by_keys``.  Returns ``(groups [nq, size], counts, scores [nq, size, top_hits], ids,
        n_buckets [nq], total_hits)``: a bucket's hits best first (score descending, row ascending), ``(-inf, -1)`` past its
        last hit, ``(-1, 0, -inf, -1)`` past the last bucket.  fp32 indices with dim <= 1024."""
        q = self._queries(queries)
        nq = q.shape[0]
        thr = self._thresholds(min_score, nq)
        size, n_groups, top_hits, by = self._check_counts_hits(size, n_groups, top_hits, order_by)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        self._check_keys(keys, allow, nq)
        out_g = np.empty((nq, size), dtype=np.int32)
        out_c = np.empty((nq, size), dtype=np.int64)
        out_s = np.empty((nq, size, top_hits), dtype=np.float32)
        out_i = np.empty((nq, size, top_hits), dtype=np.int64)
        n_buckets = np.empty((nq,), dtype=np.int64)
        total = np.empty((nq,), dtype=np.int64)
        if nq > 0:
            fn = "rass_index_aggregate_hits_keys"
            self._by_keys(fn, keys, allow, lambda d_keys, n_keys, d_allow, n_bitmaps, words: self._L.rass_index_aggregate_hits_keys(
                self._h, _np_ptr(q), nq, _np_ptr(thr), size, d_keys, n_keys, n_groups, top_hits, by, d_allow, n_bitmaps, words,
                _np_ptr(f), _np_ptr(m), _np_ptr(out_g), _np_ptr(out_c), _np_ptr(out_s), _np_ptr(out_i), _np_ptr(n_buckets),
                _np_ptr(total)))
        return out_g, out_c, out_s, out_i, n_buckets, total

    def search_counts_hits_by_keys_device(self, d_queries_ptr: int, nq: int, d_min_score_ptr: int, size: int, d_keys_ptr: int,
                                          n_keys: int, n_groups: int, top_hits: int, d_out_groups_ptr: int, d_out_counts_ptr: int,
                                          d_out_scores_ptr: int, d_out_ids_ptr: int, d_n_buckets_ptr: int, d_total_hits_ptr: int,
                                          d_status_ptr: int, order_by: str = "_count", d_allow_ptr: int = 0, n_bitmaps: int = 0,
                                          words_per_bitmap: int = 0, id_base: int = 0, d_q_filter_ptr: int = 0,
                                          d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_counts_hits_by_keys`` (``rass_index_aggregate_hits_keys_device``); nq <= 32.
        Outputs ``[nq, size]`` groups / counts, ``[nq, size, top_hits]`` scores / ids, ``[nq]`` n_buckets / total_hits.
        Nothing is padded.  ``*d_status`` as in ``search_counts_device``."""
        size, n_groups, top_hits, by = self._check_counts_hits(size, n_groups, top_hits, order_by)
        N.check("rass_index_aggregate_hits_keys_device",
                self._L.rass_index_aggregate_hits_keys_device(
                    self._h, ctypes.c_void_p(d_queries_ptr), int(nq), ctypes.c_void_p(d_min_score_ptr), size,
                    ctypes.c_void_p(d_keys_ptr or 0), int(n_keys), n_groups, top_hits, by, ctypes.c_void_p(d_allow_ptr or 0),
                    int(n_bitmaps), int(words_per_bitmap), ctypes.c_void_p(d_q_filter_ptr or 0),
                    ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base), ctypes.c_void_p(d_out_groups_ptr),
                    ctypes.c_void_p(d_out_counts_ptr), ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr),
                    ctypes.c_void_p(d_n_buckets_ptr), ctypes.c_void_p(d_total_hits_ptr), ctypes.c_void_p(d_status_ptr)))

    # ---- allow-list search: exact top-k within a per-query row bitmap
    @property
    def allow_words(self) -> int:
        """uint32 words a bitmap of this index needs now: ceil(rows / 32)."""
        return (self.rows + 31) // 32

    ALLOW_SLACK_WORDS = 64       # words a new bitmap gets beyond ceil(rows / 32): rows appended meanwhile (2 048 of them) still fit

    def _build_bitmap(self, fn: str, call, n_bitmaps: Optional[int] = None, words: Optional[int] = None):
        """A device bitmap sized for the index as it is NOW plus slack, filled by ``call(tensor)`` (a native builder).  The
        index may grow between reading ``rows`` here and the builder's own check: the slack absorbs that, and a builder that
        still finds the bitmap too short is given a fresh, longer one.  Surplus words allow nothing."""
        import torch
        for _ in range(4):
            fixed, words = words, (self.allow_words + self.ALLOW_SLACK_WORDS if words is None else int(words))
            out = torch.empty((words,) if n_bitmaps is None else (n_bitmaps, words), dtype=torch.int32,
                              device=f"cuda:{self.engine.device}")
            rc = call(out)
            if rc < 0 and self.allow_words > words and fixed is None:
                words = None
                continue            # the index outgrew the slack meanwhile
            N.check(fn, rc)
            return out
        raise RuntimeError(f"{self.name}: the index kept outgrowing the bitmap under construction")

    def allow_from_rows(self, rows):
        """A device bitmap (torch int32 CUDA tensor holding the uint32 words, ``allow_words`` of them plus slack) allowing
        exactly the given row ordinals (``rass_index_allow_from_rows``): ids outside [0, rows) are ignored, duplicates are
        fine.  It belongs to the layout epoch it was built under; rows appended later are not allowed by it."""
        r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
        return self._build_bitmap("rass_index_allow_from_rows", lambda out: self._L.rass_index_allow_from_rows(
            self._h, _np_ptr(r), r.shape[0], ctypes.c_void_p(out.data_ptr()), out.shape[0]))

    def allow_from_tag_values(self, values, mask: int, words: Optional[int] = None):
        """A device bitmap allowing every live row whose ``(tag & mask)`` is one of ``values`` (``rass_index_allow_from_tag_values``):
        OpenSearch's ``terms`` filter.  ``mask``: ``RASS_TAG_PATIENT_MASK`` (values = patient codes), ``RASS_TAG_DOCTYPE_MASK``
        (values = codes << 24) or both.  Rows appended after the call are not allowed by it."""
        v = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.int32)
        mask = int(mask)
        if not 0 <= mask <= 0x7FFFFFFF:
            raise ValueError(f"mask must be within 0x7fffffff, got {mask:#x}")
        return self._build_bitmap("rass_index_allow_from_tag_values", lambda out: self._L.rass_index_allow_from_tag_values(
            self._h, _np_ptr(v), v.shape[0], mask, ctypes.c_void_p(out.data_ptr()), out.shape[0]), words=words)

    # ---- attribute columns and the predicates over them
    ATTR_MISSING = N.RASS_ATTR_MISSING
    ATTR_MODES = {"all": N.RASS_ATTR_ALL, "any": N.RASS_ATTR_ANY}
    ATTR_COMBINES = {"replace": N.RASS_ATTR_REPLACE, "and": N.RASS_ATTR_AND, "or": N.RASS_ATTR_OR}

    def set_attr(self, col: int, first_row: int, values) -> None:
        """Store int32 ``values`` in attribute column ``col`` (0 .. 7) for rows [first_row, first_row + len(values)), which
        must exist (``rass_index_set_attr``).  The column is allocated, all ``ATTR_MISSING``, on its first use; storing
        ``ATTR_MISSING`` un-sets a value.  Rows appended by ``add`` read missing until they are set here."""
        v = np.asarray(values)
        if v.dtype.kind not in "iu" or v.ndim != 1:
            raise ValueError(f"values must be a 1-d integer array, got {v.dtype} {v.shape}")
        if v.size and (int(v.min()) < -(1 << 31) or int(v.max()) > (1 << 31) - 1):
            raise OverflowError("attribute values must fit int32")
        v = np.ascontiguousarray(v, dtype=np.int32)
        N.check("rass_index_set_attr", self._L.rass_index_set_attr(self._h, int(col), int(first_row), v.shape[0], _np_ptr(v)))

    def get_attr(self, col: int, first_row: int, n: int) -> np.ndarray:
        """Column ``col`` of rows [first_row, first_row + n) as int32 [n]; a column never set reads all ``ATTR_MISSING``."""
        out = np.empty(int(n), dtype=np.int32)
        N.check("rass_index_get_attr", self._L.rass_index_get_attr(self._h, int(col), int(first_row), int(n), _np_ptr(out)))
        return out

    @property
    def attr_mask(self) -> int:
        """Bit c set iff attribute column c is allocated (``rass_index_attr_mask``)."""
        return int(N.check("rass_index_attr_mask", self._L.rass_index_attr_mask(self._h)))

    def device_attr_ptr(self, col: int) -> int:
        return int(self._L.rass_index_device_attr(self._h, int(col)) or 0)

    def allow_from_attr_clauses(self, clauses, nq: int = 1, shared: bool = False, mode: str = "all", combine: str = "replace",
                                allow=None):
        """Device bitmaps from predicates over the attribute columns (``rass_index_allow_from_attr_clauses``).  ``clauses``:
        int32 [n, 5] rows ``(query, col, lo, hi, negate)``; a clause holds where the row's value v in ``col`` is not missing
        and lo <= v <= hi, inverted under ``negate`` (a missing value then passes).  ``mode`` "all": query q allows a live
        row iff all of its clauses hold (none: every live row); "any": iff one does (none: no row).  At most 64 clauses per
        query per call.  ``shared``: ONE bitmap for every query (the clauses name query 0).  With ``allow=None`` a new
        tensor is returned — int32 CUDA [words] when shared, else [nq, words], words = ``allow_words`` plus slack — and
        ``combine`` must be "replace"; otherwise ``allow`` (such a tensor, e.g. from ``allow_from_tag_values``) is refined in
        place with ``combine`` "replace" / "and" / "or" and returned.  The result is what ``search_allowed`` /
        ``search_allowed_device`` take; it names rows of one ``layout_epoch``."""
        import torch
        c = np.ascontiguousarray(np.asarray(clauses, dtype=np.int64).reshape(-1, 5))
        if c.size and (int(c.min()) < -(1 << 31) or int(c.max()) > (1 << 31) - 1):
            raise OverflowError("clause fields must fit int32")
        c = np.ascontiguousarray(c, dtype=np.int32)
        nq, n_bitmaps = int(nq), 1 if shared else int(nq)
        try:
            mode_c, comb_c = self.ATTR_MODES[mode], self.ATTR_COMBINES[combine]
        except KeyError:
            raise ValueError(f"mode must be all / any and combine replace / and / or, not {mode!r} / {combine!r}") from None
        fn = "rass_index_allow_from_attr_clauses"

        def call(out) -> int:
            words = int(out.shape[-1])
            torch.cuda.current_stream(out.device).synchronize()     # the engine works on its own stream
            return self._L.rass_index_allow_from_attr_clauses(self._h, _np_ptr(c), c.shape[0], nq, n_bitmaps, mode_c, comb_c,
                                                              ctypes.c_void_p(out.data_ptr()), words)
        if allow is None:
            if comb_c != N.RASS_ATTR_REPLACE:
                raise ValueError("combine 'and' / 'or' needs the bitmap to refine (allow=...)")
            return self._build_bitmap(fn, call, None if shared else n_bitmaps)
        if not allow.is_cuda or allow.dtype != torch.int32 or not allow.is_contiguous():
            raise ValueError("a device bitmap must be a contiguous int32 CUDA tensor")
        if tuple(allow.shape[:-1]) not in (((), (1,)) if shared else ((n_bitmaps,),) + (((),) if n_bitmaps == 1 else ())):
            raise ValueError(f"allow has shape {tuple(allow.shape)} for {n_bitmaps} bitmap(s)")
        N.check(fn, call(allow))
        return allow

    def allow_combine(self, dst, src, op: str):
        """``dst`` = ``dst`` and / or / andnot ``src`` word for word, in place (``rass_index_allow_combine``): two device
        bitmaps of one shape, as the builders return them.  Returns ``dst``."""
        import torch
        ops = {"and": N.RASS_ATTR_AND, "or": N.RASS_ATTR_OR, "andnot": N.RASS_ATTR_ANDNOT}
        if op not in ops:
            raise ValueError(f"op must be and / or / andnot, not {op!r}")
        for t in (dst, src):
            if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
                raise ValueError("a device bitmap must be a contiguous int32 CUDA tensor")
        if tuple(dst.shape) != tuple(src.shape) or dst.data_ptr() == src.data_ptr():
            raise ValueError(f"dst {tuple(dst.shape)} and src {tuple(src.shape)} must be two bitmaps of one shape")
        torch.cuda.current_stream(dst.device).synchronize()     # the engine works on its own stream
        N.check("rass_index_allow_combine", self._L.rass_index_allow_combine(
            self._h, ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), int(dst.numel()), ops[op]))
        return dst

    def allow_plan(self, allow, nq: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The work list an allowed search of one launch group of ``nq`` <= 32 queries walks (``rass_index_allow_plan``), for
        tests and tools: (tile i32 [n], rows i32 [n], mask u32 [n]), tiles ascending.  ``allow``: a device bitmap ([words]
        shared, or [nq, words])."""
        n_bitmaps, words = (1, allow.shape[0]) if allow.dim() == 1 else (allow.shape[0], allow.shape[1])
        cap = max(self.allow_words, 1)
        tile, rows, mask = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.uint32)
        n = ctypes.c_int64(0)
        N.check("rass_index_allow_plan",
                self._L.rass_index_allow_plan(self._h, ctypes.c_void_p(allow.data_ptr()), int(n_bitmaps), int(words), int(nq),
                                              _np_ptr(tile), _np_ptr(rows), _np_ptr(mask), cap, ctypes.byref(n)))
        return tile[:n.value], rows[:n.value], mask[:n.value]

    def allow_count(self, allow) -> np.ndarray:
        """How many rows each bitmap names: its set bits below ``rows``, tombstoned rows included (``rass_index_allow_count``),
        int64 [n_bitmaps] ([1] for a shared bitmap).  ``allow`` as ``search_allowed`` takes it: numpy uint32 words or a device
        bitmap, [words] or [n, words], words >= ``allow_words``."""
        import torch
        on_device = not isinstance(allow, np.ndarray) and hasattr(allow, "data_ptr")
        if on_device:
            if not allow.is_cuda or allow.dtype != torch.int32 or not allow.is_contiguous():
                raise ValueError("a device bitmap must be a contiguous int32 CUDA tensor")
            d = allow
        else:
            a = np.ascontiguousarray(allow, dtype=np.uint32)
            d = torch.from_numpy(a.view(np.int32)).to(f"cuda:{self.engine.device}")
        if d.dim() not in (1, 2):
            raise ValueError(f"allow must be [words] or [n, words], got {tuple(d.shape)}")
        n_bitmaps, words = (1, int(d.shape[0])) if d.dim() == 1 else (int(d.shape[0]), int(d.shape[1]))
        out = np.zeros(n_bitmaps, dtype=np.int64)
        if n_bitmaps == 0:
            return out
        torch.cuda.current_stream(d.device).synchronize()     # the engine works on its own stream
        N.check("rass_index_allow_count",
                self._L.rass_index_allow_count(self._h, ctypes.c_void_p(d.data_ptr()), n_bitmaps, words, _np_ptr(out)))
        return out

    def search_allowed(self, queries: np.ndarray, k: int, allow, q_filter: Optional[np.ndarray] = None,
                       q_filter_mask: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Exact cosine top-k among the rows a bitmap allows (``rass_index_search_allowed``).  ``allow``: uint32 words
        (``pack_allow``) as a numpy array, or a device bitmap from ``allow_from_rows`` / ``allow_from_tag_values``; shape
        [words] = one bitmap shared by every query, [nq, words] = one per query; words >= ``allow_words``.  A row matches
        when it is live, passes ``q_filter`` / ``q_filter_mask`` as in ``search`` and has its bit set.  Returns (scores f32
        [nq, k], ids i64 [nq, k]) as ``search`` does: best first, ties by id ascending, (-inf, -1) padding; k <= 4096, nq
        <= 4096.  The scan streams only the 32-row tiles with a bit set.  fp32 indices with dim <= 1024; the prefilter mode
        is ignored.  A bitmap names rows of one ``layout_epoch``.  Thread-safe."""
        q = self._queries(queries)
        nq, k = q.shape[0], int(k)
        if not 1 <= k <= N.RASS_MAX_K_MULTIPASS:
            raise ValueError(f"k must be in [1, {N.RASS_MAX_K_MULTIPASS}], got {k}")
        if nq > N.RASS_MAX_DEVICE_BATCH:
            raise ValueError(f"at most {N.RASS_MAX_DEVICE_BATCH} queries per call, got {nq}")
        f, m = self._filters(q_filter, q_filter_mask, nq)
        on_device = not isinstance(allow, np.ndarray) and hasattr(allow, "data_ptr")
        if not on_device:
            allow = np.ascontiguousarray(allow, dtype=np.uint32)
        shape = tuple(allow.shape)
        if len(shape) not in (1, 2) or (len(shape) == 2 and shape[0] not in (1, nq)):
            raise ValueError(f"allow must be [words] (shared) or [nq, words], got {shape} for {nq} queries")
        out_s = np.empty((nq, k), dtype=np.float32)
        out_i = np.empty((nq, k), dtype=np.int64)
        if nq == 0:
            return out_s, out_i
        if on_device:
            import torch
            if not allow.is_cuda or allow.dtype != torch.int32 or not allow.is_contiguous():
                raise ValueError("a device bitmap must be a contiguous int32 CUDA tensor")
            dev = allow.device
            dq = torch.from_numpy(q).to(dev)
            df = torch.from_numpy(f).to(dev) if f is not None else None
            dm = torch.from_numpy(m).to(dev) if m is not None else None
            ds = torch.empty((nq, k), dtype=torch.float32, device=dev)
            di = torch.empty((nq, k), dtype=torch.int64, device=dev)
        # A bitmap speaks for the rows the index had when it was made.  Rows appended since (an ingest may land between the
        # build and this search; the layout epoch does not move on an append) are not allowed by it: the bitmap is extended
        # with zero words to what the index needs now, plus slack for rows that land before the native call's own check.
        for _ in range(4):
            words = int(allow.shape[-1])
            need = self.allow_words
            if words < need:
                pad = need + self.ALLOW_SLACK_WORDS - words
                if on_device:
                    allow = torch.cat([allow, torch.zeros(tuple(allow.shape[:-1]) + (pad,), dtype=torch.int32, device=dev)], dim=-1).contiguous()
                else:
                    allow = np.ascontiguousarray(np.concatenate([allow, np.zeros(allow.shape[:-1] + (pad,), dtype=np.uint32)], axis=-1))
                words = int(allow.shape[-1])
            n_bitmaps = 1 if allow.ndim == 1 else int(allow.shape[0])
            if on_device:
                torch.cuda.current_stream(dev).synchronize()     # the engine works on its own stream
                rc = self._L.rass_index_search_allowed_device(
                    self._h, ctypes.c_void_p(dq.data_ptr()), nq, k, ctypes.c_void_p(allow.data_ptr()), n_bitmaps, words,
                    ctypes.c_void_p(df.data_ptr()) if df is not None else None,
                    ctypes.c_void_p(dm.data_ptr()) if dm is not None else None, 0, ctypes.c_void_p(ds.data_ptr()),
                    ctypes.c_void_p(di.data_ptr()))
            else:
                rc = self._L.rass_index_search_allowed(self._h, _np_ptr(q), nq, k, _np_ptr(allow), n_bitmaps, words, _np_ptr(f),
                                                       _np_ptr(m), _np_ptr(out_s), _np_ptr(out_i))
            if rc < 0 and self.allow_words > words:
                continue            # the index outgrew the slack between the two checks: extend again
            N.check("rass_index_search_allowed_device" if on_device else "rass_index_search_allowed", rc)
            if on_device:
                self.engine.synchronize()
                return ds.cpu().numpy(), di.cpu().numpy()
            return out_s, out_i
        raise RuntimeError(f"{self.name}: the index kept outgrowing the bitmap during the search")

    def search_allowed_device(self, d_queries_ptr: int, nq: int, k: int, d_allow_ptr: int, n_bitmaps: int, words_per_bitmap: int,
                              d_out_scores_ptr: int, d_out_ids_ptr: int, id_base: int = 0, d_q_filter_ptr: int = 0,
                              d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_allowed`` (``rass_index_search_allowed_device``): nq <= 4096 in launch groups of
        32, k <= 4096 (every pass enqueued by the one call)."""
        N.check("rass_index_search_allowed_device",
                self._L.rass_index_search_allowed_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), int(k),
                                                         ctypes.c_void_p(d_allow_ptr), int(n_bitmaps), int(words_per_bitmap),
                                                         ctypes.c_void_p(d_q_filter_ptr or 0),
                                                         ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                         ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr)))

    # ---- boosted search: exact top-k of boost * T(cos) + a per-row bonus column
    BONUS_SLACK_ROWS = 2048      # cells a new column gets beyond the rows: rows appended meanwhile still fit (and read 0)
    BOOST_TRANSFORMS = {"raw": N.RASS_BOOST_RAW, "opensearch": N.RASS_BOOST_OPENSEARCH}
    BONUS_OPS = {"replace": N.RASS_BONUS_REPLACE, "add": N.RASS_BONUS_ADD}

    def new_bonus(self, nq: Optional[int] = None):
        """A zero bonus column block for ``search_boosted``: float32 CUDA [stride] (``nq=None``: one column shared by every
        query) or [nq, stride]; stride = rows + slack, rounded up to 32.  Fill it with ``bonus_scatter``,
        ``bonus_from_attr_clauses`` and ``bonus_mask``.  It names rows of one ``layout_epoch``; rows appended later read 0."""
        import torch
        stride = (self.rows + self.BONUS_SLACK_ROWS + 31) // 32 * 32
        if nq is not None and not 1 <= int(nq) <= N.RASS_MAX_DEVICE_BATCH:
            raise ValueError(f"nq must be in [1, {N.RASS_MAX_DEVICE_BATCH}], got {nq}")
        return torch.zeros((stride,) if nq is None else (int(nq), stride), dtype=torch.float32, device=f"cuda:{self.engine.device}")

    @staticmethod
    def _bonus_shape(bonus) -> Tuple[int, int]:
        """(n_bonus, stride) of a device column block, checked."""
        import torch
        if not hasattr(bonus, "data_ptr") or not bonus.is_cuda or bonus.dtype != torch.float32 or not bonus.is_contiguous():
            raise ValueError("a bonus column block must be a contiguous float32 CUDA tensor")
        if bonus.dim() not in (1, 2) or int(bonus.shape[-1]) % 32 != 0:
            raise ValueError(f"bonus must be [stride] or [n, stride] with stride a multiple of 32, got {tuple(bonus.shape)}")
        return (1, int(bonus.shape[0])) if bonus.dim() == 1 else (int(bonus.shape[0]), int(bonus.shape[1]))

    def bonus_scatter(self, bonus, q_of, rows, values):
        """``bonus[q_of[i], rows[i]] += values[i]`` (``rass_index_bonus_scatter``): one rounded fp32 add per entry.  The
        (column, row) pairs must be unique within a call (sum duplicates first) and in range, or the call is refused.  For a
        shared column ``q_of`` is all zeros (or None).  Returns ``bonus``."""
        import torch
        n_bonus, stride = self._bonus_shape(bonus)
        r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
        v = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.float32)
        q = np.zeros(r.shape[0], dtype=np.int32) if q_of is None else np.ascontiguousarray(np.asarray(q_of).reshape(-1), dtype=np.int32)
        if not (q.shape == r.shape == v.shape):
            raise ValueError("q_of, rows and values must have one length")
        torch.cuda.current_stream(bonus.device).synchronize()     # the engine works on its own stream
        N.check("rass_index_bonus_scatter", self._L.rass_index_bonus_scatter(
            self._h, _np_ptr(q), _np_ptr(r), _np_ptr(v), r.shape[0], ctypes.c_void_p(bonus.data_ptr()), n_bonus, stride))
        return bonus

    def bonus_from_attr_clauses(self, bonus, clauses, weights, op: str = "replace"):
        """Weighted predicates over the attribute columns into ``bonus`` (``rass_index_bonus_from_attr_clauses``).
        ``clauses``: int32 [n, 5] rows ``(query, col, lo, hi, negate)`` as ``allow_from_attr_clauses`` takes them (a shared
        column's clauses name query 0); ``weights``: float32 [n].  Per (query, row): start from 0 (``op`` "replace") or the
        cell's value ("add"), then add the weight of every clause of the query that holds, in list order, one rounded fp32
        add each.  At most 64 clauses per query per call.  Returns ``bonus``."""
        import torch
        n_bonus, stride = self._bonus_shape(bonus)
        c = np.ascontiguousarray(np.asarray(clauses, dtype=np.int64).reshape(-1, 5))
        if c.size and (int(c.min()) < -(1 << 31) or int(c.max()) > (1 << 31) - 1):
            raise OverflowError("clause fields must fit int32")
        c = np.ascontiguousarray(c, dtype=np.int32)
        w = np.ascontiguousarray(np.asarray(weights).reshape(-1), dtype=np.float32)
        if w.shape[0] != c.shape[0]:
            raise ValueError(f"{c.shape[0]} clauses but {w.shape[0]} weights")
        if op not in self.BONUS_OPS:
            raise ValueError(f"op must be replace / add, not {op!r}")
        torch.cuda.current_stream(bonus.device).synchronize()     # the engine works on its own stream
        N.check("rass_index_bonus_from_attr_clauses", self._L.rass_index_bonus_from_attr_clauses(
            self._h, _np_ptr(c), _np_ptr(w), c.shape[0], n_bonus, n_bonus, ctypes.c_void_p(bonus.data_ptr()), stride,
            self.BONUS_OPS[op]))
        return bonus

    def bonus_mask(self, bonus, allow):
        """``bonus`` = -inf wherever the device bitmap ``allow`` ([words] shared, or one per column) has no bit
        (``rass_index_bonus_mask``): the rows a ``where`` filter excludes never rank in ``search_boosted``.  Returns ``bonus``."""
        import torch
        n_bonus, stride = self._bonus_shape(bonus)
        if not hasattr(allow, "data_ptr") or not allow.is_cuda or allow.dtype != torch.int32 or not allow.is_contiguous():
            raise ValueError("a device bitmap must be a contiguous int32 CUDA tensor")
        n_bitmaps, words = (1, int(allow.shape[0])) if allow.dim() == 1 else (int(allow.shape[0]), int(allow.shape[1]))
        if n_bitmaps not in (1, n_bonus):
            raise ValueError(f"{n_bitmaps} bitmaps for {n_bonus} bonus column(s)")
        torch.cuda.current_stream(bonus.device).synchronize()     # the engine works on its own stream
        N.check("rass_index_bonus_mask", self._L.rass_index_bonus_mask(
            self._h, ctypes.c_void_p(bonus.data_ptr()), n_bonus, stride, ctypes.c_void_p(allow.data_ptr()), n_bitmaps, words))
        return bonus

    def _check_boosted(self, nq: int, k: int, boost, transform, n_bonus: int, stride: int, bonus_rows,
                       what: str = "boosted") -> Tuple[Optional[np.ndarray], int, int]:
        """The argument checks of ``search_boosted``, made before any native call: (boost f32 [nq] or None, transform code,
        bonus_rows)."""
        if not 1 <= k <= N.RASS_MAX_K_MULTIPASS:
            raise ValueError(f"k must be in [1, {N.RASS_MAX_K_MULTIPASS}], got {k}")
        if nq > N.RASS_MAX_DEVICE_BATCH:
            raise ValueError(f"at most {N.RASS_MAX_DEVICE_BATCH} queries per call, got {nq}")
        if transform not in self.BOOST_TRANSFORMS:
            raise ValueError(f"transform must be raw / opensearch, not {transform!r}")
        if nq > 0 and n_bonus not in (1, nq):
            raise ValueError(f"bonus must be [stride] (shared) or [nq, stride], got {n_bonus} columns for {nq} queries")
        b = None
        if boost is not None:
            b = np.asarray(boost, dtype=np.float32)
            b = np.ascontiguousarray(np.full(nq, b, dtype=np.float32) if b.ndim == 0 else b)
            if b.shape != (nq,):
                raise ValueError("boost must be one number, or one per query")
            if not np.isfinite(b).all():
                raise ValueError("boost must be finite")
        rows = stride if bonus_rows is None else int(bonus_rows)
        if not 0 <= rows <= stride:
            raise ValueError(f"bonus_rows must be in [0, {stride}], got {rows}")
        if self.dtype != "f32" or self.row_stride > 1024:
            raise ValueError(f"{what} search needs an fp32 index with dim <= 1024")
        return b, self.BOOST_TRANSFORMS[transform], rows

    def search_boosted(self, queries: np.ndarray, k: int, bonus, boost=None, transform: str = "raw", bonus_rows: Optional[int] = None,
                       q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None,
                       on_device: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Exact top-k of ``boost[q] * T(cos) + bonus[q][row]`` (``rass_index_search_boosted``).  ``bonus``: a device column
        block from ``new_bonus`` ([stride] shared, [nq, stride] one per query), or a numpy array of that shape, uploaded.
        ``boost``: one finite number or one per query (None: 1.0); ``transform`` "raw" (T(s) = s) or "opensearch" (T(s) =
        1 / (2 - s)).  Rows at or past ``bonus_rows`` (default: the whole column) read 0.  A row ranks when it is live, passes
        ``q_filter`` / ``q_filter_mask`` as in ``search``, has a cosine above -inf and a fused score above -inf: a bonus of
        -inf or NaN excludes the row.  Returns (fused scores f32 [nq, k], ids i64 [nq, k]): best first, ties by id ascending,
        (-inf, -1) padding; k <= 4096, nq <= 4096.  One corpus pass per 32 queries.  fp32 indices with dim <= 1024.
        ``on_device``: go through the device-resident entry point.  Thread-safe."""
        q = self._queries(queries)
        nq, k = q.shape[0], int(k)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        host = None
        if isinstance(bonus, np.ndarray):
            host = np.ascontiguousarray(bonus, dtype=np.float32)
            if host.ndim not in (1, 2) or host.shape[-1] % 32 != 0:
                raise ValueError(f"bonus must be [stride] or [n, stride] with stride a multiple of 32, got {host.shape}")
            n_bonus, stride = (1, host.shape[0]) if host.ndim == 1 else host.shape
        else:
            n_bonus, stride = self._bonus_shape(bonus)
        b, t_code, rows = self._check_boosted(nq, k, boost, transform, n_bonus, stride, bonus_rows)
        out_s = np.empty((nq, k), dtype=np.float32)
        out_i = np.empty((nq, k), dtype=np.int64)
        if nq == 0:
            return out_s, out_i
        import torch
        dev = f"cuda:{self.engine.device}"
        if host is not None:
            bonus = torch.from_numpy(host).to(dev)
        torch.cuda.current_stream(bonus.device).synchronize()     # the engine works on its own stream
        if on_device:
            dq = torch.from_numpy(q).to(dev)
            db = torch.from_numpy(b).to(dev) if b is not None else None
            df = torch.from_numpy(f).to(dev) if f is not None else None
            dm = torch.from_numpy(m).to(dev) if m is not None else None
            ds = torch.empty((nq, k), dtype=torch.float32, device=dev)
            di = torch.empty((nq, k), dtype=torch.int64, device=dev)
            torch.cuda.current_stream(bonus.device).synchronize()
            self.search_boosted_device(dq.data_ptr(), nq, k, bonus.data_ptr(), n_bonus, rows, stride, ds.data_ptr(), di.data_ptr(),
                                       d_boost_ptr=db.data_ptr() if db is not None else 0, transform=transform,
                                       d_q_filter_ptr=df.data_ptr() if df is not None else 0,
                                       d_q_filter_mask_ptr=dm.data_ptr() if dm is not None else 0)
            self.engine.synchronize()
            return ds.cpu().numpy(), di.cpu().numpy()
        N.check("rass_index_search_boosted", self._L.rass_index_search_boosted(
            self._h, _np_ptr(q), nq, k, _np_ptr(b), t_code, ctypes.c_void_p(bonus.data_ptr()), n_bonus, rows, stride, _np_ptr(f),
            _np_ptr(m), _np_ptr(out_s), _np_ptr(out_i)))
        return out_s, out_i

    def search_boosted_device(self, d_queries_ptr: int, nq: int, k: int, d_bonus_ptr: int, n_bonus: int, bonus_rows: int,
                              bonus_stride: int, d_out_scores_ptr: int, d_out_ids_ptr: int, d_boost_ptr: int = 0,
                              transform: str = "raw", id_base: int = 0, d_q_filter_ptr: int = 0, d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_boosted`` (``rass_index_search_boosted_device``): nq <= 4096 in launch groups of
        32, k <= 4096 (every pass enqueued by the one call).  The boosts are device memory: keeping them finite is the caller's."""
        if transform not in self.BOOST_TRANSFORMS:
            raise ValueError(f"transform must be raw / opensearch, not {transform!r}")
        N.check("rass_index_search_boosted_device",
                self._L.rass_index_search_boosted_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), int(k),
                                                         ctypes.c_void_p(d_boost_ptr or 0), self.BOOST_TRANSFORMS[transform],
                                                         ctypes.c_void_p(d_bonus_ptr), int(n_bonus), int(bonus_rows), int(bonus_stride),
                                                         ctypes.c_void_p(d_q_filter_ptr or 0),
                                                         ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                         ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr)))

    # ---- function-score search: exact top-k of combine(boost * T(cos), a function column), gated by the similarity
    COMBINE_MODES = {"sum": N.RASS_COMBINE_SUM, "multiply": N.RASS_COMBINE_MULTIPLY, "avg": N.RASS_COMBINE_AVG,
                     "max": N.RASS_COMBINE_MAX, "min": N.RASS_COMBINE_MIN, "replace": N.RASS_COMBINE_REPLACE}
    FN_KINDS = {"gauss": N.RASS_FN_GAUSS, "exp": N.RASS_FN_EXP, "linear": N.RASS_FN_LINEAR,
                "field_value_factor": N.RASS_FN_FIELD_VALUE, "weight": N.RASS_FN_WEIGHT}
    FN_MODIFIERS = {"none": N.RASS_FN_MOD_NONE, "log": N.RASS_FN_MOD_LOG, "log1p": N.RASS_FN_MOD_LOG1P, "log2p": N.RASS_FN_MOD_LOG2P,
                    "ln": N.RASS_FN_MOD_LN, "ln1p": N.RASS_FN_MOD_LN1P, "ln2p": N.RASS_FN_MOD_LN2P, "square": N.RASS_FN_MOD_SQUARE,
                    "sqrt": N.RASS_FN_MOD_SQRT, "reciprocal": N.RASS_FN_MOD_RECIPROCAL}
    FN_SCORE_MODES = {"multiply": N.RASS_FN_SCORE_MULTIPLY, "sum": N.RASS_FN_SCORE_SUM, "avg": N.RASS_FN_SCORE_AVG,
                      "first": N.RASS_FN_SCORE_FIRST, "max": N.RASS_FN_SCORE_MAX, "min": N.RASS_FN_SCORE_MIN}
    MAX_SCORE_FNS = N.RASS_MAX_SCORE_FNS

    @classmethod
    def _fn_records(cls, functions):
        """``functions`` (dicts, see ``fn_from_attr``) as a ctypes array of ``rass_score_fn_t``."""
        functions = list(functions or [])
        recs = (N.ScoreFn * max(1, len(functions)))()
        for r, f in zip(recs, functions):
            if not isinstance(f, dict) or f.get("kind") not in cls.FN_KINDS:
                raise ValueError(f"a function is a dict whose kind is one of {sorted(cls.FN_KINDS)}, got {f!r}")
            unknown = set(f) - {"query", "kind", "col", "filter", "weight", "origin", "scale", "offset", "decay", "factor",
                                "modifier", "missing"}
            if unknown:
                raise ValueError(f"unknown function field(s) {sorted(unknown)}")
            mod = f.get("modifier") or "none"
            if mod not in cls.FN_MODIFIERS:
                raise ValueError(f"modifier must be one of {sorted(cls.FN_MODIFIERS)}, not {mod!r}")
            r.query, r.kind, r.col = int(f.get("query", 0)), cls.FN_KINDS[f["kind"]], int(f.get("col", 0))
            r.filter = -1 if f.get("filter") is None else int(f["filter"])
            r.modifier, r.reserved, r.weight = cls.FN_MODIFIERS[mod], 0, float(f.get("weight", 1.0))
            r.origin, r.scale, r.offset = float(f.get("origin", 0.0)), float(f.get("scale", 1.0)), float(f.get("offset", 0.0))
            r.decay, r.factor = float(f.get("decay", 0.5)), float(f.get("factor", 1.0))
            r.missing = float("nan") if f.get("missing") is None else float(f["missing"])
        return recs, len(functions)

    def fn_from_attr(self, column, functions, score_mode: str = "multiply", max_boost: Optional[float] = None, filters=None):
        """Fill the device column block ``column`` (from ``new_bonus``: [stride] shared, or [nq, stride]) from a list of
        functions over the attribute columns (``rass_index_fn_from_attr``): OpenSearch's ``function_score.functions``.
        A function is a dict: ``kind`` "gauss" / "exp" / "linear" (``col``, ``origin``, ``scale`` > 0, ``offset`` >= 0, 0 <
        ``decay`` < 1; a missing value gives 1.0), "field_value_factor" (``col``, ``factor``, ``modifier`` none / log / log1p
        / log2p / ln / ln1p / ln2p / square / sqrt / reciprocal, ``missing``: the stand-in for a missing value, None = the
        function skips the row) or "weight" (the constant 1.0); ``query`` (the column it belongs to, default 0), ``weight``
        (default 1.0), ``filter`` (None, or an index into ``filters``).  ``filters``: int32 CUDA [n, words] (or [words], or a
        list of [words] tensors) row bitmaps as ``allow_from_attr_clauses`` / ``run_plan`` build them.  A query's applying functions are folded in list
        order by ``score_mode`` (multiply / sum / avg / first / max / min), capped at ``max_boost``; a row no function applies
        to gets 1.0.  At most 16 functions per query per call.  Double arithmetic on the device, rounded to fp32 once.  A
        non-positive argument of a log modifier gives -inf / NaN, which ``search_scored`` treats as "row excluded".
        Returns ``column``."""
        import torch
        n_fn, stride = self._bonus_shape(column)
        if score_mode not in self.FN_SCORE_MODES:
            raise ValueError(f"score_mode must be one of {sorted(self.FN_SCORE_MODES)}, not {score_mode!r}")
        recs, n = self._fn_records(functions)
        cap = float("inf") if max_boost is None else float(max_boost)
        n_filters, words, fptr = 0, 0, None
        if isinstance(filters, (list, tuple)):      # one bitmap per entry, each [words]
            filters = torch.stack(list(filters)).contiguous() if filters else None
        if filters is not None:
            if not hasattr(filters, "data_ptr") or not filters.is_cuda or filters.dtype != torch.int32 or not filters.is_contiguous():
                raise ValueError("filters must be a contiguous int32 CUDA tensor [n, words] (or [words])")
            n_filters, words = (1, int(filters.shape[0])) if filters.dim() == 1 else (int(filters.shape[0]), int(filters.shape[1]))
            fptr = ctypes.c_void_p(filters.data_ptr())
        torch.cuda.current_stream(column.device).synchronize()     # the engine works on its own stream
        N.check("rass_index_fn_from_attr", self._L.rass_index_fn_from_attr(
            self._h, ctypes.cast(recs, ctypes.c_void_p), n, n_fn, self.FN_SCORE_MODES[score_mode], cap, fptr, n_filters, words,
            ctypes.c_void_p(column.data_ptr()), stride))
        return column

    def search_scored(self, queries: np.ndarray, k: int, column, boost=None, transform: str = "raw", combine: str = "multiply",
                      min_score=None, q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None,
                      on_device: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """Exact top-k of ``combine(boost[q] * T(cos), column[q][row])`` (``rass_index_search_scored``): OpenSearch's
        ``function_score`` around a k-NN clause.  ``column``: a device block ([stride] shared, [nq, stride] one per query)
        from ``new_bonus`` filled by ``fn_from_attr`` (and ``bonus_mask``), or a numpy array of that shape, uploaded; it must
        hold a value for every row of the index.  ``combine``: sum / multiply / avg / max / min / replace (``boost_mode``).
        ``min_score``: one number or one per query, a gate on T(cos) (None / -inf: no gate).  ``boost`` / ``transform`` /
        filters as in ``search_boosted``.  A row ranks when it is live, passes the filters and the gate, and its cosine, its
        column value and its fused score are all above -inf: a NaN or -inf cell excludes the row in every mode.  Returns
        (fused f32 [nq, k], ids i64 [nq, k]): best first, ties by id ascending, (-inf, -1) padding.  fp32 indices with dim <=
        1024.  ``on_device``: go through the device-resident entry point.  Thread-safe."""
        q = self._queries(queries)
        nq, k = q.shape[0], int(k)
        f, m = self._filters(q_filter, q_filter_mask, nq)
        host = None
        if isinstance(column, np.ndarray):
            host = np.ascontiguousarray(column, dtype=np.float32)
            if host.ndim not in (1, 2) or host.shape[-1] % 32 != 0:
                raise ValueError(f"column must be [stride] or [n, stride] with stride a multiple of 32, got {host.shape}")
            n_fn, stride = (1, host.shape[0]) if host.ndim == 1 else host.shape
        else:
            n_fn, stride = self._bonus_shape(column)
        if combine not in self.COMBINE_MODES:
            raise ValueError(f"combine must be one of {sorted(self.COMBINE_MODES)}, not {combine!r}")
        rows = self.rows
        if stride < rows:
            raise ValueError(f"the column holds {stride} cells, the index {rows} rows")
        b, t_code, _ = self._check_boosted(nq, k, boost, transform, n_fn, stride, rows, what="function-score")
        gate = None if min_score is None else self._thresholds(min_score, nq)
        out_s = np.empty((nq, k), dtype=np.float32)
        out_i = np.empty((nq, k), dtype=np.int64)
        if nq == 0:
            return out_s, out_i
        import torch
        dev = f"cuda:{self.engine.device}"
        if host is not None:
            column = torch.from_numpy(host).to(dev)
        torch.cuda.current_stream(column.device).synchronize()     # the engine works on its own stream
        if on_device:
            dq = torch.from_numpy(q).to(dev)
            db = torch.from_numpy(b).to(dev) if b is not None else None
            dg = torch.from_numpy(gate).to(dev) if gate is not None else None
            df = torch.from_numpy(f).to(dev) if f is not None else None
            dm = torch.from_numpy(m).to(dev) if m is not None else None
            ds = torch.empty((nq, k), dtype=torch.float32, device=dev)
            di = torch.empty((nq, k), dtype=torch.int64, device=dev)
            torch.cuda.current_stream(column.device).synchronize()
            self.search_scored_device(dq.data_ptr(), nq, k, column.data_ptr(), n_fn, rows, stride, ds.data_ptr(), di.data_ptr(),
                                      d_boost_ptr=db.data_ptr() if db is not None else 0, transform=transform, combine=combine,
                                      d_min_score_ptr=dg.data_ptr() if dg is not None else 0,
                                      d_q_filter_ptr=df.data_ptr() if df is not None else 0,
                                      d_q_filter_mask_ptr=dm.data_ptr() if dm is not None else 0)
            self.engine.synchronize()
            return ds.cpu().numpy(), di.cpu().numpy()
        N.check("rass_index_search_scored", self._L.rass_index_search_scored(
            self._h, _np_ptr(q), nq, k, _np_ptr(b), t_code, self.COMBINE_MODES[combine], _np_ptr(gate),
            ctypes.c_void_p(column.data_ptr()), n_fn, rows, stride, _np_ptr(f), _np_ptr(m), _np_ptr(out_s), _np_ptr(out_i)))
        return out_s, out_i

    def search_scored_device(self, d_queries_ptr: int, nq: int, k: int, d_fn_ptr: int, n_fn: int, fn_rows: int, fn_stride: int,
                             d_out_scores_ptr: int, d_out_ids_ptr: int, d_boost_ptr: int = 0, transform: str = "raw",
                             combine: str = "multiply", d_min_score_ptr: int = 0, id_base: int = 0, d_q_filter_ptr: int = 0,
                             d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_scored`` (``rass_index_search_scored_device``): nq <= 4096 in launch groups of 32,
        k <= 4096 (every pass enqueued by the one call).  Boosts and gates are device memory: their values are the caller's."""
        if transform not in self.BOOST_TRANSFORMS:
            raise ValueError(f"transform must be raw / opensearch, not {transform!r}")
        if combine not in self.COMBINE_MODES:
            raise ValueError(f"combine must be one of {sorted(self.COMBINE_MODES)}, not {combine!r}")
        N.check("rass_index_search_scored_device",
                self._L.rass_index_search_scored_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), int(k),
                                                        ctypes.c_void_p(d_boost_ptr or 0), self.BOOST_TRANSFORMS[transform],
                                                        self.COMBINE_MODES[combine], ctypes.c_void_p(d_min_score_ptr or 0),
                                                        ctypes.c_void_p(d_fn_ptr), int(n_fn), int(fn_rows), int(fn_stride),
                                                        ctypes.c_void_p(d_q_filter_ptr or 0),
                                                        ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                        ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr)))

    MAX_MMR_FETCH = N.RASS_MAX_MMR_FETCH   # search_mmr: candidates per query; rows_gram: rows per list

    def rows_gram(self, rows) -> np.ndarray:
        """Gram matrices of short row lists, ``rass_index_rows_gram``: ``rows`` is int64 [n_lists, L] (or [L]: one list) row
        ordinals, 1 <= L <= 128.  Returns float32 [n_lists, L, L]: the fp32 dot products of the stored (normalised) rows,
        bitwise symmetric.  An ordinal < 0 or >= ``rows``, or a tombstoned row, is padding: zeros in its row and column.
        fp32 indices only."""
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if r.ndim == 1:
            r = r[None, :]
        if r.ndim != 2 or not 1 <= r.shape[1] <= self.MAX_MMR_FETCH:
            raise ValueError(f"expected [n_lists, 1..{self.MAX_MMR_FETCH}] row ordinals, got {r.shape}")
        out = np.empty((r.shape[0], r.shape[1], r.shape[1]), dtype=np.float32)
        if r.shape[0] == 0:
            return out
        N.check("rass_index_rows_gram", self._L.rass_index_rows_gram(self._h, _np_ptr(r), r.shape[0], r.shape[1], _np_ptr(out)))
        return out

    def rows_gram_device(self, d_rows_ptr: int, n_lists: int, list_len: int, d_out_ptr: int) -> None:
        """Async, device-resident ``rows_gram`` (``rass_index_rows_gram_device``): int64 [n_lists][list_len] ordinals in,
        float32 [n_lists][list_len][list_len] out, stream-ordered, nothing read back."""
        N.check("rass_index_rows_gram_device",
                self._L.rass_index_rows_gram_device(self._h, ctypes.c_void_p(d_rows_ptr), int(n_lists), int(list_len),
                                                    ctypes.c_void_p(d_out_ptr)))

    @classmethod
    def _check_mmr(cls, k, fetch_k) -> Tuple[int, int]:
        k = int(k)
        fetch_k = min(cls.MAX_MMR_FETCH, max(4 * k, 16)) if fetch_k is None else int(fetch_k)
        if not 1 <= fetch_k <= cls.MAX_MMR_FETCH:
            raise ValueError(f"fetch_k must be in [1, {cls.MAX_MMR_FETCH}], got {fetch_k}")
        if not 1 <= k <= fetch_k:
            raise ValueError(f"k must be in [1, fetch_k = {fetch_k}], got {k}")
        return k, fetch_k

    def search_mmr(self, queries: np.ndarray, k: int, fetch_k: Optional[int] = None, lambda_mult=0.5,
                   q_filter: Optional[np.ndarray] = None, q_filter_mask: Optional[np.ndarray] = None
                   ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Diversified (MMR) search, ``rass_index_search_mmr``: a greedy maximal-marginal-relevance re-rank of the exact
        top ``fetch_k`` (default ``min(128, max(4 k, 16))``; 1 <= k <= fetch_k <= 128).  At every step the candidate with
        the largest ``lambda * cos(query, row) - (1 - lambda) * max(cos(row, picked))`` is picked, ties to the better
        rank; ``lambda_mult`` is one number in [0, 1] or one per query (1: plain top-k; 0: the best hit, then the least
        similar).  Returns (scores f32 [nq, k], ids i64 [nq, k], ranks i32 [nq, k]) in selection order: the raw cosine to
        the query, the row id, and the row's rank in the plain top ``fetch_k``; (-inf, -1, -1) padding.  Filters as
        ``search``.  Always the exact fp32 scan (the prefilter mode is ignored); fp32 indices only.  Thread-safe."""
        q = self._queries(queries)
        nq = q.shape[0]
        k, fetch_k = self._check_mmr(k, fetch_k)
        lam = np.asarray(lambda_mult)
        if lam.dtype.kind not in "fiu":
            raise ValueError(f"lambda_mult must be real numbers, not {lam.dtype}")
        if lam.ndim == 0:
            lam = np.full(nq, lam)
        lam = np.ascontiguousarray(lam, dtype=np.float32)
        if lam.shape != (nq,):
            raise ValueError("lambda_mult must be one number, or one per query")
        if not np.all((lam >= 0.0) & (lam <= 1.0)):     # False for NaN
            raise ValueError("lambda_mult must be in [0, 1]")
        f, m = self._filters(q_filter, q_filter_mask, nq)
        out_s = np.empty((nq, k), dtype=np.float32)
        out_i = np.empty((nq, k), dtype=np.int64)
        out_r = np.empty((nq, k), dtype=np.int32)
        if nq == 0:
            return out_s, out_i, out_r
        N.check("rass_index_search_mmr",
                self._L.rass_index_search_mmr(self._h, _np_ptr(q), nq, k, fetch_k, _np_ptr(lam), _np_ptr(f), _np_ptr(m),
                                              _np_ptr(out_s), _np_ptr(out_i), _np_ptr(out_r)))
        return out_s, out_i, out_r

    def search_mmr_device(self, d_queries_ptr: int, nq: int, k: int, fetch_k: int, d_lambda_ptr: int, d_out_scores_ptr: int,
                          d_out_ids_ptr: int, d_out_rank_ptr: int = 0, id_base: int = 0, d_q_filter_ptr: int = 0,
                          d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident ``search_mmr`` (``rass_index_search_mmr_device``); nq <= 32, every candidate pass enqueued
        by the one call.  A query whose lambda is NaN or outside [0, 1] gets the empty list."""
        k, fetch_k = self._check_mmr(k, fetch_k)
        N.check("rass_index_search_mmr_device",
                self._L.rass_index_search_mmr_device(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), k, fetch_k,
                                                     ctypes.c_void_p(d_lambda_ptr), ctypes.c_void_p(d_q_filter_ptr or 0),
                                                     ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                     ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr),
                                                     ctypes.c_void_p(d_out_rank_ptr or 0)))

    def search_device(self, d_queries_ptr: int, nq: int, k: int, d_out_scores_ptr: int, d_out_ids_ptr: int,
                      id_base: int = 0, d_q_filter_ptr: int = 0, d_q_filter_mask_ptr: int = 0) -> None:
        """Async, device-resident variant (multi-GPU path, benchmark); nq <= 32."""
        N.check("rass_index_search_device_ex",
                self._L.rass_index_search_device_ex(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), int(k),
                                                    ctypes.c_void_p(d_q_filter_ptr or 0),
                                                    ctypes.c_void_p(d_q_filter_mask_ptr or 0), int(id_base),
                                                    ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr)))

    def search_device_after(self, d_queries_ptr: int, nq: int, k: int, d_after_score_ptr: int, d_after_row_ptr: int,
                            d_out_scores_ptr: int, d_out_ids_ptr: int, d_q_filter_ptr: int = 0,
                            d_q_filter_mask_ptr: int = 0) -> None:
        """One continuation pass (``rass_index_search_device_after``): only rows strictly after (after_score[q],
        after_row[q]) in (score desc, row asc) rank for query q.  Async, device-resident, nq <= 32, k <= 32."""
        N.check("rass_index_search_device_after",
                self._L.rass_index_search_device_after(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), int(k),
                                                       ctypes.c_void_p(d_q_filter_ptr or 0),
                                                       ctypes.c_void_p(d_q_filter_mask_ptr or 0),
                                                       ctypes.c_void_p(d_after_score_ptr), ctypes.c_void_p(d_after_row_ptr),
                                                       ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr)))

    def search_device_batch(self, d_queries_ptr: int, nq: int, k: int, d_out_scores_ptr: int, d_out_ids_ptr: int,
                            id_base: int = 0, d_q_filter_ptr: int = 0, out_scores_group_stride: int = 0,
                            out_ids_group_stride: int = 0) -> None:
        """Async, device-resident, MANY launch groups per call (nq <= 4096, k <= 32): bit-identical to
        ``search_device`` on consecutive groups of 32 queries, with one normalise and one merge launch for the whole
        batch.  Group g's results go to out + g * group_stride (elements; 0 = contiguous [nq][k])."""
        N.check("rass_index_search_device_batch",
                self._L.rass_index_search_device_batch(self._h, ctypes.c_void_p(d_queries_ptr), int(nq), int(k),
                                                       ctypes.c_void_p(d_q_filter_ptr or 0), int(id_base),
                                                       ctypes.c_void_p(d_out_scores_ptr), ctypes.c_void_p(d_out_ids_ptr),
                                                       int(out_scores_group_stride), int(out_ids_group_stride)))


class HipTimer:
    """hipEvent pair on an explicit stream (rass_timer_*)."""

    def __init__(self):
        self._L = N.lib()
        h = ctypes.c_void_p()
        N.check("rass_timer_create", self._L.rass_timer_create(ctypes.byref(h)))
        self._h = h

    def start(self, stream_ptr: int = 0) -> None:
        N.check("rass_timer_start", self._L.rass_timer_start(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def stop(self, stream_ptr: int = 0) -> None:
        N.check("rass_timer_stop", self._L.rass_timer_stop(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def elapsed_ms(self) -> float:
        ms = ctypes.c_float(0)
        N.check("rass_timer_elapsed_ms", self._L.rass_timer_elapsed_ms(self._h, ctypes.byref(ms)))
        return float(ms.value)

    def __del__(self):  # pragma: no cover
        try:
            if self._h:
                self._L.rass_timer_destroy(self._h)
                self._h = None
        except Exception:
            pass


def scan_kernel_name(dim: int, nq: int) -> str:
    return N.lib().rass_scan_kernel_name(int(dim), int(nq)).decode()
