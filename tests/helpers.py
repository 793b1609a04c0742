"""Test doubles: a CPU stand-in for FlatIndex (oracle-backed) so the host-side shim logic
can be exercised without a GPU.  Lives under tests/ — never imported by the product."""
import zlib

import numpy as np

from oracle import oracle as O


class OracleIndex:
    """Same surface as rassengine_amd.engine.FlatIndex; arithmetic = the CPU oracle."""

    def __init__(self, dim=1024):
        self.dim = dim
        self._rows = np.zeros((0, dim), dtype=np.float32)
        self._tags = np.zeros((0,), dtype=np.int32)

    @property
    def rows(self):
        return self._rows.shape[0]

    @property
    def count(self):
        return int((self._tags != -1).sum())

    def add(self, vecs, tags=None, normalize=True):
        v = np.ascontiguousarray(vecs, dtype=np.float32)
        first = self.rows
        if normalize:
            v = O.normalize_ref(v).astype(np.float32)
        t = np.zeros(v.shape[0], dtype=np.int32) if tags is None else np.asarray(tags, dtype=np.int32)
        self._rows = np.concatenate([self._rows, v])
        self._tags = np.concatenate([self._tags, t])
        return first

    def delete(self, row):
        if not 0 <= row < self.rows:
            raise IndexError(row)
        self._tags[row] = -1

    def get_row(self, row):
        return self._rows[row].copy()

    def get_rows(self, first_row, n):
        return self._rows[first_row:first_row + n].copy()

    def search(self, queries, k, q_filter=None, q_filter_mask=None):
        qn = O.normalize_ref(np.ascontiguousarray(queries, dtype=np.float32)).astype(np.float32)
        s, i = O.search(self._rows, qn, k, tags=self._tags, qfilter=q_filter, qmask=q_filter_mask)
        return s.astype(np.float32), i


class HashEmbedder:
    """Deterministic text -> vector stand-in for the encoder (host-logic tests only)."""

    def __init__(self, dim=1024):
        self.dim = dim
        self.calls = []

    def encode(self, texts):
        self.calls.append(list(texts))
        out = np.zeros((len(texts), self.dim), dtype=np.float32)
        for r, t in enumerate(texts):
            for w in t.lower().split():
                rng = np.random.default_rng(zlib.crc32(w.encode("utf-8")))   # not hash(): that is salted per process
                out[r] += rng.standard_normal(self.dim).astype(np.float32)
        return out * 3.0  # deliberately un-normalised


class TokenHashEncoder:
    """Process-independent stand-in for the sentence encoder with the surface serving.py's data-parallel ingest
    uses: ``tokenize(texts) -> (ids, cu)`` on rank 0, ``encode_flat(ids, cu) -> [n, dim]`` on every rank, and
    ``encode(texts)`` for the single-index path.  A token id is crc32(word) (no PYTHONHASHSEED dependence: the ranks
    are different processes), a sequence's vector the sum of its tokens' seeded Gaussian vectors."""

    def __init__(self, dim=1024):
        self.dim = dim
        self.encoded_seqs = 0

    def tokenize(self, texts):
        import zlib
        seqs = [[zlib.crc32(w.encode("utf-8")) % 30000 + 1 for w in t.lower().split()] for t in texts]
        cu = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum([len(q) for q in seqs], out=cu[1:])
        ids = np.concatenate([np.asarray(q, dtype=np.int32) for q in seqs]) if cu[-1] else np.zeros(0, np.int32)
        return ids, cu

    def encode_flat(self, ids, cu):
        n = len(cu) - 1
        out = np.zeros((n, self.dim), dtype=np.float32)
        for r in range(n):
            for tok in np.asarray(ids[int(cu[r]):int(cu[r + 1])]):
                out[r] += np.random.default_rng(int(tok)).standard_normal(self.dim).astype(np.float32)
        self.encoded_seqs += n
        return out * 3.0  # deliberately un-normalised

    def encode(self, texts):
        ids, cu = self.tokenize(texts)
        return self.encode_flat(ids, cu)


# ------------------------------------------------------------------------------------------ the encoder GEMM routing mirror
# An independent statement, in Python, of which kernel gemm_route.cpp gives a shape: what the GPU tests
# predict their branch from and what tests/test_gemm_route_cpu.py holds rass_gemm_bf16_route to.  `sw` overrides the
# defaults of the RASS_GEMM_* switches that move a route.
GEMM_SWITCH_DEFAULTS = dict(fewrows=True, fewrows_max=96, fewrows_res=64, mid=None, variant=None, splitk_s=None, mid_bm=None,
                            lnin_waves=16)


def _gemm_sw(sw):
    out = dict(GEMM_SWITCH_DEFAULTS)
    out.update(sw or {})
    return out


def _splitk_slices(m_pad, n, k, ws_bytes):
    tiles, steps = (n // 128) * (m_pad // 128), k // 64
    if steps < 2:
        return 0
    s = 1
    if k < 2048:
        while s < 4 and tiles * s < 128 and steps % (2 * s) == 0:
            s *= 2
    else:
        cap = 16 if tiles <= 8 else (8 if tiles < 48 else 4)
        while s < cap and tiles * s * 2 <= 512 and steps % (2 * s) == 0:
            s *= 2
    while s > 1 and s * m_pad * n * 4 > ws_bytes:
        s //= 2
    return s if s > 1 else 0


def _slices(sw, m_pad, n, k, ws_bytes):
    s = sw["splitk_s"]
    if s is None:
        return _splitk_slices(m_pad, n, k, ws_bytes)
    return s if 2 <= s <= 16 and (k // 64) % s == 0 and s * m_pad * n * 4 <= ws_bytes else 0   # RASS_GEMM_SPLITK_S: that split or none


def _fewrows_waves(M, N, K, max_rows=96):
    if M < 1 or N % 16 or N < 1024:
        return 0
    if K % 1024 == 0 and K <= 3072:
        return 4 if M <= max_rows else 0
    if M > 64:
        return 0
    return 16 if (K % 4096 == 0 and K <= 8192) else 0


def _mid_rows(sw, m):
    return sw["mid"] == 2 or (sw["mid"] is None and 96 < m <= 1024)


def _residual_branch(m, m_pad, n, k, ws_bytes, forced_s=None, sw=None):
    """the branch launch_gemm_bf16_residual_layernorm takes: mirrors its conditions"""
    sw = _gemm_sw(sw)
    if not ws_bytes:
        return "pair"
    if sw["fewrows"] and m_pad >= 64 and m <= sw["fewrows_res"] and \
            _fewrows_waves(m, n, k // 4 if k % 4096 == 0 else k, sw["fewrows_max"]):
        rows_pad = 64 if m <= 64 else 128
        if k % 4096 == 0 and k // 4 <= 3072 and n % 8 == 0 and n <= 2048 and 4 * rows_pad * n * 4 <= ws_bytes:
            return "fewrows4+ln" + ("_exact" if n == 1024 else "")
        return "fewrows+pair"
    mid = _mid_rows(sw, m)
    if m_pad % 128 == 0 and n % 128 == 0 and k % 64 == 0 and n <= 2048 and not (mid and 256 <= k <= 1024):
        mp = (m + 127) // 128 * 128
        s = forced_s if forced_s else _slices(sw, mp, n, k, ws_bytes)
        if s:
            return "splitk%d+ln" % s + ("_exact" if n == 1024 and s in (2, 4, 8) else "")
    return "pair"


def _persistent_kernel(sw, m_pad, n, k, epi):
    fits = m_pad * k * 2 < 2 ** 32 - 2 ** 24 and n * k * 2 < 2 ** 32 - 2 ** 24   # p4's 32-bit buffer descriptors
    p4 = sw["variant"] == "p4" or (sw["variant"] is None and epi != 5)          # the folded GELU epilogue stays on p5
    return "p4" if p4 and k >= 512 and fits else "p5"


def _persistent_shape(m, m_pad, n, k, any_tile_count=False):
    return n % 256 == 0 and m_pad % 256 == 0 and k % 64 == 0 and k >= 128 and m >= 1024 and \
        (any_tile_count or (n // 256) * (m_pad // 256) >= 192)


def _gemm_branch(m, m_pad, n, k, epi, ws_bytes, sw=None):
    """the kernel launch_gemm_bf16 (epilogue 0 / 1 / 2) gives a shape"""
    sw = _gemm_sw(sw)
    if m < 1 or m_pad < m or m_pad % 128 or n % 128 or k % 64:
        return "unsupported"
    if ws_bytes and m_pad >= 64 and sw["fewrows"]:
        w = _fewrows_waves(m, n, k, sw["fewrows_max"])
        if w:
            return "fewrows%d" % w
    mid = _mid_rows(sw, m)
    if ws_bytes and not (mid and 256 <= k <= 1024):
        s = _slices(sw, (m + 127) // 128 * 128, n, k, ws_bytes)
        if s:
            return "splitk%d" % s
    if _persistent_shape(m, m_pad, n, k, any_tile_count=sw["variant"] is not None):
        return _persistent_kernel(sw, m_pad, n, k, epi)
    if mid and k >= 256 and m_pad * k * 2 < 2 ** 32 - 2 ** 24 and n * k * 2 < 2 ** 32 - 2 ** 24:
        bm = sw["mid_bm"] or (64 if (n // 128) * ((m + 63) // 64) <= 256 else 128)
        return "mid%d" % bm
    return "tile128"


def _fold_branch(m, m_pad, n, k, epi, sw=None):
    """launch_gemm_bf16_fold (epilogue 3 / 4 / 5): the persistent kernels, from 192 tiles of 256 x 256 on"""
    return _persistent_kernel(_gemm_sw(sw), m_pad, n, k, epi) if _persistent_shape(m, m_pad, n, k) else "unsupported"


def _ln_input_branch(m, n, k, sw=None):
    sw = _gemm_sw(sw)
    return "lnin%d" % sw["lnin_waves"] if 1 <= m <= 32 and k == 1024 and n % 16 == 0 and n >= 1024 and sw["fewrows"] else "unsupported"
