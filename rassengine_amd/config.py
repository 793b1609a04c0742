"""Configuration: the same environment names the reference reads at import
(app/main.py:60-108, app/embedding_gen.py:39-70), plus ``RASS_*`` for the engine."""
import os


def _int(name: str, default: int) -> int:
    try:
        return int(os.getenv(name, default))
    except (TypeError, ValueError):
        return default


EMBED_MODEL_NAME = os.getenv("OLLAMA_EMBED_MODEL", "mxbai-embed-large:latest")  # app/main.py:67
BATCH_SIZE = _int("BATCH_SIZE", 64)            # app/main.py:78
CHUNK_SIZE = _int("CHUNK_SIZE", 512)           # app/main.py:79
EMBED_DIM = _int("EMBED_DIM", 1024)            # app/main.py:80
OPENSEARCH_INDEX_NAME = os.getenv("OPENSEARCH_INDEX_NAME", "")  # app/main.py:87
TOP_K = _int("TOP_K", 3)                       # app/main.py:88
SHARD_COUNT = _int("SHARD_COUNT", 1)           # app/main.py:89 (here: informational; shards = GPUs)

RASS_DEVICE = _int("RASS_DEVICE", _int("LOCAL_RANK", 0))   # the GPU this process drives
RASS_MODEL_DIR = os.getenv("RASS_MODEL_DIR", "")           # local dir with encoder weights + vocab.txt
RASS_SCORE_MODE = os.getenv("RASS_SCORE_MODE", "opensearch")  # "opensearch": 1/(2-cos); "cosine": raw
RASS_RETURN_EMBEDDING = os.getenv("RASS_RETURN_EMBEDDING", "0") == "1"
RASS_POOLING = os.getenv("RASS_POOLING", "")               # "cls" | "mean" | "" (from the model dir)
# embed micro-batcher (batcher.EmbedBatcher): sequences per coalesced forward (0 = off: one encoder call per request),
# the longest a request waits for company from idle, and the quiet gap that ends the wait early
RASS_EMBED_BATCH_MAX = _int("RASS_EMBED_BATCH_MAX", 64)
try:
    RASS_EMBED_BATCH_DELAY_MS = float(os.getenv("RASS_EMBED_BATCH_DELAY_MS", "0.2"))
    RASS_EMBED_BATCH_QUIET_US = float(os.getenv("RASS_EMBED_BATCH_QUIET_US", "50"))
except ValueError:
    RASS_EMBED_BATCH_DELAY_MS, RASS_EMBED_BATCH_QUIET_US = 0.2, 50.0
# k-NN prefetch at ask()'s `await ensure_index_exists` (prefetch.py): 0 = off, 1 = when other requests are in flight, 2 = always
RASS_KNN_PREFETCH = _int("RASS_KNN_PREFETCH", 1)
# IVF behind the boundary (ivf.IvfPolicy): 0 = every index stays flat (exact; the default).  > 0: an index of at least
# RASS_IVF_MIN_ROWS rows gets an IVF-<nlist> (probed with RASS_IVF_NPROBE lists per query) + a flat delta for the rows
# appended since; the IVF is rebuilt once the delta exceeds RASS_IVF_REBUILD_FRACTION of the rows it covers
RASS_IVF_NLIST = _int("RASS_IVF_NLIST", 0)
RASS_IVF_NPROBE = _int("RASS_IVF_NPROBE", 8)
RASS_IVF_MIN_ROWS = _int("RASS_IVF_MIN_ROWS", 262144)
RASS_IVF_DTYPE = os.getenv("RASS_IVF_DTYPE", "f32")            # the IVF's own copy of the rows: "f32" | "bf16" | "int8" (+ exact re-rank, k <= 16)
# Candidate scan of a flat index's searches with k <= 16: "off" (exact fp32 scan, the default), "bf16" (half the bytes per pass)
# or "int8" (a quarter: per-row-scaled int8 copy); the 32 candidates per query are re-scored exactly in fp32 either way
# (include/rass_engine.h: rass_index_set_prefilter).  The reference's own index is approximate (HNSW, app/main.py:563-572).
# "int8_exact": the int8 scan keeps 128 candidates, a per-query certificate proves the exact top-k among them and the fp32
# scan answers the queries it cannot prove: the flat scan's results bit for bit, for k <= 32.
RASS_PREFILTER = os.getenv("RASS_PREFILTER", "off").strip().lower() or "off"
if RASS_PREFILTER not in ("off", "bf16", "int8", "int8_exact"):
    raise ValueError(f"RASS_PREFILTER must be off, bf16, int8 or int8_exact, not {RASS_PREFILTER!r}")
try:
    RASS_IVF_REBUILD_FRACTION = float(os.getenv("RASS_IVF_REBUILD_FRACTION", "0.25"))
except ValueError:
    RASS_IVF_REBUILD_FRACTION = 0.25
# RASS_IVF_ABSORB_FRACTION: 0 = never (the default: the delta only leaves through a rebuild).  > 0: once the delta exceeds
# that fraction of the covered rows the IVF is extended over it on the GPU with the centroids it has (ivf.IvfBackedIndex.
# absorb_delta: no training, no host pass over the rows), and RASS_IVF_REBUILD_FRACTION then counts growth since the
# centroids were last TRAINED.  Out of place: needs HBM for the new IVF next to the old one.
try:
    RASS_IVF_ABSORB_FRACTION = float(os.getenv("RASS_IVF_ABSORB_FRACTION", "0"))
except ValueError:
    RASS_IVF_ABSORB_FRACTION = 0.0
# RASS_IVF_ALLOW: 1 = an index with an fp32 IVF answers its bitmap-filtered searches (search_allowed: `where=`, `within`) by
# probing the IVF within the bitmap where the byte rule of ivf.IvfPolicy.allow_route says that is cheaper than the exact
# allow scan; anything else (the default: 0) = every filtered search is the exact allow scan over the flat index, as before
RASS_IVF_ALLOW = os.getenv("RASS_IVF_ALLOW", "0").strip() == "1"
# Compaction of tombstoned rows (docstore.IndexState.compact, rass_index_compact): an `_id` overwrite appends the new row and
# tombstones the old one, whose 4 KiB every later scan still streams.  RASS_COMPACT_FRACTION: 0 = never (the default);
# > 0: add_documents compacts the index once its tombstones exceed that fraction of its rows and it holds at least
# RASS_COMPACT_MIN_ROWS rows.  Out of place: needs HBM for the compacted index next to the old one.
try:
    RASS_COMPACT_FRACTION = float(os.getenv("RASS_COMPACT_FRACTION", "0"))
except ValueError:
    RASS_COMPACT_FRACTION = 0.0
RASS_COMPACT_MIN_ROWS = _int("RASS_COMPACT_MIN_ROWS", 65536)
# Attribute columns (docstore.AttrSchema): up to 8 `field:kind` pairs, kind = keyword | int | date, e.g.
# "resourceType:keyword,file_type:keyword,chunkDate:date".  add_documents stores these fields of every doc as int32 columns
# next to the vectors and HipIndexer.semantic_search_filtered filters on them.  Empty (the default): no schema, no columns,
# the files of an index are what they were.
RASS_ATTR_FIELDS = os.getenv("RASS_ATTR_FIELDS", "").strip()
# RASS_HYBRID_EXACT: 1 = the hybrid builders answer through the boosted scan (HipIndexer.semantic_search_boosted): the text
# list, read at today's depth, becomes a bonus column and EVERY row gets boost * knn score + its text score, so a text hit
# outside the k-NN list keeps its cosine.  Anything else (the default: 0) = the two ranked lists are fused on the host, as before.
RASS_HYBRID_EXACT = os.getenv("RASS_HYBRID_EXACT", "0").strip() == "1"


def get_index_name(user_id: str) -> str:
    """app/main.py:346-347."""
    return f"{OPENSEARCH_INDEX_NAME}-{user_id}"
