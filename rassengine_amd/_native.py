"""ctypes binding of ``librass_hip.so`` (the C ABI declared in ``include/rass_engine.h``).

There is NO fallback: if the HIP library is missing or fails to load, importing the
product path raises.  A CPU stand-in exists only under ``oracle/`` for the tests.

H1 of SURVEY §7 (two HIP runtimes): ``torch 2.10+rocm7.0`` ships its own
``libamdhip64.so`` with the same soname (``libamdhip64.so.7``) as ROCm 7.2's.  We import
torch first so the HIP runtime torch uses is the one already mapped when
``librass_hip.so`` resolves its ``DT_NEEDED``; device pointers from torch tensors and from
the engine then belong to one runtime.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# RASS_HIP_LIB: A/B another build of the same ABI (kernel experiments); the default is the in-tree library
LIB_PATH = os.environ.get("RASS_HIP_LIB") or os.path.join(_HERE, "lib", "librass_hip.so")

RASS_OK = 0
RASS_MAX_K = 32
RASS_MAX_K_MULTIPASS = 4096
RASS_TAG_PATIENT_MASK = 0x00FFFFFF
RASS_TAG_DOCTYPE_SHIFT = 24
RASS_TAG_DOCTYPE_MASK = 0x7F000000
RASS_MAX_QBATCH = 32
RASS_MAX_DEVICE_BATCH = 4096
RASS_MAX_MMR_FETCH = 128
RASS_MAX_GROUP_SIZE = 16
RASS_F32 = 0
RASS_BF16 = 1
RASS_QFILTER_NONE = -1
RASS_MAX_ATTRS = 8
RASS_ATTR_MISSING = -(1 << 31)
RASS_MAX_ATTR_CLAUSES = 64
RASS_ATTR_ALL, RASS_ATTR_ANY = 0, 1
RASS_ATTR_REPLACE, RASS_ATTR_AND, RASS_ATTR_OR, RASS_ATTR_ANDNOT = 0, 1, 2, 3
RASS_KEY_NONE = -1
RASS_STATS_BY_COUNT, RASS_STATS_BY_VALUE_COUNT, RASS_STATS_BY_MIN, RASS_STATS_BY_MAX = range(4)
RASS_AGG_BY_COUNT, RASS_AGG_BY_SCORE = range(2)
RASS_BOOST_RAW, RASS_BOOST_OPENSEARCH = 0, 1
RASS_BONUS_REPLACE, RASS_BONUS_ADD = 0, 1
(RASS_COMBINE_SUM, RASS_COMBINE_MULTIPLY, RASS_COMBINE_AVG, RASS_COMBINE_MAX, RASS_COMBINE_MIN,
 RASS_COMBINE_REPLACE) = range(6)
RASS_MAX_SCORE_FNS = 16
RASS_FN_GAUSS, RASS_FN_EXP, RASS_FN_LINEAR, RASS_FN_FIELD_VALUE, RASS_FN_WEIGHT = range(5)
(RASS_FN_MOD_NONE, RASS_FN_MOD_LOG, RASS_FN_MOD_LOG1P, RASS_FN_MOD_LOG2P, RASS_FN_MOD_LN, RASS_FN_MOD_LN1P, RASS_FN_MOD_LN2P,
 RASS_FN_MOD_SQUARE, RASS_FN_MOD_SQRT, RASS_FN_MOD_RECIPROCAL) = range(10)
(RASS_FN_SCORE_MULTIPLY, RASS_FN_SCORE_SUM, RASS_FN_SCORE_AVG, RASS_FN_SCORE_FIRST, RASS_FN_SCORE_MAX,
 RASS_FN_SCORE_MIN) = range(6)


class ScoreFn(ctypes.Structure):
    """``rass_score_fn_t``: one function record of ``rass_index_fn_from_attr``."""
    _fields_ = [("query", ctypes.c_int32), ("kind", ctypes.c_int32), ("col", ctypes.c_int32), ("filter", ctypes.c_int32),
                ("modifier", ctypes.c_int32), ("reserved", ctypes.c_int32), ("weight", ctypes.c_double),
                ("origin", ctypes.c_double), ("scale", ctypes.c_double), ("offset", ctypes.c_double), ("decay", ctypes.c_double),
                ("factor", ctypes.c_double), ("missing", ctypes.c_double)]


RASS_MAX_KEY_EDGES = 4097

c_float_p = ctypes.POINTER(ctypes.c_float)
c_i32_p = ctypes.POINTER(ctypes.c_int32)
c_i64_p = ctypes.POINTER(ctypes.c_int64)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes); the export test walks this table against the header.
SIGNATURES = {
    "rass_abi_version": (ctypes.c_int, []),
    "rass_last_error": (ctypes.c_char_p, []),
    "rass_device_count": (ctypes.c_int, []),
    "rass_engine_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, c_void_pp]),
    "rass_engine_destroy": (None, [ctypes.c_void_p]),
    "rass_engine_dim": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_engine_device": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_engine_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rass_engine_reset_stream": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_engine_get_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rass_engine_synchronize": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_index_open": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, c_void_pp]),
    "rass_index_drop": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "rass_index_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "rass_index_rows": (ctypes.c_int64, [ctypes.c_void_p]),
    "rass_index_dtype": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_index_has_global_ids": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_index_dim": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_index_row_stride": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_index_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                      ctypes.c_int, c_i64_p]),
    "rass_index_add_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_int, c_i64_p]),
    "rass_index_add_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_int, ctypes.c_int64, ctypes.c_int, c_i64_p]),
    "rass_index_delete": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "rass_index_compact": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, c_i64_p, c_i64_p]),
    "rass_index_layout_epoch": (ctypes.c_int64, [ctypes.c_void_p]),
    "rass_index_get_row": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rass_index_get_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "rass_index_search": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_multi": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "rass_index_search_device_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                   ctypes.c_void_p]),
    "rass_index_search_device_after": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_device_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_int64, ctypes.c_int64]),
    "rass_index_search_range": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "rass_index_search_range_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_grouped": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int32,
                                                 ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_grouped_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_allowed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "rass_index_search_allowed_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_allow_from_rows": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                                  ctypes.c_int64]),
    "rass_index_allow_from_tag_values": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                                        ctypes.c_void_p, ctypes.c_int64]),
    "rass_index_allow_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, c_i64_p]),
    "rass_index_allow_count": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p]),
    "rass_index_set_attr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "rass_index_get_attr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    "rass_index_attr_mask": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_index_device_attr": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "rass_index_allow_from_attr_clauses": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64]),
    "rass_index_allow_combine": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    "rass_index_search_boosted": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_boosted_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                        ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                        ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_bonus_scatter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "rass_index_bonus_scatter_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]),
    "rass_index_bonus_from_attr_clauses": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int]),
    "rass_index_bonus_mask": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_int64]),
    "rass_index_search_scored": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "rass_index_search_scored_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_fn_from_attr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_double, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                               ctypes.c_int64]),
    "rass_index_aggregate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_aggregate_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_keys_from_attr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    "rass_index_keys_from_attr_edges": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    "rass_index_keys_from_tag": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    "rass_index_attr_minmax": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_grouped_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_grouped_keys_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_group_hits_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_search_group_hits_keys_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_aggregate_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_aggregate_keys_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_aggregate_stats_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_aggregate_stats_keys_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_aggregate_hits_keys": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_aggregate_hits_keys_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_rows_gram": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "rass_index_rows_gram_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_void_p]),
    "rass_index_search_mmr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "rass_index_search_mmr_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_set_prefilter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rass_index_get_prefilter": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_index_candidates_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_certify_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_candidates_exact_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_void_p]),
    "rass_index_sample_floor_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_step_floors_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_void_p, ctypes.c_void_p]),
    "rass_index_save": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "rass_index_load": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, c_void_pp]),
    "rass_index_fill_synthetic": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64,
                                                 ctypes.c_int64]),
    "rass_scan_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "rass_scan_topk_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "rass_pack_rows_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p]),
    "rass_unpack_rows_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rass_gather_rows_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rass_compact_plan": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "rass_compact_plan_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64]),
    "rass_compact_rows_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_void_p]),
    "rass_topk_merge": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_topk_merge_strided": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p]),
    "rass_topk_merge_strided_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                     ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_void_p]),
    "rass_normalize_rows_f32": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "rass_peer_buffer_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_size_t, c_void_pp, ctypes.c_char_p]),
    "rass_peer_buffer_open": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, c_void_pp]),
    "rass_peer_buffer_close": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rass_peer_post": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_uint64, ctypes.c_void_p]),
    "rass_peer_wait": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p,
                                      ctypes.c_int64, ctypes.c_void_p]),
    "rass_kmeans_assign": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_kmeans_accumulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "rass_ivf_save": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "rass_ivf_load": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, c_void_pp]),
    "rass_ivf_build": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, c_void_pp]),
    "rass_ivf_destroy": (None, [ctypes.c_void_p]),
    "rass_ivf_build_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                         c_void_pp]),
    "rass_ivf_dtype": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_ivf_rows": (ctypes.c_int64, [ctypes.c_void_p]),
    "rass_ivf_nlist": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_ivf_search": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i64_p]),
    "rass_ivf_search_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_ivf_search_device_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p]),
    "rass_ivf_build_prefix": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_int64, c_void_pp]),
    "rass_ivf_covered_rows": (ctypes.c_int64, [ctypes.c_void_p]),
    "rass_ivf_delete": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "rass_ivf_search_delta": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, c_i64_p]),
    "rass_ivf_search_delta_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                    ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_void_p]),
    "rass_ivf_search_allowed_delta": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_i64_p]),
    "rass_ivf_search_allowed_delta_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                            ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                            ctypes.c_void_p]),
    "rass_ivf_probe_lists": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "rass_ivf_plan_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "rass_ivf_plan_lists": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "rass_ivf_build_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_int64, c_void_pp]),
    "rass_ivf_absorb": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, c_void_pp]),
    "rass_ivf_lists_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    "rass_encoder_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, c_void_pp]),
    "rass_encoder_destroy": (None, [ctypes.c_void_p]),
    "rass_encoder_hidden": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_encoder_get_stream": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rass_encoder_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rass_encoder_set_weight": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64]),
    "rass_encoder_finalize": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rass_encode_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_gemm_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_void_p]),
    "rass_gemm_bf16_ws": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "rass_attention_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_attention_out_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_int, ctypes.c_void_p]),
    "rass_embed_layernorm_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "rass_layernorm_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_gemm_bf16_residual_layernorm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                                         ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                         ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "rass_gemm_bf16_ln_input": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "rass_fold_gamma_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rass_gemm_bf16_fold": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    "rass_gemm_bf16_route": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]),
    "rass_ln_stats_finalize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p,
                                              ctypes.c_void_p]),
    "rass_pool_bf16": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "rass_tokenizer_create": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, c_void_pp]),
    "rass_tokenizer_destroy": (None, [ctypes.c_void_p]),
    "rass_tokenizer_vocab_size": (ctypes.c_int, [ctypes.c_void_p]),
    "rass_tokenizer_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_void_p]),
    "rass_tokenizer_encode_batch": (ctypes.c_int64, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p),
                                                     ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_int]),
    "rass_timer_create": (ctypes.c_int, [c_void_pp]),
    "rass_timer_destroy": (None, [ctypes.c_void_p]),
    "rass_timer_start": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rass_timer_stop": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rass_timer_elapsed_ms": (ctypes.c_int, [ctypes.c_void_p, c_float_p]),
    "rass_engine_kernel_timing_begin": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rass_engine_kernel_timing_end": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double),
                                                     ctypes.POINTER(ctypes.c_int)]),
    "rass_index_device_rows": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rass_index_device_tags": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rass_scan_kernel_name": (ctypes.c_char_p, [ctypes.c_int, ctypes.c_int]),
}

_lib: Optional[ctypes.CDLL] = None


class RassError(RuntimeError):
    """A C-ABI call returned a negative rass_status."""

    def __init__(self, fn: str, code: int, text: str):
        super().__init__(f"{fn} failed ({code}): {text}")
        self.code = code


def lib() -> ctypes.CDLL:
    """Load librass_hip.so once.  Raises (never falls back) when it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C rassengine_amd/csrc`. rassengine_amd has no CPU fallback.")
    try:
        import torch  # noqa: F401  -- map torch's HIP runtime first (see module docstring)
    except Exception:  # torch-free C/ctypes users link against the system ROCm instead
        pass
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError = header/library mismatch: fail loudly
        fn.restype = restype
        fn.argtypes = argtypes
    if L.rass_abi_version() != 1:
        raise ImportError(f"librass_hip.so ABI {L.rass_abi_version()} != 1")
    _lib = L
    return L


def check(fn: str, code: int) -> int:
    if code < 0:
        raise RassError(fn, code, lib().rass_last_error().decode("utf-8", "replace"))
    return code
