"""ctypes mirror of include/ratelimit_hip.h (data layout only; loads no library)."""
import ctypes as C

import numpy as np

RL_OK, RL_E_INVALID, RL_E_TABLE_FULL, RL_E_ARENA_FULL, RL_E_HIP, RL_E_CAPACITY, RL_E_TIME, \
    RL_E_COMM, RL_E_INTERNAL = range(9)
STATUS_NAMES = {0: "RL_OK", 1: "RL_E_INVALID", 2: "RL_E_TABLE_FULL", 3: "RL_E_ARENA_FULL",
                4: "RL_E_HIP", 5: "RL_E_CAPACITY", 6: "RL_E_TIME", 7: "RL_E_COMM", 8: "RL_E_INTERNAL"}
RL_FLAG_SHADOW = 1
RL_NUM_STATS = 6
STAT_FIELDS = ("total_hits", "over_limit", "near_limit", "over_limit_with_local_cache",
               "within_limit", "shadow_mode")

P = C.c_void_p


class RlConfig(C.Structure):
    _fields_ = [("table_slots", C.c_uint64), ("arena_bytes", C.c_uint64),
                ("max_batch", C.c_uint32), ("max_requests", C.c_uint32),
                ("max_rules", C.c_uint32), ("max_stem_bytes", C.c_uint32),
                ("near_limit_ratio", C.c_float), ("local_cache_enabled", C.c_int32),
                ("per_second_split", C.c_int32), ("device", C.c_int32),
                ("expiration_jitter_max_seconds", C.c_int64), ("hash_seed", C.c_uint64),
                ("n_shards", C.c_uint32), ("debug_hash_bits", C.c_uint32), ("shard_device", C.c_int32 * 16),
                ("history_entries", C.c_uint64), ("reserved", C.c_int32 * 6)]


class RlBatch(C.Structure):
    _fields_ = [("n", C.c_uint32), ("n_requests", C.c_uint32), ("n_rules", C.c_uint32),
                ("reserved", C.c_uint32), ("stem_bytes", P), ("stem_off", P), ("now", P),
                ("req_idx", P), ("unit", P), ("flags", P), ("limit", P), ("hits", P),
                ("rule_id", P)]


# rl_limit (12 B): one entry of a compact batch's limit table
LIMIT_DTYPE = np.dtype([("requests_per_unit", np.uint32), ("rule_id", np.uint32), ("unit", np.uint8),
                        ("flags", np.uint8), ("reserved", np.uint16)])


class RlLimit(C.Structure):
    _fields_ = [("requests_per_unit", C.c_uint32), ("rule_id", C.c_uint32), ("unit", C.c_uint8),
                ("flags", C.c_uint8), ("reserved", C.c_uint16)]


assert LIMIT_DTYPE.itemsize == C.sizeof(RlLimit)


class RlBatchCompact(C.Structure):
    _fields_ = [("n", C.c_uint32), ("n_requests", C.c_uint32), ("n_rules", C.c_uint32), ("n_limits", C.c_uint32),
                ("buf", P), ("buf_bytes", C.c_uint64), ("stem_bytes", C.c_uint64), ("stem_off", C.c_uint64),
                ("limit_idx", C.c_uint64), ("req_first", C.c_uint64), ("now", C.c_uint64), ("hits", C.c_uint64),
                ("limits", C.c_uint64)]


RL_PREFIXED_TILE = 256  # include/ratelimit_hip.h: requests per index tile


class RlBatchPrefixed(C.Structure):
    _fields_ = [("n", C.c_uint32), ("n_requests", C.c_uint32), ("n_rules", C.c_uint32), ("n_limits", C.c_uint32),
                ("buf", P), ("buf_bytes", C.c_uint64), ("req", C.c_uint64), ("now", C.c_uint64),
                ("hits", C.c_uint64), ("desc", C.c_uint64), ("prefix_bytes", C.c_uint64),
                ("suffix_bytes", C.c_uint64), ("limits", C.c_uint64), ("index", C.c_uint64)]


class RlResult(C.Structure):
    _fields_ = [("code", P), ("limit_remaining", P), ("reset_s", P), ("stats", P), ("status", P)]


class RlRestoreBatch(C.Structure):
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("stem_bytes", P), ("stem_off", P),
                ("unit", P), ("now", P), ("count", P), ("lc", P)]


class RlTableInfo(C.Structure):
    _fields_ = [("table_slots", C.c_uint64), ("live_slots", C.c_uint64), ("tombstones", C.c_uint64),
                ("arena_bytes_used", C.c_uint64), ("exact_stems", C.c_uint64),
                ("batches", C.c_uint64), ("decisions", C.c_uint64),
                ("history_entries", C.c_uint64), ("history_appended", C.c_uint64),
                ("history_lost", C.c_uint64), ("history_slots", C.c_uint64), ("history_refused", C.c_uint64)]


class RlLogTear(C.Structure):
    """rl_log_tear (include/ratelimit_hip.h): rl_debug_log_tear's armed tear and its outcome."""
    _fields_ = [("armed", C.c_uint32), ("protocol", C.c_uint32), ("sched", C.c_uint32 * 3),
                ("entry", C.c_uint32 * 8), ("before", C.c_uint32 * 8), ("seen", C.c_uint32 * 12),
                ("verdict", C.c_int32), ("reserved", C.c_uint32)]


class RlConfigNode(C.Structure):
    _fields_ = [("parent", C.c_int32), ("key_off", C.c_uint32), ("key_len", C.c_uint32),
                ("requests_per_unit", C.c_uint32), ("rule_id", C.c_uint32), ("unit", C.c_uint8),
                ("has_limit", C.c_uint8), ("unlimited", C.c_uint8), ("shadow_mode", C.c_uint8)]


# numpy view of rl_config_node (24 B), for building the node array in one go
CONFIG_NODE_DTYPE = np.dtype([("parent", np.int32), ("key_off", np.uint32), ("key_len", np.uint32),
                              ("requests_per_unit", np.uint32), ("rule_id", np.uint32), ("unit", np.uint8),
                              ("has_limit", np.uint8), ("unlimited", np.uint8), ("shadow_mode", np.uint8)])


class RlConfigTree(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("cache_key_prefix_len", C.c_uint32), ("nodes", P),
                ("key_bytes", P), ("key_bytes_len", C.c_uint64), ("cache_key_prefix", P)]


class RlRequestBatch(C.Structure):
    _fields_ = [("n_requests", C.c_uint32), ("n_descriptors", C.c_uint32), ("n_entries", C.c_uint32),
                ("n_rules", C.c_uint32), ("domain_bytes", P), ("domain_off", P), ("now", P), ("hits", P),
                ("req_idx", P), ("entry_first", P), ("desc_off", P), ("desc_bytes", P), ("key_len", P),
                ("value_len", P), ("override_flags", P), ("override_rpu", P), ("override_unit", P),
                ("override_rule", P)]


class RlRequestResult(C.Structure):
    _fields_ = [("code", P), ("limit_remaining", P), ("reset_s", P), ("match", P), ("rule_id", P),
                ("requests_per_unit", P), ("unit", P), ("stats", P)]


RL_NO_DESCRIPTOR = 0xFFFFFFFF
RL_VERDICT_OVER_LIMIT, RL_VERDICT_GLOBAL_SHADOW = 1, 2  # rl_request_verdict.flags
RL_VERDICT_OPT_GLOBAL_SHADOW = 1  # rl_do_limit_requests_verdict opts


class RlRequestVerdict(C.Structure):
    """rl_request_verdict: per request, the overall code and the header descriptor's values."""
    _fields_ = [("overall_code", P), ("flags", P), ("min_descriptor", P), ("header_limit", P),
                ("header_remaining", P), ("header_reset_s", P), ("global_shadow", P)]


RL_REQUESTS_TILE = 256  # include/ratelimit_hip.h
RL_REQUESTS_INFLIGHT = 4  # include/ratelimit_hip.h (packed request batches waiting for their second half)


class RlRequestOverride(C.Structure):
    """rl_request_override: one entry of a packed request batch's sparse override list."""
    _fields_ = [("descriptor", C.c_uint32), ("requests_per_unit", C.c_uint32), ("rule_id", C.c_uint32),
                ("unit", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class RlRequestBatchPacked(C.Structure):
    """rl_request_batch_packed: rl_request_batch in one pinned buffer (sections as byte offsets)."""
    _fields_ = [("n_requests", C.c_uint32), ("n_descriptors", C.c_uint32), ("n_entries", C.c_uint32),
                ("n_rules", C.c_uint32), ("n_overrides", C.c_uint32), ("reserved", C.c_uint32), ("buf", P),
                ("buf_bytes", C.c_uint64), ("req", C.c_uint64), ("now", C.c_uint64), ("hits", C.c_uint64),
                ("desc", C.c_uint64), ("key_len", C.c_uint64), ("value_len", C.c_uint64),
                ("domain_bytes", C.c_uint64), ("entry_bytes", C.c_uint64), ("overrides", C.c_uint64),
                ("index", C.c_uint64)]


RL_WIRE_TILE = 256  # include/ratelimit_hip.h
RL_WIRE_OK, RL_WIRE_DEFERRED, RL_WIRE_MALFORMED = 0, 1, 2  # enum rl_wire_status


class RlWireBatch(C.Structure):
    """rl_wire_batch: serialized RateLimitRequest payloads in one pinned buffer (sections as byte offsets)."""
    _fields_ = [("n_requests", C.c_uint32), ("n_rules", C.c_uint32), ("buf", P), ("buf_bytes", C.c_uint64),
                ("msg_off", C.c_uint64), ("now", C.c_uint64), ("msgs", C.c_uint64), ("msgs_bytes", C.c_uint64)]


class RlWireResult(C.Structure):
    """rl_wire_result: per-message status and each request's first descriptor (rl_do_limit_wire_async)."""
    _fields_ = [("req_status", P), ("desc_first", P), ("n_descriptors", P), ("desc_cap", C.c_uint32),
                ("reserved", C.c_uint32)]


class RlOverrideRulesConfig(C.Structure):
    """rl_override_rules_config: the rule ids and the room of the device-interned override stats keys."""
    _fields_ = [("first_rule", C.c_uint32), ("capacity", C.c_uint32), ("key_bytes", C.c_uint64),
                ("reserved", C.c_uint32 * 4)]


class RlOverrideRulesInfo(C.Structure):
    """rl_override_rules_info: what rl_override_rules_info_get reports."""
    _fields_ = [("first_rule", C.c_uint32), ("capacity", C.c_uint32), ("rules", C.c_uint32), ("reserved", C.c_uint32),
                ("key_bytes_used", C.c_uint64), ("key_bytes_cap", C.c_uint64), ("deferred_full", C.c_uint64)]


RL_RESPONSE_KEY_MAX = 64  # include/ratelimit_hip.h
RL_RESPONSE_STATUS_MAX = 26


class RlResponseFormat(C.Structure):
    """rl_response_format: the three RateLimit-* header names of the serialized responses (all NULL: no headers)."""
    _fields_ = [("limit_key", P), ("remaining_key", P), ("reset_key", P), ("limit_key_len", C.c_uint16),
                ("remaining_key_len", C.c_uint16), ("reset_key_len", C.c_uint16), ("reserved", C.c_uint16)]


class RlResponseBatch(C.Structure):
    """rl_response_batch: the serialized RateLimitResponse payloads and their offsets (host memory)."""
    _fields_ = [("bytes", P), ("bytes_cap", C.c_uint64), ("resp_off", P)]


def make_response_format(header_keys):
    """(limit, remaining, reset) header names as bytes, or None for no headers ->
    (RlResponseFormat, the buffers it points into)."""
    f = RlResponseFormat()
    keep = []
    if header_keys is not None:
        for name, k in zip(("limit_key", "remaining_key", "reset_key"), header_keys):
            b = C.create_string_buffer(bytes(k), max(len(k), 1))
            keep.append(b)
            setattr(f, name, C.cast(b, P))
            setattr(f, name + "_len", len(k))
    return f, keep


# the per-request arrays of rl_request_verdict (global_shadow apart: one uint64)
REQUEST_VERDICT_DTYPES = {"overall_code": np.uint8, "flags": np.uint8, "min_descriptor": np.uint32,
                          "header_limit": np.uint32, "header_remaining": np.uint32, "header_reset_s": np.uint32}


class RlLocalCacheInfo(C.Structure):
    _fields_ = [("entry_count", C.c_uint64), ("lookup_count", C.c_uint64), ("hit_count", C.c_uint64),
                ("miss_count", C.c_uint64)]


RL_REC_CHAIN_LOST = 1  # rl_records.flags: older windows of the key may have had records the log lost


class RlRecords(C.Structure):
    """rl_records: portable window records, one per (stem, unit, window) (rl_export_range / rl_import)."""
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("stem_cap", C.c_uint64), ("stem_bytes", P),
                ("stem_off", P), ("unit", P), ("flags", P), ("ws", P), ("count", P), ("expire", P), ("lc", P)]


class RlExportInfo(C.Structure):
    _fields_ = [("shard_slots", C.c_uint64), ("records", C.c_uint64), ("stem_bytes", C.c_uint64),
                ("keys", C.c_uint64), ("chains_lost", C.c_uint64), ("time_floor", C.c_int64)]


# the per-record arrays of rl_records (stem_bytes / stem_off apart)
RECORD_DTYPES = {"unit": np.uint8, "flags": np.uint8, "ws": np.uint32, "count": np.uint32,
                 "expire": np.uint32, "lc": np.uint32}


class RlKeys(C.Structure):
    """rl_keys: the (stem, unit, clock) keys of one rl_lookup call."""
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("stem_bytes", P), ("stem_off", P), ("unit", P),
                ("now", P)]


class RlKeyState(C.Structure):
    """rl_key_state: rl_lookup's answers, one per key."""
    _fields_ = [("status", P), ("found", P), ("count", P), ("expire", P), ("lc", P)]


# the per-key arrays of rl_key_state
KEY_STATE_DTYPES = {"status": np.uint8, "found": np.uint8, "count": np.uint32, "expire": np.uint32, "lc": np.uint32}

RL_HOT_BLOCKED = 1  # rl_hot_query.flags: only keys whose local over-limit cache entry is live (now < lc)


class RlHotQuery(C.Structure):
    """rl_hot_query: what rl_hot_keys selects (the table read at `now`)."""
    _fields_ = [("now", C.c_int64), ("k", C.c_uint32), ("min_count", C.c_uint32), ("unit_mask", C.c_uint32),
                ("flags", C.c_uint32)]


class RlHotInfo(C.Structure):
    """rl_hot_info: totals of the records that satisfy an rl_hot_query."""
    _fields_ = [("slots", C.c_uint64), ("matched", C.c_uint64), ("hits", C.c_uint64), ("above", C.c_uint64),
                ("threshold", C.c_uint32), ("reserved", C.c_uint32), ("time_floor", C.c_int64)]


class RlResizeInfo(C.Structure):
    """rl_resize_info: what one rl_resize moved (summed over shards; longest_probe the maximum)."""
    _fields_ = [("slots_before", C.c_uint64), ("slots_after", C.c_uint64), ("keys", C.c_uint64),
                ("tombstones_dropped", C.c_uint64), ("log_entries_relinked", C.c_uint64),
                ("longest_probe", C.c_uint32), ("reserved", C.c_uint32)]


class RlHistoryResizeInfo(C.Structure):
    """rl_history_resize_info: what one rl_resize_history kept and dropped (summed over
    shards; longest_chain and fill_max the maxima)."""
    _fields_ = [("entries_before", C.c_uint64), ("entries_after", C.c_uint64), ("written_before", C.c_uint64),
                ("entries_kept", C.c_uint64), ("entries_dropped", C.c_uint64), ("chains", C.c_uint64),
                ("chains_lost", C.c_uint64), ("fill_max", C.c_uint64), ("longest_chain", C.c_uint32),
                ("reserved", C.c_uint32)]


RL_FORGET_PREFIX = 1   # rl_stems.flags: every entry is a stem prefix, not a whole stem
RL_FORGET_DRY_RUN = 2  # select and count, change nothing
RL_FORGET_PREFIX_MAX = 64      # prefixes per call
RL_FORGET_PREFIX_BYTES = 4096  # their bytes per call


class RlStems(C.Structure):
    """rl_stems: the stems (or stem prefixes) of one rl_forget call."""
    _fields_ = [("n", C.c_uint32), ("flags", C.c_uint32), ("stem_bytes", P), ("stem_off", P)]


class RlForgetInfo(C.Structure):
    """rl_forget_info: what one rl_forget removed (summed over shards)."""
    _fields_ = [("slots_scanned", C.c_uint64), ("keys", C.c_uint64), ("keys_with_history", C.c_uint64),
                ("arena_bytes", C.c_uint64)]


RL_SCAN_NEWEST = 1   # rl_scan_query.flags: only each key's newest window record (the history log is never walked)
RL_SCAN_LIVE = 2     # only records whose Redis key exists at the query's now: now <= expire
RL_SCAN_TILE = 1024  # a cursor advances in whole tiles of this many slots


class RlScanQuery(C.Structure):
    """rl_scan_query: which keys and records one rl_scan call selects."""
    _fields_ = [("n_prefixes", C.c_uint32), ("flags", C.c_uint32), ("prefix_bytes", P), ("prefix_off", P),
                ("now", C.c_int64), ("unit_mask", C.c_uint32), ("reserved", C.c_uint32)]


class RlScanCursor(C.Structure):
    """rl_scan_cursor: where the next page starts (all zero: the start; shard == n_shards: done)."""
    _fields_ = [("shard", C.c_uint32), ("reserved", C.c_uint32), ("slot", C.c_uint64)]


class RlScanPrefixSum(C.Structure):
    """rl_scan_prefix_sum: one page's keys, records and summed counts under one prefix."""
    _fields_ = [("keys", C.c_uint64), ("records", C.c_uint64), ("hits", C.c_uint64)]


class RlScanInfo(C.Structure):
    """rl_scan_info: sums over the tiles one rl_scan call covered."""
    _fields_ = [("slots_scanned", C.c_uint64), ("keys", C.c_uint64), ("records", C.c_uint64),
                ("stem_bytes", C.c_uint64), ("chains_lost", C.c_uint64), ("need_records", C.c_uint64),
                ("need_stem_bytes", C.c_uint64), ("time_floor", C.c_int64)]


RL_MATCH_NONE, RL_MATCH_UNLIMITED, RL_MATCH_LIMIT = 0, 1, 2
REQUEST_ARRAYS = ("domain_bytes", "domain_off", "now", "hits", "req_idx", "entry_first", "desc_off", "desc_bytes",
                  "key_len", "value_len", "override_flags", "override_rpu", "override_unit", "override_rule")
REQUEST_DTYPES = {"domain_bytes": np.uint8, "domain_off": np.uint32, "now": np.int64, "hits": np.uint32,
                  "req_idx": np.uint32, "entry_first": np.uint32, "desc_off": np.uint32, "desc_bytes": np.uint8,
                  "key_len": np.uint16, "value_len": np.uint16, "override_flags": np.uint8,
                  "override_rpu": np.uint32, "override_unit": np.uint8, "override_rule": np.uint32}
REQUEST_RESULT_DTYPES = {"code": np.uint8, "limit_remaining": np.uint32, "reset_s": np.uint32, "match": np.uint8,
                         "rule_id": np.uint32, "requests_per_unit": np.uint32, "unit": np.uint8}


def ptr(a):
    """Address of a numpy array (host) or a torch tensor (device) as c_void_p."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(a.data_ptr())  # torch.Tensor


BATCH_ARRAYS = ("stem_bytes", "stem_off", "now", "req_idx", "unit", "flags", "limit", "hits", "rule_id")
BATCH_DTYPES = {"stem_bytes": np.uint8, "stem_off": np.uint32, "now": np.int64, "req_idx": np.uint32,
                "unit": np.uint8, "flags": np.uint8, "limit": np.uint32, "hits": np.uint32,
                "rule_id": np.uint32}
RESULT_DTYPES = {"code": np.uint8, "limit_remaining": np.uint32, "reset_s": np.uint32, "stats": np.uint64,
                 "status": np.uint8}
ABI_VERSION = 8
RL_COMM_ID_BYTES = 128  # include/ratelimit_hip.h
RL_ROUTED_INFLIGHT = 6  # include/ratelimit_hip.h (routed batches in flight: the input-reuse distance)
RL_ROUTED_LAG = 3  # include/ratelimit_hip.h (calls between a routed batch's partition and its owner pipeline)


def make_batch_struct(arrays, n, n_requests, n_rules):
    b = RlBatch()
    b.n, b.n_requests, b.n_rules = n, n_requests, n_rules
    for k in BATCH_ARRAYS:
        setattr(b, k, ptr(arrays[k]))
    return b


def make_result_struct(arrays):
    r = RlResult()
    for k in ("code", "limit_remaining", "reset_s", "stats", "status"):
        setattr(r, k, ptr(arrays.get(k)))
    return r
