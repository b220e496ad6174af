"""ctypes binding of ``include/bsdb_mi355x.h`` (``libbsdb_mi355x.so``).

This is the product path: every call lands in a hand-written gfx950 kernel.
There is no CPU fallback -- if the library is missing or a call fails, a
:class:`BsdbError` is raised (mirroring the reference's JNI convention of
negative return codes turned into exceptions, ``src/main/c/native.c:29-34``).

Device buffers are ``torch`` tensors (torch is plumbing here: HBM allocation,
streams, ``torch.distributed``); the C ABI itself takes plain pointers.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
# BSDB_LIB: an alternative in-tree build of the same library (tools/ variant
# experiments); the default is the product build
LIB_PATH = os.environ.get("BSDB_LIB") or os.path.join(HERE, "libbsdb_mi355x.so")
HEADER = os.path.join(os.path.dirname(HERE), "include", "bsdb_mi355x.h")

BSDB_OK = 0
ERRORS = {-22: "EINVAL", -12: "ENOMEM", -5: "EIO", -19: "ENODEV", -17: "EDUP", -34: "ESEEDS", -7: "E2BIG",
          -70: "ECOMM", -9: "EFILE", -74: "EVERIFY"}
COMM_ID_BYTES = 128

# (name, restype, argtypes) -- kept in the order of include/bsdb_mi355x.h
_vp, _u64, _u32, _i = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SIGNATURES = [
    ("bsdb_abi_version", _i, []),
    ("bsdb_strerror", C.c_char_p, [_i]),
    ("bsdb_open", _i, [_i, C.POINTER(_vp)]),
    ("bsdb_close", _i, [_vp]),
    ("bsdb_num_buckets", _u64, [_u64]),
    ("bsdb_dev_hash_fixed", _i, [_vp, _vp, _u32, _u64, _u64, _vp, _vp]),
    ("bsdb_dev_hash_var", _i, [_vp, _vp, _u64, _vp, _u64, _u64, _vp, _vp]),
    ("bsdb_dev_histogram_fixed", _i, [_vp, _vp, _u32, _u64, _u64, _u64, _vp, _vp]),
    ("bsdb_dev_histogram_var", _i, [_vp, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    ("bsdb_dev_edge_offsets", _i, [_vp, _vp, _u64, _vp, _vp]),
    ("bsdb_dev_lookup", _i, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _u32, _vp, _i, _vp, _vp]),
    ("bsdb_dev_sign", _i, [_vp, _vp, _u64, _u64, _vp, _vp, _u32, _vp, _vp]),
    ("bsdb_dev_index_scatter", _i, [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_values_words", _u64, [_u64]),
    ("bsdb_dev_gov_build", _i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_gov_build_ranks", _i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_gov_build_range", _i, [_vp, _vp, _u64, _u64, _u64, _u64, _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_gov_range_windows", _i, [_u64, _u32, _u64, _u64, _vp]),
    ("bsdb_dev_gov_build_window", _i, [_vp, _vp, _u64, _u64, _u64, _u64, _u64, _u32, _vp, _vp, _u64, _u64, _vp, _u64,
                                       _u64, _vp, _vp]),
    ("bsdb_dev_mph_build_index_passes_fixed", _i, [_vp, _vp, _u32, _u64, _u32, _u32, _vp, _u64, _u64, _vp, _vp,
                                                   _vp, _vp, _vp, C.POINTER(_u32), _vp]),
    ("bsdb_dev_mph_build_index_passes_var", _i, [_vp, _vp, _u64, _vp, _u64, _u32, _u32, _vp, _u64, _u64, _vp, _vp,
                                                 _vp, _vp, _vp, C.POINTER(_u32), _vp]),
    ("bsdb_dev_partition_owners", _i, [_vp, _vp, _vp, _u64, _u64, _i, _vp, _vp, _vp, _vp]),
    ("bsdb_release_workspace", _i, [_vp]),
    ("bsdb_set_verify", _i, [_vp, _i]),
    ("bsdb_set_histogram_mode", _i, [_vp, _i]),
    ("bsdb_set_frontend", _i, [_vp, _i]),
    ("bsdb_set_chunk_keys", _i, [_vp, _u64]),
    ("bsdb_set_pipeline", _i, [_vp, _i, _u64, _u32]),
    ("bsdb_fallback_count", _i, [_vp, C.POINTER(_u64)]),
    ("bsdb_fused_status", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    ("bsdb_set_profiling", _i, [_vp, _i]),
    ("bsdb_profile_read", _i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(_u64), C.POINTER(_u64)]),
    ("bsdb_histogram_fixed", _i, [_vp, _vp, _u32, _u64, _u64, _u64, _vp]),
    ("bsdb_hash_fixed", _i, [_vp, _vp, _u32, _u64, _u64, _vp]),
    ("bsdb_histogram_var", _i, [_vp, _vp, _vp, _u64, _u64, _u64, _vp]),
    ("bsdb_hash_var", _i, [_vp, _vp, _vp, _u64, _u64, _vp]),
    ("bsdb_dev_gen_keys13", _i, [_vp, _u64, _u64, _vp, _vp]),
    ("bsdb_dev_gen_keys_var", _i, [_vp, _u64, _u64, _vp, _vp, _u64, _vp]),
    ("bsdb_comm_available", _i, []),
    ("bsdb_comm_unique_id", _i, [_vp]),
    ("bsdb_comm_init", _i, [_vp, _i, _i, _vp]),
    ("bsdb_dev_histogram_finalize", _i, [_vp, _vp, _u64, _u64, _vp, _vp]),
    ("bsdb_dev_allreduce_u64", _i, [_vp, _vp, _u64, _vp]),
    ("bsdb_multi_open", _i, [_i, _vp, C.POINTER(_vp)]),
    ("bsdb_multi_close", _i, [_vp]),
    ("bsdb_multi_size", _i, [_vp]),
    ("bsdb_multi_ctx", _i, [_vp, _i, C.POINTER(_vp)]),
    ("bsdb_multi_histogram_fixed", _i, [_vp, _vp, _u32, _u64, _u64, _vp]),
    ("bsdb_multi_histogram_var", _i, [_vp, _vp, _vp, _u64, _u64, _vp]),
    ("bsdb_multi_mph_build_index_fixed", _i, [_vp, _vp, _u32, _u64, _u32, _vp, _vp, _vp, _i, C.c_char_p, C.c_char_p,
                                              _vp, _vp, _vp]),
    ("bsdb_multi_mph_build_index_var", _i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _i, C.c_char_p, C.c_char_p,
                                            _vp, _vp, _vp]),
    ("bsdb_mph_build_fixed", _i, [_vp, _vp, _u32, _u64, _u32, C.POINTER(_vp)]),
    ("bsdb_mph_build_var", _i, [_vp, _vp, _vp, _u64, _u32, C.POINTER(_vp)]),
    ("bsdb_mph_build_index_fixed", _i, [_vp, _vp, _u32, _u64, _u32, _vp, _vp, _vp, _i, C.c_char_p, C.c_char_p,
                                        C.POINTER(_vp)]),
    ("bsdb_mph_build_index_var", _i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _i, C.c_char_p, C.c_char_p,
                                      C.POINTER(_vp)]),
    ("bsdb_mph_info", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u32), C.POINTER(_u64), C.POINTER(_u64)]),
    ("bsdb_mph_sizes", _i, [_u64, _u32, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    ("bsdb_mph_export", _i, [_vp, _vp, _vp, _vp]),
    ("bsdb_mph_import", _i, [_vp, _u64, _u32, _vp, _vp, _vp, C.POINTER(_vp)]),
    ("bsdb_mph_dump", _i, [_vp, C.c_char_p]),
    ("bsdb_mph_load", _i, [_vp, C.c_char_p, C.POINTER(_vp)]),
    ("bsdb_mph_lookup_fixed", _i, [_vp, _vp, _u32, _u64, _i, _vp]),
    ("bsdb_mph_lookup_var", _i, [_vp, _vp, _vp, _u64, _i, _vp]),
    ("bsdb_mph_free", _i, [_vp]),
    ("bsdb_mph_build_index_passes_fixed", _i, [_vp, _vp, _u32, _u64, _u32, _vp, _u64, _u64, _vp, _vp, _i, _u32,
                                               C.c_char_p, C.c_char_p, C.POINTER(_vp), C.POINTER(_u32)]),
    ("bsdb_mph_build_index_passes_var", _i, [_vp, _vp, _vp, _u64, _u32, _vp, _u64, _u64, _vp, _vp, _i, _u32,
                                             C.c_char_p, C.c_char_p, C.POINTER(_vp), C.POINTER(_u32)]),
    ("bsdb_builder_open", _i, [_vp, _u32, _u64, _u64, _i, _u64, _u64, C.POINTER(_vp)]),
    ("bsdb_builder_add_fixed", _i, [_vp, _vp, _u32, _u64, _vp, _vp, _vp]),
    ("bsdb_builder_add_var", _i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    ("bsdb_builder_count", _i, [_vp, C.POINTER(_u64)]),
    ("bsdb_builder_finish", _i, [_vp, _u32, _u32, C.c_char_p, C.c_char_p, C.POINTER(_vp), C.POINTER(_u32)]),
    ("bsdb_builder_free", _i, [_vp]),
    ("bsdb_index_open", _i, [_vp, _i, _u64, C.c_char_p, C.c_char_p, C.POINTER(_vp), C.POINTER(_u64)]),
    ("bsdb_index_begin_pass", _i, [_vp, _u64]),
    ("bsdb_index_put_var", _i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    ("bsdb_index_put_fixed", _i, [_vp, _vp, _u32, _u64, _vp, _vp, _vp]),
    ("bsdb_index_end_pass", _i, [_vp]),
    ("bsdb_index_close", _i, [_vp]),
    ("bsdb_kv_scan", _i, [C.c_char_p, _i, _i, _u32, _i, C.POINTER(_vp)]),
    ("bsdb_kv_records_info", _i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u32)]),
    ("bsdb_kv_records_arrays", _i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                                    C.POINTER(_vp)]),
    ("bsdb_kv_records_free", _i, [_vp]),
    ("bsdb_kv_build_index", _i, [_vp, C.c_char_p, _i, _i, _u32, _i, _u32, _i, C.c_char_p, C.c_char_p,
                                 C.POINTER(_vp)]),
    ("bsdb_dev_verify_fixed", _i, [_vp, _vp, _u32, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _u64, _vp, _vp, _u32,
                                   _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_verify_var", _i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _u64, _vp, _vp,
                                 _u32, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    ("bsdb_mph_verify_index_fixed", _i, [_vp, _vp, _u32, _u64, _vp, _vp, _vp, _i, C.c_char_p, C.c_char_p, _u32, _vp]),
    ("bsdb_mph_verify_index_var", _i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, C.c_char_p, C.c_char_p, _u32, _vp]),
    ("bsdb_kv_verify_index", _i, [_vp, C.c_char_p, _i, _i, _u32, _i, _i, C.c_char_p, C.c_char_p, _u32, _vp]),
    ("bsdb_dev_find_duplicates_fixed", _i, [_vp, _vp, _u32, _u64, _u32, _u64, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_find_duplicates_var", _i, [_vp, _vp, _u64, _vp, _u64, _u32, _u64, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_find_duplicates_sig", _i, [_vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    ("bsdb_dev_classify_pairs_fixed", _i, [_vp, _vp, _u32, _u64, _vp, _u64, _vp, _vp]),
    ("bsdb_dev_classify_pairs_var", _i, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    ("bsdb_find_duplicates_fixed", _i, [_vp, _vp, _u32, _u64, _u64, _vp, _vp, _vp]),
    ("bsdb_find_duplicates_var", _i, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    ("bsdb_builder_find_duplicates", _i, [_vp, _u64, _vp, _vp, _vp]),
    ("bsdb_kv_find_duplicates", _i, [_vp, C.c_char_p, _i, _i, _u32, _i, _u64, _vp, _vp, _vp]),
    ("bsdb_db_open", _i, [_vp, C.c_char_p, _i, _i, _u32, _i, C.c_char_p, C.POINTER(_vp)]),
    ("bsdb_db_info", _i, [_vp, _vp]),
    ("bsdb_db_set_batch", _i, [_vp, _u64]),
    ("bsdb_db_get_fixed", _i, [_vp, _vp, _u32, _u64, _u64, _vp, _vp, _vp, _vp]),
    ("bsdb_db_get_var", _i, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp]),
    ("bsdb_db_free", _i, [_vp]),
    ("bsdb_dev_db_locate_fixed", _i, [_vp, _vp, _u32, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_db_locate_var", _i, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_db_gather", _i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    ("bsdb_text_max_records", _u64, [_u64]),
    ("bsdb_dev_text_split", _i, [_vp, _vp, _u64, _i, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_text_pack", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _i, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp,
                                C.POINTER(_u64), _vp, _vp, _vp]),
    ("bsdb_builder_add_dev_var", _i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    ("bsdb_text_set_chunk", _i, [_vp, _u64]),
    ("bsdb_text_build", _i, [_vp, C.POINTER(C.c_char_p), _i, _i, C.c_char_p, _i, _u32, _i, C.c_char_p, C.c_char_p, _vp,
                             C.POINTER(_vp)]),
    ("bsdb_text_image_max", _u64, [_u64, _i, _i, _u32]),
    ("bsdb_dev_text_pack_blocked", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _i, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _u64,
                                        _vp, C.POINTER(_u64), _vp, _vp, _vp]),
    ("bsdb_text_build_layout", _i, [_vp, C.POINTER(C.c_char_p), _i, _i, C.c_char_p, _i, _i, _u32, _u32, _i, C.c_char_p,
                                    C.c_char_p, _vp, C.POINTER(_vp)]),
    ("bsdb_dev_db_check", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    ("bsdb_db_check_text", _i, [_vp, C.POINTER(C.c_char_p), _i, _i, _vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(_u64)]),
    ("bsdb_dev_db_records", _i, [_vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_db_dump_lengths", _i, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_db_dump_text", _i, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _u64, _vp, _u64, _vp, _vp]),
    ("bsdb_db_set_text_chunk", _i, [_vp, _u64]),
    ("bsdb_db_scan", _i, [_vp, _u64, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_db_dump_text", _i, [_vp, C.c_char_p, _i, _u64, _u64, _i, _vp]),
    ("bsdb_dev_db_diff", _i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    ("bsdb_dev_db_select", _i, [_vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_db_diff", _i, [_vp, _vp, _i, C.c_char_p, C.c_char_p, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_db_merge_status", _i, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("bsdb_dev_db_pack", _i, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _i, _i, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp,
                              C.POINTER(_u64), _vp, _vp, _vp]),
    ("bsdb_db_merge", _i, [_vp, _vp, _vp, C.c_char_p, _i, _i, _u32, _u32, _i, C.c_char_p, C.c_char_p, _vp, C.POINTER(_vp)]),
]

TEXT_WORDS = 10
# the text report's words in the header's order (uint64_t[BSDB_TEXT_WORDS])
TEXT_FIELDS = ("lines", "records", "not_two_fields", "empty_key", "too_large", "key_bytes", "value_bytes", "max_key_len",
               "max_value_len", "chunks")
TEXT_MAX_KEY, TEXT_MAX_VALUE = 255, 32510  # Common.MAX_KEY_SIZE, Common.MAX_VALUE_SIZE

BSDB_E2BIG = -7
GET_WORDS = 6
# the get report's words in the header's order (uint64_t[BSDB_GET_WORDS])
GET_FIELDS = ("queries", "found", "rejected", "key_mismatch", "bad_addr", "value_bytes")
GET_FOUND, GET_REJECTED, GET_KEY_MISMATCH, GET_BAD_ADDR = 0, 1, 2, 3  # a query's status byte
DB_INFO_WORDS = 8
DB_INFO_FIELDS = ("n", "partitions", "format", "block_size", "approximate", "image_bytes", "index_bytes", "batch")

CHECK_WORDS = 8
# the check report's words in the header's order (uint64_t[BSDB_CHECK_WORDS])
CHECK_FIELDS = ("records", "ok", "rejected", "key_mismatch", "bad_addr", "value_len", "value_bytes", "first_bad")
CHECK_OK, CHECK_VALUE_LEN, CHECK_VALUE_BYTES = 0, 4, 5  # a record's status byte; 1 .. 3 are the get's
CHECK_NONE = (1 << 64) - 1  # first_bad when every record is OK
CHECK_STATUS_NAMES = CHECK_FIELDS[1:7]  # a status byte's name is its counter's

SCAN_WORDS = 8
# the scan report's words in the header's order (uint64_t[BSDB_SCAN_WORDS])
SCAN_FIELDS = ("slots", "ok", "bad_addr", "not_text", "key_bytes", "value_bytes", "text_bytes", "first_bad")
SCAN_OK, SCAN_BAD_ADDR, SCAN_NOT_TEXT = 0, 1, 2  # a slot's status byte
SCAN_NONE = (1 << 64) - 1  # first_bad when every slot is OK
DUMP_MAX_LINE = 255 + 65535 + 2  # the smallest text-chunk cap: the longest line

DIFF_WORDS = 10
# the diff report's words in the header's order (uint64_t[BSDB_DIFF_WORDS])
DIFF_FIELDS = ("slots", "same", "rejected", "key_mismatch", "bad_addr", "value_len", "value_bytes", "bad_slot", "first_diff",
               "compared_bytes")
DIFF_SAME, DIFF_BAD_SLOT = 0, 6  # a slot's status byte; 1 .. 3 are the get's, 4 and 5 the check's
DIFF_NONE = (1 << 64) - 1  # first_diff when every slot is SAME
DIFF_STATUS_NAMES = DIFF_FIELDS[1:8]  # a status byte's name is its counter's
DIFF_MASK_ABSENT = 1 << GET_REJECTED | 1 << GET_KEY_MISMATCH  # bsdb_db_diff's removed file
DIFF_MASK_UPSERT = DIFF_MASK_ABSENT | 1 << CHECK_VALUE_LEN | 1 << CHECK_VALUE_BYTES  # its upsert file

MERGE_WORDS = 12
# the merge report's words in the header's order (uint64_t[BSDB_MERGE_WORDS])
MERGE_FIELDS = ("base_slots", "kept", "replaced", "removed", "bad_slot", "bad_addr", "delta_slots", "delta_written",
                "delta_bad_slot", "out_records", "out_key_bytes", "out_value_bytes")
MERGE_KEPT, MERGE_REPLACED, MERGE_REMOVED, MERGE_BAD_SLOT, MERGE_BAD_ADDR = range(5)  # a slot of base after the merge
MERGE_MAX_RECORD = 3 + TEXT_MAX_KEY + TEXT_MAX_VALUE  # the longest record a pack writes

BSDB_EVERIFY = -74
VERIFY_WORDS = 8
# the report's words in the header's order (out[BSDB_VERIFY_WORDS])
VERIFY_FIELDS = ("records", "rejected", "in_window", "wrong_addr", "wrong_value", "min_bad_addr", "flags", "windows")
VERIFY_E_INVALID, VERIFY_INDEX_SIZE, VERIFY_RECORD_COUNT = 1, 2, 4  # bits of "flags"

BSDB_EDUP = -17
DUP_WORDS = 4
# the report's words in the header's order (uint64_t[BSDB_DUP_WORDS])
DUP_FIELDS = ("found", "collisions", "flags", "keys")
DUP_LIST_FULL, DUP_PARTIAL = 1, 2  # bits of "flags"
DUP_SAME_KEY, DUP_COLLISION, DUP_UNCOMPARED = 0, 1, 2  # a pair's kind
DUP_DEFAULT_CAP = 1 << 16

HIST_AUTO, HIST_PARTITIONED, HIST_ATOMIC = 0, 1, 2


class BsdbError(RuntimeError):
    def __init__(self, fn: str, code: int):
        super().__init__(f"{fn} failed: {code} ({ERRORS.get(code, '?')})")
        self.code = code


class DuplicateKeyError(BsdbError):
    """A build that ended with BSDB_EDUP, with what the duplicate finder found:
    ``report`` is the finder's dict (``pairs``, ``kinds``, ``found``, ...),
    ``keys`` the first <= 16 duplicate keys as bytes.  ``code`` stays -17, so
    code that catches BsdbError and checks it keeps working."""

    def __init__(self, fn: str, report: dict, keys=()):
        super().__init__(fn, BSDB_EDUP)
        self.report = report
        self.keys = list(keys)
        shown = ", ".join(repr(k) for k in self.keys[:4])
        self.args = (f"{self.args[0]}: {report['found']} duplicate pair(s)"
                     + (f", {report['collisions']} of them signature collisions" if report.get("collisions") else "")
                     + (f"; keys {shown}" + (" ..." if len(self.keys) > 4 else "") if self.keys else ""),)


def _dup_report(pairs, kinds, report) -> dict:
    """The finder's result as a dict: the listed pairs sorted (rows by anchor,
    then other), their kinds in the same order, and the report's words."""
    import numpy as np
    found, collisions, flags, keys = (int(x) for x in report)
    k = min(found, pairs.shape[0])
    pairs = np.asarray(pairs[:k], np.uint64).reshape(k, 2)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    rep = {"pairs": pairs[order], "kinds": np.asarray(kinds[:k], np.uint8)[order] if kinds is not None else None,
           "found": found, "collisions": collisions, "list_full": bool(flags & DUP_LIST_FULL),
           "partial": bool(flags & DUP_PARTIAL), "keys": keys}
    return rep


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Loads the gfx950 library; raises if it was not built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C bsdb_amd/csrc` (hipcc --offload-arch=gfx950)")
        # torch's bundled HIP runtime shares the soname libamdhip64.so.7: import
        # torch first so this library binds to the same runtime instance.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(fn: str, rc: int):
    if rc != BSDB_OK:
        raise BsdbError(fn, rc)


def _verify_report(fn: str, rc: int, out) -> dict:
    """The report of a verify call as a dict (VERIFY_FIELDS + ``ok``): BSDB_OK
    and BSDB_EVERIFY both return it, every other code raises."""
    if rc not in (BSDB_OK, BSDB_EVERIFY):
        raise BsdbError(fn, rc)
    rep = {k: int(v) for k, v in zip(VERIFY_FIELDS, out)}
    rep["ok"] = rc == BSDB_OK
    return rep


def num_buckets(n: int) -> int:
    return int(lib().bsdb_num_buckets(n))


def mph_sizes(n: int, width: int) -> dict:
    """bsdb_mph_sizes: the field sizes of an MPHF on n keys (no device needed)."""
    m, vw, vb, sw = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check("bsdb_mph_sizes", lib().bsdb_mph_sizes(n, width, C.byref(m), C.byref(vw), C.byref(vb), C.byref(sw)))
    return {"num_buckets": m.value, "values_words": vw.value, "value_bits": vb.value, "sig_words": sw.value}


def text_max_records(nbytes: int) -> int:
    """bsdb_text_max_records: the most records `nbytes` of text can hold (host only)."""
    return int(lib().bsdb_text_max_records(nbytes))


def range_windows(n_global: int, width: int, e_lo: int, n_local: int):
    """bsdb_gov_range_windows: (values_w0, values_words, sig_w0, sig_words), the
    words the keys [e_lo, e_lo + n_local) of a range build write (host only)."""
    out = (C.c_uint64 * 4)()
    _check("bsdb_gov_range_windows", lib().bsdb_gov_range_windows(n_global, width, e_lo, n_local, out))
    return tuple(int(x) for x in out)


def _ptr(t) -> int:
    return t.data_ptr()


def _stream(stream) -> Optional[int]:
    import torch
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def text_image_max(nbytes: int, partitions: int = 1, fmt: int = 0, block_size: int = 4096) -> int:
    """bsdb_text_image_max: an upper bound of the image of `nbytes` of text (host only)."""
    return int(lib().bsdb_text_image_max(nbytes, partitions, fmt, block_size))


class Context:
    """One ``bsdb_ctx`` on one HIP device.  All ``*_dev`` methods take torch
    tensors resident on that device and enqueue on the current torch stream."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _check("bsdb_open", lib().bsdb_open(device, C.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            _check("bsdb_close", lib().bsdb_close(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- configuration
    def set_histogram_mode(self, mode: int):
        _check("bsdb_set_histogram_mode", lib().bsdb_set_histogram_mode(self._h, mode))

    def set_frontend(self, frontend: int):
        _check("bsdb_set_frontend", lib().bsdb_set_frontend(self._h, frontend))

    def set_pipeline(self, mode: int, chunks: int = 0, p2_cus: int = 0):
        """Pass 2 of chunk i beside pass 1 of chunk i + 1 (13-byte keys): -1 default, 0 off, 1 on."""
        _check("bsdb_set_pipeline", lib().bsdb_set_pipeline(self._h, mode, chunks, p2_cus))

    def set_chunk_keys(self, n: int):
        _check("bsdb_set_chunk_keys", lib().bsdb_set_chunk_keys(self._h, n))

    def fallback_count(self) -> int:
        """Chunks recounted by the overflow fallback since open (synchronises)."""
        v = C.c_uint64()
        _check("bsdb_fallback_count", lib().bsdb_fallback_count(self._h, C.byref(v)))
        return v.value

    def fused_status(self):
        """(single-pass launches since open, launches that timed out) -- synchronises."""
        a, b = C.c_uint64(), C.c_uint64()
        _check("bsdb_fused_status", lib().bsdb_fused_status(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- live per-kernel timing (HIP events on the launch stream)
    PASS1, PASS2, SCAN, CHECK_VALUES, DUMP_TEXT, DIFF_VALUES, REC_PACK = 0, 1, 2, 3, 4, 5, 6

    def set_profiling(self, on: bool):
        _check("bsdb_set_profiling", lib().bsdb_set_profiling(self._h, 1 if on else 0))

    def profile_read(self, kind: int):
        t, nl, nk = C.c_double(), C.c_uint64(), C.c_uint64()
        _check("bsdb_profile_read", lib().bsdb_profile_read(self._h, kind, C.byref(t), C.byref(nl), C.byref(nk)))
        return t.value, nl.value, nk.value

    # ---- A3: signatures
    def hash_fixed(self, keys, key_len: int, seed: int = 0, out=None, stream=None):
        import torch
        n = keys.numel() // key_len if key_len else 0
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int64, device=keys.device)
        _check("bsdb_dev_hash_fixed", lib().bsdb_dev_hash_fixed(
            self._h, _ptr(keys), key_len, n, seed & (2**64 - 1), _ptr(out), _stream(stream)))
        return out

    def hash_var(self, blob, offsets, seed: int = 0, out=None, stream=None):
        import torch
        n = offsets.numel() - 1
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int64, device=offsets.device)
        _check("bsdb_dev_hash_var", lib().bsdb_dev_hash_var(
            self._h, _ptr(blob), blob.numel(), _ptr(offsets), n, seed & (2**64 - 1), _ptr(out), _stream(stream)))
        return out

    # ---- A3+A4+A6: bucket-occupancy histogram (accumulating)
    def histogram_fixed(self, keys, key_len: int, m: int, counts=None, seed: int = 0, n: Optional[int] = None,
                        stream=None):
        import torch
        if n is None:
            n = keys.numel() // key_len
        if counts is None:
            counts = torch.zeros(m, dtype=torch.int32, device=keys.device)
        _check("bsdb_dev_histogram_fixed", lib().bsdb_dev_histogram_fixed(
            self._h, _ptr(keys), key_len, n, seed & (2**64 - 1), m, _ptr(counts), _stream(stream)))
        return counts

    def histogram_var(self, blob, offsets, m: int, counts=None, seed: int = 0, stream=None):
        import torch
        if counts is None:
            counts = torch.zeros(m, dtype=torch.int32, device=offsets.device)
        _check("bsdb_dev_histogram_var", lib().bsdb_dev_histogram_var(
            self._h, _ptr(blob), blob.numel(), _ptr(offsets), offsets.numel() - 1, seed & (2**64 - 1), m,
            _ptr(counts), _stream(stream)))
        return counts

    def edge_offsets(self, counts, out=None, stream=None):
        import torch
        m = counts.numel()
        if out is None:
            out = torch.empty(m + 1, dtype=torch.int64, device=counts.device)
        _check("bsdb_dev_edge_offsets", lib().bsdb_dev_edge_offsets(
            self._h, _ptr(counts), m, _ptr(out), _stream(stream)))
        return out

    # ---- A5/A6/A8/A11: GOV build on the device
    @staticmethod
    def _gov_outputs(sig, width: int, E, values, sigbits):
        """The build's output tensors: the caller's, or fresh ones of the
        sizes bsdb_dev_gov_build documents (sigbits None when width = 0)."""
        import torch
        n = sig.shape[0]

        def out(t, words):
            if t is None:
                return torch.empty(words, dtype=torch.int64, device=sig.device)
            if t.dtype != torch.int64 or t.numel() < words or not t.is_contiguous():
                raise ValueError("an output must be a contiguous int64 tensor of at least the documented size")
            return t
        return (out(E, num_buckets(n) + 1), out(values, int(lib().bsdb_values_words(n))),
                out(sigbits, (n * width + 63) // 64 + 1) if width else None)

    def gov_build(self, sig, width: int, stream=None, E=None, values=None, sigbits=None):
        n = sig.shape[0]
        E, values, sigbits = self._gov_outputs(sig, width, E, values, sigbits)
        _check("bsdb_dev_gov_build", lib().bsdb_dev_gov_build(
            self._h, _ptr(sig), n, width, _ptr(E), _ptr(values), _ptr(sigbits) if sigbits is not None else None,
            _stream(stream)))
        return E, values, sigbits

    def gov_build_ranks(self, sig, width: int, stream=None, E=None, values=None, sigbits=None, rank=None):
        """F2: (E, values, sigbits, rank) -- rank[i] = getLong of sig[i], from the solve."""
        import torch
        n = sig.shape[0]
        E, values, sigbits = self._gov_outputs(sig, width, E, values, sigbits)
        if rank is None:
            rank = torch.empty(max(n, 1), dtype=torch.int64, device=sig.device)[:n]
        elif rank.dtype != torch.int64 or rank.numel() < n:
            raise ValueError("rank holds fewer than n int64")
        _check("bsdb_dev_gov_build_ranks", lib().bsdb_dev_gov_build_ranks(
            self._h, _ptr(sig), n, width, _ptr(E), _ptr(values), _ptr(sigbits) if sigbits is not None else None,
            _ptr(rank), _stream(stream)))
        return E, values, sigbits, rank

    def gov_build_range(self, sig, n_global: int, b_lo: int, b_hi: int, e_lo: int, width: int, E, values, sigbits=None,
                        rank=None, stream=None):
        """E4: one rank's bucket range [b_lo, b_hi) into FULL-size zeroed arrays
        (rank: optional, the global rank of each local signature)."""
        _check("bsdb_dev_gov_build_range", lib().bsdb_dev_gov_build_range(
            self._h, _ptr(sig), sig.shape[0], n_global, b_lo, b_hi, e_lo, width, _ptr(E), _ptr(values),
            _ptr(sigbits) if sigbits is not None else None, _ptr(rank) if rank is not None else None, _stream(stream)))

    def gov_build_window(self, sig, n_global: int, b_lo: int, b_hi: int, e_lo: int, width: int, E_win, values_win,
                         values_w0: int, sigbits_win=None, sig_w0: int = 0, rank=None, stream=None):
        """E4 with O(n/G) memory: the range build into zeroed windows of the
        structure (E[b_lo..b_hi], value words from values_w0, checksum words
        from sig_w0; range_windows gives the words the range writes)."""
        assert E_win.numel() >= b_hi - b_lo + 1
        _check("bsdb_dev_gov_build_window", lib().bsdb_dev_gov_build_window(
            self._h, _ptr(sig), sig.shape[0], n_global, b_lo, b_hi, e_lo, width, _ptr(E_win), _ptr(values_win),
            values_w0, values_win.numel(), _ptr(sigbits_win) if sigbits_win is not None else None, sig_w0,
            sigbits_win.numel() if sigbits_win is not None else 0, _ptr(rank) if rank is not None else None,
            _stream(stream)))

    def mph_build_index_passes(self, keys, key_len: int, n: int, width: int, passes: int = 0, offsets=None,
                               addr=None, addr_base: int = 0, addr_stride: int = 0, index=None, stream=None):
        """The whole build from keys resident on the device by sequential
        bucket-range passes (fixed key_len, or a var-len blob with offsets).
        index: None (structure only), a device int64 tensor of n slots, or a
        host numpy uint64/int64 array of n slots (each pass's slice copied out
        while the next solves).  addr: device int64 tensor of n addresses, else
        addr_base + addr_stride * i.  Returns (E, values, sigbits, passes_used)."""
        import torch
        import numpy as np
        dev = keys.device
        m = num_buckets(n)
        E = torch.empty(m + 1, dtype=torch.int64, device=dev)
        values = torch.empty(int(lib().bsdb_values_words(n)), dtype=torch.int64, device=dev)
        sigbits = torch.empty((n * width + 63) // 64 + 1, dtype=torch.int64, device=dev) if width else None
        d_index = h_index = None
        if index is not None:
            if isinstance(index, np.ndarray):
                assert index.dtype.itemsize == 8 and index.size >= n and index.flags.c_contiguous
                h_index = index.ctypes.data
            else:
                assert index.dtype == torch.int64 and index.numel() >= n and index.device == dev
                d_index = _ptr(index)
        used = C.c_uint32()
        sb = _ptr(sigbits) if sigbits is not None else None
        ad = _ptr(addr) if addr is not None else None
        if offsets is None:
            _check("bsdb_dev_mph_build_index_passes_fixed", lib().bsdb_dev_mph_build_index_passes_fixed(
                self._h, _ptr(keys), key_len, n, width, passes, ad, addr_base, addr_stride, _ptr(E), _ptr(values), sb,
                d_index, h_index, C.byref(used), _stream(stream)))
        else:
            _check("bsdb_dev_mph_build_index_passes_var", lib().bsdb_dev_mph_build_index_passes_var(
                self._h, _ptr(keys), keys.numel(), _ptr(offsets), n, width, passes, ad, addr_base, addr_stride,
                _ptr(E), _ptr(values), sb, d_index, h_index, C.byref(used), _stream(stream)))
        return E, values, sigbits, used.value

    def partition_owners(self, sig, m: int, nranks: int, payload=None, stream=None, out=None, payload_out=None):
        """Signatures (and one int64 payload per key) grouped by owning rank
        (bucket ranges); returns (sig_out, payload_out or None, counts)."""
        import torch
        import numpy as np
        n = sig.shape[0]
        if out is None:
            out = torch.empty((max(n, 1), 2), dtype=torch.int64, device=sig.device)[:n]
        elif out.dtype != torch.int64 or out.numel() < 2 * n:
            raise ValueError("out holds fewer than 2n int64")
        pout = payload_out
        if payload is None:
            pout = None
        elif pout is None:
            pout = torch.empty(max(n, 1), dtype=torch.int64, device=sig.device)[:n]
        elif pout.dtype != torch.int64 or pout.numel() < n:
            raise ValueError("payload_out holds fewer than n int64")
        counts = np.zeros(nranks, np.uint64)
        _check("bsdb_dev_partition_owners", lib().bsdb_dev_partition_owners(
            self._h, _ptr(sig), _ptr(payload) if payload is not None else None, n, m, nranks, _ptr(out),
            _ptr(pout) if pout is not None else None, counts.ctypes.data, _stream(stream)))
        return out, pout, [int(x) for x in counts]

    def release_workspace(self):
        _check("bsdb_release_workspace", lib().bsdb_release_workspace(self._h))

    def set_verify(self, on: bool):
        _check("bsdb_set_verify", lib().bsdb_set_verify(self._h, 1 if on else 0))

    # ---- B4: the histogram collective (RCCL) inside the library
    @staticmethod
    def comm_available() -> bool:
        return bool(lib().bsdb_comm_available())

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check("bsdb_comm_unique_id", lib().bsdb_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes):
        buf = C.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        _check("bsdb_comm_init", lib().bsdb_comm_init(self._h, nranks, rank, buf))

    def histogram_finalize(self, counts, n_total: int, out=None, stream=None):
        """All-reduce of the local counts over RCCL + scan -> E (every rank)."""
        import torch
        m = counts.numel()
        if out is None:
            out = torch.empty(m + 1, dtype=torch.int64, device=counts.device)
        _check("bsdb_dev_histogram_finalize", lib().bsdb_dev_histogram_finalize(
            self._h, _ptr(counts), m, n_total, _ptr(out), _stream(stream)))
        return out

    def allreduce_u64(self, buf, stream=None):
        _check("bsdb_dev_allreduce_u64", lib().bsdb_dev_allreduce_u64(self._h, _ptr(buf), buf.numel(), _stream(stream)))

    # ---- A14/A15/F4: a device-resident MPHF built from host keys
    def mph_build_fixed(self, keys_np, key_len: int, width: int) -> "Mph":
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        h = C.c_void_p()
        _check("bsdb_mph_build_fixed", lib().bsdb_mph_build_fixed(
            self._h, keys_np.ctypes.data, key_len, keys_np.size // key_len, width, C.byref(h)))
        return Mph(h, self)

    @staticmethod
    def _records_args(n, addr_np, value8_np, vlen_np, approximate):
        import numpy as np
        addr_np = np.ascontiguousarray(addr_np, np.uint64)
        if addr_np.size != n:
            raise ValueError("one address per key")
        v8 = vl = None
        if approximate:
            if value8_np is None or vlen_np is None:
                raise ValueError("approximate mode needs value8 and vlen")
            v8 = np.ascontiguousarray(value8_np, np.uint64)
            vl = np.ascontiguousarray(vlen_np, np.uint8)
            if v8.size != n or vl.size != n:
                raise ValueError("one value8/vlen per key")
        return addr_np, v8, vl

    def mph_build_index_fixed(self, keys_np, key_len: int, width: int, addr_np, index_path: str,
                              index_a_path: Optional[str] = None, approximate: bool = False, value8_np=None,
                              vlen_np=None) -> "Mph":
        """F2: MPHF + index.db (+ index_a.db) in one call from the solve's
        ranks (bsdb_mph_build_index_fixed), no rescan of the records."""
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        n = keys_np.size // key_len
        addr_np, v8, vl = self._records_args(n, addr_np, value8_np, vlen_np, approximate)
        h = C.c_void_p()
        _check("bsdb_mph_build_index_fixed", lib().bsdb_mph_build_index_fixed(
            self._h, keys_np.ctypes.data, key_len, n, width, addr_np.ctypes.data,
            v8.ctypes.data if v8 is not None else None, vl.ctypes.data if vl is not None else None,
            1 if approximate else 0, index_path.encode(), index_a_path.encode() if index_a_path else None,
            C.byref(h)))
        return Mph(h, self)

    def mph_build_index_passes_host(self, keys_np, key_len: int, width: int, index_path: str,
                                    index_a_path: Optional[str] = None, addr_np=None, addr_base: int = 0,
                                    addr_stride: int = 0, approximate: bool = False, value8_np=None, vlen_np=None,
                                    passes: int = 0, offsets_np=None):
        """F2 in bounded device memory from host records
        (bsdb_mph_build_index_passes_{fixed,var}): keys uploaded once, built by
        bucket-range passes, each pass's slots written at their file offset.
        key_len 0 with offsets_np: variable-length keys.  addr_np None:
        addresses addr_base + addr_stride * i.  Returns (Mph, passes_used)."""
        import numpy as np
        if offsets_np is not None:
            blob, off, n = self._var_host_args(keys_np, offsets_np)
        else:
            blob = np.ascontiguousarray(keys_np, np.uint8)
            n = blob.size // key_len
        if addr_np is not None:
            a, v8, vl = self._records_args(n, addr_np, value8_np, vlen_np, approximate)
        else:
            a = None
            _, v8, vl = self._records_args(n, np.zeros(n, np.uint64), value8_np, vlen_np, approximate)
        h = C.c_void_p()
        used = C.c_uint32()
        ip, ap = index_path.encode(), index_a_path.encode() if index_a_path else None
        if offsets_np is not None:
            _check("bsdb_mph_build_index_passes_var", lib().bsdb_mph_build_index_passes_var(
                self._h, blob.ctypes.data, off.ctypes.data, n, width, _np_ptr(a), addr_base, addr_stride, _np_ptr(v8),
                _np_ptr(vl), 1 if approximate else 0, passes, ip, ap, C.byref(h), C.byref(used)))
        else:
            _check("bsdb_mph_build_index_passes_fixed", lib().bsdb_mph_build_index_passes_fixed(
                self._h, blob.ctypes.data, key_len, n, width, _np_ptr(a), addr_base, addr_stride, _np_ptr(v8),
                _np_ptr(vl), 1 if approximate else 0, passes, ip, ap, C.byref(h), C.byref(used)))
        return Mph(h, self), used.value

    def builder(self, key_len: int = 0, key_capacity: int = 0, blob_capacity: int = 0, approximate: bool = False,
                addr_base: int = 0, addr_stride: int = 0) -> "Builder":
        """A streaming builder (bsdb_builder_*): keys added in batches into
        HBM, then one bucket-range-pass build into the index files."""
        return Builder(self, key_len, key_capacity, blob_capacity, approximate, addr_base, addr_stride)

    def kv_build_index(self, kv_base: str, partitions: int, width: int, index_path: str,
                       index_a_path: Optional[str] = None, approximate: bool = False, fmt: int = 0,
                       block_size: int = 4096, threads: int = 0) -> "Mph":
        """W:91-155 from the data files: native kv.db scan + the one-call build."""
        h = C.c_void_p()
        _check("bsdb_kv_build_index", lib().bsdb_kv_build_index(
            self._h, kv_base.encode(), partitions, fmt, block_size, threads, width, 1 if approximate else 0,
            index_path.encode(), index_a_path.encode() if index_a_path else None, C.byref(h)))
        return Mph(h, self)

    def mph_build_index_var(self, blob_np, off_np, width: int, addr_np, index_path: str,
                            index_a_path: Optional[str] = None, approximate: bool = False, value8_np=None,
                            vlen_np=None) -> "Mph":
        blob_np, off_np, n = self._var_host_args(blob_np, off_np)
        addr_np, v8, vl = self._records_args(n, addr_np, value8_np, vlen_np, approximate)
        h = C.c_void_p()
        _check("bsdb_mph_build_index_var", lib().bsdb_mph_build_index_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, width, addr_np.ctypes.data,
            v8.ctypes.data if v8 is not None else None, vl.ctypes.data if vl is not None else None,
            1 if approximate else 0, index_path.encode(), index_a_path.encode() if index_a_path else None,
            C.byref(h)))
        return Mph(h, self)

    def mph_build_var(self, blob_np, off_np, width: int) -> "Mph":
        blob_np, off_np, n = self._var_host_args(blob_np, off_np)
        h = C.c_void_p()
        _check("bsdb_mph_build_var", lib().bsdb_mph_build_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, width, C.byref(h)))
        return Mph(h, self)

    def mph_import(self, n: int, width: int, E, values, sigbits=None) -> "Mph":
        import numpy as np
        E = np.ascontiguousarray(E, np.uint64)
        values = np.ascontiguousarray(values, np.uint64)
        sb = np.ascontiguousarray(sigbits, np.uint64) if sigbits is not None else None
        h = C.c_void_p()
        _check("bsdb_mph_import", lib().bsdb_mph_import(
            self._h, n, width, E.ctypes.data, values.ctypes.data, sb.ctypes.data if sb is not None else None,
            C.byref(h)))
        return Mph(h, self)

    def mph_load(self, path: str) -> "Mph":
        h = C.c_void_p()
        _check("bsdb_mph_load", lib().bsdb_mph_load(self._h, path.encode(), C.byref(h)))
        return Mph(h, self)

    # ---- A11-A13: MPHF evaluation over (E, values[, checksum bits])
    def lookup(self, sig, n: int, E, values, width: int = 0, sigbits=None, check: bool = True, out=None,
               stream=None):
        import torch
        nq = sig.shape[0]
        if out is None:
            out = torch.empty(nq, dtype=torch.int64, device=sig.device)
        _check("bsdb_dev_lookup", lib().bsdb_dev_lookup(
            self._h, _ptr(sig), nq, n, E.numel() - 1, _ptr(E), _ptr(values), width,
            _ptr(sigbits) if sigbits is not None else None, 1 if check else 0, _ptr(out), _stream(stream)))
        return out

    def sign(self, sig, E, values, width: int, out=None, stream=None):
        import torch
        n = sig.shape[0]
        if out is None:
            out = torch.zeros((n * width + 63) // 64 + 1, dtype=torch.int64, device=sig.device)
        _check("bsdb_dev_sign", lib().bsdb_dev_sign(
            self._h, _ptr(sig), n, E.numel() - 1, _ptr(E), _ptr(values), width, _ptr(out), _stream(stream)))
        return out

    def index_scatter(self, rank, addr, start: int, length: int, index, value8=None, value_len=None, index_a=None,
                      stream=None):
        _check("bsdb_dev_index_scatter", lib().bsdb_dev_index_scatter(
            self._h, _ptr(rank), _ptr(addr), rank.numel(), start, length, _ptr(index),
            _ptr(value8) if value8 is not None else None, _ptr(value_len) if value_len is not None else None,
            _ptr(index_a) if index_a is not None else None, _stream(stream)))

    # ---- F4: the fused database check on device-resident records
    @staticmethod
    def verify_out(device):
        """A zeroed report for verify_fixed / verify_var ([5] = all ones)."""
        import torch
        out = torch.zeros(VERIFY_WORDS, dtype=torch.int64, device=device)
        out[5] = -1
        return out

    def _verify_args(self, n, E, values, width, sigbits, start, length, index, index_a, out, stream):
        return (n, E.numel() - 1, _ptr(E), _ptr(values), width, _ptr(sigbits) if sigbits is not None else None,
                start, length, _ptr(index), _ptr(index_a) if index_a is not None else None, _ptr(out), _stream(stream))

    @staticmethod
    def _verify_counters(out):
        return tuple(int(x) & (2**64 - 1) for x in out[:6].cpu().tolist())

    def verify_fixed(self, keys, key_len: int, n: int, E, values, index, start: int = 0, length: Optional[int] = None,
                     width: int = 0, sigbits=None, addr=None, addr_base: int = 0, addr_stride: int = 0, first: int = 0,
                     value8=None, vlen=None, index_a=None, out=None, stream=None):
        """bsdb_dev_verify_fixed: keys.numel() // key_len records against the
        slots of ranks [start, start + length) in `index` (and `index_a`).
        Accumulates into `out` (verify_out()); returns the six counters
        (records, rejected, in_window, wrong_addr, wrong_value, min_bad_addr)."""
        count = keys.numel() // key_len
        if length is None:
            length = index.numel()
        if out is None:
            out = self.verify_out(keys.device)
        _check("bsdb_dev_verify_fixed", lib().bsdb_dev_verify_fixed(
            self._h, _ptr(keys), key_len, count, _ptr(addr) if addr is not None else None, addr_base, addr_stride,
            first, _ptr(value8) if value8 is not None else None, _ptr(vlen) if vlen is not None else None,
            *self._verify_args(n, E, values, width, sigbits, start, length, index, index_a, out, stream)))
        return self._verify_counters(out)

    def verify_var(self, blob, offsets, n: int, E, values, index, start: int = 0, length: Optional[int] = None,
                   width: int = 0, sigbits=None, addr=None, addr_base: int = 0, addr_stride: int = 0, first: int = 0,
                   value8=None, vlen=None, index_a=None, out=None, stream=None):
        """bsdb_dev_verify_var: as verify_fixed for a key blob with offsets."""
        count = offsets.numel() - 1
        if length is None:
            length = index.numel()
        if out is None:
            out = self.verify_out(offsets.device)
        _check("bsdb_dev_verify_var", lib().bsdb_dev_verify_var(
            self._h, _ptr(blob), blob.numel(), _ptr(offsets), count, _ptr(addr) if addr is not None else None,
            addr_base, addr_stride, first, _ptr(value8) if value8 is not None else None,
            _ptr(vlen) if vlen is not None else None,
            *self._verify_args(n, E, values, width, sigbits, start, length, index, index_a, out, stream)))
        return self._verify_counters(out)

    # ---- which keys are duplicates (the query behind BSDB_EDUP)
    @staticmethod
    def _dup_bufs(device, cap: int, kinds: bool = True, pairs=None, kd=None, report=None):
        """The finder's outputs: the caller's (pairs int64 [cap, 2], kinds uint8
        [cap], report int64 [DUP_WORDS]), or zeroed ones."""
        import torch
        if pairs is None:
            pairs = torch.zeros((max(cap, 1), 2), dtype=torch.int64, device=device)
        elif pairs.dtype != torch.int64 or pairs.numel() < 2 * cap:
            raise ValueError("pairs holds fewer than 2 * cap int64")
        if not kinds:
            kd = None
        elif kd is None:
            kd = torch.zeros(max(cap, 1), dtype=torch.uint8, device=device)
        elif kd.dtype != torch.uint8 or kd.numel() < cap:
            raise ValueError("kinds holds fewer than cap bytes")
        if report is None:
            report = torch.zeros(DUP_WORDS, dtype=torch.int64, device=device)
        elif report.dtype != torch.int64 or report.numel() < DUP_WORDS:
            raise ValueError("report holds fewer than DUP_WORDS int64")
        return pairs, kd, report

    @staticmethod
    def _dup_result(cap: int, pairs, kinds, report) -> dict:
        import numpy as np
        rep = [int(x) & (2**64 - 1) for x in report.cpu().tolist()]
        k = min(rep[0], cap)
        return _dup_report(pairs[:k].cpu().numpy().view(np.uint64), kinds[:k].cpu().numpy() if kinds is not None else None,
                           rep)

    def find_duplicates_fixed(self, keys, key_len: int, n: Optional[int] = None, passes: int = 0,
                              cap: int = DUP_DEFAULT_CAP, stream=None, pairs=None, kinds=None, report=None) -> dict:
        """bsdb_dev_find_duplicates_fixed over keys resident on the device:
        {"pairs": ndarray[k, 2] of input positions, sorted, "kinds", "found",
        "collisions", "list_full", "partial", "keys"}."""
        if n is None:
            n = keys.numel() // key_len
        pairs, kinds, report = self._dup_bufs(keys.device, cap, True, pairs, kinds, report)
        _check("bsdb_dev_find_duplicates_fixed", lib().bsdb_dev_find_duplicates_fixed(
            self._h, _ptr(keys), key_len, n, passes, cap, _ptr(pairs), _ptr(kinds), _ptr(report), _stream(stream)))
        return self._dup_result(cap, pairs, kinds, report)

    def find_duplicates_var(self, blob, offsets, passes: int = 0, cap: int = DUP_DEFAULT_CAP, stream=None,
                            pairs=None, kinds=None, report=None) -> dict:
        """bsdb_dev_find_duplicates_var: a key blob with int64 offsets[n + 1] on the device."""
        n = offsets.numel() - 1
        pairs, kinds, report = self._dup_bufs(offsets.device, cap, True, pairs, kinds, report)
        _check("bsdb_dev_find_duplicates_var", lib().bsdb_dev_find_duplicates_var(
            self._h, _ptr(blob), blob.numel(), _ptr(offsets), n, passes, cap, _ptr(pairs), _ptr(kinds), _ptr(report),
            _stream(stream)))
        return self._dup_result(cap, pairs, kinds, report)

    def find_duplicates_sig(self, sig, cap: int = DUP_DEFAULT_CAP, stream=None) -> dict:
        """bsdb_dev_find_duplicates_sig: (n, 2) int64 signatures on the device; positions, no kinds."""
        n = sig.shape[0]
        pairs, _, report = self._dup_bufs(sig.device, cap, kinds=False)
        _check("bsdb_dev_find_duplicates_sig", lib().bsdb_dev_find_duplicates_sig(
            self._h, _ptr(sig) if n else None, n, cap, _ptr(pairs), _ptr(report), _stream(stream)))
        return self._dup_result(cap, pairs, None, report)

    @staticmethod
    def _kinds_out(kinds, k: int, device):
        import torch
        if kinds is None:
            return torch.zeros(max(k, 1), dtype=torch.uint8, device=device)
        if kinds.dtype != torch.uint8 or kinds.numel() < k:
            raise ValueError("kinds holds fewer bytes than there are pairs")
        return kinds

    def classify_pairs_fixed(self, keys, key_len: int, pairs, n: Optional[int] = None, stream=None, kinds=None):
        """bsdb_dev_classify_pairs_fixed: the kind (0 same key, 1 collision) of
        each row of `pairs` (int64 [k, 2] positions, device); a uint8 tensor."""
        if n is None:
            n = keys.numel() // key_len
        k = pairs.shape[0]
        kinds = self._kinds_out(kinds, k, keys.device)
        _check("bsdb_dev_classify_pairs_fixed", lib().bsdb_dev_classify_pairs_fixed(
            self._h, _ptr(keys), key_len, n, _ptr(pairs), k, _ptr(kinds), _stream(stream)))
        return kinds[:k]

    def classify_pairs_var(self, blob, offsets, pairs, stream=None, kinds=None):
        """bsdb_dev_classify_pairs_var: as classify_pairs_fixed for a blob with offsets."""
        k = pairs.shape[0]
        kinds = self._kinds_out(kinds, k, offsets.device)
        _check("bsdb_dev_classify_pairs_var", lib().bsdb_dev_classify_pairs_var(
            self._h, _ptr(blob), blob.numel(), _ptr(offsets), offsets.numel() - 1, _ptr(pairs), k, _ptr(kinds),
            _stream(stream)))
        return kinds[:k]

    @staticmethod
    def _dup_host_bufs(cap: int):
        import numpy as np
        return np.zeros((max(cap, 1), 2), np.uint64), np.zeros(max(cap, 1), np.uint8), np.zeros(DUP_WORDS, np.uint64)

    def find_duplicates_fixed_host(self, keys_np, key_len: int, cap: int = DUP_DEFAULT_CAP) -> dict:
        """bsdb_find_duplicates_fixed: keys in host memory, streamed through a builder."""
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        pairs, kinds, report = self._dup_host_bufs(cap)
        _check("bsdb_find_duplicates_fixed", lib().bsdb_find_duplicates_fixed(
            self._h, keys_np.ctypes.data, key_len, keys_np.size // key_len, cap, pairs.ctypes.data, kinds.ctypes.data,
            report.ctypes.data))
        return _dup_report(pairs[:cap], kinds[:cap], report)

    def find_duplicates_var_host(self, blob_np, off_np, cap: int = DUP_DEFAULT_CAP) -> dict:
        """bsdb_find_duplicates_var: a key blob with offsets in host memory."""
        blob_np, off_np, n = self._var_host_args(blob_np, off_np)
        pairs, kinds, report = self._dup_host_bufs(cap)
        _check("bsdb_find_duplicates_var", lib().bsdb_find_duplicates_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, cap, pairs.ctypes.data, kinds.ctypes.data,
            report.ctypes.data))
        return _dup_report(pairs[:cap], kinds[:cap], report)

    def kv_find_duplicates(self, kv_base: str, partitions: int, fmt: int = 0, block_size: int = 4096, threads: int = 0,
                           cap: int = DUP_DEFAULT_CAP) -> dict:
        """bsdb_kv_find_duplicates: the duplicate records of kv.db files, as
        pairs of record addresses (kv_scan's "addr")."""
        pairs, kinds, report = self._dup_host_bufs(cap)
        _check("bsdb_kv_find_duplicates", lib().bsdb_kv_find_duplicates(
            self._h, kv_base.encode(), partitions, fmt, block_size, threads, cap, pairs.ctypes.data, kinds.ctypes.data,
            report.ctypes.data))
        return _dup_report(pairs[:cap], kinds[:cap], report)

    # ---- batched get on device-resident keys: locate -> edge_offsets(vlen) -> gather
    @staticmethod
    def _locate_outs(nq: int, device, src, vlen, status, report):
        import torch
        k = max(nq, 1)
        if src is None:
            src = torch.empty(k, dtype=torch.int64, device=device)
        if vlen is None:
            vlen = torch.empty(k, dtype=torch.int32, device=device)
        if status is None:
            status = torch.empty(k, dtype=torch.uint8, device=device)
        if report is None:
            report = torch.zeros(GET_WORDS, dtype=torch.int64, device=device)
        if (src.dtype != torch.int64 or vlen.dtype != torch.int32 or status.dtype != torch.uint8
                or report.dtype != torch.int64 or min(src.numel(), vlen.numel(), status.numel()) < nq
                or report.numel() < GET_WORDS):
            raise ValueError("src int64[nq], vlen int32[nq], status uint8[nq], report int64[GET_WORDS]")
        return src, vlen, status, report

    def db_locate_fixed(self, db: "Database", keys, key_len: int, nq: Optional[int] = None, src=None, vlen=None,
                        status=None, report=None, stream=None):
        """bsdb_dev_db_locate_fixed: (src, vlen, status, report) tensors of the
        nq keys; `report` (int64[GET_WORDS], zeroed by the caller) accumulates."""
        if nq is None:
            nq = keys.numel() // key_len
        src, vlen, status, report = self._locate_outs(nq, keys.device, src, vlen, status, report)
        _check("bsdb_dev_db_locate_fixed", lib().bsdb_dev_db_locate_fixed(
            db._h, _ptr(keys), key_len, nq, _ptr(src), _ptr(vlen), _ptr(status), _ptr(report), _stream(stream)))
        return src[:nq], vlen[:nq], status[:nq], report

    def db_locate_var(self, db: "Database", blob, offsets, src=None, vlen=None, status=None, report=None, stream=None):
        """bsdb_dev_db_locate_var: as db_locate_fixed for a key blob with int64 offsets[nq + 1]."""
        nq = offsets.numel() - 1
        src, vlen, status, report = self._locate_outs(nq, offsets.device, src, vlen, status, report)
        _check("bsdb_dev_db_locate_var", lib().bsdb_dev_db_locate_var(
            db._h, _ptr(blob), blob.numel(), _ptr(offsets), nq, _ptr(src), _ptr(vlen), _ptr(status), _ptr(report),
            _stream(stream)))
        return src[:nq], vlen[:nq], status[:nq], report

    def db_gather(self, db: "Database", src, voff, values=None, value_bytes: Optional[int] = None, stream=None):
        """bsdb_dev_db_gather: value i to values[voff[i]:voff[i + 1]]; voff =
        edge_offsets(vlen).  `values`: a uint8 tensor (any alignment) of at
        least value_bytes = voff[nq] bytes (read back when not given)."""
        import torch
        nq = src.numel()
        if value_bytes is None:
            value_bytes = int(voff[nq])
        if values is None:
            values = torch.empty(max(value_bytes, 1), dtype=torch.uint8, device=src.device)
        elif values.dtype != torch.uint8 or values.numel() < value_bytes or not values.is_contiguous():
            raise ValueError("values holds fewer than value_bytes contiguous bytes")
        _check("bsdb_dev_db_gather", lib().bsdb_dev_db_gather(
            db._h, _ptr(src), _ptr(voff), nq, _ptr(values), value_bytes, _stream(stream)))
        return values[:value_bytes]

    @staticmethod
    def check_report(device):
        """A fresh device report for db_check: int64[CHECK_WORDS], zero with first_bad = UINT64_MAX (-1)."""
        import torch
        report = torch.zeros(CHECK_WORDS, dtype=torch.int64, device=device)
        report[CHECK_WORDS - 1] = -1
        return report

    def db_check(self, db: "Database", text, vpos, vlen, src, dbvlen, status, nbytes: Optional[int] = None,
                 count: Optional[int] = None, record_base: int = 0, report=None, stream=None):
        """bsdb_dev_db_check: the text's values (descriptors vpos / vlen int32
        of text_split) against the database's (src int64, dbvlen int32, status
        uint8 of db_locate_var for the same records' keys).  `status` is
        rewritten in place to the check's; `report` (Context.check_report,
        made here when not given) accumulates.  Returns (status, report)."""
        import torch
        if nbytes is None:
            nbytes = text.numel()
        if count is None:
            count = status.numel()
        if report is None:
            report = self.check_report(text.device)
        if (vpos.dtype != torch.int32 or vlen.dtype != torch.int32 or src.dtype != torch.int64 or dbvlen.dtype != torch.int32
                or status.dtype != torch.uint8 or report.dtype != torch.int64 or report.numel() < CHECK_WORDS
                or min(vpos.numel(), vlen.numel(), src.numel(), dbvlen.numel(), status.numel()) < count):
            raise ValueError("vpos / vlen / dbvlen int32[count], src int64[count], status uint8[count], report int64[CHECK_WORDS]")
        _check("bsdb_dev_db_check", lib().bsdb_dev_db_check(
            db._h, _ptr(text), nbytes, _ptr(vpos), _ptr(vlen), _ptr(src), _ptr(dbvlen), _ptr(status), count, record_base,
            _ptr(report), _stream(stream)))
        return status[:count], report

    # ---- a resident database enumerated by slot: records -> lengths -> text
    @staticmethod
    def scan_report(device):
        """A fresh device report for db_records / db_dump_text: int64[SCAN_WORDS], zero with first_bad = UINT64_MAX (-1)."""
        import torch
        report = torch.zeros(SCAN_WORDS, dtype=torch.int64, device=device)
        report[SCAN_WORDS - 1] = -1
        return report

    def db_records(self, db: "Database", first: int = 0, count: Optional[int] = None, report=None, stream=None):
        """bsdb_dev_db_records: slots [first, first + count) of the resident
        database as (ksrc, klen, vsrc, vlen, status, report) tensors: the
        byte positions (int64) and lengths (int32) of every record's key and
        value in the image, a status byte, and the report
        (Context.scan_report, made here when not given; it accumulates).
        Packed keys: ``db_gather(db, ksrc, edge_offsets(klen))``; values alike."""
        import torch
        if count is None:
            count = db.info()["n"] - first
        dev = torch.device(f"cuda:{self.device}") if report is None else report.device
        if report is None:
            report = self.scan_report(dev)
        k = max(count, 1)
        ksrc, vsrc = (torch.empty(k, dtype=torch.int64, device=dev) for _ in range(2))
        klen, vlen = (torch.empty(k, dtype=torch.int32, device=dev) for _ in range(2))
        status = torch.empty(k, dtype=torch.uint8, device=dev)
        _check("bsdb_dev_db_records", lib().bsdb_dev_db_records(
            db._h, first, count, _ptr(ksrc), _ptr(klen), _ptr(vsrc), _ptr(vlen), _ptr(status), _ptr(report), _stream(stream)))
        return ksrc[:count], klen[:count], vsrc[:count], vlen[:count], status[:count], report

    def db_dump_lengths(self, db: "Database", klen, vlen, status, stream=None):
        """bsdb_dev_db_dump_lengths: (llen int32[count], loff int64[count + 1]):
        every record's line length and their exclusive scan; `status` gets
        the length part of NOT_TEXT in place."""
        import torch
        count = status.numel()
        llen = torch.empty(max(count, 1), dtype=torch.int32, device=status.device)
        loff = torch.empty(count + 1, dtype=torch.int64, device=status.device)
        if klen.dtype != torch.int32 or vlen.dtype != torch.int32 or status.dtype != torch.uint8 or min(klen.numel(), vlen.numel()) < count:
            raise ValueError("klen / vlen int32[count], status uint8[count]")
        _check("bsdb_dev_db_dump_lengths", lib().bsdb_dev_db_dump_lengths(
            db._h, count, _ptr(klen), _ptr(vlen), _ptr(status), _ptr(llen), _ptr(loff), _stream(stream)))
        return llen[:count], loff

    def db_dump_text(self, db: "Database", ksrc, klen, vsrc, vlen, status, separator=" ", first: int = 0, text=None, llen=None,
                     loff=None, text_bytes: Optional[int] = None, report=None, stream=None):
        """bsdb_dev_db_dump_text: the records' lines ``key<sep>value\n`` in
        slot order as a uint8 tensor, (text, status, report).  Without llen /
        loff it runs db_dump_lengths first and reads the text's length back
        (which synchronises, as does reading loff[count] when text_bytes is not
        given).  `text`: a uint8 tensor (any alignment) of at least
        loff[count] bytes; `status` (db_records') gets NOT_TEXT in
        place; `report` as for db_records, a fresh one when not given; `first`
        is the slot of record 0 (for the report's first_bad)."""
        import torch
        count = status.numel()
        if llen is None or loff is None:
            llen, loff = self.db_dump_lengths(db, klen, vlen, status, stream=stream)
        if text_bytes is None:
            text_bytes = int(loff[count])
        if text is None:
            text = torch.empty(max(text_bytes, 1), dtype=torch.uint8, device=status.device)
        elif text.dtype != torch.uint8 or text.numel() < text_bytes or not text.is_contiguous():
            raise ValueError("text holds fewer than loff[count] contiguous bytes")
        if report is None:
            report = self.scan_report(status.device)
        if (ksrc.dtype != torch.int64 or vsrc.dtype != torch.int64 or klen.dtype != torch.int32 or vlen.dtype != torch.int32
                or llen.dtype != torch.int32 or loff.dtype != torch.int64 or status.dtype != torch.uint8
                or report.dtype != torch.int64 or report.numel() < SCAN_WORDS or loff.numel() < count + 1
                or min(ksrc.numel(), vsrc.numel(), klen.numel(), vlen.numel(), llen.numel()) < count):
            raise ValueError("ksrc / vsrc int64[count], klen / vlen / llen int32[count], loff int64[count + 1], "
                             "status uint8[count], report int64[SCAN_WORDS]")
        _check("bsdb_dev_db_dump_text", lib().bsdb_dev_db_dump_text(
            db._h, count, _ptr(ksrc), _ptr(klen), _ptr(vsrc), _ptr(vlen), _ptr(llen), _ptr(loff), self._sep(separator), _ptr(text),
            text_bytes, _ptr(status), first, _ptr(report), _stream(stream)))
        return text[:text_bytes], status, report

    # ---- two resident databases compared: records(A) -> gather keys -> locate in B -> diff -> select
    @staticmethod
    def diff_report(device):
        """A fresh device report for db_diff: int64[DIFF_WORDS], zero with first_diff = UINT64_MAX (-1)."""
        import torch
        report = torch.zeros(DIFF_WORDS, dtype=torch.int64, device=device)
        report[8] = -1
        return report

    def db_diff(self, a: "Database", b: "Database", vsrc_a, vlen_a, status_a, src_b, vlen_b, status, slot_base: int = 0,
                count: Optional[int] = None, report=None, stream=None):
        """bsdb_dev_db_diff: A's values (vsrc_a int64, vlen_a int32, status_a
        uint8 of db_records on `a`) against B's (src_b int64, vlen_b int32,
        status uint8 of db_locate_var on `b` for the same records' keys).
        `status` is rewritten in place to the diff's; `report`
        (Context.diff_report, made here when not given) accumulates;
        `slot_base` is A's slot of record 0.  Returns (status, report)."""
        import torch
        if count is None:
            count = status.numel()
        if report is None:
            report = self.diff_report(status.device)
        if (vsrc_a.dtype != torch.int64 or src_b.dtype != torch.int64 or vlen_a.dtype != torch.int32 or vlen_b.dtype != torch.int32
                or status_a.dtype != torch.uint8 or status.dtype != torch.uint8 or report.dtype != torch.int64
                or report.numel() < DIFF_WORDS
                or min(vsrc_a.numel(), src_b.numel(), vlen_a.numel(), vlen_b.numel(), status_a.numel(), status.numel()) < count):
            raise ValueError("vsrc_a / src_b int64[count], vlen_a / vlen_b int32[count], status_a / status uint8[count], "
                             "report int64[DIFF_WORDS]")
        _check("bsdb_dev_db_diff", lib().bsdb_dev_db_diff(
            a._h, b._h, count, _ptr(vsrc_a), _ptr(vlen_a), _ptr(status_a), _ptr(src_b), _ptr(vlen_b), _ptr(status), slot_base,
            _ptr(report), _stream(stream)))
        return status[:count], report

    def db_select(self, db: "Database", status, mask: int, ksrc, klen, vsrc, vlen, stream=None):
        """bsdb_dev_db_select: the records whose status bit is set in `mask`,
        in slot order: (sel int64, ksrc, klen, vsrc, vlen) cut to the number
        selected (read back, which synchronises).  The descriptors feed
        db_dump_text with a zeroed status array."""
        import torch
        count = status.numel()
        if (status.dtype != torch.uint8 or ksrc.dtype != torch.int64 or vsrc.dtype != torch.int64 or klen.dtype != torch.int32
                or vlen.dtype != torch.int32 or min(ksrc.numel(), vsrc.numel(), klen.numel(), vlen.numel()) < count):
            raise ValueError("status uint8[count], ksrc / vsrc int64[count], klen / vlen int32[count]")
        dev, k = status.device, max(count, 1)
        sel, ksrc_o, vsrc_o = (torch.empty(k, dtype=torch.int64, device=dev) for _ in range(3))
        klen_o, vlen_o = (torch.empty(k, dtype=torch.int32, device=dev) for _ in range(2))
        nsel = torch.zeros(1, dtype=torch.int64, device=dev)
        _check("bsdb_dev_db_select", lib().bsdb_dev_db_select(
            db._h, count, _ptr(status), mask, _ptr(ksrc), _ptr(klen), _ptr(vsrc), _ptr(vlen), _ptr(sel), _ptr(ksrc_o), _ptr(klen_o),
            _ptr(vsrc_o), _ptr(vlen_o), _ptr(nsel), _stream(stream)))
        n = int(nsel[0])
        return sel[:n], ksrc_o[:n], klen_o[:n], vsrc_o[:n], vlen_o[:n]

    # ---- resident databases merged: records(base) -> locate in delta / removed -> status -> select -> pack
    def db_merge_status(self, status_base, status_delta=None, status_removed=None, report=None, stream=None):
        """bsdb_dev_db_merge_status: db_records' status of base's slots and
        locate's statuses of their keys in delta / removed (either None: that
        database is not there), all uint8[count], into the merge's status
        byte.  `report` int64[MERGE_WORDS] (zeros when made here)
        accumulates.  Returns (status, report); ``db_select(db, status, 1 <<
        MERGE_KEPT, ...)`` gives the records that go on."""
        import torch
        count = status_base.numel()
        for t in (status_base, status_delta, status_removed):
            if t is not None and (t.dtype != torch.uint8 or t.numel() < count):
                raise ValueError("status arrays are uint8[count]")
        if report is None:
            report = torch.zeros(MERGE_WORDS, dtype=torch.int64, device=status_base.device)
        elif report.dtype != torch.int64 or report.numel() < MERGE_WORDS:
            raise ValueError("report int64[MERGE_WORDS]")
        out = torch.empty(max(count, 1), dtype=torch.uint8, device=status_base.device)
        _check("bsdb_dev_db_merge_status", lib().bsdb_dev_db_merge_status(
            self._h, count, _ptr(status_base), None if status_delta is None else _ptr(status_delta),
            None if status_removed is None else _ptr(status_removed), _ptr(out), _ptr(report), _stream(stream)))
        return out[:count], report

    def db_pack(self, db: "Database", ksrc, klen, vsrc, vlen, partitions: int, part_sizes, approximate: bool = False,
                count: Optional[int] = None, image=None, addr=None, blob=None, off=None, value8=None, value_len=None,
                stream=None, block_size: Optional[int] = None, want_image: bool = True) -> dict:
        """bsdb_dev_db_pack: the records of db's resident image that the
        descriptors name (db_records' or db_select's: ksrc / vsrc int64, klen /
        vlen int32) into a kv.db image, compact or -- with `block_size` --
        blocked.  Arguments and result as text_pack's."""
        import numpy as np
        import torch
        if count is None:
            count = ksrc.numel()
        if (ksrc.dtype != torch.int64 or vsrc.dtype != torch.int64 or klen.dtype != torch.int32 or vlen.dtype != torch.int32
                or min(ksrc.numel(), vsrc.numel(), klen.numel(), vlen.numel()) < count):
            raise ValueError("ksrc / vsrc int64[count], klen / vlen int32[count]")
        dev = ksrc.device
        sizes = np.ascontiguousarray(part_sizes, np.uint64)
        if sizes.size != partitions:
            raise ValueError("one size per partition")
        most = count * MERGE_MAX_RECORD
        if image is None and want_image:
            image = torch.empty((2 * most + partitions * block_size if block_size else most) + 16, dtype=torch.uint8, device=dev)
        if blob is None:
            blob = torch.empty(count * TEXT_MAX_KEY + 16, dtype=torch.uint8, device=dev)
        if addr is None:
            addr = torch.empty(max(count, 1), dtype=torch.int64, device=dev)
        if off is None:
            off = torch.empty(count + 1, dtype=torch.int64, device=dev)
        if approximate and value8 is None:
            value8 = torch.empty(max(count, 1), dtype=torch.int64, device=dev)
        if approximate and value_len is None:
            value_len = torch.empty(max(count, 1), dtype=torch.uint8, device=dev)
        if addr.numel() < count or off.numel() < count + 1 or (approximate and min(value8.numel(), value_len.numel()) < count):
            raise ValueError("addr / value8 / value_len hold count entries, off count + 1")
        runs = np.zeros(partitions, np.uint64)
        blob_bytes = C.c_uint64()
        _check("bsdb_dev_db_pack", lib().bsdb_dev_db_pack(
            self._h, db._h, _ptr(ksrc), _ptr(klen), _ptr(vsrc), _ptr(vlen), count, partitions, 0 if block_size is None else 1,
            block_size or 0, sizes.ctypes.data, _ptr(image) if want_image else None, image.numel() if want_image else 0,
            runs.ctypes.data, _ptr(addr), _ptr(blob), blob.numel(), _ptr(off), C.byref(blob_bytes),
            _ptr(value8) if approximate else None, _ptr(value_len) if approximate else None, _stream(stream)))
        return {"image": image[: int(runs.sum())] if want_image else None, "run_bytes": [int(x) for x in runs], "addr": addr[:count],
                "blob": blob[: blob_bytes.value], "off": off[: count + 1],
                "value8": value8[:count] if approximate else None, "value_len": value_len[:count] if approximate else None}

    # ---- text front end: lines of "key<sep>value" -> descriptors -> kv.db image
    @staticmethod
    def _sep(separator) -> int:
        s = separator.encode("latin-1") if isinstance(separator, str) else bytes(separator)
        if len(s) != 1:
            raise ValueError("the separator is one byte")
        return s[0]

    def text_split(self, text, separator=" ", nbytes: Optional[int] = None, desc=None, report=None, stream=None):
        """bsdb_dev_text_split: `text` a uint8 tensor at a 16-byte aligned
        address.  Returns (desc, report): desc int32[4, cap] with rows kpos,
        klen, vpos, vlen (cap >= text_max_records(nbytes)), the first
        report[1] columns written in input order; report int64[TEXT_WORDS]
        (zeroed by the caller when given) accumulates."""
        import torch
        if nbytes is None:
            nbytes = text.numel()
        cap = text_max_records(nbytes)
        if desc is None:
            desc = torch.empty((4, cap), dtype=torch.int32, device=text.device)
        elif desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[0] != 4 or not desc.is_contiguous():
            raise ValueError("desc is a contiguous int32[4, cap]")
        if report is None:
            report = torch.zeros(TEXT_WORDS, dtype=torch.int64, device=text.device)
        elif report.dtype != torch.int64 or report.numel() < TEXT_WORDS:
            raise ValueError("report int64[TEXT_WORDS]")
        _check("bsdb_dev_text_split", lib().bsdb_dev_text_split(
            self._h, _ptr(text), nbytes, self._sep(separator), desc.shape[1], _ptr(desc[0]), _ptr(desc[1]),
            _ptr(desc[2]), _ptr(desc[3]), _ptr(report), _stream(stream)))
        return desc, report

    def text_pack(self, text, desc, count: int, partitions: int, part_sizes, approximate: bool = False,
                  nbytes: Optional[int] = None, image=None, addr=None, blob=None, off=None, value8=None, value_len=None,
                  stream=None, block_size: Optional[int] = None, want_image: bool = True) -> dict:
        """bsdb_dev_text_pack of the first `count` descriptors of text_split;
        with `block_size`, bsdb_dev_text_pack_blocked: the blocked layout in
        blocks of that many bytes (part_sizes multiples of 4096).
        The outputs are the caller's tensors or allocated here: image / blob /
        value_len uint8 at any address, addr / off / value8 int64.  Returns
        {"image", "run_bytes", "addr", "blob", "off", "value8", "value_len"},
        each cut to what was written; run p is image[sum(run_bytes[:p]):][:run_bytes[p]].
        ``want_image=False``: no image is written (the key blob and offsets alone)."""
        import numpy as np
        import torch
        if nbytes is None:
            nbytes = text.numel()
        dev = text.device
        sizes = np.ascontiguousarray(part_sizes, np.uint64)
        if sizes.size != partitions:
            raise ValueError("one size per partition")
        if image is None and want_image:
            image = torch.empty(text_image_max(nbytes, partitions, 0 if block_size is None else 1, block_size or 0),
                                dtype=torch.uint8, device=dev)
        if blob is None:
            blob = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
        if addr is None:
            addr = torch.empty(max(count, 1), dtype=torch.int64, device=dev)
        if off is None:
            off = torch.empty(count + 1, dtype=torch.int64, device=dev)
        if approximate and value8 is None:
            value8 = torch.empty(max(count, 1), dtype=torch.int64, device=dev)
        if approximate and value_len is None:
            value_len = torch.empty(max(count, 1), dtype=torch.uint8, device=dev)
        if addr.numel() < count or off.numel() < count + 1 or (approximate and min(value8.numel(), value_len.numel()) < count):
            raise ValueError("addr / value8 / value_len hold count entries, off count + 1")
        runs = np.zeros(partitions, np.uint64)
        blob_bytes = C.c_uint64()
        head = (self._h, _ptr(text), nbytes, _ptr(desc[0]), _ptr(desc[1]), _ptr(desc[2]), _ptr(desc[3]), count, partitions)
        tail = (sizes.ctypes.data, _ptr(image) if want_image else None, image.numel() if want_image else 0, runs.ctypes.data, _ptr(addr), _ptr(blob), blob.numel(),
                _ptr(off), C.byref(blob_bytes), _ptr(value8) if approximate else None,
                _ptr(value_len) if approximate else None, _stream(stream))
        if block_size is None:
            _check("bsdb_dev_text_pack", lib().bsdb_dev_text_pack(*head, *tail))
        else:
            _check("bsdb_dev_text_pack_blocked", lib().bsdb_dev_text_pack_blocked(*head, block_size, *tail))
        return {"image": image[: int(runs.sum())] if want_image else None, "run_bytes": [int(x) for x in runs], "addr": addr[:count],
                "blob": blob[: blob_bytes.value], "off": off[: count + 1],
                "value8": value8[:count] if approximate else None, "value_len": value_len[:count] if approximate else None}

    def text_set_chunk(self, nbytes: int = 0):
        """Text bytes bsdb_text_build handles at a time (0 = default)."""
        _check("bsdb_text_set_chunk", lib().bsdb_text_set_chunk(self._h, nbytes))

    def text_build(self, paths, separator, kv_base: str, partitions: int, width: int, index_path: str,
                   index_a_path: Optional[str] = None, approximate: bool = False, fmt: int = 0, block_size: int = 4096):
        """bsdb_text_build_layout: (Mph, report dict); fmt 0 the compact kv.db
        layout (bsdb_text_build), 1 the blocked one in blocks of `block_size`
        bytes.  A failure raises BsdbError with the report so far in
        ``.text_report``."""
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        report = (C.c_uint64 * TEXT_WORDS)()
        h = C.c_void_p()
        rc = lib().bsdb_text_build_layout(self._h, arr, len(paths), self._sep(separator), os.fsencode(kv_base), partitions,
                                          fmt, block_size, width, 1 if approximate else 0, os.fsencode(index_path),
                                          os.fsencode(index_a_path) if index_a_path else None, report, C.byref(h))
        rep = {k: int(v) for k, v in zip(TEXT_FIELDS, report)}
        if rc != BSDB_OK:
            e = BsdbError("bsdb_text_build", rc)
            e.text_report = rep
            raise e
        return Mph(h, self), rep

    def gen_keys_var(self, first: int, n: int, stream=None, offsets=None, blob=None):
        """Config C5 var-len keys on the device: (blob u8, offsets int64[n+1]).
        offsets / blob: the caller's tensors (blob.numel() is the capacity the
        library checks the key bytes against)."""
        import torch
        off = offsets
        if off is None:
            off = torch.empty(n + 1, dtype=torch.int64, device=f"cuda:{self.device}")
        elif off.dtype != torch.int64 or off.numel() < n + 1:
            raise ValueError("offsets holds fewer than n + 1 int64")
        _check("bsdb_dev_gen_keys_var", lib().bsdb_dev_gen_keys_var(self._h, first, n, _ptr(off), None, 0,
                                                                    _stream(stream)))
        if blob is None:
            total = int(off[n])
            blob = torch.empty(total + 16, dtype=torch.uint8, device=f"cuda:{self.device}")
        _check("bsdb_dev_gen_keys_var", lib().bsdb_dev_gen_keys_var(self._h, first, n, _ptr(off), _ptr(blob),
                                                                    blob.numel(), _stream(stream)))
        return blob, off

    def gen_keys13(self, first: int, n: int, out=None, stream=None):
        """13*n key bytes (a view of a 16-B-padded allocation when `out` is
        None, so keys.numel() // 13 == n)."""
        import torch
        if out is None:
            out = torch.empty(13 * n + 16, dtype=torch.uint8, device=f"cuda:{self.device}")[: 13 * n]
        elif out.numel() < 13 * n:
            raise ValueError("out holds fewer than 13*n bytes")
        _check("bsdb_dev_gen_keys13", lib().bsdb_dev_gen_keys13(self._h, first, n, _ptr(out), _stream(stream)))
        return out

    # ---- host-buffer API (numpy in, numpy out; includes H2D/D2H)
    def histogram_fixed_host(self, keys_np, key_len: int, m: int, counts_np=None, seed: int = 0):
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        if counts_np is None:
            counts_np = np.zeros(m, np.uint32)
        n = keys_np.size // key_len
        _check("bsdb_histogram_fixed", lib().bsdb_histogram_fixed(
            self._h, keys_np.ctypes.data, key_len, n, seed & (2**64 - 1), m, counts_np.ctypes.data))
        return counts_np

    def hash_fixed_host(self, keys_np, key_len: int, seed: int = 0):
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        n = keys_np.size // key_len
        out = np.zeros((max(n, 1), 2), np.uint64)
        _check("bsdb_hash_fixed", lib().bsdb_hash_fixed(
            self._h, keys_np.ctypes.data, key_len, n, seed & (2**64 - 1), out.ctypes.data))
        return out[:n]

    @staticmethod
    def _var_host_args(blob_np, off_np):
        import numpy as np
        blob_np = np.ascontiguousarray(blob_np, np.uint8)
        off_np = np.ascontiguousarray(off_np, np.uint64)
        if off_np.ndim != 1 or off_np.size < 1:
            raise ValueError("offsets must be a 1-D array of n+1 entries")
        if off_np.size > 1 and (int(off_np[-1]) > blob_np.size or np.any(off_np[1:] < off_np[:-1])):
            raise ValueError("offsets must be non-decreasing and within the blob")
        return blob_np, off_np, off_np.size - 1

    def histogram_var_host(self, blob_np, off_np, m: int, counts_np=None, seed: int = 0):
        """Host-buffer var-len histogram (bsdb_histogram_var): key i is
        blob[off[i]:off[i+1]]; counts accumulate into counts_np (u32[m])."""
        import numpy as np
        blob_np, off_np, n = self._var_host_args(blob_np, off_np)
        if counts_np is None:
            counts_np = np.zeros(m, np.uint32)
        _check("bsdb_histogram_var", lib().bsdb_histogram_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, seed & (2**64 - 1), m, counts_np.ctypes.data))
        return counts_np

    def hash_var_host(self, blob_np, off_np, seed: int = 0):
        """Host-buffer var-len signatures (bsdb_hash_var), (n, 2) u64."""
        import numpy as np
        blob_np, off_np, n = self._var_host_args(blob_np, off_np)
        out = np.zeros((max(n, 1), 2), np.uint64)
        _check("bsdb_hash_var", lib().bsdb_hash_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, seed & (2**64 - 1), out.ctypes.data))
        return out[:n]


class Mph:
    """A GOV MPHF resident on one device (``bsdb_mph``)."""

    def __init__(self, h, ctx: Context):
        self._h = h
        self.ctx = ctx  # keeps the context alive

    def close(self):
        if self._h:
            _check("bsdb_mph_free", lib().bsdb_mph_free(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        n, m, vw, sw = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        w = C.c_uint32()
        _check("bsdb_mph_info", lib().bsdb_mph_info(self._h, C.byref(n), C.byref(m), C.byref(w), C.byref(vw),
                                                    C.byref(sw)))
        return {"n": n.value, "num_buckets": m.value, "width": w.value, "values_words": vw.value,
                "sig_words": sw.value}

    def export(self):
        """(E u64[m+1], values u64[], sigbits u64[] or None) -- the fields of
        GOVMinimalPerfectHashFunctionModified (GOV:284-313)."""
        import numpy as np
        i = self.info()
        E = np.zeros(i["num_buckets"] + 1, np.uint64)
        vals = np.zeros(i["values_words"], np.uint64)
        sb = np.zeros(i["sig_words"], np.uint64) if i["width"] else None
        _check("bsdb_mph_export", lib().bsdb_mph_export(self._h, E.ctypes.data, vals.ctypes.data,
                                                        sb.ctypes.data if sb is not None else None))
        return E, vals, sb

    def dump(self, path: str):
        _check("bsdb_mph_dump", lib().bsdb_mph_dump(self._h, path.encode()))

    def lookup_fixed(self, keys_np, key_len: int, check: bool = True):
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        n = keys_np.size // key_len
        out = np.zeros(max(n, 1), np.int64)
        _check("bsdb_mph_lookup_fixed", lib().bsdb_mph_lookup_fixed(
            self._h, keys_np.ctypes.data, key_len, n, 1 if check else 0, out.ctypes.data))
        return out[:n]

    def lookup_var(self, blob_np, off_np, check: bool = True):
        import numpy as np
        blob_np, off_np, n = Context._var_host_args(blob_np, off_np)
        out = np.zeros(max(n, 1), np.int64)
        _check("bsdb_mph_lookup_var", lib().bsdb_mph_lookup_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, 1 if check else 0, out.ctypes.data))
        return out[:n]

    # ---- F4: the database check (report dict: VERIFY_FIELDS + "ok"; BSDB_EVERIFY does not raise)
    def verify_index_fixed(self, keys_np, key_len: int, addr_np, index_path: str, index_a_path: Optional[str] = None,
                           approximate: bool = False, value8_np=None, vlen_np=None, windows: int = 0) -> dict:
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        n = keys_np.size // key_len
        a, v8, vl = Context._records_args(n, addr_np, value8_np, vlen_np, approximate)
        out = (C.c_uint64 * VERIFY_WORDS)()
        rc = lib().bsdb_mph_verify_index_fixed(
            self._h, keys_np.ctypes.data, key_len, n, a.ctypes.data, _np_ptr(v8), _np_ptr(vl), 1 if approximate else 0,
            index_path.encode(), index_a_path.encode() if index_a_path else None, windows, out)
        return _verify_report("bsdb_mph_verify_index_fixed", rc, out)

    def verify_index_var(self, blob_np, off_np, addr_np, index_path: str, index_a_path: Optional[str] = None,
                         approximate: bool = False, value8_np=None, vlen_np=None, windows: int = 0) -> dict:
        blob_np, off_np, n = Context._var_host_args(blob_np, off_np)
        a, v8, vl = Context._records_args(n, addr_np, value8_np, vlen_np, approximate)
        out = (C.c_uint64 * VERIFY_WORDS)()
        rc = lib().bsdb_mph_verify_index_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, a.ctypes.data, _np_ptr(v8), _np_ptr(vl),
            1 if approximate else 0, index_path.encode(), index_a_path.encode() if index_a_path else None, windows, out)
        return _verify_report("bsdb_mph_verify_index_var", rc, out)

    def verify_kv(self, kv_base: str, partitions: int, index_path: str, index_a_path: Optional[str] = None,
                  approximate: bool = False, fmt: int = 0, block_size: int = 4096, threads: int = 0,
                  windows: int = 0) -> dict:
        """bsdb_kv_verify_index: the records from the kv.db partition scan."""
        out = (C.c_uint64 * VERIFY_WORDS)()
        rc = lib().bsdb_kv_verify_index(
            self._h, kv_base.encode(), partitions, fmt, block_size, threads, 1 if approximate else 0,
            index_path.encode(), index_a_path.encode() if index_a_path else None, windows, out)
        return _verify_report("bsdb_kv_verify_index", rc, out)

    def open_db(self, kv_base: Optional[str], partitions: int, index_path: str, approximate: bool = False,
                fmt: int = 0, block_size: int = 4096) -> "Database":
        """bsdb_db_open: the finished database resident on this MPHF's device
        for batched gets.  Exact mode: index_path is index.db and kv_base the
        kv.db files' common prefix; approximate mode: index_path is index_a.db
        (kv_base may be None)."""
        return Database(self, kv_base, partitions, index_path, approximate, fmt, block_size)

    def write_index(self, index_path: str, index_a_path: Optional[str], approximate: bool, pass_cache_bytes: int,
                    feed):
        """BSDBWriter.buildIndex (W:107-155): for every pass, ``feed(put)``
        must call ``put(keys..., addr, value8, vlen)`` for every record (the
        kv.db scan).  Returns the number of passes."""
        return IndexWriter(self, index_path, index_a_path, approximate, pass_cache_bytes).run(feed)


def _get_report(report) -> dict:
    """The get report's words as a dict (GET_FIELDS, the header's order)."""
    return {k: int(v) for k, v in zip(GET_FIELDS, report)}


def _scan_report(report) -> dict:
    """The scan report's words as a dict (SCAN_FIELDS, the header's order); words taken as unsigned."""
    return {k: int(v) & SCAN_NONE for k, v in zip(SCAN_FIELDS, report)}


def _check_report(report) -> dict:
    """The check report's words as a dict (CHECK_FIELDS, the header's order); words taken as unsigned."""
    return {k: int(v) & CHECK_NONE for k, v in zip(CHECK_FIELDS, report)}


def _diff_report(report) -> dict:
    """The diff report's words as a dict (DIFF_FIELDS, the header's order); words taken as unsigned."""
    return {k: int(v) & DIFF_NONE for k, v in zip(DIFF_FIELDS, report)}


class Database:
    """``bsdb_db``: a finished database resident on one device; batched gets
    key -> value (SyncReader.getAsBytes for a batch).  Borrows its Mph."""

    def __init__(self, mph: Mph, kv_base: Optional[str], partitions: int, index_path: str, approximate: bool = False,
                 fmt: int = 0, block_size: int = 4096):
        self.mph = mph  # keeps the MPHF (and its context) alive
        self.approximate = approximate
        self._h = C.c_void_p()
        _check("bsdb_db_open", lib().bsdb_db_open(
            mph._h, kv_base.encode() if kv_base else None, partitions, fmt, block_size, 1 if approximate else 0,
            index_path.encode(), C.byref(self._h)))

    def close(self):
        if self._h:
            _check("bsdb_db_free", lib().bsdb_db_free(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        out = (C.c_uint64 * DB_INFO_WORDS)()
        _check("bsdb_db_info", lib().bsdb_db_info(self._h, out))
        return {k: int(v) for k, v in zip(DB_INFO_FIELDS, out)}

    def set_batch(self, max_queries: int = 0):
        """Queries per chunk of the host forms (0 = default); results do not depend on it."""
        _check("bsdb_db_set_batch", lib().bsdb_db_set_batch(self._h, max_queries))

    def _get(self, fn: str, call, nq: int, value_cap: Optional[int]):
        """One host get, once more with the reported size on BSDB_E2BIG."""
        import numpy as np
        status = np.zeros(max(nq, 1), np.uint8)
        voff = np.zeros(nq + 1, np.uint64)
        report = np.zeros(GET_WORDS, np.uint64)
        cap = (8 if self.approximate else 64) * nq if value_cap is None else value_cap
        for _ in range(2):
            values = np.zeros(max(cap, 1), np.uint8)
            rc = call(cap, values.ctypes.data, voff.ctypes.data, status.ctypes.data, report.ctypes.data)
            if rc != BSDB_E2BIG:
                break
            cap = int(report[5])
        _check(fn, rc)
        return {"status": status[:nq], "voff": voff, "values": values[: int(voff[nq])], "report": _get_report(report)}

    def get_fixed(self, keys_np, key_len: int, value_cap: Optional[int] = None) -> dict:
        """bsdb_db_get_fixed: {"status" u8[nq], "voff" u64[nq + 1], "values"
        u8[voff[nq]], "report" dict}; value i is values[voff[i]:voff[i + 1]]."""
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        nq = keys_np.size // key_len
        return self._get("bsdb_db_get_fixed", lambda cap, v, o, s, r: lib().bsdb_db_get_fixed(
            self._h, keys_np.ctypes.data, key_len, nq, cap, v, o, s, r), nq, value_cap)

    def get_var(self, blob_np, off_np, value_cap: Optional[int] = None) -> dict:
        """bsdb_db_get_var: as get_fixed for a key blob with offsets[nq + 1]."""
        blob_np, off_np, nq = Context._var_host_args(blob_np, off_np)
        return self._get("bsdb_db_get_var", lambda cap, v, o, s, r: lib().bsdb_db_get_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, nq, cap, v, o, s, r), nq, value_cap)

    def check_text(self, paths, separator=" ", bad_cap: int = 16) -> dict:
        """bsdb_db_check_text: the files of ``key<sep>value`` lines against
        this database, every record's key -> value compared on the device.
        Returns {"text": the split's report (TEXT_FIELDS), "check": the
        check's (CHECK_FIELDS), "bad": up to bad_cap (path, file offset of the
        record's key, status) of the records that are not OK in input order,
        "n_bad": how many there are, "ok": every record is OK}.  It tells
        whether the text is in the database, not the converse."""
        import numpy as np
        paths = [os.fspath(p) for p in paths]
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        text = (C.c_uint64 * TEXT_WORDS)()
        rep = (C.c_uint64 * CHECK_WORDS)()
        cap = max(int(bad_cap), 0)
        bfile, boff, bst = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint8)
        n_bad = C.c_uint64()
        rc = lib().bsdb_db_check_text(self._h, arr, len(paths), Context._sep(separator), text, rep, cap, bfile.ctypes.data,
                                      boff.ctypes.data, bst.ctypes.data, C.byref(n_bad))
        if rc not in (BSDB_OK, BSDB_EVERIFY):
            _check("bsdb_db_check_text", rc)
        held = min(cap, n_bad.value)
        return {"text": {k: int(v) for k, v in zip(TEXT_FIELDS, text)}, "check": _check_report(rep),
                "bad": [(paths[int(f)], int(o), int(s)) for f, o, s in zip(bfile[:held], boff[:held], bst[:held])],
                "n_bad": int(n_bad.value), "ok": rc == BSDB_OK}

    # ---- what the database holds, by slot
    def set_text_chunk(self, nbytes: int = 0):
        """Text bytes of one step of dump_text (0 = default, 256 MiB; at least DUMP_MAX_LINE); results do not depend on it."""
        _check("bsdb_db_set_text_chunk", lib().bsdb_db_set_text_chunk(self._h, nbytes))

    def items(self, first: int = 0, count: Optional[int] = None, key_cap: Optional[int] = None,
              value_cap: Optional[int] = None) -> dict:
        """bsdb_db_scan: the records of slots [first, first + count) (to the
        last slot when count is None) in slot order: {"keys" u8, "koff"
        u64[count + 1], "values" u8, "voff" u64[count + 1], "status"
        u8[count], "report" dict (SCAN_FIELDS)}; key i is
        keys[koff[i]:koff[i + 1]], value i alike; a BAD_ADDR slot has neither.
        Once more with the reported sizes on BSDB_E2BIG."""
        import numpy as np
        if count is None:
            count = self.info()["n"] - first
        status = np.zeros(max(count, 1), np.uint8)
        koff, voff = np.zeros(count + 1, np.uint64), np.zeros(count + 1, np.uint64)
        report = np.zeros(SCAN_WORDS, np.uint64)
        kcap = 16 * count if key_cap is None else key_cap
        vcap = 64 * count if value_cap is None else value_cap
        for _ in range(2):
            keys, values = np.zeros(max(kcap, 1), np.uint8), np.zeros(max(vcap, 1), np.uint8)
            rc = lib().bsdb_db_scan(self._h, first, count, kcap, vcap, keys.ctypes.data, koff.ctypes.data, values.ctypes.data,
                                    voff.ctypes.data, status.ctypes.data, report.ctypes.data)
            if rc != BSDB_E2BIG:
                break
            kcap, vcap = max(kcap, int(report[4])), max(vcap, int(report[5]))
        _check("bsdb_db_scan", rc)
        return {"keys": keys[: int(koff[count])], "koff": koff, "values": values[: int(voff[count])], "voff": voff,
                "status": status[:count], "report": _scan_report(report)}

    def dump_text(self, path, separator=" ", first: int = 0, count: Optional[int] = None, append: bool = False) -> dict:
        """bsdb_db_dump_text: the lines ``key<sep>value\n`` of slots [first,
        first + count) to the file `path` (appended to it when `append`), in
        slot order.  Returns the report (SCAN_FIELDS): a BAD_ADDR slot wrote
        nothing, a NOT_TEXT record was written raw and does not read back."""
        if count is None:
            count = self.info()["n"] - first
        report = (C.c_uint64 * SCAN_WORDS)()
        _check("bsdb_db_dump_text", lib().bsdb_db_dump_text(
            self._h, os.fsencode(os.fspath(path)), Context._sep(separator), first, count, 1 if append else 0, report))
        return _scan_report(report)

    def diff(self, other: "Database", upsert=None, removed=None, separator=" ") -> dict:
        """bsdb_db_diff: this database (A) against `other` (B, on the same
        Context), in both directions on the device.  `removed` receives the
        ``key<sep>value`` lines of A's records whose key B does not hold,
        `upsert` those of B's records that A does not hold or holds with
        another value; either may be None.  Returns {"ab", "ba": the two
        reports (DIFF_FIELDS), "upsert", "removed": the two files' reports
        (SCAN_FIELDS; empty without a file), "identical": every slot of
        either side is SAME in the other}."""
        ab, ba = (C.c_uint64 * DIFF_WORDS)(), (C.c_uint64 * DIFF_WORDS)()
        up, rm = (C.c_uint64 * SCAN_WORDS)(), (C.c_uint64 * SCAN_WORDS)()
        _check("bsdb_db_diff", lib().bsdb_db_diff(
            self._h, other._h, Context._sep(separator), None if upsert is None else os.fsencode(os.fspath(upsert)),
            None if removed is None else os.fsencode(os.fspath(removed)), ab, ba, up, rm))
        ab, ba = _diff_report(ab), _diff_report(ba)
        return {"ab": ab, "ba": ba, "upsert": _scan_report(up), "removed": _scan_report(rm),
                "identical": ab["same"] == self.info()["n"] and ba["same"] == other.info()["n"]}


    def merge(self, kv_base: str, partitions: int, width: int, index_path: str, index_a_path: Optional[str] = None,
              approximate: bool = False, fmt: int = 0, block_size: int = 4096, delta: Optional["Database"] = None,
              removed: Optional["Database"] = None):
        """bsdb_db_merge: this database (base), `delta`'s records over it and
        `removed`'s keys out of it (both on the same Context, either may be
        None: a rebuild) into new kv.db files at `kv_base` and new index
        files.  Returns (report dict (MERGE_FIELDS), Mph).  A damaged input
        stops the merge: BsdbError with code BSDB_EVERIFY and the report up to
        that chunk in ``.merge_report``; every other failure carries it too."""
        report = (C.c_uint64 * MERGE_WORDS)()
        h = C.c_void_p()
        rc = lib().bsdb_db_merge(self._h, delta._h if delta is not None else None, removed._h if removed is not None else None,
                                 os.fsencode(kv_base), partitions, fmt, block_size, width, 1 if approximate else 0,
                                 os.fsencode(index_path), os.fsencode(index_a_path) if index_a_path else None, report, C.byref(h))
        rep = {k: int(v) for k, v in zip(MERGE_FIELDS, report)}
        if rc != BSDB_OK:
            e = BsdbError("bsdb_db_merge", rc)
            e.merge_report = rep
            raise e
        return rep, Mph(h, self.mph.ctx)


class Builder:
    """``bsdb_builder``: BSDBWriter.put's key stream into one device's HBM,
    then the whole build by bucket-range passes (``finish``)."""

    def __init__(self, ctx: Context, key_len: int, key_capacity: int, blob_capacity: int, approximate: bool,
                 addr_base: int, addr_stride: int):
        self.ctx = ctx
        self.approx = approximate
        self._h = C.c_void_p()
        _check("bsdb_builder_open", lib().bsdb_builder_open(ctx._h, key_len, key_capacity, blob_capacity,
                                                            1 if approximate else 0, addr_base, addr_stride,
                                                            C.byref(self._h)))

    def close(self):
        if self._h:
            _check("bsdb_builder_free", lib().bsdb_builder_free(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count(self) -> int:
        n = C.c_uint64()
        _check("bsdb_builder_count", lib().bsdb_builder_count(self._h, C.byref(n)))
        return n.value

    def add_fixed(self, keys_np, key_len: int, addr_np=None, value8_np=None, vlen_np=None):
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        n = keys_np.size // key_len
        a = np.ascontiguousarray(addr_np, np.uint64) if addr_np is not None else None
        v8 = np.ascontiguousarray(value8_np, np.uint64) if value8_np is not None else None
        vl = np.ascontiguousarray(vlen_np, np.uint8) if vlen_np is not None else None
        _check("bsdb_builder_add_fixed", lib().bsdb_builder_add_fixed(
            self._h, keys_np.ctypes.data, key_len, n, _np_ptr(a), _np_ptr(v8), _np_ptr(vl)))

    def add_var(self, blob_np, off_np, addr_np=None, value8_np=None, vlen_np=None):
        import numpy as np
        blob_np, off_np, n = Context._var_host_args(blob_np, off_np)
        a = np.ascontiguousarray(addr_np, np.uint64) if addr_np is not None else None
        v8 = np.ascontiguousarray(value8_np, np.uint64) if value8_np is not None else None
        vl = np.ascontiguousarray(vlen_np, np.uint8) if vlen_np is not None else None
        _check("bsdb_builder_add_var", lib().bsdb_builder_add_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, _np_ptr(a), _np_ptr(v8), _np_ptr(vl)))

    def add_dev_var(self, blob, off, addr=None, value8=None, vlen=None, stream=None):
        """bsdb_builder_add_dev_var: the batch in device memory (torch
        tensors): blob uint8, off int64[count + 1] into it, addr / value8
        int64[count], vlen uint8[count]."""
        count = off.numel() - 1
        _check("bsdb_builder_add_dev_var", lib().bsdb_builder_add_dev_var(
            self._h, _ptr(blob), _ptr(off), count, _ptr(addr) if addr is not None else None,
            _ptr(value8) if value8 is not None else None, _ptr(vlen) if vlen is not None else None, _stream(stream)))

    def finish(self, width: int, index_path: Optional[str] = None, index_a_path: Optional[str] = None,
               passes: int = 0):
        """Builds everything added; returns (Mph, passes_used)."""
        h = C.c_void_p()
        used = C.c_uint32()
        _check("bsdb_builder_finish", lib().bsdb_builder_finish(
            self._h, width, passes, index_path.encode() if index_path else None,
            index_a_path.encode() if index_a_path else None, C.byref(h), C.byref(used)))
        return Mph(h, self.ctx), used.value

    def find_duplicates(self, cap: int = DUP_DEFAULT_CAP) -> dict:
        """bsdb_builder_find_duplicates: the duplicates among everything added
        so far, as pairs of record ADDRESSES (valid before finish)."""
        pairs, kinds, report = Context._dup_host_bufs(cap)
        _check("bsdb_builder_find_duplicates", lib().bsdb_builder_find_duplicates(
            self._h, cap, pairs.ctypes.data, kinds.ctypes.data, report.ctypes.data))
        return _dup_report(pairs[:cap], kinds[:cap], report)


class IndexWriter:
    """``bsdb_index``: index.db / index_a.db of BSDBWriter.buildIndex."""

    def __init__(self, mph: Mph, index_path: str, index_a_path: Optional[str], approximate: bool,
                 pass_cache_bytes: int):
        self.mph = mph
        self.approx = approximate
        self._h = C.c_void_p()
        p = C.c_uint64()
        _check("bsdb_index_open", lib().bsdb_index_open(
            mph._h, 1 if approximate else 0, pass_cache_bytes, index_path.encode(),
            index_a_path.encode() if index_a_path else None, C.byref(self._h), C.byref(p)))
        self.passes = p.value

    def begin_pass(self, i: int):
        _check("bsdb_index_begin_pass", lib().bsdb_index_begin_pass(self._h, i))

    def end_pass(self):
        _check("bsdb_index_end_pass", lib().bsdb_index_end_pass(self._h))

    def put_fixed(self, keys_np, key_len: int, addr_np, value8_np=None, vlen_np=None):
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        addr_np = np.ascontiguousarray(addr_np, np.uint64)
        v8 = np.ascontiguousarray(value8_np, np.uint64) if value8_np is not None else None
        vl = np.ascontiguousarray(vlen_np, np.uint8) if vlen_np is not None else None
        _check("bsdb_index_put_fixed", lib().bsdb_index_put_fixed(
            self._h, keys_np.ctypes.data, key_len, addr_np.size, addr_np.ctypes.data,
            v8.ctypes.data if v8 is not None else None, vl.ctypes.data if vl is not None else None))

    def put_var(self, blob_np, off_np, addr_np, value8_np=None, vlen_np=None):
        import numpy as np
        blob_np, off_np, n = Context._var_host_args(blob_np, off_np)
        addr_np = np.ascontiguousarray(addr_np, np.uint64)
        v8 = np.ascontiguousarray(value8_np, np.uint64) if value8_np is not None else None
        vl = np.ascontiguousarray(vlen_np, np.uint8) if vlen_np is not None else None
        _check("bsdb_index_put_var", lib().bsdb_index_put_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, addr_np.ctypes.data,
            v8.ctypes.data if v8 is not None else None, vl.ctypes.data if vl is not None else None))

    def close(self):
        if self._h:
            rc = lib().bsdb_index_close(self._h)
            self._h = C.c_void_p()
            _check("bsdb_index_close", rc)

    def run(self, feed):
        try:
            for i in range(self.passes):
                self.begin_pass(i)
                feed(self)
                self.end_pass()
        finally:
            self.close()
        return self.passes


class Multi:
    """``bsdb_multi``: every listed device of this process + one RCCL communicator."""

    def __init__(self, ndev: int, devices=None):
        self._h = C.c_void_p()
        arr = (C.c_int * ndev)(*devices) if devices is not None else None
        _check("bsdb_multi_open", lib().bsdb_multi_open(ndev, arr, C.byref(self._h)))

    def close(self):
        if self._h:
            _check("bsdb_multi_close", lib().bsdb_multi_close(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def size(self) -> int:
        return int(lib().bsdb_multi_size(self._h))

    def histogram_fixed(self, keys_np, key_len: int, seed: int = 0):
        """E[0..m] of host keys sharded over the devices (one all-reduce)."""
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        n = keys_np.size // key_len
        E = np.zeros(num_buckets(n) + 1, np.uint64)
        _check("bsdb_multi_histogram_fixed", lib().bsdb_multi_histogram_fixed(
            self._h, keys_np.ctypes.data, key_len, n, seed & (2**64 - 1), E.ctypes.data))
        return E

    def histogram_var(self, blob_np, off_np, seed: int = 0):
        import numpy as np
        blob_np, off_np, n = Context._var_host_args(blob_np, off_np)
        E = np.zeros(num_buckets(n) + 1, np.uint64)
        _check("bsdb_multi_histogram_var", lib().bsdb_multi_histogram_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, seed & (2**64 - 1), E.ctypes.data))
        return E

    def _build_outputs(self, n: int, width: int):
        import numpy as np
        E = np.zeros(num_buckets(n) + 1, np.uint64)
        vals = np.zeros(int(lib().bsdb_values_words(n)), np.uint64)
        sb = np.zeros((n * width + 63) // 64 + 1, np.uint64) if width else None
        return E, vals, sb

    def mph_build_index_fixed(self, keys_np, key_len: int, width: int, addr_np=None, index_path: Optional[str] = None,
                              index_a_path: Optional[str] = None, approximate: bool = False, value8_np=None,
                              vlen_np=None):
        """E4 over this process's devices (bsdb_multi_mph_build_index_fixed):
        the structure's fields (E, values, sigbits) as host arrays -- the same
        as Mph.export() of a one-device build -- and, with index_path, the
        index files written by every device at its slice's offset."""
        import numpy as np
        keys_np = np.ascontiguousarray(keys_np, np.uint8)
        n = keys_np.size // key_len
        addr_np, v8, vl = (Context._records_args(n, addr_np, value8_np, vlen_np, approximate) if index_path
                           else (None, None, None))
        E, vals, sb = self._build_outputs(n, width)
        _check("bsdb_multi_mph_build_index_fixed", lib().bsdb_multi_mph_build_index_fixed(
            self._h, keys_np.ctypes.data, key_len, n, width, _np_ptr(addr_np), _np_ptr(v8), _np_ptr(vl),
            1 if approximate else 0, index_path.encode() if index_path else None,
            index_a_path.encode() if index_a_path else None, E.ctypes.data, vals.ctypes.data, _np_ptr(sb)))
        return E, vals, sb

    def mph_build_index_var(self, blob_np, off_np, width: int, addr_np=None, index_path: Optional[str] = None,
                            index_a_path: Optional[str] = None, approximate: bool = False, value8_np=None,
                            vlen_np=None):
        blob_np, off_np, n = Context._var_host_args(blob_np, off_np)
        addr_np, v8, vl = (Context._records_args(n, addr_np, value8_np, vlen_np, approximate) if index_path
                           else (None, None, None))
        E, vals, sb = self._build_outputs(n, width)
        _check("bsdb_multi_mph_build_index_var", lib().bsdb_multi_mph_build_index_var(
            self._h, blob_np.ctypes.data, off_np.ctypes.data, n, width, _np_ptr(addr_np), _np_ptr(v8), _np_ptr(vl),
            1 if approximate else 0, index_path.encode() if index_path else None,
            index_a_path.encode() if index_a_path else None, E.ctypes.data, vals.ctypes.data, _np_ptr(sb)))
        return E, vals, sb


def kv_scan(kv_base: str, partitions: int, fmt: int = 0, block_size: int = 4096, threads: int = 0) -> dict:
    """The native kv.db scan (bsdb_kv_scan): dict of numpy copies -- blob,
    offsets, addr, value8, vlen, fixed_len.  Host only (no device needed)."""
    import numpy as np
    h = C.c_void_p()
    _check("bsdb_kv_scan", lib().bsdb_kv_scan(kv_base.encode(), partitions, fmt, block_size, threads, C.byref(h)))
    try:
        n, nb, fl = C.c_uint64(), C.c_uint64(), C.c_uint32()
        _check("bsdb_kv_records_info", lib().bsdb_kv_records_info(h, C.byref(n), C.byref(nb), C.byref(fl)))
        ptrs = [C.c_void_p() for _ in range(5)]
        _check("bsdb_kv_records_arrays", lib().bsdb_kv_records_arrays(h, *[C.byref(q) for q in ptrs]))

        def arr(q, count, dt):
            if count == 0 or not q.value:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(q, C.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                         shape=(count,)).copy()
        N = n.value
        return {"blob": arr(ptrs[0], nb.value, np.uint8), "offsets": arr(ptrs[1], N + 1, np.uint64),
                "addr": arr(ptrs[2], N, np.uint64), "value8": arr(ptrs[3], N, np.uint64),
                "vlen": arr(ptrs[4], N, np.uint8), "fixed_len": fl.value}
    finally:
        lib().bsdb_kv_records_free(h)


def _np_ptr(a):
    return a.ctypes.data if a is not None else None
