"""redrock_old_amd — MI355X-native batch serialize/deserialize engine for RedRock value blobs.

The product is the C-ABI library ``redrock_old_amd/librr_serdes.so`` (include/rr_serdes.h):
hand-written gfx950 HIP kernels behind a plain-C host layer.  This module is a thin ctypes
binding used by the tests, ``bench.py`` and ``__graft_entry__``; it adds no compute of its own
and has no CPU fallback: if the library is missing or no GPU is present, calls raise.

Reference interface it mirrors (src/rock_serdes.h:47-49): ``serObject`` / ``desObject`` turn
one Redis object into a blob and back; here ``Engine.encode*`` / ``Engine.decode*`` do the same
for whole batches in the flat form of include/rr_format.h.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RR_LIB selects an alternative in-tree build (e.g. the probe build librr_serdes_probe.so).
LIB_PATH = os.path.join(_HERE, os.environ.get("RR_LIB", "librr_serdes.so"))

# --- flat form dtypes (include/rr_format.h) ---------------------------------------------
VALUE_DT = np.dtype([("type", "u1"), ("enc", "u1"), ("status", "<u2"), ("lru", "<u4"),
                     ("n_elems", "<u4"), ("elem_base", "<u4")])
ELEM_DT = np.dtype([("data", "<u8"), ("len", "<u4"), ("kind", "u1"), ("zenc", "u1"), ("rsv", "<u2")])
assert VALUE_DT.itemsize == 16 and ELEM_DT.itemsize == 16

T_STRING, T_SET_HT, T_HASH_HT, T_ZSET_SKIPLIST = 0, 2, 4, 5
T_SET_INTSET, T_ZSET_ZIPLIST, T_HASH_ZIPLIST, T_LIST_QUICKLIST = 11, 12, 13, 14
K_STR, K_INT, K_SCORE, K_ZLRAW = 0, 1, 2, 3
STATUS_NAMES = {0: "OK", 1: "SHORT", 2: "TYPE", 3: "STR_ENC", 4: "STR_INTLEN", 5: "EMBSTR_LEN",
                6: "TRUNC", 7: "COUNT", 8: "INTSET", 9: "ZL_LEN", 10: "ZL_CORRUPT", 11: "CAPACITY",
                12: "ENCODE", 13: "DUP", 14: "NAN"}

CONFIG_MIXED = 4
CTX_NO_SMALL = 1          # rr_ctx_set_options: no one-launch small-batch kernels
CTX_ZL_RAW = 2            # rr_ctx_set_options / the host codec's _ex calls: ziplists kept raw, the
                          # reference's acceptance rule (one ZLRAW descriptor, no entry walk)
SMALL_N, SMALL_BYTES = 4096, 128 * 1024   # the one-launch kernels' limits (rr_serdes.h)


class RRError(RuntimeError):
    pass


class Totals(C.Structure):
    _fields_ = [("n_elems", C.c_uint64), ("bytes", C.c_uint64), ("n_bad", C.c_uint64),
                ("payload", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class BlobBatch(C.Structure):
    _fields_ = [("data", C.c_void_p), ("offsets", C.c_void_p), ("n", C.c_uint64), ("data_cap", C.c_uint64)]


class FlatBatch(C.Structure):
    _fields_ = [("values", C.c_void_p), ("elems", C.c_void_p), ("arena", C.c_void_p), ("n", C.c_uint64),
                ("elem_cap", C.c_uint64), ("arena_cap", C.c_uint64)]


class RdbSaveOpts(C.Structure):
    _fields_ = [("list_fill", C.c_int32), ("flags", C.c_uint32)]   # flags: 0 or RDBSAVE_LZF


class RdbLoadOpts(C.Structure):
    """rr_rdbload_opts (include/rr_rdbload.h); the defaults are the reference's (config.c:2261-2267)."""
    _fields_ = [("lru", C.c_uint32), ("set_max_intset_entries", C.c_uint32), ("hash_max_ziplist_entries", C.c_uint32),
                ("hash_max_ziplist_value", C.c_uint32), ("zset_max_ziplist_entries", C.c_uint32),
                ("zset_max_ziplist_value", C.c_uint32), ("flags", C.c_uint32)]

    def __init__(self, lru=0, set_max_intset_entries=512, hash_max_ziplist_entries=512, hash_max_ziplist_value=64,
                 zset_max_ziplist_entries=128, zset_max_ziplist_value=64, flags=0):
        super().__init__(lru, set_max_intset_entries, hash_max_ziplist_entries, hash_max_ziplist_value,
                         zset_max_ziplist_entries, zset_max_ziplist_value, flags)


class RdbFileIn(C.Structure):
    """rr_rdbfile_in (include/rr_rdbfile.h): device pointers for rr_rdbfile_section, host ones for _host."""
    _fields_ = [("payloads", BlobBatch), ("keys", BlobBatch), ("types", C.c_void_p), ("status", C.c_void_p),
                ("expires", C.c_void_p), ("idle", C.c_void_p), ("freq", C.c_void_p), ("head", C.c_void_p),
                ("head_bytes", C.c_uint64)]


class RdbFileResult(C.Structure):
    _fields_ = [("bytes", C.c_uint64), ("n_bad", C.c_uint64), ("status", C.c_uint32), ("rsv", C.c_uint32)]

    def as_dict(self):
        return {"bytes": int(self.bytes), "n_bad": int(self.n_bad), "status": int(self.status)}


class RdbFileRepl(C.Structure):
    _fields_ = [("stream_db", C.c_int32), ("replid", C.c_char_p), ("offset", C.c_int64)]


class RdbReadState(C.Structure):
    """rr_rdbread_state (include/rr_rdbread.h): zeroed before the first rr_rdbread_index call."""
    _fields_ = [("version", C.c_uint32), ("rsv", C.c_uint32), ("db", C.c_uint64), ("pos", C.c_uint64)]


class RdbReadIndexResult(C.Structure):
    _fields_ = [("n_recs", C.c_uint64), ("n_items", C.c_uint64), ("eof_at", C.c_uint64), ("cksum", C.c_uint64),
                ("err_at", C.c_uint64), ("has_cksum", C.c_uint32), ("rsv", C.c_uint32)]


class RdbReadOut(C.Structure):
    """rr_rdbread_out: device pointers for rr_rdbread_split, host ones for _host."""
    _fields_ = [("keys", BlobBatch), ("payloads", BlobBatch), ("types", C.c_void_p), ("expires", C.c_void_p),
                ("idle", C.c_void_p), ("freq", C.c_void_p), ("status", C.c_void_p)]


RDBREAD_ITEM_DT = np.dtype([("opcode", "<u4"), ("rsv", "<u4"), ("at", "<u8"), ("end", "<u8")])   # rr_rdbread_item


class Shard(C.Structure):
    _fields_ = [("v0", C.c_uint64), ("v1", C.c_uint64), ("b0", C.c_uint64), ("b1", C.c_uint64)]


class Xfer(C.Structure):
    _fields_ = [("peer", C.c_int32), ("dir", C.c_int32), ("buf", C.c_int32), ("rsv", C.c_int32),
                ("offset", C.c_uint64), ("bytes", C.c_uint64)]


# rr_xfer directions and buffers (include/rr_serdes.h)
XFER_SEND, XFER_RECV = 0, 1
BUF_WHOLE_DATA, BUF_WHOLE_OFFSETS, BUF_MINE_DATA, BUF_MINE_OFFSETS = 0, 1, 2, 3
BUF_MINE_VALUES, BUF_MINE_ELEMS, BUF_WHOLE_VALUES, BUF_WHOLE_ELEMS = 4, 5, 6, 7


class HostBatch(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_uint8)), ("offsets", C.POINTER(C.c_uint64)), ("n", C.c_uint64),
                ("bytes", C.c_uint64)]


# Every symbol include/rr_serdes.h declares (the ABI test checks they are all exported).
EXPORTS = ["rr_ctx_create", "rr_ctx_destroy", "rr_ctx_reserve", "rr_last_error", "rr_decode_batch",
           "rr_encode_batch", "rr_decode_elem_bound", "rr_decode_batch_host", "rr_encode_batch_host",
           "rr_gen_batch", "rr_host_batch_free", "rr_gen_default_seed", "rr_shard_plan", "rr_flat_rebase",
           "rr_comm_get_id", "rr_comm_init", "rr_comm_destroy", "rr_split_plan", "rr_split", "rr_gather",
           "rr_flat_rebase_host", "rr_gather_layout", "rr_copy_device", "rr_gen_sizes", "rr_gen_range",
           "rr_split_schedule", "rr_gather_schedule", "rr_ctx_set_options", "rr_host_decode_value_ex",
           "rr_host_decode_batch_ex"]
COMM_ID_BYTES = 128
# include/rr_snappy.h (GPU block compression)
SNAPPY_EXPORTS = ["rr_snappy_max_compressed_length", "rr_snappy_compress_bound", "rr_snappy_compress_batch",
                  "rr_snappy_decompress_batch", "rr_snappy_compress_batch_host", "rr_snappy_decompress_batch_host"]
# include/rr_lz4.h (GPU LZ4 block compression beside snappy, row f3)
LZ4_EXPORTS = ["rr_lz4_max_compressed_length", "rr_lz4_compress_bound", "rr_lz4_compress_batch",
               "rr_lz4_decompress_batch", "rr_lz4_compress_batch_host", "rr_lz4_decompress_batch_host"]
# include/rr_rdb.h (batched snapshot restore over the fork-child pipes, row f4; used from C)
RDB_EXPORTS = ["rr_rdb_request_batch", "rr_rdb_blobs_free", "rr_rdb_request_flat", "rr_rdb_flat_free", "rr_rdb_serve"]
# include/rr_kv.h (batched store I/O around the GPU path, row f2; used from C)
KV_EXPORTS = ["rr_kv_dump_batch", "rr_kv_restore_batch"]
# include/rr_host.h (the host codec: RedRock's per-key call sites through the compat shim, row f1)
HOST_EXPORTS = ["rr_host_reserve", "rr_host_decode_value", "rr_host_check_value", "rr_host_decode_batch",
                "rr_host_encode_size", "rr_host_encode_value", "rr_host_encode_batch"]
# include/rr_rdbsave.h (flat batch -> RDB value payloads for the snapshot child, row f4)
RDBSAVE_EXPORTS = ["rr_rdbsave_bound", "rr_rdbsave_batch", "rr_rdbsave_batch_host", "rr_rdbsave_request",
                   "rr_rdbsave_result_free"]
RDBSAVE_LZF = 1                 # rr_rdbsave_opts.flags: strings of more than 20 bytes try the LZF form
E_CAPACITY, E_ENCODE = 11, 12   # the per-value statuses of rdbsave (RR_E_*, rr_format.h)
# include/rr_rdbload.h (RDB value payloads -> rock blobs, the load direction of rr_rdbsave.h)
RDBLOAD_EXPORTS = ["rr_rdbload_bound", "rr_rdbload_batch", "rr_rdbload_batch_host"]
RDBLOAD_E_TYPE, RDBLOAD_E_LEN, RDBLOAD_E_TRUNC, RDBLOAD_E_LZF = 32, 33, 34, 35
RDBLOAD_E_EXTRA, RDBLOAD_E_ZIPLIST, RDBLOAD_E_CONVERT = 36, 37, 38
RDBLOAD_LZF_NODE_MAX = 10240    # the longest List node taken in the LZF form
# include/rr_rdbconvert.h (the values rdbload left with RDBLOAD_E_CONVERT, in the encoding rdbLoadObject picks)
RDBCONVERT_EXPORTS = ["rr_rdbconvert_bound", "rr_rdbconvert_batch", "rr_rdbconvert_batch_host"]
RDBCONVERT_SKIP = 45            # not attempted: load_status != RDBLOAD_E_CONVERT
RDBCONVERT_MAX_N = 512          # the most members of a Set or ZSet that is sorted
RDBCONVERT_MAX_WAVES = 16384    # a wave an attempted value, a grid stride beyond
# include/rr_d2string.h (d2string with an exact %.17g, host and GPU)
D2STRING_EXPORTS = ["rr_d2string", "rr_d2string_batch", "rr_d2string_batch_host"]
D2STRING_MAX = 24               # the longest text: "-4.9406564584124654e-324"
D2STRING_SLOT = 32              # the batch calls' bytes per text
# include/rr_rdbzset.h (the small ZSets rdbconvert left because a score needs %.17g)
RDBZSET_EXPORTS = ["rr_rdbzset_bound", "rr_rdbzset_batch", "rr_rdbzset_batch_host"]
RDBZSET_SKIP = 55               # not attempted: not a ZSET_2 that rdbconvert left at RDBLOAD_E_CONVERT
# include/rr_rdbloadall.h (the three load stages merged into one blob batch)
RDBLOADALL_EXPORTS = ["rr_rdbmerge_batch", "rr_rdbloadall_caps", "rr_rdbloadall_ws_bytes", "rr_rdbloadall_batch",
                      "rr_rdbloadall_batch_host"]
RDBMERGE_E_SLICE = 57           # the holding stage's slice is reversed or past that batch's data_cap
RDBMERGE_SPAN = 8192            # bytes of the output a wave of the merge's emit kernel owns at a time
RDBMERGE_MAX_WAVES = 8192       # waves of that launch at most, a grid stride over the spans beyond
# include/rr_aof.h (flat batch -> AOF rewrite commands, the AOF half of row f4)
AOF_EXPORTS = ["rr_aof_bound", "rr_aof_select", "rr_aof_score_text", "rr_aof_batch", "rr_aof_batch_host"]
AOF_E_CPU = 56                  # left to the CPU path: a ZLRAW-only ziplist, a score text that is not taken
AOF_ITEMS_PER_CMD = 64          # AOF_REWRITE_ITEMS_PER_CMD
AOF_MAX_WAVES = 16384           # a wave a value, a grid stride beyond
AOF_SCORE_TEXT_MAX = 40         # the longest score text taken
# include/rr_rdbfile.h (RDB stream framing, DUMP payloads and their CRC-64 around the payloads above)
RDBFILE_EXPORTS = ["rr_rdbfile_bound", "rr_rdbfile_section", "rr_rdbfile_section_host", "rr_crc64_device",
                   "rr_rdbdump_batch", "rr_rdbdump_batch_host", "rr_rdbdump_verify_batch", "rr_rdbdump_verify_batch_host",
                   "rr_rdbfile_head", "rr_rdbfile_selectdb", "rr_crc64", "rr_crc64_shift", "rr_crc64_mul"]
RDBFILE_IDLE, RDBFILE_FREQ, RDBFILE_EOF, RDBFILE_NO_CKSUM = 1, 2, 4, 8
RDBFILE_E_VALUE, RDBFILE_E_KEY, RDBDUMP_E_SHORT, RDBDUMP_E_VERSION, RDBDUMP_E_CRC = 40, 41, 42, 43, 44
# the CRC kernels' shape (rr_rdbfile.h): bytes a lane, bytes a wave and step, waves a launch at most
CRC64_RUN, CRC64_PIECE, CRC64_MAX_WAVES = 256, 64 * 256, 2048
RDBDUMP_MAX_WAVES = 16384       # rr_rdbdump_batch / rr_rdbdump_verify_batch: a wave a value
# include/rr_rdbread.h (reading a complete RDB stream: host record index, GPU split and checksum verdict)
RDBREAD_EXPORTS = ["rr_rdbread_index", "rr_rdbread_string", "rr_rdbread_len", "rr_rdbread_split", "rr_rdbread_split_host",
                   "rr_rdbread_verify", "rr_rdbread_verify_host"]
RDBREAD_DONE, RDBREAD_MORE, RDBREAD_FULL = 0, 1, 2
RDBREAD_E_SLICE, RDBREAD_E_TRUNC, RDBREAD_E_OPCODE, RDBREAD_E_KEY, RDBREAD_NO_CKSUM = 46, 47, 48, 49, 50
RDBREAD_E_MAGIC, RDBREAD_E_VERSION, RDBREAD_E_UNSUPPORTED, RDBREAD_E_LEN = 51, 52, 53, 54
# the split's shape (rr_rdbread.h): waves a launch at most, bytes a lane copies a step, bytes a wave and step
RDBREAD_MAX_WAVES, RDBREAD_LANE_BYTES, RDBREAD_WAVE_STEP = 16384, 16, 64 * 16
API_EINVAL = -1                 # RR_API_EINVAL (rr_serdes.h)
SNAPPY_STATUS = {0: "OK", 1: "HEADER", 2: "TRUNC", 3: "OFFSET", 4: "OVERFLOW", 5: "LENGTH", 6: "CAPACITY"}
LZ4_STATUS = dict(SNAPPY_STATUS)   # RR_LZ4_* parallel RR_SNAPPY_*

_lib = None


def lib():
    """Load the in-tree engine library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RRError(f"{LIB_PATH} not built: run __graft_entry__.build()")
    # torch (used for device buffers and streams) ships its own libamdhip64.so.7; load it first
    # so this library binds to the same HIP runtime instead of a second copy from /opt/rocm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64 = C.c_void_p, C.c_uint64
    L.rr_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.rr_ctx_destroy.argtypes = [vp]
    L.rr_ctx_destroy.restype = None
    L.rr_ctx_reserve.argtypes = [vp, u64, u64]
    if hasattr(L, "rr_ctx_set_options"):   # (RR_LIB: an older build for A/B timing may predate it)
        L.rr_ctx_set_options.argtypes = [vp, C.c_uint]
    if hasattr(L, "rr_debug_fail_second"):   # test hook, not in rr_serdes.h
        L.rr_debug_fail_second.argtypes = [vp]
    if hasattr(L, "rr_debug_one_help"):   # test hook, not in rr_serdes.h
        L.rr_debug_one_help.argtypes = [vp]
    L.rr_last_error.restype = C.c_char_p
    L.rr_decode_batch.argtypes = [vp, C.POINTER(BlobBatch), C.POINTER(FlatBatch), vp, vp]
    L.rr_encode_batch.argtypes = [vp, C.POINTER(FlatBatch), C.POINTER(BlobBatch), vp, vp]
    L.rr_decode_elem_bound.argtypes = [u64, u64]
    L.rr_decode_elem_bound.restype = u64
    L.rr_decode_batch_host.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp, C.POINTER(Totals)]
    L.rr_encode_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, u64, vp, u64, vp, C.POINTER(Totals)]
    L.rr_gen_batch.argtypes = [C.c_int, u64, u64, C.POINTER(HostBatch)]
    L.rr_host_batch_free.argtypes = [C.POINTER(HostBatch)]
    L.rr_host_batch_free.restype = None
    L.rr_gen_sizes.argtypes = [C.c_int, u64, u64, u64, vp, vp, C.c_int]
    L.rr_gen_range.argtypes = [C.c_int, u64, u64, u64, C.POINTER(HostBatch), C.c_int]
    L.rr_gen_default_seed.argtypes = [C.c_int]
    L.rr_gen_default_seed.restype = u64
    L.rr_shard_plan.argtypes = [vp, u64, C.c_uint32, C.POINTER(Shard)]
    L.rr_flat_rebase.argtypes = [vp, vp, u64, vp, u64, u64, u64, vp]
    L.rr_flat_rebase_host.argtypes = [vp, u64, vp, u64, u64, u64]
    L.rr_gather_layout.argtypes = [vp, C.c_int, vp]
    if hasattr(L, "rr_split_schedule"):   # (RR_LIB: an older build for A/B timing may predate them)
        L.rr_split_schedule.argtypes = [C.POINTER(Shard), C.c_int, C.c_int, C.c_int, C.POINTER(Xfer)]
        L.rr_gather_schedule.argtypes = [C.POINTER(Shard), vp, C.c_int, C.c_int, C.c_int, C.POINTER(Xfer)]
    L.rr_gather_layout.restype = u64
    L.rr_copy_device.argtypes = [vp, vp, vp, u64, vp]
    L.rr_comm_get_id.argtypes = [vp]
    L.rr_comm_init.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.rr_comm_destroy.argtypes = [vp]
    L.rr_comm_destroy.restype = None
    L.rr_split_plan.argtypes = [vp, C.POINTER(BlobBatch), C.c_int, C.POINTER(Shard), vp]
    L.rr_split.argtypes = [vp, C.POINTER(BlobBatch), C.POINTER(Shard), C.c_int, C.POINTER(BlobBatch), vp]
    L.rr_gather.argtypes = [vp, C.POINTER(FlatBatch), u64, C.POINTER(Shard), C.c_int, C.POINTER(FlatBatch), vp]
    L.rr_snappy_max_compressed_length.argtypes = [u64]
    L.rr_snappy_max_compressed_length.restype = u64
    L.rr_snappy_compress_bound.argtypes = [u64, u64]
    L.rr_snappy_compress_bound.restype = u64
    L.rr_snappy_compress_batch.argtypes = [vp, C.POINTER(BlobBatch), C.POINTER(BlobBatch), vp]
    L.rr_snappy_decompress_batch.argtypes = [vp, C.POINTER(BlobBatch), C.POINTER(BlobBatch), vp, vp]
    L.rr_snappy_compress_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, vp]
    L.rr_snappy_decompress_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_lz4_compress_batch"):   # (RR_LIB: an older build may predate them)
        L.rr_lz4_max_compressed_length.argtypes = [u64]
        L.rr_lz4_max_compressed_length.restype = u64
        L.rr_lz4_compress_bound.argtypes = [u64, u64]
        L.rr_lz4_compress_bound.restype = u64
        L.rr_lz4_compress_batch.argtypes = [vp, C.POINTER(BlobBatch), C.POINTER(BlobBatch), vp]
        L.rr_lz4_decompress_batch.argtypes = [vp, C.POINTER(BlobBatch), C.POINTER(BlobBatch), vp, vp]
        L.rr_lz4_compress_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, vp]
        L.rr_lz4_decompress_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_rdbsave_batch"):   # (RR_LIB: an older build may predate them)
        L.rr_rdbsave_bound.argtypes = [u64, u64, u64]
        L.rr_rdbsave_bound.restype = u64
        L.rr_rdbsave_batch.argtypes = [vp, C.POINTER(FlatBatch), C.POINTER(BlobBatch), vp, vp, vp, C.POINTER(RdbSaveOpts), vp]
        L.rr_rdbsave_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, u64, C.POINTER(RdbSaveOpts), vp, u64, vp, vp, vp,
                                            C.POINTER(Totals)]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_rdbload_batch"):   # (RR_LIB: an older build may predate them)
        L.rr_rdbload_bound.argtypes = [u64, u64]
        L.rr_rdbload_bound.restype = u64
        L.rr_rdbload_batch.argtypes = [vp, C.POINTER(BlobBatch), vp, C.POINTER(BlobBatch), vp, vp, C.POINTER(RdbLoadOpts), vp]
        L.rr_rdbload_batch_host.argtypes = [vp, vp, vp, vp, u64, C.POINTER(RdbLoadOpts), vp, u64, vp, vp, C.POINTER(Totals)]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_rdbconvert_batch"):   # (RR_LIB: an older build may predate them)
        L.rr_rdbconvert_bound.argtypes = [u64, u64]
        L.rr_rdbconvert_bound.restype = u64
        L.rr_rdbconvert_batch.argtypes = [vp, C.POINTER(BlobBatch), vp, vp, C.POINTER(BlobBatch), vp, vp, vp,
                                          C.POINTER(RdbLoadOpts), vp]
        L.rr_rdbconvert_batch_host.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(RdbLoadOpts), vp, u64, vp, vp, vp,
                                               C.POINTER(Totals)]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_rdbzset_batch"):   # (RR_LIB: an older build may predate them)
        L.rr_d2string.argtypes = [vp, C.c_double]
        L.rr_d2string_batch.argtypes = [vp, vp, u64, vp, vp, vp]
        L.rr_d2string_batch_host.argtypes = [vp, vp, u64, vp, vp]
        L.rr_rdbzset_bound.argtypes = [u64, u64]
        L.rr_rdbzset_bound.restype = u64
        L.rr_rdbzset_batch.argtypes = [vp, C.POINTER(BlobBatch), vp, vp, C.POINTER(BlobBatch), vp, vp, C.POINTER(RdbLoadOpts), vp]
        L.rr_rdbzset_batch_host.argtypes = [vp, vp, vp, vp, vp, u64, C.POINTER(RdbLoadOpts), vp, u64, vp, vp, C.POINTER(Totals)]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_rdbloadall_batch"):   # (RR_LIB: an older build may predate them)
        bb = C.POINTER(BlobBatch)
        L.rr_rdbmerge_batch.argtypes = [vp, bb, vp, bb, vp, vp, bb, vp, vp, bb, vp, vp, vp, vp]
        L.rr_rdbloadall_caps.argtypes = [u64, u64, C.POINTER(u64)]
        L.rr_rdbloadall_caps.restype = None
        L.rr_rdbloadall_ws_bytes.argtypes = [u64, C.POINTER(u64)]
        L.rr_rdbloadall_ws_bytes.restype = u64
        L.rr_rdbloadall_batch.argtypes = [vp, bb, vp, vp, u64, C.POINTER(u64), bb, vp, vp, vp, vp, C.POINTER(RdbLoadOpts), vp]
        L.rr_rdbloadall_batch_host.argtypes = [vp, vp, vp, vp, u64, C.POINTER(RdbLoadOpts), vp, u64, vp, vp, vp, vp,
                                               C.POINTER(Totals)]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_aof_batch"):   # (RR_LIB: an older build may predate them)
        L.rr_aof_bound.argtypes = [u64, u64, u64, u64]
        L.rr_aof_bound.restype = u64
        L.rr_aof_select.argtypes = [vp, u64, C.c_int]
        L.rr_aof_score_text.argtypes = [vp, C.c_char_p, u64]
        L.rr_aof_batch.argtypes = [vp, C.POINTER(FlatBatch), C.POINTER(BlobBatch), vp, C.POINTER(BlobBatch), vp, vp, vp]
        L.rr_aof_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, u64, vp, vp, u64, vp, vp, u64, vp, vp, C.POINTER(Totals)]
    if "RR_LIB" not in os.environ or hasattr(L, "rr_rdbfile_section"):   # (RR_LIB: an older build may predate them)
        L.rr_rdbfile_bound.argtypes = [u64, u64, u64, u64]
        L.rr_rdbfile_bound.restype = u64
        L.rr_rdbfile_section.argtypes = [vp, C.POINTER(RdbFileIn), C.c_uint32, vp, u64, vp, vp, vp, vp, vp]
        L.rr_rdbfile_section_host.argtypes = [vp, C.POINTER(RdbFileIn), C.c_uint32, vp, u64, vp, vp, vp,
                                              C.POINTER(RdbFileResult)]
        L.rr_crc64_device.argtypes = [vp, vp, u64, vp, vp]
        L.rr_rdbdump_batch.argtypes = [vp, C.POINTER(BlobBatch), vp, vp, C.POINTER(BlobBatch), vp, vp, vp]
        L.rr_rdbdump_batch_host.argtypes = [vp, vp, vp, vp, vp, u64, vp, u64, vp, vp, C.POINTER(RdbFileResult)]
        L.rr_rdbdump_verify_batch.argtypes = [vp, C.POINTER(BlobBatch), C.POINTER(BlobBatch), vp, vp, vp, vp]
        L.rr_rdbdump_verify_batch_host.argtypes = [vp, vp, vp, u64, vp, u64, vp, vp, vp, C.POINTER(RdbFileResult)]
        L.rr_rdbfile_head.argtypes = [vp, u64, C.c_char_p, C.c_int64, u64, C.POINTER(RdbFileRepl), C.c_int]
        L.rr_rdbfile_head.restype = u64
        L.rr_rdbfile_selectdb.argtypes = [vp, u64, u64, u64, u64]
        L.rr_rdbfile_selectdb.restype = u64
        L.rr_crc64.argtypes = [u64, vp, u64]
        L.rr_crc64.restype = u64
        L.rr_crc64_shift.argtypes = [u64, u64]
        L.rr_crc64_shift.restype = u64
        L.rr_crc64_mul.argtypes = [u64, u64]
        L.rr_crc64_mul.restype = u64
    if "RR_LIB" not in os.environ or hasattr(L, "rr_rdbread_split"):   # (RR_LIB: an older build may predate them)
        L.rr_rdbread_index.argtypes = [C.POINTER(RdbReadState), vp, u64, vp, vp, vp, u64, vp, u64, C.POINTER(RdbReadIndexResult)]
        L.rr_rdbread_string.argtypes = [vp, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.rr_rdbread_len.argtypes = [vp, u64, u64, C.POINTER(u64), C.POINTER(u64)]
        L.rr_rdbread_split.argtypes = [vp, vp, u64, vp, vp, u64, C.c_uint32, C.POINTER(RdbReadOut), vp, vp]
        L.rr_rdbread_split_host.argtypes = [vp, vp, u64, vp, vp, u64, C.c_uint32, C.POINTER(RdbReadOut), C.POINTER(RdbFileResult)]
        L.rr_rdbread_verify.argtypes = [vp, vp, u64, u64, vp, vp, vp]
        L.rr_rdbread_verify_host.argtypes = [vp, vp, u64, u64, vp, C.POINTER(RdbFileResult)]
    if hasattr(L, "rr_host_decode_batch"):   # (RR_LIB: an older build for A/B timing may predate it)
        L.rr_host_reserve.argtypes = [vp, u64]
        L.rr_host_reserve.restype = u64
        L.rr_host_decode_value.argtypes = [vp, u64, u64, vp, vp, u64, C.POINTER(C.c_uint64)]
        L.rr_host_decode_batch.argtypes = [vp, vp, u64, vp, vp, u64, vp, C.POINTER(Totals)]
        L.rr_host_check_value.argtypes = [vp, u64, vp]
        L.rr_host_encode_size.argtypes = [vp, vp, u64, u64, C.POINTER(C.c_uint64)]
        L.rr_host_encode_value.argtypes = [vp, vp, vp, vp]
        L.rr_host_encode_value.restype = None
        L.rr_host_encode_batch.argtypes = [vp, vp, u64, vp, u64, u64, vp, u64, vp, C.POINTER(Totals)]
        # (the product library must export them: a missing one fails here, at load; only an older
        #  build named by RR_LIB for A/B timing may predate them)
        if "RR_LIB" not in os.environ or hasattr(L, "rr_host_decode_batch_ex"):
            L.rr_host_decode_value_ex.argtypes = [vp, u64, u64, vp, vp, u64, C.POINTER(C.c_uint64), C.c_uint]
            L.rr_host_decode_batch_ex.argtypes = [vp, vp, u64, vp, vp, u64, vp, C.POINTER(Totals), C.c_uint]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise RRError(f"rr call failed ({rc}): {lib().rr_last_error().decode()}")


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def gen_batch(config: int, n: int, seed: int | None = None):
    """Synthetic blob batch: returns (data uint8 padded to 16, offsets uint64)."""
    L = lib()
    if seed is None:
        seed = L.rr_gen_default_seed(config)
    hb = HostBatch()
    _check(L.rr_gen_batch(config, n, seed, C.byref(hb)))
    try:
        nbytes = int(hb.bytes)
        padded = (nbytes + 15) & ~15
        data = np.ctypeslib.as_array(hb.data, shape=(max(padded, 1),))[:padded].copy() if padded else \
            np.zeros(0, np.uint8)
        offs = np.ctypeslib.as_array(hb.offsets, shape=(n + 1,)).copy()
    finally:
        L.rr_host_batch_free(C.byref(hb))
    return data, offs


def gen_sizes(config: int, v0: int, v1: int, seed: int | None = None, nthreads: int = 8):
    """Config 5 (seekable): (blob bytes uint64, descriptor counts uint32) of values [v0, v1)."""
    L = lib()
    if seed is None:
        seed = L.rr_gen_default_seed(config)
    nb = np.zeros(max(v1 - v0, 1), np.uint64)
    nd = np.zeros(max(v1 - v0, 1), np.uint32)
    _check(L.rr_gen_sizes(config, v0, v1, seed, _ptr(nb), _ptr(nd), nthreads))
    return nb[:v1 - v0], nd[:v1 - v0]


def gen_range(config: int, v0: int, v1: int, seed: int | None = None, nthreads: int = 8):
    """Config 5 (seekable): (data uint8 padded to 16, offsets relative to v0) of values [v0, v1)."""
    L = lib()
    if seed is None:
        seed = L.rr_gen_default_seed(config)
    hb = HostBatch()
    _check(L.rr_gen_range(config, v0, v1, seed, C.byref(hb), nthreads))
    try:
        n, nbytes = v1 - v0, int(hb.bytes)
        padded = (nbytes + 15) & ~15
        data = np.ctypeslib.as_array(hb.data, shape=(max(padded, 1),))[:padded].copy() if padded else \
            np.zeros(0, np.uint8)
        offs = np.ctypeslib.as_array(hb.offsets, shape=(n + 1,)).copy()
    finally:
        L.rr_host_batch_free(C.byref(hb))
    return data, offs


def shard_plan(offsets: np.ndarray, g: int) -> np.ndarray:
    """The C library's byte-balanced plan (rr_shard_plan): (g, 4) uint64 rows v0, v1, b0, b1."""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    plan = (Shard * g)()
    _check(lib().rr_shard_plan(_ptr(offsets), len(offsets) - 1, g, plan))
    return np.array([[p.v0, p.v1, p.b0, p.b1] for p in plan], np.uint64).reshape(g, 4)


def flat_rebase_host(values: np.ndarray, elems: np.ndarray, elem_add: int, byte_add: int):
    """In place on host records (rr_flat_rebase_host): the placement rr_gather makes on the device."""
    assert values.dtype == VALUE_DT and elems.dtype == ELEM_DT and values.flags.c_contiguous and elems.flags.c_contiguous
    _check(lib().rr_flat_rebase_host(_ptr(values), len(values), _ptr(elems), len(elems), elem_add, byte_add))


def gather_layout(shard_elems) -> tuple[np.ndarray, int]:
    """(elem_at per shard, total) of the C library's gather placement (rr_gather_layout)."""
    ne = np.ascontiguousarray(shard_elems, np.uint64)
    at = np.zeros(max(len(ne), 1), np.uint64)
    tot = int(lib().rr_gather_layout(_ptr(ne), len(ne), _ptr(at)))
    if tot == 2 ** 64 - 1:
        raise RRError("gather layout past 2^32 - 1 descriptors")
    return at[:len(ne)], tot


def _plan_arg(plan):
    plan = np.ascontiguousarray(plan, np.uint64).reshape(-1, 4)
    arr = (Shard * len(plan))()
    for k, (v0, v1, b0, b1) in enumerate(plan):
        arr[k] = Shard(int(v0), int(v1), int(b0), int(b1))
    return arr, len(plan)


def _xfers(out, m):
    if m < 0:
        raise RRError("bad schedule arguments")
    return [(int(x.peer), int(x.dir), int(x.buf), int(x.offset), int(x.bytes)) for x in out[:m]]


def split_schedule(plan, rank: int, root: int = 0):
    """The transfers rr_split posts on `rank` (rr_split_schedule): [(peer, dir, buf, offset, bytes)]."""
    arr, g = _plan_arg(plan)
    out = (Xfer * (2 * g))()
    return _xfers(out, lib().rr_split_schedule(arr, g, rank, root, out))


def gather_schedule(plan, shard_elems, rank: int, root: int = 0):
    """The transfers rr_gather posts on `rank` (rr_gather_schedule)."""
    arr, g = _plan_arg(plan)
    ne = np.ascontiguousarray(shard_elems, np.uint64)
    out = (Xfer * (2 * g))()
    return _xfers(out, lib().rr_gather_schedule(arr, _ptr(ne), g, rank, root, out))


# ---- the host codec (include/rr_host.h) ------------------------------------------------------
# The CPU routing target of the compat shim for RedRock's per-key calls: explicit functions, never
# reached from Engine (the GPU entry points have no CPU fallback).
def host_decode(data: np.ndarray, offsets: np.ndarray, elem_cap: int | None = None):
    """rr_host_decode_batch: (values, elems, arena, totals) with rr_decode_batch_host's contract."""
    n = len(offsets) - 1
    nbytes = int(offsets[-1])
    if elem_cap is None:
        elem_cap = elem_bound(n, nbytes)
    data = np.ascontiguousarray(data, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    values = np.zeros(n, VALUE_DT)
    elems = np.zeros(max(elem_cap, 1), ELEM_DT)
    arena = np.zeros(max(nbytes, 1), np.uint8)
    t = Totals()
    _check(lib().rr_host_decode_batch(_ptr(data), _ptr(offsets), n, _ptr(values), _ptr(elems), elem_cap,
                                      _ptr(arena), C.byref(t)))
    ne = min(int(t.n_elems), elem_cap)
    return values, elems[:ne], arena[:nbytes], t.as_dict()


def host_decode_value(blob: bytes, base: int = 0, cap: int = 64):
    """rr_host_decode_value: (status, record, descriptors, need) of one blob."""
    b = np.frombuffer(bytes(blob) or b"\0", np.uint8)
    v = np.zeros(1, VALUE_DT)
    e = np.zeros(max(cap, 1), ELEM_DT)
    need = C.c_uint64()
    st = lib().rr_host_decode_value(_ptr(b), len(blob), base, _ptr(v), _ptr(e), cap, C.byref(need))
    return int(st), v[0], e[:min(int(v[0]["n_elems"]), cap)], int(need.value)


def host_decode_ex(data: np.ndarray, offsets: np.ndarray, flags: int, elem_cap: int | None = None):
    """rr_host_decode_batch_ex: host_decode with the RR_CTX_* decode flags (CTX_ZL_RAW)."""
    n = len(offsets) - 1
    nbytes = int(offsets[-1])
    if elem_cap is None:
        elem_cap = elem_bound(n, nbytes)
    data = np.ascontiguousarray(data, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    values = np.zeros(n, VALUE_DT)
    elems = np.zeros(max(elem_cap, 1), ELEM_DT)
    arena = np.zeros(max(nbytes, 1), np.uint8)
    t = Totals()
    _check(lib().rr_host_decode_batch_ex(_ptr(data), _ptr(offsets), n, _ptr(values), _ptr(elems), elem_cap,
                                         _ptr(arena), C.byref(t), flags))
    ne = min(int(t.n_elems), elem_cap)
    return values, elems[:ne], arena[:nbytes], t.as_dict()


def host_decode_value_ex(blob: bytes, flags: int, base: int = 0, cap: int = 64):
    """rr_host_decode_value_ex: host_decode_value with the RR_CTX_* decode flags (CTX_ZL_RAW)."""
    b = np.frombuffer(bytes(blob) or b"\0", np.uint8)
    v = np.zeros(1, VALUE_DT)
    e = np.zeros(max(cap, 1), ELEM_DT)
    need = C.c_uint64()
    st = lib().rr_host_decode_value_ex(_ptr(b), len(blob), base, _ptr(v), _ptr(e), cap, C.byref(need), flags)
    return int(st), v[0], e[:min(int(v[0]["n_elems"]), cap)], int(need.value)


def host_check(data: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """rr_host_check_value per blob: the records (elem_base 0) rr_host_decode_value gives."""
    data = np.ascontiguousarray(data, np.uint8)
    n = len(offsets) - 1
    out = np.zeros(n, VALUE_DT)
    L = lib()
    base = data.ctypes.data
    for i in range(n):
        o, ln = int(offsets[i]), int(offsets[i + 1] - offsets[i])
        L.rr_host_check_value(C.c_void_p(base + o), ln, C.c_void_p(out.ctypes.data + 16 * i))
    return out


def host_encode(values: np.ndarray, elems: np.ndarray, arena: np.ndarray, data_cap: int | None = None):
    """rr_host_encode_batch: (data, offsets, totals) with rr_encode_batch_host's contract."""
    n = len(values)
    values = np.ascontiguousarray(values, VALUE_DT)
    elems = np.ascontiguousarray(elems, ELEM_DT)
    arena = np.ascontiguousarray(arena, np.uint8)
    if data_cap is None:
        data_cap = encode_bound(values, elems)
    data = np.zeros(max(data_cap, 1), np.uint8)
    offsets = np.zeros(n + 1, np.uint64)
    t = Totals()
    _check(lib().rr_host_encode_batch(_ptr(values), _ptr(elems), len(elems), _ptr(arena), arena.size, n, _ptr(data),
                                      data_cap, _ptr(offsets), C.byref(t)))
    return data[:int(offsets[-1])], offsets, t.as_dict()


def elem_bound(n: int, nbytes: int) -> int:
    return int(lib().rr_decode_elem_bound(n, nbytes))


class Engine:
    """One engine context (one per host thread) on a HIP device."""

    def __init__(self, device: int = 0):
        self._L = lib()
        self._ctx = C.c_void_p()
        _check(self._L.rr_ctx_create(device, C.byref(self._ctx)))

    def close(self):
        if self._ctx:
            self._L.rr_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_options(self, flags: int):
        """RR_CTX_* flags (CTX_NO_SMALL: every call takes the batch pipeline; CTX_ZL_RAW: decode
        keeps Hash / ZSet ziplists raw, the reference's acceptance rule).  Read at every call."""
        _check(self._L.rr_ctx_set_options(self._ctx, flags))

    def debug_fail_second(self):
        """Test hook: the next pipeline call launches only its first kernel and fails."""
        _check(self._L.rr_debug_fail_second(self._ctx))

    def debug_one_help(self):
        """Test hook: the next one-launch decode sums every earlier window itself (the look-back's
        help for windows whose workgroups have not started)."""
        _check(self._L.rr_debug_one_help(self._ctx))

    def reserve(self, n: int, nbytes: int = 0):
        _check(self._L.rr_ctx_reserve(self._ctx, n, nbytes))

    # ---- host entry points ------------------------------------------------------------
    def decode_host(self, data: np.ndarray, offsets: np.ndarray, elem_cap: int | None = None):
        n = len(offsets) - 1
        nbytes = int(offsets[-1])
        if elem_cap is None:
            elem_cap = elem_bound(n, nbytes)
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        values = np.zeros(n, VALUE_DT)
        elems = np.zeros(max(elem_cap, 1), ELEM_DT)
        arena = np.zeros(max(nbytes, 1), np.uint8)
        t = Totals()
        _check(self._L.rr_decode_batch_host(self._ctx, _ptr(data), _ptr(offsets), n, _ptr(values), _ptr(elems),
                                            elem_cap, _ptr(arena), C.byref(t)))
        ne = min(int(t.n_elems), elem_cap)
        return values, elems[:ne], arena[:nbytes], t.as_dict()

    def encode_host(self, values: np.ndarray, elems: np.ndarray, arena: np.ndarray, data_cap: int | None = None):
        n = len(values)
        values = np.ascontiguousarray(values, VALUE_DT)
        elems = np.ascontiguousarray(elems, ELEM_DT)
        arena = np.ascontiguousarray(arena, np.uint8)
        if data_cap is None:
            data_cap = encode_bound(values, elems)
        data = np.zeros(max(data_cap, 1), np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        t = Totals()
        _check(self._L.rr_encode_batch_host(self._ctx, _ptr(values), _ptr(elems), len(elems), _ptr(arena),
                                            arena.size, n, _ptr(data), data_cap, _ptr(offsets), C.byref(t)))
        return data[:int(offsets[-1])], offsets, t.as_dict()

    # ---- device entry points (torch tensors on the engine's device) ----------------------
    def decode_device(self, data, offsets, values, elems, arena, totals, stream=None):
        """All arguments are torch CUDA tensors; no host sync.  stream: torch stream or None."""
        n = offsets.numel() - 1
        inb = BlobBatch(data.data_ptr(), offsets.data_ptr(), n, data.numel())
        outb = FlatBatch(values.data_ptr(), elems.data_ptr(), arena.data_ptr(), n, elems.numel() // 16,
                         arena.numel())
        s = stream.cuda_stream if stream is not None else None
        _check(self._L.rr_decode_batch(self._ctx, C.byref(inb), C.byref(outb), C.c_void_p(totals.data_ptr()),
                                       C.c_void_p(s) if s else None))

    def flat_rebase(self, values, elems, elem_add: int, byte_add: int, stream=None):
        """In place on torch CUDA tensors (uint8 views of the flat records): rr_flat_rebase."""
        _check(self._L.rr_flat_rebase(self._ctx, C.c_void_p(values.data_ptr()), values.numel() // 16,
                                      C.c_void_p(elems.data_ptr()), elems.numel() // 16, elem_add, byte_add,
                                      _sp(stream)))

    def copy_device(self, dst, src, nbytes: int | None = None, stream=None):
        """The engine's streaming copy (rr_copy_device) between torch CUDA tensors."""
        nb = src.numel() * src.element_size() if nbytes is None else nbytes
        _check(self._L.rr_copy_device(self._ctx, C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nb,
                                      _sp(stream)))

    # ---- snappy block compression (include/rr_snappy.h) -----------------------------------
    def snappy_compress_host(self, data: np.ndarray, offsets: np.ndarray):
        """Blocks [offsets[i], offsets[i+1]) of data -> (packed compressed bytes, offsets)."""
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        cap = int(self._L.rr_snappy_compress_bound(n, int(offsets[-1])))
        out = np.zeros(max(cap, 1), np.uint8)
        oo = np.zeros(n + 1, np.uint64)
        _check(self._L.rr_snappy_compress_batch_host(self._ctx, _ptr(data), _ptr(offsets), n, _ptr(out), cap, _ptr(oo)))
        return out[:int(oo[-1])], oo

    def snappy_decompress_host(self, comp: np.ndarray, offsets: np.ndarray, out_cap: int):
        """(out bytes, out offsets, per-block status) of snappy blocks."""
        comp = np.ascontiguousarray(comp, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros(max(out_cap, 1), np.uint8)
        oo = np.zeros(n + 1, np.uint64)
        st = np.zeros(max(n, 1), np.uint8)
        _check(self._L.rr_snappy_decompress_batch_host(self._ctx, _ptr(comp), _ptr(offsets), n, _ptr(out), out_cap,
                                                       _ptr(oo), _ptr(st)))
        return out[:int(oo[-1])], oo, st[:n]

    def snappy_compress_device(self, data, offsets, out, out_offsets, stream=None):
        n = offsets.numel() - 1
        inb = BlobBatch(data.data_ptr(), offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(out.data_ptr(), out_offsets.data_ptr(), n, out.numel())
        _check(self._L.rr_snappy_compress_batch(self._ctx, C.byref(inb), C.byref(outb), _sp(stream)))

    def snappy_decompress_device(self, comp, offsets, out, out_offsets, status, stream=None):
        n = offsets.numel() - 1
        inb = BlobBatch(comp.data_ptr(), offsets.data_ptr(), n, comp.numel())
        outb = BlobBatch(out.data_ptr(), out_offsets.data_ptr(), n, out.numel())
        _check(self._L.rr_snappy_decompress_batch(self._ctx, C.byref(inb), C.byref(outb),
                                                  C.c_void_p(status.data_ptr()), _sp(stream)))

    # ---- LZ4 block compression (include/rr_lz4.h) -----------------------------------------
    def lz4_compress_host(self, data: np.ndarray, offsets: np.ndarray):
        """Blocks [offsets[i], offsets[i+1]) of data -> (packed compressed bytes, offsets)."""
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        cap = int(self._L.rr_lz4_compress_bound(n, int(offsets[-1])))
        out = np.zeros(max(cap, 1), np.uint8)
        oo = np.zeros(n + 1, np.uint64)
        _check(self._L.rr_lz4_compress_batch_host(self._ctx, _ptr(data), _ptr(offsets), n, _ptr(out), cap, _ptr(oo)))
        return out[:int(oo[-1])], oo

    def lz4_decompress_host(self, comp: np.ndarray, offsets: np.ndarray, out_cap: int):
        """(out bytes, out offsets, per-block status) of LZ4 blocks."""
        comp = np.ascontiguousarray(comp, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        out = np.zeros(max(out_cap, 1), np.uint8)
        oo = np.zeros(n + 1, np.uint64)
        st = np.zeros(max(n, 1), np.uint8)
        _check(self._L.rr_lz4_decompress_batch_host(self._ctx, _ptr(comp), _ptr(offsets), n, _ptr(out), out_cap,
                                                       _ptr(oo), _ptr(st)))
        return out[:int(oo[-1])], oo, st[:n]

    def lz4_compress_device(self, data, offsets, out, out_offsets, stream=None):
        n = offsets.numel() - 1
        inb = BlobBatch(data.data_ptr(), offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(out.data_ptr(), out_offsets.data_ptr(), n, out.numel())
        _check(self._L.rr_lz4_compress_batch(self._ctx, C.byref(inb), C.byref(outb), _sp(stream)))

    def lz4_decompress_device(self, comp, offsets, out, out_offsets, status, stream=None):
        n = offsets.numel() - 1
        inb = BlobBatch(comp.data_ptr(), offsets.data_ptr(), n, comp.numel())
        outb = BlobBatch(out.data_ptr(), out_offsets.data_ptr(), n, out.numel())
        _check(self._L.rr_lz4_decompress_batch(self._ctx, C.byref(inb), C.byref(outb),
                                                  C.c_void_p(status.data_ptr()), _sp(stream)))

    # ---- RDB value payloads (include/rr_rdbsave.h) -----------------------------------------
    def rdbsave_host(self, values: np.ndarray, elems: np.ndarray, arena: np.ndarray, list_fill: int = -2,
                     data_cap: int | None = None, lzf: bool = False, flags: int | None = None):
        """Flat batch -> (types, data, offsets, status, totals): the bytes rdbSaveObject writes per value.
        lzf: RR_RDBSAVE_LZF (`rdbcompression yes`); flags, when given, is the options' word as it is."""
        n = len(values)
        values = np.ascontiguousarray(values, VALUE_DT)
        elems = np.ascontiguousarray(elems, ELEM_DT)
        arena = np.ascontiguousarray(arena, np.uint8)
        if data_cap is None:
            data_cap = rdbsave_bound(values, elems)
        data = np.zeros(max(data_cap, 1), np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        types = np.zeros(max(n, 1), np.uint8)
        status = np.zeros(max(n, 1), np.uint8)
        t = Totals()
        opts = RdbSaveOpts(list_fill, (RDBSAVE_LZF if lzf else 0) if flags is None else flags)
        _check(self._L.rr_rdbsave_batch_host(self._ctx, _ptr(values), _ptr(elems), len(elems), _ptr(arena), arena.size,
                                             n, C.byref(opts), _ptr(data), data_cap, _ptr(offsets), _ptr(types),
                                             _ptr(status), C.byref(t)))
        return types[:n], data[:min(int(offsets[-1]), data_cap)], offsets, status[:n], t.as_dict()

    def rdbsave_device(self, values, elems, arena, out_data, out_offsets, types, status, totals, list_fill: int = -2,
                       stream=None, lzf: bool = False, flags: int | None = None):
        """rr_rdbsave_batch on torch CUDA tensors (uint8 views of the flat records); no host sync.
        lzf: RR_RDBSAVE_LZF (`rdbcompression yes`); flags, when given, is the options' word as it is."""
        n = out_offsets.numel() - 1
        inb = FlatBatch(values.data_ptr(), elems.data_ptr(), arena.data_ptr(), n, elems.numel() // 16, arena.numel())
        outb = BlobBatch(out_data.data_ptr(), out_offsets.data_ptr(), n, out_data.numel())
        opts = RdbSaveOpts(list_fill, (RDBSAVE_LZF if lzf else 0) if flags is None else flags)
        _check(self._L.rr_rdbsave_batch(self._ctx, C.byref(inb), C.byref(outb), C.c_void_p(types.data_ptr()),
                                        C.c_void_p(status.data_ptr()), C.c_void_p(totals.data_ptr()), C.byref(opts),
                                        _sp(stream)))

    # ---- RDB value payloads -> rock blobs (include/rr_rdbload.h) --------------------------------
    def rdbload_host(self, data: np.ndarray, offsets: np.ndarray, types: np.ndarray, opts: RdbLoadOpts | None = None,
                     out_cap: int | None = None):
        """RDB payloads -> (blob data, offsets, status, totals): the blob desObject turns into the object
        rdbLoadObject builds.  out_cap None: asks for the size first (a call with out_cap 0)."""
        n = len(offsets) - 1
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        types = np.ascontiguousarray(types, np.uint8)
        out_offsets = np.zeros(n + 1, np.uint64)
        status = np.zeros(max(n, 1), np.uint8)
        t = Totals()
        po = C.byref(opts) if opts is not None else None
        if out_cap is None:
            _check(self._L.rr_rdbload_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), n, po, None, 0,
                                                 _ptr(out_offsets), _ptr(status), C.byref(t)))
            out_cap = int(out_offsets[-1])
        out = np.zeros(max(out_cap, 1), np.uint8)
        _check(self._L.rr_rdbload_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), n, po, _ptr(out), out_cap,
                                             _ptr(out_offsets), _ptr(status), C.byref(t)))
        return out[:min(int(out_offsets[-1]), out_cap)], out_offsets, status[:n], t.as_dict()

    def rdbload(self, data, offsets, types, out_data, out_offsets, status, totals, opts: RdbLoadOpts | None = None,
                stream=None):
        """rr_rdbload_batch on torch CUDA tensors; no host sync.  out_data may be empty (sizes only)."""
        n = out_offsets.numel() - 1
        inb = BlobBatch(data.data_ptr() if data.numel() else None, offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(out_data.data_ptr() if out_data.numel() else None, out_offsets.data_ptr(), n, out_data.numel())
        _check(self._L.rr_rdbload_batch(self._ctx, C.byref(inb), C.c_void_p(types.data_ptr()), C.byref(outb),
                                        C.c_void_p(status.data_ptr()), C.c_void_p(totals.data_ptr()),
                                        C.byref(opts) if opts is not None else None, _sp(stream)))

    # ---- the encodings rdbLoadObject picks for RDBLOAD_E_CONVERT values (include/rr_rdbconvert.h) ----
    def rdbconvert_host(self, data: np.ndarray, offsets: np.ndarray, types: np.ndarray, load_status: np.ndarray,
                        opts: RdbLoadOpts | None = None, out_cap: int | None = None):
        """RDB payloads and rdbload's status -> (blob data, offsets, out_types, status, totals): the blobs of
        the values rdbload left with RDBLOAD_E_CONVERT.  out_cap None: asks for the size first."""
        n = len(offsets) - 1
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        types = np.ascontiguousarray(types, np.uint8)
        load_status = np.ascontiguousarray(load_status, np.uint8)
        out_offsets = np.zeros(n + 1, np.uint64)
        out_types = np.zeros(max(n, 1), np.uint8)
        status = np.zeros(max(n, 1), np.uint8)
        t = Totals()
        po = C.byref(opts) if opts is not None else None
        if out_cap is None:
            _check(self._L.rr_rdbconvert_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), _ptr(load_status), n, po,
                                                    None, 0, _ptr(out_offsets), _ptr(out_types), _ptr(status), C.byref(t)))
            out_cap = int(out_offsets[-1])
        out = np.zeros(max(out_cap, 1), np.uint8)
        _check(self._L.rr_rdbconvert_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), _ptr(load_status), n, po,
                                                _ptr(out), out_cap, _ptr(out_offsets), _ptr(out_types), _ptr(status),
                                                C.byref(t)))
        return out[:min(int(out_offsets[-1]), out_cap)], out_offsets, out_types[:n], status[:n], t.as_dict()

    def rdbconvert(self, data, offsets, types, load_status, out_data, out_offsets, out_types, status, totals,
                   opts: RdbLoadOpts | None = None, stream=None):
        """rr_rdbconvert_batch on torch CUDA tensors; no host sync.  out_data may be empty (sizes only)."""
        n = out_offsets.numel() - 1
        inb = BlobBatch(data.data_ptr() if data.numel() else None, offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(out_data.data_ptr() if out_data.numel() else None, out_offsets.data_ptr(), n, out_data.numel())
        _check(self._L.rr_rdbconvert_batch(self._ctx, C.byref(inb), C.c_void_p(types.data_ptr()),
                                           C.c_void_p(load_status.data_ptr()), C.byref(outb), C.c_void_p(out_types.data_ptr()),
                                           C.c_void_p(status.data_ptr()), C.c_void_p(totals.data_ptr()),
                                           C.byref(opts) if opts is not None else None, _sp(stream)))

    # ---- small ZSets with fractional scores (include/rr_d2string.h, include/rr_rdbzset.h) ---------
    def d2string_host(self, bits: np.ndarray, fill: int = 0):
        """rr_d2string_batch_host: the GPU's d2string of the doubles with these bits (uint64) -> (text
        uint8[n, 32], len uint8[n]).  The slots are pre-filled with `fill`; bytes past len keep it."""
        bits = np.ascontiguousarray(bits, np.uint64)
        n = len(bits)
        text = np.full((max(n, 1), D2STRING_SLOT), fill, np.uint8)
        ln = np.zeros(max(n, 1), np.uint8)
        _check(self._L.rr_d2string_batch_host(self._ctx, _ptr(bits), n, _ptr(text), _ptr(ln)))
        return text[:n], ln[:n]

    def d2string(self, bits, text, length, stream=None):
        """rr_d2string_batch on torch CUDA tensors (bits int64[n], text uint8[32 n], length uint8[n]); no host sync."""
        n = bits.numel()
        dp = lambda t: t.data_ptr() if t.numel() else None
        _check(self._L.rr_d2string_batch(self._ctx, dp(bits), n, dp(text), dp(length), _sp(stream)))

    def rdbzset_host(self, data: np.ndarray, offsets: np.ndarray, types: np.ndarray, convert_status: np.ndarray,
                     opts: RdbLoadOpts | None = None, out_cap: int | None = None):
        """RDB payloads and rdbconvert's status -> (blob data, offsets, status, totals): the ZSET_ZIPLIST
        blobs of the ZSET_2 values rdbconvert left with RDBLOAD_E_CONVERT.  out_cap None: asks for the size first."""
        n = len(offsets) - 1
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        types = np.ascontiguousarray(types, np.uint8)
        convert_status = np.ascontiguousarray(convert_status, np.uint8)
        out_offsets = np.zeros(n + 1, np.uint64)
        status = np.zeros(max(n, 1), np.uint8)
        t = Totals()
        po = C.byref(opts) if opts is not None else None
        if out_cap is None:
            _check(self._L.rr_rdbzset_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), _ptr(convert_status), n, po,
                                                 None, 0, _ptr(out_offsets), _ptr(status), C.byref(t)))
            out_cap = int(out_offsets[-1])
        out = np.zeros(max(out_cap, 1), np.uint8)
        _check(self._L.rr_rdbzset_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), _ptr(convert_status), n, po,
                                             _ptr(out), out_cap, _ptr(out_offsets), _ptr(status), C.byref(t)))
        return out[:min(int(out_offsets[-1]), out_cap)], out_offsets, status[:n], t.as_dict()

    def rdbzset(self, data, offsets, types, convert_status, out_data, out_offsets, status, totals,
                opts: RdbLoadOpts | None = None, stream=None):
        """rr_rdbzset_batch on torch CUDA tensors; no host sync.  out_data may be empty (sizes only)."""
        n = out_offsets.numel() - 1
        inb = BlobBatch(data.data_ptr() if data.numel() else None, offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(out_data.data_ptr() if out_data.numel() else None, out_offsets.data_ptr(), n, out_data.numel())
        _check(self._L.rr_rdbzset_batch(self._ctx, C.byref(inb), C.c_void_p(types.data_ptr()),
                                        C.c_void_p(convert_status.data_ptr()), C.byref(outb), C.c_void_p(status.data_ptr()),
                                        C.c_void_p(totals.data_ptr()), C.byref(opts) if opts is not None else None,
                                        _sp(stream)))

    # ---- the three load stages merged into one blob batch (include/rr_rdbloadall.h) ---------------
    def rdbloadall_host(self, data: np.ndarray, offsets: np.ndarray, types: np.ndarray, opts: RdbLoadOpts | None = None,
                        out_cap: int | None = None):
        """RDB payloads -> (blob data, offsets, out_types, status, stage_bytes, totals): rdbload, rdbconvert and
        rdbzset merged into one batch.  out_cap None: asks for the size first (a call with out_cap 0)."""
        n = len(offsets) - 1
        data = np.ascontiguousarray(data, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        types = np.ascontiguousarray(types, np.uint8)
        out_offsets = np.zeros(n + 1, np.uint64)
        out_types = np.zeros(max(n, 1), np.uint8)
        status = np.zeros(max(n, 1), np.uint8)
        sb = np.zeros(3, np.uint64)
        t = Totals()
        po = C.byref(opts) if opts is not None else None
        if out_cap is None:
            _check(self._L.rr_rdbloadall_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), n, po, None, 0,
                                                    _ptr(out_offsets), _ptr(out_types), _ptr(status), _ptr(sb), C.byref(t)))
            out_cap = int(out_offsets[-1])
        out = np.zeros(max(out_cap, 1), np.uint8)
        _check(self._L.rr_rdbloadall_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), n, po, _ptr(out), out_cap,
                                                _ptr(out_offsets), _ptr(out_types), _ptr(status), _ptr(sb), C.byref(t)))
        return out[:min(int(out_offsets[-1]), out_cap)], out_offsets, out_types[:n], status[:n], sb, t.as_dict()

    def rdbmerge(self, stage1, stage2, stage3, conv_types, types, out_data, out_offsets, out_types, status, totals, stream=None):
        """rr_rdbmerge_batch on torch CUDA tensors; no host sync.  stage1 / stage2 / stage3: (data, offsets, status)
        of rdbload, rdbconvert and rdbzset for the same values; out_data may be empty (sizes only), out_types None."""
        n = out_offsets.numel() - 1
        dp = lambda t: t.data_ptr() if t is not None and t.numel() else None
        bs = [BlobBatch(dp(d), o.data_ptr(), n, d.numel()) for d, o, _ in (stage1, stage2, stage3)]
        outb = BlobBatch(dp(out_data), out_offsets.data_ptr(), n, out_data.numel())
        _check(self._L.rr_rdbmerge_batch(self._ctx, C.byref(bs[0]), dp(stage1[2]), C.byref(bs[1]), dp(stage2[2]), dp(conv_types),
                                         C.byref(bs[2]), dp(stage3[2]), dp(types), C.byref(outb), dp(out_types), dp(status),
                                         C.c_void_p(totals.data_ptr()), _sp(stream)))

    def rdbloadall(self, data, offsets, types, ws, stage_cap, out_data, out_offsets, out_types, status, stage_bytes, totals,
                   opts: RdbLoadOpts | None = None, stream=None, ws_bytes: int | None = None):
        """rr_rdbloadall_batch on torch CUDA tensors; no host sync.  ws: a uint8 workspace of rdbloadall_ws_bytes(n,
        stage_cap) bytes; stage_cap: three ints (all zero: the sizing run); stage_bytes: int64[3]."""
        n = out_offsets.numel() - 1
        dp = lambda t: t.data_ptr() if t is not None and t.numel() else None
        inb = BlobBatch(dp(data), offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(dp(out_data), out_offsets.data_ptr(), n, out_data.numel())
        caps = (C.c_uint64 * 3)(*[int(x) for x in stage_cap])
        _check(self._L.rr_rdbloadall_batch(self._ctx, C.byref(inb), dp(types), C.c_void_p(ws.data_ptr()),
                                           ws.numel() if ws_bytes is None else ws_bytes, caps, C.byref(outb), dp(out_types),
                                           dp(status), C.c_void_p(stage_bytes.data_ptr()), C.c_void_p(totals.data_ptr()),
                                           C.byref(opts) if opts is not None else None, _sp(stream)))

    # ---- AOF rewrite commands (include/rr_aof.h) --------------------------------------------------
    def aof_host(self, values: np.ndarray, elems: np.ndarray, arena: np.ndarray, key_data, key_offsets, expires=None,
                 data_cap: int | None = None, key_bytes: int | None = None):
        """Flat batch and keys -> (data, offsets, status, totals): the commands rewriteAppendOnlyFileRio writes
        per value.  expires: ms, -1 none (None: no value has one).  data_cap None: asks for the size first."""
        n = len(values)
        values = np.ascontiguousarray(values, VALUE_DT)
        elems = np.ascontiguousarray(elems, ELEM_DT)
        arena = np.ascontiguousarray(arena, np.uint8)
        key_data = np.ascontiguousarray(key_data, np.uint8)
        key_offsets = np.ascontiguousarray(key_offsets, np.uint64)
        expires = None if expires is None else np.ascontiguousarray(expires, np.int64)
        kb = key_data.size if key_bytes is None else key_bytes
        offsets = np.zeros(n + 1, np.uint64)
        status = np.zeros(max(n, 1), np.uint8)
        t = Totals()

        def call(data, cap):
            _check(self._L.rr_aof_batch_host(self._ctx, _ptr(values), _ptr(elems), len(elems), _ptr(arena), arena.size, n,
                                             _ptr(key_data), _ptr(key_offsets), kb, _ptr(expires) if expires is not None else None,
                                             _ptr(data) if data is not None else None, cap, _ptr(offsets), _ptr(status),
                                             C.byref(t)))
        if data_cap is None:
            call(None, 0)
            data_cap = int(offsets[-1])
        data = np.zeros(max(data_cap, 1), np.uint8)
        call(data, data_cap)
        return data[:min(int(offsets[-1]), data_cap)], offsets, status[:n], t.as_dict()

    def aof(self, values, elems, arena, key_data, key_offsets, out_data, out_offsets, status, totals, expires=None,
            stream=None, key_cap: int | None = None, out_cap: int | None = None):
        """rr_aof_batch on torch CUDA tensors (uint8 views of the flat records; expires int64 or None); no
        host sync.  out_data may be empty (sizes only); *_cap default to the tensors' sizes."""
        n = out_offsets.numel() - 1
        dp = lambda t: t.data_ptr() if t is not None and t.numel() else None
        inb = FlatBatch(values.data_ptr(), elems.data_ptr(), arena.data_ptr(), n, elems.numel() // 16, arena.numel())
        kb = BlobBatch(dp(key_data), key_offsets.data_ptr(), n, key_data.numel() if key_cap is None else key_cap)
        outb = BlobBatch(dp(out_data), out_offsets.data_ptr(), n, out_data.numel() if out_cap is None else out_cap)
        _check(self._L.rr_aof_batch(self._ctx, C.byref(inb), C.byref(kb), dp(expires), C.byref(outb), dp(status),
                                    C.c_void_p(totals.data_ptr()), _sp(stream)))

    # ---- RDB streams and DUMP payloads with their CRC-64 (include/rr_rdbfile.h) -------------------
    def rdbfile_section(self, pay_data, pay_offsets, types, status, key_data, key_offsets, out, rec_offsets, rec_status,
                        state, result, expires=None, idle=None, freq=None, head=None, flags: int = 0, stream=None,
                        out_cap: int | None = None, key_cap: int | None = None, pay_cap: int | None = None):
        """rr_rdbfile_section on torch CUDA tensors; no host sync.  state: int64[2] (checksum in and out,
        section bytes), result: uint8[24] (rr_rdbfile_result).  *_cap default to the tensors' sizes."""
        n = _n_offsets(pay_offsets)
        dp = lambda t: t.data_ptr() if t is not None and t.numel() else None
        arg = RdbFileIn(BlobBatch(dp(pay_data), pay_offsets.data_ptr(), n, pay_data.numel() if pay_cap is None else pay_cap),
                        BlobBatch(dp(key_data), key_offsets.data_ptr(), n, key_data.numel() if key_cap is None else key_cap),
                        dp(types), dp(status), dp(expires), dp(idle), dp(freq), dp(head),
                        head.numel() if head is not None else 0)
        _check(self._L.rr_rdbfile_section(self._ctx, C.byref(arg), flags, dp(out), out.numel() if out_cap is None else out_cap,
                                          rec_offsets.data_ptr(), dp(rec_status), state.data_ptr(), result.data_ptr(),
                                          _sp(stream)))

    def rdbfile_section_host(self, pay_data, pay_offsets, types, status, key_data, key_offsets, expires=None, idle=None,
                             freq=None, head: bytes = b"", flags: int = 0, crc_in: int = 0, out_cap: int | None = None):
        """rr_rdbfile_section_host over numpy arrays: (section bytes, rec_offsets, rec_status, checksum out,
        result dict).  out_cap None: rr_rdbfile_bound."""
        n = len(pay_offsets) - 1
        pay_data, key_data = np.ascontiguousarray(pay_data, np.uint8), np.ascontiguousarray(key_data, np.uint8)
        pay_offsets, key_offsets = np.ascontiguousarray(pay_offsets, np.uint64), np.ascontiguousarray(key_offsets, np.uint64)
        types, status = np.ascontiguousarray(types, np.uint8), np.ascontiguousarray(status, np.uint8)
        expires = None if expires is None else np.ascontiguousarray(expires, np.int64)
        idle = None if idle is None else np.ascontiguousarray(idle, np.uint64)
        freq = None if freq is None else np.ascontiguousarray(freq, np.uint8)
        hd = np.frombuffer(bytes(head), np.uint8)
        if out_cap is None:
            out_cap = rdbfile_bound(n, key_data.size, pay_data.size, len(hd))
        out = np.zeros(max(out_cap, 1), np.uint8)
        ro, rs = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8)
        st = np.array([crc_in, 0], np.uint64)
        res = RdbFileResult()
        arg = RdbFileIn(BlobBatch(_ptr(pay_data), _ptr(pay_offsets), n, pay_data.size),
                        BlobBatch(_ptr(key_data), _ptr(key_offsets), n, key_data.size), _ptr(types), _ptr(status),
                        _ptr(expires), _ptr(idle), _ptr(freq), _ptr(hd), len(hd))
        _check(self._L.rr_rdbfile_section_host(self._ctx, C.byref(arg), flags, _ptr(out), out_cap, _ptr(ro), _ptr(rs),
                                               _ptr(st), C.byref(res)))
        nb = int(res.bytes) if res.status == 0 else 0
        return out[:nb], ro, rs[:n], int(st[0]), res.as_dict()

    def crc64_device(self, data, nbytes: int, state, stream=None):
        """state[0] = crc64(state[0], data[:nbytes]) on the device (torch CUDA tensors; state int64[2])."""
        _check(self._L.rr_crc64_device(self._ctx, data.data_ptr() if nbytes else None, nbytes, state.data_ptr(), _sp(stream)))

    def rdbdump(self, data, offsets, types, status, out, out_offsets, out_status, result, stream=None,
                out_cap: int | None = None):
        """rr_rdbdump_batch on torch CUDA tensors; no host sync."""
        n = _n_offsets(offsets)
        dp = lambda t: t.data_ptr() if t.numel() else None
        inb = BlobBatch(dp(data), offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(dp(out), out_offsets.data_ptr(), n, out.numel() if out_cap is None else out_cap)
        _check(self._L.rr_rdbdump_batch(self._ctx, C.byref(inb), dp(types), dp(status), C.byref(outb), dp(out_status),
                                        result.data_ptr(), _sp(stream)))

    def rdbdump_host(self, data, offsets, types, status, out_cap: int | None = None):
        """Payloads -> (DUMP bytes, offsets, status, result dict)."""
        n = len(offsets) - 1
        data, offsets = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(offsets, np.uint64)
        types, status = np.ascontiguousarray(types, np.uint8), np.ascontiguousarray(status, np.uint8)
        if out_cap is None:
            out_cap = data.size + 11 * n
        out = np.zeros(max(out_cap, 1), np.uint8)
        oo, os_ = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8)
        res = RdbFileResult()
        _check(self._L.rr_rdbdump_batch_host(self._ctx, _ptr(data), _ptr(offsets), _ptr(types), _ptr(status), n, _ptr(out),
                                             out_cap, _ptr(oo), _ptr(os_), C.byref(res)))
        return out[:min(int(oo[-1]), out_cap)], oo, os_[:n], res.as_dict()

    def rdbdump_verify(self, data, offsets, out, out_offsets, types, status, result, stream=None):
        """rr_rdbdump_verify_batch on torch CUDA tensors; no host sync.  out may be empty (sizes only)."""
        n = _n_offsets(offsets)
        dp = lambda t: t.data_ptr() if t.numel() else None
        inb = BlobBatch(dp(data), offsets.data_ptr(), n, data.numel())
        outb = BlobBatch(dp(out), out_offsets.data_ptr(), n, out.numel())
        _check(self._L.rr_rdbdump_verify_batch(self._ctx, C.byref(inb), C.byref(outb), dp(types), dp(status),
                                               result.data_ptr(), _sp(stream)))

    def rdbdump_verify_host(self, data, offsets, out_cap: int | None = None):
        """DUMP payloads -> (payload bytes, offsets, types, status, result dict)."""
        n = len(offsets) - 1
        data, offsets = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(offsets, np.uint64)
        if out_cap is None:
            out_cap = data.size
        out = np.zeros(max(out_cap, 1), np.uint8)
        oo, ty, st = np.zeros(n + 1, np.uint64), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        res = RdbFileResult()
        _check(self._L.rr_rdbdump_verify_batch_host(self._ctx, _ptr(data), _ptr(offsets), n, _ptr(out), out_cap, _ptr(oo),
                                                    _ptr(ty), _ptr(st), C.byref(res)))
        return out[:min(int(oo[-1]), out_cap)], oo, ty[:n], st[:n], res.as_dict()

    # ---- reading a complete RDB stream (include/rr_rdbread.h) ---------------------------------------
    def rdbread_split(self, data, rec_start, rec_end, version: int, key_data, key_offsets, pay_data, pay_offsets, types,
                      expires, idle, freq, status, result, stream=None, data_cap: int | None = None,
                      key_cap: int | None = None, pay_cap: int | None = None):
        """rr_rdbread_split on torch CUDA tensors; no host sync.  rec_start / rec_end: int64[n] (rr_rdbread_index's);
        expires / idle: int64[n], freq: int16[n], result: uint8[24].  key_data / pay_data may be empty (sizes only);
        *_cap default to the tensors' sizes."""
        n = _n_offsets(key_offsets)
        dp = lambda t: t.data_ptr() if t is not None and t.numel() else None
        out = RdbReadOut(BlobBatch(dp(key_data), key_offsets.data_ptr(), n, key_data.numel() if key_cap is None else key_cap),
                         BlobBatch(dp(pay_data), pay_offsets.data_ptr(), n, pay_data.numel() if pay_cap is None else pay_cap),
                         dp(types), dp(expires), dp(idle), dp(freq), dp(status))
        _check(self._L.rr_rdbread_split(self._ctx, dp(data), data.numel() if data_cap is None else data_cap, dp(rec_start),
                                        dp(rec_end), n, version, C.byref(out), result.data_ptr(), _sp(stream)))

    def rdbread_split_host(self, data, rec_start, rec_end, version: int, key_cap: int | None = None, pay_cap: int | None = None):
        """rr_rdbread_split_host over numpy arrays: dict(key_data, key_offsets, pay_data, pay_offsets, types, expires,
        idle, freq, status, result).  A cap of None: asks for the sizes first (a call with both caps 0)."""
        data = np.ascontiguousarray(data, np.uint8)
        rs, re_ = np.ascontiguousarray(rec_start, np.uint64), np.ascontiguousarray(rec_end, np.uint64)
        n = len(rs)
        ko, po = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        m = max(n, 1)
        ty, st = np.zeros(m, np.uint8), np.zeros(m, np.uint8)
        ex, idl, fq = np.zeros(m, np.int64), np.zeros(m, np.uint64), np.zeros(m, np.int16)
        res = RdbFileResult()

        def call(kd, kc, pd, pc):
            out = RdbReadOut(BlobBatch(_ptr(kd) if kc else None, _ptr(ko), n, kc), BlobBatch(_ptr(pd) if pc else None, _ptr(po), n, pc),
                             _ptr(ty), _ptr(ex), _ptr(idl), _ptr(fq), _ptr(st))
            _check(self._L.rr_rdbread_split_host(self._ctx, _ptr(data), data.size, _ptr(rs), _ptr(re_), n, version, C.byref(out),
                                                 C.byref(res)))

        if key_cap is None or pay_cap is None:
            call(None, 0, None, 0)
            key_cap = int(ko[-1]) if key_cap is None else key_cap
            pay_cap = int(po[-1]) if pay_cap is None else pay_cap
        kd, pd = np.zeros(max(key_cap, 1), np.uint8), np.zeros(max(pay_cap, 1), np.uint8)
        call(kd, key_cap, pd, pay_cap)
        return dict(key_data=kd[:min(int(ko[-1]), key_cap)], key_offsets=ko, pay_data=pd[:min(int(po[-1]), pay_cap)],
                    pay_offsets=po, types=ty[:n], expires=ex[:n], idle=idl[:n], freq=fq[:n], status=st[:n], result=res.as_dict())

    def rdbread_verify(self, data, eof_at: int, state, result, stream=None, data_cap: int | None = None):
        """rr_rdbread_verify on torch CUDA tensors; no host sync.  state: int64[2] (checksum in and out, the bytes
        summed), result: uint8[24] (status: 0, RDBDUMP_E_CRC or RDBREAD_NO_CKSUM)."""
        _check(self._L.rr_rdbread_verify(self._ctx, data.data_ptr(), data.numel() if data_cap is None else data_cap, eof_at,
                                         state.data_ptr(), result.data_ptr(), _sp(stream)))

    def rdbread_verify_host(self, data, eof_at: int, crc_in: int = 0):
        """rr_rdbread_verify_host over a numpy array: (verdict, the computed checksum)."""
        data = np.ascontiguousarray(data, np.uint8)
        st = np.array([crc_in, 0], np.uint64)
        res = RdbFileResult()
        _check(self._L.rr_rdbread_verify_host(self._ctx, _ptr(data), data.size, eof_at, _ptr(st), C.byref(res)))
        return int(res.status), int(st[0])

    def encode_device(self, values, elems, arena, out_data, out_offsets, totals, stream=None):
        n = out_offsets.numel() - 1
        inb = FlatBatch(values.data_ptr(), elems.data_ptr(), arena.data_ptr(), n, elems.numel() // 16,
                        arena.numel())
        outb = BlobBatch(out_data.data_ptr(), out_offsets.data_ptr(), n, out_data.numel())
        s = stream.cuda_stream if stream is not None else None
        _check(self._L.rr_encode_batch(self._ctx, C.byref(inb), C.byref(outb), C.c_void_p(totals.data_ptr()),
                                       C.c_void_p(s) if s else None))


class Comm:
    """An RCCL communicator over one engine's device (include/rr_serdes.h multi-GPU calls).
    Every rank builds one with the same 128-byte id (``Comm.new_id()`` on one rank, handed to
    the others by any means).  Device arguments are torch CUDA tensors."""

    def __init__(self, engine: Engine, nranks: int, rank: int, cid: bytes):
        self._L = lib()
        self.nranks, self.rank = nranks, rank
        self._c = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(cid)
        _check(self._L.rr_comm_init(engine._ctx, nranks, rank, buf, C.byref(self._c)))

    @staticmethod
    def new_id() -> bytes:
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        _check(lib().rr_comm_get_id(buf))
        return bytes(buf)

    def close(self):
        if self._c:
            self._L.rr_comm_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def split_plan(self, data=None, offsets=None, root=0, stream=None):
        whole = BlobBatch(data.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, data.numel()) \
            if offsets is not None else BlobBatch()
        plan = (Shard * self.nranks)()
        _check(self._L.rr_split_plan(self._c, C.byref(whole), root, plan, _sp(stream)))
        return plan

    def split(self, plan, data, offsets, mine_data, mine_offsets, root=0, stream=None):
        whole = BlobBatch(data.data_ptr(), offsets.data_ptr(), offsets.numel() - 1, data.numel()) \
            if offsets is not None else BlobBatch()
        mine = BlobBatch(mine_data.data_ptr(), mine_offsets.data_ptr(), 0, mine_data.numel())
        _check(self._L.rr_split(self._c, C.byref(whole), plan, root, C.byref(mine), _sp(stream)))
        return int(mine.n)

    def gather(self, plan, values, elems, mine_elems, whole_values=None, whole_elems=None, root=0, stream=None):
        mine = FlatBatch(values.data_ptr(), elems.data_ptr(), None, values.numel() // 16, elems.numel() // 16, 0)
        whole = FlatBatch(whole_values.data_ptr(), whole_elems.data_ptr(), None, whole_values.numel() // 16,
                          whole_elems.numel() // 16, 0) if whole_values is not None else FlatBatch()
        _check(self._L.rr_gather(self._c, C.byref(mine), mine_elems, plan, root, C.byref(whole), _sp(stream)))


def _n_offsets(t) -> int:
    """The values of an offsets tensor of n + 1 u64 words, whatever dtype it is viewed as."""
    return t.numel() * t.element_size() // 8 - 1


def _sp(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def encode_bound(values: np.ndarray, elems: np.ndarray) -> int:
    """Upper bound on encoded bytes for a flat batch (decimal ints <= 20 chars + 4-byte prefix;
    every other element costs <= 16 + len)."""
    return int(len(values) * 13 + len(elems) * 24 + int(elems["len"].astype(np.uint64).sum()) + 16)


def rdbsave_bound(values: np.ndarray, elems: np.ndarray) -> int:
    """rr_rdbsave_bound of a flat batch: an upper bound on the bytes rdbsave writes for it."""
    pay = int(elems["len"][(elems["kind"] == K_STR) | (elems["kind"] == K_ZLRAW)].astype(np.uint64).sum())
    return int(lib().rr_rdbsave_bound(len(values), len(elems), pay))


def rdbload_bound(n: int, payload_bytes: int) -> int:
    """rr_rdbload_bound: an upper bound on the blob bytes of n payloads without LZF strings."""
    return int(lib().rr_rdbload_bound(n, payload_bytes))


def d2string(v: float) -> bytes:
    """rr_d2string: the reference's d2string of v (the host twin of the GPU's printer)."""
    buf = C.create_string_buffer(D2STRING_MAX)
    n = lib().rr_d2string(buf, float(v))
    return buf.raw[:n]


def aof_bound(n: int, n_elems: int, payload_bytes: int, key_bytes: int) -> int:
    """rr_aof_bound: an upper bound on a batch's command bytes (include/rr_aof.h)."""
    return int(lib().rr_aof_bound(n, n_elems, payload_bytes, key_bytes))


def aof_select(dbi: int) -> bytes:
    """rr_aof_select: the SELECT command rewriteAppendOnlyFileRio writes in front of db dbi."""
    buf = C.create_string_buffer(48)
    n = lib().rr_aof_select(buf, 48, dbi)
    if n <= 0:
        raise RRError(f"rr_aof_select({dbi}) failed")
    return buf.raw[:n]


def aof_score_text(text: bytes):
    """rr_aof_score_text: %.17g of the score a ziplist string entry holds, or None for a text that is not taken."""
    buf = C.create_string_buffer(32)
    n = lib().rr_aof_score_text(buf, bytes(text), len(text))
    return None if n < 0 else buf.raw[:n]


def rdbzset_bound(n: int, payload_bytes: int) -> int:
    """rr_rdbzset_bound: an upper bound on the blob bytes of n ZSET_2 payloads converted with printed scores."""
    return int(lib().rr_rdbzset_bound(n, payload_bytes))


def rdbloadall_caps(n: int, payload_bytes: int) -> tuple[int, int, int]:
    """rr_rdbloadall_caps: the three stages' bounds (rdbload_bound, rdbconvert_bound, rdbzset_bound)."""
    caps = (C.c_uint64 * 3)()
    lib().rr_rdbloadall_caps(n, payload_bytes, caps)
    return int(caps[0]), int(caps[1]), int(caps[2])


def rdbloadall_ws_bytes(n: int, stage_cap) -> int:
    """rr_rdbloadall_ws_bytes: the one call's workspace for n values and these three stage capacities."""
    return int(lib().rr_rdbloadall_ws_bytes(n, (C.c_uint64 * 3)(*[int(x) for x in stage_cap])))


def rdbconvert_bound(n: int, payload_bytes: int) -> int:
    """rr_rdbconvert_bound: an upper bound on the blob bytes of n converted payloads without LZF strings."""
    return int(lib().rr_rdbconvert_bound(n, payload_bytes))


# ---- include/rr_rdbfile.h: the host helpers (no GPU) ---------------------------------------------
def crc64(crc: int, data) -> int:
    """rr_crc64: crc64.c's crc64() over tables generated from the polynomial."""
    b = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    return int(lib().rr_crc64(crc, _ptr(b), b.size))


def crc64_shift(crc: int, n: int) -> int:
    """rr_crc64_shift: crc * x^(8n) mod P, the checksum after n more zero bytes."""
    return int(lib().rr_crc64_shift(crc, n))


def rdbfile_bound(n: int, key_bytes: int, payload_bytes: int, head_bytes: int = 0) -> int:
    return int(lib().rr_rdbfile_bound(n, key_bytes, payload_bytes, head_bytes))


def rdbfile_head(ver: str, ctime: int, used_mem: int, repl=None, aof_preamble: bool = False, cap: int | None = None):
    """rr_rdbfile_head: "REDIS0009" and the aux fields; repl: None or (stream_db, replid, offset).
    cap None: the size first.  Returns (bytes needed, the buffer of cap bytes as the call left it)."""
    r = RdbFileRepl(repl[0], repl[1].encode(), repl[2]) if repl is not None else None
    pr = C.byref(r) if r is not None else None
    L = lib()
    if cap is None:
        cap = int(L.rr_rdbfile_head(None, 0, ver.encode(), ctime, used_mem, pr, int(aof_preamble)))
    buf = np.full(max(cap, 1), 0xA5, np.uint8)
    need = int(L.rr_rdbfile_head(_ptr(buf), cap, ver.encode(), ctime, used_mem, pr, int(aof_preamble)))
    return need, buf[:cap].tobytes()


def rdbfile_selectdb(dbid: int, db_size: int, expires_size: int, cap: int = 32):
    """rr_rdbfile_selectdb: (bytes needed, the buffer of cap bytes as the call left it)."""
    buf = np.full(max(cap, 1), 0xA5, np.uint8)
    need = int(lib().rr_rdbfile_selectdb(_ptr(buf), cap, dbid, db_size, expires_size))
    return need, buf[:cap].tobytes()


# ---- include/rr_rdbread.h: the record index and the host string reader (no GPU) -------------------
def rdbread_index(buf, state: RdbReadState | None = None, max_recs: int | None = None, max_items: int | None = None):
    """rr_rdbread_index over buf from state.pos (a fresh state when None): dict(rc, rec_start, rec_end, rec_db, items
    (RDBREAD_ITEM_DT), eof_at, cksum, has_cksum, err_at, state).  max_* None: room for every byte of buf."""
    b = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, np.uint8)
    st = state if state is not None else RdbReadState()
    max_recs = b.size if max_recs is None else max_recs
    max_items = b.size if max_items is None else max_items
    rs, re_, rd = (np.zeros(max(max_recs, 1), np.uint64) for _ in range(3))
    items = np.zeros(max(max_items, 1), RDBREAD_ITEM_DT)
    res = RdbReadIndexResult()
    rc = int(lib().rr_rdbread_index(C.byref(st), _ptr(b), b.size, _ptr(rs), _ptr(re_), _ptr(rd), max_recs, _ptr(items), max_items,
                                    C.byref(res)))
    if rc < 0:
        raise RRError(f"rr_rdbread_index failed ({rc})")
    nr, ni = int(res.n_recs), int(res.n_items)
    return dict(rc=rc, rec_start=rs[:nr], rec_end=re_[:nr], rec_db=rd[:nr], items=items[:ni], eof_at=int(res.eof_at),
                cksum=int(res.cksum), has_cksum=bool(res.has_cksum), err_at=int(res.err_at), state=st)


def rdbread_string(buf, at: int, out_cap: int | None = None):
    """rr_rdbread_string: (rc, the string's bytes or None, its length, the offset behind it).  out_cap None: the
    length first."""
    b = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, np.uint8)
    ln, end = C.c_uint64(0), C.c_uint64(0)
    L = lib()
    if out_cap is None:
        rc = int(L.rr_rdbread_string(_ptr(b), b.size, at, None, 0, C.byref(ln), C.byref(end)))
        if rc not in (RDBREAD_DONE, E_CAPACITY):
            return rc, None, int(ln.value), int(end.value)
        out_cap = int(ln.value)
    out = np.full(out_cap + 8, 0xA5, np.uint8)
    rc = int(L.rr_rdbread_string(_ptr(b), b.size, at, _ptr(out), out_cap, C.byref(ln), C.byref(end)))
    assert (out[out_cap:] == 0xA5).all()
    if rc != RDBREAD_DONE:
        assert (out == 0xA5).all()
        return rc, None, int(ln.value), int(end.value)
    return rc, out[:int(ln.value)].tobytes(), int(ln.value), int(end.value)


def rdbread_len(buf, at: int):
    """rr_rdbread_len: (rc, the number, the offset behind it)."""
    b = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, np.uint8)
    val, end = C.c_uint64(0), C.c_uint64(0)
    rc = int(lib().rr_rdbread_len(_ptr(b), b.size, at, C.byref(val), C.byref(end)))
    return rc, int(val.value), int(end.value)
