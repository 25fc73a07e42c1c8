"""ctypes binding of include/rhj.h (librhj_hip.so).  No compute happens in Python."""
import contextlib
import ctypes as C
import os

import numpy as np

TUPLE = np.dtype([("key", "<u8"), ("payload", "<u8")])   # rhj_tuple == reference `tuple` (structs.h:33-36)
PAIR = np.dtype([("keyR", "<u8"), ("keyS", "<u8")])      # rhj_pair  == reference `key_tuple` (Result.h:9-12)

RHJ_OK, RHJ_E_INVALID, RHJ_E_NODEVICE, RHJ_E_HIP, RHJ_E_NOMEM, RHJ_E_OVERFLOW = 0, -1, -2, -3, -4, -5
KERNEL_KINDS = ("hist", "scan", "scatter", "tasks", "join", "aux")

_vp, _u64, _i32 = C.c_void_p, C.c_uint64, C.c_int32


class Opts(C.Structure):
    """rhj_opts: passes=-1 auto; bits per pass; probe_split = max probe tuples per join task."""
    _fields_ = [("passes", _i32), ("bits1", _i32), ("bits2", _i32), ("probe_split", _i32)]

    def __init__(self, passes=-1, bits1=0, bits2=0, probe_split=0):
        super().__init__(passes, bits1, bits2, probe_split)

    def __repr__(self):
        return f"Opts(passes={self.passes}, bits1={self.bits1}, bits2={self.bits2}, probe_split={self.probe_split})"


class JoinDesc(C.Structure):
    """rhj_join_desc (include/rhj.h): one join of an rhj_join_batch call"""
    _fields_ = [("R", C.c_void_p), ("nR", C.c_uint64), ("S", C.c_void_p), ("nS", C.c_uint64)]


class Timings(C.Structure):
    _fields_ = [("ms", C.c_double * 6), ("launches", C.c_uint32 * 6), ("total_ms", C.c_double),
                ("passes", _i32), ("bits1", _i32), ("bits2", _i32), ("ntasks", _u64)]

    def as_dict(self):
        d = {k: {"ms": self.ms[i], "launches": self.launches[i]} for i, k in enumerate(KERNEL_KINDS)}
        d.update(total_ms=self.total_ms, passes=self.passes, bits1=self.bits1, bits2=self.bits2, ntasks=self.ntasks)
        return d


class KeysLayout(C.Structure):
    """rhj_keys_layout_t (include/rhj.h): how up to four key columns share one 64-bit word.  kind[j]: KEYS_RANGE / KEYS_DICT of key
    column j; fold f packs the fields fold_a[f] and fold_b[f] (ids 0 .. 3: the columns, KEYS_FOLD0 + f: a fold's output) and
    replaces them by the word's dense id; field i of the final word is field_id[i] at field_shift[i], field_width[i] bits wide."""
    _fields_ = [("nkeys", C.c_uint32), ("kind", C.c_uint32 * 4), ("range_bits", C.c_uint32 * 4), ("wd", C.c_uint32),
                ("nfolds", C.c_uint32), ("fold_a", C.c_uint32 * 2), ("fold_b", C.c_uint32 * 2), ("fold_shift", C.c_uint32 * 2),
                ("nfields", C.c_uint32), ("field_id", C.c_uint32 * 4), ("field_width", C.c_uint32 * 4),
                ("field_shift", C.c_uint32 * 4), ("total_bits", C.c_uint32), ("base", C.c_uint64 * 4),
                ("dict_size", C.c_uint64 * 4), ("fold_size", C.c_uint64 * 2)]

    def as_dict(self):
        k, f, m = self.nkeys, self.nfolds, self.nfields
        return {"nkeys": k, "kind": list(self.kind[:k]), "range_bits": list(self.range_bits[:k]), "wd": self.wd,
                "folds": [(self.fold_a[i], self.fold_b[i]) for i in range(f)], "fold_shift": list(self.fold_shift[:f]),
                "fields": list(self.field_id[:m]), "widths": list(self.field_width[:m]), "shifts": list(self.field_shift[:m]),
                "total_bits": self.total_bits, "base": list(self.base[:k]), "dict_size": list(self.dict_size[:k]),
                "fold_size": list(self.fold_size[:f])}


class RhjError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rhj error {code}: {msg}")
        self.code = code


def lib_path():
    """the in-tree library; RHJ_LIB_PATH names another build of it (development A/B runs: tools/ab/)"""
    return os.environ.get("RHJ_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "librhj_hip.so")


_LIB = None

# every symbol include/rhj.h declares: name -> (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "rhj_abi_version": (C.c_int, []),
    "rhj_device_count": (C.c_int, []),
    "rhj_init": (C.c_int, [C.c_int, _P(_vp)]),
    "rhj_destroy": (None, [_vp]),
    "rhj_last_error": (C.c_char_p, [_vp]),
    "rhj_set_stream": (C.c_int, [_vp, _vp]),
    "rhj_set_profiling": (C.c_int, [_vp, C.c_int]),
    "rhj_set_option": (C.c_int, [_vp, C.c_char_p, C.c_int64]),
    "rhj_get_info": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_int64)]),
    "rhj_get_timings": (C.c_int, [_vp, _P(Timings)]),
    "rhj_get_launch_timings": (C.c_int, [_vp, _P(_i32), _P(C.c_double), C.c_uint32, _P(C.c_uint32)]),
    "rhj_sync": (C.c_int, [_vp]),
    "rhj_reserve": (C.c_int, [_vp, _u64, _u64, _P(Opts)]),
    "rhj_release_workspace": (C.c_int, [_vp]),
    "rhj_default_opts": (None, [_P(Opts)]),
    "rhj_plan": (C.c_int, [_u64, _u64, _P(Opts), _P(Opts)]),
    "rhj_join": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _P(Opts), _P(_vp), _P(_u64)]),
    "rhj_join_batch": (C.c_int, [_vp, C.c_uint32, _P(JoinDesc), _P(_vp), _P(_u64)]),
    "rhj_join_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_join_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_semi_join_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, C.c_int, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_semi_join_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, C.c_int, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_outer_join_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_int, _P(Opts), _vp, _u64, _P(_u64), _P(_u64)]),
    "rhj_outer_join_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, C.c_int, _P(Opts), _vp, _u64, _P(_u64), _P(_u64)]),
    "rhj_join_sum_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _P(_vp), C.c_uint32, _u64, _P(Opts), _P(_u64), _P(_u64)]),
    "rhj_join_sum_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _P(_vp), C.c_uint32, _u64, _P(Opts), _P(_u64), _P(_u64)]),
    "rhj_join_mult_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_join_mult_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _vp, _u64, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_lookup_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_int, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_lookup_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, C.c_int, _P(Opts), _vp, _u64, _P(_u64)]),
    "rhj_group_sum_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _P(_vp), C.c_uint32, _u64, _P(Opts), _vp, _vp, _P(_vp), _u64, _P(_u64)]),
    "rhj_group_sum_dev": (C.c_int, [_vp, _vp, _u64, _P(_vp), C.c_uint32, _u64, _P(Opts), _vp, _vp, _P(_vp), _u64, _P(_u64)]),
    "rhj_group_join_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _P(_vp), C.c_uint32, _u64, _P(_vp), C.c_uint32, _u64, C.c_int,
                                          _P(Opts), _vp, _vp, _vp, _P(_vp), _P(_vp), _u64, _P(_u64)]),
    "rhj_group_join_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _P(_vp), C.c_uint32, _u64, _P(_vp), C.c_uint32, _u64, C.c_int,
                                     _P(Opts), _vp, _vp, _vp, _P(_vp), _P(_vp), _u64, _P(_u64)]),
    "rhj_group_agg_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(Opts), _vp, _vp, _P(_vp), _u64,
                                         _P(_u64)]),
    "rhj_group_agg_dev": (C.c_int, [_vp, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(Opts), _vp, _vp, _P(_vp), _u64, _P(_u64)]),
    "rhj_group_join_agg_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(_vp),
                                              _P(C.c_uint32), C.c_uint32, _u64, C.c_int, _P(Opts), _vp, _vp, _vp, _P(_vp), _P(_vp), _u64,
                                              _P(_u64)]),
    "rhj_group_join_agg_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(_vp), _P(C.c_uint32),
                                         C.c_uint32, _u64, C.c_int, _P(Opts), _vp, _vp, _vp, _P(_vp), _P(_vp), _u64, _P(_u64)]),
    "rhj_group_agg_ids_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(Opts), _vp, _vp, _P(_vp),
                                             _u64, _P(_u64), _vp, _u64]),
    "rhj_group_agg_ids_dev": (C.c_int, [_vp, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(Opts), _vp, _vp, _P(_vp), _u64,
                                        _P(_u64), _vp, _u64]),
    "rhj_group_join_agg_ids_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(_vp),
                                                  _P(C.c_uint32), C.c_uint32, _u64, C.c_int, _P(Opts), _vp, _vp, _vp, _P(_vp), _P(_vp),
                                                  _u64, _P(_u64), _vp, _u64, _vp, _u64]),
    "rhj_group_join_agg_ids_dev": (C.c_int, [_vp, _vp, _u64, _vp, _u64, _P(_vp), _P(C.c_uint32), C.c_uint32, _u64, _P(_vp), _P(C.c_uint32),
                                             C.c_uint32, _u64, C.c_int, _P(Opts), _vp, _vp, _vp, _P(_vp), _P(_vp), _u64, _P(_u64),
                                             _vp, _u64, _vp, _u64]),
    "rhj_group_arg_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _P(_vp), _P(C.c_uint32), _P(C.c_uint32), C.c_uint32, _u64, _P(Opts), _vp, _vp,
                                         _P(_vp), _P(_vp), _u64, _P(_u64)]),
    "rhj_group_arg_dev": (C.c_int, [_vp, _vp, _u64, _P(_vp), _P(C.c_uint32), _P(C.c_uint32), C.c_uint32, _u64, _P(Opts), _vp, _vp, _P(_vp),
                                    _P(_vp), _u64, _P(_u64)]),
    "rhj_keys_layout": (C.c_int, [C.c_uint32, _P(C.c_uint8), _u64, _P(KeysLayout)]),
    "rhj_keys_pack_dev": (C.c_int, [_vp, C.c_uint32, _P(_vp), _u64, _P(_vp), _u64, C.c_uint32, _vp, _vp, _P(_vp)]),
    "rhj_keys_unpack_dev": (C.c_int, [_vp, _vp, _vp, _u64, _P(_vp)]),
    "rhj_keys_plan_info": (C.c_int, [_vp, _P(KeysLayout)]),
    "rhj_keys_plan_free": (C.c_int, [_vp, _vp]),
    "rhj_asof_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_uint32, _u64, _vp, _P(_u64)]),
    "rhj_sort_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, C.c_uint32, _vp, _vp]),
    "rhj_sort_dev": (C.c_int, [_vp, _vp, _u64, C.c_uint32, _vp]),
    "rhj_topk_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, _u64, C.c_uint32, _vp, _vp, _P(_u64)]),
    "rhj_topk_dev": (C.c_int, [_vp, _vp, _u64, _u64, C.c_uint32, _vp, _P(_u64)]),
    "rhj_window_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, C.c_uint32, _P(C.c_uint32), _P(_u64), _P(_vp), C.c_uint32, _P(_vp), _P(_u64)]),
    "rhj_frame_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, C.c_uint32, _P(C.c_uint32), _P(_u64), _P(_u64), _P(_vp), C.c_uint32, _P(_vp), _P(_u64)]),
    "rhj_frame_range_cols_dev": (C.c_int, [_vp, _vp, _vp, _u64, C.c_uint32, _P(C.c_uint32), _P(_u64), _P(_u64), _P(_vp), C.c_uint32, _P(_vp), _P(_u64)]),
    "rhj_range_join_cols_dev": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_uint32, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _P(_u64)]),
    "rhj_range_expand_dev": (C.c_int, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _P(_u64)]),
    "rhj_histogram": (C.c_int, [_vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "rhj_prefix": (C.c_int, [_vp, _vp, _u64, _vp]),
    "rhj_partition": (C.c_int, [_vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "rhj_partition_at": (C.c_int, [_vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "rhj_owner_histogram": (C.c_int, [_vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "rhj_owner_split": (C.c_int, [_vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "rhj_mix64": (_u64, [_u64]),
    "rhj_unmix64": (_u64, [_u64]),
    "rhj_bucket_join": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _u64, _P(_u64)]),
    "rhj_narrow_key_offset": (_u64, [_u64]),
    "rhj_narrow_bytes": (_u64, [_u64]),
    "rhj_shard_plan": (C.c_int, [_u64, _u64, _P(Opts), _P(Opts)]),
    "rhj_shard_stats": (C.c_int, [_vp, C.c_int, _vp, _u64, C.c_int, C.c_int, _vp, _P(_u64), _P(_u64)]),
    "rhj_shard_split": (C.c_int, [_vp, C.c_int, _vp, _u64, C.c_int, C.c_int, _u64, _vp, _vp]),
    "rhj_shard_split_peer": (C.c_int, [_vp, C.c_int, _vp, _u64, C.c_int, C.c_int, _u64, _vp, _vp, _vp, _vp, C.c_int]),
    "rhj_ipc_export": (C.c_int, [_vp, _vp, _vp]),
    "rhj_ipc_open": (C.c_int, [_vp, _vp, _P(_vp)]),
    "rhj_ipc_close": (C.c_int, [_vp, _vp]),
    "rhj_shard_partition": (C.c_int, [_vp, C.c_int, _vp, _vp, _u64, C.c_int, _vp, _vp, _P(Opts), C.c_int]),
    "rhj_shard_join": (C.c_int, [_vp, _vp, _u64, _P(_u64)]),
    "rhj_pairs_checksum_dev": (C.c_int, [_vp, _vp, _u64, _P(_u64)]),
    "rhj_generate_dev": (C.c_int, [_vp, C.c_int, _vp, _u64, _u64, _u64, _u64, C.c_int]),
    "rhj_expected_pkfk_dev": (C.c_int, [_vp, _vp, _u64, _P(_u64), _P(_u64)]),
    "rhj_remap_keys_dev": (C.c_int, [_vp, _vp, _u64, C.c_int, _u64]),
    "rhj_col_filter": (C.c_int, [_vp, _vp, _vp, _u64, C.c_int, _u64, _vp, _P(_u64)]),
    "rhj_gather_tuples": (C.c_int, [_vp, _vp, _vp, _u64, C.c_int, _vp]),
    "rhj_pairs_split": (C.c_int, [_vp, _vp, _u64, _vp, _vp]),
    "rhj_gather_u64": (C.c_int, [_vp, _vp, _vp, _u64, _vp]),
    "rhj_gather_cols_fill": (C.c_int, [_vp, _P(_vp), C.c_uint32, _u64, _vp, _u64, _P(_u64), _P(_vp)]),
    "rhj_rows_filter_equal": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _P(_u64)]),
    "rhj_sum_gather": (C.c_int, [_vp, _vp, _vp, _u64, _P(_u64)]),
    "rhj_mul_u64": (C.c_int, [_vp, _vp, _vp, _u64, _vp]),
    "rhj_sum_gather_weighted": (C.c_int, [_vp, _vp, _vp, _vp, _u64, _P(_u64)]),
    "rhj_dev_alloc": (C.c_int, [_vp, _u64, _P(_vp)]),
    "rhj_dev_free": (C.c_int, [_vp, _vp]),
    "rhj_copy_h2d": (C.c_int, [_vp, _vp, _vp, _u64]),
    "rhj_copy_d2h": (C.c_int, [_vp, _vp, _vp, _u64]),
    "rhj_dev_mem_info": (C.c_int, [_vp, _P(_u64), _P(_u64)]),
}


def load_library():
    """Load librhj_hip.so and declare every prototype.  Raises if the library is not built."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: build it with `make -C radixhashjoin_amd/csrc` "
                              f"(or __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(path)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)         # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def plan(nR, nS, opts=None):
    """Resolved radix plan for these sizes (host logic only, works without a GPU)."""
    lib = load_library()
    out = Opts()
    rc = lib.rhj_plan(nR, nS, C.byref(opts) if opts is not None else None, C.byref(out))
    if rc != RHJ_OK:
        raise RhjError(rc, "bad options")
    return out


def mix64(x):
    """numpy form of rhj_mix64 (include/rhj.h): the bijection whose bits the engine's joins take their radix digits and
    owner classes from (splitmix64's finaliser).  x: uint64 array or scalar."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def unmix64(h):
    """inverse of mix64: unmix64(mix64(x)) == x (tests craft inputs whose MIXED value has a chosen bit pattern)"""
    with np.errstate(over="ignore"):
        x = np.asarray(h, dtype=np.uint64)
        x = x ^ (x >> np.uint64(31)) ^ (x >> np.uint64(62))
        x = x * np.uint64(0x319642B2D24D8EC3)
        x = x ^ (x >> np.uint64(27)) ^ (x >> np.uint64(54))
        x = x * np.uint64(0x96DE1B173F119089)
        x = x ^ (x >> np.uint64(30)) ^ (x >> np.uint64(60))
        return x - np.uint64(0x9E3779B97F4A7C15)


def narrow_key_offset(n):
    """byte offset of the rowID array in a narrow buffer of n tuples (include/rhj.h, multi-GPU wire format)"""
    return load_library().rhj_narrow_key_offset(n)


def narrow_bytes(n):
    return load_library().rhj_narrow_bytes(n)


SUM_MAX_COLS = 4                                         # include/rhj.h RHJ_SUM_MAX_COLS: weight columns of a join_sum_* call
GROUP_MAX_COLS = 4                                       # include/rhj.h RHJ_GROUP_MAX_COLS: weight columns of a group_sum_* call
GROUP_JOIN_MAX_COLS = 4                                  # include/rhj.h RHJ_GROUP_JOIN_MAX_COLS: weight columns per side of a group_join_* call
GJ_INNER, GJ_LEFT = 0, 1                                 # include/rhj.h RHJ_GJ_INNER / RHJ_GJ_LEFT: the mode of a group_join_* call
# include/rhj.h RHJ_AGG_*: the aggregate of a column of a group_agg_* / group_join_agg_* call
AGG_SUM, AGG_MIN_U64, AGG_MAX_U64, AGG_MIN_I64, AGG_MAX_I64 = 0, 1, 2, 3, 4
# ... of an int64 tensor by name (group_by_columns / join_group_by_columns), and what a minimum / maximum over no tuple holds
_AGG_BY_NAME = {"sum": AGG_SUM, "min": AGG_MIN_I64, "max": AGG_MAX_I64}
_AGG_IDENTITY_I64 = {AGG_SUM: 0, AGG_MIN_I64: 2**63 - 1, AGG_MAX_I64: -2**63}


def _agg_ops(ops, n, name):
    """the RHJ_AGG_* of n int64 weight tensors from their names ("sum" | "min" | "max"); ValueError on a wrong length or name"""
    ops = list(ops)
    if len(ops) != n:
        raise ValueError(f"{name}: {len(ops)} ops for {n} weight tensors")
    for i, o in enumerate(ops):
        if o not in _AGG_BY_NAME:
            raise ValueError(f"{name}[{i}]: 'sum', 'min' or 'max', not {o!r}")
    return [_AGG_BY_NAME[o] for o in ops]
# include/rhj.h RHJ_ARG_*: what a column of a group_arg_* call orders, RHJ_ARG_TIE_*: which of the rows that tie, and the columns per call
ARG_MIN_U64, ARG_MAX_U64, ARG_MIN_I64, ARG_MAX_I64, ARG_ROW = 0, 1, 2, 3, 4
ARG_TIE_FIRST, ARG_TIE_LAST = 0, 1
GROUP_ARG_MAX_COLS = 4
# ... by name (group_by_columns_arg): "min" / "max" order int64 tensors as signed words
_ARG_BY_NAME = {"min": ARG_MIN_I64, "max": ARG_MAX_I64, "min_u64": ARG_MIN_U64, "max_u64": ARG_MAX_U64, "row": ARG_ROW}
_TIE_BY_NAME = {"first": ARG_TIE_FIRST, "last": ARG_TIE_LAST}


def _arg_ops(by, ops, ties):
    """(RHJ_ARG_* words, RHJ_ARG_TIE_* words) of a group_by_columns_arg call from their names; ValueError on a wrong length, name, a
    column too many or a value op without a tensor -- nothing here touches a device"""
    by, ops = list(by), list(ops)
    if len(by) > GROUP_ARG_MAX_COLS:
        raise ValueError(f"at most {GROUP_ARG_MAX_COLS} columns per call, not {len(by)}")
    if len(ops) != len(by):
        raise ValueError(f"ops: {len(ops)} ops for {len(by)} columns")
    ties = [ties] * len(by) if isinstance(ties, str) else list(ties)
    if len(ties) != len(by):
        raise ValueError(f"ties: {len(ties)} ties for {len(by)} columns")
    for i, o in enumerate(ops):
        if not isinstance(o, str) or o not in _ARG_BY_NAME:
            raise ValueError(f"ops[{i}]: 'min', 'max', 'min_u64', 'max_u64' or 'row', not {o!r}")
        if o != "row" and by[i] is None:
            raise ValueError(f"by[{i}]: {o!r} needs a tensor; None goes with 'row' only")
    for i, t in enumerate(ties):
        if not isinstance(t, str) or t not in _TIE_BY_NAME:
            raise ValueError(f"ties[{i}]: 'first' or 'last', not {t!r}")
    return [_ARG_BY_NAME[o] for o in ops], [_TIE_BY_NAME[t] for t in ties]
# include/rhj.h RHJ_KEYS_*: key columns per pack call; the flag of a pack that keeps no dictionaries; the kind of a column; fold ids
KEYS_MAX_COLS, KEYS_NO_UNPACK, KEYS_RANGE, KEYS_DICT, KEYS_MAX_FOLDS, KEYS_FOLD0 = 4, 1, 0, 1, 2, 4
SEMI, ANTI = 0, 1                                        # include/rhj.h RHJ_SEMI / RHJ_ANTI: the kind of a semi_join_* call
OUTER_LEFT, OUTER_RIGHT, OUTER_FULL = 1, 2, 3           # include/rhj.h RHJ_OUTER_*: the preserved side(s) of an outer_join_* call
NO_ROW = 0xFFFFFFFFFFFFFFFF                              # include/rhj.h RHJ_NO_ROW: the missing side of an unmatched row (-1 as int64)
LOOKUP_FIRST, LOOKUP_LAST = 0, 1                         # include/rhj.h RHJ_LOOKUP_*: the smallest / largest rowID of S among the partners
LOOKUP_MAX_COLS = 4                                      # include/rhj.h RHJ_LOOKUP_MAX_COLS: columns of a gather_cols_fill call
SORT_I64, SORT_DESC = 1, 2                               # include/rhj.h RHJ_SORT_*: flags of the sort entries
# include/rhj.h RHJ_WIN_*: the ops of a window_cols_dev call, and how many one call takes
WINDOW_MAX_OPS = 4
WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_LAG_ROW, WIN_LEAD_ROW = 0, 1, 2, 3, 4
WIN_CUMSUM, WIN_CUMMIN_U64, WIN_CUMMAX_U64, WIN_CUMMIN_I64, WIN_CUMMAX_I64 = 5, 6, 7, 8, 9
# ... by name (window_columns): "cummin" / "cummax" order int64 tensors as signed words
_WIN_BY_NAME = {"row_number": WIN_ROW_NUMBER, "rank": WIN_RANK, "dense_rank": WIN_DENSE_RANK, "lag": WIN_LAG_ROW, "lead": WIN_LEAD_ROW,
                "cumsum": WIN_CUMSUM, "cummin": WIN_CUMMIN_I64, "cummax": WIN_CUMMAX_I64, "cummin_u64": WIN_CUMMIN_U64,
                "cummax_u64": WIN_CUMMAX_U64}


def _window_args(order_by, values, ops, descending, unsigned, offsets, fill):
    """(RHJ_WIN_* words, value tensors or None, offsets) of a window_columns call; ValueError on a wrong name, length, flag or offset --
    nothing here touches a device"""
    if isinstance(ops, str):
        raise ValueError(f"ops: a sequence of op names is needed, not the string {ops!r}")
    ops = list(ops)
    if not ops:
        raise ValueError("ops: at least one op is needed")
    if len(ops) > WINDOW_MAX_OPS:
        raise ValueError(f"ops: at most {WINDOW_MAX_OPS} ops per call, not {len(ops)}")
    for i, o in enumerate(ops):
        if not isinstance(o, str) or o not in _WIN_BY_NAME:
            raise ValueError(f"ops[{i}]: one of {', '.join(repr(k) for k in _WIN_BY_NAME)}, not {o!r}")
    values = list(values) if values is not None else []
    if not values:
        values = [None] * len(ops)
    if len(values) != len(ops):
        raise ValueError(f"values: {len(values)} entries for {len(ops)} ops (None for an op without a column)")
    if offsets is None:
        offs = [1] * len(ops)
    else:
        offs = list(offsets)
        if len(offs) != len(ops):
            raise ValueError(f"offsets: {len(offs)} entries for {len(ops)} ops")
    if not isinstance(descending, bool):
        raise ValueError(f"descending: a bool is needed, not {descending!r}")
    if not isinstance(unsigned, bool):
        raise ValueError(f"unsigned: a bool is needed, not {unsigned!r}")
    if descending and order_by is None:
        raise ValueError("descending: True needs an order_by tensor; without one the order is the input order")
    if isinstance(order_by, (list, tuple)):
        raise ValueError("order_by: one tensor or None -- for ORDER BY a, b run sort_columns([k, a, b]) first and pass order_by=None")
    for i, o in enumerate(ops):
        if o in ("lag", "lead"):
            if isinstance(offs[i], bool) or not isinstance(offs[i], int) or offs[i] < 1:
                raise ValueError(f"offsets[{i}]: an int >= 1 is needed for {o!r}, not {offs[i]!r}")
        elif o in ("row_number", "rank", "dense_rank"):
            if values[i] is not None:
                raise ValueError(f"values[{i}]: {o!r} takes no column; None is needed")
        elif values[i] is None:
            raise ValueError(f"values[{i}]: {o!r} needs a tensor")
    if isinstance(fill, bool) or not isinstance(fill, int):
        raise ValueError(f"fill: an int is needed, not {fill!r}")
    return [_WIN_BY_NAME[o] for o in ops], values, [o if isinstance(o, int) and not isinstance(o, bool) else 1 for o in offs]


# include/rhj.h RHJ_ASOF_*: flags of an asof_cols_dev call -- the int64 view, at or after, equal words excluded, the distance bound
ASOF_I64, ASOF_FORWARD, ASOF_STRICT, ASOF_TOLERANCE = 1, 2, 4, 8


def _asof_args(by_R, by_S, values_S, direction, allow_exact_matches, tolerance, unsigned, fill):
    """(flags, tolerance word, value tensors, fills) of an asof_join_columns call; ValueError on a wrong direction, flag, tolerance, `by`
    or number of tensors -- nothing here touches a device"""
    if direction == "nearest":
        raise ValueError("direction: 'nearest' is not supported -- run 'backward' and 'forward' and keep the closer partner per row")
    if not isinstance(direction, str) or direction not in ("backward", "forward"):
        raise ValueError(f"direction: 'backward' or 'forward' is needed ('nearest' is not supported), not {direction!r}")
    if not isinstance(allow_exact_matches, bool):
        raise ValueError(f"allow_exact_matches: a bool is needed, not {allow_exact_matches!r}")
    if not isinstance(unsigned, bool):
        raise ValueError(f"unsigned: a bool is needed, not {unsigned!r}")
    if tolerance is not None and (isinstance(tolerance, bool) or not isinstance(tolerance, int) or not 0 <= tolerance <= NO_ROW):
        raise ValueError(f"tolerance: an int >= 0 (below 2^64) or None is needed, not {tolerance!r}")
    if (by_R is None) != (by_S is None):
        raise ValueError(f"{'by_S' if by_S is None else 'by_R'}: None, but the other side has a `by`: both sides or neither")
    if by_R is not None:
        counts = [len(b) if isinstance(b, (list, tuple)) else 1 for b in (by_R, by_S)]
        for name, k in zip(("by_R", "by_S"), counts):
            if not 1 <= k <= KEYS_MAX_COLS:
                raise ValueError(f"{name}: 1 to {KEYS_MAX_COLS} tensors are needed, not {k}")
        if counts[0] != counts[1]:
            raise ValueError(f"by_S: {counts[1]} tensors, by_R has {counts[0]}")
    values_S = tuple(values_S)
    if len(values_S) > LOOKUP_MAX_COLS:
        raise ValueError(f"values_S: at most {LOOKUP_MAX_COLS} value tensors per call, not {len(values_S)}")
    fills = [fill] * len(values_S) if isinstance(fill, int) else list(fill) if isinstance(fill, (list, tuple)) else [None]
    if len(fills) != len(values_S) or not all(isinstance(f, int) and not isinstance(f, bool) for f in fills):
        raise ValueError(f"fill: an int, or one int per tensor of values_S ({len(values_S)}), is needed")
    flags = ((0 if unsigned else ASOF_I64) | (ASOF_FORWARD if direction == "forward" else 0) | (0 if allow_exact_matches else ASOF_STRICT) |
             (ASOF_TOLERANCE if tolerance is not None else 0))
    return flags, tolerance or 0, values_S, fills


# include/rhj.h RHJ_RANGE_*: flags of a range_join_cols_dev call -- the int64 view, the open ends, the band form
RANGE_I64, RANGE_LO_OPEN, RANGE_HI_OPEN, RANGE_BAND = 1, 2, 4, 8
_RANGE_CLOSED = {"both": 0, "left": RANGE_HI_OPEN, "right": RANGE_LO_OPEN, "neither": RANGE_LO_OPEN | RANGE_HI_OPEN}


def _range_args(by_R, by_S, closed, unsigned, below=0, above=0, lo_R=None, hi_R=None):
    """the flags of a range_join_columns / band_join_columns call (without RANGE_BAND); ValueError on a wrong `closed`, flag, distance,
    `by`, number of tensors or length -- nothing here touches a device"""
    if not isinstance(closed, str) or closed not in _RANGE_CLOSED:
        raise ValueError(f"closed: 'both', 'left', 'right' or 'neither' is needed, not {closed!r}")
    if not isinstance(unsigned, bool):
        raise ValueError(f"unsigned: a bool is needed, not {unsigned!r}")
    for name, d in (("below", below), ("above", above)):
        if isinstance(d, bool) or not isinstance(d, int) or not 0 <= d <= NO_ROW:
            raise ValueError(f"{name}: an int >= 0 (below 2^64) is needed, not {d!r}")
    if (by_R is None) != (by_S is None):
        raise ValueError(f"{'by_S' if by_S is None else 'by_R'}: None, but the other side has a `by`: both sides or neither")
    if by_R is not None:
        counts = [len(b) if isinstance(b, (list, tuple)) else 1 for b in (by_R, by_S)]
        for name, k in zip(("by_R", "by_S"), counts):
            if not 1 <= k <= KEYS_MAX_COLS:
                raise ValueError(f"{name}: 1 to {KEYS_MAX_COLS} tensors are needed, not {k}")
        if counts[0] != counts[1]:
            raise ValueError(f"by_S: {counts[1]} tensors, by_R has {counts[0]}")
    if hasattr(lo_R, "numel") and hasattr(hi_R, "numel") and lo_R.numel() != hi_R.numel():
        raise ValueError(f"hi_R: {hi_R.numel()} elements, lo_R has {lo_R.numel()}")
    return (0 if unsigned else RANGE_I64) | _RANGE_CLOSED[closed]


# include/rhj.h RHJ_FRAME_*: the ops of a frame_cols_dev call, how many one call takes, and "to the partition's edge"
FRAME_MAX_OPS = 4
FRAME_UNBOUNDED = 0xFFFFFFFFFFFFFFFF
FRAME_COUNT, FRAME_SUM, FRAME_MIN_U64, FRAME_MAX_U64, FRAME_MIN_I64, FRAME_MAX_I64, FRAME_FIRST_ROW, FRAME_LAST_ROW = range(8)
_FRAME_NAMES = ("count", "sum", "min", "max", "first_row", "last_row")


def _frame_args(order, cols, ops, preceding, following, descending, unsigned):
    """(RHJ_FRAME_* words, column tensors or None, preceding words, following words) of a frame_columns call; ValueError on a wrong
    name, length, bound or flag -- nothing here touches a device"""
    if isinstance(ops, str):
        raise ValueError(f"ops: a sequence of op names is needed, not the string {ops!r}")
    ops = list(ops) if ops is not None else []
    if not ops:
        raise ValueError("ops: at least one op is needed")
    if len(ops) > FRAME_MAX_OPS:
        raise ValueError(f"ops: at most {FRAME_MAX_OPS} ops per call, not {len(ops)}")
    for i, o in enumerate(ops):
        if not isinstance(o, str) or o not in _FRAME_NAMES:
            raise ValueError(f"ops[{i}]: one of {', '.join(repr(k) for k in _FRAME_NAMES)}, not {o!r}")
    cols = list(cols) if cols is not None else []
    if not cols:
        cols = [None] * len(ops)
    if len(cols) != len(ops):
        raise ValueError(f"cols: {len(cols)} entries for {len(ops)} ops (None for an op without a column)")
    bounds = []
    for name, b in (("preceding", preceding), ("following", following)):
        side = list(b) if isinstance(b, (list, tuple)) else [b] * len(ops)
        if len(side) != len(ops):
            raise ValueError(f"{name}: {len(side)} entries for {len(ops)} ops")
        for i, x in enumerate(side):
            if x is not None and (isinstance(x, bool) or not isinstance(x, int) or not 0 <= x <= FRAME_UNBOUNDED):
                raise ValueError(f"{name}{f'[{i}]' if isinstance(b, (list, tuple)) else ''}: an int >= 0 (below 2^64) or None (unbounded) is needed, not {x!r}")
        bounds.append([FRAME_UNBOUNDED if x is None else x for x in side])
    if not isinstance(descending, bool):
        raise ValueError(f"descending: a bool is needed, not {descending!r}")
    if not isinstance(unsigned, bool):
        raise ValueError(f"unsigned: a bool is needed, not {unsigned!r}")
    if descending and order is None:
        raise ValueError("descending: True needs an order tensor; without one the order is the input order")
    if isinstance(order, (list, tuple)):
        raise ValueError("order: one tensor or None -- for ORDER BY a, b run sort_columns([k, a, b]) first and pass order=None")
    for i, o in enumerate(ops):
        if o in ("count", "first_row", "last_row"):
            if cols[i] is not None:
                raise ValueError(f"cols[{i}]: {o!r} takes no column; None is needed")
        elif cols[i] is None:
            raise ValueError(f"cols[{i}]: {o!r} needs a tensor")
    words = {"count": FRAME_COUNT, "sum": FRAME_SUM, "min": FRAME_MIN_U64 if unsigned else FRAME_MIN_I64,
             "max": FRAME_MAX_U64 if unsigned else FRAME_MAX_I64, "first_row": FRAME_FIRST_ROW, "last_row": FRAME_LAST_ROW}
    return [words[o] for o in ops], cols, bounds[0], bounds[1]


SHARD_TAGGED, SHARD_GLOBAL16, SHARD_PLAIN = 1, 2, 3      # include/rhj.h: how the receiver restores global rowIDs


def shard_plan(nR, nS, opts=None):
    """(mode, plan): mode = SHARD_TAGGED / SHARD_GLOBAL16 (or SHARD_PLAIN for the 17-18-bit local plans of receivers beyond
    1.1 * 10^9 tuples, which cannot restore rowIDs) when the narrow sharded path (rhj_shard_*) serves a local join of these sizes
    under `plan`, 0 when it does not (exchange 16-byte tuples instead).  The host may use SHARD_PLAIN instead of the other two
    whenever every rowID of both relations is below 2^32."""
    lib = load_library()
    out = Opts()
    rc = lib.rhj_shard_plan(nR, nS, C.byref(opts) if opts is not None else None, C.byref(out))
    if rc < 0:
        raise RhjError(rc, "bad options")
    return rc, out


def keys_layout(range_bits, n_total):
    """rhj_keys_layout: the KeysLayout a pack of key columns of these widths (bits, 0 .. 64) over n_total rows will use (host logic
    only, works without a GPU); RhjError where there is none"""
    lib = load_library()
    widths = list(range_bits)
    out = KeysLayout()
    rc = lib.rhj_keys_layout(len(widths), (C.c_uint8 * max(len(widths), 1))(*widths), n_total, C.byref(out))
    if rc != RHJ_OK:
        raise RhjError(rc, f"no layout for widths {widths} over {n_total} rows")
    return out


def _addr(x):
    """device address of: int, DeviceBuffer, or anything with data_ptr() (torch tensor)"""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    raise TypeError(f"not a device pointer: {type(x)}")


class DeviceBuffer:
    """A raw HBM allocation owned through the C-ABI (rhj_dev_alloc / rhj_dev_free)."""

    def __init__(self, engine, nbytes):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = _vp()
        engine._chk(engine.lib.rhj_dev_alloc(engine.ctx, self.nbytes, C.byref(p)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, engine, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(engine, max(arr.nbytes, 16))
        if arr.nbytes:
            engine._chk(engine.lib.rhj_copy_h2d(engine.ctx, b.ptr, arr.ctypes.data, arr.nbytes))
        return b

    def to_numpy(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self.engine._chk(self.engine.lib.rhj_copy_d2h(self.engine.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.engine.lib.rhj_dev_free(self.engine.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class KeyPlan:
    """An rhj_keyplan: what Engine.keys_pack_dev / pack_keys made of a set of key columns -- the layout of the packed word and, unless
    packed with KEYS_NO_UNPACK, the dictionaries that turn packed words back into the columns.  Owns device memory: close() it (or
    let it go out of scope, as a DeviceBuffer)."""

    def __init__(self, engine, handle):
        self.engine = engine
        self.handle = handle
        self.layout = KeysLayout()
        engine._chk(engine.lib.rhj_keys_plan_info(handle, C.byref(self.layout)))
        self.nkeys = self.layout.nkeys

    def unpack(self, packed):
        """the nkeys key columns of a 1-D tensor of packed words this plan produced (a pack output, the unique_keys of a group-by
        over one): a list of tensors of packed's dtype and length, bit for bit the values that were packed"""
        import torch
        eng = self.engine
        with eng._on_torch_stream(packed, packed) as dev:
            n = packed.numel()
            cols = [torch.empty(n, dtype=packed.dtype, device=dev) for _ in range(self.nkeys)]
            if n:
                eng.keys_unpack_dev(self, packed, n, cols)
        return cols

    def close(self):
        if self.handle:
            h, self.handle = self.handle, None
            if self.engine.ctx:
                self.engine.lib.rhj_keys_plan_free(self.engine.ctx, h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_libc = C.CDLL(None)
_libc.free.argtypes = [_vp]
_libc_free = _libc.free


class Engine:
    """One rhj_ctx: a HIP stream + HBM workspace on one GPU.  Not thread-safe (one per caller thread)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.ctx = None
        self.device = device
        self.bound_stream = None        # the caller's stream set_stream bound the context to (None: the context's own stream)
        c = _vp()
        rc = self.lib.rhj_init(device, C.byref(c))
        if rc != RHJ_OK:
            raise RhjError(rc, (self.lib.rhj_last_error(None) or b"").decode())
        self.ctx = c

    def close(self):
        if self.ctx:
            self.lib.rhj_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=()):
        if rc != RHJ_OK and rc not in allow:
            raise RhjError(rc, (self.lib.rhj_last_error(self.ctx) or b"").decode())
        return rc

    # ---- context ------------------------------------------------------------------------------
    def set_stream(self, raw_stream):
        """rhj_set_stream: run on a caller-owned hipStream_t; None / 0: the context's own stream.  Synchronises the stream in use."""
        self._chk(self.lib.rhj_set_stream(self.ctx, raw_stream))
        self.bound_stream = raw_stream or None

    def set_option(self, name, value):
        """tuning / test knobs of include/rhj.h (results never depend on them)"""
        self._chk(self.lib.rhj_set_option(self.ctx, name.encode(), int(value)))

    def info(self, name):
        """what the last join did ("last.narrow", "last.countfree_R" / "_S", "last.cols_R" / "_S", "last.join_kernel", "last.semi_tables", "last.outer_sweeps", "last.group_rounds",
        "last.sort_bits", "last.sort_passes", "last.sort_units", "last.topk_bits", "last.topk_passes", "last.topk_candidates",
        "last.topk_sorted_rows", "last.window_units", "last.window_sorts", "last.window_partitions", "last.asof_units", "last.asof_sorts",
        "last.asof_matched", "last.frame_units", "last.frame_sorts", "last.frame_scans", "last.frame_partitions", "last.frame_range_units", "last.frame_range_sorts",
        "last.frame_range_scans", "last.frame_range_levels", "last.frame_range_partitions", "last.range_join_units", "last.range_join_sorts",
        "last.range_join_pairs", "last.range_join_expand_tiles"; include/rhj.h) and constants of the build ("sort.tile_rows", "topk.auto_candidates", "window.tile_rows",
        "asof.tile_rows", "range_join.tile_rows", "range_join.expand_tile")"""
        v = C.c_int64(0)
        self._chk(self.lib.rhj_get_info(self.ctx, name.encode(), C.byref(v)))
        return v.value

    def set_profiling(self, on=True):
        """True / 1: time every launch of a call; 2: accumulate the launches of successive calls (see rhj.h); False / 0: off"""
        self._chk(self.lib.rhj_set_profiling(self.ctx, 2 if on == 2 and on is not True else 1 if on else 0))

    def timings(self):
        t = Timings()
        self._chk(self.lib.rhj_get_timings(self.ctx, C.byref(t)))
        return t.as_dict()

    def launch_timings(self, capacity=4096):
        """[(kind name, ms)] of every timed launch span of the last call, in launch order (profiling must be on)"""
        kinds, ms, n = (_i32 * capacity)(), (C.c_double * capacity)(), C.c_uint32()
        self._chk(self.lib.rhj_get_launch_timings(self.ctx, kinds, ms, capacity, C.byref(n)))
        return [(KERNEL_KINDS[kinds[i]], ms[i]) for i in range(min(n.value, capacity))]

    def sync(self):
        self._chk(self.lib.rhj_sync(self.ctx))

    def reserve(self, nR, nS, opts=None):
        self._chk(self.lib.rhj_reserve(self.ctx, nR, nS, C.byref(opts) if opts is not None else None))

    def release_workspace(self):
        self._chk(self.lib.rhj_release_workspace(self.ctx))

    def mem_info(self):
        f, t = _u64(), _u64()
        self._chk(self.lib.rhj_dev_mem_info(self.ctx, C.byref(f), C.byref(t)))
        return f.value, t.value

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        return DeviceBuffer.from_numpy(self, arr)

    # ---- the drop-in (host arrays) -----------------------------------------------------------
    def join(self, R, S, opts=None):
        """rhj_join: host AoS in -> numpy array of (rowR,rowS) pairs (copied out of the result page)."""
        R = np.ascontiguousarray(R, dtype=TUPLE)
        S = np.ascontiguousarray(S, dtype=TUPLE)
        page, n = _vp(), _u64()
        self._chk(self.lib.rhj_join(self.ctx, R.ctypes.data, len(R), S.ctypes.data, len(S),
                                    C.byref(opts) if opts is not None else None, C.byref(page), C.byref(n)))
        out = np.empty(n.value, dtype=PAIR)
        if page.value:
            head = C.c_uint64.from_address(page.value).value       # bucket_info::next must be NULL
            assert head == 0
            C.memmove(out.ctypes.data, page.value + 8, out.nbytes)
            C.CDLL(None).free(_vp(page.value))
        else:
            assert n.value == 0
        return out

    def join_batch(self, joins, keep_pairs=True, timed=False):
        """rhj_join_batch over a list of (R, S) host relations: list of pair arrays (or of counts with keep_pairs=False: the pages
        are then freed right away, as ~Result does); timed: also the seconds spent inside the C call"""
        import time
        rel = [(np.ascontiguousarray(R, dtype=TUPLE), np.ascontiguousarray(S, dtype=TUPLE)) for R, S in joins]
        n = len(rel)
        desc = (JoinDesc * max(n, 1))()
        for i, (R, S) in enumerate(rel):
            desc[i] = JoinDesc(R.ctypes.data, len(R), S.ctypes.data, len(S))
        pages, counts = (_vp * max(n, 1))(), (_u64 * max(n, 1))()
        t0 = time.perf_counter()
        rc = self.lib.rhj_join_batch(self.ctx, n, desc, pages, counts)
        dt = time.perf_counter() - t0
        self._chk(rc)
        out = []
        for i in range(n):
            if keep_pairs:
                a = np.empty(counts[i], dtype=PAIR)
                if pages[i]:
                    assert C.c_uint64.from_address(pages[i]).value == 0          # bucket_info::next
                    C.memmove(a.ctypes.data, pages[i] + 8, a.nbytes)
                else:
                    assert counts[i] == 0
                out.append(a)
            else:
                out.append(int(counts[i]))
            if pages[i]:
                _libc_free(_vp(pages[i]))
        return (out, dt) if timed else out

    def join_count_only_page(self, R, S, opts=None, timed=False):
        """rhj_join exactly as the C++ mirror calls it, the result page freed right away (what ~Result does): for
        timing the drop-in without numpy's copy of the pairs.  timed=True also returns the seconds spent in the C call."""
        import time
        R = np.ascontiguousarray(R, dtype=TUPLE)
        S = np.ascontiguousarray(S, dtype=TUPLE)
        page, n = _vp(), _u64()
        t0 = time.perf_counter()
        rc = self.lib.rhj_join(self.ctx, R.ctypes.data, len(R), S.ctypes.data, len(S),
                               C.byref(opts) if opts is not None else None, C.byref(page), C.byref(n))
        dt = time.perf_counter() - t0
        self._chk(rc)
        if page.value:
            _libc_free(_vp(page.value))
        return (n.value, dt) if timed else n.value

    # ---- device-resident ------------------------------------------------------------------------
    def join_dev(self, d_R, nR, d_S, nS, d_out=None, capacity=0, opts=None, allow_overflow=False):
        n = _u64()
        rc = self.lib.rhj_join_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS,
                                   C.byref(opts) if opts is not None else None, _addr(d_out), capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def join_cols_dev(self, d_valR, d_idR, nR, d_valS, d_idS, nS, d_out=None, capacity=0, opts=None, allow_overflow=False):
        """rhj_join_cols_dev: join_dev with each relation as columns in HBM (uint64 join values; uint64 rowIDs, or None: the
        rowID of a tuple is its index)"""
        n = _u64()
        rc = self.lib.rhj_join_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), _addr(d_idS), nS,
                                        C.byref(opts) if opts is not None else None, _addr(d_out), capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def semi_join_cols_dev(self, d_valR, d_idR, nR, d_valS, nS, kind, d_out=None, capacity=0, opts=None, allow_overflow=False):
        """rhj_semi_join_cols_dev: the rowIDs of the R tuples whose join value occurs (kind SEMI) / does not occur (ANTI) in the
        value column of S, each once; d_out: uint64[capacity] in HBM, or None to count"""
        n = _u64()
        rc = self.lib.rhj_semi_join_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), nS, kind,
                                             C.byref(opts) if opts is not None else None, _addr(d_out), capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def semi_join_dev(self, d_R, nR, d_S, nS, kind, d_out=None, capacity=0, opts=None, allow_overflow=False):
        """rhj_semi_join_dev: semi_join_cols_dev on 16-byte tuples (the rowIDs of S are not looked at)"""
        n = _u64()
        rc = self.lib.rhj_semi_join_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, kind,
                                        C.byref(opts) if opts is not None else None, _addr(d_out), capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def outer_join_cols_dev(self, d_valR, d_idR, nR, d_valS, d_idS, nS, how, d_out=None, capacity=0, opts=None, allow_overflow=False):
        """rhj_outer_join_cols_dev: (count, (matched, R-only, S-only)) -- the pairs of join_cols_dev, then {rowR, NO_ROW} per tuple of R
        without a partner (how & OUTER_LEFT), then {NO_ROW, rowS} per tuple of S without one (how & OUTER_RIGHT), in that order in
        d_out: PAIR[capacity] in HBM, or None to count"""
        n, sec = _u64(), (_u64 * 3)()
        rc = self.lib.rhj_outer_join_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), _addr(d_idS), nS, how,
                                              C.byref(opts) if opts is not None else None, _addr(d_out), capacity, C.byref(n), sec)
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value, tuple(int(x) for x in sec)

    def outer_join_dev(self, d_R, nR, d_S, nS, how, d_out=None, capacity=0, opts=None, allow_overflow=False):
        """rhj_outer_join_dev: outer_join_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n, sec = _u64(), (_u64 * 3)()
        rc = self.lib.rhj_outer_join_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, how,
                                         C.byref(opts) if opts is not None else None, _addr(d_out), capacity, C.byref(n), sec)
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value, tuple(int(x) for x in sec)

    @staticmethod
    def _sum_args(d_cols):
        cols = (_vp * max(len(d_cols), 1))(*[_addr(c) for c in d_cols])
        return cols, (_u64 * max(len(d_cols), 1))()

    def join_sum_cols_dev(self, d_valR, d_idR, nR, d_valS, nS, d_cols=(), col_rows=0, opts=None):
        """rhj_join_sum_cols_dev: (count, [sums]) -- |R join S| and, per column of d_cols (at most SUM_MAX_COLS device columns of
        col_rows uint64, indexed by R's rowID), the sum of the column over the pairs mod 2^64, as Python ints; no pair is written"""
        n = _u64()
        cols, sums = self._sum_args(d_cols)
        self._chk(self.lib.rhj_join_sum_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), nS, cols, len(d_cols),
                                                 col_rows, C.byref(opts) if opts is not None else None, C.byref(n), sums))
        return n.value, [int(sums[j]) for j in range(len(d_cols))]

    def join_sum_dev(self, d_R, nR, d_S, nS, d_cols=(), col_rows=0, opts=None):
        """rhj_join_sum_dev: join_sum_cols_dev on 16-byte tuples (rowR = .key; the rowIDs of S are not looked at)"""
        n = _u64()
        cols, sums = self._sum_args(d_cols)
        self._chk(self.lib.rhj_join_sum_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, cols, len(d_cols), col_rows,
                                            C.byref(opts) if opts is not None else None, C.byref(n), sums))
        return n.value, [int(sums[j]) for j in range(len(d_cols))]

    def join_mult_cols_dev(self, d_valR, d_idR, nR, d_valS, d_idS, nS, d_out, out_rows, d_wS=None, wS_rows=0, opts=None):
        """rhj_join_mult_cols_dev: d_out (out_rows uint64 words, zeroed by the call) receives, per rowID of R, the number of tuples
        of S with that tuple's join value -- with d_wS (wS_rows words indexed by S's rowID) the sum of their weights -- mod 2^64;
        returns the sum of all of them (unweighted: |R join S|) as a Python int"""
        total = _u64()
        self._chk(self.lib.rhj_join_mult_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), _addr(d_idS), nS,
                                                  _addr(d_wS), wS_rows, C.byref(opts) if opts is not None else None,
                                                  _addr(d_out), out_rows, C.byref(total)))
        return total.value

    def join_mult_dev(self, d_R, nR, d_S, nS, d_out, out_rows, d_wS=None, wS_rows=0, opts=None):
        """rhj_join_mult_dev: join_mult_cols_dev on 16-byte tuples (rowR / rowS = .key)"""
        total = _u64()
        self._chk(self.lib.rhj_join_mult_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, _addr(d_wS), wS_rows,
                                             C.byref(opts) if opts is not None else None, _addr(d_out), out_rows, C.byref(total)))
        return total.value

    def lookup_cols_dev(self, d_valR, d_idR, nR, d_valS, d_idS, nS, d_out, out_rows, which=LOOKUP_FIRST, opts=None):
        """rhj_lookup_cols_dev: d_out (out_rows uint64 words, set to NO_ROW by the call) receives, per rowID of R, the smallest
        (LOOKUP_FIRST) or largest (LOOKUP_LAST) rowID of S among the tuples of S with that tuple's join value; returns the number
        of words that found a partner"""
        matched = _u64()
        self._chk(self.lib.rhj_lookup_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), _addr(d_idS), nS, which,
                                               C.byref(opts) if opts is not None else None, _addr(d_out), out_rows, C.byref(matched)))
        return matched.value

    def lookup_dev(self, d_R, nR, d_S, nS, d_out, out_rows, which=LOOKUP_FIRST, opts=None):
        """rhj_lookup_dev: lookup_cols_dev on 16-byte tuples (rowR / rowS = .key)"""
        matched = _u64()
        self._chk(self.lib.rhj_lookup_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, which,
                                          C.byref(opts) if opts is not None else None, _addr(d_out), out_rows, C.byref(matched)))
        return matched.value

    def _group_args(self, d_cols, d_out_sums):
        """the two host arrays of a group_sum_* call (a sum column that is missing goes in as NULL: the library answers)"""
        k = max(len(d_cols), 1)
        sums = list(d_out_sums)[:len(d_cols)]
        return (_vp * k)(*[_addr(c) for c in d_cols]), (_vp * k)(*[_addr(c) for c in sums + [None] * (len(d_cols) - len(sums))])

    @staticmethod
    def _ops_arg(ops, ncols):
        """the host array of a side's ops, one per column (None: NULL, every column a sum)"""
        if ops is None:
            return None
        ops = list(ops)
        if len(ops) != ncols:
            raise ValueError(f"{len(ops)} ops for {ncols} columns")
        return (C.c_uint32 * max(ncols, 1))(*ops)

    def group_sum_cols_dev(self, d_valR, d_idR, nR, d_cols=(), col_rows=0, d_out_keys=None, d_out_counts=None, d_out_sums=(),
                           capacity=0, opts=None, allow_overflow=False):
        """rhj_group_sum_cols_dev: one output row per distinct join value of R (uint64 value column; uint64 rowIDs, or None: the
        rowID of a tuple is its index) -- d_out_keys[g] the value, d_out_counts[g] (may be None) how many tuples carry it,
        d_out_sums[j][g] the sum of d_cols[j][rowID] over them mod 2^64 (at most GROUP_MAX_COLS device columns of col_rows uint64) --
        in no particular order; every output is uint64[capacity] in HBM.  d_out_keys None with capacity 0 counts the distinct
        values only.  Returns the number of groups (with allow_overflow also when it exceeds capacity)"""
        n = _u64()
        cols, sums = self._group_args(d_cols, d_out_sums)
        rc = self.lib.rhj_group_sum_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, cols, len(d_cols), col_rows,
                                             C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_counts),
                                             sums, capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_sum_dev(self, d_R, nR, d_cols=(), col_rows=0, d_out_keys=None, d_out_counts=None, d_out_sums=(), capacity=0, opts=None,
                      allow_overflow=False):
        """rhj_group_sum_dev: group_sum_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n = _u64()
        cols, sums = self._group_args(d_cols, d_out_sums)
        rc = self.lib.rhj_group_sum_dev(self.ctx, _addr(d_R), nR, cols, len(d_cols), col_rows,
                                        C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_counts), sums,
                                        capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_agg_cols_dev(self, d_valR, d_idR, nR, d_cols=(), ops=None, col_rows=0, d_out_keys=None, d_out_counts=None, d_out_aggs=(),
                           capacity=0, opts=None, allow_overflow=False):
        """rhj_group_agg_cols_dev: group_sum_cols_dev with an aggregate per column -- ops[j] one of AGG_SUM, AGG_MIN_U64, AGG_MAX_U64,
        AGG_MIN_I64, AGG_MAX_I64 (None: every column a sum), d_out_aggs[j][g] that aggregate of d_cols[j][rowID] over the tuples of
        group g.  The same column may be given twice with different ops.  Costs and everything else as group_sum_cols_dev."""
        n = _u64()
        cols, aggs = self._group_args(d_cols, d_out_aggs)
        rc = self.lib.rhj_group_agg_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, cols, self._ops_arg(ops, len(d_cols)), len(d_cols),
                                             col_rows, C.byref(opts) if opts is not None else None, _addr(d_out_keys),
                                             _addr(d_out_counts), aggs, capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_agg_dev(self, d_R, nR, d_cols=(), ops=None, col_rows=0, d_out_keys=None, d_out_counts=None, d_out_aggs=(), capacity=0,
                      opts=None, allow_overflow=False):
        """rhj_group_agg_dev: group_agg_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n = _u64()
        cols, aggs = self._group_args(d_cols, d_out_aggs)
        rc = self.lib.rhj_group_agg_dev(self.ctx, _addr(d_R), nR, cols, self._ops_arg(ops, len(d_cols)), len(d_cols), col_rows,
                                        C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_counts), aggs,
                                        capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def _group_arg_args(self, d_cols, ops, ties, d_out_vals, d_out_rows):
        """the five host arrays of a group_arg_* call (a missing pointer goes in as NULL: the library answers)"""
        ncols = len(ops)
        k = max(ncols, 1)

        def ptrs(xs):
            xs = list(xs)[:ncols]
            return (_vp * k)(*[_addr(x) for x in xs + [None] * (ncols - len(xs))])
        if ties is not None and len(ties) != ncols:
            raise ValueError(f"{len(ties)} ties for {ncols} columns")
        return (ptrs(d_cols), (C.c_uint32 * k)(*ops), None if ties is None else (C.c_uint32 * k)(*ties), ptrs(d_out_vals),
                ptrs(d_out_rows))

    def group_arg_cols_dev(self, d_valR, d_idR, nR, d_cols=(), ops=(), ties=None, col_rows=0, d_out_keys=None, d_out_counts=None,
                           d_out_vals=(), d_out_rows=(), capacity=0, opts=None, allow_overflow=False):
        """rhj_group_arg_cols_dev: the group-by of group_agg_cols_dev with the ROW of every extreme -- ops[j] one of ARG_MIN_U64,
        ARG_MAX_U64, ARG_MIN_I64, ARG_MAX_I64 (d_out_vals[j][g] the extreme of d_cols[j][rowID] over group g, d_out_rows[j][g] the
        rowID of a tuple of the group that holds it: the smallest under ties[j] == ARG_TIE_FIRST, the largest under ARG_TIE_LAST) or
        ARG_ROW (no column: d_out_rows[j][g] the smallest / largest rowID of the group; d_cols[j] and d_out_vals[j] may be None).
        ties None: every column ARG_TIE_FIRST.  The number of columns is len(ops), at most GROUP_ARG_MAX_COLS.  Everything else as
        group_agg_cols_dev.  Costs: two sweeps and two gathers per value column, one global atomic per tuple that holds its group's
        extreme; a row column one sweep in LDS."""
        n = _u64()
        ops = list(ops)
        cols, opw, tiew, vals, rows = self._group_arg_args(d_cols, ops, None if ties is None else list(ties), d_out_vals, d_out_rows)
        rc = self.lib.rhj_group_arg_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, cols, opw, tiew, len(ops), col_rows,
                                             C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_counts),
                                             vals, rows, capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_arg_dev(self, d_R, nR, d_cols=(), ops=(), ties=None, col_rows=0, d_out_keys=None, d_out_counts=None, d_out_vals=(),
                      d_out_rows=(), capacity=0, opts=None, allow_overflow=False):
        """rhj_group_arg_dev: group_arg_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n = _u64()
        ops = list(ops)
        cols, opw, tiew, vals, rows = self._group_arg_args(d_cols, ops, None if ties is None else list(ties), d_out_vals, d_out_rows)
        rc = self.lib.rhj_group_arg_dev(self.ctx, _addr(d_R), nR, cols, opw, tiew, len(ops), col_rows,
                                        C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_counts), vals, rows,
                                        capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_join_cols_dev(self, d_valR, d_idR, nR, d_valS, d_idS, nS, d_colsR=(), colR_rows=0, d_colsS=(), colS_rows=0, mode=GJ_INNER,
                            d_out_keys=None, d_out_cntR=None, d_out_cntS=None, d_out_sumsR=(), d_out_sumsS=(), capacity=0, opts=None,
                            allow_overflow=False):
        """rhj_group_join_cols_dev: one output row per join value of R join S (uint64 value columns; uint64 rowIDs, or None: the
        rowID of a tuple is its index) -- d_out_keys[g] the value, d_out_cntR[g] / d_out_cntS[g] (each may be None) how many tuples
        of R / S carry it, d_out_sumsR[j][g] / d_out_sumsS[j][g] the sums of d_colsR[j][rowR] / d_colsS[j][rowS] over them mod 2^64
        (at most GROUP_JOIN_MAX_COLS device columns per side, of colR_rows / colS_rows uint64) -- in no particular order; every
        output is uint64[capacity] in HBM.  mode GJ_INNER: the values both sides have; GJ_LEFT: every value of R (cntS may be 0).
        COUNT(*) = cntR*cntS, SUM(r.a) = sumsR*cntS, SUM(s.b) = sumsS*cntR.  d_out_keys None with capacity 0 counts the groups
        only.  Returns the number of groups (with allow_overflow also when it exceeds capacity)"""
        n = _u64()
        colsR, sumsR = self._group_args(d_colsR, d_out_sumsR)
        colsS, sumsS = self._group_args(d_colsS, d_out_sumsS)
        rc = self.lib.rhj_group_join_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), _addr(d_idS), nS,
                                              colsR, len(d_colsR), colR_rows, colsS, len(d_colsS), colS_rows, mode,
                                              C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_cntR),
                                              _addr(d_out_cntS), sumsR, sumsS, capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_join_dev(self, d_R, nR, d_S, nS, d_colsR=(), colR_rows=0, d_colsS=(), colS_rows=0, mode=GJ_INNER, d_out_keys=None,
                       d_out_cntR=None, d_out_cntS=None, d_out_sumsR=(), d_out_sumsS=(), capacity=0, opts=None, allow_overflow=False):
        """rhj_group_join_dev: group_join_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n = _u64()
        colsR, sumsR = self._group_args(d_colsR, d_out_sumsR)
        colsS, sumsS = self._group_args(d_colsS, d_out_sumsS)
        rc = self.lib.rhj_group_join_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, colsR, len(d_colsR), colR_rows, colsS, len(d_colsS),
                                         colS_rows, mode, C.byref(opts) if opts is not None else None, _addr(d_out_keys),
                                         _addr(d_out_cntR), _addr(d_out_cntS), sumsR, sumsS, capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_join_agg_cols_dev(self, d_valR, d_idR, nR, d_valS, d_idS, nS, d_colsR=(), opsR=None, colR_rows=0, d_colsS=(), opsS=None,
                                colS_rows=0, mode=GJ_INNER, d_out_keys=None, d_out_cntR=None, d_out_cntS=None, d_out_aggsR=(),
                                d_out_aggsS=(), capacity=0, opts=None, allow_overflow=False):
        """rhj_group_join_agg_cols_dev: group_join_cols_dev with an aggregate per column and side -- opsR[j] / opsS[j] one of the AGG_*
        (None: every column of that side a sum); d_out_aggsR[j][g] / d_out_aggsS[j][g] the RAW per-side aggregate (a minimum or
        maximum over the pairs of a group is the per-side one as it stands: no product with the other side's count).  Under GJ_LEFT
        a group with cntS == 0 holds the op's identity in S's MIN / MAX columns (MIN_U64: 2^64 - 1, MAX_U64: 0, MIN_I64: INT64_MAX,
        MAX_I64: INT64_MIN) and 0 in its SUM columns: cntS tells which rows these are.  Costs and everything else as
        group_join_cols_dev."""
        n = _u64()
        colsR, aggsR = self._group_args(d_colsR, d_out_aggsR)
        colsS, aggsS = self._group_args(d_colsS, d_out_aggsS)
        rc = self.lib.rhj_group_join_agg_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), _addr(d_idS), nS,
                                                  colsR, self._ops_arg(opsR, len(d_colsR)), len(d_colsR), colR_rows,
                                                  colsS, self._ops_arg(opsS, len(d_colsS)), len(d_colsS), colS_rows, mode,
                                                  C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_cntR),
                                                  _addr(d_out_cntS), aggsR, aggsS, capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_join_agg_dev(self, d_R, nR, d_S, nS, d_colsR=(), opsR=None, colR_rows=0, d_colsS=(), opsS=None, colS_rows=0, mode=GJ_INNER,
                           d_out_keys=None, d_out_cntR=None, d_out_cntS=None, d_out_aggsR=(), d_out_aggsS=(), capacity=0, opts=None,
                           allow_overflow=False):
        """rhj_group_join_agg_dev: group_join_agg_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n = _u64()
        colsR, aggsR = self._group_args(d_colsR, d_out_aggsR)
        colsS, aggsS = self._group_args(d_colsS, d_out_aggsS)
        rc = self.lib.rhj_group_join_agg_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, colsR, self._ops_arg(opsR, len(d_colsR)),
                                             len(d_colsR), colR_rows, colsS, self._ops_arg(opsS, len(d_colsS)), len(d_colsS), colS_rows,
                                             mode, C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_cntR),
                                             _addr(d_out_cntS), aggsR, aggsS, capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_agg_ids_cols_dev(self, d_valR, d_idR, nR, d_cols=(), ops=None, col_rows=0, d_out_keys=None, d_out_counts=None,
                               d_out_aggs=(), capacity=0, d_out_gid=None, gid_rows=0, opts=None, allow_overflow=False):
        """rhj_group_agg_ids_cols_dev: group_agg_cols_dev with the group of every row -- d_out_gid[rowID] = g, the index of the
        tuple's group in this call's d_out_keys (uint64[gid_rows] in HBM; words no rowID names are left as they are; a rowID >=
        gid_rows is never written: RhjError).  Ids are exact group indices also beyond capacity (allow_overflow) and in a count-only
        call.  d_out_gid None: group_agg_cols_dev."""
        n = _u64()
        cols, aggs = self._group_args(d_cols, d_out_aggs)
        rc = self.lib.rhj_group_agg_ids_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, cols, self._ops_arg(ops, len(d_cols)),
                                                 len(d_cols), col_rows, C.byref(opts) if opts is not None else None, _addr(d_out_keys),
                                                 _addr(d_out_counts), aggs, capacity, C.byref(n), _addr(d_out_gid), gid_rows)
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_agg_ids_dev(self, d_R, nR, d_cols=(), ops=None, col_rows=0, d_out_keys=None, d_out_counts=None, d_out_aggs=(), capacity=0,
                          d_out_gid=None, gid_rows=0, opts=None, allow_overflow=False):
        """rhj_group_agg_ids_dev: group_agg_ids_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n = _u64()
        cols, aggs = self._group_args(d_cols, d_out_aggs)
        rc = self.lib.rhj_group_agg_ids_dev(self.ctx, _addr(d_R), nR, cols, self._ops_arg(ops, len(d_cols)), len(d_cols), col_rows,
                                            C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_counts), aggs,
                                            capacity, C.byref(n), _addr(d_out_gid), gid_rows)
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_join_agg_ids_cols_dev(self, d_valR, d_idR, nR, d_valS, d_idS, nS, d_colsR=(), opsR=None, colR_rows=0, d_colsS=(), opsS=None,
                                    colS_rows=0, mode=GJ_INNER, d_out_keys=None, d_out_cntR=None, d_out_cntS=None, d_out_aggsR=(),
                                    d_out_aggsS=(), capacity=0, d_out_gidR=None, gidR_rows=0, d_out_gidS=None, gidS_rows=0, opts=None,
                                    allow_overflow=False):
        """rhj_group_join_agg_ids_cols_dev: group_join_agg_cols_dev with the group of every row of either side -- d_out_gidR[rowR] /
        d_out_gidS[rowS] = g, the index of the tuple's group in this call's d_out_keys, for the tuples whose value has a group;
        every other word of the two arrays (uint64[gidR_rows] / uint64[gidS_rows] in HBM) is all ones when the call returns.  Either
        may be None; a rowID >= its array's length is never written: RhjError that names the array."""
        n = _u64()
        colsR, aggsR = self._group_args(d_colsR, d_out_aggsR)
        colsS, aggsS = self._group_args(d_colsS, d_out_aggsS)
        rc = self.lib.rhj_group_join_agg_ids_cols_dev(self.ctx, _addr(d_valR), _addr(d_idR), nR, _addr(d_valS), _addr(d_idS), nS,
                                                      colsR, self._ops_arg(opsR, len(d_colsR)), len(d_colsR), colR_rows,
                                                      colsS, self._ops_arg(opsS, len(d_colsS)), len(d_colsS), colS_rows, mode,
                                                      C.byref(opts) if opts is not None else None, _addr(d_out_keys), _addr(d_out_cntR),
                                                      _addr(d_out_cntS), aggsR, aggsS, capacity, C.byref(n), _addr(d_out_gidR), gidR_rows,
                                                      _addr(d_out_gidS), gidS_rows)
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def group_join_agg_ids_dev(self, d_R, nR, d_S, nS, d_colsR=(), opsR=None, colR_rows=0, d_colsS=(), opsS=None, colS_rows=0,
                               mode=GJ_INNER, d_out_keys=None, d_out_cntR=None, d_out_cntS=None, d_out_aggsR=(), d_out_aggsS=(),
                               capacity=0, d_out_gidR=None, gidR_rows=0, d_out_gidS=None, gidS_rows=0, opts=None, allow_overflow=False):
        """rhj_group_join_agg_ids_dev: group_join_agg_ids_cols_dev on 16-byte tuples (value = .payload, rowID = .key)"""
        n = _u64()
        colsR, aggsR = self._group_args(d_colsR, d_out_aggsR)
        colsS, aggsS = self._group_args(d_colsS, d_out_aggsS)
        rc = self.lib.rhj_group_join_agg_ids_dev(self.ctx, _addr(d_R), nR, _addr(d_S), nS, colsR, self._ops_arg(opsR, len(d_colsR)),
                                                 len(d_colsR), colR_rows, colsS, self._ops_arg(opsS, len(d_colsS)), len(d_colsS),
                                                 colS_rows, mode, C.byref(opts) if opts is not None else None, _addr(d_out_keys),
                                                 _addr(d_out_cntR), _addr(d_out_cntS), aggsR, aggsS, capacity, C.byref(n),
                                                 _addr(d_out_gidR), gidR_rows, _addr(d_out_gidS), gidS_rows)
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    def keys_pack_dev(self, d_keysR, nR, d_keysS=(), nS=0, d_outR=None, d_outS=None, flags=0):
        """rhj_keys_pack_dev: packs the key columns d_keysR (1 .. KEYS_MAX_COLS device columns of nR uint64) and d_keysS (as many
        columns of nS; none with nS 0: one relation) into d_outR / d_outS (uint64[nR] / uint64[nS] in HBM) such that two rows of
        either side get the same word exactly when all their key columns agree.  Returns the KeyPlan; flags KEYS_NO_UNPACK: one
        without dictionaries (a join needs none)."""
        if nS and len(d_keysS) != len(d_keysR):
            raise ValueError(f"{len(d_keysR)} key columns of R, {len(d_keysS)} of S")
        k = len(d_keysR)
        colsR = (_vp * max(k, 1))(*[_addr(c) for c in d_keysR])
        colsS = (_vp * max(k, 1))(*[_addr(c) for c in d_keysS]) if nS else None
        h = _vp()
        self._chk(self.lib.rhj_keys_pack_dev(self.ctx, k, colsR, nR, colsS, nS, flags, _addr(d_outR), _addr(d_outS), C.byref(h)))
        return KeyPlan(self, h)

    def keys_unpack_dev(self, plan, d_packed, n, d_out_cols):
        """rhj_keys_unpack_dev: d_out_cols[j][i] (the plan's nkeys device columns of n uint64) = key column j of the packed word
        d_packed[i]; a word the plan did not produce is never used as an index: RhjError"""
        if len(d_out_cols) != plan.nkeys:
            raise ValueError(f"{len(d_out_cols)} output columns for a plan of {plan.nkeys} key columns")
        cols = (_vp * max(plan.nkeys, 1))(*[_addr(c) for c in d_out_cols])
        self._chk(self.lib.rhj_keys_unpack_dev(self.ctx, plan.handle, _addr(d_packed), n, cols))

    @staticmethod
    def _key_list(keys, name):
        """a key argument as a list of tensors: a tensor is one column; ValueError for an empty or too long sequence or unequal lengths"""
        cols = list(keys) if isinstance(keys, (list, tuple)) else [keys]
        if not cols:
            raise ValueError(f"{name}: an empty sequence of key tensors")
        if len(cols) > KEYS_MAX_COLS:
            raise ValueError(f"{name}: at most {KEYS_MAX_COLS} key tensors, not {len(cols)}")
        for i, c in enumerate(cols):
            if not hasattr(c, "numel"):
                raise ValueError(f"{name}[{i}]: a 1-D torch tensor of 64-bit integers is needed")
            if c.numel() != cols[0].numel():
                raise ValueError(f"{name}[{i}]: {c.numel()} elements, {name}[0] has {cols[0].numel()}")
        return cols

    def pack_keys(self, keys_R, keys_S=None, keep_dictionaries=True):
        """(packed_R, packed_S or None, plan): composite keys as one key tensor per side.  keys_R / keys_S: sequences of 1 to
        KEYS_MAX_COLS contiguous 1-D 64-bit integer tensors on the engine's device, one length per side, as many on either side
        (keys_S None: one relation); column j of keys_R is compared with column j of keys_S, by bit pattern.  packed_R[i] ==
        packed_S[k] exactly when keys_R[j][i] == keys_S[j][k] for every j (and likewise within a side), so every entry that takes a
        key tensor takes these.  plan: the KeyPlan; plan.unpack(t) gives the columns back for a tensor of packed words
        (keep_dictionaries=False: a plan that cannot -- enough for a join, and no dictionary is kept in HBM).  A different number of
        columns per side, more than KEYS_MAX_COLS, none, or unequal lengths within a side: ValueError before any launch.  Streams
        and completion as join_columns."""
        import torch
        cols_R = self._key_list(keys_R, "keys_R")
        cols_S = self._key_list(keys_S, "keys_S") if keys_S is not None else []
        if keys_S is not None and len(cols_S) != len(cols_R):
            raise ValueError(f"keys_R has {len(cols_R)} key tensors, keys_S has {len(cols_S)}")
        with self._on_torch_stream(cols_R[0], cols_S[0] if cols_S else cols_R[0], cols_R[1:], weights_S=cols_S[1:]) as dev:
            nR, nS = cols_R[0].numel(), cols_S[0].numel() if cols_S else 0
            packed_R = torch.empty(nR, dtype=cols_R[0].dtype, device=dev)
            packed_S = torch.empty(nS, dtype=cols_S[0].dtype, device=dev) if cols_S else None
            plan = self.keys_pack_dev(cols_R, nR, cols_S if nS else (), nS, packed_R if nR else None, packed_S if nS else None,
                                      0 if keep_dictionaries else KEYS_NO_UNPACK)
        return packed_R, packed_S, plan

    def _packed_pair(self, keys_R, keys_S, keep_dictionaries=False):
        """(packed_R, packed_S, plan) when either key argument is a sequence of tensors, None when both are single tensors"""
        if not isinstance(keys_R, (list, tuple)) and not isinstance(keys_S, (list, tuple)):
            return None
        return self.pack_keys(keys_R, keys_S, keep_dictionaries)

    @contextlib.contextmanager
    def _on_torch_stream(self, keys_R, keys_S, weights=(), weights_on_S=False, weights_S=()):
        """What join_columns, outer_join_columns, semi_join_columns, join_sum_columns, join_multiplicity_columns, group_by_columns (keys_S = keys_R) and join_group_by_columns (weights_S: further tensors, each as long as keys_S) share.  keys_R / keys_S: contiguous 1-D 64-bit integer torch tensors on this
        engine's device (ValueError otherwise); weights: tensors of the same kind, each as long as keys_R (weights_on_S: as keys_S).  The body runs ordered behind the work torch has queued on its current stream: on a
        stream of its own (torch.cuda.stream(s)) the engine runs on that stream for the length of the body; torch's default stream
        has no handle to hand over (its raw value is 0, which rhj_set_stream reads as "the context's own stream"), so there the call
        waits on the host for the stream first and runs on the stream the engine has.  Either way the results are complete when
        the block is left, and a stream bound earlier with set_stream is bound again.  Yields the tensors' device."""
        import torch
        ints = tuple(t for t in (torch.int64, getattr(torch, "uint64", None)) if t is not None)
        for name, k in ((("keys_R", keys_R), ("keys_S", keys_S)) + tuple((f"weights[{i}]", w) for i, w in enumerate(weights)) +
                        tuple((f"weights_S[{i}]", w) for i, w in enumerate(weights_S))):
            if not isinstance(k, torch.Tensor) or k.dtype not in ints or k.dim() != 1:
                raise ValueError(f"{name}: a 1-D torch tensor of 64-bit integers is needed")
            if k.device.type != "cuda" or (k.device.index or 0) != self.device:
                raise ValueError(f"{name}: the tensor must live on the engine's device (cuda:{self.device}), not {k.device}")
            if not k.is_contiguous():
                raise ValueError(f"{name}: the tensor must be contiguous")
        side, keys = ("S", keys_S) if weights_on_S else ("R", keys_R)
        for i, w in enumerate(weights):
            if w.numel() != keys.numel():
                raise ValueError(f"weights[{i}]: {w.numel()} elements for {keys.numel()} keys of {side}")
        for i, w in enumerate(weights_S):
            if w.numel() != keys_S.numel():
                raise ValueError(f"weights_S[{i}]: {w.numel()} elements for {keys_S.numel()} keys of S")
        dev = keys_R.device
        with torch.cuda.device(dev):
            torch_stream = torch.cuda.current_stream(dev)
            cur, before = torch_stream.cuda_stream, self.bound_stream
            if cur == 0:
                torch_stream.synchronize()      # the keys are written, and no queued torch work still uses a block torch.empty may hand out
            elif cur != before:
                self.set_stream(cur)
            try:
                yield dev
            finally:
                if cur != 0 and cur != before:
                    self.set_stream(before)     # (synchronises torch's stream first: the results are complete)
                else:
                    self.sync()

    def join_columns(self, keys_R, keys_S):
        """Equi-join of two key tensors: (idx_R, idx_S), int64 tensors with keys_R[idx_R[i]] == keys_S[idx_S[i]] for every i,
        every matching index pair exactly once, in no particular order.  keys_R / keys_S: contiguous 1-D 64-bit integer torch
        tensors on this engine's device, compared by bit pattern.  Count, allocate, join -- ordered behind the work torch has queued
        on its current stream (see _on_torch_stream); the results are complete when it returns, and a stream bound earlier with
        set_stream is bound again.
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); rows match when every column agrees."""
        packed = self._packed_pair(keys_R, keys_S)
        if packed is not None:
            packed[2].close()                      # (a join needs no dictionary: the plan holds nothing)
            return self.join_columns(packed[0], packed[1])

        import torch
        with self._on_torch_stream(keys_R, keys_S) as dev:
            nR, nS = keys_R.numel(), keys_S.numel()
            count = self.join_cols_dev(keys_R, None, nR, keys_S, None, nS) if nR and nS else 0
            idx_R = torch.empty(count, dtype=torch.int64, device=dev)
            idx_S = torch.empty(count, dtype=torch.int64, device=dev)
            if count:
                pairs = torch.empty((count, 2), dtype=torch.int64, device=dev)
                got = self.join_cols_dev(keys_R, None, nR, keys_S, None, nS, pairs, count)
                assert got == count, (got, count)
                self.pairs_split(pairs, count, idx_R, idx_S)
        return idx_R, idx_S

    def semi_join_columns(self, keys_R, keys_S, anti=False):
        """idx_R, an int64 tensor: every i for which keys_R[i] occurs in keys_S -- with anti=True, does NOT occur -- exactly once,
        in no particular order, however often the key is repeated in keys_S (torch.isin as indices; EXISTS / NOT EXISTS).  Tensors,
        streams and completion as join_columns.  Count, allocate, fill.  (For a left, right or full outer join see
        outer_join_columns: one call, both sides partitioned once.)
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); rows match when every column agrees."""
        packed = self._packed_pair(keys_R, keys_S)
        if packed is not None:
            packed[2].close()                      # (a join needs no dictionary: the plan holds nothing)
            return self.semi_join_columns(packed[0], packed[1], anti)

        import torch
        kind = ANTI if anti else SEMI
        with self._on_torch_stream(keys_R, keys_S) as dev:
            nR, nS = keys_R.numel(), keys_S.numel()
            count = self.semi_join_cols_dev(keys_R, None, nR, keys_S, nS, kind) if nR else 0
            idx_R = torch.empty(count, dtype=torch.int64, device=dev)
            if count:
                got = self.semi_join_cols_dev(keys_R, None, nR, keys_S, nS, kind, idx_R, count)
                assert got == count, (got, count)
        return idx_R

    def outer_join_columns(self, keys_R, keys_S, how="left"):
        """Outer equi-join of two key tensors: (idx_R, idx_S), int64 tensors of one length.  First the rows of join_columns; then,
        for how "left" or "full", one row (i, -1) per i whose keys_R[i] does not occur in keys_S; then, for how "right" or "full", one
        row (-1, j) per j whose keys_S[j] does not occur in keys_R (merge(how=..), how="full" being pandas' "outer"; LEFT / RIGHT /
        FULL OUTER JOIN).  Order inside each of the three sections is unspecified.  Tensors, streams and completion as join_columns.
        Count, allocate, fill.
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); rows match when every column agrees."""
        packed = self._packed_pair(keys_R, keys_S)
        if packed is not None:
            packed[2].close()                      # (a join needs no dictionary: the plan holds nothing)
            return self.outer_join_columns(packed[0], packed[1], how)

        import torch
        modes = {"left": OUTER_LEFT, "right": OUTER_RIGHT, "full": OUTER_FULL}
        if not isinstance(how, str) or how not in modes:
            raise ValueError(f"how: one of 'left', 'right', 'full' is needed, not {how!r}")
        with self._on_torch_stream(keys_R, keys_S) as dev:
            nR, nS = keys_R.numel(), keys_S.numel()
            count, _ = self.outer_join_cols_dev(keys_R, None, nR, keys_S, None, nS, modes[how])
            idx_R = torch.empty(count, dtype=torch.int64, device=dev)
            idx_S = torch.empty(count, dtype=torch.int64, device=dev)
            if count:
                pairs = torch.empty((count, 2), dtype=torch.int64, device=dev)
                got, _ = self.outer_join_cols_dev(keys_R, None, nR, keys_S, None, nS, modes[how], pairs, count)
                assert got == count, (got, count)
                self.pairs_split(pairs, count, idx_R, idx_S)
        return idx_R, idx_S

    def join_sum_columns(self, keys_R, keys_S, weights=()):
        """(count, sums): count = the number of index pairs (i, j) with keys_R[i] == keys_S[j], sums[k] = the sum of weights[k][i]
        over those pairs mod 2^64 (SELECT COUNT(*), SUM(r.x) FROM R JOIN S USING (key)), as Python ints in [0, 2^64) -- without the
        pairs, in time linear in the inputs however often a key repeats.  weights: up to SUM_MAX_COLS contiguous 1-D 64-bit integer
        tensors of len(keys_R) on the engine's device (int64 weights: read the sums as two's complement).  Tensors, streams and
        completion as join_columns.
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); rows match when every column agrees."""
        packed = self._packed_pair(keys_R, keys_S)
        if packed is not None:
            packed[2].close()                      # (a join needs no dictionary: the plan holds nothing)
            return self.join_sum_columns(packed[0], packed[1], weights)

        weights = tuple(weights)
        if len(weights) > SUM_MAX_COLS:
            raise ValueError(f"at most {SUM_MAX_COLS} weight tensors per call, not {len(weights)}")
        with self._on_torch_stream(keys_R, keys_S, weights):
            nR, nS = keys_R.numel(), keys_S.numel()
            return self.join_sum_cols_dev(keys_R, None, nR, keys_S, nS, weights, nR)

    def join_multiplicity_columns(self, keys_R, keys_S, weights_S=None):
        """(mult, total): mult[i] = the number of j with keys_S[j] == keys_R[i] -- with weights_S, the sum of weights_S[j] over
        those j, mod 2^64 -- as an int64 tensor of len(keys_R) on the keys' device that holds the bit pattern of the uint64 result
        (the degree of every key; value_counts looked up per row); total = the sum of mult mod 2^64 as a Python int in [0, 2^64),
        unweighted the number of pairs join_columns would return.  No pair is written: linear in the inputs however often a key
        repeats.  weights_S: a contiguous 1-D 64-bit integer tensor of len(keys_S) on the engine's device.  Tensors, streams and
        completion as join_columns.
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); rows match when every column agrees."""
        packed = self._packed_pair(keys_R, keys_S)
        if packed is not None:
            packed[2].close()                      # (a join needs no dictionary: the plan holds nothing)
            return self.join_multiplicity_columns(packed[0], packed[1], weights_S)

        import torch
        weights = () if weights_S is None else (weights_S,)
        with self._on_torch_stream(keys_R, keys_S, weights, weights_on_S=True) as dev:
            nR, nS = keys_R.numel(), keys_S.numel()
            mult = torch.empty(nR, dtype=torch.int64, device=dev)
            total = self.join_mult_cols_dev(keys_R, None, nR, keys_S, None, nS, mult if nR else None, nR, weights_S, nS)
        return mult, total

    def lookup_columns(self, keys_R, keys_S, values_S=(), fill=0, which="first"):
        """(idx_S, matched, values): idx_S[i] = the smallest (which="first") or largest (which="last") j with keys_S[j] ==
        keys_R[i], -1 where there is none -- an int64 tensor of len(keys_R) on the keys' device, aligned with keys_R
        (Index.get_indexer, Series.map, merge(how="left") against a dimension table); matched = how many rows found a partner, a
        Python int; values = one int64 tensor of len(keys_R) per tensor of values_S: values[k][i] = values_S[k][idx_S[i]], or fill
        where idx_S[i] == -1.  No pair is written: linear in the inputs, 8 bytes out per row of R, bit-exact from run to run also
        where S carries a key twice.  values_S: up to LOOKUP_MAX_COLS contiguous 1-D 64-bit integer tensors of len(keys_S) on the
        engine's device; fill: an int, or one int per tensor of values_S.  matched == the total of join_multiplicity_columns on the
        same keys says that no key of R occurs twice in S (validate="m:1").  A wrong which, tensor, length or number of value
        tensors: ValueError before any launch.  Tensors, streams and completion as join_columns.
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); rows match when every column agrees."""
        modes = {"first": LOOKUP_FIRST, "last": LOOKUP_LAST}
        if not isinstance(which, str) or which not in modes:
            raise ValueError(f"which: one of 'first', 'last' is needed, not {which!r}")
        values_S = tuple(values_S)
        if len(values_S) > LOOKUP_MAX_COLS:
            raise ValueError(f"at most {LOOKUP_MAX_COLS} value tensors per call, not {len(values_S)}")
        fills = [fill] * len(values_S) if isinstance(fill, int) else list(fill) if isinstance(fill, (list, tuple)) else [None]
        if len(fills) != len(values_S) or not all(isinstance(f, int) for f in fills):
            raise ValueError(f"fill: an int, or one int per tensor of values_S ({len(values_S)}), is needed")
        packed = self._packed_pair(keys_R, keys_S)
        if packed is not None:
            packed[2].close()                      # (a join needs no dictionary: the plan holds nothing)
            return self.lookup_columns(packed[0], packed[1], values_S, fills, which)

        import torch
        with self._on_torch_stream(keys_R, keys_S, weights_S=values_S) as dev:
            nR, nS = keys_R.numel(), keys_S.numel()
            idx_S = torch.empty(nR, dtype=torch.int64, device=dev)
            matched = self.lookup_cols_dev(keys_R, None, nR, keys_S, None, nS, idx_S if nR else None, nR, modes[which])
            values = [torch.empty(nR, dtype=torch.int64, device=dev) for _ in values_S]
            if values and nR:
                self.gather_cols_fill(values_S, nS, idx_S, nR, fills, values)
        return idx_S, matched, values

    def group_by_columns(self, keys, weights=(), ops=None):
        """(unique_keys, counts, sums): the distinct values of keys, how often each occurs, and per tensor of weights the sum of
        weights[k][i] over the rows i that carry the value, mod 2^64 (SELECT key, COUNT(*), SUM(x) FROM R GROUP BY key; torch.unique
        with return_counts + index_add_) -- int64 tensors of one length on the keys' device, sums a list of len(weights) of them,
        group g of all at index g, groups in no particular order.  keys: a contiguous 1-D 64-bit integer tensor on the engine's
        device; weights: up to GROUP_MAX_COLS tensors of the same kind and length.  Negative keys and weights are bit patterns: a
        key comes back as it went in, an int64 sum is the two's complement sum.  The outputs are allocated at len(keys), the upper
        bound, and returned as the views [:groups].  Streams and completion as join_columns.
        ops: None -- every tensor of weights is summed (rhj_group_sum_cols_dev) --, or one of "sum" | "min" | "max" per tensor of
        weights (SELECT key, MIN(x), MAX(x), SUM(y) ..; scatter_reduce_ with amin / amax): sums[k] is then that aggregate of weights[k]
        over the group, minimum and maximum of the int64 values (rhj_group_agg_cols_dev; the same tensor may be given twice).  A
        wrong length or name: ValueError before any launch.  Costs as for sums, whatever the ops.
        The group of every row beside them: group_by_columns_with_inverse.
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors is packed first (pack_keys); unique_keys is then a list of as many tensors."""
        return self._group_by_columns(keys, weights, ops, False)

    def group_by_columns_with_inverse(self, keys, weights=(), ops=None):
        """(unique_keys, counts, sums, inverse): group_by_columns with torch.unique's return_inverse -- inverse an int64 tensor of
        len(keys) with unique_keys[inverse] == keys, the group every row belongs to, so that whatever the ops do not cover (a mean,
        a float sum, an argmin, the group's total broadcast back to its rows) is a direct-indexed torch op behind one call.  The
        order of groups is unspecified and may differ from run to run: inverse goes with this call's unique_keys.  Everything else
        as group_by_columns (rhj_group_agg_ids_cols_dev: one more sweep per class and one scattered 8-byte store per row).
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors is packed first (pack_keys); unique_keys is then a list of as many tensors."""
        return self._group_by_columns(keys, weights, ops, True)

    def _group_by_columns(self, keys, weights, ops, return_inverse):
        import torch
        if isinstance(keys, (list, tuple)):
            packed, _, plan = self.pack_keys(keys)
            out = self._group_by_columns(packed, weights, ops, return_inverse)
            uniques = plan.unpack(out[0])
            plan.close()
            return (uniques,) + out[1:]
        weights = tuple(weights)
        if len(weights) > GROUP_MAX_COLS:
            raise ValueError(f"at most {GROUP_MAX_COLS} weight tensors per call, not {len(weights)}")
        if ops is not None:
            ops = _agg_ops(ops, len(weights), "ops")
        with self._on_torch_stream(keys, keys, weights) as dev:
            n = keys.numel()
            out_keys = torch.empty(n, dtype=torch.int64, device=dev)
            counts = torch.empty(n, dtype=torch.int64, device=dev)
            sums = [torch.empty(n, dtype=torch.int64, device=dev) for _ in weights]
            inverse = torch.empty(n, dtype=torch.int64, device=dev) if return_inverse else None
            if not n:
                groups = 0
            elif return_inverse:
                groups = self.group_agg_ids_cols_dev(keys, None, n, weights, ops, n, out_keys, counts, sums, n, inverse, n)
            elif ops is None:
                groups = self.group_sum_cols_dev(keys, None, n, weights, n, out_keys, counts, sums, n)
            else:
                groups = self.group_agg_cols_dev(keys, None, n, weights, ops, n, out_keys, counts, sums, n)
        if return_inverse:
            return out_keys[:groups], counts[:groups], [s[:groups] for s in sums], inverse
        return out_keys[:groups], counts[:groups], [s[:groups] for s in sums]

    def group_by_columns_arg(self, keys, by, ops, ties="first"):
        """(unique_keys, counts, vals, rows): group_by_columns with the ROW that holds every minimum / maximum (pandas groupby.idxmin /
        idxmax; SELECT DISTINCT ON (key) .. ORDER BY key, t DESC; the latest record per key) -- vals[k][g] the extreme of by[k] over
        group g, rows[k][g] the index i of a row of the group with by[k][i] == vals[k][g]; int64 tensors, groups in no particular
        order.  by: up to GROUP_ARG_MAX_COLS contiguous 1-D 64-bit integer tensors as long as keys (the same tensor may be given
        several times), None where the op is "row".  ops: per tensor "min" | "max" (the int64 values), "min_u64" | "max_u64" (the
        words as unsigned), or "row": no tensor, rows[k][g] the first / last row of the group and vals[k] None.  ties: "first" |
        "last", one for all or one per column: among the rows that hold the extreme the smallest / the largest index.  A wrong name
        or length, or a column too many: ValueError before any device use.  Everything else as group_by_columns
        (rhj_group_arg_cols_dev: two sweeps per value column).
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors is packed first (pack_keys); unique_keys is then a list of as many tensors."""
        import torch
        by = list(by)
        opw, tiew = _arg_ops(by, ops, ties)
        if isinstance(keys, (list, tuple)):
            packed, _, plan = self.pack_keys(keys)
            out = self.group_by_columns_arg(packed, by, ops, ties)
            uniques = plan.unpack(out[0])
            plan.close()
            return (uniques,) + out[1:]
        with self._on_torch_stream(keys, keys, tuple(b for b in by if b is not None)) as dev:
            n = keys.numel()
            out_keys = torch.empty(n, dtype=torch.int64, device=dev)
            counts = torch.empty(n, dtype=torch.int64, device=dev)
            vals = [None if b is None else torch.empty(n, dtype=torch.int64, device=dev) for b in by]
            rows = [torch.empty(n, dtype=torch.int64, device=dev) for _ in by]
            groups = self.group_arg_cols_dev(keys, None, n, by, opw, tiew, n, out_keys, counts, vals, rows, n) if n else 0
        return out_keys[:groups], counts[:groups], [None if v is None else v[:groups] for v in vals], [r[:groups] for r in rows]

    def drop_duplicates_columns(self, keys, keep="first"):
        """idx: pandas drop_duplicates(keep="first" | "last") -- the int64 indices of the rows kept, one per distinct value of keys (its
        first or its last row), SORTED ASCENDING, so keys[idx] is in the original order.  One group_by_columns_arg call with a single
        "row" column and one torch.sort over the groups.  keep other than "first" / "last": ValueError before any device use.  keys as
        group_by_columns_arg (composite keys: a list of tensors; index idx into each)."""
        import torch
        if not isinstance(keep, str) or keep not in _TIE_BY_NAME:
            raise ValueError(f"keep: 'first' or 'last', not {keep!r}")
        rows = self.group_by_columns_arg(keys, [None], ["row"], keep)[3][0]
        return torch.sort(rows).values

    def sort_cols_dev(self, d_keys, d_rows, n, flags=0, d_out_keys=None, d_out_rows=None):
        """rhj_sort_cols_dev: the stable sort of the tuples (d_keys[i], d_rows[i]) -- d_rows None: rowID = i -- by key word, unsigned
        or (SORT_I64) as int64, ascending or (SORT_DESC) descending, ties in input order either way; d_out_keys / d_out_rows:
        uint64[n] in HBM, either may be None (a keys-only sort, an argsort)"""
        self._chk(self.lib.rhj_sort_cols_dev(self.ctx, _addr(d_keys), _addr(d_rows), n, flags, _addr(d_out_keys), _addr(d_out_rows)))

    def sort_dev(self, d_R, n, flags=0, d_out=None):
        """rhj_sort_dev: ... of n 16-byte tuples (value = .payload, rowID = .key) into d_out"""
        self._chk(self.lib.rhj_sort_dev(self.ctx, _addr(d_R), n, flags, _addr(d_out)))

    @staticmethod
    def _sort_args(keys, descending, unsigned, values=()):
        """(key tensors, one descending flag per tensor, value tensors) of sort_columns / argsort_columns; ValueError before any device use"""
        many = isinstance(keys, (list, tuple))
        cols = list(keys) if many else [keys]
        if not cols:
            raise ValueError("keys: an empty sequence of key tensors")
        if len(cols) > KEYS_MAX_COLS:
            raise ValueError(f"keys: at most {KEYS_MAX_COLS} key tensors, not {len(cols)}")
        if isinstance(descending, bool):
            desc = [descending] * len(cols)
        elif many and isinstance(descending, (list, tuple)) and all(isinstance(d, bool) for d in descending):
            if len(descending) != len(cols):
                raise ValueError(f"descending: one bool, or one per key tensor ({len(cols)}), not {len(descending)}")
            desc = list(descending)
        else:
            raise ValueError(f"descending: a bool{', or one bool per key tensor,' if many else ''} is needed, not {descending!r}")
        if not isinstance(unsigned, bool):
            raise ValueError(f"unsigned: a bool is needed, not {unsigned!r}")
        values = tuple(values)
        if len(values) > LOOKUP_MAX_COLS:
            raise ValueError(f"at most {LOOKUP_MAX_COLS} value tensors per call, not {len(values)}")
        return cols, desc, values

    def _sort_tensors(self, cols, values, many):
        """the tensors of a sort under the names the caller gave them: ValueError for one that is not a contiguous 1-D 64-bit integer
        tensor on the engine's device, or not as long as the first key tensor (_on_torch_stream would say keys_R / weights[i])"""
        import torch
        ints = tuple(t for t in (torch.int64, getattr(torch, "uint64", None)) if t is not None)
        named = [(f"keys[{i}]" if many else "keys", c) for i, c in enumerate(cols)] + [(f"values[{i}]", v) for i, v in enumerate(values)]
        for name, k in named:
            if not isinstance(k, torch.Tensor) or k.dtype not in ints or k.dim() != 1:
                raise ValueError(f"{name}: a 1-D torch tensor of 64-bit integers is needed")
            if k.device.type != "cuda" or (k.device.index or 0) != self.device:
                raise ValueError(f"{name}: the tensor must live on the engine's device (cuda:{self.device}), not {k.device}")
            if not k.is_contiguous():
                raise ValueError(f"{name}: the tensor must be contiguous")
            if k.numel() != cols[0].numel():
                raise ValueError(f"{name}: {k.numel()} elements, {named[0][0]} has {cols[0].numel()}")

    def _sort_chain(self, cols, desc, unsigned, values, want_keys):
        """ORDER BY cols[0], cols[1], ..: a chain of stable sorts, last key first, each later one over the key gathered through the
        permutation so far, with that permutation as its rows.  (sorted key tensors or None, perm, gathered values)"""
        import torch
        with self._on_torch_stream(cols[0], cols[0], tuple(cols[1:]) + values) as dev:       # (the tensors: checked by _sort_tensors)
            n = cols[0].numel()
            view = 0 if unsigned else SORT_I64
            perm, first = None, None
            for j in range(len(cols) - 1, -1, -1):
                src = cols[j]
                if perm is not None and n:
                    src = torch.empty(n, dtype=cols[j].dtype, device=dev)
                    self.gather_u64(cols[j], perm, n, src)
                nxt = torch.empty(n, dtype=torch.int64, device=dev)
                if j == 0 and want_keys:
                    first = torch.empty(n, dtype=cols[0].dtype, device=dev)
                if n:
                    self.sort_cols_dev(src, perm, n, view | (SORT_DESC if desc[j] else 0), first if j == 0 else None, nxt)
                perm = nxt
            out_keys = None
            if want_keys:
                out_keys = [first] + [torch.empty(n, dtype=c.dtype, device=dev) for c in cols[1:]]
                if n and len(cols) > 1:
                    self.gather_cols_fill(cols[1:], n, perm, n, [0] * (len(cols) - 1), out_keys[1:])
            gathered = [torch.empty(n, dtype=v.dtype, device=dev) for v in values]
            if n and values:
                self.gather_cols_fill(values, n, perm, n, [0] * len(values), gathered)
        return out_keys, perm, gathered

    def sort_columns(self, keys, values=(), descending=False, unsigned=False):
        """(sorted_keys, perm, gathered_values): ORDER BY on a key tensor -- sorted_keys = keys[perm] in ascending (descending=True:
        descending) order, perm the STABLE argsort as an int64 tensor (rows with equal keys keep their input order in both
        directions, as torch.sort(stable=True, descending=..)), gathered_values one tensor per tensor of values: values[k][perm].
        keys: a contiguous 1-D 64-bit integer tensor on the engine's device, ordered as int64 (unsigned=True: the words as uint64);
        values: up to LOOKUP_MAX_COLS tensors of the same kind and length (rhj_gather_cols_fill).  A stable LSD radix sort whose number of passes
        follows the width of the key's value range, not 64 bits (rhj_sort_cols_dev).
        A list of 1 to KEYS_MAX_COLS key tensors is ORDER BY k0, k1, ..: descending is then one bool or one per tensor, sorted_keys a list
        of as many tensors; it runs as a chain of stable sorts, last key first.  A wrong descending length, more than KEYS_MAX_COLS
        key tensors, too many values or a non-bool flag: ValueError before any device use.  Streams and completion as join_columns."""
        cols, desc, values = self._sort_args(keys, descending, unsigned, values)
        self._sort_tensors(cols, values, isinstance(keys, (list, tuple)))
        out_keys, perm, gathered = self._sort_chain(cols, desc, unsigned, values, True)
        return (out_keys if isinstance(keys, (list, tuple)) else out_keys[0]), perm, gathered

    def argsort_columns(self, keys, descending=False, unsigned=False):
        """perm: sort_columns' permutation alone (torch.argsort(stable=True)); no key output is passed, so the last pass stores 8
        bytes per row.  Arguments and errors as sort_columns."""
        cols, desc, _ = self._sort_args(keys, descending, unsigned)
        self._sort_tensors(cols, (), isinstance(keys, (list, tuple)))
        return self._sort_chain(cols, desc, unsigned, (), False)[1]

    def topk_cols_dev(self, d_keys, d_rows, n, k, flags=0, d_out_keys=None, d_out_rows=None, want_kth=False):
        """rhj_topk_cols_dev: the first min(k, n) tuples of what sort_cols_dev would write, ties in input order also at the cut;
        d_out_keys / d_out_rows: uint64[min(k, n)] in HBM, either may be None, both only with want_kth (a pure selection).
        want_kth: returns (key word, row word) of the tuple of rank min(k, n) - 1, or None when n or k is 0; else returns None"""
        kth = (_u64 * 2)() if want_kth else None
        self._chk(self.lib.rhj_topk_cols_dev(self.ctx, _addr(d_keys), _addr(d_rows), n, k, flags, _addr(d_out_keys), _addr(d_out_rows), kth))
        return (kth[0], kth[1]) if want_kth and n and k else None

    def topk_dev(self, d_R, n, k, flags=0, d_out=None, want_kth=False):
        """rhj_topk_dev: ... of n 16-byte tuples (value = .payload, rowID = .key) into d_out; the k-th tuple as (value, rowID)"""
        kth = (_u64 * 2)() if want_kth else None
        self._chk(self.lib.rhj_topk_dev(self.ctx, _addr(d_R), n, k, flags, _addr(d_out), kth))
        return (kth[0], kth[1]) if want_kth and n and k else None

    @staticmethod
    def _topk_args(keys, k, descending, unsigned, values=()):
        """ValueError before any device use: the arguments of topk_columns / kth_value_columns that are not tensors"""
        if isinstance(keys, (list, tuple)):
            raise ValueError("keys: one key tensor is needed, not a list -- ORDER BY k0, k1, .. LIMIT k is sort_columns(keys, ..) and a slice")
        if isinstance(k, bool) or not isinstance(k, int):
            raise ValueError(f"k: an int is needed, not {k!r}")
        if k < 0:
            raise ValueError(f"k: a count of rows is needed, not {k}")
        if not isinstance(descending, bool):
            raise ValueError(f"descending: a bool is needed, not {descending!r}")
        if not isinstance(unsigned, bool):
            raise ValueError(f"unsigned: a bool is needed, not {unsigned!r}")
        values = tuple(values)
        if len(values) > LOOKUP_MAX_COLS:
            raise ValueError(f"at most {LOOKUP_MAX_COLS} value tensors per call, not {len(values)}")
        return values

    def topk_columns(self, keys, k, values=(), descending=False, unsigned=False):
        """(top_keys, idx, gathered_values): ORDER BY keys LIMIT k -- the first min(k, len(keys)) entries of what sort_columns returns
        for the same arguments, without sorting the column: top_keys sorted ascending (descending=True: the k largest, descending),
        idx their rows as an int64 tensor, ties in input order also at the cut (torch.sort(stable=True)[:k]), gathered_values one
        tensor per tensor of values: values[j][idx].  A radix select, a stable compaction and a sort of what is left
        (rhj_topk_cols_dev).  keys: ONE contiguous 1-D 64-bit integer tensor on the engine's device (a list: ValueError, see
        sort_columns); k: an int >= 0.  Every ValueError comes before any device use.  Streams and completion as join_columns."""
        import torch
        values = self._topk_args(keys, k, descending, unsigned, values)
        self._sort_tensors([keys], values, False)
        with self._on_torch_stream(keys, keys, values) as dev:
            n = keys.numel()
            m = min(k, n)
            top = torch.empty(m, dtype=keys.dtype, device=dev)
            idx = torch.empty(m, dtype=torch.int64, device=dev)
            if m:
                self.topk_cols_dev(keys, None, n, k, (0 if unsigned else SORT_I64) | (SORT_DESC if descending else 0), top, idx)
            gathered = [torch.empty(m, dtype=v.dtype, device=dev) for v in values]
            if m and values:
                self.gather_cols_fill(values, n, idx, m, [0] * len(values), gathered)
        return top, idx, gathered

    def kth_value_columns(self, keys, k, descending=False, unsigned=False):
        """(value, row): the k-th smallest (descending=True: k-th largest) key and the row that holds it, as Python ints -- k is
        1-based as in torch.kthvalue; among equal keys the row is the one a stable sort puts at rank k - 1.  A pure selection: nothing
        of size k is written (rhj_topk_cols_dev with out_kth alone).  value is an int64 value unless unsigned.  k < 1 or k > len(keys):
        ValueError; every ValueError comes before any device use."""
        self._topk_args(keys, k, descending, unsigned)
        if k < 1:
            raise ValueError(f"k: a rank from 1 (as torch.kthvalue) is needed, not {k}")
        self._sort_tensors([keys], (), False)
        if k > keys.numel():
            raise ValueError(f"k: 1 .. {keys.numel()} (the length of keys) is needed, not {k}")
        with self._on_torch_stream(keys, keys, ()):
            value, row = self.topk_cols_dev(keys, None, keys.numel(), k, (0 if unsigned else SORT_I64) | (SORT_DESC if descending else 0),
                                            None, None, want_kth=True)
        return (value if unsigned or value < 1 << 63 else value - (1 << 64)), row

    def window_cols_dev(self, d_part, d_order, n, flags=0, ops=(), args=None, d_cols=None, d_outs=()):
        """rhj_window_cols_dev: per row a value from the rows before it in its partition (rows with the same d_part word; None: one
        partition), ordered by d_order under flags (SORT_I64, SORT_DESC; None: input order), ties in input order -- ops[j] one of
        WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_LAG_ROW / WIN_LEAD_ROW (args[j]: the offset >= 1; args None: 1; NO_ROW where
        there is no such row), WIN_CUMSUM, WIN_CUMMIN_U64 / WIN_CUMMAX_U64 / WIN_CUMMIN_I64 / WIN_CUMMAX_I64 (of d_cols[j], over the
        rows up to and including this one: ROWS UNBOUNDED PRECEDING).  d_outs[j]: uint64[n] in HBM, aligned with the rows.  The
        number of ops is len(ops), at most WINDOW_MAX_OPS.  Returns the number of partitions.  (A sequence that is None goes in as
        NULL: the library answers.)"""
        k = len(ops) if ops is not None else 0
        opw = (C.c_uint32 * max(k, 1))(*[int(o) for o in ops]) if ops is not None else None
        argw = (_u64 * max(k, 1))(*[int(a) for a in args]) if args is not None else None
        cols = (_vp * max(k, 1))(*[_addr(c) for c in d_cols]) if d_cols is not None else None
        outs = (_vp * max(k, 1))(*[_addr(o) for o in d_outs]) if d_outs is not None else None
        parts = _u64()
        self._chk(self.lib.rhj_window_cols_dev(self.ctx, _addr(d_part), _addr(d_order), n, flags, opw, argw, cols, k, outs, C.byref(parts)))
        return parts.value

    def window_columns(self, partition_by, order_by=None, values=(), ops=("row_number",), descending=False, unsigned=False, offsets=None,
                       fill=0):
        """[out_0, out_1, ..]: window functions over the rows of a table -- one int64 tensor per op, ALIGNED WITH THE ROWS (not in
        sorted order).  Rows with equal partition_by form a partition; inside it they are ordered by order_by as int64 (unsigned=True:
        the words as uint64), ascending (descending=True: descending), rows with equal order keys in input order in both directions --
        every result is defined and the same from run to run.  order_by None: input order.  partition_by: None (one partition), a
        contiguous 1-D 64-bit integer tensor on the engine's device, or a list of 1 to KEYS_MAX_COLS of them (packed first, as
        group_by_columns does).  ops, with q the 0-based position of a row in its partition:
          "row_number"  q + 1 (pandas groupby.cumcount() + 1)            "rank"  1 + the rows with a strictly earlier order key (rank(method="min"))
          "dense_rank"  1 + the distinct earlier order keys               "cumsum"  the running sum mod 2^64 of values[j]
          "cummin" / "cummax"  the running minimum / maximum of values[j] as int64;  "cummin_u64" / "cummax_u64": of the words as uint64
          "lag" / "lead"  values[j] None: the index of the row offsets[j] (default 1) positions before / behind in the partition, -1
                          where there is none; values[j] a tensor: that tensor at that row, fill where there is none (groupby.shift)
        The running aggregates cover the rows up to and including the current one (ROWS UNBOUNDED PRECEDING), not its later peers.
        values[j] is None for an op without a column (values=() : every op without one).  At most WINDOW_MAX_OPS ops per call.
        ORDER BY a, b inside the partitions: _, perm, (k2, ..) = sort_columns([k, a, b], values=[k, ..]) first, then window_columns(k2,
        None, ..) on the gathered tensors -- the results are then aligned with the sorted rows; out[perm] = result puts them back.
        An unknown op, more than WINDOW_MAX_OPS ops, a length mismatch among values / ops / offsets, a non-bool flag, an offset < 1,
        descending=True without order_by: ValueError before any device use.  One rhj_window_cols_dev call, and one rhj_gather_cols_fill
        per lagged payload.  Streams and completion as join_columns."""
        import torch
        opw, values, offs = _window_args(order_by, values, ops, descending, unsigned, offsets, fill)
        if isinstance(partition_by, (list, tuple)):
            packed, _, plan = self.pack_keys(partition_by, keep_dictionaries=False)
            plan.close()
            partition_by = packed
        named = [("partition_by", partition_by), ("order_by", order_by)] + [(f"values[{j}]", v) for j, v in enumerate(values)]
        named = [(name, t) for name, t in named if t is not None]
        if not named:
            raise ValueError("partition_by, order_by and values are all None: the number of rows is unknown")
        ints = tuple(t for t in (torch.int64, getattr(torch, "uint64", None)) if t is not None)
        for name, t in named:
            if not isinstance(t, torch.Tensor) or t.dtype not in ints or t.dim() != 1:
                raise ValueError(f"{name}: a 1-D torch tensor of 64-bit integers is needed")
            if t.numel() != named[0][1].numel():
                raise ValueError(f"{name}: {t.numel()} elements, {named[0][0]} has {named[0][1].numel()}")
        tensors = [t for _, t in named]
        flags = 0 if order_by is None else (0 if unsigned else SORT_I64) | (SORT_DESC if descending else 0)
        with self._on_torch_stream(tensors[0], tensors[0], tuple(tensors[1:])) as dev:
            n = tensors[0].numel()
            outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in opw]
            if n:
                cols = [v if o >= WIN_CUMSUM else None for o, v in zip(opw, values)]
                self.window_cols_dev(partition_by, order_by, n, flags, opw, offs, cols, outs)
                for j, o in enumerate(opw):
                    if o in (WIN_LAG_ROW, WIN_LEAD_ROW) and values[j] is not None:
                        got = torch.empty(n, dtype=values[j].dtype, device=dev)
                        self.gather_cols_fill([values[j]], n, outs[j], n, [fill], [got])
                        outs[j] = got
        return outs

    def topk_per_group_columns(self, partition_by, order_by, k, descending=False, unsigned=False):
        """idx: the rows with ROW_NUMBER() OVER (PARTITION BY partition_by ORDER BY order_by) <= k -- the first k rows of every partition
        in that order (descending=True: the k largest per group), ties in input order also at the cut -- as an int64 tensor SORTED
        ASCENDING.  One window_columns call and one torch.nonzero.  k: an int >= 0; the other arguments and errors as window_columns."""
        import torch
        if isinstance(k, bool) or not isinstance(k, int):
            raise ValueError(f"k: an int is needed, not {k!r}")
        if k < 0:
            raise ValueError(f"k: a count of rows is needed, not {k}")
        number = self.window_columns(partition_by, order_by, (), ("row_number",), descending, unsigned)[0]
        return torch.nonzero(number <= k).reshape(-1)

    def frame_cols_dev(self, d_part, d_order, n, flags=0, ops=(), preceding=None, following=None, d_cols=None, d_outs=()):
        """rhj_frame_cols_dev: per row a value over the ROWS frame [q - preceding[j], q + following[j]] around its position q in its
        partition (rows with the same d_part word; None: one partition), ordered by d_order under flags (SORT_I64, SORT_DESC; None:
        input order), ties in input order -- ops[j] one of FRAME_COUNT, FRAME_SUM, FRAME_MIN_U64 / FRAME_MAX_U64 / FRAME_MIN_I64 /
        FRAME_MAX_I64 (of d_cols[j]), FRAME_FIRST_ROW / FRAME_LAST_ROW (the row at the frame's first / last position).  preceding /
        following: one word per op, FRAME_UNBOUNDED: to the partition's edge; preceding None: unbounded for every op, following None:
        0 for every op.  d_outs[j]: uint64[n] in HBM, aligned with the rows.  The number of ops is len(ops), at most FRAME_MAX_OPS.
        Returns the number of partitions.  (A sequence that is None goes in as NULL: the library answers.)"""
        k = len(ops) if ops is not None else 0
        opw = (C.c_uint32 * max(k, 1))(*[int(o) for o in ops]) if ops is not None else None
        pre = (_u64 * max(k, 1))(*[int(a) for a in preceding]) if preceding is not None else None
        fol = (_u64 * max(k, 1))(*[int(a) for a in following]) if following is not None else None
        cols = (_vp * max(k, 1))(*[_addr(c) for c in d_cols]) if d_cols is not None else None
        outs = (_vp * max(k, 1))(*[_addr(o) for o in d_outs]) if d_outs is not None else None
        parts = _u64()
        self._chk(self.lib.rhj_frame_cols_dev(self.ctx, _addr(d_part), _addr(d_order), n, flags, opw, pre, fol, cols, k, outs, C.byref(parts)))
        return parts.value

    def frame_columns(self, part, order, cols, ops, preceding=None, following=0, descending=False, unsigned=False):
        """[out_0, out_1, ..]: framed window aggregates over the rows of a table -- one int64 tensor per op, ALIGNED WITH THE ROWS.
        Partitions, order and ties as window_columns: rows with equal part form a partition (None: one partition; a list of 1 to
        KEYS_MAX_COLS tensors is packed first), ordered inside it by order as int64 (unsigned=True: as uint64), ascending
        (descending=True: descending), equal order keys in input order; order None: input order.  For the row at 0-based position q of
        a partition of m rows the frame of op j is the positions [max(0, q - preceding[j]), min(m - 1, q + following[j])] -- ROWS
        BETWEEN preceding PRECEDING AND following FOLLOWING.  preceding / following: an int >= 0, None (unbounded: to the partition's
        edge), or a list with one of those per op.  The defaults are the running frame of window_columns.  ops:
          "count"  the rows in the frame; with both sides None the partition's size (groupby.transform("size"))
          "sum"    the sum mod 2^64 of cols[j] over the frame (groupby.rolling(w).sum() is preceding=w - 1)
          "min" / "max"  the minimum / maximum of cols[j] over the frame as int64 (unsigned=True: of the words as uint64); its cost does
                   not depend on the frame's width
          "first_row" / "last_row"  the index of the row at the frame's first / last position; x[out] is FIRST_VALUE / LAST_VALUE(x)
        cols[j] is None for an op without a column (cols=() or None: every op without one).  At most FRAME_MAX_OPS ops per call.
        An unknown op, too many ops, a length mismatch, a negative, bool or float bound, a non-bool flag, descending=True without
        order: ValueError before any device use.  One rhj_frame_cols_dev call.  Streams and completion as join_columns."""
        import torch
        opw, cols, pre, fol = _frame_args(order, cols, ops, preceding, following, descending, unsigned)
        if isinstance(part, (list, tuple)):
            packed, _, plan = self.pack_keys(part, keep_dictionaries=False)
            plan.close()
            part = packed
        named = [("part", part), ("order", order)] + [(f"cols[{j}]", v) for j, v in enumerate(cols)]
        named = [(name, t) for name, t in named if t is not None]
        if not named:
            raise ValueError("part, order and cols are all None: the number of rows is unknown")
        ints = tuple(t for t in (torch.int64, getattr(torch, "uint64", None)) if t is not None)
        for name, t in named:
            if not isinstance(t, torch.Tensor) or t.dtype not in ints or t.dim() != 1:
                raise ValueError(f"{name}: a 1-D torch tensor of 64-bit integers is needed")
            if t.numel() != named[0][1].numel():
                raise ValueError(f"{name}: {t.numel()} elements, {named[0][0]} has {named[0][1].numel()}")
        tensors = [t for _, t in named]
        flags = 0 if order is None else (0 if unsigned else SORT_I64) | (SORT_DESC if descending else 0)
        with self._on_torch_stream(tensors[0], tensors[0], tuple(tensors[1:])) as dev:
            n = tensors[0].numel()
            outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in opw]
            if n:
                self.frame_cols_dev(part, order, n, flags, opw, pre, fol, cols, outs)
        return outs

    def frame_range_cols_dev(self, d_part, d_order, n, flags=0, ops=(), preceding=None, following=None, d_cols=None, d_outs=()):
        """rhj_frame_range_cols_dev: frame_cols_dev with a RANGE frame -- per row a value over the rows of its partition whose d_order
        value lies in [t - preceding[j], t + following[j]] around its own value t (under SORT_DESC [t - following[j], t +
        preceding[j]]), saturating at the view's ends; the current row's peers are always inside.  d_order is needed.  preceding /
        following: one distance per op, FRAME_UNBOUNDED: to the partition's edge; preceding None: unbounded for every op, following
        None: 0 for every op -- SQL's default frame.  Everything else as frame_cols_dev.  Returns the number of partitions."""
        k = len(ops) if ops is not None else 0
        opw = (C.c_uint32 * max(k, 1))(*[int(o) for o in ops]) if ops is not None else None
        pre = (_u64 * max(k, 1))(*[int(a) for a in preceding]) if preceding is not None else None
        fol = (_u64 * max(k, 1))(*[int(a) for a in following]) if following is not None else None
        cols = (_vp * max(k, 1))(*[_addr(c) for c in d_cols]) if d_cols is not None else None
        outs = (_vp * max(k, 1))(*[_addr(o) for o in d_outs]) if d_outs is not None else None
        parts = _u64()
        self._chk(self.lib.rhj_frame_range_cols_dev(self.ctx, _addr(d_part), _addr(d_order), n, flags, opw, pre, fol, cols, k, outs, C.byref(parts)))
        return parts.value

    def frame_range_columns(self, part, order, cols, ops, preceding=None, following=0, descending=False, unsigned=False):
        """[out_0, out_1, ..]: window aggregates over RANGE frames -- one int64 tensor per op, ALIGNED WITH THE ROWS.  As frame_columns,
        but the frame is a VALUE distance on `order`, which is needed: for a row with order value t the frame of op j is every row of
        its partition whose order value lies in [t - preceding[j], t + following[j]] (descending=True: [t - following[j], t +
        preceding[j]]; preceding still means earlier in the order) -- RANGE BETWEEN preceding PRECEDING AND following FOLLOWING.  The
        values are compared as int64 (unsigned=True: as uint64), distances are exact and saturate at the type's ends.  preceding /
        following: an int >= 0, None (unbounded: to the partition's edge), or a list with one of those per op.  The defaults are SQL's
        default frame, RANGE UNBOUNDED PRECEDING to CURRENT ROW: the running aggregate in which peers share a value.  The frame always
        holds the current row and ALL its peers, also at distance 0; pandas' time-based rolling stops at the current row among peers,
        so groupby.rolling("5s").sum() is preceding=4_999_999_999 (closed="both": 5_000_000_000) exactly when the order keys are
        distinct within a partition.  part: a tensor, None (one partition), or a list of 1 to KEYS_MAX_COLS tensors, packed first.
        ops and cols as frame_columns; the cost of "min" / "max" depends on the frame here.  An unknown op, too many ops, a length
        mismatch, a negative, bool or float bound, a non-bool flag, order None or a list: ValueError before any device use.  One
        rhj_frame_range_cols_dev call.  Streams and completion as join_columns."""
        import torch
        if order is None or isinstance(order, (list, tuple)):
            raise ValueError("order: one tensor is needed -- a value distance needs a value")
        opw, cols, pre, fol = _frame_args(order, cols, ops, preceding, following, descending, unsigned)
        if isinstance(part, (list, tuple)):
            packed, _, plan = self.pack_keys(part, keep_dictionaries=False)
            plan.close()
            part = packed
        named = [("order", order), ("part", part)] + [(f"cols[{j}]", v) for j, v in enumerate(cols)]
        named = [(name, t) for name, t in named if t is not None]
        ints = tuple(t for t in (torch.int64, getattr(torch, "uint64", None)) if t is not None)
        for name, t in named:
            if not isinstance(t, torch.Tensor) or t.dtype not in ints or t.dim() != 1:
                raise ValueError(f"{name}: a 1-D torch tensor of 64-bit integers is needed")
            if t.numel() != order.numel():
                raise ValueError(f"{name}: {t.numel()} elements, order has {order.numel()}")
        tensors = [t for _, t in named]
        flags = (0 if unsigned else SORT_I64) | (SORT_DESC if descending else 0)
        with self._on_torch_stream(tensors[0], tensors[0], tuple(tensors[1:])) as dev:
            n = order.numel()
            outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in opw]
            if n:
                self.frame_range_cols_dev(part, order, n, flags, opw, pre, fol, cols, outs)
        return outs

    def ntile_columns(self, part, order, buckets, descending=False, unsigned=False):
        """tile: NTILE(buckets) OVER (PARTITION BY part ORDER BY order) as an int64 tensor aligned with the rows -- the rows of a
        partition of m rows, in order, dealt into buckets 1 .. buckets whose sizes differ by at most one, the m % buckets larger ones
        first (SQL's rule; with m < buckets the rows get 1 .. m).  ROW_NUMBER from window_columns, the partition's size from
        frame_columns(.., ["count"], None, None), the rule in torch: TWO calls, so two sets of sorts.  buckets: an int >= 1; the
        other arguments and errors as window_columns."""
        import torch
        if isinstance(buckets, bool) or not isinstance(buckets, int) or buckets < 1:
            raise ValueError(f"buckets: an int >= 1 is needed, not {buckets!r}")
        number = self.window_columns(part, order, (), ("row_number",), descending, unsigned)[0]
        size = self.frame_columns(part, order, (), ["count"], None, None, descending, unsigned)[0]
        small = torch.div(size, buckets, rounding_mode="floor")
        big = size - small * buckets                      # that many buckets hold small + 1 rows, and they come first
        cut = big * (small + 1)
        q = number - 1
        return torch.where(q < cut, torch.div(q, small + 1, rounding_mode="floor"),
                           big + torch.div(q - cut, torch.clamp(small, min=1), rounding_mode="floor")) + 1

    def asof_cols_dev(self, d_byR, d_onR, nR, d_byS, d_onS, nS, flags=0, tolerance=0, d_out_rowS=None):
        """rhj_asof_cols_dev: d_out_rowS[i] = the row of S nearest to row i of R among the rows with a bit-equal `by` word (d_byR and
        d_byS None: one partition) whose `on` word is at or before onR[i] -- flags: ASOF_I64 (the words as int64), ASOF_FORWARD (at or
        after), ASOF_STRICT (equal words excluded), ASOF_TOLERANCE (only within tolerance; ignored without the bit) --, NO_ROW where
        there is none; among equal `on` words backward takes the largest row of S, forward the smallest.  d_out_rowS: uint64[nR] in
        HBM, aligned with R.  Returns the number of rows of R with a partner."""
        matched = _u64()
        self._chk(self.lib.rhj_asof_cols_dev(self.ctx, _addr(d_byR), _addr(d_onR), nR, _addr(d_byS), _addr(d_onS), nS, flags, tolerance,
                                             _addr(d_out_rowS), C.byref(matched)))
        return matched.value

    def asof_join_columns(self, on_R, on_S, by_R=None, by_S=None, values_S=(), direction="backward", allow_exact_matches=True, tolerance=None,
                          unsigned=False, fill=0):
        """(idx_S, matched, values): the as-of join, pandas.merge_asof(R, S, on=.., by=..) as indices -- idx_S[i] = the row of S whose
        on_S is the nearest at or before on_R[i] (direction="forward": at or after) among the rows of S with by_S equal to by_R[i],
        -1 where there is none; an int64 tensor of len(on_R) on the tensors' device, aligned with R.  matched = how many rows of R found
        a partner, a Python int; values = one int64 tensor of len(on_R) per tensor of values_S: values[k][i] = values_S[k][idx_S[i]], or
        fill where idx_S[i] == -1 (shaped as lookup_columns returns them).  on_R / on_S: contiguous 1-D 64-bit integer tensors on the
        engine's device, ordered as int64 (unsigned=True: the words as uint64); NEITHER needs to be sorted.  by_R / by_S: None (one
        partition), a tensor per side, or a list of 1 to KEYS_MAX_COLS tensors per side (packed first, pack_keys).
        allow_exact_matches=False excludes equal on values; tolerance: None, or an int >= 0 -- only partners with |on_R[i] - on_S[j]|
        <= tolerance, as exact integers.  Where S repeats a (by, on), backward returns the LAST of the duplicates and forward the
        FIRST, as pandas does.  values_S: up to LOOKUP_MAX_COLS tensors of len(on_S); fill: an int, or one per tensor.
        direction="nearest" is not supported (a backward call, a forward call and a comparison of the two distances give it).  A wrong
        direction, a non-bool flag, a negative, bool or float tolerance, `by` on one side only, a different number of `by` tensors per
        side, more than KEYS_MAX_COLS of them, too many value tensors: ValueError before any device use.  One rhj_asof_cols_dev call
        and one rhj_gather_cols_fill.  Streams and completion as join_columns."""
        import torch
        flags, tol, values_S, fills = _asof_args(by_R, by_S, values_S, direction, allow_exact_matches, tolerance, unsigned, fill)
        if isinstance(by_R, (list, tuple)) or isinstance(by_S, (list, tuple)):
            by_R, by_S, plan = self.pack_keys(by_R if isinstance(by_R, (list, tuple)) else [by_R],
                                              by_S if isinstance(by_S, (list, tuple)) else [by_S], keep_dictionaries=False)
            plan.close()                           # (a join needs no dictionary: the plan holds nothing)
        with self._on_torch_stream(on_R, on_S, () if by_R is None else (by_R,), weights_S=values_S + (() if by_S is None else (by_S,))) as dev:
            nR, nS = on_R.numel(), on_S.numel()
            idx_S = torch.empty(nR, dtype=torch.int64, device=dev)
            matched = self.asof_cols_dev(by_R, on_R, nR, by_S, on_S, nS, flags, tol, idx_S if nR else None)
            values = [torch.empty(nR, dtype=torch.int64, device=dev) for _ in values_S]
            if values and nR:
                self.gather_cols_fill(values_S, nS, idx_S, nR, fills, values)
        return idx_S, matched, values

    def range_join_cols_dev(self, d_byR, d_loR, d_hiR, nR, d_byS, d_onS, nS, flags=0, below=0, above=0, d_out_offsets=None, d_out_first=None,
                            d_out_rowsS=None, d_out=None, out_capacity=0, allow_overflow=False):
        """rhj_range_join_cols_dev: the rows of S with a bit-equal `by` word (d_byR and d_byS None: one partition) whose `on` word lies
        in [lo[i], hi[i]] -- flags: RANGE_I64 (the words as int64), RANGE_LO_OPEN / RANGE_HI_OPEN (that end excluded), RANGE_BAND (d_loR
        holds x, d_hiR is None, the interval is [x - below, x + above], saturating) -- as d_out_rowsS (uint64[nS]: the rows of S ordered
        by (by, on, row)), d_out_first (uint64[nR]) and d_out_offsets (uint64[nR + 1]): the partners of row i are rowsS[first[i] ..
        first[i] + offsets[i + 1] - offsets[i]); and as d_out, out_capacity pairs {rowR, rowS} ordered by rowR, then as rowsS.  Each
        output may be None.  Returns the exact number of pairs; with allow_overflow a capacity below it is not an error (the first
        out_capacity pairs are written, the CSR outputs are complete)."""
        count = _u64()
        rc = self.lib.rhj_range_join_cols_dev(self.ctx, _addr(d_byR), _addr(d_loR), _addr(d_hiR), nR, _addr(d_byS), _addr(d_onS), nS, flags, below,
                                              above, _addr(d_out_offsets), _addr(d_out_first), _addr(d_out_rowsS), _addr(d_out), out_capacity,
                                              C.byref(count))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return count.value

    def range_expand_dev(self, d_offsets, d_first, nR, d_rowsS, nS, d_out=None, out_capacity=0, allow_overflow=False):
        """rhj_range_expand_dev: the pairs of a CSR result (range_join_cols_dev's three arrays, validated on the device first: RhjError
        for arrays that are none) into d_out, out_capacity pairs.  Returns the exact number of pairs; allow_overflow as there."""
        count = _u64()
        rc = self.lib.rhj_range_expand_dev(self.ctx, _addr(d_offsets), _addr(d_first), nR, _addr(d_rowsS), nS, _addr(d_out), out_capacity,
                                           C.byref(count))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return count.value

    def _range_csr(self, lo_R, hi_R, on_S, by_R, by_S, flags, below=0, above=0):
        """one rhj_range_join_cols_dev call without pairs: (offsets, first, rows_S, total, device)"""
        import torch
        if isinstance(by_R, (list, tuple)) or isinstance(by_S, (list, tuple)):
            by_R, by_S, plan = self.pack_keys(by_R if isinstance(by_R, (list, tuple)) else [by_R],
                                              by_S if isinstance(by_S, (list, tuple)) else [by_S], keep_dictionaries=False)
            plan.close()                           # (a join needs no dictionary: the plan holds nothing)
        with self._on_torch_stream(lo_R, on_S, tuple(t for t in (hi_R, by_R) if t is not None), weights_S=() if by_S is None else (by_S,)) as dev:
            nR, nS = lo_R.numel(), on_S.numel()
            offsets = torch.zeros(nR + 1, dtype=torch.int64, device=dev)
            first = torch.zeros(nR, dtype=torch.int64, device=dev)
            rows_S = torch.empty(nS, dtype=torch.int64, device=dev)
            total = 0
            if nR and nS:
                total = self.range_join_cols_dev(by_R, lo_R, hi_R, nR, by_S, on_S, nS, flags, below, above, offsets, first, rows_S)
            elif nS:
                rows_S = torch.empty(0, dtype=torch.int64, device=dev)     # no row of R: S is not sorted, nothing refers to it
        return offsets, first, rows_S, total, dev

    def _range_pairs(self, csr):
        """(idx_R, idx_S) of a CSR result: one rhj_range_expand_dev and one rhj_pairs_split -- no second set of sorts"""
        import torch
        offsets, first, rows_S, total, dev = csr
        idx_R = torch.empty(total, dtype=torch.int64, device=dev)
        idx_S = torch.empty(total, dtype=torch.int64, device=dev)
        if total:
            with self._on_torch_stream(offsets, rows_S, weights_S=()):
                pairs = torch.empty((total, 2), dtype=torch.int64, device=dev)
                got = self.range_expand_dev(offsets, first, first.numel(), rows_S, rows_S.numel(), pairs, total)
                assert got == total, (got, total)
                self.pairs_split(pairs, total, idx_R, idx_S)
        return idx_R, idx_S

    def range_join_csr_columns(self, lo_R, hi_R, on_S, by_R=None, by_S=None, closed="both", unsigned=False):
        """(offsets, first, rows_S, total): the range join SELECT .. FROM R JOIN S ON r.by = s.by AND s.on BETWEEN r.lo AND r.hi in its
        compact form -- rows_S the indices of S ordered by (by, on, index), and for row i of R its partners rows_S[first[i] : first[i] +
        offsets[i + 1] - offsets[i]]; offsets the exclusive prefix of the counts (len(lo_R) + 1 words, offsets[-1] == total); total a
        Python int.  int64 tensors on the tensors' device: 16 bytes per row of R and 8 per row of S however many pairs there are.
        lo_R / hi_R / on_S: contiguous 1-D 64-bit integer tensors on the engine's device, ordered as int64 (unsigned=True: the words as
        uint64); NEITHER table needs to be sorted.  closed: "both" (lo <= on <= hi), "left" (on < hi), "right" (lo < on) or "neither".
        An interval with lo > hi has no partner.  by_R / by_S: None (one partition), a tensor per side, or a list of 1 to KEYS_MAX_COLS
        tensors per side (packed first, pack_keys; rows_S is then ordered by the packed word first -- the runs hold the same rows in
        the same order for any packing).  With no row of R rows_S is empty.  A wrong closed, a non-bool unsigned, `by` on
        one side only, a different number of `by` tensors per side, hi_R of another length than lo_R: ValueError before any device
        use.  One rhj_range_join_cols_dev call.  Streams and completion as join_columns."""
        flags = _range_args(by_R, by_S, closed, unsigned, lo_R=lo_R, hi_R=hi_R)
        return self._range_csr(lo_R, hi_R, on_S, by_R, by_S, flags)[:4]

    def range_join_columns(self, lo_R, hi_R, on_S, by_R=None, by_S=None, closed="both", unsigned=False):
        """(idx_R, idx_S): the range join as index pairs -- every (i, j) with by_R[i] == by_S[j] and lo_R[i] <= on_S[j] <= hi_R[i]
        exactly once, ordered by i and within one i by (on_S[j], j): a defined order, bit-identical from run to run.  Arguments and
        errors as range_join_csr_columns.  One csr call, then total pairs are allocated and filled by one rhj_range_expand_dev and one
        rhj_pairs_split: the sorts run once."""
        flags = _range_args(by_R, by_S, closed, unsigned, lo_R=lo_R, hi_R=hi_R)
        return self._range_pairs(self._range_csr(lo_R, hi_R, on_S, by_R, by_S, flags))

    def band_join_columns(self, on_R, on_S, below, above, by_R=None, by_S=None, closed="both", unsigned=False):
        """(idx_R, idx_S): the band join on_R[i] - below <= on_S[j] <= on_R[i] + above (and by_R[i] == by_S[j]) as index pairs, ordered
        as range_join_columns' -- "every quote within 5 s around each trade".  below / above: ints >= 0, exact distances: both ends
        saturate at the view's minimum and maximum, nothing wraps, and 2^64 - 1 is "to the end of the view".  closed applies to the
        saturated ends.  A negative, bool or float below / above: ValueError before any device use; the other arguments and errors as
        range_join_csr_columns.  RANGE_BAND: no bound tensor is materialised."""
        flags = _range_args(by_R, by_S, closed, unsigned, below, above) | RANGE_BAND
        return self._range_pairs(self._range_csr(on_R, None, on_S, by_R, by_S, flags, below, above))

    def factorize_columns(self, keys):
        """(codes, uniques): pandas.factorize without the ordering promise -- uniques the distinct values of keys in no particular
        order, codes an int64 tensor of len(keys) with uniques[codes] == keys (dictionary encoding of a 64-bit key column into dense
        ids).  Tensors, streams and completion as group_by_columns_with_inverse, which this is without the counts.
        Composite keys: a list or tuple of key tensors gives uniques as a list of tensors, uniques[j][codes] == keys[j] for every j."""
        uniques, _, _, codes = self._group_by_columns(keys, (), None, True)
        return codes, uniques

    def join_group_by_columns(self, keys_R, keys_S, weights_R=(), weights_S=(), how="inner", ops_R=None, ops_S=None):
        """(keys, count, sums_R, sums_S): SELECT key, COUNT(*), SUM(r.a).., SUM(s.b).. FROM R JOIN S USING (key) GROUP BY key -- per
        join value the number of index pairs (i, j) with keys_R[i] == keys_S[j] == key, and per tensor of weights_R / weights_S the
        sum of weights_R[k][i] / weights_S[k][j] over those pairs, mod 2^64 -- without the pairs: int64 tensors of one length on the
        keys' device, sums_R / sums_S lists of len(weights_R) / len(weights_S) of them, group g of all at index g, groups in no
        particular order.  how="inner": the values both tensors have.  how="left" (LEFT JOIN): every distinct value of keys_R; a
        value keys_S lacks is one row per occurrence in keys_R with NULLs for S, so its count is its number of occurrences, its
        sums_R their plain sums and its sums_S 0.  The products are formed from the raw per-side results of rhj_group_join_cols_dev
        with wrapping int64 multiplies (count = cntR * cntS, sums_R = sumsR * cntS, sums_S = sumsS * cntR; under how="left"
        max(cntS, 1) multiplies R's side).  keys_R / keys_S: contiguous 1-D 64-bit integer tensors on the engine's device; weights_R
        / weights_S: up to GROUP_JOIN_MAX_COLS tensors each, of the same kind, as long as keys_R / keys_S.  Negative keys and weights
        are bit patterns: a key comes back as it went in, an int64 sum is the two's complement sum.  The outputs are allocated at
        len(keys_R), the upper bound, and returned as views [:groups] or products of them.  Streams and completion as join_columns.
        ops_R / ops_S: None -- every tensor of that side is summed --, or one of "sum" | "min" | "max" per tensor of weights_R /
        weights_S (SELECT key, MIN(r.a), MAX(s.b) ..): a "min" / "max" entry of sums_R / sums_S is the minimum / maximum of the int64
        values over the group's pairs, which is the one over that side's rows: it is returned RAW, with no multiplication by the
        other side's count.  Under how="left" S's "min" / "max" of a value keys_S lacks is the op's identity (min: INT64_MAX, max:
        INT64_MIN; SQL's NULL), its "sum" 0.  With both None the call is rhj_group_join_cols_dev, otherwise
        rhj_group_join_agg_cols_dev.  A wrong length or name: ValueError before any launch.  Costs as for sums, whatever the ops.
        The group of every row of either side beside them: join_group_by_columns_with_inverse.
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); keys is then a list of as many tensors."""
        return self._join_group_by_columns(keys_R, keys_S, weights_R, weights_S, how, ops_R, ops_S, False)

    def join_group_by_columns_with_inverse(self, keys_R, keys_S, weights_R=(), weights_S=(), how="inner", ops_R=None, ops_S=None):
        """(keys, count, sums_R, sums_S, (inverse_R, inverse_S)): join_group_by_columns with the group of every row -- int64 tensors
        of len(keys_R) / len(keys_S) with keys[inverse_R[i]] == keys_R[i] and keys[inverse_S[j]] == keys_S[j] where the row's value
        has a group, and -1 (SQL's NULL) where it has none: under how="inner" the rows whose value the other tensor lacks, under
        how="left" only such rows of keys_S.  A joint dictionary encoding of two key tensors: shared dense ids, "no partner" marked.
        Ids go with this call's keys.  Everything else as join_group_by_columns (rhj_group_join_agg_ids_cols_dev: both id tensors are
        filled, then one more sweep per side and class and one scattered 8-byte store per row that has a group).
        Composite keys: a list of 1 to KEYS_MAX_COLS key tensors per side is packed first (pack_keys); keys is then a list of as many tensors."""
        return self._join_group_by_columns(keys_R, keys_S, weights_R, weights_S, how, ops_R, ops_S, True)

    def _join_group_by_columns(self, keys_R, keys_S, weights_R, weights_S, how, ops_R, ops_S, return_inverse):
        import torch
        packed = self._packed_pair(keys_R, keys_S, keep_dictionaries=True)
        if packed is not None:
            out = self._join_group_by_columns(packed[0], packed[1], weights_R, weights_S, how, ops_R, ops_S, return_inverse)
            keys = packed[2].unpack(out[0])
            packed[2].close()
            return (keys,) + out[1:]
        weights_R, weights_S = tuple(weights_R), tuple(weights_S)
        if how not in ("inner", "left"):
            raise ValueError(f"how: 'inner' or 'left', not {how!r}")
        for name, w in (("weights_R", weights_R), ("weights_S", weights_S)):
            if len(w) > GROUP_JOIN_MAX_COLS:
                raise ValueError(f"at most {GROUP_JOIN_MAX_COLS} {name} tensors per call, not {len(w)}")
        with_ops = ops_R is not None or ops_S is not None
        ops_R = [AGG_SUM] * len(weights_R) if ops_R is None else _agg_ops(ops_R, len(weights_R), "ops_R")
        ops_S = [AGG_SUM] * len(weights_S) if ops_S is None else _agg_ops(ops_S, len(weights_S), "ops_S")
        with self._on_torch_stream(keys_R, keys_S, weights_R, weights_S=weights_S) as dev:
            nR, nS = keys_R.numel(), keys_S.numel()
            new = lambda: torch.empty(nR, dtype=torch.int64, device=dev)
            out_keys, cntR, cntS = new(), new(), new()
            sumsR = [new() for _ in weights_R]
            # (tensors without elements have no address to hand over: an empty S goes in without columns, its sums are 0)
            # ... or, for a minimum / maximum, the op's identity)
            sumsS = [new() if nS else torch.full((nR,), _AGG_IDENTITY_I64[o], dtype=torch.int64, device=dev) for o in ops_S]
            mode = GJ_LEFT if how == "left" else GJ_INNER
            if return_inverse:
                inv_R = new()
                inv_S = torch.full((nS,), -1, dtype=torch.int64, device=dev)     # (an empty tensor has no address: it stays out of the call)
            if not nR:
                groups = 0
            elif return_inverse:
                groups = self.group_join_agg_ids_cols_dev(keys_R, None, nR, keys_S if nS else None, None, nS, weights_R, ops_R, nR,
                                                          weights_S if nS else (), ops_S if nS else None, nS, mode, out_keys, cntR, cntS,
                                                          sumsR, sumsS if nS else (), nR, inv_R, nR, inv_S if nS else None, nS)
            elif not with_ops:
                groups = self.group_join_cols_dev(keys_R, None, nR, keys_S if nS else None, None, nS, weights_R, nR,
                                                  weights_S if nS else (), nS, mode, out_keys, cntR, cntS, sumsR, sumsS if nS else (), nR)
            else:
                groups = self.group_join_agg_cols_dev(keys_R, None, nR, keys_S if nS else None, None, nS, weights_R, ops_R, nR,
                                                      weights_S if nS else (), ops_S if nS else None, nS, mode, out_keys, cntR, cntS,
                                                      sumsR, sumsS if nS else (), nR)
        cntR, cntS = cntR[:groups], cntS[:groups]
        mult_R = cntS.clamp(min=1) if how == "left" else cntS    # (counts are < 2^63: clamp on int64 is on the true values)
        out = (out_keys[:groups], cntR * mult_R, [s[:groups] * mult_R if o == AGG_SUM else s[:groups] for s, o in zip(sumsR, ops_R)],
               [s[:groups] * cntR if o == AGG_SUM else s[:groups] for s, o in zip(sumsS, ops_S)])
        return out + ((inv_R, inv_S),) if return_inverse else out

    def mul_u64(self, d_a, d_b, n, d_dst):
        """rhj_mul_u64: d_dst[i] = d_a[i] * d_b[i] mod 2^64 (d_dst may be d_a)"""
        self._chk(self.lib.rhj_mul_u64(self.ctx, _addr(d_a), _addr(d_b), n, _addr(d_dst)))

    def sum_gather_weighted(self, d_col, d_rows, d_w, n):
        """rhj_sum_gather_weighted: the sum of d_col[d_rows[i] or i] * d_w[i] mod 2^64 (d_col None: the sum of d_w)"""
        s = _u64()
        self._chk(self.lib.rhj_sum_gather_weighted(self.ctx, _addr(d_col), _addr(d_rows), _addr(d_w), n, C.byref(s)))
        return s.value

    def histogram(self, d_rel, n, shift, bits, d_hist):
        self._chk(self.lib.rhj_histogram(self.ctx, _addr(d_rel), n, shift, bits, _addr(d_hist)))

    def prefix(self, d_hist, nbins, d_start):
        self._chk(self.lib.rhj_prefix(self.ctx, _addr(d_hist), nbins, _addr(d_start)))

    def partition(self, d_in, n, bits1, bits2, d_out, d_part_start):
        self._chk(self.lib.rhj_partition(self.ctx, _addr(d_in), n, bits1, bits2, _addr(d_out), _addr(d_part_start)))

    def partition_at(self, d_in, n, shift, bits, d_out, d_part_start):
        self._chk(self.lib.rhj_partition_at(self.ctx, _addr(d_in), n, shift, bits, _addr(d_out), _addr(d_part_start)))

    def owner_histogram(self, d_rel, n, shift, bits, d_hist):
        """rhj_histogram on bits of mix64(payload): the multi-GPU owner classes"""
        self._chk(self.lib.rhj_owner_histogram(self.ctx, _addr(d_rel), n, shift, bits, _addr(d_hist)))

    def owner_split(self, d_in, n, shift, bits, d_out, d_class_start):
        """rhj_partition_at on bits of mix64(payload), tuples unchanged"""
        self._chk(self.lib.rhj_owner_split(self.ctx, _addr(d_in), n, shift, bits, _addr(d_out), _addr(d_class_start)))

    def bucket_join(self, d_Rp, d_startR, d_Sp, d_startS, nparts, radix_bits, d_out=None, capacity=0,
                    probe_split=0, allow_overflow=False):
        n = _u64()
        rc = self.lib.rhj_bucket_join(self.ctx, _addr(d_Rp), _addr(d_startR), _addr(d_Sp), _addr(d_startS), nparts,
                                      radix_bits, probe_split, _addr(d_out), capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    # ---- multi-GPU stage entry points (include/rhj.h) --------------------------------------
    def shard_stats(self, side, d_rel, n, shift, bits):
        """class histogram (numpy int64 [2^bits]) and rowID range (min, max) of a shard; synchronises"""
        hist = np.zeros(1 << bits, dtype=np.uint64)
        kmin, kmax = _u64(), _u64()
        self._chk(self.lib.rhj_shard_stats(self.ctx, side, _addr(d_rel), n, shift, bits, hist.ctypes.data, C.byref(kmin), C.byref(kmax)))
        return hist.astype(np.int64), kmin.value, kmax.value

    def shard_split(self, side, d_rel, n, shift, bits, key_base, d_narrow_out, d_class_start=None):
        self._chk(self.lib.rhj_shard_split(self.ctx, side, _addr(d_rel), n, shift, bits, key_base, _addr(d_narrow_out),
                                           _addr(d_class_start)))

    def shard_split_peer(self, side, d_rel, n, shift, bits, key_base, owner, dst_class_start, peer_payloads, peer_rowids):
        """rhj_shard_split_peer: owner (uint8[2^bits]) and dst_class_start (uint64[2^bits]) numpy arrays, peer_* lists of device
        pointers / buffers, one per rank"""
        owner = np.ascontiguousarray(owner, dtype=np.uint8)
        dst = np.ascontiguousarray(dst_class_start, dtype=np.uint64)
        nr = len(peer_payloads)
        pp = (_vp * nr)(*[_addr(x) for x in peer_payloads])
        pk = (_vp * nr)(*[_addr(x) for x in peer_rowids])
        self._chk(self.lib.rhj_shard_split_peer(self.ctx, side, _addr(d_rel), n, shift, bits, key_base, owner.ctypes.data, dst.ctypes.data,
                                                pp, pk, nr))

    def shard_partition(self, side, d_payloads, d_rowids, m, seg_off, row0, plan, mode):
        assert len(row0) == len(seg_off) - 1
        seg = (C.c_uint64 * len(seg_off))(*[int(x) for x in seg_off])
        base = (C.c_uint64 * len(row0))(*[int(x) for x in row0])
        self._chk(self.lib.rhj_shard_partition(self.ctx, side, _addr(d_payloads), _addr(d_rowids), m, len(seg_off) - 1, seg, base,
                                               C.byref(plan), mode))

    def shard_join(self, d_out=None, capacity=0, allow_overflow=False):
        n = _u64()
        rc = self.lib.rhj_shard_join(self.ctx, _addr(d_out), capacity, C.byref(n))
        self._chk(rc, allow=(RHJ_E_OVERFLOW,) if allow_overflow else ())
        return n.value

    # ---- query-layer kernels -------------------------------------------------------------
    def col_filter(self, d_col, d_rows_in, n_in, op, value, d_rows_out):
        n = _u64()
        self._chk(self.lib.rhj_col_filter(self.ctx, _addr(d_col), _addr(d_rows_in), n_in, ord(op), value, _addr(d_rows_out), C.byref(n)))
        return n.value

    def gather_tuples(self, d_col, d_rows, n, key_is_position, d_tuples):
        self._chk(self.lib.rhj_gather_tuples(self.ctx, _addr(d_col), _addr(d_rows), n, 1 if key_is_position else 0, _addr(d_tuples)))

    def pairs_split(self, d_pairs, n, d_r, d_s):
        self._chk(self.lib.rhj_pairs_split(self.ctx, _addr(d_pairs), n, _addr(d_r), _addr(d_s)))

    def gather_u64(self, d_src, d_idx, n, d_dst):
        self._chk(self.lib.rhj_gather_u64(self.ctx, _addr(d_src), _addr(d_idx), n, _addr(d_dst)))

    def gather_cols_fill(self, d_srcs, src_rows, d_idx, n, fills, d_dsts):
        """rhj_gather_cols_fill: d_dsts[j][i] = fills[j] where d_idx[i] == NO_ROW, d_srcs[j][d_idx[i]] otherwise -- 1 to
        LOOKUP_MAX_COLS device columns of src_rows uint64 gathered by one index column of n uint64 into as many device columns of n
        uint64; fills: one int per column, taken mod 2^64.  Any other index >= src_rows: RhjError, nothing is read there.  (A
        sequence that is None goes in as NULL: the library answers.)"""
        k = len(d_srcs) if d_srcs is not None else len(d_dsts) if d_dsts is not None else len(fills or ())
        srcs = (_vp * max(k, 1))(*[_addr(c) for c in d_srcs]) if d_srcs is not None else None
        dsts = (_vp * max(k, 1))(*[_addr(c) for c in d_dsts]) if d_dsts is not None else None
        vals = (_u64 * max(k, 1))(*[int(f) & NO_ROW for f in fills]) if fills is not None else None
        self._chk(self.lib.rhj_gather_cols_fill(self.ctx, srcs, k, src_rows, _addr(d_idx), n, vals, dsts))

    def rows_filter_equal(self, d_colA, d_rowsA, d_colB, d_rowsB, n, d_pos_out):
        m = _u64()
        self._chk(self.lib.rhj_rows_filter_equal(self.ctx, _addr(d_colA), _addr(d_rowsA), _addr(d_colB), _addr(d_rowsB), n,
                                                 _addr(d_pos_out), C.byref(m)))
        return m.value

    def sum_gather(self, d_col, d_rows, n):
        s = _u64()
        self._chk(self.lib.rhj_sum_gather(self.ctx, _addr(d_col), _addr(d_rows), n, C.byref(s)))
        return s.value

    def pairs_checksum(self, d_pairs, n):
        c = _u64()
        self._chk(self.lib.rhj_pairs_checksum_dev(self.ctx, _addr(d_pairs), n, C.byref(c)))
        return c.value

    def generate(self, kind, d_out, n, row0=0, D=1, seed=0, theta_milli=0):
        self._chk(self.lib.rhj_generate_dev(self.ctx, kind, _addr(d_out), n, row0, D, seed, theta_milli))

    def remap_keys(self, d_rel, n, shift, add=0):
        """payload = (k << shift) + add for generated payloads mix(k), in place (same PK/FK pair set, aligned / dense join values)"""
        self._chk(self.lib.rhj_remap_keys_dev(self.ctx, _addr(d_rel), n, shift, add))

    def expected_pkfk(self, d_S, n):
        cnt, c = _u64(), _u64()
        self._chk(self.lib.rhj_expected_pkfk_dev(self.ctx, _addr(d_S), n, C.byref(cnt), C.byref(c)))
        return cnt.value, c.value


GEN_R, GEN_S_UNIFORM, GEN_S_ZIPF, GEN_S_DISJOINT, GEN_CONST = 0, 1, 2, 3, 4
