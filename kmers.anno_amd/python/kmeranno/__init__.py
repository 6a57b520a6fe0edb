"""ctypes binding of libkmeranno.so (include/kmeranno.h) for tests and bench.py.

The library is the product; this module only marshals numpy buffers (host entry points) or
raw device pointers (the ``*_device`` entry points, e.g. torch tensors' ``data_ptr()``).
There is no CPU fallback: if the shared library is missing or no HIP device is usable,
calls raise ``KmerAnnoError``.
"""

from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB_PATH = os.environ.get("KMERANNO_LIB") or os.path.join(PKG_ROOT, "build", "libkmeranno.so")

OK = 0
E_INVALID, E_DEVICE, E_NOMEM, E_CAPACITY, E_ALPHABET, E_TABLE_FULL = -1, -2, -3, -4, -5, -6
E_IO = -7
STATUS_NONE, STATUS_CALLED, STATUS_AMBIGUOUS, STATUS_BELOW_MIN = 0, 1, 2, 3
F_END_EXCLUSIVE, F_MULTISET = 0x1, 0x2
MAX_K = 12  # K <= 8: narrow tables (8-byte slots); 9..12: wide tables (16-byte slots)
ORF_KEPT, ORF_REJECTED, ORF_WEAK, ORF_SMALL = 0, 1, 2, 3  # extend_proposals' status
TR_PEG = 1  # translate_locations' flag: pegTranslate (last codon dropped, start codon -> 'M')
MD5_UPPER = 1  # sequence_md5 / check_sequences' flag: 'a'..'z' hashed as 'A'..'Z'
MD5_STATIC, MD5_COOP = 1, 2  # kernel forms of the measurement hook (csrc/kma_md5.h)

# Every symbol include/kmeranno.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "kma_abi_version", "kma_last_error", "kma_device_count", "kma_pack_kmers",
    "kma_table_create", "kma_table_create_packed", "kma_table_info_get", "kma_table_destroy",
    "kma_table_buckets_for", "kma_table_build_device", "kma_table_wrap_device",
    "kma_table_device_ptr", "kma_workspace_create", "kma_workspace_reserve",
    "kma_workspace_destroy", "kma_workspace_timing", "kma_workspace_timing_read",
    "kma_annotate_proteins", "kma_annotate_proteins_device", "kma_annotate_contigs",
    "kma_workspace_reserve_contigs", "kma_annotate_contigs_device", "kma_contig_window_count",
    "kma_peg_table_create", "kma_connect_pegs", "kma_build_signatures", "kma_table_layout_for",
    "kma_table_create_replicated", "kma_table_replicate", "kma_table_replicas",
    "kma_bucket_slots", "kma_protein_distances", "kma_protein_best_match",
    "kma_workspace_reserve_batch", "kma_workspace_phases_read", "kma_propose_pegs",
    "kma_hash_annotate", "kma_bucket_slots_for", "kma_table_buckets_for_k",
    "kma_option_set", "kma_option_get", "kma_workspace_option_set",
    "kma_packed_bytes", "kma_pack_residues", "kma_annotate_packed_device",
    "kma_table_create_from_tsv", "kma_free",
    "kma_orf_index_create", "kma_orf_index_destroy", "kma_extend_proposals",
    "kma_translate_locations",
    "kma_sequence_md5_device", "kma_sequence_md5", "kma_check_sequences",
    "kma_proto_index_create", "kma_proto_index_info", "kma_proto_index_destroy",
    "kma_hash_annotate_indexed",
    "kma_hash_scratch_bytes", "kma_hash_annotate_indexed_device",
    "kma_sig_builder_create", "kma_sig_builder_add", "kma_sig_builder_info_get",
    "kma_sig_builder_finish", "kma_sig_builder_destroy",
)

# Tuning options (include/kmeranno.h "options"): library-wide defaults read per call.
OPT_LAYOUT, OPT_BLOCK_PROTEINS, OPT_DEFER, OPT_HOST_PIECES, OPT_HASH_SLICE = 1, 2, 3, 4, 5
OPT_PACKED_INPUT, OPT_HOST_THREADS, OPT_HOST_SLICE, OPT_PLACEMENT = 6, 7, 8, 9
OPT_HOST_PIECE_MIN, OPT_HASH_CAP, OPT_HASH_LDS_KEYS = 10, 12, 13  # (11 is no option)
OPT_DEFAULTS = {OPT_LAYOUT: -1, OPT_BLOCK_PROTEINS: 0, OPT_DEFER: -1, OPT_HOST_PIECES: 0,
                OPT_HASH_SLICE: 0, OPT_PACKED_INPUT: 1, OPT_HOST_THREADS: 0, OPT_HOST_SLICE: 0,
                OPT_PLACEMENT: -1, OPT_HOST_PIECE_MIN: 0, OPT_HASH_CAP: 0,
                OPT_HASH_LDS_KEYS: 0}
LAYOUT_TWO_CHOICE = 0x100  # layout code flag: two-choice placement (include/kmeranno.h)
LAYOUT_MOD_SAMPLING = 0x40  # layout code flag: the mod-sampling minimizer order (K = 8, m = 6)
OPT_DEFAULT = -(1 << 63)  # kma_workspace_option_set: follow the library default
_OPT_NAMES = {"layout": OPT_LAYOUT, "block_proteins": OPT_BLOCK_PROTEINS, "defer": OPT_DEFER,
              "host_pieces": OPT_HOST_PIECES, "hash_slice": OPT_HASH_SLICE,
              "packed_input": OPT_PACKED_INPUT, "host_threads": OPT_HOST_THREADS,
              "host_slice": OPT_HOST_SLICE, "placement": OPT_PLACEMENT,
              "host_piece_min": OPT_HOST_PIECE_MIN, "hash_cap": OPT_HASH_CAP,
              "hash_lds_keys": OPT_HASH_LDS_KEYS}


class KmerAnnoError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"kmeranno error {code}: {msg}")
        self.code = code


class TableInfo(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_skipped", C.c_uint64), ("n_entries", C.c_uint64),
                ("n_buckets", C.c_uint64), ("bytes", C.c_uint64), ("k", C.c_int32),
                ("device", C.c_int32), ("max_probe", C.c_uint32), ("n_extra_syms", C.c_uint32),
                ("extra_syms", C.c_uint8 * 4), ("minimizer_len", C.c_int32),
                ("n_displaced", C.c_uint64), ("n_replicas", C.c_int32),
                ("slots_per_bucket", C.c_int32), ("replicate_ms", C.c_double),
                ("replicate_bytes", C.c_uint64), ("two_choice", C.c_int32),
                ("minimizer_order", C.c_int32), ("replicate_peer", C.c_int32),
                ("replicate_local", C.c_int32)]


class ProtoIndexInfo(C.Structure):
    _fields_ = [("n_proto", C.c_uint32), ("k", C.c_int32), ("n_keys", C.c_uint64),
                ("n_postings", C.c_uint64), ("bytes", C.c_uint64)]


class SigBuilderInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("flags", C.c_uint32), ("tile", C.c_uint32),
                ("n_adds", C.c_uint32), ("n_residues", C.c_uint64), ("n_keys", C.c_uint64),
                ("n_role", C.c_uint64), ("n_conflict", C.c_uint64), ("n_buffered", C.c_uint64),
                ("bytes", C.c_uint64)]


HIT_DTYPE = np.dtype([("contig", "<u4"), ("left", "<i4"), ("fid", "<u4"), ("strand", "u1"),
                      ("frame", "u1"), ("pad", "<u2")])
PROPOSAL_DTYPE = np.dtype([("peg", "<u4"), ("contig", "<u4"), ("left", "<i4"), ("right", "<i4"),
                           ("evidence", "<u4"), ("strand", "u1"), ("frame", "u1"),
                           ("pad", "<u2")])
LOCATION_DTYPE = np.dtype([("contig", "<u4"), ("left", "<i4"), ("right", "<i4"),
                           ("strand", "u1"), ("pad", "u1", (3,))])

_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C")
_vp, _u64, _u32, _int = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
_lib = None


def load(path: str | None = None):
    """Load libkmeranno.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise KmerAnnoError(E_DEVICE, f"{p} not built (run `make -C kmers.anno_amd`)")
        L = C.CDLL(p)
        L.kma_last_error.restype = C.c_char_p
        L.kma_device_count.argtypes = [C.POINTER(C.c_int)]
        L.kma_pack_kmers.argtypes = [_vp, C.c_char_p, _u64p, _u64, _u64p]
        L.kma_table_create.argtypes = [C.c_char_p, _u64p, _u32p, _u64, _int, _int, C.c_double,
                                       C.POINTER(_vp)]
        L.kma_table_create_packed.argtypes = [_u64p, _u32p, _u64, _int, _int, C.c_double,
                                              C.POINTER(_vp)]
        L.kma_table_info_get.argtypes = [_vp, C.POINTER(TableInfo)]
        L.kma_table_destroy.argtypes = [_vp]
        L.kma_table_buckets_for.restype = _u64
        L.kma_table_buckets_for.argtypes = [_u64, C.c_double]
        L.kma_table_buckets_for_k.restype = _u64
        L.kma_table_buckets_for_k.argtypes = [_u64, C.c_double, _int]
        L.kma_bucket_slots_for.argtypes = [_int]
        L.kma_table_build_device.argtypes = [_vp, _u64, _int, _int, _vp, _vp, _vp, _u64, _vp,
                                             _vp]
        L.kma_table_wrap_device.argtypes = [_vp, _u64, _int, _int, _int, C.POINTER(_vp)]
        L.kma_table_layout_for.argtypes = [_int, _u64]
        L.kma_protein_distances.argtypes = [_u8p, _u64p, _u32, _int, _u32, _u32p, _u32p, _u64,
                                            _int, _u32p, _vp, _vp]
        L.kma_protein_best_match.argtypes = [_u8p, _u64p, _u32, _int, _u32, _u32p, _u64p, _u32p,
                                             _u32, C.c_double, _int, _i32p, _vp]
        L.kma_table_create_replicated.argtypes = [C.c_char_p, _u64p, _u32p, _u64, _int, _int,
                                                  _i32p, C.c_double, C.POINTER(_vp)]
        L.kma_table_replicate.argtypes = [_vp, _int, _i32p]
        L.kma_table_create_from_tsv.argtypes = [C.c_char_p, _int, _int, _i32p, C.c_double,
                                                C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64),
                                                C.POINTER(_u32), C.POINTER(_int)]
        L.kma_free.argtypes = [_vp]
        L.kma_free.restype = None
        L.kma_table_replicas.argtypes = [_vp, C.POINTER(_int), _vp, _int]
        L.kma_table_device_ptr.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_u64)]
        L.kma_workspace_create.argtypes = [_int, C.POINTER(_vp)]
        L.kma_workspace_destroy.argtypes = [_vp]
        L.kma_workspace_reserve.argtypes = [_vp, _u64]
        L.kma_workspace_timing.argtypes = [_vp, _int]
        L.kma_workspace_timing_read.argtypes = [_vp, C.POINTER(_u32), C.POINTER(C.c_double),
                                                C.POINTER(C.c_double)]
        L.kma_workspace_reserve_batch.argtypes = [_vp, _u64, _u64]
        L.kma_workspace_phases_read.argtypes = [_vp, C.POINTER(_u32), C.POINTER(_int),
                                                C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
        L.kma_annotate_proteins.argtypes = [_vp, _u8p, _u64p, _u32, _int, _u32, _i32p, _i32p,
                                            _u8p, _vp, _u32]
        L.kma_annotate_proteins_device.argtypes = [_vp, _vp, _vp, _vp, _u32, _u64, _int, _u32,
                                                   _vp, _vp, _vp, _vp, _u32, _vp]
        L.kma_annotate_contigs.argtypes = [_vp, _u8p, _u64p, _u32, _int, _vp, _u64,
                                           C.POINTER(_u64), _vp, _u32]
        L.kma_workspace_reserve_contigs.argtypes = [_vp, _u64]
        L.kma_annotate_contigs_device.argtypes = [_vp, _vp, _vp, _vp, _u32, _u64, _int, _vp,
                                                  _u64, _vp, _vp, _u32, _vp]
        L.kma_build_signatures.argtypes = [_u8p, _u64p, _i32p, _u32, _int, _u32, _int, _vp, _vp,
                                           _u64, C.POINTER(_u64)]
        L.kma_sig_builder_create.argtypes = [_int, _u32, _int, C.POINTER(_vp)]
        L.kma_sig_builder_add.argtypes = [_vp, _vp, _vp, _vp, _u32]
        L.kma_sig_builder_info_get.argtypes = [_vp, C.POINTER(SigBuilderInfo)]
        L.kma_sig_builder_finish.argtypes = [_vp, _vp, _vp, _u64, C.POINTER(_u64)]
        L.kma_sig_builder_destroy.argtypes = [_vp]
        L.kma_peg_table_create.argtypes = [_u8p, _u64p, _u32, _int, _int, C.c_double,
                                           C.POINTER(_vp), C.POINTER(_u64)]
        L.kma_connect_pegs.argtypes = [_vp, _u8p, _u64p, _u32, _int, _int, _vp, _u64,
                                       C.POINTER(_u64)]
        L.kma_hash_annotate.argtypes = [_u8p, _u64p, _u32, _u8p, _u64p, _u32, _int, C.c_double,
                                        _int, _vp, _vp, _vp]
        L.kma_propose_pegs.argtypes = [_vp, _u64, _u32p, _u32, _int, C.c_double, C.c_double,
                                       C.c_double, _int, _vp, _u64, C.POINTER(_u64), _u64p]
        L.kma_orf_index_create.argtypes = [_vp, _vp, _u32, _int, _int, C.POINTER(_vp)]
        L.kma_orf_index_destroy.argtypes = [_vp]
        L.kma_extend_proposals.argtypes = [_vp, _vp, _u64, C.c_double, _int, _vp, _vp, _vp, _vp]
        L.kma_translate_locations.argtypes = [_vp, _vp, _u32, _int, _int, _vp, _u64, _int, _vp,
                                              _u64, _vp]
        L.kma_sequence_md5_device.argtypes = [_int, _vp, _vp, _u32, _u64, _u32, _vp, _vp]
        L.kma_debug_sequence_md5_device.argtypes = [_int, _vp, _vp, _u32, _u64, _u32, _vp, _vp,
                                                    _u32, _u32]
        L.kma_sequence_md5.argtypes = [_vp, _vp, _u32, _u32, _int, _vp]
        L.kma_check_sequences.argtypes = [_vp, _vp, _u32, _u32, _vp, _int, _vp, _vp, _vp, _vp,
                                          _vp]
        L.kma_proto_index_create.argtypes = [_vp, _vp, _u32, _int, _int, C.POINTER(_vp)]
        L.kma_proto_index_info.argtypes = [_vp, C.POINTER(ProtoIndexInfo)]
        L.kma_proto_index_destroy.argtypes = [_vp]
        L.kma_hash_annotate_indexed.argtypes = [_vp, _vp, _vp, _u32, C.c_double, _vp, _vp, _vp,
                                                _vp]
        L.kma_hash_scratch_bytes.restype = _u64
        L.kma_hash_scratch_bytes.argtypes = [_u64, _u32]
        L.kma_hash_annotate_indexed_device.argtypes = [_vp, _vp, _vp, _u32, _u64, C.c_double,
                                                       _vp, _u64, _vp, _vp, _vp, _vp, _vp]
        L.kma_debug_translate_ms.restype = C.c_double
        L.kma_debug_translate_ms.argtypes = []
        L.kma_contig_window_count.restype = _u64
        L.kma_contig_window_count.argtypes = [_u64p, _u32, _int]
        L.kma_option_set.argtypes = [_int, C.c_int64]
        L.kma_option_get.argtypes = [_int, C.POINTER(C.c_int64)]
        L.kma_workspace_option_set.argtypes = [_vp, _int, C.c_int64]
        L.kma_packed_bytes.restype = _u64
        L.kma_packed_bytes.argtypes = [_u64]
        L.kma_pack_residues.argtypes = [_vp, _u8p, _u64, _u8p, _u64]
        L.kma_annotate_packed_device.argtypes = [_vp, _vp, _vp, _vp, _u32, _u64, _int, _u32,
                                                 _vp, _vp, _vp, _vp, _u32, _vp]
        _lib = L
    return _lib


def _check(rc: int):
    if rc != OK:
        raise KmerAnnoError(rc, load().kma_last_error().decode(errors="replace"))


def set_option(option: int, value: int):
    """Library-wide tuning default (OPT_* ; see include/kmeranno.h)."""
    _check(load().kma_option_set(option, int(value)))


def get_option(option: int) -> int:
    v = C.c_int64()
    _check(load().kma_option_get(option, C.byref(v)))
    return v.value


def reset_options():
    for o, v in OPT_DEFAULTS.items():
        set_option(o, v)


@contextlib.contextmanager
def options(**kw):
    """Set options by name (layout=, block_proteins=, defer=, host_pieces=, hash_slice=, ...) for
    the body, then restore the previous values."""
    old = {_OPT_NAMES[k]: get_option(_OPT_NAMES[k]) for k in kw}
    try:
        for k, v in kw.items():
            set_option(_OPT_NAMES[k], v)
        yield
    finally:
        for o, v in old.items():
            set_option(o, v)


def source_digest() -> str:
    """sha256[:16] of the native sources (csrc/ and the ABI header): stamps counter summaries
    under profiles/ so that a bench run can tell whether they describe the kernels it runs."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(PKG_ROOT, "csrc")
    hdr = os.path.join(os.path.dirname(PKG_ROOT), "include", "kmeranno.h")
    for f in sorted(os.listdir(csrc)) + [hdr]:
        path = f if os.path.isabs(f) else os.path.join(csrc, f)
        if os.path.isfile(path):
            h.update(os.path.basename(path).encode())
            h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def device_count() -> int:
    n = C.c_int(0)
    _check(load().kma_device_count(C.byref(n)))
    return n.value


def pack_strings(strs):
    """Concatenate strings -> (uint8 buffer padded by 32 bytes, uint64 offsets)."""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in strs]
    offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(bs) + b"\0" * 32, dtype=np.uint8).copy()
    return buf, offsets


def std_codes(ascii_bytes: np.ndarray) -> np.ndarray:
    """Standard 5-bit residue codes ('A'..'Z' -> 1..26, '*' -> 27, other -> 0)."""
    b = ascii_bytes.astype(np.int64)
    c = np.where((b >= 65) & (b <= 90), b - 64, 0)
    return np.where(b == 42, 27, c).astype(np.uint64)


def pack_std(kmers_u8: np.ndarray) -> np.ndarray:
    """Pack an (n, k) uint8 array of ASCII kmers into keys (standard alphabet, 0 if invalid)."""
    codes = std_codes(kmers_u8)
    k = kmers_u8.shape[1]
    keys = np.zeros(len(kmers_u8), np.uint64)
    for j in range(k):
        keys = (keys << np.uint64(5)) | codes[:, j]
    keys[(codes == 0).any(axis=1)] = 0
    return keys


class SignatureTable:
    """A signature table resident on one GPU (ApplyKmerProcessor.java:100-110)."""

    def __init__(self, handle, owner=True):
        self._h = handle
        self._owner = owner

    @classmethod
    def from_rows(cls, kmers, fids, k: int = 8, device: int = 0, load_factor: float = 0.5):
        buf, off = pack_strings(kmers)
        h = _vp()
        _check(load().kma_table_create(buf.tobytes(), off, np.ascontiguousarray(fids, np.uint32),
                                       len(off) - 1, k, device, load_factor, C.byref(h)))
        return cls(h)

    @classmethod
    def from_packed(cls, keys, fids, k: int = 8, device: int = 0, load_factor: float = 0.5):
        keys = np.ascontiguousarray(keys, np.uint64)
        h = _vp()
        _check(load().kma_table_create_packed(keys, np.ascontiguousarray(fids, np.uint32),
                                              len(keys), k, device, load_factor, C.byref(h)))
        return cls(h)

    @classmethod
    def from_pegs(cls, residues, offsets, k: int = 8, device: int = 0, load_factor: float = 0.5):
        """Singleton peg-kmer table of a close genome (fid = peg index); see kma_peg_table_create.
        Returns (table, counted windows)."""
        residues = np.ascontiguousarray(residues, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        h, nw = _vp(), _u64()
        _check(load().kma_peg_table_create(residues, offsets, len(offsets) - 1, k, device,
                                           load_factor, C.byref(h), C.byref(nw)))
        return cls(h), nw.value

    @classmethod
    def from_rows_replicated(cls, kmers, fids, devices, k: int = 8, load_factor: float = 0.5):
        """One table with a replica on each listed device (a device may repeat); host calls
        shard their batch over the replicas."""
        buf, off = pack_strings(kmers)
        dv = np.ascontiguousarray(devices, np.int32)
        h = _vp()
        _check(load().kma_table_create_replicated(buf.tobytes(), off,
                                                  np.ascontiguousarray(fids, np.uint32),
                                                  len(off) - 1, k, len(dv), dv, load_factor,
                                                  C.byref(h)))
        return cls(h)

    @classmethod
    def from_tsv(cls, path: str, k: int = 8, devices=(0,), load_factor: float = 0.5):
        """The table of apply's kmerdb.tbl read by the library (kma_table_create_from_tsv):
        returns (table, role ids in fid order, the last row's kmer length)."""
        dv = np.ascontiguousarray(devices, np.int32)
        h, names, nb, nr, last = _vp(), _vp(), _u64(), _u32(), _int()
        _check(load().kma_table_create_from_tsv(os.fsencode(path), k, len(dv), dv, load_factor,
                                                C.byref(h), C.byref(names), C.byref(nb),
                                                C.byref(nr), C.byref(last)))
        try:
            blob = C.string_at(names.value, nb.value) if nb.value else b""
        finally:
            load().kma_free(names)
        roles = [r.decode() for r in blob.split(b"\0")[:-1]] if blob else []
        assert len(roles) == nr.value
        return cls(h), roles, last.value

    @classmethod
    def wrap_device(cls, d_slots: int, n_buckets: int, k: int = 8, device: int = 0,
                    layout: int = -1):
        h = _vp()
        _check(load().kma_table_wrap_device(d_slots, n_buckets, k, layout, device, C.byref(h)))
        return cls(h)

    def replicate(self, devices):
        dv = np.ascontiguousarray(devices, np.int32)
        _check(load().kma_table_replicate(self._h, len(dv), dv))

    @property
    def replicas(self):
        n = _int(0)
        _check(load().kma_table_replicas(self._h, C.byref(n), None, 0))
        out = (C.c_int * max(n.value, 1))()
        _check(load().kma_table_replicas(self._h, C.byref(n), out, n.value))
        return list(out)[:n.value]

    @property
    def info(self) -> TableInfo:
        i = TableInfo()
        _check(load().kma_table_info_get(self._h, C.byref(i)))
        return i

    def device_ptr(self):
        p, n = _vp(), _u64()
        _check(load().kma_table_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def pack(self, kmers) -> np.ndarray:
        buf, off = pack_strings(kmers)
        out = np.zeros(len(off) - 1, np.uint64)
        _check(load().kma_pack_kmers(self._h, buf.tobytes(), off, len(off) - 1, out))
        return out

    def close(self):
        if self._h:
            load().kma_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Workspace:
    def __init__(self, device: int = 0, n_residues: int = 0, n_seq: int = 0):
        self._h = _vp()
        _check(load().kma_workspace_create(device, C.byref(self._h)))
        if n_residues:
            self.reserve(n_residues, n_seq)

    def reserve(self, n_residues: int, n_seq: int = 0):
        """Scratch for device calls of up to n_residues residues and n_seq proteins (0: the
        library's default of n_residues / 16 + 256)."""
        if n_seq:
            _check(load().kma_workspace_reserve_batch(self._h, n_residues, n_seq))
        else:
            _check(load().kma_workspace_reserve(self._h, n_residues))

    def reserve_contigs(self, n_bases: int):
        _check(load().kma_workspace_reserve_contigs(self._h, n_bases))

    def set_option(self, option: int, value: int = OPT_DEFAULT):
        """Per-workspace override of OPT_BLOCK_PROTEINS / OPT_DEFER (OPT_DEFAULT: none)."""
        _check(load().kma_workspace_option_set(self._h, option, int(value)))

    def timing(self, enable: bool = True):
        """Per-phase hipEvent timing of the device calls made with this workspace."""
        _check(load().kma_workspace_timing(self._h, int(enable)))

    def timing_read(self):
        """(n_calls, kernel_ms_total, rest_ms_total) since the last read; clears them."""
        n, p, v = _u32(), C.c_double(), C.c_double()
        _check(load().kma_workspace_timing_read(self._h, C.byref(n), C.byref(p), C.byref(v)))
        return n.value, p.value, v.value

    def phases_read(self):
        """(n_calls, {phase name: summed ms}) of the calls laid out like the last one (same
        path) since the last read; clears them."""
        n, k = _u32(), _int()
        ms = (C.c_double * 8)()
        names = (C.c_char_p * 8)()
        _check(load().kma_workspace_phases_read(self._h, C.byref(n), C.byref(k), ms, names))
        return n.value, {names[i].decode(): ms[i] for i in range(k.value)}

    def close(self):
        if self._h:
            load().kma_workspace_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def buckets_for(n_keys: int, load_factor: float = 0.5, k: int = 8) -> int:
    return int(load().kma_table_buckets_for_k(n_keys, load_factor, k))


def bucket_slots(k: int = 8) -> int:
    """Slots per bucket of a table of k-mers: narrow (k <= 8) u64 slots of this build (8: 64-byte
    buckets; 16: the 128-byte variant), wide (k 9..12) 4 slots of 16 bytes."""
    return int(load().kma_bucket_slots_for(k))


def layout_for(k: int, n_buckets: int) -> int:
    """The size-derived table layout code (minimizer length, 0 = flat; | LAYOUT_TWO_CHOICE when
    the creators try two-choice placement first)."""
    return int(load().kma_table_layout_for(k, n_buckets))


# The creators' layout rule by measurement (kma_internal.h kRetryDisplaced / kMaxDisplaced /
# kMaxChain / kMaxDisplacedTwoChoice; kma_abi.cpp create_from_device_keys).
RETRY_DISPLACED, MAX_DISPLACED, MAX_CHAIN = 0.10, 0.15, 32
MAX_DISPLACED_TWO_CHOICE = 0.40


def choose_layout(k: int, n_buckets: int, build):
    """The library creators' layout choice for hosts that build tables on the device
    themselves (kma_table_build_device into their own buffer, e.g. one RCCL broadcasts):
    build(code) builds the table with that layout code (minimizer length | LAYOUT_TWO_CHOICE)
    into the caller's buffer and returns its status {failed, entries, longest chain,
    displaced}. Returns (code, status); the kept layout is the one built last. Two-choice
    placement first (narrow tables; a failed minimizer build is retried flat); a failed
    two-choice build falls back to the chained rule.
    A forced layout (OPT_LAYOUT) is the size rule's answer."""
    def disp(s):
        return s[3] / max(s[1], 1)
    forced = get_option(OPT_LAYOUT) != -1
    code = layout_for(k, n_buckets)
    m = code & 0xFF
    if code & LAYOUT_TWO_CHOICE:
        st = build(code)
        if st[0] != 0 and m != 0 and not forced:  # out of evictions: retried flat
            s2 = build(LAYOUT_TWO_CHOICE)
            if s2[0] == 0:
                return LAYOUT_TWO_CHOICE, s2
        if st[0] == 0:
            if not forced and m != 0 and disp(st) > MAX_DISPLACED_TWO_CHOICE:
                s2 = build(LAYOUT_TWO_CHOICE)
                if s2[0] == 0 and 2 * s2[3] < st[3]:
                    return LAYOUT_TWO_CHOICE, s2
                st = build(code)
            return code, st
    st = build(m)
    if forced:
        return m, st
    m6, m7 = min(k, 6), min(k, 7)
    if m & 0x3F == m6 and m6 != m7 and disp(st) > RETRY_DISPLACED:
        s2 = build(m7)
        if s2[3] < st[3]:
            m, st = m7, s2
        else:
            st = build(m)
    if m != 0 and (disp(st) > MAX_DISPLACED or st[2] > MAX_CHAIN):
        s2 = build(0)
        if 2 * s2[3] < st[3] or (st[2] > MAX_CHAIN and 2 * s2[2] < st[2]):
            m, st = 0, s2
        else:
            st = build(m)
    return m, st


def build_device(d_slots: int, n_buckets: int, d_winner: int, d_keys: int, d_fids: int, n: int,
                 d_status: int, stream: int = 0, k: int = 8, layout: int = -1):
    """Device-resident table build; d_status (4 x u32) <- {full, entries, longest chain,
    displaced keys}."""
    _check(load().kma_table_build_device(d_slots, n_buckets, k, layout, d_winner, d_keys, d_fids,
                                         n, d_status, stream or None))


def annotate_proteins(table: SignatureTable, residues: np.ndarray, offsets: np.ndarray,
                      min_hits: int = 5, flags: int = 0, n_fid: int = 0, out=None):
    """Host form of the apply loop: returns (fid, count, status, tally-or-None). out: the
    caller's (fid, count, status[, tally]) arrays to fill (reused buffers, as a JNI caller
    passes its direct buffers: fresh arrays cost their first-touch page faults)."""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    if out is not None:
        fid, cnt, st = out[:3]
        assert fid.dtype == np.int32 and cnt.dtype == np.int32 and st.dtype == np.uint8
        assert len(fid) == len(cnt) == len(st) == n and fid.flags.c_contiguous
        tally = (out[3] if len(out) > 3 else np.zeros(n_fid, np.uint32)) if n_fid else None
        if tally is not None:
            tally[:] = 0
    else:
        fid, cnt, st = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8)
        tally = np.zeros(n_fid, np.uint32) if n_fid else None
    _check(load().kma_annotate_proteins(table._h, residues, offsets, n, min_hits, flags, fid, cnt,
                                        st, tally.ctypes.data if n_fid else None, n_fid))
    return fid, cnt, st, tally


def annotate_proteins_device(table: SignatureTable, ws: Workspace, d_residues: int,
                             d_offsets: int, n_seq: int, n_residues: int, min_hits: int,
                             flags: int, d_fid: int, d_count: int, d_status: int, d_tally: int = 0,
                             n_fid: int = 0, stream: int = 0):
    _check(load().kma_annotate_proteins_device(table._h, ws._h, d_residues, d_offsets, n_seq,
                                               n_residues, min_hits, flags, d_fid, d_count,
                                               d_status, d_tally or None, n_fid, stream or None))


HOST_PROFILE_FIELDS = ("setup_ms", "stage_ms", "launch_ms", "wait_ms", "outputs_ms", "call_ms",
                       "staging_threads", "pieces")


def host_profile(replica: int | None = None) -> dict:
    """The library's host-side phase profile (measurement hook, not in kmeranno.h) of the last
    host protein shard call, or of replica `replica`'s last shard of a fanned-out call."""
    L = load()
    p = (C.c_double * len(HOST_PROFILE_FIELDS))()
    if replica is None:
        _check(L.kma_debug_host_profile(p, len(p)))
    else:
        _check(L.kma_debug_host_profile_replica(replica, p, len(p)))
    return dict(zip(HOST_PROFILE_FIELDS, list(p)))


def host_cores() -> int:
    """CPUs the library sizes its staging jobs by (affinity mask bounded by the cgroup quota)."""
    return int(load().kma_debug_host_cores())


def packed_bytes(n_residues: int) -> int:
    return int(load().kma_packed_bytes(n_residues))


def pack_residues(table, residues: np.ndarray, n: int | None = None) -> np.ndarray:
    """The packed residue stream (5 bits per residue, the table's codes; table None: the
    standard alphabet) of residues[0, n)."""
    residues = np.ascontiguousarray(residues, np.uint8)
    n = len(residues) if n is None else n
    out = np.empty(packed_bytes(n), np.uint8)
    _check(load().kma_pack_residues(table._h if table is not None else None, residues, n, out,
                                    len(out)))
    return out


def annotate_packed_device(table: SignatureTable, ws: Workspace, d_stream: int, d_offsets: int,
                           n_seq: int, n_residues: int, min_hits: int, flags: int, d_fid: int,
                           d_count: int, d_status: int, d_tally: int = 0, n_fid: int = 0,
                           stream: int = 0):
    _check(load().kma_annotate_packed_device(table._h, ws._h, d_stream, d_offsets, n_seq,
                                             n_residues, min_hits, flags, d_fid, d_count,
                                             d_status, d_tally or None, n_fid, stream or None))


def annotate_contigs(table: SignatureTable, dna: np.ndarray, offsets: np.ndarray,
                     genetic_code: int = 11, n_fid: int = 0):
    """6-frame annotation: returns (hits structured array, tally[n_contig, n_fid] or None)."""
    dna = np.ascontiguousarray(dna, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n_contig = len(offsets) - 1
    cap = max(1024, int(load().kma_contig_window_count(offsets, n_contig, table.info.k)) // 8)
    while True:
        hits = np.empty(cap, HIT_DTYPE)
        tally = np.zeros((n_contig, n_fid), np.uint32) if n_fid else None
        nh = _u64()
        rc = load().kma_annotate_contigs(table._h, dna, offsets, n_contig, genetic_code,
                                         hits.ctypes.data, cap, C.byref(nh),
                                         tally.ctypes.data if n_fid else None, n_fid)
        if rc == E_CAPACITY:
            cap = nh.value
            continue
        _check(rc)
        return hits[:nh.value], tally


def annotate_contigs_device(table: SignatureTable, ws: Workspace, d_dna: int, d_offsets: int,
                            n_contig: int, n_bases: int, genetic_code: int, d_hits: int, cap: int,
                            d_n_hits: int, d_tally: int = 0, n_fid: int = 0, stream: int = 0):
    """Device form of the 6-frame pass (asynchronous on `stream`; *d_n_hits gets the total)."""
    _check(load().kma_annotate_contigs_device(table._h, ws._h, d_dna, d_offsets, n_contig,
                                              n_bases, genetic_code, d_hits or None, cap,
                                              d_n_hits, d_tally or None, n_fid, stream or None))


def connect_pegs(peg_table: SignatureTable, dna: np.ndarray, offsets: np.ndarray,
                 genetic_code: int = 11, strict: bool = False):
    """KmerProcessor.java:195-207: (hits with fid = peg index) in canonical order."""
    dna = np.ascontiguousarray(dna, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n_contig = len(offsets) - 1
    cap = 1024
    while True:
        hits = np.empty(cap, HIT_DTYPE)
        nh = _u64()
        rc = load().kma_connect_pegs(peg_table._h, dna, offsets, n_contig, genetic_code,
                                     int(strict), hits.ctypes.data, cap, C.byref(nh))
        if rc == E_CAPACITY:
            cap = nh.value
            continue
        _check(rc)
        return hits[:nh.value]


def propose_pegs(hits: np.ndarray, peg_len, k: int = 8, min_strength: float = 0.5,
                 max_fuzz: float = 1.5, min_fuzz: float = 0.8, device: int = 0):
    """KmerProcessor.java:209-264 on the GPU: the proposal sweep over the framed location lists
    of connect_pegs' hits (fid = peg index). Returns (PROPOSAL_DTYPE array, stats[4] =
    lists, too few kmers, too short, proposals)."""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    peg_len = np.ascontiguousarray(peg_len, np.uint32)
    stats = np.zeros(4, np.uint64)
    cap = max(16, len(hits) // 4)
    while True:
        out = np.empty(cap, PROPOSAL_DTYPE)
        n = _u64()
        rc = load().kma_propose_pegs(hits.ctypes.data if len(hits) else None, len(hits), peg_len,
                                     len(peg_len), k, min_strength, max_fuzz, min_fuzz, device,
                                     out.ctypes.data, cap, C.byref(n), stats)
        if rc == E_CAPACITY:
            cap = n.value
            continue
        _check(rc)
        return out[:n.value], stats


class OrfIndex:
    """One genome's ORF index on one GPU (kma_orf_index_create): per (contig, strand, frame) the
    next in-frame stop and the farthest start since the previous stop, built once per new genome
    and read by extend_proposals for every close genome. dna / offsets as pack_strings gives
    them; genetic_code 1, 4 or 11."""

    def __init__(self, dna, offsets, genetic_code: int = 11, device: int = 0):
        dna = np.ascontiguousarray(dna, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        self._h = None
        h = _vp()
        _check(load().kma_orf_index_create(dna.ctypes.data if len(dna) else None,
                                           offsets.ctypes.data, len(offsets) - 1, genetic_code,
                                           device, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            load().kma_orf_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def extend_proposals(index: OrfIndex, proposals: np.ndarray, min_strength: float,
                     min_evidence: int):
    """PegProposalList.propose's first half on the GPU (kma_extend_proposals): every proposal
    (PROPOSAL_DTYPE, as propose_pegs returns them) extended to its ORF and filtered. min_strength
    is the DNA strength (minStrength / 3). Returns (left, right, status, stats[4] = made,
    rejected, weak, small), entry i for proposal i; left = right = 0 where status is
    ORF_REJECTED."""
    if index._h is None:
        raise KmerAnnoError(E_INVALID, "the ORF index is closed")
    proposals = np.ascontiguousarray(proposals, PROPOSAL_DTYPE)
    n = len(proposals)
    left, right = np.zeros(n, np.int32), np.zeros(n, np.int32)
    status = np.zeros(n, np.uint8)
    stats = np.zeros(4, np.uint64)
    _check(load().kma_extend_proposals(index._h, proposals.ctypes.data if n else None, n,
                                       min_strength, min_evidence, left.ctypes.data,
                                       right.ctypes.data, status.ctypes.data, stats.ctypes.data))
    return left, right, status, stats


def make_locations(rows) -> np.ndarray:
    """rows of (contig index, strand '+' / '-', left, right) -> LOCATION_DTYPE."""
    rows = list(rows)
    locs = np.zeros(len(rows), LOCATION_DTYPE)
    if rows:
        locs["contig"] = [r[0] for r in rows]
        locs["strand"] = [ord(r[1]) for r in rows]
        locs["left"] = [r[2] for r in rows]
        locs["right"] = [r[3] for r in rows]
    return locs


def translate_locations(dna, offsets, locs, genetic_code: int = 11, peg: bool = False,
                        device: int = 0):
    """kma_translate_locations: the proteins of locations (LOCATION_DTYPE; 1-based inclusive
    forward edges, either strand) of a genome (dna / offsets as pack_strings gives them) on the
    GPU. peg: KmerProcessor.makeFeature's pegTranslate (the last codon dropped, a start codon
    first gives 'M'). Returns (residues u8 padded by 32 bytes, offsets u64), the layout
    annotate_proteins takes. The output is sized here by the library's own length rule (invalid
    locations are the library's to refuse)."""
    dna = np.ascontiguousarray(dna, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    locs = np.ascontiguousarray(locs, LOCATION_DTYPE)
    n = len(locs)
    codons = (locs["right"].astype(np.int64) - locs["left"] + 1) // 3 - (1 if peg else 0)
    total = int(np.maximum(codons, 0).sum())
    out = np.zeros(total + 32, np.uint8)
    out_off = np.zeros(n + 1, np.uint64)
    _check(load().kma_translate_locations(dna.ctypes.data if len(dna) else None,
                                          offsets.ctypes.data, len(offsets) - 1, genetic_code,
                                          device, locs.ctypes.data if n else None, n,
                                          TR_PEG if peg else 0, out.ctypes.data, total,
                                          out_off.ctypes.data))
    return out, out_off


def translate_kernel_ms() -> float:
    """hipEvent time of the kernel of this thread's last translate_locations call (measurement
    hook, not in kmeranno.h)."""
    return float(load().kma_debug_translate_ms())


def sequence_md5(residues, offsets, flags: int = 0, device: int = 0) -> np.ndarray:
    """kma_sequence_md5: the RFC 1321 digests of a host batch (residues / offsets as
    pack_strings gives them) on the GPU, an (n, 16) uint8 array; bytes(row).hex() is the usual
    string. flags: MD5_UPPER folds a-z to A-Z first."""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    out = np.zeros((n, 16), np.uint8)
    _check(load().kma_sequence_md5(residues.ctypes.data if len(residues) else None,
                                   offsets.ctypes.data, n, flags, device,
                                   out.ctypes.data if n else None))
    return out


def sequence_md5_device(d_residues: int, d_offsets: int, n_seq: int, n_residues: int,
                        d_digest: int, flags: int = 0, device: int = 0, stream: int = 0,
                        form: int | None = None, waves_per_cu: int = 0):
    """kma_sequence_md5_device (asynchronous on `stream`, one kernel): device pointers, the
    layout and padding of annotate_proteins_device; d_digest gets 16 bytes per sequence. form
    (MD5_STATIC | MD5_COOP; measurements only) goes through the library's measurement hook."""
    if form is None:
        _check(load().kma_sequence_md5_device(device, d_residues or None, d_offsets or None,
                                              n_seq, n_residues, flags, d_digest or None,
                                              stream or None))
    else:
        _check(load().kma_debug_sequence_md5_device(device, d_residues or None,
                                                    d_offsets or None, n_seq, n_residues, flags,
                                                    d_digest or None, stream or None, form,
                                                    waves_per_cu))


def check_sequences(residues, offsets, fun=None, flags: int = 0, device: int = 0,
                    digests: bool = False):
    """kma_check_sequences (SequenceCheckProcessor.java:92-133 on the GPU): returns (rep, size,
    mixed, stats[3] = groups, groups of more than one member, mixed groups[, digests]). rep[s]
    = the first sequence equal to s (-1 for an empty one), size[s] its group's members, mixed[s]
    = 1 iff that group holds more than one member and more than one of the function ids fun."""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    if fun is not None:
        fun = np.ascontiguousarray(fun, np.uint32)
        if len(fun) != n:
            raise KmerAnnoError(E_INVALID, "one function id per sequence")
    rep, size = np.zeros(n, np.int32), np.zeros(n, np.uint32)
    mixed, stats = np.zeros(n, np.uint8), np.zeros(3, np.uint64)
    dig = np.zeros((n, 16), np.uint8) if digests else None
    _check(load().kma_check_sequences(residues.ctypes.data if len(residues) else None,
                                      offsets.ctypes.data, n, flags,
                                      fun.ctypes.data if fun is not None and n else None, device,
                                      dig.ctypes.data if digests and n else None,
                                      rep.ctypes.data if n else None,
                                      size.ctypes.data if n else None,
                                      mixed.ctypes.data if n else None, stats.ctypes.data))
    return (rep, size, mixed, stats, dig) if digests else (rep, size, mixed, stats)


def hash_annotate(genome_residues, genome_offsets, proto_residues, proto_offsets, k: int = 8,
                  min_sim: float = 0.0125, device: int = 0):
    """HashAnnotationProcessor.java:233-306 scoring on the GPU: (best prototype per genome
    protein or -1, its similarity (0.0 if none), matches per prototype)."""
    gr = np.ascontiguousarray(genome_residues, np.uint8)
    go = np.ascontiguousarray(genome_offsets, np.uint64)
    pr = np.ascontiguousarray(proto_residues, np.uint8)
    po = np.ascontiguousarray(proto_offsets, np.uint64)
    n_g, n_p = len(go) - 1, len(po) - 1
    best = np.empty(max(n_g, 1), np.int32)
    sim = np.empty(max(n_g, 1), np.float64)
    cnt = np.empty(max(n_p, 1), np.uint32)
    _check(load().kma_hash_annotate(gr if len(gr) else np.zeros(1, np.uint8), go, n_g,
                                    pr if len(pr) else np.zeros(1, np.uint8), po, n_p, k,
                                    min_sim, device, best.ctypes.data, sim.ctypes.data,
                                    cnt.ctypes.data))
    return best[:n_g], sim[:n_g], cnt[:n_p]


class ProtoIndex:
    """kma_proto_index: the prototypes of a role annotation file resident on one GPU (their
    sorted unique K-mer keys, postings and set sizes), built once and scored against genome
    after genome with hash_annotate_indexed. Read-only after creation; a context manager."""

    def __init__(self, proto_residues, proto_offsets, k: int = 8, device: int = 0):
        pr = np.ascontiguousarray(proto_residues, np.uint8)
        po = np.ascontiguousarray(proto_offsets, np.uint64)
        self._h = _vp()
        if not len(pr):
            pr = np.zeros(1, np.uint8)
        _check(load().kma_proto_index_create(pr.ctypes.data,
                                             po.ctypes.data, len(po) - 1, k, device,
                                             C.byref(self._h)))

    @classmethod
    def from_strings(cls, proteins, k: int = 8, device: int = 0):
        return cls(*pack_strings(proteins), k=k, device=device)

    @property
    def handle(self):
        if not self._h:
            raise KmerAnnoError(E_INVALID, "the prototype index is closed")
        return self._h

    def info(self) -> ProtoIndexInfo:
        out = ProtoIndexInfo()
        _check(load().kma_proto_index_info(self.handle, C.byref(out)))
        return out

    def close(self):
        if self._h:
            load().kma_proto_index_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hash_annotate_indexed(index: ProtoIndex, genome_residues, genome_offsets,
                          min_sim: float = 0.0125, stats: bool = False):
    """kma_hash_annotate_indexed: hash_annotate's three results for one genome against a
    resident ProtoIndex (its K and device); with stats, also [proteins with a candidate,
    proteins scored in more than one prototype range, ranges scored]."""
    gr = np.ascontiguousarray(genome_residues, np.uint8)
    go = np.ascontiguousarray(genome_offsets, np.uint64)
    n_g, n_p = len(go) - 1, index.info().n_proto
    best = np.empty(max(n_g, 1), np.int32)
    sim = np.empty(max(n_g, 1), np.float64)
    cnt = np.empty(max(n_p, 1), np.uint32)
    st = np.zeros(3, np.uint64)
    if not len(gr):
        gr = np.zeros(1, np.uint8)
    _check(load().kma_hash_annotate_indexed(index.handle, gr.ctypes.data,
                                            go.ctypes.data, n_g, min_sim, best.ctypes.data,
                                            sim.ctypes.data, cnt.ctypes.data, st.ctypes.data))
    out = (best[:n_g], sim[:n_g], cnt[:n_p])
    return out + (st,) if stats else out


def hash_scratch_bytes(n_residues: int, n_genome: int) -> int:
    """kma_hash_scratch_bytes: the device scratch hash_annotate_indexed_device needs for a batch
    of n_genome proteins and n_residues residues (a host function, monotone in both)."""
    return int(load().kma_hash_scratch_bytes(n_residues, n_genome))


def hash_annotate_indexed_device(index: ProtoIndex, d_residues: int, d_offsets: int,
                                 n_genome: int, n_residues: int, d_scratch: int,
                                 scratch_bytes: int, d_best: int, d_sim: int, d_count: int,
                                 d_stats: int, min_sim: float = 0.0125, stream: int = 0):
    """kma_hash_annotate_indexed_device (asynchronous on `stream`: memsets and two kernels, no
    allocation, no copy): hash_annotate_indexed for a genome already on the index's device, in
    the layout and padding of annotate_proteins_device. Integer device pointers; d_best int32
    and d_sim float64 per protein, d_count uint32 per prototype, d_stats 4 uint64 (the host
    entry's three, then nonzero iff a window holds a byte outside the alphabet)."""
    _check(load().kma_hash_annotate_indexed_device(
        index.handle, d_residues or None, d_offsets or None, n_genome, n_residues, min_sim,
        d_scratch or None, scratch_bytes, d_best or None, d_sim or None, d_count or None,
        d_stats or None, stream or None))


def build_signatures(residues: np.ndarray, offsets: np.ndarray, roles, k: int = 8,
                     flags: int = 0, device: int = 0):
    """BuildKmerProcessor's discriminating kmers on the GPU: (packed keys, roles), key order."""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    roles = np.ascontiguousarray(roles, np.int32)
    n = len(offsets) - 1
    cap = 1 << 16
    while True:
        keys, rl, nout = np.empty(cap, np.uint64), np.empty(cap, np.uint32), _u64()
        rc = load().kma_build_signatures(residues, offsets, roles, n, k, flags, device,
                                         keys.ctypes.data, rl.ctypes.data, cap, C.byref(nout))
        if rc == E_CAPACITY:
            cap = nout.value
            continue
        _check(rc)
        return keys[:nout.value], rl[:nout.value]


class SigBuilder:
    """kma_sig_builder: build_signatures for a training set fed batch by batch. Every add folds
    its proteins into the rows resident on the GPU (one per distinct kmer, with its state);
    finish() returns what build_signatures returns for the concatenation of the adds, whatever
    the split into adds and their order. A context manager; one thread at a time."""

    def __init__(self, k: int = 8, flags: int = 0, device: int = 0):
        self._h = _vp()
        _check(load().kma_sig_builder_create(k, flags, device, C.byref(self._h)))

    @property
    def handle(self):
        if not self._h:
            raise KmerAnnoError(E_INVALID, "the signature builder is closed")
        return self._h

    def add(self, residues, offsets, roles):
        """One batch: roles[s] >= 0 the single good role of an interesting peg, -1 a buffered
        protein, any other negative value a skipped one. All-or-nothing."""
        residues = np.ascontiguousarray(residues, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        roles = np.ascontiguousarray(roles, np.int32)
        n = len(offsets) - 1
        if len(roles) != n:
            raise KmerAnnoError(E_INVALID, f"{len(roles)} roles for {n} proteins")
        if not len(residues):
            residues = np.zeros(1, np.uint8)
        if not len(roles):
            roles = np.zeros(1, np.int32)
        _check(load().kma_sig_builder_add(self.handle, residues.ctypes.data, offsets.ctypes.data,
                                          roles.ctypes.data, n))

    def info(self) -> SigBuilderInfo:
        out = SigBuilderInfo()
        _check(load().kma_sig_builder_info_get(self.handle, C.byref(out)))
        return out

    def finish(self):
        """(packed keys, roles) of the discriminating kmers so far, key order; the builder is
        left as it is."""
        n = int(self.info().n_role)
        keys, rl, nout = np.empty(n, np.uint64), np.empty(n, np.uint32), _u64()
        _check(load().kma_sig_builder_finish(self.handle, keys.ctypes.data, rl.ctypes.data, n,
                                             C.byref(nout)))
        assert nout.value == n
        return keys, rl

    def close(self):
        if self._h:
            load().kma_sig_builder_destroy(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def contig_window_count(offsets: np.ndarray, k: int = 8) -> int:
    offsets = np.ascontiguousarray(offsets, np.uint64)
    return int(load().kma_contig_window_count(offsets, len(offsets) - 1, k))


def protein_distances(residues, offsets, pair_a, pair_b, k: int = 8, flags: int = 0,
                      device: int = 0):
    """ProteinKmers.distance per pair (GeneCopyProcessor.java:137-142) on the GPU:
    (similarity, per-protein set sizes, distances)."""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    pa = np.ascontiguousarray(pair_a, np.uint32)
    pb = np.ascontiguousarray(pair_b, np.uint32)
    n = len(offsets) - 1
    sim = np.empty(len(pa), np.uint32)
    size = np.empty(n, np.uint32)
    dist = np.empty(len(pa), np.float64)
    _check(load().kma_protein_distances(residues, offsets, n, k, flags, pa, pb, len(pa), device,
                                        sim, size.ctypes.data, dist.ctypes.data))
    return sim, size, dist


def protein_best_match(residues, offsets, query, cand_off, cand, max_dist: float, k: int = 8,
                       flags: int = 0, device: int = 0):
    """GeneCopyProcessor's closest-source choice (:135-146): (best index or -1, distance)."""
    residues = np.ascontiguousarray(residues, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    query = np.ascontiguousarray(query, np.uint32)
    cand_off = np.ascontiguousarray(cand_off, np.uint64)
    cand = np.ascontiguousarray(cand, np.uint32)
    best = np.empty(len(query), np.int32)
    bd = np.empty(len(query), np.float64)
    _check(load().kma_protein_best_match(residues, offsets, len(offsets) - 1, k, flags, query,
                                         cand_off, cand if len(cand) else np.zeros(1, np.uint32),
                                         len(query), max_dist, device, best, bd.ctypes.data))
    return best, bd

