"""ctypes binding of libstrainscan_hip.so (the C ABI declared in include/strainscan_hip.h).

Fails loudly: a missing library is an ImportError-like RuntimeError, a missing GPU surfaces as
SSError(SS_ENODEV) from the first call that needs the device.  Nothing here falls back to a CPU
implementation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SS_LIB") or os.path.join(_HERE, "lib", "libstrainscan_hip.so")

SS_OK, SS_EINVAL, SS_ENOMEM, SS_EIO, SS_EHIP, SS_ENODEV, SS_EKEY, SS_ERANGE = 0, -22, -12, -5, -1000, -19, -2, -34
SS_EAGAIN = -11
GZ_CHAIN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p)      # ss_gz_chain_fn (strainscan_hip.h)
NO_CHAIN = C.cast(None, GZ_CHAIN_FN)
ROW_VALID, ROW_LOWER = 1, 2


def cli_clock(what):
    """SS_CLI_TRACE=1: seconds since the interpreter started, at the milestones of a run (stderr).  scripts/bench_cli_l2.py
    reads these lines to say where a fresh `strainscan` process spends its time."""
    if os.environ.get("SS_CLI_TRACE"):
        import sys
        import time
        try:
            import psutil
            t0 = psutil.Process().create_time()
        except Exception:                   # noqa: B902
            t0 = time.time()
        sys.stderr.write("[cli] %-44s %.3f s after process start\n" % (what, time.time() - t0))


class SSError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        lib = _lib
        msg = lib.ss_strerror(code).decode() if lib is not None else str(code)
        if code == SS_EHIP and lib is not None:
            msg += ": " + lib.ss_last_error().decode()
        super().__init__("%s failed: %s (%d)" % (where, msg, code))


class NodeStat(C.Structure):
    _fields_ = [("length", C.c_uint32), ("n_pos", C.c_uint32), ("n_kept", C.c_uint32), ("reserved", C.c_uint32),
                ("sum_kept", C.c_uint64), ("median2", C.c_uint64)]


NODE_STAT_DTYPE = np.dtype([("length", "<u4"), ("n_pos", "<u4"), ("n_kept", "<u4"), ("reserved", "<u4"),
                            ("sum_kept", "<u8"), ("median2", "<u8")])

_lib = None

u64, u32, i32, vp, cp = C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_char_p
P = C.POINTER

# name -> (restype, argtypes); kept in one table so tests can check it against the header
SIGNATURES = {
    "ss_version": (i32, []),
    "ss_strerror": (cp, [i32]),
    "ss_last_error": (cp, []),
    "ss_device_count": (i32, [P(i32)]),
    "ss_set_device": (i32, [i32]),
    "ss_device_sync": (i32, []),
    "ss_stream_sync": (i32, [vp]),
    "ss_dev_alloc": (i32, [P(vp), u64]),
    "ss_dev_alloc_async": (i32, [P(vp), u64]),
    "ss_dev_free_async": (i32, [vp]),
    "ss_dev_free": (i32, [vp]),
    "ss_memcpy_h2d": (i32, [vp, vp, u64, vp]),
    "ss_memcpy_d2h": (i32, [vp, vp, u64, vp]),
    "ss_memset_dev": (i32, [vp, i32, u64, vp]),
    "ss_revcomp": (i32, [cp, cp, u64]),
    "ss_shuffle_split_bits": (i32, [u64, i32, u64, u32, vp]),
    "ss_gz_inflate": (i32, [cp, i32, i32, P(vp), P(u64)]),
    "ss_gz_inflate_gpu": (i32, [cp, P(vp), P(u64)]),
    "ss_gz_gpu_counters": (i32, [P(u64), P(u64)]),
    "ss_gz_gpu_release": (i32, []),
    "ss_dev_big_blocks": (i32, [P(u64)]),
    "ss_dev_big_release": (i32, []),
    "ss_gz_set_policy": (i32, [i32]),
    "ss_gz_set_range": (i32, [i32, i32, u64, GZ_CHAIN_FN, vp]),
    "ss_gz_range_counters": (i32, [P(u64), P(u64)]),
    "ss_test_hook": (i32, [i32, C.c_longlong]),
    "ss_gz_free": (None, [vp]),
    "ss_gz_inflate_to_file": (i32, [cp, cp, i32, P(u64)]),
    "ss_host_cpus": (i32, []),
    "ss_revcomp_dev": (i32, [vp, vp, u64, u64, vp]),
    "ss_kmerfa_count_rows": (i32, [cp, P(u64)]),
    "ss_node_lists_parse": (i32, [cp, vp, C.c_uint32, u64, vp, vp, vp, P(C.c_uint32)]),
    "ss_kmerfa_encode": (i32, [cp, i32, u64, vp, vp, i32]),
    "ss_kmerfa_encode_mem": (i32, [cp, u64, i32, u64, vp, vp]),
    "ss_encode_kmer": (i32, [cp, i32, P(u64)]),
    "ss_db_build": (i32, [vp, vp, u64, i32, i32, P(vp)]),
    "ss_db_destroy": (i32, [vp]),
    "ss_db_export": (i32, [vp, cp]),
    "ss_db_import": (i32, [cp, P(vp)]),
    "ss_db_info": (i32, [vp, P(u64), P(u64), P(u64), P(i32)]),
    "ss_db_row_valid": (i32, [vp, vp]),
    "ss_db_row_valid_dev": (vp, [vp]),
    "ss_db_device_bytes": (u64, [vp]),
    "ss_db_index_info": (i32, [vp, vp]),
    "ss_db_expect_hits": (i32, [vp, i32]),
    "ss_db_probe_info": (i32, [vp, vp]),
    "ss_scan_reads_multi": (i32, [vp, i32, vp, vp]),
    "ss_scan_multi_launches": (i32, [P(u64)]),
    "ss_reads_support": (i32, [vp, vp, u32, vp, P(u64)]),
    "ss_reads_support_calls": (i32, [P(u64)]),
    "ss_reads_select": (i32, [vp, vp, u32, P(vp)]),
    "ss_reads_select_calls": (i32, [P(u64)]),
    "ss_reads_support_labeled": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
    "ss_reads_select_labeled": (i32, [vp, vp, vp, u32, u32, u32, P(vp)]),
    "ss_reads_labeled_calls": (i32, [P(u64)]),
    "ss_reads_resample": (i32, [vp, u64, u32, P(vp)]),
    "ss_reads_resample_calls": (i32, [P(u64)]),
    "ss_scan_reads_resampled": (i32, [vp, vp, u64, u32, u32, vp]),
    "ss_scan_reads_resampled_calls": (i32, [P(u64)]),
    "ss_reads_classify": (i32, [vp, vp, vp, u32, vp, u32, vp, vp, vp, vp]),
    "ss_reads_classify_calls": (i32, [P(u64)]),
    "ss_reads_classify_ties": (i32, [P(u64)]),
    "ss_reads_select_class": (i32, [vp, vp, vp, u32, vp, u32, vp, u32, P(vp), vp, vp, vp]),
    "ss_reads_select_class_calls": (i32, [P(u64)]),
    "ss_reads_classify_strains": (i32, [vp, vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, vp]),
    "ss_reads_classify_strains_calls": (i32, [P(u64)]),
    "ss_reads_classify_strains_ties": (i32, [P(u64)]),
    "ss_reads_select_strains": (i32, [vp, vp, vp, u32, u32, vp, vp, u32, P(vp), vp, vp, vp, vp]),
    "ss_reads_select_strains_calls": (i32, [P(u64)]),
    "ss_reads_strain_sets_resampled": (i32, [vp, vp, vp, u32, u32, u64, u32, u32, vp]),
    "ss_reads_strain_sets_resampled_calls": (i32, [P(u64)]),
    "ss_em_strain_sets": (i32, [vp, vp, u32, u32, u32, u32, C.c_double, vp, vp]),
    "ss_em_strain_sets_calls": (i32, [P(u64)]),
    "ss_reads_gaps": (i32, [vp, vp, vp, u32, vp, vp]),
    "ss_reads_gaps_calls": (i32, [P(u64)]),
    "ss_reads_order": (i32, [vp]),
    "ss_flat_record_keys": (i32, [cp, u64, vp, u64, P(u64)]),
    "ss_extract_write": (i32, [P(cp), i32, vp, u64, P(cp), P(u64)]),
    "ss_extract_write_pairs": (i32, [P(cp), i32, vp, u64, P(cp), P(u64)]),
    "ss_reads_join_pairs_dev": (i32, [vp, u64, vp, u64, i32, P(vp)]),
    "ss_reads_join_pairs_calls": (i32, [P(u64)]),
    "ss_reads_load_pairs": (i32, [cp, cp, i32, P(vp)]),
    "ss_reads_calls": (i32, [vp, vp, vp, u32, vp, u32, vp, vp, vp, vp, vp, u64, P(u64), vp, vp, vp]),
    "ss_reads_calls_calls": (i32, [P(u64)]),
    "ss_reads_load_ordered": (i32, [cp, P(vp)]),
    "ss_read_calls_write": (i32, [P(cp), i32, P(cp), u64, vp, vp, vp, vp, vp, vp, u32, P(u64)]),
    "ss_scan_reset": (i32, [vp, vp]),
    "ss_scan_flat_dev": (i32, [vp, vp, u64, vp]),
    "ss_scan_flat_host": (i32, [vp, cp, u64]),
    "ss_scan_files": (i32, [vp, P(cp), i32, P(u64), P(u64)]),
    "ss_scan_files_shard": (i32, [vp, P(cp), i32, i32, i32, P(u64), P(u64)]),
    "ss_counts_rows_dev": (i32, [vp, vp, vp]),
    "ss_counts_rows": (i32, [vp, vp]),
    "ss_counts_load_rows_dev": (i32, [vp, vp, vp]),
    "ss_scan_kernel_launches": (u64, [vp]),
    "ss_ingest_warm_up": (i32, []),
    "ss_ingest_threads": (i32, [P(i32)]),
    "ss_gz_warm_up": (i32, [i32]),
    "ss_reads_load": (i32, [P(cp), i32, i32, i32, P(vp)]),
    "ss_reads_from_flat_dev": (i32, [vp, u64, i32, P(vp)]),
    "ss_reads_read_back": (i32, [vp, vp, u64, P(u64)]),
    "ss_reads_destroy": (i32, [vp]),
    "ss_reads_info": (i32, [vp, P(u64), P(u64), P(u64), P(u64)]),
    "ss_scan_reads": (i32, [vp, vp, vp]),
    "ss_reads_order_timing": (i32, [vp]),
    "ss_reads_order_counters": (i32, [P(u64)]),
    "ss_reads_packed_slabs": (i32, [vp, P(u64)]),
    "ss_fastx_to_flat": (i32, [cp, u64, vp, P(u64), P(u64)]),
    "ss_input_kind": (i32, [cp, P(i32)]),
    "ss_bam_decode": (i32, [vp, u64, i32, i32, vp, u64, P(u64), P(u64)]),
    "ss_bam_counters": (i32, [P(u64)]),
    "ss_bam_select": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, u64, P(u64), P(u64)]),
    "ss_bam_extract": (i32, [cp, vp, vp, u32, u32, u32, cp, P(u64)]),
    "ss_bgzf_write": (i32, [cp, vp, u64, vp, u64, i32]),
    "ss_bam_extract_calls": (i32, [P(u64)]),
    "ss_bam_extract_timing": (i32, [P(C.c_double)]),
    "ss_bam_mates": (i32, [vp, u64, vp, u64, P(u64)]),
    "ss_reads_join_pairs_bam": (i32, [vp, u64, i32, P(vp), P(u64)]),
    "ss_reads_load_pairs_bam": (i32, [cp, i32, P(vp), P(u64)]),
    "ss_bam_select_pairs": (i32, [vp, u64, vp, vp, u32, u32, u32, vp, u64, P(u64), P(u64)]),
    "ss_bam_extract_pairs": (i32, [cp, vp, vp, u32, u32, u32, cp, P(u64)]),
    "ss_bam_pairs_timing": (i32, [P(C.c_double)]),
    "ss_bam_tag_stream": (i32, [vp, u64, vp, vp, u32, vp, u32, vp, cp, i32, vp, u64, P(u64), P(u64), vp, vp, vp]),
    "ss_bam_tag_file": (i32, [cp, vp, vp, u32, vp, u32, vp, cp, i32, cp, P(u64), vp, vp, vp]),
    "ss_bam_tag_calls": (i32, [P(u64)]),
    "ss_bam_tag_timing": (i32, [P(C.c_double)]),
    "ss_set_min_base_qual": (i32, [i32]),
    "ss_get_min_base_qual": (i32, []),
    "ss_mask_counters": (i32, [P(u64)]),
    "ss_reader_open": (i32, [P(cp), i32, P(vp)]),
    "ss_reader_set_overlap": (i32, [vp, i32]),
    "ss_reader_next": (i32, [vp, vp, u64, P(u64), P(u64)]),
    "ss_reader_close": (i32, [vp]),
    "ss_nodes_create": (i32, [vp, vp, u32, P(vp)]),
    "ss_nodes_destroy": (i32, [vp]),
    "ss_nodes_reduce_dev": (i32, [vp, vp, vp, vp, vp]),
    "ss_nodes_reduce": (i32, [vp, vp, vp]),
    "ss_nodes_bind": (i32, [vp, vp]),
    "ss_nodes_harvest_dev": (i32, [vp, vp, vp]),
    "ss_nodes_reduce_touched_dev": (i32, [vp, vp, vp]),
    "ss_nodes_touched_get_dev": (i32, [vp, vp, vp]),
    "ss_nodes_touched_set_dev": (i32, [vp, vp, vp]),
    "ss_nodes_pack_dev": (i32, [vp, vp, u64, P(u64), vp]),
    "ss_nodes_unpack_dev": (i32, [vp, vp, vp]),
    "ss_nodes_pack_capped_dev": (i32, [vp, vp, u64, vp, vp]),
    "ss_nodes_unpack_capped_dev": (i32, [vp, vp, u64, vp]),
    "ss_nodes_clear_dev": (i32, [vp, vp]),
    "ss_rows_reduce": (i32, [vp, vp, u64, P(NodeStat)]),
    "ss_l2_create": (i32, [vp, vp, u64, u32, P(vp)]),
    "ss_l2_create_dev": (i32, [vp, vp, u64, u32, P(vp)]),
    "ss_npz_member_dev": (i32, [C.c_char_p, u64, u64, C.c_uint32, u64, i32, P(vp), P(u64), P(vp)]),
    "ss_npz_member_done": (i32, [vp]),
    "ss_crc32_repeat": (i32, [C.c_uint32, i32, u64, P(C.c_uint32)]),
    "ss_l2_create_planes": (i32, [vp, u64, u32, P(vp)]),
    "ss_l2_export_planes": (i32, [vp, vp]),
    "ss_l2_destroy": (i32, [vp]),
    "ss_l2_info": (i32, [vp, P(u64), P(u32), P(u64)]),
    "ss_l2_popc2": (i32, [vp, vp, vp, vp, vp]),
    "ss_l2_andnot_col": (i32, [vp, u32, vp]),
    "ss_l2_set_overlap": (i32, [vp, vp, vp, vp, u32]),
    "ss_l2_prepare": (i32, [vp, vp, vp, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp]),
    "ss_l2_import": (i32, [C.c_char_p, u64, C.c_uint32, u64, u64, u64, u64, u64, C.c_uint32, vp]),
    "ss_l2_fold": (i32, [vp, vp, vp, u64, vp]),
    "ss_l2_fold_train": (i32, [vp, vp, vp, u64, i32, vp]),
    "ss_split_dev_start": (i32, [u64, i32, u64, C.c_uint32, vp]),
    "ss_split_dev_wait": (i32, [vp, vp, vp]),
    "ss_split_dev_free": (i32, [vp]),
    "ss_l2_count_keep": (i32, [vp, u64, C.c_double, C.c_double, C.c_double, vp]),
    "ss_l2_quantile_sums": (i32, [vp, vp, vp, u32, C.c_double, C.c_double, vp, vp, vp, vp, vp]),
    "ss_l2_pattern_stats": (i32, [vp, vp, i32, vp, vp, i32, vp]),
    "ss_enet_path_gram": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, i32, C.c_double, i32, C.c_double, i32, vp, vp,
                                vp, vp, vp]),
    "ss_enet_cd": (i32, [vp, vp, u64, i32, C.c_double, C.c_double, i32, C.c_double, i32, vp, vp, vp]),
}


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (same soname as
    /opt/rocm's); whichever is loaded first serves both.  If this library were loaded first it
    would pull /opt/rocm's runtime and a later `import torch` (multi-GPU plumbing, bench.py)
    then fails with "No HIP GPUs are available".  So when torch is installed, map ITS runtime
    first; without torch the RUNPATH of libstrainscan_hip.so finds /opt/rocm's."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


_LIB_LOCK = __import__("threading").Lock()


def lib():
    """The loaded library; raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _LIB_LOCK:
        return _load()


def warm_up(ingest=False, gz=0):
    """Load the library and start the HIP runtime (0.1-0.2 s in a fresh process); `ingest`: also the one-time costs of the
    first read of plain-text files (pinned parse buffers, streams: another 0.1 s); `gz`: the pinned upload buffers of that
    many .gz inputs -- the CLI calls this on a worker thread while the interpreter is still importing modules and parsing
    arguments."""
    try:
        if device_count() > 0 and ingest:
            lib().ss_ingest_warm_up()
        if device_count() > 0 and gz:
            lib().ss_gz_warm_up(int(gz))

    except Exception:                       # noqa: B902 -- whoever needs the GPU next gets the real error
        pass


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "strainscan_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C strainscan_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here = library older than the binding
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, where):
    if rc != SS_OK:
        if rc == SS_EKEY:
            raise KeyError("%s: a database k-mer has no owning row (identify_low_mem.py:88)" % where)
        raise SSError(rc, where)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class gz_policy:
    """with gz_policy(1): ...  -- who inflates .gz inputs inside the block (ss_gz_set_policy: 1 = the device or SS_EAGAIN,
    2 = the host inflaters); back to 0 (device, then host for what it declines) afterwards."""

    def __init__(self, mode):
        self.mode = int(mode)

    def __enter__(self):
        check(lib().ss_gz_set_policy(self.mode), "ss_gz_set_policy")
        return self

    def __exit__(self, *exc):
        lib().ss_gz_set_policy(0)
        return False


def device_count():
    n = C.c_int(0)
    rc = lib().ss_device_count(C.byref(n))
    return n.value if rc == SS_OK else 0


def require_gpu():
    if device_count() < 1:
        raise SSError(SS_ENODEV, "strainscan_amd (no MI355X visible; there is no CPU fallback)")


# -------------------------------------------------------------------------------------------------
class KmerDB:
    """Device k-mer table built from a k-mer FASTA (`--if` argument of the reference's jellyfish
    calls, library/identify.py:82-86) with per-row bookkeeping of identify.py:90-101."""

    def __init__(self, keys, flags, k=31, upper_keys=True):
        require_gpu()
        keys = np.ascontiguousarray(keys, np.uint64)
        flags = np.ascontiguousarray(flags, np.uint8)
        assert keys.shape == flags.shape
        h = C.c_void_p()
        check(lib().ss_db_build(ptr(keys), ptr(flags), keys.size, int(k), int(upper_keys), C.byref(h)),
              "ss_db_build")
        self._h = h
        self.k = int(k)
        self.n_rows = int(keys.size)
        self._row_valid = None

    @classmethod
    def from_image(cls, path):
        """A previously exported index image (ss_db_export); raises SSError if it is not usable."""
        require_gpu()
        h = C.c_void_p()
        check(lib().ss_db_import(os.fsencode(path), C.byref(h)), "ss_db_import(%s)" % path)
        self = cls.__new__(cls)
        self._h = h
        self._row_valid = None
        i = self.info()
        self.k, self.n_rows = i["k"], i["n_rows"]
        return self

    def export(self, path):
        check(lib().ss_db_export(self._h, os.fsencode(path)), "ss_db_export(%s)" % path)

    @classmethod
    def from_fasta(cls, path, k=31, upper_keys=True, threads=0):
        n = C.c_uint64()
        check(lib().ss_kmerfa_count_rows(os.fsencode(path), C.byref(n)), "ss_kmerfa_count_rows(%s)" % path)
        keys = np.empty(n.value, np.uint64)
        flags = np.empty(n.value, np.uint8)
        check(lib().ss_kmerfa_encode(os.fsencode(path), int(k), n.value, ptr(keys), ptr(flags), threads),
              "ss_kmerfa_encode(%s)" % path)
        return cls(keys, flags, k, upper_keys)

    @classmethod
    def from_text(cls, text, k=31, upper_keys=True):
        keys, flags = encode_kmer_fasta(text, k)
        return cls(keys, flags, k, upper_keys)

    def close(self):
        if getattr(self, "_h", None):
            lib().ss_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def info(self):
        a, b, c, k = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib().ss_db_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(k)), "ss_db_info")
        ix = np.zeros(8, np.uint64)
        check(lib().ss_db_index_info(self._h, ptr(ix)), "ss_db_index_info")
        return dict(n_rows=a.value, n_distinct=b.value, capacity=c.value, k=k.value,
                    device_bytes=int(lib().ss_db_device_bytes(self._h)), layout=int(ix[0]), n_slots=int(ix[1]),
                    n_buckets=int(ix[2]), n_dir=int(ix[3]), filter_bits=int(ix[4]), n_mslots=int(ix[6]), n_inline=int(ix[7]))

    @property
    def row_valid(self):
        if self._row_valid is None:
            v = np.zeros(self.n_rows, np.uint8)
            check(lib().ss_db_row_valid(self._h, ptr(v)), "ss_db_row_valid")
            self._row_valid = v
        return self._row_valid

    @property
    def row_valid_dev(self):
        return lib().ss_db_row_valid_dev(self._h)

    def expect_hits(self, expect=True):
        """Hint: most read k-mers are in this table (a layer-2 cluster table)."""
        check(lib().ss_db_expect_hits(self._h, 1 if expect else 0), "ss_db_expect_hits")
        return self

    def probe_info(self):
        """What the last binned scan's probe found for this table: dict(set, comb, runs_per_tile)."""
        out = np.zeros(3, np.uint64)
        check(lib().ss_db_probe_info(self._h, ptr(out)), "ss_db_probe_info")
        return dict(set=int(out[0]), comb=bool(out[1]), runs_per_tile=float(out[2]) / 1000.0)

    def reset(self, stream=None):
        check(lib().ss_scan_reset(self._h, stream), "ss_scan_reset")

    def scan_flat_dev(self, dptr, n, stream=None):
        check(lib().ss_scan_flat_dev(self._h, dptr, int(n), stream), "ss_scan_flat_dev")

    def scan_flat(self, bases):
        b = bytes(bases) if not isinstance(bases, bytes) else bases
        check(lib().ss_scan_flat_host(self._h, b, len(b)), "ss_scan_flat_host")

    def scan_files(self, paths, shard_rank=0, shard_world=1):
        """Count in the reads of the files; with shard_world > 1 only this rank's share of them (parsed, copied, scanned)."""
        paths = [os.fsencode(p) for p in paths if p]
        arr = (C.c_char_p * len(paths))(*paths)
        nrec, nb = C.c_uint64(), C.c_uint64()
        check(lib().ss_scan_files_shard(self._h, arr, len(paths), int(shard_rank), int(shard_world), C.byref(nrec), C.byref(nb)),
              "ss_scan_files_shard")
        return nrec.value, nb.value

    def counts_rows(self):
        out = np.zeros(self.n_rows, np.uint32)
        check(lib().ss_counts_rows(self._h, ptr(out)), "ss_counts_rows")
        return out

    def load_counts_rows_dev(self, dptr, stream=None):
        check(lib().ss_counts_load_rows_dev(self._h, dptr, stream), "ss_counts_load_rows_dev")

    def counts_rows_dev(self, dptr, stream=None):
        check(lib().ss_counts_rows_dev(self._h, dptr, stream), "ss_counts_rows_dev")


class ReadSet:
    """FASTA/FASTQ(.gz) files parsed once and kept in HBM as flat base blocks."""

    def __init__(self, paths, shard_rank=0, shard_world=1):
        require_gpu()
        ps = [os.fsencode(p) for p in paths if p]
        arr = (C.c_char_p * len(ps))(*ps)
        h = C.c_void_p()
        check(lib().ss_reads_load(arr, len(ps), int(shard_rank), int(shard_world), C.byref(h)), "ss_reads_load")
        self._h = h

    @classmethod
    def from_flat_dev(cls, dptr, n, order=True):
        """A resident read set from a flat base block already on the device (copied; `order`: locality order)."""
        require_gpu()
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().ss_reads_from_flat_dev(dptr, int(n), int(bool(order)), C.byref(h)), "ss_reads_from_flat_dev")
        self._h = h
        return self

    @classmethod
    def join_pairs_dev(cls, dptr1, n1, dptr2, n2, order=True):
        """A resident set whose records are the PAIRS of two flat base blocks on the device: record i is line i of block 1,
        'N', line i of block 2 (ss_reads_join_pairs_dev; tests/pairs_model.py restates it).  order=False: in line order."""
        require_gpu()
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().ss_reads_join_pairs_dev(dptr1, int(n1), dptr2, int(n2), int(bool(order)), C.byref(h)), "ss_reads_join_pairs_dev")
        self._h = h
        return self

    @classmethod
    def load_pairs(cls, p1, p2, order=True):
        """The same set from the two files of a paired sample, each read in file order (ss_reads_load_pairs)."""
        require_gpu()
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().ss_reads_load_pairs(os.fsencode(p1), os.fsencode(p2), int(bool(order)), C.byref(h)), "ss_reads_load_pairs")
        self._h = h
        return self

    @classmethod
    def load_ordered(cls, path):
        """One FASTA/FASTQ file as one ASCII, unbinned slab in FILE ORDER (ss_reads_load_ordered): record i of the set is the i-th
        record of the file that has a sequence.  What `--read_calls` classifies."""
        require_gpu()
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().ss_reads_load_ordered(os.fsencode(path), C.byref(h)), "ss_reads_load_ordered")
        self._h = h
        return self

    @classmethod
    def _pairs_bam(cls, call, where):
        require_gpu()
        self = cls.__new__(cls)
        h, c = C.c_void_p(), (C.c_uint64 * 6)()
        rc = call(C.byref(h), c)
        counters = dict(zip(BAM_PAIR_COUNTERS, (int(v) for v in c)))
        if rc != SS_OK:
            e = SSError(rc, where)
            e.pair_counters = counters      # (SS_EIO with "violating" != 0: names that are not one first and one second mate)
            raise e
        self._h = h
        self.pair_counters = counters
        return self

    @classmethod
    def join_pairs_bam(cls, stream, order=True):
        """A resident set whose records are the FRAGMENTS of an inflated BAM stream (bytes from b'BAM\\1'): mate 1, 'N', mate 2 of
        every pair, orphans and singles with the N alone (ss_reads_join_pairs_bam; tests/bam_pairs_model.py restates the rule).
        .pair_counters: dict(records=, kept=, pairs=, orphans=, singles=, violating=); an SSError carries them too."""
        stream = bytes(stream)
        return cls._pairs_bam(lambda h, c: lib().ss_reads_join_pairs_bam(stream, len(stream), int(bool(order)), h, c), "ss_reads_join_pairs_bam")

    @classmethod
    def load_pairs_bam(cls, path, order=True):
        """The same set from one BAM file (ss_reads_load_pairs_bam)."""
        return cls._pairs_bam(lambda h, c: lib().ss_reads_load_pairs_bam(os.fsencode(path), int(bool(order)), h, c), "ss_reads_load_pairs_bam")

    def close(self):
        if getattr(self, "_h", None):
            lib().ss_reads_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def read_back(self):
        """The resident flat blocks as bytes (tests)."""
        n = C.c_uint64()
        check(lib().ss_reads_read_back(self._h, None, 0, C.byref(n)), "ss_reads_read_back")
        buf = np.zeros(max(1, n.value), np.uint8)
        check(lib().ss_reads_read_back(self._h, ptr(buf), buf.size, C.byref(n)), "ss_reads_read_back")
        return buf[:n.value].tobytes()

    def info(self):
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().ss_reads_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "ss_reads_info")
        return dict(n_records=a.value, n_bases=b.value, n_blocks=c.value, device_bytes=d.value)

    def packed_slabs(self):
        """Slabs of the set held packed (ss_reads_packed_slabs)."""
        n = C.c_uint64()
        check(lib().ss_reads_packed_slabs(self._h, C.byref(n)), "ss_reads_packed_slabs")
        return n.value

    def scan_into_many(self, kdbs, stream=None):
        """One pass over the resident reads for several tables (ss_scan_reads_multi); counts as scan_into on each."""
        arr = (C.c_void_p * len(kdbs))(*[k.handle for k in kdbs])
        check(lib().ss_scan_reads_multi(arr, len(kdbs), self._h, stream), "ss_scan_reads_multi")

    def scan_into(self, kdb, stream=None):
        check(lib().ss_scan_reads(kdb.handle, self._h, stream), "ss_scan_reads")

    def support(self, kdb, n_bins=65):
        """(hist, hits): hist[b] = records of the set with exactly b k-mer hits against `kdb` (the last bin: that many or more),
        np.uint64[n_bins]; hits = the hits of all records (ss_reads_support).  The table's counters are left alone."""
        hist = np.zeros(max(int(n_bins), 1), np.uint64)
        hits = C.c_uint64()
        check(lib().ss_reads_support(kdb.handle, self._h, int(n_bins), ptr(hist), C.byref(hits)), "ss_reads_support")
        return hist, int(hits.value)

    def select(self, kdb, min_hits):
        """A new ReadSet: the records of this one with at least `min_hits` k-mer hits against `kdb` (ss_reads_select), as one
        ASCII, unbinned block in an unspecified order.  The caller closes it.  The table's counters are left alone."""
        h = C.c_void_p()
        check(lib().ss_reads_select(kdb.handle, self._h, int(min_hits), C.byref(h)), "ss_reads_select")
        sub = ReadSet.__new__(ReadSet)
        sub._h = h
        return sub

    def support_labeled(self, kdb, row_labels, n_labels, n_bins=65):
        """support() per label of the table's rows (ss_reads_support_labeled): row_labels[i] in 0..n_labels for row i of the
        table, 0 = counts for nobody.  -> (hist np.uint64[n_labels, n_bins], hits np.uint64[n_labels], kmers np.uint64[n_labels]:
        the distinct k-mers of each label).  Rows that share a k-mer under different labels count for nobody."""
        lab = _row_labels(kdb, row_labels)
        nl = max(int(n_labels), 0)
        hist = np.zeros((max(nl, 1), max(int(n_bins), 1)), np.uint64)
        hits = np.zeros(max(nl, 1), np.uint64)
        kmers = np.zeros(max(nl, 1), np.uint64)
        check(lib().ss_reads_support_labeled(kdb.handle, self._h, ptr(lab), nl, int(n_bins), ptr(hist), ptr(hits), ptr(kmers)),
              "ss_reads_support_labeled")
        return hist, hits, kmers

    def select_labeled(self, kdb, row_labels, n_labels, label, min_hits):
        """select() on the hits of one label (ss_reads_select_labeled): the records with at least `min_hits` hits whose k-mer has
        label `label`, as a new ReadSet.  The caller closes it."""
        lab = _row_labels(kdb, row_labels)
        h = C.c_void_p()
        check(lib().ss_reads_select_labeled(kdb.handle, self._h, ptr(lab), max(int(n_labels), 0), max(int(label), 0), int(min_hits),
                                            C.byref(h)), "ss_reads_select_labeled")
        sub = ReadSet.__new__(ReadSet)
        sub._h = h
        return sub

    def classify(self, kdb, row_node, parent, min_score, want_classes=False):
        """Every record assigned to a node of a tree over the table's k-mers (ss_reads_classify; tests/class_model.py restates it).
        row_node[i] in 0..n for row i of the table (0 = counts for nobody), parent[v] for v in 1..n (entry 0 is not read; 0 = no
        parent), n = len(parent) - 1.  -> dict(direct=, node_hits=, kmers= np.uint64[n + 1], ties= records whose class came from a
        tie, classes= np.uint32 per record in read_back() order, or None).  Rows that share a k-mer under different nodes count
        for nobody.  The table's counters are left alone."""
        rn = np.ascontiguousarray(row_node, np.uint32)
        if rn.ndim != 1 or rn.size != kdb.n_rows:
            raise ValueError("one node per row of the table (%d), not %r" % (kdb.n_rows, rn.shape))
        par = np.ascontiguousarray(parent, np.uint32)
        if par.ndim != 1 or par.size < 1:
            raise ValueError("parent holds an entry per node and entry 0")
        n = par.size - 1
        direct, node_hits, kmers = (np.zeros(n + 1, np.uint64) for _ in range(3))
        # (the records as ss_reads_support counts them: ss_reads_info's count includes reads without a base)
        classes = np.zeros(max(1, int(self.support(kdb, 2)[0].sum())), np.uint32) if want_classes else None
        check(lib().ss_reads_classify(kdb.handle, self._h, ptr(rn if rn.size else np.zeros(1, np.uint32)), n, ptr(par), int(min_score),
                                      ptr(direct), ptr(node_hits), ptr(kmers), ptr(classes) if want_classes else None), "ss_reads_classify")
        ties = C.c_uint64()
        check(lib().ss_reads_classify_ties(C.byref(ties)), "ss_reads_classify_ties")
        if want_classes:
            classes = classes[:int(direct.sum())]
        return dict(direct=direct, node_hits=node_hits, kmers=kmers, ties=int(ties.value), classes=classes)

    def calls(self, kdb, row_node, parent, min_score, cap=None):
        """classify() per record (ss_reads_calls): -> dict(classes=, scores= np.uint32[records], first= np.uint64[records + 1],
        list_node=, list_hits= np.uint32[n_list], direct=, node_hits=, kmers=, ties=).  The hit list of record i -- every node
        v >= 1 the record has hits of, ascending, with the hits -- is entries first[i] .. first[i + 1] - 1 of list_node / list_hits;
        records are numbered in read_back() order.  cap: the list entries to bring room for; None: four per record, and the call
        is made again with the number it names where that was too few (a second classification: tens of milliseconds)."""
        rn = np.ascontiguousarray(row_node, np.uint32)
        if rn.ndim != 1 or rn.size != kdb.n_rows:
            raise ValueError("one node per row of the table (%d), not %r" % (kdb.n_rows, rn.shape))
        par = np.ascontiguousarray(parent, np.uint32)
        if par.ndim != 1 or par.size < 1:
            raise ValueError("parent holds an entry per node and entry 0")
        n = par.size - 1
        room = int(self.info()["n_records"]) + 1           # (ss_reads_info's count includes reads without a base: no fewer)
        direct, node_hits, kmers = (np.zeros(n + 1, np.uint64) for _ in range(3))
        classes, scores, first = np.zeros(room, np.uint32), np.zeros(room, np.uint32), np.zeros(room + 1, np.uint64)
        n_list = C.c_uint64()
        want = 4 * room + 1024 if cap is None else int(cap)
        for _ in range(2):
            list_node, list_hits = np.zeros(max(want, 1), np.uint32), np.zeros(max(want, 1), np.uint32)
            rc = lib().ss_reads_calls(kdb.handle, self._h, ptr(rn if rn.size else np.zeros(1, np.uint32)), n, ptr(par), int(min_score),
                                      ptr(classes), ptr(scores), ptr(first), ptr(list_node) if want else None,
                                      ptr(list_hits) if want else None, want, C.byref(n_list), ptr(direct), ptr(node_hits), ptr(kmers))
            if rc != SS_ERANGE or cap is not None or n_list.value <= want:
                break
            want = int(n_list.value)
        if rc != SS_OK:
            e = SSError(rc, "ss_reads_calls")
            e.n_list = int(n_list.value)                    # (SS_ERANGE with n_list > cap: the room to come again with)
            raise e
        ties = C.c_uint64()
        check(lib().ss_reads_classify_ties(C.byref(ties)), "ss_reads_classify_ties")
        records = int(direct.sum())
        return dict(classes=classes[:records], scores=scores[:records], first=first[:records + 1], list_node=list_node[:n_list.value],
                    list_hits=list_hits[:n_list.value], direct=direct, node_hits=node_hits, kmers=kmers, ties=int(ties.value))

    def select_class(self, kdb, row_node, parent, min_score, clades, want_counts=False):
        """A list of new ReadSets, one per entry of `clades`: the records that classify() with the same arguments puts in that
        clade (ss_reads_select_class; tests/select_class_model.py restates it).  Clade 0: the unclassified records; clade v in
        1..n: the records of class v or of a node below v.  The set is classified once, the classes stay on the device.  Each set
        is one ASCII, unbinned block in an unspecified order; the caller closes each.  want_counts: -> (sets, dict(direct=,
        node_hits=, kmers=, ties=)), classify()'s numbers from the same call.  The table's counters are left alone."""
        rn = np.ascontiguousarray(row_node, np.uint32)
        if rn.ndim != 1 or rn.size != kdb.n_rows:
            raise ValueError("one node per row of the table (%d), not %r" % (kdb.n_rows, rn.shape))
        par = np.ascontiguousarray(parent, np.uint32)
        if par.ndim != 1 or par.size < 1:
            raise ValueError("parent holds an entry per node and entry 0")
        n = par.size - 1
        cl = np.ascontiguousarray(clades, np.uint32)
        if cl.ndim != 1:
            raise ValueError("clades is a list of nodes")
        direct, node_hits, kmers = (np.zeros(n + 1, np.uint64) if want_counts else None for _ in range(3))
        hs = (C.c_void_p * max(int(cl.size), 1))()
        check(lib().ss_reads_select_class(kdb.handle, self._h, ptr(rn if rn.size else np.zeros(1, np.uint32)), n, ptr(par), int(min_score),
                                          ptr(cl if cl.size else np.zeros(1, np.uint32)), int(cl.size), hs,
                                          *(ptr(a) if want_counts else None for a in (direct, node_hits, kmers))), "ss_reads_select_class")
        sets = []
        for h in hs[:cl.size]:
            sub = ReadSet.__new__(ReadSet)
            sub._h = C.c_void_p(h)
            sets.append(sub)
        if not want_counts:
            return sets
        ties = C.c_uint64()
        check(lib().ss_reads_classify_ties(C.byref(ties)), "ss_reads_classify_ties")
        return sets, dict(direct=direct, node_hits=node_hits, kmers=kmers, ties=int(ties.value))

    def classify_strains(self, kdb, row_sets, n_strains, min_score, want_sets=True, want_records=False):
        """Every record assigned to the set of called strains that explain it best (ss_reads_classify_strains;
        tests/strain_set_model.py restates it).  row_sets[i]: the mask of row i of the table, bit j - 1 set when called strain j
        (1..n_strains) has its k-mer.  -> dict(unique=, tied=, strain_hits=, kmers= np.uint64[n_strains + 1], ties= records with a
        tie, set_reads= np.uint64[1 << n_strains] or None, sets= np.uint16 and scores= np.uint32 per record in read_back() order,
        or None).  Rows that share a k-mer under different masks count for mask 0.  The table's counters are left alone."""
        rs = _row_sets(kdb, row_sets)
        n = max(int(n_strains), 0)
        uniq, tied, hits, kmers = (np.zeros(n + 1, np.uint64) for _ in range(4))
        set_reads = np.zeros(1 << n, np.uint64) if want_sets and 1 <= n <= STRAIN_SET_MAX else None
        sets = scores = None
        if want_records:
            # (the records as ss_reads_support counts them: ss_reads_info's count includes reads without a base)
            room = max(1, int(self.support(kdb, 2)[0].sum()))
            sets, scores = np.zeros(room, np.uint16), np.zeros(room, np.uint32)
        check(lib().ss_reads_classify_strains(kdb.handle, self._h, ptr(rs), n, int(min_score), ptr(uniq), ptr(tied), ptr(hits), ptr(kmers),
                                              ptr(set_reads) if set_reads is not None else None, ptr(sets) if want_records else None,
                                              ptr(scores) if want_records else None), "ss_reads_classify_strains")
        ties = C.c_uint64()
        check(lib().ss_reads_classify_strains_ties(C.byref(ties)), "ss_reads_classify_strains_ties")
        if want_records:
            records = int(uniq.sum() + tied[0])
            sets, scores = sets[:records], scores[:records]
        return dict(unique=uniq, tied=tied, strain_hits=hits, kmers=kmers, ties=int(ties.value), set_reads=set_reads, sets=sets, scores=scores)

    def select_strains(self, kdb, row_sets, n_strains, min_score, want, how, want_counts=False):
        """A list of new ReadSets, one per entry of `want` (masks) and `how` (0: the records whose set equals the mask, mask 0 the
        unassigned ones; 1: the records whose set shares a strain with it), from the sets classify_strains() with the same
        arguments gives (ss_reads_select_strains).  The set is classified once.  Each set is one ASCII, unbinned block in an
        unspecified order; the caller closes each.  want_counts: -> (sets, dict(unique=, tied=, strain_hits=, kmers=, ties=))."""
        rs = _row_sets(kdb, row_sets)
        n = max(int(n_strains), 0)
        w = np.ascontiguousarray(want, np.uint16)
        h = np.ascontiguousarray(how, np.uint8)
        if w.ndim != 1 or h.shape != w.shape:
            raise ValueError("want and how are lists of the same length")
        uniq, tied, hits, kmers = (np.zeros(n + 1, np.uint64) if want_counts else None for _ in range(4))
        hs = (C.c_void_p * max(int(w.size), 1))()
        check(lib().ss_reads_select_strains(kdb.handle, self._h, ptr(rs), n, int(min_score), ptr(w if w.size else np.zeros(1, np.uint16)),
                                            ptr(h if h.size else np.zeros(1, np.uint8)), int(w.size), hs,
                                            *(ptr(a) if want_counts else None for a in (uniq, tied, hits, kmers))), "ss_reads_select_strains")
        sets = []
        for x in hs[:w.size]:
            sub = ReadSet.__new__(ReadSet)
            sub._h = C.c_void_p(x)
            sets.append(sub)
        if not want_counts:
            return sets
        ties = C.c_uint64()
        check(lib().ss_reads_classify_strains_ties(C.byref(ties)), "ss_reads_classify_strains_ties")
        return sets, dict(unique=uniq, tied=tied, strain_hits=hits, kmers=kmers, ties=int(ties.value))

    def strain_sets_resampled(self, kdb, row_sets, n_strains, min_score, seed, first, n_rep):
        """np.uint64[n_rep, 1 << n_strains]: row j is the set_reads that classify_strains() with the same arguments returns on
        resample(seed, first + j) -- the weights of the records of every set added up, from one classification and one pass over
        the records, nothing materialised (ss_reads_strain_sets_resampled).  n_rep in 1..SCAN_REPLICATES_MAX.  The table's
        counters are left alone."""
        rs = _row_sets(kdb, row_sets)
        n, reps = max(int(n_strains), 0), max(int(n_rep), 0)
        out = np.zeros((max(reps, 1), 1 << n if n <= STRAIN_SET_MAX else 1), np.uint64)
        check(lib().ss_reads_strain_sets_resampled(kdb.handle, self._h, ptr(rs), n, int(min_score), int(seed), int(first), reps, ptr(out)),
              "ss_reads_strain_sets_resampled")
        return out

    def gaps(self, kdb, row_called, min_hits, want_records=False):
        """The runs of missing k-mers inside the records, against the k-mers of the called strains (ss_reads_gaps;
        tests/gap_model.py restates it).  row_called[i]: non-zero when a called strain has the k-mer of row i of the table; None:
        every row is called.  A k-mer listed twice is called when any of its rows is.  -> dict of GAPS_FIELDS (ints), and with
        want_records (dict, np.uint32[n, 4]: hits_called, gaps, sites, detectable per record in read_back() order, also of the
        records below min_hits).  The table's counters are left alone."""
        rc = None
        if row_called is not None:
            rc = np.ascontiguousarray(np.asarray(row_called) != 0, np.uint8)
            if rc.ndim != 1 or rc.size != kdb.n_rows:
                raise ValueError("one flag per row of the table (%d), not %r" % (kdb.n_rows, rc.shape))
            if not rc.size:
                rc = np.zeros(1, np.uint8)
        out = np.zeros(GAPS_OUT, np.uint64)
        rec = None
        if want_records:
            # (the records as ss_reads_support counts them: ss_reads_info's count includes reads without a base)
            rec = np.zeros((max(1, int(self.support(kdb, 2)[0].sum())), 4), np.uint32)
        check(lib().ss_reads_gaps(kdb.handle, self._h, ptr(rc) if rc is not None else None, int(min_hits), ptr(out),
                                  ptr(rec) if want_records else None), "ss_reads_gaps")
        res = {name: int(v) for name, v in zip(GAPS_FIELDS, out)}
        return (res, rec[:res["records"]]) if want_records else res

    def order(self):
        """Put the records of a set in file order (from_flat_dev(order=False), select(), resample()) in locality order, in place
        (ss_reads_order): the records and every count stay, a scan of a cluster table gets faster.  -> self"""
        check(lib().ss_reads_order(self._h), "ss_reads_order")
        return self

    def resample(self, seed, replicate):
        """A new ReadSet: every record of this one w times, w in 0..13 a Poisson(1) draw that depends on the record's bytes,
        `seed` and `replicate` alone (ss_reads_resample; tests/boot_model.py restates it) -- identical reads share a weight.  One
        ASCII, unbinned block in an unspecified order.  The caller closes it."""
        h = C.c_void_p()
        check(lib().ss_reads_resample(self._h, int(seed), int(replicate), C.byref(h)), "ss_reads_resample")
        sub = ReadSet.__new__(ReadSet)
        sub._h = h
        return sub

    def scan_resampled(self, kdb, seed, first, n):
        """The counts of bootstrap replicates first .. first + n - 1 of this set against `kdb` from ONE pass over the reads
        (ss_scan_reads_resampled): a ReplicateCounts holding n row vectors on the device, vector j bit for bit what
        resample(seed, first + j) scanned into the reset table would give.  n in 1..SCAN_REPLICATES_MAX.  The table's counters
        are left alone.  The caller closes it."""
        out = ReplicateCounts(max(int(n), 0), kdb.n_rows)
        try:
            check(lib().ss_scan_reads_resampled(kdb.handle, self._h, int(seed), int(first), max(int(n), 0), out.dptr),
                  "ss_scan_reads_resampled")
        except Exception:
            out.close()
            raise
        return out


SCAN_REPLICATES_MAX = 16    # SS_SCAN_REPLICATES_MAX (strainscan_hip.h): replicates per call of scan_resampled


class ReplicateCounts:
    """uint32[n, n_rows] on the device: the row vectors ReadSet.scan_resampled fills, one per replicate."""

    def __init__(self, n, n_rows):
        self.n, self.n_rows = int(n), int(n_rows)
        d = C.c_void_p()
        check(lib().ss_dev_alloc(C.byref(d), max(16, self.n * self.n_rows * 4)), "ss_dev_alloc")
        self.dptr = d

    def vector_dptr(self, j):
        """The device address of replicate j's vector (what KmerDB.load_counts_rows_dev takes)."""
        if not 0 <= int(j) < self.n:
            raise IndexError("replicate %r of %d" % (j, self.n))
        return C.c_void_p(self.dptr.value + int(j) * self.n_rows * 4)

    def load_into(self, kdb, j, stream=None):
        """Replicate j's counts become the table's (ss_counts_load_rows_dev)."""
        kdb.load_counts_rows_dev(self.vector_dptr(j), stream)

    def row_vector(self, j):
        """A host copy of replicate j's vector, np.uint32[n_rows]."""
        out = np.zeros(self.n_rows, np.uint32)
        if self.n_rows:
            check(lib().ss_memcpy_d2h(ptr(out), self.vector_dptr(j), self.n_rows * 4, None), "ss_memcpy_d2h")
            check(lib().ss_device_sync(), "ss_device_sync")
        return out

    def close(self):
        if getattr(self, "dptr", None):
            lib().ss_dev_free(self.dptr)
            self.dptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LABELS_MAX = 15     # SS_LABELS_MAX (strainscan_hip.h): labels per call of the labelled forms


def _row_labels(kdb, row_labels):
    lab = np.ascontiguousarray(row_labels, np.uint8)
    if lab.ndim != 1 or lab.size != kdb.n_rows:
        raise ValueError("one label per row of the table (%d), not %r" % (kdb.n_rows, lab.shape))
    return lab if lab.size else np.zeros(1, np.uint8)


def _calls(name):
    """what the counter entry point `name` reports: calls so far in this process"""
    n = C.c_uint64()
    check(getattr(lib(), name)(C.byref(n)), name)
    return n.value


def labeled_calls():
    """Calls of ss_reads_support_labeled and ss_reads_select_labeled so far in this process."""
    return _calls("ss_reads_labeled_calls")


def select_calls():
    """Calls of ss_reads_select so far in this process."""
    return _calls("ss_reads_select_calls")


def resample_calls():
    """Calls of ss_reads_resample so far in this process."""
    return _calls("ss_reads_resample_calls")


def scan_resampled_calls():
    """Calls of ss_scan_reads_resampled so far in this process."""
    return _calls("ss_scan_reads_resampled_calls")


CLASS_NODES_MAX = 65535     # SS_CLASS_NODES_MAX (strainscan_hip.h)


def classify_calls():
    """Calls of ss_reads_classify so far in this process."""
    return _calls("ss_reads_classify_calls")


CLASS_CLADES_MAX = 64       # SS_SELECT_CLADES_MAX (strainscan_hip.h): clades per call of select_class


def select_class_calls():
    """Calls of ss_reads_select_class so far in this process."""
    return _calls("ss_reads_select_class_calls")


STRAIN_SET_MAX = 16         # SS_STRAIN_SET_MAX (strainscan_hip.h): called strains per call of classify_strains
SELECT_STRAINS_MAX = 32     # SS_SELECT_STRAINS_MAX (strainscan_hip.h): entries per call of select_strains


def _row_sets(kdb, row_sets):
    rs = np.ascontiguousarray(row_sets, np.uint16)
    if rs.ndim != 1 or rs.size != kdb.n_rows:
        raise ValueError("one mask per row of the table (%d), not %r" % (kdb.n_rows, rs.shape))
    return rs if rs.size else np.zeros(1, np.uint16)


def classify_strains_calls():
    """Calls of ss_reads_classify_strains so far in this process."""
    return _calls("ss_reads_classify_strains_calls")


def select_strains_calls():
    """Calls of ss_reads_select_strains so far in this process."""
    return _calls("ss_reads_select_strains_calls")


EM_VECTORS_MAX = 1024       # SS_EM_VECTORS_MAX (strainscan_hip.h): count vectors per call of em_strain_sets
EM_LDS_SETS = 6144          # SS_EM_LDS_SETS (strainscan_hip.h): the sets a workgroup of em_strain_sets keeps in LDS


GAPS_OUT = 18               # SS_GAPS_OUT (strainscan_hip.h): the totals of gaps()
GAPS_FIELDS = ("records", "assessed", "windows", "hits_called", "hits_cluster", "misses", "gap_lt", "gap_km1", "gap_k", "gap_k_2k", "gap_ge2k",
               "gaps_in_cluster", "sites", "reads_with_sites", "detectable", "kmers", "kmers_called", "long_records")


def gaps_calls():
    """Calls of ss_reads_gaps so far in this process."""
    return _calls("ss_reads_gaps_calls")


def strain_sets_resampled_calls():
    """Calls of ss_reads_strain_sets_resampled so far in this process."""
    return _calls("ss_reads_strain_sets_resampled_calls")


def em_strain_sets(counts, masks, n_strains, max_iter, tol):
    """The EM over equivalence classes on the device (ss_em_strain_sets; tests/em_model.py restates it): counts[v][s] = the reads
    of vector v whose set is masks[s] (non-zero, distinct masks of strains 1..n_strains) -> (rho np.float64[n_vec, n_strains],
    iters np.uint32[n_vec]).  One launch for all vectors; the same input gives the same bits."""
    counts = np.ascontiguousarray(counts, np.uint64)
    masks = np.ascontiguousarray(masks, np.uint16)
    if counts.ndim != 2 or masks.ndim != 1 or counts.shape[1] != masks.size:
        raise ValueError("counts is [vectors][sets] and masks [sets], not %r and %r" % (counts.shape, masks.shape))
    n_vec, n_sets = counts.shape
    n = max(int(n_strains), 0)
    rho = np.zeros((max(n_vec, 1), max(n, 1)), np.float64)
    iters = np.zeros(max(n_vec, 1), np.uint32)
    check(lib().ss_em_strain_sets(ptr(counts if counts.size else np.zeros(1, np.uint64)), ptr(masks if masks.size else np.zeros(1, np.uint16)),
                                  n_sets, n, n_vec, int(max_iter), float(tol), ptr(rho), ptr(iters)), "ss_em_strain_sets")
    return rho[:n_vec, :n], iters[:n_vec]


def em_strain_sets_calls():
    """Calls of ss_em_strain_sets so far in this process."""
    return _calls("ss_em_strain_sets_calls")


def flat_record_keys(flat):
    """np.uint64[n, 2]: the 128-bit digest of every non-empty record of a flat block (bytes), in order (ss_flat_record_keys)."""
    flat = bytes(flat)
    n = C.c_uint64()
    check(lib().ss_flat_record_keys(flat, len(flat), None, 0, C.byref(n)), "ss_flat_record_keys")
    keys = np.zeros((n.value, 2), np.uint64)
    if n.value:
        check(lib().ss_flat_record_keys(flat, len(flat), ptr(keys), n.value, C.byref(n)), "ss_flat_record_keys")
    return keys


def extract_write(in_paths, keys, out_paths):
    """Every record of the input files (one, or a pair walked in lockstep) whose flat form has a digest among `keys`
    (np.uint64[n, 2]) goes to out_paths, original text byte for byte; a pair when either mate is selected (ss_extract_write).
    -> dict(read=, written=, mate1_only=, mate2_only=).  No output file is left behind when it fails (SSError)."""
    ins = [os.fsencode(p) for p in in_paths]
    outs = [os.fsencode(p) for p in out_paths]
    if len(ins) != len(outs):
        raise ValueError("one output path per input path")
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1, 2)
    c = (C.c_uint64 * 4)()
    check(lib().ss_extract_write((C.c_char_p * len(ins))(*ins), len(ins), ptr(keys) if keys.size else None, keys.shape[0],
                                 (C.c_char_p * len(outs))(*outs), c), "ss_extract_write")
    return dict(zip(("read", "written", "mate1_only", "mate2_only"), (int(v) for v in c)))


def extract_write_pairs(in_paths, keys, out_paths):
    """extract_write for a selection made on joined pairs (ReadSet.load_pairs): both records of pair i go to the two out_paths
    when the digest of mate 1 + 'N' + mate 2 is among `keys` (ss_extract_write_pairs).  -> dict(read=, written=, pairs=)."""
    ins = [os.fsencode(p) for p in in_paths]
    outs = [os.fsencode(p) for p in out_paths]
    if len(ins) != 2 or len(outs) != 2:
        raise ValueError("two input paths and two output paths")
    keys = np.ascontiguousarray(keys, np.uint64).reshape(-1, 2)
    c = (C.c_uint64 * 4)()
    check(lib().ss_extract_write_pairs((C.c_char_p * 2)(*ins), 2, ptr(keys) if keys.size else None, keys.shape[0],
                                       (C.c_char_p * 2)(*outs), c), "ss_extract_write_pairs")
    return dict(zip(("read", "written", "pairs"), (int(v) for v in c)))


def read_calls_calls():
    """Calls of ss_reads_calls so far in this process."""
    return _calls("ss_reads_calls_calls")


def read_calls_write(in_paths, out_paths, calls, node_value):
    """The table of `--read_calls` (ss_read_calls_write): out_paths[f] gets the header and one line  name, node, score, length,
    hits  per record of in_paths[f], in file order.  calls: what ReadSet.calls returned for the set loaded from in_paths[0] in
    file order (ReadSet.load_ordered) or, for two paths, joined from both in line order (ReadSet.load_pairs(order=False));
    node_value: np.int64[n_nodes + 1], what is written for a class or a listed node.  -> dict(read=, written=, classified=,
    empty=).  No output file is left behind when it fails (SSError; SS_EIO: the files are not those the set was loaded from)."""
    ins = [os.fsencode(p) for p in in_paths]
    outs = [os.fsencode(p) for p in out_paths]
    if len(ins) != len(outs) or len(ins) not in (1, 2):
        raise ValueError("one or two input paths and as many output paths")
    classes, scores = (np.ascontiguousarray(calls[k], np.uint32) for k in ("classes", "scores"))
    first = np.ascontiguousarray(calls["first"], np.uint64)
    nodes, hits = (np.ascontiguousarray(calls[k], np.uint32) for k in ("list_node", "list_hits"))
    value = np.ascontiguousarray(node_value, np.int64)
    if first.size != classes.size + 1 or scores.size != classes.size or nodes.size != hits.size or value.size < 1:
        raise ValueError("classes, scores [records], first [records + 1], list_node, list_hits [n_list], node_value [n_nodes + 1]")
    c = (C.c_uint64 * 4)()
    check(lib().ss_read_calls_write((C.c_char_p * len(ins))(*ins), len(ins), (C.c_char_p * len(outs))(*outs), classes.size,
                                    ptr(classes) if classes.size else None, ptr(scores) if scores.size else None, ptr(first),
                                    ptr(nodes) if nodes.size else None, ptr(hits) if hits.size else None, ptr(value), value.size - 1, c),
          "ss_read_calls_write")
    return dict(zip(("read", "written", "classified", "empty"), (int(v) for v in c)))


def join_pairs_calls():
    """Joins (ss_reads_join_pairs_dev, ss_reads_load_pairs) so far in this process."""
    return _calls("ss_reads_join_pairs_calls")


def support_calls():
    """Calls of ss_reads_support so far in this process."""
    return _calls("ss_reads_support_calls")


def scan_multi_launches():
    """Launches of the several-tables kernel so far, per filter kind: dict(bloom=, expect_hits=, plain=)."""
    out = (C.c_uint64 * 3)()
    check(lib().ss_scan_multi_launches(out), "ss_scan_multi_launches")
    return dict(bloom=out[0], expect_hits=out[1], plain=out[2])


class NodeSet:
    """All tree-node k-mer row lists on the device (files <db>/kmers/<id>, identify.py:116-118)."""

    def __init__(self, row_lists):
        require_gpu()
        offs = np.zeros(len(row_lists) + 1, np.uint64)
        dedup = []
        for i, r in enumerate(row_lists):
            r = np.unique(np.asarray(r, np.int64))  # set(map(int, ...)) at identify.py:118
            dedup.append(r.astype(np.uint32))
            offs[i + 1] = offs[i] + r.size
        rows = np.concatenate(dedup) if dedup else np.zeros(0, np.uint32)
        rows = np.ascontiguousarray(rows, np.uint32)
        h = C.c_void_p()
        check(lib().ss_nodes_create(ptr(rows), ptr(offs), len(row_lists), C.byref(h)), "ss_nodes_create")
        self._h = h
        self.n_nodes = len(row_lists)
        self.n_rows_total = int(offs[-1])

    @classmethod
    def from_sorted(cls, rows, offsets):
        """Node lists that are already de-duplicated and sorted, back to back: rows u32[offsets[-1]],
        offsets[n_nodes + 1] (no per-list np.unique: 0.1 s for the 1645 lists of an E. coli database)."""
        require_gpu()
        rows = np.ascontiguousarray(rows, np.uint32)
        offs = np.ascontiguousarray(offsets, np.uint64)
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().ss_nodes_create(ptr(rows), ptr(offs), offs.size - 1, C.byref(h)), "ss_nodes_create")
        self._h = h
        self.n_nodes = offs.size - 1
        self.n_rows_total = int(offs[-1]) if offs.size else 0
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().ss_nodes_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reduce(self, db):
        st = np.zeros(self.n_nodes, NODE_STAT_DTYPE)
        check(lib().ss_nodes_reduce(self._h, db.handle, ptr(st)), "ss_nodes_reduce")
        return st

    # -- harvest path (ss_nodes.hip): bind once per database, then per scan harvest + reduce over the touched nodes
    def bind(self, db):
        check(lib().ss_nodes_bind(self._h, db.handle), "ss_nodes_bind")
        self._bound = db
        return self

    def harvest_dev(self, db, stream=None):
        check(lib().ss_nodes_harvest_dev(self._h, db.handle, stream), "ss_nodes_harvest_dev")

    def reduce_touched_dev(self, stats_dptr, stream=None):
        check(lib().ss_nodes_reduce_touched_dev(self._h, stats_dptr, stream), "ss_nodes_reduce_touched_dev")

    def harvest(self, db, between=None):
        """Statistics of all nodes from the counters of `db` (bound): harvest, [between(self): the multi-GPU
        exchange], reduce over the touched nodes.  `between` may return an object with .complete() (read after the
        statistics have arrived: dist.exchange_touched's capped packing never waits for the host; when the packed counts
        did not fit its buffer, the harvest is simply run again -- the counters are still in the table -- and the
        exchange repeats with the larger buffer it has sized meanwhile; all ranks see the same total and repeat together)."""
        if getattr(self, "_bound", None) is not db:
            self.bind(db)
        dst = C.c_void_p()
        nbytes = max(1, self.n_nodes) * NODE_STAT_DTYPE.itemsize
        check(lib().ss_dev_alloc(C.byref(dst), nbytes), "ss_dev_alloc")
        dirty = False
        try:
            for _ in range(3):
                dirty = True
                self.harvest_dev(db)
                pending = between(self) if between is not None else None
                self.reduce_touched_dev(dst)          # clears the count buffer and the flags
                dirty = False
                st = np.zeros(self.n_nodes, NODE_STAT_DTYPE)
                if self.n_nodes:
                    check(lib().ss_memcpy_d2h(ptr(st), dst, self.n_nodes * NODE_STAT_DTYPE.itemsize, None), "ss_memcpy_d2h")
                check(lib().ss_device_sync(), "ss_device_sync")
                if pending is None or not hasattr(pending, "complete") or pending.complete():
                    return st
            raise RuntimeError("exchange of the touched nodes did not fit its buffer after three rounds")
        finally:
            if dirty:
                # harvest or the exchange raised: the dense buffer still holds counts that the next harvest would add to
                lib().ss_nodes_clear_dev(self._h, None)
                lib().ss_device_sync()
            lib().ss_dev_free(dst)

    def reduce_dev(self, counts_rows_dptr, row_valid_dptr, stats_dptr, stream=None):
        check(lib().ss_nodes_reduce_dev(self._h, counts_rows_dptr, row_valid_dptr, stats_dptr, stream),
              "ss_nodes_reduce_dev")


def rows_reduce(db, rows):
    rows = np.ascontiguousarray(np.unique(np.asarray(rows, np.int64)), np.uint32)
    st = NodeStat()
    check(lib().ss_rows_reduce(db.handle, ptr(rows), rows.size, C.byref(st)), "ss_rows_reduce")
    return dict(length=st.length, n_pos=st.n_pos, n_kept=st.n_kept, sum_kept=st.sum_kept, median2=st.median2)


def gz_inflate(path, threads=0, mode=0):
    """Whole-file gunzip as the ingest does it (ss_gz_inflate): bytes, or None when the file is not inflated this
    way (see include/strainscan_hip.h).  mode 1 = threaded inflater only, 2 = libdeflate only."""
    text, n = C.c_void_p(), C.c_uint64()
    rc = lib().ss_gz_inflate(os.fsencode(path), int(threads), int(mode), C.byref(text), C.byref(n))
    if rc != SS_OK:
        return None
    try:
        return C.string_at(text, n.value)
    finally:
        lib().ss_gz_free(text)


def encode_kmer_fasta(text, k=31):
    nl = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    n = nl // 2
    keys = np.empty(n, np.uint64)
    flags = np.empty(n, np.uint8)
    check(lib().ss_kmerfa_encode_mem(text, len(text), int(k), n, ptr(keys), ptr(flags)), "ss_kmerfa_encode_mem")
    return keys, flags


def fastx_to_flat(text):
    out = np.empty(len(text) + 2, np.uint8)
    n, nrec = C.c_uint64(), C.c_uint64()
    check(lib().ss_fastx_to_flat(text, len(text), ptr(out), C.byref(n), C.byref(nrec)), "ss_fastx_to_flat")
    return out[:n.value].tobytes(), nrec.value


# ss_input_kind: what an input path holds (BAM is told apart by its inflated magic, not by its name)
INPUT_KINDS = {0: "fastx", 1: "bam", 2: "bam", 3: "cram"}


def input_kind(path):
    """'bam' (gzip'ed or an uncompressed stream), 'cram', or 'fastx' (FASTA/FASTQ, plain or gzip, and unreadable paths)."""
    k = C.c_int()
    check(lib().ss_input_kind(os.fsencode(path), C.byref(k)), "ss_input_kind")
    return INPUT_KINDS[k.value]


def refuse_cram(paths):
    """ValueError naming the format when one of the paths is a CRAM file (not decoded; never parsed as text)."""
    for p in paths:
        try:
            with open(p, "rb") as f:
                magic = f.read(4)
        except (OSError, TypeError):
            continue                         # (no such file: the load reports it)
        if magic == b"CRAM":
            raise ValueError("%s is a CRAM file: CRAM input is not supported (BAM, FASTA and FASTQ, plain or gzip, are)" % p)


def bam_decode(stream, shard_rank=0, shard_world=1):
    """The host BAM decoder over an inflated stream (bytes from b'BAM\\1') -> (flat block bytes, this rank's kept records)."""
    stream = bytes(stream)
    n, nrec = C.c_uint64(), C.c_uint64()
    check(lib().ss_bam_decode(stream, len(stream), int(shard_rank), int(shard_world), None, 0, C.byref(n), C.byref(nrec)),
          "ss_bam_decode")
    out = np.empty(max(n.value, 1), np.uint8)
    check(lib().ss_bam_decode(stream, len(stream), int(shard_rank), int(shard_world), ptr(out), n.value, C.byref(n),
                              C.byref(nrec)), "ss_bam_decode")
    return out[:n.value].tobytes(), nrec.value


def bam_counters():
    """{'device', 'host', 'kept', 'skipped'}: BAM files decoded on the device / on the host, records kept / skipped."""
    out = (C.c_uint64 * 4)()
    check(lib().ss_bam_counters(out), "ss_bam_counters")
    return dict(zip(("device", "host", "kept", "skipped"), (int(v) for v in out)))


BAM_SELECT_COUNTERS = ("records", "kept", "selected", "written")


def _label_args(kdb, labels, n_labels, label):
    if labels is None:
        return None, 0, 0
    return ptr(_row_labels(kdb, labels)), max(int(n_labels), 0), max(int(label), 0)


def bam_select(stream, kdb, min_hits, labels=None, n_labels=0, label=0, pairs=False):
    """The kept records of the selected templates of an inflated BAM stream (bytes from b'BAM\\1'), concatenated in file order,
    and dict(records=, kept=, selected=, written=) (ss_bam_select).  labels: one label per row of the table, the hits counted
    are those of `label` (as ReadSet.select_labeled).  pairs: by fragment (ss_bam_select_pairs) -- a kept record is written when
    its hits and its mate's together reach min_hits, `selected` counts fragments."""
    stream = bytes(stream)
    lab, nl, lb = _label_args(kdb, labels, n_labels, label)
    out = np.empty(max(len(stream), 1), np.uint8)                  # (the records written are records of the stream)
    n, c = C.c_uint64(), (C.c_uint64 * 4)()
    name = "ss_bam_select_pairs" if pairs else "ss_bam_select"
    check(getattr(lib(), name)(stream, len(stream), kdb.handle, lab, nl, lb, int(min_hits), ptr(out), len(stream), C.byref(n), c), name)
    return out[:n.value].tobytes(), dict(zip(BAM_SELECT_COUNTERS, (int(v) for v in c)))


def bam_extract(in_path, kdb, min_hits, out_path, labels=None, n_labels=0, label=0, pairs=False):
    """One BAM file -> out_path, a BGZF BAM of the input's header and the kept records of the selected templates
    (ss_bam_extract) -> dict(records=, kept=, selected=, written=).  No file is left behind when it fails (SSError).
    pairs: by fragment, as bam_select (ss_bam_extract_pairs)."""
    lab, nl, lb = _label_args(kdb, labels, n_labels, label)
    c = (C.c_uint64 * 4)()
    name = "ss_bam_extract_pairs" if pairs else "ss_bam_extract"
    check(getattr(lib(), name)(os.fsencode(in_path), kdb.handle, lab, nl, lb, int(min_hits), os.fsencode(out_path), c), name)
    return dict(zip(BAM_SELECT_COUNTERS, (int(v) for v in c)))


BAM_PAIR_COUNTERS = ("records", "kept", "pairs", "orphans", "singles", "violating")
BAM_NO_MATE, BAM_NOT_KEPT = 0xFFFFFFFE, 0xFFFFFFFF


def bam_mates(stream):
    """The mate link of an inflated BAM stream (bytes from b'BAM\\1') -> (np.uint32[records], dict of BAM_PAIR_COUNTERS):
    mate[r] = the record index of kept record r's mate, BAM_NO_MATE, or BAM_NOT_KEPT (ss_bam_mates).  Names that are not one first
    and one second mate show in "violating" (the link of the other records is still returned); a damaged stream raises."""
    require_gpu()
    stream = bytes(stream)
    c = (C.c_uint64 * 6)()
    mate = np.empty(len(stream) // 36 + 1, np.uint32)              # (a record is 36 bytes and more)
    rc = lib().ss_bam_mates(stream, len(stream), ptr(mate), mate.size, c)
    if rc != SS_OK and not (rc == SS_EIO and c[5]):
        raise SSError(rc, "ss_bam_mates")
    return mate[:int(c[0])], dict(zip(BAM_PAIR_COUNTERS, (int(v) for v in c)))


def _bam_timing(name, steps):
    """the eight slots of the timing entry point `name`, in milliseconds, under the names of `steps`"""
    out = (C.c_double * 8)()
    check(getattr(lib(), name)(out), name)
    return dict(zip(steps, (float(v) for v in out)))


BAM_PAIRS_STEPS = ("stream", "walk_decode", "keys", "sort", "link", "lengths_scan", "join", "total")


def bam_pairs_timing():
    """The last ReadSet.load_pairs_bam in milliseconds, step by step (ss_bam_pairs_timing)."""
    return _bam_timing("ss_bam_pairs_timing", BAM_PAIRS_STEPS)


BAM_TAG_COUNTERS = ("records", "tagged", "classified", "already_tagged", "fragments", "ties")
BAM_TAG_BYTES = 14      # SS_BAM_TAG_BYTES (strainscan_hip.h)
BAM_TAG_STEPS = ("stream", "walk_decode", "mates_join", "classify", "check_copy", "download", "compress_write", "total")


class BamTagError(SSError):
    """SSError of bam_tag / bam_tag_file with `counters`, the dict of BAM_TAG_COUNTERS the call had filled: SS_EIO with
    counters["already_tagged"] != 0 says how many kept records already bear one of the tags."""
    def __init__(self, code, where, counters):
        super().__init__(code, where)
        self.counters = counters


def _tag_args(kdb, row_node, parent, node_value, tags, want_counts):
    rn = np.ascontiguousarray(row_node, np.uint32)
    if rn.ndim != 1 or rn.size != kdb.n_rows:
        raise ValueError("one node per row of the table (%d), not %r" % (kdb.n_rows, rn.shape))
    par = np.ascontiguousarray(parent, np.uint32)
    if par.ndim != 1 or par.size < 1:
        raise ValueError("parent holds an entry per node and entry 0")
    n = par.size - 1
    val = np.ascontiguousarray(node_value, np.int32)
    if val.ndim != 1 or val.size != n + 1:
        raise ValueError("node_value holds an entry per node and entry 0 (%d), not %r" % (n + 1, val.shape))
    tags = bytes(tags)
    if len(tags) != 4:
        raise ValueError("tags is four bytes: two tags of two")
    counts = tuple(np.zeros(n + 1, np.uint64) if want_counts else None for _ in range(3))
    return rn if rn.size else np.zeros(1, np.uint32), par, n, val, tags, counts


def bam_tag(stream, kdb, row_node, parent, m, node_value, pairs=False, tags=b"snsc", want_counts=False):
    """An inflated BAM stream (bytes from b'BAM\\1') with the class of every kept record appended as two aux tags
    (ss_bam_tag_stream; tests/bam_tag_model.py restates it): every record behind the header in file order, a kept one with
    tags[0:2]:i:node_value[class] and tags[2:4]:i:score behind its last aux field and its block_size raised by 14.  row_node,
    parent and m as ReadSet.classify; node_value: one int32 per node and entry 0.  pairs: both mates of a pair carry the class of
    the fragment.  -> (body bytes, dict of BAM_TAG_COUNTERS[, direct, node_hits, kmers]).  BamTagError (code SS_EIO) when a kept
    record already bears one of the tags, has damaged aux fields, or a name group is no pair."""
    stream = bytes(stream)
    rn, par, n, val, tags, counts = _tag_args(kdb, row_node, parent, node_value, tags, want_counts)
    cap = len(stream) + BAM_TAG_BYTES * (len(stream) // 36 + 1)      # (a record is 36 bytes and more)
    out = np.empty(max(cap, 1), np.uint8)
    ln, c = C.c_uint64(), (C.c_uint64 * 6)()
    rc = lib().ss_bam_tag_stream(stream, len(stream), kdb.handle, ptr(rn), n, ptr(par), int(m), ptr(val), tags, int(bool(pairs)), ptr(out),
                                 cap, C.byref(ln), c, *(ptr(a) if want_counts else None for a in counts))
    cd = dict(zip(BAM_TAG_COUNTERS, (int(v) for v in c)))
    if rc != SS_OK:
        raise BamTagError(rc, "ss_bam_tag_stream", cd)
    return (out[:ln.value].tobytes(), cd) + (counts if want_counts else ())


def bam_tag_file(in_path, kdb, row_node, parent, m, node_value, out_path, pairs=False, tags=b"snsc", want_counts=False):
    """One BAM file -> out_path, a BGZF BAM of the input's header and bam_tag's body (ss_bam_tag_file) -> dict of
    BAM_TAG_COUNTERS[, direct, node_hits, kmers].  No file is left behind when it fails (BamTagError)."""
    rn, par, n, val, tags, counts = _tag_args(kdb, row_node, parent, node_value, tags, want_counts)
    c = (C.c_uint64 * 6)()
    rc = lib().ss_bam_tag_file(os.fsencode(in_path), kdb.handle, ptr(rn), n, ptr(par), int(m), ptr(val), tags, int(bool(pairs)),
                               os.fsencode(out_path), c, *(ptr(a) if want_counts else None for a in counts))
    cd = dict(zip(BAM_TAG_COUNTERS, (int(v) for v in c)))
    if rc != SS_OK:
        raise BamTagError(rc, "ss_bam_tag_file", cd)
    return (cd,) + counts if want_counts else cd


def bam_tag_calls():
    """Calls of ss_bam_tag_stream and ss_bam_tag_file so far in this process."""
    return _calls("ss_bam_tag_calls")


def bam_tag_timing():
    """The last bam_tag_file in milliseconds, step by step (ss_bam_tag_timing)."""
    return _bam_timing("ss_bam_tag_timing", BAM_TAG_STEPS)


def bgzf_write(path, head, body, level=1):
    """head + body as a BGZF file: members of at most 0xff00 bytes each and the EOF block (ss_bgzf_write; host only)."""
    head, body = bytes(head), bytes(body)
    check(lib().ss_bgzf_write(os.fsencode(path), head, len(head), body, len(body), int(level)), "ss_bgzf_write")


def bam_extract_calls():
    """Calls of ss_bam_select and ss_bam_extract so far in this process."""
    return _calls("ss_bam_extract_calls")


BAM_EXTRACT_STEPS = ("stream", "walk_decode", "hits", "join", "gather", "download", "compress_write", "total")


def bam_extract_timing():
    """The last bam_extract in milliseconds, step by step (ss_bam_extract_timing)."""
    return _bam_timing("ss_bam_extract_timing", BAM_EXTRACT_STEPS)


def set_min_base_qual(q):
    """The base-quality mask of every later load in this process (ss_set_min_base_qual): a base whose Phred quality is below
    `q` becomes N (FASTQ: quality character < chr(33 + q), as `jellyfish count -Q`; BAM: qual[i] < q; FASTA untouched).
    0 = off, the default.  ValueError unless q is an integer in 0..93."""
    if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= int(q) <= 93:
        raise ValueError("min_base_qual must be an integer in 0..93, not %r" % (q,))
    check(lib().ss_set_min_base_qual(int(q)), "ss_set_min_base_qual")


def get_min_base_qual():
    return int(lib().ss_get_min_base_qual())


def mask_counters():
    """{'masked', 'bam_no_qual'}: bases the quality mask turned into N so far in this process, BAM records that carried no
    qualities (left unmasked) while it was on."""
    out = (C.c_uint64 * 2)()
    check(lib().ss_mask_counters(out), "ss_mask_counters")
    return dict(masked=int(out[0]), bam_no_qual=int(out[1]))


def read_flat_blocks(paths, cap=32 << 20, overlap=30):
    """Generator of (flat block bytes, n_records) from FASTA/FASTQ(.gz) files."""
    paths = [os.fsencode(p) for p in paths if p]
    arr = (C.c_char_p * len(paths))(*paths)
    h = C.c_void_p()
    check(lib().ss_reader_open(arr, len(paths), C.byref(h)), "ss_reader_open")
    try:
        check(lib().ss_reader_set_overlap(h, overlap), "ss_reader_set_overlap")
        buf = np.empty(cap, np.uint8)
        while True:
            n, nrec = C.c_uint64(), C.c_uint64()
            check(lib().ss_reader_next(h, ptr(buf), cap, C.byref(n), C.byref(nrec)), "ss_reader_next")
            if n.value == 0:
                break
            yield buf[:n.value].tobytes(), nrec.value
    finally:
        lib().ss_reader_close(h)


def revcomp(s):
    b = s.encode() if isinstance(s, str) else bytes(s)
    out = C.create_string_buffer(len(b))
    check(lib().ss_revcomp(b, out, len(b)), "ss_revcomp")
    return out.raw.decode() if isinstance(s, str) else out.raw
