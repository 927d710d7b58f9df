"""ctypes binding of libpaffy_hip.so plus helpers named after the reference commands.

Names follow the reference CLI (`paffy invert | trim | shatter`, impl/paf_<cmd>.c): a Stage is
one command of a pipe; `trim` takes the reference's -r/-t/-f options. torch is used only for
device buffers and the stream handle.
"""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
_LIB = os.environ.get("PAFFY_HIP_LIB", os.path.join(HERE, "libpaffy_hip.so"))  # override for A/B experiments only

INVERT, TRIM_IDENTITY, TRIM_FIXED, SHATTER, ADD_MISMATCHES, REMOVE_MISMATCHES, PASS, FILTER, TRIM_ENDS, STATS = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
DECHUNK, UPCONVERT = 12, 13  # PAFFY_DECHUNK (first stage only), PAFFY_UPCONVERT (a stage list of its own)


class BedOpts(C.Structure):
    _fields_ = [("binary", C.c_int32), ("exclude_unaligned", C.c_int32), ("exclude_aligned", C.c_int32), ("include_inverted", C.c_int32),
                ("min_size", C.c_int64)]


class Stage(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p0", C.c_float), ("p1", C.c_float)]


class Filter(C.Structure):
    """Thresholds of `paffy filter` (impl/paf_filter.c:27-32): -s, -t, -u, -v, -w, -x."""
    _fields_ = [("min_chain_score", C.c_int64), ("min_alignment_score", C.c_int64), ("min_identity", C.c_double),
                ("min_identity_with_gaps", C.c_double), ("max_tile_level", C.c_int64), ("invert", C.c_int32)]


class _Error(C.Structure):
    _fields_ = [("code", C.c_int32), ("stage", C.c_int32), ("record", C.c_int64), ("aux", C.c_int64)]


class PlanInfo(C.Structure):
    _fields_ = [("n_records", C.c_int64), ("n_rows", C.c_int64), ("in_bytes", C.c_int64), ("out_bytes", C.c_int64),
                ("error", _Error)]


class SplitGroup(C.Structure):
    """paffy_split_group: one stretch of a split_file plan's output and the file it belongs to."""
    _fields_ = [("file", C.c_int64), ("out_off", C.c_int64), ("bytes", C.c_int64), ("lines", C.c_int64), ("first_record", C.c_int64),
                ("new_file", C.c_int32), ("is_small", C.c_int32)]


class FastaRecord(C.Structure):
    """paffy_fasta_record: the header in the text (after '>'), the bases in the compact buffer."""
    _fields_ = [("hdr_off", C.c_int64), ("hdr_len", C.c_int64), ("seq_off", C.c_int64), ("seq_len", C.c_int64)]


class ChainOpts(C.Structure):
    _fields_ = [("gap_open", C.c_int64), ("gap_extend", C.c_int64), ("max_gap_length", C.c_int64), ("trim_fraction", C.c_float)]


class PafError(RuntimeError):
    """A record the reference would abort on; .info holds the plan (records before it are emitted)."""

    def __init__(self, msg, info, exit_status):
        super().__init__(msg)
        self.info = info
        self.exit_status = exit_status


FLAT_WHY_ENCODER = 11  # flat_stats(): under [ADD_MISMATCHES, TRIM_IDENTITY / FILTER] the encoder on the pieces did not keep the record


def stage(kind, trim_identity=0.05, trim_fraction=1.0):
    """One command of a pipe. trim_identity = `paffy trim -r`, trim_fraction = `-t` (impl/paf_trim.c:14-16)."""
    return Stage(kind, trim_identity, trim_fraction)


def stage_trim_ends(end_bases):
    """paf_trim_ends(paf, end_bases) (impl/paf.c:575-598): the int64 argument travels in the two float slots, bit for bit."""
    import struct

    p0, p1 = struct.unpack("<ff", struct.pack("<q", end_bases))
    st = Stage(TRIM_ENDS, 0.0, 0.0)
    C.memmove(C.addressof(st) + Stage.p0.offset, struct.pack("<ff", p0, p1), 8)  # no float round trip: NaN payloads must survive
    return st


def stage_dechunk(query=True, target=True):
    """`paffy dechunk` as a stage (the first of a pipe): query=False is `-t`, target=False is `-q`."""
    return Stage(DECHUNK, 1.0 if query else 0.0, 1.0 if target else 0.0)


def library_path():
    return _LIB


def build_library(force=False):
    """Compile the gfx950 shared library in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(HERE), "include", "paffy_hip.h"))
    stale = not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s"])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise RuntimeError(f"{_LIB} is missing: run paffy_amd.build_library() (there is no CPU fallback)")
        L = C.CDLL(_LIB)
        vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
        L.paffy_hip_create.argtypes = [C.POINTER(vp), C.c_int]
        L.paffy_hip_destroy.argtypes = [vp]
        L.paffy_hip_set_stream.argtypes = [vp, vp]
        L.paffy_hip_plan.argtypes = [vp, C.POINTER(Stage), i32, vp, i64, C.POINTER(PlanInfo)]
        L.paffy_hip_emit.argtypes = [vp, vp, i64]
        L.paffy_hip_tile_plan.argtypes = [vp, vp, i64, C.POINTER(PlanInfo)]
        L.paffy_hip_tile_begin.argtypes = [vp]
        L.paffy_hip_tile_add.argtypes = [vp, vp, i64]
        L.paffy_hip_tile_run.argtypes = [vp, C.POINTER(PlanInfo)]
        L.paffy_hip_chain_begin.argtypes = [vp]
        L.paffy_hip_chain_add.argtypes = [vp, vp, i64]
        L.paffy_hip_chain_run.argtypes = [vp, C.POINTER(ChainOpts), C.POINTER(PlanInfo)]
        L.paffy_hip_chain_tags.restype = i64
        L.paffy_hip_chain_tags.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i64)]
        if hasattr(L, "paffy_hip_chain_fresh_walk"):  # an older library under PAFFY_HIP_LIB has none: the calls then raise
            L.paffy_hip_chain_fresh_walk.argtypes = [vp, C.c_int]
            L.paffy_hip_chain_fresh_stats.argtypes = [vp, C.POINTER(i64)]
        L.paffy_hip_chain_add_indexed.argtypes = [vp, vp, i64, vp]
        L.paffy_hip_chain_run_part.argtypes = [vp, C.POINTER(ChainOpts), C.POINTER(PlanInfo)]
        L.paffy_hip_chain_tail_keys.restype = i64
        L.paffy_hip_chain_tail_keys.argtypes = [vp, i64, vp]
        L.paffy_hip_chain_renumber.argtypes = [vp, vp, C.POINTER(PlanInfo), C.POINTER(i64)]
        L.paffy_hip_chain_line_keys.restype = i64
        L.paffy_hip_chain_line_keys.argtypes = [vp, i64, vp]
        L.paffy_hip_plan_rows.restype = i64
        L.paffy_hip_plan_rows.argtypes = [vp, i64, C.POINTER(C.c_uint32), C.POINTER(i64)]
        L.paffy_hip_tile_keys.restype = i64
        L.paffy_hip_tile_keys.argtypes = [vp, i64, vp]
        L.paffy_hip_emit_lines.argtypes = [vp, i64, i64, vp, i64, C.POINTER(i64)]
        L.paffy_hip_bed_begin.argtypes = [vp, C.POINTER(BedOpts)]
        L.paffy_hip_bed_add.argtypes = [vp, vp, i64]
        L.paffy_hip_bed_run.argtypes = [vp, C.POINTER(BedOpts), C.POINTER(PlanInfo)]
        L.paffy_hip_query_names.restype = i64
        L.paffy_hip_query_names.argtypes = [vp, vp, i64, i64, C.POINTER(C.c_uint64), C.POINTER(i64)]
        L.paffy_hip_query_names_counts.restype = i64
        L.paffy_hip_query_names_counts.argtypes = [vp, vp, i64, i64, C.POINTER(C.c_uint64), C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_split_by_owner.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), i64, vp, i64, C.POINTER(i64), C.POINTER(i64), vp, i64,
                                               C.POINTER(i64)]
        L.paffy_hip_split_to.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), i64, vp, i64, C.POINTER(i64), C.POINTER(i64), i64, C.POINTER(i64),
                                         C.POINTER(i64), vp, i64, C.POINTER(i64)]
        L.paffy_hip_drop_index.argtypes = [vp, vp]
        L.paffy_hip_side_names_counts.restype = i64
        L.paffy_hip_side_names_counts.argtypes = [vp, vp, i64, C.c_int, i64, C.POINTER(C.c_uint64), C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_split_sides_count.argtypes = [vp, vp, i64, C.c_int, i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_split_sides_to.argtypes = [vp, vp, i64, C.c_int, i32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), i64, vp, i64, C.POINTER(i64), C.POINTER(i64), i64,
                                               C.POINTER(i64), C.POINTER(i64), vp, vp, i64, C.POINTER(i64)]
        L.paffy_hip_bed_add_sides.argtypes = [vp, vp, i64, vp]
        L.paffy_hip_bed_failure_side.argtypes = [vp]
        L.paffy_hip_bed_sequence_keys.restype = i64
        L.paffy_hip_bed_sequence_keys.argtypes = [vp, i64, vp]
        L.paffy_hip_bed_sequences.restype = i64
        L.paffy_hip_bed_sequences.argtypes = [vp]
        L.paffy_hip_scatter_lines.argtypes = [vp, vp, vp, vp, i64, vp]
        L.paffy_hip_stream_open.argtypes = [vp, C.POINTER(Stage), i32, i64, i64, C.POINTER(vp)]
        L.paffy_hip_stream_input.restype = vp
        L.paffy_hip_stream_input.argtypes = [vp, i64, i64, C.POINTER(i64)]
        L.paffy_hip_stream_submit.argtypes = [vp, i64, C.POINTER(PlanInfo)]
        L.paffy_hip_stream_read.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
        L.paffy_hip_stream_close.argtypes = [vp]
        L.paffy_hip_sync.argtypes = [vp]
        L.paffy_hip_dedupe_plan.argtypes = [vp, vp, i64, C.c_int, C.POINTER(PlanInfo)]
        L.paffy_hip_dedupe_reset.argtypes = [vp]
        L.paffy_hip_split_begin.argtypes = [vp, C.c_int, i64]
        L.paffy_hip_split_plan.argtypes = [vp, vp, i64, C.POINTER(PlanInfo)]
        L.paffy_hip_split_groups.restype = i64
        L.paffy_hip_split_groups.argtypes = [vp, i64, C.POINTER(SplitGroup)]
        L.paffy_hip_split_file_name.restype = i64
        L.paffy_hip_split_file_name.argtypes = [vp, i64, C.c_char_p, i64]
        L.paffy_hip_split_file_count.restype = i64
        L.paffy_hip_split_file_count.argtypes = [vp]
        L.paffy_hip_split_salt.argtypes = [vp]
        L.paffy_hip_dedupe_part_keys.argtypes = [vp, vp, i64, C.c_int, i64, i32, vp, i64, C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_dedupe_part_decide.argtypes = [vp, vp, i64, C.c_int, vp]
        L.paffy_hip_dedupe_part_verdicts.argtypes = [vp, vp, i64, C.POINTER(i64)]
        L.paffy_hip_dedupe_part_plan.argtypes = [vp, i64, C.POINTER(PlanInfo)]
        L.paffy_hip_set_sequences.argtypes = [vp, i64, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(i64)]
        L.paffy_hip_set_filter.argtypes = [vp, C.POINTER(Filter)]
        L.paffy_hip_set_intervals.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(i64), i64]
        L.paffy_hip_error_exit_status.argtypes = [i32]
        L.paffy_hip_error_string.restype = C.c_char_p
        L.paffy_hip_error_string.argtypes = [i32]
        L.paffy_hip_last_error.restype = C.c_char_p
        L.paffy_hip_last_error.argtypes = [vp]
        L.paffy_hip_profile_enable.argtypes = [vp, C.c_int]
        L.paffy_hip_profile_reset.argtypes = [vp]
        L.paffy_hip_profile_only.argtypes = [vp, C.c_char_p]
        L.paffy_hip_stream_trim.argtypes = [vp]
        L.paffy_hip_profile_read.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(i64), C.c_int]
        L.paffy_hip_synth.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, vp, i64, C.POINTER(i64)]
        L.paffy_hip_synth_contigs.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, vp, i64, C.POINTER(i64)]
        L.paffy_hip_plan_stats.argtypes = [vp, C.POINTER(i64)]
        L.paffy_hip_flat_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_bed_plan.argtypes = [vp, vp, i64, C.POINTER(BedOpts), C.POINTER(PlanInfo)]
        L.paffy_hip_synth4_setup.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, i64, i64, C.c_int]
        L.paffy_hip_synth4.argtypes = [vp, C.c_uint64, C.c_uint64, vp, i64, C.POINTER(i64)]
        L.paffy_hip_device_count.restype = C.c_int
        L.paffy_hip_device_buffers.argtypes = [C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_fasta_index.argtypes = [vp, vp, i64, C.POINTER(i64), i32, C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_fasta_records.restype = i64
        L.paffy_hip_fasta_records.argtypes = [vp, i64, i64, C.POINTER(FastaRecord)]
        L.paffy_hip_fasta_copy_bases.argtypes = [vp, i64, i64, vp]
        L.paffy_hip_faffy_chunk_plan.argtypes = [vp, i64, i64, C.POINTER(PlanInfo)]
        L.paffy_hip_faffy_chunk_files.restype = i64
        L.paffy_hip_faffy_chunk_files.argtypes = [vp, i64, C.POINTER(i64)]
        L.paffy_hip_faffy_extract_plan.argtypes = [vp, C.c_char_p, i64, i64, i64, C.c_int, C.POINTER(PlanInfo)]
        if hasattr(L, "paffy_hip_faffy_extract_plan_device"):  # an older library under PAFFY_HIP_LIB has none: the call then raises
            L.paffy_hip_faffy_extract_plan_device.argtypes = [vp, vp, i64, i64, i64, C.c_int, C.POINTER(PlanInfo)]
        L.paffy_hip_faffy_merge_plan.argtypes = [vp, C.POINTER(PlanInfo)]
        L.paffy_hip_faffy_emit.argtypes = [vp, vp, i64, C.POINTER(_Error)]
        L.paffy_hip_set_sequences_fasta.argtypes = [vp, vp, i64, C.POINTER(i64), i32, C.POINTER(i64)]
        L.paffy_hip_set_intervals_fasta.argtypes = [vp, vp, i64, C.POINTER(i64), i32, C.POINTER(i64)]
        L.paffy_hip_fasta_index_headers.argtypes = [vp, vp, i64, C.POINTER(i64), i32, C.POINTER(i64)]
        L.paffy_hip_fasta_seen.argtypes = [vp, vp, i64, C.c_int, C.POINTER(C.c_uint8)]
        if hasattr(L, "paffy_hip_fasta_name_order"):  # an older library under PAFFY_HIP_LIB has neither: the calls then raise
            L.paffy_hip_fasta_name_order.argtypes = [vp, i64, vp, vp, C.POINTER(i64)]
            L.paffy_hip_name_sort_stats.argtypes = [vp, C.POINTER(i64)]
        if hasattr(L, "paffy_hip_intervals_info"):  # an older library under PAFFY_HIP_LIB has neither: the calls then raise
            L.paffy_hip_intervals_info.argtypes = [vp, C.POINTER(i64)]
            L.paffy_hip_intervals_read.argtypes = [vp, i64, i64, C.POINTER(i64), C.POINTER(C.c_uint32), vp]
        L.paffy_hip_keep_raw_sequences.argtypes = [vp, C.c_int]
        L.paffy_hip_stats_only.argtypes = [vp, C.c_int]
        L.paffy_hip_plan_record_stats.restype = i64
        L.paffy_hip_plan_record_stats.argtypes = [vp, i64, C.POINTER(i64)]
        L.paffy_hip_plan_record_layout.argtypes = [vp, i64, i64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.paffy_hip_plan_alignment_sizes.argtypes = [vp, i64, i64, C.POINTER(i64)]
        L.paffy_hip_plan_alignment_rows.argtypes = [vp, i64, i64, C.POINTER(i64), C.c_void_p, C.POINTER(_Error)]
        L.paffy_hip_plan_view_sizes.argtypes = [vp, i64, i64, C.c_int, C.POINTER(i64)]
        L.paffy_hip_plan_view_text.argtypes = [vp, i64, i64, C.c_int, C.POINTER(i64), vp, i64, C.POINTER(_Error)]
        L.paffy_hip_plan_view_layout.argtypes = [vp, C.c_int, i64, C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_plan_view_ranges.restype = i64
        L.paffy_hip_plan_view_ranges.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i64)]
        L.paffy_hip_plan_view_emit_range.argtypes = [vp, i64, vp, i64, C.POINTER(i64), C.POINTER(_Error)]
        L.paffy_hip_stream_open_view.argtypes = [vp, C.c_int, i64, i64, i64, C.POINTER(vp)]
        L.paffy_hip_stream_view_status.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(_Error)]
        _lib = L
    return _lib


def device_buffers():
    """(buffers, bytes) of device memory the library owns in this process right now: contexts, their command states, streams."""
    n, b = C.c_int64(), C.c_int64()
    rc = lib().paffy_hip_device_buffers(C.byref(n), C.byref(b))
    if rc:
        raise RuntimeError(f"paffy_hip_device_buffers failed ({rc})")
    return n.value, b.value


def _pad16(n):
    return (n + 15) // 16 * 16 + 16


class Engine:
    """One HIP context (workspace + stream) on the current torch device."""

    def __init__(self, device=None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("paffy_amd needs a GPU: the hot path has no CPU implementation")
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._ctx = C.c_void_p()
        rc = lib().paffy_hip_create(C.byref(self._ctx), self.device.index)
        if rc:
            raise RuntimeError(f"paffy_hip_create failed ({rc})")
        self.use_stream(torch.cuda.current_stream(self.device))

    def close(self):
        if self._ctx:
            lib().paffy_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def use_stream(self, stream):
        self.stream = stream
        lib().paffy_hip_set_stream(self._ctx, C.c_void_p(stream.cuda_stream))

    def _check(self, rc, what):
        if rc:
            raise RuntimeError(f"{what} failed ({rc}): {lib().paffy_hip_last_error(self._ctx).decode()}")

    def set_filter(self, min_chain_score=-1, min_alignment_score=-1, min_identity=-1.0, min_identity_with_gaps=-1.0, max_tile_level=-1,
                   invert=False):
        """Thresholds used by FILTER stages of later plans (`paffy filter -s -t -u -v -w -x`)."""
        f = Filter(min_chain_score, min_alignment_score, min_identity, min_identity_with_gaps, max_tile_level, 1 if invert else 0)
        self._check(lib().paffy_hip_set_filter(self._ctx, C.byref(f)), "paffy_hip_set_filter")

    # ---- device-buffer level (what bench.py times) ----
    def to_device(self, data):
        """bytes -> padded uint8 device tensor (the library reads up to the next multiple of 16)."""
        t = self.torch
        buf = t.zeros(_pad16(len(data)), dtype=t.uint8, device=self.device)
        if len(data):
            buf[: len(data)] = t.frombuffer(bytearray(data), dtype=t.uint8).to(self.device)
        return buf

    def plan(self, stages, d_in, in_len):
        arr = (Stage * max(1, len(stages)))(*stages)
        info = PlanInfo()
        rc = lib().paffy_hip_plan(self._ctx, arr, len(stages), C.c_void_p(d_in.data_ptr()), in_len, C.byref(info))
        self._check(rc, "paffy_hip_plan")
        return info

    def tile_plan(self, d_in, in_len):
        info = PlanInfo()
        self._check(lib().paffy_hip_tile_plan(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, C.byref(info)), "paffy_hip_tile_plan")
        return info

    def tile_batches(self, bufs):
        """paffy tile over an input held as several device batches [(uint8 tensor, nbytes)], each a whole number of lines and
        below 2 GiB; they must stay alive until the output has been emitted. Returns the PlanInfo."""
        self._check(lib().paffy_hip_tile_begin(self._ctx), "paffy_hip_tile_begin")
        for buf, nbytes in bufs:
            self._check(lib().paffy_hip_tile_add(self._ctx, C.c_void_p(buf.data_ptr()), nbytes), "paffy_hip_tile_add")
        info = PlanInfo()
        self._check(lib().paffy_hip_tile_run(self._ctx, C.byref(info)), "paffy_hip_tile_run")
        return info

    def tile_keys(self, n_lines):
        """After a tile plan: int64 tensor [n_lines, 5] on the device -- chain_score, score, input record, line bytes, tile level
        of every output line, in output order (what the ranks of a sharded tile exchange)."""
        keys = self.torch.empty((max(1, n_lines), 5), dtype=self.torch.int64, device=self.device)
        n = lib().paffy_hip_tile_keys(self._ctx, n_lines, C.c_void_p(keys.data_ptr()))
        if n < 0:
            raise RuntimeError(f"paffy_hip_tile_keys failed ({n})")
        return keys[:n]

    # ---- `paffy tile` sharded by query sequence: the device side of the partition and of the ordered write ----
    def query_names(self, d_in, in_len, cap=1 << 20):
        """Distinct query names of a device batch as ({hash: bytes of its lines}): what the partitioner balances."""
        h, w = (C.c_uint64 * cap)(), (C.c_int64 * cap)()
        n = lib().paffy_hip_query_names(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, cap, h, w)
        if n < 0:
            raise RuntimeError(f"paffy_hip_query_names failed ({n}): {lib().paffy_hip_last_error(self._ctx).decode()}")
        return {int(h[i]): int(w[i]) for i in range(n)}

    def query_names_counts(self, d_in, in_len, cap=1 << 20, sides=None):
        """Distinct query names of a device batch as {hash: (bytes of its lines, number of its lines)}. sides (None, or the
        include_inverted of a to_bed in parts): the names of the counted sides instead (paffy_hip_side_names_counts)."""
        cap0 = 4096  # the usual input has a few dozen sequences; the host arrays are kept and grown on demand
        while True:
            arrs = getattr(self, "_name_arrays", None)
            if arrs is None or len(arrs[0]) < cap0:
                arrs = self._name_arrays = ((C.c_uint64 * cap0)(), (C.c_int64 * cap0)(), (C.c_int64 * cap0)())
            h, w, r = arrs
            if sides is None:
                n = lib().paffy_hip_query_names_counts(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, len(h), h, w, r)
            else:
                n = lib().paffy_hip_side_names_counts(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, int(bool(sides)), len(h), h, w, r)
            if n == -4 and len(h) < cap:  # PAFFY_E_CAPACITY: more names than the arrays hold
                cap0 = min(cap, len(h) * 16)
                continue
            break
        if n < 0:
            raise RuntimeError(f"paffy_hip_query_names_counts failed ({n}): {lib().paffy_hip_last_error(self._ctx).decode()}")
        return {int(h[i]): (int(w[i]), int(r[i])) for i in range(n)}

    def split_by_owner(self, d_in, in_len, n_parts, owner_of):
        """Lines of a device batch regrouped by owner_of[hash of the query name] (input order inside a part). Returns (uint8 tensor,
        bytes per part, records per part, int64 tensor: batch index of every output line)."""
        t = self.torch
        items = sorted(owner_of.items())
        nt = len(items)
        th = (C.c_uint64 * max(1, nt))(*[k for k, _ in items])
        to = (C.c_uint32 * max(1, nt))(*[v for _, v in items])
        out = t.empty(_pad16(in_len + 1), dtype=t.uint8, device=self.device)
        pb, pr, nrec = (C.c_int64 * n_parts)(), (C.c_int64 * n_parts)(), C.c_int64()
        idx = t.empty(max(1, in_len // 24 + 16), dtype=t.int64, device=self.device)  # a PAF line that parses has at least 24 bytes (the call checks the capacity)
        self._check(lib().paffy_hip_split_by_owner(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, n_parts, th, to, nt, C.c_void_p(out.data_ptr()), out.numel(), pb, pr,
                                                   C.c_void_p(idx.data_ptr()), idx.numel(), C.byref(nrec)), "paffy_hip_split_by_owner")
        return out, list(pb), list(pr), idx[: nrec.value]

    def owner_arrays(self, owner_of):
        """{name hash: part} as the two ctypes arrays the split calls take (ascending hashes), built once per partition."""
        items = sorted(owner_of.items())
        nt = len(items)
        return (C.c_uint64 * max(1, nt))(*[k for k, _ in items]), (C.c_uint32 * max(1, nt))(*[v for _, v in items]), nt

    def split_to(self, d_in, in_len, n_parts, owner_arrays, d_out, part_dst, d_rec_index, rec_dst, rec_base):
        """split_by_owner straight into a send buffer: part p's lines go to d_out[part_dst[p]:], the global index (batch index +
        rec_base) of every one of them to d_rec_index[rec_dst[p]:]. Returns (bytes per part, records per part, records of the batch)."""
        th, to, nt = owner_arrays
        pb, pr, nrec = (C.c_int64 * n_parts)(), (C.c_int64 * n_parts)(), C.c_int64()
        pd, rd = (C.c_int64 * n_parts)(*part_dst), (C.c_int64 * n_parts)(*rec_dst)
        self._check(lib().paffy_hip_split_to(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, n_parts, th, to, nt, C.c_void_p(d_out.data_ptr()), d_out.numel(), pd, rd, rec_base,
                                             pb, pr, C.c_void_p(d_rec_index.data_ptr()), d_rec_index.numel(), C.byref(nrec)), "paffy_hip_split_to")
        return list(pb), list(pr), nrec.value

    # ---- to_bed in parts: `paffy to_bed` sharded by sequence (include/paffy_hip.h; shard.to_bed_sharded drives these) ----
    def side_names_counts(self, d_in, in_len, include_inverted, cap=1 << 20):
        """{hash: (bytes, lines)} of the names a device batch counts on: its query names and, with include_inverted, its target names."""
        return self.query_names_counts(d_in, in_len, cap, sides=bool(include_inverted))

    def split_sides_count(self, d_in, in_len, include_inverted, n_parts, owner_arrays):
        """(bytes per part, lines per part, records of the batch) split_sides_to would write: a line whose two names share an owner is
        sent once, so these are not sums over names. Nothing is written, the batch's kept index stays."""
        th, to, nt = owner_arrays
        pb, pr, nrec = (C.c_int64 * n_parts)(), (C.c_int64 * n_parts)(), C.c_int64()
        self._check(lib().paffy_hip_split_sides_count(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, int(bool(include_inverted)), n_parts, th, to, nt, pb, pr, C.byref(nrec)),
                    "paffy_hip_split_sides_count")
        return list(pb), list(pr), nrec.value

    def split_sides_to(self, d_in, in_len, include_inverted, n_parts, owner_arrays, d_out, part_dst, d_rec_index, d_sides, rec_dst, rec_base):
        """split_to by the names of both sides: part p's lines to d_out[part_dst[p]:], the global index of every one of them to
        d_rec_index[rec_dst[p]:] (int64) and its side mask to d_sides[rec_dst[p]:] (uint8). Returns (bytes per part, lines per part,
        records of the batch)."""
        th, to, nt = owner_arrays
        pb, pr, nrec = (C.c_int64 * n_parts)(), (C.c_int64 * n_parts)(), C.c_int64()
        pd, rd = (C.c_int64 * n_parts)(*part_dst), (C.c_int64 * n_parts)(*rec_dst)
        self._check(lib().paffy_hip_split_sides_to(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, int(bool(include_inverted)), n_parts, th, to, nt, C.c_void_p(d_out.data_ptr()),
                                                   d_out.numel(), pd, rd, rec_base, pb, pr, C.c_void_p(d_rec_index.data_ptr()), C.c_void_p(d_sides.data_ptr()),
                                                   min(d_rec_index.numel(), d_sides.numel()), C.byref(nrec)), "paffy_hip_split_sides_to")
        return list(pb), list(pr), nrec.value

    def bed_part(self, bufs, sides=None, binary=False, exclude_unaligned=False, exclude_aligned=False, min_size=1, include_inverted=False):
        """begin, add every device batch [(uint8 tensor, nbytes)] -- with sides[b], a uint8 device tensor holding the side mask of every
        line of batch b, where given (None: every side) -- and run. Returns the PlanInfo (error.record counts the lines added)."""
        L = lib()
        opts = BedOpts(int(binary), int(exclude_unaligned), int(exclude_aligned), int(include_inverted), min_size)
        self._check(L.paffy_hip_bed_begin(self._ctx, C.byref(opts)), "paffy_hip_bed_begin")
        for b, (buf, nbytes) in enumerate(bufs):
            m = sides[b] if sides is not None else None
            if m is not None and (m.dtype != self.torch.uint8 or not m.is_contiguous() or m.device != self.device):
                raise ValueError("the side masks of a batch: a contiguous uint8 tensor on the engine's device")
            self._check(L.paffy_hip_bed_add_sides(self._ctx, C.c_void_p(buf.data_ptr()), nbytes, C.c_void_p(m.data_ptr()) if m is not None and m.numel() else None),
                        "paffy_hip_bed_add_sides")
        info = PlanInfo()
        self._check(L.paffy_hip_bed_run(self._ctx, C.byref(opts), C.byref(info)), "paffy_hip_bed_run")
        return info

    def bed_failure_side(self):
        """After a bed run that failed: 0 = on the record's query side, 1 = on its target side, -1 = the line did not parse."""
        return int(lib().paffy_hip_bed_failure_side(self._ctx))

    def bed_sequence_keys(self):
        """After a bed run: int64 device tensor [sequences, 3] -- the local entry (2 * record + side) a sequence first appeared with, the
        bytes of its block of BED lines, its number of lines -- in the run's order of first appearance (the order of the output)."""
        n = lib().paffy_hip_bed_sequences(self._ctx)
        if n < 0:
            self._check(int(n), "paffy_hip_bed_sequences")
        keys = self.torch.empty((max(1, n), 3), dtype=self.torch.int64, device=self.device)
        got = lib().paffy_hip_bed_sequence_keys(self._ctx, n, C.c_void_p(keys.data_ptr()))
        if got < 0:
            self._check(int(got), "paffy_hip_bed_sequence_keys")
        return keys[:got]

    def drop_index(self, d_in=None):
        """Forget the line index query_names kept for a batch that will not be split (None: for every batch)."""
        lib().paffy_hip_drop_index(self._ctx, C.c_void_p(d_in.data_ptr()) if d_in is not None else None)

    def scatter_lines(self, d_src, src_off, dst_off, d_dst):
        """Line k = d_src[src_off[k] : src_off[k + 1]] to d_dst[dst_off[k]:] (int64 device tensors)."""
        n = dst_off.numel()
        self._check(lib().paffy_hip_scatter_lines(self._ctx, C.c_void_p(d_src.data_ptr()), C.c_void_p(src_off.data_ptr()), C.c_void_p(dst_off.data_ptr()), n,
                                                  C.c_void_p(d_dst.data_ptr())), "paffy_hip_scatter_lines")

    def emit_lines(self, first, n, d_out):
        """Lines [first, first + n) of a tile / dedupe plan into d_out (from its first byte); returns the bytes written."""
        nbytes = C.c_int64()
        self._check(lib().paffy_hip_emit_lines(self._ctx, first, n, C.c_void_p(d_out.data_ptr()), d_out.numel(), C.byref(nbytes)), "paffy_hip_emit_lines")
        return nbytes.value

    def split_lines(self, data, max_bytes):
        """Cut PAF text into pieces of at most max_bytes that end on line boundaries (one line may exceed it)."""
        out, at = [], 0
        while at < len(data):
            end = min(len(data), at + max_bytes)
            if end < len(data):
                nl = data.rfind(b"\n", at, end)
                end = nl + 1 if nl >= at else (data.find(b"\n", end) + 1 or len(data))
            out.append(data[at:end])
            at = end
        return out

    def tile(self, data, raise_on_error=True, batch_bytes=None):
        """paffy tile (impl/paf_tile.c) over PAF text; returns (output bytes, PlanInfo). With batch_bytes the text goes to the
        device in pieces of at most that size (inputs of 2 GiB and more must)."""
        if batch_bytes:
            bufs = [(self.to_device(p), len(p)) for p in self.split_lines(data, batch_bytes)]
            info = self.tile_batches(bufs)
        else:
            d_in = self.to_device(data)
            info = self.tile_plan(d_in, len(data))
        out = b""
        if info.out_bytes:
            d_out = self.alloc_out(info.out_bytes)
            self.emit(d_out)
            self.sync()
            out = bytes(d_out[: info.out_bytes].cpu().numpy().tobytes())
        if info.error.code and raise_on_error:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        return out, info

    def chain_fresh_walk(self, on=True):
        """The reference's walk from a fresh iterator (impl/chaining.c:71-86): an alignment that abuts a record exactly on both sequences
        but stands later in the input is chained after all. Sticky, off by default; chain_part refuses while it is on."""
        self._check(lib().paffy_hip_chain_fresh_walk(self._ctx, 1 if on else 0), "paffy_hip_chain_fresh_walk")

    def chain_fresh_stats(self):
        """Of the last chain run: [records of leading runs the flag kernel processed (0: not launched), flagged fresh, links of the
        result only the fresh walk gives, such candidates the first recurrence skipped]."""
        out = (C.c_int64 * 4)()
        self._check(lib().paffy_hip_chain_fresh_stats(self._ctx, out), "paffy_hip_chain_fresh_stats")
        return list(out)

    def chain(self, data, gap_open=5000, gap_extend=1, max_gap=1000000, trim=1.0, raise_on_error=True, batch_bytes=None, fresh_walk=False):
        """paffy chain (impl/paf_chain.c, impl/chaining.c) over PAF text; returns (output bytes, PlanInfo). The keyword defaults are
        the command's (-d, -e, -g, -t). fresh_walk: this run with the switch of chain_fresh_walk on (and off again afterwards)."""
        if fresh_walk:
            self.chain_fresh_walk(True)
            try:
                return self.chain(data, gap_open, gap_extend, max_gap, trim, raise_on_error, batch_bytes)
            finally:
                self.chain_fresh_walk(False)
        pieces = self.split_lines(data, batch_bytes) if batch_bytes else [data]
        bufs = [(self.to_device(p), len(p)) for p in pieces if len(p)]
        self._check(lib().paffy_hip_chain_begin(self._ctx), "paffy_hip_chain_begin")
        for buf, nbytes in bufs:
            self._check(lib().paffy_hip_chain_add(self._ctx, C.c_void_p(buf.data_ptr()), nbytes), "paffy_hip_chain_add")
        info, opts = PlanInfo(), ChainOpts(gap_open, gap_extend, max_gap, trim)
        self._check(lib().paffy_hip_chain_run(self._ctx, C.byref(opts), C.byref(info)), "paffy_hip_chain_run")
        out = b""
        if info.out_bytes and not info.error.code:
            d_out = self.alloc_out(info.out_bytes)
            self.emit(d_out)
            self.sync()
            out = bytes(d_out[: info.out_bytes].cpu().numpy().tobytes())
        del bufs  # the batches had to stay in place until the lines were written
        if info.error.code and raise_on_error:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        return out, info

    def chain_tags(self, n):
        """(chain ids, chain scores) of the n output lines of the last chain run."""
        ids, scores = (C.c_int64 * max(n, 1))(), (C.c_int64 * max(n, 1))()
        got = lib().paffy_hip_chain_tags(self._ctx, n, ids, scores)
        if got < 0:
            self._check(int(got), "paffy_hip_chain_tags")
        return list(ids[:got]), list(scores[:got])

    # ---- chain in parts: `paffy chain` sharded by query sequence (include/paffy_hip.h; shard.chain_sharded drives these) ----
    def chain_part(self, bufs, gidx=None, gap_open=5000, gap_extend=1, max_gap=1000000, trim=1.0):
        """begin, add every device batch [(uint8 tensor, nbytes)] -- with gidx[b], an int64 device tensor holding the global input
        record number of every line of batch b, where given -- and run the part: everything up to the cut of the chains. The batches
        must stay alive until the lines have been written. Returns the PlanInfo (error.record is a global record number)."""
        L = lib()
        self._check(L.paffy_hip_chain_begin(self._ctx), "paffy_hip_chain_begin")
        for b, (buf, nbytes) in enumerate(bufs):
            g = gidx[b] if gidx is not None else None
            if g is None:
                self._check(L.paffy_hip_chain_add(self._ctx, C.c_void_p(buf.data_ptr()), nbytes), "paffy_hip_chain_add")
            else:
                if g.dtype != self.torch.int64 or not g.is_contiguous() or g.device != self.device:
                    raise ValueError("the global record numbers of a batch: a contiguous int64 tensor on the engine's device")
                self._check(L.paffy_hip_chain_add_indexed(self._ctx, C.c_void_p(buf.data_ptr()), nbytes, C.c_void_p(g.data_ptr())), "paffy_hip_chain_add_indexed")
        info, opts = PlanInfo(), ChainOpts(gap_open, gap_extend, max_gap, trim)
        self._check(L.paffy_hip_chain_run_part(self._ctx, C.byref(opts), C.byref(info)), "paffy_hip_chain_run_part")
        return info

    def chain_tail_keys(self, cap_chains):
        """After chain_part: int64 device tensor [chains, 4] -- strand class, chain-end score, processing key, global record number of
        the chain end -- in the part's chain order. cap_chains: an upper bound (the part's records will do)."""
        keys = self.torch.empty((max(1, cap_chains), 4), dtype=self.torch.int64, device=self.device)
        n = lib().paffy_hip_chain_tail_keys(self._ctx, cap_chains, C.c_void_p(keys.data_ptr()))
        if n < 0:
            self._check(int(n), "paffy_hip_chain_tail_keys")
        return keys[:n]

    def chain_renumber(self, global_ids):
        """global_ids: int64 device tensor, the number of every chain of the part in the whole input (the order of chain_tail_keys).
        Finishes the run. Returns (PlanInfo, None), or with a failed paf_check (PlanInfo, (own score, chain id, link) of that line)."""
        g = global_ids.to(device=self.device, dtype=self.torch.int64).contiguous()
        info, fail = PlanInfo(), (C.c_int64 * 3)()
        self._check(lib().paffy_hip_chain_renumber(self._ctx, C.c_void_p(g.data_ptr()) if g.numel() else None, C.byref(info), fail), "paffy_hip_chain_renumber")
        return info, (tuple(fail) if info.error.code else None)

    def chain_line_keys(self, n_lines):
        """After chain_renumber (or a chain run): int64 device tensor [n_lines, 4] -- own score, chain id, link, bytes -- of every output
        line, in output order."""
        keys = self.torch.empty((max(1, n_lines), 4), dtype=self.torch.int64, device=self.device)
        n = lib().paffy_hip_chain_line_keys(self._ctx, n_lines, C.c_void_p(keys.data_ptr()))
        if n < 0:
            self._check(int(n), "paffy_hip_chain_line_keys")
        return keys[:n]

    def plan_rows(self, n_lines):
        """(input record, first output byte) of every line emit will write, and the total, after a tile / chain / dedupe plan."""
        rec, off = (C.c_uint32 * (n_lines + 1))(), (C.c_int64 * (n_lines + 1))()
        n = lib().paffy_hip_plan_rows(self._ctx, n_lines + 1, rec, off)
        if n < 0:
            self._check(int(n), "paffy_hip_plan_rows")
        return list(rec[:n]), list(off[: n + 1])

    def dedupe_plan(self, d_in, in_len, check_inverse=False):
        info = PlanInfo()
        self._check(lib().paffy_hip_dedupe_plan(self._ctx, C.c_void_p(d_in.data_ptr()), in_len, 1 if check_inverse else 0, C.byref(info)),
                    "paffy_hip_dedupe_plan")
        return info

    def dedupe(self, data, check_inverse=False, reset=True, raise_on_error=True):
        """paffy dedupe [-a] (impl/paf_dedupe.c) over PAF text; with reset=False the records written by earlier calls count too."""
        if reset:
            lib().paffy_hip_dedupe_reset(self._ctx)
        d_in = self.to_device(data)
        info = self.dedupe_plan(d_in, len(data), check_inverse)
        out = b""
        if info.out_bytes:
            d_out = self.alloc_out(info.out_bytes)
            self.emit(d_out)
            self.sync()
            out = bytes(d_out[: info.out_bytes].cpu().numpy().tobytes())
        if info.error.code and raise_on_error:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        return out, info

    # ---- paffy split_file: the lines of a batch grouped by output file (include/paffy_hip.h) ----
    def split_begin(self, by_query=False, min_length=0):
        """Starts a split_file run on this context and forgets the files of an earlier one."""
        self._check(lib().paffy_hip_split_begin(self._ctx, 1 if by_query else 0, int(min_length)), "paffy_hip_split_begin")

    def split_plan(self, d_in, in_len):
        """Plans the grouped lines of a device batch; emit follows, split_groups says which stretch of the output is whose."""
        info = PlanInfo()
        self._check(lib().paffy_hip_split_plan(self._ctx, C.c_void_p(d_in.data_ptr()) if in_len else None, in_len, C.byref(info)), "paffy_hip_split_plan")
        return info

    def split_groups(self):
        """The stretches of the last split plan in output order, one per file that gets lines of the batch (SplitGroup: file, out_off, bytes,
        lines, first_record, new_file, is_small)."""
        L = lib()
        cap = 256
        while True:
            buf = (SplitGroup * cap)()
            n = L.paffy_hip_split_groups(self._ctx, cap, buf)
            if n == -4:  # PAFFY_E_CAPACITY
                cap *= 8
                continue
            if n < 0:
                self._check(int(n), "paffy_hip_split_groups")
            return list(buf[:n])

    def split_file_name(self, file):
        """Name of a file of the run without prefix and ".paf" (bytes): the contig name with '/' as '_', or small_<k>."""
        L = lib()
        cap = 256
        while True:
            buf = C.create_string_buffer(cap)
            n = L.paffy_hip_split_file_name(self._ctx, file, buf, cap)
            if n == -4:  # PAFFY_E_CAPACITY
                cap *= 8
                continue
            if n < 0:
                self._check(int(n), "paffy_hip_split_file_name")
            return buf.raw[:n]

    def split_salt(self):
        """Salt of the name hash the last split plan's grouping passed its byte check with (0 unless names collided)."""
        n = lib().paffy_hip_split_salt(self._ctx)
        if n < 0:
            self._check(int(n), "paffy_hip_split_salt")
        return n

    def split_file(self, data, by_query=False, min_length=0, batch_bytes=None, raise_on_error=True):
        """paffy split_file [-q] [-m min_length] (impl/paf_split_file.c) over PAF text; returns ({file name without prefix and ".paf"
        (str): its bytes}, in opening order, PlanInfo of the last batch). With batch_bytes the text goes to the device in pieces of at most that
        size; the files carry on from piece to piece. A failing record ends the run behind the records in front of it."""
        self.split_begin(by_query, min_length)
        files, names = {}, {}
        info = PlanInfo()
        done = 0
        for piece in (self.split_lines(data, batch_bytes) if batch_bytes else [data]):
            d_in = self.to_device(piece)
            info = self.split_plan(d_in, len(piece))
            out = b""
            if info.out_bytes:
                d_out = self.alloc_out(info.out_bytes)
                self.emit(d_out)
                self.sync()
                out = d_out[: info.out_bytes].cpu().numpy().tobytes()
            for g in self.split_groups():
                if g.new_file:
                    names[g.file] = os.fsdecode(self.split_file_name(g.file))  # as os.listdir would name the file
                    files.setdefault(names[g.file], [])
                files[names[g.file]].append(out[g.out_off : g.out_off + g.bytes])
            if info.error.code:
                info.error.record += done  # counted over the whole text
                break
            done += info.n_records
        files = {k: b"".join(v) for k, v in files.items()}
        if info.error.code and raise_on_error:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        return files, info

    # ---- dedupe in parts: `paffy dedupe` sharded by key owner (include/paffy_hip.h; shard.dedupe_sharded drives these) ----
    def dedupe_reset(self):
        self._check(lib().paffy_hip_dedupe_reset(self._ctx), "paffy_hip_dedupe_reset")

    def dedupe_part_keys(self, d_in, in_len, check_inverse, rec_base, n_parts, entries=None):
        """The round's entries of a device batch, grouped by owner: (int64 device tensor [n, 4] -- class hi, class lo, global number,
        flags --, entries per owner, records of the batch). entries: a tensor to write into (its rows are the capacity); by default one
        row per line end of the batch, plus one. The batch must stay alive until the round's lines have been written."""
        t = self.torch
        if entries is None:
            entries = t.empty((int((d_in[:in_len] == 10).sum().item()) + 1 if in_len else 1, 4), dtype=t.int64, device=self.device)
        counts, n_rec = (C.c_int64 * n_parts)(), C.c_int64()
        self._check(lib().paffy_hip_dedupe_part_keys(self._ctx, C.c_void_p(d_in.data_ptr()) if in_len else None, in_len, 1 if check_inverse else 0, rec_base, n_parts,
                                                     C.c_void_p(entries.data_ptr()), entries.shape[0], counts, C.byref(n_rec)), "paffy_hip_dedupe_part_keys")
        counts = list(counts)
        return entries[: sum(counts)], counts, n_rec.value

    def dedupe_part_decide(self, entries, check_inverse):
        """Owner side: one verdict byte per entry (uint8 device tensor; bit 0 written, bit 1 fails), in the entries' order."""
        t = self.torch
        e = entries.to(device=self.device, dtype=t.int64).contiguous()
        n = e.shape[0] if e.dim() == 2 else e.numel() // 4
        v = t.zeros(max(16, n), dtype=t.uint8, device=self.device)
        self._check(lib().paffy_hip_dedupe_part_decide(self._ctx, C.c_void_p(e.data_ptr()) if n else None, n, 1 if check_inverse else 0, C.c_void_p(v.data_ptr())),
                    "paffy_hip_dedupe_part_decide")
        return v[:n]

    def dedupe_part_verdicts(self, verdicts):
        """Source side: the verdict bytes of this part's entries, in the order dedupe_part_keys wrote them. Returns the lowest failing
        global record of this part, or -1."""
        v = verdicts.to(device=self.device, dtype=self.torch.uint8).contiguous()
        bad = C.c_int64(-1)
        self._check(lib().paffy_hip_dedupe_part_verdicts(self._ctx, C.c_void_p(v.data_ptr()) if v.numel() else None, v.numel(), C.byref(bad)), "paffy_hip_dedupe_part_verdicts")
        return bad.value

    def dedupe_part_plan(self, first_bad_global=-1):
        """Source side: plans this part's lines in front of first_bad_global (-1: no failure anywhere). Returns the PlanInfo; emit follows."""
        info = PlanInfo()
        self._check(lib().paffy_hip_dedupe_part_plan(self._ctx, first_bad_global, C.byref(info)), "paffy_hip_dedupe_part_plan")
        return info

    def emit(self, d_out):
        rc = lib().paffy_hip_emit(self._ctx, C.c_void_p(d_out.data_ptr()), d_out.numel())
        self._check(rc, "paffy_hip_emit")

    def set_sequences(self, seqs):
        """FASTA sequences for add_mismatches: {header: bases}, as `paffy add_mismatches a.fa b.fa` would load them."""
        names = [k if isinstance(k, bytes) else k.encode() for k in seqs]
        vals = [v if isinstance(v, bytes) else v.encode() for v in seqs.values()]
        n = len(names)
        a = (C.c_char_p * max(1, n))(*names)
        b = (C.c_char_p * max(1, n))(*vals)
        ln = (C.c_int64 * max(1, n))(*[len(v) for v in vals])
        self._check(lib().paffy_hip_set_sequences(self._ctx, n, a, b, ln), "paffy_hip_set_sequences")

    def set_intervals(self, headers, seq_lens):
        """Intervals for UPCONVERT: the FASTA headers ("name|length|start") of extracted subsequences and the lengths of their sequences,
        as `paffy upconvert a.fa b.fa` loads them. A header that does not decode raises (the reference aborts)."""
        hs = [h if isinstance(h, bytes) else h.encode() for h in headers]
        n = len(hs)
        if len(seq_lens) != n:
            raise ValueError("one sequence length per header")
        a = (C.c_char_p * max(1, n))(*hs)
        ln = (C.c_int64 * max(1, n))(*[int(x) for x in seq_lens])
        self._check(lib().paffy_hip_set_intervals(self._ctx, a, ln, n), "paffy_hip_set_intervals")

    def sync(self):
        self._check(lib().paffy_hip_sync(self._ctx), "paffy_hip_sync")

    def alloc_out(self, nbytes):
        return self.torch.empty(_pad16(nbytes), dtype=self.torch.uint8, device=self.device)

    # ---- bytes level (tests, small inputs) ----
    def run(self, stages, data, raise_on_error=True):
        """Apply a pipe of commands to PAF text; returns (output bytes, PlanInfo)."""
        d_in = self.to_device(data)
        info = self.plan(stages, d_in, len(data))
        out = b""
        if info.out_bytes:
            d_out = self.alloc_out(info.out_bytes)
            self.emit(d_out)
            self.sync()
            out = bytes(d_out[: info.out_bytes].cpu().numpy().tobytes())
        if info.error.code and raise_on_error:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        return out, info

    def run_chain(self, stages, data):
        """Run the commands one by one over text, as separate `paffy` processes in a shell pipe would."""
        for st in stages:
            data, _ = self.run([st], data)
        return data

    def synth(self, seed, mean_ops, r0, n, n_contigs=24):
        """Synthetic PAF records [r0, r0+n) generated on the device; returns (tensor, nbytes)."""
        nbytes = C.c_int64()
        self._check(lib().paffy_hip_synth_contigs(self._ctx, seed, mean_ops, n_contigs, r0, n, None, 0, C.byref(nbytes)), "paffy_hip_synth(size)")
        buf = self.torch.zeros(_pad16(nbytes.value), dtype=self.torch.uint8, device=self.device)
        self._check(lib().paffy_hip_synth_contigs(self._ctx, seed, mean_ops, n_contigs, r0, n, C.c_void_p(buf.data_ptr()), buf.numel(), C.byref(nbytes)),
                    "paffy_hip_synth(fill)")
        return buf, nbytes.value

    def to_bed(self, data, binary=False, exclude_unaligned=False, exclude_aligned=False, min_size=1, include_inverted=False, raise_on_error=True,
               batch_bytes=None):
        """paffy to_bed [-b -e -f -m -n] (impl/paf_to_bed.c) over PAF text; returns (BED bytes, PlanInfo). With batch_bytes the text
        goes to the device in pieces of at most that size."""
        info = PlanInfo()
        opts = BedOpts(int(binary), int(exclude_unaligned), int(exclude_aligned), int(include_inverted), min_size)
        if batch_bytes:
            bufs = [(self.to_device(p), len(p)) for p in self.split_lines(data, batch_bytes)]
            self._check(lib().paffy_hip_bed_begin(self._ctx, C.byref(opts)), "paffy_hip_bed_begin")
            for buf, nbytes in bufs:
                self._check(lib().paffy_hip_bed_add(self._ctx, C.c_void_p(buf.data_ptr()), nbytes), "paffy_hip_bed_add")
            self._check(lib().paffy_hip_bed_run(self._ctx, C.byref(opts), C.byref(info)), "paffy_hip_bed_run")
        else:
            d_in = self.to_device(data)
            self._check(lib().paffy_hip_bed_plan(self._ctx, C.c_void_p(d_in.data_ptr()), len(data), C.byref(opts), C.byref(info)), "paffy_hip_bed_plan")
        out = b""
        if info.out_bytes:
            d_out = self.alloc_out(info.out_bytes)
            self.emit(d_out)
            self.sync()
            out = bytes(d_out[: info.out_bytes].cpu().numpy().tobytes())
        if info.error.code and raise_on_error:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        return out, info

    def flat_stats(self):
        """(records the flat sizing pass left to the record kernels in the last plan, or -1 when the plan did not take it; counts per reason:
        FLAT_WHY_* of csrc/flat_kernel.h, e.g. FLAT_WHY_ENCODER)"""
        left, why = C.c_int64(), (C.c_int64 * 16)()
        self._check(lib().paffy_hip_flat_stats(self._ctx, C.byref(left), why), "paffy_hip_flat_stats")
        return left.value, list(why)

    def plan_stats(self):
        """Sums of the STATS stage of the last plan (the last one, should a pipe hold several): (matches, mismatches, inserts, deletes, insert bases, delete bases)."""
        out = (C.c_int64 * 6)()
        self._check(lib().paffy_hip_plan_stats(self._ctx, out), "paffy_hip_plan_stats")
        return tuple(out)

    def record_stats(self, n):
        """The six sums of plan_stats for each of the n records of the last plan (a STATS stage in it): a list of 6-tuples, the numbers of
        the per-alignment line of `paffy view`."""
        out = (C.c_int64 * (6 * max(1, n)))()
        got = lib().paffy_hip_plan_record_stats(self._ctx, n, out)
        if got < 0:
            self._check(int(got), "paffy_hip_plan_record_stats")
        return [tuple(out[6 * i:6 * i + 6]) for i in range(got)]

    def stats_only(self, on=True):
        """Sums only (`paffy view` without base-level rows): later plans of [ADD_MISMATCHES, STATS] count the matching columns on the
        pieces of the flat pass and build nothing else -- plan_stats and record_stats answer, emit and the row getters raise. Sticky;
        every other stage list plans as without it."""
        self._check(lib().paffy_hip_stats_only(self._ctx, 1 if on else 0), "paffy_hip_stats_only")

    def record_layout(self, first, count):
        """(RecPlan flags, classes) of records [first, first + count) of the last plan: how each record's ops are kept (diagnostics, as
        flat_stats: the tests use it to know which representation was read)."""
        flags, klass = (C.c_uint32 * max(1, count))(), (C.c_uint32 * max(1, count))()
        self._check(lib().paffy_hip_plan_record_layout(self._ctx, first, count, flags, klass), "paffy_hip_plan_record_layout")
        return list(flags[:count]), list(klass[:count])

    def alignment_sizes(self, first, count):
        """Bytes of the base-level rows (`paffy view -a`) of records [first, first + count) of the last plan."""
        out = (C.c_int64 * max(1, count))()
        self._check(lib().paffy_hip_plan_alignment_sizes(self._ctx, first, count, out), "paffy_hip_plan_alignment_sizes")
        return list(out[:count])

    def alignment_rows(self, first, count, offsets=None, guard=0):
        """The rows of records [first, first + count) of the last plan, block after block: (bytes, error), error = None or (code, record)
        with the record's index in the planned batch. offsets: count + 1 running sums of the sizes (default: built from
        alignment_sizes); only their differences count, so the slice of a whole batch's offsets fetches a piece of it. guard: that
        many bytes of 0xA5 are kept behind the host buffer and returned with the rows (the tests check that nothing wrote there)."""
        if offsets is None:
            offsets = [0]
            for b in self.alignment_sizes(first, count):
                offsets.append(offsets[-1] + b)
        if len(offsets) != count + 1:
            raise ValueError("count + 1 offsets")
        off = (C.c_int64 * (count + 1))(*offsets)
        total = offsets[count] - offsets[0]
        buf = (C.c_ubyte * (max(0, total) + guard + 1))()
        C.memset(C.addressof(buf) + max(0, total), 0xA5, guard)
        err = _Error()
        self._check(lib().paffy_hip_plan_alignment_rows(self._ctx, first, count, off, C.cast(buf, C.c_void_p), C.byref(err)), "paffy_hip_plan_alignment_rows")
        return bytes(buf[: total + guard]), ((err.code, err.record) if err.code else None)

    def view_sizes(self, first, count, with_rows=False):
        """Bytes of what `paffy view` writes for each of records [first, first + count) of the last plan (a STATS stage in it): the stats
        line of paf_pretty_print and, with_rows, the base-level rows behind it."""
        out = (C.c_int64 * max(1, count))()
        self._check(lib().paffy_hip_plan_view_sizes(self._ctx, first, count, 1 if with_rows else 0, out), "paffy_hip_plan_view_sizes")
        return list(out[:count])

    def view_text(self, first, count, with_rows=False, offsets=None, guard=0, out_cap=None):
        """That text, written on the device (paffy_hip_plan_view_text) and copied back: bytes. offsets: count + 1 running sums of the sizes
        (default: built from view_sizes); only their differences count. guard: the destination lies between that many bytes of 0xA5 on
        either side, and the call asserts that they are intact afterwards. out_cap: the capacity the library is told (default: the
        text's bytes). A failing record of the rows raises PafError with the record's index in the planned batch."""
        t = self.torch
        if offsets is None:
            offsets = [0]
            for b in self.view_sizes(first, count, with_rows):
                offsets.append(offsets[-1] + b)
        if len(offsets) != count + 1:
            raise ValueError("count + 1 offsets")
        off = (C.c_int64 * (count + 1))(*offsets)
        total = max(0, offsets[count] - offsets[0])
        lead = (guard + 15) // 16 * 16  # the destination itself need not be aligned; its front guard ends right at it
        buf = t.full((lead + total + guard + 16,), 0xA5, dtype=t.uint8, device=self.device)
        err = _Error()
        rc = lib().paffy_hip_plan_view_text(self._ctx, first, count, 1 if with_rows else 0, off, C.c_void_p(buf.data_ptr() + lead),
                                            total if out_cap is None else out_cap, C.byref(err))
        self._check(rc, "paffy_hip_plan_view_text")
        host = buf.cpu().numpy().tobytes()
        assert host[:lead] == b"\xa5" * lead and host[lead + total:] == b"\xa5" * (guard + 16), "paffy_hip_plan_view_text wrote outside its destination"
        if err.code:
            L = lib()
            raise PafError(f"record {err.record}: {L.paffy_hip_error_string(err.code).decode()}", err, L.paffy_hip_error_exit_status(err.code))
        return host[lead:lead + total]

    def synth4_setup(self, seed, mean_ops, n_contigs=24, tlen_min=50_000_000, tlen_span=200_000_000, genomes=True):
        """cfg4 workload: master alignments of n_contigs contig pairs and, with `genomes`, both genomes
        written into the sequence store of this engine (what set_sequences would hold)."""
        self._check(lib().paffy_hip_synth4_setup(self._ctx, seed, mean_ops, n_contigs, tlen_min, tlen_span, 1 if genomes else 0),
                    "paffy_hip_synth4_setup")

    def synth4(self, r0, n):
        """cfg4 records [r0, r0+n) generated on the device; returns (tensor, nbytes)."""
        nbytes = C.c_int64()
        self._check(lib().paffy_hip_synth4(self._ctx, r0, n, None, 0, C.byref(nbytes)), "paffy_hip_synth4(size)")
        buf = self.torch.zeros(_pad16(nbytes.value), dtype=self.torch.uint8, device=self.device)
        self._check(lib().paffy_hip_synth4(self._ctx, r0, n, C.c_void_p(buf.data_ptr()), buf.numel(), C.byref(nbytes)), "paffy_hip_synth4(fill)")
        return buf, nbytes.value

    # ---- host buffers in, host buffers out: the streaming runtime of the CLI ----
    def stream_host(self, stages, chunks, sink=None):
        """Push host chunks (bytes objects of whole lines) through paffy_hip_stream_*: pinned staging, H2D / kernels / D2H
        overlapped. sink(piece_bytes) gets the output pieces in order (default: they are only counted). Returns (records, output bytes)."""
        import time

        L = lib()
        arr = (Stage * max(1, len(stages)))(*stages)
        st = C.c_void_p()
        cap0 = max(4096, max((len(c) for c in chunks), default=4096))
        t_open = time.perf_counter()
        self._check(L.paffy_hip_stream_open(self._ctx, arr, len(stages), cap0, getattr(self, "stream_piece_bytes", 64 << 20), C.byref(st)), "paffy_hip_stream_open")
        # where the time of the call went: opening the stream pins its host buffers (two input slots, three output pieces) and allocates the
        # device buffers -- once per process in the CLI, and seconds on some hosts; the host's copy of a chunk into its pinned slot
        self.stream_seconds = {"open": time.perf_counter() - t_open, "input_copy": 0.0, "run": 0.0, "close": 0.0}
        t_run = time.perf_counter()
        records = out_bytes = 0

        def drain():
            nonlocal out_bytes
            while True:
                piece, n = C.c_void_p(), C.c_int64()
                self._check(L.paffy_hip_stream_read(st, C.byref(piece), C.byref(n)), "paffy_hip_stream_read")
                if n.value == 0:
                    return
                out_bytes += n.value
                if sink:
                    sink(C.string_at(piece.value, n.value))

        try:
            pending = False
            for chunk in chunks:
                cap = C.c_int64()
                buf = L.paffy_hip_stream_input(st, len(chunk), 0, C.byref(cap))
                if not buf:
                    raise RuntimeError("paffy_hip_stream_input: no free slot")
                t_in = time.perf_counter()
                C.memmove(buf, chunk, len(chunk))
                self.stream_seconds["input_copy"] += time.perf_counter() - t_in
                info = PlanInfo()
                self._check(L.paffy_hip_stream_submit(st, len(chunk), C.byref(info)), "paffy_hip_stream_submit")
                if info.error.code:
                    raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info, L.paffy_hip_error_exit_status(info.error.code))
                records += info.n_records
                if pending:
                    drain()  # the chunk before, while the GPU works on this one
                pending = True
            if pending:
                drain()
            self.stream_seconds["run"] = time.perf_counter() - t_run
        finally:
            t_close = time.perf_counter()
            L.paffy_hip_stream_close(st)
            self.stream_seconds["close"] = time.perf_counter() - t_close
        return records, out_bytes

    # ---- `paffy view` as a stream: the layout of every chunk's text stays on the device ----
    def view_layout(self, with_rows=False, range_bytes=128 << 20):
        """Lay out the view text of the last plan on the device (paffy_hip_plan_view_layout): (total bytes, ranges), ranges being the
        n_ranges + 1 pairs (first record, first byte), the last one (n_records, total)."""
        L = lib()
        total, nr = C.c_int64(), C.c_int64()
        self._check(L.paffy_hip_plan_view_layout(self._ctx, 1 if with_rows else 0, range_bytes, C.byref(total), C.byref(nr)), "paffy_hip_plan_view_layout")
        rec, byte = (C.c_int64 * (nr.value + 1))(), (C.c_int64 * (nr.value + 1))()
        got = L.paffy_hip_plan_view_ranges(self._ctx, nr.value + 1, rec, byte)
        if got != nr.value:
            raise RuntimeError(f"paffy_hip_plan_view_ranges: {got} for {nr.value} ranges")
        return total.value, list(zip(rec, byte))

    def view_emit_range(self, rng, nbytes, guard=0, out_cap=None):
        """Range `rng` of that layout, written on the device and copied back: (bytes, None) or, when the rows of a record fail, (what the
        reference had printed of the range by then, (code, record in the batch)). nbytes: the range's bytes; guard as in view_text."""
        t = self.torch
        lead = (guard + 15) // 16 * 16
        buf = t.full((lead + nbytes + guard + 16,), 0xA5, dtype=t.uint8, device=self.device)
        err, n = _Error(), C.c_int64()
        rc = lib().paffy_hip_plan_view_emit_range(self._ctx, rng, C.c_void_p(buf.data_ptr() + lead), nbytes if out_cap is None else out_cap, C.byref(n), C.byref(err))
        self._check(rc, "paffy_hip_plan_view_emit_range")
        host = buf.cpu().numpy().tobytes()
        assert host[:lead] == b"\xa5" * lead and host[lead + nbytes:] == b"\xa5" * (guard + 16), "paffy_hip_plan_view_emit_range wrote outside its destination"
        return host[lead:lead + n.value], ((err.code, err.record) if err.code else None)

    def open_view_stream(self, text=1, chunk_bytes=1 << 20, range_bytes=128 << 20, piece_bytes=None):
        """A stream in view mode (paffy_hip_stream_open_view) as an object: input / submit / read / status / close."""
        return ViewStream(self, text, chunk_bytes, range_bytes, piece_bytes or getattr(self, "stream_piece_bytes", 64 << 20))

    def view_stream(self, chunks, text=1, range_bytes=128 << 20, sink=None, piece_bytes=None):
        """What `bin/paffy view` does with its input: host chunks (bytes of whole lines) through a stream in view mode, chunk k + 1
        submitted before chunk k is drained, a chunk of more than one range drained before the next buffer is asked for. text: 0 sums
        only, 1 stats lines, 2 lines and base-level rows. sink(piece) gets the text in order (default: it is collected). Returns a dict:
        text (bytes; None with a sink), sums (six), records, error (None, or (code, record counted from the stream's first record, aux,
        stage) of the failure that ends the run -- a chunk's failing record, or the rows' failure with stage -1 -- after which nothing
        more is read), open_chunks (how many chunks had more than one range)."""
        parts = []
        put = sink or parts.append
        st = self.open_view_stream(text, max(4096, max((len(c) for c in chunks), default=4096)), range_bytes, piece_bytes)
        error, open_chunks, records_done = None, 0, 0
        pending = None  # the record base of the chunk not yet drained

        def drain(base):
            for piece in st.pieces():
                put(piece)
            rows = st.status()[2]
            return (rows[0], base + rows[1], 0, -1) if rows else None

        try:
            for chunk in chunks:
                if not st.input(chunk):  # the chunk before is open: read it out first
                    open_chunks += 1
                    error = drain(pending)
                    pending = None
                    if error:
                        break
                    if not st.input(chunk):
                        raise RuntimeError("paffy_hip_stream_input: no buffer behind a drained chunk")
                info = st.submit(len(chunk))
                if pending is not None:
                    error = drain(pending)  # the earlier failure speaks
                    if error:
                        break
                pending = records_done
                if info.error.code:
                    drain(pending)
                    pending = None
                    error = (info.error.code, records_done + info.error.record, info.error.aux, info.error.stage)
                    break
                records_done += info.n_records
            if pending is not None and not error:
                error = drain(pending)
            sums, records, _ = st.status()
        finally:
            st.close()
        return {"text": None if sink else b"".join(parts), "sums": sums, "records": records, "error": error, "open_chunks": open_chunks}

    # ---- faffy chunk / extract / merge (FASTA index + item emit) ----
    def fasta_index(self, d_text, text_len, file_starts=(0,)):
        """Index FASTA text on the device (files back to back from file_starts); returns (records, bases). d_text must stay alive
        until the last faffy_emit."""
        n = len(file_starts)
        st = (C.c_int64 * max(1, n))(*[int(x) for x in file_starts])
        n_rec, n_bases = C.c_int64(), C.c_int64()
        self._fasta_d_text = d_text  # kept alive with the index (not under the name of the _fasta_text method below)
        self._check(lib().paffy_hip_fasta_index(self._ctx, C.c_void_p(d_text.data_ptr()), text_len, st, n, C.byref(n_rec), C.byref(n_bases)),
                    "paffy_hip_fasta_index")
        return n_rec.value, n_bases.value

    def fasta_table(self):
        """The record table: a list of (hdr_off, hdr_len, seq_off, seq_len)."""
        n = lib().paffy_hip_fasta_records(self._ctx, 0, 0, None)
        if n < 0:
            self._check(n, "paffy_hip_fasta_records")
        arr = (FastaRecord * max(1, n))()
        lib().paffy_hip_fasta_records(self._ctx, 0, n, arr)
        return [(r.hdr_off, r.hdr_len, r.seq_off, r.seq_len) for r in arr[:n]]

    def fasta_bases(self, first, n, d_dst):
        """Copy bases [first, first + n) of the compact buffer into the device tensor d_dst."""
        self._check(lib().paffy_hip_fasta_copy_bases(self._ctx, first, n, C.c_void_p(d_dst.data_ptr())), "paffy_hip_fasta_copy_bases")

    def _files(self, files):
        files = [f if isinstance(f, bytes) else f.encode() for f in files]
        starts, at = [], 0
        for f in files:
            starts.append(at)
            at += len(f)
        data = b"".join(files)
        d_text = self.to_device(data)
        self.fasta_index(d_text, len(data), starts or [0])
        return d_text

    @staticmethod
    def _fasta_text(files):
        """FASTA files -> (text back to back, file starts); a str is a path, bytes are a file's contents."""
        parts = []
        for f in files:
            if isinstance(f, bytes):
                parts.append(f)
            else:
                with open(f, "rb") as fh:
                    parts.append(fh.read())
        starts, at = [], 0
        for p in parts:
            starts.append(at)
            at += len(p)
        return b"".join(parts), starts or [0]

    def _load_fasta(self, fn, files, what):
        data, starts = self._fasta_text(files)
        d_text = self.to_device(data)
        st = (C.c_int64 * len(starts))(*starts)
        n_rec = C.c_int64()
        rc = fn(self._ctx, C.c_void_p(d_text.data_ptr()), len(data), st, len(starts), C.byref(n_rec))
        self.torch.cuda.synchronize(self.device)
        del d_text  # the loaders keep nothing of the text
        self._check(rc, what)
        return n_rec.value

    def keep_raw_sequences(self, on=True):
        """Keep the bases as loaded beside the upper-cased store (what `paffy view -a` prints); set before loading them."""
        self._check(lib().paffy_hip_keep_raw_sequences(self._ctx, 1 if on else 0), "paffy_hip_keep_raw_sequences")

    def set_sequences_fasta(self, files):
        """Sequences for add_mismatches from FASTA files (paths, or bytes each) read on the device, as `paffy add_mismatches a.fa b.fa`
        loads them; returns the number of records."""
        return self._load_fasta(lib().paffy_hip_set_sequences_fasta, files, "paffy_hip_set_sequences_fasta")

    def set_intervals_fasta(self, files):
        """Intervals for UPCONVERT from FASTA files (paths, or bytes each) read on the device, as `paffy upconvert a.fa b.fa` loads them;
        returns the number of records. A header that does not decode raises (the reference aborts)."""
        return self._load_fasta(lib().paffy_hip_set_intervals_fasta, files, "paffy_hip_set_intervals_fasta")

    def intervals_info(self):
        """The context's interval table (set_intervals or set_intervals_fasta): {intervals, blob_bytes, on_device, rounds}; on_device is 1
        when the device built it, rounds are that build's name-sort rounds."""
        out = (C.c_int64 * 4)()
        self._check(lib().paffy_hip_intervals_info(self._ctx, out), "paffy_hip_intervals_info")
        return {"intervals": out[0], "blob_bytes": out[1], "on_device": out[2], "rounds": out[3]}

    def intervals(self):
        """The interval table as upconvert searches it: [(name, start, end, length, out_name)] in table order."""
        info = self.intervals_info()
        n, nb = info["intervals"], info["blob_bytes"]
        nums = (C.c_int64 * max(1, 3 * n))()
        slices = (C.c_uint32 * max(1, 4 * n))()
        blob = C.create_string_buffer(max(1, nb))
        self._check(lib().paffy_hip_intervals_read(self._ctx, n, nb, nums, slices, blob), "paffy_hip_intervals_read")
        raw = blob.raw
        out = []
        for k in range(n):
            no, nl, oo, ol = slices[4 * k:4 * k + 4]
            out.append((raw[no:no + nl], nums[3 * k], nums[3 * k + 1], nums[3 * k + 2], raw[oo:oo + ol]))
        return out

    def fasta_seen(self, files, paf, with_target=False):
        """`paffy to_bed -q`'s query: [(name, sequence length, named)] per FASTA record, named = a line of the PAF text names it as its
        query (or, with with_target, as its target)."""
        data, starts = self._fasta_text(files)
        d_text = self.to_device(data)
        st = (C.c_int64 * len(starts))(*starts)
        n = C.c_int64()
        rc = lib().paffy_hip_fasta_index_headers(self._ctx, C.c_void_p(d_text.data_ptr()), len(data), st, len(starts), C.byref(n))
        del d_text
        self._check(rc, "paffy_hip_fasta_index_headers")
        table = self.fasta_table()
        d_paf = self.to_device(paf)
        seen = (C.c_uint8 * max(1, n.value))()
        self._check(lib().paffy_hip_fasta_seen(self._ctx, C.c_void_p(d_paf.data_ptr()), len(paf), 1 if with_target else 0, seen), "paffy_hip_fasta_seen")
        out = []
        for k, (h, hl, _, sl) in enumerate(table):
            name = data[h:h + hl].split(b"\0", 1)[0]
            out.append((name, sl, bool(seen[k])))
        return out

    def fasta_name_order(self):
        """The names of the context's FASTA index as the name tables order them (bytes, then the shorter first, then the input index),
        sorted on the device: (order, name_of, n_names) with order[k] = the record at place k and name_of[r] = the index of record r's
        name among the distinct names, both lists of int."""
        n = lib().paffy_hip_fasta_records(self._ctx, 0, 0, None)
        if n < 0:
            self._check(n, "paffy_hip_fasta_records")
        d = self.torch.zeros((2, max(1, n)), dtype=self.torch.int32, device=self.device)
        n_names = C.c_int64()
        rc = lib().paffy_hip_fasta_name_order(self._ctx, n, C.c_void_p(d[0].data_ptr()), C.c_void_p(d[1].data_ptr()), C.byref(n_names))
        self._check(rc, "paffy_hip_fasta_name_order")
        h = d[:, :n].cpu().numpy()
        return h[0].tolist(), h[1].tolist(), n_names.value

    def name_sort_stats(self):
        """The context's last name sort: {records, rounds, tied_after_first, names}."""
        out = (C.c_int64 * 4)()
        self._check(lib().paffy_hip_name_sort_stats(self._ctx, out), "paffy_hip_name_sort_stats")
        return {"records": out[0], "rounds": out[1], "tied_after_first": out[2], "names": out[3]}

    def fasta_records(self, files):
        """FASTA files (bytes each) -> [(header, bases)] as the device index reads them."""
        d_text = self._files(files)
        data = b"".join(f if isinstance(f, bytes) else f.encode() for f in files)
        table = self.fasta_table()
        total = table[-1][2] + table[-1][3] if table else 0
        buf = self.torch.zeros(max(1, total), dtype=self.torch.uint8, device=self.device)
        if total:
            self.fasta_bases(0, total, buf)
        bases = bytes(buf[:total].cpu().numpy().tobytes())
        del d_text
        return [(data[h:h + hl], bases[s:s + sl]) for h, hl, s, sl in table]

    def _faffy_fail(self, code, record):
        L = lib()
        info = PlanInfo()
        info.error.code, info.error.record = code, record
        raise PafError(f"record {record}: {L.paffy_hip_error_string(code).decode()}", info, L.paffy_hip_error_exit_status(code))

    def _faffy_emit(self, info):
        if info.error.code:
            self._faffy_fail(info.error.code, info.error.record)
        if not info.out_bytes:
            return b""
        d_out = self.alloc_out(info.out_bytes)
        err = _Error()
        self._check(lib().paffy_hip_faffy_emit(self._ctx, C.c_void_p(d_out.data_ptr()), d_out.numel(), C.byref(err)), "paffy_hip_faffy_emit")
        if err.code:
            self._faffy_fail(err.code, err.record)
        return bytes(d_out[: info.out_bytes].cpu().numpy().tobytes())

    def faffy_chunk(self, files, chunk_size=10000000, overlap=100000, d="./temp_fastas"):
        """`faffy chunk -c -o -d` over FASTA files (bytes each): [(file name, bytes)], names as the CLI prints them."""
        d_text = self._files(files)
        info = PlanInfo()
        rc = lib().paffy_hip_faffy_chunk_plan(self._ctx, chunk_size, overlap, C.byref(info))
        if rc == -2:
            raise ValueError(f"chunk size {chunk_size} with overlap {overlap} gives no chunks")
        self._check(rc, "paffy_hip_faffy_chunk_plan")
        out = self._faffy_emit(info)
        n = lib().paffy_hip_faffy_chunk_files(self._ctx, 0, None)
        ends = (C.c_int64 * max(1, n))()
        lib().paffy_hip_faffy_chunk_files(self._ctx, n, ends)
        res, at = [], 0
        for k in range(n):
            res.append((f"{d}/{k}.fa", out[at:ends[k]]))
            at = ends[k]
        del d_text
        return res

    def faffy_extract(self, files, bed, flank=10, min_size=100, skip_missing=False):
        """`faffy extract -f -m [-n]` of BED text over FASTA files: bytes."""
        d_text = self._files(files)
        bed = bed if isinstance(bed, bytes) else bed.encode()
        info = PlanInfo()
        self._check(lib().paffy_hip_faffy_extract_plan(self._ctx, bed, len(bed), flank, min_size, 1 if skip_missing else 0, C.byref(info)),
                    "paffy_hip_faffy_extract_plan")
        out = self._faffy_emit(info)
        del d_text
        return out

    def faffy_extract_device(self, files, d_bed, bed_len=None, flank=10, min_size=100, skip_missing=False):
        """faffy_extract with the BED text in device memory: d_bed is a uint8 device tensor (for example the buffer a to_bed run emitted
        into), bed_len the bytes of it that are text (default: all). Its allocation must be readable up to the next multiple of 16
        past bed_len, as to_device's and alloc_out's are. The plan keeps nothing of d_bed."""
        bed_len = d_bed.numel() if bed_len is None else int(bed_len)
        if bed_len < 0 or bed_len > d_bed.numel():
            raise ValueError(f"bed_len {bed_len} outside the tensor of {d_bed.numel()} bytes")
        d_text = self._files(files)
        info = PlanInfo()
        ptr = C.c_void_p(d_bed.data_ptr() if bed_len else None)
        self._check(lib().paffy_hip_faffy_extract_plan_device(self._ctx, ptr, bed_len, flank, min_size, 1 if skip_missing else 0, C.byref(info)),
                    "paffy_hip_faffy_extract_plan_device")
        out = self._faffy_emit(info)
        del d_text
        return out

    def faffy_merge(self, files):
        """`faffy merge` of chunk files (bytes each, in list order): bytes."""
        d_text = self._files(files)
        info = PlanInfo()
        self._check(lib().paffy_hip_faffy_merge_plan(self._ctx, C.byref(info)), "paffy_hip_faffy_merge_plan")
        out = self._faffy_emit(info)
        del d_text
        return out

    # ---- per-kernel HIP-event timing ----
    def profile(self, on=True, only=None):
        """HIP events around every kernel launch, or around the launches of the kernel `only` alone."""
        lib().paffy_hip_profile_only(self._ctx, only.encode() if only else None)
        lib().paffy_hip_profile_enable(self._ctx, 1 if on else 0)
        lib().paffy_hip_profile_reset(self._ctx)

    def profile_read(self):
        cap = 32
        names, ms, cnt = (C.c_char_p * cap)(), (C.c_double * cap)(), (C.c_int64 * cap)()
        n = lib().paffy_hip_profile_read(self._ctx, names, ms, cnt, cap)
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(min(n, cap))}


_default = None


class ViewStream:
    """paffy_hip_stream_open_view and the stream calls, one to one (Engine.open_view_stream)."""

    def __init__(self, engine, text, chunk_bytes, range_bytes, piece_bytes):
        self._e = engine
        self._st = C.c_void_p()
        engine._check(lib().paffy_hip_stream_open_view(engine._ctx, text, max(4096, chunk_bytes), piece_bytes, range_bytes, C.byref(self._st)), "paffy_hip_stream_open_view")

    def input(self, chunk):
        """Copies chunk into the next input buffer; False when paffy_hip_stream_input gives none (NULL)."""
        cap = C.c_int64()
        buf = lib().paffy_hip_stream_input(self._st, len(chunk), 0, C.byref(cap))
        if not buf:
            return False
        C.memmove(buf, chunk, len(chunk))
        return True

    def submit_rc(self, n):
        info = PlanInfo()
        return lib().paffy_hip_stream_submit(self._st, n, C.byref(info)), info

    def submit(self, n):
        rc, info = self.submit_rc(n)
        self._e._check(rc, "paffy_hip_stream_submit")
        return info

    def pieces(self):
        """The pieces of the oldest submitted chunk, until it is read out."""
        while True:
            piece, n = C.c_void_p(), C.c_int64()
            self._e._check(lib().paffy_hip_stream_read(self._st, C.byref(piece), C.byref(n)), "paffy_hip_stream_read")
            if n.value == 0:
                return
            yield C.string_at(piece.value, n.value)

    def status(self):
        """(six sums, records, None or (code, record) of the rows' failure of the chunk read last)."""
        sums, n, err = (C.c_int64 * 6)(), C.c_int64(), _Error()
        self._e._check(lib().paffy_hip_stream_view_status(self._st, sums, C.byref(n), C.byref(err)), "paffy_hip_stream_view_status")
        return list(sums), n.value, ((err.code, err.record) if err.code else None)

    def close(self):
        if self._st:
            lib().paffy_hip_stream_close(self._st)
            self._st = C.c_void_p()


def _engine():
    global _default
    if _default is None:
        _default = Engine()
    return _default


def pipe(stages, data):
    """`paffy a | paffy b | ...` over PAF text (bytes in, bytes out)."""
    return _engine().run(stages, data)[0]


def invert(data):
    """paffy invert (impl/paf_invert.c)."""
    return pipe([stage(INVERT)], data)


def dechunk(data, query=True, target=True):
    """paffy dechunk [-q] [-t] (impl/paf_dechunk.c): query=False is -t, target=False is -q."""
    return pipe([stage_dechunk(query, target)], data)


def upconvert(data, fasta=None, fasta_files=None):
    """paffy upconvert [fasta...] (impl/paf_upconvert.c); fasta: {header: bases} of the extracted subsequences, in file order, or
    fasta_files: the FASTA files themselves (paths, or bytes each), read on the device."""
    e = _engine()
    if fasta_files is not None:
        e.set_intervals_fasta(fasta_files)
    else:
        fasta = fasta or {}
        e.set_intervals(list(fasta), [len(v) for v in fasta.values()])
    return e.run([stage(UPCONVERT)], data)[0]


def shatter(data):
    """paffy shatter (impl/paf_shatter.c)."""
    return pipe([stage(SHATTER)], data)


def add_mismatches(data, seqs=None, remove=False):
    """paffy add_mismatches [fasta...] / paffy add_mismatches -a (impl/paf_add_mismatches.c)."""
    if remove:
        return pipe([stage(REMOVE_MISMATCHES)], data)
    e = _engine()
    e.set_sequences(seqs)
    return e.run([stage(ADD_MISMATCHES)], data)[0]


def view_stats(data, seqs):
    """The numbers of `paffy view [fasta...]` (impl/paf_view.c) without its base-level rows: paf_stats_calc of every record as
    add_mismatches encodes it against seqs ({header: bases}). Returns (six totals, list of six-tuples per record): matches, mismatches,
    inserts, deletes, insert bases, delete bases."""
    e = _engine()
    e.set_sequences(seqs)
    e.stats_only(True)
    try:
        d_in = e.to_device(data)
        info = e.plan([stage(ADD_MISMATCHES), stage(STATS)], d_in, len(data))
        if info.error.code:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        return e.plan_stats(), e.record_stats(info.n_records)
    finally:
        e.stats_only(False)


def view(data, seqs, include_alignment=False, per_alignment=True, aggregate=False):
    """What `paffy view [fasta...] [-a] [-t] [-s]` (impl/paf_view.c) writes to its output for PAF text `data` and seqs ({header: bases}):
    per record the stats line of paf_pretty_print (with include_alignment the base-level rows behind it) unless per_alignment is off,
    then with `aggregate` the totals' line. All of the per-record text is written on the GPU (Engine.view_text); the plans are sums-only
    exactly when the CLI's are: whenever no rows are printed."""
    import struct

    e = _engine()
    rows = bool(include_alignment and per_alignment)
    e.keep_raw_sequences(bool(include_alignment))
    e.set_sequences(seqs)
    e.stats_only(not rows)
    try:
        d_in = e.to_device(data)
        info = e.plan([stage(ADD_MISMATCHES), stage(STATS)], d_in, len(data))
        if info.error.code:
            L = lib()
            raise PafError(f"record {info.error.record}: {L.paffy_hip_error_string(info.error.code).decode()}", info,
                           L.paffy_hip_error_exit_status(info.error.code))
        out = e.view_text(0, info.n_records, rows) if per_alignment else b""
        if aggregate:
            def f32(x):
                return struct.unpack("<f", struct.pack("<f", x))[0]

            def ratio(a, b):  # (float)a / b: a float division, "-nan" for 0.0f / 0.0f as x86-64 glibc prints it
                return "-nan" if b == 0 else "%f" % f32(f32(a) / f32(b))

            m, x, qi, qd, qib, qdb = e.plan_stats()
            out += ("Total-alignments:%d\tAvg-Identity:%s\tAvg-Identity-with-gaps:%s\tAligned-bases:%d\tAligned-bases-with-gaps:%d\tQuery-inserts:%d\tQuery-deletes:%d\n"
                    % (info.n_records, ratio(m, m + x), ratio(m, m + x + qib + qdb), m + x, m + x + qib + qdb, qi, qd)).encode()
        return out
    finally:
        e.stats_only(False)
        e.keep_raw_sequences(False)


def tile(data):
    """paffy tile (impl/paf_tile.c)."""
    return _engine().tile(data)[0]


def chain(data, gap_open=5000, gap_extend=1, max_gap=1000000, trim=1.0, fresh_walk=False):
    """paffy chain [-d gap_open] [-e gap_extend] [-g max_gap] [-t trim] (impl/paf_chain.c); fresh_walk: Engine.chain_fresh_walk."""
    return _engine().chain(data, gap_open, gap_extend, max_gap, trim, fresh_walk=fresh_walk)[0]


def trim(data, trim_identity=0.05, trim_fraction=1.0, fixed_trim=False):
    """paffy trim [-r trim_identity] [-t trim_fraction] [-f] (impl/paf_trim.c)."""
    return pipe([stage(TRIM_FIXED if fixed_trim else TRIM_IDENTITY, trim_identity, trim_fraction)], data)


def filter(data, **thresholds):  # noqa: A001 -- named after the reference command
    """paffy filter [-s -t -u -v -w -x] (impl/paf_filter.c); keyword arguments as in Engine.set_filter."""
    e = _engine()
    e.set_filter(**thresholds)
    return e.run([stage(FILTER)], data)[0]


def dedupe(data, check_inverse=False):
    """paffy dedupe [-a] (impl/paf_dedupe.c)."""
    return _engine().dedupe(data, check_inverse)[0]


def split_file(data, by_query=False, min_length=0, batch_bytes=None):
    """paffy split_file [-q] [-m min_length] (impl/paf_split_file.c): {file name without prefix and ".paf": bytes}, in opening order."""
    return _engine().split_file(data, by_query, min_length, batch_bytes)[0]
