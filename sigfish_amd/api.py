"""Host-side mirror of the reference's interface for the alignment stage, over the C-ABI.

Names follow the reference (hasindu2008/sigfish v0.2.0): a RefModel is refsynth_t (src/sigfish.h:90-99) as
produced by gen_ref (src/genref.c:86-241); Aligner.align_db is align_db (src/sigfish.c:1003-1015) for a whole
batch; result rows carry the aln_t fields (src/sigfish.h:146-158) the PAF writer (src/sigfish.c:628-660) prints.
"""
import ctypes as C
import gzip

import numpy as np

from . import _lib

# opt.flag bits (src/sigfish.h:30-39)
RNA, DTW, INV, REF, END = 0x001, 0x002, 0x004, 0x010, 0x020
PRESS_NONE, PRESS_ZLIB, PRESS_ZSTD = 0, 1, 2  # SFA_PRESS_*: the record_zlib argument of align_blow5 / decode_blow5_device (True = zlib)
BLOW5_INFLATE, BLOW5_FIELDS, BLOW5_STREAM = 1, 2, 3  # SFA_BLOW5_*: why decode_blow5_device's device stages declined a record

RESULT_DTYPE = np.dtype([("rid", "<i4"), ("pos_st", "<i4"), ("pos_end", "<i4"), ("score", "<f4"), ("score2", "<f4"),
                         ("strand", "i1"), ("mapq", "u1"), ("valid", "u1"), ("pad", "u1")])
assert RESULT_DTYPE.itemsize == C.sizeof(_lib.SfaResult)


QUERY_INFO_DTYPE = np.dtype([("n_events", "<i8"), ("qstart", "<i8"), ("qend", "<i8"), ("start_raw_idx", "<u8"),
                             ("end_raw_idx", "<u8"), ("status", "<i4"), ("pad", "<i4")])
assert QUERY_INFO_DTYPE.itemsize == C.sizeof(_lib.SfaQueryInfo)


SESSION_RAW_INFO_DTYPE = np.dtype([("n_samples", "<i8"), ("n_events", "<i8"), ("q_events", "<i8"), ("norm_mean", "<f4"), ("norm_sd", "<f4"),
                                   ("status", "<i4"), ("norm_window", "<i4")])
assert SESSION_RAW_INFO_DTYPE.itemsize == C.sizeof(_lib.SfaSessionRawInfo)
RAW_CALIBRATED, RAW_FULL, RAW_ENDED, RAW_POISONED = 1, 2, 4, 8  # bits of SESSION_RAW_INFO_DTYPE's status
SESSION_AUTO_DTYPE = np.dtype([("target", "<i8"), ("frozen_at", "<i8"), ("skip", "<i4"), ("status", "<i4")])  # sfa_session_auto_t
AUTO_PENDING, AUTO_RESOLVED, AUTO_NO_TARGET, AUTO_NO_EVENT, AUTO_BEYOND_MAX, AUTO_AT_FINAL = 0, 1, 2, 3, 4, 16  # SFA_AUTO_*
TARGET_DTYPE = np.dtype([("contig", "<i4"), ("begin", "<i4"), ("end", "<i4")])  # sfa_target_t
CLASS_DTYPE = np.dtype([("on_score", "<f4"), ("off_score", "<f4"), ("on_rid", "<i4"), ("on_pos_end", "<i4"), ("off_rid", "<i4"), ("off_pos_end", "<i4"),
                        ("on_strand", "i1"), ("off_strand", "i1"), ("pad", "i1", (2,)), ("n_events", "<i4"), ("valid", "<i4")])  # sfa_class_t
assert TARGET_DTYPE.itemsize == C.sizeof(_lib.SfaTarget) and CLASS_DTYPE.itemsize == C.sizeof(_lib.SfaClass)
ENRICH, DEPLETE = 0, 1  # the modes of target_decide
REACH_TARGET_DTYPE = np.dtype([("contig", "<i4"), ("begin", "<i4"), ("end", "<i4"), ("lead", "<i4"), ("strand", "i1"), ("pad", "i1", (3,))])  # sfa_reach_target_t
assert REACH_TARGET_DTYPE.itemsize == C.sizeof(_lib.SfaReachTarget) == 20
REACH_GROUP_TARGET_DTYPE = np.dtype([("contig", "<i4"), ("begin", "<i4"), ("end", "<i4"), ("lead", "<i4"), ("group", "<i4"), ("strand", "i1"),
                                     ("pad", "i1", (3,))])  # sfa_reach_group_target_t
assert REACH_GROUP_TARGET_DTYPE.itemsize == C.sizeof(_lib.SfaReachGroupTarget) == 24
REACH_NONE, REACH_BELOW_TRACK = -1, -2  # anchors of reach_tables(): off target; an anchor below st_offset (no depth is counted there)
REACH_LEAD_MAX = 1 << 30
GROUP_TARGET_DTYPE = np.dtype([("contig", "<i4"), ("begin", "<i4"), ("end", "<i4"), ("group", "<i4")])  # sfa_group_target_t
GROUP_BEST_DTYPE = np.dtype([("score", "<f4"), ("rid", "<i4"), ("pos_end", "<i4"), ("strand", "i1"), ("pad", "i1", (3,))])  # sfa_group_best_t
GROUP_HEAD_DTYPE = np.dtype([("best", "<i4"), ("second", "<i4"), ("best_score", "<f4"), ("second_score", "<f4"), ("n_events", "<i4"),
                             ("valid", "<i4")])  # sfa_group_head_t
assert GROUP_TARGET_DTYPE.itemsize == C.sizeof(_lib.SfaGroupTarget) and GROUP_BEST_DTYPE.itemsize == C.sizeof(_lib.SfaGroupBest) == 16
assert GROUP_HEAD_DTYPE.itemsize == C.sizeof(_lib.SfaGroupHead)
GROUP_MAX = 1023  # n_groups at most
OPEN_CLASS_DTYPE = np.dtype([("cls", CLASS_DTYPE), ("on_group", "<i4"), ("off_group", "<i4")])  # sfa_open_class_t
assert OPEN_CLASS_DTYPE.itemsize == CLASS_DTYPE.itemsize + 8
GROUP_COVER_DTYPE = np.dtype([("columns", "<i8"), ("capped", "<i8"), ("depth_sum", "<u8"), ("depth_min", "<u4"), ("depth_max", "<u4")])  # sfa_group_cover_t
assert GROUP_COVER_DTYPE.itemsize == C.sizeof(_lib.SfaGroupCover) == 32
RAW_RECALIBRATED = 16  # ... and the bit of one call: the slot was recalibrated and swept again from event 0
RECAL_AT_END = 0x1     # SFA_RECAL_AT_END
RECAL_MAX_POINTS = 32


def recal_window(q_avail, ended, norm, query, at=(), at_end=False):
    """The window a raw-session slot is normalised over (sfa::recal_window, csrc/recal_rule.hpp): q_avail = min(n_events - skip,
    query) query events are available, `ended` tells whether the end of the read has been seen.  0: not calibrated."""
    if at_end and ended and 25 <= q_avail < query:
        return q_avail
    w = 0
    for p in at:
        if p <= q_avail:
            w = p
    if w > 0:
        return w
    return norm if q_avail >= norm else 0


def recal_double(norm, query):
    """The doubling list (sfa::recal_double): 2 norm, 4 norm, ... below query, then query; empty when norm == query."""
    if norm < 1 or norm >= query:
        return ()
    at, w = [], 2 * norm
    while w < query and len(at) < RECAL_MAX_POINTS - 1:
        at.append(w)
        w *= 2
    return tuple(at + [query])


class SfaError(RuntimeError):
    pass


def _press(record_zlib):
    """record_zlib as the C-ABI takes it: 0 none, 1 zlib (any flag that is true), 2 zstd"""
    return PRESS_ZSTD if (record_zlib is not True and record_zlib == PRESS_ZSTD) else int(bool(record_zlib))


def _check(rc, what):
    if rc != 0:
        raise SfaError(f"{what} failed ({rc}): {_lib.load().sfa_last_error().decode()}")


def version():
    return _lib.load().sfa_version().decode()


def build_id():
    return _lib.load().sfa_build_id().decode()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def znormalise(v):
    v = _f32(v).copy()
    _lib.load().sfa_znormalise(v.ctypes.data_as(_lib.f32p), len(v))
    return v


def read_fasta(path):
    """[(name, sequence)]: name is the first word of the header, sequence lines are concatenated (kseq.h)."""
    op = gzip.open if str(path).endswith(".gz") else open
    recs, name, chunks = [], None, []
    with op(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    recs.append((name, "".join(chunks)))
                w = line[1:].split()
                name, chunks = (w[0] if w else ""), []
            elif name is not None:
                chunks.append("".join(line.split()))
    if name is not None:
        recs.append((name, "".join(chunks)))
    return recs


class RefModel:
    """refsynth_t: per-contig z-normalised expected event levels, forward and (DNA) reverse complement."""

    def __init__(self, names, seq_lengths, ref_lengths, st_offset, forward, reverse):
        self.names = list(names)
        self.seq_lengths = np.asarray(seq_lengths, np.int32)
        self.ref_lengths = np.ascontiguousarray(ref_lengths, np.int32)
        self.st_offset = np.ascontiguousarray(st_offset, np.int32)
        self.forward = [_f32(a) for a in forward]
        self.reverse = None if reverse is None else [_f32(a) for a in reverse]
        self.num_ref = len(self.names)

    @classmethod
    def from_records(cls, records, level_mean, k, flag=0, query_size=250):
        """gen_ref (src/genref.c:86-241) over [(name, sequence)] with a 4^k table of k-mer level means."""
        L = _lib.load()
        lv = _f32(level_mean)
        if len(lv) != 4 ** k:
            raise ValueError(f"k-mer model needs {4 ** k} levels, got {len(lv)}")
        rna = bool(flag & RNA)
        names, sl, rl, so, fw, rv = [], [], [], [], [], []
        for name, seq in records:
            b = seq.encode()
            cap = max(len(b) + 1 - k, 1)
            f = np.zeros(cap, np.float32)
            r = np.zeros(cap, np.float32)
            off = C.c_int32(0)
            n = L.sfa_gen_ref_record(b, len(b), lv.ctypes.data_as(_lib.f32p), k, flag, query_size,
                                     f.ctypes.data_as(_lib.f32p), None if rna else r.ctypes.data_as(_lib.f32p),
                                     C.byref(off))
            if n <= 0:
                raise SfaError(f"contig {name}: cannot build reference events (length {len(b)}, k={k})")
            names.append(name)
            sl.append(len(b))
            rl.append(n)
            so.append(off.value)
            fw.append(f[:n].copy())
            rv.append(r[:n].copy())
        return cls(names, sl, rl, so, fw, None if rna else rv)

    @classmethod
    def from_fasta(cls, path, level_mean, k, flag=0, query_size=250):
        return cls.from_records(read_fasta(path), level_mean, k, flag, query_size)

    def total_columns(self):
        return int(self.ref_lengths.sum()) * (1 if self.reverse is None else 2)

    def _as_c(self):
        n = self.num_ref
        fa = (_lib.f32p * n)(*[a.ctypes.data_as(_lib.f32p) for a in self.forward])
        ra = None
        if self.reverse is not None:
            ra = (_lib.f32p * n)(*[a.ctypes.data_as(_lib.f32p) for a in self.reverse])
        ref = _lib.SfaRef(n, self.ref_lengths.ctypes.data_as(_lib.i32p), self.st_offset.ctypes.data_as(_lib.i32p),
                          fa, C.cast(ra, C.POINTER(_lib.f32p)) if ra is not None else None)
        return ref, (fa, ra)


class Aligner:
    """The accelerator context: reference arrays resident in HBM, batches aligned by the gfx950 kernels."""

    def __init__(self, ref: RefModel, flag=0, device=0, devices=None):
        """device: one GPU (sfa_init).  devices: a list of GPUs (sfa_init_devices) -- every batch is then sharded over them
        in contiguous read ranges and comes back in input order; a GPU may be listed more than once."""
        self._L = _lib.load()
        self._h = C.c_void_p()
        self._last_n = 0
        self._last_rows = None  # primaries of the most recent call (event_maps' default)
        self.maps_on_host = 0
        self.ref, self.flag, self.device = ref, int(flag), int(device)
        cref, keep = ref._as_c()
        if devices is None:
            _check(self._L.sfa_init(C.byref(self._h), C.byref(cref), self.flag, self.device), "sfa_init")
        else:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            _check(self._L.sfa_init_devices(C.byref(self._h), C.byref(cref), self.flag, devs, len(devices)), "sfa_init_devices")
        del keep

    def n_devices(self):
        return int(self._L.sfa_n_devices(self._h))

    def close(self):
        if self._h:
            self._L.sfa_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- align_db over packed host arrays -------------------------------------------------------------------
    def align_db(self, queries, q_off):
        """queries: concatenated z-normalised event means (event order); q_off: int64[n+1]. -> RESULT_DTYPE[n]"""
        q = _f32(queries)
        qo = np.ascontiguousarray(q_off, np.int64)
        n = len(qo) - 1
        out = np.zeros(n, RESULT_DTYPE)
        self._last_n = n
        self._last_rows = out
        if q.size == 0:
            q = np.zeros(1, np.float32)
        _check(self._L.sfa_align_batch(self._h, q.ctypes.data_as(_lib.f32p), qo.ctypes.data_as(_lib.i64p), n,
                                       out.ctypes.data_as(C.c_void_p)), "sfa_align_batch")
        return out

    def submit(self, queries, q_off):
        """First half of align_db: queue the batch and return; collect the rows with wait().  One batch in flight."""
        q = _f32(queries)
        qo = np.ascontiguousarray(q_off, np.int64)
        if q.size == 0:
            q = np.zeros(1, np.float32)
        self._pending = (q, qo)  # the library reads `queries` until wait()
        _check(self._L.sfa_submit_batch(self._h, q.ctypes.data_as(_lib.f32p), qo.ctypes.data_as(_lib.i64p), len(qo) - 1),
               "sfa_submit_batch")

    def wait(self):
        q, qo = getattr(self, "_pending", None) or (None, np.zeros(1, np.int64))
        n = len(qo) - 1
        out = np.zeros(n, RESULT_DTYPE)
        self._last_n = n
        self._last_rows = out
        try:
            _check(self._L.sfa_wait_batch(self._h, out.ctypes.data_as(C.c_void_p), n), "sfa_wait_batch")
        finally:
            self._pending = None
        return out

    # -- same with device-resident buffers (torch tensors or raw pointers) ------------------------------------
    def align_db_device(self, d_queries_ptr, q_off, n, d_out_ptr, sync=True):
        qo = np.ascontiguousarray(q_off, np.int64)
        _check(self._L.sfa_align_batch_device(self._h, C.c_void_p(d_queries_ptr), qo.ctypes.data_as(_lib.i64p), n,
                                              C.c_void_p(d_out_ptr), 1 if sync else 0), "sfa_align_batch_device")

    def align_events(self, event_tables, qstart, qend):
        """event_tables: list of structured arrays with sfa_event_t layout (or None)."""
        n = len(event_tables)
        EP = C.POINTER(_lib.SfaEvent)
        ptrs = (EP * n)()
        nev = np.zeros(n, np.int64)
        keep = []
        for i, t in enumerate(event_tables):
            if t is None or len(t) == 0:
                ptrs[i] = None
                continue
            a = np.ascontiguousarray(t)
            keep.append(a)
            ptrs[i] = C.cast(a.ctypes.data, EP)
            nev[i] = len(a)
        qs = np.ascontiguousarray(qstart, np.int64)
        qe = np.ascontiguousarray(qend, np.int64)
        out = np.zeros(n, RESULT_DTYPE)
        self._last_n = n
        self._last_rows = out
        _check(self._L.sfa_align_events(self._h, ptrs, nev.ctypes.data_as(_lib.i64p), qs.ctypes.data_as(_lib.i64p),
                                        qe.ctypes.data_as(_lib.i64p), n, out.ctypes.data_as(C.c_void_p)),
               "sfa_align_events")
        return out

    def session(self, n_slots, starts=True, resweep=False, flags=None, candidates=0, auto_start=None, keep_events=0, spread=False):
        """An alignment session of n_slots growing reads on this aligner (sfa_session_create); starts=False carries costs only
        (SFA_SESSION_NO_START: half the memory, the coordinate on the start side of every row is -1).  resweep=True
        (SFA_SESSION_RESWEEP): a raw-mode-only session that sweeps a slot only when its normalisation window changes, over the
        window's events -- the one kind of session an RNA aligner without INV can have (its query is the events reversed).
        flags: the raw flag word in place of starts / resweep.  candidates=1..4: configure_candidates() on the new session.
        auto_start=dict(skip=, norm=, query=, every=, max_samples=[, recalibrate=, at_end=]): configure_raw() with skip as the
        largest skip, then configure_auto_start(every, max_samples), on the new session.  keep_events=N: keep_events(N) on the
        new (event-mode) session, so that event_maps() has the slots' events.
        spread=True (SFA_SESSION_SPREAD): on an Aligner made with devices= the slots are dealt over its devices, slot i on the
        i % G-th; every method keeps the caller's slot numbers and returns the same bytes.  Without it such an Aligner has no
        sessions; on a single device it changes nothing."""
        s = Session(self, n_slots, starts, resweep, flags, spread)
        if keep_events:
            try:
                s.keep_events(keep_events)
            except Exception:
                s.close()
                raise
        if auto_start is not None:
            try:
                a = dict(auto_start)
                every, max_samples = a.pop("every"), a.pop("max_samples")
                s.configure_raw(**a)
                s.configure_auto_start(every, max_samples)
            except Exception:
                s.close()
                raise
        if candidates:
            try:
                s.configure_candidates(candidates)
            except Exception:
                s.close()
                raise
        return s

    def set_option(self, key, value):
        _check(self._L.sfa_set_option(self._h, key.encode(), int(value)), f"sfa_set_option({key})")

    def set_secondary(self, n):
        """Secondary mappings per read, 0..4 (0: off, the default); read them with secondary_rows() after each call.  Reads of more
        than 2048 events have none unless set_option("secondary_strips", 1) is in force as well."""
        self.set_option("secondary", n)

    def secondary_rows(self, n_reads=None):
        """The secondaries of the most recent call as RESULT_DTYPE[n_reads, 4], best first (valid = 0 for absent slots, and for every
        slot of a read of more than 2048 events unless set_option("secondary_strips", 1) was in force for that call)."""
        n = self._last_n if n_reads is None else int(n_reads)
        out = np.zeros((n, 4), RESULT_DTYPE)
        _check(self._L.sfa_secondary_rows(self._h, out.ctypes.data_as(C.c_void_p), n), "sfa_secondary_rows")
        return out

    def event_maps(self, rows=None, read_of_row=None):
        """aln_t.r2qevent_map of rows of the most recent call, computed on the device: a list of int32 [size, 2] arrays (start, stop
        per reference column, as r2qevent_map returns for one row; size 0 for a row without a map).  rows: RESULT_DTYPE rows that
        call returned -- default: its primaries -- or rows of secondary_rows(); read_of_row: the read of each row (default: the
        identity).  The number of rows the library computed on the host instead is left in `maps_on_host`: rows whose moves exceed
        the "map_scratch_bytes" budget, and rows of reads beyond 2048 events unless set_option("map_strips", 1) is in force, which
        runs those on the device in row strips (same maps)."""
        if rows is None:
            rows = self._last_rows
            if rows is None:
                raise SfaError("event_maps: no rows of a previous call to default to")
        rows = np.ascontiguousarray(rows, RESULT_DTYPE).reshape(-1)
        n = len(rows)
        ror = None if read_of_row is None else np.ascontiguousarray(read_of_row, np.int32).reshape(-1)
        if ror is not None and len(ror) != n:
            raise SfaError("event_maps: read_of_row must name one read per row")
        ok = (rows["valid"] != 0) & (rows["rid"] >= 0)
        size = np.where(ok, rows["pos_end"].astype(np.int64) - rows["pos_st"] + 1, 0)
        size = np.maximum(size, 0)
        off = np.zeros(n + 1, np.int64)
        np.cumsum(size, out=off[1:])
        pairs = np.full((max(int(off[-1]), 1), 2), np.iinfo(np.int32).min, np.int32)
        on_host = C.c_int32(0)
        _check(self._L.sfa_event_maps(self._h, rows.ctypes.data_as(C.c_void_p), None if ror is None else ror.ctypes.data_as(_lib.i32p), n,
                                      off.ctypes.data_as(_lib.i64p), pairs.ctypes.data_as(_lib.i32p), C.byref(on_host)), "sfa_event_maps")
        self.maps_on_host = int(on_host.value)
        out = []
        for k in range(n):
            m = pairs[off[k]:off[k + 1]]
            # a row the library wrote nothing for (no complete map, see sfa_event_maps) keeps the fill value
            out.append(m.copy() if len(m) and m[0, 0] != np.iinfo(np.int32).min else np.zeros((0, 2), np.int32))
        return out

    def set_pore(self, pore):
        """The reference's opt.pore_flag: 0 R9 (default), 1 R10, 2 RNA004 (the RNA automatic query start depends on it)."""
        _check(self._L.sfa_set_pore(self._h, int(pore)), "sfa_set_pore")

    def align_raw(self, raw, raw_off, scaling, prefix_size=50, query_size=250, return_events=False):
        """process_db on the device: raw int16 samples (concatenated) -> (rows, info).  scaling: float64 [n,3] =
        digitisation, offset, range per read.  prefix_size=-1: RNA automatic query start (info.status bit 2 where
        it fell back to event 50).  return_events: also the query windows' event tables,
        EVENT_DTYPE[n, query_size] (means z-normalised; read i uses the first info.qend - info.qstart entries)."""
        raw = np.ascontiguousarray(raw, np.int16)
        ro = np.ascontiguousarray(raw_off, np.int64)
        sc = np.ascontiguousarray(scaling, np.float64).reshape(-1)
        n = len(ro) - 1
        rows = np.zeros(n, RESULT_DTYPE)
        info = np.zeros(n, QUERY_INFO_DTYPE)
        self._last_n = n
        self._last_rows = rows
        if raw.size == 0:
            raw = np.zeros(1, np.int16)
        qev = np.zeros((n, query_size), EVENT_DTYPE) if return_events else None
        _check(self._L.sfa_align_raw_ex(self._h, raw.ctypes.data_as(C.POINTER(C.c_int16)), ro.ctypes.data_as(_lib.i64p),
                                        sc.ctypes.data_as(C.POINTER(C.c_double)), n, prefix_size, query_size,
                                        rows.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p),
                                        qev.ctypes.data_as(C.c_void_p) if return_events else None), "sfa_align_raw_ex")
        return (rows, info, qev) if return_events else (rows, info)

    def align_blow5(self, records, rec_off, record_zlib, signal_svb, prefix_size=50, query_size=250, return_events=False):
        """load_db's records straight to the device: `records` = the BLOW5 records of a batch back to back (bytes / uint8 array,
        without their size prefixes), rec_off int64[n+1].  -> (rows, info, heads[, query events])"""
        rec = np.frombuffer(records, np.uint8) if isinstance(records, (bytes, bytearray, memoryview)) else np.ascontiguousarray(records, np.uint8)
        ro = np.ascontiguousarray(rec_off, np.int64)
        n = len(ro) - 1
        rows = np.zeros(n, RESULT_DTYPE)
        info = np.zeros(n, QUERY_INFO_DTYPE)
        self._last_n = n
        self._last_rows = rows
        heads = (_lib.SfaReadHead * max(n, 1))()
        qev = np.zeros((n, query_size), EVENT_DTYPE) if return_events else None
        if rec.size == 0:
            rec = np.zeros(1, np.uint8)
        _check(self._L.sfa_align_blow5(self._h, rec.ctypes.data_as(C.c_void_p), ro.ctypes.data_as(_lib.i64p), n, _press(record_zlib),
                                       int(bool(signal_svb)), prefix_size, query_size, rows.ctypes.data_as(C.c_void_p),
                                       info.ctypes.data_as(C.c_void_p), C.cast(heads, C.c_void_p),
                                       qev.ctypes.data_as(C.c_void_p) if return_events else None), "sfa_align_blow5")
        hs = [dict(read_id=heads[i].read_id.decode(), n_samples=heads[i].n_samples, digitisation=heads[i].digitisation,
                   offset=heads[i].offset, range=heads[i].range, record_bytes=heads[i].record_bytes) for i in range(n)]
        return (rows, info, hs, qev) if return_events else (rows, info, hs)

    def inflate_device(self, streams, cap_factor=4, cap_extra=4096):
        """The device-side DEFLATE decoder alone: list of zlib streams -> list of bytes (None where the decoder declined).  Stream i
        gets a slot of len(stream) * cap_factor + cap_extra bytes, the slots back to back; cap_extra: one number, or one per stream."""
        n = len(streams)
        in_off = np.concatenate([[0], np.cumsum([len(x) for x in streams])]).astype(np.int64)
        blob = np.frombuffer(b"".join(streams) + b"\0" * 8, np.uint8)
        extra = np.broadcast_to(np.asarray(cap_extra, np.int64), (n,))
        out_off = np.concatenate([[0], np.cumsum([len(x) * cap_factor + int(e) for x, e in zip(streams, extra)])]).astype(np.int64)
        out = np.zeros(int(out_off[-1]) + 8, np.uint8)
        lens = np.zeros(max(n, 1), np.int32)
        _check(self._L.sfa_inflate_zlib_device(self._h, blob.ctypes.data_as(C.c_void_p), in_off.ctypes.data_as(_lib.i64p), n,
                                               out.ctypes.data_as(C.c_void_p), out_off.ctypes.data_as(_lib.i64p),
                                               lens.ctypes.data_as(_lib.i32p)), "sfa_inflate_zlib_device")
        return [None if lens[i] < 0 else out[out_off[i]:out_off[i] + lens[i]].tobytes() for i in range(n)]

    def zstd_device(self, streams, cap_factor=4, cap_extra=4096):
        """The device-side zstd decoder alone: list of zstd records -> list of bytes (None where the decoder declined).  Slots as
        inflate_device's, each rounded up to 16 bytes."""
        n = len(streams)
        in_off = np.concatenate([[0], np.cumsum([len(x) for x in streams])]).astype(np.int64)
        blob = np.frombuffer(b"".join(streams) + b"\0" * 8, np.uint8)
        extra = np.broadcast_to(np.asarray(cap_extra, np.int64), (n,))
        out_off = np.concatenate([[0], np.cumsum([(len(x) * cap_factor + int(e) + 15) & ~15 for x, e in zip(streams, extra)])]).astype(np.int64)
        out = np.zeros(int(out_off[-1]) + 8, np.uint8)
        lens = np.zeros(max(n, 1), np.int32)
        _check(self._L.sfa_zstd_device(self._h, blob.ctypes.data_as(C.c_void_p), in_off.ctypes.data_as(_lib.i64p), n,
                                       out.ctypes.data_as(C.c_void_p), out_off.ctypes.data_as(_lib.i64p),
                                       lens.ctypes.data_as(_lib.i32p)), "sfa_zstd_device")
        return [None if lens[i] < 0 else out[out_off[i]:out_off[i] + lens[i]].tobytes() for i in range(n)]

    def decode_blow5_device(self, records, rec_off, record_zlib, signal_svb, capacity=None):
        """The device-side record decoder alone (tests): the stages of align_blow5 before the alignment, no host reader behind
        them.  -> (status int32[n], heads, raw_off int64[n+1], samples int16[raw_off[n]]).  status: 0 decoded, BLOW5_INFLATE /
        BLOW5_FIELDS (no samples counted, empty head) or BLOW5_STREAM (samples undefined).  capacity: room for that many
        samples (default: what any record of these sizes can hold); SfaError (SFA_ERANGE) where the records announce more."""
        rec = np.frombuffer(records, np.uint8) if isinstance(records, (bytes, bytearray, memoryview)) else np.ascontiguousarray(records, np.uint8)
        ro = np.ascontiguousarray(rec_off, np.int64)
        n = len(ro) - 1
        if capacity is None:  # svb-zd: at most 4 samples per byte; inflated: 4x + 4 KB per record
            capacity = 4 * (4 * int(ro[-1]) + 4096 * n if record_zlib else int(ro[-1]))
        status = np.zeros(max(n, 1), np.int32)
        heads = (_lib.SfaReadHead * max(n, 1))()
        raw_off = np.zeros(n + 1, np.int64)
        samples = np.zeros(max(int(capacity), 1), np.int16)
        if rec.size == 0:
            rec = np.zeros(1, np.uint8)
        _check(self._L.sfa_decode_blow5_device(self._h, rec.ctypes.data_as(C.c_void_p), ro.ctypes.data_as(_lib.i64p), n, _press(record_zlib),
                                               int(bool(signal_svb)), status.ctypes.data_as(_lib.i32p), C.cast(heads, C.c_void_p),
                                               raw_off.ctypes.data_as(_lib.i64p), samples.ctypes.data_as(C.POINTER(C.c_int16)), int(capacity)),
               "sfa_decode_blow5_device")
        hs = [dict(read_id=heads[i].read_id.decode(), n_samples=heads[i].n_samples, digitisation=heads[i].digitisation,
                   offset=heads[i].offset, range=heads[i].range, record_bytes=heads[i].record_bytes) for i in range(n)]
        return status[:n], hs, raw_off, samples[:int(raw_off[-1])]

    def detect_events_device(self, raw, raw_off, scaling, tstats=False):
        """The event detection of align_raw alone (tests): -> (tables, routes[, t_short, t_long]).  tables: one EVENT_DTYPE
        array per read, the whole table, means in pA; routes int32[n]: bit 0 = sequential prefix sums, bit 1 = sequential
        peak picker; tstats: also the two t-statistics, float32[raw_off[n]] each."""
        raw = np.ascontiguousarray(raw, np.int16)
        ro = np.ascontiguousarray(raw_off, np.int64)
        sc = np.ascontiguousarray(scaling, np.float64).reshape(-1)
        n = len(ro) - 1
        total = int(ro[-1]) if n > 0 else 0
        ev = np.zeros(max(total, 0) + 2 * n, EVENT_DTYPE)
        nev = np.zeros(max(n, 1), np.int32)
        routes = np.zeros(max(n, 1), np.int32)
        t1 = np.zeros(max(total, 1), np.float32) if tstats else None
        t2 = np.zeros(max(total, 1), np.float32) if tstats else None
        if raw.size == 0:
            raw = np.zeros(1, np.int16)
        _check(self._L.sfa_detect_events_device(self._h, raw.ctypes.data_as(C.POINTER(C.c_int16)), ro.ctypes.data_as(_lib.i64p),
                                                sc.ctypes.data_as(C.POINTER(C.c_double)), n, ev.ctypes.data_as(C.c_void_p),
                                                nev.ctypes.data_as(_lib.i32p), routes.ctypes.data_as(_lib.i32p),
                                                t1.ctypes.data_as(_lib.f32p) if tstats else None,
                                                t2.ctypes.data_as(_lib.f32p) if tstats else None), "sfa_detect_events_device")
        tables = [ev[int(ro[i]) + 2 * i:int(ro[i]) + 2 * i + int(nev[i])] for i in range(n)]
        return (tables, routes[:n], t1[:total], t2[:total]) if tstats else (tables, routes[:n])

    def sync(self):
        _check(self._L.sfa_sync(self._h), "sfa_sync")

    def profile(self):
        p = _lib.SfaProfile()
        _check(self._L.sfa_get_profile(self._h, C.byref(p)), "sfa_get_profile")
        return {k: getattr(p, k) for k, _ in _lib.SfaProfile._fields_}

    def stream(self):
        return self._L.sfa_stream(self._h)


SESSION_NO_START = 0x1
SESSION_RESWEEP = 0x4  # (0x2 is unassigned)
SESSION_SPREAD = 0x10  # (and so is 0x8): the slots dealt over the devices of an Aligner made with devices=


def _session_flags(starts, resweep):
    return (0 if starts else SESSION_NO_START) | (SESSION_RESWEEP if resweep else 0)


class Session:
    """Slots whose alignment is extended as their events arrive: after every extend() a slot's row is the row align_db returns
    for all events the slot has received since its last reset.  Belongs to its Aligner: close it first (closing the Aligner frees
    the native session as well, this object is then closed).
    resweep=True: raw mode only (extend() is refused).  A slot is swept when the window W of its normalisation changes
    (recal_window), over events [skip, skip + W) -- reversed on an RNA aligner without INV -- and between such calls its row
    stands: after every extend_raw() the row is align_db of those W events normalised over themselves, and info["q_events"] and
    lengths() report W."""

    def __init__(self, aligner, n_slots, starts=True, resweep=False, flags=None, spread=False):
        self._al = aligner
        self._L = aligner._L
        self._h = C.c_void_p()
        fl = (_session_flags(starts, resweep) if flags is None else int(flags)) | (SESSION_SPREAD if spread else 0)
        self.n_slots, self.starts, self.resweep = int(n_slots), not fl & SESSION_NO_START, bool(fl & SESSION_RESWEEP)
        _check(self._L.sfa_session_create(aligner._h, self.n_slots, fl, C.byref(self._h)), "sfa_session_create")
        self._al_h = aligner._h.value  # the native context this session belongs to

    def _live(self):
        if not self._h or self._al._h.value != self._al_h:
            raise SfaError("the session is closed (or its Aligner is)")

    def extend(self, slots, events, ev_off):
        """Append events[ev_off[i]:ev_off[i+1]] (z-normalised means, event order) to slot slots[i]. -> RESULT_DTYPE[len(slots)]"""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        ev = _f32(events)
        eo = np.ascontiguousarray(ev_off, np.int64)
        n = len(sl)
        if len(eo) != n + 1:
            raise SfaError("extend: ev_off must have one entry more than slots")
        out = np.zeros(n, RESULT_DTYPE)
        if ev.size == 0:
            ev = np.zeros(1, np.float32)
        _check(self._L.sfa_session_extend(self._h, sl.ctypes.data_as(_lib.i32p), ev.ctypes.data_as(_lib.f32p),
                                          eo.ctypes.data_as(_lib.i64p), n, out.ctypes.data_as(C.c_void_p)), "sfa_session_extend")
        return out

    def keep_events(self, max_events):
        """Event mode: keep up to max_events events per slot in device memory (sfa_session_keep_events), the query event_maps()
        reads; n_slots x max_events x 4 bytes (session_keep_bytes).  A slot that outgrows it keeps its rows and loses its maps
        until it is reset.  0 switches it off.  Only while every slot is empty; a raw-mode session keeps its query already."""
        self._live()
        _check(self._L.sfa_session_keep_events(self._h, int(max_events)), "sfa_session_keep_events")

    def event_maps(self, rows, slots):
        """aln_t.r2qevent_map of rows this session returned, computed on the device from the slots' resident queries
        (sfa_session_event_maps): rows[k] is a row of slot slots[k] in its current state -- the primary of the last extend() /
        extend_raw(), or a row of candidates(); a slot may be named several times.  -> (pairs int32 [total, 2], map_off int64
        [len(rows) + 1], n_on_host): the map of row k is pairs[map_off[k]:map_off[k + 1]], start and stop per reference column as
        r2qevent_map returns them; rows without a row (valid = 0) have an empty slice; a row the library wrote nothing for (no
        complete map) keeps INT32_MIN.  n_on_host: rows computed by the host routine inside the call (moves beyond the
        "map_scratch_bytes" budget; a slot beyond 2048 query events too, unless the aligner's option "map_strips" is 1, which runs
        such slots on the device in row strips)."""
        self._live()
        rows = np.ascontiguousarray(rows, RESULT_DTYPE).reshape(-1)
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(rows)
        if len(sl) != n:
            raise SfaError("event_maps: slots must name one slot per row")
        off = map_offsets(rows)
        pairs = np.full((max(int(off[-1]), 1), 2), np.iinfo(np.int32).min, np.int32)
        on_host = C.c_int32(0)
        _check(self._L.sfa_session_event_maps(self._h, rows.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(_lib.i32p), n, off.ctypes.data_as(_lib.i64p),
                                              pairs.ctypes.data_as(_lib.i32p), C.byref(on_host)), "sfa_session_event_maps")
        return pairs[:int(off[-1])], off, int(on_host.value)

    def configure_candidates(self, n):
        """Keep the n = 1..4 candidates behind every slot's row (sfa_session_candidates_config): the secondaries of the batch path,
        for all events a slot has received, however many.  0 switches them off.  Only while every slot is empty."""
        self._live()
        _check(self._L.sfa_session_candidates_config(self._h, int(n)), "sfa_session_candidates_config")

    def candidates(self, slots):
        """The candidates behind the current rows of `slots` -> RESULT_DTYPE[len(slots), 4], best first; valid = 0 for ranks that
        are absent or beyond the configured count, and for slots without events or poisoned."""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros((len(sl), 4), RESULT_DTYPE)
        _check(self._L.sfa_session_candidates(self._h, sl.ctypes.data_as(_lib.i32p), len(sl), out.ctypes.data_as(C.c_void_p)), "sfa_session_candidates")
        return out

    def configure_raw(self, skip=50, norm=100, query=2048, recalibrate=(), at_end=False):
        """Raw mode (sfa_session_raw_config): the session takes samples (extend_raw) and runs event detection and normalisation on
        the device.  The first `skip` final events of a slot are dropped, mean and sd over the next `norm` are frozen, the slot is
        full at `query` query events.  Only while every slot is empty.
        recalibrate: ascending window lengths, norm < ... <= query (sfa_session_raw_recalibrate): when a slot reaches one, it is
        normalised over that many events and swept again from event 0 inside the call; at_end: a read that ends with 25 <= events -
        skip < query is normalised over all of them.  The window after any call is recal_window(); info["norm_window"] reports it."""
        self._live()
        _check(self._L.sfa_session_raw_config(self._h, int(skip), int(norm), int(query)), "sfa_session_raw_config")
        self.raw_shape = (int(skip), int(norm), int(query))
        if len(recalibrate) or at_end:
            self.recalibrate(recalibrate, at_end)

    def recalibrate(self, at=(), at_end=False, flags=None):
        """sfa_session_raw_recalibrate on a raw-mode session whose slots are all empty; at=() and at_end=False switch it off.
        flags: the raw flag word in place of at_end."""
        self._live()
        pts = np.ascontiguousarray(at, np.int32).reshape(-1)
        fl = (RECAL_AT_END if at_end else 0) if flags is None else int(flags)
        _check(self._L.sfa_session_raw_recalibrate(self._h, pts.ctypes.data_as(_lib.i32p) if len(pts) else None, len(pts), fl), "sfa_session_raw_recalibrate")

    def configure_auto_start(self, every, max_samples):
        """The RNA automatic query start (-p -1) as the read streams (sfa_session_raw_auto_start), on a resweep session in raw mode
        over an RNA aligner without INV / END, while every slot is empty: the target of a slot is auto_start_target() of its
        first N samples at N = every, 2 every, ... <= max_samples and at one final point (end of read, or max_samples samples),
        frozen at the first point that gives one; its skip is the first event at or behind the target, or the fallback 50.  The
        skip given to configure_raw() is the largest skip a slot may resolve.  max_samples=0 switches it off."""
        self._live()
        _check(self._L.sfa_session_raw_auto_start(self._h, int(every), int(max_samples), 0), "sfa_session_raw_auto_start")

    def auto_start(self, slots):
        """The automatic start of `slots` as the last call left it -> SESSION_AUTO_DTYPE[len(slots)]: target sample (-1), the point
        it was frozen at, skip (-1 while unresolved), status (AUTO_* | AUTO_AT_FINAL)."""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros(len(sl), SESSION_AUTO_DTYPE)
        _check(self._L.sfa_session_auto_start(self._h, sl.ctypes.data_as(_lib.i32p), len(sl), out.ctypes.data_as(C.c_void_p)), "sfa_session_auto_start")
        return out

    def auto_ms(self):
        """Device ms the feature's own kernels (retention, evaluation) took in the last extend_raw call (sfa_session_auto_ms)."""
        self._live()
        return float(self._L.sfa_session_auto_ms(self._h))

    def extend_raw(self, slots, raw, raw_off, scaling, end=None):
        """Append raw[raw_off[i]:raw_off[i+1]] (int16 samples) to slot slots[i]; scaling[i] = (digitisation, offset, range); end[i]
        true: the read of slot i ends behind these samples. -> (RESULT_DTYPE[len(slots)], SESSION_RAW_INFO_DTYPE[len(slots)])"""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = len(sl)
        rw = np.ascontiguousarray(raw, np.int16).reshape(-1)
        ro = np.ascontiguousarray(raw_off, np.int64)
        sc = np.ascontiguousarray(scaling, np.float64).reshape(-1)
        if len(ro) != n + 1 or len(sc) != 3 * n:
            raise SfaError("extend_raw: raw_off must have one entry more than slots, scaling three per slot")
        en = None if end is None else np.ascontiguousarray(end, np.uint8).reshape(-1)
        if en is not None and len(en) != n:
            raise SfaError("extend_raw: end must have one entry per slot")
        if rw.size == 0:
            rw = np.zeros(1, np.int16)
        out, info = np.zeros(n, RESULT_DTYPE), np.zeros(n, SESSION_RAW_INFO_DTYPE)
        _check(self._L.sfa_session_extend_raw(self._h, sl.ctypes.data_as(_lib.i32p), rw.ctypes.data_as(C.POINTER(C.c_int16)),
                                              ro.ctypes.data_as(_lib.i64p), sc.ctypes.data_as(C.POINTER(C.c_double)),
                                              None if en is None else en.ctypes.data_as(C.POINTER(C.c_uint8)), n,
                                              out.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p)), "sfa_session_extend_raw")
        return out, info

    def events(self, slot):
        """The final events of `slot` (raw mode) as an EVENT_DTYPE array: means in pA, `start` in samples since the slot's reset."""
        self._live()
        n = int(self._L.sfa_session_events(self._h, int(slot), 0, None, 0))
        if n < 0:
            _check(n, "sfa_session_events")
        out = np.zeros(n, EVENT_DTYPE)
        if n:
            n = int(self._L.sfa_session_events(self._h, int(slot), 0, C.cast(out.ctypes.data, C.POINTER(_lib.SfaEvent)), n))
            if n < 0:
                _check(n, "sfa_session_events")
        return out

    def query_span(self, slots):
        """Raw coordinates of the queries of `slots` (raw mode, sfa_session_query_span): (start, end) as uint64 arrays -- the start
        of final event `skip` and start + length of the last query event swept, in samples since the slot's reset; 0 / 0 for a slot
        that is not calibrated.  What paf_row takes as start_raw / end_raw."""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        a, b = np.zeros(len(sl), np.uint64), np.zeros(len(sl), np.uint64)
        u64p = C.POINTER(C.c_uint64)
        _check(self._L.sfa_session_query_span(self._h, sl.ctypes.data_as(_lib.i32p), len(sl), a.ctypes.data_as(u64p), b.ctypes.data_as(u64p)),
               "sfa_session_query_span")
        return a, b

    def set_targets(self, intervals):
        """The session's targets (sfa_session_targets): (contig, begin, end) triples or a TARGET_DTYPE array, [begin, end) in the
        coordinates rows report (pos_st / pos_end: after the strand flip and ref_st_offset); they may overlap, touch and come in
        any order.  A column is on target when the coordinate a row reports for an alignment ENDING in it lies in an interval of
        its contig.  An empty list switches the feature off.  Allowed at any time; refused on a resweep session.  The mask takes
        total_columns / 8 bytes of device memory, once per session."""
        self._live()
        t = _targets(intervals)
        _check(self._L.sfa_session_targets(self._h, t.ctypes.data_as(C.POINTER(_lib.SfaTarget)) if len(t) else None, len(t)), "sfa_session_targets")

    def set_reach_targets(self, targets):
        """The session's targets from a reach list (sfa_session_targets_reach): (contig, begin, end, lead, strand) tuples -- strand
        '+', '-', or None / '.' / 0 for both -- or a REACH_TARGET_DTYPE array.  A column of a '+' job is on target when its
        coordinate x has begin - lead <= x < end for a target of its contig and strand, a column of a '-' job when
        begin <= x < end + lead: the lead is the stretch IN FRONT of the target, in the direction the read goes on.  Its anchor
        is the first base of a target the read will reach; under configure_coverage() a column stays live while the depth of its
        ANCHOR lies below the cap.  It replaces the mask of set_targets(), which replaces it in turn; a depth track is kept
        across both.  An empty list switches targets off.  session_reach_bytes() of memory beside the mask."""
        self._live()
        t = _reach_targets(targets)
        _check(self._L.sfa_session_targets_reach(self._h, t.ctypes.data_as(C.POINTER(_lib.SfaReachTarget)) if len(t) else None, len(t)), "sfa_session_targets_reach")

    def reach_tables(self):
        """The base mask and the anchors of a reach session as the device holds them (sfa_session_reach_tables) ->
        (bool[total columns], int32[total columns]): the anchor of a column as an index into its contig's depth track
        (coordinate - st_offset), REACH_NONE off target, REACH_BELOW_TRACK for an anchor below st_offset."""
        self._live()
        cols = int(np.sum(self._al.ref.ref_lengths)) * (1 if self._al.flag & RNA else 2)
        words = np.zeros((cols + 31) // 32 + 1, np.uint32)
        anchor = np.zeros(cols, np.int32)
        _check(self._L.sfa_session_reach_tables(self._h, words.ctypes.data_as(C.POINTER(C.c_uint32)), len(words), anchor.ctypes.data_as(_lib.i32p), cols),
               "sfa_session_reach_tables")
        if words[-1] != 0:
            raise SfaError("sfa_session_reach_tables: the spare word behind the mask is not zero")
        bits = (words[:-1, None] >> np.arange(32, dtype=np.uint32)[None, :]) & np.uint32(1)
        return bits.reshape(-1)[:cols].astype(bool), anchor

    def target_columns(self):
        """Columns of a slot's row that are on target (0 without targets)."""
        self._live()
        n = int(self._L.sfa_session_target_columns(self._h))
        if n < 0:
            _check(n, "sfa_session_target_columns")
        return n

    def classes(self, slots):
        """The best on-target and the best off-target column of the carried rows of `slots` (sfa_session_classes) ->
        CLASS_DTYPE[len(slots)]: score, contig, coordinate and strand of either; an empty class has score +inf and rid -1; ties go
        to the lowest cost, then the lowest column of the row (jobs in order, '+' before '-').  valid = 0: the slot is empty or
        poisoned.  A slot may be named once."""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros(len(sl), CLASS_DTYPE)
        _check(self._L.sfa_session_classes(self._h, sl.ctypes.data_as(_lib.i32p), len(sl), out.ctypes.data_as(C.c_void_p)), "sfa_session_classes")
        return out

    def set_target_groups(self, intervals, n_groups):
        """The session's target groups (sfa_session_target_groups): (contig, begin, end, group) tuples or a GROUP_TARGET_DTYPE
        array with 0 <= group < n_groups <= 1023, intervals as for set_targets.  A column belongs to the lowest group id among
        the intervals that cover it, or to the background (index n_groups).  An empty list switches the feature off.  Allowed at
        any time, beside a mask or without one; refused on a resweep session.  The label table takes 2 * total_columns bytes of
        device memory, once per session."""
        self._live()
        t = _group_targets(intervals)
        _check(self._L.sfa_session_target_groups(self._h, t.ctypes.data_as(C.POINTER(_lib.SfaGroupTarget)) if len(t) else None, len(t), int(n_groups)),
               "sfa_session_target_groups")

    def set_reach_target_groups(self, targets, n_groups):
        """The session's target groups from a reach group list (sfa_session_target_groups_reach): (contig, begin, end, lead,
        group, strand) tuples -- strand as for set_reach_targets -- or a REACH_GROUP_TARGET_DTYPE array, 0 <= group < n_groups
        <= 1023.  Admission and the anchor of a column are set_reach_targets'; the label of a column is the lowest group among
        the admitting targets the read reaches first (whose own anchor is the column's), the background (n_groups) where nobody
        admits it.  It replaces the label table of set_target_groups(), which replaces it in turn.  group_bests(), open_classes()
        and group_count() work unchanged; under configure_group_coverage() a column stays live while the depth of its ANCHOR lies
        below the cap, and group_coverage() counts the '+' jobs' body columns only.  An empty list switches groups off.
        session_group_reach_bytes() of memory."""
        self._live()
        t = _reach_group_targets(targets)
        _check(self._L.sfa_session_target_groups_reach(self._h, t.ctypes.data_as(C.POINTER(_lib.SfaReachGroupTarget)) if len(t) else None, len(t), int(n_groups)),
               "sfa_session_target_groups_reach")

    def group_reach_tables(self):
        """The base label table and its anchors of a session with reach groups as the device holds them
        (sfa_session_group_reach_tables) -> (uint16[total columns], int32[total columns]): the anchor of a column as an index into
        its contig's depth track, REACH_NONE for a background column, REACH_BELOW_TRACK for an anchor below st_offset."""
        self._live()
        cols = int(np.sum(self._al.ref.ref_lengths)) * (1 if self._al.flag & RNA else 2)
        label = np.zeros(cols, np.uint16)
        anchor = np.zeros(cols, np.int32)
        _check(self._L.sfa_session_group_reach_tables(self._h, label.ctypes.data_as(C.POINTER(C.c_uint16)), anchor.ctypes.data_as(_lib.i32p), cols),
               "sfa_session_group_reach_tables")
        return label, anchor

    def group_count(self):
        """n_groups of the session (0 without groups)."""
        self._live()
        n = int(self._L.sfa_session_group_count(self._h))
        if n < 0:
            _check(n, "sfa_session_group_count")
        return n

    def group_bests(self, slots):
        """The best column of every group and of the background in the carried rows of `slots` (sfa_session_group_bests) ->
        (GROUP_BEST_DTYPE[len(slots), n_groups + 1], GROUP_HEAD_DTYPE[len(slots)]): an entry without columns has score +inf and
        rid -1; a head names the two best entries (-1: none); ties as for classes.  valid = 0: the slot is empty or poisoned."""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        bests = np.zeros((len(sl), self.group_count() + 1), GROUP_BEST_DTYPE)
        heads = np.zeros(len(sl), GROUP_HEAD_DTYPE)
        _check(self._L.sfa_session_group_bests(self._h, sl.ctypes.data_as(_lib.i32p), len(sl), bests.ctypes.data_as(C.c_void_p), heads.ctypes.data_as(C.c_void_p)),
               "sfa_session_group_bests")
        return bests, heads

    def open_classes(self, slots, open=None):
        """The class results of `slots` under a bitmap of open groups (sfa_session_open_classes) -> OPEN_CLASS_DTYPE[len(slots)].
        open: uint32[open_words(n_groups)], bit g % 32 of word g // 32 set: group g is open; None: every group is.  A column is ON
        when its label is a group whose bit is set, OFF otherwise (closed groups, the background).  `cls` is a CLASS_DTYPE record
        filled as classes() fills it (target_decide takes it); on_group / off_group are the labels of the two best columns
        (off_group n_groups: the background; -1: the class has no column).  Needs target groups, no mask."""
        self._live()
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros(len(sl), OPEN_CLASS_DTYPE)
        bits = None if open is None else np.ascontiguousarray(open, np.uint32).reshape(-1)
        _check(self._L.sfa_session_open_classes(self._h, sl.ctypes.data_as(_lib.i32p), len(sl), None if bits is None else bits.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                0 if bits is None else len(bits), out.ctypes.data_as(C.c_void_p)), "sfa_session_open_classes")
        return out

    def configure_coverage(self, cap):
        """A coverage cap on the session's targets (sfa_session_coverage_config): cap >= 1 switches it on -- a depth track per
        contig on the device, zeroed, and a live mask beside the mask of set_targets -- and 0 switches it off and frees both.  A
        column is live while it is on target and the depth of the coordinate it reports lies below cap; classes() and
        target_columns() then read the live mask.  Needs targets; allowed at any time.  session_coverage_bytes() of memory."""
        self._live()
        _check(self._L.sfa_session_coverage_config(self._h, int(cap)), "sfa_session_coverage_config")

    def add_coverage(self, intervals):
        """depth += 1 over every interval ((contig, begin, end) triples or a TARGET_DTYPE array, as for set_targets; they may
        overlap), then the live mask is derived again (sfa_session_coverage_add) -> the live on-target columns.  An empty list
        adds nothing and derives the mask."""
        self._live()
        t = _targets(intervals)
        n_open = C.c_int64(0)
        _check(self._L.sfa_session_coverage_add(self._h, t.ctypes.data_as(C.POINTER(_lib.SfaTarget)) if len(t) else None, len(t), C.byref(n_open)),
               "sfa_session_coverage_add")
        return int(n_open.value)

    def coverage(self, contig):
        """The depth track of `contig` (sfa_session_coverage_depth) -> uint32[ref_length + 1]: entry x - st_offset is the depth of
        coordinate x, both strands together."""
        self._live()
        c = int(contig)
        n = int(self._al.ref.ref_lengths[c]) + 1 if 0 <= c < len(self._al.ref.ref_lengths) else 1
        out = np.zeros(n, np.uint32)
        _check(self._L.sfa_session_coverage_depth(self._h, c, out.ctypes.data_as(C.POINTER(C.c_uint32)), n), "sfa_session_coverage_depth")
        return out

    def configure_group_coverage(self, cap):
        """A depth cap on the session's target groups (sfa_session_group_coverage_config): cap >= 1 switches it on -- a live label
        table beside the table of set_target_groups, derived from the session's one depth track -- and 0 switches it off.  The
        live label of a column is its base label while the depth of the coordinate it reports lies below cap, the background
        from then on; open_classes() and group_bests() then read the live table.  Needs groups, no mask; the track is shared with
        configure_coverage(), whose cap is a number of its own.  add_coverage() and coverage() work with either cap set.
        session_group_coverage_bytes() of memory."""
        self._live()
        _check(self._L.sfa_session_group_coverage_config(self._h, int(cap)), "sfa_session_group_coverage_config")

    def group_coverage(self):
        """How deep every group is (sfa_session_group_coverage) -> GROUP_COVER_DTYPE[n_groups + 1], the background last: columns,
        capped (depth >= the group cap), depth_sum, depth_min, depth_max over the forward-strand columns whose BASE label is the
        entry.  An entry without columns: 0, 0, 0, 2^32 - 1, 0."""
        self._live()
        out = np.zeros(self.group_count() + 1, GROUP_COVER_DTYPE)
        _check(self._L.sfa_session_group_coverage(self._h, out.ctypes.data_as(C.POINTER(_lib.SfaGroupCover)), len(out)), "sfa_session_group_coverage")
        return out

    def reset(self, slots=None):
        """Forget the events of `slots` (None: of every slot); in raw mode the detector, normalisation and scaling as well."""
        self._live()
        if slots is None:
            _check(self._L.sfa_session_reset(self._h, None, 0), "sfa_session_reset")
            return
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        _check(self._L.sfa_session_reset(self._h, sl.ctypes.data_as(_lib.i32p), len(sl)), "sfa_session_reset")

    def lengths(self, slots=None):
        """Events received since the last reset, int64 per slot of `slots` (None: every slot in order)."""
        self._live()
        sl = None if slots is None else np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = self.n_slots if sl is None else len(sl)
        out = np.zeros(n, np.int64)
        _check(self._L.sfa_session_lengths(self._h, None if sl is None else sl.ctypes.data_as(_lib.i32p), n,
                                           out.ctypes.data_as(_lib.i64p)), "sfa_session_lengths")
        return out

    def row(self, slot, contig, strand):
        """The carried row of (slot, contig, strand '+' or '-') read back (sfa_session_row): (cost float32[ref_length], start
        int32[ref_length] or None without starts).  Start columns are as stored: columns of the strand's own array, before the
        flip of '-' and before ref_st_offset."""
        self._live()
        ch = ord(strand) if isinstance(strand, str) else int(strand)
        n = int(self._al.ref.ref_lengths[contig]) if 0 <= int(contig) < len(self._al.ref.ref_lengths) else 1
        cost = np.zeros(n, np.float32)
        start = np.zeros(n, np.int32) if self.starts else None
        got = int(self._L.sfa_session_row(self._h, int(slot), int(contig), ch, cost.ctypes.data_as(_lib.f32p),
                                          None if start is None else start.ctypes.data_as(_lib.i32p)))
        if got < 0:
            _check(got, "sfa_session_row")
        return cost, start

    def close(self):
        if self._h and self._al._h.value == self._al_h:  # (an Aligner that was closed took its sessions with it)
            self._L.sfa_session_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _targets(intervals):
    if isinstance(intervals, np.ndarray) and intervals.dtype == TARGET_DTYPE:
        return np.ascontiguousarray(intervals).reshape(-1)
    t = np.zeros(len(intervals), TARGET_DTYPE)
    for k, (contig, begin, end) in enumerate(intervals):
        t[k] = (int(contig), int(begin), int(end))
    return t


def _reach_targets(targets):
    if isinstance(targets, np.ndarray) and targets.dtype == REACH_TARGET_DTYPE:
        return np.ascontiguousarray(targets).reshape(-1)
    t = np.zeros(len(targets), REACH_TARGET_DTYPE)
    for k, (contig, begin, end, lead, strand) in enumerate(targets):
        code = 0 if strand in (None, 0, ".", "") else (ord(strand) if isinstance(strand, str) and len(strand) == 1 else int(strand))
        if not -128 <= code <= 127:
            raise SfaError(f"reach target {k}: strand {strand!r} is none of None, '+', '-'")
        t[k] = (int(contig), int(begin), int(end), int(lead), code, (0, 0, 0))
    return t


def _reach_group_targets(targets):
    if isinstance(targets, np.ndarray) and targets.dtype == REACH_GROUP_TARGET_DTYPE:
        return np.ascontiguousarray(targets).reshape(-1)
    t = np.zeros(len(targets), REACH_GROUP_TARGET_DTYPE)
    for k, (contig, begin, end, lead, group, strand) in enumerate(targets):
        code = 0 if strand in (None, 0, ".", "") else (ord(strand) if isinstance(strand, str) and len(strand) == 1 else int(strand))
        if not -128 <= code <= 127:
            raise SfaError(f"reach group target {k}: strand {strand!r} is none of None, '+', '-'")
        t[k] = (int(contig), int(begin), int(end), int(lead), int(group), code, (0, 0, 0))
    return t


def _group_targets(intervals):
    if isinstance(intervals, np.ndarray) and intervals.dtype == GROUP_TARGET_DTYPE:
        return np.ascontiguousarray(intervals).reshape(-1)
    t = np.zeros(len(intervals), GROUP_TARGET_DTYPE)
    for k, (contig, begin, end, group) in enumerate(intervals):
        t[k] = (int(contig), int(begin), int(end), int(group))
    return t


def group_decide(head, min_events, margin):
    """The decision from one GROUP_HEAD_DTYPE record (sfa_group_decide; host arithmetic): the index of the best entry (a group,
    or n_groups for the background) when n_events >= min_events and second_score - best_score >= margin * n_events (no
    runner-up counts as +inf); None otherwise.  margin is a cost per z-normalised event; there is no default."""
    rec = np.ascontiguousarray(head, GROUP_HEAD_DTYPE).reshape(-1)
    if len(rec) != 1:
        raise SfaError("group_decide: one head record at a time")
    got = int(_lib.load().sfa_group_decide(C.cast(rec.ctypes.data, C.POINTER(_lib.SfaGroupHead)), int(min_events), float(margin)))
    return got if got >= 0 else None


def open_words(n_groups):
    """Words of 32 bits in the bitmap of open groups of a session with n_groups groups."""
    return (int(n_groups) + 31) // 32


class QuotaBook:
    """Who has enough (the twin of quota_rules.hpp's QuotaBook; host arithmetic only): a quota and an accepted count per group and
    the bitmap of open groups Session.open_classes takes.  A quota of 0 is unlimited."""

    def __init__(self, n_groups, quota=0):
        self.n_groups = int(n_groups)
        self.quota = [int(quota)] * self.n_groups
        self.accepted = [0] * self.n_groups
        self.open = np.zeros(open_words(self.n_groups), np.uint32)
        for g in range(self.n_groups):
            self.open[g >> 5] |= np.uint32(1 << (g & 31))

    def is_open(self, group):
        return 0 <= group < self.n_groups and bool((int(self.open[group >> 5]) >> (group & 31)) & 1)

    def note_accept(self, group):
        """One accepted read of `group` (the background and -1 count nowhere) -> True when this read closed the group."""
        if not 0 <= group < self.n_groups:
            return False
        self.accepted[group] += 1
        if self.quota[group] <= 0 or self.accepted[group] < self.quota[group] or not self.is_open(group):
            return False
        self.open[group >> 5] &= np.uint32(~(1 << (group & 31)) & 0xffffffff)
        return True


def target_decide(cls, mode, min_events, margin):
    """The decision from one CLASS_DTYPE record (sfa_target_decide; host arithmetic): with n = n_events >= min_events,
    off_score - on_score >= margin * n says on target and on_score - off_score >= margin * n off target; mode ENRICH: on target
    -> 'A' (accept), off target -> 'U' (unblock); DEPLETE the other way round; None: no decision.  margin is a cost per
    z-normalised event; no good value has been measured, so there is no default."""
    rec = np.ascontiguousarray(cls, CLASS_DTYPE).reshape(-1)
    if len(rec) != 1:
        raise SfaError("target_decide: one class record at a time")
    got = int(_lib.load().sfa_target_decide(C.cast(rec.ctypes.data, C.POINTER(_lib.SfaClass)), int(mode), int(min_events), float(margin)))
    return chr(got) if got else None


def read_targets(path, names):
    """A BED file as targets for Session.set_targets -> TARGET_DTYPE array: three columns (name, begin, end; further columns are
    ignored), blank lines and lines that begin with '#', 'track' or 'browser' skipped.  names: the reference's contig names in
    order (RefModel.names).  A contig that is not among them, a line with fewer than three columns or a coordinate that is no
    integer is an error; the intervals themselves are checked by set_targets."""
    index = {str(n): i for i, n in enumerate(names)}
    out = []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith("#") or text.split()[0] in ("track", "browser"):
                continue
            f = text.split("\t") if "\t" in text else text.split()
            if len(f) < 3:
                raise SfaError(f"read_targets: {path}:{no}: a BED line has at least three columns")
            if f[0] not in index:
                raise SfaError(f"read_targets: {path}:{no}: contig {f[0]!r} is not in the reference")
            try:
                out.append((index[f[0]], int(f[1]), int(f[2])))
            except ValueError:
                raise SfaError(f"read_targets: {path}:{no}: begin and end must be integers") from None
    return _targets(out)


def read_reach_targets(path, names, lead, stranded=False):
    """A BED file as reach targets for Session.set_reach_targets -> REACH_TARGET_DTYPE array: the dialect of read_targets, every
    target with the lead `lead` (0 .. 2^30).  stranded: column 6 is the target's strand -- '+', '-', or '.' for both; a line
    without it, or with anything else there, is an error.  Without `stranded` every target is for both strands."""
    if isinstance(lead, bool) or not isinstance(lead, (int, np.integer)) or not 0 <= int(lead) <= REACH_LEAD_MAX:
        raise SfaError(f"read_reach_targets: lead should be an integer 0..{REACH_LEAD_MAX}, not {lead!r}")
    index = {str(n): i for i, n in enumerate(names)}
    out = []
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith("#") or text.split()[0] in ("track", "browser"):
                continue
            f = text.split("\t") if "\t" in text else text.split()
            if len(f) < 3:
                raise SfaError(f"read_reach_targets: {path}:{no}: a BED line has at least three columns")
            if f[0] not in index:
                raise SfaError(f"read_reach_targets: {path}:{no}: contig {f[0]!r} is not in the reference")
            strand = None
            if stranded:
                if len(f) < 6:
                    raise SfaError(f"read_reach_targets: {path}:{no}: the line has no sixth column (the strand)")
                if f[5] not in ("+", "-", "."):
                    raise SfaError(f"read_reach_targets: {path}:{no}: strand {f[5]!r} is none of '+', '-', '.'")
                strand = None if f[5] == "." else f[5]
            try:
                out.append((index[f[0]], int(f[1]), int(f[2]), int(lead), strand))
            except ValueError:
                raise SfaError(f"read_reach_targets: {path}:{no}: begin and end must be integers") from None
    return _reach_targets(out)


def read_target_groups(path, names):
    """A BED file as group targets for Session.set_target_groups -> (GROUP_TARGET_DTYPE array, group names): the dialect of
    read_targets, with column 4 the group's name; groups are numbered by first appearance.  A line without a fourth column and
    more than 1023 names are errors, beside those of read_targets."""
    index = {str(n): i for i, n in enumerate(names)}
    out, groups = [], {}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            text = line.strip()
            if not text or text.startswith("#") or text.split()[0] in ("track", "browser"):
                continue
            f = text.split("\t") if "\t" in text else text.split()
            if len(f) < 3:
                raise SfaError(f"read_target_groups: {path}:{no}: a BED line has at least three columns")
            if len(f) < 4 or not f[3].strip():
                raise SfaError(f"read_target_groups: {path}:{no}: the line has no fourth column (the group's name)")
            if f[0] not in index:
                raise SfaError(f"read_target_groups: {path}:{no}: contig {f[0]!r} is not in the reference")
            name = f[3].strip()
            if name not in groups:
                if len(groups) == GROUP_MAX:
                    raise SfaError(f"read_target_groups: {path}:{no}: more than {GROUP_MAX} group names")
                groups[name] = len(groups)
            try:
                out.append((index[f[0]], int(f[1]), int(f[2]), groups[name]))
            except ValueError:
                raise SfaError(f"read_target_groups: {path}:{no}: begin and end must be integers") from None
    return _group_targets(out), list(groups)


def read_reach_target_groups(path, names, lead, stranded=False):
    """A BED file as reach group targets for Session.set_reach_target_groups -> (REACH_GROUP_TARGET_DTYPE array, group names):
    read_target_groups' dialect and numbering of the names (column 4), every target with the lead `lead` (0 .. 2^30).  stranded:
    column 6 is the target's strand as in read_reach_targets; without it every target is for both strands."""
    if isinstance(lead, bool) or not isinstance(lead, (int, np.integer)) or not 0 <= int(lead) <= REACH_LEAD_MAX:
        raise SfaError(f"read_reach_target_groups: lead should be an integer 0..{REACH_LEAD_MAX}, not {lead!r}")
    try:
        plain, groups = read_target_groups(path, names)
        strands = read_reach_targets(path, names, int(lead), stranded=True)["strand"] if stranded else 0
    except SfaError as e:
        raise SfaError(str(e).replace("read_target_groups:", "read_reach_target_groups:").replace("read_reach_targets:", "read_reach_target_groups:")) from None
    t = np.zeros(len(plain), REACH_GROUP_TARGET_DTYPE)
    for f in ("contig", "begin", "end", "group"):
        t[f] = plain[f]
    t["lead"] = int(lead)
    t["strand"] = strands
    return t, groups


def read_truth(path, names):
    """A PAF file as the truth of replay(truth=) -> {read id: (contig index, begin, end)}, (-1, 0, 0) for a read that belongs nowhere
    (the twin of truth_rules.hpp's TruthTable; what `sigfish-amd eval` takes as truth): column 1 the read id, column 6 the contig's
    name (`*`: the read belongs nowhere, its coordinates are not read), columns 8 and 9 begin and end on the forward strand, 0-based
    and half open.  Empty lines are skipped.  names: the reference's contig names in order.  Fewer than 9 tab-separated columns, a
    coordinate that is no integer in 0 .. 2^31 - 1, end <= begin, a contig that is not among the names and a read id that appears
    twice are errors, each with file name and line number.  A read that is not in the file has no truth."""
    index = {}
    for i, n in enumerate(names):
        index[str(n)] = i  # (a name held twice: the last one, as the binary looks it up)
    out = {}
    with open(path, newline="") as fh:
        for no, line in enumerate(fh.read().split("\n"), 1):
            if line.endswith("\r"):
                line = line[:-1]
            if not line:
                continue
            f = line.split("\t")
            if len(f) < 9:
                raise SfaError(f"read_truth: {path}:{no}: a PAF line has at least 9 tab-separated columns (this one has {len(f)})")
            if not f[0]:
                raise SfaError(f"read_truth: {path}:{no}: the read id (column 1) is empty")
            if f[5] == "*":
                rec = (-1, 0, 0)
            else:
                if f[5] not in index:
                    raise SfaError(f"read_truth: {path}:{no}: contig {f[5]!r} is not in the reference")
                digits = lambda s: 0 < len(s) <= 10 and all("0" <= c <= "9" for c in s) and int(s) <= 2 ** 31 - 1
                if not digits(f[7]) or not digits(f[8]):
                    raise SfaError(f"read_truth: {path}:{no}: begin and end (columns 8 and 9) must be integers in 0 .. 2147483647")
                if int(f[8]) <= int(f[7]):
                    raise SfaError(f"read_truth: {path}:{no}: the interval [{f[7]}, {f[8]}) is empty")
                rec = (index[f[5]], int(f[7]), int(f[8]))
            if f[0] in out:
                raise SfaError(f"read_truth: {path}:{no}: read id {f[0]!r} appears twice")
            out[f[0]] = rec
    return out


def _target_ptr(t):
    return C.cast(t.ctypes.data, C.POINTER(_lib.SfaTarget)) if len(t) else None


def truth_class(targets, contig, begin, end):
    """'T' when [begin, end) of `contig` shares a base with one of `targets` (TARGET_DTYPE, or (contig, begin, end) triples), else 'O'
    -- also for contig < 0, a read that belongs nowhere (sfa_truth_class; host arithmetic)."""
    t = _targets(targets)
    return chr(_lib.load().sfa_truth_class(_target_ptr(t), len(t), int(contig), int(begin), int(end)))


def truth_edge(targets, contig, begin, end):
    """True for a read that overlaps a target but is contained in no single one (sfa_truth_edge): its class decision may honestly
    go either way."""
    t = _targets(targets)
    return bool(_lib.load().sfa_truth_edge(_target_ptr(t), len(t), int(contig), int(begin), int(end)))


def truth_group(group_targets, n_groups, contig, begin, end):
    """The lowest group id among the group targets [begin, end) of `contig` overlaps, else n_groups, the background
    (sfa_truth_group)."""
    t = _group_targets(group_targets)
    ptr = C.cast(t.ctypes.data, C.POINTER(_lib.SfaGroupTarget)) if len(t) else None
    return int(_lib.load().sfa_truth_group(ptr, len(t), int(n_groups), int(contig), int(begin), int(end)))


def truth_verdict(decided, truth):
    """'C' when the decided class ('T', 'O'; anything else is none) equals the true one, 'W' when it differs, 'N' when either is
    none (sfa_truth_verdict)."""
    code = lambda c: ord(c) if isinstance(c, str) and len(c) == 1 else 0
    return chr(_lib.load().sfa_truth_verdict(code(decided), code(truth)))


def truth_group_verdict(decided, truth):
    """The same over two entries (a group id, or n_groups for the background; negative or None: none) (sfa_truth_group_verdict)."""
    return chr(_lib.load().sfa_truth_group_verdict(-1 if decided is None else int(decided), -1 if truth is None else int(truth)))


def session_bytes(total_columns, n_slots, starts=True, resweep=False):
    """Device memory the carried rows of a session take (sfa_session_bytes; host arithmetic, no GPU needed): RefModel.total_columns()
    x n_slots x 8 bytes, x 4 without starts; the same with resweep (a window beyond 2048 events runs as pieces over a carried row)."""
    b = int(_lib.load().sfa_session_bytes(int(total_columns), int(n_slots), _session_flags(starts, resweep)))
    if b < 0:
        raise SfaError(f"sfa_session_bytes failed ({b}): total_columns and n_slots must be positive")
    return b


def map_offsets(rows):
    """The map_off of rows for event_maps: int64 [len(rows) + 1], pos_end - pos_st + 1 pairs for every mapped row, none otherwise."""
    rows = np.ascontiguousarray(rows, RESULT_DTYPE).reshape(-1)
    ok = (rows["valid"] != 0) & (rows["rid"] >= 0)
    size = np.maximum(np.where(ok, rows["pos_end"].astype(np.int64) - rows["pos_st"] + 1, 0), 0)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(size, out=off[1:])
    return off


def session_keep_bytes(n_slots, max_events):
    """Device memory Session.keep_events takes (sfa_session_keep_bytes; host arithmetic): n_slots x max_events x 4 bytes."""
    b = int(_lib.load().sfa_session_keep_bytes(int(n_slots), int(max_events)))
    if b < 0:
        raise SfaError(f"sfa_session_keep_bytes failed ({b}): n_slots and max_events must be positive, their product x 4 below 2^63")
    return b


def session_coverage_bytes(ref, flag=0):
    """Device memory Session.configure_coverage takes for a RefModel (sfa_session_coverage_bytes; host arithmetic): 4 bytes per
    coordinate (ref_length + 1 per contig) and a second mask of total_columns / 8 bytes."""
    cref, _keep = ref._as_c()
    return int(_lib.load().sfa_session_coverage_bytes(C.byref(cref), int(flag)))


def session_group_reach_bytes(ref, flag=0):
    """Device memory Session.set_reach_target_groups takes for a RefModel (sfa_session_group_reach_bytes; host arithmetic): the
    label table's 2 and the anchors' 4 bytes per column."""
    cref, _keep = ref._as_c()
    return int(_lib.load().sfa_session_group_reach_bytes(C.byref(cref), int(flag)))


def session_reach_bytes(ref, flag=0):
    """Device memory Session.set_reach_targets takes beside the mask for a RefModel (sfa_session_reach_bytes; host arithmetic):
    4 bytes per column, the anchors."""
    cref, _keep = ref._as_c()
    return int(_lib.load().sfa_session_reach_bytes(C.byref(cref), int(flag)))


def session_group_coverage_bytes(ref, n_groups, flag=0):
    """Device memory Session.configure_group_coverage takes for a RefModel with n_groups groups (sfa_session_group_coverage_bytes;
    host arithmetic): the depth tracks (shared with configure_coverage), a second label table and 36 bytes per entry."""
    cref, _keep = ref._as_c()
    return int(_lib.load().sfa_session_group_coverage_bytes(C.byref(cref), int(flag), int(n_groups)))


def session_raw_bytes(n_slots, skip=50, query=2048):
    """Device memory raw mode adds to session_bytes (sfa_session_raw_bytes; host arithmetic): per slot (skip + query) x 24 bytes of
    events, query x 4 bytes of query, 592 bytes of detector state."""
    b = int(_lib.load().sfa_session_raw_bytes(int(n_slots), int(skip), int(query)))
    if b < 0:
        raise SfaError(f"sfa_session_raw_bytes failed ({b}): n_slots and query must be positive, skip not negative")
    return b


def session_auto_bytes(n_slots, max_samples):
    """Device memory the automatic query start adds to a session (sfa_session_auto_bytes; host arithmetic): per slot max_samples x 2
    bytes of samples, 16 bytes of state, (max_samples + 1) x 4 bytes of prefix sums for a call in which every slot has a point."""
    b = int(_lib.load().sfa_session_auto_bytes(int(n_slots), int(max_samples)))
    if b < 0:
        raise SfaError(f"sfa_session_auto_bytes failed ({b}): n_slots and max_samples must be positive, max_samples at most 2^20")
    return b


class EventStream:
    """The event detector fed a read in chunks, on the host (sfa_event_stream_*): push() returns the events the new samples made
    final -- each equal, bit for bit, to the same event of detect_events over the complete read -- and finish() the rest."""

    def __init__(self, meta, rna=False):
        self._L = _lib.load()
        self._h = self._L.sfa_event_stream_create(meta["digitisation"], meta["offset"], meta["range"], int(rna))
        if not self._h:
            raise SfaError("sfa_event_stream_create failed")

    def _call(self, fn, *args):
        cap = 64
        while True:
            out = np.zeros(cap, EVENT_DTYPE)
            n = int(fn(self._h, *args, C.cast(out.ctypes.data, C.POINTER(_lib.SfaEvent)), cap))
            if n < 0:
                raise SfaError(f"the event stream refused the call ({n}): it has finished")
            if n <= cap:
                return out[:n]
            cap = n  # nothing was consumed

    def push(self, raw):
        raw = np.ascontiguousarray(raw, np.int16).reshape(-1)
        keep = raw if raw.size else np.zeros(1, np.int16)
        return self._call(self._L.sfa_event_stream_push, keep.ctypes.data_as(C.POINTER(C.c_int16)), len(raw))

    def finish(self):
        return self._call(self._L.sfa_event_stream_finish)

    def close(self):
        if self._h:
            self._L.sfa_event_stream_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def plan_batch(q_off, job_len, ckpt_interval=0, ckpt_budget_bytes=0, lane_widening=0):
    """Host-side batch layout (no GPU needed): (info dict, slot_of_read int32[n])."""
    qo = np.ascontiguousarray(q_off, np.int64)
    jl = np.ascontiguousarray(job_len, np.int32)
    n = len(qo) - 1
    slot = np.zeros(max(n, 1), np.int32)
    info = _lib.SfaPlanInfo()
    _check(_lib.load().sfa_plan_batch(qo.ctypes.data_as(_lib.i64p), n, jl.ctypes.data_as(_lib.i32p), len(jl),
                                      int(ckpt_interval), int(ckpt_budget_bytes), int(lane_widening),
                                      slot.ctypes.data_as(_lib.i32p),
                                      C.byref(info)), "sfa_plan_batch")
    return {k: getattr(info, k) for k, _ in _lib.SfaPlanInfo._fields_}, slot[:n]


EVENT_DTYPE = np.dtype([("start", "<u8"), ("length", "<f4"), ("mean", "<f4"), ("stdv", "<f4")], align=True)


def paf_row(res, read_id, rname, start_raw, end_raw, query_size, len_raw, rlength, tp="P"):
    """paf_str (src/sigfish.c:628-660) for one result row; tp="S" for a row of Aligner.secondary_rows()."""
    r = _lib.SfaResult(int(res["rid"]), int(res["pos_st"]), int(res["pos_end"]), float(res["score"]),
                       float(res["score2"]), int(res["strand"]), int(res["mapq"]), int(res["valid"]), 0)
    buf = C.create_string_buffer(4096)
    n = _lib.load().sfa_paf_row_ex(buf, 4096, C.byref(r), str(read_id).encode(), str(rname).encode(), int(start_raw),
                                   int(end_raw), int(query_size), int(len_raw), int(rlength), str(tp).encode()[:1])
    if n < 0:
        raise SfaError("sfa_paf_row: buffer too small")
    return buf.raw[:n].decode()


# ---- host pre-DP stages and readers ------------------------------------------------------------
class Blow5File:
    """Sequential BLOW5 reader: iterates (read_id, meta dict, raw int16 array)."""

    def __init__(self, path):
        self._L = _lib.load()
        self._h = self._L.sfa_blow5_open(str(path).encode())
        if not self._h:
            raise SfaError(self._L.sfa_last_error().decode())

    def attr(self, key):
        v = self._L.sfa_blow5_attr(self._h, key.encode())
        return None if v is None else v.decode()

    def select_shard(self, r, G):
        """Only the records starting in the r-th of G equal byte slices of the file (one rank of a read-sharded run)."""
        if self._L.sfa_blow5_select_shard(self._h, r, G) != 0:
            raise SfaError(self._L.sfa_last_error().decode())
        return self

    def select_records(self, first, count=-1):
        """Only records [first, first + count) by position in the file (count < 0: to the end)."""
        if self._L.sfa_blow5_select_records(self._h, first, count) != 0:
            raise SfaError(self._L.sfa_last_error().decode())
        return self

    def __iter__(self):
        rid = C.c_char_p()
        meta = (C.c_double * 4)()
        raw = C.POINTER(C.c_int16)()
        n = C.c_int64()
        while True:
            rc = self._L.sfa_blow5_next(self._h, C.byref(rid), meta, C.byref(raw), C.byref(n))
            if rc == 0:
                return
            if rc < 0:
                raise SfaError(self._L.sfa_last_error().decode())
            sig = np.ctypeslib.as_array(raw, (n.value,)).copy() if n.value else np.zeros(0, np.int16)
            yield rid.value.decode(), dict(digitisation=meta[0], offset=meta[1], range=meta[2], sampling_rate=meta[3]), sig

    def close(self):
        if self._h:
            self._L.sfa_blow5_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def zstd_decompress(data, cap=None):
    """The zstd record decompressor of the BLOW5 reader on its own (the library's decoder, no libzstd): bytes -> bytes, or None
    where the frames are malformed or hold more than `cap` bytes (default: 4x the input + 4 KB, the reader's rule)."""
    L = _lib.load()
    data = bytes(data)
    if cap is None:
        cap = 4 * len(data) + 4096
    out = np.zeros(max(int(cap), 1), np.uint8)
    got = L.sfa_zstd_decompress(data, len(data), out.ctypes.data_as(C.c_void_p), int(cap))
    return None if got < 0 else out[:got].tobytes()


def detect_events(raw, meta, rna=False):
    """event_single: raw int16 samples + scaling -> EVENT_DTYPE array."""
    raw = np.ascontiguousarray(raw, np.int16)
    L = _lib.load()
    cap = max(len(raw) // 2, 16)
    out = np.zeros(cap, EVENT_DTYPE)
    n = L.sfa_detect_events(raw.ctypes.data_as(C.POINTER(C.c_int16)), len(raw), meta["digitisation"], meta["offset"],
                            meta["range"], int(rna), C.cast(out.ctypes.data, C.POINTER(_lib.SfaEvent)), cap)
    if n < 0:
        raise SfaError("sfa_detect_events failed")
    if n > cap:
        out = np.zeros(n, EVENT_DTYPE)
        n = L.sfa_detect_events(raw.ctypes.data_as(C.POINTER(C.c_int16)), len(raw), meta["digitisation"], meta["offset"],
                                meta["range"], int(rna), C.cast(out.ctypes.data, C.POINTER(_lib.SfaEvent)), n)
    return out[:n]


def select_query(events, raw, meta, prefix_size=50, query_size=250, flag=0, pore=0):
    """normalise_single: returns (keep, qstart, qend); `events` is normalised in place over [qstart,qend)."""
    raw = np.ascontiguousarray(raw, np.int16)
    qs, qe = C.c_int64(), C.c_int64()
    keep = _lib.load().sfa_select_query(C.cast(events.ctypes.data, C.POINTER(_lib.SfaEvent)), len(events),
                                        raw.ctypes.data_as(C.POINTER(C.c_int16)), len(raw), meta["digitisation"],
                                        meta["offset"], meta["range"], prefix_size, query_size, flag, pore,
                                        C.byref(qs), C.byref(qe))
    return bool(keep), qs.value, qe.value


def detect_query_start(raw, meta, events, pore=0):
    """detect_query_start: the RNA automatic query start of one read (first event behind the poly-A tail), -1 if not found."""
    raw = np.ascontiguousarray(raw, np.int16)
    ev = np.ascontiguousarray(events, EVENT_DTYPE)
    return int(_lib.load().sfa_detect_query_start(raw.ctypes.data_as(C.POINTER(C.c_int16)), len(raw), meta["digitisation"],
                                                  meta["offset"], meta["range"], C.cast(ev.ctypes.data, C.POINTER(_lib.SfaEvent)),
                                                  len(ev), int(pore)))


def auto_start_target(raw, meta, pore=0):
    """What detect_query_start computes before it looks at events, for the samples `raw` (a read or a prefix of one): the sample
    index behind the poly-A tail that follows the adaptor, or -1 (sfa_auto_start_target)."""
    raw = np.ascontiguousarray(raw, np.int16)
    return int(_lib.load().sfa_auto_start_target(raw.ctypes.data_as(C.POINTER(C.c_int16)), len(raw), meta["digitisation"], meta["offset"],
                                                 meta["range"], int(pore)))


def read_kmer_model(path, warnings=None):
    """read_model: (level_mean[4^k], k).  Rows the reference would only log as corrupted are appended to `warnings` (a list)."""
    lv = np.zeros(262144, np.float32)
    k = C.c_uint32()
    L = _lib.load()
    _check(L.sfa_read_kmer_model(str(path).encode(), lv.ctypes.data_as(_lib.f32p), C.byref(k)), "sfa_read_kmer_model")
    if warnings is not None:
        warnings.extend(w for w in L.sfa_last_error().decode().split("\n") if w)
    return lv[:4 ** k.value].copy(), k.value


def r2qevent_map(res, events, qstart, qend, ref_array, ref_st_offset, flag):
    """aln_t.r2qevent_map (path_to_map, src/sigfish.c:530-571) for one result row: int32 [r2qevent_size, 2] = start, stop."""
    r = _lib.SfaResult(int(res["rid"]), int(res["pos_st"]), int(res["pos_end"]), float(res["score"]),
                       float(res["score2"]), int(res["strand"]), int(res["mapq"]), int(res["valid"]), 0)
    y = _f32(ref_array)
    L = _lib.load()
    evp = C.cast(events.ctypes.data, C.POINTER(_lib.SfaEvent))
    need = L.sfa_r2qevent_map(C.byref(r), evp, int(qstart), int(qend), y.ctypes.data_as(_lib.f32p), len(y), int(ref_st_offset),
                              int(flag), None, 0)
    if need < 0:
        raise SfaError(f"sfa_r2qevent_map failed ({need})")
    out = np.zeros((need, 2), np.int32)
    n = L.sfa_r2qevent_map(C.byref(r), evp, int(qstart), int(qend), y.ctypes.data_as(_lib.f32p), len(y), int(ref_st_offset),
                           int(flag), out.ctypes.data_as(_lib.i32p), need)
    if n != need:
        raise SfaError(f"sfa_r2qevent_map failed ({n})")
    return out


def sam_row(res, read_id, rname, events, qstart, qend, ref_array, ref_st_offset, flag, secondary=False):
    """sam_str (src/sigfish.c:770-794) for one result row; `events` normalised as for align_events; secondary: FLAG | 256."""
    r = _lib.SfaResult(int(res["rid"]), int(res["pos_st"]), int(res["pos_end"]), float(res["score"]),
                       float(res["score2"]), int(res["strand"]), int(res["mapq"]), int(res["valid"]), 0)
    y = _f32(ref_array)
    buf = C.create_string_buffer(1 << 22)
    n = _lib.load().sfa_sam_row_ex(buf, len(buf), C.byref(r), str(read_id).encode(), str(rname).encode(),
                                   C.cast(events.ctypes.data, C.POINTER(_lib.SfaEvent)), int(qstart), int(qend),
                                   y.ctypes.data_as(_lib.f32p), len(y), int(ref_st_offset), int(flag), int(bool(secondary)))
    if n < 0:
        raise SfaError(f"sfa_sam_row failed ({n})")
    return buf.raw[:n].decode()


def sam_row_from_map(res, read_id, rname, events, qstart, qend, pairs, flag, secondary=False):
    """sam_row from the row's reference-column -> query-event map (r2qevent_map or Aligner.event_maps) instead of its path."""
    r = _lib.SfaResult(int(res["rid"]), int(res["pos_st"]), int(res["pos_end"]), float(res["score"]),
                       float(res["score2"]), int(res["strand"]), int(res["mapq"]), int(res["valid"]), 0)
    p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    buf = C.create_string_buffer(1 << 22)
    n = _lib.load().sfa_sam_row_from_map(buf, len(buf), C.byref(r), str(read_id).encode(), str(rname).encode(),
                                         C.cast(events.ctypes.data, C.POINTER(_lib.SfaEvent)), int(qstart), int(qend),
                                         p.ctypes.data_as(_lib.i32p), len(p), int(flag), int(bool(secondary)))
    if n < 0:
        raise SfaError(f"sfa_sam_row_from_map failed ({n})")
    return buf.raw[:n].decode()
