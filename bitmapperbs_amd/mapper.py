"""Host-side mirror of the reference's `--search` mapping drivers over the C-ABI.

`Index`   == Load_Index / load_index (Index.cpp:940, bwt.cpp:2458): the on-disk index files.
`Mapper`  == Prepare_alignment + Map_Single_Seq (Schema.cpp:639, 26330) for one GPU: batches of
             equal-length reads in, 32-byte result records + CIGAR pool out; SAM text is formatted on
             the host from the records (output_sam_end_to_end, Schema.cpp:11989-12039).
All mapping work happens in libbmbs_hip.so on the GPU; this module only moves buffers and prints.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


class Index:
    def __init__(self, prefix: str):
        self._lib = capi.lib()
        self._h = self._lib.bmbs_index_file_load(prefix.encode())
        if not self._h:
            raise FileNotFoundError(f"cannot load BitMapperBS index files at {prefix}.index*")
        self.view = capi.IndexView()
        self._lib.bmbs_index_file_view(self._h, C.byref(self.view))
        self.chrom_names = [self._lib.bmbs_index_file_chrom_name(self._h, i).decode()
                            for i in range(self.view.n_chrom)]
        self.chrom_len = np.ctypeslib.as_array(
            C.cast(self.view.chrom_len, C.POINTER(C.c_uint64)), shape=(self.view.n_chrom,)).copy()
        self.ref_len = int(self.view.ref_len)

    @staticmethod
    def build(fasta: str, prefix: str | None = None, threads: int = 8, device: int | None = None) -> None:
        """createIndex equivalent; device=None: host cores (bmbs_index_build), device=d: the GPU builder (same files)"""
        if device is None:
            rc = capi.lib().bmbs_index_build(fasta.encode(), (prefix or fasta).encode(), threads)
        else:
            rc = capi.lib().bmbs_index_build_device(device, fasta.encode(), (prefix or fasta).encode(), threads)
        if rc:
            raise RuntimeError(f"bmbs_index_build{'' if device is None else '_device'} failed ({rc})")

    def close(self):
        if self._h:
            self._lib.bmbs_index_file_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BamSortNoRoom(RuntimeError):
    """Mapper.bam_sort: the output buffer was too small (BMBS_ENOMEM); `needed` = the bytes the library asks for"""
    needed = 0


class Mapper:
    def __init__(self, index: Index, device: int = 0, share: "Mapper | None" = None, **params):
        """index None: a context with no index attached (enough for bam_sort and inflate_bgzf).
        share: another Mapper on the same device whose attached index this one uses (bmbs_index_share) -- for two batches
        in flight from two host threads; `share` has to stay open for as long as this one is used"""
        self._lib = capi.lib()
        self.params = capi.default_params(**params)
        self._ctx = self._lib.bmbs_create(device, C.byref(self.params))
        if not self._ctx:
            raise RuntimeError("bmbs_create failed: no usable HIP device (the mapper has no CPU path)")
        self.index = index
        self._owner = share
        if index is None and share is None:
            pass                                   # a context without an index: what bam_sort() needs
        elif share is None:
            self._chk(self._lib.bmbs_index_attach(self._ctx, C.byref(index.view)))
        else:
            self._chk(self._lib.bmbs_index_share(self._ctx, share._ctx))

    def _chk(self, rc: int):
        if rc:
            raise RuntimeError(f"bmbs error {rc}: {self._lib.bmbs_last_error(self._ctx).decode()}")

    def close(self):
        if self._ctx:
            self._lib.bmbs_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def threshold(self, L: int) -> int:
        k = int(np.uint64(self.params.e_f * L))   # Schema.cpp:24546
        return min(k, 31)

    def max_cigar_ops(self, L: int) -> int:
        """slots per read the cigar pool needs (bmbs_max_cigar_ops): 2k + 8 with the default penalties"""
        return int(self._lib.bmbs_max_cigar_ops(C.byref(self.params), int(L)))

    # ---- fused single-end mapping ------------------------------------------------------------------
    def map_se(self, seq: np.ndarray, qual: np.ndarray, L: int | None = None):
        """seq/qual: uint8 [n, stride] (ASCII, upper case).  -> (results[n] RESULT_DTYPE, cigar_pool u32)"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        n, stride = seq.shape
        L = stride if L is None else L
        res = np.zeros(n, dtype=capi.RESULT_DTYPE)
        cap = max(1, n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        self._chk(self._lib.bmbs_map_se(self._ctx, capi.ptr(seq), capi.ptr(qual), L, stride, n, capi.ptr(res),
                                        capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    def map_se_device(self, d_seq: int, d_qual: int, L: int, stride: int, n: int, d_results: int,
                      d_cigar_pool: int, cigar_cap: int):
        self._chk(self._lib.bmbs_map_se_device(self._ctx, d_seq, d_qual, L, stride, n, d_results, d_cigar_pool, cigar_cap))

    # ---- fused paired-end mapping (fast mode) ------------------------------------------------------
    def map_pe(self, seq1, qual1, seq2, qual2, L: int | None = None):
        """seq2/qual2 = mate 2 as in the FASTQ file.  -> (results[2n] (mate1, mate2 interleaved), cigar_pool)"""
        a = [np.ascontiguousarray(x, dtype=np.uint8) for x in (seq1, qual1, seq2, qual2)]
        n, stride = a[0].shape
        L = stride if L is None else L
        res = np.zeros(2 * n, dtype=capi.RESULT_DTYPE)
        cap = max(1, 2 * n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        self._chk(self._lib.bmbs_map_pe(self._ctx, capi.ptr(a[0]), capi.ptr(a[1]), capi.ptr(a[2]), capi.ptr(a[3]), L, stride, n,
                                        capi.ptr(res), capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    def map_pe_device(self, d_seq1, d_qual1, d_seq2, d_qual2, L, stride, n, d_results, d_cigar_pool, cigar_cap):
        self._chk(self._lib.bmbs_map_pe_device(self._ctx, d_seq1, d_qual1, d_seq2, d_qual2, L, stride, n, d_results,
                                               d_cigar_pool, cigar_cap))

    # ---- reads of different lengths in one batch (trimmed libraries) -------------------------------
    def map_se_var(self, seq: np.ndarray, qual: np.ndarray, lens: np.ndarray):
        """seq/qual: uint8 [n, stride]; lens[i] <= stride valid characters in row i"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint16)
        n, stride = seq.shape
        L = int(lens.max()) if n else 1
        res = np.zeros(n, dtype=capi.RESULT_DTYPE)
        cap = max(1, n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        self._chk(self._lib.bmbs_map_se_var(self._ctx, capi.ptr(seq), capi.ptr(qual), capi.ptr(lens), L, stride, n, capi.ptr(res),
                                            capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    def map_pe_var(self, seq1, qual1, seq2, qual2, lens1, lens2):
        a = [np.ascontiguousarray(x, dtype=np.uint8) for x in (seq1, qual1, seq2, qual2)]
        l1 = np.ascontiguousarray(lens1, dtype=np.uint16); l2 = np.ascontiguousarray(lens2, dtype=np.uint16)
        n, stride = a[0].shape
        L = int(max(l1.max(), l2.max())) if n else 1
        res = np.zeros(2 * n, dtype=capi.RESULT_DTYPE)
        cap = max(1, 2 * n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        self._chk(self._lib.bmbs_map_pe_var(self._ctx, capi.ptr(a[0]), capi.ptr(a[1]), capi.ptr(a[2]), capi.ptr(a[3]), capi.ptr(l1),
                                            capi.ptr(l2), L, stride, n, capi.ptr(res), capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    # ---- packed reads: 2 bits per base + an 'N' plane (bmbs_map_*_packed) -----------------------------
    @staticmethod
    def pack_rows(seq: np.ndarray, L: int, lens: np.ndarray | None = None, pwords: int | None = None, threads: int = 8) -> np.ndarray:
        """ASCII rows [n][stride] -> packed rows [n][pwords] of u64 (bmbs_pack_rows); raises when a row holds something other than ACGTN"""
        a = np.ascontiguousarray(seq, dtype=np.uint8)
        n, stride = a.shape
        if pwords is None:
            pwords = (L + 31) // 32 + (L + 63) // 64
        rows = np.empty((n, pwords), dtype=np.uint64)
        bad = C.c_int64(-1)
        ln = np.ascontiguousarray(lens, dtype=np.uint16) if lens is not None else None
        rc = capi.lib().bmbs_pack_rows(capi.ptr(a), L, stride, n, capi.ptr(ln) if ln is not None else None, capi.ptr(rows), pwords, threads, C.byref(bad))
        if rc:
            raise ValueError("bmbs_pack_rows: row %d cannot be packed (rc %d)" % (bad.value, rc))
        return rows

    def map_se_packed(self, rows: np.ndarray, qual: np.ndarray, L: int, lens: np.ndarray | None = None):
        q = np.ascontiguousarray(qual, dtype=np.uint8)
        n, stride = q.shape
        res = np.zeros(n, dtype=capi.RESULT_DTYPE)
        cap = max(1, n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        ln = np.ascontiguousarray(lens, dtype=np.uint16) if lens is not None else None
        self._chk(self._lib.bmbs_map_se_packed(self._ctx, capi.ptr(rows), rows.shape[1], capi.ptr(q), capi.ptr(ln) if ln is not None else None, L, stride, n,
                                               capi.ptr(res), capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    def map_pe_packed(self, rows1: np.ndarray, rows2: np.ndarray, qual1: np.ndarray, qual2: np.ndarray, L: int, lens1=None, lens2=None):
        q1 = np.ascontiguousarray(qual1, dtype=np.uint8); q2 = np.ascontiguousarray(qual2, dtype=np.uint8)
        n, stride = q1.shape
        res = np.zeros(2 * n, dtype=capi.RESULT_DTYPE)
        cap = max(1, 2 * n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        l1 = np.ascontiguousarray(lens1, dtype=np.uint16) if lens1 is not None else None
        l2 = np.ascontiguousarray(lens2, dtype=np.uint16) if lens2 is not None else None
        self._chk(self._lib.bmbs_map_pe_packed(self._ctx, capi.ptr(rows1), capi.ptr(rows2), rows1.shape[1], capi.ptr(q1), capi.ptr(q2),
                                               capi.ptr(l1) if l1 is not None else None, capi.ptr(l2) if l2 is not None else None, L, stride, n,
                                               capi.ptr(res), capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    # ---- packed quality classes: 4 bits per quality (bmbs_map_*_packedq) -------------------------------
    def qual_classes(self):
        """(class_of u8[256], penalty_of i32[n_classes]) under this mapper's mp_max / mp_min / q_base (bmbs_qual_classes): class 0 is the
        largest penalty, class_of 0xFF marks a byte that cannot be packed"""
        return qual_classes(self.params)

    def pack_quals(self, qual: np.ndarray, L: int, lens: np.ndarray | None = None, qwords: int | None = None, threads: int = 8) -> np.ndarray:
        """quality rows [n][stride] -> packed class rows [n][qwords] of u64 (bmbs_pack_quals) under this mapper's parameters; raises when a
        row holds a byte without a class"""
        return pack_quals(self.params, qual, L, lens, qwords, threads)

    def map_se_packedq(self, rows: np.ndarray, qrows: np.ndarray, L: int, lens: np.ndarray | None = None):
        n = rows.shape[0]
        res = np.zeros(n, dtype=capi.RESULT_DTYPE)
        cap = max(1, n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        ln = np.ascontiguousarray(lens, dtype=np.uint16) if lens is not None else None
        self._chk(self._lib.bmbs_map_se_packedq(self._ctx, capi.ptr(rows), rows.shape[1], capi.ptr(qrows), qrows.shape[1],
                                                capi.ptr(ln) if ln is not None else None, L, n, capi.ptr(res), capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    def map_pe_packedq(self, rows1: np.ndarray, rows2: np.ndarray, qrows1: np.ndarray, qrows2: np.ndarray, L: int, lens1=None, lens2=None):
        n = rows1.shape[0]
        assert qrows1.shape == qrows2.shape and rows1.shape == rows2.shape
        res = np.zeros(2 * n, dtype=capi.RESULT_DTYPE)
        cap = max(1, 2 * n * self.max_cigar_ops(L))
        pool = np.zeros(cap, dtype=np.uint32)
        used = C.c_int64(0)
        l1 = np.ascontiguousarray(lens1, dtype=np.uint16) if lens1 is not None else None
        l2 = np.ascontiguousarray(lens2, dtype=np.uint16) if lens2 is not None else None
        self._chk(self._lib.bmbs_map_pe_packedq(self._ctx, capi.ptr(rows1), capi.ptr(rows2), rows1.shape[1], capi.ptr(qrows1), capi.ptr(qrows2),
                                                qrows1.shape[1], capi.ptr(l1) if l1 is not None else None, capi.ptr(l2) if l2 is not None else None,
                                                L, n, capi.ptr(res), capi.ptr(pool), cap, C.byref(used)))
        return res, pool[:used.value]

    # ---- FASTQ text in, SAM text out (newline index and SAM formatting on the device) ---------------
    TEXT_PBAT, TEXT_UNMAPPED, TEXT_BAM = 1, 2, 16
    TEXT_BAM_SORTED = 32      # with TEXT_BAM: the batch's uncompressed BAM records, stably sorted by bam_key order (include/bmbs.h)
    BAMSORT_RAW = 1

    def _set_refs(self):
        if getattr(self, "_refs_set", False):
            return
        names = (C.c_char_p * len(self.index.chrom_names))(*[n.encode() for n in self.index.chrom_names])
        self._chk(self._lib.bmbs_sam_refs(self._ctx, names, len(self.index.chrom_names)))
        self._refs_set = True

    def map_text(self, text1: bytes, n: int, text2: bytes | None = None, flags: int = 0, cap: int | None = None) -> bytes:
        """FASTQ text of n records (pairs with text2) -> the SAM lines the reference prints for them, in input order (flags & TEXT_BAM:
        their BAM records as complete BGZF blocks).  cap: bytes of the output buffer handed to the library (default: ample)"""
        self._set_refs()
        if cap is None:
            cap = len(text1) + (len(text2) if text2 else 0) + (2 if text2 else 1) * n * 640 + 4096
        out = np.empty(cap, dtype=np.uint8)
        used = C.c_uint64(0); lines = C.c_int64(0)
        a1 = np.frombuffer(text1, dtype=np.uint8)
        if text2 is None:
            self._chk(self._lib.bmbs_map_se_text(self._ctx, capi.ptr(a1), a1.size, n, flags, capi.ptr(out), cap, C.byref(used), C.byref(lines)))
        else:
            a2 = np.frombuffer(text2, dtype=np.uint8)
            self._chk(self._lib.bmbs_map_pe_text(self._ctx, capi.ptr(a1), a1.size, capi.ptr(a2), a2.size, n, flags, capi.ptr(out), cap,
                                                 C.byref(used), C.byref(lines)))
        return out[:used.value].tobytes()

    def inflate_bgzf(self, data: bytes, shift: int | None = None):
        """the text of a BGZF byte string (bgzip's format), inflated on the device (bmbs_inflate_bgzf); raises on a malformed block"""
        import struct
        blk = [0]; out = [0]
        at = 0
        while at < len(data):
            bs = struct.unpack("<H", data[at + 16:at + 18])[0] + 1
            isz = struct.unpack("<I", data[at + bs - 4:at + bs])[0]
            at += bs; blk.append(at); out.append(out[-1] + isz)
        n = len(blk) - 1
        a = np.frombuffer(data, dtype=np.uint8)
        b = np.array(blk, dtype=np.uint64); o = np.array(out, dtype=np.uint64)
        text = np.empty(max(1, out[-1]), dtype=np.uint8)
        if shift is None:
            self._chk(self._lib.bmbs_inflate_bgzf(self._ctx, capi.ptr(a), a.size, capi.ptr(b), capi.ptr(o), n, capi.ptr(text), out[-1], None, 0))
            return text[:out[-1]].tobytes()
        cnt = np.zeros(max(1, (shift + out[-1] + 65535) >> 16), dtype=np.uint32)
        self._chk(self._lib.bmbs_inflate_bgzf(self._ctx, capi.ptr(a), a.size, capi.ptr(b), capi.ptr(o), n, capi.ptr(text), out[-1], capi.ptr(cnt), shift))
        return text[:out[-1]].tobytes(), cnt

    @staticmethod
    def _ztext(prefix: bytes, blocks: bytes, keep):
        """a capi.ZText over `prefix` + the BGZF blocks in `blocks` (objects that must stay alive are appended to `keep`)"""
        import struct
        blk = [0]; out = [0]
        at = 0
        while at < len(blocks):
            bs = struct.unpack("<H", blocks[at + 16:at + 18])[0] + 1
            isz = struct.unpack("<I", blocks[at + bs - 4:at + bs])[0]
            at += bs; blk.append(at); out.append(out[-1] + isz)
        a = np.frombuffer(blocks, dtype=np.uint8) if blocks else np.zeros(1, dtype=np.uint8)
        pf = np.frombuffer(prefix, dtype=np.uint8) if prefix else np.zeros(1, dtype=np.uint8)
        b = np.array(blk, dtype=np.uint64); o = np.array(out, dtype=np.uint64)
        keep += [a, pf, b, o]
        z = capi.ZText()
        z.prefix = capi.ptr(pf) if prefix else None; z.prefix_bytes = len(prefix)
        z.comp = capi.ptr(a); z.comp_bytes = len(blocks); z.blk_off = capi.ptr(b); z.out_off = capi.ptr(o); z.n_blocks = len(blk) - 1
        return z

    def text_open_bgzf(self, w1, w2=None, max_records=1 << 30, last=(False, False), tail_cap=1 << 24):
        """w = (prefix bytes, BGZF blocks): the window(s) are assembled and indexed on the device -> (records, tail1, tail2)"""
        self._set_refs()
        keep = []
        z1 = self._ztext(w1[0], w1[1], keep)
        z2 = self._ztext(w2[0], w2[1], keep) if w2 is not None else None
        t1 = np.empty(tail_cap, dtype=np.uint8); t2 = np.empty(tail_cap, dtype=np.uint8)
        n = C.c_int64(0); b1 = C.c_uint64(0); b2 = C.c_uint64(0)
        self._chk(self._lib.bmbs_text_open_bgzf(self._ctx, C.byref(z1), C.byref(z2) if z2 is not None else None, max_records, int(last[0]), int(last[1]),
                                                C.byref(n), capi.ptr(t1), tail_cap, C.byref(b1), capi.ptr(t2), C.byref(b2)))
        return int(n.value), t1[:b1.value].tobytes(), t2[:b2.value].tobytes()

    def text_map_open(self, flags: int = 0, cap: int = 1 << 28) -> bytes:
        out = np.empty(cap, dtype=np.uint8)
        used = C.c_uint64(0); lines = C.c_int64(0)
        self._chk(self._lib.bmbs_text_map_open(self._ctx, flags, capi.ptr(out), cap, C.byref(used), C.byref(lines)))
        return out[:used.value].tobytes()

    # trim_galore's defaults (bmbs_search --trim)
    TRIM_DEFAULTS = dict(quality=20, adapter="AGATCGGAAGAGC", adapter2=None, min_overlap=1, error_permille=100, min_length=20,
                         clip_5p=(0, 0), clip_3p=(0, 0))

    def set_trim(self, **opts):
        """adapter and quality trimming in map_text / text_map_open (bmbs_set_trim; the rule: include/bmbs.h, tests/trim_spec.py).
        set_trim(off=True) turns it off; otherwise the keywords of TRIM_DEFAULTS replace trim_galore's defaults: quality (0: no
        quality step), adapter / adapter2 (mate 1 / mate 2; adapter2 None: mate 1's; "": no adapter step), min_overlap,
        error_permille, min_length, clip_5p / clip_3p (a pair, or one number for both mates)"""
        if opts.pop("off", False):
            assert not opts
            self._chk(self._lib.bmbs_set_trim(self._ctx, None))
            return
        o = dict(self.TRIM_DEFAULTS)
        for k, v in opts.items():
            if k not in o:
                raise TypeError("set_trim: unknown option %r" % k)
            o[k] = v
        t = capi.TrimOpts()
        t.quality, t.min_overlap, t.error_permille, t.min_length = int(o["quality"]), int(o["min_overlap"]), int(o["error_permille"]), int(o["min_length"])
        for name in ("clip_5p", "clip_3p"):
            v = o[name] if isinstance(o[name], (tuple, list)) else (o[name], o[name])
            getattr(t, name)[0], getattr(t, name)[1] = int(v[0]), int(v[1])
        ads = (o["adapter"] or "", o["adapter"] or "" if o["adapter2"] is None else o["adapter2"])
        for m, a in enumerate(ads):
            if len(a) > 32:
                raise ValueError("set_trim: an adapter has at most 32 letters (bmbs_trim_opts holds no more)")
            t.adapter[m].value = a.encode()
        self._chk(self._lib.bmbs_set_trim(self._ctx, C.byref(t)))

    def trim_counts(self):
        """(counters, kept) of the last map_text / text_map_open call with trimming on (bmbs_text_trim_counts): counters = a dict of
        capi.TRIM_COUNTERS -> (mate 1, mate 2) and "templates_dropped"; kept = the templates that were mapped"""
        cnt = capi.TrimCounts(); kept = C.c_int64(0)
        self._chk(self._lib.bmbs_text_trim_counts(self._ctx, C.byref(cnt), C.byref(kept)))
        d = {k: (int(getattr(cnt, k)[0]), int(getattr(cnt, k)[1])) for k in capi.TRIM_COUNTERS}
        d["templates_dropped"] = int(cnt.templates_dropped)
        return d, int(kept.value)

    def trim_text(self, text: bytes, n: int, mate: int = 0):
        """the trim stage alone (bmbs_trim_text): (seq_off u32[n], qual_off u32[n], seq_len u16[n], qual_len u16[n]) of the n records of
        `text`, read as mate `mate`, after the quality, adapter and clip steps and before the length filter"""
        a = np.frombuffer(text, dtype=np.uint8)
        so = np.zeros(max(1, n), dtype=np.uint32); qo = np.zeros(max(1, n), dtype=np.uint32)
        sl = np.zeros(max(1, n), dtype=np.uint16); ql = np.zeros(max(1, n), dtype=np.uint16)
        self._chk(self._lib.bmbs_trim_text(self._ctx, capi.ptr(a), a.size, n, int(mate), capi.ptr(so), capi.ptr(qo), capi.ptr(sl), capi.ptr(ql)))
        return so[:n], qo[:n], sl[:n], ql[:n]

    def sorted_index(self):
        """(keys u64[n], lengths u32[n]) of the records the last map_text / text_map_open call with TEXT_BAM | TEXT_BAM_SORTED returned, in
        the order returned (bmbs_text_sorted_index)"""
        n = C.c_int64(0)
        rc = self._lib.bmbs_text_sorted_index(self._ctx, None, None, 0, C.byref(n))
        if rc and rc != -12:
            self._chk(rc)
        key = np.empty(max(1, n.value), dtype=np.uint64); ln = np.empty(max(1, n.value), dtype=np.uint32)
        self._chk(self._lib.bmbs_text_sorted_index(self._ctx, capi.ptr(key), capi.ptr(ln), n.value, C.byref(n)))
        return key[:n.value], ln[:n.value]

    def bam_sort(self, records: bytes, lens, raw: bool = False, cap: int | None = None) -> bytes:
        """concatenated BAM records + their sizes -> the records stably sorted by coordinate key (bmbs_bam_sort): BGZF blocks, or the
        uncompressed records with raw=True.  cap: bytes of the output buffer handed to the library (default: ample); a buffer that is
        too small raises BamSortNoRoom, whose `needed` is the size the library asks for"""
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        a = np.frombuffer(records, dtype=np.uint8) if len(records) else np.zeros(1, dtype=np.uint8)
        if cap is None:
            cap = len(records) + (len(records) // 0xff00 + 2) * 64 + 4096
        out = np.empty(max(1, cap), dtype=np.uint8)
        used = C.c_uint64(0)
        rc = self._lib.bmbs_bam_sort(self._ctx, capi.ptr(a), len(records), capi.ptr(ln) if ln.size else None, ln.size, self.BAMSORT_RAW if raw else 0,
                                     capi.ptr(out), cap, C.byref(used))
        if rc == -12:
            e = BamSortNoRoom(f"bmbs error {rc}: {self._lib.bmbs_last_error(self._ctx).decode()}")
            e.needed = int(used.value)
            raise e
        self._chk(rc)
        return out[:used.value].tobytes()

    def bam_sort_index(self):
        """the .bai pieces of the last bam_sort() call that returned BGZF blocks (bmbs_bam_sort_index), computed on the device:
        (chunks BAI_CHUNK_DTYPE ordered by (ref, bin, beg), windows BAI_WIN_DTYPE ordered by (ref, win), references BAI_REF_DTYPE,
        n_no_coor); virtual offsets are relative to the first byte that call returned"""
        nc = C.c_int64(0); nw = C.c_int64(0); nr = C.c_int64(0); nn = C.c_uint64(0)
        rc = self._lib.bmbs_bam_sort_index(self._ctx, None, 0, C.byref(nc), None, 0, C.byref(nw), None, 0, C.byref(nr), C.byref(nn))
        if rc and rc != -12:
            self._chk(rc)
        ch = np.zeros(max(1, nc.value), dtype=capi.BAI_CHUNK_DTYPE); wi = np.zeros(max(1, nw.value), dtype=capi.BAI_WIN_DTYPE)
        rf = np.zeros(max(1, nr.value), dtype=capi.BAI_REF_DTYPE)
        self._chk(self._lib.bmbs_bam_sort_index(self._ctx, capi.ptr(ch), nc.value, C.byref(nc), capi.ptr(wi), nw.value, C.byref(nw), capi.ptr(rf), nr.value,
                                                C.byref(nr), C.byref(nn)))
        return ch[:nc.value], wi[:nw.value], rf[:nr.value], int(nn.value)

    def dup_sigs(self, records: bytes, lens, paired: bool = False) -> np.ndarray:
        """concatenated BAM records in input order + their sizes (0: no record here) -> the duplicate signature of every template
        (capi.DUP_SIG_DTYPE; bmbs_bam_dup_sigs): one record each, or with paired=True the entries 2p and 2p + 1"""
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        a = np.frombuffer(records, dtype=np.uint8) if len(records) else np.zeros(1, dtype=np.uint8)
        n = C.c_int64(0)
        rc = self._lib.bmbs_bam_dup_sigs(self._ctx, capi.ptr(a), len(records), capi.ptr(ln) if ln.size else None, ln.size, int(paired), None, 0, C.byref(n))
        if rc and rc != -12:
            self._chk(rc)
        sig = np.zeros(max(1, n.value), dtype=capi.DUP_SIG_DTYPE)
        self._chk(self._lib.bmbs_bam_dup_sigs(self._ctx, capi.ptr(a), len(records), capi.ptr(ln) if ln.size else None, ln.size, int(paired), capi.ptr(sig), n.value,
                                              C.byref(n)))
        return sig[:n.value]

    def sorted_dup(self):
        """(signatures DUP_SIG_DTYPE[templates of the batch], tmpl u32[records]) of the last map_text / text_map_open call with TEXT_BAM |
        TEXT_BAM_SORTED: tmpl[j] = the template of the j-th record that call returned (bmbs_text_sorted_dup)"""
        ns = C.c_int64(0); n = C.c_int64(0)
        rc = self._lib.bmbs_text_sorted_dup(self._ctx, None, 0, C.byref(ns), None, 0, C.byref(n))
        if rc and rc != -12:
            self._chk(rc)
        sig = np.zeros(max(1, ns.value), dtype=capi.DUP_SIG_DTYPE); tmpl = np.zeros(max(1, n.value), dtype=np.uint32)
        self._chk(self._lib.bmbs_text_sorted_dup(self._ctx, capi.ptr(sig), ns.value, C.byref(ns), capi.ptr(tmpl), n.value, C.byref(n)))
        return sig[:ns.value], tmpl[:n.value]

    def dup_select(self, sig: np.ndarray):
        """signatures in input order -> (dup u8[n]: 1 where a template loses its group, their number) (bmbs_dup_select)"""
        s = np.ascontiguousarray(sig, dtype=capi.DUP_SIG_DTYPE)
        dup = np.zeros(max(1, s.size), dtype=np.uint8)
        nd = C.c_int64(0)
        self._chk(self._lib.bmbs_dup_select(self._ctx, capi.ptr(s) if s.size else None, s.size, capi.ptr(dup), C.byref(nd)))
        return dup[:s.size], int(nd.value)

    def sorted_clip(self) -> np.ndarray:
        """clip u32[records] of the last map_text / text_map_open call with TEXT_BAM | TEXT_BAM_SORTED: the mate-overlap clip of the j-th
        record that call returned (bmbs_text_sorted_clip)"""
        n = C.c_int64(0)
        rc = self._lib.bmbs_text_sorted_clip(self._ctx, None, 0, C.byref(n))
        if rc and rc != -12:
            self._chk(rc)
        clip = np.zeros(max(1, n.value), dtype=np.uint32)
        self._chk(self._lib.bmbs_text_sorted_clip(self._ctx, capi.ptr(clip), n.value, C.byref(n)))
        return clip[:n.value]

    @staticmethod
    def _nonconv_params(threshold, percent, min_count, min_phred):
        return capi.NonconvParams(int(threshold), int(percent), int(min_count), int(min_phred))

    def bam_nonconv(self, records: bytes, lens, paired: bool = False, threshold: int = 3, percent: int = 0, min_count: int = 5, min_phred: int = 0):
        """concatenated BAM records in input order + their sizes (0: no record here) -> (count NONCONV_COUNT_DTYPE[records]: the non-CpG
        calls of each, fail u8[templates]: 1 where a template failed the non-conversion filter, their number, totals u64
        NONCONV_TOTALS_SHAPE: the calls of all examined records); a template is one record, or with paired=True the entries 2p and
        2p + 1 (bmbs_bam_nonconv)"""
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        a = np.frombuffer(records, dtype=np.uint8) if len(records) else np.zeros(1, dtype=np.uint8)
        par = self._nonconv_params(threshold, percent, min_count, min_phred)
        nt = C.c_int64(0); nf = C.c_int64(0)
        cap = ln.size // 2 if paired else ln.size
        count = np.zeros(max(1, ln.size), dtype=capi.NONCONV_COUNT_DTYPE)
        fail = np.zeros(max(1, cap), dtype=np.uint8)
        totals = np.zeros(capi.NONCONV_TOTALS_SHAPE, dtype=np.uint64)
        self._chk(self._lib.bmbs_bam_nonconv(self._ctx, capi.ptr(a), len(records), capi.ptr(ln) if ln.size else None, ln.size, int(paired), C.byref(par),
                                             capi.ptr(count), capi.ptr(fail), cap, C.byref(nt), C.byref(nf), capi.ptr(totals)))
        return count[:ln.size], fail[:nt.value], int(nf.value), totals

    def sorted_nonconv(self, threshold: int = 3, percent: int = 0, min_count: int = 5, min_phred: int = 0):
        """(fail u8[records], failed templates, totals u64 NONCONV_TOTALS_SHAPE) of the last map_text / text_map_open call with TEXT_BAM |
        TEXT_BAM_SORTED: fail[j] = 1 where the template of the j-th record that call returned failed the non-conversion filter
        (bmbs_text_sorted_nonconv)"""
        par = self._nonconv_params(threshold, percent, min_count, min_phred)
        n = C.c_int64(0); nf = C.c_int64(0)
        rc = self._lib.bmbs_text_sorted_nonconv(self._ctx, C.byref(par), None, 0, C.byref(n), C.byref(nf), None)
        if rc and rc != -12:
            self._chk(rc)
        fail = np.zeros(max(1, n.value), dtype=np.uint8)
        totals = np.zeros(capi.NONCONV_TOTALS_SHAPE, dtype=np.uint64)
        self._chk(self._lib.bmbs_text_sorted_nonconv(self._ctx, C.byref(par), capi.ptr(fail), n.value, C.byref(n), C.byref(nf), capi.ptr(totals)))
        return fail[:n.value], int(nf.value), totals

    @staticmethod
    def _methyl_params(contexts, min_mapq, min_phred):
        return capi.MethylParams(int(contexts), int(min_mapq), int(min_phred), 0)

    def methyl_sites(self) -> np.ndarray:
        """the sites (capi.METHYL_SITE_DTYPE) the last bam_methyl / bam_sort_methyl call left on the device (bmbs_methyl_sites)"""
        n = C.c_int64(0)
        rc = self._lib.bmbs_methyl_sites(self._ctx, None, 0, C.byref(n))
        if rc and rc != -12:
            self._chk(rc)
        site = np.zeros(max(1, n.value), dtype=capi.METHYL_SITE_DTYPE)
        self._chk(self._lib.bmbs_methyl_sites(self._ctx, capi.ptr(site), n.value, C.byref(n)))
        return site[:n.value]

    @staticmethod
    def _methyl_opts(contexts, min_mapq, min_phred, ignore_5p, ignore_3p, mbias):
        """None with the defaults of the three new keywords (the call then goes to the entry point without options), else MethylOpts"""
        i5, i3 = tuple(int(x) for x in ignore_5p), tuple(int(x) for x in ignore_3p)
        if len(i5) != 2 or len(i3) != 2:
            raise ValueError("ignore_5p and ignore_3p: one value per mate")
        if not mbias and i5 == (0, 0) and i3 == (0, 0):
            return None
        return capi.MethylOpts(int(contexts), int(min_mapq), int(min_phred), capi.METHYL_MBIAS if mbias else 0, (C.c_int32 * 2)(*i5), (C.c_int32 * 2)(*i3))

    def methyl_mbias(self) -> np.ndarray:
        """the M-bias table the last bam_methyl / bam_sort_methyl call with mbias=True left: uint64 [mate][strand][context][0 unmethylated,
        1 methylated][cycle] (capi.MBIAS_SHAPE), every call that passed every filter but the trim (bmbs_methyl_mbias)"""
        n = C.c_int64(0)
        rc = self._lib.bmbs_methyl_mbias(self._ctx, None, 0, C.byref(n))
        if rc and rc != -12:
            self._chk(rc)
        table = np.zeros(max(1, n.value), dtype=np.uint64)
        self._chk(self._lib.bmbs_methyl_mbias(self._ctx, capi.ptr(table), n.value, C.byref(n)))
        return table[:n.value].reshape(capi.MBIAS_SHAPE)

    def bam_methyl(self, records: bytes, lens, clip=None, contexts: int = 1, min_mapq: int = 10, min_phred: int = 5, ignore_5p=(0, 0), ignore_3p=(0, 0),
                   mbias: bool = False) -> np.ndarray:
        """concatenated BAM records + their sizes (0: no record here) [+ their mate-overlap clips] -> the methylation counts of every
        cytosine of the selected contexts (1 CpG | 2 CHG | 4 CHH) that a record calls, ordered by (ref, pos) (bmbs_bam_methyl).
        ignore_5p / ignore_3p = (read 1 or single end, read 2): cycles left out at either end of a read; mbias: keep the M-bias table for
        methyl_mbias() (bmbs_bam_methyl_opts)"""
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        a = np.frombuffer(records, dtype=np.uint8) if len(records) else np.zeros(1, dtype=np.uint8)
        cl = None if clip is None else np.ascontiguousarray(clip, dtype=np.uint32)
        if cl is not None and cl.size != ln.size:
            raise ValueError("bam_methyl: one clip per record")
        opts = self._methyl_opts(contexts, min_mapq, min_phred, ignore_5p, ignore_3p, mbias)
        par = self._methyl_params(contexts, min_mapq, min_phred)
        n = C.c_int64(0)
        call = self._lib.bmbs_bam_methyl if opts is None else self._lib.bmbs_bam_methyl_opts
        self._chk(call(self._ctx, capi.ptr(a), len(records), capi.ptr(ln) if ln.size else None, ln.size,
                       capi.ptr(cl) if cl is not None and cl.size else None, C.byref(par if opts is None else opts), C.byref(n)))
        return self.methyl_sites()

    def bam_sort_methyl(self, clip=None, contexts: int = 1, min_mapq: int = 10, min_phred: int = 5, ignore_5p=(0, 0), ignore_3p=(0, 0), mbias: bool = False) -> np.ndarray:
        """the same for the records of the last bam_sort call, which are still on the device; clip in that call's input order
        (bmbs_bam_sort_methyl, bmbs_bam_sort_methyl_opts)"""
        cl = None if clip is None else np.ascontiguousarray(clip, dtype=np.uint32)
        opts = self._methyl_opts(contexts, min_mapq, min_phred, ignore_5p, ignore_3p, mbias)
        par = self._methyl_params(contexts, min_mapq, min_phred)
        n = C.c_int64(0)
        call = self._lib.bmbs_bam_sort_methyl if opts is None else self._lib.bmbs_bam_sort_methyl_opts
        self._chk(call(self._ctx, capi.ptr(cl) if cl is not None and cl.size else None, C.byref(par if opts is None else opts), C.byref(n)))
        return self.methyl_sites()

    def methyl_opposite(self) -> np.ndarray:
        """the entries (capi.METHYL_SITE_DTYPE: meth = variants, unmeth = matches) the last bam_methyl_opposite / bam_sort_methyl_opposite
        call left on the device (bmbs_methyl_opposite)"""
        n = C.c_int64(0)
        rc = self._lib.bmbs_methyl_opposite(self._ctx, None, 0, C.byref(n))
        if rc and rc != -12:
            self._chk(rc)
        entry = np.zeros(max(1, n.value), dtype=capi.METHYL_SITE_DTYPE)
        self._chk(self._lib.bmbs_methyl_opposite(self._ctx, capi.ptr(entry), n.value, C.byref(n)))
        return entry[:n.value]

    @staticmethod
    def _opposite_opts(contexts, min_mapq, min_phred, ignore_5p, ignore_3p):
        i5, i3 = tuple(int(x) for x in ignore_5p), tuple(int(x) for x in ignore_3p)
        if len(i5) != 2 or len(i3) != 2:
            raise ValueError("ignore_5p and ignore_3p: one value per mate")
        return capi.MethylOpts(int(contexts), int(min_mapq), int(min_phred), 0, (C.c_int32 * 2)(*i5), (C.c_int32 * 2)(*i3))

    def bam_methyl_opposite(self, records: bytes, lens, clip=None, contexts: int = 1, min_mapq: int = 10, min_phred: int = 5, ignore_5p=(0, 0),
                            ignore_3p=(0, 0)) -> np.ndarray:
        """the records of bam_methyl -> what they show of the OTHER strand's cytosines: per (ref, pos) where an OB record lies over a
        forward C of a selected context or an OT record over a forward G, the read bases that are another letter (meth) and the genome's
        own (unmeth), ordered by (ref, pos) (bmbs_bam_methyl_opposite); drop_variants() filters a call's sites with them"""
        ln = np.ascontiguousarray(lens, dtype=np.uint32)
        a = np.frombuffer(records, dtype=np.uint8) if len(records) else np.zeros(1, dtype=np.uint8)
        cl = None if clip is None else np.ascontiguousarray(clip, dtype=np.uint32)
        if cl is not None and cl.size != ln.size:
            raise ValueError("bam_methyl_opposite: one clip per record")
        opts = self._opposite_opts(contexts, min_mapq, min_phred, ignore_5p, ignore_3p)
        n = C.c_int64(0)
        self._chk(self._lib.bmbs_bam_methyl_opposite(self._ctx, capi.ptr(a), len(records), capi.ptr(ln) if ln.size else None, ln.size,
                                                     capi.ptr(cl) if cl is not None and cl.size else None, C.byref(opts), C.byref(n)))
        return self.methyl_opposite()

    def bam_sort_methyl_opposite(self, clip=None, contexts: int = 1, min_mapq: int = 10, min_phred: int = 5, ignore_5p=(0, 0), ignore_3p=(0, 0)) -> np.ndarray:
        """the same for the records of the last bam_sort call, which are still on the device; clip in that call's input order
        (bmbs_bam_sort_methyl_opposite)"""
        cl = None if clip is None else np.ascontiguousarray(clip, dtype=np.uint32)
        opts = self._opposite_opts(contexts, min_mapq, min_phred, ignore_5p, ignore_3p)
        n = C.c_int64(0)
        self._chk(self._lib.bmbs_bam_sort_methyl_opposite(self._ctx, capi.ptr(cl) if cl is not None and cl.size else None, C.byref(opts), C.byref(n)))
        return self.methyl_opposite()

    def methyl_report(self, ref: int, beg: int, end: int, sites, runs=None, contexts: int = 1) -> bytes:
        """the cytosine-report lines of forward positions [beg, end) of sequence ref (bmbs_methyl_report): one line per cytosine of a
        selected context, covered or not.  sites: capi.METHYL_SITE_DTYPE, those of that window in position order (kind | capi.REPORT_OMIT:
        no line there); runs: the [beg, end) runs of that sequence that the FASTA does not spell A, C, G or T.  The size query, then the call"""
        self._set_refs()
        st = np.ascontiguousarray(sites, dtype=capi.METHYL_SITE_DTYPE)
        rn = np.ascontiguousarray(runs if runs is not None else [], dtype=np.int64).reshape(-1, 2)
        args = (self._ctx, int(ref), int(beg), int(end), capi.ptr(st) if st.size else None, st.size, capi.ptr(rn) if rn.size else None, rn.shape[0], int(contexts))
        used = C.c_uint64(0); lines = C.c_int64(0)
        rc = self._lib.bmbs_methyl_report(*args, None, 0, C.byref(used), C.byref(lines))
        if rc and rc != -12:
            self._chk(rc)
        out = np.empty(max(1, used.value), dtype=np.uint8)
        self._chk(self._lib.bmbs_methyl_report(*args, capi.ptr(out), used.value, C.byref(used), C.byref(lines)))
        self.report_lines = lines.value
        return out[:used.value].tobytes()

    def sync(self):
        self._chk(self._lib.bmbs_sync(self._ctx))

    # ---- stages -------------------------------------------------------------------------------------
    def locate(self, rows: np.ndarray) -> np.ndarray:
        """K5: text position SA[row] of suffix-array rows"""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = np.zeros(rows.size, dtype=np.uint64)
        self._chk(self._lib.bmbs_locate_batch(self._ctx, capi.ptr(rows), rows.size, capi.ptr(out)))
        return out

    def vote_order(self, vote: np.ndarray, seg_off: np.ndarray, form: int) -> np.ndarray:
        """a9: the visiting order std::sort gives each vote list vote[seg_off[s]:seg_off[s+1]] (form 0: wave kernel, 1: block kernel)"""
        vote = np.ascontiguousarray(vote, dtype=np.uint8)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        perm = np.zeros(vote.size, dtype=np.uint32)
        self._chk(self._lib.bmbs_vote_order_batch(self._ctx, capi.ptr(vote), capi.ptr(seg_off), seg_off.size - 1, form, capi.ptr(perm)))
        return perm

    def windows(self, site: np.ndarray, length: int) -> np.ndarray:
        """K7: the doubled-genome windows starting at `site` (uint64), uint8 [n, length] (0 bytes = out-of-strand)"""
        site = np.ascontiguousarray(site, dtype=np.uint64)
        out = np.zeros((site.size, length), dtype=np.uint8)
        self._chk(self._lib.bmbs_window_batch(self._ctx, capi.ptr(site), site.size, length, capi.ptr(out)))
        return out

    def filter(self, seq: np.ndarray, L: int, read_of: np.ndarray, site: np.ndarray, packed: bool = False):
        """K7+K8 on (read, site) pairs.  packed: the rows are packed on the device first and the Myers rows read the packed words -- the
        form the mapping calls run (bmbs_filter_batch_packed)"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        read_of = np.ascontiguousarray(read_of, dtype=np.uint32)
        site = np.ascontiguousarray(site, dtype=np.uint64)
        m = read_of.size
        err = np.zeros(m, dtype=np.uint32)
        end = np.zeros(m, dtype=np.int32)
        fn = self._lib.bmbs_filter_batch_packed if packed else self._lib.bmbs_filter_batch
        self._chk(fn(self._ctx, capi.ptr(seq), L, seq.shape[1], seq.shape[0], capi.ptr(read_of),
                                              capi.ptr(site), m, capi.ptr(err), capi.ptr(end)))
        return err, end

    def align(self, seq, qual, L, read_of, site, end_in, err_in, packed: bool = False, rev_from: int | None = None):
        """K11-K13 on (read, site, end, err) jobs; ops[j][:n_ops[j]] = the operations of job j (n_ops 0: all M).  packed: the rows are
        packed on the device first and the DP form is chosen as in a mapping call (bmbs_align_batch_packed); rev_from (packed only):
        reads from this index on read their qualities mirrored"""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        read_of = np.ascontiguousarray(read_of, dtype=np.uint32)
        site = np.ascontiguousarray(site, dtype=np.uint64)
        end_in = np.ascontiguousarray(end_in, dtype=np.int32)
        err_in = np.ascontiguousarray(err_in, dtype=np.uint32)
        m = read_of.size
        if rev_from is not None and not packed:
            raise ValueError("rev_from needs packed=True (bmbs_align_batch has no such argument)")
        max_ops = self.max_cigar_ops(L)
        out = {k: np.zeros(m, dtype=t) for k, t in (("start", np.int32), ("end", np.int32), ("nm", np.uint32),
                                                     ("score", np.int32), ("n_ops", np.int32))}
        ops = np.zeros((m, max_ops), dtype=np.uint32)
        args = (self._ctx, capi.ptr(seq), capi.ptr(qual), L, seq.shape[1], seq.shape[0],
                capi.ptr(read_of), capi.ptr(site), capi.ptr(end_in), capi.ptr(err_in), m,
                capi.ptr(out["start"]), capi.ptr(out["end"]), capi.ptr(out["nm"]),
                capi.ptr(out["score"]), capi.ptr(ops), capi.ptr(out["n_ops"]), max_ops)
        if packed:
            self._chk(self._lib.bmbs_align_batch_packed(*args, 0xFFFFFFFF if rev_from is None else int(rev_from)))
        else:
            self._chk(self._lib.bmbs_align_batch(*args))
        out["ops"] = ops
        return out

    def seed(self, seq: np.ndarray, L: int, vote_cap: int | None = None):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        n, stride = seq.shape
        cap = vote_cap or max(1024, 64 * n)
        verdict = np.zeros(n, dtype=np.uint8)
        exit_site = np.zeros(n, dtype=np.uint64)
        seg_off = np.zeros(n + 1, dtype=np.uint64)
        n_votes = np.zeros(n, dtype=np.uint32)
        vsite = np.zeros(cap, dtype=np.uint64)
        vcnt = np.zeros(cap, dtype=np.uint32)
        tot = C.c_int64(0)
        self._chk(self._lib.bmbs_seed_batch(self._ctx, capi.ptr(seq), L, stride, n, capi.ptr(verdict), capi.ptr(exit_site),
                                            capi.ptr(seg_off), capi.ptr(n_votes), capi.ptr(vsite), capi.ptr(vcnt), cap,
                                            C.byref(tot)))
        return dict(verdict=verdict, exit_site=exit_site, seg_off=seg_off, n_votes=n_votes, vote_site=vsite[:tot.value],
                    vote_cnt=vcnt[:tot.value])

    # ---- stats / measurement -----------------------------------------------------------------------
    def stats(self) -> np.ndarray:
        s = np.zeros(5, dtype=np.int64)
        self._chk(self._lib.bmbs_stats_get(self._ctx, capi.ptr(s)))
        return s

    def reset_stats(self):
        self._chk(self._lib.bmbs_stats_reset(self._ctx))

    def profile(self) -> list[tuple[str, float]]:
        n = C.c_int(512)
        names = (C.c_char_p * 512)()
        ms = (C.c_float * 512)()
        self._chk(self._lib.bmbs_profile_last(self._ctx, names, ms, C.byref(n)))
        return [(names[i].decode(), float(ms[i])) for i in range(n.value)]

    def profile_total(self) -> tuple[dict, int]:
        """({kernel: ms summed over the mapping calls since profile_reset()}, number of lane-calls)"""
        n = C.c_int(512)
        names = (C.c_char_p * 512)()
        ms = (C.c_double * 512)()
        calls = C.c_int64(0)
        self._chk(self._lib.bmbs_profile_total(self._ctx, names, ms, C.byref(n), C.byref(calls)))
        return {names[i].decode(): float(ms[i]) for i in range(n.value)}, int(calls.value)

    def profile_reset(self):
        self._chk(self._lib.bmbs_profile_reset(self._ctx))

    def retries(self) -> int:
        """calls that were issued again with exact sizes (a stage count exceeded the learned capacity); diagnostic"""
        return int(self._lib.bmbs_retries(self._ctx))

    def counters(self) -> dict:
        c = np.zeros(32, dtype=np.uint64)
        self._chk(self._lib.bmbs_counters_all(self._ctx, capi.ptr(c)))
        keys = ("n_hash", "n_ext", "n_sa", "n_filter", "n_sw", "n_ungapped", "n_cand_slots", "n_jobs")
        d = {k: int(v) for k, v in zip(keys, c[:8])}
        d["n_jump"] = int(c[8])          # three-letter index steps taken (each counts three in n_ext)
        # what the list kernels handled (round 6): candidates located by the mid / wave / block forms, their lists, the entries
        # filter_pairs read, re-seeded candidates (--sensitive), sites dropped by the paired-end pre-filter
        for j, nm in enumerate(("n_cand_mid", "n_cand_long", "n_cand_big", "n_lists_long", "n_pef_entries", "n_cand_reseed", "n_prefilter_drop")):
            d[nm] = int(c[9 + j])
        for kid, nm in enumerate(("k_seed_first", "k_seed_second", "k_seed_extra")):
            d[nm] = {"n_hash": int(c[16 + 4 * kid]), "n_ext": int(c[17 + 4 * kid]), "n_sa": int(c[18 + 4 * kid])}
        return d


# ---- packed quality classes (host arithmetic only: no device, no Mapper needed) ---------------------
def qual_classes(params: capi.Params | None = None):
    """bmbs_qual_classes -> (class_of u8[256], penalty_of i32[n_classes]); params None: the defaults"""
    class_of = np.zeros(256, dtype=np.uint8)
    pen = np.zeros(16, dtype=np.int32)
    nc = C.c_int32(0)
    rc = capi.lib().bmbs_qual_classes(C.byref(params) if params is not None else None, capi.ptr(class_of), capi.ptr(pen), C.byref(nc))
    if rc:
        raise RuntimeError("bmbs_qual_classes failed (%d)" % rc)
    return class_of, pen[:nc.value].copy()


def pack_quals(params, qual: np.ndarray, L: int, lens: np.ndarray | None = None, qwords: int | None = None, threads: int = 8) -> np.ndarray:
    """bmbs_pack_quals: quality rows [n][stride] -> class rows [n][qwords] of u64 under `params` (None: the defaults)"""
    a = np.ascontiguousarray(qual, dtype=np.uint8)
    n, stride = a.shape
    if qwords is None:
        qwords = (L + 15) // 16
    qrows = np.empty((n, qwords), dtype=np.uint64)
    bad = C.c_int64(-1)
    ln = np.ascontiguousarray(lens, dtype=np.uint16) if lens is not None else None
    rc = capi.lib().bmbs_pack_quals(C.byref(params) if params is not None else None, capi.ptr(a), L, stride, n,
                                    capi.ptr(ln) if ln is not None else None, capi.ptr(qrows), qwords, threads, C.byref(bad))
    if rc:
        raise ValueError("bmbs_pack_quals: row %d cannot be packed (rc %d)" % (bad.value, rc))
    return qrows


# ---- the variant filter of the methylation calls (host arithmetic only: no device, no Mapper needed) ----
def drop_variants(site: np.ndarray, opp: np.ndarray, min_opposite_depth: int, max_variant_ppm: int) -> np.ndarray:
    """bmbs_methyl_drop_variants: the sites (capi.METHYL_SITE_DTYPE, ordered by (ref, pos)) without those where the opposite-strand
    entries `opp` (Mapper.methyl_opposite) show at least min_opposite_depth bases of which more than max_variant_ppm / 10^6 are a
    variant; a new array, the arguments stay as they are"""
    s = np.array(site, dtype=capi.METHYL_SITE_DTYPE, copy=True, ndmin=1)
    o = np.ascontiguousarray(opp, dtype=capi.METHYL_SITE_DTYPE)
    kept = C.c_int64(0)
    rc = capi.lib().bmbs_methyl_drop_variants(capi.ptr(s) if s.size else None, s.size, capi.ptr(o) if o.size else None, o.size,
                                              int(min_opposite_depth), int(max_variant_ppm), C.byref(kept))
    if rc:
        raise ValueError("bmbs_methyl_drop_variants: a list out of order, min_opposite_depth < 1 or max_variant_ppm outside 0..1000000 (rc %d)" % rc)
    return s[:kept.value]


# ---- SAM text (host emit) --------------------------------------------------------------------------
def cigar_text(res_row, pool: np.ndarray, L: int) -> str:
    n = int(res_row["n_cigar"])
    if n == 0:
        return "%dM" % L
    if n == 255:
        raise ValueError("an alignment overflowed its CIGAR slots (bmbs_max_cigar_ops rules this out: internal error)")
    ops = pool[int(res_row["cigar_off"]):int(res_row["cigar_off"]) + n]
    return "".join("%d%s" % (int(o) >> 4, "MDISH"[int(o) & 0xf]) for o in ops)


def sam_header(index: Index, command_line: str = "") -> str:
    """OutPutSAM_Nounheader, Process_sam_out.cpp:1137-1153"""
    out = ["@HD\tVN:1.4\tSO:unsorted"]
    for nm, ln in zip(index.chrom_names, index.chrom_len):
        out.append("@SQ\tSN:%s\tLN:%d" % (nm, int(ln)))
    out.append("@PG\tID:BitMapperBS\tVN:1.0.2.3\tCL:%s" % command_line)
    return "\n".join(out) + "\n"


def sam_lines_se(index: Index, names, seq: np.ndarray, qual: np.ndarray, L: int, res: np.ndarray, pool: np.ndarray):
    """output_sam_end_to_end text branch (Schema.cpp:11989-12039); one line per uniquely mapped read."""
    out = []
    for i in np.nonzero(res["status"] == capi.ST_UNIQUE)[0]:
        r = res[i]
        nm = names[i]
        if isinstance(nm, bytes):
            nm = nm.decode()
        if nm.startswith("@"):
            nm = nm[1:]
        for cut in (" ", "/"):
            j = nm.find(cut)
            if j >= 0:
                nm = nm[:j]
        s, q = seq[i, :L], qual[i, :L]
        if int(r["flag"]) & 16:
            s = _COMP[s][::-1]
            q = q[::-1]
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\n" % (
            nm, int(r["flag"]), index.chrom_names[int(r["chrom"])], int(r["pos"]), int(r["mapq"]),
            cigar_text(r, pool, L), s.tobytes().decode(), q.tobytes().decode(), int(r["nm"])))
    return out


def pe_name(n1, n2) -> str:
    """inputReads_paired_directly (Process_Reads.cpp:296-307): cut at the first differing char, ' ' or '/'"""
    a = n1.decode() if isinstance(n1, bytes) else n1
    b = n2.decode() if isinstance(n2, bytes) else n2
    j = 0
    while j < len(a) and j < len(b) and a[j] == b[j] and a[j] not in " /":
        j += 1
    a = a[:j]
    return a[1:] if a.startswith("@") else a


def sam_lines_pe(index: Index, names1, names2, seq1, qual1, seq2, qual2, L: int, res: np.ndarray, pool: np.ndarray):
    """directly_output_read1 / directly_output_read2 (Schema.cpp:10537-10640, 11494-11590); two lines per unique pair"""
    out = []
    n = seq1.shape[0]
    for i in range(n):
        r1, r2 = res[2 * i], res[2 * i + 1]
        if int(r1["status"]) != capi.ST_UNIQUE:
            continue
        nm = pe_name(names1[i], names2[i])
        tlen = int(r1["tlen"])
        p1, p2 = int(r1["pos"]), int(r2["pos"])
        t1 = "-%d" % tlen if p2 < p1 else "%d" % tlen           # read 1: negative only if the mate lies to the left
        t2 = "%d" % tlen if p1 > p2 else "-%d" % tlen           # read 2: positive only if the mate lies to the right
        s1, q1 = seq1[i, :L], qual1[i, :L]
        if not (int(r1["flag"]) & 32):
            s1 = _COMP[s1][::-1]; q1 = q1[::-1]
        s2, q2 = seq2[i, :L], qual2[i, :L]                       # FASTQ orientation
        if int(r2["flag"]) & 16:
            s2 = _COMP[s2][::-1]; q2 = q2[::-1]
        chrom1 = index.chrom_names[int(r1["chrom"])]; chrom2 = index.chrom_names[int(r2["chrom"])]
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t=\t%d\t%s\t%s\t%s\tNM:i:%d\n" % (
            nm, int(r1["flag"]), chrom1, p1, int(r1["mapq"]), cigar_text(r1, pool, L), p2, t1,
            s1.tobytes().decode(), q1.tobytes().decode(), int(r1["nm"])))
        out.append("%s\t%d\t%s\t%d\t%d\t%s\t=\t%d\t%s\t%s\t%s\tNM:i:%d\n" % (
            nm, int(r2["flag"]), chrom2, p2, int(r2["mapq"]), cigar_text(r2, pool, L), p1, t2,
            s2.tobytes().decode(), q2.tobytes().decode(), int(r2["nm"])))
    return out
