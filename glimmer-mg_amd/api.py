"""Thin object wrappers over the C ABI (include/gmg.h, include/gmg_icm.h) for tests and bench.py.

Names follow the reference: an Icm is an ICM_t (src/ICM/icm.hh:116-180), reads are the sequences
glimmer3 / glimmer-mg score, a segment is an ORF-style scoring buffer cut from a read.
Nothing here computes a score: every function forwards to libgmg.so and raises GmgError with the
library's message when a call fails (including "no GPU").
"""
import ctypes as C
import numpy as np

from . import capi

FORWARD, REVERSED, COMPLEMENTED, REVCOMP = 0, 1, 2, 3
DEFAULT_STOPS = ("taa", "tag", "tga")     # src/Glimmer/glimmer_base.cc Set_Start_And_Stop_Codons defaults


class GmgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gmg status %d: %s" % (code, msg))
        self.code = code


def _ck(rc):
    if rc != 0:
        raise GmgError(rc, capi.lib().gmg_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def init(device=0):
    """gmg_init: bind this process to one GPU.  Raises GmgError (GMG_ENODEV) without a gfx950 device."""
    _ck(capi.lib().gmg_init(int(device)))


def set_option(key, value):
    """gmg_set_option: tuning / test switches (include/gmg.h)"""
    _ck(capi.lib().gmg_set_option(key.encode(), int(value)))


def get_option(key):
    v = C.c_longlong()
    _ck(capi.lib().gmg_get_option(key.encode(), C.byref(v)))
    return v.value


class option:
    """with gmg.option("mg_err_flat", 1): ...   -- sets a switch for the block and restores it"""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = get_option(self.key)
        set_option(self.key, self.value)

    def __exit__(self, *exc):
        set_option(self.key, self.old)


def read_fasta(path):
    """Host-side ingest with the reference's semantics (src/Common/fasta.cc:236-286 Fasta_Read):
    header = text after '>' (leading blanks skipped) up to the newline; sequence = every
    non-whitespace character up to the next '>'.  Returns (headers, sequences) as str lists."""
    hdrs, seqs = [], []
    with open(path, "rb") as fh:
        data = fh.read()
    pos = data.find(b">")
    while pos >= 0:
        pos += 1
        while pos < len(data) and data[pos:pos + 1] == b" ":
            pos += 1
        eol = data.find(b"\n", pos)
        if eol < 0:
            eol = len(data)
        nxt = data.find(b">", eol)
        body = data[eol:nxt if nxt >= 0 else len(data)]
        hdrs.append(data[pos:eol].decode("latin-1"))
        seqs.append(b"".join(body.split()).decode("latin-1"))
        pos = nxt
    return hdrs, seqs


class _DeviceBuffer:
    """device scratch from gmg_device_malloc, copied back with gmg_memcpy_d2h"""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        _ck(capi.lib().gmg_device_malloc(C.byref(self.ptr), self.nbytes))

    @classmethod
    def from_host(cls, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        buf = cls(max(arr.nbytes, 1))
        if arr.nbytes:
            _ck(capi.lib().gmg_memcpy_h2d(buf.ptr, _ptr(arr), arr.nbytes, stream))
        return buf

    def to_host(self, dtype, count, stream=None):
        out = np.empty(count, dtype)
        if out.nbytes:
            _ck(capi.lib().gmg_memcpy_d2h(_ptr(out), self.ptr, out.nbytes, stream))
        return out

    def free(self):
        if self.ptr:
            capi.lib().gmg_device_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Icm:
    """Host ICM_t behind gmg_icm (model I/O + null-model builder run on the host, as in the reference)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def open(cls, path):
        h = C.c_void_p()
        _ck(capi.lib().gmg_icm_open(str(path).encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def new(cls, model_len=12, model_depth=7, periodicity=3):
        h = C.c_void_p()
        _ck(capi.lib().gmg_icm_new(model_len, model_depth, periodicity, C.byref(h)))
        return cls(h)

    @classmethod
    def indep(cls, gc_frac, stops=DEFAULT_STOPS):
        """ICM_t Indep_Model(3,2,3); Indep_Model.Build_Indep_WO_Stops(gc, stops)  (glimmer3.cc:64,214)"""
        m = cls.new(3, 2, 3)
        arr = (C.c_char_p * len(stops))(*[s.encode() for s in stops])
        _ck(capi.lib().gmg_icm_build_indep(m.h, float(gc_frac), arr, len(stops)))
        return m

    @classmethod
    def train(cls, strings, model_len=12, model_depth=7, periodicity=3):
        """ICM_Training_t model(w, d, p); model.Train_Model(strings)  (src/ICM/build-icm.cc:67,120).  strings: lower-case
        str/bytes in the orientation Train_Model gets them.  The counting runs on the device (gmg_trainer_*)."""
        raw = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in strings]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        h = C.c_void_p()
        _ck(capi.lib().gmg_icm_train(arr, len(raw), model_len, model_depth, periodicity, C.byref(h)))
        return cls(h)

    @classmethod
    def train_reads(cls, reads, model_len=12, model_depth=7, periodicity=3):
        """gmg_icm_train_reads: the same from training strings that already are a batch on the device (Reads.extract)"""
        h = C.c_void_p()
        _ck(capi.lib().gmg_icm_train_reads(reads.h, model_len, model_depth, periodicity, C.byref(h)))
        return cls(h)

    @property
    def params(self):
        w, d, p, n = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _ck(capi.lib().gmg_icm_params(self.h, C.byref(w), C.byref(d), C.byref(p), C.byref(n)))
        return w.value, d.value, p.value, n.value

    def tables(self):
        """(mip int16 [P,N], prob float32 [P,N,4])"""
        _, _, p, n = self.params
        mip = np.empty((p, n), np.int16)
        prob = np.empty((p, n, 4), np.float32)
        _ck(capi.lib().gmg_icm_tables(self.h, _ptr(mip), _ptr(prob)))
        return mip, prob

    def write(self, path):
        _ck(capi.lib().gmg_icm_write(self.h, str(path).encode()))

    def device(self):
        """gmg_model handle (uploaded once, owned by this Icm)"""
        out = C.c_void_p()
        _ck(capi.lib().gmg_icm_device_model(self.h, C.byref(out)))
        return out

    def close(self):
        if self.h:
            capi.lib().gmg_icm_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SetModel:
    """member k of a ModelSet: usable wherever an Icm's device model is (the set owns it)"""

    def __init__(self, owner, handle):
        self.owner, self.h = owner, handle

    def device(self):
        if not self.owner.h:
            raise GmgError(-1, "the ModelSet of this model is closed")
        return self.h


class ModelSet:
    """gmg_model_set: the raw bytes of many binary .icm files parsed and flattened on the device, in one block.
    ModelSet.load queues the work on `stream` and returns; finish() waits and raises GmgError (with .bad_file) when the device
    refused a file; model(k) is valid after finish()."""

    def __init__(self, handle, blobs, n):
        self.h, self._blobs, self.n, self._done = handle, blobs, n, False

    @classmethod
    def load(cls, list_of_bytes, stream=None):
        blobs = [np.frombuffer(bytes(b), np.uint8) if len(b) else np.zeros(0, np.uint8) for b in list_of_bytes]     # kept until finish()
        n = len(blobs)
        ptrs = (C.c_void_p * max(n, 1))(*[b.ctypes.data if b.size else None for b in blobs])
        sizes = (C.c_uint64 * max(n, 1))(*[b.size for b in blobs])
        h = C.c_void_p()
        _ck(capi.lib().gmg_model_set_load(ptrs, sizes, n, C.byref(h), stream))
        return cls(h, blobs, n)

    def finish(self):
        bad = C.c_int(-1)
        rc = capi.lib().gmg_model_set_finish(self.h, C.byref(bad))
        self._blobs = None
        if rc != 0:
            err = GmgError(rc, capi.lib().gmg_last_error().decode("utf-8", "replace"))
            err.bad_file = bad.value
            raise err
        self._done = True
        return self

    def model(self, k):
        if not self._done:
            self.finish()
        h = capi.lib().gmg_model_set_model(self.h, int(k))
        if not h:
            raise GmgError(-1, capi.lib().gmg_last_error().decode("utf-8", "replace"))
        return _SetModel(self, C.c_void_p(h))

    def __len__(self):
        return self.n

    def close(self):
        if self.h:
            capi.lib().gmg_model_set_free(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def icm_bytes_info(data):
    """gmg_icm_bytes_info: (model_len, model_depth, periodicity, num_nodes, blob_bytes) of a binary .icm's bytes (host only)"""
    buf = np.frombuffer(bytes(data), np.uint8)
    w, d, p, n, b = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
    _ck(capi.lib().gmg_icm_bytes_info(buf.ctypes.data if buf.size else None, buf.size, C.byref(w), C.byref(d), C.byref(p), C.byref(n), C.byref(b)))
    return w.value, d.value, p.value, n.value, b.value


def model_info(m):
    """gmg_model_info of an Icm's or a ModelSet member's device model: (model_len, model_depth, periodicity, num_nodes)"""
    w, d, p, n = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _ck(capi.lib().gmg_model_info(m.device(), C.byref(w), C.byref(d), C.byref(p), C.byref(n)))
    return w.value, d.value, p.value, n.value


def model_blob(m):
    """gmg_model_blob: the device tables of a model as bytes, in gmg_model_upload's layout"""
    size = C.c_size_t(0)
    _ck(capi.lib().gmg_model_blob(m.device(), None, C.byref(size)))
    out = np.empty(size.value, np.uint8)
    _ck(capi.lib().gmg_model_blob(m.device(), _ptr(out), C.byref(size)))
    return out.tobytes()


def model_value_stats(m):
    """gmg_model_value_stats: (min_exp, max_exp, odd_values)"""
    lo, hi, odd = C.c_int(), C.c_int(), C.c_int()
    _ck(capi.lib().gmg_model_value_stats(m.device(), C.byref(lo), C.byref(hi), C.byref(odd)))
    return lo.value, hi.value, odd.value


class NullSet:
    """gmg_null_set: (3,2,3) null models side by side on the device (glimmer-mg -c: Indep_Model per read)"""

    def __init__(self, icms):
        self.icms = list(icms)                           # keep the host models (and their device mirrors) alive
        arr = (C.c_void_p * len(self.icms))(*[m.device() for m in self.icms])
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_null_set_upload(arr, len(self.icms), C.byref(self.h)))

    @classmethod
    def build(cls, gcs, stops=DEFAULT_STOPS):
        """gmg_null_set_build: Build_Indep_WO_Stops (gc, stops) for every GC value, one upload"""
        self = cls.__new__(cls)
        gcs = np.ascontiguousarray(gcs, np.float64)
        buf = ((C.c_char * 4) * 8)()
        for i, c in enumerate(stops):
            buf[i].value = c.encode()
        self.icms = [Icm.indep(float(gcs[0]), stops)]    # (mg_score_reads wants a model object for the unused null argument)
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_null_set_build(_ptr(gcs), len(gcs), buf, len(stops), C.byref(self.h)))
        return self

    def close(self):
        if self.h:
            capi.lib().gmg_null_set_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_strings(seqs):
    """Filter + lower + 2-bit pack a list of str/bytes sequences -> (packed uint32, offsets uint64)."""
    lens = np.array([len(s) for s in seqs], np.uint64)
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    packed = np.zeros(int(capi.lib().gmg_packed_words(total)), np.uint32)
    blob = b"".join(s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs)
    _ck(capi.lib().gmg_pack_bases(blob, total, 0, _ptr(packed)))
    return packed, off


class Reads:
    """A batch of reads resident in HBM (gmg_reads)."""

    def __init__(self, packed, offsets):
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        packed = np.ascontiguousarray(packed, np.uint32)
        self.n_reads = len(self.offsets) - 1
        self.total_bases = int(self.offsets[-1]) if len(self.offsets) else 0
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_reads_upload(_ptr(packed), _ptr(self.offsets), self.n_reads, C.byref(self.h)))

    @classmethod
    def from_strings(cls, seqs):
        return cls(*pack_strings(seqs))

    @classmethod
    def from_fasta_bytes(cls, data, stream=None):
        """gmg_fasta_ingest_on: the file's bytes are parsed on the device (Fasta_Read + Filter + tolower + 2-bit packing), every copy
        and kernel on `stream`.  -> (Reads, headers [bytes], gc_count)"""
        data = bytes(data)
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        index = C.c_void_p()
        _ck(capi.lib().gmg_fasta_ingest_on(data, len(data), C.byref(self.h), C.byref(index), stream))
        try:
            n, total, gc = C.c_uint64(), C.c_uint64(), C.c_uint64()
            _ck(capi.lib().gmg_fasta_info(index, C.byref(n), C.byref(total), C.byref(gc)))
            hb, he = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint64)
            _ck(capi.lib().gmg_fasta_headers(index, _ptr(hb), _ptr(he)))
        finally:
            capi.lib().gmg_fasta_free(index)
        self.n_reads, self.total_bases = int(n.value), int(total.value)
        self.offsets = None                              # live on the device only
        headers = [data[int(b):int(e)] for b, e in zip(hb[:n.value], he[:n.value])]
        return self, headers, int(gc.value)

    def download(self):
        """-> (packed uint32 words, offsets uint64): the batch as it sits in HBM (tests)"""
        n, total = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_reads_info(self.h, C.byref(n), C.byref(total)))
        words = int(capi.lib().gmg_packed_words(total.value))
        packed, off = np.zeros(max(words, 1), np.uint32), np.zeros(n.value + 1, np.uint64)
        _ck(capi.lib().gmg_reads_download(self.h, _ptr(packed), _ptr(off)))
        return packed[:words], off

    def select(self, idx):
        """gmg_reads_select: a new device batch made of the reads idx (any order, repeats allowed)"""
        idx = np.ascontiguousarray(idx, np.uint64)
        sub = Reads.__new__(Reads)
        sub.h = C.c_void_p()
        _ck(capi.lib().gmg_reads_select(self.h, _ptr(idx), len(idx), C.byref(sub.h)))
        n, total = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_reads_info(sub.h, C.byref(n), C.byref(total)))
        sub.n_reads, sub.total_bases, sub.offsets = int(n.value), int(total.value), None
        return sub

    def extract(self, regions, reversed=False, amb=None):
        """gmg_reads_extract: a new device batch whose string k is region k = (read, first, len, strand) of this one, modulo its
        read, strand < 0 downwards and complemented; reversed: every string back to front (build-icm -r); amb: (base indices,
        codes) of fasta_ambiguous, the letters whose reverse-strand code is not the code complement"""
        arr = (capi.GeneRegion * max(len(regions), 1))(*[capi.GeneRegion(int(r), int(f), int(ln), int(s)) for r, f, ln, s in regions])
        base, code, n_amb = None, None, 0
        if amb is not None and len(amb[0]):
            base, code = np.ascontiguousarray(amb[0], np.uint64), np.ascontiguousarray(amb[1], np.uint8)
            n_amb = len(base)
        sub = Reads.__new__(Reads)
        sub.h = C.c_void_p()
        _ck(capi.lib().gmg_reads_extract(self.h, arr, len(regions), EXTRACT_REVERSED if reversed else 0,
                                         _ptr(base) if n_amb else None, _ptr(code) if n_amb else None, n_amb, C.byref(sub.h)))
        n, total = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_reads_info(sub.h, C.byref(n), C.byref(total)))
        sub.n_reads, sub.total_bases, sub.offsets = int(n.value), int(total.value), None
        return sub

    def splice(self, runs, string_run_off, reversed=False):
        """gmg_reads_splice: a new device batch whose string k is the concatenation of runs[string_run_off[k] : string_run_off[k + 1]],
        a run = (read, first, len, kind) with kind one of RUN_UP, RUN_DOWN, RUN_SUB_UP, RUN_SUB_DOWN, RUN_LITERAL + code,
        RUN_LITERAL_AS_IS + code; reversed: every string back to front"""
        runs = np.ascontiguousarray(np.asarray(runs, np.uint32).reshape(-1, 4))
        sro = np.ascontiguousarray(string_run_off, np.uint64)
        sub = Reads.__new__(Reads)
        sub.h = C.c_void_p()
        _ck(capi.lib().gmg_reads_splice(self.h, _ptr(runs) if len(runs) else None, len(runs), _ptr(sro), len(sro) - 1,
                                        EXTRACT_REVERSED if reversed else 0, C.byref(sub.h)))
        n, total = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_reads_info(sub.h, C.byref(n), C.byref(total)))
        sub.n_reads, sub.total_bases, sub.offsets = int(n.value), int(total.value), None
        return sub

    def close(self):
        if self.h:
            capi.lib().gmg_reads_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


EXTRACT_REVERSED = 1                                    # GMG_EXTRACT_REVERSED
COORD_USE_DIR, COORD_NOWRAP, COORD_SKIP_START, COORD_SKIP_STOP, COORD_MULTI = 1, 2, 4, 8, 16      # GMG_COORD_*


RUN_UP, RUN_DOWN, RUN_SUB_UP, RUN_SUB_DOWN, RUN_LITERAL, RUN_LITERAL_AS_IS = 0, 1, 2, 3, 4, 8      # GMG_RUN_*


def edits_plan(offsets, genes, odd=None):
    """gmg_edits_plan (host): the gene lines of a predict file -- (read, column 2, column 3, frame, insertions, deletions,
    substitutions), positions 1-based as written, in file order -- to the strings extract_aa.py prints: -> (runs uint32 [n, 4],
    string_run_off uint64, strings [(line, start, end, strand, pad_front, pad_behind)]).  odd: (base indices, letters) of the
    bases whose letter is no upper-case A C G T"""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    arr = (capi.EditGene * max(len(genes), 1))(*[capi.EditGene(int(g[0]), int(g[3]), int(g[1]), int(g[2]), len(g[4]), len(g[5]), len(g[6]), 0)
                                                  for g in genes])
    pos = np.array([p for g in genes for lst in g[4:7] for p in lst] + [0], np.int64)
    odd_base, odd_letter, n_odd = None, None, 0
    if odd is not None and len(odd[0]):
        odd_base, odd_letter, n_odd = np.ascontiguousarray(odd[0], np.uint64), bytes(odd[1]), len(odd[0])
    strings = (capi.EditString * max(len(genes), 1))()
    sro = np.zeros(len(genes) + 1, np.uint64)
    n = C.c_uint64()
    args = (_ptr(offsets), len(offsets) - 1, arr, len(genes), _ptr(pos), _ptr(odd_base) if n_odd else None, odd_letter, n_odd)
    _ck(capi.lib().gmg_edits_plan(*args, None, 0, C.byref(n), _ptr(sro), strings))
    runs = np.zeros((max(n.value, 1), 4), np.uint32)
    _ck(capi.lib().gmg_edits_plan(*args, _ptr(runs), n.value, C.byref(n), _ptr(sro), strings))
    rows = [(int(s.gene), int(s.start), int(s.end), int(s.strand), int(s.pad_front), int(s.pad_behind)) for s in strings[:len(genes)]]
    return runs[:n.value], sro, rows


def fasta_ambiguous(data):
    """gmg_fasta_ambiguous (host): -> (base indices uint64, codes uint8) of the sequence bytes of a FASTA file outside acgtACGT:
    where gmg_fasta_ingest puts them, and Subscript (Complement (byte))"""
    data = bytes(data)
    n = C.c_uint64()
    _ck(capi.lib().gmg_fasta_ambiguous(data, len(data), None, None, 0, C.byref(n)))
    base, code = np.zeros(max(n.value, 1), np.uint64), np.zeros(max(n.value, 1), np.uint8)
    _ck(capi.lib().gmg_fasta_ambiguous(data, len(data), _ptr(base), _ptr(code), n.value, C.byref(n)))
    return base[:n.value], code[:n.value]


def fasta_not_upper_acgt(data):
    """gmg_fasta_not_upper_acgt (host): -> base indices uint64 of the sequence bytes of a FASTA file that are no upper-case ACGT"""
    data = bytes(data)
    n = C.c_uint64()
    _ck(capi.lib().gmg_fasta_not_upper_acgt(data, len(data), None, 0, C.byref(n)))
    base = np.zeros(max(n.value, 1), np.uint64)
    _ck(capi.lib().gmg_fasta_not_upper_acgt(data, len(data), _ptr(base), n.value, C.byref(n)))
    return base[:n.value]


FEATURES_BLOCK, FEATURES_LENGTHS, FEATURES_STARTS, FEATURES_ORIENTS, FEATURES_DIST = 0, 1, 2, 3, 4     # GMG_FEATURES_*


class FeatureTable:
    """One table of train_features.py (GENE or NON) after destrand_orientations: lengths int64 [1 + largest bin], starts int64 [3]
    (ATG GTG TTG), orient / orient_raw float64 [4] in the order (1,1) (1,-1) (-1,1) (-1,-1), dist: three float64 arrays, entry j the
    bin of distance j - max_overlap (empty array: empty table)."""

    def __init__(self, lengths, starts, orient, dist, orient_raw=None):
        self.lengths = np.ascontiguousarray(lengths, np.int64)
        self.starts = np.ascontiguousarray(starts, np.int64)
        self.orient = np.ascontiguousarray(orient, np.float64)
        self.orient_raw = np.ascontiguousarray(orient if orient_raw is None else orient_raw, np.float64)
        self.dist = [np.ascontiguousarray(d, np.float64) for d in dist]

    def _struct(self):
        t = capi.FeaturesTable()
        t.n_lengths = len(self.lengths)
        t.lengths = self.lengths.ctypes.data_as(C.POINTER(C.c_int64)) if len(self.lengths) else None
        for k in range(3):
            t.starts[k] = int(self.starts[k])
            t.n_dist[k] = len(self.dist[k])
            t.dist[k] = self.dist[k].ctypes.data_as(C.POINTER(C.c_double)) if len(self.dist[k]) else None
        for k in range(4):
            t.orient[k] = float(self.orient[k])
            t.orient_raw[k] = float(self.orient_raw[k])
        return t


def features_format(table, orf_type, what=FEATURES_BLOCK, max_overlap=50):
    """gmg_features_format (host): the text of output_featurefile's block for one table, or the body of one of output_stats' files"""
    t = table._struct()
    n = C.c_size_t(0)
    _ck(capi.lib().gmg_features_format(C.byref(t), orf_type.encode(), int(what), int(max_overlap), None, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    _ck(capi.lib().gmg_features_format(C.byref(t), orf_type.encode(), int(what), int(max_overlap), buf, C.byref(n)))
    return buf.raw[:n.value].decode()


def features_count(reads, genes, opaque=None, min_length=75, max_overlap=50, drop_tga=False, stream=None):
    """gmg_features_count: genes = [(read, strand, start, end, start_codon)] grouped by read, clipped; opaque = ascending job-wide
    indices of the bases that are no upper-case ACGT.  -> (GENE FeatureTable, NON FeatureTable, info dict)"""
    arr = (capi.FeatureGene * max(len(genes), 1))(*[capi.FeatureGene(int(r), int(s), int(a), int(b), int(bool(sc))) for r, s, a, b, sc in genes])
    n_opq = 0 if opaque is None else len(opaque)
    opq = np.ascontiguousarray(opaque, np.uint64) if n_opq else None
    prm = capi.FeaturesParams(int(min_length), int(max_overlap), int(bool(drop_tga)), 0)
    h = C.c_void_p()
    _ck(capi.lib().gmg_features_count(reads.h, arr, len(genes), _ptr(opq) if n_opq else None, n_opq, C.byref(prm), C.byref(h), stream))
    try:
        tables = []
        for which in (0, 1):
            t = capi.FeaturesTable()
            _ck(capi.lib().gmg_features_fetch(h, which, C.byref(t)))
            tables.append(FeatureTable(np.array(t.lengths[:t.n_lengths], np.int64), list(t.starts), list(t.orient),
                                       [np.array(t.dist[k][:t.n_dist[k]], np.float64) for k in range(3)], list(t.orient_raw)))
        n_units, n_rec = C.c_uint64(), C.c_uint64()
        ms = np.zeros(8, np.float32)
        _ck(capi.lib().gmg_features_info(h, C.byref(n_units), C.byref(n_rec), _ptr(ms)))
    finally:
        capi.lib().gmg_features_free(h)
    return tables[0], tables[1], {"n_units": n_units.value, "n_records": n_rec.value, "stage_ms": ms[:5].copy(), "host_ms": ms[5:8].copy()}


def extract_plan(offsets, coords, flags=0, min_len=0):
    """gmg_extract_plan (host): coordinate lines (read, start, end[, dir]), 1-based inclusive, -> (regions [(read, first, len,
    strand)], the line of every region) by extract's arithmetic, or multi-extract's with COORD_MULTI"""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    arr = (capi.Coord * max(len(coords), 1))(*[capi.Coord(int(c[0]), int(c[3]) if len(c) > 3 else 0, int(c[1]), int(c[2])) for c in coords])
    out = (capi.GeneRegion * max(len(coords), 1))()
    line = np.zeros(max(len(coords), 1), np.uint64)
    n = C.c_uint64()
    _ck(capi.lib().gmg_extract_plan(_ptr(offsets), len(offsets) - 1, arr, len(coords), int(flags), int(min_len), out, _ptr(line), C.byref(n)))
    return [(r.read, r.first, r.len, r.strand) for r in out[:n.value]], line[:n.value].copy()


def text_params(width=60, fwd=None, rev=None):
    """gmg_text_params_reference (host): the tables extract prints through -- every byte itself on the forward strand, the
    reference's Complement on the reverse strand -- unless fwd / rev (256 bytes each) replace them"""
    p = capi.TextParams()
    _ck(capi.lib().gmg_text_params_reference(C.byref(p), int(width)))
    for name, tab in (("fwd", fwd), ("rev", rev)):
        if tab is not None:
            tab = bytes(tab)
            assert len(tab) == 256
            C.memmove(getattr(p, name), tab, 256)
    return p


RUNS_TEXT_DNA, RUNS_TEXT_PROTEIN = 0, 1               # GMG_RUNS_TEXT_*


def runs_text_params(mode=RUNS_TEXT_DNA, transl_table=0, width=0, **fields):
    """gmg_runs_text_params_script (host): the rules extract_aa.py prints by, under the translation table given (0: the script's
    own) -- unless fields replace them: up / down / sub_up / sub_down (256 bytes each), literal (4), aa (64), pad, unknown (a byte)"""
    p = capi.RunsTextParams()
    _ck(capi.lib().gmg_runs_text_params_script(C.byref(p), int(mode), int(transl_table)))
    p.width = int(width)
    for name, value in fields.items():
        if name in ("pad", "unknown"):
            setattr(p, name, value if isinstance(value, int) else ord(value))
        else:
            value = bytes(value)
            field = getattr(capi.RunsTextParams, name)
            assert len(value) == field.size
            C.memmove(C.addressof(p) + field.offset, value, len(value))
    return p


class Letters:
    """gmg_letters: the sequence bytes of a batch in HBM, one per base, and the text of regions of them (gmg_regions_text)"""

    def __init__(self, letters, offsets):
        """letters: bytes, or a uint8 array (uploaded from where it lies: no copy of a batch of gigabytes)"""
        self.offsets = np.ascontiguousarray(offsets, np.uint64)
        self.h = C.c_void_p()
        if isinstance(letters, np.ndarray):
            letters = np.ascontiguousarray(letters, np.uint8)
            assert letters.size == int(self.offsets[-1])
            _ck(capi.lib().gmg_letters_upload(_ptr(letters), _ptr(self.offsets), len(self.offsets) - 1, C.byref(self.h)))
            return
        letters = bytes(letters)
        assert len(letters) == int(self.offsets[-1])
        _ck(capi.lib().gmg_letters_upload(letters, _ptr(self.offsets), len(self.offsets) - 1, C.byref(self.h)))

    @staticmethod
    def _args(regions, heads):
        """regions [(read, first, len, strand)] or a GeneRegion array; heads: a list of bytes, or (blob, offsets)"""
        n = len(regions)
        if isinstance(regions, np.ndarray):              # int [n, 4]: the bytes of a gmg_gene_region array
            regions = np.ascontiguousarray(regions.reshape(-1, 4), np.int32)
            regions = (capi.GeneRegion * max(n, 1)).from_buffer_copy(regions.tobytes() if n else bytes(C.sizeof(capi.GeneRegion)))
        if not isinstance(regions, C.Array):
            regions = (capi.GeneRegion * max(n, 1))(*[capi.GeneRegion(*[int(x) for x in r]) for r in regions])
        if isinstance(heads, tuple):
            blob, off = bytes(heads[0]), np.ascontiguousarray(heads[1], np.uint64)
        else:
            assert len(heads) == n
            blob = b"".join(heads)
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum([len(h) for h in heads], dtype=np.uint64)
        return regions, n, blob, off

    def _size(self, regions, n, blob, off, params):
        size = C.c_size_t(0)
        _ck(capi.lib().gmg_regions_text(self.h, regions, n, blob, _ptr(off), C.byref(params), None, C.byref(size), None))
        return size.value

    def text_size(self, regions, heads, params):
        """gmg_regions_text with host_out = NULL: the length of the text"""
        return self._size(*self._args(regions, heads), params)

    def regions_text(self, regions, heads, params, capacity=None, out=None, stream=None):
        """gmg_regions_text -> the text (bytes).  capacity: the size of the host buffer (default: what text_size says); out: a
        uint8 array to write into instead (its size is the capacity), then the length is returned"""
        regions, n, blob, off = self._args(regions, heads)
        if out is None:
            if capacity is None:
                capacity = self._size(regions, n, blob, off, params)
            buf = np.zeros(max(int(capacity), 1), np.uint8)
        else:
            buf, capacity = out, out.size
        size = C.c_size_t(int(capacity))
        _ck(capi.lib().gmg_regions_text(self.h, regions, n, blob, _ptr(off), C.byref(params), _ptr(buf), C.byref(size), stream))
        return size.value if out is not None else buf[:size.value].tobytes()

    def regions_text_device(self, regions, heads, params, stream=None):
        """gmg_regions_text_device -> (device pointer, bytes): the text stays in the handle's buffer until the next call"""
        regions, n, blob, off = self._args(regions, heads)
        ptr, size = C.c_void_p(), C.c_size_t(0)
        _ck(capi.lib().gmg_regions_text_device(self.h, regions, n, blob, _ptr(off), C.byref(params), C.byref(ptr), C.byref(size), stream))
        return ptr, size.value

    @staticmethod
    def _run_args(runs, string_run_off, heads, pad_front, pad_behind):
        """runs [(read, first, len, kind)] or a uint32 [n, 4] array; heads as for regions; pads: None (0) or one count per string"""
        runs = np.ascontiguousarray(np.asarray(runs, np.uint32).reshape(-1, 4))
        sro = np.ascontiguousarray(string_run_off, np.uint64)
        n = len(sro) - 1
        if isinstance(heads, tuple):
            blob, off = bytes(heads[0]), np.ascontiguousarray(heads[1], np.uint64)
        else:
            assert len(heads) == n
            blob = b"".join(heads)
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum([len(h) for h in heads], dtype=np.uint64)
        pads = [None if p is None else np.ascontiguousarray(p, np.uint32) for p in (pad_front, pad_behind)]
        assert all(p is None or len(p) == n for p in pads)
        keep = (runs, sro, off, pads)                   # (the arrays the pointers point into)
        return keep, (_ptr(runs) if len(runs) else None, len(runs), _ptr(sro), n, *[None if p is None or n == 0 else _ptr(p) for p in pads],
                      blob, _ptr(off))

    def runs_text_size(self, runs, string_run_off, heads, params, pad_front=None, pad_behind=None):
        """gmg_runs_text with host_out = NULL: the length of the text"""
        keep, args = self._run_args(runs, string_run_off, heads, pad_front, pad_behind)
        size = C.c_size_t(0)
        _ck(capi.lib().gmg_runs_text(self.h, *args, C.byref(params), None, C.byref(size), None))
        return size.value

    def runs_text(self, runs, string_run_off, heads, params, pad_front=None, pad_behind=None, capacity=None, out=None, stream=None):
        """gmg_runs_text -> the text (bytes): string k = pad_front[k] pad bytes, runs[string_run_off[k] : string_run_off[k + 1]],
        pad_behind[k] pad bytes, or its translation (runs_text_params).  capacity / out as for regions_text"""
        keep, args = self._run_args(runs, string_run_off, heads, pad_front, pad_behind)
        if out is None:
            if capacity is None:
                size = C.c_size_t(0)
                _ck(capi.lib().gmg_runs_text(self.h, *args, C.byref(params), None, C.byref(size), None))
                capacity = size.value
            buf = np.zeros(max(int(capacity), 1), np.uint8)
        else:
            buf, capacity = out, out.size
        size = C.c_size_t(int(capacity))
        _ck(capi.lib().gmg_runs_text(self.h, *args, C.byref(params), _ptr(buf), C.byref(size), stream))
        return size.value if out is not None else buf[:size.value].tobytes()

    def runs_text_device(self, runs, string_run_off, heads, params, pad_front=None, pad_behind=None, stream=None):
        """gmg_runs_text_device -> (device pointer, bytes): the text stays in the handle's buffer until the next text call"""
        keep, args = self._run_args(runs, string_run_off, heads, pad_front, pad_behind)
        ptr, size = C.c_void_p(), C.c_size_t(0)
        _ck(capi.lib().gmg_runs_text_device(self.h, *args, C.byref(params), C.byref(ptr), C.byref(size), stream))
        return ptr, size.value

    def kernel_ms(self):
        ms = C.c_float()
        _ck(capi.lib().gmg_letters_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            capi.lib().gmg_letters_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def memcpy_d2h(ptr, nbytes, stream=None):
    """nbytes of device memory at ptr as bytes (gmg_memcpy_d2h on `stream`, waited for)"""
    out = np.empty(max(int(nbytes), 1), np.uint8)
    if nbytes:
        _ck(capi.lib().gmg_memcpy_d2h(_ptr(out), ptr, int(nbytes), stream))
    return out[:int(nbytes)].tobytes()


def icm_train_reads(reads, model_len=12, model_depth=7, periodicity=3):
    return Icm.train_reads(reads, model_len, model_depth, periodicity)


class Trainer:
    """gmg_trainer: the pair counts of build-icm's training, one tree level per call (levels in order)."""

    def __init__(self, strings, model_len=12, model_depth=7, periodicity=3):
        self.strings = strings            # the Reads batch must outlive the trainer
        self.shape = (model_len, model_depth, periodicity)
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_trainer_create(strings.h, model_len, model_depth, periodicity, C.byref(self.h)))

    def level_counts(self, level, mip_prev=None):
        """-> int32 [periodicity, 4^level, max(model_len - 1, 1), 16]; mip_prev: int16 [periodicity, 4^(level-1)]"""
        w, _, p = self.shape
        out = np.zeros((p, 4 ** level, max(w - 1, 1), 16), np.int32)
        if mip_prev is not None:
            mip_prev = np.ascontiguousarray(mip_prev, np.int16)
        _ck(capi.lib().gmg_trainer_level_counts(self.h, level, _ptr(mip_prev) if mip_prev is not None else None,
                                                _ptr(out)))
        return out

    def close(self):
        if self.h:
            capi.lib().gmg_trainer_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Segments:
    """ORF-style scoring buffers (gmg_segments): rows of (read, lo, len, orient)."""

    def __init__(self, reads, rows):
        rows = np.ascontiguousarray(np.asarray(rows, np.uint32).reshape(-1, 4))
        self.n = rows.shape[0]
        self.rows = rows
        self.offsets = np.zeros(self.n + 1, np.uint64)
        total = C.c_uint64()
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_segments_upload(reads.h, _ptr(rows), self.n, _ptr(self.offsets), C.byref(total),
                                           C.byref(self.h)))
        self.total_len = int(total.value)

    def split(self, flat):
        return [flat[int(self.offsets[i]):int(self.offsets[i + 1])] for i in range(self.n)]

    def close(self):
        if self.h:
            capi.lib().gmg_segments_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def frame_score6(gene, null, reads, d_out=None, stream=None, row_stride=None, read_null=None):
    """Score_All_Frames (glimmer-mg.cc:1468-1510) for every read.  With d_out (a device pointer to
    6*row_stride doubles) the call is asynchronous on `stream` and returns None; otherwise the
    result comes back as a float64 array [6, total_bases].  row_stride (default total_bases) is the
    distance between the six rows in doubles (gmg_frame_score6_strided).
    null may be a NullSet with read_null[r] = the null model of read r (gmg_frame_score6_nulls)."""
    stride = reads.total_bases if row_stride is None else int(row_stride)

    def call(ptr):
        if isinstance(null, NullSet):
            rn = np.ascontiguousarray(read_null, np.uint32)
            assert len(rn) == reads.n_reads
            _ck(capi.lib().gmg_frame_score6_nulls(gene.device(), null.h, _ptr(rn), reads.h, ptr, stride, stream))
        else:
            _ck(capi.lib().gmg_frame_score6_strided(gene.device(), null.device(), reads.h, ptr, stride, stream))

    if d_out is not None:
        call(C.c_void_p(d_out))
        return None
    buf = _DeviceBuffer(6 * max(stride, 1) * 8)
    call(buf.ptr)
    _ck(capi.lib().gmg_synchronize(stream))
    out = buf.to_host(np.float64, 6 * stride, stream).reshape(6, stride)[:, :reads.total_bases].copy()
    buf.free()
    return out


def _seg_call(fn, model, reads, segs, frame, count, d_out=None, stream=None):
    """every per-segment call: on `stream`; with d_out (a device pointer to `count` doubles) asynchronous, returns None"""
    if d_out is not None:
        _ck(fn(model.device(), reads.h, segs.h, int(frame), C.c_void_p(d_out), stream))
        return None
    buf = _DeviceBuffer(max(count, 1) * 8)
    _ck(fn(model.device(), reads.h, segs.h, int(frame), buf.ptr, stream))
    out = buf.to_host(np.float64, count, stream)
    buf.free()
    return out


def segment_frame_score(model, reads, segs, frame, d_out=None, stream=None):
    """ICM_t::Frame_Score (icm.cc:485-509) per segment, flat float64[total_len]"""
    return _seg_call(capi.lib().gmg_segment_frame_score, model, reads, segs, frame, segs.total_len, d_out, stream)


def segment_cumscore(model, reads, segs, frame0, d_out=None, stream=None):
    """ICM_t::Cumulative_Score (icm.cc:354-405) per segment, flat float64[total_len]"""
    return _seg_call(capi.lib().gmg_segment_cumscore, model, reads, segs, frame0, segs.total_len, d_out, stream)


def score_string(model, reads, segs, frame0, d_out=None, stream=None):
    """ICM_t::Score_String (icm.cc:864-903) per segment, float64[n]"""
    return _seg_call(capi.lib().gmg_score_string, model, reads, segs, frame0, segs.n, d_out, stream)


def segment_partial_prob(model, reads, segs, frame, d_out=None, stream=None):
    """ICM_t::Partial_Window_Prob (icm.cc:807-842) of each segment's last base, float64[n]"""
    return _seg_call(capi.lib().gmg_segment_partial_prob, model, reads, segs, frame, segs.n, d_out, stream)


def all_frame_score(gene, reads, segs, prefix_len, frames, d_out=None, stream=None):
    """All_Frame_Score (glimmer3.cc:328-359) per segment -> float64[n, 6]; with d_out (a device pointer to 6 n doubles) the result
    stays there and None is returned (the two input arrays are uploaded and released behind the stream's work)"""
    pre = _DeviceBuffer.from_host(np.asarray(prefix_len, np.uint32), stream)
    frs = _DeviceBuffer.from_host(np.asarray(frames, np.int32), stream)
    buf = _DeviceBuffer(max(segs.n, 1) * 48) if d_out is None else None
    _ck(capi.lib().gmg_all_frame_score(gene.device(), reads.h, segs.h, pre.ptr, frs.ptr, buf.ptr if buf else C.c_void_p(d_out), stream))
    _ck(capi.lib().gmg_synchronize(stream))
    out = buf.to_host(np.float64, 6 * segs.n, stream).reshape(segs.n, 6) if buf else None
    for b in (pre, frs, buf):
        if b:
            b.free()
    return out


ORF_DTYPE = np.dtype([("read", "<u4"), ("frame", "<i4"), ("stop_position", "<i4"), ("orf_len", "<i4")])
START_DTYPE = np.dtype([("score", "<f8"), ("j", "<i4"), ("pos", "<i4"), ("which", "<i4"), ("truncated", "<i2"),
                        ("first", "<i2")])
ORF_RESULT_DTYPE = np.dtype([("gene_score", "<f8"), ("best_score", "<f8"), ("start_begin", "<u4"), ("n_starts", "<u4"),
                             ("first_j", "<i4"), ("best_j", "<i4"), ("best_pos", "<i4"), ("is_tentative_gene", "<i2"),
                             ("orf_is_truncated", "<i2")])


def score_orfs(gene, null, reads, orfs, min_gene_len=75, allow_truncated=False, use_first_start=False,
               ignore_score_len=2**31 - 1, start_threshold=-6.0, start_codons=("atg", "gtg", "ttg"), stream=None):
    """The scoring part of Score_Orfs (glimmer3.cc:1275-1552) for a batch of ORFs.
    orfs: rows (read, frame, stop_position, orf_len) as Find_Orfs produced them.
    -> (results[ORF_RESULT_DTYPE], starts[START_DTYPE]); ORF i's starts are
       starts[res.start_begin : res.start_begin + res.n_starts]."""
    rows = np.asarray(orfs)
    o = np.zeros(len(rows), ORF_DTYPE)
    if len(rows):
        o["read"], o["frame"], o["stop_position"], o["orf_len"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    assert ORF_DTYPE.itemsize == 16 and START_DTYPE.itemsize == 24 and ORF_RESULT_DTYPE.itemsize == 40
    prm = capi.OrfParams(min_gene_len, int(allow_truncated), int(use_first_start), ignore_score_len,
                         start_threshold, len(start_codons))
    for i, c in enumerate(start_codons):
        prm.start_codon[i].value = c.encode()
    batch, max_starts = C.c_void_p(), C.c_uint64()
    _ck(capi.lib().gmg_orfs_upload(reads.h, _ptr(o), len(o), C.byref(max_starts), C.byref(batch)))
    res = np.zeros(len(o), ORF_RESULT_DTYPE)
    try:
        n_st = C.c_uint64()
        _ck(capi.lib().gmg_score_orfs_begin(gene.device(), null.device(), reads.h, batch, C.byref(prm), C.byref(n_st), stream))
        starts = np.zeros(max(int(n_st.value), 1), START_DTYPE)
        _ck(capi.lib().gmg_score_orfs_fetch(batch, _ptr(res), _ptr(starts), stream))
    finally:
        capi.lib().gmg_orf_batch_free(batch)
    return res, starts


MG_ORF_DTYPE = np.dtype([("read", "<u4"), ("frame", "<i4"), ("stop_position", "<i4"), ("orf_len", "<i4"),
                         ("gene_len", "<i4"), ("lo", "<i4"), ("hi", "<i4"), ("first_j", "<i4"),
                         ("start_begin", "<u4"), ("n_starts", "<u4"), ("accepted", "<i2"),
                         ("orf_is_truncated", "<i2"), ("reserved", "<i4"), ("best_score", "<f8")])


def find_orfs(reads, min_gene_len=75, allow_truncated=False, start_codons=("atg", "gtg", "ttg"),
              stop_codons=("taa", "tag", "tga"), circular=False, ignore_regions=(), stream=None):
    """gmg_find_orfs: Find_Orfs for every read -> (orfs[MG_ORF_DTYPE], read_orf_off[uint64 n_reads+1]).
    circular: Genome_Is_Circular; ignore_regions: [(lo, hi)] as Get_Ignore_Regions leaves them (0-based lo, hi one past the end)"""
    prm = capi.MgParams(min_gene_len, int(allow_truncated), 2**31 - 1, len(start_codons), len(stop_codons), 0, 0.0)
    for i, c in enumerate(start_codons):
        prm.start_codon[i].value = c.encode()
    for i, c in enumerate(stop_codons):
        prm.stop_codon[i].value = c.encode()
    prm.circular = int(bool(circular))
    lo = np.ascontiguousarray([r[0] for r in ignore_regions], np.int32)
    hi = np.ascontiguousarray([r[1] for r in ignore_regions], np.int32)
    prm.n_ignore_regions = len(lo)
    if len(lo):
        prm.ignore_lo, prm.ignore_hi = lo.ctypes.data, hi.ctypes.data
    res = C.c_void_p()
    _ck(capi.lib().gmg_find_orfs(reads.h, C.byref(prm), C.byref(res), stream))
    try:
        n_orfs, n_starts = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_mg_result_info(res, C.byref(n_orfs), C.byref(n_starts)))
        orfs = np.zeros(max(n_orfs.value, 1), MG_ORF_DTYPE)
        off = np.zeros(reads.n_reads + 1, np.uint64)
        _ck(capi.lib().gmg_mg_result_fetch_on(res, _ptr(orfs), None, _ptr(off), stream))
    finally:
        capi.lib().gmg_mg_result_free(res)
    return orfs[:n_orfs.value], off


class OrfResult:
    """A gmg_find_orfs result that stays on the device (gmg_mg_result): what gmg_entropy_orfs reads.  fetch() -> (orfs, read_orf_off)"""

    def __init__(self, reads, min_gene_len=75, allow_truncated=False, start_codons=("atg", "gtg", "ttg"),
                 stop_codons=("taa", "tag", "tga"), circular=False, stream=None):
        prm = capi.MgParams(min_gene_len, int(allow_truncated), 2**31 - 1, len(start_codons), len(stop_codons), 0, 0.0)
        for i, c in enumerate(start_codons):
            prm.start_codon[i].value = c.encode()
        for i, c in enumerate(stop_codons):
            prm.stop_codon[i].value = c.encode()
        prm.circular = int(bool(circular))
        self.h = C.c_void_p()
        self.n_reads = reads.n_reads
        self.stream = stream
        _ck(capi.lib().gmg_find_orfs(reads.h, C.byref(prm), C.byref(self.h), stream))
        n_orfs, n_starts = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_mg_result_info(self.h, C.byref(n_orfs), C.byref(n_starts)))
        self.n_orfs = int(n_orfs.value)

    def fetch(self):
        orfs = np.zeros(max(self.n_orfs, 1), MG_ORF_DTYPE)
        off = np.zeros(self.n_reads + 1, np.uint64)
        _ck(capi.lib().gmg_mg_result_fetch_on(self.h, _ptr(orfs), None, _ptr(off), self.stream))
        return orfs[:self.n_orfs], off

    def close(self):
        if self.h:
            capi.lib().gmg_mg_result_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def xlate_table(code):
    """gmg_xlate_table: Codon_Translation (gene.cc:1016-1080) of the 64 codons (index 16*b0 + 4*b1 + b2, a=0 c=1 g=2 t=3) -> bytes"""
    buf = C.create_string_buffer(64)
    _ck(capi.lib().gmg_xlate_table(int(code), buf))
    return buf.raw


def entropy_default_profiles():
    """gmg_entropy_default_profiles -> (pos[20], neg[20])"""
    pos, neg = np.zeros(20), np.zeros(20)
    _ck(capi.lib().gmg_entropy_default_profiles(_ptr(pos), _ptr(neg)))
    return pos, neg


def entropy_from_counts(counts, pos, neg):
    """gmg_entropy_from_counts: the host finish of count vectors [n, 20] (or [20]) -> float64 [n, 3] (or [3]): pos_dist, neg_dist, ratio"""
    counts = np.ascontiguousarray(counts, np.int32)
    pos, neg = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(neg, np.float64)
    rows = counts.reshape(-1, 20)
    out = np.zeros((len(rows), 3))
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    for k, row in enumerate(rows):
        _ck(capi.lib().gmg_entropy_from_counts(_ptr(row), _ptr(pos), _ptr(neg), C.byref(a), C.byref(b), C.byref(c)))
        out[k] = a.value, b.value, c.value
    return out.reshape(counts.shape[:-1] + (3,))


def _entropy_call(n, want_counts, want_dist, call, stream=None):
    """runs call(d_counts, d_dist) with device buffers for n rows -> (counts int32 [n, 20] or None, dist float64 [n, 3] or None)"""
    cbuf = _DeviceBuffer(max(n, 1) * 80) if want_counts else None
    dbuf = _DeviceBuffer(max(n, 1) * 24) if want_dist else None
    try:
        _ck(call(cbuf.ptr if cbuf else None, dbuf.ptr if dbuf else None))
        counts = cbuf.to_host(np.int32, n * 20, stream).reshape(n, 20) if cbuf else None
        dist = dbuf.to_host(np.float64, n * 3, stream).reshape(n, 3) if dbuf else None
    finally:
        for b in (cbuf, dbuf):
            if b:
                b.free()
    return counts, dist


def entropy_regions(reads, regions, aa, pos, neg, want_counts=True, want_dist=True, stream=None, d_counts=None, d_dist=None):
    """gmg_entropy_regions: regions = [(read, first, len, strand)] -> (counts [n, 20] or None, dist [n, 3] or None); with d_counts or
    d_dist (device pointers) the call is asynchronous on `stream`, the rows stay there and None is returned"""
    arr = (capi.GeneRegion * max(len(regions), 1))(*[capi.GeneRegion(int(r), int(f), int(ln), int(s)) for r, f, ln, s in regions])
    aa = bytes(aa)
    pos, neg = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(neg, np.float64)
    if d_counts is not None or d_dist is not None:
        _ck(capi.lib().gmg_entropy_regions(reads.h, arr, len(regions), aa, _ptr(pos), _ptr(neg), d_counts, d_dist, stream))
        return None
    return _entropy_call(len(regions), want_counts, want_dist, lambda c, d: capi.lib().gmg_entropy_regions(
        reads.h, arr, len(regions), aa, _ptr(pos), _ptr(neg), c, d, stream), stream)


def entropy_orfs(reads, orf_result, aa, pos, neg, want_counts=True, want_dist=True, stream=None, d_counts=None, d_dist=None):
    """gmg_entropy_orfs on an OrfResult -> (counts [n_orfs, 20] or None, dist [n_orfs, 3] or None); d_counts / d_dist as for
    entropy_regions"""
    aa = bytes(aa)
    pos, neg = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(neg, np.float64)
    if d_counts is not None or d_dist is not None:
        _ck(capi.lib().gmg_entropy_orfs(reads.h, orf_result.h, aa, _ptr(pos), _ptr(neg), d_counts, d_dist, stream))
        return None
    return _entropy_call(orf_result.n_orfs, want_counts, want_dist, lambda c, d: capi.lib().gmg_entropy_orfs(
        reads.h, orf_result.h, aa, _ptr(pos), _ptr(neg), c, d, stream), stream)


AUDIT_NEXT_STOP = 1                                     # GMG_AUDIT_NEXT_STOP
GENE_AUDIT_DTYPE = np.dtype([("first_codon", "<i4"), ("last_codon", "<i4"), ("start_which", "<i4"), ("stop_which", "<i4"),
                             ("n_inner_stops", "<i4"), ("inner_begin", "<u4"), ("last_back_stop", "<i4"), ("next_stop", "<i4")])


def audit_params(start_codons=("atg", "gtg", "ttg"), stop_codons=DEFAULT_STOPS, flags=AUDIT_NEXT_STOP):
    """a gmg_audit_params; the codons go in as they are given (the library refuses all but lower-case acgt triplets)"""
    prm = capi.AuditParams()
    prm.n_start_codons, prm.n_stop_codons, prm.flags = len(start_codons), len(stop_codons), int(flags)
    for dst, lst in ((prm.start_codon, start_codons), (prm.stop_codon, stop_codons)):
        for i, c in enumerate(lst[:8]):
            dst[i].value = (c.encode() if isinstance(c, str) else bytes(c))[:4]
    return prm


def _region_array(regions):
    """regions as the bytes of a gmg_gene_region array: an int array [n, 4] as it is, a list of (read, first, len, strand) rows"""
    arr = np.ascontiguousarray(np.asarray(regions, np.int64).reshape(-1, 4).astype(np.int32))
    return arr, len(arr)


def genes_audit(reads, regions, start_codons=("atg", "gtg", "ttg"), stop_codons=DEFAULT_STOPS, flags=AUDIT_NEXT_STOP, amb=None,
                stream=None, fetch=True):
    """gmg_genes_audit: regions = [(read, first, len, strand)] (or an int array [n, 4]); amb = ascending job-wide indices of the
    bases whose letter is outside acgtACGT.  -> (records GENE_AUDIT_DTYPE [n], inner int32 [n_inner], hist int64 [65]); fetch=False:
    only (n_regions, n_inner), nothing copied back"""
    arr, n = _region_array(regions)
    n_amb = 0 if amb is None else len(amb)
    ab = np.ascontiguousarray(amb, np.uint64) if n_amb else None
    prm = audit_params(start_codons, stop_codons, flags)
    h = C.c_void_p()
    _ck(capi.lib().gmg_genes_audit(reads.h, _ptr(arr) if n else None, n, C.byref(prm), _ptr(ab) if n_amb else None, n_amb, C.byref(h), stream))
    try:
        nr, ni = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_audit_info(h, C.byref(nr), C.byref(ni)))
        if not fetch:
            _ck(capi.lib().gmg_synchronize(stream))
            return nr.value, ni.value
        rec, inner, hist = np.zeros(max(nr.value, 1), GENE_AUDIT_DTYPE), np.zeros(max(ni.value, 1), np.int32), np.zeros(65, np.int64)
        _ck(capi.lib().gmg_audit_fetch(h, _ptr(rec), _ptr(inner), _ptr(hist)))
    finally:
        capi.lib().gmg_audit_free(h)
    return rec[:nr.value], inner[:ni.value], hist


def window_counts(reads, window_len, window_skip, amb=None, stream=None, fetch=True, device=False):
    """gmg_window_counts: the {a, c, g, t, other} counts of every window of every read; amb = ascending job-wide indices of the bases
    whose letter is outside acgtACGT.  -> (read_window_off uint64 [n_reads + 1], counts int32 [n_windows, 5]); fetch=False: only
    (n_reads, n_windows), nothing copied back; device=True: the rows are also read back through the pointers of gmg_windows_device
    and returned as a third and fourth value"""
    n_amb = 0 if amb is None else len(amb)
    ab = np.ascontiguousarray(amb, np.uint64) if n_amb else None
    h = C.c_void_p()
    _ck(capi.lib().gmg_window_counts(reads.h, int(window_len), int(window_skip), _ptr(ab) if n_amb else None, n_amb, C.byref(h), stream))
    try:
        nr, nw = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_windows_info(h, C.byref(nr), C.byref(nw)))
        if not fetch:
            _ck(capi.lib().gmg_synchronize(stream))
            return nr.value, nw.value
        off, counts = np.zeros(nr.value + 1, np.uint64), np.zeros((max(nw.value, 1), 5), np.int32)
        _ck(capi.lib().gmg_windows_fetch(h, _ptr(off), _ptr(counts)))
        if device:
            d_off, d_counts = C.c_void_p(), C.c_void_p()
            _ck(capi.lib().gmg_windows_device(h, C.byref(d_off), C.byref(d_counts)))
            off2, counts2 = np.zeros(nr.value + 1, np.uint64), np.zeros((max(nw.value, 1), 5), np.int32)
            _ck(capi.lib().gmg_memcpy_d2h(_ptr(off2), d_off, off2.nbytes, stream))
            if nw.value:
                _ck(capi.lib().gmg_memcpy_d2h(_ptr(counts2), d_counts, nw.value * 20, stream))
            _ck(capi.lib().gmg_synchronize(stream))
            return off, counts[:nw.value], off2, counts2[:nw.value]
    finally:
        capi.lib().gmg_windows_free(h)
    return off, counts[:nw.value]


def regions_uncovered(reads, intervals, min_len=0, stream=None, fetch=True):
    """gmg_regions_uncovered: intervals = [(read, lo, hi)], 0-based half open, any order -> (gaps int32 [n_gaps, 4] = rows (read, first,
    len, +1), ready for Reads.extract / entropy_regions / genes_audit; read_gap_off uint64 [n_reads + 1]); fetch=False: only n_gaps"""
    arr = np.ascontiguousarray(np.asarray(intervals, np.int64).reshape(-1, 3).astype(np.uint32).view(np.int32))
    n = len(arr)
    h = C.c_void_p()
    _ck(capi.lib().gmg_regions_uncovered(reads.h, _ptr(arr) if n else None, n, int(min_len), C.byref(h), stream))
    try:
        ng = C.c_uint64()
        _ck(capi.lib().gmg_gaps_info(h, C.byref(ng)))
        if not fetch:
            _ck(capi.lib().gmg_synchronize(stream))
            return ng.value
        gaps, off = np.zeros((max(ng.value, 1), 4), np.int32), np.zeros(reads.n_reads + 1, np.uint64)
        _ck(capi.lib().gmg_gaps_fetch(h, _ptr(gaps), _ptr(off)))
    finally:
        capi.lib().gmg_gaps_free(h)
    return gaps[:ng.value], off


def uncovered_plan(offsets, coords, flags=0):
    """gmg_uncovered_plan (host): coordinate lines (read, start, end[, dir]), 1-based inclusive, -> [(read, lo, hi)] by uncovered's
    arithmetic (a line that runs over the sequence's end gives two)"""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    arr = (capi.Coord * max(len(coords), 1))(*[capi.Coord(int(c[0]), int(c[3]) if len(c) > 3 else 0, int(c[1]), int(c[2])) for c in coords])
    out = np.zeros((max(2 * len(coords), 1), 3), np.int32)
    n = C.c_uint64()
    _ck(capi.lib().gmg_uncovered_plan(_ptr(offsets), len(offsets) - 1, arr, len(coords), int(flags), _ptr(out), C.byref(n)))
    return [(int(r), int(a), int(b)) for r, a, b in out[:n.value]]


START_ERRORS_DTYPE = np.dtype([("pos", "<i4", (2,)), ("type", "i1", (2,)), ("n", "i1"), ("reserved", "i1")])
MG_ACCEPTED_ONLY, MG_ALLOW_INDELS, MG_ALLOW_SUBS = 1, 2, 4


class Classes:
    """gmg_classes: glimmer-mg -c bookkeeping (Parse_Classes, Read_Meta_ICMs / _GC / _Stops; host only)"""

    def __init__(self, class_text, icm_dir):
        if isinstance(class_text, str):
            class_text = class_text.encode()
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_classes_load(class_text, len(class_text), icm_dir.encode(), C.byref(self.h)))
        n, k, c, miss = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        _ck(capi.lib().gmg_classes_info(self.h, C.byref(n), C.byref(k), C.byref(c), C.byref(miss)))
        self.n_reads, self.n_icms, self.n_classes, self.n_missing_gc = n.value, k.value, c.value, miss.value

    def icm_file(self, k):
        p = capi.lib().gmg_classes_icm_file(self.h, k)
        if p is None:
            _ck(-1)
        return p.decode()

    def plan(self, headers):
        """headers: the header LINES of one chunk -> (order, icm_begin, gc, transl): gmg_classes_plan"""
        hb = [h.encode() if isinstance(h, str) else h for h in headers]
        n = len(hb)
        arr = (C.c_char_p * max(n, 1))(*hb)
        lens = np.array([len(h) for h in hb], np.uint32)
        order = np.zeros(max(n, 1), np.uint64)
        icm_begin = np.zeros(self.n_icms + 1, np.uint64)
        gc = np.zeros(max(n, 1), np.float64)
        transl = np.zeros(max(n, 1), np.int32)
        k = C.c_uint64()
        _ck(capi.lib().gmg_classes_plan(self.h, arr, _ptr(lens), n, _ptr(order), _ptr(icm_begin), _ptr(gc), _ptr(transl), C.byref(k)))
        return order[:k.value], icm_begin, gc[:k.value], transl[:k.value]

    def close(self):
        if self.h:
            capi.lib().gmg_classes_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stop_codons_by_code(code):
    """gmg_stop_codons_by_code: Set_Stop_Codons_By_Code (gene.cc:1560-1624) -> tuple of codons"""
    buf = ((C.c_char * 4) * 8)()
    n = C.c_int()
    _ck(capi.lib().gmg_stop_codons_by_code(int(code), buf, C.byref(n)))
    return tuple(buf[i].value.decode() for i in range(n.value))


def ignore_score_len(gc, stops=DEFAULT_STOPS):
    """gmg_ignore_score_len: Set_Ignore_Score_Len (glimmer_base.cc:2597-2633)"""
    buf = ((C.c_char * 4) * 8)()
    for i, c in enumerate(stops):
        buf[i].value = c.encode()
    out = C.c_int32()
    _ck(capi.lib().gmg_ignore_score_len(float(gc), buf, len(stops), C.byref(out)))
    return out.value


def mg_score_reads(gene, null, reads, min_gene_len=75, allow_truncated=True, ignore_score_len=2**31 - 1,
                   start_threshold=-6.0, start_codons=("atg", "gtg", "ttg"), stop_codons=("taa", "tag", "tga"),
                   frame_scores=None, accepted_only=False, allow_indels=False, allow_subs=False, quality=None,
                   min_indel_orf_len=15, indel_quality_threshold=18, indel_max=2, indel_suffix_score_threshold=-12.0,
                   read_null=None, read_ignore_score_len=None, groups=None, stream=None):
    """glimmer-mg's front half for a batch of reads (include/gmg.h: gmg_mg_score_reads): Score_All_Frames,
    Find_Orfs, Score_Orf_Starts and the filter of Score_Orfs_Errors.
    -> (orfs[MG_ORF_DTYPE], starts[START_DTYPE], read_orf_off[uint64 n_reads+1]).
    frame_scores: optional _DeviceBuffer of 6*total_bases doubles that receives the Frame_Scores table.
    allow_indels / allow_subs: glimmer-mg's error branch (-i / -s); the starts' Error_t lists come back as a fourth
    array (START_ERRORS_DTYPE, parallel to starts).  quality: uint8 Phred values of all bases (the -q file), or None
    for Set_Quality_454."""
    assert MG_ORF_DTYPE.itemsize == 56 and START_ERRORS_DTYPE.itemsize == 12
    err = bool(allow_indels or allow_subs)
    flags = (MG_ACCEPTED_ONLY if accepted_only else 0) | (MG_ALLOW_INDELS if allow_indels else 0) | (MG_ALLOW_SUBS if allow_subs else 0)
    prm = capi.MgParams(min_gene_len, int(allow_truncated), ignore_score_len, len(start_codons), len(stop_codons),
                        flags, start_threshold)
    prm.min_indel_orf_len, prm.indel_quality_threshold, prm.indel_max = min_indel_orf_len, indel_quality_threshold, indel_max
    prm.indel_suffix_score_threshold = indel_suffix_score_threshold
    if quality is not None:
        quality = np.ascontiguousarray(quality, np.uint8)
        if quality.size != reads.total_bases:
            raise ValueError("quality needs one value per base of the batch")
        prm.quality = quality.ctypes.data
    for i, c in enumerate(start_codons):
        prm.start_codon[i].value = c.encode()
    for i, c in enumerate(stop_codons):
        prm.stop_codon[i].value = c.encode()
    null_model = null
    if isinstance(null, NullSet):                       # classification mode: null model (and Ignore_Score_Len) per read
        read_null = np.ascontiguousarray(read_null, np.uint32)
        assert len(read_null) == reads.n_reads
        prm.nulls, prm.read_null = null.h, read_null.ctypes.data
        if read_ignore_score_len is not None:
            read_ignore_score_len = np.ascontiguousarray(read_ignore_score_len, np.int32)
            assert len(read_ignore_score_len) == reads.n_reads
            prm.read_ignore_score_len = read_ignore_score_len.ctypes.data
        null_model = null.icms[0]
    res = C.c_void_p()
    if groups is not None:                              # gmg_mg_score_groups: [(Icm, read_begin, read_end), ...], `gene` is not used
        arr = (capi.MgGroup * max(len(groups), 1))(*[capi.MgGroup(m.device(), int(b), int(e)) for m, b, e in groups])
        _ck(capi.lib().gmg_mg_score_groups(arr, len(groups), null_model.device(), reads.h, C.byref(prm), C.byref(res), stream))
    else:
        _ck(capi.lib().gmg_mg_score_reads(gene.device(), null_model.device(), reads.h, C.byref(prm),
                                          frame_scores.ptr if frame_scores is not None else None, C.byref(res), stream))
    try:
        n_orfs, n_starts = C.c_uint64(), C.c_uint64()
        _ck(capi.lib().gmg_mg_result_info(res, C.byref(n_orfs), C.byref(n_starts)))
        orfs = np.zeros(max(n_orfs.value, 1), MG_ORF_DTYPE)
        starts = np.zeros(max(n_starts.value, 1), START_DTYPE)
        off = np.zeros(reads.n_reads + 1, np.uint64)
        _ck(capi.lib().gmg_mg_result_fetch_on(res, _ptr(orfs), _ptr(starts), _ptr(off), stream))
        if err:
            errs = np.zeros(max(n_starts.value, 1), START_ERRORS_DTYPE)
            _ck(capi.lib().gmg_mg_result_fetch_errors(res, _ptr(errs)))
    finally:
        capi.lib().gmg_mg_result_free(res)
    if err:
        return orfs[:n_orfs.value], starts[:n_starts.value], off, errs[:n_starts.value]
    return orfs[:n_orfs.value], starts[:n_starts.value], off


def score_reads_strings(models, reads, d_out=None, stream=None):
    """gmg_score_reads_strings on `stream`: whole-read Score_String (frame 0) of every read and of its reverse complement under
    every model -> float64 [n_models, n_reads, 2]; with d_out (a device pointer to that many doubles) the sums stay there"""
    n = len(models)
    arr = (C.c_void_p * max(n, 1))(*[m.device() for m in models])
    if d_out is not None:
        _ck(capi.lib().gmg_score_reads_strings(arr, n, reads.h, C.c_void_p(d_out), stream))
        return None
    buf = _DeviceBuffer(max(n * reads.n_reads * 2, 1) * 8)
    _ck(capi.lib().gmg_score_reads_strings(arr, n, reads.h, buf.ptr, stream))
    out = buf.to_host(np.float64, n * reads.n_reads * 2, stream).reshape(n, reads.n_reads, 2)
    buf.free()
    return out


class TopHits:
    """gmg_tophits: the best `top_hits` models of every read of `reads`, kept in HBM while a database of ICMs streams through in
    batches (Phymm's raw matrix + glimmer-mg.py's parse_phymm / score_insert; include/gmg.h).  Keys are the %.4f text of a score as
    an integer count of 1e-4 units."""

    def __init__(self, reads, top_hits):
        self.reads = reads                              # (the handle scores this batch: it must outlive the handle)
        self.top_hits = int(top_hits)
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_tophits_create(reads.h, self.top_hits, C.byref(self.h)))

    @staticmethod
    def _inf(informative, B):
        if informative is None:
            return None, None
        inf = np.ascontiguousarray(informative, np.uint8)
        assert len(inf) == B
        return inf, _ptr(inf)

    def update_sums(self, sums, first_model=0, informative=None, forward_only=False, stream=None):
        """gmg_tophits_update_sums on HOST sums float64 [B, n_reads, 2] (uploaded first, on the same stream)"""
        sums = np.ascontiguousarray(sums, np.float64)
        B = sums.shape[0]
        buf = _DeviceBuffer.from_host(sums, stream)
        inf, p = self._inf(informative, B)
        try:
            _ck(capi.lib().gmg_tophits_update_sums(self.h, buf.ptr, B, int(first_model), p, int(bool(forward_only)), stream))
        finally:
            buf.free()

    def scores(self, models, first_model=0, informative=None, forward_only=False, return_sums=False, stream=None):
        """gmg_tophits_scores: the models scored on the device into the handle's scratch, then the update; return_sums: the
        scratch copied back, float64 [B, n_reads, 2]"""
        B = len(models)
        arr = (C.c_void_p * max(B, 1))(*[m.device() for m in models])
        inf, p = self._inf(informative, B)
        d = C.c_void_p()
        _ck(capi.lib().gmg_tophits_scores(self.h, arr, B, int(first_model), p, int(bool(forward_only)), stream, C.byref(d)))
        if return_sums:
            out = np.empty(B * self.reads.n_reads * 2, np.float64)
            if out.nbytes:
                _ck(capi.lib().gmg_memcpy_d2h(_ptr(out), d, out.nbytes, stream))
            return out.reshape(B, self.reads.n_reads, 2)

    def fetch(self):
        """-> (keys int64 [n_reads, top_hits], models int32 [n_reads, top_hits]); an empty slot has model -1"""
        n = self.reads.n_reads
        keys = np.zeros((max(n, 1), self.top_hits), np.int64)
        models = np.zeros((max(n, 1), self.top_hits), np.int32)
        _ck(capi.lib().gmg_tophits_fetch(self.h, _ptr(keys), _ptr(models)))
        return keys[:n], models[:n]

    def format_rows(self, sums, forward_only=False, stream=None):
        """gmg_tophits_format_rows on HOST sums float64 [B, n_reads, 2] -> the B data-matrix lines (bytes)"""
        sums = np.ascontiguousarray(sums, np.float64)
        B = sums.shape[0]
        buf = _DeviceBuffer.from_host(sums, stream)
        cap = max(B * self.reads.n_reads * capi.TOPHITS_MAX_FIELD, B, 1)
        out = np.empty(cap, np.uint8)
        size = C.c_size_t(cap)
        try:
            _ck(capi.lib().gmg_tophits_format_rows(self.h, buf.ptr, B, int(bool(forward_only)), _ptr(out), C.byref(size), stream))
        finally:
            buf.free()
        return out[:size.value].tobytes()

    def close(self):
        if self.h:
            capi.lib().gmg_tophits_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def window_distrib(model, windows, frames, stream=None):
    """Full_Window_Distrib / Full_Window_Prob (icm.cc:512-610) on `stream`.  windows: uint8 codes [n, model_len]
    -> (dist float32 [n,4], prob float64 [n])"""
    windows = np.ascontiguousarray(windows, np.uint8)
    n = windows.shape[0]
    dw = _DeviceBuffer.from_host(windows, stream)
    df = _DeviceBuffer.from_host(np.asarray(frames, np.int32), stream)
    dd = _DeviceBuffer(max(n, 1) * 16)
    dp = _DeviceBuffer(max(n, 1) * 8)
    _ck(capi.lib().gmg_window_distrib(model.device(), dw.ptr, df.ptr, n, dd.ptr, dp.ptr, stream))
    dist = dd.to_host(np.float32, 4 * n, stream).reshape(n, 4)
    prob = dp.to_host(np.float64, n, stream)
    for b in (dw, df, dd, dp):
        b.free()
    return dist, prob


class FixedIcm:
    """Fixed_Length_ICM_t (src/ICM/icm.hh:216-255) behind gmg_fixed_icm: a model read from a .fix file, or trained here as
    build-fixed trains it (Fixed_Length_ICM_Training_t, the counting on the device)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def open(cls, path):
        h = C.c_void_p()
        _ck(capi.lib().gmg_fixed_icm_read(str(path).encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def train(cls, strings, max_depth=7, special=-1, perm=None):
        """build-fixed: strings of one length L (str / bytes, as read: case and ambiguity codes are Subscript's business),
        depth max_depth, special position, permutation (None: none).  The caller's strings are not permuted."""
        raw = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in strings]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        p = None if perm is None else (C.c_int * len(perm))(*[int(x) for x in perm])
        h = C.c_void_p()
        _ck(capi.lib().gmg_fixed_icm_train(arr, len(raw), int(max_depth), int(special), p, C.byref(h)))
        return cls(h)

    def write(self, path, binary=True):
        """Fixed_Length_ICM_Training_t::Output (binary, or the -t text); only for a model trained here"""
        _ck(capi.lib().gmg_fixed_icm_write(self.h, str(path).encode(), 1 if binary else 0))

    @property
    def params(self):
        """(length, max_depth, special_position, model_type, permutation list)"""
        L, d, s, t = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        perm = (C.c_int * 32)()
        _ck(capi.lib().gmg_fixed_icm_params(self.h, C.byref(L), C.byref(d), C.byref(s), C.byref(t), perm))
        return L.value, d.value, s.value, t.value, list(perm[:L.value])

    def score(self, strings, lo=0, hi=None):
        """Fixed_Length_ICM_t::Score_Windows: subrange_score (s, lo, hi) of every string, ONE device call -> float64[n]"""
        if hi is None:
            hi = self.params[0]
        raw = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in strings]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        out = np.empty(len(raw), np.float64)
        _ck(capi.lib().gmg_fixed_icm_score(self.h, arr, len(raw), int(lo), int(hi), _ptr(out)))
        return out

    def device(self):
        """gmg_fixed_model handle (uploaded once, owned by this FixedIcm)"""
        out = C.c_void_p()
        _ck(capi.lib().gmg_fixed_icm_device_model(self.h, C.byref(out)))
        return out

    def close(self):
        if self.h:
            capi.lib().gmg_fixed_icm_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FixedModel:
    """A gmg_fixed_model uploaded from tables: perm[L], and per sub-model i (mip int16 [N_i], prob float32 [N_i, 4], depth)."""

    def __init__(self, perm, subs):
        L = len(perm)
        self._keep = [(np.ascontiguousarray(m, np.int16), np.ascontiguousarray(p, np.float32)) for m, p, _ in subs]
        perm_a = np.ascontiguousarray(perm, np.int32)
        mips = (C.c_void_p * max(L, 1))(*[m.ctypes.data for m, _ in self._keep])
        probs = (C.c_void_p * max(L, 1))(*[p.ctypes.data for _, p in self._keep])
        depth = np.array([d for _, _, d in subs], np.int32)
        nodes = np.array([len(m) for m, _ in self._keep], np.int32)
        self.h = C.c_void_p()
        _ck(capi.lib().gmg_fixed_model_upload(L, _ptr(perm_a), mips, probs, _ptr(depth), _ptr(nodes), C.byref(self.h)))

    def info(self):
        L, d, b = C.c_int(), C.c_int(), C.c_uint64()
        _ck(capi.lib().gmg_fixed_model_info(self.h, C.byref(L), C.byref(d), C.byref(b)))
        return L.value, d.value, b.value

    def device(self):
        return self.h

    def close(self):
        if self.h:
            capi.lib().gmg_fixed_model_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fixed_score(model, reads, segs, lo=0, hi=None, d_out=None, stream=None):
    """gmg_fixed_score: subrange_score (lo, hi) of the window at the start of every segment's buffer -> float64[n].
    model: a FixedIcm or FixedModel.  With d_out (device pointer of n doubles) the call is asynchronous and returns None."""
    h = model.device()
    if hi is None:
        L = C.c_int()
        _ck(capi.lib().gmg_fixed_model_info(h, C.byref(L), None, None))
        hi = L.value
    if d_out is not None:
        _ck(capi.lib().gmg_fixed_score(h, reads.h, segs.h, int(lo), int(hi), C.c_void_p(d_out), stream))
        return None
    buf = _DeviceBuffer(max(segs.n, 1) * 8)
    _ck(capi.lib().gmg_fixed_score(h, reads.h, segs.h, int(lo), int(hi), buf.ptr, stream))
    out = buf.to_host(np.float64, segs.n, stream)
    buf.free()
    return out
