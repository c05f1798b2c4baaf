"""network-aware-bwa_amd -- MI355X-native per-read alignment hot path of mpieva/network-aware-bwa.

This package is only the thin Python face (ctypes) of ``libnabwa.so`` -- the C-ABI library declared
in ``include/nabwa.h`` whose HIP kernels do the work.  It mirrors the reference's own operator
interface for the path (``bwa_cal_sa_reg_gap``, ``bwt_sa``; reference bwtaln.h:187, bwt.h:100) in
flat-array form.  There is no CPU fallback: if the library or a GPU is missing, calls raise.

The directory name contains a hyphen; import it with
``importlib.import_module("network-aware-bwa_amd")``.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NABWA_LIB", os.path.join(_HERE, "libnabwa.so"))   # NABWA_LIB: A/B builds

OK, ENODEV, EINVAL, EIO, ENOMEM, ECAP, EHITS, EDATA = 0, -1, -2, -3, -4, -5, -6, -7

ALN_DT = np.dtype([("info", "<u4"), ("k", "<u4"), ("l", "<u4"), ("score", "<i4")])  # bwt_aln1_t, bwtaln.h:41-45


class GapOpt(C.Structure):
    """gap_opt_t (reference bwtaln.h:143-153), 64 bytes."""
    _fields_ = [("s_mm", C.c_int), ("s_gapo", C.c_int), ("s_gape", C.c_int), ("mode", C.c_int),
                ("indel_end_skip", C.c_int), ("max_del_occ", C.c_int), ("max_entries", C.c_int),
                ("fnr", C.c_float), ("max_diff", C.c_int), ("max_gapo", C.c_int), ("max_gape", C.c_int),
                ("max_seed_diff", C.c_int), ("seed_len", C.c_int), ("n_threads", C.c_int),
                ("max_top2", C.c_int), ("trim_qual", C.c_int)]


MAX_CIGAR, MAX_MD, MAX_MULTI = 64, 512, 16


class BatchConfig(C.Structure):
    """nabwa_batch_config_t (include/nabwa.h): what the batch-wide switches of one batch's search came to."""
    _fields_ = [("n", C.c_int32), ("min_len", C.c_int32), ("max_len", C.c_int32), ("deep_only", C.c_int32),
                ("ns1", C.c_int32), ("ns_wide", C.c_int32), ("w_sync", C.c_int32), ("trip_budget", C.c_int32),
                ("trip_budget_hard", C.c_int32), ("n_sync", C.c_int32), ("hard_budget", C.c_int32), ("cls", C.c_int32 * 3),
                ("coop_lanes", C.c_int32), ("lds_rd", C.c_int32)]


class SeMulti(C.Structure):
    """nabwa_multi_t"""
    _fields_ = [("pos", C.c_uint32), ("gap", C.c_int32), ("mm", C.c_int32), ("strand", C.c_int32),
                ("n_cigar", C.c_int32), ("cigar", C.c_uint16 * MAX_CIGAR)]


class SeRec(C.Structure):
    """nabwa_se_t: a finished single-end alignment"""
    _fields_ = [("type", C.c_int32), ("strand", C.c_int32), ("n_mm", C.c_int32), ("n_gapo", C.c_int32),
                ("n_gape", C.c_int32), ("score", C.c_int32), ("sa", C.c_uint32), ("pos", C.c_uint32),
                ("c1", C.c_uint32), ("c2", C.c_uint32), ("mapQ", C.c_int32), ("seQ", C.c_int32),
                ("len", C.c_int32), ("full_len", C.c_int32), ("clip_len", C.c_int32),
                ("n_cigar", C.c_int32), ("cigar", C.c_uint16 * MAX_CIGAR), ("nm", C.c_int32), ("md", C.c_char * MAX_MD),
                ("n_multi", C.c_int32), ("multi", SeMulti * MAX_MULTI),
                ("flag", C.c_int32), ("seqid", C.c_int32), ("nn", C.c_int32), ("rpos", C.c_int64), ("xt", C.c_char)]


class IsizeInfo(C.Structure):
    """nabwa_isize_t = isize_info_t without the histogram pointer (reference bwape.h:16-20)"""
    _fields_ = [("avg", C.c_double), ("std", C.c_double), ("ap_prior", C.c_double), ("low", C.c_uint32),
                ("high", C.c_uint32), ("high_bayesian", C.c_uint32)]


class PeEnd(C.Structure):
    """nabwa_pe_end_t: the bwa_seq_t fields pairing() touches"""
    _fields_ = [("pos", C.c_uint32), ("strand", C.c_int32), ("mapQ", C.c_int32), ("seQ", C.c_int32), ("len", C.c_int32),
                ("full_len", C.c_int32), ("n_mm", C.c_int32), ("n_gapo", C.c_int32), ("n_gape", C.c_int32),
                ("score", C.c_int32), ("extra_flag", C.c_int32)]


class PeOpt(C.Structure):
    """nabwa_pe_opt_t = pe_opt_t (reference bwtaln.h:158-164)"""
    _fields_ = [("max_isize", C.c_int32), ("force_isize", C.c_int32), ("max_occ", C.c_int32), ("max_occ_se", C.c_int32),
                ("n_multi", C.c_int32), ("N_multi", C.c_int32), ("type", C.c_int32), ("is_sw", C.c_int32),
                ("is_preload", C.c_int32), ("ap_prior", C.c_double)]


class PeRec(C.Structure):
    """nabwa_pe_t: one end of a finished pair"""
    _fields_ = [("se", SeRec), ("extra_flag", C.c_int32), ("m_seqid", C.c_int32), ("am", C.c_int32), ("mapQ_paired", C.c_int32),
                ("m_rpos", C.c_int64), ("isize", C.c_int64)]


def pe_opt_default():
    """bwa_init_pe_opt (reference bwape.c:27-41)"""
    po = PeOpt()
    lib().nabwa_pe_opt_default(C.byref(po))
    return po


def isize_infer(hist, ap_prior, L):
    """infer_isize_hist (reference insert_size.c:50-139) -> (rc, IsizeInfo)"""
    h = np.ascontiguousarray(hist, np.uint16)
    ii = IsizeInfo()
    rc = lib().nabwa_isize_infer(_ptr(h), float(ap_prior), int(L), C.byref(ii))
    return rc, ii


ISIZE_FEW, ISIZE_WEIRD = 1, 2


def isize_infer_pairs(pos, length, mapq, ap_prior, L):
    """infer_isize (reference bwape.c:74-175), `bwa sampe`'s estimate over one chunk of positioned pairs: pos / length / mapq per end,
    indexed 2 * pair + end -> (rc, IsizeInfo, the reference's `[infer_isize]` log lines); rc 0, ISIZE_FEW or ISIZE_WEIRD"""
    p = np.ascontiguousarray(pos, np.uint32)
    ln = np.ascontiguousarray(length, np.int32)
    q = np.ascontiguousarray(mapq, np.int32)
    assert p.size == ln.size == q.size and p.size % 2 == 0
    ii = IsizeInfo()
    log = C.create_string_buffer(4096)
    L_ = lib()
    L_.nabwa_isize_infer_pairs.argtypes = [C.c_int, _P, _P, _P, C.c_double, C.c_int64, _P, C.c_char_p, C.c_int]
    rc = L_.nabwa_isize_infer_pairs(p.size // 2, _ptr(p), _ptr(ln), _ptr(q), float(ap_prior), int(L), C.byref(ii), log, len(log))
    if rc < 0:
        raise NabwaError(int(rc), L_.nabwa_last_error().decode())
    return rc, ii, log.value.decode()


def isize_add_pairs(recs, n_pairs, hist):
    """improve_isize_est (reference insert_size.c:141-165) over a batch of positioned pairs; hist: 100000 uint16 bins"""
    assert hist.dtype == np.uint16 and hist.flags.c_contiguous
    lib().nabwa_isize_add_pairs.argtypes = [C.c_int, _P, _P]
    _chk(lib().nabwa_isize_add_pairs(int(n_pairs), C.cast(recs, _P), _ptr(hist)))


def pairing(ends, hits, rows0, rows1, max_isize, s_mm, ii):
    """pairing (reference bwape.c:180-293); ends: (PeEnd * 2), modified in place; returns cnt_chg"""
    hits = np.ascontiguousarray(hits, np.uint64)
    r0 = np.ascontiguousarray(rows0, ALN_DT)
    r1 = np.ascontiguousarray(rows1, ALN_DT)
    return lib().nabwa_pairing(ends, len(hits), _ptr(hits), _ptr(r0), _ptr(r1), int(max_isize), int(s_mm), C.byref(ii))


def pairing_typed(ends, hits, rows0, rows1, max_isize, s_mm, ii, pe_type):
    """pairing with pe_opt_t.type: 1 BWA_PET_STD, 2 BWA_PET_SOLID (colour space, reference bwape.c:234-247)"""
    hits = np.ascontiguousarray(hits, np.uint64)
    r0 = np.ascontiguousarray(rows0, ALN_DT)
    r1 = np.ascontiguousarray(rows1, ALN_DT)
    rc = lib().nabwa_pairing_typed(ends, len(hits), _ptr(hits), _ptr(r0), _ptr(r1), int(max_isize), int(s_mm), C.byref(ii), int(pe_type))
    if rc < 0:
        raise NabwaError(int(rc), lib().nabwa_last_error().decode())
    return rc


CS2NT_MAX = 1024


def cs2nt(off, nt_ref, cs_read, device=0):
    """cs2nt_DP + cs2nt_nt_qual (reference cs2nt.c:36-109) for a batch on the GPU.  Case i has size = off[i + 1] - off[i] colours:
    cs_read[off[i]:off[i + 1]] = colour << 6 | quality (63: N), nt_ref[off[i] + i:off[i + 1] + i + 1] = size + 1 codes 0-4.  Returns the
    uint8 array whose [off[i] - i:off[i + 1] - i - 1] are the size - 1 bytes base << 6 | quality of case i."""
    off = np.ascontiguousarray(off, np.int64)
    n = len(off) - 1
    ref = np.ascontiguousarray(nt_ref, np.uint8)
    cs = np.ascontiguousarray(cs_read, np.uint8)
    assert n >= 0 and cs.size == int(off[-1]) and ref.size == cs.size + n
    out = np.zeros(max(cs.size - n, 1), np.uint8)
    _chk(lib().nabwa_cs2nt(int(device), n, _ptr(off), _ptr(ref), _ptr(cs), _ptr(out)))
    return out[:max(cs.size - n, 0)]


class BwaSeq(C.Structure):
    """bwa_seq_t (reference bwtaln.h:64-90), 200 bytes, as nabwa_bwa_seq_t declares it"""
    _fields_ = [("name", C.c_void_p), ("seq", C.c_void_p), ("rseq", C.c_void_p), ("qual", C.c_void_p),
                ("bits0", C.c_uint32), ("bits1", C.c_uint32), ("score", C.c_int32), ("clip_len", C.c_int32),
                ("n_aln", C.c_int32), ("pad0", C.c_int32), ("aln", C.c_void_p), ("n_multi", C.c_int32), ("pad1", C.c_int32),
                ("multi", C.c_void_p), ("sa", C.c_uint32), ("pos", C.c_uint32), ("c1c2seq", C.c_uint64),
                ("n_cigar", C.c_int32), ("pad2", C.c_int32), ("cigar", C.c_void_p), ("tid", C.c_int32), ("bc", C.c_char * 64),
                ("lenbits", C.c_uint32), ("md", C.c_void_p), ("max_entries", C.c_int32), ("pad3", C.c_int32)]


def encode_read(codes, qual=None, reverse=False, trim_qual=0, is_comp=True):
    """bam1_to_seq's encoding (reference bwaseqio.c:272-307): -> (seq, rseq) of the trimmed length"""
    codes = np.ascontiguousarray(codes, np.uint8)
    q = np.ascontiguousarray(qual, np.uint8) if qual is not None else None
    s = np.zeros(max(len(codes), 1), np.uint8)
    r = np.zeros(max(len(codes), 1), np.uint8)
    L = lib().nabwa_encode_read(len(codes), _ptr(codes), _ptr(q), int(reverse), int(trim_qual), int(is_comp), _ptr(s), _ptr(r))
    return s[:L], r[:L]


def srand48_state(seed):
    """state of the reference's process-global drand48 stream right after srand48(seed)"""
    return ((seed & 0xffffffff) << 16) | 0x330E


def global_align(ref, ref_off, qry, qry_off, gap_open, gap_ext, gap_end, matrix25, band, device=0, max_cigar=MAX_CIGAR):
    """aln_global_core + aln_path2cigar32 (reference stdaln.c:345-525, :1009-1039) for a batch of pairs"""
    n = len(ref_off) - 1
    ref = np.ascontiguousarray(ref, np.uint8)
    qry = np.ascontiguousarray(qry, np.uint8)
    ref_off = np.ascontiguousarray(ref_off, np.int64)
    qry_off = np.ascontiguousarray(qry_off, np.int64)
    mat = np.ascontiguousarray(matrix25, np.int32)
    score = np.zeros(max(n, 1), np.int32)
    ncig = np.zeros(max(n, 1), np.int32)
    cig = np.zeros((max(n, 1), max_cigar), np.uint32)
    _chk(lib().nabwa_global_align(device, n, _ptr(ref_off), _ptr(ref), _ptr(qry_off), _ptr(qry), gap_open, gap_ext,
                                  gap_end, _ptr(mat), band, _ptr(score), _ptr(ncig), _ptr(cig), max_cigar))
    return score[:n], [cig[i, :ncig[i]] for i in range(n)]


def local_align(ref, ref_off, qry, qry_off, gap_open, gap_ext, matrix25, band, thres=1, device=0, max_cigar=MAX_CIGAR):
    """aln_local_core (reference stdaln.c:529-761) for a batch of pairs -> (score, coords[n,4], subo, cigars)"""
    n = len(ref_off) - 1
    ref = np.ascontiguousarray(ref, np.uint8)
    qry = np.ascontiguousarray(qry, np.uint8)
    ref_off = np.ascontiguousarray(ref_off, np.int64)
    qry_off = np.ascontiguousarray(qry_off, np.int64)
    mat = np.ascontiguousarray(matrix25, np.int32)
    score = np.zeros(max(n, 1), np.int32)
    coords = np.zeros((max(n, 1), 4), np.int32)
    subo = np.zeros(max(n, 1), np.int32)
    ncig = np.zeros(max(n, 1), np.int32)
    cig = np.zeros((max(n, 1), max_cigar), np.uint32)
    _chk(lib().nabwa_local_align(device, n, _ptr(ref_off), _ptr(ref), _ptr(qry_off), _ptr(qry), gap_open, gap_ext, _ptr(mat),
                                 band, thres, _ptr(score), _ptr(coords), _ptr(subo), _ptr(ncig), _ptr(cig), max_cigar))
    return score[:n], coords[:n], subo[:n], [cig[i, :ncig[i]] for i in range(n)]


def extend_align(ref, ref_off, qry, qry_off, gap_open, gap_ext, matrix25, band, g0, device=0, max_cigar=MAX_CIGAR):
    """aln_extend_core (reference stdaln.c:862-1007) for a batch of pairs"""
    n = len(ref_off) - 1
    ref = np.ascontiguousarray(ref, np.uint8)
    qry = np.ascontiguousarray(qry, np.uint8)
    ref_off = np.ascontiguousarray(ref_off, np.int64)
    qry_off = np.ascontiguousarray(qry_off, np.int64)
    mat = np.ascontiguousarray(matrix25, np.int32)
    g0 = np.ascontiguousarray(g0, np.int32)
    score = np.zeros(max(n, 1), np.int32)
    ncig = np.zeros(max(n, 1), np.int32)
    cig = np.zeros((max(n, 1), max_cigar), np.uint32)
    _chk(lib().nabwa_extend_align(device, n, _ptr(ref_off), _ptr(ref), _ptr(qry_off), _ptr(qry), gap_open, gap_ext,
                                  _ptr(mat), band, _ptr(g0), _ptr(score), _ptr(ncig), _ptr(cig), max_cigar))
    return score[:n], [cig[i, :ncig[i]] for i in range(n)]


def dp_form_counts():
    """launches of the alignment kernels by form since the library was loaded (nabwa_dp_form_counts):
    global wave / global LDS lanes / global HBM lanes / local rows in LDS / local rows in HBM / extension rows in LDS /
    extension rows in HBM"""
    out = (C.c_uint64 * 7)()
    lib().nabwa_dp_form_counts(out, 7)
    return list(out)


def finish_counts():
    """the finishing chains' device path since the library was loaded (nabwa_finish_counts): jobs refined on the device, records whose
    MD / NM the device wrote, chain calls that took the device path (NABWA_FINISH=gpu), bytes of reference held in HBM for it"""
    out = (C.c_uint64 * 4)()
    lib().nabwa_finish_counts(out)
    return list(out)


class NabwaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libnabwa error %d: %s" % (code, msg))
        self.code = code


def build(verbose=False):
    """Compile libnabwa.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "all"], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libnabwa.so failed:\n%s\n%s" % (r.stdout, r.stderr))


_lib = None
_P = C.c_void_p


def lib():
    """The loaded library.  Raises if it has not been built -- there is no other implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libnabwa.so is missing (%s): run __graft_entry__.build() / make -C %s"
                           % (LIB_PATH, os.path.join(_HERE, "csrc")))
    L = C.CDLL(LIB_PATH)
    L.nabwa_last_error.restype = C.c_char_p
    L.nabwa_device_count.restype = C.c_int
    L.nabwa_gap_init_opt.argtypes = [_P]
    L.nabwa_cal_maxdiff.restype = C.c_int
    L.nabwa_cal_maxdiff.argtypes = [C.c_int, C.c_double, C.c_double]
    L.nabwa_index_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, _P]
    L.nabwa_index_from_arrays.argtypes = [C.c_int, C.c_int, _P, C.c_uint64, _P, C.c_uint64, _P, C.c_uint64, _P,
                                          C.c_uint64, _P]
    L.nabwa_index_destroy.argtypes = [_P]
    L.nabwa_index_destroy.restype = None
    L.nabwa_index_seq_len.restype = C.c_uint32
    L.nabwa_index_seq_len.argtypes = [_P, C.c_int]
    L.nabwa_index_device_bytes.restype = C.c_uint64
    L.nabwa_index_device_bytes.argtypes = [_P]
    L.nabwa_cal_sa_reg_gap.argtypes = [_P, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, C.c_int64, _P, _P]
    L.nabwa_batch_create.argtypes = [_P, _P, C.c_int, _P, _P, _P, C.c_int, _P]
    L.nabwa_batch_run.argtypes = [_P]
    L.nabwa_batch_sync.argtypes = [_P, _P]
    L.nabwa_batch_last_kernel_ms.restype = C.c_float
    L.nabwa_batch_last_kernel_ms.argtypes = [_P]
    L.nabwa_batch_last_width_ms.restype = C.c_float
    L.nabwa_batch_last_width_ms.argtypes = [_P]
    L.nabwa_batch_last_deep_ms.restype = C.c_float
    L.nabwa_batch_last_deep_ms.argtypes = [_P]
    L.nabwa_batch_fetch.argtypes = [_P, _P, _P, C.c_int64, _P, _P]
    L.nabwa_batch_checksum.argtypes = [_P, _P, _P]
    L.nabwa_batch_count_touches.argtypes = [_P, _P, _P]
    L.nabwa_batch_config.argtypes = [_P, _P]
    if hasattr(L, "nabwa_batch_sure0_stats"):      # (a library of an earlier build, loaded through NABWA_LIB for an A/B run, has no such entry)
        L.nabwa_batch_sure0_stats.restype = C.c_int
        L.nabwa_batch_sure0_stats.argtypes = [_P, _P]
    if hasattr(L, "nabwa_batch_sure0_stats_ex"):
        L.nabwa_batch_sure0_stats_ex.restype = C.c_int
        L.nabwa_batch_sure0_stats_ex.argtypes = [_P, _P]
    if hasattr(L, "nabwa_batch_dedup_stats"):
        L.nabwa_batch_dedup_stats.restype = C.c_int
        L.nabwa_batch_dedup_stats.argtypes = [_P, _P]
    for f in ("nabwa_batch_dedup_stats_ex", "nabwa_index_dedup_cache_stats"):
        if hasattr(L, f):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [_P, _P]
    if hasattr(L, "nabwa_index_dedup_cache_clear"):
        L.nabwa_index_dedup_cache_clear.restype = C.c_int
        L.nabwa_index_dedup_cache_clear.argtypes = [_P]
    L.nabwa_dp_form_counts.argtypes = [_P, C.c_int]
    L.nabwa_dp_form_counts.restype = None
    L.nabwa_batch_destroy.argtypes = [_P]
    L.nabwa_batch_destroy.restype = None
    L.nabwa_sa_lookup.argtypes = [_P, C.c_int, _P, _P, _P]
    L.nabwa_occ4.argtypes = [_P, C.c_int, C.c_int, _P, _P]
    L.nabwa_global_align.argtypes = [C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P,
                                     C.c_int]
    L.nabwa_extend_align.argtypes = [C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P, C.c_int]
    L.nabwa_local_align.argtypes = [C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P,
                                    C.c_int]
    L.nabwa_index_attach_reference.argtypes = [_P, C.c_char_p]
    L.nabwa_bwa_cal_sa_reg_gap.argtypes = [_P, C.c_int, _P, _P]
    L.nabwa_isize_infer.argtypes = [_P, C.c_double, C.c_int64, _P]
    L.nabwa_isize_bin.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_int]
    L.nabwa_pairing.argtypes = [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P]
    L.nabwa_encode_read.restype = C.c_int
    L.nabwa_encode_read.argtypes = [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P]
    L.nabwa_se_finish.argtypes = [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P]
    L.nabwa_index_export.argtypes = [_P, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _P]
    L.nabwa_pe_opt_default.argtypes = [_P]
    L.nabwa_pe_opt_default.restype = None
    L.nabwa_pe_posn.argtypes = [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P]
    L.nabwa_pe_finish.argtypes = [_P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P]
    L.nabwa_index_fa2pac.restype = C.c_int64
    L.nabwa_index_fa2pac.argtypes = [C.c_char_p, C.c_char_p]
    L.nabwa_index_fa2cspac.restype = C.c_int64
    L.nabwa_index_fa2cspac.argtypes = [C.c_char_p, C.c_char_p]
    L.nabwa_index_build.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.nabwa_index_build_estimate.argtypes = [C.c_uint64, _P]
    L.nabwa_cs2nt.argtypes = [C.c_int, C.c_int, _P, _P, _P, _P]
    L.nabwa_index_attach_nt_reference.argtypes = [_P, C.c_char_p]
    L.nabwa_se_finish_cs.argtypes = [_P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P]
    L.nabwa_pe_finish_sampe_cs.argtypes = [_P, _P, _P, _P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]
    L.nabwa_pairing_typed.argtypes = [_P, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int]
    L.nabwa_bgzf_bound.restype = C.c_int64
    L.nabwa_bgzf_bound.argtypes = [C.c_int64]
    L.nabwa_bgzf_compress.argtypes = [C.c_int, _P, C.c_int64, _P, C.c_int64, _P, _P]
    L.nabwa_bgzf_create.argtypes = [C.c_int, _P]
    L.nabwa_bgzf_handle_compress.argtypes = [_P, _P, C.c_int64, _P, C.c_int64, _P, _P]
    L.nabwa_bgzf_destroy.argtypes = [_P]
    L.nabwa_bgzf_compress_ex.argtypes = [C.c_int, C.c_int, _P, C.c_int64, _P, C.c_int64, _P, _P]
    L.nabwa_bgzf_handle_compress_ex.argtypes = [_P, C.c_int, _P, C.c_int64, _P, C.c_int64, _P, _P]
    L.nabwa_bgzf_inflated_size.argtypes = [_P, C.c_int64, _P, _P]
    L.nabwa_bgzf_decompress.argtypes = [C.c_int, _P, C.c_int64, _P, C.c_int64, _P, _P]
    L.nabwa_bgzf_handle_decompress.argtypes = [_P, _P, C.c_int64, _P, C.c_int64, _P, _P]
    L.nabwa_bgzf_destroy.restype = None
    if hasattr(L, "nabwa_bam_sort_run"):           # (likewise)
        L.nabwa_bam_sort_create.argtypes = [C.c_int, _P]
        L.nabwa_bam_sort_destroy.argtypes = [_P]
        L.nabwa_bam_sort_destroy.restype = None
        L.nabwa_bam_sort_run.argtypes = [_P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P]
        L.nabwa_bam_sort.argtypes = [C.c_int, C.c_int64, _P, _P, _P, C.c_int64, _P, _P]
        L.nabwa_bam_sort_times.argtypes = [_P, _P]
    if hasattr(L, "nabwa_bam_sort_run_ex"):        # (likewise)
        L.nabwa_bam_sort_run_ex.argtypes = [_P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, _P]
        L.nabwa_bam_sort_ex.argtypes = [C.c_int, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, _P]
    if hasattr(L, "nabwa_markdup_add"):            # (likewise)
        L.nabwa_markdup_default_opt.argtypes = [_P]
        L.nabwa_markdup_default_opt.restype = None
        L.nabwa_markdup_create.argtypes = [C.c_int, _P, _P]
        L.nabwa_markdup_add.argtypes = [_P, C.c_int64, _P, _P]
        L.nabwa_markdup_resolve.argtypes = [_P, _P, C.c_int64, _P]
        L.nabwa_markdup_clear.argtypes = [_P]
        L.nabwa_markdup_destroy.argtypes = [_P]
        L.nabwa_markdup_destroy.restype = None
        L.nabwa_markdup_times.argtypes = [_P, _P]
    if hasattr(L, "nabwa_bai_add"):                # (likewise)
        L.nabwa_bai_create.argtypes = [C.c_int, C.c_int32, _P]
        L.nabwa_bai_add.argtypes = [_P, C.c_int64, _P, _P, C.c_int64]
        L.nabwa_bai_finish.argtypes = [_P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P]
        L.nabwa_bai_clear.argtypes = [_P]
        L.nabwa_bai_destroy.argtypes = [_P]
        L.nabwa_bai_destroy.restype = None
        L.nabwa_bai_times.argtypes = [_P, _P]
        L.nabwa_bgzf_block_table.argtypes = [_P, C.c_int64, _P, _P, C.c_int64, _P]
    if hasattr(L, "nabwa_damage_add"):             # (likewise)
        L.nabwa_damage_default_opt.argtypes = [_P]
        L.nabwa_damage_default_opt.restype = None
        L.nabwa_damage_create.argtypes = [_P, _P, _P]
        L.nabwa_damage_add.argtypes = [_P, C.c_int64, _P, _P]
        L.nabwa_damage_fetch.argtypes = [_P, _P, _P, _P, _P]
        L.nabwa_damage_clear.argtypes = [_P]
        L.nabwa_damage_destroy.argtypes = [_P]
        L.nabwa_damage_destroy.restype = None
        L.nabwa_damage_times.argtypes = [_P, _P]
    if hasattr(L, "nabwa_finish_counts"):          # (a library of an earlier build, loaded through NABWA_LIB for an A/B run, has no such entries)
        L.nabwa_refine_gapped_core.argtypes = [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_int]
        L.nabwa_cal_md.argtypes = [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P, C.c_int64]
        L.nabwa_finish_counts.argtypes = [_P]
        L.nabwa_finish_counts.restype = None
    _lib = L
    return L


def _chk(rc):
    if rc != OK:
        raise NabwaError(rc, lib().nabwa_last_error().decode())


def _ptr(a):
    return a.ctypes.data_as(_P) if a is not None else None


def gap_init_opt():
    """gap_init_opt (reference bwtaln.c:19-35)."""
    o = GapOpt()
    lib().nabwa_gap_init_opt(C.byref(o))
    return o


def cal_maxdiff(length, err=0.02, thres=0.04):
    """bwa_cal_maxdiff (reference bwtaln.c:37-49)."""
    return lib().nabwa_cal_maxdiff(int(length), float(err), float(thres))


def index_fa2pac(fasta, prefix, colour=False):
    """`bwa index` up to the BWT (reference bntseq.c:166-256, bwtmisc.c:168-193): FASTA (plain or gzip) -> <prefix>.pac, .ann,
    .amb, .rpac; colour=True: `bwa index -c`'s <prefix>.nt.pac/.ann/.amb and the colour <prefix>.pac/.ann/.amb/.rpac
    (bwtmisc.c:210-254).  Host only.  Returns l_pac."""
    f = lib().nabwa_index_fa2cspac if colour else lib().nabwa_index_fa2pac
    n = f(os.fsencode(fasta), os.fsencode(prefix))
    if n < 0:
        raise NabwaError(int(n), lib().nabwa_last_error().decode())
    return int(n)


SAMSE_PATH = os.path.join(_HERE, "nabwa_samse")
SAMPE_PATH = os.path.join(_HERE, "nabwa_sampe")


def samse(prefix, sai, reads, out=None, args=(), device=None, timeout=None):
    """`bwa samse [args] <prefix> <in.sai> <reads>` (reference bwase.c:723-750) with the finishing chain on the GPU: runs the
    nabwa_samse tool and returns its subprocess.CompletedProcess (SAM in .stdout unless out is given, which is written through
    final_rename: a name ending in '_' loses it once the file is complete)"""
    return _sai2sam(SAMSE_PATH, list(args), [prefix, sai, reads], out, device, timeout)


def sampe(prefix, sai1, sai2, reads1, reads2, out=None, args=(), device=None, timeout=None):
    """`bwa sampe [args] <prefix> <in1.sai> <in2.sai> <in1.fq> <in2.fq>` (reference bwape.c:764-817) with the finishing chain on
    the GPU; as samse()"""
    return _sai2sam(SAMPE_PATH, list(args), [prefix, sai1, sai2, reads1, reads2], out, device, timeout)


def _sai2sam(tool, args, operands, out, device, timeout):
    if not os.path.exists(tool):
        raise RuntimeError("%s is missing: run __graft_entry__.build()" % tool)
    env = dict(os.environ)
    if device is not None:
        env["NABWA_DEVICE"] = str(int(device))
    cmd = [tool] + [str(a) for a in args] + (["-f", str(out)] if out else []) + [os.fspath(x) for x in operands]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=timeout)


WORKER_PATH = os.path.join(_HERE, "nabwa_worker")


def worker(host, port, args=(), device=None, timeout=None):
    """`bwa worker -h <host> -p <port> [args]` (reference bam2bam.c:2213-2309) with the alignment on the GPU: runs the nabwa_worker tool
    until the master ends it and returns its subprocess.CompletedProcess (the log and the record counts in .stderr).  libzmq is bound
    by the tool at run time (NABWA_ZMQ_LIB, libzmq.so.5, .so.3, .so); args: -t N connections, -T minutes."""
    if not os.path.exists(WORKER_PATH):
        raise RuntimeError("%s is missing: run __graft_entry__.build()" % WORKER_PATH)
    env = dict(os.environ)
    if device is not None:
        env["NABWA_DEVICE"] = str(int(device))
    cmd = [WORKER_PATH, "-h", str(host), "-p", str(int(port))] + [str(a) for a in args]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=timeout)


def index_build(prefix, device=0, sa_intv=32, verbose=False):
    """The FM-indexes of <prefix>.pac on the GPU: <prefix>.bwt, .rbwt, .sa, .rsa (reference bwtindex.c:104-191)."""
    _chk(lib().nabwa_index_build(os.fsencode(prefix), int(device), int(sa_intv), int(verbose)))


def index_build_estimate(l_pac):
    """Worst-case device bytes nabwa_index_build needs for l_pac bases (what it checks before allocating)."""
    out = C.c_uint64()
    _chk(lib().nabwa_index_build_estimate(int(l_pac), C.byref(out)))
    return out.value


def bgzf_bound(n):
    """upper bound of bgzf_compress's output for n input bytes (nabwa_bgzf_bound)"""
    return int(lib().nabwa_bgzf_bound(int(n)))


def _bgzf_call(f, first, data, cap):
    a = np.frombuffer(bytes(data), np.uint8)
    cap = bgzf_bound(a.size) if cap is None else int(cap)
    out = np.empty(max(cap, 1), np.uint8)
    n_out, n_blocks = C.c_int64(), C.c_int64()
    rc = f(first, _ptr(a), a.size, _ptr(out), cap, C.byref(n_out), C.byref(n_blocks))
    if rc != OK:
        e = NabwaError(rc, lib().nabwa_last_error().decode())
        e.needed = n_out.value
        raise e
    return out[:n_out.value].tobytes()


BGZF_CODES = {"fixed": 0, "dynamic": 1}                # NABWA_BGZF_CODES_FIXED, NABWA_BGZF_CODES_DYNAMIC


def _bgzf_codes(codes):
    if not isinstance(codes, str) or codes not in BGZF_CODES:
        raise ValueError("codes: 'fixed' or 'dynamic', not %r" % (codes,))
    return BGZF_CODES[codes]


def bgzf_compress(data, device=0, cap=None, codes="fixed"):
    """data -> its BGZF blocks (slices of <= 0xff00 bytes, one block each, no end-of-file block), compressed on the GPU
    (nabwa_bgzf_compress_ex).  Only the inflated bytes are contract.  cap: the output capacity handed to the library (default: the
    bound); a NabwaError of code ECAP carries the size that would do in .needed.  codes: "fixed" (fixed Huffman codes or stored
    blocks) or "dynamic" (a dynamic Huffman block where that is shorter; no block is larger than with "fixed")"""
    k = _bgzf_codes(codes)
    return _bgzf_call(lambda dev, *a: lib().nabwa_bgzf_compress_ex(dev, k, *a), int(device), data, cap)


def bgzf_inflated_size(data):
    """whole BGZF members back to back -> (inflated bytes, members), from their headers alone; needs no device.  NabwaError of code
    EDATA for input that is not whole BGZF members (nabwa_bgzf_inflated_size)"""
    a = np.frombuffer(bytes(data), np.uint8)
    n_out, n_blocks = C.c_int64(), C.c_int64()
    _chk(lib().nabwa_bgzf_inflated_size(_ptr(a), a.size, C.byref(n_out), C.byref(n_blocks)))
    return n_out.value, n_blocks.value


def bgzf_block_table(data):
    """a BGZF file that ends with its end-of-file block -> (blk_uoff, blk_coff): where every member starts in the inflated stream and in the
    file, the end-of-file block last (int64 arrays of the members' number), from the BSIZE and ISIZE fields alone; needs no device.  It is
    what Bai.finish takes.  NabwaError of code EDATA as bgzf_inflated_size, and for a file whose last member is not empty"""
    a = np.frombuffer(bytes(data), np.uint8)
    n_blk = C.c_int64()
    _chk(lib().nabwa_bgzf_block_table(_ptr(a), a.size, None, None, 0, C.byref(n_blk)))
    uoff, coff = np.zeros(n_blk.value + 1, np.int64), np.zeros(n_blk.value + 1, np.int64)
    _chk(lib().nabwa_bgzf_block_table(_ptr(a), a.size, _ptr(uoff), _ptr(coff), uoff.size, C.byref(n_blk)))
    return uoff, coff


def bgzf_decompress(data, device=0, cap=None):
    """whole BGZF members back to back -> their inflated bytes, inflated and checked against each member's CRC-32 and ISIZE on the
    GPU (nabwa_bgzf_decompress).  cap: the output capacity handed to the library (default: what the headers say); a NabwaError of
    code ECAP carries the size that would do in .needed, one of code EDATA names the member that is damaged"""
    if cap is None:
        cap = bgzf_inflated_size(data)[0]
    return _bgzf_call(lib().nabwa_bgzf_decompress, int(device), data, cap)


class Bgzf:
    """the compressor and the decompressor as a handle that keeps its stream and buffers between calls (nabwa_bgzf_create)"""

    def __init__(self, device=0):
        self._h = _P()
        _chk(lib().nabwa_bgzf_create(int(device), C.byref(self._h)))

    def compress(self, data, cap=None, codes="fixed"):
        k = _bgzf_codes(codes)
        return _bgzf_call(lambda h, *a: lib().nabwa_bgzf_handle_compress_ex(h, k, *a), self._h, data, cap)

    def decompress(self, data, cap=None):
        if cap is None:
            cap = bgzf_inflated_size(data)[0]
        return _bgzf_call(lib().nabwa_bgzf_handle_decompress, self._h, data, cap)

    def close(self):
        if self._h:
            lib().nabwa_bgzf_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bam_sort_key(tid, pos):
    """the sort key of a BAM record (NABWA_BAM_SORT_KEY): the reference id as an unsigned word, so that -1 sorts last, then pos + 1, so that
    -1 sorts first"""
    return ((int(tid) & 0xffffffff) << 32) | ((int(pos) + 1) & 0xffffffff)


def bam_record_offsets(records):
    """the offsets (n + 1) of the records of an uncompressed BAM record stream, from their block_size words"""
    a = np.frombuffer(bytes(records), np.uint8)
    off, q = [0], 0
    while q < a.size:
        if a.size - q < 4:
            raise ValueError("a record is cut short at byte %d" % q)
        q += 4 + int.from_bytes(a[q:q + 4].tobytes(), "little")
        off.append(q)
    if q != a.size:
        raise ValueError("the last record runs past the end of the bytes")
    return np.array(off, np.int64)


def _bam_sort_call(f, first, records, off, cap, perm=False):
    a = np.frombuffer(bytes(records), np.uint8)
    off = bam_record_offsets(a) if off is None else np.ascontiguousarray(off, np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("off: n + 1 offsets")
    n = off.size - 1
    total = int(off[-1] - off[0])
    cap = max(total, 0) if cap is None else int(cap)
    out = np.empty(max(cap, 1), np.uint8)
    out_off, keys = np.zeros(n + 1, np.int64), np.zeros(n, np.uint64)
    if perm:
        order = np.zeros(n, np.uint32)
        rc = f(first, n, _ptr(a) if a.size else None, _ptr(off), _ptr(out), cap, _ptr(out_off), _ptr(keys), _ptr(order))
    else:
        rc = f(first, n, _ptr(a) if a.size else None, _ptr(off), _ptr(out), cap, _ptr(out_off), _ptr(keys))
    if rc != OK:
        e = NabwaError(rc, lib().nabwa_last_error().decode())
        e.needed = total
        raise e
    res = (out[:total].tobytes() if n else b"", out_off, keys)
    return res + (order,) if perm else res


def bam_sort(records, off=None, device=0, cap=None, perm=False):
    """finished BAM records (an uncompressed record stream: u32 block_size + block, back to back) -> (the records sorted by coordinate,
    their offsets, their keys), sorted and gathered on the GPU (nabwa_bam_sort).  The order is that of bam_sort_key, stable: records of
    equal key keep their order.  off: the records' offsets (n + 1), as nabwa_bam_batch_output gives them; None: walked from the block_size
    words on the host.  cap: the output capacity handed to the library (default: the records' total); a NabwaError of code ECAP
    carries the size that would do in .needed, one of code EDATA names the first record whose block_size is not what its offsets say.
    perm=True appends the permutation as a fourth result: for each output record the index it had in the input (nabwa_bam_sort_ex)"""
    if perm:
        return _bam_sort_call(lib().nabwa_bam_sort_ex, int(device), records, off, cap, True)
    return _bam_sort_call(lib().nabwa_bam_sort, int(device), records, off, cap)


class BamSort:
    """the coordinate sort as a handle that keeps its stream and its device buffers between calls (nabwa_bam_sort_create)"""

    def __init__(self, device=0):
        self._h = _P()
        _chk(lib().nabwa_bam_sort_create(int(device), C.byref(self._h)))

    def sort(self, records, off=None, cap=None, perm=False):
        if perm:
            return _bam_sort_call(lib().nabwa_bam_sort_run_ex, self._h, records, off, cap, True)
        return _bam_sort_call(lib().nabwa_bam_sort_run, self._h, records, off, cap)

    run = sort                                     # (nabwa_bam_sort_run)

    def times(self):
        """device-event times of the last sort in ms: upload, key kernel, radix sort, sizes + scan, gather kernel, download"""
        ms = (C.c_float * 6)()
        _chk(lib().nabwa_bam_sort_times(self._h, ms))
        return list(ms)

    def close(self):
        if self._h:
            lib().nabwa_bam_sort_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DamageOpt(C.Structure):
    """nabwa_damage_opt_t"""
    _fields_ = [("n_pos", C.c_int32), ("min_mapq", C.c_int32), ("exclude_flags", C.c_uint32), ("require_flags", C.c_uint32), ("which_ref", C.c_int32), ("pad", C.c_int32)]


DAMAGE_LEN_BINS = 1024
damage_stat_names = ("seen", "counted", "skipped_flags", "skipped_place", "skipped_mapq", "skipped_empty", "columns_counted", "columns_skipped_read",
                     "columns_skipped_ref")       # the slots of stats[], NABWA_DAMAGE_STAT_*


class Damage:
    """the damage profile of finished BAM records on the GPU (nabwa_damage_*): the substitutions of the mapped reads against the index's
    reference by distance from the read's ends, and the read lengths; include/nabwa.h has the rules.  The handle works on the index's device
    with the index's copy of the reference, and the index must outlive it"""

    def __init__(self, index, n_pos=25, min_mapq=0, exclude_flags=0xF04, require_flags=0, which_ref=0):
        self._h = _P()
        self._index = index                        # (kept alive)
        self.n_pos = int(n_pos)
        o = DamageOpt(int(n_pos), int(min_mapq), int(exclude_flags), int(require_flags), int(which_ref), 0)
        _chk(lib().nabwa_damage_create(index._h, C.byref(o), C.byref(self._h)))

    def add(self, records, off=None):
        """counts the records of an uncompressed BAM record stream; off: their offsets (n + 1), None: walked from the block_size words on
        the host.  A NabwaError of code EDATA names the first damaged record, and that call has counted nothing"""
        a = np.frombuffer(bytes(records), np.uint8) if not isinstance(records, np.ndarray) else np.ascontiguousarray(records, np.uint8)
        off = bam_record_offsets(a) if off is None else np.ascontiguousarray(off, np.int64)
        if off.ndim != 1 or off.size < 1:
            raise ValueError("off: n + 1 offsets")
        _chk(lib().nabwa_damage_add(self._h, off.size - 1, _ptr(a) if a.size else None, _ptr(off)))

    def fetch(self):
        """-> (sub5, sub3, len_hist, stats): uint64 arrays of shape (n_pos + 1, 4, 4), (n_pos + 1, 4, 4), (1024,) and (len(damage_stat_names),);
        sub5[p][r][q]: reference base r read as q at distance p from the 5' end, on the read's own strand; row n_pos: everything further in"""
        sub5, sub3 = np.zeros((self.n_pos + 1, 4, 4), np.uint64), np.zeros((self.n_pos + 1, 4, 4), np.uint64)
        len_hist, stats = np.zeros(DAMAGE_LEN_BINS, np.uint64), np.zeros(len(damage_stat_names), np.uint64)
        _chk(lib().nabwa_damage_fetch(self._h, _ptr(sub5), _ptr(sub3), _ptr(len_hist), _ptr(stats)))
        return sub5, sub3, len_hist, stats

    def clear(self):
        _chk(lib().nabwa_damage_clear(self._h))

    def times(self):
        """device-event times of the last add in ms: upload, kernel, adding the call's table to the totals"""
        ms = (C.c_float * 3)()
        _chk(lib().nabwa_damage_times(self._h, ms))
        return list(ms)

    def close(self):
        if self._h:
            lib().nabwa_damage_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MarkDupOpt(C.Structure):
    """nabwa_markdup_opt_t"""
    _fields_ = [("min_qual", C.c_int32), ("single_ends", C.c_int32), ("exclude_flags", C.c_uint32), ("pad", C.c_int32)]


MARKDUP_ENDS = {"5p": 0, "both": 1}                # NABWA_MARKDUP_ENDS_5P, _BOTH
markdup_stat_names = ("seen", "skipped_flags", "already", "unmapped", "fragments", "pairs", "orphans", "dup_fragments", "dup_pairs",
                      "dup_records")               # the slots of stats[], NABWA_MARKDUP_STAT_*


def _records_and_offsets(records, off):
    a = np.frombuffer(bytes(records), np.uint8) if not isinstance(records, np.ndarray) else np.ascontiguousarray(records, np.uint8)
    off = bam_record_offsets(a) if off is None else np.ascontiguousarray(off, np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("off: n + 1 offsets")
    return a, off


class MarkDup:
    """duplicate marking of finished BAM records on the GPU (nabwa_markdup_*): records that share their unclipped 5' end and strand (pairs:
    both ends) are one group, its best-scoring member stays and the others are marked; include/nabwa.h has the rules.  Mates must lie
    next to each other within one add."""

    def __init__(self, device=0, min_qual=15, single_ends="5p", exclude_flags=0xB00):
        if single_ends not in MARKDUP_ENDS:
            raise ValueError('single_ends: "5p" or "both"')
        self._h = _P()
        self.n = 0                                 # records added since create / clear
        o = MarkDupOpt(int(min_qual), MARKDUP_ENDS[single_ends], int(exclude_flags), 0)
        _chk(lib().nabwa_markdup_create(int(device), C.byref(o), C.byref(self._h)))

    def add(self, records, off=None):
        """takes the records of an uncompressed BAM record stream; off: their offsets (n + 1), None: walked from the block_size words on
        the host.  A NabwaError of code EDATA names the first damaged record, and that call has added nothing"""
        a, off = _records_and_offsets(records, off)
        _chk(lib().nabwa_markdup_add(self._h, off.size - 1, _ptr(a) if a.size else None, _ptr(off)))
        self.n += off.size - 1

    def resolve(self):
        """-> (dup, stats): dup[i] = 1 where the i-th record added is a duplicate (uint8), stats by markdup_stat_names (uint64)"""
        dup, stats = np.zeros(self.n, np.uint8), np.zeros(len(markdup_stat_names), np.uint64)
        _chk(lib().nabwa_markdup_resolve(self._h, _ptr(dup) if self.n else None, self.n, _ptr(stats)))
        return dup, stats

    def clear(self):
        _chk(lib().nabwa_markdup_clear(self._h))
        self.n = 0

    def times(self):
        """device-event times in ms: of the last add upload and signature kernels, of the last resolve sorts, mark kernels and download"""
        ms = (C.c_float * 5)()
        _chk(lib().nabwa_markdup_times(self._h, ms))
        return list(ms)

    def close(self):
        if self._h:
            lib().nabwa_markdup_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def markdup(records, off=None, device=0, **opts):
    """finished BAM records -> (the same bytes with flag 0x400 set on the duplicates, dup, stats), marked on the GPU (MarkDup used once)"""
    a, off = _records_and_offsets(records, off)
    with MarkDup(device, **opts) as m:
        m.add(a, off)
        dup, stats = m.resolve()
    out = a.copy()
    out[off[:-1][dup != 0] + 19] |= 0x04           # flag: bytes 18..19 of a record; 0x400 is bit 2 of the upper one
    return out.tobytes(), dup, stats


bai_stat_names = ("records", "placed", "no_coor", "bins", "chunks", "windows", "bytes")      # the slots of stats[], NABWA_BAI_STAT_*


class Bai:
    """the BAM index (.bai) of finished, coordinate-sorted BAM records, built on the GPU (nabwa_bai_*); include/nabwa.h has the rules.
    n_ref: the reference sequences of the file's header."""

    def __init__(self, n_ref, device=0):
        self._h = _P()
        self.end = 0                               # where the records added so far end in the uncompressed stream
        _chk(lib().nabwa_bai_create(int(device), int(n_ref), C.byref(self._h)))

    def add(self, records, off=None, stream_off=0):
        """takes the next records of the file; off: their offsets (n + 1), None: walked from the block_size words on the host; stream_off:
        where the first of them lies in the uncompressed BAM stream, header included -- not before the end of those added so far.  A
        NabwaError of code EDATA names the first damaged or misplaced record, and that call has added nothing"""
        a, off = _records_and_offsets(records, off)
        _chk(lib().nabwa_bai_add(self._h, off.size - 1, _ptr(a) if a.size else None, _ptr(off), int(stream_off)))
        if off.size > 1:
            self.end = int(stream_off) + int(off[-1] - off[0])

    def size(self, blk_uoff, blk_coff):
        """the bytes finish would return"""
        u, c = np.ascontiguousarray(blk_uoff, np.int64), np.ascontiguousarray(blk_coff, np.int64)
        if u.ndim != 1 or u.size < 1 or u.shape != c.shape:
            raise ValueError("blk_uoff, blk_coff: n_blk + 1 entries each")
        n = C.c_int64()
        _chk(lib().nabwa_bai_finish(self._h, u.size - 1, _ptr(u), _ptr(c), None, 0, C.byref(n), None))
        return n.value

    def finish(self, blk_uoff, blk_coff):
        """blk_uoff, blk_coff: where every BGZF block of the finished file starts in the uncompressed stream and in the file, the
        end-of-file block last (bgzf_block_table) -> (the .bai file's bytes, stats by bai_stat_names (uint64)).  The handle keeps what was
        added: more adds and another finish may follow"""
        u, c = np.ascontiguousarray(blk_uoff, np.int64), np.ascontiguousarray(blk_coff, np.int64)
        out = np.zeros(self.size(u, c), np.uint8)
        n, stats = C.c_int64(), np.zeros(len(bai_stat_names), np.uint64)
        _chk(lib().nabwa_bai_finish(self._h, u.size - 1, _ptr(u), _ptr(c), _ptr(out), out.size, C.byref(n), _ptr(stats)))
        return out[:n.value].tobytes(), stats

    def clear(self):
        _chk(lib().nabwa_bai_clear(self._h))
        self.end = 0

    def times(self):
        """device-event times in ms: of the last add upload and signature kernel, of the last finish radix sort, virtual offsets / chunks /
        layout, linear index, writer kernels and download"""
        ms = (C.c_float * 7)()
        _chk(lib().nabwa_bai_times(self._h, ms))
        return list(ms)

    def close(self):
        if self._h:
            lib().nabwa_bai_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bai(records, blk_uoff, blk_coff, n_ref, stream_off=0, off=None, device=0):
    """finished, coordinate-sorted BAM records that start at stream_off of the uncompressed stream, and the block table of the BGZF file they
    were written to -> (the .bai file's bytes, stats), built on the GPU (Bai used once)"""
    with Bai(n_ref, device) as b:
        b.add(records, off, stream_off)
        return b.finish(blk_uoff, blk_coff)


class Index:
    """Both FM-indexes (forward and reversed text) resident in HBM; replaces the globals set up by
    init_genome_index (reference bam2bam.c:844-858)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, prefix, device=0, with_sa=True, with_ref=False):
        h = _P()
        _chk(lib().nabwa_index_load(prefix.encode(), device, int(with_sa), int(with_ref), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, bwt0, bwt1, sa0=None, sa1=None, device=0, device_ptrs=False):
        """bwt0/bwt1: .bwt/.rbwt file content as uint32 words (numpy arrays, or (ptr, n_words) tuples of
        device memory when device_ptrs)."""
        h = _P()

        def pn(x):
            if x is None:
                return None, 0
            if isinstance(x, tuple):
                return C.c_void_p(x[0]), int(x[1])
            return _ptr(x), x.size
        p0, n0 = pn(bwt0)
        p1, n1 = pn(bwt1)
        s0, m0 = pn(sa0)
        s1, m1 = pn(sa1)
        _chk(lib().nabwa_index_from_arrays(device, int(device_ptrs), p0, n0, p1, n1, s0, m0, s1, m1, C.byref(h)))
        return cls(h)

    def bwa_cal_sa_reg_gap(self, seqs, n_seqs, opt):
        """drop-in for bwa_cal_sa_reg_gap on an array of the reference's bwa_seq_t records (BwaSeq * n)"""
        _chk(lib().nabwa_bwa_cal_sa_reg_gap(self._h, n_seqs, seqs, C.byref(opt)))

    def attach_reference(self, prefix):
        """.ann/.amb/.pac of the index (reference bns_restore + bwt_restore_pac)"""
        _chk(lib().nabwa_index_attach_reference(self._h, prefix.encode()))

    def attach_nt_reference(self, prefix):
        """.nt.ann/.nt.amb/.nt.pac of a colour index (reference bwa_open_nt + bwt_restore_pac); the bases go to HBM"""
        _chk(lib().nabwa_index_attach_nt_reference(self._h, prefix.encode()))

    def se_finish_cs(self, opt, seq, rseq, qual, off, full_len, hits, n_occ, rng_state):
        """se_finish for colour reads (nabwa_se_finish_cs); qual: the reads' qualities (+33, read order) at off[].
        Returns (array of SeRec, new rng state, nt_seq, nt_rseq, nt_qual): the decoded read of a mapped record i is the first
        recs[i].len bytes at off[i] -- reversed, its reverse complement, its qualities + 33 in read order."""
        n = len(off) - 1
        n_aln = np.array([len(h) for h in hits], np.int32)
        rows = np.ascontiguousarray(np.concatenate([np.asarray(h, ALN_DT) for h in hits] + [np.zeros(0, ALN_DT)]))
        out = (SeRec * max(n, 1))()
        st = C.c_uint64(rng_state)
        off = np.ascontiguousarray(off, np.int64)
        side = [np.zeros(max(int(off[-1]), 1), np.uint8) for _ in range(3)]
        _chk(lib().nabwa_se_finish_cs(self._h, C.byref(opt), n, _ptr(off), _ptr(np.ascontiguousarray(seq, np.uint8)),
                                      _ptr(np.ascontiguousarray(rseq, np.uint8)), _ptr(np.ascontiguousarray(qual, np.uint8)),
                                      _ptr(np.ascontiguousarray(full_len, np.int32)), _ptr(n_aln), _ptr(rows), int(n_occ), C.byref(st), out,
                                      _ptr(side[0]), _ptr(side[1]), _ptr(side[2]), None))
        return (out, st.value) + tuple(side)

    def pe_finish_sampe_cs(self, opt, popt, ii, seq, rseq, qual, off, n_aln, rows, recs, cache=None):
        """nabwa_pe_finish_sampe_cs on flat arrays; recs (from pe_posn_flat) are updated in place.
        Returns (cnt_chg, nt_seq, nt_rseq, nt_qual) as se_finish_cs, index 2 * pair + end."""
        off = np.ascontiguousarray(off, np.int64)
        n = len(off) - 1
        side = [np.zeros(max(int(off[-1]), 1), np.uint8) for _ in range(3)]
        chg = C.c_int()
        _chk(lib().nabwa_pe_finish_sampe_cs(self._h, C.byref(opt), C.byref(popt), C.byref(ii), n // 2, _ptr(off),
                                            _ptr(np.ascontiguousarray(seq, np.uint8)), _ptr(np.ascontiguousarray(rseq, np.uint8)),
                                            _ptr(np.ascontiguousarray(qual, np.uint8)), _ptr(np.ascontiguousarray(n_aln, np.int32)),
                                            _ptr(np.ascontiguousarray(rows)), recs, cache, C.byref(chg), _ptr(side[0]), _ptr(side[1]), _ptr(side[2]), None))
        return (chg.value,) + tuple(side)

    def set_reference(self, l_pac, seed, pac, n_contigs=16, name="synth"):
        """nabwa_index_set_reference: n_contigs equal contigs "synth1".. over the reference (a contig's length is an int32 in the
        reference's bntann1_t), no ambiguity holes, .pac bytes from memory.  Returns the contig (names, offsets, lengths)."""
        L = lib()
        L.nabwa_index_set_reference.argtypes = [_P, C.c_int64, C.c_uint32, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, _P]
        offs = np.array([l_pac * i // n_contigs for i in range(n_contigs)], np.int64)
        lens = np.diff(np.append(offs, l_pac)).astype(np.int32)
        nm = ["%s%d" % (name, i + 1) for i in range(n_contigs)]
        names = (C.c_char_p * n_contigs)(*[x.encode() for x in nm])
        pac = np.ascontiguousarray(pac, np.uint8)
        _chk(L.nabwa_index_set_reference(self._h, int(l_pac), int(seed), n_contigs, names, _ptr(offs), _ptr(lens), 0, None, None, None, _ptr(pac)))
        return nm, offs, lens

    def pe_posn_flat(self, opt, off, full_len, n_aln, rows, rng_state, out=None):
        """nabwa_pe_posn on flat arrays (n_aln per read, rows back to back) -> (PeRec array, new rng state)"""
        n = len(off) - 1
        if out is None:
            out = (PeRec * max(n, 1))()
        st = C.c_uint64(rng_state)
        _chk(lib().nabwa_pe_posn(self._h, C.byref(opt), n // 2, _ptr(np.ascontiguousarray(off, np.int64)), _ptr(np.ascontiguousarray(full_len, np.int32)),
                                 _ptr(np.ascontiguousarray(n_aln, np.int32)), _ptr(np.ascontiguousarray(rows)), C.byref(st), out))
        return out, st.value

    def pe_finish_flat(self, opt, popt, ii, seq, rseq, off, n_aln, rows, recs):
        """nabwa_pe_finish on flat arrays; recs (from pe_posn_flat) are updated in place -> (n_tot, n_mapped)"""
        n = len(off) - 1
        tot, mp = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        _chk(lib().nabwa_pe_finish(self._h, C.byref(opt), C.byref(popt), C.byref(ii), n // 2, _ptr(np.ascontiguousarray(off, np.int64)),
                                   _ptr(np.ascontiguousarray(seq, np.uint8)), _ptr(np.ascontiguousarray(rseq, np.uint8)),
                                   _ptr(np.ascontiguousarray(n_aln, np.int32)), _ptr(np.ascontiguousarray(rows)), recs, tot, mp))
        return list(tot), list(mp)

    def se_finish(self, opt, seq, rseq, off, full_len, hits, n_occ, rng_state):
        """aln2seq + positions + mapQ + gap refinement + MD/NM for a batch, in record order.
        hits: per-read arrays of bwt_aln1_t rows.  Returns (array of SeRec, new rng state)."""
        n = len(off) - 1
        n_aln = np.array([len(h) for h in hits], np.int32)
        rows = np.concatenate([np.asarray(h, ALN_DT) for h in hits] + [np.zeros(0, ALN_DT)]) if n else np.zeros(0, ALN_DT)
        rows = np.ascontiguousarray(rows)
        out = (SeRec * max(n, 1))()
        st = C.c_uint64(rng_state)
        fl = np.ascontiguousarray(full_len, np.int32)
        _chk(lib().nabwa_se_finish(self._h, C.byref(opt), n, _ptr(np.ascontiguousarray(off, np.int64)),
                                   _ptr(np.ascontiguousarray(seq, np.uint8)), _ptr(np.ascontiguousarray(rseq, np.uint8)),
                                   _ptr(fl), _ptr(n_aln), _ptr(rows), n_occ, C.byref(st), out))
        return out, st.value

    def pe_posn(self, opt, off, full_len, hits, rng_state):
        """posn_pair (reference bam2bam.c:683-703) for interleaved ends (index 2*pair + end), in record order.
        Returns (array of PeRec, new rng state)."""
        n = len(off) - 1
        assert n % 2 == 0
        n_aln = np.array([len(h) for h in hits], np.int32)
        rows = np.ascontiguousarray(np.concatenate([np.asarray(h, ALN_DT) for h in hits] + [np.zeros(0, ALN_DT)]))
        out = (PeRec * max(n, 1))()
        st = C.c_uint64(rng_state)
        fl = np.ascontiguousarray(full_len, np.int32)
        _chk(lib().nabwa_pe_posn(self._h, C.byref(opt), n // 2, _ptr(np.ascontiguousarray(off, np.int64)), _ptr(fl), _ptr(n_aln),
                                 _ptr(rows), C.byref(st), out))
        return out, st.value

    def pe_finish(self, opt, popt, ii, seq, rseq, off, hits, recs):
        """finish_pair (reference bam2bam.c:705-811) on the records pe_posn returned (updated in place).
        Returns (n_tot, n_mapped) of the mate rescue."""
        n = len(off) - 1
        n_aln = np.array([len(h) for h in hits], np.int32)
        rows = np.ascontiguousarray(np.concatenate([np.asarray(h, ALN_DT) for h in hits] + [np.zeros(0, ALN_DT)]))
        tot = (C.c_uint64 * 2)()
        mp = (C.c_uint64 * 2)()
        _chk(lib().nabwa_pe_finish(self._h, C.byref(opt), C.byref(popt), C.byref(ii), n // 2, _ptr(np.ascontiguousarray(off, np.int64)),
                                   _ptr(np.ascontiguousarray(seq, np.uint8)), _ptr(np.ascontiguousarray(rseq, np.uint8)),
                                   _ptr(n_aln), _ptr(rows), recs, tot, mp))
        return list(tot), list(mp)

    def refine_gapped_core(self, qry, qry_off, ext, pos, is_end_correct=True, which_ref=0, max_cigar=MAX_CIGAR):
        """refine_gapped_core (reference bwase.c:189-237) for a batch of queries in alignment orientation, on the device
        (nabwa_refine_gapped_core).  Returns (new positions, list of bwa_cigar_t arrays)."""
        n = len(qry_off) - 1
        qry = np.ascontiguousarray(qry, np.uint8)
        qry_off = np.ascontiguousarray(qry_off, np.int64)
        ext = np.ascontiguousarray(ext, np.int32)
        pos = np.array(pos, np.uint32)
        ncig = np.zeros(max(n, 1), np.int32)
        cig = np.zeros((max(n, 1), max_cigar), np.uint16)
        _chk(lib().nabwa_refine_gapped_core(self._h, which_ref, 1 if is_end_correct else 0, n, _ptr(qry_off), _ptr(qry), _ptr(ext), _ptr(pos),
                                            _ptr(ncig), _ptr(cig), max_cigar))
        return pos[:n], [cig[i, :ncig[i]].copy() for i in range(n)]

    def cal_md(self, qry, qry_off, pos, cigars, which_ref=0, md_cap=None):
        """bwa_cal_md1 (reference bwase.c:253-315) for a batch of queries in alignment orientation, on the device (nabwa_cal_md).
        cigars: per-record bwa_cigar_t arrays, an empty one for the ungapped branch.  md_cap None: sized by a first call.
        Returns (NM array, list of MD strings)."""
        n = len(qry_off) - 1
        qry = np.ascontiguousarray(qry, np.uint8)
        qry_off = np.ascontiguousarray(qry_off, np.int64)
        pos = np.ascontiguousarray(pos, np.uint32)
        width = max([len(c) for c in cigars] + [1])
        ncig = np.array([len(c) for c in cigars], np.int32)
        cig = np.zeros((max(n, 1), width), np.uint16)
        for i, c in enumerate(cigars):
            cig[i, :len(c)] = c
        nm = np.zeros(max(n, 1), np.int32)
        off = np.zeros(n + 1, np.int64)

        def call(cap):
            md = np.zeros(max(cap, 1), np.uint8)
            rc = lib().nabwa_cal_md(self._h, which_ref, n, _ptr(qry_off), _ptr(qry), _ptr(pos), _ptr(ncig), _ptr(cig), width, _ptr(nm),
                                    _ptr(off), _ptr(md), cap)
            return rc, md
        rc, md = call(0 if md_cap is None else md_cap)
        if rc == ECAP and md_cap is None:
            rc, md = call(int(off[n]))
        _chk(rc)
        raw = md.tobytes()
        return nm[:n], [raw[off[i]:off[i + 1] - 1].decode() for i in range(n)]

    def export(self, which, what, first, n):
        """derived index parts for tests (nabwa_index_export): 0 full SA, 1 inverse SA, 2 text bases, 3 interval table, 4 its depth,
        5 the primary keys of its levels first.. (levels 0..16)"""
        out = np.zeros(int(n) * (2 if what == 3 else 1), np.uint32)
        _chk(lib().nabwa_index_export(self._h, int(which), int(what), int(first), int(n), _ptr(out)))
        return out.reshape(-1, 2) if what == 3 else out

    def seq_len(self, which=0):
        return lib().nabwa_index_seq_len(self._h, which)

    def device_bytes(self):
        return lib().nabwa_index_device_bytes(self._h)

    def dedup_cache_stats(self):
        """the index's read cache (NABWA_DEDUP_CACHE): [device bytes reserved, bytes of the entries written, entries, table slots, reads looked up,
        reads served, times emptied for another option block, batches that went without it] (nabwa_index_dedup_cache_stats); all 0 without one"""
        out = (C.c_uint64 * 8)()
        _chk(lib().nabwa_index_dedup_cache_stats(self._h, out))
        return [int(x) for x in out]

    def dedup_cache_clear(self):
        """empty the read cache (nabwa_index_dedup_cache_clear); NabwaError EINVAL while a live batch holds reads served from it"""
        _chk(lib().nabwa_index_dedup_cache_clear(self._h))

    def close(self):
        if self._h:
            lib().nabwa_index_destroy(self._h)
            self._h = None

    def sa_lookup(self, which, k):
        """bwt_sa (reference bwt.c:72-81) for many rows."""
        which = np.ascontiguousarray(which, np.uint8)
        k = np.ascontiguousarray(k, np.uint32)
        out = np.zeros(len(k), np.uint32)
        _chk(lib().nabwa_sa_lookup(self._h, len(k), _ptr(which), _ptr(k), _ptr(out)))
        return out

    def occ4(self, which, k):
        """bwt_occ4 (reference bwt.c:159-176) for many rows."""
        k = np.ascontiguousarray(k, np.uint32)
        out = np.zeros((len(k), 4), np.uint32)
        _chk(lib().nabwa_occ4(self._h, which, len(k), _ptr(k), _ptr(out)))
        return out

    def cal_sa_reg_gap_flat(self, opt, seq, rseq, off, per_read=False, cap_rows=None):
        """The C one-shot entry (nabwa_cal_sa_reg_gap) on host buffers, results as flat arrays:
        (n_aln int32[n], rows ALN_DT[total], max_entries int32[n]) -- what a C caller of the boundary gets."""
        n = len(off) - 1
        seq = np.ascontiguousarray(seq, np.uint8); rseq = np.ascontiguousarray(rseq, np.uint8)
        off = np.ascontiguousarray(off, np.int64)
        n_aln = np.empty(max(n, 1), np.int32); maxe = np.empty(max(n, 1), np.int32)
        cap = int(cap_rows if cap_rows is not None else n + n // 8 + 1024)
        while True:
            buf = np.empty(max(cap, 1), ALN_DT)
            rows = C.c_int64()
            rc = lib().nabwa_cal_sa_reg_gap(self._h, C.byref(opt), n, _ptr(off), _ptr(seq), _ptr(rseq), int(per_read),
                                            _ptr(n_aln), _ptr(buf), cap, C.byref(rows), _ptr(maxe))
            if rc == ECAP and rows.value > cap:
                cap = rows.value
                continue
            _chk(rc)
            return n_aln[:n], buf[:rows.value], maxe[:n]

    def cal_sa_reg_gap(self, opt, seq, rseq, off, per_read=False):
        """bwa_cal_sa_reg_gap (reference bwtaln.c:93-142) over a flat batch.
        Returns (list of per-read hit arrays, max_entries)."""
        b = Batch(self, opt, seq, rseq, off, per_read)
        try:
            b.run()
            b.sync()
            return b.fetch()
        finally:
            b.close()


class Batch:
    """Device-resident batch of reads: upload once, run the FM search many times."""

    def __init__(self, index, opt, seq, rseq, off, per_read=False):
        self.n = len(off) - 1
        self._seq = np.ascontiguousarray(seq, np.uint8)
        self._rseq = np.ascontiguousarray(rseq, np.uint8)
        self._off = np.ascontiguousarray(off, np.int64)
        self._h = _P()
        _chk(lib().nabwa_batch_create(index._h, C.byref(opt), self.n, _ptr(self._off), _ptr(self._seq),
                                      _ptr(self._rseq), int(per_read), C.byref(self._h)))

    def run(self):
        _chk(lib().nabwa_batch_run(self._h))

    def sync(self):
        n2 = C.c_int()
        _chk(lib().nabwa_batch_sync(self._h, C.byref(n2)))
        return n2.value

    def last_kernel_ms(self):
        return float(lib().nabwa_batch_last_kernel_ms(self._h))

    def last_width_ms(self):
        return float(lib().nabwa_batch_last_width_ms(self._h))

    def last_deep_ms(self):
        """HIP-event time of kernel D (the deep searches the first pass handed on) in the most recent run; 0 if it did not run"""
        return float(lib().nabwa_batch_last_deep_ms(self._h))

    def checksum(self):
        s = C.c_uint64()
        r = C.c_int64()
        _chk(lib().nabwa_batch_checksum(self._h, C.byref(s), C.byref(r)))
        return s.value, r.value

    def count_touches(self):
        """Occ-bucket touches of the reference algorithm on this batch (untimed instrumented run)."""
        v, w = C.c_uint64(), C.c_uint64()
        _chk(lib().nabwa_batch_count_touches(self._h, C.byref(v), C.byref(w)))
        return v.value, w.value   # (search kernel, width kernel)

    def fetch(self):
        n_aln = np.zeros(max(self.n, 1), np.int32)
        maxe = np.zeros(max(self.n, 1), np.int32)
        rows = C.c_int64()
        rc = lib().nabwa_batch_fetch(self._h, _ptr(n_aln), None, 0, C.byref(rows), _ptr(maxe))
        if rc not in (OK, ECAP):
            _chk(rc)
        buf = np.zeros(max(rows.value, 1), ALN_DT)
        if rows.value:
            _chk(lib().nabwa_batch_fetch(self._h, _ptr(n_aln), _ptr(buf), rows.value, C.byref(rows), _ptr(maxe)))
        n_aln = n_aln[:self.n]
        bounds = np.concatenate([[0], np.cumsum(n_aln)])
        return [buf[bounds[i]:bounds[i + 1]] for i in range(self.n)], maxe[:self.n]

    def fetch_flat(self, keep=None):
        """-> (n_aln per read, all rows back to back, max_entries per read).  keep: a dict the caller holds from batch to batch -- the three
        arrays live in it and are used again (a streaming caller's buffers: no fresh pages per batch, one fetch where the rows fit)"""
        if keep is not None and "n_aln" in keep and len(keep["n_aln"]) >= max(self.n, 1):
            n_aln, maxe, buf = keep["n_aln"], keep["maxe"], keep["rows"]
        else:
            n_aln = np.zeros(max(self.n, 1), np.int32)
            maxe = np.zeros(max(self.n, 1), np.int32)
            buf = None
        rows = C.c_int64()
        rc = lib().nabwa_batch_fetch(self._h, _ptr(n_aln), _ptr(buf) if buf is not None else None, len(buf) if buf is not None else 0, C.byref(rows), _ptr(maxe))
        if rc not in (OK, ECAP):
            _chk(rc)
        if rc == ECAP or buf is None:
            buf = np.zeros(max(rows.value + rows.value // 8, 1), ALN_DT)
            if rows.value:
                _chk(lib().nabwa_batch_fetch(self._h, _ptr(n_aln), _ptr(buf), len(buf), C.byref(rows), _ptr(maxe)))
        if keep is not None:
            keep["n_aln"], keep["maxe"], keep["rows"] = n_aln, maxe, buf
        return n_aln[:self.n], buf[:rows.value], maxe[:self.n]

    def config(self):
        """the batch's derived configuration as a dict (nabwa_batch_config); -1: not decided yet"""
        c = BatchConfig()
        _chk(lib().nabwa_batch_config(self._h, C.byref(c)))
        return {f: (list(getattr(c, f)) if f == "cls" else getattr(c, f)) for f, _ in BatchConfig._fields_}

    def sure0_stats(self):
        """NABWA_SURE0_STATS=1: [reads that took kernel S's exact-occurrence shortcut, children resolved as dead, children stored
        landed, reads its safety net handed to kernel D] over the runs so far (nabwa_batch_sure0_stats); all 0 without the variable"""
        out = (C.c_uint64 * 4)()
        _chk(lib().nabwa_batch_sure0_stats(self._h, out))
        return [int(x) for x in out]

    def sure0_stats_ex(self):
        """sure0_stats()'s four values, then [leaps taken, levels leapt over, proven entries that walked instead (expected 0), 0]
        (nabwa_batch_sure0_stats_ex; NABWA_SURE0=3)"""
        out = (C.c_uint64 * 8)()
        _chk(lib().nabwa_batch_sure0_stats_ex(self._h, out))
        return [int(x) for x in out]

    def dedup_stats(self):
        """[reads given, reads searched, reads whose hash met that of an earlier read they differ from, 1 if the batch was created with
        NABWA_DEDUP=1 else 0] (nabwa_batch_dedup_stats); without the switch [n, n, 0, 0]"""
        out = (C.c_uint64 * 4)()
        _chk(lib().nabwa_batch_dedup_stats(self._h, out))
        return [int(x) for x in out]

    def dedup_stats_ex(self):
        """dedup_stats()'s four values, then what NABWA_DEDUP_CACHE did: [distinct reads served from the index's read cache, reads entered into
        it, reads not entered (cache full, over the row cap), 1 if the batch went without the cache] (nabwa_batch_dedup_stats_ex)"""
        out = (C.c_uint64 * 8)()
        _chk(lib().nabwa_batch_dedup_stats_ex(self._h, out))
        return [int(x) for x in out]

    def close(self):
        if self._h:
            lib().nabwa_batch_destroy(self._h)
            self._h = None
