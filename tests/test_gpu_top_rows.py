"""Search, SA lookup and the size limits at the top of the 32-bit row range, on the GPU.

Two texts are built on the device (synth.synth_text plus planted stretches: poly-T and poly-A runs, a tandem repeat, stretches within
the first and last 10 kb): 0xfffffefe bases, the largest whose searches keep key form, and 0xffffffdf, the largest the loader accepts,
where the rows reach kernel D's key-form marker (DEEP_KEYL, fm_deep.hpp) and the search runs without it.  At each size:
  1. occ4 on the last three buckets, primary +- 200, 2^31 +- 200 and random rows = counts of the .bwt words in int64 = the oracle's;
  2. sa_lookup (text mode on and off) on the same rows: SA[LF(r)] = SA[r] - 1 with LF from the int64 counts, the sampled rows' values
     from the .sa words, the inverse SA, the BWT base = text[SA - 1], suffix order over 64-base windows, and the text's last 4096 bases;
  3. cal_sa_reg_gap rows and max_entries = the oracle's (and the compiled reference's, on the same arrays written as its files, when it
     travelled), for reads cut at the top rows, around row 2^31 and the primary, at the text's ends, from the planted stretches and
     synth_reads (16 000, 1 % substitutions, an indel in 15 %), default and ancient-DNA options, every search through kernel D
     (NABWA_CAP1=48); at 0xfffffefe also with key form off and with the text kernels off;
  4. reads at the text's ends and around text position 2^31 (contig borders and holes on both sides of it) through se_finish,
     field by field against the compiled reference's chain on the same files (where the compiled reference travelled).
The refusals above the limits are checked cheaply: a hand-written .pac through nabwa_index_build and a header through from_arrays."""
import ctypes as C
import importlib
import os
import shutil
import time

import numpy as np
import pytest

import bigindex as BI
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
synth = importlib.import_module("network-aware-bwa_amd.synth")
pytestmark = pytest.mark.gpu

SIZES = [0xfffffefe, 0xffffffdf]
TMP_NEED = 12 << 30            # the reference's files of one size (5.0 GiB measured), with room; needed where the compiled reference is there


def dev_need(n):
    """device bytes the test needs at its peak, the reverse index's build: the builder holds 41 B per row at once (64-bit keys and
    32-bit values double-buffered, rank, group start, head, slots, tied flag: synth_index.hip), beside the 1-byte-per-base text and
    the forward index's words (4.5 bits per base); 12 GiB on top for the radix sort's scratch and the runtime.  The loaded index
    (text mode, T = 14) needs less: about 75 GiB."""
    return 41 * (n + 1) + n + (n * 9 + 7) // 16 + (12 << 30)


class PeakWatch:
    """the lowest free device memory seen while a block runs (polled from a thread: the library's calls release the GIL)"""

    def __init__(self, low):
        self.low = low

    def __enter__(self):
        import threading
        self.stop = threading.Event()

        def poll():
            while not self.stop.wait(0.01):
                self.low.append(dev_free()[0])
        self.th = threading.Thread(target=poll, daemon=True)
        self.th.start()
        return self

    def __exit__(self, *a):
        self.stop.set()
        self.th.join()
        self.low.append(dev_free()[0])


_HIP = []


def dev_free():
    """hipMemGetInfo of device 0, from the HIP runtime libnabwa itself loaded"""
    if not _HIP:
        nabwa.lib()
        _HIP.append(C.CDLL(next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)))
    hip = _HIP[0]
    f, t = C.c_size_t(), C.c_size_t()
    assert hip.hipSetDevice(0) == 0 and hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
    return f.value, t.value


def host_counts(words, k):
    """bwt_occ4 (bwt.c:159-176) of the .bwt words in int64: the checkpoint of the 128-row block, then the bases up to k"""
    prim, body = int(words[0]), words[5:]
    k = np.asarray(k, np.int64)
    out = np.zeros((len(k), 4), np.int64)
    ok = k >= 0
    kk = np.where(k[ok] >= prim, k[ok] - 1, k[ok])
    p = (kk >> 7) * 12
    cnt = body[p[:, None] + np.arange(4)].astype(np.int64)
    bw = body[p[:, None] + 4 + np.arange(8)].astype(np.int64)                              # 8 words x 16 bases, first base in the top bits
    bases = (bw[:, :, None] >> ((15 - np.arange(16)) * 2)) & 3
    bases = bases.reshape(len(kk), 128)
    take = np.arange(128)[None, :] <= (kk & 127)[:, None]
    for c in range(4):
        cnt[:, c] += ((bases == c) & take).sum(1)
    out[ok] = cnt
    return out


def host_base(words, r):
    """the BWT base of row r (r != primary)"""
    prim, body = int(words[0]), words[5:]
    r = np.asarray(r, np.int64)
    rr = np.where(r > prim, r - 1, r)
    w = body[(rr >> 7) * 12 + 4 + ((rr & 127) >> 4)].astype(np.int64)
    return (w >> ((15 - (rr & 15)) * 2)) & 3


def plant(d_text, n, rng):
    """poly-T / poly-A runs, a tandem repeat and stretches at both ends, written into the device text -> [(pos, length)] of the stretches"""
    unit = rng.integers(0, 4, 37).astype(np.uint8)
    stretches = [
        (50, np.full(400, 3, np.uint8)), (3000, np.tile(unit, 30)), (n - 9000, np.full(350, 0, np.uint8)), (n - 600, np.full(320, 3, np.uint8)),
        (1_000_000_007, np.full(600, 3, np.uint8)), (2**31 - 500, np.full(700, 0, np.uint8)), (3_000_000_011, np.tile(unit, 60)),
        (n - 2_000_000, np.full(512, 3, np.uint8)),
    ]
    for p, s in stretches:
        synth._chk(synth.lib().nabwa_synth_h2d(C.c_void_p(d_text.ptr + p), s.ctypes.data_as(C.c_void_p), s.nbytes))
    return [(p, len(s)) for p, s in stretches]


def encode(text, starts, lengths, rng, noisy, strands=None):
    """reads from the text, of the other strand where strands[i] (default: every second one); a few with a substitution -> (seq, rseq, off)"""
    reads = []
    for i, (p, L) in enumerate(zip(starts, lengths)):
        r = text[p:p + L].copy()
        if noisy and i % 4 == 1 and L > 20:
            r[int(rng.integers(5, L - 5))] ^= 1
        if (strands[i] if strands is not None else i % 2):
            r = (3 - r)[::-1]
        reads.append(r)
    seq = np.concatenate([r[::-1] for r in reads]).astype(np.uint8)                        # bwa_seq_t.seq: the read reversed
    rseq = (3 - seq).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return seq, rseq, off


def as_gap(opt):
    g = nabwa.GapOpt()
    C.memmove(C.byref(g), C.byref(opt), 64)
    return g


def same_rows(got, want, what):
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, "%s: %d of %d reads differ, e.g. %d: %s vs %s" % (what, len(bad), len(want), bad[0], got[bad[0]][:3], want[bad[0]][:3])


def test_refusals_above_the_limits(tmp_path, monkeypatch):
    """a .pac of 0xffffff81 bases: EINVAL, nothing written; 0xffffff80 passes the size check (ENOMEM under a tiny budget);
    a header claiming 0xffffffe0 bases: EINVAL from the loader.  The .pac files are sparse: only their last bytes are written."""
    for n in (0xffffff81, 0xffffff80):
        pre = str(tmp_path / ("t%x" % n))
        with open(pre + ".pac", "wb") as f:               # n // 4 + 1 packed bytes (all zero here, sparse), then n % 4 (bntseq.c:240-250)
            f.truncate(n // 4 + 1)
            f.seek(0, 2)
            f.write(bytes([n % 4]))
        sz = os.path.getsize(pre + ".pac")
        assert (sz - 2) * 4 + n % 4 == n
        monkeypatch.setenv("NABWA_INDEX_MAX_BYTES", str(1 << 20))
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.index_build(pre, 0)
        want = "EINVAL" if n > 0xffffff80 else "ENOMEM"
        assert e.value.code == {"EINVAL": -2, "ENOMEM": -4}[want], (hex(n), str(e.value))
        if want == "EINVAL":
            assert "bwtmisc.c:131" in str(e.value), str(e.value)
        assert sorted(os.listdir(tmp_path)) == sorted(x for x in os.listdir(tmp_path) if x.endswith(".pac")), os.listdir(tmp_path)
    hdr = np.zeros(64, np.uint32)
    hdr[:5] = [1, 0x40000000, 0x80000000, 0xc0000000, 0xffffffe0]
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.Index.from_arrays(hdr, hdr)
    assert e.value.code == -2 and "bwtio.c:175" in str(e.value), str(e.value)


@pytest.mark.parametrize("n", SIZES, ids=[hex(n) for n in SIZES])
def test_top_rows(n, monkeypatch):
    free, total = dev_free()
    if free < dev_need(n):
        pytest.skip("device memory: %.1f GiB free, %.1f GiB needed" % (free / 2**30, dev_need(n) / 2**30))
    ref = T.load_ref()
    root = os.environ.get("NABWA_TEST_TMP", "/tmp")
    if ref is not None and shutil.disk_usage(root).free < TMP_NEED:
        pytest.skip("%s: %.1f GiB free, %.1f GiB needed for the reference's files" % (root, shutil.disk_usage(root).free / 2**30, TMP_NEED / 2**30))
    t0 = time.time()
    low = [free]
    rng = np.random.default_rng(n & 0xffff)
    parts, ix, ox, rix, prefix = [], None, None, None, None
    olib = T.load_oracle()
    try:
        d_text = synth.synth_text(n, 20261015 + (n & 0xff), device=0)
        parts.append(d_text)
        stretches = plant(d_text, n, rng)
        text = d_text.to_host(np.uint8)
        with PeakWatch(low):
            for rev in (0, 1):
                bw, nbw, sa, nsa = synth.build_index(d_text, n, rev, 32, True, device=0)
                parts += [bw, sa]
                parts.append((bw, nbw, sa, nsa))
        built = [x for x in parts if isinstance(x, tuple)]
        words = [bw.to_host(np.uint32, nbw) for bw, nbw, _, _ in built]
        sa_words = [sa.to_host(np.uint32, nsa) for _, _, sa, nsa in built]
        seq_s, rseq_s, off_s = synth.synth_reads(d_text, n, 16000, 100, 10000, 150000, 5, device=0)      # 1 % substitutions, an indel in 15 % of the reads
        if ref is not None:
            prefix = os.path.join(root, "nabwa_top%x_%d" % (n, os.getpid()), "top")
            os.makedirs(os.path.dirname(prefix), exist_ok=True)
            for t in (0, 1):
                words[t].tofile(prefix + (".rbwt" if t else ".bwt"))
                sa_words[t].tofile(prefix + (".rsa" if t else ".sa"))
            BI.write_pac(prefix, BI.pack_pac(d_text, n), n)
            # contigs under 2^31 bases that end and start on both sides of 2^31 (one of 100 bases across it), holes around it and at the ends
            BI.write_ann_amb(prefix, n, None, cuts=[1_100_000_000, 2**31 - 40, 2**31 + 60, 3_300_000_000],
                             holes=[(2000, 30), (2**31 - 3000, 40), (2**31 + 500, 30), (2**31 + 5000, 10), (n - 5000, 25)])
        d_text.free()
        ox = olib.orc_index_wrap(T.ptr(words[0]), len(words[0]), T.ptr(words[1]), len(words[1]))
        monkeypatch.setenv("NABWA_KMER_T", "14")
        monkeypatch.delenv("NABWA_TEXT_MODE", raising=False)
        with PeakWatch(low):
            ix = nabwa.Index.from_arrays((built[0][0].ptr, built[0][1]), (built[1][0].ptr, built[1][1]), (built[0][2].ptr, built[0][3]),
                                         (built[1][2].ptr, built[1][3]), device=0, device_ptrs=True)
        for x in parts:
            if not isinstance(x, tuple):
                x.free()
        low.append(dev_free()[0])
        loaded_low = low[-1]
        assert ix.seq_len(0) == n and ix.seq_len(1) == n
        assert int(ix.export(0, 4, 0, 1)[0]) == 14 and int(ix.export(1, 4, 0, 1)[0]) == 14
        if ref is not None:
            ref.ref_index_load.restype = C.c_void_p
            ref.ref_index_load.argtypes = [C.c_char_p, C.c_int]
            rix = C.c_void_p(ref.ref_index_load(prefix.encode(), 1))
            ref.ref_occ4.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
            ref.ref_cal_sa_reg_gap_mt.restype = C.c_long
            ref.ref_cal_sa_reg_gap_mt.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
        prim = int(words[0][0])
        # ---- 1. occ4
        rows = np.unique(np.concatenate([np.arange(n - 3 * 192 + 1, n + 1), np.arange(prim - 200, prim + 201), np.arange(2**31 - 200, 2**31 + 201),
                                         rng.integers(0, n + 1, 10000)]))
        rows = rows[(rows >= 1) & (rows <= n)]                 # (row 0, the empty suffix, has no SA value: -1 in the reference)
        for t in (0, 1):
            want = host_counts(words[t], rows)
            got = ix.occ4(t, rows.astype(np.uint32)).astype(np.int64)
            bad = np.nonzero((got != want).any(1))[0]
            assert len(bad) == 0, (hex(n), t, [(int(rows[i]), got[i].tolist(), want[i].tolist()) for i in bad[:3]])
            cnt = np.zeros(4, np.uint32)
            for i in range(0, len(rows), 7):
                olib.orc_occ4(C.c_void_p(ox + t * T.OracleIndex.BWT_SIZE), int(rows[i]), T.ptr(cnt))
                assert cnt.tolist() == want[i].tolist(), (hex(n), t, int(rows[i]))
                if rix is not None:
                    ref.ref_occ4(rix, t, int(rows[i]), T.ptr(cnt))
                    assert cnt.tolist() == want[i].tolist(), (hex(n), t, int(rows[i]), "reference")
        # ---- 2. sa_lookup, text mode on, then (second index below) off
        L2 = [np.array([0] + [int(x) for x in words[t][1:5]], np.int64) for t in (0, 1)]
        sa_on = [ix.sa_lookup(np.full(len(rows), t, np.uint8), rows).astype(np.int64) for t in (0, 1)]
        for t in (0, 1):
            sa = sa_on[t]
            assert sa.max() <= n
            samp = rows % 32 == 0
            idx = rows[samp] // 32
            sw = sa_words[t][7:].astype(np.int64)
            assert (sa[samp] == sw[idx - 1]).all()
            nz = rows != prim
            c = host_base(words[t], rows[nz])
            lf = L2[t][c] + host_counts(words[t], rows[nz])[np.arange(nz.sum()), c]
            sa_lf = ix.sa_lookup(np.full(len(lf), t, np.uint8), lf.astype(np.uint32)).astype(np.int64)
            assert (sa_lf == sa[nz] - 1).all(), hex(n)
            isa = np.array([int(ix.export(t, 1, int(v), 1)[0]) for v in sa[:: 97]], np.int64)
            assert (isa == rows[:: 97]).all()
            if rix is not None:
                sa_ref = np.array([ref.ref_sa(rix, t, int(r)) for r in rows[:: 13]], np.int64)
                assert (sa_ref == sa[:: 13]).all(), (hex(n), t)
            if t == 0:
                assert (c == text[sa[nz] - 1]).all()
                st = sa_on[0][rows > n - 300]
                win = [bytes(text[s:s + 64]) for s in st]            # 64-base windows; a shorter suffix sorts first ($ is smallest), as bytes do
                assert all(win[i] <= win[i + 1] for i in range(len(win) - 1)), hex(n)
        assert (ix.export(0, 2, n - 4096, 4096) == text[n - 4096:]).all()
        # ---- 3. searches against the oracle and the reference
        sa_top = [int(v) for v in ix.export(0, 0, n - 300, 301)]
        sa_mid = [int(v) for v in ix.export(0, 0, 2**31 - 100, 201)]
        sa_prim = [int(v) for v in ix.export(0, 0, prim - 32, 65)]
        starts, lens = [], []
        for k, p in enumerate(sa_top + sa_mid + sa_prim):
            L = [16, 20, 36, 50, 100][k % 5]
            if p + L <= n:
                starts.append(p); lens.append(L)
        for p in sa_mid[98:103]:                                 # short reads at rows 2^31 - 2 .. 2^31 + 2: intervals of ~100 rows across it
            for L in (12, 14):
                if p + L <= n:
                    starts.append(p); lens.append(L)
        for p, l in stretches:
            for j in range(0, l, 60):
                if p + j + 100 <= n:
                    starts.append(p + j); lens.append(100)
                if p + j + 32 <= n:
                    starts.append(max(0, p + j - 20)); lens.append(32)
        strands = [k % 2 for k in range(len(starts))]
        for L in (32, 36, 100, 150):                             # the text's first and last bases, each from both strands
            for p in (0, n - L):
                starts += [p, p]; lens += [L, L]; strands += [0, 1]
        seq, rseq, off = encode(text, starts, lens, rng, True, strands)
        ss = np.concatenate([seq, seq_s]); rs = np.concatenate([rseq, rseq_s]); oo = np.concatenate([off, off_s[1:] + off[-1]])
        opts = [("default", T.read_sai(os.path.join(T.GOLDEN, "se_default.sai"))[0]), ("adna", T.read_sai(os.path.join(T.GOLDEN, "se_adna.sai"))[0])]
        monkeypatch.setenv("NABWA_CAP1", "48")
        n_top = n_straddle = 0
        for name, opt in opts:
            want, wmaxe = T.oracle_cal_sa_reg_gap(olib, ox, opt, ss, rs, oo, n_threads=16)
            if rix is not None:
                na = np.zeros(len(oo) - 1, np.int32)
                flat = np.zeros(max(64 * len(na), 1 << 20), T.ALN_DT)
                tot = ref.ref_cal_sa_reg_gap_mt(rix, C.byref(opt), len(na), T.ptr(oo), T.ptr(ss), T.ptr(rs), 16, T.ptr(na), T.ptr(flat), len(flat))
                assert tot >= 0
                b = np.concatenate([[0], np.cumsum(na)])
                same_rows([flat[b[i]:b[i + 1]] for i in range(len(na))], want, "%s: the oracle vs the reference, %s" % (hex(n), name))
            variants = [("", {})] if n >= 0xffffff00 else [("", {}), ("key form off", {"NABWA_DEEP_KEYFORM": "0"}), ("text kernels off", {"NABWA_TEXT_KERNELS": "0"})]
            for vname, env in variants:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                bt = nabwa.Batch(ix, as_gap(opt), ss, rs, oo, per_read=False)
                bt.run()
                n_deep = bt.sync()
                got, maxe = bt.fetch()
                bt.close()
                for k in env:
                    monkeypatch.delenv(k)
                same_rows(got, want, "%s, %s options %s" % (hex(n), name, vname))
                assert (np.asarray(maxe)[:len(wmaxe)] == wmaxe).all(), (hex(n), name, vname)
                assert n_deep > 0, "no search reached kernel D"
            n_top += sum(int(x["l"]) >= 0xffffff00 for h in want for x in h)
            n_straddle += sum(int(x["k"]) < 2**31 <= int(x["l"]) for h in want for x in h)
        if n >= 0xffffff00:
            assert n_top > 0, "no hit reaches the marker's rows"
        assert n_straddle > 0, "no hit straddles row 2^31"
        monkeypatch.delenv("NABWA_CAP1")
        # ---- 4. the finishing chain against the reference on the same files: reads at the text's ends and around text position 2^31
        # (contig borders at 2^31 - 40 and 2^31 + 60, holes on both sides), both strands, every fourth with a substitution
        n_fin = 0
        if rix is not None:
            ix.attach_reference(prefix)
            fs = list(range(0, 51, 5)) + list(range(n - 150, n - 99, 5)) + list(range(2**31 - 3100, 2**31 + 600, 20)) + list(range(2**31 + 4900, 2**31 + 5000, 10))
            fs = [p for p in fs for _ in (0, 1)]
            f_seq, f_rseq, f_off = encode(text, fs, [100] * len(fs), rng, True, [k % 2 for k in range(len(fs))])
            n_map, n_hole, n_bridge, recs = BI.se_chain_vs_reference(ix, ref, rix, nabwa.gap_init_opt(), f_seq, f_rseq, f_off)
            n_fin = len(fs)
            assert n_map > 0.9 * n_fin and n_hole > 0 and n_bridge > 0, (n_map, n_hole, n_bridge, n_fin)
            assert any(recs[i].type and recs[i].pos >= 2**31 for i in range(n_fin)) and any(recs[i].type and recs[i].pos >= n - 150 for i in range(n_fin))
        ix.close(); ix = None
        # ---- 2 again with text mode off: sa_lookup walks LF from the samples
        monkeypatch.setenv("NABWA_TEXT_MODE", "0")
        ix = nabwa.Index.from_arrays(words[0], words[1], sa_words[0], sa_words[1], device=0)
        assert int(ix.export(0, 4, 0, 1)[0]) == 14 and int(ix.export(1, 4, 0, 1)[0]) == 14
        for t in (0, 1):
            got = ix.sa_lookup(np.full(len(rows), t, np.uint8), rows).astype(np.int64)
            assert (got == sa_on[t]).all(), (hex(n), t)
        files = sum(os.path.getsize(os.path.join(os.path.dirname(prefix), f)) for f in os.listdir(os.path.dirname(prefix))) if prefix else 0
        print("top rows %#x: device memory in use at the peak %.1f GiB (the builder; the loaded index %.1f GiB; checked against %.1f GiB), "
              "files %.1f GiB, %d reads searched, %d finished, %.0f s" % (
                  n, (free - min(low)) / 2**30, (free - loaded_low) / 2**30, dev_need(n) / 2**30, files / 2**30, len(oo) - 1, n_fin, time.time() - t0))
    finally:
        if ix is not None:
            ix.close()
        for x in parts:
            if not isinstance(x, tuple):
                x.free()
        if ox is not None:
            olib.orc_index_free(C.c_void_p(ox))
        if rix is not None:
            ref.ref_index_free(rix)
        if prefix:
            shutil.rmtree(os.path.dirname(prefix), ignore_errors=True)
