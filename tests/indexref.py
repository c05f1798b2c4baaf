"""A plain reference of the FM-index, NumPy only: no GPU, no product code, no oracle.

From a uint8 text of codes 0..3 (A C G T):
  suffix_array   the suffix array of text + '$', '$' smallest (prefix doubling with argsort), n + 1 rows
  bwt_words      the .bwt word stream (bwtio.c:184-204 read it back): primary, L2[1..4], then the '$'-less BWT 16 bases a word,
                 first base in the top bits, with the four running counts before every 8th word and once after the last
                 (bwtmisc.c:125-152)
  sa_words       the .sa word stream (bwtio.c:27-37, :161-182): primary, L2[1..4], sa_intv, n, then SA[intv], SA[2 intv], ...
  occ_table      the cumulative occ[k + 1][c] for rows k = -1..n with the reference's '$' convention (bwt.c:159-176)
  kmer_intervals the SA interval of every string of t symbols, from the sorted suffixes themselves
The reverse index is the same functions applied to text[::-1].  RefIndex holds all of it for one text.

Also the text makers and the edge-read generator of tests/test_gpu_index_geometry.py and tests/test_indexref_host.py.
tests/test_indexref_host.py pins all of this against the committed toy index, the compiled reference and the oracle."""
import numpy as np

# ------------------------------------------------------------------ the index


def suffix_array(text):
    """SA of text + '$' ('$' sorts first): SA[0] = n, n + 1 rows, int64"""
    text = np.asarray(text, np.int64)
    m = len(text) + 1
    rank = np.concatenate([text + 1, [0]])
    h = 1
    sa = np.argsort(rank, kind="stable")
    while True:
        nxt = np.zeros(m, np.int64)                        # rank of the suffix h further on; 0 (= '$', nothing there) past the end
        if h < m:
            nxt[:m - h] = rank[h:]
        key = rank * (m + 1) + nxt
        sa = np.argsort(key, kind="stable")
        ks = key[sa]
        new = np.concatenate([[0], np.cumsum(ks[1:] != ks[:-1])])
        rank = np.empty(m, np.int64)
        rank[sa] = new
        if new[-1] == m - 1:
            return sa
        h *= 2
        assert h < 2 * m


def bwt_column(text, sa):
    """the last column over the n + 1 rows: text[SA - 1], 4 at the row of the whole text (primary)"""
    text = np.asarray(text, np.int64)
    return np.where(sa == 0, 4, text[sa - 1])


def bwt_words(text, sa=None):
    text = np.asarray(text, np.uint8)
    n = len(text)
    sa = suffix_array(text) if sa is None else sa
    col = bwt_column(text, sa)
    primary = int(np.nonzero(sa == 0)[0][0])
    b0 = col[col != 4]                                     # the '$' row left out (is.c:210-215)
    nw = (n + 15) // 16
    pad = np.zeros(nw * 16, np.uint64)
    pad[:n] = b0
    packed = (pad.reshape(nw, 16) << ((15 - np.arange(16, dtype=np.uint64)) * np.uint64(2))).sum(1).astype(np.uint32)
    onehot = (b0[:, None] == np.arange(4)[None, :]).astype(np.int64)
    run = np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(onehot, 0)])       # run[j] = counts of b0[:j]
    out = []
    for blk in range((n + 127) // 128):
        out.append(run[blk * 128].astype(np.uint32))
        out.append(packed[blk * 8:blk * 8 + 8])
    out.append(run[n].astype(np.uint32))
    L2 = np.cumsum(np.bincount(text, minlength=4)[:4])
    return np.concatenate([np.array([primary] + [int(x) for x in L2], np.uint32)] + out).astype(np.uint32)


def sa_words(text, sa_intv, sa=None):
    text = np.asarray(text, np.uint8)
    n = len(text)
    sa = suffix_array(text) if sa is None else sa
    primary = int(np.nonzero(sa == 0)[0][0])
    L2 = np.cumsum(np.bincount(text, minlength=4)[:4])
    hdr = [primary] + [int(x) for x in L2] + [int(sa_intv), n]
    return np.concatenate([np.array(hdr, np.uint32), sa[sa_intv::sa_intv].astype(np.uint32)])


def occ_table(text, sa):
    """occ[k + 1] = bwt_occ4 of row k, k = -1..n: the bases of the last column in rows 0..k, the '$' of row primary not counted"""
    col = bwt_column(text, sa)
    onehot = (col[:, None] == np.arange(4)[None, :]).astype(np.int64)
    return np.concatenate([np.zeros((1, 4), np.int64), np.cumsum(onehot, 0)])


def kmer_intervals(text, sa, t):
    """(k, l) int64 arrays of 4^t entries: the rows whose suffix starts with the t symbols P; the entry of P is at
    sum(P[j] * 4^j) -- the backward search consumes P from its end, first consumed symbol most significant.  Empty: k > l (1, 0)."""
    text = np.asarray(text, np.int64)
    n = len(text)
    rows = np.nonzero(sa + t <= n)[0]                      # suffixes of t symbols and more, in suffix order: their codes ascend
    code_sorted = np.zeros(len(rows), np.int64)            # first symbol most significant: the order of the suffixes
    code_key = np.zeros(len(rows), np.int64)
    for j in range(t):
        sym = text[sa[rows] + j]
        code_sorted = code_sorted * 4 + sym
        code_key += sym << (2 * j)
    assert (np.diff(code_sorted) >= 0).all()
    k = np.ones(4 ** t, np.int64)
    l = np.zeros(4 ** t, np.int64)
    allc = np.arange(4 ** t, dtype=np.int64)
    lo = np.searchsorted(code_sorted, allc, "left")
    hi = np.searchsorted(code_sorted, allc, "right")
    have = hi > lo
    key_of = np.zeros(4 ** t, np.int64)                    # sorted-order code -> table key (digits reversed)
    c = allc.copy()
    for j in range(t):
        key_of += (c % 4) << (2 * (t - 1 - j))
        c //= 4
    k[key_of[have]] = rows[lo[have]]
    l[key_of[have]] = rows[hi[have] - 1]
    assert (l[key_of[have]] - k[key_of[have]] == hi[have] - lo[have] - 1).all()       # a string's rows are consecutive
    return k, l


def table_depth(n):
    """floor(log4 n) + 1, 1 for n < 4"""
    t = 1
    while n >= 4:
        n >>= 2
        t += 1
    return t


def pac_bytes(text):
    """.pac: 4 bases a byte, first base in the top bits, n // 4 + 1 bytes, then n % 4 (bntseq.c:240-250)"""
    text = np.asarray(text, np.uint8)
    n = len(text)
    pad = np.zeros((n // 4 + 1) * 4, np.uint8)
    pad[:n] = text
    q = pad.reshape(-1, 4)
    return bytes((q[:, 0] << 6 | q[:, 1] << 4 | q[:, 2] << 2 | q[:, 3]).astype(np.uint8)) + bytes([n % 4])


class RefDir:
    """one direction: sa, isa, primary, occ, and the word streams on request"""

    def __init__(self, text):
        self.text = np.ascontiguousarray(text, np.uint8)
        self.n = len(self.text)
        self.sa = suffix_array(self.text)
        self.isa = np.empty(self.n + 1, np.int64)
        self.isa[self.sa] = np.arange(self.n + 1)
        self.primary = int(self.isa[0])
        self.occ = occ_table(self.text, self.sa)
        self.bwt = bwt_words(self.text, self.sa)

    def sa_words(self, intv):
        return sa_words(self.text, intv, self.sa)

    def kmer(self, t):
        return kmer_intervals(self.text, self.sa, t)


class RefIndex:
    """both directions of one text: d[0] over the text, d[1] over text[::-1]"""

    def __init__(self, text):
        text = np.ascontiguousarray(text, np.uint8)
        self.text = text
        self.n = len(text)
        self.d = [RefDir(text), RefDir(text[::-1])]

    def streams(self, intv=32):
        """(.bwt, .rbwt, .sa, .rsa) as uint32 arrays"""
        return self.d[0].bwt, self.d[1].bwt, self.d[0].sa_words(intv), self.d[1].sa_words(intv)

    def write(self, prefix, intv=32):
        for ext, w in zip(("bwt", "rbwt", "sa", "rsa"), self.streams(intv)):
            w.tofile("%s.%s" % (prefix, ext))


# ------------------------------------------------------------------ the texts

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 28, 29, 30, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385,
           575, 576, 577, 1000]
SPECIAL_LENGTHS = [192, 193, 384, 385]
INTV_LENGTHS = [192, 193, 385, 1000]
UNIT = np.array([0, 1, 2, 3, 3, 1, 0, 2], np.uint8)        # ACGTTCAG: no shorter period


def random_text(n, seed=None):
    return np.random.default_rng(20261020 + n if seed is None else seed).integers(0, 4, n).astype(np.uint8)


def homopolymer(n):
    """A^n: the whole text is the largest suffix, primary = n"""
    return np.zeros(n, np.uint8)


def a_then_c(n):
    """A^(n-1) C: the whole text is the smallest suffix after '$', primary = 1"""
    t = np.zeros(n, np.uint8)
    t[-1] = 1
    return t


def tandem(n):
    return np.tile(UNIT, n // 8 + 1)[:n].copy()


# seeds of random_text(1000, seed) whose forward primary has the property (searched with this module; asserted where they are used)
PRIMARY_SEEDS = {(192, 0): 10, (192, 1): 733, (192, 191): 131, (128, 0): 35, (128, 127): 131}      # {(modulus, residue): seed}


def special_intvs(n):
    return [1, 2, 31, 33, 64, 192, n, n + 1]


# ------------------------------------------------------------------ the edge reads

READ_LENS = (36, 50, 70)
HEAD_POS = (0, 1, 15, 16, 17, 31, 32, 33)
TAIL_BACK = (0, 1, 15, 16, 17, 32)


def _variants(r):
    """a read and its six one-difference variants (substitution at 0, last, 16, len / 2; a base deleted at 5; one inserted 6 from the end)"""
    L = len(r)
    out = [r.copy()]
    for p in (0, L - 1, 16, L // 2):
        v = r.copy()
        v[p] = (v[p] + 1) & 3
        out.append(v)
    out.append(np.delete(r, 5))
    out.append(np.insert(r, L - 6, (r[L - 6] + 2) & 3))
    return out


def edge_reads(text, seed=1, short=False):
    """the reads of one text as code arrays, each once as written and once reverse-complemented"""
    text = np.asarray(text, np.uint8)
    n = len(text)
    rng = np.random.default_rng(seed)
    reads = []
    for L in READ_LENS:
        if L > n:
            continue
        pos = sorted(set(p for p in list(HEAD_POS) + [n - L - d for d in TAIL_BACK] if 0 <= p <= n - L))
        for p in pos:
            r = text[p:p + L]
            vs = _variants(r)
            reads += vs
            if p == 0:                                     # two foreign bases in front: the read hangs off the text's start
                reads += [np.concatenate([[(r[0] + 1) & 3, (r[0] + 2) & 3], v]).astype(np.uint8) for v in vs[:2]]
            if p + L == n:                                 # two behind: it hangs off the end
                reads += [np.concatenate([v, [(r[-1] + 1) & 3, (r[-1] + 3) & 3]]).astype(np.uint8) for v in vs[:2]]
    if short:
        for extra in (1, 2, 10, 40):                       # reads longer than the text: the text inside, the text at either end
            f = rng.integers(0, 4, extra).astype(np.uint8)
            reads += [np.concatenate([f, text]), np.concatenate([text, f]), np.concatenate([f, text, f])]
        reads += [rng.integers(0, 4, 40).astype(np.uint8) for _ in range(20)]
        reads += [np.tile(text, 40 // n + 2)[:40].copy(), np.tile(text, 40 // n + 2)[n // 2:n // 2 + 40].copy()]
    out = []
    for r in reads:
        r = np.ascontiguousarray(r, np.uint8)
        out += [r, (3 - r)[::-1].copy()]
    return out


def encode(reads):
    """code arrays -> (seq, rseq, off): bwa_seq_t.seq is the read reversed, rseq its complement (bwaseqio.c:225-232)"""
    seq = np.concatenate([r[::-1] for r in reads]).astype(np.uint8)
    rseq = (3 - seq).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return seq, rseq, off


def fastq(reads):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, "".join("ACGT"[c] for c in r), "I" * len(r)) for i, r in enumerate(reads))


def fasta(text, name="t", width=60):
    s = "".join("ACGT"[c] for c in text)
    return ">%s\n" % name + "".join(s[i:i + width] + "\n" for i in range(0, len(s), width))


def search_texts():
    """[(name, text, short)] of part 4"""
    out = [("random%d" % n, random_text(n), False) for n in (193, 384, 577, 1000, 1024)]
    out += [("A385", homopolymer(385), False), ("A191C", a_then_c(192), False), ("tandem576", tandem(576), False)]
    out += [("random%d" % n, random_text(n), True) for n in (20, 33, 64)] + [("A30", homopolymer(30), True)]
    return out


# gap_opt_t fields the option sets change from gap_init_opt (bwtaln.c:19-35, :309-345): what `bwa aln` makes of the switches
OPTION_SETS = [
    ("default", [], {}),
    ("n3o2e3", ["-n", "3", "-o", "2", "-e", "3"], dict(max_diff=3, fnr=-1.0, max_gapo=2, max_gape=3, mode=0x02)),
    ("l20k1", ["-l", "20", "-k", "1"], dict(seed_len=20, max_seed_diff=1)),
]
