"""What tests/test_bam_front.py and tests/golden/make_golden_bam.py share: BAM records with every field free (on top of bamlib), a Python
model of the create stage and of the record edits, the well-formed cases that are also held against the reference, and the runner of
tests/emu/bam_front_main.cpp."""
import os
import struct
import subprocess

import numpy as np

import bamlib as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "bam_front_main.cpp")
NT16_NT4 = [4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4]
ERASED = "AM NM CM SM MD X0 X1 XA XC XG XM XN XO XT YQ".split()
BROKEN, DROP, NODUP = 1, 2, 4                          # NABWA_BAM_BROKEN_INPUT, _DROP_ALIGNED, _SKIP_DUPLICATES
PD, SU, SR, R1, R2, QC, DP = 1, 4, 16, 64, 128, 512, 1024
EINVAL = -2
SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}


# ------------------------------------------------------------------ records

def record(name, seq, quals, flag, tags=b"", cigar=(), tid=-1, pos=-1, mapq=0, b_in=4680, mtid=-1, mpos=-1, tlen=0):
    """seq: NT16 letters or a list of nt16 codes; quals: phred values (0..255); cigar: raw 32-bit words"""
    codes = [B.NT16.index(c) for c in seq] if isinstance(seq, str) else list(seq)
    assert len(codes) == len(quals)
    nm = name.encode() + b"\0"
    packed = bytearray((len(codes) + 1) // 2)
    for i, c in enumerate(codes):
        packed[i >> 1] |= c << (4 if i % 2 == 0 else 0)
    core = struct.pack("<iiIIiiii", tid, pos, b_in << 16 | mapq << 8 | len(nm), flag << 16 | len(cigar), len(codes), mtid, mpos, tlen)
    body = core + nm + struct.pack("<%dI" % len(cigar), *cigar) + bytes(packed) + bytes(quals) + tags
    return struct.pack("<I", len(body)) + body


def split(r):
    """a record's bytes -> its fields; seq as one nt16 code per base"""
    bs, tid, pos, y, z, l_seq, mtid, mpos, tlen = struct.unpack_from("<IiiIIiiii", r, 0)
    assert bs + 4 == len(r)
    l_name, n_cig = y & 0xff, z & 0xffff
    p = 36
    name = r[p:p + l_name]; p += l_name
    cigar = list(struct.unpack_from("<%dI" % n_cig, r, p)); p += 4 * n_cig
    seq = [r[p + (j >> 1)] >> (4 if j % 2 == 0 else 0) & 15 for j in range(l_seq)]; p += (l_seq + 1) // 2
    qual = list(r[p:p + l_seq]); p += l_seq
    return dict(tid=tid, pos=pos, b_in=y >> 16, mapq=y >> 8 & 0xff, flag=z >> 16, mtid=mtid, mpos=mpos, tlen=tlen, name=name, cigar=cigar,
                seq=seq, qual=qual, tags=r[p:])


def join(d):
    return record(d["name"][:-1].decode(), d["seq"], d["qual"], d["flag"], d["tags"], d["cigar"], d["tid"], d["pos"], d["mapq"], d["b_in"],
                  d["mtid"], d["mpos"], d["tlen"])


def tag(key, ty, payload):
    return key.encode() + ty.encode() + payload


def tag_b(key, sub, values):
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f", "d": "d"}[sub]
    return key.encode() + b"B" + sub.encode() + struct.pack("<I", len(values)) + struct.pack("<%d%s" % (len(values), fmt), *values)


def walk(tags):
    """well-formed tags -> [(offset, key, type, bytes of the whole tag)]"""
    out, p = [], 0
    while p < len(tags):
        key, ty = tags[p:p + 2].decode(), chr(tags[p + 2])
        if ty in SIZE:
            n = 3 + SIZE[ty]
        elif ty in "ZH":
            n = tags.index(b"\0", p + 3) + 1 - p
        else:
            assert ty == "B"
            n = 8 + SIZE[chr(tags[p + 3])] * struct.unpack_from("<I", tags, p + 4)[0]
        out.append((p, key, ty, tags[p:p + n])); p += n
    assert p == len(tags)
    return out


# ------------------------------------------------------------------ the model of the create stage

def model_erase(tags):
    """erase_unwanted_tags (bwaseqio.c:413-464)"""
    return b"".join(t for _, key, _, t in walk(tags) if key not in ERASED)


def model_rg(tags):
    """bam_get_rg (bamlite.c:157-201): the first RG:Z or RG:A that begins more than four bytes before the end of the record"""
    for p, key, ty, t in walk(tags):
        if p + 4 >= len(tags):
            break
        if key == "RG" and ty == "Z":
            return t[3:-1]
        if key == "RG" and ty == "A":
            return t[3:4]
    return b""


def model_trim(quals, trim_qual):
    """bwa_trim_read (bwaseqio.c:110-123) on phred values in the read's orientation"""
    s, best, best_l = 0, 0, len(quals) - 1
    if trim_qual < 1:
        return len(quals)
    for l in range(len(quals) - 1, 33, -1):
        s += trim_qual - quals[l]
        if s < 0:
            break
        if s > best:
            best, best_l = s, l
    return best_l + 1


def model_encode(d, trim_qual):
    """bam1_to_seq (bwaseqio.c:272-307) with is_comp = 1 -> seq, rseq"""
    comp = lambda c: 3 - c if c < 4 else c
    read = [NT16_NT4[c] for c in d["seq"]]
    qual = [min(q, 93) for q in d["qual"]]                       # phred + 33 capped at 126
    if d["flag"] & SR:
        read, qual = [comp(c) for c in reversed(read)], qual[::-1]
    read = read[:model_trim(qual, trim_qual)]
    return bytes(reversed(read)), bytes(comp(c) for c in reversed(read))


def model_front(recs, flags, trim_qual):
    """-> dict(rc, msg) or what bam_front_main's `front` writes (see parse_front)"""
    d = [split(r) for r in recs]
    for x in d:
        x["tags"] = model_erase(x["tags"])
    err = lambda m: dict(rc=EINVAL, msg=m)
    logical, i = [], 0
    while i < len(d):
        k = 1
        if d[i]["flag"] & PD:
            if i + 1 >= len(d):
                if flags & BROKEN:
                    break
                return err("a paired read at the end of the batch without its mate (keep mates in one batch)")
            if d[i]["name"] != d[i + 1]["name"]:
                if flags & BROKEN:
                    i += 1
                    continue
                return err("lone mate: two paired reads whose names do not match")
            f0, f1 = d[i]["flag"] & (PD | R1 | R2), d[i + 1]["flag"] & (PD | R1 | R2)
            if (f0, f1) == (PD | R2, PD | R1):
                d[i], d[i + 1] = d[i + 1], d[i]
            elif (f0, f1) != (PD | R1, PD | R2):
                if not flags & BROKEN:
                    return err("a pair whose read 1 / read 2 flags are wrong")
                d[i]["flag"] = d[i]["flag"] & ~R2 | PD | R1
                d[i + 1]["flag"] = d[i + 1]["flag"] & ~R1 | PD | R2
            k = 2
        mates = d[i:i + k]
        if not (flags & DROP and not all(m["flag"] & SU for m in mates)):
            qc = max(m["flag"] & QC for m in mates)
            for m in mates:
                m["flag"] |= qc
            logical.append((mates, bool(flags & NODUP and any(m["flag"] & DP for m in mates))))
        i += k
    out = dict(rc=0, kind=[], first=[], rg=[], skip=[], rg_names=[], full_len=[], seq=[], rseq=[], recs=[])
    for mates, skip in logical:
        name = model_rg(mates[0]["tags"])
        if name not in out["rg_names"]:
            out["rg_names"].append(name)
        out["kind"].append(len(mates)); out["first"].append(len(out["recs"])); out["rg"].append(out["rg_names"].index(name)); out["skip"].append(int(skip))
        for m in mates:
            s, r = (b"", b"") if skip else model_encode(m, trim_qual)
            out["recs"].append(join(m)); out["full_len"].append(len(m["seq"])); out["seq"].append(s); out["rseq"].append(r)
    return out


# ------------------------------------------------------------------ the model of the record edits

def model_revcom(d):
    """revcom_bam1 (bam2bam.c:335-362)"""
    comp = lambda c: int("{:04b}".format(c)[::-1], 2)            # the complement of an nt16 code is its bits reversed
    return dict(d, flag=d["flag"] ^ SR, seq=[comp(c) for c in reversed(d["seq"])], qual=d["qual"][::-1])


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


# ------------------------------------------------------------------ the cases that are also put to the reference

def well_formed_cases():
    """name -> records: pairing, tag erasure, read groups and encoding on input the reference reads without leaving the record"""
    rng = np.random.default_rng(20261018)
    bases = lambda n: "".join(rng.choice(list("ACGT"), n))
    q30 = lambda n: [30] * n
    se = lambda name, n=40, flag=SU, tags=b"", seq=None, qual=None: record(name, seq if seq is not None else bases(n), qual if qual is not None else q30(n), flag, tags)
    pe = lambda name, f1, f2, t1=b"", t2=b"", n=36: [record(name, bases(n), q30(n), f1, t1), record(name, bases(n), q30(n), f2, t2)]
    P1, P2 = PD | SU | 8 | R1, PD | SU | 8 | R2
    c = {}
    c["mates_in_order_and_reversed"] = pe("a", P1, P2) + pe("b", P2, P1) + [se("s")] + pe("c", P1, P2)
    c["wrong_read_flags"] = pe("a", P1, P2) + pe("w", P1, P1) + pe("x", PD | SU, PD | SU | R1 | R2) + [se("s")]
    c["lone_mate_in_mid_batch"] = pe("a", P1, P2) + [record("lone", bases(36), q30(36), P1)] + pe("b", P1, P2) + [se("s")]
    c["lone_mate_before_singleton"] = [record("lone", bases(36), q30(36), P2), se("s")] + pe("b", P1, P2)
    c["paired_read_last"] = [se("s")] + pe("a", P1, P2) + [record("last", bases(36), q30(36), P1)]
    c["mapped_ends"] = pe("a", P1 & ~SU, P2) + pe("b", P1, P2 & ~SU) + pe("c", P1 & ~SU, P2 & ~SU) + pe("d", P1, P2) + [se("m", flag=0), se("u")]
    c["duplicates_and_qc"] = pe("a", P1 | DP, P2) + pe("b", P1, P2 | QC) + pe("c", P1 | QC | DP, P2 | DP) + [se("d", flag=SU | DP), se("q", flag=SU | QC)]
    c["singletons_only"] = [se("s%d" % i, n=35 + i) for i in range(6)]
    every = b"".join([tag(k, "i", struct.pack("<i", 5)) for k in ("AM", "NM", "CM", "SM", "X0", "X1", "XC", "XG", "XM", "XN", "XO")]
                     + [tag("MD", "Z", b"36\0"), tag("XA", "Z", b"chr1,+5,36M,0;\0"), tag("XT", "A", b"U"), tag("YQ", "c", b"\x07")])
    near = b"".join([tag("XB", "i", struct.pack("<i", 1)), tag("AS", "C", b"\x09"), tag("MC", "Z", b"36M\0"), tag("YS", "s", struct.pack("<h", -3)),
                     tag("RG", "Z", b"grp\0"), tag_b("ZB", "i", [1, -2, 3]), tag("ZH", "H", b"1AE301\0")])
    go, stay = [t for _, _, _, t in walk(every)], [t for _, _, _, t in walk(near)]
    mixed = b"".join(x + y for x, y in zip(go, stay)) + b"".join(go[len(stay):])
    c["erase_and_keep"] = [se("all_go", tags=every), se("all_stay", tags=near), se("mixed", tags=mixed), se("none")]
    rgz, rga = tag("RG", "Z", b"lib one\0"), tag("RG", "A", b"x")
    tail = tag("ZZ", "i", struct.pack("<i", 9))
    c["read_groups"] = [se("z", tags=rgz), se("z_then_more", tags=rgz + tail), se("a_last", tags=rga), se("a_then_more", tags=rga + tail), se("none"),
                        se("behind_array", tags=tag_b("ZB", "S", [1, 2, 3, 65535]) + rgz), se("behind_double", tags=tag("ZD", "d", struct.pack("<d", 2.5)) + rgz),
                        se("empty_name", tags=tag("RG", "Z", b"\0") + tail), se("second_wins_not", tags=tag("RG", "Z", b"first\0") + tag("RG", "Z", b"second\0"))]
    ga, gb = tag("RG", "Z", b"A\0"), tag("RG", "Z", b"B\0")
    c["two_groups_alternating"] = pe("p0", P1, P2, gb, gb) + [se("s0", tags=ga)] + pe("p1", P1, P2, gb, ga) + [se("s1", tags=gb), se("s2", tags=gb), se("s3", tags=ga), se("s4")]
    enc = []
    for L in range(6):
        for fl in (SU, SU | SR):
            enc.append(se("len%d_%d" % (L, fl), seq=bases(L), qual=q30(L), flag=fl))
    for L, at in ((7, 0), (7, 3), (7, 6), (8, 0), (8, 4), (8, 7)):
        for code in (15, 5):                                   # N, and R: a non-ACGT nt16 code
            s = [B.NT16.index(x) for x in bases(L)]
            s[at] = code
            for fl in (SU, SU | SR):
                enc.append(se("amb%d_%d_%d_%d" % (L, at, code, fl), seq=s, qual=q30(L), flag=fl))
    c["encode"] = enc
    trim = []
    for L in (34, 35, 36, 60):
        shapes = {"none": [40] * L, "floor": [40] * min(L, 20) + [2] * max(L - 20, 0), "between": [40] * (L - 3) + [2] * 3 if L > 36 else [40] * (L - 1) + [2],
                  "q255": [40] * (L - 12) + [2] * 6 + [255] + [2] * 5, "rise": [2] * (L - 4) + [19, 21, 19, 25]}
        for what, q in shapes.items():
            for fl in (SU, SU | SR):
                trim.append(se("trim%d_%s_%d" % (L, what, fl), seq=bases(L), qual=(q[::-1] if fl & SR else q), flag=fl))
    c["trim"] = trim
    return c


# ------------------------------------------------------------------ the harness

def build(out, *flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17"] + list(flags) + ["-o", out, SRC, "-lpthread"], capture_output=True, text=True)


def offsets_of(recs):
    off = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return off


def run(exe, args, env=None, timeout=60):
    e = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    e.update(env or {})
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=e, timeout=timeout)
    assert r.returncode == 0 and r.stderr == "", (args, r.returncode, r.stderr[-3000:])
    return r.stdout


def parse_records(raw, p, n):
    off = np.frombuffer(raw, np.int64, n + 1, p); p += 8 * (n + 1)
    return [raw[p + off[i]:p + off[i + 1]] for i in range(n)], p + int(off[n])


def parse_front(raw):
    rc = struct.unpack_from("<i", raw, 0)[0]
    if rc:
        return dict(rc=rc, msg=raw[4:].decode())
    n, nk, nrg = struct.unpack_from("<iii", raw, 4)
    p = 16
    t = np.frombuffer(raw, np.int32, 4 * nk, p).reshape(nk, 4); p += 16 * nk
    names = []
    for _ in range(nrg):
        l = struct.unpack_from("<i", raw, p)[0]
        names.append(raw[p + 4:p + 4 + l]); p += 4 + l
    off = np.frombuffer(raw, np.int64, n + 1, p); p += 8 * (n + 1)
    full = np.frombuffer(raw, np.int32, n, p); p += 4 * n
    tot = int(off[n])
    seq, rseq = raw[p:p + tot], raw[p + tot:p + 2 * tot]; p += 2 * tot
    recs, p = parse_records(raw, p, n)
    assert p == len(raw)
    return dict(rc=0, kind=t[:, 0].tolist(), first=t[:, 1].tolist(), rg=t[:, 2].tolist(), skip=t[:, 3].tolist(), rg_names=names, full_len=full.tolist(),
                seq=[seq[off[i]:off[i + 1]] for i in range(n)], rseq=[rseq[off[i]:off[i + 1]] for i in range(n)], recs=recs)


def parse_ref(blob):
    """what oracle/ref_harness.c's ref_read_bam_pairs wrote -> (the result of the last call, [(kind, [record fields])])"""
    p, logical = 0, []
    while True:
        r, kind = struct.unpack_from("<ii", blob, p); p += 8
        if r <= 0:
            assert p == len(blob)
            return r, logical
        mates = []
        for _ in range(kind):
            tid, pos, b_in, mapq, l_name, flag, n_cig, l_seq, mtid, mpos, tlen, n = struct.unpack_from("<12i", blob, p); p += 48
            data = blob[p:p + n]; p += n
            n = struct.unpack_from("<i", blob, p)[0]; rg = blob[p + 4:p + 4 + n]; p += 4 + n
            n = struct.unpack_from("<i", blob, p)[0]; seq, rseq = blob[p + 4:p + 4 + n], blob[p + 4 + n:p + 4 + 2 * n]; p += 4 + 2 * n
            rec = struct.pack("<IiiIIiiii", 32 + len(data), tid, pos, b_in << 16 | mapq << 8 | l_name, flag << 16 | n_cig, l_seq, mtid, mpos, tlen) + data
            mates.append(dict(rec=rec, rg=rg, seq=seq, rseq=rseq, full_len=l_seq))
        logical.append((r, mates))


def front(exe, tmp, recs, flags, trim_qual, off=None, env=None, raw=False):
    """the create stages over `recs` (off: other offsets than the records' own) -> parse_front's dict"""
    tmp = str(tmp)
    with open(os.path.join(tmp, "in.bytes"), "wb") as f:
        f.write(b"".join(recs))
    (offsets_of(recs) if off is None else np.asarray(off, np.int64)).tofile(os.path.join(tmp, "in.off"))
    run(exe, ["front", os.path.join(tmp, "in.bytes"), os.path.join(tmp, "in.off"), flags, trim_qual, os.path.join(tmp, "out.bin")], env=env)
    data = open(os.path.join(tmp, "out.bin"), "rb").read()
    return data if raw else parse_front(data)
