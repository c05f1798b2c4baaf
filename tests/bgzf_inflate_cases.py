"""What the BGZF decompressor's tests share: the members (valid ones with the bytes zlib inflates them to, damaged ones with the status
the kernel body gives them), a small bit-writer for deflate blocks that zlib would never emit, and the CPU builds of the kernel body
(tests/emu/bgzf_inflate_emu.cpp, tests/emu/bgzf_inflate_main.cpp).  The yardstick is zlib on the CPU.  Test infrastructure only."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np

import bgzf_cases as Z

EOF_BLOCK = Z.EOF_BLOCK
EMU_DIR, CSRC = Z.EMU_DIR, Z.CSRC

# the status words of csrc/bgzf_inflate_body.hpp
(OK, BTYPE3, STORED_LEN, TRUNCATED, OVERSUBSCRIBED, INCOMPLETE, REPEAT_FIRST, LENGTHS_OVERRUN, NO_EOB, BAD_SYMBOL, DIST_TOO_FAR,
 OUTPUT_LONG, OUTPUT_SHORT, CRC, TOO_MANY_CODES, INVALID_CODE, INTERNAL) = range(17)


def member(payload, raw=b"", crc=None, isize=None, extra_first=False):
    """one BGZF member around a deflate payload, as tests/test_bgzf_in.py's bgzf() wraps it; crc and isize default to those of raw"""
    crc = zlib.crc32(raw) if crc is None else crc
    isize = len(raw) if isize is None else isize
    if extra_first:                       # another subfield in front of BC: the header is longer, BSIZE counts it
        xtra = b"XY" + struct.pack("<H", 3) + b"abc" + b"BC" + struct.pack("<HH", 2, len(payload) + 12 + 13 + 8 - 1)
    else:
        xtra = b"BC" + struct.pack("<HH", 2, len(payload) + 12 + 6 + 8 - 1)
    return bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", len(xtra)) + xtra + payload + struct.pack("<II", crc & 0xffffffff, isize)


def deflate(raw, level=6, strategy=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(raw) + c.flush()


def split(m):
    """a member -> (payload, crc, isize)"""
    xlen = struct.unpack_from("<H", m, 10)[0]
    crc, isize = struct.unpack_from("<II", m, len(m) - 8)
    return m[12 + xlen:len(m) - 8], crc, isize


def zlib_verdict(m):
    """what zlib on the CPU makes of a member: its bytes if the payload inflates to the end of its stream and length and CRC are the
    trailer's, else None"""
    payload, crc, isize = split(m)
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return None
    if not d.eof or len(out) != isize or zlib.crc32(out) != crc:
        return None
    return out


# ---------------------------------------------------------------- deflate blocks by hand
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nb):                 # nb bits of v, the lowest first (header fields, extra bits)
        self.acc |= (v & ((1 << nb) - 1)) << self.n
        self.n += nb
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nb):                # a Huffman code: the highest bit first
        for i in range(nb - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951 3.2.2)"""
    count = [0] * 16
    for x in lens:
        count[x] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, x in enumerate(lens):
        if x:
            out[s] = (nxt[x], x)
            nxt[x] += 1
    return out


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def put_tokens(bw, ll, dd, tokens):
    """tokens: ("L", byte), ("M", length, distance), ("E",), ("S", literal/length symbol), ("MS", length, distance symbol)"""
    for t in tokens:
        if t[0] == "L":
            bw.code(*ll[t[1]])
        elif t[0] == "E":
            bw.code(*ll[256])
        elif t[0] == "S":
            bw.code(*ll[t[1]])
        else:
            ls = max(i for i in range(29) if LBASE[i] <= t[1])
            if t[1] == 258:
                ls = 28
            bw.code(*ll[257 + ls])
            bw.put(t[1] - LBASE[ls], LEXT[ls])
            if t[0] == "MS":
                bw.code(*dd[t[2]])
            else:
                ds = max(i for i in range(30) if DBASE[i] <= t[2])
                bw.code(*dd[ds])
                bw.put(t[2] - DBASE[ds], DEXT[ds])


def fixed_block(bw, tokens, final=True):
    bw.put(1 if final else 0, 1)
    bw.put(1, 2)
    put_tokens(bw, canonical(FIXED_LL), canonical(FIXED_D), tokens)


def stored_block(bw, raw, final=True):
    bw.put(1 if final else 0, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(raw), 16)
    bw.put(len(raw) ^ 0xffff, 16)
    for x in raw:
        bw.put(x, 8)


def complete_lens(symbols):
    """lengths of a complete code over the given symbols of the code-length alphabet (at least two)"""
    k = len(symbols)
    m = max(1, (k - 1).bit_length())
    short = (1 << m) - k
    lens = [0] * 19
    for i, s in enumerate(symbols):
        lens[s] = m - 1 if i < short else m
    return lens


def plain_seq(lens):
    return [(x, 0) for x in lens]


def zeros(n):
    """n zero lengths as codes 18 and 17 (and single zeros)"""
    out = []
    while n >= 11:
        k = min(n, 138)
        out.append((18, k - 11))
        n -= k
    if n >= 3:
        out.append((17, n - 3))
        n = 0
    return out + [(0, 0)] * n


def dynamic_block(bw, nlen, ndist, seq, tokens, final=True, hclen=None, ll_lens=None, d_lens=None):
    """a dynamic block whose code lengths are sent as seq: [(symbol of the code-length alphabet, value of its extra bits)].  The
    codes the tokens are written with come from the lengths seq stands for, unless ll_lens / d_lens say otherwise"""
    used = sorted(set(s for s, _ in seq))
    assert len(used) >= 2                 # the code-length code has to be complete: one symbol alone cannot be
    cl = complete_lens(used)
    count = max(4, 1 + max(ORDER.index(s) for s in used)) if hclen is None else hclen
    bw.put(1 if final else 0, 1)
    bw.put(2, 2)
    bw.put(nlen - 257, 5)
    bw.put(ndist - 1, 5)
    bw.put(count - 4, 4)
    for i in range(count):
        bw.put(cl[ORDER[i]], 3)
    cc = canonical(cl)
    lens = []
    for s, e in seq:
        bw.code(*cc[s])
        if s < 16:
            lens.append(s)
        elif s == 16:
            bw.put(e, 2)
            lens += [lens[-1] if lens else 0] * (3 + e)
        elif s == 17:
            bw.put(e, 3)
            lens += [0] * (3 + e)
        else:
            bw.put(e, 7)
            lens += [0] * (11 + e)
    lens += [0] * (nlen + ndist)
    ll = canonical(ll_lens if ll_lens is not None else lens[:nlen])
    dd = canonical(d_lens if d_lens is not None else lens[nlen:nlen + ndist])
    put_tokens(bw, ll, dd, tokens)
    return count


def hand_built():
    """-> [(name, payload, bytes)]: dynamic blocks zlib reads and never writes"""
    out = []
    # literal/length code lengths 1..15 (1, 2, ..., 14, 15, 15: a complete code); no distance code; all 19 code-length codes sent
    lens = [0] * 257
    for i in range(14):
        lens[65 + i] = i + 1
    lens[65 + 14] = 15
    lens[256] = 15
    bw = Bits()
    msg = bytes(65 + (i * 7) % 15 for i in range(200))
    n = dynamic_block(bw, 257, 1, plain_seq(lens) + [(0, 0)] + [], [("L", x) for x in msg] + [("E",)], hclen=19)
    assert n == 19
    out.append(("lens1to15_hclen19", bw.bytes(), msg))
    # a distance code of one 1-bit code
    lens = [0] * 286
    lens[97] = lens[98] = lens[256] = 2
    lens[257] = lens[285] = 3
    bw = Bits()
    dynamic_block(bw, 286, 1, zeros(97) + [(2, 0), (2, 0)] + zeros(157) + [(2, 0), (3, 0)] + zeros(27) + [(3, 0), (1, 0)],
                  [("L", 97), ("M", 258, 1), ("L", 98), ("M", 3, 1), ("E",)])
    out.append(("dist_one_1bit_code", bw.bytes(), b"a" * 259 + b"b" * 4))
    # repeat code 16 carries the last literal/length length (3, of symbols 256 and 257) over into the eight distance lengths
    bw = Bits()
    dynamic_block(bw, 258, 8, zeros(120) + [(1, 0)] + zeros(133) + [(2, 0), (0, 0), (3, 0), (16, 3), (16, 0)],
                  [("L", 120)] * 4 + [("M", 3, 4), ("L", 254), ("L", 254), ("M", 3, 2), ("E",)])
    out.append(("repeat16_into_distances", bw.bytes(), b"x" * 7 + b"\xfe" * 5))
    # codes 18 and 17 at their maximum counts (138 and 10)
    bw = Bits()
    dynamic_block(bw, 257, 1, [(18, 127), (17, 7), (2, 0), (2, 0), (18, 106 - 11), (1, 0), (0, 0)],
                  [("L", 148), ("L", 149), ("L", 149), ("L", 148), ("E",)])
    out.append(("repeat17_18_maximum", bw.bytes(), bytes([148, 149, 149, 148])))
    # HCLEN = 4: eight code-length codes (16, 17, 18, 0, 8, 7, 9, 6), so only lengths 0 and 6..9 can be sent; literals only.
    # (Four code-length codes -- 16, 17, 18 and 0 -- can send no length but 0, so no valid block has fewer than these.)
    lens = [8] * 254 + [9] * 4
    bw = Bits()
    msg = bytes(range(256)) * 2
    n = dynamic_block(bw, 258, 1, plain_seq(lens) + [(0, 0)], [("L", x) for x in msg] + [("E",)], hclen=8)
    assert n == 8
    out.append(("hclen4", bw.bytes(), msg))
    return out


def bad_dynamic(name):
    """payloads of dynamic blocks with one rule broken"""
    bw = Bits()
    if name == "oversubscribed":          # three codes of one bit
        dynamic_block(bw, 257, 1, zeros(97) + [(1, 0), (1, 0)] + zeros(157) + [(1, 0), (0, 0)], [], ll_lens=[0] * 257)
    elif name == "incomplete":            # two codes of two bits and nothing else
        dynamic_block(bw, 257, 1, zeros(97) + [(2, 0)] + zeros(158) + [(2, 0), (0, 0)], [("L", 97), ("E",)])
    elif name == "code16_first":
        dynamic_block(bw, 257, 1, [(16, 0)] + zeros(94) + [(1, 0)] + zeros(158) + [(1, 0), (0, 0)], [], ll_lens=[0] * 257)
    elif name == "repeat_overrun":        # 97 + 1 + 158 + 1 = 257 lengths, then eleven zeros where one distance length is left
        dynamic_block(bw, 257, 1, zeros(97) + [(1, 0)] + zeros(158) + [(1, 0), (18, 0)], [], ll_lens=[0] * 257)
    elif name == "no_end_of_block":
        dynamic_block(bw, 257, 1, zeros(97) + [(1, 0), (1, 0)] + zeros(157) + [(0, 0), (0, 0)], [("L", 97)], ll_lens=[0] * 97 + [1, 1] + [0] * 158)
    bw.put(0, 32)
    return bw.bytes()


# ---------------------------------------------------------------- the valid cases
def _levels(tag, raw):
    return [("%s_level%d" % (tag, lv), [member(deflate(raw, lv), raw)], raw) for lv in (1, 6, 9)]


def valid_cases():
    """-> [(name, [members], bytes)], built once per process; the members of a case back to back are one input"""
    global _VALID
    if _VALID is not None:
        return _VALID
    rng = np.random.default_rng(1951)
    text = Z.text_like(40000, 11)
    bam = Z.golden_bam_bytes()[:60000]
    rand = rng.integers(0, 256, 0xff00).astype(np.uint8).tobytes()
    c = [("empty_input", [], b""), ("eof_block_alone", [EOF_BLOCK], b"")]
    c += [("len%d" % n, [member(deflate(bytes(range(65, 65 + n))), bytes(range(65, 65 + n)))], bytes(range(65, 65 + n))) for n in (1, 2, 3, 4)]
    c.append(("other_subfield_first", [member(deflate(text[:5000]), text[:5000], extra_first=True)], text[:5000]))
    c.append(("stored_ff00", [member(deflate(rand, 0), rand)], rand))
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    p = z.compress(text[:3000]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(text[3000:4001]) + z.flush(zlib.Z_FULL_FLUSH) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(text[4001:6000]) + z.flush()
    c.append(("full_flush_empty_stored", [member(p, text[:6000])], text[:6000]))
    c.append(("fixed_codes", [member(deflate(text, 6, 4), text)], text))
    c.append(("huffman_only", [member(deflate(text, 6, 2), text)], text))
    rle = b"".join(bytes([int(v)]) * int(n) for v, n in zip(rng.integers(0, 256, 200), rng.integers(1, 700, 200)))[:0x10000]
    c.append(("rle", [member(deflate(rle, 6, 3), rle)], rle))
    c += _levels("text", text) + _levels("bam", bam)
    full = ((b"ACGT" * 7 + b"N") * 2260)[:0x10000]
    assert len(full) == 0x10000
    c.append(("isize_10000", [member(deflate(full), full)], full))
    half = rng.integers(0, 256, 32768).astype(np.uint8).tobytes()
    bw = Bits()
    stored_block(bw, half, final=False)
    fixed_block(bw, [("M", 258, 32768), ("M", 100, 32768), ("E",)])
    c.append(("distance_32768", [member(bw.bytes(), half + half[:358])], half + half[:358]))
    bw = Bits()
    fixed_block(bw, [("L", 97), ("L", 98), ("L", 99), ("M", 5, 3), ("E",)])
    c.append(("match_from_byte_0", [member(bw.bytes(), b"abcabcab")], b"abcabcab"))
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    p = z.compress(text[:7001]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(rand[:5003]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(text[7001:15000]) + z.flush()
    raw = text[:7001] + rand[:5003] + text[7001:15000]
    c.append(("three_deflate_blocks", [member(p, raw)], raw))
    c += [("hand_" + n, [member(p, raw)], raw) for n, p, raw in hand_built()]
    bw = Bits()                           # blocks of all three kinds whose boundaries are not byte-aligned
    fixed_block(bw, [("L", 65), ("E",)], final=False)
    stored_block(bw, b"", final=False)
    fixed_block(bw, [("L", 66), ("M", 4, 2), ("E",)], final=False)
    stored_block(bw, b"xyz", final=False)
    fixed_block(bw, [("M", 6, 3), ("E",)])
    c.append(("hand_mixed_blocks", [member(bw.bytes(), b"ABABABxyzxyzxyz")], b"ABABABxyzxyzxyz"))
    # >= 300 members of mixed kinds and sizes in one call
    pool = text * 2 + bam + rand + rle + full
    ms, raws = [], []
    for k in range(320):
        n = int(rng.integers(1, 20000)) if k % 16 else 0xff00
        o = int(rng.integers(0, len(pool) - n))
        raw = pool[o:o + n]
        ms.append(member(deflate(raw, (0, 1, 6, 9)[k % 4], (0, 0, 0, 2, 3, 4)[k % 6]), raw, extra_first=k % 7 == 0))
        raws.append(raw)
        if k % 50 == 49:
            ms.append(EOF_BLOCK)
    c.append(("many_members", ms, b"".join(raws)))
    _VALID = c
    return c


# ---------------------------------------------------------------- the damaged cases
def damaged_cases():
    """-> [(name, member, status)]: each a valid member with one edit; status: the kernel body's word for it, or None where the host's
    walk over the headers refuses the member before any kernel sees it.  tests assert that zlib refuses every one of them
    (zlib_verdict() is None); none had to be dropped for that."""
    global _BAD
    if _BAD is not None:
        return _BAD
    text = Z.text_like(9000, 5)
    good = member(deflate(text), text)
    pay, crc, isize = split(good)
    rnd = np.random.default_rng(7).integers(0, 256, 300).astype(np.uint8).tobytes()
    spay = deflate(rnd, 0)
    c = [("crc_one_bit", member(pay, text, crc=crc ^ 0x100), CRC),
         ("isize_one_too_small", member(pay, text, isize=isize - 1), OUTPUT_LONG),
         ("isize_one_too_large", member(pay, text, isize=isize + 1), OUTPUT_SHORT),
         ("isize_0_on_a_stream", member(pay, text, isize=0), OUTPUT_LONG),
         ("btype_11", member(bytes([pay[0] | 6]) + pay[1:], text), BTYPE3),
         ("stored_nlen_wrong", member(spay[:3] + bytes([spay[3] ^ 1]) + spay[4:], rnd), STORED_LEN),
         ("stored_len_past_payload", member(spay[:1] + struct.pack("<HH", 301, 301 ^ 0xffff) + spay[5:], rnd, isize=301), TRUNCATED),
         ("payload_cut_by_1", member(pay[:-1], text), TRUNCATED),
         ("payload_cut_by_half", member(pay[:len(pay) // 2], text), TRUNCATED)]
    bw = Bits()
    fixed_block(bw, [("L", 97), ("L", 98), ("M", 3, 3), ("E",)])
    c.append(("distance_one_beyond_output", member(bw.bytes(), b"ab" + b"aba"), DIST_TOO_FAR))
    for name, st in (("oversubscribed", OVERSUBSCRIBED), ("incomplete", INCOMPLETE), ("code16_first", REPEAT_FIRST),
                     ("repeat_overrun", LENGTHS_OVERRUN), ("no_end_of_block", NO_EOB)):
        c.append((name, member(bad_dynamic(name), b"a" * 16), st))
    bw = Bits()
    fixed_block(bw, [("L", 97), ("S", 286), ("E",)])
    c.append(("fixed_length_symbol_286", member(bw.bytes(), b"a" * 4), BAD_SYMBOL))
    bw = Bits()
    fixed_block(bw, [("L", 97), ("MS", 3, 30), ("E",)])
    c.append(("fixed_distance_symbol_30", member(bw.bytes(), b"a" * 4), BAD_SYMBOL))
    c.append(("bsize_past_the_input", good[:16] + struct.pack("<H", len(good) + 40) + good[18:], None))
    c.append(("trailing_half_header", good[:9], None))
    _BAD = c
    return c


_VALID = _BAD = None


def sandwich(bad):
    """a damaged member between two valid ones: -> (input, the damaged member's index)"""
    a = valid_cases()[2][1][0]
    return a + bad + a, 1


# ---------------------------------------------------------------- the CPU builds of the kernel body
def _build(out, srcs, flags):
    deps = srcs + [os.path.join(CSRC, "bgzf_inflate_body.hpp"), os.path.join(CSRC, "bgzf_deflate_body.hpp")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-I" + CSRC, "-Wall", "-Wno-unused-function"] + flags + srcs + ["-o", out], check=True)
    return out


def build_emu():
    return _build(os.path.join(EMU_DIR, "libbgzf_inflate_emu.so"), [os.path.join(EMU_DIR, "bgzf_inflate_emu.cpp")], ["-O2", "-fPIC", "-shared"])


def build_main():
    """the stand-alone program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    return _build(os.path.join(EMU_DIR, "bgzf_inflate_main_asan"), [os.path.join(EMU_DIR, "bgzf_inflate_main.cpp"), os.path.join(EMU_DIR, "bgzf_inflate_emu.cpp")],
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def emu_inflate(lib, m):
    """one member through the kernel body on the CPU -> (status, bytes)"""
    lib.emu_bgzf_inflate.restype = C.c_int
    lib.emu_bgzf_inflate.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    payload, crc, isize = split(m)
    out = C.create_string_buffer(max(isize, 1))
    st = lib.emu_bgzf_inflate(payload, len(payload), out, isize, crc)
    return st, out.raw[:isize]
