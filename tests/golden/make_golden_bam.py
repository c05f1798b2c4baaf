#!/usr/bin/env python3
"""vectors_bam_front.npz: the create stage of bam2bam as the compiled reference does it (oracle/_ref/libbwaref.so, `make -C oracle ref`).

Every case of bam_front_lib.well_formed_cases() goes, as a gzip stream of "BAM\\1", an empty header and its records, through
ref_read_bam_pairs of oracle/ref_harness.c -- bwa_bam_open, read_bam_pair, bam_get_rg and bam1_to_seq (bwaseqio.c:340-494,272-307;
bamlite.c:157-201), all the reference's own -- with allow_broken and ignore_aligned each off and on and trim_qual 0 and 20 (is_comp = 1,
what bam2bam runs with by default).  The file holds the cases' records (in_<case>, off_<case>) and what came back (ref_<case>_<allow_broken>
<ignore_aligned>_<trim_qual>, the harness's serial form, read by bam_front_lib.parse_ref).  Its members carry no time stamp: a rerun writes
the same bytes.  Run from anywhere: python tests/golden/make_golden_bam.py"""
import ctypes as C
import gzip
import io
import os
import struct
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_front_lib as F  # noqa: E402

REFLIB = os.path.join(ROOT, "oracle", "_ref", "libbwaref.so")


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    if not os.path.exists(REFLIB):
        sys.exit("the compiled reference is missing: make -C oracle ref")
    lib = C.CDLL(REFLIB)
    lib.ref_read_bam_pairs.restype = C.c_int64
    lib.ref_read_bam_pairs.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, recs in F.well_formed_cases().items():
            out["in_" + name] = np.frombuffer(b"".join(recs), np.uint8)
            out["off_" + name] = F.offsets_of(recs)
            fn = os.path.join(d, name + ".bam")
            with gzip.open(fn, "wb") as f:
                f.write(b"BAM\1" + struct.pack("<ii", 0, 0) + b"".join(recs))
            for broken in (0, 1):
                for drop in (0, 1):
                    for trim in (0, 20):
                        buf = np.zeros(1 << 20, np.uint8)
                        n = lib.ref_read_bam_pairs(fn.encode(), broken, drop, 1, trim, buf.ctypes.data_as(C.c_void_p), buf.size)
                        assert 0 < n <= buf.size
                        out["ref_%s_%d%d_%d" % (name, broken, drop, trim)] = buf[:n].copy()
                        r, logical = F.parse_ref(buf[:n].tobytes())
            print("%-28s %3d records; strict: %s" % (name, len(recs), "read through" if F.parse_ref(out["ref_%s_00_0" % name].tobytes())[0] == 0 else "refused"))
    path = os.path.join(HERE, "vectors_bam_front.npz")
    write_npz(path, out)
    print("vectors_bam_front.npz: %d cases, %d bytes" % (len(F.well_formed_cases()), os.path.getsize(path)))


if __name__ == "__main__":
    main()
