#!/usr/bin/env python3
"""Write tests/golden/ref_abi.json: the reference's struct layouts as the C compiler reports them from its own headers, the raw
blocks of the worker message (test_wire.py), and the digest of INTEGRATION.md's C snippets after they compiled against those
headers.  Runs only where the reference's headers are (NABWA_REFERENCE, default as in oracle/Makefile).  Only numbers are stored.

Usage:  python tests/golden/make_ref_abi.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import refabi as R                      # noqa: E402
import test_abi_headers as H            # noqa: E402


def main():
    if not R.have_reference():
        sys.exit("the reference's headers are not at %s (set NABWA_REFERENCE)" % R.REF)
    blocks = R.integration_snippets()
    with tempfile.TemporaryDirectory() as td:
        H.cc(H.ASSERTS, td, "layout.c")
        H.compile_integration_snippets(td, blocks)
    out = {"layouts": R.measure_reference_layouts(), "raw_blocks": R.measure_raw_blocks(),
           "integration_snippets_sha256": R.snippets_digest(blocks)}
    with open(R.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", R.GOLDEN)


if __name__ == "__main__":
    main()
