#!/usr/bin/env python3
"""Generate tests/golden/reference_func_lines.json from a checkout of the Go reference.

For every reference file that tests/test_go_shim_matches_header.py's REFERENCE_SIGNATURES names, the sha256 of each
top-level `func ` line (as read, trailing whitespace removed).  Only digests are stored: the test checks that each
signature of its table is one of its file's declarations without the reference tree being present.

    python tests/golden/make_reference_func_lines.py PATH_TO_REFERENCE
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_go_shim_matches_header import REFERENCE_SIGNATURES  # noqa: E402


def main(ref):
    files = sorted({fname for fname, _ in REFERENCE_SIGNATURES.values()})
    out = {"_comment": "sha256 of each `func ` line of the reference's files; made by tests/golden/make_reference_func_lines.py",
           "files": {}}
    for fname in files:
        lines = open(os.path.join(ref, fname)).read().splitlines()
        out["files"][fname] = sorted(hashlib.sha256(ln.rstrip().encode()).hexdigest() for ln in lines if ln.startswith("func "))
    with open(os.path.join(HERE, "reference_func_lines.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {sum(len(v) for v in out['files'].values())} digests of {len(files)} files")


if __name__ == "__main__":
    main(sys.argv[1])
