#!/usr/bin/env python3
"""Writes tests/golden/fir_head_parent.json: one SHA-256 of the output bytes per case of tests/test_gpu_fir_head.py.

Run it on the GPU with the library built from the commit whose bits are to be pinned (the parent of a change to the
fused kernel's loads); the test then recomputes the hashes from the library under test.  Inputs are seeded, so only the
hashes are stored.  --check compares instead of writing and prints the cases that differ."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import test_gpu_fir_head as T       # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=T.GOLDEN)
    ap.add_argument("--check", action="store_true", help="compare with --out instead of writing it")
    ap.add_argument("--records", help="also keep the full per-case records (error figures) in this JSON file")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        res = T.run_child(os.path.join(d, "results.json"))
    if a.records:
        with open(a.records, "w") as f:
            json.dump(res, f, indent=0, sort_keys=True)
    hashes = {k: v["sha"] for k, v in sorted(res.items())}
    assert sorted(hashes) == sorted(T.IDS), "the child did not run every case"
    if a.check:
        with open(a.out) as f:
            want = json.load(f)
        bad = [k for k in hashes if want.get(k) != hashes[k]]
        print(f"{len(hashes) - len(bad)} of {len(hashes)} cases match {a.out}")
        for k in bad:
            print("  differs:", k)
        return 1 if bad else 0
    with open(a.out, "w") as f:
        json.dump(hashes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(hashes)} hashes -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
