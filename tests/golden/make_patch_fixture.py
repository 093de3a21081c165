#!/usr/bin/env python3
"""Generate tests/golden/reference_patch_targets.json: what tests/test_integration_patches.py needs to know about the four
pristine reference files that integration/*.patch edit, without any of their text entering this repository.

    HALO_REFERENCE=<reference checkout> python tests/golden/make_patch_fixture.py

Per file: its line count, whether it ends in a newline, the SHA-256 of the whole file and of the lines every hunk of the
committed patch replaces (at the hunk's own position), and how often each string the test looks for occurs in it.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_integration_patches import NEEDLES, PATCHES, parse_patch  # noqa: E402


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def main():
    ref = os.environ.get("HALO_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not ref:
        sys.exit("set HALO_REFERENCE (or pass the path) to a pristine reference checkout")
    files = {}
    for name in PATCHES:
        rel, hunks = parse_patch(open(os.path.join(ROOT, "integration", name)).read())
        text = open(os.path.join(ref, rel)).read()
        lines = text.splitlines(keepends=True)
        files[rel] = {
            "lines": len(lines), "ends_with_newline": text.endswith("\n"), "sha256": sha(text),
            "hunks": [{"old_start": h["old_start"], "old_len": h["old_len"],
                       "sha256": sha("".join(lines[h["old_start"] - 1: h["old_start"] - 1 + h["old_len"]]))} for h in hunks],
            "counts": {s: text.count(s) for s in NEEDLES},
        }
    with open(os.path.join(HERE, "reference_patch_targets.json"), "w") as f:
        json.dump({"note": "pristine reference files behind integration/*.patch (tests/golden/make_patch_fixture.py)", "files": files}, f, indent=1)
        f.write("\n")
    print("wrote reference_patch_targets.json")


if __name__ == "__main__":
    main()
