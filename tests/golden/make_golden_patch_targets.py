"""Write tests/golden/ref_patch_targets.json: per-line digests of the reference
files that go/patches/*.patch modify.

    python tests/golden/make_golden_patch_targets.py <reference checkout>

The fixture holds no text of the reference, only the first 16 hex digits of
each line's SHA-256 (the line without its newline). With it
tests/test_go_adapter.py::test_patches_apply_to_the_reference checks, without
the reference tree, that every hunk's context and removed lines stand in the
file they patch.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TARGETS = ["src/settings/settings.go", "src/service_cmd/runner/runner.go", "Dockerfile", "src/service/ratelimit.go"]


def digest(line):
    return hashlib.sha256(line.encode()).hexdigest()[:16]


def main():
    ref = sys.argv[1]
    files = {}
    for rel in TARGETS:
        with open(os.path.join(ref, rel)) as f:
            files[rel] = [digest(l) for l in f.read().split("\n")]
    out = {"kind": "patch_targets",
           "note": "sha256[:16] of every line of the reference files the Go patches modify (no reference text)",
           "files": files}
    with open(os.path.join(HERE, "ref_patch_targets.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
