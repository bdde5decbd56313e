#!/usr/bin/env python3
"""Pin integration/ocaml/hvc_backend.patch to the reference it is a diff against, as data (ocaml_patch_preimage.json):

  * for every file the patch touches: the reference's line count and SHA-256,
  * for every hunk: where it applies and the SHA-256 of its pre-image, i.e. of the reference's own lines at that place,
  * ANCHORS: the line numbers of definitions outside the hunks that tests/test_ocaml_binding.py orders the patched functions
    against.

Before it writes anything it applies the patch with `patch` to copies of the reference's files (no fuzz) and checks that every
hunk's pre-image hashes to what the reference holds.  Hashes and line numbers only: no line of the reference is written.

    python tests/golden/make_patch_preimage.py <reference checkout>
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ocaml_binding as chk  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ocaml_patch_preimage.json")
ANCHORS = {"jpeg/model/src/decoder.ml": ["let get_yuv_frame decoder"]}


def sha256_lines(lines):
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def main(ref):
    with open(chk.PATCH) as f:
        files = chk.parse_patch(f.read())
    with tempfile.TemporaryDirectory() as tmp:
        for path in files:
            os.makedirs(os.path.dirname(os.path.join(tmp, path)), exist_ok=True)
            shutil.copy(os.path.join(ref, path), os.path.join(tmp, path))
        with open(chk.PATCH) as f:
            r = subprocess.run(["patch", "-p1", "--dry-run", "--no-backup-if-mismatch"], stdin=f, cwd=tmp, capture_output=True, text=True)
        if r.returncode != 0 or "FAILED" in r.stdout or "fuzz" in r.stdout or "offset" in r.stdout:
            sys.exit("the patch does not apply exactly to %s:\n%s%s" % (ref, r.stdout, r.stderr))
    out = {"what": "integration/ocaml/hvc_backend.patch against the reference: line counts, SHA-256 of the files and of every "
                   "hunk's pre-image, anchor line numbers (tests/golden/make_patch_preimage.py)", "files": {}}
    for path, hunks in sorted(files.items()):
        with open(os.path.join(ref, path), "rb") as f:
            raw = f.read()
        lines = raw.decode().splitlines()
        entry = {"lines": len(lines), "sha256": hashlib.sha256(raw).hexdigest(), "hunks": [], "anchors": {}}
        for h in hunks:
            pre = lines[h["old_start"] - 1:h["old_start"] - 1 + h["old_len"]]
            assert pre == [ln[1:] for ln in h["lines"] if ln[0] in " -"], (path, h["old_start"])
            entry["hunks"].append({"old_start": h["old_start"], "old_len": h["old_len"], "sha256": sha256_lines(pre)})
        for a in ANCHORS.get(path, []):
            entry["anchors"][a] = next(n for n, ln in enumerate(lines, 1) if a in ln)
        out["files"][path] = entry
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
