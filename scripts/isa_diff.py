#!/usr/bin/env python3
"""Compare the gfx950 device assembly of the kernel sources at a git revision with the working tree's.  CPU only.

    python scripts/isa_diff.py REV [file.hip ...] [--define NAME ...] [--hashes]

For each named k_*.hip (default: every k_* source of mdgen_amd/build.py) the file is compiled as build.check_isa does
(hipcc, build.flags_for(src) without -fPIC, -S --cuda-device-only), once from `git archive REV mdgen_amd/csrc include`
unpacked into a temporary directory and once from the tree.  Lines that contain `__hip_cuid_` are ignored: that symbol is
a hash of the translation unit and is the only thing that differs when a source gains a blank line.  Prints `identical`
per file or the first differing lines; exit status 1 on any difference.  --define passes -DNAME to both compiles (the
surviving experiment builds: --define MDGEN_DEV_BUILD --define MDGEN_DEV_FLASH_STAMPS); --hashes prints one line per
file with the sha256 of the normalised assembly, REV's and the tree's.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import difflib
import hashlib
import io
import os
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mdgen_amd import build  # noqa: E402

CSRC_REL = os.path.relpath(build.CSRC, ROOT)


def assembly(cc, root, name, defines):
    """Normalised device assembly (list of lines) of csrc/<name> under `root`."""
    src = os.path.join(root, CSRC_REL, name)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [cc] + [f for f in build.flags_for(src) if f != "-fPIC"] + ["-D" + d for d in defines] + ["-S", "--cuda-device-only", src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd) + "\n" + r.stderr)
        with open(out) as f:
            return [line for line in f if "__hip_cuid_" not in line]


def sha(lines):
    return hashlib.sha256("".join(lines).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("files", nargs="*", help="k_*.hip names (default: all kernel sources of build.SOURCES)")
    ap.add_argument("--define", action="append", default=[], metavar="NAME", help="pass -DNAME to both compiles (repeatable)")
    ap.add_argument("--hashes", action="store_true", help="print `file  sha256(REV)  sha256(tree)` per file")
    ap.add_argument("-j", type=int, default=8, help="compiles at a time (at most 8)")
    a = ap.parse_args()
    names = [os.path.basename(f) for f in a.files] or [s for s in build.SOURCES if s.startswith("k_")]
    cc = build.hipcc()
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, CSRC_REL, "include"], capture_output=True, check=True).stdout
        with tarfile.open(fileobj=io.BytesIO(tar)) as t:
            t.extractall(old)
        with cf.ThreadPoolExecutor(max_workers=max(1, min(a.j, 8))) as ex:
            jobs = {(n, side): ex.submit(assembly, cc, root, n, a.define) for n in names for side, root in (("old", old), ("new", ROOT))}
            differ = 0
            for n in names:
                o, w = jobs[n, "old"].result(), jobs[n, "new"].result()
                if a.hashes:
                    print(f"{n}  {sha(o)}  {sha(w)}")
                if o == w:
                    if not a.hashes:
                        print(f"{n}: identical")
                    continue
                differ += 1
                print(f"{n}: DIFFERENT")
                for i, line in enumerate(difflib.unified_diff(o, w, a.rev, "tree", n=1)):
                    if i >= 40:
                        print("    ...")
                        break
                    print("    " + line.rstrip("\n"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
