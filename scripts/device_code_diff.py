#!/usr/bin/env python
"""Device code of two trees, kernel by kernel:  python scripts/device_code_diff.py PARENT_TREE CHANGE_TREE [file.hip ...]

For a change that is meant to touch host code only.  Each .hip file (default: every source of nsfnet_amd/build.py
whose text, or any header's, differs between the trees) is compiled in both trees to device-only gfx950 assembly with
the file's own flags (FLAGS + EXTRA_FLAGS[file]).  The assembly is cut into kernels at the .globl symbols; a kernel's
text is its instructions and directives without `;` comments, with the compiler's local labels (.LBB<fn>_<n>,
.Lfunc_end<fn>, ...) renumbered in order of appearance: the function index in them follows the order of emission,
which a host-side change may alter.  Prints  file | kernels | equal/DIFFERS  and exits 1 where a kernel differs, is
added or is missing.  Needs hipcc and no GPU."""
import filecmp
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nsfnet_amd import build as B  # noqa: E402

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def kernels(asm):
    """{symbol: normalised text} of every global function of a device assembly file."""
    out, name = {}, None
    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.type\s+(\S+),@function$", line)
        if m:      # a function runs from its .type to its .size: instructions, then the kernel descriptor
            name = m.group(1)
            out[name] = []
        elif name is not None:
            out[name].append(line)
            if re.match(r"\.size\s+%s," % re.escape(name), line):
                name = None
    norm = {}
    for k, lines in out.items():
        seen = {}
        text = "\n".join(lines)
        norm[k] = LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), text)
    return norm


def device_asm(tree, src, tmp):
    s = os.path.join(tree, "nsfnet_amd", "csrc", src)
    o = os.path.join(tmp, src + ".s")
    cmd = [B._hipcc()] + B.FLAGS + B.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", s, "-o", o]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (s, r.stderr))
    with open(o) as f:
        return kernels(f.read())


def main():
    parent, change, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    csrc = lambda t, f: os.path.join(t, "nsfnet_amd", "csrc", f)
    if not files:
        hdr = any(not (os.path.exists(csrc(parent, h)) and filecmp.cmp(csrc(parent, h), csrc(change, h), False)) for h in B.HEADERS)
        files = [s for s in B.SOURCES if hdr or not filecmp.cmp(csrc(parent, s), csrc(change, s), False)]
    bad = 0
    print("# file | kernels (parent / change) | verdict")
    with tempfile.TemporaryDirectory() as tp, tempfile.TemporaryDirectory() as tc, ThreadPoolExecutor(max_workers=8) as ex:
        jobs = [(f, ex.submit(device_asm, parent, f, tp), ex.submit(device_asm, change, f, tc)) for f in files]
        for f, a, b in jobs:
            a, b = a.result(), b.result()
            differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
            only = sorted(a.keys() ^ b.keys())
            ok = not differ and not only
            bad += not ok
            print("%s | %d / %d | %s" % (f, len(a), len(b), "equal" if ok else "DIFFERS"))
            for k in differ:
                print("#   body differs: %s" % k)
            for k in only:
                print("#   only in %s: %s" % ("parent" if k in a else "change", k))
    print("# %d files, %d differ" % (len(files), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
