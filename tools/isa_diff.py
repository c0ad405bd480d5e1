#!/usr/bin/env python3
"""Compare two directories of device assembly (`make isa` writes build/isa/<name>.s) function by function.

    python3 tools/isa_diff.py PARENT/build/isa build/isa

Each .s file is split at its function labels (a label at column 0 that is not a compiler-local `.L...` one). What comes
before the first label is `<preamble>`, a kernel's `.amdhsa_kernel` block follows its code and belongs to it, and the
`.amdgpu_metadata` block at the end is `<metadata>`. Lines that contain `__hip_cuid_` are dropped: that symbol hashes
the source text. Per file and per symbol the result is `identical` or the number of differing lines. The exit status is
non-zero if anything differs, or if the two sets of files or of symbols differ. This compares text only; it looks for no
particular instruction.
"""
import difflib
import os
import re
import sys

_LABEL = re.compile(r"^([A-Za-z_$][\w.$]*):")


def split_functions(text):
    """{symbol: [lines]} in file order; lines with __hip_cuid_ dropped"""
    out = {"<preamble>": []}
    cur = out["<preamble>"]
    meta = False
    for line in text.splitlines():
        if "__hip_cuid_" in line:
            continue
        if line.strip() == ".amdgpu_metadata":
            meta, cur = True, out.setdefault("<metadata>", [])
        m = None if meta else _LABEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        cur.append(line.rstrip())
    return out


def diff_texts(a, b):
    """{symbol: differing lines (0 = identical), or 'only in A' / 'only in B'} for two assembly texts"""
    fa, fb = split_functions(a), split_functions(b)
    res = {}
    for sym in list(fa) + [s for s in fb if s not in fa]:
        if sym not in fb:
            res[sym] = "only in A"
        elif sym not in fa:
            res[sym] = "only in B"
        elif fa[sym] == fb[sym]:
            res[sym] = 0
        else:
            sm = difflib.SequenceMatcher(None, fa[sym], fb[sym], autojunk=False)
            res[sym] = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
    return res


def diff_dirs(a_dir, b_dir, out=sys.stdout):
    """prints the per-file, per-symbol result; returns True when everything is identical"""
    names = lambda d: sorted(f for f in os.listdir(d) if f.endswith(".s"))
    na, nb = names(a_dir), names(b_dir)
    ok = True
    for name in sorted(set(na) | set(nb)):
        if name not in na or name not in nb:
            print(f"{name}: only in {'A' if name in na else 'B'}", file=out)
            ok = False
            continue
        with open(os.path.join(a_dir, name)) as f:
            a = f.read()
        with open(os.path.join(b_dir, name)) as f:
            b = f.read()
        res = diff_texts(a, b)
        bad = {s: r for s, r in res.items() if r != 0}
        kernels = sum(1 for line in b.splitlines() if line.lstrip().startswith(".amdhsa_kernel "))
        if not bad:
            print(f"{name}: identical ({len(res)} symbols, {kernels} kernels)", file=out)
            continue
        ok = False
        print(f"{name}: DIFFERS in {len(bad)} of {len(res)} symbols", file=out)
        for s, r in bad.items():
            print(f"    {s}: {r if isinstance(r, str) else str(r) + ' differing lines'}", file=out)
    print("all identical" if ok else "DIFFERENT", file=out)
    return ok


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(0 if diff_dirs(sys.argv[1], sys.argv[2]) else 1)
