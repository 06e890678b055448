#!/usr/bin/env python3
"""Do two versions of the kernel library compile to the same instructions?  For a refactor that moves kernels between files.

    python tools/isa_same.py OLD_CSRC NEW_CSRC [--removed SYMBOL ...]

Cross-compiles every .hip of both directories (as tools/kres.py does, eight at a time) and compares the instruction stream
of every kernel symbol, whichever file it sits in: comments and directives dropped, local labels numbered in order of
appearance.  Prints the symbols only in OLD, only in NEW and those whose streams differ; exit status 1 on any difference
beyond the symbols named by --removed (substrings of the mangled name)."""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

import kres


def streams(csrc):
    """{kernel symbol: normalised instruction stream} over every .hip of the directory"""
    def one(path):
        with tempfile.TemporaryDirectory() as td:
            subprocess.run([kres.HIPCC] + kres.FLAGS + [path, "-o", "k.s"], check=True, cwd=td)
            lines = open(os.path.join(td, "k.s")).read().split("\n")
        out, cur = {}, None
        for l in lines:
            m = re.match(r"^(_Z\w+):", l)
            if m:
                cur, labels = [], {}
                out[m.group(1)] = cur
            elif l.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and (l.startswith(".L") or (l.startswith("\t") and not l.startswith(("\t.", "\t;")))):
                l = l.split(";")[0].rstrip()      # no instruction of this ISA carries a ';' before its trailing comment
                cur.append(re.sub(r"\.L(?:BB|tmp)[\d_]+", lambda x: labels.setdefault(x.group(0), f".L{len(labels)}"), l))
        return out
    paths = sorted(os.path.join(os.path.abspath(csrc), f) for f in os.listdir(csrc) if f.endswith(".hip"))
    res = {}                                  # a symbol of an anonymous namespace may exist in several files: keep all
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        for ks in ex.map(one, paths):
            for sym, body in ks.items():
                res.setdefault(sym, []).append(body)
    return {sym: sorted(bodies) for sym, bodies in res.items()}


def main(argv):
    cut = argv.index("--removed") if "--removed" in argv else len(argv)
    (old_dir, new_dir), removed = argv[:cut], argv[cut + 1:]
    old, new = streams(old_dir), streams(new_dir)
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(s for s in set(old) & set(new) if old[s] != new[s])
    for title, syms in (("only in OLD", gone), ("only in NEW", added), ("streams differ", differ)):
        print(f"# {title}: {len(syms)}")
        for s in syms:
            print(f"  {s}")
    print(f"# {len(set(old) & set(new)) - len(differ)} of {len(set(old) & set(new))} common kernels identical")
    unexpected = [s for s in gone if not any(r in s for r in removed)] + [r for r in removed if not any(r in s for s in gone)]
    return 1 if unexpected or added or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
