#!/usr/bin/env python3
"""Compare two `hipcc --cuda-device-only -S` outputs kernel by kernel:  tools/kernel_isa_diff.py old.s new.s [more pairs ...]

For a host-only refactor the device code must not move.  A whole-file diff cannot show that, because the order in which the
compiler emits template instantiations - and with it the number in every local label - follows the host code.  So: cut each file
into one text per kernel symbol (its body from the label to .Lfunc_end, plus its .amdhsa_kernel descriptor), replace the number in
`.LBB<n>_` / `.Lfunc_end<n>` labels, drop the `;` comments (they quote those numbers and are padded to the label's width), and
compare the texts by symbol.  Prints one summary line per pair and every symbol that is missing on one side or differs; exit
status 1 if any does.  It compares text and looks for no particular instruction.
"""
import re
import sys

LOCAL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")


def kernels(path):
    lines = open(path).read().split("\n")
    names = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    out = {n: [] for n in names}
    cur = None
    for l in lines:
        m = re.match(r"(\S+):", l)
        if cur is None and m and m.group(1) in names:
            cur = m.group(1)  # the body: from the symbol's label ...
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)  # ... and the descriptor
        if cur is not None:
            out[cur].append(LOCAL.sub(lambda k: "." + k.group(1), l.split(";")[0].rstrip()))
            if re.match(r"\.Lfunc_end\d+:", l) or l.strip() == ".end_amdhsa_kernel":
                cur = None
    return {n: "\n".join(t) for n, t in out.items()}


def main(argv):
    if len(argv) < 2 or len(argv) % 2:
        sys.exit(__doc__)
    bad = 0
    for old, new in zip(argv[0::2], argv[1::2]):
        a, b = kernels(old), kernels(new)
        gone, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        differ = sorted(n for n in set(a) & set(b) if a[n] != b[n])
        print(f"{old} -> {new}: {len(a)} -> {len(b)} kernel symbols, {len(gone)} only in old, {len(added)} only in new, "
              f"{len(differ)} differing, {sum(t.count(chr(10)) + 1 for t in b.values())} lines compared")
        for tag, names in (("only in old", gone), ("only in new", added), ("differs", differ)):
            for n in names:
                print(f"  {tag}: {n}")
        bad += len(gone) + len(added) + len(differ)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
