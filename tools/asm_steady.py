#!/usr/bin/env python3
"""Steady-state loops of one wide-kernel instance in a hipcc -S file: for each loop whose
body holds the full level work of B rows (fp64 count = 5 x columns x levels x rows), its
instruction mix (tools/asm_loops.py's counters) -- the evidence that the production loops
issue the modelled 5 fp64 per cell and level (the box-sum step of round 6, 22 on an even row
and 18 on the odd row after it at C = 4) and no scratch.

The loops are found by their fp64 count, which the bit-exact contract fixes, and not by how
the +-1 column neighbours travel: 4 shifts per level-row, as DPP moves (VALU) or as
ds_bpermute_b32 (the DS pipe; mm_wide.hpp MM_WIDE6_SHIFT), so SHIFTS_PER_TRIP = 4 x levels x
rows names the trip and the fp64 count is 5 C / 4 times it: 5 x at C = 4 (the default),
7.5 x at C = 6 -- mm_wide6_kernel's interior loops, 600 fp64 per 4 rows x 5 levels:
`asm_steady.py FILE.s mm_wide6_kernel 80 6`. (The same kernel's frame loops are the C = 4
ones: `... 80`.) Every line reports dpp, bpermute, waitcnt and scratch, 0 included.

usage: asm_steady.py FILE.s KERNEL_SUBSTRING SHIFTS_PER_TRIP [COLUMNS_PER_LANE]
"""
import re
import sys

sys.path.insert(0, __import__("os").path.dirname(__file__))
from asm_loops import kernel_lines, mix  # noqa: E402

ALWAYS = ("dpp", "bpermute", "waitcnt", "scratch")


def main():
    path, sub, shifts = sys.argv[1], sys.argv[2], int(sys.argv[3])
    cols = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    f64 = 5 * cols * shifts // 4  # 5 C fp64 per 4 shifts
    body = kernel_lines(path, sub)
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            labels[m.group(1)] = i
    seen = set()
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\S+)|s_branch\s+(\.LBB\S+)", l)
        if not m:
            continue
        tgt = m.group(1) or m.group(2)
        if tgt in labels and labels[tgt] < i:
            c = mix(body[labels[tgt]:i + 1])
            for k in ALWAYS:
                c.setdefault(k, 0)
            key = tuple(sorted(c.items()))
            if c.get("f64", 0) == f64 and key not in seen:
                seen.add(key)
                role = "first wave (loads)" if c.get("bload") else (
                    "last wave (stores)" if c.get("bstore") else "middle wave (LDS in/out)")
                print(f"{role}: " + ", ".join(f"{k}={v}" for k, v in sorted(c.items())))


if __name__ == "__main__":
    main()
