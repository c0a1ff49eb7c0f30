"""mm_geom.hpp's geometry of the K-step closed pass (mm_closedk_kernel), evaluated from the
header's own text so that the tests move with it: the integer constants and the one-line
`return` functions named in FUNCS. A plain module, not a conftest."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("field_ring", "fieldk_max_rows", "closedk_halo_cols", "closedk_out_cols", "closed_ring",
         "closedk_max_rows")


def geom():
    text = open(os.path.join(REPO, "mpi-model_amd", "csrc", "mm_geom.hpp")).read()
    ns = {n: int(v) for n, v in re.findall(r"constexpr int (\w+) = (\d+);", text)}
    for name in FUNCS:
        m = re.search(r"\b%s\(([^)]*)\)\s*\{\s*return\s+(.*?);\s*\}" % name, text, re.S)
        assert m, name
        params = [p.split()[-1] for p in m.group(1).split(",")]
        expr = re.sub(r"(\d)LL\b", r"\1", m.group(2)).replace("/", "//")
        ns[name] = eval("lambda %s: %s" % (", ".join(params), expr), ns)
    return ns
