#!/usr/bin/env python3
"""Record what the engine plans, for a table of slabs and MM_* settings, into
tests/golden/plan_table.json (tests/test_plan.py replays it on the CPU planner).

Engine creation and queries only -- no step runs. Uses the public Python API alone
(Engine, add_diffuse, add_transfer, info, pass_plan, pass_kernel), so the same script runs
against any build of the library; a refactor of the planner must reproduce the committed
file byte for byte:

    python3 tools/plan_table.py [--out tests/golden/plan_table.json]
"""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpi-model_amd"))
import mpimodel as mm  # noqa: E402

C5_FLOWS = [(2, 0, 1, 0.05), (2, 1, 2, 0.03), (2, 2, 3, 0.02), (2, 3, 0, 0.01),
            (1, 0, 0, 0.1), (1, 1, 1, 0.1), (1, 2, 2, 0.05), (1, 3, 3, 0.2)]
CHAINS = [(64, 300, 2), (37, 130, 3), (27, 257, 3), (100, 488, 3), (41, 200, 8),
          (24, 257, 8), (16, 130, 8), (9, 124, 8), (300, 700, 2)]  # tests/test_gpu_halo.py
C5_CHAINS = [(67, 300, 3), (40, 130, 8)]
PLAN_N = list(range(46)) + [64, 100, 200, 256, 257, 1000]
INFO_FIELDS = ["kernel", "steps_per_launch", "halo_depth", "rows_per_wave", "waves_per_pass",
               "seg_waves_per_cu"]


def rle(xs):
    out = []
    for x in xs:
        if out and out[-1][0] == x:
            out[-1][1] += 1
        else:
            out.append([x, 1])
    return out


def slab(H, W, G=1, g=0, program="diffuse"):
    return dict(H=H, W=W, G=G, g=g, program=program)


def case_list():
    cases = []

    def add(s, env=None):
        cases.append(dict(s, env=dict(env or {})))

    # the benchmark's grids (BASELINE.json): c2 / c5 4096^2 per GPU, c3 32768^2 in slabs,
    # c4 16384^2 per GPU; rank 0 and a middle rank of each chain
    for G in (1, 2, 4, 8):
        for g in sorted({0, G // 2}):
            add(slab(32768, 32768, G, g))
            add(slab(16384 * G, 16384, G, g))
            add(slab(4096 * G, 4096, G, g))
            add(slab(4096 * G, 4096, G, g, "c5"))
    for H, W in [(16384, 16384), (8192, 32768), (4096, 32768), (8192, 8192), (4096, 4096),
                 (2048, 2048), (1024, 1024)]:
        if (H, W) not in [(16384, 16384), (4096, 4096)]:  # already above
            add(slab(H, W))
    for H, W, G in CHAINS:
        for g in range(G):
            add(slab(H, W, G, g))
    for H, W, G in C5_CHAINS:
        for g in range(G):
            add(slab(H, W, G, g, "c5"))
    # the settings, on a few large and small slabs
    some = [slab(32768, 32768), slab(32768, 32768, 8, 4), slab(4096, 32768), slab(4096, 4096),
            slab(4096, 4096, program="c5"), slab(1024, 1024), slab(64, 300, 2, 0),
            slab(41, 200, 8, 3), slab(67, 300, 3, 1, "c5")]
    for env in [{"MM_WIDE": 0}, {"MM_WIDE": 1}, {"MM_PASS_PLAN": 0}, {"MM_PASSK": 0},
                {"MM_SEG_WAVES": 2}, {"MM_SEG_EDGE": 0.3}]:
        for s in some:
            add(s, env)
    for k in list(range(1, 11)) + [12, 16, 20]:
        for s in [slab(32768, 32768), slab(4096, 4096), slab(64, 300, 2, 0),
                  slab(4096, 4096, program="c5")]:
            add(s, {"MM_STEPS_PER_PASS": k})
    for k in (4, 8, 12, 16, 20):
        for s in [slab(4096, 4096), slab(64, 300, 2, 0)]:
            add(s, {"MM_WIDE": 1, "MM_STEPS_PER_PASS": k})
    return cases


def record(c, ncu):
    H, W, G, g = c["H"], c["W"], c["G"], c["g"]
    na = 4 if c["program"] == "c5" else 1
    x0, h = mm.partition_rows(H, G, g)
    for k, v in c["env"].items():
        os.environ[k] = str(v)
    try:
        eng = mm.Engine(H, W, x0, h, n_attr=na, rank=g, nranks=G,
                        halo_mode=mm.MM_HALO_HOST if G > 1 else mm.MM_HALO_NONE)
    finally:
        for k in c["env"]:
            del os.environ[k]
    with eng as e:
        if na == 1:
            e.add_diffuse(0, 0.1)
        else:
            for kind, a, b, r in C5_FLOWS:
                e.add_diffuse(a, r) if kind == 1 else e.add_transfer(a, b, r)
        info = e.info()
        return {
            "in": {"H": H, "W": W, "x_init": x0, "h": h, "rank": g, "nranks": G,
                   "halo": "host" if G > 1 else "none", "n_attr": na, "program": c["program"],
                   "env": {k: str(v) for k, v in c["env"].items()}, "ncu": ncu},
            "info": {k: info[k] for k in INFO_FIELDS},
            "pass_kernel": [list(e.pass_kernel(k)) for k in range(1, 21)],
            "pass_plan": [[n, rle(e.pass_plan(n))] for n in PLAN_N],
        }


def pack(rows, ncu):
    """The file: every distinct list of plans (one string per n of PLAN_N, "8*2 4" = passes
    of 8, 8, 4) and of pass_kernel answers once, and one line per case that points at them
    (tests/test_plan.py's `table` fixture expands it again)."""
    def dumps(x):
        return json.dumps(x, sort_keys=True, separators=(",", ":"))

    def index(seen, x):
        if x not in seen:
            seen.append(x)
        return seen.index(x)

    plans, kernels, cases = [], [], []
    for r in rows:
        i = r["in"]
        p = [" ".join(f"{k}*{n}" if n > 1 else str(k) for k, n in runs) for _, runs in r["pass_plan"]]
        cases.append({"in": [i["H"], i["W"], i["x_init"], i["h"], i["rank"], i["nranks"],
                             i["program"], i["env"]],
                      "info": [r["info"][k] for k in INFO_FIELDS],
                      "plans": index(plans, p), "kernels": index(kernels, r["pass_kernel"])})
    head = {"ncu": ncu, "plan_n": PLAN_N, "info_fields": INFO_FIELDS}
    parts = [f'"{k}":{dumps(v)}' for k, v in head.items()]
    for name, items in (("plans", plans), ("kernels", kernels), ("cases", cases)):
        parts.append(f'"{name}":[\n' + ",\n".join(dumps(x) for x in items) + "\n]")
    return "{\n" + ",\n".join(parts) + "\n}\n"


def cu_count(device=0):
    """Compute units of the device, asked of the HIP runtime the engine itself loaded."""
    mm.lib()
    with open("/proc/self/maps") as f:
        hip = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})[0]
    v = ctypes.c_int()
    rc = ctypes.CDLL(hip).hipDeviceGetAttribute(ctypes.byref(v), 63, device)  # ...MultiprocessorCount
    assert rc == 0 and v.value > 0, (rc, v.value)
    return v.value


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "plan_table.json"))
    args = ap.parse_args()
    ncu = cu_count()
    rows = [record(c, ncu) for c in case_list()]
    with open(args.out, "w") as f:
        f.write(pack(rows, ncu))
    print(f"{len(rows)} cases -> {args.out}")


if __name__ == "__main__":
    main()
