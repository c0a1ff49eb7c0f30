#!/usr/bin/env python3
"""Rate-field pass (mm_field_kernel) against the one-step uniform kernel (mm_pass_kernel,
MM_PASSK=0) on the same grid, in one process: HIP-event time per pass, GCUPS and achieved
algorithmic bytes/s -- 24 B per cell for the field pass (read v, read f, write v'), 16 B for
the uniform pass -- as a fraction of the 8 TB/s HBM peak, alternated `--rounds` times.
Needs a GPU; nothing here falls back.

  python tools/bench_field.py [--size 8192] [--warmup 20] [--steps 200] [--rounds 3]

Prints one JSON line per arm and round, then a summary line: bytes_ratio is the field pass's
bytes/s over the uniform pass's (target: >= 0.9).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpi-model_amd"))
import mpimodel as mm  # noqa: E402

mm.lib()
PEAK = 8e12  # B/s, MI355X HBM3E


def engine(H, W, field):
    old = os.environ.get("MM_PASSK")
    os.environ["MM_PASSK"] = "0"  # the uniform arm: one step per pass; the field arm is anyway
    try:
        e = mm.Engine(H, W)
    finally:
        if old is None:
            os.environ.pop("MM_PASSK", None)
        else:
            os.environ["MM_PASSK"] = old
    e.fill_random(0)
    if field:
        e.rate_field_fill(0.1)
        e.add_diffuse_field(0)
    else:
        e.add_diffuse(0, 0.1)
    info = e.info()
    assert info["kernel"] == 0 and info["steps_per_launch"] == 1, info
    return e


def measure(e, cells, warmup, steps):
    e.set_timing(False)
    e.run(warmup)
    e.synchronize()
    e.set_timing(True)
    e.run(steps)
    e.synchronize()
    n, ms, nbytes = e.timing()
    e.set_timing(False)
    assert n == steps, (n, steps)
    us = ms / n * 1e3
    bps = nbytes / (us * 1e-6)
    return {"pass_us": round(us, 2), "GCUPS": round(cells / us / 1e3, 1),
            "bytes_per_cell": round(nbytes / cells, 1), "TBps": round(bps / 1e12, 3),
            "of_peak": round(bps / PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    H = W = a.size
    arms = {"field": engine(H, W, True), "uniform": engine(H, W, False)}
    res = {k: [] for k in arms}
    for rnd in range(a.rounds):
        for name, e in arms.items():
            r = measure(e, H * W, a.warmup, a.steps)
            res[name].append(r)
            print(json.dumps({"arm": name, "round": rnd, "H": H, "W": W, **r}), flush=True)
    for e in arms.values():
        e.close()

    def span(name, key):
        v = [r[key] for r in res[name]]
        return {"min": min(v), "max": max(v), "mean": round(sum(v) / len(v), 3)}

    ratios = [f["TBps"] / u["TBps"] for f, u in zip(res["field"], res["uniform"])]
    print(json.dumps({"summary": "field vs uniform one-step pass", "H": H, "W": W,
                      "steps": a.steps, "rounds": a.rounds,
                      "field_pass_us": span("field", "pass_us"),
                      "uniform_pass_us": span("uniform", "pass_us"),
                      "field_TBps": span("field", "TBps"), "uniform_TBps": span("uniform", "TBps"),
                      "field_of_peak": span("field", "of_peak"),
                      "uniform_of_peak": span("uniform", "of_peak"),
                      "bytes_ratio": {"min": round(min(ratios), 3), "max": round(max(ratios), 3),
                                      "mean": round(sum(ratios) / len(ratios), 3)},
                      "target_met": min(ratios) >= 0.9}), flush=True)


if __name__ == "__main__":
    main()
