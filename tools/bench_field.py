#!/usr/bin/env python3
"""Rate-field passes on one grid, in one process: the one-step pass (mm_field_kernel,
MM_FIELD_STEPS=1), the K-step pass for every built K (mm_fieldk_kernel, MM_FIELD_STEPS=K)
and the one-step uniform kernel (mm_pass_kernel, MM_PASSK=0). HIP-event time per pass and
per step, GCUPS, algorithmic bytes per cell-update (24 / K for a field pass: read v, read f,
write v' once per K steps; 16 for the uniform pass) and the achieved algorithmic bytes/s of
a launch, as a fraction of the 8 TB/s HBM peak; the arms alternate `--rounds` times.
Needs a GPU; nothing here falls back.

  python tools/bench_field.py [--sizes 2048,4096,8192,16384] [--warmup 20] [--steps 200]
                              [--rounds 3] [--self-halo] [--closed [--self-halo]]

A size is N (an N x N grid) or HxW. Every arm also reports wall_step_us: host time per step
of an untimed run of the same length (graph replay where the engine captures), the measure
that includes a split pass's border launches and exchange, which the HIP events around the
interior launch do not.

--self-halo creates the engines with MM_HALO_RCCL, MM_SELF_HALO=1 and MM_FIELD_HALO=4: one
rank that exchanges its border rows with itself, the only way to run the split schedule
(interior segments beside the exchange, border blocks after it) with RCCL on one GPU. The
field arms alone run; the summary compares wall_step_us, and the last line derives the auto
rule of a slab with a halo: the smallest shape at which split K = 4 beat the split one-step
arm of the same run in every round.

--closed runs the closed rate-field pass (MM_FLOW_DIFFUSE_CLOSED, mm_closed_kernel) instead
of the K arms: `field`, the one-step field pass as the baseline of the same run; `closed`, the
same engine shape and the same mm_rate_field_fill(0.1) field, every cell open (the ballot
takes the division-free body on every interior row); `closed_disc`, that field with a disc
of walls of about a quarter of the grid in its middle (rows that cross the disc's rim run the
general body, rows inside it the body of rows in which nothing emits); `closed2` ..
`closedK` and `closed2_disc` .. `closedK_disc`, the K-step closed pass (mm_closedk_kernel,
MM_CLOSED_STEPS=K) for every built K on those two fields; and `field2` .. `fieldK`, the K-step
field pass of the same run. The summary's bytes_ratio is the all-open closed pass's bytes/s
over the field pass's (target: >= 0.9); a K arm's x_one_step is its time per step over the
one-step closed arm's of the same field (`closed` / `closed_disc`), beats_one_step whether it
was below it in every round, pass_x its time per pass over that arm's, and over_fieldk the
all-open pass's time over the field kind's pass of the same K.

--closed --self-halo runs the closed arms split: every `closed*` engine is created with
MM_HALO_RCCL, MM_SELF_HALO=1 and MM_CLOSED_HALO=K+1 (the one-step arms: 2), so its passes run
interior segments beside the exchange and border blocks after it; `closedK_unsplit` and
`closedK_disc_unsplit` are the same passes on an engine without a halo. The arms are compared
by wall_step_us: a K arm's speedup is the split one-step arm's time per step over its own,
beats_one_step whether it was below it in every round, over_unsplit its time over the unsplit
arm's of the same K.

Every arm times at least --steps steps, rounded up to a multiple of its K. Prints one JSON
line per arm and round, then per size a summary line. For the K arms the summary holds the
model of DESIGN.md 4.1 -- 24/K * 128/out_cols(K) B per cell-update moved at the one-step
field pass's measured bytes/s -- and the share of it the kernel reached; bytes_ratio is the
one-step field pass's bytes/s over the uniform pass's (target: >= 0.9). The last line
derives the auto rule of MM_FIELD_STEPS from the table: the K of the best time per step at
8192^2 (the largest size, if 8192 was not run) and the smallest size at which that K beat
the one-step pass in every round.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "mpi-model_amd"))
import mpimodel as mm  # noqa: E402

mm.lib()
PEAK = 8e12  # B/s, MI355X HBM3E
KS = list(range(2, mm.FIELD_MAX_STEPS + 1))
CLOSED_KS = list(range(2, mm.CLOSED_MAX_STEPS + 1))


def out_cols(k):
    return 128 - 4 * ((k + 1) // 2)


def engine(H, W, k, self_halo=False):
    """k = 0: the uniform one-step arm; 1: the one-step field pass; >= 2: the K-step pass."""
    env = {"MM_PASSK": "0"} if k == 0 else {"MM_FIELD_STEPS": str(k)}
    if self_halo:
        env.update(MM_SELF_HALO="1", MM_FIELD_HALO=str(mm.FIELD_MAX_STEPS))
    old = {name: os.environ.get(name)
           for name in ("MM_PASSK", "MM_FIELD_STEPS", "MM_SELF_HALO", "MM_FIELD_HALO")}
    for name in old:
        os.environ.pop(name, None)
    os.environ.update(env)
    try:
        if self_halo:
            e = mm.Engine(H, W, halo_mode=mm.MM_HALO_RCCL, comm_id_bytes=mm.comm_id())
        else:
            e = mm.Engine(H, W)
    finally:
        for name, v in old.items():
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v
    e.fill_random(0)
    if k:
        e.rate_field_fill(0.1)
        e.add_diffuse_field(0)
    else:
        e.add_diffuse(0, 0.1)
    info = e.info()
    want = (4, k) if k >= 2 else (0, 1)
    assert (info["kernel"], info["steps_per_launch"]) == want, info
    return e


def closed_engine(H, W, disc, k=1, self_halo=False):
    """The closed pass on the field of the `field` arm, k steps per pass; disc: a disc of walls
    of a quarter of the grid's cells in the middle; self_halo: one RCCL rank that exchanges with
    itself, created with MM_CLOSED_HALO = k + 1 (the split schedule)."""
    old = {name: os.environ.pop(name, None) for name in ("MM_PASSK", "MM_FIELD_STEPS", "MM_SELF_HALO",
                                                         "MM_FIELD_HALO", "MM_CLOSED_STEPS",
                                                         "MM_CLOSED_HALO")}
    env = {"MM_CLOSED_STEPS": str(k)}
    if self_halo:
        env.update(MM_SELF_HALO="1", MM_CLOSED_HALO=str(k + 1))
    try:
        os.environ.update(env)
        if self_halo:
            e = mm.Engine(H, W, halo_mode=mm.MM_HALO_RCCL, comm_id_bytes=mm.comm_id())
        else:
            e = mm.Engine(H, W)
    finally:
        for name in env:
            os.environ.pop(name, None)
        os.environ.update({name: v for name, v in old.items() if v is not None})
    e.fill_random(0)
    e.rate_field_fill(0.1)
    if disc:
        import numpy as np
        r2 = H * W / (4.0 * np.pi)
        y = (np.arange(W) - (W - 1) / 2.0) ** 2
        chunk = max(1, (1 << 24) // W)
        for x0 in range(0, H, chunk):
            x = (np.arange(x0, min(H, x0 + chunk)) - (H - 1) / 2.0) ** 2
            e.rate_field_upload(np.where(x[:, None] + y[None, :] <= r2, 0.0, 0.1), row0=x0)
    e.add_diffuse_closed(0)
    info = e.info()
    want = (5, k, 1) if k >= 2 else (0, 1, 1)
    assert (info["kernel"], info["steps_per_launch"], info["n_passes"]) == want, info
    return e


def run_closed_self_halo(size, a):
    """The closed arms on one self-halo rank (split passes) beside the unsplit K-step arms,
    compared by wall_step_us."""
    H, W = shape_of(size)
    engines, arms = {}, {}
    for tail, disc in (("", False), ("_disc", True)):
        engines["closed" + tail] = closed_engine(H, W, disc, 1, True)
        arms["closed" + tail] = 1
        for k in CLOSED_KS:
            engines["closed%d%s" % (k, tail)] = closed_engine(H, W, disc, k, True)
            engines["closed%d%s_unsplit" % (k, tail)] = closed_engine(H, W, disc, k)
            arms["closed%d%s" % (k, tail)] = arms["closed%d%s_unsplit" % (k, tail)] = k
    res = {name: [] for name in engines}
    for rnd in range(a.rounds):
        for name, e in engines.items():
            r = measure(e, H * W, arms[name], a.warmup, a.steps)
            res[name].append(r)
            print(json.dumps({"arm": name, "self_halo": not name.endswith("_unsplit"), "round": rnd,
                              "H": H, "W": W, **r}), flush=True)
    for e in engines.values():
        e.close()
    out = {"summary": "closed rate-field passes, self-halo (split)", "H": H, "W": W,
           "rounds": a.rounds, "arms": {}}
    for name, rows in res.items():
        out["arms"][name] = {key: span(rows, key) for key in ("pass_us", "step_us", "wall_step_us")}
    for k in CLOSED_KS:
        for tail in ("", "_disc"):
            name, one, flat = "closed%d%s" % (k, tail), "closed" + tail, "closed%d%s_unsplit" % (k, tail)
            arm = out["arms"][name]
            arm["speedup"] = round(out["arms"][one]["wall_step_us"]["mean"] /
                                   arm["wall_step_us"]["mean"], 3)
            ratios = [c["wall_step_us"] / r["wall_step_us"] for r, c in zip(res[name], res[one])]
            arm["speedup_range"] = [round(min(ratios), 2), round(max(ratios), 2)]
            arm["beats_one_step"] = all(r["wall_step_us"] < c["wall_step_us"]
                                        for r, c in zip(res[name], res[one]))
            over = [r["wall_step_us"] / u["wall_step_us"] for r, u in zip(res[name], res[flat])]
            arm["over_unsplit"] = [round(min(over), 3), round(max(over), 3)]
    print(json.dumps(out), flush=True)
    return out


def run_closed(size, a):
    """The closed pass, all open and around a disc of walls, beside the one-step field pass."""
    H, W = shape_of(size)
    engines = {"field": engine(H, W, 1), "closed": closed_engine(H, W, False),
               "closed_disc": closed_engine(H, W, True)}
    arms = {name: 1 for name in engines}
    for k in CLOSED_KS:
        engines["closed%d" % k] = closed_engine(H, W, False, k)
        engines["closed%d_disc" % k] = closed_engine(H, W, True, k)
        arms["closed%d" % k] = arms["closed%d_disc" % k] = k
        if k in KS:
            engines["field%d" % k] = engine(H, W, k)
            arms["field%d" % k] = k
    res = {name: [] for name in engines}
    for rnd in range(a.rounds):
        for name, e in engines.items():
            r = measure(e, H * W, arms[name], a.warmup, a.steps)
            res[name].append(r)
            print(json.dumps({"arm": name, "round": rnd, "H": H, "W": W, **r}), flush=True)
    for e in engines.values():
        e.close()
    ratios = [c["TBps"] / f["TBps"] for c, f in zip(res["closed"], res["field"])]
    out = {"summary": "closed rate-field pass", "H": H, "W": W, "rounds": a.rounds,
           "bytes_ratio": {"min": round(min(ratios), 3), "max": round(max(ratios), 3),
                           "mean": round(sum(ratios) / len(ratios), 3)},
           "target_met": min(ratios) >= 0.9, "arms": {}}
    for name, rows in res.items():
        out["arms"][name] = {key: span(rows, key) for key in
                             ("pass_us", "step_us", "wall_step_us", "GCUPS", "bytes_per_cell_update",
                              "TBps", "of_peak")}
    for k in CLOSED_KS:
        for tail in ("", "_disc"):
            name, one = "closed%d%s" % (k, tail), "closed" + tail
            arm = out["arms"][name]
            arm["x_one_step"] = round(arm["step_us"]["mean"] / out["arms"][one]["step_us"]["mean"], 3)
            arm["pass_x"] = round(arm["pass_us"]["mean"] / out["arms"][one]["pass_us"]["mean"], 3)
            # faster per step than the one-step closed pass of the same round, in every round
            arm["beats_one_step"] = all(r["step_us"] < c["step_us"]
                                        for r, c in zip(res[name], res[one]))
        if "field%d" % k in res:
            out["arms"]["closed%d" % k]["over_fieldk"] = round(
                out["arms"]["closed%d" % k]["pass_us"]["mean"] /
                out["arms"]["field%d" % k]["pass_us"]["mean"], 3)
    print(json.dumps(out), flush=True)
    return out


def measure(e, cells, k, warmup, steps):
    k = max(k, 1)
    steps = -(-steps // k) * k
    e.set_timing(False)
    e.run(warmup)
    e.synchronize()
    e.set_timing(True)
    e.run(steps)
    e.synchronize()
    n, ms, nbytes = e.timing()
    e.set_timing(False)
    assert n == steps // k, (n, steps, k)
    us = ms / n * 1e3
    bps = nbytes / (us * 1e-6)
    # the same run untimed, by the host's clock: every launch of a split pass and its exchange
    e.prepare(steps)
    e.run(warmup)
    e.synchronize()
    t0 = time.perf_counter()
    e.run(steps)
    e.synchronize()
    wall = (time.perf_counter() - t0) / steps * 1e6
    return {"steps": steps, "pass_us": round(us, 2), "step_us": round(us / k, 2),
            "wall_step_us": round(wall, 2),
            "GCUPS": round(cells * k / us / 1e3, 1),
            "bytes_per_cell_update": round(nbytes / cells / k, 2), "TBps": round(bps / 1e12, 3),
            "of_peak": round(bps / PEAK, 3)}


def span(rows, key):
    v = [r[key] for r in rows]
    return {"min": min(v), "max": max(v), "mean": round(sum(v) / len(v), 3)}


def shape_of(size):
    h, _, w = str(size).partition("x")
    return int(h), int(w or h)


def run_self_halo(size, a):
    """The field arms on one self-halo rank: split passes, compared by wall_step_us."""
    H, W = shape_of(size)
    arms = {"field": 1, **{"field%d" % k: k for k in KS}}
    engines = {name: engine(H, W, k, True) for name, k in arms.items()}
    res = {name: [] for name in arms}
    for rnd in range(a.rounds):
        for name, e in engines.items():
            r = measure(e, H * W, arms[name], a.warmup, a.steps)
            res[name].append(r)
            print(json.dumps({"arm": name, "self_halo": True, "round": rnd, "H": H, "W": W, **r}),
                  flush=True)
    for e in engines.values():
        e.close()
    out = {"summary": "rate-field passes, self-halo (split)", "H": H, "W": W, "rounds": a.rounds,
           "arms": {}}
    for name, rows in res.items():
        out["arms"][name] = {key: span(rows, key) for key in ("pass_us", "step_us", "wall_step_us")}
    for k in KS:
        arm = out["arms"]["field%d" % k]
        arm["speedup"] = round(out["arms"]["field"]["wall_step_us"]["mean"] /
                               arm["wall_step_us"]["mean"], 3)
        arm["beats_one_step"] = all(r["wall_step_us"] < f["wall_step_us"]
                                    for r, f in zip(res["field%d" % k], res["field"]))
    print(json.dumps(out), flush=True)
    return out


def run_size(size, a):
    H, W = shape_of(size)
    arms = {"field": 1, **{"field%d" % k: k for k in KS}, "uniform": 0}
    engines = {name: engine(H, W, k) for name, k in arms.items()}
    res = {name: [] for name in arms}
    for rnd in range(a.rounds):
        for name, e in engines.items():
            r = measure(e, H * W, arms[name], a.warmup, a.steps)
            res[name].append(r)
            print(json.dumps({"arm": name, "round": rnd, "H": H, "W": W, **r}), flush=True)
    for e in engines.values():
        e.close()

    ratios = [f["TBps"] / u["TBps"] for f, u in zip(res["field"], res["uniform"])]
    out = {"summary": "rate-field passes", "H": H, "W": W, "rounds": a.rounds,
           "bytes_ratio": {"min": round(min(ratios), 3), "max": round(max(ratios), 3),
                           "mean": round(sum(ratios) / len(ratios), 3)},
           "target_met": min(ratios) >= 0.9, "arms": {}}
    for name, rows in res.items():
        out["arms"][name] = {key: span(rows, key) for key in
                             ("pass_us", "step_us", "wall_step_us", "GCUPS",
                              "bytes_per_cell_update", "TBps", "of_peak")}
    bps1 = out["arms"]["field"]["TBps"]["mean"] * 1e12
    for k in KS:
        arm = out["arms"]["field%d" % k]
        model_bytes = 24.0 / k * 128.0 / out_cols(k)
        model_us = H * W * model_bytes / bps1 * 1e6
        arm["model_bytes_per_cell_update"] = round(model_bytes, 3)
        arm["model_step_us"] = round(model_us, 2)
        arm["share_of_model"] = round(model_us / arm["step_us"]["mean"], 3)
        arm["speedup"] = round(out["arms"]["field"]["step_us"]["mean"] / arm["step_us"]["mean"], 3)
        # faster than the one-step pass of the same round, in every round
        arm["beats_one_step"] = all(r["step_us"] < f["step_us"]
                                    for r, f in zip(res["field%d" % k], res["field"]))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,4096,8192,16384")
    ap.add_argument("--size", default="", help="one size or several (instead of --sizes)")
    ap.add_argument("--self-halo", action="store_true",
                    help="MM_HALO_RCCL + MM_SELF_HALO=1 + MM_FIELD_HALO=4: the split schedule")
    ap.add_argument("--closed", action="store_true",
                    help="the closed pass, one step and K steps per pass (all open, and around a "
                         "disc of walls), beside the field pass")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    sizes = (a.size or a.sizes).split(",")
    cells = lambda s: shape_of(s)[0] * shape_of(s)[1]  # noqa: E731
    if a.closed:
        for size in sizes:
            (run_closed_self_halo if a.self_halo else run_closed)(size, a)
        return
    if a.self_halo:
        table = {size: run_self_halo(size, a) for size in sizes}
        kmax = "field%d" % KS[-1]
        wins = [s for s in sorted(table, key=cells) if table[s]["arms"][kmax]["beats_one_step"]]
        lost = [s for s in sorted(table, key=cells) if s not in wins]
        print(json.dumps({"auto_rule": "MM_FIELD_STEPS unset, slab with a halo", "K": KS[-1],
                          "threshold_cells": max(cells(wins[0]), 1 << 16) if wins else None,
                          "shapes_won": wins, "shapes_lost": lost}), flush=True)
        return
    table = {size: run_size(size, a) for size in sizes}

    ref = "8192" if "8192" in table else max(table, key=cells)
    best = min(KS, key=lambda k: table[ref]["arms"]["field%d" % k]["step_us"]["mean"])
    wins = [s for s in sorted(table, key=cells)
            if table[s]["arms"]["field%d" % best]["beats_one_step"]]
    print(json.dumps({"auto_rule": "MM_FIELD_STEPS unset", "reference_size": ref, "K": best,
                      "threshold_cells": max(cells(wins[0]), 1 << 16) if wins else None,
                      "sizes_won": wins}), flush=True)


if __name__ == "__main__":
    main()
