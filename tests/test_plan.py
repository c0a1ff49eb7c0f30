"""The host-only planner (mpi-model_amd/csrc/mm_plan.cpp) on the CPU: compiled with plain
g++ into tests/plan_cli.cpp's line-protocol program, fed the plans an MI355X engine
recorded (tests/golden/plan_table.json, written by tools/plan_table.py), and held to the
planner's contract: pass lists that sum up and have kernels, the same plan on every rank
of a chain, segment plans that fit their slots, pass launches that cover the slab once
and stay inside the partials buffer."""
import json
import os

import numpy as np
import pytest

from plan_build import REPO, SANITIZE, build, run

CHAINS = [(64, 300, 2), (37, 130, 3), (27, 257, 3), (100, 488, 3), (41, 200, 8),
          (24, 257, 8), (16, 130, 8), (9, 124, 8), (300, 700, 2)]  # test_gpu_halo.py
C5_CHAINS = [(67, 300, 3), (40, 130, 8)]
PASSK_K = tuple(range(1, 11))
WIDE_K = (4, 8, 12, 16, 20)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("plan") / "plan_cli"), "plan_cli.cpp")


@pytest.fixture(scope="module")
def table():
    """The recorded cases, expanded from the file's shared lists (tools/plan_table.py pack):
    in, info by field, pass_kernel[k - 1], pass_plan as [n, [[length, count], ...]]."""
    with open(os.path.join(REPO, "tests", "golden", "plan_table.json")) as f:
        doc = json.load(f)

    def runs(s):
        return [[int(x.split("*")[0]), int((x + "*1").split("*")[1])] for x in s.split()]

    cases = []
    for c in doc["cases"]:
        H, W, x0, h, rank, nranks, program, env = c["in"]
        cases.append({
            "in": {"H": H, "W": W, "x_init": x0, "h": h, "rank": rank, "nranks": nranks,
                   "n_attr": 4 if program == "c5" else 1, "program": program, "env": env,
                   "ncu": doc["ncu"]},
            "info": dict(zip(doc["info_fields"], c["info"])),
            "pass_kernel": doc["kernels"][c["kernels"]],
            "pass_plan": [[n, runs(s)] for n, s in zip(doc["plan_n"], doc["plans"][c["plans"]])]})
    return cases


def ask(exe, lines):
    """Run the commands; one list of ints per answered query."""
    out = run(exe, input="\n".join(lines) + "\n")
    return [[int(x) for x in ln.split()] for ln in out.split("\n")[:-1]]


def slab_lines(H, W, G=1, g=0, program="diffuse", env=None, ncu=256, swpc=8, x0=None, h=None):
    """The `in` line (and its env lines) of slab g of G; slabs as mm_partition_rows."""
    if h is None:
        x0, h = g * H // G, (g + 1) * H // G - g * H // G
    na, mask, chains = (4, 15, 1) if program == "c5" else (1, 1, 0)
    return (["envclear"] + [f"env {k} {v}" for k, v in (env or {}).items()] +
            [f"in {H} {W} {x0} {h} {G} {na} {int(G > 1)} 1 {mask} {chains} {chains} {ncu} {swpc}"])


def case_lines(c):
    i = c["in"]
    return slab_lines(i["H"], i["W"], i["nranks"], i["rank"], i["program"], i["env"], i["ncu"],
                      c["info"]["seg_waves_per_cu"], i["x_init"], i["h"])


def unrle(r):
    return [k for k, n in r for _ in range(n)]


def table_script(table):
    lines = []
    for c in table:
        lines += case_lines(c) + ["info"] + [f"kern {k}" for k in range(1, 21)]
        lines += [f"plan {n}" for n, _ in c["pass_plan"]]
    return lines


def test_recorded_plans_replay_on_the_cpu(cli, table):
    """Every recorded output of the device engine, from the recorded inputs, CU count and
    slots per CU: integers, so equality."""
    assert len(table) > 100
    out = iter(ask(cli, table_script(table)))
    for c in table:
        kernel, spl, th, waves, swpc = next(out)
        i = c["info"]
        assert [kernel, spl, spl, th, waves] == [i["kernel"], i["steps_per_launch"], i["halo_depth"],
                                                 i["rows_per_wave"], i["waves_per_pass"]], c["in"]
        assert swpc == i["seg_waves_per_cu"] or kernel == 0, c["in"]
        for want in c["pass_kernel"]:
            assert next(out) == want, c["in"]
        for n, want in c["pass_plan"]:
            assert next(out) == unrle(want), (c["in"], n)


def test_recorded_plans_under_sanitizers(tmp_path, table):
    """The same program under ASan + UBSan (runtimes linked statically into the stand-alone
    program), once over the whole table and over a sweep of launches."""
    exe = build(str(tmp_path / "plan_cli_san"), "plan_cli.cpp", *SANITIZE)
    lines = table_script(table) + ["graph 1000 3 0", "graph 48 1 1"]
    for h in (1, 26, 27, 41, 120):
        lines += slab_lines(2 * h, 300, 2, 0, env={"MM_WIDE": 1})
        lines += [f"launch {k} {r}" for k in range(1, 21) for r in (0, 1)]
        lines += ["seg 3 20 1 1 600 3", "seg 2 10 16 1 600 293"]
    assert len(ask(exe, lines)) > 1000


def plans(cli, ins, ns):
    out = ask(cli, [ln for i in ins for ln in i + [f"plan {n}" for n in ns]])
    return [out[j * len(ns):(j + 1) * len(ns)] for j in range(len(ins))]


def test_planner_literals(cli):
    """The literal plans tests/test_gpu_large.py asserts on the device."""
    def plan(H, W, ns, env=None, **kw):
        return plans(cli, [slab_lines(H, W, env=env, **kw)], ns)[0]

    for H, W in ((8192, 32768), (16384, 16384)):
        assert plan(H, W, [20, 16, 12, 9, 0]) == [[20], [16], [12], [9], []]
        p = plan(H, W, [1000])[0]
        assert sum(p) == 1000 and len(p) <= 51 and p.count(20) >= 45
        assert all(k in WIDE_K or k <= 10 for k in p)
    assert plan(8192, 32768, [20, 45], {"MM_PASS_PLAN": 0}) == [[20], [20, 20, 5]]
    assert plan(8192, 32768, [20, 1000], {"MM_WIDE": 0}) == [[10, 10], [8] * 125]
    assert plan(16384, 16384, [20], {"MM_WIDE": 0}) == [[7, 7, 6]]  # 152 strips: no planner
    assert plan(4096, 4096, [20, 1000]) == [[8, 8, 4], [8] * 125]
    assert plan(8192, 8192, [20]) == [[7, 7, 6]]
    # the mid slab (4096 x 32768), in an 8-rank chain and alone: the K = 20 planner
    assert plan(32768, 32768, [20], G=8, g=0) == [[20]]
    assert plan(4096, 32768, [20]) == [[20]]
    assert plan(4096, 4096, [21], program="c5") == [[8, 8, 4, 1]]


def test_pass_plans_sum_and_have_kernels(cli, table):
    lines = []
    for c in table:
        lines += case_lines(c) + [f"kern {k}" for k in range(1, 21)]
    kern = ask(cli, lines)
    for j, c in enumerate(table):
        i = c["in"]
        has = {k for k in range(1, 21) if kern[20 * j + k - 1][0] in ((3,) if k > 10 or (i["n_attr"] > 1 and k > 2) else (2, 3))}
        if c["info"]["kernel"] == 0:
            has = {1}
        for n, r in c["pass_plan"]:
            p = unrle(r)
            assert sum(p) == n, (i, n)
            assert set(p) <= has, (i, n, p)
            if i["nranks"] > 1:
                assert all(k <= min(i["h"], i["H"] // i["nranks"]) for k in p), (i, n, p)


@pytest.mark.parametrize("H,W,G,program", [c + ("diffuse",) for c in CHAINS] + [c + ("c5",) for c in C5_CHAINS])
@pytest.mark.parametrize("env", [{}, {"MM_WIDE": 0}, {"MM_WIDE": 1}], ids=["auto", "wide0", "wide1"])
def test_every_rank_plans_the_same(cli, H, W, G, program, env):
    ns = list(range(46)) + [64, 100, 257]
    outs = []
    for g in range(G):
        lines = slab_lines(H, W, G, g, program, env)
        outs.append(ask(cli, lines + [f"plan {n}" for n in ns] + [f"kern {k}" for k in range(1, 21)]))
    assert all(o == outs[0] for o in outs)


def seg_count(n, ns, r, re):
    cr, ce = -(-n // r), -(-n // re)
    return np.where(ns < 3, ns * ce, 2 * ce + (ns - 2) * cr)


@pytest.mark.parametrize("na,kernel,ks", [(1, 2, PASSK_K), (1, 3, WIDE_K), (4, 2, (1, 2)), (4, 3, (4, 8))])
@pytest.mark.parametrize("seg_waves", [0, 2])
def test_segment_plans(cli, na, kernel, ks, seg_waves):
    """n rows 1..600 x strips x K x slots 1..16, on a device of 4 CUs (so the slots bind):
    even lengths, 8 <= th_edge <= th <= the row cap, the count the kernels' segment map
    gives, and no more segments than the wanted slots unless th is at its cap."""
    ncu, strips = 4, (1, 2, 3, 4, 5, 152, 293)
    env = {"MM_SEG_WAVES": seg_waves} if seg_waves else {}
    lines = slab_lines(600, 293 * 100, program="c5" if na == 4 else "diffuse", env=env, ncu=ncu)
    keys = [(k, s, ns) for k in ks for s in range(1, 17) for ns in strips]
    lines += [f"seg {kernel} {k} {s} 1 600 {ns}" for k, s, ns in keys]
    out = np.array(run(cli, input="\n".join(lines) + "\n").split(), dtype=np.int64).reshape(len(keys), 600, 4)
    n = np.arange(1, 601)[None, :]
    slots = np.array([s for _, s, _ in keys])[:, None]
    ns = np.array([x for _, _, x in keys])[:, None]
    th, the, count, maxr = (out[:, :, j] for j in range(4))
    assert np.all(th % 2 == 0) and np.all(the % 2 == 0)
    assert np.all(8 <= the) and np.all(the <= th) and np.all(th <= maxr)
    assert np.array_equal(count, seg_count(n, ns, th, the))
    want = np.maximum(1, int(seg_waves or 4) * ncu * slots)  # auto: at most 4 per slot
    assert np.all((count <= want) | (th == (maxr & ~1)))


def test_segments_at_the_offset_cap(cli):
    """Where passk_max_rows binds: the grid of tests/test_gpu_field_large.py (8200 x 32768 with
    MM_SEG_WAVES=0.001: per strip one segment of the cap and the rest) and 65536^2 under the
    default knobs. The cap is (2^31 / row bytes) less 3K + 2 * kSegPrefetch1 + 8 rows, cut to
    an even length."""
    tiny = {"MM_SEG_WAVES": 0.001}
    cases = [(8200, {**tiny, "MM_WIDE": 0, "MM_STEPS_PER_PASS": 10}, 2, 10, 8138),
             (8200, {**tiny, "MM_WIDE": 1, "MM_STEPS_PER_PASS": 20}, 3, 20, 8108),
             (65536, {}, 3, 20, 4012), (65536, {"MM_WIDE": 0}, 2, 8, 4048)]
    for H, env, kernel, k, want in cases:
        W = 32768 if H == 8200 else H
        info, cap, l0, l1 = ask(cli, slab_lines(H, W, env=env) +
                                ["info", f"cap {k}", f"launch {k} 0", f"launch {k} 1"])
        assert cap == [want, (1 << 31) // (W * 8) - (3 * k + 2 * 8 + 8), want & ~1], (H, env)
        assert info[:3] == [kernel, k, want & ~1], (H, env, info)
        for l in (l0, l1):
            assert (l[0], l[3], l[4], l[5]) == (kernel, 0, H, want & ~1), (H, env, l)
            assert 8 <= l[6] <= l[5]
        if H == 8200:  # two segments per interior strip, the second ends at the last row
            assert 16 <= H - info[2] <= 92


@pytest.mark.parametrize("env,ks", [({"MM_PASSK": 0}, (1,)), ({"MM_WIDE": 0}, PASSK_K),
                                    ({"MM_WIDE": 1}, tuple(range(1, 21))),
                                    ({"MM_WIDE": 1, "MM_BORDER_SEGMENTS": 0}, WIDE_K)],
                         ids=["onestep", "passk", "wide", "wide_kborders"])
@pytest.mark.parametrize("W,program", [(300, "diffuse"), (1000, "diffuse"), (300, "c5")])
def test_pass_launches_cover_the_slab(cli, env, ks, W, program):
    """h = 1..120 in a 2-slab chain: interior and border ranges disjoint, covering [0, h)
    exactly, each border >= depth rows, the border's partials after the interior's, and
    the pass's partials (units x K x attributes doubles) within the buffer's size."""
    na = 4 if program == "c5" else 1
    ks = [k for k in ks if na == 1 or k <= 2 or k in (4, 8)]
    lines, keys = [], []
    for h in range(1, 121):
        lines += slab_lines(2 * h, W, 2, 0, program, env)
        for k in ks:
            for red in (0, 1):
                lines.append(f"launch {k} {red}")
                keys.append((h, k))
    for (h, k), o in zip(keys, ask(cli, lines)):
        kernel, split, depth, ilo, ihi, ith, ithe, icount, ibase = o[:9]
        blo, bhi, blo2, bhi2, bth, bcount, bbase, total, need = o[9:]
        assert kernel == (0 if "MM_PASSK" in env else 3 if env["MM_WIDE"] and (k in (4, 8) or (na == 1 and k in WIDE_K)) else 2)
        assert depth == (k if kernel else 1) and split == (h >= 2 * depth + 1), (h, k)
        assert ibase == 0 and total == icount + bcount
        if split:
            assert (blo, bhi, blo2, bhi2) == (0, ilo, ihi, h), (h, k, o)
            assert depth <= bhi - blo == bhi2 - blo2 and ilo <= ihi, (h, k, o)
            assert bbase == icount and bcount > 0
        else:
            assert (ilo, ihi, bcount) == (0, h, 0), (h, k, o)
        assert total * (k * na if kernel else na) <= need, (h, k, o)
