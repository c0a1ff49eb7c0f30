"""GPU: the fused six-column K = 20 pass (mm_wide6_kernel), bit for bit against
oracle.field_step.

MM_WIDE_COLS=6 forces the pass on small grids (with MM_STEPS_PER_PASS=20: the auto K of a
small slab is 8). One launch runs the grid's frame at 4 columns per lane -- two row bands over
every column, the strip of the first column, the strips right of the interior -- and the
interior at 6 columns per lane on the FAST body alone, so every seam the pass adds is run
here on the value classes of tests/value_classes.py: the columns either side of the frame /
interior boundaries and of a six-column strip boundary, the rows either side of the band
boundaries and of an interior segment boundary, with non-finite seeds on each. Cells compare
as bits (signs of zeros and infinities included); the non-finite cells after s steps must be
exactly the Chebyshev ball of radius s around the seeds.

Widths: 768 (one six-column strip; the right frame strip holds the last column as a lane's
last: the EDGE body), 770 (W % 6 = 2; right frame on the GEN body, in two strips), 1000 (two
six-column strips, a right frame of 112 columns), 577 (left frame + one six-column strip + the
narrowest right frame the FAST columns allow, 25 columns). Heights: 150, 151 (odd: a bottom
band of 23 rows), 46 (two interior rows), 40 (the bands meet: no interior block). Steps: 20
(eager), then 40 (a replayed graph, both buffer parities), then 27 (a K = 20 pass, then
mm_passk_kernel's 7). The runs take no step sums: a pass with sums stays at 4 columns (its
own case below).

The interior's first row and its segment lengths are even (tests/test_plan_wide6.py), so no
interior segment starts at an odd row: the odd-start shift cannot occur in this pass, and the
MM_SEG_WAVES case checks several segments instead.
"""
import numpy as np
import pytest

import value_classes as vc
from test_gpu_parity import make_env_engine

pytestmark = pytest.mark.gpu

K = 20
PASSK, WIDE = 2, 3
O4, O6 = 216, 336
FORCE = {"MM_WIDE_COLS": 6, "MM_STEPS_PER_PASS": K}
RUNS = (20, 40, 27)
# (H, W, extra environment, (six-column strips, right strips))
CASES = [(150, 768, {}, (1, 1)), (150, 770, {}, (1, 2)), (150, 1000, {}, (2, 1)),
         (150, 577, {}, (1, 1)), (151, 768, {}, (1, 1)), (150, 768, {"MM_SEG_WAVES": 0.02}, (1, 1)),
         (46, 577, {}, (1, 1)), (40, 768, {}, (1, 1))]

_refs = {}


def reference(O, key, start, rate, steps):
    """Oracle states after 0..steps steps, computed once per key and kept read-only."""
    states = _refs.setdefault(key, [start])
    while len(states) <= steps:
        nxt = O.field_step(states[-1], rate)
        nxt.setflags(write=False)
        states.append(nxt)
    return states


def seam_positions(H, W, n6, th):
    """Non-finite seeds on the seams of the fused pass's plan."""
    top, bot = min(K + 2, H), max(min(K + 2, H), (H - K - 2) & ~1)
    rcol = O4 + n6 * O6
    mid = (top + bot) // 2 if bot > top else H // 2
    cols = [O4 - 1, O4, rcol - 1, rcol] + ([O4 + O6 - 1, O4 + O6] if n6 > 1 else [])
    pos = [(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, O4), (H // 3, W - 1)]
    pos += [(mid + (i % 3) - 1, y) for i, y in enumerate(cols)]      # the column seams
    pos += [(top - 1, O4 + 40), (top, O4 + 90), (top, 7), (top - 1, rcol + 9)]  # the top band's
    if bot < H:
        pos += [(bot - 1, O4 + 140), (bot, O4 + 190), (bot, 3), (bot - 1, W - 4)]
    if bot - top > th:  # an interior segment seam, in a six-column strip and in both frame parts
        pos += [(top + th - 1, O4 + 240), (top + th, O4 + 290), (top + th, 100), (top + th - 1, W - 9)]
    out = []
    for x, y in pos:
        if 0 <= x < H and 0 <= y < W and (x, y) not in out:
            out.append((x, y))
    return tuple(out)


def check_plan(e, H, W, tiling):
    n6, nr = tiling
    info = e.info()
    assert (info["kernel"], info["steps_per_launch"]) == (WIDE, K), info
    assert e.pass_kernel(K) == (WIDE, 6, 1 + n6 + nr)
    assert e.pass_kernel(7)[0] == PASSK
    assert [e.pass_plan(n) for n in RUNS] == [[20], [20, 20], [20, 7]]
    assert info["rows_per_wave"] % 2 == 0 and info["waves_per_pass"] % 4 == 0
    return info


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}" + ("-seg" if c[2] else ""))
def test_fused_pass_value_classes(gpu, O, monkeypatch, case):
    H, W, env, tiling = case
    for cls in vc.CLASSES:
        rate = vc.RATES[cls]
        e = make_env_engine(gpu, monkeypatch, H, W, **FORCE, **env)
        try:
            e.add_diffuse(0, rate)
            info = check_plan(e, H, W, tiling)
            th = info["rows_per_wave"]
            if env:  # several interior segments
                assert H - 2 * (K + 2) > th, info
            pos = seam_positions(H, W, tiling[0], th)
            assert len(pos) >= 14, pos
            start = vc.make(cls, H, W, positions=pos)
            start.setflags(write=False)
            e.upload(start)
            done = 0
            for n in RUNS:
                e.run(n)
                done += n
                want = reference(O, (H, W, cls, pos), start, rate, done)[done]
                got = e.download()
                vc.assert_same_bits(got, want, (case, cls, done))
                if cls == "nonfinite":
                    ball = vc.ball_mask((H, W), pos, done)
                    assert np.array_equal(~np.isfinite(got), ball), (case, done)
            assert e.info()["graph_state"] in (0, 1)
        finally:
            e.close()


def test_pass_with_sums_stays_at_four_columns(gpu, O, monkeypatch):
    """Steps whose sums are taken run the 4-column instance, the others the fused pass, in one
    engine: 20 steps without sums, 20 with a sum after the last, 20 without."""
    H, W = 150, 768
    e = make_env_engine(gpu, monkeypatch, H, W, **FORCE)
    try:
        e.add_diffuse(0, 0.1)
        start = O.fill_random(H, W)
        e.upload(start)
        for i, reduce_every in enumerate((0, 20, 0)):
            e.run(K, reduce_every)
            want = reference(O, ("sums", H, W), start, 0.1, K * (i + 1))[K * (i + 1)]
            assert np.array_equal(e.download(), want), i
        hist = e.sums_history()
        assert hist.shape == (1, 1)
        vc.assert_sum_close(hist[0, 0], reference(O, ("sums", H, W), start, 0.1, 2 * K)[2 * K])
    finally:
        e.close()


def plan_facts(e):
    info = e.info()
    keys = ("kernel", "steps_per_launch", "halo_depth", "n_passes", "rows_per_wave",
            "waves_per_pass", "seg_waves_per_cu")
    plans = {n: e.pass_plan(n) for n in (1, 7, 20, 45)}
    return ({k: info[k] for k in keys}, plans,
            {k: e.pass_kernel(k) for k in sorted({k for p in plans.values() for k in p})})


def test_reprogrammed_engine_plans_as_a_fresh_one(gpu, O, monkeypatch):
    H, W = 150, 770
    programs = [[(0, 0.1)], [(0, 0.1), (0, 0.2)], [(0, 0.25)]]  # one pass, two passes, one pass
    fresh = []
    for prog in programs:
        f = make_env_engine(gpu, monkeypatch, H, W, **FORCE)
        try:
            for a, r in prog:
                f.add_diffuse(a, r)
            fresh.append(plan_facts(f))
        finally:
            f.close()
    assert fresh[0][2][K] == fresh[2][2][K] == (WIDE, 6, 4) and fresh[1][0]["kernel"] == 0
    e = make_env_engine(gpu, monkeypatch, H, W, **FORCE)
    try:
        v = O.fill_random(H, W)
        e.upload(v)
        for prog, want in zip(programs, fresh):
            e.clear_flows()
            for a, r in prog:
                e.add_diffuse(a, r)
            assert plan_facts(e) == want, prog
            e.run(K)
            for _ in range(K):
                for _, r in prog:
                    v = O.field_step(v, r)
            assert np.array_equal(e.download(), v), prog
            assert plan_facts(e) == want, prog
    finally:
        e.close()


def test_auto_rule(gpu, monkeypatch):
    """Slabs of 2^27 cells and more take the fused pass by themselves, MM_WIDE_COLS=4 keeps
    the 4-column pass, a slab with a halo and a smaller slab keep it too."""
    with gpu.Engine(4096, 32768) as e:
        e.add_diffuse(0, 0.1)
        assert e.pass_plan(40) == [20, 20] and e.pass_kernel(K) == (WIDE, 6, 1 + 96 + 2)
    e = make_env_engine(gpu, monkeypatch, 4096, 32768, MM_WIDE_COLS=4)
    try:
        e.add_diffuse(0, 0.1)
        assert e.pass_kernel(K) == (WIDE, 4, 152)
    finally:
        e.close()
    with gpu.Engine(32768, 32768, 0, 4096, rank=0, nranks=8, halo_mode=gpu.MM_HALO_HOST) as e:
        e.add_diffuse(0, 0.1)
        assert e.pass_kernel(K) == (WIDE, 4, 152)
    e = make_env_engine(gpu, monkeypatch, 150, 768, MM_STEPS_PER_PASS=K)
    try:
        e.add_diffuse(0, 0.1)
        assert e.pass_kernel(K) == (WIDE, 4, 4)
    finally:
        e.close()
