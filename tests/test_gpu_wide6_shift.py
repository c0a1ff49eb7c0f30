"""GPU: the halo lanes of the six-column interior strips (mm_wide6_kernel's fast_segment), bit
for bit against oracle.field_step.

A six-column strip loads 384 columns and stores the middle 336: lanes 0..3 (strip columns
0..23) and 60..63 (360..383) are halo. The +-1 column neighbours of a lane's edge columns come
from the lanes beside it, and at the wave's two ends from nowhere: whatever arrives there
enters strip column 0 / 383 at level 1 and moves one column inward per level, 20 columns in a
K = 20 pass -- it must stay inside the halo. Wave p of the workgroup (levels 5 p + 1 .. 5 p +
5) also runs with its outermost p lanes a side out of EXEC (fast_segment, MM_WIDE6_MASK): what
those lanes hold, and what their neighbours read from them, must not reach a stored column
either. tests/test_gpu_wide6.py puts non-finite seeds on the
pass's seams; here they sit in the halo lanes themselves, one in every halo lane of both
strips of a 150 x 1000 grid (loaded origins 192 and 528: grid columns 192..215 and 552..575,
528..551 and 888..911), on interior rows, in the lanes' first and last columns among others
(strip columns 0, 23, 360 and 383). A non-finite value that crossed the wave's end, or came
out of the halo a column too early, would show as a non-finite cell outside the Chebyshev
ball of the seeds or as a wrong bit inside it.

Cases: one interior segment, and MM_SEG_WAVES=0.02 (several) with the seeds on the two rows
either side of an interior segment seam. Classes: nonfinite, and signed as the finite one.
Runs: 20 steps, then 40 more (a replayed graph, both buffer parities).
"""
import numpy as np
import pytest

import test_gpu_wide6 as w6
import value_classes as vc
from test_gpu_parity import make_env_engine

H, W = 150, 1000
TILING = (2, 1)          # six-column strips, right frame strips
HALO = 4                 # halo lanes a side: ceil(20 / 6)
LANES = (0, 1, 2, 3, 60, 61, 62, 63)
OFFS = (0, 3, 2, 5)      # the seed's column inside its lane, by lane & 3: strip columns 0, 9,
                         # 14, 23 and 360, 369, 374, 383
RUNS = (20, 40)
TOP, BOT = w6.K + 2, (H - w6.K - 2) & ~1  # the interior's rows (test_gpu_wide6.seam_positions)


def halo_positions(rows):
    """One seed in every halo lane of both six-column strips, on `rows` in turn."""
    pos = []
    for s in range(TILING[0]):
        origin = w6.O4 + s * w6.O6 - 6 * HALO
        for lane in LANES:
            pos.append((rows[len(pos) % len(rows)], origin + 6 * lane + OFFS[lane & 3]))
    return tuple(pos)


def test_seed_columns():
    """(No GPU.) The seeds lie where the module says."""
    pos = halo_positions((TOP,))
    cols = sorted(y for _, y in pos)
    assert len(pos) == 16 and len(set(cols)) == 16
    spans = ((192, 215), (552, 575), (528, 551), (888, 911))
    assert all(sum(a <= y <= b for y in cols) == 4 for a, b in spans)
    assert {192, 215, 552, 575, 528, 551, 888, 911} <= set(cols)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"MM_SEG_WAVES": 0.02}], ids=["one-seg", "seam"])
@pytest.mark.parametrize("cls", ["nonfinite", "signed"])
def test_halo_lane_seeds(gpu, O, monkeypatch, cls, env):
    rate = vc.RATES[cls]
    e = make_env_engine(gpu, monkeypatch, H, W, **w6.FORCE, **env)
    try:
        e.add_diffuse(0, rate)
        info = w6.check_plan(e, H, W, TILING)
        th = info["rows_per_wave"]
        if env:  # the two rows either side of the first interior segment seam
            assert BOT - TOP > th, info
            rows = (TOP + th - 1, TOP + th)
        else:
            rows = tuple(range(TOP, BOT, 13))
        assert all(TOP <= x < BOT for x in rows)
        pos = halo_positions(rows)
        start = vc.make(cls, H, W, positions=pos)
        start.setflags(write=False)
        e.upload(start)
        done = 0
        for n in RUNS:
            e.run(n)
            done += n
            want = w6.reference(O, ("halo", cls, pos), start, rate, done)[done]
            got = e.download()
            vc.assert_same_bits(got, want, (cls, env, done))
            if cls == "nonfinite":
                ball = vc.ball_mask((H, W), pos, done)
                assert np.array_equal(~np.isfinite(got), ball), (env, done)
    finally:
        e.close()
