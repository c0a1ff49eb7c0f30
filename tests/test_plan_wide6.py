"""The plan of the fused six-column K = 20 pass (mm_plan.cpp wide6_on / wide6_launch,
mm_geom.hpp wide6_cols) on the CPU, through tests/plan6_cli.cpp: the column tiling covers
every column once and leaves the grid's last column to the frame whatever W % 6 is, every
interior segment reads interior rows and columns only (the FAST body's condition), segment
lengths are even, the blocks add up, and every shape the rule leaves out plans exactly as
without the fused instance."""
import pytest

import plan_build

K = 20
O4, O6, HALO6 = 216, 336, 24  # output columns of a 4- / 6-column strip, a 6-column strip's halo
FIELDS = ("lo hi lo2 hi2 seg th th_edge xcd nstrips waves_a waves_total partial_base "
          "top bot col rcol strips rstrips th6 band0 band1 frame").split()
FORCE = {"MM_WIDE_COLS": 6, "MM_STEPS_PER_PASS": K}
WIDTHS = (32768, 16384, 770, 768, 1000)


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return plan_build.build(str(tmp_path_factory.mktemp("plan6") / "plan6_cli"), "plan6_cli.cpp")


def run(exe, lines):
    return plan_build.run(exe, input="\n".join(lines) + "\n")


def slab(H, W, env=None, s6=2, G=1, g=0, split=0, n_attr=1, ncu=256):
    x0, h = g * H // G, (g + 1) * H // G - g * H // G
    mask, chains = (15, 1) if n_attr > 1 else (1, 0)
    return (["envclear"] + [f"env {k} {v}" for k, v in (env or {}).items()] +
            [f"in {H} {W} {x0} {h} {G} {n_attr} {split} 1 {mask} {chains} {chains} {ncu} 8 {s6}"])


def launch(exe, H, W, env=None, k=K, red=0, **kw):
    """(kernel, cols, strips, total, interior launch as a dict) of one pass."""
    v = [int(x) for x in run(exe, slab(H, W, env, **kw) + [f"launch {k} {red}"]).split()]
    return v[0], v[1], v[2], v[5], dict(zip(FIELDS, v[6:6 + len(FIELDS)]))


def shapes():
    big = [(32768, W) for W in (32768, 16384)] + [(16384, 16384), (4096, 32768)]
    small = [(H, W) for H in (150, 151, 64, 30) for W in WIDTHS[2:] + (577, 578, 912, 913)]
    return [(s, {}) for s in big] + [(s, FORCE) for s in small]


def test_columns_are_covered_once_and_the_frame_takes_the_last(cli):
    for W in WIDTHS + tuple(range(577, 577 + 2 * O6 + 12)):
        kernel, cols, strips, _, l = launch(cli, 150, W, FORCE)
        assert (kernel, cols) == (3, 6), W
        n, nr = l["strips"], l["rstrips"]
        assert n >= 1 and nr >= 1 and strips == 1 + n + nr, W
        # [0, col) the first strip, n strips of 336 from col, nr strips of 216 from rcol to W
        assert l["col"] == O4 and l["rcol"] == O4 + n * O6, W
        spans = [(0, O4)] + [(O4 + i * O6, O4 + (i + 1) * O6) for i in range(n)]
        spans += [(l["rcol"] + i * O4, min(W, l["rcol"] + (i + 1) * O4)) for i in range(nr)]
        assert all(a < b for a, b in spans), W
        assert spans[0][0] == 0 and spans[-1][1] == W, W
        assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1)), W
        # each six-column strip's output origin is even; the columns it loads are interior
        # columns of the grid (the FAST body): the last column is a frame strip's
        assert all(a % 2 == 0 for a, _ in spans[1:1 + n]), W
        assert spans[1][0] - HALO6 >= 1 and spans[n][1] + HALO6 - 1 <= W - 2, W
        # no narrower right part would do with one more strip
        assert W - l["rcol"] - O6 < HALO6 + 1, W
        # the band rows: 4-column strips of the whole width
        assert l["nstrips"] == -(-W // O4), W
    assert {W % 6 for W in range(577, 577 + 2 * O6 + 12)} == set(range(6))


def test_recorded_tilings(cli):
    want = {32768: (96, 2), 16384: (48, 1), 770: (1, 2), 768: (1, 1), 1000: (2, 1), 577: (1, 1)}
    for W, (n, nr) in want.items():
        l = launch(cli, 150, W, FORCE)[4]
        assert (l["strips"], l["rstrips"]) == (n, nr), W


def test_interior_segments_read_interior_rows_and_are_even(cli):
    for (H, W), env in shapes() + [((150, 768), {**FORCE, "MM_SEG_WAVES": 0.02}),
                                   ((4000, 768), {**FORCE, "MM_SEG_WAVES": 0.05})]:
        kernel, cols, _, total, l = launch(cli, H, W, env)
        assert (kernel, cols) == (3, 6), (H, W)
        top, bot, th = l["top"], l["bot"], l["th6"]
        assert (l["lo"], l["hi"], l["seg"]) == (0, H, 1)
        assert 0 < top <= bot <= H
        nb = l["nstrips"]
        assert l["band0"] == nb and l["band1"] == nb + (nb if bot < H else 0)
        if bot == top:  # the bands meet: no block between them
            assert l["frame"] == l["band1"] == l["waves_total"] == total
            assert H < 2 * (K + 2) + 2
            continue
        # rows any level of an interior segment reads: [top - K, bot + K - 1], inside [2, H - 3];
        # and no shorter band would do (even rows)
        assert top - K >= 2 and bot + K - 1 <= H - 3, (H, W)
        assert top % 2 == 0 and bot % 2 == 0 and top - 2 - K < 2 and bot + 2 + K - 1 > H - 3
        assert th % 2 == 0 and th == l["th"] and th >= 2
        per = -(-(bot - top) // th)
        starts = [top + i * th for i in range(per)]
        assert all(s % 2 == 0 for s in starts)  # no segment pays the odd-start shift
        assert l["frame"] == l["band1"] + (1 + l["rstrips"]) * per
        assert l["waves_total"] == l["frame"] + l["strips"] * per == l["waves_a"] == total
        if "MM_SEG_WAVES" in env:
            assert per > 1
    # the flagship slab: the resident slots (256 CUs x 2) are filled about four times over
    total = launch(cli, 32768, 32768)[3]
    assert 1500 < total <= 4 * 512 + 2 * 152 + 8


def test_info_reports_the_fused_plan(cli):
    out = run(cli, slab(32768, 32768) + ["info", f"kern {K} 0", f"kern {K} 1", "kern 16 0"])
    info, k0, k1, k16 = [[int(x) for x in ln.split()] for ln in out.splitlines()]
    l = launch(cli, 32768, 32768)[4]
    assert info == [3, K, l["th6"], 4 * l["waves_total"], 8]
    assert k0 == [3, 6, 1 + 96 + 2] and k1 == [3, 4, 152] and k16[:2] == [3, 4]


def other_shapes():
    big = {}
    yield "halo", slab(32768, 32768, big, G=8, g=3, split=1), [(K, 0)]
    yield "self-halo", slab(32768, 32768, big, split=1), [(K, 0)]
    yield "sums", slab(32768, 32768, big), [(K, 1)]
    yield "k16", slab(32768, 32768, big), [(16, 0), (10, 0), (8, 1)]
    yield "small", slab(4096, 4096, big), [(K, 0), (8, 0)]
    yield "small-k20", slab(150, 768, {"MM_STEPS_PER_PASS": K}), [(K, 0)]
    yield "cols4", slab(32768, 32768, {"MM_WIDE_COLS": 4}), [(K, 0)]
    yield "cols5", slab(150, 768, {"MM_WIDE_COLS": 5, "MM_STEPS_PER_PASS": K}), [(K, 0)]
    yield "narrow", slab(150, 576, FORCE), [(K, 0)]
    yield "no-wide", slab(32768, 32768, {"MM_WIDE": 0, "MM_WIDE_COLS": 6}), [(K, 0), (8, 0)]
    yield "c5", slab(8192, 8192, {"MM_WIDE_COLS": 6}, n_attr=4), [(8, 0), (8, 1)]
    yield "forced-halo", slab(300, 768, FORCE, G=2, g=1, split=1), [(K, 0)]
    yield "forced-sums", slab(150, 768, FORCE), [(K, 1)]


def test_other_shapes_plan_as_before(cli):
    """Halo, sums, K != 20, a small slab without the variable, MM_WIDE_COLS=4: the planner's
    every answer with the fused instance on offer equals, byte for byte, its answer without
    one (s6 = 0: nothing of the fused plan can apply)."""
    for name, lines, passes in other_shapes():
        # (a pass with sums, or of K != 20, on a slab whose other passes qualify: that pass's
        # answers; elsewhere also the slab's info and pass plans)
        asks = [] if name in ("sums", "k16", "forced-sums") else ["info"]
        asks += ["plan 20", "plan 27", "plan 1000"]
        asks += [f"kern {k} {r}" for k, r in passes] + [f"launch {k} {r}" for k, r in passes]
        assert lines[-1].endswith(" 2")
        with_inst = run(cli, lines + asks)
        without = run(cli, lines[:-1] + [lines[-1][:-2] + " 0"] + asks)
        assert with_inst == without and with_inst.count("\n") == len(asks), name
        assert all(ln.split()[1] != "6" for ln in with_inst.splitlines()[-2 * len(passes):]), name
    # and the qualifying slab does differ
    q = slab(32768, 32768)
    assert run(cli, q + [f"launch {K} 0"]) != run(cli, q[:-1] + [q[-1][:-2] + " 0", f"launch {K} 0"])
