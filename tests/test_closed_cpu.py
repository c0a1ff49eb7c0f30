"""Closed rate-field diffusion (MM_FLOW_DIFFUSE_CLOSED) without a GPU: the numpy model of its
contract (tests/closed_model.py) against the oracle, the properties the contract promises
(an embedded rectangle is a grid of its own, conservation over the open cells, walls keep
their bits), the planner on programs that hold a closed diffusion
(tests/plan_closed_cli.cpp against mpi-model_amd/csrc/mm_plan.cpp, built with plain g++ the
way tests/test_plan.py builds its program), and the constant in header and binding."""
import math
import os
import re

import numpy as np
import pytest

import closed_model as cm
from plan_build import REPO, SANITIZE, build, run
from value_classes import assert_same_bits

HEADER = os.path.join(REPO, "include", "mpimodel.h")
SHAPES = [(1, 1), (1, 9), (2, 2), (3, 3), (13, 6), (27, 257), (130, 97)]
# the embedded rectangles: (rows, columns) at (row, column) of 27 x 257 -- a corner of the
# grid, across the strip seam 127 / 128 from the block seam 7 / 8 on, inside the last strip.
# Every block at every offset, but 9 x 11 at column 250, which does not fit 257 columns.
BLOCKS = [(b, o) for b in ((9, 11), (1, 5), (2, 2)) for o in ((0, 0), (8, 120), (3, 250))
          if o[1] + b[1] <= 257]


def geo_counts(O, H, W):
    return np.array([[O.neighbor_count(H, W, x, y) for y in range(W)] for x in range(H)])


def oracle_step(O, v, f):
    """or_field_step_general with outf = f * v (0 by select for the cell without neighbours,
    as tests/test_gpu_ratefield.py feeds it)."""
    return O.field_step_general(v, np.where(geo_counts(O, *v.shape) > 0, f * v, 0.0))


def values(H, W, seed=0):
    return np.random.default_rng(seed + 1000003 * H + W).uniform(0.5, 2.0, (H, W))


@pytest.mark.parametrize("H,W", SHAPES)
def test_all_open_is_the_field_step(O, H, W):
    """f != 0 everywhere: bit for bit or_field_step_general with outf = f * v."""
    v = values(H, W)
    f = cm.rates(np.ones((H, W), dtype=bool))
    assert (f != 0).all() and (f < 0).any()
    w = v.copy()
    for step in range(5):
        v = cm.closed_step(v, f)
        w = oracle_step(O, w, f)
        assert_same_bits(v, w, f"{H}x{W} step {step + 1}")


@pytest.mark.parametrize("block,off", BLOCKS)
def test_embedded_rectangle_is_a_grid_of_its_own(O, block, off):
    """A p x q block of non-zero rates in a zero field evolves like the stand-alone p x q grid:
    the geometric 3 / 5 / 8 counts of that grid are the block's open counts, and the zero
    shares of walls and of cells outside a grid are both +0 by select."""
    H, W = 27, 257
    (p, q), (x0, y0) = block, off
    assert x0 + p <= H and y0 + q <= W
    fb = cm.rates(np.ones((p, q), dtype=bool), seed=1)
    f = np.zeros((H, W))
    f[x0:x0 + p, y0:y0 + q] = fb
    cnt = cm.open_counts(f)[x0:x0 + p, y0:y0 + q]
    assert np.array_equal(cnt, geo_counts(O, p, q))
    v = values(H, W, seed=2)
    v0 = v.copy()
    w = v[x0:x0 + p, y0:y0 + q].copy()
    outside = np.ones((H, W), dtype=bool)
    outside[x0:x0 + p, y0:y0 + q] = False
    for step in range(6):
        v = cm.closed_step(v, f)
        w = oracle_step(O, w, fb)
        assert_same_bits(v[x0:x0 + p, y0:y0 + q], w, f"block {p}x{q} at {off}, step {step + 1}")
        assert_same_bits(v[outside], v0[outside], "walls")


@pytest.mark.parametrize("H,W", [(27, 257), (130, 97)])
def test_conserves_over_the_open_cells(H, W):
    mask = cm.domain("random", H, W)
    assert 0.6 < mask.mean() < 0.8
    f = cm.rates(mask, negative=False)
    v = values(H, W, seed=3)
    s0 = math.fsum(v[mask])
    for step in range(20):
        v = cm.closed_step(v, f)
        s, scale = math.fsum(v[mask]), math.fsum(np.abs(v[mask]))
        assert abs(s - s0) <= 1e-12 * scale, (step, s, s0)


@pytest.mark.parametrize("kind", ["random", "checker", "disc", "seams", "one"])
def test_walls_keep_their_bits(kind):
    """Walls holding NaN, +-inf and -0 keep exactly those bits (a NaN its payload too) and
    change no other cell: the open cells evolve as they do beside walls of 1.0."""
    H, W = 27, 257
    mask = cm.domain(kind, H, W)
    f = cm.rates(mask)
    v = values(H, W, seed=4)
    plain = v.copy()
    weird = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0])
    walls = np.argwhere(~mask)
    for i, (x, y) in enumerate(walls):
        v[x, y] = weird[i % len(weird)]
    payload = np.array([0x7FF8000000BEEF01], dtype=np.uint64).view(np.float64)[0]
    if len(walls):
        v[tuple(walls[0])] = payload
    v0 = v.copy()
    for step in range(4):
        v = cm.closed_step(v, f)
        plain = cm.closed_step(plain, f)
        assert np.array_equal(v[~mask].view(np.uint64), v0[~mask].view(np.uint64))
        assert np.isfinite(v[mask]).all()
        assert_same_bits(v[mask], plain[mask], f"{kind} step {step + 1}")


def test_lone_cell_stays_put():
    f = np.zeros((5, 7))
    f[2, 3] = 0.25
    v = values(5, 7)
    assert cm.open_counts(f)[2, 3] == 0
    assert_same_bits(cm.closed_steps(v, f, 3), v)


def test_zero_of_either_sign_is_a_wall():
    f = np.full((4, 4), 0.1)
    f[1, 1], f[2, 2] = 0.0, -0.0
    assert not cm.open_cells(f)[1, 1] and not cm.open_cells(f)[2, 2]
    assert cm.open_cells(f).sum() == 14


# ---- the planner -------------------------------------------------------------
def build_and_run(exe, *flags):
    out = run(build(exe, "plan_closed_cli.cpp", *flags))
    assert out.strip() == "ok", out[-3000:]


def test_planner_keeps_closed_programs_at_one_step(tmp_path):
    """One step per pass, field_k == 0, halo depth 1 under MM_FIELD_STEPS=4, MM_FIELD_HALO=4
    and slabs of 2^22 cells and more; every other program plans as the commit before did."""
    build_and_run(str(tmp_path / "plan_closed_cli"))


def test_planner_under_sanitizers(tmp_path):
    build_and_run(str(tmp_path / "plan_closed_cli_san"), *SANITIZE)


# ---- header and binding ---------------------------------------------------------
def test_header_and_binding_agree(mm):
    text = open(HEADER).read()
    enums = dict(re.findall(r"\b(MM_FLOW_[A-Z_]+)\s*=\s*(-?\d+)", text))
    assert enums == {"MM_FLOW_DIFFUSE": "1", "MM_FLOW_TRANSFER": "2", "MM_FLOW_DIFFUSE_FIELD": "3",
                     "MM_FLOW_DIFFUSE_CLOSED": "4"}
    assert mm.MM_FLOW_DIFFUSE_CLOSED == 4
    assert "#define MM_ABI_VERSION 3" in text
    assert mm.lib().mm_abi_version() == 3
    assert callable(mm.Engine.add_diffuse_closed)
    # the field kind no longer claims to be a mask, and points to the closed kind
    field = text[text.index("MM_FLOW_TRANSFER = 2"):text.index("MM_FLOW_DIFFUSE_FIELD = 3")]
    assert "a 0/1-scaled field a mask" not in field and "MM_FLOW_DIFFUSE_CLOSED" in field
    api = open(os.path.join(REPO, "mpi-model_amd", "api", "mm_engine.hpp")).read()
    assert "add_diffuse_closed(int attr)" in api and "MM_FLOW_DIFFUSE_CLOSED" in api
