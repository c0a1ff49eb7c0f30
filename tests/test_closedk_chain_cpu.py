"""K-step closed rate-field passes on slabs with a halo (MM_CLOSED_HALO) without a GPU: the
cone of a slab in numpy with tests/closed_model.py -- K ghost rows of the state and K + 1 of
the rate field are enough for the slab's K steps, and K of the field are not -- and the planner
(tests/plan_closedk_chain_cli.cpp against mpi-model_amd/csrc/mm_plan.cpp: the knob's parsing,
mm::closed_k_for, the split plan of mm_closedk_kernel, rank-invariance, the recorded table;
built with plain g++ and once more as a stand-alone program under ASan + UBSan)."""
import os

import numpy as np
import pytest

import closed_model as cm
from closedk_geom import geom
from plan_build import REPO, SANITIZE, build, run

HEADER = os.path.join(REPO, "include", "mpimodel.h")
N, W = 41, 23  # the cone's grid
SLABS = [(0, 9), (9, 20), (16, 25), (30, 41), (20, 22)]  # [x0, x1): edge slabs, inner ones, a thin one


def shipped_ks():
    return range(2, geom()["kClosedMaxSteps"] + 1)


def slab_after(v, f, x0, x1, K, f_rows):
    """Rows [x0, x1) after K steps of a slab that knows v of rows x0-K .. x1+K-1 and f of rows
    x0-f_rows .. x1+f_rows-1: everything further is garbage (state) and walls (rates)."""
    rng = np.random.default_rng(99)
    w = np.where(rng.random(v.shape) < 0.5, np.nan, -7.0)
    g = np.zeros_like(f)
    lo, hi = max(x0 - K, 0), min(x1 + K, N)
    w[lo:hi] = v[lo:hi]
    lo, hi = max(x0 - f_rows, 0), min(x1 + f_rows, N)
    g[lo:hi] = f[lo:hi]
    return cm.closed_steps(w, g, K)[x0:x1]


@pytest.mark.parametrize("K", list(shipped_ks()))
def test_slab_cone(K):
    rng = np.random.default_rng(40 + K)
    mask = rng.random((N, W)) < 0.8
    v = rng.uniform(0.5, 2.0, (N, W))
    f = np.where(mask, rng.uniform(0.05, 0.3, (N, W)), 0.0)
    whole = cm.closed_steps(v, f, K)
    for x0, x1 in SLABS:
        got = slab_after(v, f, x0, x1, K, K + 1)
        assert got.tobytes() == whole[x0:x1].tobytes(), (K, x0, x1)
        # K ghost rows of the field are one too few wherever the slab has a neighbour: row
        # x0 - K - 1 (x1 + K) closed changes the count of row x0 - K, whose share arrives at step K
        if x0 - K - 1 >= 0 or x1 + K < N:
            short = slab_after(v, f, x0, x1, K, K)
            assert short.tobytes() != whole[x0:x1].tobytes(), (K, x0, x1)


def test_every_slab_of_the_cone_fits_the_grid():
    K = max(shipped_ks())
    assert any(x0 - K - 1 >= 0 and x1 + K < N for x0, x1 in SLABS)
    assert any(x1 - x0 < K for x0, x1 in SLABS)  # thinner than the deepest pass


# ---- the planner -------------------------------------------------------------
def build_and_run(exe, *flags):
    out = run(build(exe, "plan_closedk_chain_cli.cpp", *flags), HEADER)
    assert out.startswith("ok "), out[-3000:]
    return int(out.split()[1])  # the planner's kClosedMaxSteps


def test_planner_splits_closed_passes(tmp_path, mm):
    assert build_and_run(str(tmp_path / "plan_closedk_chain_cli")) == mm.CLOSED_MAX_STEPS


def test_planner_under_sanitizers(tmp_path, mm):
    assert build_and_run(str(tmp_path / "plan_closedk_chain_cli_san"), *SANITIZE) == mm.CLOSED_MAX_STEPS


def test_header_and_binding_name_the_knob(mm):
    text = open(HEADER).read()
    env = text[text.index("Environment:"):text.index("int mm_engine_create(")]
    assert "MM_CLOSED_HALO" in env and "lockstep" in env[env.index("MM_CLOSED_HALO"):]
    kind = text[text.index("MM_CLOSED_STEPS=K"):text.index("MM_FLOW_DIFFUSE_CLOSED = 4")]
    assert "MM_CLOSED_HALO" in kind and "-(K+1)..h+K" in kind and "MM_ERR_STATE" in kind
    assert "#define MM_ABI_VERSION 3" in text
    assert "MM_CLOSED_HALO" in open(mm.__file__).read()
