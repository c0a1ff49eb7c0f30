"""K fused steps of the closed rate-field diffusion (MM_CLOSED_STEPS, mm_closedk_kernel) without
a GPU: the dependency cone the kernel's halo and its segments' input rows are sized by, in
numpy with tests/closed_model.py; the geometry of mm_geom.hpp against that cone; the planner
(tests/plan_closedk_cli.cpp against mpi-model_amd/csrc/mm_plan.cpp, built with plain g++ and
once more as a stand-alone program under the sanitizers); the constant in header and binding."""
import os
import re

import numpy as np
import pytest

import closed_model as cm
from closedk_geom import geom
from plan_build import REPO, SANITIZE, build, run

HEADER = os.path.join(REPO, "include", "mpimodel.h")
N, C = 41, 20  # the cone's grid and its centre


def shipped_ks():
    return range(2, geom()["kClosedMaxSteps"] + 1)


def ring(d):
    """The cells at Chebyshev distance exactly d from the centre."""
    x, y = np.mgrid[0:N, 0:N]
    return np.argwhere(np.maximum(abs(x - C), abs(y - C)) == d)


def centre_after(v, f, K):
    return cm.closed_steps(v, f, K)[C, C].tobytes()


def test_every_k_of_the_cone_is_shipped_and_fits_the_grid():
    ks = list(shipped_ks())
    assert ks and ks[0] == 2 and C - (ks[-1] + 2) >= 1 and C + ks[-1] + 2 <= N - 2


@pytest.mark.parametrize("K", list(shipped_ks()))
def test_cone_of_the_rates(K):
    """A wall at distance K + 1 changes the cell after K steps (through the count of a cell at
    distance K, whose share of step 1 arrives at step K); at K + 2 it does not."""
    rng = np.random.default_rng(K)
    v, f = rng.uniform(0.5, 2.0, (N, N)), rng.uniform(0.05, 0.3, (N, N))
    base = centre_after(v, f, K)
    for x, y in ring(K + 1):
        g = f.copy()
        g[x, y] = 0.0
        assert centre_after(v, g, K) != base, (K, x, y)
    for x, y in ring(K + 2):
        g = f.copy()
        g[x, y] = 0.0
        assert centre_after(v, g, K) == base, (K, x, y)
    # everything from distance K + 2 on at once, values included
    far = np.maximum(*np.abs(np.mgrid[0:N, 0:N] - C)) >= K + 2
    g, w = np.where(far, 0.0, f), np.where(far, np.nan, v)
    assert centre_after(w, g, K) == base
    # a band of rows widened by K + 1 rows a side is enough for the band
    lo, hi = C - 2, C + 3
    band = cm.closed_steps(v[lo - K - 1:hi + K + 1], f[lo - K - 1:hi + K + 1], K)[K + 1:-(K + 1)]
    assert band.tobytes() == cm.closed_steps(v, f, K)[lo:hi].tobytes()


@pytest.mark.parametrize("K", list(shipped_ks()))
def test_cone_of_the_values(K):
    """A value at distance K changes the cell after K steps; at K + 1 it does not."""
    rng = np.random.default_rng(10 + K)
    v, f = rng.uniform(0.5, 2.0, (N, N)), rng.uniform(0.05, 0.3, (N, N))
    base = centre_after(v, f, K)
    for x, y in ring(K):
        w = v.copy()
        w[x, y] += 1.0
        assert centre_after(w, f, K) != base, (K, x, y)
    for x, y in ring(K + 1):
        w = v.copy()
        w[x, y] = np.nan
        assert centre_after(w, f, K) == base, (K, x, y)


def test_strip_halo_covers_the_cone():
    """A strip that loads 128 columns knows the count of all but its first and last column: its
    level-K values are valid K + 1 columns in from either end (the cone of the rates), so the
    discarded halo is at least that, a whole number of two-column lanes."""
    g = geom()
    assert g["kStripCols"] == 128
    for K in shipped_ks():
        halo = g["closedk_halo_cols"](K)
        assert halo >= K + 1 and halo % 2 == 0 and halo - 2 < K + 1, (K, halo)
        assert g["closedk_out_cols"](K) == 128 - 2 * halo
        # the ring: the prefetch depth ahead of level 1, the 2(K-1) rows behind it and the row
        # that runs ahead for the count
        assert g["closed_ring"](K) >= g["kFieldPrefetch"] + 2 * (K - 1) + 1
        assert g["closed_ring"](K) % g["kFieldPrefetch"] == 0
        for pitch in (128, 32768):
            assert g["closedk_max_rows"](K, pitch) < g["fieldk_max_rows"](K, pitch)


# ---- the planner -------------------------------------------------------------
def build_and_run(exe, *flags):
    out = run(build(exe, "plan_closedk_cli.cpp", *flags))
    assert out.strip() == "ok", out[-3000:]
    return int(run(exe, "max"))


def test_planner(tmp_path, mm):
    assert build_and_run(str(tmp_path / "plan_closedk_cli")) == mm.CLOSED_MAX_STEPS


def test_planner_under_sanitizers(tmp_path):
    build_and_run(str(tmp_path / "plan_closedk_cli_san"), *SANITIZE)


# ---- header and binding ---------------------------------------------------------
def test_header_and_binding_agree(mm):
    text = open(HEADER).read()
    m = re.search(r"^#define\s+MM_CLOSED_MAX_STEPS\s+(\d+)", text, re.M)
    assert m, "include/mpimodel.h has no MM_CLOSED_MAX_STEPS"
    assert int(m.group(1)) == mm.CLOSED_MAX_STEPS == geom()["kClosedMaxSteps"] >= 2
    assert "MM_CLOSED_STEPS" in text.replace("MM_CLOSED_MAX_STEPS", "")
    assert "5 mm_closedk_kernel" in text
    assert "a program that\n     * holds one runs one step per pass" not in text
    assert "#define MM_ABI_VERSION 3" in text and mm.lib().mm_abi_version() == 3
