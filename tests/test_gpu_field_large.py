"""The rate-field kernels as they ship, and every K-step kernel's segments at the 2^31 cap.

1. The default. No MM_FIELD_STEPS, MM_SEG_WAVES or MM_KERNEL_VARIANT: at 2048 x 2048, the
   smallest grid on which the auto rule (mm_plan.cpp field_steps_for) takes K = 4, and at
   4104 x 4096, the smallest convenient one whose two buffers pass 256 MiB (kernel_variant:
   the non-temporal-store instances), under the occupancy-sized segment plan; 2047 x 2048
   stays on one step per pass. Seven steps (passes of 4 + 3), the WHOLE grid bit for bit
   against or_field_step_general (oracle/mm_oracle.c) with outf = f * v iterated, the seven
   step sums to 1e-12 relative against math.fsum of the reference states. At 4104 x 4096
   once more with MM_FIELD_STEPS=1: mm_field_kernel's non-temporal instance under the size
   rule. tests/test_fieldk_cpu.py pins the two rules at these shapes without a GPU.

2. Segments at the offset cap. fieldk_max_rows / passk_max_rows (mm_geom.hpp) cut a segment
   so that every 32-bit buffer offset of a wave stays below 2^31; the margin is a count of
   how far each kernel's prefetch and ring run ahead of the rows it emits. On 8200 x 32768
   (pitch 32768: the cap is about 2^28 cells at any pitch, so no smaller grid reaches it)
   with MM_SEG_WAVES=0.001 every interior strip is one segment of exactly the cap and a rest
   that ends at the grid's last row. One pass of K of mm_fieldk_kernel (K = 2 and the
   largest), mm_passk_kernel K = 10 and mm_wide_kernel K = 20, sums off and on: three bands
   of rows, every column, bit for bit against the oracle on the band widened by its
   dependency cone -- the top rows, the rows where the byte offset crosses 2^30, and from 64
   rows before the seam to the last row (the deepest offsets of the first segment, the seam,
   the grid's edge). A margin one row short would not fault: a row would read as zeros or a
   store be dropped a few rows before the seam, which is what the third band would show.
"""
import math
import os
import re

import numpy as np
import pytest

import test_gpu_large as large
from test_gpu_ratefield import neighbour_counts, oracle_step

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDK, PASSK, WIDE = 4, 2, 3  # mm_info.kernel
KNOBS = ("MM_FIELD_STEPS", "MM_SEG_WAVES", "MM_KERNEL_VARIANT", "MM_WIDE", "MM_STEPS_PER_PASS",
         "MM_SEG_EDGE", "MM_PASSK", "MM_GRAPH")
STEPS = 7


def engine(gpu, monkeypatch, H, W, **env):
    """An engine created with exactly `env` of the planner's knobs set."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, str(v))
    try:
        return gpu.Engine(H, W)
    finally:
        for name in env:
            monkeypatch.delenv(name)


# ---- 1. the shipped default ----------------------------------------------------------------
def hash_field(H, W):
    """An integer hash of (row, column): a quarter of the cells exactly 0.0, 3 % exactly 1.0,
    the others uniform in [0, 0.5) -- the classes of test_gpu_ratefield.random_field."""
    x = (np.arange(H, dtype=np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15) +
         np.arange(W, dtype=np.uint64)[None, :] * np.uint64(0xC2B2AE3D27D4EB4F))
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    pick = x >> np.uint64(56)  # 0..255
    f = ((x >> np.uint64(3)) & np.uint64((1 << 52) - 1)).astype(np.float64) * 2.0 ** -53
    f[pick < 64] = 0.0
    f[pick >= 248] = 1.0
    return f


_DEFAULT = {}


def default_case(O, H, W):
    """(field, state after STEPS steps, math.fsum of the state after each step): once per
    shape, never modified."""
    if (H, W) not in _DEFAULT:
        f, cnt = hash_field(H, W), neighbour_counts(H, W)
        zero, one = np.count_nonzero(f == 0.0) / f.size, np.count_nonzero(f == 1.0) / f.size
        assert 0.24 < zero < 0.26 and 0.025 < one < 0.04 and f.max() == 1.0 and f.min() == 0.0
        v, sums = O.fill_random(H, W), []
        for _ in range(STEPS):
            v = oracle_step(O, v, f, cnt)
            sums.append(math.fsum(memoryview(v.ravel())))  # (the buffer: 4 x faster than the array)
        for a in (f, v):
            a.setflags(write=False)
        _DEFAULT[H, W] = (f, v, sums)
    return _DEFAULT[H, W]


def run_default(O, e, H, W):
    f, want, sums = default_case(O, H, W)
    e.fill_random(0)
    e.rate_field_upload(f)
    e.run(STEPS, reduce_every=1)
    got = e.download()
    hist = e.sums_history()
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), bad[-1].tolist())
    assert hist.shape == (STEPS, 1)
    for s in range(STEPS):
        assert abs(hist[s, 0] - sums[s]) <= 1e-12 * abs(sums[s]), (s, hist[s, 0], sums[s])


@pytest.mark.parametrize("H,W", [(2048, 2048), (4104, 4096)])
def test_default_fuses_four_steps(gpu, O, monkeypatch, H, W):
    with engine(gpu, monkeypatch, H, W) as e:
        e.add_diffuse_field(0)
        info = e.info()
        assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (FIELDK, 4, 4), info
        assert e.pass_plan(STEPS) == [4, 3]
        assert e.pass_kernel(4)[0] == FIELDK and e.pass_kernel(3)[0] == FIELDK
        assert e.pass_kernel(4)[2] == -(-W // 120) >= 3  # strips of 120 output columns
        assert 16 <= info["rows_per_wave"] < H, info  # several segments per strip
        run_default(O, e, H, W)


def test_one_step_kernel_above_the_store_rule(gpu, O, monkeypatch):
    H, W = 4104, 4096
    with engine(gpu, monkeypatch, H, W, MM_FIELD_STEPS=1) as e:
        e.add_diffuse_field(0)
        info = e.info()
        assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1), info
        assert 2 * 8 * info["pitch"] * H > 256 << 20  # kernel_variant's rule: variant 1
        assert e.pass_plan(STEPS) == [1] * STEPS
        run_default(O, e, H, W)


def test_below_the_auto_rule_stays_one_step(gpu, O, monkeypatch):
    H, W = 2047, 2048
    with engine(gpu, monkeypatch, H, W) as e:
        e.add_diffuse_field(0)
        info = e.info()
        assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1), info
        assert e.pass_plan(STEPS) == [1] * STEPS and e.pass_kernel(4)[0] == 0
        run_default(O, e, H, W)


# ---- 2. segments at the 2^31 offset cap ------------------------------------------------------
CAP_H, CAP_W = 8200, 32768
RATE = 0.1
BAND = 64
# exactly representable sixteenths: every product of two is exact, zeros and ones included
ROW_TABLE = np.array([0, 16, 8, 4, 12, 2, 6, 10, 14, 8, 4, 1, 5, 7, 3, 9]) / 16.0
COL_TABLE = np.array([8, 0, 16, 12, 4, 6, 2, 14, 10, 3, 16, 1, 9, 5, 7, 11]) / 16.0


def geom():
    """mm_geom.hpp's constants and its constexpr / inline integer functions, evaluated from
    the header's own text: a changed margin moves the expected segment lengths with it."""
    text = open(os.path.join(REPO, "mpi-model_amd", "csrc", "mm_geom.hpp")).read()
    ns = {n: int(v) for n, v in re.findall(r"constexpr int (\w+) = (\d+);", text)}
    for n, v in re.findall(r"constexpr int (\w+) = (\w+);", text):
        if not v.isdigit():
            ns[n] = ns[v]
    for name in ("field_ring", "fieldk_max_rows", "passk_max_rows"):
        m = re.search(r"\b%s\(([^)]*)\)\s*\{(.*?)\n\}" % name, text, re.S)
        params = [p.split()[-1] for p in m.group(1).split(",")]
        expr = re.search(r"return\s+(.*?);", m.group(2), re.S).group(1)
        expr = re.sub(r"(\d)LL\b", r"\1", expr).replace("/", "//")
        ns[name] = eval("lambda %s: %s" % (", ".join(params), expr), ns)
    return ns


def cap_field_rows(row0, n):
    """Rows [row0, row0 + n) of the cap grid's rate field: an outer product of a per-row and
    a per-column table entry picked by a multiplicative hash, so it differs by row and by
    column without a period."""
    i = np.arange(row0, row0 + n, dtype=np.uint64)
    j = np.arange(CAP_W, dtype=np.uint64)
    r = ROW_TABLE[(((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28)).astype(np.int64)]
    c = COL_TABLE[(((j * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28)).astype(np.int64)]
    return np.outer(r, c)


def cap_bands(rpw, K):
    """(first row, rows): the top; 64 rows around rpw / 2, where the byte offset passes 2^30
    -- at row 2^30 / row bytes of the output descriptor (base: the segment's first row) and
    K rows earlier in the input's (base: K rows above it), so a band that would end before
    the first is longer; and from 64 rows before the seam at `rpw` to the grid's last row."""
    cross = (1 << 30) // (CAP_W * 8)
    b = rpw // 2 - BAND // 2
    assert b + 8 <= cross - K - 1  # (a segment whose first input row is odd starts one higher)
    return [(0, BAND), (b, max(BAND, cross + 8 - b)), (rpw - BAND, CAP_H - rpw + BAND)]


def field_band_oracle(O, b, n, steps):
    """Rows [b, b + n) after `steps` rate-field steps. or_field_step_general weighs the first
    and last row of what it is given as grid edges: that error reaches `steps` rows into the
    band's shares and one row further into its values, so the cone is steps + 1 rows a side."""
    lo, hi = max(0, b - steps - 1), min(CAP_H, b + n + steps + 1)
    v = O.fill_random(CAP_H, CAP_W, lo, hi - lo)
    f, cnt = cap_field_rows(lo, hi - lo), neighbour_counts(hi - lo, CAP_W)
    for _ in range(steps):
        v = oracle_step(O, v, f, cnt)
    return v[b - lo:b - lo + n]


def uniform_band_oracle(O, b, n, steps):
    lo, hi = max(0, b - steps), min(CAP_H, b + n + steps)
    return large.band_oracle(O, CAP_H, CAP_W, lo, hi, steps, RATE)[b - lo:b - lo + n]


def check_cap_pass(e, O, K, rpw, oracle):
    """One pass of K with the sums off, then from a fresh state with the sums on (the same
    engine: the state buffers and the rate field stay where they are)."""
    bands = cap_bands(rpw, K)
    # two segments per strip: the cap, and a rest that ends at the grid's last row
    assert bands[2][0] + bands[2][1] == CAP_H and 16 <= CAP_H - rpw <= 92
    want = [oracle(O, b, n, K) for b, n in bands]
    for reduce_every in (0, 1):
        e.fill_random(0)
        s0 = e.sums()[0]
        assert e.pass_plan(K) == [K]
        e.clear_history()
        e.run(K, reduce_every)
        s1 = e.sums()[0]
        got = [e.read_rows(b, n) for b, n in bands]
        hist = e.sums_history()
        for (b, n), g, w in zip(bands, got, want):
            rows = np.flatnonzero(np.any(g != w, axis=1)) + b
            assert rows.size == 0, (K, reduce_every, "rows", rows[:8].tolist(), "seam", rpw,
                                    int(np.count_nonzero(g != w)))
        assert abs(s1 - s0) <= 1e-12 * s0, (K, reduce_every, s0, s1)
        if reduce_every:
            # every level's total is the conserved one. A wave adds at most 2 * rpw (16 300)
            # positive terms per lane before the tree: independent roundings, an expected
            # relative error of sqrt(16 300) * 2^-53 = 1.4e-14, far inside the project's bound
            assert hist.shape == (K, 1), hist.shape
            for s in range(K):
                assert abs(hist[s, 0] - s0) <= 1e-12 * s0, (K, s, hist[s, 0], s0)


@pytest.mark.parametrize("last", [False, True], ids=["K=2", "K=max"])
def test_fieldk_segment_at_the_offset_cap(gpu, O, monkeypatch, last):
    g = geom()
    K = gpu.FIELD_MAX_STEPS if last else 2
    assert g["kFieldMaxSteps"] == gpu.FIELD_MAX_STEPS
    with engine(gpu, monkeypatch, CAP_H, CAP_W, MM_SEG_WAVES=0.001, MM_FIELD_STEPS=K) as e:
        e.add_diffuse_field(0)
        info = e.info()
        assert info["pitch"] == CAP_W
        rpw = g["fieldk_max_rows"](K, info["pitch"]) & ~1
        assert (info["kernel"], info["steps_per_launch"], info["rows_per_wave"]) == (FIELDK, K, rpw), info
        assert e.pass_kernel(K)[0] == FIELDK
        # the deepest row a wave addresses stays below 2^31, and four more rows would not
        assert (rpw + 3 * K + 2 * g["field_ring"](K)) * CAP_W * 8 < 1 << 31
        assert (rpw + 3 * K + 2 * g["field_ring"](K) + 12) * CAP_W * 8 >= 1 << 31
        for row0 in range(0, CAP_H, 1024):  # the host holds one chunk at a time
            e.rate_field_upload(cap_field_rows(row0, min(1024, CAP_H - row0)), row0=row0)
        check_cap_pass(e, O, K, rpw, field_band_oracle)


@pytest.mark.parametrize("kernel,K", [(PASSK, 10), (WIDE, 20)], ids=["passk-K10", "wide-K20"])
def test_uniform_segment_at_the_offset_cap(gpu, O, monkeypatch, kernel, K):
    g = geom()
    assert (g["kMaxSteps"], g["kMaxWide"]) == (10, 20)  # each kernel's largest K
    with engine(gpu, monkeypatch, CAP_H, CAP_W, MM_SEG_WAVES=0.001, MM_WIDE=int(kernel == WIDE),
                MM_STEPS_PER_PASS=K) as e:
        e.add_diffuse(0, RATE)
        info = e.info()
        assert info["pitch"] == CAP_W
        rpw = g["passk_max_rows"](K, info["pitch"]) & ~1
        assert (info["kernel"], info["steps_per_launch"], info["rows_per_wave"]) == (kernel, K, rpw), info
        assert e.pass_kernel(K)[0] == kernel
        check_cap_pass(e, O, K, rpw, uniform_band_oracle)
