"""Every instance the K-step kernels' lookup table can return, bit for bit against the oracle.

One case per descriptor family: mm_passk_kernel K = 1..10 and mm_wide_kernel K = 4..20 (one
attribute), the four-attribute mm_wide_kernel instances (K = 4; K = 8 with N = 1..4 diffusing
attributes, with and without a post-chain; the ring instance and its run-time-chain stand-in),
the border launches of a halo-split slab, and the rate-field family (mm_field_kernel and
mm_fieldk_kernel K = 2..4, against or_field_step_general). Every case runs with the step sums off and on
and with MM_KERNEL_VARIANT 0 and 1 (non-temporal stores), and checks through mm_pass_kernel /
mm_engine_info that the intended kernel, K and columns per lane are the ones planned, so a
silent fall-back to another instance fails it.
"""
import math

import pytest

import numpy as np

import test_gpu_ratefield as ratefield
from test_gpu_halo import close, gather, make_chain, run_chain
from test_gpu_parity import C5_FLOWS, WIDE_PROGRAMS, add_flows

pytestmark = pytest.mark.gpu

RATE = 0.3
ONE = (130, 450)   # >= 3 strips at K = 20 (216 output columns per strip), 5 at K = 10
FOUR = (67, 300)   # 3 strips of 112 output columns for the four-attribute instances
PASSK, WIDE = 2, 3  # mm_info.kernel
# MM_SEG_WAVES as the parity tests set it: the shortest segments the planner makes
SEG = {"MM_SEG_WAVES": 64}

_refs = {}


def reference(O, shape, n_attr, flows, steps):
    """Oracle states and per-step sums after 1..steps steps, computed once per program."""
    key = (shape, n_attr, tuple(flows))
    states, sums = _refs.setdefault(
        key, ([[O.fill_random(*shape, seed=O.SEED + a) for a in range(n_attr)]], [None]))
    while len(states) <= steps:
        nxt, s = O.program_step(states[-1], list(flows), steps=1, sums_per_step=True)
        states.append(nxt)
        sums.append(s[0])
    return states, sums


def out_cols(kernel, k, cols):
    if kernel == PASSK:
        return 128 - 4 * ((k + 1) // 2)
    return 64 * cols - 2 * cols * ((k + cols - 1) // cols)


def check_plan(e, shape, kernel, k, cols, chain=None):
    """The kernel family, K and columns per lane that will run, and a segment plan with a
    segment wholly inside rows [K+1, H-K-2] of an interior strip (the FAST body)."""
    H, W = shape
    info = e.info()
    ns = -(-W // out_cols(kernel, k, cols))
    assert (info["kernel"], info["steps_per_launch"]) == (kernel, k), info
    assert e.pass_kernel(k) == (kernel, cols, ns)
    if chain is not None:
        assert info["chain_kernel"] == chain, info
    r = info["rows_per_wave"]
    nseg = -(-H // r)
    assert any(i * r >= k + 1 and (i + 1) * r - 1 <= H - k - 2 for i in range(nseg)), info
    # (the one-attribute wide strips of K = 4, 8, 12 are 248, 240, 232 columns: two strips
    # of 450 columns, both edge strips; every other case has interior strips)
    assert ns >= 3 or (kernel == WIDE and cols == 4 and k <= 12)
    per = 4 if kernel == WIDE else 1  # waves per workgroup of every mm_wide_kernel instance
    assert info["waves_per_pass"] % per == 0
    assert info["waves_per_pass"] // per >= max(ns - 2, 0) * nseg + 2, info


def run_case(gpu, O, monkeypatch, shape, n_attr, flows, env, kernel, k, cols, chain=None):
    steps = 4 if k <= 4 else k + 1  # K <= 4: four steps; else one pass of K and one more step
    states, sums = reference(O, shape, n_attr, flows, steps)
    for variant in (0, 1):
        for reduce_every in (0, 1):
            full = {**SEG, **env, "MM_KERNEL_VARIANT": variant}
            for name, v in full.items():
                monkeypatch.setenv(name, str(v))
            e = gpu.Engine(*shape, n_attr=n_attr)
            for name in full:
                monkeypatch.delenv(name)
            try:
                for a in range(n_attr):
                    e.fill_random(a, seed=O.SEED + a)
                add_flows(e, flows)
                check_plan(e, shape, kernel, k, cols, chain)
                # a run of K steps is one pass of K (a longer run is split into balanced
                # passes, which need not hold one of K); the remaining steps in a second run
                assert e.pass_plan(k) == [k]
                e.run(k, reduce_every)
                if steps > k:
                    e.run(steps - k, reduce_every)
                got = [e.download(a) for a in range(n_attr)]
                hist = e.sums_history()
            finally:
                e.close()
            what = (variant, reduce_every)
            for a in range(n_attr):
                assert np.array_equal(got[a], states[steps][a]), (what, a)
            if reduce_every:
                assert hist.shape == (steps, n_attr), what
                for s in range(steps):
                    for a in range(n_attr):
                        w = sums[s + 1][a]
                        assert abs(hist[s, a] - w) <= 1e-12 * abs(w), (what, s, a)


DIFFUSE = [(1, 0, 0, RATE)]


@pytest.mark.parametrize("k", range(1, 11))
def test_passk_instance(gpu, O, monkeypatch, k):
    run_case(gpu, O, monkeypatch, ONE, 1, DIFFUSE, {"MM_WIDE": 0, "MM_STEPS_PER_PASS": k},
             PASSK, k, 2)


@pytest.mark.parametrize("k", [4, 8, 12, 16, 20])
def test_wide_instance(gpu, O, monkeypatch, k):
    run_case(gpu, O, monkeypatch, ONE, 1, DIFFUSE, {"MM_WIDE": 1, "MM_STEPS_PER_PASS": k},
             WIDE, k, 4)


@pytest.mark.parametrize("prog", range(len(WIDE_PROGRAMS)))
def test_widea_k4_instance(gpu, O, monkeypatch, prog):
    run_case(gpu, O, monkeypatch, FOUR, 4, WIDE_PROGRAMS[prog],
             {"MM_WIDE": 1, "MM_STEPS_PER_PASS": 4}, WIDE, 4, 2, gpu.MM_CHAIN_RUNTIME)


# K = 8, four attributes: N of them diffuse (not the first N: the engine relabels them), a
# pre-chain, with or without a post-chain (one transfer into a sink)
PRE = [(2, 0, 1, 0.1), (2, 3, 2, 0.05)]
POST = [(2, 1, 0, 0.07), (2, 2, -1, 0.01)]
DIFFUSING = {1: (2,), 2: (1, 3), 3: (0, 2, 3), 4: (0, 1, 2, 3)}


@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_widea_k8_instance(gpu, O, monkeypatch, n, post):
    flows = PRE + [(1, a, a, 0.05 * (a + 1)) for a in DIFFUSING[n]] + (POST if post else [])
    run_case(gpu, O, monkeypatch, FOUR, 4, flows, {"MM_WIDE": 1}, WIDE, 8, 2,
             gpu.MM_CHAIN_RUNTIME)


@pytest.mark.parametrize("ring", [1, 0])
def test_widea_ring_instance(gpu, O, monkeypatch, ring):
    # C5's pre-chain is the ring t -> t+1 mod 4: the compile-time-chain instance, or with
    # MM_CHAIN_RING=0 the run-time-chain instance of four diffusing attributes, no post-chain
    run_case(gpu, O, monkeypatch, FOUR, 4, C5_FLOWS, {"MM_WIDE": 1, "MM_CHAIN_RING": ring},
             WIDE, 8, 2, gpu.MM_CHAIN_RING if ring else gpu.MM_CHAIN_RUNTIME)


# ---- the rate-field family: mm_field_kernel and mm_fieldk_kernel K = 2..FIELD_MAX_STEPS --------
FIELD = (50, 257)  # with SEG: four 16-row segments, an interior strip between two edge strips
FIELD_KS = (1, 2, 3, 4)  # MM_FIELD_STEPS: 1 is mm_field_kernel, the others mm_fieldk_kernel<K>


def run_field_case(gpu, O, monkeypatch, k):
    """run_case for a one-attribute rate-field diffusion: state fill_random, rates
    random_field, one pass of K and one more step, against or_field_step_general iterated."""
    import test_gpu_fieldk as fieldk  # (imports this module through test_gpu_values)
    H, W = FIELD
    steps = k + 1
    for variant in (0, 1):
        for reduce_every in (0, 1):
            with fieldk.fk_engine(gpu, O, monkeypatch, H, W, k, **SEG,
                                  MM_KERNEL_VARIANT=variant) as e:
                info = e.info()
                if k == 1:
                    assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1)
                    assert e.pass_kernel(1)[0] == 0 and info["pitch"] == 3 * 128
                else:
                    fieldk.check_fieldk_plan(e, W, k)
                    assert W > 2 * fieldk.out_cols(k)  # an interior strip
                assert info["rows_per_wave"] * 3 <= H, info  # several segments, one interior
                assert e.pass_plan(k) == [k] and e.pass_plan(1) == [1]
                e.run(k, reduce_every)
                e.run(1, reduce_every)
                got = e.download()
                hist = e.sums_history()
            what = (k, variant, reduce_every)
            assert np.array_equal(got, ratefield.reference(O, H, W, steps)), what
            if reduce_every:
                assert hist.shape == (steps, 1), what
                for s in range(1, steps + 1):
                    w = math.fsum(ratefield.reference(O, H, W, s).ravel())
                    assert abs(hist[s - 1, 0] - w) <= 1e-12 * abs(w), (what, s)


@pytest.mark.parametrize("k", FIELD_KS)
def test_field_instance(gpu, O, monkeypatch, k):
    run_field_case(gpu, O, monkeypatch, k)


def test_every_built_field_k_is_tested(gpu):
    # a K = 5 instance added to mm_fieldk_kernel must be added to FIELD_KS
    import test_gpu_fieldk as fieldk
    assert list(FIELD_KS) == list(range(1, gpu.FIELD_MAX_STEPS + 1))
    assert list(fieldk.built_ks(gpu)) == list(FIELD_KS[1:])


@pytest.mark.parametrize("kernel,k", [(PASSK, 5), (WIDE, 8)])
def test_border_instances_host_halo(gpu, O, monkeypatch, kernel, k):
    # two slabs of 65 rows with a host halo: interior segments and, for the 2 x K rows that
    # read exchanged ghost rows, the border launches (mm_passk_kernel: 4-row blocks)
    H, W = ONE
    steps = k + 1
    states, sums = reference(O, ONE, 1, DIFFUSE, steps)
    for reduce_every in (0, 1):
        env = {**SEG, "MM_WIDE": int(kernel == WIDE), "MM_STEPS_PER_PASS": k}
        engines = make_chain(gpu, monkeypatch, H, W, 2, env=env)
        try:
            for e in engines:
                e.fill_random(0)
                add_flows(e, DIFFUSE)
                info = e.info()
                assert (info["kernel"], info["steps_per_launch"]) == (kernel, k), info
                assert info["halo_depth"] == k
                assert e.pass_kernel(k)[:2] == (kernel, 4 if kernel == WIDE else 2)
            assert all(e.pass_plan(k) == [k] for e in engines)
            run_chain(engines, k, reduce_every)
            run_chain(engines, steps - k, reduce_every)
            got = gather(engines)
            hists = [e.sums_history() for e in engines]
        finally:
            close(engines)
        assert np.array_equal(got, states[steps][0]), reduce_every
        if reduce_every:
            assert all(h.shape == (steps, 1) for h in hists)
            for s in range(steps):
                w = sums[s + 1][0]
                assert abs(sum(h[s, 0] for h in hists) - w) <= 1e-12 * abs(w), s
