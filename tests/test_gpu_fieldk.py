"""K fused steps of the rate-field diffusion per pass on the GPU (mm_fieldk_kernel,
MM_FIELD_STEPS). Every fused level is the one-step kernel's arithmetic, so K fused steps are
or_field_step_general of oracle/mm_oracle.c with outf = f * v applied K times, bit for bit:
cells are compared with np.array_equal / tobytes, only the step sums (another summation
order) get the project's 1e-12 relative bound. The kernel is forced with MM_FIELD_STEPS=K
around engine creation; by default these small grids stay on the one-step kernel.
"""
import math

import numpy as np
import pytest

import value_classes as vc
from test_gpu_ratefield import (field_engine, make_chain, neighbour_counts, oracle_step,
                                random_field, reference, run_chain)
from test_gpu_values import run_engine, seed_positions
from test_gpu_values import reference as class_reference

pytestmark = pytest.mark.gpu

FIELDK = 4  # mm_info.kernel of mm_fieldk_kernel
SEG = {"MM_SEG_WAVES": 64}  # the shortest segments the planner makes: 16 rows


def out_cols(k):
    return 128 - 4 * ((k + 1) // 2)


# no neighbours, a single row / column, all corners, fewer rows than K, exactly one strip of
# output columns and one column more for out_cols 124 / 120 / 116, the loaded width and one
# more, a last strip of few columns, three strips, and several 16-row segments with a short
# tail (every level is recomputed across the segment seams)
SHAPES = [((1, 1), {}), ((1, 7), {}), ((5, 1), {}), ((2, 2), {}), ((3, 5), {}), ((3, 130), {}),
          ((9, 124), {}), ((9, 125), {}), ((9, 120), {}), ((9, 121), {}), ((9, 116), {}),
          ((9, 117), {}), ((8, 128), {}), ((9, 129), {}), ((27, 257), {}), ((17, 384), {}),
          ((64, 130), {}), ((50, 257), SEG)]


def shape_id(s):
    return "%dx%d" % s[0] + ("-seg" if s[1] else "")


def built_ks(gpu):
    return range(2, gpu.FIELD_MAX_STEPS + 1)


def fk_engine(gpu, O, monkeypatch, H, W, K=None, f=None, **env):
    """field_engine (fill_random state, random_field rates, one field diffusion) created with
    MM_FIELD_STEPS=K and `env` set."""
    if K is not None:
        env = dict(env, MM_FIELD_STEPS=K)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return field_engine(gpu, O, H, W, f=f)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def check_fieldk_plan(e, W, K):
    info = e.info()
    assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (FIELDK, K, K), info
    assert e.pass_kernel(K) == (FIELDK, 2, -(-W // out_cols(K)))
    assert e.pass_kernel(1)[0] == 0


# ---- 1. parity with the oracle, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("K", range(2, 5))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_parity_with_general_step(gpu, O, monkeypatch, shape, K):
    (H, W), env = shape
    assert gpu.FIELD_MAX_STEPS >= 4
    for steps in (K, 2 * K + 1, 17):
        with fk_engine(gpu, O, monkeypatch, H, W, K, **env) as e:
            check_fieldk_plan(e, W, K)
            plan = e.pass_plan(steps)
            assert sum(plan) == steps and max(plan) <= K and min(plan) >= 1, plan
            e.run(steps)
            got = e.download()
        assert np.array_equal(got, reference(O, H, W, steps)), (steps, plan)


def test_every_built_k_is_tested(gpu):
    assert list(built_ks(gpu)) == [2, 3, 4]  # the K of test_parity_with_general_step


# ---- 2. K-step equals one-step, no oracle involved --------------------------------------------
def test_k_step_equals_one_step(gpu, O, monkeypatch):
    H, W, steps = 130, 300, 20
    with fk_engine(gpu, O, monkeypatch, H, W, 4) as e:
        check_fieldk_plan(e, W, 4)
        e.run(steps)
        fused = e.download()
    with fk_engine(gpu, O, monkeypatch, H, W, 1) as e:
        info = e.info()
        assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1)
        e.run(steps)
        single = e.download()
    assert fused.tobytes() == single.tobytes()


# ---- 3. NaN in the pitch padding of the state and of the field --------------------------------
@pytest.mark.parametrize("last", [False, True], ids=["K=2", "K=max"])
@pytest.mark.parametrize("shape", [((9, 129), {}), ((27, 257), {}), ((50, 257), SEG)], ids=shape_id)
def test_parity_with_nan_padding(gpu, O, monkeypatch, shape, last):
    (H, W), env = shape
    K = gpu.FIELD_MAX_STEPS if last else 2
    steps = 2 * K + 1
    with fk_engine(gpu, O, monkeypatch, H, W, K, **env) as e:
        check_fieldk_plan(e, W, K)
        e.fill_padding(float("nan"))
        e.run(steps, reduce_every=1)
        got = e.download()
        hist = e.sums_history()
    assert np.array_equal(got, reference(O, H, W, steps))
    assert hist.shape == (steps, 1) and np.all(np.isfinite(hist))
    for s in range(1, steps + 1):
        want = math.fsum(reference(O, H, W, s).ravel())
        assert abs(hist[s - 1, 0] - want) <= 1e-12 * abs(want), s


# ---- 4. the value classes: signed, zero, subnormal, huge, non-finite ---------------------------
@pytest.mark.parametrize("last", [False, True], ids=["K=2", "K=max"])
def test_value_classes(gpu, O, monkeypatch, last):
    shape = (50, 257)
    K = gpu.FIELD_MAX_STEPS if last else 2
    f, cnt = random_field(*shape), neighbour_counts(*shape)
    for cls in vc.CLASSES:
        with fk_engine(gpu, O, monkeypatch, *shape, K, f=f, **SEG) as e:
            check_fieldk_plan(e, shape[1], K)
            info = e.info()
            # the plan has every seam: several segments, an interior strip between two edge ones
            assert shape[0] > info["rows_per_wave"] and shape[1] > 2 * out_cols(K), info
            pos = seed_positions(shape, info["rows_per_wave"], out_cols(K))
            assert len(pos) >= 8, pos
            start = [vc.make(cls, *shape, positions=pos)]
            key = ("fieldk", shape, cls, pos)
            run_engine(O, e, cls, start,
                       lambda n: class_reference(key, start,
                                                 lambda v: [oracle_step(O, v[0], f, cnt)], n),
                       (K, 1), pos, (shape, K))  # one pass of K, then one more step


# ---- 5. step sums and conservation ------------------------------------------------------------
def test_step_sums_and_conservation(gpu, O, monkeypatch):
    H, W, steps = 64, 130, 10
    with fk_engine(gpu, O, monkeypatch, H, W, 4) as e:
        check_fieldk_plan(e, W, 4)
        e.run(steps, reduce_every=1)
        hist = e.sums_history()
        assert e.info()["hist_entries"] == steps
    assert hist.shape == (steps, 1)
    total = math.fsum(O.fill_random(H, W).ravel())
    for s in range(1, steps + 1):
        want = math.fsum(reference(O, H, W, s).ravel())
        assert abs(hist[s - 1, 0] - want) <= 1e-12 * abs(want), s
        assert abs(hist[s - 1, 0] - total) <= 1e-12 * abs(total), s
    with fk_engine(gpu, O, monkeypatch, H, W, 4) as e:
        e.run(steps, reduce_every=3)
        hist = e.sums_history()
        got = e.download()
    assert hist.shape == (3, 1)
    for i, s in enumerate((3, 6, 9)):
        want = math.fsum(reference(O, H, W, s).ravel())
        assert abs(hist[i, 0] - want) <= 1e-12 * abs(want), s
    assert np.array_equal(got, reference(O, H, W, steps))


# ---- 6. graphs, prepare, a re-uploaded field --------------------------------------------------
def test_graph_replay_and_prepare(gpu, O, monkeypatch):
    H, W, steps = 64, 130, 64
    with fk_engine(gpu, O, monkeypatch, H, W, 4) as e:
        check_fieldk_plan(e, W, 4)
        e.run(steps)
        graphed = e.download()
        assert e.info()["graph_state"] == 1
    with fk_engine(gpu, O, monkeypatch, H, W, 4, MM_GRAPH=0) as e:
        check_fieldk_plan(e, W, 4)
        e.run(steps)
        eager = e.download()
        assert e.info()["graph_state"] == 0
    with fk_engine(gpu, O, monkeypatch, H, W, 4) as e:
        e.prepare(steps)
        assert np.array_equal(e.download(), O.fill_random(H, W))  # prepare ran no step
        e.run(steps)
        prepared = e.download()
        assert e.info()["graph_state"] == 1
    assert graphed.tobytes() == eager.tobytes()
    assert prepared.tobytes() == eager.tobytes()
    assert np.array_equal(eager, reference(O, H, W, steps))


def test_reuploaded_field_takes_effect(gpu, O, monkeypatch):
    # the graphs hold the field's address, not its values
    H, W, steps = 64, 130, 16
    f2, cnt = random_field(H, W, seed=99), neighbour_counts(H, W)
    with fk_engine(gpu, O, monkeypatch, H, W, 4) as e:
        check_fieldk_plan(e, W, 4)
        e.run(steps)
        e.rate_field_upload(f2)
        e.run(steps)
        got = e.download()
        info = e.info()
    assert info["graph_state"] == 1 and info["steps_done"] == 2 * steps
    want = reference(O, H, W, steps)
    for _ in range(steps):
        want = oracle_step(O, want, f2, cnt)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("K", [4, 3])
def test_odd_flip_graph_replays(gpu, O, monkeypatch, K):
    """run(3K) is three passes: one graph with an odd number of buffer flips, so its three
    replays start from alternating buffer parities; run(K) after them is an eager pass. The
    state after every call against the oracle and against an engine that never captures, with
    another field uploaded between the second and the third replay."""
    H, W = 64, 130
    calls = [3 * K, 3 * K, 3 * K, K, K]
    f1, f2, cnt = random_field(H, W), random_field(H, W, seed=99), neighbour_counts(H, W)
    want, v = [], O.fill_random(H, W)
    for i, n in enumerate(calls):
        for _ in range(n):
            v = oracle_step(O, v, f2 if i >= 2 else f1, cnt)
        want.append(v)
    assert np.array_equal(want[1], reference(O, H, W, 6 * K))
    got = {}
    for graphs in (1, 0):
        env = {} if graphs else {"MM_GRAPH": 0}
        with fk_engine(gpu, O, monkeypatch, H, W, K, **env) as e:
            check_fieldk_plan(e, W, K)
            assert e.pass_plan(3 * K) == [K] * 3 and e.pass_plan(K) == [K]
            done = 0
            for i, n in enumerate(calls):
                if i == 2:
                    e.rate_field_upload(f2)
                e.run(n)
                done += n
                got[graphs, i] = e.download()
                info = e.info()
                assert info["steps_done"] == done, (graphs, i, info)
                if i == 0:
                    assert info["graph_state"] == graphs, info
                    if graphs:
                        assert info["graph_launches"] == 1, info
                if i == 2 and graphs:  # one captured graph per buffer parity, replayed
                    assert info["graph_launches"] == 3 and info["graph_count"] == 2, info
            if not graphs:
                assert info["graph_state"] == 0 and info["graph_launches"] == 0, info
    for i in range(len(calls)):
        assert np.array_equal(got[1, i], want[i]), (K, i)
        assert got[1, i].tobytes() == got[0, i].tobytes(), (K, i)


# ---- 7. where it must not run -----------------------------------------------------------------
def one_step(e):
    info = e.info()
    return (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1)


def test_chains_stay_one_step(gpu, O, monkeypatch):
    H, W, G, steps = 27, 257, 3, 5
    f = random_field(H, W)
    engines = make_chain(gpu, monkeypatch, H, W, G, env={"MM_FIELD_STEPS": 4})
    try:
        for e in engines:
            e.fill_random(0)
            lo, hi = max(e.x_init - 1, 0), min(e.x_init + e.h + 1, H)
            e.rate_field_upload(f[lo:hi], row0=lo - e.x_init)
            e.add_diffuse_field(0)
            assert one_step(e)
        assert run_chain(engines, steps) == 1
        got = np.vstack([e.download() for e in engines])
    finally:
        for e in engines:
            e.close()
    assert np.array_equal(got, reference(O, H, W, steps))


def test_self_halo_stays_one_step(gpu, O, monkeypatch):
    H, W, steps = 64, 130, 5
    monkeypatch.setenv("MM_SELF_HALO", "1")
    monkeypatch.setenv("MM_FIELD_STEPS", "4")
    e = gpu.Engine(H, W, halo_mode=gpu.MM_HALO_RCCL, comm_id_bytes=gpu.comm_id())
    monkeypatch.delenv("MM_SELF_HALO")
    monkeypatch.delenv("MM_FIELD_STEPS")
    try:
        e.upload(O.fill_random(H, W))
        e.rate_field_upload(random_field(H, W))
        e.add_diffuse_field(0)
        assert one_step(e)
        e.run(steps)
        got = e.download()
    finally:
        e.close()
    assert np.array_equal(got, reference(O, H, W, steps))


def test_other_programs_stay_one_step(gpu, O, monkeypatch):
    H, W, steps = 27, 257, 4
    f, cnt = random_field(H, W), neighbour_counts(H, W)
    init = [O.fill_random(H, W, seed=O.SEED + a) for a in range(3)]

    def engine3():
        monkeypatch.setenv("MM_FIELD_STEPS", "4")
        e = gpu.Engine(H, W, n_attr=3)
        monkeypatch.delenv("MM_FIELD_STEPS")
        for a in range(3):
            e.upload(init[a], a)
        e.rate_field_upload(f, attr=1)
        return e

    # three attributes, one field diffusion: the others are copied through
    with engine3() as e:
        e.add_diffuse_field(1)
        assert one_step(e) and e.info()["n_passes"] == 1
        e.run(steps)
        got = [e.download(a) for a in range(3)]
    want = init[1]
    for _ in range(steps):
        want = oracle_step(O, want, f, cnt)
    assert got[0].tobytes() == init[0].tobytes() and got[2].tobytes() == init[2].tobytes()
    assert np.array_equal(got[1], want)

    # a field diffusion between a transfer and a uniform diffusion: three passes per step
    with engine3() as e:
        e.add_transfer(0, 1, 0.05)
        e.add_diffuse_field(1)
        e.add_diffuse(2, 0.2)
        assert one_step(e) and e.info()["n_passes"] == 3
        e.run(steps)
        got = [e.download(a) for a in range(3)]
    fields = list(init)
    for _ in range(steps):
        fields = O.program_step(fields, [(O.TRANSFER, 0, 1, 0.05)])
        fields[1] = oracle_step(O, fields[1], f, cnt)
        fields = O.program_step(fields, [(O.DIFFUSE, 2, 2, 0.2)])
    for a in range(3):
        assert np.array_equal(got[a], fields[a]), a

    # MM_PASSK=0 means one step per kernel pass, here too
    with fk_engine(gpu, O, monkeypatch, H, W, 4, MM_PASSK=0) as e:
        assert one_step(e)
        assert e.pass_plan(7) == [1] * 7 and e.pass_kernel(4)[0] == 0
        e.run(steps)
        got1 = e.download()
    assert np.array_equal(got1, reference(O, H, W, steps))


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_defaults_on_small_grids_are_untouched(gpu, O, monkeypatch, shape):
    (H, W), env = shape
    with fk_engine(gpu, O, monkeypatch, H, W, None, **env) as e:
        assert one_step(e)
        assert e.pass_plan(5) == [1] * 5


# ---- 8. refusals --------------------------------------------------------------------------------
def test_refusals(gpu, monkeypatch):
    H, W = 8, 130
    monkeypatch.setenv("MM_FIELD_STEPS", "4")
    e = gpu.Engine(H, W)
    monkeypatch.delenv("MM_FIELD_STEPS")
    with e:
        e.fill(0, value=1.0)
        e.add_diffuse_field(0)
        assert e.info()["kernel"] == FIELDK
        with pytest.raises(gpu.MMError):
            e.run(4)  # no field yet
        with pytest.raises(gpu.MMError):
            e.prepare(8)
        e.rate_field_fill(0.0)
        e.run(4)
        assert np.array_equal(e.download(), np.ones((H, W)))
