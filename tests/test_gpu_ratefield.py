"""Rate-field diffusion on the GPU (MM_FLOW_DIFFUSE_FIELD, mm_field_kernel): a per-cell
Exponencial rate. The contract is or_field_step_general of oracle/mm_oracle.c with
outf = f * v, bit for bit -- the reference's per-emitter update (src/Model.hpp:199,206-211,
234) applied to an outflow field -- so the cells are compared with np.array_equal and only
the step sums (another summation order) and the per-receiver uniform kernel (another
rounding) get the project's 1e-12 relative bound.
"""
import math

import numpy as np
import pytest

from conftest import golden, golden_points

pytestmark = pytest.mark.gpu

# no neighbours, a single row / column, all-corner grids, a row block that is exactly full,
# a strip boundary at 128 and at 256 with one column beyond, an odd W, three exact strips
SHAPES = [(1, 1), (1, 7), (5, 1), (2, 2), (3, 5), (8, 128), (9, 129), (27, 257), (64, 130),
          (17, 384)]
STEPS = (1, 3, 17)


def random_field(H, W, seed=7):
    """Uniform in [0, 0.5], about a quarter of the cells exactly 0.0, a few exactly 1.0."""
    rng = np.random.default_rng(seed + 1000003 * H + W)
    f = rng.uniform(0.0, 0.5, (H, W))
    pick = rng.random((H, W))
    f[pick < 0.25] = 0.0
    f[pick > 0.97] = 1.0
    return f


def neighbour_counts(H, W):
    sx = 1 + (np.arange(H) > 0) + (np.arange(H) < H - 1)
    sy = 1 + (np.arange(W) > 0) + (np.arange(W) < W - 1)
    return np.outer(sx, sy) - 1


def oracle_step(O, v, f, cnt):
    return O.field_step_general(v, np.where(cnt > 0, f * v, 0.0))


_REF = {}


def reference(O, H, W, steps):
    """State after `steps` steps of fill_random(H, W) under random_field(H, W): computed once
    per shape (every step up to the deepest asked for so far is kept), never modified."""
    states = _REF.setdefault((H, W), [O.fill_random(H, W)])
    f, cnt = random_field(H, W), neighbour_counts(H, W)
    while len(states) <= steps:
        nxt = oracle_step(O, states[-1], f, cnt)
        nxt.setflags(write=False)
        states.append(nxt)
    return states[steps]


def field_engine(gpu, O, H, W, f=None, **kw):
    e = gpu.Engine(H, W, **kw)
    e.upload(O.fill_random(H, W))
    e.rate_field_upload(random_field(H, W) if f is None else f)
    e.add_diffuse_field(0)
    return e


@pytest.mark.parametrize("name", golden_points())
def test_point_source_field_matches_reference_golden(gpu, name):
    # a field that is zero but at the source, on a grid of 1.0: the outflow f * 1.0 is
    # exactly the reference's rate * captured, and one step is its single-source flow
    g = golden(name)
    H, W = g["dimx"], g["dimy"]
    f = np.zeros((H, W))
    f[g["src_x"], g["src_y"]] = float.fromhex(g["rate_hex"]) * float.fromhex(g["value_hex"])
    with gpu.Engine(H, W) as e:
        e.fill(0, value=1.0)
        e.rate_field_upload(f)
        e.add_diffuse_field(0)
        e.run(1)
        v = e.download()
    changed = sorted([x, y, val.hex()] for (x, y), val in np.ndenumerate(v) if val != 1.0)
    assert changed == g["changed"]


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_parity_with_general_step(gpu, O, H, W, steps):
    with field_engine(gpu, O, H, W) as e:
        info = e.info()
        assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1)
        e.run(steps)
        got = e.download()
    assert np.array_equal(got, reference(O, H, W, steps))


@pytest.mark.parametrize("H,W", SHAPES)
def test_parity_with_nan_padding(gpu, O, H, W):
    # the pitch padding of the state AND of the field holds NaN: columns >= W weigh 0 by select
    with field_engine(gpu, O, H, W) as e:
        e.fill_padding(float("nan"))
        e.run(3, reduce_every=1)
        got = e.download()
        hist = e.sums_history()
    assert np.array_equal(got, reference(O, H, W, 3))
    assert np.all(np.isfinite(hist)) and hist.shape == (3, 1)


def test_zero_field_changes_nothing(gpu, O):
    H, W = 27, 257
    with field_engine(gpu, O, H, W, f=np.zeros((H, W))) as e:
        e.run(5)
        got = e.download()
    assert np.array_equal(got, O.fill_random(H, W))


@pytest.mark.parametrize("H,W", [(64, 96), (130, 97)])
def test_constant_field_tracks_uniform_diffusion(gpu, O, H, W):
    # per-emitter against per-receiver rounding: the project's bound (tests/test_oracle.py,
    # 3.6e-14 measured there)
    r, steps = 0.1, 20
    with gpu.Engine(H, W) as e:
        e.fill_random(0)
        e.rate_field_fill(r)
        e.add_diffuse_field(0)
        e.run(steps)
        got = e.download()
    with gpu.Engine(H, W) as e:
        e.fill_random(0)
        e.add_diffuse(0, r)
        e.run(steps)
        uni = e.download()
    err = np.max(np.abs(got - uni) / np.abs(uni))
    print(f"constant field vs uniform diffusion {H}x{W}: max relative difference {err:.3e}")
    assert err <= 1e-12


def test_step_sums_and_conservation(gpu, O):
    H, W, steps = 64, 130, 10
    with field_engine(gpu, O, H, W) as e:
        e.run(steps, reduce_every=1)
        hist = e.sums_history()
        assert e.info()["hist_entries"] == steps
    assert hist.shape == (steps, 1)
    total = math.fsum(O.fill_random(H, W).ravel())
    for s in range(1, steps + 1):
        want = math.fsum(reference(O, H, W, s).ravel())
        assert abs(hist[s - 1, 0] - want) <= 1e-12 * abs(want), s
        assert abs(hist[s - 1, 0] - total) <= 1e-12 * abs(total), s


def test_other_attributes_are_copied_through(gpu, O):
    H, W, steps = 27, 257, 4
    init = [O.fill_random(H, W, seed=O.SEED + a) for a in range(3)]
    init[0][3, 5] = -0.0  # a copy keeps the sign of zero; v + 0.0 would not
    f, cnt = random_field(H, W), neighbour_counts(H, W)
    with gpu.Engine(H, W, n_attr=3) as e:
        for a in range(3):
            e.upload(init[a], a)
        e.rate_field_upload(f, attr=1)
        e.add_diffuse_field(1)
        assert e.info()["n_passes"] == 1
        e.run(steps, reduce_every=1)
        got = [e.download(a) for a in range(3)]
        hist = e.sums_history()
    want = init[1]
    for _ in range(steps):
        want = oracle_step(O, want, f, cnt)
    assert got[0].tobytes() == init[0].tobytes()
    assert got[2].tobytes() == init[2].tobytes()
    assert np.array_equal(got[1], want)
    for a, w in enumerate((init[0], want, init[2])):
        assert abs(hist[-1, a] - math.fsum(w.ravel())) <= 1e-12 * abs(math.fsum(w.ravel()))


def test_field_pass_between_other_passes(gpu, O):
    # transfer 0 -> 1, field-diffuse 1, uniform diffuse 2: three passes per step, composed on
    # the CPU from the oracle's program step and its general step
    H, W, steps = 27, 257, 6
    fields = [O.fill_random(H, W, seed=O.SEED + a) for a in range(3)]
    f, cnt = random_field(H, W), neighbour_counts(H, W)
    with gpu.Engine(H, W, n_attr=3) as e:
        for a in range(3):
            e.upload(fields[a], a)
        e.rate_field_upload(f, attr=1)
        e.add_transfer(0, 1, 0.05)
        e.add_diffuse_field(1)
        e.add_diffuse(2, 0.2)
        assert e.info()["n_passes"] == 3
        e.run(steps)
        got = [e.download(a) for a in range(3)]
    for _ in range(steps):
        fields = O.program_step(fields, [(O.TRANSFER, 0, 1, 0.05)])
        fields[1] = oracle_step(O, fields[1], f, cnt)
        fields = O.program_step(fields, [(O.DIFFUSE, 2, 2, 0.2)])
    for a in range(3):
        assert np.array_equal(got[a], fields[a]), a


def test_field_diffusions_back_to_back_share_a_pass(gpu, O):
    H, W, steps = 9, 129, 3
    init = [O.fill_random(H, W, seed=O.SEED + a) for a in range(3)]
    fs = [random_field(H, W, seed=11 + a) for a in range(3)]
    cnt = neighbour_counts(H, W)
    with gpu.Engine(H, W, n_attr=3) as e:
        for a in range(3):
            e.upload(init[a], a)
        for a in (0, 2):
            e.rate_field_upload(fs[a], attr=a)
            e.add_diffuse_field(a)
        assert e.info()["n_passes"] == 1
        e.run(steps)
        got = [e.download(a) for a in range(3)]
        e.add_diffuse_field(2)  # the same attribute again: a pass of its own
        assert e.info()["n_passes"] == 2
    want = list(init)
    for _ in range(steps):
        for a in (0, 2):
            want[a] = oracle_step(O, want[a], fs[a], cnt)
    for a in range(3):
        assert np.array_equal(got[a], want[a]), a


# ---- chains: copies of tests/test_gpu_halo.py's host-transport helpers ---------------------
def make_chain(gpu, monkeypatch, H, W, G, n_attr=1, env=None):
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    engines = []
    try:
        for g in range(G):
            x0, h = gpu.partition_rows(H, G, g)
            engines.append(gpu.Engine(H, W, x0, h, n_attr=n_attr, rank=g, nranks=G,
                                      halo_mode=gpu.MM_HALO_HOST))
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return engines


def run_chain(engines, steps, reduce_every=0):
    G = len(engines)
    depth = engines[0].info()["halo_depth"]
    assert all(e.info()["halo_depth"] == depth for e in engines)
    plan = engines[0].pass_plan(steps)
    assert all(e.pass_plan(steps) == plan for e in engines)
    for k in plan:
        halos = [e.halo_export(k) for e in engines]
        for g, e in enumerate(engines):
            e.halo_import(halos[g - 1][1] if g > 0 else None,
                          halos[g + 1][0] if g < G - 1 else None, nrows=k)
        for e in engines:
            e.run(k, reduce_every)
    return depth


@pytest.mark.parametrize("H,W,G", [(77, 300, 4), (27, 257, 3), (16, 130, 8)])
def test_chain_with_host_transport(gpu, O, monkeypatch, H, W, G):
    # slabs split into interior and one-row border launches (77 / 4, 27 / 3) and slabs too
    # thin to split (16 / 8: two rows); every slab holds its rows -1..h of one global field
    steps = 5
    f = random_field(H, W)
    engines = make_chain(gpu, monkeypatch, H, W, G)
    try:
        for e in engines:
            e.fill_random(0)
            lo, hi = max(e.x_init - 1, 0), min(e.x_init + e.h + 1, H)
            e.rate_field_upload(f[lo:hi], row0=lo - e.x_init)
            e.add_diffuse_field(0)
        assert run_chain(engines, steps, reduce_every=1) == 1
        got = np.vstack([e.download() for e in engines])
        hists = [e.sums_history() for e in engines]
    finally:
        for e in engines:
            e.close()
    assert np.array_equal(got, reference(O, H, W, steps))
    tot = np.zeros(steps)
    for hst in hists:  # rank order, as src/Model.hpp:89-92
        assert hst.shape == (steps, 1)
        tot = tot + hst[:, 0]
    for s in range(1, steps + 1):
        want = math.fsum(reference(O, H, W, s).ravel())
        assert abs(tot[s - 1] - want) <= 1e-12 * abs(want), s


def test_rccl_path_single_rank(gpu, O, monkeypatch):
    # one RCCL rank whose neighbours are itself: the exchange and the border launches run,
    # the received rows land in ghost rows outside the grid, the result is unchanged
    H, W, steps = 64, 130, 5
    monkeypatch.setenv("MM_SELF_HALO", "1")
    e = gpu.Engine(H, W, halo_mode=gpu.MM_HALO_RCCL, comm_id_bytes=gpu.comm_id())
    monkeypatch.delenv("MM_SELF_HALO")
    try:
        e.upload(O.fill_random(H, W))
        e.rate_field_upload(random_field(H, W))
        e.add_diffuse_field(0)
        e.run(steps, reduce_every=1)
        got = e.download()
        hist = e.sums_history()
    finally:
        e.close()
    assert np.array_equal(got, reference(O, H, W, steps))
    want = math.fsum(reference(O, H, W, steps).ravel())
    assert abs(hist[-1, 0] - want) <= 1e-12 * abs(want)


def test_graph_replay_and_prepare(gpu, O, monkeypatch):
    H, W, steps = 64, 130, 64
    with field_engine(gpu, O, H, W) as e:
        e.run(steps)
        graphed = e.download()
        assert e.info()["graph_state"] == 1
    monkeypatch.setenv("MM_GRAPH", "0")
    e = field_engine(gpu, O, H, W)
    monkeypatch.delenv("MM_GRAPH")
    with e:
        e.run(steps)
        eager = e.download()
        assert e.info()["graph_state"] == 0
    with field_engine(gpu, O, H, W) as e:
        e.prepare(steps)
        assert np.array_equal(e.download(), O.fill_random(H, W))  # prepare ran no step
        e.run(steps)
        prepared = e.download()
        assert e.info()["graph_state"] == 1
    assert np.array_equal(graphed, eager)
    assert np.array_equal(prepared, eager)
    assert np.array_equal(eager, reference(O, H, W, steps))


def test_reuploaded_field_takes_effect(gpu, O):
    # the graphs hold the field's address, not its values
    H, W, steps = 64, 130, 16
    f2, cnt = random_field(H, W, seed=99), neighbour_counts(H, W)
    with field_engine(gpu, O, H, W) as e:
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


def test_field_memory_is_reported(gpu):
    H, W = 9, 129
    with gpu.Engine(H, W, n_attr=2) as e:
        before = e.info()
        e.rate_field_fill(0.25, attr=1)
        after = e.info()
        e.rate_field_fill(0.5, attr=1)  # the same buffer
        assert e.info()["bytes_device"] == after["bytes_device"]
    assert after["bytes_device"] - before["bytes_device"] == (H + 40) * before["pitch"] * 8


def test_refusals(gpu):
    H, W = 8, 130
    with gpu.Engine(H, W, n_attr=2) as e:
        e.fill(0, value=1.0)
        e.add_diffuse_field(0)
        with pytest.raises(gpu.MMError):
            e.run(1)  # no field yet
        with pytest.raises(gpu.MMError):
            e.prepare(4)
        with pytest.raises(gpu.MMError):
            e.rate_field_upload(np.zeros((2, W)), row0=H + 19)  # past the ghost zone
        with pytest.raises(gpu.MMError):
            e.rate_field_upload(np.zeros((1, W)), row0=-21)
        bad = np.zeros((H, W))
        bad[3, 129] = float("nan")
        with pytest.raises(gpu.MMError):
            e.rate_field_upload(bad)
        with pytest.raises(gpu.MMError):
            e.rate_field_upload(np.zeros((H, W)), attr=2)  # attr = n_attr
        with pytest.raises(gpu.MMError):
            e.rate_field_fill(0.1, attr=2)
        with pytest.raises(gpu.MMError):
            e.run(1)  # the refused uploads made no field
        e.rate_field_upload(np.zeros((H + 40, W)), row0=-20)  # the whole ghost zone is fine
        e.run(1)
        assert np.array_equal(e.download(), np.ones((H, W)))
