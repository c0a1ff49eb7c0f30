"""K fused steps of the closed rate-field diffusion per pass on the GPU (mm_closedk_kernel,
MM_CLOSED_STEPS). Every fused level is mm_closed_kernel's arithmetic, so K fused steps are
tests/closed_model.py's closed_step applied K times, bit for bit: expected states come from
closed_model.closed_steps and are compared as bits (value_classes.assert_same_bits), sums()
and the history within 1e-12 * |want| as tests/test_gpu_closed.py does. The kernel is asked
for with MM_CLOSED_STEPS=K around engine creation; without the knob every closed program
stays at one step per pass (tests/test_gpu_closed.py). No grid is larger than 130 x 257 except
in the two tests of section 9.
"""
import math

import numpy as np
import pytest

import closed_model as cm
import engine_model as M
import test_gpu_closed as closed
import value_classes as vc
from closedk_geom import geom
from test_gpu_closed import C, ClosedModel, assert_history, assert_sums, dilate_open, program, values
from test_gpu_lifetime import make_engine, mismatch, plan_facts

pytestmark = pytest.mark.gpu

CLOSEDK = 5  # mm_info.kernel of mm_closedk_kernel
GEOM = geom()
KS = list(range(2, GEOM["kClosedMaxSteps"] + 1))  # the shipped K
KMAX = KS[-1]
KNOBS = closed.KNOBS + ("MM_CLOSED_STEPS", "MM_SEG_EDGE")
SHAPES = [(1, 1), (1, 9), (2, 2), (3, 3), (13, 6), (27, 257), (130, 97)]
DOMAINS = closed.DOMAINS + ["kseams"]
SEG = {"MM_SEG_WAVES": 64}  # the shortest segments the planner makes: 16 rows


def out_cols(K):
    return GEOM["closedk_out_cols"](K)


def balanced(n, K):
    """ceil(n / K) passes of balanced length (mm_plan.cpp next_pass_len)."""
    lens = []
    while n > 0:
        lens.append(-(-n // -(-n // K)))
        n -= lens[-1]
    return lens


def engine(gpu, monkeypatch, H, W, K=None, n_attr=1, **env):
    """An engine created with MM_CLOSED_STEPS=K (None: unset) and `env`, every other knob of
    the planner cleared."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if K is not None:
        env = dict(env, MM_CLOSED_STEPS=K)
    return make_engine(gpu, monkeypatch, (n_attr, env, (H, W)))


def closed_engine(gpu, monkeypatch, v, f, K, **env):
    e = engine(gpu, monkeypatch, *v.shape, K, **env)
    e.upload(v)
    e.rate_field_upload(f)
    e.add_diffuse_closed(0)
    return e


def check_plan(e, W, K):
    info = e.info()
    assert (info["n_passes"], info["kernel"], info["steps_per_launch"]) == (1, CLOSEDK, K), info
    assert e.pass_plan(7) == balanced(7, K) and e.pass_plan(K + 1) == balanced(K + 1, K)
    for k in range(2, K + 1):
        assert e.pass_kernel(k) == (CLOSEDK, 2, -(-W // out_cols(k))), (k, e.pass_kernel(k))
    assert e.pass_kernel(1)[0] == 0


def one_step(e):
    info = e.info()
    return (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1)


def domain(kind, H, W, K):
    """closed_model's six domains, and `kseams`: one-cell wall lines with gaps on the seams of
    the K-step strips, columns o-1, o, 2o-1, 2o for o = closedk_out_cols(K)."""
    if kind != "kseams":
        return cm.domain(kind, H, W)
    o = out_cols(K)
    m = np.ones((H, W), dtype=bool)
    for c in (o - 1, o, 2 * o - 1, 2 * o):
        if c < W:
            m[:, c] = False
            m[(c % 5)::6, c] = True  # gaps
    return m


_REF = {}


def reference(key, v, f, steps):
    """closed_step applied `steps` times, every state kept; computed once per key."""
    states = _REF.setdefault(key, [np.array(v, dtype=np.float64)])
    while len(states) <= steps:
        states.append(cm.closed_step(states[-1], f))
    for s in states:
        s.setflags(write=False)
    return states


def test_every_shipped_k_is_tested(gpu):
    assert KS == list(range(2, gpu.CLOSED_MAX_STEPS + 1)) and KS
    for K in KS:
        assert out_cols(K) % 2 == 0 and 128 - out_cols(K) >= 2 * (K + 1)
    assert 2 * out_cols(2) < 257 and 27 * 257 > 0  # 27 x 257: three strips at every K


# ---- 1. shapes x domains: K, K + 1 and 7 steps, eager and as the run plans it -------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", DOMAINS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_domains(gpu, monkeypatch, H, W, kind, K):
    mask = domain(kind, H, W, K)
    f = cm.rates(mask)
    v = values(H, W)
    key = ("dom", H, W, kind, K if kind == "kseams" else 0)
    states = reference(key, v, f, 7)
    final = {}
    for steps in (K, K + 1, 7):
        # eager, the sums after every step
        with closed_engine(gpu, monkeypatch, v, f, K, MM_GRAPH=0) as e:
            check_plan(e, W, K)
            e.run(steps, reduce_every=1)
            got = e.download()
            vc.assert_same_bits(got, states[steps], (H, W, kind, K, "eager", steps))
            assert_sums(e.sums()[0], states[steps], (H, W, kind, K, "sums", steps))
            assert e.info()["graph_state"] == 0
            assert_history(e.sums_history(), states, range(1, steps + 1), (H, W, kind, K, "eager"))
        # graphs allowed, the sums after steps 3 and 6
        with closed_engine(gpu, monkeypatch, v, f, K) as e:
            e.run(steps, reduce_every=3)
            got = e.download()
            vc.assert_same_bits(got, states[steps], (H, W, kind, K, "graph", steps))
            if steps >= 3:
                assert_history(e.sums_history(), states, range(3, steps + 1, 3), (H, W, kind, K, "graph"))
            # walls: exactly the bits that were uploaded
            assert np.array_equal(got[~mask].view(np.uint64), v[~mask].view(np.uint64))
        final[steps] = got
    if kind == "one":
        assert final[7].tobytes() == v.tobytes()  # cnt = 0: the cell stays put
    # the same runs at one step per pass: the same bytes
    with closed_engine(gpu, monkeypatch, v, f, 1) as e:
        assert one_step(e) and e.pass_plan(7) == [1] * 7
        for steps, n in ((K, K), (K + 1, 1), (7, 7 - K - 1)):
            if n:
                e.run(n)
            assert e.download().tobytes() == final[steps].tobytes(), (H, W, kind, K, steps)
    if kind == "open":
        # f != 0 everywhere: MM_FLOW_DIFFUSE_FIELD under MM_FIELD_STEPS=K, the same bytes
        with engine(gpu, monkeypatch, H, W, None, MM_FIELD_STEPS=K) as e:
            e.upload(v)
            e.rate_field_upload(f)
            e.add_diffuse_field(0)
            assert e.info()["kernel"] == 4 and e.info()["steps_per_launch"] == K
            e.run(7)
            assert e.download().tobytes() == final[7].tobytes()


# ---- 2. replayed graphs, prepare -----------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_graph_replay_and_prepare(gpu, monkeypatch, K):
    H, W, steps = 27, 257, 24
    mask = domain("kseams", H, W, K) & cm.domain("random", H, W, seed=5)
    f, v = cm.rates(mask), values(H, W, seed=8)
    states = reference(("replay", K), v, f, 2 * steps)
    with closed_engine(gpu, monkeypatch, v, f, K) as e:
        check_plan(e, W, K)
        e.prepare(steps, 3)
        assert e.download().tobytes() == v.tobytes()  # prepare ran no step
        e.run(steps, reduce_every=3)
        vc.assert_same_bits(e.download(), states[steps], (K, "first"))
        e.run(steps, reduce_every=3)
        vc.assert_same_bits(e.download(), states[2 * steps], (K, "second"))
        info = e.info()
        assert info["graph_state"] == 1 and info["graph_launches"] >= 2, info
        assert_history(e.sums_history(), states, range(3, 2 * steps + 1, 3), (K, "replay"))


# ---- 3. segment seams ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_segment_seams(gpu, monkeypatch, K):
    """16-row segments: wall lines with gaps on the rows either side of every segment seam and
    on the strip seams; every level is recomputed across both."""
    H, W = 50, 257
    with engine(gpu, monkeypatch, H, W, K, **SEG) as e:
        e.rate_field_fill(0.0)
        e.add_diffuse_closed(0)
        th = e.info()["rows_per_wave"]
    assert 16 <= th and 3 * th <= H
    mask = domain("kseams", H, W, K)
    for seam in range(th, H, th):
        for r in (seam - 1, seam):
            mask[r, :] = False
            mask[r, (r % 4)::9] = True
    f, v = cm.rates(mask), values(H, W, seed=3)
    states = reference(("segseam", K), v, f, 2 * K + 1)
    for graph in (0, 1):
        with closed_engine(gpu, monkeypatch, v, f, K, MM_GRAPH=graph, **SEG) as e:
            check_plan(e, W, K)
            assert e.info()["rows_per_wave"] == th
            assert e.info()["waves_per_pass"] == 3 * -(-H // th)
            e.run(K, reduce_every=1)
            vc.assert_same_bits(e.download(), states[K], (K, graph, "one pass"))
            e.run(K + 1, reduce_every=1)
            vc.assert_same_bits(e.download(), states[2 * K + 1], (K, graph, "three passes"))
            assert_history(e.sums_history(), states, range(1, 2 * K + 2), (K, graph))


# ---- 4. value classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cls", vc.CLASSES)
def test_value_classes(gpu, monkeypatch, cls, K):
    H, W = 27, 257
    mask = cm.domain("random", H, W)
    rng = np.random.default_rng(11)
    f = np.where(mask, vc.RATES[cls] * rng.uniform(0.5, 1.0, (H, W)), 0.0)
    cnt = cm.open_counts(f)
    near_open = (cnt > 0) & ~mask          # walls beside open cells
    near_wall = mask & (cnt < 8) & (cnt > 0)  # open cells beside walls (or the grid's edge)
    walls, opens = np.argwhere(near_open), np.argwhere(near_wall)
    pick_w = [tuple(walls[i]) for i in np.linspace(0, len(walls) - 1, 9).astype(int)]
    pick_o = [tuple(opens[i]) for i in np.linspace(0, len(opens) - 1, 6).astype(int)]
    start = vc.make(cls, H, W, positions=pick_w + pick_o)
    for x, y in pick_w[::3] + pick_o[::3]:
        if cls != "nonfinite":
            start[x, y] = -0.0
    passes = 2
    states = reference(("vc", cls), start, f, passes * K)
    with closed_engine(gpu, monkeypatch, start, f, K) as e:
        check_plan(e, W, K)
        bad = ~np.isfinite(start) & mask
        for p in range(1, passes + 1):
            assert e.pass_plan(K) == [K]
            e.run(K, reduce_every=1)  # one K-step pass
            got = e.download()
            vc.assert_same_bits(got, states[p * K], (cls, K, p))
            assert np.array_equal(got[~mask].view(np.uint64), start[~mask].view(np.uint64)), (cls, K, p)
            if cls == "nonfinite":
                # without the model: the K-fold dilation of the open seeds through open cells;
                # the walls' seeds stay where they are
                for _ in range(K):
                    bad = dilate_open(bad, mask)
                assert bad.sum() > len(pick_o)
                assert np.array_equal(~np.isfinite(got), bad | (~np.isfinite(start) & ~mask)), (K, p)
        hist = e.sums_history()
    assert hist.shape == (passes * K, 1)
    for s in range(1, passes * K + 1):
        if np.all(np.isfinite(states[s])):
            vc.assert_sum_close(hist[s - 1, 0], states[s], (cls, K, s))
        else:
            assert not np.isfinite(hist[s - 1, 0])


# ---- 5. NaN in the pitch padding of the state and of the field -----------------------------------
@pytest.mark.parametrize("K", KS)
def test_nan_padding(gpu, monkeypatch, K):
    H, W = 27, 257
    mask = cm.domain("random", H, W, seed=1)
    f, v = cm.rates(mask), values(H, W, seed=5)
    states = reference(("pad",), v, f, 7)
    for graph in (0, 1):
        with closed_engine(gpu, monkeypatch, v, f, K, MM_GRAPH=graph) as e:
            check_plan(e, W, K)
            e.fill_padding(float("nan"))  # of the state and of the field, ghost rows included
            e.run(7, reduce_every=1)
            vc.assert_same_bits(e.download(), states[7], ("padding", K, graph))
            hist = e.sums_history()
            assert np.all(np.isfinite(hist))
            assert_history(hist, states, range(1, 8), ("padding", K, graph))


# ---- 6. the non-temporal instances ---------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_instances(gpu, monkeypatch, K):
    """Plain and non-temporal stores (MM_KERNEL_VARIANT), each with the step sums and without."""
    H, W = 27, 257
    mask = domain("kseams", H, W, K) & cm.domain("disc", H, W)
    f, v = cm.rates(mask), values(H, W, seed=9)
    states = reference(("inst", K), v, f, K + 1)
    for variant in (0, 1):
        for reduce_every in (0, 1):
            with closed_engine(gpu, monkeypatch, v, f, K, MM_KERNEL_VARIANT=variant) as e:
                check_plan(e, W, K)
                assert e.pass_kernel(K) == (CLOSEDK, 2, 3) and e.pass_plan(K) == [K]
                e.run(K, reduce_every)
                vc.assert_same_bits(e.download(), states[K], (K, variant, reduce_every))
                e.run(1, reduce_every)
                vc.assert_same_bits(e.download(), states[K + 1], (K, variant, reduce_every, "+1"))
                hist = e.sums_history()
            if reduce_every:
                assert_history(hist, states, range(1, K + 2), (K, variant))
            else:
                assert hist.shape[0] == 0


# ---- 7. an odd number of flips replayed ----------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_odd_flip_graph_replays(gpu, monkeypatch, K):
    """run(3K) is three passes: one graph with an odd number of buffer flips, so its three
    replays start from alternating buffer parities; run(K) after them is an eager pass. The
    state after every call against the model and against an engine that never captures, with
    another field (other walls) uploaded between the second and the third replay."""
    H, W = 64, 130
    calls = [3 * K, 3 * K, 3 * K, K, K]
    f1 = cm.rates(domain("kseams", H, W, K) & cm.domain("random", H, W))
    f2 = cm.rates(cm.domain("disc", H, W), seed=9)
    want, v = [], values(H, W, seed=12)
    v0 = v
    for i, n in enumerate(calls):
        v = cm.closed_steps(v, f2 if i >= 2 else f1, n)
        want.append(v)
    got = {}
    for graphs in (1, 0):
        env = {} if graphs else {"MM_GRAPH": 0}
        with closed_engine(gpu, monkeypatch, v0, f1, K, **env) as e:
            check_plan(e, W, K)
            assert e.pass_plan(3 * K) == [K] * 3 and e.pass_plan(K) == [K]
            done = 0
            for i, n in enumerate(calls):
                if i == 2:
                    e.rate_field_upload(f2)  # the graphs hold the field's address, not its values
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
        vc.assert_same_bits(got[1, i], want[i], (K, i))
        assert got[1, i].tobytes() == got[0, i].tobytes(), (K, i)


# ---- 8. lifetime, and where the kernel must not run ----------------------------------------------
def lifetime_script(H, W, K):
    f1 = cm.rates(cm.domain("disc", H, W))
    f2 = cm.rates(cm.domain("random", H, W, seed=9), seed=9)  # the walls moved
    s = [("fill_random", (0, M.SEED)), ("rate_field_upload", (f1, 0, 0))]
    s += program([C(0)]) + [("run", (2 * K, 0)), ("run", (3 * K, 0)), ("run", (7, 3))]
    s += [("rate_field_upload", (f2, 0, 0)), ("run", (K + 1, 1)), ("run", (16, 0))]
    s += program([M.D(0, 0.1)]) + [("run", (16, 0)), ("run", (8, 1))]
    s += program([C(0)]) + [("run", (7, 1)), ("run", (3 * K, 0))]
    # add_diffuse_closed arrives after a run: [DIFFUSE, CLOSED] is two passes of one step
    s += program([M.D(0, 0.1)]) + [("run", (4, 0)), ("add_diffuse_closed", (0,)), ("run", (5, 1))]
    s += program([C(0)]) + [("run", (2 * K, 2)), ("run", (2 * K, 2))]
    return s


@pytest.mark.parametrize("mode", ["checked", "free"])
@pytest.mark.parametrize("K", KS)
def test_lifetime(gpu, O, monkeypatch, K, mode):
    H, W = 50, 257
    cfg = (1, {"MM_CLOSED_STEPS": K, **SEG}, (H, W))
    script = lifetime_script(H, W, K)
    m = ClosedModel(O, H, W)
    program_ops = M.PROGRAM_OPS | {"add_diffuse_closed"}

    def same_plans(i, e):
        with make_engine(gpu, monkeypatch, cfg) as fresh:
            fresh.rate_field_fill(0.0, 0)
            for method, args in program(m.flows)[1:]:
                M.apply_op(fresh, method, args)
            want = plan_facts(fresh, True)
        got = plan_facts(e, True)
        assert got == want, (i, script[i][0], got, want)
        if m.flows == [C(0)]:
            assert got["info"]["kernel"] == CLOSEDK and got["info"]["steps_per_launch"] == K
            assert got["plans"][7] == balanced(7, K) and got["kernels"][K][0] == CLOSEDK
        elif any(fl[0] == closed.CLOSED for fl in m.flows):
            assert got["info"]["kernel"] == 0 and got["info"]["steps_per_launch"] == 1
            assert got["info"]["n_passes"] == len(m.flows)

    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    seen = set()
    with make_engine(gpu, monkeypatch, cfg) as e:
        for i, (method, args) in enumerate(script):
            M.apply_op(m, method, args)
            M.apply_op(e, method, args)
            if mode != "checked":
                continue
            if method in M.STATE_OPS or method == "add_diffuse_closed":
                bad = mismatch(e, m)
                assert bad is None, (i, method, bad)
            if method in program_ops and script[i + 1][0] not in program_ops:
                same_plans(i, e)
                seen.add(e.info()["kernel"])
        e.synchronize()
        bad = mismatch(e, m)
        assert bad is None, bad
        info = e.info()
        assert (info["steps_done"], info["hist_entries"]) == (m.steps_done, len(m.hist))
        same_plans(len(script) - 1, e)
        assert info["kernel"] == CLOSEDK
    if mode == "checked":
        assert seen >= {0, CLOSEDK}


@pytest.mark.parametrize("K", KS)
def test_where_it_must_not_run(gpu, monkeypatch, K):
    H, W, steps = 27, 257, 5
    mask = closed.seam_domain(H, W, 2)
    f, v = cm.rates(mask), values(H, W, seed=6)
    want = reference(("not", ), v, f, steps)[steps]
    # a second attribute on the engine: copied through by the one-step kernel
    other = values(H, W, seed=7)
    with engine(gpu, monkeypatch, H, W, K, n_attr=2) as e:
        e.upload(other, 0)
        e.upload(v, 1)
        e.rate_field_upload(f, attr=1)
        e.add_diffuse_closed(1)
        assert one_step(e) and e.pass_plan(7) == [1] * 7 and e.pass_kernel(K)[0] == 0
        e.run(steps, reduce_every=1)
        vc.assert_same_bits(e.download(1), want, (K, "two attributes"))
        assert e.download(0).tobytes() == other.tobytes()
    # other flows beside it, MM_PASSK=0, the knob at 1 or unset
    with closed_engine(gpu, monkeypatch, v, f, K) as e:
        e.add_diffuse(0, 0.1)
        assert one_step(e) and e.info()["n_passes"] == 2
    for K1, env in ((K, {"MM_PASSK": 0}), (1, {}), (0, {}), (None, {}),
                    (None, {"MM_FIELD_STEPS": K, "MM_FIELD_HALO": K})):
        with closed_engine(gpu, monkeypatch, v, f, K1, **env) as e:
            assert one_step(e) and e.pass_plan(7) == [1] * 7 and e.pass_kernel(K)[0] == 0, (K1, env)
            e.run(steps)
            vc.assert_same_bits(e.download(), want, (K, K1, env))
    # a knob above the maximum clamps
    with closed_engine(gpu, monkeypatch, v, f, 99) as e:
        check_plan(e, W, KMAX)
    # a host chain of two slabs, two ghost rows of the field promised and uploaded
    engines = closed.chain(gpu, monkeypatch, H, W, 2, MM_FIELD_HALO=2, MM_CLOSED_STEPS=K)
    try:
        for e in engines:
            e.upload(v[e.x_init:e.x_init + e.h])
            closed.upload_field(e, f, 2)
            e.add_diffuse_closed(0)
            assert one_step(e) and e.pass_kernel(K)[0] == 0
        assert closed.run_chain(engines, steps, reduce_every=1) == 1
        got = np.vstack([e.download() for e in engines])
    finally:
        for e in engines:
            e.close()
    vc.assert_same_bits(got, want, (K, "chain"))
    # one slab with a halo mode
    monkeypatch.setenv("MM_FIELD_HALO", "2")
    monkeypatch.setenv("MM_CLOSED_STEPS", str(K))
    try:
        e = gpu.Engine(H, W, halo_mode=gpu.MM_HALO_HOST)
    finally:
        monkeypatch.delenv("MM_FIELD_HALO")
        monkeypatch.delenv("MM_CLOSED_STEPS")
    with e:
        e.upload(v)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        assert one_step(e)
        e.run(steps)
        vc.assert_same_bits(e.download(), want, (K, "halo mode"))


def test_timing_bytes(gpu, monkeypatch):
    """A launch moves 24 B per cell whatever K is."""
    H, W, K = 27, 257, KMAX
    f, v = cm.rates(cm.domain("disc", H, W)), values(H, W, seed=40)
    with closed_engine(gpu, monkeypatch, v, f, K) as e:
        e.set_timing(True)
        e.run(2 * K + 1)
        n, ms, nbytes = e.timing()
        assert n == 3 and ms > 0.0
        assert nbytes == 24.0 * H * W  # per launch
        e.set_timing(False)
        vc.assert_same_bits(e.download(), cm.closed_steps(v, f, 2 * K + 1), "timed")


def test_refusals(gpu, monkeypatch):
    H, W = 8, 130
    with engine(gpu, monkeypatch, H, W, KMAX) as e:
        e.fill(0, value=1.0)
        e.add_diffuse_closed(0)
        assert e.info()["kernel"] == CLOSEDK
        with pytest.raises(gpu.MMError):
            e.run(KMAX)  # no field yet
        with pytest.raises(gpu.MMError):
            e.prepare(2 * KMAX)
        e.rate_field_fill(0.0)  # all walls
        e.run(KMAX)
        assert np.array_equal(e.download(), np.ones((H, W)))


# ---- 9. size: the occupancy-sized plan, and a segment at the 2^31 offset cap ---------------------
def test_whole_grid_2048(gpu, monkeypatch):
    """The whole 2048 x 2048 grid, a disc, under the segment plan sized by the instance's
    occupancy: 7 steps (4 + 3 at K = 4), every cell as bits."""
    H = W = 2048
    K, steps = KMAX, 7
    mask = cm.domain("disc", H, W)
    f = cm.rates(mask)
    v = values(H, W, seed=2)
    with closed_engine(gpu, monkeypatch, v, f, K) as e:
        check_plan(e, W, K)
        info = e.info()
        assert 16 <= info["rows_per_wave"] < H and info["seg_waves_per_cu"] >= 8, info
        e.run(steps, reduce_every=steps)
        got = e.download()
        hist = e.sums_history()
    want = cm.closed_steps(v, f, steps)
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), bad[-1].tolist())
    assert np.array_equal(got[~mask].view(np.uint64), v[~mask].view(np.uint64))
    assert hist.shape == (1, 1)
    w = math.fsum(memoryview(want.ravel()))
    assert abs(hist[0, 0] - w) <= 1e-12 * abs(w)


def cap_rates(row0, n):
    """Rows [row0, row0 + n) of the cap grid's rate field: test_gpu_field_large's outer product
    of exact sixteenths with its zero rows and columns opened (0.5), and an eighth of the cells,
    picked by a hash of (row, column), walls of either sign."""
    import test_gpu_field_large as fl
    f = fl.cap_field_rows(row0, n)
    f[f == 0.0] = 0.5
    i = np.arange(row0, row0 + n, dtype=np.uint64)[:, None]
    j = np.arange(fl.CAP_W, dtype=np.uint64)[None, :]
    h = (i * np.uint64(2654435761) + j * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    pick = (h >> np.uint64(13)) & np.uint64(15)
    f[pick == 0] = 0.0
    f[pick == 1] = -0.0
    return f


def test_segment_at_the_offset_cap(gpu, O, monkeypatch):
    """8200 x 32768 with MM_SEG_WAVES=0.001: one segment of exactly closedk_max_rows rows per
    strip and a rest. One pass of the largest K, sums off and on: three bands of rows
    (tests/test_gpu_field_large.py cap_bands), every column, bit for bit against closed_steps on
    the band widened by K + 1 rows a side (tests/test_closedk_cpu.py: that is the cone)."""
    import test_gpu_field_large as fl
    K = KMAX
    H, W = fl.CAP_H, fl.CAP_W
    with engine(gpu, monkeypatch, H, W, K, MM_SEG_WAVES=0.001) as e:
        e.add_diffuse_closed(0)
        info = e.info()
        assert info["pitch"] == W
        rpw = GEOM["closedk_max_rows"](K, info["pitch"]) & ~1
        assert (info["kernel"], info["steps_per_launch"], info["rows_per_wave"]) == (CLOSEDK, K, rpw), info
        # the deepest row a wave addresses stays below 2^31, and four more rows would not
        ring = GEOM["closed_ring"](K)
        assert (rpw + 3 * K + 2 * ring + 1) * W * 8 < 1 << 31
        assert (rpw + 3 * K + 2 * ring + 13) * W * 8 >= 1 << 31
        for row0 in range(0, H, 1024):  # the host holds one chunk at a time
            e.rate_field_upload(cap_rates(row0, min(1024, H - row0)), row0=row0)
        bands = fl.cap_bands(rpw, K)
        assert bands[2][0] + bands[2][1] == H and 16 <= H - rpw <= 92
        want = []
        for b, n in bands:
            lo, hi = max(0, b - K - 1), min(H, b + n + K + 1)
            w = cm.closed_steps(O.fill_random(H, W, lo, hi - lo), cap_rates(lo, hi - lo), K)
            want.append(w[b - lo:b - lo + n])
        for reduce_every in (0, 1):
            e.fill_random(0)
            s0 = e.sums()[0]
            assert e.pass_plan(K) == [K]
            e.clear_history()
            e.run(K, reduce_every)
            s1 = e.sums()[0]
            for (b, n), w in zip(bands, want):
                g = e.read_rows(b, n)
                rows = np.flatnonzero(np.any(g.view(np.uint64) != w.view(np.uint64), axis=1)) + b
                assert rows.size == 0, (K, reduce_every, "rows", rows[:8].tolist(), "seam", rpw)
            # rates in (0, 1] on positive values: every level's total is the conserved one
            assert abs(s1 - s0) <= 1e-12 * s0, (reduce_every, s0, s1)
            hist = e.sums_history()
            if reduce_every:
                assert hist.shape == (K, 1), hist.shape
                for s in range(K):
                    assert abs(hist[s, 0] - s0) <= 1e-12 * s0, (s, hist[s, 0], s0)
