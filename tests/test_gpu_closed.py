"""Closed rate-field diffusion on the GPU (MM_FLOW_DIFFUSE_CLOSED, mm_closed_kernel): cells of
rate zero are walls. The contract is tests/closed_model.py's closed_step (checked against the
oracle in tests/test_closed_cpu.py), bit for bit: every cell is compared as bits, sums() and
the history within 1e-12 * |want| as tests/test_gpu_lifetime.py does. No grid is larger than
130 x 257.

The field's pitch padding is poisoned together with the state's: mm_debug_fill_padding writes
the padding of every allocated rate field too (ghost rows included), so test_nan_padding
reaches both.
"""
import math

import numpy as np
import pytest

import closed_model as cm
import engine_model as M
import value_classes as vc
from test_gpu_lifetime import PLAN_STEPS, make_engine, mismatch, plan_facts
from test_gpu_ratefield import make_chain, run_chain

pytestmark = pytest.mark.gpu

CLOSED = 4
SHAPES = [(1, 1), (1, 9), (2, 2), (3, 3), (13, 6), (27, 257), (130, 97)]
DOMAINS = ["open", "checker", "one", "random", "disc", "seams"]
KNOBS = ("MM_FIELD_STEPS", "MM_FIELD_HALO", "MM_SEG_WAVES", "MM_KERNEL_VARIANT", "MM_WIDE",
         "MM_STEPS_PER_PASS", "MM_PASSK", "MM_GRAPH", "MM_SELF_HALO", "MM_ROWS_PER_WAVE")
# the embedded rectangles of tests/test_closed_cpu.py: (rows, columns) at (row, column)
BLOCKS = [((9, 11), (0, 0)), ((1, 5), (8, 120)), ((2, 2), (3, 250))]


def values(H, W, seed=0):
    return np.random.default_rng(seed + 1000003 * H + W).uniform(0.5, 2.0, (H, W))


def engine(gpu, monkeypatch, H, W, n_attr=1, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return make_engine(gpu, monkeypatch, (n_attr, env, (H, W)))


_REF = {}


def reference(key, v, f, steps):
    """closed_step applied `steps` times, every state kept; computed once per key."""
    states = _REF.setdefault(key, [np.array(v, dtype=np.float64)])
    while len(states) <= steps:
        states.append(cm.closed_step(states[-1], f))
    for s in states:
        s.setflags(write=False)
    return states


def assert_sums(got, want_cells, what):
    want = math.fsum(np.asarray(want_cells).ravel())
    assert abs(got - want) <= 1e-12 * abs(want), (what, got, want)


def assert_history(hist, states, steps, what):
    """hist[i] is the sum after step steps[i], over all owned cells, walls included."""
    assert hist.shape == (len(steps), 1), (what, hist.shape)
    for i, s in enumerate(steps):
        assert_sums(hist[i, 0], states[s], (what, s))


# ---- shapes x domains: 1, 2 and 7 steps, eager and replayed, reduce_every 1 and 3 ---------------
@pytest.mark.parametrize("kind", DOMAINS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_domains(gpu, monkeypatch, H, W, kind):
    mask = cm.domain(kind, H, W)
    f = cm.rates(mask)
    v = values(H, W)
    states = reference(("dom", H, W, kind), v, f, 7)
    # eager: 1 step, 1 more, 5 more, the sums after every step
    with engine(gpu, monkeypatch, H, W, MM_GRAPH=0) as e:
        e.upload(v)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        info = e.info()
        assert (info["n_passes"], info["kernel"], info["steps_per_launch"], info["halo_depth"]) == \
            (1, 0, 1, 1), info
        assert e.pass_plan(7) == [1] * 7 and e.pass_kernel(1)[0] == 0
        done = 0
        for n in (1, 1, 5):
            e.run(n, reduce_every=1)
            done += n
            vc.assert_same_bits(e.download(), states[done], (H, W, kind, "eager", done))
            assert_sums(e.sums()[0], states[done], (H, W, kind, "sums", done))
        assert e.info()["graph_state"] == 0
        assert_history(e.sums_history(), states, range(1, 8), (H, W, kind, "eager"))
    # replayed: 7 steps as one graph, the sums after steps 3 and 6
    with engine(gpu, monkeypatch, H, W) as e:
        e.upload(v)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        e.run(7, reduce_every=3)
        vc.assert_same_bits(e.download(), states[7], (H, W, kind, "graph"))
        info = e.info()
        assert info["graph_state"] == 1 and info["graph_launches"] >= 1, info
        assert_history(e.sums_history(), states, (3, 6), (H, W, kind, "graph"))
        # walls: exactly the bits that were uploaded
        assert np.array_equal(e.download()[~mask].view(np.uint64), v[~mask].view(np.uint64))
        if kind == "open":
            # f != 0 everywhere: MM_FLOW_DIFFUSE_FIELD on the same engine, bit for bit
            e.clear_flows()
            e.add_diffuse_field(0)
            e.upload(v)
            e.run(7)
            assert e.download().tobytes() == states[7].tobytes()
        if kind == "one":
            assert states[7].tobytes() == v.tobytes()  # cnt = 0: the cell stays put


@pytest.mark.parametrize("block,off", BLOCKS)
def test_embedded_rectangle_against_the_oracle(gpu, O, monkeypatch, block, off):
    """A block of non-zero rates in a zero field, compared with the oracle's general step run
    on the block as a grid of its own."""
    H, W = 27, 257
    (p, q), (x0, y0) = block, off
    fb = cm.rates(np.ones((p, q), dtype=bool), seed=1)
    f = np.zeros((H, W))
    f[x0:x0 + p, y0:y0 + q] = fb
    v = values(H, W, seed=2)
    w = v[x0:x0 + p, y0:y0 + q].copy()
    cnt = np.array([[O.neighbor_count(p, q, x, y) for y in range(q)] for x in range(p)])
    for _ in range(6):
        w = O.field_step_general(w, np.where(cnt > 0, fb * w, 0.0))
    want = v.copy()
    want[x0:x0 + p, y0:y0 + q] = w
    with engine(gpu, monkeypatch, H, W) as e:
        e.upload(v)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        e.run(6)
        vc.assert_same_bits(e.download(), want, (block, off))
        assert e.download().tobytes() == want.tobytes()


# ---- value classes ----------------------------------------------------------------------------
def dilate_open(cells, mask):
    """Cells within one king's move of `cells`, among the open ones."""
    H, W = mask.shape
    p = np.zeros((H + 2, W + 2), dtype=bool)
    p[1:-1, 1:-1] = cells
    out = np.zeros((H, W), dtype=bool)
    for dx in range(3):
        for dy in range(3):
            out |= p[dx:dx + H, dy:dy + W]
    return out & mask


@pytest.mark.parametrize("cls", vc.CLASSES)
def test_value_classes(gpu, monkeypatch, cls):
    H, W = 27, 257
    mask = cm.domain("random", H, W)
    rng = np.random.default_rng(11)
    f = np.where(mask, vc.RATES[cls] * rng.uniform(0.5, 1.0, (H, W)), 0.0)
    cnt = cm.open_counts(f)
    near_open = (cnt > 0) & ~mask          # walls beside open cells
    near_wall = mask & (cnt < 8) & (cnt > 0)  # open cells beside walls (or the grid's edge)
    walls, opens = np.argwhere(near_open), np.argwhere(near_wall)
    # on the strip seams, the block seams and inside, a few of each
    pick_w = [tuple(walls[i]) for i in np.linspace(0, len(walls) - 1, 9).astype(int)]
    pick_o = [tuple(opens[i]) for i in np.linspace(0, len(opens) - 1, 6).astype(int)]
    start = vc.make(cls, H, W, positions=pick_w + pick_o)
    for x, y in pick_w[::3] + pick_o[::3]:
        if cls != "nonfinite":
            start[x, y] = -0.0
    steps = 3
    states = reference(("vc", cls), start, f, steps)
    with engine(gpu, monkeypatch, H, W) as e:
        e.upload(start)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        bad = ~np.isfinite(start) & mask
        for s in range(1, steps + 1):
            e.run(1, reduce_every=1)
            got = e.download()
            vc.assert_same_bits(got, states[s], (cls, s))
            assert np.array_equal(got[~mask].view(np.uint64), start[~mask].view(np.uint64)), (cls, s)
            if cls == "nonfinite":
                # without the model: the Chebyshev ball of radius s around the open seeds, cut
                # to what is reachable through open cells; the walls' seeds stay where they are
                bad = dilate_open(bad, mask)
                assert bad.sum() > len(pick_o)
                assert np.array_equal(~np.isfinite(got), bad | (~np.isfinite(start) & ~mask)), s
        hist = e.sums_history()
    assert hist.shape == (steps, 1)
    for s in range(1, steps + 1):
        if np.all(np.isfinite(states[s])):
            vc.assert_sum_close(hist[s - 1, 0], states[s], (cls, s))
        else:
            assert not np.isfinite(hist[s - 1, 0])


def test_nan_padding(gpu, monkeypatch):
    H, W = 27, 257
    mask = cm.domain("random", H, W, seed=1)
    f, v = cm.rates(mask), values(H, W, seed=5)
    states = reference(("pad",), v, f, 7)
    for graph in (0, 1):
        with engine(gpu, monkeypatch, H, W, MM_GRAPH=graph) as e:
            e.upload(v)
            e.rate_field_upload(f)
            e.fill_padding(float("nan"))  # of the state and of the field, ghost rows included
            e.add_diffuse_closed(0)
            e.run(7, reduce_every=1)
            vc.assert_same_bits(e.download(), states[7], ("padding", graph))
            hist = e.sums_history()
            assert np.all(np.isfinite(hist))
            assert_history(hist, states, range(1, 8), ("padding", graph))


# ---- several attributes -----------------------------------------------------------------------
def test_other_attributes_are_copied_through(gpu, monkeypatch):
    H, W = 27, 257
    mask = cm.domain("disc", H, W)
    f = cm.rates(mask)
    vs = [values(H, W, seed=10 + a) for a in range(3)]
    states = reference(("na3",), vs[1], f, 7)
    for graph in (0, 1):
        with engine(gpu, monkeypatch, H, W, n_attr=3, MM_GRAPH=graph) as e:
            for a in range(3):
                e.upload(vs[a], a)
            e.rate_field_upload(f, attr=1)
            e.add_diffuse_closed(1)
            assert e.info()["n_passes"] == 1
            done = 0
            for n in (1, 2, 4):  # odd and even buffer parities
                e.run(n, reduce_every=1)
                done += n
                assert e.download(0).tobytes() == vs[0].tobytes()
                assert e.download(2).tobytes() == vs[2].tobytes()
                vc.assert_same_bits(e.download(1), states[done], ("na3", graph, done))
            hist = e.sums_history()
            assert hist.shape == (7, 3)
            for s in range(7):
                for a, want in enumerate((vs[0], states[s + 1], vs[2])):
                    assert_sums(hist[s, a], want, ("na3", graph, s, a))


def test_closed_pass_between_other_passes(gpu, O, monkeypatch):
    H, W = 27, 257
    mask = cm.domain("random", H, W, seed=2)
    f = cm.rates(mask)
    want = [values(H, W, seed=20 + a) for a in range(3)]
    with engine(gpu, monkeypatch, H, W, n_attr=3) as e:
        for a in range(3):
            e.upload(want[a], a)
        e.rate_field_upload(f, attr=1)
        e.add_transfer(0, 1, 0.05)
        e.add_diffuse_closed(1)
        e.add_diffuse(2, 0.1)
        info = e.info()
        assert (info["n_passes"], info["kernel"], info["steps_per_launch"]) == (3, 0, 1), info
        for step in range(4):
            e.run(1, reduce_every=1)
            want = O.program_step(want, [(M.TRANSFER, 0, 1, 0.05)])
            want[1] = cm.closed_step(want[1], f)
            want = O.program_step(want, [(M.DIFFUSE, 2, 2, 0.1)])
            for a in range(3):
                vc.assert_same_bits(e.download(a), want[a], ("between", step, a))
        hist = e.sums_history()
        assert hist.shape == (4, 3)
        for a in range(3):
            assert_sums(hist[3, a], want[a], ("between", a))


def test_two_closed_diffusions_are_two_passes(gpu, monkeypatch):
    H, W = 13, 130
    masks = [cm.domain("disc", H, W), cm.domain("checker", H, W)]
    fs = [cm.rates(m, seed=i) for i, m in enumerate(masks)]
    vs = [values(H, W, seed=30 + a) for a in range(4)]
    with engine(gpu, monkeypatch, H, W, n_attr=4) as e:
        for a in range(4):
            e.upload(vs[a], a)
        e.rate_field_upload(fs[0], attr=0)
        e.rate_field_upload(fs[1], attr=3)
        e.add_diffuse_closed(0)
        e.add_diffuse_closed(3)
        assert e.info()["n_passes"] == 2
        e.run(5, reduce_every=5)
        vc.assert_same_bits(e.download(0), cm.closed_steps(vs[0], fs[0], 5), "attribute 0")
        vc.assert_same_bits(e.download(3), cm.closed_steps(vs[3], fs[1], 5), "attribute 3")
        assert e.download(1).tobytes() == vs[1].tobytes()
        assert e.download(2).tobytes() == vs[2].tobytes()
        hist = e.sums_history()
        assert hist.shape == (1, 4)
        assert_sums(hist[0, 0], cm.closed_steps(vs[0], fs[0], 5), "sum 0")
        assert_sums(hist[0, 2], vs[2], "sum 2")


# ---- chains, host transport -------------------------------------------------------------------
def chain(gpu, monkeypatch, H, W, G, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return make_chain(gpu, monkeypatch, H, W, G, env=env)


def upload_field(e, f, depth):
    """The slab's rows -depth .. h + depth of the global field f, clipped to the grid."""
    lo, hi = max(e.x_init - depth, 0), min(e.x_init + e.h + depth, f.shape[0])
    e.rate_field_upload(f[lo:hi], row0=lo - e.x_init)


def seam_domain(H, W, G):
    """The random domain with a one-cell-wide wall line, gaps in it, on the last row of every
    slab but the last and on the first row of every slab but the first."""
    mask = cm.domain("random", H, W, seed=3)
    for g in range(1, G):
        x = g * H // G
        for r in (x - 1, x):
            mask[r, :] = False
            mask[r, (r % 4)::9] = True
    return mask


def trace(e):
    info = e.info()
    return (e.download().tobytes(), info["steps_done"], info["hist_entries"],
            e.sums_history().shape, info["graph_count"])


@pytest.mark.parametrize("H,W,G", [(27, 257, 3), (8, 257, 2)])
def test_host_chain_bit_for_bit(gpu, monkeypatch, H, W, G):
    mask = seam_domain(H, W, G)
    f, v = cm.rates(mask), values(H, W, seed=6)
    steps = 5
    states = reference(("chain", H, W, G), v, f, steps)
    with engine(gpu, monkeypatch, H, W) as e:  # the single-engine result
        e.upload(v)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        e.run(steps)
        single = e.download()
    engines = chain(gpu, monkeypatch, H, W, G, MM_FIELD_HALO=2, MM_FIELD_STEPS=4)
    try:
        for e in engines:
            e.upload(v[e.x_init:e.x_init + e.h])
            upload_field(e, f, 2)
            e.add_diffuse_closed(0)
            info = e.info()
            assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1), info
        assert run_chain(engines, steps, reduce_every=1) == 1
        got = np.vstack([e.download() for e in engines])
        tot = sum(e.sums_history() for e in engines)  # rank order, as src/Model.hpp:89-92
    finally:
        for e in engines:
            e.close()
    assert got.tobytes() == single.tobytes()
    vc.assert_same_bits(got, states[steps], (H, W, G))
    assert_history(tot, states, range(1, steps + 1), ("chain", H, W, G))


def test_chain_refusals_leave_no_trace(gpu, monkeypatch):
    H, W, G = 27, 257, 3
    mask = seam_domain(H, W, G)
    f, v = cm.rates(mask), values(H, W, seed=6)
    # no promise: refused whatever was uploaded; a promise, but only rows -1..h: refused on the
    # sides that have a neighbour
    for env, depth, sides in (({}, 2, None), ({"MM_FIELD_HALO": 2}, 1, {0: "below", 1: "above", 2: "above"})):
        engines = chain(gpu, monkeypatch, H, W, G, **env)
        try:
            for g, e in enumerate(engines):
                e.upload(v[e.x_init:e.x_init + e.h])
                upload_field(e, f, depth)
                e.add_diffuse_closed(0)
                before = trace(e)
                for call in (lambda: e.run(1, 1), lambda: e.prepare(1, 1), lambda: e.run(1, 0)):
                    with pytest.raises(gpu.MMError, match="mm error 4") as err:
                        call()
                    msg = str(err.value)
                    assert "MM_FIELD_HALO=2" in msg, msg
                    if sides:
                        assert sides[g] in msg and " 1 have been uploaded" in msg, msg
                assert trace(e) == before
            if sides:  # the missing rows arrive: the chain runs
                for e in engines:
                    upload_field(e, f, 2)
                assert run_chain(engines, 2) == 1
                got = np.vstack([e.download() for e in engines])
                vc.assert_same_bits(got, reference(("chain", H, W, G), v, f, 2)[2], "after the upload")
        finally:
            for e in engines:
                e.close()


# ---- self-halo: the RCCL path on one rank -------------------------------------------------------
def self_halo_engine(gpu, monkeypatch, H, W, **env):
    env = dict(env, MM_SELF_HALO=1)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, str(val))
    try:
        return gpu.Engine(H, W, halo_mode=gpu.MM_HALO_RCCL, comm_id_bytes=gpu.comm_id())
    finally:
        for k in env:
            monkeypatch.delenv(k)


def test_self_halo_graph_and_eager(gpu, monkeypatch):
    H, W = 50, 257
    mask = cm.domain("seams", H, W) & cm.domain("random", H, W, seed=4)
    f, v = cm.rates(mask), values(H, W, seed=7)
    states = reference(("self",), v, f, 14)
    for graph in (1, 0):
        with self_halo_engine(gpu, monkeypatch, H, W, MM_FIELD_HALO=2, MM_GRAPH=graph) as e:
            e.upload(v)
            e.rate_field_upload(f)
            e.add_diffuse_closed(0)
            info = e.info()
            assert (info["kernel"], info["steps_per_launch"], info["halo_depth"]) == (0, 1, 1), info
            e.run(7, reduce_every=1)
            vc.assert_same_bits(e.download(), states[7], ("self-halo", graph, 7))
            e.run(7, reduce_every=1)
            vc.assert_same_bits(e.download(), states[14], ("self-halo", graph, 14))
            assert e.info()["graph_state"] == graph
            assert_history(e.sums_history(), states, range(1, 15), ("self-halo", graph))


def test_one_slab_with_a_halo_mode_needs_the_promise(gpu, monkeypatch):
    """Any halo mode makes a slab one with a halo: without MM_FIELD_HALO=2 it is refused (the
    host transport on one slab: no communicator to set up)."""
    H, W = 27, 257
    f, v = cm.rates(cm.domain("disc", H, W)), values(H, W, seed=7)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    with gpu.Engine(H, W, halo_mode=gpu.MM_HALO_HOST) as e:
        e.upload(v)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        before = trace(e)
        with pytest.raises(gpu.MMError, match="mm error 4") as err:
            e.run(1)
        assert "MM_FIELD_HALO=2" in str(err.value)
        assert trace(e) == before
    monkeypatch.setenv("MM_FIELD_HALO", "2")
    try:
        e = gpu.Engine(H, W, halo_mode=gpu.MM_HALO_HOST)
    finally:
        monkeypatch.delenv("MM_FIELD_HALO")
    with e:
        e.upload(v)
        e.rate_field_upload(f)
        e.add_diffuse_closed(0)
        e.run(3)
        vc.assert_same_bits(e.download(), cm.closed_steps(v, f, 3), "with the promise")


# ---- lifetime: closed, field, closed with moved walls, mixed --------------------------------------
class ClosedModel(M.EngineModel):
    """tests/engine_model.py's model with flow kind 4."""

    def add_diffuse_closed(self, attr):
        self._attr(attr)
        self.flows.append((CLOSED, attr, attr, 0.0))

    def step(self):
        flows, self.flows = self.flows, []
        try:
            for fl in flows:
                if fl[0] == CLOSED:
                    self.v[fl[1]] = cm.closed_step(self.v[fl[1]], self.f[fl[1]])
                else:
                    self.flows = [fl]
                    M.EngineModel.step(self)
        finally:
            self.flows = flows

    def run(self, nsteps, reduce_every=0):
        for fl in self.flows:
            if nsteps > 0 and fl[0] == CLOSED and self.f[fl[1]] is None:
                raise M.ModelError(f"run: attribute {fl[1]} has no rate field")
        M.EngineModel.run(self, nsteps, reduce_every)


def C(a):
    return (CLOSED, a, a, 0.0)


def program(flows):
    out = [("clear_flows", ())]
    for fl in flows:
        out += [("add_diffuse_closed", (fl[1],))] if fl[0] == CLOSED else M.program([fl], clear=False)
    return out


def lifetime_script(H, W):
    f1 = cm.rates(cm.domain("disc", H, W))
    f2 = cm.rates(cm.domain("random", H, W, seed=9), seed=9)  # the walls moved
    s = [("fill_random", (0, M.SEED)), ("rate_field_upload", (f1, 0, 0))]
    s += program([C(0)]) + [("run", (16, 0)), ("run", (16, 0)), ("run", (7, 3))]
    s += program([M.F(0)]) + [("run", (16, 0)), ("run", (8, 1))]
    s += [("rate_field_upload", (f2, 0, 0))]
    s += program([C(0)]) + [("run", (16, 0)), ("run", (17, 2))]
    s += program([M.T(0, -1, 0.05), C(0), M.D(0, 0.1)]) + [("run", (7, 1)), ("run", (16, 0))]
    s += program([M.F(0)]) + [("run", (8, 0))]
    return s


@pytest.mark.parametrize("mode", ["checked", "free"])
@pytest.mark.parametrize("cfg", [(1, {}, (27, 257)), (1, {"MM_FIELD_STEPS": 4, "MM_SEG_WAVES": 64}, (50, 257))],
                         ids=M.config_id)
def test_lifetime(gpu, O, monkeypatch, cfg, mode):
    _, _, (H, W) = cfg
    script = lifetime_script(H, W)
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
        if any(fl[0] == CLOSED for fl in m.flows):
            assert got["info"]["kernel"] == 0 and got["info"]["steps_per_launch"] == 1
            assert got["info"]["n_passes"] == len(m.flows)
            assert all(got["plans"][n] == [1] * n for n in PLAN_STEPS)
            assert got["kernels"][1][0] == 0

    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
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
        e.synchronize()
        bad = mismatch(e, m)
        assert bad is None, bad
        info = e.info()
        assert (info["steps_done"], info["hist_entries"]) == (m.steps_done, len(m.hist))
        same_plans(len(script) - 1, e)


# ---- timing: 24 B per cell of the closed attribute, 16 B of every other -----------------------------
@pytest.mark.parametrize("n_attr", [1, 2])
def test_timing_bytes(gpu, monkeypatch, n_attr):
    H, W = 27, 257
    f = cm.rates(cm.domain("disc", H, W))
    vs = [values(H, W, seed=40 + a) for a in range(n_attr)]
    with engine(gpu, monkeypatch, H, W, n_attr=n_attr) as e:
        for a in range(n_attr):
            e.upload(vs[a], a)
        e.rate_field_upload(f, attr=n_attr - 1)
        e.add_diffuse_closed(n_attr - 1)
        e.set_timing(True)
        e.run(3)
        n, ms, nbytes = e.timing()
        assert n == 3 and ms > 0.0
        assert nbytes == (24.0 + 16.0 * (n_attr - 1)) * H * W
        e.set_timing(False)
        vc.assert_same_bits(e.download(n_attr - 1), cm.closed_steps(vs[n_attr - 1], f, 3), "timed")
        if n_attr == 2:
            assert e.download(0).tobytes() == vs[0].tobytes()
