"""K fused steps of the closed rate-field diffusion per pass on slabs with a halo
(MM_CLOSED_HALO): host-transport chains, the RCCL path on one rank (MM_SELF_HALO) and what must
stay one step per pass.

A K-step closed pass of a slab in a chain reads K ghost rows of the state (exchanged) and K + 1
of the rate field (static, never exchanged: the caller promises them with MM_CLOSED_HALO=K+1
at creation and uploads them). The interior rows run mm_closedk_kernel's segment schedule, the
K border rows of each side its block schedule. Expected states come from
closed_model.closed_steps on the WHOLE grid and are compared as bits
(value_classes.assert_same_bits); sums and the history within 1e-12 * |want| on positive
values, as tests/test_gpu_closedk.py does. Grids are at most 77 x 300 except in the last test.
"""
import numpy as np
import pytest

import closed_model as cm
import engine_model as M
import test_gpu_closed as closed
import test_gpu_closedk as ck
import value_classes as vc
from test_gpu_closed import C, ClosedModel, assert_history, dilate_open, program, values
from test_gpu_lifetime import plan_facts
from test_gpu_ratefield import run_chain

pytestmark = pytest.mark.gpu

CLOSEDK = ck.CLOSEDK
KS = ck.KS
KMAX = ck.KMAX
STEPS = 7
# (H, W, G): 19/20-row slabs with odd x_init, split, 3 strips; h = 9 = 2K + 1 at K = 4, the
# thinnest split slab (1 interior row); h = 8, too thin to split at K = 4 and split at K = 2, 3;
# h = 2, K capped by min_rows; 2 strips, both edge strips
SHAPES = [(77, 300, 4), (27, 257, 3), (24, 257, 3), (16, 130, 8), (40, 130, 2)]
DOMAINS = ["open", "random", "disc", "seam", "kborder"]
KNOBS = ck.KNOBS + ("MM_CLOSED_HALO",)


def chain(gpu, monkeypatch, H, W, G, n_attr=1, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return closed.make_chain(gpu, monkeypatch, H, W, G, n_attr=n_attr, env=env)


def close(engines):
    for e in engines:
        e.close()


def upload_field(e, f, depth):
    closed.upload_field(e, f, depth)


def plan_of(e):
    info = e.info()
    return info["kernel"], info["steps_per_launch"], info["halo_depth"]


def gather(engines):
    return np.vstack([e.download() for e in engines])


def rank_ordered_sums(engines):
    return sum(e.sums_history() for e in engines)  # rank order, as src/Model.hpp:89-92


def domain(kind, H, W, G, K):
    """open / random / disc of closed_model; `seam`: closed.seam_domain, wall lines with gaps on
    the slab seams; `kborder`: such lines on rows K-1, K, h-K-1, h-K of every slab, the seams
    between its border blocks and its interior segments. At 257 and 300 columns the `kseams`
    columns (the K-step strips' seams) are walled with gaps as well."""
    if kind == "seam":
        mask = closed.seam_domain(H, W, G)
    elif kind == "kborder":
        mask = cm.domain("random", H, W, seed=11)
        for g in range(G):
            x0, x1 = g * H // G, (g + 1) * H // G
            for r in (x0 + K - 1, x0 + K, x1 - K - 1, x1 - K):
                if x0 <= r < x1:
                    mask[r, :] = False
                    mask[r, (r % 4)::9] = True
    else:
        mask = cm.domain(kind, H, W)
    if W in (257, 300):
        mask = mask & ck.domain("kseams", H, W, K)
    return mask


def closed_chain(gpu, monkeypatch, v, f, G, K, depth=None, **env):
    """A host chain created with MM_CLOSED_STEPS=K, MM_CLOSED_HALO=K+1: the slabs of v, rows
    -depth .. h + depth of f (K + 1 unless given) on every slab, one closed diffusion."""
    H, W = v.shape
    env = dict({"MM_CLOSED_STEPS": K, "MM_CLOSED_HALO": K + 1}, **env)
    engines = chain(gpu, monkeypatch, H, W, G, **env)
    try:
        for e in engines:
            e.upload(v[e.x_init:e.x_init + e.h])
            upload_field(e, f, K + 1 if depth is None else depth)
            e.add_diffuse_closed(0)
    except BaseException:
        close(engines)
        raise
    return engines


_SINGLE = {}


def single_engine(gpu, monkeypatch, key, v, f, K, steps):
    """The single-engine K-step result after `steps` steps, computed once per key."""
    if key not in _SINGLE:
        with ck.closed_engine(gpu, monkeypatch, v, f, K) as e:
            ck.check_plan(e, v.shape[1], K)
            e.run(steps)
            _SINGLE[key] = e.download()
    return _SINGLE[key]


# ---- 1. host chains, bit for bit (fails without the feature: kernel is 0 on a chain) -----------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("kind", DOMAINS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-G%d" % s)
def test_host_chain_bit_for_bit(gpu, monkeypatch, shape, kind, K):
    H, W, G = shape
    k = min(K, H // G)
    mask = domain(kind, H, W, G, K)
    f, v = cm.rates(mask), values(H, W, seed=6)
    key = ("chain", shape, kind, K)
    states = ck.reference(key, v, f, STEPS)
    for steps in (K, K + 1, STEPS):
        engines = closed_chain(gpu, monkeypatch, v, f, G, K)
        try:
            for e in engines:
                assert plan_of(e) == (CLOSEDK, k, k), e.info()
                assert e.info()["kernel"] == 5
                assert e.pass_kernel(k) == (CLOSEDK, 2, -(-W // ck.out_cols(k)))
            plan = engines[0].pass_plan(steps)
            assert plan == ck.balanced(steps, k) and all(e.pass_plan(steps) == plan for e in engines)
            if k == 4 and steps == STEPS:
                assert plan == [4, 3]
            assert run_chain(engines, steps, reduce_every=1) == k
            got = gather(engines)
            tot = rank_ordered_sums(engines)
        finally:
            close(engines)
        vc.assert_same_bits(got, states[steps], (shape, kind, K, steps))
        assert np.array_equal(got[~mask].view(np.uint64), v[~mask].view(np.uint64))
        assert_history(tot, states, range(1, steps + 1), (shape, kind, K, steps))
        if K <= H:
            single = single_engine(gpu, monkeypatch, key + (steps,), v, f, K, steps)
            assert got.tobytes() == single.tobytes(), (shape, kind, K, steps)


# ---- 2. the field's ghost rows matter ----------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_field_ghost_rows_matter(gpu, monkeypatch, K):
    """f of ghost row -(K+1) of one slab alone is changed (walls where cells were open): that
    slab's result changes, so the row is read; the same edit at row -(K+2) changes nothing."""
    H, W, G = 40, 130, 2
    f, v = cm.rates(cm.domain("open", H, W), negative=False), values(H, W, seed=2)
    want = cm.closed_steps(v, f, K)
    x0 = H // G  # slab 1's first row
    got = {}
    for row in (None, -(K + 1), -(K + 2)):
        engines = closed_chain(gpu, monkeypatch, v, f, G, K, depth=K + 2)
        try:
            assert all(plan_of(e) == (CLOSEDK, K, K) for e in engines)
            if row is not None:
                edit = f[x0 + row:x0 + row + 1].copy()
                edit[:, 1::2] = 0.0
                e = engines[1]
                # rows row .. -1 again, the first of them edited: the recorded depth stays
                e.rate_field_upload(np.vstack([edit, f[x0 + row + 1:x0]]), row0=row)
            assert run_chain(engines, K) == K
            got[row] = gather(engines)
        finally:
            close(engines)
    vc.assert_same_bits(got[None], want, (K, "unedited"))
    assert got[-(K + 2)].tobytes() == got[None].tobytes()
    assert got[-(K + 1)][:x0].tobytes() == got[None][:x0].tobytes()  # slab 0 holds its own rows of f
    diff = np.argwhere(got[-(K + 1)] != got[None])
    assert len(diff) and set(diff[:, 0]) == {x0}, (K, sorted(set(diff[:, 0])))


# ---- 3. refusing a broken promise --------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_refusals_leave_no_trace(gpu, monkeypatch, K):
    H, W, G = 27, 257, 3
    mask = domain("seam", H, W, G, K)
    f, v = cm.rates(mask), values(H, W, seed=6)
    states = ck.reference(("refuse", K), v, f, STEPS)
    engines = closed_chain(gpu, monkeypatch, v, f, G, K, depth=K)  # one row short a side
    try:
        sides = {0: ["below"], 1: ["above", "below"], 2: ["above"]}
        for g, e in enumerate(engines):
            assert plan_of(e) == (CLOSEDK, K, K)
            before = closed.trace(e)
            for call in (lambda: e.run(K, 1), lambda: e.prepare(K, 1), lambda: e.run(1, 0)):
                with pytest.raises(gpu.MMError, match="mm error 4") as err:
                    call()
                msg = str(err.value)
                assert "attribute 0" in msg and sides[g][0] in msg and "MM_CLOSED_HALO" in msg, msg
                assert "read %d ghost rows" % (K + 1) in msg, msg
                assert " %d have been uploaded" % K in msg, msg
            assert closed.trace(e) == before
        # the missing row arrives on one side of the middle slab: the other is still refused
        e = engines[1]
        e.rate_field_upload(f[e.x_init - K - 1:e.x_init - K], row0=-K - 1)
        with pytest.raises(gpu.MMError, match="mm error 4") as err:
            e.run(K, 1)
        assert "below" in str(err.value)
        for e in engines:
            upload_field(e, f, K + 1)
        assert run_chain(engines, STEPS, reduce_every=1) == K
        got = gather(engines)
        tot = rank_ordered_sums(engines)
    finally:
        close(engines)
    vc.assert_same_bits(got, states[STEPS], (K, "after the upload"))
    assert_history(tot, states, range(1, STEPS + 1), (K, "refused runs left no entry"))


def test_fill_keeps_the_promise(gpu, monkeypatch):
    H, W, G, K, r = 27, 257, 3, KMAX, 0.125
    v = values(H, W, seed=4)
    engines = chain(gpu, monkeypatch, H, W, G, MM_CLOSED_STEPS=K, MM_CLOSED_HALO=K + 1)
    try:
        for e in engines:
            e.upload(v[e.x_init:e.x_init + e.h])
            e.rate_field_upload(np.full((e.h, W), r))  # the owned rows alone: refused
            e.add_diffuse_closed(0)
            with pytest.raises(gpu.MMError, match="mm error 4"):
                e.run(K)
            e.rate_field_fill(r)
        assert run_chain(engines, STEPS) == K
        got = gather(engines)
    finally:
        close(engines)
    vc.assert_same_bits(got, cm.closed_steps(v, np.full((H, W), r), STEPS), "fill")


# ---- 4. where it must stay one step on a chain -------------------------------------------------
def one_step_chain(gpu, monkeypatch, v, f, steps, n_attr=1, attr=0, **env):
    """A 27 x 257 chain of 3 under `env`, rows -5 .. h + 5 of the field on every slab: every slab
    plans one step per pass; the state of `attr` after `steps` steps."""
    H, W, G = 27, 257, 3
    engines = chain(gpu, monkeypatch, H, W, G, n_attr=n_attr, **env)
    try:
        for e in engines:
            e.upload(v[e.x_init:e.x_init + e.h], attr)
            lo, hi = max(e.x_init - 5, 0), min(e.x_init + e.h + 5, H)
            e.rate_field_upload(f[lo:hi], attr=attr, row0=lo - e.x_init)
            e.add_diffuse_closed(attr)
            assert plan_of(e) == (0, 1, 1), (env, e.info())
            assert e.pass_plan(5) == [1] * 5 and e.pass_kernel(KMAX)[0] == 0
        assert run_chain(engines, steps) == 1
        return np.vstack([e.download(attr) for e in engines])
    finally:
        close(engines)


@pytest.mark.parametrize("env", [{"MM_FIELD_HALO": 2, "MM_CLOSED_STEPS": 4},
                                 {"MM_FIELD_HALO": 4, "MM_CLOSED_STEPS": 4},  # tests/program_cli.cpp
                                 {"MM_CLOSED_HALO": 5},
                                 {"MM_CLOSED_HALO": 5, "MM_CLOSED_STEPS": 1},
                                 {"MM_CLOSED_HALO": 5, "MM_CLOSED_STEPS": 4, "MM_PASSK": 0},
                                 {"MM_CLOSED_HALO": 2},
                                 {"MM_CLOSED_HALO": 2, "MM_CLOSED_STEPS": 4},
                                 {"MM_CLOSED_HALO": 6, "MM_FIELD_HALO": 2, "MM_CLOSED_STEPS": 4}],
                         ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()))
def test_chain_stays_one_step(gpu, monkeypatch, env):
    H, W, steps = 27, 257, 5
    f, v = cm.rates(domain("seam", H, W, 3, 2)), values(H, W, seed=6)
    got = one_step_chain(gpu, monkeypatch, v, f, steps, **env)
    vc.assert_same_bits(got, ck.reference(("one-step",), v, f, steps)[steps], env)


def test_other_programs_stay_one_step(gpu, monkeypatch):
    H, W, steps = 27, 257, 4
    env = {"MM_CLOSED_HALO": KMAX + 1, "MM_CLOSED_STEPS": KMAX}
    f, v = cm.rates(domain("seam", H, W, 3, 2)), values(H, W, seed=6)
    want = ck.reference(("one-step",), v, f, 5)[steps]
    # two attributes: the closed one is attribute 1, the other is copied through
    got = one_step_chain(gpu, monkeypatch, v, f, steps, n_attr=2, attr=1, **env)
    vc.assert_same_bits(got, want, "two attributes")
    # a transfer beside the diffusion: two passes per step
    engines = chain(gpu, monkeypatch, H, W, 3, **env)
    try:
        for e in engines:
            e.rate_field_fill(0.1)
            e.add_transfer(0, -1, 0.05)
            e.add_diffuse_closed(0)
            assert plan_of(e) == (0, 1, 1) and e.info()["n_passes"] == 2
            assert e.pass_plan(5) == [1] * 5 and e.pass_kernel(KMAX)[0] == 0
    finally:
        close(engines)
    with closed.self_halo_engine(gpu, monkeypatch, 50, 257, **env) as e:
        e.rate_field_fill(0.1)
        e.add_transfer(0, -1, 0.05)
        e.add_diffuse_closed(0)
        assert plan_of(e) == (0, 1, 1) and e.info()["n_passes"] == 2


# ---- 5. the RCCL path on one rank --------------------------------------------------------------
def self_halo(gpu, monkeypatch, v, f, K, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    e = closed.self_halo_engine(gpu, monkeypatch, *v.shape, MM_CLOSED_HALO=K + 1, MM_CLOSED_STEPS=K, **env)
    e.upload(v)
    e.rate_field_upload(f)  # no real neighbour: no ghost rows to promise
    e.add_diffuse_closed(0)
    return e


@pytest.mark.parametrize("K", KS)
def test_self_halo_graph_and_eager(gpu, monkeypatch, K):
    H, W = 50, 257
    mask = domain("kborder", H, W, 1, K)
    f, v = cm.rates(mask), values(H, W, seed=7)
    states = ck.reference(("self", K), v, f, 14)
    for graph in (1, 0):
        with self_halo(gpu, monkeypatch, v, f, K, MM_GRAPH=graph) as e:
            assert plan_of(e) == (CLOSEDK, K, K), e.info()
            assert e.pass_plan(7) == ck.balanced(7, K)
            e.run(7, reduce_every=1)
            vc.assert_same_bits(e.download(), states[7], ("self-halo", K, graph, 7))
            e.run(7, reduce_every=1)
            vc.assert_same_bits(e.download(), states[14], ("self-halo", K, graph, 14))
            # a graph holds an even number of K-step passes: 7 steps hold one up to K = 3 (K = 4
            # replays in test_self_halo_odd_flips_and_prepare)
            assert e.info()["graph_state"] == (graph if 2 * K <= 7 else 0)
            assert_history(e.sums_history(), states, range(1, 15), ("self-halo", K, graph))


@pytest.mark.parametrize("K", KS)
def test_self_halo_odd_flips_and_prepare(gpu, monkeypatch, K):
    """run(3K) is three passes, an odd number of flips per replayed graph; prepare arrives in
    mid-life, between two runs, and runs no step."""
    H, W = 50, 257
    f, v = cm.rates(domain("disc", H, W, 1, K)), values(H, W, seed=12)
    calls = [3 * K, 3 * K, 3 * K, K]
    want, w = [], v
    for n in calls:
        w = cm.closed_steps(w, f, n)
        want.append(w)
    got = {}
    for graphs in (1, 0):
        with self_halo(gpu, monkeypatch, v, f, K, MM_GRAPH=graphs) as e:
            assert plan_of(e) == (CLOSEDK, K, K) and e.pass_plan(3 * K) == [K] * 3
            for i, n in enumerate(calls):
                if i == 1:
                    before = e.download().tobytes()
                    e.prepare(n, K)
                    assert e.download().tobytes() == before
                e.run(n, reduce_every=K if i == 1 else 0)
                got[graphs, i] = e.download()
                info = e.info()
                assert info["graph_state"] == graphs, (i, info)
            if graphs:
                assert info["graph_launches"] >= 3, info
            else:
                assert info["graph_launches"] == 0, info
            hist = e.sums_history()
        assert hist.shape == (3, 1)
        for j in range(3):
            closed.assert_sums(hist[j, 0], cm.closed_steps(want[0], f, (j + 1) * K), (K, graphs, j))
    for i in range(len(calls)):
        vc.assert_same_bits(got[1, i], want[i], (K, i))
        assert got[1, i].tobytes() == got[0, i].tobytes(), (K, i)


# ---- 6. value classes on every seam ------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("cls", vc.CLASSES)
def test_value_classes(gpu, monkeypatch, cls, K):
    H, W, G = 77, 300, 4
    mask = domain("random", H, W, G, K)
    rng = np.random.default_rng(11)
    f = np.where(mask, vc.RATES[cls] * rng.uniform(0.5, 1.0, (H, W)), 0.0)
    # seeds on the slab seams and on the seams between border blocks and interior segments
    rows = []
    for g in range(G):
        x0, x1 = g * H // G, (g + 1) * H // G
        rows += [x0, x0 + K - 1, x0 + K, x1 - K - 1, x1 - K, x1 - 1]
    o = ck.out_cols(K)
    cols = [0, o - 1, o, W // 2, 2 * o - 1, 2 * o, W - 1]
    pos_open, pos_wall = [], []
    for i, r in enumerate(rows):
        for c in (cols[i % len(cols)], cols[(i + 3) % len(cols)]):
            cands = [(r, y) for y in range(max(c - 3, 0), min(c + 4, W))]
            pos_open += [p for p in cands if mask[p]][:1]
            pos_wall += [p for p in cands if not mask[p]][:1]
    pos = tuple(dict.fromkeys(pos_open + pos_wall))
    assert len(pos_open) >= len(rows) and len(pos_wall) >= G
    start = vc.make(cls, H, W, positions=pos)
    if cls != "nonfinite":
        for x, y in pos[::3]:
            start[x, y] = -0.0
    passes = 2
    states = ck.reference(("vc-chain", cls, K), start, f, passes * K)
    engines = closed_chain(gpu, monkeypatch, start, f, G, K)
    try:
        assert all(plan_of(e) == (CLOSEDK, K, K) and e.h >= 2 * K + 1 for e in engines)
        bad = ~np.isfinite(start) & mask
        for p in range(1, passes + 1):
            assert all(e.pass_plan(K) == [K] for e in engines)
            run_chain(engines, K, 1)  # one K-step pass
            got = gather(engines)
            vc.assert_same_bits(got, states[p * K], (cls, K, p))
            assert np.array_equal(got[~mask].view(np.uint64), start[~mask].view(np.uint64)), (cls, K, p)
            if cls == "nonfinite":
                # without the model: the K-fold dilation of the open seeds through open cells;
                # the walls' seeds stay where they are
                for _ in range(K):
                    bad = dilate_open(bad, mask)
                assert bad.sum() > len(pos_open)
                assert np.array_equal(~np.isfinite(got), bad | (~np.isfinite(start) & ~mask)), (K, p)
        hist = rank_ordered_sums(engines)
    finally:
        close(engines)
    assert hist.shape == (passes * K, 1)
    for s in range(1, passes * K + 1):
        if np.all(np.isfinite(states[s])):
            vc.assert_sum_close(hist[s - 1, 0], states[s], (cls, K, s))
        else:
            assert not np.isfinite(hist[s - 1, 0])


@pytest.mark.parametrize("K", KS)
def test_nan_padding(gpu, monkeypatch, K):
    H, W, G = 27, 257, 3
    f, v = cm.rates(domain("seam", H, W, G, K)), values(H, W, seed=5)
    states = ck.reference(("pad-chain", K), v, f, STEPS)
    engines = closed_chain(gpu, monkeypatch, v, f, G, K)
    try:
        for e in engines:
            e.fill_padding(float("nan"))  # of the state and of the field, ghost rows included
        assert run_chain(engines, STEPS, reduce_every=1) == K
        got = gather(engines)
        tot = rank_ordered_sums(engines)
    finally:
        close(engines)
    vc.assert_same_bits(got, states[STEPS], ("padding", K))
    assert np.all(np.isfinite(tot))
    assert_history(tot, states, range(1, STEPS + 1), ("padding", K))


# ---- 7. lifetime: closed K-step, field, closed again -------------------------------------------
@pytest.mark.parametrize("mode", ["checked", "free"])
def test_chain_reprogrammed_in_lockstep(gpu, O, monkeypatch, mode):
    H, W, G, K = 27, 257, 3, KMAX
    env = dict(M.CHAIN_ENV, MM_CLOSED_HALO=K + 1, MM_CLOSED_STEPS=K)
    f1 = cm.rates(domain("seam", H, W, G, K))
    f2 = cm.rates(cm.domain("random", H, W, seed=9), seed=9)  # the walls moved
    script = [("fill_random", (0, M.SEED)), ("rate_field_upload", (f1, 0, 0))]
    script += program([C(0)]) + [("run", (7, 1)), ("run", (2 * K, 0))]
    script += program([M.F(0)]) + [("run", (5, 1))]
    script += [("rate_field_upload", (f2, 0, 0))]
    script += program([C(0)]) + [("run", (7, 1)), ("run", (K + 1, 2))]
    kernels = []
    m = ClosedModel(O, H, W)
    engines = chain(gpu, monkeypatch, H, W, G, **env)
    try:
        for i, (method, call) in enumerate(script):
            M.apply_op(m, method, call)
            if method == "run":
                depth = run_chain(engines, *call)
                if mode == "free" and i != len(script) - 1:
                    continue
                # a fresh chain given only this program plans the same
                fresh = chain(gpu, monkeypatch, H, W, G, **env)
                try:
                    for fe in fresh:
                        fe.rate_field_fill(0.0, 0)
                        for pm, pa in program(m.flows)[1:]:
                            M.apply_op(fe, pm, pa)
                    facts = [plan_facts(fe, True) for fe in fresh]
                finally:
                    close(fresh)
                assert facts[0]["info"]["halo_depth"] == depth, (i, script[i][0])
                assert [plan_facts(e, True) for e in engines] == facts, (i, script[i][0])
                kernels.append((facts[0]["info"]["kernel"], depth))
                assert gather(engines).tobytes() == m.v[0].tobytes(), (i, script[i][0])
                tot, want = rank_ordered_sums(engines), m.sums_history()
                assert tot.shape == want.shape, (i, script[i][0])
                assert np.all(np.abs(tot - want) <= 1e-12 * np.abs(want)), (i, script[i][0])
                assert all(e.info()["steps_done"] == m.steps_done for e in engines)
            elif method == "rate_field_upload":
                for e in engines:
                    upload_field(e, call[0], K + 1)
            else:
                for e in engines:
                    M.apply_op(e, method, call)
    finally:
        close(engines)
    if mode == "checked":
        assert kernels == [(CLOSEDK, K), (CLOSEDK, K), (0, 1), (CLOSEDK, K), (CLOSEDK, K)]
    else:
        assert kernels == [(CLOSEDK, K)]


# ---- 8. at size, once --------------------------------------------------------------------------
def test_self_halo_2048(gpu, monkeypatch):
    """A self-halo 2048 x 2048 disc, K = 4, 8 steps: the occupancy-sized segment plan, 18 strips
    of border blocks, the sums every 4 steps; as bits against the unsplit K = 4 engine."""
    H = W = 2048
    K, steps = KMAX, 8
    mask = cm.domain("disc", H, W)
    f, v = cm.rates(mask), values(H, W, seed=2)
    with ck.closed_engine(gpu, monkeypatch, v, f, K) as e:
        ck.check_plan(e, W, K)
        e.run(steps, reduce_every=4)
        want, want_hist = e.download(), e.sums_history()
    with self_halo(gpu, monkeypatch, v, f, K) as e:
        info = e.info()
        assert plan_of(e) == (CLOSEDK, K, K), info
        assert 16 <= info["rows_per_wave"] < H, info
        assert e.pass_kernel(K) == (CLOSEDK, 2, 18)
        e.run(steps, reduce_every=4)
        got, hist = e.download(), e.sums_history()
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (len(bad), bad[:4].tolist(), bad[-1].tolist())
    assert np.array_equal(got[~mask].view(np.uint64), v[~mask].view(np.uint64))
    assert hist.shape == want_hist.shape == (2, 1)
    assert np.all(np.abs(hist - want_hist) <= 1e-12 * np.abs(want_hist))
