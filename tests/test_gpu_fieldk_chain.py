"""K fused steps of the rate-field diffusion per pass on slabs with a halo (MM_FIELD_HALO):
host-transport chains, the RCCL path on one rank (MM_SELF_HALO) and what must stay one step.

A K-step pass of a slab in a chain reads K ghost rows of the state (exchanged) and of the rate
field (static, never exchanged: the caller promises them with MM_FIELD_HALO=d at creation and
uploads them). The interior rows run mm_fieldk_kernel's segment schedule, the K border rows of
each side its block schedule. Unless stated the expected state is or_field_step_general of
oracle/mm_oracle.c with outf = f * v iterated on the WHOLE grid and every cell is compared
bit for bit; only the step sums (another summation order) get the project's 1e-12 bound.
"""
import math

import numpy as np
import pytest

import engine_model as M
import value_classes as vc
from test_gpu_lifetime import plan_facts
from test_gpu_ratefield import (make_chain, neighbour_counts, oracle_step, random_field, reference,
                                run_chain)
from test_gpu_values import check_cells, check_sums, seed_positions
from test_gpu_values import reference as class_reference

pytestmark = pytest.mark.gpu

FIELDK = 4  # mm_info.kernel of mm_fieldk_kernel
HALO = 4    # MM_FIELD_HALO of these tests: the deepest K
STEPS = 7   # 4 + 3 at K = 4
# (H, W, G): 19/20-row slabs with odd x_init, split, 3 strips (the interior strip of the
# middle slabs runs FAST border blocks); h = 9 = 2K + 1 at K = 4, the thinnest split slab
# (1 interior row); h = 8, too thin to split at K = 4 and split at K = 2, 3; h = 2, K capped
# by min_rows; 2 strips, both edge strips
SHAPES = [(77, 300, 4), (27, 257, 3), (24, 257, 3), (16, 130, 8), (40, 130, 2)]
KNOBS = ("MM_FIELD_STEPS", "MM_FIELD_HALO", "MM_SEG_WAVES", "MM_KERNEL_VARIANT", "MM_WIDE",
         "MM_STEPS_PER_PASS", "MM_SEG_EDGE", "MM_PASSK", "MM_GRAPH", "MM_SELF_HALO")


def out_cols(k):
    return 128 - 4 * ((k + 1) // 2)


def chain(gpu, monkeypatch, H, W, G, n_attr=1, **env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return make_chain(gpu, monkeypatch, H, W, G, n_attr=n_attr, env=env)


def close(engines):
    for e in engines:
        e.close()


def upload_field(e, f, depth, attr=0):
    """The slab's rows -depth .. h + depth of the global field f, clipped to the grid."""
    lo, hi = max(e.x_init - depth, 0), min(e.x_init + e.h + depth, f.shape[0])
    e.rate_field_upload(f[lo:hi], attr=attr, row0=lo - e.x_init)


def plan_of(e):
    info = e.info()
    return info["kernel"], info["steps_per_launch"], info["halo_depth"]


def balanced(n, k):
    out = []
    while n:
        out.append(-(-n // -(-n // k)))
        n -= out[-1]
    return out


def gather(engines):
    return np.vstack([e.download() for e in engines])


def rank_ordered_sums(engines):
    hists = [e.sums_history() for e in engines]
    tot = np.zeros(hists[0].shape[0])
    for h in hists:  # rank order, as src/Model.hpp:89-92
        assert h.shape == (len(tot), 1), h.shape
        tot = tot + h[:, 0]
    return tot


def field_chain(gpu, monkeypatch, H, W, G, K, f, depth=HALO, **env):
    """A host chain created with MM_FIELD_HALO=HALO, MM_FIELD_STEPS=K: fill_random state, rows
    -depth .. h + depth of f on every slab, one field diffusion."""
    engines = chain(gpu, monkeypatch, H, W, G, MM_FIELD_HALO=HALO, MM_FIELD_STEPS=K, **env)
    try:
        for e in engines:
            e.fill_random(0)
            upload_field(e, f, depth)
            e.add_diffuse_field(0)
    except BaseException:
        close(engines)
        raise
    return engines


# ---- 1. host chains, bit for bit (fails without the feature: kernel is 0 on a chain) -----------
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-G%d" % s)
def test_host_chain_bit_for_bit(gpu, O, monkeypatch, shape, K):
    H, W, G = shape
    k = min(K, H // G)
    engines = field_chain(gpu, monkeypatch, H, W, G, K, random_field(H, W))
    try:
        for e in engines:
            assert plan_of(e) == (FIELDK, k, k), e.info()
            assert e.pass_kernel(k) == (FIELDK, 2, -(-W // out_cols(k)))
        plan = engines[0].pass_plan(STEPS)
        assert plan == balanced(STEPS, k) and all(e.pass_plan(STEPS) == plan for e in engines)
        if k == 4:
            assert plan == [4, 3]
        assert run_chain(engines, STEPS, reduce_every=1) == k
        got = gather(engines)
        tot = rank_ordered_sums(engines)
    finally:
        close(engines)
    assert np.array_equal(got, reference(O, H, W, STEPS))
    assert tot.shape == (STEPS,)
    for s in range(1, STEPS + 1):
        want = math.fsum(reference(O, H, W, s).ravel())
        assert abs(tot[s - 1] - want) <= 1e-12 * abs(want), s


# ---- 2. the field's ghost rows matter -------------------------------------------------------------
def seam_field(H, W, G):
    """Zero, but the four rows on each side of every seam between slabs: uniform in [0, 0.5]."""
    rng = np.random.default_rng(1234 + H)
    f = np.zeros((H, W))
    for g in range(1, G):
        x0 = g * H // G
        f[x0 - HALO:x0 + HALO] = rng.uniform(0.0, 0.5, (2 * HALO, W))
    return f


def test_field_ghost_rows_matter(gpu, O, monkeypatch):
    H, W, G, K = 27, 257, 3, 4
    f, cnt = seam_field(H, W, G), neighbour_counts(H, W)
    start = O.fill_random(H, W)
    want = start
    for _ in range(K):
        want = oracle_step(O, want, f, cnt)
    # on the CPU, the oracle alone: a slab whose ghost rows of the field were zero, or valid
    # one row deep only, computes other cells in its first pass
    for keep in (0, 1):
        for g in range(G):
            x0, x1 = g * H // G, (g + 1) * H // G
            fz = f.copy()
            fz[:max(x0 - keep, 0)] = 0.0
            fz[x1 + keep:] = 0.0
            v = start
            for _ in range(K):
                v = oracle_step(O, v, fz, cnt)
            assert not np.array_equal(v[x0:x1], want[x0:x1]), (keep, g)
    for _ in range(STEPS - K):
        want = oracle_step(O, want, f, cnt)
    engines = field_chain(gpu, monkeypatch, H, W, G, K, f)
    try:
        assert all(plan_of(e) == (FIELDK, K, K) for e in engines)
        assert run_chain(engines, STEPS) == K
        got = gather(engines)
    finally:
        close(engines)
    assert np.array_equal(got, want)


# ---- 3. refusing a broken promise -----------------------------------------------------------------
def test_missing_ghost_rows_are_refused(gpu, O, monkeypatch):
    H, W, G, K = 27, 257, 3, 4
    f = random_field(H, W)
    engines = field_chain(gpu, monkeypatch, H, W, G, K, f, depth=1)  # rows -1 .. h + 1 only
    try:
        before = []
        for e in engines:
            assert plan_of(e) == (FIELDK, K, K)
            info = e.info()
            before.append((e.download().tobytes(), info["steps_done"], info["hist_entries"],
                           e.sums_history().shape, info["graph_count"]))
        sides = {0: ["below"], 1: ["above", "below"], 2: ["above"]}
        for g, e in enumerate(engines):
            for call in (lambda: e.run(K, 1), lambda: e.prepare(K, 1), lambda: e.run(1, 0)):
                with pytest.raises(gpu.MMError, match="mm error 4") as err:
                    call()
                msg = str(err.value)
                assert "attribute 0" in msg and sides[g][0] in msg and "MM_FIELD_HALO" in msg, msg
                assert "read 4 ghost rows" in msg and " 1 have been uploaded" in msg, msg
            info = e.info()
            assert before[g] == (e.download().tobytes(), info["steps_done"], info["hist_entries"],
                                 e.sums_history().shape, info["graph_count"])
        # rows that do not continue the ones already there do not count
        e = engines[1]
        e.rate_field_upload(f[e.x_init - 4:e.x_init - 2], row0=-4)
        with pytest.raises(gpu.MMError, match="mm error 4"):
            e.run(K, 1)
        # the missing rows: the first and the last slab need nothing on their outer side
        e = engines[0]
        e.rate_field_upload(f[e.h + 1:e.h + 4], row0=e.h + 1)
        e = engines[1]
        e.rate_field_upload(f[e.x_init - 4:e.x_init - 1], row0=-4)
        with pytest.raises(gpu.MMError, match="mm error 4") as err:
            e.run(K, 1)  # the side below is still one row deep
        assert "below" in str(err.value)
        e.rate_field_upload(f[e.x_init + e.h:e.x_init + e.h + 4], row0=e.h)
        e = engines[2]
        e.rate_field_upload(f[e.x_init - 4:e.x_init], row0=-4)
        assert run_chain(engines, STEPS, reduce_every=1) == K
        got = gather(engines)
        tot = rank_ordered_sums(engines)
    finally:
        close(engines)
    assert np.array_equal(got, reference(O, H, W, STEPS))
    assert tot.shape == (STEPS,)  # the refused runs left no entry
    want = math.fsum(reference(O, H, W, STEPS).ravel())
    assert abs(tot[-1] - want) <= 1e-12 * abs(want)


def test_fill_keeps_the_promise(gpu, O, monkeypatch):
    H, W, G, K, r = 27, 257, 3, 4, 0.125
    engines = chain(gpu, monkeypatch, H, W, G, MM_FIELD_HALO=HALO, MM_FIELD_STEPS=K)
    try:
        for e in engines:
            e.fill_random(0)
            e.rate_field_upload(np.full((e.h, W), r))  # the owned rows alone: refused
            e.add_diffuse_field(0)
            with pytest.raises(gpu.MMError, match="mm error 4"):
                e.run(K)
            e.rate_field_fill(r)
        assert run_chain(engines, STEPS) == K
        got = gather(engines)
    finally:
        close(engines)
    want, f, cnt = O.fill_random(H, W), np.full((H, W), r), neighbour_counts(H, W)
    for _ in range(STEPS):
        want = oracle_step(O, want, f, cnt)
    assert np.array_equal(got, want)


# ---- 4. values and padding -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(27, 257, 3), (77, 300, 4)], ids=lambda s: "%dx%d-G%d" % s)
def test_nan_padding(gpu, O, monkeypatch, shape):
    H, W, G = shape
    engines = field_chain(gpu, monkeypatch, H, W, G, 4, random_field(H, W))
    try:
        for e in engines:
            e.fill_padding(float("nan"))  # of the state and of the field, ghost rows included
        assert run_chain(engines, STEPS, reduce_every=1) == 4
        got = gather(engines)
        tot = rank_ordered_sums(engines)
    finally:
        close(engines)
    assert np.array_equal(got, reference(O, H, W, STEPS))
    assert np.all(np.isfinite(tot))
    for s in range(1, STEPS + 1):
        want = math.fsum(reference(O, H, W, s).ravel())
        assert abs(tot[s - 1] - want) <= 1e-12 * abs(want), s


@pytest.mark.parametrize("K", [2, 4])
def test_value_classes(gpu, O, monkeypatch, K):
    H, W, G = 77, 300, 4
    shape, cnt = (H, W), neighbour_counts(H, W)
    for cls in vc.CLASSES:
        # the all-zeros class keeps both signs of zero alive at a negative rate only
        f = -random_field(H, W) if cls == "zeros" else random_field(H, W)
        engines = chain(gpu, monkeypatch, H, W, G, MM_FIELD_HALO=HALO, MM_FIELD_STEPS=K)
        try:
            for e in engines:
                upload_field(e, f, HALO)
                e.add_diffuse_field(0)
                assert plan_of(e) == (FIELDK, K, K)
            info, e1 = engines[0].info(), engines[1]
            assert e1.h >= 2 * K + 1 and W > 2 * out_cols(K)  # split, an interior strip
            pos = list(seed_positions(shape, info["rows_per_wave"], out_cols(K), slab_rows=engines[0].h))
            # the seams between slab 1's border blocks and its interior segments
            pos += [(e1.x_init + K - 1, W // 7), (e1.x_init + K, W - W // 7),
                    (e1.x_init + e1.h - K - 1, W // 2 + 9), (e1.x_init + e1.h - K, W // 2 - 9)]
            pos = tuple(dict.fromkeys(pos))
            start = vc.make(cls, H, W, positions=pos)
            states = class_reference(("fieldk-chain", shape, G, cls, pos), [start],
                                     lambda v: [oracle_step(O, v[0], f, cnt)], K + 1)
            for e in engines:
                e.upload(start[e.x_init:e.x_init + e.h])
            assert all(e.pass_plan(K) == [K] for e in engines)
            run_chain(engines, K, 1)  # one pass of K, then one more step
            check_cells(cls, [gather(engines)], states[K], pos, K, (shape, G, K))
            run_chain(engines, 1, 1)
            check_cells(cls, [gather(engines)], states[K + 1], pos, K + 1, (shape, G, K))
            hist = sum(e.sums_history() for e in engines)  # rank order, as src/Model.hpp:89-92
        finally:
            close(engines)
        check_sums(cls, hist, states[:K + 2], (shape, G, K))


# ---- 5. the RCCL path on one rank ------------------------------------------------------------------
def self_halo_engine(gpu, O, monkeypatch, H, W, flows=None, **env):
    env = dict(env, MM_SELF_HALO=1, MM_FIELD_HALO=HALO, MM_FIELD_STEPS=4)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        e = gpu.Engine(H, W, halo_mode=gpu.MM_HALO_RCCL, comm_id_bytes=gpu.comm_id())
    finally:
        for k in env:
            monkeypatch.delenv(k)
    e.upload(O.fill_random(H, W))
    e.rate_field_upload(random_field(H, W))  # no real neighbour: no ghost rows to promise
    for pm, pa in M.program(flows or [M.F(0)], clear=False):
        M.apply_op(e, pm, pa)
    return e


@pytest.mark.parametrize("H,W", [(64, 130), (50, 257)])
def test_self_halo_graph_and_eager(gpu, O, monkeypatch, H, W):
    K = 4
    calls = [3 * K, 3 * K, 3 * K, K]  # three passes: one graph per buffer parity
    got = {}
    for graphs in (1, 0):
        env = {} if graphs else {"MM_GRAPH": 0}
        with self_halo_engine(gpu, O, monkeypatch, H, W, **env) as e:
            assert plan_of(e) == (FIELDK, K, K), e.info()
            assert e.pass_plan(3 * K) == [K] * 3 and e.pass_plan(7) == [4, 3]
            for i, n in enumerate(calls):
                e.run(n, reduce_every=K if i == 3 else 0)
                got[graphs, i] = e.download()
                info = e.info()
                assert info["graph_state"] == graphs, (i, info)
                if graphs and i == 2:
                    assert info["graph_launches"] == 3 and info["graph_count"] == 2, info
            if not graphs:
                assert info["graph_launches"] == 0, info
            hist = e.sums_history()
        want = math.fsum(reference(O, H, W, sum(calls)).ravel())
        assert hist.shape == (1, 1) and abs(hist[0, 0] - want) <= 1e-12 * abs(want)
    done = 0
    for i, n in enumerate(calls):
        done += n
        assert np.array_equal(got[1, i], reference(O, H, W, done)), i
        assert got[1, i].tobytes() == got[0, i].tobytes(), i


# ---- 6. lifetime: field K-step, uniform diffusion, field again -------------------------------------
def test_chain_reprogrammed_in_lockstep(gpu, O, monkeypatch):
    H, W, G = 27, 257, 3
    env = dict(M.CHAIN_ENV, MM_FIELD_HALO=HALO, MM_FIELD_STEPS=4)
    script = M.fills(1) + M.program([M.F(0)], clear=False)
    script += [("rate_field_upload", (("field", 7, H), 0, 0)), ("run", (7, 1))]
    script += M.program([M.D(0, 0.1)]) + [("run", (8, 1))]
    script += M.program([M.F(0)]) + [("rate_field_upload", (("field", 11, H), 0, 0)), ("run", (7, 1))]
    kernels = []
    m = M.EngineModel(O, H, W)
    engines = chain(gpu, monkeypatch, H, W, G, **env)
    try:
        for i, (method, args) in enumerate(script):
            call = M.materialize(method, args, m)
            M.apply_op(m, method, call)
            if method == "run":
                depth = run_chain(engines, *call)
                # a fresh chain given only this program plans the same
                fresh = chain(gpu, monkeypatch, H, W, G, **env)
                try:
                    for f in fresh:
                        for a in m.field_attrs():
                            f.rate_field_fill(0.0, a)
                        for pm, pa in M.program(m.flows, clear=False):
                            M.apply_op(f, pm, pa)
                    facts = [plan_facts(f, True) for f in fresh]
                finally:
                    close(fresh)
                assert facts[0]["info"]["halo_depth"] == depth, (i, script[i])
                assert [plan_facts(e, True) for e in engines] == facts, (i, script[i])
                kernels.append((facts[0]["info"]["kernel"], depth))
                assert gather(engines).tobytes() == m.v[0].tobytes(), (i, script[i])
                tot, want = rank_ordered_sums(engines), m.sums_history()[:, 0]
                assert tot.shape == want.shape, (i, script[i])
                assert np.all(np.abs(tot - want) <= 1e-12 * np.abs(want)), (i, script[i])
                assert all(e.info()["steps_done"] == m.steps_done for e in engines)
            elif method == "rate_field_upload":
                for e in engines:
                    upload_field(e, call[0], HALO)
            else:
                for e in engines:
                    M.apply_op(e, method, call)
    finally:
        close(engines)
    assert kernels == [(FIELDK, 4), (2, 5), (FIELDK, 4)]  # 2: mm_passk_kernel, M.CHAIN_ENV's K = 5


# ---- 7. what stays as it is ------------------------------------------------------------------------
def one_step_chain(gpu, O, monkeypatch, steps, n_attr=1, flows=None, **env):
    """A 27 x 257 chain of 3 under `env`, rows -4 .. h + 4 of the field on every slab: every
    slab plans one step per pass; the state after `steps` steps."""
    H, W, G = 27, 257, 3
    f = random_field(H, W)
    init = [O.fill_random(H, W, seed=O.SEED + a) for a in range(n_attr)]
    engines = chain(gpu, monkeypatch, H, W, G, n_attr=n_attr, **env)
    try:
        for e in engines:
            for a in range(n_attr):
                e.upload(init[a][e.x_init:e.x_init + e.h], a)
            upload_field(e, f, HALO)
            for fl in flows or [M.F(0)]:
                for pm, pa in M.program([fl], clear=False):
                    M.apply_op(e, pm, pa)
            assert plan_of(e) == (0, 1, 1), (env, e.info())
            assert e.pass_plan(5) == [1] * 5 and e.pass_kernel(4)[0] == 0
        assert run_chain(engines, steps) == 1
        return init, f, [np.vstack([e.download(a) for e in engines]) for a in range(n_attr)]
    finally:
        close(engines)


@pytest.mark.parametrize("env", [{}, {"MM_FIELD_STEPS": 4}, {"MM_FIELD_HALO": 1},
                                 {"MM_FIELD_HALO": 0, "MM_FIELD_STEPS": 4},
                                 {"MM_FIELD_HALO": 5, "MM_FIELD_STEPS": 4},
                                 {"MM_FIELD_HALO": "x", "MM_FIELD_STEPS": 4},
                                 {"MM_FIELD_HALO": 4, "MM_FIELD_STEPS": 1},
                                 {"MM_FIELD_HALO": 4, "MM_FIELD_STEPS": 4, "MM_PASSK": 0}],
                         ids=lambda e: ",".join(f"{k[3:]}={v}" for k, v in e.items()) or "default")
def test_chain_stays_one_step(gpu, O, monkeypatch, env):
    steps = 5
    _, _, got = one_step_chain(gpu, O, monkeypatch, steps, **env)
    assert np.array_equal(got[0], reference(O, 27, 257, steps))


def test_other_programs_stay_one_step(gpu, O, monkeypatch):
    steps, env = 4, {"MM_FIELD_HALO": 4, "MM_FIELD_STEPS": 4}
    cnt = neighbour_counts(27, 257)
    # two attributes: the other one is copied through
    init, f, got = one_step_chain(gpu, O, monkeypatch, steps, n_attr=2, **env)
    want = init[0]
    for _ in range(steps):
        want = oracle_step(O, want, f, cnt)
    assert np.array_equal(got[0], want) and got[1].tobytes() == init[1].tobytes()
    # a transfer beside the diffusion: two passes per step. Slabs with a halo plan it one step
    # per pass (they run one-pass programs only, as before); a single slab runs it
    H, W = 50, 257
    f, cnt = random_field(H, W), neighbour_counts(H, W)
    flows = [M.T(0, -1, 0.05), M.F(0)]
    with self_halo_engine(gpu, O, monkeypatch, H, W, flows=flows) as e:
        assert plan_of(e) == (0, 1, 1) and e.info()["n_passes"] == 2
        assert e.pass_plan(5) == [1] * 5 and e.pass_kernel(4)[0] == 0
    engines = chain(gpu, monkeypatch, 27, 257, 3, **env)
    try:
        for e in engines:
            e.rate_field_fill(0.1)
            for pm, pa in M.program(flows, clear=False):
                M.apply_op(e, pm, pa)
            assert plan_of(e) == (0, 1, 1) and e.info()["n_passes"] == 2
            assert e.pass_plan(5) == [1] * 5 and e.pass_kernel(4)[0] == 0
    finally:
        close(engines)
    for name, v in env.items():
        monkeypatch.setenv(name, str(v))
    try:
        e = gpu.Engine(H, W)
    finally:
        for name in env:
            monkeypatch.delenv(name)
    with e:
        e.upload(O.fill_random(H, W))
        e.rate_field_upload(f)
        for pm, pa in M.program(flows, clear=False):
            M.apply_op(e, pm, pa)
        assert plan_of(e) == (0, 1, 1) and e.info()["n_passes"] == 2
        e.run(steps)
        got = e.download()
    want = O.fill_random(H, W)
    for _ in range(steps):
        want = O.program_step([want], [(O.TRANSFER, 0, -1, 0.05)])[0]
        want = oracle_step(O, want, f, cnt)
    assert np.array_equal(got, want)


def test_single_slab_ignores_the_promise(gpu, O, monkeypatch):
    # no halo: MM_FIELD_HALO changes no plan, and nothing is refused
    H, W = 64, 130
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for halo in (None, 1, 4):
        monkeypatch.setenv("MM_FIELD_STEPS", "3")
        if halo is not None:
            monkeypatch.setenv("MM_FIELD_HALO", str(halo))
        try:
            e = gpu.Engine(H, W)
        finally:
            monkeypatch.delenv("MM_FIELD_STEPS")
            monkeypatch.delenv("MM_FIELD_HALO", raising=False)
        with e:
            e.upload(O.fill_random(H, W))
            e.rate_field_upload(random_field(H, W))
            e.add_diffuse_field(0)
            assert plan_of(e) == (FIELDK, 3, 3)
            e.run(STEPS)
            assert np.array_equal(e.download(), reference(O, H, W, STEPS))


# ---- 8. at size: the auto rule in a chain ----------------------------------------------------------
def hash_rows(row0, n, W):
    """Rows [row0, row0 + n) of tests/test_gpu_field_large.py's hash_field: a quarter of the
    cells exactly 0.0, 3 % exactly 1.0, the others uniform in [0, 0.5)."""
    x = (np.arange(row0, row0 + n, dtype=np.uint64)[:, None] * np.uint64(0x9E3779B97F4A7C15) +
         np.arange(W, dtype=np.uint64)[None, :] * np.uint64(0xC2B2AE3D27D4EB4F))
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(32)
    pick = x >> np.uint64(56)
    f = ((x >> np.uint64(3)) & np.uint64((1 << 52) - 1)).astype(np.float64) * 2.0 ** -53
    f[pick < 64] = 0.0
    f[pick >= 248] = 1.0
    return f


def test_auto_rule_in_a_chain_at_size(gpu, O, monkeypatch):
    H, W, G, steps, band = 4096, 2048, 2, 4, 64  # slabs of 2^22 cells
    engines = chain(gpu, monkeypatch, H, W, G, MM_FIELD_HALO=HALO)
    try:
        for e in engines:
            e.fill_random(0)
            lo, hi = max(e.x_init - HALO, 0), min(e.x_init + e.h + HALO, H)
            e.rate_field_upload(hash_rows(lo, hi - lo, W), row0=lo - e.x_init)
            e.add_diffuse_field(0)
            info = e.info()
            assert plan_of(e) == (FIELDK, 4, 4), info
            assert e.h >= 2 * 4 + 1 and 16 <= info["rows_per_wave"] < e.h, info
        assert engines[0].pass_plan(steps) == [4]
        assert run_chain(engines, steps) == 4
        seam = engines[1].x_init
        for b in (0, seam - band // 2, H - band):
            # the oracle weighs the first and last row it is given as grid edges: the band is
            # widened by its cone of steps + 1 rows (tests/test_gpu_field_large.py)
            lo, hi = max(0, b - steps - 1), min(H, b + band + steps + 1)
            v, f, cnt = O.fill_random(H, W, lo, hi - lo), hash_rows(lo, hi - lo, W), \
                neighbour_counts(hi - lo, W)
            for _ in range(steps):
                v = oracle_step(O, v, f, cnt)
            want = v[b - lo:b - lo + band]
            got = np.vstack([e.read_rows(max(b, e.x_init) - e.x_init,
                                         min(b + band, e.x_init + e.h) - max(b, e.x_init))
                             for e in engines if b < e.x_init + e.h and b + band > e.x_init])
            rows = np.flatnonzero(np.any(got != want, axis=1)) + b
            assert rows.size == 0, (b, rows[:8].tolist(), int(np.count_nonzero(got != want)))
    finally:
        close(engines)
