"""The kernels on signed, zero, subnormal, huge and non-finite values, bit for bit against
the oracle.

Every other GPU test feeds the kernels fill_random's [1, 2) or a grid of 1.0: one binade of
positive normal doubles. Here every kernel family runs the six value classes of
tests/value_classes.py, each at its own rate (a negative one for `zeros`: only then does the
oracle produce -0 at all). What that shows and positive data cannot: a mask done by
arithmetic instead of a select (u * 0 is NaN for a non-finite u, and -0 for a negative one),
the sign of a zero, a pairing of the sums other than the contract's (81 binades and mixed
signs make it a gross error, not an ulp), a flush of subnormals, an overflow in an
intermediate, and -- with no oracle involved -- the dependency cone of the temporal
blocking: after s steps the non-finite cells must be exactly the cells within Chebyshev
distance s of a seed, across strip, segment, level and slab boundaries.

The non-finite seeds sit where the plan that actually runs has its seams (seed_positions).
Cells are compared with value_classes.assert_same_bits, step sums with assert_sum_close.
"""
import numpy as np
import pytest

import value_classes as vc
from test_gpu_halo import close, gather, make_chain, run_chain
from test_gpu_instances import FOUR, ONE, PASSK, SEG, WIDE, check_plan, out_cols
from test_gpu_parity import C5_FLOWS, WIDE_PROGRAMS, add_flows, make_env_engine
from test_gpu_ratefield import neighbour_counts, oracle_step, random_field

pytestmark = pytest.mark.gpu

ONESTEP = 0  # mm_info.kernel of the one-step kernels (128-column strips)

_refs = {}


def reference(key, start, step, steps):
    """Oracle states after 0..steps steps of `start` (a list of attribute grids), computed
    once per key and kept read-only."""
    states = _refs.setdefault(key, [start])
    while len(states) <= steps:
        nxt = step(states[-1])
        for f in nxt:
            f.setflags(write=False)
        states.append(nxt)
    return states


def seed_positions(shape, rows, strip, slab_rows=None):
    """Cells for the non-finite seeds on the seams of the plan that runs: segments of `rows`
    rows, strips of `strip` output columns, slabs of `slab_rows` rows. A seam the grid does
    not have is dropped."""
    H, W = shape
    pos = [(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0)]
    # nan, +inf and -inf are cycled over the list: the grid's first row, last row, first and
    # last column each get an infinity, not only a NaN -- a cell outside the grid that is
    # masked by u * 0 turns an infinity beside it into a NaN, and a NaN hides that
    pos += [(H // 4, 0), (H - H // 4 - 2, W - 1)]
    if W > strip:  # last cell of strip 0, first of strip 1, in an interior row
        pos += [(H // 3, strip - 1), (H // 3 + 3, strip)]
    if H > rows:  # last row of segment 0, first of segment 1, in an interior column
        pos += [(rows - 1, W // 3), (rows, W // 3 + 3)]
    if W > 2 * strip and H > 4:  # deep inside an interior strip
        pos.append((H - H // 4, strip + strip // 2))
    if slab_rows:  # last owned row of slab 0, first owned row of slab 1
        pos += [(slab_rows - 1, W // 5), (slab_rows, W - W // 5)]
    out = []
    for x, y in pos:
        if 0 <= x < H and 0 <= y < W and (x, y) not in out:
            out.append((x, y))
    return tuple(out)


def check_cells(cls, got, want, pos, steps, what):
    for a, (g, w) in enumerate(zip(got, want)):
        vc.assert_same_bits(g, w, (what, cls, steps, a))
    if cls == "nonfinite" and len(got) == 1:
        # the dependency cone, with no oracle: one cell per step, in every direction
        ball = vc.ball_mask(got[0].shape, pos, steps)
        assert np.array_equal(~np.isfinite(got[0]), ball), (what, steps)


def check_sums(cls, hist, states, what):
    """hist[s]: the kernels' sums after step s + 1 (all slabs added up by the caller)."""
    assert hist.shape == (len(states) - 1, len(states[0])), (what, cls, hist.shape)
    for s in range(hist.shape[0]):
        for a, w in enumerate(states[s + 1]):
            if np.all(np.isfinite(w)):
                vc.assert_sum_close(hist[s, a], w, (what, cls, s, a))
            else:
                assert not np.isfinite(hist[s, a]), (what, cls, s, a, hist[s, a])


def diffusion_step(O, rate):
    return lambda fields: [O.field_step(fields[0], rate)]


def program_step(O, flows):
    return lambda fields: O.program_step(fields, list(flows), steps=1)


def run_engine(O, e, cls, start, states_of, runs, pos, what):
    """Upload `start`, run each of `runs` with per-step sums, compare after each."""
    for a, f in enumerate(start):
        e.upload(f, a)
    done = 0
    for n in runs:
        e.run(n, 1)
        done += n
        states = states_of(done)
        check_cells(cls, [e.download(a) for a in range(len(start))], states[done], pos, done, what)
    check_sums(cls, e.sums_history(), states[:done + 1], what)


# ---- one attribute, one diffusion: every kernel family and K ---------------------------------
ONE_CONFIGS = ([({"MM_PASSK": 0}, ONESTEP, 1, 2)]
               + [({"MM_WIDE": 0, "MM_STEPS_PER_PASS": k}, PASSK, k, 2) for k in (1, 2, 5, 10)]
               + [({"MM_WIDE": 1, "MM_STEPS_PER_PASS": k}, WIDE, k, 4) for k in (4, 8, 12, 16, 20)])


def config_id(c):
    return ",".join(f"{k[3:]}={v}" for k, v in c[0].items()) or "default"


@pytest.mark.parametrize("config", ONE_CONFIGS, ids=config_id)
def test_one_attribute_instances(gpu, O, monkeypatch, config):
    env, kernel, k, cols = config
    for cls in vc.CLASSES:
        rate = vc.RATES[cls]
        e = make_env_engine(gpu, monkeypatch, *ONE, **SEG, **env)
        try:
            e.add_diffuse(0, rate)
            info = e.info()
            if kernel == ONESTEP:
                assert (info["kernel"], info["steps_per_launch"]) == (ONESTEP, 1), info
                strip = 128
            else:
                check_plan(e, ONE, kernel, k, cols)
                assert e.pass_plan(k) == [k]
                strip = out_cols(kernel, k, cols)
            pos = seed_positions(ONE, info["rows_per_wave"], strip)
            assert cls != "nonfinite" or len(pos) >= 8, pos
            start = [vc.make(cls, *ONE, positions=pos)]
            key = ("one", cls, rate, pos)
            run_engine(O, e, cls, start,
                       lambda n: reference(key, start, diffusion_step(O, rate), n),
                       (k, 1), pos, env)  # one pass of K, then one more step
        finally:
            e.close()


# ---- four attributes: transfer chains around the diffusions ---------------------------------
def four_configs(gpu):
    return [({"MM_WIDE": 1, "MM_STEPS_PER_PASS": 4}, WIDE_PROGRAMS[3], WIDE, 4, gpu.MM_CHAIN_RUNTIME),
            ({"MM_WIDE": 1, "MM_CHAIN_RING": 1}, C5_FLOWS, WIDE, 8, gpu.MM_CHAIN_RING),
            ({"MM_WIDE": 1, "MM_CHAIN_RING": 0}, C5_FLOWS, WIDE, 8, gpu.MM_CHAIN_RUNTIME),
            ({"MM_WIDE": 1}, WIDE_PROGRAMS[1], WIDE, 8, gpu.MM_CHAIN_RUNTIME),
            ({"MM_WIDE": 0}, C5_FLOWS, PASSK, 2, gpu.MM_CHAIN_NONE)]


@pytest.mark.parametrize("n", range(5))
def test_four_attribute_instances(gpu, O, monkeypatch, n):
    env, flows, kernel, k, chain = four_configs(gpu)[n]
    for cls in vc.CLASSES:
        e = make_env_engine(gpu, monkeypatch, *FOUR, n_attr=4, **SEG, **env)
        try:
            add_flows(e, flows)
            info = e.info()
            if kernel == WIDE:
                check_plan(e, FOUR, kernel, k, 2, chain)
            else:
                assert (info["kernel"], info["steps_per_launch"]) == (kernel, k), info
                assert info["chain_kernel"] == chain, info
            assert e.pass_plan(k) == [k]
            pos = seed_positions(FOUR, info["rows_per_wave"], out_cols(kernel, k, 2))
            # the seeds go into attribute 0 only: the transfers carry them into the others
            start = [vc.make(cls, *FOUR, seed=a, positions=pos if a == 0 else ()) for a in range(4)]
            key = ("four", cls, n, pos)
            run_engine(O, e, cls, start,
                       lambda s: reference(key, start, program_step(O, flows), s),
                       (k, 1), pos, (env, n))
        finally:
            e.close()


# ---- the rate-field kernel: the class data is the state, the field is the rate --------------
@pytest.mark.parametrize("shape", [(27, 257), (9, 129)])
def test_rate_field_kernel(gpu, O, shape):
    f, cnt = random_field(*shape), neighbour_counts(*shape)
    for cls in vc.CLASSES:
        with gpu.Engine(*shape) as e:
            e.rate_field_upload(f)
            e.add_diffuse_field(0)
            info = e.info()
            assert (info["kernel"], info["steps_per_launch"]) == (ONESTEP, 1), info
            pos = seed_positions(shape, info["rows_per_wave"], 128)
            start = [vc.make(cls, *shape, positions=pos)]
            key = ("field", shape, cls, pos)
            run_engine(O, e, cls, start,
                       lambda n: reference(key, start, lambda v: [oracle_step(O, v[0], f, cnt)], n),
                       (1, 2), pos, shape)


# ---- slabs with a host halo: border launches, and slabs too thin to split -------------------
@pytest.mark.parametrize("shape,G,env", [
    (ONE, 2, {**SEG, "MM_WIDE": 0, "MM_STEPS_PER_PASS": 5}),
    (ONE, 2, {**SEG, "MM_WIDE": 1, "MM_STEPS_PER_PASS": 8}),
    ((16, 130), 8, {})], ids=["passk5", "wide8", "thin"])
def test_host_halo_chains(gpu, O, monkeypatch, shape, G, env):
    H, W = shape
    for cls in vc.CLASSES:
        rate = vc.RATES[cls]
        engines = make_chain(gpu, monkeypatch, H, W, G, env=env)
        try:
            for e in engines:
                e.add_diffuse(0, rate)
            info = engines[0].info()
            k = info["halo_depth"]
            assert k == min(env.get("MM_STEPS_PER_PASS", k), H // G), info
            kernel, cols, _ = engines[0].pass_kernel(k)
            if "MM_WIDE" in env:
                assert kernel == (WIDE if env["MM_WIDE"] else PASSK) and engines[0].h > 2 * k
            strip = 128 if kernel == ONESTEP else out_cols(kernel, k, cols)
            pos = seed_positions(shape, info["rows_per_wave"], strip, slab_rows=engines[0].h)
            start = vc.make(cls, H, W, positions=pos)
            states = reference(("chain", shape, cls, rate, pos), [start],
                               diffusion_step(O, rate), k + 1)
            for e in engines:
                e.upload(start[e.x_init:e.x_init + e.h])
            assert all(e.pass_plan(k) == [k] for e in engines)
            run_chain(engines, k, 1)
            check_cells(cls, [gather(engines)], states[k], pos, k, (shape, G))
            run_chain(engines, 1, 1)
            check_cells(cls, [gather(engines)], states[k + 1], pos, k + 1, (shape, G))
            hist = sum(e.sums_history() for e in engines)  # rank order, as src/Model.hpp:89-92
        finally:
            close(engines)
        check_sums(cls, hist, states[:k + 2], (shape, G))


# ---- grids of a few cells: the count classes 0, 1, 2, 3, 5 and the GEN-only strips ----------
SMALL = [(1, 1), (1, 9), (5, 1), (2, 2), (3, 5), (5, 130), (130, 9)]


@pytest.mark.parametrize("env", [{}, {"MM_WIDE": 0}, {"MM_PASSK": 0}],
                         ids=["default", "WIDE=0", "PASSK=0"])
@pytest.mark.parametrize("shape", SMALL)
def test_small_grids(gpu, O, monkeypatch, shape, env):
    for cls in vc.CLASSES:
        rate = vc.RATES[cls]
        e = make_env_engine(gpu, monkeypatch, *shape, **env)
        try:
            e.add_diffuse(0, rate)
            pos = seed_positions(shape, e.info()["rows_per_wave"], 128)
            start = [vc.make(cls, *shape, positions=pos)]
            key = ("small", shape, cls, rate, pos)
            run_engine(O, e, cls, start,
                       lambda n: reference(key, start, diffusion_step(O, rate), n),
                       (1, 3, 9), pos, (shape, env))
        finally:
            e.close()


# ---- the reference's single-source flow on a grid that is not 1.0 ----------------------------
@pytest.mark.parametrize("shape", [(24, 16), (37, 130)])
def test_point_apply_on_arbitrary_grid(gpu, O, shape):
    H, W = shape
    sources = [(0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, W - 1), (H // 2, W // 2)]
    for cls in ("signed", "wide", "zeros"):
        v = vc.make(cls, H, W)
        with gpu.Engine(H, W) as e:
            for sx, sy in sources:
                for captured in (v[sx, sy], -2.2):  # the source's own value; a constant
                    for rate in (0.1, -0.25):
                        want = O.point_apply(v, sx, sy, captured, rate)
                        e.upload(v)
                        e.point_apply(sx, sy, captured, rate)
                        what = (cls, sx, sy, captured, rate)
                        vc.assert_same_bits(e.download(), want, what)
                        vc.assert_sum_close(e.sums()[0], want, what)
