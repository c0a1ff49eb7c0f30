"""CPU: the engine model of tests/engine_model.py must not be the thing that is wrong.

The model is what tests/test_gpu_lifetime.py holds an engine against over a scripted life, so
it is checked on its own first: a split run equals a whole one, it reproduces the expected
states of three single-program GPU tests computed as those tests compute them, every script
the GPU tests run keeps every cell finite and >= 0 and every sum > 0 (then the project's
1e-12 * |sum| bound on the step sums means something: sum v = sum |v|), the random scripts
have the mix of ops they promise, and every entry point of the ABI is either driven by the
scripts or listed with a reason.
"""
import math

import numpy as np
import pytest

import engine_model as M
from test_gpu_padding import C5_FLOWS
from test_gpu_ratefield import neighbour_counts, oracle_step, random_field


def flows_into(m, flows):
    for method, args in M.program(flows, clear=False):
        getattr(m, method)(*args)


@pytest.mark.parametrize("reduce_every", [0, 1, 2, 3, 5])
@pytest.mark.parametrize("a,b", [(1, 1), (2, 5), (7, 8), (3, 17), (16, 1)])
def test_split_run_equals_whole_run(O, reduce_every, a, b):
    H, W = 9, 129
    models = []
    for parts in ((a, b), (a + b,), (1,) * (a + b)):
        m = M.EngineModel(O, H, W, 2)
        m.fill_random(0)
        m.fill_random(1, M.SEED + 1)
        m.rate_field_upload(random_field(H, W), 1)
        flows_into(m, [M.T(0, 1, 0.05), M.F(1), M.D(0, 0.2)])
        m.run(4, reduce_every)  # a phase that is not 0
        for n in parts:
            m.run(n, reduce_every)
        models.append(m)
    want = models[1]
    n = 4 + a + b
    assert want.steps_done == n
    assert len(want.hist) == (n // reduce_every if reduce_every else 0)
    for m in models:
        assert m.steps_done == n
        for x in range(2):
            assert m.v[x].tobytes() == want.v[x].tobytes()
        assert m.hist == want.hist  # entry for entry, bit for bit


def test_fill_resets_the_phase_and_keeps_the_history(O):
    m = M.EngineModel(O, 5, 7, 2)
    m.fill_random(0)
    m.fill_random(1)
    m.add_diffuse(0, 0.1)
    m.run(3, 2)  # step 2
    assert (m.steps_done, len(m.hist)) == (3, 1)
    m.run(1, 2)  # step 4
    assert len(m.hist) == 2
    m.fill(1, value=1.0)
    assert (m.steps_done, len(m.hist)) == (0, 2)
    m.run(1, 2)  # step 1 again
    assert len(m.hist) == 2
    m.rate_field_fill(0.1, 0)
    m.clear_flows()
    m.add_diffuse(0, 0.2)
    m.prepare(8, 1)
    m.set_timing(True)
    assert (m.steps_done, len(m.hist)) == (1, 2)
    m.clear_history()
    assert (m.steps_done, len(m.hist)) == (1, 0)


def test_partial_field_upload(O):
    H, W = 6, 4
    m = M.EngineModel(O, H, W)
    m.rate_field_upload(np.full((3, W), 0.25), 0, row0=-2)  # rows -2, -1 lie outside the grid
    want = np.zeros((H, W))
    want[0] = 0.25
    assert np.array_equal(m.f[0], want)
    m.rate_field_upload(np.full((4, W), 0.5), 0, row0=4)  # rows 6, 7 too
    want[4:] = 0.5
    assert np.array_equal(m.f[0], want)


def test_reproduces_uniform_diffusion(O):
    # tests/test_gpu_padding.py::test_nan_padding_changes_nothing
    H, W, steps = 37, 130, 23
    m = M.EngineModel(O, H, W)
    m.fill_random(0)
    m.add_diffuse(0, 0.1)
    m.run(steps, 1)
    ref, want = O.fill_random(H, W), []
    for _ in range(steps):
        ref = O.field_step(ref, 0.1)
        want.append(math.fsum(ref.ravel()))
    assert m.v[0].tobytes() == ref.tobytes()
    assert [h[0] for h in m.hist] == want


def test_reproduces_the_ring_program(O):
    # tests/test_gpu_padding.py::test_nan_padding_four_attributes
    H, W, steps = 37, 130, 9
    m = M.EngineModel(O, H, W, 4)
    for a in range(4):
        m.fill_random(a, O.SEED + a)
    flows_into(m, C5_FLOWS)
    assert m.flows == [tuple(f) for f in C5_FLOWS] == M.RING
    m.run(steps, 1)
    fields = [O.fill_random(H, W, seed=O.SEED + a) for a in range(4)]
    want, sums = O.program_step(fields, C5_FLOWS, steps=steps, sums_per_step=True)
    for a in range(4):
        assert m.v[a].tobytes() == want[a].tobytes(), a
    for s in range(steps):
        for a in range(4):
            assert abs(m.hist[s][a] - sums[s][a]) <= 1e-12 * abs(sums[s][a]), (s, a)


def test_reproduces_the_three_pass_program(O):
    # tests/test_gpu_ratefield.py::test_field_pass_between_other_passes
    H, W, steps = 27, 257, 6
    fields = [O.fill_random(H, W, seed=O.SEED + a) for a in range(3)]
    f, cnt = random_field(H, W), neighbour_counts(H, W)
    m = M.EngineModel(O, H, W, 3)
    for a in range(3):
        m.upload(fields[a], a)
    m.rate_field_upload(f, attr=1)
    m.add_transfer(0, 1, 0.05)
    m.add_diffuse_field(1)
    m.add_diffuse(2, 0.2)
    m.run(steps)
    for _ in range(steps):
        fields = O.program_step(fields, [(O.TRANSFER, 0, 1, 0.05)])
        fields[1] = oracle_step(O, fields[1], f, cnt)
        fields = O.program_step(fields, [(O.DIFFUSE, 2, 2, 0.2)])
    for a in range(3):
        assert m.v[a].tobytes() == fields[a].tobytes(), a


SCRIPTS = M.all_scripts()


@pytest.mark.parametrize("name,cfg,script", SCRIPTS, ids=[s[0] for s in SCRIPTS])
def test_scripts_keep_the_state_positive(O, name, cfg, script):
    def positive(i, m):
        if script[i][0] not in M.STATE_OPS:
            return
        for a, v in enumerate(m.v):
            assert np.all(np.isfinite(v)) and np.all(v >= 0.0), (name, i, script[i], a)
        if script[i][0] == "run":
            assert all(s > 0.0 for s in m.sums()), (name, i, script[i])

    n_attr = cfg[0]
    for method, args in script:
        # the generator's ranges (what the positivity rests on)
        if method == "add_diffuse":
            assert 0.0 <= args[1] <= 0.5
        elif method == "add_transfer":
            assert 0.0 < args[2] <= 0.3 and args[0] != args[1] and args[1] < n_attr
        elif method == "rate_field_fill":
            assert 0.0 <= args[0] <= 0.5
        elif method == "point_apply":
            assert args[2] is None and 0.0 <= args[3] <= 0.5
        elif method == "run":
            assert args[0] in M.RUN_LENGTHS and args[1] in M.REDUCE_EVERY
    m = M.run_model(O, cfg, script, positive)
    assert all(x > 0.0 for row in m.hist for x in row)
    assert len(m.hist) <= 4096 or name == "history-growth"


def program_changes(script, n_attr):
    """Program changes after the set-up: every clear_flows, and every group of add_* calls
    that follows an op of another kind."""
    n, prev = 0, None
    for method, _ in script[n_attr:]:
        if method == "clear_flows" or (method in M.PROGRAM_OPS and prev not in M.PROGRAM_OPS):
            n += 1
        prev = method
    return n - 1  # the first group is the set-up's program


@pytest.mark.parametrize("n_attr", [1, 3, 4])
@pytest.mark.parametrize("seed", M.SEEDS)
def test_random_scripts_hold_what_they_promise(seed, n_attr):
    rng = np.random.default_rng([seed, n_attr])
    script = M.gen_script(rng, n_attr)
    again = M.gen_script(np.random.default_rng([seed, n_attr]), n_attr)
    assert script == again  # the seed alone decides the script
    classes = [M.op_class(m) for m, _ in script[n_attr:]]
    assert 6 <= classes.count("run") <= 10
    assert 2 <= program_changes(script, n_attr) <= 4
    for c in ("state", "field", "point", "history", "hint"):
        assert classes.count(c) >= 1, c
    # a field program runs only once its field exists
    have, flows = set(), []
    for method, args in script:
        if method in ("rate_field_upload", "rate_field_fill"):
            have.add(args[1])
        elif method == "clear_flows":
            flows = []
        elif method == "add_diffuse_field":
            flows.append(args[0])
        elif method in ("run", "prepare"):
            assert set(flows) <= have, (method, args)


def test_every_entry_point_is_sequenced_or_listed(mm):
    called = set(M.RUNNER_CALLS)
    for _, _, script in SCRIPTS:
        called.update(method for method, _ in script)
    called -= {M.REFUSE, M.CACHED_RUN}  # refused calls and a run, of methods counted anyway
    assert called <= set(M.EXPORT_OF), called - set(M.EXPORT_OF)
    sequenced = {M.EXPORT_OF[m] for m in called}
    listed = set(M.NOT_SEQUENCED)
    assert not sequenced & listed, sequenced & listed
    assert sequenced | listed == set(mm.EXPORTS), set(mm.EXPORTS) ^ (sequenced | listed)
    assert all(reason for reason in M.NOT_SEQUENCED.values())
    # the model answers every method a script may call
    for method in called - {"info", "synchronize", "pass_plan", "pass_kernel", "timing"}:
        assert callable(getattr(M.EngineModel, method)), method
