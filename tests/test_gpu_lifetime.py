"""GPU: one engine over a long, reprogrammed life, against a CPU model of the ABI.

Every other GPU test builds an engine, gives it one program, runs and compares. The engine is
a hand-maintained state machine -- ping-pong parity, reduction phase, a graph cache keyed by
(parity, length, reduce_every, phase) whose graphs hold captured pointers and rates, a planner
view re-derived from the passes by hand -- and a missed invalidation shows only on the second
program of an engine's life. Here a script (tests/engine_model.py: a list of (method, args))
is applied to an engine and to the model side by side, twice:
  checked       after every state-changing op every attribute's download equals the model's
                bitwise, and sums() and the whole sums_history() are within 1e-12 * |want|;
  free-running  nothing is read until the end of the script, so runs, point applications,
                field uploads and reprogramming follow each other with no synchronising read;
                then the same comparison once.
At the end steps_done and hist_entries equal the model's. After every program change (checked
mode) and at the end (both modes) the engine must plan as a fresh engine of the same shape and
creation environment given only the current flow list does (include/mpimodel.h,
mm_clear_flows): the same mm_info planning fields, pass plans and pass kernels.
"""
import numpy as np
import pytest

import engine_model as M
from test_gpu_ratefield import make_chain, run_chain

pytestmark = pytest.mark.gpu

MODES = ["checked", "free"]
PLAN_INFO = ("kernel", "steps_per_launch", "halo_depth", "n_passes", "rows_per_wave",
             "waves_per_pass", "fused_attrs", "chain_kernel", "seg_waves_per_cu")
PLAN_STEPS = (1, 7, 20, 45)


def make_engine(gpu, monkeypatch, cfg):
    n_attr, env, (H, W) = cfg
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return gpu.Engine(H, W, n_attr=n_attr)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def plan_facts(e, with_plans):
    info = e.info()
    facts = {"info": {k: info[k] for k in PLAN_INFO}}
    if with_plans:  # mm_pass_plan needs a program
        facts["plans"] = {n: e.pass_plan(n) for n in PLAN_STEPS}
        facts["kernels"] = {k: e.pass_kernel(k)
                            for k in sorted({k for p in facts["plans"].values() for k in p})}
    return facts


def fresh_facts(gpu, monkeypatch, cfg, m):
    """What a fresh engine plans for the model's current program."""
    with make_engine(gpu, monkeypatch, cfg) as f:
        for a in m.field_attrs():
            f.rate_field_fill(0.0, a)
        for method, args in M.program(m.flows, clear=False):
            M.apply_op(f, method, args)
        return plan_facts(f, bool(m.flows))


def mismatch(e, m):
    """The first difference between the engine and the model, or None."""
    for a in range(m.n_attr):
        got = e.download(a)
        if got.tobytes() != m.v[a].tobytes():
            bad = np.argwhere(got != m.v[a])
            at = tuple(bad[0]) if len(bad) else "sign of zero / NaN payload"
            return f"attribute {a}: {len(bad)} cells differ, first at {at}"
    got, want = e.sums(), m.sums()
    for a in range(m.n_attr):
        if not abs(got[a] - want[a]) <= 1e-12 * abs(want[a]):
            return f"sums()[{a}] = {got[a]!r}, model {want[a]!r}"
    got, want = e.sums_history(), m.sums_history()
    if got.shape != want.shape:
        return f"history of {got.shape[0]} entries, model {want.shape[0]}"
    bad = np.argwhere(~(np.abs(got - want) <= 1e-12 * np.abs(want)))
    if len(bad):
        i, a = bad[0]
        return f"history entry {i} attribute {a} = {got[i, a]!r}, model {want[i, a]!r}"
    return None


def play(gpu, monkeypatch, O, cfg, script, mode, label, after=None):
    """The script on an engine and on the model side by side; after(i, engine, model) runs
    after entry i. Returns the model."""
    n_attr, _, (H, W) = cfg
    checked = mode == "checked"
    m = M.EngineModel(O, H, W, n_attr)

    def where(i):
        return (f"{label} [{M.config_id(cfg)}, {mode}]: first mismatch at op {i} "
                f"{script[i]!r}\nscript up to it:\n{M.format_script(script[:i + 1])}\n")

    def same_plans(i):
        got, want = plan_facts(e, bool(m.flows)), fresh_facts(gpu, monkeypatch, cfg, m)
        assert got == want, where(i) + f"plans as {got}\na fresh engine as {want}"

    with make_engine(gpu, monkeypatch, cfg) as e:
        for i, (method, args) in enumerate(script):
            if method == M.REFUSE:
                count = e.info()["graph_count"]
                with pytest.raises(gpu.MMError):
                    M.apply_op(e, args[0], M.materialize(args[0], args[1], m))
                assert e.info()["graph_count"] == count, where(i)
            elif method == M.CACHED_RUN:
                count = e.info()["graph_count"]
                m.run(*args)
                e.run(*args)
                assert e.info()["graph_count"] == count, where(i) + "the run's graph was dropped"
            else:
                call = M.materialize(method, args, m)
                M.apply_op(m, method, call)
                M.apply_op(e, method, call)
            if after:
                after(i, e, m)
            if not checked:
                continue
            if method in M.STATE_OPS or method in (M.REFUSE, M.CACHED_RUN):
                bad = mismatch(e, m)
                assert bad is None, where(i) + bad
            if method in M.PROGRAM_OPS and (i + 1 == len(script) or
                                            script[i + 1][0] not in M.PROGRAM_OPS):
                same_plans(i)
        last = len(script) - 1
        if not checked:
            e.synchronize()
        bad = mismatch(e, m)
        assert bad is None, where(last) + bad
        info = e.info()
        assert (info["steps_done"], info["hist_entries"]) == (m.steps_done, len(m.hist)), where(last)
        same_plans(last)
    return m


def scripted(configs):
    """Parametrisation of one hand-written scenario over its environments and both modes."""
    def deco(fn):
        fn = pytest.mark.parametrize("mode", MODES)(fn)
        return pytest.mark.parametrize("cfg", configs, ids=M.config_id)(fn)
    return deco


# ---- a. program A, then B, then A again -------------------------------------------------------
@scripted(M.CONFIGS)
def test_reprogrammed_engine(gpu, O, monkeypatch, cfg, mode):
    n_attr, _, (H, W) = cfg
    script, A = M.script_aba(n_attr, H, W)
    m = play(gpu, monkeypatch, O, cfg, script, mode, "aba")
    # the script ends with a refill and program A: a fresh engine given only that
    with make_engine(gpu, monkeypatch, cfg) as f:
        for method, args in M.fills(n_attr) + M.program(A, clear=False) + [script[-1]]:
            M.apply_op(f, method, args)
        for a in range(n_attr):
            assert f.download(a).tobytes() == m.v[a].tobytes(), a


# ---- b. add_* after a run, without clear_flows ------------------------------------------------
@scripted(M.CONFIGS)
def test_incremental_program(gpu, O, monkeypatch, cfg, mode):
    play(gpu, monkeypatch, O, cfg, M.script_incremental(cfg[0], *cfg[2]), mode, "incremental")


# ---- c. rate fields over a lifetime -----------------------------------------------------------
@scripted(M.CONFIGS_1 + M.CONFIGS_3 + M.CONFIGS_4[:2])
def test_rate_fields_over_a_lifetime(gpu, O, monkeypatch, cfg, mode):
    play(gpu, monkeypatch, O, cfg, M.script_fields(cfg[0], *cfg[2]), mode, "fields")


# ---- d. reductions over a lifetime ------------------------------------------------------------
@scripted(M.CONFIGS)
def test_reductions_over_a_lifetime(gpu, O, monkeypatch, cfg, mode):
    play(gpu, monkeypatch, O, cfg, M.script_reductions(cfg[0], *cfg[2]), mode, "reductions")


def test_history_grows_past_its_first_capacity(gpu, O, monkeypatch):
    # 4109 entries against the 4096 the engine starts with; growing the history drops the
    # graphs that hold its address. Free-running: checked mode would read the history 128 times
    cfg = M.CONFIGS_1[0]
    script = M.script_history_growth(1, *cfg[2])

    def after(i, e, m):
        if i == len(script) - 2:  # the next run passes the capacity
            assert e.info()["hist_entries"] == len(m.hist) == 4064

    m = play(gpu, monkeypatch, O, cfg, script, "free", "history-growth", after)
    assert len(m.hist) == 4109


# ---- e. prepare and timing in mid-life --------------------------------------------------------
@scripted(M.CONFIGS)
def test_prepare_in_mid_life(gpu, O, monkeypatch, cfg, mode):
    play(gpu, monkeypatch, O, cfg, M.script_prepare(cfg[0], *cfg[2]), mode, "prepare")


@scripted(M.CONFIGS)
def test_timing_in_mid_life(gpu, O, monkeypatch, cfg, mode):
    script = M.script_timing(cfg[0], *cfg[2])
    timed = len(script) + M.TIMED_RUN
    assert script[timed - 1] == ("set_timing", (True,)) and script[timed][0] == "run"
    seen = []

    def after(i, e, m):
        if i == timed:
            info = e.info()
            per_step = info["n_passes"] if info["kernel"] == 0 else 1
            seen.append((e.timing()[0], len(e.pass_plan(script[i][1][0])) * per_step))

    play(gpu, monkeypatch, O, cfg, script, mode, "timing", after)
    assert len(seen) == 1 and seen[0][0] == seen[0][1], seen


# ---- f. point_apply between runs --------------------------------------------------------------
@scripted(M.CONFIGS)
def test_point_apply_between_runs(gpu, O, monkeypatch, cfg, mode):
    play(gpu, monkeypatch, O, cfg, M.script_points(cfg[0], *cfg[2]), mode, "points")


# ---- g. refusals leave no trace ---------------------------------------------------------------
@scripted(M.CONFIGS)
def test_refusals_leave_no_trace(gpu, O, monkeypatch, cfg, mode):
    play(gpu, monkeypatch, O, cfg, M.script_refusals(cfg[0], *cfg[2]), mode, "refusals")


# ---- h. a host-transport chain reprogrammed in lockstep ---------------------------------------
@pytest.mark.parametrize("H,W,G", M.CHAIN_SHAPES)
def test_chain_reprogrammed_in_lockstep(gpu, O, monkeypatch, H, W, G):
    script = M.script_chain(1, H, W)
    m = M.EngineModel(O, H, W)
    engines = make_chain(gpu, monkeypatch, H, W, G, env=M.CHAIN_ENV)
    try:
        for i, (method, args) in enumerate(script):
            call = M.materialize(method, args, m)
            M.apply_op(m, method, call)
            if method == "run":
                depth = run_chain(engines, *call)
                # a fresh chain given only this program exchanges as deep
                fresh = make_chain(gpu, monkeypatch, H, W, G, env=M.CHAIN_ENV)
                try:
                    for f in fresh:
                        for a in m.field_attrs():
                            f.rate_field_fill(0.0, a)
                        for pm, pa in M.program(m.flows, clear=False):
                            M.apply_op(f, pm, pa)
                    facts = [plan_facts(f, True) for f in fresh]
                finally:
                    for f in fresh:
                        f.close()
                assert facts[0]["info"]["halo_depth"] == depth, (i, script[i])
                assert [plan_facts(e, True) for e in engines] == facts, (i, script[i])
                got = np.vstack([e.download() for e in engines])
                assert got.tobytes() == m.v[0].tobytes(), (i, script[i])
                tot = np.zeros(len(m.hist))
                for e in engines:  # rank order, as src/Model.hpp:89-92
                    hist = e.sums_history()
                    assert hist.shape == (len(m.hist), 1), (i, script[i])
                    tot = tot + hist[:, 0]
                want = m.sums_history()[:, 0]
                assert np.all(np.abs(tot - want) <= 1e-12 * np.abs(want)), (i, script[i])
                assert all(e.info()["steps_done"] == m.steps_done for e in engines)
            elif method == "rate_field_upload":
                f = call[0]  # the whole field: every slab gets its rows -1..h
                for e in engines:
                    lo, hi = max(e.x_init - 1, 0), min(e.x_init + e.h + 1, H)
                    e.rate_field_upload(f[lo:hi], row0=lo - e.x_init)
            else:
                for e in engines:
                    M.apply_op(e, method, call)
    finally:
        for e in engines:
            e.close()


# ---- seeded random scripts --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", M.SEEDS)
@pytest.mark.parametrize("cfg", M.CONFIGS, ids=M.config_id)
def test_random_script(gpu, O, monkeypatch, cfg, seed, mode):
    # no retry and no time-based seed: a failure names the seed, the first mismatching op and
    # the script up to it, ready to paste into a scripted test
    play(gpu, monkeypatch, O, cfg, M.random_script(cfg, seed), mode, f"seed {seed}")
