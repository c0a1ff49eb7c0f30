"""The engine describes its flow list to the planner through the host-only unit
(mpi-model_amd/csrc/mm_program.cpp): for each program, what a live engine reports -- passes per
step, the kernel and steps of a pass, the pass lengths of 7 steps, the kernel of a k-step pass
-- is what tests/program_cli.cpp prints for the same flows and MM_* environment on the CPU.
None of these depends on the device's occupancy, so they are compared exactly. Engines are
reprogrammed from list to list (mm_clear_flows), and every program runs 3 steps."""
import os

import numpy as np
import pytest

from plan_build import build, run
from test_gpu_lifetime import make_engine

pytestmark = pytest.mark.gpu

PRINT_K = (1, 2, 3, 4, 8, 20)  # program_cli.cpp kPrintK
FIVE = "T01 T12 T23 T30 T01"
# the flow lists of program_cli.cpp's kPassCases, by the attributes they need
PROGRAMS = {
    1: ["D0", "D0 D0", "F0 F0", "F0 D0", "D0 F0", "F0", "C0", "C0 C0", "D0 C0 D0"],
    4: ["D0", "D0 D0", "D0 D1", "T01 D0 T10", "T01 D0 T10 D1", FIVE, "D0 " + FIVE, "F0 F1", "F0 F0",
        "F0 D0", "D0 F0", "T01 F0", "C0", "F1 C0 F1", "C0 C0", "D0 C0 D0",
        "T01 T12 T23 T30 D0 D1 D2 D3"],
}


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("program") / "program_cli"), "program_cli.cpp")


def add(e, flows):
    for f in flows.split():
        attrs = [int(c) for c in f[1:]]
        if f[0] == "D":
            e.add_diffuse(attrs[0], 0.1)
        elif f[0] == "T":
            e.add_transfer(attrs[0], attrs[1], 0.05)
        else:
            e.rate_field_fill(0.1, attrs[0])
            (e.add_diffuse_field if f[0] == "F" else e.add_diffuse_closed)(attrs[0])


def engine_line(e):
    info = e.info()
    kernels = [x for k in PRINT_K for x in e.pass_kernel(k)]
    return " | ".join(" ".join(map(str, part)) for part in
                      ([info["n_passes"], info["kernel"], info["steps_per_launch"]], e.pass_plan(7), kernels))


def check_programs(gpu, monkeypatch, cli, shape, n_attr, programs, **env):
    H, W = shape
    with make_engine(gpu, monkeypatch, (n_attr, env, shape)) as e:
        # the environment the engine was created in, as the unit's stand-in for it
        knobs = [f"{k}={v}" for k, v in {**os.environ, **{k: str(v) for k, v in env.items()}}.items()
                 if k.startswith("MM_")]
        for a in range(n_attr):
            e.fill(a, value=1.0 + a)
        for flows in programs:
            e.clear_flows()
            assert e.info()["n_passes"] == 0
            add(e, flows)
            want = run(cli, "print", str(H), str(W), str(n_attr), *flows.split(), *knobs).strip()
            assert engine_line(e) == want, (flows, env)
            e.run(3)
            e.synchronize()
            assert engine_line(e) == want, (flows, env)  # a run changes no plan
            assert all(np.all(np.isfinite(e.download(a))) for a in range(n_attr)), flows
        assert e.info()["steps_done"] == 3 * len(programs)


@pytest.mark.parametrize("n_attr", [1, 4])
@pytest.mark.parametrize("shape", [(130, 97), (130, 257)])
def test_engine_reports_what_the_unit_plans(gpu, monkeypatch, cli, shape, n_attr):
    check_programs(gpu, monkeypatch, cli, shape, n_attr, PROGRAMS[n_attr])


@pytest.mark.parametrize("shape", [(130, 97), (130, 257)])
def test_reprogrammed_engine_fuses_closed_steps(gpu, monkeypatch, cli, shape):
    """MM_CLOSED_STEPS=3: [C0] alone fuses 3 steps per pass, before and after other programs."""
    programs = ["D0", "C0", "C0 C0", "F0", "C0", "D0 C0 D0", "C0"]
    check_programs(gpu, monkeypatch, cli, shape, 1, programs, MM_CLOSED_STEPS=3)
    with make_engine(gpu, monkeypatch, (1, {"MM_CLOSED_STEPS": 3}, shape)) as e:
        add(e, "C0")
        assert (e.info()["kernel"], e.info()["steps_per_launch"], e.pass_plan(7)) == (5, 3, [3, 2, 2])
        e.clear_flows()
        add(e, "C0 C0")
        assert (e.info()["kernel"], e.info()["steps_per_launch"], e.pass_plan(7)) == (0, 1, [1] * 7)
