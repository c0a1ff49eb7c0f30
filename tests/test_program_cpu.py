"""The host-only unit between a flow list and the planner (mpi-model_amd/csrc/mm_program.cpp:
compile_passes, ring_program, set_program) without a GPU: tests/program_cli.cpp, built with
plain g++ and once more as a stand-alone program under ASan + UBSan. The pass structure of its
flow lists was recorded from the engine before the unit moved out of it."""
from plan_build import SANITIZE, build, run


def build_and_run(exe, *flags):
    out = run(build(exe, "program_cli.cpp", *flags))
    assert out.strip() == "ok", out[-3000:]
    return exe


def test_program_unit(tmp_path):
    exe = build_and_run(str(tmp_path / "program_cli"))
    # the print mode the GPU test compares an engine with: n_passes, kernel, steps per launch
    assert run(exe, "print", "130", "97", "1", "D0").split(" | ")[0] == "1 3 8"
    assert run(exe, "print", "130", "97", "1", "C0", "MM_CLOSED_STEPS=3").split(" | ")[:2] == ["1 5 3", "3 2 2"]


def test_program_unit_under_sanitizers(tmp_path):
    build_and_run(str(tmp_path / "program_cli_san"), *SANITIZE)
