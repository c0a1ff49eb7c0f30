"""K-step rate-field passes (mm_fieldk_kernel, MM_FIELD_STEPS) without a GPU: the largest K in
the header and the binding, and the planner's treatment of a program whose rate-field passes
fuse K steps (tests/plan_fieldk_cli.cpp against mpi-model_amd/csrc/mm_plan.cpp, built with
plain g++ the way tests/test_ratefield_cpu.py builds its program, and once more under ASan +
UBSan as a stand-alone program the way tests/test_plan.py builds its own)."""
import os
import re

from plan_build import REPO, SANITIZE, build, run


def build_and_run(exe, *flags):
    out = run(build(exe, "plan_fieldk_cli.cpp", *flags))
    assert out.startswith("ok "), out[-3000:]
    return int(out.split()[1])  # the planner's kFieldMaxSteps


def header_max_steps():
    text = open(os.path.join(REPO, "include", "mpimodel.h")).read()
    m = re.search(r"^#define\s+MM_FIELD_MAX_STEPS\s+(\d+)", text, re.M)
    assert m, "include/mpimodel.h has no MM_FIELD_MAX_STEPS"
    assert "MM_FIELD_STEPS" in text.replace("MM_FIELD_MAX_STEPS", "")
    return int(m.group(1))


def test_max_steps_in_header_is_the_bindings(mm):
    assert header_max_steps() == mm.FIELD_MAX_STEPS >= 4


def test_planner_fuses_field_passes(tmp_path):
    assert build_and_run(str(tmp_path / "plan_fieldk_cli")) == header_max_steps()


def test_planner_under_sanitizers(tmp_path):
    assert build_and_run(str(tmp_path / "plan_fieldk_cli_san"), *SANITIZE) == header_max_steps()
