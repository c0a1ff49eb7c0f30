"""Rate-field diffusion (MM_FLOW_DIFFUSE_FIELD) without a GPU: the flow kind's value in the
header and the binding, and the planner's treatment of a program with a rate-field pass
(tests/plan_field_cli.cpp against mpi-model_amd/csrc/mm_plan.cpp, built with plain g++ the
way tests/test_plan.py builds its program)."""
import os
import re

from plan_build import REPO, build, run


def test_flow_kind_in_header_is_the_bindings(mm):
    text = open(os.path.join(REPO, "include", "mpimodel.h")).read()
    m = re.search(r"\bMM_FLOW_DIFFUSE_FIELD\s*=\s*(\d+)", text)
    assert m, "include/mpimodel.h has no MM_FLOW_DIFFUSE_FIELD"
    assert int(m.group(1)) == mm.MM_FLOW_DIFFUSE_FIELD == 3
    for name in ("mm_rate_field_upload", "mm_rate_field_fill"):
        assert name in mm.EXPORTS and hasattr(mm.lib(), name)
    for method in ("add_diffuse_field", "rate_field_upload", "rate_field_fill"):
        assert callable(getattr(mm.Engine, method))


def test_planner_runs_field_programs_one_step_per_pass(tmp_path):
    out = run(build(str(tmp_path / "plan_field_cli"), "plan_field_cli.cpp"))
    assert out.strip() == "ok", out[-3000:]
