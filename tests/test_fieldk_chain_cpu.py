"""K-step rate-field passes on slabs with a halo (MM_FIELD_HALO) without a GPU: the knob's
parsing, mm::field_k_for, the split plan of mm_fieldk_kernel (interior segments, K-row border
blocks, partials), the balanced pass lengths and the header's text
(tests/plan_fieldk_chain_cli.cpp against mpi-model_amd/csrc/mm_plan.cpp, built with plain g++
the way tests/test_fieldk_cpu.py builds its program, and once more under ASan + UBSan as a
stand-alone program)."""
import os

from plan_build import REPO, SANITIZE, build, run

HEADER = os.path.join(REPO, "include", "mpimodel.h")


def build_and_run(exe, *flags):
    out = run(build(exe, "plan_fieldk_chain_cli.cpp", *flags), HEADER)
    assert out.startswith("ok "), out[-3000:]
    return int(out.split()[1])  # the planner's kFieldMaxSteps


def test_planner_splits_field_passes(tmp_path, mm):
    assert build_and_run(str(tmp_path / "plan_fieldk_chain_cli")) == mm.FIELD_MAX_STEPS


def test_planner_under_sanitizers(tmp_path, mm):
    assert build_and_run(str(tmp_path / "plan_fieldk_chain_cli_san"), *SANITIZE) == mm.FIELD_MAX_STEPS


def test_header_names_the_knob():
    text = open(HEADER).read()
    env = text[text.index("Environment:"):text.index("int mm_engine_create(")]
    assert "MM_FIELD_HALO" in env and "lockstep" in env[env.index("MM_FIELD_HALO"):]
    upload = text[text.index("/* The rate field of attribute attr"):text.index("int mm_rate_field_upload(")]
    assert "MM_FIELD_HALO" in upload and "MM_ERR_STATE" in upload
