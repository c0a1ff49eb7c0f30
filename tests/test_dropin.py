"""Drop-in tests: Main.cpp-style MPI programs built against mpi-model_amd/api/ run on
the GPU under mpirun, and their output files are compared with the reference's.

* oracle/_ref/dropin_ref_main is the reference's own src/Main.cpp, UNCHANGED, compiled
  against our headers (mpi-model_amd/api/Makefile; built only where the reference lies. It
  finds the engine relative to its own path or through engine_env below, so it runs
  wherever oracle/_ref/ comes along with the tree; without it these runs use examples/drop_in_main alone; the CPU test
  tests/test_abi.py::test_reference_main_compiles_and_links_unchanged compiles and links it).
* examples/drop_in_main.cpp is our Main.cpp-style program.
The reference writes ../output/comm_rank%d.txt per worker plus a merged file
(src/Model.hpp:97-131,245-260); golden sha256s come from the reference itself
(tests/golden/c1_default_text.json).
"""
import glob
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden

pytestmark = pytest.mark.gpu

MPIRUN = os.environ.get("MPIRUN", "/opt/conda/bin/mpirun")


def engine_env(env=None):
    """The tests' environment with this tree's engine on the loader's path: a program
    reaches libmpimodel_hip.so through its own RPATH where it was built in place, and
    through this where it was built elsewhere and came along with oracle/_ref/ (a copied or
    linked directory, whose $ORIGIN is not this tree)."""
    e = dict(os.environ)
    e.update(env or {})
    e["LD_LIBRARY_PATH"] = os.pathsep.join(
        [os.path.join(REPO, "mpi-model_amd")] + [p for p in [e.get("LD_LIBRARY_PATH")] if p])
    return e


def run_mpi(tmp_path, binary, np_, args=(), timeout=120, env=None):
    run = tmp_path / "run"
    out = tmp_path / "output"
    run.mkdir()
    out.mkdir()
    e = engine_env(env)
    p = subprocess.run([MPIRUN, "-np", str(np_), binary] + [str(a) for a in args], cwd=run,
                       capture_output=True, text=True, timeout=timeout, env=e)
    assert p.returncode == 0, p.stdout + p.stderr
    files = {os.path.basename(f): open(f, "rb").read() for f in glob.glob(str(out / "*"))}
    return p.stdout, files


def binaries():
    out = []
    ref = os.path.join(REPO, "oracle", "_ref", "dropin_ref_main")
    if os.path.exists(ref):
        out.append(ref)
    out.append(os.path.join(REPO, "examples", "drop_in_main"))
    return out


@pytest.mark.parametrize("binary", binaries(), ids=os.path.basename)
def test_default_run_matches_reference_output_files(tmp_path, binary):
    g = golden("c1_default_text.json")
    stdout, files = run_mpi(tmp_path, binary, 6)
    for name, want in g["rank_files"].items():
        assert hashlib.sha256(files[name]).hexdigest() == want["sha256"], name
    merged = [v for k, v in files.items() if k.startswith("output ")]
    assert len(merged) == 1
    assert hashlib.sha256(merged[0]).hexdigest() == g["concat_sha256"]
    for line in ["1|19:3|0.100000", "19 3 8", "1: 0.22"]:
        assert line in stdout


@pytest.mark.parametrize("np_", [1, 2, 3])
def test_default_run_other_layouts(tmp_path, np_):
    # one process (master = only worker), 1 and 2 workers: same cells, same bytes in order.
    # np 2 is BASELINE.json configs[0] ("mpirun -np 2"), where the reference itself
    # overflows its static cell array
    g = golden("c1_default_text.json")
    _, files = run_mpi(tmp_path, os.path.join(REPO, "examples", "drop_in_main"), np_)
    ranks = sorted(k for k in files if k.startswith("comm_rank"))
    assert len(ranks) == max(np_ - 1, 1)
    cat = b"".join(files[k] for k in sorted(ranks, key=lambda s: int(s[9:-4])))
    assert hashlib.sha256(cat).hexdigest() == g["concat_sha256"]


def test_reference_main_at_np2(tmp_path):
    # the reference's own src/Main.cpp, unchanged, over our headers at BASELINE.json
    # configs[0]'s layout: one worker owns the whole grid
    ref = os.path.join(REPO, "oracle", "_ref", "dropin_ref_main")
    if not os.path.exists(ref):
        pytest.skip("dropin_ref_main is built only where /root/reference exists")
    g = golden("c1_default_text.json")
    stdout, files = run_mpi(tmp_path, ref, 2)
    assert sorted(k for k in files if k.startswith("comm_rank")) == ["comm_rank1.txt"]
    assert hashlib.sha256(files["comm_rank1.txt"]).hexdigest() == g["concat_sha256"]
    assert "1|19:3|0.100000" in stdout


def mpi_sends(stderr):
    out = {}
    for ln in stderr.splitlines():
        if ln.startswith("MPISEND "):
            f = dict(kv.split("=", 1) for kv in ln[8:].split(" ", 5))
            out.setdefault(int(f["src"]), []).append(
                [int(f["dest"]), int(f["tag"]), f["type"], int(f["count"]), f["data"]])
    return out


def run_logged(tmp_path, binary, np_, args=()):
    run = tmp_path / "run"
    out = tmp_path / "output"
    run.mkdir()
    out.mkdir()
    p = subprocess.run([MPIRUN, "-np", str(np_), binary] + [str(a) for a in args], cwd=run,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    files = {os.path.basename(f): open(f, "rb").read() for f in glob.glob(str(out / "*"))}
    return p.stdout, mpi_sends(p.stderr), files


def test_dropin_control_messages_match_reference(tmp_path):
    # the drop-in driver speaks the reference's wire protocol: the master's 23-char
    # partition / flow descriptors (src/Model.hpp:70-86) and the workers' sums and file
    # names (src/Model.hpp:243,260), against the reference's own traffic
    # (tests/golden/wire_row_100_100_5_0.json, recorded from the reference binary)
    g = golden("wire_row_100_100_5_0.json")
    binary = os.path.join(REPO, "oracle", "_build", "dropin_wire_main")
    stdout, sends, _ = run_logged(tmp_path, binary, g["np"])
    ref = g["sends_by_rank"]
    want = [m for m in ref["0"] if m[2] == "char"]
    got = [m for m in sends[0] if m[2] == "char" and m[1] in (0, 999)]
    assert got == want
    for k in range(1, g["np"]):
        rs = [m for m in ref[str(k)] if m[0] == 0]  # worker -> master: sum, file name
        gs = [m for m in sends[k] if m[0] == 0 and m[1] == k]
        assert [m[:4] for m in gs] == [m[:4] for m in rs], k
        a, b = float.fromhex(gs[0][4]), float.fromhex(rs[0][4])
        assert abs(a - b) <= 1e-12 * b  # slab sums: device reduction vs serial loop
        assert gs[1][4] == rs[1][4]  # "../output/comm_rank<k>.txt"
    for line in g["reference_stdout_lines"]:
        assert line in stdout


def test_rect_model_matches_reference(tmp_path):
    # ModelRectangular (src/ModelRectangular.hpp:52-272) on the reference's defaults
    # (20 x 60 cells, 2 x 3 blocks, -np 7, source (18,19)): the same block descriptors and
    # flow descriptor on the wire, the same printed lines, no result files (as the
    # reference); MPI_Report carries the descriptors and the owner
    import json
    g = golden("wire_rect_20_60_2_3_2.json")
    binary = os.path.join(REPO, "oracle", "_build", "rect_wire_main")
    stdout, sends, files = run_logged(tmp_path, binary, g["np"])
    want = [m for m in g["sends_by_rank"]["0"] if m[2] == "char"]
    got = [m for m in sends[0] if m[2] == "char" and m[1] in (0, 999)]
    assert got == want
    lines = stdout.splitlines()
    owner = int(want[-1][4].split("|")[0])
    # ranks share one stdout pipe and write a line in pieces, so two ranks' lines can
    # interleave: count occurrences in the whole text, not whole lines
    assert stdout.count(f"{want[-1][4]} {owner}") == 1         # master, :88
    assert stdout.count(want[-1][4]) == g["np"]                # + every worker, :158
    assert f"{owner}: 0.22" in stdout                          # the owner, :180
    assert not files
    rep = json.loads([ln for ln in lines if ln.startswith("{")][-1])
    assert rep["owner"] == owner
    descs = [[int(t) for t in m[4].replace(":", "|").split("|")] for m in want if m[1] == 0]
    assert rep["blocks"] == descs
    # the point flow itself changes no total
    assert float.fromhex(rep["final_sum"]) == 20 * 60


@pytest.mark.parametrize("np_", [1, 3, 4])
def test_whole_grid_flow_program(tmp_path, O, np_):
    # Exponencial(rate) on every cell, 51 steps (time 10, dt 0.2: src/Model.hpp:47-51);
    # workers sharing the one GPU exchange border rows through MPI (MM_HALO_HOST)
    import json
    H, W = 100, 100
    stdout, files = run_mpi(tmp_path, os.path.join(REPO, "examples", "grid_flow_main"), np_,
                            [H, W, 10.0, 0.2, 0.1])
    rep = json.loads([ln for ln in stdout.splitlines() if ln.startswith("{")][-1])
    assert rep["steps"] == 51
    v = np.ones((H, W))
    sums = []
    for _ in range(51):
        v = O.field_step(v, 0.1)
        sums.append(math.fsum(v.ravel()))
    got = [float.fromhex(s) for s in rep["sums"]]
    assert len(got) == 51
    for a, b in zip(got, sums):
        assert abs(a - b) <= 1e-12 * b
    lines = []
    for k in sorted((k for k in files if k.startswith("comm_rank")), key=lambda s: int(s[9:-4])):
        lines.extend(files[k].decode().splitlines())
    want = [f"{x}\t{y}\t{v[x, y]:g}" for x in range(H) for y in range(W)]
    assert lines == want


@pytest.mark.parametrize("H,W,sx,sy,fits", [
    (1000, 1000, 999, 500, True),       # "10|999:500|0.100000": fits the 23-byte message
    (20000, 10001, 19999, 10000, False),  # "10|19999:10000|0.100000": one byte too long
])
def test_point_flow_many_workers_wire_limit(tmp_path, H, W, sx, sy, fits):
    # 10 workers and 5-digit coordinates: the flow descriptor no longer fits the
    # reference's 23-char message (src/Model.hpp:81,85). That is a limit of the wire format,
    # not of the run: the message goes out as NUL bytes, every rank uses its own owner and
    # partition, rank 0 warns once, and the flow is applied and conserved as usual
    import json
    stdout_err = []
    run = tmp_path / "run"
    out = tmp_path / "output"
    run.mkdir()
    out.mkdir()
    env = dict(os.environ)
    env["MM_WRITE_OUTPUT"] = "0"
    p = subprocess.run([MPIRUN, "-np", "11", os.path.join(REPO, "examples", "point_flow_main"),
                        str(H), str(W), str(sx), str(sy), "2.2", "0.1"], cwd=run,
                       capture_output=True, text=True, timeout=240, env=env)
    stdout_err.append(p.stdout + p.stderr)
    assert p.returncode == 0, stdout_err[0][-3000:]
    rep = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert rep["owner"] == sx // (H // 10) + 1 == 10  # src/Model.hpp:80
    assert float.fromhex(rep["final_sum"]) == pytest.approx(H * W, rel=1e-12)
    assert len(rep["blocks"]) == 10
    assert rep["blocks"][9] == [9 * (H // 10), 0, H // 10, W]
    warned = "does not fit the reference's 23-byte message" in p.stderr
    assert warned == (not fits)
