"""Builds and runs the stand-alone C++ programs of tests/ (plan*_cli.cpp, program_cli.cpp)
against the host-only units of mpi-model_amd/csrc with plain g++: no ROCm headers, no GPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = [os.path.join(REPO, "mpi-model_amd", "csrc", name) for name in ("mm_plan.cpp", "mm_program.cpp")]
# ASan + UBSan with their runtimes linked statically into the stand-alone program
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
            "-static-libubsan")


def build(exe, cli, *flags):
    """Compile tests/<cli> and the host-only units into the program `exe`; returns exe."""
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", *flags,
                        os.path.join(REPO, "tests", cli), *UNITS, "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def run(exe, *args, input=None):
    """The program's output; it must exit 0."""
    r = subprocess.run([exe, *args], input=input, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout
