"""csrc/driving_vec.h on the CPU: the branch-free Driving-v1 step, reward and
observation key that k_search runs per lane, compiled for the host (vary() is
the identity there) into a stand-alone program with -fsanitize=address,undefined
and compared case by case, bit for bit, with the scalar functions of
csrc/driving.h (tests/native/driving_vec_check.cpp).  The cases are those of
tests/driving_vec_cases.py; the GPU self-test feeds the same ones to the device.
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from driving_vec_cases import driving_cases  # noqa: E402

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ not found"
    exe = str(tmp_path_factory.mktemp("driving_vec") / "driving_vec_check")
    src = os.path.join(ROOT, "tests", "native", "driving_vec_check.cpp")
    subprocess.run([cxx] + FLAGS + ["-I" + os.path.join(ROOT, "posggym-baselines_amd", "csrc"), src,
                                    "-o", exe], check=True, capture_output=True, text=True)
    return exe


def test_driving_vec_matches_scalar_model(checker, tmp_path):
    from posggym_baselines_amd.envs import DrivingModel
    model = DrivingModel("14x14RoundAbout")
    cases = driving_cases(model)
    # every tier is there: the sweep of vehicle 0 alone is cells x 4 x 4 x 5 x 2
    free = sum(not w for row in model._wall for w in row)
    assert len(cases) == free * (4 * 4 * 5 * 2 + 4 * 4 * 5 * 3 * 2 + 4 * 8 * 5 * 3)
    assert set(cases[:, 4]) == {0, 1} and set(cases[:, 2]) == set(range(5)) == set(cases[:, 3])
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(bytes(model.pomcp_grid()))
        f.write(cases.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([checker, str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert p.stdout.strip().splitlines()[-1] == f"cases {len(cases)} mismatches 0"
