"""The owner types of az-net_amd/csrc/az_res.h (device list, buffer, buffer group, event, stream, event pool) on a counting
fake of the runtime: tests/host/az_res_main.cpp, a stand-alone program built here with the address and
undefined-behaviour sanitizers.  No GPU, no Python extension."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owners_release_exactly_once(tmp_path):
    exe = str(tmp_path / "az_res_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "host", "az_res_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout
    assert "az_res: ok" in run.stdout
