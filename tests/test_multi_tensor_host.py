"""csrc/multi_tensor.h's table-filling loop (host code with an overflow split) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/multi_tensor_host.cpp has its own main and no GPU call, so nothing loaded into Python is
sanitized and nothing here needs a device."""
import os
import subprocess

from where2edit_amd import build


def test_table_loop_under_asan_and_ubsan(tmp_path):
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "multi_tensor_host.cpp")
    exe = str(tmp_path / "multi_tensor_host")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cc = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", *san, "-x", "hip", src, "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "multi_tensor_host: ok" in run.stdout, run.stdout
