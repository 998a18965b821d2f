"""The owning types of csrc/rtx_mem.hpp (DeviceBuf, PinnedBuf, Counter, Event, Stream) without a GPU: tests/host/test_mem.cpp defines the HIP
entry points the header calls itself -- malloc behind them, a log of calls, a live count, an allocation that fails on request -- so no
HIP library is linked; compiled with the g++ line of tests/test_host_delta.py plus the HIP API header's include path, and run directly
under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owning_types_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_mem")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-Wno-unused-result",
                           os.path.join(ROOT, "tests", "host", "test_mem.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0 and "all ownership tests passed" in p.stdout, p.stdout[-4000:]
