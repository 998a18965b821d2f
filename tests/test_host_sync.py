"""The stream-ordering contract of csrc/rtx_sync.hpp (rtxsync::Shared and the stream-keyed table) without a GPU:
tests/host/test_sync.cpp defines the HIP entry points the header calls as a happens-before model -- a vector clock per fake stream,
events that copy and join clocks, a stream that can be destroyed, a log of calls -- so no HIP library is linked; compiled with the g++
line of tests/test_host_mem.py and run directly under AddressSanitizer + UndefinedBehaviorSanitizer.  Scripted sequences pin the exact
calls of the two users (the coarse-cell list cache, the world grid); 4000 seeded random sequences check that reads queued before a
write finish before it and reads queued after it start after it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_ordering_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_sync")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                           os.path.join(ROOT, "tests", "host", "test_sync.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0 and "all ordering tests passed" in p.stdout, p.stdout[-4000:]
    assert "4000 random sequences of 40 operations, 0 broke the contract" in p.stdout, p.stdout[-4000:]
