"""Delta frames without a GPU: rtxplan::cup_length, delta_bound and delta_block_bound (csrc/rtx_plan.hpp) against brute force --
tests/host/test_delta.cpp, compiled as host-only C++ and run under AddressSanitizer + UndefinedBehaviorSanitizer with the g++ line of
tests/test_host_scene_remove.py -- and the Python restatement of the rule (tests/restate_delta.py) against itself."""
import os
import subprocess

import restate_delta as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_delta_planning_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_delta")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_delta.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all delta planning tests passed" in p.stdout, p.stdout[-4000:]


def test_replaying_a_delta_over_the_previous_records_gives_the_current_ones():
    assert RD.self_test()


def test_the_restated_records_and_escapes():
    assert RD.record_of_word(RD.RGB_ASCII, 0) == b"\x1b[48;2;\x00\x000;\x00\x000;\x00\x000m "
    assert RD.record_of_word(RD.RGB_ASCII, 0x41000000) == b"\x1b[38;2;\x00\x000;\x00\x000;\x00\x000mA"
    assert RD.record_of_word(RD.RGB_PIXEL, 0x200A64FF) == b"\x1b[48;2;255;100;\x0010m "
    assert RD.record_of_word(RD.BIT_ASCII, 0) == b"\x1b[48;5;\x0016m "
    assert RD.record_of_word(RD.BIT_ASCII, 0x23000010) == b"\x1b[38;5;\x0016m#"
    assert RD.record_of_word(RD.BIT_PIXEL, 0xFFFFFFFF) == bytes(12)
    assert RD.cup(0, 0) == b"\x1b[1;1H" and RD.cup(9, 99) == b"\x1b[10;100H"
    # a miss beside a black hit: the same colour digits, another selector in an ASCII mode -- the record is sent whole
    cur = [0, 0x41000000, 0xFFFFFFFF]
    prev = [5, 5, 0xFFFFFFFF]
    s, cells, runs = RD.delta_stream(RD.RGB_ASCII, 3, 1, cur, prev)
    assert (cells, runs) == (2, 1) and s == RD.cup(0, 0) + RD.record_of_word(RD.RGB_ASCII, 0) + RD.record_of_word(RD.RGB_ASCII, 0x41000000)
    s, _, _ = RD.delta_stream(RD.RGB_PIXEL, 3, 1, cur, prev)
    assert s == RD.cup(0, 0) + RD.record_of_word(RD.RGB_PIXEL, 0) + b"A"
