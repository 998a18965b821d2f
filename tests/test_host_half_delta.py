"""Delta frames of half-block streams without a GPU: the Python restatement of the rule (tests/restate_half_delta.py) against its own
replay -- a terminal that forgets both colours at every cursor escape -- against its bound and against known answers; and
rtxplan::half_delta_bound / half_delta_block_bound / plan_update's new entry (csrc/rtx_plan.hpp) against brute force --
tests/host/test_half_delta.cpp, compiled as host-only C++ and run under AddressSanitizer + UndefinedBehaviorSanitizer with the g++
line of tests/test_host_half.py."""
import os
import subprocess

import pytest

import restate_half as RH
import restate_half_delta as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = RH.NO


def test_half_delta_planning_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_half_delta")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_half_delta.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and "all half-block delta planning tests passed" in p.stdout, p.stdout[-4000:]


def test_the_restatement_replays_and_stays_within_its_bound():
    assert RD.self_test()


def test_known_answers():
    G = RH.GLYPH
    # W = 4: three cells; rows top then bottom.  Cell 0 unchanged, cells 1 and 2 changed: one run at (1, 2)
    prev = [1, 2, 3, NO, 4, 5, 6, NO]
    cur = [1, 7, 7, NO, 4, 5, 9, NO]
    assert RD.half_delta_stream(RH.BIT_PIXEL, 4, 1, cur, prev) == (
        b"\x1b[1;2H\x1b[38;5;7m\x1b[48;5;5m" + G + b"\x1b[48;5;9m" + G, 2, 1)  # cell 2: T as its left neighbour's, B differs
    # a start emits both escapes although only B changed; column 0 of the next row starts a run of its own
    prev = [1, NO, 2, NO, 1, NO, 2, NO]
    cur = [1, NO, 3, NO, 1, NO, 3, NO]
    assert RD.half_delta_stream(RH.BIT_PIXEL, 2, 2, cur, prev) == (
        b"\x1b[1;1H\x1b[38;5;1m\x1b[48;5;3m" + G + b"\x1b[2;1H\x1b[38;5;1m\x1b[48;5;3m" + G, 2, 2)
    assert RD.half_delta_stream(RH.RGB_PIXEL, 2, 1, [0x200A64FF, NO, 0, NO], [0, NO, 0, NO]) == (
        b"\x1b[1;1H\x1b[38;2;255;100;10m\x1b[48;2;0;0;0m" + G, 1, 1)
    assert RD.half_delta_stream(RH.RGB_PIXEL, 1, 3, [1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1]) == (b"", 0, 0)
    with pytest.raises(ValueError):
        RD.half_delta_stream(RH.SDL, 2, 1, [0, NO, 0, NO], [1, NO, 1, NO])


def test_the_replay_rejects_what_is_not_a_stream():
    mode = RH.RGB_PIXEL
    good, _, _ = RD.half_delta_stream(mode, 3, 1, [0x200A64FF, 0x200A64FF, NO, 0, 1, NO], [5, 5, NO, 5, 5, NO])
    assert RD.apply_half_delta(mode, [[(5, 5), (5, 5)]], good) == [[(0x0A64FF, 0), (0x0A64FF, 1)]]
    for bad in (good[6:],                                    # no cursor escape
                good.replace(b"\x1b[48;2;0;0;0m", b"", 1),   # a run that does not set its background
                good.replace(b"[1;1H", b"[1;3H"),            # runs off the row
                good.replace(b"[1;1H", b"[01;1H"),           # leading zeros
                good.replace(b"255", b"256"),                # a component out of range
                good.replace(b"48;2;0;0;0", b"48;5;0"),      # the other family's escape
                good + b"\n"):                               # a delta has no newlines
        with pytest.raises(ValueError):
            RD.apply_half_delta(mode, [[(5, 5), (5, 5)]], bad)


def test_the_bound_is_met_by_rows_that_changed_everywhere():
    for mode, C in ((RH.RGB_PIXEL, 41), (RH.BIT_PIXEL, 25)):
        W, H = 120, 101
        # every cell differs from prev and from its left neighbour in both halves, every component has three digits
        cur = [NO] * (W * 2 * H)
        for r in range(2 * H):
            for c in range(W - 1):
                v = 100 + ((r * 7 + c * 3) % 150)
                cur[r * W + c] = v | ((v + 1) << 8) | ((v + 2) << 16)
        prev = [NO if (i + 1) % W == 0 else 0x00FFFFFF ^ 1 for i in range(W * 2 * H)]
        s, cells, runs = RD.half_delta_stream(mode, W, H, cur, prev)
        assert (cells, runs) == ((W - 1) * H, H)
        want = sum(C * (W - 1) + RD.cup_length(r, 0) for r in range(H))
        assert len(s) == want <= RD.half_delta_bound(mode, W, H)
        # ... and the bound itself is that with the row's longest escape
        assert RD.half_delta_bound(mode, W, H) == sum(C * (W - 1) + RD.cup_length(r, W - 2) for r in range(H))
