"""csrc/rtx_options.hpp -- the context's options as one struct and one table -- compiled as host-only C++ and run under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/host/test_options.cpp holds the expected rows, written out by hand), and the
table against include/rtx.h: every RTX_OPT_* of the header is one row, or one of a device group's four."""
import os
import re
import shutil
import subprocess

import pytest

from test_abi_reflect_shadows import header_enums

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_OPTIONS = {"RTX_OPT_GROUP_EXCHANGE", "RTX_OPT_GROUP_WIRE", "RTX_OPT_GROUP_THREADS", "RTX_OPT_GROUP_UPDATE"}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_option_table_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_options")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", os.path.join(ROOT, "tests", "host", "test_options.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert p.returncode == 0 and "all option table tests passed" in p.stdout, p.stdout[-4000:]


def table_rows():
    """The option name each row of rtxopt::kRows starts with, in order."""
    src = open(os.path.join(ROOT, "raytracing-in-windows-console_amd", "csrc", "rtx_options.hpp")).read()
    body = src[src.index("kRows[] = {"):]
    body = body[:body.index("\n};")]
    return re.findall(r"^\s*\{(RTX_OPT_[A-Z0-9_]+),", body, flags=re.M)


def test_every_header_option_is_one_row_or_a_group_option():
    names = {k for k in header_enums() if k.startswith("RTX_OPT_")}
    rows = table_rows()
    assert GROUP_OPTIONS <= names
    assert len(rows) == 27 and len(set(rows)) == len(rows)
    assert set(rows) == names - GROUP_OPTIONS
    # nobody switches over the context's options a second time: rtx_get_option and the query counters read through the table
    csrc = os.path.join(ROOT, "raytracing-in-windows-console_amd", "csrc")
    assert open(os.path.join(csrc, "rtx_api.cpp")).read().count("case RTX_OPT_") <= 5
    assert "case RTX_OPT_" not in open(os.path.join(csrc, "rtx_query.cpp")).read()
