"""The dispatch helpers of csrc/as_common.h on the host (as_up_to, as_exactly, as_flag): tests/dispatch_check.cpp, which includes
the header under AS_HOST_ONLY, is compiled with g++ and run as a child process -- once plainly and once with the address and
undefined-behaviour sanitizers (the runtime inside the program, nothing preloaded).  It walks every list a call site uses against
the if-ladder the helper replaced; see the file's head for what it checks per case."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_dispatch_helpers_match_the_ladders(tmp_path, sanitize):
    exe = str(tmp_path / "dispatch_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "artspeech_amd", "csrc"), os.path.join(ROOT, "tests", "dispatch_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stdout[-4000:] + run.stderr[-4000:]
    m = re.fullmatch(r"dispatch: (\d+) checks", run.stdout.strip())
    assert m and int(m.group(1)) > 0, run.stdout[-2000:]
