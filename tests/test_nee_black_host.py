"""direct_nee's decider (simplepath_amd/csrc/common/sp_nee_black.h) on the host:
tests/cpp/nee_black_main.cpp sweeps mf_pdf, mf_eval, the albedo, the coat factor and the Lambert
luminance over tables that hold +-0, subnormals, the values one step inside and outside each guard
face, +inf and NaN and a coat factor of exactly 0, forms the weights as glossy_weights does for
estimate luminances from 0 to the proven bound, and asserts that an answer other than "unknown" is
cblack of the finishing expression for every one of them, and that no point inside the guard's
box gets "unknown".  Then 2e6 random points of the box.  The same program once more under
AddressSanitizer and UBSan."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "nee_black_main.cpp")
FLAGS = ["g++", "-std=c++17", "-mfma", "-ffp-contract=off"]


def build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(FLAGS + extra + [SOURCE, "-o", exe], check=True, timeout=600)
    return exe


def check(r):
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert re.search(r"^0 failing$", r.stdout, re.M), r.stdout[-2000:]
    assert re.search(r"^0 unknown inside the box$", r.stdout, re.M), r.stdout[-2000:]
    m = re.search(r"^tables: (\d+) cases, (\d+) inside the box, (\d+) unknown \(0 inside the box\), (\d+) black, (\d+) not black$",
                  r.stdout, re.M)
    assert m, r.stdout[-2000:]
    cases, inside, unknown, black, not_black = (int(x) for x in m.groups())
    # the tables reach all three answers, and every point inside the box got one of the two firm ones
    assert min(inside, unknown, black, not_black) > cases // 1000
    assert black + not_black >= inside and black + not_black + unknown == cases
    m = re.search(r"^random: (\d+) cases, 0 unknown, (\d+) black, (\d+) not black$", r.stdout, re.M)
    assert m and min(int(m.group(2)), int(m.group(3))) > int(m.group(1)) // 10, r.stdout[-2000:]


def test_decider_equals_cblack_of_the_finishing_expression(tmp_path):
    exe = build(tmp_path, "nee_black", ["-O2"])
    check(subprocess.run([exe], capture_output=True, text=True, timeout=300))


def test_nee_black_program_under_sanitizers(tmp_path):
    exe = build(tmp_path, "nee_black_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([exe, "7"], capture_output=True, text=True, timeout=300)
    check(r)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
