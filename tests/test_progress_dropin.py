"""sp_amd::ProgressiveRender (include/simplepath_amd.hpp): tests/cpp/progressive_main.cpp compiled
and linked as a host program would (g++ -I include -l simplepath_hip), rendering 2 + 2 samples;
its PFM equals the CPU oracle's 4-sample image bit for bit, also when the second pass runs in a
second object that imported the first one's exported state."""
import os
import subprocess

import numpy as np
import pytest

import simplepath_amd as sp
from tests import _oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "simplepath_amd", "_build")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("progressive") / "progressive_main")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "progressive_main.cpp"), "-o", out,
                    "-L", LIBDIR, "-lsimplepath_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=600)
    return out


def read_pfm(path):
    with open(path, "rb") as fh:
        assert fh.readline().strip() == b"PF"
        w, h = (int(x) for x in fh.readline().split())
        scale = float(fh.readline())
        data = np.frombuffer(fh.read(), dtype="<f4" if scale < 0 else ">f4")
    return data.reshape(h, w, 3)[::-1]  # rows bottom-up in the file (Image/Image.cpp:40)


@pytest.mark.parametrize("extra", [[], ["--checkpoint"]])
def test_progressive_drop_in_matches_oracle(exe, scene_dir, tmp_path, extra):
    out = str(tmp_path / "img.pfm")
    path = os.path.join(scene_dir, "bunny.sp")
    r = subprocess.run([exe, path, "--passes", "2,2", "--integrator", "direct_lighting", "--bvh", "1", "--size", "48", "32",
                        "--output", out, *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "4 spp in 2 passes" in r.stdout
    img = read_pfm(out)
    s = sp.Scene.from_file(path)
    s.set_resolution(48, 32)
    tiles, st = _oracle.render(s, sp.string_to_integrator_type("direct_lighting"), 4, variant="spm")
    ref = sp.tiles_to_image(48, 32, tiles)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert f"{st['rays']} rays" in r.stdout
