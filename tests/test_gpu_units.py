"""Device numerics, function by function, on the GPU against the oracle, bit for bit.

tests/cpp/device_units evaluates one device leaf function (the renderer's own headers, compiled
with the library's flags, in a kernel of the render kernels' shape) on the rows of tests/_units.py;
the words must equal those of liboracle_glibc.so's orc_unit, the reference semantics.  There are
no tolerances.  On a mismatch the message shows the first rows three ways -- device, glibc, and
liboracle_spm.so (the same headers compiled for the host): device != glibc == spm is a problem of
the device compilation, device == spm != glibc one of the header that tests/test_libm_exact.py
should see too.

NaN rule (tests/_units.py): for the lm_* functions, fmod1, round_f and rsqrtss_emulated all bits are
compared for every input, NaN inputs and results included; for everything else an output word that
is a NaN in the reference only has to be a NaN on the device, and the rows concerned are counted
and printed.  One named exception (_units.EXCEPTIONS): a negative denormal argument of
rsqrtss_emulated / rsqrt_ref, which no kernel can produce; those rows are counted and left out.

powf_unit's rows carry device lm_powf_unit and device lm_powf, beck11_pre's the precomputed form
and beckmann_sample11 on the same cosine: each pair is compared with the same reference words, so
the two device forms are equal to each other wherever the test passes.

The evaluator exists once per kernel option set (tests/cpp/Makefile SET_*).  The
default set's runs every unit; the other sets' run the pixel stream and the units that own a
generator, the code the options change.  The stream-fed units (rho16 .. material_pdf) also compare
the number of stream words consumed and one further draw; the served forms, mf_sample_pre and the
image light's replayed lookups are compared with the same reference words as the form they restate.

Each test runs the evaluator once, in a child process, one at a time; after a child that ended
abnormally (signal, HIP error, time limit) the remaining tests of this module are skipped."""
import os
import subprocess
import time

import numpy as np
import pytest

import simplepath_amd as sp
from tests import _units

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "_build", "device_units")
_abnormal = []  # the first child that ended abnormally: nothing more is started on the GPU after it


@pytest.fixture(scope="session")
def exe():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "_build/device_units"], check=True, timeout=600)
    return EXE


@pytest.fixture(scope="session")
def table_file(tmp_path_factory):
    """This host's RSQRTSS table (the one the library installs): bits, zero_result, denorm_result, entries."""
    t = sp.rsqrt_table()
    path = str(tmp_path_factory.mktemp("units") / "rsqrt_table.bin")
    np.concatenate([np.array([t["bits"], t["zero_result"], t["denorm_result"]], dtype=np.uint32),
                    t["entries"].astype(np.uint32)]).tofile(path)
    return path


def _hex(a):
    return " ".join(f"{int(v):08x}" for v in a)


@pytest.fixture(scope="session")
def set_exe():
    """The evaluator of one kernel option set (tests/cpp/Makefile SET_<name>)."""
    def get(option_set):
        path = _units.evaluator(option_set)
        if not os.path.exists(path):
            subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), os.path.relpath(path, os.path.join(ROOT, "tests", "cpp"))],
                           check=True, timeout=600)
        return path
    return get


@pytest.fixture(scope="module")
def expected():
    """Rows and reference words per unit, computed once and shared by the option sets (read-only)."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        rows = _units.rows(name)
        ref = _units.reference("glibc", name, rows)
        rows.setflags(write=False)
        ref.setflags(write=False)
        if name in SET_UNITS:  # run once per option set; the leaf functions run once and are not kept
            cache[name] = (rows, ref)
        return rows, ref
    return get


def run_device(exe, name, rows, tmp_path, table_file):
    if _abnormal:
        pytest.skip(f"device_units ended abnormally in {_abnormal[0]}: nothing more is run on the GPU")
    spec = _units.FUNCTIONS[name]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)
    cmd = [exe, _units.device_name(name), fin, fout] + ([table_file] if spec.table else [])
    if spec.image:
        _units.image_words(spec.image).tofile(str(tmp_path / "image.bin"))
        cmd.append(str(tmp_path / "image.bin"))
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired:
        _abnormal.append(name)
        raise
    if r.returncode != 0:
        if r.returncode < 0 or r.returncode not in (1, 2):  # a signal, or a HIP error (exit 3)
            _abnormal.append(name)
        pytest.fail(f"device_units {name}: exit {r.returncode}\n{r.stdout}{r.stderr}")
    fn, n, ms = r.stdout.split()
    assert fn == _units.device_name(name) and int(n) == rows.shape[0], r.stdout
    return np.fromfile(fout, dtype=np.uint32).reshape(rows.shape[0], spec.m), float(ms)


@pytest.mark.parametrize("name", _units.units_of("default"))
def test_device_function_matches_oracle(exe, table_file, tmp_path, expected, name):
    """Every unit in the evaluator of the default option set (sp_mega.hip's)."""
    _compare(exe, "default", table_file, tmp_path, expected, name)


# The other option sets run the units that read an option: the pixel stream and the units that own a
# generator (_units.DRAWING).  The leaf functions of sections a-e, the light units and the image
# light's take no generator and read none of the options, so their code is the same in every
# evaluator and the default one stands for all.
SET_UNITS = [n for n in _units.FUNCTIONS if n == "stream" or n in _units.DRAWING]


@pytest.mark.parametrize("option_set,name", [(s, n) for s in _units.OPTION_SETS if s != "default"
                                             for n in _units.units_of(s) if n in SET_UNITS])
def test_unit_in_option_set(set_exe, table_file, tmp_path, expected, option_set, name):
    _compare(set_exe(option_set), option_set, table_file, tmp_path, expected, name)


def _compare(exe, option_set, table_file, tmp_path, expected, name):
    if _abnormal:
        pytest.skip(f"device_units ended abnormally in {_abnormal[0]}: nothing more is run on the GPU")
    t0 = time.perf_counter()
    rows, glibc = expected(name)
    t1 = time.perf_counter()
    dev, ms = run_device(exe, name, rows, tmp_path, table_file)
    t2 = time.perf_counter()
    bad, nan_rows, excepted = _units.mismatches(name, rows, dev, glibc)
    print(f"[{option_set}] {name}: {rows.shape[0]} rows, kernel {ms:.3f} ms, child {t2 - t1:.2f} s, inputs+reference {t1 - t0:.2f} s, "
          f"{nan_rows} rows with a reference NaN ({_units.FUNCTIONS[name].rule}), {excepted} rows excepted"
          f"{' (' + _units.EXCEPTIONS[name][0] + ')' if name in _units.EXCEPTIONS else ''}, {bad.size} mismatching rows")
    if bad.size:
        spm = _units.reference("spm", name, rows[bad[:8]])
        lines = [f"  in {_hex(rows[i])}\n    device {_hex(dev[i])}\n    glibc  {_hex(glibc[i])}\n    spm    {_hex(spm[j])}"
                 for j, i in enumerate(bad[:8])]
        pytest.fail(f"{name}: {bad.size} of {rows.shape[0]} rows differ from the reference\n" + "\n".join(lines))
