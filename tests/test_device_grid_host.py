"""host/DeviceGrid.cpp — the owner of a kw_ctx that ThermalSolver, CwPropagator, AngularSpectrum, AngularSpectrumTime and
PlaneRecon hold as a member — stand-alone on the CPU under the sanitizers, over a fake of the kw_* functions it calls
(tests/native/device_grid_check.cpp): the success paths and, for the first time, the failure half of those constructors."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARRAYS = ["malloc(400)#0", "malloc(800)#1", "malloc(1200)#2", "malloc(1600)#3", "malloc(2000)#4"]
FUSED = "init set_constants(48) fused_supported fused_create "


def _fails_at(k):
    """the k-th of the five allocations fails: the earlier ones are freed, the pipeline and the context destroyed"""
    made = ARRAYS[:k - 1]
    return "bad_alloc | " + FUSED + " ".join(made + [ARRAYS[k - 1].split("#")[0] + "!", "sync"] +
                                             ["free#%d" % i for i in range(k - 1)] + ["fused_destroy", "destroy"])


EXPECTED = {
    "success_fused": "fused | " + FUSED + " ".join(ARRAYS) + " sync free#0 free#1 free#2 free#3 free#4 fused_destroy destroy",
    "success_rocfft": "rocfft | init set_constants(48) plans_3d " + " ".join(ARRAYS) + " sync free#0 free#1 free#2 free#3 free#4 destroy",
    # wanted but not supported: the plans, for the constants given for that case
    "unsupported": "rocfft | init set_constants(48) fused_supported set_constants(1) plans_3d " + " ".join(ARRAYS) +
                   " sync free#0 free#1 free#2 free#3 free#4 destroy",
    # no context: no further call, no kw_destroy(NULL)
    "init_fails": "DeviceError 6 fake: init failed | init!",
    **{"malloc_%d_fails" % k: _fails_at(k) for k in range(1, 6)},
    # kw_fused_destroy frees what a failed kw_fused_create left
    "fused_create_fails": "DeviceError 2 fake: fused_create failed | " + FUSED.rstrip() + "! sync fused_destroy destroy",
    "set_constants_fails": "DeviceError 1 fake: set_constants failed | init set_constants(48)! sync destroy",
    # freed at once, and not again by the destructor
    "release": "ok | init malloc(40)#0 malloc(80)#1 free#0 released sync free#1 destroy",
    # kw_fused_reduced_elems floats (the fake says 1234), owned
    "import_reduced": "ok | " + FUSED + "malloc(12)#0 h2d#0 reduced_elems malloc(4936)#1 import#1<-#0 sync free#0 free#1 "
                      "fused_destroy destroy",
    "grid_constants": "n=16x32x48=24576 complex=9x32x48=13824 dividers_bit_equal=1 others_zero=1 |",
}


def test_device_grid_under_address_and_ub_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    host = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "host")
    exe = str(tmp_path / "device_grid_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-I" + host,
           os.path.join(ROOT, "tests", "native", "device_grid_check.cpp"), os.path.join(host, "DeviceGrid.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stdout and "ERROR: LeakSanitizer" not in r.stdout and \
        "runtime error" not in r.stdout, r.stdout[-4000:]
    lines = dict(line.split(": ", 1) for line in r.stdout.strip().splitlines())
    assert sorted(lines) == sorted(EXPECTED)
    for name, what in EXPECTED.items():
        assert lines[name].strip() == what.strip(), (name, lines[name])
    # and whatever the case: every pointer handed out is freed exactly once, kw_destroy comes once and last, and never
    # without a context
    for name, line in lines.items():
        log = line.split("|", 1)[1].split()
        made = re.findall(r"malloc\(\d+\)(#\d+)", " ".join(log))
        assert sorted("free" + p for p in made) == sorted(e for e in log if e.startswith("free")), name
        assert "destroy(null)" not in log, name
        if "init" in log:
            assert log.count("destroy") == 1 and log[-1] == "destroy", name
            sync = log.index("sync")
            assert all(e.startswith("free") or e == "fused_destroy" for e in log[sync + 1:-1]), name
            assert log.count("fused_destroy") == (1 if any(e.startswith("fused_create") for e in log) else 0), name
