"""csrc/host.h, the host toolkit every C-ABI entry is written on, checked directly: `make host_selftest` builds csrc/host_selftest.cpp
host-only with AddressSanitizer + UBSan against csrc/host_stub_hip.cpp.  The program asserts the allocators' offsets, the tensor map's
messages, the create / destroy discipline (the leak check at exit is the witness that a failed create frees its uploads), the per-clip
length filler and range_check's texts.  It is an ordinary executable that carries its own sanitizer runtime: nothing is preloaded."""
import os
import subprocess

from conftest import PKG


def test_host_toolkit_selftest():
    csrc = os.path.join(PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "host_selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([os.path.join(csrc, "build_asan", "host_selftest")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "host_selftest ok" in p.stdout, (p.returncode, p.stdout[-1500:], p.stderr[-4000:])
    assert "ERROR: " not in p.stderr and "runtime error:" not in p.stderr, p.stderr[-4000:]
