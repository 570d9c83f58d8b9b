"""The single-op entries behind tests/test_gpu_conv_modes.py without a GPU: include/lds_test.h declares them, lds/native.py binds them with a
struct mirror, the built library exports them (tests/test_cpu_boundary.py checks the signatures field by field)."""
import os
import re
import subprocess

from conftest import PKG, ROOT

ENTRIES = {"lds_test_dconv_pair", "lds_test_dconv_ex", "lds_test_voc_ups"}


def test_conv_mode_entries_declared_and_exported():
    import ctypes as C
    from lds import native
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "lds_test.h")).read(), flags=re.S)
    for n in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*lds_dconv_ex_test\s*;", hdr)
    assert re.search(r"int\s+lds_test_dconv_ex\(const lds_dconv_ex_test\* a, float\* out, float\* gnpart, int B, char\* cfg_out, size_t cfg_cap, void\* stream\);", hdr)
    assert ENTRIES <= set(native.TEST_EXPORTS) and not ENTRIES & set(native.EXPORTS)
    # every entry hands back the launch's configuration: a buffer and its size_t capacity in front of the stream
    assert all(native.SIGNATURES[n].endswith("pzp") for n in ENTRIES)
    assert issubclass(native.DConvExTest, C.Structure) and {"epilogue", "lengths", "lvl_in", "lvl_out", "ln_gamma", "ln_beta", "tile_batch", "fmt"} <= \
        {f[0] for f in native.DConvExTest._fields_}
    if not os.path.exists(native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", "8"], check=True, capture_output=True)
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert ENTRIES <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
