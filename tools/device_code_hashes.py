"""What a host-only refactor must leave alone, as one JSON document: the SHA-256 of every object's gfx950 code object and the library's
exported C entries.

    python tools/device_code_hashes.py [CSRC_DIR]      # default: this tree's csrc; its build/*.o and ../lds/liblds.so must exist

Run it on two builds (say, the parent commit's and this one's) and compare the documents: equal "device_sha256" means that no text a
compiler turns into device code differs, so kernel times are unchanged by construction; equal "exports" means the C ABI's symbol list is
the same.  The code objects are extracted with llvm-objdump --offloading, the way tests/test_cpu_no_spills.py does."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def device_sha(obj):
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(obj, os.path.join(tmp, "o.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "o.o"], check=True, capture_output=True, cwd=tmp)
        outs = sorted(f for f in os.listdir(tmp) if "gfx950" in f)      # the bundles are extracted next to the input
        assert len(outs) <= 1, (obj, outs)
        if not outs: return None      # a file without device code (model.hip)
        return hashlib.sha256(open(os.path.join(tmp, outs[0]), "rb").read()).hexdigest()


def main():
    csrc = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "latent-diffusion-speech_amd", "csrc")
    objs = sorted(f for f in os.listdir(os.path.join(csrc, "build")) if f.endswith(".o"))
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(csrc, "..", "lds", "liblds.so")], check=True, capture_output=True, text=True).stdout
    syms = sorted(line.split()[-1] for line in nm.splitlines())
    print(json.dumps({"device_sha256": {o[:-2] + ".hip": device_sha(os.path.join(csrc, "build", o)) for o in objs},
                      "exports": [s for s in syms if s.startswith("lds_")],
                      "exports_cxx_naming_lds": [s for s in syms if "lds_" in s and not s.startswith("lds_")]}, indent=1))


if __name__ == "__main__":
    main()
