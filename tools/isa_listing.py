"""The gfx950 listing of a built object, kernel by kernel: the disassembly step shared by the ISA checks of tools/.

`llvm-objdump --offloading` unpacks the device code objects of a host object or shared library (libdvt_hip.so, or a single
csrc/*.o), `llvm-objdump -d` disassembles each gfx950 one.  Used by check_flat_ops.py and check_mfma_hazards.py.
"""
import os
import re
import shutil
import subprocess
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ARCH = "gfx950"

_SYM = re.compile(r"^([0-9a-f]+) <(.+)>:$")
_ADDR = re.compile(r"//\s*([0-9A-Fa-f]+):")


def kernel_listings(path, demangle=False):
    """{symbol: [(address, instruction text), ...]} over the gfx950 code objects of `path`, in address order.  The text is
    the mnemonic and its operands (the trailing `// address: encoding` comment stripped); symbols are mangled unless
    `demangle`."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        obj = shutil.copy(path, tmp)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", obj], check=True, capture_output=True, cwd=tmp)
        for name in sorted(os.listdir(tmp)):
            if ARCH not in name:
                continue
            cmd = [f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", *(["-C"] if demangle else []), os.path.join(tmp, name)]
            dis = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = _SYM.match(line)
                if m:
                    cur = out.setdefault(m.group(2), [])
                    continue
                if cur is None or not line.startswith(("\t", " ")):
                    continue
                text, _, comment = line.partition("//")
                a = _ADDR.search("//" + comment)
                text = text.strip()
                if text and a:
                    cur.append((int(a.group(1), 16), text))
    return out
