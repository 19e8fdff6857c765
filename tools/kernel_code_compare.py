"""Which kernels of two builds of libyolov3_hip.so differ: every gfx950 code object of both libraries is disassembled
(llvm-objdump) and each kernel's instruction text -- addresses and encodings dropped -- is hashed.
usage: kernel_code_compare.py OLD.so NEW.so"""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/llvm/bin/llvm-objdump")


def kernels(lib):
    """{kernel symbol: sha256 of its disassembly} over all gfx950 code objects of ``lib``"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        subprocess.run([OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
        for co in sorted(glob.glob(local + ".*gfx950")):
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
            name, body = None, []
            for line in text.splitlines() + ["0 <end>:"]:
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    if name:
                        out[name] = hashlib.sha256("\n".join(body).encode()).hexdigest()
                    name, body = m.group(1), []
                elif name and line.strip() and not line.startswith("Disassembly"):
                    body.append(re.sub(r"//.*$", "", line).strip())
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    changed = sorted(k for k in old if k in new and old[k] != new[k])
    added, removed = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    print("kernels: old %d, new %d; identical %d, changed %d, added %d, removed %d" % (
        len(old), len(new), len(old) - len(changed) - len(removed), len(changed), len(added), len(removed)))
    for tag, names in (("changed", changed), ("added", added), ("removed", removed)):
        for k in names:
            print("  %-8s %s %s" % (tag, new.get(k, old.get(k))[:16], k))
    if "-v" in sys.argv:
        for k in sorted(set(old) & set(new) - set(changed)):
            print("  same     %s %s" % (new[k][:16], k))


if __name__ == "__main__":
    main()
