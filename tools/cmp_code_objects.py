"""Developer tool: is the device code of two builds the same?  No GPU needed.
usage: python tools/cmp_code_objects.py <csrc/_obj of build A> <csrc/_obj of build B>

For every translation unit, the gfx950 code object is taken out of the object file (llvm-objdump --offloading) and the two
are compared: byte for byte, then kernel by kernel -- the set of kernels, each kernel's instructions with their encodings
(addresses dropped: a kernel may sit elsewhere in .text) and each kernel's metadata note (registers, LDS, scratch,
arguments).  Two builds from different directories never match byte for byte: the compilation-unit id hashes the path."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def code_object(obj, into):
    """the gfx950 code object of one object file, or None for a unit without device code"""
    os.makedirs(into)
    shutil.copy(obj, into)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(obj)], cwd=into, check=True,
                   stdout=subprocess.DEVNULL)
    hits = glob.glob(os.path.join(into, "*gfx950*"))
    return hits[0] if hits else None


def kernels(path):
    """kernel -> its lines of `llvm-objdump -d` without addresses, in .text order"""
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
    found, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = found.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":  # ("...": the padding between two kernels)
            cur.append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line).strip())
    return found


def metadata(path):
    """kernel -> its record of the amdhsa.kernels note, lines sorted"""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    found = {}
    for rec in re.split(r"\n  - ", out.split("amdhsa.kernels:")[1].split("amdhsa.target")[0]):
        m = re.search(r"\.name:\s+(\S+)", rec)
        if m:
            found[m.group(1)] = sorted(l.strip() for l in rec.splitlines())
    return found


def main(dir_a, dir_b):
    bad = 0
    print("| unit | kernels | instructions | bytes | kernel set | kernels whose instructions differ | whose metadata differ | order in .text |")
    print("|---|---|---|---|---|---|---|---|")
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(dir_a, "*.o"))):
            unit = os.path.basename(obj)[:-2]
            a = code_object(obj, os.path.join(tmp, "a", unit))
            b = code_object(os.path.join(dir_b, unit + ".o"), os.path.join(tmp, "b", unit))
            if a is None or b is None:
                print(f"| {unit} | {'no device code' if a is None and b is None else 'ONE SIDE ONLY'} | | | | | | |")
                bad += (a is None) != (b is None)
                continue
            ka, kb, ma, mb = kernels(a), kernels(b), metadata(a), metadata(b)
            same = open(a, "rb").read() == open(b, "rb").read()
            text = [k for k in ka if ka[k] != kb.get(k)]
            meta = [k for k in ma if ma[k] != mb.get(k)]
            sets = sorted(ka) == sorted(kb) and sorted(ma) == sorted(mb)
            bad += bool(text or meta or not sets)
            print(f"| {unit} | {len(ma)} / {len(mb)} | {sum(map(len, ka.values()))} / {sum(map(len, kb.values()))} | "
                  f"{'identical' if same else 'differ'} | {'same' if sets else 'DIFFERS'} | {len(text)} | {len(meta)} | "
                  f"{'same' if list(ka) == list(kb) else 'differs'} |")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
