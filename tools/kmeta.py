"""Per-kernel resources of a built HIP object (VGPR / SGPR / LDS / scratch per
lane / spills), read from the gfx950 code object's metadata notes:

    python3 tools/kmeta.py rendering-algorithms-raytracer_amd/lib/build/mrt_device.o [regex]

No GPU needed (the same numbers rocprofv3's kernel trace reports per dispatch).

    python3 tools/kmeta.py --diff OLD.o NEW.o

compares two builds of one object function by function (kernels and out-of-line device
functions): address, size and a hash of the bytes in .text.  Exit status 1 unless the
only differences are renames (same position, size and bytes under another name)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

B = "/opt/rocm/lib/llvm/bin"


def unbundle(obj, t):
    """The gfx950 code object of a host object, written into directory t."""
    fat, co = os.path.join(t, "fat.bin"), os.path.join(t, "dev.co")
    subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fat}", obj], check=True)
    subprocess.run([f"{B}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return co


def readelf(flag, co):
    return subprocess.run([f"{B}/llvm-readelf", flag, co], capture_output=True, text=True, check=True).stdout


def kernels(obj):
    with tempfile.TemporaryDirectory() as t:
        notes = readelf("--notes", unbundle(obj, t))
    rows, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s+- \.agpr_count:", line)
        if m:
            cur = {}
            rows.append(cur)
        m = re.match(r"\s+\.(\w+):\s+(\S+)", line)
        if m and cur is not None:
            cur.setdefault(m.group(1), m.group(2))
    return rows


def functions(obj):
    """{name: (address, size, sha1 of its bytes)} of every FUNC symbol of the code object."""
    with tempfile.TemporaryDirectory() as t:
        co, txt = unbundle(obj, t), os.path.join(t, "text.bin")
        m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)", readelf("-SW", co))
        base = int(m.group(1), 16)
        subprocess.run([f"{B}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, txt], check=True)
        text = open(txt, "rb").read()
        syms = readelf("-sW", co)
    out = {}
    for p in (line.split() for line in syms.splitlines()):
        if len(p) >= 8 and p[3] == "FUNC" and p[6] != "UND":
            a, n = int(p[1], 16), int(p[2])
            out[p[7]] = (a, n, hashlib.sha1(text[a - base:a - base + n]).hexdigest())
    return out


def diff(old, new):
    a, b = functions(old), functions(new)
    ka, kb = ({r.get("name"): r for r in kernels(o)} for o in (old, new))
    only_a = {v[0]: n for n, v in a.items() if n not in b}   # by address: a rename keeps its position
    only_b = {v[0]: n for n, v in b.items() if n not in a}
    pairs = [(n, n) for n in a if n in b] + [(only_a[x], only_b[x]) for x in only_a if x in only_b]
    renamed = [(m, n) for m, n in pairs if m != n]
    changed = [(m, n) for m, n in pairs if a[m][1:] != b[n][1:]]
    gone = [n for x, n in only_a.items() if x not in only_b]
    added = [n for x, n in only_b.items() if x not in only_a]
    for m, n in renamed:
        print("renamed   %s -> %s" % (m, n))
    for n in gone:
        print("only old  %s" % n)
    for n in added:
        print("only new  %s" % n)
    fig = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")
    for m, n in changed:
        print("differs   %s: size %d -> %d" % (n, a[m][1], b[n][1]))
        if m in ka and n in kb:
            print("          vgpr/sgpr/lds/scratch/vspill %s -> %s" % (
                "/".join(ka[m].get(f, "?") for f in fig), "/".join(kb[n].get(f, "?") for f in fig)))
    print("%s: %d kernels, %d functions old, %d new; %d identical, %d renamed, %d differ, %d only old, %d only new" % (
        os.path.basename(new), len(kb), len(a), len(b), len(pairs) - len(changed), len(renamed), len(changed),
        len(gone), len(added)))
    return 1 if changed or gone or added or len(ka) != len(kb) else 0


def main():
    if sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    obj = sys.argv[1]
    pat = sys.argv[2] if len(sys.argv) > 2 else ""
    for r in kernels(obj):
        name = r.get("name", "?")
        dm = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if pat and not (re.search(pat, name) or pat in dm):
            continue
        dm = dm.replace("mrt::", "").replace("(RenderParams)", "").replace("void ", "")
        print("%-60s vgpr %4s sgpr %4s lds %6s scratch %5s vspill %4s" % (
            dm[:60], r.get("vgpr_count"), r.get("sgpr_count"), r.get("group_segment_fixed_size"),
            r.get("private_segment_fixed_size"), r.get("vgpr_spill_count")))


if __name__ == "__main__":
    main()
