"""gfx950 device code of two builds compared kernel by kernel: text size, SHA-256 of every __global__ symbol's bytes and the resource metadata of the code
object's notes -- the report format of profiles/enc_shared_device_text.txt.  A template that gained trailing defaulted parameters keeps its code but not its
mangled name: a kernel of the second build that the first does not have is paired with the first build's kernel whose mangled name is the same without one
trailing `false` template argument ("Lb0E" in front of the argument list's end) and marked '~'.  A kernel that was renamed outright (a copy that became an
instantiation of a shared template) is paired with a kernel of the same object that only the first build has and whose (size, SHA-256, resource tuple) are
equal, and marked '@' (no such kernel in the same object: one of any object, for a kernel whose source file was merged into another).
usage: python tools/device_text_diff.py PARENT_BUILD_DIR THIS_BUILD_DIR > profiles/NAME.txt"""
import glob, hashlib, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size", ".uses_dynamic_stack")


def kernels_of(obj, tmp):
    """{mangled name: (size, sha256 of the text bytes, resource tuple)} and the SHA-256 / size of the whole .text, or None for a host-only object"""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "co.o")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"],
                       capture_output=True, text=True)
    if r.returncode or not os.path.exists(co):
        return None
    sec = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "--wide", co], capture_output=True, text=True).stdout
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    addr, off, size = (int(x, 16) for x in m.groups())
    blob = open(co, "rb").read()
    text = blob[off:off + size]
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    res = {}
    for block in notes.split("- .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1).strip("'\"")
        res[name] = tuple(re.search(re.escape(k) + r":\s+(\S+)", block).group(1) if re.search(re.escape(k) + r":\s+(\S+)", block) else "?" for k in KEYS)
    out = {}
    sym = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "--wide", co], capture_output=True, text=True).stdout
    for line in sym.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[4] == "GLOBAL" and not f[7].endswith(".kd"):
            a, n = int(f[1], 16), int(f[2])
            out[f[7]] = (n, hashlib.sha256(text[a - addr:a - addr + n]).hexdigest(), res.get(f[7], ("?",) * len(KEYS)))
    return out, hashlib.sha256(text).hexdigest(), size


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, r))


def main():
    parent_dir, this_dir = sys.argv[1:3]
    tmp = tempfile.mkdtemp()
    print("# gfx950 device code of every object of two builds (same make, same toolchain): parent commit against this change.")
    print("# extraction: llvm-objcopy --only-section=.hip_fatbin | clang-offload-bundler --unbundle --targets=hipv4-amdgcn-amd-amdhsa--gfx950 | the .text bytes of every FUNC GLOBAL symbol")
    print("# per __global__ symbol: text size, SHA-256 of the symbol's bytes, and the resource metadata of the code object's notes")
    print("# (" + " ".join(k[1:] for k in KEYS) + ")")
    print("# kernels are paired by mangled name; a template that gained a trailing defaulted `false` parameter is paired with its parent name ('~');")
    print("# a kernel that only this change has is paired with a kernel that only the parent has (of the same object, else of any) when their size, bytes and resources are equal ('@')")
    print("#\n# object                 text bytes  parent .text SHA-256[:16]  this .text SHA-256[:16]  kernels (parent/this)")
    P, Tk = {}, {}
    for obj in sorted(glob.glob(os.path.join(this_dir, "*.o"))):
        base = os.path.basename(obj)
        t = kernels_of(obj, tmp)
        pobj = os.path.join(parent_dir, base)
        p = kernels_of(pobj, tmp) if os.path.exists(pobj) else None
        if t is None:
            print(f"{base:24s} {0:10d}  (host only)")
            continue
        for k, v in t[0].items():
            Tk[k] = (base,) + v
        for k, v in (p[0] if p else {}).items():
            P[k] = (base,) + v
        same = p is not None and p[1] == t[1]
        print(f"{base:24s} {t[2]:10d}  {(p[1][:16] if p else '-'):24s}  {t[1][:16]:22s}  {'equal  ' if same else 'DIFFERS'}  kernels {len(p[0]) if p else 0}/{len(t[0])}")
    for pobj in sorted(glob.glob(os.path.join(parent_dir, "*.o"))):      # an object only the parent has (its source file went into another): its kernels still pair by bytes
        base = os.path.basename(pobj)
        if os.path.exists(os.path.join(this_dir, base)):
            continue
        p = kernels_of(pobj, tmp)
        print(f"{base:24s} {(p[2] if p else 0):10d}  {(p[1][:16] if p else '-'):24s}  {'-':22s}  {'GONE   '}  kernels {len(p[0]) if p else 0}/0")
        for k, v in (p[0] if p else {}).items():
            P[k] = (base,) + v
    dp, dt = demangle(list(P)), demangle(list(Tk))
    key_t = {k: (k if k in P or k.replace("Lb0EEv", "Ev", 1) not in P else k.replace("Lb0EEv", "Ev", 1)) for k in Tk}
    by_name_p = {k: k for k in P}
    paired, new = [], []
    for k in sorted(Tk, key=lambda k: (Tk[k][0], key_t[k])):
        (paired if key_t[k] in by_name_p else new).append(k)
    # renamed outright: a kernel only this build has, paired by its bytes with a kernel that only the parent has (each parent kernel once): one of the same object,
    # else -- its source file went into another -- one of any object
    unclaimed = sorted(set(by_name_p) - {key_t[k] for k in paired})
    by_bytes = {}
    for same_object in (True, False):
        for k in list(new):
            for q in unclaimed:
                if P[q][1:] == Tk[k][1:] and (P[q][0] == Tk[k][0] or not same_object):
                    by_bytes[k] = q
                    unclaimed.remove(q)
                    new.remove(k)
                    break
    gone = sorted(set(by_name_p) - {key_t[k] for k in paired} - set(by_bytes.values()))
    differ = [k for k in paired if Tk[k][1:] != P[by_name_p[key_t[k]]][1:]]
    renamed = [k for k in paired if k != by_name_p[key_t[k]]]
    print(f"#\n# kernel symbols: parent {len(P)}, this change {len(Tk)}; only in parent: {gone}; only in this change: {len(new)} (listed below as 'new')")
    print(f"# kernels in both: {len(paired)}; with a size, byte or resource difference: {len(differ)}; same bytes under a longer mangled name: {len(renamed)}")
    print(f"# kernels under a new name whose size, bytes and resources equal those of a kernel only the parent has: {len(by_bytes)}")
    print("#\n# size  sha256[:16]  resources  object  symbol     ('=' : size, bytes and resources equal the parent's; '~' : equal, the mangled name gained defaulted parameters;")
    print("#                                                    '@' : equal to the parent kernel named on the next line, paired by its bytes; '*' : differs; 'new')")
    for k in sorted(Tk, key=lambda k: (Tk[k][0], dt[k])):
        base, n, h, res = Tk[k]
        if k in new:
            mark = "new"
        elif k in by_bytes:
            mark = "@"
        else:
            mark = "*" if k in differ else ("~" if k in renamed else "=")
        print(f"{n:8d}  {h[:16]}  {' '.join(res)}  {base:20s} {mark:3s}  {dt[k][:170]}")
        if mark == "*":
            pb, pn, ph, pres = P[by_name_p[key_t[k]]]
            print(f"{pn:8d}  {ph[:16]}  {' '.join(pres)}  (parent)")
        if mark == "@":
            print(f"{'':8s}  {'':16s}  (parent, {P[by_bytes[k]][0]}: {dp[by_bytes[k]][:170]})")
    if gone:
        print("#\n# only in the parent (renamed here with other bytes, or removed): their size, bytes and resources, to read a renamed kernel's 'new' line against")
        for k in sorted(gone, key=lambda k: (P[k][0], dp[k])):
            base, n, h, res = P[k]
            print(f"{n:8d}  {h[:16]}  {' '.join(res)}  {base:20s} gone {dp[k][:170]}")


if __name__ == "__main__":
    main()
