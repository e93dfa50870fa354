"""Device code of two builds, kernel by kernel: a host-only refactoring must not change one instruction.

    UBD_SAVE_TEMPS=1 bash ubdvss_amd/csrc/build.sh         # in each tree: leaves _obj/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s
    python tools/cmp_device_code.py <parent>/ubdvss_amd/csrc/_obj ubdvss_amd/csrc/_obj

Kernels are matched by symbol over all translation units, so one may move between files.  Compared: the set of .amdhsa_kernel
names, each kernel's instruction text (block labels renumbered: their numbers count the functions in front of them in the file)
and its whole .amdhsa descriptor (registers, LDS, scratch, ...).  Prints the kernels that differ; exit status 1 if there is any."""
import glob, os, re, sys


def kernels(obj_dir):
    out = {}
    files = sorted(glob.glob(os.path.join(obj_dir, "*-hip-amdgcn-*.s")))
    if not files:
        sys.exit(f"no *-hip-amdgcn-*.s under {obj_dir}: build with UBD_SAVE_TEMPS=1")
    for path in files:
        text = open(path).read()
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
            name, desc = m.group(1), m.group(2)
            body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.amdhsa_kernel " % re.escape(name), text, re.M | re.S).group(1)
            body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", body))      # without comments: they name the labels, and pad behind them
            assert name not in out, f"{name} defined twice under {obj_dir}"
            out[name] = (body, desc)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = [f"only in {sys.argv[1]}: {k}" for k in sorted(set(a) - set(b))] + [f"only in {sys.argv[2]}: {k}" for k in sorted(set(b) - set(a))]
for k in sorted(set(a) & set(b)):
    what = [w for w, i in (("instructions", 0), ("descriptor", 1)) if a[k][i] != b[k][i]]
    if what:
        bad.append(f"differs ({', '.join(what)}): {k}")
print("\n".join(bad))
print(f"CMP_DEVICE_CODE {'FAILED' if bad else 'OK'}: {len(a)} / {len(b)} kernels, {len(bad)} differ")
sys.exit(1 if bad else 0)
