#!/usr/bin/env python3
"""Is the device code of two trees the same, kernel by kernel?  No GPU needed.

    python tools/kernel_table_codeobj_diff.py asm  <tree> <outdir>      # compile <tree>'s HIP units with -save-temps
    python tools/kernel_table_codeobj_diff.py diff <old outdir> <new outdir>  > profiles/kernel_table_codeobj_diff.txt

`asm` takes the compile lines of <tree>/rust-raytracer_amd/build.py as they are (both libraries, every unit, the product's flags and
defines), adds -save-temps and keeps each unit's gfx950 assembly as <outdir>/<object name>.s.  `diff` compares, for every
function of every unit, the assembly body and the kernel's metadata record (VGPRs, SGPRs, spills, private segment, LDS, kernarg,
arguments).  Local labels carry the function's index within its unit, which moves with the emission order, so they are
renumbered in order of appearance; comments are dropped, and so is the directive that returns to the function's text section
after a kernel's descriptor (a kernel that became a template has a COMDAT section of its own).  A kernel must stay in its unit (UNIT_OF: old object name -> new) and
keep its mangled name, but for the AOV kernels, which are compared under the old -> new map of aov_new_name."""
import concurrent.futures
import importlib.util
import os
import re
import shutil
import subprocess
import sys

ASM_SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
# the units of the kernel sets were files of their own; now they are rt_kernel_set.hip compiled with -DRT_KERNEL_SET=<key >> 6>
UNIT_OF = {"rt_kernel_motion": "rt_kernel_set1", "rt_kernel_medium": "rt_kernel_set2", "rt_kernel_medium_motion": "rt_kernel_set3",
           "rt_kernel_solid": "rt_kernel_set4", "rt_kernel_solid_motion": "rt_kernel_set5", "rt_kernel_solid_medium": "rt_kernel_set6",
           "rt_kernel_solid_medium_motion": "rt_kernel_set7"}
AOV_ARGS = "N3rtc8DevSceneEjP15HIP_vector_typeIfLj4EE"


def aov_new_name(old):
    """rt_aov[_lens][_motion][_medium](...) -> rt_aov<LENS, MOTION, MEDIUM, false>; rt_aov_solid<L, MO, ME> -> rt_aov<L, MO, ME, true>"""
    m = re.fullmatch(r"_ZN3rtk\d+rt_aov((?:_lens)?)((?:_motion)?)((?:_medium)?)E" + AOV_ARGS, old)
    if m:
        return "_ZN3rtk6rt_aovI" + "".join("Lb%dE" % bool(g) for g in m.groups()) + "Lb0EEEv" + AOV_ARGS
    m = re.fullmatch(r"_ZN3rtk12rt_aov_solidI((?:Lb[01]E){3})EEv" + AOV_ARGS, old)
    if m:
        return "_ZN3rtk6rt_aovI" + m.group(1) + "Lb1EEEv" + AOV_ARGS
    return old


def compile_lines(tree):
    """the hipcc -c lines build.py's build_hip(force=True) would start, recorded instead of run"""
    spec = importlib.util.spec_from_file_location("rt_build_of_tree", os.path.join(tree, "rust-raytracer_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    lines = []

    class Recorded:
        def __init__(self, cmd, **kw):
            lines.append(cmd)

        def wait(self):
            return 0
    real = b.subprocess.Popen
    b.subprocess.Popen = Recorded
    try:
        b.build_hip(force=True)
    finally:
        b.subprocess.Popen = real
    return [c for c in lines if "-c" in c]


def asm(tree, outdir):
    os.makedirs(outdir, exist_ok=True)

    def one(cmd):
        name = os.path.splitext(os.path.basename(cmd[cmd.index("-o") + 1]))[0]
        src = cmd[cmd.index("-c") + 1]
        td = os.path.join(outdir, "tmp_" + name)   # (a directory per object: -save-temps names its files after the source)
        os.makedirs(td, exist_ok=True)
        cmd = cmd[:cmd.index("-o")] + ["-o", os.path.join(td, "x.o"), "-save-temps=obj"]
        subprocess.run(cmd, check=True, cwd=td)
        shutil.copy(os.path.join(td, os.path.splitext(os.path.basename(src))[0] + ASM_SUFFIX), os.path.join(outdir, name + ".s"))
        shutil.rmtree(td)
        return name
    with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        for name in pool.map(one, compile_lines(tree)):
            print("assembled", name, file=sys.stderr, flush=True)


def functions(text):
    """{symbol: (normalised body, normalised metadata record or None)} of one unit's assembly"""
    meta = {}
    if "amdhsa.kernels:" in text:
        for rec in re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")])[1:]:
            name = re.search(r"\.name:\s+(\S+)", rec).group(1)
            meta[name] = re.sub(r"^\s*\.(name|symbol):.*\n", "", rec, flags=re.M).replace(name, "@SELF").strip()
    out = {}
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        while not lines[i].startswith(name + ":"):
            i += 1
        body = []   # the instructions, a kernel's descriptor, .size, and the .set lines of the function's resource symbols
        while not lines[i].strip().startswith(".size"):
            body.append(lines[i])
            i += 1
        while lines[i].strip().startswith((".size", ".set", ";")) or not lines[i].strip():
            body.append(lines[i])
            i += 1
        labels = {}

        def renumber(mm):
            return labels.setdefault(mm.group(0), "%s%d" % (mm.group(1), len(labels)))
        norm = []
        for ln in body:
            ln = ln.split(";")[0].rstrip().replace(name, "@SELF")
            if ln and not re.match(r"\s*\.(text$|section\s+\.text)", ln):   # (back to .text after the descriptor: a template's is a COMDAT section)
                norm.append(re.sub(r"(\.L[A-Za-z_]+?)\d+(?:_\d+)?\b", renumber, ln))
        out[name] = ("\n".join(norm), meta.get(name))
    return out


def diff(old_dir, new_dir):
    differing = []
    n_mega = 0
    units = sorted(f[:-2] for f in os.listdir(old_dir) if f.endswith(".s"))
    new_units = sorted(f[:-2] for f in os.listdir(new_dir) if f.endswith(".s"))
    print("# old unit -> new unit: functions (kernels, rt_megakernel instantiations, AOV kernels under their new names)")
    for u in units:
        probe = "_probe" if u.endswith("_probe") else ""
        nu = UNIT_OF.get(u[:len(u) - len(probe)], u[:len(u) - len(probe)]) + probe
        if nu not in new_units:
            differing.append(f"{u}: no unit {nu} on the new side")
            continue
        new_units.remove(nu)
        old = functions(open(os.path.join(old_dir, u + ".s")).read())
        new = functions(open(os.path.join(new_dir, nu + ".s")).read())
        renamed = {aov_new_name(k): k for k in old}
        mega = sum("rt_megakernel" in k for k in old)
        n_mega += mega if not probe else 0
        print(f"{u} -> {nu}: {len(old)} -> {len(new)} functions ({sum(v[1] is not None for v in old.values())} -> "
              f"{sum(v[1] is not None for v in new.values())} kernels, {mega} -> {sum('rt_megakernel' in k for k in new)} rt_megakernel, "
              f"{sum(k != v for k, v in renamed.items())} AOV renamed)")
        for k in sorted(k for k, v in renamed.items() if k != v):
            print(f"  {renamed[k]} -> {k}")
        for k in sorted(set(renamed) | set(new)):
            if k not in new:
                differing.append(f"{nu}: {k} (was {renamed[k]}) is missing")
            elif k not in renamed:
                differing.append(f"{nu}: {k} is new")
            else:
                ob, om = old[renamed[k]]
                nb, nm = new[k]
                if ob != nb:
                    differing.append(f"{nu}: {k}: body differs")
                if om != nm:
                    differing.append(f"{nu}: {k}: metadata differs")
    for nu in new_units:
        differing.append(f"{nu}: no such unit on the old side")
    print(f"rt_megakernel instantiations per library: {n_mega}")
    print(f"{len(differing)} differing")
    for d in differing:
        print("  " + d)
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "asm":
        asm(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]))
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
