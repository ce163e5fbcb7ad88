#!/usr/bin/env python3
"""Register / spill / scratch figures of every kernel in librt_hip.so, from the compiler's own metadata.

    python tools/codeobj_stats.py [--brief] [extra hipcc flags ...]  > profiles/rNN_codeobj.txt

Compiles rt_hip_api.hip, rt_grid_build.hip (the device grid build) and rt_flat_build.hip (the flat primitives moved and their
structure refit or built anew, §24 and §26) for gfx950 with the product's flags (+ extras) and -save-temps into a scratch directory
and prints one line per kernel: VGPRs, SGPRs, spilled VGPRs / SGPRs, scratch bytes per lane, code size, and a static
instruction census of the megakernel instantiations (v_mov share: the copies at control-flow joins).
--brief: the register, spill and scratch figures alone, for before / after pairs that are compared line by line.  No GPU needed."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "rust-raytracer_amd", "csrc", "hip", f) for f in ("rt_hip_api.hip", "rt_grid_build.hip", "rt_flat_build.hip")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-DRT_WAVES_PER_EU=4"]


def demangle_mk(name):
    m = re.match(r"_ZN3rtk13rt_megakernelILb(\d)ELb(\d)ELb(\d)ELb(\d)(?:ELb(\d))?(?:ELb(\d))?(?:ELb(\d))?(?:ELb(\d))?(?:ELb(\d))?(?:ELb(\d))?EEEvNS_5KArgsE", name)
    if m:
        hl, simple, lds, wide, accum, lens, motion, medium, solid, quads = (int(x or 0) for x in m.groups())
        return (f"rt_megakernel<lights={hl}, simple_colour={simple}, lds_tables={lds}" + (", wide_tables=1" if wide else "")
                + (", accum=1" if accum else "") + (", lens=1" if lens else "") + (", motion=1" if motion else "") + (", medium=1" if medium else "")
                + (", solid=1" if solid else "") + (", quads=1" if quads else "") + ">")
    out = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return out.replace("(anonymous namespace)::", "").split("(")[0] if out else name


def main():
    extra = [x for x in sys.argv[1:] if x != "--brief"]
    print("# hipcc " + " ".join(FLAGS + extra))
    for src in SRCS:
        with tempfile.TemporaryDirectory() as td:
            subprocess.run(["hipcc", *FLAGS, *extra, "-shared", src, "-o", os.path.join(td, "x.so"), "-save-temps"], check=True, cwd=td,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            asm = open(os.path.join(td, os.path.splitext(os.path.basename(src))[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
        report(asm, "--brief" in sys.argv[1:])


def report(asm, brief=False):
    # metadata block: one YAML record per kernel
    meta = {}
    for rec in re.split(r"\n  - \.", asm[asm.index("amdhsa.kernels:"):]):
        f = dict(re.findall(r"\.?(\w+):\s+(\S+)", rec))
        if "name" in f and "vgpr_count" in f:
            meta[f["name"]] = f
    # static census per function body
    bodies = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\s*s_endpgm", asm, flags=re.S | re.M):
        bodies[m.group(1)] = m.group(2)
    for name, f in meta.items():
        line = (f"{demangle_mk(name):70s} vgpr {int(f['vgpr_count']):3d}  sgpr {int(f['sgpr_count']):3d}  vgpr_spill {int(f['vgpr_spill_count']):3d}  "
                f"sgpr_spill {int(f['sgpr_spill_count']):3d}  scratch {int(f['private_segment_fixed_size']):4d} B/lane")
        if brief:
            print(re.sub(r"  +", "  ", line))
            continue
        b = bodies.get(name)
        if "rtgb" in name:   # (the grid build's kernels: their static LDS too)
            line += f"  lds {int(f.get('group_segment_fixed_size', 0)):5d} B"
        if b and "megakernel" in name:
            ins = re.findall(r"^\s+([vsd][a-z0-9_]+|scratch_\w+|global_\w+|flat_\w+|buffer_\w+)\b", b, flags=re.M)
            v = [i for i in ins if i.startswith("v_")]
            line += (f"  | static: {len(ins)} instr, {len(v)} VALU, v_mov {sum(i.startswith('v_mov') for i in v)} ({100.0 * sum(i.startswith('v_mov') for i in v) / max(1, len(v)):.1f} % of VALU), "
                     f"v_cndmask {sum(i.startswith('v_cndmask') for i in v)}, scratch ld/st {sum(i.startswith('scratch_') for i in ins)}, "
                     f"v_xor_b32 {sum(i.startswith('v_xor_b32') for i in v)}, v_bitop3_b32 {sum(i.startswith('v_bitop3_b32') for i in v)}, "
                     f"v_mad_u64_u32 {sum(i.startswith('v_mad_u64_u32') for i in v)}")
        print(line)


if __name__ == "__main__":
    main()
