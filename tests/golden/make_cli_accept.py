"""Generator of cli_accept.json: which command lines `raytracer` accepts.

    python tests/golden/make_cli_accept.py <path to the raytracer binary>

The committed cli_accept.json was written by this script run on the binary of the commit BEFORE the argument parser moved into
csrc/host/cli_args.h (main.cpp's one boolean expression over fifteen variables), so it records that binary's decisions, not the
new parser's.  Run it on a later binary only to extend the table on purpose.

Every row names a config file that does not exist.  A refused row prints the usage line and exits 0 before anything touches the
GPU; an accepted row exits 101 with `Unable to read config file`.  Anything else stops the generator.

The table: the full lattice over GROUPS (row k holds group i if bit i of k is set, in the order of GROUPS, after CONFIG and OUTPUT),
stored as one string of 4096 characters, '1' = accepted; and EDGES, whole argument lists with their decision."""
import json
import os
import subprocess
import sys

CONFIG, OUTPUT = "no_such_config.json", "out.png"
GROUPS = [["--frames", "3"], ["--orbit", "5"], ["--shutter", "0.5"], ["--passes", "2"], ["--adaptive", "0.1"], ["--min-spp", "4"],
          ["--denoise"], ["--flat-bvh"], ["--flat-frames", "P_"], ["--temporal-surface"], ["--temporal-alpha", "0.2"],
          ["--temporal-alpha-specular", "0.5"]]
ANIM = ["--frames", "3"]
TEMPORAL = ["--frames", "3", "--orbit", "5", "--denoise"]


def edges():
    rows = []
    # each value malformed or out of range, beside the flags that would make a good value acceptable
    for bad in ("x", "1.5", "-0.1", "0.5x", ""):
        rows.append(ANIM + ["--shutter", bad])
        rows.append(TEMPORAL + ["--temporal-alpha", bad])
        rows.append(TEMPORAL + ["--temporal-surface", "--temporal-alpha-specular", bad])
    for bad in ("x", "0", "-1", "2x", "", "1.5"):
        rows.append(["--passes", bad])
        rows.append(["--adaptive", "0.1", "--min-spp", bad])
    rows += [["--adaptive", "0.1", "--min-spp", "4294967295"], ["--adaptive", "0.1", "--min-spp", "4294967296"]]
    for bad in ("x", "-1", "inf", "nan", "", "0.1x", "0"):
        rows.append(["--adaptive", bad])
    rows += [ANIM + ["--orbit", "x"], ANIM + ["--orbit", ""], ANIM + ["--shutter", "0"], ANIM + ["--shutter", "1"]]
    # each flag last, without its value
    rows += [["--frames"], ANIM + ["--orbit"], ANIM + ["--shutter"], ["--passes"], ["--adaptive"], ["--adaptive", "0.1", "--min-spp"],
             ANIM + ["--flat-frames"], TEMPORAL + ["--temporal-alpha"], TEMPORAL + ["--temporal-surface", "--temporal-alpha-specular"]]
    # the two flags that may not be repeated; the others: the last occurrence wins
    rows += [["--flat-bvh", "--flat-bvh"], ANIM + ["--flat-bvh", "--flat-bvh"], ANIM + ["--flat-frames", "P_", "--flat-frames", "Q_"],
             ANIM + ["--flat-frames", ""], ["--passes", "2", "--passes", "3"], ["--passes", "2", "--passes", "0"],
             ANIM + ["--shutter", "2", "--shutter", "0.5"], ["--denoise", "--denoise"]]
    # --frames through atoi
    rows += [["--frames", "x"], ["--frames", "0"], ["--frames", "3", "--frames", "0"], ["--frames", "0", "--frames", "3"],
             ["--frames", "-2"], ["--frames", "0", "--flat-bvh"], ["--frames", "3x"]]
    for mode in (["--passes", "2"], ["--adaptive", "0.1"], ["--denoise"]):
        rows += [["--frames", "0"] + mode, ["--frames", "-2"] + mode, ["--frames", "3", "--frames", "0"] + mode]
    rows += [["--frames", "-2", "--orbit", "5", "--denoise"], ["--frames", "0", "--orbit", "5", "--denoise"]]
    # an unknown flag, a stray word
    rows += [["--bogus"], ["--bogus", "1"], ["extra"], ANIM + ["--bogus"], ["--flat-bvh", "extra"]]
    return [[], [CONFIG]] + [[CONFIG, OUTPUT] + r for r in rows]   # ... and no arguments at all, or the config alone


def lattice_args(k):
    return [CONFIG, OUTPUT] + [a for i, g in enumerate(GROUPS) if k >> i & 1 for a in g]


def decide(exe, args, cwd):
    r = subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=60)
    if r.returncode == 0 and r.stdout.startswith("Usage: ") and not r.stderr:
        return False
    if r.returncode == 101 and "Unable to read config file" in r.stderr and not r.stdout:
        return True
    raise SystemExit("neither refused nor accepted: %r -> %d %r %r" % (args, r.returncode, r.stdout, r.stderr))


def main():
    exe = os.path.abspath(sys.argv[1])
    here = os.path.dirname(os.path.abspath(__file__))   # (no file called CONFIG here)
    table = {"config": CONFIG, "output": OUTPUT, "groups": GROUPS,
             "lattice": "".join("1" if decide(exe, lattice_args(k), here) else "0" for k in range(1 << len(GROUPS))),
             "edges": [{"args": a, "accept": decide(exe, a, here)} for a in edges()]}
    with open(os.path.join(here, "cli_accept.json"), "w") as f:
        head = ",\n".join("%s: %s" % (json.dumps(k), json.dumps(table[k])) for k in ("config", "output", "groups", "lattice"))
        f.write("{%s,\n\"edges\": [\n%s\n]}\n" % (head, ",\n".join(json.dumps(e) for e in table["edges"])))   # (one edge row per line)
    print("%d lattice rows (%d accepted), %d edge rows (%d accepted)" % (len(table["lattice"]), table["lattice"].count("1"), len(table["edges"]),
                                                                        sum(e["accept"] for e in table["edges"])))


if __name__ == "__main__":
    main()
