"""The whole table of which command lines `raytracer` accepts (csrc/host/cli_args.h), against tests/golden/cli_accept.json: the
decisions of the binary before the parser became a header of its own (tests/golden/make_cli_accept.py) over the full lattice of
twelve flag groups, each present or absent with a valid value, and a list of edge rows.  The header is run alone
(tests/cliargs/cli_args_main.cpp) over every row; about a hundred rows go through the real binary, which shows that main.cpp uses
that parser.  Each feature's own test file pins the rows of its flags besides."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rust-raytracer_amd", "raytracer")
MAIN = os.path.join(ROOT, "tests", "cliargs", "cli_args_main.cpp")
HEADER = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "host", "cli_args.h")


def fixture_rows():
    """[(argument list after argv[0], accepted, lattice index or None)]"""
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "cli_accept.json")))
    assert len(t["groups"]) == 12 and len(t["lattice"]) == 4096
    rows = []
    for k, c in enumerate(t["lattice"]):
        rows.append(([t["config"], t["output"]] + [a for i, g in enumerate(t["groups"]) if k >> i & 1 for a in g], c == "1", k))
    return rows + [(e["args"], e["accept"], None) for e in t["edges"]]


def run_parser(exe, rows, env=None):
    """the stand-alone program over the rows: ['usage' | 'accept <mode>'] per row"""
    assert not any("\t" in a or "\n" in a for args, _, _ in rows for a in args)
    text = "".join("\t".join(args) + "\n" for args, _, _ in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert len(out) == len(rows)
    return out


def expected_mode(args):
    """the seven modes as a function of which of --frames, --passes, --adaptive and --denoise are present (accepted rows
    only; a `--frames 0` that was accepted stands beside another mode's flag and counts as absent)"""
    has = {f: f in args for f in ("--passes", "--adaptive", "--denoise")}
    frames = [args[i + 1] for i, a in enumerate(args[:-1]) if a == "--frames"]
    animation = bool(frames) and frames[-1] not in ("0", "x", "")
    if has["--adaptive"]:
        return "adaptive"
    if has["--passes"]:
        return "progressive"
    if animation:
        return "denoised-animation" if has["--denoise"] else "animation"
    return "denoised-one-shot" if has["--denoise"] else "one-shot"


def check(rows, got):
    wrong = [(args, accept, g) for (args, accept, _), g in zip(rows, got) if (g != "usage") != accept]
    assert not wrong, (len(wrong), wrong[:10])
    modes = [(args, g) for (args, accept, _), g in zip(rows, got) if accept and g != "accept " + expected_mode(args)]
    assert not modes, (len(modes), modes[:10])


@pytest.fixture(scope="module")
def parser_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cliargs") / "cli_args_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", MAIN, "-o", exe], check=True, cwd=ROOT)
    return exe


def test_the_header_decides_every_row_as_the_fixture(parser_exe):
    rows = fixture_rows()
    assert len(rows) > 4096 + 60
    assert 0 < sum(a for _, a, _ in rows) < len(rows) // 4   # (most combinations are refused)
    check(rows, run_parser(parser_exe, rows))


def test_the_binary_decides_as_the_header(pkg, tmp_path):
    """every edge row and every 64th lattice row through the real binary, on a config path that does not exist: refused = the usage line
    and exit 0 before anything touches HIP; accepted = exit 101 with `Unable to read config file`"""
    rows = [r for r in fixture_rows() if r[2] is None or r[2] % 64 == 0]
    assert 90 <= len(rows) <= 200
    for args, accept, _ in rows:
        r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
        if accept:
            assert r.returncode == 101 and "Unable to read config file" in r.stderr and r.stdout == "", (args, r.returncode, r.stdout, r.stderr)
        else:
            assert r.returncode == 0 and r.stdout == "Usage: %s <config_file> <output_file>\n" % EXE and r.stderr == "", (args, r.returncode, r.stdout, r.stderr)


def test_the_header_has_no_hip_no_globals_and_no_io():
    src = open(HEADER).read()
    for word in ("hip", "rt_abi", "printf", "iostream", "fopen", "getenv", "static "):
        assert word not in src.replace("No HIP", ""), word
