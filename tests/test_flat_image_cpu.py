"""Images on flat primitives without a GPU: the host build of csrc/common/rt_flat_image.h against the restatement
(tests/flat_image_mini.py) bit for bit on tables of hits; the prepare kernel of rt_flat_build.hip compiled by g++ against the
kernel-language emulation, against the host path; the CPU build of the QUADS lane code against the restatement's frames; the
constant-image identity, which needs no restatement; the schema, its load errors and the round trip."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import flat_image_frames as IF
import flat_image_mini as IM
import flat_image_points as IP
import flat_image_sim as IS
import mini_oracle as M
from parity import assert_parity, pooled_atol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARTH = os.path.join(ROOT, "scenes", "data", "earth.jpg")
MOON = os.path.join(ROOT, "scenes", "data", "moon.jpg")
NONE = 0xFFFFFFFF
FILL = 0x7FF8DEADBEEF0000


@pytest.fixture(scope="module")
def sim(abi):
    return IS.load(abi)


# ------------------------------------------------------------------ the header against the restatement
@pytest.mark.parametrize("cls", IP.CLASSES)
def test_texel_of_the_host_build_is_the_restatements(sim, cls):
    """col, row and the index of 10^5 hits of the class, every bit; no index leaves its texture"""
    rec, ouvw, P = IP.table(cls)
    got = sim.texel(rec, ouvw, P)
    assert (got[:, 0] < rec["W"]).all() and (got[:, 1] < rec["H"]).all()
    assert np.array_equal(got[:, 2], rec["texel_off"] + got[:, 1] * rec["W"] + got[:, 0])
    recs = [(int(r["texel_off"]), int(r["W"]), int(r["H"]), int(r["wrap"]), tuple(float(x) for x in r["uv"])) for r in rec]
    f, p = ouvw.tolist(), P.tolist()
    want = np.array([IM.texel(recs[i], f[i][0:3], f[i][3:6], f[i][6:9], f[i][9:12], p[i]) for i in range(len(rec))], np.uint32)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (cls, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    if cls in ("triangle", "parallelogram", "tiling"):     # the class means something: many texels are reached
        assert len(np.unique(got[rec["W"] == 8][:, 0])) == 8 and len(np.unique(got[rec["H"] == 4][:, 1])) == 4
    if cls == "integer_edges":                             # -tiny in REPEAT wraps to column 0 / the bottom row, not past the edge
        assert ((got[:, 0] == 0) & (P[:, 0] < 0) & (P[:, 0] > -1e-10)).any()


def test_colour_of_every_byte(sim):
    """the three f32 of the colour: bytes / 255 through rt_div255f equal the IEEE quotient the restatement forms"""
    words = np.arange(256, dtype=np.uint32) | ((255 - np.arange(256, dtype=np.uint32)) << 8) | (((np.arange(256, dtype=np.uint32) * 7) % 256) << 16)
    got = sim.colour(words)
    px = np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255], axis=1).astype(np.uint8).reshape(-1)
    want = np.array([IM.colour(px, i) for i in range(256)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_cold_function_on_a_table_of_its_own(sim):
    """flat_image_albedo: record, frame, fetch — the restatement's colour of each hit; a record with W = 0 answers with a negative red"""
    rng = np.random.default_rng(4)
    tex = IF.texture_arrays()[0]
    tex4 = (tex[..., 0].astype(np.uint32) | (tex[..., 1].astype(np.uint32) << 8) | (tex[..., 2].astype(np.uint32) << 16)).reshape(-1)
    quv = np.array([0.3, -1.0, 2.0, 1.5, 0.2, 0.1, -0.3, 1.1, 0.4])
    rec = IS.records([8], [4], [2], [[-0.5, 0.1, 2.2, 0.3, 0.2, 1.9]])
    ab = rng.uniform(0, 1, (4000, 2))
    origin = np.tile(quv[:3] + 0.25, (4000, 1))            # (an entry away from its record's Q: the shutter's origin is the frame)
    P = origin + np.outer(ab[:, 0], quv[3:6]) + np.outer(ab[:, 1], quv[6:9])
    got = sim.albedo(rec, quv, tex4, origin, P)
    c = __import__("quad_mini").QuadConsts(quv[:3], quv[3:6], quv[6:9])
    r = (0, 8, 4, 2, tuple(rec["uv"][0]))
    want = np.array([IM.colour(tex.reshape(-1), IM.texel(r, tuple(o), c.u, c.v, c.w, tuple(p))[2]) for o, p in zip(origin, P)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert len(np.unique(got[:, 0])) > 20
    none = sim.albedo(IS.records([0], [0], [0], [[0.0] * 6]), quv, tex4, origin[:4], P[:4])
    assert (none[:, 0] < 0).all()


# ------------------------------------------------------------------ the prepare kernel against the host path
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """as tests/test_smooth_prepare_cpu.py builds it, behind the C interface of tests/flatimage/flat_images_emu.cpp"""
    hip_dir = os.path.join(ROOT, "rust-raytracer_amd", "csrc", "hip")
    hdr = open(os.path.join(hip_dir, "rt_flat_build.h")).read()
    decl = hdr[hdr.index("#if defined(__HIPCC__)"):].replace("#if defined(__HIPCC__)", "").replace("#include <hip/hip_runtime.h>", "").rsplit("#endif", 1)[0]
    body = open(os.path.join(hip_dir, "rt_flat_build.hip")).read().replace("#include <hip/hip_runtime.h>", "").replace('#include "rt_flat_build.h"', "")
    d = tmp_path_factory.mktemp("flat_images_emu")
    src = d / "emu.cpp"
    src.write_text('#include "hip/hip_runtime.h"\n#include "' + os.path.join(hip_dir, "rt_tables.h") + '"\n' + decl + body
                   + open(os.path.join(ROOT, "tests", "flatimage", "flat_images_emu.cpp")).read())
    so = d / "libflat_images_emu.so"
    subprocess.run(["g++", "-std=c++20", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-DRT_TEST_PROBES", "-Wno-unknown-pragmas",
                    "-I", os.path.join(ROOT, "tests", "flatupdate", "emu"), str(src), "-o", str(so), "-lpthread"], check=True)
    L = C.CDLL(str(so))
    P, u32 = C.c_void_p, C.c_uint32
    L.fie_device.argtypes = [P, u32, P, u32, P, P, P]
    L.fie_host.argtypes = [P, u32, P, u32, P, P, P]
    L.fie_host.restype = None
    return L


TEX_TABLE = np.array([(0, 8, 4, 1), (32, 5, 3, 1), (47, 1, 1, 1), (0, 7, 0, 2), (0, 9, 9, 3)], np.uint32)   # two usable ones it refuses


def _entries(abi, n=1000, seed=9):
    """n entries (several workgroups, the last one partial): every third without an image; kinds Lambertian and Metal"""
    rng = np.random.default_rng(seed)
    arr = (abi.RtFlatImage * n)()
    for k in range(n):
        arr[k] = abi.flat_image(int(rng.integers(0, 3)), tuple(rng.uniform(-3, 3, 6)), int(rng.integers(0, 2)), int(rng.integers(0, 2)))
        if k % 3 == 0:
            arr[k].tex_id = NONE
            arr[k].uv[2] = float("nan")       # (the rest of an entry without an image is ignored)
            arr[k].reserved = 5
    kind = rng.integers(0, 2, n).astype(np.uint32)         # RT_MAT_LAMBERTIAN = 0, RT_MAT_METAL = 1
    return arr, kind


def _device(emu, arr, kind):
    n = len(arr)
    out = np.full((n, 8), FILL, np.uint64)
    status = np.zeros(4, np.uint32)
    assert emu.fie_device(C.addressof(arr), n, TEX_TABLE.ctypes.data, len(TEX_TABLE), kind.ctypes.data, out.ctypes.data, status.ctypes.data) == 0
    return out, [int(x) for x in status]


def _host(emu, arr, kind):
    out = np.full((len(arr), 8), FILL, np.uint64)
    code = np.zeros(len(arr), np.int32)
    emu.fie_host(C.addressof(arr), len(arr), TEX_TABLE.ctypes.data, len(TEX_TABLE), kind.ctypes.data, out.ctypes.data, code.ctypes.data)
    return out, code


def test_device_path_table_equals_the_host_path_table(abi, emu):
    """byte for byte the host's records, 64 zero bytes for an entry without an image, the count; the restatement makes the same records"""
    assert C.sizeof(abi.RtFlatImage) == 64 and IS.REC.itemsize == 64
    arr, kind = _entries(abi)
    got, status = _device(emu, arr, kind)
    want, code = _host(emu, arr, kind)
    assert set(code.tolist()) == {IM.ABSENT, IM.PRESENT} and (code[::3] == IM.ABSENT).all() and not want[::3].any()
    assert np.array_equal(got, want) and status[1:] == [NONE, int((code == IM.PRESENT).sum()), 0]
    table = [tuple(int(x) for x in r) for r in TEX_TABLE]
    rec = want.view(IS.REC).reshape(-1)
    for k in range(len(arr)):
        c, r = IM.prepare(list(arr[k].uv), arr[k].tex_id, arr[k].wrap_s, arr[k].wrap_t, arr[k].reserved, table, int(kind[k]))
        assert c == code[k] and (int(rec[k]["texel_off"]), int(rec[k]["W"]), int(rec[k]["H"]), int(rec[k]["wrap"])) == r[:4], k
        assert np.array_equal(np.array(r[4]).view(np.uint64), rec[k]["uv"].view(np.uint64)), k


def _break(abi, im, what):
    if what == "nan uv":
        im.uv[4] = float("nan")
    elif what == "inf uv":
        im.uv[0] = float("-inf")
    elif what == "tex_id":
        im.tex_id = len(TEX_TABLE)
    elif what == "texture size":
        im.tex_id = 3
    elif what == "texture far":
        im.tex_id = 4
    elif what == "wrap_s":
        im.wrap_s = 2
    elif what == "wrap_t":
        im.wrap_t = 7
    elif what == "reserved":
        im.reserved = 1


REFUSALS = [("nan uv", IM.BAD_UV), ("inf uv", IM.BAD_UV), ("tex_id", IM.BAD_TEX_ID), ("texture size", IM.BAD_TEX_SIZE), ("texture far", IM.BAD_TEX_FAR),
            ("wrap_s", IM.BAD_WRAP), ("wrap_t", IM.BAD_WRAP), ("reserved", IM.BAD_RESERVED), ("material", IM.BAD_MATERIAL)]


@pytest.mark.parametrize("what,code", REFUSALS)
def test_each_refusal_names_the_lowest_bad_entry(abi, emu, what, code):
    arr, kind = _entries(abi)
    kind = kind.copy()
    bad_at = [700, 40, 301] if what != "reserved" else [998]
    assert all(k % 3 for k in bad_at)
    for k in bad_at:
        if what == "material":
            kind[k] = abi.RT_MAT_GLASS if k != 40 else abi.RT_MAT_CHECKER
        else:
            _break(abi, arr[k], what)
    got, status = _device(emu, arr, kind)
    assert status[1] == min(bad_at) and status[0] == code, (what, status)
    assert (got[bad_at] == FILL).all()                                    # a refused entry writes nothing
    assert _host(emu, arr, kind)[1][bad_at].tolist() == [code] * len(bad_at)
    table = [tuple(int(x) for x in r) for r in TEX_TABLE]
    k = min(bad_at)
    assert IM.prepare(list(arr[k].uv), arr[k].tex_id, arr[k].wrap_s, arr[k].wrap_t, arr[k].reserved, table, int(kind[k]))[0] == code
    # two classes at once: the lowest entry wins, with ITS reason
    arr[7].wrap_s = 3
    _, status = _device(emu, arr, kind)
    assert status[:2] == [IM.BAD_WRAP, 7]


def test_the_texture_table_of_a_scene(abi, host, sim):
    """what creation uploads for the prepare kernel: build_texels' layout, the decoded sizes"""
    w = IF.world(host, abi, "poster")
    got = sim.tex_table(w["sc"].c)
    assert got.tolist() == [[0, 8, 4, 1], [32, 5, 3, 1], [47, 1, 1, 1]]
    assert [tuple(r) for r in got.tolist()] == IM.tex_table([(8, 4, 96), (5, 3, 45), (1, 1, 3)])
    far = IM.tex_table([(8, 4, 96), (65536, 32768, 3 * 2 ** 31), (1, 1, 3), (2, 2, 11)])
    assert [r[3] for r in far] == [1, 3, 3, 2]


# ------------------------------------------------------------------ the lane code against the restatement
@pytest.mark.parametrize("case", IF.PARITY_CASES)
def test_lane_code_frames_against_the_restatement(abi, oracle, host, sim, case):
    """tests/parity.py's bar with the exact segment count; the structure gives the scan's frame bit for bit; the frame without images differs"""
    w = IF.world(host, abi, case)
    rc, rgb, lin, segs, info = sim.render(w)
    assert rc == 0 and info[0] & IS.FLAT_IMAGES_BIT and info[1] == sum(im.tex_id != NONE for im in w["images"]) > 0, info
    m = IF.mini_frame(oracle, abi, host, case)
    print(f"{case}: max |linear diff| {float(np.abs(lin - m['lin']).max()):.3g}, segments {segs} mini {m['segments']} - {m['discarded']}, lookups {m['hits']}")
    assert_parity(rgb, lin, m["rgb"], m["lin"], case, atol=pooled_atol(IF.SPP))
    assert segs == m["segments"] - m["discarded"]
    assert m["hits"] and min(m["hits"].values()) > 20, m["hits"]
    rc, rgb2, lin2, segs2, info2 = sim.render(w, flat_bvh=True)
    assert rc == 0 and info2[0] & IS.FLAT_BVH_BIT and segs2 == segs
    assert np.array_equal(rgb, rgb2) and np.array_equal(lin.view(np.uint32), lin2.view(np.uint32))
    plain = dict(w, images=None)
    rc, _, lin3, _, info3 = sim.render(plain)
    assert rc == 0 and not info3[0] & IS.FLAT_IMAGES_BIT and not np.array_equal(lin.view(np.uint32), lin3.view(np.uint32))
    if case == "image_and_emit":           # emission wins: the panel's image changes nothing
        k = int(np.flatnonzero((w["emit"] != 0).any(axis=1))[0])
        assert w["images"][k].tex_id != NONE and k not in m["hits"]
        other = (abi.RtFlatImage * len(w["images"]))(*w["images"])
        other[k] = abi.flat_image()
        rc, _, lin4, segs4, _ = sim.render(dict(w, images=other))
        assert rc == 0 and segs4 == segs and np.array_equal(lin.view(np.uint32), lin4.view(np.uint32))


@pytest.mark.parametrize("case", ["poster", "moving_quad", "image_and_emit"])
def test_first_hit_records_are_the_restatements(abi, oracle, host, sim, case):
    w = IF.world(host, abi, case)
    want = IF.mini(oracle, abi, w).aovs(IF.SPP)
    rc, got = sim.aovs(w, IF.SPP)
    assert rc == 0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    rc, plain = sim.aovs(dict(w, images=None), IF.SPP)
    assert rc == 0 and not np.array_equal(plain.view(np.uint32), got.view(np.uint32))


def test_an_entry_list_without_any_image_is_the_scene_without_the_call(abi, host, sim):
    w = IF.world(host, abi, "poster")
    none = (abi.RtFlatImage * len(w["quads"]))(*[abi.flat_image() for _ in w["quads"]])
    a, b = sim.render(dict(w, images=none)), sim.render(dict(w, images=None))
    assert a[0] == 0 and a[4][0] == b[4][0] and not a[4][0] & IS.FLAT_IMAGES_BIT
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and a[3] == b[3]


def test_constant_image_identity(abi, host, sim):
    """a one-colour image c on a Lambertian wall: the frame is, bit for bit, the frame of the scene without images whose wall has
    albedo = c / 255 — a path that never enters the new function"""
    div255 = lambda b: float(sim.colour(np.array([b], np.uint32))[0, 0])
    assert div255(200) == float(M.F(200) / M.F(255.0))
    a, b = IF.constant_pair(host, abi, div255)
    ra, rb = sim.render(a), sim.render(b)
    assert ra[0] == 0 and rb[0] == 0 and ra[4][0] & IS.FLAT_IMAGES_BIT and not rb[4][0] & IS.FLAT_IMAGES_BIT
    assert ra[3] == rb[3] > 0
    assert np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2].view(np.uint32), rb[2].view(np.uint32))
    ga, gb = sim.aovs(a, IF.SPP), sim.aovs(b, IF.SPP)
    assert np.array_equal(ga[1].view(np.uint32), gb[1].view(np.uint32))
    grey = dict(b, quads=(type(b["quads"][0]) * len(b["quads"]))(*b["quads"]))
    grey["quads"][2].albedo[0] = 0.5
    assert not np.array_equal(sim.render(grey)[2].view(np.uint32), rb[2].view(np.uint32))     # (the wall is in the picture)


# ------------------------------------------------------------------ the schema
def _file(objs, **top):
    cfg = IF._cfg(objs)
    cfg.update(top)
    return cfg


def _poster(**image):
    o = IF._quad((-2, -1, -2), (4, 0, 0), (0, 4, 0), IF.WHITE)
    o["image"] = dict({"pixels": EARTH}, **image)
    return o


def _loads(host, cfg):
    return host.Scene.loads(json.dumps(cfg))


def test_schema_quad_triangle_box_mesh(abi, host):
    tri = {"triangle": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "material": IF._metal((0.9, 0.9, 0.9), 0.1), "image": {"pixels": MOON, "wrap": ["clamp", "repeat"]},
           "uvs": [[0.1, 0.2], [0.9, 0.25], [0.5, 1.5]]}
    mesh = {"mesh": {"vertices": [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.3]], "faces": [[0, 1, 2], [1, 3, 2]], "uvs": [[0, 0], [1, 0], [0, 1], [1, 1]]},
            "material": IF.WHITE, "image": {"pixels": EARTH, "wrap": "clamp"}}
    box = dict(IF._box((-1, -1, -1), (1, 1, 1), IF.WHITE), image={"pixels": MOON})
    quad = dict(_poster(), uvs=[[0, 0], [2, 0], [0, 3]])
    plain = IF._quad((0, 0, 0), (1, 0, 0), (0, 1, 0), IF.WHITE)
    sc = _loads(host, _file([IF._obj((0, 0, 0), 1.0, IF.WHITE), quad, plain, tri, mesh, box, _poster()]))
    im = sc.flat_images()
    assert len(im) == len(sc.quads()) == 1 + 1 + 1 + 2 + 6 + 1
    assert sc.c.n_textures == 2                                           # (one decode per file: the cache of the Texture materials)
    earth, moon = im[0].tex_id, im[2].tex_id
    assert {earth, moon} == {0, 1} and (sc.c.textures[earth].width, sc.c.textures[earth].height) != (0, 0)
    assert list(im[0].uv) == [0, 0, 2, 0, 0, 3] and (im[0].wrap_s, im[0].wrap_t) == (0, 0)
    assert im[1].tex_id == NONE
    assert list(im[2].uv) == [0.1, 0.2, 0.9, 0.25, 0.5, 1.5] and (im[2].wrap_s, im[2].wrap_t) == (1, 0)
    assert list(im[3].uv) == [0, 0, 1, 0, 0, 1] and list(im[4].uv) == [1, 0, 1, 1, 0, 1] and im[3].tex_id == earth and (im[4].wrap_s, im[4].wrap_t) == (1, 1)
    for k in range(5, 11):
        assert im[k].tex_id == moon and list(im[k].uv) == [0, 0, 1, 0, 0, 1]
    assert im[11].tex_id == earth and list(im[11].uv) == [0, 0, 1, 0, 0, 1]
    assert all(x.reserved == 0 for x in im)
    assert _loads(host, _file([plain])).flat_images() is None
    # load -> write -> load: bit for bit, and the text is a fixed point
    text = sc.to_json()
    again = _loads(host, json.loads(text))
    assert bytes(again.flat_images()) == bytes(im) and again.to_json() == text
    assert bytes(again.quads()) == bytes(sc.quads())
    assert "image" not in _loads(host, _file([plain])).to_json() and "uvs" not in _loads(host, _file([plain, _poster()])).to_json()


LOAD_ERRORS = [
    ("image on a sphere", lambda: dict(IF._obj((0, 0, 0), 1.0, IF.WHITE), image={"pixels": EARTH}), "a sphere takes no `image`"),
    ("uvs without image", lambda: dict(IF._quad((0, 0, 0), (1, 0, 0), (0, 1, 0), IF.WHITE), uvs=[[0, 0], [1, 0], [0, 1]]), "`uvs` without `image`"),
    ("uvs on a box", lambda: dict(IF._box((-1, -1, -1), (1, 1, 1), IF.WHITE), image={"pixels": EARTH}, uvs=[[0, 0], [1, 0], [0, 1]]), "a box takes no uvs"),
    ("non-finite", lambda: dict(_poster(), uvs=[[0, 0], [12345.5, 0], [0, 1]]), "uv 1"),      # (written as 1e999 below: JSON has no infinity)
    ("unknown wrap", lambda: _poster(wrap="mirror"), "unknown wrap `mirror`"),
    ("unknown wrap in a pair", lambda: _poster(wrap=["repeat", "edge"]), "unknown wrap `edge`"),
    ("glass", lambda: dict(_poster(), material=IF.GLASS), "Lambertian or Metal"),
    ("checker", lambda: dict(_poster(), material={"Checker": {"even": [1, 1, 1], "odd": [0, 0, 0], "scale": 1.0}}), "Lambertian or Metal"),
    ("two uvs", lambda: dict(_poster(), uvs=[[0, 0], [1, 0]]), "expected 3 uvs"),
    ("mesh count", lambda: {"mesh": {"vertices": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "faces": [[0, 1, 2]], "uvs": [[0, 0], [1, 0]]}, "material": IF.WHITE,
                            "image": {"pixels": EARTH}}, "mesh.uvs: expected 3 uvs"),
    ("mesh without uvs", lambda: {"mesh": {"vertices": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "faces": [[0, 1, 2]]}, "material": IF.WHITE, "image": {"pixels": EARTH}},
     "needs `uvs`"),
    ("no pixels", lambda: dict(_poster(), image={"wrap": "clamp"}), "missing field `pixels`"),
]


@pytest.mark.parametrize("what,make,text", LOAD_ERRORS, ids=[e[0] for e in LOAD_ERRORS])
def test_load_errors_name_the_object(host, what, make, text):
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(json.dumps(_file([IF._obj((0, 5, 0), 1.0, IF.WHITE), make()])).replace("12345.5", "1e999"))
    assert "objects[1]" in str(e.value) and text in str(e.value), str(e.value)


@pytest.mark.parametrize("key", ["image", "uvs"])
def test_duplicate_keys(host, key):
    text = json.dumps(_file([dict(_poster(), uvs=[[0, 0], [1, 0], [0, 1]])]))
    dup = {"image": ',"image":{"pixels":"x.jpg"}', "uvs": ',"uvs":[[0,0],[1,0],[0,1]]'}[key]
    at = text.index('"material"')
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(text[:at] + dup[1:] + "," + text[at:])
    assert "objects[0]" in str(e.value) and f"duplicate field `{key}`" in str(e.value), str(e.value)


def test_texture_material_on_a_flat_primitive_stays_refused(host):
    o = IF._quad((0, 0, 0), (1, 0, 0), (0, 1, 0), {"Texture": {"albedo": [1, 1, 1], "pixels": EARTH, "width": 8, "height": 4, "h_offset": 0.0}})
    with pytest.raises(host.RtError) as e:
        _loads(host, _file([o]))
    assert "a quad cannot be a Texture" in str(e.value)
