"""Participating media without a GPU: the schema, rt_neg_log built for the host, and rt_tables.h + hit_world_grid with
media (tests/lanesim, a g++ build) against a brute force of the contract restated in tests/medium_mini.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import adversarial_rays as AR
import lane_sim
import medium_mini as MM
import mini_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVER = os.path.join(ROOT, "scenes", "cfg2_cover_1200x800_spp128.json")
FOG_SCENE = os.path.join(ROOT, "scenes", "cover_fog_1200x800_spp128.json")


def _cfg(material, radius=1.0, extra=""):
    return ('{"width":8,"height":8,"samples_per_pixel":1,"max_depth":2,"sky":{"texture":""},"camera":{"look_from":{"x":0.0,"y":0.0,"z":5.0},'
            '"look_at":{"x":0.0,"y":0.0,"z":0.0},"vup":{"x":0.0,"y":1.0,"z":0.0},"vfov":40.0,"aspect":1.0},"objects":['
            '{"center":{"x":0.0,"y":-100.0,"z":0.0},"radius":99.0,"material":{"Lambertian":{"albedo":[0.5,0.5,0.5]}}},'
            '{"center":{"x":0.0,"y":0.0,"z":0.0}' + extra + ',"radius":' + radius + ',"material":' + material + '}]}')


def test_schema_loads_and_round_trips_the_variant(host, abi):
    sc = host.Scene.loads(_cfg('{"Medium":{"albedo":[0.25,0.5,0.75],"density":1.5}}', "2.0"))
    s = sc.c.spheres[1]
    assert abi.RT_MAT_MEDIUM == 5 and s.kind == abi.RT_MAT_MEDIUM and s.fuzz_or_ior == 1.5 and list(s.albedo) == [0.25, 0.5, 0.75]
    text = sc.to_json()
    obj = json.loads(text)["objects"][1]
    assert obj["material"] == {"Medium": {"albedo": [0.25, 0.5, 0.75], "density": 1.5}} and obj["radius"] == 2.0
    again = host.Scene.loads(text)
    assert again.to_json() == text and again.c.spheres[1].kind == abi.RT_MAT_MEDIUM
    # the sequence form of the payload, as for every struct variant
    seq = host.Scene.loads(_cfg('{"Medium":[[0.25,0.5,0.75],1.5]}', "2.0"))
    assert seq.to_json() == text


@pytest.mark.parametrize("material,radius,msg", [
    ('{"Medium":{"albedo":[0.5,0.5,0.5],"density":0.0}}', "1.0", "density"),
    ('{"Medium":{"albedo":[0.5,0.5,0.5],"density":-1.0}}', "1.0", "density"),
    ('{"Medium":{"albedo":[0.5,0.5,0.5],"density":1e999}}', "1.0", "density"),
    ('{"Medium":{"albedo":[0.5,0.5,0.5],"density":1.0}}', "0.0", "radius"),
    ('{"Medium":{"albedo":[0.5,0.5,0.5],"density":1.0}}', "-1.0", "radius"),
    ('{"Medium":{"albedo":[0.5,0.5,0.5],"density":1.0,"density":2.0}}', "1.0", "duplicate field `density`"),
    ('{"Medium":{"albedo":[0.5,0.5,0.5],"albedo":[0.5,0.5,0.5],"density":1.0}}', "1.0", "duplicate field `albedo`"),
])
def test_schema_errors_name_the_object(host, material, radius, msg):
    with pytest.raises(host.RtError) as e:
        host.Scene.loads(_cfg(material, radius))
    assert "objects[1]" in str(e.value) and msg in str(e.value), str(e.value)


def test_old_scenes_load_and_serialize_as_before(host, abi):
    """a scene without a medium is the scene it was: no sphere of the new kind, the same JSON out"""
    for path in ("scenes/cfg2_cover_1200x800_spp128.json", "scenes/cfg1_test_800x600_spp16.json", "scenes/cover_motion_1200x800_spp128.json"):
        sc = host.Scene.load(os.path.join(ROOT, path))
        assert all(sc.c.spheres[i].kind <= abi.RT_MAT_LIGHT for i in range(sc.c.n_spheres))
        assert '"Medium"' not in sc.to_json()
        if "Texture" not in sc.to_json():   # (a texture serializes as the reference's placeholder path: not loadable again)
            assert host.Scene.loads(sc.to_json()).to_json() == sc.to_json()


@pytest.fixture(scope="module")
def medium_walk(abi):
    return lane_sim.load(abi)


# rt_neg_log's error against the platform's log, measured on the argument set below: 1.000 ulp at worst.  The routine's
# own analysis promises below 1 ulp; asserted with one ulp of margin.
NEG_LOG_MAX_ULP = 2.0


def test_neg_log_bits_accuracy_and_zero(medium_walk):
    """the host build of rt_neg_log is the Python restatement bit for bit on 10^6 arguments 1 - k 2^-53 (random k over every
    magnitude, the smallest and the largest k) and the extremes; within NEG_LOG_MAX_ULP of math.log; +0.0 at 1.0"""
    rng = np.random.default_rng(1503)
    k = np.concatenate([rng.integers(1, 1 << 53, 600_000, dtype=np.uint64),
                        (rng.integers(1, 1 << 53, 300_000, dtype=np.uint64) >> rng.integers(0, 52, 300_000).astype(np.uint64)) | np.uint64(1),
                        np.arange(1, 50_001, dtype=np.uint64), np.uint64((1 << 53) - 1) - np.arange(0, 50_000, dtype=np.uint64)])
    x = 1.0 - k.astype(np.float64) * 2.0 ** -53      # (exact: k < 2^53, and 1 - k 2^-53 is a multiple of 2^-53 below 1)
    x = np.concatenate([x, [2.0 ** -53, 1.0 - 2.0 ** -53, 1.0, 0.5, 2.0 ** -0.5, np.nextafter(2.0 ** -0.5, 0.0)]])
    assert len(x) >= 1_000_000 and (x > 0.0).all()
    out = medium_walk.medium_neg_log_v(x)
    worst = 0.0
    for xi, oi in zip(x.tolist(), out.tolist()):
        r = MM.neg_log(xi)
        assert r == oi and math.copysign(1.0, r) == math.copysign(1.0, oi), (xi, r, oi)
        if xi != 1.0:
            ref = -math.log(xi)
            worst = max(worst, abs(oi - ref) / math.ulp(ref))
    print(f"rt_neg_log: worst error against math.log {worst:.3f} ulp over {len(x)} arguments")
    assert worst <= NEG_LOG_MAX_ULP, worst
    res = medium_walk.medium_neg_log_v(np.array([1.0]))
    assert res[0] == 0.0 and math.copysign(1.0, res[0]) == 1.0 and math.copysign(1.0, MM.neg_log(1.0)) == 1.0


def _inside_rays(rng, centres, radii, media, count):
    """rays whose origin lies deep inside a medium (within 0.4 r of its centre: cells fully inside the ball for the big ones), short
    and long directions"""
    rays = np.zeros((count, 6))
    for k in range(count):
        j = int(media[k % len(media)])
        n = rng.standard_normal(3); n /= np.linalg.norm(n)
        rays[k, :3] = centres[j] + n * radii[j] * rng.uniform(0.0, 0.4)
        rays[k, 3:] = rng.standard_normal(3) * 10.0 ** rng.uniform(-2, 2)
    return rays


def _through_rays(rng, centres, radii, media, count):
    """rays from outside aimed through the heart of a medium: with a small density the candidate lies several cells past the first
    cell that lists the sphere"""
    rays = np.zeros((count, 6))
    for k in range(count):
        j = int(media[k % len(media)])
        n = rng.standard_normal(3); n /= np.linalg.norm(n)
        o = centres[j] + n * radii[j] * rng.uniform(1.5, 6.0)
        rays[k, :3] = o
        rays[k, 3:] = (centres[j] + rng.uniform(-0.3, 0.3, 3) * radii[j] - o) * rng.uniform(0.2, 2.0)
    return rays


WALK_WORLDS = {
    # (adversarial world, moving, environment): static / moving media, the packed tables and the wide ones
    "static": (0, False, {}),
    "static_ground": (1, False, {}),
    "big_radii": (3, False, {}),
    "moving": (0, True, {}),
    "moving_layer": (4, True, {}),
    "wide_tables": (0, False, {"RT_GRID_WIDE": "1"}),
    "thin_cells": (3, False, {"RT_GRID_N": "48,48,48"}),
}


@pytest.mark.parametrize("name", sorted(WALK_WORLDS))
def test_grid_walk_with_media_equals_brute_force(abi, medium_walk, monkeypatch, name):
    """hit_world_grid with a MediumCtx (CPU build) against the brute force of the contract, bit for bit on (t, index): the ray families
    of tests/adversarial_rays.py, rays that start deep inside a medium, and rays whose candidate lies cells past the first listing"""
    wi, moving, env = WALK_WORLDS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(9100 + sorted(WALK_WORLDS).index(name))
    sc, spheres, n = AR.adversarial_world(abi, rng, wi)
    sc.seed = 0x1234567 + wi
    tot = len(spheres)
    # a quarter of the ordinary spheres become media (positive radius), some thin and some dense; three of them are made BIG so
    # that they cover many cells, interior ones included
    media = [i for i in range(n) if i % 4 == 1]
    for i in media:
        spheres[i].radius = abs(spheres[i].radius)
        spheres[i].kind = abi.RT_MAT_MEDIUM
        spheres[i].fuzz_or_ior = float(10.0 ** rng.uniform(-1.5, 1.5))
        spheres[i].albedo[:] = [0.5, 0.5, 0.5]
    for i in media[:3]:
        spheres[i].radius = spheres[i].radius * 4.0 + 1.0
        spheres[i].fuzz_or_ior = float(rng.uniform(0.05, 0.3))
    c0, radii = AR.sphere_arrays(spheres, tot)
    dens = np.array([spheres[i].fuzz_or_ior if spheres[i].kind == abi.RT_MAT_MEDIUM else 0.0 for i in range(tot)])
    c1 = c0.copy()
    if moving:
        for i in range(n):
            if i % 3 != 2:
                c1[i] = c0[i] + rng.uniform(-0.7, 0.7, 3)
    c1c = np.ascontiguousarray(c1) if moving else None
    rc, info, listed, is_large = medium_walk.medium_tables(sc, c1c)
    assert rc == 0
    assert info[0] == len(media) and info[1] > 0, "the world must be gridded and know its media"
    assert bool(info[6]) == ("RT_GRID_WIDE" in env)
    # interior cells are kept: a big static medium in the grid is listed in about as many cells as its ball overlaps
    if not moving:
        cell = (c0[:n].max(0) - c0[:n].min(0) + 2 * np.abs(radii[:n]).max()) / info[1:4]
        for i in media[:3]:
            if not is_large[i]:
                ball_cells = 4.0 / 3.0 * math.pi * radii[i] ** 3 / float(np.prod(cell))
                assert listed[i] >= 0.5 * ball_cells, (i, listed[i], ball_cells)
    dv = np.where(c1 == c0, -0.0, c1 - c0)
    blocks = []
    for tau in ([0.0] if not moving else [0.0, 1.0 - 2.0 ** -24, float(np.float32(rng.integers(0, 1 << 24) * 2.0 ** -24))]):
        ct = c0 + dv * np.float64(tau)
        moved = (abi.RtSphere * tot)()
        C.memmove(moved, spheres, C.sizeof(moved))
        for i in range(tot):
            moved[i].center[:] = list(ct[i])
        per = 84 if moving else 210
        rays = np.concatenate([AR.ray_table(rng, moved, n, per, list(range(AR.FAMILIES)))[0],
                               _inside_rays(rng, ct, radii, media, per // 3), _through_rays(rng, ct, radii, media, per // 3)])
        blocks.append((tau, ct, rays))
    rays = np.ascontiguousarray(np.concatenate([b[2] for b in blocks]))
    tau_v = np.concatenate([np.full(len(b[2]), b[0], np.float32) for b in blocks])
    nodes = np.ascontiguousarray(rng.choice(np.array([0, 1, 7, 0x80000002, 0xFFFFFFFE], np.uint32), len(rays)))
    rc, best, t, work = medium_walk.hit_world_v(sc, rays, c1c, tau=tau_v, node=nodes)
    assert rc == 0
    k = 0
    n_medium_hits = 0
    for tau, ct, rr in blocks:
        # (the brute force addresses ray i of the whole table: pixel = its index there)
        idx = np.arange(k, k + len(rr))
        bb, tb = _brute_at(rr, idx, nodes[k:k + len(rr)], ct, radii, dens, sc.seed)
        g_b, g_t = best[k:k + len(rr)], t[k:k + len(rr)]
        bad = np.nonzero((g_b != bb) | (g_t.view(np.uint64) != tb.view(np.uint64)))[0]
        assert len(bad) == 0, (name, tau, bad[:5], g_b[bad[:5]], bb[bad[:5]], g_t[bad[:5]], tb[bad[:5]])
        n_medium_hits += int((dens[np.maximum(bb, 0)] > 0.0)[bb >= 0].sum())
        k += len(rr)
    assert n_medium_hits > 0.05 * len(rays), n_medium_hits       # (the rays do scatter inside media)
    assert (work[:, 1] > 2).mean() > 0.1                          # (and the walks do step through cells)


def _brute_at(rays, pixels, nodes, centres, radii, dens, seed):
    n = len(rays)
    t_all = AR.sphere_hit_t(rays[:, :3], rays[:, 3:], centres, radii)
    k0, k1 = seed & M.M32, (seed >> 32) & M.M32
    for j in np.nonzero(dens > 0.0)[0]:
        c, r, den = tuple(float(v) for v in centres[j]), float(radii[j]), float(dens[j])
        for i in range(n):
            w = M.philox4x32_10(int(pixels[i]), 0, int(nodes[i]), MM.MEDIUM_SLOT | int(j), k0, k1)
            t = MM.medium_candidate(tuple(float(v) for v in rays[i, :3]), tuple(float(v) for v in rays[i, 3:]), c, r, den, M.u01_53(w[0], w[1]))
            t_all[i, j] = t if (t is not None and t > MM.T_MIN) else np.inf
    best = np.argmin(t_all, axis=1).astype(np.int32)
    t = t_all[np.arange(n), best].copy()
    miss = ~np.isfinite(t)
    best[miss] = -1
    t[miss] = AR.F64_MAX
    return best, t


def test_tables_refuse_a_bad_medium(abi, medium_walk):
    """through the C structs (what rt_hip_scene_create* sees): a medium whose radius or density is not finite and > 0 is refused"""
    rng = np.random.default_rng(5)
    for field, v in (("radius", 0.0), ("radius", -1.0), ("radius", float("inf")), ("radius", float("nan")),
                     ("fuzz_or_ior", 0.0), ("fuzz_or_ior", -2.0), ("fuzz_or_ior", float("nan")), ("fuzz_or_ior", float("inf"))):
        sc, spheres = AR.random_scene(abi, rng, 40, 3.0, 0.1, 0.4)
        spheres[5].radius = 0.5
        spheres[5].kind = abi.RT_MAT_MEDIUM
        spheres[5].fuzz_or_ior = 1.0
        rc, info, _, _ = medium_walk.medium_tables(sc)
        assert rc == 0 and info[0] == 1
        setattr(spheres[5], field, v)
        assert medium_walk.medium_tables(sc)[0] == 1, (field, v)
    sc, spheres = AR.random_scene(abi, rng, 40, 3.0, 0.1, 0.4)
    spheres[5].kind = 6
    assert medium_walk.medium_tables(sc)[0] == 1


def test_every_cell_inside_a_gridded_medium_lists_it(abi, medium_walk, monkeypatch):
    """interior cells stay listed: for big media that stay in the grid, the cell of EVERY sampled point of the ball — its heart
    included, cells wholly inside the ball — lists the sphere (rt_tables.h drops only cells farther from the centre than the radius)"""
    L = medium_walk
    monkeypatch.setenv("RT_GRID_N", "24,24,24")      # (cells of ~0.55: a ball of radius 1.2 has cells wholly inside it)
    rng = np.random.default_rng(77)
    sc, spheres, n = AR.adversarial_world(abi, rng, 0)
    media = [3, 50, 121]
    for i in media:
        spheres[i].radius = 1.2
        spheres[i].kind = abi.RT_MAT_MEDIUM
        spheres[i].fuzz_or_ior = 0.2
    rc, info, listed, is_large = L.medium_tables(sc)
    assert rc == 0 and info[1] > 0
    cell = 2.0 * (5.0 + 1.2) / info[1:4].astype(np.float64)
    assert (info[1:4] == 24).all() and (cell * math.sqrt(3.0) < 1.2).all(), cell   # (a cell's diagonal is shorter than the radius)
    checked = 0
    for i in media:
        assert not is_large[i], "the medium must be gridded for this test"
        c = np.array(spheres[i].center[:])
        for _ in range(400):
            v = rng.standard_normal(3); v /= np.linalg.norm(v)
            p = np.ascontiguousarray(c + v * 1.2 * rng.uniform(0.0, 0.999) ** (1.0 / 3.0))
            got = L.medium_cell_lists(sc, p, i)
            assert got in (1, -1), (i, p, got)      # (-1: the point lies outside the grid's box)
            checked += got == 1
    assert checked > 1000


SIM_CASES = [("unlit", False, 8), ("unlit", False, 50), ("unlit", True, 8), ("lit", False, 8), ("lit", True, 50)]


@pytest.mark.parametrize("world,moving,depth", SIM_CASES)
def test_cpu_build_of_the_lane_code_equals_the_restatement(abi, oracle, host, medium_walk, world, moving, depth):
    """rt_core.h's MEDIUM lane code built for the host (hit_world_grid<true>, lane_shade<true> / scatter<true>; tests/lanesim/) against
    MediumMini on the scenes of the GPU parity test: tests/parity.py's bar and the exact segment identity, without a GPU"""
    import test_medium_gpu as G
    from parity import assert_parity, pooled_atol
    objs = G._unlit_objs(moving) if world == "unlit" else G._lit_objs(moving)
    spp = 2 if world == "unlit" else 4
    sc, c1, _ = G._load(host, G._cfg(objs, sky=world == "unlit"), 18, 12, spp, depth, seed=21 + depth)
    rc, rgb, lin, segs = medium_walk.render(sc.ptr, c1)
    assert rc == 0 and rgb.shape == (12, 18, 3)
    OL = oracle.lib(abi)
    m = MM.MediumMini(sc.c, lambda y, x: OL.rt_oracle_atan2(y, x), c1)
    m_rgb, m_lin, m_segs = m.render()
    assert_parity(rgb, lin, m_rgb, m_lin, f"{world} moving={moving}", atol=pooled_atol(spp))
    assert segs == m_segs - m.discarded, (segs, m_segs, m.discarded)
    if world == "lit":
        assert m.discarded > 0


def test_the_fog_example_is_generated_and_has_its_two_media(host, abi):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_fog_scene", os.path.join(ROOT, "scenes", "make_fog_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.make() == open(FOG_SCENE).read()
    sc = host.Scene.load(FOG_SCENE)
    media = [sc.c.spheres[i] for i in range(sc.c.n_spheres) if sc.c.spheres[i].kind == abi.RT_MAT_MEDIUM]
    assert sorted(m.radius for m in media) == [1.0, 60.0]
    cam = json.load(open(FOG_SCENE))["camera"]["look_from"]
    assert cam["x"] ** 2 + cam["y"] ** 2 + cam["z"] ** 2 < 60.0 ** 2      # (the camera sits inside the haze)
