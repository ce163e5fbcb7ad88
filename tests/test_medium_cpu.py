"""Participating media without a GPU: the schema, rt_neg_log built for the host against the restatement and against
correctly rounded values (tests/golden/neg_log_cr.npz), and rt_tables.h + hit_world_grid with media (tests/lanesim, a g++ build) against a
brute force of the contract restated in tests/medium_mini.py — on the adversarial walk worlds and on the ray classes of
tests/medium_rays.py, whose conditions are stated here and which tests/test_medium_rays_gpu.py puts through the device."""
import json
import math
import os

import numpy as np
import pytest

import adversarial_rays as AR
import lane_sim
import medium_mini as MM
import medium_rays as MR
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


NEG_LOG_FIXTURE = os.path.join(ROOT, "tests", "golden", "neg_log_cr.npz")


def neg_log_arguments():
    """the 10^6 arguments of the bit test (and of the device's): 1 - k 2^-53 with random k over every magnitude, the smallest and the largest
    k, and the extremes"""
    rng = np.random.default_rng(1503)
    k = np.concatenate([rng.integers(1, 1 << 53, 600_000, dtype=np.uint64),
                        (rng.integers(1, 1 << 53, 300_000, dtype=np.uint64) >> rng.integers(0, 52, 300_000).astype(np.uint64)) | np.uint64(1),
                        np.arange(1, 50_001, dtype=np.uint64), np.uint64((1 << 53) - 1) - np.arange(0, 50_000, dtype=np.uint64)])
    x = 1.0 - k.astype(np.float64) * 2.0 ** -53      # (exact: k < 2^53, and 1 - k 2^-53 is a multiple of 2^-53 below 1)
    return np.concatenate([x, [2.0 ** -53, 1.0 - 2.0 ** -53, 1.0, 0.5, 2.0 ** -0.5, np.nextafter(2.0 ** -0.5, 0.0)]])


def neg_log_fixture():
    """-> the fixture's arguments, the correctly rounded -ln x, (true value - rounded) / ulp(rounded), [(category, count)]"""
    z = np.load(NEG_LOG_FIXTURE)
    return z["x_bits"].view(np.float64), z["neg_log"], z["residual_ulp"].astype(np.float64), [(c.split(":")[0], int(c.split(":")[1])) for c in z["categories"].tolist()]


def neg_log_error_ulp(out, cr, residual):
    """the error of `out` against the TRUE -ln x, in ulps of the correctly rounded value: out - cr is exact for neighbouring doubles, and the
    true value is cr + residual ulps"""
    return np.abs((out - cr) / np.spacing(np.abs(cr)) - residual)


def test_neg_log_bits_accuracy_and_zero(medium_walk):
    """the host build of rt_neg_log is the Python restatement bit for bit on 10^6 arguments 1 - k 2^-53 (random k over every
    magnitude, the smallest and the largest k) and the extremes, and on the arguments of tests/golden/neg_log_cr.npz; against that
    fixture's correctly rounded values (mpmath at 200 bits) its error stays below 1 ulp, the header's own claim; the special values are
    exact"""
    x = neg_log_arguments()
    assert len(x) >= 1_000_000 and (x > 0.0).all()
    out = medium_walk.medium_neg_log_v(x)
    for xi, oi in zip(x.tolist(), out.tolist()):
        r = MM.neg_log(xi)
        assert r == oi and math.copysign(1.0, r) == math.copysign(1.0, oi), (xi, r, oi)
    fx, cr, residual, cats = neg_log_fixture()
    assert 25_000 <= len(fx) <= 60_000 and os.path.getsize(NEG_LOG_FIXTURE) < 512 * 1024 and (np.abs(residual) <= 0.5).all()
    assert dict(cats)["smallest"] == 5000 and dict(cats)["largest"] == 5000 and dict(cats)["sqrt2"] == 5 * 53 and dict(cats)["subnormal"] == 10
    fo = medium_walk.medium_neg_log_v(fx)
    for xi, oi in zip(fx.tolist(), fo.tolist()):
        r = MM.neg_log(xi)
        assert r == oi and math.copysign(1.0, r) == math.copysign(1.0, oi), (xi, r, oi)
    err = neg_log_error_ulp(fo, cr, residual)
    at = int(np.argmax(err))
    print(f"rt_neg_log: worst error against the true value {err[at]:.3f} ulp at {float(fx[at]).hex()} over {len(fx)} arguments; "
          f"{100.0 * (fo == cr).mean():.1f} % correctly rounded")
    k = 0
    for name, count in cats:
        print(f"  {name}: worst {err[k:k + count].max():.3f} ulp, {100.0 * (fo[k:k + count] == cr[k:k + count]).mean():.1f} % correctly rounded")
        k += count
    assert err.max() < 1.0, (err[at], float(fx[at]).hex())
    with np.errstate(all="ignore"):
        sp = medium_walk.medium_neg_log_v(np.array([0.0, -0.0, -1.0, -5e-324, -np.inf, np.nan, np.inf, 1.0]))
    assert sp[0] == np.inf and sp[1] == np.inf and np.isnan(sp[2:6]).all() and sp[6] == -np.inf
    assert sp[7] == 0.0 and math.copysign(1.0, sp[7]) == 1.0 and math.copysign(1.0, MM.neg_log(1.0)) == 1.0
    assert MM.neg_log(0.0) == math.inf and math.isnan(MM.neg_log(-1.0)) and math.isnan(MM.neg_log(math.nan)) and MM.neg_log(math.inf) == -math.inf


def test_neg_log_fixture_is_what_its_generator_writes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_neg_log_fixture", os.path.join(ROOT, "tests", "golden", "make_neg_log_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.fixture_bytes()[0] == open(NEG_LOG_FIXTURE, "rb").read()


WALK_WORLDS = MR.WALK_WORLDS          # (the worlds, their ray tables and the two ray helpers live in tests/medium_rays.py: the device test walks them too)


@pytest.mark.parametrize("name", sorted(WALK_WORLDS))
def test_grid_walk_with_media_equals_brute_force(abi, medium_walk, monkeypatch, name):
    """hit_world_grid with a MediumCtx (CPU build) against the brute force of the contract, bit for bit on (t, index): the ray families
    of tests/adversarial_rays.py, rays that start deep inside a medium, and rays whose candidate lies cells past the first listing"""
    wd = MR.WalkWorld(abi, name)
    for k, v in wd.env.items():
        monkeypatch.setenv(k, v)
    sc, n, media, moving, c0, radii, dens = wd.sc, wd.n, wd.media, wd.moving, wd.c0, wd.radii, wd.dens
    rc, info, listed, is_large = medium_walk.medium_tables(sc, wd.c1c)
    assert rc == 0
    assert info[0] == len(media) and info[1] > 0, "the world must be gridded and know its media"
    assert bool(info[6]) == ("RT_GRID_WIDE" in wd.env)
    # interior cells are kept: a big static medium in the grid is listed in about as many cells as its ball overlaps
    if not moving:
        cell = (c0[:n].max(0) - c0[:n].min(0) + 2 * np.abs(radii[:n]).max()) / info[1:4]
        for i in media[:3]:
            if not is_large[i]:
                ball_cells = 4.0 / 3.0 * math.pi * radii[i] ** 3 / float(np.prod(cell))
                assert listed[i] >= 0.5 * ball_cells, (i, listed[i], ball_cells)
    rays, nodes = wd.rays, wd.nodes
    rc, best, t, work = medium_walk.hit_world_v(sc, rays, wd.c1c, tau=wd.tau, node=nodes)
    assert rc == 0
    k = 0
    n_medium_hits = 0
    for tau, ct, rr in wd.blocks:
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


# ------------------------------------------------------------------ the classes of tests/medium_rays.py (the device test's tables)
def _class_stats(cls, abi, L):
    ref = MR.class_reference(cls, abi, L)
    T = ref.terms
    return ref, T, T[:, 7], ref.best >= 0


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", MR.CLASSES)
def test_class_tables_straddle_their_decisions(abi, medium_walk, cls):
    """the conditions tests/medium_rays.py's classes are drawn for, on the host build: hit_world_v's answer and medium_terms_v's figures for
    the sphere each ray is aimed at (stage 0: no discriminant, 1: not t_in < t2, 2: dist > inside, 3: a candidate)"""
    worlds = MR.class_worlds(cls, medium_walk)
    assert len(worlds) == MR.N_W and all(w.rays.shape == (MR.N_R, 6) and set(w.nodes.tolist()) <= set(MR.NODES.tolist()) for w in worlds)
    assert len({w.seed for w in worlds}) == MR.N_W and any(w.seed >> 32 for w in worlds)
    assert set(np.concatenate([w.nodes for w in worlds]).tolist()) == set(MR.NODES.tolist())
    assert all(1 <= int(w.is_medium().sum()) <= 2 for w in worlds) or cls == "boundary_density"
    ref, T, stage, hit = _class_stats(cls, abi, medium_walk)
    n = len(stage)
    assert n == MR.N_W * MR.N_R
    took = ref.took.mean()
    print(f"{cls}: {100 * took:.1f} % of the rays take a medium, {100 * hit.mean():.1f} % hit; stages {[round(float((stage == k).mean()), 3) for k in range(4)]}")
    finite = np.concatenate([np.isfinite(w.rays).all(axis=1) for w in worlds])
    assert finite.all() == (cls != "non_finite")
    if cls in MR.FRAME_CLASSES:
        assert all(np.abs(w.rays).max() < 1e3 for w in worlds), "a frame may be given these rays"
    if cls == "generic":
        assert 0.05 < took < 0.95
        inside = np.concatenate([np.linalg.norm(w.rays[:, :3] - w.spheres4()[:, :3], axis=1) < w.spheres4()[:, 3] for w in worlds])
        assert 0.3 < inside.mean() < 0.7, "origins outside and inside"
    if cls == "tangent":
        assert (T[:, 0] >= 0.0).mean() >= 0.20 and (T[:, 0] < 0.0).mean() >= 0.20, ((T[:, 0] >= 0.0).mean(), (T[:, 0] < 0.0).mean())
        assert (T[:, 0] == 0.0).sum() >= 5000 and ((np.abs(T[:, 0]) < 2.0 ** -1022) & (T[:, 0] != 0.0)).sum() >= 5000, "discriminants that are 0, and denormal ones"
        assert took >= 0.1, "and where there is a chord, the dense medium takes the ray"
    if cls == "surface_origin":
        has = stage >= 1
        above = has & (T[:, 1] > MR.T_MIN)
        assert has.all() and above.mean() >= 0.20 and (has & ~above).mean() >= 0.20 and (stage == 1).mean() >= 0.10, (above.mean(), (stage == 1).mean())
        ulps1, ulps2 = np.abs(T[:, 1] - MR.T_MIN) / np.spacing(MR.T_MIN), np.abs(T[:, 2] - MR.T_MIN) / np.spacing(MR.T_MIN)
        assert (ulps1 <= 4.0).mean() >= 0.15 and (ulps2 <= 4.0).mean() >= 0.10 and (T[:, 1] == MR.T_MIN).any() and (T[:, 2] == MR.T_MIN).any()
        fam = np.concatenate([w.notes["fam"] for w in worlds])
        assert ((T[:, 2] - np.maximum(T[:, 1], 0.0)) < MR.T_MIN)[fam == 2].mean() > 0.9, "the short chords are shorter than T_MIN"
    if cls == "boundary_density":
        aimed = np.concatenate([w.notes["aimed"] for w in worlds])
        assert aimed.mean() > 0.99 and (stage == 3).mean() >= 0.30 and (stage == 2).mean() >= 0.30, ((stage == 3).mean(), (stage == 2).mean())
        off = (T[:, 5] - T[:, 3]) / np.spacing(T[:, 3])
        assert (np.abs(off[aimed]) <= 8.0).all() and (off[aimed] == 0.0).mean() >= 0.1, "dist lies within a few ulps of the chord, and on it"
        assert all(len(w.objs) == MR.N_R for w in worlds)
    if cls == "magnitudes":
        assert (T[:, 6] == 0.0).mean() >= 0.10 and took >= 0.05, ((T[:, 6] == 0.0).mean(), took)
        assert (ref.took & (T[:, 6] == 0.0)).sum() >= 1000, "rays on ray_consts' slow path do take media"
    if cls == "occluder_inside":
        assert hit.mean() > 0.9 and 0.30 <= ref.took[hit].mean() <= 0.70, ref.took[hit].mean()
    if cls == "nested":
        inner = np.concatenate([np.full(MR.N_R, w.notes["inner"]) for w in worlds])
        assert (ref.best == inner).mean() >= 0.15 and (hit & (ref.best != inner)).mean() >= 0.15 and (~hit).mean() >= 0.02
        assert all((ref.best[w * MR.N_R:(w + 1) * MR.N_R] == k).any() for w in range(MR.N_W) for k in (0, 1)), "in either table order"
    if cls in ("tangent", "surface_origin"):       # one medium and nothing else: hit_world takes it exactly where medium_terms_v has a candidate
        assert np.array_equal(ref.took, (stage == 3) & (T[:, 5] > 0.0))


SUBSET_PER_WORLD = 20            # rays 0, 50, 100 ... of every world: 2 000 inputs of a class, all of its worlds among them


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", MR.CLASSES)
def test_new_classes_host_build_equals_the_restatement(abi, medium_walk, cls):
    """hit_world_v (the host build of hit_world_grid<true>) against the brute force over tests/medium_mini.py's medium_candidate on 20 rays of
    each of the class's 100 worlds: (index, bits of t).  Every world carries its class's edge, so every world is in the subset."""
    ref = MR.class_reference(cls, abi, medium_walk)
    rows = np.arange(0, MR.N_R, MR.N_R // SUBSET_PER_WORLD)
    checked = took = 0
    for w, wd in enumerate(MR.class_worlds(cls, medium_walk)):
        centres = np.array([o[0] for o in wd.objs], np.float64)
        radii = np.array([o[1] for o in wd.objs], np.float64)
        dens = np.array([o[3] if o[2] == "medium" else 0.0 for o in wd.objs], np.float64)
        bb, tb = _brute_at(wd.rays[rows], rows, wd.nodes[rows], centres, radii, dens, wd.seed, sparse=True)
        g_b, g_t = ref.best[w * MR.N_R + rows], ref.t[w * MR.N_R + rows]
        bad = np.nonzero((g_b != bb) | (g_t.view(np.uint64) != tb.view(np.uint64)))[0]
        assert len(bad) == 0, (cls, w, rows[bad[:5]], g_b[bad[:5]], bb[bad[:5]], g_t[bad[:5]], tb[bad[:5]])
        checked += len(rows)
        took += int((dens[np.maximum(bb, 0)] > 0.0)[bb >= 0].sum())
    assert checked >= 2000
    if cls != "non_finite":
        assert took >= 0.05 * checked, took


def _disc_ok(o, d, centres, radii):
    """where Sphere::hit's discriminant is >= 0 (n x m), with sphere_hit_t's operations: where a medium can have a candidate at all"""
    dx, dy, dz = (d[:, k:k + 1] for k in range(3))
    a = (dx * dx + dy * dy) + dz * dz
    ocx, ocy, ocz = (o[:, k:k + 1] - centres[None, :, k] for k in range(3))
    half_b = (ocx * dx + ocy * dy) + ocz * dz
    c = ((ocx * ocx + ocy * ocy) + ocz * ocz) - radii[None, :] * radii[None, :]
    return (half_b * half_b) - (a * c) >= 0.0


def _brute_at(rays, pixels, nodes, centres, radii, dens, seed, sparse=False):
    """sparse: the restatement runs only where numpy finds a discriminant >= 0 (it returns None elsewhere: a world of 1 000 media)"""
    n = len(rays)
    with np.errstate(all="ignore"):
        t_all = AR.sphere_hit_t(rays[:, :3], rays[:, 3:], centres, radii)
        may = _disc_ok(rays[:, :3], rays[:, 3:], centres, radii) if sparse else np.ones((n, len(radii)), bool)
    k0, k1 = seed & M.M32, (seed >> 32) & M.M32
    for j in np.nonzero(dens > 0.0)[0]:
        c, r, den = tuple(float(v) for v in centres[j]), float(radii[j]), float(dens[j])
        t_all[:, j] = np.inf
        for i in np.nonzero(may[:, j])[0]:
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
