"""The device quad code on adversarial rays, bit for bit.

The contract of quads and boxes is "the bits of csrc/common/rt_quad.h".  tests/test_quad_cpu.py pins them for the host build of that
header against the restatement of tests/quad_mini.py; the device compiles the header with another compiler and wraps it in another form
— rt_core.h quads_hit, a cold call with the table pointer and the count made wave-uniform and the 128-byte records read through the
constant address space.  Here the ray tables of tests/quad_rays.py (the CPU test's own) go through the device:
  - rt_hip_quad_probe (librt_hip_probe.so): quads_hit and object_surface<true>, one ray per thread with its own closest-so-far, against
    one quad (the nine classes), against an ordered range with the closest carried from quad to quad, and against RT_MAX_QUADS quads.
    Every accept decision, t, P, hit normal and front_face must equal tests/lane_sim.py's quad_hit_v — the g++ build of the same header
    — bit for bit.  With the CPU test this reads: device = host build = restatement;
  - rt_hip_render_rays_probe: the real QUADS megakernels render 64 x 48 frames whose camera rays are the tables' finite rays.  Sample
    0's camera segment records the (closest, best) hit_world returned — behind the lock-step walk, the `large` list and step (4), the
    quads: it must equal lane_sim's hit_world_v, the host build of the same hit_world, in id and in the bits of t.  The tie rules
    (a sphere beats a quad and an earlier quad a later one at an equal t; one ulp nearer wins) are checked on the device this way.
There is no tolerance anywhere.  The conditions on the inputs — 5 % .. 95 % of a class's rays hit, spheres and quads each win 10 % of a
frame's hit rays, every quad of a class but `magnitudes` is accepted as drawn — are checked on the host build by the tests without the
gpu mark, whose results the device tests reuse.  non_finite and magnitudes rays go through the quad probe only, never through a frame."""
import ctypes as C
import functools

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import lane_sim
from quad_rays import AXIS_CLASSES, CLASSES, N_R, STRADDLING, T_MAX, _aimed, _quads, class_tables, device_class_tables

W, H, SPP, DEPTH = 64, 48, 2, 5                  # a frame of 3 072 camera rays, as tests/test_walk_rays_gpu.py
QUADS, SOLID, MEDIUM, MOTION, HL = 512, 256, 128, 64, 4
FRAME_CLASSES = ("generic", "edges", "skewed", "needle")        # finite rays of ordinary magnitude: what a frame may be given
CHUNK = N_R                                       # rays per probe launch: 1 000 = 15 waves + 40 lanes, the last wave partial


@pytest.fixture(scope="module")
def sim(abi):
    return lane_sim.load(abi)


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _sim():
    """the lane simulator outside a fixture (the cached references below)"""
    from conftest import graft
    return lane_sim.load(graft.load_package().abi)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared tables are read-only)


# ------------------------------------------------------------------ worlds through the C structs
def _quad(abi, quv, kind=0, **kw):
    r = abi.RtQuad()
    r.q[:] = [float(x) for x in quv[0:3]]; r.u[:] = [float(x) for x in quv[3:6]]; r.v[:] = [float(x) for x in quv[6:9]]
    r.albedo[:] = [0.7, 0.6, 0.5]
    r.kind, r.fuzz_or_ior = kind, (0.25 if kind == abi.RT_MAT_METAL else 1.5)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _quad_array(abi, quads):
    return (abi.RtQuad * len(quads))(*quads)


def _scene(abi, spheres, width=W, height=H, seed=4242):
    """an RtScene over `spheres` = [(centre, radius, kind)], gradient sky; (scene, the array that keeps its spheres alive)"""
    arr = (abi.RtSphere * len(spheres))()
    for s, (c, r, kind) in zip(arr, spheres):
        s.center[:] = [float(x) for x in c]
        s.radius = float(r)
        s.albedo[:] = [0.6, 0.5, 0.7]
        s.kind = kind
        s.fuzz_or_ior = 1.5 if kind != abi.RT_MAT_METAL else 0.25
    sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=width, height=height, samples_per_pixel=SPP, max_depth=DEPTH, sky_mode=abi.RT_SKY_GRADIENT,
                     spheres=arr, n_spheres=len(spheres), seed=seed)
    sc.cam_origin[:] = [0.0, 0.0, 30.0]               # (a frame's own camera rays are replaced by the probe's; the camera is an ordinary one)
    sc.cam_lower_left[:] = [-1.5, -1.0, 29.0]
    sc.cam_horizontal[:] = [3.0, 0.0, 0.0]
    sc.cam_vertical[:] = [0.0, 2.0, 0.0]
    return sc, arr


@functools.lru_cache(maxsize=None)
def _class_table(cls):
    """device_class_tables(cls) drawn once per session, read-only: [(quv, rays, closest)]"""
    out = []
    for quv, rays, closest in device_class_tables(cls):
        for a in (quv, rays, closest):
            a.setflags(write=False)
        out.append((quv, rays, closest))
    return out


# ------------------------------------------------------------------ (a) the nine classes, one quad per launch
@functools.lru_cache(maxsize=None)
def _class_reference(cls):
    """the host build (quad_hit_v) on the class's table: hit, t, P, normal, front over all its rays, the quad index of every ray"""
    L = _sim()
    parts, which = [], []
    with np.errstate(all="ignore"):
        for k, (quv, rays, closest) in enumerate(_class_table(cls)):
            st, *res = L.quad_hit_v(quv, rays, closest)
            assert st == 0, (cls, k)
            parts.append(res)
            which.append(np.full(len(rays), k, np.int32))
    hit, t, P, nrm, front = (np.concatenate([p[i] for p in parts]) for i in range(5))
    return hit, t, P, nrm, front, np.concatenate(which)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")     # (the classes make NaN, inf and overflow on purpose)
@pytest.mark.parametrize("cls", CLASSES)
def test_device_tables_on_the_host_build(sim, cls):
    """the inputs of the device test, checked without a GPU: >= 10^5 rays; every class but `magnitudes` has its first 100 quads accepted, so
    its table is the CPU test's byte for byte (device_class_tables asserts the acceptance; the bytes are compared here); the six classes
    about a decision straddle it on the host build, which the CPU test equated with the restatement on these very tables"""
    table = _class_table(cls)
    assert len(table) == (1 if cls in AXIS_CLASSES else 100)
    if cls != "magnitudes":
        cpu = list(class_tables(cls))
        assert len(cpu) == len(table)
        for a, b in zip(cpu, table):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), cls
    else:
        first = [q for q, _, _ in class_tables(cls)]
        st = sim.quad_prepare_v(np.array(first))[1]
        kept = [q for q, s in zip(first, st) if s == 0]
        assert 0 < len(kept) < 100, "some of the CPU test's magnitudes quads are refused: the reason this table draws on"
        assert all(a.tobytes() == b[0].tobytes() for a, b in zip(kept, table)), "the accepted ones lead the device table, in order"
    hit = _class_reference(cls)[0]
    total, hits = len(hit), int(hit.sum())
    assert total >= 100_000
    print(f"{cls}: {hits} of {total} rays hit (host build)")
    if cls in STRADDLING:
        assert 0.05 * total < hits < 0.95 * total, "the class straddles the decision it is about"


class _ProbeOut:
    """the five outputs of rt_hip_quad_probe for n rays in ONE device buffer (one copy back): t [n], P [3n], normal [3n] as f64 then best
    [n], front [n] as i32; filled with a pattern no result has, so that a miss can be seen to have written nothing but its -1"""
    FILL64, FILL32 = 0x7FF8DEADBEEF0000, -2

    def __init__(self, n):
        self.n = n
        host = np.full(8 * n, self.FILL64, np.uint64)
        host[7 * n:].view(np.int32)[:] = self.FILL32
        self.d = _dev(host.view(np.int64))
        self.base = self.d.data_ptr()

    def ptrs(self, off):
        """(d_best, d_t, d_point, d_normal, d_front) of the rays from `off` on"""
        n, b = self.n, self.base
        return b + 56 * n + 4 * off, b + 8 * off, b + 8 * n + 24 * off, b + 32 * n + 24 * off, b + 60 * n + 4 * off

    def fetch(self):
        n = self.n
        host = self.d.cpu().numpy().view(np.uint64)
        ints = host[7 * n:].view(np.int32)
        return ints[:n], host[:n], host[n:4 * n].reshape(n, 3), host[4 * n:7 * n].reshape(n, 3), ints[n:]


def _assert_probe_equals(what, got, want_best, t, P, nrm, front):
    """got = _ProbeOut.fetch(); want_best = the id or -1 per ray; t, P, nrm, front = the host build's record where want_best >= 0"""
    g_best, g_t, g_P, g_n, g_front = got
    bad = np.flatnonzero(g_best != want_best)
    assert bad.size == 0, f"{what}: the accept decision / id differs on {bad.size} rays; first {bad[:5].tolist()}: device {g_best[bad[:5]].tolist()} host {want_best[bad[:5]].tolist()}"
    hit = want_best >= 0
    for name, g, w in (("t", g_t, _bits(t)), ("P", g_P, _bits(P)), ("the normal", g_n, _bits(nrm))):
        bad = np.flatnonzero((g[hit] != w[hit]).reshape(int(hit.sum()), g[0].size).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs in its bits on {bad.size} of {int(hit.sum())} hits; first (among the hits) {bad[:5].tolist()}"
    assert np.array_equal(g_front[hit], front[hit].astype(np.int32)), f"{what}: front_face differs"
    miss = ~hit
    assert (g_t[miss] == _ProbeOut.FILL64).all() and (g_P[miss] == _ProbeOut.FILL64).all() and (g_n[miss] == _ProbeOut.FILL64).all() \
        and (g_front[miss] == _ProbeOut.FILL32).all(), f"{what}: a miss wrote a record"


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", CLASSES)
def test_device_quad_code_equals_the_host_build(pkg, abi, sim, torch_cuda, cls):
    """one scene per class — a small sphere and the class's quads (100, or the axis-aligned one) — and each quad's 1 000 rays with their
    closest-so-far through rt_hip_quad_probe(first_quad = k, n_quads = 1): 100 launches of 1 000 rays (the last wave of each is partial),
    one copy back; against quad_hit_v of the host build: accept decision, t, P, hit normal, front_face, bit for bit"""
    table = _class_table(cls)
    hit, t, P, nrm, front, which = _class_reference(cls)
    n = len(hit)
    sc, keep = _scene(abi, [((0.0, 0.0, -60.0), 0.5, abi.RT_MAT_LAMBERTIAN)], 8, 8)
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=_quad_array(abi, [_quad(abi, q) for q, _, _ in table]))
    try:
        assert gs.query("quads") == len(table)
        d_rays = _dev(np.concatenate([r for _, r, _ in table]))
        d_closest = _dev(np.concatenate([c for _, _, c in table]))
        out = _ProbeOut(n)
        stream = torch.cuda.current_stream().cuda_stream
        for off in range(0, n, CHUNK):
            m = min(CHUNK, n - off)
            assert (which[off:off + m] == which[off]).all()
            gs.quad_probe(d_rays.data_ptr() + 48 * off, d_closest.data_ptr() + 8 * off, m, int(which[off]), 1, *out.ptrs(off), stream=stream)
        torch.cuda.synchronize()
        got = out.fetch()
    finally:
        gs.close()
    hits = int((got[0] >= 0).sum())
    print(f"{cls}: {hits} of {n} rays hit (device)")
    want_best = np.where(hit == 1, 1 + which, -1).astype(np.int32)
    _assert_probe_equals(cls, got, want_best, t, P, nrm, front)
    assert hits == int(hit.sum())
    if cls in STRADDLING:
        assert 0.05 * n < hits < 0.95 * n, "the class straddles the decision it is about"


# ------------------------------------------------------------------ (b), (c) the ordered scan, closest carried
def _host_scan(L, quvs, first, rays, closest, id_base):
    """quads_hit restated over the host build's single-quad test: quvs in order, every accepted t fed forward as the next closest ->
    best (id_base + first + k, or -1), t, P, normal, front of the last accepted quad"""
    n = len(rays)
    best, cl = np.full(n, -1, np.int32), np.array(closest, np.float64)
    t, P, nrm, front = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int32)
    for k, quv in enumerate(quvs):
        st, h, tk, Pk, nk, fk = L.quad_hit_v(quv, rays, cl)
        assert st == 0
        h = h == 1
        best[h], cl[h], t[h], P[h], nrm[h], front[h] = id_base + first + k, tk[h], tk[h], Pk[h], nk[h], fk[h]
    return best, t, P, nrm, front


def _probe_scan(gs, rays, closest, first, count):
    out = _ProbeOut(len(rays))
    d_rays, d_closest = _dev(rays), _dev(closest)
    gs.quad_probe(d_rays.data_ptr(), d_closest.data_ptr(), len(rays), first, count, *out.ptrs(0), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.fetch()


DUP_OF = [5 * m for m in range(10)]      # the scan scene: the generic class's 100 quads, then quad 100 + m = quad DUP_OF[m] again


@functools.lru_cache(maxsize=None)
def _scan_inputs():
    """(quvs of the scan scene, the mixed rays and their closest, the 200 rays through the duplicated quads)"""
    table = _class_table("generic")
    quvs = [q for q, _, _ in table] + [table[i][0] for i in DUP_OF]
    rays = np.concatenate([r[:41] for _, r, _ in table])           # 41 rays of every quad: 4 100 = 64 waves + 4 lanes
    closest = np.concatenate([c[:41] for _, _, c in table])
    rng = np.random.default_rng(2300)
    dup = np.concatenate([_aimed(rng, quvs[i], 20, rng.uniform(0.05, 0.95, (20, 2))) for i in DUP_OF])
    for a in (rays, closest, dup):
        a.setflags(write=False)
    return quvs, rays, closest, dup


@pytest.mark.gpu
def test_ordered_scan_carries_the_closest(pkg, abi, sim, torch_cuda):
    """quads_hit over a range: the whole list and a middle range (37, 21) of the generic class's quads, 4 100 of its rays with their
    closest-so-far: id and record equal a host loop over quad_hit_v in quad order that feeds each accepted t forward.  200 rays aimed
    into quads that are in the list twice (quad j = quad i, i < j): the later copy never wins, and where the nearest hit is on the
    duplicated quad, the id is i."""
    quvs, rays, closest, dup = _scan_inputs()
    sc, keep = _scene(abi, [((0.0, 0.0, -60.0), 0.5, abi.RT_MAT_LAMBERTIAN)], 8, 8)
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=_quad_array(abi, [_quad(abi, q) for q in quvs]))
    try:
        for first, count in ((0, 100), (37, 21)):
            got = _probe_scan(gs, rays, closest, first, count)
            want = _host_scan(sim, quvs[first:first + count], first, rays, closest, 1)
            _assert_probe_equals(f"scan ({first}, {count})", got, *want)
            n_hit = int((want[0] >= 0).sum())
            print(f"scan ({first}, {count}): {n_hit} of {len(rays)} rays hit, {len(np.unique(want[0]))} ids")
            assert n_hit > 0.2 * len(rays) and len(np.unique(want[0])) > count // 2
        free = np.full(len(dup), T_MAX)
        got = _probe_scan(gs, dup, free, 0, len(quvs))
        want = _host_scan(sim, quvs, 0, dup, free, 1)
        _assert_probe_equals("duplicated quads", got, *want)
        assert (got[0] >= 0).all() and (got[0] < 1 + 100).all(), "a later copy of a quad never wins"
        own = np.repeat(np.array(DUP_OF, np.int32), 20)
        alone = np.concatenate([sim.quad_hit_v(quvs[i], dup[20 * m:20 * m + 20], free[:20])[2] for m, i in enumerate(DUP_OF)])
        nearest = got[1] == _bits(alone)
        assert nearest.sum() >= 100, int(nearest.sum())
        assert (got[0][nearest] == 1 + own[nearest]).all(), "on the duplicated quad the first copy is kept"
        # a range outside the scene's quads is refused
        for first, count in ((0, len(quvs) + 1), (len(quvs), 1), (len(quvs) + 1, 0), (7, 0xFFFFFFFF)):
            with pytest.raises(pkg.host.RtError) as e:
                _probe_scan(gs, dup[:8], free[:8], first, count)
            assert e.value.code == abi.RT_ERR_INVALID
    finally:
        gs.close()


MANY_TARGETS = (0, 511, 512, 1022, 1023)


@functools.lru_cache(maxsize=None)
def _many_inputs():
    """RT_MAX_QUADS generic quads from a fixed seed (every one accepted), 4 096 rays aimed at them from nearby — the first 5 x 64 at quads
    0, 511, 512, 1022 and 1023 — with half of the closest-so-far finite"""
    rng = np.random.default_rng(2400)
    quvs = _quads(rng, 1024, "generic")
    aim = np.concatenate([np.repeat(MANY_TARGETS, 64), rng.integers(0, 1024, 4096 - 64 * len(MANY_TARGETS))])
    rays = np.concatenate([_aimed(rng, quvs[k], 1, rng.uniform(0.05, 0.95, (1, 2)), dist=(0.05, 1.5)) for k in aim])
    closest = np.where(rng.random(4096) < 0.5, T_MAX, rng.uniform(0.0, 8.0, 4096))
    for a in (quvs, rays, closest):
        a.setflags(write=False)
    return quvs, rays, closest


@functools.lru_cache(maxsize=None)
def _many_reference():
    quvs, rays, closest = _many_inputs()
    return _host_scan(_sim(), list(quvs), 0, rays, closest, 1)


def test_the_1024_quads_are_accepted_and_the_ends_of_the_table_win(sim):
    """the inputs of the 1024-quad test on the host build: every quad accepted; each of quads 0, 511, 512, 1022, 1023 wins rays, and so do
    hundreds of others on both sides of record 512"""
    quvs, rays, closest = _many_inputs()
    assert (sim.quad_prepare_v(quvs)[1] == 0).all() and len(np.unique(quvs, axis=0)) == 1024
    best = _many_reference()[0]
    for k in MANY_TARGETS:
        assert (best == 1 + k).sum() >= 8, (k, int((best == 1 + k).sum()))
    ids = np.unique(best[best >= 0]) - 1
    assert (ids < 512).sum() > 200 and (ids >= 512).sum() > 200
    print(f"1024 quads: {int((best >= 0).sum())} of {len(rays)} rays hit, {len(ids)} quads win")


@pytest.mark.gpu
def test_1024_quads(pkg, abi, sim, torch_cuda):
    """RT_MAX_QUADS distinct quads: record offsets up to 128 KB through quads_hit's load path.  The full-range scan of 4 096 aimed rays
    (at least 64 at each of quads 0, 511, 512, 1022, 1023) equals the host loop in id and record.  (The frame of this scene:
    test_megakernel_first_hit_with_quads[many].)"""
    quvs, rays, closest = _many_inputs()
    sc, keep = _scene(abi, [((0.0, 0.0, -60.0), 0.5, abi.RT_MAT_LAMBERTIAN)], 8, 8)
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=_quad_array(abi, [_quad(abi, q) for q in quvs]))
    try:
        assert gs.query("quads") == abi.RT_MAX_QUADS == 1024
        got = _probe_scan(gs, rays, closest, 0, 1024)
    finally:
        gs.close()
    _assert_probe_equals("1024 quads", got, *_many_reference())


# ------------------------------------------------------------------ (d) through the real megakernel
FRAME_CASES = ["unlit", "lit", "moving_medium_checker", "many"]
FRAME_KEY = {"unlit": QUADS, "lit": QUADS | HL, "moving_medium_checker": QUADS | MOTION | MEDIUM | SOLID, "many": QUADS}


class _FrameWorld:
    """one case of the megakernel test: 30 spheres (two of them big: the `large` list) and the quads, the frame's 3 072 camera rays, and
    what the host build of hit_world returns for them"""

    def __init__(self, abi, case):
        from mini_oracle import M32, philox4x32_10
        rng = np.random.default_rng(2500 + FRAME_CASES.index(case))
        kinds = (abi.RT_MAT_LAMBERTIAN, abi.RT_MAT_METAL, abi.RT_MAT_GLASS)
        n_s = 30
        centres = rng.uniform(-8.0, 8.0, (n_s, 3))
        radii = rng.uniform(0.8, 2.2, n_s)
        spheres = [(centres[i], radii[i], kinds[i % 3]) for i in range(n_s)]
        spheres[0] = ((0.0, -15.0, 0.0), 8.0, abi.RT_MAT_LAMBERTIAN)
        spheres[1] = ((14.0, 0.0, 0.0), 7.0, abi.RT_MAT_METAL)
        self.center1 = None
        if case == "lit":
            spheres[3] = (spheres[3][0], spheres[3][1], abi.RT_MAT_LIGHT)
        if case == "moving_medium_checker":
            spheres[4] = (spheres[4][0], spheres[4][1], abi.RT_MAT_MEDIUM)
            c1 = np.array([np.asarray(s[0], np.float64) for s in spheres])
            c1[5] += [0.6, -0.4, 0.5]
            self.center1 = c1.tolist()
        self.sc, self.keep = _scene(abi, spheres, seed=97531 + FRAME_CASES.index(case))
        if case == "moving_medium_checker":
            self.keep[4].fuzz_or_ior = 0.9         # (a Medium's density)
        if case == "many":
            quvs, rays, _ = _many_inputs()
            self.quvs = list(quvs)
            # the rays at the five marked quads; rays from further off; and rays that start inside a sphere, aimed at a quad: in so dense a
            # world a sphere seldom wins otherwise
            near, inside = 64 * len(MANY_TARGETS), 1000
            far = np.concatenate([_aimed(rng, quvs[k], 1, dist=(0.5, 16.0)) for k in rng.integers(0, 1024, W * H - near - inside)])
            i = rng.integers(0, n_s, inside)
            step = rng.standard_normal((inside, 3))
            c_all, r_all = np.array([np.asarray(s[0], np.float64) for s in spheres]), np.array([s[1] for s in spheres])
            o = c_all[i] + step / np.linalg.norm(step, axis=1)[:, None] * (r_all[i] * rng.uniform(0.0, 0.9, inside))[:, None]
            q = quvs[rng.integers(0, 1024, inside)]
            ab = rng.uniform(0.0, 1.0, (inside, 2))
            target = q[:, 0:3] + ab[:, :1] * q[:, 3:6] + ab[:, 1:] * q[:, 6:9]
            self.rays = np.concatenate([rays[:near], far, np.concatenate([o, (target - o) * rng.uniform(0.25, 4.0, (inside, 1))], axis=1)])
        else:
            picked = [(cls, k) for cls in FRAME_CLASSES for k in range(3)]
            self.quvs = [_class_table(cls)[k][0] for cls, k in picked]
            self.rays = np.concatenate([_class_table(cls)[k][1][:W * H // len(picked)] for cls, k in picked])
        assert self.rays.shape == (W * H, 6) and np.isfinite(self.rays).all() and np.abs(self.rays).max() < 1e3
        mats = [dict(kind=kinds[k % 3]) for k in range(len(self.quvs))] if case != "many" else [dict(kind=abi.RT_MAT_LAMBERTIAN)] * len(self.quvs)
        if case == "moving_medium_checker":
            tw, th = abi.checker_odd_pack((0.1, 0.2, 0.3))
            mats[0] = dict(kind=abi.RT_MAT_CHECKER, h_offset=1.5, tex_w=tw, tex_h=th)
        self.quads = _quad_array(abi, [_quad(abi, q, **m) for q, m in zip(self.quvs, mats)])
        self.tau = self.node = None
        if case == "moving_medium_checker":    # sample 0's shutter time of every pixel (tests/test_motion.py tau_of), the camera segment's node 0
            seed = self.sc.seed
            self.tau = np.array([float(philox4x32_10(p, 0, 0xFFFFFFFD, 0, seed & M32, (seed >> 32) & M32)[0] >> 8) * 2.0 ** -24 for p in range(W * H)], np.float32)
            self.node = np.zeros(W * H, np.uint32)
        rc, self.best, self.t, _ = _sim().hit_world_v(self.sc, self.rays, center1=self.center1, quads=self.quads, tau=self.tau, node=self.node)
        assert rc == 0
        self.n_spheres = n_s


@functools.lru_cache(maxsize=None)
def _frame_world(case):
    from conftest import graft
    return _FrameWorld(graft.load_package().abi, case)


@pytest.mark.parametrize("case", FRAME_CASES)
def test_frame_worlds_let_spheres_and_quads_win(abi, case):
    """the inputs of the megakernel test on the host build: of the rays that hit, at least 10 % end on a sphere and at least 10 % on a quad"""
    wd = _frame_world(case)
    hit = wd.best >= 0
    on_quad = wd.best >= wd.n_spheres
    print(f"{case}: {int(hit.sum())} of {W * H} rays hit: {int((hit & ~on_quad).sum())} spheres ({len(np.unique(wd.best[hit & ~on_quad]))} ids), "
          f"{int(on_quad.sum())} quads ({len(np.unique(wd.best[on_quad]))} ids)")
    assert hit.sum() > 0.5 * W * H
    assert (hit & ~on_quad).sum() >= 0.1 * hit.sum() and on_quad.sum() >= 0.1 * hit.sum()
    assert {0, 1} <= set(wd.best[hit].tolist()), "the two big spheres win rays too"
    if case == "many":
        assert all((wd.best == wd.n_spheres + k).any() for k in MANY_TARGETS)


def _probe_frame(gs, rays, w, h):
    """one rt_hip_render_rays_probe frame -> (rgb8, linear, segments), first_t, first_best, last_kernel"""
    d_rays = _dev(rays.reshape(h, w, 6))
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda:0")
    lin = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
    first_t = torch.full((h, w), float("nan"), dtype=torch.float64, device="cuda:0")
    first_b = torch.full((h, w), -2, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = gs.render_rays_probe(d_rays.data_ptr(), rgb.data_ptr(), lin.data_ptr(), first_t.data_ptr(), first_b.data_ptr())
    return (rgb.cpu().numpy(), lin.cpu().numpy(), st["segments"]), first_t.cpu().numpy().reshape(-1), first_b.cpu().numpy().reshape(-1), gs.query("last_kernel")


def _frames_of_both_variants(gs, rays, w, h, what):
    """the probe frame under the grid walk and under the full scan ("variant" 1): rgb8, linear and segments equal bit for bit, and so is
    the first-hit record; returns the grid walk's"""
    a = _probe_frame(gs, rays, w, h)
    gs.set_option("variant", 1)
    b = _probe_frame(gs, rays, w, h)
    gs.set_option("variant", 0)
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1].view(np.uint32), b[0][1].view(np.uint32)) and a[0][2] == b[0][2], f"{what}: variant 1 differs"
    assert np.array_equal(a[2], b[2]) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[3] == b[3], f"{what}: variant 1's first hits differ"
    return a


def _assert_first_hits(what, p_t, p_b, best, t):
    bad = np.flatnonzero((p_b != best) | ((best >= 0) & (_bits(p_t) != _bits(t))))
    assert bad.size == 0, (f"{what}: the megakernel's first hit differs from the host build of hit_world on {bad.size} of {len(best)} rays; first "
                           f"{bad[:5].tolist()}: device {p_b[bad[:5]].tolist()} {p_t[bad[:5]].tolist()} host {best[bad[:5]].tolist()} {t[bad[:5]].tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", FRAME_CASES)
def test_megakernel_first_hit_with_quads(pkg, abi, torch_cuda, case):
    """64 x 48 at spp 2, depth 5 through rt_hip_render_rays_probe: the (closest, best) the QUADS megakernel's hit_world returned for sample
    0's camera segment — the lock-step walk's closest handed to quads_hit — equals lane_sim's hit_world_v in id and in the bits of t (a
    miss: -1).  unlit: 12 quads of the classes generic, edges, skewed and needle with 256 rays of each; lit: + a Light; moving_medium_checker:
    a moving sphere, a Medium sphere and a Checker quad, every ray at its pixel's sample-0 shutter time and RNG address; many: the 1 024
    quads of test_1024_quads.  Each frame equals the full scan's ("variant" 1) bit for bit."""
    wd = _frame_world(case)
    gs = pkg.hip.HipScene(C.pointer(wd.sc), 0, library=pkg.hip.probe_lib(), center1=wd.center1, quads=wd.quads)
    try:
        frame, p_t, p_b, key = _frames_of_both_variants(gs, wd.rays, W, H, case)
    finally:
        gs.close()
    assert key == FRAME_KEY[case], (case, key)
    _assert_first_hits(case, p_t, p_b, wd.best, wd.t)
    hit = wd.best >= 0
    assert (hit & (wd.best < wd.n_spheres)).sum() >= 0.1 * hit.sum() and (wd.best >= wd.n_spheres).sum() >= 0.1 * hit.sum()
    assert np.isfinite(frame[1]).all() and len(np.unique(frame[0].reshape(-1, 3), axis=0)) > 100 and frame[2] >= W * H * SPP


def _tie_world(abi):
    """tests/test_quad_cpu.py::test_ids_and_ties' world and its six rays"""
    spheres = [((5.0, 5.0, 5.0), 0.5, abi.RT_MAT_LAMBERTIAN), ((0.0, 1.0, 0.0), 1.0, abi.RT_MAT_LAMBERTIAN)]
    floor = np.array([-2.0, 0.0, -2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 4.0])
    quvs = [np.array([-2.0, -1.0, -2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 4.0]), floor, floor]
    rays = np.array([[0.0, -3.0, 0.0, 0.0, 1.0, 0.0],      # the tie of sphere 1 and quads 1, 2 (quad 0 lies at t = 2: it wins outright)
                     [0.0, -0.5, 0.0, 0.0, 1.0, 0.0],      # from between the planes: the tie at t = 0.5
                     [1.5, -0.5, 0.0, 0.0, 2.0, 0.0],      # beside the sphere: the coincident quads alone
                     [1.5, 3.0, 0.0, 0.0, -1.0, 0.0],      # from above: the coincident quads before quad 0
                     [5.0, 9.0, 5.0, 0.0, -1.0, 0.0],      # sphere 0, off every quad
                     [9.0, 9.0, 9.0, 0.0, 1.0, 0.0]])      # nothing
    return spheres, quvs, rays


def _ulp_world(abi):
    """Three unit spheres at (x, 1, 0), x = 0, 10, 20, each touching the plane y = 0 from above, and under each a floor quad in the plane
    y = 0, y = +2^-51 and y = -2^-51.  A ray from (x, -3, 0) along (0, s, 0) meets its sphere at t = 3 / s exactly (half_b = -4 s, c = 15,
    a = s^2) and its quad at t = (3 + y) / s (N = (0, -1, 0), D = -y, N.o = 3, den = -s: every step exact for s = 1, 2): one ulp of 3
    (2^-51) farther, where the sphere wins; one ulp nearer, where the quad wins; and the tie, which the sphere wins."""
    e = 2.0 ** -51
    spheres = [((x, 1.0, 0.0), 1.0, abi.RT_MAT_LAMBERTIAN) for x in (0.0, 10.0, 20.0)]
    quvs = [np.array([x - 2.0, y, -2.0, 4.0, 0.0, 0.0, 0.0, 0.0, 4.0]) for x, y in ((0.0, 0.0), (10.0, e), (20.0, -e))]
    rays = np.array([[x, -3.0, 0.0, 0.0, s, 0.0] for s in (1.0, 2.0) for x in (0.0, 10.0, 20.0)])
    return spheres, quvs, rays, [0, 1, 3 + 2, 0, 1, 3 + 2], [3.0, 3.0, 3.0 - e, 1.5, 1.5, (3.0 - e) / 2.0]


@pytest.mark.gpu
def test_ties_on_the_device(pkg, abi, sim, torch_cuda):
    """the tie rules through the megakernel, where quads_hit gets the lock-step walk's closest: test_ids_and_ties' world and rays as the
    pixels of a 6 x 1 frame — a sphere beats a quad at an equal t, the first of two coincident quads is kept — then without the sphere;
    and quads one ulp behind / in front of a sphere's root: the ids and t the host build names, both outcomes among them"""
    def frame(spheres, quvs, rays, n_spheres=None):
        sc, keep = _scene(abi, spheres, len(rays), 1)
        if n_spheres is not None:
            sc.n_spheres = n_spheres
        quads = _quad_array(abi, [_quad(abi, q) for q in quvs])
        rc, best, t, _ = sim.hit_world_v(sc, rays, quads=quads)
        assert rc == 0
        gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib(), quads=quads)
        try:
            _, p_t, p_b, key = _frames_of_both_variants(gs, rays, len(rays), 1, "ties")
        finally:
            gs.close()
        assert key == QUADS
        _assert_first_hits("ties", p_t, p_b, best, t)
        return p_b.tolist(), p_t.tolist()
    spheres, quvs, rays = _tie_world(abi)
    b, t = frame(spheres, quvs, rays)
    assert b == [2 + 0, 1, 2 + 1, 2 + 1, 0, -1] and t[:4] == [2.0, 0.5, 0.25, 3.0]
    b, t = frame(spheres, quvs, rays[:2], n_spheres=1)
    assert b == [1 + 0, 1 + 1] and t == [2.0, 0.5]
    spheres, quvs, rays, ids, ts = _ulp_world(abi)
    b, t = frame(spheres, quvs, rays)
    assert b == ids and t == ts, (b, t)
