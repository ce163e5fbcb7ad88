"""The device media code on adversarial rays, bit for bit.

The contract of participating media is "the bits": rt_core.h medium_hit is a fixed sequence of IEEE f64 operations around
csrc/common/rt_neg_log.h.  tests/test_medium_cpu.py pins them for the host build against the restatement of tests/medium_mini.py, and
rt_neg_log against correctly rounded values; the device compiles the same text with another compiler and wraps it in another form — a cold
by-value call, rt_sqrt's own v_rsq_f64 sequence in front of the free-flight arithmetic, the library's expansion of three f64 divisions —
and a frame reaches it with some thousand ordinary segments.  Here the tables of tests/medium_rays.py (the CPU test's own) go through the
device:
  - rt_hip_neg_log_probe: rt_neg_log of the CPU test's 10^6 arguments, of the arguments of tests/golden/neg_log_cr.npz (so its "below 1
    ulp" holds on the device by equality) and of 10^5 arbitrary bit patterns, against tests/lane_sim.py's medium_neg_log_v;
  - rt_hip_medium_probe (librt_hip_probe.so): hit_world with a MediumCtx, one ray per thread with its own RNG address and shutter time,
    over the eight classes (100 worlds x 1 000 rays: the last wave of a launch is partial) and the adversarial walk worlds (static, moving,
    thin cells; the one with the wide tables is refused at creation, as every scene with media and wide tables is).  (best, bits of t) and the walk's work counters must equal lane_sim's hit_world_v, the g++ build of
    the same code.  With the CPU test this reads: device = host build = restatement;
  - rt_hip_render_rays_probe: the real MEDIUM megakernels render 64 x 48 frames whose camera rays are rays of the six finite classes of
    ordinary magnitude, in a world with a medium in the `large` list and media in cells — static and with movers (with the wide tables: refused).
    Sample 0's camera segment records the (closest, best) the lock-step walk returned, behind medium_hit's call sites in it: it must
    equal the host build's hit_world at that segment's RNG address and shutter time, under the grid walk and under the full scan.
There is no tolerance anywhere.  The conditions on the inputs are checked on the host build by the tests without the gpu mark
(tests/test_medium_cpu.py), whose cached results the device tests reuse.  non_finite and magnitudes rays go through the probe only."""
import ctypes as C
import functools

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import lane_sim
import medium_rays as MR

W, H, SPP, DEPTH = 64, 48, 2, 5                  # a frame of 3 072 camera rays, as tests/test_walk_rays_gpu.py
MEDIUM, MOTION = 128, 64
T_MAX = 1.7976931348623157e308


@pytest.fixture(scope="module")
def sim(abi):
    return lane_sim.load(abi)


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _sim():
    """the lane simulator and the ABI outside a fixture (the cached references below)"""
    from conftest import graft
    abi = graft.load_package().abi
    return lane_sim.load(abi), abi


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared tables are read-only)


# ------------------------------------------------------------------ rt_neg_log
def _neg_log_on_device(pkg, x):
    d_x = _dev(x)
    d_out = torch.full((len(x),), float("nan"), dtype=torch.float64, device="cuda:0")
    assert pkg.hip.probe_lib().rt_hip_neg_log_probe(d_x.data_ptr(), d_out.data_ptr(), len(x), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _assert_same_doubles(what, x, got, want):
    """bit for bit, except that a NaN must only match a NaN"""
    nan = np.isnan(want)
    bad = np.flatnonzero((np.isnan(got) != nan) | (~nan & (_bits(got) != _bits(want))))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(x)} differ; first arguments {[float(v).hex() for v in x[bad[:4]]]} device "
                           f"{[float(v).hex() for v in got[bad[:4]]]} host {[float(v).hex() for v in want[bad[:4]]]}")


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_device_neg_log_equals_the_host_build(pkg, abi, sim, torch_cuda):
    """the 10^6 arguments of test_neg_log_bits_accuracy_and_zero; the fixture's arguments, on which the device's error is then the host
    build's, below 1 ulp; 10^5 arbitrary bit patterns and the special values, where a NaN must match a NaN"""
    import test_medium_cpu as TC
    x = TC.neg_log_arguments()
    _assert_same_doubles("1 - k 2^-53", x, _neg_log_on_device(pkg, x), sim.medium_neg_log_v(x))
    fx, cr, residual, _ = TC.neg_log_fixture()
    got = _neg_log_on_device(pkg, fx)
    _assert_same_doubles("the fixture", fx, got, sim.medium_neg_log_v(fx))
    err = TC.neg_log_error_ulp(got, cr, residual)
    print(f"rt_neg_log on the device: worst error against the true value {err.max():.3f} ulp over {len(fx)} arguments")
    assert err.max() < 1.0
    rng = np.random.default_rng(1504)
    pat = rng.integers(0, 1 << 64, 100_000, dtype=np.uint64)
    pat[:20_000] &= np.uint64(0x800FFFFFFFFFFFFF)                      # subnormals of both signs
    pat[20_000:30_000] |= np.uint64(0x7FF0000000000000)               # NaNs of every payload, and the infinities
    pat[30_000:30_008] = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 5e-324, -5e-324]).view(np.uint64)
    y = pat.view(np.float64)
    assert np.isnan(y).sum() > 5000 and (y < 0.0).sum() > 30_000 and ((np.abs(y) < 2.0 ** -1022) & (y != 0.0)).sum() > 10_000
    want = sim.medium_neg_log_v(y)
    got = _neg_log_on_device(pkg, y)
    _assert_same_doubles("bit patterns", y, got, want)
    assert got[30_000] == np.inf and got[30_001] == np.inf and got[30_002] == -np.inf and np.isnan(got[30_003]) and _bits(got[30_004:30_005])[0] == 0


# ------------------------------------------------------------------ rt_hip_medium_probe on the classes
@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", MR.CLASSES)
def test_device_medium_code_equals_the_host_build(pkg, abi, sim, torch_cuda, cls):
    """one resident scene per world and its 1 000 rays through rt_hip_medium_probe in one launch (15 waves and a partial one), 100 launches,
    one copy back; against hit_world_v of the host build: object id, the bits of t, the walk's work counters"""
    worlds = MR.class_worlds(cls, sim)
    ref = MR.class_reference(cls, abi, sim)
    n = MR.N_W * MR.N_R
    d_rays = _dev(np.concatenate([w.rays for w in worlds]))
    d_node = _dev(np.concatenate([w.nodes for w in worlds]).view(np.int32))
    d_t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
    d_best = torch.full((n,), -2, dtype=torch.int32, device="cuda:0")
    d_work = torch.full((n, 2), -1, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    scenes = []
    try:
        for w, wd in enumerate(worlds):
            sc, keep = MR.scene(abi, wd.objs, wd.seed)
            gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib())
            scenes.append(gs)
            off = w * MR.N_R
            gs.medium_probe(d_rays.data_ptr() + 48 * off, d_node.data_ptr() + 4 * off, d_t.data_ptr() + 8 * off, d_best.data_ptr() + 4 * off, MR.N_R,
                            d_work=d_work.data_ptr() + 8 * off, stream=stream)
        torch.cuda.synchronize()
    finally:
        for gs in scenes:
            gs.close()
    g_t, g_best, g_work = d_t.cpu().numpy(), d_best.cpu().numpy(), d_work.cpu().numpy().view(np.uint32)
    _assert_hits(cls, g_best, g_t, g_work, ref.best, ref.t, ref.work, np.concatenate([w.rays for w in worlds]))
    took = int(ref.took.sum())
    print(f"{cls}: {took} of {n} rays take a medium (device = host build)")


def _assert_hits(what, g_best, g_t, g_work, best, t, work, rays):
    bad = np.flatnonzero((g_best != best) | (_bits(g_t) != _bits(t)))
    assert bad.size == 0, (f"{what}: the device's hit_world differs from the host build's on {bad.size} of {len(best)} rays; first {bad[:4].tolist()}: rays "
                           f"{rays[bad[:4]].tolist()} device {g_best[bad[:4]].tolist()} {[float(v).hex() for v in g_t[bad[:4]]]} host "
                           f"{best[bad[:4]].tolist()} {[float(v).hex() for v in t[bad[:4]]]}")
    assert (g_t[g_best < 0] == T_MAX).all(), "a miss leaves t = f64::MAX"
    if g_work is not None:
        bad = np.flatnonzero((g_work != work).any(axis=1))
        assert bad.size == 0, (f"{what}: the device walk differs from the host build's on {bad.size} rays; first {bad[:4].tolist()}: device "
                               f"{g_work[bad[:4]].tolist()} host {work[bad[:4]].tolist()}")


def _assert_wide_media_refused(pkg, abi, sc):
    """The device has no MEDIUM kernel over the wide tables: rt_hip_scene_create refuses such a scene (tests/test_medium_gpu.py
    test_media_with_wide_tables_are_refused), so there is no resident scene to probe.  The wide arm of hit_world_grid<true> is compiled
    for the host alone, where tests/test_medium_cpu.py walks it; here the refusal is what is checked."""
    with pytest.raises(pkg.host.RtError) as e:
        pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib())
    assert e.value.code == abi.RT_ERR_UNSUPPORTED and "wide tables" in str(e.value)


@functools.lru_cache(maxsize=None)
def _walk_reference(name):
    """(the walk world, the host build's best, t, work): drawn and walked with the world's environment set"""
    import os
    L, abi = _sim()
    wd = MR.WalkWorld(abi, name)
    old = {k: os.environ.get(k) for k in wd.env}
    os.environ.update(wd.env)
    try:
        rc, best, t, work = L.hit_world_v(wd.sc, wd.rays, wd.c1c, tau=wd.tau, node=wd.nodes)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    assert rc == 0
    return wd, best, t, work


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MR.WALK_WORLDS))
def test_device_walk_with_media_equals_the_host_build(pkg, abi, torch_cuda, monkeypatch, name):
    """the seven adversarial walk worlds of tests/test_medium_cpu.py — a quarter of the spheres media, moving media at three shutter times,
    the wide tables, RT_GRID_N thin cells — and their ray tables through rt_hip_medium_probe: (best, bits of t) and the walk's counters
    equal the host build's, which that test equates with the brute force of the contract.  wide_tables: refused at creation."""
    wd, best, t, work = _walk_reference(name)
    for k, v in wd.env.items():
        monkeypatch.setenv(k, v)
    n = len(wd.rays)
    if "RT_GRID_WIDE" in wd.env:
        _assert_wide_media_refused(pkg, abi, wd.sc)
        return
    gs = pkg.hip.HipScene(C.pointer(wd.sc), 0, library=pkg.hip.probe_lib(), center1=wd.c1c.tolist() if wd.moving else None)
    try:
        assert gs.query("media") == len(wd.media) and not gs.query("grid_wide")
        d_rays, d_node, d_tau = _dev(wd.rays), _dev(wd.nodes.view(np.int32)), _dev(wd.tau)
        d_t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
        d_best = torch.full((n,), -2, dtype=torch.int32, device="cuda:0")
        d_work = torch.full((n, 2), -1, dtype=torch.int32, device="cuda:0")
        gs.medium_probe(d_rays.data_ptr(), d_node.data_ptr(), d_t.data_ptr(), d_best.data_ptr(), n, d_tau=d_tau.data_ptr(), d_work=d_work.data_ptr(),
                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        gs.close()
    _assert_hits(name, d_best.cpu().numpy(), d_t.cpu().numpy(), d_work.cpu().numpy().view(np.uint32), best, t, work, wd.rays)
    is_medium = wd.dens > 0.0
    assert (is_medium[np.maximum(best, 0)] & (best >= 0)).mean() > 0.05 and (work[:, 1] > 2).mean() > 0.1


@pytest.mark.gpu
def test_medium_probe_refuses_a_scene_without_media(pkg, abi, torch_cuda):
    sc, keep = MR.scene(abi, [((0.0, 0.0, 0.0), 1.0, "opaque", 0.0)], 5)
    gs = pkg.hip.HipScene(C.pointer(sc), 0, library=pkg.hip.probe_lib())
    try:
        d_rays, d_node = _dev(np.zeros((8, 6))), _dev(np.zeros(8, np.int32))
        d_t, d_best = torch.zeros(8, dtype=torch.float64, device="cuda:0"), torch.zeros(8, dtype=torch.int32, device="cuda:0")
        with pytest.raises(pkg.host.RtError) as e:
            gs.medium_probe(d_rays.data_ptr(), d_node.data_ptr(), d_t.data_ptr(), d_best.data_ptr(), 8)
        assert e.value.code == abi.RT_ERR_INVALID
    finally:
        gs.close()


# ------------------------------------------------------------------ through the real MEDIUM megakernels
FRAME_CASES = ["static", "movers", "wide"]
PER_CLASS = W * H // len(MR.FRAME_CLASSES)        # 512 rays of each class


class _FrameWorld:
    """The worlds of six classes put into one scene: world 0 of generic, occluder_inside and nested, worlds 0 and 1 of tangent (a sphere in
    general position and a whole-number one), world 0 of surface_origin, 512 media of a boundary_density lattice, 24 opaque spheres so that
    there is a grid, and one thin medium of radius 300 around it all, which the table builder puts in the `large` list.  The frame's 3 072
    camera rays are 512 rays of each class; pixel p's camera segment has the RNG address (p, sample 0, node 0), and the densities of the
    boundary media are set from the host build's figures at THAT address.  movers: the spheres of the generic, occluder and nested worlds
    move while the shutter is open, every ray is taken at its pixel's sample-0 shutter time.  wide: the wide tables."""

    def __init__(self, abi, L, case):
        from mini_oracle import M32, philox4x32_10
        rng = np.random.default_rng(3100)                     # (one draw for the three cases: "the same world")
        pick = {"generic": [0], "tangent": [0, 1], "surface_origin": [0], "occluder_inside": [0], "nested": [0]}
        objs, rays, target = [], [], []
        for cls in MR.FRAME_CLASSES:
            if cls == "boundary_density":
                continue
            for w in pick[cls]:
                wd = MR.class_worlds(cls, L)[w]
                m = PER_CLASS // len(pick[cls])
                rays.append(wd.rays[:m])
                target.append(wd.target[:m] + len(objs))
                objs += list(wd.objs)
        n_own = len(objs)
        # the boundary lattice, away from the other worlds (they lie within 10 of the origin): 8 x 8 x 8 cells of side 8 from x = 20 on
        nb = PER_CLASS
        g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
        bc = g * 8.0 + np.array([20.0, -28.0, -28.0]) + rng.uniform(-1.0, 1.0, (nb, 3))
        br = rng.uniform(0.5, 1.5, nb)
        b_rays = np.where((np.arange(nb) % 2 == 0)[:, None], MR._through(rng, bc, br, nb, spread=0.7, far=(1.5, 3.0)), MR._inside(rng, bc, br, nb))
        first_b = n_own
        rays.insert(4, b_rays)                              # (in FRAME_CLASSES' order: generic, tangent, surface_origin, boundary_density, ...)
        target.insert(4, first_b + np.arange(nb))
        filler = [(rng.uniform(-12.0, 12.0, 3) + np.array([0.0, 40.0, 0.0]), rng.uniform(0.5, 1.5), "opaque", 0.0) for _ in range(24)]
        assert len(rays) == 7
        self.rays = np.ascontiguousarray(np.concatenate(rays))
        self.target = np.concatenate(target)
        assert self.rays.shape == (W * H, 6) and np.isfinite(self.rays).all() and np.abs(self.rays).max() < 1e3
        self.seed = 0x5EED7000
        self.b_rows = np.arange(3 * PER_CLASS, 4 * PER_CLASS)
        self.j = rng.integers(-2, 3, nb)
        addr = np.stack([self.b_rows, np.zeros(nb), first_b + np.arange(nb)], axis=1).astype(np.uint32)
        geom = np.concatenate([bc, br[:, None]], axis=1)
        terms = L.medium_terms_v(b_rays, geom, np.ones(nb), addr, self.seed)
        ok = (terms[:, 7] >= 2.0) & (terms[:, 4] > 0.0)
        dens = np.where(ok, L.medium_neg_log_v(1.0 - terms[:, 4]) / (terms[:, 3] * (1.0 + self.j * MR.EPS)), 1.0)
        self.b_terms = L.medium_terms_v(b_rays, geom, dens, addr, self.seed)
        self.objs = objs + [(bc[i], br[i], "medium", dens[i]) for i in range(nb)] + filler + [((0.0, 0.0, 0.0), 300.0, "medium", 2e-4)]
        self.big = len(self.objs) - 1
        self.is_medium = np.array([o[2] == "medium" for o in self.objs])
        self.sc, self.keep = MR.scene(abi, self.objs, self.seed, W, H, SPP, DEPTH)
        self.env = {"RT_GRID_WIDE": "1"} if case == "wide" else {}
        self.center1 = self.tau = None
        if case == "movers":
            c1 = np.array([np.asarray(o[0], np.float64) for o in self.objs])
            movers = [i for i in range(n_own) if i not in set(np.concatenate(target[1:4]).tolist())]      # not the tangent and surface_origin spheres
            c1[movers] += rng.uniform(-0.4, 0.4, (len(movers), 3))
            self.center1 = c1
            self.movers = movers
            seed = self.seed        # sample 0's shutter time of every pixel (tests/test_motion.py tau_of)
            self.tau = np.array([float(philox4x32_10(p, 0, 0xFFFFFFFD, 0, seed & M32, (seed >> 32) & M32)[0] >> 8) * 2.0 ** -24 for p in range(W * H)], np.float32)
        self.node = np.zeros(W * H, np.uint32)
        import os
        old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        try:
            rc, self.best, self.t, _ = L.hit_world_v(self.sc, self.rays, center1=self.center1, tau=self.tau, node=self.node)
            rc2, self.info, self.listed, self.is_large = L.medium_tables(self.sc, self.center1)
        finally:
            for k, v in old.items():
                os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
        assert rc == 0 and rc2 == 0


@functools.lru_cache(maxsize=None)
def _frame_world(case):
    L, abi = _sim()
    return _FrameWorld(abi, L, case)


@pytest.mark.parametrize("case", FRAME_CASES)
def test_frame_worlds_reach_the_medium_call_sites(abi, case):
    """the inputs of the megakernel test on the host build: a medium in the `large` list and media in cells of a grid; the big medium, the
    media in cells and the opaque spheres each win camera rays; the boundary rays' free-flight distances lie within ulps of their chords at
    the address the frame uses, on both sides"""
    wd = _frame_world(case)
    assert wd.info[1] > 0 and bool(wd.info[6]) == (case == "wide"), "a gridded world"
    assert wd.is_large[wd.big] == 1 and wd.listed[wd.big] == 0, "the big medium is in the `large` list"
    in_cells = wd.is_medium & (wd.is_large == 0) & (wd.listed > 0)
    assert in_cells.sum() >= 500, int(in_cells.sum())
    hit = wd.best >= 0
    took = hit & wd.is_medium[np.maximum(wd.best, 0)]
    print(f"{case}: {int(hit.sum())} of {W * H} rays hit, {int(took.sum())} in a medium ({int((wd.best == wd.big).sum())} in the big one), "
          f"{len(np.unique(wd.best[took]))} media win")
    assert (took & (wd.best != wd.big) & in_cells[np.maximum(wd.best, 0)]).sum() >= 0.3 * W * H and (wd.best == wd.big).sum() >= 20 and (hit & ~took).sum() >= 50
    assert (~hit).sum() + (wd.best == wd.big).sum() >= 100, "rays whose own medium lets them through"
    stage = wd.b_terms[:, 7]
    off = (wd.b_terms[:, 5] - wd.b_terms[:, 3]) / np.spacing(wd.b_terms[:, 3])
    assert (stage >= 2).mean() > 0.99 and (np.abs(off[stage >= 2]) <= 8.0).all() and (stage == 3).mean() >= 0.30 and (stage == 2).mean() >= 0.30
    rows = wd.b_rows[stage == 3]
    assert (wd.best[rows] == wd.target[rows]).mean() > 0.9, "a boundary ray whose candidate is accepted ends in its own medium"
    if case == "movers":
        assert len(wd.movers) >= 5 and len(np.unique(wd.tau)) > 3000


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


@pytest.mark.gpu
@pytest.mark.parametrize("case", FRAME_CASES)
def test_megakernel_first_hit_with_media(pkg, abi, torch_cuda, monkeypatch, case):
    """64 x 48 at spp 2, depth 5 through rt_hip_render_rays_probe, at "variant" 0 (the grid walk) and 1 (the full scan): the (closest, best)
    the MEDIUM megakernel's hit_world returned for sample 0's camera segment of every pixel equals lane_sim's hit_world_v at that segment's
    RNG address (pixel, sample 0, node 0) and shutter time, in id and in the bits of t (a miss: -1); the two variants' frames are equal bit
    for bit.  wide: the device has no MEDIUM kernel over the wide tables; the scene is refused, and that is asserted."""
    wd = _frame_world(case)
    for k, v in wd.env.items():
        monkeypatch.setenv(k, v)
    if case == "wide":
        _assert_wide_media_refused(pkg, abi, wd.sc)
        return
    gs = pkg.hip.HipScene(C.pointer(wd.sc), 0, library=pkg.hip.probe_lib(), center1=wd.center1.tolist() if wd.center1 is not None else None)
    try:
        assert not gs.query("grid_wide")
        a = _probe_frame(gs, wd.rays, W, H)
        gs.set_option("variant", 1)
        b = _probe_frame(gs, wd.rays, W, H)
    finally:
        gs.close()
    for what, (frame, p_t, p_b, key) in (("variant 0", a), ("variant 1", b)):
        assert key & MEDIUM and bool(key & MOTION) == (case == "movers"), (case, what, key)
        bad = np.flatnonzero((p_b != wd.best) | ((wd.best >= 0) & (_bits(p_t) != _bits(wd.t))))
        assert bad.size == 0, (f"{case} {what}: the megakernel's first hit differs from the host build of hit_world on {bad.size} of {W * H} rays; first "
                               f"{bad[:5].tolist()}: device {p_b[bad[:5]].tolist()} {p_t[bad[:5]].tolist()} host {wd.best[bad[:5]].tolist()} {wd.t[bad[:5]].tolist()}")
        assert np.isfinite(frame[1]).all() and frame[2] >= W * H * SPP
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1].view(np.uint32), b[0][1].view(np.uint32)) and a[0][2] == b[0][2], f"{case}: variant 1's frame differs"
    assert a[3] == b[3]
