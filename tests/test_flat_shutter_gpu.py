"""The device surface of flat primitives that move within the frame, ray by ray: rt_hip_flat_shutter_probe
(include/rt_abi_test_flat_motion.h) — motion_tables at the ray's tau, flats_hit through them with the ray's own closest-so-far and the hit
it already holds, object_surface<true> of a newly accepted flat entry: what a QUADS ∧ MOTION megakernel does for a segment — against the host
build of the same two calls (tests/flat_motion_sim.py list_surface), itself held to the restatement by tests/test_flat_shutter_cpu.py.
Every comparison is on the bits: the id, front_face, t, P, the normal and the origin the kernel leaves in g.cx, g.cy, g.cz; no tolerance
anywhere.  Outputs are pre-filled with sentinels: a ray that accepts nothing leaves them untouched, and nothing is written past a table."""
import ctypes as C

import numpy as np
import pytest

try:   # (before librt_hip.so is loaded: the process then holds ONE HIP runtime, torch's)
    import torch
except ImportError:
    torch = None

import flat_shutter_mini as SM
import flat_shutter_rays as R
import quad_rays as QR
from test_flat_shutter_cpu import F64, SMOOTH_WAYS, bits_equal, class_conditions

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
GUARD = 8                                            # rows behind every output table that must keep their sentinels
CHUNK, BLOCK = 1000, 192                             # launches of 1 000 threads in workgroups of 192: five full ones and a partial last wave
WIDTH = dict(best=1, t=1, P=3, normal=3, front=1, origin=3)


@pytest.fixture(scope="module")
def torch_cuda():
    assert torch is not None and torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class Scene:
    """a device scene over a world of tests/flat_shutter_rays.py, created through the probe library: one sphere far behind everything
    (entry k is object 1 + k), which moves when `sphere_moves`; the world's normals and motion unless told otherwise"""

    def __init__(self, pkg, abi, w, bvh, move="world", normals="world", sphere_moves=False, textures=None, images=None, quads=True):
        self.spheres = (abi.RtSphere * 1)()
        self.spheres[0].center[:] = [0.0, 0.0, -60.0]
        self.spheres[0].radius, self.spheres[0].kind, self.spheres[0].fuzz_or_ior = 0.5, abi.RT_MAT_LAMBERTIAN, 1.5
        self.spheres[0].albedo[:] = [0.6, 0.5, 0.7]
        self.sc = abi.RtScene(abi_version=abi.RT_ABI_VERSION, width=8, height=8, samples_per_pixel=2, max_depth=5, sky_mode=abi.RT_SKY_GRADIENT,
                              spheres=self.spheres, n_spheres=1, seed=4242)
        self.sc.cam_origin[:] = [0.0, 0.0, 30.0]; self.sc.cam_lower_left[:] = [-1.5, -1.0, 29.0]
        self.sc.cam_horizontal[:] = [3.0, 0.0, 0.0]; self.sc.cam_vertical[:] = [0.0, 2.0, 0.0]
        if textures is not None:
            self.textures = textures
            self.tex = (abi.RtTexture * len(textures))()
            for i, a in enumerate(textures):
                self.tex[i].rgb8 = a.ctypes.data_as(C.POINTER(C.c_uint8))
                self.tex[i].nbytes, self.tex[i].height, self.tex[i].width = a.size, a.shape[0], a.shape[1]
            self.sc.textures, self.sc.n_textures = self.tex, len(textures)
        self.flats = R.flats(abi, w) if quads else None
        self.gs = pkg.hip.HipScene(C.pointer(self.sc), 0, library=pkg.hip.probe_lib(), center1=[(0.25, 0.0, -60.0)] if sphere_moves else None,
                                   quads=self.flats, flat_bvh=bvh and quads)
        move = w["move"] if isinstance(move, str) else move
        normals = w["normals"] if isinstance(normals, str) else normals
        if quads and normals is not None:
            self.gs.set_flat_normals(normals)
        if quads and images is not None:
            self.gs.set_flat_images(images)
        if quads and move is not None:
            self.gs.set_flat_motion(move)

    def __enter__(self):
        return self.gs

    def __exit__(self, *exc):
        self.gs.close()


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")      # (a copy: the shared tables are read-only)


class Outputs:
    """the six output tables on the device, pre-filled with the sentinels of flat_shutter_rays.sentinels, GUARD rows behind each"""

    def __init__(self, m):
        self.m = m
        blank = R.sentinels(m + GUARD)
        self.d = {k: _dev(v) for k, v in blank.items()}

    def ptrs(self, off):
        """d_best, d_t, d_point, d_normal, d_front, d_origin at ray `off`"""
        return [self.d[k].data_ptr() + off * WIDTH[k] * self.d[k].element_size() for k in ("best", "t", "P", "normal", "front", "origin")]

    def fetch(self):
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.d.items()}
        blank = R.sentinels(GUARD)
        assert bits_equal({k: got[k][self.m:] for k in got}, blank) == {}, "the probe wrote past a table"
        return {k: np.ascontiguousarray(v[:self.m]) for k, v in got.items()}


def probe(gs, w, rows=None, block=BLOCK, chunk=CHUNK):
    """rt_hip_flat_shutter_probe over the world's rays (or `rows` of them) in launches of `chunk` threads -> the outputs"""
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    rays, tau, closest = pick(w["rays"]), pick(w["tau"]), pick(w["closest"])
    m = len(rays)
    d_rays, d_tau, d_closest = _dev(rays), _dev(tau), _dev(closest)
    d_held = _dev(pick(w["best_in"])) if w["best_in"] is not None else None
    out = Outputs(m)
    stream = torch.cuda.current_stream().cuda_stream
    for off in range(0, m, chunk):
        b, t, P, nrm, front, origin = out.ptrs(off)
        gs.flat_shutter_probe(d_rays.data_ptr() + 48 * off, d_closest.data_ptr() + 8 * off, min(chunk, m - off), b, t, P, nrm, front, origin,
                              d_tau=d_tau.data_ptr() + 4 * off, d_best_in=d_held.data_ptr() + 4 * off if d_held is not None else 0, block=block,
                              stream=stream)
    return out.fetch()


def quad_probe(gs, w, n_quads):
    """rt_hip_quad_probe over the whole list: the plain path (GlobalTables) -> best, t, P, normal, front with the same sentinels"""
    m = len(w["rays"])
    d_rays, d_closest = _dev(w["rays"]), _dev(w["closest"])
    out = Outputs(m)
    b, t, P, nrm, front, _ = out.ptrs(0)
    gs.quad_probe(d_rays.data_ptr(), d_closest.data_ptr(), m, 0, n_quads, b, t, P, nrm, front, stream=torch.cuda.current_stream().cuda_stream)
    got = out.fetch()
    return {k: got[k] for k in ("best", "t", "P", "normal", "front")}


def same(got, want, what):
    bad = bits_equal(want, got)
    assert bad == {}, f"{what}: rays that differ from the host build in some bit, per output: {bad}"


def untouched(w, got):
    """a ray that accepted no new flat entry left every output but the id as it was"""
    acc = R.accepted(w, got["best"])
    blank = R.sentinels(int((~acc).sum()))
    assert bits_equal({k: got[k][~acc] for k in F64 + ("front",)}, {k: blank[k] for k in F64 + ("front",)}) == {}, "a ray that accepted nothing wrote"
    return acc


# ------------------------------------------------------------------ a. nine ray classes x {scan, structure}
@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
@pytest.mark.parametrize("cls", QR.CLASSES)
def test_nine_ray_classes(pkg, abi, torch_cuda, cls, bvh):
    """10^4 rays of each class of tests/quad_rays.py, each at its own tau (0, 1 - 2^-24, multiples of 2^-24) and with the TABLE'S OWN
    closest-so-far: the pruning of swept boxes by a real closest, the range test against it, the surface of the entry at tau.  No ray is
    left out."""
    w = R.class_world(abi, cls)
    want, cnt = R.host_pass(abi, w, bvh, out=R.sentinels(len(w["rays"])))
    class_conditions(cls, w, want["best"], cnt, bvh)
    with Scene(pkg, abi, w, bvh) as gs:
        assert gs.query("flat_motion") == 50 and (gs.query("flat_bvh") > 0) == bvh
        got = probe(gs, w)
    same(got, want, f"{cls} bvh={bvh}")
    untouched(w, got)


# ------------------------------------------------------------------ b. a hit already held
@pytest.mark.gpu
@pytest.mark.parametrize("cls", R.HELD_CLASSES)
def test_a_hit_already_held(pkg, abi, torch_cuda, cls):
    """best_in from {-1, the sphere, a flat id below the true hit, one above it} and closest the ray's true t in half of the rays: exact ties
    against a larger index (it gives way), a smaller index and a sphere (they stay), each at least 100 times; the scan and the structure
    equal the host build and each other"""
    w = R.held_world(abi, cls)
    got = {}
    for bvh in (False, True):
        want, _ = R.host_pass(abi, w, bvh, out=R.sentinels(len(w["rays"])))
        with Scene(pkg, abi, w, bvh) as gs:
            got[bvh] = probe(gs, w)
        same(got[bvh], want, f"{cls} bvh={bvh}")
        untouched(w, got[bvh])
    same(got[True], got[False], f"{cls}: the structure against the scan")
    for kind, name in enumerate(R.TIE_KINDS):
        sel = w["tie"] == kind
        assert sel.sum() >= 100 and (w["closest"][sel] == w["true_t"][sel]).all()
        gave_way = got[True]["best"][sel] == w["true_best"][sel]
        assert gave_way.all() if name == "larger" else (got[True]["best"][sel] == w["best_in"][sel]).all(), name


# ------------------------------------------------------------------ c. shading normals at tau
@pytest.mark.gpu
@pytest.mark.parametrize("way", list(SMOOTH_WAYS))
def test_shading_normals_at_tau(pkg, abi, torch_cuda, way):
    """200 triangles of the shading normals' adversarial classes, 50 rays each, three ways: normals and flat motion; normals alone with
    one moving sphere far away — FLAT_NORMALS_BIT alone reaches the normals through flat_surface_shutter, and must give what
    rt_hip_quad_probe gives through flat_shading_normal on the same scene, the origin the record's q —; motion alone"""
    w = R.smooth_world()
    move, normals = SMOOTH_WAYS[way]
    for bvh in (False, True):
        want, _ = R.host_pass(abi, w, bvh, move, normals, out=R.sentinels(len(w["rays"])))
        with Scene(pkg, abi, w, bvh, move, normals, sphere_moves=way == "normals_alone") as gs:
            assert (gs.query("flat_motion") > 0) == (move is not None) and gs.query("motion") == (1 if way == "normals_alone" else 0)
            got = probe(gs, w)
            plain = quad_probe(gs, w, len(w["quvs"])) if way == "normals_alone" else None
        same(got, want, f"{way} bvh={bvh}")
        acc = untouched(w, got)
        assert acc.sum() > 5000
        if plain is not None:
            same({k: got[k] for k in plain}, plain, f"{way} bvh={bvh}: the MOTION path against the plain one")
            assert bits_equal({"origin": got["origin"][acc]}, {"origin": np.ascontiguousarray(w["quvs"][got["best"][acc] - R.ID_BASE, 0:3])}) == {}


# ------------------------------------------------------------------ d. still bits
@pytest.mark.gpu
@pytest.mark.parametrize("bvh", [False, True])
def test_still_bits(pkg, abi, torch_cuda, bvh):
    """every displacement zero but a far speck's: every output is rt_hip_quad_probe's on the same list created without motion, in every
    bit, and the origin is the entry's q — zeros of either sign included"""
    w = R.still_world(abi)
    want, _ = R.host_pass(abi, w, bvh, out=R.sentinels(len(w["rays"])))
    with Scene(pkg, abi, w, bvh) as gs:
        assert gs.query("flat_motion") == 1
        got = probe(gs, w)
    with Scene(pkg, abi, w, bvh, move=None) as never:
        assert never.query("flat_motion") == 0 and never.query("motion") == 0
        plain = quad_probe(never, w, len(w["quvs"]))
    same(got, want, f"still bvh={bvh}")
    same({k: got[k] for k in plain}, plain, f"still bvh={bvh}: against the scene without motion")
    acc = untouched(w, got)
    k = got["best"][acc] - R.ID_BASE
    assert acc.sum() > 4000 and (k == 101).sum() >= 20 and (k == 102).sum() >= 20 and not (k == 100).any()
    assert bits_equal({"origin": got["origin"][acc]}, {"origin": np.ascontiguousarray(w["quvs"][k, 0:3])}) == {}


# ------------------------------------------------------------------ e. the origin feeds the image lookup
@pytest.mark.gpu
def test_the_origin_feeds_the_image_lookup(pkg, abi, torch_cuda):
    """16 entries with 8 x 8 images, wrap modes mixed, every other one moving: the probe's own d_origin and d_point go into
    rt_hip_flat_image_probe, and the rgb is the restatement's (tests/flat_image_mini.py) on the frame at tau that plain Python floats
    give (flat_shutter_mini): kernel -> origin -> texel on the device"""
    import flat_image_mini as IM
    w = R.image_world()
    n, textures, uvs, modes, tau = len(w["quvs"]), w["textures"], w["uvs"], w["modes"], w["tau"]
    images = (abi.RtFlatImage * n)(*[abi.flat_image(k % 2, uvs[k], *modes[k]) for k in range(n)])
    mini = SM.restate(w, np.arange(len(w["rays"])), R.ID_BASE, R.sentinels(len(w["rays"])))
    L = pkg.hip.probe_lib()
    L.rt_hip_flat_image_probe.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p]
    with Scene(pkg, abi, w, False, textures=textures, images=images) as gs:
        assert gs.query("flat_images") == n and gs.query("flat_motion") == n // 2
        got = probe(gs, w)
        same(got, mini, "the image world against the restatement")
        acc = R.accepted(w, got["best"])
        rows = np.flatnonzero(acc)
        k = (got["best"][rows] - R.ID_BASE).astype(np.uint32)
        d_k, d_o, d_P = _dev(k.view(np.int32)), _dev(got["origin"][rows]), _dev(got["P"][rows])
        d_rgb = torch.full((len(rows) + GUARD, 3), -7.0, dtype=torch.float32, device="cuda:0")
        pkg.hip._check(L.rt_hip_flat_image_probe(gs._h, d_k.data_ptr(), d_o.data_ptr(), d_P.data_ptr(), d_rgb.data_ptr(), len(rows),
                                                 torch.cuda.current_stream().cuda_stream), L)
        torch.cuda.synchronize()
        rgb = d_rgb.cpu().numpy()
    assert (rgb[len(rows):] == -7.0).all() and len(rows) > 600 and ((k % 2) == 0).sum() > 200
    table = IM.tex_table([(a.shape[1], a.shape[0], a.size) for a in textures])
    W = SM.World(w, R.ID_BASE)
    want = np.zeros((len(rows), 3), np.float32)
    for j, i in enumerate(rows):
        e = int(k[j])
        code, rec = IM.prepare(list(uvs[e]), e % 2, modes[e][0], modes[e][1], 0, table, 0)
        assert code == IM.PRESENT
        at = W.at(e, float(tau[i]))
        index = IM.texel(rec, at.Q, at.u, at.v, at.w, tuple(mini["P"][i].tolist()))[2]
        want[j] = IM.colour(textures[e % 2].reshape(-1), index - table[e % 2][0])
    assert len({tuple(x) for x in want.tolist()}) >= 32, "the lookups do not spread over the texels"
    assert np.array_equal(rgb[:len(rows)].view(np.uint32), want.view(np.uint32)), int((rgb[:len(rows)].view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())


# ------------------------------------------------------------------ f. launch shapes and refusals
@pytest.mark.gpu
def test_launch_shapes(pkg, abi, torch_cuda):
    """workgroups of 1, 64, 96 and 1024 threads and launches of 1, 63 and 65 rays give the bits of the launches of 1 000 in workgroups of 192"""
    w = R.class_world(abi, "generic")
    rows = np.arange(0, 10_000, 7)[:1300]                # (a slice over every entry)
    with Scene(pkg, abi, w, True) as gs:
        ref = probe(gs, w, rows)
        assert R.accepted(w, ref["best"]).sum() > 400
        for block in (1, 64, 96, 1024):
            same(probe(gs, w, rows, block=block), ref, f"block {block}")
        for n in (1, 63, 65):
            got = probe(gs, w, rows[:n], block=64, chunk=n)
            same(got, {k: v[:n] for k, v in ref.items()}, f"n {n}")
        same(probe(gs, w, rows[:130], block=96, chunk=65), {k: v[:130] for k, v in ref.items()}, "two launches of 65")


@pytest.mark.gpu
def test_refusals(pkg, abi, torch_cuda):
    """n = 0 launches nothing; a null required pointer, a block out of range, a scene without flat primitives and one in which nothing
    moves are RT_ERR_INVALID, d_tau and d_best_in may be null; after each refusal the scene renders the frame it rendered before"""
    w = R.class_world(abi, "generic")
    L = pkg.hip.probe_lib()
    rows = np.arange(256)
    d_rays, d_tau, d_closest = _dev(w["rays"][rows]), _dev(w["tau"][rows]), _dev(w["closest"][rows])
    d_held = _dev(np.full(len(rows), -1, np.int32))
    stream = torch.cuda.current_stream().cuda_stream

    def call(gs, out, n=len(rows), block=BLOCK, null=None, tau=True, held=True):
        args = [gs._h if gs is not None else None, d_rays.data_ptr(), d_tau.data_ptr() if tau else None, d_closest.data_ptr(),
                d_held.data_ptr() if held else None, n, block, *out.ptrs(0), stream]
        if null is not None:
            args[null] = None
        return L.rt_hip_flat_shutter_probe(*args)

    def refused(gs, before, what, **kw):
        out = Outputs(len(rows))
        assert call(gs, out, **kw) == abi.RT_ERR_INVALID, what
        same(out.fetch(), R.sentinels(len(rows)), what + ": nothing is written")
        if gs is not None:
            assert np.array_equal(gs.render_to_host()[0], before), what + ": the frame changed"

    with Scene(pkg, abi, w, True) as gs:
        before = gs.render_to_host()[0]
        out = Outputs(len(rows))
        assert call(gs, out) == abi.RT_OK
        ref = out.fetch()
        assert R.accepted(w, ref["best"]).sum() > 50
        out = Outputs(len(rows))
        assert call(gs, out, n=0) == abi.RT_OK                                      # n = 0: nothing is launched, nothing written
        same(out.fetch(), R.sentinels(len(rows)), "n = 0")
        out = Outputs(len(rows))
        assert call(gs, out, held=False) == abi.RT_OK                               # no d_best_in: -1
        same(out.fetch(), ref, "d_best_in NULL")
        out = Outputs(len(rows))
        assert call(gs, out, tau=False) == abi.RT_OK                                # no d_tau: time 0
        zero = dict(w, rays=w["rays"][rows], tau=np.zeros(len(rows), np.float32), closest=w["closest"][rows])
        same(out.fetch(), R.host_pass(abi, zero, True, out=R.sentinels(len(rows)))[0], "d_tau NULL")
        for null, name in ((0, "the scene"), (1, "d_rays"), (3, "d_closest"), (7, "d_best"), (8, "d_t"), (9, "d_point"), (10, "d_normal"), (11, "d_front"),
                           (12, "d_origin")):
            refused(gs if null else None, before, name + " NULL", null=null)
        for block in (0, 1025, 0xFFFFFFFF):
            refused(gs, before, f"block {block}", block=block)
        assert np.array_equal(gs.render_to_host()[0], before)
    with Scene(pkg, abi, w, False, move=None) as still:                             # flat primitives, nothing moves: DevScene::motion is null
        refused(still, still.render_to_host()[0], "nothing moves")
    with Scene(pkg, abi, w, False, sphere_moves=True, quads=False) as bare:         # a moving sphere, no flat primitive
        assert bare.query("motion") == 1
        refused(bare, bare.render_to_host()[0], "no flat primitive")
    with Scene(pkg, abi, w, False, move=None, sphere_moves=True) as plain:          # no header slot at all: every bit of n_tris clear
        want, _ = R.host_pass(abi, dict(w, rays=w["rays"][rows], tau=w["tau"][rows], closest=w["closest"][rows]), False, move=None,
                              out=R.sentinels(len(rows)))
        out = Outputs(len(rows))
        assert call(plain, out) == abi.RT_OK
        same(out.fetch(), want, "a moving sphere and still flat primitives")
