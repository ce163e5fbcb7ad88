"""What the shutter probe computes, on the CPU: the host build of the probe's two calls (tests/flatmotion/flat_motion_sim.cpp
fm_list_surface: flats_hit through motion_tables at the ray's tau, then object_surface<true> — rt_core.h compiled by g++ with
-ffp-contract=off) against the restatement in plain Python floats (tests/flat_shutter_mini.py), on the worlds the device is later held to the
host build on (tests/flat_shutter_rays.py).  A break in rt_core.h that host and device share shows here; one the device alone has shows in
tests/test_flat_shutter_gpu.py.  Per world a fixed-seed subsample of 1 000 rays — in a `held` world 200 of each tie kind among them — through
every entry in Python: the id, front_face and every bit of t, P, the normal and the origin at tau; untouched outputs keep their sentinels."""
import numpy as np
import pytest

import flat_shutter_mini as SM
import flat_shutter_rays as R
import quad_rays as QR

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")
N_SUB = 1000
F64 = ("t", "P", "normal", "origin")


def bits_equal(a, b, rows=None):
    """{output: the number of rays whose value differs in any bit} — empty when the two sets of outputs are the same"""
    bad = {}
    for k in a:
        x, y = (np.ascontiguousarray(v if rows is None else v[rows]) for v in (a[k], b[k]))
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if not len(x):
            continue
        x, y = (v.view(np.uint64 if k in F64 else np.uint32).reshape(len(v), -1) for v in (x, y))
        n = int((x != y).any(axis=1).sum())
        if n:
            bad[k] = n
    return bad


def subsample(w, seed):
    m = len(w["rays"])
    rng = np.random.default_rng(seed)
    rows = set(rng.choice(m, N_SUB if "tie" not in w else N_SUB - 600, replace=False).tolist())
    if "tie" in w:
        for kind in range(3):
            rows |= set(rng.choice(np.flatnonzero(w["tie"] == kind), 200, replace=False).tolist())
    return np.array(sorted(rows))


def check(abi, w, seed, move="world", normals="world"):
    """host scan == host structure on every ray; host == restatement on the subsample; sentinels where nothing is written -> the scan's
    outputs, the structure's counts, the subsample"""
    m = len(w["rays"])
    scan, _ = R.host_pass(abi, w, False, move, normals, out=R.sentinels(m))
    tree, cnt = R.host_pass(abi, w, True, move, normals, out=R.sentinels(m))
    assert bits_equal(scan, tree) == {}, "the scan and the structure differ"
    acc = R.accepted(w, scan["best"])
    blank = R.sentinels(int((~acc).sum()))
    assert bits_equal({k: scan[k][~acc] for k in F64 + ("front",)}, {k: blank[k] for k in F64 + ("front",)}) == {}, "a ray that accepted nothing wrote"
    rows = subsample(w, seed)
    assert len(rows) >= 500
    mini = SM.restate(w, rows, R.ID_BASE, R.sentinels(m), move, normals)
    assert bits_equal(scan, mini, rows) == {}, "the host build differs from the restatement"
    return scan, cnt, rows


# the hit share over all rays and the moving-entry share among the hits of the reduced tables, as the host build gives them
SHARES = {"generic": (.54, .64), "den": (.43, .84), "edges": (.63, .63), "on_plane": (.28, .66), "t_range": (.65, .94), "magnitudes": (.017, .65),
          "non_finite": (.24, .60), "skewed": (.18, .67), "needle": (.17, .66)}


def class_conditions(cls, w, best, cnt, bvh=True):
    """what the nine tables must keep giving for the comparison to mean something (asserted from the host build, on the CPU and the GPU alike)"""
    acc = R.accepted(w, best)
    hits, moving = int(acc.sum()), float(((best[acc] - R.ID_BASE) % 2 == 0).mean())
    print(f"{cls}: {hits} of {len(best)} rays hit, moving share {moving:.2f}; structure: walk {cnt['rays_bvh']} scan {cnt['rays_scan']}")
    assert len(best) == 10_000 and cnt["rays_bvh"] + cnt["rays_scan"] == len(best)
    if cls in QR.STRADDLING:
        assert hits >= 0.10 * len(best)
    if cls == "magnitudes":
        assert hits >= 100
    assert moving >= 0.5
    if bvh:
        assert cnt["rays_bvh"] > 0
        if cls in ("den", "magnitudes", "non_finite"):
            assert cnt["rays_scan"] > 0, "the per-lane scan fallback is not reached"
    else:
        assert cnt["rays_scan"] == len(best)
    return hits, moving


@pytest.mark.parametrize("cls", QR.CLASSES)
def test_nine_ray_classes(abi, cls):
    """each ray with the table's own closest-so-far: the pruning of a swept box by a real closest, the range test against it"""
    w = R.class_world(abi, cls)
    scan, cnt, _ = check(abi, w, 6100 + QR.CLASSES.index(cls))
    hits, moving = class_conditions(cls, w, scan["best"], cnt)
    assert abs(hits / len(scan["best"]) - SHARES[cls][0]) < 0.01 and abs(moving - SHARES[cls][1]) < 0.015, (hits, moving)
    assert (w["closest"] < QR.T_MAX).sum() > 1000 or cls == "den"                  # (den's table has no bound of its own)
    assert {0.0, float(np.float32(1.0 - 2.0 ** -24))} <= set(w["tau"].tolist()) and len(set(w["tau"].tolist())) > 1000


@pytest.mark.parametrize("cls", R.HELD_CLASSES)
def test_a_hit_already_held(abi, cls):
    """best_in from {-1, the sphere, a flat id below the true hit, one above it}, closest the true t in half of the rays: on an exact tie a
    larger index held gives way, a smaller index and a sphere stay — through the scan and the structure alike"""
    w = R.held_world(abi, cls)
    scan, _, rows = check(abi, w, 6200 + QR.CLASSES.index(cls))
    for kind, name in enumerate(R.TIE_KINDS):
        sel = w["tie"] == kind
        print(f"{cls}: {int(sel.sum())} ties against a {name}")
        assert sel.sum() >= 100 and (w["closest"][sel] == w["true_t"][sel]).all()
        if name == "larger":
            assert (scan["best"][sel] == w["true_best"][sel]).all() and (scan["t"][sel] == w["true_t"][sel]).all()
        else:
            assert (scan["best"][sel] == w["best_in"][sel]).all() and (scan["t"][sel] == R.SENTINEL["t"]).all()
        assert (w["tie"][rows] == kind).sum() >= 200
    assert set(np.unique(w["best_in"][w["best_in"] < R.ID_BASE]).tolist()) == {-1, 0}


SMOOTH_WAYS = {"normals_and_motion": ("world", "world"), "normals_alone": (None, "world"), "motion_alone": ("world", None)}


@pytest.mark.parametrize("way", list(SMOOTH_WAYS))
def test_shading_normals_at_tau(abi, way):
    """200 triangles of the shading normals' adversarial classes three ways; with normals the weights come from the frame at tau, and every
    fallback of rt_flat_normal.h is taken on an entry that moves and on one that does not"""
    import smooth_mini as SMM
    w = R.smooth_world()
    move, normals = SMOOTH_WAYS[way]
    scan, _, rows = check(abi, w, 6300, move, normals)
    acc = R.accepted(w, scan["best"])
    on_aim = acc & (scan["best"] - R.ID_BASE == w["aim"])
    per_class = [int((on_aim & (w["cls"] == c)).sum()) for c in range(len(R.SMOOTH_CLASSES))]
    print(f"{way}: {int(acc.sum())} of {len(acc)} rays hit, on the entry aimed at per class {per_class}")
    if way != "normals_alone":                       # (without flat motion the rays moved along with their entries are off target)
        assert min(per_class) >= 100 and ((scan["best"][on_aim] - R.ID_BASE) % 2 == 0).sum() >= 1000
    if normals is not None:
        W = SM.World(w, R.ID_BASE, move, normals)
        fell = {}
        for i in rows[acc[rows]]:
            k = int(scan["best"][i]) - R.ID_BASE
            _, f = SMM.shade(W.at(k, float(w["tau"][i])), W.nrec[k], tuple(w["rays"][i, 3:].tolist()), tuple(scan["P"][i].tolist()))
            for b in (SMM.FELL_MM, SMM.FELL_SIDE, SMM.FELL_GRAZING):
                fell[b, k % 2] = fell.get((b, k % 2), 0) + bool(f & b)
        print(f"{way}: fallbacks (which, entry parity): {fell}")
        if way == "normals_and_motion":
            assert all(fell[b, p] > 0 for b in (SMM.FELL_MM, SMM.FELL_SIDE, SMM.FELL_GRAZING) for p in (0, 1)), fell


def test_still_bits(abi):
    """every displacement zero but a speck's that no ray reaches: the outputs are those of the same list without any motion, in every bit,
    and the origin is the entry's q, zeros of either sign included"""
    w = R.still_world(abi)
    scan, _, _ = check(abi, w, 6400)
    never, _ = R.host_pass(abi, w, False, move=None, out=R.sentinels(len(w["rays"])))
    assert bits_equal(scan, never) == {}
    acc = R.accepted(w, scan["best"])
    assert acc.sum() > 4000 and not (scan["best"] == R.ID_BASE + 100).any()
    for k in (101, 102):                                     # the origins made of zeros of either sign are reached
        assert (scan["best"] == R.ID_BASE + k).sum() >= 20 and (w["quvs"][k, 0:3] == 0.0).all() and np.signbit(w["quvs"][k, 0:3]).any()
    assert bits_equal({"origin": scan["origin"][acc]}, {"origin": np.ascontiguousarray(w["quvs"][scan["best"][acc] - R.ID_BASE, 0:3])}) == {}


def test_image_world(abi):
    """the 16 entries with images of the device's origin-to-texel test: the P and the origin at tau that feed the lookup there are the
    restatement's in the host build too, on every ray, and the lookups they give spread over the texels of both textures"""
    import flat_image_mini as IM
    w = R.image_world()
    m = len(w["rays"])
    scan, _, _ = check(abi, w, 6500)
    mini = SM.restate(w, np.arange(m), R.ID_BASE, R.sentinels(m))
    assert bits_equal(scan, mini) == {}
    acc = R.accepted(w, scan["best"])
    k = scan["best"][acc] - R.ID_BASE
    assert acc.sum() > 600 and (k % 2 == 0).sum() > 200 and (k % 2 == 1).sum() > 200
    table = IM.tex_table([(a.shape[1], a.shape[0], a.size) for a in w["textures"]])
    W = SM.World(w, R.ID_BASE)
    seen = set()
    for i in np.flatnonzero(acc):
        e = int(scan["best"][i]) - R.ID_BASE
        code, rec = IM.prepare(list(w["uvs"][e]), e % 2, w["modes"][e][0], w["modes"][e][1], 0, table, 0)
        assert code == IM.PRESENT
        at = W.at(e, float(w["tau"][i]))
        assert at.Q == tuple(scan["origin"][i].tolist())
        seen.add(IM.texel(rec, at.Q, at.u, at.v, at.w, tuple(scan["P"][i].tolist()))[2])
    assert len(seen) >= 32, len(seen)
