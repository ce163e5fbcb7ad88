"""Shading normals on triangles and meshes without a GPU: the host build of csrc/common/rt_flat_normal.h against the
restatement (tests/smooth_mini.py) bit for bit on adversarial tables; the prepare step; the schema, the writer's round trip and the load
errors; and the checks that need no restatement (the axis-aligned identity's premise, the sphere limit on the host build)."""
import json
import math

import numpy as np
import pytest

import smooth_mini as SMM
import smooth_points as SP
import smooth_sim
import smooth_worlds as SW
import quad_mini as QM
from test_medium_gpu import _cfg, _lam, _load


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _same_f64(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("cls", SP.CLASSES)
def test_host_build_equals_the_restatement_bit_for_bit(cls):
    """prepare and shade on >= 1e5 points per class: the record, the normal and WHICH fallback was taken"""
    L = smooth_sim.load()
    quv, nr, d, P = SP.table(cls)
    assert len(quv) >= 100_000
    with np.errstate(all="ignore"):
        kind, rec = L.prepare(nr)
        rec_in = np.where((kind == SMM.BAD)[:, None], nr, rec)   # (a refused vector still goes through shade: a NaN falls back)
        nrm, fell, st = L.shade_each(quv, rec_in, d, P)
    taken = {SMM.FELL_MM: 0, SMM.FELL_SIDE: 0, SMM.FELL_GRAZING: 0, 0: 0}
    bad = 0
    for i in range(len(quv)):
        k, r = SMM.prepare(nr[i])
        assert k == kind[i], (cls, i, k, kind[i])
        if k != SMM.BAD:
            assert all(_same_f64(r, rec[i])), (cls, i)
        c = QM.QuadConsts(quv[i, 0:3], quv[i, 3:6], quv[i, 6:9])
        if not c.ok:
            assert st[i] != 0, (cls, i)
            bad += 1
            continue
        assert st[i] == 0, (cls, i)
        try:
            n, f = SMM.shade(c, tuple(rec_in[i]), tuple(d[i]), tuple(P[i]))
        except OverflowError:   # (math.sqrt never raises; a float product never does: kept for clarity)
            raise
        assert f == fell[i], (cls, i, f, fell[i])
        assert all(_same_f64(n, nrm[i])), (cls, i, n, nrm[i])
        taken[0] += f == 0
        for b in (SMM.FELL_MM, SMM.FELL_SIDE, SMM.FELL_GRAZING):
            taken[b] += bool(f & b)
    print(cls, "fallbacks taken:", taken, "refused entries:", bad)
    if cls == "generic":
        assert taken[0] > 0.4 * len(quv)
    if cls == "opposite":
        assert taken[SMM.FELL_MM] > 1000 and taken[0] + taken[SMM.FELL_SIDE] + taken[SMM.FELL_GRAZING] > 1000   # both sides of 1e-24
    if cls == "side":
        assert taken[SMM.FELL_SIDE] > 1000 and taken[0] + taken[SMM.FELL_GRAZING] > 1000
    if cls == "grazing":
        assert taken[SMM.FELL_GRAZING] > 1000 and taken[0] > 1000
    if cls == "non_finite":
        assert (kind == SMM.BAD).sum() > 1000 and taken[SMM.FELL_MM] > 1000


def test_prepare_zero_records_refusals_and_unit_length():
    L = smooth_sim.load()
    z = np.zeros((4, 9)); z[1, 4] = -0.0; z[2] = -0.0
    kind, rec = L.prepare(z)
    assert list(kind) == [SMM.FLAT] * 4 and not _bits(rec).any()          # +0.0 and -0.0 alike: flat, nine +0.0
    one = np.array([[0, 0, 2.0, 0, 3.0, 0, 1e-100, 0, 0]])
    kind, rec = L.prepare(one)
    assert kind[0] == SMM.SMOOTH and list(rec[0]) == [0, 0, 1.0, 0, 1.0, 0, 1.0, 0, 0]
    for bad in ([0, 0, 1, 0, 0, 0, 0, 0, 1], [0, 0, 1, 0, math.nan, 0, 0, 0, 1], [0, 0, 1, math.inf, 0, 0, 0, 0, 1], [1e-170, 0, 0, 0, 1, 0, 0, 0, 1],
                [1e160, 0, 0, 0, 1, 0, 0, 0, 1]):
        assert L.prepare(np.array([bad], np.float64))[0][0] == SMM.BAD == SMM.prepare(bad)[0], bad


def test_axis_aligned_identity_premise():
    """y / sqrt(y * y) == 1 exactly for the gamma + alpha + beta sums that occur: with one axis as all three normals m is y times the axis"""
    L = smooth_sim.load()
    rng = np.random.default_rng(7)
    a = rng.uniform(0, 1, 200_000); b = rng.uniform(0, 1, 200_000) * (1 - a)
    y = ((1.0 - a) - b + a) + b
    assert all(L.unit_1d(v) == 1.0 for v in y[:50_000])
    quv = np.array([0.3, -0.2, 1.0, 1.25, 0, 0, 0, 1.25, 0])
    rec = np.array([0, 0, 1.0] * 3)
    P = quv[0:3] + a[:, None] * quv[3:6] + b[:, None] * quv[6:9]
    d = rng.uniform(-1, 1, (len(a), 3))
    st, nrm, fell = L.shade(quv, rec, d, P)
    assert st == 0 and not (fell & 3).any()
    want = np.where((d[:, 2] < 0)[:, None], [0, 0, 1.0], [0, 0, -1.0]) + 0.0
    assert np.array_equal(np.abs(nrm), np.abs(want)) and np.array_equal(np.sign(nrm[:, 2]), np.sign(want[:, 2]))


def test_sphere_limit_on_the_host_build():
    """a level-2 icosphere on the unit sphere with normals = vertices: m = P in exact arithmetic, so the shading normal of a hit at P is
    unit_vector(P) to 1e-12 per component (about 30 f64 operations on values <= 1, |w| <= 1 / (edge^2 sin 60) ~ 13 for edges ~ 0.3)"""
    L = smooth_sim.load()
    v, f = SW.icosphere(2)
    assert len(f) == 320
    rng = np.random.default_rng(11)
    worst = 0.0
    for a_, b_, c_ in f:
        A, B, Cc = (np.array(v[i]) for i in (a_, b_, c_))
        quv = np.concatenate([A, B - A, Cc - A])
        kind, rec = L.prepare(np.concatenate([A, B, Cc])[None])
        assert kind[0] == SMM.SMOOTH
        al = rng.uniform(0, 1, 64); be = rng.uniform(0, 1, 64) * (1 - al)
        P = A + al[:, None] * (B - A) + be[:, None] * (Cc - A)
        d = -P + rng.uniform(-0.2, 0.2, P.shape)     # from outside, towards the centre
        st, nrm, fell = L.shade(quv, rec[0], d, P)
        assert st == 0 and not fell.any()
        worst = max(worst, float(np.abs(nrm - P / np.linalg.norm(P, axis=1, keepdims=True)).max()))
    print("sphere limit, host build: max |normal - unit(P)| =", worst)
    assert worst <= 1e-12


# ------------------------------------------------------------------ schema
def _loads(host, cfg):
    return host.Scene.loads(json.dumps(cfg))


def test_schema_normals_smooth_and_triangle_normals_load(host):
    v, f = SW.icosphere(1)
    sc = _loads(host, _cfg([SW.ico_mesh(1, (0.5, 0.2, 0.1), 2.0, _lam(0.5, 0.5, 0.5))]))
    n = sc.flat_normals()
    assert n.shape == (80, 9)
    for k, (a, b, c) in enumerate(f):
        assert list(n[k]) == list(v[a]) + list(v[b]) + list(v[c])      # as written, not normalised, in entry order
    tri = {"triangle": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "normals": [[0, 0, 2], [0, 1, 1], [1, 0, 1]], "material": _lam(0.5, 0.5, 0.5)}
    plain = {"triangle": [[0, 0, 1], [1, 0, 1], [0, 1, 1]], "material": _lam(0.5, 0.5, 0.5)}
    sc = _loads(host, _cfg([plain, tri]))
    assert sc.flat_normals().tolist() == [[0.0] * 9, [0, 0, 2, 0, 1, 1, 1, 0, 1]]
    assert _loads(host, _cfg([plain])).flat_normals() is None


def test_schema_smooth_equals_the_formula(host):
    v, f = SW.icosphere(1)
    verts = [[0.3 + 1.7 * p[0], -0.2 + 1.7 * p[1], 0.9 + 1.7 * p[2]] for p in v]
    mesh = {"mesh": {"vertices": verts, "faces": [list(t) for t in f], "smooth": True}, "material": _lam(0.5, 0.5, 0.5)}
    got = _loads(host, _cfg([mesh])).flat_normals()
    acc = [[0.0, 0.0, 0.0] for _ in verts]
    for a, b, c in f:    # in face order, component-wise, one add per face; u and v as the loader forms them
        u = [verts[b][k] - verts[a][k] for k in range(3)]; w = [verts[c][k] - verts[a][k] for k in range(3)]
        n = QM.cross(u, w)
        for i in (a, b, c):
            for k in range(3):
                acc[i][k] += n[k]
    want = np.array([acc[a] + acc[b] + acc[c] for a, b, c in f])
    assert np.array_equal(_bits(got), _bits(want))
    off = dict(mesh, mesh=dict(mesh["mesh"], smooth=False))
    assert _loads(host, _cfg([off])).flat_normals() is None


def test_schema_round_trip_bit_for_bit(host):
    cfg = _cfg(SW.box_triangles((-1, -1, -1), (0.3, 0.7, 1.1), _lam(0.4, 0.5, 0.6), True) + [SW.ico_mesh(1, (0.1, 0.2, 0.3), 0.7, _lam(0.5, 0.5, 0.5)),
               {"triangle": [[0, 0, 1], [1, 0, 1], [0, 1, 1]], "material": _lam(0.5, 0.5, 0.5)}])
    a = _loads(host, cfg)
    text = a.to_json()
    b = host.Scene.loads(text)
    assert bytes(a.quads()) == bytes(b.quads())
    assert np.array_equal(_bits(a.flat_normals()), _bits(b.flat_normals()))
    assert b.to_json() == text
    assert text.count('"normals"') == 12 + 80
    plain = _loads(host, SW.strip_normals(cfg))
    assert '"normals"' not in plain.to_json() and plain.flat_normals() is None


@pytest.mark.parametrize("obj,needle", [
    (SW.ico_mesh(1, (0, 0, 0), 1.0, {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}, normals=[[0, 0, 1]] * 3), "mesh.normals: expected 42 normals"),
    (SW.ico_mesh(1, (0, 0, 0), 1.0, {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}, smooth=True), "mixed keys"),
    (SW.ico_mesh(1, (0, 0, 0), 1.0, {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}, normals=[[0, 0, 1]] * 41 + [[0, 0, 0]]), "mesh normal 41"),
    (SW.ico_mesh(1, (0, 0, 0), 1.0, {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}, normals=[[0, 0, 1]] * 41 + [[0, "up", 0]]), "mesh normal 41"),
    ({"mesh": {"vertices": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "faces": [[0, 1, 2], [0, 2, 1]], "smooth": True}, "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}},
     "mesh vertex 0"),
    ({"mesh": {"vertices": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "faces": [[0, 1, 2]], "smooth": 1}, "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}},
     "mesh.smooth"),
    ({"triangle": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "normals": [[0, 0, 1]] * 2, "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}}, "triangle.normals: expected 3 normals"),
    ({"triangle": [[0, 0, 0], [1, 0, 0], [0, 1, 0]], "normals": [[0, 0, 1], [0, 0, 0], [0, 0, 1]], "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}}, "triangle normal 1"),
    ({"q": [0, 0, 0], "u": [1, 0, 0], "v": [0, 1, 0], "normals": [[0, 0, 1]] * 3, "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}}, "parallelogram takes no normals"),
    ({"box": {"min": [0, 0, 0], "max": [1, 1, 1]}, "normals": [[0, 0, 1]] * 3, "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}}, "a box takes no normals"),
])
def test_every_new_load_error_names_its_object(host, obj, needle):
    sphere = {"center": {"x": 0.0, "y": 5.0, "z": 0.0}, "radius": 0.5, "material": {"Lambertian": {"albedo": [0.5, 0.5, 0.5]}}}
    with pytest.raises(Exception) as e:
        _loads(host, _cfg([sphere, obj]))
    assert "objects[1]" in str(e.value) and needle in str(e.value), str(e.value)


# ------------------------------------------------------------------ the glass case's fallbacks, checked here for the GPU test
def test_glass_parity_camera_takes_both_fallbacks(abi, oracle, host):
    """the restatement's frame of the GPU test's smooth Glass icosphere takes the side-or-degenerate and the grazing fallback (> 0 each is
    what makes that frame a test of them); computed once per session, shared with tests/test_smooth_gpu.py"""
    import smooth_frames as SF
    m = SF.mini_frame(oracle, abi, host, "glass")
    print("glass: shaded", m["shaded"], "fell", m["fell"])
    assert m["shaded"] > 500 and m["fell"][SMM.FELL_GRAZING] > 0 and m["fell"][SMM.FELL_SIDE] > 0


def test_a_duplicate_normals_key_is_an_error_in_every_form(host):
    mat = '"material":{"Lambertian":{"albedo":[0.5,0.5,0.5]}}'
    nrm = '"normals":[[0,0,1],[0,0,1],[0,0,1]]'
    for obj in ('{"q":[0,0,0],"u":[1,0,0],"v":[0,1,0],"shape":"triangle",%s,%s,%s}' % (nrm, nrm, mat),
                '{"triangle":[[0,0,0],[1,0,0],[0,1,0]],%s,%s,%s}' % (nrm, nrm, mat),
                '{"mesh":{"vertices":[[0,0,0],[1,0,0],[0,1,0]],"faces":[[0,1,2]],%s,%s},%s}' % (nrm, nrm, mat)):
        text = json.dumps(_cfg([])).replace('"objects": []', '"objects": [%s]' % obj)
        with pytest.raises(Exception) as e:
            host.Scene.loads(text)
        assert "objects[0]" in str(e.value) and "duplicate field `normals`" in str(e.value), str(e.value)
