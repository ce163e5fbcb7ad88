"""TEST INFRASTRUCTURE: a numpy restatement of the two contracts of temporal denoising with surface tracking (include/rt_abi.h
rt_hip_render_surface and rt_hip_reproject_surface).

Written from the header's description: every operation is one IEEE numpy operation (numpy never fuses a*b+c) in the order the header
gives — float64 for the geometry and the depth test, float32 from the weights on — so the GPU kernels and the CPU builds of rt_core.h's
surface_pixel and reproject_surface_pixel must match it bit for bit.  The surface record's hit is the brute force of hit_world over all
spheres in scene order with Sphere::hit's own arithmetic (sphere.rs:47-58), no grid."""
import numpy as np

from temporal_ref import _cross, _dot, _sq3

F = np.float32
D = np.float64
NONE = 0xFFFFFFFF
SURF = np.dtype([("id", "<u4"), ("kind", "<u4"), ("t", "<f8")])   # the 16-byte record
MAT_METAL, MAT_GLASS = 1, 2


def centre_rays(cam, h, w):
    """the pixel-centre pinhole rays of the 12-double camera: d [h, w, 3]"""
    cam = np.asarray(cam, D)
    org, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    ys, xs = np.meshgrid(np.arange(h, dtype=D), np.arange(w, dtype=D), indexing="ij")
    with np.errstate(all="ignore"):
        u = (xs + D(0.5)) / D(w - 1)
        v = (D(h) - (ys + D(0.5))) / D(h - 1)
        return ((ll + hor * u[..., None]) + ver * v[..., None]) - org


def mid_centres(center, center1=None):
    """each sphere's centre at shutter time 0.5: c + (c1 - c) * 0.5 in float64"""
    c = np.asarray(center, D).reshape(-1, 3)
    if center1 is None:
        return c.copy()
    return c + (np.asarray(center1, D).reshape(-1, 3) - c) * D(0.5)


def surface(centres, radii, kinds, cam, h, w, t_min=0.001):
    """the surface record [h, w] (dtype SURF) of spheres with centres [n, 3], radii [n] and RT_MAT_* kinds [n] (no media): hit_world's scan in
    scene order, a sphere accepted iff its first root in (t_min, closest so far) exists — strict '<', so the earlier sphere wins a tie"""
    centres, radii = np.asarray(centres, D).reshape(-1, 3), np.asarray(radii, D)
    org = np.asarray(cam, D)[0:3]
    d = centre_rays(cam, h, w)
    closest = np.full((h, w), np.finfo(D).max)
    best = np.full((h, w), -1, np.int64)
    with np.errstate(all="ignore"):
        a = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for i in range(len(radii)):
            oc = org - centres[i]
            half_b = (oc[0] * d[..., 0] + oc[1] * d[..., 1]) + oc[2] * d[..., 2]
            c = ((oc[0] * oc[0] + oc[1] * oc[1]) + oc[2] * oc[2]) - radii[i] * radii[i]
            disc = (half_b * half_b) - (a * c)
            sq = np.sqrt(np.where(disc >= 0.0, disc, 0.0))
            root_a, root_b = ((-half_b) - sq) / a, ((-half_b) + sq) / a
            ok_a = (disc >= 0.0) & (root_a < closest) & (root_a > t_min)
            ok_b = (disc >= 0.0) & (root_b < closest) & (root_b > t_min)
            root = np.where(ok_a, root_a, root_b)
            hit = ok_a | ok_b
            closest = np.where(hit, root, closest)
            best = np.where(hit, i, best)
    out = np.zeros((h, w), SURF)
    hit = best >= 0
    out["id"] = np.where(hit, best, NONE).astype(np.uint32)
    out["kind"] = np.where(hit, np.asarray(kinds, np.int64)[np.clip(best, 0, None)], NONE).astype(np.uint32)
    out["t"] = np.where(hit, closest, 0.0)
    return out


def surface_all_at_once(centres, radii, kinds, cam, h, w, t_min=0.001):
    """surface() for scenes of very many spheres, a row of pixels against all spheres at a time.  A far root is never below the near one, so
    the scan accepts sphere i iff its first root above t_min, f_i, is below the closest so far: the answer is the smallest f_i, the earliest
    sphere among equals — numpy's argmin.  Same operations per sphere, same bits (tests/test_temporal_surface_cpu.py holds the two together)."""
    centres, radii = np.asarray(centres, D).reshape(-1, 3), np.asarray(radii, D)
    org = np.asarray(cam, D)[0:3]
    d = centre_rays(cam, h, w)
    out = np.zeros((h, w), SURF)
    oc = org - centres                                                                  # [n, 3]
    c = ((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - radii * radii
    kinds = np.asarray(kinds, np.int64)
    with np.errstate(all="ignore"):
        for y in range(h):
            dy = d[y][:, None, :]                                                       # [w, 1, 3]
            a = (dy[..., 0] * dy[..., 0] + dy[..., 1] * dy[..., 1]) + dy[..., 2] * dy[..., 2]
            half_b = (oc[:, 0] * dy[..., 0] + oc[:, 1] * dy[..., 1]) + oc[:, 2] * dy[..., 2]     # [w, n]
            disc = (half_b * half_b) - (a * c)
            sq = np.sqrt(np.where(disc >= 0.0, disc, 0.0))
            root_a, root_b = ((-half_b) - sq) / a, ((-half_b) + sq) / a
            f = np.where(root_a > t_min, root_a, np.where(root_b > t_min, root_b, np.inf))
            f = np.where((disc >= 0.0) & (f < np.finfo(D).max), f, np.inf)
            best = np.argmin(f, axis=1)
            t = f[np.arange(w), best]
            hit = np.isfinite(t)
            out["id"][y] = np.where(hit, best, NONE).astype(np.uint32)
            out["kind"][y] = np.where(hit, kinds[best], NONE).astype(np.uint32)
            out["t"][y] = np.where(hit, t, 0.0)
    return out


def scene_surface(sc, cam=None, center=None, center1=None):
    """surface() of a loaded host scene (tests' load_scene) with its own camera, or `cam`; center / center1: moved spheres"""
    n = sc.c.n_spheres
    c0 = np.array([[sc.c.spheres[i].center[k] for k in range(3)] for i in range(n)], D) if center is None else np.asarray(center, D).reshape(-1, 3)
    radii = np.array([sc.c.spheres[i].radius for i in range(n)], D)
    kinds = np.array([sc.c.spheres[i].kind for i in range(n)])
    if cam is None:
        cam = np.array(list(sc.c.cam_origin) + list(sc.c.cam_lower_left) + list(sc.c.cam_horizontal) + list(sc.c.cam_vertical), D)
    fn = surface_all_at_once if n > 4096 else surface
    return fn(mid_centres(c0, center1), radii, kinds, cam, sc.c.height, sc.c.width)


def positions(surf, cam, prev_cam, disp=None):
    """where each pixel's surface point was in the previous frame: (fx, fy, a, hit, ok)"""
    h, w = surf.shape
    cam, prev_cam = np.asarray(cam, D), np.asarray(prev_cam, D)
    org = cam[0:3]
    porg, pll, phor, pver = prev_cam[0:3], prev_cam[3:6], prev_cam[6:9], prev_cam[9:12]
    d = centre_rays(cam, h, w)
    hit = surf["id"] != NONE
    with np.errstate(all="ignore"):
        point = org + d * surf["t"][..., None]
        if disp is not None:
            disp = np.asarray(disp, D).reshape(-1, 3)
            known = hit & (surf["id"] < len(disp))
            Dv = disp[np.where(known, surf["id"], 0)]
            point = np.where(known[..., None], point - Dv, point)
        q = np.where(hit[..., None], point - porg, d)
        A = pll - porg
        n0, n1, n2 = _cross(phor, pver), _cross(pver, A), _cross(A, phor)
        det = _dot(A, n0)
        a, b, e = _dot(q, n0) / det, _dot(q, n1) / det, _dot(q, n2) / det
        ok = (a > 0.0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(e)
        fx = (b / a) * D(w - 1) - D(0.5)
        fy = (D(h) - (e / a) * D(h - 1)) - D(0.5)
        ok &= (fx >= -1.0) & (fx < D(w)) & (fy >= -1.0) & (fy < D(h))
    return fx, fy, a, hit, ok


def taps(surf, prev_surf, cam, prev_cam, disp=None):
    """per pixel: ok, and for the four taps (j outer, i inner) whether the tap lies inside the frame on a previous record of the same id"""
    h, w = surf.shape
    fx, fy, a, hit, ok = positions(surf, cam, prev_cam, disp)
    x0 = np.floor(np.where(ok, fx, 0.0)).astype(np.int64)
    y0 = np.floor(np.where(ok, fy, 0.0)).astype(np.int64)
    same = []
    for j in range(2):
        for i in range(2):
            qy, qx = y0 + j, x0 + i
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            same.append(ok & inside & (prev_surf["id"][np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)] == surf["id"]))
    return ok, same


def reproject(lin, aov, surf, prev_hist, prev_aov, prev_surf, cam, prev_cam, disp, alpha_min, alpha_specular, n_max, tau_n, tau_a, tau_z):
    """lin [h, w, 3], aov / prev_aov [h, w, 8], prev_hist [h, w, 4] float32; surf / prev_surf [h, w] SURF; cameras 12 doubles; disp None or
    [n, 3] float64 -> the new history [h, w, 4] float32"""
    lin, aov = np.ascontiguousarray(lin, F), np.ascontiguousarray(aov, F)
    prev_hist, prev_aov = np.ascontiguousarray(prev_hist, F), np.ascontiguousarray(prev_aov, F)
    h, w, _ = lin.shape
    alpha_min, alpha_specular, n_max, tau_n, tau_a = F(alpha_min), F(alpha_specular), F(n_max), F(tau_n), F(tau_a)
    tau_z = D(F(tau_z))
    fx, fy, a, hit, ok = positions(surf, cam, prev_cam, disp)
    with np.errstate(all="ignore"):
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        x0d, y0d = np.floor(fx), np.floor(fy)
        x0, y0 = x0d.astype(np.int64), y0d.astype(np.int64)
        wx, wy = (fx - x0d).astype(F), (fy - y0d).astype(F)
        lim = tau_z * a
        lim2 = lim * lim
        s = [np.zeros((h, w), F) for _ in range(3)]
        sw, sn = np.zeros((h, w), F), np.zeros((h, w), F)
        for j in range(2):
            qy = y0 + j
            wj = wy if j else F(1.0) - wy
            for i in range(2):
                qx = x0 + i
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qyc, qxc = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                H, g, sp = prev_hist[qyc, qxc], prev_aov[qyc, qxc], prev_surf[qyc, qxc]
                use = ok & inside & (H[..., 3] > F(0.0)) & ~np.isnan(H[..., 0:3]).any(-1)
                use &= sp["id"] == surf["id"]
                use &= _sq3(g[..., 4:7] - aov[..., 4:7]) <= tau_n
                use &= _sq3(g[..., 0:3] - aov[..., 0:3]) <= tau_a
                dt = sp["t"] - a
                use &= ~hit | (dt * dt <= lim2)
                wt = (wx if i else F(1.0) - wx) * wj
                for c in range(3):
                    s[c] = np.where(use, s[c] + wt * H[..., c], s[c])
                sw = np.where(use, sw + wt, sw)
                sn = np.where(use, sn + wt * H[..., 3], sn)
        have = sw > F(0.0)
        m = sn / sw + F(1.0)
        n = np.where(m < n_max, m, n_max).astype(F)
        r = F(1.0) / n
        specular = (surf["kind"] == MAT_METAL) | (surf["kind"] == MAT_GLASS)
        floor = np.where(specular, alpha_specular, alpha_min).astype(F)
        alpha = np.where(floor > r, floor, r).astype(F)
        out = np.zeros((h, w, 4), F)
        for c in range(3):
            hist = s[c] / sw
            out[..., c] = np.where(have, hist + alpha * (lin[..., c] - hist), lin[..., c])
        out[..., 3] = np.where(have, n, F(1.0))
    nan_px = np.isnan(lin).any(-1)
    out[nan_px, 0:3] = lin[nan_px]
    out[nan_px, 3] = F(0.0)
    return out
