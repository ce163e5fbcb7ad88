"""TEST INFRASTRUCTURE: a numpy restatement of the temporal reprojection step of include/rt_abi.h (rt_hip_reproject).

Written from the header's description alone: every operation is one IEEE numpy operation (numpy never fuses a*b+c) — float64 up to
the tap positions, float32 from the weights on — in the order the header gives, so the GPU kernel and the CPU build of rt_core.h's
reproject_pixel must match it bit for bit."""
import numpy as np

F = np.float32
D = np.float64


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], -1)


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def positions(aov, cam, prev_cam):
    """where each pixel's surface was in the previous frame: (fx, fy, a, hit, ok) with ok = the pixel may have history"""
    h, w, _ = aov.shape
    cam, prev_cam = np.asarray(cam, D), np.asarray(prev_cam, D)
    org, ll, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    porg, pll, phor, pver = prev_cam[0:3], prev_cam[3:6], prev_cam[6:9], prev_cam[9:12]
    ys, xs = np.meshgrid(np.arange(h, dtype=D), np.arange(w, dtype=D), indexing="ij")
    with np.errstate(all="ignore"):
        u = (xs + D(0.5)) / D(w - 1)
        v = (D(h) - (ys + D(0.5))) / D(h - 1)
        d = ((ll + hor * u[..., None]) + ver * v[..., None]) - org
        cov, iz = aov[..., 7], aov[..., 3]
        hit = (cov > F(0.0)) & (iz > F(0.0))
        t = cov.astype(D) / iz.astype(D)
        q = np.where(hit[..., None], (org + d * t[..., None]) - porg, d)
        A = pll - porg
        n0, n1, n2 = _cross(phor, pver), _cross(pver, A), _cross(A, phor)
        det = _dot(A, n0)
        a, b, e = _dot(q, n0) / det, _dot(q, n1) / det, _dot(q, n2) / det
        ok = (a > 0.0) & np.isfinite(a) & np.isfinite(b) & np.isfinite(e)
        fx = (b / a) * D(w - 1) - D(0.5)
        fy = (D(h) - (e / a) * D(h - 1)) - D(0.5)
        ok &= (fx >= -1.0) & (fx < D(w)) & (fy >= -1.0) & (fy < D(h))
    return fx, fy, a, hit, ok


def reproject(lin, aov, prev_hist, prev_aov, cam, prev_cam, alpha_min, n_max, tau_n, tau_a, tau_z):
    """lin [h, w, 3], aov / prev_aov [h, w, 8], prev_hist [h, w, 4] float32; cameras 12 doubles -> the new history [h, w, 4] float32"""
    lin, aov = np.ascontiguousarray(lin, F), np.ascontiguousarray(aov, F)
    prev_hist, prev_aov = np.ascontiguousarray(prev_hist, F), np.ascontiguousarray(prev_aov, F)
    h, w, _ = lin.shape
    alpha_min, n_max, tau_n, tau_a, tau_z = F(alpha_min), F(n_max), F(tau_n), F(tau_a), F(tau_z)
    fx, fy, a, hit, ok = positions(aov, cam, prev_cam)
    with np.errstate(all="ignore"):
        fx, fy = np.where(ok, fx, 0.0), np.where(ok, fy, 0.0)
        x0d, y0d = np.floor(fx), np.floor(fy)
        x0, y0 = x0d.astype(np.int64), y0d.astype(np.int64)
        wx, wy = (fx - x0d).astype(F), (fy - y0d).astype(F)
        ez = np.where(hit, (aov[..., 7].astype(D) / a).astype(F), F(0.0)).astype(F)
        lim = tau_z * ez
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
                H, g = prev_hist[qyc, qxc], prev_aov[qyc, qxc]
                use = ok & inside & (H[..., 3] > F(0.0)) & ~np.isnan(H[..., 0:3]).any(-1)
                use &= _sq3(g[..., 4:7] - aov[..., 4:7]) <= tau_n
                use &= _sq3(g[..., 0:3] - aov[..., 0:3]) <= tau_a
                dz = g[..., 3] - ez
                use &= dz * dz <= lim2
                wt = (wx if i else F(1.0) - wx) * wj
                for c in range(3):
                    s[c] = np.where(use, s[c] + wt * H[..., c], s[c])
                sw = np.where(use, sw + wt, sw)
                sn = np.where(use, sn + wt * H[..., 3], sn)
        have = sw > F(0.0)
        m = sn / sw + F(1.0)
        n = np.where(m < n_max, m, n_max).astype(F)
        r = F(1.0) / n
        alpha = np.where(alpha_min > r, alpha_min, r).astype(F)
        out = np.zeros((h, w, 4), F)
        for c in range(3):
            hist = s[c] / sw
            out[..., c] = np.where(have, hist + alpha * (lin[..., c] - hist), lin[..., c])
        out[..., 3] = np.where(have, n, F(1.0))
    nan_px = np.isnan(lin).any(-1)
    out[nan_px, 0:3] = lin[nan_px]
    out[nan_px, 3] = F(0.0)
    return out
