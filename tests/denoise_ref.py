"""TEST INFRASTRUCTURE: a numpy restatement of the denoising arithmetic of include/rt_abi.h (rt_hip_denoise).

Written from the header's description alone: every operation is one IEEE float32 numpy operation (numpy never fuses a*b+c), in the
order the header gives, so the GPU kernel and the CPU build of rt_core.h must match it bit for bit."""
import numpy as np

F = np.float32
FLT_MAX = F(3.4028234663852886e38)
H = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
SIXTH = F(1.0 / 6.0)


def consts(i, sigmas):
    """(k_c, k_n, k_a, k_z) of iteration i"""
    def k(num, s):
        s = F(s)
        with np.errstate(all="ignore"):
            v = F(num) / (s * s)
        return min(v, FLT_MAX)
    sc, sn, sa, sz = sigmas
    return k(4.0 ** i, sc), k(1.0, sn), k(1.0, sa), k(1.0, sz)


def weight(x):
    """W(x) = 1 / (1 + x (1 + x (1/2 + x (1/6 + x / 24))))"""
    with np.errstate(all="ignore"):
        return F(1.0) / (F(1.0) + x * (F(1.0) + x * (F(0.5) + x * (SIXTH + x / F(24.0)))))


def iteration(col, aov, i, sigmas):
    """one pass: col [h, w, 3] float32, aov [h, w, 8] float32 -> [h, w, 3] float32"""
    h, w, _ = col.shape
    kc, kn, ka, kz = consts(i, sigmas)
    step = 1 << i
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sr = np.zeros((h, w), F); sg = np.zeros((h, w), F); sb = np.zeros((h, w), F); sw = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for j in range(5):
            qy = ys + (j - 2) * step
            for k in range(5):
                qx = xs + (k - 2) * step
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qyc, qxc = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                c, g = col[qyc, qxc], aov[qyc, qxc]
                d = c - col
                dc2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                dn = g[..., 4:7] - aov[..., 4:7]
                dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                da = g[..., 0:3] - aov[..., 0:3]
                da2 = (da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2]
                dz = g[..., 3] - aov[..., 3]
                x = ((dc2 * kc + dn2 * kn) + da2 * ka) + (dz * dz) * kz
                wt = (H[k] * H[j]) * weight(x)
                use = inside & (wt > F(0.0))
                sr = np.where(use, sr + wt * c[..., 0], sr)
                sg = np.where(use, sg + wt * c[..., 1], sg)
                sb = np.where(use, sb + wt * c[..., 2], sb)
                sw = np.where(use, sw + wt, sw)
        out = np.stack([sr / sw, sg / sw, sb / sw], -1).astype(F)
    nan_px = np.isnan(col).any(-1)
    out[nan_px] = col[nan_px]
    return out


def denoise(lin, aov, iterations, sigmas):
    """the filter's L iterations; lin [h, w, 3], aov [h, w, 8] -> linear [h, w, 3] float32"""
    col = np.ascontiguousarray(lin, F).copy()
    aov = np.ascontiguousarray(aov, F)
    for i in range(iterations):
        col = iteration(col, aov, i, sigmas)
    return col


def to_rgb8(lin):
    """f32_to_u8(sqrt(x)): round-half-even of min(255 sqrt(x), 255), NaN -> 255, <= 0 -> 0 (rt_hip_resolve's bytes)"""
    with np.errstate(all="ignore"):
        s = np.sqrt(lin.astype(F)) * F(255.0)
        out = np.rint(np.minimum(np.where(s > F(0.0), s, F(0.0)), F(255.0)))
    out = np.where(np.isnan(s), F(255.0), out)
    return out.astype(np.uint8)
