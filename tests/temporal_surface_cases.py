"""TEST INFRASTRUCTURE: crafted surface records and parameter sets for the tests of temporal denoising with surface tracking
(tests/test_temporal_surface_cpu.py on the CPU build of reproject_surface_pixel, tests/test_temporal_surface_gpu.py on
rt_hip_reproject_surface), each compared with tests/temporal_surface_ref.py bit for bit.  The colours, guides and histories are
temporal_cases.crafted's."""
import numpy as np

import temporal_surface_ref as R

N_IDS = 40   # ids of the crafted records: below every test scene's sphere count, so a displacement table row exists for each


def crafted_surface(rng, aov, h, w):
    """(surf, prev_surf) to go with temporal_cases.crafted's aov: ids and kinds constant over the same 4 x 4 blocks, every RT_MAT_* kind,
    sky where the guides have no coverage; the previous frame has blocks of another id, sky where this frame has a surface and a
    surface where it has sky, and depths t' off by 0, 1 % and 30 % in both directions (both sides of a 5 % depth limit)"""
    by, bx = (np.arange(h) // 4)[:, None], (np.arange(w) // 4)[None, :]
    nb = (h // 4 + 1, w // 4 + 1)
    id_b = rng.integers(0, N_IDS, nb)
    kind_b = rng.integers(0, 8, nb)
    surf = np.zeros((h, w), R.SURF)
    sky = aov[..., 7] == 0
    surf["id"], surf["kind"] = id_b[by, bx], kind_b[by, bx]
    with np.errstate(all="ignore"):
        surf["t"] = np.where(sky, 0.0, aov[..., 7].astype(np.float64) / aov[..., 3].astype(np.float64))
    surf["id"][sky] = surf["kind"][sky] = R.NONE
    prev = surf.copy()
    other = (rng.random(nb) < 0.2)[by, bx]                      # another sphere stood there
    prev["id"][other & ~sky] = (prev["id"][other & ~sky] + 1) % N_IDS
    to_sky = (rng.random(nb) < 0.1)[by, bx] & ~sky              # a surface now, sky then
    prev["id"][to_sky] = prev["kind"][to_sky] = R.NONE
    prev["t"][to_sky] = 0.0
    from_sky = (rng.random(nb) < 0.3)[by, bx] & sky             # sky now, a surface then
    prev["id"][from_sky], prev["kind"][from_sky], prev["t"][from_sky] = 3, 0, 9.0
    off = rng.choice([0.0, 0.01, -0.01, 0.3, -0.3], (h, w))
    prev["t"] = np.where(prev["id"] != R.NONE, prev["t"] * (1.0 + off), 0.0)
    return surf, prev


def displacements(rng):
    """name -> None or [N_IDS, 3]"""
    return {"null": None, "zero": np.zeros((N_IDS, 3)), "moved": 0.6 * (rng.random((N_IDS, 3)) - 0.5)}


# alpha_min, alpha_specular, n_max, tau_n, tau_a, tau_z: both alphas 0 and 1, thresholds 0 and huge, a 5 % depth limit, n_max small and unbounded
PARAMS = [(0.0, 0.0, 1e30, 1e30, 1e30, 1e30), (0.0, 1.0, 1e30, 1e30, 1e30, 1e30), (1.0, 0.0, 4.0, 1e30, 1e30, 1e30), (0.2, 1.0, 3.0, 0.5, 0.5, 0.05),
          (0.0, 0.0, float("inf"), 0.0, 0.0, 0.0), (0.1, 0.6, 32.0, 0.001, 0.001, 0.05)]
