// anim_path.h — where `raytracer ... --frames N --shutter S` puts the spheres of frame f.  With the flag a sphere's
// center -> center1 is its path over the WHOLE animation: with dv = center1 - center in f64, frame f is exposed from
//   center_f = center + dv * ((double)f / N)   to   center1_f = center + dv * (((double)f + S) / N),
// evaluated in exactly this form (IEEE f64, no contraction), S in [0, 1] the part of a frame's interval the shutter is open.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../../include/rt_abi.h"

// center1: n x 3 (rt_scene_motion) or NULL (no sphere moves); c_out, c1_out: n x 3 each
inline void rt_anim_centres(const RtSphere* spheres, const double* center1, uint32_t n, int f, int N, double S, double* c_out, double* c1_out) {
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      const double c = spheres[i].center[k];
      const double dv = (center1 ? center1[3 * (size_t)i + k] : c) - c;
      c_out[3 * (size_t)i + k] = c + dv * ((double)f / N);
      c1_out[3 * (size_t)i + k] = c + dv * (((double)f + S) / N);
    }
}
