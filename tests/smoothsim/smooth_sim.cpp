// tests/smoothsim/smooth_sim.cpp — the host build of csrc/common/rt_flat_normal.h behind a C interface for
// tests/smooth_sim.py: g++ with -ffp-contract=off, the bits tests/smooth_mini.py restates and the device must give.
#include "../../rust-raytracer_amd/csrc/common/rt_flat_normal.h"

extern "C" {

// rt_flat_normal_prepare of n entries: kind[k] and the 72-byte record (nine zeros for a refused entry)
void smooth_prepare_v(const double* in, uint64_t n, int32_t* kind, double* rec) {
  for (uint64_t k = 0; k < n; ++k) {
    double out[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    kind[k] = rt_flat_normal_prepare(in + 9 * k, out);
    for (int c = 0; c < 9; ++c) rec[9 * k + c] = kind[k] == RT_FLAT_NORMAL_BAD ? 0.0 : out[c];
  }
}

// rt_flat_normal_shade of n hits on ONE entry (quv through rt_quad_prepare; rec: its PREPARED normals): per hit d (3) and P (3) ->
// the normal and the fallbacks taken.  Returns rt_quad_prepare's status.
int smooth_shade_v(const double* quv, const double* rec, const double* d, const double* P, uint64_t n, double* normal, int32_t* fell) {
  RtQuadRec r;
  const int st = rt_quad_prepare(quv, quv + 3, quv + 6, &r);
  if (st) return st;
  for (uint64_t i = 0; i < n; ++i) fell[i] = rt_flat_normal_shade(r, rec, d + 3 * i, P + 3 * i, normal + 3 * i);
  return 0;
}

// the same with one entry PER hit (quv n x 9, rec n x 9); status[i]: rt_quad_prepare's
void smooth_shade_each(const double* quv, const double* rec, const double* d, const double* P, uint64_t n, double* normal, int32_t* fell, int32_t* status) {
  for (uint64_t i = 0; i < n; ++i) {
    RtQuadRec r;
    status[i] = rt_quad_prepare(quv + 9 * i, quv + 9 * i + 3, quv + 9 * i + 6, &r);
    fell[i] = status[i] ? -1 : rt_flat_normal_shade(r, rec + 9 * i, d + 3 * i, P + 3 * i, normal + 3 * i);
  }
}

// y / sqrt(y * y), as the contract divides (the axis-aligned identity's premise)
double smooth_unit_1d(double y) { return y / sqrt(y * y); }

}
