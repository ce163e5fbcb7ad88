/*
 * rt_neg_log.h — ONE -ln(x) for the kernel (the free-flight distance of a participating medium, rt_core.h medium_hit,
 * DESIGN.md §15) and for every restatement of it (tests/medium_mini.py), so that media are bit-identical everywhere.
 *
 * What is the contract is the BITS, not the accuracy: the routine is a fixed sequence of IEEE f64 operations (+, -, *, /; no fused
 * operation, no contraction, no library call) around an exact split of the argument into exponent and mantissa, so a restatement
 * in any language with IEEE doubles reproduces it.  Measured against correctly rounded values (tests/golden/neg_log_cr.npz: 27 372
 * arguments 1 - k 2^-53, either side of the sqrt 2 switch, powers of two, subnormals; tests/test_medium_cpu.py): within 1 ulp (0.758).
 *
 * The steps, in this order (x finite and > 0; the scheme is the classical one of argument reduction to [sqrt(1/2), sqrt(2))):
 *   1. bits = the 64 bits of x; a subnormal x is first multiplied by 2^54 (exact) and 54 is taken off the exponent below.
 *   2. k = (bits >> 52) - 1023; mant = bits & (2^52 - 1).
 *      mant >= 0x6A09E667F3BCD (the mantissa of sqrt 2):  m = the double with exponent field 1022 and mantissa mant, k = k + 1;
 *      else:                                              m = the double with exponent field 1023 and mantissa mant.
 *      Now x = m 2^k exactly with m in [sqrt(1/2), sqrt(2)).
 *   3. f = m - 1.0                      (exact)
 *      s = f / (2.0 + f)
 *      z = s * s;  w = z * z
 *      t1 = w * (L2 + w * (L4 + w * L6))
 *      t2 = z * (L1 + w * (L3 + w * (L5 + w * L7)))
 *      R = t2 + t1
 *      hfsq = (0.5 * f) * f
 *      dk = (double)k                   (exact)
 *      result = ((hfsq - (s * (hfsq + R) + dk * LN2_LO)) - f) - dk * LN2_HI
 *    (ln(1 + f) = f - hfsq + s (hfsq + R) with R ~ the tail of 2 atanh(s) - 2 s; LN2_HI has 21 trailing zero bits, so dk * LN2_HI
 *     is exact.)  At x = 1.0: f = s = R = hfsq = dk = 0 and the result is (0 - 0) - 0 = +0.0 exactly.
 * x = 0 gives +inf, x < 0 and NaN give NaN, +inf gives -inf.
 *
 * Plain C; RT_NEG_LOG_FN may be predefined (e.g. `__host__ __device__ inline`).
 */
#ifndef RT_NEG_LOG_H
#define RT_NEG_LOG_H

#include <stdint.h>

#ifndef RT_NEG_LOG_FN
#define RT_NEG_LOG_FN static inline
#endif

#define RT_NL_LN2_HI 6.93147180369123816490e-01 /* 0x3FE62E42FEE00000 */
#define RT_NL_LN2_LO 1.90821492927058770002e-10 /* 0x3DEA39EF35793C76 */
#define RT_NL_L1 6.666666666666735130e-01
#define RT_NL_L2 3.999999999940941908e-01
#define RT_NL_L3 2.857142874366239149e-01
#define RT_NL_L4 2.222219843214978396e-01
#define RT_NL_L5 1.818357216161805012e-01
#define RT_NL_L6 1.531383769920937332e-01
#define RT_NL_L7 1.479819860511658591e-01

RT_NEG_LOG_FN double rt_neg_log(double x) {
  uint64_t bits;
  int64_t k = 0;
  __builtin_memcpy(&bits, &x, 8);
  if ((bits >> 52) == 0u || (bits >> 52) >= 0x7FFu) { /* zero, subnormal, negative, infinite, NaN */
    if ((bits << 1) == 0u) return __builtin_inf();
    if ((bits >> 63) != 0u || x != x) return __builtin_nan("");
    if ((bits >> 52) == 0x7FFu) return -__builtin_inf();
    x = x * 18014398509481984.0; /* 2^54, exact */
    k = -54;
    __builtin_memcpy(&bits, &x, 8);
  }
  k += (int64_t)(bits >> 52) - 1023;
  {
    const uint64_t mant = bits & 0x000FFFFFFFFFFFFFull;
    uint64_t mb;
    double m, f, s, z, w, t1, t2, R, hfsq, dk;
    if (mant >= 0x6A09E667F3BCDull) { mb = (1022ull << 52) | mant; k += 1; }
    else mb = (1023ull << 52) | mant;
    __builtin_memcpy(&m, &mb, 8);
    f = m - 1.0;
    s = f / (2.0 + f);
    z = s * s;
    w = z * z;
    t1 = w * (RT_NL_L2 + w * (RT_NL_L4 + w * RT_NL_L6));
    t2 = z * (RT_NL_L1 + w * (RT_NL_L3 + w * (RT_NL_L5 + w * RT_NL_L7)));
    R = t2 + t1;
    hfsq = (0.5 * f) * f;
    dk = (double)k;
    return ((hfsq - (s * (hfsq + R) + dk * RT_NL_LN2_LO)) - f) - dk * RT_NL_LN2_HI;
  }
}

#endif
