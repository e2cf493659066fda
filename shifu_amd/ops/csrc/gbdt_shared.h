// Device code shared by gbdt_kernels.hip (features of <= 256 bins) and gbdt_wide_kernels.hip
// (257 .. 16384 bins): the packed fixed-point histogram entry, the impurity gains and the
// quad-blocked bins addressing.  Both files must quantise, unpack and score identically so that
// narrow and wide split candidates share units.
#pragma once
#include "common.h"

constexpr int QF = 128;        // features per row record (one 128-B line); 4 groups per record
constexpr int PACK_G = 36;     // low field bits (signed qg) of a packed (qw << 36) + qg entry

// byte offset of feature f of data row `row` in the quad-blocked layout (qs = N * 128)
__device__ __forceinline__ size_t bin_off(long qs, long row, int f) {
  return (size_t)(f >> 7) * qs + (size_t)row * QF + (f & (QF - 1));
}

__device__ __forceinline__ void unpack_add(unsigned long long v, long long& aw, long long& ag) {
  const long long gq = ((long long)(v << (64 - PACK_G))) >> (64 - PACK_G);
  ag += gq;
  aw += (long long)((v - (unsigned long long)gq) >> PACK_G);
}

enum Imp : int { IMP_VARIANCE = 0, IMP_FRIEDMAN = 1, IMP_ENTROPY = 2, IMP_GINI = 3 };

__device__ __forceinline__ double imp_gain(int imp, double lw, double ls, double rw, double rs) {
  const double c = lw + rw, s = ls + rs;
  switch (imp) {
    case IMP_FRIEDMAN: { const double d = rw * ls - lw * rs; return d * d / (lw * rw * c); }
    case IMP_ENTROPY: {
      auto ent = [](double n, double p1) {   // binary classes: p1 = weight of class 1
        if (n <= 0.0) return 0.0;
        double r1 = p1 / n, r0 = 1.0 - r1, e = 0.0;
        if (r1 > 0.0) e -= r1 * log2(r1);
        if (r0 > 0.0) e -= r0 * log2(r0);
        return e;
      };
      return ent(c, s) - (lw / c) * ent(lw, ls) - (rw / c) * ent(rw, rs);
    }
    case IMP_GINI: {
      auto gin = [](double n, double p1) {
        if (n <= 0.0) return 0.0;
        double r1 = p1 / n, r0 = 1.0 - r1;
        return -(r1 * r1 + r0 * r0);
      };
      return gin(c, s) - (lw / c) * gin(lw, ls) - (rw / c) * gin(rw, rs);
    }
    default:   // variance: (sL^2/cL + sR^2/cR - s^2/c) / c  (sum-of-squares terms cancel)
      return (ls * ls / lw + rs * rs / rw - s * s / c) / c;
  }
}
