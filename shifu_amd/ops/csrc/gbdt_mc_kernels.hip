// Native multi-class RF (Entropy / Gini over C > 2 classes, Impurity.java:368-734) for MI355X
// (gfx950): ONE histogram pass per level for all classes and one split kernel, instead of C runs
// of the binary packed kernels with a one-hot target and a split search in torch.
//
//   * gbdt_hist_mc_kernel    a work item = (node, row range, FI features of one 128-B record).  The
//                            bin axis is keyed by the class: LDS [key = cls * nbp + bin][FI] of
//                            u64, one ds_add_u64 of q = rn(w * scale_g) per (row, feature).  q is
//                            what the binary kernel adds to its sum w*g plane for a one-hot
//                            target, so the int64 sums are the C-pass path's bit for bit.  Nothing
//                            is packed (q < 2^23 times any int32 row count stays inside 64 bits),
//                            so there is no periodic unpack and no barrier in the row loop; the
//                            LDS image is the item's slab, streamed out with 16-B stores.
//                            FI = 32, 16, 8 or 4: the most features whose C * nbp keys fit 128 KiB.
//                            A thread owns min(FI, 16) bytes of a row and rotates them by its lane
//                            (as gbdt_hist_kernel) so the lanes of an LDS group always update
//                            distinct features = distinct bank pairs whatever the keys are.  The
//                            sub-items of one record are consecutive items: one XCD (xcd_remap),
//                            every fetched line is consumed from that XCD's L2.
//   * gbdt_reduce_mc_kernel  sums a built node's item slabs in item order and transposes them
//                            through LDS into hist[node][C][F][256] (the all-reduced tensor).
//   * gbdt_split_mc_kernel   one block per (node, feature), one thread per bin: class sums (built)
//                            or parent - sibling (derived, written back), categorical order by
//                            counting ranks, per-class int64 prefix (wave scan + carry), fp64 gain.
//   * gbdt_choose_mc_kernel  one wave per node: the lowest feature with the largest gain.
#include "common.h"
#include "gbdt_shared.h"
#include <type_traits>

namespace {

constexpr int NB = 256;             // bins of a feature in hist / order (uint8 codes)
constexpr int MT = 512;             // threads per histogram block (8 waves)
constexpr int MC_LDS = 128 * 1024;  // LDS of one histogram item
constexpr int MC_KEYS = 4096;       // most class-keyed bins (C * nbp)
constexpr int NCAND = 10;           // doubles per split candidate / chosen split

struct McHistArgs {
  const uint8_t* bins; long gs;      // quad-blocked bins [Q][N][128]: gs = N * 128
  const int* pos2row;                // [P] position -> (virtual) row id; nullptr: identity (root)
  const float* w;                    // per (virtual) row weight
  const uint8_t* cls;                // per (virtual) row class; >= C: the row is in no class
  const int* items;                  // [n_items][4] = {node, pos_lo, pos_hi, sub}: features [sub * FI, +FI)
  unsigned long long* slab;          // [n_items][C * nbp][FI]
  int n_feat, C, nbp;
  float scale_g;                     // power of two, w * scale_g < 2^23
  long nmod;                         // > 0: forest batch, bins row = virtual row % nmod
};

template <int FI>
__global__ __launch_bounds__(MT) void gbdt_hist_mc_kernel(McHistArgs a) {
  constexpr int TF = FI < 16 ? FI : 16;      // feature bytes a thread owns of a row
  constexpr int TPR = FI / TF;               // threads per row (2 or 1)
  constexpr int RPP = MT / TPR;              // rows per pass
  constexpr int NW = TF / 4;                 // 32-bit words of those bytes
  extern __shared__ __attribute__((aligned(16))) unsigned long long msm[];   // [C * nbp][FI]
  const int item = xcd_remap(blockIdx.x, gridDim.x);
  const int lo = a.items[item * 4 + 1], hi = a.items[item * 4 + 2], f0 = a.items[item * 4 + 3] * FI;
  if (f0 >= a.n_feat) return;                // padding features only: the reduction never reads it
  const int ne2 = a.C * a.nbp * FI / 2;
  ulonglong2* sm2 = (ulonglong2*)msm;
  ulonglong2* out2 = (ulonglong2*)(a.slab + (size_t)item * ne2 * 2);
  if (lo >= hi) {
    for (int i = threadIdx.x; i < ne2; i += MT) out2[i] = make_ulonglong2(0ull, 0ull);
    return;
  }
  for (int i = threadIdx.x; i < ne2; i += MT) sm2[i] = make_ulonglong2(0ull, 0ull);
  __syncthreads();
  const int part = TPR == 2 ? (threadIdx.x & 1) : 0, r = threadIdx.x & (TF - 1), t = threadIdx.x / TPR;
  const uint8_t* gb = a.bins + (size_t)(f0 >> 7) * a.gs + (f0 & (QF - 1)) + part * 16;
  unsigned long long* base = msm + part * 16;
  const uint32_t nbp = a.nbp;

  using Rec = std::conditional_t<NW == 4, uint4, std::conditional_t<NW == 2, uint2, uint32_t>>;
  auto rec = [&](int v) { return *(const Rec*)(gb + (size_t)(a.nmod ? (long)v % a.nmod : (long)v) * QF); };
  // one row: q added to the row's class-keyed bin of each of the thread's TF features
  auto update = [&](float wv, uint32_t c, const Rec& bv) {
    if (wv == 0.f || c >= (uint32_t)a.C) return;
    const unsigned long long q = __float2uint_rn(wv * a.scale_g);
    // rotate the TF bytes left by r: byte j of R = feature (j + r) & (TF - 1)
    uint32_t W[NW], X[NW], Y[NW], R[NW];
    if constexpr (NW == 4) { W[0] = bv.x; W[1] = bv.y; W[2] = bv.z; W[3] = bv.w; }
    else if constexpr (NW == 2) { W[0] = bv.x; W[1] = bv.y; }
    else W[0] = bv;
#pragma unroll
    for (int k = 0; k < NW; ++k) X[k] = NW >= 2 && (r & 4) ? W[(k + 1) % NW] : W[k];
#pragma unroll
    for (int k = 0; k < NW; ++k) Y[k] = NW >= 4 && (r & 8) ? X[(k + 2) % NW] : X[k];
#pragma unroll
    for (int k = 0; k < NW; ++k) R[k] = __builtin_amdgcn_alignbyte(Y[(k + 1) % NW], Y[k], r & 3);
    unsigned long long* kb = base + (size_t)c * nbp * FI;
#pragma unroll
    for (int j = 0; j < TF; ++j) {
      const uint32_t b = (R[j >> 2] >> ((j & 3) * 8)) & 0xff;
      // a code at or past nbp lies outside every feature's bin count: not counted
      if (b < nbp) atomicAdd(&kb[b * FI + ((j + r) & (TF - 1))], q);
    }
  };
  // Software pipeline over two static register slots (as gbdt_hist_kernel): slot k's row is added,
  // then the slot is refilled with the pass two ahead, whose row id was gathered two passes
  // earlier.  Positions past `hi` are clamped to hi - 1 (valid memory, no branch around a load)
  // and get weight 0 when consumed.
  constexpr int SL = 2;
  auto row_of = [&](long p) { const int pc = (int)min(p, (long)hi - 1); return a.pos2row ? a.pos2row[pc] : pc; };
  int rn[SL];
  float wc[SL];
  uint32_t cc[SL];
  Rec bc[SL];
#pragma unroll
  for (int k = 0; k < SL; ++k) {
    const int rr = row_of((long)lo + k * RPP + t);
    wc[k] = a.w[rr]; cc[k] = a.cls[rr]; bc[k] = rec(rr);
  }
#pragma unroll
  for (int k = 0; k < SL; ++k) rn[k] = row_of((long)lo + (SL + k) * RPP + t);
  for (long p0 = lo; p0 < hi; p0 += SL * RPP) {
#pragma unroll
    for (int k = 0; k < SL; ++k) {
      const long pk = p0 + k * RPP + t;
      update(pk < hi ? wc[k] : 0.f, cc[k], bc[k]);
      wc[k] = a.w[rn[k]]; cc[k] = a.cls[rn[k]]; bc[k] = rec(rn[k]);
      rn[k] = row_of(pk + 2 * SL * RPP);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ne2; i += MT) out2[i] = sm2[i];
}

// ---------------------------------------------------------------------------------------
// Slab reduction: block (built node i, FI-feature sub-group s, class c) sums the node's items of
// that sub-group in item order (coalesced reads of the class's [nbp][FI] slice) and writes
// hist[node][c][f][0 .. 256) through an LDS transpose (row stride FI + 1: no bank conflicts);
// bins at or past nbp are 0.
// ---------------------------------------------------------------------------------------
struct McReduceArgs {
  const long long* slab;             // [n_items][C * nbp][FI]
  const int* node_items;             // [n_nodes][G][max_items] ids of the 32-feature group items, -1
                                     // padded; sub-item s of group item i is item i * (32 / FI) + s
  int max_items, G;
  const int* node_list;              // the built nodes
  long long* hist;                   // [n_nodes][C][F][NB]
  int C, F, nbp, FI;
};

__global__ __launch_bounds__(256) void gbdt_reduce_mc_kernel(McReduceArgs a) {
  extern __shared__ __attribute__((aligned(16))) long long rsm[];   // [nbp][FI + 1]
  const int FI = a.FI, S = 32 / FI, nsub = (a.F + FI - 1) / FI;
  const int c = blockIdx.x % a.C, s = (blockIdx.x / a.C) % nsub, node = a.node_list[blockIdx.x / (a.C * nsub)];
  const int* its = a.node_items + ((size_t)node * a.G + s / S) * a.max_items;
  const size_t isz = (size_t)a.C * a.nbp * FI;
  const int ne = a.nbp * FI;
  for (int e = threadIdx.x; e < ne; e += 256) {
    long long v = 0;
    for (int k = 0; k < a.max_items; ++k) {
      const int it = its[k];
      if (it < 0) break;
      v += a.slab[((size_t)it * S + s % S) * isz + (size_t)c * ne + e];
    }
    rsm[(e / FI) * (FI + 1) + e % FI] = v;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < FI * NB; o += 256) {
    const int fl = o / NB, b = o % NB, f = s * FI + fl;
    if (f < a.F) a.hist[(((size_t)node * a.C + c) * a.F + f) * NB + b] = b < a.nbp ? rsm[b * (FI + 1) + fl] : 0;
  }
}

// ---------------------------------------------------------------------------------------
// Split search, one block per (node, feature), thread t = bin / ordered position t.
//   gain(pos) = imp(T) - lw/tw imp(L) - rw/tw imp(R), imp = -sum p^2 (gini) or -sum p log2 p,
//   left = ordered bins [0 .. pos]; admissible: pos < nbins - 1, lw, rw > min_inst, gain >
//   min_gain, feature not masked; the first admissible maximum wins.
// Categorical order: key = H1 / (H0 + H1) ascending (0 when empty), ties to the lower bin, bins
// at or past nbins last.  The per-class prefixes run in int64 over the ordered bins and become
// doubles once per candidate (inv_g is a power of two), so they are exact and independent of the
// summation order; only the rates, log2 and products round (fp64, not contracted into FMAs so a
// plain host loop reproduces them).
// cand[node][f] = {gain, pos, lw, L1, rw, R1, valid, argmax class left, right, 0}.
// ---------------------------------------------------------------------------------------
struct McSplitArgs {
  long long* hist;                   // [n_nodes][C][F][NB]
  const long long* prev;             // [n_parents][C][F][NB] previous level (nullable: no derived node)
  const int* node_parent;            // [n_nodes] parent slot in prev, < 0: built node
  const int* node_sibling;           // [n_nodes] sibling slot of a derived node
  const int* nbins; const uint8_t* is_cat;
  const uint8_t* feat_mask;          // [n_nodes][F] nullable
  double* cand;                      // [n_nodes][F][NCAND]
  uint8_t* order;                    // [n_nodes][F][NB] nullable
  int C, F, nbp, gini;
  double min_inst, min_gain, inv_g;
};

__global__ __launch_bounds__(NB) void gbdt_split_mc_kernel(McSplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) long long ssm[];   // [C][nbp] sums -> prefixes, [C] totals
  __shared__ double skey[NB];
  __shared__ uint8_t sord[NB];
  __shared__ long long swave[2][NB / 64];
  __shared__ double sgain[NB / 64];
  __shared__ int spos[NB / 64];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int node = blockIdx.x / a.F, f = blockIdx.x % a.F;
  const int C = a.C, nbp = a.nbp;
  long long* stot = ssm + C * nbp;
  const size_t plane = (size_t)a.F * NB;
  long long* h = a.hist + ((size_t)node * C * a.F + f) * NB + t;
  const int par = a.prev ? a.node_parent[node] : -1;
  if (par >= 0) {       // derived: parent - sibling, kept for the next level's subtraction
    const long long* p = a.prev + ((size_t)par * C * a.F + f) * NB + t;
    const long long* s = a.hist + ((size_t)a.node_sibling[node] * C * a.F + f) * NB + t;
    for (int c = 0; c < C; ++c) {
      const long long v = p[c * plane] - s[c * plane];
      h[c * plane] = v;
      if (t < nbp) ssm[c * nbp + t] = v;
    }
  } else if (t < nbp) {
    for (int c = 0; c < C; ++c) ssm[c * nbp + t] = h[c * plane];
  }
  double* cand = a.cand + ((size_t)node * a.F + f) * NCAND;
  if (a.feat_mask && !a.feat_mask[(size_t)node * a.F + f]) {
    if (t < NCAND) cand[t] = 0.0;
    return;
  }
  const int nb = min(a.nbins[f], nbp);
  __syncthreads();
  if (a.is_cat[f]) {
    double key = __builtin_inf();
    if (t < nb) {
      const long long h1 = ssm[nbp + t], den = ssm[t] + h1;
      key = den != 0 ? (double)h1 / (double)den : 0.0;
    }
    skey[t] = key;
    __syncthreads();
    int rank = 0;       // bins ordered before bin t (every lane reads the same key: LDS broadcast)
    for (int i = 0; i < NB; ++i) {
      const double ki = skey[i];
      rank += (ki < key || (ki == key && i < t)) ? 1 : 0;
    }
    sord[rank] = (uint8_t)t;
  } else {
    sord[t] = (uint8_t)t;
  }
  __syncthreads();
  const int b = sord[t];
  if (a.order) a.order[((size_t)node * a.F + f) * NB + t] = (uint8_t)b;
  // per-class inclusive prefix over the ordered bins, in place; one barrier per class (the wave
  // totals alternate between two buffers)
  for (int c = 0; c < C; ++c) {
    long long x = b < nbp ? ssm[c * nbp + b] : 0;
    for (int off = 1; off < 64; off <<= 1) {
      const long long u = __shfl_up(x, off, 64);
      if (lane >= off) x += u;
    }
    if (lane == 63) swave[c & 1][wv] = x;
    __syncthreads();               // the class's sums are read, its wave totals written
    long long tot = 0;
    for (int v = 0; v < NB / 64; ++v) {
      const long long sv = swave[c & 1][v];
      if (v < wv) x += sv;
      tot += sv;
    }
    if (t < nbp) ssm[c * nbp + t] = x;
    if (t == 0) stot[c] = tot;
  }
  __syncthreads();
  double gain = -__builtin_inf();
  int pos = -1;
  if (t < nb - 1) {
#pragma clang fp contract(off)
    long long lq = 0, tq = 0;
    for (int c = 0; c < C; ++c) { lq += ssm[c * nbp + t]; tq += stot[c]; }
    const double lw = (double)lq * a.inv_g, tw = (double)tq * a.inv_g, rw = (double)(tq - lq) * a.inv_g;
    if (lw > a.min_inst && rw > a.min_inst) {
      const double sl = lw > 0.0 ? lw : 1.0, sr = rw > 0.0 ? rw : 1.0, st = tw > 0.0 ? tw : 1.0;
      double it = 0.0, il = 0.0, ir = 0.0;
      for (int c = 0; c < C; ++c) {
        const long long lc = ssm[c * nbp + t], tc = stot[c];
        const double pl = (double)lc * a.inv_g / sl, pr = (double)(tc - lc) * a.inv_g / sr;
        const double pt = (double)tc * a.inv_g / st;
        if (a.gini) { it -= pt * pt; il -= pl * pl; ir -= pr * pr; }
        else {
          if (pt > 0.0) it -= pt * log2(pt);
          if (pl > 0.0) il -= pl * log2(pl);
          if (pr > 0.0) ir -= pr * log2(pr);
        }
      }
      const double g = it - (tw > 0.0 ? lw / tw : 0.0) * il - (tw > 0.0 ? rw / tw : 0.0) * ir;
      if (g > a.min_gain) { gain = g; pos = t; }
    }
  }
  // block argmax: max gain, ties -> lowest position
  auto take = [&](double og, int op) {
    if (og > gain || (og == gain && op >= 0 && (pos < 0 || op < pos))) { gain = og; pos = op; }
  };
  for (int off = 32; off > 0; off >>= 1) {
    const double og = __shfl_xor(gain, off, 64);
    const int op = __shfl_xor(pos, off, 64);
    take(og, op);
  }
  if (lane == 0) { sgain[wv] = gain; spos[wv] = pos; }
  __syncthreads();
  for (int v = 0; v < NB / 64; ++v) take(sgain[v], spos[v]);
  if (pos < 0) {
    if (t < NCAND) cand[t] = 0.0;
  } else if (t == pos) {
    long long lq = 0, tq = 0, ml = -1, mr = -1;
    int cl = 0, cr = 0;
    for (int c = 0; c < C; ++c) {      // argmax class of each side, the lowest class on ties
      const long long lc = ssm[c * nbp + t], rc = stot[c] - lc;
      lq += lc; tq += stot[c];
      if (lc > ml) { ml = lc; cl = c; }
      if (rc > mr) { mr = rc; cr = c; }
    }
    const long long l1 = ssm[nbp + t];
    cand[0] = gain;
    cand[1] = (double)pos;
    cand[2] = (double)lq * a.inv_g;
    cand[3] = (double)l1 * a.inv_g;
    cand[4] = (double)(tq - lq) * a.inv_g;
    cand[5] = (double)(stot[1] - l1) * a.inv_g;
    cand[6] = 1.0;
    cand[7] = (double)cl;
    cand[8] = (double)cr;
    cand[9] = 0.0;
  }
}

// one wave per node: best[node] = {feature, pos, gain, lw, L1, rw, R1, valid, class left, class
// right} of the lowest feature with the largest gain (zeros when no feature has a valid split)
// and that feature's bin order
__global__ __launch_bounds__(64) void gbdt_choose_mc_kernel(const double* cand, const uint8_t* order, int F,
                                                            double* best, uint8_t* order_out) {
  const int node = blockIdx.x, lane = threadIdx.x;
  const double* cn = cand + (size_t)node * F * NCAND;
  double g = -__builtin_inf();
  int bf = -1;
  for (int f = lane; f < F; f += 64)
    if (cn[f * NCAND + 6] > 0.0 && cn[f * NCAND] > g) { g = cn[f * NCAND]; bf = f; }
  for (int off = 32; off > 0; off >>= 1) {
    const double og = __shfl_xor(g, off, 64);
    const int of = __shfl_xor(bf, off, 64);
    if (og > g || (og == g && of >= 0 && (bf < 0 || of < bf))) { g = og; bf = of; }
  }
  double* b = best + (size_t)node * NCAND;
  if (bf < 0) {
    if (lane < NCAND) b[lane] = 0.0;
  } else if (lane == 0) {
    const double* c = cn + bf * NCAND;
    b[0] = (double)bf; b[1] = c[1]; b[2] = c[0]; b[3] = c[2]; b[4] = c[3]; b[5] = c[4]; b[6] = c[5];
    b[7] = 1.0; b[8] = c[7]; b[9] = c[8];
  }
  if (order_out)
    ((uint32_t*)order_out)[node * (NB / 4) + lane] =
        ((const uint32_t*)(order + ((size_t)node * F + max(bf, 0)) * NB))[lane];
}

// features per histogram item: the most of 32, 16, 8, 4 whose class-keyed histogram fits the LDS
int mc_tier(int C, int nbp) {
  for (int fi = 32; fi >= 4; fi >>= 1)
    if ((long)C * nbp * fi * 8 <= MC_LDS) return fi;
  return 0;
}

template <int FI>
int launch_hist(const McHistArgs& a, int n_items, hipStream_t stream) {
  const size_t lds = (size_t)a.C * a.nbp * FI * 8;
  hipError_t e = hipFuncSetAttribute((const void*)gbdt_hist_mc_kernel<FI>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((gbdt_hist_mc_kernel<FI>), dim3(n_items), dim3(MT), lds, stream, a);
  return 0;
}

}  // namespace

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// features per item for (C, nbp), 0: too many class-keyed bins (the caller keeps the C-pass path)
SHIFU_API int shifu_gbdt_mc_tier(int C, int nbp) {
  if (C < 2 || C > 255 || nbp < 2 || nbp > NB || (nbp & (nbp - 1)) || C * nbp > MC_KEYS) return 0;
  return mc_tier(C, nbp);
}

// One pass over the level's rows for all classes, then the slab reduction of the built nodes.
// items [n_items][4] = {node, lo, hi, sub}: the 32 / FI sub-items of a 32-feature group item are
// consecutive (group item i -> items i * 32 / FI + s, sub = group * 32 / FI + s); node_items as
// for shifu_gbdt_split, ids of the group items.  slab: n_items * C * nbp * FI int64 of scratch;
// hist [n_nodes][C][F][256] gets the rows of node_list[0 .. n_list).
SHIFU_API int shifu_gbdt_hist_mc(const void* bins, long gs, const int* pos2row, const float* w, const void* cls,
                                 const int* items, int n_items, void* slab, const int* node_items, int max_items,
                                 const int* node_list, int n_list, void* hist, int C, int F, int nbp,
                                 double scale_g, long nmod, hipStream_t stream) {
  const int FI = shifu_gbdt_mc_tier(C, nbp);
  if (!FI || gs % QF || F <= 0 || n_items < 0 || n_list < 0 || max_items <= 0) return -1;
  if (n_items) {
    McHistArgs a{(const uint8_t*)bins, gs, pos2row, w, (const uint8_t*)cls, items, (unsigned long long*)slab,
                 F, C, nbp, (float)scale_g, nmod};
    int rc;
    if (FI == 32) rc = launch_hist<32>(a, n_items, stream);
    else if (FI == 16) rc = launch_hist<16>(a, n_items, stream);
    else if (FI == 8) rc = launch_hist<8>(a, n_items, stream);
    else rc = launch_hist<4>(a, n_items, stream);
    if (rc) return rc;
  }
  if (n_list) {
    McReduceArgs r{(const long long*)slab, node_items, max_items, (F + 31) / 32, node_list, (long long*)hist,
                   C, F, nbp, FI};
    const int nsub = (F + FI - 1) / FI;
    hipLaunchKernelGGL(gbdt_reduce_mc_kernel, dim3((unsigned)n_list * nsub * C), dim3(256),
                       (size_t)nbp * (FI + 1) * 8, stream, r);
  }
  CHECK_HIP(hipGetLastError());
  return 0;
}

// Split search of every node of the level (built: node_parent[node] < 0 or prev == nullptr) and
// the choice of each node's feature.  cand [n_nodes][F][10] and order [n_nodes][F][256] (nullable:
// no categorical feature) are scratch; best [n_nodes][10] doubles, order_out [n_nodes][256].
SHIFU_API int shifu_gbdt_split_mc(void* hist, const void* prev, const int* node_parent, const int* node_sibling,
                                  int n_nodes, const int* nbins, const void* is_cat, const void* feat_mask,
                                  void* cand, void* order, int C, int F, int nbp, int impurity, double min_inst,
                                  double min_gain, double inv_g, void* best, void* order_out, hipStream_t stream) {
  if (n_nodes <= 0) return 0;
  if (!shifu_gbdt_mc_tier(C, nbp) || F <= 0 || (impurity != IMP_ENTROPY && impurity != IMP_GINI)) return -1;
  if ((order == nullptr) != (order_out == nullptr)) return -1;
  McSplitArgs a{(long long*)hist, (const long long*)prev, node_parent, node_sibling, nbins, (const uint8_t*)is_cat,
                (const uint8_t*)feat_mask, (double*)cand, (uint8_t*)order, C, F, nbp, impurity == IMP_GINI,
                min_inst, min_gain, inv_g};
  hipLaunchKernelGGL(gbdt_split_mc_kernel, dim3((unsigned)n_nodes * F), dim3(NB), (size_t)(C * nbp + C) * 8, stream,
                     a);
  hipLaunchKernelGGL(gbdt_choose_mc_kernel, dim3(n_nodes), dim3(64), 0, stream, (const double*)cand,
                     (const uint8_t*)order, F, (double*)best, (uint8_t*)order_out);
  CHECK_HIP(hipGetLastError());
  return 0;
}
