// Tree-ensemble (GBT / RF) kernels for features with 257 .. 16384 bins ("wide" features:
// high-cardinality categoricals, finely binned numerics) on MI355X (gfx950).
//
// The narrow path (gbdt_kernels.hip) packs 32 uint8 features per work item and 256 bins per
// feature into 64 KiB of LDS.  A wide feature has up to 64x the bins, so here the split of the
// work is transposed: the codes are uint16 and column-major ([Fw][N], one column per wide
// feature, always in HBM), a histogram work item is {node, row range, ONE wide feature}, and the
// whole 160-KiB LDS of a CU holds that one feature's packed histogram.
//   * gbdt_hist_wide_kernel   one packed ds_add_u64 per row into one of up to 8 LDS copies chosen
//                             by the lane id, unpacked to int64 registers every 4096 rows per copy
//   * gbdt_split_wide_kernel  one block per (node, wide feature): slab reduce / parent - sibling,
//                             rank-by-counting sort of the categorical keys in LDS, int64 block
//                             prefix over the ordered bins, gain scan
//   * gbdt_partition_flag_wide_kernel / gbdt_apply_tree_wide_kernel
//                             routing when a split feature may be wide (code from the uint16
//                             column, categorical left sets of CW 32-bit words)
// Fixed-point units, scan rules and candidate rows are those of gbdt_kernels.hip (gbdt_shared.h),
// so wide and narrow candidates compete in the same cand[node][feature][8] table.
#include "common.h"
#include "gbdt_shared.h"

namespace {

constexpr int WT = 1024;             // threads per block (16 waves, one block per CU)
constexpr int WMAX = 16384;          // most bins of a feature = packed u64 LDS entries (128 KiB)
constexpr int WNE = WMAX / WT;       // histogram entries / scan positions a thread owns (<= 16)
constexpr int WU = 4;                // rows in flight per thread and pass

// a feature's bins rounded up to the block's unpack stride (host: models/gbdt.py _pad_bins)
__device__ __forceinline__ int pad_bins(int nb) { return (nb + WT - 1) / WT * WT; }

struct WideHistArgs {
  const uint16_t* wbins; long n;     // [Fw][n] codes of the wide features, column-major
  const int* nbins_w;                // [Fw]
  const int* pos2row;                // position -> (virtual) row; nullptr: identity (the root)
  const float* w; const float* g;    // per row, or per position when wg_by_pos
  int wg_by_pos;
  const int* items;                  // [n_items][4] = {node slot, pos_lo, pos_hi, wide feature j}
  long long* slab;                   // [n_items][2][nbp] int64 fixed point
  int nbp;                           // slab stride: the widest feature's padded bins
  float scale_w, scale_g;
  long nmod;                         // > 0: forest batch, row = pos2row[p] % nmod
};

// LDS: copies x nbf packed u64 entries, nbf = this feature's padded bins, copies = min(8,
// 16384 / nbf) rounded down to a power of two.  Lane l adds into copy l & (copies - 1): with one
// category holding most rows a wave's 64 atomics spread over `copies` addresses (distinct banks,
// nbf is a multiple of 1024) instead of serialising on one.  Every copy gets 1024 / copies rows
// per 1024-row pass, so after `copies` iterations of WU passes it has seen exactly 4096 rows: the
// field-width bound of the packed entry (qw < 2^16 -> 28 bits, |qg| < 2^23 -> 36 bits signed).
// Then every thread unpacks its <= 16 entries (summed over the copies) into int64 registers --
// the same sums as two independent int64 accumulations, whatever the row order.
__global__ __launch_bounds__(WT) void gbdt_hist_wide_kernel(WideHistArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long wsm[];
  const int item = blockIdx.x, tid = threadIdx.x;
  const int lo = a.items[item * 4 + 1], hi = a.items[item * 4 + 2], j = a.items[item * 4 + 3];
  long long* out = a.slab + (size_t)item * 2 * a.nbp;
  if (lo >= hi) {
    for (int i = tid; i < 2 * a.nbp; i += WT) out[i] = 0;
    return;
  }
  const int nbf = min(pad_bins(a.nbins_w[j]), a.nbp);
  const int cmax = min(8, WMAX / nbf);
  const int copies = 1 << (31 - __clz(cmax));
  for (int i = tid; i < copies * nbf; i += WT) wsm[i] = 0ull;
  __syncthreads();
  const uint16_t* col = a.wbins + (size_t)j * a.n;
  unsigned long long* my = wsm + (size_t)(tid & (copies - 1)) * nbf;
  long long accw[WNE], accg[WNE];
#pragma unroll
  for (int k = 0; k < WNE; ++k) { accw[k] = 0; accg[k] = 0; }
  auto unpack = [&](bool clear) {
#pragma unroll
    for (int k = 0; k < WNE; ++k) {
      const int e = tid + k * WT;
      if (e < nbf)
        for (int c = 0; c < copies; ++c) {
          unpack_add(wsm[c * nbf + e], accw[k], accg[k]);
          if (clear) wsm[c * nbf + e] = 0ull;
        }
    }
  };
  int it = 0;
  for (long p0 = lo; p0 < hi; p0 += WU * WT) {        // block-uniform trip count (unpack barriers)
    float wv[WU], gv[WU];
    uint32_t code[WU];
#pragma unroll
    for (int u = 0; u < WU; ++u) {
      const long p = p0 + u * WT + tid;
      wv[u] = 0.f; gv[u] = 0.f; code[u] = 0;
      if (p < hi) {
        const long v = a.pos2row ? a.pos2row[p] : p, k = a.wg_by_pos ? p : v;
        wv[u] = a.w[k]; gv[u] = a.g[k];
        code[u] = col[a.nmod ? v % a.nmod : v];
      }
    }
#pragma unroll
    for (int u = 0; u < WU; ++u)
      if (wv[u] != 0.f && code[u] < (uint32_t)nbf)
        atomicAdd(&my[code[u]], ((unsigned long long)__float2uint_rn(wv[u] * a.scale_w) << PACK_G) +
                                    (unsigned long long)(long long)__float2int_rn(wv[u] * gv[u] * a.scale_g));
    if (++it == copies) {
      it = 0;
      __syncthreads();
      unpack(true);
      __syncthreads();
    }
  }
  __syncthreads();
  unpack(false);
#pragma unroll
  for (int k = 0; k < WNE; ++k) {
    const int e = tid + k * WT;
    if (e < nbf) { out[e] = accw[k]; out[a.nbp + e] = accg[k]; }
  }
  for (int e = nbf + tid; e < a.nbp; e += WT) { out[e] = 0; out[a.nbp + e] = 0; }
}

// ---------------------------------------------------------------------------------------
// Split search, one block per (node, wide feature j).  Modes as gbdt_split_kernel:
//   0  hist_w[node][.][j] = sum of the node's item slabs (no scan: the all-reduce comes next)
//   2  scan the reduced histogram
//   1  hist_w[node] = parent - sibling, then scan
// Scan: left = ordered bins [0..b], b < nb - 1; lw, rw > min_inst; gain > min_gain; best gain,
// ties to the lowest b.  Categorical order: key = s / w ascending (empty bin 4.9e-324), stable by
// bin index, bins >= nb last.  The prefix sums run in int64 over the ordered bins and become
// doubles once per candidate ((double)sum * inv, the scales are powers of two), so they do not
// depend on the summation order and the host oracle reproduces them exactly.
// ---------------------------------------------------------------------------------------
struct WideSplitArgs {
  const long long* slab;             // [n_items][2][nbp]
  const int* node_items;             // [n_nodes][Fw][max_items] item ids, -1 padded (mode 0)
  int max_items;
  const long long* parent_hist;      // [n_parent][2][Fw][nbp] (mode 1)
  const int* node_parent; const int* node_sibling;
  long long* hist;                   // [n_nodes][2][Fw][nbp]
  const int* node_list; int n_list;
  const int* wide_feat;              // [Fw] feature index of wide column j
  const int* nbins_w;                // [Fw]
  int Fw, nbp;
  const uint8_t* is_cat;             // [F]
  const uint8_t* feat_mask;          // [n_nodes][F] nullable
  float* cand;                       // [n_nodes][F][8]: the row the narrow kernel leaves invalid
  uint16_t* cat_order;               // [n_nodes][Fw][nbp] nullable
  int F, mode, impurity;
  float min_inst, min_gain;
  double inv_w, inv_g;
};

__global__ __launch_bounds__(WT) void gbdt_split_wide_kernel(WideSplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) double skey[];   // [nbp] keys, then uint16 order
  __shared__ long long swave[WT / 64][2];
  __shared__ double sbest[WT / 64][3];
  __shared__ int sbin[WT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int node = a.node_list[blockIdx.x / a.Fw], j = blockIdx.x % a.Fw;
  const int f = a.wide_feat[j], nbp = a.nbp;
  const size_t plane = (size_t)a.Fw * nbp;
  long long* hw = a.hist + (size_t)node * 2 * plane + (size_t)j * nbp;
  long long* hg = hw + plane;
  if (a.mode == 0) {
    const int* its = a.node_items + ((size_t)node * a.Fw + j) * a.max_items;
    for (int b = tid; b < nbp; b += WT) {
      long long qw = 0, qg = 0;
      for (int t = 0; t < a.max_items; ++t) {
        const int it = its[t];
        if (it < 0) break;
        const long long* s = a.slab + (size_t)it * 2 * nbp;
        qw += s[b]; qg += s[nbp + b];
      }
      hw[b] = qw; hg[b] = qg;
    }
    return;
  }
  if (a.mode == 1) {
    const int par = a.node_parent[node], sib = a.node_sibling[node];
    const long long* pw = a.parent_hist + (size_t)par * 2 * plane + (size_t)j * nbp;
    const long long* sw = a.hist + (size_t)sib * 2 * plane + (size_t)j * nbp;
    for (int b = tid; b < nbp; b += WT) {
      hw[b] = pw[b] - sw[b];
      hg[b] = pw[plane + b] - sw[plane + b];
    }
    __syncthreads();               // the scan below reads other threads' bins
  }
  float* cand = a.cand + ((size_t)node * a.F + f) * 8;
  if (a.feat_mask && !a.feat_mask[(size_t)node * a.F + f]) {
    if (tid == 0) { cand[0] = -1.f; cand[6] = 0.f; }
    return;
  }
  const int nb = min(a.nbins_w[j], nbp), nbf = min(pad_bins(nb), nbp);
  const bool cat = a.is_cat[f] != 0;
  uint16_t* sord = (uint16_t*)skey;
  if (cat) {
    // keys of this thread's bins (registers) and of every bin (LDS)
    double kk[WNE];
    int rank[WNE];
#pragma unroll
    for (int k = 0; k < WNE; ++k) {
      const int e = tid + k * WT;
      kk[k] = 0.0; rank[k] = 0;
      if (e < nb) {
        const double cw = (double)hw[e] * a.inv_w, cs = (double)hg[e] * a.inv_g;
        kk[k] = cw != 0.0 ? cs / cw : 4.9e-324;
        skey[e] = kk[k];
      }
    }
    __syncthreads();
    // rank by counting: bins ordered before bin e (every lane reads the same key: LDS broadcast)
    const int nk = (nb + WT - 1) / WT;
    for (int i = 0; i < nb; ++i) {
      const double ki = skey[i];
#pragma unroll
      for (int k = 0; k < WNE; ++k)
        if (k < nk) rank[k] += (ki < kk[k] || (ki == kk[k] && i < tid + k * WT)) ? 1 : 0;
    }
    __syncthreads();               // every key is read: the order takes over the LDS
#pragma unroll
    for (int k = 0; k < WNE; ++k) {
      const int e = tid + k * WT;
      if (e < nb) sord[rank[k]] = (uint16_t)e;
      else if (e < nbf) sord[e] = (uint16_t)e;
    }
    __syncthreads();
    if (a.cat_order) {
      uint16_t* co = a.cat_order + ((size_t)node * a.Fw + j) * nbp;
      for (int b = tid; b < nbp; b += WT) co[b] = b < nbf ? sord[b] : (uint16_t)b;
    }
  }
  // ---- int64 inclusive prefix over the ordered bins: thread t owns positions [t per, (t + 1) per)
  const int per = nbf / WT;
  long long pw[WNE], ps[WNE];
  long long tw_ = 0, ts_ = 0;
#pragma unroll
  for (int k = 0; k < WNE; ++k) {
    pw[k] = 0; ps[k] = 0;
    if (k < per) {
      const int i = tid * per + k, b = cat ? sord[i] : i;
      tw_ += hw[b]; ts_ += hg[b];
      pw[k] = tw_; ps[k] = ts_;
    }
  }
  long long xw = tw_, xs = ts_;
  for (int off = 1; off < 64; off <<= 1) {
    const long long uw = __shfl_up(xw, off, 64), us = __shfl_up(xs, off, 64);
    if (lane >= off) { xw += uw; xs += us; }
  }
  if (lane == 63) { swave[wv][0] = xw; swave[wv][1] = xs; }
  __syncthreads();
  long long ew = xw - tw_, es = xs - ts_, totw = 0, tots = 0;   // exclusive offsets, totals
  for (int v = 0; v < WT / 64; ++v) {
    if (v < wv) { ew += swave[v][0]; es += swave[v][1]; }
    totw += swave[v][0]; tots += swave[v][1];
  }
  const double tw = (double)totw * a.inv_w, ts = (double)tots * a.inv_g;
  double best = -1.0, blw = 0, bls = 0;
  int bbin = -1;
#pragma unroll
  for (int k = 0; k < WNE; ++k) {
    const int i = tid * per + k;
    if (k < per && i < nb - 1) {
      const double lw = (double)(ew + pw[k]) * a.inv_w, ls = (double)(es + ps[k]) * a.inv_g;
      const double rw = tw - lw, rs = ts - ls;
      if (lw > a.min_inst && rw > a.min_inst) {
        const double gain = imp_gain(a.impurity, lw, ls, rw, rs);
        if (gain > a.min_gain && gain > best) { best = gain; bbin = i; blw = lw; bls = ls; }
      }
    }
  }
  // block argmax: max gain, ties -> lowest position
  auto take = [&](double og, int ob, double olw, double ols) {
    if ((og > best) || (og == best && ob >= 0 && (bbin < 0 || ob < bbin))) { best = og; bbin = ob; blw = olw; bls = ols; }
  };
  for (int off = 32; off > 0; off >>= 1) {
    const double og = __shfl_xor(best, off, 64), olw = __shfl_xor(blw, off, 64), ols = __shfl_xor(bls, off, 64);
    const int ob = __shfl_xor(bbin, off, 64);
    take(og, ob, olw, ols);
  }
  if (lane == 0) { sbest[wv][0] = best; sbest[wv][1] = blw; sbest[wv][2] = bls; sbin[wv] = bbin; }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < WT / 64; ++v) take(sbest[v][0], sbin[v], sbest[v][1], sbest[v][2]);
    cand[0] = (float)best;
    cand[1] = (float)bbin;
    cand[2] = (float)blw;
    cand[3] = (float)bls;
    cand[4] = (float)(tw - blw);
    cand[5] = (float)(ts - bls);
    cand[6] = bbin >= 0 ? 1.f : 0.f;
    cand[7] = (float)tw;
  }
}

// ---------------------------------------------------------------------------------------
// Routing when the data has wide features: a row's code of feature f comes from the uint16
// column wide_of[f] (>= 0) or from the quad-blocked uint8 record; a categorical left set is cw
// 32-bit words per node.
// ---------------------------------------------------------------------------------------
struct WideBins {
  const uint8_t* bins; long gs;      // quad-blocked [Q][N][128] (a wide feature's byte is 0)
  const uint16_t* wbins; long n;     // [Fw][n]
  const int* wide_of;                // [F] column of a wide feature, -1: narrow
};

__device__ __forceinline__ uint32_t code_of(const WideBins& d, long row, int f) {
  const int j = d.wide_of[f];
  return j >= 0 ? d.wbins[(size_t)j * d.n + row] : d.bins[bin_off(d.gs, row, f)];
}

__device__ __forceinline__ bool goes_left(uint32_t b, bool cat, const uint32_t* words, int cw, int thr) {
  if (cat) return (int)(b >> 5) < cw && ((words[b >> 5] >> (b & 31)) & 1);
  return (int)b <= thr;
}

struct WidePartArgs {
  WideBins d;
  const int* pos2row; const int* pos_node;
  const int* split_feat; const int* split_bin;
  const uint32_t* cat_left; int cw;  // [n_nodes][cw]
  const uint8_t* is_cat;
  unsigned long long* fbits; int* wcnt;     // nullable, as gbdt_partition_flag_kernel
  long n, nmod;
  float* pred; const float* node_val; const float* child_l_val; const float* child_r_val;
  float scale; int final_level;
};

__global__ __launch_bounds__(256) void gbdt_partition_flag_wide_kernel(WidePartArgs a) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int fl = 0;
  if (p < a.n) {
    const int nd = a.pos_node[p];
    const long v = a.pos2row[p], row = a.nmod ? v % a.nmod : v;
    const int f = nd >= 0 ? a.split_feat[nd] : -1;
    if (f >= 0) {
      fl = goes_left(code_of(a.d, row, f), a.is_cat[f] != 0, a.cat_left + (size_t)nd * a.cw, a.cw, a.split_bin[nd]);
      if (a.pred && a.final_level) a.pred[row] += a.scale * (fl ? a.child_l_val[nd] : a.child_r_val[nd]);
    } else if (a.pred && nd >= 0) {
      a.pred[row] += a.scale * a.node_val[nd];
    }
  }
  if (a.fbits) {
    const unsigned long long m = __ballot(fl);
    if ((threadIdx.x & 63) == 0 && p < a.n) {
      a.fbits[p >> 6] = m;
      a.wcnt[p >> 6] = __popcll(m);
    }
  }
}

struct WideTreeArgs {
  WideBins d;
  const int* feat; const int* thr; const uint32_t* cat_left; int cw; const float* value; const uint8_t* is_cat;
  float* pred; float scale; int set_mode;
  long n; int max_nodes;
};

__global__ void gbdt_apply_tree_wide_kernel(WideTreeArgs a) {
  const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= a.n) return;
  int id = 1;
  while (id < a.max_nodes && a.feat[id] >= 0) {
    const int f = a.feat[id];
    id = 2 * id + (goes_left(code_of(a.d, row, f), a.is_cat[f] != 0, a.cat_left + (size_t)id * a.cw, a.cw, a.thr[id]) ? 0 : 1);
  }
  const float v = a.value[id];
  if (a.set_mode) a.pred[row] = v; else a.pred[row] += a.scale * v;
}

}  // namespace

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

// nbp: the widest feature's bins rounded up to 1024 (the slab stride; every nbins_w[j] <= nbp)
SHIFU_API int shifu_gbdt_hist_wide(const void* wbins, long n, const int* nbins_w, const int* pos2row, const float* w,
                                   const float* g, int wg_by_pos, const int* items, int n_items, void* slab, int nbp,
                                   double scale_w, double scale_g, long nmod, hipStream_t stream) {
  if (n <= 0 || n_items <= 0 || nbp <= 0 || nbp > WMAX || nbp % WT || (wg_by_pos && nmod)) return -1;
  WideHistArgs a{(const uint16_t*)wbins, n, nbins_w, pos2row, w, g, wg_by_pos, items, (long long*)slab, nbp,
                 (float)scale_w, (float)scale_g, nmod};
  const size_t lds = (size_t)(8 * nbp < WMAX ? 8 * nbp : WMAX) * 8;
  hipLaunchKernelGGL(gbdt_hist_wide_kernel, dim3(n_items), dim3(WT), lds, stream, a);
  CHECK_HIP(hipGetLastError());
  return 0;
}

SHIFU_API int shifu_gbdt_split_wide(const void* slab, const int* node_items, int max_items, const void* parent_hist,
                                    const int* node_parent, const int* node_sibling, void* hist, const int* node_list,
                                    int n_list, const int* wide_feat, const int* nbins_w, int Fw, int nbp,
                                    const void* is_cat, const void* feat_mask, float* cand, void* cat_order, int F,
                                    int mode, int impurity, float min_inst, float min_gain, double inv_w,
                                    double inv_g, hipStream_t stream) {
  if (n_list <= 0 || Fw <= 0) return 0;
  if (nbp <= 0 || nbp > WMAX || nbp % WT || mode < 0 || mode > 2) return -1;
  WideSplitArgs a{(const long long*)slab, node_items, max_items, (const long long*)parent_hist, node_parent,
                  node_sibling, (long long*)hist, node_list, n_list, wide_feat, nbins_w, Fw, nbp,
                  (const uint8_t*)is_cat, (const uint8_t*)feat_mask, cand, (uint16_t*)cat_order, F, mode, impurity,
                  min_inst, min_gain, inv_w, inv_g};
  const size_t lds = mode == 0 ? 0 : (size_t)nbp * 8;
  hipLaunchKernelGGL(gbdt_split_wide_kernel, dim3((unsigned)n_list * Fw), dim3(WT), lds, stream, a);
  CHECK_HIP(hipGetLastError());
  return 0;
}

SHIFU_API int shifu_gbdt_partition_flag_wide(const void* bins, long gs, const void* wbins, long n_rows,
                                             const int* wide_of, const int* pos2row, const int* pos_node,
                                             const int* split_feat, const int* split_bin, const void* cat_left,
                                             int cw, const void* is_cat, void* fbits, int* wcnt, long n, long nmod,
                                             float* pred, const float* node_val, const float* child_l_val,
                                             const float* child_r_val, float scale, int final_level,
                                             hipStream_t stream) {
  if (n <= 0) return 0;
  if (!pos_node || !wide_of || cw <= 0 || n_rows <= 0) return -1;
  WidePartArgs a{{(const uint8_t*)bins, gs, (const uint16_t*)wbins, n_rows, wide_of}, pos2row, pos_node, split_feat,
                 split_bin, (const uint32_t*)cat_left, cw, (const uint8_t*)is_cat, (unsigned long long*)fbits, wcnt,
                 n, nmod, pred, node_val, child_l_val, child_r_val, scale, final_level};
  hipLaunchKernelGGL(gbdt_partition_flag_wide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  CHECK_HIP(hipGetLastError());
  return 0;
}

SHIFU_API int shifu_gbdt_apply_tree_wide(const void* bins, long gs, const void* wbins, long n_rows,
                                         const int* wide_of, const int* feat, const int* thr, const void* cat_left,
                                         int cw, const float* value, const void* is_cat, float* pred, float scale,
                                         int set_mode, long n, int max_nodes, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!wide_of || cw <= 0 || n_rows < n) return -1;
  WideTreeArgs a{{(const uint8_t*)bins, gs, (const uint16_t*)wbins, n_rows, wide_of}, feat, thr,
                 (const uint32_t*)cat_left, cw, value, (const uint8_t*)is_cat, pred, scale, set_mode, n, max_nodes};
  hipLaunchKernelGGL(gbdt_apply_tree_wide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
  CHECK_HIP(hipGetLastError());
  return 0;
}
