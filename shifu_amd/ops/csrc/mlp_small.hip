// Fused one-kernel gradient step for small MLPs (gfx950 / CDNA4): 1 or 2 hidden layers of at most
// 64 nodes, one output, first-layer padded input width kp0 = 128 or 256 (mlp_small_kernel: at
// kp0 = 256 the 128-row tile, the weights and the delta tiles fill 153 of the CU's 160 KiB of LDS)
// or 384 or 512 (mlp_small_wide_kernel, the same step on a 64-row tile, described where it stands).
//
// One launch per row chunk does forward, output neuron, loss, deltas, hidden dgrad and every
// layer's wgrad.  X is read from HBM once; no activation or delta goes to HBM.
//
//   grid    one 256-thread block per CU (at most one per 128-row tile); block b takes tiles b,
//           b + grid, ...  Wave w owns rows [32 w, 32 w + 32) of the tile for the forward/backward
//           row math and a quarter of the X columns for the first layer's wgrad.
//   LDS     W1 [64][kp0] bf16 (16-B chunk c of row h at c ^ (h & 15)), W2 [64][64] bf16 (bias and
//           padding zeroed), output weights / layer-2 biases fp32, the tile's X [128][kp0] (chunk
//           c of row r at c ^ ((r & 7) << 1)) and the bf16 tiles D1, H1, D2 [128][64].
//   forward transposed: Z1^T = W1 X^T, so a lane holds ONE row (lane & 15) and the 4 nodes
//           4 q + i (q = lane >> 4) of every 16-node block.  Two packed blocks are the B fragment of
//           the next MFMA as they are (the k order inside a 32-block is permuted the same way on
//           the weight side), so H1 -> Z2 and D2 -> D1 (dgrad, weights by ds_read_b64_tr_b16)
//           need no shuffle; the output dot product is 16 VALU FMAs and two xor shuffles.
//   wgrad   after a barrier every wave reads the whole tile's D (A operand) and its X column slice
//           (B operand) transposed from LDS (ds_read_b64_tr_b16) and accumulates dW1 [64][kp0/4]
//           and dW2 [64][16] in registers across all of the block's tiles.
//   output  every block writes one fp32 row [params.numel] of a slab and its fp64 (error, weight)
//           pair; small_reduce_kernel adds the rows in block order into the gradient.  No atomics:
//           gradient and error are bitwise reproducible.
// Rows are addressed with 64-bit bases, so a chunk may be any size an int row count allows.
#include <type_traits>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;

constexpr int SM_T = 256;          // 4 waves
constexpr int SM_TILE = 128;       // rows per block tile (32 per wave)
constexpr int SM_KU = 128;         // padded width of every layer above the first (hidden <= 64)
constexpr int SM_TILE_B = SM_TILE * 64 * 2;   // one [128][64] bf16 tile

struct SmallArgs {
  const bf16_t* X; long ldx;       // [M][ldx] rows, bias column 1, padding 0
  const bf16_t* W1;                // [h1][kp0] bf16
  const bf16_t* W2;                // [h2][128] bf16, bias at column h1 (two hidden layers)
  const float* Wo;                 // [128] fp32 output weights, bias at the last hidden width
  const float* Y; const float* S;  // [M] targets, [M] row weights (nullable -> 1)
  float* slab;                     // [grid][numel] per-block gradient rows
  double* err_slab;                // [grid][2]
  float* P;                        // [M] predictions (forward only)
  long numel;
  int M, ntiles, h1, h2, act1, act2, out_act, loss;
  float flat1, flat2, flat_out;
};

__host__ __device__ constexpr int sm_lds_bytes(int kp0, bool train) {
  return 64 * kp0 * 2 + 8192 + 1024 + (train ? SM_TILE * kp0 * 2 + 3 * SM_TILE_B : 0);
}
// byte offset of columns col.. (col % 4 == 0) of row r in the X tile / in a [128][64] tile
__device__ __forceinline__ int sm_xoff(int r, int col, int pitch) {
  return r * pitch + ((((col >> 3) ^ ((r & 7) << 1))) << 4) + ((col & 4) << 1);
}
__device__ __forceinline__ int sm_toff(int r, int col) {
  return r * 128 + ((((col >> 4) ^ ((r >> 1) & 3))) << 5) + ((col & 12) << 1);
}
// transposed fragment: lane (g, tq, tp) passes the quad at 4 tp of rows tq and tq + 4 (or + 16) of
// its group's rows and receives column (lane & 15) of the 8 rows
__device__ __forceinline__ bf16x8 sm_tr(const char* lo, const char* hi) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)lo);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)hi);
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ void sm_unpk(const uint2 v, float* f) {
  f[0] = bf2f(v.x & 0xffff); f[1] = bf2f(v.x >> 16); f[2] = bf2f(v.y & 0xffff); f[3] = bf2f(v.y >> 16);
}
__device__ __forceinline__ bf16x8 sm_join(const uint2 a, const uint2 b) {
  return __builtin_bit_cast(bf16x8, make_uint4(a.x, a.y, b.x, b.y));
}

template <int KS, bool TWO, bool TRAIN>
__global__ __launch_bounds__(SM_T) void mlp_small_kernel(SmallArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KP0 = 32 * KS, PITCH = KP0 * 2, CB = KS / 2;
  constexpr int oW1 = 0, oW2 = 64 * PITCH, oF = oW2 + 8192, oX = oF + 1024, oD1 = oX + SM_TILE * PITCH,
                oH1 = oD1 + SM_TILE_B, oD2 = oH1 + SM_TILE_B;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int tq = lr >> 2, tp = lane & 3;
  const int nb1 = (p.h1 + 15) >> 4, nb2 = TWO ? (p.h2 + 15) >> 4 : 0;
  const int nvl = TWO ? p.h2 : p.h1, nbl = TWO ? nb2 : nb1;     // the last hidden layer
  const int actl = TWO ? p.act2 : p.act1;
  const float flatl = TWO ? p.flat2 : p.flat1;
  float* fw = (float*)(smem + oF);                              // [0,64) Wo, [64] its bias, [128,192) b2

  // ---- weights -> LDS, once per block (rows / columns past the real widths are zero)
  for (int idx = tid; idx < 64 * (KP0 / 8); idx += SM_T) {
    const int h = idx / (KP0 / 8), c = idx % (KP0 / 8);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (h < p.h1) v = *(const uint4*)(p.W1 + (size_t)h * KP0 + c * 8);
    *(uint4*)(smem + oW1 + h * PITCH + ((c ^ (h & 15)) << 4)) = v;
  }
  if (TWO)
    for (int idx = tid; idx < 64 * 64; idx += SM_T) {
      const int j = idx >> 6, i = idx & 63;
      ((bf16_t*)(smem + oW2))[idx] = (j < p.h2 && i < p.h1) ? p.W2[(size_t)j * SM_KU + i] : (bf16_t)0;
    }
  if (tid < 64) {
    fw[tid] = tid < nvl ? p.Wo[tid] : 0.f;
    fw[128 + tid] = (TWO && tid < p.h2) ? bf2f(p.W2[(size_t)tid * SM_KU + p.h1]) : 0.f;
  }
  if (tid == 64) fw[64] = p.Wo[nvl];
  __syncthreads();

  uint4 xf[2][KS];                 // the wave's 32 rows as MFMA fragments: row lr (+16), k 32 ks + 8 q ..
  float yv[2], sv[2];
  auto load_x = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const long row = (long)tile * SM_TILE + 32 * w + 16 * mb + lr;
      const bool ok = row < p.M;
      const bf16_t* src = p.X + row * p.ldx + 8 * q;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xf[mb][ks] = ok ? *(const uint4*)(src + 32 * ks) : make_uint4(0, 0, 0, 0);
      yv[mb] = (TRAIN && ok) ? p.Y[row] : 0.f;
      sv[mb] = (TRAIN && ok && p.S) ? p.S[row] : 1.f;
    }
  };

  f32x4 acc1[4][CB], acc2[4];      // dW1 [h block][column block of the wave's slice], dW2 [j block]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CB; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float gwo[4][4], gb2[4][4], gbo = 0.f;   // output-weight / layer-2 bias gradient partials of the lane's rows
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) gwo[i][j] = gb2[i][j] = 0.f;
  double esum = 0.0, wsum = 0.0;

  load_x(blockIdx.x);
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    // ---- layer 1: Z1^T = W1 X^T (the bias rides in X's 1-column), the X tile goes to LDS
    f32x4 z1[4][2];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) z1[nb][0] = z1[nb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (TRAIN) {
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
          *(uint4*)(smem + oX + sm_xoff(32 * w + 16 * mb + lr, 32 * ks + 8 * q, PITCH)) = xf[mb][ks];
      }
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        if (nb < nb1) {
          const bf16x8 wf = *(const bf16x8*)(smem + oW1 + (16 * nb + lr) * PITCH + (((4 * ks + q) ^ lr) << 4));
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
            z1[nb][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(bf16x8, xf[mb][ks]),
                                                                 z1[nb][mb], 0, 0, 0);
        }
    }
    // activation, zero padding, bf16 rounding (where the layer kernels round)
    auto activate = [&](const f32x4 (&z)[4][2], uint2 (&pk)[4][2], int nb_, int nv, int act) __attribute__((always_inline)) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          float a[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            a[i] = (nb < nb_ && 16 * nb + 4 * q + i < nv) ? act_fwd(act, z[nb][mb][i]) : 0.f;
          pk[nb][mb] = make_uint2(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]));
        }
    };
    uint2 pk1[4][2], pk2[4][2];
    activate(z1, pk1, nb1, p.h1, p.act1);
    if (TWO) {
      // ---- layer 2: Z2^T = W2 H1^T + b2; the packed H1 blocks 2 ks, 2 ks + 1 are the B fragment
      f32x4 z2[4][2];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const f32x4 b = *(const f32x4*)(fw + 128 + 16 * jb + 4 * q);
        z2[jb][0] = z2[jb][1] = b;
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        if (2 * ks < nb1) {
#pragma unroll
          for (int jb = 0; jb < 4; ++jb)
            if (jb < nb2) {
              const char* wr = smem + oW2 + (16 * jb + lr) * 128 + (32 * ks + 4 * q) * 2;
              const bf16x8 wf = sm_join(*(const uint2*)wr, *(const uint2*)(wr + 32));
#pragma unroll
              for (int mb = 0; mb < 2; ++mb)
                z2[jb][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, sm_join(pk1[2 * ks][mb], pk1[2 * ks + 1][mb]),
                                                                     z2[jb][mb], 0, 0, 0);
            }
        }
      activate(z2, pk2, nb2, p.h2, p.act2);
    }
    const uint2 (&pkl)[4][2] = TWO ? pk2 : pk1;

    // ---- output neuron, loss, output delta: every lane of a row's 4 holds the same values
    float dl[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      float zo = 0.f;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        if (nb < nbl) {
          float h[4];
          sm_unpk(pkl[nb][mb], h);
#pragma unroll
          for (int i = 0; i < 4; ++i) zo += h[i] * fw[16 * nb + 4 * q + i];
        }
      zo += __shfl_xor(zo, 16, 64);
      zo += __shfl_xor(zo, 32, 64);
      zo += fw[64];
      const long row = (long)tile * SM_TILE + 32 * w + 16 * mb + lr;
      const bool valid = row < p.M;
      const float a = act_fwd(p.out_act, zo);
      if (!TRAIN) {
        if (valid && q == 0) p.P[row] = a;
        continue;
      }
      float contrib;
      out_loss_delta(p.out_act, p.loss, true, p.flat_out, zo, a, yv[mb], sv[mb], dl[mb], contrib);
      if (!valid) dl[mb] = 0.f;
      if (valid && q == 0) { esum += contrib; wsum += sv[mb]; }
      gbo += dl[mb];
    }
    if (!TRAIN) {
      load_x(tile + gridDim.x);
      continue;
    }

    // ---- deltas of the last hidden layer D = dl * Wo * (f'(H) + flat), output-weight gradient
    uint2 dkl[4][2];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        float h[4], d[4];
        sm_unpk(pkl[nb][mb], h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = 16 * nb + 4 * q + i;
          d[i] = (nb < nbl && c < nvl) ? dl[mb] * fw[c] * (act_deriv_out(actl, h[i]) + flatl) : 0.f;
          gwo[nb][i] += dl[mb] * h[i];
          if (TWO) gb2[nb][i] += d[i];
        }
        dkl[nb][mb] = make_uint2(pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3]));
      }
    auto put_tile = [&](int off, const uint2 (&v)[4][2], int nb_) __attribute__((always_inline)) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        if (nb < nb_) {
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
            *(uint2*)(smem + off + sm_toff(32 * w + 16 * mb + lr, 16 * nb + 4 * q)) = v[nb][mb];
        }
    };
    if (TWO) {
      // ---- dgrad: D1^T = (W2^T D2^T) * (f'(H1) + flat1); W2^T fragments by transposed reads
      f32x4 b1[4][2];
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) b1[ib][0] = b1[ib][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        if (2 * ks < nb2) {
#pragma unroll
          for (int ib = 0; ib < 4; ++ib)
            if (ib < nb1) {
              const char* wr = smem + oW2 + (32 * ks + 4 * q + tq) * 128 + (16 * ib + 4 * tp) * 2;
              const bf16x8 wf = sm_tr(wr, wr + 16 * 128);
#pragma unroll
              for (int mb = 0; mb < 2; ++mb)
                b1[ib][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, sm_join(dkl[2 * ks][mb], dkl[2 * ks + 1][mb]),
                                                                     b1[ib][mb], 0, 0, 0);
            }
        }
      uint2 dk1[4][2];
#pragma unroll
      for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          float h[4], d[4];
          sm_unpk(pk1[ib][mb], h);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            d[i] = (ib < nb1 && 16 * ib + 4 * q + i < p.h1) ? b1[ib][mb][i] * (act_deriv_out(p.act1, h[i]) + p.flat1) : 0.f;
          dk1[ib][mb] = make_uint2(pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3]));
        }
      put_tile(oD1, dk1, nb1);
      put_tile(oH1, pk1, nb1);
      put_tile(oD2, dkl, nb2);
    } else {
      put_tile(oD1, dkl, nb1);
    }
    __syncthreads();
    load_x(tile + gridDim.x);        // the next tile's rows land during the wgrad

    // ---- wgrad over the tile's 128 rows, 32 per MFMA: dW1 slice [64][KP0 / 4], dW2 slice [64][16]
#pragma unroll
    for (int rs = 0; rs < 4; ++rs) {
      const int R = 32 * rs + 8 * q + tq;
      bf16x8 xb[CB];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int col = w * (KP0 / 4) + 16 * cb + 4 * tp;
        xb[cb] = sm_tr(smem + oX + sm_xoff(R, col, PITCH), smem + oX + sm_xoff(R + 4, col, PITCH));
      }
#pragma unroll
      for (int hb = 0; hb < 4; ++hb)
        if (hb < nb1) {
          const bf16x8 da = sm_tr(smem + oD1 + sm_toff(R, 16 * hb + 4 * tp), smem + oD1 + sm_toff(R + 4, 16 * hb + 4 * tp));
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc1[hb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, xb[cb], acc1[hb][cb], 0, 0, 0);
        }
      if (TWO && w < nb1) {
        const bf16x8 hb_ = sm_tr(smem + oH1 + sm_toff(R, 16 * w + 4 * tp), smem + oH1 + sm_toff(R + 4, 16 * w + 4 * tp));
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
          if (jb < nb2) {
            const bf16x8 da = sm_tr(smem + oD2 + sm_toff(R, 16 * jb + 4 * tp), smem + oD2 + sm_toff(R + 4, 16 * jb + 4 * tp));
            acc2[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, hb_, acc2[jb], 0, 0, 0);
          }
      }
    }
    __syncthreads();                 // the tiles are free for the next forward
  }
  if (!TRAIN) return;

  // ---- the block's slab row, laid out like the flat parameters: W1 [h1][KP0], (W2 [h2][128],) Wo [128]
  float* out = p.slab + (size_t)blockIdx.x * p.numel;
#pragma unroll
  for (int hb = 0; hb < 4; ++hb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int h = 16 * hb + 4 * q + i;
        if (h < p.h1) out[(size_t)h * KP0 + w * (KP0 / 4) + 16 * cb + lr] = acc1[hb][cb][i];
      }
  const long off2 = (long)p.h1 * KP0;
  if (TWO && 16 * w + lr < p.h1)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * jb + 4 * q + i;
        if (j < p.h2) out[off2 + (long)j * SM_KU + 16 * w + lr] = acc2[jb][i];
      }
  // per-wave partials through LDS (the X tile is free after the loop's last barrier), summed in
  // wave order
  float* sg = (float*)(smem + oX);             // [4][64] output-weight gradient
  float* sb = sg + 256;                        // [4][64] layer-2 bias gradient
  float* so = sb + 256;                        // [4] output bias gradient
  double* se = (double*)(so + 4);              // [4][2] error, weight
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float g = gwo[nb][i], b = gb2[nb][i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) { g += __shfl_xor(g, o, 64); b += __shfl_xor(b, o, 64); }
      if (lr == 0) { sg[w * 64 + 16 * nb + 4 * q + i] = g; sb[w * 64 + 16 * nb + 4 * q + i] = b; }
    }
  const float go = wave_sum(q == 0 ? gbo : 0.f);
  esum = wave_sum_d(esum);
  wsum = wave_sum_d(wsum);
  if (lane == 0) { so[w] = go; se[2 * w] = esum; se[2 * w + 1] = wsum; }
  __syncthreads();
  if (tid < SM_KU) {
    float v = 0.f;
    if (tid < nvl) v = sg[tid] + sg[64 + tid] + sg[128 + tid] + sg[192 + tid];
    else if (tid == nvl) v = so[0] + so[1] + so[2] + so[3];
    out[p.numel - SM_KU + tid] = v;
  }
  if (TWO) {                                   // W2 columns h1 (bias) .. 127 (padding)
    const int rest = SM_KU - p.h1;
    for (int idx = tid; idx < p.h2 * rest; idx += SM_T) {
      const int j = idx / rest, c = p.h1 + idx % rest;
      out[off2 + (long)j * SM_KU + c] = c == p.h1 ? sb[j] + sb[64 + j] + sb[128 + j] + sb[192 + j] : 0.f;
    }
  }
  if (tid == 0) {
    p.err_slab[2 * blockIdx.x] = se[0] + se[2] + se[4] + se[6];
    p.err_slab[2 * blockIdx.x + 1] = se[1] + se[3] + se[5] + se[7];
  }
}

// ---- the wide variant: kp0 = 384 or 512 on a 64-row tile -------------------------------------
// W1 and the X tile grow with kp0, so the tile shrinks to 64 rows: at kp0 = 512 W1 and X take
// 64 KiB each.  The algorithm, the fragment layouts and the swizzles are those of mlp_small_kernel
// (sm_xoff's and W1's XORs touch only the low 4 bits of a chunk index, and both pitches hold a
// whole number of 16-chunk groups); what differs:
//   split   4 waves, wave w owns the ONE 16-row strip [16 w, 16 w + 16) of the tile: xf[KS] is 64
//           registers at KS = 16, dW1's slice [64][kp0 / 4] 128 accumulator registers, every other
//           per-row value half of the 128-row kernel's.  8 waves with kp0 / 8 column slices would
//           halve the accumulators, but the transposed forward needs all of a row's nodes in one
//           wave: with 64 rows only 4 waves have a strip, and the other 4 would idle through the
//           forward (or the strips shrink to 8 rows, half-empty MFMAs).  The price of one strip per
//           wave is that a W1 fragment read feeds one MFMA, not two.
//   LDS     kp0 = 512, two layers: W1 [0, 64K), W2 [64K, 72K), X tile [72K, 136K), D1 [136K, 144K),
//           H1 [144K, 152K), D2 [152K, 160K): exactly the CU's 160 KiB.  The fp32 output weights,
//           the output bias and the layer-2 biases a lane needs (16 + 1 + 16 values, they depend
//           on lane >> 4 only) live in registers, which is what makes that build fit; every wide
//           build does the same.  One-layer builds hold no W2, H1 and D2.
//   loads   xf is free once the layer-1 loop has used it, so the next tile's rows are requested
//           there and land during layer 2, the backward row math and the wgrad (the 128-row kernel
//           has no registers for that and requests them after the first barrier).
//   wgrad   two 32-row MFMA steps per tile instead of four; the D fragments are held and the X
//           fragments stream, which keeps the two-layer kp0 = 512 build out of scratch.
//   VALU    the activation id is switched on once per 16 values (sw_with_act), not once per value:
//           the counters showed 2400 VALU instructions and 380 branches per strip against 96 MFMAs.
constexpr int SW_TILE = 64;        // rows per block tile (16 per wave)
constexpr int SW_TILE_B = SW_TILE * 64 * 2;   // one [64][64] bf16 tile

__host__ __device__ constexpr int sw_lds_bytes(int kp0, bool two, bool train) {
  return 64 * kp0 * 2 + (two ? 8192 : 0) + (train ? SW_TILE * kp0 * 2 + (two ? 3 : 1) * SW_TILE_B : 0);
}

// f(integral constant of the activation id): ONE switch for a strip's 16 values.  The id is uniform,
// but act_fwd / act_deriv_out switch per value: about 370 scalar branches per 16-row strip, a
// quarter of a wave's cycles with one wave per SIMD.
template <typename F>
__device__ __forceinline__ void sw_with_act(int act, F&& f) {
  switch (act) {
    case ACT_SIGMOID: f(std::integral_constant<int, ACT_SIGMOID>{}); break;
    case ACT_TANH: f(std::integral_constant<int, ACT_TANH>{}); break;
    case ACT_LINEAR: f(std::integral_constant<int, ACT_LINEAR>{}); break;
    case ACT_RELU: f(std::integral_constant<int, ACT_RELU>{}); break;
    case ACT_LEAKYRELU: f(std::integral_constant<int, ACT_LEAKYRELU>{}); break;
    case ACT_LOG: f(std::integral_constant<int, ACT_LOG>{}); break;
    case ACT_LEAKYRELU_TF: f(std::integral_constant<int, ACT_LEAKYRELU_TF>{}); break;
  }
}

template <int KS, bool TWO, bool TRAIN>
__global__ __launch_bounds__(SM_T) void mlp_small_wide_kernel(SmallArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KP0 = 32 * KS, PITCH = KP0 * 2, CB = KS / 2;
  constexpr int oW1 = 0, oW2 = 64 * PITCH, oX = oW2 + (TWO ? 8192 : 0), oD1 = oX + SW_TILE * PITCH,
                oH1 = oD1 + SW_TILE_B, oD2 = oH1 + SW_TILE_B;
  static_assert(sw_lds_bytes(KP0, TWO, true) <= 160 * 1024, "LDS budget");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane & 15, q = lane >> 4;
  const int nb1 = (p.h1 + 15) >> 4, nb2 = TWO ? (p.h2 + 15) >> 4 : 0;
  const int nvl = TWO ? p.h2 : p.h1, nbl = TWO ? nb2 : nb1;     // the last hidden layer
  const int actl = TWO ? p.act2 : p.act1;
  const float flatl = TWO ? p.flat2 : p.flat1;

  // ---- weights -> LDS, once per block (rows / columns past the real widths are zero)
  for (int idx = tid; idx < 64 * (KP0 / 8); idx += SM_T) {
    const int h = idx / (KP0 / 8), c = idx % (KP0 / 8);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (h < p.h1) v = *(const uint4*)(p.W1 + (size_t)h * KP0 + c * 8);
    *(uint4*)(smem + oW1 + h * PITCH + ((c ^ (h & 15)) << 4)) = v;
  }
  if (TWO)
    for (int idx = tid; idx < 64 * 64; idx += SM_T) {
      const int j = idx >> 6, i = idx & 63;
      ((bf16_t*)(smem + oW2))[idx] = (j < p.h2 && i < p.h1) ? p.W2[(size_t)j * SM_KU + i] : (bf16_t)0;
    }
  // the lane's nodes 16 nb + 4 q + i: output weights, layer-2 biases; the output bias
  float wo[4][4];
  uint2 b2[4];                     // bf16 as stored, 4 to a register pair
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    unsigned b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * nb + 4 * q + i;
      wo[nb][i] = c < nvl ? p.Wo[c] : 0.f;
      b[i] = (TWO && c < p.h2) ? (unsigned short)p.W2[(size_t)c * SM_KU + p.h1] : 0u;
    }
    b2[nb] = make_uint2(b[0] | b[1] << 16, b[2] | b[3] << 16);
  }
  const float bo = p.Wo[nvl];
  __syncthreads();

  uint4 xf[KS];                    // the wave's 16 rows as MFMA fragments: row lr, k 32 ks + 8 q ..
  float yn, sn;                    // the loaded tile's target and row weight
  auto load_x = [&](int tile) __attribute__((always_inline)) {
    const long row = (long)tile * SW_TILE + 16 * w + lr;
    const bool ok = row < p.M;
    const bf16_t* src = p.X + row * p.ldx + 8 * q;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xf[ks] = ok ? *(const uint4*)(src + 32 * ks) : make_uint4(0, 0, 0, 0);
    yn = (TRAIN && ok) ? p.Y[row] : 0.f;
    sn = (TRAIN && ok && p.S) ? p.S[row] : 1.f;
  };

  f32x4 acc1[4][CB], acc2[4];      // dW1 [h block][column block of the wave's slice], dW2 [j block]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CB; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float gwo[4][4], gb2[4][4], gbo = 0.f;   // output-weight / layer-2 bias gradient partials of the lane's row
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) gwo[i][j] = gb2[i][j] = 0.f;
  double esum = 0.0, wsum = 0.0;

  load_x(blockIdx.x);
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    // The swizzled LDS addresses are XORs of lane bits and constants: loop invariants the compiler
    // would keep in ~60 registers across the tiles, next to dW1's 128 and xf's 64.  The lane index
    // passes through an empty asm here and before the wgrad, so each phase recomputes its own.
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int lr = ln & 15, q = ln >> 4;
    const float yv = yn, sv = sn;
    // activation, zero padding, bf16 rounding (where the layer kernels round)
    auto activate = [&](const f32x4 (&z)[4], uint2 (&pk)[4], int nb_, int nv, int act) __attribute__((always_inline)) {
      sw_with_act(act, [&](auto A) __attribute__((always_inline)) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
          float a[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            a[i] = (nb < nb_ && 16 * nb + 4 * q + i < nv) ? act_fwd(decltype(A)::value, z[nb][i]) : 0.f;
          pk[nb] = make_uint2(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]));
        }
      });
    };
    auto put_tile = [&](int off, const uint2 (&v)[4], int nb_) __attribute__((always_inline)) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        if (nb < nb_) *(uint2*)(smem + off + sm_toff(16 * w + lr, 16 * nb + 4 * q)) = v[nb];
    };

    // ---- layer 1: Z1^T = W1 X^T (the bias rides in X's 1-column), the X tile goes to LDS
    f32x4 z1[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) z1[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (TRAIN) *(uint4*)(smem + oX + sm_xoff(16 * w + lr, 32 * ks + 8 * q, PITCH)) = xf[ks];
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
        if (nb < nb1) {
          const bf16x8 wf = *(const bf16x8*)(smem + oW1 + (16 * nb + lr) * PITCH + (((4 * ks + q) ^ lr) << 4));
          z1[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, __builtin_bit_cast(bf16x8, xf[ks]), z1[nb], 0, 0, 0);
        }
    }
    load_x(tile + gridDim.x);        // xf is free: the next tile's rows land during the rest of this one
    uint2 pk1[4], pk2[4];
    activate(z1, pk1, nb1, p.h1, p.act1);
    if (TWO) {
      // ---- layer 2: Z2^T = W2 H1^T + b2; the packed H1 blocks 2 ks, 2 ks + 1 are the B fragment
      f32x4 z2[4];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        float b[4];
        sm_unpk(b2[jb], b);
        z2[jb] = f32x4{b[0], b[1], b[2], b[3]};
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        if (2 * ks < nb1) {
#pragma unroll
          for (int jb = 0; jb < 4; ++jb)
            if (jb < nb2) {
              const char* wr = smem + oW2 + (16 * jb + lr) * 128 + (32 * ks + 4 * q) * 2;
              const bf16x8 wf = sm_join(*(const uint2*)wr, *(const uint2*)(wr + 32));
              z2[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, sm_join(pk1[2 * ks], pk1[2 * ks + 1]), z2[jb], 0, 0, 0);
            }
        }
      activate(z2, pk2, nb2, p.h2, p.act2);
    }
    const uint2 (&pkl)[4] = TWO ? pk2 : pk1;

    // ---- output neuron, loss, output delta: every lane of a row's 4 holds the same values
    float zo = 0.f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
      if (nb < nbl) {
        float h[4];
        sm_unpk(pkl[nb], h);
#pragma unroll
        for (int i = 0; i < 4; ++i) zo += h[i] * wo[nb][i];
      }
    zo += __shfl_xor(zo, 16, 64);
    zo += __shfl_xor(zo, 32, 64);
    zo += bo;
    const long row = (long)tile * SW_TILE + 16 * w + lr;
    const bool valid = row < p.M;
    const float a = act_fwd(p.out_act, zo);
    if (!TRAIN) {
      if (valid && q == 0) p.P[row] = a;
      continue;
    }
    float dl, contrib;
    out_loss_delta(p.out_act, p.loss, true, p.flat_out, zo, a, yv, sv, dl, contrib);
    if (!valid) dl = 0.f;
    if (valid && q == 0) { esum += contrib; wsum += sv; }
    gbo += dl;

    // ---- deltas of the last hidden layer D = dl * Wo * (f'(H) + flat), output-weight gradient
    uint2 dkl[4];
    sw_with_act(actl, [&](auto A) __attribute__((always_inline)) {
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        float h[4], d[4];
        sm_unpk(pkl[nb], h);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          d[i] = (nb < nbl && 16 * nb + 4 * q + i < nvl)
                     ? dl * wo[nb][i] * (act_deriv_out(decltype(A)::value, h[i]) + flatl) : 0.f;
          gwo[nb][i] += dl * h[i];
          if (TWO) gb2[nb][i] += d[i];
        }
        dkl[nb] = make_uint2(pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3]));
      }
    });
    if (TWO) {
      // ---- dgrad: D1^T = (W2^T D2^T) * (f'(H1) + flat1); W2^T fragments by transposed reads
      f32x4 b1[4];
#pragma unroll
      for (int ib = 0; ib < 4; ++ib) b1[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        if (2 * ks < nb2) {
#pragma unroll
          for (int ib = 0; ib < 4; ++ib)
            if (ib < nb1) {
              const char* wr = smem + oW2 + (32 * ks + 4 * q + (lr >> 2)) * 128 + (16 * ib + 4 * (ln & 3)) * 2;
              b1[ib] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sm_tr(wr, wr + 16 * 128),
                                                               sm_join(dkl[2 * ks], dkl[2 * ks + 1]), b1[ib], 0, 0, 0);
            }
        }
      uint2 dk1[4];
      sw_with_act(p.act1, [&](auto A) __attribute__((always_inline)) {
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
          float h[4], d[4];
          sm_unpk(pk1[ib], h);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            d[i] = (ib < nb1 && 16 * ib + 4 * q + i < p.h1)
                       ? b1[ib][i] * (act_deriv_out(decltype(A)::value, h[i]) + p.flat1) : 0.f;
          dk1[ib] = make_uint2(pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3]));
        }
      });
      put_tile(oD1, dk1, nb1);
      put_tile(oH1, pk1, nb1);
      put_tile(oD2, dkl, nb2);
    } else {
      put_tile(oD1, dkl, nb1);
    }
    __syncthreads();

    // ---- wgrad over the tile's 64 rows, 32 per MFMA: dW1 slice [64][KP0 / 4], dW2 slice [64][16]
    int lw = lane;
    asm volatile("" : "+v"(lw));
    const int tp = lw & 3;
#pragma unroll
    for (int rs = 0; rs < SW_TILE / 32; ++rs) {
      const int R = 32 * rs + 8 * (lw >> 4) + ((lw >> 2) & 3);
      bf16x8 da[4];                  // the D fragments stay, the X fragments stream (4 live registers, not 4 CB)
#pragma unroll
      for (int hb = 0; hb < 4; ++hb)
        if (hb < nb1)
          da[hb] = sm_tr(smem + oD1 + sm_toff(R, 16 * hb + 4 * tp), smem + oD1 + sm_toff(R + 4, 16 * hb + 4 * tp));
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) {
        const int col = w * (KP0 / 4) + 16 * cb + 4 * tp;
        const bf16x8 xb = sm_tr(smem + oX + sm_xoff(R, col, PITCH), smem + oX + sm_xoff(R + 4, col, PITCH));
#pragma unroll
        for (int hb = 0; hb < 4; ++hb)
          if (hb < nb1) acc1[hb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da[hb], xb, acc1[hb][cb], 0, 0, 0);
      }
      if (TWO && w < nb1) {
        const bf16x8 hb_ = sm_tr(smem + oH1 + sm_toff(R, 16 * w + 4 * tp), smem + oH1 + sm_toff(R + 4, 16 * w + 4 * tp));
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
          if (jb < nb2) {
            const bf16x8 da = sm_tr(smem + oD2 + sm_toff(R, 16 * jb + 4 * tp), smem + oD2 + sm_toff(R + 4, 16 * jb + 4 * tp));
            acc2[jb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(da, hb_, acc2[jb], 0, 0, 0);
          }
      }
    }
    __syncthreads();                 // the tiles are free for the next forward
  }
  if (!TRAIN) return;

  // ---- the block's slab row, laid out like the flat parameters: W1 [h1][KP0], (W2 [h2][128],) Wo [128]
  float* out = p.slab + (size_t)blockIdx.x * p.numel;
#pragma unroll
  for (int hb = 0; hb < 4; ++hb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int h = 16 * hb + 4 * q + i;
        if (h < p.h1) out[(size_t)h * KP0 + w * (KP0 / 4) + 16 * cb + lr] = acc1[hb][cb][i];
      }
  const long off2 = (long)p.h1 * KP0;
  if (TWO && 16 * w + lr < p.h1)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = 16 * jb + 4 * q + i;
        if (j < p.h2) out[off2 + (long)j * SM_KU + 16 * w + lr] = acc2[jb][i];
      }
  // per-wave partials through LDS (the X tile is free after the loop's last barrier), summed in
  // wave order
  float* sg = (float*)(smem + oX);             // [4][64] output-weight gradient
  float* sb = sg + 256;                        // [4][64] layer-2 bias gradient
  float* so = sb + 256;                        // [4] output bias gradient
  double* se = (double*)(so + 4);              // [4][2] error, weight
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float g = gwo[nb][i], b = gb2[nb][i];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) { g += __shfl_xor(g, o, 64); b += __shfl_xor(b, o, 64); }
      if (lr == 0) { sg[w * 64 + 16 * nb + 4 * q + i] = g; sb[w * 64 + 16 * nb + 4 * q + i] = b; }
    }
  const float go = wave_sum(q == 0 ? gbo : 0.f);
  esum = wave_sum_d(esum);
  wsum = wave_sum_d(wsum);
  if (lane == 0) { so[w] = go; se[2 * w] = esum; se[2 * w + 1] = wsum; }
  __syncthreads();
  if (tid < SM_KU) {
    float v = 0.f;
    if (tid < nvl) v = sg[tid] + sg[64 + tid] + sg[128 + tid] + sg[192 + tid];
    else if (tid == nvl) v = so[0] + so[1] + so[2] + so[3];
    out[p.numel - SM_KU + tid] = v;
  }
  if (TWO) {                                   // W2 columns h1 (bias) .. 127 (padding)
    const int rest = SM_KU - p.h1;
    for (int idx = tid; idx < p.h2 * rest; idx += SM_T) {
      const int j = idx / rest, c = p.h1 + idx % rest;
      out[off2 + (long)j * SM_KU + c] = c == p.h1 ? sb[j] + sb[64 + j] + sb[128 + j] + sb[192 + j] : 0.f;
    }
  }
  if (tid == 0) {
    p.err_slab[2 * blockIdx.x] = se[0] + se[2] + se[4] + se[6];
    p.err_slab[2 * blockIdx.x + 1] = se[1] + se[3] + se[5] + se[7];
  }
}

// grad[c] += sum_b slab[b][c], err += sum_b err_slab[b], both in block order
__global__ __launch_bounds__(256) void small_reduce_kernel(const float* slab, const double* err_slab, int G, long numel,
                                                           float* grad, double* err) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c < numel) {
    float s = 0.f;
    for (int b = 0; b < G; ++b) s += slab[(size_t)b * numel + c];
    grad[c] += s;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    double e = 0.0;
    for (int b = 0; b < G; ++b) e += err_slab[2 * b + threadIdx.x];
    err[threadIdx.x] += e;
  }
}

// rows per block tile of the build that takes kp0
int sm_tile(int kp0) { return kp0 <= 256 ? SM_TILE : SW_TILE; }
int sm_tiles(int M, int tile) { return (int)(((long)M + tile - 1) / tile); }

// one block per CU, at most one per tile
int sm_grid(int M, int tile) {
  int dev = 0, ncu = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  const int ntiles = sm_tiles(M, tile);
  return ntiles < ncu ? ntiles : ncu;
}

bool sm_act_ok(int a) { return a == 0 || a == 1 || a == 2 || a == 3 || a == 4 || a == 7 || a == 9; }

bool sm_shape_ok(long ldx, int M, int kp0, int h1, int h2, int act1, int act2, int out_act) {
  return M > 0 && (kp0 == 128 || kp0 == 256 || kp0 == 384 || kp0 == 512) && ldx >= kp0 && ldx % 8 == 0 && h1 >= 1 &&
         h1 <= 64 && h2 >= 0 && h2 <= 64 && sm_act_ok(act1) && (h2 == 0 || sm_act_ok(act2)) && out_act >= 0 &&
         out_act <= 9;
}

template <int KS, bool TWO, bool TRAIN>
hipError_t sm_launch(const SmallArgs& p, int grid, hipStream_t stream) {
  constexpr int lds = sm_lds_bytes(32 * KS, TRAIN);
  static const hipError_t attr = hipFuncSetAttribute((const void*)mlp_small_kernel<KS, TWO, TRAIN>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((mlp_small_kernel<KS, TWO, TRAIN>), dim3(grid), dim3(SM_T), lds, stream, p);
  return hipGetLastError();
}

template <int KS, bool TWO, bool TRAIN>
hipError_t sw_launch(const SmallArgs& p, int grid, hipStream_t stream) {
  constexpr int lds = sw_lds_bytes(32 * KS, TWO, TRAIN);
  static const hipError_t attr = hipFuncSetAttribute((const void*)mlp_small_wide_kernel<KS, TWO, TRAIN>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((mlp_small_wide_kernel<KS, TWO, TRAIN>), dim3(grid), dim3(SM_T), lds, stream, p);
  return hipGetLastError();
}

template <bool TRAIN>
hipError_t sm_dispatch(const SmallArgs& p, int kp0, int grid, hipStream_t stream) {
  if (kp0 == 128) return p.h2 ? sm_launch<4, true, TRAIN>(p, grid, stream) : sm_launch<4, false, TRAIN>(p, grid, stream);
  if (kp0 == 384) return p.h2 ? sw_launch<12, true, TRAIN>(p, grid, stream) : sw_launch<12, false, TRAIN>(p, grid, stream);
  if (kp0 == 512) return p.h2 ? sw_launch<16, true, TRAIN>(p, grid, stream) : sw_launch<16, false, TRAIN>(p, grid, stream);
  return p.h2 ? sm_launch<8, true, TRAIN>(p, grid, stream) : sm_launch<8, false, TRAIN>(p, grid, stream);
}

}  // namespace

// Rows of the slabs shifu_mlp_small_step writes for an M-row chunk (slab [rows][numel] fp32,
// err_slab [rows][2] fp64): one per block of the persistent grid.  The 64-row builds have the
// larger grid, so their count covers every build.
SHIFU_API int shifu_mlp_small_rows(int M) { return M > 0 ? sm_grid(M, SW_TILE) : 0; }

// Whole gradient step of an M-row chunk of a small MLP: grad [numel] += the chunk's gradient in the
// flat parameter layout (W1 [h1][kp0], W2 [h2][128] when h2 > 0, Wo [128]), err[2] += (error,
// weight sum).  Returns -1 for a shape it does not take.
SHIFU_API int shifu_mlp_small_step(const void* X, long ldx, const void* W1, const void* W2, const float* Wo,
                                   const float* Y, const float* S, float* slab, double* err_slab, float* grad,
                                   double* err, long numel, int M, int kp0, int h1, int h2, int act1, int act2,
                                   int out_act, int loss, float flat1, float flat2, float flat_out,
                                   hipStream_t stream) {
  if (!sm_shape_ok(ldx, M, kp0, h1, h2, act1, act2, out_act) || (h2 > 0 && W2 == nullptr) || loss < 0 || loss > 5 ||
      numel != (long)h1 * kp0 + (long)h2 * SM_KU + SM_KU)
    return -1;
  const int tile = sm_tile(kp0), grid = sm_grid(M, tile);
  SmallArgs p{(const bf16_t*)X, ldx, (const bf16_t*)W1, (const bf16_t*)W2, Wo, Y, S, slab, err_slab, nullptr, numel,
              M, sm_tiles(M, tile), h1, h2, act1, act2, out_act, loss, flat1, flat2, flat_out};
  hipError_t e = sm_dispatch<true>(p, kp0, grid, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(small_reduce_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, stream, slab, err_slab,
                     grid, numel, grad, err);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

// Forward only: P [M] = the network's output for every row.
SHIFU_API int shifu_mlp_small_forward(const void* X, long ldx, const void* W1, const void* W2, const float* Wo,
                                      float* P, int M, int kp0, int h1, int h2, int act1, int act2, int out_act,
                                      hipStream_t stream) {
  if (!sm_shape_ok(ldx, M, kp0, h1, h2, act1, act2, out_act) || (h2 > 0 && W2 == nullptr) || P == nullptr) return -1;
  SmallArgs p{(const bf16_t*)X, ldx, (const bf16_t*)W1, (const bf16_t*)W2, Wo, nullptr, nullptr, nullptr, nullptr, P, 0,
              M, sm_tiles(M, sm_tile(kp0)), h1, h2, act1, act2, out_act, 0, 0.f, 0.f, 0.f};
  const hipError_t e = sm_dispatch<false>(p, kp0, sm_grid(M, sm_tile(kp0)), stream);
  return e == hipSuccess ? 0 : (int)e;
}
