// What gemm_kernels.hip (the dispatcher) shares with the persistent forward engines
// gemm_ring_nt.hip and gemm_strip_nt.hip: the epilogue codes and the engines' C entry points.
#pragma once
#include "common.h"

enum Epi : int { EPI_ACT = 0, EPI_DACT = 1, EPI_STORE = 2,
                 EPI_F32 = 3 };   // fp32 output tile (split-bf16 fp32-accurate products: algos/varsel.py)

// C[m][n] = epilogue( sum_k A[m][k] B[n][k] ): 0 on success, a hipError_t when the launch failed,
// -1 when the shape is not one the engine takes (the caller falls back).  epi: EPI_ACT (activation
// whose derivative is computable from the output: no f'(z) side output) or EPI_STORE (store z).
SHIFU_API int shifu_ring_nt(const void* A, long lda, const void* B, long ldb, int NB, void* C, long ldc, int M,
                            int N, int K, int epi, int act, int n_valid, int bias_col, hipStream_t stream);
SHIFU_API int shifu_strip_nt(const void* A, long lda, const void* B, long ldb, int NB, void* C, long ldc, int M,
                             int N, int K, int epi, int act, int n_valid, int bias_col, hipStream_t stream);
