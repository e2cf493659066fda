// GPU dictionary encoder for the categorical columns of a parsed text block (K0c) for MI355X
// (gfx950): the field bounds csv_parse_kernel hands back (moffs) -> int32 codes per row in HBM and
// a per-column dictionary, identical to what the host parser (runtime/csrc/csv_parser.cpp) builds
// from the same bytes.
//
// Host rules reproduced here (csv_parser.cpp `general`): a field is trimmed of ' ', '\t', '\r' on
// both sides; the trimmed bytes are compared with the trimmed missing tokens (the empty string is
// one of them when the token list holds it or is empty) -> code -1; every other value gets the
// id of its dictionary entry.  Dictionary order, confirmed in shifu_csv_fill: every thread chunk
// lists its values in first-seen order and the chunks (contiguous row ranges, in row order) are
// merged in chunk order, a value already seen keeping its id -- so entry i is the value whose
// FIRST APPEARANCE (smallest row of the block) is the i-th smallest.  That is independent of the
// thread count, and it is what the rank step below computes.
//
// Launches (one C entry point, the caller's stream):
//   cat_init     clears the tables, the first-row bitmap and the overflow flags (a kernel, so the
//                entry point is safe to record anywhere a memset is not).
//   cat_insert   workgroup = 4096 consecutive rows of ONE categorical column (grid.y = column;
//                moffs is column-major, so a wave's 64 lanes read 64 consecutive bounds).  A lane
//                owns one field: trim, missing tokens, 64-bit hash of the bytes from 8-byte words
//                (tail masked; reads stay below L + 8).  Lanes of a wave with the same hash are
//                merged first (leader loop: read the first open lane's hash, ballot the equal
//                lanes; rows rise with the lane, so the leader holds the group's smallest row).
//                Leaders go to a 256-entry LDS front table {hash, min row} (64-bit LDS CAS on the
//                hash, LDS atomicMin on the row, 8 probes); a low-cardinality column -- the common
//                case -- therefore costs one HBM insert per distinct value and WORKGROUP, not a
//                machine's worth of atomics on three addresses.  A full front table sends the
//                leader straight to HBM.  At the end each occupied LDS entry is flushed once.
//                HBM table per column: open addressing, power-of-two `cap`, keys u64 (0 = empty),
//                first row int32: 64-bit CAS claims the key, atomicMin keeps the smallest row.
//                At most CAT_PROBE probes: a table that is (nearly) full raises the column's
//                overflow flag instead of scanning `cap` slots per field.
//   cat_mark / cat_scan / cat_ids   the rank step.  Each entry's first row is unique within its
//                column (a row has one field per column), so the order is a rank over rows: set
//                bit first_row of a per-column bitmap, scan the word popcounts (one workgroup per
//                column), id = words before + bits below.  No sort, no limit below `cap`.  cat_ids
//                also writes the distinct list {trimmed offset, length} of the first-row field,
//                compacted over the columns (column c's entries start at sum(counts[:c])), so
//                the host copies back only the used part.
//   cat_codes    a lane looks its field's hash up and writes codes[column][row] (-1 missing;
//                blank lines get -1 and are dropped by the caller with the numeric rows).
//
// Deviations from the first design, and why:
//   * The entry holds {hash, first_row} only.  The representative is DEFINED as the field at
//     first_row, whose bounds are in moffs; storing rep_offset / rep_len next to an atomicMin'd
//     row would need a 128-bit update to stay consistent.
//   * Exactness is checked in cat_codes, not at insert time: during the insert the representative
//     still moves, afterwards it is final.  Every field whose row is not first_row compares its
//     trimmed bytes with the representative's; any mismatch (a true hash collision) raises the
//     column's overflow flag.  If no field of a column mismatches, its hash classes are its
//     string classes, so codes and dictionary are exact.  No chaining.
//   * cat_codes has no LDS table: its lookups are read-only, the hot entries of a low-cardinality
//     column sit in every CU's vector L1, and equal lanes read the same address (one fetch).  The
//     LDS table exists to absorb atomics, and this pass has none.
//   * One column per workgroup rather than a tile of columns: coalesced bounds reads and a single
//     LDS table; grid.y supplies the column parallelism.
// `hash_bits` masks the hash before use (64 in production; small values make collisions on
// purpose in the tests).  A flagged column is re-done on the host by the caller, for that column
// and block only.  Rows flagged blank or with a wrong field count are never dereferenced (their
// bounds may be unwritten), and bounds outside [0, L] raise the flag instead of being read.
#include "common.h"
#include <limits.h>
#include <string.h>

#define CHECK_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)

namespace {

constexpr int CAT_MAXTOK = 8;
constexpr int CAT_TOKLEN = 16;
constexpr int CAT_ROWS = 4096;                // rows of one column per insert workgroup
constexpr int CAT_LDS = 256;                  // LDS front-table entries
constexpr int CAT_LDS_PROBE = 8;
constexpr int CAT_PROBE = 64;                 // HBM probes before the column overflows
constexpr int CAT_CODE_ROWS = 1024;           // rows per cat_codes workgroup

typedef unsigned long long u64;

struct CatArgs {
  const uint8_t* buf; long L;                 // block bytes (>= 64 readable bytes past L)
  const int* moffs;                           // [n_host][nl][2] raw field bounds
  const int* lflags;                          // [nl]: 1 blank, 2 field count != ncols
  const int* ccol;                            // [ncat] moffs row of each categorical column
  long nl; int ncat;
  int cap; u64 hmask;
  u64* keys; int* frow; int* ids;             // [ncat][cap]
  unsigned* bits; int* wbase; long nw;        // [ncat][nw]: first-row bitmap, words-before counts
  int* codes; long ldc;                       // [ncat][ldc]
  int* dl;                                    // distinct list [sum counts][2] = {offset, length}
  int* counts; int* flags;                    // [ncat]
  int empty_missing;
  int ntok;
  int toklen[CAT_MAXTOK];
  unsigned char tok[CAT_MAXTOK][CAT_TOKLEN];
};

__device__ __forceinline__ bool cat_ws(unsigned c) { return c == ' ' || c == '\t' || c == '\r'; }

__device__ __forceinline__ u64 cat_word(const uint8_t* p, int left) {   // bytes [0, min(left, 8)) of p
  u64 w;
  __builtin_memcpy(&w, p, 8);
  return left < 8 ? w & ((1ull << (8 * left)) - 1) : w;
}

struct CatField { int a, n; bool live; };     // trimmed start, length; live: a dictionary value

// the trimmed field of (column, row); live = false for blank / ragged rows and missing values
__device__ CatField cat_field(const CatArgs& A, int col, long row, bool check_missing) {
  CatField f{0, 0, false};
  if (A.lflags[row] & 3) return f;
  const int* o = A.moffs + 2 * ((long)A.ccol[col] * A.nl + row);
  long a = o[0], b = o[1];
  if (a < 0 || b < a || b > A.L) { A.flags[col] = 1; return f; }
  const uint8_t* p = A.buf;
  while (a < b && cat_ws(p[a])) ++a;
  while (b > a && cat_ws(p[b - 1])) --b;
  f.a = (int)a; f.n = (int)(b - a); f.live = true;
  if (!check_missing) return f;
  if (f.n == 0) { f.live = !A.empty_missing; return f; }
  for (int t = 0; t < A.ntok; ++t) {
    if (A.toklen[t] != f.n) continue;
    bool eq = true;
    for (int i = 0; i < f.n && eq; ++i) eq = p[a + i] == A.tok[t][i];
    if (eq) { f.live = false; return f; }
  }
  return f;
}

__device__ u64 cat_hash(const uint8_t* p, int n, u64 mask) {
  u64 h = 0x9E3779B97F4A7C15ull ^ ((u64)n * 0xFF51AFD7ED558CCDull);
  for (int i = 0; i < n; i += 8) {
    h = (h ^ cat_word(p + i, n - i)) * 0x9FB21C651E98DF25ull;
    h ^= h >> 32;
  }
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  h &= mask;
  return h ? h : 1;                           // 0 marks an empty slot
}

__device__ void cat_hbm_insert(const CatArgs& A, int col, u64 h, int row) {
  u64* keys = A.keys + (long)col * A.cap;
  int* frow = A.frow + (long)col * A.cap;
  const unsigned m = (unsigned)A.cap - 1;
  const unsigned s = (unsigned)h & m;
  const int np = A.cap < CAT_PROBE ? A.cap : CAT_PROBE;
  for (int p = 0; p < np; ++p) {
    const unsigned i = (s + p) & m;
    u64 old = __atomic_load_n(&keys[i], __ATOMIC_RELAXED);
    if (old == 0) old = atomicCAS(&keys[i], 0ull, h);
    if (old == 0 || old == h) { atomicMin(&frow[i], row); return; }
  }
  A.flags[col] = 1;
}

__global__ __launch_bounds__(256) void cat_init_kernel(CatArgs A) {
  const long stride = (long)gridDim.x * 256;
  const long ne = (long)A.ncat * A.cap, nb = (long)A.ncat * A.nw;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < ne; i += stride) { A.keys[i] = 0; A.frow[i] = INT_MAX; }
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nb; i += stride) A.bits[i] = 0;
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < A.ncat; i += 256) { A.flags[i] = 0; A.counts[i] = 0; }
}

__global__ __launch_bounds__(256) void cat_insert_kernel(CatArgs A) {
  __shared__ u64 lk[CAT_LDS];
  __shared__ int lr[CAT_LDS];
  const int t = threadIdx.x, lane = t & 63, col = blockIdx.y;
  lk[t] = 0;
  lr[t] = INT_MAX;
  __syncthreads();
  const long r0 = (long)blockIdx.x * CAT_ROWS;
  for (int it = 0; it < CAT_ROWS / 256; ++it) {
    const long row = r0 + it * 256 + t;       // row - lane is wave-uniform: whole waves skip together
    if (row - lane >= A.nl) break;
    bool act = false;
    u64 h = 0;
    if (row < A.nl) {
      const CatField f = cat_field(A, col, row, true);
      act = f.live;
      if (act) h = cat_hash(A.buf + f.a, f.n, A.hmask);
    }
    // merge the wave's equal hashes: the lowest lane of a group leads it (and has its smallest row)
    u64 open = __ballot(act);
    bool lead = false;
    while (open) {
      const int l = __ffsll((long long)open) - 1;
      const u64 lh = __shfl(h, l, 64);
      open &= ~__ballot(act && h == lh);
      lead |= lane == l;
    }
    if (lead) {
      const unsigned s = (unsigned)((h * 0x9E3779B97F4A7C15ull) >> 56);
      bool done = false;
      for (int p = 0; p < CAT_LDS_PROBE && !done; ++p) {
        const unsigned i = (s + p) & (CAT_LDS - 1);
        u64 old = __atomic_load_n(&lk[i], __ATOMIC_RELAXED);
        if (old == 0) old = atomicCAS(&lk[i], 0ull, h);
        if (old == 0 || old == h) { atomicMin(&lr[i], (int)row); done = true; }
      }
      if (!done) cat_hbm_insert(A, col, h, (int)row);
    }
  }
  __syncthreads();
  if (lk[t]) cat_hbm_insert(A, col, lk[t], lr[t]);
}

__global__ __launch_bounds__(256) void cat_mark_kernel(CatArgs A) {
  const int col = blockIdx.y;
  const long i = (long)col * A.cap + (long)blockIdx.x * 256 + threadIdx.x;
  if (!A.keys[i]) return;
  const int r = A.frow[i];
  if (r < 0 || r >= A.nl) { A.flags[col] = 1; return; }
  atomicOr(&A.bits[(long)col * A.nw + (r >> 5)], 1u << (r & 31));
}

// per column: wbase[w] = set bits in the words before w, counts[col] = all set bits
__global__ __launch_bounds__(256) void cat_scan_kernel(CatArgs A) {
  __shared__ int sh[256];
  const int t = threadIdx.x, col = blockIdx.x;
  const unsigned* bits = A.bits + (long)col * A.nw;
  int* wbase = A.wbase + (long)col * A.nw;
  int carry = 0;
  for (long b = 0; b < A.nw; b += 256) {
    const long w = b + t;
    const int v = w < A.nw ? __builtin_popcount(bits[w]) : 0;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int u = t >= o ? sh[t - o] : 0;
      __syncthreads();
      sh[t] += u;
      __syncthreads();
    }
    if (w < A.nw) wbase[w] = carry + sh[t] - v;
    const int tot = sh[255];
    __syncthreads();
    carry += tot;
  }
  if (t == 0) A.counts[col] = carry;
}

__global__ __launch_bounds__(256) void cat_ids_kernel(CatArgs A) {
  __shared__ int sh[256];
  const int t = threadIdx.x, col = blockIdx.y;
  int s = 0;
  for (int j = t; j < col; j += 256) s += A.counts[j];
  sh[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  const long base = sh[0];                    // distinct-list offset of this column
  const long i = (long)col * A.cap + (long)blockIdx.x * 256 + t;
  if (!A.keys[i]) return;
  const int r = A.frow[i];
  if (r < 0 || r >= A.nl) return;             // flagged by cat_mark
  const long w = (long)col * A.nw + (r >> 5);
  const int id = A.wbase[w] + __builtin_popcount(A.bits[w] & ((1u << (r & 31)) - 1));
  A.ids[i] = id;
  const CatField f = cat_field(A, col, r, false);
  A.dl[2 * (base + id)] = f.a;
  A.dl[2 * (base + id) + 1] = f.n;
}

__global__ __launch_bounds__(256) void cat_codes_kernel(CatArgs A) {
  const int col = blockIdx.y;
  const u64* keys = A.keys + (long)col * A.cap;
  const unsigned m = (unsigned)A.cap - 1;
  const int np = A.cap < CAT_PROBE ? A.cap : CAT_PROBE;
  for (int it = 0; it < CAT_CODE_ROWS / 256; ++it) {
    const long row = (long)blockIdx.x * CAT_CODE_ROWS + it * 256 + threadIdx.x;
    if (row >= A.nl) return;
    int code = -1;
    const CatField f = cat_field(A, col, row, true);
    if (f.live) {
      const u64 h = cat_hash(A.buf + f.a, f.n, A.hmask);
      const unsigned s = (unsigned)h & m;
      long e = -1;
      for (int p = 0; p < np; ++p) {
        const unsigned i = (s + p) & m;
        const u64 k = keys[i];
        if (k == h) { e = (long)col * A.cap + i; break; }
        if (k == 0) break;
      }
      if (e < 0) {
        A.flags[col] = 1;                     // the insert overflowed
      } else {
        const int r = A.frow[e];
        code = A.ids[e];
        if (r != row) {                       // exactness: my bytes == the representative's bytes
          const CatField g = (r >= 0 && r < A.nl) ? cat_field(A, col, r, false) : CatField{0, -1, false};
          bool eq = g.n == f.n;
          for (int i = 0; i < f.n && eq; i += 8)
            eq = cat_word(A.buf + f.a + i, f.n - i) == cat_word(A.buf + g.a + i, f.n - i);
          if (!eq) A.flags[col] = 1;          // a true hash collision: this column goes to the host
        }
      }
    }
    A.codes[(long)col * A.ldc + row] = code;
  }
}

inline long cat_align(long b) { return (b + 255) & ~255l; }

}  // namespace

// bytes of the workspace shifu_csv_cat_encode needs for ncat columns, nl lines, table capacity cap
SHIFU_API long shifu_csv_cat_ws_bytes(int ncat, int cap, long nl) {
  const long ne = (long)ncat * cap, nb = (long)ncat * ((nl + 31) / 32);
  return cat_align(ne * 8) + 2 * cat_align(ne * 4) + 2 * cat_align(nb * 4);
}

// buf: the block in HBM (L bytes + >= 64 readable); moffs [n_host][nl][2] / lflags [nl]: what
// shifu_csv_gpu_parse wrote; ccol [ncat]: the moffs row of each categorical column; toks: ntok
// '\0'-separated trimmed missing tokens (each < 16 bytes), empty_missing: the empty field is
// missing too; cap: table slots per column (a power of two in [256, 2^24]); hash_bits in [1, 64];
// ws: 256-B aligned, shifu_csv_cat_ws_bytes.  Out: codes [ncat][ldc] int32 (every line, blank
// ones -1); dl [<= ncat * cap][2] int32 distinct list, column c's entries in dictionary order
// from sum(counts[:c]); counts [ncat]; flags [ncat] (1: redo this column on the host).
SHIFU_API int shifu_csv_cat_encode(const void* buf, long L, const int* moffs, const int* lflags, long nl,
                                   const int* ccol, int ncat, int ntok, const char* toks, int empty_missing,
                                   int cap, int hash_bits, void* ws, int* codes, long ldc, int* dl, int* counts,
                                   int* flags, hipStream_t stream) {
  if (nl <= 0 || ncat <= 0) return 0;
  if (nl >= INT_MAX || ncat > 65535 || ldc < nl || ntok < 0 || ntok > CAT_MAXTOK || cap < 256 ||
      cap > (1 << 24) || (cap & (cap - 1)) || hash_bits < 1 || hash_bits > 64 || ((uintptr_t)ws & 255) ||
      L < 0 || L > (long)INT_MAX)
    return -1;
  CatArgs A{};
  A.buf = (const uint8_t*)buf; A.L = L; A.moffs = moffs; A.lflags = lflags; A.ccol = ccol; A.nl = nl;
  A.ncat = ncat; A.cap = cap; A.hmask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1;
  A.nw = (nl + 31) / 32;
  const long ne = (long)ncat * cap, nb = (long)ncat * A.nw;
  char* w = (char*)ws;
  A.keys = (u64*)w; w += cat_align(ne * 8);
  A.frow = (int*)w; w += cat_align(ne * 4);
  A.ids = (int*)w; w += cat_align(ne * 4);
  A.bits = (unsigned*)w; w += cat_align(nb * 4);
  A.wbase = (int*)w;
  A.codes = codes; A.ldc = ldc; A.dl = dl; A.counts = counts; A.flags = flags;
  A.empty_missing = empty_missing != 0; A.ntok = ntok;
  const char* t = toks;
  for (int i = 0; i < ntok; ++i) {
    const int n = (int)strlen(t);
    if (n == 0 || n >= CAT_TOKLEN) return -1;
    A.toklen[i] = n;
    memcpy(A.tok[i], t, n);
    t += n + 1;
  }
  const unsigned tiles = (unsigned)((nl + CAT_ROWS - 1) / CAT_ROWS);
  const unsigned ctiles = (unsigned)((nl + CAT_CODE_ROWS - 1) / CAT_CODE_ROWS);
  const long init_blocks = (ne + 255) / 256;
  hipLaunchKernelGGL(cat_init_kernel, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(cat_insert_kernel, dim3(tiles, ncat), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(cat_mark_kernel, dim3(cap / 256, ncat), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(cat_scan_kernel, dim3(ncat), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(cat_ids_kernel, dim3(cap / 256, ncat), dim3(256), 0, stream, A);
  hipLaunchKernelGGL(cat_codes_kernel, dim3(ctiles, ncat), dim3(256), 0, stream, A);
  CHECK_HIP(hipGetLastError());
  return 0;
}
