// knn_csv.hip -- the reference's CSV reader (cpp:154-222, host/csv.h) on the
// device (gfx950): text bytes in HBM -> fp64 rows and int32 labels, bit for
// bit what atof / atoi give the reference.
//
// The reference's token rule (getline on '\n', then getline on ',': every
// segment followed by a comma is a token, possibly empty; a line's last
// segment only if non-empty; ONE running token counter over the whole file)
// is byte-parallel:
//   position p TERMINATES a token iff text[p] == ',', or text[p] == '\n' (or
//   p == bytes, the end of the file) and p > 0 and text[p-1] is neither ','
//   nor '\n';
//   the token begins after the previous ',' or '\n', or at 0.
// So the token index of a terminator is the number of terminators before it.
//
// Three stream-ordered steps, no host wait between them:
//   count    a workgroup owns KNN_CSV_BLOCK_BYTES consecutive positions (the
//            positions run to `bytes` inclusive: the end of the file is one);
//            each lane takes 16 of them per tile with one 16-byte load and the
//            one look-back byte in front of its chunk; terminators per block
//   scan     exclusive scan of the block counts in int64 (one workgroup);
//            the total is the file's token count
//   convert  the same partition; an in-block scan gives each terminator its
//            file-wide index c; the owning lane finds the token's start (in
//            its own 16 bytes, else walking back at most 64 bytes -- a longer
//            token is slow), converts it with csv_fast_atof / csv_fast_atoi
//            (knn_csv_num.h: exact or "slow") and stores by the reference's
//            rule: with labels c % (dim+1) == 0 -> labels[c / (dim+1)], any
//            other -> data[c - c/(dim+1) - 1]; without, data[c].  Tokens at c
//            >= cap are counted only; cells no token reaches are not written.
//            A slow token appends (c, p) to the slow list through one atomic
//            counter, which keeps counting past the list's capacity.
// Geometry: 256 lanes x 16 B = one 4 KiB tile per load instruction per
// workgroup (the widest coalesced access), four tiles per workgroup so the
// block scan's two barriers and the block's count amortise over 16 KiB; a
// 1 GB file is 64 Ki block counts, which the one-workgroup scan walks in 256
// steps.  No LDS beyond the four wave totals, no scratch, no read outside
// [0, bytes).
#include <algorithm>

#include "../../include/knn_amd.h"
#include "knn_csv_num.h"
#include "knn_kernels.h"

namespace knnk {

namespace {

constexpr int kCsvThreads = 256;
constexpr int kCsvWaves = kCsvThreads / 64;
constexpr int kCsvTile = kCsvThreads * 16;
constexpr int kCsvTiles = KNN_CSV_BLOCK_BYTES / kCsvTile;
static_assert(KNN_CSV_BLOCK_BYTES % kCsvTile == 0, "a block is whole tiles");

__device__ inline bool csv_is_delim(unsigned int c) { return c == ',' || c == '\n'; }

// Positions [p0, p0 + 16), p0 a multiple of 16 and <= bytes: bit i of the
// result = position p0 + i terminates a token; *delim: bit i = a ',' or '\n'
// (or the end of the file) stands there.  Positions beyond `bytes` are blank.
__device__ inline unsigned int csv_masks(const unsigned char* __restrict__ text, int64_t bytes,
                                         int64_t p0, unsigned int* delim) {
  unsigned int w[4] = {0, 0, 0, 0};
  if (p0 + 16 <= bytes) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + p0);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t p = p0 + i;
      const unsigned int c = p < bytes ? text[p] : p == bytes ? (unsigned int)'\n' : 0u;
      w[i >> 2] |= c << (8 * (i & 3));
    }
  }
  // the look-back byte (the line in front of position 0 counts as ended)
  const unsigned int prev = p0 == 0 ? (unsigned int)'\n' : text[p0 - 1];
  unsigned int comma = 0, nl = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const unsigned int c = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
    comma |= (unsigned int)(c == ',') << i;
    nl |= (unsigned int)(c == '\n') << i;
  }
  const unsigned int d = comma | nl;
  const unsigned int prevd = ((d << 1) | (unsigned int)csv_is_delim(prev)) & 0xFFFFu;
  *delim = d;
  return comma | (nl & ~prevd);
}

__global__ void __launch_bounds__(kCsvThreads)
csv_count_kernel(const unsigned char* __restrict__ text, int64_t bytes,
                 unsigned int* __restrict__ cnt) {
  __shared__ int wtot[kCsvWaves];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * KNN_CSV_BLOCK_BYTES;
  int n = 0;
#pragma unroll
  for (int j = 0; j < kCsvTiles; ++j) {
    const int64_t p0 = base + (int64_t)j * kCsvTile + tid * 16;
    if (p0 <= bytes) {
      unsigned int delim;
      n += __popc(csv_masks(text, bytes, p0, &delim));
    }
  }
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) wtot[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < kCsvWaves; ++w) s += wtot[w];
    cnt[blockIdx.x] = (unsigned int)s;
  }
}

// one workgroup: base[i] = cnt[0] + .. + cnt[i-1], *tokens = the total
__global__ void __launch_bounds__(kCsvThreads)
csv_scan_kernel(const unsigned int* __restrict__ cnt, int64_t nblk, int64_t* __restrict__ base,
                int64_t* __restrict__ tokens) {
  __shared__ long long wtot[kCsvWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  long long carry = 0;
  for (int64_t i0 = 0; i0 < nblk; i0 += kCsvThreads) {
    const int64_t i = i0 + tid;
    const long long v = i < nblk ? (long long)cnt[i] : 0;
    long long incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const long long t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    long long off = 0, tot = 0;
    for (int w = 0; w < kCsvWaves; ++w) {
      if (w < wv) off += wtot[w];
      tot += wtot[w];
    }
    __syncthreads();
    if (i < nblk) base[i] = carry + off + incl - v;
    carry += tot;
  }
  if (tid == 0) *tokens = carry;
}

__global__ void __launch_bounds__(kCsvThreads)
csv_convert_kernel(const unsigned char* __restrict__ text, int64_t bytes,
                   const int64_t* __restrict__ base, const knncsv::NumTable* __restrict__ tab,
                   int dim, int with_label, int64_t cap, double* __restrict__ data,
                   int32_t* __restrict__ labels, int64_t* __restrict__ slow, int64_t slow_cap,
                   unsigned long long* __restrict__ nslow) {
  __shared__ int wtot[kCsvWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t blk0 = (int64_t)blockIdx.x * KNN_CSV_BLOCK_BYTES;
  int64_t c0 = base[blockIdx.x];  // index of the block's (then the tile's) first terminator
  for (int j = 0; j < kCsvTiles; ++j) {
    const int64_t p0 = blk0 + (int64_t)j * kCsvTile + tid * 16;
    unsigned int term = 0, delim = 0;
    if (p0 <= bytes) term = csv_masks(text, bytes, p0, &delim);
    const int n = __popc(term);
    int incl = n;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < kCsvWaves; ++w) {
      if (w < wv) off += wtot[w];
      tot += wtot[w];
    }
    __syncthreads();
    int64_t c = c0 + off + incl - n;
    c0 += tot;
    for (unsigned int m = term; m; m &= m - 1, ++c) {
      if (c >= cap) break;  // counted, not stored (c only grows)
      const int i = __ffs(m) - 1;
      const int64_t p = p0 + i;
      // the token's start: after the last delimiter in front of p
      const unsigned int below = delim & ((1u << i) - 1u);
      int64_t s;
      if (below) {
        s = p0 + (32 - __clz(below));
      } else {
        s = p0;
        while (s > 0 && p - s <= 64 && !csv_is_delim(text[s - 1])) --s;
      }
      const char* tb = reinterpret_cast<const char*>(text) + s;
      const char* te = reinterpret_cast<const char*>(text) + p;
      bool ok = p - s <= 64;
      bool is_label = false;
      int64_t row = 0;
      if (with_label) {
        row = c / (dim + 1);
        is_label = c - row * (dim + 1) == 0;
      }
      if (is_label) {
        int32_t l = 0;
        ok = ok && knncsv::csv_fast_atoi(tb, te, &l);
        if (ok) labels[row] = l;
      } else {
        double v = 0.0;
        ok = ok && knncsv::csv_fast_atof(tb, te, tab, &v);
        if (ok) data[with_label ? c - row - 1 : c] = v;
      }
      if (!ok) {
        const unsigned long long k = atomicAdd(nslow, 1ull);
        if (k < (unsigned long long)slow_cap) {
          slow[2 * k] = c;
          slow[2 * k + 1] = p;
        }
      }
    }
  }
}

// the host's values of the slow tokens: ent[2 i] = token index c, ent[2 i + 1]
// = the fp64 bits (a data token) or the int32 value (a label token)
__global__ void __launch_bounds__(kCsvThreads)
csv_scatter_kernel(const int64_t* __restrict__ ent, int64_t n, int dim, int with_label,
                   int64_t cap, double* __restrict__ data, int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * kCsvThreads + threadIdx.x;
  if (i >= n) return;
  const int64_t c = ent[2 * i];
  if (c < 0 || c >= cap) return;
  const int64_t bits = ent[2 * i + 1];
  if (with_label) {
    const int64_t row = c / (dim + 1);
    if (c - row * (dim + 1) == 0)
      labels[row] = (int32_t)bits;
    else
      reinterpret_cast<int64_t*>(data)[c - row - 1] = bits;
  } else {
    reinterpret_cast<int64_t*>(data)[c] = bits;
  }
}

}  // namespace

int64_t csv_block_count(int64_t bytes) { return bytes / KNN_CSV_BLOCK_BYTES + 1; }

void launch_csv_count_scan(const char* text, int64_t bytes, unsigned int* cnt, int64_t* base,
                           int64_t* tokens, hipStream_t s) {
  const int64_t nblk = csv_block_count(bytes);
  hipLaunchKernelGGL(csv_count_kernel, dim3((unsigned)nblk), dim3(kCsvThreads), 0, s,
                     reinterpret_cast<const unsigned char*>(text), bytes, cnt);
  hipLaunchKernelGGL(csv_scan_kernel, dim3(1), dim3(kCsvThreads), 0, s, cnt, nblk, base, tokens);
}

void launch_csv_convert(const char* text, int64_t bytes, const int64_t* base,
                        const knncsv::NumTable* tab, int dim, bool with_label, int64_t cap,
                        double* data, int32_t* labels, int64_t* slow, int64_t slow_cap,
                        int64_t* nslow, hipStream_t s) {
  hipLaunchKernelGGL(csv_convert_kernel, dim3((unsigned)csv_block_count(bytes)),
                     dim3(kCsvThreads), 0, s, reinterpret_cast<const unsigned char*>(text), bytes,
                     base, tab, dim, with_label ? 1 : 0, cap, data, labels, slow, slow_cap,
                     reinterpret_cast<unsigned long long*>(nslow));
}

void launch_csv_scatter(const int64_t* ent, int64_t n, int dim, bool with_label, int64_t cap,
                        double* data, int32_t* labels, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(csv_scatter_kernel, dim3((unsigned)((n + kCsvThreads - 1) / kCsvThreads)),
                     dim3(kCsvThreads), 0, s, ent, n, dim, with_label ? 1 : 0, cap, data, labels);
}

}  // namespace knnk
