// knn_loo.hip -- K sweep under exclusion (leave-one-out): each query's
// neighbour row with one train row taken out (gfx950).
//
// The reference judges K on a separate validation set (cpp:308-343).  With a
// train set alone the standard answer is leave-one-out: classify each train
// row against all the OTHER train rows.  The rule that fixes every output:
// for a query with excluded train row e the result is the K sweep's on the
// train set with row e removed (the labels lose the same entry), the reported
// indices >= e shifted back up by one.
//
// The search runs once at kmax + 1 and leaves the (dist, idx)-ordered top
// (kmax + 1) of the FULL set.  Removing one record from a total order leaves
// the order of the rest, so the (dist, idx) order of the reduced set is the
// full set's order minus e.  Two cases follow for the reduced top kmax:
//   1. e is inside the full top (kmax + 1): the reduced top kmax is that row
//      minus e, and the reduced set's record kmax (its successor) is the full
//      set's record kmax + 1 -- outside the row, but the search's
//      KNN_FLAG_TIE_BOUNDARY bit for kmax + 1 is exactly "dist[kmax] ==
//      dist[kmax + 1]" of the full order, i.e. the reduced boundary bit;
//   2. e is outside it (e = -1, a far row, or more than kmax rows at the same
//      distance and of lower index than e, e.g. zero-distance duplicates of a
//      leave-one-out query): the reduced top kmax is the row's first kmax
//      entries and its successor the row's entry kmax (not e), so the
//      boundary bit is dist[kmax - 1] == dist[kmax], read inside the row.
// KNN_FLAG_TIE_VOTE / KNN_FLAG_TIE_ORDER are finish_single's over the kept
// row (equal adjacent distances with different / equal labels).  The order
// among exactly equal distances that the reference's std::sort leaves over
// the n - 1 remaining records is restored afterwards by tie_order_kernel
// with the same exclusion (knn_select.hip).
#include "knn_device.h"

#include <algorithm>

namespace knnk {

namespace {

constexpr int kLooWaves = 4;  // waves (queries in flight) per workgroup, as the sweep kernels

// label of row entry gi (global index); -1 for an empty slot or a foreign index
__device__ __forceinline__ int loo_label(const int32_t* __restrict__ lab, int64_t gi,
                                         int64_t idx_base, int64_t n) {
  const int64_t r = gi - idx_base;
  return r >= 0 && r < n ? lab[r] : -1;
}

// One wave per query, a grid-stride loop over the queries; rows of any length
// are walked 64 entries at a time (nothing is staged in LDS).
// in_*: [m][kmax + 1] rows and the flags of the search at kmax + 1;
// out_*: [m][kmax] rows and the flags for kmax on the reduced set.
__global__ void __launch_bounds__(kLooWaves * 64)
loo_drop_kernel(const double* __restrict__ in_dist, const int64_t* __restrict__ in_idx,
                const int32_t* __restrict__ in_flags, const int64_t* __restrict__ excl, int64_t m,
                int kmax, const int32_t* __restrict__ lab, int64_t idx_base, int64_t n,
                double* __restrict__ out_dist, int64_t* __restrict__ out_idx,
                int32_t* __restrict__ out_flags) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = kmax + 1;
  for (int64_t q = (int64_t)blockIdx.x * kLooWaves + wv; q < m;
       q += (int64_t)gridDim.x * kLooWaves) {
    const int64_t* irow = in_idx + q * w;
    const double* drow = in_dist + q * w;
    int64_t* orow_i = out_idx + q * kmax;
    double* orow_d = out_dist + q * kmax;
    const int f_in = in_flags[q];
    if (irow[0] < 0) {  // no neighbours (a non-finite query): an empty row
      for (int t = lane; t < kmax; t += 64) {
        orow_i[t] = irow[t];
        orow_d[t] = drow[t];
      }
      if (lane == 0) out_flags[q] = f_in;
      continue;
    }
    // a value outside [-1] U [idx_base, idx_base + n) excludes nothing
    const int64_t e = excl ? excl[q] : -1;
    const bool has = e >= idx_base && e < idx_base + n;
    // position of e in the row: a ballot per 64 entries (e occurs at most once)
    int p = w;
    if (has) {
      for (int t0 = 0; t0 < w && p == w; t0 += 64) {
        const int t = t0 + lane;
        const unsigned long long hit = __ballot(t < w && irow[t] == e);
        if (hit) p = t0 + __ffsll((long long)hit) - 1;
      }
    }
    // kept entry t comes from row entry t + (hits before it): t + (t >= p)
    int tie = 0;
    for (int t = lane; t < kmax; t += 64) {
      const int s0 = t + (t >= p);
      const int64_t gi = irow[s0];
      const double dv = drow[s0];
      orow_i[t] = gi;
      orow_d[t] = dv;
      if (t + 1 < kmax) {
        const int s1 = t + 1 + (t + 1 >= p);
        if (dv == drow[s1])  // TIE_VOTE / TIE_ORDER of the kept row (finish_single)
          tie |= loo_label(lab, gi, idx_base, n) != loo_label(lab, irow[s1], idx_base, n) ? 4 : 8;
      }
    }
    tie = wave_or_i(tie);
    if (lane == 0) {
      // case 1: the search's boundary bit for kmax + 1; case 2: inside the row
      const bool bnd = p < w ? (f_in & 2) != 0 : drow[kmax - 1] == drow[kmax];
      out_flags[q] = (f_in & (1 | 16)) | tie | (bnd ? 2 : 0);  // EXACT_RESCAN, NONFINITE kept
    }
  }
}

// leave-one-out over train rows [row0, row0 + rows): query i excludes itself
__global__ void loo_self_kernel(int64_t* __restrict__ excl, int64_t rows, int64_t first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) excl[i] = first + i;
}

}  // namespace

void launch_loo_drop(const double* in_dist, const int64_t* in_idx, const int32_t* in_flags,
                     const int64_t* excl, int64_t m, int kmax, const int32_t* lab,
                     int64_t idx_base, int64_t n, double* out_dist, int64_t* out_idx,
                     int32_t* out_flags, int cus, hipStream_t s) {
  if (m <= 0 || kmax <= 0) return;
  const int64_t wgs = (m + kLooWaves - 1) / kLooWaves;
  const unsigned grid =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>(wgs, (int64_t)std::max(cus, 1) * 8));
  hipLaunchKernelGGL(loo_drop_kernel, dim3(grid), dim3(kLooWaves * 64), 0, s, in_dist, in_idx,
                     in_flags, excl, m, kmax, lab, idx_base, n, out_dist, out_idx, out_flags);
}

void launch_loo_self(int64_t* excl, int64_t rows, int64_t first, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(loo_self_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, excl,
                     rows, first);
}

}  // namespace knnk
