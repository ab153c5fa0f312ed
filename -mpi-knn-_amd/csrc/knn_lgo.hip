// knn_lgo.hip -- K sweep under group exclusion (leave-one-group-out): each
// query's neighbour row with every train row of one group taken out (gfx950).
//
// Leave-one-out (knn_loo.hip) overstates accuracy when train rows are not
// independent (several samples of one subject, augmented copies, duplicates):
// the held-out row's siblings stay and vote for it.  Here a train set carries
// a group id per row and a query a group gq; the rule that fixes every output:
// the result is the K sweep's on the train set with every row r, groups[r] ==
// gq, removed (the labels lose the same entries), the reported indices mapped
// back to the full set.
//
// The search runs once at k1 = kmax + gmax (gmax: the largest group) and
// leaves the (dist, idx)-ordered top k1 of the FULL set.  A total order minus
// a set of records is the order of the rest, so the (dist, idx) order of the
// reduced set is the full order minus the group.  At most gmax records leave,
// so at least kmax of the row's k1 entries survive: the reduced top kmax is the
// row minus its excluded entries, truncated to kmax.  With c the number of the
// row's entries that are dropped, the reduced set's record kmax (the successor
// that decides KNN_FLAG_TIE_BOUNDARY) is
//   1. c < gmax: at least kmax + 1 entries survive, the successor is the kept
//      entry kmax, inside the row: the bit is dist'[kmax - 1] == dist'[kmax];
//   2. c == gmax: exactly kmax entries survive and the whole group lies inside
//      the row, so the successor is the full order's record k1 -- outside the
//      row.  The search's KNN_FLAG_TIE_BOUNDARY bit for k1 says dist[k1 - 1] ==
//      dist[k1] of the full order.  The last kept entry is entry k1 - 1 only
//      when that one is kept; when the row ENDS with dropped entries the last
//      kept distance may be smaller.  Distances ascend, so dist'[kmax - 1] <=
//      dist[k1 - 1] <= dist[k1] and the reduced bit is "the search's bit AND
//      dist'[kmax - 1] == dist[k1 - 1]".
// KNN_FLAG_TIE_VOTE / KNN_FLAG_TIE_ORDER are finish_single's over the kept
// row (equal adjacent distances with different / equal labels).  The order
// among exactly equal distances that the reference's std::sort leaves over
// the n - c remaining records is restored afterwards by
// tie_order_group_kernel (knn_select.hip).
//
// Large groups are served correctly but through the wide search (k1 grows with
// gmax); masking the group inside the candidate pass is a separate change.
#include "knn_device.h"

#include <algorithm>

namespace knnk {

namespace {

constexpr int kLgoWaves = 4;  // waves (queries in flight) per workgroup, as loo_drop_kernel

// lanes below `lane` set in a wave ballot
__device__ __forceinline__ int lgo_rank(unsigned long long b) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                        __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// One wave per query, a grid-stride loop over the queries; the row is walked
// 64 entries at a time.  Entry t is kept iff groups[idx[t] - idx_base] != gq;
// its position in the kept row is the count of kept entries before the chunk
// plus the lane's rank in the chunk's ballot.
// in_*: [m][k1] rows and the flags of the search at k1 = kmax + gmax;
// out_*: [m][kmax] rows and the flags for kmax on the reduced set.
__global__ void __launch_bounds__(kLgoWaves * 64)
lgo_drop_kernel(const double* __restrict__ in_dist, const int64_t* __restrict__ in_idx,
                const int32_t* __restrict__ in_flags, const int32_t* __restrict__ qgroup,
                const int32_t* __restrict__ groups, int64_t m, int kmax, int k1,
                const int32_t* __restrict__ lab, int64_t idx_base, int64_t n,
                double* __restrict__ out_dist, int64_t* __restrict__ out_idx,
                int32_t* __restrict__ out_flags) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t q = (int64_t)blockIdx.x * kLgoWaves + wv; q < m;
       q += (int64_t)gridDim.x * kLgoWaves) {
    const int64_t* irow = in_idx + q * k1;
    const double* drow = in_dist + q * k1;
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
    const int gq = qgroup[q];  // ids lie in [0, n_groups): any other value matches no row
    int kept = 0;              // kept entries before the chunk (wave-uniform)
    int tie = 0;
    // the last kept entry before the chunk (wave-uniform; valid once kept > 0)
    double pd = 0.0;
    int pl = -1;
    double succ = 0.0;  // kept entry kmax, if the row holds one
    for (int t0 = 0; t0 < k1 && kept <= kmax; t0 += 64) {
      const int t = t0 + lane;
      int64_t gi = -1;
      double dv = 0.0;
      int lb = -1;
      bool keep = false;
      if (t < k1) {
        gi = irow[t];
        dv = drow[t];
        const int64_t r = gi - idx_base;
        if (r >= 0 && r < n) {
          keep = groups[r] != gq;
          lb = lab[r];
        } else {
          keep = gi >= 0;  // (a foreign index belongs to no group; -1 pads the row)
        }
      }
      const unsigned long long b = __ballot(keep);
      const int pos = kept + lgo_rank(b);
      if (keep && pos < kmax) {
        orow_i[pos] = gi;
        orow_d[pos] = dv;
      }
      // the kept entry before this one: the nearest kept lane below, else the
      // last kept entry of the earlier chunks
      const unsigned long long below = b & ((1ull << lane) - 1ull);
      const int src = below ? 63 - __clzll((long long)below) : lane;
      const double sd = __shfl(dv, src, 64);
      const int sl = __shfl(lb, src, 64);
      const double qd = below ? sd : pd;
      const int ql = below ? sl : pl;
      if (keep && pos > 0 && pos < kmax && qd == dv)  // TIE_VOTE / TIE_ORDER (finish_single)
        tie |= ql != lb ? 4 : 8;
      const unsigned long long hit = __ballot(keep && pos == kmax);
      if (hit) succ = __shfl(dv, __ffsll((long long)hit) - 1, 64);
      // the last kept entry at a position < kmax carries over (the boundary
      // bit compares against it)
      const unsigned long long inrow = __ballot(keep && pos < kmax);
      if (inrow) {
        const int last = 63 - __clzll((long long)inrow);
        pd = __shfl(dv, last, 64);
        pl = __shfl(lb, last, 64);
      }
      kept += __popcll(b);
    }
    // (a row cannot run short: groups hold at most gmax rows and k1 <= n)
    tie = wave_or_i(tie);
    if (lane == 0) {
      // pd = dist'[kmax - 1].  kept > kmax: the successor is inside the row;
      // else every entry was visited, exactly kmax survive and the successor is
      // the full order's record k1 (the search's bit for k1, see above)
      const bool bnd = kept > kmax ? pd == succ : (f_in & 2) != 0 && pd == drow[k1 - 1];
      out_flags[q] = (f_in & (1 | 16)) | tie | (bnd ? 2 : 0);  // EXACT_RESCAN, NONFINITE kept
    }
  }
}

// leave-one-group-out over train rows [row0, row0 + rows): query i excludes
// the group of row row0 + i (and so itself)
__global__ void lgo_self_kernel(int32_t* __restrict__ qgroup, const int32_t* __restrict__ groups,
                                int64_t rows, int64_t row0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) qgroup[i] = groups[row0 + i];
}

// group sizes hist[n_groups] (zeroed by the caller) and the first row whose id
// lies outside [0, n_groups) (*bad, preset to n)
__global__ void lgo_hist_kernel(const int32_t* __restrict__ groups, int64_t n, int32_t n_groups,
                                int32_t* __restrict__ hist, unsigned long long* __restrict__ bad) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t g = groups[r];
    if (g < 0 || g >= n_groups) atomicMin(bad, (unsigned long long)r);
    else atomicAdd(&hist[g], 1);
  }
}

// *gmax (zeroed by the caller) = the largest group's size
__global__ void lgo_max_kernel(const int32_t* __restrict__ hist, int32_t n_groups,
                               int32_t* __restrict__ gmax) {
  int v = 0;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups;
       g += (int64_t)gridDim.x * blockDim.x)
    v = max(v, hist[g]);
  v = wave_max_i(v);
  if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(gmax, v);
}

}  // namespace

void launch_lgo_drop(const double* in_dist, const int64_t* in_idx, const int32_t* in_flags,
                     const int32_t* qgroup, const int32_t* groups, int64_t m, int kmax, int k1,
                     const int32_t* lab, int64_t idx_base, int64_t n, double* out_dist,
                     int64_t* out_idx, int32_t* out_flags, int cus, hipStream_t s) {
  if (m <= 0 || kmax <= 0) return;
  const int64_t wgs = (m + kLgoWaves - 1) / kLgoWaves;
  const unsigned grid =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>(wgs, (int64_t)std::max(cus, 1) * 8));
  hipLaunchKernelGGL(lgo_drop_kernel, dim3(grid), dim3(kLgoWaves * 64), 0, s, in_dist, in_idx,
                     in_flags, qgroup, groups, m, kmax, k1, lab, idx_base, n, out_dist, out_idx,
                     out_flags);
}

void launch_lgo_self(int32_t* qgroup, const int32_t* groups, int64_t rows, int64_t row0,
                     hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(lgo_self_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s,
                     qgroup, groups, rows, row0);
}

void launch_lgo_group_stats(const int32_t* groups, int64_t n, int32_t n_groups, int32_t* hist,
                            unsigned long long* bad, int32_t* gmax, int cus, hipStream_t s) {
  const int64_t cap = (int64_t)std::max(cus, 1) * 8;
  const unsigned g1 = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
  const unsigned g2 =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n_groups + 255) / 256, cap));
  hipLaunchKernelGGL(lgo_hist_kernel, dim3(g1), dim3(256), 0, s, groups, n, n_groups, hist, bad);
  hipLaunchKernelGGL(lgo_max_kernel, dim3(g2), dim3(256), 0, s, hist, n_groups, gmax);
}

}  // namespace knnk
