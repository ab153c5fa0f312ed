// knn_fold.hip -- F-fold cross-validated K sweep on fold shards (gfx950).
//
// knn_set_folds gathers the train set fold by fold into one fold-major fp64
// copy; every fold's slice is the train set of a sub-context of its own.  The
// rows of fold f are then classified against the other F - 1 shards: each
// shard's exact partial list (knn_search_partial_device), the k-way merge, the
// sweep tie scan, the reference-order pass and the prefix votes -- the
// train-sharded chain on one GPU and one stream.  The kernels here are the two
// pieces that chain lacks:
//   fold_gather_kernel   the stable gather into fold-major order;
//   fold_map_idx_kernel  a shard's local list indices -> original train rows.
// The gather is stable (rows_of[g] ascends), so a list sorted by (dist, local
// index) is sorted by (dist, original index) after the map, which is the
// order the merge expects of its parts and breaks cross-part ties by.
#include "knn_device.h"

#include <algorithm>

namespace knnk {

namespace {

// Register bounds (tests/test_kernel_resources_kfold.py): both kernels are
// plain streaming loops -- no LDS, no scratch, at most 32 VGPRs, no AGPRs.

// Xf[j][c] = X[rows[j]][c], labf[j] = lab[rows[j]] for the n rows of the
// fold-major order; one thread per value, a grid-stride loop
__global__ void __launch_bounds__(256)
fold_gather_kernel(const double* __restrict__ X, const int32_t* __restrict__ lab,
                   const int32_t* __restrict__ rows, int64_t n, int d, double* __restrict__ Xf,
                   int32_t* __restrict__ labf) {
  const int64_t total = n * d;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = e / d;
    const int c = (int)(e - j * d);
    const int64_t r = rows[j];
    Xf[e] = X[r * d + c];
    if (c == 0) labf[j] = lab[r];
  }
}

// idx[e] (a shard's local row, -1 in a padded slot) -> base + rows_g[idx[e]];
// a value outside [0, n_g) becomes -1 (nothing is read out of bounds)
__global__ void __launch_bounds__(256)
fold_map_idx_kernel(int64_t* __restrict__ idx, int64_t cnt, const int32_t* __restrict__ rows_g,
                    int64_t n_g, int64_t base) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < cnt;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = idx[e];
    idx[e] = (v >= 0 && v < n_g) ? base + (int64_t)rows_g[v] : (int64_t)-1;
  }
}

unsigned fold_grid(int64_t work, int cus) {
  return (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((work + 255) / 256, (int64_t)std::max(cus, 1) * 16));
}

}  // namespace

void launch_fold_gather(const double* X, const int32_t* lab, const int32_t* rows, int64_t n, int d,
                        double* Xf, int32_t* labf, int cus, hipStream_t s) {
  if (n <= 0 || d <= 0) return;
  hipLaunchKernelGGL(fold_gather_kernel, dim3(fold_grid(n * d, cus)), dim3(256), 0, s, X, lab,
                     rows, n, d, Xf, labf);
}

void launch_fold_map_idx(int64_t* idx, int64_t cnt, const int32_t* rows_g, int64_t n_g,
                         int64_t base, int cus, hipStream_t s) {
  if (cnt <= 0) return;
  hipLaunchKernelGGL(fold_map_idx_kernel, dim3(fold_grid(cnt, cus)), dim3(256), 0, s, idx, cnt,
                     rows_g, n_g, base);
}

}  // namespace knnk
