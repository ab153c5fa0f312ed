// knn_eval.hip -- per-class evaluation of the K sweep (gfx950): the confusion
// matrix at every K of the list, and the vote counts of each query.
//
// Both are defined by what the library already reproduces from the reference:
// its neighbour order (std::sort over all N_train records, cpp:323/366) and
// its first-to-strictly-exceed vote (cpp:324-337).
//   eval_confusion_kernel    conf[i][t][p] += #{q : truth[q] == t and
//                            labels[i][q] == p} over the sweep's [nk][m] label
//                            array (≙ Val_label against Val_label_buffer,
//                            cpp:341-343, per class pair instead of one cnt);
//                            unl[i] += the queries whose label or truth lies
//                            outside [0, C) (label -1 at K = 0 or for a
//                            non-finite query, any truth the caller supplies)
//   eval_vote_counts_kernel  counts[q][c] = #{t < k : label of row entry t ==
//                            c} over ordered neighbour rows (the per-class
//                            counters the vote kernel never keeps)
// The confusion histograms are privatised in LDS and flushed with one 64-bit
// global atomic per non-zero bin per workgroup, as sweep_vote_kernel does for
// `correct`.  Three regimes by C (kEvalSmallC / kEvalLdsC, chosen on the host):
//   small   C <= 16: one LDS copy per wave (the diagonal bins are hot: at C =
//           10 about 90 % of a wave's lanes hit about 10 bins);
//   medium  C <= 96: one LDS histogram per workgroup (C * C 32-bit counters,
//           36 KB at C = 96: four workgroups share a CU's 160 KB);
//   large   beyond: 64-bit global atomics directly.
// 32-bit LDS counters suffice: a workgroup counts at most m < 2^31 queries.
#include "knn_device.h"

#include <algorithm>

namespace knnk {

namespace {

constexpr int kEvalWaves = 4;  // waves per workgroup (both kernels)
constexpr int kEvalThreads = kEvalWaves * 64;
constexpr int kEvalSmallBins = kEvalSmallC * kEvalSmallC;
constexpr int kEvalLdsBins = kEvalLdsC * kEvalLdsC;

// REG 0 small (per-wave LDS copies), 1 medium (one LDS histogram), 2 large
// (global atomics).  Grid: x = tiles of qt queries, y = the K of the list.
// Reads are coalesced along q; nothing is indexed by a label or a truth value
// before it is checked against [0, C).
template <int REG>
__global__ void __launch_bounds__(kEvalThreads)
eval_confusion_kernel(const int32_t* __restrict__ labels, int64_t m,
                      const int32_t* __restrict__ truth, int C, int qt,
                      unsigned long long* __restrict__ conf,
                      unsigned long long* __restrict__ unl) {
  constexpr int kBins = REG == 0 ? kEvalWaves * kEvalSmallBins : REG == 1 ? kEvalLdsBins : 1;
  __shared__ unsigned int hist[kBins];
  const int tid = threadIdx.x, wv = tid >> 6;
  const int i = blockIdx.y;
  const int64_t bins64 = (int64_t)C * C;  // (fits an int in the LDS regimes: C <= kEvalLdsC)
  const int bins = (int)bins64;
  if (REG == 0)
    for (int b = tid; b < kEvalWaves * bins; b += kEvalThreads) hist[b] = 0;
  if (REG == 1)
    for (int b = tid; b < bins; b += kEvalThreads) hist[b] = 0;
  if (REG != 2) __syncthreads();
  unsigned int* h = REG == 0 ? hist + wv * bins : hist;
  const int32_t* lrow = labels + (int64_t)i * m;
  unsigned long long* crow = conf ? conf + (int64_t)i * bins64 : nullptr;
  const int64_t q0 = (int64_t)blockIdx.x * qt;
  const int64_t q1 = q0 + qt < m ? q0 + qt : m;
  int bad = 0;
  for (int64_t q = q0 + tid; q < q1; q += kEvalThreads) {
    const unsigned int p = (unsigned int)lrow[q];
    const unsigned int t = (unsigned int)truth[q];
    if (p < (unsigned int)C && t < (unsigned int)C) {
      if (REG == 2) {
        if (crow) atomicAdd(&crow[(int64_t)t * C + p], 1ull);
      } else {
        atomicAdd(&h[(int)t * C + (int)p], 1u);
      }
    } else {
      ++bad;
    }
  }
  // unlabelled queries: one global atomic per wave that saw any
  if (unl) {
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((tid & 63) == 0 && bad) atomicAdd(&unl[i], (unsigned long long)bad);
  }
  if (REG != 2) {
    __syncthreads();
    if (crow)
      for (int b = tid; b < bins; b += kEvalThreads) {
        unsigned int v = hist[b];
        if (REG == 0)
          for (int w = 1; w < kEvalWaves; ++w) v += hist[w * bins + b];
        if (v) atomicAdd(&crow[b], (unsigned long long)v);
      }
  }
}

// One wave per query (4 per workgroup, a grid-stride loop over the queries),
// the row walked 64 entries at a time: nothing of the row is staged, so rows
// of any length take the same path.  LDS: per-wave counters [C] while C <=
// kEvalCountsLdsC; beyond, 32-bit global atomics on the output row the host
// zeroed before the launch.  Entries with idx -1 (or below idx_base) and
// labels outside [0, C) count nothing.
template <bool LDS>
__global__ void __launch_bounds__(kEvalThreads)
eval_vote_counts_kernel(const int64_t* __restrict__ idx, int64_t m, int kmax,
                        const int32_t* __restrict__ lab, int64_t idx_base, int k, int C,
                        int32_t* __restrict__ counts) {
  __shared__ int cnt[LDS ? kEvalWaves * kEvalCountsLdsC : 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* c = cnt + (LDS ? wv * C : 0);
  for (int64_t q = (int64_t)blockIdx.x * kEvalWaves + wv; q < m;
       q += (int64_t)gridDim.x * kEvalWaves) {
    const int64_t* irow = idx + q * kmax;
    int32_t* orow = counts + q * C;
    if (LDS) {
      for (int j = lane; j < C; j += 64) c[j] = 0;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    for (int t = lane; t < k; t += 64) {
      const int64_t gi = irow[t];
      const int64_t r = gi - idx_base;
      if (gi < 0 || r < 0) continue;
      const unsigned int l = (unsigned int)lab[r];
      if (l >= (unsigned int)C) continue;
      if (LDS)
        atomicAdd(&c[l], 1);
      else
        atomicAdd(&orow[l], 1);
    }
    if (LDS) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int j = lane; j < C; j += 64) orow[j] = c[j];
      // (the next query's zeroing follows these reads in program order)
      __builtin_amdgcn_wave_barrier();
    }
  }
}

}  // namespace

int eval_confusion_regime(int class_cnt) {
  return class_cnt <= kEvalSmallC ? 0 : class_cnt <= kEvalLdsC ? 1 : 2;
}

void launch_eval_confusion(const int32_t* labels, int nk, int64_t m, const int32_t* truth,
                           int class_cnt, unsigned long long* conf, unsigned long long* unl,
                           hipStream_t s) {
  if (nk <= 0 || m <= 0 || (!conf && !unl)) return;
  const int reg = eval_confusion_regime(class_cnt);
  // queries per workgroup: enough to pay for zeroing and flushing its bins
  const int qt = reg == 1 ? 8192 : 2048;
  const dim3 grid((unsigned)((m + qt - 1) / qt), (unsigned)nk);
  if (reg == 0)
    hipLaunchKernelGGL(eval_confusion_kernel<0>, grid, dim3(kEvalThreads), 0, s, labels, m, truth,
                       class_cnt, qt, conf, unl);
  else if (reg == 1)
    hipLaunchKernelGGL(eval_confusion_kernel<1>, grid, dim3(kEvalThreads), 0, s, labels, m, truth,
                       class_cnt, qt, conf, unl);
  else
    hipLaunchKernelGGL(eval_confusion_kernel<2>, grid, dim3(kEvalThreads), 0, s, labels, m, truth,
                       class_cnt, qt, conf, unl);
}

hipError_t launch_eval_vote_counts(const int64_t* idx, int64_t m, int kmax, const int32_t* lab,
                                   int64_t idx_base, int k, int class_cnt, int32_t* counts,
                                   int cus, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  const int64_t wgs = (m + kEvalWaves - 1) / kEvalWaves;
  const unsigned grid =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>(wgs, (int64_t)std::max(cus, 1) * 8));
  if (class_cnt <= kEvalCountsLdsC) {
    hipLaunchKernelGGL(eval_vote_counts_kernel<true>, dim3(grid), dim3(kEvalThreads), 0, s, idx, m,
                       kmax, lab, idx_base, k, class_cnt, counts);
    return hipSuccess;
  }
  const hipError_t e =
      hipMemsetAsync(counts, 0, (size_t)m * (size_t)class_cnt * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(eval_vote_counts_kernel<false>, dim3(grid), dim3(kEvalThreads), 0, s, idx, m,
                     kmax, lab, idx_base, k, class_cnt, counts);
  return hipSuccess;
}

}  // namespace knnk
