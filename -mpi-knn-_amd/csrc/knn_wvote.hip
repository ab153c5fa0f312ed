// knn_wvote.hip -- distance-weighted voting over ordered neighbour rows
// (gfx950): the weighted twins of sweep_vote_kernel (knn_sweep.hip) and
// eval_vote_counts_kernel (knn_eval.hip).
//
// The rule (include/knn_amd.h, KNN_VOTE_DISTANCE).  For one query with the
// ascending row idx[t], dist[t] (the fp64 reference distances), l_t = the label
// of entry t, the label at prefix length K is
//   z = #{t < K : dist[t] == 0}   (ascending row: the first z entries)
//   z >= 1: entries t < z vote with weight 1.0, the others do not vote;
//   else    w_t = 1.0 / dist[t]   (IEEE fp64 division; 1 / inf = 0)
//   S[c] = 0, best = -inf, label = -1
//   for t < K in row order (voting entries; empty slots idx -1 never vote):
//     S[l_t] = S[l_t] + w_t;  if S[l_t] > best: best = S[l_t], label = l_t
// With unit weights this scan is the reference's first-to-strictly-exceed vote
// (cpp:324-337).  The adds of one class happen in row order, one fp64 add per
// entry, so the sums -- and with them the labels -- are reproducible bit for
// bit by a sequential loop on any machine.
//
// Both kernels run one wave per query (4 waves per workgroup, a grid-stride
// loop over the queries).  In the kernels the row counts as "exact match" mode
// when dist[0] == 0; an entry then votes iff its own distance is 0, which on an
// ascending row is the rule above at every K.
//   wvote_sweep_kernel  the label at every K of a list.  The row's labels and
//     weights are resident in LDS, kWvChunkMax entries at a time; lane t forms
//     S_t = the running sum of its entry's class by a sequential loop over the
//     earlier entries (those of earlier chunks restaged 64 at a time), a wave
//     scan over (sum, label) pairs -- "the later entry takes the lead only when
//     its sum strictly exceeds the earlier maximum" -- leaves the winner of
//     every prefix, and each K of the list looks its winner up.  The per-K
//     correct counts go through per-workgroup LDS counters.
//   wvote_sums_kernel   the class sums S[c] after the first k entries, lane c
//     (mod 64) owning class c in a register and walking the row, staged 64
//     entries at a time, in order.
// No per-class array indexed by a label exists, so labels need no bound; a
// sum that is NaN (a NaN distance in caller-supplied rows) never takes the
// lead, as in the sequential loop.  Built without -fno-honor-nans for that.
#include "knn_device.h"

#include <algorithm>

namespace knnk {

namespace {

constexpr int kWvWaves = 4;        // waves (queries in flight) per workgroup
constexpr int kWvChunkMax = 512;   // row entries per LDS chunk

__device__ __forceinline__ void wv_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Row entry t: its label (-1: the entry does not vote -- an empty slot, an
// index below idx_base, or a non-zero distance on an exact-match row) and its
// weight.
__device__ __forceinline__ void wv_entry(const int64_t* __restrict__ irow,
                                         const double* __restrict__ drow,
                                         const int32_t* __restrict__ lab, int64_t idx_base, int t,
                                         bool zmode, int& l, double& w) {
  const int64_t gi = irow[t];
  const int64_t r = gi - idx_base;
  const double d = drow[t];
  const bool votes = gi >= 0 && r >= 0 && (!zmode || d == 0.0);
  l = votes ? lab[r] : -1;
  w = zmode ? 1.0 : 1.0 / d;
}

// Inclusive wave scan over (sum, label) pairs: the pair of the first entry
// that reaches the prefix maximum (an earlier entry keeps the lead unless a
// later one strictly exceeds it).
__device__ __forceinline__ void wv_scan_lead(double& v, int& l) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double uv = __shfl_up(v, o, 64);
    const int ul = __shfl_up(l, o, 64);
    if (lane >= o && !(v > uv)) {
      v = uv;
      l = ul;
    }
  }
}

// doubles of dynamic LDS per wave: wa[ch] sa[ch] wb[64] | la[ch] lb[64] (ints)
__host__ __device__ constexpr int wv_wave_doubles(int ch) { return 2 * ch + 64 + (ch + 64) / 2; }

__global__ void __launch_bounds__(kWvWaves * 64)
wvote_sweep_kernel(const int64_t* __restrict__ idx, const double* __restrict__ dist, int64_t m,
                   int kmax, const int32_t* __restrict__ lab, int64_t idx_base,
                   const int* __restrict__ ks, int nk, int ch, int32_t* __restrict__ labels,
                   const int32_t* __restrict__ truth, unsigned long long* __restrict__ correct) {
  extern __shared__ double wv_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int* acc = (int*)wv_lds;  // [nk] (with truth), padded to whole doubles
  double* wa = wv_lds + (truth ? (nk + 1) / 2 : 0) + wv * wv_wave_doubles(ch);
  double* sa = wa + ch;
  double* wb = sa + ch;
  int* la = (int*)(wb + 64);
  int* lb = la + ch;
  if (truth) {
    for (int j = tid; j < nk; j += blockDim.x) acc[j] = 0;
    __syncthreads();
  }
  const double ninf = -__builtin_huge_val();
  for (int64_t q = (int64_t)blockIdx.x * kWvWaves + wv; q < m;
       q += (int64_t)gridDim.x * kWvWaves) {
    for (int j = lane; j < nk; j += 64)
      if (ks[j] == 0) labels[(int64_t)j * m + q] = -1;  // (kmax == 0: every K is 0)
    if (kmax == 0) continue;
    const int64_t* irow = idx + q * kmax;
    const double* drow = dist + q * kmax;
    const int tr = truth ? truth[q] : -1;
    const bool zmode = drow[0] == 0.0;
    double P = ninf;  // best / label before this chunk
    int Wl = -1;
    for (int a0 = 0; a0 < kmax; a0 += ch) {
      const int len = min(ch, kmax - a0);
      for (int t = lane; t < len; t += 64) {
        int l;
        double w;
        wv_entry(irow, drow, lab, idx_base, a0 + t, zmode, l, w);
        la[t] = l;
        wa[t] = w;
        sa[t] = 0.0;
      }
      wv_wave_sync();
      // the entries before the chunk, 64 at a time (a0 is a multiple of 64)
      for (int b0 = 0; b0 < a0; b0 += 64) {
        int l;
        double w;
        wv_entry(irow, drow, lab, idx_base, b0 + lane, zmode, l, w);
        lb[lane] = l;
        wb[lane] = w;
        wv_wave_sync();
        for (int t = lane; t < len; t += 64) {
          const int lt = la[t];
          if (lt < 0) continue;
          double s = sa[t];
          for (int u = 0; u < 64; ++u)
            if (lb[u] == lt) s = s + wb[u];
          sa[t] = s;
        }
        wv_wave_sync();
      }
      for (int t = lane; t < len; t += 64) {
        const int lt = la[t];
        if (lt < 0) continue;
        double s = sa[t];
        for (int u = 0; u <= t; ++u)
          if (la[u] == lt) s = s + wa[u];
        sa[t] = s;
      }
      wv_wave_sync();
      for (int t0 = 0; t0 < len; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < len;
        int l = valid ? la[t] : -1;
        double v = l >= 0 ? sa[t] : ninf;
        if (!(v == v)) v = ninf;  // a NaN sum never exceeds
        wv_scan_lead(v, l);
        if (!(v > P)) {
          v = P;
          l = Wl;
        }
        if (valid) la[t] = l;  // winner of the prefix a0 + t + 1
        P = __shfl(v, 63, 64);
        Wl = __shfl(l, 63, 64);
      }
      wv_wave_sync();
      for (int j = lane; j < nk; j += 64) {
        const int K = ks[j];
        if (K - 1 < a0 || K - 1 >= a0 + len) continue;
        const int lbl = la[K - 1 - a0];
        labels[(int64_t)j * m + q] = lbl;
        if (truth && lbl >= 0 && lbl == tr) atomicAdd(&acc[j], 1);
      }
      wv_wave_sync();
    }
  }
  if (truth) {
    __syncthreads();
    for (int j = tid; j < nk; j += blockDim.x)
      if (acc[j]) atomicAdd(&correct[j], (unsigned long long)acc[j]);
  }
}

__global__ void __launch_bounds__(kWvWaves * 64)
wvote_sums_kernel(const int64_t* __restrict__ idx, const double* __restrict__ dist, int64_t m,
                  int kmax, const int32_t* __restrict__ lab, int64_t idx_base, int k, int C,
                  double* __restrict__ wsum) {
  __shared__ double wb_all[kWvWaves * 64];
  __shared__ int lb_all[kWvWaves * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* wb = wb_all + wv * 64;
  int* lb = lb_all + wv * 64;
  for (int64_t q = (int64_t)blockIdx.x * kWvWaves + wv; q < m;
       q += (int64_t)gridDim.x * kWvWaves) {
    const int64_t* irow = idx + q * kmax;
    const double* drow = dist + q * kmax;
    double* orow = wsum + q * C;
    const bool zmode = k > 0 && drow[0] == 0.0;
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int c = c0 + lane;
      double s = 0.0;
      for (int b0 = 0; b0 < k; b0 += 64) {
        int l = -1;
        double w = 0.0;
        if (b0 + lane < k) wv_entry(irow, drow, lab, idx_base, b0 + lane, zmode, l, w);
        lb[lane] = l;
        wb[lane] = w;
        wv_wave_sync();
        const int nb = min(64, k - b0);
        for (int u = 0; u < nb; ++u)
          if (lb[u] == c) s = s + wb[u];
        wv_wave_sync();
      }
      if (c < C) orow[c] = s;
    }
  }
}

int wv_chunk(int kmax) {
  return kmax >= kWvChunkMax ? kWvChunkMax : std::max(64, (kmax + 63) / 64 * 64);
}

unsigned wv_grid(int64_t m, int cus) {
  const int64_t wgs = (m + kWvWaves - 1) / kWvWaves;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(wgs, (int64_t)std::max(cus, 1) * 8));
}

}  // namespace

size_t wvote_sweep_lds_bytes(int kmax, int nk, bool with_truth) {
  const int ch = wv_chunk(kmax);
  return ((size_t)(with_truth ? (nk + 1) / 2 : 0) + (size_t)kWvWaves * wv_wave_doubles(ch)) *
         sizeof(double);
}

void launch_wvote_sweep(const int64_t* idx, const double* dist, int64_t m, int kmax,
                        const int32_t* lab, int64_t idx_base, const int* ks, int nk,
                        int32_t* labels, const int32_t* truth, unsigned long long* correct, int cus,
                        hipStream_t s) {
  if (m <= 0) return;
  const int ch = wv_chunk(kmax);
  const size_t lds = wvote_sweep_lds_bytes(kmax, nk, truth != nullptr);
  hipLaunchKernelGGL(wvote_sweep_kernel, dim3(wv_grid(m, cus)), dim3(kWvWaves * 64), lds, s, idx,
                     dist, m, kmax, lab, idx_base, ks, nk, ch, labels, truth, correct);
}

void launch_wvote_sums(const int64_t* idx, const double* dist, int64_t m, int kmax,
                       const int32_t* lab, int64_t idx_base, int k, int class_cnt, double* wsum,
                       int cus, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(wvote_sums_kernel, dim3(wv_grid(m, cus)), dim3(kWvWaves * 64), 0, s, idx, dist,
                     m, kmax, lab, idx_base, k, class_cnt, wsum);
}

}  // namespace knnk
