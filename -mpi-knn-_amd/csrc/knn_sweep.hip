// knn_sweep.hip -- K sweep: the reference's label at every K of a list from
// one search at kmax = max K (gfx950).
//
// The reference's neighbour order does not depend on K (its std::sort runs
// over all N_train records, cpp:323/366, and the vote scans the first K,
// cpp:324-337), so the label at K is a prefix vote over one ordered top-kmax
// row.  With c_t = #{s <= t : l_s == l_t} (finish_single's formulation) the
// reference keeps the label whose count first strictly exceeds the running
// maximum: position t is a "record" when c_t > max_{s<t} c_s, the running
// maximum grows by exactly one at each record, and the label at K is l at the
// last record before K.  One pass over the row serves every K.
//
// Two kernels, both one wave per query (4 waves per workgroup, a grid-stride
// loop over the queries), the row's labels and counts resident in LDS and
// rows longer than the LDS chunk walked in chunks:
//   sweep_tie_scan_kernel  queues the queries whose label at some K of the
//                          list the reference's order among equal distances
//                          could change (tie_order_matters' rule on each
//                          prefix), for tie_order_kernel / tie_resolve_kernel;
//   sweep_vote_kernel      the prefix votes and the per-K correct counts.
// Neither keeps per-class counters: c_t comes from label compares, so labels
// need no bound.
#include "knn_device.h"

#include <algorithm>

namespace knnk {

namespace {

constexpr int kSweepWaves = 4;      // waves (queries in flight) per workgroup
constexpr int kSweepChunkMax = 1024;  // row entries per LDS chunk (covers k <= kMaxK in one)

__device__ __forceinline__ void sweep_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// inclusive prefix max over the wave's lanes
__device__ __forceinline__ int wave_scan_max_i(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v = max(v, u);
  }
  return v;
}

// label of row entry (global index gi): -1 for an empty slot (idx -1)
__device__ __forceinline__ int sweep_label(const int32_t* __restrict__ lab, int64_t gi,
                                           int64_t idx_base) {
  const int64_t r = gi - idx_base;
  return gi >= 0 && r >= 0 ? lab[r] : -1;
}

// Chunk [a0, a0 + len) of one row: la[t] = label of entry a0 + t, ca[t] = its
// running count c over the WHOLE row prefix (entries of earlier chunks are
// staged through lb, ch entries at a time).  Empty slots count nothing.  One
// wave; ends synchronised.
__device__ void sweep_chunk_counts(const int64_t* __restrict__ irow, const int32_t* __restrict__ lab,
                                   int64_t idx_base, int a0, int len, int ch, int* la, int* ca,
                                   int* lb) {
  const int lane = threadIdx.x & 63;
  for (int t = lane; t < len; t += 64) {
    la[t] = sweep_label(lab, irow[a0 + t], idx_base);
    ca[t] = 0;
  }
  sweep_wave_sync();
  for (int b0 = 0; b0 < a0; b0 += ch) {  // (earlier chunks are full: ch entries)
    for (int s = lane; s < ch; s += 64) lb[s] = sweep_label(lab, irow[b0 + s], idx_base);
    sweep_wave_sync();
    for (int t = lane; t < len; t += 64) {
      const int lt = la[t];
      int c = 0;
      for (int s = 0; s < ch; ++s) c += (lb[s] == lt);
      ca[t] += c;
    }
    sweep_wave_sync();
  }
  for (int t = lane; t < len; t += 64) {
    const int lt = la[t];
    int c = ca[t];
    for (int s = 0; s <= t; ++s) c += (la[s] == lt);
    ca[t] = lt < 0 ? 0 : c;
  }
  sweep_wave_sync();
}

// ------------------------------------------------------------ prefix votes
// labels[j][q] = the vote over the first ks[j] entries of row q (any order of
// ks, duplicates allowed: each lane looks its K up in the chunk's per-prefix
// winners); correct[j] += (label == truth[q]) through per-workgroup LDS
// counters, one global atomic per K per workgroup at the end.
__global__ void __launch_bounds__(kSweepWaves * 64)
sweep_vote_kernel(const int64_t* __restrict__ idx, int64_t m, int kmax,
                  const int32_t* __restrict__ lab, int64_t idx_base, const int* __restrict__ ks,
                  int nk, int ch, int32_t* __restrict__ labels, const int32_t* __restrict__ truth,
                  unsigned long long* __restrict__ correct) {
  extern __shared__ int sweep_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int* acc = sweep_lds;  // [nk] (with truth)
  int* la = sweep_lds + (truth ? nk : 0) + wv * 3 * ch;
  int* ca = la + ch;
  int* lb = ca + ch;
  if (truth) {
    for (int j = tid; j < nk; j += blockDim.x) acc[j] = 0;
    __syncthreads();
  }
  for (int64_t q = (int64_t)blockIdx.x * kSweepWaves + wv; q < m;
       q += (int64_t)gridDim.x * kSweepWaves) {
    const int64_t* irow = idx + q * kmax;
    // K = 0 (max_label stays -1, cpp:324) and rows without neighbours (a
    // non-finite query: idx -1)
    const bool empty = kmax == 0 || irow[0] < 0;
    for (int j = lane; j < nk; j += 64)
      if (empty || ks[j] == 0) labels[(int64_t)j * m + q] = -1;
    if (empty) continue;
    const int tr = truth ? truth[q] : -1;
    int P = 0, Wl = -1;  // running max count / winner before this chunk
    for (int a0 = 0; a0 < kmax; a0 += ch) {
      const int len = min(ch, kmax - a0);
      sweep_chunk_counts(irow, lab, idx_base, a0, len, ch, la, ca, lb);
      for (int t0 = 0; t0 < len; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < len;
        const int c = valid ? ca[t] : 0;
        const int pm = max(wave_scan_max_i(c), P);
        int pe = __shfl_up(pm, 1, 64);
        if (lane == 0) pe = P;
        const bool rec = valid && c > pe;  // c_t strictly exceeds the running max
        const int lr = wave_scan_max_i(rec ? t : -1);
        const int w = lr >= 0 ? la[lr] : Wl;
        if (valid) ca[t] = w;  // winner of the prefix a0 + t + 1
        P = __shfl(pm, 63, 64);
        Wl = __shfl(w, 63, 64);
      }
      sweep_wave_sync();
      for (int j = lane; j < nk; j += 64) {
        const int K = ks[j];
        if (K - 1 < a0 || K - 1 >= a0 + len) continue;
        const int lbl = ca[K - 1 - a0];
        labels[(int64_t)j * m + q] = lbl;
        if (truth && lbl >= 0 && lbl == tr) atomicAdd(&acc[j], 1);
      }
      sweep_wave_sync();
    }
  }
  if (truth) {
    __syncthreads();
    for (int j = tid; j < nk; j += blockDim.x)
      if (acc[j]) atomicAdd(&correct[j], (unsigned long long)acc[j]);
  }
}

// ------------------------------------------------------------ sweep tie scan
// dist / idx: the (dist, idx)-ordered top kmax of each query; flags: the
// search's flags for kmax (KNN_FLAG_TIE_BOUNDARY: dist[kmax-1] == the next
// row's).  Query q is appended to tie_q when the reference's order among
// equal distances could change its label at some K of the list:
//   mode 2: any equal distances in the top kmax, or the boundary bit;
//   mode 1: tie_order_matters' rule on the prefix K, for each K of the list:
//     (bnd && M - m2 <= 2 gin) || (tie4 && m2 == M), where per prefix
//     M   = the running max count (the number of records so far),
//     m2  = the runner-up count: the max of c_t over the non-record entries
//           (an entry of the current winner is always a record) and of the
//           running max just before each record that changed the winner (the
//           class it overtook stays at that count),
//     tie4 = equal adjacent distances with different labels inside the prefix,
//     bnd  = dist[K-1] == dist[K] (K < kmax: read inside the row), gin = the
//           length of the run of equal distances ending at K-1.
__global__ void __launch_bounds__(kSweepWaves * 64)
sweep_tie_scan_kernel(const double* __restrict__ dist, const int64_t* __restrict__ idx,
                      const int32_t* __restrict__ flags, int64_t m, int kmax,
                      const int32_t* __restrict__ lab, int64_t idx_base,
                      const int* __restrict__ ks, int nk, int ch, int mode,
                      int* __restrict__ tie_q, int* __restrict__ tie_cnt) {
  extern __shared__ int sweep_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* la = sweep_lds + wv * 3 * ch;
  int* ca = la + ch;
  int* lb = ca + ch;
  for (int64_t q = (int64_t)blockIdx.x * kSweepWaves + wv; q < m;
       q += (int64_t)gridDim.x * kSweepWaves) {
    const int64_t* irow = idx + q * kmax;
    const double* drow = dist + q * kmax;
    if (kmax == 0 || irow[0] < 0) continue;  // no neighbours (non-finite query)
    const bool bnd_last = (flags[q] & 2) != 0;
    int any = 0;
    if (mode == 2) {
      for (int t = lane + 1; t < kmax; t += 64) any |= drow[t] == drow[t - 1];
      any = wave_or_i(any) | (bnd_last ? 1 : 0);
    } else {
      int P = 0, Wl = -1, Gc = 0, Nc = 0, Tc = 0, Rc = 0, lprev = -1;
      for (int a0 = 0; a0 < kmax; a0 += ch) {
        const int len = min(ch, kmax - a0);
        sweep_chunk_counts(irow, lab, idx_base, a0, len, ch, la, ca, lb);
        for (int t0 = 0; t0 < len; t0 += 64) {
          const int t = t0 + lane, at = a0 + t;
          const bool valid = t < len;
          const int c = valid ? ca[t] : 0;
          const int l = valid ? la[t] : -1;
          const int pm = max(wave_scan_max_i(c), P);  // M of the prefix at + 1
          int pe = __shfl_up(pm, 1, 64);
          if (lane == 0) pe = P;
          const bool rec = valid && c > pe;
          const int lr = wave_scan_max_i(rec ? t : -1);
          const int w = lr >= 0 ? la[lr] : Wl;
          int wp = __shfl_up(w, 1, 64);  // the winner before this entry
          if (lane == 0) wp = Wl;
          const int G = max(wave_scan_max_i(rec && wp != l ? pe : 0), Gc);
          const int N = max(wave_scan_max_i(valid && !rec ? c : 0), Nc);
          const int m2 = max(G, N);
          const double dt = valid ? drow[at] : 0.0;
          const bool eqp = valid && at > 0 && dt == drow[at - 1];
          const int lp = t > 0 ? (valid ? la[t - 1] : -1) : lprev;
          const int T4 = max(wave_scan_max_i(eqp && l != lp ? 1 : 0), Tc);
          const int rs = max(wave_scan_max_i(valid && !eqp ? at : -1), Rc);  // run start
          const bool bnd = valid && (at + 1 < kmax ? dt == drow[at + 1] : bnd_last);
          const int gin = at - rs + 1;
          if (valid) lb[t] = (bnd && pm - m2 <= 2 * gin) || (T4 && m2 == pm);
          P = __shfl(pm, 63, 64);
          Wl = __shfl(w, 63, 64);
          Gc = __shfl(G, 63, 64);
          Nc = __shfl(N, 63, 64);
          Tc = __shfl(T4, 63, 64);
          Rc = __shfl(rs, 63, 64);
        }
        lprev = la[len - 1];  // (read before the next chunk restages la)
        sweep_wave_sync();
        for (int j = lane; j < nk; j += 64) {
          const int K = ks[j];
          if (K - 1 >= a0 && K - 1 < a0 + len) any |= lb[K - 1 - a0];
        }
        sweep_wave_sync();
      }
      any = wave_or_i(any);
    }
    if (any && lane == 0) tie_q[atomicAdd(tie_cnt, 1)] = (int)q;
  }
}

// LDS chunk (row entries) and dynamic LDS bytes of a launch
int sweep_chunk(int kmax, int acc_ints) {
  const int cap = acc_ints > 1024 ? kSweepChunkMax / 2 : kSweepChunkMax;  // <= 64 KB in all
  return std::max(64, std::min(cap, (kmax + 63) / 64 * 64));
}

unsigned sweep_grid(int64_t m, int cus) {
  const int64_t wgs = (m + kSweepWaves - 1) / kSweepWaves;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(wgs, (int64_t)std::max(cus, 1) * 8));
}

}  // namespace

void launch_sweep_tie_scan(const double* dist, const int64_t* idx, const int32_t* flags, int64_t m,
                           int kmax, const int32_t* lab, int64_t idx_base, const int* ks, int nk,
                           int mode, int* tie_q, int* tie_cnt, int cus, hipStream_t s) {
  if (m <= 0 || kmax <= 0 || mode == 0) return;
  const int ch = sweep_chunk(kmax, 0);
  const size_t lds = (size_t)kSweepWaves * 3 * ch * sizeof(int);
  hipLaunchKernelGGL(sweep_tie_scan_kernel, dim3(sweep_grid(m, cus)), dim3(kSweepWaves * 64), lds, s,
                     dist, idx, flags, m, kmax, lab, idx_base, ks, nk, ch, mode, tie_q, tie_cnt);
}

void launch_sweep_vote(const int64_t* idx, int64_t m, int kmax, const int32_t* lab,
                       int64_t idx_base, const int* ks, int nk, int32_t* labels,
                       const int32_t* truth, unsigned long long* correct, int cus, hipStream_t s) {
  if (m <= 0) return;
  const int acc = truth ? nk : 0;
  const int ch = sweep_chunk(kmax, acc);
  const size_t lds = ((size_t)acc + (size_t)kSweepWaves * 3 * ch) * sizeof(int);
  hipLaunchKernelGGL(sweep_vote_kernel, dim3(sweep_grid(m, cus)), dim3(kSweepWaves * 64), lds, s,
                     idx, m, kmax, lab, idx_base, ks, nk, ch, labels, truth, correct);
}

}  // namespace knnk
