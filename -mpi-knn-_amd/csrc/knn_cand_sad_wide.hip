// knn_cand_sad_wide.hip -- kernel metric 7 at 256 < DP <= 1024: the L1
// candidate pass on int8 codes (knn_cand_sad.hip) for rows whose query codes
// do not fit a lane's registers (196 dwords at d = 784).
//
// The arithmetic, the sign flip and the exactness argument are those of the
// narrow kernel: the integer sum of absolute code differences is 2^s times
// the reference's L1 distance, at most 255 * 1024 = 261120 < 2^24, an exact
// float; lists, selection, thresholds and merge are unchanged.
//
// Operands: plain rows of DP code bytes (launch_prep_i8_rows: train order,
// zero codes in the pad dims, n_pad rows) and the query codes in step-major
// order (launch_prep_i8_queries, wide form): the 16 codes of step c (dims
// 16 c .. 16 c + 15) of query j of 32-query group g at uint4 index
// (g * CPR + c) * 32 + j, CPR = DP / 16, so a wave's load of one step is 512
// contiguous bytes.
//
// Lane (j = lane & 31, h = lane >> 5) of wave w owns query j of the wave and
// the rows (i & 3) + 8 (i >> 2) + 4h of the tile, as the narrow kernel: one
// staged tile is one 32-row sub-tile (a split's 64-row tile is two of them,
// one after the other), staged through registers (sign flip on the
// way) into one of two LDS buffers at a row stride of DP bytes, the tile
// after it in flight behind the compute, one barrier per tile.  The loop
// order is tile -> dim chunk -> rows: per chunk of 64 dims the lane loads 4
// uint4 of its query's codes from global memory (L2: a workgroup's queries
// are 100-200 KB, read once per tile by every split), flips them, and walks
// its 16 rows with one ds_read_b128 and four v_sad_u8 per 16 dims into 16
// integer accumulators; the chunk after it is loaded before the walk.  Per
// tile a lane issues DP / 16 global loads against DP ds_read_b128 and 4 DP
// v_sad_u8 (one query dword per 16 v_sad_u8).  After the last chunk the
// sums are converted and selected once (select_block).  DP is a run-time
// argument: one instantiation per (R, NW).
#include "knn_cand_codes.h"

namespace knnk {

constexpr int kSadWideRows = kTR;   // rows per staged tile: one sub-tile
// rows per tile of the split walk (cand_tile_rows): two staged tiles, so that
// a split's rows come in whole 64-row units as the rescan's per-split masks
// need (knn_select.hip, 64 | trows)
constexpr int kSadWideSplitRows = 2 * kSadWideRows;
constexpr int kSadWideMaxCPR = 64;  // 16-B steps per row at most (DP <= 1024)

template <int R, int NW>
__global__ void __launch_bounds__(NW * 64)
cand_sad_wide_kernel(const uint4* __restrict__ X8, const uint4* __restrict__ Q8,
                     const float* __restrict__ xinit, int CPR, int n_tiles, int S, int n_qt,
                     float* __restrict__ out_v, int* __restrict__ out_i, uint32_t* gthr, int gk,
                     int gmask) {
  constexpr int NT = NW * 64;
  constexpr int TR = kSadWideRows;
  constexpr int NCHMAX = TR * kSadWideMaxCPR;  // chunks per staged tile at most
  constexpr int NPT = NCHMAX / NT;             // chunks per thread at most
  constexpr uint32_t FLIP = 0x80808080u;
  __shared__ uint4 lds[2][NCHMAX];
  __shared__ float sx[2][TR];  // the tile's rows' seeds

  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = bid / n_qt, qt = bid - split * n_qt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int64_t qg = (int64_t)qt * (NW * 32) + wv * 32 + j;
  const int nch = TR * CPR;  // chunks of this tile width

  // the query's codes: step c at qp[c * 32]
  const uint4* qp = Q8 + ((int64_t)qt * NW + wv) * CPR * 32 + j;

  float L[R];
  int I[R];
#pragma unroll
  for (int t = 0; t < R; ++t) {
    L[t] = KNN_INF_F;
    I[t] = -1;
  }
  float thr = KNN_INF_F, tq = KNN_INF_F;
  uint32_t last_pub = kKeyInf;
  uint32_t* gq = gthr ? gthr + qg * kGthrSlots : nullptr;

  // split s walks the 64-row tiles s, s + S, ..., each as two staged tiles
  const int my_nt = split < n_tiles ? 2 * ((n_tiles - split + S - 1) / S) : 0;
  auto tile_of = [&](int it) { return 2 * (split + (it >> 1) * S) + (it & 1); };

  // the image's rows are DP bytes, so a tile is nch contiguous chunks, kept
  // in that order in LDS
  CodeStage<NT, NPT, TR, FLIP, false> stg;
  auto load_tile = [&](int t) {
    stg.load(X8 + (int64_t)t * nch, xinit, t, tid, nch);
  };
  // steps c .. c + 3 of the query's codes (clamped to the row: a step past the
  // end is loaded again and not used)
  auto load_q = [&](uint4 (&qv)[4], int c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) qv[u] = qp[(int64_t)min(c + u, CPR - 1) * 32];
  };

  if (my_nt > 0) {
    load_tile(tile_of(0));
    stg.store(lds[0], sx[0], tid, nch);
  }
  __syncthreads();

  for (int it = 0; it < my_nt; ++it) {
    const int t = tile_of(it);
    const int cur = it & 1;
    const bool xch = gq && it + 1 < my_nt && code_exchange_tile(it);
    uint32_t gmx = 0;
    if (xch) gmx = code_publish_fetch<R>(L, thr, last_pub, gq, gk, h, split, gmask);
    if (it + 1 < my_nt) load_tile(tile_of(it + 1));

    // this lane's 16 rows of the tile, advanced a chunk at a time
    const uint4* rp[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) rp[i] = &lds[cur][(code_row(i) + 4 * h) * CPR];
    uint32_t acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;
    uint4 qn[4];
    load_q(qn, 0);
#pragma unroll 1
    for (int c = 0; c < CPR; c += 4) {
      uint32_t q[16];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        q[4 * u + 0] = qn[u].x ^ FLIP;
        q[4 * u + 1] = qn[u].y ^ FLIP;
        q[4 * u + 2] = qn[u].z ^ FLIP;
        q[4 * u + 3] = qn[u].w ^ FLIP;
      }
      if (c + 4 < CPR) load_q(qn, c + 4);
      const int ns = __builtin_amdgcn_readfirstlane(min(4, CPR - c));
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (u < ns) {
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[i] = code_sad4<SadU8>(rp[i][u], &q[4 * u], acc[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) rp[i] += 4;
    }
    // (the sums are below 2^24: exact floats; a pad row's seed makes it +inf)
    f32x16 av;
    const float* sr = &sx[cur][4 * h];
#pragma unroll
    for (int i = 0; i < 16; ++i) av[i] = (float)acc[i] + sr[code_row(i)];
    select_block<R>(av, t * TR, h, L, I, thr, tq);

    if (xch) tq = __builtin_fminf(tq, code_fetched(gmx));
    if (it + 1 < my_nt) stg.store(lds[cur ^ 1], sx[cur ^ 1], tid, nch);
    // the next tile is in LDS for every wave, and every wave is done reading
    // this one before tile it + 2 is stored over it
    __syncthreads();
  }
  write_lists<R>(out_v, out_i, qg, S, split, h, L, I);
}

bool sad_wide_dp(int DP) { return DP > 256 && DP <= 16 * kSadWideMaxCPR && DP % 16 == 0; }

bool launch_cand_sad_wide(const CandLaunch& c, hipStream_t s) {
  // the host's query tile and train rows must be this kernel's
  if (!sad_wide_dp(c.DP) || c.qpb != c.nw * 32 || !c.xinit || c.n_pad % kSadWideSplitRows) return false;
  return code_dispatch(c.R, c.nw, [&](auto r, auto nw) {
    launch_code_kernel(cand_sad_wide_kernel<r.value, nw.value>, c, s, c.DP / 16,
                       (int)(c.n_pad / kSadWideSplitRows));
  });
}

int sad_wide_blocks_per_cu(int R, int nw) {
  int out = 1;
  code_dispatch(R, nw, [&](auto r, auto w) {
    out = occupancy_of(cand_sad_wide_kernel<r.value, w.value>, w.value * 64);
  });
  return out;
}

int sad_wide_tile_rows() { return kSadWideSplitRows; }

}  // namespace knnk
