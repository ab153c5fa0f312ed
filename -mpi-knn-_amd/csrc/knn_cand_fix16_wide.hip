// knn_cand_fix16_wide.hip -- kernel metric 8 at 256 < DP <= 1024: the L1
// candidate pass on 16-bit fixed-point codes (knn_cand_fix16.hip) for rows
// whose query codes do not fit a lane's registers (392 dwords at d = 784).
//
// The codes, the scale and the coding-error bound 2^-e (Dq + Dx) are those of
// the narrow kernel.  What changes is the sum's range: P <= 65535 * 1024 <
// 2^26 is exact in the uint32 accumulators, but its conversion to float
// (v_cvt_f32_u32, round to nearest) is not: |fl(P) - P| <= 1 code unit for P
// < 2^25 (DP <= 512) and <= 2 for P < 2^26 (DP <= 1024), half an ulp of the
// binade.  Rounding is monotone, so lists, thresholds and merge stay
// consistent with one another; the host adds that term to the train side's
// coding error (fix16_wide_round, ProxyScale::u16dx).
//
// Operands (knn_prep.hip, launch_prep_u16_*_wide).  A row of DP codes is CPR
// = DP / 8 chunks of 16 bytes (8 codes), cut into dim slabs of at most
// kFix16WideSlabCPR chunks (512 dims): one slab up to DP = 512, two halves
// above it (fix16_wide_slab0).  Train image: 32-row tiles in train order,
// and within a tile the slabs one after the other, each as 32 rows of the
// slab's chunks -- a (tile, slab) unit is contiguous, 32 KB at most, and is
// staged as it lies.  Query codes in step-major order: the 8 codes of step c
// of query j of 32-query group g at uint4 index (g * CPR + c) * 32 + j, so a
// wave's load of one step is 512 contiguous bytes.
//
// Lane (j = lane & 31, h = lane >> 5) of wave w owns query j of the wave and
// the rows (i & 3) + 8 (i >> 2) + 4h of a tile, as the narrow kernel.  The
// loop order is tile -> slab -> dim chunk -> rows.  A unit is staged through
// registers into one of two LDS buffers, the unit after it in flight behind
// the compute, one barrier per unit.  Per chunk of 32 dims the lane loads 4
// uint4 of its query's codes from global memory (L2) and walks its 16 rows
// with one ds_read_b128 and four v_sad_u16 per 8 dims into 16 integer
// accumulators, which carry across the slabs of a tile; the chunk after it is
// loaded before the walk.  After the tile's last slab the sums are converted
// and selected once (select_block).  DP is a run-time argument: one
// instantiation per (R, NW).
#include "knn_cand_codes.h"

namespace knnk {

constexpr int kFix16WideRows = kTR;  // rows per staged unit: one sub-tile
// rows per tile of the split walk (cand_tile_rows): two staged tiles, so that
// a split's rows come in whole 64-row units as the rescan's per-split masks
// need (knn_select.hip, 64 | trows)
constexpr int kFix16WideSplitRows = 2 * kFix16WideRows;
constexpr int kFix16WideMaxCPR = 128;  // 16-B steps per row at most (DP <= 1024)
constexpr int kFix16WideSlabCPR = 64;  // ... and per slab (512 dims)

// waves_per_eu(2): at most 256 registers per lane, so that the two workgroups
// of 4 waves that the CU's LDS admits (64 KB each) also fit its registers; an
// 8-wave workgroup has that limit from its launch bounds
template <int R, int NW>
__global__ void __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2)))
cand_fix16_wide_kernel(const uint4* __restrict__ X16, const uint4* __restrict__ Q16,
                       const float* __restrict__ xinit, int CPR, int n_tiles, int S, int n_qt,
                       float* __restrict__ out_v, int* __restrict__ out_i, uint32_t* gthr, int gk,
                       int gmask) {
  constexpr int NT = NW * 64;
  constexpr int TR = kFix16WideRows;
  constexpr int NCHMAX = TR * kFix16WideSlabCPR;  // chunks per staged unit at most
  constexpr int NPT = NCHMAX / NT;                // chunks per thread at most
  __shared__ uint4 lds[2][NCHMAX];
  __shared__ float sx[2][TR];  // the unit's rows' seeds

  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = bid / n_qt, qt = bid - split * n_qt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int64_t qg = (int64_t)qt * (NW * 32) + wv * 32 + j;
  // the slabs of a row: chunks [0, c0) and [c0, CPR)
  const int c0 = fix16_wide_slab0(CPR);
  const int NS = c0 < CPR ? 2 : 1;

  // the query's codes: step c at qp[c * 32]
  const uint4* qp = Q16 + ((int64_t)qt * NW + wv) * CPR * 32 + j;

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
  const int my_nu = my_nt * NS;  // staged units
  auto tile_of = [&](int it) { return 2 * (split + (it >> 1) * S) + (it & 1); };

  // unit v of the walk: slab v % NS of staged tile v / NS, contiguous in the
  // image and kept in that order in LDS
  CodeStage<NT, NPT, TR, 0, false> stg;
  auto load_unit = [&](int v) {
    const int it = NS == 2 ? v >> 1 : v, sl = NS == 2 ? v & 1 : 0;
    const int t = tile_of(it);
    stg.load(X16 + (int64_t)t * TR * CPR + (sl ? TR * c0 : 0), xinit, t, tid,
             TR * (sl ? CPR - c0 : c0));
  };
  auto store_unit = [&](int v, int b) {
    const int sl = NS == 2 ? v & 1 : 0;
    stg.store(lds[b], sx[b], tid, TR * (sl ? CPR - c0 : c0));
  };

  if (my_nu > 0) {
    load_unit(0);
    store_unit(0, 0);
  }
  __syncthreads();

  int v = 0;
  for (int it = 0; it < my_nt; ++it) {
    const int t = tile_of(it);
    const bool xch = gq && it + 1 < my_nt && code_exchange_tile(it);
    uint32_t gmx = 0;
    if (xch) gmx = code_publish_fetch<R>(L, thr, last_pub, gq, gk, h, split, gmask);
    uint32_t acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0;

    for (int sl = 0; sl < NS; ++sl, ++v) {
      const int cur = v & 1;
      const int cw = sl ? CPR - c0 : c0;  // chunks per row of this slab
      if (v + 1 < my_nu) load_unit(v + 1);

      // steps c .. c + 3 of the slab's part of the query's codes (clamped to
      // the slab: a step past its end is loaded again and not used)
      const uint4* qs = qp + (int64_t)(sl ? c0 : 0) * 32;
      auto load_q = [&](uint4 (&qv)[4], int c) {
#pragma unroll
        for (int u = 0; u < 4; ++u) qv[u] = qs[(int64_t)min(c + u, cw - 1) * 32];
      };
      // this lane's 16 rows of the unit, advanced a chunk at a time
      const uint4* rp[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) rp[i] = &lds[cur][(code_row(i) + 4 * h) * cw];
      uint4 qn[4];
      load_q(qn, 0);
#pragma unroll 1
      for (int c = 0; c < cw; c += 4) {
        uint32_t q[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          q[4 * u + 0] = qn[u].x;
          q[4 * u + 1] = qn[u].y;
          q[4 * u + 2] = qn[u].z;
          q[4 * u + 3] = qn[u].w;
        }
        if (c + 4 < cw) load_q(qn, c + 4);
        const int ns = __builtin_amdgcn_readfirstlane(min(4, cw - c));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u < ns) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = code_sad4<SadU16>(rp[i][u], &q[4 * u], acc[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) rp[i] += 4;
      }

      if (sl + 1 == NS) {
        // (the sums are below 2^26: floats within 2 code units, which the
        // host's bound carries; a pad row's seed makes it +inf)
        f32x16 av;
        const float* sr = &sx[cur][4 * h];
#pragma unroll
        for (int i = 0; i < 16; ++i) av[i] = (float)acc[i] + sr[code_row(i)];
        select_block<R>(av, t * TR, h, L, I, thr, tq);
        if (xch) tq = __builtin_fminf(tq, code_fetched(gmx));
      }
      if (v + 1 < my_nu) store_unit(v + 1, cur ^ 1);
      // the next unit is in LDS for every wave, and every wave is done reading
      // this one before unit v + 2 is stored over it
      __syncthreads();
    }
  }
  write_lists<R>(out_v, out_i, qg, S, split, h, L, I);
}

bool fix16_wide_dp(int DP) {
  return DP > 256 && DP <= 8 * kFix16WideMaxCPR && DP % 16 == 0;
}

bool launch_cand_fix16_wide(const CandLaunch& c, hipStream_t s) {
  // the host's query tile and train rows must be this kernel's
  if (!fix16_wide_dp(c.DP) || c.qpb != c.nw * 32 || !c.xinit || c.n_pad % kFix16WideSplitRows)
    return false;
  return code_dispatch(c.R, c.nw, [&](auto r, auto nw) {
    launch_code_kernel(cand_fix16_wide_kernel<r.value, nw.value>, c, s, c.DP / 8,
                       (int)(c.n_pad / kFix16WideSplitRows));
  });
}

int fix16_wide_blocks_per_cu(int R, int nw) {
  int out = 1;
  code_dispatch(R, nw, [&](auto r, auto w) {
    out = occupancy_of(cand_fix16_wide_kernel<r.value, w.value>, w.value * 64);
  });
  return out;
}

int fix16_wide_tile_rows() { return kFix16WideSplitRows; }

}  // namespace knnk
