// knn_cand_fix16.hip -- kernel metric 8: the L1 candidate pass on 16-bit
// fixed-point codes of any finite train set (d <= 256), two dims per lane per
// instruction on v_sad_u16.
//
// Codes (knn_prep.hip, launch_prep_u16_*): one power-of-two scale 2^e for
// every dim and the train centre mu_c as the per-dim offset,
//   code_c = clamp(rint(2^e (x_c - mu_c)), -32768, 32767) + 32768,
// e = jx + 5, so the train rows' codes stay within 32768 +- 2^14 (a little
// over half the range) and a query up to max|x - mu| outside the train hull
// still codes without clamping.  The integer sum of absolute code differences
// P satisfies
//   |2^-e P - SUM_c |q_c - x_c|| <= 2^-e (Dq + Dx),
// D = SUM_c |code_c - 32768 - 2^e (v_c - mu_c)| the coding error of the query
// / the row (clamping only enlarges D); the merge measures Dq per query and
// takes the train rows' largest Dx from the image builder.  P <=
// 65535 * 256 < 2^24 is exact as a float, so the lists, the selection, the
// thresholds and the merge are those of the fp32 L1 kernel (cand_kernel metric
// 1) with proxies in units of 2^-e.  Pad dims hold code 0 on both sides and
// add nothing; a pad row's seed (xinit_l1) is +inf.
//
// The structure is knn_cand_codes.h's.  The query's codes stay in DP / 2
// VGPRs -- 128 at DP = 256, which is why the 8-wave form (256 registers per
// lane) exists only up to DP = 128; wider rows run 4 waves (512 per lane).  A
// tile is 64 rows, 128 at DP <= 64 (at most 64 KB of LDS for the two
// buffers), at a row stride of 2 DP bytes.  Per 8 dims of a (query, row) pair
// the loop issues one ds_read_b128 and four v_sad_u16.
#include "knn_cand_codes.h"

namespace knnk {

constexpr int fix16_tile_rows_c(int DP) { return DP > 64 ? 64 : 128; }

template <int DP, int R, int NW>
__global__ void __launch_bounds__(NW * 64)
cand_fix16_kernel(const uint4* __restrict__ X16, const uint4* __restrict__ Q16,
                  const float* __restrict__ xinit, int n_tiles, int S, int n_qt,
                  float* __restrict__ out_v, int* __restrict__ out_i, uint32_t* gthr, int gk,
                  int gmask) {
  constexpr int NT = NW * 64;
  constexpr int TR = fix16_tile_rows_c(DP);  // rows per staged tile
  constexpr int CPR = DP / 8;                // 16-B chunks (8 codes) per row
  constexpr int NCH = TR * CPR;              // chunks per staged tile
  constexpr int NPT = (NCH + NT - 1) / NT;   // chunks per thread
  __shared__ uint4 lds[2][NCH];
  __shared__ float sx[2][TR];  // the tile's rows' seeds (xinit_l1: 0, +inf on pad rows)

  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = bid / n_qt, qt = bid - split * n_qt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int64_t qg = (int64_t)qt * (NW * 32) + wv * 32 + j;

  // the query's codes, resident for the whole kernel
  uint32_t q[DP / 2];
  {
    const uint4* qp = Q16 + qg * CPR;
#pragma unroll
    for (int c = 0; c < CPR; ++c) {
      const uint4 v = qp[c];
      q[4 * c + 0] = v.x;
      q[4 * c + 1] = v.y;
      q[4 * c + 2] = v.z;
      q[4 * c + 3] = v.w;
    }
  }

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

  const int my_nt = split < n_tiles ? (n_tiles - split + S - 1) / S : 0;

  CodeStage<NT, NPT, TR, 0, NCH % NT == 0> stg;
  auto load_tile = [&](int t) {
    stg.load(X16 + (int64_t)t * NCH, xinit, t, tid, NCH);
  };
  auto store_tile = [&](int b) { stg.store(lds[b], sx[b], tid, NCH); };

  if (my_nt > 0) {
    load_tile(split);
    store_tile(0);
  }
  __syncthreads();

  for (int it = 0; it < my_nt; ++it) {
    const int t = split + it * S;
    const int cur = it & 1;
    const bool xch = gq && it + 1 < my_nt && code_exchange_tile(it);
    uint32_t gmx = 0;
    if (xch) gmx = code_publish_fetch<R>(L, thr, last_pub, gq, gk, h, split, gmask);
    if (it + 1 < my_nt) load_tile(t + S);

#pragma unroll 1
    for (int sub = 0; sub < TR / kTR; ++sub) {
      const uint4* base = &lds[cur][(sub * kTR + 4 * h) * CPR];
      uint32_t acc[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0;
#pragma unroll
      for (int c = 0; c < CPR; ++c) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          acc[i] = code_sad4<SadU16>(base[code_row(i) * CPR + c], &q[4 * c], acc[i]);
      }
      // (the sums are below 2^24: exact floats; a pad row's seed makes it +inf)
      f32x16 av;
      const float* sr = &sx[cur][sub * kTR + 4 * h];
#pragma unroll
      for (int i = 0; i < 16; ++i) av[i] = (float)acc[i] + sr[code_row(i)];
      select_block<R>(av, (t * (TR / kTR) + sub) * kTR, h, L, I, thr, tq);
    }

    if (xch) tq = __builtin_fminf(tq, code_fetched(gmx));
    if (it + 1 < my_nt) store_tile(cur ^ 1);
    // the next tile is in LDS for every wave, and every wave is done reading
    // this one before tile it + 2 is stored over it
    __syncthreads();
  }
  write_lists<R>(out_v, out_i, qg, S, split, h, L, I);
}

// Instantiated: DP = pad_dim_u16l1's values, R in {8, 16}, 4 waves, and 8
// waves up to DP = 128 -- what the plan can ask for (knn_plan.cpp,
// resident_variant).
#define KNN_FIX16_NARROW(X) X(32) X(64) X(96) X(128)
#define KNN_FIX16_WIDE(X) X(160) X(192) X(256)

template <class F>
static bool fix16_dispatch(int DP, int R, int nw, F f) {
#define KNN_CASE(v, w) \
  if (DP == v && nw == w) \
    return code_dispatch_r(R, [&](auto r) { f(code_ic<v>{}, r, code_ic<w>{}); });
#define KNN_CASE4(v) KNN_CASE(v, 4)
#define KNN_CASE8(v) KNN_CASE(v, 8)
  KNN_FIX16_NARROW(KNN_CASE4)
  KNN_FIX16_WIDE(KNN_CASE4)
  KNN_FIX16_NARROW(KNN_CASE8)
#undef KNN_CASE8
#undef KNN_CASE4
#undef KNN_CASE
  return false;
}

bool launch_cand_fix16(const CandLaunch& c, hipStream_t s) {
  // the host's query tile must be this kernel's: nw waves x 32 queries, and
  // the image a whole number of tiles
  if (c.qpb != c.nw * 32 || !c.xinit || c.n_pad % 128) return false;
  return fix16_dispatch(c.DP, c.R, c.nw, [&](auto dp, auto r, auto nw) {
    launch_code_kernel(cand_fix16_kernel<dp.value, r.value, nw.value>, c, s,
                       (int)(c.n_pad / fix16_tile_rows_c(dp.value)));
  });
}

int fix16_blocks_per_cu(int DP, int R, int nw) {
  int out = 1;
  fix16_dispatch(DP, R, nw, [&](auto dp, auto r, auto w) {
    out = occupancy_of(cand_fix16_kernel<dp.value, r.value, w.value>, w.value * 64);
  });
  return out;
}

int fix16_tile_rows(int DP) { return fix16_tile_rows_c(DP); }

}  // namespace knnk
