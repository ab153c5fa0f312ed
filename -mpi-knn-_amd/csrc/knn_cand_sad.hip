// knn_cand_sad.hip -- kernel metric 7: the L1 candidate pass on int8 codes
// (d <= 256), four dims per lane per instruction on v_sad_u8.
//
// For a train set on a grid, x_i = (cent_i + cx_i) / 2^s with integer codes
// cx_i in [-128, 127] (detect_i8), and a query on the same grid, |q_i - x_i| =
// |cq_i - cx_i| / 2^s: the integer sum of absolute code differences is 2^s
// times the reference's L1 distance, exactly (every term and every partial
// sum of the reference's fp64 loop is a multiple of 2^-s below 2^53), so it
// orders the rows as the reference does, equal distances included.  The sum
// is at most 255 * 256 = 65280 < 2^24: exact as a float, so the lists, the
// selection, the thresholds and the merge are those of the fp32 L1 kernel
// (cand_kernel metric 1) with proxies in units of 2^-s and an error bound of 0.
//
// Operands: the unswizzled int8 image of kernel metric 6 (rows of DP + 16
// bytes, DP = pad_dim_i8w(d); the 16 pad bytes -- L2 seeds and sub-tile
// maxima -- are not read) and launch_prep_i8_queries' code rows.  The codes
// are signed and centred, v_sad_u8 is unsigned: flipping the top bit of every
// byte (^ 0x80808080) maps [-128, 127] to [0, 255] and leaves every
// difference unchanged.  The query dwords are flipped once when loaded; the
// train dwords are flipped on their way into LDS, once per staged tile for
// all the workgroup's queries (the image itself stays as the L2 int8 kernels
// read it; a second, unsigned image would cost n (DP + 16) bytes of HBM for
// the same effect).  Zero pad dims are 0x80 on both sides: no contribution.
//
// The structure is knn_cand_codes.h's.  The query's codes stay in DP / 4
// VGPRs; a tile is 128 rows, 64 at DP > 128, at a row stride of DP bytes in
// LDS.  Per 16 dims of a (query, row) pair the loop issues one ds_read_b128
// and four v_sad_u8.
#include "knn_cand_codes.h"

namespace knnk {

constexpr int sad_tile_rows_c(int DP) { return DP > 128 ? 64 : 128; }

template <int DP, int R, int NW>
__global__ void __launch_bounds__(NW * 64)
cand_sad_kernel(const uint4* __restrict__ X8, const uint4* __restrict__ Q8,
                const float* __restrict__ xinit, int n_tiles, int S, int n_qt,
                float* __restrict__ out_v, int* __restrict__ out_i, uint32_t* gthr, int gk,
                int gmask) {
  constexpr int NT = NW * 64;
  constexpr int TR = sad_tile_rows_c(DP);  // rows per staged tile
  constexpr int CPR = DP / 16;             // 16-B chunks of codes per row
  constexpr int RC = CPR + 1;              // chunks per image row (codes | pad)
  constexpr int NCH = TR * CPR;            // chunks per staged tile
  constexpr int NPT = (NCH + NT - 1) / NT; // chunks per thread
  constexpr uint32_t FLIP = 0x80808080u;
  __shared__ uint4 lds[2][NCH];
  __shared__ float sx[2][TR];  // the tile's rows' seeds (xinit_l1: 0, +inf on pad rows)

  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = bid / n_qt, qt = bid - split * n_qt;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int64_t qg = (int64_t)qt * (NW * 32) + wv * 32 + j;

  // the query's codes, flipped to unsigned, resident for the whole kernel
  uint32_t q[DP / 4];
  {
    const uint4* qp = Q8 + qg * CPR;
#pragma unroll
    for (int c = 0; c < CPR; ++c) {
      const uint4 v = qp[c];
      q[4 * c + 0] = v.x ^ FLIP;
      q[4 * c + 1] = v.y ^ FLIP;
      q[4 * c + 2] = v.z ^ FLIP;
      q[4 * c + 3] = v.w ^ FLIP;
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

  // staging: chunk e = (row e / CPR, chunk e % CPR) of the tile, this
  // thread's chunks e = tid, tid + NT, ... (the image's rows carry a pad
  // chunk, so not CodeStage: through it the index arithmetic compiles differently)
  uint4 st[NPT];
  float sxv = 0.0f;
  auto load_tile = [&](int t) {
    const uint4* g = X8 + (int64_t)t * TR * RC;
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int e = tid + u * NT;
      if (NCH % NT == 0 || e < NCH) st[u] = g[(e / CPR) * RC + e % CPR];
    }
    if (tid < TR) sxv = xinit[(int64_t)t * TR + tid];
  };
  auto store_tile = [&](int b) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int e = tid + u * NT;
      if (NCH % NT == 0 || e < NCH)
        lds[b][e] = make_uint4(st[u].x ^ FLIP, st[u].y ^ FLIP, st[u].z ^ FLIP, st[u].w ^ FLIP);
    }
    if (tid < TR) sx[b][tid] = sxv;
  };

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
          acc[i] = code_sad4<SadU8>(base[code_row(i) * CPR + c], &q[4 * c], acc[i]);
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

// Instantiated: DP = pad_dim_i8w's values, R in {8, 16}, NW in {4, 8} -- what
// the plan can ask for (knn_plan.cpp, resident_variant).
#define KNN_SAD_DPS(X) X(32) X(64) X(96) X(128) X(160) X(192) X(256)

template <class F>
static bool sad_dispatch(int DP, int R, int nw, F f) {
#define KNN_CASE(v) \
  if (DP == v) return code_dispatch(R, nw, [&](auto r, auto w) { f(code_ic<v>{}, r, w); });
  KNN_SAD_DPS(KNN_CASE)
#undef KNN_CASE
  return false;
}

bool launch_cand_sad(const CandLaunch& c, hipStream_t s) {
  // the host's query tile must be this kernel's: nw waves x 32 queries
  if (c.qpb != c.nw * 32 || !c.xinit) return false;
  return sad_dispatch(c.DP, c.R, c.nw, [&](auto dp, auto r, auto nw) {
    launch_code_kernel(cand_sad_kernel<dp.value, r.value, nw.value>, c, s,
                       (int)(c.n_pad / sad_tile_rows_c(dp.value)));
  });
}

int sad_blocks_per_cu(int DP, int R, int nw) {
  int out = 1;
  sad_dispatch(DP, R, nw, [&](auto dp, auto r, auto w) {
    out = occupancy_of(cand_sad_kernel<dp.value, r.value, w.value>, w.value * 64);
  });
  return out;
}

int sad_tile_rows(int DP) { return sad_tile_rows_c(DP); }

}  // namespace knnk
