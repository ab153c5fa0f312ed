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
// Lane (j = lane & 31, h = lane >> 5) of wave w owns query j of the wave and
// the rows (i & 3) + 8 (i >> 2) + 4h of every 32-row sub-tile, as metrics 1
// and 7 (knn_cand_sad.hip, whose structure this kernel keeps): select_block,
// write_lists and the merge's 2-lists-per-split layout apply unchanged.  The
// query's codes stay in DP / 2 VGPRs -- 128 at DP = 256, which is why the
// 8-wave form (256 registers per lane) exists only up to DP = 128; wider rows
// run 4 waves (512 per lane).  A tile (64 rows, 128 at DP <= 64: at most 64 KB
// of LDS for the two buffers) is staged through registers at a row stride of
// 2 DP bytes; the tile after it is in flight (global loads) behind the
// current tile's compute, one barrier per tile.  Every ds_read_b128 of the
// loop has two distinct addresses per wave (one per h), in different 16-lane
// groups: conflict-free at any stride.  Per 8 dims of a (query, row) pair the
// loop issues one ds_read_b128 and four v_sad_u16.
#include "knn_device.h"

#include <hip/hip_ext.h>

namespace knnk {

constexpr int fix16_tile_rows_c(int DP) { return DP > 64 ? 64 : 128; }

// tiles at which a workgroup publishes its lists' thresholds and fetches the
// query's slots (cand_kernel's schedule: early at 0, 1, 2, 4, then every 8th)
__device__ __forceinline__ bool fix16_exchange_tile(int it) {
  if (it < 8) return it == 0 || it == 1 || it == 2 || it == 4;
  return (it & 7) == 7;
}

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
  // this query's threshold slots (cand_kernel: "Global per-query threshold");
  // lane (j, h) fetches slots 4h .. 4h + 3, the split publishes into slot
  // split & gmask
  uint32_t* gq = gthr ? gthr + qg * kGthrSlots : nullptr;

  const int my_nt = split < n_tiles ? (n_tiles - split + S - 1) / S : 0;

  // staging: the tile's chunks are contiguous in the image (rows of CPR
  // chunks, no pad); this thread's chunks e = tid, tid + NT, ...
  uint4 st[NPT];
  float sxv = 0.0f;
  auto load_tile = [&](int t) {
    const uint4* g = X16 + (int64_t)t * NCH;
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int e = tid + u * NT;
      if (NCH % NT == 0 || e < NCH) st[u] = g[e];
    }
    if (tid < TR) sxv = xinit[(int64_t)t * TR + tid];
  };
  auto store_tile = [&](int b) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int e = tid + u * NT;
      if (NCH % NT == 0 || e < NCH) lds[b][e] = make_uint4(st[u].x, st[u].y, st[u].z, st[u].w);
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
    // the exchange: publish the lists' threshold (one lane per query, only
    // when it improved) and fetch the slots; they are read after the tile's
    // compute.  A fetched value that is stale is larger: still a valid bound.
    const bool xch = gq && it + 1 < my_nt && fix16_exchange_tile(it);
    uint32_t gmx = 0;
    if (xch) {
      float mv;
      if (gk) {
        // the gk-th smallest of the union of the query's two lists here
        float u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = L[e];
        mv = union_kth<2>(u, gk);
      } else {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(thr), __float_as_uint(thr),
                                                         false, false);
        mv = __builtin_fminf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      const uint32_t pk = f2key(mv);
      if (h == 0 && pk < last_pub) {
        atomicMin(gq + (split & gmask), pk);
        last_pub = pk;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        gmx = max(gmx, __hip_atomic_load(gq + 4 * h + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
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
        for (int i = 0; i < 16; ++i) {
          const uint4 x = base[((i & 3) + 8 * (i >> 2)) * CPR + c];
          uint32_t a = acc[i];
          a = __builtin_amdgcn_sad_u16(x.x, q[4 * c + 0], a);
          a = __builtin_amdgcn_sad_u16(x.y, q[4 * c + 1], a);
          a = __builtin_amdgcn_sad_u16(x.z, q[4 * c + 2], a);
          a = __builtin_amdgcn_sad_u16(x.w, q[4 * c + 3], a);
          acc[i] = a;
        }
      }
      // (the sums are below 2^24: exact floats; a pad row's seed makes it +inf)
      f32x16 av;
      const float* sr = &sx[cur][sub * kTR + 4 * h];
#pragma unroll
      for (int i = 0; i < 16; ++i) av[i] = (float)acc[i] + sr[(i & 3) + 8 * (i >> 2)];
      select_block<R>(av, (t * (TR / kTR) + sub) * kTR, h, L, I, thr, tq);
    }

    if (xch) {
      // lanes l and l ^ 32 hold the two halves of the query's slots
      const auto sw = __builtin_amdgcn_permlane32_swap(gmx, gmx, false, false);
      tq = __builtin_fminf(tq, key2f(max(sw[0], sw[1])));
    }
    if (it + 1 < my_nt) store_tile(cur ^ 1);
    // the next tile is in LDS for every wave, and every wave is done reading
    // this one before tile it + 2 is stored over it
    __syncthreads();
  }
  write_lists<R>(out_v, out_i, qg, S, split, h, L, I);
}

template <int DP, int R, int NW>
static void launch_fix16(const CandLaunch& c, hipStream_t s) {
  const int nt = (int)(c.n_pad / fix16_tile_rows_c(DP));
  const dim3 grid((unsigned)(c.n_qt * c.S)), block(NW * 64);
  if (c.ev_start)
    hipExtLaunchKernelGGL((cand_fix16_kernel<DP, R, NW>), grid, block, 0, s, c.ev_start, c.ev_stop,
                          0, (const uint4*)c.X32, (const uint4*)c.Q32, c.xinit, nt, c.S, c.n_qt,
                          c.out_v, c.out_i, c.gthr, c.gk, c.gmask);
  else
    hipLaunchKernelGGL((cand_fix16_kernel<DP, R, NW>), grid, block, 0, s, (const uint4*)c.X32,
                       (const uint4*)c.Q32, c.xinit, nt, c.S, c.n_qt, c.out_v, c.out_i, c.gthr,
                       c.gk, c.gmask);
}

// Instantiated: DP = pad_dim_u16l1's values, R in {8, 16}, 4 waves, and 8
// waves up to DP = 128 -- what the plan can ask for (knn_plan.cpp,
// resident_variant).
#define KNN_FIX16_NARROW(X) X(32) X(64) X(96) X(128)
#define KNN_FIX16_WIDE(X) X(160) X(192) X(256)

template <class F>
static bool fix16_dispatch(int DP, int R, int nw, F f) {
  if ((R != 8 && R != 16) || (nw != 4 && nw != 8)) return false;
  using std::integral_constant;
#define KNN_CASE4(v)                                                                      \
  if (DP == v && nw == 4) {                                                               \
    if (R == 8) f(integral_constant<int, v>{}, integral_constant<int, 8>{}, integral_constant<int, 4>{});  \
    else f(integral_constant<int, v>{}, integral_constant<int, 16>{}, integral_constant<int, 4>{});        \
    return true;                                                                          \
  }
#define KNN_CASE8(v)                                                                      \
  if (DP == v && nw == 8) {                                                               \
    if (R == 8) f(integral_constant<int, v>{}, integral_constant<int, 8>{}, integral_constant<int, 8>{});  \
    else f(integral_constant<int, v>{}, integral_constant<int, 16>{}, integral_constant<int, 8>{});        \
    return true;                                                                          \
  }
  KNN_FIX16_NARROW(KNN_CASE4)
  KNN_FIX16_WIDE(KNN_CASE4)
  KNN_FIX16_NARROW(KNN_CASE8)
#undef KNN_CASE4
#undef KNN_CASE8
  return false;
}

bool launch_cand_fix16(const CandLaunch& c, hipStream_t s) {
  // the host's query tile must be this kernel's: nw waves x 32 queries, and
  // the image a whole number of tiles
  if (c.qpb != c.nw * 32 || !c.xinit || c.n_pad % 128) return false;
  return fix16_dispatch(c.DP, c.R, c.nw, [&](auto dp, auto r, auto nw) {
    launch_fix16<dp.value, r.value, nw.value>(c, s);
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
