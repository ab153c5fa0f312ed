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
// Lane (j = lane & 31, h = lane >> 5) of wave w owns query j of the wave and
// the rows (i & 3) + 8 (i >> 2) + 4h of every 32-row sub-tile, as metric 1:
// select_block, write_lists and the merge's 2-lists-per-split layout apply
// unchanged.  The query's codes stay in DP / 4 VGPRs.  A tile (128 rows, 64
// at DP > 128) is staged through registers into one of two LDS buffers at a
// row stride of DP bytes; the tile after it is in flight (global loads)
// behind the current tile's compute, one barrier per tile.  Every
// ds_read_b128 of the loop has two distinct addresses per wave (one per h),
// in different 16-lane groups: conflict-free at any stride.  Per 16 dims of a
// (query, row) pair the loop issues one ds_read_b128 and four v_sad_u8.
#include "knn_device.h"

#include <hip/hip_ext.h>

namespace knnk {

constexpr int sad_tile_rows_c(int DP) { return DP > 128 ? 64 : 128; }

// tiles at which a workgroup publishes its lists' thresholds and fetches the
// query's slots (cand_kernel's schedule: early at 0, 1, 2, 4, then every 8th)
__device__ __forceinline__ bool sad_exchange_tile(int it) {
  if (it < 8) return it == 0 || it == 1 || it == 2 || it == 4;
  return (it & 7) == 7;
}

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
  // this query's threshold slots (cand_kernel: "Global per-query threshold");
  // lane (j, h) fetches slots 4h .. 4h + 3, the split publishes into slot
  // split & gmask
  uint32_t* gq = gthr ? gthr + qg * kGthrSlots : nullptr;

  const int my_nt = split < n_tiles ? (n_tiles - split + S - 1) / S : 0;

  // staging: chunk e = (row e / CPR, chunk e % CPR) of the tile, this
  // thread's chunks e = tid, tid + NT, ...
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
    // the exchange: publish the lists' threshold (one lane per query, only
    // when it improved) and fetch the slots; they are read after the tile's
    // compute.  A fetched value that is stale is larger: still a valid bound.
    const bool xch = gq && it + 1 < my_nt && sad_exchange_tile(it);
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
          a = __builtin_amdgcn_sad_u8(x.x, q[4 * c + 0], a);
          a = __builtin_amdgcn_sad_u8(x.y, q[4 * c + 1], a);
          a = __builtin_amdgcn_sad_u8(x.z, q[4 * c + 2], a);
          a = __builtin_amdgcn_sad_u8(x.w, q[4 * c + 3], a);
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
static void launch_sad(const CandLaunch& c, hipStream_t s) {
  const int nt = (int)(c.n_pad / sad_tile_rows_c(DP));
  const dim3 grid((unsigned)(c.n_qt * c.S)), block(NW * 64);
  if (c.ev_start)
    hipExtLaunchKernelGGL((cand_sad_kernel<DP, R, NW>), grid, block, 0, s, c.ev_start, c.ev_stop, 0,
                          (const uint4*)c.X32, (const uint4*)c.Q32, c.xinit, nt, c.S, c.n_qt,
                          c.out_v, c.out_i, c.gthr, c.gk, c.gmask);
  else
    hipLaunchKernelGGL((cand_sad_kernel<DP, R, NW>), grid, block, 0, s, (const uint4*)c.X32,
                       (const uint4*)c.Q32, c.xinit, nt, c.S, c.n_qt, c.out_v, c.out_i, c.gthr,
                       c.gk, c.gmask);
}

// Instantiated: DP = pad_dim_i8w's values, R in {8, 16}, NW in {4, 8} -- what
// the plan can ask for (knn_plan.cpp, resident_variant).
#define KNN_SAD_DPS(X) X(32) X(64) X(96) X(128) X(160) X(192) X(256)

template <class F>
static bool sad_dispatch(int DP, int R, int nw, F f) {
  if ((R != 8 && R != 16) || (nw != 4 && nw != 8)) return false;
#define KNN_CASE(v)                                                              \
  if (DP == v) {                                                                 \
    if (R == 8 && nw == 4) f(std::integral_constant<int, v>{}, std::integral_constant<int, 8>{}, std::integral_constant<int, 4>{});        \
    else if (R == 8) f(std::integral_constant<int, v>{}, std::integral_constant<int, 8>{}, std::integral_constant<int, 8>{});             \
    else if (nw == 4) f(std::integral_constant<int, v>{}, std::integral_constant<int, 16>{}, std::integral_constant<int, 4>{});           \
    else f(std::integral_constant<int, v>{}, std::integral_constant<int, 16>{}, std::integral_constant<int, 8>{});                        \
    return true;                                                                 \
  }
  KNN_SAD_DPS(KNN_CASE)
#undef KNN_CASE
  return false;
}

bool launch_cand_sad(const CandLaunch& c, hipStream_t s) {
  // the host's query tile must be this kernel's: nw waves x 32 queries
  if (c.qpb != c.nw * 32 || !c.xinit) return false;
  return sad_dispatch(c.DP, c.R, c.nw, [&](auto dp, auto r, auto nw) {
    launch_sad<dp.value, r.value, nw.value>(c, s);
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
