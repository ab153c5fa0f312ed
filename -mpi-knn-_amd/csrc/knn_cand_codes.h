// knn_cand_codes.h -- what the L1 candidate passes on integer codes share
// (knn_cand_sad.hip, knn_cand_sad_wide.hip, knn_cand_fix16.hip), each piece
// written once.  Internal; only those three translation units include it.
//
// The three kernels have one structure.  Lane (j = lane & 31, h = lane >> 5)
// of wave w owns query j of the wave and the rows code_row(i) + 4h of every
// 32-row sub-tile, as the fp32 L1 kernel (cand_kernel metric 1): select_block,
// write_lists and the merge's 2-lists-per-split layout apply unchanged.  A
// tile of train codes is staged through registers into one of two LDS
// buffers, rows packed; the tile after it is in flight (global loads) behind
// the current tile's compute, one barrier per tile.  Every ds_read_b128 of the
// row walk has two distinct addresses per wave (one per h), in different
// 16-lane groups: conflict-free at any stride.  Per 16-byte chunk of a (query,
// row) pair the walk issues one ds_read_b128 and four SAD instructions
// (code_sad4) into an integer accumulator; the sums stay below 2^24, exact as
// floats, so the lists, the selection, the thresholds and the merge are those
// of metric 1.
//
// Shared here: the SAD step, the exchange (its schedule, publish-and-fetch, the
// fetched bound), the staging of plain-row images, the launch and the (R, NW)
// dispatch.  Left in the kernels, because as helpers they compile to another
// (equivalent) instruction stream than the text they would replace: the list
// state and the lane indices as structs, the 16-row loop around code_sad4 and
// the sums' conversion as functions, and one body function behind two kernel
// wrappers for the two resident-query kernels (it inverts the tile loop's
// branch).  A helper added here is checked the same way: the kernels' ISA
// does not change.
#pragma once
#include "knn_device.h"

#include <hip/hip_ext.h>

namespace knnk {

// the two SAD instructions: four u8 / two u16 differences per dword
struct SadU8 {
  static __device__ __forceinline__ uint32_t op(uint32_t x, uint32_t q, uint32_t a) {
    return __builtin_amdgcn_sad_u8(x, q, a);
  }
};
struct SadU16 {
  static __device__ __forceinline__ uint32_t op(uint32_t x, uint32_t q, uint32_t a) {
    return __builtin_amdgcn_sad_u16(x, q, a);
  }
};

// row of value i (0..15) of lane (j, h) within its 32-row sub-tile, less 4h
constexpr int code_row(int i) { return (i & 3) + 8 * (i >> 2); }

// tiles at which a workgroup publishes its lists' thresholds and fetches the
// query's slots (cand_kernel's schedule: early at 0, 1, 2, 4, then every 8th)
__device__ __forceinline__ bool code_exchange_tile(int it) {
  if (it < 8) return it == 0 || it == 1 || it == 2 || it == 4;
  return (it & 7) == 7;
}

// The exchange of the global per-query thresholds (cand_kernel: "Global
// per-query threshold"), for a lane's list L with threshold thr: gq is the
// query's slots, lane (j, h) fetches slots 4h .. 4h + 3, the split publishes
// into slot split & gmask.  Publish the lists' threshold (one lane per query,
// only when it improved) and fetch the slots; the largest fetched key is
// returned and read after the tile's compute (code_fetched).  A fetched value
// that is stale is larger: still a valid bound.
template <int R>
__device__ __forceinline__ uint32_t code_publish_fetch(const float (&L)[R], float thr,
                                                       uint32_t& last_pub, uint32_t* gq, int gk,
                                                       int h, int split, int gmask) {
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
  uint32_t gmx = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    gmx = max(gmx, __hip_atomic_load(gq + 4 * h + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return gmx;
}
// the query's bound from what code_publish_fetch returned: lanes l and l ^ 32
// hold the two halves of the query's slots
__device__ __forceinline__ float code_fetched(uint32_t gmx) {
  const auto sw = __builtin_amdgcn_permlane32_swap(gmx, gmx, false, false);
  return key2f(max(sw[0], sw[1]));
}

// A staged tile on its way from an image of plain rows to LDS: the tile is
// nch contiguous chunks from g, kept in that order in LDS; this thread's are
// e = tid, tid + NT, ... (NPT at most), XORed with FLIP on the way in, and the
// seed of row tid (xinit_l1: 0, +inf on pad rows).  WHOLE: nch = NPT NT, known
// when compiling -- no bound check.
template <int NT, int NPT, int TR, uint32_t FLIP, bool WHOLE>
struct CodeStage {
  uint4 st[NPT];
  float sxv = 0.0f;

  __device__ __forceinline__ void load(const uint4* g, const float* xinit, int t, int tid, int nch) {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int e = tid + u * NT;
      if (WHOLE || e < nch) st[u] = g[e];
    }
    if (tid < TR) sxv = xinit[(int64_t)t * TR + tid];
  }
  __device__ __forceinline__ void store(uint4* lds, float* sx, int tid, int nch) const {
#pragma unroll
    for (int u = 0; u < NPT; ++u) {
      const int e = tid + u * NT;
      if (WHOLE || e < nch)
        lds[e] = make_uint4(st[u].x ^ FLIP, st[u].y ^ FLIP, st[u].z ^ FLIP, st[u].w ^ FLIP);
    }
    if (tid < TR) sx[tid] = sxv;
  }
};

// One 16-byte chunk x of a row against the query's four dwords q of the same
// dims, added to a.
template <class Sad>
__device__ __forceinline__ uint32_t code_sad4(const uint4& x, const uint32_t* q, uint32_t a) {
  a = Sad::op(x.x, q[0], a);
  a = Sad::op(x.y, q[1], a);
  a = Sad::op(x.z, q[2], a);
  a = Sad::op(x.w, q[3], a);
  return a;
}

// ------------------------------------------------------------------ host
// One launch of n_qt x S workgroups of c.nw waves; the kernel's arguments are
// (X, Q, xinit, head..., S, n_qt, out_v, out_i, gthr, gk, gmask).
template <class K, class... A>
static void launch_code_kernel(K kernel, const CandLaunch& c, hipStream_t s, A... head) {
  const dim3 grid((unsigned)(c.n_qt * c.S)), block(c.nw * 64);
  if (c.ev_start)
    hipExtLaunchKernelGGL(kernel, grid, block, 0, s, c.ev_start, c.ev_stop, 0, (const uint4*)c.X32,
                          (const uint4*)c.Q32, c.xinit, head..., c.S, c.n_qt, c.out_v, c.out_i,
                          c.gthr, c.gk, c.gmask);
  else
    hipLaunchKernelGGL(kernel, grid, block, 0, s, (const uint4*)c.X32, (const uint4*)c.Q32, c.xinit,
                       head..., c.S, c.n_qt, c.out_v, c.out_i, c.gthr, c.gk, c.gmask);
}

// f(R) / f(R, NW) as integral constants for R in {8, 16}, NW in {4, 8} -- what
// the plan can ask for (knn_plan.cpp, resident_variant); false and no call for
// anything else.
template <int V>
using code_ic = std::integral_constant<int, V>;
template <class F>
static bool code_dispatch_r(int R, F f) {
  if (R == 8) f(code_ic<8>{});
  else if (R == 16) f(code_ic<16>{});
  else return false;
  return true;
}
template <class F>
static bool code_dispatch(int R, int nw, F f) {
  if (nw != 4 && nw != 8) return false;
  return code_dispatch_r(R, [&](auto r) {
    if (nw == 4) f(r, code_ic<4>{});
    else f(r, code_ic<8>{});
  });
}

}  // namespace knnk
