// knn_plan.cpp -- the host-side decisions of a search (knn_plan.h): padding
// rules, candidate path, workgroup shape, list geometry, thresholds, tuning
// keys.  No device code and no HIP call: g++ alone compiles this file.
#include "knn_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/knn_amd.h"

namespace knnk {

int pad_dim(int d) {
#define KNN_CASE(v) if (d <= v) return v;
  KNN_DP_LIST(KNN_CASE)
#undef KNN_CASE
  return (d + kStreamDC - 1) / kStreamDC * kStreamDC;  // streamed kernel
}

bool cand_supported(int DP) { return DP > 0 && pad_dim(DP) == DP; }

// bf16x3 path: resident kernel for DP <= 256 (a multiple of 16 in the
// resident list), the S3 stream kernel above it (any multiple of 16).
int pad_dim_bf16x3(int d) {
  const int d16 = (d + 15) / 16 * 16;
  if (d16 > 256) return d16;
  const int DP = pad_dim(d16);
  return (DP <= 256 && DP % 16 == 0) ? DP : -1;
}

bool bf16x3_streamed(int DP) { return DP > 256; }

// fp16 path: resident 16x16x32 kernel, DP % 32 == 0 and <= 256.
int pad_dim_fp16(int d) {
  const int DP = pad_dim((d + 31) / 32 * 32);
  return (DP <= 256 && DP % 32 == 0) ? DP : -1;
}

// int8 path: the resident 16x16x64 kernel, DP a multiple of 64, <= 256
int pad_dim_i8(int d) {
  const int DP = (d + 63) / 64 * 64;
  return DP <= 256 ? DP : -1;
}

// int8 on the 32x32x32 kernel (metric 6): the smallest resident DP >= d
// that is a multiple of 32 (d = 96 -> 96, where 16x16x64 pads to 128)
int pad_dim_i8w(int d) {
  for (int DP : {32, 64, 96, 128, 160, 192, 256})
    if (DP >= d) return DP;
  return -1;
}

// L1 on int8 codes above 256 dims (knn_cand_sad_wide.hip): one ds_read_b128
// of a row is 16 codes, the kernel's step, so any multiple of 16 up to 1024
// (255 * 1024 < 2^24: the sums stay exact floats); d = 784 pads nothing
int pad_dim_i8l1w(int d) {
  return d > 256 && d <= 1024 ? (d + 15) / 16 * 16 : -1;
}

// L1 on 16-bit fixed-point codes (knn_cand_fix16.hip): the resident widths
// that are multiples of 32, up to 256 -- the integer sums stay below 65535 *
// 256 < 2^24, exact as floats
int pad_dim_u16l1(int d) { return pad_dim_i8w(d); }

// ... and above 256 dims (knn_cand_fix16_wide.hip): one ds_read_b128 of a row
// is 8 codes and the query's steps come in pairs, so any multiple of 16 up to
// 1024 (65535 * 1024 < 2^26: exact in the integer accumulators, and within
// fix16_wide_round code units as floats); d = 784 pads nothing
int pad_dim_u16l1w(int d) {
  return d > 256 && d <= 1024 ? (d + 15) / 16 * 16 : -1;
}

// fp16 S3 kernel above 256 dims: any multiple of 32
int pad_dim_fp16_s3(int d) {
  const int DP = (d + 31) / 32 * 32;
  return DP > 256 ? DP : -1;
}

// the wide rescan filter's queries per pass (knn_dims.h): on a gfx950 CU
// (160 KiB) 8 up to DP = 5088, 4 up to 10208, 2 up to 20448, 1 up to 40896
int rescan_wide_queries(int DP, int64_t lds_limit) {
  for (int fqw : {8, 4, 2, 1})
    if ((int64_t)fqw * (DP + 1) * 4 + 128 <= lds_limit) return fqw;
  return 0;
}

// the S3 grouping (s3_map) that n_qt and S admit, the largest up to gq_max
// (a row chunk then serves gq workgroups of the XCD, a query chunk 32 / gq):
// 32, 16, 8, 4, 2, 1, else 0
int s3_group(int n_qt, int S, int gq_max) {
  for (int gq : {32, 16, 8, 4, 2, 1})
    if (gq <= gq_max && n_qt % gq == 0 && S % (32 / gq) == 0) return gq;
  return 0;
}

// Region order of the train images (knn_order.hip): regions for n rows (0:
// train order).  Only where the resident kernels run (d <= 256).  Auto: 64
// regions (at most one per 16K rows) for integer-coded train sets (the int8
// pass) whose image fits the 256 MB MALL with room to spare, and for other
// sets (the fp16 pass) whose fp16 image is at most 512 MB.  With the
// order, a split's query tiles start their streams at different rows and no
// longer share the staged tiles in L2, so a larger image is re-read from
// HBM: the 12.5M x 96 shard ran 12.11 -> 13.87 ms, cfg2 1.342 -> 1.266 ms,
// 1M x 128 x 100K queries 13.16 -> 11.47 ms; the fp16 pass on continuous
// data gained nothing (2.343 / 2.342 ms; profiles/ab_log.md r4i, r4j).
// 1: on at any size, 2..64: that many regions.
constexpr int64_t kOrderMaxImage = 192ll << 20;
// Train sets that are not integer-coded (the fp16 pass, continuous data):
// auto on for fp16 images up to 512 MB.  Round 6, continuous cfg2 (272 MB
// fp16 image): candidate kernel 2.353-2.363 -> 2.170-2.197 ms, rescans 2 ->
// 1 per call, query ordering +17 us per call (profiles/ab_log.md r6h) --
// the wave-uniform fp16 test (KNN_M4_FAST) turned the tight early
// thresholds into skipped slow paths (round 4 measured 1.6 % without it).
constexpr int64_t kOrderMaxImageF16 = 512ll << 20;
// Query tiles start their streams at one of 8 phases of the region chain
// (the first region of their region's eighth), not at their own region:
// tiles of one phase share the staged tiles in L2 again -- cfg2 candidate
// 1.212 -> 1.209 ms, L2-miss traffic 1.94 -> 1.34 GB per launch; 4 phases
// 1.250 ms (profiles/ab_log.md r4p).  Tuning key "ophase": -1 auto, 0 the
// tile's own region, N phases.
constexpr int kOrderPhases = 8;
int region_count(const Tuning& tune, bool i8_ok, int64_t n, int d) {
  if (tune.order == 0 || pad_dim_fp16(d) <= 0) return 0;
  int P = (int)std::min<int64_t>(kRegionMax, n / 16384);
  if (tune.order < 0) {
    if (i8_ok && pad_dim_i8(d) > 0)
      return P >= 8 && n * (pad_dim_i8(d) + 16) <= kOrderMaxImage ? P : 0;
    const int DPh = pad_dim_fp16(d);
    return DPh > 0 && P >= 8 && n * (int64_t)(DPh / 2 + 4) * 4 <= kOrderMaxImageF16 ? P : 0;
  }
  if (tune.order >= 2) P = (int)std::min<int64_t>(tune.order, kRegionMax);
  P = (int)std::min<int64_t>(P, n / 256);
  return P >= 2 ? P : 0;
}

// Which int8 kernel: metric 6 (v_mfma_i32_32x32x32_i8, K granularity 32)
// where it issues fewer padded dims than metric 5 (16x16x64, K 64) -- d = 96
// runs 96 dims instead of 128 (configs[3]) -- and at DP = 128 (cfg2), where
// its two 4-entry lists per lane (KNN_I8W_Q4) made it the faster kernel:
// 1.278-1.290 vs 1.290-1.303 ms candidate, all phases 1.466-1.478 vs
// 1.500-1.518 ms (profiles/ab_log.md r5g; its 32x32 MFMA holds the vector
// issue for 8 of 32 cycles, the 16x16x64 one for 8 of 16).  Tuning key
// "i8w": -1 auto, 0 always 16x16x64, 1 always 32x32x32.
int i8_kernel_d(const Tuning& tune, int d) {
  if (tune.i8w >= 0) return tune.i8w > 0 && pad_dim_i8w(d) > 0 ? 6 : 5;
  const int w = pad_dim_i8w(d);
  return w > 0 && (w < pad_dim_i8(d) || w == 128) ? 6 : 5;
}

// Norm blocks (knn_order.hip, launch_norm_blocks): the int8 kernels bound a
// sub-tile by its largest seed instead of reading every row's seed from LDS
// (knn_cand_res.hip), which needs rows of nearly equal norm side by side.
// Auto: integer-coded train sets of more than one window at d <= 256.
bool norm_blocks_on(const Tuning& tune, bool i8_ok, int64_t n, int d) {
  if (tune.nblk == 0 || pad_dim_fp16(d) <= 0 || n < 2) return false;
  if (tune.nblk > 0) return true;
  return i8_ok && (pad_dim_i8(d) > 0 || pad_dim_i8w(d) > 0) && n > kNormWin;
}

// AUTO for the query-resident fp16 kernel (d > 256; profiles/ab_log.md r6v)
constexpr bool kQresAuto = false;

// Seeded thresholds (resident fp16 / int8 kernels with the global threshold).
// Workgroups of the first grid round start with no published threshold: every
// lane inserts nearly every row of its first tiles (a 10K-query batch runs
// ~3 rounds, so a third of its workgroups).  A pre-pass runs the same kernel
// over a strided sample of the train rows (its own image, built once per
// train set: identical operands and seeds for those rows, hence identical
// proxies) and seeds every query's slots with the need-th smallest proxy of
// its sample lists (launch_seed_gthr).  Measured a net loss at cfg2, one
// setting per process (profiles/ab_log.md: r3o_*): int8 candidate phase 1.40-1.43
// ms off, 1.42-1.45 with 8192 rows, 1.44-1.46 with 16384, 1.53 with 32768;
// fp16 2.28 off vs 2.47 -- the sample pass runs cold itself (every lane
// inserts) and a sample-rank threshold saves little next to the thresholds
// the first round publishes within a tile or two.  Off by default; tuning
// key "seed": 0 / -1 off, N = sample rows (experiments).

static int64_t seed_rows(const PlanIn& in) {
  // (the sample image takes train rows by stride: train order only)
  if (in.tune.seed <= 0 || in.ord_P || in.ord_nb) return 0;
  const int64_t ns = std::min<int64_t>(in.tune.seed, in.n / 8) / 256 * 256;
  return ns < 4096 ? 0 : ns;
}

// fp16 candidate pass (kernel metric 4): PRECISION_FP16, or AUTO -- at
// d <= 256 for batches of >= 4096 queries (8-wave workgroups of the resident
// kernel), at d > 256 (S3 kernel) always -- until a batch certifies poorly.
// Tuning key "fp16": -1 auto, 0 off, 1 on.
// (W > kQuadMaxW: the R = 4 lists of the 16x16 layouts would overflow too
// often -- AUTO keeps those for the 32x32 bf16x3 kernel with R = 8/16 lists)
constexpr int kQuadMaxW = 64;
static bool use_fp16(const PlanIn& in) {
  if (in.metric != KNN_METRIC_L2) return false;
  const bool streamed = pad_dim_fp16_s3(in.d) > 0;
  if (!streamed && pad_dim_fp16(in.d) <= 0) return false;
  if (in.tune.fp16 >= 0) return in.tune.fp16 > 0;
  if (in.precision == KNN_PRECISION_FP16) return true;
  if (in.precision != KNN_PRECISION_AUTO || in.fp16_off) return false;
  return streamed || (in.m >= 4096 && in.W <= kQuadMaxW);
}

// int8 candidate pass (kernel metric 5): integer-coded train sets (detect_i8)
// at d <= 256 for batches of >= 4096 queries, in AUTO mode only, until a
// batch sends more than 1/16 of its queries to the rescan (queries off the
// train set's grid).  Tuning key "i8": -1 auto, 0 off, 1 on (where possible);
// "fp16" = 1 (an explicit fp16 request) turns it off, "fp16" = 0 does not.
static bool use_i8(const PlanIn& in) {
  if (in.metric != KNN_METRIC_L2 || !in.i8_ok || pad_dim_i8(in.d) <= 0) return false;
  if (in.tune.i8 >= 0) return in.tune.i8 > 0;
  if (in.tune.fp16 == 1) return false;
  if (in.precision != KNN_PRECISION_AUTO || in.i8_off) return false;
  return in.m >= 4096 && in.W <= kQuadMaxW;
}

// L1 on int8 codes (kernel metric 7, knn_cand_sad.hip): integer-coded train
// sets at d <= 256 under the L1 metric.  Tuning key "i8l1": 0 off, 1 on at
// every batch size, -1 auto: use_i8's rule (AUTO precision, batches of >=
// 4096 queries, W <= kQuadMaxW, until a batch sends more than 1/16 of its
// queries to the rescan), gated by kI8L1Auto -- the pass beat the fp32 L1
// kernel's whole call (prep + candidate + re-rank + rescan) far beyond the
// run-to-run spread at both measured shapes: 1M x 10k, d = 128: 88.47-88.71
// -> 11.80-11.83 ms; 40000 x 4096: 1.677-1.688 -> 0.415-0.432 ms
// (profiles/ab_log.md, "l1sad").  "i8" (the L2 pass) does not reach it.
// Value 2: as 1, and at 256 < d <= 1024 the wide form of the pass
// (knn_cand_sad_wide.hip, query codes re-read per tile).  Opt-in only: AUTO
// and 1 leave those widths on the fp32 stream kernel.
constexpr bool kI8L1Auto = true;
static bool use_i8l1_wide(const PlanIn& in) {
  return in.metric == KNN_METRIC_L1 && in.i8_ok && in.tune.i8l1 == 2 && pad_dim_i8l1w(in.d) > 0;
}
static bool use_i8l1(const PlanIn& in) {
  if (in.metric != KNN_METRIC_L1 || !in.i8_ok || pad_dim_i8w(in.d) <= 0) return false;
  if (in.tune.i8l1 >= 0) return in.tune.i8l1 > 0;
  if (!kI8L1Auto || in.precision != KNN_PRECISION_AUTO || in.i8_off) return false;
  return in.m >= 4096 && in.W <= kQuadMaxW;
}

// L1 on 16-bit fixed-point codes (kernel metric 8, knn_cand_fix16.hip): any
// train set at d <= 256 under the L1 metric.  Tuning key "u16l1": 0 off (the
// default), 1 on at every batch size.  Opt-in only: AUTO never chooses it
// (DESIGN.md §4 has the measurement a change of AUTO would rest on).  Where
// "i8l1" puts an integer-coded train set on the exact byte-code pass (metric
// 7, either form), that pass wins: plan_search asks use_i8l1 first.
static bool use_u16l1(const PlanIn& in) {
  return in.metric == KNN_METRIC_L1 && in.tune.u16l1 == 1 && pad_dim_u16l1(in.d) > 0;
}

// The same pass at 256 < d <= 1024 (its wide form, knn_cand_fix16_wide.hip:
// query codes re-read per tile, sums rounded to float within a bounded term).
// Tuning key "u16l1w": 0 off (the default), 1 on at every batch size.  Opt-in
// only, and a key of its own: "u16l1" moves no call above 256 dims.  Where
// "i8l1" = 2 puts an integer-coded train set on the exact byte-code pass
// (metric 7 wide), that pass wins: plan_search asks use_i8l1_wide first.
static bool use_u16l1_wide(const PlanIn& in) {
  return in.metric == KNN_METRIC_L1 && in.tune.u16l1w == 1 && pad_dim_u16l1w(in.d) > 0;
}

static bool use_bf16x3(const PlanIn& in) {
  if (in.metric != KNN_METRIC_L2) return false;
  if (in.precision == KNN_PRECISION_FP32) return false;
  return pad_dim_bf16x3(in.d) > 0;  // AUTO and BF16X3 (where supported)
}

// The resident kernel's instantiated variants in the default build
// (knn_cand_res.hip, res_variant, which refuses the launch of any other): a
// variant build that instantiates more extends this with it.
static bool resident_variant(int DP, int R, int M, int NW) {
  // metric 7 (knn_cand_sad.hip): DP of pad_dim_i8w, R in {8, 16}, 4 or 8 waves;
  // its wide form (knn_cand_sad_wide.hip) takes DP at run time
  if (M == 7)
    return (pad_dim_i8w(DP) == DP || pad_dim_i8l1w(DP) == DP) && (R == 8 || R == 16) &&
           (NW == 4 || NW == 8);
  // metric 8 (knn_cand_fix16.hip): DP of pad_dim_u16l1, R in {8, 16}, 4 waves,
  // or 8 up to DP = 128 (the resident query takes DP / 2 registers); its wide
  // form (knn_cand_fix16_wide.hip) takes DP at run time, 4 or 8 waves
  if (M == 8 && DP > 256)
    return pad_dim_u16l1w(DP) == DP && (R == 8 || R == 16) && (NW == 4 || NW == 8);
  if (M == 8)
    return pad_dim_u16l1(DP) == DP && (R == 8 || R == 16) && (NW == 4 || (NW == 8 && DP <= 128));
  return (M != 2 || DP % 16 == 0) && (M != 1 || (NW == 4 && R != 4)) &&
         (M < 3 || (DP % 32 == 0 && (R == 4 || (M >= 5 && R == 8)) && (NW == 8 || M >= 4))) &&
         (NW != 16 || M == 4) && (M != 5 || (DP % 64 == 0 && (NW == 8 || NW == 4))) &&
         (M != 6 || (NW == 8 && (R == 4 || R == 8)));
}

// Work decomposition of the candidate kernel: S train splits per 128-query
// tile, R list entries per lane.  The grid (n_qt * S workgroups) is sized so
// its last wave of workgroups is nearly full on the resident slots of this
// kernel (occupancy x CUs): a mostly-empty final round costs up to a whole
// workgroup duration.  The union of the 2S lists must hold the C re-rank
// candidates; R grows to 16 when the expected per-list share of C is large.
// Sets p.lps, p.S and p.R from the plan's kernel, tiles and C.
static void choose_geometry(const PlanIn& in, SearchPlan& p) {
  const Tuning& tune = in.tune;
  const int metric = p.kmetric, DP = p.DP, W = in.W, n_qt = p.n_qt;
  const int64_t n_tiles = p.n_tiles;
  int S_hi = (int)std::max<int64_t>(1, std::min<int64_t>(64, n_tiles));
  int bestS = 1, bestR = 8;
  const bool quad = !p.s3 && metric >= 3 && metric <= 5;  // 16x16 layouts (bf16x3, fp16, int8)
  // int8 on 32x32x32: 4 lists of R = 4 per split (two per lane), or 2 of R =
  // 8 (one per lane, tuning "R" = 8)
  // metric 6: 4 lists of R = 4 per query per split (two per lane, one per
  // half of its rows: knn_cand_res.hip, KNN_I8W_Q4), the quad layout of the
  // 16x16 kernels; tuning "R" = 8 selects one list of 8 per lane (2 per
  // query per split, round 4's form)
  const bool pair4 = metric == 6;
  const bool w4 = pair4 && tune.R != 8;
  // (int8: R = 8 quad lists on request, tuning key "R")
  const bool q8 = quad && metric == 5 && tune.R == 8;
  // 16x16 layouts (and w4): 4 lists per query per split
  p.lps = quad || p.s3q || w4 ? 4 : 2;
  const int lps = p.lps;
  // kernel metrics 3, 4 (16x16x32 layout) have R = 4 only; elsewhere R = 4
  // only on request (resident kernel; tuning experiments)
  auto list_len_ok = [&](int R) {
    if (p.s3q && R != 8) return false;
    if (pair4) return R == (w4 ? 4 : 8);
    if (quad) return R == (q8 ? 8 : 4);
    return tune.R ? R == tune.R : R != 4;
  };
  // S3 on 16x16x32 (s3q): R = 8 quad lists, 4 * S * 8 <= kMaxUnion entries
  if (p.s3q) S_hi = std::min(S_hi, kMaxUnion / (4 * 8));
  for (int R : {4, 8, 16}) {
    if (!list_len_ok(R)) continue;
    if (R == 4 && (DP > 256 || metric == 1 || metric == 7 || metric == 8)) continue;
    const int64_t slots = (int64_t)(p.s3q ? in.facts.s3q_blocks_per_cu()
                                          : in.facts.cand_blocks_per_cu(metric, DP, R, p.nw)) *
                          in.cu_count;
    // the union of the lists must hold the C re-rank candidates; with R = 4
    // lists (16x16 layouts) also S >= W, i.e. at most W/4S of the query's
    // top W expected per list: a list holding 5 of them (an overflow ->
    // the query fails certification) then has probability ~C(W,5)/(4S)^5
    int S_lo = std::max(1, (p.C + lps * R - 1) / (lps * R));
    // quad lists: S >= 2W where every split still walks >= 32 tiles (a list
    // then expects at most 1/8 of the query's top W; an overflow, 5 of them in
    // one list, fails the query's certification: 0.35 % of cfg3's 1M queries
    // at S = W, 0.05 % at 2W, 0.007 % at 4W, each an exact rescan); 4W for
    // batches of >= 128K queries, whose many workgroup rounds make the longer
    // walks of fewer splits worth nothing (cfg3: candidate +0.8 %, rescan
    // phase 11.9 -> 1.8 ms); at least S >= W
    if (q8) {
      S_lo = std::max(S_lo, W);  // an 8-entry list holding 8 of the top W: negligible
      S_hi = std::min(S_hi, kMaxUnion / (4 * 8));
    } else if (quad || pair4) {
      const int mult = n_qt >= 512 ? 4 : 2;
      S_lo = std::max(S_lo, std::max<int>(W, (int)std::min<int64_t>(mult * W, n_tiles / 32)));
    }
    // R = 8 needs an expected share of the top W per list (2S lists) of at
    // most 0.8 (S >= W / 1.6): a list overflow (9 of them in one list -> the
    // query fails certification) then has probability < 1e-6 per list; at a
    // share of 1.6 (cfg5, W = 101, S = 32) 1.6 % of the queries failed.
    // Where no such S exists R = 16 runs instead.
    if (R == 8 && !tune.R) {
      const int s8 = p.s3q ? (W * 5 + 15) / 16 : (W * 5 + 7) / 8;  // share W / (lps S) <= 0.8
      if (s8 > S_hi) continue;
      S_lo = std::max(S_lo, s8);
    }
    S_lo = std::min(S_hi, S_lo);
    auto eff_of = [&](int S) {
      const int64_t wg = (int64_t)n_qt * S;
      const int64_t rounds = (wg + slots - 1) / slots;
      return (double)wg / (double)(rounds * slots);
    };
    double best = -1.0;
    for (int S = S_lo; S <= S_hi; S++) best = std::max(best, eff_of(S));
    // smallest S within 2 % of the best fill: fewer, longer lists mean fewer
    // list insertions per tile (the early, insertion-heavy part of each
    // list's stream is paid once per list)
    int bS = S_lo;
    for (int S = S_lo; S <= S_hi; S++)
      if (eff_of(S) >= best - 0.02) { bS = S; break; }
    // S3: prefer a split count that lets the XCD's concurrent workgroups
    // share staged chunks (s3_map; gq 4 over 2 over none) within the same fill
    if (p.s3 && DP > 256) {
      const int gmax = p.s3gq;
      int bq = s3_group(n_qt, bS, gmax);
      for (int S = bS + 1; S <= S_hi && bq < gmax; S++)
        if (eff_of(S) >= best - 0.02 && s3_group(n_qt, S, gmax) > bq) { bS = S; bq = s3_group(n_qt, S, gmax); }
    }
    // L1 on int8 codes over a norm-blocked image (knn_order.hip): a window's
    // sub-tiles in norm order sit one 256-row tile apart (norm_spread), i.e.
    // 2 or 4 of this kernel's tiles, and the rows near a query in L1 have
    // nearly its code norm.  An even S sends such a band to half of the
    // splits (tile mod S keeps its parity) and its lists overflow: 63 of 96
    // queries failed certification at W = 512, n = 20000, d = 48 with S = 44,
    // 26 with S = 64, against 5 in train order (profiles/ab_log.md, "l1kcap").
    // R = 16 has no share rule to absorb that (R = 8 keeps 0.8 per list), so
    // it takes the largest odd S: every split sees the band, over the most
    // lists the union allows.
    if (metric == 7 && in.ord_nb && R == 16 && S_hi >= 3) {
      const int odd = S_hi - (S_hi % 2 == 0);
      if (odd >= S_lo) bS = odd;
    }
    if (tune.S) bS = std::min(tune.S, S_hi);
    bestS = bS;
    bestR = R;
    break;
  }
  p.S = bestS;
  p.R = bestR;
}

SearchPlan plan_search(const PlanIn& in) {
  const Tuning& tune = in.tune;
  const int64_t m = in.m;
  const int W = in.W;
  SearchPlan p{};
  // candidate-pass flavour: kmetric 4 = L2 via fp16 MFMA, 2/3 = bf16x3, else fp32
  p.kmetric = in.metric;
  p.DP = in.DP;
  p.image = IMG_FP32;
  if (use_i8l1(in)) {
    // L1 on the codes of metric 6's plain int8 image, one list per lane as
    // the fp32 L1 kernel
    p.kmetric = 7;
    p.image = IMG_I8;
    p.DP = pad_dim_i8w(in.d);
  } else if (use_i8l1_wide(in)) {
    // the same pass on plain rows of DP code bytes (train order: no region
    // order and no norm blocks above 256 dims)
    p.kmetric = 7;
    p.image = IMG_I8W;
    p.DP = pad_dim_i8l1w(in.d);
  } else if (use_u16l1(in)) {
    // L1 on 16-bit fixed-point codes of the centred rows, its own image; one
    // list per lane as the fp32 L1 kernel
    p.kmetric = 8;
    p.image = IMG_U16;
    p.DP = pad_dim_u16l1(in.d);
  } else if (use_u16l1_wide(in)) {
    // the same pass on tiles of dim slabs (train order: no region order and
    // no norm blocks above 256 dims)
    p.kmetric = 8;
    p.image = IMG_U16W;
    p.DP = pad_dim_u16l1w(in.d);
  } else if (use_i8(in)) {
    p.kmetric = i8_kernel_d(tune, in.d);
    p.image = IMG_I8;
    p.DP = p.kmetric == 6 ? pad_dim_i8w(in.d) : pad_dim_i8(in.d);
  } else if (use_fp16(in)) {
    p.kmetric = 4;
    p.s3h = pad_dim_fp16(in.d) <= 0;  // fp16 on the S3 stream kernel (d > 256)
    p.image = p.s3h ? IMG_FP16_S3 : IMG_FP16;
    p.DP = p.s3h ? pad_dim_fp16_s3(in.d) : pad_dim_fp16(in.d);
  } else if (use_bf16x3(in)) {
    p.kmetric = 2;
    p.image = IMG_BF16X3;
    p.DP = pad_dim_bf16x3(in.d);
  }
  const int DP = p.DP;
  p.s3 = (p.kmetric == 2 && bf16x3_streamed(DP)) || p.s3h;
  // bf16x3 on the 16x16x32 MFMA layout (resident kernel, 8 waves, DP % 32 ==
  // 0): kernel metric 3, R = 4 lists, 4 lists per split.  Tuning key
  // "mfma16": -1 auto (on for batches of >= 4096 queries), 0 off, 1 on.
  const bool m16 = tune.m16 < 0 ? m >= 4096 && W <= kQuadMaxW : tune.m16 > 0;
  if (p.kmetric == 2 && !p.s3 && m16 && DP % 32 == 0) p.kmetric = 3;
  const int kmetric = p.kmetric;
  // waves per workgroup of the resident kernel: 8 (256 queries share each
  // staged tile) when there are enough queries, else 4; the large-d fp32
  // stream kernel always takes 128 queries, the bf16x3 one (S3) 256
  if (p.s3) p.nw = 8;
  // fp16: 4, 8 or 16; int8 16x16x64: 4 or 8 (16x16x64 builds have both)
  else if ((kmetric == 4 || kmetric == 5) && tune.nw) p.nw = tune.nw;
  // int8 32x32x32: 16 waves (512 queries per staged tile) only in builds
  // with KNN_I8W_NW16 (otherwise the launch is refused: no such kernel)
  else if (kmetric == 6 && tune.nw == 16) p.nw = 16;
  // L1 on int8 codes: 4 or 8 (256 queries share each staged tile)
  else if (kmetric == 7) p.nw = tune.nw == 4 || tune.nw == 8 ? tune.nw : (m >= 4096 ? 8 : 4);
  // L1 on 16-bit codes: 8 only up to DP = 128 (no 8-wave resident kernel above
  // it); the wide form re-reads its queries and has both, as metric 7's
  else if (kmetric == 8)
    p.nw = DP > 128 && DP <= 256 ? 4
                                 : (tune.nw == 4 || tune.nw == 8 ? tune.nw : (m >= 4096 ? 8 : 4));
  else if (kmetric >= 3) p.nw = 8;  // (the 16x16 layouts: fp16, bf16x3, int8)
  else if (DP <= 256 && kmetric != 1) p.nw = tune.nw ? std::min(tune.nw, 8) : (m >= 4096 ? 8 : 4);
  else p.nw = 4;
  // queries per wave of the resident kernel (int8: 16 x the build's query
  // blocks); the int8 kernel with 64 queries per wave also runs 4 waves
  // (metrics 7 and 8 at DP > 256 are resident-style kernels too: their own
  // facts, not the stream kernel's 128 queries)
  const bool res = !p.s3 && (DP <= 256 || kmetric == 7 || kmetric == 8);
  p.qpw = res ? in.facts.cand_queries_per_wave(kmetric, DP) : 32;
  p.qpb = p.s3 ? kS3Rows : (res ? p.qpw * p.nw : kQPB);
  p.n_qt = (int)((m + p.qpb - 1) / p.qpb);
  p.m_pad = (int64_t)p.n_qt * p.qpb;
  p.n_pad3 = (in.n + kS3Rows - 1) / kS3Rows * kS3Rows;
  p.trows = in.facts.cand_tile_rows(kmetric, DP);  // rows per tile of the launched kernel
  p.n_tiles = p.s3 ? p.n_pad3 / kS3Rows : in.n_pad / p.trows;
  p.C = (int)std::min<int64_t>(in.n, std::max(2 * W, W + 16));
  p.C = std::min(p.C, kMaxUnion);
  // fp16 S3 on v_mfma_f32_16x16x32_f16 (quad lists of R = 8) where its lists
  // can hold the query's top W (share W / 4S <= 0.8 at S <= 32, i.e. W <= 102)
  // and the train set has that many tiles to split (else the 32x32x16 form,
  // whose R = 16 lists need fewer splits); tuning key "s3q": -1 auto, 0 off
  // (32x32x16), 1 on where feasible
  const int s3q_S = (W * 5 + 15) / 16;
  p.s3q = p.s3h && tune.s3q != 0 && s3q_S <= kMaxUnion / 32 && s3q_S <= p.n_tiles;
  p.s3gq = tune.s3gq > 0 ? tune.s3gq : kS3GqMax;
  choose_geometry(in, p);
  // the query-resident kernel in place of S3's q16 form (same images, lists
  // and thresholds; knn_cand_qres.hip); tuning key "qres": -1 auto (kQresAuto),
  // 0 off, 1 on where supported
  p.qres = p.s3q && in.facts.qres_supported(DP) && (tune.qres < 0 ? kQresAuto : tune.qres > 0);
  p.NL = p.lps * p.S;
  p.C = std::min(p.C, p.NL * p.R);
  // rescan workspace: the fast path serves the first `cap` failed queries
  p.cap = (int)std::min<int64_t>(m, kRescanFastQueries);
  // per-query global thresholds of the resident candidate kernel
  // (tuning switch "ablate" bit 2 turns the exchange off; results stay exact)
  // gk: what the lists publish into gthr (cand_kernel, cand_s3_kernel's q16
  // form): the K-th smallest of the union of a query's lists in a workgroup,
  // 8 groups, with 8K >= W + 5 rows guaranteed below the threshold (K <= 4
  // for the resident kernel's 4-entry lists, so W <= 27; K <= 16 in S3,
  // W <= 123); else, in the resident kernel, the lists' R-th entries in 4
  // groups.  cfg2 (W = 11): K = 2, the candidate pass 3 % faster than K = 3
  // and 2-4 % faster than the list thresholds (in-process A/B,
  // profiles/ab_log.md: r2f_ab_gk, r2g_ab_pair); K = 1 (8 rows < W) sends 5 %
  // of the queries to the rescan.
  // slot groups G (resident kernel): the first grid round of a 10k batch
  // runs only ~6 of the 38 splits of each query tile, so with 8 groups group
  // 7 has published nothing until the second round and tq = max over the
  // slots stays +inf there; with 4 groups (K = (W + 5) / 4, the same G K >=
  // W + 5 rows below tq) every group has a split in round 1: cfg2 candidate
  // -0.5..0.9 %, the 12.5M x 96 shard -0.5 % (profiles/ab_log.md r5n).  Auto:
  // 4 where K stays <= 4 (W <= 11), else 8; tuning "gg" 4 / 8 forces.
  p.G = p.s3 ? kGthrSlots : tune.gg > 0 ? tune.gg : ((W + 5 + 3) / 4 <= 4 ? 4 : kGthrSlots);
  p.gk = (W + 5 + p.G - 1) / p.G;
  if (p.gk > (p.s3 ? 16 : 4)) p.gk = 0;
  if (tune.gk >= 0) p.gk = std::min(tune.gk, p.s3 ? 16 : 4);
  p.ablate = tune.ablate;
  p.use_gthr = (p.s3 ? p.s3q && p.gk > 0 : res) && !(tune.ablate & 4);
  // gthr init (slots of groups without a split stay 0, never the max); the
  // int8 query builder writes it with the operands (ablate bit 5, an
  // experiment: keep the previous call's final thresholds -- valid only for
  // a repeat of the same queries; measures what perfect seeds would save)
  p.gthr_init = p.use_gthr && !(tune.ablate & 32);
  p.active = std::min(p.S, p.gk ? p.G : 4);
  p.gmask = p.gk ? p.G - 1 : 3;
  p.qblk = tune.qblk > 0 ? std::min(tune.qblk, p.n_qt) : 0;
  // region order of the queries (resident kernels, metrics 4-6; knn_order.hip)
  // (metric 7 takes its queries in call order and starts every stream at the
  // split's first tile: a train set laid out by region or in norm blocks is
  // just another row order to it -- lists carry image positions either way)
  // (metric 8 likewise)
  p.query_order = in.ord_P > 0 && tune.order != 0 && !p.s3 && kmetric >= 4 && kmetric < 7 && DP <= 256;
  p.ophase = std::min(tune.ophase < 0 ? kOrderPhases : tune.ophase, in.ord_P);
  // the int8 image's chunks are swizzled for the 16x16x64 kernel, plain for
  // 32x32x32; the fp16 image's as tuning "xhswz" says (only the metric 4 and
  // 5 kernels read xsw)
  p.i8_swz = kmetric >= 6 ? 0 : 1;
  p.xsw = kmetric >= 5 ? p.i8_swz : tune.xhswz != 0;
  // the int8 rescan filter (metric 6's plain image; knn_select.hip)
  // (tuning key "i8resc": -1 / 1 auto, 0 every failed query on the fp32 filter)
  p.i8resc = tune.i8resc != 0 && kmetric == 6 && DP <= 256 && DP % 16 == 0;
  p.seed_rows = p.gthr_init && (kmetric == 4 || kmetric == 5) && !p.s3 ? seed_rows(in) : 0;
  // the fast rescan's per-query setup, run by the merge on the queries it
  // fails (timing-only ablations leave every query uncertified: none then)
  p.abl = tune.ablate & 27;
  // launch_cand records the "cand" events with the kernel's own dispatch
  // (hipExtLaunchKernelGGL), so that phase is the kernel alone (the seed pass
  // and threshold fill fall into "prep"); the streamed kernels get separate
  // event records around them
  p.ev_ext = (!p.s3 || p.qres) && in.timed;
  // the deferred AUTO decision reads done_ev and h_counts, which belong to
  // the LAST call: it is armed by an fp16 call and dropped by any other
  // (a later fp16 call re-arms it with its own count)
  p.auto_arm = !p.abl && ((kmetric == 4 && in.precision == KNN_PRECISION_AUTO && tune.fp16 < 0) ||
                          ((kmetric == 5 || kmetric == 6) && tune.i8 < 0) ||
                          (kmetric == 7 && tune.i8l1 < 0));
  p.ok = true;
  if (p.qres)
    snprintf(p.kernel, sizeof p.kernel, "cand_qres_kernel<%d>", DP / 32);
  else if (p.s3)
    snprintf(p.kernel, sizeof p.kernel, "cand_s3_kernel<%d,%s,%s>", p.R, p.s3h ? "true" : "false",
             p.s3q ? "true" : "false");
  else if (kmetric == 7) {
    if (DP > 256)
      snprintf(p.kernel, sizeof p.kernel, "cand_sad_wide_kernel<%d,%d>", p.R, p.nw);
    else
      snprintf(p.kernel, sizeof p.kernel, "cand_sad_kernel<%d,%d,%d>", DP, p.R, p.nw);
    p.ok = resident_variant(DP, p.R, kmetric, p.nw);
  } else if (kmetric == 8) {
    if (DP > 256)
      snprintf(p.kernel, sizeof p.kernel, "cand_fix16_wide_kernel<%d,%d>", p.R, p.nw);
    else
      snprintf(p.kernel, sizeof p.kernel, "cand_fix16_kernel<%d,%d,%d>", DP, p.R, p.nw);
    p.ok = resident_variant(DP, p.R, kmetric, p.nw);
  } else if (DP <= 256) {
    snprintf(p.kernel, sizeof p.kernel, "cand_kernel<%d,%d,%d,%d>", DP, p.R, kmetric, p.nw);
    p.ok = cand_supported(DP) && resident_variant(DP, p.R, kmetric, p.nw);
  } else
    snprintf(p.kernel, sizeof p.kernel, "cand_stream_kernel<%d,%d,%d>", kStreamDC, p.R, kmetric);
  return p;
}

// Relative factor f of the candidate-pass error bound used by the
// certification: |proxy - exact| <= f * (max||x||^2 +
// 2.1 ||q|| max||x||) for L2, f * (||q||_1 + max||x||_1) for L1.
//   kmetric 0 (fp32 MFMA, an fmaf chain of DP+1 terms): gamma_{DP+1} + 5u
//   kmetric 1 (fp32 VALU L1):                           gamma_DP + 3u
//   kmetric 2 (bf16x3): products exact, accumulation of 3DP+1 terms bounded
//     with u' = 2^-23 (covers truncating adders), + 2^-15 for the hi/lo
//     representation error (~3 * 2^-18 relative per product, x2 for -2q).
//   kmetric 4 (fp16): products of the fp16 operands exact in fp32, DP+1
//     accumulated terms with u' = 2^-23.  The operands' representation
//     error is measured (train: TrainDev::dxmax, queries: by the merge from
//     the operands themselves) and added by the merge with the seed's own
//     rounding and the fp16 subnormal-range terms.
//   kmetric 8 (16-bit fixed-point L1): the integer sums are exact; the
//     coding error itself is measured (the merge adds 2^-e (Dq + Dx),
//     ProxyScale::u16dx).  What remains is fp64 rounding, relative to ||q -
//     mu||_1 + max||x - mu||_1 >= the distance: v - mu before the coding (u64
//     = 2^-53 per element, on both sides) and the reference's own loop (a
//     subtraction and DP - 1 additions: gamma_DP) -- (DP + 4) u64, doubled.
//     (Above 256 dims the sums' conversion to float adds fix16_wide_round(DP)
//     code units, which the host folds into ProxyScale::u16dx.)
double err_factor(int kmetric, int DP) {
  if (kmetric == 7) return 0.0;  // integer sums of code differences: exact
  if (kmetric == 8) return 2.0 * (DP + 4) * std::ldexp(1.0, -53);
  const double u = std::ldexp(1.0, -24);
  if (kmetric == 4) {
    const double u2 = std::ldexp(1.0, -23);
    const int n = DP + 1;
    return n * u2 / (1.0 - n * u2) * 1.02;
  }
  if (kmetric == 2 || kmetric == 3) {  // bf16x3 on either MFMA shape
    const double u2 = std::ldexp(1.0, -23);
    const int n = 3 * DP + 1;
    return (n * u2 / (1.0 - n * u2) + std::ldexp(1.0, -15)) * 1.02;
  }
  const int n = kmetric == 0 ? DP + 1 : DP;
  const double gam = n * u / (1.0 - n * u);
  return (gam + (kmetric == 0 ? 5.0 : 3.0) * u) * 1.01;
}

// Tuning keys: the accepted values are a range [lo, hi] or, with `set`, the
// listed values (0-terminated after the first entry).
namespace {
struct TuneKey {
  const char* key;
  int Tuning::*field;
  int64_t lo, hi;
  const int* set;
  const char* err;
};
constexpr int kSetR[] = {0, 4, 8, 16, 0};
constexpr int kSetS3gq[] = {0, 1, 2, 4, 8, 16, 32, 0};
constexpr int kSetGg[] = {-1, 4, 8, 0};
const TuneKey kTuneKeys[] = {
    {"fp16", &Tuning::fp16, -1, 1, nullptr, "fp16 must be -1, 0 or 1"},
    {"mfma16", &Tuning::m16, -1, 1, nullptr, "mfma16 must be -1, 0 or 1"},
    {"R", &Tuning::R, 0, 0, kSetR, "R must be 0 (auto), 4, 8 or 16"},
    {"nw", &Tuning::nw, 0, 0, kSetR, "nw must be 0, 4, 8 or 16 (16: fp16 16x16x32 only)"},
    // timing experiments only: results become invalid
    {"ablate", &Tuning::ablate, INT64_MIN, INT64_MAX, nullptr, ""},
    {"S", &Tuning::S, 0, 64, nullptr, "S must be 0 (auto) .. 64"},
    {"qres", &Tuning::qres, -1, 1, nullptr, "qres must be -1, 0 or 1"},
    {"s3q", &Tuning::s3q, -1, 1, nullptr, "s3q must be -1, 0 or 1"},
    {"xhswz", &Tuning::xhswz, 0, 1, nullptr, "xhswz must be 0 or 1"},
    {"i8", &Tuning::i8, -1, 1, nullptr, "i8 must be -1, 0 or 1"},
    {"i8w", &Tuning::i8w, -1, 1, nullptr, "i8w must be -1, 0 or 1"},
    {"i8l1", &Tuning::i8l1, -1, 2, nullptr, "i8l1 must be -1, 0, 1 or 2 (2: also at 256 < d <= 1024)"},
    {"u16l1", &Tuning::u16l1, 0, 1, nullptr, "u16l1 must be 0 or 1"},
    {"u16l1w", &Tuning::u16l1w, 0, 1, nullptr, "u16l1w must be 0 or 1 (1: at 256 < d <= 1024)"},
    {"s3gq", &Tuning::s3gq, 0, 0, kSetS3gq, "s3gq must be 0 (auto) or 1, 2, 4, 8, 16, 32"},
    {"ophase", &Tuning::ophase, -1, kRegionMax, nullptr, "ophase must be -1 (auto) .. 64"},
    {"order", &Tuning::order, -1, kRegionMax, nullptr,
     "order must be -1 (auto), 0, 1 or 2..64 regions"},
    {"qblk", &Tuning::qblk, 0, 1 << 20, nullptr, "qblk must be 0 (split-major) or >= 1"},
    {"i8resc", &Tuning::i8resc, -1, 1, nullptr, "i8resc must be -1 (auto), 0 or 1"},
    {"gg", &Tuning::gg, 0, 0, kSetGg, "gg must be -1 (auto), 4 or 8"},
    {"nblk", &Tuning::nblk, -1, 3, nullptr, "nblk must be -1 (auto), 0, 1, 2 or 3"},
    {"ties", &Tuning::ties, 0, 2, nullptr, "ties must be 0, 1 or 2"},
    {"gk", &Tuning::gk, -1, 16, nullptr, "gk must be -1 (auto) .. 16"},
};
}  // namespace

int set_tuning(Tuning& t, const char* key, int64_t value, const char** err) {
  *err = nullptr;
  if (!strcmp(key, "seed")) {  // the one 64-bit key
    if (value < -1) return *err = "seed must be 0 / -1 (off) or N = sample rows", KNN_ERR_ARG;
    t.seed = value;
    return KNN_OK;
  }
  for (const TuneKey& k : kTuneKeys) {
    if (strcmp(key, k.key)) continue;
    bool ok = value >= k.lo && value <= k.hi;
    if (k.set) {
      ok = value == k.set[0];
      for (const int* v = k.set + 1; *v && !ok; ++v) ok = value == *v;
    }
    if (!ok) return *err = k.err, KNN_ERR_ARG;
    t.*k.field = (int)value;
    return KNN_OK;
  }
  return KNN_ERR_ARG;
}

}  // namespace knnk
