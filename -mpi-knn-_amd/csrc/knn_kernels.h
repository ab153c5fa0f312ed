// knn_kernels.h -- internal launch interface of the HIP kernels (gfx950).
// Not part of the public ABI (see include/knn_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_dims.h"

namespace knncsv {
struct NumTable;  // knn_csv_num.h
}

namespace knnk {

constexpr int kTR = 32;          // train rows per MFMA sub-tile of the resident kernel
constexpr int kResTileRows = 64; // resident kernel: train rows per staged tile (2 sub-tiles)
constexpr int kSortN = 2048;     // rows per exact-rescan chunk / reduce block
constexpr int kMaxK = 1000;      // largest k served (k+1 <= kMaxUnion)
constexpr int kRowAlign = 256;   // train rows are padded to a multiple of this (<= one staged tile)

enum { MODE_SINGLE = 0, MODE_PARTIAL = 1 };

// Output sinks of a search: MODE_SINGLE writes the vote, MODE_PARTIAL the
// exact top-w list with labels (train-sharded building block).
struct Sink {
  int mode;
  int k;                 // neighbours voted / reported (single)
  int w;                 // list length (partial)
  int64_t idx_off;       // added to reported indices
  int32_t* labels;       // single: [m]
  int64_t* idx;          // single: [m*k] (nullable); partial: [m*w]
  double* dist;          // single: [m*k] (nullable); partial: [m*w]
  int32_t* flags;        // single: [m] (nullable)
  int32_t* plab;         // partial: [m*w]
  // single: tied queries appended to tie_q (count in tie_cnt[0]) for the
  // reference-order pass (launch_tie_order): tie_mode 0 none, 1 those whose
  // label the reference's tie order could change, 2 every tied query
  int tie_mode;
  int* tie_q;
  int* tie_cnt;
  // single: 1 = the search neither queues tied queries nor runs the
  // reference-order pass (tie_mode 0 on the device): the K sweep queues them
  // itself from the finished rows (launch_sweep_tie_scan) and runs the pass
  int tie_defer = 0;
};

// Train-set side state resident in HBM.
struct TrainDev {
  const double* X64;     // [n][d] fp64 (reference values)
  const double* mu;      // [d] train column means: the candidate pass's centre
  const int32_t* lab;    // [n]
  const float* X32;      // [n_pad][DP+4] fp32 padded rows (payload | seeds), zero padded
  const float* xinit_l2; // [n_pad] fl32(||x32||^2); +inf on pad rows
  const float* xinit_l1; // [n_pad] 0; +inf on pad rows
  int64_t n, n_pad;
  int d, DP;
  double x2max, x1max;   // max ||x - mu||_2^2, max ||x - mu||_1 over the train rows
  double dxmax;          // max ||fp16 row / 2^jx - (x - mu)||_2 of the fp16 copy (when built)
  int jx;                // candidate operands are 2^jx (x - mu) (knn_prep.hip)
  // Region order (knn_order.hip): row p of every candidate image (X32, the
  // fp16 / bf16 / int8 copies) is train row perm[p]; ipos is the inverse.
  // Null: images in train order.  Candidate lists carry image positions; the
  // merge and the rescan report train rows.
  const int* perm = nullptr;  // [n]
  const int* ipos = nullptr;  // [n]
};

int s3_blocks_per_cu(int R);
// S3 kernel (bf16x3, DP > 256): XT/QT are tile-chunk images made by
// launch_prep_split_tiled, XS the per-row seeds [n_pad]; n_pad and m_pad are
// multiples of kS3Rows.
// gq_max: the largest XCD grouping of query tiles to use (s3_group)
void launch_cand_s3(const unsigned short* XT, const float* XS, const unsigned short* QT, int DP,
                    int64_t n_pad, int R, int S, int n_qt, float* out_v, int* out_i, int ablate,
                    hipStream_t s, int gq_max = kS3GqMax);
// fp64 rows -> bf16 hi/lo tile-chunk images of scale*x (S3 layout); seed_out
// (train only, else null) receives seed_src[row] (+inf on pad rows)
void launch_prep_split_tiled(const double* X64, const double* mu, int64_t n, int d, int DP,
                             int64_t n_pad, double scale, unsigned short* out,
                             const float* seed_src, float* seed_out, hipStream_t s,
                             const int* perm = nullptr);
// fp16 S3 kernel (DP > 256, DP % 32 == 0): XT/QT made by launch_prep_half_tiled
// q16: the v_mfma_f32_16x16x32_f16 form (R = 8 quad lists: [m_pad][4S][8])
// gthr / gk: the global threshold exchange of the q16 form (null / 0: none)
void launch_cand_s3h(const unsigned short* XT, const float* XS, const unsigned short* QT, int DP,
                     int64_t n_pad, int R, int S, int n_qt, float* out_v, int* out_i, int ablate,
                     bool q16, uint32_t* gthr, int gk, hipStream_t s, int gq_max = kS3GqMax);
int s3h_blocks_per_cu(int R);
int s3q_blocks_per_cu();
// query-resident fp16 kernel for d > 256 (knn_cand_qres.hip): the S3 q16
// kernel's outputs from the same images, 2 n_qt workgroup tiles of 128
// queries; false: no instantiation for DP (run S3)
bool qres_supported(int DP);
bool launch_cand_qres(const unsigned short* XT, const float* XS, const unsigned short* QT, int DP,
                      int64_t n_pad, int S, int n_qt, float* out_v, int* out_i, uint32_t* gthr, int gk,
                      hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop);
// fp64 rows -> fp16 S3 tile-chunk images of mult * 2^jx (x - mu) (knn_prep.hip);
// train: seed_out[row] = seed_src[row] (+inf on pad rows) and the running max
// of the rows' squared representation error in dx2max; queries: seed_out =
// dx2max = null, valid[row] <= 0 -> zero operands
void launch_prep_half_tiled(const double* X64, const double* mu, int64_t n, int d, int DP,
                            int64_t n_pad, int jx, double mult, unsigned short* out,
                            const float* seed_src, float* seed_out, const float* valid,
                            unsigned long long* dx2max, hipStream_t s, const int* perm = nullptr);
// train rows per tile of the candidate kernel serving (kernel metric, DP):
// split s of a launch walks tiles s, s + S, ... (rows (r / tile) % S == s)
int cand_tile_rows(int metric, int DP);
int cand_blocks_per_cu(int metric, int DP, int R, int nw);  // resident workgroups per CU
int cand_queries_per_wave(int metric, int DP);  // resident kernel: queries per wave

// metric: 0 = L2 fp32 MFMA, 1 = L1 fp32 VALU, 2 = L2 bf16x3 MFMA (32x32x16),
// 3 = L2 bf16x3 on 16x16x32, 4 = L2 fp16 on 16x16x32, 5 = L2 int8 on
// 16x16x64, 6 = L2 int8 on 32x32x32 (see knn_cand_res.hip), 7 = L1 on int8
// codes, v_sad_u8 (knn_cand_sad.hip: X32 = metric 6's int8 image, Q32 = the
// int8 query codes, xinit = xinit_l1), 8 = L1 on 16-bit fixed-point codes,
// v_sad_u16 (knn_cand_fix16.hip: X32 = launch_prep_u16_train's rows, Q32 =
// launch_prep_u16_queries' rows, xinit = xinit_l1)
struct CandLaunch {
  int metric, DP, R, S, n_qt;
  int64_t n_pad;
  const float* X32;
  const float* xinit;
  const float* Q32;
  float* out_v;
  int* out_i;
  int ablate;   // timing-only ablation bits (0 in production)
  int nw;       // resident kernel: waves per workgroup, 4, 8 or 16
  int qpb;      // resident kernel: queries per workgroup the host laid out (nw x
                // queries per wave; checked against the kernel before launch)
  uint32_t* gthr;  // resident kernel: per-query global thresholds [m_pad][kGthrSlots] (keys)
  int xsw;         // fp16 (metric 4): the train image's chunks are swizzled (xh_swz)
  int gk;          // what a list group publishes into gthr (see cand_kernel): 0 = the
                   // lists' R-th entries into split % 4, K = 1..4: the K-th smallest of
                   // the union of the query's lists in the workgroup into split % 8
  // resident kernel, region order: qstart[p] = the image position where the
  // region of the query at position p starts; each workgroup starts its
  // split's stream at the first of its tiles at or after qstart[first
  // query of the tile] (null: at the split's first tile)
  const int* qstart = nullptr;
  int gmask = 7;   // slot groups of gthr - 1: a split publishes into slot split & gmask
  int qblk = 0;    // workgroup order: 0 split-major, B: query blocks of B tiles (cand_kernel)
  // "cand" timing events recorded by the resident kernel's own dispatch
  // (hipExtLaunchKernelGGL), so the phase is the kernel's execution as
  // rocprofv3 times it (profiles/ab_log.md r6u); null: none
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
};
constexpr uint32_t kGthrInit = 0xFF800000u;  // order-preserving key of +inf
// gthr init: slots [0, active) = +inf keys, the rest 0 (never the max)
void launch_fill_gthr(uint32_t* g, int64_t m_pad, int active, hipStream_t s);
// seeded thresholds: the need-th smallest of each query's U pre-pass list entries
void launch_seed_gthr(const float* v, int64_t m_pad, int U, int need, int active, uint32_t* g,
                      hipStream_t s);

// Candidate-pass operands are centred on the train column means mu (see knn_prep.hip).
int col_mean_blocks(int64_t n);  // rows of the `partial` scratch (x d doubles)
void launch_col_mean(const double* X64, int64_t n, int d, double* partial, double* mu,
                     hipStream_t s);
void launch_absmax(const double* X64, const double* mu, int64_t n, int d, unsigned long long* out,
                   unsigned long long* nonfinite, hipStream_t s);
void launch_label_check(const int32_t* lab, int64_t n, int class_cnt, unsigned long long* bad,
                        hipStream_t s);
// perm (every train image builder): image row p <- train row perm[p] (null: p)
void launch_prep_train(const double* X64, const double* mu, int64_t n, int d, int DP,
                       int64_t n_pad, int jx, float* X32, float* xl2, float* xl1,
                       unsigned long long* stats, hipStream_t s, const int* perm = nullptr);
void launch_query_check(const double* Q64, const double* mu, int64_t m, int d, int64_t m_pad,
                        double scale, int jx, double limit, float* valid, hipStream_t s);
void launch_prep_queries(const double* Q64, const double* mu, int64_t m, int d, int DP,
                         int64_t m_pad, double scale, int jx, float* Q32, hipStream_t s);
// false: no kernel instantiated for this (DP, R, metric, nw) -- nothing launched
bool launch_cand(const CandLaunch& c, hipStream_t s);
// kernel metric 7 (knn_cand_sad.hip; reached through launch_cand and the
// cand_* queries above)
bool launch_cand_sad(const CandLaunch& c, hipStream_t s);
int sad_blocks_per_cu(int DP, int R, int nw);
int sad_tile_rows(int DP);
// kernel metric 7 at 256 < DP <= 1024 (knn_cand_sad_wide.hip): X32 = the plain
// code rows of launch_prep_i8_rows, Q32 = the step-major query codes of
// launch_prep_i8_queries' wide form
bool sad_wide_dp(int DP);
bool launch_cand_sad_wide(const CandLaunch& c, hipStream_t s);
int sad_wide_blocks_per_cu(int R, int nw);
int sad_wide_tile_rows();
// kernel metric 8 (knn_cand_fix16.hip; reached through launch_cand and the
// cand_* queries above): DP of pad_dim_u16l1
bool launch_cand_fix16(const CandLaunch& c, hipStream_t s);
int fix16_blocks_per_cu(int DP, int R, int nw);
int fix16_tile_rows(int DP);
// kernel metric 8 at 256 < DP <= 1024 (knn_cand_fix16_wide.hip): X32 = the
// tiles of dim slabs of launch_prep_u16_train_wide, Q32 = the step-major query
// codes of launch_prep_u16_queries_wide.  Its proxies are floats within
// fix16_wide_round(DP) code units of the integer sums (knn_dims.h).
bool fix16_wide_dp(int DP);
bool launch_cand_fix16_wide(const CandLaunch& c, hipStream_t s);
int fix16_wide_blocks_per_cu(int R, int nw);
int fix16_wide_tile_rows();
// The narrow kernel's operands (knn_prep.hip): rows of DP unsigned 16-bit codes
// clamp(rint(2^e (x - mu)), -32768, 32767) + 32768, zero codes in the pad dims
// and on pad rows.  Train: n_pad rows, image row p <- train row perm[p];
// dmax receives the largest row sum of |code - 32768 - 2^e (x - mu)| (code
// units, fp64 bits, atomicMax: clear it first).  Queries: m_pad rows, a query
// with valid[q] <= 0 gets zero codes.
void launch_prep_u16_train(const double* X64, const double* mu, int64_t n, int d, int DP,
                           int64_t n_pad, int e, unsigned short* out, unsigned long long* dmax,
                           hipStream_t s, const int* perm = nullptr);
void launch_prep_u16_queries(const double* Q64, const double* mu, int64_t m, int d, int DP,
                             int64_t m_pad, int e, unsigned short* out, const float* valid,
                             hipStream_t s);
// The wide kernel's operands: the same codes, DP a multiple of 16 in (256,
// 1024], a row of DP / 8 16-byte chunks cut into fix16_wide_slab0's dim
// slabs.  Train (train order, n_pad a multiple of 32): 32-row tiles, within a
// tile slab after slab, each as 32 rows of the slab's chunks; dmax as above.
// Queries (m_pad a multiple of 32): step-major, the 8 codes of step c of query
// j of 32-query group g at uint4 index (g * DP / 8 + c) * 32 + j.
void launch_prep_u16_train_wide(const double* X64, const double* mu, int64_t n, int d, int DP,
                                int64_t n_pad, int e, unsigned short* out,
                                unsigned long long* dmax, hipStream_t s, const int* perm = nullptr);
void launch_prep_u16_queries_wide(const double* Q64, const double* mu, int64_t m, int d, int DP,
                                  int64_t m_pad, int e, unsigned short* out, const float* valid,
                                  hipStream_t s);
// gthr: the candidate kernel's per-query global thresholds ([m_pad][kGthrSlots] keys)
// or null when the kernel kept none
// failed queries are appended to rescan_q with rescan_tau = the W-th exact
// distance among their re-ranked rows (+inf if unknown)
// Proxies are in units 2^(2 t.jx) (L2) / 2^t.jx (L1).  valid[q] = 0: the
// query's operands left the format's range, its proxies are void (exact
// rescan).  ue / up: absolute error per operand element / per product in
// scaled units, for values outside the format's normal range.
// f16: the candidate pass ran on fp16 operands; the merge measures each
// query's representation error (rebuilding its operand's rounding) instead
// of assuming the format's worst case.
struct ProxyScale {
  const float* valid;
  double ue, up;
  bool f16 = false;
  // int8 pass: the per-dimension code centres (queries are coded
  // clamp(rint(q 2^s - cent), -128, 127); the merge measures the rounding)
  const double* i8c = nullptr;
  // queries in region order: query q's lists and thresholds sit at position
  // qpos[q] (null: at q)
  const int* qpos = nullptr;
  // int8 pass: the train image (rows of i8rb bytes, i8dp codes, chunks
  // swizzled when i8swz) -- the exact re-rank of a query on the train grid
  // reads it instead of the fp64 rows (merge_rerank_kernel, exact_sorted_i8)
  const signed char* i8x = nullptr;
  int i8rb = 0, i8dp = 0, i8swz = 0;
  // 16-bit fixed-point L1 pass (kernel metric 8; t.jx = the code scale e):
  // the largest coding error of a train row, max over rows of SUM_c |code -
  // 32768 - 2^e (x_c - mu_c)| in code units (< 0: another pass).  The merge
  // rebuilds the query's codes and measures its own sum.
  double u16dx = -1.0;
};
// Per-split certification (merge) and the targeted rescan: a query whose
// bound fails only through some splits' lists (a list holding R of its top
// W, its R-th entry inside the top W) rescans just those splits' rows.
struct SplitMap {
  int S = 0;                  // splits of the candidate launch (0: whole-set rescans only)
  int lps = 0;                // lists per query per split (4 quad, 2 otherwise)
  int64_t trows = 0;          // train rows per tile
  int cap = 0;                // failed queries the fast rescan serves
  unsigned long long* mask = nullptr;  // [m] splits each failed query rescans (~0: all rows)
  int* nkeep = nullptr;       // [cap] re-ranked rows of the other splits handed to the rescan
  int* keep = nullptr;        // [cap][kRescanCap] (the fast rescan's row buffer)
};
// The fast rescan's per-query setup, done by the merge for each query it
// fails (the first `cap`): the fp32 query operand of the rescan's X32 image
// (its centre mu, scale 2^jx, padded dim DP and norms x2max / x1max), the
// proxy threshold every row within tau passes (f_err: the fp32 error factor
// of DP) and the count of rows the merge already handed over (fcnt = nkeep).
struct RescanPrep {
  const double* mu = nullptr;
  double x2max = 0.0, x1max = 0.0, f_err = 0.0;
  float* qf = nullptr;   // [cap][DP]
  float* thr = nullptr;  // [cap]
  int* fcnt = nullptr;   // [cap]
  int jx = 0, DP = 0, cap = 0;
  // int8 pass with an unswizzled image (kernel metric 6): a failed query on
  // the train grid is filtered on the codes instead (rescan_filter_i8_kernel):
  // its codes [cap][256] and the largest exact integer squared distance
  // (code units) a row may have to reach tau; t8 < 0: the fp32 filter's
  // query (off the grid, tau unknown, or no int8 pass).  Null: none.
  signed char* qc8 = nullptr;
  long long* t8 = nullptr;
};
void launch_merge_rerank(int metric, const float* cv, const int* ci, int NL, int R,
                         const TrainDev& t, const double* Q64, int64_t m, int W, int C,
                         double f_err, ProxyScale ps, const uint32_t* gthr, const Sink& sink,
                         int* rescan_q, double* rescan_tau, int* rescan_cnt, const SplitMap& sm,
                         const RescanPrep& rp, hipStream_t s);
constexpr int kRescanCap = 1024;        // rows a fast rescan may append per query
constexpr int kRescanStageMaxDP = 256;  // fast rescan stages rows in LDS up to this DP
// Device-driven rescan (knn_select.hip): every buffer sized for `cap` fast-
// path queries (cap <= m); the merge fills q/tau and counts cnt[0].
struct RescanBufs {
  int* q;                    // [m] failed queries (merge)
  double* tau;               // [m] W-th exact distance among the re-ranked rows (+inf unknown)
  int* cnt;                  // [2] failed queries (merge) / passed on to the full scan
  float* qf;                 // [cap][DP] fp32 query operands of the fast path
  float* thr;                // [cap] proxy thresholds
  int* fcnt;                 // [cap] rows appended per query
  int* buf;                  // [cap][kRescanCap] appended rows
  int* slow_q;               // [m] queries for the full scan
  int* counts;               // host-mapped {cnt[0], full scans} of the call (nullable)
  unsigned long long* totals;  // device running sums of the same (nullable)
  const unsigned long long* mask;  // [m] splits to scan per failed query (null: all rows)
  const int* nkeep;          // [cap] rows the merge already put in buf (null: none)
  int S;                     // splits / tile rows of the candidate launch (mask bits)
  int64_t trows;
  int cus;                   // compute units (the staged filter's grid)
  // int8 filter (RescanPrep::qc8 / t8; null: every query on the fp32 filter):
  // the int8 image [n_pad][i8rb] bytes, codes of dims [0, i8dp) plain
  const signed char* qc8 = nullptr;
  const long long* t8 = nullptr;
  const signed char* i8img = nullptr;
  int i8rb = 0, i8dp = 0;
};
// Enqueues the rescan path (filter, exact finish, full scan; the merge did
// each fast-path query's setup, RescanPrep); every kernel reads the counts on
// the device.  f_err: the fp32 candidate
// error factor of t.DP; full_blocks: workgroups of the full-scan kernel.
void launch_rescan(int metric, const TrainDev& t, const double* Q64, const RescanBufs& rb, int cap,
                   int W, double f_err, const Sink& sink, int full_blocks, hipStream_t s);
// k-way merge + vote of [parts][m][w] sorted lists for queries [q0, q0+mq).
// Unions of up to 4096 entries sort in LDS; larger ones (any k <= n) rank
// each entry by binary searches and need merge_scratch_bytes() of device
// scratch (0 when the LDS kernel serves the geometry).
int64_t merge_scratch_bytes(int parts, int w, int k, int64_t mq);
// Reference tie order in the merge: mode as Sink::tie_mode; a query whose
// label can depend on the order among equal distances across shards gets
// kFlagTiePending and, when q is set, its output row appended to q (count in
// cnt[0]) for the train-sharded reference-order pass (launch_tie_resolve).
constexpr int kFlagTiePending = 64;  // KNN_FLAG_TIE_PENDING
struct MergeTies {
  int mode = 0;
  int* q = nullptr;
  int* cnt = nullptr;
};
void launch_merge_vote_partials(const double* dist, const int64_t* idx, const int32_t* lab,
                                int parts, int64_t m, int w, int k, int32_t* out_lab,
                                int64_t* out_idx, double* out_dist, int32_t* out_flags,
                                hipStream_t s, int64_t q0 = 0, int64_t mq = -1,
                                int64_t pstride = 0, void* scratch = nullptr,
                                const MergeTies& mt = MergeTies{});
// Train-sharded reference tie order (knn_select.hip): out[i][j] = the exact
// fp64 distance (reference operation order) of shard row j to query
// Q64[qsel[i]] (qsel null: row i), [nsel][t.n].
void launch_shard_dist(int metric, const TrainDev& t, const double* Q64, const int* qsel, int nsel,
                       double* out, hipStream_t s);
// Global row layout of the exchanged distance blocks: part p holds rows
// [off[p], off[p+1]) (parts <= kMaxParts).
constexpr int kMaxParts = 64;
struct PartRows {
  int parts;
  int64_t off[kMaxParts + 1];
};
// D = parts blocks [nsel][rows_p] at offsets nsel * off[p]; lab_all the labels
// of all off[parts] rows; outputs at sink rows orow[i] (labels, idx = global
// row, dist, flags: TIE_PENDING -> TIE_REF).  Scratch per workgroup:
// tie_scratch_bytes(off[parts], class_cnt); totals: running count (nullable).
void launch_tie_resolve(const double* D, const PartRows& pr, int nsel, const int32_t* lab_all,
                        const int* orow, int class_cnt, unsigned char* scratch, int64_t per_wg,
                        int nwg, const Sink& sink, unsigned long long* totals, hipStream_t s);
// byte stride of one part's packed [dist | idx | label] lists of m x w entries
inline int64_t packed_part_bytes(int64_t m, int w) { return (m * w * 20 + 15) / 16 * 16; }
// k beyond kMaxK (knn_select.hip, large_k_kernel): the exact path over every
// row, nwg workgroups with per_wg bytes of scratch each (large_k_scratch_bytes)
int64_t large_k_scratch_bytes(int64_t n, int W, int class_cnt);
void launch_large_k(int metric, const TrainDev& t, const double* Q64, int64_t m, int W,
                    int class_cnt, unsigned char* scratch, int64_t per_wg, int nwg,
                    const Sink& sink, hipStream_t s);
void launch_fill_i32(int32_t* p, int64_t n, int32_t v, hipStream_t s);
// int8 images (kernel metric 5, knn_prep.hip): train values x = (cent_i + k) /
// 2^s with integer codes k in [-128, 127].  grid_stats: per-dim min | max
// (out[2d]) and the largest fractional bit count (frac, atomicMax) of the
// train values; partial holds col_mean_blocks(n) x 2d doubles.
void launch_grid_stats(const double* X64, int64_t n, int d, double* partial, double* out,
                       unsigned* frac, hipStream_t s);
// swz: 16-B chunks at ch ^ xh_swz(row) (the 16x16x64 kernel's image); 0 for
// the 32x32x32 kernel's (its reads are conflict-free unswizzled)
void launch_prep_i8_train(const double* X64, const double* cent, int64_t n, int d, int DP,
                          int64_t n_pad, int s, signed char* out, unsigned* codes_max, int swz,
                          hipStream_t st, const int* perm = nullptr);
// qperm (query operand builders): operand row p <- query qperm[p] (null: p).
// The int8 builder also runs launch_query_check's test (mu, scale, jx, limit)
// into valid, with gthr set launch_fill_gthr's init of each row's slots, and
// clears zero[0, nzero) and zero4[0, 4) (when set).
void launch_prep_i8_queries(const double* Q64, const double* mu, double scale, int jx,
                            double limit, const double* cent, int64_t m, int d, int DP,
                            int64_t m_pad, int s, signed char* out, float* valid, hipStream_t st,
                            const int* qperm, uint32_t* gthr, int active, int* zero = nullptr,
                            int64_t nzero = 0, int* zero4 = nullptr, bool wide = false);
// wide (kernel metric 7 at DP > 256, knn_cand_sad_wide.hip): the same codes
// and validity test, the code rows step-major -- the 16 codes of step c of
// query j of 32-query group g at byte ((g DP / 16 + c) 32 + j) 16.
// The train side of that pass: plain rows of DP code bytes (zero codes in the
// pad dims and on pad rows), n_pad rows, no seeds
void launch_prep_i8_rows(const double* X64, const double* cent, int64_t n, int d, int DP,
                         int64_t n_pad, int s, signed char* out, hipStream_t st,
                         const int* perm = nullptr);
// The reference's exact neighbour order on exact distance ties (knn_select.hip,
// "reference tie order"): libstdc++ std::sort (introsort) emulated over all
// n exact distances of each listed query, restricted to the ranges that
// reach the first k positions.  Per workgroup scratch: tie_scratch_bytes.
constexpr int kFlagTieRef = 32;  // KNN_FLAG_TIE_REF: order resolved as the reference's
int64_t tie_scratch_bytes(int64_t n, int class_cnt);
// totals: device running count of the queries re-ordered (nullable)
// excl (nullable, [m] global indices): query q's std::sort runs over the n - 1
// records left when train row excl[q] is taken out (knn_loo.hip; a value
// outside [idx_off, idx_off + n) excludes nothing); null: exactly the pass
// without it
void launch_tie_order(int metric, const TrainDev& t, const double* Q64, const int* tie_q,
                      const int* tie_cnt, int class_cnt, unsigned char* scratch, int64_t per_wg,
                      int nwg, const Sink& sink, unsigned long long* totals, hipStream_t s,
                      const int64_t* excl = nullptr);
// The same pass under group exclusion (knn_lgo.hip; a kernel of its own):
// query q's std::sort runs over the records left, in row order, when every
// train row r with groups[r] == qgroup[q] is taken out (groups [n], local
// rows; a qgroup value that no row carries excludes nothing)
void launch_tie_order_group(int metric, const TrainDev& t, const double* Q64, const int* tie_q,
                            const int* tie_cnt, int class_cnt, unsigned char* scratch,
                            int64_t per_wg, int nwg, const Sink& sink, unsigned long long* totals,
                            hipStream_t s, const int32_t* qgroup, const int32_t* groups);
// K sweep under group exclusion (knn_lgo.hip): compacts the search's rows at
// k1 = kmax + gmax (in_dist / in_idx [m][k1], in_flags [m]) into [m][kmax] rows
// without the train rows of group qgroup[q] (groups [n]: the id of every local
// row, at most gmax rows per id) and the flags of a kmax search on the reduced
// set, as launch_loo_drop.
void launch_lgo_drop(const double* in_dist, const int64_t* in_idx, const int32_t* in_flags,
                     const int32_t* qgroup, const int32_t* groups, int64_t m, int kmax, int k1,
                     const int32_t* lab, int64_t idx_base, int64_t n, double* out_dist,
                     int64_t* out_idx, int32_t* out_flags, int cus, hipStream_t s);
// qgroup[i] = groups[row0 + i] (leave-one-group-out: query i is train row row0 + i)
void launch_lgo_self(int32_t* qgroup, const int32_t* groups, int64_t rows, int64_t row0,
                     hipStream_t s);
// group sizes into hist [n_groups] (zeroed by the caller), the first row whose
// id lies outside [0, n_groups) into *bad (preset to n by the caller) and the
// largest group's size into *gmax (zeroed by the caller)
void launch_lgo_group_stats(const int32_t* groups, int64_t n, int32_t n_groups, int32_t* hist,
                            unsigned long long* bad, int32_t* gmax, int cus, hipStream_t s);
// K-fold sweep on fold shards (knn_fold.hip).  rows [n]: the original train
// row of every row of the fold-major order (ascending inside a fold); the
// gather writes Xf [n][d] and labf [n] in that order
void launch_fold_gather(const double* X, const int32_t* lab, const int32_t* rows, int64_t n, int d,
                        double* Xf, int32_t* labf, int cus, hipStream_t s);
// a shard's list indices (local rows of fold g, -1 = padded slot) rewritten in
// place to base + rows_g[local]: original train rows, the lists still sorted
void launch_fold_map_idx(int64_t* idx, int64_t cnt, const int32_t* rows_g, int64_t n_g,
                         int64_t base, int cus, hipStream_t s);
// K sweep under exclusion (knn_loo.hip): compacts the search's rows at kmax + 1
// (in_dist / in_idx [m][kmax + 1], in_flags [m]) into [m][kmax] rows without
// train row excl[q] (global index; excl null or a value outside [idx_base,
// idx_base + n): nothing excluded) and the flags of a kmax search on the
// reduced set (TIE_BOUNDARY / TIE_VOTE / TIE_ORDER; EXACT_RESCAN / NONFINITE
// carried over).  lab[idx - idx_base]: the entries' labels; cus sizes the grid.
void launch_loo_drop(const double* in_dist, const int64_t* in_idx, const int32_t* in_flags,
                     const int64_t* excl, int64_t m, int kmax, const int32_t* lab,
                     int64_t idx_base, int64_t n, double* out_dist, int64_t* out_idx,
                     int32_t* out_flags, int cus, hipStream_t s);
// excl[i] = first + i (leave-one-out: query i is train row first + i)
void launch_loo_self(int64_t* excl, int64_t rows, int64_t first, hipStream_t s);
// K sweep (knn_sweep.hip): the reference's label at every K of a list from
// one ordered top-kmax row per query (kmax >= every K).  ks: device array of
// nk values in the caller's order (duplicates allowed); lab[idx - idx_base] is
// the label of a row entry (idx -1: an empty slot; a row starting with one has
// no neighbours and gets -1 at every K); cus sizes the grid.
// tie scan: appends to tie_q (count in tie_cnt[0]) the queries whose label at
// some K of the list the reference's order among equal distances could
// change (mode as Sink::tie_mode); dist / idx [m][kmax] in (dist, idx) order,
// flags [m] the search's flags for kmax (its KNN_FLAG_TIE_BOUNDARY bit).
void launch_sweep_tie_scan(const double* dist, const int64_t* idx, const int32_t* flags, int64_t m,
                           int kmax, const int32_t* lab, int64_t idx_base, const int* ks, int nk,
                           int mode, int* tie_q, int* tie_cnt, int cus, hipStream_t s);
// prefix votes: labels[j][q] (nk x m) = the vote over the first ks[j] entries
// of row q; with truth [m], correct[j] += #{q : labels[j][q] == truth[q]}
// (correct zeroed by the caller; one atomic per K per workgroup)
void launch_sweep_vote(const int64_t* idx, int64_t m, int kmax, const int32_t* lab,
                       int64_t idx_base, const int* ks, int nk, int32_t* labels,
                       const int32_t* truth, unsigned long long* correct, int cus, hipStream_t s);
// Per-class evaluation (knn_eval.hip).
// confusion: conf[i][t][p] (nk x C x C, 64-bit) += #{q : truth[q] == t and
// labels[i][q] == p} over labels [nk][m]; unl[i] += #{q : labels[i][q] or
// truth[q] outside [0, C)}.  Both ADD (zeroed by the caller) and each is
// nullable.  The histograms live in LDS by class_cnt: per-wave copies up to
// kEvalSmallC, one per workgroup up to kEvalLdsC, global atomics beyond
// (eval_confusion_regime: 0 / 1 / 2).
constexpr int kEvalSmallC = 16;
constexpr int kEvalLdsC = 96;
int eval_confusion_regime(int class_cnt);
void launch_eval_confusion(const int32_t* labels, int nk, int64_t m, const int32_t* truth,
                           int class_cnt, unsigned long long* conf, unsigned long long* unl,
                           hipStream_t s);
// vote counts: counts[q][c] (m x C, int32) = #{t < k : lab[idx[q][t] - idx_base]
// == c} over ordered rows idx [m][kmax] (k <= kmax; idx -1: an empty slot,
// counted nowhere).  Per-wave LDS counters up to kEvalCountsLdsC classes;
// beyond, the rows are zeroed on the stream and counted with global atomics.
constexpr int kEvalCountsLdsC = 1024;
hipError_t launch_eval_vote_counts(const int64_t* idx, int64_t m, int kmax, const int32_t* lab,
                                   int64_t idx_base, int k, int class_cnt, int32_t* counts,
                                   int cus, hipStream_t s);
// Distance-weighted voting (knn_wvote.hip; the rule: knn_amd.h,
// KNN_VOTE_DISTANCE).  Rows idx / dist [m][kmax] ascending by distance, label
// of an entry lab[idx - idx_base] (idx -1, an index below idx_base or a
// negative label: the entry does not vote).
// sweep: launch_sweep_vote's arguments plus dist; labels[j][q] = the weighted
// label over the first ks[j] entries, correct as there.  Dynamic LDS:
// wvote_sweep_lds_bytes (<= 64 KB for every kmax and nk <= 4096).
size_t wvote_sweep_lds_bytes(int kmax, int nk, bool with_truth);
void launch_wvote_sweep(const int64_t* idx, const double* dist, int64_t m, int kmax,
                        const int32_t* lab, int64_t idx_base, const int* ks, int nk,
                        int32_t* labels, const int32_t* truth, unsigned long long* correct, int cus,
                        hipStream_t s);
// sums: wsum[q][c] (m x C, fp64) = the class sums after the first k entries (k
// <= kmax), each class added up in row order; every cell is written
void launch_wvote_sums(const int64_t* idx, const double* dist, int64_t m, int kmax,
                       const int32_t* lab, int64_t idx_base, int k, int class_cnt, double* wsum,
                       int cus, hipStream_t s);
// fp64 rows -> [hi(DP) | lo(DP)] bf16 rows of scale*x (candidate metric 2 = L2 via bf16x3)
// rows of `out` are row_shorts 16-bit words; xl2/xl1 (train only, else null)
// fill the padded row's seed floats after the 2*DP bf16 payload
// fp16 images of kernel metric 4 (knn_prep.hip): train rows of DP halves + 4
// seed floats, scaled by 2^jx; query rows of DP halves of -2 * 2^jx (q - mu)
// (zero for queries launch_query_check marked invalid)
// dx2max: running max (u64 bits of a non-negative double) of the rows'
// ||fp16 / 2^jx - (x - mu)||_2^2 (measured representation error)
// swz: store the payload chunks swizzled (xh_swz, knn_device.h)
void launch_prep_half_train(const double* X64, const double* mu, int64_t n, int d, int DP,
                            int64_t n_pad, int jx, unsigned short* out, const float* xl2,
                            unsigned long long* dx2max, int swz, hipStream_t s,
                            const int* perm = nullptr);
// mu <- mu rounded to a multiple of 2^-g (the centre then sits on any data
// grid at least as coarse, so such data is exact in the fp16 operands)
void launch_round_mu(double* mu, int d, int g, hipStream_t s);
void launch_prep_half_queries(const double* Q64, const double* mu, int64_t m, int d, int DP,
                              int64_t m_pad, int jx, unsigned short* out, const float* valid,
                              hipStream_t s, const int* qperm = nullptr);
void launch_prep_split(const double* X64, const double* mu, int64_t n, int d, int DP,
                       int64_t n_pad, double scale, unsigned short* out, int row_shorts,
                       const float* xl2, const float* xl1, hipStream_t s, const int* perm = nullptr);

// Region order (knn_order.hip).  Features are the fp32 operands 2^jx (x - mu).
// out[r] = rank[nearest centroid of row r * stride] (rank null: the centroid)
// Assignment on bf16 MFMA against a centroid image (launch_region_kmeans):
// out[r] = rank[nearest centroid of row r * stride] (rank null: the centroid);
// bcnt (nullable, zeroed): per-1024-row-block key counts
constexpr int kRegionImgBytes = 2 * 16 * 32 * 16 * 2;  // centroid image at d <= 256
void launch_region_assign(const double* X, const double* mu, int64_t n, int d, int64_t stride,
                          int jx, const unsigned short* img, const float* cnorm, const int* rank, int* out,
                          int* bcnt, hipStream_t s);
// k-means over ns sample rows (row i = X row i * stride): cent [P][d], img /
// cnorm the final centroids' bf16 image (kRegionImgBytes) and squared norms
// [kRegionMax], assign [ns] scratch, rank [P] = each centroid's place in the
// greedy chain
void launch_region_kmeans(const double* X, const double* mu, int64_t ns, int d, int64_t stride,
                          int jx, int P, int iters, float* cent, unsigned short* img, float* cnorm,
                          int* assign, int* rank, hipStream_t s);
// Stable counting sort of n keys in [0, kRegionMax): bcnt holds
// region_sort_blocks(n) x kRegionMax ints, tot kRegionMax; outputs (nullable)
// perm[pos] = i, ipos[i] = pos, qstart[pos] = rstart[key] (phases > 0: of
// the first key of the key's group, P keys in `phases` groups), bases[k] =
// the first position of key k
int64_t region_sort_blocks(int64_t n);
void launch_region_sort(const int* key, int64_t n, int* bcnt, int* tot, int* perm, int* ipos,
                        const int* rstart, int* qstart, int* bases, hipStream_t s, int P = 1,
                        int phases = 0);
// Per call: queries assigned to regions and counting-sorted (qperm / qpos /
// qstart as above); bcnt region_sort_blocks(m) x kRegionMax ints, cleared
// first unless bcnt_zero (already zero)
void launch_region_sort_queries(const double* Q, const double* mu, int64_t m, int d, int jx,
                                const unsigned short* img, const float* cnorm, int P, const int* rank,
                                const int* rstart, int phases, int* bcnt, int* tot, int* qkey,
                                int* qperm, int* qpos, int* qstart, hipStream_t s,
                                bool bcnt_zero = false);

// Norm blocks (knn_order.hip): every window of kNormWin image positions
// sorted by the rows' squared norm (int8 code norm with cent, else ||x -
// mu||^2): perm[p] = perm0[source] (perm0 null: train order), ipos inverse;
// key holds n uint32 of scratch.  perm0 must not alias perm / ipos.  il: the
// int8 kernel metric (5 / 6) whose lane lists the norm ranks of each 32-row
// sub-tile are interleaved over (0: sorted order).
void launch_norm_blocks(const double* X, const double* cent, int s, const double* mu, int64_t n,
                        int d, const int* perm0, uint32_t* key, int* perm, int* ipos, int il,
                        hipStream_t st);
// Int8 images carry, in the pad of row 128u + 1, the largest seed of each of
// the 32-row sub-tiles 4u .. 4u+3 (the seed-free accumulation's bound,
// knn_cand_res.hip)
constexpr int kI8SmaxRow = 1;
// ... and in the pad of row 128u + 2 the largest PARTIAL seed -ceil(||k_A||^2
// / 2) over the first i8_part_dims(DP) dims of the same sub-tiles: the
// metric-6 kernel's early prune after those dims' MFMAs (knn_cand_res.hip,
// KNN_I8_PART).  0 dims: no partial test (the pads get 0, a valid bound).
// Only for 128 <= DP <= 192: at DP = 96 the test after 64 of 96 dims prunes
// too little to pay for its tree (the 12.5M x 96 shard +21 %, ab_log r6r).
constexpr int kI8SmaxARow = 2;
constexpr int i8_part_dims(int DP) { return DP >= 128 && DP <= 192 ? DP - 32 : 0; }

// Min-max normalisation (knn_normalize.hip, cpp:229-306).  R = rows per
// grid sweep; `partial` holds 2*d*R doubles.  launch_minmax folds the set's
// per-dim max/min into out_max/out_min (init: start from -1 / 999999).
int64_t minmax_rows_per_sweep(int64_t rows, int d, int cu_count);
void launch_minmax(const double* X, int64_t rows, int d, int64_t R, double* partial,
                   double* out_max, double* out_min, int init, hipStream_t s);
void launch_normalize_apply(double* X, int64_t rows, int d, int64_t R, const double* vmax,
                            const double* vmin, hipStream_t s);

// ---- CSV text -> fp64 rows / int32 labels (knn_csv.hip; the reference's
// reader, cpp:154-222).  csv_block_count: workgroups of a file of `bytes` > 0
// bytes = entries of cnt (uint32) and base (int64).  count + scan: terminators
// per block, their exclusive scan and the file's token count (*tokens).
// convert: every token c < cap converted (knn_csv_num.h) and stored by the
// reference's rule, or appended as (c, terminator position) to slow [slow_cap]
// [2] through the counter *nslow (zeroed by the caller; counts past slow_cap).
// scatter: ent [n][2] = (c, fp64 bits or int32 label) written by the same rule.
// text must be 16-byte aligned.
int64_t csv_block_count(int64_t bytes);
void launch_csv_count_scan(const char* text, int64_t bytes, unsigned int* cnt, int64_t* base,
                           int64_t* tokens, hipStream_t s);
void launch_csv_convert(const char* text, int64_t bytes, const int64_t* base,
                        const knncsv::NumTable* tab, int dim, bool with_label, int64_t cap,
                        double* data, int32_t* labels, int64_t* slow, int64_t slow_cap,
                        int64_t* nslow, hipStream_t s);
void launch_csv_scatter(const int64_t* ent, int64_t n, int dim, bool with_label, int64_t cap,
                        double* data, int32_t* labels, hipStream_t s);

}  // namespace knnk
