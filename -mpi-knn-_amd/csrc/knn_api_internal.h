// knn_api_internal.h -- context state shared by knn_api.cpp and knn_group.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "knn_kernels.h"
#include "knn_plan.h"

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes);  // grow-only; KNN_OK or KNN_ERR_NOMEM
  void release();
};

// Per-call timing record (ring): events around the phases of one classify /
// search call, read back lazily so a call never waits for the device.
constexpr int kTimingRing = 32;
struct TimedCall {
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  bool pending = false;
  int mode = 1;  // knn_set_timing: 1 every phase, 2 the candidate kernel only (ev[1], ev[2])
};

struct knn_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int* h_counts = nullptr;  // pinned, device-mapped: {failed queries, full scans} of the last call
  int* d_counts = nullptr;  // device alias of h_counts
  unsigned long long h_stats[6] = {0, 0, 0, 0, 0, 0};  // train statistics read back at build
  bool trained = false;
  int class_cnt = 0;
  int64_t idx_off = 0;
  int cu_count = 0;
  int precision = 0;     // KNN_PRECISION_*
  int vote = 0;          // KNN_VOTE_* (knn_set_vote)
  int DPb = 0;           // padded dim of the bf16x3 copy (0 = not built)
  int DPh = 0;           // padded dim of the fp16 copy (0 = not built)
  int xh_swz = 0;        // the fp16 copy's chunks are swizzled (xh_swz)
  int DPs = 0;           // padded dim of the fp16 S3 image (0 = not built)
  double xamax = 0.0;    // max |x_i - mu_i| over the train set
  // int8 candidate pass (kernel metric 5): the train values are integer codes
  // x = (cent_i + k) / 2^i8_s, k in [-128, 127] (i8_ok, set at set_train)
  bool i8_ok = false;
  int i8_s = 0;
  int DPi = 0;           // padded dim of the int8 image (0 = not built)
  int i8_swz = 1;        // the int8 image's chunks are swizzled (16x16x64 kernel; 0: 32x32x32)
  double i8_x2max = 0.0; // max ||k||^2 / 2^(2 s) of the image
  bool i8_off = false;   // AUTO: int8 pass retired for this train set
  int auto_kind = 0;     // the pass the pending AUTO decision is about (4 fp16, 5 int8)
  bool fp16_off = false; // AUTO: fp16 candidate pass retired for this train set
                         // (a batch certified too few queries, see knn_run_search)
  // the last call, for the deferred AUTO decision: its completion event,
  // query count and whether it ran the fp16 pass (decided once it completed)
  hipEvent_t done_ev = nullptr;
  bool auto_pending = false;
  int64_t auto_m = 0;
  knnk::Tuning tune;     // knn_set_tuning (knn_plan.h)
  int ord_P = 0;         // regions of the current train layout (0: train order)
  bool ord_nb = false;   // the current layout has norm blocks (ord_perm / ord_ipos valid)
  // ints of ord_bcnt known to be zero (the int8 query builder clears the
  // region sort's block counts after the sort read them; 0: unknown)
  int64_t ord_bcnt_zero = 0;
  // sample image of the seeding pre-pass (strided train rows in the image
  // format of kernel metric smp_kind at width smp_dp; 0 = not built)
  int smp_kind = 0, smp_dp = 0, smp_swz = -1;
  int64_t smp_n = 0;
  int last_nw = 0;
  int last_kmetric = -1; // candidate kernel metric of the last search (knn_kernels.h)
  char last_kernel[96] = {0};  // name of the last candidate kernel launched
  knnk::TrainDev train{};
  int timing = 0;  // knn_set_timing mode
  TimedCall ring[kTimingRing];
  int ring_next = 0, ring_last = -1;
  double tsum[4] = {0, 0, 0, 0};
  int64_t tcalls = 0;
  int64_t geom[4] = {0, 0, 0, 0};
  // train-side HBM
  DevBuf X64_own, lab_own, X32, xl2, xl1, stats, XB, XS, XH, XT16, XS16, mu, mu_part;
  // int8 image: codes [n_pad][DP + 16 B]; per-dim centres [code units d |
  // value units d] (the latter the merge's mu for this pass); grid stats scratch
  DevBuf XI, i8_cent, i8_gs;
  // the wide L1-on-codes pass's own image (256 < d <= 1024): plain rows of
  // DPiw code bytes, n_pad rows (0 = not built)
  DevBuf XIW;
  int DPiw = 0;
  // the 16-bit fixed-point L1 pass's image (kernel metric 8): rows of DPu
  // unsigned short codes at scale 2^u16_e, n_pad rows (0 = not built), and
  // the largest coding error of a row in code units (ProxyScale::u16dx)
  DevBuf XU;
  int DPu = 0, u16_e = 0;
  double u16_dx = 0.0;
  // its wide form's own image (256 < d <= 1024): 32-row tiles of dim slabs,
  // DPuw codes per row, n_pad rows (0 = not built); u16_e and u16_dx as above
  DevBuf XUW;
  int DPuw = 0;
  DevBuf smp_x64, smp_xl2, smp_img, smp_scr, smp_v, smp_i;
  // region order: centroids [P][d], chain ranks, region starts, image
  // position <-> train row maps; k-means / sort scratch; per-call query order
  DevBuf ord_cent, ord_cnorm, ord_img, ord_rank, ord_rstart, ord_perm, ord_ipos, ord_key, ord_bcnt, ord_tot, ord_qkey,
      ord_qperm, ord_qpos, ord_qstart, ord_perm0;
  // per-classify workspace
  DevBuf Q64, Q32, qvalid, cand_v, cand_i, gthr, rescan_q, rescan_tau, rescan_cnt, fr_cnt, fr_buf,
      fr_q, fr_thr, slow_q, totals, lk, rescan_mask, rescan_nkeep, rescan_qc8, rescan_t8;
  // train-sharded merge of unions beyond 4096 entries (rank merge scratch)
  DevBuf mrg;
  // reference tie order pass: queued queries, per-workgroup scratch
  DevBuf tie_q, tie_ws;
  // K sweep: the list of K, the search's label / idx / dist / flags at kmax,
  // host-API staging of labels [nk][m], truth [m] and correct counts [nk]
  DevBuf sw_ks, sw_lab, sw_idx, sw_dist, sw_flags, sw_out, sw_truth, sw_corr;
  // K sweep under exclusion: the search's rows / flags at kmax + 1, the
  // exclusions of a leave-one-out batch (and the host twin's staging)
  DevBuf loo_idx, loo_dist, loo_flags, loo_excl;
  // K sweep under group exclusion (knn_set_groups): the train rows' group ids
  // (own copy or the caller's device array; null = none set), their count and
  // the largest group's size; the host variant's copy, the histogram and
  // {first bad row, gmax} of the check, the groups of a leave-group-out batch
  const int32_t* groups = nullptr;
  int32_t n_groups = 0, gmax = 0;
  DevBuf grp_own, grp_hist, grp_stat, lgo_qg;
  // K-fold sweep on fold shards (knn_set_folds): the fold count and the largest
  // fold's size (0 = none set), the folds' first rows in the fold-major order
  // [n_folds + 1], that order's original train rows (rows_of, host copy), one
  // sub-context per fold over its slice of the fold-major fp64 copy; on the
  // device: the fold ids, rows_of, the copy and its labels, the packed partial
  // lists [F - 1][m][w] of a batch, its queries' fold, its tie queue | count
  int32_t n_folds = 0, fold_max = 0;
  std::vector<int64_t> fold_off;
  std::vector<int32_t> fold_rows;
  std::vector<knn_ctx*> fold_ctx;
  DevBuf fold_ids, fold_rowsd, fold_X, fold_lab, fold_pk, fold_qg, fold_tq;
  // per-class evaluation: the sweep's labels [nk][m] when the caller wants
  // none, host-API staging of conf [nk][C][C] and unl [nk]
  DevBuf ev_lab, ev_conf, ev_unl;
  // host-API outputs
  DevBuf o_lab, o_idx, o_dist, o_flags;
  // normalisation: per-thread partial max/min, bounds, host-API staging
  DevBuf nrm_part, nrm_mm, nrm_X;
  // CSV reader: the conversion table (uploaded once), block counts and bases,
  // and the file entry points' staging: text, values, labels, slow list,
  // {tokens, slow count}, the host's (index, value) list
  DevBuf csv_tab, csv_ws, csv_text, csv_data, csv_lab, csv_slow, csv_misc, csv_fix;
  bool csv_tab_ready = false;
  int64_t csv_last_slow = -1;                  // slow tokens of the last file call
  double csv_phase_s[5] = {0, 0, 0, 0, 0};     // its read / h2d / parse / d2h / slow seconds
  std::vector<DevBuf*> all_bufs() {
    return {&X64_own, &lab_own, &X32,   &xl2,   &xl1,    &stats,  &XB,       &XS, &XI, &XIW, &XU, &XUW, &i8_cent, &i8_gs,
            &XH,      &XT16,    &XS16,  &mu,      &mu_part, &Q64, &Q32,    &qvalid, &cand_v,   &cand_i,
            &gthr,    &rescan_q, &rescan_tau, &rescan_cnt, &fr_cnt, &fr_buf, &fr_q, &fr_thr,
            &slow_q,  &totals,  &lk, &mrg, &tie_q, &tie_ws, &o_lab, &o_idx, &o_dist, &o_flags, &nrm_part, &nrm_mm, &nrm_X,
            &rescan_mask, &rescan_nkeep, &rescan_qc8, &rescan_t8, &smp_x64, &smp_xl2, &smp_img, &smp_scr, &smp_v, &smp_i,
            &ord_cent, &ord_cnorm, &ord_img, &ord_rank, &ord_rstart, &ord_perm, &ord_ipos, &ord_key, &ord_bcnt, &ord_tot,
            &ord_qkey, &ord_qperm, &ord_qpos, &ord_qstart, &ord_perm0, &sw_ks, &sw_lab, &sw_idx, &sw_dist, &sw_flags,
            &sw_out, &sw_truth, &sw_corr, &loo_idx, &loo_dist, &loo_flags, &loo_excl,
            &grp_own, &grp_hist, &grp_stat, &lgo_qg,
            &fold_ids, &fold_rowsd, &fold_X, &fold_lab, &fold_pk, &fold_qg, &fold_tq,
            &ev_lab, &ev_conf, &ev_unl, &csv_tab, &csv_ws, &csv_text, &csv_data, &csv_lab, &csv_slow,
            &csv_misc, &csv_fix};
  }
};

int knn_fail(int code, const std::string& msg);
// K sweep argument check shared with knn_group.cpp: 1 <= nk <= 4096 and 0 <=
// ks[i] <= n (KNN_ERR_ARG naming the offending entry); *kmax = max K
int knn_sweep_check_ks(const int32_t* ks, int32_t nk, int64_t n, int32_t* kmax);
// K sweep of train rows [row0, row0 + rows) against the train set without the
// row itself (own_group false: leave-one-out, the body of knn_loo_sweep_device
// and knn_loo_sweep_eval_device) or without the row's whole group (own_group:
// leave-group-out, knn_lgo_sweep_device's body), on stream s.  Every output is
// nullable: without d_labels the labels stay in the context's workspace, d_conf
// / d_unl ask for the per-class evaluation against the rows' own labels.  zero
// = false ADDS into d_conf / d_unl, so the callers that walk the train set in
// batches sum them on the device.
int knn_sweep_rows(knn_ctx* ctx, int64_t row0, int64_t rows, bool own_group, const int32_t* ks,
                   int32_t nk, int32_t metric, int32_t* d_labels, int64_t* d_correct,
                   int64_t* d_idx, double* d_dist, int32_t* d_flags, int64_t* d_conf,
                   int64_t* d_unl, bool zero, hipStream_t s);
// K-fold sweep (knn_kfold_sweep's body, shared with knn_group.cpp): folds fold0,
// fold0 + step, ... of the context's folds, each in batches of at most 16384 of
// its rows; the outputs are host arrays in train row order of which only the
// walked folds' rows are written, out_correct / out_conf / out_unl receive the
// walk's own sums.  Every output is nullable; waits for the result.
int knn_kfold_walk(knn_ctx* ctx, int fold0, int step, const int32_t* ks, int32_t nk,
                   int32_t metric, int32_t* out_labels, int64_t* out_correct, int64_t* out_conf,
                   int64_t* out_unl, int64_t* out_idx, double* out_dist, int32_t* out_flags);
int knn_run_search(knn_ctx* ctx, const double* dQ, int64_t m, int W, int metric,
                   const knnk::Sink& sink, hipStream_t s);
