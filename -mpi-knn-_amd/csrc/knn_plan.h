// knn_plan.h -- every decision of a search, made on the host before anything
// is allocated or launched: candidate path, workgroup shape, list geometry,
// thresholds.  Plain C++17 with no HIP types: tools/plan_check.cpp walks
// plan_search over a grid of inputs on a CPU.
#pragma once
#include <stdint.h>

#include "knn_dims.h"

namespace knnk {

// Tuning keys (knn_set_tuning); the defaults are the production behaviour.
struct Tuning {
  int R = 0, S = 0;      // 0 = automatic
  int ablate = 0;        // timing-only kernel ablations
  int nw = 0;            // resident kernel waves per workgroup (0 = auto)
  int s3q = -1;          // fp16 S3 on the 16x16x32 layout: -1 auto, 0 off, 1 on
  int qres = -1;         // query-resident fp16 kernel for d > 256 (knn_cand_qres.hip): -1 auto, 0 off
  int gk = -1;           // what the lists publish into gthr (-1 auto, 0 list R-th, 1..16)
  int xhswz = 1;         // fp16 train image chunk swizzle (xh_swz): 1 on, 0 off (A/B)
  int fp16 = -1;         // fp16 candidate pass: -1 auto, 0 off, 1 on
  int i8 = -1;           // int8 candidate pass: -1 auto, 0 off, 1 on (where the data allow)
  int i8w = -1;          // int8 on 32x32x32 (metric 6): -1 auto (where it pads less), 0 off, 1 on
  // L1 on int8 codes (metric 7): -1 auto, 0 off, 1 on (where the data allow),
  // 2 as 1 and also at 256 < d <= 1024 (knn_cand_sad_wide.hip)
  int i8l1 = -1;
  // L1 on 16-bit fixed-point codes of any train set at d <= 256 (metric 8,
  // knn_cand_fix16.hip): 0 off, 1 on at every batch size.  Opt-in: no auto.
  int u16l1 = 0;
  // the same pass at 256 < d <= 1024 (knn_cand_fix16_wide.hip): 0 off, 1 on at
  // every batch size.  Opt-in: no auto; "u16l1" moves no call above 256 dims.
  int u16l1w = 0;
  int ties = 1;          // reference tie order: 0 off, 1 vote-affecting ties, 2 all ties
  int m16 = -1;          // bf16x3 on the 16x16x32 MFMA layout: -1 auto, 0 off, 1 on
  int64_t seed = 0;      // seeded thresholds: 0 / -1 off, N sample rows (experiment)
  // region order (knn_order.hip): -1 auto, 0 off, 1 on, N >= 2 that many
  // regions.  The train layout is decided at set_train; a train set laid out
  // by region still serves calls with 0 (queries in call order, streams
  // starting at each split's first tile).
  int order = -1;
  // norm blocks (knn_order.hip): -1 auto (integer-coded train sets, d <= 256),
  // 0 off, 1 on
  int nblk = -1;
  int gg = -1;           // gthr slot groups of the resident kernel: -1 auto, 4 or 8
  int i8resc = -1;       // int8 rescan filter (metric 6): -1 auto (on), 0 off
  int qblk = 0;          // resident kernel workgroup order: 0 split-major, B query blocks
  int s3gq = 0;          // S3 kernel: largest XCD query-tile grouping (0 = kS3GqMax)
  // query streams start at one of N phases of the region chain (P regions in
  // N groups; -1 auto = 8, 0 = at the query tile's own region)
  int ophase = -1;
};
// KNN_OK, or KNN_ERR_ARG with *err = the message (unknown key: *err = null)
int set_tuning(Tuning& t, const char* key, int64_t value, const char** err);

// What only the built kernels know (knn_cand*.hip).  Plain function
// pointers: the plan runs on the host path of every call.
struct KernelFacts {
  int (*cand_blocks_per_cu)(int metric, int DP, int R, int nw);  // resident workgroups per CU
  int (*s3q_blocks_per_cu)();
  int (*cand_queries_per_wave)(int metric, int DP);  // resident kernel: queries per wave
  int (*cand_tile_rows)(int metric, int DP);         // train rows per tile
  bool (*qres_supported)(int DP);
};

// Everything a decision reads.
struct PlanIn {
  int64_t n, n_pad;  // train rows, padded rows of the fp32 image
  int d, DP;         // dimension, padded dim of the fp32 image (pad_dim)
  int metric;        // KNN_METRIC_*
  int64_t m;         // queries
  int W;             // list length asked of the search
  int precision;     // KNN_PRECISION_*
  bool fp16_off, i8_off;  // AUTO retired the pass for this train set
  bool i8_ok;        // the train set is integer-coded
  int ord_P;         // regions of the train layout (0: train order)
  bool ord_nb;       // the train layout has norm blocks
  int cu_count;
  bool timed;        // the call records timing events
  const Tuning& tune;
  const KernelFacts& facts;
};

// the train image the candidate kernel reads (knn_api.cpp: ensure_*)
// (IMG_I8W: the plain int8 rows of the wide L1-on-codes pass, d > 256;
// IMG_U16: the 16-bit fixed-point rows of kernel metric 8; IMG_U16W: its
// wide form's tiles of dim slabs, d > 256)
enum TrainImage { IMG_FP32, IMG_BF16X3, IMG_FP16, IMG_FP16_S3, IMG_I8, IMG_I8W, IMG_U16, IMG_U16W };

struct SearchPlan {
  bool ok;           // false: no kernel is instantiated for this geometry
  int kmetric;       // kernel metric (knn_kernels.h, CandLaunch)
  TrainImage image;
  int DP;            // padded dim of that image
  bool s3, s3h, s3q, qres;  // S3 stream kernel; its fp16 form; on 16x16x32; query-resident
  int nw, qpw, qpb, n_qt;   // waves and queries per workgroup, query tiles
  int64_t m_pad, trows, n_tiles, n_pad3;
  int C, S, R, lps, NL;     // union size, splits, list length, lists per split, lists
  int G, gk, active, gmask, qblk;
  bool use_gthr, gthr_init;
  bool query_order;  // queries sorted by region
  int ophase;
  bool i8resc;       // the int8 rescan filter
  int i8_swz, xsw;   // the int8 image's / the launched kernel's image's chunk swizzle
  int64_t seed_rows; // sample rows of the seeding pre-pass (0: none)
  int s3gq, ablate, cap;
  bool abl;          // a timing-only ablation leaves every query uncertified
  bool ev_ext;       // the kernel's own dispatch records the "cand" events
  bool auto_arm;     // the call arms the deferred AUTO decision
  char kernel[96];   // the kernel's printed name
};
SearchPlan plan_search(const PlanIn& in);

int i8_kernel_d(const Tuning& tune, int d);
int region_count(const Tuning& tune, bool i8_ok, int64_t n, int d);
bool norm_blocks_on(const Tuning& tune, bool i8_ok, int64_t n, int d);
double err_factor(int kmetric, int DP);

}  // namespace knnk
